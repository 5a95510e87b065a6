"""Flax-layout view of the agent's parameter arena (what `server.publish_network(agent.state.params)`
and flax checkpoints expect; examples/async_drq_sim/async_drq_sim.py:104-108,229,295-307).

Tree derived from flax naming rules at the reference's construction sites
(agents/continuous/drq.py:165-222, common/common.py:58-78, vision/resnet_v1.py): modules passed as attributes are
named by attachment (`modules_actor`, `network`, `encoder_<key>`), a module instance shared by several owners
(the EncodingWrapper of actor and critic, the frozen `pretrained_encoder` of all cameras) is adopted once -- the
evidence is the reference's own loader, which patches `modules_actor` only and guards
`if "pretrained_encoder" in new_encoder_params` (utils/train_utils.py:118-127).  tests/test_reference_update.py checks
these paths against the tree the reference's own code builds under the flax stand-in (oracle/jaxshim); no real flax
install is available, so the alias switches below remain for the alternative readings.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict

import numpy as np

from ..utils.init import STAGES, NetSpec, theta_shapes, trunk_shapes


# optax.adam's state (optax/_src/transform.py ScaleByAdamState; base.EmptyState of scale_by_learning_rate)
ScaleByAdamState = namedtuple("ScaleByAdamState", ["count", "mu", "nu"])
EmptyState = namedtuple("EmptyState", [])

# per-camera encoder head on the frozen trunk: leaf below enc/<i>/ -> path below encoder_<key>
CAM_PATHS = {"sle": ("SpatialLearnedEmbeddings_0", "kernel"), "dense/kernel": ("Dense_0", "kernel"),
             "dense/bias": ("Dense_0", "bias"), "ln/scale": ("LayerNorm_0", "scale"), "ln/bias": ("LayerNorm_0", "bias")}


def adam_moments(opt):
    """(mu, nu) of optax.adam's state, given as the (ScaleByAdamState, EmptyState) tuple or in its state-dict form
    {"0": {"count", "mu", "nu"}, "1": {}}."""
    adam = opt[0] if isinstance(opt, (tuple, list)) else opt["0"]
    return (adam.mu, adam.nu) if hasattr(adam, "mu") else (adam["mu"], adam["nu"])


class AdamTrainState:
    """TrainState fields of a handle trained by ONE optax.adam over its whole parameter tree (BC, the trainable reward
    classifier): the optax tuple (ScaleByAdamState(count, mu, nu), EmptyState()) -- the moments of a frozen leaf are
    exact zeros --, flax's state-dict form and `replace`.  `fields` are the TrainState's fields in flax's order and
    `opt_field` the one that holds the optax tuple; the class provides `step`, `params` (and `rng` when it is a field),
    `_export(section)` / `_import(tree, section)` of the trees "params", "opt/mu", "opt/nu" and `_set_step(step)`."""

    fields = ("step", "params", "opt_state")
    opt_field = "opt_state"
    replace_error = NotImplementedError

    def adam_state(self):
        return (ScaleByAdamState(np.int32(self.step), self._export("opt/mu"), self._export("opt/nu")), EmptyState())

    def state_dict(self) -> dict:
        """flax.serialization.to_state_dict form (what flax checkpoints store): tuples become {'0', '1', ...} and
        NamedTuples dicts of their fields; target_params, where it is a field, equals params."""
        adam, _ = self.adam_state()
        params = self.params
        sd = {"step": np.int32(self.step), "params": params, "target_params": params,
              self.opt_field: {"0": {"count": adam.count, "mu": adam.mu, "nu": adam.nu}, "1": {}}}
        if "rng" in self.fields:
            sd["rng"] = self.rng
        return {f: sd[f] for f in self.fields}

    def load_state_dict(self, sd: dict):
        if sd.get("params") is not None:
            self._import(sd["params"], "params")
        opt = sd.get(self.opt_field)
        if opt is not None:
            mu, nu = adam_moments(opt)
            self._import(mu, "opt/mu")
            self._import(nu, "opt/nu")
        if sd.get("step") is not None:
            self._set_step(int(np.asarray(sd["step"])))
        return self

    def replace(self, **kw):
        bad = set(kw) - set(self.fields)
        if bad:
            raise self.replace_error(f"unknown TrainState fields: {sorted(bad)}")
        self.load_state_dict(kw)
        return self


def _aliases(path):
    """the paths of one leaf: theta_paths lists aliases, the other tables give one path"""
    return path if isinstance(path, list) else [path]


def tree_from_leaves(paths, shapes, get) -> Dict:
    """{leaf: path} table -> nested dict holding get(leaf).reshape(shapes[leaf]) at the leaf's path (one array at
    every alias)."""
    tree: Dict = {}
    for leaf, path in paths.items():
        v = get(leaf).reshape(shapes[leaf])
        for p in _aliases(path):
            d = tree
            for k in p[:-1]:
                d = d.setdefault(k, {})
            d[p[-1]] = v
    return tree


def leaves_from_tree(paths, tree):
    """{leaf: path} table, nested dict -> (leaf, the value at its (first) path)"""
    for leaf, path in paths.items():
        d = tree
        for k in _aliases(path)[0]:
            d = d[k]
        yield leaf, d


def _trunk_paths():
    """flat trunk leaf -> path below `pretrained_encoder`."""
    m = {"trunk/conv_init": ("conv_init", "kernel"), "trunk/norm_init/scale": ("norm_init", "scale"),
         "trunk/norm_init/bias": ("norm_init", "bias")}
    cin = 64
    for i, (f, s) in enumerate(STAGES):
        p, b = f"trunk/block{i}/", f"ResNetBlock_{i}"
        m[p + "conv0"] = (b, "Conv_0", "kernel")
        m[p + "gn0/scale"] = (b, "MyGroupNorm_0", "scale")
        m[p + "gn0/bias"] = (b, "MyGroupNorm_0", "bias")
        m[p + "conv1"] = (b, "Conv_1", "kernel")
        m[p + "gn1/scale"] = (b, "MyGroupNorm_1", "scale")
        m[p + "gn1/bias"] = (b, "MyGroupNorm_1", "bias")
        if s != 1 or cin != f:
            m[p + "proj"] = (b, "conv_proj", "kernel")
            m[p + "gnp/scale"] = (b, "norm_proj", "scale")
            m[p + "gnp/bias"] = (b, "norm_proj", "bias")
        cin = f
    return m


def _policy_std_paths(std_parameterization):
    """the leaves behind the policy's mean head: Dense_1, or Policy's own `log_stds` parameter with "uniform"
    (actor_critic_nets.py:199-201: self.param("log_stds", zeros, (action_dim,))); nothing with "fixed" (:190-192: fixed_std is a
    constant of the module, modules_actor holds the encoder, the MLP and Dense_0 alone)"""
    if std_parameterization == "fixed":
        return {}
    if std_parameterization == "uniform":
        return {"actor/log_stds": [("modules_actor", "log_stds")]}
    return {"actor/logstd/kernel": [("modules_actor", "Dense_1", "kernel")], "actor/logstd/bias": [("modules_actor", "Dense_1", "bias")]}


def net_spec_of(core) -> NetSpec:
    """the network options of an AgentCore, as far as the leaf tables depend on them (NetSpec.leaf_kwargs); an attribute the handle
    does not have is the default's: a core that only has cfg.hidden is the (hidden, hidden), LayerNorm, "exp" agent"""
    names = ("std_parameterization", "critic_dims", "policy_dims", "critic_layer_norm", "policy_layer_norm")
    kw = {n: getattr(core, n) for n in names if hasattr(core, n)}
    if getattr(core, "_h", None) is not None and hasattr(core, "L"):      # whether the library's agent has its proprio branch
        kw["use_proprio"] = int(core.L.serl_agent_use_proprio(core._h)) != 0
    elif hasattr(core, "use_proprio"):
        kw["use_proprio"] = bool(core.use_proprio)
    return NetSpec(hidden=int(getattr(core.cfg, "hidden", 256)), **kw)


def _mlp_paths(m, pre, base, n_layers, layer_norm=True):
    """layer j = 1..n of MLP `pre` -> Dense_{j-1} / LayerNorm_{j-1} below `base` (mlp.py:19-31 names them in loop order); with
    use_layer_norm=False (mlp.py:29-30) no LayerNorm module is made and the tree holds none"""
    for j in range(1, n_layers + 1):
        m[f"{pre}/w{j}"] = [base + (f"Dense_{j - 1}", "kernel")]
        m[f"{pre}/b{j}"] = [base + (f"Dense_{j - 1}", "bias")]
        if layer_norm:
            m[f"{pre}/ln{j}/scale"] = [base + (f"LayerNorm_{j - 1}", "scale")]
            m[f"{pre}/ln{j}/bias"] = [base + (f"LayerNorm_{j - 1}", "bias")]


def theta_paths(image_keys, critic_mlp_name="network", encoder_type="resnet-pretrained", std_parameterization="exp",
                critic_dims=None, policy_dims=None, critic_layer_norm=True, policy_layer_norm=True, use_proprio=True):
    """flat trainable leaf -> list of flax paths (aliases).  use_proprio False: `encoder` holds the cameras' `encoder_<key>` alone,
    no Dense_0 or LayerNorm_0 (common/encoding.py:53-72).  critic_dims / policy_dims: the hidden widths of each MLP (only their
    count matters here; None: two layers).  critic_layer_norm / policy_layer_norm False: no LayerNorm_<j> under that network."""
    enc = ("modules_actor", "encoder")
    m = {}
    nc, na = (2 if critic_dims is None else len(critic_dims)), (2 if policy_dims is None else len(policy_dims))
    if len(image_keys) == 0:
        # SACAgent.create_states: Policy(encoder=None, network=MLP) and ensemblize(Critic(encoder=None, network=MLP))
        # -- the vmapped Critic keeps its module names, every leaf gains a leading ensemble axis (sac.py:516-524)
        return _state_paths(std_parameterization, nc, na, critic_layer_norm, policy_layer_norm)
    for i, k in enumerate(image_keys):
        e = enc + (f"encoder_{k}",)
        if encoder_type == "small":   # SmallEncoder (small_encoders.py:9-55): Conv_0..3 {kernel, bias}
            for l in range(4):
                m[f"enc/{i}/conv{l}/kernel"] = [e + (f"Conv_{l}", "kernel")]
                m[f"enc/{i}/conv{l}/bias"] = [e + (f"Conv_{l}", "bias")]
        else:
            m[f"enc/{i}/sle"] = [e + ("SpatialLearnedEmbeddings_0", "kernel")]
        m[f"enc/{i}/dense/kernel"] = [e + ("Dense_0", "kernel")]
        m[f"enc/{i}/dense/bias"] = [e + ("Dense_0", "bias")]
        m[f"enc/{i}/ln/scale"] = [e + ("LayerNorm_0", "scale")]
        m[f"enc/{i}/ln/bias"] = [e + ("LayerNorm_0", "bias")]
    if use_proprio:
        m["enc/proprio/dense/kernel"] = [enc + ("Dense_0", "kernel")]
        m["enc/proprio/dense/bias"] = [enc + ("Dense_0", "bias")]
        m["enc/proprio/ln/scale"] = [enc + ("LayerNorm_0", "scale")]
        m["enc/proprio/ln/bias"] = [enc + ("LayerNorm_0", "bias")]
    _mlp_paths(m, "critic", ("modules_critic", critic_mlp_name), nc, critic_layer_norm)
    m["critic/head/kernel"] = [("modules_critic", "Dense_0", "kernel")]
    m["critic/head/bias"] = [("modules_critic", "Dense_0", "bias")]
    _mlp_paths(m, "actor", ("modules_actor", "network"), na, policy_layer_norm)
    m["actor/mean/kernel"] = [("modules_actor", "Dense_0", "kernel")]
    m["actor/mean/bias"] = [("modules_actor", "Dense_0", "bias")]
    m.update(_policy_std_paths(std_parameterization))
    m["temp/lagrange"] = [("modules_temperature", "lagrange")]
    return m


def _state_paths(std_parameterization="exp", n_critic=2, n_policy=2, critic_layer_norm=True, policy_layer_norm=True):
    m = {}
    for mod, pre, n, ln in (("modules_critic", "critic", n_critic, critic_layer_norm), ("modules_actor", "actor", n_policy, policy_layer_norm)):
        _mlp_paths(m, pre, (mod, "network"), n, ln)
    m["critic/head/kernel"] = [("modules_critic", "Dense_0", "kernel")]
    m["critic/head/bias"] = [("modules_critic", "Dense_0", "bias")]
    m["actor/mean/kernel"] = [("modules_actor", "Dense_0", "kernel")]
    m["actor/mean/bias"] = [("modules_actor", "Dense_0", "bias")]
    m.update(_policy_std_paths(std_parameterization))
    m["temp/lagrange"] = [("modules_temperature", "lagrange")]
    return m


def bc_paths(image_keys, use_proprio=True):
    """flat BC leaf (csrc/bc.hip) -> flax path in BCAgent.state.params (bc.py:118-204): Policy is `modules_actor`, its
    EncodingWrapper `encoder` (per camera `encoder_<key>`, the proprio Dense_0 / LayerNorm_0), its MLP `network`
    (Dense_0, Dense_1 -- no LayerNorm), the heads Dense_0 (mean) and Dense_1 (log_std); the shared frozen trunk sits under
    the first camera in sorted-key order, as in DrQ.  use_proprio False (BCAgent.create's own default): no Dense_0 / LayerNorm_0
    under `encoder`."""
    enc = ("modules_actor", "encoder")
    m = {}
    for leaf, sub in _trunk_paths().items():
        m[leaf] = enc + (f"encoder_{trunk_owner(image_keys)}", "pretrained_encoder") + sub
    for i, k in enumerate(image_keys):
        for leaf, sub in CAM_PATHS.items():
            m[f"enc/{i}/{leaf}"] = enc + (f"encoder_{k}",) + sub
    if use_proprio:
        m["enc/proprio/dense/kernel"] = enc + ("Dense_0", "kernel")
        m["enc/proprio/dense/bias"] = enc + ("Dense_0", "bias")
        m["enc/proprio/ln/scale"] = enc + ("LayerNorm_0", "scale")
        m["enc/proprio/ln/bias"] = enc + ("LayerNorm_0", "bias")
    for j in (0, 1):
        m[f"actor/w{j + 1}"] = ("modules_actor", "network", f"Dense_{j}", "kernel")
        m[f"actor/b{j + 1}"] = ("modules_actor", "network", f"Dense_{j}", "bias")
    m["actor/mean/kernel"] = ("modules_actor", "Dense_0", "kernel")
    m["actor/mean/bias"] = ("modules_actor", "Dense_0", "bias")
    m["actor/logstd/kernel"] = ("modules_actor", "Dense_1", "kernel")
    m["actor/logstd/bias"] = ("modules_actor", "Dense_1", "bias")
    return m


def _camera_shapes(n_cam, H, W, bottleneck):
    """flat leaf -> flax shape of the per-camera heads on the frozen trunk (enc/<i>/...)"""
    from ..utils.init import feat_hw
    fh, fw = feat_hw(H, W)
    sh = {}
    for i in range(n_cam):
        sh[f"enc/{i}/sle"] = (fh, fw, 512, 8)
        sh[f"enc/{i}/dense/kernel"] = (512 * 8, bottleneck)
        sh[f"enc/{i}/dense/bias"] = sh[f"enc/{i}/ln/scale"] = sh[f"enc/{i}/ln/bias"] = (bottleneck,)
    return sh


def bc_shapes(image_keys, H, W, S, A, hidden=256, bottleneck=256, proprio_dim=64, use_proprio=True):
    """flat BC leaf -> flax shape; use_proprio False: no enc/proprio leaves, actor/w1 (bottleneck * n_cam, hidden)"""
    sh = dict(trunk_shapes(), **_camera_shapes(len(image_keys), H, W, bottleneck))
    if use_proprio:
        sh["enc/proprio/dense/kernel"] = (S, proprio_dim)
        sh["enc/proprio/dense/bias"] = sh["enc/proprio/ln/scale"] = sh["enc/proprio/ln/bias"] = (proprio_dim,)
    sh["actor/w1"], sh["actor/b1"] = (bottleneck * len(image_keys) + (proprio_dim if use_proprio else 0), hidden), (hidden,)
    sh["actor/w2"], sh["actor/b2"] = (hidden, hidden), (hidden,)
    sh["actor/mean/kernel"], sh["actor/mean/bias"] = (hidden, A), (A,)
    sh["actor/logstd/kernel"], sh["actor/logstd/bias"] = (hidden, A), (A,)
    return sh


def trunk_owner(image_keys):
    """camera whose subtree holds the shared frozen trunk (first key in sorted order)."""
    return sorted(image_keys)[0]


def export_tree(core, section: str, image_keys, duplicate_encoder_under_critic: bool = False,
                critic_mlp_name: str = "network", trunk_under_every_camera: bool = False, get=None) -> Dict:
    """Nested dict of np.float32 arrays in flax layout (HWIO convs, (in,out) dense, ensemble axis 0).  get(section, leaf) -> the
    leaf's flat values; None = core.get, a copy out of HBM (a StateSnapshot passes views into its pinned buffer)."""
    get = core.get if get is None else get
    cfg = core.cfg
    etype = "small" if cfg.encoder_type == 1 else "resnet-pretrained"
    net = net_spec_of(core).leaf_kwargs()
    shapes = theta_shapes(cfg.n_cam, cfg.H, cfg.W, cfg.state_dim, cfg.act_dim, ensemble=cfg.ensemble, encoder_type=etype,
                          num_stack=max(cfg.num_stack, 1), **net)
    shapes.update(trunk_shapes())
    paths = theta_paths(image_keys, critic_mlp_name, etype, **net)
    if cfg.n_cam and etype != "small":
        # ONE frozen trunk: drq.py:165-176 passes the same `pretrained_encoder` module to every camera's
        # PreTrainedResNetEncoder, flax adopts a shared module once -- under the first camera in sorted-key order --
        # which is why train_utils.py:118-123 guards with `if "pretrained_encoder" in new_encoder_params`
        owners = image_keys if trunk_under_every_camera else (trunk_owner(image_keys),)
        for leaf, sub in _trunk_paths().items():
            paths[leaf] = [("modules_actor", "encoder", f"encoder_{k}", "pretrained_encoder") + sub for k in owners]
    if duplicate_encoder_under_critic:
        for leaf, ps in paths.items():
            paths[leaf] = [q for p in ps
                           for q in ([p, ("modules_critic",) + p[1:]] if p[:2] == ("modules_actor", "encoder") else [p])]
    return tree_from_leaves(paths, shapes, lambda leaf: get(section, leaf))


def trunk_from_flax(pretrained: Dict) -> Dict[str, np.ndarray]:
    """resnet10_params.pkl tree -> flat leaves.  Top-level keys are matched by name and a top-level key the pickle
    does not hold keeps its current value (train_utils.py:124-127: `for k in new_encoder_params: if k in encoder_params`);
    a top-level key that is present must hold the whole sub-tree."""
    present = {leaf: sub for leaf, sub in _trunk_paths().items() if sub[0] in pretrained}
    return {leaf: np.asarray(v, np.float32) for leaf, v in leaves_from_tree(present, pretrained)}
