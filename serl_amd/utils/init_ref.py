"""Parameter initialisation from the seed as the reference does it (param_init="reference").

The reference builds every network with `model_def.init(init_rng, ...)` (agents/continuous/drq.py:69-75, sac.py:368-374, bc.py:118-204,
networks/reward_classifier.py:31-90): flax hands each parameter the key `make_rng("params")` of its module -- the root key folded
with the module's path and the scope's call counter (kernel 1, bias 2; jaxrng.flax_make_rng) -- and the initialiser draws from
jax.random's threefry stream.  This module derives those keys and draws the leaves on the device (serl_jax_init_fill, one launch
per 64 leaves), with the flat leaf names and shapes of init.init_theta / init.init_classifier:

  * Dense kernels of MLPs, policy heads and the critic head: default_init = xavier_uniform (common/common.py:15, networks/mlp.py:24,
    actor_critic_nets.py:72,189-192); the proprio Dense: xavier_uniform (common/encoding.py:63-65);
  * SpatialLearnedEmbeddings: lecun_normal (vision/resnet_v1.py:86); the camera bottleneck Dense, the SmallEncoder convs and Dense,
    and the classifier head: flax's default lecun_normal (truncated normal, std sqrt(1 / fan_in) / 0.87962566);
  * LayerNorm scale ones, biases zeros; the temperature: log(exp(temperature_init) - 1) in float32 ops (networks/lagrange.py:28-29);
  * the critic ensemble (nn.vmap with split_rngs={"params": True}, actor_critic_nets.py:156-164): member i draws under
    split(init_rng, N)[i] with the same path suffix -- flax's lifted split of the LazyRng's key (flax/core/lift.py vmap), not fold_in.

variance_scaling's float32 op order (jax/_src/nn/initializers.py): var = float32(scale / denominator); uniform(-1, 1) * sqrt(3 * var)
and truncated_normal(-2, 2) * (sqrt(var) / 0.87962566).  The frozen ResNet-10 trunk is not drawn here: the reference overwrites it
with the pretrained pickle, so it keeps init.init_trunk's values until load_resnet10_params / load_trunk_params.

What rests on restatement (no jax / flax install exists to run against): threefry and split / fold_in are pinned on known-answer
vectors (tests/test_threefry_oracle.py); XLA's float32 erf and ErfInv32 polynomials, the truncated normal's clip, flax's
`_fold_in_static` key rule, its lifted vmap split and the counter order inside a scope are restated from the published sources.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from .. import jaxrng as J
from .init import theta_shapes

XAVIER_UNIFORM, LECUN_NORMAL, ONES, ZEROS, LAGRANGE = "xavier_uniform", "lecun_normal", "ones", "zeros", "lagrange"


class Leaf(NamedTuple):
    name: str                  # flat leaf name (init.init_theta / init.init_classifier)
    path: tuple                # flax module path of the parameter's module (names from the root)
    counter: int               # make_rng("params") call of that scope: kernel / scale 1, bias 2
    init: str
    shape: tuple               # the full leaf shape (ensemble axis first for vmapped leaves)
    members: int = 0           # > 0: nn.vmap over `members`; each member draws shape[1:] under split(init_rng, members)[i]


def _fans(shape):
    """jax.nn.initializers._compute_fans with in_axis=-2, out_axis=-1"""
    receptive = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    return shape[-2] * receptive, shape[-1] * receptive


def _job_args(init, shape):
    """(kind, minval, maxval, scale) of variance_scaling's draw for one array of `shape`, in float32 as jax computes them."""
    fan_in, fan_out = _fans(shape)
    if init == XAVIER_UNIFORM:     # variance_scaling(1.0, "fan_avg", "uniform")
        var = np.float32(1.0 / ((fan_in + fan_out) / 2))
        return J.INIT_UNIFORM, -1.0, 1.0, np.sqrt(np.float32(3) * var)
    if init == LECUN_NORMAL:       # variance_scaling(1.0, "fan_in", "truncated_normal")
        var = np.float32(1.0 / fan_in)
        return J.INIT_TRUNCATED_NORMAL, -2.0, 2.0, np.sqrt(var) / np.float32(0.87962566103423978)
    raise ValueError(init)


def _split_path(path):
    """flax path of a parameter -> (module path, parameter name)"""
    return tuple(path[:-1]), path[-1]


def _counter(pname):
    return 2 if pname == "bias" else 1


def _init_of(name, shape):
    if name.endswith("/scale"):
        return ONES
    if name.endswith("bias") or name.startswith("critic/b") or name.startswith("actor/b") or name == "actor/log_stds":
        return ZEROS    # (log_stds: nn.initializers.zeros, actor_critic_nets.py:199-201 -- no draw, no key consumed)
    if name == "temp/lagrange":
        return LAGRANGE
    if name.endswith("/sle") or "/conv" in name or (name.startswith("enc/") and "proprio" not in name) or name.startswith("head/"):
        return LECUN_NORMAL
    return XAVIER_UNIFORM


def theta_leaves(image_keys: Sequence[str], H, W, S, A, ensemble=10, encoder_type="resnet-pretrained", num_stack=1,
                 hidden=256, std_parameterization="exp", critic_dims=None, policy_dims=None, critic_layer_norm=True,
                 policy_layer_norm=True, use_proprio=True) -> List[Leaf]:
    """The trainable leaves of DrQAgent.create_drq (image_keys non-empty) or SACAgent.create_states (image_keys empty);
    hidden: the MLPs' width (hidden_dims=[hidden, hidden]), or critic_dims / policy_dims: each MLP's own widths, layer by layer
    (Dense_2 / LayerNorm_2 and up take their keys from their paths like every other leaf).  std_parameterization="uniform": the zero-initialised log_stds
    vector in place of Dense_1; every other leaf keeps its key (a flax key depends on the module's path and the scope's own
    counter, not on its siblings), so the rest of the tree is bit-identical to the "exp" agent's.  "fixed"
    (actor_critic_nets.py:189-192): no std leaf at all, the rest as for "exp" by the same argument.
    critic_layer_norm / policy_layer_norm False (mlp.py:29-30): that MLP has no LayerNorm leaves; a LayerNorm draws nothing, so the
    Dense leaves keep their keys and values.
    use_proprio False (common/encoding.py:53-72): `encoder` has no Dense_0 / LayerNorm_0; the camera heads keep their keys by the
    same argument, and the two first kernels draw with the fan-in of the image codes alone."""
    from ..agents.flax_tree import theta_paths
    shapes = theta_shapes(len(image_keys), H, W, S, A, ensemble=ensemble, hidden=hidden, encoder_type=encoder_type,
                          num_stack=num_stack, std_parameterization=std_parameterization, critic_dims=critic_dims,
                          policy_dims=policy_dims, critic_layer_norm=critic_layer_norm, policy_layer_norm=policy_layer_norm,
                          use_proprio=use_proprio)
    paths = theta_paths(tuple(image_keys), encoder_type=encoder_type, std_parameterization=std_parameterization,
                        critic_dims=critic_dims, policy_dims=policy_dims, critic_layer_norm=critic_layer_norm,
                        policy_layer_norm=policy_layer_norm, use_proprio=use_proprio)
    # the vmapped module: DrQ ensemblizes the critic's MLP (drq.py:206-209), state SAC the whole Critic (sac.py:516-517)
    vm = ("modules_critic", "network") if image_keys else ("modules_critic",)
    out = []
    for name, shp in shapes.items():
        mod, pname = _split_path(paths[name][0])
        members = ensemble if mod[:len(vm)] == vm else 0
        out.append(Leaf(name, mod, _counter(pname), _init_of(name, shp), tuple(shp), members))
    return out


def bc_leaves(image_keys: Sequence[str], H, W, S, A, use_proprio=True) -> List[Leaf]:
    """The trainable leaves of BCAgent.create (no LayerNorm in the policy MLP); use_proprio False: without the proprio branch."""
    from ..agents.flax_tree import bc_paths, bc_shapes
    from .init import trunk_shapes
    shapes, paths = bc_shapes(tuple(image_keys), H, W, S, A, use_proprio=use_proprio), bc_paths(tuple(image_keys), use_proprio)
    out = []
    for name, shp in shapes.items():
        if name in trunk_shapes():
            continue
        mod, pname = _split_path(paths[name])
        out.append(Leaf(name, mod, _counter(pname), _init_of(name, shp), tuple(shp)))
    return out


def classifier_leaves(image_keys: Sequence[str], H, W) -> List[Leaf]:
    """The trainable leaves of create_classifier (BinaryClassifier over EncodingWrapper(use_proprio=False))."""
    from ..agents.flax_tree import _trunk_paths
    from ..networks.reward_classifier import _tree_paths, _tree_shapes
    keys = tuple(image_keys)
    shapes, paths = _tree_shapes(keys, H, W), _tree_paths(keys)
    trunk = _trunk_paths()
    out = []
    for name, shp in shapes.items():
        if name in trunk:
            continue
        mod, pname = _split_path(paths[name])
        flat = name
        if name.startswith("enc/"):    # init_classifier's names carry the camera index
            _, k, rest = name.split("/", 2)
            flat = f"enc/{keys.index(k)}/{rest}" if k in keys else name
        out.append(Leaf(flat, mod, _counter(pname), _init_of(flat, shp), tuple(shp)))
    return out


def leaf_keys(leaf: Leaf, init_rng) -> np.ndarray:
    """uint32[max(members, 1)][2]: the key(s) the leaf's initialiser is called with."""
    if leaf.members:
        return np.stack([J.flax_make_rng(k, leaf.path, leaf.counter) for k in J.split(init_rng, leaf.members)])
    return J.flax_make_rng(init_rng, leaf.path, leaf.counter)[None]


def lagrange_init(temperature_init: float) -> np.float32:
    """GeqLagrangeMultiplier's softplus parameterisation in float32 ops: log(exp(t) - 1), each op rounded to float32."""
    e = np.float32(np.exp(np.float64(np.float32(temperature_init))))
    return np.float32(np.log(np.float64(np.float32(e - np.float32(1.0)))))


def draw(leaves: Sequence[Leaf], init_rng, device: int = 0, temperature_init: float = 1.0, stream=None) -> Dict:
    """{flat name: tensor on `device`} of every leaf: the random ones in one serl_jax_init_fill launch (per 64 draws)."""
    import torch
    dev = torch.device("cuda", device)
    out, jobs = {}, []
    for lf in leaves:
        if lf.init in (ONES, ZEROS):
            out[lf.name] = (torch.ones if lf.init == ONES else torch.zeros)(lf.shape, dtype=torch.float32, device=dev)
            continue
        if lf.init == LAGRANGE:
            out[lf.name] = torch.full(lf.shape, float(lagrange_init(temperature_init)), dtype=torch.float32, device=dev)
            continue
        t = torch.empty(lf.shape, dtype=torch.float32, device=dev)
        per = lf.shape[1:] if lf.members else lf.shape
        kind, lo, hi, scale = _job_args(lf.init, per)
        n = int(np.prod(per))
        for i, k in enumerate(leaf_keys(lf, init_rng)):
            jobs.append(J.init_job(kind, k, n, t.data_ptr() + i * n * 4, lo, hi, scale))
        out[lf.name] = t
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    J.init_fill(device, jobs, stream)
    torch.cuda.synchronize(dev)
    return out


def draw_host(leaves: Sequence[Leaf], init_rng, temperature_init: float = 1.0) -> Dict[str, np.ndarray]:
    """The same leaves from the library's host code (serl_jax_init_host): tests and machines without a GPU."""
    out = {}
    for lf in leaves:
        if lf.init in (ONES, ZEROS):
            out[lf.name] = (np.ones if lf.init == ONES else np.zeros)(lf.shape, np.float32)
        elif lf.init == LAGRANGE:
            out[lf.name] = np.full(lf.shape, lagrange_init(temperature_init), np.float32)
        else:
            per = lf.shape[1:] if lf.members else lf.shape
            kind, lo, hi, scale = _job_args(lf.init, per)
            n = int(np.prod(per))
            out[lf.name] = np.stack([J.init_host(kind, k, n, lo, hi, scale) for k in leaf_keys(lf, init_rng)]).reshape(lf.shape)
    return out


def init_rng_of(rng) -> np.ndarray:
    """`rng, init_rng = jax.random.split(rng)` of the agents' create paths -> init_rng"""
    return J.split(rng)[1]


create_rng_of = J.create_rng       # state.rng the create paths leave, from an int seed or a key


def reference_key(rng) -> np.ndarray:
    """an int seed (PRNGKey(seed)) or a key uint32[2]"""
    return J.prngkey(int(rng)) if np.ndim(rng) == 0 else np.asarray(rng, np.uint32).reshape(2)


def to_host(flat: Dict) -> Dict[str, np.ndarray]:
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in flat.items()}


def draw_flat(leaves: Sequence[Leaf], init_rng, device: Optional[int] = 0, temperature_init: float = 1.0) -> Dict[str, np.ndarray]:
    """{flat name: float32 array} drawn on `device` (on the host when device is None), ready for the handles' load_flat / set."""
    if device is None:
        return draw_host(leaves, init_rng, temperature_init)
    return to_host(draw(leaves, init_rng, device, temperature_init))


def theta_reference(image_keys, H, W, S, A, rng, ensemble=10, encoder_type="resnet-pretrained", temperature_init=1.0,
                    device: Optional[int] = 0, num_stack=1, hidden=256, std_parameterization="exp", critic_dims=None,
                    policy_dims=None, critic_layer_norm=True, policy_layer_norm=True, use_proprio=True) -> Dict[str, np.ndarray]:
    """init_theta's leaves as the reference's DrQ / state-SAC create path draws them from `rng` (drq.py:69, sac.py:368).
    S is the flattened proprio width T * S of a stack of T = num_stack frames; the widened leaves draw with their real fan-in.
    hidden: the MLPs' width; its leaves draw with the fans of that width."""
    return draw_flat(theta_leaves(image_keys, H, W, S, A, ensemble, encoder_type, num_stack, hidden, std_parameterization,
                                  critic_dims, policy_dims, critic_layer_norm, policy_layer_norm, use_proprio),
                     init_rng_of(reference_key(rng)),
                     device, temperature_init)


def bc_reference(image_keys, H, W, S, A, rng, device: Optional[int] = 0, use_proprio=True) -> Dict[str, np.ndarray]:
    """BCAgent.create's trainable leaves from `rng` (bc.py: rng, init_rng = split(rng))."""
    return draw_flat(bc_leaves(image_keys, H, W, S, A, use_proprio), init_rng_of(reference_key(rng)), device)


def classifier_reference(image_keys, H, W, key, device: Optional[int] = 0) -> Dict[str, np.ndarray]:
    """create_classifier's trainable leaves: classifier_def.init(key, sample) -- the key itself, no split
    (reward_classifier.py:59)."""
    return draw_flat(classifier_leaves(image_keys, H, W), reference_key(key), device)


PARAM_INITS = ("numpy", "reference")


def check_param_init(param_init: str) -> bool:
    """-> True for "reference"; raises on an unknown value"""
    if param_init not in PARAM_INITS:
        raise ValueError(f"param_init must be one of {PARAM_INITS}, got {param_init!r}")
    return param_init == "reference"
