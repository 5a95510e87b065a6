"""Checkpoint save / restore of `agent.state` (next-row N1).

The reference calls `flax.training.checkpoints.save_checkpoint(path, agent.state, step=, keep=)`
(examples/async_drq_sim/async_drq_sim.py:303-307), which writes `<path>/checkpoint_<step>` containing
`flax.serialization.to_bytes(state)`: a msgpack map of the state's pytree fields (`step, params,
target_params, opt_states, rng`; common/common.py:108-114) in which every ndarray is a msgpack ExtType(1)
holding msgpack((shape, dtype.name, raw bytes)).  flax is not installable here, so this writer/reader
restates that published format; the TREE inside (parameter paths, the optax InjectHyperparamsState / chain /
ScaleByAdamState nesting of `opt_states`) is checked against the state the reference's own code builds under the
stand-ins of oracle/jaxshim (tests/test_reference_update.py).  `restore_checkpoint` below reads such files back into
the HIP agent (params, target_params, Adam moments, step).
"""
from __future__ import annotations

import os
import re
import shutil
from typing import Optional

import msgpack
import numpy as np

from ..agents.core import TX_NAMES
from ..agents.flax_tree import leaves_from_tree, net_spec_of, theta_paths, trunk_owner, _trunk_paths

_EXT_NDARRAY = 1


def _pack_default(x):
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.asarray(x)
        return msgpack.ExtType(_EXT_NDARRAY, msgpack.packb((list(a.shape), a.dtype.name, a.tobytes("C")), use_bin_type=True))
    raise TypeError(f"cannot serialise {type(x)}")


def _unpack_ext(code, data):
    if code == _EXT_NDARRAY:
        shape, dtype, buf = msgpack.unpackb(data, raw=False)
        return np.frombuffer(buf, dtype=np.dtype(dtype)).reshape(shape).copy()
    return msgpack.ExtType(code, data)


def _own_form(agent):
    """A train state that writes / reads its own state-dict form (BCAgent's single-optimizer state, agents/bc.py; the
    trainable reward classifier's flax TrainState, networks/reward_classifier.py), given as the agent or as its `.state`
    -- or None."""
    for x in (agent, getattr(agent, "state", None)):
        if x is not None and hasattr(x, "state_dict") and hasattr(x, "load_state_dict"):
            return x
    return None


def state_dict(agent) -> dict:
    own = _own_form(agent)
    if own is not None:
        return own.state_dict()
    st = agent.state
    return {"step": np.int32(st.step), "params": st.params, "target_params": st.target_params,
            "opt_states": st.opt_states, "rng": st.rng}


def save_checkpoint(ckpt_dir: str, agent, step: int, prefix: str = "checkpoint_", keep: int = 1, overwrite: bool = False) -> str:
    """`agent`: an agent, or a StateSnapshot of all three sections (agent.snapshot(("params", "target_params", "opt_states")),
    agents/snapshot.py), which writes the file the agent would have written at the snapshot's step.  A snapshot that holds Inf or
    NaN values is refused before any file is touched: a diverged run does not overwrite its last good checkpoint."""
    if getattr(agent, "finite", True) is False:
        raise ValueError(f"the snapshot of step {getattr(agent, 'step', '?')} holds non-finite values {getattr(agent, 'nonfinite', {})}: "
                         f"no checkpoint written, {ckpt_dir} is left as it was")
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, f"{prefix}{step}")
    if os.path.exists(path) and not overwrite:
        raise ValueError(f"checkpoint {path} exists (overwrite=False)")
    blob = msgpack.packb(state_dict(agent), default=_pack_default, strict_types=True, use_bin_type=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(blob)
    os.replace(tmp, path)
    # keep the `keep` most recent checkpoints (flax semantics)
    steps = sorted(int(m.group(1)) for m in (re.fullmatch(re.escape(prefix) + r"(\d+)", n) for n in os.listdir(ckpt_dir)) if m)
    for s in steps[:-keep] if keep > 0 else []:
        os.remove(os.path.join(ckpt_dir, f"{prefix}{s}"))
    return path


def latest_checkpoint(ckpt_dir: str, prefix: str = "checkpoint_") -> Optional[str]:
    if not os.path.isdir(ckpt_dir):
        return None
    steps = [int(m.group(1)) for m in (re.fullmatch(re.escape(prefix) + r"(\d+)", n) for n in os.listdir(ckpt_dir)) if m]
    return os.path.join(ckpt_dir, f"{prefix}{max(steps)}") if steps else None


def restore_checkpoint(ckpt_dir_or_file: str, agent, step: Optional[int] = None, prefix: str = "checkpoint_",
                       restore_rng: bool = False):
    """Loads params / target_params / Adam moments / step back into the agent's HBM arena; with restore_rng=True also
    `state.rng` (see load_state_dict)."""
    path = ckpt_dir_or_file
    if os.path.isdir(path):
        path = os.path.join(path, f"{prefix}{step}") if step is not None else latest_checkpoint(path, prefix)
        if path is None:
            return agent  # flax returns the target unchanged when there is nothing to restore
    with open(path, "rb") as f:
        sd = msgpack.unpackb(f.read(), ext_hook=_unpack_ext, raw=False, strict_map_key=False)
    return load_state_dict(agent, sd, restore_rng=restore_rng)


def read_checkpoint_tree(ckpt_dir_or_file: str, step: Optional[int] = None, prefix: str = "checkpoint_") -> dict:
    """The state dict stored in a flax checkpoint file (or the latest / the given step of a directory of them)."""
    path = ckpt_dir_or_file
    if os.path.isdir(path):
        path = os.path.join(path, f"{prefix}{step}") if step is not None else latest_checkpoint(path, prefix)
        if path is None:
            raise FileNotFoundError(f"no {prefix}<step> file in {ckpt_dir_or_file}")
    with open(path, "rb") as f:
        return msgpack.unpackb(f.read(), ext_hook=_unpack_ext, raw=False, strict_map_key=False)


def write_checkpoint_tree(ckpt_dir: str, tree: dict, step: int, prefix: str = "checkpoint_") -> str:
    """Writes `tree` (nested dicts of ndarrays / scalars) as <ckpt_dir>/<prefix><step> in the same msgpack layout."""
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, f"{prefix}{step}")
    with open(path, "wb") as f:
        f.write(msgpack.packb(tree, default=_pack_default, strict_types=True, use_bin_type=True))
    return path


def _find_adam_state(node):
    """The ScaleByAdamState {count, mu, nu} inside an InjectHyperparamsState / chain state dict (any nesting), or the
    node itself for the flat {count, mu, nu} layout written by earlier versions of this module."""
    if isinstance(node, dict):
        if "mu" in node and "nu" in node:
            return node
        for v in node.values():
            r = _find_adam_state(v)
            if r is not None:
                return r
    return None


STD_LEAVES = ("actor/logstd/kernel", "actor/logstd/bias", "actor/log_stds")


def _absent(tree, path) -> bool:
    for k in path:
        if not isinstance(tree, dict) or k not in tree:
            return True
        tree = tree[k]
    return False


def load_state_dict(agent, sd: dict, restore_rng: bool = False):
    """Loads any of {params, target_params, opt_states, step} (flax-layout trees, e.g. a restored checkpoint or
    `agent.state.replace(...)` arguments) into the agent's HBM arena.  restore_rng=True also takes `state.rng` from `sd["rng"]`
    (DrQAgent / SACAgent): crop offsets, REDQ indices, policy normals and Dropout masks all derive from it, so only then does the
    agent CONTINUE the run the state was saved from.  Off by default: a restored agent keeps the rng it was created with, as
    before.  Agents with their own state-dict form decide themselves and ignore the flag: BCAgent's form carries `rng` and
    restores it whenever it is present; the reward classifier's TrainState has no rng (its Dropout keys come from the caller)."""
    own = _own_form(agent)
    if own is not None:
        own.load_state_dict(sd)
        return agent
    core, keys = agent.core, agent.image_keys
    etype = "small" if core.cfg.encoder_type == 1 else "resnet-pretrained"
    spec = net_spec_of(core)
    cd, pd = spec.dims
    lns = {"critic": spec.critic_layer_norm, "actor": spec.policy_layer_norm}
    tp = theta_paths(keys, encoder_type=etype, **spec.leaf_kwargs())
    # the leaves whose PRESENCE is geometry: the policy's std leaves (std_parameterization "uniform": log_stds, else Dense_1) and
    # the MLPs' layers (hidden_dims of any length: Dense_j / LayerNorm_j below each `network`)
    mlp_leaves = tuple(leaf for leaf in tp if re.fullmatch(r"(critic|actor)/(w|b|ln)\d+(/scale|/bias)?", leaf))
    optional = STD_LEAVES + mlp_leaves
    mlp_modules = {net: (tp[f"{net}/w1"][0][:-2], n) for net, n in (("critic", len(cd)), ("actor", len(pd)))}
    trunk = _trunk_paths() if (keys and etype != "small") else {}   # state-only / SmallEncoder agents have no frozen trunk
    todo = []      # (section, leaf, array): everything is sized against the agent's leaves before the first one is written

    std_mode = spec.std_parameterization
    std_modules = {"Dense_1": "actor/logstd", "log_stds": "actor/log_stds"}   # what Policy keeps its std in, below modules_actor

    def leaves_of(tree, section):
        # std_parameterization="fixed" against a state with std leaves, either way round: said in those words, before any size
        actor = tree.get("modules_actor") if isinstance(tree, dict) else None
        if isinstance(actor, dict):
            held = [m for m in std_modules if m in actor]
            if std_mode == "fixed" and held:
                raise ValueError(f"{section}: the state holds the policy's std leaves ('modules_actor/{held[0]}'), this agent's head has "
                                 "a fixed std and no std leaf (std_parameterization='fixed'); nothing was loaded")
            if std_mode != "fixed" and not held and not _absent(tree, tp["actor/mean/kernel"][0]):
                raise ValueError(f"{section}: the state holds no std leaf of the policy (neither 'modules_actor/Dense_1' nor "
                                 "'modules_actor/log_stds': written by a std_parameterization='fixed' agent), this agent's head has "
                                 f"'{std_modules['log_stds' if std_mode == 'uniform' else 'Dense_1']}'; nothing was loaded")
        # an image-only state (use_proprio=False: `encoder` holds the cameras alone) against an agent with the proprio branch, either
        # way round: said in those words, before any size
        enc = ("modules_actor", "encoder")
        if keys and not _absent(tree, enc):
            held = not _absent(tree, enc + ("Dense_0",)) or not _absent(tree, enc + ("LayerNorm_0",))
            if held and not spec.use_proprio:
                raise ValueError(f"{section}: the state holds the proprio branch ('modules_actor/encoder/Dense_0': written by a "
                                 "use_proprio=True agent), this agent is image-only (use_proprio=False) and has no such leaf; nothing was loaded")
            if not held and spec.use_proprio:
                raise ValueError(f"{section}: the state holds no proprio branch ('modules_actor/encoder/Dense_0' is absent: written by an "
                                 "image-only agent, use_proprio=False), this agent has one (use_proprio=True); nothing was loaded")
        # a tree of another kind holds nothing at the paths of such a leaf, which the size check below reports as 0 elements ...
        for leaf in optional:
            if leaf in tp and _absent(tree, tp[leaf][0]):
                if re.fullmatch(r"(critic|actor)/ln1/scale", leaf) and not _absent(tree, tp[leaf.split("/")[0] + "/w1"][0]):
                    net = leaf.split("/")[0]
                    raise ValueError(f"{section}: the state's {net} MLP has no LayerNorm ('{'/'.join(tp[leaf][0][:-1])}' is absent: "
                                     f"use_layer_norm=False), this agent's {net} MLP has one; nothing was loaded")
                yield leaf, np.zeros((0,), np.float32)
        # ... and a layer the tree holds and this agent lacks is refused here: no leaf of the agent would ever meet it
        for net, (mod, n) in mlp_modules.items():
            if _absent(tree, mod):
                continue
            d = tree
            for k in mod:
                d = d[k]
            for name in sorted(d):
                m = re.fullmatch(r"(Dense|LayerNorm)_(\d+)", name)
                if m and m.group(1) == "LayerNorm" and not lns[net]:
                    raise ValueError(f"{section}: '{'/'.join(mod + (name,))}' is a LayerNorm in the state, this agent's {net} MLP has "
                                     f"none (use_layer_norm=False); nothing was loaded")
                if m and int(m.group(2)) >= n:
                    got = sum(int(np.size(v)) for v in d[name].values()) if isinstance(d[name], dict) else int(np.size(d[name]))
                    raise ValueError(f"{section}: '{'/'.join(mod + (name,))}' holds {got} elements in the state, this agent's {net} MLP "
                                     f"has {n} layers and 0 elements there; nothing was loaded")
        yield from leaves_from_tree({leaf: p for leaf, p in tp.items() if leaf not in optional or not _absent(tree, p[0])}, tree)
    for section in ("params", "target_params"):
        tree = sd.get(section)
        if tree is None:
            continue
        todo += [(section, leaf, v) for leaf, v in leaves_of(tree, section)]
        if trunk:
            # Where flax puts the ONE shared frozen trunk is derived from its adoption rule (first camera in sorted-key
            # order) and unverified against a real flax install: accept it under any camera, like
            # reward_classifier.load_params and the reference's own `if "pretrained_encoder" in ...` guard do
            enc = tree["modules_actor"]["encoder"]
            owners = [k for k in [trunk_owner(keys)] + sorted(keys) if "pretrained_encoder" in enc.get(f"encoder_{k}", {})]
            if not owners:
                raise KeyError(f"'{section}' holds no pretrained_encoder under any of encoder_{{{', '.join(sorted(keys))}}}")
            root = enc[f"encoder_{owners[0]}"]["pretrained_encoder"]
            todo += [(section, leaf, v) for leaf, v in leaves_from_tree(trunk, root)]
    if sd.get("opt_states") is not None:
        for tx in TX_NAMES:
            adam = _find_adam_state(sd["opt_states"][tx])
            if adam is None:
                raise KeyError(f"opt_states['{tx}'] holds no ScaleByAdamState (mu / nu)")
            for mom in ("mu", "nu"):
                # leaves outside the optimizer's support are exact zeros; the C ABI accepts (and checks) them
                todo += [(f"opt/{tx}/{mom}", leaf, np.asarray(v, np.float32)) for leaf, v in leaves_of(adam[mom], f"opt_states/{tx}/{mom}")]
    # A state saved by an agent of another geometry (MLP width, ensemble, action or state dimension, std leaves) is refused whole: a leaf
    # that does not depend on the differing dimension would otherwise be overwritten before the first mismatch is met
    counts = getattr(core, "leaves", {})
    for section, leaf, v in todo:
        have, got = counts.get(leaf), int(np.size(v))
        if have is not None and have != got:
            raise ValueError(f"{section}: leaf '{leaf}' has {have} elements in this agent, the state holds {got} "
                             f"(shape {tuple(np.shape(v))}); nothing was loaded")
    for section, leaf, v in todo:
        core.set(section, leaf, v)
    if sd.get("step") is not None:
        core.step = int(np.asarray(sd["step"]))
    if restore_rng:
        if sd.get("rng") is None:
            raise KeyError("restore_rng=True, but the state dict holds no 'rng'")
        agent._rng_key = np.asarray(sd["rng"], np.uint32).reshape(2).copy()
    return agent


# ---------------------------------------------------------------------------------------------------------------------------
# Run state: the agent's checkpoint plus one snapshot directory per replay store (serl_amd/data/snapshot.py), so that a learner
# process can be stopped and continued.  <run_dir>/checkpoint_<step> is the agent (format unchanged);
# <run_dir>/store_<name>_<step>/ is the store `name` at that step.
# ---------------------------------------------------------------------------------------------------------------------------
def _store_dir(run_dir: str, name: str, step: int) -> str:
    return os.path.join(run_dir, f"store_{name}_{step}")


def _store_steps(run_dir: str, name: str):
    ms = (re.fullmatch(r"store_" + re.escape(name) + r"_(\d+)", n) for n in os.listdir(run_dir))
    return sorted(int(m.group(1)) for m in ms if m)


def _link_snapshot(src: str, dst: str) -> bool:
    """Hard-links the files of the snapshot in `src` into the new directory `dst` (and copies its manifest), so that an
    incremental save into `dst` extends it without copying a byte and pruning `src` later frees nothing `dst` needs.  False
    (and `dst` left empty) where there is no readable snapshot or the file system has no hard links."""
    from ..data import snapshot as snap
    try:
        m = snap.read_manifest(src)
        os.makedirs(dst, exist_ok=True)
        for e in [m["valid"]] + m["segments"]:
            if not os.path.exists(os.path.join(dst, e["file"])):
                os.link(os.path.join(src, e["file"]), os.path.join(dst, e["file"]))
        shutil.copyfile(os.path.join(src, snap.MANIFEST), os.path.join(dst, snap.MANIFEST + ".tmp"))
        os.replace(os.path.join(dst, snap.MANIFEST + ".tmp"), os.path.join(dst, snap.MANIFEST))
        return True
    except (ValueError, OSError):
        shutil.rmtree(dst, ignore_errors=True)
        return False


def _complete_steps(run_dir: str):
    """steps that have a `checkpoint_<step>` file: only these were saved to the end"""
    ms = (re.fullmatch(r"checkpoint_(\d+)", n) for n in os.listdir(run_dir))
    return sorted(int(m.group(1)) for m in ms if m)


def save_run(run_dir: str, agent, stores: dict, step: int, keep: int = 1) -> str:
    """Saves the agent (`checkpoint_<step>`, as save_checkpoint) and every store of `stores` ({name: data store}) into `run_dir`.
    The checkpoint file is written LAST: a step is COMPLETE once it exists.  A store's snapshot extends the one of the latest
    complete earlier step where there is one (only the slots written since are copied out of HBM and written); store directories
    of steps without a checkpoint file -- a save that died, whose slots a resumed run never wrote -- are removed first and never
    extended.  A step's directory is built under a temporary name and renamed, so saving a complete step again keeps its old
    snapshot until the new one is whole.  The `keep` most recent steps stay, as for checkpoints.  `run_dir` belongs to ONE run:
    its stores' history is what the incremental saves extend, and nothing else may write `checkpoint_<n>` files into it.  Call
    it from the learner thread between updates; inserts from other threads wait only while a store's slots are copied to host
    memory."""
    os.makedirs(run_dir, exist_ok=True)
    for name in stores:
        if not re.fullmatch(r"[A-Za-z0-9._-]+", name):
            raise ValueError(f"store name {name!r}: letters, digits, '.', '_' and '-' only")
    complete = _complete_steps(run_dir)
    for n in os.listdir(run_dir):
        m = re.fullmatch(r"store_.+_(\d+)(\.tmp)?", n)
        if m and (m.group(2) or int(m.group(1)) not in complete):
            shutil.rmtree(os.path.join(run_dir, n), ignore_errors=True)
    earlier = [s for s in complete if s < step]
    for name, store in stores.items():
        dst = _store_dir(run_dir, name, step)
        tmp = dst + ".tmp"
        linked = bool(earlier) and _link_snapshot(_store_dir(run_dir, name, earlier[-1]), tmp)
        store.save_snapshot(tmp, incremental=linked)
        if os.path.exists(dst):
            shutil.rmtree(dst)
        os.rename(tmp, dst)
    path = save_checkpoint(run_dir, agent, step, keep=keep, overwrite=True)
    kept = set(_complete_steps(run_dir))
    for name in stores:
        for s in _store_steps(run_dir, name):
            if s not in kept:
                shutil.rmtree(_store_dir(run_dir, name, s), ignore_errors=True)
    return path


def restore_run(run_dir: str, agent, stores: dict, step: Optional[int] = None) -> int:
    """Restores what save_run wrote into an agent and stores constructed as for the original run (same configuration and
    geometry), `state.rng` and the stores' sampler states included, and returns the step: the given `step`, or the newest
    complete step whose store snapshots all check (a newer one that does not is passed over).  Every snapshot -- manifest,
    geometry against its store, length and checksum of every file -- is checked before anything is loaded: ValueError (naming
    the bad file) leaves agent and stores untouched."""
    if not os.path.isdir(run_dir):
        raise FileNotFoundError(f"no checkpoint_<step> file in {run_dir}")
    candidates = [step] if step is not None else _complete_steps(run_dir)[::-1]
    if not candidates or (step is not None and not os.path.isfile(os.path.join(run_dir, f"checkpoint_{step}"))):
        raise FileNotFoundError(f"no checkpoint_<step> file in {run_dir}" if step is None else os.path.join(run_dir, f"checkpoint_{step}"))
    first_error = None
    for s in candidates:
        try:
            manifests = {name: store.check_snapshot(_store_dir(run_dir, name, s)) for name, store in stores.items()}
        except ValueError as e:
            first_error = first_error or e
            continue
        restore_checkpoint(os.path.join(run_dir, f"checkpoint_{s}"), agent, restore_rng=True)
        for name, store in stores.items():
            store.restore_snapshot(_store_dir(run_dir, name, s), manifest=manifests[name])
        return s
    raise first_error
