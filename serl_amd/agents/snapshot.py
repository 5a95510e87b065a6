"""Parameter snapshots: `agent.snapshot()` -> StateSnapshot, a consistent copy of the train state that reaches the host without
stalling the updates (csrc/snapshot.hip; include/serl_mi355.h "Parameter snapshots").

The reference's learner sends `agent.state.params` to the actor every 30 iterations and writes a checkpoint every few thousand
(examples/async_drq_sim/async_drq_sim.py:229,295-307).  `agent.state.params` here is one blocking copy per leaf on the training
thread.  A snapshot is taken in one kernel launch on the stream the updates run on, copied to pinned host memory on a stream of
its own, and read -- by `TrainerServer.publish_network(snapshot)` on its publisher thread, or by `save_checkpoint(dir, snapshot,
step=snapshot.step)` -- as numpy VIEWS into that pinned buffer.  It also knows whether it is finite: the pack kernel counts the
Inf / NaN values it moves, per section.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib_agent import SNAP_BITS, SerlSnapshotMeta
from .flax_tree import export_tree

SECTIONS = tuple(SNAP_BITS)   # ("params", "target_params", "opt_states"): the TrainState fields a snapshot can hold


class _Pinned:
    """`n` read-only floats at `addr` inside a snapshot slot; np.asarray keeps this object, and with it the owner of the
    memory, as the array's base."""

    def __init__(self, addr, n, owner):
        self.__array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (addr, True), "version": 3}
        self._owner = owner


class SnapshotHandle:
    """One serl_snapshot of an AgentCore: a choice of sections and a number of slots.  It holds no reference to the core (the
    core owns it: AgentCore._snapshots, closed by AgentCore.__del__), so an agent that took snapshots is still freed by
    reference counting; the views into its slots keep the CORE alive (`leaf(..., owner)`), and with it this handle."""

    def __init__(self, core, mask: int, slots: int):
        self.mask, self.slots, self.device = mask, slots, core.device
        self.L = core.L
        self._h = C.c_void_p()
        _lib.check(self.L.serl_snapshot_create(core._h, mask, slots, C.byref(self._h)))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.L.serl_snapshot_destroy(h)

    __del__ = close

    def take(self) -> int:
        """on the stream the agent's updates run on: the current stream of its device, what AgentCore passes to every update"""
        slot = C.c_int()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.L.serl_snapshot_take(self._h, stream, C.byref(slot)))
        return slot.value

    def ready(self, slot) -> bool:
        r = self.L.serl_snapshot_ready(self._h, slot)
        if r < 0:
            _lib.check(r)
        return bool(r)

    def wait(self, slot):
        _lib.check(self.L.serl_snapshot_wait(self._h, slot))

    def info(self, slot) -> SerlSnapshotMeta:
        m = SerlSnapshotMeta()
        _lib.check(self.L.serl_snapshot_info(self._h, slot, C.byref(m)))
        return m

    def leaf(self, slot, section, leaf, owner) -> np.ndarray:
        """a read-only view; `owner` (the AgentCore that owns this handle) stays alive as long as the view does.  The leaf of a
        ragged MLP layer is a NON-CONTIGUOUS view of shape (blocks, rows, cols) into its padded storage: a caller that needs flat
        data copies it (np.ascontiguousarray, or the reshape to the leaf's shape that export_tree does)."""
        p, n = C.POINTER(C.c_float)(), C.c_int64()
        _lib.check(self.L.serl_snapshot_leaf(self._h, slot, section.encode(), leaf.encode(), C.byref(p), C.byref(n)))
        v = np.asarray(_Pinned(C.addressof(p.contents), n.value, owner))
        # a leaf of a ragged MLP layer arrives as its zero-padded storage (serl_agent_leaf_layout): the view of its own elements
        blocks, rows, cols, rows_p, ld = owner.leaf_layout(leaf)
        return v if v.size == blocks * rows * cols else v.reshape(blocks, rows_p, ld)[:, :rows, :cols]

    def release(self, slot):
        if self._h:
            _lib.check(self.L.serl_snapshot_release(self._h, slot))


def section_mask(sections) -> int:
    if isinstance(sections, str):
        sections = (sections,)
    bad = [s for s in sections if s not in SNAP_BITS]
    if bad:
        raise KeyError(f"unknown snapshot sections {bad}: a snapshot holds any of {SECTIONS}")
    mask = 0
    for s in sections:
        mask |= SNAP_BITS[s]
    return mask


def take_snapshot(agent, sections=("params",), slots=3) -> "StateSnapshot":
    """agent.snapshot: the handle of (sections, slots) is created at the first call and reused afterwards; the take runs on the
    stream the agent's updates run on (torch.cuda.current_stream of the agent's device)."""
    core, key = agent.core, (section_mask(sections), int(slots))
    if key not in core._snapshots:
        core._snapshots[key] = SnapshotHandle(core, *key)    # (refuses sections == 0 and slots outside 1..4)
    handle = core._snapshots[key]
    return StateSnapshot(agent, handle, handle.take())


class StateSnapshot:
    """The train state as it was when `agent.snapshot()` was called, JaxRLTrainState-shaped like `agent.state`: `step`, `rng`, and
    the trees `params`, `target_params`, `opt_states` of the sections selected -- same paths, shapes and duplication rules as
    `agent.state`, built on first access (which waits for the copy), their leaves read-only numpy views into the snapshot's pinned
    host buffer.  The views are valid until `release()`, which hands the slot back; a tree asked for after it raises.
    `nonfinite` is {section: number of Inf / NaN values}, `finite` whether all are zero.  `snapshot.state` is the snapshot, so that
    serl_amd.utils.checkpoint.save_checkpoint(dir, snapshot, step=snapshot.step) writes the file the agent would have written at
    that step (all three sections selected).  Use it as a context manager to release on exit."""

    def __init__(self, agent, handle: SnapshotHandle, slot: int):
        self._agent, self._handle, self._slot = agent, handle, slot
        self.sections = tuple(s for s in SECTIONS if handle.mask & SNAP_BITS[s])
        self.step = int(agent.core.step)          # (host bookkeeping: the steps enqueued so far, which the snapshot holds)
        self.rng = agent._rng_key.copy()
        self._released = False
        self._info = None
        self._trees = {}

    # ---- JaxRLTrainState surface
    @property
    def state(self):
        return self

    @property
    def params(self):
        return self._tree("params")

    @property
    def target_params(self):
        return self._tree("target_params")

    @property
    def opt_states(self):
        return self._tree("opt_states")

    # ---- the copy
    def ready(self) -> bool:
        """has the copy reached the host?  (never blocks)"""
        self._check_live("ready()")
        return self._handle.ready(self._slot)

    def wait(self):
        """blocks the calling thread until the copy has reached the host; the updates behind the take do not wait for it"""
        self._check_live("wait()")
        self._handle.wait(self._slot)
        return self

    @property
    def info(self) -> SerlSnapshotMeta:
        if self._info is None:
            self.wait()
            self._info = self._handle.info(self._slot)
        return self._info

    @property
    def nonfinite(self) -> dict:
        m = self.info
        return {s: int(m.nonfinite[SECTIONS.index(s)]) for s in self.sections}

    @property
    def finite(self) -> bool:
        return not any(self.nonfinite.values())

    @property
    def nbytes(self) -> int:
        return int(self.info.bytes)

    def release(self):
        """hands the slot back without waiting for anything (idempotent); the trees' views are invalid from here on, `step`, `rng`
        and -- if they were read before -- the non-finite counts stay"""
        if not self._released:
            self._released = True
            self._trees = {}
            self._handle.release(self._slot)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            if not getattr(self, "_released", True):
                self._released = True
                self._handle.release(self._slot)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    # ---- trees
    def _check_live(self, what):
        if self._released:
            raise RuntimeError(f"{what} on a released snapshot (step {self.step}): its slot may hold another state by now")

    def _get(self, section, leaf):
        return self._handle.leaf(self._slot, section, leaf, self._agent.core)

    def _export(self, section):
        return export_tree(self._agent.core, section, self._agent.image_keys, get=self._get)

    def _tree(self, name):
        self._check_live(f"'{name}'")
        if name not in self.sections:
            raise KeyError(f"'{name}' is not in this snapshot: it holds {self.sections} (agent.snapshot(sections=...))")
        if name not in self._trees:
            self.wait()
            if name == "opt_states":
                from .drq import opt_states_tree
                self._trees[name] = opt_states_tree(self._agent, self.step, self._export)
            else:
                self._trees[name] = self._export(name)
        return self._trees[name]
