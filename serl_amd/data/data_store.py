"""HBM-resident replay buffer with the reference's data-store interface.

Mirrors (same names, argument meaning and error behaviour):
  serl_launcher/data/memory_efficient_replay_buffer.py:12-164  MemoryEfficientReplayBuffer
  serl_launcher/data/replay_buffer.py:77-90                    get_iterator (prefetch queue)
  serl_launcher/data/data_store.py:83-144                      MemoryEfficientReplayBufferDataStore
  serl_launcher/data/dataset.py:66-74                          seed / np_random
  serl_launcher/utils/train_utils.py:16-31                     concat_batches
  serl_launcher/data/data_store.py:147-196                     populate_data_store, populate_data_store_with_z_axis_only

Storage and sampling live in libserl_mi355.so (serl_amd/csrc/replay.hip); this file only adapts
Python dicts to the C ABI.  There is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import itertools
import threading
from typing import Iterable, Optional

import numpy as np
import torch

from .. import _lib
from . import snapshot as _snap
from ..transport.endpoint import DataStoreBase


def _space_shape(space):
    return tuple(space.shape)


class LazyBatch:
    """A sampled-but-not-yet-gathered batch: (buffer, slot indices) parts in concat order.

    The agent's update turns it into device tensors with ONE fused gather+concat+unpack+crop
    kernel (serl_rb_gather_crop).  `materialize()` gives the reference's packed dict instead.
    """

    def __init__(self, parts, peek_next=None):
        self.parts = list(parts)  # [(buffer, np.int64[n])]
        # peek_next() -> the LazyBatch the iterator will yield next (already sampled by its prefetch queue), or None.
        # The agent uses it to run gather + crop + frozen trunk of the NEXT batch on a second stream under the update
        # of this one (the reference's iterator prefetches two batches to the device for the same reason).
        self.peek_next = peek_next

    @property
    def batch_size(self):
        return sum(len(ix) for _, ix in self.parts)

    @property
    def num_stack(self):
        """T, frames per observation of the stores the batch was drawn from"""
        return int(getattr(self.parts[0][0], "_num_stack", 1) or 1)

    def materialize(self):
        out = None
        for buf, ix in self.parts:
            d = buf.gather(ix)
            out = d if out is None else concat_batches(out, d, axis=0)
        return out


def _after(queue, me):
    """The batch the iterator yields after `me` if it is already in the prefetch queue."""
    return queue[0] if queue and queue[0] is not me else (queue[1] if len(queue) > 1 and queue[0] is me else None)


def concat_batches(offline_batch, online_batch, axis=1):
    """train_utils.py:16-31 (first argument first).  Works on dict batches of torch tensors and
    on LazyBatch (axis must be 0 there)."""
    if isinstance(offline_batch, LazyBatch) or isinstance(online_batch, LazyBatch):
        assert isinstance(offline_batch, LazyBatch) and isinstance(online_batch, LazyBatch)
        assert axis == 0, "lazy batches concatenate along the batch axis only"
        a, b = offline_batch, online_batch

        def peek():
            if a.peek_next is None or b.peek_next is None:
                return None
            na, nb = a.peek_next(), b.peek_next()
            if na is None or nb is None:
                return None
            if getattr(peek, "_cache", (None, None, None))[:2] != (id(na), id(nb)):
                peek._cache = (id(na), id(nb), concat_batches(na, nb, axis=0))
            return peek._cache[2]
        return LazyBatch(a.parts + b.parts, peek)
    batch = {}
    for k, v in offline_batch.items():
        if isinstance(v, dict):
            batch[k] = concat_batches(v, online_batch[k], axis=axis)
        else:
            batch[k] = torch.cat((v, online_batch[k]), dim=axis)
    return batch


class MemoryEfficientReplayBufferDataStore(DataStoreBase):
    """Drop-in for the reference class of the same name (data_store.py:83-144), an agentlace `DataStoreBase`: a
    TrainerServer thread may call insert() / batch_insert() while the learner thread samples (the buffer mutex lives in
    libserl_mi355.so)."""

    def __init__(self, observation_space, action_space, capacity: int,
                 image_keys: Iterable[str] = ("image",), rlds_logger=None, device: int = 0):
        if rlds_logger is not None:
            raise NotImplementedError("RLDS logging is outside the MI355X hot path")
        self.pixel_keys = tuple(image_keys)
        spaces = observation_space.spaces
        self._num_stack = None
        for k in self.pixel_keys:
            shp = _space_shape(spaces[k])
            if self._num_stack is None:
                self._num_stack = shp[0]
            else:
                assert self._num_stack == shp[0]
            self._img_shape = shp[1:]
        other = [k for k in spaces.keys() if k not in self.pixel_keys]
        if other != ["state"]:
            raise NotImplementedError(f"non-pixel observation keys must be exactly ['state'], got {other}")
        sshape = _space_shape(spaces["state"])
        assert len(sshape) == 2 and sshape[0] == self._num_stack, sshape
        self._S = sshape[1]
        self._A = _space_shape(action_space)[0]
        self._capacity = int(capacity)
        DataStoreBase.__init__(self, self._capacity)
        self.device = device
        self._torch_device = torch.device("cuda", device)
        H, W, Cc = self._img_shape
        self._h = C.c_void_p()
        _lib.check(_lib.lib().serl_rb_create(device, self._capacity, len(self.pixel_keys), H, W, Cc,
                                             self._num_stack, self._S, self._A, C.byref(self._h)))
        self._np_random = None
        self._seed = None
        self._lock = threading.Lock()   # insert() against the device -> host phase of save_snapshot()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().serl_rb_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    # -- Dataset.seed / np_random (dataset.py:66-74)
    def seed(self, seed: Optional[int] = None) -> list:
        ss = np.random.SeedSequence(seed)
        self._np_random = np.random.Generator(np.random.PCG64(ss))
        self._seed = ss.entropy
        st = self._np_random.bit_generator.state
        s, inc = st["state"]["state"], st["state"]["inc"]
        m = (1 << 64) - 1
        _lib.check(_lib.lib().serl_rb_seed(self._h, s >> 64, s & m, inc >> 64, inc & m,
                                           st["has_uint32"], st["uinteger"]))
        return [self._seed]

    def _ensure_seeded(self):
        if self._seed is None:
            self.seed()  # lazy OS-entropy seed like the reference (dataset.py:66-70)

    def __len__(self) -> int:
        return int(_lib.lib().serl_rb_len(self._h))

    def latest_data_id(self):  # data_store.py:138-140
        return int(_lib.lib().serl_rb_insert_index(self._h))

    def get_latest_data(self, from_id: int):  # data_store.py:142-144
        raise NotImplementedError  # same as the reference

    def valid_mask(self) -> np.ndarray:
        out = np.zeros(self._capacity, np.uint8)
        _lib.check(_lib.lib().serl_rb_valid_mask(self._h, out.ctypes.data))
        return out.astype(bool)

    # -- insert (memory_efficient_replay_buffer.py:53-89; thread-safe, data_store.py:104-106)
    def _checked(self, data_dict):
        """-> (observation frames per camera, next frames per camera, state, next state, action) of one transition as contiguous
        arrays of the store's types, their shapes checked."""
        obs, nobs = data_dict["observations"], data_dict["next_observations"]
        T = self._num_stack
        fo, fn = [], []
        for k in self.pixel_keys:
            a = np.ascontiguousarray(obs[k], dtype=np.uint8)
            b = np.ascontiguousarray(nobs[k], dtype=np.uint8)
            assert a.shape == (T,) + tuple(self._img_shape), (k, a.shape)
            assert b.shape == a.shape, (k, b.shape)
            fo.append(a)
            fn.append(b)
        st = np.ascontiguousarray(obs["state"], dtype=np.float32).reshape(-1)
        nst = np.ascontiguousarray(nobs["state"], dtype=np.float32).reshape(-1)
        act = np.ascontiguousarray(data_dict["actions"], dtype=np.float32).reshape(-1)
        assert st.size == T * self._S and nst.size == T * self._S and act.size == self._A
        return fo, fn, st, nst, act

    def insert(self, data):   # (the reference's data stores name the transition `data`, data_store.py:104)
        fo, fn, st, nst, act = self._checked(data)
        n = len(self.pixel_keys)
        obs_p = (C.c_void_p * n)(*[a.ctypes.data for a in fo]) if n else None
        next_p = (C.c_void_p * n)(*[b.ctypes.data for b in fn]) if n else None
        with self._lock:
            _lib.check(_lib.lib().serl_rb_insert(
                self._h, obs_p, next_p, st.ctypes.data, nst.ctypes.data, act.ctypes.data,
                float(data["rewards"]), float(data["masks"]), int(bool(data["dones"]))))

    def batch_insert(self, batch_data):
        """insert() of every transition of `batch_data`, in order, as ONE library call (serl_rb_insert_batch: one host-to-device
        copy and one kernel launch per 2 MB of slot writes instead of n_cam + 1 copies per slot write) -- what TrainerServer does
        with an actor's message.  Every transition is checked before the first is inserted."""
        batch = list(batch_data)
        if len(batch) <= 1:
            for d in batch:
                self.insert(d)
            return
        checked = [self._checked(d) for d in batch]
        n, n_cam = len(batch), len(self.pixel_keys)
        obs_p = next_p = None
        if n_cam:   # pointer tables straight from each transition's arrays (`checked` keeps them alive): entry i * n_cam + c
            obs_p = (C.c_void_p * (n * n_cam))(*[a.ctypes.data for c in checked for a in c[0]])
            next_p = (C.c_void_p * (n * n_cam))(*[b.ctypes.data for c in checked for b in c[1]])
        st, nst, act = (np.stack([c[j] for c in checked]) for j in (2, 3, 4))
        rew = np.array([float(d["rewards"]) for d in batch], np.float32)
        msk = np.array([float(d["masks"]) for d in batch], np.float32)
        done = np.array([bool(d["dones"]) for d in batch], np.uint8)
        with self._lock:
            _lib.check(_lib.lib().serl_rb_insert_batch(self._h, n, obs_p, next_p, st.ctypes.data, nst.ctypes.data, act.ctypes.data,
                                                       rew.ctypes.data, msk.ctypes.data, done.ctypes.data))

    def insert_stats(self) -> dict:
        """What the inserts into this store have cost so far (serl_rb_insert_stats): transitions inserted, batch_insert library
        calls, host-to-device copies and kernel launches enqueued."""
        out = (C.c_int64 * 4)()
        _lib.check(_lib.lib().serl_rb_insert_stats(self._h, out))
        return dict(zip(("transitions", "batch_calls", "h2d_copies", "launches"), (int(v) for v in out)))

    # -- index draw (memory_efficient_replay_buffer.py:111-122)
    def sample_indices(self, batch_size: int) -> np.ndarray:
        self._ensure_seeded()
        idx = np.empty(batch_size, np.int64)
        _lib.check(_lib.lib().serl_rb_sample_indices(self._h, batch_size, idx.ctypes.data))
        return idx

    # -- gather (memory_efficient_replay_buffer.py:126-164), packed frames on the device
    def gather(self, indx: np.ndarray, stream=None):
        indx = np.ascontiguousarray(indx, dtype=np.int64)   # (stale indices are re-drawn in place by the library)
        if not indx.flags.writeable:
            indx = indx.copy()
        B, T = len(indx), self._num_stack
        H, W, Cc = self._img_shape
        dev = self._torch_device
        frames = {k: torch.empty((B, T + 1, H, W, Cc), dtype=torch.uint8, device=dev) for k in self.pixel_keys}
        st = torch.empty((B, T, self._S), dtype=torch.float32, device=dev)
        nst = torch.empty_like(st)
        act = torch.empty((B, self._A), dtype=torch.float32, device=dev)
        rew = torch.empty((B,), dtype=torch.float32, device=dev)
        msk = torch.empty((B,), dtype=torch.float32, device=dev)
        done = torch.empty((B,), dtype=torch.uint8, device=dev)
        fp = (C.c_void_p * len(self.pixel_keys))(*[frames[k].data_ptr() for k in self.pixel_keys])
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.lib().serl_rb_gather_packed(
            self._h, indx.ctypes.data, B, fp, st.data_ptr(), nst.data_ptr(), act.data_ptr(),
            rew.data_ptr(), msk.data_ptr(), done.data_ptr(), C.c_void_p(s)))
        obs = {"state": st}
        obs.update(frames)
        return {"observations": obs, "next_observations": {"state": nst}, "actions": act,
                "rewards": rew, "masks": msk, "dones": done.bool()}

    def sample(self, batch_size: int, keys=None, indx=None, pack_obs_and_next_obs: bool = False,
               lazy: bool = False):
        if indx is not None:
            raise NotImplementedError()  # memory_efficient_replay_buffer.py:123-124
        if keys is not None:
            raise NotImplementedError("key sub-selection is not used on the hot path")
        idx = self.sample_indices(batch_size)
        if lazy:
            return LazyBatch([(self, idx)])
        batch = self.gather(idx)
        if not pack_obs_and_next_obs:  # memory_efficient_replay_buffer.py:159-162
            for k in self.pixel_keys:
                packed = batch["observations"][k]
                batch["observations"][k] = packed[:, :-1]
                batch["next_observations"][k] = packed[:, 1:]
        return batch

    # -- replay_buffer.py:77-90: depth-`queue_size` prefetch; `device` is accepted and ignored
    # (data never leaves HBM)
    def get_iterator(self, queue_size: int = 2, sample_args: dict = {}, device=None):
        queue = collections.deque()

        def enqueue(n):
            for _ in range(n):
                b = self.sample(**sample_args)
                if isinstance(b, LazyBatch):
                    b.peek_next = lambda me=b: _after(queue, me)
                queue.append(b)

        enqueue(queue_size)
        while queue:
            yield queue.popleft()
            enqueue(1)

    @property
    def handle(self):
        return self._h

    # -- snapshot / restore (run resume; file form: serl_amd/data/snapshot.py)
    def insert_count(self) -> int:
        """Slot writes ever made (serl_rb_insert_count): unlike latest_data_id() it does not wrap."""
        return int(_lib.lib().serl_rb_insert_count(self._h))

    def rng_state(self) -> dict:
        """The sampler's PCG64 in numpy's terms: {"state", "inc", "has_uint32", "uinteger"}."""
        return _meta_state(self._meta())["rng"]

    def _meta(self):
        m = _lib.SerlRbMeta()
        _lib.check(_lib.lib().serl_rb_export_meta(self._h, C.byref(m)))
        return m

    def save_snapshot(self, path: str, incremental: bool = False) -> dict:
        """Writes the store (slots, valid mask, ring bookkeeping, sampler state) into the directory `path` and returns the
        manifest.  incremental=True extends the snapshot already in `path` -- which must be an earlier snapshot of THIS store's
        history -- by one segment holding the slots written since; with no usable snapshot there, or a whole ring of slot writes
        since, it saves everything.  Inserts wait while HBM is copied to host buffers (sampling and gathers go on) and run again
        while the files are written; a save that dies leaves the previous snapshot in `path` readable."""
        self._ensure_seeded()   # a snapshot always carries a generator state
        base = None
        if incremental:
            try:
                base = _snap.read_manifest(path)
            except ValueError:
                base = None
        n_cam = len(self.pixel_keys)
        with self._lock:
            m = self._meta()
            geometry, state = _meta_geometry(m), _meta_state(m)
            count, cap = state["count"], geometry["capacity"]
            if base is not None and base["geometry"] == geometry and 0 <= count - base["count"] < cap:
                first_count = base["count"]
            else:
                base, first_count = None, max(0, count - cap)
            n = count - first_count
            frames = [np.empty((n, m.H, m.W, m.C), np.uint8) for _ in range(n_cam)]
            records = np.empty((n, m.rec_len), np.float32)
            valid = np.empty(cap, np.uint8)
            fp = (C.c_void_p * max(n_cam, 1))(*[f.ctypes.data for f in frames])
            _lib.check(_lib.lib().serl_rb_export_slots(self._h, first_count % cap, n, fp if n_cam else None,
                                                       records.ctypes.data, valid.ctypes.data))
        state["seed"] = self._seed
        return _snap.write_snapshot(path, geometry, state, valid, first_count, frames, records, base)

    def check_snapshot(self, path: str) -> dict:
        """Checks the snapshot in `path` against this store WITHOUT loading anything: the manifest's form and geometry, and the
        length and checksum of every file.  Returns the manifest; ValueError names the bad file."""
        manifest = _snap.read_manifest(path, _meta_geometry(self._meta()))
        _snap.verify_snapshot(path, manifest)
        return manifest

    def restore_snapshot(self, path: str, manifest: Optional[dict] = None) -> dict:
        """Loads the snapshot in `path` into this (already constructed) store of the same geometry and returns its manifest.
        Every file is checked first: a truncated or missing file, a checksum or a geometry mismatch raises ValueError naming the
        file, and the store keeps its contents.  `manifest`: what check_snapshot(path) returned just before (the files are then
        not read a second time for their checksums)."""
        if manifest is None:
            manifest = self.check_snapshot(path)
        valid = _snap.load_valid(path, manifest)
        m = _lib.SerlRbMeta(**{k: manifest["geometry"][k] for k in _snap.GEOMETRY_KEYS})
        m.size, m.insert_index, m.insert_count, m.first = manifest["size"], manifest["insert_index"], manifest["count"], int(manifest["first"])
        s, inc, mask = int(manifest["rng"]["state"]), int(manifest["rng"]["inc"]), (1 << 64) - 1
        m.rng_seeded, m.rng_has_uint32, m.rng_uinteger = 1, manifest["rng"]["has_uint32"], manifest["rng"]["uinteger"]
        m.rng_state_inc[:] = [s >> 64, s & mask, inc >> 64, inc & mask]
        n_cam = len(self.pixel_keys)
        with self._lock:
            _lib.check(_lib.lib().serl_rb_import_meta(self._h, C.byref(m)))
            for seg in manifest["segments"]:
                frames, records = _snap.load_segment(path, manifest, seg)
                fp = (C.c_void_p * max(n_cam, 1))(*[f.ctypes.data for f in frames])
                _lib.check(_lib.lib().serl_rb_import_slots(self._h, seg["slot_begin"], seg["n_slots"], fp if n_cam else None,
                                                           records.ctypes.data, None))
            _lib.check(_lib.lib().serl_rb_import_slots(self._h, 0, 0, None, None, valid.ctypes.data))
        # the generator is the snapshot's: _ensure_seeded() must not draw a fresh OS-entropy seed over it
        self._seed = int(manifest["seed"]) if manifest.get("seed") not in (None, "None") else 0
        self._np_random = np.random.Generator(np.random.PCG64())
        self._np_random.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": s, "inc": inc},
                                               "has_uint32": manifest["rng"]["has_uint32"], "uinteger": manifest["rng"]["uinteger"]}
        return manifest


def _meta_geometry(m) -> dict:
    return {k: int(getattr(m, k)) for k in _snap.GEOMETRY_KEYS}


def _meta_state(m) -> dict:
    st = m.rng_state_inc
    return {"size": int(m.size), "insert_index": int(m.insert_index), "count": int(m.insert_count), "first": bool(m.first),
            "rng": {"state": (st[0] << 64) | st[1], "inc": (st[2] << 64) | st[3], "has_uint32": int(m.rng_has_uint32),
                    "uinteger": int(m.rng_uinteger)}}


class ReplayBufferDataStore(MemoryEfficientReplayBufferDataStore):
    """Drop-in for the reference's plain `ReplayBufferDataStore` (data_store.py:27-80) of flat observations
    (ReplayBuffer, replay_buffer.py:41-75: every inserted slot is valid, `Dataset.sample` draws
    `integers(len, size=B)` with no rejection) -- the store of BASELINE.json configs[0] `async_sac_state_sim`."""

    def __init__(self, observation_space, action_space, capacity: int, rlds_logger=None, device: int = 0):
        if rlds_logger is not None:
            raise NotImplementedError("RLDS logging is outside the MI355X hot path")
        if hasattr(observation_space, "spaces"):
            raise TypeError("ReplayBufferDataStore holds flat (Box) observations; use the memory-efficient store for pixels")
        self.pixel_keys = ()
        self._num_stack = 1
        self._img_shape = (0, 0, 0)
        self._S = int(np.prod(_space_shape(observation_space)))
        self._A = _space_shape(action_space)[0]
        self._capacity = int(capacity)
        DataStoreBase.__init__(self, self._capacity)
        self.device = device
        self._torch_device = torch.device("cuda", device)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().serl_rb_create(device, self._capacity, 0, 0, 0, 0, 1, self._S, self._A, C.byref(self._h)))
        self._np_random = None
        self._seed = None
        self._lock = threading.Lock()   # insert() against the device -> host phase of save_snapshot()

    # insert (replay_buffer.py:71-75 under the data store's lock, data_store.py:44-46), batch_insert and insert_stats are the
    # parent's: a transition of this store has no frames
    def _checked(self, data_dict):
        st = np.ascontiguousarray(data_dict["observations"], dtype=np.float32).reshape(-1)
        nst = np.ascontiguousarray(data_dict["next_observations"], dtype=np.float32).reshape(-1)
        act = np.ascontiguousarray(data_dict["actions"], dtype=np.float32).reshape(-1)
        assert st.size == self._S and nst.size == self._S and act.size == self._A
        return [], [], st, nst, act

    def gather(self, indx: np.ndarray, stream=None):
        indx = np.ascontiguousarray(indx, dtype=np.int64)
        B, dev = len(indx), self._torch_device
        st = torch.empty((B, self._S), dtype=torch.float32, device=dev)
        nst = torch.empty_like(st)
        act = torch.empty((B, self._A), dtype=torch.float32, device=dev)
        rew = torch.empty((B,), dtype=torch.float32, device=dev)
        msk = torch.empty((B,), dtype=torch.float32, device=dev)
        done = torch.empty((B,), dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.lib().serl_rb_gather_packed(
            self._h, indx.ctypes.data, B, None, st.data_ptr(), nst.data_ptr(), act.data_ptr(),
            rew.data_ptr(), msk.data_ptr(), done.data_ptr(), C.c_void_p(s)))
        return {"observations": st, "next_observations": nst, "actions": act, "rewards": rew, "masks": msk,
                "dones": done.bool()}

    def sample(self, batch_size: int, keys=None, indx=None, lazy: bool = False, **kwargs):
        """Dataset.sample (dataset.py:79-102): `indx` may be given (used by `download`)."""
        if keys is not None:
            raise NotImplementedError("key sub-selection is not used on the hot path")
        idx = self.sample_indices(batch_size) if indx is None else np.asarray(indx, np.int64)
        return LazyBatch([(self, idx)]) if lazy else self.gather(idx)


def gather_crop(parts, crop_obs: Optional[np.ndarray], crop_next: Optional[np.ndarray], out, stream=None):
    """Fused K2+K3+K4 into a DeviceBatch `out` (serl_amd.agents.batch.DeviceBatch)."""
    n = len(parts)
    assert 1 <= n <= _lib.MAX_BUFFERS
    rbs = (C.c_void_p * n)(*[p[0].handle.value for p in parts])
    # the library re-draws, IN PLACE, indices whose slot an insert invalidated since they were drawn: pass the callers'
    # own arrays whenever possible so that LazyBatch.parts keep describing the gathered batch
    idxs = [p[1] if (isinstance(p[1], np.ndarray) and p[1].dtype == np.int64 and p[1].flags.c_contiguous and p[1].flags.writeable)
            else np.ascontiguousarray(p[1], dtype=np.int64).copy() for p in parts]
    idp = (C.c_void_p * n)(*[ix.ctypes.data for ix in idxs])
    counts = (C.c_int * n)(*[len(ix) for ix in idxs])
    co = None if crop_obs is None else np.ascontiguousarray(crop_obs, dtype=np.int32)
    cn = None if crop_next is None else np.ascontiguousarray(crop_next, dtype=np.int32)
    dev = parts[0][0]._torch_device
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().serl_rb_gather_crop(
        rbs, n, idp, counts, None if co is None else co.ctypes.data,
        None if cn is None else cn.ctypes.data, C.byref(out.cstruct), C.c_void_p(s)))


def _demo_transitions(demos_path):
    """Transitions of the pickled demonstration files (each file: a list of transition dicts, the format the reference's
    record_demo scripts write).  `demos_path` is a LIST of paths, as at the reference's call sites
    (examples/bc_policy.py:152-156); a single string is accepted as one path instead of being iterated per character."""
    import pickle
    paths = [demos_path] if isinstance(demos_path, (str, bytes)) else list(demos_path)
    for path in paths:
        with open(path, "rb") as f:
            demo = pickle.load(f)
        for transition in demo:
            yield transition


def _insert_in_chunks(data_store, transitions, chunk=256):
    """The transitions go into `data_store` in order: through batch_insert, `chunk` at a time, if the store has one."""
    if not hasattr(data_store, "batch_insert"):
        for transition in transitions:
            data_store.insert(transition)
        return
    it = iter(transitions)
    while True:
        part = list(itertools.islice(it, chunk))
        if not part:
            return
        data_store.batch_insert(part)


def populate_data_store(data_store, demos_path):
    """data_store.py:147-163: insert every transition of the demonstration pickles into `data_store` (any object with
    insert() and __len__: the HBM stores above or a QueuedDataStore) and return it."""
    _insert_in_chunks(data_store, _demo_transitions(demos_path))
    print(f"Loaded {len(data_store)} transitions.")
    return data_store


def _z_axis_only(state: np.ndarray) -> np.ndarray:
    """data_store.py:180-196: drop the x / y Cartesian components of a [T, D] proprio state -- columns 0..3, column 6 and
    columns 10.. are kept (the reference concatenates state[:, :4], state[:, 6][None] and state[:, 10:])."""
    state = np.asarray(state)
    return np.concatenate((state[:, :4], state[:, 6][None, ...], state[:, 10:]), axis=-1)


def populate_data_store_with_z_axis_only(data_store, demos_path):
    """data_store.py:166-196: as populate_data_store, with the x / y coordinates removed from both observations' state
    (the caller's transitions are not modified)."""
    def z_only():
        for transition in _demo_transitions(demos_path):
            t = dict(transition)
            for side in ("observations", "next_observations"):
                t[side] = dict(transition[side])
                t[side]["state"] = _z_axis_only(transition[side]["state"])
            yield t
    _insert_in_chunks(data_store, z_only())
    print(f"Loaded {len(data_store)} transitions.")
    return data_store
