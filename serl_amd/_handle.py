"""Python side of the library's handles (serl_agent, serl_bc, serl_classifier) and of their lazy info dicts."""
from __future__ import annotations

import ctypes as C
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib


class Handle:
    """Owns one `<prefix>_create` handle: its leaf table, host copies of one leaf and the destroy.  A subclass sets
    `prefix` and `device` (the cuda device whose current stream `_stream` gives)."""

    prefix = ""

    def __init__(self, cfg):
        self.L = _lib.lib()
        self._h = C.c_void_p()
        _lib.check(self._create(cfg))
        self._counts, self._trainable = {}, {}   # leaf -> element count / trainable (where leaf_info reports it)
        leaf_info = self._fn("leaf_info")
        name, cnt, tr = C.create_string_buffer(128), C.c_int64(), C.c_int()
        flag = (C.byref(tr),) if len(leaf_info.argtypes) == 6 else ()   # serl_bc_leaf_info's trailing int* trainable
        for i in range(self._fn("num_leaves")(self._h)):
            _lib.check(leaf_info(self._h, i, name, 128, C.byref(cnt), *flag))
            self._counts[name.value.decode()] = cnt.value
            if flag:
                self._trainable[name.value.decode()] = bool(tr.value)

    def _create(self, cfg):
        """<prefix>_create(cfg, &handle) -> status; a subclass with another constructor overrides it"""
        return self._fn("create")(C.byref(cfg), C.byref(self._h))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._fn("destroy")(h)

    def _fn(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _leaf_call(self, op, section, leaf, data, count):
        """<prefix>_set / _get (handle, section, leaf, host data, count) -> status"""
        return self._fn(op)(self._h, section.encode(), leaf.encode(), data, count)

    def set(self, section: str, leaf: str, value):
        v = np.ascontiguousarray(np.asarray(value, np.float32).reshape(-1))
        _lib.check(self._leaf_call("set", section, leaf, v.ctypes.data, v.size))

    def get(self, section: str, leaf: str) -> np.ndarray:
        out = np.empty(self._counts[leaf], np.float32)
        _lib.check(self._leaf_call("get", section, leaf, out.ctypes.data, out.size))
        return out


class LazyInfo(Mapping):
    """The info dict of an update, read from the device on first access (no host synchronisation per step): `_read()`
    gives it once."""

    _val = None

    def resolve(self) -> dict:
        if self._val is None:
            self._val = self._read()
        return self._val

    def __getitem__(self, k):
        return self.resolve()[k]

    def __iter__(self):
        return iter(self.resolve())

    def __len__(self):
        return len(self.resolve())

    def __repr__(self):
        return repr(self.resolve())
