"""ctypes binding of libserl_mi355.so (the C ABI declared in include/serl_mi355.h).

The product path has NO CPU fallback: if the shared library is missing this module raises at
import of the symbols, and every op raises SerlError on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SERL_MI355_LIB: load another build of the same ABI (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("SERL_MI355_LIB") or os.path.join(_HERE, "lib", "libserl_mi355.so")

MAX_CAMS = 4
MAX_BUFFERS = 2


class SerlError(RuntimeError):
    status = None     # the library's status code (SERL_ERR_*) where the error came from a call of it


class SerlBatch(C.Structure):
    _fields_ = [
        ("batch", C.c_int), ("n_cam", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
        ("state_dim", C.c_int), ("act_dim", C.c_int),
        ("frames", C.c_void_p), ("state", C.c_void_p), ("action", C.c_void_p),
        ("reward", C.c_void_p), ("mask", C.c_void_p), ("done", C.c_void_p),
        ("num_stack", C.c_int),   # T, frames per observation; 0 = 1
    ]


class SerlRbMeta(C.Structure):   # serl_rb_meta
    _fields_ = [
        ("capacity", C.c_int64),
        ("n_cam", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("S", C.c_int32),
        ("A", C.c_int32), ("rec_len", C.c_int32),
        ("size", C.c_int64), ("insert_index", C.c_int64), ("insert_count", C.c_int64),
        ("first", C.c_int32), ("rng_seeded", C.c_int32),
        ("rng_state_inc", C.c_uint64 * 4),
        ("rng_has_uint32", C.c_int32), ("rng_uinteger", C.c_uint32),
    ]


vp, i32, i64, u64, u32, f32, P = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_float, C.POINTER

# function -> argtypes; every function returns an int status unless RESTYPES says otherwise.  The agent, BC and classifier
# handles are declared in _lib_agent.py; tests/test_bindings.py checks both tables against include/serl_mi355.h.
SIGNATURES = {
    "serl_last_error": [],
    "serl_version": [],
    "serl_device_count": [],
    "serl_rb_create": [i32, i64, i32, i32, i32, i32, i32, i32, i32, P(vp)],
    "serl_rb_destroy": [vp],
    "serl_rb_seed": [vp, u64, u64, u64, u64, i32, u32],
    "serl_rb_rng_state": [vp, P(u64), P(i32), P(u32)],
    "serl_rb_insert": [vp, P(vp), P(vp), vp, vp, vp, f32, f32, i32],
    "serl_rb_insert_batch": [vp, i32, P(vp), P(vp), vp, vp, vp, vp, vp, vp],
    "serl_rb_insert_stats": [vp, P(i64)],
    "serl_rb_len": [vp],
    "serl_rb_insert_index": [vp],
    "serl_rb_valid_mask": [vp, vp],
    "serl_rb_insert_count": [vp],
    # snapshot of a store (run resume; serl_amd/data/data_store.py save_snapshot / restore_snapshot)
    "serl_rb_export_meta": [vp, P(SerlRbMeta)],
    "serl_rb_export_slots": [vp, i64, i64, P(vp), vp, vp],
    "serl_rb_import_meta": [vp, P(SerlRbMeta)],
    "serl_rb_import_slots": [vp, i64, i64, P(vp), vp, vp],
    "serl_rb_sample_indices": [vp, i32, vp],
    "serl_rb_gather_packed": [vp, vp, i32, P(vp), vp, vp, vp, vp, vp, vp, vp],
    "serl_rb_gather_crop": [P(vp), i32, P(vp), P(i32), vp, vp, P(SerlBatch), vp],
    "serl_crop_packed": [i32, P(vp), i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "serl_crop_packed_stacked": [i32, P(vp), i32, i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "serl_profile_enable": [i32],
    "serl_profile_reset": [],
    "serl_profile_read": [i32, vp, vp, vp, P(i32)],
    # JAX's PRNG (csrc/jaxrng.hip; serl_amd/jaxrng.py)
    "serl_jax_prngkey": [u64, P(u32)],
    "serl_jax_split": [P(u32), i32, P(u32)],
    "serl_jax_fold_in": [P(u32), u32, P(u32)],
    "serl_jax_random_bits": [P(u32), i64, P(u32)],
    "serl_jax_randint": [P(u32), i64, i32, i32, P(i32)],
    "serl_jax_normal_host": [P(u32), i64, P(f32)],
    "serl_jax_crop_offsets": [P(u32), i32, i32, P(i32)],
    "serl_jax_update_keys": [P(u32), i32, i32, i32, i32, vp],
    "serl_jax_update_keys_dropout": [P(u32), i32, i32, i32, i32, i32, vp, vp],
    "serl_jax_fill": [i32, vp, i32, vp],
    "serl_jax_init_fill": [i32, vp, i32, vp],
    "serl_jax_init_host": [vp],
}
RESTYPES = {"serl_last_error": C.c_char_p, "serl_rb_len": i64, "serl_rb_insert_index": i64, "serl_rb_insert_count": i64}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SerlError(
                f"{LIB_PATH} not found: build it with `python -m serl_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        from . import _lib_agent
        L = C.CDLL(LIB_PATH)
        for sigs, restypes in ((SIGNATURES, RESTYPES), (_lib_agent.SIGNATURES, _lib_agent.RESTYPES)):
            for name, args in sigs.items():
                fn = getattr(L, name)
                fn.argtypes, fn.restype = args, restypes.get(name, i32)
        _lib = L
    return _lib


def check(status: int):
    if status != 0:
        msg = lib().serl_last_error()
        e = SerlError(f"libserl_mi355 status {status}: {msg.decode() if msg else '?'}")
        e.status = status
        raise e


def profile_read(max_entries=64):
    """-> {tag: (total_ms, count)} of the instrumented kernels since the last reset."""
    import numpy as np
    names = C.create_string_buffer(max_entries * 64)
    ms = np.zeros(max_entries, np.float64)
    cnt = np.zeros(max_entries, np.int64)
    n = C.c_int()
    check(lib().serl_profile_read(max_entries, C.cast(names, C.c_void_p), ms.ctypes.data, cnt.ctypes.data, C.byref(n)))
    out = {}
    for i in range(n.value):
        tag = names.raw[i * 64:(i + 1) * 64].split(b"\0")[0].decode()
        out[tag] = (float(ms[i]), int(cnt[i]))
    return out


def exported_symbols():
    """{name: parameter count} of every function include/serl_mi355.h declares (parsed), for the ABI tests."""
    import re
    hdr = os.path.join(_HERE, "..", "include", "serl_mi355.h")
    txt = open(hdr).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(serl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out
