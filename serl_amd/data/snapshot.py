"""File form of a replay-store snapshot (run resume).  Pure functions over numpy arrays: nothing here
touches the GPU or the C library -- `save_snapshot` / `restore_snapshot` of serl_amd/data/data_store.py move the arrays
between HBM and the host and call these.

A snapshot is a DIRECTORY:

    manifest.json            format version, geometry, ring bookkeeping, the sampler's PCG64 state (decimal strings), and the list of
                             the files below with their byte length and zlib.crc32
    valid-<count>-<crc>.u8   the whole valid mask, u8[capacity] -- rewritten at every save (an insert changes the mask of slots
                             other than the one it writes)
    seg-<first>-<n>-<crc>.bin  one segment: the n slots written by slot writes first .. first + n - 1 (ring slots first % capacity
                             onwards, in write order): frames u8[n][H][W][C] of camera 0, of camera 1, ..., then records f32[n][rec_len]

A full save holds one segment (the min(count, capacity) live slots); an incremental save appends one with the slots written
since the manifest's count.  Restoring applies the segments in order, so a later segment overwrites the slots it shares with an
earlier one; segments whose slots are all covered by later ones are dropped from the list.

Every file is written under a temporary name and `os.replace`d; a file's name carries its checksum, so a name is never reused
for other contents; the manifest goes last and files it no longer lists are removed after it.  A save that dies anywhere leaves
the previous manifest and every file it lists in place.
"""
from __future__ import annotations

import json
import os
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

FORMAT_VERSION = 1
MANIFEST = "manifest.json"
GEOMETRY_KEYS = ("capacity", "n_cam", "H", "W", "C", "T", "S", "A", "rec_len")
_CHUNK = 1 << 24


def frame_bytes(geometry: dict) -> int:
    return int(geometry["H"]) * int(geometry["W"]) * int(geometry["C"])


def segment_nbytes(geometry: dict, n_slots: int) -> int:
    return int(n_slots) * (int(geometry["n_cam"]) * frame_bytes(geometry) + 4 * int(geometry["rec_len"]))


def _write_file(directory: str, stem: str, suffix: str, arrays: Sequence[np.ndarray]) -> dict:
    """Writes the arrays' bytes back to back as <stem>-<crc32><suffix> (through a temporary name) -> {file, bytes, crc32}."""
    tmp = os.path.join(directory, f"{stem}{suffix}.tmp")
    crc, n = 0, 0
    with open(tmp, "wb") as f:
        for a in arrays:
            buf = memoryview(np.ascontiguousarray(a)).cast("B")
            for o in range(0, len(buf), _CHUNK):
                piece = buf[o:o + _CHUNK]
                crc = zlib.crc32(piece, crc)
                f.write(piece)
            n += len(buf)
        f.flush()
        os.fsync(f.fileno())
    name = f"{stem}-{crc:08x}{suffix}"
    os.replace(tmp, os.path.join(directory, name))
    return {"file": name, "bytes": n, "crc32": crc}


def _prune(segments: List[dict], capacity: int) -> List[dict]:
    """Drops the leading segments whose slots later segments overwrite completely (later ones hold >= capacity slots)."""
    later, keep = 0, []
    for seg in reversed(segments):
        if later >= capacity:
            break
        keep.append(seg)
        later += seg["n_slots"]
    return keep[::-1]


def stage_snapshot(path: str, geometry: dict, state: dict, valid: np.ndarray, first_count: int,
                   frames: Sequence[np.ndarray], records: np.ndarray, base: Optional[dict] = None) -> dict:
    """Writes the valid mask and one segment (the slots written by slot writes first_count .. state["count"] - 1) into `path`
    and returns the manifest that `commit_snapshot` makes current.  `base`: the manifest this save extends (incremental; its
    count must be first_count), or None for a full save."""
    os.makedirs(path, exist_ok=True)
    geometry = {k: int(geometry[k]) for k in GEOMETRY_KEYS}
    cap, count = geometry["capacity"], int(state["count"])
    n = count - int(first_count)
    if not 0 <= n <= cap:
        raise ValueError(f"a segment holds 0..{cap} slots, not {n}")
    if base is not None and (int(base["count"]) != first_count or base["geometry"] != geometry):
        raise ValueError(f"{os.path.join(path, MANIFEST)}: cannot extend it from count {first_count} at this geometry")
    if base is None and first_count != max(0, count - cap):
        raise ValueError(f"a full save starts at count {max(0, count - cap)}, not {first_count}")
    valid = np.ascontiguousarray(valid, dtype=np.uint8)
    records = np.ascontiguousarray(records, dtype=np.float32)
    frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    if valid.size != cap or len(frames) != geometry["n_cam"] or records.size != n * geometry["rec_len"] \
            or any(f.size != n * frame_bytes(geometry) for f in frames):
        raise ValueError("arrays do not have the geometry's sizes")
    segments = list(base["segments"]) if base is not None else []
    if n > 0:
        entry = _write_file(path, f"seg-{first_count:012d}-{n}", ".bin", list(frames) + [records])
        entry.update(first_count=int(first_count), slot_begin=int(first_count % cap), n_slots=int(n))
        segments.append(entry)
    manifest = {"format": FORMAT_VERSION, "geometry": geometry,
                "size": int(state["size"]), "insert_index": int(state["insert_index"]), "count": count, "first": bool(state["first"]),
                "rng": {"state": str(int(state["rng"]["state"])), "inc": str(int(state["rng"]["inc"])),
                        "has_uint32": int(state["rng"]["has_uint32"]), "uinteger": int(state["rng"]["uinteger"])},
                "seed": None if state.get("seed") is None else str(state["seed"]),
                "valid": _write_file(path, f"valid-{count:012d}", ".u8", [valid]),
                "segments": _prune(segments, cap)}
    return manifest


def commit_snapshot(path: str, manifest: dict) -> dict:
    """Makes `manifest` the snapshot of `path` (temporary name + os.replace), then removes the files it does not list."""
    tmp = os.path.join(path, MANIFEST + ".tmp")
    with open(tmp, "w") as f:
        json.dump(manifest, f, indent=1)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(path, MANIFEST))
    listed = {manifest["valid"]["file"]} | {s["file"] for s in manifest["segments"]} | {MANIFEST}
    for name in os.listdir(path):
        if name not in listed and (name.startswith(("seg-", "valid-")) or name.endswith(".tmp")):
            try:
                os.remove(os.path.join(path, name))
            except OSError:
                pass
    return manifest


def write_snapshot(path, geometry, state, valid, first_count, frames, records, base=None) -> dict:
    return commit_snapshot(path, stage_snapshot(path, geometry, state, valid, first_count, frames, records, base))


def read_manifest(path: str, geometry: Optional[dict] = None) -> dict:
    """The manifest of the snapshot directory `path`, checked for form and (when given) against `geometry`.  ValueError names
    the file."""
    mf = os.path.join(path, MANIFEST)
    try:
        with open(mf) as f:
            m = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{mf}: no readable snapshot manifest ({e})") from None
    if not isinstance(m, dict) or m.get("format") != FORMAT_VERSION:
        raise ValueError(f"{mf}: format version {m.get('format') if isinstance(m, dict) else None}, this reader knows {FORMAT_VERSION}")
    try:
        g = {k: int(m["geometry"][k]) for k in GEOMETRY_KEYS}
        cap, count = g["capacity"], int(m["count"])
        ok = int(m["insert_index"]) == count % cap and int(m["size"]) == min(count, cap) and count >= 0
        ok = ok and int(m["valid"]["bytes"]) == cap
        nxt = None
        for s in m["segments"]:
            ok = ok and 0 < int(s["n_slots"]) <= cap and int(s["slot_begin"]) == int(s["first_count"]) % cap
            ok = ok and int(s["bytes"]) == segment_nbytes(g, s["n_slots"]) and (nxt is None or int(s["first_count"]) == nxt)
            nxt = int(s["first_count"]) + int(s["n_slots"])
        if m["segments"]:   # together the segments hold every live slot and end at the manifest's count
            ok = ok and nxt == count and int(m["segments"][0]["first_count"]) <= max(0, count - cap)
        else:
            ok = ok and count == 0
        int(m["rng"]["state"]), int(m["rng"]["inc"]), int(m["rng"]["has_uint32"]), int(m["rng"]["uinteger"])
    except (KeyError, TypeError, ValueError, AttributeError) as e:
        raise ValueError(f"{mf}: malformed manifest ({e!r})") from None
    if not ok:
        raise ValueError(f"{mf}: inconsistent manifest (bookkeeping, segment sizes or segment order)")
    if geometry is not None:
        want = {k: int(geometry[k]) for k in GEOMETRY_KEYS}
        if g != want:
            raise ValueError(f"{mf}: snapshot geometry {g} is not the store's {want}")
    return m


def _check_file(path: str, entry: dict) -> None:
    fn = os.path.join(path, entry["file"])
    if not os.path.isfile(fn):
        raise ValueError(f"{fn}: missing")
    size = os.path.getsize(fn)
    if size != int(entry["bytes"]):
        raise ValueError(f"{fn}: {size} bytes, the manifest lists {entry['bytes']} (truncated?)")
    crc = 0
    with open(fn, "rb") as f:
        while True:
            piece = f.read(_CHUNK)
            if not piece:
                break
            crc = zlib.crc32(piece, crc)
    if crc != int(entry["crc32"]):
        raise ValueError(f"{fn}: crc32 {crc:08x}, the manifest lists {int(entry['crc32']):08x}")


def verify_snapshot(path: str, manifest: dict) -> None:
    """Length and zlib.crc32 of every file the manifest lists; ValueError names the first bad file."""
    _check_file(path, manifest["valid"])
    for s in manifest["segments"]:
        _check_file(path, s)


def load_valid(path: str, manifest: dict) -> np.ndarray:
    fn = os.path.join(path, manifest["valid"]["file"])
    v = np.fromfile(fn, dtype=np.uint8)
    if v.size != manifest["geometry"]["capacity"]:
        raise ValueError(f"{fn}: {v.size} bytes, expected {manifest['geometry']['capacity']}")
    return v


def load_segment(path: str, manifest: dict, seg: dict) -> Tuple[List[np.ndarray], np.ndarray]:
    """-> ([frames u8[n][H][W][C] per camera], records f32[n][rec_len]) of one verified segment."""
    g, n = manifest["geometry"], int(seg["n_slots"])
    fn = os.path.join(path, seg["file"])
    raw = np.fromfile(fn, dtype=np.uint8)
    if raw.size != segment_nbytes(g, n):
        raise ValueError(f"{fn}: {raw.size} bytes, expected {segment_nbytes(g, n)} (truncated?)")
    fb = frame_bytes(g)
    frames = [raw[c * n * fb:(c + 1) * n * fb].reshape(n, g["H"], g["W"], g["C"]) for c in range(g["n_cam"])]
    records = raw[g["n_cam"] * n * fb:].view(np.float32).reshape(n, g["rec_len"])
    return frames, records


def read_snapshot(path: str, geometry: Optional[dict] = None):
    """-> (manifest, valid u8[capacity], [(segment entry, frames, records)]) after every check; ValueError names the bad file."""
    m = read_manifest(path, geometry)
    verify_snapshot(path, m)
    return m, load_valid(path, m), [(s,) + load_segment(path, m, s) for s in m["segments"]]


def assemble(manifest: dict, valid: np.ndarray, segments) -> dict:
    """The ring a restore produces, as host arrays: {"frames": [u8[capacity][H][W][C]], "records": f32[capacity][rec_len],
    "valid": u8[capacity], "written": bool[capacity]} -- the segments applied in order."""
    g = manifest["geometry"]
    cap = g["capacity"]
    frames = [np.zeros((cap, g["H"], g["W"], g["C"]), np.uint8) for _ in range(g["n_cam"])]
    records = np.zeros((cap, g["rec_len"]), np.float32)
    written = np.zeros(cap, bool)
    for seg, fr, rec in segments:
        slots = (int(seg["slot_begin"]) + np.arange(int(seg["n_slots"]))) % cap
        for c in range(g["n_cam"]):
            frames[c][slots] = fr[c]
        records[slots] = rec
        written[slots] = True
    return {"frames": frames, "records": records, "valid": np.asarray(valid, np.uint8), "written": written}
