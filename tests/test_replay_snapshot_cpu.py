"""CPU: the file form of a replay-store snapshot (serl_amd/data/snapshot.py) as pure functions over numpy arrays -- round
trips of full and incremental saves, every kind of damage raises ValueError naming the file, and a save that dies before the
manifest rename leaves the previous snapshot readable."""
import json
import os

import numpy as np
import pytest

from serl_amd.data import snapshot as snap

GEOM = dict(capacity=48, n_cam=2, H=32, W=32, C=3, T=1, S=5, A=3, rec_len=2 * 5 + 3 + 3)


class Ring:
    """A host model of the store's ring: slot write number w fills slot w % capacity with bytes / floats derived from w."""

    def __init__(self, geometry=GEOM):
        g = self.g = dict(geometry)
        self.frames = [np.zeros((g["capacity"], g["H"], g["W"], g["C"]), np.uint8) for _ in range(g["n_cam"])]
        self.records = np.zeros((g["capacity"], g["rec_len"]), np.float32)
        self.valid = np.zeros(g["capacity"], np.uint8)
        self.count = 0
        self.rng = np.random.default_rng(5)

    def write(self, n):
        cap = self.g["capacity"]
        for _ in range(n):
            s = self.count % cap
            for c, f in enumerate(self.frames):
                f[s] = self.rng.integers(0, 256, f[s].shape, dtype=np.uint8)
            self.records[s] = self.rng.standard_normal(self.g["rec_len"]).astype(np.float32)
            self.valid[s] = self.count % 3 != 0
            self.valid[(s + 1) % cap] = 0      # an insert touches the mask of ANOTHER slot too
            self.count += 1

    def state(self):
        cap = self.g["capacity"]
        return {"size": min(self.count, cap), "insert_index": self.count % cap, "count": self.count, "first": self.count % 2 == 0,
                "rng": {"state": (1 << 127) + 12345678901234567890 + self.count, "inc": (1 << 100) | 1, "has_uint32": 1, "uinteger": 4000000000},
                "seed": 2 ** 70 + 3}

    def save(self, path, base=None, commit=True):
        cap = self.g["capacity"]
        first = base["count"] if base is not None else max(0, self.count - cap)
        slots = (first + np.arange(self.count - first)) % cap
        m = snap.stage_snapshot(path, self.g, self.state(), self.valid, first, [f[slots] for f in self.frames], self.records[slots], base)
        return snap.commit_snapshot(path, m) if commit else m


def _same(ring, path):
    m, valid, segs = snap.read_snapshot(path, ring.g)
    got = snap.assemble(m, valid, segs)
    cap = ring.g["capacity"]
    live = np.arange(cap) < min(ring.count, cap)
    assert (got["written"] == live).all()
    assert (got["valid"] == ring.valid).all()
    for c in range(ring.g["n_cam"]):
        assert (got["frames"][c][live] == ring.frames[c][live]).all()
    assert got["records"][live].tobytes() == ring.records[live].tobytes()
    st = ring.state()
    assert (m["size"], m["insert_index"], m["count"], m["first"]) == (st["size"], st["insert_index"], st["count"], st["first"])
    assert int(m["rng"]["state"]) == st["rng"]["state"] and int(m["rng"]["inc"]) == st["rng"]["inc"]
    assert (m["rng"]["has_uint32"], m["rng"]["uinteger"], int(m["seed"])) == (1, 4000000000, st["seed"])
    return m


@pytest.mark.parametrize("writes", [0, 30, 48, 72])
def test_full_save_round_trip(tmp_path, writes):
    r = Ring()
    r.write(writes)
    p = str(tmp_path / "snap")
    r.save(p)
    m = _same(r, p)
    assert len(m["segments"]) == (1 if writes else 0)
    assert m["geometry"] == GEOM and m["format"] == snap.FORMAT_VERSION
    for e in [m["valid"]] + m["segments"]:
        assert os.path.getsize(os.path.join(p, e["file"])) == e["bytes"]
    assert sorted(os.listdir(p)) == sorted([snap.MANIFEST, m["valid"]["file"]] + [s["file"] for s in m["segments"]])


def test_incremental_saves_round_trip_and_prune(tmp_path):
    r = Ring()
    p = str(tmp_path / "snap")
    r.write(30)
    m = r.save(p)
    r.write(20)                       # runs over the end of the ring
    m = r.save(p, base=m)
    assert [s["n_slots"] for s in m["segments"]] == [30, 20] and m["segments"][1]["slot_begin"] == 30
    _same(r, p)
    r.write(40)                       # past the first segment's slots: 20 + 40 >= capacity, the first segment is dropped
    m = r.save(p, base=m)
    assert [s["n_slots"] for s in m["segments"]] == [20, 40]
    _same(r, p)
    r.write(0)                        # nothing new: no segment, the small metadata is still rewritten
    m2 = r.save(p, base=m)
    assert m2["segments"] == m["segments"]
    _same(r, p)
    assert sorted(os.listdir(p)) == sorted([snap.MANIFEST, m2["valid"]["file"]] + [s["file"] for s in m2["segments"]])
    # the same ring from one full save
    q = str(tmp_path / "full")
    r.save(q)
    a, b = snap.assemble(*snap.read_snapshot(p)), snap.assemble(*snap.read_snapshot(q))
    assert all((x == y).all() for x, y in zip(a["frames"], b["frames"])) and a["records"].tobytes() == b["records"].tobytes()


def test_single_camera_and_no_camera_geometries(tmp_path):
    for g in (dict(GEOM, n_cam=1, W=48), dict(capacity=50, n_cam=0, H=0, W=0, C=0, T=1, S=4, A=2, rec_len=13)):
        r = Ring(g)
        r.write(70)
        p = str(tmp_path / f"snap{g['n_cam']}")
        r.save(p)
        _same(r, p)


def _saved(tmp_path):
    r = Ring()
    r.write(30)
    p = str(tmp_path / "snap")
    m = r.save(p)
    r.write(20)
    m = r.save(p, base=m)
    return r, p, m


def test_truncated_segment_raises(tmp_path):
    r, p, m = _saved(tmp_path)
    fn = os.path.join(p, m["segments"][1]["file"])
    with open(fn, "r+b") as f:
        f.truncate(m["segments"][1]["bytes"] - 7)
    with pytest.raises(ValueError, match=m["segments"][1]["file"]):
        snap.read_snapshot(p, r.g)


def test_flipped_byte_raises(tmp_path):
    r, p, m = _saved(tmp_path)
    for entry in (m["segments"][0], m["valid"]):
        fn = os.path.join(p, entry["file"])
        raw = bytearray(open(fn, "rb").read())
        raw[len(raw) // 2] ^= 0x10
        open(fn, "wb").write(bytes(raw))
        with pytest.raises(ValueError, match=entry["file"]):
            snap.read_snapshot(p, r.g)
        raw[len(raw) // 2] ^= 0x10
        open(fn, "wb").write(bytes(raw))
    _same(r, p)


def test_missing_segment_raises(tmp_path):
    r, p, m = _saved(tmp_path)
    os.remove(os.path.join(p, m["segments"][0]["file"]))
    with pytest.raises(ValueError, match=m["segments"][0]["file"]):
        snap.read_snapshot(p, r.g)


@pytest.mark.parametrize("change", [{"H": 64}, {"W": 48}, {"capacity": 64}, {"S": 6}, {"n_cam": 1}])
def test_wrong_geometry_raises(tmp_path, change):
    r, p, m = _saved(tmp_path)
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(p, dict(r.g, **change))
    if "S" in change:
        return
    # ... and a manifest edited to another image size, camera count or capacity no longer agrees with its own segment sizes
    m2 = json.load(open(os.path.join(p, snap.MANIFEST)))
    m2["geometry"].update(change)
    json.dump(m2, open(os.path.join(p, snap.MANIFEST), "w"))
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(p)


def test_no_or_malformed_manifest_raises(tmp_path):
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(str(tmp_path / "nothing"))
    r, p, m = _saved(tmp_path)
    open(os.path.join(p, snap.MANIFEST), "w").write("{not json")
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(p)
    bad = dict(m, segments=m["segments"][1:])       # a segment list that does not hold every live slot
    json.dump(bad, open(os.path.join(p, snap.MANIFEST), "w"))
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(p)


def test_save_interrupted_before_the_manifest_rename_reads_as_the_previous_snapshot(tmp_path):
    r, p, m = _saved(tmp_path)
    before = Ring()
    before.write(30)
    before.write(20)                   # == r at its last committed save (same generator seed)
    for full in (False, True):
        r.write(40)
        staged = r.save(p, base=None if full else m, commit=False)       # every file written, the manifest not yet
        json.dump(staged, open(os.path.join(p, snap.MANIFEST + ".tmp"), "w"))   # ... died between write and rename
        assert json.load(open(os.path.join(p, snap.MANIFEST))) == m
        _same(before, p)
        r = Ring()                      # rewind to the committed state for the second variant
        r.write(50)
    # the next complete save clears what the dead ones left behind
    m3 = r.save(p, base=m)
    _same(r, p)
    assert sorted(os.listdir(p)) == sorted([snap.MANIFEST, m3["valid"]["file"]] + [s["file"] for s in m3["segments"]])


@pytest.mark.parametrize("damage", [lambda m: m.update(count="x"), lambda m: m["rng"].update(state="seven"),
                                    lambda m: m["segments"][0].update(n_slots=None), lambda m: m.update(geometry=[1, 2]),
                                    lambda m: m.pop("valid")])
def test_manifest_with_a_bad_field_raises_naming_the_file(tmp_path, damage):
    r, p, m = _saved(tmp_path)
    damage(m)
    json.dump(m, open(os.path.join(p, snap.MANIFEST), "w"))
    with pytest.raises(ValueError, match=snap.MANIFEST):
        snap.read_snapshot(p, r.g)
