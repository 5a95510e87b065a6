"""CPU: the callers of batch_insert, against fake stores that record their calls -- populate_data_store and
populate_data_store_with_z_axis_only feed a store with batch_insert in chunks of 256 (and a store without one per transition),
ReplicatedDataStore._apply_through hands each batch boundary's transitions to the replica's batch_insert together and in order."""
import pickle

import numpy as np

from serl_amd.data.data_store import populate_data_store, populate_data_store_with_z_axis_only
from serl_amd.data.replicated import ReplicatedDataStore


class InsertOnly:
    def __init__(self):
        self.calls, self.items = [], []

    def insert(self, d):
        self.calls.append(("insert", 1))
        self.items.append(d)

    def __len__(self):
        return len(self.items)


class Batching(InsertOnly):
    def batch_insert(self, batch):
        batch = list(batch)
        self.calls.append(("batch_insert", len(batch)))
        self.items.extend(batch)


def _demos(tmp_path, n, D=12):
    trs = [{"observations": {"state": np.full((1, D), k, np.float32)}, "next_observations": {"state": np.full((1, D), k + 0.5, np.float32)},
            "actions": np.zeros(2, np.float32), "rewards": float(k), "masks": 1.0, "dones": False} for k in range(n)]
    paths = [str(tmp_path / "a.pkl"), str(tmp_path / "b.pkl")]
    for path, part in zip(paths, (trs[:n // 3], trs[n // 3:])):
        with open(path, "wb") as f:
            pickle.dump(part, f)
    return trs, paths


def test_populate_data_store_uses_batch_insert_in_chunks_of_256(tmp_path, capsys):
    trs, paths = _demos(tmp_path, 600)
    b, a = Batching(), InsertOnly()
    assert populate_data_store(b, paths) is b and populate_data_store(a, paths) is a
    assert capsys.readouterr().out == "Loaded 600 transitions.\n" * 2
    assert b.calls == [("batch_insert", 256), ("batch_insert", 256), ("batch_insert", 88)]      # chunks run across the files
    assert a.calls == [("insert", 1)] * 600
    assert [d["rewards"] for d in b.items] == [d["rewards"] for d in a.items] == [float(k) for k in range(600)]


def test_populate_with_z_axis_only_uses_batch_insert(tmp_path, capsys):
    trs, paths = _demos(tmp_path, 300)
    b, a = Batching(), InsertOnly()
    populate_data_store_with_z_axis_only(b, paths)
    populate_data_store_with_z_axis_only(a, paths)
    assert capsys.readouterr().out == "Loaded 300 transitions.\n" * 2
    assert b.calls == [("batch_insert", 256), ("batch_insert", 44)] and a.calls == [("insert", 1)] * 300
    for x, y, tr in zip(b.items, a.items, trs):
        for side in ("observations", "next_observations"):
            assert x[side]["state"].shape == (1, 12 - 5) and (x[side]["state"] == y[side]["state"]).all()
            assert tr[side]["state"].shape == (1, 12)       # the caller's transitions are not modified
        assert x["rewards"] == y["rewards"] == tr["rewards"]


def test_replicated_store_applies_a_boundary_as_one_batch():
    for replica, want in ((Batching(), [("batch_insert", 3), ("batch_insert", 2)]), (InsertOnly(), [("insert", 1)] * 5)):
        r = ReplicatedDataStore(replica, rank=0, world=1, lag=0)
        for k in range(3):
            r.insert({"k": k})
        r.step_barrier()
        r.step_barrier()            # an empty boundary: no call
        r.batch_insert([{"k": 3}, {"k": 4}])
        r.flush()
        assert replica.calls == want and [d["k"] for d in replica.items] == list(range(5))
        r.close()
