"""CPU (gloo, world_size 2): DataParallelLearner's label phase (serl_amd/parallel.py; vice.py:546,594,609) with a NumPy stand-in for
the HIP core -- every rank labels its own rows after the slot is selected and before the critic phase, in every call, and
vice_rewards() is the mean label over the GLOBAL batch; a core without a classifier is never asked to label; the trunk farm refuses."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from serl_amd.parallel import DataParallelLearner, TrunkFarmLearner
from test_parallel_cpu import FakeBuffer, FakeCore, _free_port, _tagged_gather


class LabelCore(FakeCore):
    """label of a sample = (its id is a multiple of 3); records the order of the phases"""
    device = "cpu"

    def __init__(self, attached=True):
        super().__init__()
        self.reward_classifier = object() if attached else None
        self.events, self.labels = [], None

    def select_slot(self, slot):
        super().select_slot(slot)
        self.events.append("select")
        self.labels = None

    def label_rewards(self):
        assert self.reward_classifier is not None
        self.events.append("label")
        self.labels = (self.batch["ids"] % 3 == 0).astype(np.float32)

    def critic_grads(self, *a, **kw):
        self.events.append("critic")
        assert self.labels is not None or self.reward_classifier is None, "critic phase in front of the label phase"
        super().critic_grads(*a, **kw)

    def read_reward_labels(self):
        return self.labels, self.labels, float(self.labels.mean())


def _learner(rank, world, attached=True):
    bufs = [FakeBuffer(500, 0), FakeBuffer(60, 1)]
    core = LabelCore(attached)
    return core, DataParallelLearner(core, _tagged_gather(bufs), bufs, [12, 12], rank, world,
                                     all_reduce=(lambda t: dist.all_reduce(t)) if world > 1 else None, seed=3)


def _run(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    core, lr = _learner(rank, world)
    means = []
    for _ in range(2):
        lr.update_critics()
        lr.update_high_utd()
        means.append((lr.vice_rewards(), float(core.labels.mean()), len(core.labels)))
    out[rank] = (means, list(core.events))
    dist.destroy_process_group()


def test_two_ranks_label_their_rows_and_report_the_global_mean():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_run, args=(world, port, out), nprocs=world, join=True)
    core, lr = _learner(0, 1)
    for it in range(2):
        lr.update_critics()
        lr.update_high_utd()
        want = lr.vice_rewards()
        assert len(core.labels) == 24 and want == float(core.labels.mean())
        (g0, l0, n0), (g1, l1, n1) = out[0][0][it], out[1][0][it]
        assert n0 == n1 == 12
        assert abs(g0 - want) < 1e-6 and g0 == g1               # both ranks hold the global mean ...
        assert abs(0.5 * (l0 + l1) - want) < 1e-6               # ... of their local means
    for r in range(2):
        assert out[r][1] == ["select", "label", "critic"] * 4
    assert core.events == ["select", "label", "critic"] * 4


def test_a_core_without_a_classifier_is_not_asked_to_label():
    core, lr = _learner(0, 1, attached=False)
    lr.update_critics()
    lr.update_high_utd()
    assert core.events == ["select", "critic"] * 2


def test_the_trunk_farm_refuses_an_attached_core():
    with pytest.raises(NotImplementedError, match="trunk farm"):
        TrunkFarmLearner(LabelCore(), None, [], [8], rank=0, world=2)
