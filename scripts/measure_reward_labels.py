"""Cost of reward labelling at the benchmark shape (B = 256, 2 x 128 x 128): the same agent detached, attached on shared
features, attached on its own trunk; median of 3 x 200 update_critics steps each, interleaved, one resident batch."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serl_amd import _lib
from serl_amd.agents.batch import DeviceBatch
from serl_amd.networks.reward_classifier import Classifier
from serl_amd.utils import init as pinit
from serl_amd.utils.launcher import make_drq_agent

KEYS, H, W, S, A, B = ("front", "wrist"), 128, 128, 24, 6, 256
obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in KEYS}
obs["state"] = np.zeros((1, S), np.float32)
agent = make_drq_agent(0, obs, np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained", batch_size=B)
agent.prefetch = False
db = DeviceBatch(B, 2, H, W, 3, S, A, 0)
g = torch.Generator(device="cuda").manual_seed(0)
db.frames.copy_(torch.randint(0, 256, db.frames.shape, dtype=torch.uint8, device="cuda", generator=g))
db.state.normal_(generator=g); db.action.uniform_(-1, 1, generator=g)
db.reward.zero_(); db.mask.fill_(1.0); db.done.zero_()

def classifier(same_trunk):
    c = Classifier(KEYS, H, W, max_batch=B)
    for leaf, v in pinit.init_classifier(2, H, W, 1).items():
        c.set(leaf, v)
    trunk = {k: agent.core.get("params", k) for k in agent.core.leaves if k.startswith("trunk/")} if same_trunk else pinit.init_trunk(seed=99)
    for leaf, v in trunk.items():
        c.set(leaf, v)
    return c

variants = {"detached": None, "features": classifier(True), "frames": classifier(False)}
L = _lib.lib()
res = {k: [] for k in variants}
launches = {}
for rep in range(4):                      # round 0 = warm-up of every variant
    for name, c in variants.items():
        agent.set_reward_classifier(c)
        assert agent.reward_label_mode == (None if c is None else name), agent.reward_label_mode
        for _ in range(10):
            agent.update_critics(db)
        torch.cuda.synchronize()
        n0 = L.serl_debug_chain_launches()
        t0 = time.perf_counter()
        for _ in range(200):
            agent.update_critics(db)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / 200
        launches[name] = (L.serl_debug_chain_launches() - n0) / 200
        if rep:
            res[name].append(ms)
        if c is not None:
            lab, lg = agent.last_reward_labels()
            print(name, "mean label", float(lab.mean()), "logit range", float(lg.min()), float(lg.max()), flush=True)
out = {"shape": "B=256 2x128x128, update_critics, serial, resident batch", "ms_per_step_median_of_3x200": {k: float(np.median(v)) for k, v in res.items()},
       "ms_per_step_all": res, "chain_launches_per_step": launches}
print(json.dumps(out))
