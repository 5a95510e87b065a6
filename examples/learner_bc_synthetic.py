"""The behaviour-cloning loop of the reference's examples/bc_policy.py:152-168 on the MI355X path: demonstrations go into an
HBM replay buffer (populate_data_store), `get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True})` feeds
`agent.update(batch)`, and the loop prints ms per BC step.  For comparison it then times the frozen ResNet-10 trunk pass
over the same n_cam x B observation images alone (what the BC step has to do at least).

    python examples/learner_bc_synthetic.py --steps 200 --batch_size 256

Only the import lines differ from the reference script: make_bc_agent comes from serl_amd.agents.bc (not yet from
serl_amd.utils.launcher) and the demonstrations are synthetic.
"""
import argparse
import itertools
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serl_amd.agents.bc import make_bc_agent  # noqa: E402
from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, populate_data_store  # noqa: E402
from serl_amd.utils.synthetic import transition_stream  # noqa: E402


class _Sp:
    def __init__(self, shape):
        self.shape = shape


class _Obs:
    def __init__(self, keys, H, W, S):
        self.spaces = {k: _Sp((1, H, W, 3)) for k in keys}
        self.spaces["state"] = _Sp((1, S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--demos", type=int, default=2000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--state_dim", type=int, default=24)
    ap.add_argument("--act_dim", type=int, default=6)
    args = ap.parse_args()
    keys, H, W, S, A, B = ("front", "wrist"), args.size, args.size, args.state_dim, args.act_dim, args.batch_size

    # demos as the reference's record_demo scripts write them: a pickled list of transitions
    path = os.path.join(tempfile.mkdtemp(prefix="bc_demos_"), "demos.pkl")
    with open(path, "wb") as f:
        pickle.dump(list(itertools.islice(transition_stream(keys, H, W, 3, 1, S, A, 100, 7), args.demos)), f)
    replay_buffer = MemoryEfficientReplayBufferDataStore(_Obs(keys, H, W, S), _Sp((A,)), args.demos + 10, image_keys=keys)
    replay_buffer = populate_data_store(replay_buffer, [path])

    sample_obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in keys}
    sample_obs["state"] = np.zeros((1, S), np.float32)
    agent = make_bc_agent(0, sample_obs, np.zeros((A,), np.float32), image_keys=keys, batch_size=B)

    # bc_policy.py:158-168
    it = replay_buffer.get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True})
    for _ in range(args.warmup):
        agent, info = agent.update(next(it))
    torch.cuda.synchronize()
    batches = [next(it) for _ in range(min(args.steps, 8))]   # (sampling is not what is timed)
    t0 = time.perf_counter()
    for i in range(args.steps):
        agent, info = agent.update(batches[i % len(batches)])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    print(f"BC step  B={B} {len(keys)}x{H}x{W}: {ms:.3f} ms/step ({1e3 / ms:.0f} grad-steps/s)  info {dict(info)}")

    # the frozen trunk alone over the same n_cam x B images (the floor of the step)
    from serl_amd.agents.core import AgentCore
    core = AgentCore(n_cam=len(keys), H=H, W=W, state_dim=S, act_dim=A, batch=B)
    frames = torch.randint(0, 256, (len(keys) * B, H, W, 3), dtype=torch.uint8, device="cuda")
    for _ in range(args.warmup):
        core.trunk_forward(frames)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        core.trunk_forward(frames)
    torch.cuda.synchronize()
    tms = (time.perf_counter() - t0) * 1e3 / args.steps
    print(f"trunk    {len(keys) * B} images {H}x{W}: {tms:.3f} ms/pass  (BC step = trunk + {ms - tms:.3f} ms)")


if __name__ == "__main__":
    main()
