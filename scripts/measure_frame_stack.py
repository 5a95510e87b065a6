"""Cost of frame stacks on the SmallEncoder learner at B = 256, 2 x 128 x 128: for T = 1, 2, 3 one learner step = fused gather +
crop of a lazy batch from an HBM store of stacks of T + DrQAgent.update_critics.  Per T: the median step time of 3 x 200 steps
(un-profiled), then one profiled pass (serl_profile_enable(1)) for the per-kernel table: gather_crop, small_conv0_fwd and
small_conv0_wgrad (layer 0 alone), small_encoder_fwd / small_encoder_bwd (the whole conv stack).  Bytes and FMAs of layer 0 and of
the gather are proportional to T; the last column is each time relative to T = 1, to be read against that.

SERL_MI355_LIB selects another build of the library (the parent commit's, for T = 1): run this script once per build in one job,
alternating, and compare the T = 1 lines.  --stacks 1 limits the run to T = 1 (a build without frame stacks serves nothing else).
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serl_amd import _lib  # noqa: E402
from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore  # noqa: E402
from serl_amd.utils.launcher import make_drq_agent  # noqa: E402
from serl_amd.utils.synthetic import transition_stream  # noqa: E402

KEYS, H, W, S, A, B = ("front", "wrist"), 128, 128, 24, 6, 256
TAGS = ("gather_crop", "small_conv0_fwd", "small_conv0_wgrad", "small_encoder_fwd", "small_encoder_bwd")


class _Sp:
    def __init__(self, shape):
        self.shape = tuple(shape)


class _Dict:
    def __init__(self, spaces):
        self.spaces = {k: spaces[k] for k in sorted(spaces)}


def measure(T, steps, repeats, fill):
    spaces = {k: _Sp((T, H, W, 3)) for k in KEYS}
    spaces["state"] = _Sp((T, S))
    rb = MemoryEfficientReplayBufferDataStore(_Dict(spaces), _Sp((A,)), 2 * fill, image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, H, W, 3, T, S, A, 100, 1), fill):
        rb.insert(tr)
    obs = {k: np.zeros((T, H, W, 3), np.uint8) for k in KEYS}
    obs["state"] = np.zeros((T, S), np.float32)
    agent = make_drq_agent(0, obs, np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="small", batch_size=B)
    it = rb.get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True, "lazy": True})

    def run(n):
        nonlocal agent
        for _ in range(n):
            agent, _ = agent.update_critics(next(it))
        torch.cuda.synchronize()

    run(20)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    L = _lib.lib()
    _lib.check(L.serl_profile_enable(1))
    _lib.check(L.serl_profile_reset())
    run(steps)
    prof = _lib.profile_read()
    _lib.check(L.serl_profile_enable(0))
    return {"T": T, "step_ms_median": float(np.median(ms)), "step_ms_all": [round(v, 4) for v in ms],
            "kernel_us": {t: round(1e3 * prof[t][0] / prof[t][1], 2) for t in TAGS if t in prof and prof[t][1]},
            "launches_per_step": {t: prof[t][1] / steps for t in TAGS if t in prof}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fill", type=int, default=1500)
    args = ap.parse_args()
    rows = [measure(T, args.steps, args.repeats, args.fill) for T in args.stacks]
    base = rows[0]
    for r in rows:
        r["relative_to_first"] = {"step": round(r["step_ms_median"] / base["step_ms_median"], 3),
                                  **{t: round(v / base["kernel_us"][t], 3) for t, v in r["kernel_us"].items() if t in base["kernel_us"]}}
        print(json.dumps(r), flush=True)
    print(json.dumps({"library": _lib.LIB_PATH, "shape": f"B={B} 2x{H}x{W} S={S} A={A}, SmallEncoder, gather+crop + update_critics",
                      "rows": rows}))


if __name__ == "__main__":
    main()
