"""Cost of Q for N candidate actions per observation: serl_agent_eval_q_actions against the loop of N serl_agent_eval_q calls it
replaces, on one GPU at the benchmark shape (two 128x128 cameras on the frozen trunk, ensemble 10, width 256; n = 32 observations
x N = 8 candidates).  Both are timed with device events on the calling stream after a warm-up, in alternating windows of
`--calls` calls; the launches are the library's own count of update-chain kernels (serl_debug_chain_launches: encoder heads, GEMMs
and row kernels, not the trunk's convolutions).  Prints the agreement of the two results and one JSON line.

    python scripts/q_actions_cost.py [--n 32] [--actions 8] [--calls 20] [--windows 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--actions", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "q_actions_cost.py measures on a GPU"
    import agent_helpers as AH
    from oracle import drq_oracle as O
    n, N = args.n, args.actions
    cfg = O.Config(H=128, W=128)
    trunk, theta = O.init_params(cfg, 42)
    core = AH.load_leaves(AH.make_core(cfg, n * N), cfg, trunk, theta)
    rng = np.random.default_rng(0)
    frames = torch.tensor(rng.integers(0, 256, (cfg.n_cam, n, cfg.H, cfg.W, 3), dtype=np.uint8), device="cuda")
    state = torch.tensor(rng.standard_normal((n, cfg.S)).astype(np.float32), device="cuda")
    cand = torch.tensor(rng.uniform(-1, 1, (n, N, cfg.A)).astype(np.float32), device="cuda")
    cols = [cand[:, j].contiguous() for j in range(N)]

    def fanned():
        return core.eval_q(frames, state, cand)

    def loop():
        return torch.stack([core.eval_q(frames, state, c) for c in cols], -1)

    launches = {}
    for name, f in (("fanned", fanned), ("loop", loop)):      # warm-up, the launch counts and the agreement
        f()
        before = core.L.serl_debug_chain_launches()
        out = f()
        launches[name] = int(core.L.serl_debug_chain_launches() - before)
        launches[name + "_out"] = out
    torch.cuda.synchronize()
    a, b = launches.pop("fanned_out").double(), launches.pop("loop_out").double()
    agreement = float((a - b).abs().max() / b.abs().max())
    times = {"fanned": [], "loop": []}
    for _ in range(args.windows):
        for name, f in (("fanned", fanned), ("loop", loop)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                f()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.calls)
    res = {"n": n, "actions": N, "cameras": cfg.n_cam, "image": [cfg.H, cfg.W], "ensemble": cfg.ensemble, "hidden": cfg.hidden,
           "calls_per_window": args.calls, "windows": args.windows, "max_rel_diff_fanned_vs_loop": agreement}
    for name in ("fanned", "loop"):
        res[name] = {"ms_median": statistics.median(times[name]), "ms_min": min(times[name]), "ms_max": max(times[name]),
                     "chain_launches": launches[name]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
