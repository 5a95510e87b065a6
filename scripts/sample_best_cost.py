"""Cost of acting on the critic: serl_agent_sample_best against the composition it replaces -- serl_agent_eval_policy, mean and
std to the host, NumPy sampling and tanh there, the candidates back through serl_agent_eval_q_actions, Q to the host and a host
argmax -- on one GPU at the benchmark shape (two 128x128 cameras on the frozen trunk, ensemble 10, width 256; n = 32 observations
x N = 8 candidates).  Both are timed with device events on the calling stream after a warm-up, in alternating windows of `--calls`
calls (the composition's host work and copies lie inside its window: they are part of what it costs); the launches are the
library's own count of update-chain kernels (serl_debug_chain_launches: encoder heads, GEMMs and row kernels, not the trunk's
convolutions, of which the composition runs two passes and the one call one).  Prints one JSON line.

    python scripts/sample_best_cost.py [--n 32] [--candidates 8] [--calls 20] [--windows 9]
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
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_best_cost.py measures on a GPU"
    import agent_helpers as AH
    from oracle import drq_oracle as O
    n, N = args.n, args.candidates
    cfg = O.Config(H=128, W=128)
    trunk, theta = O.init_params(cfg, 42)
    core = AH.load_leaves(AH.make_core(cfg, n * N), cfg, trunk, theta)
    rng = np.random.default_rng(0)
    frames = torch.tensor(rng.integers(0, 256, (cfg.n_cam, n, cfg.H, cfg.W, 3), dtype=np.uint8), device="cuda")
    state = torch.tensor(rng.standard_normal((n, cfg.S)).astype(np.float32), device="cuda")
    eps_host = rng.standard_normal((N, n, cfg.A)).astype(np.float32)
    eps = torch.tensor(eps_host, device="cuda")

    def one_call():
        out = core.sample_best(frames, state, eps, info=True)
        return out["action"].cpu().numpy(), out["index"].cpu().numpy(), out["score"].cpu().numpy()

    def composition():
        pi = core.eval_policy(frames, state)
        mean, std = pi["mean"].cpu().numpy(), pi["std"].cpu().numpy()
        cand = np.tanh(mean[:, None] + std[:, None] * eps_host.transpose(1, 0, 2)).astype(np.float32)
        score = core.eval_q(frames, state, torch.from_numpy(cand).to("cuda")).cpu().numpy().min(0)
        index = score.argmax(1)
        return cand[np.arange(n), index], index, score.max(1)

    launches, answers = {}, {}
    for name, f in (("sample_best", one_call), ("composition", composition)):      # warm-up, the launch counts and the agreement
        f()
        before = core.L.serl_debug_chain_launches()
        answers[name] = f()
        launches[name] = int(core.L.serl_debug_chain_launches() - before)
    (a0, i0, s0), (a1, i1, s1) = answers["sample_best"], answers["composition"]
    times = {"sample_best": [], "composition": []}
    for _ in range(args.windows):
        for name, f in (("sample_best", one_call), ("composition", composition)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                f()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.calls)
    res = {"n": n, "candidates": N, "cameras": cfg.n_cam, "image": [cfg.H, cfg.W], "ensemble": cfg.ensemble, "hidden": cfg.hidden,
           "calls_per_window": args.calls, "windows": args.windows, "rows_with_the_same_index": int((i0 == i1).sum()),
           "max_abs_diff_action": float(np.abs(a0 - a1).max()), "max_abs_diff_score": float(np.abs(s0 - s1).max())}
    for name in ("sample_best", "composition"):
        res[name] = {"ms_median": statistics.median(times[name]), "ms_min": min(times[name]), "ms_max": max(times[name]),
                     "chain_launches": launches[name]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
