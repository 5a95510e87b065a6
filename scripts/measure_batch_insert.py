"""Measures the batched replay insert against the per-transition loop on one GPU (profiles/README.md):
  1. host microseconds per transition of batch_insert at payloads of 1, 8, 50 and 256 transitions (2 cameras of 128x128x3, T = 1),
     and of a loop over insert() with the same payloads in the same process;
  2. the longest and the median sample_indices(256) call a second thread sees with no insert running, under the insert() loop
     and under batch_insert of payloads of 256.
Prints one JSON line; --out writes it to a file as well.  No thresholds: the numbers are recorded as seen."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

KEYS, H, W, S, A = ("front", "wrist"), 128, 128, 24, 6


def transitions(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        done = k % 50 == 49
        obs, nobs = ({"state": rng.standard_normal((1, S)).astype(np.float32),
                      **{c: rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8) for c in KEYS}} for _ in range(2))
        out.append({"observations": obs, "next_observations": nobs, "actions": np.zeros(A, np.float32), "rewards": np.float32(k),
                    "masks": np.float32(1 - done), "dones": done})
    return out


def store(cap=5000):
    from helpers import make_spaces
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    osp, asp = make_spaces(KEYS, H, W, 3, 1, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, cap, image_keys=KEYS)
    rb.seed(0)
    return rb


def per_transition_us(rb, feed, payload, reps):
    feed(payload)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            feed(payload)
        best = min(best, (time.perf_counter() - t0) / (reps * len(payload)))
        torch.cuda.synchronize()
    return best * 1e6


def sampler_waits(rb, feed, payload, draws=3000):
    """-> (longest, median) microseconds of sample_indices(256) on a second thread while the main thread runs feed(payload)"""
    waits, stop = [], threading.Event()

    def sampler():
        for _ in range(draws):
            t0 = time.perf_counter()
            rb.sample_indices(256)
            waits.append(time.perf_counter() - t0)
        stop.set()

    th = threading.Thread(target=sampler)
    th.start()
    fed = 0
    while not stop.is_set():
        if feed is None:
            stop.wait(0.01)
        else:
            feed(payload)
            fed += len(payload)
    th.join()
    torch.cuda.synchronize()
    w = np.array(waits) * 1e6
    return {"longest_us": round(float(w.max()), 1), "median_us": round(float(np.median(w)), 1), "p99_us": round(float(np.percentile(w, 99)), 1),
            "transitions_fed_meanwhile": fed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pool = transitions(256)
    rb = store()

    def loop(payload):
        for d in payload:
            rb.insert(d)

    res = {"geometry": "2 x 128x128x3, T=1, S=24, A=6, capacity 5000", "host_us_per_transition": {}}
    for p in (1, 8, 50, 256):
        reps = max(2, 1024 // p)
        res["host_us_per_transition"][str(p)] = {"batch_insert": round(per_transition_us(rb, rb.batch_insert, pool[:p], reps), 2),
                                                 "insert_loop": round(per_transition_us(rb, loop, pool[:p], reps), 2)}
    res["sample_indices_256_on_a_second_thread"] = {
        "no_insert_running": sampler_waits(rb, None, None),
        "insert_loop_running": sampler_waits(rb, loop, pool),
        "batch_insert_256_running": sampler_waits(rb, rb.batch_insert, pool),
    }
    res["insert_stats"] = rb.insert_stats()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
