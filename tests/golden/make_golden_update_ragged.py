"""Generates the ragged-width fixtures: the REFERENCE's own SACAgent / DrQAgent with critic and policy MLP widths off the 64 grid,
imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim, recorded as make_golden_update_shapes.py
records its fixtures (the same wrappers, the same file format, the two lists under "mlp_shapes" in the meta block).  Run in the
build container (needs the reference):
    python tests/golden/make_golden_update_ragged.py [case ...]

  ragged_update_sac_state.npz  critic [400, 300], policy [400, 300] (TD3's and DDPG's published widths), B = 72;
                               high_utd 2, update (all three), high_utd 1
  ragged_update_drq.npz        one camera 64x64, critic [100, 200], policy [300], B = 6; critics, high_utd 2
  ragged_init_sac_state.npz    seed 0, critic [100, 50], policy [65, 127, 3]: the initial leaves, state.rng and one high_utd 1
                               (make_golden_init.py's run_agent_case, threefry stream, 512 samples per leaf)

Before a file is written the reference's own parameter tree is asserted to have the true widths (_check_shapes).  The names do
not start with "update_" / "init_": other tests glob those prefixes.  tests/test_mlp_ragged_{cpu,gpu}.py read them."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
import mlp_ragged as MR  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SH = _load("make_golden_update_shapes")     # shape_general, _meta, _check_shapes: the recorder's wrappers for two lists of any width
ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


FULL_MAX = 2048     # leaves up to this size are stored whole (G.FULL_MAX = 4096 would keep every [10][400] vector in all eight sections)


def write(path, res, n_sample, meta):
    """variant_recorder.write with G.pack's full_max lowered, so that the [400, 300] file stays under the 1 MiB of a committed file"""
    res["prng"] = "philox"
    rec = G.pack(res, MR.PARAM_SEED, MR.BATCH_SEED, n_sample=n_sample, full_max=FULL_MAX)
    m = json.loads(str(rec["meta"]))
    m["mlp_shapes"] = meta
    rec["meta"] = np.array(json.dumps(m))
    np.savez_compressed(path, shapes_n_sample=np.int64(n_sample), **rec)
    size = os.path.getsize(path)
    assert size < 1 << 20, (path, size)
    print(os.path.basename(path)[:-4], "->", path, f"{size / 1e6:.2f} MB", "final step", res["final"]["step"], meta,
          {k: round(v, 6) for k, v in res["steps"][-1]["info"].items()})


def main():
    for name, (cfg, B, sched, n_sample) in MR.golden_update_cases().items():
        if ONLY and f"update_{name}" not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        with SH.shape_general(cfg):
            res = RR.run_reference(cfg, B, sched, MR.PARAM_SEED, MR.BATCH_SEED)
            SH._check_shapes(res["final"]["param_tree"], cfg)
            write(os.path.join(HERE, f"ragged_update_{name}.npz"), res, n_sample, SH._meta(cfg))
    if ONLY and "init_sac_state" not in ONLY:
        return
    cfg, B, sched = MR.golden_init_case()
    mi = _load("make_golden_init")          # sets SERL_JAXSHIM_PRNG=threefry; records mi.N_SAMPLE = 512 samples, as for init_*.npz
    with SH.shape_general(cfg):
        rec = mi.run_agent_case(cfg, B, sched)
        rec["init_cfg"] = np.frombuffer(repr(G.cfg_to_dict(cfg)).encode(), np.uint8)
    assert tuple(rec["init_shape/actor/w3"]) == cfg.policy_dims[1:], rec["init_shape/actor/w3"]
    m = json.loads(str(rec["meta"]))
    SH._check_shapes(m["param_tree"], cfg)
    m["mlp_shapes"] = SH._meta(cfg)
    rec["meta"] = np.array(json.dumps(m))
    rec["shapes_n_sample"] = np.int64(mi.N_SAMPLE)
    path = os.path.join(HERE, "ragged_init_sac_state.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 1 << 20, path
    print("init_sac_state ->", path, f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
