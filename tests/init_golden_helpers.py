"""Shared by tests/test_init_reference_cpu.py and tests/test_init_reference_gpu.py: reading tests/golden/init_*.npz
(tests/golden/make_golden_init.py) -- per leaf the reference's initial value, full for small leaves, else 512 sampled elements and
three sums (oracle/golden_update.leaf_record)."""
import ast
import glob
import os

import numpy as np

from oracle import golden_update as G

N_SAMPLE = 512          # make_golden_init.py's sample count
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "init_*.npz")))


def case_name(path):
    return os.path.basename(path)[5:-4]


def load(path):
    g = np.load(path)
    cfg = G.cfg_from_dict(ast.literal_eval(bytes(g["init_cfg"]).decode()))
    leaves = {}
    for k in g.files:
        if k.startswith("init/"):
            name, part = k[5:].rsplit("/", 1)
            leaves.setdefault(name, {})[part] = g[k]
    shapes = {k[11:]: tuple(int(s) for s in g[k]) for k in g.files if k.startswith("init_shape/")}
    leaves = {product_name(k, cfg.image_keys): (k, v) for k, v in leaves.items()}
    shapes = {product_name(k, cfg.image_keys): v for k, v in shapes.items()}
    return g, cfg, leaves, shapes


def product_name(name, keys):
    """the golden's leaf names carry the camera's key (enc/<key>/...), the product's its index"""
    parts = name.split("/")
    if parts[0] == "enc" and parts[1] in keys:
        parts[1] = str(list(keys).index(parts[1]))
    return "/".join(parts)


def sample_idx(n, name):
    r = np.random.Generator(np.random.PCG64(np.random.SeedSequence([n, G._salt(name), 7])))
    return np.sort(r.choice(n, size=N_SAMPLE, replace=False))


def mismatch(name, entry, got):
    """-> None when `got` (float32) equals the recorded reference leaf (an entry of load()'s dict) bit for bit, else a
    description"""
    name, rec = entry
    got = np.asarray(got, np.float32).reshape(-1)
    if "full" in rec:
        want = rec["full"].astype(np.float32)
        if got.shape != want.shape:
            return f"{name}: {got.size} elements, golden {want.size}"
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    else:
        idx = sample_idx(got.size, name)
        want = rec["val"].astype(np.float32)
        bad = idx[np.flatnonzero(got[idx].view(np.uint32) != want.view(np.uint32))]
        st = np.array([got.astype(np.float64).sum(), (got.astype(np.float64) ** 2).sum()])
        if not bad.size and not np.allclose(st, rec["stat"][:2], rtol=1e-9, atol=1e-9):
            return f"{name}: sums {st} vs {rec['stat'][:2]}"
    if bad.size:
        i = int(bad[0])
        return f"{name}: {bad.size} elements differ, first at {i}: {got[i]!r}"
    return None


def product_leaves(case, cfg, device=None):
    """the flat leaves utils/init_ref.py draws for a golden case (device None: the host twins)"""
    from serl_amd.utils import init_ref as IR
    if case.startswith("bc"):
        return IR.bc_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, device=device)
    if case == "classifier":
        return IR.classifier_reference(cfg.image_keys, cfg.H, cfg.W, 0, device=device)
    return IR.theta_reference(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, 0, ensemble=cfg.ensemble, encoder_type=cfg.encoder_type,
                              temperature_init=1e-2, device=device)
