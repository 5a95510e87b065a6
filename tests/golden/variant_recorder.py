"""Shared by the generators of the variant fixtures (make_golden_update_{widths,trained,policy,activations}.py): the wrapper of
the reference's create functions that overrides kwargs the launcher factories write, and the tail that packs a run of
oracle.ref_update_runner.run_reference into its file."""
import contextlib
import json
import os

import numpy as np

from oracle import golden_update as G
from oracle import ref_update_shim as R


@contextlib.contextmanager
def reference_create_overrides(overrides):
    """SACAgent.create_states / DrQAgent.create_drq with k[name] = {**k[name], **overrides[name]} for every kwarg name of
    `overrides`, whatever the launcher factory passes (utils/launcher.py:50-116 writes its own and has no argument for them)"""
    R.install(True)
    from serl_launcher.agents.continuous.drq import DrQAgent
    from serl_launcher.agents.continuous.sac import SACAgent
    saved = []
    for target, name in ((SACAgent, "create_states"), (DrQAgent, "create_drq")):
        cm = target.__dict__[name]
        saved.append((target, name, cm))

        def patched(cls, *a, _orig=cm.__func__, **k):
            for nk, over in overrides.items():
                assert nk in k, f"the factory no longer passes {nk} by keyword"
                k[nk] = {**k[nk], **over}
            return _orig(cls, *a, **k)
        setattr(target, name, classmethod(patched))
    try:
        yield
    finally:
        for target, name, cm in saved:
            setattr(target, name, cm)


def write(path, res, param_seed, batch_seed, *, n_sample_key, n_sample, meta_key=None, meta=None, extra=None):
    """G.pack of a run under the stand-in's default (philox) stream with `n_sample` sampled elements per large leaf, recorded under
    n_sample_key; meta[meta_key] = meta; extra: further arrays.  The file stays under the 1 MiB of a committed file."""
    res["prng"] = "philox"
    rec = G.pack(res, param_seed, batch_seed, n_sample=n_sample)
    if meta_key is not None:
        m = json.loads(str(rec["meta"]))
        m[meta_key] = meta
        rec["meta"] = np.array(json.dumps(m))
    np.savez_compressed(path, **{n_sample_key: np.int64(n_sample)}, **rec, **(extra or {}))
    size = os.path.getsize(path)
    assert size < 1 << 20, (path, size)
    print(os.path.basename(path)[:-4], "->", path, f"{size / 1e6:.2f} MB", "final step", res["final"]["step"], meta or "",
          {k: round(v, 6) for k, v in res["steps"][-1]["info"].items()})
