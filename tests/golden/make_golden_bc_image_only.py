"""Generates tests/golden/imgonly_bc_64.npz: the REFERENCE's own behaviour-cloning agent (serl_launcher/agents/continuous/bc.py)
with use_proprio=False -- BCAgent.create's own default (bc.py:126) -- run by tests/golden/make_golden_bc.py's run_case, unmodified.
Run in the build container (needs the reference):
    python tests/golden/make_golden_bc_image_only.py

make_bc_agent writes use_proprio=True into its call of BCAgent.create (utils/launcher.py:26-47), so BCAgent.create is wrapped AT
RUN TIME to set the flag.  For the duration of the run make_golden_bc's table of trainable leaves loses the four enc/proprio
entries, the oracle's leaf tables are tests/image_only.py's, and G.cfg_to_dict keeps the record of the Config the launcher's (the
flag stands in the meta block, under "image_only").  The run asserts on the reference's own parameter tree that `encoder` holds
the cameras alone and that network/Dense_0's kernel has 256 n_cam rows.  Nothing under oracle/ changes.

  imgonly_bc_64.npz   two cameras 64x64, S = 5, A = 3, B = 8, two updates with recorded Dropout masks, then inference
"""
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
from oracle import ref_update_shim as R  # noqa: E402
import image_only as IO  # noqa: E402

_OWN = ("critic_dims", "policy_dims", "critic_layer_norm", "policy_layer_norm", "fixed_std", "use_proprio")
NAME, B, STEPS = "imgonly_bc_64", 8, 2
CFG = IO.ImageOnlyConfig(image_keys=("front", "wrist"), H=64, W=64, S=5, A=3, use_proprio=False)


def main():
    spec = importlib.util.spec_from_file_location("make_golden_bc", os.path.join(HERE, "make_golden_bc.py"))
    mb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mb)
    R.install(True)
    from serl_launcher.agents.continuous.bc import BCAgent
    cm = BCAgent.__dict__["create"]

    def patched(cls, *a, _orig=cm.__func__, **k):
        assert "use_proprio" in k, "the factory no longer passes use_proprio by keyword"
        k["use_proprio"] = False
        return _orig(cls, *a, **k)
    saved = mb.TRAIN_PATHS, G.cfg_to_dict
    mb.TRAIN_PATHS = {k: v for k, v in saved[0].items() if not k.startswith("enc/proprio/")}
    G.cfg_to_dict = lambda c: {k: v for k, v in saved[1](c).items() if k not in _OWN}
    BCAgent.create = classmethod(patched)
    os.environ.pop("SERL_JAXSHIM_PRNG", None)
    try:
        with IO.installed():
            rec = mb.run_case(CFG, B, STEPS, "philox")
    finally:
        BCAgent.create = cm
        mb.TRAIN_PATHS, G.cfg_to_dict = saved
    m = json.loads(str(rec["meta"]))
    paths = m["param_paths"] if "param_paths" in m else [str(p) for p in rec["param_paths"]]
    enc = [p for p in paths if p.startswith("modules_actor/encoder/")]
    assert enc and all(p.split("/")[2].startswith("encoder_") for p in enc), enc      # no Dense_0 / LayerNorm_0 under `encoder`
    m["image_only"] = {"use_proprio": False}
    rec["meta"] = np.array(json.dumps(m))
    path = os.path.join(HERE, f"{NAME}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 1 << 20, (path, size)
    print(NAME, "->", path, f"{size / 1e6:.2f} MB", m["final_step"], [list(rec[f"s{i}_info"]) for i in range(STEPS)][-1])


if __name__ == "__main__":
    main()
