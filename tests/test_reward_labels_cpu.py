"""CPU: the surface of reward labelling inside the DrQ update (vice.py:546,594) -- the C ABI declares and binds the new symbols,
the Python names do not collide with names the API-surface test keeps absent, and the example parses its arguments."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"serl_classifier_logits_from_features": 7, "serl_agent_set_reward_classifier": 4, "serl_agent_label_rewards": 2,
               "serl_agent_reward_label_rows": 1, "serl_agent_read_reward_labels": 5}


def test_header_declares_and_bindings_cover_the_new_symbols():
    from serl_amd import _lib, _lib_agent
    declared = _lib.exported_symbols()
    for name, nargs in NEW_SYMBOLS.items():
        assert declared.get(name) == nargs, (name, declared.get(name))
        assert len(_lib_agent.SIGNATURES[name]) == nargs, name
    hdr = open(os.path.join(ROOT, "include", "serl_mi355.h")).read()
    assert "vice.py:546" in hdr and "vice.py:594" in hdr and "vice.py:609" in hdr
    for mode in ("SERL_LABEL_NONE 0", "SERL_LABEL_FEATURES 1", "SERL_LABEL_FRAMES 2"):
        assert f"#define {mode}" in hdr


def test_library_exports_the_new_symbols():
    from serl_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None


def test_python_names_are_not_among_the_names_kept_absent():
    import test_api_surface as S
    from serl_amd.agents.drq import DrQAgent
    from serl_amd.agents.sac import SACAgent
    ours = ("set_reward_classifier", "reward_classifier", "reward_label_mode", "last_reward_labels")
    forbidden = {qual.split(".")[-1] for _, qual in S.NOT_MIRRORED}
    for name in ours:
        assert name not in forbidden, name
        assert hasattr(DrQAgent, name) and hasattr(SACAgent, name)
    import serl_amd.utils.launcher as launcher
    assert not hasattr(launcher, "make_vice_agent")


def test_example_parses_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "learner_vice_synthetic.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--critic_actor_ratio" in out.stdout and "--goal_frames" in out.stdout
