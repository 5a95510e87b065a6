"""Generates the read-only evaluation fixtures: the REFERENCE's own SACAgent / DrQAgent, imported unmodified from its checkout, built
by its launcher factories and patched with our leaves by the construct-and-patch steps of oracle.ref_update_runner.run_reference,
under the stand-ins of oracle/jaxshim in fp64 -- and then ASKED, not stepped:

    agent.forward_critic(obs, actions, rng, train=False)                                         -> q          [ensemble, B]
    agent.forward_critic(obs, actions, rng, grad_params=agent.state.target_params, train=False)  -> q_target   [ensemble, B]
    d = agent.forward_policy(obs, train=False)
    d.distribution.loc, d.distribution.scale_diag  (d.loc, d.scale_diag without the squash)     -> mean, std  [B, A]
    d.mode(), d.log_prob(actions)                                                                -> mode [B, A], log_prob [B]

Run in the build container (needs the reference):
    python tests/golden/make_golden_eval.py [name ...]

  eval_sac_state.npz                 S = 10, A = 4, 8 rows, the launcher's exp + tanh policy
  eval_drq_one_cam.npz               one camera 64x64, S = 5, A = 3, 6 rows
  eval_sac_state_softplus_gauss.npz  softplus std, no squash   } the run-time override of tests/golden/variant_recorder.py, as
  eval_sac_state_uniform.npz         one log_stds vector, tanh } make_golden_update_policy.py uses it; nothing under oracle/ changes

Every case starts from tests/eval_oracle.leaves: trained-regime leaves (tests/trained_regime.trained_like), a target copy from
perturb_target so that q_target differs from q, and stored actions scaled to max |a| <= 1 - 2^-10 (exact fp32 inputs; atanh is well
conditioned for what the oracle and the kernel both read).  The six quantities are stored with oracle.golden_update.leaf_record
under "<quantity>/full"; the inputs are regenerated from their seed (tests/eval_oracle.golden_inputs), not stored.
tests/test_evaluate_{cpu,gpu}.py read these files; their names start with "eval_", which no update_*.npz / init_*.npz glob matches.
"""
import contextlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import golden_update as G  # noqa: E402
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402
import eval_oracle as EO  # noqa: E402
import golden_replay as GR  # noqa: E402
import policy_modes as PM  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def reference_answers(name):
    cfg, B, (std, squash) = EO.GOLDEN[name]
    assert R.reference_available(), "the reference checkout is not present"
    jax = R.install(True)
    import jax.numpy as jnp
    assert (cfg.std_parameterization, cfg.tanh_squash) == (std, squash)
    trunk, theta, target = EO.leaves(cfg)
    launcher = (std, squash) == PM.DEFAULT_MODE
    over = contextlib.nullcontext() if launcher else \
        VR.reference_create_overrides({"policy_kwargs": {"std_parameterization": std, "tanh_squash_distribution": squash}})
    with over:
        agent = RR._make_reference_agent(jax, jnp, cfg, trunk)
    paths = RR.theta_flax_paths(cfg)
    assert set(paths) == set(theta) == set(target), (sorted(paths), sorted(theta))

    def patched(leaves):
        tree = jax.tree_map(lambda a: a, agent.state.params)      # fresh containers, shared leaves
        for leaf, path in paths.items():
            cur = RR._get(tree, path)
            RR._set(tree, path, jnp.asarray(np.asarray(leaves[leaf], np.float64).reshape(tuple(cur.shape))))
        return jax.tree_map(lambda a: jnp.asarray(np.asarray(a)), tree)

    agent = agent.replace(state=agent.state.replace(params=patched(theta), target_params=patched(target)))
    pb = EO.golden_inputs(name)
    if cfg.state_only:
        obs = jnp.asarray(pb["state"][:, 0])
    else:
        obs = {k: jnp.asarray(v[:, :1]) for k, v in pb["frames"].items()}
        obs["state"] = jnp.asarray(pb["state"])
    actions = jnp.asarray(pb["action"])
    rng = agent.state.rng
    q = agent.forward_critic(obs, actions, rng, train=False)
    qt = agent.forward_critic(obs, actions, rng, grad_params=agent.state.target_params, train=False)
    dist = agent.forward_policy(obs, train=False)
    base = dist.distribution if squash else dist
    out = {"q": q, "q_target": qt, "mean": base.loc, "std": base.scale_diag, "mode": dist.mode(), "log_prob": dist.log_prob(actions)}
    out = {k: np.asarray(v, np.float64) for k, v in out.items()}
    assert out["q"].shape == (cfg.ensemble, B) and out["mean"].shape == (B, cfg.A) and out["log_prob"].shape == (B,), \
        {k: v.shape for k, v in out.items()}
    assert np.abs(out["q"] - out["q_target"]).max() > 1e-3, "the target copy does not differ"
    assert all(np.isfinite(v).all() for v in out.values())
    return cfg, B, std, squash, out


def main():
    for name in EO.GOLDEN:
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        cfg, B, std, squash, out = reference_answers(name)
        rec = {"meta": np.array(json.dumps({
            "cfg": G.cfg_to_dict(cfg), "B": B, "std_parameterization": std, "tanh_squash_distribution": squash,
            "param_seed": GR.PARAM_SEED, "batch_seed": EO.BATCH_SEED, "action_bound": EO.ACTION_BOUND,
            "leaves": "eval_oracle.leaves", "shapes": {k: list(v.shape) for k, v in out.items()}}))}
        for k, v in out.items():
            for part, arr in G.leaf_record(k, v).items():
                rec[f"{k}/{part}"] = arr
        path = EO.golden_path(name)
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1 << 20, (path, size)
        print(name, "->", path, size, "bytes", {k: (float(np.min(v)), float(np.max(v))) for k, v in out.items()})


if __name__ == "__main__":
    main()
