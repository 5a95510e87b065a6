"""Generates the MLP-activation fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py,
networks/mlp.py:10-32), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim in fp64, with an
activation other than the launcher's tanh in the critic's and / or the policy's MLP.  Run in the build container (needs the
reference):
    python tests/golden/make_golden_update_activations.py [name ...]

The launcher factories write their own network kwargs into create_states / create_drq (utils/launcher.py:50-116), so the two create
functions are wrapped AT RUN TIME, as make_golden_update_policy.py wraps them for policy_kwargs: the wrapper overrides `activations`
in the critic_network_kwargs / policy_network_kwargs the factory passes.  What it passes is a callable (mlp.py:19-21 takes one as it
is) that reports every tensor it is applied to -- the pre-activations -- to a tests/mlp_activations.Recorder and then calls the
shim's own jax.nn function of that name.  The run itself is given the launcher's Config: that is the cfg record of the files.

  act_update_sac_state_{swish,relu,mixed}.npz   S = 10, A = 5, 72 rows; high_utd 2, update, high_utd 1; mixed = critic relu, policy swish
  act_trained_sac_state_swish.npz               the same schedule from trained_regime.trained_like leaves: |pre-activation| of tens
  act_update_drq_swish.npz                      one camera 64x64, S = 5, A = 3, 6 rows; critics, high_utd 2

ReLU's kink: a fixture with a relu network counts only if the smallest |pre-activation| of EVERY evaluation is at least
mlp_activations.KINK_MIN = 1e-4 (an fp32 run could otherwise land on the other side of 0 and flip a gradient term).  The batch seed
moves from BATCH_SEED in steps of 16 (a run uses batch_seed + schedule item) until that holds; meta["activations"] records the seed
used, the seeds tried and the minimum.  From O.init_params' LayerNorm leaves no seed can satisfy it (8e6 pre-activations of density
0.4 at 0 per run: over the seeds 100, 116, ..., 244 the smallest was between 5.4e-9 and 1.0e-6), so the two relu fixtures start from
mlp_activations.kink_margin's leaves: a few live columns per LayerNorm vector, whose sign changes from row to row, and all others on
in every row or off in every row.

Every file records under meta["activations"] the two names, the regime, and min / max |pre-activation| over the run.  The file names
do not start with "update_": tests/test_reference_update.py and tests/test_golden_update_gpu.py run every update_*.npz through the
launcher's tanh.  tests/test_mlp_activations_{cpu,gpu}.py read these files.
"""
import contextlib
import dataclasses
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402
import golden_replay as GR  # noqa: E402
import mlp_activations as MA  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]
SEED_STEP = 16
MAX_SEEDS = 400      # the seed moves on until the condition holds; a bound so that a broken recipe ends


@contextlib.contextmanager
def reference_activations(critic, policy, recs, floors):
    """create_states / create_drq with these activations; recs = {"critic": Recorder, "policy": Recorder}; floors = {network:
    the Recorder's floor for the run proper} (set once the agent exists: the factory's init pass sits at 0)"""
    R.install(True)
    import jax.nn
    from jax._core import raw

    def recording(name, rec):
        fn = getattr(jax.nn, name)

        def activation(x):
            rec.see(raw(x))
            return fn(x)
        activation.__name__ = name
        return activation
    acts = {"critic_network_kwargs": {"activations": recording(critic, recs["critic"])},
            "policy_network_kwargs": {"activations": recording(policy, recs["policy"])}}
    # the factory's model_def.init runs both networks on zero observations (pre-activation = the LayerNorm bias = 0 everywhere):
    # what the recorders saw until the agent exists is no evaluation of the run
    make = RR._make_reference_agent

    def make_and_forget(*a, **k):
        agent = make(*a, **k)
        for rec in recs.values():
            assert rec.min_abs, "an activation was never called: the kwarg did not arrive"
            rec.reset()
        for w, floor in floors.items():
            recs[w].floor = floor
        return agent
    RR._make_reference_agent = make_and_forget
    try:
        with VR.reference_create_overrides(acts):
            yield
    finally:
        RR._make_reference_agent = make


def main():
    for name, (cfg, B, sched, (critic, policy), regime, n_sample) in MA.GOLDEN.items():
        if ONLY and name not in ONLY:
            continue
        os.environ.pop("SERL_JAXSHIM_PRNG", None)
        relu = [w for w, a in (("critic", critic), ("policy", policy)) if a == "relu"]
        tried = []
        for k in range(MAX_SEEDS if relu else 1):
            batch_seed = GR.BATCH_SEED + SEED_STEP * k
            recs = {"critic": MA.Recorder(), "policy": MA.Recorder()}
            try:
                with reference_activations(critic, policy, recs, {w: MA.KINK_MIN for w in relu}):
                    assert (cfg.critic_activation, cfg.policy_activation) == (critic, policy)
                    res = RR.run_reference(dataclasses.replace(cfg, critic_activation="tanh", policy_activation="tanh"), B, sched,
                                           GR.PARAM_SEED, batch_seed,
                                           theta_transform=lambda th, c: MA.act_theta(th, c, regime))
            except MA.Kink as e:      # this seed is out at its first evaluation inside the margin: the next one
                tried.append((batch_seed, e.args[0]))
                continue
            assert recs["critic"].min_abs and recs["policy"].min_abs, "an activation was never called: the kwarg did not arrive"
            kink = min([min(recs[w].min_abs) for w in relu], default=None)
            tried.append((batch_seed, kink))
            assert not relu or all(recs[w].kink_free for w in relu)
            break
        else:
            print(name, f"NOT WRITTEN: no batch seed among {MAX_SEEDS} keeps every relu pre-activation {MA.KINK_MIN:g} away from 0;",
                  "(seed, the |pre-activation| that put it out):", [(s, float(f"{m:.3g}")) for s, m in tried[:20]])
            continue
        if relu:      # the run crossed the kink: the live units were on in some rows and off in others
            frac = {w: recs[w].off_fraction for w in relu}
            print(name, "seeds tried", len(tried), "live-unit rows off:", frac)
        meta = {"critic": critic, "policy": policy, "regime": regime, "transform": "mlp_activations.act_theta",
                "batch_seed": batch_seed, "relu_min_abs_pre": kink, "seeds_tried": len(tried), "margin_seed": MA.MARGIN_SEED,
                "relu_off_fraction": {w: recs[w].off_fraction for w in relu},
                "evaluations": {w: len(recs[w].min_abs) for w in recs},
                "min_abs_pre": {w: min(recs[w].min_abs) for w in recs},
                "max_abs_pre": {w: max(recs[w].max_abs) for w in recs}}
        if regime == "trained":     # swish's saturated branch: sigmoid's exponent reaches ten and more
            assert max(meta["max_abs_pre"].values()) >= 10.0, meta["max_abs_pre"]
        VR.write(GR.variant_path("act", name), res, GR.PARAM_SEED, batch_seed, n_sample_key="act_n_sample", n_sample=n_sample,
                 meta_key="activations", meta=meta)


if __name__ == "__main__":
    main()
