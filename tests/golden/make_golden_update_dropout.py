"""Generates the MLP-Dropout fixtures: the REFERENCE's own SACAgent / DrQAgent (serl_launcher/agents/continuous/{sac,drq}.py,
networks/mlp.py:10-32), imported unmodified from its checkout and run under the stand-ins of oracle/jaxshim in fp64, with a
positive `dropout_rate` in the critic's and / or the policy's network kwargs.  Run in the build container (needs the reference):
    python tests/golden/make_golden_update_dropout.py [name ...]

The recipe of make_golden_update_activations.py: the two create functions are wrapped AT RUN TIME
(variant_recorder.reference_create_overrides) so that the kwargs the launcher factories pass carry the rate (and, for the
w320_swish file, the width and the activation; for the droq file, an ensemble of 2: critic_ensemble_size is a scalar kwarg and gets
a wrapper of its own here).  oracle.ref_update_runner._parse_noise is wrapped at run time too: the wrapper takes the `bernoulli`
records of the MLPs' Dropout layers (context .../Dropout_<i> outside an encoder) off the tape, checks their shape, probability
and order against mlp_dropout.site_order -- per critic update: policy at next_obs, target critic, [the REDQ randint], online critic; then policy at
obs, critic inside the actor loss, policy at next_obs for the temperature loss -- and that all ensemble members of a critic forward
drew the same values (ensemblize splits only the params stream: 2 x ensemble records per forward, member-major), keeps one copy per
(site, layer, critic update) and hands the rest of the tape to the original parser.

Recorded under SERL_JAXSHIM_PRNG=threefry: the stand-in's default stream hashes only the first bytes of a make_rng path, so that
Dropout_0 and Dropout_1 of a network -- and every forward that shares an rng -- would draw identical masks and a fixture could not
tell the layers apart.  The masks are stored bit-packed as s<i>_drop_<site> (u8[2 layers, rows, hidden]); the names do not begin
with mask_, which golden_update.unpack reads as camera masks.  meta["dropout"] records the rates, meta["activations"] the
activations (golden_replay.load_variant lays them over the Config), meta["prng"] = "threefry".

  drop_update_sac_state.npz             golden_replay.STATE shape, 72 rows, STATE_SCHED, hidden 256, critic 0.1, policy 0.05
  drop_update_sac_state_droq.npz        ensemble 2, critic_subsample_size None, critic 0.01, policy 0: target and online critic share rng and masks
  drop_update_sac_state_w320_swish.npz  hidden 320 (the width-generic rows), swish, critic 0.1, policy 0.1
  drop_update_drq_one_cam.npz           one camera 64x64, S = 5, A = 3, 6 rows; critics, high_utd 2: camera masks and MLP masks on one tape
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
os.environ["SERL_JAXSHIM_PRNG"] = "threefry"
from oracle import ref_update_runner as RR  # noqa: E402
from oracle import ref_update_shim as R  # noqa: E402
import golden_replay as GR  # noqa: E402
import mlp_dropout as MD  # noqa: E402
import variant_recorder as VR  # noqa: E402

ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]


def _is_mlp_dropout(r):
    return r["kind"] == "bernoulli" and r["context"] and "Dropout_" in r["context"][-1] and "encoder" not in r["context"][-1]


def take_mlp_masks(cfg, rates, B, recs, kind, utd, nets):
    """-> ({site: u8[2, B, hidden]}, the tape without the MLP Dropout records)"""
    rate = {"critic": rates[0], "policy": rates[1]}
    n_critic = utd if kind == "high_utd" else (1 if kind == "critics" or "critic" in nets else 0)
    mb = B // max(n_critic, 1)
    mine = [r for r in recs if _is_mlp_dropout(r)]
    rest = [r for r in recs if not _is_mlp_dropout(r)]
    masks, pos = {}, 0
    for site, i in MD.site_order(kind, n_critic, nets):
        net = MD.MLP_SITE_NETWORK[site]
        if not rate[net] > 0:
            continue
        rows = B if i is None else mb
        members = cfg.ensemble if net == "critic" else 1
        group = mine[pos:pos + 2 * members]
        pos += 2 * members
        assert len(group) == 2 * members, (site, i, len(group))
        for m in range(members):
            for layer in (0, 1):
                r = group[2 * m + layer]
                assert r["context"][-1] == "dropout:" + "/".join(MD.standin_dropout_path(net, layer, cfg.state_only)), (site, r["context"])
                assert r["value"].shape == (rows, cfg.hidden) and abs(r["p"] - (1 - rate[net])) < 1e-12, (site, r["value"].shape, r["p"])
                assert np.array_equal(r["value"], group[layer]["value"]), f"{site}: member {m} drew another mask than member 0"
        dst = masks.setdefault(site, np.zeros((2, B, cfg.hidden), np.uint8))
        lo = 0 if i is None else i * mb
        for layer in (0, 1):
            dst[layer, lo:lo + rows] = group[layer]["value"].astype(np.uint8)
    assert pos == len(mine), f"{len(mine) - pos} unexpected MLP Dropout draws"
    # where the target and the online critic run under one rng (critic_subsample_size None), they draw the same mask
    if cfg.subsample is None and "q_target" in masks:
        assert np.array_equal(masks["q_target"], masks["q_online"])
    elif "q_target" in masks:
        assert not np.array_equal(masks["q_target"], masks["q_online"])
    for m in masks.values():      # the layers are told apart
        assert not np.array_equal(m[0], m[1])
    return masks, rest


@contextlib.contextmanager
def reference_dropout(cfg, rates, taken):
    """create_states / create_drq at the Config's width, activations and ensemble with these rates; `taken` collects the MLP masks
    of every schedule item, in order"""
    R.install(True)
    from serl_launcher.agents.continuous.sac import SACAgent
    over = {"critic_network_kwargs": MD.network_kwargs(cfg, "critic", rates[0]), "policy_network_kwargs": MD.network_kwargs(cfg, "policy", rates[1])}
    parse = RR._parse_noise

    def parse_without_mlp_masks(c, B, recs, kind, utd, nets=()):
        masks, rest = take_mlp_masks(cfg, rates, B, recs, kind, utd, nets)
        taken.append(masks)
        return parse(c, B, rest, kind, utd, nets)
    RR._parse_noise = parse_without_mlp_masks
    cm = SACAgent.__dict__["create_states"]
    try:
        with VR.reference_create_overrides(over):
            inner = SACAgent.__dict__["create_states"]

            def with_ensemble(cls, *a, _orig=inner.__func__, **k):      # (make_sac_agent has no argument for it)
                return _orig(cls, *a, **{**k, "critic_ensemble_size": cfg.ensemble})
            if cfg.state_only:
                SACAgent.create_states = classmethod(with_ensemble)
            try:
                yield
            finally:
                if cfg.state_only:
                    setattr(SACAgent, "create_states", inner)
    finally:
        RR._parse_noise = parse
        assert SACAgent.__dict__["create_states"] is cm


def main():
    for name, row in MD.GOLDEN.items():
        if ONLY and name not in ONLY:
            continue
        cfg, B, sched, rates = row["cfg"], row["B"], row["sched"], row["rates"]
        taken = []
        with reference_dropout(cfg, rates, taken):
            res = RR.run_reference(MD.launcher_cfg(cfg), B, sched, GR.PARAM_SEED, GR.BATCH_SEED)
        assert len(taken) == len(sched)
        for step, masks in zip(res["steps"], taken):
            assert set(masks) == set(MD.sites_of(rates)) & {s for s, _ in MD.site_order(*MD.step_shape(step))}
            step["noise"].update(MD.pack(masks))
        kept = {s: float(np.mean([m[s].mean() for m in taken if s in m])) for s in MD.sites_of(rates)}
        meta = {"critic": rates[0], "policy": rates[1], "kept_fraction": kept, "standin_critic_path": list(MD.standin_dropout_path("critic", 0, cfg.state_only))}
        path = GR.variant_path("drop", name)
        VR.write(path, res, GR.PARAM_SEED, GR.BATCH_SEED, n_sample_key="drop_n_sample", n_sample=row["n_sample"], meta_key="dropout", meta=meta)
        # (variant_recorder.write stamps the stand-in's default stream; this run drew from its threefry one)
        z = dict(np.load(path))
        m = json.loads(str(z["meta"]))
        m["prng"] = "threefry"
        m["activations"] = {"critic": cfg.critic_activation, "policy": cfg.policy_activation}
        z["meta"] = np.array(json.dumps(m))
        np.savez_compressed(path, **z)
        assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
        print(name, "written,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
