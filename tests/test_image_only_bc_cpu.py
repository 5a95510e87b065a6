"""CPU: the image-only behaviour-cloning agent (BCAgent.create(use_proprio=False); serl_bc_opts.no_proprio): the fp64 statement of
tests/image_only_bc.py (tests/bc_oracle.py on the image codes alone), the C ABI's refusal, the ctypes declarations."""
import ctypes as C

import numpy as np
import torch

import bc_oracle as BO
import image_only_bc as IB

SERL_ERR_INVALID = -1      # include/serl_mi355.h


def test_the_statement_trains_the_two_layers_and_the_heads_alone_and_never_reads_the_state():
    with IB.installed():
        assert BO.TRAIN == IB.TRAIN and len(IB.TRAIN) == 8 and not any("proprio" in k for k in IB.TRAIN)
        case = IB.CASES[0]
        cfg, B = IB.case_config(case)
        trunk, theta = IB.theta_of(cfg)
        assert theta["actor/w1"].shape == (256, 256) and not any(k.startswith("enc/proprio") for k in theta)
        infos = []
        for fill in (None, float("nan")):
            st = BO.State(cfg, trunk, theta)
            inp = IB.inputs(cfg, B, 70)
            state = inp["state"] if fill is None else np.full_like(inp["state"], fill)
            info, grads, aux = BO.update(st, BO.features(trunk, cfg, inp["frames"]), state, inp["action"], inp["masks"])
            assert set(grads) == set(IB.TRAIN) and aux["enc"].shape == (B, 256)
            infos.append(info)
        assert infos[0] == infos[1] and all(np.isfinite(v) for v in infos[0].values())
    assert len(BO.TRAIN) == 12      # the original is back


def test_with_the_proprio_branch_the_statement_is_bc_oracles_own():
    import image_only as IO
    from oracle import drq_oracle as O
    case = IB.CASES[0]
    cfg, B = IB.case_config(case, use_proprio=True)
    plain = O.Config(image_keys=cfg.image_keys, H=cfg.H, W=cfg.W, S=cfg.S, A=cfg.A)
    trunk, theta = O.init_params(plain, 42)
    inp = IB.inputs(cfg, B, 70)
    out = []
    for c, ctx in ((cfg, IO.installed), (plain, None)):
        st = BO.State(c, trunk, theta)
        feats = BO.features(trunk, c, inp["frames"])
        if ctx is None:
            out.append((BO.update(st, feats, inp["state"], inp["action"], inp["masks"])[0], st))
        else:
            with ctx():
                out.append((BO.update(st, feats, inp["state"], inp["action"], inp["masks"])[0], st))
    assert out[0][0] == out[1][0]
    for k in BO.TRAIN:
        assert torch.equal(out[0][1].params[k], out[1][1].params[k]), k


def test_c_refusal_and_declarations():
    from serl_amd import _lib, _lib_agent
    L = _lib.lib()
    assert _lib_agent.SerlBcOpts._fields_ == [("no_proprio", C.c_int)] and bytes(_lib_agent.SerlBcOpts()) == b"\0" * 4
    assert _lib_agent.SerlBcCfg._fields_[-1][0] == "std_max"          # serl_bc_cfg is the struct it was
    cfg = _lib_agent.SerlBcCfg(0, 1, 32, 32, 5, 3, 4, 3e-4, 0.1, 1e-5, 5.0)
    for value in (2, -1):
        h = C.c_void_p()
        rc = int(L.serl_bc_create_opts(C.byref(cfg), C.byref(_lib_agent.SerlBcOpts(value)), C.byref(h)))
        assert rc == SERL_ERR_INVALID and f"no_proprio {value} is not" in (L.serl_last_error() or b"").decode()
    assert int(L.serl_bc_use_proprio(None)) == -1


def test_create_refuses_a_use_proprio_that_is_no_bool():
    import pytest
    with pytest.raises(ValueError, match="use_proprio"):
        IB.create(use_proprio="no")


# ---- the reference's own code: tests/golden/imgonly_bc_64.npz ----------------------------------------------------------------------
def test_tables_match_the_tree_the_reference_built():
    from oracle import golden_update as G
    from serl_amd.agents.flax_tree import bc_paths, bc_shapes, tree_from_leaves
    d, meta, cfg = IB.golden()
    want = meta["param_tree"]
    enc = want["modules_actor"]["encoder"]
    assert sorted(enc) == sorted(f"encoder_{k}" for k in cfg.image_keys)          # no Dense_0 / LayerNorm_0
    sh, paths = bc_shapes(cfg.image_keys, cfg.H, cfg.W, cfg.S, cfg.A, use_proprio=False), bc_paths(cfg.image_keys, use_proprio=False)
    got = G.shape_tree(tree_from_leaves(paths, sh, lambda leaf: np.zeros(int(np.prod(sh[leaf])), np.float32)))
    assert got == want
    assert tuple(want["modules_actor"]["network"]["Dense_0"]["kernel"]) == (256 * cfg.n_cam, 256)


def test_the_statement_reproduces_the_reference_golden():
    from oracle import golden_update as G
    from oracle.ref_update_runner import synth_packed_batch
    from test_reference_update import F64_TOL
    d, meta, cfg = IB.golden()
    B = meta["B"]
    with IB.installed():
        trunk, theta = IB.theta_of(cfg, meta["param_seed"])
        st = BO.State(cfg, trunk, theta)
        for i in range(meta["steps"]):
            pb = synth_packed_batch(cfg, B, meta["batch_seed"] + i)
            feats = BO.features(trunk, cfg, {k: v[:, 0] for k, v in pb["frames"].items()})
            info, _, aux = BO.update(st, feats, pb["state"][:, 0], pb["action"], IB.golden_masks(d, cfg, i, B))
            ref = d[f"s{i}_info"]
            assert abs(info["actor_loss"] - ref[0]) <= F64_TOL * max(1.0, abs(ref[0])) and abs(info["mse"] - ref[1]) <= F64_TOL * max(1.0, abs(ref[1]))
            if i == 0:
                assert np.abs(aux["enc"].numpy() - d["enc0"]).max() < F64_TOL and d["enc0"].shape == (B, 256 * cfg.n_cam)
        for leaf in IB.TRAIN:
            for sec, tree in (("params", st.params), ("mu", st.mu), ("nu", st.nu)):
                rec = {k.split("|")[2]: d[k] for k in d.files if k.startswith(f"f_{sec}|{leaf}|")}
                e, how = G.leaf_compare(f"{sec}/{leaf}", rec, tree[leaf].numpy())
                assert e < F64_TOL, (sec, leaf, how, e)
        assert not any(k.startswith("f_params|enc/proprio") for k in d.files)
