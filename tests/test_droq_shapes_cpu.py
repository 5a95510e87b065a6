"""CPU: MLP Dropout at every served shape (mlp_dropout="any", serl_agent_opts.dropout_any): what the arguments alone decide, the
header and the binding table, and the oracle hook of tests/droq_shapes.py (one mask per site and layer, relu off the kink)."""
import dataclasses
import os
import re

import pytest

from serl_amd import _lib_agent
from serl_amd.utils import init as pinit
import droq_shapes as DS
import mlp_plain as MP
import mlp_shapes as MS

_KW = dict(mlp_shapes=True, mlp_plain=True, mlp_ragged=True, mlp_wide=True)


def _spec(name, mode, **over):
    cfg, _, rates, _ = DS.case_config(name)
    nets = [MP.mlp_kwargs(d, ln, activations=a, dropout_rate=r) for d, ln, a, r in zip(
        (cfg.critic_dims, cfg.policy_dims), (cfg.critic_layer_norm, cfg.policy_layer_norm), (cfg.critic_activation, cfg.policy_activation), rates)]
    return pinit.network_spec(nets[0], nets[1], dict(MS.POLICY_KWARGS, **over.pop("pk", {})), cfg.A, mlp_dropout=mode,
                              use_proprio=cfg.use_proprio, **_KW, **over)


@pytest.mark.parametrize("name", list(DS.CASES))
def test_any_accepts_what_true_refuses_in_its_own_words(name):
    spec = _spec(name, "any")
    assert spec.dropout_any and spec.to_c().dropout_any == 1 and spec.config_entries()["dropout_any"] is True
    assert pinit.NetSpec().to_c().dropout_any == 0 and "dropout_any" not in pinit.NetSpec().config_entries()
    # mlp_dropout=True refuses in the words of NetSpec.check (utils/init.py) on the same options without the switch
    with pytest.raises(NotImplementedError) as want:
        dataclasses.replace(spec, dropout_any=False).check()
    with pytest.raises(NotImplementedError) as got:
        _spec(name, True)
    assert str(got.value) == str(want.value) and "mlp_dropout=True" in str(got.value)


def test_what_any_still_refuses():
    with pytest.raises(NotImplementedError, match="std_parameterization='fixed'"):
        _spec("shapes", "any", policy_fixed=True, pk={"std_parameterization": "fixed", "fixed_std": 0.1})
    for rate in (1.0, 1.5):      # (a rate <= 0 means no Dropout, as mlp.py reads it)
        with pytest.raises(NotImplementedError, match="dropout_rate"):
            pinit.network_spec(MS.mlp_kwargs((64, 64), dropout_rate=rate), MS.mlp_kwargs((64, 64)), dict(MS.POLICY_KWARGS), 4, mlp_dropout="any", **_KW)
    with pytest.raises(ValueError, match="mlp_dropout must be False, True or 'any'"):
        _spec("shapes", "maybe")


def test_header_and_binding_table():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "serl_mi355.h")).read()
    assert re.search(r"int dropout_any;", header) and "int serl_agent_dropout_any(serl_agent* a);" in header
    assert "serl_agent_dropout_any" in _lib_agent.SIGNATURES and ("dropout_any", _lib_agent.C.c_int) in _lib_agent.SerlAgentOpts._fields_


@pytest.mark.parametrize("name", list(DS.CASES))
def test_the_oracle_uses_one_mask_per_site_and_layer_and_keeps_relu_off_the_kink(name):
    with DS.installed():
        for call in DS.calls_of(name):
            run = DS.oracle_run(name, call)      # (oracle_dropout asserts that the queue is used up)
            assert all(m >= MP.RELU_MARGIN for m in run["relu"]), (name, call, min(run["relu"]))
