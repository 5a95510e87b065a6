"""CPU: MLP widths above 1024 (mlp_wide=True, serl_agent_opts.wide_widths): what the arguments alone decide on both sides of the C
ABI, and the relu condition of the GPU case table (tests/mlp_wide.py).  All but the last fail on a tree without the switch."""
import pytest

import mlp_plain as MP
import mlp_shapes as MS
import mlp_wide as MW
from serl_amd.utils import init as pinit
from serl_amd.utils.init import NetSpec
from test_agent_opts_cpu import SERL_ERR_INVALID, _cfg, _create


def _spec(dims, **kw):
    return pinit.network_spec(MS.mlp_kwargs(dims, **kw.pop("extra", {})), MS.mlp_kwargs(kw.pop("pd", [64])), None, 4, mlp_shapes=True, **kw)


@pytest.mark.parametrize("w,ragged,ok", [(4096, False, True), (1088, False, True), (4160, False, False), (1100, False, False),
                                         (1100, True, True), (4097, True, False)])
def test_the_switch_ends_the_widths_at_4096(w, ragged, ok):
    if not ok:
        with pytest.raises(NotImplementedError, match=rf"width {w} in .*4096\D.*mlp_wide=True"):
            _spec([64, w], mlp_wide=True, mlp_ragged=ragged)
        return
    spec = _spec([64, w], mlp_wide=True, mlp_ragged=ragged)
    o = spec.to_c()
    assert spec.wide and spec.core_kwargs()["wide"] and (o.wide_widths, o.ragged_widths, o.critic.dims[1]) == (1, int(ragged), w)
    assert _create(o)[0] != SERL_ERR_INVALID      # (made and destroyed where a device is present; a device error where none is)
    o.critic.dims[1] = 4097 if ragged else 4160
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and f"critic MLP: layer 2 has width {o.critic.dims[1]} (served with wide_widths 1" in msg and "4096] wide" in msg, msg


def test_without_the_switch_the_old_messages_come_back_and_dropout_is_refused_with_it():
    with pytest.raises(NotImplementedError, match=r"width 1088 in hidden_dims=\[64, 1088\] is off the grid \(served: .* a multiple of 64 in \[64, 1024\],"):
        _spec([64, 1088])
    with pytest.raises(NotImplementedError, match=r"is outside \[1, 1024\] \(served: .* any integer in \[1, 1024\] under mlp_ragged=True,"):
        _spec([64, 1100], mlp_ragged=True)
    assert _spec([64, 1024], mlp_wide=True) == _spec([64, 1024]) and NetSpec().to_c().wide_widths == 0      # up to 1024: the call without
    rc, msg = _create(NetSpec(critic_dims=(1088,), policy_dims=(64,)).to_c())
    assert rc == SERL_ERR_INVALID and "critic MLP: layer 1 has width 1088 (served: 1 to 4 layers, each a multiple of 64 in [64, 1024] wide)" in msg, msg
    rc, msg = _create(NetSpec().to_c(), _cfg(hidden=2048))
    assert rc == SERL_ERR_INVALID and "hidden must be a multiple of 64 in [64, 1024] (got 2048)" in msg, msg
    with pytest.raises(NotImplementedError, match="mlp_wide=True with mlp_dropout=True and a positive dropout_rate .* beside the width 2048"):
        _spec([64, 64], pd=[2048, 64], extra=dict(dropout_rate=0.1), mlp_dropout=True, mlp_wide=True)
    o = NetSpec(hidden=2048, wide=True).to_c()
    o.critic.dropout = 0.1
    rc, msg = _create(o, _cfg(hidden=2048))
    assert rc == SERL_ERR_INVALID and "beside an MLP width of 2048 under wide_widths 1" in msg and "dropout 0.1" in msg, msg


def test_relu_pre_activations_of_the_case_table_keep_the_margin():
    name = "w3_plain_relu_critic_2048_one_row"
    with MW.installed():
        for call in MW.case_config(name)[2]:
            relu = MW.oracle_run(name, call)["relu"]
            assert relu and min(relu) >= MP.RELU_MARGIN, (call, min(relu))
