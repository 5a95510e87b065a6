"""CPU: action widths above 64 (wide_actions=True, serl_agent_opts.wide_actions): what the arguments alone
decide on both sides of the C ABI.  All but the refusal without the switch fail on a tree that lacks it."""
import pytest

from serl_amd.utils import init as pinit
from serl_amd.utils.init import NetSpec
from test_agent_opts_cpu import SERL_ERR_INVALID, _cfg, _create


def _with_act_dim(A):
    cfg = _cfg()
    cfg.act_dim = A
    return cfg


@pytest.mark.parametrize("A,switch,sent", [(7, True, 0), (64, True, 0), (65, True, 1), (256, True, 1), (65, False, 0)])
def test_the_spec_carries_the_switch_where_the_width_needs_it(A, switch, sent):
    spec = pinit.network_spec(None, None, None, A, wide_actions=switch)
    o = spec.to_c()
    assert spec.wide_actions == bool(sent) == spec.core_kwargs()["wide_actions"] and o.wide_actions == sent and NetSpec().to_c().wide_actions == 0
    rc, msg = _create(o, _with_act_dim(A))      # (made and destroyed where a device is present; a device error where none is)
    if A > 64 and not switch:
        assert rc == SERL_ERR_INVALID and "bad dims" in msg, (rc, msg)      # refused as always
    else:
        assert rc != SERL_ERR_INVALID, (rc, msg)


def test_refusals_from_the_arguments_alone():
    with pytest.raises(NotImplementedError, match=r"action_dim 257 under wide_actions=True \(served: 1 to 256"):
        pinit.network_spec(None, None, None, 257, wide_actions=True)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="wide_actions must be a bool"):
            pinit.network_spec(None, None, None, 4, wide_actions=bad)
    rc, msg = _create(NetSpec(wide_actions=True).to_c(), _with_act_dim(257))
    assert rc == SERL_ERR_INVALID and "act_dim 257 with wide_actions 1: served are 1 to 256" in msg, (rc, msg)
    o = NetSpec().to_c()
    o.wide_actions = 2
    rc, msg = _create(o)
    assert rc == SERL_ERR_INVALID and "wide_actions 2 is not 0" in msg, (rc, msg)


@pytest.mark.parametrize("A,switch,what", [(65, 0, "act_dim 65 unsupported"), (257, 1, "act_dim 257 with wide_actions 1"), (4, 2, "wide_actions 2 is not 0")])
def test_the_bc_library_refuses_alike(A, switch, what):
    import ctypes as C
    from serl_amd import _lib
    from serl_amd._lib_agent import SerlBcCfg, SerlBcOpts
    L, h = _lib.lib(), C.c_void_p()
    rc = int(L.serl_bc_create_wide(C.byref(SerlBcCfg(0, 1, 64, 64, 5, A, 8, 3e-4, 0.1, 1e-5, 5.0)), C.byref(SerlBcOpts(0)), switch, C.byref(h)))
    assert rc == SERL_ERR_INVALID and what in (L.serl_last_error() or b"").decode(), (rc, L.serl_last_error())

