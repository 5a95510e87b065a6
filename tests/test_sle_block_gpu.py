"""GPU: the sample-blocked SpatialLearnedEmbeddings forward (heads.hip sle_proprio_fwd_kernel: SLE_BLOCK samples per workgroup
above 64 rows, pixels in chunks) against the un-blocked sle_fwd_kernel, which the one-launch-per-operation chain
(SERL_CHAIN_FUSE=0) runs.  Both sum a sample's pixels in ascending order, so everything downstream agrees TO THE BIT.

One camera of 84x84 frames gives a 3x3 SLE: 9 pixels are no multiple of the pixel chunk, so the chunk's clamp is exercised.  The
row counts sit just over the 64-row switch to the blocked path, with last blocks of 1, 2 and SLE_BLOCK - 1 samples (the
branch-free sample clamp).  A last case draws the Dropout mask inside the kernel from the call's keys, against the same draws
supplied as a mask tensor (tests/test_call_noise_gpu.py holds the two forms to each other at 16 rows, on the two-sample path); it
samples from a replay store, whose frame rows are multiples of 16 bytes, so its frames are 80x80 -- a 3x3 SLE as well."""
import itertools

import numpy as np
import pytest
import torch

from helpers import make_spaces
from oracle import drq_oracle as O
import agent_helpers as AH

pytestmark = pytest.mark.gpu
SLE_BLOCK = 4                      # samples per workgroup of the path above 64 rows (heads.hip sle_proprio_fwd_multi)
ROWS = sorted({64 + 1, 64 + 2, 64 + SLE_BLOCK - 1})
KEYS, H, W, S, A = ("wrist",), 84, 84, 7, 5
HS = WS = 80                       # frames of the replay-store case: 80 * 3 bytes per row; 80 -> 40 -> 20 -> 10 -> 5 -> 3


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _taps(cfg, B):
    sl, _ = AH.leaf_slices(cfg)
    return (("x", B * (cfg.enc_dim + cfg.A)), ("x_target", B * (cfg.enc_dim + cfg.A)), ("g_critic", sl["enc/proprio/ln/bias"][1]),
            ("g_actor", sl["actor/logstd/bias"][1] - sl["enc/proprio/dense/kernel"][0]), ("scalars", 8))


@pytest.mark.parametrize("B", ROWS)
def test_blocked_sle_forward_equals_the_unblocked_kernel(gpu, B):
    cfg = O.Config(image_keys=KEYS, H=H, W=W, S=S, A=A)
    fused, plain = AH.make_pair(cfg, B, fuse=True)[1], AH.make_pair(cfg, B, fuse=False)[1]
    b = AH.synth_batch(cfg, B, seed=21)
    noise = O.make_noise(cfg, B, seed=22, utd_ratio=1)
    for core in (fused, plain):
        db, dn = AH.batch_to_device(cfg, b), AH.noise_to_device(cfg, noise)
        core.update_critics(db, dn)
        core.update_high_utd(db, 1, dn)
        torch.cuda.synchronize()
    for tap, n in _taps(cfg, B):
        f, p = fused.debug(tap, n), plain.debug(tap, n)
        assert np.abs(p).max() > 0, tap
        assert _bits_equal(f, p), (B, tap, AH.rel_err(f, p))


def _agent_taps(form, B):
    """-> the taps after one update_critics + update_high_utd(1) of a fresh agent on a fresh store, Dropout masks in `form`"""
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.utils.launcher import make_drq_agent
    from serl_amd.utils.synthetic import transition_stream
    osp, asp = make_spaces(KEYS, HS, WS, 3, 1, S, A)
    rb = MemoryEfficientReplayBufferDataStore(osp, asp, 200, image_keys=KEYS)
    rb.seed(0)
    for tr in itertools.islice(transition_stream(KEYS, HS, WS, 3, 1, S, A, 20, 1), 120):
        rb.insert(tr)
    obs = {k: np.zeros((1, HS, WS, 3), np.uint8) for k in KEYS}
    obs["state"] = np.zeros((1, S), np.float32)
    agent = make_drq_agent(5, obs, np.zeros((A,), np.float32), image_keys=KEYS, encoder_type="resnet-pretrained", batch_size=B)
    agent.noise_form = form
    it = rb.get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True, "lazy": True})
    agent.update_critics(next(it))
    agent.update_high_utd(next(it), utd_ratio=1)
    torch.cuda.synchronize()
    cfg = O.Config(image_keys=KEYS, H=HS, W=WS, S=S, A=A)
    return {tap: agent.core.debug(tap, n).copy() for tap, n in _taps(cfg, B)}


def test_masks_drawn_from_keys_in_the_blocked_kernel_equal_the_mask_tensor(gpu):
    B = 64 + SLE_BLOCK - 1
    keys, tensors = _agent_taps("keys", B), _agent_taps("tensors", B)
    for tap in keys:
        assert np.abs(tensors[tap]).max() > 0, tap
        assert _bits_equal(keys[tap], tensors[tap]), (tap, AH.rel_err(keys[tap], tensors[tap]))
