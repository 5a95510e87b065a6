"""The product's JAX PRNG (serl_amd/csrc/jaxrng.hip through serl_amd/jaxrng.py) against oracle/jaxshim/jax/threefry.py, which is
pinned on the Random123 known-answer vectors and the values of JAX's documentation (tests/test_threefry_oracle.py).
CPU part: every host entry point (keys, integers: BIT-EXACT; host normals: within 1e-5 relative of the oracle's float64 erf_inv)
and the key schedule of one learner call (agents/continuous/drq.py:276-318, sac.py:137,151,197,222,287-289, common/common.py:197-200)
against the same schedule written out with the oracle's split.  GPU part: the device draws."""
import numpy as np
import pytest

from oracle.jaxshim.jax import threefry as T
from serl_amd import jaxrng as J


def test_threefry_known_answers_through_the_library():
    # Random123 KAT for threefry2x32-20: key (0, 0), counter (0, 0); all-ones; the pi digits
    for key, ctr, want in (((0, 0), (0, 0), (0x6B200159, 0x99BA4EFE)),
                           ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x1CB996FC, 0xBB002BE7)),
                           ((0x13198A2E, 0x03707344), (0x243F6A88, 0x85A308D3), (0xC4923A9C, 0x483DF7A0))):
        # random_bits over n = 2 hashes the counter pair (0, 1); the KAT counters need the raw block: fold_in gives (0, data)
        got = T.threefry2x32(key[0], key[1], np.array([ctr[0]], np.uint32), np.array([ctr[1]], np.uint32))
        assert (int(got[0][0]), int(got[1][0])) == want          # the oracle itself (pinned elsewhere too)
    # the library's block function through fold_in: counter (0, data)
    for key, data in (((0, 0), 0), ((0x13198A2E, 0x03707344), 0x85A308D3), ((1, 2), 12345)):
        assert np.array_equal(J.fold_in(np.array(key, np.uint32), data), T.fold_in(np.array(key, np.uint32), data))


def test_keys_and_integers_are_bit_exact():
    rng = np.random.default_rng(0)
    for seed in (0, 1, 42, 2**31 - 1, 2**32 + 7, -1):
        k = J.prngkey(seed)
        assert np.array_equal(k, T.PRNGKey(seed))
        for num in (1, 2, 3, 4, 7, 256):
            assert np.array_equal(J.split(k, num), T.split(k, num)), (seed, num)
        for n in (1, 2, 3, 5, 8, 1001):
            assert np.array_equal(J.random_bits(k, n), T.random_bits(k, (n,))), (seed, n)
        for lo, hi in ((0, 9), (0, 10), (-3, 4), (0, 1), (5, 5), (0, 2**31 - 1), (-2**31, 2**31 - 1)):
            for n in (1, 2, 3, 16):
                assert np.array_equal(J.randint(k, n, lo, hi), T.randint(k, (n,), lo, hi)), (seed, lo, hi, n)
        d = int(rng.integers(0, 2**32))
        assert np.array_equal(J.fold_in(k, d), T.fold_in(k, d))


def test_prngkey_follows_jax_with_x64_disabled():
    """jax._src.prng.threefry_seed on an int32 seed (the reference never enables x64): high word 0, low word the seed's 32 bits
    (a 64-bit split of the seed started the learner from another state.rng for seed = -1 or seed >= 2**32)."""
    for seed, want in ((0, [0, 0]), (42, [0, 42]), (-1, [0, 0xFFFFFFFF]), (2**32 + 5, [0, 5]), (2**31, [0, 2**31])):
        assert J.prngkey(seed).tolist() == want
        assert T.PRNGKey(seed).tolist() == want


def test_randint_multiplier_wraps_in_uint32_for_large_spans():
    """jax._src.random._randint: multiplier = (2**16 % span)**2 % span with lax.mul on uint32, which WRAPS (the product
    was taken in 64 bits).  span = 2**31 - 1: 65536**2 = 2**32 wraps to 0, so a draw is minval + lower_bits % span -- checked
    from the raw bits, independently of both randint implementations; span = 100000: (65536**2 mod 2**32) % span = 0 as well,
    span = 70000: 65536 % 70000 = 65536 again."""
    k = T.PRNGKey(123)
    k1, k2 = T.split(k)
    n = 64
    lb = T.random_bits(k2, (n,)).astype(np.uint64)
    for lo, span in ((0, 2**31 - 1), (-5, 100000), (7, 70000)):
        want = (lo + (lb % np.uint64(span)).astype(np.int64)).astype(np.int32)
        assert np.array_equal(J.randint(k, n, lo, lo + span), want), span
        assert np.array_equal(T.randint(k, (n,), lo, lo + span), want), span
    # a span below 2**16 keeps a non-zero multiplier: hb contributes
    hb = T.random_bits(k1, (n,)).astype(np.uint64)
    span = np.uint64(1000)
    mult = (np.uint64(65536) % span) ** 2 % span
    want = (((hb % span) * mult + lb % span) % span).astype(np.int32)
    assert np.array_equal(J.randint(k, n, 0, 1000), want)


def test_update_keys_chain_beyond_the_struct_capacity():
    """utd_ratio > SERL_JAX_MAX_UTD (the reference takes any divisor of the batch, sac.py:544-596): the schedule is a chain, so 40
    critic updates + the actor update = the 40-update prefix of the same rng followed by the rest."""
    rng = T.split(T.PRNGKey(17))[0]
    big = J.UpdateKeys(rng, True, 40, True)
    head = J.UpdateKeys(rng, True, 32, False)
    tail = J.UpdateKeys(head.rng_out, False, 8, True)
    assert len(big.k_next_action) == 40 and len(big.k_subsample) == 40
    for i in range(32):
        assert np.array_equal(big.k_next_action[i], head.k_next_action[i]) and np.array_equal(big.k_subsample[i], head.k_subsample[i])
    for i in range(8):
        assert np.array_equal(big.k_next_action[32 + i], tail.k_next_action[i]) and np.array_equal(big.k_subsample[32 + i], tail.k_subsample[i])
    assert np.array_equal(big.k_obs, head.k_obs) and np.array_equal(big.k_policy, tail.k_policy) and np.array_equal(big.k_temp, tail.k_temp)
    assert np.array_equal(big.rng_out, tail.rng_out)
    # and the written-out schedule: 41 x (rng = split(rng)[0]) after the 3-way augmentation split
    r = T.split(rng, 3)[0]
    for _ in range(41):
        r = T.split(r)[0]
    assert np.array_equal(big.rng_out, r)


def test_crop_offsets_follow_batched_random_crop():
    # vision/data_augmentations.py:22-36: rngs = split(rng, frames); per frame randint(rng_i, (2,), 0, 2 * padding + 1) = (y, x)
    for seed, frames in ((3, 1), (4, 8), (5, 256)):
        k = T.PRNGKey(seed)
        want = np.stack([T.randint(ki, (2,), 0, 9) for ki in T.split(k, frames)])
        got = J.crop_offsets(k, frames, 4)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert got.min() >= 0 and got.max() <= 8


def test_create_rng_and_crop_pair_are_the_chains_they_name():
    """state.rng after create (rng, init_rng = split(rng); rng, create_rng = split(rng)) and the crop keys of a DrQ call
    (rng, obs_rng, next_obs_rng = split(rng, 3)), shared by the agents and the learners"""
    for seed in (0, 3, 2**31 + 7):
        rng = J.split(J.split(J.prngkey(seed))[0])[1]
        assert np.array_equal(J.create_rng(seed), rng)
        assert np.array_equal(J.create_rng(J.prngkey(seed)), rng)                   # a key is taken as it is
        co, cn = J.crop_pair(rng, 7)
        k = J.split(rng, 3)
        assert np.array_equal(co, J.crop_offsets(k[1], 7, 4)) and np.array_equal(cn, J.crop_offsets(k[2], 7, 4))
        assert co.shape == cn.shape == (7, 2) and not np.array_equal(co, cn)


def test_host_normals_are_within_a_few_ulps_of_the_oracle():
    k = T.PRNGKey(7)
    for n in (1, 6, 1537):
        got, want = J.normal_host(k, n), T.normal(k, (n,))
        # same 32-bit draws, same uniform; erf_inv: XLA's float32 formula here (Giles' polynomial on w = -log1p(-u*u) evaluated in
        # float32: a few 1e-7 in the centre, up to 6e-6 for |x| > 3 where 1 - u*u cancels -- which IS what a JAX run computes),
        # float64 scipy rounded to float32 in the oracle
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= 1e-5 * np.abs(want) + 2e-7).all(), float((err / (np.abs(want) + 1e-30)).max())


def _schedule_by_hand(rng, drq_aug, n_critic, has_actor, combined=False):
    out = {}
    if drq_aug:
        rng, out["k_obs"], out["k_next"] = T.split(rng, 3)
    out["k_next_action"], out["k_subsample"] = [], []
    for u in range(1 if combined else n_critic + (1 if has_actor else 0)):
        _, r_actor, r_critic, r_temp = T.split(rng, 4)
        if u < n_critic:
            c, k_na = T.split(r_critic)
            _, k_sub = T.split(c)
            out["k_next_action"].append(k_na)
            out["k_subsample"].append(k_sub)
        if combined or u >= n_critic:
            _, out["k_policy"], out["k_sample"], _ = T.split(r_actor, 4)
            _, out["k_temp"] = T.split(r_temp)
        rng = T.split(rng)[0]
    out["rng_out"] = rng
    return out


@pytest.mark.parametrize("drq_aug,n_critic,has_actor,combined", [(1, 1, 0, 0), (1, 1, 1, 0), (1, 4, 1, 0), (0, 2, 1, 0), (0, 0, 1, 0),
                                                                  (0, 1, 0, 0), (0, 1, 1, 1)])
def test_update_key_schedule(drq_aug, n_critic, has_actor, combined):
    rng = T.split(T.PRNGKey(11))[1]
    want = _schedule_by_hand(rng, drq_aug, n_critic, has_actor, combined)
    got = J.UpdateKeys(rng, drq_aug, n_critic, has_actor, combined)
    assert np.array_equal(got.rng_out, want["rng_out"])
    if drq_aug:
        assert np.array_equal(got.k_obs, want["k_obs"]) and np.array_equal(got.k_next, want["k_next"])
    for u in range(n_critic):
        assert np.array_equal(got.k_next_action[u], want["k_next_action"][u])
        assert np.array_equal(got.k_subsample[u], want["k_subsample"][u])
    if has_actor:
        for name in ("k_policy", "k_sample", "k_temp"):
            assert np.array_equal(getattr(got, name), want[name]), name


def test_flax_make_rng_equals_the_oracle_restatement():
    k = T.PRNGKey(5)
    for path, c in ((J.dropout_path("front"), 1), (("a", "b"), 2), (("modules_actor",), 300)):
        assert np.array_equal(J.flax_make_rng(k, path, c), T.flax_fold_in_static(k, tuple(path) + (c,)))


@pytest.mark.gpu
def test_device_draws(gpu):
    import torch
    k = T.PRNGKey(9)
    s = torch.cuda.current_stream().cuda_stream
    for n in (1, 6, 1536, 2 * 4096 + 1):
        nrm = torch.empty(n, dtype=torch.float32, device="cuda")
        bits = torch.empty(n, dtype=torch.int32, device="cuda")
        msk = torch.empty(n, dtype=torch.uint8, device="cuda")
        J.fill(0, [J.job(J.NORMAL, k, n, nrm.data_ptr()), J.job(J.BITS, k, n, bits.data_ptr()),
                   J.job(J.BERNOULLI_U8, k, n, msk.data_ptr(), p=0.9)], s)
        torch.cuda.synchronize()
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), T.random_bits(k, (n,)))
        assert np.array_equal(msk.cpu().numpy().astype(bool), T.bernoulli(k, 0.9, (n,)))
        got, want = nrm.cpu().numpy(), T.normal(k, (n,))
        assert (np.abs(got.astype(np.float64) - want) <= 1e-5 * np.abs(want) + 2e-7).all()
        assert np.abs(got - J.normal_host(k, n)).max() < 1e-6      # host and device libm differ in the last bits of log1p / sqrt
    # a window of a larger array (a rank's rows of a data-parallel batch, a UTD minibatch)
    n, first, count = 256 * 6, 64 * 6, 32 * 6
    win = torch.empty(count, dtype=torch.float32, device="cuda")
    J.fill(0, [J.job(J.NORMAL, k, n, win.data_ptr(), first=first, count=count)], s)
    torch.cuda.synchronize()
    full = J.normal_host(k, n)
    assert np.abs(win.cpu().numpy() - full[first:first + count]).max() < 1e-6
