"""The float64 restatements of tests/entropy_ref.py against the fp32 oracle (to fp32 accuracy) and scipy's survival-function form, the
structure of the Philox restatement, and every property of the seeded inputs that tests/test_gpu_entropy_direct.py relies on: no
likelihood in the floor window, the rounding margin, the exact ties, the sigma cases, floor elements under the negative bit weight, and
the size / dispatch arithmetic each case claims.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle import crdr_oracle as O
from tests import entropy_ref as R


def _d(t):
    return t.double()


# ---- restatements ----------------------------------------------------------------------------------------------------------------------

def test_bounds_are_the_fp32_values():
    assert R.SCALE_BOUND == float(np.float32(0.11)) != 0.11 and R.LIK_BOUND == float(np.float32(1e-9)) != 1e-9


def test_gaussian_restatement_matches_oracle_and_scipy():
    from scipy.stats import norm
    d = R.gc_case("gcd.small.cl.6", *R.gc_shape("small", 6))
    y, mu, sg, nz = d["y"], d["mu"], d["sigma"], d["noise"]
    for noise in (nz, None):
        yh64, l64 = R.gaussian_conditional(_d(y), _d(mu), _d(sg), None if noise is None else _d(noise))
        yh32, l32 = O.gaussian_conditional(y, mu, sg, noise)
        assert (yh64 - yh32).abs().max().item() <= 2.0 ** -23 * yh64.abs().max().item()
        # fp32 erfc: relative in the tail, 2^-24-ish absolute where the two erfc values are O(1)
        assert bool(((l64 - l32).abs() <= 5e-6 * l64 + 4e-7).all())
        assert bool(((l64 == R.LIK_BOUND) == (l32.double() == R.LIK_BOUND)).all())
        b64, b32 = R.bits_per_image(l64), O.bits_per_image(l32)
        assert ((b64 - b32).abs() / b64).max().item() <= 1e-5
        v = (yh64 if noise is None else _d(y) + _d(noise)) - _d(mu)
        a, s = v.abs().numpy(), np.maximum(_d(sg).numpy(), R.SCALE_BOUND)
        sf = np.maximum(norm.sf((a - 0.5) / s) - norm.sf((a + 0.5) / s), R.LIK_BOUND)
        assert np.all(np.abs(l64.numpy() - sf) <= 1e-9 * sf + 1e-16)
    # the same restatement evaluated in fp32 is the oracle's function of the fp32 operands
    assert torch.equal(R.gaussian_conditional(y, mu, sg, nz)[1], O.gaussian_conditional(y, mu, sg, nz)[1])


@pytest.mark.parametrize("c", [1, 6])
def test_eb_restatement_matches_oracle(c):
    sd, d = R.eb_case(c, 48)
    sd64 = R.as_dtype(sd, torch.float64)
    for noise in (d["noise"], None):
        zh64, l64 = R.entropy_bottleneck(sd64, _d(d["z"]), None if noise is None else _d(noise))
        zh32, l32 = O.entropy_bottleneck(sd, R.EB, d["z"], noise)
        assert (zh64 - zh32).abs().max().item() <= 2.0 ** -23 * zh64.abs().max().item()
        assert (l64 - l32).abs().max().item() <= 2e-5 * l64.max().item()
        assert ((R.bits_per_image(l64) - O.bits_per_image(l32)).abs() / R.bits_per_image(l64)).max().item() <= 2e-5
    a64, a32 = R.eb_aux_loss(sd64), O.eb_aux_loss(sd, R.EB)
    assert abs(a64.item() - a32.item()) <= 2e-5 * a64.item()


@pytest.mark.parametrize("levels", R.SYMBOL_LEVELS)
def test_symbol_restatement_and_inputs(levels):
    y, mu, sg, table = R.symbol_case(levels)
    assert table.numel() == levels and table.dtype == torch.float32
    assert torch.equal(R.build_indexes(_d(sg), _d(table)), O.build_indexes(sg, table, float(np.float32(0.11))))
    idx = R.build_indexes(_d(sg), _d(table))
    assert idx.min().item() == 0 and idx.max().item() == levels - 1
    # exact in fp32, ties of both parities, sigma exactly on table entries, at the bound and below it
    v = _d(y) - _d(mu)
    assert torch.equal((y - mu).double(), v)
    tie = (v - torch.floor(v)) == 0.5
    assert bool((tie & (torch.floor(v) % 2 == 0)).any()) and bool((tie & (torch.floor(v) % 2 == 1)).any())
    assert int(torch.isin(sg, table).sum()) >= min(levels, 40) and bool((sg == float(np.float32(0.11))).any()) and bool((sg < 0.11).any())
    assert torch.equal(R.symbols(_d(y), _d(mu)), torch.round(v).int())


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------

def test_philox_known_answer_and_structure():
    # Random123's known answer for counter = key = 0 (kat_vectors: philox4x32 10 rounds)
    w = R.philox4x32_10(np.zeros(1, dtype=np.uint64), 0)
    assert [int(v[0]) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    n, hw, c = 2, 7, 12
    full = R.philox_uniform(R.PHILOX_SEED, R.PHILOX_OFFSET, n, hw, c)
    assert full.dtype == torch.float32 and full.min().item() >= -0.5 and full.max().item() < 0.5
    # a channel slice equals the full tensor at those channels (any offset, any width)
    for c0, cs in ((4, 4), (3, 5), (0, 1), (7, 5)):
        assert torch.equal(R.philox_uniform(R.PHILOX_SEED, R.PHILOX_OFFSET, n, hw, cs, c, c0), full[:, c0:c0 + cs])
    # idx and idx + 1 within one group of four share a counter and take consecutive words; the next group moves the counter by one
    grp, lane = R.philox_counter_lane(n, hw, c)
    flat_g, flat_l = grp.transpose(0, 2, 1).reshape(-1), lane.transpose(0, 2, 1).reshape(-1)   # element order (n, px, c) = idx order
    assert np.array_equal(flat_l, np.arange(flat_l.size) % 4) and np.array_equal(flat_g, np.arange(flat_g.size, dtype=np.uint64) // 4)
    # the counter carries into its second word: offset + idx / 4 crosses 2^32 inside the tensor
    assert R.PHILOX_OFFSET < (1 << 32) <= R.PHILOX_OFFSET + int(flat_g[-1]) and (R.PHILOX_SEED >> 32) != 0
    # samples are multiples of 2^-24: the float32 tensor holds them exactly
    assert torch.equal(full.double() * 2 ** 24, torch.round(full.double() * 2 ** 24))
    assert abs(R.philox_uniform(1234, 0, 4, 1024, 32).mean().item()) < 5e-3


# ---- gauss_cond inputs -------------------------------------------------------------------------------------------------------------------

def _check_gc_case(d, n):
    ln, lq = R.gc_raw_likelihoods(d)
    assert not bool(R.in_window(ln).any()) and not bool(R.in_window(lq).any())                  # the floor window is empty
    assert R.round_margin(_d(d["y"]) - _d(d["mu"])) >= R.ROUND_MARGIN                             # rounding margin
    assert d["noise"].min().item() >= -0.5 and d["noise"].max().item() < 0.5
    sg = d["sigma"].view(-1)
    b = np.float32(0.11)
    assert sg[0].item() == float(b) == R.SCALE_BOUND and sg[1].item() == float(np.nextafter(b, np.float32(1)))
    assert sg[2].item() == float(np.nextafter(b, np.float32(0))) and 0 < sg[3].item() < R.SCALE_BOUND and sg[4].item() < 0
    g = d["gbits"]
    assert g.numel() == n and int((g < 0).sum()) == 1 and (n == 1 or int((g > 0).sum()) == n - 1)
    neg = int(torch.argmin(g))
    assert bool((ln[neg] < R.WINDOW[0]).any()) and bool((ln[neg] > R.WINDOW[1]).any())         # floor elements and others under the negative weight
    for i in range(n):
        assert bool((ln[i] < R.WINDOW[0]).any()) and bool((lq[i] < R.WINDOW[0]).any())
    # below the scale bound the gradient that reaches the scale LowerBound has either sign (blocked and passed elements both exist) and
    # is never within the margin of a change of sign
    gs, low = R.gc_scale_grad(d), d["sigma"].double() < R.SCALE_BOUND
    assert bool((low & (gs > 0)).any()) and bool((low & (gs < 0)).any())
    assert not bool((low & (ln > R.WINDOW[1]) & (gs.abs() < R.SIGMA_GRAD_MARGIN)).any())


@pytest.mark.parametrize("size,cases", [("small", R.GC_SMALL), ("medium", R.GC_MEDIUM)])
def test_gc_cases_have_the_properties_the_gpu_tests_rely_on(size, cases):
    for c in sorted({c for _, c in cases}):
        n, _, h, w = R.gc_shape(size, c)
        _check_gc_case(R.gc_case(f"gcd.{size}.{c}", n, c, h, w), n)
        blocks = R.gc_blocks(h * w, c)
        if size == "small":
            assert h * w * c <= 1024 and blocks == 1
        else:
            assert 3 <= blocks <= 5 and (h * w * c) % 1024 != 0 and (h * w * c) % 256 != 0
        # (a block covers 1024 elements of its image per pass with four channels per thread, 256 with one)
        vec = c % 4 == 0
        assert R.fwd_passes(h * w, c, vec) == (1 if vec else min(4, -(-h * w * c // 256))) and R.bwd_passes(n, h * w, c, vec) == 1
    for kind, c in cases:
        assert kind in R.GC_KINDS and (kind != "padded" or c == 3)


def test_gc_big_cases_reach_the_second_passes():
    (n, c, h, w), (n2, c2, h2, w2) = R.GC_BIG
    # vector: per_img = 2 105 352 > 2048 x 1024, so the forward strides and the finish kernel sees 2048 > 256 partials per image;
    # total / 4 = 1 052 676 > 4096 x 256, so the backward strides
    assert R.gc_vector(c) and h * w * c == 2105352 > 2048 * 1024 and R.gc_blocks(h * w, c) == 2048 > 256
    assert n * h * w * c // 4 == 1052676 > 4096 * 256
    assert R.fwd_passes(h * w, c, True) == 2 and R.bwd_passes(n, h * w, c, True) == 2
    # scalar: C = 3; total = 1 053 366 > 4096 x 256, the backward strides (the scalar forward strides at every size above 256 elements)
    assert not R.gc_vector(c2) and n2 * h2 * w2 * c2 == 1053366 > 4096 * 256
    assert R.bwd_passes(n2, h2 * w2, c2, False) == 2 and R.gc_blocks(h2 * w2, c2) == 515 > 256
    # one element less in either direction and the loops run once: these are the smallest square sizes
    assert R.bwd_passes(n, 512 * 512, c, True) == 1 and R.bwd_passes(n2, 418 * 418, c2, False) == 1


def test_gc_dispatch_arithmetic():
    assert R.gc_vector(32, lds=(40, 40, 40), offsets=(4, 4, 4)) and not R.gc_vector(6, lds=(16,), offsets=(4,))
    assert not R.gc_vector(8, lds=(20,), offsets=(3,)) and not R.gc_vector(8, lds=(18,)) and not R.gc_vector(8, ctot=20, c0=6)
    assert R.gc_vector(8, ctot=20, c0=8)
    assert [R.gc_blocks(1, 1), R.gc_blocks(1024, 1), R.gc_blocks(1025, 1), R.gc_blocks(513 * 513, 8)] == [1, 1, 2, 2048]


def test_gc_big_case_inputs():
    n, c, h, w = R.GC_BIG[1]
    _check_gc_case(R.gc_case("gcd.big.3", n, c, h, w), n)


def test_gc_grid_case_is_exact_with_ties_on_both_parities():
    g = R.gc_grid_case("gcd.grid.6", 3, 6, 5, 5)
    y, mu = g["y"], g["mu"]
    assert torch.equal(y * 16, torch.round(y * 16)) and torch.equal(mu * 16, torch.round(mu * 16)) and max(y.abs().max(), mu.abs().max()) < 128
    v = _d(y) - _d(mu)
    assert torch.equal((y - mu).double(), v)                                         # y - mu is exact in fp32
    q = torch.round(v)
    assert torch.equal((q.float() + mu).double(), q + _d(mu))                        # and so is round(y - mu) + mu
    tie = (v - torch.floor(v)) == 0.5
    even, odd = tie & (torch.floor(v) % 2 == 0), tie & (torch.floor(v) % 2 == 1)
    assert int(even.sum()) >= 4 and int(odd.sum()) >= 4 and bool((v[tie] > 0).any()) and bool((v[tie] < 0).any())
    assert torch.equal(q[even], torch.floor(v)[even]) and torch.equal(q[odd], torch.floor(v)[odd] + 1)   # half to even


# ---- entropy bottleneck inputs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.EB_CHANNELS)
def test_eb_cases_have_the_properties_the_gpu_tests_rely_on(c):
    for nhw in R.EB_SIZES:
        for grid in (False, True):
            sd, d = R.eb_case(c, nhw, grid)
            n, _, h, w = d["z"].shape
            assert n * h * w == nhw and n == (3 if nhw % 3 == 0 else 1) and d["gbits"].numel() == n
            sd64 = R.as_dtype(sd, torch.float64)
            med = sd64[R.EB + ".quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
            ln = R.eb_likelihood(sd64, _d(d["z"]) + _d(d["noise"]), raw=True)
            lq = R.eb_likelihood(sd64, R.entropy_bottleneck(sd64, _d(d["z"]))[0], raw=True)
            assert not bool(R.in_window(ln).any()) and not bool(R.in_window(lq).any())
            assert R.round_margin(_d(d["z"]) - med) >= R.ROUND_MARGIN
            assert d["noise"].min().item() >= -0.5 and d["noise"].max().item() < 0.5
            assert not bool(torch.equal(med * 16, torch.round(med * 16)))                        # medians off the grid
            if grid:
                assert torch.equal(d["z"] * 16, torch.round(d["z"] * 16))
            if nhw >= 48:
                assert bool((ln < R.WINDOW[0]).any()) and ln.max().item() > 0.1                   # saturated tails and the centre
                if n == 3 or d["gbits"][0] < 0:
                    neg = 1 if n == 3 else 0
                    assert d["gbits"][neg] < 0
                    assert bool((ln[neg] < R.WINDOW[0]).any(-1).any(-1).all()) and bool((ln[neg] > R.WINDOW[1]).any(-1).any(-1).all())
    assert [R.eb_shape(c, s)[0] for s in R.EB_SIZES] == [1, 3, 3, 1, 1, 1]


def test_aux_sizes():
    assert [3 * c > 256 for c in R.AUX_CHANNELS] == [False, False, True, True] and 3 * 86 == 258
