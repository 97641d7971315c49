"""k_err_stats_masked through its stage call (wr_dev_err_stats_masked / _f32) against numpy and math.fsum: the maximum and the
count of compared samples exact, the sum of squares within the stated 2^-36, the same bits on every run, nothing looked at where
a bit is set (the arrays hold NaNs, infinities and huge values there, and around themselves), nothing written anywhere.

Sizes: the small ones around the 64-sample and 128-sample turns; one below, at and one above 2 * WR_RED_THREADS = 512 samples
(one block's turn) and 2^20 (one turn of the whole grid: 2048 blocks of 256 threads, two samples each); 2^18 + 3.  Arrays
aligned for two-sample loads and one element off (the element-wise form); the mask pointer 8-byte aligned and one byte off."""
import math

import numpy as np
import pytest

from util import bits_equal
from waverange_amd import api

pytestmark = pytest.mark.gpu

ACCURACY = 2.0 ** -36
BLOCK_TURN, GRID_TURN = 512, 1 << 20
SMALL = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 257, BLOCK_TURN - 1, BLOCK_TURN, BLOCK_TURN + 1]
LARGE = [(1 << 18) + 3, GRID_TURN - 1, GRID_TURN, GRID_TURN + 1]
MASKS = ["all clear", "all set but one", "alternating", "run of 128 at 0", "run of 128 at 64", "run of 128 at 37", "random 1 %", "random 50 %",
         "last bit set"]
LARGE_MASKS = ["all clear", "all set but one", "run of 128 at 37", "random 1 %", "random 50 %"]
PAD = 16  # elements in front of and behind the samples: the canaries


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def make_mask(name, n, rng):
    und = np.zeros(n, bool)
    if name == "all set but one":
        und[:] = True
        und[(2 * n) // 3] = False
    elif name == "alternating":
        und[::2] = True
    elif name.startswith("run of 128 at "):
        at = int(name.rsplit(" ", 1)[1])
        und[at:at + 128] = True
    elif name == "random 1 %":
        und = rng.random(n) < 0.01
    elif name == "random 50 %":
        und = rng.random(n) < 0.5
    elif name == "last bit set":
        und[n - 1] = True
    return und


def expected(a, b, und):
    d = a[~und].astype(np.float64) - b[~und].astype(np.float64)
    fin = np.isfinite(d)
    q = d[fin]
    return (float(np.abs(q).max()) if q.size else 0.0), int((~fin).sum()), math.fsum(q * q), int((~und).sum())


def run_case(ctx, dt, n, a, b, und, a_el, b_el, mask_off, rng, repeats):
    """a, b: the samples; the arrays on the device are PAD + a_el / b_el elements of canary, the samples, PAD of canary"""
    huge = 1e300 if dt == np.float64 else 3e38
    canary = np.array([np.nan, np.inf, -np.inf, huge], dtype=dt)

    def framed(x, el):
        full = np.tile(canary, (2 * PAD + n + 8) // 4 + 1)[:2 * PAD + n + 1].copy()
        full[PAD + el:PAD + el + n] = x
        return full

    ha, hb = framed(a, a_el), framed(b, b_el)
    nbytes = (n + 7) // 8
    packed = np.packbits(und, bitorder="little")
    if n & 7:  # the unused high bits of the last byte: the kernel must not count them, whatever they hold
        packed[-1] |= np.uint8((int(rng.integers(0, 256)) << (n & 7)) & 0xFF)
    hm = np.zeros(16 + nbytes + 32, np.uint8)  # clear bits around the mask: a byte read beyond it would add compared samples
    hm[:8 + mask_off] = 0x00
    hm[8 + mask_off:8 + mask_off + nbytes] = packed
    da, db, dm = ctx.to_device(ha), ctx.to_device(hb), ctx.to_device(hm)
    try:
        runs = [ctx.err_stats_masked(da, db, n, dm, dtype=dt, a_off=PAD + a_el, b_off=PAD + b_el, bits_offset=8 + mask_off) for _ in range(repeats)]
        back = da.download(dt, ha.size), db.download(dt, hb.size), dm.download(np.uint8, hm.size)
    finally:
        da.free(); db.free(); dm.free()
    assert back[0].tobytes() == ha.tobytes() and back[1].tobytes() == hb.tobytes() and back[2].tobytes() == hm.tobytes()
    for r in runs[1:]:
        assert all(bits_equal(np.float64(r[k]), np.float64(runs[0][k])) for k in ("max_abs", "sumsq", "rms")) and r["defined"] == runs[0]["defined"]
        assert r["nonfinite"] == runs[0]["nonfinite"]
    return runs[0]


def check(ctx, dt, n, mask, a_el, b_el, mask_off, poison, seed, repeats=3):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(dt)
    b = (a.astype(np.float64) + 1e-3 * rng.standard_normal(n)).astype(dt)
    und = make_mask(mask, n, rng)
    huge = 1e300 if dt == np.float64 else 3e38
    bad = np.resize(np.array([np.nan, np.inf, -np.inf, huge, -huge], dtype=dt), int(und.sum()))
    if poison in ("a", "both"):
        a[und] = bad
    if poison in ("b", "both"):
        b[und] = bad[::-1]
    got = run_case(ctx, dt, n, a, b, und, a_el, b_el, mask_off, rng, repeats)
    mx, nonfinite, s, nd = expected(a, b, und)
    what = (np.dtype(dt).name, n, mask, a_el, b_el, mask_off, poison, got)
    assert got["defined"] == nd and got["nonfinite"] == nonfinite == 0, (what, nd)
    assert got["max_abs"] == mx, (what, mx)
    assert abs(got["sumsq"] - s) <= ACCURACY * s, (what, s)
    if nd:
        assert got["rms"] == math.sqrt(got["sumsq"] / nd), what
    else:
        assert math.isnan(got["rms"]), what
    assert math.isnan(got["lo"]) and math.isnan(got["hi"]) and math.isnan(got["psnr"]), what


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_every_mask_alignment_and_poison(ctx, n, dt):
    k = 0
    for mask in MASKS:
        for a_el, b_el in ((0, 0), (1, 1), (0, 1)):  # (both one element off: still the element-wise form; one of them off too)
            for mask_off in (0, 1):
                k += 1
                check(ctx, dt, n, mask, a_el, b_el, mask_off, ("a", "b", "both")[k % 3], seed=1000 * n + k, repeats=3 if k % 4 == 0 else 1)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", LARGE)
def test_large_sizes(ctx, n, dt):
    k = 0
    for mask in LARGE_MASKS:
        for a_el, mask_off in ((0, 0), (1, 1)) if mask != "random 50 %" else ((0, 0), (1, 1), (0, 1), (1, 0)):
            k += 1
            check(ctx, dt, n, mask, a_el, a_el, mask_off, ("both", "a", "b")[k % 3], seed=n + k, repeats=3 if mask == "random 50 %" else 1)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_nan_at_a_defined_sample_is_counted_and_nothing_else(ctx, dt):
    for n, at in ((300, 299), (300, 0), (1025, 511), (129, 128)):
        for a_el in (0, 1):
            rng = np.random.default_rng(n + at)
            a = rng.standard_normal(n).astype(dt)
            b = (a.astype(np.float64) + 1e-3 * rng.standard_normal(n)).astype(dt)
            und = rng.random(n) < 0.3
            und[at] = False
            a[und] = np.nan
            b[und] = np.inf
            a[at] = np.nan
            got = run_case(ctx, dt, n, a, b, und, a_el, a_el, 0, rng, 1)
            mx, nonfinite, s, nd = expected(a, b, und)
            assert nonfinite == 1 and got["nonfinite"] == 1 and got["defined"] == nd, got
            assert got["max_abs"] == mx and abs(got["sumsq"] - s) <= ACCURACY * s, (got, mx, s)
    # an infinity minus an infinity of the same sign, and a difference that overflows, at defined samples
    if dt == np.float64:
        a = np.array([np.inf, 1e308, 1.0, 2.0]); b = np.array([np.inf, -1e308, 1.5, 2.0])
        got = run_case(ctx, dt, 4, a, b, np.zeros(4, bool), 0, 0, 0, np.random.default_rng(0), 1)
        assert got["nonfinite"] == 2 and got["defined"] == 4 and got["max_abs"] == 0.5 and got["sumsq"] == 0.25, got


def test_refusals(ctx):
    d = ctx.to_device(np.zeros(16))
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.err_stats_masked(d, d, 0, d)
        assert "error -1:" in str(e.value), str(e.value)
        st = api.ErrorStats()
        assert api.lib().wr_dev_err_stats_masked(ctx.h, d.ptr, d.ptr, 8, None, api.C.byref(st), api.C.byref(api.C.c_ulonglong(0))) == -1
        assert api.lib().wr_dev_err_stats_masked(ctx.h, d.ptr, d.ptr, 8, d.ptr, api.C.byref(st), None) == -1
    finally:
        d.free()
