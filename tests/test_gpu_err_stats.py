"""wr_dev_err_stats on the GPU, alone: the maximum of the finite |a - b| equal to numpy's, the count of non-finite differences
exact, the sum of squares within 2^-36 (relative) of math.fsum over the rounded squares -- the real sum of the very terms the
kernel adds --, the same bits on a second call, and zero for identical arrays.  Sizes: one sample, one pair, less than a block,
an odd tail behind whole pairs, and 2^20 + 3, where every thread of the full grid takes a second turn.  fp64 and fp32; both
arrays aligned for the two-sample loads, and one of them moved by one element (the element-wise form)."""
import math

import numpy as np
import pytest

from waverange_amd import api

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 513, 2 ** 20 + 3]
ACCURACY = 2.0 ** -36


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def arrays(n, dtype):
    """random data; from 255 samples on a planted NaN, a planted infinity and one large difference"""
    rng = np.random.default_rng(1000 + n)
    a = rng.standard_normal(n).astype(dtype)
    b = (a.astype(np.float64) + 1e-3 * rng.standard_normal(n)).astype(dtype)
    if n >= 255:
        a[n // 3] = np.nan
        b[n // 2] = np.inf
        b[(2 * n) // 3] = a[(2 * n) // 3] + dtype(37.5)
    return a, b


def reference(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    fin = d[np.isfinite(d)]
    return (float(np.abs(fin).max()) if fin.size else 0.0), int(d.size - fin.size), math.fsum(fin * fin)


def bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 0), (0, 1)], ids=["aligned", "a+1", "b+1"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_err_stats_against_numpy_and_fsum(ctx, n, dtype, offsets):
    a, b = arrays(n, dtype)
    want_max, want_bad, want_s = reference(a, b)
    ao, bo = offsets
    d_a = ctx.to_device(np.concatenate([np.zeros(ao, dtype), a]))
    d_b = ctx.to_device(np.concatenate([np.zeros(bo, dtype), b]))
    try:
        st = ctx.err_stats(d_a, d_b, n, dtype, a_off=ao, b_off=bo)
        again = ctx.err_stats(d_a, d_b, n, dtype, a_off=ao, b_off=bo)
        same = ctx.err_stats(d_a, d_a, n, dtype, a_off=ao, b_off=ao)
    finally:
        d_a.free()
        d_b.free()
    print("n %d %s %s: sumsq %r, fsum %r, relative difference %.3g" % (n, np.dtype(dtype).name, offsets, st["sumsq"], want_s,
                                                                    abs(st["sumsq"] - want_s) / want_s if want_s else 0.0))
    assert bits(st["max_abs"]) == bits(want_max), (st, want_max)
    assert st["nonfinite"] == want_bad, (st, want_bad)
    assert abs(st["sumsq"] - want_s) <= ACCURACY * want_s, (st["sumsq"], want_s)
    assert abs(st["rms"] - math.sqrt(want_s / n)) <= ACCURACY * math.sqrt(want_s / n)
    assert all(bits(st[k]) == bits(again[k]) for k in ("max_abs", "sumsq", "rms")) and st["nonfinite"] == again["nonfinite"]
    # identical arrays: nothing but the NaN (a - a of a NaN is a NaN; the infinity sits in b)
    assert same["max_abs"] == 0.0 and same["sumsq"] == 0.0 and same["rms"] == 0.0
    assert same["nonfinite"] == (1 if n >= 255 else 0)


def test_err_stats_of_an_overflowing_square_and_its_refusals(ctx):
    a = np.array([1e200, 1.0, 2.0, 3.0])
    b = np.array([-1e200, 1.0, 2.0, 3.5])
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    try:
        st = ctx.err_stats(d_a, d_b, 4)
        assert st["max_abs"] == 2e200 and st["nonfinite"] == 0 and st["sumsq"] == np.inf and st["rms"] == np.inf
        with pytest.raises(api.WaveRangeError) as e:
            ctx.err_stats(d_a, d_b, 0)
        assert "error -1:" in str(e.value), str(e.value)
        with pytest.raises(TypeError):
            ctx.err_stats(d_a, d_b, 4, np.int32)
    finally:
        d_a.free()
        d_b.free()
