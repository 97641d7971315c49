"""The stage calls of a masked field on the GPU, alone: wr_dev_mask_split (the packed bits, the exact count, the mean of the
defined samples against math.fsum, the same bits twice), wr_dev_mask_fill and wr_dev_mask_restore (exactly the marked samples,
whole-array bit compares with a guard element on each side).  fp64 and fp32.  Sizes: around one mask byte, around one wave's
64 samples (a wave's __ballot is its 8 mask bytes), less and more than a block, and 2^20 + 3, where every thread of the full
grid takes a second turn.  Each array starts 0 and 1 elements into its buffer.  From 255 samples on, the data carry a NaN, both
infinities and a run of 70 samples below the threshold: one wave's ballot is all ones, its neighbours' are mixed.
The mean: |pad - fsum(defined) / count| <= 2^-36 mean|defined| for fp64.  For fp32 the call returns the mean rounded to float, so
the same bound is held against the fsum mean rounded to float, plus one float spacing for a mean that lies at a rounding tie."""
import math

import numpy as np
import pytest

from waverange_amd import api

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 513, 2 ** 20 + 3]
ACCURACY = 2.0 ** -36  # of the mean, relative to mean(|defined|): k_err_stats' bound holds for each sign's part of the sum
BELOW = -1e30
UNDEF = -9.99e33
GUARD = 12345.5


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def data(n, dtype):
    rng = np.random.default_rng(500 + n)
    a = rng.standard_normal(n).astype(dtype)
    if n >= 255:
        a[n // 5] = np.nan
        a[n // 2] = np.inf
        a[n - 2] = -np.inf
        a[100:170] = dtype(UNDEF)
    elif n >= 7:
        a[n // 2] = np.nan
        a[n - 1] = dtype(UNDEF)
    return a


def undefined_of(a, below):
    x = a.astype(np.float64)
    return ~np.isfinite(x) | (x < below)


def bits_u(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


class Dev:
    """`a` on the device `off` elements into its buffer, a guard element on each side; the mask bits behind a guard byte"""

    def __init__(self, ctx, a, off, boff=8):
        self.ctx, self.a, self.off, self.boff, self.dt = ctx, a, off, boff, a.dtype.type
        self.n = a.size
        self.nb = (self.n + 7) // 8
        self.host = np.concatenate([np.full(off + 1, GUARD, a.dtype), a, np.full(1, GUARD, a.dtype)])
        self.fld = ctx.to_device(self.host)
        self.bits = ctx.to_device(np.full(16 + self.nb + 16, 0xA5, np.uint8))

    def field(self):
        return self.fld.download(self.dt, self.host.size)

    def mask(self):
        """(the guard bytes in front, the mask's ceil(n / 8) bytes, the guard bytes behind)"""
        m = self.bits.download(np.uint8, 16 + self.nb + 16)
        return m[:self.boff], m[self.boff:self.boff + self.nb], m[self.boff + self.nb:]

    def free(self):
        self.fld.free()
        self.bits.free()


@pytest.mark.parametrize("off,boff", [(0, 8), (1, 8), (0, 11)], ids=["aligned", "+1", "bits+3"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_split_fill_restore(ctx, n, dtype, off, boff):
    a = data(n, dtype)
    und = undefined_of(a, BELOW)
    defined = a[~und].astype(np.float64)
    d = Dev(ctx, a, off, boff)
    try:
        kw = dict(dtype=dtype, offset=off + 1, bits_offset=boff)
        undefined, pad = ctx.mask_split(d.fld, n, d.bits, BELOW, **kw)
        front, m, behind = d.mask()
        again = ctx.mask_split(d.fld, n, d.bits, BELOW, **kw)
        assert np.array_equal(bits_u(d.field()), bits_u(d.host)), "the split wrote the field"
        only_nonfinite = ctx.mask_split(d.fld, n, d.bits, -np.inf, **kw)
        m_inf = d.mask()[1]
        ctx.mask_split(d.fld, n, d.bits, BELOW, **kw)
        # fill: exactly the marked samples
        ctx.mask_fill(d.fld, n, d.bits, 3.25, **kw)
        filled = d.field()
        # restore with a NaN and with a finite value, on top of the filled field
        count_nan = ctx.mask_restore(d.fld, n, d.bits, np.nan, **kw)
        restored_nan = d.field()
        count_fin = ctx.mask_restore(d.fld, n, d.bits, -7.5, **kw)
        restored_fin = d.field()
    finally:
        d.free()
    want_bits = np.packbits(und, bitorder="little")
    assert np.array_equal(m, want_bits)
    assert (front == 0xA5).all() and (behind == 0xA5).all(), "the split wrote outside its ceil(n / 8) bytes"
    if n % 8:
        assert m[-1] >> (n % 8) == 0
    assert undefined == int(und.sum())
    want_mean = math.fsum(defined) / defined.size
    want_pad = float(dtype(want_mean)) if dtype is np.float32 else want_mean
    scale = float(np.abs(defined).mean())
    print("n %d %s +%d: pad %r, fsum mean %r, difference / mean|x| %.3g" % (n, np.dtype(dtype).name, off, pad, want_mean, abs(pad - want_mean) / scale))
    if dtype is np.float64:
        assert abs(pad - want_mean) <= ACCURACY * scale
    else:  # the mean rounded to float: within the bound of a float next to the exact mean's rounding
        assert pad == float(np.float32(pad))
        assert abs(pad - want_pad) <= ACCURACY * scale + float(np.spacing(np.float32(abs(want_pad))))
    assert again[0] == undefined and np.float64(again[1]).view(np.uint64) == np.float64(pad).view(np.uint64)
    nonfinite = ~np.isfinite(a.astype(np.float64))
    assert only_nonfinite[0] == int(nonfinite.sum())
    assert np.array_equal(m_inf, np.packbits(nonfinite, bitorder="little"))

    def expect(value):
        h = d.host.copy()
        seg = h[off + 1: off + 1 + n]
        seg[und] = dtype(value)
        return h

    assert np.array_equal(bits_u(filled), bits_u(expect(3.25)))
    assert count_nan == count_fin == int(und.sum())
    assert np.array_equal(bits_u(restored_nan), bits_u(expect(np.nan)))
    assert np.array_equal(bits_u(restored_fin), bits_u(expect(-7.5)))
    for h in (filled, restored_nan, restored_fin):
        assert h[off] == GUARD and h[-1] == GUARD


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_all_defined_and_all_undefined(ctx, dtype):
    n = 1005
    rng = np.random.default_rng(9)
    a = rng.standard_normal(n).astype(dtype)
    for arr, want in ((a, 0), (np.full(n, UNDEF, dtype), n), (np.full(n, np.nan, dtype), n)):
        d = Dev(ctx, arr, 0)
        try:
            undefined, pad = ctx.mask_split(d.fld, n, d.bits, BELOW, dtype=dtype, offset=1, bits_offset=8)
            m = d.mask()[1]
        finally:
            d.free()
        assert undefined == want
        assert np.array_equal(m, np.packbits(np.full(n, bool(want)), bitorder="little"))
        assert n - undefined == (n if not want else 0)  # the count of defined samples
        assert math.isnan(pad) if want else abs(pad - float(arr.astype(np.float64).mean())) < 1e-6
    # the encode refuses a field without a defined sample, and a NaN threshold
    f = np.full((3, 5, 7), np.nan, dtype)
    enc = ctx.encode_host_seg_masked if dtype is np.float64 else ctx.encode_host_seg_masked_f32
    with pytest.raises(api.WaveRangeError) as e:
        enc(f, 1e-5, BELOW)
    assert "error -1" in str(e.value) and "no defined sample" in str(e.value)
    with pytest.raises(api.WaveRangeError) as e:
        enc(np.ones((3, 5, 7), dtype), 1e-5, np.nan)
    assert "error -1" in str(e.value)
    d = Dev(ctx, a, 0)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.mask_split(d.fld, n, d.bits, np.nan, dtype=dtype, offset=1, bits_offset=8)
        assert "error -1" in str(e.value)
    finally:
        d.free()


def test_restore_refuses_a_bit_beyond_n(ctx):
    n = 13
    a = np.zeros(n)
    d = Dev(ctx, a, 0)
    try:
        d.bits.upload(np.concatenate([np.zeros(8, np.uint8), np.array([0x01, 0x20], np.uint8)]))  # (from byte 8 on)  # bit 13 of 13 samples
        with pytest.raises(api.WaveRangeError) as e:
            ctx.mask_restore(d.fld, n, d.bits, 1.0, offset=1, bits_offset=8)
        assert "error -4" in str(e.value)
        assert d.field()[-1] == GUARD
    finally:
        d.free()
