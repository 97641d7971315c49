"""The batched mask stage calls on the GPU against the loop of the single ones: wr_dev_mask_split_batch (mask bytes, the
count, and the BIT PATTERN of pad: block (x, f) of the batched kernel is block x of k_mask_split on field f, so the sums agree to
the last bit), wr_dev_mask_fill_batch (sentinel bit patterns: nothing but the marked samples moves; a NULL field is skipped)
and wr_dev_mask_check_batch (population counts against np.unpackbits, the flag for a bit at or beyond n).  fp64 and fp32.
The fields of a batch lie in ONE device buffer, field f at element f * stride, its bits at byte 16 + f * bstride of another, so
that a table of 1024 entries costs two allocations."""
import numpy as np
import pytest

from waverange_amd import api

pytestmark = pytest.mark.gpu

BELOW = -1e30
UNDEF = -9.99e33
# what each n is here for
SIZES = {
    1: "one sample, one mask byte, one lane",
    7: "a partial mask byte",
    63: "one short of a wave's 64 samples",
    64: "exactly one chunk: one whole word where the bits are aligned",
    65: "a second chunk of one sample: the byte path in the last chunk",
    511: "two blocks, the last chunk short",
    513: "a third block of one sample",
    8192 * 64 * 4 + 64 * 3 + 5: "the full grid's waves take a second round of kTurns with some turns missing",
}


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def field(n, dtype, seed):
    rng = np.random.default_rng(7000 + 13 * seed + n % 1000)
    a = rng.standard_normal(n).astype(dtype)
    if n >= 7:
        a[rng.integers(0, n, size=max(1, n // 9))] = dtype(UNDEF)
        a[n // 2] = np.nan
    if n >= 63:
        a[n // 3] = np.inf
        a[n - 2] = -np.inf
    return a


def u64(x):
    return np.float64(x).view(np.uint64)


class Batch:
    """the fields of a batch in one device buffer, their bits in another; odd: the field whose bits pointer is odd"""

    def __init__(self, ctx, arrays, odd=None):
        self.ctx, self.arrays, self.nf = ctx, arrays, len(arrays)
        self.n, self.dt = arrays[0].size, arrays[0].dtype.type
        self.nb = (self.n + 7) // 8
        self.stride = self.n + 1  # (a guard element behind every field)
        self.bstride = (self.nb + 8 + 7) & ~7
        host = np.full(self.nf * self.stride, 12345.5, self.dt)
        for f, a in enumerate(arrays):
            host[f * self.stride: f * self.stride + self.n] = a
        self.host = host
        self.fld = ctx.to_device(host)
        self.bits = ctx.to_device(np.full(16 + self.nf * self.bstride + 16, 0xA5, np.uint8))
        self.offsets = [f * self.stride for f in range(self.nf)]
        self.boffs = [16 + f * self.bstride + (1 if f == odd else 0) for f in range(self.nf)]

    def kw(self):
        return dict(dtype=self.dt, offsets=self.offsets, bits_offsets=self.boffs)

    def all_bits(self):
        return self.bits.download(np.uint8, 16 + self.nf * self.bstride + 16)

    def fields(self):
        return self.fld.download(self.dt, self.host.size)

    def free(self):
        self.fld.free()
        self.bits.free()


def split_both_ways(ctx, arrays, below, odd=None):
    """(the batched call's results and bits buffer, the loop's) on two identical batches"""
    a, b = Batch(ctx, arrays, odd), Batch(ctx, arrays, odd)
    try:
        got = ctx.mask_split_batch([a.fld] * a.nf, a.n, [a.bits] * a.nf, below, **a.kw())
        want = [ctx.mask_split(b.fld, b.n, b.bits, below, dtype=b.dt, offset=b.offsets[f], bits_offset=b.boffs[f]) for f in range(b.nf)]
        assert np.array_equal(a.fields().view(np.uint8), a.host.view(np.uint8)), "the split wrote a field"
        return got, a.all_bits(), want, b.all_bits(), a
    finally:
        a.free()
        b.free()


def check_split(arrays, below, got, got_bits, want, want_bits, batch):
    assert np.array_equal(got_bits, want_bits), "mask bytes (and every byte around them) differ from the single calls'"
    for f, a in enumerate(arrays):
        und = ~np.isfinite(a.astype(np.float64)) | (a.astype(np.float64) < below)
        m = got_bits[batch.boffs[f]: batch.boffs[f] + batch.nb]
        assert np.array_equal(m, np.packbits(und, bitorder="little")), f
        assert got[f][0] == want[f][0] == int(und.sum()), f
        assert u64(got[f][1]) == u64(want[f][1]), (f, got[f][1], want[f][1])


@pytest.mark.parametrize("odd", [None, 0], ids=["aligned", "one-odd"])
@pytest.mark.parametrize("nfields", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", sorted(SIZES))
def test_split_batch_is_the_loop_of_split(ctx, n, dtype, nfields, odd):
    arrays = [field(n, dtype, f) for f in range(nfields)]
    if odd is not None:
        odd = nfields - 1
    got, got_bits, want, want_bits, batch = split_both_ways(ctx, arrays, BELOW, odd)
    check_split(arrays, BELOW, got, got_bits, want, want_bits, batch)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_split_batch_full_table(ctx, dtype):
    """1024 fields of 65 samples: gridDim.y = 1024, every entry of the table used; one bits pointer odd"""
    arrays = [field(65, dtype, f) for f in range(api.SEG_BATCH_MAX)]
    got, got_bits, want, want_bits, batch = split_both_ways(ctx, arrays, BELOW, 517)
    check_split(arrays, BELOW, got, got_bits, want, want_bits, batch)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_split_batch_special_fields(ctx, dtype):
    """in one batch: no undefined sample; none defined (pad NaN, the call succeeds); only NaN and +-inf undefined"""
    n = 1005
    rng = np.random.default_rng(3)
    plain = rng.standard_normal(n).astype(dtype)
    nothing = np.full(n, UNDEF, dtype)
    nothing[::3] = np.nan
    nonfinite = rng.standard_normal(n).astype(dtype)
    nonfinite[[5, 64, 700]] = [np.nan, np.inf, -np.inf]
    arrays = [plain, nothing, nonfinite, field(n, dtype, 9)]
    got, got_bits, want, want_bits, batch = split_both_ways(ctx, arrays, BELOW)
    check_split(arrays, BELOW, got, got_bits, want, want_bits, batch)
    assert got[0][0] == 0 and got[1][0] == n and got[2][0] == 3
    assert np.isnan(got[1][1])


def test_split_batch_refusals(ctx):
    a = Batch(ctx, [field(65, np.float64, 0)])
    try:
        for bad in (lambda: ctx.mask_split_batch([a.fld], 65, [a.bits], np.nan),
                    lambda: ctx.mask_split_batch([a.fld], 0, [a.bits], BELOW),
                    lambda: ctx.mask_split_batch([], 65, [], BELOW),
                    lambda: ctx.mask_split_batch([a.fld] * (api.SEG_BATCH_MAX + 1), 65, [a.bits] * (api.SEG_BATCH_MAX + 1), BELOW),
                    lambda: ctx.mask_check_batch([a.bits], 0),
                    lambda: ctx.mask_fill_batch([a.fld], 0, [a.bits], [1.0])):
            with pytest.raises(api.WaveRangeError) as e:
                bad()
            assert "error -1" in str(e.value)
    finally:
        a.free()


@pytest.mark.parametrize("odd", [None, 1], ids=["aligned", "one-odd"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 65, 513, 70001])
def test_fill_batch_is_the_loop_of_fill(ctx, n, dtype, odd):
    """sentinel bit patterns (NaN payloads among them): every sample not under a bit keeps its bits; field 2 is NULL"""
    nf = 4
    rng = np.random.default_rng(n)
    utype = np.uint64 if dtype is np.float64 else np.uint32
    arrays = [rng.integers(0, np.iinfo(utype).max, size=n, dtype=utype).view(dtype) for _ in range(nf)]
    masks = [rng.random(n) < (0.0 if f == 3 else 0.3) for f in range(nf)]  # (field 3: no bit set, nothing stored)
    values = [3.25, np.nan, 7.0, -1.0]
    a, b = Batch(ctx, arrays, odd), Batch(ctx, arrays, odd)
    try:
        for bt in (a, b):
            allb = np.full(16 + nf * bt.bstride + 16, 0, np.uint8)
            for f in range(nf):
                allb[bt.boffs[f]: bt.boffs[f] + bt.nb] = np.packbits(masks[f], bitorder="little")
            bt.bits.upload(allb)
        flds = [a.fld, a.fld, None, a.fld]
        ctx.mask_fill_batch(flds, n, [a.bits] * nf, values, **a.kw())
        for f in (0, 1, 3):
            ctx.mask_fill(b.fld, n, b.bits, values[f], dtype=dtype, offset=b.offsets[f], bits_offset=b.boffs[f])
        got, want = a.fields(), b.fields()
    finally:
        a.free()
        b.free()
    assert np.array_equal(got.view(utype), want.view(utype))
    expect = a.host.copy()
    for f in (0, 1, 3):
        expect[f * a.stride: f * a.stride + n][masks[f]] = dtype(values[f])
    assert np.array_equal(got.view(utype), expect.view(utype)), "a sample outside the masks moved, or the NULL field was written"


@pytest.mark.parametrize("odd", [None, 2], ids=["aligned", "one-odd"])
@pytest.mark.parametrize("n", [5, 61, 509, 4099, 8192 * 64 + 61])
def test_check_batch_counts_and_flags(ctx, n, odd):
    nm, nb = 4, (n + 7) // 8
    assert n % 8 and 8 * nb - 1 > n
    rng = np.random.default_rng(n)
    bits = [np.packbits(rng.random(n) < 0.4, bitorder="little") for _ in range(nm)]
    bits[1][n >> 3] |= 1 << (n & 7)  # the first bit beyond the field
    bits[2][nb - 1] |= 0x80          # bit 8 * ceil(n / 8) - 1, the last of the mask's bytes
    bstride = (nb + 8 + 7) & ~7
    boffs = [16 + m * bstride + (1 if m == odd else 0) for m in range(nm)]
    allb = np.zeros(16 + nm * bstride + 16, np.uint8)
    for m in range(nm):
        allb[boffs[m]: boffs[m] + nb] = bits[m]
    allb[:16] = 0xFF  # (set bits outside every mask: not counted)
    buf = ctx.to_device(allb)
    try:
        got = ctx.mask_check_batch([buf] * nm, n, boffs)
    finally:
        buf.free()
    assert [g[0] for g in got] == [int(np.unpackbits(b).sum()) for b in bits]
    assert [g[1] for g in got] == [False, True, True, False]
