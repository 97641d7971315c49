"""Masked fields through the whole path on the GPU: wr_encode_*_seg_masked / wr_decode_*_seg_masked against the plain calls on
the numpy-padded field.  The field part of a masked record must be, bit for bit, the plain call's stream of the field with its
undefined samples replaced by the returned pad; the mask part the host definition of the blob; the decode np.where(undefined,
fill, plain decode).  Shapes: two single-plane slivers, an odd box, one shape whose four levels all run on the fused kernels and
one that takes the general kernels (both asserted through wr_fused_plan first).  WRS1, WRS2 (brick 32), WRS3 (8 strands); fp64
and fp32.  About 30 % of the samples are undefined in one coherent region (a value far below the threshold), a few isolated
ones are NaNs."""
import numpy as np
import pytest

from fused_cases import EDGE_SHAPES, check_plan
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

FUSED, GENERAL = (64, 64, 64), (37, 21, 13)
SHAPES = [(5, 3, 1), (13, 5, 1), (33, 17, 9), FUSED, GENERAL]  # (nx, ny, nz)
FORMATS = {"wrs1": dict(brick=0, strands=0), "wrs2": dict(brick=32, strands=0), "wrs3": dict(brick=0, strands=8)}
TOL = 1e-5
BELOW = -1e30
UNDEF = -9.99e33


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def plain_format(fmt):
    """the masked calls' (brick, strands) as the plain Python calls spell them"""
    return dict(brick=fmt["brick"] or None, strands=fmt["strands"] or None)


_fields = {}


def masked_field(shape_xyz, dtype):
    """(field with its undefined samples planted, the boolean mask); read-only, built once"""
    key = (shape_xyz, np.dtype(dtype).name)
    if key not in _fields:
        nx, ny, nz = shape_xyz
        f = synth.field(nx, ny, nz, seed=31 + nx + 7 * ny + 49 * nz)
        z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
        g = np.sin(5.0 * x + 1.0) + np.cos(4.0 * y) + np.sin(3.0 * z + 2.0 * x)
        und = g > np.quantile(g, 0.7)
        f = f.astype(dtype)
        f[und] = dtype(UNDEF)
        rng = np.random.default_rng(nx * ny * nz)
        lone = rng.integers(0, f.size, size=3)
        f.reshape(-1)[lone] = np.nan
        und = und.copy()
        und.reshape(-1)[lone] = True
        assert 0 < und.sum() < und.size
        f.setflags(write=False)
        und.setflags(write=False)
        _fields[key] = (f, und)
    return _fields[key]


def calls(ctx, dtype):
    if np.dtype(dtype) == np.float64:
        return ctx.encode_host_seg_masked, ctx.decode_host_seg_masked, ctx.encode_host_seg, ctx.decode_host_seg
    return ctx.encode_host_seg_masked_f32, ctx.decode_host_seg_masked_f32, ctx.encode_host_seg_f32, ctx.decode_host_seg_f32


def same_info(a, b):
    for k in ("tolabs", "midval", "halfspanval"):
        assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), k
    assert (a["wlev"], a["nlay"], a["ntot_enc"], a["len_enc_vec"]) == (b["wlev"], b["nlay"], b["ntot_enc"], b["len_enc_vec"])
    for k in ("deps_vec", "minval_vec"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint64), np.asarray(b[k]).view(np.uint64)), k


def ints(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_the_shapes_take_the_paths_they_are_here_for():
    check_plan(api, FUSED, EDGE_SHAPES[FUSED])
    check_plan(api, GENERAL, EDGE_SHAPES[GENERAL])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_record_is_the_plain_record_of_the_padded_field_plus_the_mask(ctx, shape, fmt, dtype):
    f, und = masked_field(shape, dtype)
    enc_m, dec_m, enc_p, dec_p = calls(ctx, dtype)
    kw = FORMATS[fmt]
    rec, _ = enc_m(f, TOL, BELOW, **kw)
    rec["data"] = rec["data"].copy()
    mask = rec["mask"]
    n = f.size
    assert mask["undefined"] == int(und.sum())
    pad = mask["pad"]
    if dtype is np.float32:
        assert pad == float(np.float32(pad))
    defined_mean = float(f[~und].astype(np.float64).mean())
    assert abs(pad - defined_mean) <= 1e-6 * float(np.abs(f[~und].astype(np.float64)).mean()) + 1e-12
    # (a) the field part: the plain call on the numpy-padded field
    padded = np.where(und, dtype(pad), f)
    want, _ = enc_p(padded, TOL, **plain_format(kw))
    same_info(rec, want)
    nt = rec["ntot_enc"]
    assert np.array_equal(rec["data"][:nt], want["data"])
    # (b) the mask part: the host definition of the blob
    assert rec["data"].size == nt + mask["mask_len"]
    assert np.array_equal(rec["data"][nt:], api.mask_blob_host_ref(und.reshape(-1), 0, pad))
    assert mask["mask_len"] <= api.mask_bound(n, 0)
    # (c) the decode, with a NaN and with a finite fill, compared as integers
    plain_out = np.empty(f.shape, dtype)
    dec_p(plain_out, dict(rec, data=rec["data"][:nt]))
    for fill in (np.nan, -77.25):
        out = np.full(f.shape, 4242.0, dtype)
        got, _ = dec_m(out, rec, fill)
        assert got["undefined"] == mask["undefined"] and got["mask_len"] == mask["mask_len"]
        assert np.array_equal(ints(out), ints(np.where(und, dtype(fill), plain_out)))
    # (e) the older decoders read the field part and return the padded field's results
    want_out = np.empty(f.shape, dtype)
    dec_p(want_out, want)
    assert np.array_equal(ints(plain_out), ints(want_out))
    # a record without the blob decodes as the plain call does
    out = np.empty(f.shape, dtype)
    got, _ = dec_m(out, dict(rec, data=rec["data"][:nt]))
    assert got["mask_len"] == 0 and np.array_equal(ints(out), ints(plain_out))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_region_and_lowres_decodes_read_the_field_part(ctx, fmt):
    """(e) for the partial decodes, on the odd box: what they return for the masked record's field part is what they return
    for the plain record of the padded field"""
    shape = (33, 17, 9)
    f, und = masked_field(shape, np.float64)
    kw = FORMATS[fmt]
    rec, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, **kw)
    rec["data"] = rec["data"].copy()
    field_part = dict(rec, data=rec["data"][:rec["ntot_enc"]])
    want, _ = ctx.encode_host_seg(np.where(und, rec["mask"]["pad"], f), TOL, **plain_format(kw))
    want["data"] = want["data"].copy()
    roi = ((1, 6), (2, 11), (3, 20))
    a, b = np.empty(api.roi_shape(roi)), np.empty(api.roi_shape(roi))
    ctx.decode_host_seg_roi(a, f.shape, 0, roi, field_part)
    ctx.decode_host_seg_roi(b, f.shape, 0, roi, want)
    assert np.array_equal(ints(a), ints(b))
    a, b = np.empty(api.lowres_shape(f.shape, 1)), np.empty(api.lowres_shape(f.shape, 1))
    ctx.decode_host_seg_lowres(a, f.shape, 1, field_part)
    ctx.decode_host_seg_lowres(b, f.shape, 1, want)
    assert np.array_equal(ints(a), ints(b))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(13, 5, 1), FUSED], ids=lambda s: "x".join(map(str, s)))
def test_no_undefined_sample_gives_the_plain_record(ctx, shape, dtype):
    """(d)"""
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=5).astype(dtype)
    enc_m, dec_m, enc_p, _ = calls(ctx, dtype)
    rec, _ = enc_m(f, TOL, BELOW)
    want, _ = enc_p(f, TOL)
    same_info(rec, want)
    assert rec["mask"]["undefined"] == 0 and rec["mask"]["mask_len"] == 0
    assert np.array_equal(rec["data"], want["data"])
    # with the threshold off only the non-finite samples count: a field of finite values far below any data is plain too
    rec2, _ = enc_m(f - dtype(1e6), TOL, -np.inf)
    assert rec2["mask"]["undefined"] == 0 and rec2["mask"]["mask_len"] == 0


def test_constant_padded_field_is_the_trivial_record_plus_the_mask(ctx):
    f = np.full((3, 5, 7), 2.5)
    und = np.zeros(f.shape, bool)
    und[1, 2:4, 1:6] = True
    f[und] = np.nan
    rec, _ = ctx.encode_host_seg_masked(f, TOL)
    rec["data"] = rec["data"].copy()
    assert rec["nlay"] == 0 and rec["ntot_enc"] == 0 and rec["mask"]["pad"] == 2.5 and rec["mask"]["undefined"] == int(und.sum())
    assert np.array_equal(rec["data"], api.mask_blob_host_ref(und.reshape(-1), 0, 2.5))
    for fill in (np.nan, 9.0):
        out = np.full(f.shape, 4242.0)
        ctx.decode_host_seg_masked(out, rec, fill)
        assert np.array_equal(ints(out), ints(np.where(und, fill, 2.5)))
    buf = ctx.to_device(np.full(f.shape, 4242.0))
    try:
        ctx.decode_seg_masked(buf, f.shape, rec, -1.0)
        out = buf.download(np.float64, f.size).reshape(f.shape)
    finally:
        buf.free()
    assert np.array_equal(out, np.where(und, -1.0, 2.5))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("shape", [(33, 17, 9), FUSED], ids=lambda s: "x".join(map(str, s)))
def test_device_field_forms_agree_with_the_host_forms(ctx, shape, fmt):
    """(f)"""
    f, und = masked_field(shape, np.float64)
    kw = FORMATS[fmt]
    rec, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, **kw)
    rec["data"] = rec["data"].copy()
    host_out = np.empty(f.shape)
    ctx.decode_host_seg_masked(host_out, rec, np.nan)
    buf = ctx.to_device(f)
    try:
        dev, _ = ctx.encode_seg_masked(buf, f.shape, TOL, BELOW, **kw)
        dev["data"] = dev["data"].copy()
        same_info(dev, rec)
        assert dev["mask"]["undefined"] == rec["mask"]["undefined"] and dev["mask"]["mask_len"] == rec["mask"]["mask_len"]
        assert np.float64(dev["mask"]["pad"]).view(np.uint64) == np.float64(rec["mask"]["pad"]).view(np.uint64)
        assert np.array_equal(dev["data"], rec["data"])
        ctx.decode_seg_masked(buf, f.shape, rec, np.nan)
        dev_out = buf.download(np.float64, f.size).reshape(f.shape)
    finally:
        buf.free()
    assert np.array_equal(ints(dev_out), ints(host_out))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_corrupted_mask_blob_is_refused_and_leaves_the_field_alone(ctx, dtype):
    """(g) every way a blob can be wrong that the host parse knows (tests/test_mask_format_cpu.py), here through the decoder: the
    header on the host, the segment that does not decode and the two properties of the bits on the device"""
    import struct
    shape = (33, 17, 9)
    f, und = masked_field(shape, dtype)
    enc_m, dec_m, _, _ = calls(ctx, dtype)
    rec, _ = enc_m(f, TOL, BELOW)
    rec["data"] = rec["data"].copy()
    nt, n, count = rec["ntot_enc"], f.size, int(und.sum())
    planes, blob = rec["data"][:nt], rec["data"][nt:]
    bits = np.packbits(und.reshape(-1), bitorder="little")
    assert n % 8

    def head(n_, count_, magic=b"WRM1", reserved=0):
        return np.frombuffer(magic + struct.pack("<IQQd", reserved, n_, count_, 0.0), dtype=np.uint8)

    nseg = struct.unpack("<I", bytes(blob[40:44]))[0]
    flipped = blob.copy()
    flipped[32 + 12 + 4 * nseg + 2] ^= 0x40
    one_more = bits.copy()
    clear = int(np.flatnonzero(~und.reshape(-1))[0])
    one_more[clear >> 3] |= 1 << (clear & 7)
    beyond = bits.copy()
    last = int(np.flatnonzero(und.reshape(-1))[-1])
    beyond[last >> 3] = int(beyond[last >> 3]) & (0xFF ^ (1 << (last & 7)))
    beyond[-1] |= 0x80
    bad_blobs = {
        "magic": np.concatenate([head(n, count, magic=b"WRM2"), blob[32:]]),
        "reserved": np.concatenate([head(n, count, reserved=7), blob[32:]]),
        "n": np.concatenate([head(n - 1, count), blob[32:]]),
        "truncated": blob[:-1],
        "overlong": np.concatenate([blob, np.zeros(3, np.uint8)]),
        "short header": blob[:17],
        "does not decode": flipped,
        "count": np.concatenate([head(n, count), api.seg_encode_host_ref(one_more, 0)]),
        "beyond n": np.concatenate([head(n, count), api.seg_encode_host_ref(beyond, 0)]),
    }
    for name, bad in bad_blobs.items():
        out = np.full(f.shape, 4242.0, dtype)
        with pytest.raises(api.WaveRangeError) as e:
            dec_m(out, dict(rec, data=np.concatenate([planes, bad])))
        assert "error -4" in str(e.value), (name, str(e.value))
        assert (out == 4242.0).all(), name
    # the device-field form as well: nothing reaches the caller's array
    if dtype is np.float64:
        buf = ctx.to_device(np.full(f.shape, 4242.0))
        try:
            for name in ("does not decode", "count", "beyond n"):
                with pytest.raises(api.WaveRangeError) as e:
                    ctx.decode_seg_masked(buf, f.shape, dict(rec, data=np.concatenate([planes, bad_blobs[name]])))
                assert "error -4" in str(e.value), (name, str(e.value))
                assert (buf.download(np.float64, n) == 4242.0).all(), name
        finally:
            buf.free()
    # and the record still decodes
    out = np.empty(f.shape, dtype)
    dec_m(out, rec)
    assert np.array_equal(np.isnan(out), und)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_cap_too_small_is_an_overflow(ctx, fmt):
    """(h) the buffer must hold the field's planes and the mask blob's bound"""
    f, und = masked_field((33, 17, 9), np.float64)
    kw = FORMATS[fmt]
    rec, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, **kw)
    nt = rec["ntot_enc"]
    need = nt + api.mask_bound(f.size, 0)
    for cap in (nt, nt + rec["mask"]["mask_len"], need - 1):
        out = np.full(need, 0xEE, np.uint8)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_masked(f, TOL, BELOW, out=out[:cap], **kw)
        assert "error -5" in str(e.value), str(e.value)
        assert (out == 0xEE).all(), "an encode that overflows writes nothing"
    out = np.empty(need, np.uint8)
    again, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, out=out, **kw)
    assert np.array_equal(again["data"], rec["data"])
