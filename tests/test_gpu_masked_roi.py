"""The masked region / low-resolution decode through the whole path on the GPU (wr_decode_*_seg_roi_masked), over the case
table of masked_roi_cases.py.

Level 0: the result is, bit for bit, the crop of what decode_host_seg_masked returns with the same fill (nan and -77.25), and
res.undefined is the region's count: fp64 host form in WRS1, WRS2 (brick 32) and WRS3 (8 strands), the fp32 host form and the
device form in WRS1.  Levels 1 .. 4 and the whole box: where(coarse mask, fill, plain region / low-resolution call on the field
part).  A case's segment length is the record's: the field's planes and the mask plane are cut at it.  A WRS3 record needs
16 * strands <= seg, which 16 and 48 are not for 8 strands: there the records are cut at 128 and 144, the shortest legal lengths
that keep one a multiple of the other's third, so small regions still cross segment boundaries (a mask segment of 1024 or 1152
samples); the lists are compared at the length actually used.
Then: only the listed mask segments are touched (the counter's delta; a byte flipped in a segment the region does not list
changes nothing, one flipped in a listed segment is refused), records without a blob, a constant padded field, damaged blobs,
refused regions."""
import struct

import numpy as np
import pytest

import masked_roi_cases as mc
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

FORMATS = {"wrs1": dict(brick=0, strands=0), "wrs2": dict(brick=32, strands=0), "wrs3": dict(brick=0, strands=8)}
WRS3_SEG = {16: 128, 48: 144, 0: 0}
TOL = 1e-5
BELOW = -1e30
UNDEF = -9.99e33
SENTINEL = 4242.0
LEVEL0 = [c for c in mc.CASES if c[1] == 0]
COARSE = [c for c in mc.CASES if c[1] > 0]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def ints(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def seg_of(case, fmt):
    return WRS3_SEG[case[3]] if fmt == "wrs3" else case[3]


_fields, _records, _full = {}, {}, {}


def field_of(shape, dtype):
    """(the field with the recipe's undefined samples planted, the boolean mask); read-only, built once"""
    key = (shape, np.dtype(dtype).name)
    if key not in _fields:
        nx, ny, nz = shape
        und = mc.und_recipe(shape)
        f = synth.field(nx, ny, nz, seed=31 + nx + 7 * ny + 49 * nz).astype(dtype)
        f[und] = dtype(UNDEF)
        f.reshape(-1)[np.flatnonzero(und.reshape(-1))[::1000]] = np.nan
        f.setflags(write=False)
        _fields[key] = (f, und)
    return _fields[key]


def record_of(ctx, shape, fmt, seg, dtype=np.float64):
    """the masked record of the shape's field, encoded once per (shape, format, segment length, precision)"""
    key = (shape, fmt, seg, np.dtype(dtype).name)
    if key not in _records:
        f, _ = field_of(shape, dtype)
        enc = ctx.encode_host_seg_masked if np.dtype(dtype) == np.float64 else ctx.encode_host_seg_masked_f32
        rec, _ = enc(f, TOL, BELOW, seg=seg, **FORMATS[fmt])
        rec["data"] = rec["data"].copy()
        rec["data"].setflags(write=False)
        _records[key] = rec
    return _records[key]


def full_of(ctx, shape, fmt, seg, fill, dtype=np.float64):
    """decode_host_seg_masked of that record: the reference of the level-0 compares, computed once"""
    key = (shape, fmt, seg, repr(fill), np.dtype(dtype).name)
    if key not in _full:
        nx, ny, nz = shape
        out = np.empty((nz, ny, nx), dtype)
        dec = ctx.decode_host_seg_masked if np.dtype(dtype) == np.float64 else ctx.decode_host_seg_masked_f32
        dec(out, record_of(ctx, shape, fmt, seg, dtype), fill)
        out.setflags(write=False)
        _full[key] = out
    return _full[key]


def crop(a, case):
    x0, x1, y0, y1, z0, z1 = mc.region_of(case)
    return a[z0:z1, y0:y1, x0:x1]


def field_part(rec):
    return dict(rec, data=rec["data"][:rec["ntot_enc"]])


def plain(ctx, case, rec, max_planes=0, dtype=np.float64):
    """the plain region / low-resolution call on the field part"""
    (nx, ny, nz), level, roi, _ = case
    out = np.empty(mc.out_shape(case), dtype)
    f64 = np.dtype(dtype) == np.float64
    if roi is None:
        (ctx.decode_host_seg_lowres if f64 else ctx.decode_host_seg_lowres_f32)(out, (nz, ny, nx), level, field_part(rec), max_planes)
    else:
        (ctx.decode_host_seg_roi if f64 else ctx.decode_host_seg_roi_f32)(out, (nz, ny, nx), level, roi, field_part(rec), max_planes)
    return out


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("case", LEVEL0, ids=mc.case_id)
def test_level_0_is_the_crop_of_the_full_masked_decode(ctx, case, fmt):
    (nx, ny, nz), level, roi, _ = case
    seg = seg_of(case, fmt)
    rec = record_of(ctx, case[0], fmt, seg)
    _, und = field_of(case[0], np.float64)
    want_count = int(mc.coarse_und(und, case).sum())
    for fill in (np.nan, -77.25):
        out = np.full(mc.out_shape(case), SENTINEL)
        res, _ = ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), 0, roi, rec, fill)
        assert np.array_equal(ints(out), ints(crop(full_of(ctx, case[0], fmt, seg, fill), case)))
        assert res["undefined"] == want_count and res["mask_len"] == rec["mask"]["mask_len"] and res["split_ms"] == 0
        assert np.float64(res["pad"]).view(np.uint64) == np.float64(rec["mask"]["pad"]).view(np.uint64)


@pytest.mark.parametrize("case", LEVEL0, ids=mc.case_id)
def test_level_0_f32_and_device_forms(ctx, case):
    (nx, ny, nz), level, roi, seg = case
    _, und = field_of(case[0], np.float64)
    want_count = int(mc.coarse_und(und, case).sum())
    rec32 = record_of(ctx, case[0], "wrs1", seg, np.float32)
    rec = record_of(ctx, case[0], "wrs1", seg)
    nbox = int(np.prod(mc.out_shape(case)))
    buf = ctx.to_device(np.full(nbox + 1, SENTINEL))
    try:
        for fill in (np.nan, -77.25):
            out = np.full(mc.out_shape(case), SENTINEL, np.float32)
            res, _ = ctx.decode_host_seg_roi_masked_f32(out, (nz, ny, nx), 0, roi, rec32, fill)
            assert np.array_equal(ints(out), ints(crop(full_of(ctx, case[0], "wrs1", seg, fill, np.float32), case)))
            assert res["undefined"] == want_count
            res, _ = ctx.decode_seg_roi_masked(buf, (nz, ny, nx), 0, roi, rec, fill)
            got = buf.download(np.float64, nbox + 1)
            assert np.array_equal(ints(got[:nbox]), ints(crop(full_of(ctx, case[0], "wrs1", seg, fill), case).reshape(-1)))
            assert got[nbox] == SENTINEL and res["undefined"] == want_count
    finally:
        buf.free()


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("case", COARSE, ids=mc.case_id)
def test_coarse_levels_are_the_plain_call_with_the_coarse_mask(ctx, case, fmt):
    (nx, ny, nz), level, roi, _ = case
    rec = record_of(ctx, case[0], fmt, seg_of(case, fmt))
    _, und = field_of(case[0], np.float64)
    coarse = mc.coarse_und(und, case)
    base = plain(ctx, case, rec)
    for fill in (np.nan, -77.25):
        out = np.full(mc.out_shape(case), SENTINEL)
        res, _ = ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), level, roi, rec, fill)
        assert np.array_equal(ints(out), ints(np.where(coarse, fill, base)))
        assert res["undefined"] == int(coarse.sum())


def test_coarse_f32_device_and_one_plane(ctx):
    for case in (c for c in COARSE if c[0] in (mc.CHAIN, mc.GENERAL)):
        (nx, ny, nz), level, roi, seg = case
        _, und = field_of(case[0], np.float64)
        coarse = mc.coarse_und(und, case)
        rec32 = record_of(ctx, case[0], "wrs1", seg, np.float32)
        out = np.full(mc.out_shape(case), SENTINEL, np.float32)
        res, _ = ctx.decode_host_seg_roi_masked_f32(out, (nz, ny, nx), level, roi, rec32, -77.25)
        assert np.array_equal(ints(out), ints(np.where(coarse, np.float32(-77.25), plain(ctx, case, rec32, dtype=np.float32))))
        assert res["undefined"] == int(coarse.sum())
        rec = record_of(ctx, case[0], "wrs1", seg)
        nbox = coarse.size
        buf = ctx.to_device(np.full(nbox, SENTINEL))
        try:
            ctx.decode_seg_roi_masked(buf, (nz, ny, nx), level, roi, rec, np.nan)
            got = buf.download(np.float64, nbox).reshape(coarse.shape)
        finally:
            buf.free()
        assert np.array_equal(ints(got), ints(np.where(coarse, np.nan, plain(ctx, case, rec))))
    # max_planes = 1, a region and the whole box
    for case in ((mc.GENERAL, 1, ((1, 6), (0, 11), (2, 19)), 16), (mc.GENERAL, 2, None, 16), (mc.GENERAL, 0, ((2, 11), (3, 19), (5, 36)), 16)):
        (nx, ny, nz), level, roi, seg = case
        rec = record_of(ctx, case[0], "wrs1", seg)
        assert rec["nlay"] > 1
        coarse = mc.coarse_und(field_of(case[0], np.float64)[1], case)
        out = np.full(mc.out_shape(case), SENTINEL)
        ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), level, roi, rec, np.nan, max_planes=1)
        assert np.array_equal(ints(out), ints(np.where(coarse, np.nan, plain(ctx, case, rec, max_planes=1))))


def mask_front(rec):
    """(offset of the mask's first segment stream in rec["data"], seg, the segments' lengths)"""
    at = rec["ntot_enc"] + 32
    magic, seg, nseg = bytes(rec["data"][at:at + 4]), *struct.unpack("<II", bytes(rec["data"][at + 4:at + 12]))
    assert magic == b"WRS1"
    lens = np.frombuffer(bytes(rec["data"][at + 12:at + 12 + 4 * nseg]), "<u4")
    return at + 12 + 4 * nseg, seg, lens


@pytest.mark.parametrize("case", [c for c in mc.CASES if c[3] and c[0] in (mc.GENERAL, mc.FUSED, mc.CHAIN)], ids=mc.case_id)
def test_only_the_listed_mask_segments_are_touched(ctx, case):
    (nx, ny, nz), level, roi, seg = case
    rec = record_of(ctx, case[0], "wrs1", seg)
    first, seg_in_blob, lens = mask_front(rec)
    assert seg_in_blob == seg
    listed = api.mask_roi_segments((nz, ny, nx), level, roi, seg)
    out = np.full(mc.out_shape(case), SENTINEL)
    before = api.stat(api.STAT_MASK_ROI_SEGMENTS), api.stat(api.STAT_MASK_ROI_BYTES_UP)
    ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), level, roi, rec, np.nan)
    assert api.stat(api.STAT_MASK_ROI_SEGMENTS) - before[0] == len(listed)
    assert api.stat(api.STAT_MASK_ROI_BYTES_UP) - before[1] == int(lens[listed].sum())
    if roi is not None:
        assert len(listed) < len(lens)
    starts = first + np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    unlisted = np.setdiff1d(np.arange(len(lens)), listed)
    if len(unlisted):  # damage in a segment the region does not list: the same result, the same return code
        k = int(unlisted[len(unlisted) // 2])
        data = rec["data"].copy()
        data[starts[k] + lens[k] // 2] ^= 0x40
        again = np.full(mc.out_shape(case), SENTINEL)
        res, _ = ctx.decode_host_seg_roi_masked(again, (nz, ny, nx), level, roi, dict(rec, data=data), np.nan)
        assert np.array_equal(ints(again), ints(out))


def test_a_listed_segment_that_does_not_decode_is_refused(ctx):
    case = (mc.GENERAL, 0, ((2, 11), (3, 19), (5, 36)), 16)
    (nx, ny, nz), level, roi, seg = case
    rec = record_of(ctx, case[0], "wrs1", seg)
    first, _, lens = mask_front(rec)
    listed = api.mask_roi_segments((nz, ny, nx), level, roi, seg)
    starts = first + np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    refused = 0
    buf = ctx.to_device(np.full(int(np.prod(mc.out_shape(case))), SENTINEL))
    try:
        for k in listed[:6]:
            data = rec["data"].copy()
            data[starts[k] + 2] ^= 0x40  # (the model's counts at the head of the stream)
            out = np.full(mc.out_shape(case), SENTINEL)
            try:
                ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), level, roi, dict(rec, data=data), np.nan)
            except api.WaveRangeError as e:
                assert "error -4" in str(e)
                assert (out == SENTINEL).all()
                with pytest.raises(api.WaveRangeError):
                    ctx.decode_seg_roi_masked(buf, (nz, ny, nx), level, roi, dict(rec, data=data), np.nan)
                assert (buf.download(np.float64, out.size) == SENTINEL).all()
                refused += 1
    finally:
        buf.free()
    assert refused >= 1, "a flipped bit in the model of a listed segment was never noticed"


def test_a_record_without_a_blob_decodes_as_the_plain_call(ctx):
    for case in ((mc.CHAIN, 0, ((1, 6), (2, 11), (3, 20)), 48), (mc.CHAIN, 2, None, 16)):
        (nx, ny, nz), level, roi, seg = case
        rec = record_of(ctx, case[0], "wrs1", seg)
        out = np.full(mc.out_shape(case), SENTINEL)
        res, _ = ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), level, roi, field_part(rec), np.nan)
        assert np.array_equal(ints(out), ints(plain(ctx, case, rec)))
        assert res == dict(res, undefined=0, pad=0.0, mask_len=0, split_ms=0.0, fill_ms=0.0, mask_coder_ms=0.0)
    # and a record of a field without an undefined sample
    f = synth.field(33, 17, 9, seed=5)
    rec, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, seg=16)
    rec["data"] = rec["data"].copy()
    assert rec["mask"]["mask_len"] == 0
    roi = ((1, 6), (2, 11), (3, 20))
    out, want = np.empty(api.roi_shape(roi)), np.empty(api.roi_shape(roi))
    res, _ = ctx.decode_host_seg_roi_masked(out, f.shape, 0, roi, rec, np.nan)
    ctx.decode_host_seg_roi(want, f.shape, 0, roi, rec)
    assert np.array_equal(ints(out), ints(want)) and res["undefined"] == 0 and res["mask_len"] == 0


def test_constant_padded_field(ctx):
    f = np.full((7, 9, 13), 2.5)
    und = mc.und_recipe(mc.ODD).copy()
    f[und] = np.nan
    rec, _ = ctx.encode_host_seg_masked(f, TOL, seg=16)
    rec["data"] = rec["data"].copy()
    assert rec["nlay"] == 0 and rec["ntot_enc"] == 0
    for case in ((mc.ODD, 0, ((1, 3), (0, 8), (2, 11)), 16), (mc.ODD, 0, None, 16), (mc.ODD, 0, ((3, 4), (4, 5), (6, 7)), 16)):
        roi = case[2]
        coarse = mc.coarse_und(und, case)
        for fill in (np.nan, 9.0):
            want = np.where(coarse, fill, 2.5)
            out = np.full(mc.out_shape(case), SENTINEL)
            res, _ = ctx.decode_host_seg_roi_masked(out, f.shape, 0, roi, rec, fill)
            assert np.array_equal(ints(out), ints(want)) and res["undefined"] == int(coarse.sum())
            out32 = np.full(mc.out_shape(case), SENTINEL, np.float32)
            ctx.decode_host_seg_roi_masked_f32(out32, f.shape, 0, roi, rec, fill)
            assert np.array_equal(ints(out32), ints(want.astype(np.float32)))
            buf = ctx.to_device(np.full(coarse.size, SENTINEL))
            try:
                res, _ = ctx.decode_seg_roi_masked(buf, f.shape, 0, roi, rec, fill)
                got = buf.download(np.float64, coarse.size).reshape(coarse.shape)
            finally:
                buf.free()
            assert np.array_equal(ints(got), ints(want)) and res["undefined"] == int(coarse.sum())


def test_damaged_blobs_are_refused_and_leave_the_output_alone(ctx):
    case = (mc.CHAIN, 0, ((1, 6), (2, 11), (3, 20)), 48)
    (nx, ny, nz), level, roi, seg = case
    rec = record_of(ctx, case[0], "wrs1", seg)
    nt = rec["ntot_enc"]
    planes, blob = rec["data"][:nt], rec["data"][nt:]
    n, count = nx * ny * nz, rec["mask"]["undefined"]

    def head(n_, count_, magic=b"WRM1", reserved=0):
        return np.frombuffer(magic + struct.pack("<IQQd", reserved, n_, count_, 0.0), dtype=np.uint8)

    bad_blobs = {
        "magic": np.concatenate([head(n, count, magic=b"WRM2"), blob[32:]]),
        "reserved": np.concatenate([head(n, count, reserved=7), blob[32:]]),
        "n": np.concatenate([head(n - 1, count), blob[32:]]),
        "truncated": blob[:-1],
        "overlong": np.concatenate([blob, np.zeros(3, np.uint8)]),
        "short header": blob[:17],
    }
    nbox = int(np.prod(mc.out_shape(case)))
    buf = ctx.to_device(np.full(nbox, SENTINEL))
    try:
        for name, bad in bad_blobs.items():
            data = np.concatenate([planes, bad])
            for lvl, r in ((0, roi), (1, None)):
                out = np.full(mc.out_shape((case[0], lvl, r, seg)), SENTINEL)
                with pytest.raises(api.WaveRangeError) as e:
                    ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), lvl, r, dict(rec, data=data), np.nan)
                assert "error -4" in str(e.value), (name, str(e.value))
                assert (out == SENTINEL).all(), name
            with pytest.raises(api.WaveRangeError) as e:
                ctx.decode_seg_roi_masked(buf, (nz, ny, nx), 0, roi, dict(rec, data=data), np.nan)
            assert "error -4" in str(e.value), (name, str(e.value))
            assert (buf.download(np.float64, nbox) == SENTINEL).all(), name
    finally:
        buf.free()
    # and the record still decodes
    out = np.empty(mc.out_shape(case))
    ctx.decode_host_seg_roi_masked(out, (nz, ny, nx), 0, roi, rec, np.nan)
    assert np.array_equal(np.isnan(out), mc.coarse_und(field_of(case[0], np.float64)[1], case))


def test_refused_regions(ctx):
    nx, ny, nz = mc.CHAIN
    rec = record_of(ctx, mc.CHAIN, "wrs1", 16)
    shape = (nz, ny, nx)
    bad = [(0, ((1, 1), (2, 11), (3, 20))), (0, ((1, 6), (2, 18), (3, 20))), (0, ((1, 6), (2, 11), (3, 34))), (2, ((0, 4), (0, 5), (0, 9))), (5, None),
           (5, ((0, 1), (0, 1), (0, 1)))]
    for level, roi in bad:
        out = np.full(api.roi_shape(roi) if roi is not None else (1, 1, 1), SENTINEL)
        info = api.EncInfo.from_dict(rec)
        tm, res = api.Timings(), api.MaskResult()
        box = api._box(roi) if roi is not None else None
        rc = api.lib().wr_decode_host_seg_roi_masked(ctx.h, out.ctypes.data, nx, ny, nz, level, 0, box, info, rec["data"].ctypes.data, rec["data"].size,
                                                   np.nan, tm, res)
        assert rc == -1, (level, roi, rc)
        assert (out == SENTINEL).all()
    # level > wlev: a record coded without the transform has level 0 only
    f, _ = field_of(mc.CHAIN, np.float64)
    flat, _ = ctx.encode_host_seg_masked(f, TOL, BELOW, wtflag=0, seg=16)
    flat["data"] = flat["data"].copy()
    assert flat["wlev"] == 0
    out = np.full(api.lowres_shape(shape, 1), SENTINEL)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_roi_masked(out, shape, 1, None, flat, np.nan)
    assert "error -1" in str(e.value) and (out == SENTINEL).all()
    out = np.full(shape, SENTINEL)
    res, _ = ctx.decode_host_seg_roi_masked(out, shape, 0, None, flat, np.nan)
    assert np.array_equal(np.isnan(out), mc.und_recipe(mc.CHAIN))
