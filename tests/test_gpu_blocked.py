"""The blocked symbol order of segmented streams ("WRS2", include/waverange_amd.h) on the GPU: the reorder kernel against the
permutation, the encoder against the host reference of the format, and every decode of a blocked stream against the same
decode of the WRS1 stream of the same field.  Every comparison is equality of bytes or of bit patterns: the order changes
where a symbol is coded, never its value, so there is no tolerance anywhere."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

# (nz, ny, nx), brick: (203,203,203) has odd origins and extents everywhere (the byte path, every partial-brick case);
# (64,64,64) takes the 16-byte path in its finer levels at bricks 16 and 32 and the byte path in the coarse ones
REORDER = [((64, 64, 64), 8), ((64, 64, 64), 16), ((64, 64, 64), 32), ((77, 129, 200), 8), ((1, 50, 70), 8), ((130, 40, 40), 16),
           ((203, 203, 203), 32)]
# the regions of tests/test_gpu_roi.py, at level 0: ((z0, z1), (y0, y1), (x0, x1))
REGIONS = {
    (203, 203, 203): ((100, 104), (100, 104), (100, 104)),  # window [32,176)^3: the fused inverse on the window only
    (24, 400, 40): ((0, 24), (0, 4), (0, 40)),
    (301, 37, 50): ((150, 153), (0, 37), (49, 50)),
    (77, 129, 200): ((20, 30), (70, 71), (100, 133)),
    (240, 48, 64): ((118, 122), (0, 48), (0, 64)),
    (1, 50, 300): ((0, 1), (10, 20), (140, 160)),
    (64, 64, 64): ((30, 34), (5, 6), (60, 64)),
}
BRICK_OF = {(203, 203, 203): 32, (24, 400, 40): 8, (301, 37, 50): 16, (77, 129, 200): 16, (240, 48, 64): 16, (1, 50, 300): 8, (64, 64, 64): 8}
LEVELS = range(5)


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def field(shape, seed=41):
    return synth.field(shape[2], shape[1], shape[0], seed=seed)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32), b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def own(enc):
    enc[0]["data"] = enc[0]["data"].copy()
    return enc[0]


_STREAMS = {}


def streams(ctx, shape, tol, brick, seg=4096, wtflag=1):
    """One field coded both ways per key: shared by the tests, never written to."""
    key = (shape, tol, brick, seg, wtflag)
    if key not in _STREAMS:
        f = field(shape)
        wrs1 = own(ctx.encode_host_seg(f, tol, wtflag, seg))
        wrs2 = own(ctx.encode_host_seg(f, tol, wtflag, seg, brick=brick))
        _STREAMS[key] = dict(f=f, wrs1=wrs1, wrs2=wrs2)
    return _STREAMS[key]


def same_header(a, b):
    for k in ("tolabs", "midval", "halfspanval"):
        if float(a[k]).hex() != float(b[k]).hex():
            return False
    u = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)  # noqa: E731
    return a["wlev"] == b["wlev"] and a["nlay"] == b["nlay"] and np.array_equal(u(a["deps_vec"]), u(b["deps_vec"])) and \
        np.array_equal(u(a["minval_vec"]), u(b["minval_vec"]))


# ---- wr_dev_plane_reorder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wlev", [0, 4])
@pytest.mark.parametrize("shape,brick", REORDER, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_plane_reorder(ctx, shape, brick, wlev):
    n = int(np.prod(shape))
    pi = api.blocked_order(shape, wlev, brick).astype(np.int64)
    plane = np.random.default_rng(n + brick + wlev).integers(0, 256, n, dtype=np.uint8)
    blocked = ctx.plane_reorder(plane, shape, wlev, brick)
    assert np.array_equal(blocked, plane[pi]), (shape, brick, wlev, "forward")
    want = np.empty_like(plane)
    want[pi] = plane
    assert np.array_equal(ctx.plane_reorder(plane, shape, wlev, brick, inverse=True), want), (shape, brick, wlev, "inverse")
    assert np.array_equal(ctx.plane_reorder(blocked, shape, wlev, brick, inverse=True), plane), (shape, brick, wlev, "round trip")


def test_plane_reorder_defaults_and_refusals(ctx):
    shape = (40, 48, 64)
    plane = np.random.default_rng(1).integers(0, 256, int(np.prod(shape)), dtype=np.uint8)
    assert np.array_equal(ctx.plane_reorder(plane, shape), plane[api.blocked_order(shape, 4, 32).astype(np.int64)])  # brick 0: 32
    assert np.array_equal(ctx.plane_reorder(plane, shape, brick=64), plane[api.blocked_order(shape, 4, 64).astype(np.int64)])
    for wlev, brick in ((4, 12), (4, 128), (3, 32)):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.plane_reorder(plane, shape, wlev, brick)
        assert "error -1" in str(e.value), str(e.value)


# ---- encode ----------------------------------------------------------------------------------------------------------------
def check_encode(ctx, f, tol, wtflag, seg, brick, cutoff=None, m=(1, 1, 1), f32=False, device=False):
    """The blocked stream of a field: the header scalars of the WRS1 stream, every plane the host reference's WRS2 blob of the
    plane that the WRS1 stream holds; the decode of it bit for bit the decode of the WRS1 stream."""
    what = (f.shape, tol, wtflag, seg, brick, m, f32, device)
    if f32:
        f = f.astype(np.float32)
    enc_fn = ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg
    wrs1 = own(enc_fn(f, tol, wtflag, seg, cutoff=cutoff, m=m))
    if device:
        buf = ctx.to_device(f)
        try:
            wrs2 = own(ctx.encode_seg(buf, f.shape, tol, wtflag, seg, cutoff=cutoff, m=m, brick=brick))
        finally:
            buf.free()
    else:
        wrs2 = own(enc_fn(f, tol, wtflag, seg, cutoff=cutoff, m=m, brick=brick))
    assert same_header(wrs2, wrs1), what
    assert wrs2["ntot_enc"] == sum(wrs2["len_enc_vec"]) == wrs2["data"].size, what
    assert wrs2["nlay"] > 0
    for l, (b1, b2) in enumerate(zip(split_planes(wrs1), split_planes(wrs2))):
        plane = api.seg_decode_host_ref(b1, f.size)
        assert np.array_equal(b2, api.seg_encode_host_ref_blocked(plane, f.shape, wrs1["wlev"], brick, seg)), (what, "plane %d" % l)
    want, rec = np.empty_like(f), np.empty_like(f)
    dec_fn = ctx.decode_host_seg_f32 if f32 else ctx.decode_host_seg
    dec_fn(want, wrs1)
    if device:
        buf = ctx.alloc(f.nbytes)
        try:
            ctx.decode_seg(buf, f.shape, wrs2)
            rec = buf.download(np.float64, f.size).reshape(f.shape)
        finally:
            buf.free()
    else:
        dec_fn(rec, wrs2)
    assert same_bits(rec, want), what
    return wrs2


@pytest.mark.parametrize("seg", [1008, 4096, 0])
def test_encode_is_the_host_reference(ctx, seg):
    check_encode(ctx, field((77, 129, 200), seed=7), 1e-6, 1, seg, 8)
    check_encode(ctx, field((64, 64, 64), seed=8), 1e-3, 1, seg, 16)
    check_encode(ctx, field((40, 48, 64), seed=8), 1e-5, 1, seg, 0)  # brick 0: the default


def test_encode_fp32_device_no_transform_local_cutoff(ctx):
    f = field((77, 129, 200), seed=7)
    check_encode(ctx, f, 1e-6, 1, 4096, 16, f32=True)
    check_encode(ctx, f, 1e-6, 1, 4096, 32, device=True)
    wrs2 = check_encode(ctx, f, 1e-6, 0, 4096, 8)  # wtflag = 0: one box, the field
    assert wrs2["wlev"] == 0
    check_encode(ctx, field((64, 64, 64), seed=8), 1e-3, 0, 1008, 32, f32=True)
    # the local-cutoff case of tests/test_gpu_seg.py::test_codec_level_local_cutoff
    cutoff = np.array([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-4, 1e-5], dtype=np.float64)
    check_encode(ctx, synth.field(64, 48, 40, seed=9), None, 1, 4096, 8, cutoff=cutoff, m=(2, 2, 2))


# ---- full decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(203, 203, 203), (64, 64, 64), (1, 50, 300)], ids=lambda s: "x".join(map(str, s)))
def test_full_decode(ctx, shape):
    s = streams(ctx, shape, 1e-6, BRICK_OF[shape])
    f, wrs1, wrs2 = s["f"], s["wrs1"], s["wrs2"]
    want, got = np.empty_like(f), np.empty_like(f)
    ctx.decode_host_seg(want, wrs1)
    ctx.decode_host_seg(got, wrs2)
    assert same_bits(got, want), shape
    want32, got32 = np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)
    ctx.decode_host_seg_f32(want32, wrs1)
    ctx.decode_host_seg_f32(got32, wrs2)
    assert same_bits(got32, want32), shape
    buf = ctx.alloc(f.nbytes)
    try:
        ctx.decode_seg(buf, shape, wrs2)
        assert same_bits(buf.download(np.float64, f.size).reshape(shape), want), shape
    finally:
        buf.free()


def test_constant_field_and_overflow(ctx):
    flat = np.full((8, 6, 10), 3.25)
    enc = own(ctx.encode_host_seg(flat, 1e-6, brick=8))
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    out = np.empty_like(flat)
    ctx.decode_host_seg(out, enc)
    assert np.array_equal(out, flat)
    low = np.empty(api.lowres_shape(flat.shape, 2))
    ctx.decode_host_seg_lowres(low, flat.shape, 2, enc)
    assert np.all(low == 3.25)
    # a cap one byte short: WR_ERR_OVERFLOW
    f = field((40, 48, 64), seed=3)
    enc = own(ctx.encode_host_seg(f, 1e-5, 1, 4096, brick=16))
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg(f, 1e-5, 1, 4096, out=np.empty(enc["ntot_enc"] - 1, dtype=np.uint8), brick=16)
    assert "error -5" in str(e.value), str(e.value)
    exact = own(ctx.encode_host_seg(f, 1e-5, 1, 4096, out=np.empty(enc["ntot_enc"], dtype=np.uint8), brick=16))
    assert np.array_equal(exact["data"], enc["data"])
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg(f, 1e-5, 1, 4096, brick=24)
    assert "error -1" in str(e.value), str(e.value)


# ---- low-resolution and region decode ------------------------------------------------------------------------------------
def index_of(blob):
    assert bytes(blob[:4]) == b"WRS2"
    seg, nseg, brick = (int(v) for v in blob[4:16].view("<u4"))
    return seg, brick, blob[16:16 + 4 * nseg].view("<u4").astype(np.int64)


def masked(enc, sets):
    """A copy of the blocked stream in which every byte of every segment that is not listed is 0xFF; the indices stay."""
    data = enc["data"].copy()
    at = 0
    for (need, lens), ln in zip(sets, enc["len_enc_vec"]):
        start = at + 16 + 4 * lens.size + np.concatenate(([0], np.cumsum(lens)))
        keep = np.zeros(lens.size, dtype=bool)
        keep[need] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    return dict(enc, data=data)


def region_at(shape, level):
    out = []
    for (lo, hi), n in zip(REGIONS[shape], api.lowres_shape(shape, level)):
        a = lo >> level
        out.append((a, min(n, max(a + 1, -(-hi >> level)))))
    return tuple(out)


def lowres_all_ways(ctx, shape, level, enc, p):
    bshape = api.lowres_shape(shape, level)
    h64, h32 = np.empty(bshape), np.empty(bshape, dtype=np.float32)
    ctx.decode_host_seg_lowres(h64, shape, level, enc, p)
    ctx.decode_host_seg_lowres_f32(h32, shape, level, enc, p)
    buf = ctx.alloc(max(h64.nbytes, 16))
    try:
        ctx.decode_seg_lowres(buf, shape, level, enc, p)
        d64 = buf.download(np.float64, h64.size).reshape(bshape)
    finally:
        buf.free()
    return h64, h32, d64


def roi_all_ways(ctx, shape, level, roi, enc, p):
    rshape = api.roi_shape(roi)
    h64, h32 = np.empty(rshape), np.empty(rshape, dtype=np.float32)
    ctx.decode_host_seg_roi(h64, shape, level, roi, enc, p)
    ctx.decode_host_seg_roi_f32(h32, shape, level, roi, enc, p)
    buf = ctx.alloc(max(h64.nbytes, 16))
    try:
        ctx.decode_seg_roi(buf, shape, level, roi, enc, p)
        d64 = buf.download(np.float64, h64.size).reshape(rshape)
    finally:
        buf.free()
    return h64, h32, d64


@pytest.mark.parametrize("shape", list(REGIONS), ids=lambda s: "x".join(map(str, s)))
def test_lowres_decode(ctx, shape):
    """Every level, one plane and all: the blocked stream with everything outside the prefix overwritten gives, bit for bit,
    what the WRS1 stream gives; the counters move by what the list function predicts."""
    brick = BRICK_OF[shape]
    s = streams(ctx, shape, 1e-6, brick)
    wrs1, wrs2 = s["wrs1"], s["wrs2"]
    for level in LEVELS:
        sets = []
        for blob in split_planes(wrs2):
            seg, b, lens = index_of(blob)
            assert b == brick
            sets.append((api.seg_lowres_segments_blocked(shape, level, seg, brick=brick).astype(np.int64), lens))
        bad = masked(wrs2, sets)
        for p in sorted({1, wrs2["nlay"]}):
            want = lowres_all_ways(ctx, shape, level, wrs1, p)
            s0, b0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)
            got = lowres_all_ways(ctx, shape, level, bad, p)
            ds, db = api.stat(api.STAT_LOWRES_SEGMENTS) - s0, api.stat(api.STAT_LOWRES_BYTES_UP) - b0
            assert all(same_bits(g, w) for g, w in zip(got, want)), (shape, level, p)
            assert ds == 3 * sum(need.size for need, _ in sets[:p]), (shape, level, p, ds)
            assert db == 3 * sum(int(lens[need].sum()) for need, lens in sets[:p]), (shape, level, p, db)


@pytest.mark.parametrize("shape", list(REGIONS), ids=lambda s: "x".join(map(str, s)))
def test_region_decode(ctx, shape):
    """The same for the regions of tests/test_gpu_roi.py carried to every level.  (203,203,203): the window [32,176)^3 runs
    the fused inverse."""
    brick = BRICK_OF[shape]
    s = streams(ctx, shape, 1e-6, brick)
    wrs1, wrs2 = s["wrs1"], s["wrs2"]
    if shape == (203, 203, 203):
        win = api.roi_window(shape, 0, REGIONS[shape])
        assert win == ((32, 176),) * 3 and api.fused_plan(tuple(b - a for a, b in win), inverse=True)["used"]
    for level in LEVELS:
        roi = region_at(shape, level)
        sets = []
        for blob in split_planes(wrs2):
            seg, b, lens = index_of(blob)
            sets.append((api.seg_roi_segments_blocked(shape, level, roi, seg, brick=b).astype(np.int64), lens))
        bad = masked(wrs2, sets)
        for p in sorted({1, wrs2["nlay"]}):
            want = roi_all_ways(ctx, shape, level, roi, wrs1, p)
            s0, b0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
            got = roi_all_ways(ctx, shape, level, roi, bad, p)
            ds, db = api.stat(api.STAT_ROI_SEGMENTS) - s0, api.stat(api.STAT_ROI_BYTES_UP) - b0
            assert all(same_bits(g, w) for g, w in zip(got, want)), (shape, level, p)
            assert ds == 3 * sum(need.size for need, _ in sets[:p]), (shape, level, p, ds)
            assert db == 3 * sum(int(lens[need].sum()) for need, lens in sets[:p]), (shape, level, p, db)
    # max_planes = 0 means all of them; level 0 with every plane is the crop of the full decode
    roi = REGIONS[shape]
    full, got = np.empty(shape), np.empty(api.roi_shape(roi))
    ctx.decode_host_seg(full, wrs2)
    ctx.decode_host_seg_roi(got, shape, 0, roi, wrs2)
    assert same_bits(got, np.ascontiguousarray(full[tuple(slice(lo, hi) for lo, hi in roi)])), shape


def test_default_segment_length_launches_what_the_geometry_lists(ctx):
    """(203,203,203) at the default segment length and brick 32.  The probe's window is 144 of 203 samples per axis, most of
    every subband: the blocked stream needs 135 of the 140 segments where row-major needs 114 -- the order pays at sizes where a
    window is a small part of a subband (tests/test_blocked_cpu.py::test_known_counts), not here; level 3 needs 1 against 18."""
    shape = (203, 203, 203)
    roi = REGIONS[shape]
    blocked, rowmajor = api.seg_roi_segments_blocked(shape, 0, roi), api.seg_roi_segments(shape, 0, roi)
    assert (blocked.size, rowmajor.size) == (135, 114)
    assert (api.seg_lowres_segments_blocked(shape, 3).size, api.seg_lowres_segments(shape, 3).size) == (1, 18)
    s = streams(ctx, shape, 1e-6, 32, seg=0)
    want, got = np.empty(api.roi_shape(roi)), np.empty(api.roi_shape(roi))
    ctx.decode_host_seg_roi(want, shape, 0, roi, s["wrs1"])
    s0 = api.stat(api.STAT_ROI_SEGMENTS)
    ctx.decode_host_seg_roi(got, shape, 0, roi, s["wrs2"])
    assert api.stat(api.STAT_ROI_SEGMENTS) - s0 == blocked.size * s["wrs2"]["nlay"]
    assert same_bits(got, want)
    want, got = np.empty(api.lowres_shape(shape, 3)), np.empty(api.lowres_shape(shape, 3))
    ctx.decode_host_seg_lowres(want, shape, 3, s["wrs1"])
    s0 = api.stat(api.STAT_LOWRES_SEGMENTS)
    ctx.decode_host_seg_lowres(got, shape, 3, s["wrs2"])
    assert api.stat(api.STAT_LOWRES_SEGMENTS) - s0 == s["wrs2"]["nlay"]
    assert same_bits(got, want)


def test_without_transform(ctx):
    shape = (77, 129, 200)
    s = streams(ctx, shape, 1e-6, 16, wtflag=0)
    wrs1, wrs2, roi = s["wrs1"], s["wrs2"], REGIONS[shape]
    assert wrs2["wlev"] == 0
    for p in sorted({1, wrs2["nlay"]}):
        assert all(same_bits(g, w) for g, w in zip(roi_all_ways(ctx, shape, 0, roi, wrs2, p), roi_all_ways(ctx, shape, 0, roi, wrs1, p)))
        assert all(same_bits(g, w) for g, w in zip(lowres_all_ways(ctx, shape, 0, wrs2, p), lowres_all_ways(ctx, shape, 0, wrs1, p)))
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_lowres(np.empty(api.lowres_shape(shape, 1)), shape, 1, wrs2)
    assert "error -1" in str(e.value), str(e.value)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refused_before_any_launch(ctx):
    """A corrupted brick field, planes of mixed formats, planes with different bricks: WR_ERR_STREAM from the host-side check,
    no segment launched, and the context goes on working.  Run once each."""
    shape = (64, 64, 64)
    s = streams(ctx, shape, 1e-6, 8)
    wrs1, wrs2, f = s["wrs1"], s["wrs2"], s["f"]
    assert wrs2["nlay"] >= 2
    out, low, reg = np.empty(shape), np.empty(api.lowres_shape(shape, 2)), np.empty((4, 1, 4))
    other = own(ctx.encode_host_seg(f, 1e-6, 1, 4096, brick=16))
    first = wrs2["len_enc_vec"][0]

    def spliced(a, b):
        """plane 0 of stream a, the other planes of stream b"""
        pa, pb = split_planes(a), split_planes(b)
        blobs = [pa[0]] + pb[1:]
        return dict(b, data=np.concatenate(blobs), len_enc_vec=[int(x.size) for x in blobs], ntot_enc=int(sum(x.size for x in blobs)))

    cases = []
    for brick in (0, 7, 128, 24):
        bad = dict(wrs2, data=wrs2["data"].copy())
        bad["data"][12:16] = np.frombuffer(struct.pack("<I", brick), dtype=np.uint8)
        cases.append((bad, "brick"))
        last = dict(wrs2, data=wrs2["data"].copy())  # in a plane that a one-plane decode does not use
        last["data"][first + 12:first + 16] = np.frombuffer(struct.pack("<I", brick), dtype=np.uint8)
        cases.append((last, "brick"))
    cases.append((spliced(wrs1, wrs2), "mixes"))
    cases.append((spliced(wrs2, wrs1), "mixes"))
    cases.append((spliced(other, wrs2), "differ"))
    for bad, word in cases:
        s0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_ROI_SEGMENTS)
        for call in (lambda: ctx.decode_host_seg(out, bad), lambda: ctx.decode_host_seg_lowres(low, shape, 2, bad, 1),
                     lambda: ctx.decode_host_seg_roi(reg, shape, 0, REGIONS[shape], bad, 1)):
            with pytest.raises(api.WaveRangeError) as e:
                call()
            assert "error -4" in str(e.value) and word in str(e.value), str(e.value)
        assert (api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_ROI_SEGMENTS)) == s0
    want = np.empty(shape)
    ctx.decode_host_seg(want, wrs1)
    ctx.decode_host_seg(out, wrs2)
    assert same_bits(out, want)


def test_flipped_payload(ctx):
    """Payload bytes flipped behind a valid index: WR_ERR_STREAM or a field of n samples, and the context goes on working.
    Run once."""
    shape = (64, 64, 64)
    s = streams(ctx, shape, 1e-6, 8)
    wrs2 = s["wrs2"]
    bad = dict(wrs2, data=wrs2["data"].copy())
    rng = np.random.default_rng(3)
    at = 0
    for blob, ln in zip(split_planes(wrs2), wrs2["len_enc_vec"]):
        _, _, lens = index_of(blob)
        idx = rng.integers(at + 16 + 4 * lens.size, at + ln, 64)
        bad["data"][idx] ^= rng.integers(1, 256, 64).astype(np.uint8)
        at += ln
    out = np.full(shape, np.nan)
    try:
        ctx.decode_host_seg(out, bad)
        assert out.size == s["f"].size
    except api.WaveRangeError as e:
        assert "error -4" in str(e), str(e)
    good, want = np.empty(shape), np.empty(shape)
    ctx.decode_host_seg(good, wrs2)
    ctx.decode_host_seg(want, s["wrs1"])
    assert same_bits(good, want)


# ---- pooled planes that span two chunks -----------------------------------------------------------------------------------
CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api, synth
import test_gpu_blocked as t
api.set_verbosity(0)
with api.Context(0) as ctx:
    f = synth.field(128, 128, 128, seed=13)
    for brick, seg in ((32, 0), (8, 4096)):
        wrs2 = t.check_encode(ctx, f, 1e-6, 1, seg, brick)
        wrs1 = t.own(ctx.encode_host_seg(f, 1e-6, 1, seg))
        roi = ((60, 70), (0, 128), (30, 31))
        for level in (0, 2):
            r = tuple((lo >> level, max((lo >> level) + 1, hi >> level)) for lo, hi in roi)
            assert all(t.same_bits(g, w) for g, w in zip(t.roi_all_ways(ctx, f.shape, level, r, wrs2, 0), t.roi_all_ways(ctx, f.shape, level, r, wrs1, 0)))
            assert all(t.same_bits(g, w) for g, w in zip(t.lowres_all_ways(ctx, f.shape, level, wrs2, 0), t.lowres_all_ways(ctx, f.shape, level, wrs1, 0)))
print("ok")
"""


def test_planes_that_span_two_chunks(tmp_path):
    """WR_PLANE_CHUNK_MB=1: a 128^3 plane lives in two chunks of 1 MiB, so the reorder kernel's natural-order side goes through
    the chunk table in both directions, whole and by brick list."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]
