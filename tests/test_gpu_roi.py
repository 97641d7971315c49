"""Region decode of segmented streams on the GPU (include/waverange_amd.h, "Region decode").

The expected result is the crop of D(r, p), which is built on the CPU as tests/test_gpu_lowres.py builds it: the oracle's
dequantiser and transform on planes recovered by the host reference of the format.  Every comparison of values is equality
of bit patterns: the definition is a crop of an existing result, so there is no tolerance anywhere."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401
from test_gpu_lowres import encode_seg, expected, field, recut, same_bits, split_planes
from oracle.loader import Oracle
from waverange_amd import api

pytestmark = pytest.mark.gpu

# (nz, ny, nx) -> the region at level 0, ((z0, z1), (y0, y1), (x0, x1))
REGIONS = {
    (203, 203, 203): ((100, 104), (100, 104), (100, 104)),  # window [32,176)^3: the fused inverse on the window only
    (24, 400, 40): ((0, 24), (0, 4), (0, 40)),               # a window cut in y only
    (301, 37, 50): ((150, 153), (0, 37), (49, 50)),          # odd extents, true-end windows in y and x
    (77, 129, 200): ((20, 30), (70, 71), (100, 133)),        # partial in x only: every segment needed, still exact
    (240, 48, 64): ((118, 122), (0, 48), (0, 64)),           # the 4-wide gather path
    (1, 50, 300): ((0, 1), (10, 20), (140, 160)),            # a degenerate axis
    (64, 64, 64): ((30, 34), (5, 6), (60, 64)),              # the window is the whole field
}
SHAPES = list(REGIONS)
TOLS = [1e-3, 1e-6]
LEVELS = range(5)
# needed / nseg at level 0, from the geometry alone (tests/test_roi_cpu.py::test_known_counts)
CUT = [((203, 203, 203), 4096, 1448, 2043), ((203, 203, 203), 59904, 114, 140), ((24, 400, 40), 4096, 72, 94), ((301, 37, 50), 4096, 91, 136)]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


_STREAMS = {}


def stream(ctx, shape, tol, seg=4096, wtflag=1):
    """One coded field per key, with its planes and the D(r, p) computed so far: shared by the tests, never written to."""
    key = (shape, tol, seg, wtflag)
    if key not in _STREAMS:
        f = field(shape)
        enc = encode_seg(ctx, f, tol, seg, wtflag)
        planes = [api.seg_decode_host_ref(b, f.size) for b in split_planes(enc)]
        _STREAMS[key] = dict(f=f, enc=enc, planes=planes, D={})
    return _STREAMS[key]


def D(oracle, s, shape, level, p):
    if (level, p) not in s["D"]:
        s["D"][level, p] = expected(oracle, s["planes"], s["enc"], shape, level, p)
    return s["D"][level, p]


def region_at(shape, level):
    """The level-0 region of the shape, carried to the coordinates of the box of `level`."""
    out = []
    for (lo, hi), n in zip(REGIONS[shape], api.lowres_shape(shape, level)):
        a = lo >> level
        out.append((a, min(n, max(a + 1, -(-hi >> level)))))
    return tuple(out)


def crop(a, roi):
    return np.ascontiguousarray(a[tuple(slice(lo, hi) for lo, hi in roi)])


def decode_all_ways(ctx, shape, level, roi, enc, p):
    """(float64 from the host call, float32 from the fp32 call, float64 from the device-output call)"""
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


def check_stream(ctx, oracle, s, shape, enc, what):
    for level in LEVELS:
        roi = region_at(shape, level)
        for p in sorted({1, enc["nlay"]}):
            want = crop(D(oracle, s, shape, level, p), roi)
            h64, h32, d64 = decode_all_ways(ctx, shape, level, roi, enc, p)
            assert same_bits(h64, want), (what, level, p, "host")
            assert same_bits(d64, want), (what, level, p, "device")
            assert same_bits(h32, want.astype(np.float32)), (what, level, p, "fp32")


def test_paths_of_the_fused_case():
    """(203,203,203) itself runs the general kernels; its region's window is 144 = 9 x 16 per axis and runs the fused inverse."""
    shape = SHAPES[0]
    win = api.roi_window(shape, 0, REGIONS[shape])
    assert win == ((32, 176),) * 3
    assert not api.fused_plan(shape, inverse=True)["used"]
    plan = api.fused_plan(tuple(b - a for a, b in win), inverse=True)
    assert plan["used"] and plan["levels"] >= 2


# ---- values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_stage_level(ctx, oracle, shape, tol):
    s = stream(ctx, shape, tol)
    enc, planes, n = s["enc"], s["planes"], s["f"].size
    info = api.EncInfo.from_dict(enc)
    pitch = api.lib().wr_plane_pitch(n)
    host = np.zeros(pitch * enc["nlay"], dtype=np.uint8)
    for l, q in enumerate(planes):
        host[l * pitch:l * pitch + n] = q
    d_planes, d_out = ctx.to_device(host), ctx.alloc(max(8 * n, 16))
    try:
        for level in LEVELS:
            roi = region_at(shape, level)
            box = tuple((0, b) for b in api.lowres_shape(shape, level))
            for p in sorted({1, enc["nlay"]}):
                full = D(oracle, s, shape, level, p)
                for r in (roi, box):
                    want = crop(full, r)
                    ctx.decode_planes_roi(d_out, shape, level, r, d_planes, info, p)
                    assert same_bits(d_out.download(np.float64, want.size).reshape(want.shape), want), (shape, tol, level, p, r)
                if p == enc["nlay"]:  # max_planes = 0 means all of them
                    ctx.decode_planes_roi(d_out, shape, level, roi, d_planes, info)
                    want = crop(full, roi)
                    assert same_bits(d_out.download(np.float64, want.size).reshape(want.shape), want), (shape, tol, level, "all")
        for level, p, r in ((5, 0, roi), (-1, 0, roi), (0, enc["nlay"] + 1, roi), (0, -1, roi), (0, 0, ((0, 1), (0, 1), (3, 3))),
                            (0, 0, ((0, 1), (0, 1), (0, shape[2] + 1))), (1, 0, tuple((0, n) for n in shape))):
            with pytest.raises(api.WaveRangeError) as e:
                ctx.decode_planes_roi(d_out, shape, level, r, d_planes, info, p)
            assert "error -1" in str(e.value), str(e.value)
    finally:
        d_planes.free()
        d_out.free()


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_codec_level(ctx, oracle, shape, tol):
    s = stream(ctx, shape, tol)
    check_stream(ctx, oracle, s, shape, s["enc"], (shape, tol, 4096))
    # planes cut at different segment lengths
    check_stream(ctx, oracle, s, shape, recut(s["enc"], s["planes"], (1008, 4096, api.SEG_DEFAULT)), (shape, tol, "mixed"))


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_other_decodes(ctx, shape):
    """Level 0 with every plane is the crop of the full decode; the whole box of a level is the low-resolution decode."""
    enc, f = stream(ctx, shape, 1e-6)["enc"], stream(ctx, shape, 1e-6)["f"]
    full = np.empty_like(f)
    ctx.decode_host_seg(full, enc)
    roi = REGIONS[shape]
    got = np.empty(api.roi_shape(roi))
    ctx.decode_host_seg_roi(got, shape, 0, roi, enc)
    assert same_bits(got, crop(full, roi)), shape
    for level in LEVELS:
        bshape = api.lowres_shape(shape, level)
        low, whole = np.empty(bshape), np.empty(bshape)
        ctx.decode_host_seg_lowres(low, shape, level, enc)
        ctx.decode_host_seg_roi(whole, shape, level, tuple((0, b) for b in bshape), enc)
        assert same_bits(whole, low), (shape, level)


def test_without_transform_and_constant_field(ctx, oracle):
    shape = (77, 129, 200)
    s = stream(ctx, shape, 1e-6, wtflag=0)
    enc, roi = s["enc"], REGIONS[shape]
    assert enc["wlev"] == 0
    assert api.roi_window(shape, 0, roi, wlev=0) == roi
    for p in sorted({1, enc["nlay"]}):
        want = crop(D(oracle, s, shape, 0, p), roi)
        h64, h32, d64 = decode_all_ways(ctx, shape, 0, roi, enc, p)
        assert same_bits(h64, want) and same_bits(d64, want) and same_bits(h32, want.astype(np.float32)), p
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_roi(np.empty((1, 1, 1)), shape, 1, ((0, 1),) * 3, enc)
    assert "error -1" in str(e.value), str(e.value)
    # a constant field comes back as midval at the region's size
    flat = np.full((8, 6, 10), 3.25)
    enc, _ = ctx.encode_host_seg(flat, 1e-6)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    for level, roi in ((0, ((2, 5), (0, 6), (9, 10))), (2, ((0, 2), (1, 2), (0, 3)))):
        h64, h32, d64 = decode_all_ways(ctx, flat.shape, level, roi, enc, 0)
        assert h64.shape == api.roi_shape(roi)
        assert np.all(h64 == 3.25) and np.all(d64 == 3.25) and np.all(h32 == np.float32(3.25)), level


# ---- only what is needed is read ---------------------------------------------------------------------------------------
def index_of(blob):
    seg, nseg = (int(v) for v in blob[4:12].view("<u4"))
    return seg, blob[12:12 + 4 * nseg].view("<u4").astype(np.int64)


def needed_sets(enc, shape, level, roi):
    """Per plane: (needed ids, segment lengths from the index)."""
    out = []
    for blob in split_planes(enc):
        seg, lens = index_of(blob)
        out.append((api.seg_roi_segments(shape, level, roi, seg, wlev=enc["wlev"]).astype(np.int64), lens))
    return out


def masked(enc, sets):
    """A copy of the stream in which every byte of every segment that is not listed is 0xFF; the indices stay."""
    data = enc["data"].copy()
    at = 0
    for (need, lens), ln in zip(sets, enc["len_enc_vec"]):
        start = at + 12 + 4 * lens.size + np.concatenate(([0], np.cumsum(lens)))
        keep = np.zeros(lens.size, dtype=bool)
        keep[need] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    return dict(enc, data=data)


@pytest.mark.parametrize("shape,seg,needed,nseg", CUT)
def test_only_listed_segments_are_read(ctx, oracle, shape, seg, needed, nseg):
    s = stream(ctx, shape, 1e-6)
    roi = REGIONS[shape]
    enc = s["enc"] if seg == 4096 else recut(s["enc"], s["planes"], (seg,))
    sets = needed_sets(enc, shape, 0, roi)
    assert all((need.size, lens.size) == (needed, nseg) for need, lens in sets) and needed < nseg
    want = crop(D(oracle, s, shape, 0, enc["nlay"]), roi)
    bad = masked(enc, sets)
    assert not np.array_equal(bad["data"], enc["data"])
    low0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)
    s0, b0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
    h64, h32, d64 = decode_all_ways(ctx, shape, 0, roi, bad, 0)
    ds, db = api.stat(api.STAT_ROI_SEGMENTS) - s0, api.stat(api.STAT_ROI_BYTES_UP) - b0
    assert same_bits(h64, want) and same_bits(d64, want) and same_bits(h32, want.astype(np.float32)), (shape, seg)
    # three calls: each launches the listed segments of every plane and uploads their streams, and nothing else
    assert ds == 3 * needed * enc["nlay"], (shape, seg, ds)
    assert db == 3 * sum(int(lens[need].sum()) for need, lens in sets), (shape, seg, db)
    # fewer planes: fewer segments
    s0 = api.stat(api.STAT_ROI_SEGMENTS)
    one = np.empty(api.roi_shape(roi))
    ctx.decode_host_seg_roi(one, shape, 0, roi, bad, 1)
    assert api.stat(api.STAT_ROI_SEGMENTS) - s0 == needed
    assert same_bits(one, crop(D(oracle, s, shape, 0, 1), roi)), (shape, seg, "one plane")
    # the low-resolution counters have not moved, and a low-resolution decode does not move the region's
    assert (api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)) == low0
    r0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
    ctx.decode_host_seg_lowres(np.empty(api.lowres_shape(shape, 3)), shape, 3, enc)
    assert api.stat(api.STAT_LOWRES_SEGMENTS) > low0[0] and api.stat(api.STAT_LOWRES_BYTES_UP) > low0[1]
    assert (api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)) == r0


def test_mixed_cuts_and_coarser_levels_launch_what_the_geometry_lists(ctx, oracle):
    shape = (203, 203, 203)
    s = stream(ctx, shape, 1e-6)
    enc = recut(s["enc"], s["planes"], (1008, 4096, api.SEG_DEFAULT))
    for level in (0, 2, 4):
        roi = region_at(shape, level)
        sets = needed_sets(enc, shape, level, roi)
        bad = masked(enc, sets)
        got = np.empty(api.roi_shape(roi))
        s0, b0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
        ctx.decode_host_seg_roi(got, shape, level, roi, bad)
        assert api.stat(api.STAT_ROI_SEGMENTS) - s0 == sum(need.size for need, _ in sets), level
        assert api.stat(api.STAT_ROI_BYTES_UP) - b0 == sum(int(lens[need].sum()) for need, lens in sets), level
        assert same_bits(got, crop(D(oracle, s, shape, level, enc["nlay"]), roi)), level


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_corrupted_segments(ctx, oracle):
    """A flipped count-table byte inside a listed segment: WR_ERR_STREAM, and the context goes on working; the same byte in
    a segment that is not listed changes nothing, while its index is still validated.  Run once."""
    shape = (24, 400, 40)
    s = stream(ctx, shape, 1e-6)
    enc, roi = s["enc"], REGIONS[shape]
    want = crop(D(oracle, s, shape, 0, enc["nlay"]), roi)
    out = np.empty(api.roi_shape(roi))
    need, lens = needed_sets(enc, shape, 0, roi)[0]

    def flipped(k):
        bad = dict(enc, data=enc["data"].copy())
        bad["data"][12 + 4 * lens.size + int(lens[:k].sum()) + 40] ^= 0x55  # inside the 256 counts at the head of segment k's stream
        return bad

    bad = flipped(int(need[len(need) // 2]))
    with pytest.raises(api.WaveRangeError):  # (the host reference refuses the segment too: its counts no longer add up)
        api.seg_decode_host_ref(split_planes(bad)[0], s["f"].size)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_roi(out, shape, 0, roi, bad)
    assert "error -4" in str(e.value), str(e.value)
    ctx.decode_host_seg_roi(out, shape, 0, roi, enc)
    assert same_bits(out, want)
    other = np.setdiff1d(np.arange(lens.size), need)
    assert other.size
    out[:] = 0
    ctx.decode_host_seg_roi(out, shape, 0, roi, flipped(int(other[0])))
    assert same_bits(out, want)
    # the index of an unlisted segment, and of an unused plane, is validated before anything is launched
    first = sum(enc["len_enc_vec"][:enc["nlay"] - 1])
    for at, plane_at in ((12 + 4 * int(other[0]), 0), (12 + 4 * int(other[0]), first), (0, first)):
        bad = dict(enc, data=enc["data"].copy())
        bad["data"][plane_at + at] ^= 1
        s0 = api.stat(api.STAT_ROI_SEGMENTS)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_host_seg_roi(out, shape, 0, roi, bad, 1)
        assert "error -4" in str(e.value), str(e.value)
        assert api.stat(api.STAT_ROI_SEGMENTS) == s0


def test_refusals(ctx):
    shape = (64, 64, 64)
    enc = stream(ctx, shape, 1e-3)["enc"]
    info = api.EncInfo.from_dict(enc)
    data = enc["data"]
    big = np.empty(shape)
    good = api.Box(0, 0, 0, 8, 8, 8)
    for fn in (api.lib().wr_decode_host_seg_roi, api.lib().wr_decode_host_seg_roi_f32):
        def call(level, p, box):
            return fn(ctx.h, big.ctypes.data, 64, 64, 64, level, p, api.C.byref(box) if box else None, api.C.byref(info), data.ctypes.data, data.size, None)
        assert call(0, 0, good) == 0
        for level, p, box in ((5, 0, good), (-1, 0, good), (1, enc["nlay"] + 1, good), (1, -1, good), (0, 0, None),
                              (0, 0, api.Box(0, 0, 0, 8, 0, 8)), (0, 0, api.Box(4, 0, 0, 3, 8, 8)), (0, 0, api.Box(0, 0, 0, 8, 8, 65)),
                              (0, 0, api.Box(-1, 0, 0, 8, 8, 8)), (1, 0, api.Box(0, 0, 0, 33, 8, 8)), (4, 0, api.Box(0, 0, 0, 4, 4, 5))):
            assert call(level, p, box) == -1, (level, p, box and tuple(getattr(box, k) for k, _ in box._fields_))
    out = np.empty((4, 4, 4))
    ctx.decode_host_seg_roi(out, shape, 4, ((0, 4),) * 3, enc)  # and the context goes on working
