"""Every driver of the segmented formats on the same small coded fields: what the stages they share do through each.

The full decode, the box decode, the single-region and the multi-region decode, a batch of two, the transcode from a segmented
source and the three stage calls (wr_dev_seg_decode, _batch, _lists) parse the same stream, lay out the same work buffers and
run the same coder stage.  This file drives one field through all of them and pins the values (bit patterns, against the full
decode and its crops), the stat counters, the non-zero pattern of wr_timings' coder fields, and code and text of the errors
the shared stages raise.  The expected texts are the library's as they were before the drivers were folded onto one set of
stages; they are literals here on purpose."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401
from roi_multi_cases import SETS, regions_at
from test_gpu_lowres import field, same_bits, split_planes
from test_gpu_roi import crop
from waverange_amd import api

pytestmark = pytest.mark.gpu

C = api.C
TOL, SEG = 1e-6, 1008
FORMATS = {"wrs1": dict(), "wrs2": dict(brick=16), "wrs3": dict(strands=8)}
HEAD = {"wrs1": 12, "wrs2": 16, "wrs3": 20}  # bytes in front of a plane's index
CASES = [("W", "wrs1"), ("W", "wrs2"), ("W", "wrs3"), ("T", "wrs1"), ("T", "wrs2"), ("T", "wrs3")]
STATS = (api.STAT_LOWRES_SEGMENTS, api.STAT_LOWRES_BYTES_UP, api.STAT_ROI_SEGMENTS, api.STAT_ROI_BYTES_UP, api.STAT_ROI_CODER_LAUNCHES)
BAD = "1 segment(s) do not decode to their symbols"


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


_CODED = {}


def coded(ctx, name):
    """Per region set: the field, its three streams, and the full decodes (all planes; the first plane alone) that everything
    else is compared with.  Computed once, never written to."""
    if name not in _CODED:
        shape = SETS[name][0]
        f = field(shape)
        encs = {}
        for fmt, kw in FORMATS.items():
            enc, _ = ctx.encode_host_seg(f, TOL, 1, SEG, **kw)
            enc["data"] = enc["data"].copy()
            encs[fmt] = enc
        nlay = encs["wrs1"]["nlay"]
        assert nlay >= 2 and all(e["nlay"] == nlay and e["wlev"] == 4 for e in encs.values())
        full = {nlay: np.empty(shape), 1: np.empty(shape)}
        ctx.decode_host_seg(full[nlay], encs["wrs1"])
        ctx.decode_host_seg(full[1], first_planes(encs["wrs1"], 1))
        _CODED[name] = dict(shape=shape, f=f, encs=encs, nlay=nlay, full=full, box2={})
    return _CODED[name]


def first_planes(enc, p):
    """The stream of the first p planes: its full decode is what a decode with max_planes = p stops at."""
    ln = enc["len_enc_vec"][:p]
    return dict(enc, nlay=p, len_enc_vec=ln, ntot_enc=sum(ln), data=enc["data"][:sum(ln)], deps_vec=enc["deps_vec"][:p], minval_vec=enc["minval_vec"][:p])


def box2(ctx, s, p):
    """The box of level 2 from the first p planes, as the box decode of the WRS1 stream gives it: the other streams, the
    regions' crops and the device and fp32 outputs are compared with it"""
    if p not in s["box2"]:
        s["box2"][p] = np.empty(api.lowres_shape(s["shape"], 2))
        ctx.decode_host_seg_lowres(s["box2"][p], s["shape"], 2, s["encs"]["wrs1"], p)
    return s["box2"][p]


def index_of(blob, fmt):
    nseg = int(blob[8:12].view("<u4")[0])
    return blob[HEAD[fmt]:HEAD[fmt] + 4 * nseg].view("<u4").astype(np.int64)


def ids_of(fmt, shape, level, rois):
    """The segments a decode of `rois` (None: the box of `level`) lists in every plane."""
    brick = FORMATS[fmt].get("brick")
    if rois is None:
        return api.seg_lowres_segments(shape, level, SEG) if brick is None else api.seg_lowres_segments_blocked(shape, level, SEG, 4, brick)
    return api.seg_roi_segments_multi(shape, level, rois, SEG, wlev=4, brick=brick)


def listed(enc, fmt, ids, p):
    """(segments, bytes of their streams) over the first p planes"""
    ids = np.asarray(ids, dtype=np.int64)
    return ids.size * p, sum(int(index_of(b, fmt)[ids].sum()) for b in split_planes(enc)[:p])


class Counters:
    def __enter__(self):
        self.at = [api.stat(k) for k in STATS]
        return self

    def __exit__(self, *exc):
        self.delta = tuple(api.stat(k) - a for k, a in zip(STATS, self.at))


def coder_pattern(tm, count):
    """plane_coder_s is positive in its first `count` entries and zero behind them, and rangecoder is their sum"""
    s = tm["plane_coder_s"]
    return all(v > 0 for v in s[:count]) and all(v == 0 for v in s[count:]) and tm["rangecoder"] == sum(s[:count])


def device_out(ctx, count, call):
    buf = ctx.alloc(max(8 * count, 16))
    try:
        tm = call(buf)
        return buf.download(np.float64, count), tm
    finally:
        buf.free()


# ---- values, counters, timings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt", CASES)
def test_full_and_box(ctx, name, fmt):
    s = coded(ctx, name)
    shape, enc, nlay = s["shape"], s["encs"][fmt], s["nlay"]
    n = int(np.prod(shape))
    with Counters() as k:
        h64, h32 = np.empty(shape), np.empty(shape, dtype=np.float32)
        tm = ctx.decode_host_seg(h64, enc)
        tm32 = ctx.decode_host_seg_f32(h32, enc)
        d64, tmd = device_out(ctx, n, lambda buf: ctx.decode_seg(buf, shape, enc))
    assert same_bits(h64, s["full"][nlay]) and same_bits(d64.reshape(shape), s["full"][nlay]) and same_bits(h32, s["full"][nlay].astype(np.float32))
    assert k.delta == (0, 0, 0, 0, 0)
    assert all(coder_pattern(t, nlay) for t in (tm, tm32, tmd)), (tm, tm32, tmd)
    for level in (0, 2):
        bshape = api.lowres_shape(shape, level)
        ids = ids_of(fmt, shape, level, None)
        for p in (1, nlay):
            with Counters() as k:
                h64, h32 = np.empty(bshape), np.empty(bshape, dtype=np.float32)
                tm = ctx.decode_host_seg_lowres(h64, shape, level, enc, p)
                ctx.decode_host_seg_lowres_f32(h32, shape, level, enc, p)
                d64, _ = device_out(ctx, h64.size, lambda buf: ctx.decode_seg_lowres(buf, shape, level, enc, p))
            want = s["full"][p] if level == 0 else box2(ctx, s, p)
            assert same_bits(h64, want) and same_bits(d64.reshape(bshape), want) and same_bits(h32, want.astype(np.float32)), (level, p)
            segs, nbytes = listed(enc, fmt, ids, p)
            assert k.delta == (3 * segs, 3 * nbytes, 0, 0, 0), (level, p, k.delta)
            assert coder_pattern(tm, p), (level, p, tm)
    assert 0 < ids_of(fmt, shape, 2, None).size < -(-n // SEG)  # the box of level 2 lists some segments, not all


@pytest.mark.parametrize("name,fmt", CASES)
def test_regions(ctx, name, fmt):
    s = coded(ctx, name)
    shape, enc, nlay = s["shape"], s["encs"][fmt], s["nlay"]
    one_launch = fmt != "wrs3"
    for level in (0, 2):
        rois = regions_at(name, level)
        offs = api.roi_multi_offsets(shape, level, rois)
        for p in (1, nlay):
            full = s["full"][p] if level == 0 else box2(ctx, s, p)
            # ---- one region per call: a launch per used plane
            for r in rois:
                rshape = api.roi_shape(r)
                with Counters() as k:
                    h64, h32 = np.empty(rshape), np.empty(rshape, dtype=np.float32)
                    tm = ctx.decode_host_seg_roi(h64, shape, level, r, enc, p)
                    ctx.decode_host_seg_roi_f32(h32, shape, level, r, enc, p)
                    d64, _ = device_out(ctx, h64.size, lambda buf: ctx.decode_seg_roi(buf, shape, level, r, enc, p))
                want = crop(full, r)
                assert same_bits(h64, want) and same_bits(d64.reshape(rshape), want) and same_bits(h32, want.astype(np.float32)), (level, p, r)
                segs, nbytes = listed(enc, fmt, ids_of(fmt, shape, level, [r]), p)
                assert k.delta == (0, 0, 3 * segs, 3 * nbytes, 3 * p), (level, p, r, k.delta)
                assert coder_pattern(tm, p), (level, p, r, tm)
            # ---- all regions in one call: one launch over the used planes, or a launch per plane of a WRS3 stream
            with Counters() as k:
                tm = {}
                h64 = ctx.decode_host_seg_rois(shape, level, rois, enc, p, timings=tm)
                h32 = ctx.decode_host_seg_rois(shape, level, rois, enc, p, dtype=np.float32)
                flat, _ = device_out(ctx, int(offs[-1]), lambda buf: ctx.decode_seg_rois(buf, shape, level, rois, enc, p))
            for i, r in enumerate(rois):
                want = crop(full, r)
                d64 = flat[offs[i]:offs[i + 1]].reshape(api.roi_shape(r))
                assert same_bits(h64[i], want) and same_bits(d64, want) and same_bits(h32[i], want.astype(np.float32)), (level, p, i)
            segs, nbytes = listed(enc, fmt, ids_of(fmt, shape, level, rois), p)
            assert k.delta == (0, 0, 3 * segs, 3 * nbytes, 3 * (1 if one_launch else p)), (level, p, k.delta)
            assert coder_pattern(tm, 1 if one_launch else p), (level, p, tm)
            assert not one_launch or tm["plane_coder_s"][0] == tm["rangecoder"]


@pytest.mark.parametrize("name", ["W", "T"])
def test_batch_of_two(ctx, name):
    s = coded(ctx, name)
    shape, nlay = s["shape"], s["nlay"]
    short = first_planes(s["encs"]["wrs2"], 1)  # the second field has one plane: plane index 1 is a launch over one job
    with Counters() as k:
        outs = [np.empty(shape), np.empty(shape)]
        tm = ctx.decode_host_seg_batch(outs, [s["encs"]["wrs1"], short])
        o32 = [np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)]
        ctx.decode_host_seg_batch_f32(o32, [s["encs"]["wrs2"], s["encs"]["wrs1"]])
    assert same_bits(outs[0], s["full"][nlay]) and same_bits(outs[1], s["full"][1])
    assert same_bits(o32[0], s["full"][nlay].astype(np.float32)) and same_bits(o32[1], s["full"][nlay].astype(np.float32))
    assert k.delta == (0, 0, 0, 0, 0)
    assert coder_pattern(tm, nlay), tm  # one entry per plane index
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_batch(outs, [s["encs"]["wrs1"], s["encs"]["wrs3"]])
    assert str(e.value) == ("libwaverange_amd error -3: field 1: a WRS3 stream: stranded segments are not decoded in a batch "
                            "(wr_decode_host_seg reads them)")


@pytest.mark.parametrize("name,fmt", CASES)
def test_transcode_from_a_segmented_source(ctx, name, fmt):
    s = coded(ctx, name)
    shape, enc, nlay = s["shape"], s["encs"][fmt], s["nlay"]
    for target in ("ref", "wrs1:seg=4096", "wrs2:seg=1008:brick=16"):
        want, _ = api.transcode_host_ref(shape, enc, enc["data"], target)
        with Counters() as k:
            tm = {}
            got, info = ctx.transcode(enc, enc["data"], target, shape=shape, timings=tm)
        assert got.tobytes() == want.tobytes() and info["nlay"] == nlay, target
        assert k.delta == (0, 0, 0, 0, 0)
        assert all(v > 0 for v in tm["plane_coder_s"][:nlay]) and all(v == 0 for v in tm["plane_coder_s"][nlay:]) and tm["rangecoder"] > 0, tm
    assert got.tobytes() == s["encs"]["wrs2"]["data"].tobytes()  # the last target is the format of the wrs2 stream


@pytest.mark.parametrize("name", ["W", "T"])
def test_stage_calls(ctx, name):
    s = coded(ctx, name)
    shape, nlay = s["shape"], s["nlay"]
    n = int(np.prod(shape))
    blobs = {fmt: split_planes(s["encs"][fmt]) for fmt in FORMATS}
    planes = [api.seg_decode_host_ref(b, n) for b in blobs["wrs1"]]
    with Counters() as k:
        for l in (0, nlay - 1):
            for fmt in ("wrs1", "wrs3"):  # (a WRS3 blob in the natural order decodes to the plane itself)
                sym, bad = ctx.seg_decode_plane(blobs[fmt][l], n)
                assert bad == 0 and np.array_equal(sym, planes[l]), (fmt, l)
        syms, bad = ctx.seg_decode_planes_batch(blobs["wrs1"], n)
        assert bad == [0] * nlay and all(np.array_equal(a, b) for a, b in zip(syms, planes))
        # lists: every other segment of a WRS1 blob, the last (short) segment alone, nothing, and a WRS2 blob in stream order
        nseg = -(-n // SEG)
        order = api.blocked_order(shape, 4, 16)
        lists = [np.arange(0, nseg, 2), [nseg - 1], [], np.arange(1, nseg, 3)]
        jobs = [blobs["wrs1"][0], blobs["wrs1"][nlay - 1], blobs["wrs1"][0], blobs["wrs2"][0]]
        src = [planes[0], planes[nlay - 1], planes[0], planes[0][order]]
        syms, bad = ctx.seg_decode_lists(jobs, [n] * 4, lists)
        assert bad == [0] * 4
        for j in range(4):
            want = np.full(n, 0xEE, dtype=np.uint8)
            for i in lists[j]:
                want[int(i) * SEG:(int(i) + 1) * SEG] = src[j][int(i) * SEG:(int(i) + 1) * SEG]
            assert np.array_equal(syms[j], want), j
    assert k.delta == (0, 0, 0, 0, 0)
    assert n % SEG != 0  # a short last segment


# ---- errors of the shared stages, through every driver -------------------------------------------------------------------
def entries(ctx, s, fmt, p):
    """name -> (call(info, data pointer, data length) -> rc, message prefix, planes it decodes): every driver on the W field,
    straight at the C entry points so that a null buffer can be passed"""
    shape = s["shape"]
    nz, ny, nx = shape
    L, h = api.lib(), ctx.h
    n = int(np.prod(shape))
    out = np.empty(n + 512)  # the two regions of "regions" behind one another
    box = api.Box(0, 0, 0, nx, ny, nz)
    boxes = (api.Box * 2)(box, api.Box(0, 0, 0, 8, 8, 8))
    good = s["encs"]["wrs1"]
    good_info, cap = api.EncInfo.from_dict(good), api.transcode_bound(n, s["nlay"], api._format_args("wrs1:seg=4096"))
    t_out, t_info = np.empty(cap, dtype=np.uint8), api.EncInfo()

    def batch(info, data, ln):
        infos = (api.EncInfo * 2)(good_info, info)
        outs = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
        datas = (C.c_void_p * 2)(good["data"].ctypes.data, data)
        lens = (C.c_size_t * 2)(good["data"].size, ln)
        return L.wr_decode_host_seg_batch(h, 2, outs, nx, ny, nz, infos, datas, lens, None)

    e = {
        "full": (lambda i, d, ln: L.wr_decode_host_seg(h, out.ctypes.data, nx, ny, nz, C.byref(i), d, ln, None), "", s["nlay"]),
        "box": (lambda i, d, ln: L.wr_decode_host_seg_lowres(h, out.ctypes.data, nx, ny, nz, 0, p, C.byref(i), d, ln, None), "", p),
        "region": (lambda i, d, ln: L.wr_decode_host_seg_roi(h, out.ctypes.data, nx, ny, nz, 0, p, C.byref(box), C.byref(i), d, ln, None), "", p),
        "regions": (lambda i, d, ln: L.wr_decode_host_seg_roi_multi(h, out.ctypes.data, nx, ny, nz, 0, p, boxes, 2, C.byref(i), d, ln, None), "", p),
        "transcode": (lambda i, d, ln: L.wr_transcode_host(h, nx, ny, nz, C.byref(i), d, ln, *api._format_args("wrs1:seg=4096"), C.byref(t_info),
                                                           t_out.ctypes.data, cap, None), "", s["nlay"]),
    }
    if fmt != "wrs3":
        e["batch"] = (batch, "field 1: ", s["nlay"])
    return e, out


def last_error():
    return api.lib().wr_last_error().decode()


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("p", [1, 0])
def test_errors(ctx, fmt, p):
    s = coded(ctx, "W")
    enc, nlay = s["encs"][fmt], s["nlay"]
    p = p or nlay
    calls, out = entries(ctx, s, fmt, p)
    data = enc["data"]

    def run(what, want_rc, want_text, call, info_dict, buf):
        info = api.EncInfo.from_dict(info_dict)
        rc = call(info, buf.ctypes.data if buf is not None else None, buf.size if buf is not None else 0)
        assert (rc, last_error() if rc else "") == (want_rc, want_text), (what, rc, last_error())

    for name, (call, who, used) in calls.items():
        run((name, "good"), 0, "", call, enc, data)
        run((name, "lengths"), -4, who + "len_enc_vec exceeds ntot_enc", call, dict(enc, ntot_enc=enc["ntot_enc"] - 1), data)
        run((name, "short"), -4, who + "ntot_enc exceeds the length of the coded buffer", call, dict(enc, ntot_enc=data.size + 1), data)
        run((name, "null"), -1, who + "null coded buffer", call, enc, None)
        # one byte inside the model at the head of the first segment's stream, behind a valid index: the kernels flag the segment
        for l in sorted({0, used - 1}):
            at = sum(enc["len_enc_vec"][:l])
            bad = data.copy()
            bad[at + HEAD[fmt] + 4 * int(bad[at + 8:at + 12].view("<u4")[0]) + 3] ^= 0x55
            run((name, "flipped", l), -4, who + "plane %d: " % l + BAD, call, enc, bad)
        run((name, "good again"), 0, "", call, enc, data)
        assert name == "transcode" or same_bits(out[:out.size - 512].reshape(s["shape"]), s["full"][used]), name


def test_errors_of_the_stage_calls(ctx):
    s = coded(ctx, "W")
    n = int(np.prod(s["shape"]))
    for fmt in ("wrs1", "wrs3"):
        bad = split_planes(s["encs"][fmt])[0].copy()
        bad[HEAD[fmt] + 4 * int(bad[8:12].view("<u4")[0]) + 3] ^= 0x55
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_plane(bad, n)
        assert str(e.value) == "libwaverange_amd error -4: segmented plane: " + BAD, fmt
    good = split_planes(s["encs"]["wrs1"])[0]
    bad = good.copy()
    bad[HEAD["wrs1"] + 4 * int(bad[8:12].view("<u4")[0]) + 3] ^= 0x55
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_planes_batch([good, bad], n)
    assert str(e.value) == "libwaverange_amd error -4: job 1: segmented plane: " + BAD
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_lists([good, bad], [n, n], [[0, 1], [0, 5]])
    assert str(e.value) == "libwaverange_amd error -4: job 1: segmented plane: " + BAD
    syms, nbad = ctx.seg_decode_lists([good, bad], [n, n], [[0, 1], [5]])  # the flipped segment is not listed
    assert nbad == [0, 0]
    for call, text in ((lambda b: ctx.seg_decode_plane(b, n), "segmented plane: shorter than its header"),
                       (lambda b: ctx.seg_decode_planes_batch([good, b], n), "job 1: segmented plane: shorter than its header"),
                       (lambda b: ctx.seg_decode_lists([good, b], [n, n], [[0], [0]]), "job 1: segmented plane: shorter than its header")):
        with pytest.raises(api.WaveRangeError) as e:
            call(good[:8])
        assert str(e.value) == "libwaverange_amd error -4: " + text


def test_constant_field(ctx):
    """ntot_enc == 0: midval, at the element count of what the call returns"""
    shape = SETS["T"][0]
    enc, _ = ctx.encode_host_seg(np.full(shape, 3.25), TOL, 1, SEG)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    n = int(np.prod(shape))

    def check(count, host, host32, dev):
        h64, h32 = np.zeros(count + 1), np.zeros(count + 1, dtype=np.float32)  # one element more: it stays
        host(h64[:count])
        host32(h32[:count])
        d64, _ = device_out(ctx, count, dev)
        assert np.all(h64[:count] == 3.25) and h64[count] == 0 and np.all(h32[:count] == np.float32(3.25)) and h32[count] == 0 and np.all(d64 == 3.25)

    check(n, lambda o: ctx.decode_host_seg(o.reshape(shape), enc), lambda o: ctx.decode_host_seg_f32(o.reshape(shape), enc),
          lambda buf: ctx.decode_seg(buf, shape, enc))
    for level in (0, 2):
        bshape = api.lowres_shape(shape, level)
        check(int(np.prod(bshape)), lambda o: ctx.decode_host_seg_lowres(o.reshape(bshape), shape, level, enc),
              lambda o: ctx.decode_host_seg_lowres_f32(o.reshape(bshape), shape, level, enc), lambda buf: ctx.decode_seg_lowres(buf, shape, level, enc))
        rois = regions_at("T", level)
        r = rois[0]
        check(int(np.prod(api.roi_shape(r))), lambda o: ctx.decode_host_seg_roi(o.reshape(api.roi_shape(r)), shape, level, r, enc),
              lambda o: ctx.decode_host_seg_roi_f32(o.reshape(api.roi_shape(r)), shape, level, r, enc), lambda buf: ctx.decode_seg_roi(buf, shape, level, r, enc))
        total = int(api.roi_multi_offsets(shape, level, rois)[-1])
        for dt in (np.float64, np.float32):
            got = ctx.decode_host_seg_rois(shape, level, rois, enc, dtype=dt)
            assert sum(g.size for g in got) == total and all(np.all(g == dt(3.25)) for g in got)
        d64, _ = device_out(ctx, total, lambda buf: ctx.decode_seg_rois(buf, shape, level, rois, enc))
        assert np.all(d64 == 3.25)
    # in a batch, between two coded fields
    s = coded(ctx, "T")
    outs = [np.zeros(shape) for _ in range(3)]
    ctx.decode_host_seg_batch(outs, [s["encs"]["wrs1"], enc, s["encs"]["wrs2"]])
    assert same_bits(outs[0], s["full"][s["nlay"]]) and np.all(outs[1] == 3.25) and same_bits(outs[2], s["full"][s["nlay"]])
    # a transcode passes the header through
    got, info = ctx.transcode(enc, enc["data"], "wrs3", shape=shape)
    assert got.size == 0 and info["ntot_enc"] == 0 and info["midval"] == 3.25
