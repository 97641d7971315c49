"""Every encode driver of the segmented formats on the same small fields: what the stages they share do through each.

The single-field encode (host, fp32 host and device fields), the batch, the transcode's two target halves, the stage calls
(wr_dev_seg_encode, _strands, _batch) and the encodes to a byte budget and to an error bound upload a field the same way, code
a plane into a blob the same way, and read lengths back and copy blobs out the same way.  This file drives three fields
through all of them and pins the coded bytes and every wr_enc_info field (driver against driver), the residual, the non-zero
pattern of wr_timings, the stat counters, and code and text of the refusals the shared stages make.  The expected texts are the
library's as they were before the encode drivers were folded onto one set of stages; they are literals here on purpose.

Shapes (nz, ny, nx): the smallest at which each upload branch and each trial-copy branch of the encode is taken; the test
looks the dispatch up itself (api.fused_plan), so a changed dispatch rule fails here instead of dropping a branch."""
import ctypes as C
import math

import numpy as np
import pytest

from util import ROOT  # noqa: F401
from test_gpu_lowres import same_bits, split_planes
from test_gpu_seg_drivers import FORMATS, coder_pattern, field
from waverange_amd import api

pytestmark = pytest.mark.gpu

TOL, SEG = 1e-6, 1008
# all four levels fused: an fp32 field lands in the field buffer, a bounded encode needs no copy of the field
# two fused levels: fused, but no min/max records: a bounded encode copies the field
# one level, not fused: an fp32 field lands in scratch and is widened
SHAPES = {"fused4": (64, 64, 64), "fused2": (20, 24, 40), "general": (18, 18, 18)}
PLAN = {"fused4": (4, True), "fused2": (2, True), "general": (1, False)}
TARGET = {"wrs1": "wrs1:seg=1008", "wrs2": "wrs2:seg=1008:brick=16", "wrs3": "wrs3:seg=1008:strands=8"}
BOUNDED = {"wrs1": dict(), "wrs2": dict(brick=16), "wrs3": dict(strands=8)}
HEAD = {"wrs1": 12, "wrs3": 20}
CASES = [(s, d) for s in SHAPES for d in ("f64", "f32")]

BAD_SEG = "segment length must be a multiple of 16 in [16, 59999]"
BAD_BRICK = "brick edge must be one of 8, 16, 32, 64"
BAD_STRANDS = "strands must be one of 1, 2, 4, 8, 16, 32 with 16 * strands <= seg"
TOO_LARGE = "Error: encoded array is too large. Use larger SAFETY_BUFFER_FACTOR"
ERR = "libwaverange_amd error %d: %s"


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def own(r):
    enc = r[0] if isinstance(r, tuple) else r
    enc["data"] = enc["data"].copy()
    return enc


def same_stream(a, b):
    """byte for byte, and every wr_enc_info field"""
    return (a["data"].tobytes() == b["data"].tobytes() and a["ntot_enc"] == b["ntot_enc"] == a["data"].size
            and all(float(a[k]).hex() == float(b[k]).hex() for k in ("tolabs", "midval", "halfspanval"))
            and a["wlev"] == b["wlev"] and a["nlay"] == b["nlay"] and list(a["len_enc_vec"]) == list(b["len_enc_vec"])
            and same_bits(a["deps_vec"], b["deps_vec"]) and same_bits(a["minval_vec"], b["minval_vec"]))


_CODED = {}


def coded(ctx, name, dt):
    """Per shape and field type: the field, the stream of encode_host_seg in the three formats and of encode_host in the
    reference's.  Computed once, never written to."""
    if (name, dt) not in _CODED:
        shape = SHAPES[name]
        plan = api.fused_plan(shape)
        assert (plan["levels"], plan["used"]) == PLAN[name], plan
        f = field(shape)
        if dt == "f32":
            f = f.astype(np.float32)
        seg_call, ref_call = (ctx.encode_host_seg, ctx.encode_host) if dt == "f64" else (ctx.encode_host_seg_f32, ctx.encode_host_f32)
        encs = {fmt: own(seg_call(f, TOL, 1, SEG, **kw)) for fmt, kw in FORMATS.items()}
        ref = own(ref_call(f, TOL))
        nlay = ref["nlay"]
        assert nlay >= 2 and all(e["nlay"] == nlay and e["wlev"] == 4 for e in encs.values())
        _CODED[(name, dt)] = dict(shape=shape, f=f, encs=encs, ref=ref, nlay=nlay, n=int(np.prod(shape)))
    return _CODED[(name, dt)]


def planes_of(ctx, f64):
    n = f64.size
    pitch = api.lib().wr_plane_pitch(n)
    buf, planes = ctx.to_device(f64), ctx.alloc(pitch * api.NLAYMAX)
    try:
        info = ctx.encode_planes(buf, f64.shape, TOL, planes)
        return [planes.download(np.uint8, n, offset=l * pitch).copy() for l in range(info.nlay)]
    finally:
        buf.free()
        planes.free()


# ---- cross-driver byte identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", CASES)
def test_single_field_drivers(ctx, name, dt):
    s = coded(ctx, name, dt)
    shape, f, nlay = s["shape"], s["f"], s["nlay"]
    wide = f.astype(np.float64)  # (the device-field call takes fp64; widening is exact)
    for fmt, kw in FORMATS.items():
        want = s["encs"][fmt]
        buf = ctx.to_device(wide)
        try:
            got, tm = ctx.encode_seg(buf, shape, TOL, 1, SEG, **kw)
        finally:
            buf.free()
        assert same_stream(own(got), want), fmt
        assert coder_pattern(tm, nlay), (fmt, tm)
        # the transcode into this format: from the reference's stream and from the other segmented formats
        for src in ("ref", "wrs1", "wrs2", "wrs3"):
            if src == fmt:
                continue
            e = s["ref"] if src == "ref" else s["encs"][src]
            tm = {}
            data, info = ctx.transcode(e, e["data"], TARGET[fmt], shape=shape, timings=tm)
            assert same_stream(info, want), (src, fmt)
            if src != "ref":  # both halves add into the same entries (in another order than the entries are summed in)
                c = tm["plane_coder_s"]
                assert all(v > 0 for v in c[:nlay]) and all(v == 0 for v in c[nlay:]) and math.isclose(tm["rangecoder"], sum(c[:nlay]), rel_tol=1e-12), (src, fmt, tm)
    # the planes one by one through the stage calls
    planes = planes_of(ctx, wide)
    assert len(planes) == nlay
    blobs1, blobs3 = split_planes(s["encs"]["wrs1"]), split_planes(s["encs"]["wrs3"])
    for l in range(nlay):
        assert ctx.seg_encode_plane(planes[l], SEG).tobytes() == blobs1[l].tobytes(), l
        assert ctx.seg_encode_plane(planes[l], SEG, strands=8).tobytes() == blobs3[l].tobytes(), l
    got = ctx.seg_encode_planes_batch(planes, SEG)
    assert [g.tobytes() for g in got] == [b.tobytes() for b in blobs1]


@pytest.mark.parametrize("name,dt", CASES)
def test_batch(ctx, name, dt):
    s = coded(ctx, name, dt)
    shape, f = s["shape"], s["f"]
    single, batch = (ctx.encode_host_seg, ctx.encode_host_seg_batch) if dt == "f64" else (ctx.encode_host_seg_f32, ctx.encode_host_seg_batch_f32)
    g = field(shape, seed=7).astype(f.dtype)
    const = np.full(shape, 3.25, dtype=f.dtype)
    for fmt in ("wrs1", "wrs2"):
        kw = FORMATS[fmt]
        want_g = own(single(g, TOL, 1, SEG, **kw))
        encs, tm = batch([f, g], TOL, 1, SEG, **kw)
        assert same_stream(encs[0], s["encs"][fmt]) and same_stream(encs[1], want_g), fmt
        maxlay = max(s["nlay"], want_g["nlay"])
        assert coder_pattern(tm, maxlay) and tm["h2d_ms"] > 0 and tm["d2h_ms"] > 0, (fmt, tm)
        encs, tm = batch([f, const, g], TOL, 1, SEG, **kw)
        assert same_stream(encs[0], s["encs"][fmt]) and same_stream(encs[2], want_g), fmt
        assert encs[1]["nlay"] == 0 and encs[1]["ntot_enc"] == 0 and encs[1]["midval"] == 3.25
        assert coder_pattern(tm, maxlay), (fmt, tm)
    if dt == "f64":  # device fields
        bufs = [ctx.to_device(f), ctx.to_device(g)]
        try:
            encs, tm = ctx.encode_seg_batch(bufs, shape, TOL, 1, SEG, brick=16)
        finally:
            for b in bufs:
                b.free()
        assert same_stream(encs[0], s["encs"]["wrs2"]) and same_stream(encs[1], want_g)
        assert coder_pattern(tm, maxlay) and tm["h2d_ms"] == 0, tm


@pytest.mark.parametrize("name,dt", CASES)
def test_budget_and_bounded(ctx, name, dt):
    s = coded(ctx, name, dt)
    shape, f = s["shape"], s["f"]
    f32 = dt == "f32"
    single = ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg
    # ---- to a byte budget (WRS1): what the plain call at 1e-6 takes, plus 1 %
    max_bytes = s["encs"]["wrs1"]["ntot_enc"] * 101 // 100
    calls = [ctx.encode_host_seg_budget_f32 if f32 else ctx.encode_host_seg_budget]
    if not f32:
        calls.append(lambda fld, *a, **k: device_call(ctx, fld, lambda buf: ctx.encode_seg_budget(buf, shape, *a, **k)))
    for call in calls:
        at = api.stat(api.STAT_BUDGET_CODER_RUNS)
        info, data, res = call(f, max_bytes, seg=SEG)
        info = own(info)
        assert api.stat(api.STAT_BUDGET_CODER_RUNS) - at == info["nlay"] >= 1
        assert same_stream(info, own(single(f, res["tolrel"], 1, SEG))) and info["ntot_enc"] <= res["bound"] <= max_bytes
        assert coder_pattern(res["timings"], info["nlay"]), res
    # ---- to an error bound, the three formats
    max_err = 1e-5 * float(np.abs(f.astype(np.float64)).max())
    for fmt, kw in BOUNDED.items():
        calls = [ctx.encode_host_seg_bounded_f32 if f32 else ctx.encode_host_seg_bounded]
        if not f32 and fmt == "wrs2":
            calls.append(lambda fld, *a, **k: device_call(ctx, fld, lambda buf: ctx.encode_seg_bounded(buf, shape, *a, **k)))
        for call in calls:
            at = api.stat(api.STAT_BOUNDED_CODER_RUNS)
            info, data, res = call(f, max_err, seg=SEG, **kw)
            info = own(info)
            assert api.stat(api.STAT_BOUNDED_CODER_RUNS) - at == info["nlay"] >= 1, fmt
            assert same_stream(info, own(single(f, res["tolrel"], 1, SEG, **FORMATS[fmt]))) and res["err"] <= max_err, fmt
            assert coder_pattern(res["timings"], info["nlay"]), (fmt, res)


def device_call(ctx, fld, call):
    buf = ctx.to_device(fld)
    try:
        return call(buf)
    finally:
        buf.free()


# ---- the reference target ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", CASES)
def test_reference_target(ctx, name, dt):
    """Once with room for every plane at the sum of the bounds before it, once with cap at the exact total: no plane but the
    first fits at its place then, the others go through the context's buffers and the gaps are closed from there."""
    s = coded(ctx, name, dt)
    shape, f, ref = s["shape"], s["f"], s["ref"]
    total = ref["ntot_enc"]
    ref_call = ctx.encode_host if dt == "f64" else ctx.encode_host_f32
    for cap in (None, total):
        got, tm = ref_call(f, TOL, out=None if cap is None else np.empty(cap, dtype=np.uint8))
        assert same_stream(own(got), ref), cap
        assert tm["h2d_ms"] > 0 and tm["d2h_ms"] > 0 and tm["rangecoder"] == max(tm["plane_coder_s"]) > 0, tm
        for fmt, enc in s["encs"].items():
            tm = {}
            data, info = ctx.transcode(enc, enc["data"], "ref", shape=shape, cap=cap, timings=tm)
            assert same_stream(info, ref), (fmt, cap)
            assert all(v > 0 for v in tm["plane_coder_s"][:s["nlay"]]) and tm["rangecoder"] > 0, tm


# ---- the residual -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_residual(ctx, name):
    s = coded(ctx, name, "f64")
    shape, f = s["shape"], s["f"]
    ctx.set_keep_residual(True)
    try:
        want = f.copy()
        assert same_stream(own(ctx.encode_host(want, TOL)), s["ref"])
        assert not same_bits(want, f)
        for fmt, kw in FORMATS.items():
            src = f.copy()
            assert same_stream(own(ctx.encode_host_seg(src, TOL, 1, SEG, **kw)), s["encs"][fmt]), fmt
            assert same_bits(src, want), fmt
            buf = ctx.to_device(f)
            try:
                assert same_stream(own(ctx.encode_seg(buf, shape, TOL, 1, SEG, **kw)), s["encs"][fmt]), fmt
                assert same_bits(buf.download(np.float64, f.size).reshape(shape), want), fmt
            finally:
                buf.free()
        for call, code, text in (
                (lambda: ctx.encode_host_seg_batch([f, f], TOL, 1, SEG), -3,
                 "a batch does not write residuals back: wr_ctx_set_keep_residual(ctx, 0) for batched encodes"),
                (lambda: ctx.encode_host_seg_budget(f, 1 << 30, seg=SEG), -3,
                 "an encode to a byte budget does not keep the residual: wr_ctx_set_keep_residual(ctx, 0)"),
                (lambda: ctx.encode_host_seg_bounded(f, 1.0, seg=SEG), -3,
                 "an encode to an error bound does not keep the residual: wr_ctx_set_keep_residual(ctx, 0)"),
                (lambda: ctx.encode_host_seg_f32(f.astype(np.float32), TOL, 1, SEG), -3,
                 "an fp32 field cannot take the residual back: wr_ctx_set_keep_residual(ctx, 0) for fp32 encodes")):
            with pytest.raises(api.WaveRangeError) as e:
                call()
            assert str(e.value) == ERR % (code, text)
    finally:
        ctx.set_keep_residual(False)
    assert same_stream(own(ctx.encode_host_seg(f, TOL, 1, SEG)), s["encs"]["wrs1"])


# ---- timings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", CASES)
def test_timings_of_the_host_calls(ctx, name, dt):
    s = coded(ctx, name, dt)
    call = ctx.encode_host_seg if dt == "f64" else ctx.encode_host_seg_f32
    for fmt, kw in FORMATS.items():
        enc, tm = call(s["f"], TOL, 1, SEG, **kw)
        assert coder_pattern(tm, s["nlay"]) and tm["h2d_ms"] > 0 and tm["d2h_ms"] > 0, (fmt, tm)
        assert tm["quant_ms"] > 0 and tm["transform_ms"] > 0 and tm["total"] > 0 and tm["gpu"] > 0 and tm["transfer"] == 0, (fmt, tm)


# ---- refusals: code and full text -------------------------------------------------------------------------------------------
def last_error():
    return api.lib().wr_last_error().decode()


def refused(rc, code, text):
    return (rc, last_error() if rc else "") == (code, text)


def test_parameter_refusals_of_the_pipeline_calls(ctx):
    """Each of the three refusals through every encode entry point that takes the parameter; where two bad arguments meet,
    which one wins."""
    s = coded(ctx, "general", "f64")
    nz, ny, nx = s["shape"]
    L, h = api.lib(), ctx.h
    f64, f32 = s["f"], s["f"].astype(np.float32)
    dbuf = ctx.to_device(f64)
    cut = np.array([TOL])
    cp = cut.ctypes.data_as(C.POINTER(C.c_double))
    out = np.empty(1 << 20, dtype=np.uint8)
    info, bres, nres = api.EncInfo(), api.BudgetResult(), api.BoundedResult()
    dims = (nx, ny, nz, 1, 1, 1, 1)
    tail = (out.ctypes.data, out.size, None)
    # name -> (call(field pointer, seg, brick, strands, info), the parameters it takes, its text for a null field)
    entries = {}
    for kind, p, null in (("host", f64.ctypes.data, "null field pointer"), ("host_f32", f32.ctypes.data, "null field pointer"),
                          ("device", dbuf.ptr, "null device field pointer")):
        plain = {"host": L.wr_encode_host_seg, "host_f32": L.wr_encode_host_seg_f32, "device": L.wr_encode_device_seg}[kind]
        blocked = {"host": L.wr_encode_host_seg_blocked, "host_f32": L.wr_encode_host_seg_blocked_f32, "device": L.wr_encode_device_seg_blocked}[kind]
        strands = {"host": L.wr_encode_host_seg_strands, "host_f32": L.wr_encode_host_seg_strands_f32, "device": L.wr_encode_device_seg_strands}[kind]
        budget = {"host": L.wr_encode_host_seg_budget, "host_f32": L.wr_encode_host_seg_budget_f32, "device": L.wr_encode_device_seg_budget}[kind]
        bounded = {"host": L.wr_encode_host_seg_bounded, "host_f32": L.wr_encode_host_seg_bounded_f32, "device": L.wr_encode_device_seg_bounded}[kind]
        entries[kind + " seg"] = (lambda q, sg, b, k, i, fn=plain: fn(h, q, *dims, cp, sg, i, *tail), "s", p, null)
        entries[kind + " blocked"] = (lambda q, sg, b, k, i, fn=blocked: fn(h, q, *dims, cp, sg, b, i, *tail), "sb", p, null)
        entries[kind + " strands"] = (lambda q, sg, b, k, i, fn=strands: fn(h, q, *dims, cp, sg, b, k, i, *tail), "sbk", p, null)
        entries[kind + " budget"] = (lambda q, sg, b, k, i, fn=budget: fn(h, q, *dims, 1 << 30, 2.0 ** -60, sg, i, *tail, C.byref(bres)), "s", p, null)
        entries[kind + " bounded"] = (lambda q, sg, b, k, i, fn=bounded: fn(h, q, *dims, 1.0, 2.0 ** -60, sg, b, k, i, *tail, C.byref(nres)), "sbk", p, null)
    try:
        for name, (call, takes, p, null) in entries.items():
            ok = C.byref(info)
            device = name.startswith("device")
            assert refused(call(p, 17, 16, 8, ok), -1, BAD_SEG), name
            assert refused(call(p, 60000, 16, 8, ok), -1, BAD_SEG), name
            assert refused(call(p, 17, 16, 8, None), -1, BAD_SEG), name           # a bad seg and a null wr_enc_info
            assert refused(call(None, 17, 16, 8, ok), -1, null if device else BAD_SEG), name  # a bad seg and a null field
            assert refused(call(None, SEG, 16, 8, ok), -1, null), name
            assert refused(call(p, SEG, 16, 8, None), -1, "null wr_enc_info"), name
            if "b" in takes:
                assert refused(call(p, SEG, 17, 8, ok), -1, BAD_BRICK), name
                assert refused(call(p, 17, 17, 8, ok), -1, BAD_SEG), name         # seg before brick
                assert refused(call(p, SEG, 17, 8, None), -1, BAD_BRICK), name
                assert refused(call(None, SEG, 17, 8, ok), -1, null if device else BAD_BRICK), name
            if "k" in takes:
                assert refused(call(p, SEG, 16, 3, ok), -1, BAD_STRANDS), name
                assert refused(call(p, 32, 0, 4, ok), -1, BAD_STRANDS), name      # 16 * strands > seg
                assert refused(call(p, SEG, 17, 3, ok), -1, BAD_BRICK), name      # brick before strands
                assert refused(call(p, SEG, 16, 3, None), -1, BAD_STRANDS), name
                assert refused(call(None, SEG, 16, 3, ok), -1, null if device else BAD_STRANDS), name
        # a null result record is refused before the format parameters are looked at
        assert refused(L.wr_encode_host_seg_budget(h, f64.ctypes.data, *dims, 1 << 30, 2.0 ** -60, 17, C.byref(info), *tail, None), -1, "null wr_budget_result")
        assert refused(L.wr_encode_host_seg_bounded(h, f64.ctypes.data, *dims, 1.0, 2.0 ** -60, 17, 0, 0, C.byref(info), *tail, None), -1, "null wr_bounded_result")
        # the cutoff description, behind the format parameters
        bad_m = (nx, ny, nz, 1, 0, 1, 1)
        assert refused(L.wr_encode_host_seg(h, f64.ctypes.data, *bad_m, cp, SEG, C.byref(info), *tail), -1, "bad local cutoff description")
        assert refused(L.wr_encode_host_seg(h, f64.ctypes.data, *dims, None, SEG, C.byref(info), *tail), -1, "bad local cutoff description")
        assert refused(L.wr_encode_host_seg(h, f64.ctypes.data, *bad_m, cp, 17, C.byref(info), *tail), -1, BAD_SEG)
        assert refused(L.wr_encode_host(h, f64.ctypes.data, *bad_m, cp, C.byref(info), *tail), -1, "bad local cutoff description")
        assert refused(L.wr_encode_host(h, None, *dims, cp, C.byref(info), *tail), -1, "null field pointer")
        # everything still codes
        assert same_stream(own(ctx.encode_host_seg(f64, TOL, 1, SEG)), s["encs"]["wrs1"])
    finally:
        dbuf.free()


def test_parameter_refusals_of_the_batch(ctx):
    s = coded(ctx, "general", "f64")
    nz, ny, nx = s["shape"]
    L, h = api.lib(), ctx.h
    f64, f32 = s["f"], s["f"].astype(np.float32)
    dbufs = [ctx.to_device(f64), ctx.to_device(f64)]
    cut = np.array([TOL])
    outs = [np.empty(1 << 20, dtype=np.uint8) for _ in range(2)]
    infos = (api.EncInfo * 2)()
    cp = (C.c_void_p * 2)(cut.ctypes.data, cut.ctypes.data)
    dp = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    sz = (C.c_size_t * 2)(*[o.size for o in outs])
    try:
        for fn, ptrs in ((L.wr_encode_host_seg_batch, [f64.ctypes.data] * 2), (L.wr_encode_host_seg_batch_f32, [f32.ctypes.data] * 2),
                         (L.wr_encode_device_seg_batch, [b.ptr for b in dbufs])):
            fp = (C.c_void_p * 2)(*ptrs)
            half = (C.c_void_p * 2)(ptrs[0], None)
            call = lambda flds, sg, b, cuts, m=1: fn(h, 2, flds, nx, ny, nz, 1, m, 1, 1, cuts, sg, b, infos, dp, sz, None)
            assert refused(call(fp, 17, 16, cp), -1, BAD_SEG)
            assert refused(call(fp, SEG, 17, cp), -1, BAD_BRICK)
            assert refused(call(fp, 17, 17, cp), -1, BAD_SEG)
            assert refused(call(fp, 17, 16, None), -1, BAD_SEG)        # a bad seg and a null array
            assert refused(call(fp, SEG, 17, None), -1, BAD_BRICK)
            assert refused(call(fp, SEG, 16, None), -1, "null array")
            assert refused(call(half, 17, 16, cp), -1, BAD_SEG)        # a bad seg and a null field
            assert refused(call(half, SEG, 16, cp), -1, "field 1: null field pointer")
            assert refused(call(None, 17, 16, cp), -1, "null array")   # the array of fields is looked at first
            assert refused(call(fp, SEG, 16, cp, m=0), -1, "bad local cutoff description")
            assert refused(call(fp, SEG, 16, (C.c_void_p * 2)(cut.ctypes.data, None)), -1, "field 1: bad local cutoff description")
    finally:
        for b in dbufs:
            b.free()


def test_refusals_of_the_stage_calls(ctx):
    s = coded(ctx, "general", "f64")
    n, shape = s["n"], s["shape"]
    nz, ny, nx = shape
    L, h = api.lib(), ctx.h
    plane = planes_of(ctx, s["f"])[0]
    blob1, blob3 = split_planes(s["encs"]["wrs1"])[0], split_planes(s["encs"]["wrs3"])[0]
    nseg = -(-n // SEG)
    bound = max(api.seg_bound(n, SEG), api.seg_bound_strands(n, SEG, 8))
    d_sym, d_blob, d_blob2 = ctx.to_device(plane), ctx.alloc(bound + 16), ctx.alloc(bound + 16)
    got = C.c_size_t(0)
    g = C.byref(got)
    try:
        one = lambda sym, sg, blob, cap, ln: L.wr_dev_seg_encode(h, sym, n, sg, blob, cap, ln)
        strands = lambda sym, sg, blob, cap, ln, k=8: L.wr_dev_seg_encode_strands(h, sym, n, sg, k, blob, cap, ln)
        for call, head, blob, word in ((one, HEAD["wrs1"], blob1, "segment"), (strands, HEAD["wrs3"], blob3, "record")):
            assert refused(call(d_sym.ptr, 17, d_blob.ptr, bound, g), -1, BAD_SEG)
            assert refused(call(None, 17, None, 0, None), -1, BAD_SEG)            # a bad seg and null pointers
            assert refused(call(None, SEG, d_blob.ptr, bound, g), -1, "null pointer")
            assert refused(call(d_sym.ptr, SEG, None, bound, g), -1, "null pointer")
            assert refused(call(d_sym.ptr, SEG, d_blob.ptr, bound, None), -1, "null pointer")
            assert refused(call(d_sym.ptr + 8, SEG, d_blob.ptr, bound, g), -1, "plane and blob buffers must be 16-byte aligned")
            assert refused(call(d_sym.ptr, SEG, d_blob.ptr + 8, bound, g), -1, "plane and blob buffers must be 16-byte aligned")
            assert refused(call(d_sym.ptr, SEG, d_blob.ptr, head + 4 * nseg - 1, g), -5, "the blob buffer does not hold the plane's index")
            assert refused(call(d_sym.ptr, SEG, d_blob.ptr, blob.size - 1, g), -5, "the blob buffer is too small for the plane")
            assert refused(call(d_sym.ptr, SEG, d_blob.ptr, blob.size, g), 0, "") and got.value == blob.size
            assert d_blob.download(np.uint8, blob.size).tobytes() == blob.tobytes()
        assert refused(strands(d_sym.ptr, SEG, d_blob.ptr, bound, g, k=3), -1, BAD_STRANDS)
        assert refused(strands(d_sym.ptr, 17, d_blob.ptr, bound, g, k=3), -1, BAD_SEG)
        assert refused(strands(None, SEG, None, 0, None, k=3), -1, BAD_STRANDS)
        # ---- the batched stage call
        syms = (C.c_void_p * 2)(d_sym.ptr, d_sym.ptr)
        blobs = (C.c_void_p * 2)(d_blob.ptr, d_blob2.ptr)
        lens = (C.c_size_t * 2)()
        caps = lambda a, b: (C.c_size_t * 2)(a, b)
        batch = lambda sy, sg, bl, cap, ln, nj=2: L.wr_dev_seg_encode_batch(h, nj, sy, n, sg, bl, cap, ln)
        assert refused(batch(syms, 17, blobs, caps(bound, bound), lens), -1, BAD_SEG)
        assert refused(batch(None, 17, None, None, None), -1, BAD_SEG)
        assert refused(batch(syms, 17, blobs, caps(bound, bound), lens, nj=0), -1, BAD_SEG)  # seg before the job count
        assert refused(batch(syms, SEG, blobs, caps(bound, bound), lens, nj=0), -1, "njobs must be in 1..1024")
        assert refused(batch(None, SEG, blobs, caps(bound, bound), lens), -1, "null array")
        assert refused(batch((C.c_void_p * 2)(d_sym.ptr, None), SEG, blobs, caps(bound, bound), lens), -1, "job 1: null pointer")
        assert refused(batch((C.c_void_p * 2)(d_sym.ptr, d_sym.ptr + 8), SEG, blobs, caps(bound, bound), lens), -1,
                       "job 1: plane and blob buffers must be 16-byte aligned")
        assert refused(batch(syms, SEG, blobs, caps(bound, HEAD["wrs1"] + 4 * nseg - 1), lens), -5, "job 1: the blob buffer does not hold the plane's index")
        assert refused(batch(syms, SEG, blobs, caps(bound, blob1.size - 1), lens), -5, "job 1: the blob buffer is too small for the plane")
        assert lens[0] == blob1.size  # (the job that fits has its length)
        assert refused(batch(syms, SEG, blobs, caps(blob1.size, blob1.size), lens), 0, "") and list(lens) == [blob1.size] * 2
        assert d_blob2.download(np.uint8, blob1.size).tobytes() == blob1.tobytes()
        # ---- the two probes and the reorder call
        bnd = C.c_size_t(0)
        assert refused(L.wr_dev_plane_size_bound(h, d_sym.ptr, n, 17, C.byref(bnd)), -1, BAD_SEG)
        assert refused(L.wr_dev_plane_size_bound(h, None, n, 17, None), -1, BAD_SEG)
        assert refused(L.wr_dev_plane_size_bound(h, None, n, SEG, C.byref(bnd)), -1, "null pointer")
        assert refused(L.wr_dev_plane_size_bound(h, d_sym.ptr + 8, n, SEG, C.byref(bnd)), -1, "the plane must be 16-byte aligned")
        assert refused(L.wr_dev_plane_size_bound(h, d_sym.ptr, n, SEG, C.byref(bnd)), 0, "") and bnd.value >= blob1.size
        deps = (C.c_double * 1)(1.0)
        bounds = (C.c_size_t * 1)()
        d_res = ctx.to_device(np.linspace(0.0, 200.0, n))
        try:
            probe = lambda res, nc, dv, sg, out: L.wr_dev_quant_size_probe(h, res, n, 0.0, nc, dv, sg, out)
            assert refused(probe(d_res.ptr, 1, deps, 17, bounds), -1, BAD_SEG)
            assert refused(probe(None, 0, None, 17, None), -1, BAD_SEG)       # seg before the candidate count and the pointers
            assert refused(probe(None, 0, None, SEG, None), -1, "a size probe takes 1 to 8 candidate steps")
            assert refused(probe(None, 1, deps, SEG, bounds), -1, "null pointer")
            assert refused(probe(d_res.ptr + 8, 1, deps, SEG, bounds), -1, "the residual array must be 16-byte aligned")
            assert refused(probe(d_res.ptr, 1, deps, SEG, bounds), 0, "") and bounds[0] > 0
        finally:
            d_res.free()
        reorder = lambda dst, src, wlev, brick: L.wr_dev_plane_reorder(h, dst, src, nx, ny, nz, wlev, brick, 0)
        assert refused(reorder(d_blob.ptr, d_sym.ptr, 4, 17), -1, BAD_BRICK)
        assert refused(reorder(None, None, 3, 17), -1, BAD_BRICK)             # brick before wlev and the pointers
        assert refused(reorder(None, None, 3, 16), -1, "wlev must be 0 or 4")
        assert refused(reorder(None, d_sym.ptr, 4, 16), -1, "null pointer, or source and destination are the same")
        assert refused(reorder(d_blob.ptr, d_sym.ptr + 8, 4, 16), -1, "plane buffers must be 16-byte aligned")
        assert refused(reorder(d_blob.ptr, d_sym.ptr, 4, 16), 0, "")
        assert np.array_equal(d_blob.download(np.uint8, n), plane[api.blocked_order(shape, 4, 16)])
    finally:
        for d in (d_sym, d_blob, d_blob2):
            d.free()


@pytest.mark.parametrize("name", list(SHAPES))
def test_overflow(ctx, name):
    """cap one byte short of the stream: the single call, the batch (with the field in front), the transcode into a segmented
    format and into the reference's"""
    s = coded(ctx, name, "f64")
    shape, f = s["shape"], s["f"]
    for fmt, kw in FORMATS.items():
        want = s["encs"][fmt]
        total = want["ntot_enc"]
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg(f, TOL, 1, SEG, out=np.empty(total - 1, dtype=np.uint8), **kw)
        assert str(e.value) == ERR % (-5, TOO_LARGE), fmt
        assert same_stream(own(ctx.encode_host_seg(f, TOL, 1, SEG, out=np.empty(total, dtype=np.uint8), **kw)), want), fmt
        with pytest.raises(api.WaveRangeError) as e:
            ctx.transcode(s["ref"], s["ref"]["data"], TARGET[fmt], shape=shape, cap=total - 1)
        assert str(e.value) == ERR % (-5, TOO_LARGE), fmt
        data, info = ctx.transcode(s["ref"], s["ref"]["data"], TARGET[fmt], shape=shape, cap=total)
        assert same_stream(info, want), fmt
        if fmt != "wrs3":
            with pytest.raises(api.WaveRangeError) as e:
                ctx.encode_host_seg_batch([f, f], TOL, 1, SEG, caps=[total, total - 1], **kw)
            assert str(e.value) == ERR % (-5, "field 1: " + TOO_LARGE), fmt
            encs, _ = ctx.encode_host_seg_batch([f, f], TOL, 1, SEG, caps=[total, total], **kw)
            assert same_stream(encs[0], want) and same_stream(encs[1], want), fmt
    total = s["ref"]["ntot_enc"]
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host(f, TOL, out=np.empty(total - 1, dtype=np.uint8))
    assert str(e.value) == ERR % (-5, TOO_LARGE)
    enc = s["encs"]["wrs1"]
    with pytest.raises(api.WaveRangeError) as e:
        ctx.transcode(enc, enc["data"], "ref", shape=shape, cap=total - 1)
    assert str(e.value) == ERR % (-5, TOO_LARGE)
