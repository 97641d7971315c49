"""Encode to a pointwise error bound on the GPU (include/waverange_amd.h): the trial kernel against the oracle's quantizer and
dequantizer, bit for bit; the measuring half (seg_error_host) against a decode; and the driver against E(g) computed on the CPU
(tests/bounded_ref.py) -- every bound and every verdict comes from there, for the inputs tests/bounded_cases.py holds and
tests/test_bounded_cpu.py has held the reference itself against.  No tolerance appears anywhere: errors are equal doubles,
streams equal bytes, reconstructions equal bits."""
import numpy as np
import pytest

import bounded_cases as bc
from bounded_ref import BoundedRef
from util import bits_equal
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

GMAX = api.BUDGET_GMAX
HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")
# the trial kernel, as flat arrays: odd and smaller than one tile; 16^3; whole tiles plus a tail; an odd count (half a pair at
# the end); a power of two (whole tiles only)
KERNEL_SHAPES = [(13, 9, 7), (16, 16, 16), (40, 36, 33), (39, 37, 33), (64, 64, 32)]
FORMATS = [("wrs1", dict()), ("wrs2", dict(brick=32)), ("wrs3", dict(strands=8))]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
_DEEP = {}


def deep_planes(kind, dims):
    """(coefficients, [(deps, minval)] of the planes of a tol-1e-16 encode -- all eight -- and the oracle's sum after 1, 3 and 8)"""
    key = (kind, dims)
    if key not in _DEEP:
        o = Oracle()
        f = bc.make_field(kind, dims)
        ref = BoundedRef(o, f, 1024)  # (the quantizer loop restated: the oracle's own encode has no room for eight planes of 819 symbols)
        coef = ref.resid[0]
        planes = ref.planes(api.budget_index(1e-16))
        assert len(planes) == 8
        steps = [(float(deps), float(lo)) for _, deps, lo in planes]
        want, acc = {}, np.zeros(coef.size)
        for l, (q, deps, lo) in enumerate(planes):
            assert np.array_equal(q, o.quantize_plane(ref.resid[l], deps, lo)[0])
            acc = o.dequant_accum(acc, q, deps, lo)
            if l + 1 in (1, 3, 8):
                want[l + 1] = acc.copy()
        _DEEP[key] = (coef, steps, want)
    return _DEEP[key]


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("dims", KERNEL_SHAPES, ids=case_id)
def test_requant_accum_equals_the_oracles_planes_summed(ctx, dims, kind):
    coef, steps, want = deep_planes(kind, dims)
    for nlay in (1, 3, 8):
        d = [s[0] for s in steps[:nlay]]
        m = [s[1] for s in steps[:nlay]]
        assert bits_equal(ctx.requant_accum(coef, d, m), want[nlay]), (dims, kind, nlay)
        # the coefficient array 8 bytes off its alignment: the element-wise form, the same bits
        assert bits_equal(ctx.requant_accum(coef, d, m, offset=8), want[nlay]), (dims, kind, nlay, "unaligned")


def test_requant_accum_refuses_zero_and_nine_planes(ctx):
    coef, steps, _ = deep_planes("smooth", (16, 16, 16))
    for nlay in (0, 9):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.requant_accum(coef, [steps[l % 8][0] for l in range(nlay)], [steps[l % 8][1] for l in range(nlay)])
        assert "error -1:" in str(e.value), str(e.value)  # WR_ERR_ARG


# ---- the measuring half --------------------------------------------------------------------------------------------------------
# fused both ways; general; forward fused and inverse general (tests/fused_cases.py)
@pytest.mark.parametrize("dims", [(16, 16, 16), (40, 36, 33), (258, 130, 66)], ids=case_id)
@pytest.mark.parametrize("fmt,kw", FORMATS, ids=[f[0] for f in FORMATS])
def test_seg_error_host_equals_the_error_of_a_decode(ctx, dims, fmt, kw):
    f = bc.make_field("smooth", dims)
    enc, _ = ctx.encode_host_seg(f, 1e-5, seg=1024, **kw)
    rec = np.empty_like(f)
    ctx.decode_host_seg(rec, enc)
    assert ctx.seg_error_host(f, enc) == float(np.abs(f - rec).max())
    f32 = f.astype(np.float32)
    enc32, _ = ctx.encode_host_seg_f32(f32, 1e-5, seg=1024, **kw)
    rec32 = np.empty_like(f32)
    ctx.decode_host_seg_f32(rec32, enc32)
    assert ctx.seg_error_host_f32(f32, enc32) == float(np.abs(f32.astype(np.float64) - rec32.astype(np.float64)).max())


def test_seg_error_host_of_a_constant_field_and_of_a_nan(ctx):
    f = np.full((8, 8, 16), 2.5)
    enc, _ = ctx.encode_host_seg(f, 1e-5, seg=1024)
    assert enc["nlay"] == 0 and ctx.seg_error_host(f, enc) == 0.0
    g = bc.make_field("smooth", (16, 16, 16))
    enc, _ = ctx.encode_host_seg(g, 1e-5)
    bad = g.copy()
    bad[3, 4, 5] = np.nan
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_error_host(bad, enc)
    assert "error -1:" in str(e.value) and "1 difference" in str(e.value), str(e.value)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def check_call(ctx, f, ref, seg, m, g_min=0, wtflag=1, encode=None, formats=FORMATS):
    """One bounded call per format checked against the Python E: it holds, it is tight, err is E(g), the same stream as the plain
    call at the chosen tolerance, the oracle's reconstruction, every plane coded once.  Returns the result record of the first."""
    first = None
    for fmt, kw in formats:
        before = api.stat(api.STAT_BOUNDED_CODER_RUNS)
        if encode is None:
            info, data, res = ctx.encode_host_seg_bounded(f, m, tol_min=api.budget_tol(g_min), seg=seg, wtflag=wtflag, **kw)
        else:
            info, data, res = encode(f, m, api.budget_tol(g_min), seg, kw)
        grew = api.stat(api.STAT_BOUNDED_CODER_RUNS) - before
        g = res["g"]
        what = (f.shape, fmt, seg, m, g_min, res)
        assert g_min <= g <= GMAX and res["tolrel"] == api.budget_tol(g), what
        assert ref.verdict(g, m, g_min) is None, (what, ref.verdict(g, m, g_min))
        assert ref.E(g) <= m and (g == GMAX or ref.E(g + 1) > m), what
        assert res["err"] == ref.E(g), (what, ref.E(g))
        assert res["trials"] >= 1 and grew == info["nlay"] == ref.nlay(g), (what, grew, info["nlay"])
        if first is None:
            first = res
        else:  # the search does not depend on the format
            assert (res["g"], res["err"], res["trials"]) == (first["g"], first["err"], first["trials"]), what
        # the same stream as the plain call of the format
        plain_kw = dict(kw)
        plain_enc = ctx.encode_host_seg_f32 if f.dtype == np.float32 else ctx.encode_host_seg
        plain, _ = plain_enc(f, api.budget_tol(g), wtflag=wtflag, seg=seg, **plain_kw)
        for k in HEADER_KEYS:
            assert info[k] == plain[k], (what, k)
        assert list(info["len_enc_vec"]) == list(plain["len_enc_vec"]), what
        assert bits_equal(info["deps_vec"], plain["deps_vec"]) and bits_equal(info["minval_vec"], plain["minval_vec"]), what
        assert data.size == info["ntot_enc"] and np.array_equal(data, plain["data"]), what
        # the oracle's reconstruction, and the measuring half agrees
        rec = np.empty(f.shape, dtype=f.dtype)
        (ctx.decode_host_seg_f32 if f.dtype == np.float32 else ctx.decode_host_seg)(rec, info)
        assert bits_equal(rec, ref.recon(g)), what
        assert (ctx.seg_error_host_f32 if f.dtype == np.float32 else ctx.seg_error_host)(np.ascontiguousarray(f), info) == ref.E(g), what
    return first


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("dims,seg", bc.DRIVER_CASES, ids=case_id)
def test_driver_at_bounds_from_the_python_E(ctx, dims, seg, kind):
    f, ref = bc.ref_of(kind, dims, seg)
    for name, m in bc.bounds_of(ref):
        res = check_call(ctx, f, ref, seg, m)
        if name == "above max|f|":
            assert res["g"] >= GMAX - 64, (name, res)
    # equality counts as holding: G_EXACT itself is allowed for E(G_EXACT), and refused for the double below it
    e = ref.E(bc.G_EXACT)
    _, _, at_e = ctx.encode_host_seg_bounded(f, e, tol_min=api.budget_tol(bc.G_EXACT), seg=seg)
    assert at_e["g"] >= bc.G_EXACT and at_e["err"] <= e
    if ref.E(bc.G_EXACT + 1) > e:
        assert at_e["g"] == bc.G_EXACT and at_e["err"] == e


@pytest.mark.parametrize("kind", bc.KINDS)
def test_driver_without_the_transform(ctx, kind):
    dims, seg = bc.WT0_CASE
    f, ref = bc.ref_of(kind, dims, seg, wtflag=0)
    for name, m in bc.bounds_of(ref):
        check_call(ctx, f, ref, seg, m, wtflag=0, formats=FORMATS[:1])


def test_driver_respects_tol_min(ctx):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = bc.ref_of("smooth", dims, seg)
    m = 1e-7 * ref.absmax
    free = ref.solve(m)
    for g_min in (free - 5, free, 0):
        res = check_call(ctx, f, ref, seg, m, g_min=g_min, formats=FORMATS[:1])
        assert res["g"] >= g_min


def test_driver_fp32_field(ctx):
    f, ref = bc.ref_of("smooth", (64, 64, 64), 0, f32=True)

    def enc(fld, m, tol_min, seg, kw):
        return ctx.encode_host_seg_bounded_f32(fld, m, tol_min=tol_min, seg=seg, **kw)

    for name, m in bc.bounds_of(ref):
        check_call(ctx, f, ref, 0, m, encode=enc)


@pytest.mark.parametrize("dims,seg", [bc.DRIVER_CASES[0], bc.DRIVER_CASES[2]], ids=case_id)
def test_driver_device_field(ctx, dims, seg):
    f, ref = bc.ref_of("noise", dims, seg)

    def on_device(fld, m, tol_min, s, kw):
        buf = ctx.to_device(fld)
        try:
            return ctx.encode_seg_bounded(buf, fld.shape, m, tol_min=tol_min, seg=s, **kw)
        finally:
            buf.free()

    for name, m in bc.bounds_of(ref)[:3]:
        check_call(ctx, f, ref, seg, m, encode=on_device)


def test_driver_is_deterministic(ctx):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = bc.ref_of("noise", dims, seg)
    m = 1e-3 * ref.absmax
    runs = [ctx.encode_host_seg_bounded(f, m, seg=seg) for _ in range(3)]
    for info, data, res in runs[1:]:
        assert (res["g"], res["err"], res["trials"]) == (runs[0][2]["g"], runs[0][2]["err"], runs[0][2]["trials"])
        assert np.array_equal(data, runs[0][1]) and all(info[k] == runs[0][0][k] for k in HEADER_KEYS)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_driver_bound_below_what_tol_min_reaches(ctx):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = bc.ref_of("smooth", dims, seg)
    g_min = api.budget_index(1e-2)
    m = 1e-7 * ref.absmax
    assert ref.E(g_min) > m
    out = np.full(ctx._seg_cap(f.shape, seg), 0xAB, np.uint8)
    before = api.stat(api.STAT_BOUNDED_CODER_RUNS)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_bounded(f, m, tol_min=api.budget_tol(g_min), seg=seg, out=out)
    assert "error %d:" % api.ERR_BOUND in str(e.value) and ("%.17g" % ref.E(g_min)) in str(e.value), (str(e.value), ref.E(g_min))
    assert np.all(out == 0xAB) and api.stat(api.STAT_BOUNDED_CODER_RUNS) == before
    # the bound the message names does
    res = check_call(ctx, f, ref, seg, ref.E(g_min), g_min=g_min, formats=FORMATS[:1])
    assert res["g"] >= g_min


def test_driver_constant_field(ctx):
    f = np.full((8, 8, 16), 2.5)
    info, data, res = ctx.encode_host_seg_bounded(f, 1e-3, tol_min=1e-9, seg=1024)
    assert info["nlay"] == 0 and info["ntot_enc"] == 0 and data.size == 0
    assert res["g"] == GMAX and res["err"] == 0.0 and res["trials"] == 0 and res["tolrel"] == 1.0
    rec = np.empty_like(f)
    ctx.decode_host_seg(rec, info)
    assert bits_equal(rec, f)


@pytest.mark.parametrize("dims", [(16, 16, 16), (13, 9, 7)], ids=case_id)
def test_driver_refuses_a_nan_and_an_infinity(ctx, dims):
    f = bc.make_field("smooth", dims).copy()
    f[1, 2, 3] = np.nan
    f[2, 3, 4] = np.inf
    out = np.full(ctx._seg_cap(f.shape, 1024), 0xAB, np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_bounded(f, 1e-3, seg=1024, out=out)
    assert "error -1:" in str(e.value) and "2 sample(s)" in str(e.value), str(e.value)
    assert np.all(out == 0xAB)
    f[2, 3, 4] = 0.5  # the NaN alone: the field's range is finite, the first trial finds it
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_bounded(f, 1e-3, seg=1024, out=out)
    assert "error -1:" in str(e.value) and "1 sample(s)" in str(e.value), str(e.value)


def test_driver_refusals(ctx):
    f = synth.field(16, 16, 16, seed=1)
    for m in ((2, 1, 1), (1, 2, 2)):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_bounded(f, 1e-3, seg=1024, m=m)
        assert "error -3:" in str(e.value) and "local cutoff" in str(e.value), str(e.value)
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_bounded(f, 1e-3, seg=1024)
        assert "error -3:" in str(e.value) and "residual" in str(e.value), str(e.value)
    finally:
        ctx.set_keep_residual(False)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_bounded(f, bad, seg=1024)
        assert "error -1:" in str(e.value), str(e.value)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_bounded(f, 1e-3, tol_min=bad, seg=1024)
        assert "error -1:" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError):
        ctx.encode_host_seg_bounded(f, 1e-3, seg=17)
