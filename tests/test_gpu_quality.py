"""Encode to an RMS or PSNR target on the GPU (include/waverange_amd.h), whole calls, against S* and R* computed on the CPU
(tests/rms_ref.py) for the inputs tests/rms_cases.py holds and tests/test_rms_cpu.py has held the reference -- contract and guard
condition -- against.  Every call: the verdict of the reference on the chosen g, the RMS error reported within 2^-36 of R*, the
stream and header of the plain call at t(g), every plane coded once, and the measuring half returning the same bits.  Then what
needs no reference: with the search confined to [g, GMAX] a target equal to the RMS reached returns the same g, and the double
below it is refused."""
import math

import numpy as np
import pytest

import bounded_cases as bc
import rms_cases as rc
from rms_ref import ACCURACY, GMAX
from util import bits_equal
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def quality_call(ctx, f, form, norm, target, seg, wtflag, kw, tol_min=2.0 ** -60):
    if form == "device":
        buf = ctx.to_device(f)
        try:
            return ctx.encode_seg_quality(buf, f.shape, norm, target, tol_min=tol_min, seg=seg, wtflag=wtflag, **kw)
        finally:
            buf.free()
    enc = ctx.encode_host_seg_quality_f32 if f.dtype == np.float32 else ctx.encode_host_seg_quality
    return enc(f, norm, target, tol_min=tol_min, seg=seg, wtflag=wtflag, **kw)


def check_call(ctx, f, ref, form, norm, target, m, seg, wtflag, kw, g_min=0):
    before = api.stat(api.STAT_QUALITY_CODER_RUNS), api.stat(api.STAT_BOUNDED_CODER_RUNS)
    info, data, res = quality_call(ctx, f, form, norm, target, seg, wtflag, kw, tol_min=api.budget_tol(g_min))
    grew = api.stat(api.STAT_QUALITY_CODER_RUNS) - before[0]
    g = res["g"]
    what = (f.shape, f.dtype.name, form, kw, norm, target, res)
    print("%s %s %s norm %d target %r: g %d (start %d), rms %r, R* %r, max_rms %r, trials %d" %
          (f.shape, form, kw, norm, target, g, ref.start(m), res["rms"], ref.R(g), res["max_rms"], res["trials"]))
    assert res["max_rms"] == m and res["tolrel"] == api.budget_tol(g), (what, m)
    assert ref.verdict(g, res["max_rms"], g_min) is None, (what, ref.verdict(g, res["max_rms"], g_min))
    assert res["rms"] <= res["max_rms"], what
    assert abs(res["rms"] - ref.R(g)) <= ACCURACY * ref.R(g), (what, ref.R(g))
    assert abs(res["sumsq"] - ref.S(g)) <= ACCURACY * ref.S(g), (what, ref.S(g))
    assert res["rms"] == math.sqrt(res["sumsq"] / f.size), what
    assert res["max_abs"] == ref.E(g), (what, ref.E(g))
    assert res["range"] == ref.range and abs(res["psnr"] - 20.0 * math.log10(res["range"] / res["rms"])) <= 1e-12 * abs(res["psnr"]), what
    assert res["trials"] >= 1 and grew == info["nlay"] == ref.nlay(g), (what, grew, info["nlay"])
    assert api.stat(api.STAT_BOUNDED_CODER_RUNS) == before[1], what
    # the same stream as the plain call of the format at t(g)
    plain_enc = ctx.encode_host_seg_f32 if f.dtype == np.float32 else ctx.encode_host_seg
    plain, _ = plain_enc(f, api.budget_tol(g), wtflag=wtflag, seg=seg, **kw)
    for k in HEADER_KEYS:
        assert info[k] == plain[k], (what, k)
    assert list(info["len_enc_vec"]) == list(plain["len_enc_vec"]), what
    assert bits_equal(info["deps_vec"], plain["deps_vec"]) and bits_equal(info["minval_vec"], plain["minval_vec"]), what
    assert data.size == info["ntot_enc"] and np.array_equal(data, plain["data"]), what
    # the measuring half on the result: the same bits
    st = (ctx.seg_error_stats_host_f32 if f.dtype == np.float32 else ctx.seg_error_stats_host)(np.ascontiguousarray(f), info)
    assert bits_equal(np.float64(st["rms"]), np.float64(res["rms"])) and bits_equal(np.float64(st["max_abs"]), np.float64(res["max_abs"])), (what, st)
    assert st["sumsq"] == res["sumsq"] and st["nonfinite"] == 0 and st["psnr"] == res["psnr"], (what, st)
    assert st["lo"] == ref.b.flo and st["hi"] == ref.b.fhi, (what, st)
    return res


@pytest.mark.parametrize("call", rc.CALLS, ids=[c[0] for c in rc.CALLS])
def test_quality_call_against_the_reference(ctx, call):
    _, kind, dims, seg, wtflag, f32, kw, form = call
    f, ref = rc.ref_of(kind, dims, seg, wtflag, f32)
    for name, norm, target, m in rc.targets_of(kind, dims, seg, wtflag, f32):
        res = check_call(ctx, f, ref, form, norm, target, m, seg, wtflag, kw)
        if name == "above max|f|":
            assert res["g"] >= GMAX - 64, (name, res)


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("dims,seg", bc.DRIVER_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_quality_call_is_consistent_with_itself(ctx, dims, seg, kind):
    """Needs no reference.  The RMS error a call reached, given as the target, returns the same g: equality holds.  The double
    below it cannot be held at that g.

    Both second calls are made with tol_min = t(g).  R is not monotone and the contract is local, so a second call that may
    start elsewhere can end on ANOTHER grid point that meets the contract: on the smooth (64,64,64) field the target 1e-3 max|f|
    gives g = 3385 with R = 0.0050586, and the free call with that R as its target gives g = 3341 (R(3342) exceeds it, and so
    does R(3386): both answers are tight).  With the search confined to [g, GMAX] the outcome follows from the contract alone:
    at the target R(g) the walk starts on g, finds it holding only if equality counts, steps to g + 1, which the first call
    formed and found above its own, larger target, and ends on g; one double lower g itself misses the target, which is
    WR_ERR_BOUND naming R(g).  The free call with the lower target must then settle on another point, with a smaller error."""
    f, ref = rc.ref_of(kind, dims, seg)
    for tol in (1e-3, 1e-7):
        _, _, res = ctx.encode_host_seg_quality(f, api.NORM_RMS, tol * ref.absmax, seg=seg)
        if res["g"] == GMAX:
            continue
        pinned = api.budget_tol(res["g"])
        _, _, at = ctx.encode_host_seg_quality(f, api.NORM_RMS, res["rms"], tol_min=pinned, seg=seg)
        print(dims, kind, tol, "g", res["g"], "rms", res["rms"], "again", at["g"], at["trials"])
        assert at["g"] == res["g"] and at["rms"] == res["rms"] == at["max_rms"], (res, at)
        lower = float(np.nextafter(res["rms"], 0.0))
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality(f, api.NORM_RMS, lower, tol_min=pinned, seg=seg)
        assert "error %d:" % api.ERR_BOUND in str(e.value) and ("= %.17g" % res["rms"]) in str(e.value), str(e.value)
        _, _, below = ctx.encode_host_seg_quality(f, api.NORM_RMS, lower, seg=seg)
        print(dims, kind, tol, "one double lower: g", below["g"], "rms", below["rms"])
        assert below["g"] != res["g"] and below["rms"] < res["rms"], (res, below)


def test_quality_call_is_deterministic(ctx):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = rc.ref_of("noise", dims, seg)
    runs = [ctx.encode_host_seg_quality(f, api.NORM_PSNR, 60.0, seg=seg) for _ in range(3)]
    for info, data, res in runs[1:]:
        assert all(bits_equal(np.float64(res[k]), np.float64(runs[0][2][k])) for k in ("rms", "sumsq", "max_abs", "psnr", "max_rms"))
        assert (res["g"], res["trials"]) == (runs[0][2]["g"], runs[0][2]["trials"]) and np.array_equal(data, runs[0][1])


@pytest.mark.parametrize("kw", [dict(), dict(brick=32), dict(strands=8)], ids=["wrs1", "wrs2", "wrs3"])
def test_norm_max_is_the_bounded_call(ctx, kw):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = rc.ref_of("smooth", dims, seg)
    m = 1e-5 * ref.absmax
    b_info, b_data, b_res = ctx.encode_host_seg_bounded(f, m, seg=seg, **kw)
    before = api.stat(api.STAT_QUALITY_CODER_RUNS)
    info, data, res = ctx.encode_host_seg_quality(f, api.NORM_MAX, m, seg=seg, **kw)
    assert api.stat(api.STAT_QUALITY_CODER_RUNS) - before == info["nlay"]
    assert (res["g"], res["tolrel"], res["max_abs"], res["trials"]) == (b_res["g"], b_res["tolrel"], b_res["err"], b_res["trials"])
    assert all(info[k] == b_info[k] for k in HEADER_KEYS) and list(info["len_enc_vec"]) == list(b_info["len_enc_vec"])
    assert np.array_equal(data, b_data)
    assert res["range"] == ref.range and all(math.isnan(res[k]) for k in ("rms", "sumsq", "psnr", "max_rms"))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_target_below_what_tol_min_reaches(ctx):
    dims, seg = bc.DRIVER_CASES[2]
    f, ref = rc.ref_of("smooth", dims, seg)
    g_min = api.budget_index(1e-2)
    m = 1e-7 * ref.absmax
    assert ref.R(g_min) > m
    out = np.full(ctx._seg_cap(f.shape, seg), 0xAB, np.uint8)
    before = api.stat(api.STAT_QUALITY_CODER_RUNS)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality(f, api.NORM_RMS, m, tol_min=api.budget_tol(g_min), seg=seg, out=out)
    assert "error %d:" % api.ERR_BOUND in str(e.value) and "R(g_min = %d)" % g_min in str(e.value), str(e.value)
    named = float(str(e.value).rsplit("= ", 1)[1])
    assert abs(named - ref.R(g_min)) <= ACCURACY * ref.R(g_min), (named, ref.R(g_min))
    assert np.all(out == 0xAB) and api.stat(api.STAT_QUALITY_CODER_RUNS) == before
    # the target the message names is met, at g_min or coarser
    _, _, res = ctx.encode_host_seg_quality(f, api.NORM_RMS, named, tol_min=api.budget_tol(g_min), seg=seg)
    assert res["g"] >= g_min and res["rms"] <= named


def test_constant_field(ctx):
    f = np.full((8, 8, 16), 2.5)
    info, data, res = ctx.encode_host_seg_quality(f, api.NORM_RMS, 1e-3, tol_min=1e-9, seg=1024)
    assert info["nlay"] == 0 and info["ntot_enc"] == 0 and data.size == 0
    assert res["g"] == GMAX and res["rms"] == 0.0 and res["sumsq"] == 0.0 and res["max_abs"] == 0.0 and res["trials"] == 0
    assert res["psnr"] == np.inf and res["range"] == 0.0 and res["tolrel"] == 1.0
    st = ctx.seg_error_stats_host(f, info)
    assert st["rms"] == 0.0 and st["max_abs"] == 0.0 and st["psnr"] == np.inf and st["lo"] == st["hi"] == 2.5
    with pytest.raises(api.WaveRangeError) as e:  # a PSNR over an empty range
        ctx.encode_host_seg_quality(f, api.NORM_PSNR, 60.0, tol_min=1e-9, seg=1024)
    assert "error -1:" in str(e.value) and "range" in str(e.value), str(e.value)


@pytest.mark.parametrize("norm,target", [(api.NORM_RMS, 1e-3), (api.NORM_PSNR, 60.0)])
def test_a_nan_in_the_field_is_refused(ctx, norm, target):
    f = bc.make_field("smooth", (16, 16, 16)).copy()
    f[1, 2, 3] = np.nan
    out = np.full(ctx._seg_cap(f.shape, 1024), 0xAB, np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality(f, norm, target, seg=1024, out=out)
    assert "error -1:" in str(e.value) and "1 sample(s)" in str(e.value), str(e.value)
    assert np.all(out == 0xAB)
    # the measuring half fills its record and says so
    g = bc.make_field("smooth", (16, 16, 16))
    enc, _ = ctx.encode_host_seg(g, 1e-5)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_error_stats_host(f, enc)
    assert "error -1:" in str(e.value) and "1 difference" in str(e.value), str(e.value)
    st = ctx.seg_error_stats_host(f, enc, allow_nonfinite=True)
    clean = ctx.seg_error_stats_host(g, enc)
    assert st["nonfinite"] == 1 and 0 < st["sumsq"] <= clean["sumsq"] and st["max_abs"] <= clean["max_abs"] and clean["nonfinite"] == 0


def test_refusals(ctx):
    f = synth.field(16, 16, 16, seed=1)
    for m in ((2, 1, 1), (1, 2, 2)):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality(f, api.NORM_RMS, 1e-3, seg=1024, m=m)
        assert "error -3:" in str(e.value) and "local cutoff" in str(e.value), str(e.value)
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality(f, api.NORM_RMS, 1e-3, seg=1024)
        assert "error -3:" in str(e.value) and "residual" in str(e.value), str(e.value)
    finally:
        ctx.set_keep_residual(False)
    for norm in (0, 4, -1):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality(f, norm, 1e-3, seg=1024)
        assert "error -1:" in str(e.value) and "norm" in str(e.value), str(e.value)
    for norm in (api.NORM_MAX, api.NORM_RMS, api.NORM_PSNR):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(api.WaveRangeError) as e:
                ctx.encode_host_seg_quality(f, norm, bad, seg=1024)
            assert "error -1:" in str(e.value), str(e.value)
            with pytest.raises(api.WaveRangeError) as e:
                ctx.encode_host_seg_quality(f, norm, 1.0, tol_min=bad, seg=1024)
            assert "error -1:" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError):
        ctx.encode_host_seg_quality(f, api.NORM_RMS, 1e-3, seg=17)
