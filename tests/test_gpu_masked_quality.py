"""Encode a masked field to a pointwise, RMS or PSNR target on the GPU (include/waverange_amd.h, "Masked fields in the tolerance
searches"), whole calls, against E_D, S_D* and R_D* computed on the CPU (tests/masked_quality_cases.py) for inputs that
tests/test_masked_quality_cpu.py has held the reference against.  Every call: the reference's verdict on the chosen g, the
errors over the defined samples only (rms dividing by their count), the returned pad equal to the CPU's to the bit, header and
field bytes of the plain call on the padded field at t(g), blob and mask record of the masked call at that tolerance, the masked
decode within the target on D and `fill` elsewhere, every plane coded once, the measuring half returning the same bits."""
import math

import numpy as np
import pytest

import masked_quality_cases as mq
from rms_ref import ACCURACY, GMAX
from util import bits_equal
from waverange_amd import api

pytestmark = pytest.mark.gpu

HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def masked_quality_call(ctx, f, form, norm, target, below, seg, wtflag, kw, tol_min=2.0 ** -60, out=None):
    if form == "device":
        buf = ctx.to_device(f)
        try:
            return ctx.encode_seg_quality_masked(buf, f.shape, norm, target, below, tol_min=tol_min, seg=seg, wtflag=wtflag, out=out, **kw)
        finally:
            buf.free()
    enc = ctx.encode_host_seg_quality_masked_f32 if f.dtype == np.float32 else ctx.encode_host_seg_quality_masked
    return enc(f, norm, target, below, tol_min=tol_min, seg=seg, wtflag=wtflag, out=out, **kw)


def same_header(a, b, what):
    for k in HEADER_KEYS:
        assert a[k] == b[k], (what, k)
    assert list(a["len_enc_vec"]) == list(b["len_enc_vec"]), what
    assert bits_equal(a["deps_vec"], b["deps_vec"]) and bits_equal(a["minval_vec"], b["minval_vec"]), what


def check_call(ctx, call, name, norm, target, m):
    _, kind, dims, seg, wtflag, f32, kw, form, mask, _, below = call
    _, ref = mq.ref_of(*mq.key_of(call))
    f = mq.field_of(call)
    n, nd = f.size, ref.nd
    before = api.stat(api.STAT_QUALITY_CODER_RUNS)
    info, data, res = masked_quality_call(ctx, f, form, norm, target, below, seg, wtflag, kw)
    data = data.copy()
    grew = api.stat(api.STAT_QUALITY_CODER_RUNS) - before
    g, mres = res["g"], info["mask"]
    what = (call[0], name, res, mres)
    print("%s %s: g %d, max_abs %r (E_D %r, outside D %r), rms %r (R_D* %r), trials %d" %
          (call[0], name, g, res["max_abs"], ref.E(g), ref.E_out(g), res["rms"], ref.R(g), res["trials"]))
    assert mres["undefined"] == n - nd and bits_equal(np.float64(mres["pad"]), np.float64(ref.pad)), (what, ref.pad)
    assert res["tolrel"] == api.budget_tol(g) and res["range"] == ref.range, what
    assert res["max_abs"] == ref.E(g), (what, ref.E(g), ref.E_out(g))
    if norm == api.NORM_MAX:
        assert ref.verdict_max(g, m) is None, (what, ref.verdict_max(g, m))
        assert res["max_abs"] <= target and all(math.isnan(res[k]) for k in ("rms", "sumsq", "psnr", "max_rms")), what
    else:
        assert res["max_rms"] == m, (what, m)
        assert ref.verdict(g, m) is None, (what, ref.verdict(g, m))
        assert res["rms"] <= m, what
        assert abs(res["rms"] - ref.R(g)) <= ACCURACY * ref.R(g), (what, ref.R(g))
        assert abs(res["sumsq"] - ref.S(g)) <= ACCURACY * ref.S(g), (what, ref.S(g))
        assert res["rms"] == math.sqrt(res["sumsq"] / nd), (what, nd)
        assert abs(res["psnr"] - 20.0 * math.log10(res["range"] / res["rms"])) <= 1e-12 * abs(res["psnr"]), what
    assert res["trials"] >= 1 and grew == info["nlay"] == ref.nlay(g), (what, grew, info["nlay"])
    # header and field bytes: the plain call of the padded field at t(g)
    nt = info["ntot_enc"]
    plain, _ = (ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg)(ref.f_pad, api.budget_tol(g), wtflag=wtflag, seg=seg, **kw)
    same_header(info, plain, what)
    assert data.size == nt + mres["mask_len"] and np.array_equal(data[:nt], plain["data"]), what
    # blob and mask record: the masked call at that tolerance
    rec, _ = (ctx.encode_host_seg_masked_f32 if f32 else ctx.encode_host_seg_masked)(f, api.budget_tol(g), below, wtflag=wtflag, seg=seg, **kw)
    same_header(info, rec, what)
    assert np.array_equal(data, rec["data"]), what
    assert all(mres[k] == rec["mask"][k] for k in ("undefined", "mask_len")) and bits_equal(np.float64(mres["pad"]), np.float64(rec["mask"]["pad"])), what
    assert np.array_equal(data[nt:], api.mask_blob_host_ref(ref.und.reshape(-1), seg, ref.pad)), what
    # the masked decode: within the target on D, `fill` elsewhere
    out = np.full(f.shape, 4242.0, f.dtype)
    (ctx.decode_host_seg_masked_f32 if f32 else ctx.decode_host_seg_masked)(out, dict(info, data=data), -77.25)
    assert np.all(out[ref.und] == -77.25), what
    d = f[~ref.und].astype(np.float64) - out[~ref.und].astype(np.float64)
    assert float(np.abs(d).max()) == res["max_abs"], what
    if norm == api.NORM_MAX:
        assert float(np.abs(d).max()) <= target, what
    else:
        assert math.sqrt(math.fsum(d * d) / nd) <= m * (1 + ACCURACY), what
    # the measuring half, on the caller's field with its NaNs and undef values: the same bits
    st = (ctx.seg_error_stats_host_masked_f32 if f32 else ctx.seg_error_stats_host_masked)(f, dict(info, data=data))
    assert st["defined"] == nd and st["nonfinite"] == 0 and bits_equal(np.float64(st["max_abs"]), np.float64(res["max_abs"])), (what, st)
    assert st["lo"] == ref.b.flo and st["hi"] == ref.b.fhi, (what, st)
    if norm != api.NORM_MAX:
        assert bits_equal(np.float64(st["rms"]), np.float64(res["rms"])) and st["sumsq"] == res["sumsq"] and st["psnr"] == res["psnr"], (what, st)
    else:
        assert abs(st["sumsq"] - ref.S(g)) <= ACCURACY * ref.S(g) and st["rms"] == math.sqrt(st["sumsq"] / nd), (what, st)
    return res


@pytest.mark.parametrize("call", mq.CALLS, ids=[c[0] for c in mq.CALLS])
def test_masked_quality_call_against_the_reference(ctx, call):
    for name, norm, target, m in mq.targets_of(*mq.key_of(call)):
        check_call(ctx, call, name, norm, target, m)


def test_no_undefined_sample_is_the_plain_quality_call(ctx):
    for call in (mq.CALLS[0], mq.CALLS[4], mq.CALLS[10]):
        _, kind, dims, seg, wtflag, f32, kw, form, _, _, _ = call
        f, _ = mq.ref_of(*mq.key_of(call))
        plain = ctx.encode_host_seg_quality_f32 if f32 else ctx.encode_host_seg_quality
        for norm, target in ((api.NORM_RMS, 1e-4), (api.NORM_PSNR, 60.0), (api.NORM_MAX, 1e-3)):
            p_info, p_data, p_res = plain(f, norm, target, seg=seg, wtflag=wtflag, **kw)
            p_data = p_data.copy()
            info, data, res = masked_quality_call(ctx, f, "host", norm, target, mq.BELOW, seg, wtflag, kw)
            assert info["mask"]["undefined"] == 0 and info["mask"]["mask_len"] == 0
            same_header(info, p_info, call[0])
            assert np.array_equal(data, p_data)
            for k in ("g", "tolrel", "max_abs", "rms", "sumsq", "range", "psnr", "max_rms", "trials"):
                assert bits_equal(np.float64(res[k]), np.float64(p_res[k])), (call[0], norm, k, res, p_res)


@pytest.mark.parametrize("call", [mq.CALLS[0], mq.CALLS[4], mq.CALLS[7]], ids=lambda c: c[0])
def test_masked_quality_call_is_consistent_with_itself(ctx, call):
    """test_gpu_quality.py's self-consistency test on a masked field: with the search confined to [g, GMAX], the RMS error a call
    reached returns the same g as a target (equality holds), and the double below it is WR_ERR_BOUND naming R(g)."""
    _, kind, dims, seg, wtflag, f32, kw, form, _, _, below = call
    _, ref = mq.ref_of(*mq.key_of(call))
    f = mq.field_of(call)
    for tol in (1e-3, 1e-7):
        _, _, res = ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, tol * ref.absmax, below, seg=seg)
        if res["g"] == GMAX:
            continue
        pinned = api.budget_tol(res["g"])
        _, _, at = ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, res["rms"], below, tol_min=pinned, seg=seg)
        assert at["g"] == res["g"] and at["rms"] == res["rms"] == at["max_rms"], (res, at)
        lower = float(np.nextafter(res["rms"], 0.0))
        out = np.full(ctx._seg_cap(f.shape, seg) + api.mask_bound(f.size, seg), 0xAB, np.uint8)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, lower, below, tol_min=pinned, seg=seg, out=out)
        assert "error %d:" % api.ERR_BOUND in str(e.value) and ("= %.17g" % res["rms"]) in str(e.value), str(e.value)
        assert np.all(out == 0xAB)


def test_masked_quality_call_is_deterministic(ctx):
    call = mq.CALLS[4]
    f = mq.field_of(call)
    runs = [ctx.encode_host_seg_quality_masked(f, api.NORM_PSNR, 60.0, call[10], seg=call[3]) for _ in range(3)]
    runs = [(i, d.copy(), r) for i, d, r in runs]
    for info, data, res in runs[1:]:
        assert all(bits_equal(np.float64(res[k]), np.float64(runs[0][2][k])) for k in ("rms", "sumsq", "max_abs", "psnr", "max_rms"))
        assert (res["g"], res["trials"]) == (runs[0][2]["g"], runs[0][2]["trials"]) and np.array_equal(data, runs[0][1])


def test_constant_padded_field(ctx):
    f = np.full((8, 8, 16), 2.5)
    f[3, 4, 5] = np.nan
    f[0, 0, :7] = np.inf
    und = ~np.isfinite(f)
    info, data, res = ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, tol_min=1e-9, seg=1024)
    assert info["nlay"] == 0 and info["ntot_enc"] == 0 and data.size == info["mask"]["mask_len"] > 0
    assert res["g"] == GMAX and res["rms"] == 0.0 and res["sumsq"] == 0.0 and res["max_abs"] == 0.0 and res["trials"] == 0
    assert info["mask"]["undefined"] == 8 and info["mask"]["pad"] == 2.5
    assert np.array_equal(data, api.mask_blob_host_ref(und.reshape(-1), 1024, 2.5))
    st = ctx.seg_error_stats_host_masked(f, info)
    assert st["defined"] == f.size - 8 and st["rms"] == 0.0 and st["max_abs"] == 0.0 and st["nonfinite"] == 0 and st["lo"] == st["hi"] == 2.5


def test_the_measuring_half_reads_nothing_at_an_undefined_sample_and_counts_a_nan_at_a_defined_one(ctx):
    call = mq.CALLS[4]
    _, ref = mq.ref_of(*mq.key_of(call))
    f = mq.field_of(call)
    info, data, res = ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-4 * ref.absmax, call[10], seg=call[3])
    enc = dict(info, data=data.copy())
    other = f.copy()
    other[ref.und] = np.resize(np.array([np.nan, np.inf, 1e300, -3.0]), int(ref.und.sum()))
    st = ctx.seg_error_stats_host_masked(other, enc)
    assert st["sumsq"] == res["sumsq"] and st["max_abs"] == res["max_abs"] and st["defined"] == ref.nd and st["nonfinite"] == 0
    at = tuple(np.argwhere(~ref.und)[5])
    other[at] = np.nan
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_error_stats_host_masked(other, enc)
    assert "error -1:" in str(e.value) and "1 difference" in str(e.value), str(e.value)
    st = ctx.seg_error_stats_host_masked(other, enc, allow_nonfinite=True)
    assert st["nonfinite"] == 1 and st["defined"] == ref.nd and 0 < st["sumsq"] <= res["sumsq"]
    # an unmasked record: every sample is defined
    plain, _ = ctx.encode_host_seg(ref.f_pad, 1e-5, seg=call[3])
    st = ctx.seg_error_stats_host_masked(ref.f_pad, plain)
    want = ctx.seg_error_stats_host(ref.f_pad, plain)
    assert st["defined"] == f.size and all(bits_equal(np.float64(st[k]), np.float64(want[k])) for k in want), (st, want)
    # a damaged blob is refused as the masked decode refuses it
    bad = dict(enc, data=enc["data"].copy())
    bad["data"][info["ntot_enc"]] ^= 0xFF
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_error_stats_host_masked(f, bad)
    assert "error -4:" in str(e.value), str(e.value)


def test_refusals(ctx):
    f = mq.field_of(mq.CALLS[2])
    seg = 1024
    cap = ctx._seg_cap(f.shape, seg) + api.mask_bound(f.size, seg)
    out = np.full(cap, 0xAB, np.uint8)
    # no defined sample
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality_masked(np.full(f.shape, np.nan), api.NORM_RMS, 1e-3, seg=seg, out=out)
    assert "error -1:" in str(e.value) and "no defined sample" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, 1e30, seg=seg, out=out)  # everything lies below the threshold
    assert "error -1:" in str(e.value) and "no defined sample" in str(e.value), str(e.value)
    # a NaN threshold
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, np.nan, seg=seg, out=out)
    assert "error -1:" in str(e.value) and "below" in str(e.value), str(e.value)
    # a buffer that holds the planes but not the bound of the mask blob
    info, data, _ = ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, seg=seg)
    short = np.full(info["ntot_enc"] + 16, 0xAB, np.uint8)
    assert short.size < info["ntot_enc"] + api.mask_bound(f.size, seg)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, seg=seg, out=short)
    assert "error -5:" in str(e.value) and "mask" in str(e.value), str(e.value)
    assert np.all(short == 0xAB)
    # a local cutoff, a kept residual
    for m in ((2, 1, 1), (1, 2, 2)):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, seg=seg, m=m, out=out)
        assert "error -3:" in str(e.value) and "local cutoff" in str(e.value), str(e.value)
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_quality_masked(f, api.NORM_RMS, 1e-3, seg=seg, out=out)
        assert "error -3:" in str(e.value) and "residual" in str(e.value), str(e.value)
    finally:
        ctx.set_keep_residual(False)
    assert np.all(out == 0xAB)
