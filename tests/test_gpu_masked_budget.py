"""Encode a masked field to a byte budget on the GPU (include/waverange_amd.h, "Masked fields in the tolerance searches").  No CPU
reference is needed: the pad and the blob's length come from wr_encode_host_seg_masked (the blob does not depend on the
tolerance), and the masked budget call at max_bytes must be the plain budget call of the padded field at max_bytes - mask_len --
g, bound, probe passes, header and bytes -- with that blob appended, the whole record within the budget."""
import numpy as np
import pytest

import masked_quality_cases as mq
from util import bits_equal
from waverange_amd import api

pytestmark = pytest.mark.gpu

HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")
# (kind, dims, seg, mask, undefined value, below)
CASES = [("smooth", (64, 64, 64), 0, "land", np.nan, -np.inf), ("noise", (64, 64, 64), 0, "speckle", mq.UNDEF, mq.BELOW),
         ("smooth", (39, 37, 33), 1024, "ball", mq.UNDEF, mq.BELOW), ("noise", (39, 37, 33), 1024, "single", np.inf, -np.inf)]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def calls(ctx, f32):
    if f32:
        return ctx.encode_host_seg_masked_f32, ctx.encode_host_seg_budget_f32, ctx.encode_host_seg_budget_masked_f32
    return ctx.encode_host_seg_masked, ctx.encode_host_seg_budget, ctx.encode_host_seg_budget_masked


def inputs(ctx, case, f32):
    """(the caller's field, the padded field, the blob) of a case"""
    kind, dims, seg, mask, value, below = case
    f = mq.make_field(kind, dims, f32)
    und = mq.make_mask(mask, dims)
    f[und] = value
    rec, _ = calls(ctx, f32)[0](f, 1e-3, below, seg=seg)
    m = rec["mask"]
    assert m["undefined"] == int(und.sum()) and m["mask_len"] > 32
    f_pad = np.where(und, f.dtype.type(m["pad"]), f)
    assert np.all(np.isfinite(f_pad))
    return f, np.ascontiguousarray(f_pad), rec["data"][rec["ntot_enc"]:].copy()


def first_number_after(text, words):
    return int(text.split(words, 1)[1].split()[0])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s" % (c[0], "x".join(map(str, c[1])), c[3]))
def test_masked_budget_call_is_the_plain_call_with_the_blob_taken_off_the_budget(ctx, case, f32):
    kind, dims, seg, mask, value, below = case
    _, plain_budget, masked_budget = calls(ctx, f32)
    f, f_pad, blob = inputs(ctx, case, f32)
    mask_len = blob.size
    # the floor: the blob alone, and one byte below the blob plus the coarsest tolerance's bound
    out = np.full(ctx._seg_cap(f.shape, seg) + api.mask_bound(f.size, seg), 0xAB, np.uint8)
    before = api.stat(api.STAT_BUDGET_CODER_RUNS)
    with pytest.raises(api.WaveRangeError) as e:
        masked_budget(f, mask_len, below, seg=seg, out=out)
    assert "error %d:" % api.ERR_BUDGET in str(e.value), str(e.value)
    floor = first_number_after(str(e.value), "coarsest tolerance takes: ")
    with pytest.raises(api.WaveRangeError) as e:  # the plain call names B(GMAX)
        plain_budget(f_pad, 1, seg=seg)
    assert floor == mask_len + first_number_after(str(e.value), "coarsest tolerance takes: "), (floor, mask_len, str(e.value))
    with pytest.raises(api.WaveRangeError) as e:
        masked_budget(f, floor - 1, below, seg=seg, out=out)
    assert "error %d:" % api.ERR_BUDGET in str(e.value) and str(floor) in str(e.value), str(e.value)
    assert np.all(out == 0xAB) and api.stat(api.STAT_BUDGET_CODER_RUNS) == before
    for max_bytes in sorted({floor, floor + floor // 3, 4 * floor, max(floor, int(0.35 * f.size * f.itemsize))}):
        before = api.stat(api.STAT_BUDGET_CODER_RUNS)
        info, data, res = masked_budget(f, max_bytes, below, seg=seg)
        data = data.copy()
        grew = api.stat(api.STAT_BUDGET_CODER_RUNS) - before
        p_info, p_data, p_res = plain_budget(f_pad, max_bytes - mask_len, seg=seg)
        what = (case, f32, max_bytes, res, p_res)
        print(case, f32, "budget", max_bytes, "mask_len", mask_len, "g", res["g"], "bound", res["bound"], "ntot_enc", info["ntot_enc"])
        assert (res["g"], res["tolrel"], res["bound"], res["probe_passes"]) == (p_res["g"], p_res["tolrel"], p_res["bound"], p_res["probe_passes"]), what
        for k in HEADER_KEYS:
            assert info[k] == p_info[k], (what, k)
        assert list(info["len_enc_vec"]) == list(p_info["len_enc_vec"]), what
        assert bits_equal(info["deps_vec"], p_info["deps_vec"]) and bits_equal(info["minval_vec"], p_info["minval_vec"]), what
        nt = info["ntot_enc"]
        assert np.array_equal(data[:nt], p_data), what
        assert info["mask"]["mask_len"] == mask_len and data.size == nt + mask_len and np.array_equal(data[nt:], blob), what
        assert nt + mask_len <= res["bound"] + mask_len <= max_bytes, what
        assert grew == info["nlay"] >= 1, what


def test_device_form_equals_the_host_form(ctx):
    case = CASES[2]
    kind, dims, seg, mask, value, below = case
    f, f_pad, blob = inputs(ctx, case, False)
    max_bytes = int(0.2 * f.size * 8)
    info, data, res = ctx.encode_host_seg_budget_masked(f, max_bytes, below, seg=seg)
    data = data.copy()
    buf = ctx.to_device(f)
    try:
        d_info, d_data, d_res = ctx.encode_seg_budget_masked(buf, f.shape, max_bytes, below, seg=seg)
    finally:
        buf.free()
    assert (d_res["g"], d_res["bound"], d_res["probe_passes"]) == (res["g"], res["bound"], res["probe_passes"])
    assert np.array_equal(d_data, data) and d_info["mask"]["mask_len"] == blob.size


def test_no_undefined_sample_is_the_plain_budget_call(ctx):
    f = mq.make_field("smooth", (39, 37, 33))
    max_bytes = int(0.2 * f.size * 8)
    p_info, p_data, p_res = ctx.encode_host_seg_budget(f, max_bytes, seg=1024)
    p_data = p_data.copy()
    info, data, res = ctx.encode_host_seg_budget_masked(f, max_bytes, mq.BELOW, seg=1024)
    assert info["mask"]["undefined"] == 0 and info["mask"]["mask_len"] == 0 and np.array_equal(data, p_data)
    assert (res["g"], res["bound"], res["probe_passes"]) == (p_res["g"], p_res["bound"], p_res["probe_passes"])


def test_constant_padded_field_and_refusals(ctx):
    f = np.full((8, 8, 16), 2.5)
    f[3, 4, 5] = np.nan
    g_min = api.budget_index(1e-4)
    rec, _ = ctx.encode_host_seg_masked(f, 1e-3, seg=1024)
    mask_len = rec["mask"]["mask_len"]
    info, data, res = ctx.encode_host_seg_budget_masked(f, mask_len, tol_min=1e-4, seg=1024)  # the blob is all there is
    assert info["nlay"] == 0 and info["ntot_enc"] == 0 and np.array_equal(data, rec["data"])
    assert res["g"] == g_min and res["bound"] == 0
    out = np.full(ctx._seg_cap(f.shape, 1024) + api.mask_bound(f.size, 1024), 0xAB, np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget_masked(f, mask_len - 1, tol_min=1e-4, seg=1024, out=out)
    assert "error %d:" % api.ERR_BUDGET in str(e.value) and str(mask_len) in str(e.value), str(e.value)
    assert np.all(out == 0xAB)
    g = mq.make_field("smooth", (16, 16, 16))
    g[1, 2, 3] = np.nan
    big = 1 << 20
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget_masked(np.full(g.shape, np.inf), big, seg=1024)
    assert "error -1:" in str(e.value) and "no defined sample" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget_masked(g, big, np.nan, seg=1024)
    assert "error -1:" in str(e.value) and "below" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget_masked(g, big, seg=1024, m=(2, 1, 1))
    assert "error -3:" in str(e.value) and "local cutoff" in str(e.value), str(e.value)
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_budget_masked(g, big, seg=1024)
        assert "error -3:" in str(e.value) and "residual" in str(e.value), str(e.value)
    finally:
        ctx.set_keep_residual(False)
    short = np.full(64, 0xAB, np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget_masked(g, big, seg=1024, out=short)
    assert "error -5:" in str(e.value), str(e.value)
    assert np.all(short == 0xAB)
