"""The three masked decode drivers against each other: the whole-field call (wr_decode_*_seg_masked), the single region call
(wr_decode_*_seg_roi_masked) and the batch call (wr_decode_*_seg_roi_batch_masked) with one field and one region.  Each is
pinned against references of its own elsewhere; here one record goes through all three and they must agree: the same output
bytes and the same undefined, pad and mask_len on the whole level-0 box; the same output and the same counter deltas on a
sub-region; the same error code and text for a damaged blob (the batch call says "field 0: " in front), the output untouched;
and a constant padded field with a mask, which every driver handles in its own place.

Shapes: masked_roi_cases.CHAIN and GENERAL with the mask cut at 16 and 48 symbols, so that a plane has tens of segments and a
small region lists a few of them, as WRS1; one FUSED record as WRS2."""
import struct

import numpy as np
import pytest

import masked_roi_cases as mc
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

TOL = 1e-5
BELOW = -1e30
UNDEF = -9.99e33
SENTINEL = 4242.0
PREFIX = "field 0: "

# (shape, mask segment length, format, level and sub-region)
RECORDS = [
    (mc.CHAIN, 16, dict(brick=0), 0, ((1, 6), (2, 11), (3, 20))),
    (mc.CHAIN, 48, dict(brick=0), 1, ((0, 4), (1, 8), (2, 15))),
    (mc.GENERAL, 16, dict(brick=0), 0, ((2, 11), (3, 19), (5, 36))),
    (mc.GENERAL, 48, dict(brick=0), 1, ((1, 6), (0, 11), (2, 19))),
    (mc.FUSED, 48, dict(brick=8), 0, ((16, 48), (16, 48), (16, 48))),
]


def rid(r):
    return "%s.seg%d.%s" % ("x".join(map(str, r[0])), r[1], "wrs2" if r[2]["brick"] else "wrs1")


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def ints(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def zyx(shape):
    nx, ny, nz = shape
    return nz, ny, nx


def whole_box(shape):
    nx, ny, nz = shape
    return ((0, nz), (0, ny), (0, nx))


_records = {}


def record_of(ctx, r, dtype=np.float64):
    """the record of a table row with the recipe's undefined set, encoded once, read-only"""
    shape, seg, fmt = r[0], r[1], r[2]
    key = (rid(r), np.dtype(dtype).name)
    if key not in _records:
        nx, ny, nz = shape
        f = synth.field(nx, ny, nz, seed=11 + nx + 7 * ny + 49 * nz).astype(dtype)
        f[mc.und_recipe(shape)] = dtype(UNDEF)
        enc = ctx.encode_host_seg_masked if np.dtype(dtype) == np.float64 else ctx.encode_host_seg_masked_f32
        rec, _ = enc(f, TOL, BELOW, seg=seg, **fmt)
        rec["data"] = rec["data"].copy()
        rec["data"].setflags(write=False)
        assert rec["nlay"] > 0 and rec["mask"]["mask_len"] > 0
        _records[key] = rec
    return _records[key]


def mask_front(rec):
    """(offset of the mask's first segment stream in rec["data"], seg, the segments' lengths)"""
    at = rec["ntot_enc"] + 32
    magic, seg, nseg = bytes(rec["data"][at:at + 4]), *struct.unpack("<II", bytes(rec["data"][at + 4:at + 12]))
    assert magic == b"WRS1"
    lens = np.frombuffer(bytes(rec["data"][at + 12:at + 12 + 4 * nseg]), "<u4")
    return at + 12 + 4 * nseg, seg, lens


# ---- the three drivers, one signature: (output array shaped like the region, mask record); a refusal raises
def host_calls(ctx, shape, level, roi, dtype=np.float64):
    """{driver: call(rec, fill, out)}; "whole" only where the region is the whole level-0 box"""
    f32 = np.dtype(dtype) == np.float32
    s = zyx(shape)

    def whole(rec, fill, out):
        fn = ctx.decode_host_seg_masked_f32 if f32 else ctx.decode_host_seg_masked
        return fn(out.reshape(s), rec, fill)[0]

    def region(rec, fill, out):
        fn = ctx.decode_host_seg_roi_masked_f32 if f32 else ctx.decode_host_seg_roi_masked
        return fn(out, s, level, roi, rec, fill)[0]

    def batch(rec, fill, out):
        masks = []
        ctx.decode_host_seg_rois_batch_masked(s, level, [roi], [rec], fill, dtype=dtype, out=out.reshape(-1), masks=masks)
        return masks[0]

    calls = {"region": region, "batch": batch}
    if level == 0 and roi == whole_box(shape):
        calls["whole"] = whole
    return calls


def device_calls(ctx, shape, level, roi):
    s = zyx(shape)
    calls = {
        "region": lambda rec, fill, buf: ctx.decode_seg_roi_masked(buf, s, level, roi, rec, fill)[0],
        "batch": lambda rec, fill, buf: ctx.decode_seg_rois_batch_masked(buf, s, level, [roi], [rec], fill)[0][0],
    }
    if level == 0 and roi == whole_box(shape):
        calls["whole"] = lambda rec, fill, buf: ctx.decode_seg_masked(buf, s, rec, fill)[0]
    return calls


def run_host(call, rec, fill, roi, dtype=np.float64):
    out = np.full(api.roi_shape(roi), SENTINEL, dtype)
    return out, call(rec, fill, out)


def run_device(ctx, call, rec, fill, roi):
    count = int(np.prod(api.roi_shape(roi)))
    buf = ctx.to_device(np.full(count + 1, SENTINEL))
    try:
        res = call(rec, fill, buf)
        flat = buf.download(np.float64, count + 1)
    finally:
        buf.free()
    assert flat[-1] == SENTINEL
    return flat[:count].reshape(api.roi_shape(roi)), res


def same_result(a, b):
    assert a["undefined"] == b["undefined"] and a["mask_len"] == b["mask_len"]
    assert np.float64(a["pad"]).view(np.uint64) == np.float64(b["pad"]).view(np.uint64)


@pytest.mark.parametrize("r", RECORDS, ids=rid)
def test_one_record_three_drivers(ctx, r):
    shape = r[0]
    roi = whole_box(shape)
    und = mc.und_recipe(shape)
    for dtype, fill in ((np.float64, np.nan), (np.float32, -77.25)):
        rec = record_of(ctx, r, dtype)
        got = {name: run_host(call, rec, fill, roi, dtype) for name, call in host_calls(ctx, shape, 0, roi, dtype).items()}
        assert sorted(got) == ["batch", "region", "whole"]
        out, res = got["whole"]
        assert res["undefined"] == int(und.sum()) == rec["mask"]["undefined"] and res["mask_len"] == rec["mask"]["mask_len"]
        assert np.array_equal(out == dtype(fill) if fill == fill else np.isnan(out), und)
        for name in ("region", "batch"):
            assert np.array_equal(ints(got[name][0]), ints(out)), (name, np.dtype(dtype).name)
            same_result(got[name][1], res)
    rec = record_of(ctx, r)
    want, want_res = run_host(host_calls(ctx, shape, 0, roi)["whole"], rec, -1.5, roi)
    for name, call in device_calls(ctx, shape, 0, roi).items():
        out, res = run_device(ctx, call, rec, -1.5, roi)
        assert np.array_equal(ints(out), ints(want)), name
        same_result(res, want_res)


@pytest.mark.parametrize("r", RECORDS, ids=rid)
def test_sub_region_single_call_against_batch_call(ctx, r):
    shape, _, _, level, roi = r
    rec = record_of(ctx, r)
    _, seg, lens = mask_front(rec)
    listed = api.mask_roi_segments(zyx(shape), level, roi, seg)
    assert 0 < len(listed) < len(lens), "the region lists some of the mask's segments, not all"
    stats = (api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP)
    got, delta = {}, {}
    for name, call in host_calls(ctx, shape, level, roi).items():
        before = [api.stat(k) for k in stats]
        got[name] = run_host(call, rec, np.nan, roi)
        delta[name] = [api.stat(k) - b for k, b in zip(stats, before)]
    assert sorted(got) == ["batch", "region"]
    assert np.array_equal(ints(got["region"][0]), ints(got["batch"][0]))
    same_result(got["region"][1], got["batch"][1])
    case = (shape, level, roi, seg)
    assert got["region"][1]["undefined"] == int(mc.coarse_und(mc.und_recipe(shape), case).sum())
    assert np.array_equal(np.isnan(got["region"][0]), mc.coarse_und(mc.und_recipe(shape), case))
    assert delta["region"] == delta["batch"]
    assert delta["region"][0] == len(listed) and delta["region"][1] == int(lens[listed].sum())


def refusal(call, rec, roi):
    """(error text without the batch's prefix, None) or (None, output) of a host call on a sentinel-filled output, which a
    refusal must leave alone"""
    out = np.full(api.roi_shape(roi), SENTINEL)
    try:
        call(rec, np.nan, out)
    except api.WaveRangeError as e:
        assert (out == SENTINEL).all(), "a refused call wrote to the output"
        return str(e), None
    return None, out


def header(n, count, pad, magic=b"WRM1", reserved=0):
    return np.frombuffer(magic + struct.pack("<IQQd", reserved, n, count, pad), dtype=np.uint8)


@pytest.mark.parametrize("r", [RECORDS[0], RECORDS[3]], ids=rid)
def test_damage_matrix(ctx, r):
    """every refusal of a blob, through all three drivers: the same code and the same text.  These are refusals on the host and
    the decoder's ordinary count of segments that do not decode."""
    shape, seg_len, _, level, sub = r
    rec = record_of(ctx, r)
    nt, n = rec["ntot_enc"], shape[0] * shape[1] * shape[2]
    planes, blob = rec["data"][:nt], rec["data"][nt:]
    count, pad = rec["mask"]["undefined"], rec["mask"]["pad"]
    first, seg, lens = mask_front(rec)
    assert seg == seg_len and n % 8
    whole = whole_box(shape)

    def with_blob(b):
        return dict(rec, data=np.concatenate([planes, np.asarray(b, dtype=np.uint8)]))

    index = blob.copy()
    index[32 + 12:32 + 16] = np.frombuffer(struct.pack("<I", int(lens[0]) + 1), np.uint8)  # the first segment's length
    host_side = {
        "truncated header": (blob[:17], "truncated header"),
        "wrong magic": (np.concatenate([header(n, count, pad, magic=b"WRM2"), blob[32:]]), "wrong magic"),
        "reserved word": (np.concatenate([header(n, count, pad, reserved=7), blob[32:]]), "reserved word"),
        "sample count": (np.concatenate([header(n - 1, count, pad), blob[32:]]), "sample count"),
        "undefined > n": (np.concatenate([header(n, n + 1, pad), blob[32:]]), "more undefined samples"),
        "segment index": (index, "mask blob: "),
    }
    stats = (api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP, api.STAT_ROI_CODER_LAUNCHES)
    for name, (bad, says) in host_side.items():
        texts = {}
        before = [api.stat(k) for k in stats]
        for roi in (whole, sub):
            for driver, call in host_calls(ctx, shape, 0 if roi == whole else level, roi).items():
                text, _ = refusal(call, with_blob(bad), roi)
                assert text is not None, (name, driver)
                assert (driver == "batch") == (PREFIX in text), (name, driver, text)
                texts[(driver, roi == whole)] = text.replace(PREFIX, "", 1)
        assert [api.stat(k) for k in stats] == before, name  # nothing was uploaded or launched
        assert len(set(texts.values())) == 1, (name, texts)
        text = texts[("whole", True)]
        assert "error -4: mask blob: " in text and says in text, (name, text)
    # ---- a byte flipped in a listed segment: the coder's model counts at the head of the segment's stream
    listed = api.mask_roi_segments(zyx(shape), level, sub, seg)
    starts = first + np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    refused = 0
    for k in listed[:6]:
        data = rec["data"].copy()
        data[starts[k] + 2] ^= 0x40
        bad = dict(rec, data=data)
        sub_calls = host_calls(ctx, shape, level, sub)
        text, out = refusal(sub_calls["region"], bad, sub)
        text_b, out_b = refusal(sub_calls["batch"], bad, sub)
        if text is None:  # the flip still decodes, to other bits: both region calls take it
            assert text_b is None and np.array_equal(ints(out), ints(out_b))
            continue
        refused += 1
        assert text_b is not None and PREFIX in text_b and text_b.replace(PREFIX, "", 1) == text
        assert "error -4: mask blob: " in text
        for driver, call in host_calls(ctx, shape, 0, whole).items():
            text_w, _ = refusal(call, bad, whole)
            assert text_w is not None and text_w.replace(PREFIX, "", 1) == text, (driver, text_w)
    assert refused >= 1, "a flipped bit in the model of a listed segment was never noticed"
    # ---- the two properties of the whole mask: the whole-field call refuses, the region calls do not look
    bits = mc.packed(mc.und_recipe(shape))
    beyond = bits.copy()
    beyond[-1] |= 0x80
    whole_only = {
        "a bit beyond n": (np.concatenate([header(n, count, pad), api.seg_encode_host_ref(beyond, seg)]), "a bit beyond the field's last sample is set"),
        "count": (np.concatenate([header(n, count - 1, pad), blob[32:]]), "the mask's set bits are not the count in its header"),
    }
    good = {roi: run_host(host_calls(ctx, shape, 0 if roi == whole else level, roi)["region"], rec, np.nan, roi) for roi in (whole, sub)}
    for name, (bad, says) in whole_only.items():
        text, _ = refusal(host_calls(ctx, shape, 0, whole)["whole"], with_blob(bad), whole)
        assert text is not None and "error -4: mask blob: " + says in text, (name, text)
        for roi in (whole, sub):
            for driver in ("region", "batch"):
                out, res = run_host(host_calls(ctx, shape, 0 if roi == whole else level, roi)[driver], with_blob(bad), np.nan, roi)
                assert np.array_equal(ints(out), ints(good[roi][0])), (name, driver)
                assert res["undefined"] == good[roi][1]["undefined"], (name, driver)
    # and the record still decodes
    out, _ = run_host(host_calls(ctx, shape, 0, whole)["whole"], rec, np.nan, whole)
    assert np.array_equal(ints(out), ints(good[whole][0]))


@pytest.mark.parametrize("r", [RECORDS[0], RECORDS[3]], ids=rid)
def test_constant_padded_field_with_a_mask(ctx, r):
    shape, seg, _, level, sub = r
    nx, ny, nz = shape
    und = mc.und_recipe(shape)
    whole = whole_box(shape)
    recs = {}
    for dtype in (np.float64, np.float32):
        f = np.full((nz, ny, nx), 2.5, dtype)
        f[und] = np.nan
        enc = ctx.encode_host_seg_masked if dtype == np.float64 else ctx.encode_host_seg_masked_f32
        rec, _ = enc(f, TOL, seg=seg)
        rec["data"] = rec["data"].copy()
        assert rec["nlay"] == 0 and rec["ntot_enc"] == 0 and rec["mask"]["mask_len"] > 0
        recs[dtype] = rec
    sub_case = (shape, level, sub, seg)
    step = 1 << level
    for dtype, fill in ((np.float64, np.nan), (np.float32, 9.0)):
        rec = recs[dtype]
        want = np.where(und, dtype(fill), dtype(2.5))
        for name, call in host_calls(ctx, shape, 0, whole, dtype).items():
            out, res = run_host(call, rec, fill, whole, dtype)
            assert np.array_equal(ints(out), ints(want)), (name, np.dtype(dtype).name)
            assert res["undefined"] == int(und.sum()) and res["pad"] == 2.5 and res["mask_len"] == rec["mask"]["mask_len"]
        (z0, z1), (y0, y1), (x0, x1) = sub
        crop = np.ascontiguousarray(np.where(und, dtype(fill), dtype(2.5))[::step, ::step, ::step][z0:z1, y0:y1, x0:x1])
        for name, call in host_calls(ctx, shape, level, sub, dtype).items():
            out, res = run_host(call, rec, fill, sub, dtype)
            assert np.array_equal(ints(out), ints(crop)), (name, np.dtype(dtype).name)
            assert res["undefined"] == int(mc.coarse_und(und, sub_case).sum())
    rec = recs[np.float64]
    for roi, lvl in ((whole, 0), (sub, level)):
        want, want_res = run_host(host_calls(ctx, shape, lvl, roi)["region"], rec, -1.5, roi)
        for name, call in device_calls(ctx, shape, lvl, roi).items():
            out, res = run_device(ctx, call, rec, -1.5, roi)
            assert np.array_equal(ints(out), ints(want)), name
            same_result(res, want_res)
