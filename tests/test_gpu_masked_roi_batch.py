"""The masked region decode across a batch of fields through the whole path on the GPU (wr_decode_*_seg_roi_batch_masked), over
the case table of masked_roi_batch_cases.py.

The yardstick is the loop of decode_host_seg_roi_masked over fields and regions: region i of field f is that call's result,
bit for bit, and masks[f]["undefined"] the sum of its counts.  The second reference is where(und[::s, ::s, ::s][roi], fill, the
plain decode_host_seg_rois_batch on the field parts).  The fields of a batch cycle through WRS1, WRS2 (brick 8) and WRS3 (4
strands) and through three tolerances, so plane counts differ; a field marked '-' in the table is a record without a blob.  A WRS3
record needs 16 * strands <= seg: there the table's 16 and 48 become 64 and 96, and the mask blob is cut at the record's length
too -- the planner is asked at the length the blob's own header holds.
Then: fp32 and the device form, max_planes below nlay, constant fields with and without a blob (also a call of nothing but
constant fields), the counters, a mask segment damaged in three ways, and one field with six regions."""
import struct

import numpy as np
import pytest

import masked_roi_batch_cases as bc
import masked_roi_cases as mc
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

FORMATS = [("wrs1", dict(brick=0, strands=0)), ("wrs2", dict(brick=8, strands=0)), ("wrs3", dict(brick=0, strands=4))]
WRS3_SEG = {16: 64, 48: 96, 0: 0}
TOLS = [1e-3, 1e-5, 1e-7]
BELOW = -1e30
UNDEF = -9.99e33
SENTINEL = 4242.0


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


def field_part(rec):
    return dict(rec, data=rec["data"][:rec["ntot_enc"]])


def mask_front(rec):
    """(offset of the mask's first segment stream in rec["data"], seg, the segments' lengths)"""
    at = rec["ntot_enc"] + 32
    magic, seg, nseg = bytes(rec["data"][at:at + 4]), *struct.unpack("<II", bytes(rec["data"][at + 4:at + 12]))
    assert magic == b"WRS1"
    lens = np.frombuffer(bytes(rec["data"][at + 12:at + 12 + 4 * nseg]), "<u4")
    return at + 12 + 4 * nseg, seg, lens


_records = {}


def record_of(ctx, shape, name, und, slot, seg, dtype=np.float64):
    """the record of a field of the batch: `und` is its undefined set (None: none, the record has no blob), `name` names the set,
    `slot` picks format and tolerance; encoded once"""
    key = (shape, name, slot, seg, np.dtype(dtype).name)
    if key not in _records:
        nx, ny, nz = shape
        fmt, params = FORMATS[slot % 3]
        f = (synth.field(nx, ny, nz, seed=31 + nx + 7 * ny + 49 * nz + slot) * (1.0 + slot)).astype(dtype)
        if und is not None:
            f[und] = dtype(UNDEF)
        enc = ctx.encode_host_seg_masked if np.dtype(dtype) == np.float64 else ctx.encode_host_seg_masked_f32
        rec, _ = enc(f, TOLS[slot % 3], BELOW, seg=WRS3_SEG[seg] if fmt == "wrs3" else seg, **params)
        rec["data"] = rec["data"].copy()
        rec["data"].setflags(write=False)
        _records[key] = rec
    return _records[key]


def batch_of(ctx, case, dtype=np.float64):
    """(records, undefined sets or None) of a case"""
    shape, _, _, seg, fields = case
    recs, unds = [], []
    for f, k in enumerate(fields):
        und = bc.und_of(case, f)
        unds.append(und)
        name = k if k in "RI-" else "A" + bc.case_id(case)
        recs.append(record_of(ctx, shape, name, und, f, seg, dtype))
    return recs, unds


_loops = {}


def loop_of(ctx, case, dtype, fill, max_planes=0):
    """the yardstick: decode_host_seg_roi_masked per field and region; ([[region arrays]], [undefined per field]); computed once"""
    key = (bc.case_id(case), np.dtype(dtype).name, repr(fill), max_planes)
    if key not in _loops:
        shape, level, rois, _, _ = case
        recs, _ = batch_of(ctx, case, dtype)
        fn = ctx.decode_host_seg_roi_masked if np.dtype(dtype) == np.float64 else ctx.decode_host_seg_roi_masked_f32
        outs, counts = [], []
        for rec in recs:
            row, count = [], 0
            for roi in rois:
                out = np.full(api.roi_shape(roi), SENTINEL, dtype)
                res, _ = fn(out, zyx(shape), level, roi, rec, fill, max_planes)
                out.setflags(write=False)
                row.append(out)
                count += res["undefined"]
            outs.append(row)
            counts.append(count)
        _loops[key] = (outs, counts)
    return _loops[key]


def check_against_loop(got, want):
    for f, (grow, wrow) in enumerate(zip(got, want)):
        for i, (g, w) in enumerate(zip(grow, wrow)):
            assert g.shape == w.shape and np.array_equal(ints(g), ints(w)), ("field", f, "region", i)


def planner(case, recs):
    """(mask segments, their stream bytes) the call must list, by wr_mask_roi_segments_multi at each blob's own seg"""
    shape, level, rois, _, _ = case
    segments = nbytes = 0
    for rec in recs:
        if rec["mask"]["mask_len"] == 0:
            continue
        _, seg, lens = mask_front(rec)
        listed = api.mask_roi_segments_multi(zyx(shape), level, rois, seg)
        segments += len(listed)
        nbytes += int(lens[listed].sum())
    return segments, nbytes


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_batch_is_the_loop_of_single_calls(ctx, case):
    shape, level, rois, _, fields = case
    recs, unds = batch_of(ctx, case)
    assert [r["mask"]["mask_len"] > 0 for r in recs] == [k != "-" for k in fields]
    assert len({r["nlay"] for r in recs}) > 1 or len(recs) < 3, "the fields of a batch differ in plane count"
    fill = np.nan
    want, want_counts = loop_of(ctx, case, np.float64, fill)
    T = int(bc.offsets(case)[-1])
    out = np.full(len(recs) * T, SENTINEL)
    masks, tm = [], {}
    before = [api.stat(k) for k in (api.STAT_ROI_CODER_LAUNCHES, api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP, api.STAT_ROI_SEGMENTS, api.STAT_ROI_BYTES_UP)]
    got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, recs, fill, out=out, masks=masks, timings=tm)
    delta = [api.stat(k) - b for k, b in zip((api.STAT_ROI_CODER_LAUNCHES, api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP, api.STAT_ROI_SEGMENTS,
                                               api.STAT_ROI_BYTES_UP), before)]
    check_against_loop(got, want)
    # the second reference: the plain batch call on the field parts, and the coarse mask
    before_plain = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
    base = ctx.decode_host_seg_rois_batch(zyx(shape), level, rois, [field_part(r) for r in recs])
    plain_delta = api.stat(api.STAT_ROI_SEGMENTS) - before_plain[0], api.stat(api.STAT_ROI_BYTES_UP) - before_plain[1]
    for f, und in enumerate(unds):
        for i in range(len(rois)):
            ref = base[f][i] if und is None else np.where(mc.coarse_und(und, bc.single(case, i)), fill, base[f][i])
            assert np.array_equal(ints(got[f][i]), ints(ref)), ("field", f, "region", i)
    # the records
    fill_ms = {m["fill_ms"] for m, k in zip(masks, fields) if k != "-"}
    assert len(fill_ms) == 1 and fill_ms.pop() > 0
    for f, (m, rec) in enumerate(zip(masks, recs)):
        if fields[f] == "-":
            assert m == dict(m, undefined=0, pad=0.0, mask_len=0, split_ms=0.0, fill_ms=0.0, mask_coder_ms=0.0)
            continue
        assert m["undefined"] == want_counts[f] == sum(int(mc.coarse_und(unds[f], bc.single(case, i)).sum()) for i in range(len(rois)))
        assert m["mask_len"] == rec["mask"]["mask_len"] and m["split_ms"] == 0 and m["mask_coder_ms"] == 0
        assert np.float64(m["pad"]).view(np.uint64) == np.float64(rec["mask"]["pad"]).view(np.uint64)
    # the counters: at most two launches; the masks' segments and bytes are the planner's; the field parts count as in the plain call
    assert 1 <= delta[0] <= 2
    assert (delta[1], delta[2]) == planner(case, recs)
    assert (delta[3], delta[4]) == plain_delta
    assert tm["rangecoder"] > 0


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_f32_and_device_forms(ctx, case):
    shape, level, rois, _, fields = case
    fill = -77.25
    T = int(bc.offsets(case)[-1])
    recs32, _ = batch_of(ctx, case, np.float32)
    want32, counts32 = loop_of(ctx, case, np.float32, fill)
    masks = []
    got = ctx.decode_host_seg_rois_batch_masked_f32(zyx(shape), level, rois, recs32, fill, masks=masks)
    check_against_loop(got, want32)
    assert [m["undefined"] for m in masks] == counts32
    recs, _ = batch_of(ctx, case)
    want, counts = loop_of(ctx, case, np.float64, fill)
    buf = ctx.to_device(np.full(len(recs) * T + 1, SENTINEL))
    try:
        masks, _ = ctx.decode_seg_rois_batch_masked(buf, zyx(shape), level, rois, recs, fill)
        flat = buf.download(np.float64, len(recs) * T + 1)
    finally:
        buf.free()
    offs = bc.offsets(case)
    assert flat[-1] == SENTINEL
    check_against_loop([[flat[f * T + offs[i]:f * T + offs[i + 1]].reshape(api.roi_shape(r)) for i, r in enumerate(rois)] for f in range(len(recs))], want)
    assert [m["undefined"] for m in masks] == counts


def test_max_planes_below_nlay(ctx):
    for case in (c for c in bc.CASES if c[0] in (mc.GENERAL, mc.CHAIN) and c[1] in (0, 1)):
        shape, level, rois, _, _ = case
        recs, _ = batch_of(ctx, case)
        assert max(r["nlay"] for r in recs) > 1 and min(r["nlay"] for r in recs) >= 1
        want, counts = loop_of(ctx, case, np.float64, np.nan, 1)
        full, _ = loop_of(ctx, case, np.float64, np.nan)
        masks = []
        got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, recs, np.nan, max_planes=1, masks=masks)
        check_against_loop(got, want)
        assert [m["undefined"] for m in masks] == counts
        assert any(not np.array_equal(ints(a), ints(b)) for ra, rb in zip(want, full) for a, b in zip(ra, rb)), "one plane decodes like all of them"


def constant_records(ctx, shape, seg):
    """(a constant padded field with a blob, its undefined set, a constant field without a blob)"""
    nx, ny, nz = shape
    und = mc.und_isolated(shape)
    f = np.full((nz, ny, nx), 2.5)
    f[und] = np.nan
    with_blob, _ = ctx.encode_host_seg_masked(f, 1e-5, seg=seg)
    without, _ = ctx.encode_host_seg_masked(np.full((nz, ny, nx), -7.0), 1e-5, seg=seg)
    for r in (with_blob, without):
        r["data"] = r["data"].copy()
        assert r["nlay"] == 0 and r["ntot_enc"] == 0
    assert with_blob["mask"]["mask_len"] > 0 and without["mask"]["mask_len"] == 0
    return with_blob, und, without


@pytest.mark.parametrize("case", [bc.CASES[0], bc.CASES[8], bc.CASES[11]], ids=bc.case_id)
def test_constant_fields_with_and_without_a_blob(ctx, case):
    shape, level, rois, seg, _ = case
    recs, unds = batch_of(ctx, case)
    cb, cund, cn = constant_records(ctx, shape, seg)
    T = int(bc.offsets(case)[-1])
    offs = bc.offsets(case)

    def want_of(batch, batch_unds, dtype, fill):
        fn = ctx.decode_host_seg_roi_masked if dtype == np.float64 else ctx.decode_host_seg_roi_masked_f32
        rows = []
        for rec in batch:
            row = []
            for roi in rois:
                out = np.full(api.roi_shape(roi), SENTINEL, dtype)
                fn(out, zyx(shape), level, roi, rec, fill)
                row.append(out)
            rows.append(row)
        return rows

    # masked, constant with a blob, constant without, unmasked or masked, constant with a blob last
    mixed = [recs[0], cb, cn, recs[1], cb]
    mixed_unds = [unds[0], cund, None, unds[1], cund]
    for dtype, fill in ((np.float64, np.nan), (np.float32, 9.0)):
        if dtype == np.float32:
            batch, batch_unds = [cb, record_of(ctx, shape, "-", None, 1, seg, np.float32), cn, cb], [cund, None, None, cund]
        else:
            batch, batch_unds = mixed, mixed_unds
        masks = []
        got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, batch, fill, dtype=dtype, masks=masks)
        check_against_loop(got, want_of(batch, batch_unds, dtype, fill))
        for f, und in enumerate(batch_unds):
            want_count = 0 if und is None else sum(int(mc.coarse_und(und, bc.single(case, i)).sum()) for i in range(len(rois)))
            assert masks[f]["undefined"] == want_count
        for f, rec in enumerate(batch):
            if rec is cb:
                for i in range(len(rois)):
                    assert np.array_equal(ints(got[f][i]), ints(np.where(mc.coarse_und(cund, bc.single(case, i)), dtype(fill), dtype(2.5))))
            if rec is cn:
                assert all((g == -7.0).all() for g in got[f])
    # the device form
    buf = ctx.to_device(np.full(len(mixed) * T, SENTINEL))
    try:
        ctx.decode_seg_rois_batch_masked(buf, zyx(shape), level, rois, mixed, np.nan)
        flat = buf.download(np.float64, len(mixed) * T)
    finally:
        buf.free()
    check_against_loop([[flat[f * T + offs[i]:f * T + offs[i + 1]].reshape(api.roi_shape(r)) for i, r in enumerate(rois)] for f in range(len(mixed))],
                       want_of(mixed, mixed_unds, np.float64, np.nan))
    # nothing but constant fields: no field part has a job, the masks still ride in a launch and the host caller gets its buffer
    only = [cb, cn, cb]
    before = api.stat(api.STAT_ROI_CODER_LAUNCHES)
    for dtype in (np.float64, np.float32):
        got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, only, -1.5, dtype=dtype)
        check_against_loop(got, want_of(only, [cund, None, cund], dtype, -1.5))
    assert api.stat(api.STAT_ROI_CODER_LAUNCHES) - before == 2  # (one launch per call)
    got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [cn, cn], -1.5)
    assert all((g == -7.0).all() for row in got for g in row)


def test_one_field_with_six_regions_is_six_single_calls(ctx):
    case = next(c for c in bc.CASES if len(c[2]) == 6)
    shape, level, rois, _, _ = case
    recs, unds = batch_of(ctx, case)
    want, counts = loop_of(ctx, case, np.float64, np.nan)
    for f in (0, 2):  # a WRS1 and a WRS3 field part
        masks = []
        before = api.stat(api.STAT_ROI_CODER_LAUNCHES)
        got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [recs[f]], np.nan, masks=masks)
        assert api.stat(api.STAT_ROI_CODER_LAUNCHES) - before == (2 if f == 2 else 1)
        check_against_loop(got, [want[f]])
        assert masks[0]["undefined"] == counts[f]


def test_a_damaged_mask_segment(ctx):
    """inside a listed segment: WR_ERR_STREAM and the output untouched; inside an unlisted one: the call succeeds; a bad blob
    header on field 2: "field 2: mask blob:", nothing launched"""
    case = next(c for c in bc.CASES if c[0] == mc.GENERAL and c[1] == 0)
    shape, level, rois, _, fields = case
    assert fields[2] != "-"
    recs, _ = batch_of(ctx, case)
    want, _ = loop_of(ctx, case, np.float64, np.nan)
    T = int(bc.offsets(case)[-1])
    rec = recs[2]
    first, seg, lens = mask_front(rec)
    listed = api.mask_roi_segments_multi(zyx(shape), level, rois, seg)
    unlisted = np.setdiff1d(np.arange(len(lens)), listed)
    assert len(unlisted) and len(listed)
    starts = first + np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    stats = (api.STAT_ROI_CODER_LAUNCHES, api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP, api.STAT_ROI_SEGMENTS, api.STAT_ROI_BYTES_UP)
    # an unlisted segment
    data = rec["data"].copy()
    k = int(unlisted[len(unlisted) // 2])
    data[starts[k] + lens[k] // 2] ^= 0x40
    got = ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [recs[0], recs[1], dict(rec, data=data)], np.nan)
    check_against_loop(got, want)
    # a listed segment: the model's counts at the head of its stream
    refused = 0
    buf = ctx.to_device(np.full(3 * T, SENTINEL))
    try:
        for k in listed[:6]:
            data = rec["data"].copy()
            data[starts[k] + 2] ^= 0x40
            out = np.full(3 * T, SENTINEL)
            try:
                ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [recs[0], recs[1], dict(rec, data=data)], np.nan, out=out)
            except api.WaveRangeError as e:
                assert "error -4" in str(e) and "field 2: mask" in str(e)
                assert (out == SENTINEL).all()
                with pytest.raises(api.WaveRangeError):
                    ctx.decode_seg_rois_batch_masked(buf, zyx(shape), level, rois, [recs[0], recs[1], dict(rec, data=data)], np.nan)
                assert (buf.download(np.float64, 3 * T) == SENTINEL).all()
                refused += 1
    finally:
        buf.free()
    assert refused >= 1, "a flipped bit in the model of a listed segment was never noticed"
    # a bad header
    nt = rec["ntot_enc"]
    for name, at in (("magic", nt + 3), ("reserved", nt + 5), ("n", nt + 8)):
        data = rec["data"].copy()
        data[at] ^= 0x01
        out = np.full(3 * T, SENTINEL)
        before = [api.stat(s) for s in stats]
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [recs[0], recs[1], dict(rec, data=data)], np.nan, out=out)
        assert "error -4" in str(e.value) and "field 2: mask blob:" in str(e.value), (name, str(e.value))
        assert [api.stat(s) for s in stats] == before and (out == SENTINEL).all(), name
    for bad in (rec["data"][:-1], np.concatenate([rec["data"], np.zeros(3, np.uint8)])):
        before = [api.stat(s) for s in stats]
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [recs[0], recs[1], dict(rec, data=bad)], np.nan)
        assert "error -4" in str(e.value) and "field 2: mask blob:" in str(e.value)
        assert [api.stat(s) for s in stats] == before
    # the region plans come first, the streams second, the blobs third
    data = rec["data"].copy()
    data[nt + 3] ^= 0x01
    broken = dict(rec, data=data)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois + [((0, 1), (0, 1), (0, 99))], [recs[0], recs[1], broken], np.nan)
    assert "error -1" in str(e.value)
    planes = recs[1]["data"].copy()
    planes[0] ^= 0xFF
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, [broken, dict(recs[1], data=planes), recs[2]], np.nan)
    assert "field 1: " in str(e.value) and "mask blob" not in str(e.value)
    # and the records still decode
    check_against_loop(ctx.decode_host_seg_rois_batch_masked(zyx(shape), level, rois, recs, np.nan), want)
