"""k_mask_restore_boxes alone, through the stage call wr_dev_mask_restore_boxes / _f32: over the case table of
masked_roi_batch_cases.py, fp64 and fp32.  The output buffer holds nfields parts of T elements of distinct values between two
guard bands; per item (field that has a mask, region) the result is numpy's where(coarse mask, fill, before), everything else
-- the unmasked fields' parts, both guard bands -- is unchanged, compared as integers over the whole buffer; the counts are
numpy's per field.  Each case runs with the output and the mask planes 1, 4 and 8 bytes off alignment; in the first run every
byte of a plane that holds no bit of a region is 0xFF: the kernel reads none of them, so the result is the same."""
import numpy as np
import pytest

import masked_roi_batch_cases as bc
import masked_roi_cases as mc
from waverange_amd import api

pytestmark = pytest.mark.gpu

GUARD_ELEMS = 64


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


def garbage_where_unread(plane, case):
    """the plane with 0xFF in every byte that holds no bit of a region of the case"""
    reads = set()
    for i in range(len(case[2])):
        reads |= mc.kernel_reads(bc.single(case, i))
    keep = np.zeros(plane.size, bool)
    keep[sorted(reads)] = True
    return np.where(keep, plane, np.uint8(0xFF))


_planes = {}


def planes_of(case, garbage):
    key = (bc.case_id(case), garbage)
    if key not in _planes:
        out = []
        for f in range(len(case[4])):
            und = bc.und_of(case, f)
            p = None if und is None else mc.packed(und)
            out.append(p if p is None or not garbage else garbage_where_unread(p, case))
        _planes[key] = out
    return _planes[key]


def expected(case, before, fill, dtype):
    """(the nfields * T elements behind the call, the per-field counts)"""
    offs = bc.offsets(case)
    T = int(offs[-1])
    want = before.copy()
    counts = []
    for f in range(len(case[4])):
        und = bc.und_of(case, f)
        count = 0
        if und is not None:
            for i in range(len(case[2])):
                coarse = mc.coarse_und(und, bc.single(case, i)).reshape(-1)
                part = want[f * T + offs[i]:f * T + offs[i + 1]]
                part[coarse] = dtype(fill)
                count += int(coarse.sum())
        counts.append(count)
    return want, counts


def run(ctx, case, dtype, fill, skew, planes):
    shape, level, rois, _, fields = case
    nf, T = len(fields), int(bc.offsets(case)[-1])
    item = np.dtype(dtype).itemsize
    before = (np.arange(nf * T, dtype=np.float64) * 0.5 + 1.0).astype(dtype)
    guard = np.full(GUARD_ELEMS, 12345.5, dtype)
    host = np.concatenate([np.zeros(skew, np.uint8), guard.view(np.uint8), before.view(np.uint8), guard.view(np.uint8)])
    buf = ctx.to_device(host)
    bits = [None if p is None else ctx.to_device(np.concatenate([np.full(skew, 0xA5, np.uint8), p, np.full(16, 0xA5, np.uint8)])) for p in planes]
    try:
        counts = ctx.mask_restore_boxes(buf, nf, zyx(shape), level, rois, bits, fill, dtype=dtype, offset=GUARD_ELEMS, bits_offset=skew, byte_offset=skew)
        got = buf.download(np.uint8, host.size)
    finally:
        buf.free()
        for b in bits:
            if b is not None:
                b.free()
    assert np.array_equal(got[:skew], host[:skew])
    elems = got[skew:].view(dtype)
    assert np.array_equal(ints(elems[:GUARD_ELEMS]), ints(guard)) and np.array_equal(ints(elems[-GUARD_ELEMS:]), ints(guard))
    return before, elems[GUARD_ELEMS:-GUARD_ELEMS], counts


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_restore_boxes_is_the_numpy_definition(ctx, case, dtype):
    offs = bc.offsets(case)
    T = int(offs[-1])
    for skew, fill, garbage in ((1, np.nan, True), (4, -77.25, False), (8, np.nan, False)):
        before, got, counts = run(ctx, case, dtype, fill, skew, planes_of(case, garbage))
        want, want_counts = expected(case, before, fill, dtype)
        assert counts == want_counts, (skew, counts, want_counts)
        for f in range(len(case[4])):  # per item first, so that a failure names it
            for i in range(len(case[2])):
                a, b = f * T + int(offs[i]), f * T + int(offs[i + 1])
                assert np.array_equal(ints(got[a:b]), ints(want[a:b])), (skew, "field", f, "region", i)
        assert np.array_equal(ints(got), ints(want))
        for f, k in enumerate(case[4]):
            if k == "-":
                assert np.array_equal(ints(got[f * T:(f + 1) * T]), ints(before[f * T:(f + 1) * T])) and counts[f] == 0


def test_it_equals_the_single_box_call_item_by_item(ctx):
    case = bc.CASES[0]
    shape, level, rois, _, fields = case
    offs = bc.offsets(case)
    nf, T = len(fields), int(offs[-1])
    before = np.arange(nf * T, dtype=np.float64) + 0.25
    planes = planes_of(case, False)
    bits = [None if p is None else ctx.to_device(np.concatenate([p, np.zeros(16, np.uint8)])) for p in planes]
    a, b = ctx.to_device(before), ctx.to_device(before)
    try:
        counts = ctx.mask_restore_boxes(a, nf, zyx(shape), level, rois, bits, -3.5)
        singles = [0] * nf
        for f in range(nf):
            if bits[f] is None:
                continue
            for i, roi in enumerate(rois):
                singles[f] += ctx.mask_restore_box(b, zyx(shape), level, roi, bits[f], -3.5, offset=f * T + int(offs[i]))
        assert counts == singles
        assert np.array_equal(ints(a.download(np.float64, nf * T)), ints(b.download(np.float64, nf * T)))
    finally:
        for d in [a, b] + [x for x in bits if x is not None]:
            d.free()


def test_no_field_has_a_plane_and_refused_arguments(ctx):
    nx, ny, nz = mc.CHAIN
    rois = [((0, 1), (0, 2), (0, 3))]
    buf = ctx.to_device(np.full(64, 4242.0))
    bits = ctx.to_device(np.full(mc.nsym_of(mc.CHAIN) + 16, 0xFF, np.uint8))
    try:
        assert ctx.mask_restore_boxes(buf, 3, (nz, ny, nx), 4, rois, [None, None, None], 1.0) == [0, 0, 0]
        for level, rr, nf in [(5, rois, 1), (4, [((0, 1), (0, 2), (0, 4))], 1), (4, [], 1), (0, [((0, 1), (3, 3), (0, 4))], 1), (4, rois, 0)]:
            with pytest.raises(api.WaveRangeError) as e:
                ctx.mask_restore_boxes(buf, nf, (nz, ny, nx), level, rr, [bits] * nf, 1.0)
            assert "error -1" in str(e.value)
        assert (buf.download(np.float64, 64) == 4242.0).all()
        assert ctx.mask_restore_boxes(buf, 2, (nz, ny, nx), 4, rois, [None, bits], 1.0) == [0, 6]
        got = buf.download(np.float64, 64)
        assert (got[:6] == 4242.0).all() and (got[6:12] == 1.0).all() and (got[12:] == 4242.0).all()
    finally:
        buf.free()
        bits.free()
