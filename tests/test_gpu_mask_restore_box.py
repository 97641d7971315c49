"""k_mask_restore_box alone, through the stage call wr_dev_mask_restore_box / _f32: over the case table of masked_roi_cases.py,
fp64 and fp32, three undefined sets (the masked codec's recipe, isolated bits, every sample of the region), the output prefilled
with a sentinel and compared as integers with the numpy definition out[coarse mask] = fill, guard elements on both sides, the
count against numpy's.  Each case runs with the mask plane at byte 0 of its buffer and the output 1 element in, and with the
mask plane at byte 3 (no wide load is aligned), the output 3 elements in, and every byte of the plane outside the listed
segments (api.mask_roi_segments) set to 0xFF: the kernel reads none of them, so the result is the same.  Then every one-sample
region of 13 x 9 x 7 at level 0, and the one-sample regions along the three axes through the centre of 33 x 17 x 9 at every
level."""
import numpy as np
import pytest

import masked_roi_cases as mc
from waverange_amd import api

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 12345.5, 4242.0


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def ints(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def garbage_outside(plane, case):
    """the plane with 0xFF in every byte of a segment the case's region does not list"""
    shape, level, roi, _ = case
    nx, ny, nz = shape
    seg = mc.seg_len(case)
    listed = np.zeros(-(-plane.size // seg), bool)
    listed[api.mask_roi_segments((nz, ny, nx), level, roi, case[3])] = True
    out = plane.copy()
    out[~np.repeat(listed, seg)[:plane.size]] = 0xFF
    return out


def run(ctx, case, und, dtype, fill, off, boff, plane):
    """(output with its guards, count) of one stage call"""
    shape, level, roi, _ = case
    nx, ny, nz = shape
    nbox = int(np.prod(mc.out_shape(case)))
    host = np.concatenate([np.full(off, GUARD, dtype), np.full(nbox, SENTINEL, dtype), np.full(1, GUARD, dtype)])
    buf = ctx.to_device(host)
    bits = ctx.to_device(np.concatenate([np.full(boff, 0xA5, np.uint8), plane, np.full(16, 0xA5, np.uint8)]))
    try:
        count = ctx.mask_restore_box(buf, (nz, ny, nx), level, roi, bits, fill, dtype=dtype, offset=off, bits_offset=boff)
        got = buf.download(dtype, host.size)
    finally:
        buf.free()
        bits.free()
    return got, count


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_restore_box_is_the_numpy_definition(ctx, case, dtype):
    shape = case[0]
    for name, und in (("recipe", mc.und_recipe(shape)), ("isolated", mc.und_isolated(shape)), ("region", mc.und_region(case))):
        coarse = mc.coarse_und(und, case).reshape(-1)
        plane = mc.packed(und)
        for fill, off, boff, p in ((np.nan, 1, 0, plane), (-77.25, 3, 3, garbage_outside(plane, case))):
            got, count = run(ctx, case, und, dtype, fill, off, boff, p)
            want = np.concatenate([np.full(off, GUARD, dtype), np.where(coarse, dtype(fill), dtype(SENTINEL)), np.full(1, GUARD, dtype)])
            assert np.array_equal(ints(got), ints(want)), (name, fill)
            assert count == int(coarse.sum()), (name, fill)
        if name == "region":
            assert coarse.all()


def sweep(ctx, shape, level, und, regions):
    """one-sample regions against the mask, one stage call each; the output element is reset only when a call wrote it"""
    nx, ny, nz = shape
    bits = ctx.to_device(np.concatenate([mc.packed(und), np.zeros(16, np.uint8)]))
    fresh = np.array([GUARD, SENTINEL, GUARD])
    buf = ctx.to_device(fresh)
    s = 1 << level
    try:
        for k, (x, y, z) in enumerate(regions):
            roi = ((z, z + 1), (y, y + 1), (x, x + 1))
            fill = float(k + 1)
            count = ctx.mask_restore_box(buf, (nz, ny, nx), level, roi, bits, fill, offset=1)
            got = buf.download(np.float64, 3)
            hit = bool(und[z * s, y * s, x * s])
            assert count == int(hit), (level, x, y, z)
            assert got.tolist() == [GUARD, fill if hit else SENTINEL, GUARD], (level, x, y, z)
            if hit:
                buf.upload(fresh)
    finally:
        buf.free()
        bits.free()


def test_every_one_sample_region_at_level_0(ctx):
    nx, ny, nz = mc.ODD
    sweep(ctx, mc.ODD, 0, mc.und_recipe(mc.ODD), [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx)])


@pytest.mark.parametrize("level", range(5))
def test_one_sample_regions_along_the_axes_through_the_centre(ctx, level):
    bx, by, bz = mc.box_of(mc.CHAIN, level)
    cx, cy, cz = bx // 2, by // 2, bz // 2
    regions = [(x, cy, cz) for x in range(bx)] + [(cx, y, cz) for y in range(by)] + [(cx, cy, z) for z in range(bz)]
    sweep(ctx, mc.CHAIN, level, mc.und_recipe(mc.CHAIN), regions)


def test_refused_arguments(ctx):
    nx, ny, nz = mc.CHAIN
    buf = ctx.to_device(np.full(64, SENTINEL))
    bits = ctx.to_device(np.zeros(mc.nsym_of(mc.CHAIN) + 16, np.uint8))
    try:
        for level, roi in [(5, None), (4, ((0, 1), (0, 2), (0, 4))), (0, ((0, 1), (3, 3), (0, 4)))]:
            with pytest.raises(api.WaveRangeError) as e:
                ctx.mask_restore_box(buf, (nz, ny, nx), level, roi, bits, 1.0)
            assert "error -1" in str(e.value)
        assert (buf.download(np.float64, 64) == SENTINEL).all()
    finally:
        buf.free()
        bits.free()
