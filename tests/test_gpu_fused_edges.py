"""The fused transform kernels (csrc/wr_fused.hip) on every remainder of the last tile in x, y and z -- the shape families
of tests/fused_edge_cases.py: pencils of 4k samples along each axis, one-level boxes with nx % 4 == 2 and an odd level-0
remainder (forward) or nx % 8 == 4 and a level-0 remainder of 2 (mod 4) (inverse), the XCD-blocked tile order with a short last column, and boxes whose four fused levels reduce min/max on partial
tiles, with the extremes on the far faces.  Bit for bit against the CPU oracle at the transform level (fp64) and through the
fp32 and fp64 codec; no tolerances.  Every check first asserts through wr_fused_plan that its shape takes the path and has
the remainders it is in the table for.
Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest

import fused_edge_cases as E
from test_gpu_f32 import narrow, roundtrip, same_enc, same_f32
from util import bits_equal

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def api():
    from waverange_amd import api as a
    a.set_verbosity(0)
    return a


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


def differing(got, want, shape_xyz):
    """'' when the bit patterns agree, else how many samples differ and the first few (z, y, x)"""
    nx, ny, nz = shape_xyz
    bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint64).ravel() != np.ascontiguousarray(want).view(np.uint64).ravel())
    if bad.size == 0:
        return ""
    return "%d of %d differ, first at (z, y, x) %s" % (bad.size, got.size, [tuple(int(v) for v in np.unravel_index(b, (nz, ny, nx))) for b in bad[:6]])


def transform_both_ways(ctx, oracle, f, shape_xyz):
    buf = ctx.to_device(f)
    try:
        ctx.transform(buf, f.shape, 4)
        ctx.sync()
        want = oracle.cdf97_3d(f, 4)
        bad = differing(buf.download(np.float64, f.size), want, shape_xyz)
        assert not bad, ("fwd", shape_xyz, sorted(E.classes(shape_xyz), key=repr), bad)
        # the inverse on the oracle's coefficients: it does not depend on what the forward kernels left
        buf.upload(want)
        ctx.transform(buf, f.shape, -4)
        ctx.sync()
        bad = differing(buf.download(np.float64, f.size), oracle.cdf97_3d(want, -4), shape_xyz)
        assert not bad, ("inv", shape_xyz, sorted(E.classes(shape_xyz), key=repr), bad)
    finally:
        buf.free()


def same_as_oracle(enc, want):
    """header scalars as bit patterns, every deps_vec / minval_vec entry bit for bit, plane lengths, every coded byte"""
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(enc[k]).hex() == float(want[k]).hex(), k
    same_enc(enc, want)


def fp32_codec(api, ctx, oracle, f):
    want = oracle.encode(f.astype(np.float64), TOL)
    enc, rec, rec2 = roundtrip(api, ctx, f, dict(tolrel=TOL, wtflag=1))   # (checks that the input is left untouched)
    same_as_oracle(enc, want)
    expect = narrow(oracle.decode(want, f.shape))
    assert same_f32(rec, expect), "decode_host_f32 differs from (float) of the fp64 reconstruction"
    assert same_f32(rec2, expect), "decode_begin + decode_finish_host_f32 differs"


TRANSFORM_ITEMS = ([("X", s) for s in E.slices("X", 25)] + [("Y", s) for s in E.slices("Y", 19)] + [("Z", s) for s in E.slices("Z", 19)]
                   + [("X1", s) for s in E.slices("X1", 1)] + [("XI1", s) for s in E.slices("XI1", 1)] + [("XCD", s) for s in E.slices("XCD", 1)]
                   + [("MM", s) for s in E.slices("MM", 11)])
F32_ITEMS = ([("X", s) for s in E.slices("X", 16)] + [("X1", s) for s in E.slices("X1", 1)] + [("XI1", s) for s in E.slices("XI1", 1)]
             + [("XCD", s) for s in E.slices("XCD", 1)] + [("MM", s) for s in E.slices("MM", 4)])


def item_id(item):
    return item[0] + "-" + E.slice_id(item[1])


def test_every_shape_of_the_table_is_run():
    assert sorted({s for _, sl in TRANSFORM_ITEMS for s in sl}) == E.SHAPES
    assert sorted({s for _, sl in F32_ITEMS for s in sl}) == sorted({s for fam in E.F32_FAMILIES for s in E.FAMILIES[fam]})


@pytest.mark.parametrize("item", TRANSFORM_ITEMS, ids=item_id)
def test_transform_vs_oracle(api, ctx, oracle, item):
    for shape in item[1]:
        E.check_plan(api, shape)
        transform_both_ways(ctx, oracle, E.field(shape), shape)


@pytest.mark.parametrize("item", F32_ITEMS, ids=item_id)
def test_fp32_codec_vs_oracle(api, ctx, oracle, item):
    """level 0 of the forward reads fp32 rows as float2 into registers (8-byte aligned rows where nx % 4 == 2), level 0 of the
    inverse narrows in its stores"""
    for shape in item[1]:
        E.check_plan(api, shape)
        fp32_codec(api, ctx, oracle, E.field(shape).astype(np.float32))


@pytest.mark.parametrize("case", E.MM_FIELDS, ids=lambda c: E.ident(c[0]) + "-" + c[1])
def test_minmax_on_partial_tiles(api, ctx, oracle, case):
    """All four levels fused: the forward kernels reduce the field's and the coefficient array's min/max on the way (MM_IN,
    MM_OUT, k_minmax_final4).  The field's extremes lie in the last pairs of the far faces; with the larger factor the
    extremes of the coefficient array do too (tests/test_fused_edge_cases_cpu.py).  midval, halfspanval and tolabs come from
    the first, deps_vec[0] / minval_vec[0] from the second."""
    shape, axis = case
    E.check_plan(api, shape)
    assert E.TABLE[shape]["fwd"][:2] == (4, True)
    for factor in E.FACE_FACTORS:
        f = E.face_field(shape, axis, factor)
        want = oracle.encode(f, TOL)
        assert want["nlay"] >= 1
        enc, _ = ctx.encode_host(f, TOL)
        enc["data"] = enc["data"].copy()
        same_as_oracle(enc, want)
        rec = np.full(f.shape, -1.0)
        ctx.decode_host(rec, enc)
        assert bits_equal(rec, oracle.decode(want, f.shape)), factor
        # fp32: the same extremes narrowed (still unique, still outside the field)
        fp32_codec(api, ctx, oracle, E.face_field(shape, axis, factor, np.float32))
