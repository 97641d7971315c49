"""The fused transform kernels (csrc/wr_fused.hip) on the launch geometries of tests/fused_cases.py -- exactly one fused
level (slabs, either side of the 2^21 threshold, forward fused with the inverse general), pencils with many tiles or z
segments, long z segments that end on a shorter one, the smallest fused boxes -- and fp64 edge-value fields (subnormals, the
reference's triviality rule, huge values, a large offset), bit for bit against the CPU oracle at the transform level and
through the fp64 and fp32 codec.  Every test first asserts through wr_fused_plan that its shape takes the path it is there for.
Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest

import fused_cases as F
from test_gpu_f32 import narrow, roundtrip, same_enc, same_f32
from util import bits_equal
from waverange_amd import synth

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


def same_as_oracle(enc, want):
    """header scalars as bit patterns, plane lengths, every coded byte"""
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(enc[k]).hex() == float(want[k]).hex(), k
    same_enc(enc, want)


def field(shape):
    nx, ny, nz = shape
    return synth.field(nx, ny, nz, seed=nx * 131 + ny)


def transform_both_ways(ctx, oracle, f, lvl, tag):
    buf = ctx.to_device(f)
    ctx.transform(buf, f.shape, lvl)
    ctx.sync()
    want = oracle.cdf97_3d(f, lvl)
    assert bits_equal(buf.download(np.float64, f.size), want), ("fwd", tag, lvl)
    # the inverse on the oracle's coefficients: it does not depend on what the forward kernels left
    buf.upload(want)
    ctx.transform(buf, f.shape, -lvl)
    ctx.sync()
    assert bits_equal(buf.download(np.float64, f.size), oracle.cdf97_3d(want, -lvl)), ("inv", tag, lvl)
    buf.free()


@pytest.mark.parametrize("shape", F.SHAPES, ids=F.ident)
def test_transform_vs_oracle(api, ctx, oracle, shape):
    F.check_plan(api, shape)
    transform_both_ways(ctx, oracle, field(shape), 4, shape)


def test_three_level_transform_vs_oracle(api, ctx, oracle):
    """levels 1, 2 and 4 are run by test_gpu_parity.py; a three-level transform never takes the fused path"""
    shape = (258, 130, 66)
    F.check_plan(api, shape)
    transform_both_ways(ctx, oracle, field(shape), 3, shape)


@pytest.mark.parametrize("shape", F.SHAPES, ids=F.ident)
def test_fp64_codec_vs_oracle(api, ctx, oracle, shape):
    F.check_plan(api, shape)
    f = field(shape)
    want = oracle.encode(f, TOL)
    expect = oracle.decode(want, f.shape)
    src = f.copy()
    enc, _ = ctx.encode_host(src, TOL)
    enc["data"] = enc["data"].copy()
    assert bits_equal(src, f), "encode_host must not write the field"
    same_as_oracle(enc, want)
    rec = np.full_like(f, -1.0)
    ctx.decode_host(rec, enc)
    assert bits_equal(rec, expect)
    if shape not in F.ONE_LEVEL:
        return
    # field resident on the device, the residual in wavelet space left in it (what the reference leaves in fld_1d)
    buf = ctx.to_device(f)
    ctx.set_keep_residual(True)
    try:
        enc_d, _ = ctx.encode(buf, f.shape, TOL)
        resid = buf.download(np.float64, f.size)
    finally:
        ctx.set_keep_residual(False)
    same_as_oracle(enc_d, want)
    assert bits_equal(resid, want["residual"])
    enc_d["data"] = enc_d["data"].copy()
    ctx.decode(buf, f.shape, enc_d)
    assert bits_equal(buf.download(np.float64, f.size), expect)
    buf.free()


@pytest.mark.parametrize("shape", F.SHAPES, ids=F.ident)
def test_fp32_codec_vs_oracle(api, ctx, oracle, shape):
    F.check_plan(api, shape)
    f = field(shape).astype(np.float32)
    want = oracle.encode(f.astype(np.float64), TOL)
    enc, rec, rec2 = roundtrip(api, ctx, f, dict(tolrel=TOL, wtflag=1))   # (checks that the input is left untouched)
    same_as_oracle(enc, want)
    expect = narrow(oracle.decode(want, f.shape))
    assert same_f32(rec, expect), "decode_host_f32 differs from (float) of the fp64 reconstruction"
    assert same_f32(rec2, expect), "decode_begin + decode_finish_host_f32 differs"


def test_zero_minimum_on_the_one_level_path(api, ctx, oracle):
    """One fused level: min/max come from the stand-alone reductions, not from the forward kernels.  The sign of a zero
    minimum is the sign of the LAST zero in memory order (it shows in midval / minval_vec); here it is -0.0."""
    shape = (512, 512, 8)
    F.check_plan(api, shape)
    nx, ny, nz = shape
    f = np.abs(synth.field(nx, ny, nz, seed=8)) + 0.25
    flat = f.reshape(-1)
    pos = np.sort(np.random.RandomState(nx).choice(flat.size, 3, replace=False))
    flat[pos] = [-0.0, 0.0, -0.0]
    want = oracle.encode(f, TOL)
    omn, omx = oracle.minmax(f)
    assert omn == 0 and np.signbit(omn), "the case is meant to have the minimum -0.0"
    buf = ctx.to_device(f)
    mn, mx = ctx.minmax(buf, f.size)
    assert mn == 0 and np.signbit(mn) and mx == omx
    enc, _ = ctx.encode(buf, f.shape, TOL)
    buf.free()
    assert float(enc["midval"]).hex() == float(want["midval"]).hex()
    assert bits_equal(enc["minval_vec"], want["minval_vec"]) and bits_equal(enc["deps_vec"], want["deps_vec"])
    assert np.array_equal(enc["data"], want["data"])


@pytest.mark.parametrize("name", F.EDGE_FIELDS)
@pytest.mark.parametrize("shape", sorted(F.EDGE_SHAPES), ids=F.ident)
def test_fp64_edge_fields(api, ctx, oracle, shape, name):
    F.check_plan(api, shape, F.EDGE_SHAPES[shape])
    f = F.edge_field(shape, name)
    F.check_edge_input(f, name)
    buf = ctx.to_device(f)
    got, omm = ctx.minmax(buf, f.size), oracle.minmax(f)
    buf.free()
    assert bits_equal(got, omm), (got, omm)
    want = oracle.encode(f, F.EDGE_TOL)
    enc, _ = ctx.encode_host(f, F.EDGE_TOL)
    enc["data"] = enc["data"].copy()
    same_as_oracle(enc, want)
    expect = oracle.decode(want, f.shape)
    rec = np.full(f.shape, -1.0)
    ctx.decode_host(rec, enc)
    assert bits_equal(rec, expect)
    if name == "below":
        # trivial by the reference's rule: nothing coded, header scalars nonzero subnormals, the decode is the constant midval
        assert (enc["nlay"], enc["ntot_enc"]) == (0, 0)
        assert 0 < enc["halfspanval"] <= 2 * F.TINY and 0 < abs(enc["midval"]) < F.TINY
        assert bits_equal(rec, np.full(f.shape, enc["midval"]))
    elif name in F.SUBNORMAL_FIELDS:
        assert enc["nlay"] == 8
        assert np.count_nonzero((rec != 0) & (np.abs(rec) < F.TINY)) > 0, "subnormals must survive"
        # the same with the field resident on the device and the residual kept (the quantizer kernels that write it back)
        buf = ctx.to_device(f)
        ctx.set_keep_residual(True)
        try:
            enc_d, _ = ctx.encode(buf, f.shape, F.EDGE_TOL)
            resid = buf.download(np.float64, f.size)
        finally:
            ctx.set_keep_residual(False)
        buf.free()
        same_as_oracle(enc_d, want)
        assert bits_equal(resid, want["residual"])


@pytest.mark.parametrize("n", [7, 100003])
def test_quantizer_plane_of_subnormals(ctx, oracle, n):
    """A residual of subnormals: deps < 2^-1024, so aopt = 1 / deps is infinite and aopt * x + bopt is +inf or NaN.  The
    reference's x86-64 builds turn both into the byte 0 (the oracle does, and tests/test_edge_fields_cpu.py holds the compiled
    reference to the same outputs); a saturating conversion would give 255 for +inf.  Next to it a deps whose reciprocal is
    still finite (subnormals then fall into the first few quantizer steps)."""
    x = np.random.RandomState(n).randint(-7, 8, n) * (F.TINY / 8)   # all subnormal or zero
    lo, hi = oracle.minmax(x)
    for deps in ((hi - lo) / 255.0, F.TINY * 0.51):
        with np.errstate(over="ignore"):
            assert np.isinf(np.float64(1.0) / np.float64(deps)) == (deps < 2.0 ** -1024)
        q_want, r_want = oracle.quantize_plane(x, deps, lo)
        buf = ctx.to_device(x)
        qbuf = ctx.alloc(n + 16)
        nlo, nhi = ctx.quantize_plane(buf, n, deps, lo, qbuf)
        assert np.array_equal(qbuf.download(np.uint8, n), q_want)
        assert bits_equal(buf.download(np.float64, n), r_want)
        assert bits_equal((nlo, nhi), oracle.minmax(r_want))
        buf.free()
        qbuf.free()
