"""Encode to a byte budget on the GPU (include/waverange_amd.h): the size probe against the host bound of the oracle-quantized
plane, integer for integer, and the driver against B(g) computed on the CPU (tests/budget_ref.py) -- every budget and every
verdict comes from there, so the reference alone decides.  No tolerance appears anywhere: bounds are equal integers, streams
are equal bytes, reconstructions equal bits.

The shapes are the smallest that reach every path of the probe kernel:
  (40, 36, 33)  seg 1024     a short last segment (416 symbols), partial groups of a wave
  (39, 37, 33)  seg 1024     an odd element count: the last pair of a segment is half a pair
  (64, 64, 64)  the default  5 segments, the last short
  (16, 16, 16)  59904        n < seg
  (64, 64, 32)  seg 16       n a multiple of seg; 8192 segments, more than one per workgroup"""
import numpy as np
import pytest

from budget_ref import BudgetRef
from util import bits_equal
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

CASES = [((40, 36, 33), 1024), ((39, 37, 33), 1024), ((64, 64, 64), 0), ((16, 16, 16), 59904), ((64, 64, 32), 16)]
KINDS = ["smooth", "noise"]
HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")
BIG = 1 << 40


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def make_field(kind, dims, seed=3):
    nx, ny, nz = dims
    if kind == "smooth":
        return synth.field(nx, ny, nz, seed=seed)
    idx = np.arange(nx * ny * nz, dtype=np.uint64)
    r = (synth.splitmix64(seed, idx) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.ascontiguousarray((r - 0.25).reshape(nz, ny, nx))


_REFS = {}


def ref_of(kind, dims, seg):
    """(field, BudgetRef, oracle) of a case; made once, shared, never written to"""
    key = (kind, dims, seg)
    if key not in _REFS:
        o = Oracle()
        f = make_field(kind, dims)
        f.flags.writeable = False
        _REFS[key] = (f, BudgetRef(o, f, seg), o)
    return _REFS[key]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- the stage calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,seg", CASES, ids=case_id)
def test_probe_and_plane_bound_equal_the_host_bound(ctx, dims, seg, kind):
    f, ref, o = ref_of(kind, dims, seg)
    g = api.budget_index(1e-6)
    planes = ref.planes(g)
    assert len(planes) >= 3
    for l, (q, deps, lo) in enumerate(planes):
        want = api.seg_size_bound_host_ref(q, seg)
        assert ctx.plane_size_bound(q, seg) == want, (l, "plane of symbols")
        assert ctx.quant_size_probe(ref.resid[l], lo, [deps], seg) == [want], (l, "one candidate")
    # K candidates in one pass: plane 1 cut with the full step and with the steps of grid points around its interval
    l = 1
    lo, hi = ref.range[l]
    a, b = ref.last_interval(l)
    steps = [(hi - lo) / 255.0] + [ref.tolabs(gk) for gk in np.linspace(a, b, api.BUDGET_PROBE_MAX - 1).astype(int)]
    assert len(steps) == api.BUDGET_PROBE_MAX
    want = [api.seg_size_bound_host_ref(o.quantize_plane(ref.resid[l], d, lo)[0], seg) for d in steps]
    assert ctx.quant_size_probe(ref.resid[l], lo, steps, seg) == want
    assert ctx.quant_size_probe(ref.resid[l], lo, steps[::-1], seg) == want[::-1]
    for bad in ([], steps + [steps[0]]):  # none, and K + 1
        with pytest.raises(api.WaveRangeError) as e:
            ctx.quant_size_probe(ref.resid[l], lo, bad, seg)
        assert "error -1:" in str(e.value), str(e.value)  # WR_ERR_ARG


def test_stage_calls_refuse_bad_arguments(ctx):
    q = np.zeros(64, np.uint8)
    for seg in (8, 17, 60000):
        with pytest.raises(api.WaveRangeError):
            ctx.plane_size_bound(q, seg)
        with pytest.raises(api.WaveRangeError):
            ctx.quant_size_probe(np.zeros(64), 0.0, [1.0], seg)
    assert ctx.plane_size_bound(np.zeros(0, np.uint8), 16) == 12


# ---- the driver --------------------------------------------------------------------------------------------------------------
def check_call(ctx, kind, dims, seg, max_bytes, g_min=0, encode=None):
    """One budget call checked against the Python B: fits, tight, the same stream as the plain call at the chosen tolerance, the
    oracle's reconstruction, every plane coded once.  Returns the result record."""
    f, ref, o = ref_of(kind, dims, seg)
    before = api.stat(api.STAT_BUDGET_CODER_RUNS)
    if encode is None:
        info, data, res = ctx.encode_host_seg_budget(f, max_bytes, tol_min=api.budget_tol(g_min), seg=seg)
    else:
        info, data, res = encode(f, max_bytes, api.budget_tol(g_min), seg)
    grew = api.stat(api.STAT_BUDGET_CODER_RUNS) - before
    g = res["g"]
    what = (kind, dims, seg, max_bytes, g_min, g)
    assert g_min <= g <= api.BUDGET_GMAX and res["tolrel"] == api.budget_tol(g), what
    # fits
    assert ref.B(g) <= max_bytes and res["bound"] == ref.B(g) and info["ntot_enc"] <= ref.B(g), (what, ref.B(g), res["bound"], info["ntot_enc"])
    assert data.size == info["ntot_enc"]
    # tight
    assert g == g_min or ref.B(g - 1) > max_bytes, (what, ref.B(g - 1))
    # the same stream
    plain, _ = ctx.encode_host_seg(f, api.budget_tol(g), seg=seg)
    for k in HEADER_KEYS:
        assert info[k] == plain[k], (what, k)
    assert info["nlay"] == ref.nlay(g), what
    assert list(info["len_enc_vec"]) == list(plain["len_enc_vec"]), what
    assert bits_equal(info["deps_vec"], plain["deps_vec"]) and bits_equal(info["minval_vec"], plain["minval_vec"]), what
    assert np.array_equal(data, plain["data"]), what
    # the oracle's reconstruction
    rec = np.empty(f.shape, dtype=np.float64)
    ctx.decode_host_seg(rec, info)
    assert bits_equal(rec, o.decode(o.encode(f, api.budget_tol(g)), f.shape)), what
    # each plane coded once
    assert grew == info["nlay"], (what, grew)
    assert res["probe_passes"] >= 1
    return res


def budgets_of(ref):
    """the budgets the issue names, all from the Python B: {name: max_bytes}"""
    a0, b0 = ref.last_interval(0)
    a1, b1 = ref.last_interval(1)
    a2, b2 = ref.last_interval(2)
    out = {
        # (B is not monotone: where the middle of plane 0's interval costs less than the grid's end, no budget below the end's is served)
        "inside plane 0": max(ref.B((a0 + b0) // 2), ref.B(api.BUDGET_GMAX)),
        "inside plane 2": ref.B((a2 + b2) // 2),
        "coarsest point of plane 1": ref.B(b1),  # the plane-count boundary: one point coarser and plane 0 is the last
        "finest point of plane 1": ref.B(a1),    # the other side: one point finer and there are three planes
    }
    return out


@pytest.mark.parametrize("name", ["inside plane 0", "inside plane 2", "coarsest point of plane 1", "finest point of plane 1"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,seg", CASES, ids=case_id)
def test_driver_at_budgets_from_the_python_B(ctx, dims, seg, kind, name):
    _, ref, _ = ref_of(kind, dims, seg)
    res = check_call(ctx, kind, dims, seg, budgets_of(ref)[name])
    nlay = ref.nlay(res["g"])
    assert nlay == {"inside plane 0": 1, "inside plane 2": 3}.get(name, nlay), (name, res)
    if name == "finest point of plane 1":  # one point finer costs a whole plane more: the boundary itself is the answer
        a1 = ref.last_interval(1)[0]
        assert ref.B(a1 - 1) > ref.B(a1) and res["g"] >= a1 and nlay <= 2, (name, res)


def record_point(ref):
    """An interior g of plane 1's interval that costs less than every finer point at which plane 1 is still the last (B is far
    from monotone on a smooth field, so not every g is like that).  No tight point of the budget B(g) is then finer than g,
    and none of the budget B(g) - 1 is g or finer.  Also returns whether every coarser point of the grid costs less than g: then
    g is the one tight point of B(g)."""
    a1, b1 = ref.last_interval(1)
    B = [ref.B(g) for g in range(a1, api.BUDGET_GMAX + 1)]
    for g in sorted(range(a1 + 1, b1), key=lambda g: abs(g - (a1 + b1) // 2)):
        if min(B[:g - a1]) > B[g - a1]:
            return g, B[g - a1] > max(B[g - a1 + 1:])
    raise AssertionError("no such point")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,seg", CASES, ids=case_id)
def test_driver_one_byte_decides(ctx, dims, seg, kind):
    """B(g) and B(g) - 1 for an interior g: the first returns a point that fits, the second a coarser one"""
    _, ref, _ = ref_of(kind, dims, seg)
    g, unique = record_point(ref)
    assert ref.B(ref.last_interval(2)[1]) > ref.B(g)  # (three planes cost more still)
    first = check_call(ctx, kind, dims, seg, ref.B(g))
    second = check_call(ctx, kind, dims, seg, ref.B(g) - 1)
    assert first["g"] >= g and second["g"] > g, (g, first, second)
    if unique:
        assert first["g"] == g, (g, first)


@pytest.mark.parametrize("dims,seg", CASES, ids=case_id)
def test_driver_generous_budget_returns_g_min(ctx, dims, seg):
    for tol in (1e-2, 1e-5):
        g_min = api.budget_index(tol)
        res = check_call(ctx, "smooth", dims, seg, BIG, g_min)
        assert res["g"] == g_min


def test_driver_budget_below_the_floor(ctx):
    dims, seg = (40, 36, 33), 1024
    f, ref, _ = ref_of("smooth", dims, seg)
    floor = ref.B(api.BUDGET_GMAX)
    out = np.full(ctx._seg_cap(f.shape, seg), 0xAB, np.uint8)
    before = api.stat(api.STAT_BUDGET_CODER_RUNS)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_budget(f, floor - 1, seg=seg, out=out)
    assert "error %d:" % api.ERR_BUDGET in str(e.value) and str(floor) in str(e.value), str(e.value)
    assert np.all(out == 0xAB)
    assert api.stat(api.STAT_BUDGET_CODER_RUNS) == before
    res = check_call(ctx, "smooth", dims, seg, floor)  # the budget the message names does
    assert ref.B(res["g"]) <= floor


def test_driver_constant_field(ctx):
    f = np.full((8, 8, 16), 2.5)
    g_min = api.budget_index(1e-4)
    info, data, res = ctx.encode_host_seg_budget(f, 1, tol_min=1e-4, seg=1024)
    assert info["nlay"] == 0 and info["ntot_enc"] == 0 and data.size == 0
    assert res["g"] == g_min and res["bound"] == 0 and res["tolrel"] == api.budget_tol(g_min)
    rec = np.empty_like(f)
    ctx.decode_host_seg(rec, info)
    assert bits_equal(rec, f)


def test_driver_refusals(ctx):
    f = synth.field(16, 16, 16, seed=1)
    for m in ((2, 1, 1), (1, 2, 2)):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_budget(f, BIG, seg=1024, m=m)
        assert "error -3:" in str(e.value) and "local cutoff" in str(e.value), str(e.value)
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_budget(f, BIG, seg=1024)
        assert "error -3:" in str(e.value) and "residual" in str(e.value), str(e.value)
    finally:
        ctx.set_keep_residual(False)
    for tol_min in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_host_seg_budget(f, BIG, tol_min=tol_min, seg=1024)
        assert "error -1:" in str(e.value), str(e.value)
    with pytest.raises(api.WaveRangeError):
        ctx.encode_host_seg_budget(f, BIG, seg=17)


@pytest.mark.parametrize("dims,seg", [CASES[1], CASES[2]], ids=case_id)
def test_driver_fp32_equals_fp64_of_the_widened_field(ctx, dims, seg):
    f32 = make_field("smooth", dims).astype(np.float32)
    wide = f32.astype(np.float64)
    ref = BudgetRef(Oracle(), wide, seg)
    a1, b1 = ref.last_interval(1)
    budget = ref.B((a1 + b1) // 2)
    i64, d64, r64 = ctx.encode_host_seg_budget(wide, budget, seg=seg)
    i32, d32, r32 = ctx.encode_host_seg_budget_f32(f32, budget, seg=seg)
    assert (r32["g"], r32["bound"]) == (r64["g"], r64["bound"]) and ref.B(r64["g"]) <= budget
    assert r64["g"] == 0 or ref.B(r64["g"] - 1) > budget
    assert all(i32[k] == i64[k] for k in HEADER_KEYS) and np.array_equal(d32, d64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,seg", [CASES[0], CASES[2], CASES[4]], ids=case_id)
def test_driver_device_field_gives_the_host_forms_bytes(ctx, dims, seg, kind):
    f, ref, _ = ref_of(kind, dims, seg)
    budget = budgets_of(ref)["inside plane 2"]

    def on_device(fld, max_bytes, tol_min, s):
        buf = ctx.to_device(fld)
        try:
            return ctx.encode_seg_budget(buf, fld.shape, max_bytes, tol_min=tol_min, seg=s)
        finally:
            buf.free()

    res = check_call(ctx, kind, dims, seg, budget, encode=on_device)  # (check_call compares with encode_host_seg's bytes)
    _, _, host = ctx.encode_host_seg_budget(f, budget, seg=seg)
    assert host["g"] == res["g"] and host["bound"] == res["bound"]


@pytest.mark.parametrize("dims,seg", [CASES[2], CASES[4]], ids=case_id)
def test_driver_is_deterministic(ctx, dims, seg):
    f, ref, _ = ref_of("noise", dims, seg)
    budget = budgets_of(ref)["inside plane 2"]
    runs = [ctx.encode_host_seg_budget(f, budget, seg=seg) for _ in range(3)]
    for info, data, res in runs[1:]:
        assert (res["g"], res["bound"], res["probe_passes"]) == (runs[0][2]["g"], runs[0][2]["bound"], runs[0][2]["probe_passes"])
        assert np.array_equal(data, runs[0][1]) and all(info[k] == runs[0][0][k] for k in HEADER_KEYS)
