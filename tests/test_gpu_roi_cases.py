"""Region decode on the GPU over the table of tests/roi_cases.py: every position of six sweeps at every level, the 64 corner
combinations of (208, 203, 200) and the degenerate fields, through the single-region and the many-region calls.

The expected result is the crop of D(r, p) as tests/test_gpu_lowres.py builds it on the CPU from the oracle's dequantiser and
transform, computed once per (field, level, p).  Every comparison is equality of bit patterns; there is no tolerance anywhere.
Every case first has its plan asserted through api.roi_plan (roi_cases.check_plan), so that it is known which kernels the
comparison has run, and a failure names the case (sweep, level, axis and position are in its id) and the classes of its plan."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401
import roi_cases as rc
from test_gpu_lowres import expected, field, same_bits, split_planes
from test_gpu_roi import crop, masked, needed_sets
from oracle.loader import Oracle
from waverange_amd import api

pytestmark = pytest.mark.gpu

# planes per field of the stage-level tests
NLAY = {"even_x": 8, "even_y": 3, "even_z": 1, "odd_x": 8, "odd_y": 1, "odd_z": 3}
DECODED = [0]  # regions decoded and compared by this module


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c
        for f in _FIELDS.values():
            f["d_planes"].free()
        _FIELDS.clear()
    print("\ntest_gpu_roi_cases: %d regions decoded and compared" % DECODED[0])


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


# ---- stage level: random planes, no coder -------------------------------------------------------------------------------
_FIELDS = {}


def planes_of(ctx, shape, wlev, nlay):
    """Random byte planes of a field in device memory at wr_plane_pitch, a wr_enc_info made by hand (deps / minval as
    tests/test_gpu_parity.py::test_dequant_accum_bit_exact) and the D(r, p) computed so far; made once, never written to."""
    key = (shape, wlev)
    if key not in _FIELDS:
        n = int(np.prod(shape))
        rs = np.random.RandomState(n % 9973 + wlev)
        planes = [rs.randint(0, 256, n).astype(np.uint8) for _ in range(nlay)]
        meta = dict(midval=0.0, wlev=wlev, nlay=nlay, ntot_enc=n * nlay, len_enc_vec=[n] * nlay,
                    deps_vec=[10.0 ** (-2 * i) * 0.37 for i in range(nlay)], minval_vec=[-(10.0 ** (-2 * i)) * 1.1 for i in range(nlay)])
        pitch = api.lib().wr_plane_pitch(n)
        host = np.zeros(pitch * nlay, dtype=np.uint8)
        for l, q in enumerate(planes):
            host[l * pitch:l * pitch + n] = q
        _FIELDS[key] = dict(planes=planes, meta=meta, info=api.EncInfo.from_dict(meta), d_planes=ctx.to_device(host), D={})
    assert _FIELDS[key]["meta"]["nlay"] == nlay
    return _FIELDS[key]


def D(oracle, fld, shape, level, p):
    if (level, p) not in fld["D"]:
        fld["D"][level, p] = expected(oracle, fld["planes"], fld["meta"], shape, level, p)
    return fld["D"][level, p]


def check_multi(ctx, oracle, fld, cases, p):
    """the cases (one field, one level) in one many-region call"""
    _, shape, _, level, _ = cases[0]
    notes = [rc.check_plan(api, c)[1] for c in cases]
    rois = [c[4] for c in cases]
    offs = api.roi_multi_offsets(shape, level, rois)
    full = D(oracle, fld, shape, level, p)
    d_out = ctx.alloc(max(8 * int(offs[-1]), 16))
    try:
        ctx.decode_planes_rois(d_out, shape, level, rois, fld["d_planes"], fld["info"], p)
        flat = d_out.download(np.float64, int(offs[-1]))
    finally:
        d_out.free()
    for i, (c, r) in enumerate(zip(cases, rois)):
        assert same_bits(flat[offs[i]:offs[i + 1]].reshape(api.roi_shape(r)), crop(full, r)), ("multi", c[0], p, notes[i])
    DECODED[0] += len(cases)


def check_singles(ctx, oracle, fld, cases, p):
    """the cases (one field, one level), one single-region call each"""
    _, shape, _, level, _ = cases[0]
    full = D(oracle, fld, shape, level, p)
    d_out = ctx.alloc(max(8 * max(int(np.prod(api.roi_shape(c[4]))) for c in cases), 16))
    try:
        for c in cases:
            note = rc.check_plan(api, c)[1]
            want = crop(full, c[4])
            ctx.decode_planes_roi(d_out, shape, level, c[4], fld["d_planes"], fld["info"], p)
            assert same_bits(d_out.download(np.float64, want.size).reshape(want.shape), want), ("single", c[0], p, note)
    finally:
        d_out.free()
    DECODED[0] += len(cases)


# the order makes the windows, and with them the slot's field, scratch and low-pass buffers, grow and shrink between calls:
# fields alternate between 417 792 and 5 481 samples, levels between the widest windows (0) and the narrowest (4)
@pytest.mark.parametrize("name", ["even_x", "odd_z", "even_y", "odd_x", "even_z", "odd_y"])
def test_sweep(ctx, oracle, name):
    """every position of every level in one many-region call, and in one single-region call each (4 080 of them on an even
    sweep take under a second)"""
    shape, _ = rc.SWEEPS[name]
    fld = planes_of(ctx, shape, 4, NLAY[name])
    by_level = {}
    for c in rc.sweep_cases(name):
        by_level.setdefault(c[3], []).append(c)
    for level in (0, 4, 1, 3, 2):
        cases = by_level[level]
        assert len(cases) == rc.sweep_positions(name, level) <= api.ROI_MULTI_MAX
        for p in sorted({1, NLAY[name]}):
            check_multi(ctx, oracle, fld, cases, p)
            check_singles(ctx, oracle, fld, cases, p)


@pytest.mark.parametrize("kz", rc.CORNER_KINDS)
def test_corners(ctx, oracle, kz):
    fld = planes_of(ctx, rc.CORNER_FIELD, 4, 3)
    cases = [c for c in rc.corner_cases() if c[0].startswith("corner-%s-" % kz)]
    assert len(cases) == 16
    for p in (1, 3):
        check_multi(ctx, oracle, fld, cases, p)
        check_singles(ctx, oracle, fld, cases, p)


def test_degenerate_fields_and_single_cases(ctx, oracle):
    for c in rc.SINGLES:
        _, shape, wlev, _, _ = c
        nlay = 8 if c[0] == "cube64" else 3
        fld = planes_of(ctx, shape, wlev, nlay)
        for p in (1, nlay):
            check_singles(ctx, oracle, fld, [c], p)
            check_multi(ctx, oracle, fld, [c], p)
    # the cases of one field and level together in one call, each of them twice
    groups = {}
    for c in rc.SINGLES:
        groups.setdefault((c[1], c[2], c[3]), []).append(c)
    for (shape, wlev, _), cases in groups.items():
        check_multi(ctx, oracle, planes_of(ctx, shape, wlev, 8 if cases[0][0] == "cube64" else 3), cases + cases[::-1], 1)


def test_windows_grow_and_shrink_in_one_context(ctx, oracle):
    """One case after the other across fields, the largest windows between the smallest and fused windows between general
    ones: every call re-sizes the slot's buffers or finds them larger than it needs, and reads nothing the call before left."""
    corners = {c[0]: c for c in rc.corner_cases()}
    singles = {c[0]: c for c in rc.SINGLES}
    sweep = {c[0]: c for name in ("even_x", "odd_x") for c in rc.sweep_cases(name)}
    order = [corners["corner-whole-whole-whole"], singles["cube64"], sweep["even_x-l0-x204"], singles["linex-l0-mid"],
             corners["corner-interior-interior-interior"], sweep["odd_x-l4-x6"], corners["corner-whole-low-whole"], sweep["even_x-l0-x407"],
             corners["corner-low-low-low"], sweep["odd_x-l0-x132"], singles["wlev0-point"], corners["corner-high-high-high"],
             sweep["even_x-l2-x0"], corners["corner-whole-interior-interior"], singles["cube64"]]
    nlay_of = {rc.CORNER_FIELD: 3, (64, 64, 64): 8, (32, 32, 408): 8, (13, 21, 203): 8}
    for c in order + order[::-1]:
        fld = planes_of(ctx, c[1], c[2], nlay_of.get(c[1], 3))
        check_singles(ctx, oracle, fld, [c], fld["meta"]["nlay"])


# ---- codec level: the coder, the segment lists, the fp32 crop and the scale ----------------------------------------------
_STREAMS = {}
FORMATS = {"wrs1": dict(), "wrs2": dict(brick=8), "wrs3": dict(strands=8)}


def stream(ctx, name, fmt):
    """The synthetic field of the sweep's shape coded at 1e-6, segments of 1008 symbols; its planes from the host reference
    of the WRS1 stream (every format codes the same planes) and the D(r, p) computed so far.  Shared, never written to."""
    shape, _ = rc.SWEEPS[name]
    if name not in _STREAMS:
        f = field(shape)
        enc, _ = ctx.encode_host_seg(f, 1e-6, 1, 1008)
        enc["data"] = enc["data"].copy()
        planes = [api.seg_decode_host_ref(b, f.size) for b in split_planes(enc)]
        _STREAMS[name] = dict(f=f, planes=planes, meta=enc, D={}, enc={"wrs1": enc})
    s = _STREAMS[name]
    if fmt not in s["enc"]:
        enc, _ = ctx.encode_host_seg(s["f"], 1e-6, 1, 1008, **FORMATS[fmt])
        enc["data"] = enc["data"].copy()
        assert enc["nlay"] == s["meta"]["nlay"] and bytes(enc["data"][:4]) == fmt.upper().encode()
        s["enc"][fmt] = enc
    return s, s["enc"][fmt]


def single_all_ways(ctx, shape, level, roi, enc, p, d_buf):
    rshape = api.roi_shape(roi)
    h64, h32 = np.empty(rshape), np.empty(rshape, dtype=np.float32)
    ctx.decode_host_seg_roi(h64, shape, level, roi, enc, p)
    ctx.decode_host_seg_roi_f32(h32, shape, level, roi, enc, p)
    ctx.decode_seg_roi(d_buf, shape, level, roi, enc, p)
    return h64, h32, d_buf.download(np.float64, h64.size).reshape(rshape)


@pytest.mark.parametrize("name,fmt", [(n, f) for n in ("even_x", "odd_x") for f in FORMATS] + [("even_z", "wrs1"), ("odd_z", "wrs1")])
def test_codec_level(ctx, oracle, name, fmt):
    """Levels 0 and 2 (the scale is 1 and 2^-3): every position through the many-region calls, every 16th and the first and
    last through the single-region calls, and those again on a stream whose unlisted segments are all 0xFF (WRS1, whose
    layout tests/test_gpu_roi.py::masked knows): a list one segment short at some position shows as wrong values.  The two
    z sweeps are here for that: their level-0 windows need a run of the stream's segments, those of the x sweeps all."""
    shape, _ = rc.SWEEPS[name]
    s, enc = stream(ctx, name, fmt)
    nlay = enc["nlay"]
    assert nlay >= 2 and enc["wlev"] == 4
    d_buf = ctx.alloc(8 * 32 * 2 * 408)  # the regions of the longest sweep level
    try:
        for level in (0, 2):
            cases = [c for c in rc.sweep_cases(name) if c[3] == level]
            notes = [rc.check_plan(api, c)[1] for c in cases]
            rois = [c[4] for c in cases]
            offs = api.roi_multi_offsets(shape, level, rois)
            assert int(offs[-1]) <= 32 * 2 * 408
            for p in (1, nlay):
                if (level, p) not in s["D"]:
                    s["D"][level, p] = expected(oracle, s["planes"], s["meta"], shape, level, p)
                full = s["D"][level, p]
                h64 = ctx.decode_host_seg_rois(shape, level, rois, enc, p)
                h32 = ctx.decode_host_seg_rois(shape, level, rois, enc, p, dtype=np.float32)
                ctx.decode_seg_rois(d_buf, shape, level, rois, enc, p)
                flat = d_buf.download(np.float64, int(offs[-1]))
                for i, (c, r) in enumerate(zip(cases, rois)):
                    want = crop(full, r)
                    assert same_bits(h64[i], want), ("multi host", fmt, c[0], p, notes[i])
                    assert same_bits(h32[i], want.astype(np.float32)), ("multi fp32", fmt, c[0], p, notes[i])
                    assert same_bits(flat[offs[i]:offs[i + 1]].reshape(want.shape), want), ("multi device", fmt, c[0], p, notes[i])
                DECODED[0] += 3 * len(cases)
            full = s["D"][level, nlay]
            some = sorted(set(range(0, len(cases), 16)) | {0, len(cases) - 1})
            for i in some:
                c, r = cases[i], rois[i]
                want = crop(full, r)
                streams = [("as coded", enc)]
                if fmt == "wrs1":
                    sets = needed_sets(enc, shape, level, r)
                    if level == 2 or name.endswith("_z"):  # (at level 0 a window that spans y and z takes a run of every row)
                        assert all(need.size < lens.size for need, lens in sets), (c[0], notes[i])
                    streams.append(("unlisted segments 0xFF", masked(enc, sets)))
                for what, e in streams:
                    h64, h32, d64 = single_all_ways(ctx, shape, level, r, e, nlay, d_buf)
                    assert same_bits(h64, want), ("single host", what, fmt, c[0], notes[i])
                    assert same_bits(h32, want.astype(np.float32)), ("single fp32", what, fmt, c[0], notes[i])
                    assert same_bits(d64, want), ("single device", what, fmt, c[0], notes[i])
                    DECODED[0] += 3
    finally:
        d_buf.free()
