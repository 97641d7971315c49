"""Batched segmented streams on the GPU: plane l of all fields of a batch in one coder launch.  There is no new format, so the
oracle is equality throughout: every blob of a batch is the host reference's blob of that plane (wr_seg_encode_host_ref on the
CPU oracle's planes), every field's record and bytes are the single-field call's, every reconstruction is decode_host_seg's."""
import numpy as np
import pytest

from util import bits_equal, kat_plane
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

# (nx, ny, nz), seg: the shapes' sizes are the stage-level table's n, with the same segment lengths
SHAPES = [((48, 40, 36), 4096), ((16, 8, 8), 4096), ((40, 40, 11), 16), ((64, 64, 64), 0)]
TOLS = (1e-2, 1e-5, 1e-9)
NFIELDS = 7      # six fields and a constant one in the middle
CONSTANT_AT = 3


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


_fields = {}


def batch_fields(shape):
    """The fields of a shape's batch (made once, never written) and their tolerances."""
    if shape not in _fields:
        nx, ny, nz = shape
        fs, tols = [], []
        for i in range(NFIELDS):
            if i == CONSTANT_AT:
                fs.append(np.full((nz, ny, nx), -2.5))
            else:
                fs.append(synth.field(nx, ny, nz, seed=100 + i))
            tols.append(TOLS[i % 3])
        _fields[shape] = (fs, tols)
    return _fields[shape]


_oracle_planes = {}


def oracle_planes(oracle, key, f, tol, wtflag=1):
    """The quantized planes of a field by the CPU oracle (computed once per key)."""
    if key not in _oracle_planes:
        enc = oracle.encode(f, tol, wtflag)
        planes, at = [], 0
        for l in range(enc["nlay"]):
            ln = int(enc["len_enc_vec"][l])
            p, got = oracle.range_decode(enc["data"][at:at + ln], f.size)
            assert got == f.size
            planes.append(p[:f.size].copy())
            at += ln
        _oracle_planes[key] = planes
    return _oracle_planes[key]


def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def keep(enc):
    enc["data"] = enc["data"].copy()
    return enc


def same_record(got, want, what):
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(got[k]).hex() == float(want[k]).hex(), (what, k)
    assert got["wlev"] == want["wlev"] and got["nlay"] == want["nlay"], what
    assert bits_equal(got["deps_vec"], want["deps_vec"]) and bits_equal(got["minval_vec"], want["minval_vec"]), what
    assert list(got["len_enc_vec"]) == list(want["len_enc_vec"]) and got["ntot_enc"] == want["ntot_enc"], what
    assert got["data"].size == want["data"].size and np.array_equal(got["data"], want["data"]), what


# ---- stage level --------------------------------------------------------------------------------------------------------------
STAGE = [
    (1024, 4096, 70),      # every lane of two waves a different job
    (69120, 4096, 9),      # 17 segments per job, the last 3584 symbols long; job boundaries inside a wave and across waves
    (17600, 16, 3),        # 1100 segments per job: past the scan's 1024 threads
    (262144, 59904, 13),   # 65 lanes: one lane in a second wave
    (4097, 4096, 1),       # a batch of one
]
STAGE_FIELD = {1024: (16, 8, 8), 69120: (48, 40, 36), 17600: (40, 40, 11), 262144: (64, 64, 64), 4097: (241, 17, 1)}


def stage_planes(oracle, n, jobs):
    """`jobs` different planes of n symbols: the three known-answer planes, the oracle's quantizer planes of a field of that
    size, then rotations of those."""
    nx, ny, nz = STAGE_FIELD[n]
    base = [kat_plane(kind, n) for kind in ("uniform", "skewed", "sparse")]
    base += oracle_planes(oracle, ("stage", n), synth.field(nx, ny, nz, seed=41), 1e-6)
    out = []
    for j in range(jobs):
        out.append(np.roll(base[j % len(base)], 37 * (j // len(base))))
    return out


@pytest.mark.parametrize("n,seg,jobs", STAGE)
def test_stage_level(ctx, oracle, n, seg, jobs):
    planes = stage_planes(oracle, n, jobs)
    want = [api.seg_encode_host_ref(p, seg) for p in planes]
    got = ctx.seg_encode_planes_batch(planes, seg)
    assert len(got) == jobs
    for j in range(jobs):
        assert got[j].size == want[j].size and np.array_equal(got[j], want[j]), (n, seg, "job %d" % j)
    syms, bad = ctx.seg_decode_planes_batch(want, n)
    assert bad == [0] * jobs
    for j in range(jobs):
        assert np.array_equal(syms[j], planes[j]), (n, seg, "job %d" % j)
    # the single-plane calls read and write the same blobs
    assert np.array_equal(ctx.seg_encode_plane(planes[-1], seg), got[-1])
    sym, b = ctx.seg_decode_plane(got[0], n)
    assert b == 0 and np.array_equal(sym, planes[0])


def test_stage_level_refusals(ctx):
    p = kat_plane("skewed", 10000)
    good = api.seg_encode_host_ref(p, 4096)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_encode_planes_batch([], 4096)
    assert "error -1" in str(e.value)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_encode_planes_batch([p], 60000)
    # a malformed index in job 1 is refused on the host; nothing is launched for job 0 or 2 either
    for at, what in ((0, "magic"), (4, "segment"), (8, "segment count"), (12, "add up")):
        bad_blob = good.copy()
        bad_blob[at] ^= 1
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_planes_batch([good, bad_blob, good], 10000)
        assert "error -4" in str(e.value) and "job 1" in str(e.value) and what in str(e.value), str(e.value)
    wrs3 = api.seg_encode_host_ref_strands(p, seg=4096, strands=8)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_planes_batch([good, good, wrs3], 10000)
    assert "error -3" in str(e.value) and "job 2" in str(e.value), str(e.value)
    # one byte short in job 1: WR_ERR_OVERFLOW naming it; job 0 is complete
    L = api.lib()
    d_sym, d_blob = [ctx.to_device(p) for _ in range(2)], [ctx.alloc(good.size + 16) for _ in range(2)]
    try:
        sp = (api.C.c_void_p * 2)(*[d.ptr for d in d_sym])
        bp = (api.C.c_void_p * 2)(*[d.ptr for d in d_blob])
        cap, got = (api.C.c_size_t * 2)(good.size, good.size - 1), (api.C.c_size_t * 2)()
        assert L.wr_dev_seg_encode_batch(ctx.h, 2, sp, p.size, 4096, bp, cap, got) == -5
        assert "job 1" in L.wr_last_error().decode() and got[0] == good.size
        assert np.array_equal(d_blob[0].download(np.uint8, good.size), good)
        cap[1] = good.size
        assert L.wr_dev_seg_encode_batch(ctx.h, 2, sp, p.size, 4096, bp, cap, got) == 0 and list(got) == [good.size] * 2
        assert np.array_equal(d_blob[1].download(np.uint8, good.size), good)
    finally:
        for d in d_sym + d_blob:
            d.free()


# ---- whole path -----------------------------------------------------------------------------------------------------------------
def singles(ctx, kind, fs, tols, wtflag, seg, brick, cutoffs=None, m=(1, 1, 1)):
    """Every field through the single-field call: the yardstick of a batch."""
    out = []
    for i, f in enumerate(fs):
        kw = dict(cutoff=None if cutoffs is None else cutoffs[i], m=m, brick=brick)
        tol = None if cutoffs is not None else tols[i]
        if kind == "f32":
            enc, _ = ctx.encode_host_seg_f32(f, tol, wtflag, seg, **kw)
        elif kind == "dev":
            buf = ctx.to_device(f)
            try:
                enc, _ = ctx.encode_seg(buf, f.shape, tol, wtflag, seg, **kw)
            finally:
                buf.free()
        else:
            enc, _ = ctx.encode_host_seg(f, tol, wtflag, seg, **kw)
        out.append(keep(enc))
    return out


def batch(ctx, kind, fs, tols, wtflag, seg, brick, cutoffs=None, m=(1, 1, 1)):
    if kind == "f32":
        encs, tm = ctx.encode_host_seg_batch_f32(fs, tols, wtflag, seg, brick, cutoffs, m)
    elif kind == "dev":
        bufs = [ctx.to_device(f) for f in fs]
        try:
            encs, tm = ctx.encode_seg_batch(bufs, fs[0].shape, tols, wtflag, seg, brick, cutoffs, m)
        finally:
            for b in bufs:
                b.free()
    else:
        encs, tm = ctx.encode_host_seg_batch(fs, tols, wtflag, seg, brick, cutoffs, m)
    return [keep(e) for e in encs], tm


def decode_singles(ctx, kind, fs, encs):
    out = []
    for f, enc in zip(fs, encs):
        rec = np.empty_like(f)
        (ctx.decode_host_seg_f32 if kind == "f32" else ctx.decode_host_seg)(rec, enc)
        out.append(rec)
    return out


def decode_batch(ctx, kind, fs, encs):
    if kind == "dev":
        bufs = [ctx.alloc(f.nbytes) for f in fs]
        try:
            tm = ctx.decode_seg_batch(bufs, fs[0].shape, encs)
            return [b.download(np.float64, f.size).reshape(f.shape) for b, f in zip(bufs, fs)], tm
        finally:
            for b in bufs:
                b.free()
    outs = [np.empty_like(f) for f in fs]
    tm = (ctx.decode_host_seg_batch_f32 if kind == "f32" else ctx.decode_host_seg_batch)(outs, encs)
    return outs, tm


def same_bits(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@pytest.mark.parametrize("kind,brick", [("f64", None), ("f64", 32), ("f32", None), ("f32", 32), ("dev", None)])
@pytest.mark.parametrize("shape,seg", SHAPES)
def test_whole_path(ctx, oracle, shape, seg, kind, brick):
    fs, tols = batch_fields(shape)
    if kind == "f32":
        fs = [f.astype(np.float32) for f in fs]
    want = singles(ctx, kind, fs, tols, 1, seg, brick)
    got, tm = batch(ctx, kind, fs, tols, 1, seg, brick)
    nlays = [e["nlay"] for e in got]
    assert nlays == [2, 3, 5, 0, 3, 5, 2], nlays  # the CPU oracle's counts; plane indices with fewer jobs than fields are run
    assert len(set(nlays)) >= 3
    for i in range(NFIELDS):
        same_record(got[i], want[i], (shape, kind, brick, "field %d" % i))
        # not only GPU against GPU: every plane blob is the host reference's blob of the oracle's plane
        f64 = np.ascontiguousarray(fs[i], dtype=np.float64)
        planes = [] if i == CONSTANT_AT else oracle_planes(oracle, (shape, kind == "f32", i), f64, tols[i])
        assert len(planes) == got[i]["nlay"]
        for l, (blob, p) in enumerate(zip(split_planes(got[i]), planes)):
            ref = api.seg_encode_host_ref(p, seg) if brick is None else api.seg_encode_host_ref_blocked(p, fs[i].shape, 4, brick, seg)
            assert np.array_equal(blob, ref), (shape, kind, brick, "field %d plane %d" % (i, l))
    assert tm["rangecoder"] > 0 and all(t > 0 for t in tm["plane_coder_s"][:max(nlays)]) and not any(tm["plane_coder_s"][max(nlays):]), tm
    # the batched decode of those streams is decode_host_seg's, bit for bit
    dkind = "f64" if kind == "dev" else kind
    recs = decode_singles(ctx, dkind, fs, want)
    outs, dtm = decode_batch(ctx, kind, fs, got)
    for i in range(NFIELDS):
        assert same_bits(outs[i], recs[i]), (shape, kind, brick, "field %d" % i)
    assert np.array_equal(outs[CONSTANT_AT], fs[CONSTANT_AT])
    assert dtm["rangecoder"] > 0, dtm
    # the batch in reverse order: every field's bytes stay what they were
    rev, _ = batch(ctx, kind, fs[::-1], tols[::-1], 1, seg, brick)
    for i in range(NFIELDS):
        same_record(rev[NFIELDS - 1 - i], want[i], (shape, kind, brick, "reversed, field %d" % i))


@pytest.mark.parametrize("shape,seg", SHAPES[:2])
def test_decode_batch_mixes_wrs1_and_wrs2(ctx, shape, seg):
    """Single-call streams, WRS1 and WRS2 (two brick edges) alternating, through one batched decode."""
    fs, tols = batch_fields(shape)
    bricks = [None, 32, 8, None, 32, None, 8]
    encs = [singles(ctx, "f64", [f], [t], 1, seg, b)[0] for f, t, b in zip(fs, tols, bricks)]
    recs = decode_singles(ctx, "f64", fs, encs)
    outs, _ = decode_batch(ctx, "f64", fs, encs)
    for i in range(NFIELDS):
        assert same_bits(outs[i], recs[i]), (shape, "field %d" % i)


@pytest.mark.parametrize("brick", [None, 32])
def test_no_transform_and_local_cutoff(ctx, oracle, brick):
    shape, seg = SHAPES[0]
    fs, tols = batch_fields(shape)
    # wtflag = 0
    want = singles(ctx, "f64", fs, tols, 0, seg, brick)
    got, _ = batch(ctx, "f64", fs, tols, 0, seg, brick)
    assert [e["nlay"] for e in got] == [2, 3, 4, 0, 3, 4, 2]  # the CPU oracle's counts
    for i in range(NFIELDS):
        same_record(got[i], want[i], ("wtflag 0", brick, i))
        planes = [] if i == CONSTANT_AT else oracle_planes(oracle, (shape, "wt0", i), fs[i], tols[i], 0)
        for l, (blob, p) in enumerate(zip(split_planes(got[i]), planes)):
            ref = api.seg_encode_host_ref(p, seg) if brick is None else api.seg_encode_host_ref_blocked(p, fs[i].shape, 0, brick, seg)
            assert np.array_equal(blob, ref), ("wtflag 0", brick, i, l)
    outs, _ = decode_batch(ctx, "f64", fs, got)
    for i, rec in enumerate(decode_singles(ctx, "f64", fs, want)):
        assert same_bits(outs[i], rec), ("wtflag 0", brick, i)
    # a local cutoff per field, m = (2, 2, 2)
    base = np.array([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-4, 1e-5])
    cutoffs = [np.roll(base, i) * (10.0 ** -(i % 3)) for i in range(NFIELDS)]
    want = singles(ctx, "f64", fs, None, 1, seg, brick, cutoffs, (2, 2, 2))
    got, _ = batch(ctx, "f64", fs, None, 1, seg, brick, cutoffs, (2, 2, 2))
    assert len({e["nlay"] for e in got}) >= 3
    for i in range(NFIELDS):
        same_record(got[i], want[i], ("local cutoff", brick, i))
    outs, _ = decode_batch(ctx, "f64", fs, got)
    for i, rec in enumerate(decode_singles(ctx, "f64", fs, want)):
        assert same_bits(outs[i], rec), ("local cutoff", brick, i)


# ---- refusals: the context goes on working after each ------------------------------------------------------------------------
def test_refusals(ctx):
    shape, seg = SHAPES[1]
    fs, tols = batch_fields(shape)
    want = singles(ctx, "f64", fs, tols, 1, seg, None)
    recs = decode_singles(ctx, "f64", fs, want)

    def good_batch(what):
        got, _ = batch(ctx, "f64", fs, tols, 1, seg, None)
        for i in range(NFIELDS):
            same_record(got[i], want[i], (what, i))
        outs, _ = decode_batch(ctx, "f64", fs, got)
        for i in range(NFIELDS):
            assert same_bits(outs[i], recs[i]), (what, i)

    def refused(code, fn, *names):
        with pytest.raises(api.WaveRangeError) as e:
            fn()
        assert ("error %d" % code) in str(e.value) and all(s in str(e.value) for s in names), str(e.value)

    # the number of fields
    for many in ([], [fs[0]] * (api.SEG_BATCH_MAX + 1)):
        refused(-1, lambda: ctx.encode_host_seg_batch(many, 1e-3, 1, seg))
        good_batch("after an encode of %d fields" % len(many))
        refused(-1, lambda: ctx.decode_host_seg_batch([np.empty_like(fs[0]) for _ in many], [want[0]] * len(many)))
        good_batch("after a decode of %d fields" % len(many))
    encs, _ = ctx.encode_host_seg_batch([fs[1]] * 4, tols[1], 1, seg)  # (the same field four times is a batch like any other)
    for e in encs:
        same_record(e, want[1], "one field four times")
    # field 4's buffer one byte short
    j = 4
    caps = [e["ntot_enc"] + 64 for e in want]
    caps[j] = want[j]["ntot_enc"] - 1
    refused(-5, lambda: ctx.encode_host_seg_batch(fs, tols, 1, seg, caps=caps), "field %d" % j)
    good_batch("after an overflow")
    # a decode batch in which field j's magic, seg, nseg or one index length is flipped: refused on the host, no launch --
    # the other fields' output buffers are not touched (there is no launch counter in wr_stat)
    for at, what in ((0, "magic"), (4, "segment"), (8, "segment count"), (12, "add up")):
        bad = [dict(e) for e in want]
        bad[j] = dict(want[j], data=want[j]["data"].copy())
        bad[j]["data"][want[j]["len_enc_vec"][0] + at] ^= 1  # in the header or index of field j's SECOND plane
        outs = [np.full_like(f, 1234.5) for f in fs]
        refused(-4, lambda: ctx.decode_host_seg_batch(outs, bad), "field %d" % j, "plane 1", what)
        assert all(np.all(o == 1234.5) for o in outs), what
        good_batch("after a flipped " + what)
    bad = [dict(e) for e in want]
    bad[j] = dict(want[j], len_enc_vec=[want[j]["len_enc_vec"][0] + 1] + list(want[j]["len_enc_vec"][1:]))
    outs = [np.full_like(f, 1234.5) for f in fs]
    refused(-4, lambda: ctx.decode_host_seg_batch(outs, bad), "field %d" % j)
    assert all(np.all(o == 1234.5) for o in outs)
    # strands: a WRS3 stream in a decode batch, `strands` on encode
    wrs3, _ = ctx.encode_host_seg(fs[2], tols[2], 1, seg, strands=8)
    mixed = list(want)
    mixed[2] = keep(wrs3)
    outs = [np.full_like(f, 1234.5) for f in fs]
    refused(-3, lambda: ctx.decode_host_seg_batch(outs, mixed), "field 2")
    assert all(np.all(o == 1234.5) for o in outs)
    good_batch("after a WRS3 field")
    refused(-3, lambda: ctx.encode_host_seg_batch(fs, tols, 1, seg, strands=8))
    # a context that keeps residuals
    ctx.set_keep_residual(True)
    try:
        refused(-3, lambda: ctx.encode_host_seg_batch(fs, tols, 1, seg))
    finally:
        ctx.set_keep_residual(False)
    good_batch("after keep_residual")
