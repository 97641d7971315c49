"""The batch calls for WRS3 on the GPU: stranded fields in the batched coder launches.  There is no new format, so the oracle is
equality throughout: every blob of a strand batch is the host reference's blob of that plane and the single-plane kernel's, every
field's record and bytes are the single-field encode_*_seg(..., strands=K)'s, every reconstruction of a mixed decode is
decode_host_seg's, bit for bit.  The launches are counted (WR_STAT_BATCH_CODER_LAUNCHES)."""
import numpy as np
import pytest

import strand_batch_cases as sb
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

STAT_LAUNCHES = 18  # WR_STAT_BATCH_CODER_LAUNCHES
TOLS = (1e-2, 1e-5, 1e-9)
NFIELDS = 7      # six fields and a constant one in the middle
CONSTANT_AT = 3
# (nx, ny, nz), seg, K (0: the default of either)
SHAPES = [((48, 40, 36), 4096, 8), ((16, 8, 8), 4096, 32), ((40, 40, 11), 48, 2), ((64, 64, 64), 0, 0)]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def launches():
    return api.stat(STAT_LAUNCHES)


def keep(enc):
    enc["data"] = enc["data"].copy()
    return enc


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_record(got, want, what):
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(got[k]).hex() == float(want[k]).hex(), (what, k)
    assert got["wlev"] == want["wlev"] and got["nlay"] == want["nlay"], what
    assert bits_equal(np.asarray(got["deps_vec"]), np.asarray(want["deps_vec"])) and bits_equal(np.asarray(got["minval_vec"]), np.asarray(want["minval_vec"])), what
    assert list(got["len_enc_vec"]) == list(want["len_enc_vec"]) and got["ntot_enc"] == want["ntot_enc"], what
    assert got["data"].size == want["data"].size and np.array_equal(got["data"], want["data"]), what


def index_of(blob):
    """(bytes in front of the records, the records' lengths) of a WRS1 / WRS2 / WRS3 blob"""
    head = {b"WRS1": 12, b"WRS2": 16, b"WRS3": 20}[bytes(blob[:4])]
    nseg = int(blob[8:12].view("<u4")[0])
    return head + 4 * nseg, blob[head:head + 4 * nseg].view("<u4").astype(np.int64)


def host_refuses(blob, n):
    try:
        api.seg_decode_host_ref_blocked(blob, (1, 1, n), 0)
    except api.WaveRangeError:
        return True
    return False


# ---- stage level --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sb.STAGE, ids=sb.case_id)
def test_stage_level(ctx, case):
    n, seg, K, jobs = case
    planes = sb.planes(case)
    want = [api.seg_encode_host_ref_strands(p, seg=seg, strands=K) for p in planes]
    before = launches()
    got = ctx.seg_encode_planes_batch_strands(planes, seg, K)
    assert launches() - before == 1
    assert len(got) == jobs
    for j in range(jobs):
        assert got[j].size == want[j].size and np.array_equal(got[j], want[j]), (sb.case_id(case), "job %d" % j, got[j].size, want[j].size)
    for j in sorted({0, jobs // 2, jobs - 1}):  # the single-plane kernels write the same blobs
        assert np.array_equal(ctx.seg_encode_plane(planes[j], seg, strands=K), got[j]), (sb.case_id(case), "job %d" % j)
    before = launches()
    syms, bad = ctx.seg_decode_planes_batch_mixed(want, n)
    assert launches() - before == 1  # (stranded jobs only)
    assert bad == [0] * jobs
    for j in range(jobs):
        assert np.array_equal(syms[j], planes[j]), (sb.case_id(case), "job %d" % j)
    sym, b = ctx.seg_decode_plane(got[0], n)
    assert b == 0 and np.array_equal(sym, planes[0])
    if jobs < 2:
        return
    # a byte flipped inside a strand of job 1 -- the first one of strand 0 of its record 0 that the host reference refuses --
    # and a length word of that record that no longer adds up: the kernel counts the record, and only job 1's
    front, _ = index_of(want[1])
    _, _, _, recs = api.seg_split_strands(want[1])
    s0 = front + 4 * (K + 1) + len(recs[0][0])  # where S_0 of record 0 starts
    damaged = None
    for at in range(s0 + 1, s0 + min(len(recs[0][1][0]), 24)):
        cand = want[1].copy()
        cand[at] ^= 0x55
        if host_refuses(cand, n):
            damaged = cand
            break
    words = want[1].copy()
    words[front + 4] ^= 4  # slen[0] of record 0
    assert host_refuses(words, n)
    for blob in (damaged, words):
        if blob is None:
            continue  # (no flip of those bytes is refused by the host reference either: the flag step happens to survive them)
        _, bad = ctx.seg_decode_planes_batch_mixed([want[0], blob] + want[2:], n, check=False)
        assert bad[1] >= 1 and bad[:1] + bad[2:] == [0] * (jobs - 1), (sb.case_id(case), bad)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_planes_batch_mixed([want[0], blob] + want[2:], n)
        assert "error -4" in str(e.value) and "job 1" in str(e.value), str(e.value)
    # a malformed header or index in job 1 is refused on the host; nothing is launched for any job
    before = launches()
    for at, flip, what in ((0, 1, "magic"), (4, 1, "segment"), (8, 1, "segment count"), (20, 4, "add up")):  # (the last: an index length)
        bad_blob = want[1].copy()
        bad_blob[at] ^= flip
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_planes_batch_mixed([want[0], bad_blob] + want[2:], n)
        assert "error -4" in str(e.value) and "job 1" in str(e.value) and what in str(e.value), (at, str(e.value))
    assert launches() == before


def test_stage_level_mixed_list(ctx):
    """WRS1 and WRS3 jobs of several segment lengths and strand counts side by side: two launches"""
    jobs = sb.mixed_jobs()
    n = sb.MIXED_N
    blobs = [api.seg_encode_host_ref(p, seg) if K == 0 else api.seg_encode_host_ref_strands(p, seg=seg, strands=K) for p, seg, K in jobs]
    before = launches()
    syms, bad = ctx.seg_decode_planes_batch_mixed(blobs, n)
    assert launches() - before == 2
    assert bad == [0] * len(jobs)
    for j, (p, seg, K) in enumerate(jobs):
        assert np.array_equal(syms[j], p), (j, seg, K)
    # in reverse order, and the plain jobs alone (one launch)
    syms, bad = ctx.seg_decode_planes_batch_mixed(blobs[::-1], n)
    assert bad == [0] * len(jobs) and all(np.array_equal(s, j[0]) for s, j in zip(syms, jobs[::-1]))
    before = launches()
    plain = [b for b, j in zip(blobs, jobs) if j[2] == 0]
    syms, bad = ctx.seg_decode_planes_batch_mixed(plain, n)
    assert launches() - before == 1 and bad == [0] * len(plain)
    # the old entry point keeps its refusal
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_planes_batch(blobs, n)
    assert "error -3" in str(e.value) and "job 1" in str(e.value), str(e.value)


def test_stage_level_refusals(ctx):
    case = sb.STAGE[1]
    n, seg, K, _ = case
    p = sb.planes(case)[0]
    good = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_encode_planes_batch_strands([], seg, K)
    assert "error -1" in str(e.value)
    for bad_seg, bad_k in ((seg, 3), (seg, 64), (48, 4), (60000, 8)):
        with pytest.raises(api.WaveRangeError):
            ctx.seg_encode_planes_batch_strands([p], bad_seg, bad_k)
    assert np.array_equal(ctx.seg_encode_planes_batch_strands([p], seg, 0)[0], api.seg_encode_host_ref_strands(p, seg=seg, strands=8))  # 0: the default
    # one byte short in job 1: WR_ERR_OVERFLOW naming it; job 0 is complete
    L = api.lib()
    d_sym, d_blob = [ctx.to_device(p) for _ in range(2)], [ctx.alloc(good.size + 16) for _ in range(2)]
    try:
        sp = (api.C.c_void_p * 2)(*[d.ptr for d in d_sym])
        bp = (api.C.c_void_p * 2)(*[d.ptr for d in d_blob])
        cap, got = (api.C.c_size_t * 2)(good.size, good.size - 1), (api.C.c_size_t * 2)()
        assert L.wr_dev_seg_encode_batch_strands(ctx.h, 2, sp, p.size, seg, K, bp, cap, got) == -5
        assert "job 1" in L.wr_last_error().decode() and got[0] == good.size
        assert np.array_equal(d_blob[0].download(np.uint8, good.size), good)
        cap[1] = good.size
        assert L.wr_dev_seg_encode_batch_strands(ctx.h, 2, sp, p.size, seg, K, bp, cap, got) == 0 and list(got) == [good.size] * 2
        assert np.array_equal(d_blob[1].download(np.uint8, good.size), good)
    finally:
        for d in d_sym + d_blob:
            d.free()


# ---- whole path -----------------------------------------------------------------------------------------------------------------
_fields = {}


def batch_fields(shape):
    """The fields of a shape's batch (made once, never written) and their tolerances."""
    if shape not in _fields:
        nx, ny, nz = shape
        fs, tols = [], []
        for i in range(NFIELDS):
            fs.append(np.full((nz, ny, nx), -2.5) if i == CONSTANT_AT else synth.field(nx, ny, nz, seed=100 + i))
            tols.append(TOLS[i % 3])
        _fields[shape] = (fs, tols)
    return _fields[shape]


def singles(ctx, kind, fs, tols, wtflag, seg, brick, K):
    """Every field through the single-field call: the yardstick of a batch.  K None: WRS1 / WRS2 (brick None: WRS1)."""
    out = []
    for f, tol in zip(fs, tols):
        kw = dict(brick=brick, strands=K)
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


def batch(ctx, kind, fs, tols, wtflag, seg, brick, K, **kw):
    if kind == "f32":
        encs, tm = ctx.encode_host_seg_batch_strands_f32(fs, tols, wtflag, seg, brick, K, **kw)
    elif kind == "dev":
        bufs = [ctx.to_device(f) for f in fs]
        try:
            encs, tm = ctx.encode_seg_batch_strands(bufs, fs[0].shape, tols, wtflag, seg, brick, K, **kw)
        finally:
            for b in bufs:
                b.free()
    else:
        encs, tm = ctx.encode_host_seg_batch_strands(fs, tols, wtflag, seg, brick, K, **kw)
    return [keep(e) for e in encs], tm


def decode_singles(ctx, kind, fs, encs):
    out = []
    for f, enc in zip(fs, encs):
        rec = np.empty_like(f)
        (ctx.decode_host_seg_f32 if kind == "f32" else ctx.decode_host_seg)(rec, enc)
        out.append(rec)
    return out


def decode_mixed(ctx, kind, fs, encs):
    if kind == "dev":
        bufs = [ctx.alloc(f.nbytes) for f in fs]
        try:
            tm = ctx.decode_seg_batch_mixed(bufs, fs[0].shape, encs)
            return [b.download(np.float64, f.size).reshape(f.shape) for b, f in zip(bufs, fs)], tm
        finally:
            for b in bufs:
                b.free()
    outs = [np.empty_like(f) for f in fs]
    tm = (ctx.decode_host_seg_batch_mixed_f32 if kind == "f32" else ctx.decode_host_seg_batch_mixed)(outs, encs)
    return outs, tm


WHOLE = [(shape, seg, K, "f64", 0, 1) for shape, seg, K in SHAPES] + [
    (SHAPES[1][0], 4096, 32, "f32", 0, 1), (SHAPES[2][0], 48, 2, "dev", 0, 1), (SHAPES[1][0], 4096, 32, "f64", 0, 0), (SHAPES[0][0], 4096, 8, "f64", 8, 1)]


@pytest.mark.parametrize("shape,seg,K,kind,brick,wtflag", WHOLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_whole_path(ctx, shape, seg, K, kind, brick, wtflag):
    fs, tols = batch_fields(shape)
    if kind == "f32":
        fs = [f.astype(np.float32) for f in fs]
    want = singles(ctx, kind, fs, tols, wtflag, seg, brick, K)
    before = launches()
    got, tm = batch(ctx, kind, fs, tols, wtflag, seg, brick, K)
    nlays = [e["nlay"] for e in got]
    assert launches() - before == max(nlays)  # one launch sequence per plane index
    assert nlays[CONSTANT_AT] == 0 and len(set(nlays)) >= 3, nlays  # plane indices with fewer jobs than fields are run
    for i in range(NFIELDS):
        same_record(got[i], want[i], (shape, kind, brick, "field %d" % i))
        if nlays[i]:
            assert bytes(got[i]["data"][:4]) == b"WRS3" and int(got[i]["data"][16:20].view("<u4")[0]) == (K or 8)
    assert tm["rangecoder"] > 0 and all(t > 0 for t in tm["plane_coder_s"][:max(nlays)]) and not any(tm["plane_coder_s"][max(nlays):]), tm
    # the mixed decode of those streams is decode_host_seg's, bit for bit: one launch, every job is stranded
    dkind = "f64" if kind == "dev" else kind
    recs = decode_singles(ctx, dkind, fs, want)
    before = launches()
    outs, dtm = decode_mixed(ctx, kind, fs, got)
    assert launches() - before == 1
    for i in range(NFIELDS):
        assert bits_equal(outs[i], recs[i]), (shape, kind, brick, "field %d" % i)
    assert np.array_equal(outs[CONSTANT_AT], fs[CONSTANT_AT])
    assert dtm["rangecoder"] > 0 and dtm["plane_coder_s"][0] > 0 and not any(dtm["plane_coder_s"][1:]), dtm
    # the batch in reverse order: every field's bytes stay what they were
    rev, _ = batch(ctx, kind, fs[::-1], tols[::-1], wtflag, seg, brick, K)
    for i in range(NFIELDS):
        same_record(rev[NFIELDS - 1 - i], want[i], (shape, kind, brick, "reversed, field %d" % i))


def mixed_streams(ctx, kind, fs, tols, seg):
    """fields in order: WRS1, WRS2 brick 8, WRS3 K = 4, WRS3 K = 16 with brick 8, constant, WRS3 K = 1 -- single-call streams"""
    formats = [(None, None), (8, None), (None, 4), (8, 16), (None, None), (None, 1)]
    picks = [0, 1, 2, 4, CONSTANT_AT, 5]
    sub = [fs[i] for i in picks]
    encs = [singles(ctx, kind, [fs[i]], [tols[i]], 1, seg, b, K)[0] for i, (b, K) in zip(picks, formats)]
    return sub, encs


@pytest.mark.parametrize("kind", ["f64", "f32", "dev"])
def test_mixed_decode(ctx, kind):
    shape, seg, _ = SHAPES[0]
    fs, tols = batch_fields(shape)
    if kind == "f32":
        fs = [f.astype(np.float32) for f in fs]
    sub, encs = mixed_streams(ctx, "f64" if kind == "dev" else kind, fs, tols, seg)
    assert [bytes(e["data"][:4]) for e in encs if e["nlay"]] == [b"WRS1", b"WRS2", b"WRS3", b"WRS3", b"WRS3"] and encs[4]["nlay"] == 0
    recs = decode_singles(ctx, "f64" if kind == "dev" else kind, sub, encs)
    before = launches()
    outs, tm = decode_mixed(ctx, kind, sub, encs)
    assert launches() - before == 2  # the plain jobs, the stranded jobs
    for i in range(len(sub)):
        assert bits_equal(outs[i], recs[i]), (kind, "field %d" % i)
    assert tm["rangecoder"] > 0
    if kind != "f64":
        return
    # the old batch decode launches once per plane index, and refuses the WRS3 fields as before
    plain = [encs[0], encs[1], encs[4]]
    before = launches()
    outs = [np.empty_like(sub[0]) for _ in plain]
    ctx.decode_host_seg_batch(outs, plain)
    assert launches() - before == max(e["nlay"] for e in plain)
    assert bits_equal(outs[0], recs[0]) and bits_equal(outs[1], recs[1]) and bits_equal(outs[2], recs[4])
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_batch([np.empty_like(f) for f in sub], encs)
    assert "error -3" in str(e.value) and "field 2" in str(e.value)


def test_more_than_1024_jobs(ctx):
    """fields x planes beyond WR_SEG_BATCH_MAX: the jobs of a kind go in launches of at most 1024 each"""
    shape, seg, K = SHAPES[1]
    nx, ny, nz = shape
    base = [synth.field(nx, ny, nz, seed=300 + i) for i in range(4)]
    encs3 = singles(ctx, "f64", base, [1e-7] * 4, 1, seg, None, K)
    encs1 = singles(ctx, "f64", base[:2], [1e-7] * 2, 1, seg, None, None)
    recs3, recs1 = decode_singles(ctx, "f64", base, encs3), decode_singles(ctx, "f64", base[:2], encs1)
    nlay3 = [e["nlay"] for e in encs3]
    count = api.SEG_BATCH_MAX // min(nlay3) + 1
    assert count <= api.SEG_BATCH_MAX
    encs = [encs3[i % 4] for i in range(count)] + encs1
    want = [recs3[i % 4] for i in range(count)] + recs1
    stranded = sum(nlay3[i % 4] for i in range(count))
    plain = sum(e["nlay"] for e in encs1)
    assert stranded > api.SEG_BATCH_MAX and 0 < plain <= api.SEG_BATCH_MAX  # the test is about more jobs than one launch takes
    outs = [np.empty_like(base[0]) for _ in encs]
    before = launches()
    ctx.decode_host_seg_batch_mixed(outs, encs)
    assert launches() - before == -(-stranded // api.SEG_BATCH_MAX) + 1
    for i in range(len(encs)):
        assert bits_equal(outs[i], want[i]), "field %d" % i


# ---- refusals: the context goes on working after each ------------------------------------------------------------------------
def test_refusals(ctx):
    shape, seg, K = SHAPES[1]
    fs, tols = batch_fields(shape)
    want = singles(ctx, "f64", fs, tols, 1, seg, None, K)
    recs = decode_singles(ctx, "f64", fs, want)

    def good_batch(what):
        got, _ = batch(ctx, "f64", fs, tols, 1, seg, 0, K)
        for i in range(NFIELDS):
            same_record(got[i], want[i], (what, i))
        outs, _ = decode_mixed(ctx, "f64", fs, got)
        for i in range(NFIELDS):
            assert bits_equal(outs[i], recs[i]), (what, i)

    def refused(code, fn, *names):
        with pytest.raises(api.WaveRangeError) as e:
            fn()
        assert ("error %d" % code) in str(e.value) and all(s in str(e.value) for s in names), str(e.value)

    good_batch("at first")
    encs, _ = ctx.encode_host_seg_batch_strands([fs[1]] * 4, tols[1], 1, seg, 0, K)  # (the same field four times is a batch like any other)
    for e in encs:
        same_record(e, want[1], "one field four times")
    # the number of fields
    for many in ([], [fs[0]] * (api.SEG_BATCH_MAX + 1)):
        refused(-1, lambda: ctx.encode_host_seg_batch_strands(many, 1e-3, 1, seg, 0, K))
        refused(-1, lambda: ctx.decode_host_seg_batch_mixed([np.empty_like(fs[0]) for _ in many], [want[0]] * len(many)))
    good_batch("after a bad number of fields")
    # a bad K
    for bad_k in (3, 64):
        refused(-1, lambda: ctx.encode_host_seg_batch_strands(fs, tols, 1, seg, 0, bad_k), "strands")
    refused(-1, lambda: ctx.encode_host_seg_batch_strands(fs, tols, 1, 48, 0, 4), "strands")  # 16 K > seg
    good_batch("after a bad K")
    # field 4's buffer one byte short
    j = 4
    caps = [e["ntot_enc"] + 64 for e in want]
    caps[j] = want[j]["ntot_enc"] - 1
    refused(-5, lambda: ctx.encode_host_seg_batch_strands(fs, tols, 1, seg, 0, K, caps=caps), "field %d" % j)
    good_batch("after an overflow")
    # a flipped length word of a record in field 4's second plane: the kernel counts it, no dequantizer runs, every output
    # buffer is untouched
    assert want[j]["nlay"] >= 2
    front, _ = index_of(want[j]["data"][want[j]["len_enc_vec"][0]:])
    bad = [dict(e) for e in want]
    bad[j] = dict(want[j], data=want[j]["data"].copy())
    bad[j]["data"][want[j]["len_enc_vec"][0] + front + 4] ^= 4  # slen[0] of record 0 of plane 1
    outs = [np.full_like(f, 1234.5) for f in fs]
    refused(-4, lambda: ctx.decode_host_seg_batch_mixed(outs, bad), "field %d" % j, "plane 1")
    assert all(np.all(o == 1234.5) for o in outs)
    good_batch("after a flipped record byte")
    # ... and a header or an index of that plane: refused on the host, nothing is launched
    before = launches()
    for at, flip, what in ((0, 1, "magic"), (4, 1, "segment"), (8, 1, "segment count"), (20, 4, "add up")):  # (the last: an index length)
        bad[j] = dict(want[j], data=want[j]["data"].copy())
        bad[j]["data"][want[j]["len_enc_vec"][0] + at] ^= flip
        outs = [np.full_like(f, 1234.5) for f in fs]
        refused(-4, lambda: ctx.decode_host_seg_batch_mixed(outs, bad), "field %d" % j, "plane 1", what)
        assert all(np.all(o == 1234.5) for o in outs), what
    assert launches() == before
    good_batch("after a flipped header")
    # a context that keeps residuals
    ctx.set_keep_residual(True)
    try:
        refused(-3, lambda: ctx.encode_host_seg_batch_strands(fs, tols, 1, seg, 0, K))
    finally:
        ctx.set_keep_residual(False)
    good_batch("after keep_residual")
    # the old names keep their refusals
    refused(-3, lambda: ctx.encode_host_seg_batch(fs, tols, 1, seg, strands=8))
