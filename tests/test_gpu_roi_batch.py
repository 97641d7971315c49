"""Region decode across a batch of fields (include/waverange_amd.h, "Region decode across a batch of fields").

The specification is the whole oracle: region i of field f of a batch call is, bit for bit, what the many-region call returns
for field f alone -- and hence the crop of D(r, p), which tests/test_gpu_lowres.py builds on the CPU from the oracle's
dequantiser and transform.  Every comparison of values is equality of bit patterns; there is no tolerance anywhere.  No test
damages a segment's payload: every refusal here is decided on the host."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401
import coder_cases as cc
from roi_multi_cases import carry
from test_gpu_lowres import expected, field, same_bits, split_planes
from test_gpu_roi import crop
from oracle.loader import Oracle
from waverange_amd import api

pytestmark = pytest.mark.gpu

SHAPE = (40, 36, 44)  # four levels, odd halvings (5 -> 3, 9 -> 5, 11 -> 6), 63 segments a plane at seg = 1008
FLAT = (1, 50, 300)   # a degenerate axis
LEVELS = range(5)


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def launches():
    return api.stat(api.STAT_ROI_CODER_LAUNCHES)


def stats():
    return api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()


# ---- 1. the kernel, stage level ------------------------------------------------------------------------------------------
_BLOBS = {}


def coded(kind, n, seg, K):
    """(blob, the plane's symbols by the host reference): K = 0 is WRS1, otherwise WRS3 in the natural order.  Shared, never
    written to."""
    key = (kind, n, seg, K)
    if key not in _BLOBS:
        p = cc.plane(kind, n, seg, K)
        blob = api.seg_encode_host_ref_strands(p, seg=seg, strands=K) if K else api.seg_encode_host_ref(p, seg)
        assert bytes(blob[:4]) == (b"WRS3" if K else b"WRS1")
        ref = api.seg_decode_host_ref_blocked(blob, (1, 1, n)) if K else api.seg_decode_host_ref(blob, n)
        assert np.array_equal(ref, p)
        _BLOBS[key] = (blob, ref)
    return _BLOBS[key]


def job(blob, ref, n, seg, ids):
    """(blob, n, ids, the plane expected): the listed segments hold the reference's symbols, every other byte its 0xEE fill"""
    ids = np.asarray(ids, dtype=np.uint32)
    want = np.full(n, 0xEE, dtype=np.uint8)
    for k in ids:
        want[int(k) * seg:(int(k) + 1) * seg] = ref[int(k) * seg:(int(k) + 1) * seg]
    return blob, n, ids, want


def run_jobs(ctx, jobs, what):
    got, bad = ctx.seg_decode_lists_mixed([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert bad == [0] * len(jobs), (what, bad)
    for i, (j, g) in enumerate(zip(jobs, got)):
        assert np.array_equal(g, j[3]), (what, i, np.flatnonzero(g != j[3])[:8])


def lists_for(nseg, K):
    """every segment, the evens, first and last only, one id, empty, and the workgroup edge: 64 / K and 64 / K + 1 segments"""
    edge = 64 // K
    return [np.arange(nseg), np.arange(0, nseg, 2), [0, nseg - 1], [nseg // 2], [], np.arange(min(edge, nseg)), np.arange(min(edge + 1, nseg))]


@pytest.mark.parametrize("kind", cc.CODEC_KINDS)
def test_kernel_stranded_jobs(ctx, kind):
    for seg in (1008, 4096):
        for n in (65536, 300000):  # 65536 = 16 * 4096: no short segment at seg 4096; a short last one everywhere else
            jobs = []
            for K in (1, 4, 16, 32):
                if not cc.valid(kind, seg, K, n):
                    continue
                blob, ref = coded(kind, n, seg, K)
                jobs += [job(blob, ref, n, seg, ids) for ids in lists_for(-(-n // seg), K)]
            assert jobs
            run_jobs(ctx, jobs, (kind, seg, n))


def test_kernel_65_segments_at_k1(ctx):
    blob, ref = coded("patchwork", 300000, 1008, 1)
    run_jobs(ctx, [job(blob, ref, 300000, 1008, np.arange(65))], "65 at K = 1")
    run_jobs(ctx, [job(blob, ref, 300000, 1008, np.arange(64))], "64 at K = 1")


def test_kernel_mixed_formats_in_one_call(ctx):
    """WRS1, WRS2 (brick 8), WRS3 with two different K; an empty job between two full ones; WRS3 jobs before and after the
    WRS1 jobs; job edges that fall inside a wave for WRS1 and on a wave's edge for WRS3."""
    rng = np.random.default_rng(5)
    n, seg = 300000, 4096
    nseg = -(-n // seg)
    w1, r1 = coded("patchwork", n, seg, 0)
    k4, r4 = coded("patchwork", n, seg, 4)
    k16, r16 = coded("adversarial_K/2_first", 65536, 1008, 16)
    shape = (20, 33, 47)
    nb = int(np.prod(shape))
    plane = rng.integers(0, 7, nb).astype(np.uint8)
    w2 = api.seg_encode_host_ref_blocked(plane, shape, 4, 8, 1008)
    assert bytes(w2[:4]) == b"WRS2"
    order = api.seg_decode_host_ref_blocked(w2, shape, 4)[api.blocked_order(shape, 4, 8)]  # what the coder kernel sees
    jobs = [
        job(k4, r4, n, seg, np.arange(0, nseg, 2)),       # WRS3 first: 37 * 4 = 148 lanes, rounded to 192
        job(w1, r1, n, seg, [0, 5, nseg - 1]),            # 3 lanes: the next WRS1 job starts inside the wave
        job(k16, r16, 65536, 1008, []),                   # an empty job between two full ones
        job(w1, r1, n, seg, np.arange(nseg)),
        job(w2, order, nb, 1008, np.arange(0, -(-nb // 1008), 3)),
        job(k16, r16, 65536, 1008, np.arange(5)),         # 80 lanes, rounded to 128
        job(k4, r4, n, seg, [nseg - 1]),                  # the short last segment alone, WRS3 last
    ]
    l0 = launches()
    run_jobs(ctx, jobs, "mixed")
    assert launches() == l0  # (the stage call is no region decode)
    run_jobs(ctx, jobs[::-1], "mixed, reversed")
    run_jobs(ctx, [jobs[2]], "one empty job")
    # wr_dev_seg_decode_lists keeps refusing WRS3
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_lists([k4], [n], [np.arange(2, dtype=np.uint32)])
    assert "error -5" in str(e.value) or "WRS3" in str(e.value), str(e.value)


def test_kernel_1024_one_segment_jobs(ctx):
    rng = np.random.default_rng(6)
    jobs = []
    for j in range(api.SEG_BATCH_MAX):
        p = rng.integers(0, 256, 16).astype(np.uint8)
        blob = api.seg_encode_host_ref_strands(p, seg=16, strands=1) if j % 3 else api.seg_encode_host_ref(p, 16)
        jobs.append(job(blob, p, 16, 16, [0] if j % 5 else []))
    run_jobs(ctx, jobs, "1024")
    L = api.lib()
    assert L.wr_dev_seg_decode_lists_mixed(ctx.h, api.SEG_BATCH_MAX + 1, None, None, None, None, None, None, None) == -1
    assert L.wr_dev_seg_decode_lists_mixed(ctx.h, 0, None, None, None, None, None, None, None) == -1
    assert L.wr_dev_seg_decode_lists_mixed(ctx.h, 1, None, None, None, None, None, None, None) == -1


# ---- 2. the whole path against the per-field calls -----------------------------------------------------------------------
# Region sets in the spirit of roi_multi_cases.SETS (whose boxes belong to other shapes), at level 0 and carried to a coarser
# level by its rule: one-sample corners, overlapping and repeated boxes, a full z-plane, the whole box.
REGION_SETS = {
    SHAPE: {
        "corners": [((0, 1), (0, 1), (0, 1)), ((39, 40), (35, 36), (43, 44)), ((0, 1), (35, 36), (0, 1))],
        "overlap": [((10, 20), (8, 20), (4, 30)), ((15, 25), (0, 36), (20, 44)), ((10, 20), (8, 20), (4, 30))],
        "zplane": [((17, 18), (0, 36), (0, 44)), ((3, 5), (7, 9), (11, 13))],
        "whole": [((0, 40), (0, 36), (0, 44))],
    },
    FLAT: {
        "flat": [((0, 1), (10, 20), (140, 160)), ((0, 1), (0, 50), (0, 300)), ((0, 1), (49, 50), (299, 300))],
    },
}
ORACLE_SET = {SHAPE: "overlap", FLAT: "flat"}

_FIELDS = {}


def fields_of(ctx, shape):
    """The six coded fields of a shape with their natural-order planes; shared, never written to."""
    if shape not in _FIELDS:
        def one(seed, tol, **kw):
            f = field(shape, seed=seed)
            enc, _ = ctx.encode_host_seg(f, tol, 1, 1008, **kw)
            enc["data"] = enc["data"].copy()
            plain, _ = ctx.encode_host_seg(f, tol, 1, 1008)
            planes = [api.seg_decode_host_ref(b, f.size) for b in split_planes(dict(plain, data=plain["data"].copy()))]
            assert plain["nlay"] == enc["nlay"]
            return dict(enc=enc, planes=planes, D={})
        flat, _ = ctx.encode_host_seg(np.full(shape, 3.25), 1e-6)
        assert flat["nlay"] == 0 and flat["ntot_enc"] == 0
        fs = [one(41, 1e-3), one(42, 1e-6), one(43, 1e-4, brick=8), one(44, 1e-5, strands=4), one(45, 1e-3, strands=16, brick=8),
              dict(enc=dict(flat, data=flat["data"].copy()), planes=[], D={}, const=3.25)]
        assert [bytes(f["enc"]["data"][:4]) for f in fs[:5]] == [b"WRS1", b"WRS1", b"WRS2", b"WRS3", b"WRS3"]
        assert fs[1]["enc"]["nlay"] > fs[0]["enc"]["nlay"] >= 1
        _FIELDS[shape] = fs
    return _FIELDS[shape]


def batch_all_ways(ctx, shape, level, rois, encs, p):
    h64 = ctx.decode_host_seg_rois_batch(shape, level, rois, encs, p)
    h32 = ctx.decode_host_seg_rois_batch(shape, level, rois, encs, p, dtype=np.float32)
    offs = api.roi_multi_offsets(shape, level, rois)
    T = int(offs[-1])
    buf = ctx.alloc(max(8 * T * len(encs), 16))
    try:
        ctx.decode_seg_rois_batch(buf, shape, level, rois, encs, p)
        flat = buf.download(np.float64, T * len(encs))
    finally:
        buf.free()
    d64 = [[flat[f * T + offs[i]:f * T + offs[i + 1]].reshape(api.roi_shape(r)) for i, r in enumerate(rois)] for f in range(len(encs))]
    assert all(a.base is h64[0][0].base for per in h64 for a in per)  # views of one buffer
    return h64, h32, d64


_SINGLES = {}


def single(ctx, shape, key, level, rois, f, p):
    """decode_host_seg_rois of one field alone, computed once per case: (float64, float32)"""
    k = (shape, key, level, p)
    if k not in _SINGLES:
        if "const" in f and p > 0:
            _SINGLES[k] = None  # (the per-field call refuses max_planes above the planes of the stream: nlay is 0)
        else:
            _SINGLES[k] = (ctx.decode_host_seg_rois(shape, level, rois, f["enc"], p), ctx.decode_host_seg_rois(shape, level, rois, f["enc"], p, dtype=np.float32))
    return _SINGLES[k]


def check_batch(ctx, oracle, shape, name, order, what):
    fs = fields_of(ctx, shape)
    for level in LEVELS:
        rois = [carry(shape, level, r) for r in REGION_SETS[shape][name]]
        for p in (0, 1):
            # (a constant field has no planes: with max_planes = 1 the per-field call refuses it, and so does the batch)
            idx = [f for f in order if not ("const" in fs[f] and p > 0)]
            encs = [fs[f]["enc"] for f in idx]
            h64, h32, d64 = batch_all_ways(ctx, shape, level, rois, encs, p)
            for at, f in enumerate(idx):
                one64, one32 = single(ctx, shape, (name, f), level, rois, fs[f], p)
                for i, r in enumerate(rois):
                    assert same_bits(h64[at][i], one64[i]), (what, level, p, f, i, "host")
                    assert same_bits(d64[at][i], one64[i]), (what, level, p, f, i, "device")
                    assert same_bits(h32[at][i], one32[i]), (what, level, p, f, i, "fp32")
                if name == ORACLE_SET[shape] and "const" not in fs[f]:
                    used = p or fs[f]["enc"]["nlay"]
                    if (level, used) not in fs[f]["D"]:
                        fs[f]["D"][level, used] = expected(oracle, fs[f]["planes"], fs[f]["enc"], shape, level, used)
                    for i, r in enumerate(rois):
                        assert same_bits(h64[at][i], crop(fs[f]["D"][level, used], r)), (what, level, p, f, i, "oracle")
                elif "const" in fs[f]:
                    assert all(np.all(a == 3.25) for a in h64[at]) and all(np.all(a == np.float32(3.25)) for a in h32[at])


@pytest.mark.parametrize("name", list(REGION_SETS[SHAPE]))
def test_values(ctx, oracle, name):
    check_batch(ctx, oracle, SHAPE, name, range(6), name)


def test_values_degenerate_shape(ctx, oracle):
    check_batch(ctx, oracle, FLAT, "flat", range(6), "flat")


def test_values_reversed_order(ctx, oracle):
    check_batch(ctx, oracle, SHAPE, "overlap", range(5, -1, -1), "reversed")


def test_constant_field_and_max_planes(ctx):
    """max_planes = 1 with a constant field in the batch: refused as the per-field call refuses it, naming the field"""
    fs = fields_of(ctx, SHAPE)
    rois = REGION_SETS[SHAPE]["corners"]
    with pytest.raises(api.WaveRangeError):
        ctx.decode_host_seg_rois(SHAPE, 0, rois, fs[5]["enc"], 1)
    s0 = stats()
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, [fs[0]["enc"], fs[5]["enc"]], 1)
    assert "error -1" in str(e.value) and "field 1: region 0: " in str(e.value), str(e.value)
    assert stats() == s0


# ---- 3. counters ---------------------------------------------------------------------------------------------------------
def test_counters(ctx):
    fs = fields_of(ctx, SHAPE)
    rois = REGION_SETS[SHAPE]["overlap"]

    def moved(idx, p=0):
        s0 = stats()
        tm = {}
        ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, [fs[f]["enc"] for f in idx], p, timings=tm)
        s1 = stats()
        return tuple(b - a for a, b in zip(s0, s1)), tm

    def singles_moved(idx, p=0):
        total = 0
        for f in idx:
            b0 = api.stat(api.STAT_ROI_BYTES_UP)
            ctx.decode_host_seg_rois(SHAPE, 0, rois, fs[f]["enc"], p)
            total += api.stat(api.STAT_ROI_BYTES_UP) - b0
        return total

    def listed(idx, p=0):
        total = 0
        for f in idx:
            enc = fs[f]["enc"]
            if not enc["nlay"]:
                continue
            brick = int(np.frombuffer(enc["data"][12:16].tobytes(), dtype=np.uint32)[0]) if bytes(enc["data"][:4]) != b"WRS1" else 0
            total += api.seg_roi_segments_multi(SHAPE, 0, rois, 1008, brick=brick or None).size * (p or enc["nlay"])
        return total

    for idx, want in (((0, 1), 1), ((3, 4), 1), ((0, 1, 2, 3, 4, 5), 2), ((5, 5), 0), ((2,), 1)):
        for p in (0, 1) if 5 not in idx else (0,):
            (ds, db, dl), tm = moved(idx, p)
            assert dl == want, (idx, p, dl)
            assert ds == listed(idx, p), (idx, p, ds)
            assert db == singles_moved(idx, p), (idx, p, db)
            if want:
                assert tm["rangecoder"] > 0 and tm["plane_coder_s"][0] == tm["rangecoder"] and not any(tm["plane_coder_s"][1:])
            else:
                assert tm["rangecoder"] == 0 and ds == 0 and db == 0


# ---- 4. refusals: all decided on the host, nothing launched ----------------------------------------------------------------
def raw_call(ctx, fn, out_ptr, shape, level, p, rois, encs, nfields=None, null=()):
    nz, ny, nx = shape
    infos = (api.EncInfo * max(len(encs), 1))(*[api.EncInfo.from_dict(e) for e in encs])
    datas = [np.ascontiguousarray(e["data"] if e["data"].size else np.zeros(1, np.uint8)) for e in encs]
    ptrs = (api.C.c_void_p * max(len(encs), 1))(*[d.ctypes.data for d in datas])
    lens = (api.C.c_size_t * max(len(encs), 1))(*[d.size for d in datas])
    args = dict(infos=infos, ptrs=ptrs, lens=lens, rois=api._boxes(rois))
    for k in null:
        args[k] = None
    return fn(ctx.h, out_ptr, len(encs) if nfields is None else nfields, nx, ny, nz, level, p, args["rois"], len(rois), args["infos"], args["ptrs"], args["lens"], None)


def test_refusals(ctx):
    fs = fields_of(ctx, SHAPE)
    encs = [f["enc"] for f in fs]
    rois = REGION_SETS[SHAPE]["overlap"]
    T = int(api.roi_multi_offsets(SHAPE, 0, rois)[-1])
    L = api.lib()
    out = np.full(6 * T, 1234.5)
    d_out = ctx.alloc(out.nbytes)
    s0 = stats()
    try:
        for fn, ptr in ((L.wr_decode_host_seg_roi_batch, out.ctypes.data), (L.wr_decode_host_seg_roi_batch_f32, out.ctypes.data), (L.wr_decode_device_seg_roi_batch, d_out.ptr)):
            assert raw_call(ctx, fn, ptr, SHAPE, 0, 0, rois, encs, nfields=0) == -1
            assert raw_call(ctx, fn, ptr, SHAPE, 0, 0, rois, encs, nfields=-3) == -1
            for k in ("infos", "ptrs", "lens", "rois"):
                assert raw_call(ctx, fn, ptr, SHAPE, 0, 0, rois, encs, null=(k,)) == -1, k
            assert raw_call(ctx, fn, None, SHAPE, 0, 0, rois, encs) == -1
            assert raw_call(ctx, fn, ptr, SHAPE, 5, 0, rois, encs) == -1
            # a bad region among good ones
            bad_rois = [rois[0], rois[1], ((0, 1), (0, 1), (0, 45)), rois[2]]
            assert raw_call(ctx, fn, ptr, SHAPE, 0, 0, bad_rois, encs) == -1
            assert L.wr_last_error().decode().startswith("field 0: region 2: "), L.wr_last_error().decode()
        # more than WR_SEG_BATCH_MAX jobs: a field of eight planes, 129 times
        f16, _ = ctx.encode_host_seg(field(SHAPE), 1e-16, 1, 1008)
        f16["data"] = f16["data"].copy()
        assert f16["nlay"] == api.NLAYMAX
        many = [f16] * (api.SEG_BATCH_MAX // api.NLAYMAX + 1)
        big = np.full(len(many) * T, 1234.5)
        assert raw_call(ctx, L.wr_decode_host_seg_roi_batch, big.ctypes.data, SHAPE, 0, 0, rois, many) == -1
        assert "too many jobs" in L.wr_last_error().decode()
        assert np.all(big == 1234.5)
        # ... while 128 of them, 1024 jobs, are a call like any other
        got = ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, many[:-1])
        assert stats()[2] - s0[2] == 1
        want = ctx.decode_host_seg_rois(SHAPE, 0, rois, f16)
        assert all(same_bits(a, b) for per in (got[0], got[-1]) for a, b in zip(per, want))
        s0 = stats()
        # in field 3 (WRS3, K = 4: a 20-byte header, then the index), the second plane's magic, seg, segment count and one index
        # length: refused with the field, the plane and the word tests/test_gpu_seg_batch.py uses for that damage (the length
        # moves by 4: a record that is no multiple of 4 bytes has a message of its own), in all three forms of the call
        enc3 = encs[3]
        assert enc3["nlay"] >= 2 and bytes(enc3["data"][:4]) == b"WRS3"
        at = enc3["len_enc_vec"][0]
        out32 = np.full(6 * T, 1234.5, dtype=np.float32)
        d_out.upload(out)
        seen = set()
        for off, flip, word in ((0, 1, "magic"), (4, 1, "segment length"), (8, 1, "segment count"), (20, 4, "add up")):
            bad = dict(enc3, data=enc3["data"].copy())
            bad["data"][at + off] ^= flip
            damaged = encs[:3] + [bad] + encs[4:]
            with pytest.raises(api.WaveRangeError) as e1:  # the text behind the field is the per-field call's
                ctx.decode_host_seg_rois(SHAPE, 0, rois, bad)
            for form, call in (("f64", lambda: ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, damaged, out=out)),
                               ("f32", lambda: ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, damaged, dtype=np.float32, out=out32)),
                               ("device", lambda: ctx.decode_seg_rois_batch(d_out, SHAPE, 0, rois, damaged))):
                with pytest.raises(api.WaveRangeError) as e:
                    call()
                msg = str(e.value)
                assert "error -4" in msg and "field 3: " in msg and "plane 1" in msg and word in msg, (form, word, msg)
                assert msg.split("field 3: ", 1)[1] == str(e1.value).split(": ", 1)[1], (form, msg, str(e1.value))
            seen.add(msg)
            assert np.all(out == 1234.5) and np.all(out32 == np.float32(1234.5)), word
            assert np.all(d_out.download(np.float64, 6 * T) == 1234.5), word
        assert len(seen) == 4  # four damages, four causes
        assert stats() == s0
    finally:
        d_out.free()
    # a good batch afterwards
    got = ctx.decode_host_seg_rois_batch(SHAPE, 0, rois, encs)
    for f in range(6):
        want = ctx.decode_host_seg_rois(SHAPE, 0, rois, encs[f])
        assert all(same_bits(a, b) for a, b in zip(got[f], want)), f
