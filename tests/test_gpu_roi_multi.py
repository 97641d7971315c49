"""Region decode of segmented streams, many regions per call (include/waverange_amd.h, "Region decode, many regions per call").

The specification is the whole oracle: region i of a multi-region call is, bit for bit, what the single-region call returns for
that region alone -- and hence the crop of D(r, p), which tests/test_gpu_lowres.py builds on the CPU from the oracle's
dequantiser and transform.  Every comparison of values is equality of bit patterns; there is no tolerance anywhere."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401
from roi_multi_cases import SETS, regions_at, single_lists, union_of
from test_gpu_lowres import recut, same_bits, split_planes
from test_gpu_roi import D, crop, index_of, stream
from oracle.loader import Oracle
from waverange_amd import api

pytestmark = pytest.mark.gpu

TOLS = [1e-3, 1e-6]
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


def multi_all_ways(ctx, shape, level, rois, enc, p):
    """(float64 from the host call, float32 from the fp32 call, float64 from the device-output call): a list of regions each"""
    h64 = ctx.decode_host_seg_rois(shape, level, rois, enc, p)
    h32 = ctx.decode_host_seg_rois(shape, level, rois, enc, p, dtype=np.float32)
    offs = api.roi_multi_offsets(shape, level, rois)
    buf = ctx.alloc(max(8 * int(offs[-1]), 16))
    try:
        ctx.decode_seg_rois(buf, shape, level, rois, enc, p)
        flat = buf.download(np.float64, int(offs[-1]))
    finally:
        buf.free()
    d64 = [flat[offs[i]:offs[i + 1]].reshape(api.roi_shape(r)) for i, r in enumerate(rois)]
    assert all(a.base is h64[0].base for a in h64) and all(a.base is h32[0].base for a in h32)  # views of one buffer
    return h64, h32, d64


def singles(ctx, shape, level, rois, enc, p):
    """Per region (float64, float32) of the single-region calls; a repeated region is decoded once."""
    seen = {}
    for r in rois:
        if r not in seen:
            a, b = np.empty(api.roi_shape(r)), np.empty(api.roi_shape(r), dtype=np.float32)
            ctx.decode_host_seg_roi(a, shape, level, r, enc, p)
            ctx.decode_host_seg_roi_f32(b, shape, level, r, enc, p)
            seen[r] = (a, b)
    return [seen[r] for r in rois]


def check_against_singles(ctx, shape, level, rois, enc, p, what):
    h64, h32, d64 = multi_all_ways(ctx, shape, level, rois, enc, p)
    for i, (one64, one32) in enumerate(singles(ctx, shape, level, rois, enc, p)):
        assert same_bits(h64[i], one64), (what, level, p, i, "host")
        assert same_bits(d64[i], one64), (what, level, p, i, "device")
        assert same_bits(h32[i], one32), (what, level, p, i, "fp32")
    return h64, h32, d64


def check_against_oracle(got, oracle, s, shape, level, rois, p, what):
    h64, h32, d64 = got
    full = D(oracle, s, shape, level, p)
    for i, r in enumerate(rois):
        want = crop(full, r)
        assert same_bits(h64[i], want), (what, level, p, i, "host")
        assert same_bits(d64[i], want), (what, level, p, i, "device")
        assert same_bits(h32[i], want.astype(np.float32)), (what, level, p, i, "fp32")


# ---- 1. the kernel, stage level ------------------------------------------------------------------------------------------
def sym_plane(rng, n):
    """Symbols as a quantized plane has them: mostly a few values, some noise."""
    p = rng.integers(120, 136, size=n, dtype=np.int64)
    noisy = rng.random(n) < 0.05
    p[noisy] = rng.integers(0, 256, size=int(noisy.sum()))
    return p.astype(np.uint8)


def job(rng, n, seg, pick):
    """(blob, n, ids, the symbols expected in the plane): `pick` maps nseg to the ascending ids of the list."""
    plane = sym_plane(rng, n)
    blob = api.seg_encode_host_ref(plane, seg)
    nseg = -(-n // seg)
    ids = np.asarray(pick(nseg), dtype=np.uint32)
    ref = api.seg_decode_host_ref(blob, n)
    want = np.full(n, 0xEE, dtype=np.uint8)
    for k in ids:
        want[int(k) * seg:(int(k) + 1) * seg] = ref[int(k) * seg:(int(k) + 1) * seg]
    return blob, n, ids, want


def run_jobs(ctx, jobs, what):
    total = sum(j[2].size for j in jobs)
    got, bad = ctx.seg_decode_lists([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert bad == [0] * len(jobs), (what, bad)
    for i, (j, g) in enumerate(zip(jobs, got)):
        assert np.array_equal(g, j[3]), (what, i, total, np.flatnonzero(g != j[3])[:8])
    return total


def every(nseg):
    return np.arange(nseg)


def evens(nseg):
    return np.arange(0, nseg, 2)


def first(count):
    return lambda nseg: np.arange(min(count, nseg))


def test_kernel_one_job(ctx):
    rng = np.random.default_rng(1)
    # a list that is every segment, the short last segment among them (300 000 = 73 * 4096 + 992)
    assert run_jobs(ctx, [job(rng, 300000, 4096, every)], "every") == 74
    # the short last segment listed alone, and not listed
    run_jobs(ctx, [job(rng, 300000, 4096, lambda nseg: [nseg - 1])], "last only")
    run_jobs(ctx, [job(rng, 300000, 4096, lambda nseg: np.arange(nseg - 1))], "all but the last")
    # totals of exactly 64 and of 65: one full wave, and one lane of a second block
    assert run_jobs(ctx, [job(rng, 70000, 1008, first(64))], "64") == 64
    assert run_jobs(ctx, [job(rng, 70000, 1008, first(65))], "65") == 65
    run_jobs(ctx, [job(rng, 130000, 59904, lambda nseg: [1])], "seg 59904")


def test_kernel_eight_jobs(ctx):
    """Jobs of different n and seg, an empty list between two others, job boundaries inside a wave, a total that is no multiple
    of 64, a plane whose last segment is short and listed next to one where it is not."""
    rng = np.random.default_rng(2)
    jobs = [
        job(rng, 50000, 1008, evens),                          # 25 lanes: the next job starts inside the first wave
        job(rng, 300000, 4096, lambda nseg: [0, 5, nseg - 1]),  # the short last segment listed
        job(rng, 9000, 1008, lambda nseg: []),                 # an empty list between two others
        job(rng, 200000, 59904, every),                        # 4 lanes
        job(rng, 123456, 4096, lambda nseg: np.arange(nseg - 1)),  # the short last segment not listed
        job(rng, 70000, 1008, first(40)),                      # crosses the end of the first wave
        job(rng, 17, 1008, every),                             # one short segment
        job(rng, 65536, 4096, every),                          # exact multiple of seg
    ]
    total = run_jobs(ctx, jobs, "eight")
    assert total == 25 + 3 + 0 + 4 + 30 + 40 + 1 + 16 and total % 64 != 0
    # an empty list first and last
    run_jobs(ctx, [job(rng, 9000, 1008, lambda nseg: []), jobs[1], job(rng, 5000, 1008, lambda nseg: [])], "empty ends")


def test_kernel_a_wrs2_blob_among_wrs1_blobs(ctx):
    rng = np.random.default_rng(3)
    shape, seg = (20, 33, 47), 1008
    n = int(np.prod(shape))
    plane = sym_plane(rng, n)
    blob = api.seg_encode_host_ref_blocked(plane, shape, 4, 16, seg)
    assert bytes(blob[:4]) == b"WRS2"
    stream_order = api.seg_decode_host_ref_blocked(blob, shape, 4)[api.blocked_order(shape, 4, 16)]  # what the coder kernel sees
    ids = evens(-(-n // seg)).astype(np.uint32)
    want = np.full(n, 0xEE, dtype=np.uint8)
    for k in ids:
        want[int(k) * seg:(int(k) + 1) * seg] = stream_order[int(k) * seg:(int(k) + 1) * seg]
    run_jobs(ctx, [job(rng, 40000, 4096, evens), (blob, n, ids, want), job(rng, 30000, 1008, first(7))], "wrs2")


def test_kernel_refusals(ctx):
    rng = np.random.default_rng(4)
    good = job(rng, 50000, 1008, evens)
    nseg = -(-50000 // 1008)
    for ids in ([3, 2], [1, 1], [nseg], [0, nseg + 5]):
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_lists([good[0], good[0]], [good[1], good[1]], [good[2], np.asarray(ids, dtype=np.uint32)])
        assert "error -1" in str(e.value) and "job 1:" in str(e.value), str(e.value)
    bad = good[0].copy()
    bad[12] ^= 1  # an index word: the lengths no longer add up
    with pytest.raises(api.WaveRangeError) as e:
        ctx.seg_decode_lists([good[0], bad], [good[1], good[1]], [good[2], good[2]])
    assert "error -4" in str(e.value) and "job 1:" in str(e.value), str(e.value)
    L = api.lib()
    assert L.wr_dev_seg_decode_lists(ctx.h, 0, None, None, None, None, None, None, None) == -1
    assert L.wr_dev_seg_decode_lists(ctx.h, api.SEG_BATCH_MAX + 1, None, None, None, None, None, None, None) == -1
    assert L.wr_dev_seg_decode_lists(ctx.h, 1, None, None, None, None, None, None, None) == -1
    run_jobs(ctx, [good], "after the refusals")


# ---- 2. values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("name", list(SETS))
def test_values(ctx, oracle, name, tol):
    shape = SETS[name][0]
    s = stream(ctx, shape, tol)
    enc = s["enc"]
    for level in LEVELS:
        rois = regions_at(name, level)
        for p in sorted({1, enc["nlay"]}):
            got = check_against_singles(ctx, shape, level, rois, enc, p, (name, tol))
            check_against_oracle(got, oracle, s, shape, level, rois, p, (name, tol))
    # max_planes = 0 means all of them
    rois = regions_at(name, 0)
    for a, b in zip(ctx.decode_host_seg_rois(shape, 0, rois, enc), ctx.decode_host_seg_rois(shape, 0, rois, enc, enc["nlay"])):
        assert same_bits(a, b)


def test_windows_of_set_s_take_both_inverse_paths():
    shape, rois = SETS["S"]
    wins = [tuple(b - a for a, b in api.roi_window(shape, 0, r)) for r in rois]
    assert wins[0] == (144, 144, 144) and wins[1] == (64, 64, 64) and wins[4] == (75, 144, 203)
    assert api.fused_plan(wins[0], inverse=True)["used"] and not api.fused_plan(wins[4], inverse=True)["used"]


def test_stage_level_from_planes(ctx, oracle):
    name = "T"
    shape = SETS[name][0]
    s = stream(ctx, shape, 1e-6)
    enc, planes, n = s["enc"], s["planes"], s["f"].size
    info = api.EncInfo.from_dict(enc)
    pitch = api.lib().wr_plane_pitch(n)
    host = np.zeros(pitch * enc["nlay"], dtype=np.uint8)
    for l, q in enumerate(planes):
        host[l * pitch:l * pitch + n] = q
    d_planes, d_out = ctx.to_device(host), ctx.alloc(8 * n)
    try:
        for level in LEVELS:
            rois = regions_at(name, level)
            offs = api.roi_multi_offsets(shape, level, rois)
            for p in sorted({1, enc["nlay"]}):
                ctx.decode_planes_rois(d_out, shape, level, rois, d_planes, info, p)
                flat = d_out.download(np.float64, int(offs[-1]))
                full = D(oracle, s, shape, level, p)
                for i, r in enumerate(rois):
                    assert same_bits(flat[offs[i]:offs[i + 1]].reshape(api.roi_shape(r)), crop(full, r)), (level, p, i)
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_planes_rois(d_out, shape, 0, [rois[0], ((0, 1), (0, 1), (0, 51))], d_planes, info)
        assert "error -1" in str(e.value) and "region 1:" in str(e.value), str(e.value)
    finally:
        d_planes.free()
        d_out.free()


# ---- 3. formats ----------------------------------------------------------------------------------------------------------
def test_formats(ctx, oracle):
    """WRS1, planes recut at different lengths, WRS2, WRS3 natural and blocked: the same regions, and the coder is launched
    once per call on WRS1 / WRS2 however many planes are used, once per plane on WRS3."""
    name, tol = "T", 1e-6
    shape = SETS[name][0]
    s = stream(ctx, shape, tol)
    f, wrs1 = s["f"], s["enc"]

    def coded(**kw):
        enc, _ = ctx.encode_host_seg(f, tol, 1, 4096, **kw)
        enc["data"] = enc["data"].copy()
        assert enc["nlay"] == wrs1["nlay"]
        return enc

    nlay = wrs1["nlay"]
    assert nlay >= 2
    streams = [("wrs1", wrs1, lambda p: 1), ("recut", recut(wrs1, s["planes"], (1008, 4096, api.SEG_DEFAULT)), lambda p: 1),
               ("wrs2", coded(brick=16), lambda p: 1), ("wrs3", coded(strands=8), lambda p: p), ("wrs3 blocked", coded(strands=8, brick=16), lambda p: p)]
    for what, enc, per_call in streams:
        for level in (0, 2, 4):
            rois = regions_at(name, level)
            for p in sorted({1, nlay}):
                l0 = launches()
                got = multi_all_ways(ctx, shape, level, rois, enc, p)
                assert launches() - l0 == 3 * per_call(p), (what, level, p, launches() - l0)
                check_against_oracle(got, oracle, s, shape, level, rois, p, what)
        # ... and the single-region calls of the same stream give the same bits and launch once per plane and region
        rois = regions_at(name, 0)
        l0 = launches()
        check_against_singles(ctx, shape, 0, rois, enc, nlay, what)
        assert launches() - l0 == 3 * per_call(nlay) + 2 * len(rois) * nlay, what


# ---- 4. only the union is read -------------------------------------------------------------------------------------------
def union_sets(enc, shape, level, rois):
    """Per plane: (the union's ids, segment lengths from the index)."""
    out = []
    for blob in split_planes(enc):
        seg, lens = index_of(blob)
        out.append((api.seg_roi_segments_multi(shape, level, rois, seg, wlev=enc["wlev"]).astype(np.int64), lens))
    return out


def masked(enc, sets):
    """A copy of the stream in which every byte of every segment outside the union is 0xFF; the indices stay."""
    data = enc["data"].copy()
    at = 0
    for (need, lens), ln in zip(sets, enc["len_enc_vec"]):
        start = at + 12 + 4 * lens.size + np.concatenate(([0], np.cumsum(lens)))
        keep = np.zeros(lens.size, dtype=bool)
        keep[need] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    return dict(enc, data=data)


@pytest.mark.parametrize("name,union,nseg", [("S", 1833, 2043), ("T", 133, 136)])
def test_only_the_union_is_read(ctx, oracle, name, union, nseg):
    shape = SETS[name][0]
    s = stream(ctx, shape, 1e-6)
    enc, rois = s["enc"], regions_at(name, 0)
    nlay = enc["nlay"]
    sets = union_sets(enc, shape, 0, rois)
    assert all((need.size, lens.size) == (union, nseg) for need, lens in sets) and union < nseg
    assert np.array_equal(sets[0][0], union_of(single_lists(shape, 0, rois, 4096)))
    bad = masked(enc, sets)
    assert not np.array_equal(bad["data"], enc["data"])
    low0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)
    s0, b0, l0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()
    got = multi_all_ways(ctx, shape, 0, rois, bad, 0)
    ds, db, dl = api.stat(api.STAT_ROI_SEGMENTS) - s0, api.stat(api.STAT_ROI_BYTES_UP) - b0, launches() - l0
    check_against_oracle(got, oracle, s, shape, 0, rois, nlay, name)
    # three calls: each launches the union of every plane once and uploads its streams, and nothing else
    assert ds == 3 * union * nlay, (name, ds)
    assert db == 3 * sum(int(lens[need].sum()) for need, lens in sets), (name, db)
    assert dl == 3, (name, dl)
    # fewer planes: fewer segments
    s0 = api.stat(api.STAT_ROI_SEGMENTS)
    one = ctx.decode_host_seg_rois(shape, 0, rois, bad, 1)
    assert api.stat(api.STAT_ROI_SEGMENTS) - s0 == union
    full = D(oracle, s, shape, 0, 1)
    assert all(same_bits(a, crop(full, r)) for a, r in zip(one, rois))
    assert (api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)) == low0


# ---- 5. one region ---------------------------------------------------------------------------------------------------------
def test_one_region_is_the_single_call_with_one_launch(ctx):
    shape = SETS["S"][0]
    enc = stream(ctx, shape, 1e-6)["enc"]
    nlay = enc["nlay"]
    assert nlay >= 2
    for level in (0, 3):
        roi = regions_at("S", level)[0]
        want = np.empty(api.roi_shape(roi))
        l0, s0 = launches(), api.stat(api.STAT_ROI_SEGMENTS)
        ctx.decode_host_seg_roi(want, shape, level, roi, enc)
        assert launches() - l0 == nlay  # the single call: one launch per plane
        per_call = api.stat(api.STAT_ROI_SEGMENTS) - s0
        l0, s0 = launches(), api.stat(api.STAT_ROI_SEGMENTS)
        tm = {}
        got = ctx.decode_host_seg_rois(shape, level, [roi], enc, timings=tm)
        assert launches() - l0 == 1 and api.stat(api.STAT_ROI_SEGMENTS) - s0 == per_call
        assert len(got) == 1 and same_bits(got[0], want), level
        assert tm["rangecoder"] > 0 and tm["plane_coder_s"][0] == tm["rangecoder"] and not any(tm["plane_coder_s"][1:])


# ---- 6. constant field -----------------------------------------------------------------------------------------------------
def test_constant_field(ctx):
    flat = np.full((8, 6, 10), 3.25)
    enc, _ = ctx.encode_host_seg(flat, 1e-6)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    for level, rois in ((0, [((2, 5), (0, 6), (9, 10)), ((0, 8), (0, 6), (0, 10)), ((2, 5), (0, 6), (9, 10))]), (2, [((0, 2), (1, 2), (0, 3)), ((1, 2), (0, 1), (2, 3))])):
        l0 = launches()
        h64, h32, d64 = multi_all_ways(ctx, flat.shape, level, rois, enc, 0)
        assert launches() == l0
        for i, r in enumerate(rois):
            assert h64[i].shape == api.roi_shape(r) and h32[i].dtype == np.float32
            assert np.all(h64[i] == 3.25) and np.all(d64[i] == 3.25) and np.all(h32[i] == np.float32(3.25)), (level, i)


# ---- 7. errors -------------------------------------------------------------------------------------------------------------
def test_corrupted_segments(ctx, oracle):
    """A flipped count-table byte inside a segment of the union: WR_ERR_STREAM naming the plane, and the context goes on
    working; the same byte in a segment outside the union changes nothing, while its index is still validated.  The corrupted
    streams are streams the host reference refuses too.  Run once."""
    name = "T"
    shape = SETS[name][0]
    s = stream(ctx, shape, 1e-6)
    enc, rois = s["enc"], regions_at(name, 0)
    nlay = enc["nlay"]
    full = D(oracle, s, shape, 0, nlay)
    need, lens = union_sets(enc, shape, 0, rois)[0]

    def flipped(k, plane_at=0):
        bad = dict(enc, data=enc["data"].copy())
        bad["data"][plane_at + 12 + 4 * lens.size + int(lens[:k].sum()) + 40] ^= 0x55  # inside the 256 counts at the head of segment k's stream
        return bad

    def right(got):
        return all(same_bits(a, crop(full, r)) for a, r in zip(got, rois))

    bad = flipped(int(need[len(need) // 2]))
    with pytest.raises(api.WaveRangeError):  # (the host reference refuses the segment too: its counts no longer add up)
        api.seg_decode_host_ref(split_planes(bad)[0], s["f"].size)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_rois(shape, 0, rois, bad)
    assert "error -4" in str(e.value) and "plane 0:" in str(e.value), str(e.value)
    assert right(ctx.decode_host_seg_rois(shape, 0, rois, enc))
    other = np.setdiff1d(np.arange(lens.size), need)
    assert other.size
    assert right(ctx.decode_host_seg_rois(shape, 0, rois, flipped(int(other[0]))))
    # the index of a segment outside the union, and of an unused plane, is validated before anything is launched
    last = sum(enc["len_enc_vec"][:nlay - 1])
    for at, plane_at in ((12 + 4 * int(other[0]), 0), (12 + 4 * int(other[0]), last), (0, last)):
        bad = dict(enc, data=enc["data"].copy())
        bad["data"][plane_at + at] ^= 1
        s0, l0 = api.stat(api.STAT_ROI_SEGMENTS), launches()
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_host_seg_rois(shape, 0, rois, bad, 1)
        assert "error -4" in str(e.value) and "plane %d:" % (0 if plane_at == 0 else nlay - 1) in str(e.value), str(e.value)
        assert (api.stat(api.STAT_ROI_SEGMENTS), launches()) == (s0, l0)


def test_refusals(ctx):
    shape = (64, 64, 64)
    enc = stream(ctx, shape, 1e-3)["enc"]
    rois = regions_at("W", 0)
    # one bad box among good ones: WR_ERR_ARG naming it, and nothing is launched
    for bad_box in (((0, 1), (0, 1), (0, 65)), ((3, 3), (0, 1), (0, 1))):
        s0, b0, l0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()
        with pytest.raises(api.WaveRangeError) as e:
            ctx.decode_host_seg_rois(shape, 0, [rois[0], rois[1], bad_box, rois[2]], enc)
        assert "error -1" in str(e.value) and "region 2:" in str(e.value), str(e.value)
        assert (api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()) == (s0, b0, l0)
    info = api.EncInfo.from_dict(enc)
    data = enc["data"]
    # the same at the C entry points, whose output buffer is large enough for the good regions
    mixed, room = api._boxes([rois[0], rois[1], ((0, 1), (0, 1), (0, 65)), rois[2]]), np.empty(2 * 64 ** 3)
    s0, b0, l0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()
    for fn in (api.lib().wr_decode_host_seg_roi_multi, api.lib().wr_decode_host_seg_roi_multi_f32):
        assert fn(ctx.h, room.ctypes.data, 64, 64, 64, 0, 0, mixed, 4, api.C.byref(info), data.ctypes.data, data.size, None) == -1
        assert api.lib().wr_last_error().decode().startswith("region 2: "), api.lib().wr_last_error().decode()
    assert (api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), launches()) == (s0, b0, l0)
    big = np.empty((api.ROI_MULTI_MAX + 1) * 64)
    boxes = api._boxes([((0, 4), (0, 4), (0, 4))] * (api.ROI_MULTI_MAX + 1))
    L = api.lib()
    d_out = ctx.alloc(big.nbytes)
    try:
        for fn, ptr in ((L.wr_decode_host_seg_roi_multi, big.ctypes.data), (L.wr_decode_host_seg_roi_multi_f32, big.ctypes.data),
                        (L.wr_decode_device_seg_roi_multi, d_out.ptr)):
            def call(level, p, arr, nroi, out=ptr):
                return fn(ctx.h, out, 64, 64, 64, level, p, arr, nroi, api.C.byref(info), data.ctypes.data, data.size, None)
            assert call(0, 0, boxes, 2) == 0 and call(0, 0, boxes, api.ROI_MULTI_MAX) == 0
            for level, p, arr, nroi in ((0, 0, boxes, 0), (0, 0, boxes, api.ROI_MULTI_MAX + 1), (0, 0, boxes, -1), (0, 0, None, 2), (5, 0, boxes, 2),
                                        (0, enc["nlay"] + 1, boxes, 2)):
                assert call(level, p, arr, nroi) == -1, (level, p, nroi)
            assert call(0, 0, boxes, 2, out=None) == -1
    finally:
        d_out.free()
    with pytest.raises(api.WaveRangeError):
        ctx.decode_host_seg_rois(shape, 0, [], enc)
    got = ctx.decode_host_seg_rois(shape, 4, [((0, 4),) * 3], enc)  # and the context goes on working
    want = np.empty((4, 4, 4))
    ctx.decode_host_seg_roi(want, shape, 4, ((0, 4),) * 3, enc)
    assert same_bits(got[0], want)
