"""The batch calls for WRS3, on the CPU: the case table of tests/strand_batch_cases.py is what it claims to be, the two lane
layouts the batched strand kernels use (wr_seg_batch_strand_lane for the encoder, wr_seg_lists_lanes for the decoder) against
plain Python, the device-memory formula, every case's host-reference blob through the plain-Python coder, and the layouts
of csrc/wr_segbatch.h under ASan + UBSan in a stand-alone program."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import coder_cases as cc
import strand_batch_cases as sb
from py_coder import py_decode_model, py_decode_strand
from waverange_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "waverange_amd", "csrc")


def test_the_table_reaches_every_class():
    assert sb.reached() >= sb.REQUIRED, sb.REQUIRED - sb.reached()
    assert all(sb.classes(c) for c in sb.STAGE)
    # what the comments of the table say of its cases
    assert sb.classes(sb.STAGE[0]) >= {"one_segment_per_job", "empty_strands", "partial_last_wave", "many_jobs"}
    assert sb.classes(sb.STAGE[1]) >= {"wave_spans_jobs", "empty_strands", "K32"}
    assert sb.classes(sb.STAGE[2]) >= {"K1", "scan_past_1024"}
    assert sb.classes(sb.STAGE[3]) >= {"short_last_strand", "empty_strands", "decoder_padding"} and 367 * 2 == 734
    assert sb.classes(sb.STAGE[4]) >= {"short_last_strand", "one_symbol_segment", "decoder_exact"}
    assert sb.classes(sb.STAGE[5]) >= {"default_seg", "partial_last_wave"} and 13 * sb.nseg_of(262144, 59904) == 65
    assert sb.classes(sb.STAGE[6]) >= {"batch_of_one"}
    for case in sb.STAGE:
        n, seg, K, jobs = case
        assert cc.seg_ok(seg) and cc.strands_ok(K, seg) and 1 <= jobs <= api.SEG_BATCH_MAX
        ps = sb.planes(case)
        assert len(ps) == jobs and all(p.size == n and p.dtype == np.uint8 for p in ps)
        assert len({p.tobytes() for p in ps}) == jobs, sb.case_id(case)  # every job of a launch is another plane
    jobs = sb.mixed_jobs()
    assert len(jobs) == sb.MIXED_JOBS and {(seg, K) for _, seg, K in jobs} == set(sb.MIXED_FORMATS)
    assert sum(1 for _, _, K in jobs if K == 0) >= 2 and sum(1 for _, _, K in jobs if K) >= 2


@pytest.mark.parametrize("case", sb.STAGE, ids=sb.case_id)
def test_encoder_layout(case):
    """every (job, segment, strand) is owned by exactly one lane of the grid, and lanes past the end are dead"""
    n, seg, K, jobs = case
    nseg = sb.nseg_of(n, seg)
    want, grid = sb.encoder_layout([nseg] * jobs, K)
    first = np.arange(jobs + 1, dtype=np.uint32) * nseg
    assert grid % 64 == 0 and grid - 64 < jobs * nseg * K <= grid
    # all lanes where the table is small; otherwise the lanes around every job's boundary, the first and the last waves
    lanes = set(range(grid + 64)) if grid <= 4096 else set()
    for j in range(jobs + 1):
        lanes |= set(range(max(0, j * nseg * K - 70), min(grid + 64, j * nseg * K + 70)))
    owners = {}
    for g in sorted(lanes):
        got = api.seg_batch_strand_lane(first, K, g)
        assert got == want.get(g), (g, got, want.get(g))
        if got is not None:
            assert got not in owners, (g, got)
            owners[got] = g
    if grid <= 4096:
        assert len(owners) == jobs * nseg * K
        assert set(owners) == {(j, k, s) for j in range(jobs) for k in range(nseg) for s in range(K)}


def test_encoder_layout_of_uneven_jobs_and_refusals():
    nsegs = [3, 0, 1, 17, 0, 5]
    first = np.concatenate(([0], np.cumsum(nsegs))).astype(np.uint32)
    for K in (1, 2, 4, 8, 16, 32):
        want, grid = sb.encoder_layout(nsegs, K)
        seen = set()
        for g in range(grid + 64):
            got = api.seg_batch_strand_lane(first, K, g)
            assert got == want.get(g), (K, g)
            if got is not None:
                # the K lanes of a segment sit aligned inside one wave
                assert (g - got[2]) % K == 0 and (g - got[2]) // 64 == (g - got[2] + K - 1) // 64
                seen.add(got)
        assert len(seen) == sum(nsegs) * K
    for bad_k in (0, 3, 64):
        with pytest.raises(api.WaveRangeError):
            api.seg_batch_strand_lane(first, bad_k, 0)
    with pytest.raises(api.WaveRangeError):
        api.seg_batch_strand_lane([0, 2, 1], 8, 0)
    with pytest.raises(api.WaveRangeError):
        api.seg_batch_strand_lane([1, 2], 8, 0)
    assert api.seg_batch_strand_lane([0, 0], 8, 0) is None  # a launch without segments: every lane is past the end


@pytest.mark.parametrize("case", sb.STAGE, ids=sb.case_id)
def test_decoder_layout(case):
    n, seg, K, jobs = case
    nseg = sb.nseg_of(n, seg)
    first, want = sb.decoder_layout([nseg] * jobs, [K] * jobs)
    lanes, got_first = api.seg_lists_lanes([nseg] * jobs, [K] * jobs)
    assert lanes == first[-1] and lanes % 64 == 0 and list(got_first) == first
    per_job = first[1]
    assert ("decoder_padding" in sb.classes(case)) == (per_job != nseg * K)
    # the locator on the lanes around every job's boundary (all lanes where the launch is small)
    probe = set(range(lanes)) if lanes <= 4096 else set()
    for f in first[:-1]:
        probe |= set(range(max(0, f - 70), min(lanes, f + 70)))
    for g in sorted(probe):
        j, r = api.seg_batch_locate(got_first, g)
        k, s = r // K, r % K
        assert (want.get(g) == (j, k, s)) if k < nseg else (g not in want), (g, j, r)


def test_decoder_layout_of_the_mixed_list():
    """the stranded jobs of the mixed list, each with its own K and segment length, in one launch"""
    jobs = [(p.size, seg, K) for p, seg, K in sb.mixed_jobs() if K]
    nsegs, Ks = [sb.nseg_of(n, seg) for n, seg, _ in jobs], [K for _, _, K in jobs]
    first, want = sb.decoder_layout(nsegs, Ks)
    lanes, got_first = api.seg_lists_lanes(nsegs, Ks)
    assert lanes == first[-1] and list(got_first) == first
    for g in range(0, lanes, 61):
        j, r = api.seg_batch_locate(got_first, g)
        assert want.get(g, (j, None, None))[0] == j and (r // Ks[j] < nsegs[j]) == (g in want)


def test_device_bytes():
    f = api.seg_batch_device_bytes_strands
    for n, seg, K, _ in sb.STAGE:
        nseg, L = sb.nseg_of(n, seg), cc.strand_len(seg, K)
        bound = api.seg_bound_strands(n, seg, K)
        assert bound == 20 + nseg * (4 + 4 * (K + 1) + 520 + K * (2 * L + 8))
        for N, nlay in ((1, 1), (7, 3), (64, 8)):
            # encode: a plane and a blob at its bound per job, the staging of one plane index at the strand stride
            pieces = N * nlay * (n + bound) + N * nseg * (520 + K * (2 * L + 8)) + N * (8 * (nseg + 1) + 4 * nseg * (2 + K))
            assert f(N, n, nlay, seg, 0, K) >= pieces, (n, seg, K, N, nlay)
            # decode: a plane, a blob, the offsets and flags per job, a failure count per job
            pieces = N * nlay * (n + bound + 8 * (nseg + 1) + 4 * nseg + 4)
            assert f(N, n, nlay, seg, 0, K, True) >= pieces, (n, seg, K, N, nlay)
            for decode in (False, True):
                here = f(N, n, nlay, seg, 0, K, decode)
                assert here > 0
                assert f(N + 1, n, nlay, seg, 0, K, decode) >= here
                assert f(N, n + 1, nlay, seg, 0, K, decode) >= here and f(N, n + seg, nlay, seg, 0, K, decode) >= here
                assert f(N, n, min(nlay + 1, api.NLAYMAX), seg, 0, K, decode) >= here
                assert f(N, n, nlay, seg, 8, K, decode) >= here + (N if not decode else N * nlay) * n  # the stream-order planes
    # about 2.0 n of staging per plane where WRS1 takes 1.07 n
    n = 128 ** 3
    wrs3 = f(8, n, 1, 0, 0, 8) - 8 * (n + api.seg_bound_strands(n, 0, 8))
    wrs1 = api.seg_batch_device_bytes(8, n, 1) - 8 * (n + api.seg_bound(n, 0))
    assert 1.9 < wrs3 / (8 * n) < 2.2 and 1.0 < wrs1 / (8 * n) < 1.15, (wrs3 / (8 * n), wrs1 / (8 * n))
    # strands = 0 is the default; refusals
    assert f(8, n, 3, 0, 0, 0) == f(8, n, 3, 0, 0, 8)
    for K in (3, 64):
        assert f(8, n, 3, 0, 0, K) == 0 and f(8, n, 3, 0, 0, K, True) == 0
    assert f(8, n, 3, 48, 0, 4) == 0 and f(8, n, 3, 496, 0, 32) == 0 and f(8, n, 3, 512, 0, 32) > 0  # 16 K > seg
    assert f(0, n, 3) == 0 and f(api.SEG_BATCH_MAX + 1, n, 3) == 0 and f(8, 0, 3) == 0 and f(8, n, api.NLAYMAX + 1) == 0
    assert f(8, n, 3, 24) == 0 and f(8, n, 3, 0, 7) == 0
    assert f(8, n, 0) >= 0 and f(api.SEG_BATCH_MAX, n, 1) > 0


def py_decode_record(T, strands, bs, L):
    count = py_decode_model(T)
    assert sum(count) == bs
    out = [py_decode_strand(S, count, min(L, bs - j * L)) for j, S in enumerate(strands) if j * L < bs]
    assert all(S == b"" for j, S in enumerate(strands) if j * L >= bs)
    return np.concatenate(out)


PY_SYMBOLS = 20000  # a plane up to this size goes through the plain-Python decoder whole (it takes microseconds per symbol)


@pytest.mark.parametrize("case", sb.STAGE, ids=sb.case_id)
def test_host_blobs_decode_with_the_plain_python_coder(case):
    """Every case's blob by the host reference -- the GPU tests' yardstick -- decodes to its plane with the plain-Python coder: the
    whole plane of the different base planes where that is quick, the first and the last record of two planes otherwise, with
    the host reference's own decoder on the whole blob of every plane beside it."""
    n, seg, K, jobs = case
    L, nseg = cc.strand_len(seg, K), sb.nseg_of(n, seg)
    nbase = len(sb.base_planes(n, seg, K))
    for j, p in enumerate(sb.planes(case)):
        blob = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
        assert blob.size <= api.seg_bound_strands(n, seg, K)
        assert np.array_equal(api.seg_decode_host_ref_blocked(blob, (1, 1, n), 0), p), (sb.case_id(case), j)
        got_seg, brick, got_K, recs = api.seg_split_strands(blob)
        assert (got_seg, brick, got_K, len(recs)) == (seg, 0, K, nseg)
        whole = n <= PY_SYMBOLS and j < nbase and (nseg <= 64 or j == 0)
        for k in (range(nseg) if whole else sorted({0, nseg - 1}) if j < 2 else ()):
            bs = min(seg, n - k * seg)
            assert np.array_equal(py_decode_record(recs[k][0], recs[k][1], bs, L), p[k * seg:k * seg + bs]), (sb.case_id(case), j, k)


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]  # tests/test_seg_cpu.py


def _have_san():
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write("int main(){return 0;}\n")
        return subprocess.run(["g++"] + SAN + [src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_san(), reason="g++ with ASan/UBSan not available")
def test_lane_layouts_under_sanitizers():
    """The two lane layouts of csrc/wr_segbatch.h -- what the kernels run -- compiled by g++ under ASan + UBSan and swept over
    random job tables up to 1024 jobs (tests/native/strandbatch_fuzz.cpp: a stand-alone program)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "strandbatch_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, os.path.join(ROOT, "tests", "native", "strandbatch_fuzz.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "strand batch lane layout sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
