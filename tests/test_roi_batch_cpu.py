"""Region decode across a batch of fields without a GPU: the lane layout of a coder launch over lists with stranded jobs
(wr_seg_lists_lanes, csrc/wr_segbatch.h), the device-memory bound, the helper that cuts a series into calls, and the layout's
header under ASan + UBSan."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from util import ROOT
from test_seg_batch_cpu import SAN, _have_san
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
KS = [0, 1, 2, 4, 8, 16, 32]
LISTS = [0, 1, 63, 64, 65]


def py_layout(nlist, strands):
    """The definition, restated: a plain job owns one lane per listed segment, a stranded one nlist * K rounded up to 64."""
    first = [0]
    for n, k in zip(nlist, strands):
        first.append(first[-1] + (-(-n * k // 64) * 64 if k else n))
    return first


def check_layout(nlist, strands):
    lanes, first = api.seg_lists_lanes(nlist, strands)
    want = py_layout(nlist, strands)
    assert [int(v) for v in first] == want and lanes == want[-1], (nlist, strands)
    assert all(b >= a for a, b in zip(want, want[1:]))
    for j, (n, k) in enumerate(zip(nlist, strands)):
        span = want[j + 1] - want[j]
        if k:
            assert span % 64 == 0 and span >= n * k, (j, n, k)
    return want


def check_lanes(nlist, strands, first, every=1):
    """every lane (or every `every`-th) through wr_seg_batch_locate: live lanes land on the (job, position, strand) of the
    definition, padding lanes on a position >= nlist"""
    live = {}
    for g in range(0, first[-1], every):
        job, r = api.seg_batch_locate(np.asarray(first, dtype=np.uint32), g)
        n, k = nlist[job], strands[job]
        assert first[job] <= g < first[job + 1]
        pos, strand = (r // k, r % k) if k else (r, 0)
        if pos < n:
            assert g == first[job] + pos * max(k, 1) + strand
            live[job] = live.get(job, 0) + 1
        else:
            assert k and pos >= n  # only a stranded job has padding
    if every == 1:
        assert all(live.get(j, 0) == n * max(k, 1) for j, (n, k) in enumerate(zip(nlist, strands)))


def test_lanes_one_and_two_jobs():
    for k in KS:
        for n in LISTS:
            if n:
                check_lanes([n], [k], check_layout([n], [k]))
            else:
                assert api.seg_lists_lanes([0], [k])[0] == 0
    for (a, b), (n, m) in itertools.product(itertools.product(KS, KS), itertools.product(LISTS, LISTS)):
        if n + m:
            first = check_layout([n, m], [a, b])
            if (a, b) in ((0, 4), (8, 0), (32, 1), (2, 16)):
                check_lanes([n, m], [a, b], first)


def test_lanes_1024_jobs():
    nlist = [LISTS[j % 5] for j in range(api.SEG_BATCH_MAX)]
    strands = [KS[(j // 5) % 7] for j in range(api.SEG_BATCH_MAX)]
    first = check_layout(nlist, strands)
    check_lanes(nlist, strands, first, every=37)
    # strands None: every job is a plain one
    lanes, first = api.seg_lists_lanes(nlist)
    assert lanes == sum(nlist) and int(first[-1]) == lanes


def test_lanes_refusals():
    for nlist, strands in (([1] * (api.SEG_BATCH_MAX + 1), None), ([], None), ([1, 1], [0, 3]), ([1], [64]), ([1], [5]),
                           ([2 ** 30, 2 ** 30], [0, 0]), ([2 ** 26], [32]), ([2 ** 31], None)):
        with pytest.raises(api.WaveRangeError) as e:
            api.seg_lists_lanes(nlist, strands)
        assert "error -1" in str(e.value), str(e.value)
    assert api.seg_lists_lanes([2 ** 26], [16])[0] == 2 ** 30
    assert api.seg_lists_lanes([2 ** 31 - 1])[0] == 2 ** 31 - 1
    assert api.lib().wr_seg_lists_lanes(1, None, None, None) == 0


def up(v, a):
    return (v + a - 1) // a * a


def test_roi_batch_device_bytes():
    B = api.seg_roi_batch_device_bytes
    pitch = api.lib().wr_plane_pitch
    for brick, strands in ((0, 0), (32, 0), (0, 8), (16, 4)):
        for seg in (1008, 4096, api.SEG_DEFAULT):
            kw = dict(seg=seg, brick=brick, strands=strands)
            prev = 0
            for nfields in (1, 2, 3, 8, 64, 256):
                got = B(nfields, 69120, 4, out_elems=1000, **kw)
                assert got > prev, (nfields, kw)
                prev = got
            prev = 0
            for n in (1, 15, 16, 17, 4096, 4097, 59904, 59905, 128 ** 3, 128 ** 3 + 1, 256 ** 3):
                got = B(8, n, 3, **kw)
                assert got >= prev and got > 0, (n, kw)
                prev = got
            prev = -1
            for planes in range(api.NLAYMAX + 1):
                got = B(8, 69120, planes, **kw)
                assert got > prev, (planes, kw)
                prev = got
            # at least the pieces of the formula: per job the plane at full pitch, the blob at its bound and the offsets of its
            # segments; per WRS2 job a second plane; for a host caller the output
            for nfields, n, planes, out in ((1, 69120, 1, 0), (8, 69120, 4, 32 ** 3), (16, 128 ** 3, 8, 12345)):
                bound = api.seg_bound_strands(n, seg, strands) if strands else api.seg_bound_blocked(n, seg) if brick else api.seg_bound(n, seg)
                nseg = -(-n // seg)
                per_job = pitch(n) + bound + 8 * (nseg + 1) + 4 * nseg + 4 * nseg + (pitch(n) if brick else 0)
                assert B(nfields, n, planes, seg, brick, strands, out) >= nfields * planes * per_job + 8 * nfields * out
            assert B(8, 69120, 4, seg, brick, strands, 1000) - B(8, 69120, 4, seg, brick, strands, 0) >= 8 * 8 * 1000
    assert B(1, 1000, 3) == B(1, 1000, 3, api.SEG_DEFAULT)
    assert B(8, 69120, 3, 4096, 32) > B(8, 69120, 3, 4096, 0)
    # refused arguments
    for seg in (8, 24, 59999, 60000):
        assert B(4, 1000, 3, seg) == 0, seg
    for brick in (1, 7, 12, 128):
        assert B(4, 1000, 3, 4096, brick) == 0, brick
    for strands in (3, 64, 512):
        assert B(4, 1000, 3, 4096, 0, strands) == 0, strands
    assert B(4, 1000, 3, 16, 0, 2) == 0  # 16 * strands exceeds seg
    assert B(0, 1000, 3) == 0 and B(-1, 1000, 3) == 0 and B(4, 0, 3) == 0 and B(4, 1000, -1) == 0 and B(4, 1000, api.NLAYMAX + 1) == 0
    # the jobs of a call: fields times planes
    assert B(api.SEG_BATCH_MAX, 1000, 1) > 0 and B(api.SEG_BATCH_MAX + 1, 1000, 1) == 0
    assert B(128, 1000, 8) > 0 and B(129, 1000, 8) == 0
    assert B(5000, 1000, 0) > 0  # constant fields have no job


def test_roi_batch_groups():
    n, out = 64 ** 3, 32 ** 3
    one = api.seg_roi_batch_device_bytes(1, n, 4, out_elems=out)
    for nfields, planes, budget in ((1, 4, 10 * one), (64, 4, 10 * one), (64, 4, one), (64, 4, 3 * one + 5), (300, 8, 1 << 62), (7, [1, 8, 2, 2, 8, 1, 1], 4 * one)):
        groups, alone = api.roi_batch_groups(nfields, n, planes, budget, out_elems=out)
        assert alone == []
        assert [f for g in groups for f in g] == list(range(nfields))  # consecutive, in order, all of them
        pl = [planes] * nfields if isinstance(planes, int) else planes
        for g in groups:
            assert len(g) >= 1
            most = max(pl[f] for f in g)
            size = api.seg_roi_batch_device_bytes(len(g), n, most, out_elems=out)
            assert 0 < size <= budget, (nfields, g, size, budget)
            assert len(g) * most <= api.SEG_BATCH_MAX
        # greedy: a group could not have taken the next field too
        for g, h in zip(groups, groups[1:]):
            most = max(pl[f] for f in list(g) + [h[0]])
            size = api.seg_roi_batch_device_bytes(len(g) + 1, n, most, out_elems=out)
            assert size == 0 or size > budget
    groups, _ = api.roi_batch_groups(300, n, 8, 1 << 62, out_elems=out)
    assert [len(g) for g in groups] == [128, 128, 44]
    # a field that exceeds the budget alone is reported once, as a group of its own, and the cut goes on behind it
    groups, alone = api.roi_batch_groups(5, n, [1, 1, 8, 1, 1], api.seg_roi_batch_device_bytes(2, n, 1, out_elems=out), out_elems=out)
    assert alone == [2] and [list(g) for g in groups] == [[0, 1], [2], [3, 4]]
    groups, alone = api.roi_batch_groups(3, n, 4, 1, out_elems=out)
    assert alone == [0, 1, 2] and [list(g) for g in groups] == [[0], [1], [2]]
    assert api.roi_batch_groups(0, n, 4, one) == ([], [])


@pytest.mark.skipif(not _have_san(), reason="g++ with ASan/UBSan not available")
def test_lane_layout_under_sanitizers():
    """csrc/wr_segbatch.h -- what the kernels include -- compiled by g++ under ASan + UBSan: layouts of plain and stranded jobs,
    every lane, on exact-size arrays (tests/native/seglanes_fuzz.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "seglanes_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, os.path.join(ROOT, "tests", "native", "seglanes_fuzz.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "segment list lane layout sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
