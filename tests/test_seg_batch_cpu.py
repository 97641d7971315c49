"""Batched segmented streams without a GPU: the locator that gives every lane of a batched coder launch its (job, segment),
the device-memory formula of a batch, and the locator's header under ASan + UBSan."""
import bisect
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from util import ROOT
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")

PREFIX_CASES = {
    "70 jobs of 1": [1] * 70,
    "9 jobs of 17": [17] * 9,
    "3 jobs of 1100": [1100] * 3,
    "13 jobs of 5": [5] * 13,
    "zero-segment jobs in the middle and at both ends": [0, 0, 3, 0, 1, 0, 0, 64, 65, 0, 2, 0, 0],
}


def prefix_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def py_locate(first, g):
    """The plain-Python search: the last job whose first lane is not behind g (jobs without segments never qualify)."""
    j = bisect.bisect_right([int(v) for v in first], g) - 1
    return j, g - int(first[j])


@pytest.mark.parametrize("name", list(PREFIX_CASES))
def test_locate_every_lane(name):
    counts = PREFIX_CASES[name]
    first = prefix_of(counts)
    seen = [0] * len(counts)
    for g in range(int(first[-1])):
        job, k = api.seg_batch_locate(first, g)
        assert (job, k) == py_locate(first, g), (name, g)
        assert 0 <= k < counts[job], (name, g)
        seen[job] += 1
    assert seen == counts, name  # every segment of every job has exactly one lane


def test_locate_refusals():
    first = prefix_of([3, 0, 2])
    for g in (5, 6, 2 ** 32 - 1):  # past the end of the launch
        with pytest.raises(api.WaveRangeError) as e:
            api.seg_batch_locate(first, g)
        assert "error -1" in str(e.value)
    for bad in ([1, 2, 3], [0, 5, 4], [0]):  # does not start at 0, decreases, no job at all
        with pytest.raises(api.WaveRangeError):
            api.seg_batch_locate(np.array(bad, dtype=np.uint32), 0)
    with pytest.raises(api.WaveRangeError):  # more jobs than a launch has
        api.seg_batch_locate(prefix_of([1] * (api.SEG_BATCH_MAX + 1)), 0)
    assert api.seg_batch_locate(prefix_of([1] * api.SEG_BATCH_MAX), api.SEG_BATCH_MAX - 1) == (api.SEG_BATCH_MAX - 1, 0)


def up(v, a):
    return (v + a - 1) // a * a


def single_call_bytes(n, nlay, seg, brick):
    """What encode_seg_impl takes from the plane pool beside the planes, by its own formulas: wrk::seg_stage_bytes (restated
    here from wr_segcoder.hip), a blob buffer of the 16-byte-rounded bound per plane, and the permuted plane of a WRS2 call."""
    nseg = -(-n // seg)
    stream_bound = api.seg_bound(1, seg) - 16  # wr_seg_bound = 12 + nseg * (4 + stream_bound(seg))
    stage = 256 + up(8 * (nseg + 1) + 4 * nseg, 256) + nseg * up(stream_bound, 4)
    bound = api.seg_bound_blocked(n, seg) if brick else api.seg_bound(n, seg)
    return stage + nlay * up(bound, 16) + (n if brick else 0)


def test_device_bytes():
    """Monotone where the sum can be: in nfields, n, nlay, in brick (a WRS2 batch holds one more plane per field) and in `seg`
    over lengths that divide n.  Over all seg it is a sawtooth -- the staging is ceil(n / seg) regions of the segment bound
    seg + seg / 32 + 2064, so a longer segment that leaves the count where it was makes every region longer, and one that
    lowers the count drops a region -- and the function has to be the drivers' arithmetic, not a smoothed bound."""
    B = api.seg_batch_device_bytes
    for decode in (False, True):
        for brick in (0, 32):
            for seg in (16, 4096, 59904):
                base = dict(n=48 * 40 * 36, nlay=3, seg=seg, brick=brick, decode=decode)
                prev = 0
                for nfields in (1, 2, 3, 8, 64, 1024):
                    got = B(nfields, **base)
                    assert got > prev, (nfields, base)
                    prev = got
                prev = 0
                for n in (1, 15, 16, 17, 4096, 4097, 59904, 59905, 128 ** 3, 128 ** 3 + 1, 256 ** 3):
                    got = B(8, n, 3, seg, brick, decode)
                    assert got >= prev and got > 0, (n, base)
                    prev = got
                prev = -1
                for nlay in range(api.NLAYMAX + 1):
                    got = B(8, 48 * 40 * 36, nlay, seg, brick, decode)
                    assert got > prev, (nlay, base)
                    prev = got
            assert B(8, 69120, 3, 4096, 32, decode) > B(8, 69120, 3, 4096, 0, decode)
        n = 16 * 59904
        sizes = [B(8, n, 3, seg, 0, decode) for seg in (16, 64, 128, 576, 7488, 59904)]  # all divide n
        assert all(a > b for a, b in zip(sizes, sizes[1:])), sizes  # the fewer segments, the less index and staging per symbol
    assert B(1, 1000, 3) == B(1, 1000, 3, api.SEG_DEFAULT)  # seg = 0 is the default length
    # refused arguments
    for seg in (8, 24, 59999, 60000):
        assert B(4, 1000, 3, seg) == 0, seg
    for brick in (1, 7, 12, 128):
        assert B(4, 1000, 3, 4096, brick) == 0, brick
    for nfields in (0, -1, api.SEG_BATCH_MAX + 1):
        assert B(nfields, 1000, 3, 4096) == 0, nfields
    assert B(api.SEG_BATCH_MAX, 1000, 3, 4096) > 0
    assert B(4, 0, 3, 4096) == 0 and B(4, 1000, -1, 4096) == 0 and B(4, 1000, api.NLAYMAX + 1, 4096) == 0
    # one field: at least what the single call allocates today, and the planes on top (the single call has them in the
    # context's plane streams, a batch owns them)
    for n in (1, 2048, 69120, 64 ** 3, 128 ** 3):
        for seg in (16, 4096, 59904):
            for brick in (0, 8, 32):
                for nlay in (0, 1, 5, 8):
                    got, single = B(1, n, nlay, seg, brick), single_call_bytes(n, nlay, seg, brick)
                    if nlay:
                        assert got >= single + nlay * n, (n, seg, brick, nlay, got, single)


SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]  # tests/test_seg_cpu.py


def _have_san():
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write("int main(){return 0;}\n")
        return subprocess.run(["g++"] + SAN + [src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_san(), reason="g++ with ASan/UBSan not available")
def test_locator_under_sanitizers():
    """csrc/wr_segbatch.h -- what the kernels include -- compiled by g++ under ASan + UBSan: the prefixes above and random
    ones, every lane, on exact-size arrays (tests/native/segbatch_fuzz.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "segbatch_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, os.path.join(ROOT, "tests", "native", "segbatch_fuzz.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "segment batch locator sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
