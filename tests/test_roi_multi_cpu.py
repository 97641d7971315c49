"""Host geometry of the multi-region decode (include/waverange_amd.h, "Region decode, many regions per call"): the union of
the regions' segment lists and the offsets of the regions in the output.  No GPU."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from util import ROOT
from roi_multi_cases import SETS, regions_at, single_lists, union_of
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
SEGS = [1008, 4096, 59904]
ORDERS = [None, 16, 32]  # natural, blocked at brick 16 and 32
LEVELS = range(5)


def random_rois(rng, shape, level, count):
    box = api.lowres_shape(shape, level)
    out = []
    for _ in range(count):
        r = []
        for n in box:
            lo = int(rng.integers(0, n))
            r.append((lo, int(rng.integers(lo + 1, min(n, lo + 9) + 1))))
        out.append(tuple(r))
    return out


@pytest.mark.parametrize("brick", ORDERS)
@pytest.mark.parametrize("seg", SEGS)
def test_union_is_the_union_of_the_single_lists(seg, brick):
    for name in SETS:
        shape = SETS[name][0]
        for level in LEVELS:
            rois = regions_at(name, level)
            got = api.seg_roi_segments_multi(shape, level, rois, seg, brick=brick)
            want = union_of(single_lists(shape, level, rois, seg, brick=brick))
            assert got.dtype == np.uint32 and np.array_equal(got, want), (name, level, seg, brick)


def test_random_sweep():
    rng = np.random.default_rng(20261018)
    for _ in range(40):
        shape = tuple(int(v) for v in rng.integers(1, 70, size=3))
        wlev = int(rng.choice([0, 4]))
        level = int(rng.integers(0, wlev + 1))
        rois = random_rois(rng, shape, level, int(rng.integers(1, 7)))
        seg = int(rng.choice([16, 1008, 4096]))
        brick = [None, 8, 16][int(rng.integers(0, 3))]
        got = api.seg_roi_segments_multi(shape, level, rois, seg, wlev, brick)
        want = union_of(single_lists(shape, level, rois, seg, wlev, brick))
        assert np.array_equal(got, want), (shape, wlev, level, rois, seg, brick)
        offs = api.roi_multi_offsets(shape, level, rois)
        assert np.array_equal(offs, np.concatenate(([0], np.cumsum([np.prod(api.roi_shape(r)) for r in rois])))), (shape, level, rois)


def test_offsets():
    for name in SETS:
        shape = SETS[name][0]
        for level in LEVELS:
            rois = regions_at(name, level)
            offs = api.roi_multi_offsets(shape, level, rois)
            sizes = [int(np.prod(api.roi_shape(r))) for r in rois]
            assert offs.dtype == np.int64 and offs.size == len(rois) + 1
            assert np.array_equal(offs, np.concatenate(([0], np.cumsum(sizes)))), (name, level)
    # offs may be NULL: the total alone
    shape, rois = SETS["T"]
    arr = api._boxes(rois)
    assert api.lib().wr_roi_multi_elems(shape[2], shape[1], shape[0], 0, arr, len(rois), None) == int(api.roi_multi_offsets(shape, 0, rois)[-1])


def test_known_counts():
    """Computed from csrc/wr_roi.h alone: set S on (203,203,203) cut at 4096 has 2043 segments; the regions overlap and repeat,
    so the union is far smaller than the lists together."""
    shape = SETS["S"][0]
    assert -(-203 ** 3 // 4096) == 2043
    for level, union, together in zip(LEVELS, (1833, 534, 151, 41, 3), (5603, 1521, 383, 81, 5)):
        rois = regions_at("S", level)
        assert api.seg_roi_segments_multi(shape, level, rois, 4096).size == union, level
        assert sum(l.size for l in single_lists(shape, level, rois, 4096)) == together, level
    shape = SETS["T"][0]
    assert -(-301 * 37 * 50 // 4096) == 136
    assert api.seg_roi_segments_multi(shape, 0, regions_at("T", 0), 4096).size == 133


def test_cap_smaller_than_the_count():
    shape, rois = SETS["T"]
    full = api.seg_roi_segments_multi(shape, 0, rois, 4096)
    ids = np.full(10, 0xFFFFFFFF, dtype=np.uint32)
    got = api.lib().wr_seg_roi_segments_multi(shape[2], shape[1], shape[0], 0, 4, api._boxes(rois), len(rois), 0, 4096, ids.ctypes.data, 7)
    assert got == full.size
    assert np.array_equal(ids[:7], full[:7]) and np.all(ids[7:] == 0xFFFFFFFF)


def test_refusals():
    shape, rois = SETS["T"]
    nz, ny, nx = shape
    L = api.lib()
    good = api._boxes(rois)
    offs = (api.C.c_size_t * (api.ROI_MULTI_MAX + 2))()
    ids = np.zeros(4096, dtype=np.uint32)

    def seg_call(arr, nroi, seg=4096, brick=0, level=0, wlev=4):
        return L.wr_seg_roi_segments_multi(nx, ny, nz, level, wlev, arr, nroi, brick, seg, ids.ctypes.data, ids.size)

    assert seg_call(good, len(rois)) == 133 and L.wr_roi_multi_elems(nx, ny, nz, 0, good, len(rois), offs) > 0
    many = api._boxes([rois[0]] * (api.ROI_MULTI_MAX + 1))
    assert seg_call(many, api.ROI_MULTI_MAX) > 0 and L.wr_roi_multi_elems(nx, ny, nz, 0, many, api.ROI_MULTI_MAX, offs) > 0
    for arr, nroi in ((good, 0), (many, api.ROI_MULTI_MAX + 1), (None, 3), (good, -1)):
        assert seg_call(arr, nroi) == 0, nroi
        assert L.wr_roi_multi_elems(nx, ny, nz, 0, arr, nroi, offs) == 0, nroi
    # one out-of-range box among good ones: refused, and the message names it
    bad = api._boxes([rois[0], rois[1], ((0, 2), (0, 38), (0, 50))])
    assert seg_call(bad, 3) == 0
    assert L.wr_last_error().decode().startswith("region 2: ")
    assert L.wr_roi_multi_elems(nx, ny, nz, 0, bad, 3, offs) == 0
    assert L.wr_last_error().decode().startswith("region 2: ")
    empty = api._boxes([rois[0], ((3, 3), (0, 1), (0, 1))])
    assert seg_call(empty, 2) == 0 and L.wr_roi_multi_elems(nx, ny, nz, 0, empty, 2, None) == 0
    # a bad seg, a bad brick, a bad level or transform depth
    for seg in (8, 1000, 60000):
        assert seg_call(good, 3, seg=seg) == 0, seg
    assert seg_call(good, 3, brick=12) == 0
    assert seg_call(good, 3, level=5) == 0 and seg_call(good, 3, level=1, wlev=0) == 0 and seg_call(good, 3, wlev=3) == 0
    assert L.wr_roi_multi_elems(nx, ny, nz, 5, good, 3, None) == 0
    with pytest.raises(api.WaveRangeError):
        api.seg_roi_segments_multi(shape, 0, [], 4096)
    with pytest.raises(api.WaveRangeError):
        api.roi_multi_offsets(shape, 0, [])


# ---- sanitizers ----------------------------------------------------------------------------------------------------------
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]  # tests/test_seg_cpu.py


def _have_san():
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write("int main(){return 0;}\n")
        return subprocess.run(["g++"] + SAN + [src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_san(), reason="g++ with ASan/UBSan not available")
def test_union_geometry_under_sanitizers():
    """The union lists of csrc/wr_roi.h and csrc/wr_blocked.h compiled by g++ under ASan + UBSan, on exact-size arrays and
    with cap smaller than the count (tests/native/roimulti_fuzz.cpp): a stand-alone program, nothing is loaded into Python."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "roimulti_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "roimulti_fuzz.cpp"),
                                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "region union sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
