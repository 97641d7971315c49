"""Host geometry of the masked region / low-resolution decode (include/waverange_amd.h): which segments of the mask plane a
region needs (wr_mask_roi_segments) against the brute-force definition, over the case table of masked_roi_cases.py; that the
table reaches every path class it is there for; and that every mask byte the restore kernel's definition reads lies in a listed
segment.  No GPU."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import masked_roi_cases as mc
from util import ROOT
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_list_is_the_brute_force_set(case):
    shape, level, roi, seg = case
    nx, ny, nz = shape
    got = api.mask_roi_segments((nz, ny, nx), level, roi, seg)
    want = mc.brute_segments(case)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    nseg = -(-mc.nsym_of(shape) // mc.seg_len(case))
    assert got[-1] < nseg and (np.diff(got.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("shape", [mc.ODD, mc.LONG, mc.CHAIN, mc.GENERAL, mc.FUSED], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("seg", [16, 48, 0])
def test_whole_box_at_level_0_lists_every_segment(shape, seg):
    nx, ny, nz = shape
    nseg = -(-mc.nsym_of(shape) // (seg or mc.SEG_DEFAULT))
    assert np.array_equal(api.mask_roi_segments((nz, ny, nx), 0, None, seg), np.arange(nseg, dtype=np.uint32))
    whole = ((0, nz), (0, ny), (0, nx))
    assert np.array_equal(api.mask_roi_segments((nz, ny, nx), 0, whole, seg), np.arange(nseg, dtype=np.uint32))


def test_refused_arguments_return_0():
    shape = (9, 17, 33)  # (nz, ny, nx); the level-4 box is 3 x 2 x 1
    ok = ((0, 1), (0, 2), (0, 3))
    assert api.mask_roi_segments(shape, 4, ok, 16).tolist() == [0, 4]  # rows y = 0 and y = 16: bits 0 .. 32 and 528 .. 560
    for level, roi, seg in [(5, ok, 16), (-1, ok, 16), (4, ((0, 1), (0, 2), (0, 4)), 16), (4, ((0, 2), (0, 2), (0, 3)), 16), (4, ((0, 1), (1, 1), (0, 3)), 16),
                            (4, ((0, 1), (0, 2), (-1, 3)), 16), (0, ok, 17), (0, ok, 8), (0, ok, 60000)]:
        assert len(api.mask_roi_segments(shape, level, roi, seg)) == 0, (level, roi, seg)
    for bad in [(0, 17, 33), (9, 0, 33), (9, 17, -3)]:
        assert len(api.mask_roi_segments(bad, 0, None, 16)) == 0
    # the count without an array, and a short array
    lib = api.lib()
    assert lib.wr_mask_roi_segments(33, 17, 9, 0, None, 16, None, 0) == 40  # ceil(ceil(5049 / 8) / 16)
    few = np.full(4, 0xFFFFFFFF, np.uint32)
    assert lib.wr_mask_roi_segments(33, 17, 9, 0, None, 16, few.ctypes.data, 3) == 40
    assert few.tolist() == [0, 1, 2, 0xFFFFFFFF]


def test_the_table_reaches_every_required_class():
    reached = set()
    for case in mc.CASES:
        reached |= mc.classes_of(case)
    assert mc.REQUIRED <= reached, sorted(mc.REQUIRED - reached)
    # the reasons the shapes are in the table
    assert 13 % 8 == 5 and 149 % 8 == 5 and 149 == 2 * 64 + 21
    assert [mc.box_of(mc.CHAIN, r)[0] for r in range(5)] == [33, 17, 9, 5, 3] and 2 << 4 == 32
    assert {"word offset %d" % k for k in range(8)} <= mc.classes_of((mc.ODD, 0, ((1, 3), (0, 8), (2, 11)), 16))
    assert "the field's last sample" in mc.classes_of((mc.CHAIN, 3, None, 16))
    # a small region lists fewer segments than the mask has
    for case in mc.CASES:
        shape, level, roi, seg = case
        if roi is not None and seg and shape in (mc.GENERAL, mc.FUSED):
            assert len(mc.brute_segments(case)) < -(-mc.nsym_of(shape) // seg), mc.case_id(case)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_every_byte_the_kernel_reads_lies_in_a_listed_segment(case):
    shape, level, roi, seg = case
    nx, ny, nz = shape
    listed = set(api.mask_roi_segments((nz, ny, nx), level, roi, seg).tolist())
    reads = mc.kernel_reads(case)
    assert reads and max(reads) < mc.nsym_of(shape)
    assert {b // mc.seg_len(case) for b in reads} <= listed
    # at level 0 a turn's word comes from at most nine bytes
    if level == 0:
        for js in mc.turns_of(case):
            assert (int(js[-1]) >> 3) - (int(js[0]) >> 3) <= 8


def test_coarse_mask_is_the_strided_mask():
    """the definition: sample (i, j, k) of the level's box is undefined iff sample (i << r, j << r, k << r) of the field is"""
    for case in mc.CASES:
        shape = case[0]
        und = mc.und_recipe(shape)
        want = und.reshape(-1)[mc.bit_index(case)]
        assert np.array_equal(mc.coarse_und(und, case), want), mc.case_id(case)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_mask_crop_under_sanitizers():
    """wrmask::roi_segments and the host checks of the mask blob, compiled by g++ under ASan + UBSan
    (tests/native/maskroi_fuzz.cpp): a stand-alone program, nothing is loaded into Python."""
    san = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with tempfile.TemporaryDirectory() as d:
        probe = os.path.join(d, "t.cpp")
        open(probe, "w").write("int main(){return 0;}\n")
        if subprocess.run(["g++"] + san + [probe, "-o", os.path.join(d, "t")], capture_output=True).returncode != 0:
            pytest.skip("g++ with ASan/UBSan not available")
        exe = os.path.join(d, "maskroi_fuzz")
        subprocess.check_call(["g++"] + san + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "maskroi_fuzz.cpp"),
                                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "mask crop sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
