"""Host geometry of the masked region decode across a batch of fields (include/waverange_amd.h): the union of the mask
segments of several regions (wr_mask_roi_segments_multi) against the brute-force union, the turn prefix of the restore launch
(wr_mask_boxes_turns) against the simulated walk of masked_roi_batch_cases.py, the sizing function, that the case table reaches
every class it is there for, and the planner, the prefix and the blobs' validation order under ASan + UBSan in a stand-alone
program.  No GPU."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import masked_roi_batch_cases as bc
import masked_roi_cases as mc
from util import ROOT
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")


def zyx(shape):
    nx, ny, nz = shape
    return nz, ny, nx


def test_the_table_reaches_every_required_class():
    reached = set()
    for case in bc.CASES:
        reached |= bc.classes_of(case)
        assert 3 <= len(case[4]) <= 5 and 1 <= len(case[2]) <= 6, bc.case_id(case)
        for f in bc.masked_fields(case):  # (a field without a defined sample cannot be encoded)
            assert bc.und_of(case, f).any() and not bc.und_of(case, f).all(), bc.case_id(case)
    assert bc.REQUIRED <= reached, sorted(bc.REQUIRED - reached)
    # the reasons some cases are in the table
    first = bc.first_of(bc.CASES[0])
    assert first.tolist() == [0, 16, 17, 20, 21, 22] and 22 % bc.WAVES_PER_BLOCK
    big = next(c for c in bc.CASES if c[0] == mc.FUSED and c[1] == 0)
    turns = len(bc.masked_fields(big)) * int(bc.first_of(big)[-1])
    assert turns == 3 * 9217 and bc.grid_waves(turns) == 8192 < turns


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_union_is_the_brute_force_union(case):
    shape, level, rois, seg, _ = case
    got = api.mask_roi_segments_multi(zyx(shape), level, rois, seg)
    want = bc.brute_segments_multi(case)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    per = [api.mask_roi_segments(zyx(shape), level, r, seg) for r in rois]
    assert np.array_equal(got, np.unique(np.concatenate(per)))
    assert (np.diff(got.astype(np.int64)) > 0).all() and got[-1] < -(-mc.nsym_of(shape) // (seg or mc.SEG_DEFAULT))
    # the count without an array, and a short array
    nx, ny, nz = shape
    arr = api._boxes(rois)
    lib = api.lib()
    assert lib.wr_mask_roi_segments_multi(nx, ny, nz, level, arr, len(rois), seg, None, 0) == len(want)
    few = np.full(3, 0xFFFFFFFF, np.uint32)
    assert lib.wr_mask_roi_segments_multi(nx, ny, nz, level, arr, len(rois), seg, few.ctypes.data, 2) == len(want)
    assert few[:2].tolist() == want[:2].tolist() + [0xFFFFFFFF] * (2 - min(2, len(want))) and few[2] == 0xFFFFFFFF


def test_union_and_prefix_refuse_what_the_element_count_refuses():
    lib = api.lib()
    nx, ny, nz = mc.CHAIN
    ok = [((0, 1), (0, 2), (0, 3))]
    bad_lists = [[], ok + [((0, 1), (1, 1), (0, 3))], [((0, 1), (0, 2), (0, 4))], [((0, 2), (0, 2), (0, 3))]]
    for rois in bad_lists:
        arr = api._boxes(rois)
        assert lib.wr_roi_multi_elems(nx, ny, nz, 4, arr, len(rois), None) == 0
        assert lib.wr_mask_roi_segments_multi(nx, ny, nz, 4, arr, len(rois), 16, None, 0) == 0
        assert lib.wr_mask_boxes_turns(nx, ny, nz, 4, arr, len(rois), None) == 0
    arr = api._boxes(ok)
    assert lib.wr_mask_roi_segments_multi(nx, ny, nz, 4, arr, 1, 16, None, 0) == 2
    assert lib.wr_mask_boxes_turns(nx, ny, nz, 4, arr, 1, None) == 2
    for level, seg in [(5, 16), (-1, 16), (4, 17), (4, 8), (4, 60000)]:
        assert lib.wr_mask_roi_segments_multi(nx, ny, nz, level, arr, 1, seg, None, 0) == 0
    assert lib.wr_mask_boxes_turns(nx, ny, nz, 5, arr, 1, None) == 0
    assert lib.wr_mask_boxes_turns(nx, ny, nz, 4, None, 1, None) == 0
    assert lib.wr_mask_boxes_turns(nx, ny, nz, 4, api._boxes(ok * 1025), 1025, None) == 0
    # 2^31 turns or more: 2048 x 1024 x 1024 samples in one-sample rows ... as 1024 regions of 2^21 rows each
    rows = [((0, 1024), (0, 2048), (0, 1))] * 1024
    assert lib.wr_mask_boxes_turns(1, 2048, 1024, 0, api._boxes(rows), 1024, None) == 0
    assert lib.wr_mask_boxes_turns(1, 2048, 1024, 0, api._boxes(rows[:1023]), 1023, None) == 1023 << 21


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_prefix_is_the_simulated_walk(case):
    shape, level, rois, _, _ = case
    turns, first = api.mask_boxes_turns(zyx(shape), level, rois)
    want = bc.first_of(case)
    assert first.dtype == np.uint32 and np.array_equal(first.astype(np.int64), want) and turns == int(want[-1])
    # every turn of the launch maps to exactly one (item, row, turn), found by search in first[] as the kernel finds it
    sim = bc.walk(case)
    nm = len(bc.masked_fields(case))
    assert len(sim) == nm * turns and len(set(sim)) == len(sim)
    tpr = [-(-mc.out_shape(bc.single(case, i))[2] // 64) for i in range(len(rois))]
    step = max(1, len(sim) // 5000)  # (the 64^3 case has 27651 turns: every turn near an item's ends, a stride elsewhere)
    near = {int(m * turns + f + d) for m in range(nm) for f in want for d in (-2, -1, 0, 1)}
    for t in sorted(set(range(0, len(sim), step)) | {t for t in near if 0 <= t < len(sim)}):
        m, u = divmod(t, turns)
        i = int(np.searchsorted(first, u, side="right")) - 1
        q = u - int(first[i])
        assert (m, i, q // tpr[i], q % tpr[i]) == sim[t], t
    # the items' turns are what the single-box kernel walks for each region
    for i in range(len(rois)):
        assert int(want[i + 1] - want[i]) == sum(1 for _ in mc.turns_of(bc.single(case, i)))


def test_sizing_function():
    plain, masked = api.seg_roi_batch_device_bytes, api.seg_roi_batch_device_bytes_masked
    n = 64 ** 3
    for nf, planes, seg, brick, strands, out in [(1, 3, 0, 0, 0, 0), (8, 4, 4096, 0, 0, 1000), (5, 2, 1024, 8, 0, 77), (4, 3, 1024, 0, 4, 0), (3, 0, 0, 0, 0, 5)]:
        assert masked(nf, 0, n, planes, seg, brick, strands, 16, out) == plain(nf, n, planes, seg, brick, strands, out) > 0
        prev = plain(nf, n, planes, seg, brick, strands, out)
        for nm in range(1, nf + 1):  # every masked field adds its job
            size = masked(nf, nm, n, planes, seg, brick, strands, 48, out)
            nsym = -(-n // 8)
            assert size >= prev + api.lib().wr_plane_pitch(nsym) + api.mask_bound(n, 48)
            prev = size
        # ... and more fields, more planes, more output never take less
        assert masked(nf + 1, nf, n, planes, seg, brick, strands, 48, out) >= masked(nf, nf, n, planes, seg, brick, strands, 48, out)
        if planes < 4:
            assert masked(nf, nf, n, planes + 1, seg, brick, strands, 48, out) >= masked(nf, nf, n, planes, seg, brick, strands, 48, out)
        assert masked(nf, nf, n, planes, seg, brick, strands, 48, out + 1000) >= masked(nf, nf, n, planes, seg, brick, strands, 48, out)
        assert masked(nf, nf, 2 * n, planes, seg, brick, strands, 48, out) > masked(nf, nf, n, planes, seg, brick, strands, 48, out)
    # refusals
    assert masked(4, 5, n, 2) == 0 and masked(4, -1, n, 2) == 0 and masked(0, 0, n, 2) == 0 and masked(4, 2, 0, 2) == 0
    assert masked(4, 2, n, 2, mask_seg=17) == 0 and masked(4, 2, n, 2, seg=17) == 0 and masked(4, 2, n, 99) == 0
    assert masked(4, 2, n, 2, brick=3) == 0 and masked(4, 2, n, 2, strands=3) == 0
    assert api.SEG_BATCH_MAX == 1024
    assert masked(256, 0, n, 4) > 0 and masked(256, 1, n, 4) == 0  # 1024 jobs, and one more
    assert masked(255, 4, n, 4) > 0 and masked(255, 5, n, 4) == 0
    assert masked(1024, 0, n, 0) > 0 and masked(1024, 1024, n, 0) > 0 and masked(1025, 0, n, 0) == plain(1025, n, 0)


def test_groups_are_cut_by_the_masked_size():
    n, planes = 64 ** 3, 3
    one = api.seg_roi_batch_device_bytes_masked(1, 1, n, planes, out_elems=100)
    four = api.seg_roi_batch_device_bytes_masked(4, 4, n, planes, out_elems=100)
    groups, alone = api.roi_batch_groups_masked(10, n, planes, four, out_elems=100)
    assert [list(g) for g in groups] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]] and alone == []
    groups, alone = api.roi_batch_groups_masked(3, n, planes, one - 1, out_elems=100)
    assert [list(g) for g in groups] == [[0], [1], [2]] and alone == [0, 1, 2]
    # a masked field takes more than an unmasked one: the budget of four unmasked fields holds four of those, three masked ones
    four_plain = api.seg_roi_batch_device_bytes(4, n, planes, out_elems=100)
    assert four_plain < four
    flags = [False, False, False, False, True, True, True, True, True, True]
    g_mixed, _ = api.roi_batch_groups_masked(10, n, planes, four_plain, masked=flags, out_elems=100)
    assert [list(g) for g in g_mixed] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    g_plain, _ = api.roi_batch_groups(10, n, planes, four, out_elems=100)
    g_none, _ = api.roi_batch_groups_masked(10, n, planes, four, masked=False, out_elems=100)
    assert [list(g) for g in g_plain] == [list(g) for g in g_none]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_and_prefix_under_sanitizers():
    """wrmask::roi_segments_multi, wrmask::boxes_turns and the host checks of a batch's blobs, compiled by g++ under ASan + UBSan
    (tests/native/maskroibatch_fuzz.cpp): a stand-alone program, nothing is loaded into Python."""
    san = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with tempfile.TemporaryDirectory() as d:
        probe = os.path.join(d, "t.cpp")
        open(probe, "w").write("int main(){return 0;}\n")
        if subprocess.run(["g++"] + san + [probe, "-o", os.path.join(d, "t")], capture_output=True).returncode != 0:
            pytest.skip("g++ with ASan/UBSan not available")
        exe = os.path.join(d, "maskroibatch_fuzz")
        subprocess.check_call(["g++"] + san + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "maskroibatch_fuzz.cpp"),
                                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "mask batch sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
