"""Region sets of the multi-region decode tests (tests/test_roi_multi_cpu.py, tests/test_gpu_roi_multi.py).

A region is ((z0, z1), (y0, y1), (x0, x1)) at level 0 and is carried to the box of a coarser level by the rule of
tests/test_gpu_roi.py::region_at."""
import numpy as np

from waverange_amd import api

SETS = {
    # (203,203,203)
    "S": ((203, 203, 203), (
        ((100, 104),) * 3,                        # a 144^3 window: the fused inverse
        ((0, 3),) * 3,                            # a 64^3 corner window
        ((102, 110),) * 3,                        # overlaps the first
        ((100, 104),) * 3,                        # the first region again
        ((199, 203), (100, 101), (0, 203)),       # a 203 x 144 x 75 window with a true end: the general kernels
    )),
    "T": ((301, 37, 50), (
        ((150, 153), (0, 37), (49, 50)),
        ((0, 2), (0, 37), (0, 50)),
        ((299, 301), (10, 11), (0, 50)),
    )),
    # every window is the whole field
    "W": ((64, 64, 64), (
        ((30, 34), (5, 6), (60, 64)),
        ((0, 64), (0, 64), (0, 64)),
        ((63, 64), (0, 1), (31, 33)),
    )),
}


def carry(shape, level, roi):
    out = []
    for (lo, hi), n in zip(roi, api.lowres_shape(shape, level)):
        a = lo >> level
        out.append((a, min(n, max(a + 1, -(-hi >> level)))))
    return tuple(out)


def regions_at(name, level):
    shape, rois = SETS[name]
    return [carry(shape, level, r) for r in rois]


def single_lists(shape, level, rois, seg, wlev=4, brick=None):
    if brick is None:
        return [api.seg_roi_segments(shape, level, r, seg, wlev) for r in rois]
    return [api.seg_roi_segments_blocked(shape, level, r, seg, wlev, brick) for r in rois]


def union_of(lists):
    return np.unique(np.concatenate(lists)).astype(np.uint32)
