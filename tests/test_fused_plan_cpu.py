"""wr_fused_plan (include/waverange_amd.h) without a GPU: the path and the launch geometry of every shape of
tests/fused_cases.py, refused arguments, and the guards that no run can reach."""
import ctypes as C

import pytest

import fused_cases as F
from util import ROOT  # noqa: F401  (puts the repository on sys.path)
from waverange_amd import api

WR_ERR_ARG = -1


@pytest.mark.parametrize("shape", F.SHAPES, ids=F.ident)
def test_table_shapes_take_the_path_they_are_there_for(shape):
    F.check_plan(api, shape)


@pytest.mark.parametrize("shape", sorted(F.EDGE_SHAPES), ids=F.ident)
def test_edge_field_shapes_take_the_path_they_are_there_for(shape):
    F.check_plan(api, shape, F.EDGE_SHAPES[shape])


def test_table_covers_the_classes_it_was_built_for():
    """what the table as a whole must hold, whatever its entries are edited to"""
    fwd = {s: F.CASES[s]["fwd"] for s in F.SHAPES}
    inv = {s: F.CASES[s]["inv"] for s in F.SHAPES}
    one_both = [s for s in F.SHAPES if fwd[s][:2] == (1, True) and inv[s][:2] == (1, True)]
    assert len(one_both) >= 5
    assert any(fwd[s][:2] == (1, True) and inv[s] == F.NOT_FUSED for s in F.SHAPES), "forward fused, inverse general"
    assert any(fwd[s][:2] == (1, False) for s in F.SHAPES) and (128, 128, 130) in one_both, "both sides of 2^21"
    assert 128 * 128 * 126 < 1 << 21 <= 128 * 128 * 130
    level0 = [fwd[s][2][0] for s in F.SHAPES if fwd[s][2]]
    assert max(g[0] for g in level0) >= 33 and max(g[1] for g in level0) >= 129 and max(g[3] for g in level0) > 200
    assert any(g[2] >= 16 and g[4] < g[2] for g in level0), "a long z segment that ends on a shorter one"
    assert any(g[4] == 1 for g in level0), "a last z segment of one pair"
    assert any(g[3] == 1 and g[2] == 4 for g in level0), "a single z segment of the shortest length"
    assert all(s in F.CASES for s in F.ONE_LEVEL) and (512, 512, 8) in F.ONE_LEVEL and (128, 128, 126) not in F.ONE_LEVEL


def test_plan_agrees_with_the_rules_of_the_dispatch():
    """levels / used against the rule stated in wr_kernels.h, and the grid's own consistency, over a sweep of small shapes"""
    dims = [1, 2, 7, 8, 10, 12, 16, 18, 24, 32, 40, 64, 66, 100, 128, 130, 136]
    for nx in dims:
        for ny in dims[::2]:
            for nz in dims[1::3]:
                for inverse in (False, True):
                    p = api.fused_plan((nz, ny, nx), inverse)
                    lv = 0
                    while lv < 4:
                        n = (nx >> lv, ny >> lv, nz >> lv)
                        if any(v & 1 for v in n) or min(n) < 8 or (inverse and n[0] & 3):
                            break
                        lv += 1
                    assert p["levels"] == lv and len(p["grid"]) == lv, (nx, ny, nz, inverse, p)
                    assert p["used"] == (lv >= 2 or (lv == 1 and nx * ny * nz >= 1 << 21))
                    for l, (tx, ty, zps, zsegs, zlast) in enumerate(p["grid"]):
                        m1, m2, m3 = (nx >> l) // 2, (ny >> l) // 2, (nz >> l) // 2
                        assert (tx, ty) == (-(-m1 // 64), -(-m2 // 16))
                        assert zps >= 4 and zsegs == -(-m3 // zps) and 1 <= zlast <= zps and (zsegs - 1) * zps + zlast == m3


def test_planes_of_2_to_the_30_samples_are_never_fused():
    """the kernels' per-plane offsets are 32-bit: fused_levels gives 0 from nx * ny = 2^30 on (no run can reach this:
    such a field with nz >= 8 holds 64 GB)"""
    for inverse in (False, True):
        for shape in ((32768, 32768, 8), (1 << 20, 1 << 10, 16), (1 << 16, 1 << 15, 64)):
            nx, ny, nz = shape
            assert api.fused_plan((nz, ny, nx), inverse) == dict(levels=0, used=False, grid=[])
        p = api.fused_plan((8, 32768, 32768 - 8), inverse)
        assert p["levels"] == 1 and p["used"]


def test_refused_arguments():
    L = api.lib()
    plan = api.FusedPlan()
    assert L.wr_fused_plan(64, 64, 64, 0, None) == WR_ERR_ARG
    for dims in ((0, 64, 64), (64, -1, 64), (64, 64, 0)):
        plan.levels, plan.used = 9, 9
        assert L.wr_fused_plan(*dims, 0, C.byref(plan)) == WR_ERR_ARG
        assert b"dimension" in L.wr_last_error()
        assert (plan.levels, plan.used) == (0, 0), "a refused call leaves an empty plan"
        with pytest.raises(api.WaveRangeError):
            api.fused_plan(dims[::-1])
    # any non-zero `inverse` means inverse; entries from `levels` on are zero
    assert L.wr_fused_plan(258, 130, 66, 7, C.byref(plan)) == 0 and (plan.levels, plan.used) == (0, 0)
    assert L.wr_fused_plan(258, 130, 66, 0, C.byref(plan)) == 0 and (plan.levels, plan.used) == (1, 1)
    assert [getattr(plan.level[1], k) for k, _ in api.FusedLevel._fields_] == [0] * 5
