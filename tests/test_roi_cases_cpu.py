"""The table of tests/roi_cases.py without a GPU: every case's plan (wr_roi_plan) against the definition as tests/test_roi_cpu.py
restates it, the classes the table must reach, the exactness argument and the segment lists at every position of the sweeps.
Nothing here has a tolerance: windows, boxes and lists are integers, values are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the repository on sys.path)
import roi_cases as rc
from test_blocked_cpu import pi_of
from test_roi_cpu import WR_ERR_ARG, c_box, region_is_exact, source_coordinates, window
from oracle.loader import Oracle
from waverange_amd import api

SWEEP_NAMES = list(rc.SWEEPS)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def plan_of(case):
    _, shape, wlev, level, roi = case
    return api.roi_plan(shape, level, roi, wlev)


# ---- the rules, restated
def fused_levels_by_rule(wz, wy, wx):
    """csrc/wr_fused.hip, fused_levels (inverse): the finest levels whose boxes are even in every direction, at least 8 long
    and a multiple of 4 in x; a window runs fused from two such levels on, or one of 2^21 samples"""
    f = 0
    while f < 4:
        n = [wx >> f, wy >> f, wz >> f]
        if any(v & 1 for v in n) or min(n) < 8 or n[0] & 3:
            break
        f += 1
    return f if f >= 2 or (f == 1 and wx * wy * wz >= 1 << 21) else 0


def wide_by_rule(nx, wx, box):
    """csrc/wr_roi.hip, WindowItems: the run's offsets in the plane and in the window and its length are multiples of 4"""
    return nx % 4 == 0 and wx % 4 == 0 and box["src"][0] % 4 == 0 and box["dst"][0] % 4 == 0 and box["len"][0] % 4 == 0


_VERIFIED = {}  # (shape, wlev, level, window) -> the box list that was compared with the definition point by point


def check_plan_against_the_definition(case):
    """Every position has its plan asked for and its window, path and flags compared; the point-by-point comparison of the
    box list runs once per distinct window of a field (a sweep's positions share about one window per 2^d positions), the
    other positions must carry that very list."""
    cid, shape, wlev, level, roi = case
    plan = plan_of(case)
    box, d = rc.box_of(shape, level), wlev - level
    assert plan["box"] == box and plan["inverse"] == d, cid
    wins = tuple(window(n, lo, hi, d) for n, (lo, hi) in zip(box, roi))
    assert plan["win"] == wins == api.roi_window(shape, level, roi, wlev), cid
    wz, wy, wx = (b - a for a, b in wins)
    want_fused = fused_levels_by_rule(wz, wy, wx) if d == 4 else 0
    assert (plan["fused"], plan["fused_levels"]) == (want_fused > 0, want_fused), (cid, rc.classes(plan))
    assert 1 <= len(plan["boxes"]) <= 29
    for b in plan["boxes"]:
        assert b["wide"] == wide_by_rule(shape[2], wx, b), (cid, b)
    key = (shape, wlev, level, wins)
    if key in _VERIFIED:
        assert plan["boxes"] == _VERIFIED[key], cid
        return plan
    # the boxes, applied point by point, are the definition's map; they tile the window
    fz = np.full((wz, wy, wx), -1, dtype=np.int64)
    fy, fx = fz.copy(), fz.copy()
    for b in plan["boxes"]:
        (sx, sy, sz), (ox, oy, oz), (lx, ly, lz) = b["src"], b["dst"], b["len"]
        assert min(lx, ly, lz) >= 1 and ox + lx <= wx and oy + ly <= wy and oz + lz <= wz, (cid, b)
        at = (slice(oz, oz + lz), slice(oy, oy + ly), slice(ox, ox + lx))
        assert np.all(fz[at] == -1), (cid, b, "boxes overlap")
        fz[at] = (sz + np.arange(lz))[:, None, None]
        fy[at] = (sy + np.arange(ly))[None, :, None]
        fx[at] = (sx + np.arange(lx))[None, None, :]
    want = source_coordinates(box, wins, d)
    assert np.array_equal(fz, want[0]) and np.array_equal(fy, want[1]) and np.array_equal(fx, want[2]), (cid, rc.classes(plan))
    # every source lies inside the field: the gather reads nothing else
    assert fz.min() >= 0 and fy.min() >= 0 and fx.min() >= 0 and fz.max() < shape[0] and fy.max() < shape[1] and fx.max() < shape[2], cid
    _VERIFIED[key] = plan["boxes"]
    return plan


# ---- the table
@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_sweep_plans_are_the_definition(name):
    for case in rc.sweep_cases(name):
        check_plan_against_the_definition(case)


@pytest.mark.parametrize("kz", rc.CORNER_KINDS)
@pytest.mark.parametrize("ky", rc.CORNER_KINDS)
def test_corner_plans_are_the_definition(kz, ky):
    cases = [c for c in rc.corner_cases() if c[0].startswith("corner-%s-%s-" % (kz, ky))]
    assert len(cases) == 4 and len(rc.corner_cases()) == 64
    for case in cases:
        plan = check_plan_against_the_definition(case)
        assert "corner-" + "-".join(rc.classes(plan)[0]) == case[0], case[0]  # the region is of the class its name says, on every axis


def test_single_plans_are_the_definition():
    assert len({c[0] for c in rc.all_cases()}) == len(rc.all_cases())
    for case in rc.SINGLES:
        check_plan_against_the_definition(case)


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_pinned_plans(name):
    shape, axis = rc.SWEEPS[name]
    assert sorted(rc.PINS[name]) == list(rc.LEVELS)
    for level, pins in rc.PINS[name].items():
        n = rc.sweep_positions(name, level)
        assert {0, n // 2, n - 1} <= set(pins), (name, level)
        for pos, (win, fused, wide, byte) in pins.items():
            plan = api.roi_plan(shape, level, rc.sweep_region(name, level, pos))
            cls = rc.classes(plan)
            assert (plan["win"][axis], cls[3], cls[4], cls[5]) == (win, fused, wide, byte), (name, level, pos, plan["win"], cls)
        if level < 4:  # the pins sit on both sides of the two clips
            for p, q in zip(sorted(pins), sorted(pins)[1:]):
                if q == p + 1:
                    a0, b0 = pins[p][0]
                    a1, b1 = pins[q][0]
                    assert (a0 == 0 and a1 > 0) or (b0 < n and b1 == n), (name, level, p, q)


def test_sweeps_at_level_0_run_what_they_are_there_for():
    for name in ("even_x", "even_y", "even_z"):
        shape, axis = rc.SWEEPS[name]
        for pos in range(rc.sweep_positions(name, 0)):
            plan = api.roi_plan(shape, 0, rc.sweep_region(name, 0, pos))
            a, b = plan["win"][axis]
            cut = name == "even_x" and b == 408
            assert 64 <= b - a <= 144 and plan["fused_levels"] == (2 if cut else 3), (name, pos, plan["win"])
            kinds = {bx["wide"] for bx in plan["boxes"]}
            assert kinds == {True, False}, (name, pos)  # both kinds of gather in one launch
    for name in ("odd_x", "odd_y", "odd_z"):
        shape, axis = rc.SWEEPS[name]
        for level in rc.LEVELS:
            for pos in range(rc.sweep_positions(name, level)):
                plan = api.roi_plan(shape, level, rc.sweep_region(name, level, pos))
                assert not plan["fused"] and not any(bx["wide"] for bx in plan["boxes"]), (name, level, pos)


def test_required_classes_are_reached():
    reached, seen = set(), {}
    for case in rc.all_cases():
        cls = rc.classes(plan_of(case))
        seen.setdefault(cls, case[0])
        reached |= rc.features(cls)
    assert rc.REQUIRED <= reached, sorted(rc.REQUIRED - reached)
    # distinct (axis classes, parities, depth, fused levels, wide, byte, short) tuples: the table may grow, not shrink
    assert len(rc.all_cases()) >= 3640 and len(seen) >= 233, (len(rc.all_cases()), len(seen))


# ---- the exactness argument at every position of every sweep
class Exactness:
    """region_is_exact of tests/test_roi_cpu.py, step by step, for many regions of one box: the random coefficient array and
    its full inverse are made once per box, and the inverse of a window once per distinct window (a sweep's positions share
    about one window per 2^d positions); the crop and the comparison of bit patterns happen at every position."""

    def __init__(self, oracle, rng, box, d):
        self.oracle, self.box, self.d = oracle, box, d
        self.coef = rng.standard_normal(box)
        self.full = oracle.cdf97_3d(self.coef.copy(), -d) if d else self.coef
        self.inv = {}

    def holds(self, shape, level, roi):
        wins = api.roi_window(shape, level, roi)
        if wins not in self.inv:
            fz, fy, fx = source_coordinates(self.box, wins, self.d)
            win = np.ascontiguousarray(self.coef[fz, fy, fx])
            assert win.shape == tuple(b - a for a, b in wins)
            self.inv = {wins: self.oracle.cdf97_3d(win, -self.d) if self.d else win}  # (one window at a time)
        got = self.inv[wins][tuple(slice(lo - a, hi - a) for (lo, hi), (a, _) in zip(roi, wins))]
        want = self.full[tuple(slice(lo, hi) for lo, hi in roi)]
        return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def test_the_shared_exactness_check_is_region_is_exact(oracle):
    """the same verdicts as the function it restates, on a case that holds and on a window one level pair too short"""
    shape, level, roi = (13, 21, 203), 0, ((0, 13), (1, 3), (100, 101))
    assert region_is_exact(oracle, np.random.default_rng(5), shape, roi, 4)
    ex = Exactness(oracle, np.random.default_rng(5), shape, 4)
    assert ex.holds(shape, level, roi)
    ex.inv = {api.roi_window(shape, level, roi): ex.inv[api.roi_window(shape, level, roi)] + 1e-9}
    assert not ex.holds(shape, level, roi)


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_every_sweep_position_is_exact(oracle, name):
    shape, _ = rc.SWEEPS[name]
    rng = np.random.default_rng(3)
    for level in rc.LEVELS:
        ex = Exactness(oracle, rng, rc.box_of(shape, level), 4 - level)
        for pos in range(rc.sweep_positions(name, level)):
            roi = rc.sweep_region(name, level, pos)
            assert ex.holds(shape, level, roi), (name, level, pos, rc.classes(api.roi_plan(shape, level, roi)))


def test_singles_and_corners_are_exact(oracle):
    rng = np.random.default_rng(4)
    for cid, shape, wlev, level, roi in rc.SINGLES:
        if wlev == 4:  # (region_is_exact takes the box and the depth of a four-level stream)
            assert region_is_exact(oracle, rng, rc.box_of(shape, level), roi, 4 - level), cid
    ex = Exactness(oracle, rng, rc.CORNER_FIELD, 4)
    for cid, shape, _, level, roi in rc.corner_cases()[::5]:
        assert ex.holds(shape, level, roi), cid


# ---- segment lists at sweep positions
def source_index(shape, level, roi):
    """index of every source point of the window in the field's array, through the definition's map (the brute force of
    tests/test_roi_cpu.py and tests/test_blocked_cpu.py, once per region for all segment lengths)"""
    nz, ny, nx = shape
    box, d = rc.box_of(shape, level), 4 - level
    wins = [window(n, lo, hi, d) for n, (lo, hi) in zip(box, roi)]
    fz, fy, fx = source_coordinates(box, wins, d)
    return (fx + nx * (fy + ny * fz)).ravel()


def ids_of(index, seg):
    return np.unique(index // seg)


def check_segment_lists(name, levels, brick):
    shape, _ = rc.SWEEPS[name]
    pi = pi_of(shape, 4, brick).astype(np.int64)
    inv = np.empty(pi.size, dtype=np.int64)
    inv[pi] = np.arange(pi.size)
    for level in levels:
        want = {}  # window -> the four brute-force lists (a list depends on the region through its window only)
        for pos in range(rc.sweep_positions(name, level)):
            roi = rc.sweep_region(name, level, pos)
            wins = tuple(window(n, lo, hi, 4 - level) for n, (lo, hi) in zip(rc.box_of(shape, level), roi))
            if wins not in want:
                index = source_index(shape, level, roi)
                want[wins] = {(seg, b): ids_of(inv[index] if b else index, seg or api.SEG_DEFAULT) for seg in (1008, 0) for b in (0, brick)}
            for seg in (1008, 0):
                got = api.seg_roi_segments(shape, level, roi, seg)
                assert np.array_equal(got.astype(np.int64), want[wins][seg, 0]), (name, level, pos, seg)
                got = api.seg_roi_segments_blocked(shape, level, roi, seg, brick=brick)
                assert np.array_equal(got.astype(np.int64), want[wins][seg, brick]), (name, level, pos, seg, brick)


@pytest.mark.parametrize("name,brick", [("odd_x", 8), ("odd_y", 16), ("odd_z", 8)])
def test_segment_lists_of_the_odd_sweeps(name, brick):
    check_segment_lists(name, rc.LEVELS, brick)


def test_segment_lists_of_even_x():
    check_segment_lists("even_x", (0, 3), 8)


# ---- refusals
def test_refusals():
    fn = api.lib().wr_roi_plan
    good = ((1, 2), (3, 5), (0, 64))
    plan = api.RoiPlan()

    def refused(roi, level=0, wlev=4, dims=(64, 64, 64)):
        plan.nbox = plan.inverse = -7  # a refused call leaves the plan alone
        return fn(*dims, level, wlev, C.byref(c_box(roi)), C.byref(plan)) == WR_ERR_ARG and (plan.nbox, plan.inverse) == (-7, -7)

    assert fn(64, 64, 64, 0, 4, C.byref(c_box(good)), C.byref(plan)) == 0 and plan.nbox == 29 and plan.inverse == 4
    assert fn(64, 64, 64, 0, 4, C.byref(c_box(good)), None) == WR_ERR_ARG
    assert "out is NULL" in api.lib().wr_last_error().decode()
    assert fn(64, 64, 64, 0, 4, None, C.byref(plan)) == WR_ERR_ARG
    for roi in (((1, 1), (3, 5), (0, 64)), ((2, 1), (3, 5), (0, 64)),           # empty
                ((1, 2), (3, 65), (0, 64)), ((-1, 2), (3, 5), (0, 64)), ((1, 2), (3, 5), (0, 65)), ((64, 65), (3, 5), (0, 64))):
        assert refused(roi), roi
        with pytest.raises(api.WaveRangeError):
            api.roi_plan((64, 64, 64), 0, roi)
    assert refused(((1, 2), (3, 5), (0, 33)), level=1)      # the box of level 1 is 32 wide
    assert not refused(((1, 2), (3, 5), (0, 32)), level=1)
    assert refused(good, level=5) and refused(good, level=-1)
    assert refused(((0, 1),) * 3, level=1, wlev=0)          # level > wlev
    assert refused(good, wlev=3)
    assert refused(good, dims=(0, 64, 64))


def test_the_plan_follows_the_environment_switch(monkeypatch):
    """the plan reports what the library decides: WR_NO_FUSED sends every window to the general kernels"""
    case = rc.SINGLES[0]
    assert plan_of(case)["fused_levels"] == 4
    monkeypatch.setenv("WR_NO_FUSED", "1")
    plan = plan_of(case)
    assert not plan["fused"] and plan["fused_levels"] == 0
