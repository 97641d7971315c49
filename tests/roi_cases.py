"""Regions that pin what a region decode runs on the device (csrc/wr_roi.h, csrc/wr_roi.hip, LowresPlan in csrc/wr_codec.cpp).
A plain module, like fused_cases.py: tests/test_roi_cases_cpu.py asserts the table through wr_roi_plan and the definition
without a GPU, tests/test_gpu_roi_cases.py asserts each plan again in front of every GPU check, so that a change of the window
rule, of the gather's wide/byte rule or of the fused dispatch fails loudly and cannot turn a case into a test of other kernels.

Shapes are (nz, ny, nx), regions ((z0, z1), (y0, y1), (x0, x1)) in the box of their level, axes are numbered 0 = z, 1 = y,
2 = x.  A case is (id, shape, wlev, level, region)."""
LEVELS = range(5)
AXES = "zyx"


def h(n, times=1):
    for _ in range(times):
        n = (n + 1) // 2
    return n


def box_of(shape, level):
    return tuple(h(n, level) for n in shape)


# ---- sweeps: a one-sample region at every position of one axis of the box of every level; of the other two axes the first
# is taken whole and the second over [1, 3) (cut to the box where a coarse level is shorter), so that the crop has an offset
# on an axis that is not swept.
SWEEPS = {
    # level-0 windows are 64 .. 144 long and all run the fused inverse on 3 levels; along x, where the fused inverse wants
    # multiples of 4, on 2 where the window is cut at 408 = 25 * 16 + 8.  The level extents 408, 204, 102, 51, 26 of even_x
    # give wide boxes at the finest levels and byte boxes below in one launch; in even_y / even_z the 32-wide x decides
    "even_x": ((32, 32, 408), 2),
    "even_y": ((32, 408, 32), 1),
    "even_z": ((408, 32, 32), 0),
    # odd true ends at levels 0, 2 and 4 of the swept axis (203, 102, 51, 26, 13), the short axes odd at the others (21 -> 11,
    # 13 -> 7) and down to extents 2 and 3: the general inverse and the byte gather everywhere
    "odd_x": ((13, 21, 203), 2),
    "odd_y": ((21, 203, 13), 1),
    "odd_z": ((203, 13, 21), 0),
}


def sweep_positions(name, level):
    shape, axis = SWEEPS[name]
    return h(shape[axis], level)


def sweep_region(name, level, pos):
    shape, axis = SWEEPS[name]
    box = box_of(shape, level)
    roi = [None] * 3
    roi[axis] = (pos, pos + 1)
    whole, short = [k for k in range(3) if k != axis]
    roi[whole] = (0, box[whole])
    roi[short] = (min(1, box[short] - 1), min(3, box[short]))
    return tuple(roi)


def sweep_regions(name, level):
    return [sweep_region(name, level, pos) for pos in range(sweep_positions(name, level))]


# Pinned plans: PINS[name][level][pos] = ((a, b) of the window along the swept axis, fused levels (0: the general kernels),
# wide boxes, byte boxes) at the first and last position, one in the middle and one on each side of the positions where the
# window lets go of the low end and where it reaches the true end.
PINS = {
    "even_x": {
        0: {0: ((0, 64), 3, 17, 12), 75: ((0, 144), 3, 10, 19), 76: ((16, 144), 3, 10, 19), 204: ((144, 272), 3, 10, 19),
            339: ((272, 400), 3, 10, 19), 340: ((272, 408), 2, 7, 22), 407: ((336, 408), 2, 7, 22)},
        1: {0: ((0, 32), 0, 10, 12), 35: ((0, 64), 0, 10, 12), 36: ((8, 72), 0, 3, 19), 102: ((72, 136), 0, 3, 19),
            171: ((136, 200), 0, 3, 19), 172: ((144, 204), 0, 0, 22), 203: ((168, 204), 0, 0, 22)},
        2: {0: ((0, 16), 0, 7, 8), 15: ((0, 28), 0, 0, 15), 16: ((4, 32), 0, 0, 15), 51: ((36, 64), 0, 0, 15),
            87: ((72, 100), 0, 0, 15), 88: ((76, 102), 0, 0, 15), 101: ((88, 102), 0, 0, 15)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 25: ((20, 30), 0, 0, 8),
            45: ((40, 50), 0, 0, 8), 46: ((42, 51), 0, 0, 8), 50: ((46, 51), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 13: ((13, 14), 0, 0, 1), 25: ((25, 26), 0, 0, 1)},
    },
    "even_y": {
        0: {0: ((0, 64), 3, 21, 8), 75: ((0, 144), 3, 21, 8), 76: ((16, 144), 3, 21, 8), 204: ((144, 272), 3, 21, 8),
            339: ((272, 400), 3, 21, 8), 340: ((272, 408), 3, 21, 8), 407: ((336, 408), 3, 21, 8)},
        1: {0: ((0, 32), 0, 14, 8), 35: ((0, 64), 0, 14, 8), 36: ((8, 72), 0, 14, 8), 102: ((72, 136), 0, 14, 8),
            171: ((136, 200), 0, 14, 8), 172: ((144, 204), 0, 14, 8), 203: ((168, 204), 0, 14, 8)},
        2: {0: ((0, 16), 0, 7, 8), 15: ((0, 28), 0, 7, 8), 16: ((4, 32), 0, 7, 8), 51: ((36, 64), 0, 7, 8),
            87: ((72, 100), 0, 7, 8), 88: ((76, 102), 0, 7, 8), 101: ((88, 102), 0, 7, 8)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 25: ((20, 30), 0, 0, 8),
            45: ((40, 50), 0, 0, 8), 46: ((42, 51), 0, 0, 8), 50: ((46, 51), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 13: ((13, 14), 0, 0, 1), 25: ((25, 26), 0, 0, 1)},
    },
    "even_z": {
        0: {0: ((0, 64), 3, 21, 8), 75: ((0, 144), 3, 21, 8), 76: ((16, 144), 3, 21, 8), 204: ((144, 272), 3, 21, 8),
            339: ((272, 400), 3, 21, 8), 340: ((272, 408), 3, 21, 8), 407: ((336, 408), 3, 21, 8)},
        1: {0: ((0, 32), 0, 14, 8), 35: ((0, 64), 0, 14, 8), 36: ((8, 72), 0, 14, 8), 102: ((72, 136), 0, 14, 8),
            171: ((136, 200), 0, 14, 8), 172: ((144, 204), 0, 14, 8), 203: ((168, 204), 0, 14, 8)},
        2: {0: ((0, 16), 0, 7, 8), 15: ((0, 28), 0, 7, 8), 16: ((4, 32), 0, 7, 8), 51: ((36, 64), 0, 7, 8),
            87: ((72, 100), 0, 7, 8), 88: ((76, 102), 0, 7, 8), 101: ((88, 102), 0, 7, 8)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 25: ((20, 30), 0, 0, 8),
            45: ((40, 50), 0, 0, 8), 46: ((42, 51), 0, 0, 8), 50: ((46, 51), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 13: ((13, 14), 0, 0, 1), 25: ((25, 26), 0, 0, 1)},
    },
    "odd_x": {
        0: {0: ((0, 64), 0, 0, 29), 75: ((0, 144), 0, 0, 29), 76: ((16, 144), 0, 0, 29), 101: ((32, 176), 0, 0, 29),
            131: ((64, 192), 0, 0, 29), 132: ((64, 203), 0, 0, 29), 202: ((128, 203), 0, 0, 29)},
        1: {0: ((0, 32), 0, 0, 22), 35: ((0, 64), 0, 0, 22), 36: ((8, 72), 0, 0, 22), 51: ((16, 80), 0, 0, 22),
            67: ((32, 96), 0, 0, 22), 68: ((40, 102), 0, 0, 22), 101: ((72, 102), 0, 0, 22)},
        2: {0: ((0, 16), 0, 0, 15), 15: ((0, 28), 0, 0, 15), 16: ((4, 32), 0, 0, 15), 25: ((12, 40), 0, 0, 15),
            35: ((20, 48), 0, 0, 15), 36: ((24, 51), 0, 0, 15), 50: ((36, 51), 0, 0, 15)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 13: ((8, 18), 0, 0, 8),
            19: ((14, 24), 0, 0, 8), 20: ((16, 26), 0, 0, 8), 25: ((20, 26), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 6: ((6, 7), 0, 0, 1), 12: ((12, 13), 0, 0, 1)},
    },
    "odd_y": {
        0: {0: ((0, 64), 0, 0, 29), 75: ((0, 144), 0, 0, 29), 76: ((16, 144), 0, 0, 29), 101: ((32, 176), 0, 0, 29),
            131: ((64, 192), 0, 0, 29), 132: ((64, 203), 0, 0, 29), 202: ((128, 203), 0, 0, 29)},
        1: {0: ((0, 32), 0, 0, 22), 35: ((0, 64), 0, 0, 22), 36: ((8, 72), 0, 0, 22), 51: ((16, 80), 0, 0, 22),
            67: ((32, 96), 0, 0, 22), 68: ((40, 102), 0, 0, 22), 101: ((72, 102), 0, 0, 22)},
        2: {0: ((0, 16), 0, 0, 15), 15: ((0, 28), 0, 0, 15), 16: ((4, 32), 0, 0, 15), 25: ((12, 40), 0, 0, 15),
            35: ((20, 48), 0, 0, 15), 36: ((24, 51), 0, 0, 15), 50: ((36, 51), 0, 0, 15)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 13: ((8, 18), 0, 0, 8),
            19: ((14, 24), 0, 0, 8), 20: ((16, 26), 0, 0, 8), 25: ((20, 26), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 6: ((6, 7), 0, 0, 1), 12: ((12, 13), 0, 0, 1)},
    },
    "odd_z": {
        0: {0: ((0, 64), 0, 0, 29), 75: ((0, 144), 0, 0, 29), 76: ((16, 144), 0, 0, 29), 101: ((32, 176), 0, 0, 29),
            131: ((64, 192), 0, 0, 29), 132: ((64, 203), 0, 0, 29), 202: ((128, 203), 0, 0, 29)},
        1: {0: ((0, 32), 0, 0, 22), 35: ((0, 64), 0, 0, 22), 36: ((8, 72), 0, 0, 22), 51: ((16, 80), 0, 0, 22),
            67: ((32, 96), 0, 0, 22), 68: ((40, 102), 0, 0, 22), 101: ((72, 102), 0, 0, 22)},
        2: {0: ((0, 16), 0, 0, 15), 15: ((0, 28), 0, 0, 15), 16: ((4, 32), 0, 0, 15), 25: ((12, 40), 0, 0, 15),
            35: ((20, 48), 0, 0, 15), 36: ((24, 51), 0, 0, 15), 50: ((36, 51), 0, 0, 15)},
        3: {0: ((0, 6), 0, 0, 8), 5: ((0, 10), 0, 0, 8), 6: ((2, 12), 0, 0, 8), 13: ((8, 18), 0, 0, 8),
            19: ((14, 24), 0, 0, 8), 20: ((16, 26), 0, 0, 8), 25: ((20, 26), 0, 0, 8)},
        4: {0: ((0, 1), 0, 0, 1), 1: ((1, 2), 0, 0, 1), 6: ((6, 7), 0, 0, 1), 12: ((12, 13), 0, 0, 1)},
    },
}

# ---- corners: per axis a region at the low end, in the interior, at the high end and the whole axis, all 64 combinations at
# level 0.  x ends even (200: a window of 72 can still run fused, 2 levels), y ends odd (203: the general kernels whenever
# the window reaches it), z is a multiple of 16 (208: its high window is 64 long).  Where y is low or interior the window runs
# fused, on as many levels as its x extent allows: 64 (low), 144 (interior), 72 (high), 200 (whole).
CORNER_FIELD = (208, 203, 200)
CORNER_KINDS = ("low", "interior", "high", "whole")
CORNER_FUSED_BY_X = {"low": 4, "interior": 3, "high": 2, "whole": 2}


def corner_fused_levels(cid):
    _, _, ky, kx = cid.split("-")
    return CORNER_FUSED_BY_X[kx] if ky in ("low", "interior") else 0


def corner_range(n, kind):
    return {"low": (1, 3), "interior": (100, 104), "high": (n - 2, n), "whole": (0, n)}[kind]


def corner_cases():
    out = []
    for kz in CORNER_KINDS:
        for ky in CORNER_KINDS:
            for kx in CORNER_KINDS:
                roi = tuple(corner_range(n, k) for n, k in zip(CORNER_FIELD, (kz, ky, kx)))
                out.append(("corner-%s-%s-%s" % (kz, ky, kx), CORNER_FIELD, 4, 0, roi))
    return out


# ---- degenerate fields and single cases
SINGLES = [
    # every window of a 64-cube at level 0 is the cube: 4 fused levels, every box of the gather wide, 29 of them
    ("cube64", (64, 64, 64), 4, 0, ((30, 31), (30, 31), (30, 31))),
    # a flat field: the z axis has extent 1 at every level, 3 detail boxes per level instead of 7
    ("flat-l0", (1, 50, 300), 4, 0, ((0, 1), (10, 20), (140, 160))),
    ("flat-l2", (1, 50, 300), 4, 2, ((0, 1), (3, 5), (35, 40))),
    ("flat-l4", (1, 50, 300), 4, 4, ((0, 1), (0, 4), (0, 19))),
    # lines of 5: the box extent reaches 1 at level 3 (5, 3, 2, 1, 1), the detail boxes of the coarsest level are empty
    ("linex-l0-mid", (1, 1, 5), 4, 0, ((0, 1), (0, 1), (2, 3))),
    ("linex-l0-whole", (1, 1, 5), 4, 0, ((0, 1), (0, 1), (0, 5))),
    ("linex-l1", (1, 1, 5), 4, 1, ((0, 1), (0, 1), (2, 3))),
    ("linex-l3", (1, 1, 5), 4, 3, ((0, 1), (0, 1), (0, 1))),
    ("linez-l0-mid", (5, 1, 1), 4, 0, ((2, 3), (0, 1), (0, 1))),
    ("linez-l0-whole", (5, 1, 1), 4, 0, ((0, 5), (0, 1), (0, 1))),
    ("linez-l2", (5, 1, 1), 4, 2, ((1, 2), (0, 1), (0, 1))),
    ("linez-l4", (5, 1, 1), 4, 4, ((0, 1), (0, 1), (0, 1))),
    ("liney-l0", (1, 5, 1), 4, 0, ((0, 1), (4, 5), (0, 1))),
    ("small-l0", (3, 2, 5), 4, 0, ((1, 3), (0, 1), (1, 4))),
    ("small-l1", (3, 2, 5), 4, 1, ((0, 2), (0, 1), (2, 3))),
    # streams without the transform: the window is the region, one box; the second one is gathered 4 symbols at a time
    ("wlev0-odd", (13, 21, 50), 0, 0, ((2, 5), (1, 3), (7, 30))),
    ("wlev0-wide", (8, 8, 64), 0, 0, ((0, 8), (2, 4), (4, 36))),
    ("wlev0-point", (13, 21, 50), 0, 0, ((12, 13), (20, 21), (49, 50))),
]


# pinned plans of the single cases: id -> (levels to invert, fused levels, wide boxes, byte boxes)
SINGLE_PLANS = {
    "cube64": (4, 4, 29, 0), "flat-l0": (4, 0, 2, 11), "flat-l2": (2, 0, 4, 3), "flat-l4": (0, 0, 0, 1),
    "linex-l0-mid": (4, 0, 0, 4), "linex-l0-whole": (4, 0, 0, 4), "linex-l1": (3, 0, 0, 3), "linex-l3": (1, 0, 0, 1),
    "linez-l0-mid": (4, 0, 0, 4), "linez-l0-whole": (4, 0, 0, 4), "linez-l2": (2, 0, 0, 2), "linez-l4": (0, 0, 0, 1),
    "liney-l0": (4, 0, 0, 4), "small-l0": (4, 0, 0, 12), "small-l1": (3, 0, 0, 5),
    "wlev0-odd": (0, 0, 0, 1), "wlev0-wide": (0, 0, 1, 0), "wlev0-point": (0, 0, 0, 1),
}


def sweep_cases(name):
    shape, axis = SWEEPS[name]
    return [("%s-l%d-%s%d" % (name, level, AXES[axis], pos), shape, 4, level, sweep_region(name, level, pos))
            for level in LEVELS for pos in range(sweep_positions(name, level))]


def all_cases():
    out = []
    for name in SWEEPS:
        out += sweep_cases(name)
    return out + corner_cases() + SINGLES


# ---- what a plan is a case of
def level_extents(plan):
    """w_l per axis (z, y, x), l = 0 .. inverse"""
    return [[-(-b // (1 << l)) - (a >> l) for l in range(plan["inverse"] + 1)] for a, b in plan["win"]]


def classes(plan):
    """A plan (api.roi_plan) reduced to what decides the kernels' paths: (per-axis window class (z, y, x), per-axis parities of
    w_0 .. w_d as a string of e / o, levels to invert, fused levels (0: the general kernels), wide boxes, byte boxes, boxes
    with lx < 4)."""
    kind = []
    for (a, b), n in zip(plan["win"], plan["box"]):
        kind.append("whole" if (a, b) == (0, n) else "low" if a == 0 else "high" if b == n else "interior")
    parity = tuple("".join("eo"[w & 1] for w in ws) for ws in level_extents(plan))
    wide = sum(b["wide"] for b in plan["boxes"])
    short = sum(b["len"][0] < 4 for b in plan["boxes"])
    assert plan["fused"] == (plan["fused_levels"] > 0)
    return tuple(kind), parity, plan["inverse"], plan["fused_levels"], wide, len(plan["boxes"]) - wide, short


def features(cls):
    """The names under which REQUIRED lists what the table must reach."""
    kind, parity, d, fused, wide, byte, short = cls
    out = {"%s:%s" % (ax, k) for ax, k in zip(AXES, kind)}
    out.add("fused%d" % fused if fused else "general-d%d" % d)
    out |= {"odd-w%d" % l for p in parity for l, c in enumerate(p) if c == "o"}
    out.add("all-wide" if not byte else "all-byte" if not wide else "mixed")
    out.add("nbox%d" % (wide + byte))
    if short:
        out.add("lx<4")
    if fused and "high" in kind:
        out.add("fused-at-a-true-end")
    if d and any(p[0] == "o" and p[-1] == "o" for p in parity):
        out.add("odd-at-both-ends-of-the-chain")
    return out


def check_plan(api, case):
    """assert that the library gives the case the plan it is in the table for (where the table pins one); returns (plan, classes)"""
    cid, shape, wlev, level, roi = case
    plan = api.roi_plan(shape, level, roi, wlev)
    cls = classes(plan)
    if cid in SINGLE_PLANS:
        assert cls[2:6] == SINGLE_PLANS[cid], (cid, cls)
    elif cid.startswith("corner-"):
        assert "corner-" + "-".join(cls[0]) == cid and cls[3] == corner_fused_levels(cid), (cid, cls)
    else:
        name, lvl, pos = cid.rsplit("-", 2)
        pin = PINS[name][int(lvl[1:])].get(int(pos[1:]))
        if pin is not None:
            assert (plan["win"][SWEEPS[name][1]], cls[3], cls[4], cls[5]) == pin, (cid, plan["win"], cls)
        if name.startswith("odd_"):
            assert cls[3] == 0 and cls[4] == 0, (cid, cls)
        elif level == 0:
            assert cls[3] >= 2 and cls[4] and cls[5], (cid, cls)
    return plan, cls


REQUIRED = {
    "fused2", "fused3", "fused4", "general-d4", "general-d3", "general-d2", "general-d1", "general-d0",
    "z:low", "z:interior", "z:high", "z:whole", "y:low", "y:interior", "y:high", "y:whole", "x:low", "x:interior", "x:high", "x:whole",
    "odd-w0", "odd-w1", "odd-w2", "odd-w3",
    "all-wide", "all-byte", "mixed", "lx<4", "nbox29", "nbox1",
}
