"""Where the box ends inside the LAST tile of the fused transform kernels (csrc/wr_fused.hip).  tests/fused_cases.py pins the
launch geometry (tile counts, zps, zsegs, zlast, one-level dispatch); the tile code has no edge branches, and what happens
where a level's box ends inside a tile is index arithmetic: the right-edge mirror patched into LDS at iL = m1 - 1 - px0
(it reaches back into the left halo for a remainder of 1, 2 or 3 pairs), the forward x stage's last lane group one pair
short, `own = px0 + spair < m1` behind the inverse's quad transpose, mirror() and `oy + yp < m2` in y, a last z segment
shorter than its own warm-up.  This module sweeps every remainder.  A plain module: no GPU, no oracle.

Shapes are (nx, ny, nz).  TABLE[shape] = dict(fwd=PLAN, inv=PLAN), PLAN = (levels, used, grid) as api.fused_plan
gives it and as model_plan() below restates it; tests/test_fused_edge_cases_cpu.py asserts every entry through
wr_fused_plan without a GPU, tests/test_gpu_fused_edges.py asserts it again in front of every GPU check.

Path classes of a shape (classes()), over every level the fused path really runs (`used`):
  (d, "x", r), (d, "y", r)   r = pairs of the level's box in its last tile column / row (1 .. 64, 1 .. 16)
  (d, "z", "one")            a single z segment
  (d, "z", 1 | 2 | 3 | 4)    two segments or more, the last one 1, 2, 3 or >= 4 z-pairs long (warm-up: 2 pairs, drain: 1)
  (d, "x1", r)               level-0 remainder on the one-level path (forward: an odd r needs nx % 4 == 2, inverse: r = 2
                             (mod 4) needs nx % 8 == 4; either way level 1 is not fused)
  (d, "blocked_short")       XCD-blocked tile order (tiles_y % 8 == 0) with a last tile column of fewer than 64 pairs
REQUIRED is what the table must reach, as a condition."""
import numpy as np

from waverange_amd import synth

# tile sizes of csrc/wr_fused.hip in sample PAIRS: TXP x TYP forward, ITXP x ITYP inverse.  The CPU test holds the plan's
# tile counts against them, so a change of tile size breaks this table instead of retargeting it.
TXP, TYP = 64, 16
ITXP, ITYP = 64, 16
WG_PER_ROUND = 256      # one workgroup per CU (LDS) on 256 CUs: what pick_zps counts rounds of, either direction
DIRS = ("fwd", "inv")


# ---- the dispatch rule (wr_kernels.h, fused_levels / fused_ok / fused_grid / pick_zps) restated; asserted against
# wr_fused_plan for every shape of the table
def model_levels(nx, ny, nz, inverse):
    lv = 0
    while lv < 4:
        n = (nx >> lv, ny >> lv, nz >> lv)
        if any(v & 1 for v in n) or min(n) < 8 or (inverse and n[0] & 3):
            break
        lv += 1
    return lv


def model_zps(tiles, m3):
    best, best_cost = m3, float("inf")
    for segs in range(1, m3 + 1):
        zps = -(-m3 // segs)
        if zps < 4:
            break
        rounds = -(-tiles * -(-m3 // zps) // WG_PER_ROUND)
        cost = rounds * (zps + 4)
        if cost < best_cost:
            best, best_cost = zps, cost
    return best


def model_plan(shape, inverse):
    nx, ny, nz = shape
    lv = model_levels(nx, ny, nz, inverse)
    grid = []
    for l in range(lv):
        m1, m2, m3 = (nx >> l) // 2, (ny >> l) // 2, (nz >> l) // 2
        tx, ty = -(-m1 // (ITXP if inverse else TXP)), -(-m2 // (ITYP if inverse else TYP))
        zps = model_zps(tx * ty, m3)
        zsegs = -(-m3 // zps)
        grid.append((tx, ty, zps, zsegs, m3 - (zsegs - 1) * zps))
    return lv, lv >= 2 or (lv == 1 and nx * ny * nz >= 1 << 21), grid


# ---- shape families
X1_REMAINDERS = (3, 5, 31, 61, 63)
XI1_REMAINDERS = (2, 30, 62)
XCD_SHAPE = (264, 512, 16)
FAMILIES = {
    # forward: two fused levels of 2k and k x-pairs; inverse: the same when k is even, general kernels when k is odd
    "X": [(4 * k, 16, 16) for k in range(4, 129)],
    "Y": [(16, 4 * k, 16) for k in range(4, 41)],
    "Z": [(16, 16, 4 * k) for k in range(4, 41)],
    # forward only, one level, nx % 4 == 2: 64 + r x-pairs at level 0, rows 8-byte aligned only
    "X1": [(2 * (64 + r), 128, 128) for r in X1_REMAINDERS],
    # the inverse's counterpart: nx % 8 == 4, so the level-1 box has n1 % 4 == 2 and the inverse runs level 0 alone -- the only
    # way its level 0 (the level that narrows to fp32 in its stores) meets a box of 2 (mod 4) x-pairs.  Forward: two levels
    "XI1": [(2 * (64 + r), 128, 128) for r in XI1_REMAINDERS],
    # level 0: 132 x-pairs in 3 tile columns (the last 4 wide) x 16 tile rows; level 1: 66 in 2 (the last 2 wide) x 8
    "XCD": [XCD_SHAPE],
    # all four levels fused forward, min/max riding along (MM_IN, MM_OUT, k_minmax_final4)
    "MM": [(16 * j, 64, 64) for j in range(4, 10)] + [(64, 16 * j, 64) for j in range(5, 10)],
}
# (shape, swept axis) of the face-extreme fields: 64^3 belongs to both sweeps
MM_FIELDS = [((16 * j, 64, 64), "x") for j in range(4, 10)] + [((64, 16 * j, 64), "y") for j in range(4, 10)]
F32_FAMILIES = ("X", "X1", "XI1", "XCD", "MM")

TABLE = {}
for _shapes in FAMILIES.values():     # (16^3 opens X, Y and Z, 64^3 both sweeps of MM: one entry)
    for _s in _shapes:
        TABLE[_s] = dict(fwd=model_plan(_s, False), inv=model_plan(_s, True))
SHAPES = sorted(TABLE)


def check_plan(api, shape_xyz):
    """assert that dispatch gives `shape_xyz` the path and geometry it is in the table for, and that the tiles are the ones
    the remainders are counted in"""
    nx, ny, nz = shape_xyz
    for d in DIRS:
        got = api.fused_plan((nz, ny, nx), inverse=d == "inv")
        assert (got["levels"], got["used"], got["grid"]) == tuple(TABLE[shape_xyz][d]), (shape_xyz, d, got)
        txp, typ = (ITXP, ITYP) if d == "inv" else (TXP, TYP)
        for l, g in enumerate(got["grid"]):
            m1, m2 = (nx >> l) // 2, (ny >> l) // 2
            assert g[0] == -(-m1 // txp) and g[1] == -(-m2 // typ), (shape_xyz, d, l, g)


def classes(shape_xyz, plans=None):
    """the path classes `shape_xyz` reaches (module docstring), from its plans"""
    plans = TABLE[shape_xyz] if plans is None else plans
    nx, ny, nz = shape_xyz
    out = set()
    for d in DIRS:
        levels, used, grid = plans[d]
        if not used:
            continue
        txp, typ = (ITXP, ITYP) if d == "inv" else (TXP, TYP)
        for l, (tx, ty, zps, zsegs, zlast) in enumerate(grid):
            rx, ry = (nx >> l) // 2 - (tx - 1) * txp, (ny >> l) // 2 - (ty - 1) * typ
            out.add((d, "x", rx))
            out.add((d, "y", ry))
            out.add((d, "z", "one" if zsegs == 1 else min(zlast, 4)))
            if ty % 8 == 0 and rx < txp:
                out.add((d, "blocked_short"))
            if levels == 1:
                out.add((d, "x1", rx))
    return out


def reached(shapes=None):
    out = set()
    for s in SHAPES if shapes is None else shapes:
        out |= classes(s)
    return out


REQUIRED = (
    {("fwd", "x", r) for r in range(1, TXP + 1)}
    | {("inv", "x", r) for r in range(2, ITXP + 1, 2)}
    | {(d, "y", r) for d in DIRS for r in range(1, TYP + 1)}
    | {(d, "z", c) for d in DIRS for c in ("one", 1, 2, 3, 4)}
    | {("fwd", "x1", r) for r in X1_REMAINDERS}
    | {("inv", "x1", r) for r in XI1_REMAINDERS}
    | {(d, "blocked_short") for d in DIRS}
)


def ident(v):
    return "x".join(str(n) for n in v) if isinstance(v, tuple) else str(v)


def slices(family, per_item):
    """the family's shapes in runs of `per_item`, one GPU test item each"""
    s = FAMILIES[family]
    return [s[i:i + per_item] for i in range(0, len(s), per_item)]


def slice_id(shapes):
    return ident(shapes[0]) if len(shapes) == 1 else ident(shapes[0]) + ".." + ident(shapes[-1])


# ---- fields (read-only)
def field(shape_xyz):
    nx, ny, nz = shape_xyz
    f = synth.field(nx, ny, nz, seed=nx + 7 * ny + 49 * nz)
    f.setflags(write=False)
    return f


# The extremes lie this many field ranges outside the field.  3: the field's extremes (MM_IN) sit in the last, partial tiles,
# those of the coefficient array stay in the coarsest low-pass box (four levels give the smooth part a gain of 64 there).
# 100: the detail coefficients of the two spikes, in the last pair of their level-0 subbands, are the extremes of the
# coefficient array as well (MM_OUT); tests/test_fused_edge_cases_cpu.py asserts both.
FACE_FACTORS = (3.0, 100.0)


def face_positions(shape_xyz, axis):
    """(index of the global minimum, index of the global maximum) in the (nz, ny, nx) array: the minimum in the last x-pair,
    last y-pair and last z-pair; the maximum in the last pair of the swept axis at index 0 of the other two"""
    nx, ny, nz = shape_xyz
    return (nz - 1, ny - 1, nx - 1), {"x": (0, 0, nx - 1), "y": (0, ny - 1, 0)}[axis]


def face_field(shape_xyz, axis, factor, dtype=np.float64):
    """field() with its global extremes on the far faces, `factor` field ranges outside"""
    f = np.array(field(shape_xyz))
    lo, hi = float(f.min()), float(f.max())
    pmin, pmax = face_positions(shape_xyz, axis)
    f[pmin] = lo - factor * (hi - lo)
    f[pmax] = hi + factor * (hi - lo)
    f = np.ascontiguousarray(f.astype(dtype))
    f.setflags(write=False)
    return f
