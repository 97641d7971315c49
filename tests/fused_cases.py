"""Shapes that pin the launch geometries of the fused transform kernels (csrc/wr_fused.hip) which the cubes and near-cubes
of the other GPU tests do not reach, and fp64 edge-value fields.  A plain module: tests/test_fused_plan_cpu.py asserts the
table through wr_fused_plan without a GPU, tests/test_gpu_fused_paths.py asserts it again in front of every GPU check, so
that a change of the dispatch rule or of a tile size fails loudly and cannot turn these into tests of another kernel.

Every entry: (nx, ny, nz) -> dict(fwd=PLAN, inv=PLAN, why=...), PLAN = (levels, used, grid), as api.fused_plan gives it:
`levels` finest levels can run fused, `used` says whether a four-level transform takes the fused path at all, `grid` has
one (tiles_x, tiles_y, zps, zsegs, zlast) per fused level: tiles of 64 x 16 sample PAIRS (128 x 32 samples), each tile
column cut along z into `zsegs` segments of `zps` z-pairs, the last one `zlast` long."""
import numpy as np

from waverange_amd import synth

NOT_FUSED = (0, False, [])


def _both(plan):
    return dict(fwd=plan, inv=plan)


CASES = {
    # ---- exactly one fused level (fused_ok: f == 1 and n >= 2^21): level 0 writes its low-pass octant straight into the
    # coefficient array, the general kernels run levels 1..3 on it
    (512, 512, 8): dict(_both((1, True, [(4, 16, 4, 1, 4)])),
                        why="slab: one level both ways, a single z segment of 4 pairs, 4 x 16 tiles"),
    (8, 512, 512): dict(_both((1, True, [(1, 16, 16, 16, 16)])),
                        why="8 wide in x (one tile of 4 x-pairs), zps = 16 in 16 segments"),
    (512, 8, 512): dict(_both((1, True, [(4, 1, 4, 64, 4)])),
                        why="8 wide in y (one tile row of 4 y-pairs), 64 z segments"),
    (8, 512, 520): dict(_both((1, True, [(1, 16, 17, 16, 5)])),
                        why="zps = 17, the last of 16 segments 5 long"),
    (258, 130, 66): dict(fwd=(1, True, [(3, 5, 4, 9, 1)]), inv=NOT_FUSED,
                         why="forward: 1-pair remainder tiles in x and y, last z segment 1; inverse general (nx % 4 == 2)"),
    (130, 128, 128): dict(fwd=(1, True, [(2, 4, 4, 16, 4)]), inv=NOT_FUSED,
                          why="forward one level with a second x tile 1 pair wide; inverse general"),
    (128, 128, 126): dict(_both((1, False, [(1, 4, 4, 16, 3)])),
                          why="f == 1 just below 2^21 samples: general both ways"),
    (128, 128, 130): dict(_both((1, True, [(1, 4, 4, 17, 1)])),
                          why="f == 1 just above 2^21 samples: fused both ways, last z segment 1"),
    (180, 190, 200): dict(_both((1, True, [(2, 6, 5, 20, 5)])),
                          why="the one-level shape of the older tests, here for fp32 and the transform-level checks"),
    # ---- pencils: two fused levels, many tiles in one direction, level-1 boxes 8 wide in the other two
    (4112, 16, 16): dict(_both((2, True, [(33, 1, 4, 2, 4), (17, 1, 4, 1, 4)])), why="33 x tiles"),
    (16, 4112, 16): dict(_both((2, True, [(1, 129, 8, 1, 8), (1, 65, 4, 1, 4)])), why="129 y tiles"),
    (16, 16, 4112): dict(_both((2, True, [(1, 1, 9, 229, 4), (1, 1, 5, 206, 3)])), why="229 and 206 z segments"),
    # ---- the smallest boxes that take the fused path (f == 2)
    (16, 16, 16): dict(_both((2, True, [(1, 1, 4, 2, 4), (1, 1, 4, 1, 4)])), why="smallest fused box"),
    (24, 24, 24): dict(_both((2, True, [(1, 1, 4, 3, 4), (1, 1, 6, 1, 6)])), why="level-1 box 12^3: one segment of 6"),
}
SHAPES = sorted(CASES)
# the shapes on which the fused path runs exactly one level in at least one direction
ONE_LEVEL = [s for s in SHAPES if any(CASES[s][d][:2] == (1, True) for d in ("fwd", "inv"))]


def check_plan(api, shape_xyz, want=None):
    """assert that dispatch gives `shape_xyz` the path and geometry it is in the table for"""
    want = CASES[shape_xyz] if want is None else want
    nx, ny, nz = shape_xyz
    for d in ("fwd", "inv"):
        got = api.fused_plan((nz, ny, nx), inverse=d == "inv")
        assert (got["levels"], got["used"], got["grid"]) == tuple(want[d]), (shape_xyz, d, got)


def ident(v):
    return "x".join(str(n) for n in v) if isinstance(v, tuple) else str(v)


# ---- fp64 edge-value fields.  The arithmetic contract (strict IEEE, bit-identical to the reference) includes subnormals and
# the reference's triviality rule halfspanval <= 2 * DBL_MIN.  Each shape takes another route through min/max and transform.
EDGE_SHAPES = {
    (64, 64, 64): dict(_both((4, True, [(1, 2, 4, 8, 4), (1, 1, 4, 4, 4), (1, 1, 4, 2, 4), (1, 1, 4, 1, 4)])),
                       why="all levels fused, min/max riding along"),
    (200, 120, 72): dict(fwd=(3, True, [(2, 4, 4, 9, 4), (1, 2, 4, 5, 2), (1, 1, 5, 2, 4)]),
                         inv=(2, True, [(2, 4, 4, 9, 4), (1, 2, 4, 5, 2)]), why="partly fused, stand-alone min/max"),
    (37, 21, 13): dict(_both(NOT_FUSED), why="general kernels"),
    (512, 512, 8): CASES[(512, 512, 8)],
}
EDGE_TOL = 1e-6
TINY = float(np.finfo(np.float64).tiny)  # DBL_MIN
# A field belongs only if the reference's behaviour on it is defined: tests/test_edge_fields_cpu.py runs every one of them
# through the oracle and, where it is built, the compiled reference, and requires identical and finite outputs.
# (f * 1e307 is not a case: hi - lo overflows in the reference itself.)
# `above` and `x10` code 8 planes because their residuals cannot shrink: from the plane on whose deps lies below 2^-1024
# (`above`: the first) 1 / deps is infinite, and the reference's x86-64 builds and the oracle turn every sample of such a plane
# into the byte 0 (DESIGN.md "Arithmetic").  What these two pin is min/max, the transform and the header arithmetic on
# subnormals, and that byte.
EDGE_FIELDS = ["below", "above", "x10", "scaled_1e300", "offset_1e12", "negative"]
SUBNORMAL_FIELDS = ("below", "above", "x10")
_cache = {}


def edge_field(shape_xyz, name):
    """read-only; built once per (shape, name)"""
    key = (shape_xyz, name)
    if key not in _cache:
        nx, ny, nz = shape_xyz
        f = synth.field(nx, ny, nz, seed=nx + 7 * ny + 49 * nz)
        span = float(f.max() - f.min())
        if name == "below":      # halfspan 1.95 DBL_MIN: trivial by the reference's rule
            g = f * (3.9 * TINY / span)
        elif name == "above":    # halfspan 2.25 DBL_MIN: the smallest field that is coded
            g = f * (4.5 * TINY / span)
        elif name == "x10":
            g = f * (40.0 * TINY / span)
        elif name == "scaled_1e300":
            g = f * 1e300
        elif name == "offset_1e12":
            g = f * 1e-3 + 1e12
        elif name == "negative":
            g = -np.abs(f) - 1.0
        else:
            raise KeyError(name)
        g = np.ascontiguousarray(g, dtype=np.float64)
        g.setflags(write=False)
        _cache.clear()           # one field at a time: the largest is 16 MB
        _cache[key] = g
    return _cache[key]


def check_edge_input(f, name):
    """the field is what its name says (a host environment that flushes subnormals fails here instead of passing vacuously)"""
    assert np.isfinite(f).all()
    span = float(f.max()) - float(f.min())
    if name in SUBNORMAL_FIELDS:
        share = np.count_nonzero((f != 0) & (np.abs(f) < TINY)) / f.size
        assert share >= 0.4, (name, share)
        factor = {"below": 3.9, "above": 4.5, "x10": 40.0}[name]
        assert abs(span / TINY - factor) < 0.01, (name, span / TINY)
    elif name == "scaled_1e300":
        assert 1e300 < np.abs(f).max() < 1e302
    elif name == "offset_1e12":
        assert f.min() > 0.9e12 and 0 < span < 1.0
    elif name == "negative":
        assert f.max() <= -1.0
