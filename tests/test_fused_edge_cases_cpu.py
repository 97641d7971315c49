"""The last-tile remainder sweep of tests/fused_edge_cases.py without a GPU: every table entry against wr_fused_plan, the tile
sizes the remainders are counted in, REQUIRED against the classes the table reaches, and the face-extreme fields of family MM
(extremes where they are meant to be, defined and non-trivial in the oracle)."""
import numpy as np
import pytest

import fused_edge_cases as E
from util import ROOT  # noqa: F401  (puts the repository on sys.path)
from waverange_amd import api

TOL = 1e-6


@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_table_entries_are_what_dispatch_gives(family):
    assert E.FAMILIES[family]
    for shape in E.FAMILIES[family]:
        E.check_plan(api, shape)


def test_tile_sizes_are_the_ones_the_remainders_are_counted_in():
    """tiles_x == ceil(m1 / 64) and tiles_y == ceil(m2 / 16) at every fused level of every shape, either direction, with the
    module's constants (check_plan asserts the same in front of every GPU check)"""
    assert (E.TXP, E.TYP, E.ITXP, E.ITYP) == (64, 16, 64, 16)
    seen = 0
    for shape in E.SHAPES:
        nx, ny, nz = shape
        for d in E.DIRS:
            got = api.fused_plan((nz, ny, nx), inverse=d == "inv")
            for l, (tx, ty, zps, zsegs, zlast) in enumerate(got["grid"]):
                m1, m2, m3 = (nx >> l) // 2, (ny >> l) // 2, (nz >> l) // 2
                assert tx == -(-m1 // 64) and ty == -(-m2 // 16), (shape, d, l)
                assert zsegs == -(-m3 // zps) and 1 <= zlast <= zps and (zsegs - 1) * zps + zlast == m3, (shape, d, l)
                seen += 1
    assert seen > 2 * len(E.SHAPES)


def test_families_are_the_ones_the_sweep_was_specified_with():
    assert E.FAMILIES["X"] == [(4 * k, 16, 16) for k in range(4, 129)]
    assert set((16, 4 * k, 16) for k in range(4, 41)) <= set(E.FAMILIES["Y"])
    assert set((16, 16, 4 * k) for k in range(4, 41)) <= set(E.FAMILIES["Z"])
    assert E.FAMILIES["X1"] == [(134, 128, 128), (138, 128, 128), (190, 128, 128), (250, 128, 128), (254, 128, 128)]
    assert all(nx % 4 == 2 and nx * ny * nz >= 1 << 21 for nx, ny, nz in E.FAMILIES["X1"])
    assert E.FAMILIES["XI1"] == [(132, 128, 128), (188, 128, 128), (252, 128, 128)]
    assert all(nx % 8 == 4 and nx * ny * nz >= 1 << 21 for nx, ny, nz in E.FAMILIES["XI1"])
    assert E.FAMILIES["XCD"] == [(264, 512, 16)]
    mm = set(E.FAMILIES["MM"])
    assert mm == {(16 * j, 64, 64) for j in range(4, 10)} | {(64, 16 * j, 64) for j in range(4, 10)} and len(E.FAMILIES["MM"]) == 11
    assert len(E.MM_FIELDS) == 12 and {s for s, _ in E.MM_FIELDS} == mm
    assert max(nx * ny * nz * 8 for nx, ny, nz in E.SHAPES) < 34 << 20
    assert max(nx * ny * nz * 8 for f in ("X", "Y", "Z") for nx, ny, nz in E.FAMILIES[f]) <= 1 << 20


def test_named_entries():
    """the entries the sweep was specified by, spelled out"""
    T = E.TABLE
    # X: two fused levels forward; inverse the same for even k, general kernels for odd k
    assert T[(28, 16, 16)]["fwd"] == (2, True, [(1, 1, 4, 2, 4), (1, 1, 4, 1, 4)]) and T[(28, 16, 16)]["inv"] == (1, False, [(1, 1, 4, 2, 4)])
    assert T[(24, 16, 16)]["inv"] == T[(24, 16, 16)]["fwd"] == (2, True, [(1, 1, 4, 2, 4), (1, 1, 4, 1, 4)])
    for shape in E.FAMILIES["X"]:
        k = shape[0] // 4
        assert T[shape]["fwd"][:2] == (2, True) and T[shape]["inv"][:2] == ((2, True) if k % 2 == 0 else (1, False)), shape
        assert [g[0] for g in T[shape]["fwd"][2]] == [-(-2 * k // 64), -(-k // 64)]
    # Z: one tile; pick_zps by hand for 9, 10, 11 and 13 z-pairs
    for m3, zlast in ((9, 4), (10, 2), (11, 3), (13, 1)):
        for d in E.DIRS:
            g = T[(16, 16, 4 * m3)][d][2][1]
            assert g[:2] == (1, 1) and g[3] >= 2 and g[4] == zlast, (m3, d, g)
    # X1: one level forward, the second tile column r pairs wide; inverse general
    for r, shape in zip(E.X1_REMAINDERS, E.FAMILIES["X1"]):
        levels, used, grid = T[shape]["fwd"]
        assert (levels, used) == (1, True) and grid[0][:2] == (2, 4) and T[shape]["inv"] == (0, False, [])
        assert ("fwd", "x1", r) in E.classes(shape) and ("fwd", "x", r) in E.classes(shape)
    # XI1: the inverse runs level 0 alone on 64 + r x-pairs, r = 2 (mod 4); no other shape gives its level 0 such a box
    for r, shape in zip(E.XI1_REMAINDERS, E.FAMILIES["XI1"]):
        levels, used, grid = T[shape]["inv"]
        assert (levels, used) == (1, True) and grid[0][:2] == (2, 4) and r % 4 == 2 and T[shape]["fwd"][:2] == (2, True)
        assert ("inv", "x1", r) in E.classes(shape)
    for shape in E.SHAPES:
        if shape not in E.FAMILIES["XI1"] and T[shape]["inv"][1]:
            assert (shape[0] // 2) % 4 == 0, shape
    # XCD: both levels in the blocked tile order (tiles_y % 8 == 0), last columns 4 and 2 pairs wide
    for d in E.DIRS:
        levels, used, grid = T[E.XCD_SHAPE][d]
        assert (levels, used) == (2, True) and [g[:2] for g in grid] == [(3, 16), (2, 8)]
        assert {(d, "x", 4), (d, "x", 2), (d, "blocked_short")} <= E.classes(E.XCD_SHAPE)
    # MM: all four levels fused forward (the condition for min/max to ride along)
    for shape in E.FAMILIES["MM"]:
        assert T[shape]["fwd"][:2] == (4, True), shape


def test_required_classes_are_reached():
    got = E.reached()
    missing = sorted(E.REQUIRED - got, key=repr)
    assert not missing, missing
    # REQUIRED is the condition it was specified as
    assert len(E.REQUIRED) == 64 + 32 + 2 * 16 + 2 * 5 + 5 + 3 + 2
    # each family reaches its own part without the others
    x = E.reached(E.FAMILIES["X"])
    assert {c for c in E.REQUIRED if c[1] == "x"} <= x
    assert {c for c in E.REQUIRED if c[1] == "y"} <= E.reached(E.FAMILIES["Y"])
    assert {c for c in E.REQUIRED if c[1] == "z"} <= E.reached(E.FAMILIES["Z"])
    assert {c for c in E.REQUIRED if c[1] == "x1"} <= E.reached(E.FAMILIES["X1"] + E.FAMILIES["XI1"])
    assert {c for c in E.REQUIRED if c[1] == "blocked_short"} <= E.reached(E.FAMILIES["XCD"])
    # a class of a level that does not run fused is not counted: X with odd k reaches nothing in the inverse
    assert not {c for c in E.classes((28, 16, 16)) if c[0] == "inv"}
    # odd x remainders in the inverse cannot exist (n1 % 4 == 0)
    assert not {c for c in got if c[0] == "inv" and c[1] == "x" and c[2] % 2}
    # the MM sweeps end in partial tiles on every level, not only on whole ones
    for axis, fam in (("x", [s for s, a in E.MM_FIELDS if a == "x"]), ("y", [s for s, a in E.MM_FIELDS if a == "y"])):
        rem = {c[2] for c in E.reached(fam) if c[0] == "fwd" and c[1] == axis}
        assert len(rem) >= 10 and min(rem) <= 5, (axis, sorted(rem))


def where(a, pick):
    return tuple(int(v) for v in np.unravel_index(pick(a), a.shape))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("factor", E.FACE_FACTORS)
@pytest.mark.parametrize("case", E.MM_FIELDS, ids=lambda c: E.ident(c[0]) + "-" + c[1])
def test_face_extreme_fields(oracle, case, factor, dtype):
    shape, axis = case
    nx, ny, nz = shape
    base = E.field(shape)
    f = E.face_field(shape, axis, factor, dtype)
    assert f.dtype == dtype and f.shape == (nz, ny, nx) and np.isfinite(f).all() and not f.flags.writeable
    pmin, pmax = E.face_positions(shape, axis)
    assert where(f, np.argmin) == pmin == (nz - 1, ny - 1, nx - 1)
    assert where(f, np.argmax) == pmax == {"x": (0, 0, nx - 1), "y": (0, ny - 1, 0)}[axis]
    # unique, and `factor` field ranges outside the field
    span = float(base.max() - base.min())
    rest = np.array(f, dtype=np.float64)
    rest[pmin] = rest[pmax] = base[0, 0, 0]
    assert rest.min() - float(f[pmin]) > 0.99 * factor * span and float(f[pmax]) - rest.max() > 0.99 * factor * span
    wide = f.astype(np.float64)
    assert oracle.minmax(wide) == (float(f[pmin]), float(f[pmax]))
    # the extremes of the coefficient array: with the larger factor the spikes' own detail coefficients, the last of their
    # level-0 subbands (the samples are the odd halves of the last pairs); with the smaller one still in the low-pass box
    coef = oracle.cdf97_3d(wide, 4)
    if factor == max(E.FACE_FACTORS):
        assert where(coef, np.argmin) == pmin and where(coef, np.argmax) == pmax
    else:
        assert all(i < n // 16 for pos in (where(coef, np.argmin), where(coef, np.argmax)) for i, n in zip(pos, (nz, ny, nx)))
    # defined and non-trivial in the oracle
    want = oracle.encode(wide, TOL)
    assert want["nlay"] >= 1 and want["ntot_enc"] > 0
    assert all(np.isfinite(want[k]) for k in ("tolabs", "midval", "halfspanval"))
    assert np.isfinite(want["deps_vec"]).all() and np.isfinite(want["minval_vec"]).all()
    assert np.isfinite(oracle.decode(want, wide.shape)).all()
