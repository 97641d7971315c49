"""Planes that pin which paths of the reorder kernel run (k_plane_reorder in csrc/wr_blocked.hip, its dispatch in plane_reorder
and wr_reorder_plan).  A plain module, like roi_cases.py: tests/test_blocked_cases_cpu.py asserts the table through
wr_reorder_plan and checks the geometry below against wr_blocked_order without a GPU, tests/test_gpu_blocked_cases.py asserts each
plan again in front of every GPU check, so that a change of the wide/byte rule or of the grouping fails loudly and cannot turn a
case into a test of another path.

Shapes are (nz, ny, nx); origins, extents and brick coordinates are (x, y, z), as in the plan.

The geometry is written here from the format text of include/waverange_amd.h ("Blocked symbol order") and reads nothing from the
plan: boxes_of, bricks_of.  What a work item is a case of comes from that geometry plus the plan's `group` and the `wide` flag of
its box: item_classes."""
from collections import namedtuple

AXES = "xyz"
THREADS = 256  # lanes of a workgroup: one work item


def h(n):
    return (n + 1) // 2


# ---- the format, restated
def boxes_of(shape, wlev):
    """[(origin, extent)] in stream order: the low-pass box [0, e_wlev)^3, then for l = wlev .. 1 the octants o = 1 .. 7 (bit 0 /
    1 / 2 of o: x / y / z takes the high part [e_l, e_{l-1}) of level l), without the boxes that are empty on an axis"""
    nz, ny, nx = shape
    e = [(nx, ny, nz)]
    for _ in range(wlev):
        e.append(tuple(h(n) for n in e[-1]))
    out = [((0, 0, 0), e[wlev])]
    for l in range(wlev, 0, -1):
        for oct in range(1, 8):
            o = tuple(e[l][k] if oct >> k & 1 else 0 for k in range(3))
            x = tuple(e[l - 1][k] - e[l][k] if oct >> k & 1 else e[l][k] for k in range(3))
            if min(x) > 0:
                out.append((o, x))
    return out


Brick = namedtuple("Brick", "id box t origin h start")  # t: (tx, ty, tz) in its box; origin: in the field; h: (hx, hy, hz)


def bricks_of(shape, wlev, B):
    """Every brick in stream order: the boxes one after the other, inside a box (tz, ty, tx) with tx fastest, a partial brick
    at a high edge holding exactly its hx*hy*hz symbols -- so a brick's stream range [start, start + hx*hy*hz) begins where the
    brick before it ends"""
    out, start = [], 0
    for i, (o, e) in enumerate(boxes_of(shape, wlev)):
        nt = [-(-v // B) for v in e]
        for tz in range(nt[2]):
            for ty in range(nt[1]):
                for tx in range(nt[0]):
                    t = (tx, ty, tz)
                    hh = tuple(min(B, e[k] - t[k] * B) for k in range(3))
                    out.append(Brick(len(out), i, t, tuple(o[k] + t[k] * B for k in range(3)), hh, start))
                    start += hh[0] * hh[1] * hh[2]
    assert start == shape[0] * shape[1] * shape[2]
    return out


def brick_points(shape, brick):
    """the coefficient index x + nx * (y + ny * z) of every point of a brick, in stream order (x fastest, then y, then z)"""
    import numpy as np
    nz, ny, nx = shape
    (ox, oy, oz), (hx, hy, hz) = brick.origin, brick.h
    z, y, x = np.meshgrid(oz + np.arange(hz), oy + np.arange(hy), ox + np.arange(hx), indexing="ij")
    return (x + nx * (y + ny * z)).ravel().astype(np.int64)


# ---- what a work item is a case of
# mode: whole / list; path: wide / byte; xcase: full (W == group*B), short (W < group*B, W % B == 0), partial1 (W < B), partialN
# (W > B, W % B != 0), W the bytes of the item's row; gx: the item is not the first of its row of bricks
ItemClass = namedtuple("ItemClass", "mode B path xcase gx hy_short hz_short yloop zloop zbreak whole_brick")


def row_geometry(group, B, wide):
    """(yb, zstep) of move_rows: 2^cs lanes cover a row of the item (16 bytes each on the wide path), THREADS >> cs rows go in one
    step: yb consecutive y (at most B), then the next z"""
    cs = (group * B).bit_length() - 1 - (4 if wide else 0)
    rows = THREADS >> cs
    yb = min(B, rows)
    return yb, rows // yb


def item_classes(shape, wlev, B, plan, mode):
    """{ItemClass: an example (box, tz, ty, gx)} over every work item of a launch: a group of plan["group"] bricks along x in
    whole mode, one brick in list mode (the upper bound of a list: every brick)"""
    group = plan["group"]
    assert group == (1 if mode == "list" else 128 // B)
    out = {}
    for i, (o, e) in enumerate(boxes_of(shape, wlev)):
        wide = plan["boxes"][i]["wide"]
        yb, zstep = row_geometry(group, B, wide)
        nt = [-(-v // B) for v in e]
        for tz in range(nt[2]):
            hz = min(B, e[2] - tz * B)
            for ty in range(nt[1]):
                hy = min(B, e[1] - ty * B)
                for gx in range(-(-nt[0] // group)):
                    W = min(group * B, e[0] - gx * group * B)
                    xcase = "full" if W == group * B else "short" if W % B == 0 else "partial1" if W < B else "partialN"
                    cls = ItemClass(mode, B, "wide" if wide else "byte", xcase, gx > 0, hy < B, hz < B, hy > yb, hz > 4 * zstep,
                                    hz % (4 * zstep) != 0, xcase == "full" and hy == B and hz == B)
                    out.setdefault(cls, (i, tz, ty, gx))
    return out


def features(cls):
    """The names under which REQUIRED lists what the table must reach: "mode/B/path/property"."""
    at = "%s/B%d/%s/" % (cls.mode, cls.B, cls.path)
    out = {at + cls.xcase}
    for name in ("gx", "hy_short", "hz_short", "yloop", "zloop", "zbreak", "whole_brick"):
        if getattr(cls, name):
            out.add(at + {"gx": "gx>0", "hy_short": "hy<B", "hz_short": "hz<B"}.get(name, name))
    return out


def reached(shape, wlev, B, plans):
    """the features of a case; plans = {"whole": plan, "list": plan}"""
    out = set()
    for mode, plan in plans.items():
        for cls in item_classes(shape, wlev, B, plan, mode):
            out |= features(cls)
    return out


# ---- the table: (shape, wlev, brick) -> why it is there, and what wr_reorder_plan says of it: bricks per work item of a whole
# launch, its work items, and the `wide` flag of every box ("w" / "b") in stream order
CASES = {
    # level extents in x 288, 144, 72, 36: the two finest levels wide, rows of 128 + 128 + 32 and 128 + 16 bytes (full groups,
    # gx > 0, a short last group at brick 16, a partial last brick at brick 32), the coarse ones byte by byte off multiples of
    # 16; y and z so short that every brick is partial in both (hy = 12, 6, ..., hz = 4, 2, 1)
    ((8, 24, 576), 4, 16): dict(why="brick 16: full groups, gx > 0, short groups, short y and z", group=8, items=46, wide="bbbbbbbbbbbwwwwwwwwwwwwww"),
    ((8, 24, 576), 4, 32): dict(why="brick 32: full groups, gx > 0, one partial brick, by list 2 lanes per row", group=4, items=46, wide="bbbbbbbbbbbwwwwwwwwwwwwww"),
    # x extent 48 at level 1: bricks of 32 + 16 in one group on the wide path; z extent 20 (by list more than 4 * zstep = 16
    # rows of z), y extent 36 = 32 + 4; levels 2 .. 4 byte by byte with rows of 24, 12 and 6
    ((40, 72, 96), 4, 32): dict(why="brick 32: a group of 32 + 16 wide, the z loop's second turn by list", group=4, items=36, wide="bbbbbbbbbbbbbbbbbbbbbbwwwwwww"),
    # one box, 272 = 128 + 128 + 16: whole bricks of 32^3 in full groups, a group that is one partial brick, 40 = 32 + 8, 48 = 32 + 16
    ((48, 40, 272), 0, 32): dict(why="brick 32: whole bricks in full groups, a last group of 16 bytes", group=4, items=12, wide="w"),
    # one box, 160 = 128 + 32: a full group of two bricks and a partial brick; hy = 40 > 32 rows of y per step, hz = 64 and 8
    ((72, 40, 160), 0, 64): dict(why="brick 64: the y loop's second step, full group, gx > 0, partial brick", group=2, items=4, wide="w"),
    # x extent 80 = 64 + 16 at level 1
    ((72, 40, 160), 4, 64): dict(why="brick 64: a group of 64 + 16 wide", group=2, items=29, wide="bbbbbbbbbbbbbbbbbbbbbbwwwwwww"),
    # x extents 192 = 128 + 64 (a short group of one whole-width brick), 96 = 64 + 32, 48 (still wide at origin 48); z extent 18:
    # the batches of four z break off inside (18 % 4 != 0)
    ((36, 40, 384), 4, 64): dict(why="brick 64: a short group, z batches that break off", group=2, items=36, wide="bbbbbbbbwwwwwwwwwwwwwwwwwwwww"),
    # one box, 160 = 128 + 32: whole bricks of 16^3 in full groups of 8, a short group of 2; hz = 16 > 8 rows of z per batch
    ((24, 40, 160), 0, 16): dict(why="brick 16: whole bricks in full groups, the z loop's second turn", group=8, items=12, wide="w"),
    ((64, 64, 128), 0, 64): dict(why="brick 64: two whole bricks, one full group", group=2, items=1, wide="w"),
    # the byte path of test_gpu_blocked.py's REORDER at planes of a tenth the size: odd extents 133, 67 / 66, 34 / 33, 17 in x
    ((21, 19, 266), 4, 8): dict(why="brick 8, byte path: 128 + 5, rows of 67, 66, 34, 33, 17, every partial brick", group=16, items=78, wide="bbbbbbbbbbbbbbbbbbbbbbbbbbbbb"),
    ((5, 11, 152), 0, 8): dict(why="brick 8, byte path: a short group of 24 bytes", group=16, items=4, wide="b"),
    ((37, 45, 203), 0, 32): dict(why="brick 32, byte path: whole bricks in a full group at an odd nx, 128 + 75", group=4, items=8, wide="b"),
}


def wide_flags(plan):
    return "".join("bw"[b["wide"]] for b in plan["boxes"])


def check_plan(api, key):
    """assert that the library gives the case the plans it is in the table for; returns {"whole": plan, "list": plan}"""
    shape, wlev, B = key
    want = CASES[key]
    whole, lst = api.reorder_plan(shape, wlev, B), api.reorder_plan(shape, wlev, B, list=True)
    assert (whole["group"], whole["items"], wide_flags(whole)) == (want["group"], want["items"], want["wide"]), (key, whole["group"], whole["items"], wide_flags(whole))
    assert lst["group"] == 1 and lst["items"] == lst["nbricks"] == whole["nbricks"] and wide_flags(lst) == want["wide"], key
    return {"whole": whole, "list": lst}


def both_widths_in_one_launch(plan):
    """wide boxes and byte boxes in one launch, and a box that starts off a multiple of 16 next to one that starts on one.  Asked
    of every case with the transform and a brick that can go wide; a plane without the transform is one box at start 0."""
    b = plan["boxes"]
    return {x["wide"] for x in b} == {True, False} and any((p["start"] % 16 == 0) != (q["start"] % 16 == 0) for p, q in zip(b, b[1:]))


# ---- the brick lists of a case
def brick_lists(shape, wlev, B):
    """{name: ascending brick ids}: every brick, every second one, the first and last brick of every box, one brick"""
    bricks = bricks_of(shape, wlev, B)
    ends = sorted({f(b.id for b in bricks if b.box == i) for i in {b.box for b in bricks} for f in (min, max)})
    return {"all": [b.id for b in bricks], "every-second": [b.id for b in bricks][::2], "box-ends": ends, "one": [bricks[len(bricks) // 2].id]}


# ---- what the table must reach
def _wide(mode, B, names):
    return {"%s/B%d/wide/%s" % (mode, B, n) for n in names}


def _byte(mode, B, names):
    return {"%s/B%d/byte/%s" % (mode, B, n) for n in names}


WIDE_BOTH = ("full", "whole_brick", "partial1", "gx>0", "hy<B", "hz<B", "zloop", "zbreak")
REQUIRED = set()
for _B in (16, 32, 64):
    REQUIRED |= _wide("whole", _B, WIDE_BOTH + ("short",)) | _wide("list", _B, WIDE_BOTH)
REQUIRED |= _wide("whole", 32, ("partialN",)) | _wide("whole", 64, ("partialN", "yloop"))
# What no plane can reach.  A list item at B = 16 on the wide path is one lane per row and 16 rows of z per step (zstep = 16): a
# batch of four holds 64 z and a brick has at most 16, so the z loop never takes a second turn there.  A wide box has an x
# extent that is a multiple of 16, so at B = 16 it has no partial brick in x.
REQUIRED -= {"list/B16/wide/zloop", "list/B16/wide/partial1", "whole/B16/wide/partial1"}
# The byte path: what the planes of test_gpu_blocked.py's REORDER reach at brick 8 and at brick 32 in whole mode
# (tests/test_blocked_cases_cpu.py classifies that list and compares), and the same by list, where an item is one brick (its row
# is full or one partial brick) and the z loop has one turn at B = 8 (8 rows of y, 4 of z per step), the y loop none.
BYTE_WHOLE_8 = ("full", "short", "partial1", "partialN", "gx>0", "hy<B", "hz<B", "yloop", "zloop", "zbreak", "whole_brick")
BYTE_WHOLE_32 = tuple(n for n in BYTE_WHOLE_8 if n != "short")  # (a row of whole bricks of 32 has an x extent that is a multiple of 16)
BYTE_LIST_8 = ("full", "partial1", "gx>0", "hy<B", "hz<B", "zbreak", "whole_brick")
BYTE_LIST_32 = ("full", "partial1", "gx>0", "hy<B", "hz<B", "yloop", "zloop", "zbreak", "whole_brick")
REQUIRED |= _byte("whole", 8, BYTE_WHOLE_8) | _byte("whole", 32, BYTE_WHOLE_32) | _byte("list", 8, BYTE_LIST_8) | _byte("list", 32, BYTE_LIST_32)
