"""The case table of the masked region decode across a batch of fields (include/waverange_amd.h), shared by
test_masked_roi_batch_cases_cpu.py, test_gpu_mask_restore_boxes.py and test_gpu_masked_roi_batch.py.  Shapes, undefined sets and
the single-region helpers are those of masked_roi_cases.py.

A case is (field shape (nx, ny, nz), level, regions, mask segment length, fields).  A region is ((z0, z1), (y0, y1), (x0, x1)) in
the box of the level; the segment length counts mask SYMBOLS of 8 bits (0: the default).  `fields` has one letter per field:
  R  masked, the recipe's undefined set (a coherent 30 % and three lone samples)
  I  masked, isolated bits only
  A  masked, every sample of the case's FIRST region undefined (and every 97th of the field)
  -  no mask

The kernel's walk, which this file simulates (csrc/wr_mask.hip, k_mask_restore_boxes).  An item is a pair (field that has a
mask, region) in the order of the fields, then the regions; a turn is 64 consecutive x of one region row; region i has
ceil(cx / 64) * cy * cz turns and first[] is their exclusive prefix, tpf = first[nroi] the turns of a field.  Item (m, i) -- m
counts the masked fields -- owns the launch's turns m * tpf + first[i] .. m * tpf + first[i + 1] - 1.  The launch has
min(ceil(turns / 4), 2048) blocks of 4 waves; wave w takes the turns w, w + W, ..., W the waves of the grid.  classes_of() works
from this geometry and the undefined sets alone."""
import numpy as np

import masked_roi_cases as mc

WAVES_PER_BLOCK, MAX_BLOCKS = 4, 2048  # WR_MASK_WAVES, WR_MASK_BLOCKS


def single(case, i):
    """region i of a case as a case of masked_roi_cases.py"""
    shape, level, rois, seg, _ = case
    return (shape, level, rois[i], seg)


def masked_fields(case):
    return [f for f, k in enumerate(case[4]) if k != "-"]


def und_of(case, f):
    """the boolean undefined set (nz, ny, nx) of field f, None for a field without a mask"""
    kind = case[4][f]
    if kind == "-":
        return None
    return {"R": mc.und_recipe, "I": mc.und_isolated}[kind](case[0]) if kind in "RI" else mc.und_region(single(case, 0))


def region_turns(case, i):
    cz, cy, cx = mc.out_shape(single(case, i))
    return -(-cx // 64) * cy * cz


def first_of(case):
    """first[0 .. nroi] of one field's regions"""
    return np.concatenate([[0], np.cumsum([region_turns(case, i) for i in range(len(case[2]))])]).astype(np.int64)


def grid_waves(turns):
    return WAVES_PER_BLOCK * min(-(-turns // WAVES_PER_BLOCK), MAX_BLOCKS)


def walk(case):
    """every turn of the launch as (m, i, row, turn in the row), in the order of the launch's turn numbers"""
    first = first_of(case)
    out = []
    for m in range(len(masked_fields(case))):
        for i in range(len(case[2])):
            cz, cy, cx = mc.out_shape(single(case, i))
            tpr = -(-cx // 64)
            out += [(m, i, q // tpr, q % tpr) for q in range(int(first[i + 1] - first[i]))]
    return out


def offsets(case):
    """offs[0 .. nroi]: where a field's regions lie in its part of the output"""
    return np.concatenate([[0], np.cumsum([int(np.prod(mc.out_shape(single(case, i)))) for i in range(len(case[2]))])]).astype(np.int64)


def brute_segments_multi(case):
    return np.unique(np.concatenate([mc.brute_segments(single(case, i)) for i in range(len(case[2]))])).astype(np.uint32)


def classes_of(case):
    shape, level, rois, seg, fields = case
    got = set()
    first = first_of(case)
    tpf, nm = int(first[-1]), len(masked_fields(case))
    turns = nm * tpf
    W = grid_waves(turns)
    for i in range(len(rois)):
        one = mc.classes_of(single(case, i))
        got |= {c for c in one if c.startswith(("word", "strided", "row of several", "turn ends on the ragged"))}
        if rois[i] == whole(shape, level):
            got.add("whole box r=%d" % level)
        if region_turns(case, i) == 1 and "one sample" in one:
            got.add("an item of one turn, the one-sample probe")
    # where a block's four waves, at their first step, cover a boundary between two items
    for m in range(nm):
        for i in range(len(rois)):
            at = m * tpf + int(first[i])
            if at % WAVES_PER_BLOCK and at < turns:
                got.add("a block straddles two items of one field" if i else "a block straddles two items of different fields")
    # a wave's consecutive turns t, t + W
    items = [(m, i) for m, i, _, _ in walk(case)] if turns > W else []
    for t in range(max(turns - W, 0)):
        a, b = items[t], items[t + W]
        if a[0] == b[0] and a[1] != b[1]:
            got.add("a wave's next turn lies in another item of the field")
        if a[0] != b[0]:
            got.add("a wave's next turn lies in another field")
        if a[0] != b[0] and a[1] == b[1]:
            got.add("a wave's next turn lies in the same region of another field")  # (the region at hand is kept: no search)
        if a == b:  # (not in REQUIRED: it takes an item of more than 8192 turns, which no shape of the table has)
            got.add("a wave's next turn lies in the same item")
    if "-" in fields[1:-1] and fields[0] != "-" and fields[-1] != "-":
        got.add("an unmasked field between two masked ones")
    if fields[0] != "-" and fields[-1] != "-":
        got.add("masked first and last field")
    if fields[0] == "-" or fields[-1] == "-":
        got.add("unmasked first or last field")
    for f in masked_fields(case):
        for i in range(len(rois)):
            coarse = mc.coarse_und(und_of(case, f), single(case, i))
            if coarse.all():
                got.add("an all-undefined region")
            if not coarse.any():
                got.add("a region without an undefined sample")
    boxes = [mc.region_of(single(case, i)) for i in range(len(rois))]
    for i in range(len(rois)):
        for j in range(i):
            if boxes[i] == boxes[j]:
                got.add("a repeated region")
            elif all(max(boxes[i][2 * a], boxes[j][2 * a]) < min(boxes[i][2 * a + 1], boxes[j][2 * a + 1]) for a in range(3)):
                got.add("overlapping regions")
    union = brute_segments_multi(case)
    got.add("a mask of one segment" if -(-mc.nsym_of(shape) // (seg or mc.SEG_DEFAULT)) == 1 else "a mask of several segments")
    per = [set(mc.brute_segments(single(case, i)).tolist()) for i in range(len(rois))]
    for i in range(len(rois)):
        for j in range(len(rois)):
            if per[i] and per[j] and max(per[i]) < min(per[j]) and any(k not in set(union.tolist()) for k in range(max(per[i]) + 1, min(per[j]))):
                got.add("the union drops a segment between two regions")
    return got


REQUIRED = (
    {"an item of one turn, the one-sample probe", "a block straddles two items of one field", "a block straddles two items of different fields",
     "a wave's next turn lies in another item of the field", "a wave's next turn lies in another field", "a wave's next turn lies in the same region of another field",
     "an unmasked field between two masked ones", "masked first and last field", "unmasked first or last field", "an all-undefined region",
     "a region without an undefined sample", "overlapping regions", "a repeated region", "word 9 bytes", "row of several turns, partial last turn",
     "turn ends on the ragged last symbol", "a mask of one segment", "a mask of several segments", "the union drops a segment between two regions"}
    | {"word offset %d" % k for k in range(8)}
    | {"strided r=%d" % r for r in (1, 2, 3, 4)}
    | {"whole box r=%d" % r for r in range(5)}
)

ODD, LONG, CHAIN, GENERAL, FUSED = mc.ODD, mc.LONG, mc.CHAIN, mc.GENERAL, mc.FUSED


def whole(shape, level):
    bx, by, bz = mc.box_of(shape, level)
    return ((0, bz), (0, by), (0, bx))


PROBE = ((3, 4), (4, 5), (6, 7))

CASES = [
    # 13 = 5 mod 8: eight rows take every bit offset.  Region 0 has 2 * 8 = 16 turns, the probe 1, the next 3: items start at
    # turns 16, 17, 20 of a field of 22, so blocks straddle items of one field and (22 = 2 mod 4) of different fields
    (ODD, 0, [((1, 3), (0, 8), (2, 11)), PROBE, ((0, 1), (2, 5), (0, 13)), ((6, 7), (8, 9), (12, 13)), PROBE], 16, "R-IA"),
    (ODD, 0, [((1, 3), (0, 8), (2, 11)), whole(ODD, 0), ((2, 5), (3, 7), (4, 9))], 48, "ARR"),
    (ODD, 0, [whole(ODD, 0)], 0, "-R-I"),
    (ODD, 1, [whole(ODD, 1), ((0, 2), (1, 3), (1, 4))], 16, "IR-R"),
    (ODD, 2, [((0, 2), (1, 3), (1, 4)), whole(ODD, 2)], 16, "RRR"),
    # 149 = 2 * 64 + 21: rows of two full turns and a short one; nine-byte words
    (LONG, 0, [whole(LONG, 0), ((0, 3), (1, 4), (3, 140)), ((1, 2), (2, 3), (70, 71))], 16, "RI-R"),
    (LONG, 0, [((0, 1), (0, 1), (1, 149)), ((2, 3), (4, 5), (0, 149))], 48, "R-R"),
    (LONG, 1, [whole(LONG, 1)], 16, "IRR"),
    # 33 -> 17 -> 9 -> 5 -> 3: the last sample of an axis at every level
    (CHAIN, 0, [((1, 6), (2, 11), (3, 20)), ((0, 1), (0, 2), (0, 9)), ((8, 9), (15, 17), (20, 33))], 16, "R-RI-"),
    (CHAIN, 1, [whole(CHAIN, 1), ((1, 3), (2, 6), (4, 12))], 48, "RRI"),
    (CHAIN, 2, [whole(CHAIN, 2)], 16, "R-R"),
    (CHAIN, 3, [whole(CHAIN, 3), ((1, 2), (2, 3), (4, 5))], 16, "RIR"),
    (CHAIN, 4, [whole(CHAIN, 4), ((0, 1), (1, 2), (2, 3)), ((0, 1), (1, 2), (2, 3))], 16, "R-I-R"),
    # the general kernels of the masked codec's test: six regions, overlapping and repeated, far apart in the plane
    (GENERAL, 0, [((2, 11), (3, 19), (5, 36)), ((0, 1), (0, 3), (0, 37)), ((12, 13), (18, 21), (0, 37)), ((4, 9), (10, 15), (20, 30)),
                  ((4, 9), (10, 15), (20, 30)), ((6, 7), (11, 12), (25, 26))], 16, "RIR"),
    (GENERAL, 1, [((1, 6), (0, 11), (2, 19)), whole(GENERAL, 1)], 16, "A-R"),
    (GENERAL, 3, [((0, 2), (1, 3), (0, 5)), whole(GENERAL, 3)], 48, "RRRR"),
    (GENERAL, 4, [whole(GENERAL, 4)], 0, "R-R"),
    # 64^3: three masked fields of 4096 + 1 + 1024 + 4096 turns each, 27651 turns on a grid of 8192 waves: a wave takes three or
    # four turns, in the same item, in another item and in another field
    (FUSED, 0, [whole(FUSED, 0), ((31, 32), (31, 32), (31, 32)), ((16, 48), (16, 48), (16, 48)), whole(FUSED, 0)], 0, "RIR"),
    (FUSED, 2, [whole(FUSED, 2), ((3, 9), (2, 14), (1, 16))], 48, "R-IR"),
    (FUSED, 4, [whole(FUSED, 4), ((1, 3), (0, 4), (2, 4))], 16, "IRR"),
]


def case_id(case):
    shape, level, rois, seg, fields = case
    return "%s.r%d.q%d.seg%d.%s" % ("x".join(map(str, shape)), level, len(rois), seg, fields.replace("-", "u"))
