"""The case table of the masked region / low-resolution decode (include/waverange_amd.h), shared by
test_masked_roi_cases_cpu.py, test_gpu_mask_restore_box.py and test_gpu_masked_roi.py.

A case is (field shape (nx, ny, nz), level, roi, mask segment length).  roi is ((z0, z1), (y0, y1), (x0, x1)) in the box of the
level, or None for the whole box; the segment length counts mask SYMBOLS of 8 bits (0: the default, one segment at these sizes).
classes_of() computes, from the geometry alone, which paths of k_mask_restore_box and of the crop a case reaches; REQUIRED names
the ones the table must reach, and the CPU test holds the table to it.

The kernel's walk, which this file simulates (csrc/wr_mask.hip): a wave takes 64 consecutive x of one region row per turn.  At
level 0 the turn's bits J0 .. J0 + cnt - 1 come from the bytes J0 >> 3 .. (J0 + cnt - 1) >> 3 and no others (up to nine); at a
level r > 0 lane l reads byte J >> 3 of its own bit J = ((x0 + 64 t + l) << r) + nx * ((y << r) + ny * (z << r))."""
import numpy as np

SEG_DEFAULT = 59904  # WR_SEG_DEFAULT


def half_up(n):
    return (n + 1) // 2


def box_of(shape, level):
    """(bx, by, bz) of the level"""
    b = tuple(shape)
    for _ in range(level):
        b = tuple(half_up(v) for v in b)
    return b


def region_of(case):
    """(x0, x1, y0, y1, z0, z1) of a case"""
    shape, level, roi, _ = case
    if roi is None:
        bx, by, bz = box_of(shape, level)
        return 0, bx, 0, by, 0, bz
    (z0, z1), (y0, y1), (x0, x1) = roi
    return x0, x1, y0, y1, z0, z1


def out_shape(case):
    x0, x1, y0, y1, z0, z1 = region_of(case)
    return z1 - z0, y1 - y0, x1 - x0


def bit_index(case):
    """J of every sample of the region, shaped (cz, cy, cx): Python integers in an object-free int64 array (the shapes here are small)"""
    (nx, ny, nz), level, _, _ = case
    x0, x1, y0, y1, z0, z1 = region_of(case)
    z, y, x = np.meshgrid(np.arange(z0, z1, dtype=np.int64), np.arange(y0, y1, dtype=np.int64), np.arange(x0, x1, dtype=np.int64), indexing="ij")
    return (x << level) + nx * ((y << level) + ny * (z << level))


def coarse_und(und, case):
    """the coarse mask of the region: und is the field's boolean mask shaped (nz, ny, nx)"""
    _, level, _, _ = case
    x0, x1, y0, y1, z0, z1 = region_of(case)
    s = 1 << level
    return und[::s, ::s, ::s][z0:z1, y0:y1, x0:x1]


def seg_len(case):
    return case[3] or SEG_DEFAULT


def nsym_of(shape):
    return (shape[0] * shape[1] * shape[2] + 7) // 8


def brute_segments(case):
    """{(J >> 3) // seg} over every sample of the region, ascending"""
    return np.unique((bit_index(case) >> 3) // seg_len(case)).astype(np.uint32)


def turns_of(case):
    """(J of the turn's first sample, cnt) of every turn of the kernel's walk, level 0 or not"""
    J = bit_index(case)
    cx = J.shape[2]
    for row in J.reshape(-1, cx):
        for xs in range(0, cx, 64):
            yield row[xs:xs + 64]


def kernel_reads(case):
    """the set of mask bytes the kernel's definition reads"""
    _, level, _, _ = case
    got = set()
    for js in turns_of(case):
        if level == 0:
            got.update(range(int(js[0]) >> 3, (int(js[-1]) >> 3) + 1))
        else:
            got.update(int(j) >> 3 for j in js)
    return got


def classes_of(case):
    shape, level, roi, _ = case
    n = shape[0] * shape[1] * shape[2]
    seg = seg_len(case)
    last_sym = nsym_of(shape) - 1
    got = set()
    cz, cy, cx = out_shape(case)
    if level == 0:
        for js in turns_of(case):
            j0, j1 = int(js[0]), int(js[-1])
            if (j1 >> 3) - (j0 >> 3) == 8:
                got.add("word 9 bytes")
        for j0 in bit_index(case)[:, :, 0].reshape(-1):
            got.add("word offset %d" % (int(j0) & 7))
    else:
        got.add("strided r=%d" % level)
    if cx > 64 and cx % 64:
        got.add("row of several turns, partial last turn")
    for js in turns_of(case):
        j0, j1 = int(js[0]), int(js[-1])
        if n % 8 and (j1 >> 3) == last_sym:
            got.add("turn ends on the ragged last symbol")
        if (j0 >> 3) // seg != (j1 >> 3) // seg:
            got.add("segment boundary inside a turn")
    nseg = len(brute_segments(case))
    got.add("1 segment" if nseg == 1 else "several segments")
    if int(bit_index(case).max()) == n - 1:
        got.add("the field's last sample")
    if roi is None:
        got.add("whole box r=%d" % level)
    if cx * cy * cz == 1:
        got.add("one sample")
    return got


REQUIRED = (
    {"word offset %d" % k for k in range(8)}
    | {"word 9 bytes", "row of several turns, partial last turn", "turn ends on the ragged last symbol", "1 segment", "several segments",
       "segment boundary inside a turn", "the field's last sample", "one sample"}
    | {"strided r=%d" % r for r in (1, 2, 3, 4)}
    | {"whole box r=%d" % r for r in range(5)}
)

ODD, LONG, CHAIN, GENERAL, FUSED = (13, 9, 7), (149, 5, 3), (33, 17, 9), (37, 21, 13), (64, 64, 64)

CASES = [
    # odd nx: the row starts of eight rows take every bit offset (13 = 5 mod 8)
    (ODD, 0, None, 16), (ODD, 0, None, 48), (ODD, 0, None, 0),
    (ODD, 0, ((1, 3), (0, 8), (2, 11)), 16), (ODD, 0, ((3, 4), (4, 5), (6, 7)), 16), (ODD, 0, ((6, 7), (8, 9), (12, 13)), 48),
    (ODD, 1, None, 16), (ODD, 2, ((0, 2), (1, 3), (1, 4)), 16),
    # 149 = 2 * 64 + 21: two full turns and a short one, words that start anywhere
    (LONG, 0, None, 16), (LONG, 0, ((0, 3), (1, 4), (3, 140)), 48), (LONG, 1, None, 16), (LONG, 2, None, 0),
    # 33 -> 17 -> 9 -> 5 -> 3: 2 << 4 = 32 is the last x at level 4; 4 << 3, 2 << 3, 1 << 3 the last sample of all three axes at level 3
    (CHAIN, 0, None, 16), (CHAIN, 1, None, 48), (CHAIN, 2, None, 16), (CHAIN, 3, None, 16), (CHAIN, 4, None, 16),
    (CHAIN, 0, ((1, 6), (2, 11), (3, 20)), 48), (CHAIN, 3, ((1, 2), (2, 3), (4, 5)), 0), (CHAIN, 4, ((0, 1), (1, 2), (2, 3)), 16),
    # the general kernels of the masked codec's test
    (GENERAL, 0, None, 48), (GENERAL, 0, ((2, 11), (3, 19), (5, 36)), 16), (GENERAL, 1, ((1, 6), (0, 11), (2, 19)), 16),
    (GENERAL, 2, None, 16), (GENERAL, 3, ((0, 2), (1, 3), (0, 5)), 48), (GENERAL, 4, None, 0),
    # all four levels fused
    (FUSED, 0, None, 0), (FUSED, 0, ((16, 48), (16, 48), (16, 48)), 48), (FUSED, 0, ((31, 32), (0, 64), (0, 64)), 48),
    (FUSED, 1, None, 48), (FUSED, 2, None, 16), (FUSED, 3, None, 0), (FUSED, 4, None, 16), (FUSED, 2, ((3, 9), (2, 14), (1, 16)), 16),
]


def case_id(case):
    shape, level, roi, seg = case
    where = "box" if roi is None else "x%d-%d.y%d-%d.z%d-%d" % (roi[2] + roi[1] + roi[0])
    return "%s.r%d.%s.seg%d" % ("x".join(map(str, shape)), level, where, seg)


# ---- the undefined sets, per field shape: boolean arrays shaped (nz, ny, nx), read-only, built once
_und = {}


def und_recipe(shape):
    """the masked codec test's recipe: about 30 % in one coherent region plus three lone samples"""
    key = ("recipe", shape)
    if key not in _und:
        nx, ny, nz = shape
        z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
        g = np.sin(5.0 * x + 1.0) + np.cos(4.0 * y) + np.sin(3.0 * z + 2.0 * x)
        und = g > np.quantile(g, 0.7)
        lone = np.random.default_rng(nx * ny * nz).integers(0, und.size, size=3)
        und = und.copy()
        und.reshape(-1)[lone] = True
        und.setflags(write=False)
        _und[key] = und
    return _und[key]


def und_isolated(shape):
    """isolated bits only, about one in 150: most words of the restore are 0"""
    key = ("isolated", shape)
    if key not in _und:
        nx, ny, nz = shape
        und = np.random.default_rng(7 + nx * ny * nz).random((nz, ny, nx)) < 1.0 / 150
        und[nz - 1, ny - 1, nx - 1] = True
        und[0, 0, 0] = True
        und.setflags(write=False)
        _und[key] = und
    return _und[key]


def und_region(case):
    """every sample of the case's region undefined, and a few others"""
    shape, level, _, _ = case
    nx, ny, nz = shape
    und = np.zeros((nz, ny, nx), bool)
    und.reshape(-1)[bit_index(case).reshape(-1)] = True
    und.reshape(-1)[::97] = True
    return und


def packed(und):
    return np.packbits(und.reshape(-1), bitorder="little")
