"""The geometry of a region decode (include/waverange_amd.h, "Region decode") without a GPU: the window, the set of segments
a region needs, and the exactness argument itself -- a random coefficient array gathered by the definition's map, inverted by
the oracle inside the window and cropped is, bit for bit, the crop of the full inverse.  The definition is restated here in
plain Python / numpy; nothing below shares code with the library."""
import ctypes as C

import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the repository on sys.path)
from oracle.loader import Oracle
from waverange_amd import api

WR_ERR_ARG = -1
SEGS = [1008, 4096, 59904]

# (box (nz, ny, nx) the inverse runs on, region ((z0, z1), (y0, y1), (x0, x1)), depth = levels still to invert)
CASES = [
    ((77, 129, 200), ((20, 30), (70, 71), (100, 133)), 4),
    ((77, 129, 200), ((0, 5), (120, 129), (190, 200)), 4),
    ((77, 129, 200), ((70, 77), (0, 1), (63, 65)), 4),
    ((64, 64, 160), ((30, 34), (0, 64), (64, 96)), 4),
    ((1, 50, 300), ((0, 1), (10, 20), (140, 160)), 4),
    ((39, 65, 100), ((10, 15), (35, 36), (50, 67)), 3),
    ((20, 33, 150), ((5, 8), (17, 18), (70, 80)), 2),
    ((130, 40, 40), ((64, 66), (0, 40), (0, 40)), 4),
    ((200, 200, 16), ((100, 101), (100, 101), (3, 4)), 4),
]
BIG = ((203, 203, 203), ((100, 104), (100, 104), (100, 104)), 4)


# ---- the definition ----------------------------------------------------------------------------------------------------
def h(n, times=1):
    for _ in range(times):
        n = (n + 1) // 2
    return n


def margin(d):
    m = 0
    for _ in range(d):
        m = 2 * (m + 2)
    return m


def window(n, lo, hi, d):
    if d == 0:
        return lo, hi
    m, A = margin(d), 1 << d
    a = max(0, lo - m) // A * A
    b = -(-(hi + m) // A) * A
    return a, (n if b >= n else b)


def level_extents(a, b, d):
    return [-(-b // (1 << l)) - (a >> l) for l in range(d + 1)]


def source_coordinates(box, wins, d):
    """For every point of the window, (fz, fy, fx) in the level-r box's corner of the coefficient array: the map of the
    definition, point by point (lambda, ell, then per axis)."""
    wl = [level_extents(a, b, d) for a, b in wins]
    nl = [[h(n, l) for l in range(d + 1)] for n in box]
    idx = np.indices([w[0] for w in wl])
    lam = np.zeros(idx[0].shape, dtype=np.int64)
    for l in range(1, d + 1):
        inside = np.ones(lam.shape, dtype=bool)
        for ax in range(3):
            inside &= idx[ax] < wl[ax][l]
        lam += inside
    ell = np.minimum(lam + 1, d)
    out = []
    for ax in range(3):
        a = wins[ax][0]
        w_ell, n_ell, a_ell = np.array(wl[ax])[ell], np.array(nl[ax])[ell], a >> ell
        c = idx[ax]
        out.append(np.where(c < w_ell, a_ell + c, n_ell + a_ell + (c - w_ell)))
    return out


def field_of(box, level):
    """A field shape whose level-`level` box is `box` (every extent doubled `level` times; 1 stays 1)."""
    return tuple(n if n == 1 else n << level for n in box)


def random_roi(rng, box):
    out = []
    for n in box:
        lo = int(rng.integers(0, n))
        out.append((lo, int(rng.integers(lo + 1, n + 1))))
    return tuple(out)


def face_and_point_regions(box):
    nz, ny, nx = box
    whole = ((0, nz), (0, ny), (0, nx))
    yield whole
    for ax, n in enumerate(box):
        for lo, hi in ((0, 1), (n - 1, n), (0, min(n, 3)), (max(0, n - 3), n), (n // 2, n // 2 + 1)):
            r = list(whole)
            r[ax] = (lo, hi)
            yield tuple(r)
    yield tuple((n // 2, n // 2 + 1) for n in box)
    yield tuple((n - 1, n) for n in box)
    yield ((0, 1),) * 3


def c_box(roi):
    (z0, z1), (y0, y1), (x0, x1) = roi
    return api.Box(x0, y0, z0, x1, y1, z1)


# ---- wr_roi_window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(77, 129, 200), (1, 50, 300), (64, 64, 64), (203, 203, 203), (5, 1, 1), (24, 400, 40)])
def test_window(shape):
    rng = np.random.default_rng(7)
    for level in range(5):
        box = api.lowres_shape(shape, level)
        assert box == tuple(h(n, level) for n in shape)
        regions = list(face_and_point_regions(box)) + [random_roi(rng, box) for _ in range(20)]
        for roi in regions:
            want = tuple(window(n, lo, hi, 4 - level) for n, (lo, hi) in zip(box, roi))
            assert api.roi_window(shape, level, roi) == want, (shape, level, roi)
            for (a, b), (lo, hi), n in zip(want, roi, box):
                assert 0 <= a <= lo < hi <= b <= n and a % (1 << (4 - level)) == 0
    # a stream without the transform: level 0 only, and the window is the region
    for roi in face_and_point_regions(shape):
        assert api.roi_window(shape, 0, roi, wlev=0) == roi


def test_window_of_the_listed_cases():
    for box, roi, d in CASES + [BIG]:
        level = 4 - d
        want = tuple(window(n, lo, hi, d) for n, (lo, hi) in zip(box, roi))
        assert api.roi_window(field_of(box, level), level, roi) == want, (box, roi, d)
    assert api.roi_window(BIG[0], 0, BIG[1]) == ((32, 176),) * 3  # 144 = 9 x 16 per axis
    assert api.roi_window((64, 64, 64), 0, ((30, 31),) * 3) == ((0, 64),) * 3  # the margin of four levels covers a 64-cube


# ---- wr_seg_roi_segments -----------------------------------------------------------------------------------------------
def brute_force_segments(shape, level, roi, seg, wlev=4):
    """index // seg over every point of the window, through the definition's map, as a sorted array."""
    nz, ny, nx = shape
    box = tuple(h(n, level) for n in shape)
    d = wlev - level
    wins = [window(n, lo, hi, d) for n, (lo, hi) in zip(box, roi)]
    fz, fy, fx = source_coordinates(box, wins, d)
    return np.unique((fx + nx * (fy + ny * fz)) // seg)


SEGMENT_CASES = [
    ((77, 129, 200), 0, ((20, 30), (70, 71), (100, 133))),
    ((77, 129, 200), 0, ((70, 77), (0, 1), (63, 65))),
    ((77, 129, 200), 2, ((3, 5), (30, 33), (0, 50))),
    ((77, 129, 200), 4, ((1, 2), (2, 6), (3, 4))),
    ((1, 50, 300), 0, ((0, 1), (10, 20), (140, 160))),
    ((1, 50, 300), 1, ((0, 1), (24, 25), (0, 150))),
    ((24, 400, 40), 0, ((0, 24), (0, 4), (0, 40))),
    ((301, 37, 50), 0, ((150, 153), (0, 37), (49, 50))),
    ((301, 37, 50), 3, ((37, 38), (0, 5), (6, 7))),
    ((64, 64, 64), 0, ((30, 31), (30, 31), (30, 31))),
    ((240, 48, 64), 0, ((118, 122), (0, 48), (0, 64))),
    ((130, 140, 150), 1, ((30, 32), (30, 32), (30, 32))),
]


@pytest.mark.parametrize("seg", SEGS)
def test_segment_set(seg):
    fn = api.lib().wr_seg_roi_segments
    for shape, level, roi in SEGMENT_CASES:
        nz, ny, nx = shape
        want = brute_force_segments(shape, level, roi, seg)
        got = api.seg_roi_segments(shape, level, roi, seg)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (shape, level, roi, seg)
        r = c_box(roi)
        assert fn(nx, ny, nz, level, 4, C.byref(r), seg, None, 0) == want.size  # ids = NULL counts
        assert fn(nx, ny, nz, level, 4, C.byref(r), seg, None, 10 ** 6) == want.size
        cap = want.size // 2  # a short cap: the count comes back whole, nothing is written past the cap
        buf = np.full(want.size + 4, 0xDEADBEEF, dtype=np.uint32)
        assert fn(nx, ny, nz, level, 4, C.byref(r), seg, buf.ctypes.data, cap) == want.size
        assert np.array_equal(buf[:cap].astype(np.int64), want[:cap]) and np.all(buf[cap:] == 0xDEADBEEF), (shape, level, roi, seg)
    # without the transform a region needs the segments its own rows touch
    shape, roi = (77, 129, 200), ((20, 30), (70, 71), (100, 133))
    got = api.seg_roi_segments(shape, 0, roi, seg, wlev=0)
    assert np.array_equal(got.astype(np.int64), brute_force_segments(shape, 0, roi, seg, wlev=0))
    z, x = np.arange(20, 30), np.arange(100, 133)
    assert np.array_equal(got.astype(np.int64), np.unique(((70 + 129 * z[:, None]) * 200 + x[None, :]) // seg))


def test_whole_box_needs_what_the_level_needs():
    for shape in [(77, 129, 200), (1, 50, 300), (64, 64, 64)]:
        for level in range(5):
            whole = tuple((0, n) for n in api.lowres_shape(shape, level))
            for seg in SEGS:
                assert np.array_equal(api.seg_roi_segments(shape, level, whole, seg), api.seg_lowres_segments(shape, level, seg))


def test_known_counts():
    """Counts that the GPU tests and DESIGN.md section 10.2 quote, from the geometry alone."""
    def count(shape, roi, seg):
        n = int(np.prod(shape))
        return api.seg_roi_segments(shape, 0, roi, seg).size, -(-n // seg)
    assert count(BIG[0], BIG[1], 4096) == (1448, 2043)
    assert count(BIG[0], BIG[1], 59904) == (114, 140)
    assert count((24, 400, 40), ((0, 24), (0, 4), (0, 40)), 4096) == (72, 94)
    assert count((301, 37, 50), ((150, 153), (0, 37), (49, 50)), 4096) == (91, 136)
    assert np.array_equal(api.seg_roi_segments(BIG[0], 0, BIG[1]), api.seg_roi_segments(BIG[0], 0, BIG[1], api.SEG_DEFAULT))
    # a 1024^3 field at the default segment length (17 925 segments per plane)
    n, fn = 1024, api.lib().wr_seg_roi_segments
    def share(roi):
        r = c_box(roi)
        return fn(n, n, n, 0, 4, C.byref(r), 0, None, 0)
    cube = lambda e: ((n // 2 - e // 2, n // 2 + e // 2),) * 3  # noqa: E731
    assert [share(cube(e)) for e in (32, 64, 128, 256)] == [1202, 1577, 2387, 4514]
    assert share(((500, 501), (0, n), (0, n))) == 3468
    assert share(((0, n), (500, 501), (0, n))) == 6546
    assert share(((0, n), (0, n), (500, 501))) == 17925


# ---- the exactness argument --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def region_is_exact(oracle, rng, box, roi, d):
    level = 4 - d
    wins = api.roi_window(field_of(box, level), level, roi)
    coef = rng.standard_normal(box)  # the coefficient array of the box
    fz, fy, fx = source_coordinates(box, wins, d)
    win = np.ascontiguousarray(coef[fz, fy, fx])
    assert win.shape == tuple(b - a for a, b in wins)
    inv = oracle.cdf97_3d(win, -d) if d else win
    got = inv[tuple(slice(lo - a, hi - a) for (lo, hi), (a, _) in zip(roi, wins))]
    full = oracle.cdf97_3d(coef, -d) if d else coef
    want = full[tuple(slice(lo, hi) for lo, hi in roi)]
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


@pytest.mark.parametrize("case", CASES + [BIG, ((203, 203, 203), ((0, 3), (199, 203), (100, 104)), 4), ((160, 160, 64), ((70, 90), (64, 65), (0, 64)), 4)],
                         ids=lambda c: "x".join(map(str, c[0])) + "-d%d" % c[2])
def test_crop_of_the_window_inverse_is_the_crop_of_the_full_inverse(oracle, case):
    box, roi, d = case
    assert region_is_exact(oracle, np.random.default_rng(1), box, roi, d), case


def test_random_sweep(oracle):
    rng = np.random.default_rng(2)
    for _ in range(40):
        d = int(rng.integers(0, 5))
        box = tuple(int(rng.integers(1, 120)) for _ in range(3))
        roi = random_roi(rng, box)
        assert region_is_exact(oracle, rng, box, roi, d), (box, roi, d)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    win_fn, seg_fn = api.lib().wr_roi_window, api.lib().wr_seg_roi_segments
    good = ((1, 2), (3, 5), (0, 64))
    w = api.Box()

    def refused(roi, level=0, wlev=4, seg=4096, dims=(64, 64, 64)):
        r = c_box(roi)
        w.x0 = w.z1 = -7  # a refused call leaves the window alone
        ok_w = win_fn(*dims, level, wlev, C.byref(r), C.byref(w)) == WR_ERR_ARG and (w.x0, w.z1) == (-7, -7)
        return ok_w and seg_fn(*dims, level, wlev, C.byref(r), seg, None, 0) == 0

    assert win_fn(64, 64, 64, 0, 4, C.byref(c_box(good)), C.byref(api.Box())) == 0
    for roi in (((1, 1), (3, 5), (0, 64)), ((2, 1), (3, 5), (0, 64)),           # empty
                ((1, 2), (3, 65), (0, 64)), ((-1, 2), (3, 5), (0, 64)), ((1, 2), (3, 5), (0, 65)), ((64, 65), (3, 5), (0, 64))):
        assert refused(roi), roi
        with pytest.raises(api.WaveRangeError):
            api.roi_window((64, 64, 64), 0, roi)
        with pytest.raises(api.WaveRangeError):
            api.seg_roi_segments((64, 64, 64), 0, roi, 4096)
    assert refused(((1, 2), (3, 5), (0, 33)), level=1)      # the box of level 1 is 32 wide
    assert not refused(((1, 2), (3, 5), (0, 32)), level=1)
    assert refused(good, level=5) and refused(good, level=-1)
    assert refused(((0, 1),) * 3, level=1, wlev=0)          # level > wlev
    assert refused(good, wlev=3)
    assert refused(good, dims=(0, 64, 64))
    assert win_fn(64, 64, 64, 0, 4, None, C.byref(w)) == WR_ERR_ARG
    r = c_box(good)
    for seg in (60000, 24, 8):                               # a bad segment length
        assert seg_fn(64, 64, 64, 0, 4, C.byref(r), seg, None, 0) == 0
    with pytest.raises(api.WaveRangeError):
        api.seg_roi_segments((64, 64, 64), 0, good, 60000)
