"""The geometry of a low-resolution decode (include/waverange_amd.h) without a GPU: box dimensions, the scale, and the
set of segments a level needs, each against the formula of the definition evaluated here in plain Python / numpy."""
import ctypes as C
import math

import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the repository on sys.path)
from waverange_amd import api

SHAPES_XYZ = [(200, 129, 77), (64, 64, 64), (70, 50, 1), (5, 1, 1), (1024, 1024, 1024)]
SMALL_XYZ = SHAPES_XYZ[:4]
LEVELS = range(5)
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")
WR_ERR_ARG = -1


def h(n):
    return (n + 1) // 2


def box_and_exponent(dims, level):
    dims, e = list(dims), 0
    for _ in range(level):
        e += sum(1 for n in dims if n > 1)
        dims = [h(n) for n in dims]
    return tuple(dims), e


def brute_force_segments(nx, ny, nz, level, seg):
    """i // seg over every index of the box, as a sorted array."""
    (bx, by, bz), _ = box_and_exponent((nx, ny, nz), level)
    z, y, x = np.meshgrid(np.arange(bz, dtype=np.int64), np.arange(by, dtype=np.int64), np.arange(bx, dtype=np.int64), indexing="ij")
    return np.unique(((y + ny * z) * nx + x) // seg)


@pytest.mark.parametrize("dims", SHAPES_XYZ)
def test_dims_and_scale(dims):
    nx, ny, nz = dims
    for level in LEVELS:
        want, e = box_and_exponent(dims, level)
        b = [C.c_int() for _ in range(3)]
        assert api.lib().wr_lowres_dims(nx, ny, nz, level, *[C.byref(v) for v in b]) == 0
        assert tuple(v.value for v in b) == want, (dims, level)
        assert api.lowres_shape((nz, ny, nx), level) == want[::-1]
        s = math.ldexp(SQRT_HALF if e % 2 else 1.0, -(e // 2))
        assert api.lowres_scale((nz, ny, nx), level).hex() == s.hex(), (dims, level, e)
        if level == 0:
            assert s == 1.0
    # the exponent of a cube: three axes per level
    assert box_and_exponent((64, 64, 64), 4)[1] == 12 and api.lowres_scale((64, 64, 64), 4) == 2.0 ** -6
    assert box_and_exponent((5, 1, 1), 4) == ((1, 1, 1), 3)


@pytest.mark.parametrize("seg", [16, 4096, 59904])
@pytest.mark.parametrize("dims", SMALL_XYZ)
def test_segment_set(dims, seg):
    nx, ny, nz = dims
    n = nx * ny * nz
    fn = api.lib().wr_seg_lowres_segments
    for level in LEVELS:
        want = brute_force_segments(nx, ny, nz, level, seg)
        got = api.seg_lowres_segments((nz, ny, nx), level, seg)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (dims, seg, level)
        assert fn(nx, ny, nz, level, seg, None, 0) == want.size  # ids = NULL counts
        assert fn(nx, ny, nz, level, seg, None, 10 ** 6) == want.size
        if level == 0:
            assert np.array_equal(want, np.arange((n + seg - 1) // seg)), (dims, seg)
        # a short cap: the count comes back whole, nothing is written past the cap
        cap = want.size // 2
        buf = np.full(want.size + 4, 0xDEADBEEF, dtype=np.uint32)
        assert fn(nx, ny, nz, level, seg, buf.ctypes.data, cap) == want.size
        assert np.array_equal(buf[:cap].astype(np.int64), want[:cap]) and np.all(buf[cap:] == 0xDEADBEEF), (dims, seg, level)


def test_default_and_refused_segment_length():
    shape = (77, 129, 200)
    assert np.array_equal(api.seg_lowres_segments(shape, 2), api.seg_lowres_segments(shape, 2, 59904))
    assert api.lib().wr_seg_lowres_segments(200, 129, 77, 1, 60000, None, 0) == 0
    assert api.lib().wr_seg_lowres_segments(200, 129, 77, 1, 24, None, 0) == 0  # not a multiple of 16
    with pytest.raises(api.WaveRangeError):
        api.seg_lowres_segments(shape, 1, 60000)


def test_arguments():
    b = [C.c_int(-7) for _ in range(3)]
    for level in (-1, 5, 100):
        assert api.lib().wr_lowres_dims(64, 64, 64, level, *[C.byref(v) for v in b]) == WR_ERR_ARG
        assert [v.value for v in b] == [-7] * 3
        assert api.lib().wr_lowres_scale(64, 64, 64, level) == 0.0
        assert api.lib().wr_seg_lowres_segments(64, 64, 64, level, 4096, None, 0) == 0
        with pytest.raises(api.WaveRangeError):
            api.lowres_shape((64, 64, 64), level)
    assert api.lib().wr_lowres_dims(0, 64, 64, 1, *[C.byref(v) for v in b]) == WR_ERR_ARG


def test_shares_of_a_1024_cube():
    """The shares of a plane's segments that levels 1..4 of a 1024^3 field need at the default segment length: derived
    from the geometry alone (README)."""
    nseg = (1024 ** 3 + api.SEG_DEFAULT - 1) // api.SEG_DEFAULT
    share = [api.lib().wr_seg_lowres_segments(1024, 1024, 1024, r, 0, None, 0) / nseg for r in range(5)]
    assert share[0] == 1.0
    assert all(a > b for a, b in zip(share, share[1:]))
    assert 0.25 < share[1] < 0.30 and 0.06 < share[2] < 0.10 and share[3] < 0.04 and share[4] < 0.02, share
