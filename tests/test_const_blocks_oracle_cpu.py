"""The host coder on the real planes of the synthetic field, whose first plane is mostly constant blocks (full blocks of one
symbol, which the coder passes over in the header phase of a step): every stream byte for byte the oracle's, through every
host entry point, and every plane back.  CPU only."""
import numpy as np
import pytest

import util  # noqa: F401  (puts the repository root on sys.path)
from oracle.loader import Oracle
from waverange_amd import api, synth

BLOCK = 60000
# shape (nz, ny, nx) -> constant full blocks in plane 0 at tol 1e-3, counted on the oracle's planes: the floor below
# which an input would exercise nothing
SHAPES = {(64, 64, 128): 4, (112, 80, 96): 10, (128, 128, 128): 27}


def _constant_blocks(plane):
    full = plane[:plane.size // BLOCK * BLOCK].reshape(-1, BLOCK)
    return int((full == full[:, :1]).all(axis=1).sum())


@pytest.fixture(scope="module", params=sorted(SHAPES), ids=lambda s: "x".join(str(v) for v in s[::-1]))
def case(request):
    shape = request.param
    o = Oracle()
    f = synth.field(shape[2], shape[1], shape[0], seed=2024)
    assert f.shape == shape
    enc = o.encode(f, 1e-3)
    streams, off = [], 0
    for n in enc["len_enc_vec"]:
        streams.append(enc["data"][off:off + n].copy())
        off += n
    planes = []
    for s in streams:
        p, got = o.range_decode(s, f.size)
        assert got == f.size
        planes.append(p.copy())
    return shape, planes, streams


def test_plane0_has_constant_blocks(case):
    shape, planes, _ = case
    assert _constant_blocks(planes[0]) >= SHAPES[shape], (_constant_blocks(planes[0]), SHAPES[shape])


def _have_vec():
    """the 16-lane loops need AVX-512: the entry points raise where the CPU lacks it"""
    try:
        api.range_encode_vec([np.zeros(8, dtype=np.uint8)])
        return True
    except api.WaveRangeError:
        return False


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.size == b.size and np.array_equal(a, b), "%s: plane %d differs from the oracle's" % (what, k)


def test_streams_are_the_oracles(case):
    shape, planes, streams = case
    assert _constant_blocks(planes[0]) >= SHAPES[shape]
    n = planes[0].size
    vec = _have_vec()
    _same([api.range_encode(p) for p in planes], streams, "range_encode")
    _same(api.range_encode_multi(planes), streams, "range_encode_multi")
    # sixteen and more lanes: the field's planes five times over
    many, many_streams = planes * 5, streams * 5
    if vec:
        _same(api.range_encode_vec(many), many_streams, "range_encode_vec")
    for chunk in (BLOCK, 3 * BLOCK):
        for mode in (0, 1, 2):
            if mode == 2 and not vec:
                continue
            if mode == 1:
                api.set_coder_pool(2, 4)
            try:
                _same(api.range_encode_windowed(planes, chunk, mode), streams, "range_encode_windowed mode %d" % mode)
                back, got = api.range_decode_windowed(streams, n, chunk, mode)
            finally:
                api.set_coder_pool(0)
            assert got == [n] * len(planes)
            _same(back, planes, "range_decode_windowed mode %d" % mode)
    api.set_coder_pool(2, 4)
    try:
        _same(api.range_encode_pool(many), many_streams, "range_encode_pool")
        back, got = api.range_decode_pool(many_streams, [n] * len(many))
    finally:
        api.set_coder_pool(0)
    assert got == [n] * len(many)
    _same(back, many, "range_decode_pool")
    for p, s in zip(planes, streams):
        back, got = api.range_decode(s, n)
        assert got == n and np.array_equal(back, p)
    back, got = api.range_decode_multi(streams, n)
    assert got == [n] * len(planes)
    _same(back, planes, "range_decode_multi")
    if vec:
        back, got = api.range_decode_vec(many_streams, [n] * len(many))
        assert list(got) == [n] * len(many)
        _same(back, many, "range_decode_vec")
