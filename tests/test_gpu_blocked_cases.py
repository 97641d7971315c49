"""The reorder kernel on the table of tests/blocked_cases.py: the whole plane both ways and by brick list both ways against the
permutation, at the planes that reach the kernel's wide path in full 128-byte groups, at every brick edge and in both modes.
Each case's plan is asserted again in front of its checks.  The reference is plane[pi] with pi from wr_blocked_order, and for a
list the stream ranges of the listed bricks from the table's own geometry (tests/test_blocked_cases_cpu.py holds the two
against each other).  Every comparison is equality of whole arrays of bytes or of bit patterns: nothing has a tolerance."""
import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the repository on sys.path)
import blocked_cases as bc
from test_gpu_blocked import lowres_all_ways, roi_all_ways, same_bits, streams
from waverange_amd import api

pytestmark = pytest.mark.gpu

KEYS = list(bc.CASES)
ids_of = lambda k: "%s-w%d-b%d" % ("x".join(map(str, k[0])), k[1], k[2])  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


_REF = {}


def ref(key):
    """Per case, made once and never written to: pi, two random planes (the second is what a list call's destination holds
    beforehand), an all-equal plane, and per brick list the mask of the stream positions inside the listed bricks."""
    if key not in _REF:
        shape, wlev, B = key
        n = shape[0] * shape[1] * shape[2]
        rng = np.random.default_rng([n, wlev, B])
        pi = api.blocked_order(shape, wlev, B).astype(np.int64)
        bricks = bc.bricks_of(shape, wlev, B)
        masks = {}
        for name, ids in bc.brick_lists(shape, wlev, B).items():
            m = np.zeros(n, dtype=bool)
            for i in ids:
                b = bricks[i]
                m[b.start:b.start + b.h[0] * b.h[1] * b.h[2]] = True
            masks[name] = (np.asarray(ids, dtype=np.uint32), m)
        r = dict(pi=pi, plane=rng.integers(0, 256, n, dtype=np.uint8), fill=rng.integers(0, 256, n, dtype=np.uint8),
                 flat=np.full(n, 0xA5, dtype=np.uint8), masks=masks)
        for v in (r["pi"], r["plane"], r["fill"], r["flat"]):
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def scatter(pi, blocked):
    out = np.empty_like(blocked)
    out[pi] = blocked
    return out


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_whole_plane(ctx, key):
    shape, wlev, B = key
    bc.check_plan(api, key)
    r = ref(key)
    pi = r["pi"]
    for name in ("plane", "flat"):
        plane = r[name]
        blocked = ctx.plane_reorder(plane, shape, wlev, B)
        assert np.array_equal(blocked, plane[pi]), (key, name, "forward")
        assert np.array_equal(ctx.plane_reorder(plane, shape, wlev, B, inverse=True), scatter(pi, plane)), (key, name, "inverse")
        assert np.array_equal(ctx.plane_reorder(blocked, shape, wlev, B, inverse=True), plane), (key, name, "round trip")


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_list_inverse(ctx, key):
    """out[pi[p]] == blocked[p] for every p inside the listed bricks, and what the destination held everywhere else"""
    shape, wlev, B = key
    bc.check_plan(api, key)
    r = ref(key)
    pi = r["pi"]
    for blocked, fill in ((r["plane"], r["fill"]), (r["flat"], r["fill"])):
        for name, (ids, m) in r["masks"].items():
            want = fill.copy()
            want[pi[m]] = blocked[m]
            got = ctx.plane_reorder_list(blocked, shape, wlev, B, ids, inverse=True, fill=fill)
            assert np.array_equal(got, want), (key, name, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_list_forward(ctx, key):
    """out[p] == plane[pi[p]] for every p inside the listed bricks, and what the destination held everywhere else"""
    shape, wlev, B = key
    bc.check_plan(api, key)
    r = ref(key)
    pi = r["pi"]
    for plane, fill in ((r["plane"], r["fill"]), (r["flat"], r["fill"])):
        for name, (ids, m) in r["masks"].items():
            want = np.where(m, plane[pi], fill)
            got = ctx.plane_reorder_list(plane, shape, wlev, B, ids, fill=fill)
            assert np.array_equal(got, want), (key, name, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_list_of_every_brick_is_the_whole_plane(ctx, key):
    shape, wlev, B = key
    plans = bc.check_plan(api, key)
    r = ref(key)
    ids, m = r["masks"]["all"]
    assert ids.size == plans["list"]["nbricks"] and m.all()
    for inverse in (False, True):
        whole = ctx.plane_reorder(r["plane"], shape, wlev, B, inverse=inverse)
        assert np.array_equal(ctx.plane_reorder_list(r["plane"], shape, wlev, B, ids, inverse=inverse, fill=r["fill"]), whole), (key, inverse)


def test_list_refusals(ctx):
    """Each is WR_ERR_ARG before any copy or launch -- the destination still holds what it held -- and a good call follows."""
    key = ((8, 24, 576), 4, 32)
    shape, wlev, B = key
    nz, ny, nx = shape
    plans = bc.check_plan(api, key)
    nb = plans["list"]["nbricks"]
    r = ref(key)
    n = r["plane"].size
    fn = api.lib().wr_dev_plane_reorder_list
    d_src, d_dst = ctx.alloc(n + 16).upload(r["plane"]), ctx.alloc(n + 16).upload(r["fill"])
    try:
        def call(ids, dst=d_dst.ptr, src=d_src.ptr, nlist=None, brick=B, lev=wlev, dims=(nx, ny, nz)):
            v = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
            return fn(ctx.h, dst, src, *dims, lev, brick, 1, None if v is None or not v.size else v.ctypes.data, (v.size if v is not None else 0) if nlist is None else nlist)

        bad = [("unsorted", lambda: call([3, 2, 5])), ("repeated", lambda: call([2, 3, 3])), ("out of range", lambda: call([0, nb])),
               ("far out of range", lambda: call([0xFFFFFFFF])), ("null ids", lambda: call(None, nlist=3)),
               ("unaligned destination", lambda: call([1], dst=d_dst.ptr + 8)), ("unaligned source", lambda: call([1], src=d_src.ptr + 4)),
               ("in place", lambda: call([1], dst=d_src.ptr)), ("null source", lambda: call([1], src=None)),
               ("brick", lambda: call([1], brick=12)), ("wlev", lambda: call([1], lev=3)), ("dims", lambda: call([0], dims=(nx, 0, nz)))]
        for what, f in bad:
            assert f() == -1, what
            assert api.lib().wr_last_error(), what
            assert np.array_equal(d_dst.download(np.uint8, n), r["fill"]), what
            assert np.array_equal(d_src.download(np.uint8, n), r["plane"]), what
        assert call([]) == 0 and call(None, nlist=0) == 0  # an empty list: nothing is launched
        assert np.array_equal(d_dst.download(np.uint8, n), r["fill"])
        ids, m = r["masks"]["box-ends"]
        assert call(ids) == 0
        want = r["fill"].copy()
        want[r["pi"][m]] = r["plane"][m]
        assert np.array_equal(d_dst.download(np.uint8, n), want)
    finally:
        d_src.free()
        d_dst.free()
    with pytest.raises(api.WaveRangeError) as e:
        ctx.plane_reorder_list(r["plane"], shape, wlev, B, [5, 4])
    assert "error -1" in str(e.value), str(e.value)


# ---- codec level: a blocked stream of a table shape decodes to the bits of the WRS1 stream of the same field
CODEC = [((40, 72, 96), 32), ((72, 40, 160), 64), ((8, 24, 576), 0)]  # brick 0: the default, 32


def codec_regions(shape, level):
    """two regions in the box of `level`: its high corner, and one that straddles the boundary between the low and the high
    half of the next level in x (e_1 of that box)"""
    bz, by, bx = api.lowres_shape(shape, level)
    mid = (bx + 1) // 2
    corner = ((max(bz - 3, 0), bz), (max(by - 2, 0), by), (max(bx - 5, 0), bx))
    straddle = ((bz // 2, min(bz // 2 + 2, bz)), (by // 3, min(by // 3 + 3, by)), (mid - 3, mid + 4))
    return corner, straddle


@pytest.mark.parametrize("shape,brick", CODEC, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_codec_level(ctx, shape, brick):
    bc.check_plan(api, (shape, 4, brick or 32))
    s = streams(ctx, shape, 1e-6, brick)
    f, wrs1, wrs2 = s["f"], s["wrs1"], s["wrs2"]
    assert wrs2["wlev"] == 4 and wrs2["nlay"] > 0 and bytes(wrs2["data"][:4]) == b"WRS2"
    assert int(wrs2["data"][12:16].view("<u4")[0]) == (brick or 32)
    want, got = np.empty_like(f), np.empty_like(f)
    ctx.decode_host_seg(want, wrs1)
    ctx.decode_host_seg(got, wrs2)
    assert same_bits(got, want), shape
    want32, got32 = np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)
    ctx.decode_host_seg_f32(want32, wrs1)
    ctx.decode_host_seg_f32(got32, wrs2)
    assert same_bits(got32, want32), shape
    for level in range(5):
        assert all(same_bits(g, w) for g, w in zip(lowres_all_ways(ctx, shape, level, wrs2, 0), lowres_all_ways(ctx, shape, level, wrs1, 0))), (shape, level)
    for level in (0, 1):
        for roi in codec_regions(shape, level):
            assert all(same_bits(g, w) for g, w in zip(roi_all_ways(ctx, shape, level, roi, wrs2, 0), roi_all_ways(ctx, shape, level, roi, wrs1, 0))), (shape, level, roi)
