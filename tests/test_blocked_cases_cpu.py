"""The table of tests/blocked_cases.py without a GPU: every case's plan (wr_reorder_plan) against the table and against the
geometry the module restates from the format text, the classes the table must reach, that geometry against wr_blocked_order
(which is what entitles tests/test_gpu_blocked_cases.py to use its brick ranges as the reference), and the refusals.
Everything here is integers."""
import ctypes as C

import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the repository on sys.path)
import blocked_cases as bc
from test_gpu_blocked import BRICK_OF, REORDER
from waverange_amd import api

WR_ERR_ARG = -1
KEYS = list(bc.CASES)
ids_of = lambda k: "%s-w%d-b%d" % ("x".join(map(str, k[0])), k[1], k[2])  # noqa: E731


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_plan_is_the_table_and_the_geometry(key):
    shape, wlev, B = key
    plans = bc.check_plan(api, key)
    boxes, bricks = bc.boxes_of(shape, wlev), bc.bricks_of(shape, wlev, B)
    for mode, plan in plans.items():
        group = plan["group"]
        assert plan["nbricks"] == len(bricks) and len(plan["boxes"]) == len(boxes), (key, mode)
        first = 0
        for i, ((o, e), b) in enumerate(zip(boxes, plan["boxes"])):
            mine = [x for x in bricks if x.box == i]
            nt = tuple(-(-v // B) for v in e)
            assert (b["origin"], b["extent"], b["bricks"]) == (o, e, nt), (key, mode, i)
            assert (b["first"], b["first_brick"], b["start"]) == (first, mine[0].id, mine[0].start), (key, mode, i)
            assert len(mine) == nt[0] * nt[1] * nt[2]
            # the rule, restated: B >= 16 and the origin and extent in x, nx and the start are multiples of 16
            assert b["wide"] == (B >= 16 and shape[2] % 16 == 0 and o[0] % 16 == 0 and e[0] % 16 == 0 and mine[0].start % 16 == 0), (key, mode, i)
            first += -(-nt[0] // group) * nt[1] * nt[2]
        assert plan["items"] == first, (key, mode)
    if wlev and B >= 16:
        assert bc.both_widths_in_one_launch(plans["whole"]), key
    else:
        assert len(plans["whole"]["boxes"]) == 1 or B == 8, key
    assert shape[0] * shape[1] * shape[2] <= 1 << 20, key


def test_required_classes_are_reached():
    reached = set()
    for key in KEYS:
        shape, wlev, B = key
        got = bc.reached(shape, wlev, B, bc.check_plan(api, key))
        assert got - reached, (key, "adds nothing to the cases before it")
        reached |= got
    assert bc.REQUIRED <= reached, sorted(bc.REQUIRED - reached)
    # the three that REQUIRED leaves out as unreachable are not reached
    assert not reached & {"list/B16/wide/zloop", "list/B16/wide/partial1", "whole/B16/wide/partial1"}


def old_suite(chunked=False):
    """What tests/test_gpu_blocked.py sends through the kernel, classified: REORDER at both depths and the two planes of its
    defaults test in whole mode; every brick of the planes of its region and low-resolution tests -- the upper bound of their
    lists -- in list mode.  chunked: also the 128^3 planes of its child process that runs with planes in two chunks."""
    out = set()
    for shape, B in REORDER:
        for wlev in (0, 4):
            out |= bc.reached(shape, wlev, B, {"whole": api.reorder_plan(shape, wlev, B)})
    for shape, B in [((40, 48, 64), 32), ((40, 48, 64), 64)] + ([((128, 128, 128), 32), ((128, 128, 128), 8)] if chunked else []):
        out |= bc.reached(shape, 4, B, {"whole": api.reorder_plan(shape, 4, B)})
    for shape, B in list(BRICK_OF.items()) + ([((128, 128, 128), 32), ((128, 128, 128), 8)] if chunked else []):
        out |= bc.reached(shape, 4, B, {"list": api.reorder_plan(shape, 4, B, list=True)})
    return out | bc.reached((77, 129, 200), 0, 16, {"list": api.reorder_plan((77, 129, 200), 0, 16, list=True)})


def test_what_the_older_lists_reach():
    """what of REQUIRED the planes of tests/test_gpu_blocked.py do not reach, all of it on the wide path: why the table exists"""
    old = old_suite()
    at = lambda prefix: {f.rsplit("/", 1)[1] for f in old if f.startswith(prefix)}  # noqa: E731
    # the byte-path requirements are what REORDER reaches in whole mode at bricks 8 and 32
    assert at("whole/B8/byte/") == set(bc.BYTE_WHOLE_8) and at("whole/B32/byte/") == set(bc.BYTE_WHOLE_32)
    missing = bc.REQUIRED - old
    assert all("/wide/" in f for f in missing), sorted(f for f in missing if "/wide/" not in f)
    # no full 128-byte group, no gx > 0 and no whole brick on the wide path at any brick; nothing wide by list beyond brick 16
    for B in (16, 32, 64):
        assert {"whole/B%d/wide/%s" % (B, n) for n in ("full", "gx>0", "whole_brick")} <= missing, B
    assert not at("list/B32/wide/") and not at("list/B64/wide/") and not at("whole/B64/wide/yloop")
    assert {"whole/B32/wide/partialN", "whole/B64/wide/partialN", "whole/B64/wide/short", "whole/B64/wide/yloop"} <= missing
    assert len(missing) == 32, sorted(missing)
    # the child process of test_planes_that_span_two_chunks decodes a region and the low-resolution boxes of a 128^3 plane at
    # brick 32: with every brick of that plane as the upper bound of its lists, brick 32 by list is no longer unreached, the
    # rest is
    more = bc.REQUIRED - old_suite(chunked=True)
    assert missing - more == {"list/B32/wide/%s" % n for n in ("full", "whole_brick", "partial1", "gx>0", "hy<B", "hz<B", "zloop")}


@pytest.mark.parametrize("key", KEYS, ids=ids_of)
def test_brick_ranges_are_the_order(key):
    """every brick's stream range maps under wr_blocked_order exactly onto the brick's coordinate box, x fastest"""
    shape, wlev, B = key
    pi = api.blocked_order(shape, wlev, B).astype(np.int64)
    at = 0
    for b in bc.bricks_of(shape, wlev, B):
        assert b.start == at
        at += b.h[0] * b.h[1] * b.h[2]
        assert np.array_equal(pi[b.start:at], bc.brick_points(shape, b)), (key, b)
    assert at == pi.size
    lists = bc.brick_lists(shape, wlev, B)
    assert set(lists) == {"all", "every-second", "box-ends", "one"}
    for name, ids in lists.items():
        assert ids and list(ids) == sorted(set(ids)) and ids[-1] < at, (key, name)


def test_refusals():
    fn = api.lib().wr_reorder_plan
    plan = api.ReorderPlan()

    def refused(dims=(64, 64, 64), wlev=4, brick=32, lst=0):
        plan.nbox = plan.group = -7  # a refused call leaves the plan alone
        return fn(*dims, wlev, brick, lst, C.byref(plan)) == WR_ERR_ARG and (plan.nbox, plan.group) == (-7, -7)

    assert fn(64, 64, 64, 4, 32, 0, C.byref(plan)) == 0 and (plan.nbox, plan.group, plan.items, plan.nbricks) == (29, 4, 29, 29)
    assert fn(64, 64, 64, 4, 0, 1, C.byref(plan)) == 0 and (plan.nbox, plan.group, plan.items, plan.nbricks) == (29, 1, 29, 29)  # brick 0: 32
    assert fn(64, 64, 64, 4, 32, 0, None) == WR_ERR_ARG
    assert "out is NULL" in api.lib().wr_last_error().decode()
    # what wr_dev_plane_reorder refuses (tests/test_gpu_blocked.py::test_plane_reorder_defaults_and_refusals)
    for wlev, brick in ((4, 12), (4, 128), (3, 32), (4, 7), (-1, 32), (5, 8)):
        assert refused(wlev=wlev, brick=brick) and refused(wlev=wlev, brick=brick, lst=1), (wlev, brick)
        with pytest.raises(api.WaveRangeError):
            api.reorder_plan((64, 64, 64), wlev, brick)
    for dims in ((0, 64, 64), (64, -1, 64), (64, 64, 0)):
        assert refused(dims=dims), dims
    assert not refused() and not refused(wlev=0, brick=64, lst=1)
