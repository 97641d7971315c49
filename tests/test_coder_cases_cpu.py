"""tests/coder_cases.py is what it claims to be.  A GPU test built on a table that misses its targets hides failures, so the
conditions on the table are checked here, without a GPU, with the host reference of the formats and the plain-Python coder
(tests/py_coder.py) alone: every case round-trips within the bounds, every kind keeps its defining property, the launch-edge
planes have the segment counts intended, the cases with short segments reach every branch of the encoder's carry handling, and
the fields of the codec-level GPU test carry the chosen plane through the quantizer."""
import math
import struct

import numpy as np
import pytest

import coder_cases as cc
import py_coder
from waverange_amd import api


def natural_decode(blob, n):
    return api.seg_decode_host_ref_blocked(blob, (1, 1, n), 0)


def stream_bound(bs):
    return bs + bs // 32 + 2 * 520 + 1024  # wrseg::stream_bound


# ---- the table itself -------------------------------------------------------------------------------------------------------
def test_table_holds_every_kind_strand_count_and_size():
    cases = cc.all_cases()
    ids = [cc.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids) == len(set(cases))
    grid = cc.grid()
    assert {seg for seg, _ in grid} == {16, 48, 512, 1008, 4096, 59904, 59984}
    for seg in cc.SEGS:
        assert {K for s, K in grid if s == seg} == {0} | {K for K in (1, 2, 4, 8, 16, 32) if 16 * K <= seg}, seg
    for seg, K in grid:
        mine = cc.stage_cases(seg, K)
        kinds = {c[0] for c in mine}
        # (a one_off position that no plane of this (seg, K) has room for is the only thing that may be missing)
        assert kinds >= {k for k in cc.KINDS if k != "floor256" and not k.startswith("one_off_")} | {"one_off_first_0", "one_off_last_0",
                                                                                                     "one_off_first_bs-1", "one_off_last_bs-1"}, (seg, K)
        assert ({"one_off_first_L", "one_off_last_L", "one_off_first_L-1"} <= kinds) == (cc.plane_K(seg, K) > 1), (seg, K)
        assert ("floor256" in kinds) == (seg >= 512), (seg, K)
        L = cc.strand_len(seg, cc.plane_K(seg, K))
        want = {seg - 1, seg + 17, 2 * seg + 7} if seg > 5000 else {1, 15, 16, 17, L - 1, L, L + 1, seg - 1, seg, seg + 1, seg + 17, 3 * seg + 7} - {0}
        for kind in ("uniform", "patchwork", "const_0", "adversarial_K-1_last"):
            assert {c[3] for c in mine if c[0] == kind} >= want, (seg, K, kind)
    print("%d cases, %d of them launch-edge planes; per (seg, K): %s" % (
        len(cases), sum(len(cc.edge_cases(*g)) for g in grid), " ".join("%d/%s:%d" % (s, K or "wrs1", len(cc.stage_cases(s, K))) for s, K in grid)))


def test_launch_edge_planes_have_the_segment_counts_intended():
    seen = set()
    for seg, K in cc.grid():
        edges = cc.edge_cases(seg, K)
        assert bool(edges) == (seg in (16, 48) or (seg, K) == (512, 32)), (seg, K)
        if not edges:
            continue
        per_wave = 64 // max(K, 1)
        counts = sorted({-(-c[3] // seg) for c in edges})
        assert counts == sorted({per_wave - 1, per_wave, per_wave + 1, 1023, 1024, 1025, 2049}), (seg, K, counts)
        for kind, _, _, n in edges:
            assert kind in ("patchwork", "uniform") and n % seg == seg - 5  # a short last segment
        assert {c[0] for c in edges} == {"patchwork", "uniform"}
        # the scan kernels' per = ceil(nseg / 1024) is 1, 2 and 3
        assert {nseg: -(-nseg // 1024) for nseg in counts if nseg > 1000} == {1023: 1, 1024: 1, 1025: 2, 2049: 3}
        seen.add((seg, K))
    assert (16, 0) in seen and (16, 1) in seen and (48, 2) in seen and (512, 32) in seen


def test_patchwork_puts_unlike_segments_side_by_side():
    names = [cc.patch_kind(k) for k in range(len(cc.PATCH))]
    pairs = set(zip(names, names[1:] + names[:1]))
    assert ("const_0", "uniform") in pairs and ("const_255", "uniform") in pairs and ("adversarial", "floor256") in pairs
    assert set(names) == {"const_0", "const_137", "const_255", "one_off", "alternate", "floor256", "ramp", "uniform", "narrow", "geometric", "adversarial"}
    # and the planes are that: segment by segment what the kind's rule gives
    seg, K = 512, 8
    L = cc.strand_len(seg, K)
    p = cc.plane("patchwork", 30 * seg - 5, seg, K)
    for k in range(30):
        s = p[k * seg:(k + 1) * seg]
        name = cc.patch_kind(k)
        if name.startswith("const_"):
            assert np.all(s == int(name[6:])), k
        elif name == "floor256":
            assert np.bincount(s, minlength=256)[1:].tolist() == [1] * 255 or s.size < 512, k
        elif name == "uniform":
            assert np.unique(s).size > 200, k
        elif name == "adversarial":
            j = (k // 12) % K
            assert np.all(s[:j * L] == 0) and np.all(s[(j + 1) * L:] == 0) and np.all(s[j * L:(j + 1) * L] > 0), k
    # a longer plane only appends: the launch-edge planes of different segment counts share their segments
    assert np.array_equal(cc.plane("patchwork", 40 * seg - 5, seg, K)[:29 * seg], p[:29 * seg])


# ---- every case on the host reference ------------------------------------------------------------------------------------------
def ideal_bits(sym, count, bs):
    """what the symbols cost under the segment's model: sum of log2(bs / count)"""
    c = count[sym].astype(np.float64)
    return float(np.sum(np.log2(bs / c)))


def check_strand_sizes(c, p, seg, K, recs):
    """Bounds of every record, and the defining property of the kinds that have one in terms of coded sizes.

    The issue's wording for an adversarial segment -- the strand takes more than 1.5 L bytes, every other strand under 20 --
    is the arithmetic of K = 32 at a long segment: a strand of m symbols that occur once each (or L / 255 times each) in a
    segment of bs costs m * log2(bs * max(1, 255 / m) / ... ) bits, above 12 bits per symbol only when bs / m > 16 and
    bs > 4096, and a zero strand of m symbols costs m * log2(bs / (bs - L)) bits, under 100 bits only for K = 32.  So the
    sizes are checked against the model's own entropy for every K -- no coder can beat it by more than its last bytes, and
    this one loses at most log2(129 / 128) bits per step (csrc/wr_segcoder.h) -- and literally, with the strand's own length m for L, where the arithmetic gives it:
    K = 32, a full segment of at least 4096 symbols."""
    kind, _, _, n = c
    L = cc.strand_len(seg, K)
    for k, (T, strands) in enumerate(recs):
        s0 = k * seg
        bs = min(seg, n - s0)
        s = p[s0:s0 + bs]
        count = np.bincount(s, minlength=256)
        top = int(np.flatnonzero(count)[-1])
        assert len(T) <= 520, (cc.case_id(c), k, len(T))
        for j, S in enumerate(strands):
            m = max(0, min(L, bs - j * L))
            if not m:
                assert S == b"", (cc.case_id(c), k, j)
                continue
            assert 5 <= len(S) <= 2 * m + 5, (cc.case_id(c), k, j, len(S), m)
            bits = ideal_bits(s[j * L:j * L + m], count, bs)
            # (the highest symbol of the segment also gets what range / tot leaves over, under tot out of a share of 128 sy at least)
            gain = np.count_nonzero(s[j * L:j * L + m] == top) * math.log2(1 + bs / (128.0 * count[top]))
            assert (bits - gain) / 8 - 4 <= len(S) <= (bits + 0.0113 * (m + 1) + 1.001) / 8 + 7, (cc.case_id(c), k, j, len(S), bits)
        if np.all(s == s[0]):  # a constant segment: its symbols cost nothing
            assert all(len(S) < 20 for S in strands), (cc.case_id(c), k)
    if kind.startswith("adversarial_"):
        _, jname, where = kind.split("_")
        k = 0 if where == "first" else len(recs) - 1
        bs = min(seg, n - k * seg)
        j = min({"0": 0, "K/2": K // 2, "K-1": K - 1}[jname], (bs - 1) // L)
        strands = recs[k][1]
        s = p[k * seg:k * seg + bs]
        m = min(L, bs - j * L)
        assert np.all(s[:j * L] == 0) and np.all(s[j * L + m:] == 0) and np.array_equal(s[j * L:j * L + m], 1 + np.arange(m) % 255)
        if K == 32 and bs == seg >= 4096:
            assert len(strands[j]) > 1.5 * m, (cc.case_id(c), len(strands[j]), m)  # (m < L only for the last strand of seg 59984)
            assert all(len(S) < 20 for i, S in enumerate(strands) if i != j), cc.case_id(c)
            return 1
    return 0


@pytest.mark.parametrize("seg,K", cc.grid(), ids=lambda v: str(v))
def test_every_case_round_trips_within_the_bounds(seg, K):
    literal = 0
    for c in cc.stage_cases(seg, K):
        kind, _, _, n = c
        p = cc.case_plane(c)
        assert p.size == n and p.dtype == np.uint8
        if K == 0:
            blob = api.seg_encode_host_ref(p, seg)
            assert blob.size <= api.seg_bound(n, seg), cc.case_id(c)
            assert np.array_equal(api.seg_decode_host_ref(blob, n), p), cc.case_id(c)
            got_seg, streams = api.seg_split(blob)
            assert got_seg == seg and len(streams) == -(-n // seg)
            for k, s in enumerate(streams):
                bs = min(seg, n - k * seg)
                assert len(s) <= stream_bound(bs), (cc.case_id(c), k)
                part = p[k * seg:k * seg + bs]
                if np.all(part == part[0]):
                    # a constant segment: the 256 counts cost 16 bits each whatever they are, its symbols nothing
                    assert 512 < len(s) < 512 + 20, (cc.case_id(c), k, len(s))
        else:
            blob = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
            assert blob.size <= api.seg_bound_strands(n, seg, K), cc.case_id(c)
            assert np.array_equal(natural_decode(blob, n), p), cc.case_id(c)
            got = api.seg_split_strands(blob)
            assert got[:3] == (seg, 0, K) and len(got[3]) == -(-n // seg)
            literal += check_strand_sizes(c, p, seg, K, got[3])
        if kind == "floor256":
            for s0 in range(0, n, seg):
                count = np.bincount(p[s0:s0 + seg], minlength=256)
                if min(seg, n - s0) >= 512:
                    assert np.count_nonzero(count) == 256 and np.count_nonzero(count == 1) == 255, cc.case_id(c)
                else:
                    assert count[0] == min(seg, n - s0)
            assert n >= 512  # (at least the first segment has the floor)
        if kind.startswith("one_off_"):
            assert np.count_nonzero(p) == 1 and p.max() == 255, cc.case_id(c)
    if K == 32 and seg >= 4096:
        assert literal >= 3, (seg, K, literal)  # the three strands of the first full segment at least


# ---- the restatement and the branches it reaches ---------------------------------------------------------------------------------
_MEMO = {}


def py_record(s, seg, K):
    """py_coder's record (K > 0) or WRS1 segment stream (K == 0) of one segment, with what it added to the counters; the
    launch-edge planes repeat their segments, and a repeated segment is coded once"""
    key = (s.tobytes(), seg, K)
    if key not in _MEMO:
        before = dict(py_coder.COUNTS)
        py_coder.reset_counts()
        out = py_coder.py_record(s, seg, K) if K else py_coder.py_wrs1_segment(s)
        _MEMO[key] = (out, dict(py_coder.COUNTS))
        for k, v in before.items():
            py_coder.COUNTS[k] = max(v, py_coder.COUNTS[k]) if k.startswith("max_") else v + py_coder.COUNTS[k]
    return _MEMO[key][0]


def py_case_blob(p, seg, K):
    n = p.size
    nseg = -(-n // seg)
    recs = [py_record(p[k * seg:min(n, (k + 1) * seg)], seg, K) for k in range(nseg)]
    head = b"WRS3" + struct.pack("<IIII", seg, nseg, 0, K) if K else b"WRS1" + struct.pack("<II", seg, nseg)
    return head + b"".join(struct.pack("<I", len(r)) for r in recs) + b"".join(recs)


def host_blob(p, seg, K):
    return api.seg_encode_host_ref_strands(p, seg=seg, strands=K) if K else api.seg_encode_host_ref(p, seg)


REQUIRED = {"out": 1, "carry": 1, "pend": 1, "finish_carry": 1, "finish_plain": 1, "max_ff": 2, "max_00": 2}


def test_restatement_equals_the_host_reference_and_every_branch_is_taken(capsys):
    """The cases with seg <= 512, byte for byte as test_host_ref_is_the_definition demands for its own;
    beside the bytes, which arms of Enc::renorm and Enc::finish these cases take and how long the pending runs get."""
    py_coder.reset_counts()
    _MEMO.clear()
    per_group, ncases = {}, 0
    for seg, K in cc.grid():
        if seg > 512:
            continue
        mark = dict(py_coder.COUNTS)
        for c in cc.stage_cases(seg, K):
            p = cc.case_plane(c)
            assert py_case_blob(p, seg, K) == host_blob(p, seg, K).tobytes(), cc.case_id(c)
            ncases += 1
        per_group[(seg, K)] = {k: (v if k.startswith("max_") else v - mark[k]) for k, v in py_coder.COUNTS.items()}
    names = list(py_coder.COUNTS)
    with capsys.disabled():
        print("\nbranch counters of the plain-Python coder over %d cases with seg <= 512 (max_*: running maximum)" % ncases)
        print("%12s " % "seg/K" + " ".join("%12s" % k for k in names))
        for (seg, K), row in per_group.items():
            print("%12s " % ("%d/%s" % (seg, K or "wrs1")) + " ".join("%12d" % row[k] for k in names))
        print("%12s " % "all" + " ".join("%12d" % py_coder.COUNTS[k] for k in names))
    # every arm is reached by the table as it stands: no seed had to be searched for, and none is listed as unreached
    for k, need in REQUIRED.items():
        assert py_coder.COUNTS[k] >= need, (k, py_coder.COUNTS[k], need)


# ---- the fields of the codec-level GPU test --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.CODEC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codec_fields_carry_the_chosen_plane(oracle, shape):
    """wtflag = 0: no transform, and plane 0 is the quantizer's cut of the field itself.  A field of the integers 0..255 that
    holds both 0 and 255 has deps = 1 and minval = 0 exactly, so q = (uint8)(x + 0.5) = x: plane 0 is the chosen plane.  A
    constant plane cannot be carried -- a constant field codes no plane at all -- so const_v is not in CODEC_KINDS."""
    n = int(np.prod(shape))
    assert not any(k.startswith("const_") for k in cc.CODEC_KINDS)
    for brick in cc.CODEC_BRICKS:
        pi = api.blocked_order(shape, 0, brick).astype(np.int64) if brick else None
        for seg in cc.CODEC_SEGS:
            for K in cc.CODEC_KS:
                for kind in cc.CODEC_KINDS:
                    want = cc.codec_plane(kind, n, seg, K or 0)
                    f = cc.codec_field(want, shape, pi)
                    assert f.shape == shape and f.dtype == np.float64
                    enc = oracle.encode(f.copy(), 1e-3, wtflag=0)
                    assert enc["nlay"] >= 1 and enc["deps_vec"][0] == 1.0 and enc["minval_vec"][0] == 0.0, (kind, seg, K, brick)
                    plane0, got = oracle.range_decode(enc["data"][:int(enc["len_enc_vec"][0])], n)
                    assert got == n
                    stream_order = plane0[:n] if pi is None else plane0[:n][pi]
                    assert np.array_equal(stream_order, want), (kind, seg, K, brick)
                    # the defining property, in the order the coder sees
                    if kind.startswith("adversarial_"):
                        _, jname, where = kind.split("_")
                        Kp = cc.plane_K(seg, K or 0)
                        L = cc.strand_len(seg, Kp)
                        s0, bs = cc.segment_of(n, seg, where)
                        j = min({"0": 0, "K/2": Kp // 2, "K-1": Kp - 1}[jname], (bs - 1) // L)
                        s = stream_order[s0:s0 + bs]
                        m = min(L, bs - j * L)
                        rest = np.concatenate((s[:j * L], s[j * L + m:]))
                        assert np.all(s[j * L:j * L + m - 1] == 1 + np.arange(m - 1) % 255) and np.count_nonzero(rest) == 0
