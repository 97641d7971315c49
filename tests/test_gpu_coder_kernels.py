"""The segment coder's kernel entry points against each other (csrc/wr_segcoder.hip, csrc/wr_segbatch.hip): the plane launch,
the batch launch and the list launches run the same lane programs (csrc/wr_segcoder_dev.h), so for the same plane they give the
same bytes, and all of them the host coder's.  Stage level, symbol planes made with numpy, every comparison an equality.

Shapes: seg = 16 (the minimum) and 1008; n = 65 * seg - 5 (two waves, the second with one live lane, and a short last
segment), n = seg, n = 7 (one segment shorter than 16 symbols; with 32 strands all but the first strand are empty).  WRS3 takes
seg = 1008 only: a stranded stream needs 16 * K <= seg.  Random planes give streams of odd lengths, so the gather's
destinations hit all four alignments; a constant and a two-symbol plane give the shortest streams.

What the stage entry points do not show is not asserted.  The encoders take no brick, and wr_dev_seg_decode and
wr_dev_seg_decode_batch read no WRS2 blob, so WRS2 (whose header is all that differs) goes through the list decoder only,
with the host coder's blob.
The decoders return a job's count of failed segments, not the flag words, so a failed segment is compared by that count, the
return code, the message and the symbols it left behind."""
import numpy as np
import pytest

from waverange_amd import api

pytestmark = pytest.mark.gpu

C = api.C
BAND, FILL = 256, 0xA5
SEGS = (16, 1008)
SEG3 = 1008
STRANDS = (2, 8, 32)
KINDS = ("random", "constant", "two")
ERR_STREAM, ERR_OVERFLOW = -4, -5


def sizes(seg):
    return (65 * seg - 5, seg, 7)


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


_PLANES, _HOST = {}, {}


def plane(kind, n):
    if (kind, n) not in _PLANES:
        rng = np.random.default_rng(1000 * KINDS.index(kind) + n % 997)
        p = {"random": lambda: rng.integers(0, 256, n), "constant": lambda: np.full(n, 7),
             "two": lambda: rng.choice([3, 200], n)}[kind]().astype(np.uint8)
        p.flags.writeable = False
        _PLANES[(kind, n)] = p
    return _PLANES[(kind, n)]


def host_blob(kind, n, seg, K=0, brick=0):
    """the host coder's blob of a plane: computed once, shared, never written to.  brick: the WRS2 blob whose stream order is
    the plane as it stands (the stage decoders give the symbols in stream order)"""
    key = (kind, n, seg, K, brick)
    if key not in _HOST:
        p = plane(kind, n)
        if K:
            b = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
        else:
            b = api.seg_encode_host_ref(p, seg)
            if brick:  # the WRS1 blob with the longer header: magic, seg, nseg, brick
                b = np.concatenate([np.frombuffer(b"WRS2", np.uint8), b[4:12], np.array([brick], "<u4").view(np.uint8), b[12:]])
        b.flags.writeable = False
        _HOST[key] = b
    return _HOST[key]


def front_of(blob):
    """(bytes in front of the segments, their lengths)"""
    head = {b"WRS1": 12, b"WRS2": 16, b"WRS3": 20}[bytes(blob[:4])]
    nseg = int(blob[8:12].view("<u4")[0])
    return head + 4 * nseg, blob[head:head + 4 * nseg].view("<u4").astype(np.int64)


def up16(v):
    return (v + 15) & ~15


class Banded:
    """device memory of BAND | room rounded up to 16 | BAND bytes, all FILL except `payload` at BAND"""

    def __init__(self, ctx, payload, room):
        self.image = np.full(BAND + up16(max(room, 16)) + BAND, FILL, np.uint8)
        self.image[BAND:BAND + payload.size] = payload
        self.buf = ctx.to_device(self.image)
        self.ptr = self.buf.ptr + BAND

    def read(self):
        return self.buf.download(np.uint8, self.image.size)

    def free(self):
        self.buf.free()


def arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def encode(ctx, how, planes, seg, K=0, caps=None):
    """how: "single" (one call per plane; wr_dev_seg_encode, or _strands with K) | "batch" (one call).  caps: the room per
    blob instead of the bound.  Returns (return codes -- the batch's one code for every job --, reported lengths with
    2^64 - 1 where none was reported, the blob buffers' contents behind the leading band)."""
    lib = api.lib()
    n = planes[0].size
    bound = api.seg_bound_strands(n, seg, K) if K else api.seg_bound(n, seg)
    caps = [bound] * len(planes) if caps is None else caps
    syms = [Banded(ctx, p, n) for p in planes]
    blobs = [Banded(ctx, np.zeros(0, np.uint8), bound) for _ in planes]
    none = 2 ** 64 - 1
    try:
        if how == "batch":
            assert not K
            got = arr(C.c_size_t, [none] * len(planes))
            rc = lib.wr_dev_seg_encode_batch(ctx.h, len(planes), arr(C.c_void_p, [s.ptr for s in syms]), n, seg, arr(C.c_void_p, [b.ptr for b in blobs]),
                                             arr(C.c_size_t, caps), got)
            rcs, lens = [rc] * len(planes), [int(got[j]) for j in range(len(planes))]
        else:
            rcs, lens = [], []
            for s, b, cap in zip(syms, blobs, caps):
                got = C.c_size_t(none)
                if K:
                    rcs.append(lib.wr_dev_seg_encode_strands(ctx.h, s.ptr, n, seg, K, b.ptr, cap, C.byref(got)))
                else:
                    rcs.append(lib.wr_dev_seg_encode(ctx.h, s.ptr, n, seg, b.ptr, cap, C.byref(got)))
                lens.append(int(got.value))
        outs = []
        for s, b in zip(syms, blobs):
            out = b.read()
            assert np.all(out[:BAND] == FILL) and np.all(out[BAND + up16(bound):] == FILL), (how, "the blob's bands")
            assert np.array_equal(s.read(), s.image), (how, "the encoder wrote symbols")
            outs.append(out[BAND:BAND + up16(bound)])
        return rcs, lens, outs
    finally:
        for x in syms + blobs:
            x.free()


def decode(ctx, how, blobs, ns, lists=None):
    """how: "single" (wr_dev_seg_decode per blob) | "batch" (wr_dev_seg_decode_batch, one n) | "lists" | "mixed"
    (wr_dev_seg_decode_lists, _mixed with the ascending segment ids lists[j]).  Every plane is prefilled with FILL.  Returns
    (return codes, failed segments per job, the planes, the messages)."""
    lib = api.lib()
    nj = len(blobs)
    dblobs = [Banded(ctx, b, b.size) for b in blobs]
    syms = [Banded(ctx, np.zeros(0, np.uint8), n) for n in ns]
    try:
        bp, sp = arr(C.c_void_p, [d.ptr for d in dblobs]), arr(C.c_void_p, [s.ptr for s in syms])
        ln = arr(C.c_size_t, [b.size for b in blobs])
        bad = arr(C.c_size_t, [0] * nj)
        if how == "single":
            rcs, msgs = [], []
            for j in range(nj):
                one = C.c_size_t(0)
                rcs.append(lib.wr_dev_seg_decode(ctx.h, dblobs[j].ptr, blobs[j].size, syms[j].ptr, ns[j], C.byref(one)))
                msgs.append(lib.wr_last_error().decode() if rcs[-1] else "")
                bad[j] = one.value
        else:
            if how == "batch":
                assert len(set(ns)) == 1
                rc = lib.wr_dev_seg_decode_batch(ctx.h, nj, bp, ln, sp, ns[0], bad)
            else:
                ls = [np.ascontiguousarray(l, dtype=np.uint32) for l in lists]
                fn = lib.wr_dev_seg_decode_lists if how == "lists" else lib.wr_dev_seg_decode_lists_mixed
                rc = fn(ctx.h, nj, bp, ln, sp, arr(C.c_size_t, [int(n) for n in ns]), arr(C.c_void_p, [l.ctypes.data if l.size else None for l in ls]),
                        arr(C.c_size_t, [l.size for l in ls]), bad)
            rcs, msgs = [rc] * nj, [lib.wr_last_error().decode() if rc else ""] * nj
        outs = []
        for d, s, n in zip(dblobs, syms, ns):
            out = s.read()
            assert np.all(out[:BAND] == FILL) and np.all(out[BAND + n:] == FILL), (how, "the symbols' bands")
            assert np.array_equal(d.read(), d.image), (how, "the decoder wrote to the blob")
            outs.append(out[BAND:BAND + n])
        return rcs, [int(bad[j]) for j in range(nj)], outs, msgs
    finally:
        for x in dblobs + syms:
            x.free()


# ---- encode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seg", SEGS)
def test_encode_plane_and_batch_launch_agree(ctx, seg):
    """the single launch, a batch of one and position j of a batch of three different planes: one blob, the host coder's"""
    for n in sizes(seg):
        planes, want = [plane(k, n) for k in KINDS], [host_blob(k, n, seg) for k in KINDS]
        rcs3, lens3, three = encode(ctx, "batch", planes, seg)
        for j, kind in enumerate(KINDS):
            rc1, len1, single = encode(ctx, "single", [planes[j]], seg)
            rcb, lenb, one = encode(ctx, "batch", [planes[j]], seg)
            for what, rc, ln, out in (("single", rc1[0], len1[0], single[0]), ("batch of one", rcb[0], lenb[0], one[0]), ("batch of three", rcs3[j], lens3[j], three[j])):
                assert rc == 0 and ln == want[j].size, (what, kind, n, rc, ln, want[j].size)
                assert np.array_equal(out[:ln], want[j]), (what, kind, n)
                assert np.all(out[ln:] == FILL), (what, kind, n, "bytes behind the blob")


@pytest.mark.parametrize("K", STRANDS)
def test_encode_strands_launch(ctx, K):
    for n in sizes(SEG3):
        for kind in KINDS:
            want = host_blob(kind, n, SEG3, K)
            rc, ln, out = encode(ctx, "single", [plane(kind, n)], SEG3, K)
            assert rc[0] == 0 and ln[0] == want.size, (kind, n, rc, ln, want.size)
            assert np.array_equal(out[0][:ln[0]], want) and np.all(out[0][ln[0]:] == FILL), (kind, n)


def test_encode_cap_one_short(ctx):
    """every launcher refuses alike, reports no length, writes the header and the index and nothing behind them"""
    for seg, K, how in ((16, 0, "single"), (16, 0, "batch"), (1008, 0, "single"), (1008, 0, "batch"), (SEG3, 2, "single"), (SEG3, 32, "single")):
        n = 65 * seg - 5
        want = host_blob("random", n, seg, K)
        front, _ = front_of(want)
        rc, ln, out = encode(ctx, how, [plane("random", n)], seg, K, caps=[want.size - 1])
        assert rc[0] == ERR_OVERFLOW and ln[0] == 2 ** 64 - 1, (seg, K, how, rc, ln)
        assert "too small for the plane" in api.lib().wr_last_error().decode()
        assert np.array_equal(out[0][:front], want[:front]), (seg, K, how, "header and index")
        assert np.all(out[0][front:] == FILL), (seg, K, how, "bytes behind the index")
    # in a batch of three the short job alone is refused; its neighbours' blobs are whole
    seg, n = 16, 65 * 16 - 5
    want = [host_blob(k, n, seg) for k in KINDS]
    rc, ln, out = encode(ctx, "batch", [plane(k, n) for k in KINDS], seg, caps=[want[0].size, want[1].size - 1, want[2].size])
    assert rc[0] == ERR_OVERFLOW and "job 1: " in api.lib().wr_last_error().decode()
    assert ln == [want[0].size, 2 ** 64 - 1, want[2].size]
    front, _ = front_of(want[1])
    assert np.array_equal(out[0][:want[0].size], want[0]) and np.array_equal(out[2][:want[2].size], want[2])
    assert np.array_equal(out[1][:front], want[1][:front]) and np.all(out[1][front:] == FILL)


# ---- decode -----------------------------------------------------------------------------------------------------------------------

def formats():
    return [(seg, 0, 0) for seg in SEGS] + [(16, 0, 16), (1008, 0, 16)] + [(SEG3, K, 0) for K in STRANDS]


FORMAT_IDS = ["seg%d-%s" % (seg, "K%d" % K if K else "wrs2" if brick else "wrs1") for seg, K, brick in formats()]


def subsets(nseg):
    """the full list; the first segment alone; the last (short) one alone; every other one"""
    return [np.arange(nseg), np.array([0]), np.array([nseg - 1]), np.arange(0, nseg, 2)]


def expected(p, seg, ids):
    want = np.full(p.size, FILL, np.uint8)
    for k in ids:
        want[k * seg:(k + 1) * seg] = p[k * seg:(k + 1) * seg]
    return want


@pytest.mark.parametrize("seg,K,brick", formats(), ids=FORMAT_IDS)
def test_decode_launches_agree(ctx, seg, K, brick):
    """plane launch (WRS1 / WRS3), batch launch (WRS1) and list launch (all formats) with the full list: the plane, no failed segment.  A list of
    a subset leaves every other byte of the prefilled plane alone; a job with an empty list stands beside a full one."""
    lists_how = "mixed" if K else "lists"
    for n in sizes(seg):
        nseg = (n + seg - 1) // seg
        blobs, planes = [host_blob(k, n, seg, K, brick) for k in KINDS], [plane(k, n) for k in KINDS]
        runs = [] if brick else [("single", decode(ctx, "single", blobs, [n] * 3))]
        if not K and not brick:
            runs.append(("batch", decode(ctx, "batch", blobs, [n] * 3)))
        runs.append((lists_how, decode(ctx, lists_how, blobs, [n] * 3, [np.arange(nseg)] * 3)))
        for how, (rcs, bad, outs, _) in runs:
            assert rcs == [0] * 3 and bad == [0] * 3, (how, n, rcs, bad)
            for kind, out, p in zip(KINDS, outs, planes):
                assert np.array_equal(out, p), (how, kind, n)
        for ids in subsets(nseg)[1:]:
            rcs, bad, outs, _ = decode(ctx, lists_how, blobs[:1] * 2, [n] * 2, [ids, np.zeros(0, np.uint32)])
            assert rcs == [0, 0] and bad == [0, 0], (n, ids[:4], rcs, bad)
            assert np.array_equal(outs[0], expected(planes[0], seg, ids)), (n, ids[:4])
            assert np.all(outs[1] == FILL), (n, "the job with the empty list")
        # the empty list in front of a full one
        rcs, bad, outs, _ = decode(ctx, lists_how, blobs[:2], [n] * 2, [np.zeros(0, np.uint32), np.arange(nseg)])
        assert rcs == [0, 0] and bad == [0, 0] and np.all(outs[0] == FILL) and np.array_equal(outs[1], planes[1]), n


def test_decode_lists_mixed_strand_counts(ctx):
    """K = 2 and K = 32 jobs, a WRS1 job between them, in one call: two launches, every job its own subset"""
    n = 65 * SEG3 - 5
    nseg = 65
    p = plane("random", n)
    blobs = [host_blob("random", n, SEG3, 2), host_blob("random", n, SEG3), host_blob("random", n, SEG3, 32), host_blob("random", n, SEG3, 2)]
    for lists in ([subsets(nseg)[i] for i in (3, 2, 1, 0)], [subsets(nseg)[i] for i in (2, 0, 3, 1)]):
        rcs, bad, outs, _ = decode(ctx, "mixed", blobs, [n] * 4, lists)
        assert rcs == [0] * 4 and bad == [0] * 4, (rcs, bad)
        for out, ids in zip(outs, lists):
            assert np.array_equal(out, expected(p, SEG3, ids)), ids[:4]


@pytest.mark.parametrize("seg,K,brick", formats(), ids=FORMAT_IDS)
def test_decode_altered_payload(ctx, seg, K, brick):
    """One payload byte of one segment altered: the bounded decoder's ordinary refusal -- or another plane -- and the same from
    the plane launch, the batch launch and the list launch: return code, message, failed segments, every byte of the plane."""
    n = 65 * seg - 5
    good = host_blob("two", n, seg, K, brick)
    front, lens = front_of(good)
    starts = front + np.concatenate([[0], np.cumsum(lens)])
    results = []
    # segment 3's and the last segment's counts (their sum is no longer the segment's length: refused before a symbol), a byte
    # of segment 20's symbols (whatever it does), and for a record its first length word
    cases = [(3, 4 * (K + 1) + 10 if K else 10), (64, 4 * (K + 1) + 10 if K else 10), (20, int(lens[20]) - 8)] + ([(40, 0)] if K else [])
    for k, off in cases:
        blob = good.copy()
        blob[int(starts[k]) + off] ^= 0x5A
        runs = [] if brick else [decode(ctx, "single", [blob], [n])]
        if not K and not brick:
            runs.append(decode(ctx, "batch", [blob], [n]))
        runs.append(decode(ctx, "mixed" if K else "lists", [blob], [n], [np.arange(65)]))
        rcs, bad, outs, msgs = runs[0]
        assert rcs[0] in (0, ERR_STREAM) and (bad[0] > 0) == (rcs[0] == ERR_STREAM), (k, rcs, bad)
        assert bad[0] <= 1, (k, bad)
        untouched = np.ones(n, bool)
        untouched[k * seg:(k + 1) * seg] = False
        assert np.array_equal(outs[0][untouched], plane("two", n)[untouched]), (k, "another segment's symbols")
        for other in runs[1:]:
            assert other[0] == rcs and other[1] == bad, (k, other[0], rcs, other[1], bad)
            assert np.array_equal(other[2][0], outs[0]), k
            assert [m.replace("job 0: ", "") for m in other[3]] == [m.replace("job 0: ", "") for m in msgs], (k, other[3], msgs)
        results.append(bad[0])
    assert results[0] == 1 and results[1] == 1, "altered counts were not refused"
