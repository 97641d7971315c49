"""The planes that break coders: the case table of the segment and strand coder kernels (csrc/wr_segcoder.hip).  It plays for
them the role that fused_cases.py plays for the fused transform.  Pure numpy and seeded; nothing of the library is imported.
tests/test_coder_cases_cpu.py asserts that the table is what it claims to be, tests/test_gpu_coder_cases.py runs it on the card.

A case is the tuple (kind, seg, K, n): a plane of n symbols of that kind, coded with segments of `seg` symbols as WRS1 (K = 0)
or as WRS3 with K strands.  The plane is plane(kind, n, seg, K): kinds that speak of strands ("one_off", "adversarial") use
L = strand_len(seg, K), and for a WRS1 case the strands of plane_K(seg), so that WRS1 meets the same lopsided segments.
case_id() gives the readable id."""
import numpy as np

SEGS = [16, 48, 512, 1008, 4096, 59904, 59984]
KS = [1, 2, 4, 8, 16, 32]


def seg_ok(seg):
    return 16 <= seg <= 59999 and seg % 16 == 0


def strands_ok(K, seg):
    return 1 <= K <= 32 and K & (K - 1) == 0 and 16 * K <= seg


def strand_len(seg, K):
    return 16 * ((seg + 16 * K - 1) // (16 * K))


def plane_K(seg, K=0):
    """the strand count that a plane is built for: K, or for a WRS1 case the largest valid one up to 8"""
    return K or max(k for k in (1, 2, 4, 8) if strands_ok(k, seg))


def seed_of(seg, n):
    """planes of more than four segments share a seed: the launch-edge planes of different lengths then repeat their segments
    (numpy's generators deal a longer array out as a continuation of a shorter one), and the CPU check codes each once"""
    return 1000 * seg + (n if n <= 4 * seg else 0)


# ---- one segment of a kind -------------------------------------------------------------------------------------------------
# (bs, L, rng, j) -> bs symbols.  These are what "patchwork" deals out segment by segment; most plane kinds are the same rule
# applied to the whole plane instead.
def _const(v):
    return lambda bs, L, rng, j: np.full(bs, v, np.uint8)


def _one_off(bs, L, rng, j):
    p = np.zeros(bs, np.uint8)
    p[min(L, bs) - 1] = 255
    return p


def _alternate(bs, L, rng, j):
    return ((np.arange(bs) & 1) * 255).astype(np.uint8)


def _floor256(bs, L, rng, j):
    """every symbol 1..255 exactly once, scattered, 0 everywhere else; a segment shorter than 512 is all zero"""
    p = np.zeros(bs, np.uint8)
    if bs >= 512:
        p[rng.permutation(bs)[:255]] = np.arange(1, 256)
    return p


def _ramp(bs, L, rng, j):
    return (np.arange(bs) % 251).astype(np.uint8)


def _uniform(bs, L, rng, j):
    return rng.integers(0, 256, bs, dtype=np.uint8)


def _narrow(bs, L, rng, j):
    return rng.integers(0, 256, bs, dtype=np.uint8) & 7


def _geometric(bs, L, rng, j):
    return np.minimum(rng.geometric(0.3, bs), 255).astype(np.uint8)


def _adversarial(bs, L, rng, j):
    """0 except strand j (the last non-empty one if j is past it), which is 1 + i % 255: the construction of
    test_adversarial_strand_stays_within_the_bound"""
    p = np.zeros(bs, np.uint8)
    j = min(j, (bs - 1) // L)
    m = min(L, bs - j * L)
    p[j * L:j * L + m] = 1 + np.arange(m) % 255
    return p


# The order matters to "patchwork": segment k is entry k % 12 of this list, so a constant segment sits directly beside a uniform
# one (0 | 1, 6 | 7) and an adversarial one beside a floor256 one (2 | 3), and the 64 lanes of a wave hold different models and
# stream lengths from under 20 bytes to near the bound.  The adversarial strand moves on by one every 12 segments.
PATCH = [("const_0", _const(0)), ("uniform", _uniform), ("adversarial", _adversarial), ("floor256", _floor256), ("narrow", _narrow),
         ("ramp", _ramp), ("const_255", _const(255)), ("uniform", _uniform), ("geometric", _geometric), ("one_off", _one_off),
         ("alternate", _alternate), ("const_137", _const(137))]

ONE_OFF_AT = ("0", "L-1", "L", "bs-1")
ADVERSARIAL_J = ("0", "K/2", "K-1")
WHERE = ("first", "last")

KINDS = (["const_0", "const_137", "const_255"] + ["one_off_%s_%s" % (w, p) for w in WHERE for p in ONE_OFF_AT]
         + ["alternate", "floor256", "ramp", "uniform", "narrow", "geometric"]
         + ["adversarial_%s_%s" % (j, w) for w in WHERE for j in ADVERSARIAL_J] + ["patchwork"])
EDGE_KINDS = ["patchwork", "uniform"]  # what the launch-edge planes are made of


def segment_of(n, seg, where):
    """(first symbol, length) of the first or of the last segment of a plane of n symbols"""
    k = 0 if where == "first" else (n - 1) // seg
    return k * seg, min(seg, n - k * seg)


def patch_kind(k):
    return PATCH[k % len(PATCH)][0]


def valid(kind, seg, K, n):
    """whether plane(kind, n, seg, K) exists: some kinds need room"""
    L = strand_len(seg, plane_K(seg, K))
    if kind == "floor256":
        return seg >= 512 and n >= 512
    if kind.startswith("one_off_"):
        _, _, where, at = kind.split("_")
        bs = segment_of(n, seg, where)[1]
        return {"0": 0, "L-1": L - 1, "L": L, "bs-1": bs - 1}[at] < bs
    return True


def plane(kind, n, seg, K=0, seed=None):
    """the plane of a case; `seed` defaults to seed_of(seg, n).  Never written to by a test."""
    assert n >= 1 and seg_ok(seg) and (K == 0 or strands_ok(K, seg)) and valid(kind, seg, K, n), (kind, seg, K, n)
    Kp = plane_K(seg, K)
    L = strand_len(seg, Kp)
    rng = np.random.default_rng(seed_of(seg, n) if seed is None else seed)
    if kind.startswith("const_"):
        p = np.full(n, int(kind[6:]), np.uint8)
    elif kind.startswith("one_off_"):
        _, _, where, at = kind.split("_")
        s0, bs = segment_of(n, seg, where)
        p = np.zeros(n, np.uint8)
        p[s0 + {"0": 0, "L-1": L - 1, "L": L, "bs-1": bs - 1}[at]] = 255
    elif kind.startswith("adversarial_"):
        _, j, where = kind.split("_")
        s0, bs = segment_of(n, seg, where)
        p = np.zeros(n, np.uint8)
        p[s0:s0 + bs] = _adversarial(bs, L, rng, {"0": 0, "K/2": Kp // 2, "K-1": Kp - 1}[j])
    elif kind == "floor256":
        p = np.concatenate([_floor256(min(seg, n - s0), L, rng, 0) for s0 in range(0, n, seg)])
    elif kind == "patchwork":
        # (every segment from a generator of its own, so that segment k is the same in planes of different lengths)
        parts = []
        for k, s0 in enumerate(range(0, n, seg)):
            r = np.random.default_rng([seed_of(seg, 0) if seed is None else seed, k])
            parts.append(PATCH[k % len(PATCH)][1](min(seg, n - s0), L, r, (k // len(PATCH)) % Kp))
        p = np.concatenate(parts)
    else:
        p = {"alternate": _alternate, "ramp": _ramp, "uniform": _uniform, "narrow": _narrow, "geometric": _geometric}[kind](n, L, rng, 0)
    p = np.ascontiguousarray(p, dtype=np.uint8)
    assert p.size == n
    p.flags.writeable = False
    return p


# ---- the table -------------------------------------------------------------------------------------------------------------
def grid():
    """(seg, K): K = 0 is WRS1, which gets every segment length including 59984, then every valid strand count"""
    return [(seg, K) for seg in SEGS for K in [0] + KS if K == 0 or strands_ok(K, seg)]


def sizes(seg, K):
    L = strand_len(seg, plane_K(seg, K))
    if seg > 5000:  # as tests/native/strand_fuzz.cpp, to keep the run short
        return [seg - 1, seg + 17, 2 * seg + 7]
    return sorted({n for n in (1, 15, 16, 17, L - 1, L, L + 1, seg - 1, seg, seg + 1, seg + 17, 3 * seg + 7) if n >= 1})


def edge_nsegs(seg, K):
    """segment counts at the launch edges: the wave edge (64 / K segments per wave; one per lane for WRS1) and the 1024 threads
    of the scan kernels (per = ceil(nseg / 1024) turns 2 at 1025 and 3 at 2049)"""
    per_wave = 64 // max(K, 1)
    return sorted({per_wave - 1, per_wave, per_wave + 1, 1023, 1024, 1025, 2049} - {0})


def edge_n(seg, nseg):
    return nseg * seg - 5  # a short last segment


def has_edges(seg, K):
    return seg in (16, 48) or (seg, K) == (512, 32)


def stage_cases(seg, K):
    out = [(kind, seg, K, n) for kind in KINDS for n in sizes(seg, K) if valid(kind, seg, K, n)]
    if has_edges(seg, K):
        out += [(kind, seg, K, edge_n(seg, nseg)) for kind in EDGE_KINDS for nseg in edge_nsegs(seg, K)]
    return out


def edge_cases(seg, K):
    return [(kind, seg, K, edge_n(seg, nseg)) for kind in EDGE_KINDS for nseg in edge_nsegs(seg, K)] if has_edges(seg, K) else []


def all_cases():
    return [c for seg, K in grid() for c in stage_cases(seg, K)]


def case_id(c):
    kind, seg, K, n = c
    return "%s-seg%d-%s-n%d" % (kind, seg, "wrs1" if K == 0 else "K%d" % K, n)


def case_plane(c):
    kind, seg, K, n = c
    return plane(kind, n, seg, K)


def guard_cases(seg, K):
    """the cases that also run on sub-ranges of larger buffers between guard bands: the launch edges, the adversarial planes
    and the sizes around a 16-byte line"""
    small = {1, 15, 17, seg + 17}
    return [c for c in stage_cases(seg, K) if c in set(edge_cases(seg, K)) or c[0].startswith("adversarial_") or c[3] in small]


# ---- fields that carry a chosen plane through the codec ----------------------------------------------------------------------
CODEC_SHAPES = [(8, 64, 128), (1, 50, 300)]
CODEC_SEGS = [1008, 4096]
CODEC_KS = [None, 4, 16]
CODEC_BRICKS = [0, 8]
CODEC_KINDS = ["patchwork", "adversarial_0_first", "adversarial_K/2_first", "adversarial_K-1_last", "one_off_first_L", "one_off_last_bs-1"]


def codec_plane(kind, n, seg, K=0):
    """the plane of `kind` that a codec-level field carries: the case's plane, with 255 as its last symbol where the kind does
    not bring one (a short adversarial strand), because the quantizer maps the field onto 0..255 by its extrema"""
    p = plane(kind, n, seg, K)
    assert p.min() == 0
    if p.max() < 255:
        p = p.copy()
        p[-1] = 255
        p.flags.writeable = False
    return p


def codec_field(p, shape, pi=None):
    """the float64 field shaped (nz, ny, nx) whose plane 0 under wtflag = 0 is p in the stream's symbol order: the natural order
    (pi None) or the blocked order pi (stream position -> coefficient index) of the brick edge used"""
    f = np.empty(p.size, dtype=np.float64)
    if pi is None:
        f[:] = p
    else:
        f[pi] = p
    return f.reshape(shape)
