"""The case table of the batched strand coder kernels (csrc/wr_segbatch.hip: k_strand_encode_batch, k_strand_gather_batch,
k_strand_decode_batch).  Pure numpy and seeded; nothing of the library is imported.  tests/test_strand_batch_cpu.py asserts that
the table is what it claims to be, tests/test_gpu_strand_batch.py runs it on the card.

A stage-level case is (n, seg, K, jobs): `jobs` planes of n symbols each, coded in ONE launch sequence as WRS3 with K strands
per segment of `seg` symbols.  classes(case) names the paths of the two lane layouts the case reaches:

  the encoder   lane g is strand g & (K - 1) of launch segment g / K, the jobs' segments behind one another without padding
  the decoder   job j owns nseg * K lanes rounded up to whole waves of 64

The planes come from coder_cases.plane ("patchwork", "adversarial_*", "one_off_*": one wave holds different models, streams
from under 20 bytes to near the bound) and util.kat_plane, rolled so that every job of a launch is a different plane."""
import numpy as np

import coder_cases as cc
from util import kat_plane

WAVE = 64

# (n, seg, K, jobs): the smallest shapes that reach each class
STAGE = [
    (1024, 4096, 8, 17),      # one segment per job: every K-group of a wave is a different job; strands 2..7 empty; third wave with 8 live lanes
    (69120, 4096, 32, 3),     # 17 segments per job at two per wave: a wave spans two jobs; last segment 3584 symbols, four empty strands
    (17600, 16, 1, 3),        # K = 1; 1100 segments per job, past the scan's 1024 threads
    (17600, 48, 2, 5),        # L = 32: strand 1 holds 16 symbols; last segment 32 symbols, strand 1 empty; 734 lanes per job, decoder pads to 768
    (3025, 1008, 16, 9),      # last strand 48 symbols; a one-symbol last segment; 64 lanes per job exactly, no padding
    (262144, 59904, 8, 13),   # the default seg; 65 segments, a ninth wave with one live group
    (4097, 4096, 4, 1),       # a batch of one
]

REQUIRED = {
    "one_segment_per_job",      # every K-group of the encoder's waves belongs to another job
    "wave_spans_jobs",          # encoder: some wave holds groups of two jobs, the boundary not at a wave's edge
    "wave_inside_job",          # encoder: some wave lies inside one job
    "empty_strands",            # a last segment so short that strands have no symbols (m == 0 in live lanes)
    "short_last_strand",        # seg is no multiple of L: strand K - 1 of a full segment is shorter than L
    "one_symbol_segment",       # a last segment of one symbol
    "partial_last_wave",        # encoder: the grid's last wave has lanes past the end (not live, through both barriers)
    "full_last_wave",           # encoder: the grid ends on a wave's edge
    "K1",                       # one strand per segment: no shuffle step, kshift == 0
    "K32",                      # two segments per wave
    "scan_past_1024",           # more segments per job than the scan kernel has threads
    "decoder_padding",          # decoder: a job's lanes are rounded up, padding lanes go through the body
    "decoder_exact",            # decoder: a job's lanes are whole waves as they stand
    "default_seg",
    "batch_of_one",
    "many_jobs",                # more jobs than a wave has K-groups
}


def nseg_of(n, seg):
    return (n + seg - 1) // seg


def classes(case):
    n, seg, K, jobs = case
    nseg, L = nseg_of(n, seg), cc.strand_len(seg, K)
    last = n - (nseg - 1) * seg
    per_wave = WAVE // K
    out = set()
    if nseg == 1:
        out.add("one_segment_per_job")
    bounds = {j * nseg for j in range(1, jobs)}  # launch segments at which a new job starts
    if any(b % per_wave for b in bounds):
        out.add("wave_spans_jobs")
    waves = (jobs * nseg + per_wave - 1) // per_wave
    if any(not any(w * per_wave < b < (w + 1) * per_wave for b in bounds) for w in range(waves)):
        out.add("wave_inside_job")
    if (last + L - 1) // L < K:
        out.add("empty_strands")
    if seg % L and nseg > 1:
        out.add("short_last_strand")
    if last == 1:
        out.add("one_symbol_segment")
    out.add("partial_last_wave" if (jobs * nseg * K) % WAVE else "full_last_wave")
    if K == 1:
        out.add("K1")
    if K == 32:
        out.add("K32")
    if nseg > 1024:
        out.add("scan_past_1024")
    out.add("decoder_padding" if (nseg * K) % WAVE else "decoder_exact")
    if seg == 59904:
        out.add("default_seg")
    if jobs == 1:
        out.add("batch_of_one")
    if jobs > per_wave:
        out.add("many_jobs")
    return out


def reached():
    out = set()
    for c in STAGE:
        out |= classes(c)
    return out


KINDS = ["patchwork", "adversarial_0_first", "adversarial_K/2_last", "adversarial_K-1_last", "one_off_first_L", "one_off_last_bs-1"]
KATS = ["uniform", "skewed", "sparse"]

_planes = {}


def base_planes(n, seg, K):
    """the different planes of a case's size, made once and never written to"""
    key = (n, seg, K)
    if key not in _planes:
        out = [cc.plane(kind, n, seg, K) for kind in KINDS if cc.valid(kind, seg, K, n)]
        for kind in KATS:
            p = kat_plane(kind, n)
            p.flags.writeable = False
            out.append(p)
        _planes[key] = out
    return _planes[key]


def planes(case):
    """the `jobs` planes of a case, all different: the base planes, then rotations of them by multiples of 37 symbols; where a
    plane comes out as an earlier one (a one-segment patchwork plane is constant, "first" and "last" name the same segment) the
    skewed known-answer plane takes its place, rotated by the job's number"""
    n, seg, K, jobs = case
    base = base_planes(n, seg, K)
    out, seen = [], set()
    for j in range(jobs):
        p = np.roll(base[j % len(base)], 37 * (j // len(base)))
        if p.tobytes() in seen:
            p = np.roll(kat_plane("skewed", n), 37 * j + 1)
        assert p.tobytes() not in seen, (case, j)
        seen.add(p.tobytes())
        p.flags.writeable = False
        out.append(p)
    return out


def case_id(case):
    return "n%d-seg%d-K%d-jobs%d" % case


# ---- the mixed decode list: one launch of plain jobs and one of stranded jobs, formats and segment lengths side by side
MIXED_N = 69120
MIXED_JOBS = 11
MIXED_FORMATS = [(4096, 0), (4096, 8), (4096, 32), (16, 1), (59904, 0)]  # (seg, K); K == 0: WRS1


def mixed_jobs():
    """[(plane, seg, K)]: job i has format i % 5 and plane i of the case (69120, 4096, 8, 11)"""
    ps = planes((MIXED_N, 4096, 8, MIXED_JOBS))
    return [(ps[i],) + MIXED_FORMATS[i % len(MIXED_FORMATS)] for i in range(MIXED_JOBS)]


# ---- the two lane layouts in plain Python
def encoder_layout(nsegs, K):
    """lane -> (job, segment, strand) of a strand-encode launch over jobs of nsegs[j] segments; the grid's lanes past the end are
    absent.  Also returns the grid's size (whole waves)."""
    out, g = {}, 0
    for j, ns in enumerate(nsegs):
        for k in range(ns):
            for s in range(K):
                out[g] = (j, k, s)
                g += 1
    return out, (g + WAVE - 1) // WAVE * WAVE


def decoder_layout(nsegs, Ks):
    """(first, lane -> (job, segment, strand)) of a strand-decode launch: job j owns nsegs[j] * Ks[j] lanes rounded up to whole
    waves; padding lanes are absent"""
    first, out, g = [0], {}, 0
    for j, (ns, K) in enumerate(zip(nsegs, Ks)):
        for r in range(ns * K):
            out[g + r] = (j, r // K, r % K)
        g += (ns * K + WAVE - 1) // WAVE * WAVE
        first.append(g)
    return first, out
