// wr_budget.h -- what an encode to a byte budget is made of, shared by host and device (g++ and hipcc alike, as wr_segcoder.h):
// the grid of relative tolerances the search runs on, and a rigorous upper bound on the bytes of a WRS1 plane blob that
// needs nothing but the segments' histograms.  An encode to an error bound searches the same grid: its start point and its walk
// over the grid (bounded_start, bounded_walk) are here too, host code only.
//
// The bound.  A segment stream is start(); freq(1, 1, 2); 256 x shift16(count); freq(count, cum, bs) per symbol; freq(1, 0, 2);
// finish() (wr_segcoder.h: encode_segment).  Let P = 8 N - log2(range), N the iterations of Enc::renorm() so far.  An
// iteration leaves P alone (N + 1, range x 256); a coder step raises it by log2(range before / range after); P starts at -31.
// Every step runs behind renorm(), at range R > 2^23, so with r = R / tot rounded down, r >= (R / tot) (1 - tot / 2^23):
//   freq(c, lt, bs):   range after >= r c           the step costs at most log2(bs / c) + loss(bs),  loss(t) = -log2(1 - t / 2^23)
//   shift16(count):    range after >= R >> 16       at most 16 + loss(2^16)
//   the two flags:     range after >= r             at most 1 + loss(2) each
// finish() renormalises once more and the range never exceeds 2^31, so at the end 8 N = P + log2(range) <= the sum of the
// costs: N <= floor(bits / 8) with
//   bits = 2 (1 + loss(2)) + 256 (16 + loss(2^16)) + bs (log2(bs) + loss(bs)) - sum over the symbols s of c_s log2(c_s).
// The stream is the start byte, one byte per iteration and the four bytes finish() appends: N + 5 bytes (wr_segcoder.h
// counts a strand the same way).  This is wrrc::encode_bound_hist's sum for one block, without the 64 bytes of slack that
// function adds for the host loops' early stores.
//
// The arithmetic is integer, so that the host and the probe kernel give the same number bit for bit: bits are counted in
// units of 2^-12.  up[c] = c (log2(c) + loss(c)) rounded UP and down[c] = c log2(c) rounded DOWN, for c in [0, 59999]
// (a segment has fewer than 60000 symbols), come from one table that the host builds once and the device gets a copy of;
// every entry fits 32 bits (59999 x 15.884 x 4096 < 2^32).  256 entries rounded by less than 2^-12 bit each cost a
// segment 1/16 bit.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wr_segcoder.h"

namespace wrbud {

// ---- the tolerance grid: t(g) = (64 + (g & 63)) * 2^((g >> 6) - 66), exact doubles from 2^-60 to 1 in steps of at most 65/64
constexpr int kGMax = 3840;
// assembled from its bits: (1 + m / 64) * 2^(k - 60) has exponent field 1023 + k - 60 and m in the top six mantissa bits
inline double grid_tol(int g)
{
    if (g < 0) g = 0;
    if (g > kGMax) g = kGMax;
    const uint64_t bits = (uint64_t)(1023 - 60 + (g >> 6)) << 52 | (uint64_t)(g & 63) << 46;
    double t;
    memcpy(&t, &bits, sizeof t);
    return t;
}
// the smallest g with t(g) >= tolrel, clamped to the grid (a NaN lands on 0)
inline int grid_index(double tolrel)
{
    if (!(tolrel > grid_tol(0))) return 0;
    if (tolrel >= 1.0) return kGMax;
    int lo = 0, hi = kGMax;  // t(lo) < tolrel <= t(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (grid_tol(mid) >= tolrel) hi = mid;
        else lo = mid;
    }
    return hi;
}

// where the search of an encode to an error bound starts: the largest g with t(g) * absmax <= max_abs_err (one fp64 multiply,
// which does not fall as g grows, so a bisection by comparison finds it); -1 when even t(0) is too coarse or an argument is
// not a positive finite number
inline int bounded_start(double max_abs_err, double absmax)
{
    if (!(max_abs_err > 0) || !(absmax > 0) || max_abs_err > DBL_MAX || absmax > DBL_MAX) return -1;
    if (!(grid_tol(0) * absmax <= max_abs_err)) return -1;
    if (grid_tol(kGMax) * absmax <= max_abs_err) return kGMax;
    int lo = 0, hi = kGMax;  // t(lo) * absmax <= max_abs_err < t(hi) * absmax
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (grid_tol(mid) * absmax <= max_abs_err) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the RMS error a PSNR of `db` over the range hi - lo means: range * 10^(-db / 20); NaN unless db is finite and the range a
// positive finite number (include/waverange_amd.h: wr_psnr_rms)
inline double psnr_rms(double db, double lo, double hi)
{
    const double range = hi - lo;
    if (!(fabs(db) <= DBL_MAX) || !(range > 0) || range > DBL_MAX) return NAN;
    return range * pow(10.0, -db / 20.0);
}

// grid points a change of the error by the factor r (> 1) is worth at nominal: 64 to the octave, a quarter kept back
inline int bounded_points(double r)
{
    const double d = 48.0 * log2(r);
    return d >= (double)kGMax ? kGMax : d > 0 ? (int)d : 0;
}

// The walk of an encode to an error bound over E(g), the error reached at grid point g.  eval(g, &e) forms E(g) (0: done,
// otherwise the walk ends with that code); it is asked about a point at most once.  From `start` (clamped to [g_min, kGMax]):
// while the bound does not hold, finer by the ratio E / max_err, or by twice the last step if that is more; then coarser
// likewise by max_err / E, and when a step lands on a point that does not hold, a bisection between it and the last one that
// does ends on neighbours.  Near nominal that is a jump and a few single steps; it is never more than 2 log2 of the grid.
// Returns 0 with *g in [g_min, kGMax], *e = E(*g) <= max_err and *g == kGMax or E(*g + 1) > max_err (E is not monotone: the
// property is this local one); kBoundedMiss with *e = E(g_min) > max_err; or eval's code.
constexpr int kBoundedMiss = -1000;
template <class Eval>
int bounded_walk(double max_err, int g_min, int start, Eval eval, int* g, double* e)
{
    std::vector<double> known((size_t)kGMax + 1, -1.0);  // E >= 0 where it has been formed
    auto E = [&](int at, double* out) {
        if (known[(size_t)at] < 0) {
            if (int rc = eval(at, out)) return rc;
            known[(size_t)at] = *out;
        }
        *out = known[(size_t)at];
        return 0;
    };
    if (g_min < 0) g_min = 0;
    if (g_min > kGMax) g_min = kGMax;
    int at = start < g_min ? g_min : start > kGMax ? kGMax : start;
    double cur = 0, e2 = 0;
    if (int rc = E(at, &cur)) return rc;
    int step = 0;
    while (!(cur <= max_err)) {
        if (at == g_min) { *g = at; *e = cur; return kBoundedMiss; }
        const int d = bounded_points(cur / max_err);
        step = d > 2 * step ? d : 2 * step;  // (doubling: an error that does not follow the tolerance costs log2 of the grid, not the grid)
        if (step < 1) step = 1;
        at = at - step < g_min ? g_min : at - step;
        if (int rc = E(at, &cur)) return rc;
    }
    step = 0;
    while (at < kGMax) {
        const int d = cur > 0 ? bounded_points(max_err / cur) : kGMax;
        step = d > 2 * step ? d : 2 * step;
        if (step < 1) step = 1;
        const int far = at + step > kGMax ? kGMax : at + step;
        if (int rc = E(far, &e2)) return rc;
        if (e2 <= max_err) { at = far; cur = e2; continue; }
        int good = at, bad = far;  // E(good) holds, E(bad) does not: neighbours of that kind between them
        while (bad - good > 1) {
            const int mid = good + (bad - good) / 2;
            if (int rc = E(mid, &e2)) return rc;
            if (e2 <= max_err) { good = mid; cur = e2; }
            else bad = mid;
        }
        at = good;
        break;
    }
    *g = at; *e = cur;
    return 0;
}

// ---- the size bound
constexpr int kFrac = 12;                              // bits are counted in units of 2^-12
constexpr uint32_t kTabN = wrseg::kSegMax + 1;         // counts 0 .. 59999
constexpr size_t kTabWords = 2 * (size_t)kTabN;        // down[0, kTabN) then up[0, kTabN)
constexpr uint32_t kStreamTail = 5;                    // the start byte and the four bytes of finish()

// the bytes one segment stream of bs symbols can take at most: `fixed` is the flags' and the 256 counts' part, up_bs =
// up[bs], sum_down = the sum of down[c_s] over the 256 symbols.  (up[bs] >= bs log2(bs) >= sum c_s log2(c_s) >= sum_down.)
WRSEG_HD uint32_t segment_bytes(uint64_t fixed, uint32_t up_bs, uint64_t sum_down)
{
    return (uint32_t)((fixed + up_bs - sum_down) >> (kFrac + 3)) + kStreamTail;
}
// what the blob adds to its segment streams: the header and the index
WRSEG_HD size_t blob_overhead(size_t nseg) { return wrseg::kHeaderBytes + 4 * nseg; }

// ---- host side: the table and the bound of a plane of symbols
struct Tables {
    std::vector<uint32_t> words;  // kTabWords: what the device gets
    uint64_t fixed;
    const uint32_t* down() const { return words.data(); }
    const uint32_t* up() const { return words.data() + kTabN; }
};

// Built once.  libm's log2 is good to an ulp, products of doubles to half an ulp: 1e-12 relative (a thousand times that)
// is added before rounding up and taken off before rounding down, and one unit on top.  Exact zeros (c = 0, c = 1) stay zero.
inline const Tables& tables()
{
    static const Tables t = []() {
        Tables b;
        b.words.assign(kTabWords, 0);
        const double unit = (double)(1u << kFrac);
        auto up = [&](double bits) { return (uint64_t)ceil(bits * unit * (1.0 + 1e-12)) + 1; };
        auto down = [&](double bits) {
            const double v = floor(bits * unit * (1.0 - 1e-12)) - 1.0;
            return v > 0 ? (uint64_t)v : (uint64_t)0;
        };
        auto loss = [](double tot) { return -log2(1.0 - tot / 8388608.0); };
        for (uint32_t c = 1; c < kTabN; c++) {
            const double lg = log2((double)c);
            b.words[c] = (uint32_t)(c > 1 ? down((double)c * lg) : 0);
            b.words[kTabN + c] = (uint32_t)up((double)c * (lg + loss((double)c)));
        }
        b.fixed = up(2.0 * (1.0 + loss(2.0)) + 256.0 * (16.0 + loss(65536.0)));
        return b;
    }();
    return t;
}

// the bound of one segment from its 256 counts (which sum to bs, 1 <= bs <= 59999)
inline uint32_t segment_bound(const Tables& t, const uint32_t* counts, uint32_t bs)
{
    uint64_t sum = 0;
    for (int s = 0; s < 256; s++) sum += t.down()[counts[s]];
    return segment_bytes(t.fixed, t.up()[bs], sum);
}

// an upper bound on the length of the WRS1 blob of a plane (wrtc::seg_encode_ref, the GPU coder): header, index and the
// bound of every segment.  seg as wrseg::seg_ok wants it.
inline size_t plane_bound(const uint8_t* sym, size_t n, uint32_t seg)
{
    const Tables& t = tables();
    const size_t nseg = wrseg::seg_count(n, seg);
    size_t total = blob_overhead(nseg);
    for (size_t k = 0; k < nseg; k++) {
        const size_t s0 = k * seg;
        const uint32_t bs = (uint32_t)(n - s0 < seg ? n - s0 : seg);
        uint32_t counts[256] = {0};
        for (uint32_t i = 0; i < bs; i++) counts[sym[s0 + i]]++;
        total += segment_bound(t, counts, bs);
    }
    return total;
}

}  // namespace wrbud
