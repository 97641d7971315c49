// wr_budget.h -- what an encode to a byte budget is made of, shared by host and device (g++ and hipcc alike, as wr_segcoder.h):
// the grid of relative tolerances the search runs on, and a rigorous upper bound on the bytes of a WRS1 plane blob that
// needs nothing but the segments' histograms.
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
