// wr_segcoder_dev.h -- what a lane of the segment coder kernels works with: its column of the wave's LDS table, the symbols of
// its segment in a plane, and the sinks of coded words and decoded symbols.  Shared by wr_segcoder.hip (one plane per launch)
// and wr_segbatch.hip (the planes of a batch of fields per launch); device code only.
#ifndef WR_SEGCODER_DEV_H
#define WR_SEGCODER_DEV_H

#include "wr_kernels.h"
#include "wr_segcoder.h"

namespace wrk {

namespace {

constexpr int kLanes = 64;

struct LdsTable {
    uint32_t* col;  // &tab[0][lane]
    __device__ uint32_t get(uint32_t s) const { return col[s * kLanes]; }
    __device__ void set(uint32_t s, uint32_t v) { col[s * kLanes] = v; }
};

// the symbols [base, base + bs) of a plane: in one chunk or two (a segment is shorter than a chunk)
struct SegSpan {
    uint8_t* p0;     // symbol i < split is p0[i]
    uint8_t* p1;     // symbol i >= split is p1[i]
    uint32_t split;  // a multiple of 16 (chunks are multiples of 4096 bytes, base is a multiple of 16), or bs
    __device__ SegSpan(const PlaneRef& ref, size_t base, uint32_t bs)
    {
        p0 = ref.at(base);
        const size_t room = ref.shift >= 63 ? (size_t)bs : (((base >> ref.shift) + 1) << ref.shift) - base;
        split = room < bs ? (uint32_t)room : bs;
        p1 = split < bs ? ref.at(base + split) - split : p0;
    }
    __device__ uint8_t* at(uint32_t i) const { return (i < split ? p0 : p1) + i; }
};

struct PlaneSource {
    SegSpan span;
    __device__ void load16(uint32_t i, uint32_t w[4]) const
    {
        const uint4 v = *reinterpret_cast<const uint4*>(span.at(i));
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ uint32_t byte(uint32_t i) const { return *span.at(i); }
};

// coded bytes collected in a register, stored as words into [out, out + cap) (cap: a multiple of 4)
struct WordSink {
    uint32_t* out;
    uint32_t cap, pos, acc;
    bool overflow;
    __device__ void put(uint32_t b)
    {
        acc |= (b & 0xff) << (8 * (pos & 3));
        pos++;
        if ((pos & 3) == 0) {
            if (pos <= cap) out[(pos >> 2) - 1] = acc;
            else overflow = true;
            acc = 0;
        }
    }
    __device__ void flush()
    {
        if (!(pos & 3)) return;
        if ((pos | 3) < cap) out[pos >> 2] = acc;
        else overflow = true;
    }
};

// decoded symbols collected in a register, stored as words; never more than bs of them, never outside the segment
struct SymSink {
    SegSpan span;
    uint32_t bs, pos, acc;
    __device__ void put(uint32_t s)
    {
        if (pos >= bs) return;
        acc |= (s & 0xff) << (8 * (pos & 3));
        pos++;
        if ((pos & 3) == 0) {
            *reinterpret_cast<uint32_t*>(span.at(pos - 4)) = acc;
            acc = 0;
        }
    }
    __device__ void flush()
    {
        for (uint32_t i = pos & ~3u; i < pos; i++) *span.at(i) = (uint8_t)(acc >> (8 * (i & 3)));
    }
};

}  // namespace

}  // namespace wrk

#endif
