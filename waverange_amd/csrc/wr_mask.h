// Masked fields: the kernels that split a field into its defined samples and a packed bit mask, and put values back where
// the mask says so (wr_mask.hip), and the mask blob "WRM1" (include/waverange_amd.h), whose host side is plain code here.
//
// A sample x is UNDEFINED if it is not finite, !(fabs(x) <= DBL_MAX), or if x < below (below = -inf: no threshold).  Sample j's
// bit is bit j & 7 (least significant first) of mask byte j >> 3; a mask of n samples has ceil(n / 8) bytes, the unused high
// bits of the last one 0.
#ifndef WR_MASK_H
#define WR_MASK_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "wr_segcoder.h"

#ifndef WR_MASK_HOST_ONLY  // (defined by a host-only program that wants the blob and the crop below without the HIP runtime)
#include <hip/hip_runtime.h>
#endif

namespace wrmask {

constexpr size_t kHeaderBytes = 32;  // 'W','R','M','1' | u32 0 | u64 n | u64 undefined | f64 pad
constexpr unsigned char kMagic[4] = {'W', 'R', 'M', '1'};

inline size_t mask_bytes(size_t n) { return (n + 7) >> 3; }

inline void put_u64(unsigned char* p, unsigned long long v) { for (int k = 0; k < 8; k++) p[k] = (unsigned char)(v >> (8 * k)); }
inline unsigned long long get_u64(const unsigned char* p)
{
    unsigned long long v = 0;
    for (int k = 0; k < 8; k++) v |= (unsigned long long)p[k] << (8 * k);
    return v;
}

inline void put_header(unsigned char* p, unsigned long long n, unsigned long long undefined, double pad)
{
    memcpy(p, kMagic, 4);
    memset(p + 4, 0, 4);
    put_u64(p + 8, n);
    put_u64(p + 16, undefined);
    unsigned long long bits;
    memcpy(&bits, &pad, 8);
    put_u64(p + 24, bits);
}

inline bool sniff(const unsigned char* p, size_t len) { return p && len >= kHeaderBytes && memcmp(p, kMagic, 4) == 0; }

// What the header of a blob of `len` bytes says, for a field of n samples; nullptr, or why the blob is refused.  The WRS1 blob
// behind the header is the caller's to check (wrseg::check_index).
inline const char* check_header(const unsigned char* p, size_t len, size_t n, unsigned long long* undefined, double* pad)
{
    if (len < kHeaderBytes) return "mask blob: truncated header";
    if (memcmp(p, kMagic, 4) != 0) return "mask blob: wrong magic";
    if (p[4] | p[5] | p[6] | p[7]) return "mask blob: the reserved word is not 0";
    if (get_u64(p + 8) != (unsigned long long)n) return "mask blob: its sample count is not the field's";
    *undefined = get_u64(p + 16);
    if (*undefined > (unsigned long long)n) return "mask blob: more undefined samples than samples";
    const unsigned long long bits = get_u64(p + 24);
    memcpy(pad, &bits, 8);
    return nullptr;
}

// ---- the crop of a mask (include/waverange_amd.h, "Masked region and low-resolution decode"), host only.  Sample (i, j, k) of
// the level-r box sits at the field's sample (i << r, j << r, k << r): lifting keeps the even samples.  A region is a half-open
// box in the coordinates of the level-r box, inside it.
struct Region {
    int nx, ny, nz;  // the FIELD's extents
    int r;           // the level
    int x0, y0, z0, x1, y1, z1;
    size_t elems() const { return (size_t)(x1 - x0) * (y1 - y0) * (z1 - z0); }
    // the mask bit of the region's sample (x, y, z), region coordinates
    size_t bit(int x, int y, int z) const
    {
        return ((size_t)(x0 + x) << r) + (size_t)nx * (((size_t)(y0 + y) << r) + (size_t)ny * ((size_t)(z0 + z) << r));
    }
};

// The ascending ids of the mask-plane segments (of `seg` symbols, a symbol = 8 bits) that hold a bit of the region; at most
// `cap` are written to ids (nullptr: none), the number of all of them is returned.  The bits of a run (y, z) are 2^r <= 16
// apart and a segment holds at least 128, so a run touches every segment between its first and its last; the runs ascend in the
// plane, so do the segments.
inline size_t roi_segments(const Region& g, uint32_t seg, uint32_t* ids, size_t cap)
{
    size_t count = 0, next = 0;  // next: the first segment not yet listed
    for (int z = 0; z < g.z1 - g.z0; z++)
        for (int y = 0; y < g.y1 - g.y0; y++) {
            size_t k = (g.bit(0, y, z) >> 3) / seg;
            const size_t last = (g.bit(g.x1 - g.x0 - 1, y, z) >> 3) / seg;
            if (k < next) k = next;
            for (; k <= last; k++) {
                if (ids && count < cap) ids[count] = (uint32_t)k;
                count++;
            }
            next = last + 1;
        }
    return count;
}

// What the header and the index of a blob say: the one validation of a mask blob, for a field of n samples.  The header
// (check_header), then the whole segment index of the WRS1 plane behind it (wrseg::check_index; the plane's seg is read from its
// own header).  false: refused, *why saying what ("mask blob: ...").
struct BlobInfo {
    unsigned long long undefined = 0;
    double pad = 0;
    uint32_t seg = 0, nseg = 0;
};
inline bool check_blob(const unsigned char* blob, size_t len, size_t n, BlobInfo* info, std::string* why)
{
    if (const char* w = check_header(blob, len, n, &info->undefined, &info->pad)) { *why = w; return false; }
    const size_t rest = len - kHeaderBytes;
    if (const char* w = wrseg::check_index(blob + kHeaderBytes, rest, rest, mask_bytes(n), &info->seg, &info->nseg)) {
        *why = std::string("mask blob: ") + w;
        return false;
    }
    return true;
}

// The blobs of a batch of masked records, validated in field order as the single masked call validates its one (check_blob).
// blobs[f] == nullptr: field f has no blob and is passed over.  Returns nfields if every blob passes and info[f] is then filled
// for every field that has one; otherwise the first field whose blob fails, *why saying what, and nothing behind that field has
// been looked at.
inline int check_blobs(const unsigned char* const* blobs, const size_t* lens, int nfields, size_t n, BlobInfo* info, std::string* why)
{
    for (int f = 0; f < nfields; f++)
        if (blobs[f] && !check_blob(blobs[f], lens[f], n, &info[f], why)) return f;
    return nfields;
}

// ... of several regions of one field (the masked region decode across a batch of fields): the ascending union of the regions'
// lists, with roi_segments' conventions
inline size_t roi_segments_multi(const Region* gs, size_t nroi, uint32_t seg, uint32_t* ids, size_t cap)
{
    std::vector<uint32_t> all;
    for (size_t i = 0; i < nroi; i++) {
        const size_t at = all.size(), count = roi_segments(gs[i], seg, nullptr, 0);
        all.resize(at + count);
        roi_segments(gs[i], seg, all.data() + at, count);
    }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    if (ids)
        for (size_t k = 0; k < all.size() && k < cap; k++) ids[k] = all[k];
    return all.size();
}

// The turns of k_mask_restore_boxes over one field's regions: a turn is 64 consecutive x of one region row, region i has
// ceil(cx / 64) * cy * cz of them, first[0 .. nroi] (nullptr: not wanted) is their exclusive prefix.  Returns their number, or 0
// for 2^31 turns or more (first[] is then not to be used).
constexpr unsigned long long kTurnLimit = 1ull << 31;
inline size_t boxes_turns(const Region* gs, size_t nroi, uint32_t* first)
{
    unsigned long long run = 0;
    for (size_t i = 0; i < nroi; i++) {
        if (first) first[i] = (uint32_t)run;
        const Region& g = gs[i];
        const unsigned long long rows = (unsigned long long)(((long long)g.x1 - g.x0 + 63) >> 6) * (unsigned long long)(g.y1 - g.y0);  // (below 2^56)
        if (rows >= kTurnLimit) return 0;
        run += rows * (unsigned long long)(g.z1 - g.z0);  // (below 2^62 + 2^31)
        if (run >= kTurnLimit) return 0;
    }
    if (first) first[nroi] = (uint32_t)run;
    return (size_t)run;
}

}  // namespace wrmask

#ifndef WR_MASK_HOST_ONLY
namespace wrk {

// ---- k_mask_split: one read of the field.  bits[0, ceil(n / 8)) = the mask; result[0] = S, the fp64 sum of the defined samples
// (widened exactly for an fp32 field), result[1] = their count as an unsigned 64-bit integer (same 8 bytes).  The order of the
// sum is fixed by n alone: a thread adds its samples in index order, lanes combine by shuffles at distances 32 .. 1, thread 0
// adds the waves in wave order, the final block's thread t adds partials t, t + 256, .. and reduces the same way; no
// floating-point atomics.  partial: 2 * mask_partials() 8-byte words.  `bits` may have any alignment (8-byte aligned: a wave
// stores the 8 mask bytes of its 64 samples as one word).
int mask_partials();
void mask_split(const double* x, size_t n, double below, uint8_t* bits, double* partial, double* result, hipStream_t st);
void mask_split(const float* x, size_t n, double below, uint8_t* bits, double* partial, double* result, hipStream_t st);
// ---- k_mask_fill: x[j] = v where bit j is set; a wave whose 8 mask bytes are 0 stores nothing.
void mask_fill(double* x, size_t n, const uint8_t* bits, double v, hipStream_t st);
void mask_fill(float* x, size_t n, const uint8_t* bits, float v, hipStream_t st);
// ---- k_mask_restore: the same walk with the mask checked: counters[0] += the set bits of the mask's ceil(n / 8) bytes,
// counters[1] |= 1 if one of them lies at or beyond n (integer atomics, one per wave; zeroed here).  x == nullptr: only counted.
void mask_restore(double* x, size_t n, const uint8_t* bits, double v, unsigned long long* counters, hipStream_t st);
void mask_restore(float* x, size_t n, const uint8_t* bits, float v, unsigned long long* counters, hipStream_t st);
// ---- k_mask_restore_box: the restore on a region of a level's box.  out = the region's elements, contiguous, x fastest;
// out[x, y, z] = v where bit g.bit(x, y, z) of `bits` is set, nothing else is touched; counters[0] += the set bits among the
// region's (one integer atomic per wave; zeroed here).  `bits` is the full-length plane, any alignment; only bytes that hold a
// bit of the region are read.
void mask_restore_box(double* out, const wrmask::Region& g, const uint8_t* bits, double v, unsigned long long* counters, hipStream_t st);
void mask_restore_box(float* out, const wrmask::Region& g, const uint8_t* bits, float v, unsigned long long* counters, hipStream_t st);
// ---- k_mask_restore_boxes: mask_restore_box on every (field that has a mask, region) of a region decode across a batch of
// fields, in one launch.  out = nfields parts of field_elems elements each; region i (gs[i], all of one field shape and level)
// of field f lies at out + f * field_elems + offs[i].  bits[f] (a host array of device pointers): field f's full-length plane,
// any alignment, or nullptr: a field without a mask, whose part is not touched.  The m-th field that has a plane counts the set
// bits among its regions' (a sample in two regions twice) in mask_boxes_counters(table, nroi, nfields)[m] (integer atomics, one
// per wave and item; zeroed here).  table: mask_boxes_table_bytes(nroi, nfields) of device memory, 256-byte aligned;
// host_table: as much host memory, which stays alive until the stream has passed the copy.  Returns the fields that have a
// plane (0: nothing was launched), or -1: refused, the launch would have 2^31 turns or more (wrmask::boxes_turns).
size_t mask_boxes_table_bytes(size_t nroi, size_t nfields);
unsigned long long* mask_boxes_counters(uint8_t* table, size_t nroi, size_t nfields);
int mask_restore_boxes(double* out, const wrmask::Region* gs, const size_t* offs, size_t nroi, const uint8_t* const* bits, size_t nfields, size_t field_elems, double v,
                       uint8_t* host_table, uint8_t* table, hipStream_t st);
int mask_restore_boxes(float* out, const wrmask::Region* gs, const size_t* offs, size_t nroi, const uint8_t* const* bits, size_t nfields, size_t field_elems, float v,
                       uint8_t* host_table, uint8_t* table, hipStream_t st);
// ---- the batch forms: split, fill and check across fields of n samples each, one launch per stage on a grid of
// (mask_grid(n), fields) blocks.  The tables live in pinned host memory that the kernels read directly (d_items: the same
// block as the device sees it) and stay alive until the stream has passed the launch.
// k_mask_split_batch + k_mask_split_final_batch: field f's mask into items[f].bits, result[2f] = S and result[2f + 1] = the
// count of its defined samples, bit for bit what mask_split gives for that field alone (block (x, f) is block x of
// k_mask_split).  partial: nfields * mask_split_batch_partials(n) 8-byte words of device memory.  The kernel stores a word per
// chunk only if every field's bits pointer is 8-byte aligned (host_items is read for that).
struct MaskSplitItem {
    const void* x;  // n samples, fp64 or fp32 as the launch says
    uint8_t* bits;
};
size_t mask_split_batch_partials(size_t n);
void mask_split_batch(const MaskSplitItem* host_items, const MaskSplitItem* d_items, int nfields, bool f32, size_t n, double below, double* partial, double* result,
                      hipStream_t st);
// k_mask_fill_batch: mask_fill on every item; value = mask_fill_value(v, f32), the bits of the (T)v that mask_fill would store
struct MaskFillItem {
    void* x;
    const uint8_t* bits;
    unsigned long long value;
};
unsigned long long mask_fill_value(double v, bool f32);
void mask_fill_batch(const MaskFillItem* d_items, int nitems, bool f32, size_t n, hipStream_t st);
// k_mask_check_batch: the count-only mask_restore on nmasks masks of n bits: counters[2m] += the set bits of mask m's
// ceil(n / 8) bytes, counters[2m + 1] |= 1 if one lies at or beyond n (integer atomics, one per wave and mask; zeroed here).
// d_masks: the table of plane pointers, device-visible; counters: 2 * nmasks words of device memory.
void mask_check_batch(const uint8_t* const* d_masks, int nmasks, size_t n, unsigned long long* counters, hipStream_t st);
// x[0, n) = v in fp32 (wrk::fill is the fp64 one)
void fill_f32(float* x, size_t n, float v, hipStream_t st);
// ---- k_err_stats_masked: the compare of wrk::err_stats over the samples whose bit is clear.  result[0 .. 2] = the maximum of the
// finite |a - b|, the count of differences that are not finite, the fp64 sum of the squared finite differences; *defined = the
// clear bits below n (an exact integer; a word of its own, so that result's neighbours stay untouched).  Nothing at a position
// whose bit is set enters a result, whatever it holds, and no sample at or beyond n and no mask byte at or beyond ceil(n / 8) is read.  a, b and bits may have any alignment (both arrays aligned for two-sample loads: 128 samples and 16
// mask bytes per wave and turn; a turn whose bits are all set loads neither array).  partial: 4 * mask_partials() 8-byte words.
void err_stats_masked(const double* a, const double* b, size_t n, const uint8_t* bits, double* partial, double* result, unsigned long long* defined,
                      hipStream_t st);
void err_stats_masked(const float* a, const float* b, size_t n, const uint8_t* bits, double* partial, double* result, unsigned long long* defined,
                      hipStream_t st);

}  // namespace wrk
#endif

#endif
