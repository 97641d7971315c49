// wr_segcoder.hip -- the segmented plane stream ("WRS1", wr_segcoder.h) coded and decoded on the GPU.
//
// One lane owns one segment: a complete rngcod13 stream, an independent serial chain.  A workgroup is one wave; its 64
// models live in LDS as tab[256][64] words (count << 16 | cumulative count), 64 KiB, so two waves are resident per CU and word
// (sym, lane) lies in bank `lane` whatever `sym` is: the data-dependent look-ups of a wave never conflict.  The same table
// takes the histogram pass first.
//
//   k_seg_encode   lane k: histogram -> model -> stream of segment k, words appended to the segment's own region of the
//                  staging buffer (stride = the segment bound, 4-byte aligned); lens[k] = its length
//   k_seg_scan     exclusive scan of lens -> offs, the blob's header and index, the blob's length
//   k_seg_gather   staging regions -> the blob, coalesced, destination-aligned words
//   k_seg_decode   lane k: stream of segment k (at offs[k] in the blob) -> the plane's symbols [k*seg, k*seg + bs); with a
//                  list of segment ids, lane j takes segment ids[j] and the others are left alone (a low-resolution decode)
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

__global__ __launch_bounds__(kLanes) void k_seg_encode(PlaneRef sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t* stage,
                                                       uint32_t stride_words, uint32_t* lens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t k = (size_t)blockIdx.x * kLanes + lane;
    LdsTable t{tab + lane};
    for (uint32_t s = 0; s < 256; s++) t.set(s, 0);
    if (k >= nseg) return;
    const size_t base = k * seg;
    const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
    PlaneSource src{SegSpan(sym, base, bs)};
    wrseg::build_model(t, src, bs);
    wrseg::Enc<WordSink> e;
    e.out = WordSink{stage + k * stride_words, stride_words * 4, 0, 0, false};
    wrseg::encode_segment(e, t, src, bs);
    e.out.flush();
    lens[k] = e.out.overflow ? 0xffffffffu : e.out.pos;  // (cannot overflow: the stride is the segment bound)
}

constexpr int kScanThreads = 1024;

// result[0] = the blob's length, result[1] = segments that did not fit their region (0 always: see k_seg_encode).  The blob's
// header and index are written if they fit under cap (the host has checked that before the launch).
__global__ __launch_bounds__(kScanThreads) void k_seg_scan(const uint32_t* lens, uint32_t nseg, uint32_t seg, uint32_t brick, unsigned long long* offs,
                                                           uint8_t* blob, size_t cap, unsigned long long* result,
                                                           unsigned long long* result_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    const uint32_t t = threadIdx.x;
    const size_t head = wrseg::header_bytes(brick);  // (brick != 0: the blocked format's header, one word longer)
    if (t == 0) bad = 0;
    __syncthreads();
    const uint32_t per = (nseg + kScanThreads - 1) / kScanThreads;
    const size_t k0 = (size_t)t * per, k1 = k0 + per < nseg ? k0 + per : nseg;
    unsigned long long sum = 0;
    unsigned int mybad = 0;
    for (size_t k = k0; k < k1; k++) {
        const uint32_t l = lens[k];
        if (l == 0xffffffffu) mybad++;
        else sum += l;
    }
    part[t] = sum;
    if (mybad) atomicAdd(&bad, mybad);
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int j = 0; j < kScanThreads; j++) { const unsigned long long v = part[j]; part[j] = run; run += v; }
        const unsigned long long total = head + 4ull * nseg + run;
        offs[nseg] = run;
        result[0] = total; result[1] = bad;
        if (result_host) { result_host[0] = total; result_host[1] = bad; }
        if (cap >= head) {
            uint32_t* const h = reinterpret_cast<uint32_t*>(blob);
            const uint8_t* const mg = brick ? wrseg::kMagicBlocked : wrseg::kMagic;
            h[0] = (uint32_t)mg[0] | (uint32_t)mg[1] << 8 | (uint32_t)mg[2] << 16 | (uint32_t)mg[3] << 24;
            h[1] = seg; h[2] = nseg;
            if (brick) h[3] = brick;
        }
    }
    __syncthreads();
    const bool index_fits = cap >= head + 4ull * nseg;
    uint32_t* const index = reinterpret_cast<uint32_t*>(blob + head);
    unsigned long long run = part[t];
    for (size_t k = k0; k < k1; k++) {
        const uint32_t l = lens[k];
        offs[k] = run;
        if (index_fits) index[k] = l == 0xffffffffu ? 0 : l;
        if (l != 0xffffffffu) run += l;
    }
}

constexpr int kGatherThreads = 256;

// blob[header + index + offs[k] ...) := the first lens[k] bytes of segment k's staging region.  Nothing is written unless the
// whole blob fits under cap and every segment is good.
__global__ __launch_bounds__(kGatherThreads) void k_seg_gather(const uint32_t* stage, uint32_t stride_words, const uint32_t* lens,
                                                               const unsigned long long* offs, uint32_t nseg, uint32_t brick, uint8_t* blob,
                                                               size_t cap, const unsigned long long* result)
{
    if (result[0] > cap || result[1]) return;
    const size_t front = wrseg::header_bytes(brick) + 4 * (size_t)nseg;
    const uint32_t t = threadIdx.x;
    for (size_t k = blockIdx.x; k < nseg; k += gridDim.x) {
        const uint32_t* const src = stage + k * stride_words;
        const uint8_t* const srcb = reinterpret_cast<const uint8_t*>(src);
        const uint32_t len = lens[k];
        uint8_t* const dst = blob + front + offs[k];
        uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
        if (head > len) head = len;
        if (t < head) dst[t] = srcb[t];
        const uint32_t nwords = (len - head) / 4;
        uint32_t* const dstw = reinterpret_cast<uint32_t*>(dst + head);
        const uint32_t sh = 8 * (head & 3);
        for (uint32_t j = t; j < nwords; j += kGatherThreads) {
            // bytes head + 4j .. head + 4j + 3 of the region: from one source word, or two
            const uint32_t w = (head >> 2) + j;
            uint32_t v = src[w];
            if (sh) v = (v >> sh) | (src[w + 1] << (32 - sh));  // (word w + 1 starts below len <= the stride)
            dstw[j] = v;
        }
        const uint32_t done = head + 4 * nwords;
        if (t < len - done) dst[done + t] = srcb[done + t];
    }
}

// kList: lane j of the grid takes segment ids[j], j < nlist (ascending ids below nseg: the host made the list); otherwise
// segment j, and ids / nlist are not looked at.  flags[] is indexed by the segment either way.
template <bool kList>
__global__ __launch_bounds__(kLanes) void k_seg_decode(const uint8_t* blob, size_t blob_len, const unsigned long long* offs, PlaneRef sym, size_t n,
                                                       uint32_t seg, uint32_t nseg, uint32_t brick, uint32_t* flags, unsigned int* bad,
                                                       const uint32_t* ids, uint32_t nlist)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    size_t k = (size_t)blockIdx.x * kLanes + lane;
    if (kList) {
        if (k >= nlist) return;
        k = ids[k];
    }
    if (k >= nseg) return;
    LdsTable t{tab + lane};
    const size_t base = k * seg;
    const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
    // (the host has validated the index: the streams lie inside the blob, in order, each no longer than a segment can be)
    const size_t front = wrseg::header_bytes(brick) + 4 * (size_t)nseg;
    const unsigned long long o0 = offs[k], o1 = offs[k + 1];
    uint32_t why = wrseg::kSegOverflow;
    if (o1 >= o0 && front + o1 <= blob_len && o1 - o0 <= wrseg::stream_bound(seg)) {
        wrseg::Dec d;
        d.in.open(blob + front + o0, (uint32_t)(o1 - o0), blob, blob + blob_len);
        SymSink sink{SegSpan(sym, base, bs), bs, 0, 0};
        why = wrseg::decode_segment(d, t, sink, bs);
        sink.flush();
    }
    flags[k] = why;
    if (why != wrseg::kSegOk) atomicAdd(bad, 1u);
}

}  // namespace

size_t seg_stage_bytes(size_t n, unsigned seg)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const size_t stride = ((size_t)wrseg::stream_bound(seg) + 3) & ~(size_t)3;
    return 256 + ((8 * (nseg + 1) + 4 * nseg + 255) & ~(size_t)255) + nseg * stride;
}

void seg_encode(const PlaneRef& sym, size_t n, unsigned seg, uint8_t* stage, uint8_t* blob, size_t cap, unsigned long long* result_host,
                hipStream_t st, unsigned brick)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const uint32_t stride_words = (wrseg::stream_bound(seg) + 3) / 4;
    unsigned long long* const result = reinterpret_cast<unsigned long long*>(stage);
    unsigned long long* const offs = reinterpret_cast<unsigned long long*>(stage + 256);
    uint32_t* const lens = reinterpret_cast<uint32_t*>(offs + nseg + 1);
    uint32_t* const regions = reinterpret_cast<uint32_t*>(stage + 256 + ((8 * (nseg + 1) + 4 * nseg + 255) & ~(size_t)255));
    if (nseg)
        hipLaunchKernelGGL(k_seg_encode, dim3((unsigned)((nseg + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, sym, n, (uint32_t)seg, (uint32_t)nseg,
                           regions, stride_words, lens);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kScanThreads), 0, st, lens, (uint32_t)nseg, (uint32_t)seg, (uint32_t)brick, offs, blob, cap, result,
                       result_host);
    if (nseg) {
        const unsigned grid = (unsigned)(nseg < 65536 ? nseg : 65536);
        hipLaunchKernelGGL(k_seg_gather, dim3(grid), dim3(kGatherThreads), 0, st, regions, stride_words, lens, offs, (uint32_t)nseg, (uint32_t)brick, blob,
                           cap, result);
    }
}

size_t seg_decode_work_bytes(size_t nseg) { return 256 + ((8 * (nseg + 1) + 255) & ~(size_t)255) + 4 * nseg; }

void seg_decode(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, hipStream_t st, unsigned brick)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    if (!nseg) return;
    unsigned int* const bad = reinterpret_cast<unsigned int*>(work);
    (void)hipMemsetAsync(bad, 0, sizeof *bad, st);
    const unsigned long long* const offs = reinterpret_cast<const unsigned long long*>(work + 256);
    uint32_t* const flags = reinterpret_cast<uint32_t*>(work + 256 + ((8 * (nseg + 1) + 255) & ~(size_t)255));
    hipLaunchKernelGGL(k_seg_decode<false>, dim3((unsigned)((nseg + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym, n,
                       (uint32_t)seg, (uint32_t)nseg, (uint32_t)brick, flags, bad, (const uint32_t*)nullptr, 0u);
}

size_t seg_decode_list_work_bytes(size_t nseg, size_t nlist) { return ((seg_decode_work_bytes(nseg) + 255) & ~(size_t)255) + 4 * nlist; }

uint32_t* seg_decode_list_ids(uint8_t* work, size_t nseg) { return reinterpret_cast<uint32_t*>(work + ((seg_decode_work_bytes(nseg) + 255) & ~(size_t)255)); }

void seg_decode_list(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, size_t nlist, hipStream_t st,
                     unsigned brick)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    unsigned int* const bad = reinterpret_cast<unsigned int*>(work);
    (void)hipMemsetAsync(bad, 0, sizeof *bad, st);
    if (!nseg || !nlist) return;
    const unsigned long long* const offs = reinterpret_cast<const unsigned long long*>(work + 256);
    uint32_t* const flags = reinterpret_cast<uint32_t*>(work + 256 + ((8 * (nseg + 1) + 255) & ~(size_t)255));
    hipLaunchKernelGGL(k_seg_decode<true>, dim3((unsigned)((nlist + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym, n,
                       (uint32_t)seg, (uint32_t)nseg, (uint32_t)brick, flags, bad, seg_decode_list_ids(work, nseg), (uint32_t)nlist);
}

}  // namespace wrk
