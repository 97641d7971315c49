// wr_segcoder.hip -- the segmented plane streams ("WRS1" and, further down, "WRS3"; wr_segcoder.h) coded and decoded on the GPU.
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
#include "wr_segcoder_dev.h"

namespace wrk {

namespace {

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

// ---- stranded segments ("WRS3", wr_segcoder.h): one lane per STRAND ---------------------------------------------------------
// Lane g of the grid is (segment g / K, strand g % K); K divides 64, so the K lanes of a segment sit side by side in one
// wave.  Every lane keeps a private column of tab[256][64] as above -- the look-ups stay conflict-free -- and the K columns of
// a segment all hold that segment's model.
//
//   k_strand_encode   lane (k, j): histogram of strand j -> the segment's model in all K columns -> S_j into its own staging
//                     region; lane (k, 0) also T.  tlens[k], slens[k * K + j], lens[k] = the record's length
//   k_strand_scan     k_seg_scan with the longer header
//   k_strand_gather   length words, T, the strands and the padding -> the record's place in the blob
//   k_strand_decode   lane (k, j): the record's length words, T -> its column (257 steps, redundantly: no cross-lane traffic),
//                     S_j -> the strand's symbols

__global__ __launch_bounds__(kLanes) void k_strand_encode(PlaneRef sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t K, uint32_t kshift, uint32_t L,
                                                          uint32_t* stage, uint32_t stride_words, uint32_t* lens, uint32_t* tlens, uint32_t* slens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x, j = lane & (K - 1), g0 = lane - j;
    const size_t k = ((size_t)blockIdx.x * kLanes + lane) >> kshift;
    // all 64 lanes reach both barriers and the shuffles below: a lane past the end, or of an empty strand, has m == 0
    const bool live = k < nseg;
    const size_t base = live ? k * seg : 0;
    const uint32_t bs = !live ? 0 : n - base < seg ? (uint32_t)(n - base) : seg;
    const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
    LdsTable t{tab + lane};
    for (uint32_t s = 0; s < 256; s++) t.set(s, 0);
    PlaneSource src{SegSpan(sym, m ? base + s0 : 0, m)};
    if (m) wrseg::count_symbols(t, src, m);
    __syncthreads();
    // The K partial counts of a symbol row -> their sum, into all K columns.  Rows s = j, j + K, ... are lane j's and nobody
    // else's between the two barriers, so no lane reads a row that another one is writing.  At step i the K lanes of a
    // group are in K different columns (banks), and different groups in different columns anyway.
    for (uint32_t s = j; s < 256; s += K) {
        uint32_t* const row = tab + s * kLanes + g0;
        uint32_t c = 0;
        for (uint32_t i = 0; i < K; i++) c += row[(i + j) & (K - 1)];
        for (uint32_t i = 0; i < K; i++) row[(i + j) & (K - 1)] = c;
    }
    __syncthreads();
    wrseg::counts_to_model(t);
    const uint32_t sb = wrseg::strand_bound(L);
    uint32_t* const region = live ? stage + k * stride_words : stage;  // (only used by live lanes)
    uint32_t tlen = 0, slen = 0, over = 0;
    if (live && j == 0) {
        wrseg::Enc<WordSink> e;
        e.out = WordSink{region, wrseg::kModelBound, 0, 0, false};
        wrseg::encode_model(e, t);
        e.out.flush();
        tlen = e.out.pos;
        over |= e.out.overflow;
    }
    if (m) {
        wrseg::Enc<WordSink> e;
        e.out = WordSink{region + wrseg::kModelBound / 4 + j * (sb / 4), sb, 0, 0, false};
        wrseg::encode_strand(e, t, src, m, bs);
        e.out.flush();
        slen = e.out.pos;
        over |= e.out.overflow;  // (cannot happen: the regions are the bounds)
    }
    if (live) slens[k * K + j] = slen;
    uint32_t sum = tlen + slen;
    for (uint32_t off = 1; off < K; off <<= 1) {
        sum += __shfl_xor(sum, (int)off);
        over |= __shfl_xor(over, (int)off);
    }
    if (live && j == 0) {
        tlens[k] = tlen;
        lens[k] = over ? 0xffffffffu : (4 * (K + 1) + sum + 3) & ~3u;
    }
}

// k_seg_scan for the WRS3 header: result[0] = the blob's length, result[1] = records that did not fit their regions (0 always)
__global__ __launch_bounds__(kScanThreads) void k_strand_scan(const uint32_t* lens, uint32_t nseg, uint32_t seg, uint32_t brick, uint32_t strands,
                                                              unsigned long long* offs, uint8_t* blob, size_t cap, unsigned long long* result,
                                                              unsigned long long* result_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    const uint32_t t = threadIdx.x;
    const size_t head = wrseg::kHeaderBytesStrands;
    if (t == 0) bad = 0;
    __syncthreads();
    const uint32_t per = (nseg + kScanThreads - 1) / kScanThreads;
    const size_t k0 = (size_t)t * per < nseg ? (size_t)t * per : nseg, k1 = k0 + per < nseg ? k0 + per : nseg;
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
            const uint8_t* const mg = wrseg::kMagicStrands;
            h[0] = (uint32_t)mg[0] | (uint32_t)mg[1] << 8 | (uint32_t)mg[2] << 16 | (uint32_t)mg[3] << 24;
            h[1] = seg; h[2] = nseg; h[3] = brick; h[4] = strands;
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

// dst[0, len) := the first len bytes at src (word aligned), by the block's threads: destination-aligned words
__device__ void copy_piece(uint8_t* dst, const uint32_t* src, uint32_t len, uint32_t t)
{
    const uint8_t* const srcb = reinterpret_cast<const uint8_t*>(src);
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > len) head = len;
    if (t < head) dst[t] = srcb[t];
    const uint32_t nwords = (len - head) / 4;
    uint32_t* const dstw = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t sh = 8 * (head & 3);
    for (uint32_t j = t; j < nwords; j += kGatherThreads) {
        const uint32_t w = (head >> 2) + j;
        uint32_t v = src[w];
        if (sh) v = (v >> sh) | (src[w + 1] << (32 - sh));  // (word w + 1 starts below len <= the piece's region)
        dstw[j] = v;
    }
    const uint32_t done = head + 4 * nwords;
    if (t < len - done) dst[done + t] = srcb[done + t];
}

// record k := its length words, T, its strands and the padding, at front + offs[k] of the blob.  Nothing is written unless the
// whole blob fits under cap and every record is good.
__global__ __launch_bounds__(kGatherThreads) void k_strand_gather(const uint32_t* stage, uint32_t stride_words, const uint32_t* lens, const uint32_t* tlens,
                                                                  const uint32_t* slens, const unsigned long long* offs, uint32_t nseg, uint32_t K,
                                                                  uint32_t sb_words, uint8_t* blob, size_t cap, const unsigned long long* result)
{
    if (result[0] > cap || result[1]) return;
    const size_t front = wrseg::kHeaderBytesStrands + 4 * (size_t)nseg;
    const uint32_t t = threadIdx.x;
    for (size_t k = blockIdx.x; k < nseg; k += gridDim.x) {
        const uint32_t* const region = stage + k * stride_words;
        uint8_t* const rec = blob + front + offs[k];  // 4-byte aligned: the blob is, and every length before it is a multiple of 4
        const uint32_t tlen = tlens[k];
        if (t == 0) reinterpret_cast<uint32_t*>(rec)[0] = tlen;
        else if (t <= K) reinterpret_cast<uint32_t*>(rec)[t] = slens[k * K + t - 1];
        uint32_t at = 4 * (K + 1);
        copy_piece(rec + at, region, tlen, t);
        at += tlen;
        for (uint32_t j = 0; j < K; j++) {
            const uint32_t sl = slens[k * K + j];
            if (sl) copy_piece(rec + at, region + wrseg::kModelBound / 4 + j * sb_words, sl, t);
            at += sl;
        }
        if (t < lens[k] - at) rec[at + t] = 0;
    }
}

// kList as k_seg_decode: the grid's lane groups take the segments ids[0 .. nlist), otherwise the segments 0 .. nseg.
template <bool kList>
__global__ __launch_bounds__(kLanes) void k_strand_decode(const uint8_t* blob, size_t blob_len, const unsigned long long* offs, PlaneRef sym, size_t n,
                                                          uint32_t seg, uint32_t nseg, uint32_t K, uint32_t kshift, uint32_t L, uint32_t* flags,
                                                          unsigned int* bad, const uint32_t* ids, uint32_t nlist)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x, j = lane & (K - 1);
    size_t k = ((size_t)blockIdx.x * kLanes + lane) >> kshift;
    bool live = true;
    if (kList) {
        live = k < nlist;
        k = live ? ids[k] : 0;
    }
    live = live && k < nseg;  // (the K lanes of a segment agree; nobody returns before the shuffles)
    uint32_t why = 0;
    if (live) {
        LdsTable t{tab + lane};
        const size_t base = k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        // (the host has validated the index: the records lie inside the blob, in order, aligned, each no longer than one can be)
        const size_t front = wrseg::kHeaderBytesStrands + 4 * (size_t)nseg;
        const unsigned long long o0 = offs[k], o1 = offs[k + 1];
        const uint8_t* const rec = blob + front + o0;
        why = wrseg::kRecOverflow;
        if (o1 >= o0 && front + o1 <= blob_len && o1 - o0 <= wrseg::record_bound(seg, K) && !(reinterpret_cast<uintptr_t>(rec) & 3)) {
            uint32_t tlen = 0, off = 0, len = 0;
            why = wrseg::check_record(rec, (size_t)(o1 - o0), K, L, bs, j, &tlen, &off, &len);
            wrseg::Dec d;
            if (!why) {
                d.in.open(rec + 4 * (size_t)(K + 1), tlen, blob, blob + blob_len);
                why = wrseg::decode_model(d, t, bs);
            }
            const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
            if (!why && m) {
                d.in.open(rec + off, len, blob, blob + blob_len);
                SymSink sink{SegSpan(sym, base + s0, m), m, 0, 0};
                why = wrseg::decode_strand(d, t, sink, m, bs);
                sink.flush();
            }
        }
    }
    for (uint32_t off = 1; off < K; off <<= 1) why |= __shfl_xor(why, (int)off);
    if (live && j == 0) {
        flags[k] = why;
        if (why) atomicAdd(bad, 1u);
    }
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

static uint32_t log2_of(unsigned k)  // k: a power of two
{
    uint32_t s = 0;
    while ((1u << s) < k) s++;
    return s;
}

// the scan's arrays of a stranded encode: offs[nseg + 1] (u64), lens[nseg], tlens[nseg], slens[nseg * K]
static size_t strand_arrays_bytes(size_t nseg, unsigned strands) { return (8 * (nseg + 1) + 4 * nseg * (2 + (size_t)strands) + 255) & ~(size_t)255; }

size_t strand_stage_bytes(size_t n, unsigned seg, unsigned strands)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const size_t stride = wrseg::kModelBound + (size_t)strands * wrseg::strand_bound(wrseg::strand_len(seg, strands));
    return 256 + strand_arrays_bytes(nseg, strands) + nseg * stride;
}

void strand_encode(const PlaneRef& sym, size_t n, unsigned seg, unsigned strands, unsigned brick, uint8_t* stage, uint8_t* blob, size_t cap,
                   unsigned long long* result_host, hipStream_t st)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const uint32_t L = wrseg::strand_len(seg, strands), sb_words = wrseg::strand_bound(L) / 4;
    const uint32_t stride_words = wrseg::kModelBound / 4 + strands * sb_words;
    unsigned long long* const result = reinterpret_cast<unsigned long long*>(stage);
    unsigned long long* const offs = reinterpret_cast<unsigned long long*>(stage + 256);
    uint32_t* const lens = reinterpret_cast<uint32_t*>(offs + nseg + 1);
    uint32_t* const tlens = lens + nseg;
    uint32_t* const slens = tlens + nseg;
    uint32_t* const regions = reinterpret_cast<uint32_t*>(stage + 256 + strand_arrays_bytes(nseg, strands));
    if (nseg)
        hipLaunchKernelGGL(k_strand_encode, dim3((unsigned)((nseg * strands + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, sym, n, (uint32_t)seg,
                           (uint32_t)nseg, (uint32_t)strands, log2_of(strands), L, regions, stride_words, lens, tlens, slens);
    hipLaunchKernelGGL(k_strand_scan, dim3(1), dim3(kScanThreads), 0, st, lens, (uint32_t)nseg, (uint32_t)seg, (uint32_t)brick, (uint32_t)strands, offs, blob,
                       cap, result, result_host);
    if (nseg) {
        const unsigned grid = (unsigned)(nseg < 65536 ? nseg : 65536);
        hipLaunchKernelGGL(k_strand_gather, dim3(grid), dim3(kGatherThreads), 0, st, regions, stride_words, lens, tlens, slens, offs, (uint32_t)nseg,
                           (uint32_t)strands, sb_words, blob, cap, result);
    }
}

size_t seg_decode_work_bytes(size_t nseg) { return seg_work_flags_at(nseg) + 4 * nseg; }

void seg_decode(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, hipStream_t st, unsigned brick,
                unsigned strands)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    if (!nseg) return;
    unsigned int* const bad = seg_work_bad(work);
    (void)hipMemsetAsync(bad, 0, sizeof *bad, st);
    const unsigned long long* const offs = seg_work_offs(work);
    uint32_t* const flags = seg_work_flags(work, nseg);
    if (strands) {
        hipLaunchKernelGGL(k_strand_decode<false>, dim3((unsigned)((nseg * strands + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym,
                           n, (uint32_t)seg, (uint32_t)nseg, (uint32_t)strands, log2_of(strands), wrseg::strand_len(seg, strands), flags, bad,
                           (const uint32_t*)nullptr, 0u);
        return;
    }
    hipLaunchKernelGGL(k_seg_decode<false>, dim3((unsigned)((nseg + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym, n,
                       (uint32_t)seg, (uint32_t)nseg, (uint32_t)brick, flags, bad, (const uint32_t*)nullptr, 0u);
}

size_t seg_decode_list_work_bytes(size_t nseg, size_t nlist) { return ((seg_decode_work_bytes(nseg) + 255) & ~(size_t)255) + 4 * nlist; }

uint32_t* seg_decode_list_ids(uint8_t* work, size_t nseg) { return reinterpret_cast<uint32_t*>(work + ((seg_decode_work_bytes(nseg) + 255) & ~(size_t)255)); }

void seg_decode_list(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, size_t nlist, hipStream_t st,
                     unsigned brick, unsigned strands)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    unsigned int* const bad = seg_work_bad(work);
    (void)hipMemsetAsync(bad, 0, sizeof *bad, st);
    if (!nseg || !nlist) return;
    const unsigned long long* const offs = seg_work_offs(work);
    uint32_t* const flags = seg_work_flags(work, nseg);
    if (strands) {
        hipLaunchKernelGGL(k_strand_decode<true>, dim3((unsigned)((nlist * strands + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym,
                           n, (uint32_t)seg, (uint32_t)nseg, (uint32_t)strands, log2_of(strands), wrseg::strand_len(seg, strands), flags, bad,
                           seg_decode_list_ids(work, nseg), (uint32_t)nlist);
        return;
    }
    hipLaunchKernelGGL(k_seg_decode<true>, dim3((unsigned)((nlist + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym, n,
                       (uint32_t)seg, (uint32_t)nseg, (uint32_t)brick, flags, bad, seg_decode_list_ids(work, nseg), (uint32_t)nlist);
}

}  // namespace wrk
