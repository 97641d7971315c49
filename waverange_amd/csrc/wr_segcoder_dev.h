// wr_segcoder_dev.h -- what a lane of the segment coder kernels works with (its column of the wave's LDS table, the symbols of
// its segment in a plane, the sinks of coded words and decoded symbols) and, behind them, what it does: the seven lane programs.
// Shared by wr_segcoder.hip (one plane per launch) and wr_segbatch.hip (the planes of a batch of fields per launch).
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

// ---- the lane programs.  A kernel finds its segment (the grid index, an id list, or wrsb::locate in a job table), builds a
// SegView from its arguments or from a SegJob, calls the body with it and its plane, and stores what that returns.  Everything is inlined: the
// single-plane kernels keep their arguments in scalar registers.

constexpr int kScanThreads = 1024;
constexpr int kGatherThreads = 256;

__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// a plane's geometry and (for the decoders) its blob, as values in the kernel's registers.  The PlaneRef goes beside it as the
// kernel has it (an argument, or a job's in memory): as a member here it cost the single-plane decoders two VGPRs and
// turned their symbol stores from global into flat ones.
struct SegView {
    size_t n;
    uint32_t seg, nseg;
    uint32_t brick = 0;  // from here on: the decoders'
    const uint8_t* blob = nullptr;
    size_t blob_len = 0;
    const unsigned long long* offs = nullptr;  // (the host has validated the index they come from)
    __device__ size_t base(size_t k) const { return k * seg; }
    __device__ uint32_t len(size_t k) const { return n - base(k) < seg ? (uint32_t)(n - base(k)) : seg; }
};

// Segment k < nseg: histogram -> model -> stream, words appended to [region, region + stride_words).  Returns the stream's
// length, 0xffffffff if it did not fit (it cannot: the stride is the segment bound).  No barrier: a lane past the end need
// not come here.
__device__ inline uint32_t encode_segment_lane(LdsTable t, const PlaneRef& sym, const SegView& v, size_t k, uint32_t* region, uint32_t stride_words)
{
    for (uint32_t s = 0; s < 256; s++) t.set(s, 0);
    const uint32_t bs = v.len(k);
    PlaneSource src{SegSpan(sym, v.base(k), bs)};
    wrseg::build_model(t, src, bs);
    wrseg::Enc<WordSink> e;
    e.out = WordSink{region, stride_words * 4, 0, 0, false};
    wrseg::encode_segment(e, t, src, bs);
    e.out.flush();
    return e.out.overflow ? 0xffffffffu : e.out.pos;
}

// One workgroup of kScanThreads (t = threadIdx.x; part[kScanThreads] and *bad are its LDS) over a job's lens[0, nseg):
// offs[0 .. nseg] = their exclusive scan, result[0] = the blob's length, result[1] = segments (records) that did not fit
// their region (0 always: see encode_segment_lane); result_host (may be null) takes the same pair.  The blob's header -- WRS1,
// WRS2 with a brick, WRS3 with strands -- and its index are written if they fit under cap (the host has checked that before
// the launch).  A thread past the end of lens has k0 == k1 == nseg.
__device__ inline void scan_lengths(unsigned long long* part, unsigned int* bad, uint32_t t, const uint32_t* lens, uint32_t nseg, uint32_t seg,
                                    uint32_t brick, uint32_t strands, unsigned long long* offs, uint8_t* blob, size_t cap,
                                    unsigned long long* result, unsigned long long* result_host)
{
    const size_t head = wrseg::header_bytes(brick, strands);
    if (t == 0) *bad = 0;
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
    if (mybad) atomicAdd(bad, mybad);
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int j = 0; j < kScanThreads; j++) { const unsigned long long v = part[j]; part[j] = run; run += v; }
        const unsigned long long total = head + 4ull * nseg + run;
        offs[nseg] = run;
        result[0] = total; result[1] = *bad;
        if (result_host) { result_host[0] = total; result_host[1] = *bad; }
        if (cap >= head) {
            uint32_t* const h = reinterpret_cast<uint32_t*>(blob);
            const uint8_t* const mg = strands ? wrseg::kMagicStrands : brick ? wrseg::kMagicBlocked : wrseg::kMagic;
            h[0] = (uint32_t)mg[0] | (uint32_t)mg[1] << 8 | (uint32_t)mg[2] << 16 | (uint32_t)mg[3] << 24;
            h[1] = seg; h[2] = nseg;
            if (strands) { h[3] = brick; h[4] = strands; }
            else if (brick) h[3] = brick;
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

// dst[0, len) := the first len bytes at src (word aligned), by the kGatherThreads threads of a block (t = threadIdx.x):
// coalesced, destination-aligned words
__device__ inline void copy_piece(uint8_t* dst, const uint32_t* src, uint32_t len, uint32_t t)
{
    const uint8_t* const srcb = reinterpret_cast<const uint8_t*>(src);
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > len) head = len;
    if (t < head) dst[t] = srcb[t];
    const uint32_t nwords = (len - head) / 4;
    uint32_t* const dstw = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t sh = 8 * (head & 3);
    for (uint32_t j = t; j < nwords; j += kGatherThreads) {
        // bytes head + 4j .. head + 4j + 3 of the piece: from one source word, or two
        const uint32_t w = (head >> 2) + j;
        uint32_t v = src[w];
        if (sh) v = (v >> sh) | (src[w + 1] << (32 - sh));  // (word w + 1 starts below len <= the piece's region)
        dstw[j] = v;
    }
    const uint32_t done = head + 4 * nwords;
    if (t < len - done) dst[done + t] = srcb[done + t];
}

// Segment k < nseg: its stream (at offs[k] behind the index) -> the plane's symbols [k * seg, k * seg + bs).  Returns the
// segment's flag (wrseg::kSegOk: decoded).  A lane writes only its segment's symbols.  No barrier: a lane without a segment
// need not come here.
__device__ inline uint32_t decode_segment_lane(LdsTable t, const PlaneRef& sym, const SegView& v, size_t k)
{
    const uint32_t bs = v.len(k);
    // (the streams lie inside the blob, in order, each no longer than a segment can be: checked again, it costs nothing)
    const size_t front = wrseg::header_bytes(v.brick) + 4 * (size_t)v.nseg;
    const unsigned long long o0 = v.offs[k], o1 = v.offs[k + 1];
    uint32_t why = wrseg::kSegOverflow;
    if (o1 >= o0 && front + o1 <= v.blob_len && o1 - o0 <= wrseg::stream_bound(v.seg)) {
        wrseg::Dec d;
        d.in.open(v.blob + front + o0, (uint32_t)(o1 - o0), v.blob, v.blob + v.blob_len);
        SymSink sink{SegSpan(sym, v.base(k), bs), bs, 0, 0};
        why = wrseg::decode_segment(d, t, sink, bs);
        sink.flush();
    }
    return why;
}

// Strand j of segment k's record (WRS3, K strands of L symbols): the record's length words, T -> the lane's column (257 steps,
// redundantly: no cross-lane traffic), S_j -> the strand's symbols.  Returns the OR of `why` over the K lanes of the segment
// (0: decoded), which sit side by side in one wave.  EVERY lane of the wave comes here and nobody leaves before the shuffles:
// a lane past the end, a padding lane or one whose id is no segment has live == false (k is then not looked at) and adds 0.
// The K lanes of a segment agree on live and k.
__device__ inline uint32_t decode_strand_lane(LdsTable t, const PlaneRef& sym, const SegView& v, uint32_t K, uint32_t L, uint32_t j, bool live, size_t k)
{
    uint32_t why = 0;
    if (live) {
        const size_t base = v.base(k);
        const uint32_t bs = v.len(k);
        // (the records lie inside the blob, in order, aligned, each no longer than one can be: checked again)
        const size_t front = wrseg::kHeaderBytesStrands + 4 * (size_t)v.nseg;
        const unsigned long long o0 = v.offs[k], o1 = v.offs[k + 1];
        const uint8_t* const rec = v.blob + front + o0;
        why = wrseg::kRecOverflow;
        if (o1 >= o0 && front + o1 <= v.blob_len && o1 - o0 <= wrseg::record_bound(v.seg, K) && !(reinterpret_cast<uintptr_t>(rec) & 3)) {
            uint32_t tlen = 0, off = 0, len = 0;
            why = wrseg::check_record(rec, (size_t)(o1 - o0), K, L, bs, j, &tlen, &off, &len);
            wrseg::Dec d;
            if (!why) {
                d.in.open(rec + 4 * (size_t)(K + 1), tlen, v.blob, v.blob + v.blob_len);
                why = wrseg::decode_model(d, t, bs);
            }
            const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
            if (!why && m) {
                d.in.open(rec + off, len, v.blob, v.blob + v.blob_len);
                SymSink sink{SegSpan(sym, base + s0, m), m, 0, 0};
                why = wrseg::decode_strand(d, t, sink, m, bs);
                sink.flush();
            }
        }
    }
    for (uint32_t off = 1; off < K; off <<= 1) why |= __shfl_xor(why, (int)off);
    return why;
}

// The encoder's side of a record.  Lane `lane` of the wave is strand j = lane & (K - 1) of segment k: histogram of the strand
// into the lane's column -> the K columns of the segment summed, the sum in all K of them -> the segment's model -> S_j into
// its own piece of the record's staging region [region, region + kModelBound / 4 + K * strand_bound(L) / 4); strand 0 also T,
// at the region's start.  A live lane stores the strand's length at *slen as soon as it has it; strand 0's lane then T's length
// at *tlen and the record's at *len, 0xffffffff if a piece outgrew its bound (it cannot: the pieces are the bounds).  tab: the
// wave's whole table.  EVERY lane of the wave comes here and reaches both barriers and the shuffles: a lane past the end has
// live == false (k, region and the three places are then not looked at) and, like the lane of an empty strand, m == 0.  The K lanes of a segment
// agree on live, k and region; different groups of a wave may belong to different planes.
__device__ inline void encode_strand_lane(uint32_t* tab, uint32_t lane, const PlaneRef& sym, const SegView& v, uint32_t K, uint32_t L, bool live, size_t k,
                                              uint32_t* region, uint32_t* slen_at, uint32_t* tlen_at, uint32_t* len_at)
{
    const uint32_t j = lane & (K - 1), g0 = lane - j;
    const size_t base = live ? v.base(k) : 0;
    const uint32_t bs = live ? v.len(k) : 0;
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
    if (live) *slen_at = slen;
    uint32_t sum = tlen + slen;
    for (uint32_t off = 1; off < K; off <<= 1) {
        sum += __shfl_xor(sum, (int)off);
        over |= __shfl_xor(over, (int)off);
    }
    if (live && j == 0) {
        *tlen_at = tlen;
        *len_at = over ? 0xffffffffu : (4 * (K + 1) + sum + 3) & ~3u;
    }
}

// rec[0, len) := a record from its staging region, by the kGatherThreads threads of a block (t = threadIdx.x): the length
// words (tlen, then slens[0, K)), T, the strands behind one another, and zeros up to len.  rec is 4-byte aligned: the blob
// is, and every length before it is a multiple of 4.
__device__ inline void gather_record(uint8_t* rec, const uint32_t* region, uint32_t tlen, const uint32_t* slens, uint32_t K, uint32_t sb_words, uint32_t len,
                                     uint32_t t)
{
    if (t == 0) reinterpret_cast<uint32_t*>(rec)[0] = tlen;
    else if (t <= K) reinterpret_cast<uint32_t*>(rec)[t] = slens[t - 1];
    uint32_t at = 4 * (K + 1);
    copy_piece(rec + at, region, tlen, t);
    at += tlen;
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t sl = slens[j];
        if (sl) copy_piece(rec + at, region + wrseg::kModelBound / 4 + j * sb_words, sl, t);
        at += sl;
    }
    if (t < len - at) rec[at + t] = 0;
}

}  // namespace

}  // namespace wrk

#endif
