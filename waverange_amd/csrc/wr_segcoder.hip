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
//
// What a lane does once it knows its segment -- code it, scan the lengths, copy a staged piece, decode a segment, code, gather
// or decode a strand -- is written once, in wr_segcoder_dev.h, for these kernels and the batched ones of wr_segbatch.hip.  A kernel here
// finds its segment (the grid index or an id list), hands the body its arguments as they stand, and stores what it returns.
#include "wr_kernels.h"
#include "wr_segbatch.h"
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
    if (k >= nseg) return;
    lens[k] = encode_segment_lane(LdsTable{tab + lane}, sym, SegView{n, seg, nseg}, k, stage + k * stride_words, stride_words);
}

__global__ __launch_bounds__(kScanThreads) void k_seg_scan(const uint32_t* lens, uint32_t nseg, uint32_t seg, uint32_t brick, unsigned long long* offs,
                                                           uint8_t* blob, size_t cap, unsigned long long* result,
                                                           unsigned long long* result_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    scan_lengths(part, &bad, threadIdx.x, lens, nseg, seg, brick, 0, offs, blob, cap, result, result_host);
}

// blob[header + index + offs[k] ...) := the first lens[k] bytes of segment k's staging region.  Nothing is written unless the
// whole blob fits under cap and every segment is good.
__global__ __launch_bounds__(kGatherThreads) void k_seg_gather(const uint32_t* stage, uint32_t stride_words, const uint32_t* lens,
                                                               const unsigned long long* offs, uint32_t nseg, uint32_t brick, uint8_t* blob,
                                                               size_t cap, const unsigned long long* result)
{
    if (result[0] > cap || result[1]) return;
    const size_t front = wrseg::header_bytes(brick) + 4 * (size_t)nseg;
    for (size_t k = blockIdx.x; k < nseg; k += gridDim.x) copy_piece(blob + front + offs[k], stage + k * stride_words, lens[k], threadIdx.x);
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
    const uint32_t why = decode_segment_lane(LdsTable{tab + lane}, sym, SegView{n, seg, nseg, brick, blob, blob_len, offs}, k);
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
//   k_strand_scan     k_seg_scan with the longer header (the same body: the header is a branch in it)
//   k_strand_gather   length words, T, the strands and the padding -> the record's place in the blob
//   k_strand_decode   lane (k, j): the record's length words, T -> its column (257 steps, redundantly: no cross-lane traffic),
//                     S_j -> the strand's symbols

__global__ __launch_bounds__(kLanes) void k_strand_encode(PlaneRef sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t K, uint32_t kshift, uint32_t L,
                                                          uint32_t* stage, uint32_t stride_words, uint32_t* lens, uint32_t* tlens, uint32_t* slens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x, j = lane & (K - 1);
    const size_t k = ((size_t)blockIdx.x * kLanes + lane) >> kshift;
    // all 64 lanes go through the body, to its barriers and shuffles: a lane past the end is not live
    const bool live = k < nseg;
    encode_strand_lane(tab, lane, sym, SegView{n, seg, nseg}, K, L, live, k, stage + k * stride_words, slens + k * K + j, tlens + k, lens + k);
}

// k_seg_scan for the WRS3 header.  strands != 0 (strand_encode's callers see to it): with 0 the body would write a WRS1 / WRS2 header
__global__ __launch_bounds__(kScanThreads) void k_strand_scan(const uint32_t* lens, uint32_t nseg, uint32_t seg, uint32_t brick, uint32_t strands,
                                                              unsigned long long* offs, uint8_t* blob, size_t cap, unsigned long long* result,
                                                              unsigned long long* result_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    scan_lengths(part, &bad, threadIdx.x, lens, nseg, seg, brick, strands, offs, blob, cap, result, result_host);
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
    for (size_t k = blockIdx.x; k < nseg; k += gridDim.x)
        gather_record(blob + front + offs[k], stage + k * stride_words, tlens[k], slens + k * K, K, sb_words, lens[k], t);
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
    live = live && k < nseg;
    const uint32_t why = decode_strand_lane(LdsTable{tab + lane}, sym, SegView{n, seg, nseg, 0, blob, blob_len, offs}, K, L, j, live, k);
    if (live && j == 0) {
        flags[k] = why;
        if (why) atomicAdd(bad, 1u);
    }
}

// `stage` of an encode as its three kernels see it: {the blob's length, failed segments} at 0; at 256 the scan's arrays
// offs[nseg + 1] (u64), lens[nseg] and, stranded, tlens[nseg] and slens[nseg * strands]; then, 256-byte aligned, one region of
// stride_words per segment (the segment bound; stranded: the model's bound and `strands` regions of sb_words)
struct Stage {
    size_t nseg, at_regions, bytes;
    uint32_t sb_words, stride_words;
    Stage(size_t n, unsigned seg, unsigned strands) : nseg(wrseg::seg_count(n, seg))
    {
        // (in words what the layout is in bytes: the model's bound and a strand's, 2 L + 8 with L a multiple of 16, divide by 4)
        static_assert(wrseg::kModelBound % 4 == 0, "a record's region is carved in words");
        sb_words = strands ? wrseg::strand_bound(wrseg::strand_len(seg, strands)) / 4 : 0;
        stride_words = strands ? wrseg::kModelBound / 4 + strands * sb_words : (wrseg::stream_bound(seg) + 3) / 4;
        at_regions = 256 + up256(8 * (nseg + 1) + 4 * nseg * (strands ? 2 + (size_t)strands : 1));
        bytes = at_regions + nseg * 4 * (size_t)stride_words;
    }
    unsigned long long* result(uint8_t* stage) const { return reinterpret_cast<unsigned long long*>(stage); }
    unsigned long long* offs(uint8_t* stage) const { return reinterpret_cast<unsigned long long*>(stage + 256); }
    uint32_t* lens(uint8_t* stage) const { return reinterpret_cast<uint32_t*>(offs(stage) + nseg + 1); }
    uint32_t* regions(uint8_t* stage) const { return reinterpret_cast<uint32_t*>(stage + at_regions); }
};

}  // namespace

size_t seg_stage_bytes(size_t n, unsigned seg) { return Stage(n, seg, 0).bytes; }

void seg_encode(const PlaneRef& sym, size_t n, unsigned seg, uint8_t* stage, uint8_t* blob, size_t cap, unsigned long long* result_host,
                hipStream_t st, unsigned brick)
{
    const Stage sg(n, seg, 0);
    const size_t nseg = sg.nseg;
    unsigned long long* const result = sg.result(stage);
    unsigned long long* const offs = sg.offs(stage);
    uint32_t* const lens = sg.lens(stage);
    uint32_t* const regions = sg.regions(stage);
    if (nseg)
        hipLaunchKernelGGL(k_seg_encode, dim3((unsigned)((nseg + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, sym, n, (uint32_t)seg, (uint32_t)nseg,
                           regions, sg.stride_words, lens);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kScanThreads), 0, st, lens, (uint32_t)nseg, (uint32_t)seg, (uint32_t)brick, offs, blob, cap, result,
                       result_host);
    if (nseg) {
        const unsigned grid = (unsigned)(nseg < 65536 ? nseg : 65536);
        hipLaunchKernelGGL(k_seg_gather, dim3(grid), dim3(kGatherThreads), 0, st, regions, sg.stride_words, lens, offs, (uint32_t)nseg, (uint32_t)brick,
                           blob, cap, result);
    }
}

size_t strand_stage_bytes(size_t n, unsigned seg, unsigned strands) { return Stage(n, seg, strands).bytes; }

void strand_encode(const PlaneRef& sym, size_t n, unsigned seg, unsigned strands, unsigned brick, uint8_t* stage, uint8_t* blob, size_t cap,
                   unsigned long long* result_host, hipStream_t st)
{
    const Stage sg(n, seg, strands);
    const size_t nseg = sg.nseg;
    unsigned long long* const result = sg.result(stage);
    unsigned long long* const offs = sg.offs(stage);
    uint32_t* const lens = sg.lens(stage);
    uint32_t* const tlens = lens + nseg;
    uint32_t* const slens = tlens + nseg;
    uint32_t* const regions = sg.regions(stage);
    if (nseg)
        hipLaunchKernelGGL(k_strand_encode, dim3((unsigned)((nseg * strands + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, sym, n, (uint32_t)seg,
                           (uint32_t)nseg, (uint32_t)strands, wrsb::strands_shift(strands), wrseg::strand_len(seg, strands), regions, sg.stride_words, lens,
                           tlens, slens);
    hipLaunchKernelGGL(k_strand_scan, dim3(1), dim3(kScanThreads), 0, st, lens, (uint32_t)nseg, (uint32_t)seg, (uint32_t)brick, (uint32_t)strands, offs, blob,
                       cap, result, result_host);
    if (nseg) {
        const unsigned grid = (unsigned)(nseg < 65536 ? nseg : 65536);
        hipLaunchKernelGGL(k_strand_gather, dim3(grid), dim3(kGatherThreads), 0, st, regions, sg.stride_words, lens, tlens, slens, offs, (uint32_t)nseg,
                           (uint32_t)strands, sg.sb_words, blob, cap, result);
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
                           n, (uint32_t)seg, (uint32_t)nseg, (uint32_t)strands, wrsb::strands_shift(strands), wrseg::strand_len(seg, strands), flags, bad,
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
                           n, (uint32_t)seg, (uint32_t)nseg, (uint32_t)strands, wrsb::strands_shift(strands), wrseg::strand_len(seg, strands), flags, bad,
                           seg_decode_list_ids(work, nseg), (uint32_t)nlist);
        return;
    }
    hipLaunchKernelGGL(k_seg_decode<true>, dim3((unsigned)((nlist + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, blob, blob_len, offs, sym, n,
                       (uint32_t)seg, (uint32_t)nseg, (uint32_t)brick, flags, bad, seg_decode_list_ids(work, nseg), (uint32_t)nlist);
}

}  // namespace wrk
