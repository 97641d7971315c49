// wr_segbatch.hip -- the segment coder of wr_segcoder.hip over the planes of a BATCH of fields: one launch per plane index.
//
// A plane's coder kernel takes as long as its longest segment's chain, however few lanes it has: a 128^3 plane is 36 lanes, one
// wave on one CU.  Here plane l of all fields of a batch goes into one launch, one lane per segment of any of them, so N small
// fields take one field's coder time until the device's resident waves are used up.  A job is one (field, plane); the job
// table and first[], the exclusive prefix of the jobs' segment counts, lie in device memory, and lane g of the grid finds
// its job by a binary search in first[] (wr_segbatch.h: ten steps at most, against tens of thousands of coder steps).
//
//   k_seg_encode_batch   k_seg_encode behind the locator: lane g codes segment g - first[j] of job j into region g of the
//                        staging buffer; lens[g] = its length
//   k_seg_scan_batch     one workgroup per job: k_seg_scan on the job's slice of lens -> the job's offs, header, index, result
//   k_seg_gather_batch   k_seg_gather with the job found per segment
//   k_seg_decode_batch   k_seg_decode<false> behind the locator; flags and the count of failed segments are per job
//   k_seg_decode_list_batch   k_seg_decode<true> behind the locator: a job carries an ascending list of segment ids, first[] is
//                        the exclusive prefix of the jobs' LIST LENGTHS, and lane g takes segment ids[g - first[j]] of job j.  The
//                        planes of one stream, each with the union of the segments some regions need, go into one launch.
//   k_strand_decode_list_batch   (at the end of the file) k_strand_decode<true> behind the locator: the WRS3 jobs of a region
//                        decode over a batch of fields; a job's lanes are its list length times K, rounded up to a whole wave.
//
// The coder steps are wr_segcoder.h's and the lane's tools wr_segcoder_dev.h's, as in wr_segcoder.hip: every blob is byte for
// byte the single-plane kernels' blob.
#include "wr_kernels.h"
#include "wr_segbatch.h"
#include "wr_segcoder.h"
#include "wr_segcoder_dev.h"

namespace wrk {

namespace {

__global__ __launch_bounds__(kLanes) void k_seg_encode_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, uint32_t* stage,
                                                             uint32_t stride_words, uint32_t* lens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    LdsTable t{tab + lane};
    for (uint32_t s = 0; s < 256; s++) t.set(s, 0);
    if (g >= first[njobs]) return;  // (no barrier in this kernel: a lane past the end may go)
    uint32_t j, k;
    wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
    const SegJob& job = jobs[j];
    const size_t n = job.n;
    const uint32_t seg = job.seg;
    const size_t base = (size_t)k * seg;
    const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
    PlaneSource src{SegSpan(job.sym, base, bs)};
    wrseg::build_model(t, src, bs);
    wrseg::Enc<WordSink> e;
    e.out = WordSink{stage + g * stride_words, stride_words * 4, 0, 0, false};
    wrseg::encode_segment(e, t, src, bs);
    e.out.flush();
    lens[g] = e.out.overflow ? 0xffffffffu : e.out.pos;  // (cannot overflow: the stride is the segment bound)
}

constexpr int kScanThreads = 1024;

// Block j: results[2j] = the blob's length of job j, results[2j + 1] = its segments that did not fit their region (0 always).
// The blob's header and index are written if they fit under the job's cap (the host has checked that before the launch).
__global__ __launch_bounds__(kScanThreads) void k_seg_scan_batch(const SegJob* jobs, const uint32_t* first, const uint32_t* lens_all,
                                                                 unsigned long long* results, unsigned long long* results_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    const uint32_t t = threadIdx.x, j = blockIdx.x;
    const SegJob& job = jobs[j];
    const uint32_t nseg = job.nseg, seg = job.seg, brick = job.brick;
    const uint32_t* const lens = lens_all + first[j];
    unsigned long long* const offs = job.offs;
    uint8_t* const blob = job.blob;
    const size_t cap = job.cap;
    const size_t head = wrseg::header_bytes(brick);
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
        for (int i = 0; i < kScanThreads; i++) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        const unsigned long long total = head + 4ull * nseg + run;
        offs[nseg] = run;
        results[2 * j] = total; results[2 * j + 1] = bad;
        if (results_host) { results_host[2 * j] = total; results_host[2 * j + 1] = bad; }
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

// Segment g of the launch is segment k of job j: blob_j[header + index + offs_j[k] ...) := the first lens[g] bytes of region g.
// Nothing of a job is written unless its whole blob fits under its cap and its every segment is good.
__global__ __launch_bounds__(kGatherThreads) void k_seg_gather_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, const uint32_t* stage,
                                                                     uint32_t stride_words, const uint32_t* lens, const unsigned long long* results)
{
    const uint32_t t = threadIdx.x;
    const size_t total = first[njobs];
    for (size_t g = blockIdx.x; g < total; g += gridDim.x) {
        uint32_t j, k;
        wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
        const SegJob& job = jobs[j];
        if (results[2 * j] > job.cap || results[2 * j + 1]) continue;
        const size_t front = wrseg::header_bytes(job.brick) + 4 * (size_t)job.nseg;
        const uint32_t* const src = stage + g * stride_words;
        const uint8_t* const srcb = reinterpret_cast<const uint8_t*>(src);
        const uint32_t len = lens[g];
        uint8_t* const dst = job.blob + front + job.offs[k];
        uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
        if (head > len) head = len;
        if (t < head) dst[t] = srcb[t];
        const uint32_t nwords = (len - head) / 4;
        uint32_t* const dstw = reinterpret_cast<uint32_t*>(dst + head);
        const uint32_t sh = 8 * (head & 3);
        for (uint32_t i = t; i < nwords; i += kGatherThreads) {
            // bytes head + 4i .. head + 4i + 3 of the region: from one source word, or two
            const uint32_t w = (head >> 2) + i;
            uint32_t v = src[w];
            if (sh) v = (v >> sh) | (src[w + 1] << (32 - sh));  // (word w + 1 starts below len <= the stride)
            dstw[i] = v;
        }
        const uint32_t done = head + 4 * nwords;
        if (t < len - done) dst[done + t] = srcb[done + t];
    }
}

__global__ __launch_bounds__(kLanes) void k_seg_decode_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    if (g >= first[njobs]) return;
    uint32_t j, k;
    wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
    const SegJob& job = jobs[j];
    LdsTable t{tab + lane};
    const size_t n = job.n;
    const uint32_t seg = job.seg, nseg = job.nseg;
    const uint8_t* const blob = job.blob;
    const size_t blob_len = job.cap;
    const size_t base = (size_t)k * seg;
    const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
    // (the host has validated the index: the streams lie inside the blob, in order, each no longer than a segment can be)
    const size_t front = wrseg::header_bytes(job.brick) + 4 * (size_t)nseg;
    const unsigned long long o0 = job.offs[k], o1 = job.offs[k + 1];
    uint32_t why = wrseg::kSegOverflow;
    if (o1 >= o0 && front + o1 <= blob_len && o1 - o0 <= wrseg::stream_bound(seg)) {
        wrseg::Dec d;
        d.in.open(blob + front + o0, (uint32_t)(o1 - o0), blob, blob + blob_len);
        SymSink sink{SegSpan(job.sym, base, bs), bs, 0, 0};
        why = wrseg::decode_segment(d, t, sink, bs);
        sink.flush();
    }
    job.flags[k] = why;
    if (why != wrseg::kSegOk) atomicAdd(job.bad, 1u);
}

// Lane g is position i of the list of job j: it decodes segment ids[i] of that job, as lane i of k_seg_decode<true> launched
// for the job alone would.  No barrier: a lane past the end may go.
__global__ __launch_bounds__(kLanes) void k_seg_decode_list_batch(const SegJob* jobs, const SegList* lists, const uint32_t* first, uint32_t njobs)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    if (g >= first[njobs]) return;
    uint32_t j, i;
    wrsb::locate(first, njobs, (uint32_t)g, &j, &i);
    const SegJob& job = jobs[j];
    const size_t k = lists[j].ids[i];
    const uint32_t seg = job.seg, nseg = job.nseg;
    if (k >= nseg) return;  // (the host made the list: every id is below nseg)
    LdsTable t{tab + lane};
    const size_t n = job.n;
    const uint8_t* const blob = job.blob;
    const size_t blob_len = job.cap;
    const size_t base = k * seg;
    const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
    // (the host has validated the index: the streams lie inside the blob, in order, each no longer than a segment can be)
    const size_t front = wrseg::header_bytes(job.brick) + 4 * (size_t)nseg;
    const unsigned long long o0 = job.offs[k], o1 = job.offs[k + 1];
    uint32_t why = wrseg::kSegOverflow;
    if (o1 >= o0 && front + o1 <= blob_len && o1 - o0 <= wrseg::stream_bound(seg)) {
        wrseg::Dec d;
        d.in.open(blob + front + o0, (uint32_t)(o1 - o0), blob, blob + blob_len);
        SymSink sink{SegSpan(job.sym, base, bs), bs, 0, 0};
        why = wrseg::decode_segment(d, t, sink, bs);
        sink.flush();
    }
    job.flags[k] = why;
    if (why != wrseg::kSegOk) atomicAdd(job.bad, 1u);
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t seg_batch_table_bytes(size_t njobs) { return up256(njobs * sizeof(SegJob)) + up256(4 * (njobs + 1)); }

size_t seg_batch_table_fill(uint8_t* host_table, const SegJob* jobs, size_t njobs)
{
    memset(host_table, 0, seg_batch_table_bytes(njobs));
    memcpy(host_table, jobs, njobs * sizeof(SegJob));
    uint32_t* const first = reinterpret_cast<uint32_t*>(host_table + up256(njobs * sizeof(SegJob)));
    size_t run = 0;
    for (size_t j = 0; j < njobs; j++) { first[j] = (uint32_t)run; run += jobs[j].nseg; }
    first[njobs] = (uint32_t)run;
    return run;
}

size_t seg_batch_stage_bytes(size_t njobs, size_t n, unsigned seg)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const size_t stride = ((size_t)wrseg::stream_bound(seg) + 3) & ~(size_t)3;
    return seg_batch_table_bytes(njobs) + up256(16 * njobs) + up256(8 * (nseg + 1) * njobs) + up256(4 * nseg * njobs) + njobs * nseg * stride;
}

unsigned long long* seg_batch_results(uint8_t* stage, size_t njobs) { return reinterpret_cast<unsigned long long*>(stage + seg_batch_table_bytes(njobs)); }

void seg_encode_batch(SegJob* jobs, size_t njobs, size_t n, unsigned seg, uint8_t* host_table, uint8_t* stage, unsigned long long* result_host,
                      hipStream_t st)
{
    const size_t nseg = wrseg::seg_count(n, seg);
    const uint32_t stride_words = (wrseg::stream_bound(seg) + 3) / 4;
    unsigned long long* const results = seg_batch_results(stage, njobs);
    uint8_t* at = reinterpret_cast<uint8_t*>(results) + up256(16 * njobs);
    unsigned long long* const offs = reinterpret_cast<unsigned long long*>(at);
    at += up256(8 * (nseg + 1) * njobs);
    uint32_t* const lens = reinterpret_cast<uint32_t*>(at);
    at += up256(4 * nseg * njobs);
    uint32_t* const regions = reinterpret_cast<uint32_t*>(at);
    for (size_t j = 0; j < njobs; j++) {
        jobs[j].n = n; jobs[j].seg = seg; jobs[j].nseg = (uint32_t)nseg;
        jobs[j].offs = offs + j * (nseg + 1);
    }
    const size_t total = seg_batch_table_fill(host_table, jobs, njobs);
    (void)hipMemcpyAsync(stage, host_table, seg_batch_table_bytes(njobs), hipMemcpyHostToDevice, st);
    const SegJob* const d_jobs = reinterpret_cast<const SegJob*>(stage);
    const uint32_t* const d_first = reinterpret_cast<const uint32_t*>(stage + up256(njobs * sizeof(SegJob)));
    if (total)
        hipLaunchKernelGGL(k_seg_encode_batch, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, d_jobs, d_first, (uint32_t)njobs,
                           regions, stride_words, lens);
    hipLaunchKernelGGL(k_seg_scan_batch, dim3((unsigned)njobs), dim3(kScanThreads), 0, st, d_jobs, d_first, lens, results, result_host);
    if (total) {
        const unsigned grid = (unsigned)(total < 65536 ? total : 65536);
        hipLaunchKernelGGL(k_seg_gather_batch, dim3(grid), dim3(kGatherThreads), 0, st, d_jobs, d_first, (uint32_t)njobs, regions, stride_words, lens,
                           results);
    }
}

void seg_decode_batch(const SegJob* jobs, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    const size_t total = seg_batch_table_fill(host_table, jobs, njobs);
    if (!total) return;
    (void)hipMemcpyAsync(table, host_table, seg_batch_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_seg_decode_batch, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, reinterpret_cast<const SegJob*>(table),
                       reinterpret_cast<const uint32_t*>(table + up256(njobs * sizeof(SegJob))), (uint32_t)njobs);
}

size_t seg_lists_table_bytes(size_t njobs) { return seg_batch_table_bytes(njobs) + up256(njobs * sizeof(SegList)); }

size_t seg_decode_lists(const SegJob* jobs, const SegList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    // the table of seg_decode_batch with first[] over the list lengths, and the lists' records behind it
    const size_t at_first = up256(njobs * sizeof(SegJob)), at_lists = seg_batch_table_bytes(njobs);
    memset(host_table, 0, seg_lists_table_bytes(njobs));
    memcpy(host_table, jobs, njobs * sizeof(SegJob));
    memcpy(host_table + at_lists, lists, njobs * sizeof(SegList));
    uint32_t* const first = reinterpret_cast<uint32_t*>(host_table + at_first);
    size_t total = 0;
    for (size_t j = 0; j < njobs; j++) { first[j] = (uint32_t)total; total += lists[j].nlist; }
    first[njobs] = (uint32_t)total;
    if (!total) return 0;
    (void)hipMemcpyAsync(table, host_table, seg_lists_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_seg_decode_list_batch, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, reinterpret_cast<const SegJob*>(table),
                       reinterpret_cast<const SegList*>(table + at_lists), reinterpret_cast<const uint32_t*>(table + at_first), (uint32_t)njobs);
    return total;
}

// ---- stranded (WRS3) jobs behind the locator: the coder launch of a region decode over a batch of fields -------------------
namespace {

static_assert(kLanes == (int)wrsb::kWaveLanes, "the host's lane layout rounds a job to the coder kernels' workgroup");

// k_strand_decode<true> behind the locator.  first[] is the exclusive prefix of the jobs' lanes, job j's being nlist_j * K_j
// rounded up to a multiple of kLanes (wrsb::lists_lanes), so first[njobs] is a multiple of kLanes too: a workgroup -- one
// wave -- lies inside one job or past the end, K is uniform in it, and the K lanes of a segment sit aligned in it.  Lane
// first[j] + r is strand r & (K - 1) of list position i = r >> kshift and takes segment ids[i] if i < nlist; the other lanes of
// the job are padding.  Padding lanes and lanes past the end are not live, but nobody returns before the shuffles.
__global__ __launch_bounds__(kLanes) void k_strand_decode_list_batch(const SegJob* jobs, const StrandList* lists, const uint32_t* first, uint32_t njobs)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    bool live = g < first[njobs];
    uint32_t jb = 0, r = 0;
    if (live) wrsb::locate(first, njobs, (uint32_t)g, &jb, &r);
    const SegJob& job = jobs[jb];  // (a lane past the end looks at job 0 and decodes nothing)
    const StrandList& ls = lists[jb];
    const uint32_t K = ls.K, L = ls.L, j = r & (K - 1);
    const uint32_t i = r >> ls.kshift;
    live = live && i < ls.nlist;
    const size_t k = live ? ls.ids[i] : 0;
    const uint32_t seg = job.seg, nseg = job.nseg;
    live = live && k < nseg;  // (the K lanes of a segment agree; nobody returns before the shuffles)
    uint32_t why = 0;
    if (live) {
        LdsTable t{tab + lane};
        const size_t n = job.n;
        const uint8_t* const blob = job.blob;
        const size_t blob_len = job.cap;
        const size_t base = k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        // (the host has validated the index: the records lie inside the blob, in order, aligned, each no longer than one can be)
        const size_t front = wrseg::kHeaderBytesStrands + 4 * (size_t)nseg;
        const unsigned long long o0 = job.offs[k], o1 = job.offs[k + 1];
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
                SymSink sink{SegSpan(job.sym, base + s0, m), m, 0, 0};
                why = wrseg::decode_strand(d, t, sink, m, bs);
                sink.flush();
            }
        }
    }
    for (uint32_t off = 1; off < K; off <<= 1) why |= __shfl_xor(why, (int)off);
    if (live && j == 0) {
        job.flags[k] = why;
        if (why) atomicAdd(job.bad, 1u);
    }
}

}  // namespace

size_t strand_lists_table_bytes(size_t njobs) { return seg_batch_table_bytes(njobs) + up256(njobs * sizeof(StrandList)); }

size_t strand_decode_lists(const SegJob* jobs, const StrandList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    // the table of seg_decode_lists with first[] over the jobs' lanes (whole waves each), and the strand records behind it
    const size_t at_first = up256(njobs * sizeof(SegJob)), at_lists = seg_batch_table_bytes(njobs);
    memset(host_table, 0, strand_lists_table_bytes(njobs));
    memcpy(host_table, jobs, njobs * sizeof(SegJob));
    memcpy(host_table + at_lists, lists, njobs * sizeof(StrandList));
    uint32_t* const first = reinterpret_cast<uint32_t*>(host_table + at_first);
    size_t total = 0;
    for (size_t j = 0; j < njobs; j++) { first[j] = (uint32_t)total; total += (size_t)wrsb::job_lanes(lists[j].nlist, lists[j].K); }
    first[njobs] = (uint32_t)total;
    if (!total) return 0;
    (void)hipMemcpyAsync(table, host_table, strand_lists_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_strand_decode_list_batch, dim3((unsigned)(total / kLanes)), dim3(kLanes), 0, st, reinterpret_cast<const SegJob*>(table),
                       reinterpret_cast<const StrandList*>(table + at_lists), reinterpret_cast<const uint32_t*>(table + at_first), (uint32_t)njobs);
    return total;
}

}  // namespace wrk
