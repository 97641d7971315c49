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
//   k_strand_decode_batch        the same for whole planes: the WRS3 jobs of a mixed batch decode, every (field, plane) in one launch
//   k_strand_encode_batch, k_strand_gather_batch   k_strand_encode and k_strand_gather behind the locator: plane l of a batch
//                        of fields as WRS3, K lanes per segment of any of them (the scan is k_seg_scan_batch's)
//
// The coder steps are wr_segcoder.h's; the lane's tools and the lane programs themselves are wr_segcoder_dev.h's, the ones
// wr_segcoder.hip's kernels call: every blob is byte for byte the single-plane kernels' blob.  A kernel here finds its job and
// segment with the locator, reads the job's plane and blob from the table (view_of) and stores what the body returns.
#include "wr_kernels.h"
#include "wr_segbatch.h"
#include "wr_segcoder.h"
#include "wr_segcoder_dev.h"

namespace wrk {

namespace {

// a job of the table as the lane bodies take it, beside job.sym (the decoders' blob length is the job's cap)
__device__ inline SegView view_of(const SegJob& job) { return SegView{job.n, job.seg, job.nseg, job.brick, job.blob, job.cap, job.offs}; }

__global__ __launch_bounds__(kLanes) void k_seg_encode_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, uint32_t* stage,
                                                             uint32_t stride_words, uint32_t* lens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    if (g >= first[njobs]) return;
    uint32_t j, k;
    wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
    lens[g] = encode_segment_lane(LdsTable{tab + lane}, jobs[j].sym, view_of(jobs[j]), k, stage + g * stride_words, stride_words);
}

// Block j: results[2j], results[2j + 1] (and results_host's, if there) = the result pair of job j's scan.  A stranded job
// (job.strands != 0: strand_encode_batch's) gets the WRS3 header; the tables are zero-filled, so every other job carries 0.
__global__ __launch_bounds__(kScanThreads) void k_seg_scan_batch(const SegJob* jobs, const uint32_t* first, const uint32_t* lens_all,
                                                                 unsigned long long* results, unsigned long long* results_host)
{
    __shared__ unsigned long long part[kScanThreads];
    __shared__ unsigned int bad;
    const uint32_t j = blockIdx.x;
    const SegJob& job = jobs[j];
    scan_lengths(part, &bad, threadIdx.x, lens_all + first[j], job.nseg, job.seg, job.brick, job.strands, job.offs, job.blob, job.cap, results + 2 * j,
                 results_host ? results_host + 2 * j : nullptr);
}

// Segment g of the launch is segment k of job j: blob_j[header + index + offs_j[k] ...) := the first lens[g] bytes of region g.
// Nothing of a job is written unless its whole blob fits under its cap and its every segment is good.
__global__ __launch_bounds__(kGatherThreads) void k_seg_gather_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, const uint32_t* stage,
                                                                     uint32_t stride_words, const uint32_t* lens, const unsigned long long* results)
{
    const size_t total = first[njobs];
    for (size_t g = blockIdx.x; g < total; g += gridDim.x) {
        uint32_t j, k;
        wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
        const SegJob& job = jobs[j];
        if (results[2 * j] > job.cap || results[2 * j + 1]) continue;
        const size_t front = wrseg::header_bytes(job.brick) + 4 * (size_t)job.nseg;
        copy_piece(job.blob + front + job.offs[k], stage + g * stride_words, lens[g], threadIdx.x);
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
    const uint32_t why = decode_segment_lane(LdsTable{tab + lane}, job.sym, view_of(job), k);
    job.flags[k] = why;
    if (why != wrseg::kSegOk) atomicAdd(job.bad, 1u);
}

// Lane g is position i of the list of job j: it decodes segment ids[i] of that job, as lane i of k_seg_decode<true> launched
// for the job alone would.
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
    if (k >= job.nseg) return;  // (the host made the list: every id is below nseg)
    const uint32_t why = decode_segment_lane(LdsTable{tab + lane}, job.sym, view_of(job), k);
    job.flags[k] = why;
    if (why != wrseg::kSegOk) atomicAdd(job.bad, 1u);
}

// host_table := the table of a launch: the jobs, first[0 .. njobs] = the exclusive prefix of lanes(j), and behind them the
// jobs' list records (list_bytes each; none: lists == nullptr).  Returns the lanes of the launch.
template <class Lanes>
size_t table_fill(uint8_t* host_table, const SegJob* jobs, size_t njobs, const void* lists, size_t list_bytes, Lanes lanes)
{
    memset(host_table, 0, seg_batch_table_bytes(njobs) + up256(njobs * list_bytes));
    memcpy(host_table, jobs, njobs * sizeof(SegJob));
    if (lists) memcpy(host_table + seg_batch_table_bytes(njobs), lists, njobs * list_bytes);
    uint32_t* const first = reinterpret_cast<uint32_t*>(host_table + up256(njobs * sizeof(SegJob)));
    size_t run = 0;
    for (size_t j = 0; j < njobs; j++) { first[j] = (uint32_t)run; run += lanes(j); }
    first[njobs] = (uint32_t)run;
    return run;
}

// where the parts of a table lie in device memory
const SegJob* table_jobs(const uint8_t* table) { return reinterpret_cast<const SegJob*>(table); }
const uint32_t* table_first(const uint8_t* table, size_t njobs) { return reinterpret_cast<const uint32_t*>(table + up256(njobs * sizeof(SegJob))); }
template <class List>
const List* table_lists(const uint8_t* table, size_t njobs) { return reinterpret_cast<const List*>(table + seg_batch_table_bytes(njobs)); }

}  // namespace

size_t seg_batch_table_bytes(size_t njobs) { return up256(njobs * sizeof(SegJob)) + up256(4 * (njobs + 1)); }

size_t seg_batch_table_fill(uint8_t* host_table, const SegJob* jobs, size_t njobs)
{
    return table_fill(host_table, jobs, njobs, nullptr, 0, [&](size_t j) { return (size_t)jobs[j].nseg; });
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
    const SegJob* const d_jobs = table_jobs(stage);
    const uint32_t* const d_first = table_first(stage, njobs);
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
    hipLaunchKernelGGL(k_seg_decode_batch, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, table_jobs(table),
                       table_first(table, njobs), (uint32_t)njobs);
}

size_t seg_lists_table_bytes(size_t njobs) { return seg_batch_table_bytes(njobs) + up256(njobs * sizeof(SegList)); }

size_t seg_decode_lists(const SegJob* jobs, const SegList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    // the table of seg_decode_batch with first[] over the list lengths, and the lists' records behind it
    const size_t total = table_fill(host_table, jobs, njobs, lists, sizeof(SegList), [&](size_t j) { return (size_t)lists[j].nlist; });
    if (!total) return 0;
    (void)hipMemcpyAsync(table, host_table, seg_lists_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_seg_decode_list_batch, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, table_jobs(table),
                       table_lists<SegList>(table, njobs), table_first(table, njobs), (uint32_t)njobs);
    return total;
}

// ---- stranded (WRS3) jobs behind the locator: the coder launch of a region decode over a batch of fields -------------------
namespace {

static_assert(kLanes == (int)wrsb::kWaveLanes, "the host's lane layout rounds a job to the coder kernels' workgroup");

// k_strand_decode<true> behind the locator.  first[] is the exclusive prefix of the jobs' lanes, job j's being nlist_j * K_j
// rounded up to a multiple of kLanes (wrsb::lists_lanes), so first[njobs] is a multiple of kLanes too: a workgroup -- one
// wave -- lies inside one job or past the end, K is uniform in it, and the K lanes of a segment sit aligned in it.  Lane
// first[j] + r is strand r & (K - 1) of list position i = r >> kshift and takes segment ids[i] if i < nlist; the other lanes of
// the job are padding.  Padding lanes and lanes past the end are not live; they go through the body all the same.
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
    const uint32_t K = ls.K, j = r & (K - 1);
    const uint32_t i = r >> ls.kshift;
    live = live && i < ls.nlist;
    const size_t k = live ? ls.ids[i] : 0;
    live = live && k < job.nseg;
    const uint32_t why = decode_strand_lane(LdsTable{tab + lane}, job.sym, view_of(job), K, ls.L, j, live, k);
    if (live && j == 0) {
        job.flags[k] = why;
        if (why) atomicAdd(job.bad, 1u);
    }
}

// The same for whole planes: no lists, K and L from the job (job.strands != 0 in every job of the table), first[] the prefix
// of wrsb::job_lanes(nseg_j, K_j).  Lane first[j] + r is strand r & (K - 1) of segment r >> log2(K); a segment id >= nseg is
// padding.  Everything but the ids look-up is the list kernel's.
__global__ __launch_bounds__(kLanes) void k_strand_decode_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x;
    const size_t g = (size_t)blockIdx.x * kLanes + lane;
    bool live = g < first[njobs];
    uint32_t jb = 0, r = 0;
    if (live) wrsb::locate(first, njobs, (uint32_t)g, &jb, &r);
    const SegJob& job = jobs[jb];  // (a lane past the end looks at job 0 and decodes nothing)
    const uint32_t K = job.strands, j = r & (K - 1);
    const size_t k = r >> wrsb::strands_shift(K);
    live = live && k < job.nseg;
    const uint32_t why = decode_strand_lane(LdsTable{tab + lane}, job.sym, view_of(job), K, wrseg::strand_len(job.seg, K), j, live, k);
    if (live && j == 0) {
        job.flags[k] = why;
        if (why) atomicAdd(job.bad, 1u);
    }
}

// k_strand_encode behind the locator.  All jobs share n, seg and K; first[] is the exclusive prefix of the jobs' segment
// counts, as k_seg_encode_batch's.  Lane g of the grid is strand g & (K - 1) of launch segment G = g >> kshift
// (wrsb::strand_lane); K divides kLanes, so the K lanes of a segment lie in one wave and one job, and a wave may hold groups of
// two jobs -- the body touches only its own lane's plane and its group's columns.  A lane with G >= first[njobs] is not live:
// it does not ask the locator, looks at job 0, and goes through the body to both barriers and the shuffles all the same.
__global__ __launch_bounds__(kLanes) void k_strand_encode_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, uint32_t K, uint32_t kshift,
                                                                uint32_t L, uint32_t* stage, uint32_t stride_words, uint32_t* lens, uint32_t* tlens,
                                                                uint32_t* slens)
{
    __shared__ uint32_t tab[256 * kLanes];
    const uint32_t lane = threadIdx.x, j = lane & (K - 1);
    const size_t G = ((size_t)blockIdx.x * kLanes + lane) >> kshift;
    const bool live = G < first[njobs];
    uint32_t jb = 0, k = 0;
    if (live) wrsb::locate(first, njobs, (uint32_t)G, &jb, &k);
    const SegJob& job = jobs[jb];
    encode_strand_lane(tab, lane, job.sym, view_of(job), K, L, live, k, stage + G * stride_words, slens + G * K + j, tlens + G, lens + G);
}

// Segment g of the launch is segment k of job j: record k of blob_j := region g, as k_strand_gather writes it.  Nothing of a job
// is written unless its whole blob fits under its cap and its every record is good.
__global__ __launch_bounds__(kGatherThreads) void k_strand_gather_batch(const SegJob* jobs, const uint32_t* first, uint32_t njobs, const uint32_t* stage,
                                                                        uint32_t stride_words, const uint32_t* lens, const uint32_t* tlens,
                                                                        const uint32_t* slens, uint32_t K, uint32_t sb_words, const unsigned long long* results)
{
    const size_t total = first[njobs];
    for (size_t g = blockIdx.x; g < total; g += gridDim.x) {
        uint32_t j, k;
        wrsb::locate(first, njobs, (uint32_t)g, &j, &k);
        const SegJob& job = jobs[j];
        if (results[2 * j] > job.cap || results[2 * j + 1]) continue;
        const size_t front = wrseg::kHeaderBytesStrands + 4 * (size_t)job.nseg;
        gather_record(job.blob + front + job.offs[k], stage + g * stride_words, tlens[g], slens + g * K, K, sb_words, lens[g], threadIdx.x);
    }
}

// the staging of a stranded encode launch behind the table and the result pairs: offs, lens, tlens, slens, the regions
struct StrandStage {
    size_t nseg, at_offs, at_lens, at_regions, bytes;
    uint32_t sb_words, stride_words;
    StrandStage(size_t njobs, size_t n, unsigned seg, unsigned strands) : nseg(wrseg::seg_count(n, seg))
    {
        sb_words = wrseg::strand_bound(wrseg::strand_len(seg, strands)) / 4;
        stride_words = wrseg::kModelBound / 4 + strands * sb_words;
        at_offs = seg_batch_table_bytes(njobs) + up256(16 * njobs);
        at_lens = at_offs + up256(8 * (nseg + 1) * njobs);
        at_regions = at_lens + up256(4 * nseg * njobs * (2 + (size_t)strands));
        bytes = at_regions + njobs * nseg * 4 * (size_t)stride_words;
    }
};

}  // namespace

size_t strand_lists_table_bytes(size_t njobs) { return seg_batch_table_bytes(njobs) + up256(njobs * sizeof(StrandList)); }

size_t strand_decode_lists(const SegJob* jobs, const StrandList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    // the table of seg_decode_lists with first[] over the jobs' lanes (whole waves each), and the strand records behind it
    const size_t total = table_fill(host_table, jobs, njobs, lists, sizeof(StrandList),
                                    [&](size_t j) { return (size_t)wrsb::job_lanes(lists[j].nlist, lists[j].K); });
    if (!total) return 0;
    (void)hipMemcpyAsync(table, host_table, strand_lists_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_strand_decode_list_batch, dim3((unsigned)(total / kLanes)), dim3(kLanes), 0, st, table_jobs(table),
                       table_lists<StrandList>(table, njobs), table_first(table, njobs), (uint32_t)njobs);
    return total;
}

size_t strand_batch_stage_bytes(size_t njobs, size_t n, unsigned seg, unsigned strands) { return StrandStage(njobs, n, seg, strands).bytes; }

void strand_encode_batch(SegJob* jobs, size_t njobs, size_t n, unsigned seg, unsigned strands, uint8_t* host_table, uint8_t* stage,
                         unsigned long long* result_host, hipStream_t st)
{
    const StrandStage sg(njobs, n, seg, strands);
    const size_t nseg = sg.nseg;
    unsigned long long* const results = seg_batch_results(stage, njobs);
    unsigned long long* const offs = reinterpret_cast<unsigned long long*>(stage + sg.at_offs);
    uint32_t* const lens = reinterpret_cast<uint32_t*>(stage + sg.at_lens);
    uint32_t* const tlens = lens + nseg * njobs;
    uint32_t* const slens = tlens + nseg * njobs;
    uint32_t* const regions = reinterpret_cast<uint32_t*>(stage + sg.at_regions);
    for (size_t j = 0; j < njobs; j++) {
        jobs[j].n = n; jobs[j].seg = seg; jobs[j].nseg = (uint32_t)nseg; jobs[j].strands = strands;
        jobs[j].offs = offs + j * (nseg + 1);
    }
    const size_t total = seg_batch_table_fill(host_table, jobs, njobs);
    (void)hipMemcpyAsync(stage, host_table, seg_batch_table_bytes(njobs), hipMemcpyHostToDevice, st);
    const SegJob* const d_jobs = table_jobs(stage);
    const uint32_t* const d_first = table_first(stage, njobs);
    if (total)
        hipLaunchKernelGGL(k_strand_encode_batch, dim3((unsigned)((total * strands + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, d_jobs, d_first,
                           (uint32_t)njobs, (uint32_t)strands, wrsb::strands_shift(strands), wrseg::strand_len(seg, strands), regions, sg.stride_words, lens,
                           tlens, slens);
    hipLaunchKernelGGL(k_seg_scan_batch, dim3((unsigned)njobs), dim3(kScanThreads), 0, st, d_jobs, d_first, lens, results, result_host);
    if (total) {
        const unsigned grid = (unsigned)(total < 65536 ? total : 65536);
        hipLaunchKernelGGL(k_strand_gather_batch, dim3(grid), dim3(kGatherThreads), 0, st, d_jobs, d_first, (uint32_t)njobs, regions, sg.stride_words, lens,
                           tlens, slens, (uint32_t)strands, sg.sb_words, results);
    }
}

size_t strand_decode_batch(const SegJob* jobs, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    // the table of seg_decode_batch with first[] over the jobs' lanes (whole waves each)
    const size_t total = table_fill(host_table, jobs, njobs, nullptr, 0, [&](size_t j) { return (size_t)wrsb::job_lanes(jobs[j].nseg, jobs[j].strands); });
    if (!total) return 0;
    (void)hipMemcpyAsync(table, host_table, seg_batch_table_bytes(njobs), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_strand_decode_batch, dim3((unsigned)(total / kLanes)), dim3(kLanes), 0, st, table_jobs(table), table_first(table, njobs),
                       (uint32_t)njobs);
    return total;
}

}  // namespace wrk
