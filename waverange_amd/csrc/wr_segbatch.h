// wr_segbatch.h -- which job a lane of a batched segment-coder launch belongs to (wr_segbatch.hip).
//
// A batched launch codes the planes of several fields at once: job j is one (field, plane) with nseg_j segments, and
// first[0 .. njobs] is the exclusive prefix of the nseg_j (first[0] = 0, first[njobs] = the segments of the launch).  Lane g of
// the grid owns segment g - first[j] of the job j with first[j] <= g < first[j + 1].  Jobs without segments own no lane.
// Compiles for the host and the device; the host form is what the tests and the sanitizer harness sweep.
#ifndef WR_SEGBATCH_H
#define WR_SEGBATCH_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WRSB_HD __host__ __device__ inline
#else
#define WRSB_HD inline
#endif

namespace wrsb {

constexpr uint32_t kBatchMax = 1024;  // WR_SEG_BATCH_MAX: fields of a batch, so jobs of a launch (the search is 10 steps at most)

// g < first[njobs], njobs >= 1 (the callers' business: a lane past the end has returned before it asks).  Keeps
// first[lo] <= g < first[hi]; only first[1 .. njobs - 1] are read.
WRSB_HD void locate(const uint32_t* first, uint32_t njobs, uint32_t g, uint32_t* job, uint32_t* k)
{
    uint32_t lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    *job = lo;
    *k = g - first[lo];
}

// a prefix as locate() wants it: starts at 0, never decreases
inline bool prefix_ok(const uint32_t* first, uint32_t njobs)
{
    if (!first || njobs < 1 || first[0] != 0) return false;
    for (uint32_t j = 0; j < njobs; j++) if (first[j + 1] < first[j]) return false;
    return true;
}

// ---- the lanes of a launch over LISTS of segments, stranded jobs included (k_seg_decode_list_batch, k_strand_decode_list_batch).
// Job j decodes nlist[j] segments with strands[j] lanes each:
//   strands[j] == 0      a WRS1 / WRS2 job: one lane per listed segment, no padding; lane first[j] + i takes list position i
//   strands[j] == K > 0  a WRS3 job: nlist[j] * K lanes ROUNDED UP to a multiple of kWaveLanes.  Lane first[j] + r is strand
//                        r & (K - 1) of list position r >> log2(K); a position >= nlist[j] is padding and decodes nothing.
// So a stranded job starts and ends on a wave's edge whatever its neighbours are: no workgroup spans two such jobs, and the K
// lanes of a segment (K divides kWaveLanes) sit aligned inside one wave, as the kernel's __shfl_xor reduction needs.
// first[0 .. njobs] (may be null) is the exclusive prefix of those lane counts, as locate() wants it.
// Like locate(), all of it compiles for the host and the device.
constexpr uint32_t kWaveLanes = 64;            // = kLanes of the coder kernels: a workgroup is one wave
constexpr unsigned long long kLaneLimit = 1ull << 31;

WRSB_HD bool strands_layout_ok(unsigned k) { return k == 0 || (k <= 32 && (k & (k - 1)) == 0); }

WRSB_HD uint32_t strands_shift(unsigned k)  // k: a power of two
{
    uint32_t s = 0;
    while ((1u << s) < k) s++;
    return s;
}

// the lanes job j owns
WRSB_HD unsigned long long job_lanes(unsigned long long nlist, unsigned strands)
{
    if (!strands) return nlist;
    return (nlist * strands + kWaveLanes - 1) / kWaveLanes * kWaveLanes;
}

// Returns the lanes of the launch; 0: refused (njobs outside 1..kBatchMax, a null list, a strand count that is not 0 or a power
// of two up to 32, 2^31 lanes or more -- first[] is then not written) or every list is empty (first[] is all zeros).
// strands == nullptr: every job is a WRS1 / WRS2 job.
WRSB_HD unsigned long long lists_lanes(long long njobs, const size_t* nlist, const unsigned* strands, uint32_t* first)
{
    if (njobs < 1 || njobs > (long long)kBatchMax || !nlist) return 0;
    unsigned long long run = 0;
    for (long long j = 0; j < njobs; j++) {
        const unsigned k = strands ? strands[j] : 0;
        if (!strands_layout_ok(k) || nlist[j] >= kLaneLimit) return 0;
        run += job_lanes(nlist[j], k);
        if (run >= kLaneLimit) return 0;
    }
    if (first) {
        run = 0;
        for (long long j = 0; j < njobs; j++) { first[j] = (uint32_t)run; run += job_lanes(nlist[j], strands ? strands[j] : 0); }
        first[njobs] = (uint32_t)run;
    }
    return run;
}

// ---- the lanes of a STRANDED ENCODE launch (k_strand_encode_batch): all jobs share K, first[0 .. njobs] is the exclusive
// prefix of the jobs' SEGMENT counts as above, and lane g of the grid is strand g & (K - 1) of launch segment G = g >> log2(K),
// which locate() resolves to (job, segment).  No padding between jobs: K divides kWaveLanes, so the K lanes of a segment stay
// inside one wave and one job, while a wave may hold groups of several jobs.  The grid is rounded up to whole waves; a lane
// with G >= first[njobs] is past the end (false, nothing written), and locate() is not asked about it.
WRSB_HD bool strand_lane(const uint32_t* first, uint32_t njobs, unsigned strands, unsigned long long g, uint32_t* job, uint32_t* segment, uint32_t* strand)
{
    const unsigned long long G = g >> strands_shift(strands);
    if (G >= first[njobs]) return false;
    locate(first, njobs, (uint32_t)G, job, segment);
    *strand = (uint32_t)(g & (strands - 1));
    return true;
}

}  // namespace wrsb

#endif
