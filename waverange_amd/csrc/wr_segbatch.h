// wr_segbatch.h -- which job a lane of a batched segment-coder launch belongs to (wr_segbatch.hip).
//
// A batched launch codes the planes of several fields at once: job j is one (field, plane) with nseg_j segments, and
// first[0 .. njobs] is the exclusive prefix of the nseg_j (first[0] = 0, first[njobs] = the segments of the launch).  Lane g of
// the grid owns segment g - first[j] of the job j with first[j] <= g < first[j + 1].  Jobs without segments own no lane.
// Compiles for the host and the device; the host form is what the tests and the sanitizer harness sweep.
#ifndef WR_SEGBATCH_H
#define WR_SEGBATCH_H

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

}  // namespace wrsb

#endif
