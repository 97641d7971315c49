// The locator of the batched segment-coder kernels (csrc/wr_segbatch.h) under ASan + UBSan: the header the kernels include,
// compiled for the host.  Every lane of every prefix is located and compared with a linear walk; the prefix arrays are
// exact-size heap blocks, so a read before first[0] or past first[njobs] is an error of the run.
// Built and run by tests/test_seg_batch_cpu.py (g++ -fsanitize=address,undefined); prints one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "wr_segbatch.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int failures = 0;
static unsigned long long lanes = 0;

static void sweep(const std::vector<uint32_t>& counts, const char* what)
{
    const uint32_t njobs = (uint32_t)counts.size();
    // exact size: njobs + 1 words, nothing before, nothing behind
    uint32_t* const first = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)njobs + 1));
    uint32_t run = 0;
    for (uint32_t j = 0; j < njobs; j++) { first[j] = run; run += counts[j]; }
    first[njobs] = run;
    if (!wrsb::prefix_ok(first, njobs)) { printf("FAIL %s: prefix_ok refuses a prefix\n", what); failures++; }
    uint32_t want_job = 0;
    for (uint32_t g = 0; g < run; g++) {
        while (g >= first[want_job + 1]) want_job++;  // the linear walk: jobs without segments are stepped over
        uint32_t job = 0xffffffffu, k = 0xffffffffu;
        wrsb::locate(first, njobs, g, &job, &k);
        if (job != want_job || k != g - first[want_job] || k >= counts[job]) {
            if (failures < 10) printf("FAIL %s: lane %u -> (%u, %u), want (%u, %u)\n", what, g, job, k, want_job, g - first[want_job]);
            failures++;
        }
        lanes++;
    }
    free(first);
}

int main()
{
    sweep(std::vector<uint32_t>(70, 1), "70 jobs of 1");
    sweep(std::vector<uint32_t>(9, 17), "9 jobs of 17");
    sweep(std::vector<uint32_t>(3, 1100), "3 jobs of 1100");
    sweep(std::vector<uint32_t>(13, 5), "13 jobs of 5");
    sweep({0, 0, 3, 0, 1, 0, 0, 64, 65, 0, 2, 0, 0}, "zero-segment jobs in the middle and at both ends");
    sweep({7}, "one job");
    sweep({0, 5}, "an empty job first");
    sweep({5, 0}, "an empty job last");
    sweep(std::vector<uint32_t>(wrsb::kBatchMax, 1), "1024 jobs of 1");
    sweep(std::vector<uint32_t>(wrsb::kBatchMax, 36), "1024 jobs of 36");
    for (int round = 0; round < 400; round++) {
        const uint32_t njobs = 1 + rnd() % (round < 300 ? 40 : wrsb::kBatchMax);
        std::vector<uint32_t> counts(njobs);
        const uint32_t top = 1 + rnd() % 200, zeros = rnd() % 4;  // zeros: every job is empty with probability zeros / 4
        for (uint32_t j = 0; j < njobs; j++) counts[j] = (rnd() % 4 < zeros) ? 0 : rnd() % top;
        sweep(counts, "random");
    }
    // a prefix close to the 2^31 lanes a launch may have: three lanes at its joints, not all of them
    {
        const uint32_t first[4] = {0, 0x3fffffffu, 0x3fffffffu, 0x7fffffffu};
        const uint32_t at[6] = {0, 0x3ffffffeu, 0x3fffffffu, 0x40000000u, 0x7ffffffeu, 1};
        const uint32_t want[6] = {0, 0, 2, 2, 2, 0};
        for (int i = 0; i < 6; i++) {
            uint32_t job, k;
            wrsb::locate(first, 3, at[i], &job, &k);
            if (job != want[i] || k != at[i] - first[job]) { printf("FAIL large prefix: lane %u -> (%u, %u)\n", at[i], job, k); failures++; }
        }
    }
    // what prefix_ok refuses
    {
        const uint32_t a[3] = {1, 2, 3}, b[3] = {0, 5, 4};
        if (wrsb::prefix_ok(a, 2) || wrsb::prefix_ok(b, 2) || wrsb::prefix_ok(nullptr, 2) || wrsb::prefix_ok(b, 0)) { printf("FAIL prefix_ok accepts a bad prefix\n"); failures++; }
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("segment batch locator sanitizer run OK (%llu lanes)\n", lanes);
    return 0;
}
