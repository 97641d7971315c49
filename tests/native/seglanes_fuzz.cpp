// The lane layout of a coder launch over lists, stranded jobs included (csrc/wr_segbatch.h: lists_lanes, job_lanes, locate)
// under ASan + UBSan: the header the kernels include, compiled for the host.  For every layout first[] is an exact-size heap
// block, every lane of the launch is located and compared with a linear walk, and what the kernel derives from a lane -- list
// position, strand, live or padding -- is checked against the definition.
// Built and run by tests/test_roi_batch_cpu.py (g++ -fsanitize=address,undefined); prints one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "wr_segbatch.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int failures = 0;
static unsigned long long lanes_seen = 0;

static void fail(const char* what, const char* why, unsigned long long a = 0, unsigned long long b = 0)
{
    if (failures < 10) printf("FAIL %s: %s (%llu, %llu)\n", what, why, a, b);
    failures++;
}

static void sweep(const std::vector<size_t>& nlist, const std::vector<unsigned>& strands, const char* what)
{
    const uint32_t njobs = (uint32_t)nlist.size();
    uint32_t* const first = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)njobs + 1));  // exact size
    const unsigned long long total = wrsb::lists_lanes(njobs, nlist.data(), strands.data(), first);
    if (wrsb::lists_lanes(njobs, nlist.data(), strands.data(), nullptr) != total) fail(what, "the count depends on first[]");
    unsigned long long any = 0;
    for (size_t v : nlist) any += v;
    if (!total && any) { fail(what, "a good layout is refused"); free(first); return; }
    if (!wrsb::prefix_ok(first, njobs) || first[njobs] != total) fail(what, "first[] is no prefix of the lanes", first[njobs], total);
    bool stranded_only = true;
    for (uint32_t j = 0; j < njobs; j++) {
        const unsigned K = strands[j];
        const unsigned long long span = first[j + 1] - first[j];
        if (!K) { if (span != nlist[j]) fail(what, "a plain job is padded", j, span); if (nlist[j]) stranded_only = false; continue; }
        if (span % wrsb::kWaveLanes || span < (unsigned long long)nlist[j] * K || span >= (unsigned long long)nlist[j] * K + wrsb::kWaveLanes)
            fail(what, "a stranded job's span is not its lanes rounded up to a wave", j, span);
    }
    if (stranded_only && total % wrsb::kWaveLanes) fail(what, "a launch of stranded jobs is no whole number of waves", total);
    uint32_t want_job = 0;
    std::vector<unsigned long long> live(njobs, 0);
    for (unsigned long long g = 0; g < total; g++) {
        while (g >= first[want_job + 1]) want_job++;
        uint32_t job = 0xffffffffu, r = 0xffffffffu;
        wrsb::locate(first, njobs, (uint32_t)g, &job, &r);
        if (job != want_job || r != g - first[want_job]) { fail(what, "lane located wrongly", g, job); continue; }
        const unsigned K = strands[job];
        const uint32_t i = K ? r >> wrsb::strands_shift(K) : r, strand = K ? r & (K - 1) : 0;
        if (K && (uint64_t)i * K + strand != r) fail(what, "position and strand do not give the lane back", g, r);
        if (i < nlist[job]) live[job]++;
        if (K && stranded_only) {
            // the K lanes of a segment sit aligned inside one wave
            const unsigned long long base = g - strand;
            if (base % K || base / wrsb::kWaveLanes != (base + K - 1) / wrsb::kWaveLanes) fail(what, "a segment's lanes straddle a wave", g, K);
        }
        lanes_seen++;
    }
    for (uint32_t j = 0; j < njobs; j++)
        if (live[j] != (unsigned long long)nlist[j] * (strands[j] ? strands[j] : 1)) fail(what, "a job's live lanes are not its list times K", j, live[j]);
    free(first);
}

int main()
{
    const unsigned ks[7] = {0, 1, 2, 4, 8, 16, 32};
    const size_t ls[5] = {0, 1, 63, 64, 65};
    for (unsigned k : ks) for (size_t l : ls) sweep({l}, {k}, "one job");
    for (unsigned a : ks) for (unsigned b : ks) for (size_t l : ls) for (size_t m : ls) sweep({l, m}, {a, b}, "two jobs");
    {
        std::vector<size_t> nl(wrsb::kBatchMax);
        std::vector<unsigned> st(wrsb::kBatchMax);
        for (uint32_t j = 0; j < wrsb::kBatchMax; j++) { nl[j] = ls[j % 5]; st[j] = ks[(j / 5) % 7]; }
        sweep(nl, st, "1024 jobs");
    }
    for (int round = 0; round < 300; round++) {
        const uint32_t njobs = 1 + rnd() % (round < 250 ? 24 : wrsb::kBatchMax);
        std::vector<size_t> nl(njobs);
        std::vector<unsigned> st(njobs);
        const bool stranded = rnd() & 1;  // half of the launches are a stranded kernel's: no plain job among them
        for (uint32_t j = 0; j < njobs; j++) { nl[j] = rnd() % 4 ? rnd() % 150 : 0; st[j] = stranded ? ks[1 + rnd() % 6] : ks[rnd() % 7]; }
        sweep(nl, st, "random");
    }
    // refusals: first[] is not written
    {
        uint32_t first[3] = {7, 7, 7};
        const size_t one[2] = {1, 1}, big[2] = {(size_t)1 << 30, (size_t)1 << 30}, wide[1] = {(size_t)1 << 26};
        const unsigned bad[2] = {0, 3}, k32[1] = {32}, k16[1] = {16};
        std::vector<size_t> many(wrsb::kBatchMax + 1, 1);
        if (wrsb::lists_lanes(0, one, nullptr, first) || wrsb::lists_lanes(-1, one, nullptr, first) || wrsb::lists_lanes(2, nullptr, nullptr, first) ||
            wrsb::lists_lanes(wrsb::kBatchMax + 1, many.data(), nullptr, nullptr) || wrsb::lists_lanes(2, one, bad, first) ||
            wrsb::lists_lanes(2, big, nullptr, first) || wrsb::lists_lanes(1, wide, k32, first))
            fail("refusals", "a bad layout is accepted");
        if (first[0] != 7 || first[1] != 7 || first[2] != 7) fail("refusals", "first[] is written for a refused layout");
        if (wrsb::lists_lanes(1, wide, k16, nullptr) != (1ull << 30)) fail("refusals", "2^30 lanes are refused");
        if (wrsb::lists_lanes(2, one, nullptr, first) != 2 || first[2] != 2) fail("refusals", "null strands are not plain jobs");
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("segment list lane layout sanitizer run OK (%llu lanes)\n", lanes_seen);
    return 0;
}
