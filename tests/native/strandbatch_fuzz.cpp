// The two lane layouts of the batched strand coder (csrc/wr_segbatch.h) under ASan + UBSan: the header the kernels include,
// compiled for the host.
//   the encoder (strand_lane)   all jobs share K; first[] is the prefix of the jobs' SEGMENT counts; lane g of the grid is strand
//                               g & (K - 1) of launch segment g >> log2(K); the grid is rounded up to whole waves
//   the decoder (lists_lanes with nlist[j] = nseg_j, then locate)   job j owns nseg_j * K_j lanes rounded up to whole waves
// For every job table first[] is an exact-size heap block, every lane of the grid is resolved and compared with a linear walk:
// every (job, segment, strand) is owned by exactly one lane, the K lanes of a segment sit aligned in one wave and one job, lanes
// past the end (encoder) and padding lanes (decoder) own nothing, and a workgroup of the decoder lies inside one job.
// Built and run by tests/test_strand_batch_cpu.py (g++ -fsanitize=address,undefined); prints one OK line.
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
static unsigned long long lanes_seen = 0;

static void fail(const char* what, const char* why, unsigned long long a = 0, unsigned long long b = 0)
{
    if (failures < 10) printf("FAIL %s: %s (%llu, %llu)\n", what, why, a, b);
    failures++;
}

static void sweep_encoder(const std::vector<uint32_t>& nsegs, unsigned K, const char* what)
{
    const uint32_t njobs = (uint32_t)nsegs.size();
    uint32_t* const first = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)njobs + 1));  // exact size
    uint32_t run = 0;
    for (uint32_t j = 0; j < njobs; j++) { first[j] = run; run += nsegs[j]; }
    first[njobs] = run;
    if (!wrsb::prefix_ok(first, njobs)) fail(what, "the table is no prefix");
    const unsigned long long lanes = (unsigned long long)run * K, grid = (lanes + wrsb::kWaveLanes - 1) / wrsb::kWaveLanes * wrsb::kWaveLanes;
    uint32_t want_job = 0, want_seg = 0, want_strand = 0;
    for (unsigned long long g = 0; g < grid + wrsb::kWaveLanes; g++) {  // (a wave past the grid as well: nobody owns anything there)
        uint32_t job = 0xffffffffu, seg = 0xffffffffu, strand = 0xffffffffu;
        const bool live = wrsb::strand_lane(first, njobs, K, g, &job, &seg, &strand);
        if (live != (g < lanes)) { fail(what, "a lane is live on the wrong side of the end", g, lanes); continue; }
        if (!live) {
            if (job != 0xffffffffu || seg != 0xffffffffu || strand != 0xffffffffu) fail(what, "a lane past the end writes its results", g);
            continue;
        }
        while (want_seg >= nsegs[want_job]) { want_job++; want_seg = 0; }
        if (job != want_job || seg != want_seg || strand != want_strand) fail(what, "lane resolved wrongly", g, job);
        // the K lanes of a segment: aligned, in one wave
        const unsigned long long base = g - strand;
        if (base % K || base / wrsb::kWaveLanes != (base + K - 1) / wrsb::kWaveLanes) fail(what, "a segment's lanes straddle a wave", g, K);
        if (++want_strand == K) { want_strand = 0; want_seg++; }
        lanes_seen++;
    }
    while (want_job < njobs && want_seg >= nsegs[want_job]) { want_job++; want_seg = 0; }
    if (want_job != njobs || want_strand) fail(what, "not every strand of every segment has a lane", want_job, want_seg);
    free(first);
}

static void sweep_decoder(const std::vector<uint32_t>& nsegs, const std::vector<unsigned>& Ks, const char* what)
{
    const uint32_t njobs = (uint32_t)nsegs.size();
    std::vector<size_t> nlist(nsegs.begin(), nsegs.end());
    uint32_t* const first = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)njobs + 1));  // exact size
    const unsigned long long total = wrsb::lists_lanes(njobs, nlist.data(), Ks.data(), first);
    unsigned long long any = 0;
    for (uint32_t v : nsegs) any += v;
    if (!total) { if (any) fail(what, "a good layout is refused"); free(first); return; }
    if (total % wrsb::kWaveLanes) fail(what, "the launch is no whole number of waves", total);
    for (uint32_t j = 0; j < njobs; j++)
        if (first[j + 1] - first[j] != wrsb::job_lanes(nsegs[j], Ks[j])) fail(what, "a job's span is not job_lanes", j);
    std::vector<unsigned long long> live(njobs, 0);
    for (unsigned long long w = 0; w < total; w += wrsb::kWaveLanes) {
        uint32_t wave_job = 0xffffffffu;
        for (unsigned long long g = w; g < w + wrsb::kWaveLanes; g++) {
            uint32_t job = 0, r = 0;
            wrsb::locate(first, njobs, (uint32_t)g, &job, &r);
            if (g < first[job] || g >= first[job + 1] || r != g - first[job]) { fail(what, "lane located wrongly", g, job); continue; }
            if (wave_job == 0xffffffffu) wave_job = job;
            if (job != wave_job) fail(what, "a workgroup spans two jobs", g, job);
            const unsigned K = Ks[job];
            const uint32_t k = r >> wrsb::strands_shift(K), strand = r & (K - 1);
            if ((uint64_t)k * K + strand != r) fail(what, "segment and strand do not give the lane back", g, r);
            if (k < nsegs[job]) live[job]++;
            lanes_seen++;
        }
    }
    for (uint32_t j = 0; j < njobs; j++)
        if (live[j] != (unsigned long long)nsegs[j] * Ks[j]) fail(what, "a job's live lanes are not its segments times K", j, live[j]);
    free(first);
}

int main()
{
    const unsigned ks[6] = {1, 2, 4, 8, 16, 32};
    const uint32_t ns[7] = {0, 1, 2, 17, 63, 64, 65};
    for (unsigned k : ks) for (uint32_t a : ns) { sweep_encoder({a}, k, "one job"); sweep_decoder({a}, {k}, "one job"); }
    for (unsigned k : ks) for (uint32_t a : ns) for (uint32_t b : ns) for (uint32_t c : ns) sweep_encoder({a, b, c}, k, "three jobs");
    for (unsigned k : ks) for (unsigned m : ks) for (uint32_t a : ns) for (uint32_t b : ns) sweep_decoder({a, b}, {k, m}, "two jobs");
    // the case table of tests/strand_batch_cases.py
    const struct { uint32_t nseg; unsigned K; uint32_t jobs; } table[7] = {{1, 8, 17}, {17, 32, 3}, {1100, 1, 3}, {367, 2, 5}, {4, 16, 9}, {5, 8, 13}, {2, 4, 1}};
    for (const auto& t : table) {
        sweep_encoder(std::vector<uint32_t>(t.jobs, t.nseg), t.K, "case table");
        sweep_decoder(std::vector<uint32_t>(t.jobs, t.nseg), std::vector<unsigned>(t.jobs, t.K), "case table");
    }
    for (int round = 0; round < 300; round++) {
        const uint32_t njobs = 1 + rnd() % (round < 250 ? 24 : wrsb::kBatchMax);
        std::vector<uint32_t> nsegs(njobs);
        std::vector<unsigned> Ks(njobs);
        for (uint32_t j = 0; j < njobs; j++) { nsegs[j] = rnd() % 4 ? rnd() % 150 : 0; Ks[j] = ks[rnd() % 6]; }
        sweep_encoder(nsegs, ks[rnd() % 6], "random");
        sweep_decoder(nsegs, Ks, "random");
    }
    {
        std::vector<uint32_t> nsegs(wrsb::kBatchMax);
        std::vector<unsigned> Ks(wrsb::kBatchMax);
        for (uint32_t j = 0; j < wrsb::kBatchMax; j++) { nsegs[j] = ns[j % 7]; Ks[j] = ks[(j / 7) % 6]; }
        sweep_encoder(nsegs, 8, "1024 jobs");
        sweep_decoder(nsegs, Ks, "1024 jobs");
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("strand batch lane layout sanitizer run OK (%llu lanes)\n", lanes_seen);
    return 0;
}
