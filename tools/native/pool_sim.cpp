// pool_sim -- a closed-system model of the benchmark's host side on the coder pool, without a GPU: where session caps and
// hand-over rules are screened before GPU time is spent on them.  Per field kind (one per tolerance) L encoder threads and L
// decoder threads each keep one field in flight: all its planes go to the pool as one batch (pool_run), with their
// histograms and limits as the product's encoder passes them, and the next field follows when the batch is done.  What the
// model leaves out: the transform kernels, the plane windows (whole planes in host memory here) and the admission gate.
// Input (tools/pool_sim.py writes it): u32 kinds; per kind u32 planes, u64 n; per plane n symbols, u64 len, len stream bytes.
// usage: pool_sim FILE workers lanes seconds [decoder streams per scalar loop]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "wr_rangecoder.h"

namespace {
struct Plane {
    std::vector<uint8_t> sym, stream;
    std::vector<uint16_t> hist;
    size_t limit = 0;
};
struct Kind {
    size_t n = 0;
    std::vector<Plane> planes;
};
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
template <class T>
bool rd(FILE* f, T* v, size_t count = 1) { return fread(v, sizeof(T), count, f) == count; }
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: pool_sim FILE workers lanes seconds [decoder streams]\n"); return 2; }
    const int workers = atoi(argv[2]), lanes = atoi(argv[3]);
    const double seconds = atof(argv[4]);
    const int dec_streams = argc > 5 ? atoi(argv[5]) : 4;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t nkinds = 0;
    if (!rd(f, &nkinds) || nkinds < 1 || nkinds > 16) { fprintf(stderr, "pool_sim: not a plane file\n"); return 2; }
    std::vector<Kind> kinds(nkinds);
    for (Kind& k : kinds) {
        uint32_t np = 0;
        uint64_t n = 0;
        if (!rd(f, &np) || !rd(f, &n) || np < 1 || np > 64) { fprintf(stderr, "pool_sim: truncated plane file\n"); return 2; }
        k.n = (size_t)n;
        k.planes.resize(np);
        for (Plane& p : k.planes) {
            uint64_t len = 0;
            p.sym.resize(k.n);
            if (!rd(f, p.sym.data(), k.n) || !rd(f, &len)) { fprintf(stderr, "pool_sim: truncated plane file\n"); return 2; }
            p.stream.resize((size_t)len);
            if (!rd(f, p.stream.data(), (size_t)len)) { fprintf(stderr, "pool_sim: truncated plane file\n"); return 2; }
            p.hist.assign((k.n / wrrc::kBlock + 1) * 256, 0);
            for (size_t i = 0; i < k.n; i++) p.hist[(i / wrrc::kBlock) * 256 + p.sym[i]]++;
            p.limit = wrrc::encode_bound_hist(p.hist.data(), k.n);
        }
    }
    fclose(f);
    wrrc::pool_configure(workers, dec_streams);
    std::atomic<bool> stop{false}, bad{false};
    std::vector<std::atomic<unsigned long>> done(2 * nkinds);
    for (auto& d : done) d = 0;
    std::vector<std::thread> callers;
    for (uint32_t k = 0; k < nkinds; k++)
        for (int lane = 0; lane < lanes; lane++)
            for (int decode = 0; decode < 2; decode++)
                callers.emplace_back([&, k, decode] {
                    const Kind& kd = kinds[k];
                    const int np = (int)kd.planes.size();
                    std::vector<std::vector<uint8_t>> out((size_t)np);
                    for (int l = 0; l < np; l++) out[l].resize(decode ? kd.n : kd.planes[l].limit + wrrc::kFailedBlockSlack);
                    while (!stop.load()) {
                        std::vector<wrrc::PlaneJob> jobs((size_t)np);
                        for (int l = 0; l < np; l++) {
                            const Plane& p = kd.planes[l];
                            wrrc::PlaneJob& j = jobs[l];
                            j.n = kd.n; j.dst = out[l].data();
                            if (decode) { j.kind = wrrc::PlaneJob::kDecode; j.src = p.stream.data(); j.src_len = p.stream.size(); }
                            else { j.kind = wrrc::PlaneJob::kEncode; j.src = p.sym.data(); j.hist = p.hist.data(); j.dst_limit = p.limit; }
                        }
                        if (!wrrc::pool_run(jobs.data(), np)) { bad = true; return; }
                        for (int l = 0; l < np; l++) {
                            const Plane& p = kd.planes[l];
                            if (decode ? jobs[l].result != kd.n || memcmp(out[l].data(), p.sym.data(), kd.n)
                                       : jobs[l].result != p.stream.size() || memcmp(out[l].data(), p.stream.data(), p.stream.size()))
                                bad = true;
                        }
                        done[2 * k + decode]++;
                    }
                });
    // a warm-up second, then the timed region
    std::this_thread::sleep_for(std::chrono::milliseconds(1000));
    double s0[wrrc::kLoopKinds], b0[wrrc::kLoopKinds], s1[wrrc::kLoopKinds], b1[wrrc::kLoopKinds];
    std::vector<unsigned long> d0(2 * nkinds);
    for (size_t i = 0; i < d0.size(); i++) d0[i] = done[i].load();
    wrrc::pool_loop_stats(s0, b0);
    const double idle0 = wrrc::pool_idle_seconds(), t0 = now();
    std::this_thread::sleep_for(std::chrono::milliseconds((long)(seconds * 1000)));
    const double dt = now() - t0, idle = wrrc::pool_idle_seconds() - idle0;
    wrrc::pool_loop_stats(s1, b1);
    unsigned long enc = 0, dec = 0;
    for (uint32_t k = 0; k < nkinds; k++) { enc += done[2 * k].load() - d0[2 * k]; dec += done[2 * k + 1].load() - d0[2 * k + 1]; }
    stop = true;
    for (auto& t : callers) t.join();
    wrrc::pool_configure(0, 0);
    if (bad.load()) { printf("pool_sim: a stream or a plane DIFFERED\n"); return 1; }
    static const char* names[wrrc::kLoopKinds] = {"scalar_encoder", "scalar_decoder", "vector_decoder", "vector_encoder"};
    printf("{\"workers\": %d, \"lanes_per_kind\": %d, \"seconds\": %.2f, \"fields_encoded_per_s\": %.2f, \"fields_decoded_per_s\": %.2f, \"workers_idle\": %.2f, \"loops\": {",
           workers, lanes, dt, enc / dt, dec / dt, idle / dt);
    for (int i = 0; i < wrrc::kLoopKinds; i++) {
        const double s = s1[i] - s0[i], b = b1[i] - b0[i];
        printf("%s\"%s\": {\"workers\": %.2f, \"Msym_per_worker_s\": %.1f}", i ? ", " : "", names[i], s / dt, s > 0 ? b * wrrc::kBlock / s / 1e6 : 0.0);
    }
    printf("}}\n");
    return 0;
}
