// ASan/UBSan harness for the size bound of an encode to a byte budget (csrc/wr_budget.h), compiled by g++: random and
// adversarial histograms go through the bound and through the host segment encoder (csrc/wr_segcoder.h), and the bound must
// hold; the table look-ups must stay inside the table for every segment length a stream can have.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "wr_budget.h"
#include "wr_segcoder.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }

static int check(const std::vector<uint8_t>& p, const char* what)
{
    const uint32_t bs = (uint32_t)p.size();
    uint32_t counts[256] = {0};
    for (uint8_t v : p) counts[v]++;
    const uint32_t bound = wrbud::segment_bound(wrbud::tables(), counts, bs);
    std::vector<uint8_t> out(wrseg::stream_bound(bs));
    const uint32_t len = wrseg::encode_segment_host(p.data(), bs, out.data(), (uint32_t)out.size());
    if (!len) { printf("%s bs=%u: the encoder refused the segment\n", what, bs); return 1; }
    if (bound < len) { printf("%s bs=%u: bound %u below the stream's %u bytes\n", what, bs, bound, len); return 1; }
    if (bound > wrseg::stream_bound(bs)) { printf("%s bs=%u: bound %u above the plain bound\n", what, bs, bound); return 1; }
    return 0;
}

int main()
{
    const wrbud::Tables& t = wrbud::tables();
    // the table: exact-size allocation (an index outside is ASan's), monotone, up above down, every segment length in range
    if (t.words.size() != wrbud::kTabWords) { printf("table size\n"); return 1; }
    std::vector<uint32_t> copy(t.words);  // (exactly kTabWords words on the heap)
    for (uint32_t bs = 1; bs <= wrseg::kSegMax; bs++) {
        const uint32_t up = copy[wrbud::kTabN + bs], down = copy[bs];
        if (up < down) { printf("up[%u] < down[%u]\n", bs, bs); return 1; }
        if (bs > 1 && (down < copy[bs - 1] || up < copy[wrbud::kTabN + bs - 1])) { printf("table not monotone at %u\n", bs); return 1; }
        uint32_t counts[256] = {0};
        counts[bs & 255] = bs;  // a one-symbol segment: the largest look-up there is
        const uint32_t b = wrbud::segment_bound(t, counts, bs);
        if (b < 5 + 512 || b > wrseg::stream_bound(bs)) { printf("one-symbol bound out of range at %u: %u\n", bs, b); return 1; }
    }
    // the grid
    for (int g = 0; g <= wrbud::kGMax; g++) {
        if (wrbud::grid_index(wrbud::grid_tol(g)) != g) { printf("grid index at %d\n", g); return 1; }
        if (g && !(wrbud::grid_tol(g) > wrbud::grid_tol(g - 1))) { printf("grid not increasing at %d\n", g); return 1; }
    }
    if (wrbud::grid_tol(0) != 0x1p-60 || wrbud::grid_tol(wrbud::kGMax) != 1.0) { printf("grid ends\n"); return 1; }

    const uint32_t sizes[] = {1, 2, 3, 15, 16, 17, 255, 256, 257, 1024, 4096, 4099, 59904, 59984, 59999};
    int bad = 0;
    for (uint32_t bs : sizes) {
        std::vector<uint8_t> p(bs);
        // one symbol, two symbols, all 256 equally, a count of 1
        std::fill(p.begin(), p.end(), 137); bad += check(p, "one symbol");
        for (uint32_t i = 0; i < bs; i++) p[i] = (i & 1) ? 255 : 0; bad += check(p, "two symbols");
        for (uint32_t i = 0; i < bs; i++) p[i] = (uint8_t)i; bad += check(p, "all equally");
        std::fill(p.begin(), p.end(), 0); p[bs / 2] = 255; bad += check(p, "a count of one");
        // every symbol 1..255 once, zeros elsewhere (the most expensive rare symbols)
        std::fill(p.begin(), p.end(), 0); for (uint32_t i = 0; i < bs && i < 255; i++) p[(size_t)i * (bs / 256 ? bs / 256 : 1) % bs] = (uint8_t)(i + 1);
        bad += check(p, "floor256");
        // rare symbols last: the coder is at its narrowest range when they come
        std::fill(p.begin(), p.end(), 7); for (uint32_t i = 0; i < bs && i < 64; i++) p[bs - 1 - i] = (uint8_t)(200 + (i & 31));
        bad += check(p, "rare last");
        for (int kind = 0; kind < 6; kind++) {
            for (uint32_t i = 0; i < bs; i++) {
                const unsigned r = rnd();
                p[i] = kind == 0 ? r & 255 : kind == 1 ? ((r & 255) < 200 ? 0 : r >> 8 & 7) : kind == 2 ? (r & 1) : kind == 3 ? (i % 251)
                     : kind == 4 ? ((r & 1023) == 0 ? r >> 10 & 255 : 1) : (uint8_t)((r & 15) * (r >> 4 & 15));
            }
            bad += check(p, "random");
        }
    }
    // random histograms of random lengths, the symbols dealt out in random order
    for (int it = 0; it < 300; it++) {
        const uint32_t bs = 1 + rnd() % wrseg::kSegMax, nsym = 1 + rnd() % 256;
        std::vector<uint8_t> p(bs);
        const unsigned skew = rnd() % 4;
        for (uint32_t i = 0; i < bs; i++) {
            unsigned r = rnd() % nsym;
            for (unsigned k = 0; k < skew; k++) r = r * (rnd() % nsym) / nsym;
            p[i] = (uint8_t)r;
        }
        bad += check(p, "random histogram");
    }
    // the plane bound against the container's pieces: header, index and the segments
    {
        std::vector<uint8_t> p(3 * 1024 + 1);
        for (size_t i = 0; i < p.size(); i++) p[i] = (uint8_t)(rnd() & 31);
        size_t sum = wrbud::blob_overhead(4);
        for (size_t k = 0; k < 4; k++) {
            const uint32_t bs = k < 3 ? 1024 : 1;
            std::vector<uint8_t> out(wrseg::stream_bound(bs));
            sum += wrseg::encode_segment_host(p.data() + 1024 * k, bs, out.data(), (uint32_t)out.size());
        }
        if (wrbud::plane_bound(p.data(), p.size(), 1024) < sum) { printf("plane bound below the blob\n"); return 1; }
    }
    if (bad) return 1;
    printf("budget bound sanitizer run OK\n");
    return 0;
}
