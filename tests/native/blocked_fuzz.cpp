// ASan/UBSan harness for the host geometry of the blocked symbol order and the host reorder (csrc/wr_blocked.h), and for the
// WRS2 header check (csrc/wr_segcoder.h), compiled by g++.  Every array is an exact-size allocation: a position or an index
// outside the plane, a segment id outside the plane's segments or a brick id outside its bricks is ASan's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "wr_blocked.h"
#include "wr_segcoder.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }

static void die(const char* what, int nx, int ny, int nz, int wlev, unsigned B)
{
    printf("%s: %d x %d x %d, wlev %d, brick %u\n", what, nx, ny, nz, wlev, B);
    exit(1);
}

int main()
{
    const int shapes[][3] = {{64, 64, 64}, {200, 129, 77}, {70, 50, 1}, {40, 40, 130}, {100, 65, 39}, {1, 1, 33}, {1, 1, 1}, {17, 3, 2}};  // nx, ny, nz
    const unsigned bricks[] = {8, 16, 32, 64};
    for (const auto& sh : shapes) for (unsigned B : bricks) for (int wlev : {0, 4}) {
        const int nx = sh[0], ny = sh[1], nz = sh[2];
        const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, B);
        const size_t n = od.n();
        if (od.nbox < 1 || od.nbox > wrblk::kMaxBoxes) die("box count", nx, ny, nz, wlev, B);
        std::vector<uint64_t> pi(n);
        wrblk::fill_order(od, pi.data());
        std::vector<uint8_t> seen(n, 0);
        for (size_t p = 0; p < n; p++) {
            if (pi[p] >= n || seen[pi[p]]) die("not a permutation", nx, ny, nz, wlev, B);
            seen[pi[p]] = 1;
        }
        // the box of every level is a prefix
        for (int r = 0; r <= wlev; r++) {
            const wrlow::Box b = wrlow::box_of(nx, ny, nz, r);
            for (size_t p = 0; p < b.elems(); p++) {
                const size_t x = pi[p] % nx, y = pi[p] / nx % ny, z = pi[p] / nx / ny;
                if ((int)x >= b.bx || (int)y >= b.by || (int)z >= b.bz) die("prefix", nx, ny, nz, wlev, B);
            }
            const int nb = wrblk::prefix_boxes(od, r);
            const uint64_t end = nb < od.nbox ? od.box[nb].start : n;
            if (end != b.elems()) die("prefix boxes", nx, ny, nz, wlev, B);
        }
        // the host reorder, both ways
        std::vector<uint8_t> nat(n), blk(n), back(n);
        for (size_t i = 0; i < n; i++) nat[i] = (uint8_t)rnd();
        wrblk::reorder_host(od, nat.data(), blk.data(), false);
        for (size_t p = 0; p < n; p++) if (blk[p] != nat[pi[p]]) die("forward reorder", nx, ny, nz, wlev, B);
        wrblk::reorder_host(od, blk.data(), back.data(), true);
        if (memcmp(back.data(), nat.data(), n) != 0) die("inverse reorder", nx, ny, nz, wlev, B);
        // regions: the segments and the bricks against the permutation itself
        std::vector<uint64_t> inv(n);
        for (size_t p = 0; p < n; p++) inv[pi[p]] = p;
        for (int trial = 0; trial < 6; trial++) {
            const int level = wlev ? (int)(rnd() % 5) : 0;
            const wrlow::Box b = wrlow::box_of(nx, ny, nz, level);
            wr_box roi;
            roi.x0 = (int)(rnd() % b.bx); roi.x1 = roi.x0 + 1 + (int)(rnd() % (b.bx - roi.x0));
            roi.y0 = (int)(rnd() % b.by); roi.y1 = roi.y0 + 1 + (int)(rnd() % (b.by - roi.y0));
            roi.z0 = (int)(rnd() % b.bz); roi.z1 = roi.z0 + 1 + (int)(rnd() % (b.bz - roi.z0));
            const wrroi::Geometry g = wrroi::geometry_of(b, wlev - level, roi);
            for (uint32_t seg : {16u, 1008u, 59904u}) {
                const size_t nseg = (n + seg - 1) / seg;
                std::vector<uint8_t> want(nseg, 0);
                for (int i = 0; i < g.nbox; i++) {
                    const wrroi::SrcBox& sb = g.box[i];
                    for (int z = sb.src[2]; z < sb.src[2] + sb.len[2]; z++)
                        for (int y = sb.src[1]; y < sb.src[1] + sb.len[1]; y++)
                            for (int x = sb.src[0]; x < sb.src[0] + sb.len[0]; x++) want[inv[((size_t)y + (size_t)ny * z) * nx + x] / seg] = 1;
                }
                const size_t count = wrblk::region_segments(od, g, seg, nullptr, 0);
                std::vector<uint32_t> ids(count);
                if (wrblk::region_segments(od, g, seg, ids.data(), ids.size()) != count) die("segment count", nx, ny, nz, wlev, B);
                size_t k = 0;
                for (size_t j = 0; j < nseg; j++)
                    if (want[j]) { if (k >= count || ids[k] != j) die("segment list", nx, ny, nz, wlev, B); k++; }
                if (k != count) die("segment list length", nx, ny, nz, wlev, B);
            }
            std::vector<uint32_t> bl;
            wrblk::region_bricks(od, g, &bl);
            for (size_t j = 0; j < bl.size(); j++) if (bl[j] >= od.nbricks || (j && bl[j] <= bl[j - 1])) die("brick list", nx, ny, nz, wlev, B);
        }
    }
    // the header of a WRS2 blob: every brick value but the four is refused, nothing is read beyond `have`
    {
        const size_t n = 5000;
        const uint32_t seg = 1008, nseg = (uint32_t)((n + seg - 1) / seg);
        for (uint32_t brick = 0; brick <= 130; brick++) {
            std::vector<uint8_t> blob(wrseg::kHeaderBytesBlocked + 4 * nseg);
            memcpy(blob.data(), wrseg::kMagicBlocked, 4);
            wrseg::put_u32(blob.data() + 4, seg);
            wrseg::put_u32(blob.data() + 8, nseg);
            wrseg::put_u32(blob.data() + 12, brick);
            for (uint32_t k = 0; k < nseg; k++) wrseg::put_u32(blob.data() + 16 + 4 * k, 0);
            uint32_t s0 = 0, k0 = 0, b0 = 77;
            const char* why = wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0, &b0);
            const bool good = brick == 8 || brick == 16 || brick == 32 || brick == 64;
            if (good != (why == nullptr)) { printf("brick %u: %s\n", brick, why ? why : "accepted"); return 1; }
            if (good && (s0 != seg || k0 != nseg || b0 != brick)) { printf("brick %u: header values\n", brick); return 1; }
            if (!wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0)) { printf("a WRS2 blob passed as WRS1\n"); return 1; }
            for (size_t have = 0; have < blob.size(); have++) {  // a front that is cut short: refused, never read past
                std::vector<uint8_t> cut(blob.begin(), blob.begin() + have);
                if (!wrseg::check_index(cut.data(), cut.size(), blob.size(), n, &s0, &k0, &b0)) { printf("a cut index passed\n"); return 1; }
            }
        }
    }
    printf("blocked order sanitizer run OK\n");
    return 0;
}
