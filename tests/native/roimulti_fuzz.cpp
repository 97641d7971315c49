// roimulti_fuzz.cpp -- the union lists of a multi-region decode (csrc/wr_roi.h, csrc/wr_blocked.h) under ASan + UBSan.
// Host geometry only; a stand-alone program (tests/test_roi_multi_cpu.py builds and runs it).
//
// For random fields, levels and region sets: the union list is ascending, without duplicates, below nseg, and equal to the
// merge of the single-region lists; it is written into arrays of exactly its size, and with cap smaller than the count into
// arrays of exactly cap entries (the sanitizer sees a write past either).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "wr_blocked.h"
#include "wr_roi.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main()
{
    std::mt19937_64 rng(20261018);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    const uint32_t segs[] = {16, 48, 1008, 4096, 59904};
    const uint32_t bricks[] = {0, 8, 16, 32};
    size_t lists = 0;
    for (int round = 0; round < 300; round++) {
        const int nx = pick(1, 90), ny = pick(1, 60), nz = pick(1, 50);
        const int wlev = pick(0, 1) ? 4 : 0, level = pick(0, wlev), d = wlev - level;
        const uint32_t seg = segs[pick(0, 4)], B = bricks[pick(0, 3)];
        const wrlow::Box box = wrlow::box_of(nx, ny, nz, level);
        const int nroi = pick(1, 9);
        std::vector<wrroi::Geometry> g;
        for (int i = 0; i < nroi; i++) {
            wr_box r;
            r.x0 = pick(0, box.bx - 1); r.x1 = pick(r.x0 + 1, std::min(box.bx, r.x0 + 12));
            r.y0 = pick(0, box.by - 1); r.y1 = pick(r.y0 + 1, std::min(box.by, r.y0 + 12));
            r.z0 = pick(0, box.bz - 1); r.z1 = pick(r.z0 + 1, std::min(box.bz, r.z0 + 12));
            CHECK(wrroi::roi_ok(box, r), "a region of the harness is out of range");
            g.push_back(wrroi::geometry_of(box, d, r));
            if (i && pick(0, 3) == 0) g.back() = g[(size_t)pick(0, i - 1)];  // a repeated region
        }
        const size_t n = (size_t)nx * ny * nz, nseg = (n + seg - 1) / seg;
        const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, B ? B : 8);
        auto list = [&](const wrroi::Geometry* gs, size_t ng, uint32_t* ids, size_t cap) {
            return B ? wrblk::region_segments_multi(od, gs, ng, seg, ids, cap) : wrroi::segments_of_multi(nx, ny, nz, gs, ng, seg, ids, cap);
        };
        const size_t count = list(g.data(), g.size(), nullptr, 0);
        CHECK(count >= 1 && count <= nseg, "count %zu of %zu segments", count, nseg);
        std::unique_ptr<uint32_t[]> ids(new uint32_t[count]);  // exactly the union's size
        CHECK(list(g.data(), g.size(), ids.get(), count) == count, "the count changed between two calls");
        for (size_t k = 0; k < count; k++) {
            CHECK(ids[k] < nseg, "id %u of %zu segments", ids[k], nseg);
            CHECK(k == 0 || ids[k] > ids[k - 1], "not ascending or a duplicate at %zu", k);
        }
        // the merge of the single-region lists
        std::set<uint32_t> want;
        for (const wrroi::Geometry& one : g) {
            const size_t c1 = B ? wrblk::region_segments(od, one, seg, nullptr, 0) : wrroi::segments_of(nx, ny, nz, one, seg, nullptr, 0);
            std::unique_ptr<uint32_t[]> own(new uint32_t[c1]);
            if (B) wrblk::region_segments(od, one, seg, own.get(), c1);
            else wrroi::segments_of(nx, ny, nz, one, seg, own.get(), c1);
            want.insert(own.get(), own.get() + c1);
        }
        CHECK(want.size() == count && std::equal(want.begin(), want.end(), ids.get()), "the union differs from the merged lists");
        // cap smaller than the count: exactly cap entries are written, the count is still the union's
        const size_t cap = count > 1 ? (size_t)pick(0, (int)count - 1) : 0;
        std::unique_ptr<uint32_t[]> few(new uint32_t[cap ? cap : 1]);
        CHECK(list(g.data(), g.size(), few.get(), cap) == count, "the count depends on cap");
        for (size_t k = 0; k < cap; k++) CHECK(few[k] == ids[k], "the short list differs at %zu", k);
        if (B) {  // the union of the brick lists, built the same way
            std::vector<uint32_t> bl;
            wrblk::region_bricks_multi(od, g.data(), g.size(), &bl);
            std::set<uint32_t> wb;
            for (const wrroi::Geometry& one : g) {
                std::vector<uint32_t> own;
                wrblk::region_bricks(od, one, &own);
                wb.insert(own.begin(), own.end());
            }
            CHECK(wb.size() == bl.size() && std::equal(wb.begin(), wb.end(), bl.begin()), "the brick union differs from the merged lists");
            for (size_t k = 0; k < bl.size(); k++) CHECK(bl[k] < od.nbricks && (k == 0 || bl[k] > bl[k - 1]), "brick list at %zu", k);
        }
        lists++;
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("region union sanitizer run OK (%zu region sets)\n", lists);
    return 0;
}
