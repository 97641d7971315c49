// maskroi_fuzz.cpp -- the crop of a mask (csrc/wr_mask.h: wrmask::roi_segments) and the host checks of the mask blob under
// ASan + UBSan.  Host code only; a stand-alone program (tests/test_masked_roi_cases_cpu.py builds and runs it).
//
// For random fields, levels, regions and segment lengths: the list is ascending, without duplicates, below nseg, and equal to
// the brute-force set {(J >> 3) / seg} over every sample of the region; it is written into arrays of exactly its size, and with
// cap smaller than the count into arrays of exactly cap entries (the sanitizer sees a write past either).  Every bit that the
// restore kernel's definition reads -- at level 0 the bytes J0 >> 3 .. (J0 + cnt - 1) >> 3 of a turn of cnt <= 64 samples --
// lies in a listed segment and below ceil(n / 8).  Then the blob: a WRS1 plane of the packed bits behind the 32-byte header,
// held in an array of exactly its length, passes wrmask::check_header and wrseg::check_index; with a wrong magic, a nonzero
// reserved word, another n, cut short (at every length below the index's end, and one byte short) or with bytes appended it is
// refused, and the checks read nothing beyond the bytes they are given.
#define WR_MASK_HOST_ONLY
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <set>
#include <vector>

#include "wr_lowres.h"
#include "wr_mask.h"
#include "wr_segcoder.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the WRS1 blob of sym[0, n) cut at seg
static std::vector<uint8_t> wrs1_of(const std::vector<uint8_t>& sym, uint32_t seg)
{
    const size_t n = sym.size(), nseg = wrseg::seg_count(n, seg);
    std::vector<uint8_t> blob(wrseg::kHeaderBytes + 4 * nseg);
    memcpy(blob.data(), wrseg::kMagic, 4);
    wrseg::put_u32(blob.data() + 4, seg);
    wrseg::put_u32(blob.data() + 8, (uint32_t)nseg);
    std::vector<uint8_t> stream(wrseg::stream_bound(seg));
    for (size_t k = 0; k < nseg; k++) {
        const uint32_t bs = (uint32_t)(k + 1 < nseg ? seg : n - k * seg);
        const uint32_t len = wrseg::encode_segment_host(sym.data() + k * seg, bs, stream.data(), (uint32_t)stream.size());
        CHECK(len > 0, "a segment did not fit its bound");
        wrseg::put_u32(blob.data() + wrseg::kHeaderBytes + 4 * k, len);
        blob.insert(blob.end(), stream.begin(), stream.begin() + len);
    }
    return blob;
}

// both host checks of a mask blob held in an array of exactly len bytes
static bool blob_ok(const std::vector<uint8_t>& blob, size_t n)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[blob.size() ? blob.size() : 1]);
    if (!blob.empty()) memcpy(exact.get(), blob.data(), blob.size());
    unsigned long long undefined = 0;
    double pad = 0;
    if (wrmask::check_header(exact.get(), blob.size(), n, &undefined, &pad)) return false;
    uint32_t seg = 0, nseg = 0;
    const size_t rest = blob.size() - wrmask::kHeaderBytes;
    return wrseg::check_index(exact.get() + wrmask::kHeaderBytes, rest, rest, wrmask::mask_bytes(n), &seg, &nseg) == nullptr;
}

int main()
{
    std::mt19937_64 rng(20261020);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    const uint32_t segs[] = {16, 32, 48, 1008, 59904};
    size_t lists = 0, blobs = 0;
    for (int round = 0; round < 400; round++) {
        const int nx = pick(1, 150), ny = pick(1, 40), nz = pick(1, 30), level = pick(0, 4);
        const uint32_t seg = segs[pick(0, 4)];
        const wrlow::Box box = wrlow::box_of(nx, ny, nz, level);
        wrmask::Region g{nx, ny, nz, level, 0, 0, 0, box.bx, box.by, box.bz};
        if (pick(0, 3)) {
            g.x0 = pick(0, box.bx - 1); g.x1 = pick(g.x0 + 1, box.bx);
            g.y0 = pick(0, box.by - 1); g.y1 = pick(g.y0 + 1, box.by);
            g.z0 = pick(0, box.bz - 1); g.z1 = pick(g.z0 + 1, box.bz);
        }
        const size_t n = (size_t)nx * ny * nz, nsym = wrmask::mask_bytes(n), nseg = wrseg::seg_count(nsym, seg);
        const size_t count = wrmask::roi_segments(g, seg, nullptr, 0);
        CHECK(count >= 1 && count <= nseg, "count %zu of %zu segments", count, nseg);
        std::unique_ptr<uint32_t[]> ids(new uint32_t[count]);  // exactly the list's size
        CHECK(wrmask::roi_segments(g, seg, ids.get(), count) == count, "the count changed between two calls");
        std::set<uint32_t> want;
        for (int z = 0; z < g.z1 - g.z0; z++)
            for (int y = 0; y < g.y1 - g.y0; y++)
                for (int x = 0; x < g.x1 - g.x0; x++) {
                    const size_t J = g.bit(x, y, z);
                    CHECK(J < n, "bit %zu of a field of %zu samples", J, n);
                    want.insert((uint32_t)((J >> 3) / seg));
                }
        CHECK(want.size() == count, "%zu segments listed, %zu by brute force", count, want.size());
        size_t k = 0;
        for (uint32_t id : want) {
            if (k < count) CHECK(ids[k] == id, "entry %zu is %u, brute force says %u", k, ids[k], id);
            k++;
        }
        for (size_t i = 0; i < count; i++) CHECK(ids[i] < nseg && (i == 0 || ids[i] > ids[i - 1]), "entry %zu out of range or not ascending", i);
        // the bytes a level-0 turn reads
        if (level == 0)
            for (int z = 0; z < g.z1 - g.z0; z++)
                for (int y = 0; y < g.y1 - g.y0; y++)
                    for (int xs = 0; xs < g.x1 - g.x0; xs += 64) {
                        const int cnt = g.x1 - g.x0 - xs < 64 ? g.x1 - g.x0 - xs : 64;
                        const size_t J0 = g.bit(xs, y, z), b0 = J0 >> 3, bl = (J0 + cnt - 1) >> 3;
                        CHECK(bl < nsym && bl - b0 <= 8, "a turn reads bytes %zu .. %zu of %zu", b0, bl, nsym);
                        for (size_t b = b0; b <= bl; b++) CHECK(want.count((uint32_t)(b / seg)), "byte %zu lies in a segment that is not listed", b);
                    }
        if (count > 1) {  // a short array takes its first cap entries and the whole count comes back
            const size_t cap = (size_t)pick(1, (int)(count - 1 < 1000 ? count - 1 : 1000));
            std::unique_ptr<uint32_t[]> few(new uint32_t[cap]);
            CHECK(wrmask::roi_segments(g, seg, few.get(), cap) == count, "the count with a short array");
            for (size_t i = 0; i < cap; i++) CHECK(few[i] == ids[i], "entry %zu of a short array", i);
        }
        lists++;
        if (round % 8) continue;
        // ---- the blob of a random mask of this field
        std::vector<uint8_t> bits(nsym, 0);
        unsigned long long undefined = 0;
        for (size_t j = 0; j < n; j++)
            if (pick(0, 5) == 0) { bits[j >> 3] |= (uint8_t)(1u << (j & 7)); undefined++; }
        std::vector<uint8_t> blob(wrmask::kHeaderBytes);
        wrmask::put_header(blob.data(), n, undefined, 1.5);
        const std::vector<uint8_t> plane = wrs1_of(bits, seg);
        blob.insert(blob.end(), plane.begin(), plane.end());
        CHECK(wrmask::sniff(blob.data(), blob.size()), "the blob does not start like one");
        CHECK(blob_ok(blob, n), "a well-formed blob is refused");
        std::vector<uint8_t> bad = blob;
        bad[3] = '2';
        CHECK(!blob_ok(bad, n), "a wrong magic is accepted");
        bad = blob; bad[5] = 1;
        CHECK(!blob_ok(bad, n), "a nonzero reserved word is accepted");
        CHECK(!blob_ok(blob, n + 1), "a blob of another n is accepted");
        bad = blob; wrmask::put_u64(bad.data() + 16, (unsigned long long)n + 1);
        CHECK(!blob_ok(bad, n), "more undefined samples than samples is accepted");
        const size_t front = wrmask::kHeaderBytes + wrseg::kHeaderBytes + 4 * nseg;
        for (size_t len = 0; len < front && len < 200; len++) {
            bad.assign(blob.begin(), blob.begin() + (long)len);
            CHECK(!blob_ok(bad, n), "a blob cut to %zu bytes is accepted", len);
        }
        bad.assign(blob.begin(), blob.end() - 1);
        CHECK(!blob_ok(bad, n), "a blob one byte short is accepted");
        bad = blob; bad.push_back(0); bad.push_back(0);
        CHECK(!blob_ok(bad, n), "an overlong blob is accepted");
        blobs++;
    }
    printf("%zu lists, %zu blobs\n", lists, blobs);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("mask crop sanitizer run OK\n");
    return 0;
}
