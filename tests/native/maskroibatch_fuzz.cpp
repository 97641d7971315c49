// maskroibatch_fuzz.cpp -- the host side of the masked region decode across a batch of fields (csrc/wr_mask.h) under ASan +
// UBSan: wrmask::roi_segments_multi, wrmask::boxes_turns and wrmask::check_blobs.  Host code only; a stand-alone program
// (tests/test_masked_roi_batch_cases_cpu.py builds and runs it).
//
// For random fields, levels, lists of 1 .. 6 regions (overlapping, repeated) and segment lengths:
//   the union is ascending, without duplicates, below nseg, and equal to the brute-force set {(J >> 3) / seg} over every sample
//   of every region; it is written into arrays of exactly its size and, with cap below the count, of exactly cap entries;
//   first[] lives in an array of exactly nroi + 1 entries, is the exclusive prefix of ceil(cx / 64) * cy * cz, and every turn
//   t < first[nroi] found by bisection in it, as the kernel finds it, maps to a row and a turn inside its region, each
//   (region, row, turn) exactly once; every byte the turn reads at level 0 lies in a segment of the union;
//   a batch of blobs, each held in an array of exactly its length, some fields without one: all pass; with one or two of them
//   damaged (magic, reserved word, n, cut inside the index, one byte short, bytes appended) check_blobs names the FIRST damaged
//   field, and the blobs behind it are not looked at (their pointers are poisoned: not dereferenceable).
// Then the refusal of 2^31 turns.
#define WR_MASK_HOST_ONLY
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <set>
#include <string>
#include <tuple>
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

int main()
{
    std::mt19937_64 rng(20261021);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    const uint32_t segs[] = {16, 32, 48, 1008, 59904};
    size_t unions = 0, prefixes = 0, batches = 0;
    for (int round = 0; round < 300; round++) {
        const int nx = pick(1, 150), ny = pick(1, 40), nz = pick(1, 30), level = pick(0, 4);
        const uint32_t seg = segs[pick(0, 4)];
        const wrlow::Box box = wrlow::box_of(nx, ny, nz, level);
        const size_t nroi = (size_t)pick(1, 6);
        std::unique_ptr<wrmask::Region[]> gs(new wrmask::Region[nroi]);  // exactly the list's size
        for (size_t i = 0; i < nroi; i++) {
            wrmask::Region g{nx, ny, nz, level, 0, 0, 0, box.bx, box.by, box.bz};
            if (i && pick(0, 4) == 0) g = gs[(size_t)pick(0, (int)i - 1)];  // a repeated region
            else if (pick(0, 4)) {
                g.x0 = pick(0, box.bx - 1); g.x1 = pick(g.x0 + 1, box.bx);
                g.y0 = pick(0, box.by - 1); g.y1 = pick(g.y0 + 1, box.by);
                g.z0 = pick(0, box.bz - 1); g.z1 = pick(g.z0 + 1, box.bz);
            }
            gs[i] = g;
        }
        const size_t n = (size_t)nx * ny * nz, nsym = wrmask::mask_bytes(n), nseg = wrseg::seg_count(nsym, seg);
        // ---- the union
        const size_t count = wrmask::roi_segments_multi(gs.get(), nroi, seg, nullptr, 0);
        CHECK(count >= 1 && count <= nseg, "count %zu of %zu segments", count, nseg);
        std::unique_ptr<uint32_t[]> ids(new uint32_t[count]);
        CHECK(wrmask::roi_segments_multi(gs.get(), nroi, seg, ids.get(), count) == count, "the count changed between two calls");
        std::set<uint32_t> want;
        for (size_t i = 0; i < nroi; i++)
            for (int z = 0; z < gs[i].z1 - gs[i].z0; z++)
                for (int y = 0; y < gs[i].y1 - gs[i].y0; y++)
                    for (int x = 0; x < gs[i].x1 - gs[i].x0; x++) {
                        const size_t J = gs[i].bit(x, y, z);
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
        if (count > 1) {
            const size_t cap = (size_t)pick(1, (int)(count - 1 < 1000 ? count - 1 : 1000));
            std::unique_ptr<uint32_t[]> few(new uint32_t[cap]);
            CHECK(wrmask::roi_segments_multi(gs.get(), nroi, seg, few.get(), cap) == count, "the count with a short array");
            for (size_t i = 0; i < cap; i++) CHECK(few[i] == ids[i], "entry %zu of a short array", i);
        }
        unions++;
        // ---- the turn prefix
        std::unique_ptr<uint32_t[]> first(new uint32_t[nroi + 1]);
        const size_t turns = wrmask::boxes_turns(gs.get(), nroi, first.get());
        CHECK(turns == wrmask::boxes_turns(gs.get(), nroi, nullptr), "the turns without an array");
        size_t run = 0;
        for (size_t i = 0; i < nroi; i++) {
            CHECK(first[i] == run, "first[%zu] is %u, not %zu", i, first[i], run);
            run += (size_t)((gs[i].x1 - gs[i].x0 + 63) / 64) * (size_t)(gs[i].y1 - gs[i].y0) * (size_t)(gs[i].z1 - gs[i].z0);
        }
        CHECK(first[nroi] == run && turns == run && turns > 0, "first[nroi] is %u and the turns %zu, not %zu", first[nroi], turns, run);
        std::set<std::tuple<size_t, size_t, size_t>> seen;
        for (size_t t = 0; t < turns; t++) {
            size_t i = 0, end = nroi;  // (the kernel's bisection)
            while (end - i > 1) {
                const size_t mid = (i + end) >> 1;
                if (first[mid] <= t) i = mid;
                else end = mid;
            }
            CHECK(first[i] <= t && t < first[i + 1], "turn %zu is not in region %zu", t, i);
            const wrmask::Region& g = gs[i];
            const size_t cx = (size_t)(g.x1 - g.x0), cy = (size_t)(g.y1 - g.y0), cz = (size_t)(g.z1 - g.z0), tpr = (cx + 63) / 64;
            const size_t q = t - first[i], row = q / tpr, turn = q % tpr, z = row / cy, y = row % cy;
            CHECK(z < cz && turn * 64 < cx, "turn %zu leaves its region", t);
            CHECK(seen.insert(std::make_tuple(i, row, turn)).second, "turn %zu maps to a place another turn has", t);
            if (level == 0 && z < cz) {
                const size_t xs = turn * 64, cnt = cx - xs < 64 ? cx - xs : 64;
                const size_t J0 = g.bit((int)xs, (int)y, (int)z), b0 = J0 >> 3, bl = (J0 + cnt - 1) >> 3;
                CHECK(bl < nsym && bl - b0 <= 8, "a turn reads bytes %zu .. %zu of %zu", b0, bl, nsym);
                for (size_t b = b0; b <= bl; b++) CHECK(want.count((uint32_t)(b / seg)), "byte %zu lies in a segment that is not listed", b);
            }
        }
        CHECK(seen.size() == turns, "%zu places for %zu turns", seen.size(), turns);
        prefixes++;
        if (round % 6) continue;
        // ---- a batch of blobs of this field shape
        const int nfields = pick(1, 5);
        std::vector<std::vector<uint8_t>> blobs((size_t)nfields);
        for (int f = 0; f < nfields; f++) {
            if (pick(0, 3) == 0) continue;  // a field without a blob
            std::vector<uint8_t> bits(nsym, 0);
            unsigned long long undefined = 0;
            for (size_t j = 0; j < n; j++)
                if (pick(0, 5) == 0) { bits[j >> 3] |= (uint8_t)(1u << (j & 7)); undefined++; }
            blobs[f].resize(wrmask::kHeaderBytes);
            wrmask::put_header(blobs[f].data(), n, undefined, 1.5 + f);
            const std::vector<uint8_t> plane = wrs1_of(bits, segs[pick(0, 4)]);  // (every blob has its own seg)
            blobs[f].insert(blobs[f].end(), plane.begin(), plane.end());
        }
        for (int trial = 0; trial < 8; trial++) {
            // trial 0: nothing damaged; then one or two damaged fields
            std::vector<std::vector<uint8_t>> now = blobs;
            int first_bad = nfields;
            if (trial)
                for (int d = 0; d < 2; d++) {
                    const int f = pick(0, nfields - 1);
                    if (now[f].empty() || now[f].size() != blobs[f].size() || now[f] != blobs[f]) continue;  // (no blob, or damaged already)
                    std::vector<uint8_t>& b = now[f];
                    const size_t front = wrmask::kHeaderBytes + wrseg::kHeaderBytes + 4 * (size_t)wrseg::get_u32(b.data() + wrmask::kHeaderBytes + 8);
                    switch (pick(0, 5)) {
                    case 0: b[3] = '2'; break;
                    case 1: b[4 + pick(0, 3)] = 1; break;
                    case 2: wrmask::put_u64(b.data() + 8, (unsigned long long)n + 1); break;
                    case 3: b.resize((size_t)pick(0, (int)front - 1)); break;
                    case 4: b.pop_back(); break;
                    default: b.push_back(0); b.push_back(7); break;
                    }
                    if (f < first_bad) first_bad = f;
                }
            // every blob in an array of exactly its length; the blobs behind the first damaged one at an address nothing may read
            std::vector<std::unique_ptr<uint8_t[]>> exact((size_t)nfields);
            std::vector<const unsigned char*> ptrs((size_t)nfields, nullptr);
            std::vector<size_t> lens((size_t)nfields, 0);
            for (int f = 0; f < nfields; f++) {
                if (blobs[f].empty()) continue;
                lens[f] = now[f].size();
                if (f > first_bad) { ptrs[f] = reinterpret_cast<const unsigned char*>((uintptr_t)16); continue; }
                exact[f].reset(new uint8_t[now[f].size() ? now[f].size() : 1]);
                if (!now[f].empty()) memcpy(exact[f].get(), now[f].data(), now[f].size());
                ptrs[f] = exact[f].get();
            }
            std::unique_ptr<wrmask::BlobInfo[]> info(new wrmask::BlobInfo[(size_t)nfields]);
            std::string why;
            const int got = wrmask::check_blobs(ptrs.data(), lens.data(), nfields, n, info.get(), &why);
            CHECK(got == first_bad, "check_blobs names field %d, the first damaged one is %d (%s)", got, first_bad, why.c_str());
            if (got < nfields) CHECK(why.rfind("mask blob: ", 0) == 0, "the reason does not start with \"mask blob: \": %s", why.c_str());
            for (int f = 0; f < nfields && f < first_bad; f++) {
                if (blobs[f].empty()) continue;
                CHECK(info[f].seg == wrseg::get_u32(blobs[f].data() + wrmask::kHeaderBytes + 4) && info[f].nseg == wrseg::seg_count(nsym, info[f].seg),
                      "field %d: seg %u, nseg %u", f, info[f].seg, info[f].nseg);
                CHECK(info[f].pad == 1.5 + f, "field %d: pad %g", f, info[f].pad);
            }
            batches++;
        }
    }
    // ---- 2^31 turns or more are refused, one turn fewer is not
    {
        wrmask::Region rows[2] = {{1, 1 << 15, 1 << 15, 0, 0, 0, 0, 1, 1 << 15, 1 << 15}, {1, 1 << 15, 1 << 15, 0, 0, 0, 0, 1, 1 << 15, 1 << 15}};
        uint32_t first[3] = {9, 9, 9};
        CHECK(wrmask::boxes_turns(rows, 1, first) == (size_t)1 << 30 && first[1] == 1u << 30, "2^30 turns");
        CHECK(wrmask::boxes_turns(rows, 2, first) == 0, "2^31 turns are accepted");
        rows[1].z1 = (1 << 15) - 1; rows[1].y1 = 1 << 15;
        CHECK(wrmask::boxes_turns(rows, 2, first) == ((size_t)1 << 31) - (1 << 15), "2^31 - 2^15 turns");
        wrmask::Region wide{0x7fffffff, 0x7fffffff, 0x7fffffff, 0, 0, 0, 0, 0x7fffffff, 0x7fffffff, 0x7fffffff};
        CHECK(wrmask::boxes_turns(&wide, 1, nullptr) == 0, "a box of 2^31 - 1 per axis is accepted");
    }
    printf("%zu unions, %zu prefixes, %zu batches of blobs\n", unions, prefixes, batches);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("mask batch sanitizer run OK\n");
    return 0;
}
