// ASan/UBSan harness for the record templates of stranded segments ("WRS3") that the GPU kernels run (csrc/wr_segcoder.h),
// compiled by g++: GPU sanitizers are not available, so the bounds of that code are checked here, on the inputs a file can
// contain.  Every buffer is an exact-size allocation: any over-read or over-write is ASan's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "wr_segcoder.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }

// a symbol sink that counts every put and tells when one would have left the strand
struct CountingSink {
    uint8_t* p;
    uint32_t cap, pos, outside;
    void put(uint32_t v) { if (pos < cap) p[pos] = (uint8_t)v; else outside++; pos++; }
};

// The record in `rec` (exact size) as a segment of bs symbols, the way a kernel lane does it: the length words, T, then strand
// j through a sink of exactly the strand's size.  Returns the ORed reasons; *written counts the symbols put.
static uint32_t decode(const std::vector<uint8_t>& rec, uint32_t bs, uint32_t seg, uint32_t K, std::vector<uint8_t>& dst, uint32_t* written)
{
    const uint32_t L = wrseg::strand_len(seg, K);
    const uint8_t* const lo = rec.data();
    const uint8_t* const hi = rec.data() + rec.size();
    uint32_t why = 0;
    *written = 0;
    for (uint32_t j = 0; j < K; j++) {
        uint32_t tlen = 0, off = 0, len = 0;
        if (const uint32_t w = wrseg::check_record(rec.data(), rec.size(), K, L, bs, j, &tlen, &off, &len)) return w;
        if ((size_t)4 * (K + 1) + tlen > rec.size() || (size_t)off + len > rec.size()) { printf("check_record passed a piece outside the record\n"); exit(1); }
        wrseg::HostTable tab;
        wrseg::Dec d;
        d.in.open(rec.data() + 4 * (size_t)(K + 1), tlen, lo, hi);
        if (const uint32_t w = wrseg::decode_model(d, tab, bs)) return w;
        const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
        if (!m) continue;
        std::vector<uint8_t> strand(m);  // exact size
        CountingSink sink{strand.data(), m, 0, 0};
        d.in.open(rec.data() + off, len, lo, hi);
        why |= wrseg::decode_strand(d, tab, sink, m, bs);
        if (sink.outside || sink.pos != m) { printf("a strand decoder put %u symbols into a strand of %u\n", sink.pos, m); exit(1); }
        memcpy(dst.data() + s0, strand.data(), m);
        *written += m;
    }
    return why;
}

int main()
{
    const uint32_t segs[] = {16, 48, 512, 4096, 59904, 59984};
    const uint32_t Ks[] = {1, 2, 4, 8, 16, 32};
    for (uint32_t seg : segs) for (uint32_t K : Ks) {
        if (!wrseg::strands_ok(K, seg)) continue;
        const uint32_t L = wrseg::strand_len(seg, K);
        if (L % 16 || (size_t)K * L < seg || (K > 1 && (size_t)(K - 1) * L >= seg + 16 * (size_t)K)) { printf("strand_len(%u, %u)\n", seg, K); return 1; }
        const uint32_t sizes[] = {1, 15, 16, 17, L - 1, L, L + 1, seg - 1, seg};
        for (uint32_t bs : sizes) for (int kind = 0; kind < 5; kind++) {
            if (bs < 1 || bs > seg) continue;
            if (seg > 5000 && (bs != seg && bs != L + 1)) continue;
            std::vector<uint8_t> p(bs), back(bs);
            for (uint32_t i = 0; i < bs; i++) {
                const unsigned r = rnd();
                // kind 4: one strand uniform over symbols the rest of the segment never uses -- the expensive case of the bound
                p[i] = kind == 0 ? r & 255 : kind == 1 ? ((r & 255) < 200 ? 0 : r >> 8 & 7) : kind == 2 ? 255 : kind == 3 ? (i % 251)
                                                                                                           : (i / L == K / 2 ? 1 + i % 255 : 0);
            }
            const uint32_t bound = wrseg::record_bound(seg, K);
            std::vector<uint8_t> out(bound);
            const uint32_t len = wrseg::encode_record_host(p.data(), bs, seg, K, out.data(), bound);
            if (!len || (len & 3)) { printf("record does not fit its bound seg=%u K=%u bs=%u kind=%d\n", seg, K, bs, kind); return 1; }
            // the pieces respect their own bounds
            if (wrseg::get_u32(out.data()) > wrseg::kModelBound) { printf("T above its bound\n"); return 1; }
            for (uint32_t j = 0; j < K; j++) {
                const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0, sl = wrseg::get_u32(out.data() + 4 * (j + 1));
                if (sl > (m ? 2 * m + 5 : 0)) { printf("strand of %u symbols takes %u bytes seg=%u K=%u kind=%d\n", m, sl, seg, K, kind); return 1; }
            }
            // a buffer one byte short is refused, not overrun
            std::vector<uint8_t> tight(len - 1);
            if (wrseg::encode_record_host(p.data(), bs, seg, K, tight.data(), (uint32_t)tight.size()) != 0) { printf("short buffer not refused\n"); return 1; }
            const std::vector<uint8_t> exact(out.begin(), out.begin() + len);
            // round trip, at every alignment of the record's address (the host reads blobs anywhere)
            for (uint32_t shift = 0; shift < 4; shift++) {
                std::vector<uint8_t> blob(shift + len);
                memcpy(blob.data() + shift, exact.data(), len);
                std::fill(back.begin(), back.end(), 0xEE);
                if (wrseg::decode_record_host(blob.data() + shift, len, blob.data(), blob.data() + blob.size(), back.data(), bs, seg, K) ||
                    memcmp(back.data(), p.data(), bs)) { printf("round trip failed seg=%u K=%u bs=%u kind=%d shift=%u\n", seg, K, bs, kind, shift); return 1; }
            }
            uint32_t written = 0;
            std::fill(back.begin(), back.end(), 0xEE);
            if (decode(exact, bs, seg, K, back, &written) || written != bs || memcmp(back.data(), p.data(), bs)) { printf("lane-wise round trip failed\n"); return 1; }
            // the wrong segment length is refused before a symbol is written
            if (bs > 1) {
                std::vector<uint8_t> dst(bs - 1);
                if (!decode(exact, bs - 1, seg, K, dst, &written) || written) { printf("wrong length not refused seg=%u K=%u bs=%u\n", seg, K, bs); return 1; }
            }
            // truncated, bit-flipped and random records: a flag or bs symbols, never more, never a crash
            const int trials = seg > 5000 ? 6 : 12;
            for (int trial = 0; trial < trials; trial++) {
                std::vector<uint8_t> bad(exact);
                if (trial % 3 == 0) bad.resize(((size_t)len * (trial / 3) / 4) & ~(size_t)3);
                else if (trial % 3 == 1) for (int k = 0; k < 1 + trial; k++) bad[rnd() % bad.size()] ^= (uint8_t)(1 + rnd() % 255);
                else {
                    // random bytes behind consistent length words, so that the coder loops are reached
                    for (size_t i = 4 * (size_t)(K + 1); i < bad.size(); i++) bad[i] = (uint8_t)rnd();
                }
                bad.shrink_to_fit();
                std::vector<uint8_t> dst(bs);
                const uint32_t rc = decode(bad, bs, seg, K, dst, &written);
                if (!rc && written != bs) { printf("a good record of %u symbols for a segment of %u\n", written, bs); return 1; }
                std::vector<uint8_t> dst2(bs);
                (void)wrseg::decode_record_host(bad.data(), bad.size(), bad.data(), bad.data() + bad.size(), dst2.data(), bs, seg, K);
            }
        }
    }
    // the container: a damaged header or index is refused by check_index, or every record decodes or is flagged inside its bounds
    {
        const uint32_t seg = 4096, K = 8; const size_t n = 3 * 4096 + 7;
        std::vector<uint8_t> p(n);
        for (auto& b : p) b = (uint8_t)(rnd() & 15);
        std::vector<uint8_t> blob(wrseg::kHeaderBytesStrands + 4 * 4);
        memcpy(blob.data(), wrseg::kMagicStrands, 4);
        wrseg::put_u32(blob.data() + 4, seg); wrseg::put_u32(blob.data() + 8, 4); wrseg::put_u32(blob.data() + 12, 0); wrseg::put_u32(blob.data() + 16, K);
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t bs = k < 3 ? seg : 7;
            std::vector<uint8_t> out(wrseg::record_bound(seg, K));
            const uint32_t len = wrseg::encode_record_host(p.data() + (size_t)k * seg, bs, seg, K, out.data(), (uint32_t)out.size());
            wrseg::put_u32(blob.data() + wrseg::kHeaderBytesStrands + 4 * k, len);
            blob.insert(blob.end(), out.begin(), out.begin() + len);
        }
        uint32_t s0 = 0, k0 = 0, b0 = 7, K0 = 0;
        if (wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0, &b0, &K0) || s0 != seg || k0 != 4 || b0 != 0 || K0 != K) { printf("good index refused\n"); return 1; }
        if (!wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0, &b0) || !wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0)) {
            printf("a WRS3 blob passed a WRS1 / WRS2 reader\n"); return 1;
        }
        for (size_t have = 0; have < 36; have++) {  // a front that is cut short: refused, never read past
            std::vector<uint8_t> cut(blob.begin(), blob.begin() + have);
            if (!wrseg::check_index(cut.data(), cut.size(), blob.size(), n, &s0, &k0, &b0, &K0)) { printf("a cut index passed\n"); return 1; }
        }
        for (int trial = 0; trial < 3000; trial++) {
            std::vector<uint8_t> bad(blob);
            bad[rnd() % 36] ^= (uint8_t)(1 + rnd() % 255);
            if (trial & 1) bad.resize(rnd() % bad.size());
            bad.shrink_to_fit();
            if (wrseg::check_index(bad.data(), bad.size(), bad.size(), n, &s0, &k0, &b0, &K0)) continue;
            if (!K0) continue;  // (the damage made it a WRS1 / WRS2 header that happens to be consistent: tests/native/seg_fuzz.cpp)
            if (b0) continue;   // (another symbol order, the same records)
            size_t at = wrseg::kHeaderBytesStrands + 4 * (size_t)k0;
            uint32_t flagged = 0;
            for (uint32_t k = 0; k < k0; k++) {
                const size_t base = (size_t)k * s0;
                const uint32_t bs = n - base < s0 ? (uint32_t)(n - base) : s0, l = wrseg::get_u32(bad.data() + wrseg::kHeaderBytesStrands + 4 * k);
                std::vector<uint8_t> dst(bs);
                flagged += wrseg::decode_record_host(bad.data() + at, l, bad.data(), bad.data() + bad.size(), dst.data(), bs, s0, K0) != 0;
                at += l;
            }
            if (!flagged) { printf("damaged index accepted and decoded (trial %d)\n", trial); return 1; }
        }
    }
    printf("strand coder sanitizer run OK\n");
    return 0;
}
