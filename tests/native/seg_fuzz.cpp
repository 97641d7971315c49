// ASan/UBSan harness for the segment coder step that the GPU kernels run (csrc/wr_segcoder.h), compiled by g++: GPU
// sanitizers are not available, so the bounds of that code are checked here, on the inputs a file can contain.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "wr_rangecoder.h"
#include "wr_segcoder.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }

// a symbol sink that counts every put and tells when one would have left the segment
struct CountingSink {
    uint8_t* p;
    uint32_t cap, pos, outside;
    void put(uint32_t v) { if (pos < cap) p[pos] = (uint8_t)v; else outside++; pos++; }
};

// decodes `len` bytes at `stream` (an exact-size allocation: any over-read is ASan's) as a segment of bs symbols
static uint32_t decode(const std::vector<uint8_t>& stream, uint32_t bs, std::vector<uint8_t>& dst, uint32_t* written)
{
    wrseg::HostTable tab;
    wrseg::Dec d;
    d.in.open(stream.data(), (uint32_t)stream.size(), stream.data(), stream.data() + stream.size());
    CountingSink sink{dst.data(), bs, 0, 0};
    const uint32_t rc = wrseg::decode_segment(d, tab, sink, bs);
    *written = sink.pos;
    if (sink.outside || sink.pos > bs) { printf("decoder wrote %u symbols into a segment of %u\n", sink.pos, bs); exit(1); }
    return rc;
}

int main()
{
    const uint32_t sizes[] = {1, 2, 3, 15, 16, 17, 255, 4096, 4099, 59904, 59984, 59999};
    for (uint32_t bs : sizes) for (int kind = 0; kind < 5; kind++) {
        std::vector<uint8_t> p(bs), ref(wrrc::encode_bound(bs)), back(bs);
        for (uint32_t i = 0; i < bs; i++) {
            const unsigned r = rnd();
            p[i] = kind == 0 ? r & 255 : kind == 1 ? ((r & 255) < 200 ? 0 : r >> 8 & 7) : kind == 2 ? 255 : kind == 3 ? (i % 251) : ((r & 1023) == 0 ? 255 : 1);
        }
        // the segment stream is the host range coder's stream of the same symbols, byte for byte, and fits the bound exactly sized
        const size_t want = wrrc::encode_plane(p.data(), bs, ref.data(), nullptr);
        std::vector<uint8_t> out(wrseg::stream_bound(bs));
        if (out.size() != wrrc::encode_bound(bs)) { printf("stream_bound(%u) is not encode_bound\n", bs); return 1; }
        const uint32_t len = wrseg::encode_segment_host(p.data(), bs, out.data(), (uint32_t)out.size());
        if (len != want || memcmp(out.data(), ref.data(), len)) { printf("segment stream differs from encode_plane bs=%u kind=%d\n", bs, kind); return 1; }
        // a buffer one byte short is refused, not overrun
        std::vector<uint8_t> tight(len - 1);
        if (wrseg::encode_segment_host(p.data(), bs, tight.data(), (uint32_t)tight.size()) != 0) { printf("short buffer not refused\n"); return 1; }
        const std::vector<uint8_t> exact(out.begin(), out.begin() + len);
        // ... at every alignment of the stream inside a larger blob (the reader fetches aligned words inside the blob only)
        for (uint32_t shift = 0; shift < 4; shift++) {
            std::vector<uint8_t> blob(shift + len);
            memcpy(blob.data() + shift, exact.data(), len);
            std::fill(back.begin(), back.end(), 0xEE);
            if (wrseg::decode_segment_host(blob.data() + shift, len, blob.data(), blob.data() + blob.size(), back.data(), bs) != wrseg::kSegOk ||
                memcmp(back.data(), p.data(), bs)) { printf("round trip failed bs=%u kind=%d shift=%u\n", bs, kind, shift); return 1; }
        }
        uint32_t written = 0;
        // the wrong segment length is refused before a symbol is written
        if (bs > 1) {
            std::vector<uint8_t> dst(bs - 1);
            if (decode(exact, bs - 1, dst, &written) != wrseg::kSegLength || written) { printf("wrong length not refused bs=%u\n", bs); return 1; }
        }
        // truncated, bit-flipped and random streams: a flag or bs symbols, never more, never a crash
        for (int trial = 0; trial < 12; trial++) {
            std::vector<uint8_t> bad(exact);
            if (trial < 4) bad.resize((size_t)len * trial / 4);
            else if (trial < 8) for (int k = 0; k < 1 + trial; k++) bad[rnd() % bad.size()] ^= (uint8_t)(1 + rnd() % 255);
            else { bad.resize(1 + rnd() % (2 * len)); for (auto& b : bad) b = (uint8_t)rnd(); if (trial & 1) bad[0] = 0; }
            bad.shrink_to_fit();
            std::vector<uint8_t> dst(bs);
            const uint32_t rc = decode(bad, bs, dst, &written);
            if (rc == wrseg::kSegOk && written != bs) { printf("a good stream of %u symbols for a segment of %u\n", written, bs); return 1; }
        }
    }
    // the container: a blob with a damaged index is refused by check_index, or its segments are flagged
    {
        const uint32_t seg = 4096; const size_t n = 3 * 4096 + 7;
        std::vector<uint8_t> p(n);
        for (auto& b : p) b = (uint8_t)(rnd() & 15);
        std::vector<uint8_t> blob(wrseg::kHeaderBytes + 4 * 4);
        memcpy(blob.data(), wrseg::kMagic, 4); wrseg::put_u32(blob.data() + 4, seg); wrseg::put_u32(blob.data() + 8, 4);
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t bs = k < 3 ? seg : 7;
            std::vector<uint8_t> out(wrseg::stream_bound(bs));
            const uint32_t len = wrseg::encode_segment_host(p.data() + (size_t)k * seg, bs, out.data(), (uint32_t)out.size());
            wrseg::put_u32(blob.data() + wrseg::kHeaderBytes + 4 * k, len);
            blob.insert(blob.end(), out.begin(), out.begin() + len);
        }
        uint32_t s0 = 0, k0 = 0;
        if (wrseg::check_index(blob.data(), blob.size(), blob.size(), n, &s0, &k0) || s0 != seg || k0 != 4) { printf("good index refused\n"); return 1; }
        for (int trial = 0; trial < 2000; trial++) {
            std::vector<uint8_t> bad(blob);
            bad[rnd() % 28] ^= (uint8_t)(1 + rnd() % 255);
            if (trial & 1) bad.resize(rnd() % bad.size());
            bad.shrink_to_fit();
            if (wrseg::check_index(bad.data(), bad.size(), bad.size(), n, &s0, &k0)) continue;
            // accepted: the damage left a consistent index (another legal segment length with the same segment count).  Its
            // segments then announce lengths that are not theirs: every one decodes or is flagged inside its own bounds.
            size_t at = wrseg::kHeaderBytes + 4 * (size_t)k0;
            uint32_t flagged = 0;
            for (uint32_t k = 0; k < k0; k++) {
                const size_t base = (size_t)k * s0;
                const uint32_t bs = n - base < s0 ? (uint32_t)(n - base) : s0, l = wrseg::get_u32(bad.data() + wrseg::kHeaderBytes + 4 * k);
                std::vector<uint8_t> dst(bs);
                flagged += wrseg::decode_segment_host(bad.data() + at, l, bad.data(), bad.data() + bad.size(), dst.data(), bs) != wrseg::kSegOk;
                at += l;
            }
            if (!flagged) { printf("damaged index accepted and decoded (trial %d)\n", trial); return 1; }
        }
    }
    printf("segment coder sanitizer run OK\n");
    return 0;
}
