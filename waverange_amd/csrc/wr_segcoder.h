// wr_segcoder.h -- the coder of one SEGMENT of a segmented plane stream ("WRS1"), shared by host and device.
// (Further down: "WRS3", the same segments coded as K strands that share the segment's model.)
//
// A plane of n symbols is cut into segments of `seg` symbols (the last one shorter); every segment is a complete rngcod13
// stream of its own, byte for byte what wr_range_encode gives for those symbols.  Because seg < 60000, a segment is ONE block
// of the reference's model (src/core/wrappers.cpp:68-149): the start byte, "a block follows", 256 counts, the symbols,
// "no more blocks", done_encoding.  The arithmetic is Schindler's (src/rangecod/rangecod.c:170-404), in the form that
// never goes back to a byte it has written: the carry is kept as a held byte and a count of pending 0xff bytes
// (rangecod.c:182-207) -- a GPU lane therefore never re-reads its own stores, and the output is append-only.
//
// Everything here is plain C++ templates over three small policies, so that g++ compiles it for the host reference of the
// format and for the sanitizer tests, and hipcc for the kernels of wr_segcoder.hip:
//   Table   get(s) / set(s, v): 256 words; word s holds the symbol's cumulative count in its low half and its count in
//           its high half (both < 65536 since a segment has fewer than 60000 symbols)
//   Source  load16(i, w[4]) and byte(i): the segment's symbols
//   Sink    put(b): the coded bytes, in order; a sink refuses what does not fit and remembers that it did
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define WRSEG_HD __host__ __device__ inline
#else
#define WRSEG_HD inline
#endif

namespace wrseg {

constexpr uint32_t kTop = 0x80000000u, kBottom = 0x00800000u;  // rangecod.c:120-129
constexpr int kShift = 23, kExtra = 7;
constexpr uint32_t kSegMin = 16, kSegMax = 59999, kSegDefault = 59904;
constexpr size_t kHeaderBytes = 12;  // magic, seg, nseg
constexpr uint8_t kMagic[4] = {'W', 'R', 'S', '1'};
// "WRS2": the same container over the plane in the blocked symbol order (wr_blocked.h); its header has a fourth word, the
// brick edge.  Everywhere below `brick` == 0 stands for a WRS1 blob.
constexpr size_t kHeaderBytesBlocked = 16;  // magic, seg, nseg, brick
constexpr uint8_t kMagicBlocked[4] = {'W', 'R', 'S', '2'};
WRSEG_HD size_t header_bytes(uint32_t brick) { return brick ? kHeaderBytesBlocked : kHeaderBytes; }
WRSEG_HD bool brick_ok(uint32_t b) { return b == 8 || b == 16 || b == 32 || b == 64; }

WRSEG_HD bool seg_ok(uint32_t seg) { return seg >= kSegMin && seg <= kSegMax && seg % 16 == 0; }
WRSEG_HD size_t seg_count(size_t n, uint32_t seg) { return (n + seg - 1) / seg; }
// wr_range_encode_bound(bs) for bs < 60000: what one segment stream can take at most (wrrc::encode_bound, two blocks)
WRSEG_HD uint32_t stream_bound(uint32_t bs) { return bs + bs / 32 + 2 * 520 + 1024; }

// ---- encoder ---------------------------------------------------------------------------------------------------------
template <class Sink>
struct Enc {
    uint32_t low, range, pending, nbytes, held;
    Sink out;

    WRSEG_HD void start()
    {
        low = 0; range = kTop; held = 0; pending = 0; nbytes = 0;  // rangecod.c:170-176, start byte 0
    }
    WRSEG_HD void renorm()  // rangecod.c:182-207
    {
        while (range <= kBottom) {
            if (low < (0xffu << kShift)) {
                out.put(held);
                for (; pending; pending--) out.put(0xff);
                held = low >> kShift;
            } else if (low & kTop) {
                out.put(held + 1);
                for (; pending; pending--) out.put(0x00);
                held = (low >> kShift) & 0xff;
            } else
                pending++;
            range <<= 8;
            low = (low << 8) & (kTop - 1);
            nbytes++;
        }
    }
    WRSEG_HD void freq(uint32_t sy, uint32_t lt, uint32_t tot)  // rangecod.c:217-229
    {
        renorm();
        const uint32_t r = range / tot, t = r * lt;
        low += t;
        range -= t;
        if (lt + sy < tot) range = r * sy;
    }
    WRSEG_HD void shift16(uint32_t lt)  // encode_short: rangecod.c:231-245 with sy = 1, shift = 16
    {
        renorm();
        const uint32_t r = range >> 16, t = r * lt;
        low += t;
        if ((lt + 1) >> 16) range -= t;
        else range = r;
    }
    WRSEG_HD void finish()  // rangecod.c:254-276
    {
        renorm();
        nbytes += 5;
        uint32_t t = low >> kShift;
        if (!((low & (kBottom - 1)) < ((nbytes & 0xffffffu) >> 1))) t++;
        if (t > 0xff) {
            out.put(held + 1);
            for (; pending; pending--) out.put(0x00);
        } else {
            out.put(held);
            for (; pending; pending--) out.put(0xff);
        }
        out.put(t & 0xff);
        out.put((nbytes >> 16) & 0xff);
        out.put((nbytes >> 8) & 0xff);
        out.put(nbytes & 0xff);
    }
};

// tab := the segment's model.  In: every word zero.  Out: word s = count << 16 | cumulative count below s.
template <class Table, class Source>
WRSEG_HD void build_model(Table& tab, Source& src, uint32_t bs)
{
    uint32_t i = 0;
    for (; i + 16 <= bs; i += 16) {
        uint32_t w[4];
        src.load16(i, w);
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 16; j++) {
            const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
            tab.set(c, tab.get(c) + 0x10000u);
        }
    }
    for (; i < bs; i++) {
        const uint32_t c = src.byte(i);
        tab.set(c, tab.get(c) + 0x10000u);
    }
    uint32_t cum = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t v = tab.get(s);  // (count << 16; a count is at most bs < 60000)
        tab.set(s, v | cum);
        cum += v >> 16;
    }
}

// One segment of bs symbols (1 <= bs <= kSegMax) into e.out: at most stream_bound(bs) bytes.  tab as build_model left it.
template <class Table, class Source, class Sink>
WRSEG_HD void encode_segment(Enc<Sink>& e, Table& tab, Source& src, uint32_t bs)
{
    e.start();
    e.freq(1, 1, 2);  // "a block follows"
    for (uint32_t s = 0; s < 256; s++) e.shift16(tab.get(s) >> 16);
    uint32_t i = 0;
    for (; i + 16 <= bs; i += 16) {
        uint32_t w[4];
        src.load16(i, w);
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 16; j++) {
            const uint32_t v = tab.get((w[j >> 2] >> (8 * (j & 3))) & 0xff);
            e.freq(v >> 16, v & 0xffff, bs);
        }
    }
    for (; i < bs; i++) {
        const uint32_t v = tab.get(src.byte(i));
        e.freq(v >> 16, v & 0xffff, bs);
    }
    e.freq(1, 0, 2);  // "no more blocks"
    e.finish();
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
// The bytes [0, len) at `in`; past the end it reads zeros (as the oracle's dec_get: the reference reads its last renormalisation
// bytes from behind the stream).  It fetches the 4-byte-aligned word a byte lies in when that word lies inside
// [lo, hi) -- the blob the stream is part of -- and single bytes of the stream otherwise, so it never touches memory outside.
struct Reader {
    const uint8_t* in;
    const uint8_t* lo;
    const uint8_t* hi;
    uint32_t len, pos, word;

    WRSEG_HD void open(const uint8_t* stream, uint32_t n, const uint8_t* blob_lo, const uint8_t* blob_hi)
    {
        in = stream; len = n; pos = 0; word = 0; lo = blob_lo; hi = blob_hi;
        if (len) fetch();
    }
    WRSEG_HD void fetch()  // word := the aligned word that in[pos] lies in (bytes outside the stream: whatever is there, or zero)
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(in + pos) & ~(uintptr_t)3;
        const uint8_t* const p = reinterpret_cast<const uint8_t*>(a);
        if (p >= lo && p + 4 <= hi) {
#if defined(__HIP_DEVICE_COMPILE__)
            word = *reinterpret_cast<const uint32_t*>(p);
#else
            memcpy(&word, p, 4);
#endif
        } else {
            word = 0;
            for (int k = 0; k < 4; k++)
                if (p + k >= in && p + k < in + len) word |= (uint32_t)p[k] << (8 * k);
        }
    }
    WRSEG_HD uint32_t get()
    {
        if (pos >= len) { pos++; return 0; }
        const uint32_t k = (uint32_t)(reinterpret_cast<uintptr_t>(in + pos) & 3);
        const uint32_t b = (word >> (8 * k)) & 0xff;
        pos++;
        if (k == 3 && pos < len) fetch();
        return b;
    }
};

struct Dec {
    uint32_t low, range, help, held;
    Reader in;

    WRSEG_HD void start()  // rangecod.c:282-291
    {
        (void)in.get();  // the byte given to start_encoding
        held = in.get();
        low = held >> (8 - kExtra);
        range = 1u << kExtra;
        help = 0;
    }
    WRSEG_HD void renorm()  // rangecod.c:294-302
    {
        while (range <= kBottom) {
            low = (low << 8) | ((held << kExtra) & 0xff);
            held = in.get();
            low |= held >> (8 - kExtra);
            range <<= 8;
        }
    }
    // help cannot be zero in either of the two: after renorm() range > 2^23, and tot < 2^16 (a shift of 16 likewise), so help >= 2^7
    WRSEG_HD uint32_t culfreq(uint32_t tot)  // rangecod.c:309-319
    {
        renorm();
        help = range / tot;
        const uint32_t t = low / help;
        return t >= tot ? tot - 1 : t;
    }
    WRSEG_HD uint32_t culshift16()  // rangecod.c:321-331
    {
        renorm();
        help = range >> 16;
        const uint32_t t = low / help;
        return (t >> 16) ? 0xffffu : t;
    }
    WRSEG_HD void update(uint32_t sy, uint32_t lt, uint32_t tot)  // rangecod.c:339-351
    {
        const uint32_t t = help * lt;
        low -= t;
        if (lt + sy < tot) range = help * sy;
        else range -= t;
    }
};

// why a segment stream was refused (0: it decoded)
enum : uint32_t { kSegOk = 0, kSegNoBlock = 1, kSegLength = 2, kSegTrailer = 3, kSegOverflow = 4 };

// Decodes one segment stream into exactly `bs` symbols through sink.put -- `bs` is what the container says the segment holds;
// a stream whose header announces another length is refused before a symbol is written, so the symbol loop runs `bs` steps
// whatever the bytes are.  Returns kSegOk or the reason.
template <class Table, class Sink>
WRSEG_HD uint32_t decode_segment(Dec& d, Table& tab, Sink& sink, uint32_t bs)
{
    d.start();
    if (!d.culfreq(2)) return kSegNoBlock;
    d.update(1, 1, 2);
    uint32_t sum = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t c = d.culshift16() & 0xffffu;  // decode_short, rangecod.c:362-366
        d.update(1, c, 1u << 16);
        tab.set(s, c << 16);
        sum += c;  // (256 counts below 65536: no overflow)
    }
    if (sum != bs || bs == 0) return kSegLength;
    uint32_t cum = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t v = tab.get(s);
        tab.set(s, v | cum);
        cum += v >> 16;
    }
    for (uint32_t i = 0; i < bs; i++) {
        const uint32_t cf = d.culfreq(bs);  // < bs
        // the symbol: the last s whose cumulative count is <= cf.  (Its count is not zero: a symbol that never occurs shares
        // its cumulative count with the next one, and the last symbol's is bs > cf if it never occurs.)
        uint32_t s = 0;
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (uint32_t step = 128; step; step >>= 1)
            if ((tab.get(s + step) & 0xffff) <= cf) s += step;
        const uint32_t v = tab.get(s);
        d.update(v >> 16, v & 0xffff, bs);
        sink.put(s);
    }
    if (d.culfreq(2)) return kSegTrailer;  // a second block: not a segment of this format
    d.update(1, 0, 2);
    d.renorm();  // done_decoding, rangecod.c:371-373
    return kSegOk;
}

// ---- host policies and the host reference of the container -----------------------------------------------------------
struct HostTable {
    uint32_t w[256];
    inline uint32_t get(uint32_t s) const { return w[s]; }
    inline void set(uint32_t s, uint32_t v) { w[s] = v; }
};
struct HostSource {
    const uint8_t* p;
    inline void load16(uint32_t i, uint32_t out[4]) const { memcpy(out, p + i, 16); }
    inline uint32_t byte(uint32_t i) const { return p[i]; }
};
struct HostByteSink {  // coded bytes into [p, p + cap)
    uint8_t* p;
    uint32_t cap, pos;
    bool overflow;
    inline void put(uint32_t b)
    {
        if (pos < cap) p[pos] = (uint8_t)b;
        else overflow = true;
        pos++;
    }
};
struct HostSymSink {  // decoded symbols into [p, p + cap)
    uint8_t* p;
    uint32_t cap, pos;
    inline void put(uint32_t s)
    {
        if (pos < cap) p[pos] = (uint8_t)s;
        pos++;
    }
};

// one segment on the host; returns the stream's length, 0 if it did not fit into cap bytes
inline uint32_t encode_segment_host(const uint8_t* sym, uint32_t bs, uint8_t* out, uint32_t cap)
{
    HostTable tab;
    memset(tab.w, 0, sizeof tab.w);
    HostSource src{sym};
    build_model(tab, src, bs);
    Enc<HostByteSink> e;
    e.out = HostByteSink{out, cap, 0, false};
    encode_segment(e, tab, src, bs);
    return e.out.overflow ? 0 : e.out.pos;
}

// one segment stream of the blob [blob_lo, blob_hi) into sym[0, bs); kSegOk or the reason
inline uint32_t decode_segment_host(const uint8_t* stream, uint32_t len, const uint8_t* blob_lo, const uint8_t* blob_hi, uint8_t* sym, uint32_t bs)
{
    HostTable tab;
    Dec d;
    d.in.open(stream, len, blob_lo, blob_hi);
    HostSymSink sink{sym, bs, 0};
    const uint32_t rc = decode_segment(d, tab, sink, bs);
    if (rc == kSegOk && sink.pos != bs) return kSegOverflow;
    return rc;
}

inline uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void put_u32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// Validates the front of a plane blob (its header and index; `have` bytes of the blob's `len` are at `blob`, at least the
// header and the index if the blob is well formed) for a plane of n symbols.  nullptr, or what is wrong with it.  On success
// *seg and *nseg are the header's.  Nothing is read beyond `have`.
static const char kIndexNotAvailable[] = "segmented plane: index not available";
// *brick: 0 for a WRS1 blob, the brick edge of a WRS2 blob (refused unless it is one of 8, 16, 32, 64).
inline const char* check_index(const uint8_t* blob, size_t have, size_t len, size_t n, uint32_t* seg, uint32_t* nseg, uint32_t* brick)
{
    if (have > len) have = len;
    if (have < kHeaderBytes) return "segmented plane: shorter than its header";
    const bool blocked = memcmp(blob, kMagicBlocked, 4) == 0;
    if (!blocked && memcmp(blob, kMagic, 4) != 0) return "segmented plane: wrong magic (neither a WRS1 nor a WRS2 stream)";
    const size_t head = blocked ? kHeaderBytesBlocked : kHeaderBytes;
    if (have < head) return "segmented plane: shorter than its header";
    const uint32_t s = get_u32(blob + 4), k = get_u32(blob + 8), b = blocked ? get_u32(blob + 12) : 0;
    if (!seg_ok(s)) return "segmented plane: segment length out of range";
    if (blocked && !brick_ok(b)) return "segmented plane: brick edge is not one of 8, 16, 32, 64";
    if ((size_t)k != seg_count(n, s)) return "segmented plane: segment count does not match the plane";
    if ((len - head) / 4 < k) return "segmented plane: index longer than the blob";
    if (have < head + 4 * (size_t)k) return kIndexNotAvailable;
    size_t sum = 0;
    const uint32_t bound = stream_bound(s);
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t l = get_u32(blob + head + 4 * (size_t)j);
        if (l > bound) return "segmented plane: a segment is longer than a segment can be";
        sum += l;
    }
    if (sum != len - head - 4 * (size_t)k) return "segmented plane: segment lengths do not add up to the blob";
    *seg = s; *nseg = k; *brick = b;
    return nullptr;
}

// ---- "WRS3": stranded segments -- short coder chains that share one model -------------------------------------------------
// The two roles of a segment are separated.  The MODEL stays per segment (one table of 256 counts over its bs <= seg symbols);
// the CHAIN is cut: the segment's symbols are coded as K independent strands, each a complete coder run over a contiguous piece
// of L = 16 * ceil(seg / (16 K)) symbols (the last non-empty one shorter), every one with the segment's table.
//   plane blob := 'W','R','S','3' | u32 seg | u32 nseg | u32 brick | u32 strands | u32 len[nseg] | the segment records, in order
//   record k   := u32 tlen | u32 slen[K] | T | S_0 | ... | S_{Kk-1} | 0-3 zero bytes up to a multiple of 4
//   T          := start(); shift16(count_s), s = 0..255; finish()                             (tlen bytes)
//   S_j        := start(); freq(count, cum, bs) per symbol of strand j; freq(1, 0, 2); finish()   (slen[j] bytes; 0 for j >= Kk)
// with Kk = ceil(bs / L) and len[k] the record's length including the padding.  brick: 0 for the natural symbol order, or the
// brick edge of the blocked order (wr_blocked.h).
//
// Bounds.  A strand coded with the segment's table is NOT bounded by stream_bound: a symbol that is rare in the segment costs
// up to log2(bs) bits wherever it stands.  From the coder step (Enc::freq): renorm() leaves range R > 2^23, and tot = bs <
// 2^16, so r = floor(R / tot) >= 2^7 and hence r >= (R / tot) * 128 / 129.  The new range is r * sy >= r, or in the last
// symbol's branch R - r * lt >= r * (tot - lt) = r * sy >= r.  One step therefore shrinks the range by a factor of at most
// tot * 129 / 128, i.e. by fewer than log2(59999 * 129 / 128) = 15.884 < 16 bits; the flag step (tot = 2, r >= 2^22) by
// fewer than 1.001 bits.  Every iteration of renorm() widens the range by exactly 8 bits and the range never exceeds 2^31, its
// value at start(), so over a run of m symbols and the flag the N iterations (finish()'s included) satisfy
// 8 N <= sum of the shrinks < 16 m + 1.001, hence N <= 2 m.  The run's bytes are the start byte, one byte per iteration
// and the four bytes finish() adds: at most 2 m + 5.  (That the held-byte form puts them later changes nothing: finish()
// flushes what is held.)  strand_bound rounds this up to a multiple of 4.  The same argument for T -- 256 steps of
// exactly-16-bit shifts, r = R >> 16 >= 2^7, each shrinking by fewer than 16.012 bits -- gives 8 N < 4099, N <= 512 and
// at most 517 bytes: kModelBound.  The adversary is real: a strand uniform over 255 symbols that the rest of the segment
// never uses costs 8 + log2 K bits per symbol, 13 at K = 32, where stream_bound allows for 8.25.
constexpr size_t kHeaderBytesStrands = 20;  // magic, seg, nseg, brick, strands
constexpr uint8_t kMagicStrands[4] = {'W', 'R', 'S', '3'};
constexpr uint32_t kStrandsDefault = 8, kStrandsMax = 32, kModelBound = 520;
WRSEG_HD bool strands_ok(uint32_t K, uint32_t seg) { return K >= 1 && K <= kStrandsMax && (K & (K - 1)) == 0 && 16 * K <= seg; }
// strands == 0: a WRS1 / WRS2 blob
WRSEG_HD size_t header_bytes(uint32_t brick, uint32_t strands) { return strands ? kHeaderBytesStrands : header_bytes(brick); }
WRSEG_HD uint32_t strand_len(uint32_t seg, uint32_t K) { return 16 * ((seg + 16 * K - 1) / (16 * K)); }
WRSEG_HD uint32_t strand_bound(uint32_t m) { return 2 * m + 8; }
// what a record can take at most: the length words, T, K strands of L symbols (a multiple of 4; also the staging stride)
WRSEG_HD uint32_t record_bound(uint32_t seg, uint32_t K) { return 4 * (K + 1) + kModelBound + K * strand_bound(strand_len(seg, K)); }

// why a record was refused: bits, so that the strands' reasons can be ORed into one flag per segment (0: it decoded)
enum : uint32_t { kRecLayout = 1, kRecModel = 2, kRecFlag = 4, kRecOverflow = 8 };

// the aligned word at p (the header, the index and every record of a WRS3 blob are 4-byte aligned inside the blob; the host
// reads blobs at any address)
WRSEG_HD uint32_t load_u32(const uint8_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t*>(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

// tab[s] += the number of times s occurs among the m symbols of src (plain counts)
template <class Table, class Source>
WRSEG_HD void count_symbols(Table& tab, Source& src, uint32_t m)
{
    uint32_t i = 0;
    for (; i + 16 <= m; i += 16) {
        uint32_t w[4];
        src.load16(i, w);
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 16; j++) {
            const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
            tab.set(c, tab.get(c) + 1);
        }
    }
    for (; i < m; i++) {
        const uint32_t c = src.byte(i);
        tab.set(c, tab.get(c) + 1);
    }
}

// tab: plain counts -> count << 16 | cumulative count below s (what build_model leaves)
template <class Table>
WRSEG_HD void counts_to_model(Table& tab)
{
    uint32_t cum = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t c = tab.get(s);
        tab.set(s, c << 16 | cum);
        cum += c;
    }
}

// T: the 256 counts of the model in tab, a coder run of its own; at most kModelBound bytes
template <class Table, class Sink>
WRSEG_HD void encode_model(Enc<Sink>& e, Table& tab)
{
    e.start();
    for (uint32_t s = 0; s < 256; s++) e.shift16(tab.get(s) >> 16);
    e.finish();
}

// S_j: the m >= 1 symbols of src with the model of their segment of bs symbols; at most strand_bound(m) bytes
template <class Table, class Source, class Sink>
WRSEG_HD void encode_strand(Enc<Sink>& e, Table& tab, Source& src, uint32_t m, uint32_t bs)
{
    e.start();
    uint32_t i = 0;
    for (; i + 16 <= m; i += 16) {
        uint32_t w[4];
        src.load16(i, w);
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 16; j++) {
            const uint32_t v = tab.get((w[j >> 2] >> (8 * (j & 3))) & 0xff);
            e.freq(v >> 16, v & 0xffff, bs);
        }
    }
    for (; i < m; i++) {
        const uint32_t v = tab.get(src.byte(i));
        e.freq(v >> 16, v & 0xffff, bs);
    }
    e.freq(1, 0, 2);  // the zero flag
    e.finish();
}

// The length words of the record [rec, rec + rlen) of a segment of bs symbols cut into K strands of L, checked before
// anything is decoded.  0, or kRecLayout.  On success T is the tlen bytes at rec + 4 (K + 1), strand j the s_len bytes at
// rec + s_off, and everything lies inside the record.
WRSEG_HD uint32_t check_record(const uint8_t* rec, size_t rlen, uint32_t K, uint32_t L, uint32_t bs, uint32_t j, uint32_t* tlen, uint32_t* s_off,
                               uint32_t* s_len)
{
    if (rlen < 4 * (size_t)(K + 1) || (rlen & 3)) return kRecLayout;
    const uint32_t t = load_u32(rec);
    if (t > kModelBound) return kRecLayout;
    const uint32_t Kk = (bs + L - 1) / L, bound = strand_bound(L);
    uint32_t sum = 4 * (K + 1) + t;  // (at most 132 + 520 + 32 * strand_bound(L): no overflow)
    *s_off = 0; *s_len = 0;
    for (uint32_t i = 0; i < K; i++) {
        const uint32_t l = load_u32(rec + 4 * (size_t)(i + 1));
        if (l > bound || (i >= Kk && l)) return kRecLayout;
        if (i == j) { *s_off = sum; *s_len = l; }
        sum += l;
    }
    if (((sum + 3) & ~3u) != rlen) return kRecLayout;
    *tlen = t;
    return 0;
}

// T -> tab, the model of a segment of bs symbols.  0, or kRecModel (the counts do not sum to bs); 257 coder steps.
template <class Table>
WRSEG_HD uint32_t decode_model(Dec& d, Table& tab, uint32_t bs)
{
    d.start();
    uint32_t sum = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t c = d.culshift16() & 0xffffu;
        d.update(1, c, 1u << 16);
        tab.set(s, c);
        sum += c;
    }
    if (sum != bs || bs == 0) return kRecModel;
    counts_to_model(tab);
    return 0;
}

// S_j -> exactly m symbols through sink.put, whatever the bytes are (the reader gives zeros past the strand's end).  0, or
// kRecFlag: the run does not end with the zero flag.
template <class Table, class Sink>
WRSEG_HD uint32_t decode_strand(Dec& d, Table& tab, Sink& sink, uint32_t m, uint32_t bs)
{
    d.start();
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t cf = d.culfreq(bs);
        uint32_t s = 0;  // (decode_segment: the last s whose cumulative count is <= cf)
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
        for (uint32_t step = 128; step; step >>= 1)
            if ((tab.get(s + step) & 0xffff) <= cf) s += step;
        const uint32_t v = tab.get(s);
        d.update(v >> 16, v & 0xffff, bs);
        sink.put(s);
    }
    if (d.culfreq(2)) return kRecFlag;
    return 0;
}

// one record on the host; returns its length (a multiple of 4), 0 if it did not fit into cap bytes
inline uint32_t encode_record_host(const uint8_t* sym, uint32_t bs, uint32_t seg, uint32_t K, uint8_t* out, uint32_t cap)
{
    const uint32_t L = strand_len(seg, K), words = 4 * (K + 1);
    if (cap < words) return 0;
    HostTable tab;
    memset(tab.w, 0, sizeof tab.w);
    HostSource all{sym};
    count_symbols(tab, all, bs);
    counts_to_model(tab);
    uint32_t at = words;
    Enc<HostByteSink> e;
    e.out = HostByteSink{out + at, cap - at, 0, false};
    encode_model(e, tab);
    if (e.out.overflow) return 0;
    put_u32(out, e.out.pos);
    at += e.out.pos;
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
        uint32_t len = 0;
        if (m) {
            HostSource src{sym + s0};
            e.out = HostByteSink{out + at, cap - at, 0, false};
            encode_strand(e, tab, src, m, bs);
            if (e.out.overflow) return 0;
            len = e.out.pos;
        }
        put_u32(out + 4 * (j + 1), len);
        at += len;
    }
    const uint32_t end = (at + 3) & ~3u;
    if (end > cap) return 0;
    for (; at < end; at++) out[at] = 0;
    return end;
}

// the record [rec, rec + rlen) of the blob [blob_lo, blob_hi) into sym[0, bs); 0 or the ORed reasons
inline uint32_t decode_record_host(const uint8_t* rec, size_t rlen, const uint8_t* blob_lo, const uint8_t* blob_hi, uint8_t* sym, uint32_t bs,
                                   uint32_t seg, uint32_t K)
{
    const uint32_t L = strand_len(seg, K);
    uint32_t tlen = 0, off = 0, len = 0;
    if (const uint32_t why = check_record(rec, rlen, K, L, bs, 0, &tlen, &off, &len)) return why;
    HostTable tab;
    Dec d;
    d.in.open(rec + 4 * (size_t)(K + 1), tlen, blob_lo, blob_hi);
    if (const uint32_t why = decode_model(d, tab, bs)) return why;
    uint32_t why = 0;
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t s0 = j * L, m = s0 < bs ? (bs - s0 < L ? bs - s0 : L) : 0;
        if (!m) break;
        (void)check_record(rec, rlen, K, L, bs, j, &tlen, &off, &len);
        d.in.open(rec + off, len, blob_lo, blob_hi);
        HostSymSink sink{sym + s0, m, 0};
        why |= decode_strand(d, tab, sink, m, bs);
        if (sink.pos != m) why |= kRecOverflow;
    }
    return why;
}

// check_index for the three formats.  *strands: 0 for a WRS1 / WRS2 blob, K of a WRS3 blob (whose *brick may be 0: the
// natural order).  A WRS3 record is refused here when its length is no multiple of 4 or above record_bound.
inline const char* check_index(const uint8_t* blob, size_t have, size_t len, size_t n, uint32_t* seg, uint32_t* nseg, uint32_t* brick,
                               uint32_t* strands)
{
    const size_t got = have > len ? len : have;
    if (got < 4 || memcmp(blob, kMagicStrands, 4) != 0) {  // (an unknown magic keeps the message it always had)
        *strands = 0;
        return check_index(blob, have, len, n, seg, nseg, brick);
    }
    have = got;
    const size_t head = kHeaderBytesStrands;
    if (have < head) return "segmented plane: shorter than its header";
    const uint32_t s = get_u32(blob + 4), k = get_u32(blob + 8), b = get_u32(blob + 12), K = get_u32(blob + 16);
    if (!seg_ok(s)) return "segmented plane: segment length out of range";
    if (b && !brick_ok(b)) return "segmented plane: brick edge is not one of 0, 8, 16, 32, 64";
    if (!strands_ok(K, s)) return "segmented plane: strand count is not one of 1, 2, 4, 8, 16, 32 with 16 strands <= segment length";
    if ((size_t)k != seg_count(n, s)) return "segmented plane: segment count does not match the plane";
    if ((len - head) / 4 < k) return "segmented plane: index longer than the blob";
    if (have < head + 4 * (size_t)k) return kIndexNotAvailable;
    size_t sum = 0;
    const uint32_t bound = record_bound(s, K);
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t l = get_u32(blob + head + 4 * (size_t)j);
        if (l > bound) return "segmented plane: a segment is longer than a segment can be";
        if (l & 3) return "segmented plane: a segment record is not a multiple of 4 bytes";
        sum += l;
    }
    if (sum != len - head - 4 * (size_t)k) return "segmented plane: segment lengths do not add up to the blob";
    *seg = s; *nseg = k; *brick = b; *strands = K;
    return nullptr;
}

// the same for a caller that reads WRS1 only
inline const char* check_index(const uint8_t* blob, size_t have, size_t len, size_t n, uint32_t* seg, uint32_t* nseg)
{
    if ((have > len ? len : have) < kHeaderBytes) return "segmented plane: shorter than its header";
    if (memcmp(blob, kMagic, 4) != 0) return "segmented plane: wrong magic (not a WRS1 stream)";
    uint32_t brick = 0;
    return check_index(blob, have, len, n, seg, nseg, &brick);
}

}  // namespace wrseg
