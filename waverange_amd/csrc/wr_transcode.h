// wr_transcode.h -- a coded field from one stream format to another on its planes, on the calling thread: the definition of
// wr_transcode_host (include/waverange_amd.h), and what it is made of -- the normalisation of a target format, the
// containers of the three segmented formats around wr_segcoder.h's segment and record coders, the consistency of a segmented
// stream's planes.  Host only, no HIP, no context: wr_coder_hooks.cpp puts it behind the C ABI, wr_codec.cpp takes its
// validation for the device driver (so both make the same refusals in the same order), wr_dropin.cpp its normalisation, and
// tests/native/transcode_fuzz.cpp compiles it with g++ under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/waverange_amd.h"
#include "wr_blocked.h"
#include "wr_rangecoder.h"
#include "wr_segcoder.h"

namespace wrtc {

// ---- a stream format and its parameters
struct StreamFormat {
    int format = WR_FORMAT_REF;
    unsigned seg = 0, brick = 0, strands = 0;
};

constexpr const char* kFormatNames[4] = {"ref", "wrs1", "wrs2", "wrs3"};

// Fills in the defaults of the format and refuses what its encoder would refuse (and, for the reference's stream and for
// WRS1, parameters the format does not have).  The message starts with the offending value as "key=value".
inline bool format_normalise(StreamFormat* f, std::string* why)
{
    if (f->format < WR_FORMAT_REF || f->format > WR_FORMAT_WRS3) { *why = "format " + std::to_string(f->format) + " is not one of WR_FORMAT_REF .. WR_FORMAT_WRS3"; return false; }
    const char* name = kFormatNames[f->format];
    if (f->format == WR_FORMAT_REF) {
        if (f->seg || f->brick || f->strands) { *why = std::string(name) + " takes no seg, brick or strands"; return false; }
        return true;
    }
    if (!f->seg) f->seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(f->seg)) { *why = "seg=" + std::to_string(f->seg) + ": segment length must be a multiple of 16 in [16, 59999]"; return false; }
    if (f->format == WR_FORMAT_WRS1 && f->brick) { *why = "brick=" + std::to_string(f->brick) + ": wrs1 has no brick"; return false; }
    if (f->format == WR_FORMAT_WRS2 && !f->brick) f->brick = WR_BRICK_DEFAULT;
    if (f->brick && !wrblk::brick_ok(f->brick)) { *why = "brick=" + std::to_string(f->brick) + ": brick edge must be one of 8, 16, 32, 64"; return false; }
    if (f->format != WR_FORMAT_WRS3) {
        if (f->strands) { *why = "strands=" + std::to_string(f->strands) + ": only wrs3 has strands"; return false; }
        return true;
    }
    if (!f->strands) f->strands = WR_STRANDS_DEFAULT;
    if (!wrseg::strands_ok(f->strands, f->seg)) { *why = "strands=" + std::to_string(f->strands) + ": strands must be one of 1, 2, 4, 8, 16, 32 with 16 * strands <= seg"; return false; }
    return true;
}

// WR_FORMAT_* of a coded field's first bytes, -1: neither (wr_stream_sniff)
inline int sniff(const unsigned char* data, size_t len)
{
    if (!data || !len) return -1;
    if (len >= 4 && data[0] == 'W' && data[1] == 'R' && data[2] == 'S' && data[3] >= '1' && data[3] <= '3') return data[3] - '0';
    return data[0] == 0 ? WR_FORMAT_REF : -1;  // every plane of a reference stream starts with byte 0 (rangecod.c: start_encoding)
}

// worst-case bytes of one plane of n symbols in a normalised format
inline size_t plane_bound(size_t n, const StreamFormat& f)
{
    if (f.format == WR_FORMAT_REF) return wrrc::encode_bound(n);
    const size_t nseg = wrseg::seg_count(n, f.seg);
    if (f.format == WR_FORMAT_WRS3) return wrseg::kHeaderBytesStrands + nseg * (4 + (size_t)wrseg::record_bound(f.seg, f.strands));
    return wrseg::header_bytes(f.brick) + nseg * (4 + (size_t)wrseg::stream_bound(f.seg));
}

// ---- the containers of the segmented formats on the calling thread.  A failure sets *code (WR_ERR_*) and *why.
// WRS1 (brick == 0) or WRS2 around the symbols as they stand (the caller has permuted them); returns the blob's length, 0: failed
inline size_t seg_encode_ref(const unsigned char* sym, size_t n, unsigned seg, unsigned brick, unsigned char* blob, int* code, std::string* why)
{
    const size_t nseg = wrseg::seg_count(n, seg), head = wrseg::header_bytes(brick);
    if (nseg > 0xffffffffu) { *code = WR_ERR_ARG; *why = "too many segments"; return 0; }
    memcpy(blob, brick ? wrseg::kMagicBlocked : wrseg::kMagic, 4);
    wrseg::put_u32(blob + 4, seg);
    wrseg::put_u32(blob + 8, (uint32_t)nseg);
    if (brick) wrseg::put_u32(blob + 12, brick);
    size_t at = head + 4 * nseg;
    for (size_t k = 0; k < nseg; k++) {
        const size_t base = k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        const uint32_t len = wrseg::encode_segment_host(sym + base, bs, blob + at, wrseg::stream_bound(seg));
        if (!len) { *code = WR_ERR_OVERFLOW; *why = "internal: a segment outgrew the segment bound"; return 0; }
        wrseg::put_u32(blob + head + 4 * k, len);
        at += len;
    }
    return at;
}

// the symbols of a blob that check_index has passed, in the order they were coded in
inline int seg_decode_ref(const unsigned char* blob, size_t len, unsigned char* sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t brick, std::string* why)
{
    const size_t head = wrseg::header_bytes(brick);
    size_t at = head + 4 * (size_t)nseg;
    for (uint32_t k = 0; k < nseg; k++) {
        const size_t base = (size_t)k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        const uint32_t l = wrseg::get_u32(blob + head + 4 * (size_t)k);
        if (wrseg::decode_segment_host(blob + at, l, blob, blob + len, sym + base, bs) != wrseg::kSegOk) {
            *why = "segmented plane: segment " + std::to_string(k) + " does not decode to its symbols";
            return WR_ERR_STREAM;
        }
        at += l;
    }
    return WR_OK;
}

// the WRS3 container around the symbols as they stand (the caller has permuted them if brick != 0)
inline size_t strands_encode_ref(const unsigned char* sym, size_t n, unsigned seg, unsigned brick, unsigned K, unsigned char* blob, int* code, std::string* why)
{
    const size_t nseg = wrseg::seg_count(n, seg), head = wrseg::kHeaderBytesStrands;
    if (nseg > 0xffffffffu) { *code = WR_ERR_ARG; *why = "too many segments"; return 0; }
    memcpy(blob, wrseg::kMagicStrands, 4);
    wrseg::put_u32(blob + 4, seg);
    wrseg::put_u32(blob + 8, (uint32_t)nseg);
    wrseg::put_u32(blob + 12, brick);
    wrseg::put_u32(blob + 16, K);
    size_t at = head + 4 * nseg;
    for (size_t k = 0; k < nseg; k++) {
        const size_t base = k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        const uint32_t len = wrseg::encode_record_host(sym + base, bs, seg, K, blob + at, wrseg::record_bound(seg, K));
        if (!len) { *code = WR_ERR_OVERFLOW; *why = "internal: a record outgrew the record bound"; return 0; }
        wrseg::put_u32(blob + head + 4 * k, len);
        at += len;
    }
    return at;
}

inline int strands_decode_ref(const unsigned char* blob, size_t len, unsigned char* sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t K, std::string* why)
{
    const size_t head = wrseg::kHeaderBytesStrands;
    size_t at = head + 4 * (size_t)nseg;
    for (uint32_t k = 0; k < nseg; k++) {
        const size_t base = (size_t)k * seg;
        const uint32_t bs = n - base < seg ? (uint32_t)(n - base) : seg;
        const uint32_t l = wrseg::get_u32(blob + head + 4 * (size_t)k);
        if (wrseg::decode_record_host(blob + at, l, blob, blob + len, sym + base, bs, seg, K)) {
            *why = "segmented plane: segment " + std::to_string(k) + " does not decode to its symbols";
            return WR_ERR_STREAM;
        }
        at += l;
    }
    return WR_OK;
}

// Every plane's header and index of a segmented stream: *brick is 0 for a WRS1 stream, the brick edge of a WRS2 stream;
// *strands 0, or the strand count of a WRS3 stream (whose brick may be 0).  A stream whose planes differ in format, brick or
// strand count is refused.  false: *why, prefixed with the plane.
inline bool check_planes(const unsigned char* data_enc, const size_t* off, const wr_enc_info* info, int nlay, size_t n, uint32_t* seg, uint32_t* nseg,
                         uint32_t* brick, uint32_t* strands, std::string* why)
{
    *brick = 0; *strands = 0;
    for (int l = 0; l < nlay; l++) {
        uint32_t b = 0, K = 0;
        const char* w = wrseg::check_index(data_enc + off[l], info->len_enc_vec[l], info->len_enc_vec[l], n, &seg[l], &nseg[l], &b, &K);
        if (w) {}
        else if (l == 0) { *brick = b; *strands = K; }
        else if (K != *strands) w = "the planes of the stream differ in format or in their strand count";
        else if ((b != 0) != (*brick != 0)) w = "the stream mixes WRS1 and WRS2 planes";
        else if (b != *brick) w = "the planes of the stream differ in their brick edge";
        if (w) { *why = "plane " + std::to_string(l) + ": " + w; return false; }
    }
    return true;
}

// ---- the transcode
// What both forms of wr_transcode_host check before a symbol is decoded, in this order; the outputs describe the source.
struct Source {
    StreamFormat target;   // normalised
    bool trivial = false;  // ntot_enc == 0: the header passes through, nothing else is looked at
    size_t n = 0;
    int nlay = 0;
    int format = WR_FORMAT_REF;
    size_t off[WR_NLAYMAX + 1] = {0};
    uint32_t seg[WR_NLAYMAX] = {0}, nseg[WR_NLAYMAX] = {0}, brick = 0, strands = 0;  // a segmented source
};

inline int validate(int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg,
                    unsigned brick, unsigned strands, const wr_enc_info* info_out, const unsigned char* data_out, size_t cap, Source* s, std::string* why)
{
    if (!info_in || !info_out) { *why = "null wr_enc_info"; return WR_ERR_ARG; }
    if (nx < 1 || ny < 1 || nz < 1) { *why = "non-positive dimension"; return WR_ERR_ARG; }
    s->target.format = format; s->target.seg = seg; s->target.brick = brick; s->target.strands = strands;
    std::string detail;
    if (!format_normalise(&s->target, &detail)) { *why = "target format: " + detail; return WR_ERR_ARG; }
    s->n = (size_t)nx * ny * nz;
    if (s->target.format != WR_FORMAT_REF && wrseg::seg_count(s->n, s->target.seg) > 0xffffffffu) { *why = "too many segments"; return WR_ERR_ARG; }
    if (info_in->ntot_enc == 0) { s->trivial = true; return WR_OK; }  // wrappers.cpp:462-469
    s->nlay = info_in->nlay;
    if (s->nlay < 1 || s->nlay > WR_NLAYMAX) { *why = "nlay out of range"; return WR_ERR_ARG; }
    if (info_in->wlev != 0 && info_in->wlev != 4) { *why = "wlev must be 0 or 4"; return WR_ERR_ARG; }
    if (!data_in || !data_out) { *why = "null coded buffer"; return WR_ERR_ARG; }
    {
        const size_t have = len_in ? len_in : (size_t)info_in->ntot_enc;
        const uintptr_t a0 = (uintptr_t)data_in, a1 = a0 + have, b0 = (uintptr_t)data_out, b1 = b0 + cap;
        if (a0 < b1 && b0 < a1) { *why = "the output buffer overlaps the coded input"; return WR_ERR_ARG; }
    }
    for (int l = 0; l < s->nlay; l++) {
        s->off[l + 1] = s->off[l] + info_in->len_enc_vec[l];
        if (s->off[l + 1] < s->off[l]) { *why = "len_enc_vec exceeds ntot_enc"; return WR_ERR_STREAM; }
    }
    if (s->off[s->nlay] > info_in->ntot_enc) { *why = "len_enc_vec exceeds ntot_enc"; return WR_ERR_STREAM; }
    if (len_in && info_in->ntot_enc > len_in) { *why = "ntot_enc exceeds the length of the coded buffer"; return WR_ERR_STREAM; }
    s->format = sniff(data_in, info_in->len_enc_vec[0]);
    if (s->format < 0) { *why = "plane 0: neither a reference stream nor a segmented one"; return WR_ERR_STREAM; }
    if (s->format == WR_FORMAT_REF) {
        for (int l = 1; l < s->nlay; l++)
            if (sniff(data_in + s->off[l], info_in->len_enc_vec[l]) != WR_FORMAT_REF) { *why = "plane " + std::to_string(l) + ": the planes of the stream differ in format"; return WR_ERR_STREAM; }
        return WR_OK;
    }
    if (!check_planes(data_in, s->off, info_in, s->nlay, s->n, s->seg, s->nseg, &s->brick, &s->strands, why)) return WR_ERR_STREAM;
    return WR_OK;
}

// the header of the result: info_in with the lengths of the new planes
inline void finish_info(const wr_enc_info& in, const size_t* lens, int nlay, wr_enc_info* out)
{
    wr_enc_info r = in;
    r.ntot_enc = 0;
    for (int l = 0; l < WR_NLAYMAX; l++) r.len_enc_vec[l] = 0;
    for (int l = 0; l < nlay; l++) { r.len_enc_vec[l] = lens[l]; r.ntot_enc += lens[l]; }
    *out = r;
}

constexpr const char* kTooLarge = "Error: encoded array is too large. Use larger SAFETY_BUFFER_FACTOR";

// wr_transcode_host_ref: decode every plane with the source format's host decoder, code it with the target's host encoder.
// The planes are coded one at a time into a buffer of the plane's bound; data_out receives only what fits under cap.
inline int transcode_ref(int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg,
                         unsigned brick, unsigned strands, wr_enc_info* info_out, unsigned char* data_out, size_t cap, std::string* why)
{
    Source s;
    if (int rc = validate(nx, ny, nz, info_in, data_in, len_in, format, seg, brick, strands, info_out, data_out, cap, &s, why)) return rc;
    if (s.trivial) { const wr_enc_info keep = *info_in; *info_out = keep; return WR_OK; }
    const size_t n = s.n;
    const int wlev = (int)info_in->wlev;
    const StreamFormat& t = s.target;
    // ---- the planes, in natural order
    std::vector<std::vector<unsigned char>> planes((size_t)s.nlay);
    std::vector<unsigned char> perm;
    for (int l = 0; l < s.nlay; l++) {
        const unsigned char* const src = data_in + s.off[l];
        const size_t len = info_in->len_enc_vec[l];
        const std::string plane = "plane " + std::to_string(l) + ": ";
        planes[l].resize(n);
        if (s.format == WR_FORMAT_REF) {
            if (wrrc::decode_plane(src, len, planes[l].data(), n) != n) { *why = plane + "stream does not decode to nx*ny*nz symbols"; return WR_ERR_STREAM; }
            continue;
        }
        unsigned char* const dst = s.brick ? (perm.resize(n), perm.data()) : planes[l].data();
        std::string w;
        const int rc = s.strands ? strands_decode_ref(src, len, dst, n, s.seg[l], s.nseg[l], s.strands, &w) : seg_decode_ref(src, len, dst, n, s.seg[l], s.nseg[l], s.brick, &w);
        if (rc) { *why = plane + w; return rc; }
        if (s.brick) wrblk::reorder_host(wrblk::order_of(nx, ny, nz, wlev, s.brick), perm.data(), planes[l].data(), true);
    }
    // ---- the target's streams
    size_t lens[WR_NLAYMAX] = {0}, total = 0;
    std::vector<unsigned char> out(plane_bound(n, t));
    for (int l = 0; l < s.nlay; l++) {
        const unsigned char* sym = planes[l].data();
        if (t.format != WR_FORMAT_REF && t.brick) {
            perm.resize(n);
            wrblk::reorder_host(wrblk::order_of(nx, ny, nz, wlev, t.brick), sym, perm.data(), false);
            sym = perm.data();
        }
        int code = WR_OK;
        std::string w;
        if (t.format == WR_FORMAT_REF) lens[l] = wrrc::encode_plane(sym, n, out.data(), nullptr);
        else if (t.format == WR_FORMAT_WRS3) lens[l] = strands_encode_ref(sym, n, t.seg, t.brick, t.strands, out.data(), &code, &w);
        else lens[l] = seg_encode_ref(sym, n, t.seg, t.brick, out.data(), &code, &w);
        if (code) { *why = "plane " + std::to_string(l) + ": " + w; return code; }
        if (total <= cap && lens[l] <= cap - total) memcpy(data_out + total, out.data(), lens[l]);
        total += lens[l];
        planes[l] = std::vector<unsigned char>();
    }
    if (total > cap) { *why = kTooLarge; return WR_ERR_OVERFLOW; }
    finish_info(*info_in, lens, s.nlay, info_out);
    return WR_OK;
}

}  // namespace wrtc
