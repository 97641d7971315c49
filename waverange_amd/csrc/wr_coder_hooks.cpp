// wr_coder_hooks.cpp -- the host range coder alone behind the C ABI (rows a6/a7/a10 of SURVEY.md 8a): whole planes,
// interleaved planes, the coder pool, the 16-lane loops, and the windowed symbol path with host buffers standing in for
// device-resident planes (test hooks).
#include "wr_blocked.h"
#include "wr_budget.h"
#include "wr_internal.h"
#include "wr_lowres.h"
#include "wr_mask.h"
#include "wr_roi.h"
#include "wr_segcoder.h"
#include "wr_transcode.h"

using namespace wri;

extern "C" {

size_t wr_range_encode_bound(size_t n) { return wrrc::encode_bound(n); }
size_t wr_range_encode_bound_hist(const unsigned short* hists, size_t n) { return wrrc::encode_bound_hist(hists, n); }
size_t wr_range_encode(const unsigned char* sym, size_t n, unsigned char* out) { return wrrc::encode_plane(sym, n, out, nullptr); }
size_t wr_range_decode(const unsigned char* in, size_t len, unsigned char* sym, size_t n) { return wrrc::decode_plane(in, len, sym, n); }
void wr_range_encode_multi(int count, const unsigned char* const* sym, size_t n, unsigned char* const* out, size_t* lens)
{
    wrrc::encode_planes(count, sym, n, out, nullptr, lens);
}
void wr_range_decode_multi(int count, const unsigned char* const* in, const size_t* len, unsigned char* const* sym, size_t n, size_t* produced)
{
    wrrc::decode_planes(count, in, len, sym, n, produced);
}

int wr_range_decode_vec(int count, const unsigned char* const* in, const size_t* len, unsigned char* const* sym, const size_t* n,
                        size_t* produced)
{
    if (!wrrc::decode_planes_vec(count, in, len, sym, n, produced)) return fail(WR_ERR_UNSUPPORTED, "this CPU has no AVX-512");
    return WR_OK;
}

int wr_range_encode_vec(int count, const unsigned char* const* sym, const size_t* n, unsigned char* const* out, size_t* lens)
{
    if (!wrrc::encode_planes_vec(count, sym, n, out, lens)) return fail(WR_ERR_UNSUPPORTED, "this CPU has no AVX-512");
    return WR_OK;
}

int wr_range_encode_pool(int count, const unsigned char* const* sym, const size_t* n, unsigned char* const* out, size_t* lens)
{
    if (wrrc::pool_threads() < 1) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    if (count < 1) return WR_OK;
    std::vector<wrrc::PlaneJob> jobs((size_t)count);
    for (int k = 0; k < count; k++) { jobs[k].kind = wrrc::PlaneJob::kEncode; jobs[k].src = sym[k]; jobs[k].n = n[k]; jobs[k].dst = out[k]; }
    if (!wrrc::pool_run(jobs.data(), count)) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    for (int k = 0; k < count; k++) lens[k] = jobs[k].result;
    return WR_OK;
}

int wr_range_decode_pool(int count, const unsigned char* const* in, const size_t* len, unsigned char* const* sym, const size_t* n,
                         size_t* produced)
{
    if (wrrc::pool_threads() < 1) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    if (count < 1) return WR_OK;
    std::vector<wrrc::PlaneJob> jobs((size_t)count);
    for (int k = 0; k < count; k++) {
        jobs[k].kind = wrrc::PlaneJob::kDecode; jobs[k].src = in[k]; jobs[k].src_len = len[k]; jobs[k].dst = sym[k]; jobs[k].n = n[k];
    }
    if (!wrrc::pool_run(jobs.data(), count)) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    for (int k = 0; k < count; k++) produced[k] = jobs[k].result;
    return WR_OK;
}

namespace {
// memory-backed PlaneWindow for the windowed test hooks: the symbol side passes through two alternating buffers of
// `chunk` symbols, as a device-resident plane does through its pinned ring; the buffer not in use is poisoned
struct MemWindow {
    const uint8_t* plane = nullptr;  // encode: source plane
    uint8_t* out = nullptr;          // decode: destination plane
    size_t n = 0, chunk = 0;
    std::vector<uint8_t> buf[2];
    int cur = 1;
    size_t last_first = 0, last_count = 0;
    wrrc::PlaneWindow io;
    static uint8_t* enc_window(void* user, size_t first, size_t* count)
    {
        MemWindow* w = static_cast<MemWindow*>(user);
        const size_t c = *count < w->chunk ? *count : w->chunk;
        memset(w->buf[w->cur].data(), 0xA5, w->buf[w->cur].size());  // the window handed out before is dead now
        w->cur ^= 1;
        memcpy(w->buf[w->cur].data(), w->plane + first, c);
        *count = c;
        return w->buf[w->cur].data();
    }
    static uint8_t* dec_window(void* user, size_t first, size_t* count)
    {
        MemWindow* w = static_cast<MemWindow*>(user);
        if (w->last_count) memcpy(w->out + w->last_first, w->buf[w->cur].data(), w->last_count);  // the previous window is complete
        w->last_count = 0;
        if (*count == 0) return nullptr;
        const size_t c = *count < w->chunk ? *count : w->chunk;
        w->cur ^= 1;
        memset(w->buf[w->cur].data(), 0x5A, w->buf[w->cur].size());
        w->last_first = first; w->last_count = c;
        *count = c;
        return w->buf[w->cur].data();
    }
    void init(size_t n_, size_t chunk_, bool decode)
    {
        n = n_; chunk = chunk_;
        buf[0].assign(chunk, 0); buf[1].assign(chunk, 0);
        io.window = decode ? dec_window : enc_window;
        io.user = this;
    }
};
}  // namespace

int wr_range_encode_windowed(int mode, int count, const unsigned char* const* sym, size_t n, size_t chunk, unsigned char* const* out, size_t* lens)
{
    if (count < 1) return WR_OK;
    if (chunk == 0 || chunk % wrrc::kBlock) return fail(WR_ERR_ARG, "the window length must be a multiple of 60000");
    std::vector<MemWindow> w((size_t)count);
    std::vector<const wrrc::PlaneWindow*> io((size_t)count);
    std::vector<size_t> ns((size_t)count, n);
    std::vector<const unsigned char*> none((size_t)count, nullptr);
    std::vector<wrrc::PlaneJob> jobs((size_t)count);
    for (int k = 0; k < count; k++) {
        w[k].plane = sym[k]; w[k].init(n, chunk, false); io[k] = &w[k].io;
        jobs[k].kind = wrrc::PlaneJob::kEncode; jobs[k].n = n; jobs[k].dst = out[k]; jobs[k].io = io[k];
    }
    if (mode == 2) return wrrc::encode_planes_vec(count, none.data(), ns.data(), out, lens, io.data()) ? WR_OK : fail(WR_ERR_UNSUPPORTED, "this CPU has no AVX-512");
    if (mode == 0) wrrc::run_jobs(jobs.data(), count);
    else if (!wrrc::pool_run(jobs.data(), count)) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    for (int k = 0; k < count; k++) lens[k] = jobs[k].result;
    return WR_OK;
}

int wr_range_decode_windowed(int mode, int count, const unsigned char* const* in, const size_t* len, unsigned char* const* sym, size_t n,
                             size_t chunk, size_t* produced)
{
    if (count < 1) return WR_OK;
    if (chunk == 0 || chunk % wrrc::kBlock) return fail(WR_ERR_ARG, "the window length must be a multiple of 60000");
    std::vector<MemWindow> w((size_t)count);
    std::vector<const wrrc::PlaneWindow*> io((size_t)count);
    std::vector<size_t> ns((size_t)count, n);
    std::vector<unsigned char*> none((size_t)count, nullptr);
    std::vector<wrrc::PlaneJob> jobs((size_t)count);
    for (int k = 0; k < count; k++) {
        w[k].out = sym[k]; w[k].init(n, chunk, true); io[k] = &w[k].io;
        jobs[k].kind = wrrc::PlaneJob::kDecode; jobs[k].src = in[k]; jobs[k].src_len = len[k]; jobs[k].n = n; jobs[k].io = io[k];
    }
    if (mode == 2) return wrrc::decode_planes_vec(count, in, len, none.data(), ns.data(), produced, io.data()) ? WR_OK : fail(WR_ERR_UNSUPPORTED, "this CPU has no AVX-512");
    if (mode == 0) wrrc::run_jobs(jobs.data(), count);
    else if (!wrrc::pool_run(jobs.data(), count)) return fail(WR_ERR_ARG, "the coder pool is not running (wr_set_coder_pool)");
    for (int k = 0; k < count; k++) produced[k] = jobs[k].result;
    return WR_OK;
}

// ---- the segmented plane stream (wr_segcoder.h) on the calling thread: the definition of the format, for tests and for
// readers without a GPU
size_t wr_seg_bound(size_t n, unsigned seg)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) return 0;
    return wrseg::kHeaderBytes + wrseg::seg_count(n, seg) * (4 + (size_t)wrseg::stream_bound(seg));
}

// ---- an encode to a byte budget (wr_budget.h): the tolerance grid and the size bound of a plane, on the calling thread
double wr_budget_tol(int g) { return wrbud::grid_tol(g); }
int wr_budget_index(double tolrel) { return wrbud::grid_index(tolrel); }
int wr_bounded_start(double max_abs_err, double absmax) { return wrbud::bounded_start(max_abs_err, absmax); }
double wr_psnr_rms(double db, double lo, double hi) { return wrbud::psnr_rms(db, lo, hi); }

size_t wr_seg_size_bound_host_ref(const unsigned char* sym, size_t n, unsigned seg)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (n && !sym) { fail(WR_ERR_ARG, "null pointer"); return 0; }
    return wrbud::plane_bound(sym, n, seg);
}

// the containers (wr_transcode.h) with their failures made the thread's error
static size_t seg_encode_ref(const unsigned char* sym, size_t n, unsigned seg, unsigned brick, unsigned char* blob)
{
    int code = WR_OK;
    std::string why;
    const size_t len = wrtc::seg_encode_ref(sym, n, seg, brick, blob, &code, &why);
    if (!len) fail(code, why);
    return len;
}

static int seg_decode_ref(const unsigned char* blob, size_t len, unsigned char* sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t brick)
{
    std::string why;
    const int rc = wrtc::seg_decode_ref(blob, len, sym, n, seg, nseg, brick, &why);
    return rc ? fail(rc, why) : WR_OK;
}

size_t wr_seg_encode_host_ref(const unsigned char* sym, size_t n, unsigned seg, unsigned char* blob)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!blob || (n && !sym)) { fail(WR_ERR_ARG, "null pointer"); return 0; }
    return seg_encode_ref(sym, n, seg, 0, blob);
}

int wr_seg_decode_host_ref(const unsigned char* blob, size_t len, unsigned char* sym, size_t n)
{
    if (!blob || (n && !sym)) return fail(WR_ERR_ARG, "null pointer");
    uint32_t seg = 0, nseg = 0;
    if (const char* why = wrseg::check_index(blob, len, len, n, &seg, &nseg)) return fail(WR_ERR_STREAM, why);
    return seg_decode_ref(blob, len, sym, n, seg, nseg, 0);
}

// ---- the mask blob of a masked record ("WRM1", wr_mask.h) on the calling thread: the definition of the format
size_t wr_mask_bound(size_t n, unsigned seg)
{
    const size_t b = wr_seg_bound(wrmask::mask_bytes(n), seg);
    return b ? wrmask::kHeaderBytes + b : 0;
}

int wr_mask_sniff(const unsigned char* data, size_t len) { return wrmask::sniff(data, len) ? 1 : 0; }

size_t wr_mask_blob_host_ref(const unsigned char* undef_flags, size_t n, unsigned seg, double pad, unsigned char* blob)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!blob || !undef_flags || !n) { fail(WR_ERR_ARG, n ? "null pointer" : "empty field"); return 0; }
    std::vector<unsigned char> bits(wrmask::mask_bytes(n), 0);
    unsigned long long undefined = 0;
    for (size_t j = 0; j < n; j++)
        if (undef_flags[j]) { bits[j >> 3] |= (unsigned char)(1u << (j & 7)); undefined++; }
    wrmask::put_header(blob, n, undefined, pad);
    const size_t len = seg_encode_ref(bits.data(), bits.size(), seg, 0, blob + wrmask::kHeaderBytes);
    return len ? wrmask::kHeaderBytes + len : 0;
}

int wr_mask_parse_host_ref(const unsigned char* blob, size_t len, size_t n, unsigned char* undef_flags, unsigned long long* undefined, double* pad)
{
    if (!blob || !n) return fail(WR_ERR_ARG, n ? "null pointer" : "empty field");
    unsigned long long count = 0;
    double p = 0;
    if (const char* why = wrmask::check_header(blob, len, n, &count, &p)) return fail(WR_ERR_STREAM, why);
    const size_t nsym = wrmask::mask_bytes(n), rest = len - wrmask::kHeaderBytes;
    uint32_t seg = 0, nseg = 0;
    if (const char* why = wrseg::check_index(blob + wrmask::kHeaderBytes, rest, rest, nsym, &seg, &nseg)) return fail(WR_ERR_STREAM, std::string("mask blob: ") + why);
    std::vector<unsigned char> bits(nsym);
    if (int rc = seg_decode_ref(blob + wrmask::kHeaderBytes, rest, bits.data(), nsym, seg, nseg, 0)) return rc;
    if ((n & 7) && (bits[nsym - 1] >> (n & 7))) return fail(WR_ERR_STREAM, "mask blob: a bit beyond the field's last sample is set");
    unsigned long long pop = 0;
    for (size_t k = 0; k < nsym; k++) pop += (unsigned long long)__builtin_popcount(bits[k]);
    if (pop != count) return fail(WR_ERR_STREAM, "mask blob: the mask's set bits are not the count in its header");
    if (undef_flags) for (size_t j = 0; j < n; j++) undef_flags[j] = (bits[j >> 3] >> (j & 7)) & 1;
    if (undefined) *undefined = count;
    if (pad) *pad = p;
    return WR_OK;
}

// ---- the blocked symbol order (wr_blocked.h) and the WRS2 container on the calling thread
static bool blocked_args_ok(int nx, int ny, int nz, int wlev, unsigned* brick)
{
    if (!*brick) *brick = WR_BRICK_DEFAULT;
    if (nx < 1 || ny < 1 || nz < 1) { fail(WR_ERR_ARG, "non-positive dimension"); return false; }
    if (wlev != 0 && wlev != wrlow::kMaxLevel) { fail(WR_ERR_ARG, "wlev must be 0 or 4"); return false; }
    if (!wrblk::brick_ok(*brick)) { fail(WR_ERR_ARG, "brick edge must be one of 8, 16, 32, 64"); return false; }
    return true;
}

int wr_blocked_order(int nx, int ny, int nz, int wlev, unsigned brick, uint64_t* pi)
{
    if (!blocked_args_ok(nx, ny, nz, wlev, &brick)) return WR_ERR_ARG;
    if (!pi) return fail(WR_ERR_ARG, "null pointer");
    wrblk::fill_order(wrblk::order_of(nx, ny, nz, wlev, brick), pi);
    return WR_OK;
}

size_t wr_seg_bound_blocked(size_t n, unsigned seg)
{
    const size_t b = wr_seg_bound(n, seg);
    return b ? b + (wrseg::kHeaderBytesBlocked - wrseg::kHeaderBytes) : 0;
}

size_t wr_seg_encode_host_ref_blocked(const unsigned char* sym, int nx, int ny, int nz, int wlev, unsigned brick, unsigned seg, unsigned char* blob)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!blocked_args_ok(nx, ny, nz, wlev, &brick)) return 0;
    if (!blob || !sym) { fail(WR_ERR_ARG, "null pointer"); return 0; }
    const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, brick);
    std::vector<unsigned char> perm(od.n());
    wrblk::reorder_host(od, sym, perm.data(), false);
    return seg_encode_ref(perm.data(), od.n(), seg, brick, blob);
}

// ---- stranded segments ("WRS3", wr_segcoder.h) on the calling thread
size_t wr_seg_bound_strands(size_t n, unsigned seg, unsigned strands)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!strands) strands = WR_STRANDS_DEFAULT;
    if (!wrseg::seg_ok(seg) || !wrseg::strands_ok(strands, seg)) return 0;
    return wrseg::kHeaderBytesStrands + wrseg::seg_count(n, seg) * (4 + (size_t)wrseg::record_bound(seg, strands));
}

static size_t strands_encode_ref(const unsigned char* sym, size_t n, unsigned seg, unsigned brick, unsigned K, unsigned char* blob)
{
    int code = WR_OK;
    std::string why;
    const size_t len = wrtc::strands_encode_ref(sym, n, seg, brick, K, blob, &code, &why);
    if (!len) fail(code, why);
    return len;
}

static int strands_decode_ref(const unsigned char* blob, size_t len, unsigned char* sym, size_t n, uint32_t seg, uint32_t nseg, uint32_t K)
{
    std::string why;
    const int rc = wrtc::strands_decode_ref(blob, len, sym, n, seg, nseg, K, &why);
    return rc ? fail(rc, why) : WR_OK;
}

size_t wr_seg_encode_host_ref_strands(const unsigned char* sym, int nx, int ny, int nz, int wlev, unsigned brick, unsigned seg, unsigned strands,
                                      unsigned char* blob)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!strands) strands = WR_STRANDS_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!wrseg::strands_ok(strands, seg)) { fail(WR_ERR_ARG, "strands must be one of 1, 2, 4, 8, 16, 32 with 16 * strands <= seg"); return 0; }
    if (nx < 0 || ny < 0 || nz < 0) { fail(WR_ERR_ARG, "negative dimension"); return 0; }
    const size_t n = (size_t)nx * ny * nz;
    if (!blob || (n && !sym)) { fail(WR_ERR_ARG, "null pointer"); return 0; }
    if (!brick) return strands_encode_ref(sym, n, seg, 0, strands, blob);  // the natural order: the shape is only its product
    if (!blocked_args_ok(nx, ny, nz, wlev, &brick)) return 0;
    const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, brick);
    std::vector<unsigned char> perm(od.n());
    wrblk::reorder_host(od, sym, perm.data(), false);
    return strands_encode_ref(perm.data(), od.n(), seg, brick, strands, blob);
}

int wr_seg_decode_host_ref_blocked(const unsigned char* blob, size_t len, unsigned char* sym, int nx, int ny, int nz, int wlev)
{
    unsigned any = WR_BRICK_DEFAULT;
    if (!blocked_args_ok(nx, ny, nz, wlev, &any)) return WR_ERR_ARG;
    if (!blob || !sym) return fail(WR_ERR_ARG, "null pointer");
    const size_t n = (size_t)nx * ny * nz;
    uint32_t seg = 0, nseg = 0, brick = 0, strands = 0;
    if (const char* why = wrseg::check_index(blob, len, len, n, &seg, &nseg, &brick, &strands)) return fail(WR_ERR_STREAM, why);
    if (strands) {
        if (!brick) return strands_decode_ref(blob, len, sym, n, seg, nseg, strands);
        std::vector<unsigned char> perm(n);
        if (int rc = strands_decode_ref(blob, len, perm.data(), n, seg, nseg, strands)) return rc;
        wrblk::reorder_host(wrblk::order_of(nx, ny, nz, wlev, brick), perm.data(), sym, true);
        return WR_OK;
    }
    if (!brick) return seg_decode_ref(blob, len, sym, n, seg, nseg, 0);  // a WRS1 blob: the symbols are in natural order
    std::vector<unsigned char> perm(n);
    if (int rc = seg_decode_ref(blob, len, perm.data(), n, seg, nseg, brick)) return rc;
    wrblk::reorder_host(wrblk::order_of(nx, ny, nz, wlev, brick), perm.data(), sym, true);
    return WR_OK;
}

// ---- transcoding on the calling thread (wr_transcode.h): the definition of wr_transcode_host
size_t wr_transcode_bound(size_t n, int nlay, int format, unsigned seg, unsigned brick, unsigned strands)
{
    wrtc::StreamFormat f;
    f.format = format; f.seg = seg; f.brick = brick; f.strands = strands;
    std::string why;
    if (nlay < 0 || nlay > WR_NLAYMAX || !wrtc::format_normalise(&f, &why)) return 0;
    return (size_t)nlay * wrtc::plane_bound(n, f);
}

int wr_transcode_host_ref(int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg,
                          unsigned brick, unsigned strands, wr_enc_info* info_out, unsigned char* data_out, size_t cap)
{
    std::string why;
    const int rc = wrtc::transcode_ref(nx, ny, nz, info_in, data_in, len_in, format, seg, brick, strands, info_out, data_out, cap, &why);
    return rc ? fail(rc, why) : WR_OK;
}

// ---- the geometry of a low-resolution decode (wr_lowres.h): host only, no device is touched
int wr_lowres_dims(int nx, int ny, int nz, int level, int* bx, int* by, int* bz)
{
    if (nx < 1 || ny < 1 || nz < 1) return fail(WR_ERR_ARG, "non-positive dimension");
    if (!wrlow::level_ok(level)) return fail(WR_ERR_ARG, "level must be in [0, 4]");
    const wrlow::Box b = wrlow::box_of(nx, ny, nz, level);
    if (bx) *bx = b.bx;
    if (by) *by = b.by;
    if (bz) *bz = b.bz;
    return WR_OK;
}

double wr_lowres_scale(int nx, int ny, int nz, int level)
{
    if (nx < 1 || ny < 1 || nz < 1 || !wrlow::level_ok(level)) { fail(WR_ERR_ARG, "non-positive dimension or level outside [0, 4]"); return 0.0; }
    return wrlow::scale_of(wrlow::box_of(nx, ny, nz, level));
}

size_t wr_seg_lowres_segments(int nx, int ny, int nz, int level, unsigned seg, uint32_t* ids, size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (nx < 1 || ny < 1 || nz < 1 || !wrlow::level_ok(level)) { fail(WR_ERR_ARG, "non-positive dimension or level outside [0, 4]"); return 0; }
    return wrlow::segments_of(nx, ny, wrlow::box_of(nx, ny, nz, level), seg, ids, ids ? cap : 0);
}

// ---- the geometry of a region decode (wr_roi.h): host only
static bool roi_args_ok(int nx, int ny, int nz, int level, int wlev, const wr_box* roi)
{
    if (nx < 1 || ny < 1 || nz < 1 || !wrlow::level_ok(level)) { fail(WR_ERR_ARG, "non-positive dimension or level outside [0, 4]"); return false; }
    if (wlev != 0 && wlev != wrlow::kMaxLevel) { fail(WR_ERR_ARG, "wlev must be 0 or 4"); return false; }
    if (level > wlev) { fail(WR_ERR_ARG, "level exceeds the transform depth"); return false; }
    if (!roi || !wrroi::roi_ok(wrlow::box_of(nx, ny, nz, level), *roi)) { fail(WR_ERR_ARG, "the region is empty or reaches outside the box of the level"); return false; }
    return true;
}

int wr_roi_window(int nx, int ny, int nz, int level, int wlev, const wr_box* roi, wr_box* win)
{
    if (!roi_args_ok(nx, ny, nz, level, wlev, roi)) return WR_ERR_ARG;
    const wrroi::Geometry g = wrroi::geometry_of(wrlow::box_of(nx, ny, nz, level), wlev - level, *roi);
    if (win) *win = wr_box{g.ax[0].a, g.ax[1].a, g.ax[2].a, g.ax[0].b, g.ax[1].b, g.ax[2].b};
    return WR_OK;
}

size_t wr_seg_roi_segments(int nx, int ny, int nz, int level, int wlev, const wr_box* roi, unsigned seg, uint32_t* ids, size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!roi_args_ok(nx, ny, nz, level, wlev, roi)) return 0;
    return wrroi::segments_of(nx, ny, nz, wrroi::geometry_of(wrlow::box_of(nx, ny, nz, level), wlev - level, *roi), seg, ids, ids ? cap : 0);
}

// the crop of the mask of a masked record (wr_mask.h): host only
size_t wr_mask_roi_segments(int nx, int ny, int nz, int level, const wr_box* roi, unsigned seg, uint32_t* ids, size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (nx < 1 || ny < 1 || nz < 1 || !wrlow::level_ok(level)) { fail(WR_ERR_ARG, "non-positive dimension or level outside [0, 4]"); return 0; }
    const wrlow::Box b = wrlow::box_of(nx, ny, nz, level);
    const wr_box whole{0, 0, 0, b.bx, b.by, b.bz};
    if (roi && !wrroi::roi_ok(b, *roi)) { fail(WR_ERR_ARG, "the region is empty or reaches outside the box of the level"); return 0; }
    const wr_box& r = roi ? *roi : whole;
    return wrmask::roi_segments(wrmask::Region{nx, ny, nz, level, r.x0, r.y0, r.z0, r.x1, r.y1, r.z1}, seg, ids, ids ? cap : 0);
}

size_t wr_seg_lowres_segments_blocked(int nx, int ny, int nz, int level, int wlev, unsigned brick, unsigned seg, uint32_t* ids, size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!blocked_args_ok(nx, ny, nz, wlev, &brick)) return 0;
    if (!wrlow::level_ok(level) || level > wlev) { fail(WR_ERR_ARG, "level outside [0, wlev]"); return 0; }
    return wrblk::lowres_segments(nx, ny, nz, level, seg, ids, ids ? cap : 0);
}

size_t wr_seg_roi_segments_blocked(int nx, int ny, int nz, int level, int wlev, const wr_box* roi, unsigned brick, unsigned seg, uint32_t* ids,
                                   size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!blocked_args_ok(nx, ny, nz, wlev, &brick)) return 0;
    if (!roi_args_ok(nx, ny, nz, level, wlev, roi)) return 0;
    return wrblk::region_segments(wrblk::order_of(nx, ny, nz, wlev, brick), wrroi::geometry_of(wrlow::box_of(nx, ny, nz, level), wlev - level, *roi),
                                  seg, ids, ids ? cap : 0);
}

// ---- the geometry of a region decode over several regions (include/waverange_amd.h, "many regions per call"): host only
static bool roi_multi_args_ok(int nx, int ny, int nz, int level, int wlev, const wr_box* rois, int nroi)
{
    if (nroi < 1 || nroi > WR_ROI_MULTI_MAX) { fail(WR_ERR_ARG, "nroi must be in 1.." + std::to_string(WR_ROI_MULTI_MAX)); return false; }
    if (!rois) { fail(WR_ERR_ARG, "null region array"); return false; }
    for (int i = 0; i < nroi; i++)
        if (!roi_args_ok(nx, ny, nz, level, wlev, &rois[i])) { fail(WR_ERR_ARG, "region " + std::to_string(i) + ": " + wr_last_error()); return false; }
    return true;
}

size_t wr_roi_multi_elems(int nx, int ny, int nz, int level, const wr_box* rois, int nroi, size_t* offs)
{
    if (!roi_multi_args_ok(nx, ny, nz, level, wrlow::kMaxLevel, rois, nroi)) return 0;  // (the box of a level does not depend on wlev)
    size_t run = 0;
    for (int i = 0; i < nroi; i++) {
        if (offs) offs[i] = run;
        run += (size_t)(rois[i].x1 - rois[i].x0) * (size_t)(rois[i].y1 - rois[i].y0) * (size_t)(rois[i].z1 - rois[i].z0);
    }
    if (offs) offs[nroi] = run;
    return run;
}

size_t wr_seg_roi_segments_multi(int nx, int ny, int nz, int level, int wlev, const wr_box* rois, int nroi, unsigned brick, unsigned seg, uint32_t* ids,
                                 size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (brick && !blocked_args_ok(nx, ny, nz, wlev, &brick)) return 0;
    if (!roi_multi_args_ok(nx, ny, nz, level, wlev, rois, nroi)) return 0;
    const wrlow::Box box = wrlow::box_of(nx, ny, nz, level);
    std::vector<wrroi::Geometry> g((size_t)nroi);
    for (int i = 0; i < nroi; i++) g[i] = wrroi::geometry_of(box, wlev - level, rois[i]);
    if (brick) return wrblk::region_segments_multi(wrblk::order_of(nx, ny, nz, wlev, brick), g.data(), g.size(), seg, ids, ids ? cap : 0);
    return wrroi::segments_of_multi(nx, ny, nz, g.data(), g.size(), seg, ids, ids ? cap : 0);
}

// the regions of a masked region decode across a batch of fields as the mask sees them (wr_mask.h): host only
static std::vector<wrmask::Region> mask_regions(int nx, int ny, int nz, int level, const wr_box* rois, int nroi)
{
    std::vector<wrmask::Region> g((size_t)nroi);
    for (int i = 0; i < nroi; i++) g[i] = wrmask::Region{nx, ny, nz, level, rois[i].x0, rois[i].y0, rois[i].z0, rois[i].x1, rois[i].y1, rois[i].z1};
    return g;
}

size_t wr_mask_roi_segments_multi(int nx, int ny, int nz, int level, const wr_box* rois, int nroi, unsigned seg, uint32_t* ids, size_t cap)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!wrseg::seg_ok(seg)) { fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]"); return 0; }
    if (!roi_multi_args_ok(nx, ny, nz, level, wrlow::kMaxLevel, rois, nroi)) return 0;
    const std::vector<wrmask::Region> g = mask_regions(nx, ny, nz, level, rois, nroi);
    return wrmask::roi_segments_multi(g.data(), g.size(), seg, ids, ids ? cap : 0);
}

size_t wr_mask_boxes_turns(int nx, int ny, int nz, int level, const wr_box* rois, int nroi, uint32_t* first)
{
    if (!roi_multi_args_ok(nx, ny, nz, level, wrlow::kMaxLevel, rois, nroi)) return 0;
    const std::vector<wrmask::Region> g = mask_regions(nx, ny, nz, level, rois, nroi);
    const size_t turns = wrmask::boxes_turns(g.data(), g.size(), first);
    if (!turns) fail(WR_ERR_ARG, "too many turns: the regions have 2^31 or more");
    return turns;
}

}  // extern "C"
