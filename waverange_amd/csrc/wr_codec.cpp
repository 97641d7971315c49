// wr_codec.cpp -- the codec drivers of libwaverange_amd: a field through the stages of wr_pipeline.cpp.
//
// Mirrors the reference's codec layer (src/core/wrappers.cpp) for the path
//   encoding_wrap : min/max -> forward transform -> bit-plane quantizer loop -> range coder     (wrappers.cpp:228-452)
//   decoding_wrap : range decoder -> dequantise-accumulate -> inverse transform                  (wrappers.cpp:456-527)
// Compiled with hipcc, strict IEEE (-ffp-contract=off): the scalar arithmetic on deps/aopt/bopt/tolabs below must round
// exactly as wrappers.cpp:292-340 does.
#include <algorithm>
#include <cassert>
#include <map>

#include "wr_blocked.h"
#include "wr_budget.h"
#include "wr_internal.h"
#include "wr_lowres.h"
#include "wr_mask.h"
#include "wr_roi.h"
#include "wr_segbatch.h"
#include "wr_segcoder.h"
#include "wr_transcode.h"

using namespace wri;

namespace {

struct PlaneStep {
    double deps, minval, aopt, bopt;
    bool last;
};

// scalar side of one quantizer iteration, wrappers.cpp:316-340
PlaneStep plane_step(double lo, double hi, double tolabs, unsigned ilay)
{
    PlaneStep s;
    s.minval = lo;
    s.deps = (hi - lo) / (double)(256 - 1);
    s.last = false;
    if (s.deps < tolabs) { s.deps = tolabs; s.last = true; }
    if (ilay >= WR_NLAYMAX - 1u) s.last = true;
    s.aopt = 1.0 / s.deps;
    s.bopt = -lo * s.aopt + 0.5;
    return s;
}

// what the prologue of encoding_wrap computes, wrappers.cpp:235-266, 292-299
struct Prologue {
    bool trivial;
    double lo, hi;
};

template <typename T>
int prologue(wr_ctx* c, const T* d_fld, size_t n, int wtflag, wr_enc_info* info, Prologue* p)
{
    memset(info, 0, sizeof(*info));
    info->wlev = wtflag ? kWavLvl : 0;
    int rc = read_minmax(c, d_fld, n, false, &p->lo, &p->hi);
    if (rc) return rc;
    if (p->lo != p->lo || p->hi != p->hi) return fail(WR_ERR_ARG, "field is all NaN");
    info->halfspanval = (p->hi - p->lo) / 2;
    info->midval = p->lo + info->halfspanval;
    p->trivial = info->halfspanval <= 2 * DBL_MIN;
    return WR_OK;
}

double abs_tolerance(double tolrel, const Prologue& p)
{
    double tolabs = tolrel * fmax(fabs(p.lo), fabs(p.hi));
    tolabs /= kWavAccCoef;
    return tolabs;
}

}  // namespace

namespace {

// local cutoff description (mx*my*mz == 1: uniform cutoff, the benchmark path)
struct Cutoff {
    int mx = 1, my = 1, mz = 1;
    const double* vec = nullptr;  // host, mx*my*mz entries
    int count() const { return mx * my * mz; }
};

// where the field of an encode call comes from / the field of a decode call goes to
struct FieldRef {
    double* dev = nullptr;   // device-resident (caller's buffer), or
    double* host = nullptr;  // host buffer (pinned or pageable): staged through the slot, or
    float* host_f32 = nullptr;  // an fp32 host buffer: 4 bytes per sample cross the bus, widened / narrowed on the device
    bool none() const { return !dev && !host && !host_f32; }
};

// a constant field (ntot_enc == 0, wrappers.cpp:462-469): `count` elements of midval wherever the caller's field is
int fill_constant(wr_ctx* c, const FieldRef& fld, size_t count, double midval)
{
    if (fld.host) for (size_t j = 0; j < count; j++) fld.host[j] = midval;
    else if (fld.host_f32) for (size_t j = 0; j < count; j++) fld.host_f32[j] = (float)midval;
    else { wrk::fill(fld.dev, count, midval, c->stream); HIPCHK(hipStreamSynchronize(c->stream)); }
    return WR_OK;
}

// off[0 .. nlay]: where every plane's stream starts in the coded buffer, by the header's lengths; they must fit into ntot_enc,
// and that into the buffer (data_len == 0: its length is not known).  who: put in front of the messages ("field 3: ")
int plane_offsets(const wr_enc_info* info, int nlay, size_t data_len, size_t* off, const std::string& who = std::string())
{
    off[0] = 0;
    for (int l = 0; l < nlay; l++) off[l + 1] = off[l] + info->len_enc_vec[l];
    if (off[nlay] > info->ntot_enc) return fail(WR_ERR_STREAM, who + "len_enc_vec exceeds ntot_enc");
    if (data_len && info->ntot_enc > data_len) return fail(WR_ERR_STREAM, who + "ntot_enc exceeds the length of the coded buffer");
    return WR_OK;
}

// q[l] := ref_of(l), the symbols of plane l, for the first `used` planes; every one of them must be whole before a kernel writes it
template <class RefOf>
int plane_refs(int used, size_t n, RefOf ref_of, wrk::PlaneRef* q)
{
    for (int l = 0; l < used; l++) {
        q[l] = ref_of(l);
        if (!wrk::plane_ref_covers(q[l], n)) return fail(WR_ERR_HIP, "internal: the device buffer of plane " + std::to_string(l) + " has a hole");
    }
    return WR_OK;
}

// What the dequantizer is told: the first `used` planes of the header, their symbols as plane_refs finds them.
template <class RefOf>
int dequant_params(const wr_enc_info* info, int used, size_t n, RefOf ref_of, wrk::DequantParams* p)
{
    memset(p, 0, sizeof *p);
    p->nlay = used;
    for (int l = 0; l < used; l++) { p->deps[l] = info->deps_vec[l]; p->minval[l] = info->minval_vec[l]; }
    return plane_refs(used, n, ref_of, p->q);
}


// Kernel stage of the encoder (call with the slot leased and DevPool::cu_mu held).  Hooks for the full
// pipeline: hist_buf(l) says where plane l's block histograms go on the device (nullptr: nobody wants them);
// after_quant(l, hist_done) is called right after plane l's quantizer kernel and the read-back of the next
// plane's min/max have been enqueued (hist_done: the quantizer has written the histograms on its way; otherwise they
// are enqueued there, behind the read-back);
// plane_ready(l, last) is called from the host once everything enqueued for plane l has completed on the
// device (the download starts there).  *resid = where the coefficient array / residual lives afterwards.
// f32 != nullptr (an fp32 field on the fused path only): the field is that array, which the fused forward transform reads
// as it is; d_fld is then n doubles of work space (may be f32's memory: the transform has consumed it before it is used).
// pick != nullptr (an encode to a byte budget): the tolerance is not known when the loop starts.  Before every plane's step is
// formed, pick is told what the plane is cut from -- its number, the residual's range, the planes before and the array they
// apply to -- and sets info->tolabs: 0 for a plane that stays full, the chosen tolerance's for the last one.
using PickStep = std::function<int(unsigned ilay, double lo, double hi, const wrk::QuantPrev& prev, const double* d_coef, const Prologue& p, double* tolabs)>;

template <class PlaneBuf, class HistBuf, class AfterQuant, class PlaneReady>
int encode_planes_core(wr_ctx* c, Slot* slot, double* d_fld, int nx, int ny, int nz, int wtflag, const Cutoff& cut,
                       PlaneBuf plane_buf, HistBuf hist_buf, wr_enc_info* info, wr_timings* tm, AfterQuant after_quant, PlaneReady plane_ready,
                       double** resid, const float* f32 = nullptr, const PickStep* pick = nullptr)
{
    // minimum cutoff = the global relative tolerance (wrappers.cpp:288-290)
    double tolrel = cut.vec[0];
    for (int k = 1; k < cut.count(); k++) if (cut.vec[k] < tolrel) tolrel = cut.vec[k];
    const bool local = cut.count() > 1;
    if (local) {
        if (c->cutoff_elems < (size_t)cut.count()) {
            if (c->d_cutoff) HIPCHK(hipFree(c->d_cutoff));
            c->d_cutoff = nullptr; c->cutoff_elems = 0;
            HIPCHK(hipMalloc(&c->d_cutoff, cut.count() * sizeof(double)));
            c->cutoff_elems = cut.count();
        }
        HIPCHK(hipMemcpyAsync(c->d_cutoff, cut.vec, cut.count() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    const size_t n = (size_t)nx * ny * nz;
    Prologue p;
    *resid = d_fld;
    double lo, hi;
    float ms = 0;
    // When all four levels run on the fused kernels, those reduce min/max of the field and of the coefficient
    // array on the way (no stand-alone passes, one host round trip instead of two).  The transform then runs
    // before it is known whether the field is trivial; it is out of place, so nothing is lost if it is.
    const size_t mm_records = (wtflag && use_fused(nx, ny, nz, kWavLvl)) ? wrk::fused_minmax_records(nx, ny, nz) : 0;
    if (mm_records) {
        if (const char* why = wrk::fused_prepare()) return fail(WR_ERR_HIP, why);
        if (c->mm_records < mm_records) {
            if (c->d_mm) HIPCHK(hipFree(c->d_mm));
            c->d_mm = nullptr; c->mm_records = 0;
            HIPCHK(hipMalloc(&c->d_mm, mm_records * 4 * sizeof(double)));
            c->mm_records = mm_records;
        }
        memset(info, 0, sizeof(*info));
        info->wlev = kWavLvl;
        double* const d_in = d_fld;
        HIPCHK(hipEventRecord(c->ev_b, c->stream));
        if (f32) wrk::transform_fwd_fused_f32(f32, d_in, slot->scratch, slot->lowbuf, nx, ny, nz, c->stream, c->d_mm, c->h_result_dev + 4);
        else wrk::transform_fwd_fused(d_in, slot->scratch, slot->lowbuf, nx, ny, nz, c->stream, c->d_mm, c->h_result_dev + 4);
        HIPCHK(hipEventRecord(c->ev_c, c->stream));
        HIPCHK(hipEventRecord(c->ev_mm, c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventSynchronize(c->ev_mm));
        p.lo = c->h_result[4]; p.hi = c->h_result[5];
        lo = c->h_result[6]; hi = c->h_result[7];
        if (p.lo == 0.0) {  // sign of a zero minimum: the reference's scan semantics, rare path
            if (int rc = f32 ? read_minmax(c, f32, n, false, &p.lo, &p.hi) : read_minmax(c, d_in, n, false, &p.lo, &p.hi)) return rc;
        }
        if (p.lo != p.lo || p.hi != p.hi) return fail(WR_ERR_ARG, "field is all NaN");
        info->halfspanval = (p.hi - p.lo) / 2;
        info->midval = p.lo + info->halfspanval;
        p.trivial = info->halfspanval <= 2 * DBL_MIN;
        if (verbose()) printf("Wavelet decomposition...\n");
        if (p.trivial) {  // wrappers.cpp:256-266
            info->ntot_enc = 0; info->nlay = 0; info->tolabs = 0;
            return WR_OK;
        }
        d_fld = slot->scratch;  // d_fld := coefficients
        *resid = d_fld;
        if (verbose()) printf("Range encoding...\n");
        info->tolabs = abs_tolerance(tolrel, p);
        if (lo == 0.0)
            if (int rc = read_minmax(c, d_fld, n, false, &lo, &hi)) return rc;
        if (tm) { HIPCHK(hipEventElapsedTime(&ms, c->ev_b, c->ev_c)); tm->transform_ms = ms; tm->minmax_ms = 0; }
    } else {
    HIPCHK(hipEventRecord(c->ev_a, c->stream));
    if (int rc = f32 ? prologue(c, f32, n, wtflag, info, &p) : prologue(c, (const double*)d_fld, n, wtflag, info, &p)) return rc;
    if (verbose()) printf("Wavelet decomposition...\n");
    if (p.trivial) {  // wrappers.cpp:256-266
        info->ntot_enc = 0; info->nlay = 0; info->tolabs = 0;
        return WR_OK;
    }
    HIPCHK(hipEventRecord(c->ev_b, c->stream));
    if (int rc = run_transform(c, slot, d_fld, nx, ny, nz, (int)info->wlev, &d_fld, f32)) return rc;  // d_fld := coefficients
    *resid = d_fld;
    HIPCHK(hipEventRecord(c->ev_c, c->stream));
    if (verbose()) printf("Range encoding...\n");
    info->tolabs = abs_tolerance(tolrel, p);

    if (int rc = read_minmax(c, d_fld, n, false, &lo, &hi)) return rc;
    HIPCHK(hipEventRecord(c->ev_d, c->stream));
    HIPCHK(hipEventSynchronize(c->ev_d));
    if (tm) {
        HIPCHK(hipEventElapsedTime(&ms, c->ev_b, c->ev_c)); tm->transform_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b)); tm->minmax_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_c, c->ev_d)); tm->minmax_ms += ms;
    }
    }
    unsigned ilay = 0;
    float quant_ms = 0;
    // The residual is not kept in memory between planes (wr_kernels.hip: k_quant_blk): d_fld stays the coefficient array, every
    // plane's kernel redoes the subtractions of the planes in `prev`.  The local-cutoff quantizer and unaligned caller
    // pointers keep the reference's form (the array is updated in place after every plane).
    wrk::QuantPrev prev;
    for (;;) {
        if (pick) if (int rc = (*pick)(ilay, lo, hi, prev, d_fld, p, &info->tolabs)) return rc;
        PlaneStep s = plane_step(lo, hi, info->tolabs, ilay);
        info->minval_vec[ilay] = s.minval;
        info->deps_vec[ilay] = s.deps;
        if (verbose()) { printf("min=%g max=%g\n", lo, hi); printf("ilay=%u deps=%g\n", ilay, s.deps); }
        const wrk::PlaneRef* const d_plane = plane_buf(ilay);  // device memory of this plane (the error is set if there is none)
        if (!d_plane) return WR_ERR_HIP;
        if (!wrk::plane_ref_covers(*d_plane, n)) return fail(WR_ERR_HIP, "internal: the device buffer of plane " + std::to_string(ilay) + " has a hole");
        // (a chunked plane is only ever indexed through its table: the direct-form kernels for unaligned pointers take one array)
        if (d_plane->shift < 63 && (((uintptr_t)d_fld | (uintptr_t)d_plane->chunk[0]) & 15)) return fail(WR_ERR_ARG, "internal: chunked plane with an unaligned pointer");
        const bool blk = !local && (prev.n > 0 || ilay == 0) && wrk::quantize_plane_blk_ok(d_fld, *d_plane);
        const bool resid_upd = blk ? (s.last && c->keep_residual) : (!s.last || c->keep_residual);
        // (the histograms by a kernel of their own behind the quantizer: 10.7 + 0.9 ms per field against 6.7,
        // profiles/r04/x_quantizer_with_and_without_fused_histograms.txt)
        uint16_t* const d_hist = blk ? hist_buf(ilay) : nullptr;
        launch_note(c, local ? "quant_local" : blk ? (resid_upd ? "quant_blk<1>" : "quant_blk<0>") : resid_upd ? "quant<1>" : "quant<0>", (int)ilay, d_fld, n,
                    c->d_partial, *d_plane);
        HIPCHK(hipEventRecord(c->ev_a, c->stream));
        if (local) {
            wrk::LocalCutoff lc;
            lc.nx = nx; lc.ny = ny; lc.nz = nz; lc.wlev = info->wlev;
            lc.mx = cut.mx; lc.my = cut.my; lc.mz = cut.mz;
            lc.cutoff = c->d_cutoff;
            lc.tol_scale = info->tolabs / tolrel;
            lc.tolabs = info->tolabs;
            lc.span = hi - lo;
            wrk::quantize_plane_local(d_fld, n, s.aopt, s.bopt, s.deps, s.minval, d_plane->chunk[0], lc,  // (one array: plane_prepare(contiguous))
                                      c->d_partial, c->h_result_dev, c->stream);
        } else if (blk)
            wrk::quantize_plane_blk(d_fld, n, prev, s.aopt, s.bopt, s.deps, s.minval, *d_plane, resid_upd, !s.last, d_hist, c->d_partial,
                                    c->h_result_dev, c->stream);
        else
            wrk::quantize_plane(d_fld, n, s.aopt, s.bopt, s.deps, s.minval, *d_plane, resid_upd, c->d_partial, c->h_result_dev, c->stream);
        HIPCHK(hipEventRecord(c->ev_b, c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "quantizer launch failed" + launch_describe(c));
        // the next plane's min/max is in host memory when this event fires (the reduction stores it there); what
        // after_quant enqueues runs behind it
        HIPCHK(hipEventRecord(c->ev_mm, c->stream));
        if (int rc = after_quant(ilay, d_hist != nullptr)) return rc;
        HIPCHK(hipEventRecord(c->ev_plane[ilay], c->stream));
        HIPCHK(hipEventSynchronize(c->ev_mm));
        HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b)); quant_ms += ms;
        // plane ilay-1 is complete: what after_quant enqueued for it ran before this plane's quantizer
        if (ilay > 0) if (int rc = plane_ready(ilay - 1, false)) return rc;
        if (s.last) {
            HIPCHK(hipEventSynchronize(c->ev_plane[ilay]));
            if (int rc = plane_ready(ilay, true)) return rc;
            ilay++;
            break;
        }
        if (blk) prev.push(s.aopt, s.bopt, s.deps, s.minval);
        ilay++;
        lo = c->h_result[0]; hi = c->h_result[1];
        // (WR_TEST_ZERO_MIN_PATH=1: tests take the rare path below after every plane)
        static const bool force_rare = getenv("WR_TEST_ZERO_MIN_PATH") && atoi(getenv("WR_TEST_ZERO_MIN_PATH"));
        if (lo == 0.0 || force_rare) {  // sign of a zero minimum: rare path, goes through the full read-back -- of the residual, in memory
            if (prev.n) { wrk::residual_apply(d_fld, n, prev, c->stream); prev.n = 0; }  // (the planes from here on update it in place)
            if (int rc = read_minmax(c, d_fld, n, true, &lo, &hi)) return rc;
        }
    }
    info->nlay = (unsigned char)ilay;
    if (tm) tm->quant_ms = quant_ms;
    return WR_OK;
}

}  // namespace

extern "C" {

int wr_dev_encode_planes(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, double tolrel,
                         unsigned char* d_planes, wr_enc_info* info)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_fld)) return rc;
    if ((uintptr_t)d_planes & 15) return fail(WR_ERR_ARG, "plane buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    SlotNeed need;
    transform_need(nx, ny, nz, wtflag ? kWavLvl : 0, &need);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    StageLock cu(c->pool->cu_mu);
    Cutoff cut; cut.vec = &tolrel;
    double* resid = nullptr;
    const size_t pitch = wr_plane_pitch((size_t)nx * ny * nz);
    wrk::PlaneRef refs[WR_NLAYMAX];
    for (int l = 0; l < WR_NLAYMAX; l++) refs[l] = wrk::plane_ref(d_planes + l * pitch);
    int rc = encode_planes_core(c, slot.get(), d_fld, nx, ny, nz, wtflag, cut, [&](unsigned l) { return &refs[l]; },
                                [](unsigned) { return (uint16_t*)nullptr; }, info, nullptr, [](unsigned, bool) { return WR_OK; },
                                [](unsigned, bool) { return WR_OK; }, &resid);
    if (rc == WR_OK && resid != d_fld && info->nlay)  // d_fld holds the residual afterwards (header contract)
        if (hipMemcpyAsync(d_fld, resid, (size_t)nx * ny * nz * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = fail(WR_ERR_HIP, "residual copy failed");
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int wr_dev_decode_planes(wr_ctx* c, double* d_fld, int nx, int ny, int nz, const unsigned char* d_planes,
                         const wr_enc_info* info)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_fld)) return rc;
    const size_t n = (size_t)nx * ny * nz;
    std::lock_guard<std::mutex> lk(c->mu);
    if (info->ntot_enc == 0 && info->nlay == 0) return fill_constant(c, FieldRef{d_fld}, n, info->midval);
    if (info->nlay > WR_NLAYMAX) return fail(WR_ERR_ARG, "nlay out of range");
    SlotNeed need;
    transform_need(nx, ny, nz, info->wlev ? -kWavLvl : 0, &need);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    StageLock cu(c->pool->cu_mu);
    wrk::DequantParams p;
    memset(&p, 0, sizeof p);
    p.nlay = info->nlay;
    for (int l = 0; l < p.nlay; l++) {
        p.q[l] = wrk::plane_ref(d_planes + l * wr_plane_pitch(n));
        p.deps[l] = info->deps_vec[l];
        p.minval[l] = info->minval_vec[l];
    }
    int rc = inverse_from_planes(c, slot.get(), d_fld, nx, ny, nz, (int)info->wlev, p);
    if (rc == WR_OK && hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "kernel launch failed");
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // extern "C"

// ---- low-resolution decode (include/waverange_amd.h): the box of level r out of the first p planes, the remaining levels
// inverted on the box, the gain of the r levels that stay taken out
namespace {

// What a partial decode of segmented planes runs on: the box of level r (roi == false, the low-resolution decode) or the
// window of a region of that box (roi == true, wr_roi.h).  The plan carries the segments the planes need, the gather, the
// extents of the array the inverse runs on and the finish; the drivers below are the same for both.
struct LowresPlan {
    wrlow::Box box;
    int planes;   // p
    int inverse;  // levels the box is still transformed by: wlev - r
    double scale;
    bool roi = false;
    wrroi::Geometry win;  // roi only
    int stat_segments = WR_STAT_LOWRES_SEGMENTS, stat_bytes_up = WR_STAT_LOWRES_BYTES_UP;

    size_t out_elems() const { return roi ? win.out_elems() : box.elems(); }   // what the caller receives
    size_t work_elems() const { return roi ? win.elems() : box.elems(); }      // what the inverse runs on
    bool fused() const { return roi && use_fused_window(win.w(0), win.w(1), win.w(2), inverse); }
    // the ascending ids of the segments a plane cut at `seg` needs
    void segments(int nx, int ny, int nz, uint32_t seg, std::vector<uint32_t>* ids) const
    {
        ids->resize(roi ? wrroi::segments_of(nx, ny, nz, win, seg, nullptr, 0) : wrlow::segments_of(nx, ny, box, seg, nullptr, 0));
        if (roi) wrroi::segments_of(nx, ny, nz, win, seg, ids->data(), ids->size());
        else wrlow::segments_of(nx, ny, box, seg, ids->data(), ids->size());
    }
    // the same for a plane in the blocked order (wr_blocked.h): a prefix for a box
    void segments_blocked(const wrblk::Order& od, uint32_t seg, std::vector<uint32_t>* ids) const
    {
        if (roi) {
            ids->resize(wrblk::region_segments(od, win, seg, nullptr, 0));
            wrblk::region_segments(od, win, seg, ids->data(), ids->size());
        } else {
            ids->resize(wrblk::lowres_segments(od.nx, od.ny, od.nz, od.wlev - inverse, seg, nullptr, 0));
            wrblk::lowres_segments(od.nx, od.ny, od.nz, od.wlev - inverse, seg, ids->data(), ids->size());
        }
    }
    // the ascending ids of the bricks the plan needs: those the window's source boxes meet, or all bricks of the boxes that
    // tile the box of the level
    void bricks(const wrblk::Order& od, std::vector<uint32_t>* ids) const
    {
        if (roi) { wrblk::region_bricks(od, win, ids); return; }
        const int nb = wrblk::prefix_boxes(od, od.wlev - inverse);
        const uint64_t count = nb < od.nbox ? od.box[nb].first_brick : od.nbricks;
        ids->resize(count);
        for (uint64_t k = 0; k < count; k++) (*ids)[k] = (uint32_t)k;
    }
    // the work space of the kernel stage: a box is inverted in the caller's (or the staging) array, a window in the slot's
    // field buffer whoever the caller is, and what comes out of it is smaller
    void need(bool host, SlotNeed* nd) const
    {
        nd->scratch_elems = work_elems();
        if (host || roi) nd->field_elems = work_elems();
        if (fused()) nd->lowbuf_elems = wrk::fused_lowbuf_elems(win.w(0), win.w(1), win.w(2));
    }
};

int lowres_plan(int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info, LowresPlan* pl)
{
    if (!wrlow::level_ok(level)) return fail(WR_ERR_ARG, "level must be in [0, 4]");
    if (info->wlev != 0 && info->wlev != kWavLvl) return fail(WR_ERR_ARG, "wlev must be 0 or 4");
    if (level > (int)info->wlev) return fail(WR_ERR_ARG, "level exceeds the transform depth of the stream (a field coded without the transform has level 0 only)");
    if (info->nlay > WR_NLAYMAX) return fail(WR_ERR_ARG, "nlay out of range");
    if (max_planes < 0 || max_planes > (int)info->nlay) return fail(WR_ERR_ARG, "max_planes exceeds the planes of the stream");
    pl->box = wrlow::box_of(nx, ny, nz, level);
    pl->planes = max_planes ? max_planes : (int)info->nlay;
    pl->inverse = (int)info->wlev - level;
    pl->scale = wrlow::scale_of(pl->box);
    return WR_OK;
}

// roi == nullptr: the plan of the low-resolution decode
int region_plan(int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info, LowresPlan* pl)
{
    if (int rc = lowres_plan(nx, ny, nz, level, max_planes, info, pl)) return rc;
    if (!roi) return WR_OK;
    if (!wrroi::roi_ok(pl->box, *roi)) return fail(WR_ERR_ARG, "the region is empty or reaches outside the box of the level");
    pl->roi = true;
    pl->win = wrroi::geometry_of(pl->box, pl->inverse, *roi);
    pl->stat_segments = WR_STAT_ROI_SEGMENTS;
    pl->stat_bytes_up = WR_STAT_ROI_BYTES_UP;
    return WR_OK;
}

// Kernel stage (slot leased, DevPool::cu_mu held): d_box := the box of the planes in p, inverted and scaled.  The slot's
// scratch buffer holds box.elems() doubles.  out_f32 != nullptr: the result is wanted in fp32; *out_f32 = where it landed
// (the scratch buffer, which the transform is done with by then).  Records ev_a / ev_b / ev_c as inverse_from_planes.
int lowres_from_planes(wr_ctx* c, Slot* s, double* d_box, int nx, int ny, const LowresPlan& pl, const wrk::DequantParams& p, float** out_f32)
{
    const wrlow::Box& b = pl.box;
    HIPCHK(hipEventRecord(c->ev_a, c->stream));
    wrk::dequant_box(d_box, b.bx, b.by, b.bz, nx, ny, p, c->stream);
    HIPCHK(hipEventRecord(c->ev_b, c->stream));
    if (pl.inverse > 0) wrk::transform(d_box, s->scratch, b.bx, b.by, b.bz, -pl.inverse, c->stream);
    if (out_f32) {
        *out_f32 = reinterpret_cast<float*>(s->scratch);
        wrk::scale_narrow_f64(d_box, *out_f32, b.elems(), pl.scale, c->stream);
    } else if (pl.scale != 1.0) {
        wrk::scale_f64(d_box, d_box, b.elems(), pl.scale, c->stream);
    }
    HIPCHK(hipEventRecord(c->ev_c, c->stream));
    return WR_OK;
}

// The same for a region: the window's coefficients gathered, inverted in the slot (the fused kernels where the window's
// extents allow them: out of place, from the scratch buffer into the field buffer; otherwise in place in the field buffer),
// then the crop, scaled, into d_out -- or, d_out == nullptr (a host caller), into the scratch buffer, which the transform is
// done with by then; *landed = where.  f32: the crop is narrowed.
int roi_from_planes(wr_ctx* c, Slot* s, double* d_out, int nx, int ny, const LowresPlan& pl, const wrk::DequantParams& p, bool f32, void** landed)
{
    const wrroi::Geometry& g = pl.win;
    const int wx = g.w(0), wy = g.w(1), wz = g.w(2);
    const wrk::WindowMap m = window_map_of(g, nx, ny);
    const bool fused = pl.fused();
    if (fused) if (const char* why = wrk::fused_prepare()) return fail(WR_ERR_HIP, why);
    HIPCHK(hipEventRecord(c->ev_a, c->stream));
    wrk::dequant_window(fused ? s->scratch : s->field, m, p, c->stream);
    HIPCHK(hipEventRecord(c->ev_b, c->stream));
    if (fused) wrk::transform_inv_fused(s->scratch, s->field, s->lowbuf, wx, wy, wz, c->stream);
    else if (pl.inverse > 0) wrk::transform(s->field, s->scratch, wx, wy, wz, -pl.inverse, c->stream);
    const wrk::CropBox crop{(uint32_t)wx, (uint32_t)wy, (uint32_t)(g.ax[0].lo - g.ax[0].a), (uint32_t)(g.ax[1].lo - g.ax[1].a),
                            (uint32_t)(g.ax[2].lo - g.ax[2].a), (uint32_t)(g.ax[0].hi - g.ax[0].lo), (uint32_t)(g.ax[1].hi - g.ax[1].lo),
                            (uint32_t)(g.ax[2].hi - g.ax[2].lo)};
    *landed = d_out ? (void*)d_out : (void*)s->scratch;
    if (f32) wrk::crop_scale_narrow_f64(s->field, reinterpret_cast<float*>(*landed), crop, pl.scale, c->stream);
    else wrk::crop_scale_f64(s->field, reinterpret_cast<double*>(*landed), crop, pl.scale, c->stream);
    HIPCHK(hipEventRecord(c->ev_c, c->stream));
    return WR_OK;
}

// stage level: the plan's result from nlay full planes in device memory
int decode_planes_plan(wr_ctx* c, double* d_out, int nx, int ny, int nz, const LowresPlan& pl, const unsigned char* d_planes, const wr_enc_info* info)
{
    const size_t n = (size_t)nx * ny * nz;
    std::lock_guard<std::mutex> lk(c->mu);
    if (info->ntot_enc == 0 && info->nlay == 0) return fill_constant(c, FieldRef{d_out}, pl.out_elems(), info->midval);
    if (!d_planes) return fail(WR_ERR_ARG, "null plane pointer");
    SlotNeed need;
    pl.need(false, &need);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    StageLock cu(c->pool->cu_mu);
    wrk::DequantParams p;
    memset(&p, 0, sizeof p);
    p.nlay = pl.planes;
    for (int l = 0; l < p.nlay; l++) {
        p.q[l] = wrk::plane_ref(d_planes + l * wr_plane_pitch(n));
        p.deps[l] = info->deps_vec[l];
        p.minval[l] = info->minval_vec[l];
    }
    void* landed = nullptr;
    int rc = pl.roi ? roi_from_planes(c, slot.get(), d_out, nx, ny, pl, p, false, &landed) : lowres_from_planes(c, slot.get(), d_out, nx, ny, pl, p, nullptr);
    if (rc == WR_OK && hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "kernel launch failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the low-resolution kernel stage failed on the device");
    return rc;
}

}  // namespace

extern "C" int wr_dev_decode_planes_lowres(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const unsigned char* d_planes,
                                           const wr_enc_info* info)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_out)) return rc;
    if (!d_out || !info) return fail(WR_ERR_ARG, "null pointer");
    LowresPlan pl;
    if (int rc = region_plan(nx, ny, nz, level, max_planes, nullptr, info, &pl)) return rc;
    return decode_planes_plan(c, d_out, nx, ny, nz, pl, d_planes, info);
}

extern "C" int wr_dev_decode_planes_roi(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                                        const unsigned char* d_planes, const wr_enc_info* info)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_out)) return rc;
    if (!d_out || !info || !roi) return fail(WR_ERR_ARG, "null pointer");
    LowresPlan pl;
    if (int rc = region_plan(nx, ny, nz, level, max_planes, roi, info, &pl)) return rc;
    return decode_planes_plan(c, d_out, nx, ny, nz, pl, d_planes, info);
}

namespace {

// ---- stages that every encode driver takes, whatever codes the planes ---------------------------------------------------
// Stage "up": a host field onto the leased slot.  An fp32 field: the fused forward transform reads it where it lands (the
// slot's field buffer, which is work space of n doubles from then on); elsewhere it lands in the scratch buffer and the caller
// widens it into the field buffer in front of the fp64 path (the general transform's scratch is free until then).
struct FieldUpload {
    double* d_fld = nullptr;       // the field as doubles, or -- d_f32 set -- n doubles of work space
    const float* d_f32 = nullptr;  // the fp32 field as the fused forward transform reads it
    float* widen_from = nullptr;   // the fp32 field that wrk::widen_f32 takes to d_fld
    float ms = 0;                  // the copy, for h2d_ms
};

int upload_field(wr_ctx* c, Slot* slot, const FieldRef& fld, int nx, int ny, int nz, int wtflag, FieldUpload* u)
{
    const size_t n = (size_t)nx * ny * nz;
    u->d_fld = fld.dev ? fld.dev : slot->field;
    if (fld.dev) return WR_OK;
    if (fld.host) {
        if (int rc = xfer_field(c, &c->x_field, u->d_fld, fld.host, n * sizeof(double), kUp)) return rc;
    } else {
        float* const stage = (wtflag && use_fused(nx, ny, nz, kWavLvl)) ? reinterpret_cast<float*>(slot->field) : reinterpret_cast<float*>(slot->scratch);
        if (int rc = xfer_field(c, &c->x_field, stage, fld.host_f32, n * sizeof(float), kUp)) return rc;
        if (stage == reinterpret_cast<float*>(slot->field)) u->d_f32 = stage;
        else u->widen_from = stage;
    }
    u->ms = (float)c->x_field.ms;
    return WR_OK;
}

// The end of a single-field encode's kernel stage (cu_mu held): rc is encode_planes_core's.  With the residual kept, a
// device-resident field receives it here, where the reference leaves it; a host field's follows in the caller's "down" stage.
int encode_stage_end(wr_ctx* c, int rc, const FieldRef& fld, const double* resid, size_t n, const wr_enc_info* info)
{
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the encoder's kernel stage failed on the device" + launch_describe(c));
    if (rc == WR_OK && c->keep_residual && info->nlay && !fld.host && resid != fld.dev) {
        if (hipMemcpyAsync(fld.dev, resid, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            rc = fail(WR_ERR_HIP, "residual copy failed");
    }
    c->pool->last_stage_end.store(now());
    return rc;
}

// Where the host coder of a plane writes (an encode into the reference's format; a transcode into it).  The reference codes
// every plane into a buffer of its own and copies the streams together (wrappers.cpp:412-427); here the planes are coded at the
// same time, so a plane's place in `out` is not known when its coder starts -- but an upper bound on the length of every plane
// before it is, from their block histograms (wrrc::encode_bound_hist: rigorous, ~0.2 % above the stream).  Plane l is coded
// straight into `out` at the sum of the bounds of planes 0 .. l-1, and the gaps are closed afterwards by moving the planes down
// in order (a few megabytes each: ref_stream_tail).  The coded bytes of a field then exist once in host memory, not twice (a
// 1e-7 field at 1024^3: 2 GB), and the context keeps no per-plane output buffers.  A plane whose bound does not fit under `cap`
// takes the old way through c->enc_buf (only then can total <= cap < sum of bounds happen).  The coder is told the bound
// (dst_limit): a stream that outgrows it was coded against histograms that are not its plane's and is given up, at most one
// block (wrrc::kFailedBlockSlack) late -- which is why that much room lies behind every plane's place.
struct RefPlacement {
    size_t est_off[WR_NLAYMAX + 1] = {0}, est_len[WR_NLAYMAX] = {0};
    bool direct[WR_NLAYMAX] = {false};

    // Places plane j, the planes before it being placed: hist: its block histograms on the host (nullptr: they did not
    // arrive, the bound is that of any plane of n symbols).  *dst = where its coder writes, nullptr if there is no host memory.
    int place(wr_ctx* c, unsigned j, const uint16_t* hist, size_t n, unsigned char* out, size_t cap, uint8_t** dst)
    {
        *dst = nullptr;
        est_len[j] = hist ? wrrc::encode_bound_hist(hist, n) : wrrc::encode_bound(n);
        est_off[j + 1] = est_off[j] + est_len[j];
        direct[j] = out && est_off[j + 1] + wrrc::kFailedBlockSlack <= cap;
        if (!direct[j]) if (int rc = ensure_enc_buf(c, (int)j, est_len[j] + wrrc::kFailedBlockSlack)) return rc;
        *dst = direct[j] ? out + est_off[j] : c->enc_buf[j];
        return WR_OK;
    }
};

// what coding plane l to dst, its place (RefPlacement::place), means to whoever codes it
void ref_encode_job(wr_ctx* c, unsigned l, size_t n, const uint16_t* hist, const RefPlacement& pl, uint8_t* dst, wrrc::PlaneJob* j)
{
    j->kind = wrrc::PlaneJob::kEncode;
    j->io = &c->ps[l].io; j->dst = dst; j->n = n; j->hist = hist; j->dst_limit = pl.est_len[l];
}

// The tail of an encode into the reference's format, once every plane's coder has returned: jobs[l] coded plane l to where it
// was placed -- pl.direct[l]: at out + pl.est_off[l]; otherwise into c->enc_buf[l].  Checks every plane (download_failed(l): its
// symbols did not reach the coder), gives lens[l] and *total, closes the gaps in `out` and hands the pages of the context's
// buffers back.  too_large: the text of total > cap.
template <class Failed>
int ref_stream_tail(wr_ctx* c, const wrrc::PlaneJob* jobs, unsigned nlay, Failed download_failed, const RefPlacement& pl, unsigned char* out, size_t cap,
                    const char* too_large, size_t* lens, size_t* total)
{
    for (unsigned l = 0; l < nlay; l++) {
        if (download_failed(l)) return fail(WR_ERR_HIP, "download of plane " + std::to_string(l) + " failed");
        if (jobs[l].result == (size_t)-1)  // (a refused window sets ps[l].err as well; what is left: histograms that are not the plane's)
            return fail(WR_ERR_HIP, "internal: the coder gave plane " + std::to_string(l) + " up (its block histograms are not its symbols')");
    }
    // concatenate the plane streams (wrappers.cpp:412-427)
    size_t offs[WR_NLAYMAX] = {0};
    *total = 0;
    for (unsigned l = 0; l < nlay; l++) {
        offs[l] = *total;
        *total += jobs[l].result;
        lens[l] = jobs[l].result;
    }
    for (unsigned l = 0; l < nlay; l++)  // (cannot happen: the bound is rigorous; if it did, a neighbour's bytes are gone)
        if (jobs[l].result > pl.est_len[l]) return fail(WR_ERR_OVERFLOW, "internal: plane " + std::to_string(l) + " outgrew the bound computed from its histograms");
    if (*total > cap) return fail(WR_ERR_OVERFLOW, too_large);
    // close the gaps: plane l moves down by what the planes before it stayed below their bounds.  In plane order, one after
    // the other: plane l's new place may still hold the end of plane l-1's old one.
    for (unsigned l = 0; l < nlay; l++) {
        if (!pl.direct[l]) memcpy(out + offs[l], c->enc_buf[l], lens[l]);
        else if (pl.est_off[l] != offs[l]) memmove(out + offs[l], out + pl.est_off[l], lens[l]);
    }
    // (a plane that went through c->enc_buf: hand its pages back, a noise plane's gigabyte would otherwise stay resident in
    // every context that once coded one)
    for (unsigned l = 0; l < nlay; l++) {
        if (pl.direct[l]) continue;
        const uintptr_t a = ((uintptr_t)c->enc_buf[l] + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)c->enc_buf[l] + lens[l]) & ~(uintptr_t)4095;
        if (e > a && e - a >= ((size_t)64 << 20)) (void)madvise(reinterpret_cast<void*>(a), e - a, MADV_DONTNEED);
    }
    return WR_OK;
}

// plane_coder_s[l] += the seconds jobs[l]'s coder took; returns the slowest plane's, which is what the call waited for (the
// planes are coded at the same time)
double fold_plane_seconds(const wrrc::PlaneJob* jobs, int count, wr_timings* tm)
{
    double slowest = 0;
    for (int l = 0; l < count; l++) {
        tm->plane_coder_s[l] += jobs[l].seconds;
        slowest = std::max(slowest, jobs[l].seconds);
    }
    return slowest;
}

// Hands jobs[0, count), every one of them ready, to whoever codes them, and returns when all are done: the process-wide coder
// pool (wr_set_coder_pool), whose workers interleave planes of several fields -- or, without a pool or with one that was stopped
// meanwhile, min(count, threads) threads of this call, each with its contiguous group of planes interleaved (wr_set_threads;
// one plane each by default).  gate != nullptr: the admission-gate lock of a decode (ref_decode_planes), released once the jobs
// are queued, and on every other way out.  who ("decode: "): in front of the text of a thread that cannot start.
int run_plane_jobs(wrrc::PlaneJob* jobs, int count, int threads, int dev, std::unique_lock<std::mutex>* gate, const char* who)
{
    bool pooled = wrrc::pool_threads() > 0;
    if (pooled) {
        wrrc::JobBatch batch;
        pooled = wrrc::pool_submit(jobs, count, &batch);
        if (gate && gate->owns_lock()) gate->unlock();  // the next decode may look at the queues now
        if (pooled) wrrc::pool_wait(&batch);
    }
    if (gate && gate->owns_lock()) gate->unlock();
    if (pooled) return WR_OK;
    const int groups = std::min(count, threads);
    try {
        Workers workers;  // (joined on every way out of the block)
        for (int g = 0; g < groups; g++)
            workers.v.emplace_back([=]() {
                (void)hipSetDevice(dev);
                const int l0 = g * count / groups, l1 = (g + 1) * count / groups;
                wrrc::run_jobs(jobs + l0, l1 - l0);
            });
    } catch (const std::exception& e) {
        return fail(WR_ERR_ARG, std::string(who) + e.what());
    }
    return WR_OK;
}

// admission gate of the pooled decoder (ref_decode_planes): queued jobs of a kind at which a further decode waits
constexpr int kGateScalarJobs = 3, kGateVectorJobs = 6;

// The host half of a decode from the reference's format: plane l of the stream (`data` + off[l], info->len_enc_vec[l] bytes) is
// range-decoded into the context's device plane l, every decoded window going up while the decoder fills the next one
// (chunk by chunk: wrappers.cpp:492-516 reorganised); no field buffer and no slot is needed.  tm receives
// plane_coder_s, the slowest plane's seconds (added to rangecoder) and the uploads (h2d_ms).  Of several planes that do not
// decode, the first is named.
int ref_decode_planes(wr_ctx* c, const wr_enc_info* info, int nlay, size_t n, const unsigned char* data, const size_t* off, const char* who, wr_timings* tm)
{
    if (verbose()) printf("Range decoding...\n");
    DevPool* const pool = c->pool;
    // Admission to the coder pool.  A decoder's planes take device memory from the moment they are prepared, and with every
    // session of the pool full a decode's jobs sat in the queues for seconds (4 of a decode's 15 s at 32 lanes) -- a third of
    // the decoders' plane memory was held by planes nobody was writing yet, and plane memory is what bounds the fields in
    // flight.  So a decode waits HERE, holding nothing, until the queues of its kind are short (a free lane of a session is
    // refilled at the next block boundary, half a millisecond away: a couple of queued jobs keep every session topped up),
    // and only then prepares its planes and submits: the same wait, without the memory.  One decode at a time passes, from
    // the look at the queues to the submit (else all that wait would pass together).
    std::unique_lock<std::mutex> gate(pool->planes.gate_mu, std::defer_lock);
    if (wrrc::pool_threads() > 0) {
        gate.lock();
        const double t_gate = now();
        for (;;) {
            int qs = 0, qv = 0;
            wrrc::pool_queued_decode(&qs, &qv);
            if ((qs < kGateScalarJobs && qv < kGateVectorJobs) || now() - t_gate > 120.0) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
        g_stat[WR_STAT_DECODE_GATE_MS] += (unsigned long)((now() - t_gate) * 1e3);
    }
    {
        // one decode at a time gathers its planes: a decoder keeps them all until its field is done, so two that each hold
        // half of theirs and wait for the other half would never finish
        const double t_turn = now();
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);
        const double t_got = now();
        if (t_got - t_turn > 1e-3) g_stat[WR_STAT_PLANE_WAIT_MS] += (unsigned long)((t_got - t_turn) * 1e3);
        for (int l = 0; l < nlay; l++) if (int rc = plane_prepare(c, l, n, true)) return rc;
    }
    wrrc::PlaneJob jobs[WR_NLAYMAX];  // what decoding plane l means, whoever decodes it
    for (int l = 0; l < nlay; l++) {
        jobs[l].kind = wrrc::PlaneJob::kDecode;
        jobs[l].src = data + off[l]; jobs[l].src_len = info->len_enc_vec[l]; jobs[l].io = &c->ps[l].io; jobs[l].n = n;
    }
    if (int rc = run_plane_jobs(jobs, nlay, coder_threads(), c->device, &gate, who)) return rc;
    for (int l = 0; l < nlay; l++)
        if (jobs[l].result != n) return fail(WR_ERR_STREAM, "plane " + std::to_string(l) + ": stream does not decode to nx*ny*nz symbols");
    tm->rangecoder += fold_plane_seconds(jobs, nlay, tm);
    for (int l = 0; l < nlay; l++) {
        if (c->ps[l].err) return fail(WR_ERR_HIP, "upload of plane " + std::to_string(l) + " failed");
        tm->h2d_ms += (float)c->ps[l].copy_ms;
    }
    return WR_OK;
}

// ---- the tail that every decode driver takes, whatever filled the planes ----------------------------------------------------
// the end of a driver's kernel stage (cu_mu held): rc is the finisher's
int kernel_stage_end(wr_ctx* c, int rc)
{
    if (rc == WR_OK && hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "kernel launch failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the decoder's kernel stage failed on the device" + launch_describe(c));
    c->pool->last_stage_end.store(now());
    return rc;
}

// stage "down": `count` elements from where the finisher left them (d_f64, or d_f32 for an fp32 caller) to a host caller
int result_down(wr_ctx* c, const FieldRef& fld, const void* d_f64, const void* d_f32, size_t count, wr_timings* local)
{
    if (fld.host) {
        if (int rc = xfer_field(c, &c->x_field, fld.host, d_f64, count * sizeof(double), kDown)) return rc;
        local->d2h_ms = (float)c->x_field.ms;
    } else if (fld.host_f32) {
        if (int rc = xfer_field(c, &c->x_field, fld.host_f32, d_f32, count * sizeof(float), kDown)) return rc;
        local->d2h_ms = (float)c->x_field.ms;
    }
    return WR_OK;
}

// quant_ms and transform_ms of a finisher that ran once: its ev_a / ev_b / ev_c
int finisher_ms(wr_ctx* c, wr_timings* local)
{
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b)); local->quant_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_b, c->ev_c)); local->transform_ms = ms;
    return WR_OK;
}

// The tail of a segmented decode call: the result to a host caller, then the call's timings.  events: quant_ms and transform_ms
// are the finisher's events (a finisher that ran more than once has summed them itself).
int finish_call(wr_ctx* c, const FieldRef& fld, const void* d_f64, const void* d_f32, size_t count, bool events, double t0, double t_coded, double t_phase,
                wr_timings* local, wr_timings* tm)
{
    if (int rc = result_down(c, fld, d_f64, d_f32, count, local)) return rc;
    if (events) if (int rc = finisher_ms(c, local)) return rc;
    local->total = now() - t0;
    local->gpu = now() - t_phase;
    local->wait = t_phase - t_coded;
    local->transfer = t_coded - t0;
    if (tm) *tm = *local;
    return WR_OK;
}

int encode_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, int wtflag, const Cutoff& cut, wr_enc_info* info,
                unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null field pointer");
    if (cut.mx < 1 || cut.my < 1 || cut.mz < 1 || !cut.vec) return fail(WR_ERR_ARG, "bad local cutoff description");
    std::lock_guard<std::mutex> lk(c->mu);
    if (fld.host_f32 && c->keep_residual)  // (the residual is fp64: narrowing it into the caller's field would lose bits)
        return fail(WR_ERR_UNSUPPORTED, "an fp32 field cannot take the residual back: wr_ctx_set_keep_residual(ctx, 0) for fp32 encodes");
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    wr_timings local; memset(&local, 0, sizeof local);
    // per-60000-symbol-block byte histograms, counted on the GPU next to the quantizer and shipped
    // with the plane, so that the host coder starts every block with its model ready
    const size_t hist_per_plane = (n / wrrc::kBlock + 1) * 256;
    DevPool* const pool = c->pool;

    int copy_failed[WR_NLAYMAX] = {0};
    Sem sem(encoder_threads());
    const int dev = c->device;
    c->pend_valid = false;  // planes a wr_decode_begin parked in this context do not survive an encode on it
    PlaneHold planes(c);  // before the workers: they are joined first when the call unwinds
    Workers workers;

    // The planes stay in device memory; a coder reads its plane through the plane's ring of pinned chunks
    // (PlaneStream).  With a coder thread for every possible plane, plane l's thread starts as soon as the plane is
    // complete on the device and its histograms are on the host.  With fewer (wr_set_threads), the planes are split into that many groups once
    // their number is known and each thread codes its group with the symbol loops interleaved.
    const bool pooled = wrrc::pool_threads() > 0;  // the process-wide coder pool codes the planes (wr_set_coder_pool)
    const bool per_plane = !pooled && encoder_threads() >= WR_NLAYMAX;
    wrrc::PlaneJob jobs[WR_NLAYMAX];  // what coding plane l means, whoever codes it
    wrrc::JobBatch batch;
    // Where a plane's coder writes (RefPlacement): the planes are placed in plane order, as their histograms arrive.
    std::mutex place_mu;
    unsigned placed = 0;
    RefPlacement placement;
    uint8_t* plane_out[WR_NLAYMAX] = {nullptr};
    auto hist_of = [&](unsigned l) { return c->h_hist + l * hist_per_plane; };
    // (callable from the coder threads: the histograms of plane k and of the planes before it have been sent off)
    auto place_plane = [&](unsigned k) -> uint8_t* {
        std::lock_guard<std::mutex> lk(place_mu);
        for (unsigned j = placed; j <= k; j++) {
            if (xfer_wait(&c->x_plane[j]) != WR_OK) copy_failed[j] = 1;
            (void)placement.place(c, j, copy_failed[j] ? nullptr : hist_of(j), n, data_enc, cap, &plane_out[j]);  // (refused: the plane is not coded)
            placed = j + 1;
        }
        return plane_out[k];
    };
    // jobs[k] once plane k's histograms are on the host; false (copy_failed[k]) if the plane cannot be coded
    auto prepare_job = [&](unsigned k) -> bool {
        if (xfer_wait(&c->x_plane[k]) != WR_OK) copy_failed[k] = 1;
        uint8_t* const dst = place_plane(k);
        if (!dst || copy_failed[k]) { copy_failed[k] = 1; return false; }
        ref_encode_job(c, k, n, hist_of(k), placement, dst, &jobs[k]);
        return true;
    };
    // a thread of this call codes planes l0 .. l1-1 (prepare: their jobs are not built yet)
    auto code_group = [&](unsigned l0, unsigned l1, bool prepare) {
        (void)hipSetDevice(dev);
        for (unsigned l = l0; l < l1 && prepare; l++)
            if (!prepare_job(l)) return;
        sem.acquire();
        wrrc::run_jobs(jobs + l0, (int)(l1 - l0));
        sem.release();
    };

    SlotNeed need;
    transform_need(nx, ny, nz, wtflag ? kWavLvl : 0, &need);
    if (fld.host || fld.host_f32) need.field_elems = n;
    need.hist_elems = hist_per_plane * WR_NLAYMAX;
    if (int rc = ensure_host_hist(c, hist_per_plane * WR_NLAYMAX)) return rc;

    int rc = WR_OK;
    double t_phase = 0, t_gpu_done = 0;
    unsigned planes_started = 0;
    try {
        SlotLease slot;
        if ((rc = slot.acquire(c, need)) != WR_OK) return rc;
        t_phase = now();
        // ---- stage "up": the field goes host -> device; the kernel stage is only claimed once it has arrived, so other calls
        // compute meanwhile
        FieldUpload up;
        if ((rc = upload_field(c, slot.get(), fld, nx, ny, nz, wtflag, &up)) != WR_OK) return rc;
        local.h2d_ms = up.ms;
        double* const d_fld = up.d_fld;
        double* resid = d_fld;
        auto hist_buf = [&](unsigned l) { return slot->hist + l * hist_per_plane; };
        auto after_quant = [&](unsigned l, bool hist_done) -> int {
            if (hist_done) return WR_OK;  // the quantizer wrote them on its way (k_quant_blk)
            // block histograms of plane l on the kernel stream, behind the read-back of the next plane's min/max
            launch_note(c, "hist", (int)l, slot->hist + l * hist_per_plane, n, nullptr, c->ps[l].ref);
            wrk::block_histograms(c->ps[l].ref, n, slot->hist + l * hist_per_plane, c->stream);
            return WR_OK;
        };
        // (a plane that has to wait for device memory gives the kernel stage up meanwhile: cu)
        StageLock cu(pool->cu_mu, std::defer_lock);
        // (the local-cutoff quantizer scatters into the plane by wavelet-space index: it wants one array)
        const bool one_array = cut.count() > 1;
        // pool: plane k goes to the workers once its histograms are on the host (they set off when it completed)
        unsigned handed = 0;  // planes that have a coder (a pool job or, if the pool refused, a thread of this call)
        unsigned ready = 0;   // planes whose histograms and first window are on their way to the host (plane_ready has run)
        auto submit_plane = [&](unsigned k) {
            if (handed >> k & 1) return;
            if (!prepare_job(k)) return;
            handed |= 1u << k;
            if (!wrrc::pool_submit(&jobs[k], 1, &batch))
                workers.v.emplace_back(code_group, k, k + 1, false);  // the pool was stopped meanwhile: a thread of this call codes the plane
        };
        auto plane_ready = [&](unsigned l, bool) -> int {
            // plane l and its histograms are complete on the device: the histograms go to pinned host memory, the
            // plane's first chunk sets off into its ring, and a coder thread waits for them
            if (ready >> l & 1) return WR_OK;  // (done early, by a later plane that had to wait for device memory: before_wait)
            ready |= 1u << l;
            const Piece pc = {c->h_hist + l * hist_per_plane, slot->hist + l * hist_per_plane, hist_per_plane * sizeof(uint16_t)};
            if (int r = xfer_start(c, &c->x_plane[l], &pc, 1, kDown)) return r;
            plane_prefetch(c, (int)l);
            planes_started = l + 1;
            if (per_plane) workers.v.emplace_back(code_group, l, l + 1, true);
            // the plane before this one is handed to the pool now (its histograms have had a quantizer launch's time to
            // arrive): its coder drains it while the stage goes on -- what a later plane of this call may be waiting for
            // if device memory is short (plane_prepare)
            if (pooled && l > 0) submit_plane(l - 1);
            return WR_OK;
        };
        // A plane that finds no device memory waits for chunks to come back -- and the planes this call has quantized before
        // it are chunks that can: with the stream synchronised (plane_buffer_wait) every one of them is complete, so they
        // all go to their coders before the wait begins instead of after the next quantizer launch.  (With fewer coder
        // threads than planes and no pool the coders only start when the number of planes is known: nothing drains early.)
        unsigned preparing = 0;
        const std::function<void()> before_wait = [&]() {
            for (unsigned k = 0; k < preparing; k++)
                if (plane_ready(k, false) != WR_OK) return;
            if (pooled) for (unsigned k = 0; k < preparing; k++) submit_plane(k);
        };
        auto plane_buf = [&](unsigned l) -> const wrk::PlaneRef* {
            preparing = l;
            return plane_prepare(c, (int)l, n, false, one_array, &cu, &before_wait) == WR_OK ? &c->ps[l].ref : nullptr;
        };
        {
            // ---- stage "kernels"
            cu.lock();
            clock_warmup(c, n);
            if (up.widen_from) wrk::widen_f32(up.widen_from, d_fld, n, c->stream);
            rc = encode_planes_core(c, slot.get(), d_fld, nx, ny, nz, wtflag, cut, plane_buf, hist_buf, info, &local, after_quant, plane_ready, &resid,
                                    up.d_f32);
            rc = encode_stage_end(c, rc, fld, resid, n, info);
            cu.unlock();
        }
        // ---- stage "down": the histograms were sent off as the planes completed; the residual follows them
        if (rc == WR_OK && c->keep_residual && info->nlay && fld.host) {
            rc = xfer_field(c, &c->x_field, fld.host, resid, n * sizeof(double), kDown);
        }
        // The slot's histogram buffer must not be reused before its downloads are done (the coder threads wait
        // for the same transfers; xfer_wait is safe to call from both sides).  With the coder pool, every plane
        // is handed over the moment its histograms are on the host.
        for (unsigned l = 0; l < planes_started; l++) {
            if (xfer_wait(&c->x_plane[l]) != WR_OK) copy_failed[l] = 1;
            if (pooled && rc == WR_OK && !copy_failed[l]) submit_plane(l);
        }
        t_gpu_done = now();
        // the slot goes back here: the planes are in device buffers of their own
    } catch (const std::exception& e) {
        workers.join();
        wrrc::pool_wait(&batch);
        return fail(WR_ERR_ARG, std::string("encode: ") + e.what());
    }
    if (pooled)
        wrrc::pool_wait(&batch);
    else if (rc == WR_OK && !per_plane && info->nlay) {
        try {
            const unsigned groups = std::min<unsigned>(info->nlay, (unsigned)encoder_threads());
            for (unsigned g = 0; g < groups; g++)
                workers.v.emplace_back(code_group, g * info->nlay / groups, (g + 1) * info->nlay / groups, true);
        } catch (const std::exception& e) {
            workers.join();
            return fail(WR_ERR_ARG, std::string("encode: ") + e.what());
        }
    }
    workers.join();
    if (rc) return rc;
    const double t_coded = now();
    size_t total = 0;
    if (int r = ref_stream_tail(c, jobs, info->nlay, [&](unsigned l) { return copy_failed[l] || c->ps[l].err; }, placement, data_enc, cap, wrtc::kTooLarge,
                                info->len_enc_vec, &total))
        return r;
    local.rangecoder = fold_plane_seconds(jobs, (int)info->nlay, &local);
    for (unsigned l = 0; l < info->nlay; l++) {
        local.d2h_ms += (float)(c->x_plane[l].ms + c->ps[l].copy_ms);
        if (verbose()) fputs(plane_log(c, (int)l, n, info, true, jobs[l].result).c_str(), stdout);  // wrappers.cpp:401-409, 430
    }
    info->ntot_enc = total;
    local.total = now() - t0;
    local.wait = t_phase - t0;
    local.gpu = t_gpu_done - t_phase;  // without the wait for a slot
    local.transfer = (t_coded - t_gpu_done) - local.rangecoder;
    if (local.transfer < 0) local.transfer = 0;
    if (tm) *tm = local;
    return WR_OK;
}

// mode: the whole decode; or only its host half (range decoding, every decoded chunk going straight to the plane's device
// buffer: no field buffer and no slot needed, wr_decode_begin); or only its device half on planes decoded before
// (wr_decode_finish_*)
enum DecodeMode { kDecodeWhole, kDecodeBegin, kDecodeFinish };

int decode_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                size_t data_len, wr_timings* tm, DecodeMode mode = kDecodeWhole)
{
    if (int rc = ctx_bind(c)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    if (mode == kDecodeFinish) {
        if (!c->pend_valid) return fail(WR_ERR_ARG, "wr_decode_finish without a wr_decode_begin on this context");
        info = &c->pend_info; nx = c->pend_nx; ny = c->pend_ny; nz = c->pend_nz;
    }
    // (a finish that is refused for its arguments leaves the begin pending: the caller may try again with a usable
    // pointer, and the parked planes are not orphaned)
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (mode != kDecodeBegin && fld.none()) return fail(WR_ERR_ARG, "null field pointer");
    if (mode == kDecodeFinish) c->pend_valid = false;
    // From here on the context's device planes go back on every way out, unless a begin parks them (a finish finds the
    // planes its begin parked; a begin or a whole decode discards what an earlier begin left).
    PlaneHold planes(c);
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    wr_timings local; memset(&local, 0, sizeof local);
    if (mode == kDecodeFinish) local = c->pend_tm;
    DevPool* const pool = c->pool;
    if (mode == kDecodeBegin) { c->pend_info = *info; c->pend_nx = nx; c->pend_ny = ny; c->pend_nz = nz; }
    if (info->ntot_enc == 0) {  // wrappers.cpp:462-469
        if (mode == kDecodeBegin) { c->pend_tm = local; c->pend_valid = true; if (tm) *tm = local; return WR_OK; }
        if (int rc = fill_constant(c, fld, n, info->midval)) return rc;
        local.total += now() - t0;
        if (tm) *tm = local;
        return WR_OK;
    }
    const int nlay = info->nlay;
    if (nlay < 1 || nlay > WR_NLAYMAX) return fail(WR_ERR_ARG, "nlay out of range");
    if (info->wlev != 0 && info->wlev != kWavLvl) return fail(WR_ERR_ARG, "wlev must be 0 or 4");
    const bool host_half = mode != kDecodeFinish, device_half = mode != kDecodeBegin;
    size_t off[WR_NLAYMAX + 1] = {0};
    if (int rc = plane_offsets(info, nlay, host_half ? data_len : 0, off)) return rc;
    double t_coded = t0;
    if (host_half) {
        c->pend_valid = false;  // whatever an earlier begin parked here is overwritten now
        g_stat[WR_STAT_EARLY_DECODES]++;
        if (int rc = ref_decode_planes(c, info, nlay, n, data_enc, off, "decode: ", &local)) return rc;
        t_coded = now();
        local.transfer = (t_coded - t0) - local.rangecoder;
        if (local.transfer < 0) local.transfer = 0;
    }
    for (int l = 0; l < nlay; l++)
        if (!c->ps[l].dev || c->ps[l].n != n) return fail(WR_ERR_ARG, "wr_decode_finish: the planes of the begin are gone");
    if (!device_half) {  // the planes wait in the context's device buffers for wr_decode_finish_*
        local.total = now() - t0;
        c->pend_tm = local;
        c->pend_valid = true;
        planes.keep = true;
        if (tm) *tm = local;
        return WR_OK;
    }
    if (host_half && verbose()) {  // wrappers.cpp:489, 503-510
        for (int l = 0; l < nlay; l++) fputs(plane_log(c, l, n, info, false, 0).c_str(), stdout);
        printf("Wavelet reconstruction...\n");
    }
    // the accumulate kernel consumes the planes in plane order; they are on the device already: no "up" stage
    SlotNeed need;
    transform_need(nx, ny, nz, info->wlev ? -kWavLvl : 0, &need);
    if (fld.host || fld.host_f32) need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    wrk::DequantParams p;
    if (int rc = dequant_params(info, nlay, n, [&](int l) { return c->ps[l].ref; }, &p)) return rc;
    launch_note(c, "dequant", nlay - 1, fld.dev ? (void*)fld.dev : (void*)slot->field, n, nullptr, p.q[nlay - 1]);
    double* d_fld = fld.dev ? fld.dev : slot->field;
    float* d_f32 = nullptr;  // fp32: where inverse_from_planes leaves the narrowed reconstruction
    int rc = WR_OK;
    {
        // ---- stage "kernels"
        StageLock cu(pool->cu_mu);
        clock_warmup(c, n);
        rc = kernel_stage_end(c, inverse_from_planes(c, slot.get(), d_fld, nx, ny, nz, (int)info->wlev, p, fld.host_f32 ? &d_f32 : nullptr));
    }
    if (rc) return rc;
    if ((rc = result_down(c, fld, d_fld, d_f32, n, &local)) != WR_OK) return rc;
    if ((rc = finisher_ms(c, &local)) != WR_OK) return rc;
    local.total += now() - t0;  // (a finish adds to what its begin took)
    local.gpu = now() - t_phase;  // without the wait for a slot
    local.wait = t_phase - t_coded;
    if (tm) *tm = local;
    return WR_OK;
}

}  // namespace

extern "C" {

int wr_encode_device(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, double tolrel,
                     wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.vec = &tolrel;
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_impl(c, f, nx, ny, nz, wtflag, cut, info, data_enc, cap, tm);
}

int wr_encode_device_local(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                           const double* cutoffvec, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                           wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_impl(c, f, nx, ny, nz, wtflag, cut, info, data_enc, cap, tm);
}

int wr_decode_device(wr_ctx* c, double* d_fld, int nx, int ny, int nz, const wr_enc_info* info,
                     const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return decode_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

int wr_encode_host(wr_ctx* c, double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                   const double* cutoffvec, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host = h_fld;
    return encode_impl(c, f, nx, ny, nz, wtflag, cut, info, data_enc, cap, tm);
}

int wr_decode_host(wr_ctx* c, double* h_fld, int nx, int ny, int nz, const wr_enc_info* info,
                   const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host = h_fld;
    return decode_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

int wr_decode_begin(wr_ctx* c, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                    wr_timings* tm)
{
    FieldRef none;
    return decode_impl(c, none, nx, ny, nz, info, data_enc, data_len, tm, kDecodeBegin);
}

int wr_decode_finish_host(wr_ctx* c, double* h_fld, wr_timings* tm)
{
    FieldRef f; f.host = h_fld;
    if (!h_fld) return fail(WR_ERR_ARG, "null field pointer");
    return decode_impl(c, f, 0, 0, 0, nullptr, nullptr, 0, tm, kDecodeFinish);
}

int wr_encode_host_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                       const double* cutoffvec, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);  // (read only: an fp32 encode never writes the residual back)
    return encode_impl(c, f, nx, ny, nz, wtflag, cut, info, data_enc, cap, tm);
}

int wr_decode_host_f32(wr_ctx* c, float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                       size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_fld;
    return decode_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

int wr_decode_finish_host_f32(wr_ctx* c, float* h_fld, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_fld;
    if (!h_fld) return fail(WR_ERR_ARG, "null field pointer");
    return decode_impl(c, f, 0, 0, 0, nullptr, nullptr, 0, tm, kDecodeFinish);
}

int wr_decode_finish_device(wr_ctx* c, double* d_fld, wr_timings* tm)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return decode_impl(c, f, 0, 0, 0, nullptr, nullptr, 0, tm, kDecodeFinish);
}

int wr_transform_host(wr_ctx* c, double* h_fld, int nx, int ny, int nz, int lvl)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, nullptr)) return rc;
    if (!h_fld) return fail(WR_ERR_ARG, "null field pointer");
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t n = (size_t)nx * ny * nz;
    SlotNeed need;
    transform_need(nx, ny, nz, lvl, &need);
    need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    DevPool* const pool = c->pool;
    {
        if (int rc = xfer_field(c, &c->x_field, slot->field, h_fld, n * sizeof(double), kUp)) return rc;
    }
    double* res = nullptr;
    {
        StageLock cu(pool->cu_mu);
        if (int rc = run_transform(c, slot.get(), slot->field, nx, ny, nz, lvl, &res)) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return xfer_field(c, &c->x_field, h_fld, res, n * sizeof(double), kDown);
}

}  // extern "C"
namespace {
// CPUs this process may use: its affinity mask, cut down to a cgroup CPU quota if there is one
int usable_cpus()
{
    cpu_set_t set;
    int n = 0;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n < 1) n = (int)std::thread::hardware_concurrency();
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "max 100000" or "<quota> <period>"
        char q[64]; double period = 0;
        if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const int k = (int)(atof(q) / period + 0.5);
            if (k >= 1 && k < n) n = k;
        }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}

size_t host_mem_available()
{
    size_t avail = 0;
    if (FILE* f = fopen("/proc/meminfo", "r")) {
        char line[256];
        while (fgets(line, sizeof line, f))
            if (strncmp(line, "MemAvailable:", 13) == 0) { avail = (size_t)strtoull(line + 13, nullptr, 10) * 1024; break; }
        fclose(f);
    }
    if (FILE* f = fopen("/sys/fs/cgroup/memory.max", "r")) {
        char q[64];
        if (fscanf(f, "%63s", q) == 1 && strcmp(q, "max") != 0) {
            const size_t lim = (size_t)strtoull(q, nullptr, 10);
            if (lim && (!avail || lim < avail)) avail = lim;
        }
        fclose(f);
    }
    return avail;
}
}  // namespace
extern "C" {

int wr_autotune_batch(size_t field_elems, int nfields)
{
    if (nfields < 1) nfields = 1;
    const int cpus = usable_cpus();
    if (nfields > 1 && cpus >= 2) wr_set_coder_pool(cpus, 0);
    // 1.5 fields in flight per CPU keep the pool's workers busy (a field spends part of its time in copies, kernels and
    // waiting for its slowest plane)
    long fit = (3L * cpus + 1) / 2;
    const double fb = 8.0 * (double)(field_elems ? field_elems : 1);
    // host: the caller's field and coded buffers plus the coder's output while it is produced: ~2.5 field sizes per call
    if (const size_t mem = host_mem_available()) { const long k = (long)(0.6 * (double)mem / (2.5 * fb)); if (k < fit) fit = k; }
    // device: three work-space slots of 2.2 field sizes; per call its quantized planes (1 byte per element and plane, 4-5
    // planes at the usual tolerances, 8 at most)
    int dev = 0;
    if (const char* e = getenv("WR_DEVICE")) dev = atoi(e);
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(dev) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const long k = (long)((0.9 * (double)free_b - 3 * 2.2 * fb) / (0.75 * fb));
        if (k < fit) fit = k;
    } else
        (void)hipGetLastError();
    if (fit > nfields) fit = nfields;
    return fit < 1 ? 1 : (int)fit;
}

int wr_bench_transform(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int lvl, int reps, double* ms_out)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_fld)) return rc;
    if (reps < 1) return fail(WR_ERR_ARG, "reps < 1");
    SlotNeed need;
    transform_need(nx, ny, nz, lvl, &need);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    StageLock cu(c->pool->cu_mu);
    double* res = nullptr;
    HIPCHK(hipEventRecord(c->ev_a, c->stream));
    for (int r = 0; r < reps; r++)
        if (int rc = run_transform(c, slot.get(), d_fld, nx, ny, nz, lvl, &res)) return rc;  // fused: result stays in scratch
    HIPCHK(hipEventRecord(c->ev_b, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(c->ev_b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
    *ms_out = (double)ms / reps;
    return WR_OK;
}

}  // extern "C"

// ---- segmented plane streams: the planes are coded and decoded by the GPU (wr_segcoder.hip) -------------------------------
// The format is wr_segcoder.h's.  These drivers replace the hand-off to the host coder (block histograms, plane windows,
// coder threads or pool, the admission gate) by coder kernels and whole-blob copies; transform, quantizer and the header
// scalars are encode_planes_core's / inverse_from_planes', shared with the reference-format path.
namespace {

// device memory of a segmented call, from the plane pool (its accounting, cap and reserve); goes back when the call ends,
// behind everything the context's stream still has queued
// the event pairs around the coder kernels of a call, one per plane (or plane index of a batch); they go with the call's buffers
struct PlaneEvents {
    hipEvent_t e[2 * WR_NLAYMAX] = {nullptr};
    PlaneEvents() = default;
    PlaneEvents(const PlaneEvents&) = delete;
    PlaneEvents& operator=(const PlaneEvents&) = delete;
    ~PlaneEvents() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
    hipEvent_t operator[](int k) const { return e[k]; }
    int create(int l) { for (int k = 2 * l; k < 2 * l + 2; k++) if (!e[k]) HIPCHK(hipEventCreate(&e[k])); return WR_OK; }
    double seconds(int l) const
    {
        float ms = 0;
        if (!e[2 * l] || hipEventElapsedTime(&ms, e[2 * l], e[2 * l + 1]) != hipSuccess) { (void)hipGetLastError(); return 0; }
        return ms * 1e-3;
    }
};

struct SegBufs {
    wr_ctx* c;
    DevPlanes::Buf stage, blob[WR_NLAYMAX], work[WR_NLAYMAX];
    DevPlanes::Buf perm, bricks;  // a blocked stream: one plane in stream order (every plane in turn), the brick list of a partial decode
    DevPlanes::Buf trial[3];      // an encode to an error bound / wr_seg_error_host: two work arrays of a trial, the copy of the field
    DevPlanes::Buf mask[3];       // a masked call: the mask bits (and the restore's counters), the mask coder's stage or work buffer, its blob
    hipStream_t also = nullptr;   // a second stream that uses these buffers (a masked call's mask coder): waited for before they go back
    PlaneEvents ev;
    explicit SegBufs(wr_ctx* ctx) : c(ctx) {}
    int coded_plane(int l, size_t cap) { blob[l] = plane_scratch(c, cap); return blob[l].p ? ev.create(l) : WR_ERR_HIP; }  // an encoder's blob and event pair
    SegBufs(const SegBufs&) = delete;
    SegBufs& operator=(const SegBufs&) = delete;
    ~SegBufs()
    {
        (void)hipStreamSynchronize(c->stream);
        if (also) (void)hipStreamSynchronize(also);
        if (stage.p) c->pool->planes.give(stage);
        if (perm.p) c->pool->planes.give(perm);
        if (bricks.p) c->pool->planes.give(bricks);
        for (DevPlanes::Buf& b : trial) if (b.p) c->pool->planes.give(b);
        for (DevPlanes::Buf& b : mask) if (b.p) c->pool->planes.give(b);
        for (int l = 0; l < WR_NLAYMAX; l++) {
            if (blob[l].p) c->pool->planes.give(blob[l]);
            if (work[l].p) c->pool->planes.give(work[l]);
        }
    }
};

// a coder's result slot: the blob's length, and whether a stream outgrew its bound
unsigned long long* seg_result_host(wr_ctx* c, int l) { return reinterpret_cast<unsigned long long*>(c->h_result + 8) + 2 * l; }
unsigned long long* seg_result_dev(wr_ctx* c, int l) { return reinterpret_cast<unsigned long long*>(c->h_result_dev + 8) + 2 * l; }

// ---- the stages of a segmented encode.  The drivers -- the single field, the batch, the segmented target of a transcode, the
// stage calls -- compose these and upload_field / encode_stage_end above; the decode stages follow further down.
// The parameters of a format as every entry point takes them: seg == 0 is WR_SEG_DEFAULT (nullptr: the call has no segment
// length).  strands == 0: WRS1 (brick == 0) or WRS2 with that brick edge (wr_blocked.h); otherwise WRS3 with that many
// strands, in the natural order (brick == 0) or the blocked one.  (Where 0 names a default, the entry point has put it in.)
int seg_format_params(unsigned* seg, unsigned brick, unsigned strands)
{
    if (seg && !*seg) *seg = WR_SEG_DEFAULT;
    if (seg && !wrseg::seg_ok(*seg)) return fail(WR_ERR_ARG, "segment length must be a multiple of 16 in [16, 59999]");
    if (brick && !wrblk::brick_ok(brick)) return fail(WR_ERR_ARG, "brick edge must be one of 8, 16, 32, 64");
    if (strands && !wrseg::strands_ok(strands, *seg)) return fail(WR_ERR_ARG, "strands must be one of 1, 2, 4, 8, 16, 32 with 16 * strands <= seg");
    return WR_OK;
}

// bytes that hold any blob of a plane of n symbols, rounded up to 16: wr_transcode.h's bound, which is the public one
size_t seg_blob_cap(size_t n, unsigned seg, unsigned brick, unsigned strands)
{
    wrtc::StreamFormat f;
    f.format = strands ? WR_FORMAT_WRS3 : brick ? WR_FORMAT_WRS2 : WR_FORMAT_WRS1; f.seg = seg; f.brick = brick; f.strands = strands;
    const size_t bound = wrtc::plane_bound(n, f);
    assert(bound == (strands ? wr_seg_bound_strands(n, seg, strands) : brick ? wr_seg_bound_blocked(n, seg) : wr_seg_bound(n, seg)));
    return (bound + 15) & ~(size_t)15;
}

const char* const kOutgrew = "a segment outgrew the segment bound";

// What the planes of a call are coded into; the two buffers serve every plane in turn (the context's stream orders the coders)
struct SegTarget {
    unsigned seg = 0, brick = 0, strands = 0;
    wrblk::Order od{};         // brick != 0: the blocked order of the planes
    size_t blob_cap = 0;
    uint8_t* stage = nullptr;  // the uncompacted streams of one plane
    uint8_t* perm = nullptr;   // brick != 0: one plane in stream order
};

// ... with its buffers from the plane pool, kept in bufs (a stream-order plane that bufs has already is taken as it is)
int seg_target(wr_ctx* c, SegBufs* bufs, size_t n, unsigned seg, unsigned brick, unsigned strands, const wrblk::Order& od, SegTarget* t)
{
    t->seg = seg; t->brick = brick; t->strands = strands; t->od = od;
    t->blob_cap = seg_blob_cap(n, seg, brick, strands);
    bufs->stage = plane_scratch(c, strands ? wrk::strand_stage_bytes(n, seg, strands) : wrk::seg_stage_bytes(n, seg));
    if (bufs->stage.p && brick && !bufs->perm.p) bufs->perm = plane_scratch(c, n);
    if (!bufs->stage.p || (brick && !bufs->perm.p)) return WR_ERR_HIP;
    t->stage = bufs->stage.p; t->perm = bufs->perm.p;
    return WR_OK;
}

// the coder kernels of one plane, its symbols in stream order: the blob into [blob, blob + cap), its length into result slot l
void seg_encode_launch(wr_ctx* c, const SegTarget& t, const wrk::PlaneRef& sym, size_t n, uint8_t* blob, size_t cap, int l)
{
    if (t.strands) wrk::strand_encode(sym, n, t.seg, t.strands, t.brick, t.stage, blob, cap, seg_result_dev(c, l), c->stream);
    else wrk::seg_encode(sym, n, t.seg, t.stage, blob, cap, seg_result_dev(c, l), c->stream, t.brick);
}

// Plane l of a pipeline call (cu_mu held) into its blob of t.blob_cap bytes, behind whatever the context's stream has queued
int seg_encode_plane(wr_ctx* c, const SegTarget& t, const wrk::PlaneRef& plane, size_t n, int l, uint8_t* blob, const PlaneEvents& ev)
{
    launch_note(c, "seg_encode", l, blob, n, t.stage, plane);
    HIPCHK(hipEventRecord(ev[2 * l], c->stream));
    wrk::PlaneRef sym = plane;
    if (t.brick) {
        if (!wrk::plane_reorder(sym, t.perm, t.od, false, nullptr, 0, c->stream)) return fail(WR_ERR_ARG, "too many bricks");
        sym = wrk::plane_ref(t.perm);
    }
    seg_encode_launch(c, t, sym, n, blob, t.blob_cap, l);
    HIPCHK(hipEventRecord(ev[2 * l + 1], c->stream));
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "segmented coder launch failed" + launch_describe(c));
    return WR_OK;
}

// Stage "down", first half: the result slots of nlay planes (res_of(l)), once the stream has drained.  Every blob must have
// stayed inside blob_cap; lens[l] and *total.  who: put in front of the message ("field 3: " in a batch)
template <class ResOf>
int seg_coded_lengths(int nlay, size_t blob_cap, ResOf res_of, size_t* lens, size_t* total, const std::string& who = std::string())
{
    *total = 0;
    for (int l = 0; l < nlay; l++) {
        const unsigned long long* const res = res_of(l);
        if (res[1] || res[0] > blob_cap) return fail(WR_ERR_HIP, who + "internal: plane " + std::to_string(l) + ": " + kOutgrew);
        lens[l] = res[0];
        *total += res[0];
    }
    return WR_OK;
}

// ... second half: a copy per blob, behind one another at `out`; the coder seconds add to tm's (a transcode's source half's)
int seg_download_blobs(wr_ctx* c, const SegBufs& bufs, int nlay, const size_t* lens, unsigned char* out, wr_timings* tm)
{
    size_t at = 0;
    for (int l = 0; l < nlay; l++) {
        if (int rc = xfer_field(c, &c->x_field, out + at, bufs.blob[l].p, lens[l], kDown)) return rc;
        tm->d2h_ms += (float)c->x_field.ms;
        at += lens[l];
        const double sec = bufs.ev.seconds(l);
        tm->plane_coder_s[l] += sec;
        tm->rangecoder += sec;
    }
    return WR_OK;
}

// ---- the search of an encode to a byte budget (include/waverange_amd.h; the grid and the bound: wr_budget.h) ----------------
// Only the last plane depends on the tolerance: plane l is cut with the full step (hi - lo) / 255 of its residual until that
// falls below tolabs, and is then the last, cut with tolabs.  So the grid falls into one interval per plane count: with
// a_l the finest point at which plane l is the last one, plane l is last on [a_l, a_{l-1} - 1] (plane 0 up to the grid's end),
// and there B(g) = (the bounds of the full planes 0 .. l-1) + the bound of plane l cut with tolabs(g).  The size probe gives
// the second term for kProbeK points of the interval in one pass over the coefficients, and the first term is the probe's
// number for the full step, so the search walks down the planes and never quantizes, let alone codes, a plane to look.
//
// At plane l:  pass 1 probes points spread over [a_l, top] (both ends among them) and the full step.
//   B(a_l) > max_bytes:   a point that fits lies above (B(top) fits: for plane 0 the call fails otherwise, for the others
//                         pass 1 was only kept because it does), so a (kProbeK + 1)-section finds neighbours g - 1, g with
//                         B(g - 1) > max_bytes >= B(g).  Plane l is the last, at t(g).
//   B(a_l) fits, a_l is g_min:  done, at g_min.
//   B(a_l) fits otherwise:  finer points keep plane l full -- but whether one of them fits is plane l + 1's business, and
//                         the answer "none" would make a_l the result, with plane l the LAST plane.  So plane l is not
//                         declared full before pass 1 of plane l + 1 has run (on the residual range the full-step
//                         candidate's min/max gives) and B(a_l - 1) is known to fit.  Then plane l goes to the quantizer
//                         and its coder kernels start, under the remaining probes of plane l + 1, whose pass 1 is kept.
// The probes run on a stream of their own so that they do not queue behind those coder kernels; they only read the
// coefficient array, which nothing writes while the loop runs (no residual is kept).  The pick is called with the context's
// stream idle but for coder kernels: the quantizer's partials and its result slot are free for the probe's min/max.
struct BudgetSearch {
    // what the caller asks for
    size_t max_bytes = 0;
    int g_min = 0;
    // a masked call: the mask blob's exact length, already taken off max_bytes (reserve() below); it only enters the message
    size_t mask_len = 0, budget = 0;  // (budget: max_bytes as the caller gave it)
    bool masked = false;
    // what comes out
    int g = -1;
    size_t bound = 0;
    int passes = 0;

    wr_ctx* c = nullptr;
    hipStream_t st = nullptr;
    size_t n = 0, nseg = 0;
    unsigned seg = 0;
    size_t full_sum = 0;           // the bounds of the full planes before the current one
    int top = wrbud::kGMax;        // the coarsest point at which the current plane is the last
    bool fits_above = false;       // a point above the current interval's bottom is known to fit
    struct Pass1 {
        bool valid = false, empty = false;
        unsigned ilay = 0;
        double lo = 0, hi = 0;     // the residual range it was made for
        int a = 0, top = 0;
        size_t full_sum = 0;
        std::vector<std::pair<int, size_t>> B;  // ascending g
        size_t full_bound = 0;     // the plane cut with the full step
        double next_lo = 0, next_hi = 0;  // the range that leaves
        bool has_full = false;
    } kept;

    BudgetSearch() = default;
    BudgetSearch(const BudgetSearch&) = delete;
    BudgetSearch& operator=(const BudgetSearch&) = delete;
    ~BudgetSearch() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }

    static int tables(wr_ctx* c)
    {
        if (c->d_bound_tab) return WR_OK;
        const wrbud::Tables& t = wrbud::tables();
        uint32_t* tab = nullptr;
        HIPCHK(hipMalloc(&tab, wrbud::kTabWords * sizeof(uint32_t)));
        if (hipMemcpy(tab, t.words.data(), wrbud::kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError(); (void)hipFree(tab);
            return fail(WR_ERR_HIP, "the size bound's table could not be copied to the device");
        }
        if (!c->d_bound_tot) HIPCHK(hipMalloc(&c->d_bound_tot, wrk::kProbeK * sizeof(unsigned long long)));
        c->d_bound_tab = tab;
        return WR_OK;
    }
    static unsigned long long* totals_host(wr_ctx* c) { return reinterpret_cast<unsigned long long*>(c->h_result + 8 + 2 * WR_NLAYMAX); }

    int begin(wr_ctx* ctx, size_t count, unsigned s)
    {
        c = ctx; n = count; seg = s; nseg = wrseg::seg_count(n, seg);
        if (int rc = tables(c)) return rc;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return WR_OK;
    }

    // a masked call: B(g) + len <= max_bytes is B(g) <= max_bytes - len; a budget the blob alone uses up leaves 0 for the planes,
    // which no tolerance fits (a blob's header and index are never empty), so the first pick names the smallest budget
    void reserve(size_t len)
    {
        masked = len != 0; mask_len = len; budget = max_bytes;
        max_bytes = max_bytes > len ? max_bytes - len : 0;
    }

    // one launch: the candidates' segment sums into out[0, cd.n) (the blob's header and index added)
    static int launch(wr_ctx* c, hipStream_t st, const double* d_coef, size_t n, unsigned seg, const wrk::QuantPrev& prev, const wrk::ProbeCands& cd,
                      bool want_minmax, size_t* out)
    {
        wrk::quant_probe(d_coef, n, seg, prev, cd, want_minmax, c->d_bound_tab, wrbud::tables().fixed, c->d_bound_tot, c->d_partial, c->h_result_dev, st);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "size probe launch failed");
        HIPCHK(hipMemcpyAsync(totals_host(c), c->d_bound_tot, wrk::kProbeK * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const size_t over = wrbud::blob_overhead(wrseg::seg_count(n, seg));
        for (int k = 0; k < cd.n; k++) out[k] = over + (size_t)totals_host(c)[k];
        return WR_OK;
    }

    // up to m points of [a, b], both ends among them, ascending
    static std::vector<int> spread(int a, int b, int m)
    {
        std::vector<int> v;
        if (b - a + 1 <= m) { for (int x = a; x <= b; x++) v.push_back(x); return v; }
        for (int i = 0; i < m; i++) {
            const int x = a + (int)(((long long)(b - a) * i + (m - 1) / 2) / (m - 1));
            if (v.empty() || x > v.back()) v.push_back(x);
        }
        return v;
    }

    // B at the points gs (fewer than kProbeK with the full step, kProbeK without) of plane ilay's interval
    int eval(unsigned ilay, double lo, double hi, const wrk::QuantPrev& prev, const double* d_coef, const Prologue& p, size_t sum_before,
             const std::vector<int>& gs, bool with_full, bool want_minmax, Pass1* out)
    {
        wrk::ProbeCands cd;
        if (with_full) {
            const PlaneStep s = plane_step(lo, hi, 0.0, ilay);
            cd.aopt[0] = s.aopt; cd.bopt[0] = s.bopt; cd.deps0 = s.deps; cd.minval0 = s.minval;
            cd.n = 1;
        }
        for (int gk : gs) {
            const PlaneStep s = plane_step(lo, hi, abs_tolerance(wrbud::grid_tol(gk), p), ilay);
            cd.aopt[cd.n] = s.aopt; cd.bopt[cd.n] = s.bopt;
            cd.n++;
        }
        size_t got[wrk::kProbeK];
        if (int rc = launch(c, st, d_coef, n, seg, prev, cd, with_full && want_minmax, got)) return rc;
        passes++;
        int k = 0;
        if (with_full) {
            out->full_bound = got[k++];
            out->has_full = true;
            if (want_minmax) { out->next_lo = c->h_result[0]; out->next_hi = c->h_result[1]; }
        }
        for (int gk : gs) out->B.emplace_back(gk, sum_before + got[k++]);
        std::sort(out->B.begin(), out->B.end());
        return WR_OK;
    }

    int pass1(unsigned ilay, double lo, double hi, const wrk::QuantPrev& prev, const double* d_coef, const Prologue& p, size_t sum_before, int top_g, Pass1* out)
    {
        *out = Pass1();
        out->valid = true; out->ilay = ilay; out->lo = lo; out->hi = hi; out->top = top_g; out->full_sum = sum_before;
        auto last_at = [&](int gk) { return plane_step(lo, hi, abs_tolerance(wrbud::grid_tol(gk), p), ilay).last; };
        if (top_g < g_min || !last_at(top_g)) {  // the plane is full wherever the search may still go
            out->empty = true;
            return eval(ilay, lo, hi, prev, d_coef, p, sum_before, std::vector<int>(), true, false, out);
        }
        int a = top_g;  // the finest point of [g_min, top] at which the plane is the last (tolabs does not fall as g grows)
        if (last_at(g_min)) a = g_min;
        else {
            int below = g_min;
            while (a - below > 1) {
                const int mid = (a + below) / 2;
                if (last_at(mid)) a = mid;
                else below = mid;
            }
        }
        out->a = a;
        const bool with_full = a > g_min && ilay + 1 < (unsigned)WR_NLAYMAX;
        return eval(ilay, lo, hi, prev, d_coef, p, sum_before, spread(a, top_g, wrk::kProbeK - (with_full ? 1 : 0)), with_full, true, out);
    }

    static size_t at(const Pass1& q, int gk)
    {
        for (const auto& e : q.B) if (e.first == gk) return e.second;
        return ~(size_t)0;
    }

    int choose(int gk, size_t b, const Prologue& p, double* tolabs)
    {
        g = gk; bound = b;
        *tolabs = abs_tolerance(wrbud::grid_tol(gk), p);
        return WR_OK;
    }

    int pick(unsigned ilay, double lo, double hi, const wrk::QuantPrev& prev, const double* d_coef, const Prologue& p, double* tolabs)
    {
        if ((uintptr_t)d_coef & 15) return fail(WR_ERR_ARG, "an encode to a byte budget needs a 16-byte aligned coefficient array");
        Pass1 cur;
        // (== on the range: the probe's min/max and the quantizer's are the same values but for the sign of a zero)
        if (kept.valid && kept.ilay == ilay && kept.lo == lo && kept.hi == hi) cur = kept;
        else if (int rc = pass1(ilay, lo, hi, prev, d_coef, p, full_sum, top, &cur)) return rc;
        kept = Pass1();
        if (cur.empty) {
            if (ilay + 1 >= (unsigned)WR_NLAYMAX) return fail(WR_ERR_HIP, "internal: the budget search ran out of planes");
            full_sum += cur.full_bound;
            *tolabs = 0;
            return WR_OK;
        }
        const size_t b_top = at(cur, cur.top);
        if (!fits_above && b_top > max_bytes) {
            if (masked)
                return fail(WR_ERR_BUDGET, "the budget leaves " + std::to_string(max_bytes) + " bytes beside the mask blob of " + std::to_string(mask_len) +
                                               " bytes, below what the coarsest tolerance takes: " + std::to_string(mask_len + b_top) +
                                               " bytes is the smallest budget that would do");
            return fail(WR_ERR_BUDGET, "the budget of " + std::to_string(max_bytes) + " bytes is below what the coarsest tolerance takes: " +
                                           std::to_string(b_top) + " bytes is the smallest budget that would do");
        }
        if (b_top > max_bytes) return fail(WR_ERR_HIP, "internal: the budget search lost the point that fits");
        fits_above = true;
        const size_t b_a = at(cur, cur.a);
        if (b_a <= max_bytes) {
            if (cur.a == g_min) return choose(cur.a, b_a, p, tolabs);
            if (!cur.has_full) return fail(WR_ERR_HIP, "internal: the budget search has no bound of the full plane");
            // does a finer point fit?  pass 1 of the next plane, on what the full step leaves
            const PlaneStep s = plane_step(lo, hi, 0.0, ilay);
            wrk::QuantPrev next_prev = prev;
            if (next_prev.n >= wrk::kQuantPrevMax) return fail(WR_ERR_HIP, "internal: the budget search ran out of planes");
            next_prev.push(s.aopt, s.bopt, s.deps, s.minval);
            Pass1 nxt;
            if (int rc = pass1(ilay + 1, cur.next_lo, cur.next_hi, next_prev, d_coef, p, full_sum + cur.full_bound, cur.a - 1, &nxt)) return rc;
            if (nxt.empty) return fail(WR_ERR_HIP, "internal: the budget search found no tolerance for plane " + std::to_string(ilay + 1));
            if (at(nxt, nxt.top) > max_bytes) return choose(cur.a, b_a, p, tolabs);  // B(a - 1) does not fit: a is tight
            full_sum += cur.full_bound;
            top = cur.a - 1;
            kept = nxt;
            *tolabs = 0;
            return WR_OK;
        }
        // B(a) does not fit, B(top) does: neighbours bad, good between them
        int bad = cur.a, good = cur.top;
        size_t b_good = b_top;
        for (size_t i = cur.B.size(); i-- > 0;) {
            if (cur.B[i].second > max_bytes) { bad = cur.B[i].first; break; }
            good = cur.B[i].first; b_good = cur.B[i].second;
        }
        while (good - bad > 1) {
            Pass1 more;
            if (int rc = eval(ilay, lo, hi, prev, d_coef, p, full_sum, spread(bad + 1, good - 1, wrk::kProbeK), false, false, &more)) return rc;
            for (size_t i = more.B.size(); i-- > 0;) {
                if (more.B[i].second > max_bytes) { bad = more.B[i].first; break; }
                good = more.B[i].first; b_good = more.B[i].second;
            }
        }
        return choose(good, b_good, p, tolabs);
    }
};

// PSNR = 20 log10(range / R), +inf for R = 0 (include/waverange_amd.h)
inline double psnr_of(double range, double rms) { return rms == 0 ? INFINITY : 20.0 * log10(range / rms); }

void fill_error_stats(wr_error_stats* o, double max_abs, double bad, double sumsq, size_t n, double lo, double hi)
{
    o->max_abs = max_abs; o->sumsq = sumsq;
    o->rms = sqrt(sumsq / (double)n);
    o->lo = lo; o->hi = hi;
    o->psnr = psnr_of(hi - lo, o->rms);
    o->nonfinite = (unsigned long long)bad;
}

// The measuring calls on a constant record: the reconstruction is midval everywhere (fill_constant), so the compare runs on the
// host over the field as the caller holds it.  bits != nullptr: the record's mask, and only the samples whose bit is clear are
// compared, `count` of them.  *err_out = max |field - midval|; stats_out (or nullptr) takes S by a compensated sum (Neumaier),
// whose error does not grow with n, and lo and hi of the compared samples.
int constant_error_stats(const FieldRef& fld, size_t n, double midval, const unsigned char* bits, size_t count, double* err_out, wr_error_stats* stats_out,
                         unsigned long long* defined_out)
{
    double mx = 0;
    size_t bad = 0;
    auto undef = [&](size_t j) { return bits && ((bits[j >> 3] >> (j & 7)) & 1); };
    if (defined_out) *defined_out = count;
    for (size_t j = 0; j < n; j++) {
        if (undef(j)) continue;
        const double d = fld.host ? fabs(fld.host[j] - midval) : fabs((double)fld.host_f32[j] - (double)(float)midval);
        if (d <= DBL_MAX) mx = d > mx ? d : mx;
        else bad++;
    }
    if (stats_out) {
        double sum = 0, comp = 0, lo = NAN, hi = NAN;
        for (size_t j = 0; j < n; j++) {
            if (undef(j)) continue;
            const double v = fld.host ? fld.host[j] : (double)fld.host_f32[j];
            lo = fmin(lo, v); hi = fmax(hi, v);
            const double d = fld.host ? v - midval : v - (double)(float)midval;
            if (!(fabs(d) <= DBL_MAX)) continue;
            const double q = d * d, t = sum + q;
            comp += sum >= q ? (sum - t) + q : (q - t) + sum;
            sum = t;
        }
        if (sum <= DBL_MAX) sum += comp;
        fill_error_stats(stats_out, mx, (double)bad, sum, count, lo, hi);
    }
    if (bad) return fail(WR_ERR_ARG, std::to_string(bad) + " difference(s) between the field and the reconstruction are not finite");
    *err_out = mx;
    return WR_OK;
}

// ---- the search of an encode to an error bound (include/waverange_amd.h) ------------------------------------------------------
// E(g) is measured, not bounded: a trial at g forms the reconstruction the decoder would return and compares it with the field.
// The planes of a trial are never written.  As above only the last plane depends on the tolerance: the residual range plane l
// is cut from, given that planes 0 .. l-1 were full, is the same at every tolerance (range[l]: the size probe's min/max of the
// full-step candidate, once per depth), so the host replays the quantizer loop's scalars at tolabs(g) and one kernel
// (requant_accum) turns the coefficient array into the decoder's coefficient sum.  Then the decoder's own inverse stage, as
// inverse_from_planes runs it, and the compare; one read-back per trial.
// The whole search runs at the pick of plane 0, on the context's stream, before anything is quantized: the loop then runs at
// tolabs(g) exactly as the plain call does, which is what makes the stream the plain call's and codes every plane once.
// The walk over the grid is wrbud::bounded_walk (wr_budget.h: plain host code, fuzzed on its own), from wrbud::bounded_start.
// An encode to an RMS or PSNR target (wr_encode_*_seg_quality) is the same search with another functional: norm != WR_NORM_MAX
// makes a trial's compare wrk::err_stats, and what the walk sees is R(g) = sqrt(S(g) / n) against max_err, the RMS target (a
// PSNR target is converted once, in run(), from the prologue's range).  The walk does not know the difference.
struct BoundedSearch {
    // what the caller asks for
    double max_err = 0;
    int g_min = 0;
    int norm = WR_NORM_MAX;  // what max_err bounds: the largest |difference|, or R
    double psnr_db = 0;      // WR_NORM_PSNR: the target, from which run() makes max_err
    bool quality = false;    // one of the quality calls: their counter, their words in the messages
    // what comes out
    int g = -1;
    double err = 0;
    int trials = 0;
    double ms[3] = {0, 0, 0};
    struct Stats { double max_abs = 0, bad = 0, sumsq = 0, rms = 0; };
    std::map<int, Stats> seen;  // norm != WR_NORM_MAX: what the compare returned at every point formed
    double range = 0;           // hi - lo of the field

    wr_ctx* c = nullptr;
    Slot* slot = nullptr;
    int nx = 0, ny = 0, nz = 0, wlev = 0;
    size_t n = 0;
    unsigned seg = 0;
    const double* orig = nullptr;    // the field as the caller gave it, on the device, or
    const float* orig_f32 = nullptr;
    // a masked call with an undefined sample: the split's bits and nd = n - undefined, the size of D.  The compares are then the
    // masked kernel's (E_D, S_D, R_D = sqrt(S_D / nd)): whatever the field's copy and the reconstruction hold where a bit is set
    // -- the caller's NaNs or the pad -- is never read.  nullptr: the plain compares, the plain call's bits.
    const uint8_t* mask_bits = nullptr;
    unsigned long long nd = 0;
    double *w1 = nullptr, *w2 = nullptr;
    const double* d_coef = nullptr;
    Prologue p{};
    int nrange = 0;
    double rlo[WR_NLAYMAX], rhi[WR_NLAYMAX];  // range[l], known for l < nrange

    static double* result_host(wr_ctx* c) { return c->h_result + 8 + 2 * WR_NLAYMAX + wrk::kProbeK; }
    static double* result_dev(wr_ctx* c) { return c->h_result_dev + 8 + 2 * WR_NLAYMAX + wrk::kProbeK; }
    // the masked compare's count of compared samples: behind the mask coder's record (mask_result_host: + 5, + 6), which a masked
    // call's second stream may write while a trial runs
    static unsigned long long* defined_host(wr_ctx* c) { return reinterpret_cast<unsigned long long*>(c->h_result + 8 + 2 * WR_NLAYMAX + wrk::kProbeK + 7); }
    static unsigned long long* defined_dev(wr_ctx* c) { return reinterpret_cast<unsigned long long*>(c->h_result_dev + 8 + 2 * WR_NLAYMAX + wrk::kProbeK + 7); }

    // max |a - b| and the count of differences that are not finite, read back
    template <class T>
    static int compare(wr_ctx* c, const T* a, const T* b, size_t n, double* mx, double* bad)
    {
        wrk::linf_count(a, b, n, c->d_partial, result_dev(c), c->stream);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "compare launch failed");
        HIPCHK(hipEventRecord(c->ev_d, c->stream));
        HIPCHK(hipEventSynchronize(c->ev_d));
        *mx = result_host(c)[0]; *bad = result_host(c)[1];
        return WR_OK;
    }

    // the same with the sum of the squares of the finite differences, S, and R = sqrt(S / n) (wrk::err_stats)
    template <class T>
    static int compare_stats(wr_ctx* c, const T* a, const T* b, size_t n, Stats* st)
    {
        wrk::err_stats(a, b, n, c->d_partial, result_dev(c) + 2, c->stream);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "compare launch failed");
        HIPCHK(hipEventRecord(c->ev_d, c->stream));
        HIPCHK(hipEventSynchronize(c->ev_d));
        const double* r = result_host(c) + 2;
        st->max_abs = r[0]; st->bad = r[1]; st->sumsq = r[2];
        st->rms = sqrt(st->sumsq / (double)n);
        return WR_OK;
    }

    // the same over the samples whose bit is clear (wrk::err_stats_masked): R = sqrt(S / defined), defined read back with the rest
    template <class T>
    static int compare_stats_masked(wr_ctx* c, const T* a, const T* b, size_t n, const uint8_t* bits, Stats* st, unsigned long long* defined)
    {
        wrk::err_stats_masked(a, b, n, bits, c->d_partial, result_dev(c) + 2, defined_dev(c), c->stream);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "compare launch failed");
        HIPCHK(hipEventRecord(c->ev_d, c->stream));
        HIPCHK(hipEventSynchronize(c->ev_d));
        const double* r = result_host(c) + 2;
        st->max_abs = r[0]; st->bad = r[1]; st->sumsq = r[2];
        *defined = *defined_host(c);
        st->rms = sqrt(st->sumsq / (double)*defined);
        return WR_OK;
    }

    // wr_dev_err_stats_masked / _f32: the masked compare alone, as a stage call
    template <class T>
    static int stage_stats_masked(wr_ctx* c, const T* d_a, const T* d_b, size_t n, const unsigned char* d_bits, wr_error_stats* stats,
                                  unsigned long long* defined)
    {
        if (int rc = ctx_bind(c)) return rc;
        if (!stats || !d_a || !d_b || !d_bits || !defined) return fail(WR_ERR_ARG, "null pointer");
        if (!n) return fail(WR_ERR_ARG, "empty array");
        std::lock_guard<std::mutex> lk(c->mu);
        StageLock cu(c->pool->cu_mu);
        Stats st;
        if (int rc = compare_stats_masked(c, d_a, d_b, n, d_bits, &st, defined)) return rc;
        fill_error_stats(stats, st.max_abs, st.bad, st.sumsq, (size_t)*defined, NAN, NAN);
        stats->psnr = NAN;
        return WR_OK;
    }

    // wr_dev_err_stats / _f32: the compare alone, as a stage call
    template <class T>
    static int stage_stats(wr_ctx* c, const T* d_a, const T* d_b, size_t n, wr_error_stats* stats)
    {
        if (int rc = ctx_bind(c)) return rc;
        if (!stats || !d_a || !d_b) return fail(WR_ERR_ARG, "null pointer");
        if (!n) return fail(WR_ERR_ARG, "empty array");
        std::lock_guard<std::mutex> lk(c->mu);
        StageLock cu(c->pool->cu_mu);
        Stats st;
        if (int rc = compare_stats(c, d_a, d_b, n, &st)) return rc;
        fill_error_stats(stats, st.max_abs, st.bad, st.sumsq, n, NAN, NAN);
        stats->psnr = NAN;
        return WR_OK;
    }

    std::string who() const { return quality ? "an encode to a quality target" : "an encode to an error bound"; }

    int nonfinite_field(const std::string& what)
    {
        if (mask_bits) return fail(WR_ERR_ARG, what);  // (a sample that is not finite is undefined: the field is not to blame)
        double mx = 0, bad = 0;
        if (int rc = orig_f32 ? compare(c, orig_f32, orig_f32, n, &mx, &bad) : compare(c, orig, orig, n, &mx, &bad)) return rc;
        if (bad > 0) return fail(WR_ERR_ARG, who() + " needs a finite field: " + std::to_string((unsigned long long)bad) +
                                                 " sample(s) are a NaN or an infinity");
        return fail(WR_ERR_ARG, what);
    }

    // range[l + 1]: what the full step of plane l leaves, the planes before being `prev`
    int next_range(int l, const wrk::QuantPrev& prev, const PlaneStep& s)
    {
        if (int rc = BudgetSearch::tables(c)) return rc;
        wrk::ProbeCands cd;
        cd.n = 1; cd.aopt[0] = s.aopt; cd.bopt[0] = s.bopt; cd.deps0 = s.deps; cd.minval0 = s.minval;
        size_t unused[wrk::kProbeK];
        if (int rc = BudgetSearch::launch(c, c->stream, d_coef, n, seg, prev, cd, true, unused)) return rc;
        rlo[l + 1] = c->h_result[0]; rhi[l + 1] = c->h_result[1];
        nrange = l + 2;
        return WR_OK;
    }

    // E(gk), formed on the device
    int eval(int gk, double* e)
    {
        const double tolabs = abs_tolerance(wrbud::grid_tol(gk), p);
        wrk::QuantPrev prev;
        PlaneStep s;
        for (int l = 0;; l++) {  // (plane WR_NLAYMAX - 1 is the last whatever its step: prev never outgrows kQuantPrevMax)
            s = plane_step(rlo[l], rhi[l], tolabs, (unsigned)l);
            if (s.last) break;
            if (l + 1 >= nrange) if (int rc = next_range(l, prev, s)) return rc;
            prev.push(s.aopt, s.bopt, s.deps, s.minval);
        }
        const bool fused = wlev == kWavLvl && use_fused(nx, ny, nz, -kWavLvl);
        if (fused) if (const char* why = wrk::fused_prepare()) return fail(WR_ERR_HIP, why);
        HIPCHK(hipEventRecord(c->ev_a, c->stream));
        wrk::requant_accum(d_coef, n, prev, s.aopt, s.bopt, s.deps, s.minval, w1, c->stream);
        HIPCHK(hipEventRecord(c->ev_b, c->stream));
        // the decoder's inverse stage (inverse_from_planes), the sum in w1 and w2 in the place of the slot's arrays
        const double* rec = w1;
        const float* rec_f32 = reinterpret_cast<const float*>(w2);
        if (fused && orig_f32) wrk::transform_inv_fused_f32(w1, reinterpret_cast<float*>(w2), w2, slot->lowbuf, nx, ny, nz, c->stream);
        else if (fused) { wrk::transform_inv_fused(w1, w2, slot->lowbuf, nx, ny, nz, c->stream); rec = w2; }
        else {
            if (wlev) wrk::transform(w1, w2, nx, ny, nz, -wlev, c->stream);
            if (orig_f32) wrk::narrow_f64(w1, reinterpret_cast<float*>(w2), n, c->stream);
        }
        HIPCHK(hipEventRecord(c->ev_c, c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "a trial's kernel launch failed");
        double bad = 0;
        if (mask_bits) {  // every norm: one kernel knows the mask
            Stats st;
            unsigned long long defined = 0;
            if (int rc = orig_f32 ? compare_stats_masked(c, orig_f32, rec_f32, n, mask_bits, &st, &defined)
                                  : compare_stats_masked(c, orig, rec, n, mask_bits, &st, &defined)) return rc;
            if (defined != nd) return fail(WR_ERR_HIP, "internal: the masked compare and the split disagree on the count of defined samples");
            if (norm != WR_NORM_MAX) seen[gk] = st;
            *e = norm == WR_NORM_MAX ? st.max_abs : st.rms; bad = st.bad;
        } else if (norm == WR_NORM_MAX) {
            if (int rc = orig_f32 ? compare(c, orig_f32, rec_f32, n, e, &bad) : compare(c, orig, rec, n, e, &bad)) return rc;
        } else {
            Stats st;
            if (int rc = orig_f32 ? compare_stats(c, orig_f32, rec_f32, n, &st) : compare_stats(c, orig, rec, n, &st)) return rc;
            seen[gk] = st;
            *e = st.rms; bad = st.bad;
        }
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, c->ev_a, c->ev_b)); ms[0] += t;
        HIPCHK(hipEventElapsedTime(&t, c->ev_b, c->ev_c)); ms[1] += t;
        HIPCHK(hipEventElapsedTime(&t, c->ev_c, c->ev_d)); ms[2] += t;
        trials++;
        if (bad > 0) return nonfinite_field(who() + ": the reconstruction at tolerance " + std::to_string(wrbud::grid_tol(gk)) + " is not finite");
        return WR_OK;
    }

    int run(double lo, double hi, const double* coef, const Prologue& pro)
    {
        d_coef = coef; p = pro;
        if ((uintptr_t)d_coef & 15) return fail(WR_ERR_ARG, who() + " needs a 16-byte aligned coefficient array");
        const double absmax = fmax(fabs(p.lo), fabs(p.hi));
        if (!(absmax <= DBL_MAX)) return nonfinite_field(who() + " needs a finite field");
        range = p.hi - p.lo;
        if (norm == WR_NORM_PSNR) {  // the one conversion: everything below is stated on R against this value
            max_err = wrbud::psnr_rms(psnr_db, p.lo, p.hi);
            if (max_err != max_err) return fail(WR_ERR_ARG, "a PSNR target needs a field whose range hi - lo is a positive finite number");
        }
        rlo[0] = lo; rhi[0] = hi; nrange = 1;
        const int rc = wrbud::bounded_walk(max_err, g_min, wrbud::bounded_start(max_err, absmax), [this](int gk, double* e) { return eval(gk, e); }, &g, &err);
        if (rc == wrbud::kBoundedMiss) {
            char b[200];
            if (norm == WR_NORM_MAX)
                snprintf(b, sizeof b, "the error bound %.17g is below what the finest tolerance allowed reaches: E(g_min = %d) = %.17g", max_err, g, err);
            else
                snprintf(b, sizeof b, "the RMS target %.17g is below what the finest tolerance allowed reaches: R(g_min = %d) = %.17g", max_err, g, err);
            g = -1;
            return fail(WR_ERR_BOUND, b);
        }
        return rc;
    }
};

// ---- masked fields (include/waverange_amd.h; the kernels and the blob: wr_mask.h) -------------------------------------------
// A masked encode is the plain segmented encode with two stages in front of the prologue -- split (the mask bits, the count
// and the mean of the defined samples: one read of the field where upload_field left it) and fill (the mean into the undefined
// samples, in the slot) -- and the mask blob behind the field's planes.  The mask's coder kernels go on a stream of their own
// as soon as the split has been read back, so that they run under the field's transform and quantizer; they share nothing with
// the field's stages but the bits, which nothing writes after the split.  A masked decode runs the mask's decoder on the
// second stream under the field's coder stage, checks the mask before the finisher writes anything, and puts `fill` into the
// field behind the inverse transform, in the slot (a host field) or in the caller's array (a device field).
std::string bad_segments_text(unsigned int k);
int seg_upload_offsets(const uint8_t* front, size_t head, uint32_t nseg, uint8_t* work);

struct MaskStreams {
    hipStream_t st = nullptr;
    hipEvent_t ev[6] = {nullptr};  // pairs: split (decode: unused), fill or restore, the mask's coder
    MaskStreams() = default;
    MaskStreams(const MaskStreams&) = delete;
    MaskStreams& operator=(const MaskStreams&) = delete;
    ~MaskStreams()
    {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    int create()
    {
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
        return WR_OK;
    }
    float ms(int pair) const
    {
        float t = 0;
        if (hipEventElapsedTime(&t, ev[2 * pair], ev[2 * pair + 1]) != hipSuccess) { (void)hipGetLastError(); return 0; }
        return t;
    }
};

unsigned long long* mask_result_host(wr_ctx* c) { return reinterpret_cast<unsigned long long*>(c->h_result + 8 + 2 * WR_NLAYMAX + wrk::kProbeK + 5); }
unsigned long long* mask_result_dev(wr_ctx* c) { return reinterpret_cast<unsigned long long*>(c->h_result_dev + 8 + 2 * WR_NLAYMAX + wrk::kProbeK + 5); }

// the split's read-back: S and the count of the defined samples (c->h_result[0 .. 1]) as the count of undefined ones and the pad
// (res[0 .. 1]: where the split's final kernel left S and the count; the batched split reads a pair per field the same way)
template <class T>
void mask_split_result(const double* res, size_t n, unsigned long long* undefined, double* pad)
{
    unsigned long long count = 0;
    memcpy(&count, res + 1, sizeof count);
    *undefined = (unsigned long long)n - count;
    double mean = count ? res[0] / (double)count : NAN;
    if (sizeof(T) == sizeof(float)) mean = (double)(float)mean;  // (what an fp32 field is filled with)
    *pad = mean;
}
template <class T>
void mask_split_result(wr_ctx* c, size_t n, unsigned long long* undefined, double* pad) { mask_split_result<T>(c->h_result, n, undefined, pad); }

struct MaskEncode {
    // what the caller asks for
    double below = -INFINITY;
    // what comes out
    unsigned long long undefined = 0;
    double pad = 0;
    size_t mask_len = 0;
    float split_ms = 0, fill_ms = 0, coder_ms = 0;

    wr_ctx* c = nullptr;
    MaskStreams s;
    size_t n = 0, nsym = 0, blob_cap = 0;
    unsigned seg = 0;

    // the buffers (from the plane pool, kept in bufs) and the second stream
    int begin(wr_ctx* ctx, SegBufs* bufs, size_t count, unsigned seg_len)
    {
        c = ctx; n = count; seg = seg_len; nsym = wrmask::mask_bytes(n);
        blob_cap = (wr_seg_bound(nsym, seg) + 15) & ~(size_t)15;
        bufs->mask[0] = plane_scratch(c, (nsym + 255) & ~(size_t)255);
        bufs->mask[1] = plane_scratch(c, wrk::seg_stage_bytes(nsym, seg));
        bufs->mask[2] = plane_scratch(c, blob_cap);
        for (const DevPlanes::Buf& b : bufs->mask) if (!b.p) return WR_ERR_HIP;
        if (int rc = s.create()) return rc;
        bufs->also = s.st;
        return WR_OK;
    }

    // (cu_mu held, the context's stream) split and fill of the field at d_x; then the mask's coder kernels on the second stream
    template <class T>
    int split_fill(SegBufs* bufs, T* d_x)
    {
        uint8_t* const bits = bufs->mask[0].p;
        HIPCHK(hipEventRecord(s.ev[0], c->stream));
        wrk::mask_split(d_x, n, below, bits, c->d_partial, c->h_result_dev, c->stream);
        HIPCHK(hipEventRecord(s.ev[1], c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask split launch failed");
        HIPCHK(hipEventSynchronize(s.ev[1]));
        split_ms = s.ms(0);
        mask_split_result<T>(c, n, &undefined, &pad);
        if (undefined == (unsigned long long)n) return fail(WR_ERR_ARG, "no defined sample: every sample of the field is a NaN, an infinity or below the threshold");
        if (!(fabs(pad) <= DBL_MAX)) return fail(WR_ERR_ARG, "the mean of the defined samples is not finite");
        if (!undefined) return WR_OK;
        HIPCHK(hipEventRecord(s.ev[2], c->stream));
        wrk::mask_fill(d_x, n, bits, (T)pad, c->stream);
        HIPCHK(hipEventRecord(s.ev[3], c->stream));
        HIPCHK(hipEventRecord(s.ev[4], s.st));
        wrk::seg_encode(wrk::plane_ref(bits), nsym, seg, bufs->mask[1].p, bufs->mask[2].p, blob_cap, mask_result_dev(c), s.st);
        HIPCHK(hipEventRecord(s.ev[5], s.st));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask coder launch failed");
        return WR_OK;
    }

    // the blob's exact length, mask_len: waits for the mask's coder (an encode to a byte budget needs it before its first probe)
    int length()
    {
        if (!undefined || mask_len) return WR_OK;
        if (hipStreamSynchronize(s.st) != hipSuccess) return fail(WR_ERR_HIP, "the mask's coder failed on the device");
        const unsigned long long len = mask_result_host(c)[0], bad = mask_result_host(c)[1];
        if (bad || len > blob_cap) return fail(WR_ERR_HIP, std::string("internal: mask plane: ") + kOutgrew);
        mask_len = wrmask::kHeaderBytes + (size_t)len;
        return WR_OK;
    }

    // the blob to data_enc + at, once the field's planes are there
    int download(const SegBufs& bufs, unsigned char* data_enc, size_t at)
    {
        if (!undefined) return WR_OK;
        wrmask::put_header(data_enc + at, n, undefined, pad);
        if (int rc = xfer_field(c, &c->x_field, data_enc + at + wrmask::kHeaderBytes, bufs.mask[2].p, mask_len - wrmask::kHeaderBytes, kDown)) return rc;
        fill_ms = s.ms(1);
        coder_ms = s.ms(2);
        return WR_OK;
    }

    int finish(const SegBufs& bufs, unsigned char* data_enc, size_t at)
    {
        if (int rc = length()) return rc;
        return download(bufs, data_enc, at);
    }

    void result(wr_mask_result* res) const
    {
        if (!res) return;
        res->undefined = undefined; res->pad = pad; res->mask_len = mask_len;
        res->split_ms = split_ms; res->fill_ms = fill_ms; res->mask_coder_ms = coder_ms;
    }
};

// a region as the mask's crop takes it (wr_mask.h); roi == nullptr: the whole box of the level
wrmask::Region mask_region(int nx, int ny, int nz, int level, const wr_box* roi)
{
    const wrlow::Box b = wrlow::box_of(nx, ny, nz, level);
    const wr_box whole{0, 0, 0, b.bx, b.by, b.bz};
    if (!roi) roi = &whole;
    return wrmask::Region{nx, ny, nz, level, roi->x0, roi->y0, roi->z0, roi->x1, roi->y1, roi->z1};
}

// wr_dev_mask_split / _f32: the split alone, as a stage call
template <class T>
int dev_mask_split(wr_ctx* c, const T* d_fld, size_t n, double below, unsigned char* d_bits, unsigned long long* undefined, double* pad)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!d_fld || !d_bits || !undefined || !pad) return fail(WR_ERR_ARG, "null pointer");
    if (!n) return fail(WR_ERR_ARG, "empty array");
    if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");
    std::lock_guard<std::mutex> lk(c->mu);
    StageLock cu(c->pool->cu_mu);
    wrk::mask_split(d_fld, n, below, d_bits, c->d_partial, c->h_result_dev, c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask split launch failed");
    HIPCHK(hipStreamSynchronize(c->stream));
    mask_split_result<T>(c, n, undefined, pad);
    return WR_OK;
}

// wr_dev_mask_fill (undefined == nullptr) and wr_dev_mask_restore, and their _f32 forms
template <class T>
int dev_mask_apply(wr_ctx* c, T* d_fld, size_t n, const unsigned char* d_bits, double value, unsigned long long* undefined)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!d_fld || !d_bits) return fail(WR_ERR_ARG, "null pointer");
    if (!n) return fail(WR_ERR_ARG, "empty array");
    std::lock_guard<std::mutex> lk(c->mu);
    StageLock cu(c->pool->cu_mu);
    if (!undefined) {  // wr_dev_mask_fill
        wrk::mask_fill(d_fld, n, d_bits, (T)value, c->stream);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask fill launch failed");
        HIPCHK(hipStreamSynchronize(c->stream));
        return WR_OK;
    }
    unsigned long long* const counters = reinterpret_cast<unsigned long long*>(c->d_partial);
    unsigned long long got[2] = {0, 0};
    wrk::mask_restore(d_fld, n, d_bits, (T)value, counters, c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask restore launch failed");
    HIPCHK(hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *undefined = got[0];
    if (got[1]) return fail(WR_ERR_STREAM, "mask: a bit beyond the field's last sample is set");
    return WR_OK;
}

// wr_dev_mask_restore_box / _f32: the box restore alone, as a stage call
template <class T>
int dev_mask_restore_box(wr_ctx* c, T* d_out, int nx, int ny, int nz, int level, const wr_box* roi, const unsigned char* d_bits, double fill,
                                unsigned long long* undefined)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!d_out || !d_bits || !undefined) return fail(WR_ERR_ARG, "null pointer");
    if (nx < 1 || ny < 1 || nz < 1 || !wrlow::level_ok(level)) return fail(WR_ERR_ARG, "non-positive dimension or level outside [0, 4]");
    if (roi && !wrroi::roi_ok(wrlow::box_of(nx, ny, nz, level), *roi)) return fail(WR_ERR_ARG, "the region is empty or reaches outside the box of the level");
    const wrmask::Region g = mask_region(nx, ny, nz, level, roi);
    std::lock_guard<std::mutex> lk(c->mu);
    StageLock cu(c->pool->cu_mu);
    unsigned long long* const counters = reinterpret_cast<unsigned long long*>(c->d_partial);
    unsigned long long got = 0;
    wrk::mask_restore_box(d_out, g, d_bits, (T)fill, counters, c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask restore launch failed");
    HIPCHK(hipMemcpyAsync(&got, counters, sizeof got, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *undefined = got;
    return WR_OK;
}
// bud != nullptr: an encode to a byte budget (WRS1): the tolerance comes from the search, cut.vec[0] only names the finest one
// bnd != nullptr: an encode to an error bound (any of the formats), likewise
// msk != nullptr: a masked encode: split and fill in front of the prologue, the mask blob behind the planes
// msk with bnd: the trials compare over the defined samples only; msk with bud: the blob's exact length comes off the budget
int encode_seg_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, int wtflag, const Cutoff& cut, unsigned seg, unsigned brick, unsigned strands,
                    wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm, BudgetSearch* bud = nullptr, BoundedSearch* bnd = nullptr,
                    MaskEncode* msk = nullptr)
{
    if (int rc = seg_format_params(&seg, brick, strands)) return rc;
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null field pointer");
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    if (cut.mx < 1 || cut.my < 1 || cut.mz < 1 || !cut.vec) return fail(WR_ERR_ARG, "bad local cutoff description");
    std::lock_guard<std::mutex> lk(c->mu);
    if (fld.host_f32 && c->keep_residual)
        return fail(WR_ERR_UNSUPPORTED, "an fp32 field cannot take the residual back: wr_ctx_set_keep_residual(ctx, 0) for fp32 encodes");
    if (bud && c->keep_residual)
        return fail(WR_ERR_UNSUPPORTED, "an encode to a byte budget does not keep the residual: wr_ctx_set_keep_residual(ctx, 0)");
    if (bnd && c->keep_residual)
        return fail(WR_ERR_UNSUPPORTED, bnd->who() + " does not keep the residual: wr_ctx_set_keep_residual(ctx, 0)");
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    if (wrseg::seg_count(n, seg) > 0xffffffffu) return fail(WR_ERR_ARG, "too many segments");
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    c->pend_valid = false;  // planes a wr_decode_begin parked in this context do not survive an encode on it
    PlaneHold planes(c);
    SegBufs bufs(c);  // (after the planes: it goes first when the call unwinds, and waits for the stream)

    SlotNeed need;
    transform_need(nx, ny, nz, wtflag ? kWavLvl : 0, &need);
    if (fld.host || fld.host_f32) need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    FieldUpload up;
    if (int rc = upload_field(c, slot.get(), fld, nx, ny, nz, wtflag, &up)) return rc;
    local.h2d_ms = up.ms;
    double* const d_fld = up.d_fld;
    SegTarget t;  // (a blob buffer per plane, as the planes come)
    if (int rc = seg_target(c, &bufs, n, seg, brick, strands, brick ? wrblk::order_of(nx, ny, nz, wtflag ? kWavLvl : 0, brick) : wrblk::Order{}, &t)) return rc;
    if (msk) if (int rc = msk->begin(c, &bufs, n, seg)) return rc;
    if (bnd) {  // the trials' work arrays, and the field where the forward transform will not leave it as it is
        for (int k = 0; k < 2; k++) {
            bufs.trial[k] = plane_scratch(c, n * sizeof(double));
            if (!bufs.trial[k].p) return WR_ERR_HIP;
        }
        const bool intact = wtflag && use_fused(nx, ny, nz, kWavLvl) && wrk::fused_minmax_records(nx, ny, nz) != 0;  // all four levels out of place
        const void* src = fld.host_f32 ? (up.d_f32 ? (const void*)up.d_f32 : (const void*)up.widen_from) : (const void*)d_fld;
        if (!intact) {
            const size_t bytes = n * (fld.host_f32 ? sizeof(float) : sizeof(double));
            bufs.trial[2] = plane_scratch(c, bytes);
            if (!bufs.trial[2].p) return WR_ERR_HIP;
            HIPCHK(hipMemcpyAsync(bufs.trial[2].p, src, bytes, hipMemcpyDeviceToDevice, c->stream));
            src = bufs.trial[2].p;
        }
        bnd->c = c; bnd->slot = slot.get(); bnd->nx = nx; bnd->ny = ny; bnd->nz = nz; bnd->wlev = wtflag ? kWavLvl : 0; bnd->n = n; bnd->seg = seg;
        if (fld.host_f32) bnd->orig_f32 = static_cast<const float*>(src);
        else bnd->orig = static_cast<const double*>(src);
        bnd->w1 = reinterpret_cast<double*>(bufs.trial[0].p); bnd->w2 = reinterpret_cast<double*>(bufs.trial[1].p);
    }
    double* resid = d_fld;
    int rc = WR_OK;
    {
        StageLock cu(pool->cu_mu);
        const bool one_array = cut.count() > 1;
        auto plane_buf = [&](unsigned l) -> const wrk::PlaneRef* {
            if (plane_prepare(c, (int)l, n, false, one_array, &cu, nullptr, false) != WR_OK || bufs.coded_plane((int)l, t.blob_cap) != WR_OK) return nullptr;
            return &c->ps[l].ref;
        };
        // plane l's coder kernels go behind its quantizer (and the read-back of the next plane's min/max) on the same stream
        auto after_quant = [&](unsigned l, bool) -> int {
            if (int arc = seg_encode_plane(c, t, c->ps[l].ref, n, (int)l, bufs.blob[l].p, bufs.ev)) return arc;
            if (bud) g_stat[WR_STAT_BUDGET_CODER_RUNS]++;
            if (bnd) g_stat[bnd->quality ? WR_STAT_QUALITY_CODER_RUNS : WR_STAT_BOUNDED_CODER_RUNS]++;
            return WR_OK;
        };
        clock_warmup(c, n);
        if (msk) {  // the field where it landed: an fp32 field before anything widens it
            float* const x32 = up.d_f32 ? const_cast<float*>(up.d_f32) : up.widen_from;
            if ((rc = fld.host_f32 ? msk->split_fill(&bufs, x32) : msk->split_fill(&bufs, d_fld)) != WR_OK) return rc;
            // the trials compare over the defined samples only (the field's copy, where one was taken, went ahead of the fill
            // in stream order: it holds the caller's values; the slot holds the padded field: the masked compare reads neither
            // where a bit is set)
            if (bnd && msk->undefined) { bnd->mask_bits = bufs.mask[0].p; bnd->nd = (unsigned long long)n - msk->undefined; }
        }
        if (up.widen_from) wrk::widen_f32(up.widen_from, d_fld, n, c->stream);
        PickStep pick;
        if (bud) {
            if ((rc = bud->begin(c, n, seg)) != WR_OK) return rc;
            if (msk) {  // the planes get what the blob leaves: its exact length, so the mask's coder is waited for here
                if ((rc = msk->length()) != WR_OK) return rc;
                bud->reserve(msk->mask_len);
            }
            pick = [bud](unsigned l, double lo, double hi, const wrk::QuantPrev& prev, const double* d_coef, const Prologue& p, double* tolabs) {
                return bud->pick(l, lo, hi, prev, d_coef, p, tolabs);
            };
        }
        if (bnd) {  // the whole search at plane 0; the loop then runs at the tolerance it chose, as the plain call does
            pick = [bnd](unsigned l, double lo, double hi, const wrk::QuantPrev&, const double* d_coef, const Prologue& p, double* tolabs) {
                if (l) return (int)WR_OK;
                if (int prc = bnd->run(lo, hi, d_coef, p)) return prc;
                *tolabs = abs_tolerance(wrbud::grid_tol(bnd->g), p);
                return (int)WR_OK;
            };
        }
        rc = encode_planes_core(c, slot.get(), d_fld, nx, ny, nz, wtflag, cut, plane_buf, [](unsigned) { return (uint16_t*)nullptr; }, info, &local,
                                after_quant, [](unsigned, bool) { return WR_OK; }, &resid, up.d_f32, (bud || bnd) ? &pick : nullptr);
        rc = encode_stage_end(c, rc, fld, resid, n, info);
    }
    if (rc) return rc;
    if (c->keep_residual && info->nlay && fld.host)
        if ((rc = xfer_field(c, &c->x_field, fld.host, resid, n * sizeof(double), kDown)) != WR_OK) return rc;
    // ---- stage "down": every plane's blob, one copy each, to its place in data_enc
    size_t total = 0;
    if ((rc = seg_coded_lengths(info->nlay, t.blob_cap, [&](int l) { return seg_result_host(c, l); }, info->len_enc_vec, &total)) != WR_OK) return rc;
    if (total > cap || (total && !data_enc)) return fail(WR_ERR_OVERFLOW, wrtc::kTooLarge);
    if (msk && msk->undefined && (!data_enc || wr_mask_bound(n, seg) > cap - total))
        return fail(WR_ERR_OVERFLOW, "the coded buffer does not hold the field's planes and the bound of the mask blob (wr_mask_bound)");
    if (bud && total > bud->bound) return fail(WR_ERR_HIP, "internal: the coded planes are longer than their size bound");
    if (bud && bud->masked && total + bud->mask_len > bud->budget)  // (a constant padded field: no pick ever saw the budget)
        return fail(WR_ERR_BUDGET, "the budget is below the mask blob: " + std::to_string(msk->mask_len) + " bytes is the smallest budget that would do");
    if ((rc = seg_download_blobs(c, bufs, info->nlay, info->len_enc_vec, data_enc, &local)) != WR_OK) return rc;
    if (msk) if ((rc = msk->finish(bufs, data_enc, total)) != WR_OK) return rc;
    info->ntot_enc = total;
    local.total = now() - t0;
    local.wait = t_phase - t0;
    local.gpu = now() - t_phase;
    if (tm) *tm = local;
    return WR_OK;
}

// ---- the stages of a segmented decode.  Every driver below -- the full decode, the box and region decodes, the many-region
// decode, the batch, the segmented source of a transcode and the stage calls -- is a composition of these; none of them
// states the stream parse, the work-buffer layout, the coder stage or the tail a second time.

// The host's view of a validated coded field.  Every plane's header and index are checked on the host before anything is
// launched: the kernels only ever see offsets that lie inside their blob, in order, each stream no longer than a segment can
// be.  brick: 0 for a WRS1 stream, the brick edge of a WRS2 stream; strands: 0, or the strand count of a WRS3 stream (whose
// brick may be 0).  A stream whose planes differ in format, brick or strand count is refused.
struct SegStream {
    bool constant = false;  // ntot_enc == 0: the field is midval, nothing else is looked at (wrappers.cpp:462-469)
    int nlay = 0;
    size_t off[WR_NLAYMAX + 1] = {0};  // where plane l's blob starts in the coded buffer
    uint32_t seg[WR_NLAYMAX] = {0}, nseg[WR_NLAYMAX] = {0}, brick = 0, strands = 0;
    wrblk::Order od{};  // brick != 0: the blocked order of the planes
    size_t head() const { return wrseg::header_bytes(brick, strands); }
};

// who: put in front of every message ("field 3: " in a batch)
int seg_stream_of(int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, SegStream* s,
                  const std::string& who = std::string())
{
    if (info->ntot_enc == 0) { s->constant = true; return WR_OK; }
    const int nlay = info->nlay;
    if (nlay < 1 || nlay > WR_NLAYMAX) return fail(WR_ERR_ARG, who + "nlay out of range");
    if (info->wlev != 0 && info->wlev != kWavLvl) return fail(WR_ERR_ARG, who + "wlev must be 0 or 4");
    if (!data_enc) return fail(WR_ERR_ARG, who + "null coded buffer");
    if (int rc = plane_offsets(info, nlay, data_len, s->off, who)) return rc;
    std::string why;
    if (!wrtc::check_planes(data_enc, s->off, info, nlay, (size_t)nx * ny * nz, s->seg, s->nseg, &s->brick, &s->strands, &why)) return fail(WR_ERR_STREAM, who + why);
    if (s->brick) s->od = wrblk::order_of(nx, ny, nz, (int)info->wlev, s->brick);
    s->nlay = nlay;
    return WR_OK;
}

// the segmented source of a transcode: wrtc::validate has run the same checks (wr_transcode.h; it also serves the host-only form)
SegStream seg_stream_of(const wrtc::Source& src, int nx, int ny, int nz, int wlev)
{
    SegStream s;
    s.nlay = src.nlay;
    memcpy(s.off, src.off, sizeof s.off);
    memcpy(s.seg, src.seg, sizeof s.seg);
    memcpy(s.nseg, src.nseg, sizeof s.nseg);
    s.brick = src.brick; s.strands = src.strands;
    if (s.brick) s.od = wrblk::order_of(nx, ny, nz, wlev, s.brick);
    return s;
}

// the constant field of a call, and the call's end
int finish_constant(wr_ctx* c, const FieldRef& fld, size_t count, double midval, double t0, wr_timings* local, wr_timings* tm)
{
    if (int rc = fill_constant(c, fld, count, midval)) return rc;
    local->total = now() - t0;
    if (tm) *tm = *local;
    return WR_OK;
}

// the byte offsets of the segment streams behind the index (nseg + 1 of them), from an index that check_index has passed
std::vector<unsigned long long> seg_offsets(const uint8_t* front, size_t head, uint32_t nseg)
{
    std::vector<unsigned long long> offs((size_t)nseg + 1);
    unsigned long long run = 0;
    for (uint32_t k = 0; k < nseg; k++) { offs[k] = run; run += wrseg::get_u32(front + head + 4 * (size_t)k); }
    offs[nseg] = run;
    return offs;
}

// ... to their place in a decoder's work buffer (wr_kernels.h)
int seg_upload_offsets(const std::vector<unsigned long long>& offs, uint8_t* work)
{
    HIPCHK(hipMemcpy(wrk::seg_work_offs(work), offs.data(), offs.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return WR_OK;
}

int seg_upload_offsets(const uint8_t* front, size_t head, uint32_t nseg, uint8_t* work) { return seg_upload_offsets(seg_offsets(front, head, nseg), work); }

// The job of one plane for the batched decoder kernels: its blob of `len` bytes, decoded into sym.  work (may be null for a
// plane without segments to decode): the plane's work buffer, whose offsets, flags and failure count the job points at.
wrk::SegJob seg_job(const wrk::PlaneRef& sym, const uint8_t* blob, size_t len, uint8_t* work, size_t n, uint32_t seg, uint32_t nseg, uint32_t brick)
{
    wrk::SegJob j;
    memset(&j, 0, sizeof j);
    j.sym = sym;
    j.n = n; j.blob = const_cast<uint8_t*>(blob); j.cap = len;
    j.seg = seg; j.nseg = nseg; j.brick = brick;
    if (work) { j.offs = wrk::seg_work_offs(work); j.flags = wrk::seg_work_flags(work, nseg); j.bad = wrk::seg_work_bad(work); }
    return j;
}

// what a decoder's failure count says, behind the caller's "plane 2: " or "job 5: segmented plane: "
std::string bad_segments_text(unsigned int k) { return std::to_string(k) + " segment(s) do not decode to their symbols"; }

// the coder seconds of a call, from the event pairs the coder stage recorded: plane_coder_s[0, count) and their sum
template <class Bufs>
void fold_coder_seconds(const Bufs& bufs, int count, wr_timings* tm)
{
    for (int l = 0; l < count; l++) {
        tm->plane_coder_s[l] = bufs.ev.seconds(l);
        tm->rangecoder += tm->plane_coder_s[l];
    }
}

// (gather_mu held) plane l of the context made ready for a decoder kernel, with its blob and work buffers and, if wanted, its
// pair of events.  windows: the plane is laid out for the host coder's windows (a transcode into the reference format)
int seg_plane_bufs(wr_ctx* c, SegBufs* bufs, int l, size_t n, size_t blob_bytes, size_t work_bytes, bool windows, bool events)
{
    if (int rc = plane_prepare(c, l, n, true, false, nullptr, nullptr, windows)) return rc;
    bufs->blob[l] = plane_scratch(c, blob_bytes);
    bufs->work[l] = plane_scratch(c, work_bytes);
    if (!bufs->blob[l].p || !bufs->work[l].p) return WR_ERR_HIP;
    return events ? bufs->ev.create(l) : WR_OK;
}

// stage "up" of a decode of whole planes: one copy per blob, and its segments' offsets
int seg_upload_planes(wr_ctx* c, const SegStream& s, const wr_enc_info* info, const unsigned char* data_enc, SegBufs* bufs, float* ms)
{
    for (int l = 0; l < s.nlay; l++) {
        if (int rc = xfer_field(c, &c->x_field, bufs->blob[l].p, data_enc + s.off[l], info->len_enc_vec[l], kUp)) return rc;
        *ms += (float)c->x_field.ms;
        if (int rc = seg_upload_offsets(data_enc + s.off[l], s.head(), s.nseg[l], bufs->work[l].p)) return rc;
    }
    return WR_OK;
}

// The streams of the segments in ids (ascending), from the host blob to the same place in the device blob: consecutive
// segments go as one copy, nothing else of the blob is touched.  *ms and *bytes are added to.
int seg_upload_streams(wr_ctx* c, uint8_t* d_blob, const uint8_t* h_blob, size_t front, const std::vector<unsigned long long>& offs,
                       const std::vector<uint32_t>& ids, float* ms, size_t* bytes)
{
    constexpr size_t kPiece = (size_t)128 << 20;  // (as xfer_field: a long copy holds up whatever is queued behind it)
    Piece pc[4];
    int np = 0;
    auto flush = [&]() -> int {
        if (!np) return WR_OK;
        if (int rc = xfer_start(c, &c->x_field, pc, np, kUp)) return rc;
        if (int rc = xfer_wait(&c->x_field)) return rc;
        *ms += (float)c->x_field.ms;
        np = 0;
        return WR_OK;
    };
    for (size_t i = 0; i < ids.size();) {
        size_t j = i;
        while (j + 1 < ids.size() && ids[j + 1] == ids[j] + 1) j++;
        const size_t a = front + (size_t)offs[ids[i]], b = front + (size_t)offs[(size_t)ids[j] + 1];
        for (size_t at = a; at < b; at += kPiece) {
            pc[np++] = Piece{d_blob + at, h_blob + at, b - at < kPiece ? b - at : kPiece};
            if (np == 4) if (int rc = flush()) return rc;
        }
        *bytes += b - a;
        i = j + 1;
    }
    return flush();
}

// Per used plane the list of segments to decode; planes cut at the same length share it (planes may have been cut at
// different lengths).  list_of(seg, &ids): the ascending ids for a plane cut at seg.
template <class ListOf>
void seg_plane_lists(const SegStream& s, int used, std::vector<uint32_t>* ids, ListOf list_of)
{
    for (int l = 0; l < used; l++) {
        int same = -1;
        for (int k = 0; k < l; k++) if (s.seg[k] == s.seg[l]) same = k;
        if (same >= 0) ids[l] = ids[same];
        else list_of(s.seg[l], &ids[l]);
    }
}

// stage "up" of a partial decode: the brick list, then per used plane the offsets table, the id list and the streams of the
// listed segments -- the others are not looked at beyond their length in the index.  *bytes_up: the payload bytes copied.
// blob[l], work[l]: the device buffers of plane l; d_bricks: where the brick list goes (not looked at if there is none)
int seg_upload_lists(wr_ctx* c, const SegStream& s, int used, const unsigned char* data_enc, uint8_t* const* blob, uint8_t* const* work_of, uint8_t* d_bricks,
                     const std::vector<uint32_t>* ids, const std::vector<uint32_t>& bricks, float* ms, size_t* bytes_up)
{
    if (!bricks.empty()) HIPCHK(hipMemcpy(d_bricks, bricks.data(), bricks.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (int l = 0; l < used; l++) {
        const uint8_t* const front = data_enc + s.off[l];
        uint8_t* const work = work_of[l];
        const std::vector<unsigned long long> offs = seg_offsets(front, s.head(), s.nseg[l]);
        if (int rc = seg_upload_offsets(offs, work)) return rc;
        if (!ids[l].empty()) HIPCHK(hipMemcpy(wrk::seg_decode_list_ids(work, s.nseg[l]), ids[l].data(), ids[l].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (int rc = seg_upload_streams(c, blob[l], front, s.head() + 4 * (size_t)s.nseg[l], offs, ids[l], ms, bytes_up)) return rc;
    }
    return WR_OK;
}

int seg_upload_lists(wr_ctx* c, const SegStream& s, int used, const unsigned char* data_enc, SegBufs* bufs, const std::vector<uint32_t>* ids,
                     const std::vector<uint32_t>& bricks, float* ms, size_t* bytes_up)
{
    uint8_t *blob[WR_NLAYMAX], *work[WR_NLAYMAX];
    for (int l = 0; l < WR_NLAYMAX; l++) { blob[l] = bufs->blob[l].p; work[l] = bufs->work[l].p; }
    return seg_upload_lists(c, s, used, data_enc, blob, work, bufs->bricks.p, ids, bricks, ms, bytes_up);
}

// ---- the mask stage of the decode drivers: what every masked decode does with the WRM1 blob behind a record's planes -- validate
// it on the host, get the needed segments onto the device, decode them beside the field's planes, judge them -- written once.
// MaskJob is one blob being decoded.  The drivers differ in where its buffers come from and in who launches its decode: the
// single calls (MaskDecode below) on a stream of the mask's own, the batch call as one more job of its list launch.
struct MaskJob {
    const unsigned char* blob = nullptr;  // the WRM1 header, the WRS1 plane behind it
    size_t len = 0;
    wrmask::BlobInfo info;   // what the header and the index say
    size_t n = 0, nsym = 0;  // the field's samples, the plane's symbols
    std::vector<uint32_t> ids;  // the segments to decode, ascending; empty: the whole plane
    // the device buffers: the plane (always full length: a listed decode writes where its segments lie), the decoder's offsets,
    // flags and list, the blob's bytes
    uint8_t *bits = nullptr, *work = nullptr, *d_blob = nullptr;

    const unsigned char* plane() const { return blob + wrmask::kHeaderBytes; }
    size_t plane_len() const { return len - wrmask::kHeaderBytes; }

    // the header and the whole index, on the host; false: refused, *why saying what ("mask blob: ...", a WR_ERR_STREAM)
    bool parse(size_t count, std::string* why)
    {
        n = count; nsym = wrmask::mask_bytes(n);
        return wrmask::check_blob(blob, len, n, &info, why);
    }
    // (behind parse) only the segments that hold a bit of one of the regions are decoded
    void list(const wrmask::Region* gs, size_t nroi)
    {
        ids.resize(nroi == 1 ? wrmask::roi_segments(gs[0], info.seg, nullptr, 0) : wrmask::roi_segments_multi(gs, nroi, info.seg, nullptr, 0));
        if (nroi == 1) wrmask::roi_segments(gs[0], info.seg, ids.data(), ids.size());
        else wrmask::roi_segments_multi(gs, nroi, info.seg, ids.data(), ids.size());
    }
    // what the job takes from the plane pool; the driver says from where, and rounds as its pool does
    size_t bits_bytes() const { return (nsym + 255) & ~(size_t)255; }
    size_t work_bytes() const { return ids.empty() ? wrk::seg_decode_work_bytes(info.nseg) : wrk::seg_decode_list_work_bytes(info.nseg, ids.size()); }
    size_t blob_bytes() const { return plane_len(); }
    // stage "up" (the buffers set): the whole blob and its offsets, or the listed segments' bytes, the list and the offsets.
    // ms, *bytes_up: as seg_upload_lists counts them (a whole plane counts nothing)
    int upload(wr_ctx* c, float* ms, size_t* bytes_up) const
    {
        if (ids.empty()) {
            if (int rc = xfer_field(c, &c->x_field, d_blob, plane(), plane_len(), kUp)) return rc;
            return seg_upload_offsets(plane(), wrseg::kHeaderBytes, info.nseg, work);
        }
        SegStream one;  // the mask's plane as a stream of one WRS1 plane
        one.nlay = 1; one.off[1] = plane_len(); one.seg[0] = info.seg; one.nseg[0] = info.nseg;
        uint8_t *blob_of[1] = {d_blob}, *work_of[1] = {work};
        return seg_upload_lists(c, one, 1, plane(), blob_of, work_of, nullptr, &ids, std::vector<uint32_t>(), ms, bytes_up);
    }
    // the job and the list of its decode, for a launch someone else makes (a WRS1 plane in the natural order)
    wrk::SegJob seg_job() const { return ::seg_job(wrk::plane_ref(bits), d_blob, plane_len(), work, nsym, info.seg, info.nseg, 0); }
    wrk::SegList seg_list() const
    {
        wrk::SegList ls;
        memset(&ls, 0, sizeof ls);
        ls.ids = wrk::seg_decode_list_ids(work, info.nseg); ls.nlist = (uint32_t)ids.size();
        return ls;
    }
};

// `fill` into the elements of region g that the host holds at fld, where a bit of the plane h_bits is set (the whole field: the
// whole box of level 0).  Returns the count of those elements.
size_t mask_restore_host(const FieldRef& fld, const wrmask::Region& g, const unsigned char* h_bits, double fill)
{
    const int cx = g.x1 - g.x0, cy = g.y1 - g.y0, cz = g.z1 - g.z0;
    size_t at = 0, count = 0;
    for (int z = 0; z < cz; z++)
        for (int y = 0; y < cy; y++)
            for (int x = 0; x < cx; x++, at++) {
                const size_t J = g.bit(x, y, z);
                if (!((h_bits[J >> 3] >> (J & 7)) & 1)) continue;
                if (fld.host) fld.host[at] = fill;
                else fld.host_f32[at] = (float)fill;
                count++;
            }
    return count;
}

// The mask of the single masked calls: its job on a stream of its own, under the field's coder stage.  Two distinctions and no
// others: the job HAS A LIST (a region or low-resolution decode, plan(): only those segments are uploaded and decoded, and the
// checks over the whole mask cannot be made) or not, and the result IS A REGION of a level's box (the restore runs on the region
// as the finisher left it and counts there) or the whole field.
struct MaskDecode {
    // what the caller gives: the blob behind the field's planes (job.blob, job.len), and what the undefined samples become
    MaskJob job;
    double fill = NAN;
    // what comes out
    float coder_ms = 0, up_ms = 0;
    size_t bytes_up = 0;

    wr_ctx* c = nullptr;
    MaskStreams s;
    wrmask::Region g{};   // where the restore runs: the whole box of level 0, or the region of plan()
    bool region = false;  // plan() was called
    unsigned long long* counters = nullptr;  // behind the bits
    unsigned int h_bad = 0;
    unsigned long long h_counters[2] = {0, 0};
    bool restored = false;  // restore() has recorded its events

    // the header and the index, on the host: nothing is launched for a blob that fails here
    int parse(int nx, int ny, int nz)
    {
        if (!job.blob) return fail(WR_ERR_ARG, "null coded buffer");
        std::string why;
        if (!job.parse((size_t)nx * ny * nz, &why)) return fail(WR_ERR_STREAM, why);
        g = mask_region(nx, ny, nz, 0, nullptr);
        return WR_OK;
    }

    // (behind parse) the list of the region; roi == nullptr: the whole box of the level
    void plan(int level, const wr_box* roi)
    {
        region = true;
        g = mask_region(g.nx, g.ny, g.nz, level, roi);
        job.list(&g, 1);
    }

    // the buffers, the second stream, and the job's stage "up"
    int upload(wr_ctx* ctx, SegBufs* bufs)
    {
        c = ctx;
        bufs->mask[0] = plane_scratch(c, job.bits_bytes() + 256);
        bufs->mask[1] = plane_scratch(c, job.work_bytes());
        bufs->mask[2] = plane_scratch(c, (job.blob_bytes() + 15) & ~(size_t)15);
        for (const DevPlanes::Buf& b : bufs->mask) if (!b.p) return WR_ERR_HIP;
        job.bits = bufs->mask[0].p; job.work = bufs->mask[1].p; job.d_blob = bufs->mask[2].p;
        counters = reinterpret_cast<unsigned long long*>(job.bits + job.bits_bytes());
        if (int rc = s.create()) return rc;
        bufs->also = s.st;
        if (int rc = job.upload(c, &up_ms, &bytes_up)) return rc;
        g_stat[WR_STAT_MASK_ROI_BYTES_UP] += bytes_up;
        return WR_OK;
    }

    // (cu_mu held) on the second stream: the list decoder, or the whole plane's decoder and the count of its bits
    int launch()
    {
        HIPCHK(hipEventRecord(s.ev[4], s.st));
        if (!job.ids.empty()) wrk::seg_decode_list(job.d_blob, job.plane_len(), wrk::plane_ref(job.bits), job.nsym, job.info.seg, job.work, job.ids.size(), s.st, 0, 0);
        else wrk::seg_decode(job.d_blob, job.plane_len(), wrk::plane_ref(job.bits), job.nsym, job.info.seg, job.work, s.st);
        HIPCHK(hipEventRecord(s.ev[5], s.st));
        if (job.ids.empty()) wrk::mask_restore((double*)nullptr, job.n, job.bits, 0.0, counters, s.st);
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask decoder launch failed");
        HIPCHK(hipMemcpyAsync(&h_bad, wrk::seg_work_bad(job.work), sizeof h_bad, hipMemcpyDeviceToHost, s.st));
        if (job.ids.empty()) HIPCHK(hipMemcpyAsync(h_counters, counters, sizeof h_counters, hipMemcpyDeviceToHost, s.st));
        g_stat[WR_STAT_MASK_ROI_SEGMENTS] += job.ids.size();
        return WR_OK;
    }

    // ... waited for and judged: the caller's field has not been touched yet.  The two checks over the whole mask need the
    // whole plane: a listed decode does not make them.
    int check()
    {
        if (hipStreamSynchronize(s.st) != hipSuccess) return fail(WR_ERR_HIP, "the mask's decoder failed on the device");
        coder_ms = s.ms(2);
        if (h_bad) return fail(WR_ERR_STREAM, "mask blob: " + bad_segments_text(h_bad));
        if (!job.ids.empty()) return WR_OK;
        if (h_counters[1]) return fail(WR_ERR_STREAM, "mask blob: a bit beyond the field's last sample is set");
        if (h_counters[0] != job.info.undefined) return fail(WR_ERR_STREAM, "mask blob: the mask's set bits are not the count in its header");
        return WR_OK;
    }

    // the mask alone, decoded and judged: a constant record, which has no coder stage to run beside
    int decode_alone(wr_ctx* ctx, SegBufs* bufs)
    {
        if (int rc = upload(ctx, bufs)) return rc;
        StageLock cu(ctx->pool->cu_mu);
        if (int rc = launch()) return rc;
        return check();
    }

    // (the context's stream, behind the finisher) `fill` where a bit is set: over the whole field at d_x, or into the region at
    // d_x, whose count comes back with the stream's next synchronisation
    template <class T>
    int restore(T* d_x)
    {
        HIPCHK(hipEventRecord(s.ev[2], c->stream));
        if (region) wrk::mask_restore_box(d_x, g, job.bits, (T)fill, counters, c->stream);
        else wrk::mask_restore(d_x, job.n, job.bits, (T)fill, counters, c->stream);
        HIPCHK(hipEventRecord(s.ev[3], c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask restore launch failed");
        if (region) HIPCHK(hipMemcpyAsync(h_counters, counters, sizeof h_counters[0], hipMemcpyDeviceToHost, c->stream));
        restored = true;
        return WR_OK;
    }

    // the plane as the device holds it, to the host
    int host_bits(std::vector<unsigned char>* h) const
    {
        h->resize(job.nsym);
        HIPCHK(hipMemcpy(h->data(), job.bits, job.nsym, hipMemcpyDeviceToHost));
        return WR_OK;
    }

    // a host caller's constant padded field: the bits come to the host, as midval was put there
    int restore_host(const FieldRef& fld)
    {
        std::vector<unsigned char> h;
        if (int rc = host_bits(&h)) return rc;
        h_counters[0] = mask_restore_host(fld, g, h.data(), fill);
        return WR_OK;
    }

    // undefined: the header's count (judged against the plane), or the count inside the region
    void result(wr_mask_result* res)
    {
        if (!res) return;
        memset(res, 0, sizeof *res);
        res->undefined = region ? h_counters[0] : job.info.undefined; res->pad = job.info.pad; res->mask_len = job.len;
        res->fill_ms = restored ? s.ms(1) : 0; res->mask_coder_ms = coder_ms;
    }
};

// A constant padded field with a mask (the mask judged: decode_alone): midval in the `count` elements, then the mask.  A host
// field takes the bits on the host, as it takes midval there.
int finish_constant_masked(wr_ctx* c, const FieldRef& fld, size_t count, double midval, MaskDecode* msk, double t0, wr_timings* local, wr_timings* tm)
{
    if (int rc = fill_constant(c, fld, count, midval)) return rc;
    if (fld.dev) {
        StageLock cu(c->pool->cu_mu);
        if (int rc = kernel_stage_end(c, msk->restore(fld.dev))) return rc;
    } else if (int rc = msk->restore_host(fld)) return rc;
    local->total = now() - t0;
    if (tm) *tm = *local;
    return WR_OK;
}

// One coder stage (cu_mu held): the first `planes` planes of the stream, from bufs->blob[l] into q[l].
struct CoderCall {
    const SegStream* s;
    const wr_enc_info* info;  // the blobs' lengths
    int planes;
    size_t n;
    SegBufs* bufs;              // blob[l], work[l] as the "up" stage left them, and the event pairs
    const wrk::PlaneRef* q;     // where plane l's symbols go, in the natural order
    uint8_t* perm[WR_NLAYMAX] = {nullptr};       // a blocked stream: plane l in stream order (one buffer may serve every plane unless all go in one launch)
    const std::vector<uint32_t>* ids = nullptr;  // per plane the segments to decode; nullptr: all of them
    const uint32_t* d_bricks = nullptr;          // a blocked stream with lists: the bricks they cover (device memory) ...
    size_t nbricks = 0;                          // ... nullptr: every brick goes back to its place
    uint8_t *host_table = nullptr, *d_table = nullptr;  // set: all planes in ONE seg_decode_lists launch, timed as plane 0
    int stat_segments = -1;      // the g_stat counter of the segments launched (none: -1)
    bool stat_launches = false;  // the launches count in WR_STAT_ROI_CODER_LAUNCHES
};

// Launch per plane (the whole plane or its list) or one launch over all planes, the inverse reorder of a blocked stream, the
// event pairs; then every plane's failure count comes back once and the stream is drained: whatever runs next only sees
// planes whose every (listed) segment decoded.  tm: plane_coder_s and rangecoder.
int seg_coder_stage(wr_ctx* c, const CoderCall& k, wr_timings* tm)
{
    const SegStream& s = *k.s;
    SegBufs& b = *k.bufs;
    const bool one_launch = k.d_table != nullptr;
    auto sym = [&](int l) { return s.brick ? wrk::plane_ref(k.perm[l]) : k.q[l]; };
    // (what was decoded is in the scratch plane in stream order: the bricks go to their places in the plane)
    auto reorder = [&](int l) { return !s.brick || wrk::plane_reorder(k.q[l], k.perm[l], s.od, true, k.d_bricks, k.nbricks, c->stream); };
    if (one_launch) {
        wrk::SegJob jobs[WR_NLAYMAX];
        wrk::SegList lists[WR_NLAYMAX];
        memset(jobs, 0, sizeof jobs);
        memset(lists, 0, sizeof lists);
        for (int l = 0; l < k.planes; l++) {
            uint8_t* const work = b.work[l].p;
            jobs[l] = seg_job(sym(l), b.blob[l].p, k.info->len_enc_vec[l], work, k.n, s.seg[l], s.nseg[l], s.brick);
            lists[l].ids = wrk::seg_decode_list_ids(work, s.nseg[l]);
            lists[l].nlist = (uint32_t)k.ids[l].size();
            HIPCHK(hipMemsetAsync(wrk::seg_work_bad(work), 0, sizeof(unsigned int), c->stream));
            if (k.stat_segments >= 0) g_stat[k.stat_segments] += k.ids[l].size();
        }
        launch_note(c, "seg_decode_lists", 0, b.blob[0].p, k.n, b.work[0].p, k.q[0]);
        HIPCHK(hipEventRecord(b.ev[0], c->stream));
        wrk::seg_decode_lists(jobs, lists, (size_t)k.planes, k.host_table, k.d_table, c->stream);
        HIPCHK(hipEventRecord(b.ev[1], c->stream));
        if (k.stat_launches) g_stat[WR_STAT_ROI_CODER_LAUNCHES] += 1;
        for (int l = 0; l < k.planes; l++) if (!reorder(l)) return fail(WR_ERR_ARG, "too many bricks");
    } else {
        for (int l = 0; l < k.planes; l++) {
            launch_note(c, k.ids ? "seg_decode_list" : "seg_decode", l, b.blob[l].p, k.n, b.work[l].p, k.q[l]);
            HIPCHK(hipEventRecord(b.ev[2 * l], c->stream));
            if (k.ids) wrk::seg_decode_list(b.blob[l].p, k.info->len_enc_vec[l], sym(l), k.n, s.seg[l], b.work[l].p, k.ids[l].size(), c->stream, s.brick, s.strands);
            else wrk::seg_decode(b.blob[l].p, k.info->len_enc_vec[l], sym(l), k.n, s.seg[l], b.work[l].p, c->stream, s.brick, s.strands);
            if (!reorder(l)) return fail(WR_ERR_ARG, "too many bricks");
            HIPCHK(hipEventRecord(b.ev[2 * l + 1], c->stream));
            if (k.stat_segments >= 0) g_stat[k.stat_segments] += k.ids[l].size();
            if (k.stat_launches) g_stat[WR_STAT_ROI_CODER_LAUNCHES] += 1;
        }
    }
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "segmented decoder launch failed" + launch_describe(c));
    unsigned int bad[WR_NLAYMAX] = {0};
    for (int l = 0; l < k.planes; l++) HIPCHK(hipMemcpyAsync(&bad[l], wrk::seg_work_bad(b.work[l].p), sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the segmented decoder failed on the device" + launch_describe(c));
    for (int l = 0; l < k.planes; l++)
        if (bad[l]) return fail(WR_ERR_STREAM, "plane " + std::to_string(l) + ": " + bad_segments_text(bad[l]));
    fold_coder_seconds(b, one_launch ? 1 : k.planes, tm);
    return WR_OK;
}

// ---- the drivers.  They differ in the plan (everything; one box or region: a LowresPlan; many regions), in the finisher
// (inverse_from_planes, lowres_from_planes / roi_from_planes, roi_multi_from_planes) and in where the result lands; the rest
// is the stages above, in the same order: parse, gather the planes' buffers, "up", lease the slot, coder stage, finisher, tail.
// err_out != nullptr (wr_seg_error_host): fld is the ORIGINAL field on the host and is only read; the reconstruction stays on
// the device, where it is compared with an upload of the field: *err_out = max |field - reconstruction|
// stats_out != nullptr (wr_seg_error_stats_host): likewise, the compare being wrk::err_stats and the field's min/max read too
// msk != nullptr (wr_decode_*_seg_masked): the mask blob of a masked record, judged before the result is written anywhere the
// caller can see, and applied behind the inverse transform
// stats_out and msk (wr_seg_error_stats_host_masked): the compare runs over the record's defined samples (the masked kernel, on
// the decoded mask's bits: nothing is restored), *defined_out their count; lo and hi are those of the defined samples
int decode_seg_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                    wr_timings* tm, double* err_out = nullptr, wr_error_stats* stats_out = nullptr, MaskDecode* msk = nullptr,
                    unsigned long long* defined_out = nullptr)
{
    double err_unused = 0;
    if (stats_out && !err_out) err_out = &err_unused;
    if (int rc = ctx_bind(c)) return rc;
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null field pointer");
    c->pend_valid = false;
    PlaneHold planes(c);
    SegBufs bufs(c);
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    SegStream s;
    if (int rc = seg_stream_of(nx, ny, nz, info, data_enc, data_len, &s)) return rc;
    if (msk) if (int rc = msk->parse(nx, ny, nz)) return rc;
    if (s.constant && msk) if (int rc = msk->decode_alone(c, &bufs)) return rc;
    if (s.constant && err_out) {
        std::vector<unsigned char> cbits;  // a masked record that is measured: the mask on the host
        if (msk) if (int rc = msk->host_bits(&cbits)) return rc;
        return constant_error_stats(fld, n, info->midval, msk ? cbits.data() : nullptr, msk ? n - (size_t)msk->job.info.undefined : n, err_out, stats_out, defined_out);
    }
    if (s.constant && msk) return finish_constant_masked(c, fld, n, info->midval, msk, t0, &local, tm);
    if (s.constant) return finish_constant(c, fld, n, info->midval, t0, &local, tm);
    {
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);  // one decode at a time gathers its planes (decode_impl)
        if (s.brick) {  // the plane in stream order, every plane in turn
            bufs.perm = plane_scratch(c, n);
            if (!bufs.perm.p) return WR_ERR_HIP;
        }
        for (int l = 0; l < s.nlay; l++)
            if (int rc = seg_plane_bufs(c, &bufs, l, n, info->len_enc_vec[l], wrk::seg_decode_work_bytes(s.nseg[l]), false, true)) return rc;
        if (err_out) {  // the field, next to the reconstruction
            const size_t bytes = n * (fld.host_f32 ? sizeof(float) : sizeof(double));
            bufs.trial[2] = plane_scratch(c, bytes);
            if (!bufs.trial[2].p) return WR_ERR_HIP;
            if (int rc = xfer_field(c, &c->x_field, bufs.trial[2].p, fld.host ? (const void*)fld.host : (const void*)fld.host_f32, bytes, kUp)) return rc;
        }
    }
    if (int rc = seg_upload_planes(c, s, info, data_enc, &bufs, &local.h2d_ms)) return rc;
    if (msk) if (int rc = msk->upload(c, &bufs)) return rc;
    const double t_coded = now();
    SlotNeed need;
    transform_need(nx, ny, nz, info->wlev ? -kWavLvl : 0, &need);
    if (fld.host || fld.host_f32) need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    wrk::DequantParams p;
    if (int rc = dequant_params(info, s.nlay, n, [&](int l) { return c->ps[l].ref; }, &p)) return rc;
    double* d_fld = fld.dev ? fld.dev : slot->field;
    float* d_f32 = nullptr;
    int rc = WR_OK;
    {
        StageLock cu(pool->cu_mu);
        clock_warmup(c, n);
        if (msk) if (int rc = msk->launch()) return rc;  // (on its own stream, under the field's coder stage)
        CoderCall k{&s, info, s.nlay, n, &bufs, p.q};
        for (int l = 0; l < s.nlay; l++) k.perm[l] = bufs.perm.p;
        if (int rc = seg_coder_stage(c, k, &local)) return rc;
        if (msk) if (int rc = msk->check()) return rc;
        launch_note(c, "dequant", s.nlay - 1, d_fld, n, nullptr, p.q[s.nlay - 1]);
        rc = inverse_from_planes(c, slot.get(), d_fld, nx, ny, nz, (int)info->wlev, p, fld.host_f32 ? &d_f32 : nullptr);
        if (rc == WR_OK && msk && !err_out) rc = fld.host_f32 ? msk->restore(d_f32) : msk->restore(d_fld);
        rc = kernel_stage_end(c, rc);
        if (rc == WR_OK && err_out) {
            double bad = 0;
            if (stats_out) {
                BoundedSearch::Stats st;
                double lo = 0, hi = 0;
                unsigned long long defined = n;
                float* const f32 = reinterpret_cast<float*>(bufs.trial[2].p);
                double* const f64 = reinterpret_cast<double*>(bufs.trial[2].p);
                if (msk) {
                    rc = fld.host_f32 ? BoundedSearch::compare_stats_masked(c, (const float*)f32, (const float*)d_f32, n, msk->job.bits, &st, &defined)
                                      : BoundedSearch::compare_stats_masked(c, (const double*)f64, (const double*)d_fld, n, msk->job.bits, &st, &defined);
                    // lo and hi of the defined samples: the blob's pad, their mean, stands in for the others in the field's copy
                    if (rc == WR_OK && msk->job.info.undefined) {
                        if (fld.host_f32) wrk::mask_fill(f32, n, msk->job.bits, (float)msk->job.info.pad, c->stream);
                        else wrk::mask_fill(f64, n, msk->job.bits, msk->job.info.pad, c->stream);
                        if (hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "mask fill launch failed");
                    }
                } else {
                    rc = fld.host_f32 ? BoundedSearch::compare_stats(c, (const float*)f32, (const float*)d_f32, n, &st)
                                      : BoundedSearch::compare_stats(c, (const double*)f64, (const double*)d_fld, n, &st);
                }
                if (rc == WR_OK) rc = fld.host_f32 ? read_minmax(c, (const float*)f32, n, false, &lo, &hi) : read_minmax(c, (const double*)f64, n, false, &lo, &hi);
                if (rc == WR_OK) fill_error_stats(stats_out, st.max_abs, st.bad, st.sumsq, (size_t)defined, lo, hi);
                if (defined_out) *defined_out = defined;
                *err_out = st.max_abs; bad = st.bad;
            } else {
                rc = fld.host_f32 ? BoundedSearch::compare(c, reinterpret_cast<const float*>(bufs.trial[2].p), (const float*)d_f32, n, err_out, &bad)
                                  : BoundedSearch::compare(c, reinterpret_cast<const double*>(bufs.trial[2].p), (const double*)d_fld, n, err_out, &bad);
            }
            if (rc == WR_OK && bad > 0)
                rc = fail(WR_ERR_ARG, std::to_string((unsigned long long)bad) + " difference(s) between the field and the reconstruction are not finite");
        }
    }
    if (rc) return rc;
    if (err_out) return WR_OK;
    return finish_call(c, fld, d_fld, d_f32, n, true, t0, t_coded, t_phase, &local, tm);
}

// The box of level `level` from the first planes only, or with roi != nullptr a region of it: the segments the plan needs are
// uploaded and decoded, a launch per used plane.  fld receives the plan's out_elems() elements; a region's crop comes
// through the slot (roi_from_planes).
// msk != nullptr (wr_decode_*_seg_roi_masked): the mask blob of a masked record, cropped to the region: judged before the
// result is written anywhere the caller can see, and applied behind the finisher
int decode_seg_lowres_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                           const unsigned char* data_enc, size_t data_len, wr_timings* tm, MaskDecode* msk = nullptr)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null output pointer");
    LowresPlan pl;
    if (int rc = region_plan(nx, ny, nz, level, max_planes, roi, info, &pl)) return rc;
    c->pend_valid = false;
    PlaneHold planes(c);
    SegBufs bufs(c);
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz, nbox = pl.out_elems();  // (the box's elements, or the region's)
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    // every plane's header and index, used or not, are validated (region_plan has refused what seg_stream_of would of nlay and wlev)
    SegStream s;
    if (int rc = seg_stream_of(nx, ny, nz, info, data_enc, data_len, &s)) return rc;
    if (msk) {
        if (int rc = msk->parse(nx, ny, nz)) return rc;
        msk->plan(level, roi);
    }
    if (s.constant && msk) {
        if (int rc = msk->decode_alone(c, &bufs)) return rc;
        return finish_constant_masked(c, fld, nbox, info->midval, msk, t0, &local, tm);
    }
    if (s.constant) return finish_constant(c, fld, nbox, info->midval, t0, &local, tm);
    const int used = pl.planes;
    // a blocked stream: the bricks the plan needs, the same in every plane
    std::vector<uint32_t> bricks;
    if (s.brick) {
        if (s.od.nbricks > 0x7fffffffu) return fail(WR_ERR_ARG, "too many bricks");
        pl.bricks(s.od, &bricks);
    }
    std::vector<uint32_t> ids[WR_NLAYMAX];
    seg_plane_lists(s, used, ids, [&](uint32_t seg, std::vector<uint32_t>* out) {
        if (s.brick) pl.segments_blocked(s.od, seg, out);
        else pl.segments(nx, ny, nz, seg, out);
    });
    {
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);
        if (s.brick) {
            bufs.perm = plane_scratch(c, n);
            bufs.bricks = plane_scratch(c, 4 * bricks.size() + 4);
            if (!bufs.perm.p || !bufs.bricks.p) return WR_ERR_HIP;
        }
        for (int l = 0; l < used; l++)
            if (int rc = seg_plane_bufs(c, &bufs, l, n, info->len_enc_vec[l], wrk::seg_decode_list_work_bytes(s.nseg[l], ids[l].size()), false, true)) return rc;
    }
    size_t bytes_up = 0;
    if (int rc = seg_upload_lists(c, s, used, data_enc, &bufs, ids, bricks, &local.h2d_ms, &bytes_up)) return rc;
    g_stat[pl.stat_bytes_up] += bytes_up;
    if (msk) if (int rc = msk->upload(c, &bufs)) return rc;
    const double t_coded = now();
    SlotNeed need;
    pl.need(fld.host || fld.host_f32, &need);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    wrk::DequantParams p;
    if (int rc = dequant_params(info, used, n, [&](int l) { return c->ps[l].ref; }, &p)) return rc;
    double* d_box = fld.dev ? fld.dev : slot->field;
    float* d_f32 = nullptr;
    void* d_roi = nullptr;  // where a region's crop landed
    int rc = WR_OK;
    {
        StageLock cu(pool->cu_mu);
        clock_warmup(c, pl.work_elems());
        if (msk) if (int rc = msk->launch()) return rc;  // (on its own stream, under the field's coder stage)
        CoderCall k{&s, info, used, n, &bufs, p.q};
        for (int l = 0; l < used; l++) k.perm[l] = bufs.perm.p;
        k.ids = ids;
        k.d_bricks = reinterpret_cast<const uint32_t*>(bufs.bricks.p); k.nbricks = bricks.size();
        k.stat_segments = pl.stat_segments;
        k.stat_launches = pl.roi;
        if (int rc = seg_coder_stage(c, k, &local)) return rc;
        if (msk) if (int rc = msk->check()) return rc;
        if (pl.roi) {
            launch_note(c, "dequant_window", used - 1, slot->field, pl.work_elems(), nullptr, p.q[used - 1]);
            rc = roi_from_planes(c, slot.get(), fld.dev, nx, ny, pl, p, fld.host_f32 != nullptr, &d_roi);
            d_box = reinterpret_cast<double*>(d_roi); d_f32 = reinterpret_cast<float*>(d_roi);
        } else {
            launch_note(c, "dequant_box", used - 1, d_box, nbox, nullptr, p.q[used - 1]);
            rc = lowres_from_planes(c, slot.get(), d_box, nx, ny, pl, p, fld.host_f32 ? &d_f32 : nullptr);
        }
        if (rc == WR_OK && msk) rc = fld.host_f32 ? msk->restore(d_f32) : msk->restore(d_box);
        rc = kernel_stage_end(c, rc);
    }
    if (rc) return rc;
    return finish_call(c, fld, d_box, d_f32, nbox, true, t0, t_coded, t_phase, &local, tm);
}

// ---- transcoding: the planes of a coded field from one stream format to another (include/waverange_amd.h, wr_transcode.h)
// No transform, no quantizer, no work-space slot: the source's decoder fills the context's device planes, the target's coder
// reads them.  The halves are the drivers' above -- ref_decode_planes or the coder stage of decode_seg_impl, then the coder
// stage of encode_seg_impl or encode_impl's placement and tail (RefPlacement, run_plane_jobs, ref_stream_tail) -- with every
// plane ready at once.
//
// A plane's second role.  A plane that the host coder touches lives behind a ring of pinned windows that plane_prepare arms
// for ONE direction.  Here a plane may be written through upload windows (a reference source) or by a decoder kernel (a
// segmented source) and then read through download windows (a reference target).  The second plane_prepare(decode = false)
// keeps the plane's storage only if the layout it wants is the layout the plane has, so a plane that will be read through
// windows is laid out for windows when it is first prepared, whoever fills it.  It is re-armed only when nothing is in
// flight on it: a host decoder has waited for its last upload inside its end-of-stream request, a decoder kernel is behind a
// stream synchronisation.  The re-arming starts a new generation (wr_handover.h), resets the ring, and lets the encoder
// drain the plane chunk by chunk as it does after a quantizer.
int transcode_impl(wr_ctx* c, int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg_t,
                   unsigned brick_t, unsigned strands_t, wr_enc_info* info_out, unsigned char* data_out, size_t cap, wr_timings* tm)
{
    if (!c) return fail(WR_ERR_ARG, "null context");
    wrtc::Source s;
    {
        std::string why;
        if (int rc = wrtc::validate(nx, ny, nz, info_in, data_in, len_in, format, seg_t, brick_t, strands_t, info_out, data_out, cap, &s, &why)) return fail(rc, why);
    }
    if (int rc = ctx_bind(c)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    const double t0 = now();
    wr_timings local; memset(&local, 0, sizeof local);
    c->pend_valid = false;  // planes a wr_decode_begin parked in this context do not survive a transcode on it
    PlaneHold planes(c);
    SegBufs sbufs(c), tbufs(c);  // the source's blobs and decoder tables; the target's blobs, staging (or histograms) and the stream-order plane
    if (s.trivial) {  // the header is the field
        const wr_enc_info keep = *info_in;
        *info_out = keep;
        local.total = now() - t0;
        if (tm) *tm = local;
        return WR_OK;
    }
    const size_t n = s.n;
    const int nlay = s.nlay;
    const wrtc::StreamFormat& t = s.target;
    const bool ref_target = t.format == WR_FORMAT_REF;
    DevPool* const pool = c->pool;
    const int dev = c->device;
    double gpu_s = 0;
    if ((s.brick || (!ref_target && t.brick)) && !tbufs.perm.p) {  // one plane in stream order, for both halves in turn
        tbufs.perm = plane_scratch(c, n);
        if (!tbufs.perm.p) return WR_ERR_HIP;
    }

    // ---- source half: the planes into c->ps[l]
    if (s.format == WR_FORMAT_REF) {
        if (int rc = ref_decode_planes(c, info_in, nlay, n, data_in, s.off, "transcode: ", &local)) return rc;
    } else {
        // validation has passed (wrtc::validate): the "up" and coder stages of the full decode.  A plane the host encoder will
        // read is laid out for its windows from the start.
        const SegStream ss = seg_stream_of(s, nx, ny, nz, (int)info_in->wlev);
        {
            std::lock_guard<std::mutex> gather(pool->planes.gather_mu);
            for (int l = 0; l < nlay; l++)
                if (int rc = seg_plane_bufs(c, &sbufs, l, n, info_in->len_enc_vec[l], wrk::seg_decode_work_bytes(ss.nseg[l]), ref_target, true)) return rc;
        }
        if (int rc = seg_upload_planes(c, ss, info_in, data_in, &sbufs, &local.h2d_ms)) return rc;
        const double t_stage = now();
        StageLock cu(pool->cu_mu);
        clock_warmup(c, n);
        wrk::PlaneRef q[WR_NLAYMAX];
        if (int rc = plane_refs(nlay, n, [&](int l) { return c->ps[l].ref; }, q)) return rc;
        // the target's coder only runs on planes whose every segment decoded
        CoderCall k{&ss, info_in, nlay, n, &sbufs, q};
        for (int l = 0; l < nlay; l++) k.perm[l] = tbufs.perm.p;
        const int rc = seg_coder_stage(c, k, &local);
        pool->last_stage_end.store(now());
        if (rc) return rc;
        gpu_s += now() - t_stage;
    }

    // ---- target half
    size_t lens[WR_NLAYMAX] = {0};
    if (!ref_target) {
        // the coder stage of encode_seg_impl with every plane ready at once, then its "down" stage
        SegTarget st;
        if (int rc = seg_target(c, &tbufs, n, t.seg, t.brick, t.strands, t.brick ? wrblk::order_of(nx, ny, nz, (int)info_in->wlev, t.brick) : wrblk::Order{}, &st)) return rc;
        for (int l = 0; l < nlay; l++)
            if (int rc = tbufs.coded_plane(l, st.blob_cap)) return rc;
        const double t_stage = now();
        {
            StageLock cu(pool->cu_mu);
            for (int l = 0; l < nlay; l++)
                if (int rc = seg_encode_plane(c, st, c->ps[l].ref, n, l, tbufs.blob[l].p, tbufs.ev)) return rc;
            if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the segmented coder failed on the device" + launch_describe(c));
            pool->last_stage_end.store(now());
        }
        size_t total = 0;
        if (int rc = seg_coded_lengths(nlay, st.blob_cap, [&](int l) { return seg_result_host(c, l); }, lens, &total)) return rc;
        if (total > cap) return fail(WR_ERR_OVERFLOW, wrtc::kTooLarge);
        if (int rc = seg_download_blobs(c, tbufs, nlay, lens, data_out, &local)) return rc;
        gpu_s += now() - t_stage;
    } else {
        // block histograms of every plane, then the placement and concatenation of encode_impl with all planes ready
        const size_t hist_per_plane = (n / wrrc::kBlock + 1) * 256;
        if (int rc = ensure_host_hist(c, hist_per_plane * WR_NLAYMAX)) return rc;
        tbufs.stage = plane_scratch(c, hist_per_plane * (size_t)nlay * sizeof(uint16_t));  // (the device histograms: a reference target stages nothing else)
        if (!tbufs.stage.p) return WR_ERR_HIP;
        uint16_t* const d_hist = reinterpret_cast<uint16_t*>(tbufs.stage.p);
        const double t_stage = now();
        {
            StageLock cu(pool->cu_mu);
            for (int l = 0; l < nlay; l++) {
                launch_note(c, "hist", l, d_hist + l * hist_per_plane, n, nullptr, c->ps[l].ref);
                wrk::block_histograms(c->ps[l].ref, n, d_hist + l * hist_per_plane, c->stream);
            }
            if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "histogram launch failed" + launch_describe(c));
            if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the histogram stage failed on the device" + launch_describe(c));
            pool->last_stage_end.store(now());
        }
        gpu_s += now() - t_stage;
        for (int l = 0; l < nlay; l++) {
            const Piece pc = {c->h_hist + l * hist_per_plane, d_hist + l * hist_per_plane, hist_per_plane * sizeof(uint16_t)};
            if (int rc = xfer_start(c, &c->x_plane[l], &pc, 1, kDown)) { for (int k = 0; k < l; k++) (void)xfer_wait(&c->x_plane[k]); return rc; }
        }
        bool hist_failed = false;
        for (int l = 0; l < nlay; l++) {
            if (xfer_wait(&c->x_plane[l]) != WR_OK) hist_failed = true;
            local.d2h_ms += (float)c->x_plane[l].ms;
        }
        if (hist_failed) return fail(WR_ERR_HIP, "download of the block histograms failed");
        // the second role: the planes are complete and nothing is in flight on them (see above)
        for (int l = 0; l < nlay; l++) {
            if (int rc = plane_prepare(c, l, n, false)) return rc;
            if (!wrk::plane_ref_covers(c->ps[l].ref, n)) return fail(WR_ERR_HIP, "internal: the device buffer of plane " + std::to_string(l) + " has a hole");
        }
        // every plane is placed and handed over at once (RefPlacement)
        RefPlacement placement;
        wrrc::PlaneJob jobs[WR_NLAYMAX];
        for (int l = 0; l < nlay; l++) {
            uint8_t* dst = nullptr;
            if (int rc = placement.place(c, (unsigned)l, c->h_hist + l * hist_per_plane, n, data_out, cap, &dst)) return rc;
            ref_encode_job(c, (unsigned)l, n, c->h_hist + l * hist_per_plane, placement, dst, &jobs[l]);
        }
        for (int l = 0; l < nlay; l++) plane_prefetch(c, l);
        if (int rc = run_plane_jobs(jobs, nlay, encoder_threads(), dev, nullptr, "transcode: ")) return rc;
        size_t total = 0;
        if (int rc = ref_stream_tail(c, jobs, (unsigned)nlay, [&](unsigned l) { return c->ps[l].err != 0; }, placement, data_out, cap, wrtc::kTooLarge, lens, &total))
            return rc;
        for (int l = 0; l < nlay; l++) local.d2h_ms += (float)c->ps[l].copy_ms;
        local.rangecoder += fold_plane_seconds(jobs, nlay, &local);  // (behind the source half)
    }
    wrtc::finish_info(*info_in, lens, nlay, info_out);
    local.total = now() - t0;
    local.gpu = gpu_s;
    local.transfer = local.total - local.rangecoder;  // uploads, downloads, placement and concatenation
    if (local.transfer < 0) local.transfer = 0;
    if (tm) *tm = local;
    return WR_OK;
}

// The front of a blob in device memory for a stage call: its header comes to the host, then -- once check_index has seen that
// the index fits into the blob -- header and index, and both are validated before anything is launched.  blocked: the call
// decodes WRS2 blobs beside WRS1; no_strands: nullptr if it decodes WRS3 blobs too, else the words it refuses one with (nothing
// else of the blob has been looked at then).  Every refusal is made here, with `who` ("job 3: ") in front.
struct Front {
    std::vector<uint8_t> bytes;
    uint32_t seg = 0, nseg = 0, brick = 0, strands = 0;
};

int fetch_front(const unsigned char* d_blob, size_t blob_len, size_t n, bool blocked, const char* no_strands, const std::string& who, Front* f)
{
    if (blob_len < wrseg::kHeaderBytes) return fail(WR_ERR_STREAM, who + "segmented plane: shorter than its header");
    f->bytes.resize(blocked ? std::min(blob_len, wrseg::kHeaderBytesBlocked) : wrseg::kHeaderBytes);
    HIPCHK(hipMemcpy(f->bytes.data(), d_blob, f->bytes.size(), hipMemcpyDeviceToHost));
    const bool wrs3 = memcmp(f->bytes.data(), wrseg::kMagicStrands, 4) == 0;
    if (wrs3 && no_strands) return fail(WR_ERR_UNSUPPORTED, who + no_strands);
    if (wrs3 && blob_len >= wrseg::kHeaderBytesStrands) {
        f->bytes.resize(wrseg::kHeaderBytesStrands);
        HIPCHK(hipMemcpy(f->bytes.data(), d_blob, f->bytes.size(), hipMemcpyDeviceToHost));
    }
    auto check = [&]() {
        const uint8_t* const b = f->bytes.data();
        if (wrs3) return wrseg::check_index(b, f->bytes.size(), blob_len, n, &f->seg, &f->nseg, &f->brick, &f->strands);
        if (blocked) return wrseg::check_index(b, f->bytes.size(), blob_len, n, &f->seg, &f->nseg, &f->brick);
        return wrseg::check_index(b, f->bytes.size(), blob_len, n, &f->seg, &f->nseg);
    };
    const char* why = check();
    if (why == wrseg::kIndexNotAvailable) {  // (the index fits into the blob: check_index has looked)
        const size_t head = wrs3 ? wrseg::kHeaderBytesStrands : memcmp(f->bytes.data(), wrseg::kMagicBlocked, 4) == 0 ? wrseg::kHeaderBytesBlocked : wrseg::kHeaderBytes;
        f->bytes.resize(head + 4 * (size_t)wrseg::get_u32(f->bytes.data() + 8));
        HIPCHK(hipMemcpy(f->bytes.data(), d_blob, f->bytes.size(), hipMemcpyDeviceToHost));
        why = check();
    }
    return why ? fail(WR_ERR_STREAM, who + why) : WR_OK;
}

}  // namespace

extern "C" {

// one plane, as it stands, into the caller's blob buffer: strands == 0 a WRS1 blob, otherwise WRS3 in the natural order
static int dev_seg_encode(wr_ctx* c, const unsigned char* d_sym, size_t n, unsigned seg, unsigned strands, unsigned char* d_blob, size_t cap, size_t* blob_len)
{
    if (int rc = seg_format_params(&seg, 0, strands)) return rc;
    if (int rc = ctx_bind(c)) return rc;
    if (!d_blob || !blob_len || (n && !d_sym)) return fail(WR_ERR_ARG, "null pointer");
    if (((uintptr_t)d_sym | (uintptr_t)d_blob) & 15) return fail(WR_ERR_ARG, "plane and blob buffers must be 16-byte aligned");
    const size_t nseg = wrseg::seg_count(n, seg);
    if (nseg > 0xffffffffu) return fail(WR_ERR_ARG, "too many segments");
    if (cap < wrseg::header_bytes(0, strands) + 4 * nseg) return fail(WR_ERR_OVERFLOW, "the blob buffer does not hold the plane's index");
    std::lock_guard<std::mutex> lk(c->mu);
    SegBufs bufs(c);
    SegTarget t;
    if (int rc = seg_target(c, &bufs, n, seg, 0, strands, wrblk::Order{}, &t)) return rc;
    StageLock cu(c->pool->cu_mu);
    seg_encode_launch(c, t, wrk::plane_ref(d_sym), n, d_blob, cap, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    const unsigned long long len = seg_result_host(c, 0)[0], bad = seg_result_host(c, 0)[1];
    if (bad) return fail(WR_ERR_HIP, strands ? "internal: a record outgrew the record bound" : std::string("internal: ") + kOutgrew);
    if (len > cap) return fail(WR_ERR_OVERFLOW, "the blob buffer is too small for the plane");
    *blob_len = (size_t)len;
    return WR_OK;
}

int wr_dev_seg_encode(wr_ctx* c, const unsigned char* d_sym, size_t n, unsigned seg, unsigned char* d_blob, size_t cap, size_t* blob_len)
{
    return dev_seg_encode(c, d_sym, n, seg, 0, d_blob, cap, blob_len);
}

int wr_dev_seg_encode_strands(wr_ctx* c, const unsigned char* d_sym, size_t n, unsigned seg, unsigned strands, unsigned char* d_blob, size_t cap,
                              size_t* blob_len)
{
    return dev_seg_encode(c, d_sym, n, seg, strands ? strands : WR_STRANDS_DEFAULT, d_blob, cap, blob_len);
}

int wr_dev_seg_decode(wr_ctx* c, const unsigned char* d_blob, size_t blob_len, unsigned char* d_sym, size_t n, size_t* bad_segments)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!d_blob || (n && !d_sym)) return fail(WR_ERR_ARG, "null pointer");
    if (((uintptr_t)d_sym | (uintptr_t)d_blob) & 15) return fail(WR_ERR_ARG, "plane and blob buffers must be 16-byte aligned");
    if (bad_segments) *bad_segments = 0;
    std::lock_guard<std::mutex> lk(c->mu);
    Front f;  // (a WRS3 blob's symbols come out in stream order)
    if (int rc = fetch_front(d_blob, blob_len, n, false, nullptr, std::string(), &f)) return rc;
    if (!f.nseg) return WR_OK;
    SegBufs bufs(c);
    bufs.work[0] = plane_scratch(c, wrk::seg_decode_work_bytes(f.nseg));
    if (!bufs.work[0].p) return WR_ERR_HIP;
    if (int rc = seg_upload_offsets(f.bytes.data(), wrseg::header_bytes(0, f.strands), f.nseg, bufs.work[0].p)) return rc;
    StageLock cu(c->pool->cu_mu);
    wrk::seg_decode(d_blob, blob_len, wrk::plane_ref(d_sym), n, f.seg, bufs.work[0].p, c->stream, 0, f.strands);
    HIPCHK(hipGetLastError());
    unsigned int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, wrk::seg_work_bad(bufs.work[0].p), sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad_segments) *bad_segments = bad;
    if (bad) return fail(WR_ERR_STREAM, "segmented plane: " + bad_segments_text(bad));
    return WR_OK;
}

int wr_encode_host_seg(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                       unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (written only with wr_ctx_set_keep_residual(ctx, 1), as wr_encode_host)
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, 0, 0, info, data_enc, cap, tm);
}

int wr_decode_host_seg(wr_ctx* c, double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                       wr_timings* tm)
{
    FieldRef f; f.host = h_fld;
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

int wr_encode_host_seg_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                           unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, 0, 0, info, data_enc, cap, tm);
}

int wr_decode_host_seg_f32(wr_ctx* c, float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                           wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_fld;
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

int wr_encode_device_seg(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec, unsigned seg,
                         wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, 0, 0, info, data_enc, cap, tm);
}

// ---- encode to a byte budget (the search: BudgetSearch above)
static int encode_seg_budget(wr_ctx* c, FieldRef f, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes, double tol_min,
                             unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm, wr_budget_result* res,
                             MaskEncode* msk = nullptr)
{
    if (!res) return fail(WR_ERR_ARG, "null wr_budget_result");
    if (!(tol_min > 0) || tol_min > DBL_MAX) return fail(WR_ERR_ARG, "tol_min must be a positive number");
    if (mx < 1 || my < 1 || mz < 1) return fail(WR_ERR_ARG, "bad local cutoff description");
    if ((long long)mx * my * mz > 1) return fail(WR_ERR_UNSUPPORTED, "an encode to a byte budget takes no local cutoff (mx * my * mz > 1)");
    BudgetSearch bud;
    bud.max_bytes = max_bytes;
    bud.g_min = wrbud::grid_index(tol_min);
    const double t_min = wrbud::grid_tol(bud.g_min);  // (the loop's tolerance until the search sets it; a constant field never gets there)
    Cutoff cut; cut.vec = &t_min;
    memset(res, 0, sizeof *res);
    const int rc = encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, 0, 0, info, data_enc, cap, tm, &bud, nullptr, msk);
    res->probe_passes = bud.passes;
    if (rc) return rc;
    if (info->nlay == 0) { bud.g = bud.g_min; bud.bound = 0; }
    if (bud.g < 0) return fail(WR_ERR_HIP, "internal: the budget search chose no tolerance");
    res->g = bud.g;
    res->tolrel = wrbud::grid_tol(bud.g);
    res->bound = bud.bound;
    return WR_OK;
}

int wr_encode_host_seg_budget(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes, double tol_min,
                              unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm, wr_budget_result* res)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (never written: the residual is not kept)
    return encode_seg_budget(c, f, nx, ny, nz, wtflag, mx, my, mz, max_bytes, tol_min, seg, info, data_enc, cap, tm, res);
}

int wr_encode_host_seg_budget_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes,
                                  double tol_min, unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                                  wr_budget_result* res)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_budget(c, f, nx, ny, nz, wtflag, mx, my, mz, max_bytes, tol_min, seg, info, data_enc, cap, tm, res);
}

int wr_encode_device_seg_budget(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes, double tol_min,
                                unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm, wr_budget_result* res)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_budget(c, f, nx, ny, nz, wtflag, mx, my, mz, max_bytes, tol_min, seg, info, data_enc, cap, tm, res);
}

// ---- encode to an error bound (the search: BoundedSearch above)
static int encode_seg_bounded(wr_ctx* c, FieldRef f, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err, double tol_min,
                              unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                              wr_bounded_result* res)
{
    if (!res) return fail(WR_ERR_ARG, "null wr_bounded_result");
    if (!(max_abs_err > 0) || max_abs_err > DBL_MAX) return fail(WR_ERR_ARG, "max_abs_err must be a positive finite number");
    if (!(tol_min > 0) || tol_min > DBL_MAX) return fail(WR_ERR_ARG, "tol_min must be a positive number");
    if (mx < 1 || my < 1 || mz < 1) return fail(WR_ERR_ARG, "bad local cutoff description");
    if ((long long)mx * my * mz > 1) return fail(WR_ERR_UNSUPPORTED, "an encode to an error bound takes no local cutoff (mx * my * mz > 1)");
    BoundedSearch bnd;
    bnd.max_err = max_abs_err;
    bnd.g_min = wrbud::grid_index(tol_min);
    const double t_min = wrbud::grid_tol(bnd.g_min);  // (the loop's tolerance until the search sets it; a constant field never gets there)
    Cutoff cut; cut.vec = &t_min;
    memset(res, 0, sizeof *res);
    const int rc = encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands, info, data_enc, cap, tm, nullptr, &bnd);
    res->trials = bnd.trials;
    if (c) for (int k = 0; k < 3; k++) c->bounded_ms[k] = bnd.ms[k];
    if (rc) return rc;
    if (info->nlay == 0) { bnd.g = wrbud::kGMax; bnd.err = 0; }
    if (bnd.g < 0) return fail(WR_ERR_HIP, "internal: the search of an encode to an error bound chose no tolerance");
    res->g = bnd.g;
    res->tolrel = wrbud::grid_tol(bnd.g);
    res->err = bnd.err;
    return WR_OK;
}

int wr_encode_host_seg_bounded(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err, double tol_min,
                               unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                               wr_bounded_result* res)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (never written: the residual is not kept)
    return encode_seg_bounded(c, f, nx, ny, nz, wtflag, mx, my, mz, max_abs_err, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

int wr_encode_host_seg_bounded_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err,
                                   double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                   wr_timings* tm, wr_bounded_result* res)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_bounded(c, f, nx, ny, nz, wtflag, mx, my, mz, max_abs_err, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

int wr_encode_device_seg_bounded(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err, double tol_min,
                                 unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                                 wr_bounded_result* res)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_bounded(c, f, nx, ny, nz, wtflag, mx, my, mz, max_abs_err, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

static int seg_error(wr_ctx* c, FieldRef f, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, double* err)
{
    if (!err) return fail(WR_ERR_ARG, "null result pointer");
    if (f.none()) return fail(WR_ERR_ARG, "null field pointer");
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, nullptr, err);
}

int wr_seg_error_host(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                      double* err)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (only read: decode_seg_impl's err_out)
    return seg_error(c, f, nx, ny, nz, info, data_enc, data_len, err);
}

int wr_seg_error_host_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                          double* err)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return seg_error(c, f, nx, ny, nz, info, data_enc, data_len, err);
}

// ---- encode to an RMS or PSNR target: BoundedSearch in the L2 norm
static int encode_seg_quality(wr_ctx* c, FieldRef f, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target, double tol_min,
                              unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                              wr_quality_result* res, MaskEncode* msk = nullptr)
{
    if (!res) return fail(WR_ERR_ARG, "null wr_quality_result");
    if (norm != WR_NORM_MAX && norm != WR_NORM_RMS && norm != WR_NORM_PSNR) return fail(WR_ERR_ARG, "norm must be WR_NORM_MAX, WR_NORM_RMS or WR_NORM_PSNR");
    if (!(target > 0) || target > DBL_MAX) return fail(WR_ERR_ARG, "the quality target must be a positive finite number");
    if (!(tol_min > 0) || tol_min > DBL_MAX) return fail(WR_ERR_ARG, "tol_min must be a positive number");
    if (mx < 1 || my < 1 || mz < 1) return fail(WR_ERR_ARG, "bad local cutoff description");
    if ((long long)mx * my * mz > 1) return fail(WR_ERR_UNSUPPORTED, "an encode to a quality target takes no local cutoff (mx * my * mz > 1)");
    BoundedSearch bnd;
    bnd.quality = true;
    bnd.norm = norm;
    if (norm == WR_NORM_PSNR) bnd.psnr_db = target;  // (max_err: from the prologue's range, in run())
    else bnd.max_err = target;
    bnd.g_min = wrbud::grid_index(tol_min);
    const double t_min = wrbud::grid_tol(bnd.g_min);
    Cutoff cut; cut.vec = &t_min;
    memset(res, 0, sizeof *res);
    const int rc = encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands, info, data_enc, cap, tm, nullptr, &bnd, msk);
    res->trials = bnd.trials;
    if (c) for (int k = 0; k < 3; k++) c->bounded_ms[k] = bnd.ms[k];
    if (rc) return rc;
    BoundedSearch::Stats st;
    if (info->nlay == 0) {  // a constant field: the search never ran
        bnd.g = wrbud::kGMax;
        bnd.range = 2 * info->halfspanval;
        if (norm == WR_NORM_PSNR) {
            if (!(bnd.range > 0)) return fail(WR_ERR_ARG, "a PSNR target needs a field whose range hi - lo is a positive finite number");
            bnd.max_err = bnd.range * pow(10.0, -target / 20.0);
        }
    } else {
        if (bnd.g < 0) return fail(WR_ERR_HIP, "internal: the search of an encode to a quality target chose no tolerance");
        if (norm == WR_NORM_MAX) { st.max_abs = bnd.err; st.sumsq = st.rms = NAN; }
        else st = bnd.seen[bnd.g];
    }
    res->g = bnd.g;
    res->tolrel = wrbud::grid_tol(bnd.g);
    res->max_abs = st.max_abs; res->rms = st.rms; res->sumsq = st.sumsq;
    res->range = bnd.range;
    res->psnr = norm == WR_NORM_MAX && info->nlay ? NAN : psnr_of(bnd.range, st.rms);
    res->max_rms = norm == WR_NORM_MAX ? NAN : bnd.max_err;
    return WR_OK;
}

int wr_encode_host_seg_quality(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                               double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                               wr_timings* tm, wr_quality_result* res)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (never written: the residual is not kept)
    return encode_seg_quality(c, f, nx, ny, nz, wtflag, mx, my, mz, norm, target, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

int wr_encode_host_seg_quality_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                                   double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                   wr_timings* tm, wr_quality_result* res)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_quality(c, f, nx, ny, nz, wtflag, mx, my, mz, norm, target, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

int wr_encode_device_seg_quality(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                                 double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                 wr_timings* tm, wr_quality_result* res)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_quality(c, f, nx, ny, nz, wtflag, mx, my, mz, norm, target, tol_min, seg, brick, strands, info, data_enc, cap, tm, res);
}

static int seg_error_stats(wr_ctx* c, FieldRef f, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                           wr_error_stats* stats)
{
    if (!stats) return fail(WR_ERR_ARG, "null result pointer");
    if (f.none()) return fail(WR_ERR_ARG, "null field pointer");
    memset(stats, 0, sizeof *stats);
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, nullptr, nullptr, stats);
}

int wr_seg_error_stats_host(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                            size_t data_len, wr_error_stats* stats)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (only read)
    return seg_error_stats(c, f, nx, ny, nz, info, data_enc, data_len, stats);
}

int wr_seg_error_stats_host_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                                size_t data_len, wr_error_stats* stats)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return seg_error_stats(c, f, nx, ny, nz, info, data_enc, data_len, stats);
}

int wr_dev_err_stats(wr_ctx* c, const double* d_a, const double* d_b, size_t n, wr_error_stats* stats) { return BoundedSearch::stage_stats(c, d_a, d_b, n, stats); }
int wr_dev_err_stats_f32(wr_ctx* c, const float* d_a, const float* d_b, size_t n, wr_error_stats* stats) { return BoundedSearch::stage_stats(c, d_a, d_b, n, stats); }

int wr_ctx_bounded_trial_ms(wr_ctx* c, double* requant_ms, double* inverse_ms, double* compare_ms)
{
    if (!c) return fail(WR_ERR_ARG, "null context");
    if (requant_ms) *requant_ms = c->bounded_ms[0];
    if (inverse_ms) *inverse_ms = c->bounded_ms[1];
    if (compare_ms) *compare_ms = c->bounded_ms[2];
    return WR_OK;
}

int wr_dev_requant_accum(wr_ctx* c, const double* d_coef, size_t n, int nlay, const double* deps, const double* minval, double* d_acc)
{
    if (nlay < 1 || nlay > WR_NLAYMAX) return fail(WR_ERR_ARG, "a coefficient sum takes 1 to " + std::to_string(WR_NLAYMAX) + " planes");
    if (int rc = ctx_bind(c)) return rc;
    if (!deps || !minval || (n && (!d_coef || !d_acc))) return fail(WR_ERR_ARG, "null pointer");
    if (d_coef < d_acc + n && d_acc < d_coef + n) return fail(WR_ERR_ARG, "the coefficient array and the sum overlap");
    std::lock_guard<std::mutex> lk(c->mu);
    wrk::QuantPrev prev;
    double aopt = 0, bopt = 0;
    for (int l = 0; l < nlay; l++) {  // plane_step's expressions
        aopt = 1.0 / deps[l];
        bopt = -minval[l] * aopt + 0.5;
        if (l + 1 < nlay) prev.push(aopt, bopt, deps[l], minval[l]);
    }
    StageLock cu(c->pool->cu_mu);
    wrk::requant_accum(d_coef, n, prev, aopt, bopt, deps[nlay - 1], minval[nlay - 1], d_acc, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return WR_OK;
}

int wr_dev_plane_size_bound(wr_ctx* c, const unsigned char* d_sym, size_t n, unsigned seg, size_t* bound)
{
    if (int rc = seg_format_params(&seg, 0, 0)) return rc;
    if (int rc = ctx_bind(c)) return rc;
    if (!bound || (n && !d_sym)) return fail(WR_ERR_ARG, "null pointer");
    if ((uintptr_t)d_sym & 15) return fail(WR_ERR_ARG, "the plane must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = BudgetSearch::tables(c)) return rc;
    StageLock cu(c->pool->cu_mu);
    wrk::plane_bound(d_sym, n, seg, c->d_bound_tab, wrbud::tables().fixed, c->d_bound_tot, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(BudgetSearch::totals_host(c), c->d_bound_tot, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *bound = wrbud::blob_overhead(wrseg::seg_count(n, seg)) + (size_t)BudgetSearch::totals_host(c)[0];
    return WR_OK;
}

int wr_dev_quant_size_probe(wr_ctx* c, const double* d_resid, size_t n, double minval, int ncand, const double* deps, unsigned seg, size_t* bounds)
{
    if (int rc = seg_format_params(&seg, 0, 0)) return rc;
    if (ncand < 1 || ncand > wrk::kProbeK) return fail(WR_ERR_ARG, "a size probe takes 1 to " + std::to_string(wrk::kProbeK) + " candidate steps");
    if (int rc = ctx_bind(c)) return rc;
    if (!bounds || !deps || (n && !d_resid)) return fail(WR_ERR_ARG, "null pointer");
    if ((uintptr_t)d_resid & 15) return fail(WR_ERR_ARG, "the residual array must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = BudgetSearch::tables(c)) return rc;
    wrk::ProbeCands cd;
    cd.n = ncand;
    for (int k = 0; k < ncand; k++) {  // plane_step's expressions
        cd.aopt[k] = 1.0 / deps[k];
        cd.bopt[k] = -minval * cd.aopt[k] + 0.5;
    }
    StageLock cu(c->pool->cu_mu);
    return BudgetSearch::launch(c, c->stream, d_resid, n, seg, wrk::QuantPrev(), cd, false, bounds);
}

int wr_decode_device_seg(wr_ctx* c, double* d_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                         wr_timings* tm)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
}

// ---- masked fields: the stage calls and the whole-path calls (MaskEncode / MaskDecode above)
int wr_dev_mask_split(wr_ctx* c, const double* d_fld, size_t n, double below, unsigned char* d_bits, unsigned long long* undefined, double* pad)
{
    return dev_mask_split(c, d_fld, n, below, d_bits, undefined, pad);
}
int wr_dev_mask_split_f32(wr_ctx* c, const float* d_fld, size_t n, double below, unsigned char* d_bits, unsigned long long* undefined, double* pad)
{
    return dev_mask_split(c, d_fld, n, below, d_bits, undefined, pad);
}
int wr_dev_mask_fill(wr_ctx* c, double* d_fld, size_t n, const unsigned char* d_bits, double value) { return dev_mask_apply(c, d_fld, n, d_bits, value, nullptr); }
int wr_dev_mask_fill_f32(wr_ctx* c, float* d_fld, size_t n, const unsigned char* d_bits, double value) { return dev_mask_apply(c, d_fld, n, d_bits, value, nullptr); }
int wr_dev_mask_restore(wr_ctx* c, double* d_fld, size_t n, const unsigned char* d_bits, double fill, unsigned long long* undefined)
{
    if (!undefined) return fail(WR_ERR_ARG, "null pointer");
    return dev_mask_apply(c, d_fld, n, d_bits, fill, undefined);
}
int wr_dev_mask_restore_f32(wr_ctx* c, float* d_fld, size_t n, const unsigned char* d_bits, double fill, unsigned long long* undefined)
{
    if (!undefined) return fail(WR_ERR_ARG, "null pointer");
    return dev_mask_apply(c, d_fld, n, d_bits, fill, undefined);
}

static int encode_seg_masked(wr_ctx* c, FieldRef f, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec, unsigned seg,
                             unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                             wr_mask_result* res)
{
    if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    MaskEncode m;
    m.below = below;
    const int rc = encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands, info, data_enc, cap, tm, nullptr, nullptr, &m);
    if (rc == WR_OK) m.result(res);
    return rc;
}

static int decode_seg_masked(wr_ctx* c, FieldRef f, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                             double fill, wr_timings* tm, wr_mask_result* res)
{
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    if (res) memset(res, 0, sizeof *res);
    if (data_len == 0 || data_len <= info->ntot_enc)  // an unmasked record (a shorter buffer: the plain call refuses it)
        return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, tm);
    if (!data_enc) return fail(WR_ERR_ARG, "null coded buffer");
    MaskDecode m;
    m.job.blob = data_enc + info->ntot_enc; m.job.len = data_len - info->ntot_enc; m.fill = fill;
    const int rc = decode_seg_impl(c, f, nx, ny, nz, info, data_enc, info->ntot_enc, tm, nullptr, nullptr, &m);
    if (rc == WR_OK) m.result(res);
    return rc;
}

int wr_encode_host_seg_masked(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                              unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                              wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (written only with wr_ctx_set_keep_residual(ctx, 1), as wr_encode_host)
    return encode_seg_masked(c, f, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, seg, brick, strands, below, info, data_enc, cap, tm, res);
}
int wr_encode_host_seg_masked_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                  unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                  wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_masked(c, f, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, seg, brick, strands, below, info, data_enc, cap, tm, res);
}
int wr_encode_device_seg_masked(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_masked(c, f, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, seg, brick, strands, below, info, data_enc, cap, tm, res);
}
int wr_decode_host_seg_masked(wr_ctx* c, double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                              double fill, wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.host = h_fld;
    return decode_seg_masked(c, f, nx, ny, nz, info, data_enc, data_len, fill, tm, res);
}
int wr_decode_host_seg_masked_f32(wr_ctx* c, float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                                  size_t data_len, double fill, wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.host_f32 = h_fld;
    return decode_seg_masked(c, f, nx, ny, nz, info, data_enc, data_len, fill, tm, res);
}
int wr_decode_device_seg_masked(wr_ctx* c, double* d_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                                double fill, wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return decode_seg_masked(c, f, nx, ny, nz, info, data_enc, data_len, fill, tm, res);
}

// ---- masked fields in the tolerance searches: the quality and budget calls with a MaskEncode beside the search
#define WR_MASKED_SEARCH_CALLS(NAME, SUFFIX, FIELD_T, FIELD_MEMBER, CHECK)                                                                                \
    int wr_encode_##NAME##_quality_masked##SUFFIX(wr_ctx* c, FIELD_T fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target, \
                                          double tol_min, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info,            \
                                          unsigned char* data_enc, size_t cap, wr_timings* tm, wr_quality_result* res, wr_mask_result* mres)         \
    {                                                                                                                                             \
        FieldRef f; f.FIELD_MEMBER = const_cast<decltype(f.FIELD_MEMBER)>(fld);                                                                   \
        CHECK                                                                                                                                     \
        if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");                                \
        MaskEncode m;                                                                                                                             \
        m.below = below;                                                                                                                          \
        const int rc = encode_seg_quality(c, f, nx, ny, nz, wtflag, mx, my, mz, norm, target, tol_min, seg, brick, strands, info, data_enc, cap, tm, res, &m); \
        if (rc == WR_OK) m.result(mres);                                                                                                          \
        return rc;                                                                                                                                \
    }                                                                                                                                             \
    int wr_encode_##NAME##_budget_masked##SUFFIX(wr_ctx* c, FIELD_T fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes,       \
                                         double tol_min, unsigned seg, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap,        \
                                         wr_timings* tm, wr_budget_result* res, wr_mask_result* mres)                                               \
    {                                                                                                                                             \
        FieldRef f; f.FIELD_MEMBER = const_cast<decltype(f.FIELD_MEMBER)>(fld);                                                                   \
        CHECK                                                                                                                                     \
        if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");                                \
        MaskEncode m;                                                                                                                             \
        m.below = below;                                                                                                                          \
        const int rc = encode_seg_budget(c, f, nx, ny, nz, wtflag, mx, my, mz, max_bytes, tol_min, seg, info, data_enc, cap, tm, res, &m);          \
        if (rc == WR_OK) m.result(mres);                                                                                                          \
        return rc;                                                                                                                                \
    }
WR_MASKED_SEARCH_CALLS(host_seg, , const double*, host, )
WR_MASKED_SEARCH_CALLS(host_seg, _f32, const float*, host_f32, )
WR_MASKED_SEARCH_CALLS(device_seg, , double*, dev, if (!fld) return fail(WR_ERR_ARG, "null device field pointer");)
#undef WR_MASKED_SEARCH_CALLS

// the measuring half on a masked record: data_len = the field's planes + the mask blob (an unmasked record: every sample is defined)
static int seg_error_stats_masked(wr_ctx* c, FieldRef f, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                                  wr_error_stats* stats, unsigned long long* defined)
{
    if (!stats || !defined) return fail(WR_ERR_ARG, "null result pointer");
    if (f.none()) return fail(WR_ERR_ARG, "null field pointer");
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    memset(stats, 0, sizeof *stats);
    *defined = 0;
    if (data_len == 0 || data_len <= info->ntot_enc)
        return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, data_len, nullptr, nullptr, stats, nullptr, defined);
    if (!data_enc) return fail(WR_ERR_ARG, "null coded buffer");
    MaskDecode m;
    m.job.blob = data_enc + info->ntot_enc; m.job.len = data_len - info->ntot_enc;
    return decode_seg_impl(c, f, nx, ny, nz, info, data_enc, info->ntot_enc, nullptr, nullptr, stats, &m, defined);
}

int wr_seg_error_stats_host_masked(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                                   size_t data_len, wr_error_stats* stats, unsigned long long* defined)
{
    FieldRef f; f.host = const_cast<double*>(h_fld);  // (only read)
    return seg_error_stats_masked(c, f, nx, ny, nz, info, data_enc, data_len, stats, defined);
}
int wr_seg_error_stats_host_masked_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc,
                                       size_t data_len, wr_error_stats* stats, unsigned long long* defined)
{
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return seg_error_stats_masked(c, f, nx, ny, nz, info, data_enc, data_len, stats, defined);
}
int wr_dev_err_stats_masked(wr_ctx* c, const double* d_a, const double* d_b, size_t n, const unsigned char* d_bits, wr_error_stats* stats,
                            unsigned long long* defined)
{
    return BoundedSearch::stage_stats_masked(c, d_a, d_b, n, d_bits, stats, defined);
}
int wr_dev_err_stats_masked_f32(wr_ctx* c, const float* d_a, const float* d_b, size_t n, const unsigned char* d_bits, wr_error_stats* stats,
                                unsigned long long* defined)
{
    return BoundedSearch::stage_stats_masked(c, d_a, d_b, n, d_bits, stats, defined);
}

// ---- masked region and low-resolution decode: roi == nullptr is the whole box of the level
static int decode_seg_roi_masked(wr_ctx* c, FieldRef f, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                                 const unsigned char* data_enc, size_t data_len, double fill, wr_timings* tm, wr_mask_result* res)
{
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    if (res) memset(res, 0, sizeof *res);
    if (data_len == 0 || data_len <= info->ntot_enc)  // an unmasked record (a shorter buffer: the plain call refuses it)
        return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, tm);
    if (!data_enc) return fail(WR_ERR_ARG, "null coded buffer");
    MaskDecode m;
    m.job.blob = data_enc + info->ntot_enc; m.job.len = data_len - info->ntot_enc; m.fill = fill;
    const int rc = decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, info->ntot_enc, tm, &m);
    if (rc == WR_OK) m.result(res);
    return rc;
}

int wr_decode_host_seg_roi_masked(wr_ctx* c, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                                  const unsigned char* data_enc, size_t data_len, double fill, wr_timings* tm, wr_mask_result* res)
{
    FieldRef f; f.host = h_out;
    return decode_seg_roi_masked(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, fill, tm, res);
}
int wr_decode_host_seg_roi_masked_f32(wr_ctx* c, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                                      const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, double fill, wr_timings* tm,
                                      wr_mask_result* res)
{
    FieldRef f; f.host_f32 = h_out;
    return decode_seg_roi_masked(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, fill, tm, res);
}
int wr_decode_device_seg_roi_masked(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                                    const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, double fill, wr_timings* tm,
                                    wr_mask_result* res)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    return decode_seg_roi_masked(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, fill, tm, res);
}

int wr_dev_mask_restore_box(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, const wr_box* roi, const unsigned char* d_bits, double fill,
                            unsigned long long* undefined)
{
    return dev_mask_restore_box(c, d_out, nx, ny, nz, level, roi, d_bits, fill, undefined);
}
int wr_dev_mask_restore_box_f32(wr_ctx* c, float* d_out, int nx, int ny, int nz, int level, const wr_box* roi, const unsigned char* d_bits, double fill,
                                unsigned long long* undefined)
{
    return dev_mask_restore_box(c, d_out, nx, ny, nz, level, roi, d_bits, fill, undefined);
}

int wr_encode_host_seg_blocked(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                               unsigned seg, unsigned brick, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host = const_cast<double*>(h_fld);
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick ? brick : WR_BRICK_DEFAULT, 0, info, data_enc, cap, tm);
}

int wr_encode_host_seg_blocked_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                   unsigned seg, unsigned brick, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick ? brick : WR_BRICK_DEFAULT, 0, info, data_enc, cap, tm);
}

int wr_encode_device_seg_blocked(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                 unsigned seg, unsigned brick, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick ? brick : WR_BRICK_DEFAULT, 0, info, data_enc, cap, tm);
}

int wr_encode_host_seg_strands(wr_ctx* c, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                               unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host = const_cast<double*>(h_fld);
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, info, data_enc, cap, tm);
}

int wr_encode_host_seg_strands_f32(wr_ctx* c, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                   unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                   wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.host_f32 = const_cast<float*>(h_fld);
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, info, data_enc, cap, tm);
}

int wr_encode_device_seg_strands(wr_ctx* c, double* d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                                 unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm)
{
    Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvec;
    FieldRef f; f.dev = d_fld;
    if (!d_fld) return fail(WR_ERR_ARG, "null device field pointer");
    return encode_seg_impl(c, f, nx, ny, nz, wtflag, cut, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, info, data_enc, cap, tm);
}

int wr_transcode_host(wr_ctx* c, int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg,
                      unsigned brick, unsigned strands, wr_enc_info* info_out, unsigned char* data_out, size_t cap, wr_timings* tm)
{
    return transcode_impl(c, nx, ny, nz, info_in, data_in, len_in, format, seg, brick, strands, info_out, data_out, cap, tm);
}

int wr_dev_plane_reorder(wr_ctx* c, unsigned char* d_dst, const unsigned char* d_src, int nx, int ny, int nz, int wlev, unsigned brick, int inverse)
{
    if (!brick) brick = WR_BRICK_DEFAULT;
    if (int rc = seg_format_params(nullptr, brick, 0)) return rc;
    if (wlev != 0 && wlev != kWavLvl) return fail(WR_ERR_ARG, "wlev must be 0 or 4");
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_dst)) return rc;
    if (!d_dst || !d_src || d_dst == d_src) return fail(WR_ERR_ARG, "null pointer, or source and destination are the same");
    if (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) return fail(WR_ERR_ARG, "plane buffers must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, brick);
    StageLock cu(c->pool->cu_mu);
    // the natural-order side is the source of a forward reorder and the destination of an inverse one
    const bool ok = inverse ? wrk::plane_reorder(wrk::plane_ref(d_dst), const_cast<unsigned char*>(d_src), od, true, nullptr, 0, c->stream)
                            : wrk::plane_reorder(wrk::plane_ref(d_src), d_dst, od, false, nullptr, 0, c->stream);
    if (!ok) return fail(WR_ERR_ARG, "too many bricks");
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return WR_OK;
}

int wr_dev_plane_reorder_list(wr_ctx* c, unsigned char* d_dst, const unsigned char* d_src, int nx, int ny, int nz, int wlev, unsigned brick, int inverse,
                              const uint32_t* ids, size_t nlist)
{
    if (!brick) brick = WR_BRICK_DEFAULT;
    if (int rc = seg_format_params(nullptr, brick, 0)) return rc;
    if (wlev != 0 && wlev != kWavLvl) return fail(WR_ERR_ARG, "wlev must be 0 or 4");
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_dst)) return rc;
    if (!d_dst || !d_src || d_dst == d_src) return fail(WR_ERR_ARG, "null pointer, or source and destination are the same");
    if (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) return fail(WR_ERR_ARG, "plane buffers must be 16-byte aligned");
    if (nlist && !ids) return fail(WR_ERR_ARG, "null brick list");
    const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, brick);
    if (od.nbricks > 0x7fffffffu || nlist > od.nbricks) return fail(WR_ERR_ARG, "too many bricks");
    for (size_t k = 0; k < nlist; k++)
        if (ids[k] >= od.nbricks || (k && ids[k] <= ids[k - 1])) return fail(WR_ERR_ARG, "brick ids must be strictly ascending and below the plane's number of bricks");
    if (!nlist) return WR_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    uint32_t* d_ids = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&d_ids), nlist * sizeof(uint32_t)));
    StageLock cu(c->pool->cu_mu);
    hipError_t e = hipMemcpy(d_ids, ids, nlist * sizeof(uint32_t), hipMemcpyHostToDevice);
    bool ok = true;
    if (e == hipSuccess) {
        ok = inverse ? wrk::plane_reorder(wrk::plane_ref(d_dst), const_cast<unsigned char*>(d_src), od, true, d_ids, nlist, c->stream)
                     : wrk::plane_reorder(wrk::plane_ref(d_src), d_dst, od, false, d_ids, nlist, c->stream);
        if (ok) e = hipGetLastError();
        if (ok && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(d_ids);
    if (!ok) return fail(WR_ERR_ARG, "too many bricks");
    HIPCHK(e);
    return WR_OK;
}

int wr_reorder_plan(int nx, int ny, int nz, int wlev, unsigned brick, int list, wr_reorder_plan_t* out)
{
    if (!out) return fail(WR_ERR_ARG, "wr_reorder_plan: out is NULL");
    if (!brick) brick = WR_BRICK_DEFAULT;
    if (int rc = seg_format_params(nullptr, brick, 0)) return rc;
    if (wlev != 0 && wlev != kWavLvl) return fail(WR_ERR_ARG, "wlev must be 0 or 4");
    if (int rc = check_dims(nx, ny, nz, nullptr)) return rc;
    const wrblk::Order od = wrblk::order_of(nx, ny, nz, wlev, brick);
    const uint32_t group = wrk::reorder_group(od.B, list != 0);
    uint64_t first = 0;
    for (int i = 0; i < od.nbox; i++) first += wrk::reorder_box_items(od.box[i], group);
    if (first > 0x7fffffffu || od.nbricks > 0x7fffffffu) return fail(WR_ERR_ARG, "too many bricks");
    memset(out, 0, sizeof *out);
    out->group = (int)group;
    out->items = (uint32_t)first;
    out->nbricks = (uint32_t)od.nbricks;
    out->nbox = od.nbox;
    first = 0;
    for (int i = 0; i < od.nbox; i++) {
        const wrblk::Box& b = od.box[i];
        auto& o = out->box[i];
        for (int k = 0; k < 3; k++) { o.origin[k] = b.o[k]; o.extent[k] = b.e[k]; o.bricks[k] = (int)b.t[k]; }
        o.first = (uint32_t)first;
        o.first_brick = (uint32_t)b.first_brick;
        o.start = b.start;
        o.wide = wrk::reorder_box_wide(true, od, b);
        first += wrk::reorder_box_items(b, group);
    }
    return WR_OK;
}

int wr_decode_host_seg_lowres(wr_ctx* c, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info,
                              const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host = h_out;
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, nullptr, info, data_enc, data_len, tm);
}

int wr_decode_host_seg_lowres_f32(wr_ctx* c, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info,
                                  const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_out;
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, nullptr, info, data_enc, data_len, tm);
}

int wr_decode_device_seg_lowres(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info,
                                const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, nullptr, info, data_enc, data_len, tm);
}

int wr_decode_host_seg_roi(wr_ctx* c, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                           const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host = h_out;
    if (!roi) return fail(WR_ERR_ARG, "null region pointer");
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, tm);
}

int wr_decode_host_seg_roi_f32(wr_ctx* c, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                               const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_out;
    if (!roi) return fail(WR_ERR_ARG, "null region pointer");
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, tm);
}

int wr_decode_device_seg_roi(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi, const wr_enc_info* info,
                             const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    if (!roi) return fail(WR_ERR_ARG, "null region pointer");
    return decode_seg_lowres_impl(c, f, nx, ny, nz, level, max_planes, roi, info, data_enc, data_len, tm);
}

}  // extern "C"

// ---- batched segmented streams (include/waverange_amd.h): plane index l of all fields of a batch in one coder launch --------
// Transform and quantizer run field by field through the one leased slot, exactly as in encode_seg_impl / decode_seg_impl; the
// quantized planes wait in batch-owned buffers from the plane pool, and the coder kernels of wr_segbatch.hip take plane l of
// every field that has one in a single launch sequence.  No new format: every blob is the single-field call's.
namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// What a batch takes from the plane pool, piece by piece.  The drivers allocate by these and wr_seg_batch_device_bytes sums them.
size_t batch_plane_bytes(size_t n) { return wr_plane_pitch(n); }
size_t batch_perm_bytes(size_t n, unsigned brick) { return brick ? wr_plane_pitch(n) : 0; }  // per field: the plane in stream order
size_t batch_work_bytes(size_t nseg) { return wrk::seg_decode_work_bytes(nseg); }  // per decoded (field, plane): offsets and flags
// once per call.  encode: the staging of one plane index (strands != 0: at the strand stride); decode: a job table per plane
// index and a failure count per job
size_t batch_once_bytes(size_t nfields, size_t n, int nlay, unsigned seg, bool decode, unsigned strands = 0)
{
    if (!nlay) return 0;
    if (decode) return (size_t)nlay * wrk::seg_batch_table_bytes(nfields) + up256(4 * nfields * (size_t)nlay);
    return strands ? wrk::strand_batch_stage_bytes(nfields, n, seg, strands) : wrk::seg_batch_stage_bytes(nfields, n, seg);
}
// ... of a mixed decode: its jobs are all (field, plane) pairs, the plain ones (WRS1 / WRS2) and the stranded ones (WRS3) each in
// launches of at most WR_SEG_BATCH_MAX jobs, a table per launch, and a failure count per job behind the tables
size_t batch_chunk_tables_bytes(size_t njobs)
{
    size_t bytes = 0;
    for (size_t a = 0; a < njobs; a += wrsb::kBatchMax) bytes += wrk::seg_batch_table_bytes(std::min<size_t>(wrsb::kBatchMax, njobs - a));
    return bytes;
}
size_t batch_mixed_tables_bytes(size_t plain, size_t stranded) { return batch_chunk_tables_bytes(plain) + batch_chunk_tables_bytes(stranded); }
size_t batch_mixed_once_bytes(size_t plain, size_t stranded) { return batch_mixed_tables_bytes(plain, stranded) + up256(4 * (plain + stranded)); }
// pinned host memory of a call, per launch sequence (plane index): the job table, then 16 bytes per job for what comes back
struct BatchPinned {
    size_t table, per_l;
    explicit BatchPinned(size_t njobs_max) : table(wrk::seg_batch_table_bytes(njobs_max)), per_l(table + up256(16 * njobs_max)) {}
    size_t bytes(int nlay) const { return (size_t)nlay * per_l; }
    uint8_t* jobs(uint8_t* pinned, int l) const { return pinned + l * per_l; }
    unsigned long long* results(uint8_t* pinned, int l) const { return reinterpret_cast<unsigned long long*>(pinned + l * per_l + table); }
};

// the job of one plane for the batched coder kernels: its symbols in stream order into [blob, blob + cap)
wrk::SegJob seg_encode_job(const wrk::PlaneRef& sym, uint8_t* blob, size_t cap, uint32_t brick)
{
    wrk::SegJob j; memset(&j, 0, sizeof j);
    j.sym = sym; j.blob = blob; j.cap = cap; j.brick = brick;
    return j;
}

// device and pinned memory of a batch call; goes back when the call ends, behind everything the context's stream still has queued
struct BatchBufs {
    wr_ctx* c;
    std::vector<DevPlanes::Buf> taken;
    uint8_t* pinned = nullptr;      // the job tables (they stay alive until the stream has drained) and the results
    uint8_t* pinned_dev = nullptr;  // the same block as the device sees it
    PlaneEvents ev;                 // one pair per plane index
    hipStream_t also = nullptr;     // a second stream that uses the buffers (a masked batch: the masks' coder)
    explicit BatchBufs(wr_ctx* ctx) : c(ctx) {}
    BatchBufs(const BatchBufs&) = delete;
    BatchBufs& operator=(const BatchBufs&) = delete;
    ~BatchBufs()
    {
        (void)hipStreamSynchronize(c->stream);
        if (also) (void)hipStreamSynchronize(also);
        for (const DevPlanes::Buf& b : taken) c->pool->planes.give(b);
        if (pinned) (void)hipHostFree(pinned);
    }
    uint8_t* take(size_t bytes)  // nullptr: the error is set (plane_scratch)
    {
        const DevPlanes::Buf b = plane_scratch(c, bytes ? bytes : 256);
        if (b.p) taken.push_back(b);
        return b.p;
    }
    int pin(size_t bytes)
    {
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&pinned), bytes ? bytes : 256, hipHostMallocDefault));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&pinned_dev), pinned, 0));
        memset(pinned, 0, bytes);
        return WR_OK;
    }
};

// the error of a step that ran for one field (or job) of a batch: the same code, the message with the index in front
int fail_at(const char* what, int i, int rc)
{
    const std::string msg = last_error();
    return fail(rc, std::string(what) + " " + std::to_string(i) + ": " + msg);
}

constexpr unsigned long long kBatchLaneLimit = 1ull << 31;

// ---- masks across a batch of fields (wr_mask.h, "the batch forms").  The tables of the batched mask kernels and what they
// return live in a pinned block of the call's own; it goes back once the context's stream has drained.
struct MaskPinned {
    wr_ctx* c;
    uint8_t *host = nullptr, *dev = nullptr;
    explicit MaskPinned(wr_ctx* ctx) : c(ctx) {}
    MaskPinned(const MaskPinned&) = delete;
    MaskPinned& operator=(const MaskPinned&) = delete;
    ~MaskPinned()
    {
        if (!host) return;
        (void)hipStreamSynchronize(c->stream);
        (void)hipHostFree(host);
    }
    int alloc(size_t bytes)
    {
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&host), bytes ? bytes : 256, hipHostMallocDefault));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0));
        memset(host, 0, bytes);
        return WR_OK;
    }
};

// What the batched mask stages take: device memory per masked field and once per call, and the pinned tables.  The drivers
// allocate by these and wr_seg_batch_device_bytes_masked sums them.
size_t mask_batch_bits_bytes(size_t n) { return up256(wrmask::mask_bytes(n)); }
size_t mask_batch_blob_cap(size_t n, unsigned seg) { return (wr_seg_bound(wrmask::mask_bytes(n), seg) + 15) & ~(size_t)15; }  // (MaskEncode's)
size_t mask_batch_partial_bytes(size_t nfields, size_t n) { return up256(nfields * wrk::mask_split_batch_partials(n) * sizeof(double)); }
size_t mask_batch_counters_bytes(size_t nmasks) { return up256(2 * nmasks * sizeof(unsigned long long)); }
// the pinned block of a split: the items, then a (sum, count) pair per field
size_t mask_batch_split_results_at(size_t nfields) { return up256(nfields * sizeof(wrk::MaskSplitItem)); }
size_t mask_batch_split_pinned(size_t nfields) { return mask_batch_split_results_at(nfields) + up256(2 * nfields * sizeof(double)); }

// (cu_mu held, the context's stream) the split of nfields device fields in one launch pair, waited for: undefined[f] and
// pad[f] as mask_split_result forms them from field f's pair.  pin: mask_batch_split_pinned(nfields) bytes; partial:
// mask_batch_partial_bytes(nfields, n)
template <class T>
int mask_split_batch_run(wr_ctx* c, const MaskPinned& pin, double* partial, int nfields, const T* const* x, uint8_t* const* bits, size_t n, double below,
                         unsigned long long* undefined, double* pad)
{
    wrk::MaskSplitItem* const items = reinterpret_cast<wrk::MaskSplitItem*>(pin.host);
    for (int f = 0; f < nfields; f++) { items[f].x = x[f]; items[f].bits = bits[f]; }
    const size_t at = mask_batch_split_results_at(nfields);
    wrk::mask_split_batch(items, reinterpret_cast<const wrk::MaskSplitItem*>(pin.dev), nfields, sizeof(T) == sizeof(float), n, below, partial,
                          reinterpret_cast<double*>(pin.dev + at), c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched mask split launch failed");
    HIPCHK(hipStreamSynchronize(c->stream));
    const double* const res = reinterpret_cast<const double*>(pin.host + at);
    for (int f = 0; f < nfields; f++) mask_split_result<T>(res + 2 * f, n, &undefined[f], &pad[f]);
    return WR_OK;
}

// (cu_mu held, the context's stream) pad[f] into the undefined samples of every field that has one (x[f] == nullptr: skipped),
// one launch, not waited for.  pin: nfields items.  Returns the fields filled through *filled.
template <class T>
int mask_fill_batch_run(wr_ctx* c, const MaskPinned& pin, int nfields, T* const* x, const uint8_t* const* bits, size_t n, const double* values, int* filled)
{
    wrk::MaskFillItem* const items = reinterpret_cast<wrk::MaskFillItem*>(pin.host);
    int count = 0;
    for (int f = 0; f < nfields; f++) {
        if (!x[f]) continue;
        items[count].x = x[f]; items[count].bits = bits[f]; items[count].value = wrk::mask_fill_value(values[f], sizeof(T) == sizeof(float));
        count++;
    }
    *filled = count;
    if (!count) return WR_OK;
    wrk::mask_fill_batch(reinterpret_cast<const wrk::MaskFillItem*>(pin.dev), count, sizeof(T) == sizeof(float), n, c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched mask fill launch failed");
    return WR_OK;
}

const char* const kNoDefined = "no defined sample: every sample of the field is a NaN, an infinity or below the threshold";
const char* const kMeanNotFinite = "the mean of the defined samples is not finite";

// The masks of a batched encode (wr_encode_*_seg_batch_masked): per field the bit plane and what the split said; the blobs of
// the fields that have an undefined sample come from ONE seg_encode_batch launch on a stream of the masks' own, which runs
// under the fields' plane launches.
struct MaskBatchEncode {
    double below = -INFINITY;
    std::vector<unsigned long long> undefined;
    std::vector<double> pad;
    std::vector<size_t> mask_len;
    std::vector<float> split_ms, fill_ms;
    float coder_ms = 0;

    wr_ctx* c = nullptr;
    MaskStreams s;
    size_t n = 0, nsym = 0, blob_cap = 0;
    unsigned seg = 0;
    int nfields = 0;
    std::vector<uint8_t*> bits, blob;
    std::vector<int> job_of;  // field -> its job in the mask launch, -1: no undefined sample
    uint8_t *pinned = nullptr, *pinned_dev = nullptr;  // the mask launch's job table and results (BatchPinned)
    int njobs = 0;

    MaskBatchEncode() = default;
    MaskBatchEncode(const MaskBatchEncode&) = delete;
    MaskBatchEncode& operator=(const MaskBatchEncode&) = delete;
    ~MaskBatchEncode()
    {
        if (!pinned) return;
        if (s.st) (void)hipStreamSynchronize(s.st);
        (void)hipHostFree(pinned);
    }

    int begin(wr_ctx* ctx, BatchBufs* bufs, int count, size_t samples, unsigned seg_len)
    {
        c = ctx; nfields = count; n = samples; seg = seg_len; nsym = wrmask::mask_bytes(n);
        blob_cap = mask_batch_blob_cap(n, seg);
        undefined.assign(count, 0); pad.assign(count, 0.0); mask_len.assign(count, 0);
        split_ms.assign(count, 0.f); fill_ms.assign(count, 0.f);
        bits.assign(count, nullptr); blob.assign(count, nullptr); job_of.assign(count, -1);
        for (int f = 0; f < count; f++)
            if (!(bits[f] = bufs->take(mask_batch_bits_bytes(n)))) return WR_ERR_HIP;
        return s.create();
    }

    // what the single call refuses, with the field in front
    int check(int f) const
    {
        const std::string who = "field " + std::to_string(f) + ": ";
        if (undefined[f] == (unsigned long long)n) return fail(WR_ERR_ARG, who + kNoDefined);
        if (!(fabs(pad[f]) <= DBL_MAX)) return fail(WR_ERR_ARG, who + kMeanNotFinite);
        return WR_OK;
    }

    // (cu_mu held) a host field where upload_field left it, before anything widens it: the single-field launchers
    template <class T>
    int split_fill(int f, T* d_x)
    {
        HIPCHK(hipEventRecord(s.ev[0], c->stream));
        wrk::mask_split(d_x, n, below, bits[f], c->d_partial, c->h_result_dev, c->stream);
        HIPCHK(hipEventRecord(s.ev[1], c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask split launch failed");
        HIPCHK(hipEventSynchronize(s.ev[1]));
        split_ms[f] = s.ms(0);
        mask_split_result<T>(c, n, &undefined[f], &pad[f]);
        if (int rc = check(f)) return rc;
        if (!undefined[f]) return WR_OK;
        HIPCHK(hipEventRecord(s.ev[2], c->stream));
        wrk::mask_fill(d_x, n, bits[f], (T)pad[f], c->stream);
        HIPCHK(hipEventRecord(s.ev[3], c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask fill launch failed");
        HIPCHK(hipEventSynchronize(s.ev[3]));
        fill_ms[f] = s.ms(1);
        return WR_OK;
    }

    // (cu_mu held) device fields: all of them by one split launch pair and one fill launch, before the first transform
    int split_fill_all(BatchBufs* bufs, const std::vector<FieldRef>& flds)
    {
        MaskPinned pin(c);
        if (int rc = pin.alloc(std::max(mask_batch_split_pinned(nfields), (size_t)nfields * sizeof(wrk::MaskFillItem)))) return rc;
        double* const partial = reinterpret_cast<double*>(bufs->take(mask_batch_partial_bytes(nfields, n)));
        if (!partial) return WR_ERR_HIP;
        std::vector<double*> x(nfields);
        for (int f = 0; f < nfields; f++) x[f] = flds[f].dev;
        HIPCHK(hipEventRecord(s.ev[0], c->stream));
        if (int rc = mask_split_batch_run<double>(c, pin, partial, nfields, x.data(), bits.data(), n, below, undefined.data(), pad.data())) return rc;
        HIPCHK(hipEventRecord(s.ev[1], c->stream));
        for (int f = 0; f < nfields; f++) {
            if (int rc = check(f)) return rc;
            if (!undefined[f]) x[f] = nullptr;
        }
        int filled = 0;
        HIPCHK(hipEventRecord(s.ev[2], c->stream));
        if (int rc = mask_fill_batch_run<double>(c, pin, nfields, x.data(), bits.data(), n, pad.data(), &filled)) return rc;
        HIPCHK(hipEventRecord(s.ev[3], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int f = 0; f < nfields; f++) { split_ms[f] = s.ms(0); if (undefined[f]) fill_ms[f] = s.ms(1); }
        return WR_OK;
    }

    // (cu_mu held) every split has been read back: the masks of the fields that have an undefined sample in one launch on the
    // second stream.  Returns the launches made through *launches.
    int launch(BatchBufs* bufs, int* launches)
    {
        *launches = 0;
        std::vector<wrk::SegJob> jobs;
        for (int f = 0; f < nfields; f++) {
            if (!undefined[f]) continue;
            if (!(blob[f] = bufs->take(blob_cap))) return fail_at("field", f, WR_ERR_HIP);
            job_of[f] = (int)jobs.size();
            jobs.push_back(seg_encode_job(wrk::plane_ref(bits[f]), blob[f], blob_cap, 0));
        }
        njobs = (int)jobs.size();
        if (!njobs) return WR_OK;
        if ((unsigned long long)wrseg::seg_count(nsym, seg) * (unsigned)njobs >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the masks have 2^31 segments or more");
        uint8_t* const stage = bufs->take(wrk::seg_batch_stage_bytes(njobs, nsym, seg));
        if (!stage) return WR_ERR_HIP;
        const BatchPinned pin(njobs);
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&pinned), pin.bytes(1), hipHostMallocDefault));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&pinned_dev), pinned, 0));
        memset(pinned, 0, pin.bytes(1));
        HIPCHK(hipEventRecord(s.ev[4], s.st));
        wrk::seg_encode_batch(jobs.data(), jobs.size(), nsym, seg, pin.jobs(pinned, 0), stage, pin.results(pinned_dev, 0), s.st);
        HIPCHK(hipEventRecord(s.ev[5], s.st));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask coder launch failed");
        *launches = 1;
        return WR_OK;
    }

    // the blobs' exact lengths: waits for the mask launch
    int lengths()
    {
        if (!njobs) return WR_OK;
        if (hipStreamSynchronize(s.st) != hipSuccess) return fail(WR_ERR_HIP, "the masks' coder failed on the device");
        const unsigned long long* const res = BatchPinned(njobs).results(pinned, 0);
        for (int f = 0; f < nfields; f++) {
            if (job_of[f] < 0) continue;
            const unsigned long long len = res[2 * job_of[f]], bad = res[2 * job_of[f] + 1];
            if (bad || len > blob_cap) return fail(WR_ERR_HIP, "field " + std::to_string(f) + ": internal: mask plane: " + kOutgrew);
            mask_len[f] = wrmask::kHeaderBytes + (size_t)len;
        }
        coder_ms = s.ms(2);
        return WR_OK;
    }

    // field f's blob to data_enc + at
    int download(int f, unsigned char* data_enc, size_t at)
    {
        if (!undefined[f]) return WR_OK;
        wrmask::put_header(data_enc + at, n, undefined[f], pad[f]);
        return xfer_field(c, &c->x_field, data_enc + at + wrmask::kHeaderBytes, blob[f], mask_len[f] - wrmask::kHeaderBytes, kDown);
    }

    void result(int f, wr_mask_result* res) const
    {
        res->undefined = undefined[f]; res->pad = pad[f]; res->mask_len = mask_len[f];
        res->split_ms = split_ms[f]; res->fill_ms = fill_ms[f]; res->mask_coder_ms = undefined[f] ? coder_ms : 0;
    }
};

// msk != nullptr: a masked batch (wr_encode_*_seg_batch_masked): every field is split and filled in front of its transform,
// the masks of the fields that have an undefined sample are coded by one more launch, each blob lands behind its field's planes
int encode_seg_batch_impl(wr_ctx* c, int nfields, const std::vector<FieldRef>& flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                          const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* infos,
                          unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, MaskBatchEncode* msk = nullptr)
{
    // strands == 0: WRS1 / WRS2 (the entry points without that argument); otherwise WRS3, K lanes per segment
    if (int rc = seg_format_params(&seg, brick, strands)) return rc;
    if (!cutoffvecs || !infos || !data_encs || !caps) return fail(WR_ERR_ARG, "null array");
    if (mx < 1 || my < 1 || mz < 1) return fail(WR_ERR_ARG, "bad local cutoff description");
    if (int rc = ctx_bind(c)) return rc;
    bool any_host = false;
    for (int f = 0; f < nfields; f++) {
        if (flds[f].none()) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": null field pointer");
        if (!cutoffvecs[f]) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": bad local cutoff description");
        if (int rc = check_dims(nx, ny, nz, flds[f].dev)) return fail_at("field", f, rc);
        any_host = any_host || !flds[f].dev;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->keep_residual) return fail(WR_ERR_UNSUPPORTED, "a batch does not write residuals back: wr_ctx_set_keep_residual(ctx, 0) for batched encodes");
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    const size_t nseg = wrseg::seg_count(n, seg);
    if ((unsigned long long)nseg * (unsigned)nfields >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the planes of one index have 2^31 segments or more");
    if ((unsigned long long)nseg * strands * (unsigned)nfields >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many strands: the planes of one index have 2^31 strands or more");
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    c->pend_valid = false;
    PlaneHold planes(c);
    BatchBufs bufs(c);  // (goes first when the call unwinds, and waits for the stream)
    const size_t blob_cap = seg_blob_cap(n, seg, brick, strands);
    const BatchPinned pin(nfields);
    wrblk::Order od{};
    if (brick) od = wrblk::order_of(nx, ny, nz, wtflag ? kWavLvl : 0, brick);

    SlotNeed need;
    transform_need(nx, ny, nz, wtflag ? kWavLvl : 0, &need);
    if (any_host) need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    std::vector<wrk::PlaneRef> refs((size_t)nfields * WR_NLAYMAX);
    std::vector<uint8_t*> blob((size_t)nfields * WR_NLAYMAX, nullptr), perm(nfields, nullptr);
    std::vector<int> job_of((size_t)nfields * WR_NLAYMAX, -1);  // (field, plane) -> its job in the launch sequence of that plane index
    int maxlay = 0;
    if (msk) {
        if (int rc = msk->begin(c, &bufs, nfields, n, seg)) return rc;
        bufs.also = msk->s.st;
    }
    {
        StageLock cu(pool->cu_mu);
        clock_warmup(c, n);
        if (msk && !any_host) if (int rc = msk->split_fill_all(&bufs, flds)) return rc;
        // ---- every field in turn through the slot: upload, transform, quantizer; its planes stay in the batch's buffers
        for (int f = 0; f < nfields; f++) {
            const FieldRef& fld = flds[f];
            Cutoff cut; cut.mx = mx; cut.my = my; cut.mz = mz; cut.vec = cutoffvecs[f];
            FieldUpload up;
            if (int rc = upload_field(c, slot.get(), fld, nx, ny, nz, wtflag, &up)) return fail_at("field", f, rc);
            local.h2d_ms += up.ms;
            double* const d_fld = up.d_fld;
            if (msk && any_host) {  // the field where it landed: an fp32 field before anything widens it
                float* const x32 = up.d_f32 ? const_cast<float*>(up.d_f32) : up.widen_from;
                if (int rc = fld.host_f32 ? msk->split_fill(f, x32) : msk->split_fill(f, d_fld)) return rc;
            }
            if (up.widen_from) wrk::widen_f32(up.widen_from, d_fld, n, c->stream);  // (the stage is held: at once)
            auto plane_buf = [&](unsigned l) -> const wrk::PlaneRef* {
                uint8_t* const p = bufs.take(batch_plane_bytes(n));
                if (!p) return nullptr;
                refs[(size_t)f * WR_NLAYMAX + l] = wrk::plane_ref(p);
                return &refs[(size_t)f * WR_NLAYMAX + l];
            };
            double* resid = d_fld;
            wr_timings ft; memset(&ft, 0, sizeof ft);
            int rc = encode_planes_core(c, slot.get(), d_fld, nx, ny, nz, wtflag, cut, plane_buf, [](unsigned) { return (uint16_t*)nullptr; }, &infos[f], &ft,
                                        [](unsigned, bool) { return WR_OK; }, [](unsigned, bool) { return WR_OK; }, &resid, up.d_f32);
            // the slot is the next field's from here on
            if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the encoder's kernel stage failed on the device" + launch_describe(c));
            if (rc) return fail_at("field", f, rc);
            local.quant_ms += ft.quant_ms; local.transform_ms += ft.transform_ms; local.minmax_ms += ft.minmax_ms;
            if ((int)infos[f].nlay > maxlay) maxlay = infos[f].nlay;
        }
        if (msk) {  // ---- the masks' one launch, on their stream: it runs under the plane launches below
            int launches = 0;
            if (int rc = msk->launch(&bufs, &launches)) return rc;
            g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += (unsigned long)launches;
        }
        // ---- one launch sequence per plane index over the fields that have such a plane
        if (maxlay) {
            uint8_t* const stage = bufs.take(batch_once_bytes(nfields, n, maxlay, seg, false, strands));
            if (!stage) return WR_ERR_HIP;
            for (int f = 0; f < nfields; f++) {
                for (int l = 0; l < (int)infos[f].nlay; l++)
                    if (!(blob[(size_t)f * WR_NLAYMAX + l] = bufs.take(blob_cap))) return fail_at("field", f, WR_ERR_HIP);
                if (brick && infos[f].nlay && !(perm[f] = bufs.take(batch_perm_bytes(n, brick)))) return fail_at("field", f, WR_ERR_HIP);
            }
            if (int rc = bufs.pin(pin.bytes(maxlay))) return rc;
            std::vector<wrk::SegJob> jobs;
            for (int l = 0; l < maxlay; l++) {
                if (int rc = bufs.ev.create(l)) return rc;
                HIPCHK(hipEventRecord(bufs.ev[2 * l], c->stream));
                jobs.clear();
                for (int f = 0; f < nfields; f++) {
                    if ((int)infos[f].nlay <= l) continue;
                    const size_t at = (size_t)f * WR_NLAYMAX + l;
                    // a blocked stream: the plane in stream order first, a pass of milliseconds per field, not batched
                    if (brick && !wrk::plane_reorder(refs[at], perm[f], od, false, nullptr, 0, c->stream)) return fail(WR_ERR_ARG, "too many bricks");
                    job_of[at] = (int)jobs.size();
                    jobs.push_back(seg_encode_job(brick ? wrk::plane_ref(perm[f]) : refs[at], blob[at], blob_cap, brick));
                }
                launch_note(c, strands ? "strand_encode_batch" : "seg_encode_batch", l, stage, n, pin.jobs(bufs.pinned, l), jobs[0].sym);
                if (strands) wrk::strand_encode_batch(jobs.data(), jobs.size(), n, seg, strands, pin.jobs(bufs.pinned, l), stage, pin.results(bufs.pinned_dev, l), c->stream);
                else wrk::seg_encode_batch(jobs.data(), jobs.size(), n, seg, pin.jobs(bufs.pinned, l), stage, pin.results(bufs.pinned_dev, l), c->stream);
                HIPCHK(hipEventRecord(bufs.ev[2 * l + 1], c->stream));
                if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched segment coder launch failed" + launch_describe(c));
                g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += 1;
            }
            if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the batched segment coder failed on the device" + launch_describe(c));
        }
        if (msk) if (int rc = msk->lengths()) return rc;
        pool->last_stage_end.store(now());
    }
    // ---- stage "down": every blob, one copy each, to its place in its field's data_enc
    for (int f = 0; f < nfields; f++) {
        wr_enc_info* const info = &infos[f];
        const std::string who = "field " + std::to_string(f) + ": ";
        size_t total = 0;
        auto res_of = [&](int l) { return pin.results(bufs.pinned, l) + 2 * job_of[(size_t)f * WR_NLAYMAX + l]; };
        if (int rc = seg_coded_lengths(info->nlay, blob_cap, res_of, info->len_enc_vec, &total, who)) return rc;
        if (total > caps[f] || (total && !data_encs[f])) return fail(WR_ERR_OVERFLOW, who + wrtc::kTooLarge);
        if (msk && msk->undefined[f] && (!data_encs[f] || msk->mask_len[f] > caps[f] - total))
            return fail(WR_ERR_OVERFLOW, who + "the coded buffer does not hold the field's planes and the mask blob of " + std::to_string(msk->mask_len[f]) + " bytes");
        size_t at = 0;
        for (int l = 0; l < (int)info->nlay; l++) {
            if (int rc = xfer_field(c, &c->x_field, data_encs[f] + at, blob[(size_t)f * WR_NLAYMAX + l], info->len_enc_vec[l], kDown)) return fail_at("field", f, rc);
            local.d2h_ms += (float)c->x_field.ms;
            at += info->len_enc_vec[l];
        }
        if (msk) if (int rc = msk->download(f, data_encs[f], total)) return fail_at("field", f, rc);
        info->ntot_enc = total;
    }
    fold_coder_seconds(bufs, maxlay, &local);  // one entry per plane index
    local.total = now() - t0;
    local.wait = t_phase - t0;
    local.gpu = now() - t_phase;
    if (tm) *tm = local;
    return WR_OK;
}

struct BatchField {  // a field of a decode batch: its stream as the host has validated it (nlay == 0: a constant field, no job), and its buffers
    SegStream s;
    uint8_t *plane[WR_NLAYMAX] = {nullptr}, *blob[WR_NLAYMAX] = {nullptr}, *work[WR_NLAYMAX] = {nullptr}, *perm = nullptr;
    uint8_t* perms[WR_NLAYMAX] = {nullptr};  // a blocked field of a mixed decode: one stream-order plane per job (all jobs go in one launch)
    int job0 = 0;                            // its first job's place in the failure counts
};

// The coder launches of a mixed decode: the jobs of one kind in launches of at most WR_SEG_BATCH_MAX jobs, their tables behind
// one another at host_table / d_table.  First: whether every such launch stays below 2^31 lanes.
bool batch_chunk_lanes_ok(const std::vector<wrk::SegJob>& jobs)
{
    for (size_t a = 0; a < jobs.size(); a += wrsb::kBatchMax) {
        unsigned long long lanes = 0;
        for (size_t j = a; j < std::min<size_t>(jobs.size(), a + wrsb::kBatchMax); j++) lanes += wrsb::job_lanes(jobs[j].nseg, jobs[j].strands);
        if (lanes >= wrsb::kLaneLimit) return false;
    }
    return true;
}

// (cu_mu held) returns the launches made; *at: where the next table goes, moved on
int batch_chunk_launch(const std::vector<wrk::SegJob>& jobs, bool stranded, uint8_t* host_table, uint8_t* d_table, size_t* at, hipStream_t st)
{
    int launches = 0;
    for (size_t a = 0; a < jobs.size(); a += wrsb::kBatchMax) {
        const size_t count = std::min<size_t>(wrsb::kBatchMax, jobs.size() - a);
        size_t lanes = 0;
        for (size_t j = a; j < a + count; j++) lanes += jobs[j].nseg;
        if (!lanes) continue;  // (neither launcher launches for jobs without segments)
        if (stranded) wrk::strand_decode_batch(jobs.data() + a, count, host_table + *at, d_table + *at, st);
        else wrk::seg_decode_batch(jobs.data() + a, count, host_table + *at, d_table + *at, st);
        launches++;
        *at += wrk::seg_batch_table_bytes(count);
    }
    return launches;
}

// The masks of a batched decode (wr_decode_*_seg_batch_masked): a MaskJob per record that has a blob.  Each is one more WRS1 job
// of the mixed driver's plain launch; one k_mask_check_batch launch behind the coder stage judges them all, before any
// dequantizer runs; the existing fill then puts `fill` into each field behind its inverse transform.
struct MaskBatchDecode {
    double fill = NAN;
    std::vector<MaskJob> job;  // per field; blob == nullptr: an unmasked record
    std::vector<int> index;    // field -> its place among the masks, -1: none
    int nmask = 0;
    float coder_ms = 0;

    void result(int f, wr_mask_result* res) const
    {
        memset(res, 0, sizeof *res);
        if (index[f] < 0) return;
        res->undefined = job[f].info.undefined; res->pad = job[f].info.pad; res->mask_len = job[f].len;
        res->mask_coder_ms = coder_ms;
    }
};

// mixed == false: wr_decode_*_seg_batch -- WRS1 and WRS2 fields, a WRS3 field is refused, one coder launch per plane index.
// mixed == true: wr_decode_*_seg_batch_mixed -- WRS3 fields beside them, every (field, plane) of the call a job of its own, the
// plain jobs through k_seg_decode_batch and the stranded ones through k_strand_decode_batch: two launches while neither kind has
// more than WR_SEG_BATCH_MAX jobs.  Everything around the coder stage is the same code.
int decode_seg_batch_impl(wr_ctx* c, int nfields, const std::vector<FieldRef>& flds, int nx, int ny, int nz, const wr_enc_info* infos,
                          const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm, bool mixed = false, MaskBatchDecode* msk = nullptr)
{
    // msk != nullptr (mixed only): data_lens are the field parts' lengths, the blobs are the jobs'
    if (!infos || !data_encs) return fail(WR_ERR_ARG, "null array");
    if (int rc = ctx_bind(c)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    bool any_host = false;
    for (int f = 0; f < nfields; f++) {
        if (flds[f].none()) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": null field pointer");
        if (int rc = check_dims(nx, ny, nz, flds[f].dev)) return fail_at("field", f, rc);
        any_host = any_host || !flds[f].dev;
    }
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    // ---- every field's lengths, headers and indices, on the host, before anything is copied or launched for any field
    std::vector<BatchField> bf(nfields);
    int maxlay = 0, wlev_any = 0;
    size_t njobs = 0, nplain = 0, nstranded = 0;
    unsigned long long lanes[WR_NLAYMAX] = {0};
    for (int f = 0; f < nfields; f++) {
        const wr_enc_info* const info = &infos[f];
        SegStream& s = bf[f].s;
        if (info->ntot_enc == 0) continue;  // a constant field: filled with midval below
        const std::string who = "field " + std::to_string(f) + ": ";
        if (int rc = seg_stream_of(nx, ny, nz, info, data_encs[f], data_lens ? data_lens[f] : 0, &s, who)) return rc;
        if (s.strands && !mixed) return fail(WR_ERR_UNSUPPORTED, who + "a WRS3 stream: stranded segments are not decoded in a batch (wr_decode_host_seg reads them)");
        for (int l = 0; l < s.nlay; l++) lanes[l] += s.nseg[l];
        bf[f].job0 = (int)njobs;
        njobs += (size_t)s.nlay;
        (s.strands ? nstranded : nplain) += (size_t)s.nlay;
        if (s.nlay > maxlay) maxlay = s.nlay;
        if (info->wlev) wlev_any = kWavLvl;
    }
    for (int l = 0; l < maxlay && !mixed; l++)
        if (lanes[l] >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the planes of index " + std::to_string(l) + " have 2^31 segments or more");
    // ---- every mask blob, likewise.  A mask is one more plain job; its failure count lies behind the planes'
    const size_t mask_job0 = njobs;
    if (msk) {
        std::vector<const unsigned char*> blobs(nfields);
        std::vector<size_t> lens(nfields);
        std::vector<wrmask::BlobInfo> bi(nfields);
        for (int f = 0; f < nfields; f++) { blobs[f] = msk->job[f].blob; lens[f] = msk->job[f].len; }
        std::string why;
        const int failed = wrmask::check_blobs(blobs.data(), lens.data(), nfields, n, bi.data(), &why);
        if (failed < nfields) return fail(WR_ERR_STREAM, "field " + std::to_string(failed) + ": " + why);
        msk->index.assign(nfields, -1);
        for (int f = 0; f < nfields; f++) {
            if (!blobs[f]) continue;
            MaskJob& j = msk->job[f];
            j.info = bi[f]; j.n = n; j.nsym = wrmask::mask_bytes(n);
            msk->index[f] = msk->nmask++;
        }
        njobs += (size_t)msk->nmask;
        nplain += (size_t)msk->nmask;
    }
    const int nmask = msk ? msk->nmask : 0;
    const bool coded = maxlay || nmask;
    c->pend_valid = false;
    PlaneHold planes(c);
    BatchBufs bufs(c);
    MaskPinned mask_pin(c);  // the table of the masks' planes for their check
    unsigned long long* d_counters = nullptr;
    uint8_t* d_once = nullptr;
    const size_t table = wrk::seg_batch_table_bytes(nfields);
    // the jobs' failure counts lie behind the tables, in the order of the fields and their planes
    const size_t tables_bytes = mixed ? batch_mixed_tables_bytes(nplain, nstranded) : (size_t)maxlay * table;
    if (coded) {
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);  // one decode at a time gathers its planes (decode_impl)
        for (int f = 0; f < nfields && nmask; f++) {
            if (msk->index[f] < 0) continue;
            MaskJob& j = msk->job[f];
            j.bits = bufs.take(j.bits_bytes());
            j.work = bufs.take(j.work_bytes());
            j.d_blob = bufs.take((j.blob_bytes() + 15) & ~(size_t)15);
            if (!j.bits || !j.work || !j.d_blob) return fail_at("field", f, WR_ERR_HIP);
        }
        if (nmask) {
            if (!(d_counters = reinterpret_cast<unsigned long long*>(bufs.take(mask_batch_counters_bytes(nmask))))) return WR_ERR_HIP;
            if (int rc = mask_pin.alloc((size_t)nmask * sizeof(uint8_t*))) return rc;
        }
        for (int f = 0; f < nfields; f++) {
            BatchField& b = bf[f];
            for (int l = 0; l < b.s.nlay; l++) {
                b.plane[l] = bufs.take(batch_plane_bytes(n));
                b.blob[l] = bufs.take(infos[f].len_enc_vec[l]);
                b.work[l] = bufs.take(batch_work_bytes(b.s.nseg[l]));
                if (!b.plane[l] || !b.blob[l] || !b.work[l]) return fail_at("field", f, WR_ERR_HIP);
                if (mixed && b.s.brick && !(b.perms[l] = bufs.take(batch_perm_bytes(n, b.s.brick)))) return fail_at("field", f, WR_ERR_HIP);
            }
            if (!mixed && b.s.brick && !(b.perm = bufs.take(batch_perm_bytes(n, b.s.brick)))) return fail_at("field", f, WR_ERR_HIP);
        }
        if (!(d_once = bufs.take(mixed ? batch_mixed_once_bytes(nplain, nstranded) : batch_once_bytes(nfields, n, maxlay, 0, true)))) return WR_ERR_HIP;
        if (int rc = bufs.pin(mixed ? tables_bytes : BatchPinned(nfields).bytes(maxlay))) return rc;
    }
    // ---- stage "up": one copy per blob, and its segments' offsets
    for (int f = 0; f < nfields; f++)
        for (int l = 0; l < bf[f].s.nlay; l++) {
            const SegStream& s = bf[f].s;
            if (int rc = xfer_field(c, &c->x_field, bf[f].blob[l], data_encs[f] + s.off[l], infos[f].len_enc_vec[l], kUp)) return fail_at("field", f, rc);
            local.h2d_ms += (float)c->x_field.ms;
            if (int rc = seg_upload_offsets(data_encs[f] + s.off[l], s.head(), s.nseg[l], bf[f].work[l])) return fail_at("field", f, rc);
        }
    for (int f = 0; f < nfields && nmask; f++) {
        if (msk->index[f] < 0) continue;
        size_t bytes_up = 0;
        if (int rc = msk->job[f].upload(c, &local.h2d_ms, &bytes_up)) return fail_at("field", f, rc);
    }
    const double t_coded = now();
    SlotNeed need;
    transform_need(nx, ny, nz, wlev_any ? -kWavLvl : 0, &need);
    if (any_host) need.field_elems = n;
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    {
        StageLock cu(pool->cu_mu);
        clock_warmup(c, n);
        if (coded) {
            // job (f, l) counts into d_bad[job0 of f + l], the mask of field f into d_bad[mask_job0 + its place among the masks]
            unsigned int* const d_bad = reinterpret_cast<unsigned int*>(d_once + tables_bytes);
            const size_t per_l = BatchPinned(nfields).per_l;
            HIPCHK(hipMemsetAsync(d_bad, 0, 4 * njobs, c->stream));
            std::vector<wrk::SegJob> jobs;
            if (mixed) {
                // ---- every (field, plane) of the call: the plain jobs in one launch, the stranded ones in another
                std::vector<wrk::SegJob> stranded;
                for (int f = 0; f < nfields; f++) {
                    const BatchField& b = bf[f];
                    for (int l = 0; l < b.s.nlay; l++) {
                        wrk::SegJob job = seg_job(wrk::plane_ref(b.s.brick ? b.perms[l] : b.plane[l]), b.blob[l], infos[f].len_enc_vec[l], b.work[l], n, b.s.seg[l], b.s.nseg[l], b.s.brick);
                        job.strands = b.s.strands;
                        job.bad = d_bad + b.job0 + l;  // (the batch counts in one array, read back once)
                        (b.s.strands ? stranded : jobs).push_back(job);
                    }
                }
                std::vector<const uint8_t*> mask_planes;
                for (int f = 0; f < nfields && nmask; f++) {
                    if (msk->index[f] < 0) continue;
                    wrk::SegJob job = msk->job[f].seg_job();
                    job.bad = d_bad + mask_job0 + (size_t)msk->index[f];
                    jobs.push_back(job);
                    mask_planes.push_back(msk->job[f].bits);
                }
                if (!batch_chunk_lanes_ok(jobs) || !batch_chunk_lanes_ok(stranded)) return fail(WR_ERR_ARG, "too many segments: a launch of the call has 2^31 lanes or more");
                if (int rc = bufs.ev.create(0)) return rc;
                launch_note(c, "seg_decode_batch_mixed", 0, d_once, n, bufs.pinned, wrk::plane_ref(d_once));
                HIPCHK(hipEventRecord(bufs.ev[0], c->stream));
                size_t at = 0;
                int launches = batch_chunk_launch(jobs, false, bufs.pinned, d_once, &at, c->stream);
                launches += batch_chunk_launch(stranded, true, bufs.pinned, d_once, &at, c->stream);
                HIPCHK(hipEventRecord(bufs.ev[1], c->stream));
                if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched segment decoder launch failed" + launch_describe(c));
                g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += (unsigned long)launches;
                if (nmask) {  // every mask judged by one launch: the counts come back with the failure counts
                    memcpy(mask_pin.host, mask_planes.data(), mask_planes.size() * sizeof(uint8_t*));
                    wrk::mask_check_batch(reinterpret_cast<const uint8_t* const*>(mask_pin.dev), nmask, n, d_counters, c->stream);
                    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched mask check launch failed");
                }
            }
            for (int l = 0; l < maxlay && !mixed; l++) {
                if (int rc = bufs.ev.create(l)) return rc;
                jobs.clear();
                for (int f = 0; f < nfields; f++) {
                    const BatchField& b = bf[f];
                    if (b.s.nlay <= l) continue;
                    jobs.push_back(seg_job(wrk::plane_ref(b.s.brick ? b.perm : b.plane[l]), b.blob[l], infos[f].len_enc_vec[l], b.work[l], n, b.s.seg[l], b.s.nseg[l], b.s.brick));
                    jobs.back().bad = d_bad + b.job0 + l;  // (the batch counts in one array, read back once)
                }
                launch_note(c, "seg_decode_batch", l, d_once + l * table, n, bufs.pinned + l * per_l, jobs[0].sym);
                HIPCHK(hipEventRecord(bufs.ev[2 * l], c->stream));
                wrk::seg_decode_batch(jobs.data(), jobs.size(), bufs.pinned + l * per_l, d_once + l * table, c->stream);
                g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += 1;
                for (int f = 0; f < nfields; f++)  // WRS2 fields: back to the natural order, per field as in the single-field coder stage
                    if (bf[f].s.nlay > l && bf[f].s.brick &&
                        !wrk::plane_reorder(wrk::plane_ref(bf[f].plane[l]), bf[f].perm, bf[f].s.od, true, nullptr, 0, c->stream))
                        return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": too many bricks");
                HIPCHK(hipEventRecord(bufs.ev[2 * l + 1], c->stream));
                if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched segment decoder launch failed" + launch_describe(c));
            }
            // the dequantizers only run if every segment of every field decoded: the counts come back once
            std::vector<unsigned int> bad(njobs);
            HIPCHK(hipMemcpyAsync(bad.data(), d_bad, 4 * bad.size(), hipMemcpyDeviceToHost, c->stream));
            std::vector<unsigned long long> counters(2 * (size_t)nmask);
            if (nmask) HIPCHK(hipMemcpyAsync(counters.data(), d_counters, 8 * counters.size(), hipMemcpyDeviceToHost, c->stream));
            if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the batched segment decoder failed on the device" + launch_describe(c));
            for (int f = 0; f < nfields; f++) {
                for (int l = 0; l < bf[f].s.nlay; l++)
                    if (const unsigned int k = bad[(size_t)bf[f].job0 + l])
                        return fail(WR_ERR_STREAM, "field " + std::to_string(f) + ": plane " + std::to_string(l) + ": " + bad_segments_text(k));
                if (!nmask || msk->index[f] < 0) continue;
                // the mask, in the single call's words (MaskDecode::check): nothing of the caller's has been written yet
                const std::string who = "field " + std::to_string(f) + ": mask blob: ";
                const size_t m = (size_t)msk->index[f];
                if (const unsigned int k = bad[mask_job0 + m]) return fail(WR_ERR_STREAM, who + bad_segments_text(k));
                if (counters[2 * m + 1]) return fail(WR_ERR_STREAM, who + "a bit beyond the field's last sample is set");
                if (counters[2 * m] != msk->job[f].info.undefined) return fail(WR_ERR_STREAM, who + "the mask's set bits are not the count in its header");
            }
            fold_coder_seconds(bufs, mixed ? 1 : maxlay, &local);  // one entry per plane index; mixed: one for the call's launches
            if (nmask) msk->coder_ms = (float)(1e3 * local.plane_coder_s[0]);
        }
        // ---- every field in turn through the slot: dequantizer, inverse transform, download
        for (int f = 0; f < nfields; f++) {
            const FieldRef& fld = flds[f];
            const wr_enc_info* const info = &infos[f];
            const BatchField& b = bf[f];
            const uint8_t* const mask_bits = (nmask && msk->index[f] >= 0) ? msk->job[f].bits : nullptr;
            if (!b.s.nlay) {
                if (int rc = fill_constant(c, fld, n, info->midval)) return rc;
                if (mask_bits && fld.dev) {
                    wrk::mask_fill(fld.dev, n, mask_bits, msk->fill, c->stream);
                    if (int rc = kernel_stage_end(c, WR_OK)) return fail_at("field", f, rc);
                } else if (mask_bits) {  // a host field takes the bits on the host, as it took midval there
                    std::vector<unsigned char> h(msk->job[f].nsym);
                    HIPCHK(hipMemcpy(h.data(), mask_bits, h.size(), hipMemcpyDeviceToHost));
                    mask_restore_host(fld, mask_region(nx, ny, nz, 0, nullptr), h.data(), msk->fill);
                }
                continue;
            }
            for (int l = 0; l < b.s.nlay && mixed; l++)  // a blocked field of a mixed decode: its planes back to the natural order
                if (b.s.brick && !wrk::plane_reorder(wrk::plane_ref(b.plane[l]), b.perms[l], b.s.od, true, nullptr, 0, c->stream))
                    return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": too many bricks");
            wrk::DequantParams p;
            if (int rc = dequant_params(info, b.s.nlay, n, [&](int l) { return wrk::plane_ref(b.plane[l]); }, &p)) return fail_at("field", f, rc);
            double* const d_fld = fld.dev ? fld.dev : slot->field;
            float* d_f32 = nullptr;
            launch_note(c, "dequant", b.s.nlay - 1, d_fld, n, nullptr, p.q[b.s.nlay - 1]);
            int rc = inverse_from_planes(c, slot.get(), d_fld, nx, ny, nz, (int)info->wlev, p, fld.host_f32 ? &d_f32 : nullptr);
            if (rc == WR_OK && mask_bits) {  // `fill` where the finisher left the field: the slot (a host field) or the caller's buffer
                if (fld.host_f32) wrk::mask_fill(d_f32, n, mask_bits, (float)msk->fill, c->stream);
                else wrk::mask_fill(d_fld, n, mask_bits, msk->fill, c->stream);
            }
            if (rc == WR_OK && hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "kernel launch failed");
            if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the decoder's kernel stage failed on the device" + launch_describe(c));
            if (rc) return fail_at("field", f, rc);
            if (fld.host) {
                if ((rc = xfer_field(c, &c->x_field, fld.host, d_fld, n * sizeof(double), kDown)) != WR_OK) return fail_at("field", f, rc);
                local.d2h_ms += (float)c->x_field.ms;
            } else if (fld.host_f32) {
                if ((rc = xfer_field(c, &c->x_field, fld.host_f32, d_f32, n * sizeof(float), kDown)) != WR_OK) return fail_at("field", f, rc);
                local.d2h_ms += (float)c->x_field.ms;
            }
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b)); local.quant_ms += ms;
            HIPCHK(hipEventElapsedTime(&ms, c->ev_b, c->ev_c)); local.transform_ms += ms;
        }
        pool->last_stage_end.store(now());
    }
    local.total = now() - t0;
    local.gpu = now() - t_phase;
    local.wait = t_phase - t_coded;
    local.transfer = t_coded - t0;
    if (tm) *tm = local;
    return WR_OK;
}

// the stage calls of the batched mask kernels (wr_dev_mask_split_batch, wr_dev_mask_fill_batch and their _f32 forms)
int mask_batch_args(wr_ctx* c, int count, const char* what, const void* const* a, const void* const* b, size_t n, bool null_a_ok = false)
{
    if (count < 1 || count > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, std::string(what) + " must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (int rc = ctx_bind(c)) return rc;
    if (!a || !b) return fail(WR_ERR_ARG, "null array");
    if (!n) return fail(WR_ERR_ARG, "empty array");
    for (int f = 0; f < count; f++)
        if ((!a[f] && !null_a_ok) || (a[f] && !b[f])) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": null pointer");
    return WR_OK;
}

template <class T>
int dev_mask_split_batch(wr_ctx* c, int nfields, const T* const* d_flds, size_t n, double below, unsigned char* const* d_bits,
                                unsigned long long* undefined, double* pad)
{
    if (int rc = mask_batch_args(c, nfields, "nfields", reinterpret_cast<const void* const*>(d_flds), reinterpret_cast<const void* const*>(d_bits), n)) return rc;
    if (!undefined || !pad) return fail(WR_ERR_ARG, "null array");
    if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");
    std::lock_guard<std::mutex> lk(c->mu);
    BatchBufs bufs(c);
    MaskPinned pin(c);
    if (int rc = pin.alloc(mask_batch_split_pinned(nfields))) return rc;
    double* const partial = reinterpret_cast<double*>(bufs.take(mask_batch_partial_bytes(nfields, n)));
    if (!partial) return WR_ERR_HIP;
    StageLock cu(c->pool->cu_mu);
    return mask_split_batch_run<T>(c, pin, partial, nfields, d_flds, d_bits, n, below, undefined, pad);
}

template <class T>
int dev_mask_fill_batch(wr_ctx* c, int nfields, T* const* d_flds, size_t n, const unsigned char* const* d_bits, const double* values)
{
    if (int rc = mask_batch_args(c, nfields, "nfields", reinterpret_cast<const void* const*>(d_flds), reinterpret_cast<const void* const*>(d_bits), n, true)) return rc;
    if (!values) return fail(WR_ERR_ARG, "null array");
    std::lock_guard<std::mutex> lk(c->mu);
    MaskPinned pin(c);
    if (int rc = pin.alloc((size_t)nfields * sizeof(wrk::MaskFillItem))) return rc;
    StageLock cu(c->pool->cu_mu);
    int filled = 0;
    if (int rc = mask_fill_batch_run<T>(c, pin, nfields, d_flds, d_bits, n, values, &filled)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return WR_OK;
}

template <class T>
int batch_fields(int nfields, T* const* ptrs, int kind, std::vector<FieldRef>* out)
{
    if (nfields < 1 || nfields > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, "nfields must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (!ptrs) return fail(WR_ERR_ARG, "null array");
    out->resize(nfields);
    for (int f = 0; f < nfields; f++) {
        FieldRef& r = (*out)[f];
        if (kind == 0) r.host = (double*)ptrs[f];
        else if (kind == 1) r.host_f32 = (float*)ptrs[f];
        else r.dev = (double*)ptrs[f];
    }
    return WR_OK;
}

}  // namespace

extern "C" {

size_t wr_seg_batch_device_bytes(int nfields, size_t n, int nlay, unsigned seg, unsigned brick, int decode)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (nfields < 1 || nfields > WR_SEG_BATCH_MAX || !n || nlay < 0 || nlay > WR_NLAYMAX || !wrseg::seg_ok(seg) || (brick && !wrblk::brick_ok(brick))) return 0;
    const size_t N = (size_t)nfields;
    size_t per_plane = batch_plane_bytes(n) + up256(seg_blob_cap(n, seg, brick, 0));
    if (decode) per_plane += up256(batch_work_bytes(wrseg::seg_count(n, seg)));
    return N * (size_t)nlay * per_plane + N * batch_perm_bytes(n, brick) + up256(batch_once_bytes(N, n, nlay, seg, decode != 0));
}

size_t wr_seg_batch_device_bytes_strands(int nfields, size_t n, int nlay, unsigned seg, unsigned brick, unsigned strands, int decode)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!strands) strands = WR_STRANDS_DEFAULT;
    if (nfields < 1 || nfields > WR_SEG_BATCH_MAX || !n || nlay < 0 || nlay > WR_NLAYMAX || !wrseg::seg_ok(seg) || (brick && !wrblk::brick_ok(brick))) return 0;
    if (!wrseg::strands_ok(strands, seg)) return 0;
    const size_t N = (size_t)nfields, jobs = N * (size_t)nlay;
    size_t per_plane = batch_plane_bytes(n) + up256(seg_blob_cap(n, seg, brick, strands));
    if (!decode) return jobs * per_plane + N * batch_perm_bytes(n, brick) + up256(batch_once_bytes(N, n, nlay, seg, false, strands));
    // the mixed decode: a stream-order plane per job of a blocked field, a table per launch of at most WR_SEG_BATCH_MAX jobs
    per_plane += up256(batch_work_bytes(wrseg::seg_count(n, seg))) + batch_perm_bytes(n, brick);
    return jobs * per_plane + up256(batch_mixed_once_bytes(0, jobs));
}

int wr_seg_batch_strand_lane(const uint32_t* first, uint32_t njobs, unsigned strands, unsigned long long g, uint32_t* job, uint32_t* segment, uint32_t* strand)
{
    if (!first || !job || !segment || !strand) return fail(WR_ERR_ARG, "null pointer");
    if (njobs < 1 || njobs > wrsb::kBatchMax) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(wrsb::kBatchMax));
    if (!strands || !wrsb::strands_layout_ok(strands)) return fail(WR_ERR_ARG, "strands must be one of 1, 2, 4, 8, 16, 32");
    if (!wrsb::prefix_ok(first, njobs)) return fail(WR_ERR_ARG, "not an exclusive prefix: it must start at 0 and never decrease");
    return wrsb::strand_lane(first, njobs, strands, g, job, segment, strand) ? 1 : 0;  // (0: a lane past the end, which is no error)
}

int wr_seg_batch_locate(const uint32_t* first, uint32_t njobs, uint32_t g, uint32_t* job, uint32_t* k)
{
    if (!first || !job || !k) return fail(WR_ERR_ARG, "null pointer");
    if (njobs < 1 || njobs > wrsb::kBatchMax) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(wrsb::kBatchMax));
    if (!wrsb::prefix_ok(first, njobs)) return fail(WR_ERR_ARG, "not an exclusive prefix: it must start at 0 and never decrease");
    if (g >= first[njobs]) return fail(WR_ERR_ARG, "lane past the end of the launch");
    wrsb::locate(first, njobs, g, job, k);
    return WR_OK;
}

// `njobs` planes, as they stand, into the callers' blob buffers: strands == 0 WRS1 blobs, otherwise WRS3 in the natural order
static int dev_seg_encode_batch(wr_ctx* c, int njobs, const unsigned char* const* d_sym, size_t n, unsigned seg, unsigned strands, unsigned char* const* d_blob,
                                const size_t* cap, size_t* blob_len)
{
    if (int rc = seg_format_params(&seg, 0, strands)) return rc;
    if (njobs < 1 || njobs > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (int rc = ctx_bind(c)) return rc;
    if (!d_sym || !d_blob || !cap || !blob_len) return fail(WR_ERR_ARG, "null array");
    const size_t nseg = wrseg::seg_count(n, seg);
    if ((unsigned long long)nseg * (unsigned)njobs >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the batch has 2^31 segments or more");
    if ((unsigned long long)nseg * strands * (unsigned)njobs >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many strands: the batch has 2^31 strands or more");
    for (int j = 0; j < njobs; j++) {
        if (!d_blob[j] || (n && !d_sym[j])) return fail(WR_ERR_ARG, "job " + std::to_string(j) + ": null pointer");
        if (((uintptr_t)d_sym[j] | (uintptr_t)d_blob[j]) & 15) return fail(WR_ERR_ARG, "job " + std::to_string(j) + ": plane and blob buffers must be 16-byte aligned");
        if (cap[j] < wrseg::header_bytes(0, strands) + 4 * nseg) return fail(WR_ERR_OVERFLOW, "job " + std::to_string(j) + ": the blob buffer does not hold the plane's index");
    }
    std::lock_guard<std::mutex> lk(c->mu);
    BatchBufs bufs(c);
    uint8_t* const stage = bufs.take(batch_once_bytes(njobs, n, 1, seg, false, strands));
    if (!stage) return WR_ERR_HIP;
    const BatchPinned pin(njobs);
    if (int rc = bufs.pin(pin.bytes(1))) return rc;
    std::vector<wrk::SegJob> jobs;
    for (int j = 0; j < njobs; j++) jobs.push_back(seg_encode_job(wrk::plane_ref(d_sym[j]), d_blob[j], cap[j], 0));
    StageLock cu(c->pool->cu_mu);
    if (strands) wrk::strand_encode_batch(jobs.data(), jobs.size(), n, seg, strands, pin.jobs(bufs.pinned, 0), stage, pin.results(bufs.pinned_dev, 0), c->stream);
    else wrk::seg_encode_batch(jobs.data(), jobs.size(), n, seg, pin.jobs(bufs.pinned, 0), stage, pin.results(bufs.pinned_dev, 0), c->stream);
    HIPCHK(hipGetLastError());
    if (nseg) g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    const unsigned long long* const res = pin.results(bufs.pinned, 0);
    int rc = WR_OK;
    for (int j = 0; j < njobs; j++) {
        if (res[2 * j + 1]) { if (!rc) rc = fail(WR_ERR_HIP, "job " + std::to_string(j) + ": internal: " + (strands ? "a record outgrew the record bound" : kOutgrew)); continue; }
        if (res[2 * j] > cap[j]) { if (!rc) rc = fail(WR_ERR_OVERFLOW, "job " + std::to_string(j) + ": the blob buffer is too small for the plane"); continue; }
        blob_len[j] = (size_t)res[2 * j];
    }
    return rc;
}

int wr_dev_seg_encode_batch(wr_ctx* c, int njobs, const unsigned char* const* d_sym, size_t n, unsigned seg, unsigned char* const* d_blob, const size_t* cap,
                            size_t* blob_len)
{
    return dev_seg_encode_batch(c, njobs, d_sym, n, seg, 0, d_blob, cap, blob_len);
}

int wr_dev_seg_encode_batch_strands(wr_ctx* c, int njobs, const unsigned char* const* d_sym, size_t n, unsigned seg, unsigned strands,
                                    unsigned char* const* d_blob, const size_t* cap, size_t* blob_len)
{
    return dev_seg_encode_batch(c, njobs, d_sym, n, seg, strands ? strands : WR_STRANDS_DEFAULT, d_blob, cap, blob_len);
}

// mixed == false: WRS1 blobs, a WRS3 blob is refused; mixed == true: WRS1, WRS2 and WRS3 blobs side by side, the symbols in
// stream order, the plain jobs in one launch and the stranded ones in another
static int dev_seg_decode_batch(wr_ctx* c, int njobs, const unsigned char* const* d_blob, const size_t* blob_len, unsigned char* const* d_sym, size_t n,
                                size_t* bad_segments, bool mixed)
{
    if (njobs < 1 || njobs > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (int rc = ctx_bind(c)) return rc;
    if (!d_blob || !blob_len || !d_sym) return fail(WR_ERR_ARG, "null array");
    for (int j = 0; j < njobs; j++) {
        if (!d_blob[j] || (n && !d_sym[j])) return fail(WR_ERR_ARG, "job " + std::to_string(j) + ": null pointer");
        if (((uintptr_t)d_sym[j] | (uintptr_t)d_blob[j]) & 15) return fail(WR_ERR_ARG, "job " + std::to_string(j) + ": plane and blob buffers must be 16-byte aligned");
        if (bad_segments) bad_segments[j] = 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    // every header, then every index, come to the host and are validated before anything is launched for any job
    std::vector<Front> front(njobs);
    unsigned long long lanes = 0;
    for (int j = 0; j < njobs; j++) {
        const std::string who = "job " + std::to_string(j) + ": ";
        const char* const no_strands = mixed ? nullptr : "a WRS3 blob: stranded segments are not decoded in a batch (wr_dev_seg_decode reads them)";
        if (int rc = fetch_front(d_blob[j], blob_len[j], n, mixed, no_strands, who, &front[j])) return rc;
        lanes += wrsb::job_lanes(front[j].nseg, front[j].strands);
    }
    if (lanes >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the batch has 2^31 segments or more");
    if (!lanes) return WR_OK;
    BatchBufs bufs(c);
    // (at most WR_SEG_BATCH_MAX jobs: a table for the plain jobs, one for the stranded ones, the failure counts behind them)
    const size_t tables = 2 * wrk::seg_batch_table_bytes(njobs);
    uint8_t* const d_once = bufs.take(tables + up256(4 * (size_t)njobs));
    if (!d_once) return WR_ERR_HIP;
    if (int rc = bufs.pin(tables)) return rc;
    unsigned int* const d_bad = reinterpret_cast<unsigned int*>(d_once + tables);
    std::vector<wrk::SegJob> jobs, stranded;
    for (int j = 0; j < njobs; j++) {
        const Front& f = front[j];
        uint8_t* work = nullptr;
        if (f.nseg) {
            if (!(work = bufs.take(batch_work_bytes(f.nseg)))) return WR_ERR_HIP;
            if (int rc = seg_upload_offsets(f.bytes.data(), wrseg::header_bytes(f.brick, f.strands), f.nseg, work)) return rc;
        }
        wrk::SegJob job = seg_job(wrk::plane_ref(d_sym[j]), d_blob[j], blob_len[j], work, n, f.seg, f.nseg, f.brick);
        job.strands = f.strands;
        job.bad = d_bad + j;
        (f.strands ? stranded : jobs).push_back(job);
    }
    StageLock cu(c->pool->cu_mu);
    HIPCHK(hipMemsetAsync(d_bad, 0, 4 * (size_t)njobs, c->stream));
    size_t at = 0;
    int launches = batch_chunk_launch(jobs, false, bufs.pinned, d_once, &at, c->stream);
    launches += batch_chunk_launch(stranded, true, bufs.pinned, d_once, &at, c->stream);
    HIPCHK(hipGetLastError());
    g_stat[WR_STAT_BATCH_CODER_LAUNCHES] += (unsigned long)launches;
    std::vector<unsigned int> bad(njobs, 0);
    HIPCHK(hipMemcpyAsync(bad.data(), d_bad, 4 * (size_t)njobs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = WR_OK;
    for (int j = 0; j < njobs; j++) {
        if (bad_segments) bad_segments[j] = bad[j];
        if (bad[j] && !rc) rc = fail(WR_ERR_STREAM, "job " + std::to_string(j) + ": segmented plane: " + bad_segments_text(bad[j]));
    }
    return rc;
}

int wr_dev_seg_decode_batch(wr_ctx* c, int njobs, const unsigned char* const* d_blob, const size_t* blob_len, unsigned char* const* d_sym, size_t n,
                            size_t* bad_segments)
{
    return dev_seg_decode_batch(c, njobs, d_blob, blob_len, d_sym, n, bad_segments, false);
}

int wr_dev_seg_decode_batch_mixed(wr_ctx* c, int njobs, const unsigned char* const* d_blob, const size_t* blob_len, unsigned char* const* d_sym, size_t n,
                                  size_t* bad_segments)
{
    return dev_seg_decode_batch(c, njobs, d_blob, blob_len, d_sym, n, bad_segments, true);
}

// ---- the batch calls for WRS3: the encoders with `strands` (0: WR_STRANDS_DEFAULT), the decoders that take any mix of formats
int wr_encode_host_seg_batch_strands(wr_ctx* c, int nfields, const double* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                     const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* infos,
                                     unsigned char* const* data_encs, const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, infos, data_encs, caps, tm);
}

int wr_encode_host_seg_batch_strands_f32(wr_ctx* c, int nfields, const float* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                         const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* infos,
                                         unsigned char* const* data_encs, const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, infos, data_encs, caps, tm);
}

int wr_encode_device_seg_batch_strands(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                       const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* infos,
                                       unsigned char* const* data_encs, const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands ? strands : WR_STRANDS_DEFAULT, infos, data_encs, caps, tm);
}

int wr_decode_host_seg_batch_mixed(wr_ctx* c, int nfields, double* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                   const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm, true);
}

int wr_decode_host_seg_batch_mixed_f32(wr_ctx* c, int nfields, float* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                       const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm, true);
}

int wr_decode_device_seg_batch_mixed(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                     const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm, true);
}

// ---- masks across a batch: the stage calls, the sizing, and the whole-path calls (MaskBatchEncode / MaskBatchDecode above)
int wr_dev_mask_split_batch(wr_ctx* c, int nfields, const double* const* d_flds, size_t n, double below, unsigned char* const* d_bits,
                            unsigned long long* undefined, double* pad)
{
    return dev_mask_split_batch(c, nfields, d_flds, n, below, d_bits, undefined, pad);
}
int wr_dev_mask_split_batch_f32(wr_ctx* c, int nfields, const float* const* d_flds, size_t n, double below, unsigned char* const* d_bits,
                                unsigned long long* undefined, double* pad)
{
    return dev_mask_split_batch(c, nfields, d_flds, n, below, d_bits, undefined, pad);
}
int wr_dev_mask_fill_batch(wr_ctx* c, int nfields, double* const* d_flds, size_t n, const unsigned char* const* d_bits, const double* values)
{
    return dev_mask_fill_batch(c, nfields, d_flds, n, d_bits, values);
}
int wr_dev_mask_fill_batch_f32(wr_ctx* c, int nfields, float* const* d_flds, size_t n, const unsigned char* const* d_bits, const double* values)
{
    return dev_mask_fill_batch(c, nfields, d_flds, n, d_bits, values);
}

int wr_dev_mask_check_batch(wr_ctx* c, int nmasks, const unsigned char* const* d_bits, size_t n, unsigned long long* undefined, unsigned char* beyond)
{
    if (int rc = mask_batch_args(c, nmasks, "nmasks", reinterpret_cast<const void* const*>(d_bits), reinterpret_cast<const void* const*>(d_bits), n)) return rc;
    if (!undefined || !beyond) return fail(WR_ERR_ARG, "null array");
    std::lock_guard<std::mutex> lk(c->mu);
    BatchBufs bufs(c);
    MaskPinned pin(c);
    if (int rc = pin.alloc((size_t)nmasks * sizeof(uint8_t*))) return rc;
    unsigned long long* const d_counters = reinterpret_cast<unsigned long long*>(bufs.take(mask_batch_counters_bytes(nmasks)));
    if (!d_counters) return WR_ERR_HIP;
    memcpy(pin.host, d_bits, (size_t)nmasks * sizeof(uint8_t*));
    std::vector<unsigned long long> got(2 * (size_t)nmasks);
    StageLock cu(c->pool->cu_mu);
    wrk::mask_check_batch(reinterpret_cast<const uint8_t* const*>(pin.dev), nmasks, n, d_counters, c->stream);
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched mask check launch failed");
    HIPCHK(hipMemcpyAsync(got.data(), d_counters, 8 * got.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int m = 0; m < nmasks; m++) { undefined[m] = got[2 * (size_t)m]; beyond[m] = got[2 * (size_t)m + 1] ? 1 : 0; }
    return WR_OK;
}

size_t wr_seg_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int nlay, unsigned seg, unsigned brick, unsigned strands, int decode)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (nfields < 1 || nfields > WR_SEG_BATCH_MAX || !n || nlay < 0 || nlay > WR_NLAYMAX || !wrseg::seg_ok(seg) || (brick && !wrblk::brick_ok(brick))) return 0;
    if (strands && !wrseg::strands_ok(strands, seg)) return 0;
    if (nmasked < 0 || nmasked > nfields) return 0;
    // strands == 0 means WRS1 / WRS2 planes here (nothing is defaulted but seg).  An encode of such planes is the plain batch
    // call's; their decode is the mixed driver's all the same, with the blobs at the WRS1 / WRS2 bound.  (nlay == 0, fields that
    // are constant once padded: the base is 0 and the masks' share remains.)
    size_t base = 0;
    if (strands) base = wr_seg_batch_device_bytes_strands(nfields, n, nlay, seg, brick, strands, decode);
    else if (!decode) base = wr_seg_batch_device_bytes(nfields, n, nlay, seg, brick, 0);
    else {
        const size_t jobs = (size_t)nfields * (size_t)nlay;
        base = jobs * (batch_plane_bytes(n) + up256(seg_blob_cap(n, seg, brick, 0)) + up256(batch_work_bytes(wrseg::seg_count(n, seg))) + batch_perm_bytes(n, brick)) +
               up256(batch_mixed_once_bytes(0, jobs));
    }
    const size_t M = (size_t)nmasked, nsym = wrmask::mask_bytes(n);
    if (!decode) {
        const size_t stage = M ? up256(wrk::seg_batch_stage_bytes(M, nsym, seg)) : 0;
        return base + M * (mask_batch_bits_bytes(n) + up256(mask_batch_blob_cap(n, seg))) + stage + mask_batch_partial_bytes((size_t)nfields, n);
    }
    // the masks are plain jobs of the mixed launch: their tables and failure counts beside the planes', which the base sizes as
    // stranded jobs
    const size_t jobs = (size_t)nfields * (size_t)nlay;
    const size_t once = up256(batch_mixed_once_bytes(M, jobs)) - up256(batch_mixed_once_bytes(0, jobs));
    return base + M * (mask_batch_bits_bytes(n) + up256(wr_mask_bound(n, seg)) + up256(batch_work_bytes(wrseg::seg_count(nsym, seg)))) + once +
           mask_batch_counters_bytes(M);
}

static int encode_seg_batch_masked(wr_ctx* c, int nfields, const std::vector<FieldRef>& flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                   const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* infos,
                                   unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, wr_mask_result* results)
{
    if (below != below) return fail(WR_ERR_ARG, "the threshold `below` is a NaN (-INFINITY switches it off)");
    MaskBatchEncode m;
    m.below = below;
    const int rc = encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands, infos, data_encs, caps, tm, &m);
    if (rc == WR_OK && results)
        for (int f = 0; f < nfields; f++) m.result(f, &results[f]);
    return rc;
}

int wr_encode_host_seg_batch_masked(wr_ctx* c, int nfields, const double* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                    const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* infos,
                                    unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return encode_seg_batch_masked(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands, below, infos, data_encs, caps, tm, results);
}
int wr_encode_host_seg_batch_masked_f32(wr_ctx* c, int nfields, const float* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                        const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* infos,
                                        unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return encode_seg_batch_masked(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands, below, infos, data_encs, caps, tm, results);
}
int wr_encode_device_seg_batch_masked(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                      const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* infos,
                                      unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return encode_seg_batch_masked(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, strands, below, infos, data_encs, caps, tm, results);
}

static int decode_seg_batch_masked(wr_ctx* c, int nfields, const std::vector<FieldRef>& flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                   const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm, wr_mask_result* results)
{
    if (!infos || !data_encs || !data_lens) return fail(WR_ERR_ARG, "null array");
    // data_lens[f] == infos[f].ntot_enc or 0: an unmasked record (a shorter buffer: the plain driver refuses it)
    MaskBatchDecode m;
    m.fill = fill;
    m.job.resize(nfields);
    std::vector<size_t> field_lens(nfields);
    for (int f = 0; f < nfields; f++) {
        field_lens[f] = data_lens[f];
        if (data_lens[f] == 0 || data_lens[f] <= infos[f].ntot_enc) continue;
        if (!data_encs[f]) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": null coded buffer");
        m.job[f].blob = data_encs[f] + infos[f].ntot_enc;
        m.job[f].len = data_lens[f] - infos[f].ntot_enc;
        field_lens[f] = infos[f].ntot_enc;
    }
    const int rc = decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, field_lens.data(), tm, true, &m);
    if (rc == WR_OK && results)
        for (int f = 0; f < nfields; f++) m.result(f, &results[f]);
    return rc;
}

int wr_decode_host_seg_batch_masked(wr_ctx* c, int nfields, double* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                    const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return decode_seg_batch_masked(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, fill, tm, results);
}
int wr_decode_host_seg_batch_masked_f32(wr_ctx* c, int nfields, float* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                        const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return decode_seg_batch_masked(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, fill, tm, results);
}
int wr_decode_device_seg_batch_masked(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                      const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm, wr_mask_result* results)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return decode_seg_batch_masked(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, fill, tm, results);
}

int wr_encode_host_seg_batch(wr_ctx* c, int nfields, const double* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                             const double* const* cutoffvecs, unsigned seg, unsigned brick, wr_enc_info* infos, unsigned char* const* data_encs,
                             const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, 0, infos, data_encs, caps, tm);
}

int wr_decode_host_seg_batch(wr_ctx* c, int nfields, double* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                             const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 0, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm);
}

int wr_encode_host_seg_batch_f32(wr_ctx* c, int nfields, const float* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                 const double* const* cutoffvecs, unsigned seg, unsigned brick, wr_enc_info* infos, unsigned char* const* data_encs,
                                 const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, 0, infos, data_encs, caps, tm);
}

int wr_decode_host_seg_batch_f32(wr_ctx* c, int nfields, float* const* h_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                                 const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, h_flds, 1, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm);
}

int wr_encode_device_seg_batch(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                               const double* const* cutoffvecs, unsigned seg, unsigned brick, wr_enc_info* infos, unsigned char* const* data_encs,
                               const size_t* caps, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return encode_seg_batch_impl(c, nfields, flds, nx, ny, nz, wtflag, mx, my, mz, cutoffvecs, seg, brick, 0, infos, data_encs, caps, tm);
}

int wr_decode_device_seg_batch(wr_ctx* c, int nfields, double* const* d_flds, int nx, int ny, int nz, const wr_enc_info* infos,
                               const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    std::vector<FieldRef> flds;
    if (int rc = batch_fields(nfields, d_flds, 2, &flds)) return rc;
    return decode_seg_batch_impl(c, nfields, flds, nx, ny, nz, infos, data_encs, data_lens, tm);
}

}  // extern "C"

// ---- region decode, many regions per call (include/waverange_amd.h): the union of the regions' segments is uploaded and decoded
// once -- on a WRS1 / WRS2 stream by ONE launch over all used planes (k_seg_decode_list_batch: a job per plane, a lane per
// listed segment), on a WRS3 stream by one launch per plane --, then every region is finished as the single-region call
// finishes its one (roi_from_planes), its crop landing at its offset of one output buffer.  No new format, and the
// single-region drivers above are not touched: region i is bit for bit their result for rois[i] alone, because the planes hold
// the same symbols wherever a window reads them and the window stage is the same code.
namespace {

// the plan of every region and offs[0 .. nroi], the exclusive prefix of their element counts; the first bad region decides
int roi_multi_plans(int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi, const wr_enc_info* info,
                    std::vector<LowresPlan>* pls, std::vector<size_t>* offs)
{
    if (nroi < 1 || nroi > WR_ROI_MULTI_MAX) return fail(WR_ERR_ARG, "nroi must be in 1.." + std::to_string(WR_ROI_MULTI_MAX));
    if (!rois) return fail(WR_ERR_ARG, "null region array");
    pls->resize((size_t)nroi);
    offs->assign((size_t)nroi + 1, 0);
    size_t run = 0;
    for (int i = 0; i < nroi; i++) {
        if (int rc = region_plan(nx, ny, nz, level, max_planes, &rois[i], info, &(*pls)[i])) return fail_at("region", i, rc);
        (*offs)[i] = run;
        run += (*pls)[i].out_elems();
    }
    (*offs)[nroi] = run;
    return WR_OK;
}

// the slot of the window stage: sized for the largest window of the plans, and no smaller than `need` (a batch: the fields in turn)
SlotNeed roi_multi_need(const std::vector<LowresPlan>& pls, SlotNeed need = SlotNeed())
{
    for (const LowresPlan& pl : pls) {
        SlotNeed nd;
        pl.need(false, &nd);
        need.field_elems = std::max(need.field_elems, nd.field_elems);
        need.scratch_elems = std::max(need.scratch_elems, nd.scratch_elems);
        need.lowbuf_elems = std::max(need.lowbuf_elems, nd.lowbuf_elems);
    }
    return need;
}

// What the regions of one field need of its stream: on a blocked stream the union of their bricks, the same in every plane, and
// per used plane the union of the segments (ids[0 .. used)).  false: a blocked stream with too many bricks.
bool roi_multi_lists(const SegStream& s, int nx, int ny, int nz, const std::vector<LowresPlan>& pls, int used, std::vector<uint32_t>* ids,
                     std::vector<uint32_t>* bricks)
{
    std::vector<wrroi::Geometry> geos(pls.size());
    for (size_t i = 0; i < pls.size(); i++) geos[i] = pls[i].win;
    if (s.brick) {
        if (s.od.nbricks > 0x7fffffffu) return false;
        wrblk::region_bricks_multi(s.od, geos.data(), geos.size(), bricks);
    }
    seg_plane_lists(s, used, ids, [&](uint32_t seg, std::vector<uint32_t>* out) {
        if (s.brick) {
            out->resize(wrblk::region_segments_multi(s.od, geos.data(), geos.size(), seg, nullptr, 0));
            wrblk::region_segments_multi(s.od, geos.data(), geos.size(), seg, out->data(), out->size());
        } else {
            out->resize(wrroi::segments_of_multi(nx, ny, nz, geos.data(), geos.size(), seg, nullptr, 0));
            wrroi::segments_of_multi(nx, ny, nz, geos.data(), geos.size(), seg, out->data(), out->size());
        }
    });
    return true;
}

// Kernel stage (slot leased, cu_mu held): the regions one after another on the stream, region i's crop at d_out + offs[i]
// elements (fp32 elements if f32).  tm != nullptr: quant_ms and transform_ms are summed into it, which takes a wait per region
// (the context has one set of events).
int roi_multi_from_planes(wr_ctx* c, Slot* s, void* d_out, int nx, int ny, const std::vector<LowresPlan>& pls, const std::vector<size_t>& offs,
                          const wrk::DequantParams& p, bool f32, wr_timings* tm)
{
    for (size_t i = 0; i < pls.size(); i++) {
        uint8_t* const at = reinterpret_cast<uint8_t*>(d_out) + offs[i] * (f32 ? sizeof(float) : sizeof(double));
        void* landed = nullptr;
        if (int rc = roi_from_planes(c, s, reinterpret_cast<double*>(at), nx, ny, pls[i], p, f32, &landed)) return fail_at("region", (int)i, rc);
        if (!tm) continue;
        float ms = 0;
        HIPCHK(hipEventSynchronize(c->ev_c));
        HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b)); tm->quant_ms += ms;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_b, c->ev_c)); tm->transform_ms += ms;
    }
    return WR_OK;
}

int decode_seg_roi_multi_impl(wr_ctx* c, FieldRef fld, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                              const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!info) return fail(WR_ERR_ARG, "null wr_enc_info");
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null output pointer");
    std::vector<LowresPlan> pls;
    std::vector<size_t> out_at;
    if (int rc = roi_multi_plans(nx, ny, nz, level, max_planes, rois, nroi, info, &pls, &out_at)) return rc;
    c->pend_valid = false;
    PlaneHold planes(c);
    SegBufs bufs(c);
    BatchBufs more(c);  // the extra stream-order planes of a blocked stream, the job table, a host caller's output
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz, total = out_at[(size_t)nroi];
    const bool f32 = fld.host_f32 != nullptr;
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    // every plane's header and index, used or not, are validated (region_plan has refused what seg_stream_of would of nlay and wlev)
    SegStream s;
    if (int rc = seg_stream_of(nx, ny, nz, info, data_enc, data_len, &s)) return rc;
    if (s.constant) return finish_constant(c, fld, total, info->midval, t0, &local, tm);  // midval in every region
    const int used = pls[0].planes;
    std::vector<uint32_t> bricks, ids[WR_NLAYMAX];
    if (!roi_multi_lists(s, nx, ny, nz, pls, used, ids, &bricks)) return fail(WR_ERR_ARG, "too many bricks");
    unsigned long long lanes = 0;
    for (int l = 0; l < used; l++) lanes += ids[l].size();
    if (lanes >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the call has 2^31 segments or more");
    const bool one_launch = s.strands == 0;
    const size_t table_bytes = wrk::seg_lists_table_bytes((size_t)used);
    uint8_t* perm[WR_NLAYMAX] = {nullptr};  // the plane in stream order: one per used plane on the one-launch path
    uint8_t* d_table = nullptr;
    uint8_t* d_host_out = nullptr;
    {
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);
        if (s.brick) {
            bufs.perm = plane_scratch(c, n);
            bufs.bricks = plane_scratch(c, 4 * bricks.size() + 4);
            if (!bufs.perm.p || !bufs.bricks.p) return WR_ERR_HIP;
            perm[0] = bufs.perm.p;
            for (int l = 1; l < used; l++) {
                perm[l] = one_launch ? more.take(n) : perm[0];
                if (!perm[l]) return WR_ERR_HIP;
            }
        }
        for (int l = 0; l < used; l++)
            if (int rc = seg_plane_bufs(c, &bufs, l, n, info->len_enc_vec[l], wrk::seg_decode_list_work_bytes(s.nseg[l], ids[l].size()), false, l == 0 || !one_launch))
                return rc;
        if (one_launch) {
            d_table = more.take(table_bytes);
            if (!d_table) return WR_ERR_HIP;
            if (int rc = more.pin(table_bytes)) return rc;
        }
        if (!fld.dev) {
            d_host_out = more.take(total * (f32 ? sizeof(float) : sizeof(double)));
            if (!d_host_out) return WR_ERR_HIP;
        }
    }
    size_t bytes_up = 0;
    if (int rc = seg_upload_lists(c, s, used, data_enc, &bufs, ids, bricks, &local.h2d_ms, &bytes_up)) return rc;
    g_stat[WR_STAT_ROI_BYTES_UP] += bytes_up;
    const double t_coded = now();
    const SlotNeed need = roi_multi_need(pls);
    SlotLease slot;
    if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    wrk::DequantParams p;
    if (int rc = dequant_params(info, used, n, [&](int l) { return c->ps[l].ref; }, &p)) return rc;
    void* const d_out = fld.dev ? (void*)fld.dev : (void*)d_host_out;
    int rc = WR_OK;
    {
        StageLock cu(pool->cu_mu);
        clock_warmup(c, need.field_elems);
        CoderCall k{&s, info, used, n, &bufs, p.q};
        memcpy(k.perm, perm, sizeof perm);
        k.ids = ids;
        k.d_bricks = reinterpret_cast<const uint32_t*>(bufs.bricks.p); k.nbricks = bricks.size();
        k.host_table = more.pinned; k.d_table = d_table;  // (both null on a WRS3 stream: a launch per plane)
        k.stat_segments = WR_STAT_ROI_SEGMENTS;
        k.stat_launches = true;
        if (int rc = seg_coder_stage(c, k, &local)) return rc;
        launch_note(c, "dequant_window", used - 1, slot->field, need.field_elems, nullptr, p.q[used - 1]);
        rc = kernel_stage_end(c, roi_multi_from_planes(c, slot.get(), d_out, nx, ny, pls, out_at, p, f32, tm ? &local : nullptr));
    }
    if (rc) return rc;
    return finish_call(c, fld, d_host_out, d_host_out, total, false, t0, t_coded, t_phase, &local, tm);
}

}  // namespace

extern "C" {

int wr_dev_decode_planes_roi_multi(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                   const unsigned char* d_planes, const wr_enc_info* info)
{
    if (int rc = ctx_bind(c)) return rc;
    if (int rc = check_dims(nx, ny, nz, d_out)) return rc;
    if (!d_out || !info) return fail(WR_ERR_ARG, "null pointer");
    std::vector<LowresPlan> pls;
    std::vector<size_t> out_at;
    if (int rc = roi_multi_plans(nx, ny, nz, level, max_planes, rois, nroi, info, &pls, &out_at)) return rc;
    const size_t n = (size_t)nx * ny * nz;
    std::lock_guard<std::mutex> lk(c->mu);
    if (info->ntot_enc == 0 && info->nlay == 0) return fill_constant(c, FieldRef{d_out}, out_at[(size_t)nroi], info->midval);
    if (!d_planes) return fail(WR_ERR_ARG, "null plane pointer");
    SlotLease slot;
    if (int rc = slot.acquire(c, roi_multi_need(pls))) return rc;
    StageLock cu(c->pool->cu_mu);
    wrk::DequantParams p;
    memset(&p, 0, sizeof p);
    p.nlay = pls[0].planes;
    for (int l = 0; l < p.nlay; l++) {
        p.q[l] = wrk::plane_ref(d_planes + l * wr_plane_pitch(n));
        p.deps[l] = info->deps_vec[l];
        p.minval[l] = info->minval_vec[l];
    }
    int rc = roi_multi_from_planes(c, slot.get(), d_out, nx, ny, pls, out_at, p, false, nullptr);
    if (rc == WR_OK && hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "kernel launch failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == WR_OK) rc = fail(WR_ERR_HIP, "the region kernel stage failed on the device");
    return rc;
}

int wr_dev_seg_decode_lists(wr_ctx* c, int njobs, const unsigned char* const* d_blob, const size_t* blob_len, unsigned char* const* d_sym, const size_t* n,
                            const uint32_t* const* ids, const size_t* nlist, size_t* bad_segments)
{
    if (njobs < 1 || njobs > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (int rc = ctx_bind(c)) return rc;
    if (!d_blob || !blob_len || !d_sym || !n || !ids || !nlist) return fail(WR_ERR_ARG, "null array");
    for (int j = 0; j < njobs; j++) {
        const std::string who = "job " + std::to_string(j) + ": ";
        if (!d_blob[j] || (n[j] && !d_sym[j]) || (nlist[j] && !ids[j])) return fail(WR_ERR_ARG, who + "null pointer");
        if (((uintptr_t)d_sym[j] | (uintptr_t)d_blob[j]) & 15) return fail(WR_ERR_ARG, who + "plane and blob buffers must be 16-byte aligned");
        if (bad_segments) bad_segments[j] = 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    // every header, index and list is validated on the host before anything is launched for any job
    std::vector<Front> front(njobs);
    unsigned long long lanes = 0;
    for (int j = 0; j < njobs; j++) {
        const std::string who = "job " + std::to_string(j) + ": ";
        if (int rc = fetch_front(d_blob[j], blob_len[j], n[j], true, "a WRS3 blob: stranded segments have no batched list decoder", who, &front[j])) return rc;
        if (nlist[j] > front[j].nseg) return fail(WR_ERR_ARG, who + "the list is longer than the plane has segments");
        for (size_t i = 0; i < nlist[j]; i++)
            if (ids[j][i] >= front[j].nseg || (i && ids[j][i] <= ids[j][i - 1])) return fail(WR_ERR_ARG, who + "the list must be ascending, every id below the segment count");
        lanes += nlist[j];
    }
    if (lanes >= kBatchLaneLimit) return fail(WR_ERR_ARG, "too many segments: the launch has 2^31 lanes or more");
    if (!lanes) return WR_OK;
    BatchBufs bufs(c);
    const size_t table = wrk::seg_lists_table_bytes(njobs);
    uint8_t* const d_table = bufs.take(table);
    if (!d_table) return WR_ERR_HIP;
    if (int rc = bufs.pin(table)) return rc;
    std::vector<wrk::SegJob> jobs(njobs);
    std::vector<wrk::SegList> lists(njobs);
    std::vector<uint8_t*> works(njobs, nullptr);
    for (int j = 0; j < njobs; j++) {
        const Front& f = front[j];
        memset(&lists[j], 0, sizeof lists[j]);
        if (nlist[j]) {
            uint8_t* const work = works[j] = bufs.take(wrk::seg_decode_list_work_bytes(f.nseg, nlist[j]));
            if (!work) return WR_ERR_HIP;
            if (int rc = seg_upload_offsets(f.bytes.data(), wrseg::header_bytes(f.brick), f.nseg, work)) return rc;
            HIPCHK(hipMemcpy(wrk::seg_decode_list_ids(work, f.nseg), ids[j], nlist[j] * sizeof(uint32_t), hipMemcpyHostToDevice));
            lists[j].ids = wrk::seg_decode_list_ids(work, f.nseg);
            lists[j].nlist = (uint32_t)nlist[j];
        }
        jobs[j] = seg_job(wrk::plane_ref(d_sym[j]), d_blob[j], blob_len[j], works[j], n[j], f.seg, f.nseg, f.brick);
    }
    StageLock cu(c->pool->cu_mu);
    for (int j = 0; j < njobs; j++) if (works[j]) HIPCHK(hipMemsetAsync(wrk::seg_work_bad(works[j]), 0, sizeof(unsigned int), c->stream));
    wrk::seg_decode_lists(jobs.data(), lists.data(), jobs.size(), bufs.pinned, d_table, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<unsigned int> bad(njobs, 0);
    for (int j = 0; j < njobs; j++) if (works[j]) HIPCHK(hipMemcpyAsync(&bad[j], wrk::seg_work_bad(works[j]), sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = WR_OK;
    for (int j = 0; j < njobs; j++) {
        if (bad_segments) bad_segments[j] = bad[j];
        if (bad[j] && !rc) rc = fail(WR_ERR_STREAM, "job " + std::to_string(j) + ": segmented plane: " + bad_segments_text(bad[j]));
    }
    return rc;
}

int wr_decode_host_seg_roi_multi(wr_ctx* c, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                 const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host = h_out;
    return decode_seg_roi_multi_impl(c, f, nx, ny, nz, level, max_planes, rois, nroi, info, data_enc, data_len, tm);
}

int wr_decode_host_seg_roi_multi_f32(wr_ctx* c, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                     const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_out;
    return decode_seg_roi_multi_impl(c, f, nx, ny, nz, level, max_planes, rois, nroi, info, data_enc, data_len, tm);
}

int wr_decode_device_seg_roi_multi(wr_ctx* c, double* d_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                   const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    return decode_seg_roi_multi_impl(c, f, nx, ny, nz, level, max_planes, rois, nroi, info, data_enc, data_len, tm);
}

}  // extern "C"

// ---- region decode across a batch of fields (include/waverange_amd.h): the listed segments of all used planes of N fields in
// at most TWO coder launches -- the WRS1 / WRS2 jobs through k_seg_decode_list_batch, the WRS3 jobs through
// k_strand_decode_list_batch --, then every field's regions through the window stage of the many-region call.  A job is one
// (non-constant field, used plane) with the union of the segments the regions need, as the many-region call lists it.  The
// stages are the ones above; field f's part of the output is bit for bit the many-region call's for that field alone, because
// its planes hold the same symbols wherever a window reads them and the window stage is the same code.
namespace {

// What the call takes from the plane pool, piece by piece; the driver allocates by these and wr_seg_roi_batch_device_bytes sums
// them with every list at its longest and every blob at its bound.
size_t roi_batch_work_bytes(size_t nseg, size_t nlist) { return wrk::seg_decode_list_work_bytes(nseg, nlist); }  // per job
size_t roi_batch_bricks_bytes(size_t nbricks) { return 4 * nbricks + 4; }                                        // per WRS2 field
// once per call: the two job tables and a failure count per job (plain: the WRS1 / WRS2 jobs, stranded: the WRS3 jobs)
size_t roi_batch_tables_bytes(size_t plain, size_t stranded) { return wrk::seg_lists_table_bytes(plain) + wrk::strand_lists_table_bytes(stranded); }
size_t roi_batch_once_bytes(size_t plain, size_t stranded) { return roi_batch_tables_bytes(plain, stranded) + up256(4 * (plain + stranded)); }

// The jobs of a coder stage over lists, in the two groups the two kernels take
struct ListJobs {
    std::vector<wrk::SegJob> plain, stranded;
    std::vector<wrk::SegList> plain_lists;
    std::vector<wrk::StrandList> strand_lists;
    void add(const wrk::SegJob& job, const uint32_t* d_ids, size_t nlist, uint32_t strands)
    {
        if (strands) {
            wrk::StrandList ls;
            memset(&ls, 0, sizeof ls);
            ls.ids = d_ids; ls.nlist = (uint32_t)nlist;
            ls.K = strands; ls.kshift = wrsb::strands_shift(strands); ls.L = wrseg::strand_len(job.seg, strands);
            stranded.push_back(job);
            strand_lists.push_back(ls);
        } else {
            wrk::SegList ls;
            memset(&ls, 0, sizeof ls);
            ls.ids = d_ids; ls.nlist = (uint32_t)nlist;
            add(job, ls);
        }
    }
    void add(const wrk::SegJob& job, const wrk::SegList& ls) { plain.push_back(job); plain_lists.push_back(ls); }
    // the lanes of the two launches, each below 2^31 (false: refused)
    bool lanes_ok() const
    {
        unsigned long long a = 0, b = 0;
        for (const wrk::SegList& l : plain_lists) a += l.nlist;
        for (const wrk::StrandList& l : strand_lists) b += wrsb::job_lanes(l.nlist, l.K);
        return a < wrsb::kLaneLimit && b < wrsb::kLaneLimit;
    }
    // (cu_mu held) host_table / d_table: roi_batch_tables_bytes(plain.size(), stranded.size()), pinned and device.  Returns the
    // launches made: 0, 1 or 2.
    int launch(uint8_t* host_table, uint8_t* d_table, hipStream_t st) const
    {
        int launches = 0;
        const size_t at = wrk::seg_lists_table_bytes(plain.size());
        if (!plain.empty() && wrk::seg_decode_lists(plain.data(), plain_lists.data(), plain.size(), host_table, d_table, st)) launches++;
        if (!stranded.empty() && wrk::strand_decode_lists(stranded.data(), strand_lists.data(), stranded.size(), host_table + at, d_table + at, st)) launches++;
        return launches;
    }
};

struct RoiBatchField : BatchField {  // ... of a region decode: its plans, its lists, its brick list
    std::vector<LowresPlan> pls;
    int used = 0;
    std::vector<uint32_t> ids[WR_NLAYMAX], bricks;
    uint8_t* perms[WR_NLAYMAX] = {nullptr};  // a WRS2 field: one stream-order plane per job (all jobs go in one launch)
    uint8_t* d_bricks = nullptr;
    int job0 = 0;  // its first job's place in the failure counts
    // a masked record of the masked call (mask.len != 0): its blob as the host has validated it, the union of the mask
    // segments the regions need and the job's buffers (MaskJob); the job's place in the failure counts comes behind the planes'
    MaskJob mask;
    bool has_mask() const { return mask.len != 0; }
};

// what the masked call adds (wr_decode_*_seg_roi_batch_masked)
struct MaskBatch {
    double fill;
    wr_mask_result* res;  // nfields records, or nullptr
};

// what a masked field adds to the call's memory: the mask plane at its pitch (the blob and the work buffer go by
// roi_batch_work_bytes and the blob's length), and once the restore's table
size_t roi_batch_mask_plane_bytes(size_t n) { return batch_plane_bytes(wrmask::mask_bytes(n)); }
size_t roi_batch_restore_bytes(size_t nroi, size_t nfields) { return wrk::mask_boxes_table_bytes(nroi, nfields); }

// mb != nullptr (wr_decode_*_seg_roi_batch_masked): a record whose buffer is longer than its planes carries a mask blob.  The
// blob is one more job of the WRS1 / WRS2 launch (a plane of ceil(n / 8) symbols, the union of wrmask::roi_segments over the
// regions listed), judged with the field parts before any dequantiser runs; `fill` goes into every region of every such field
// in one launch behind the window stage (k_mask_restore_boxes).  A constant field with a blob is made on the device, for a
// host caller too, so that the restore finds it.
int decode_seg_roi_batch_impl(wr_ctx* c, FieldRef fld, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                              const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm,
                              const MaskBatch* mb = nullptr)
{
    if (nfields < 1) return fail(WR_ERR_ARG, "nfields must be at least 1");
    if (!infos || !data_encs || !data_lens) return fail(WR_ERR_ARG, "null array");
    if (int rc = ctx_bind(c)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    ActiveCall active(c->pool);
    if (tm) wrdma::enable_timing();
    if (int rc = check_dims(nx, ny, nz, fld.dev)) return rc;
    if (fld.none()) return fail(WR_ERR_ARG, "null output pointer");
    const double t0 = now();
    const size_t n = (size_t)nx * ny * nz;
    const bool f32 = fld.host_f32 != nullptr;
    const size_t elem = f32 ? sizeof(float) : sizeof(double);
    wr_timings local; memset(&local, 0, sizeof local);
    DevPool* const pool = c->pool;
    // ---- 1. every field's region plans against its own record; 2. every field's stream, every plane's header and index
    std::vector<RoiBatchField> bf((size_t)nfields);
    std::vector<size_t> out_at;
    for (int f = 0; f < nfields; f++)
        if (int rc = roi_multi_plans(nx, ny, nz, level, max_planes, rois, nroi, &infos[f], &bf[f].pls, &out_at)) return fail_at("field", f, rc);
    const size_t T = out_at[(size_t)nroi];  // (the regions' extents do not depend on the record)
    size_t njobs = 0, nmask = 0;
    for (int f = 0; f < nfields; f++) {
        RoiBatchField& b = bf[f];
        const bool masked = mb && data_lens[f] != 0 && data_lens[f] > infos[f].ntot_enc;  // (as the single masked call tells the two apart)
        if (int rc = seg_stream_of(nx, ny, nz, &infos[f], data_encs[f], masked ? infos[f].ntot_enc : data_lens[f], &b.s, "field " + std::to_string(f) + ": ")) return rc;
        if (masked) {
            b.mask.len = data_lens[f] - infos[f].ntot_enc;
            nmask++;
        }
        if (b.s.constant) continue;
        b.used = b.pls[0].planes;
        njobs += (size_t)b.used;
    }
    // ---- 3. (the masked call) every blob's header and whole segment index, as the single masked region call validates them
    for (int f = 0; f < nfields; f++) {
        if (!bf[f].has_mask()) continue;
        if (!data_encs[f]) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": null coded buffer");
        bf[f].mask.blob = data_encs[f] + infos[f].ntot_enc;
    }
    for (int f = 0; f < nfields; f++) {
        std::string why;
        if (bf[f].has_mask() && !bf[f].mask.parse(n, &why)) return fail(WR_ERR_STREAM, "field " + std::to_string(f) + ": " + why);
    }
    if (njobs + nmask > WR_SEG_BATCH_MAX)
        return fail(WR_ERR_ARG, "too many jobs: the call has " + std::to_string(njobs) + " (field, plane) pairs" + (mb ? " and " + std::to_string(nmask) + " masks" : std::string()) +
                                    ", WR_SEG_BATCH_MAX is " + std::to_string(WR_SEG_BATCH_MAX));
    std::vector<wrmask::Region> mregions;
    if (nmask) {
        for (int i = 0; i < nroi; i++) mregions.push_back(mask_region(nx, ny, nz, level, &rois[i]));
        if (!wrmask::boxes_turns(mregions.data(), mregions.size(), nullptr) ||
            (unsigned long long)nmask * wrmask::boxes_turns(mregions.data(), mregions.size(), nullptr) >= wrmask::kTurnLimit)
            return fail(WR_ERR_ARG, "too many turns: the restore launch of the call has 2^31 or more");
    }
    const size_t nall = njobs + nmask;  // the jobs of the coder launches: the (field, plane) pairs and the masks
    // ---- per field the union of the bricks and, per used plane, of the segments the regions need (as the many-region call)
    size_t nplain = 0, nstranded = 0;
    unsigned long long lanes_plain = 0, lanes_stranded = 0;
    SlotNeed need;
    for (int f = 0; f < nfields; f++) {
        RoiBatchField& b = bf[f];
        if (b.s.constant) continue;
        const SegStream& s = b.s;
        if (!roi_multi_lists(s, nx, ny, nz, b.pls, b.used, b.ids, &b.bricks)) return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": too many bricks");
        for (int l = 0; l < b.used; l++) {
            if (s.strands) lanes_stranded += wrsb::job_lanes(b.ids[l].size(), s.strands);
            else lanes_plain += b.ids[l].size();
        }
        (s.strands ? nstranded : nplain) += (size_t)b.used;
        need = roi_multi_need(b.pls, need);
    }
    // a mask is a WRS1 plane in the natural order whatever its field part is: one more job of the plain launch
    for (int f = 0; f < nfields; f++) {
        RoiBatchField& b = bf[f];
        if (!b.has_mask()) continue;
        b.mask.list(mregions.data(), mregions.size());
        lanes_plain += b.mask.ids.size();
        nplain++;
    }
    if (lanes_plain >= wrsb::kLaneLimit || lanes_stranded >= wrsb::kLaneLimit) return fail(WR_ERR_ARG, "too many segments: a launch of the call has 2^31 lanes or more");
    c->pend_valid = false;
    PlaneHold planes(c);
    BatchBufs bufs(c);
    uint8_t *d_once = nullptr, *d_host_out = nullptr, *d_restore = nullptr;
    const size_t tables = roi_batch_tables_bytes(nplain, nstranded);
    {
        std::lock_guard<std::mutex> gather(pool->planes.gather_mu);  // one decode at a time gathers its planes (decode_impl)
        for (int f = 0; f < nfields; f++) {
            RoiBatchField& b = bf[f];
            for (int l = 0; l < b.used; l++) {
                b.plane[l] = bufs.take(batch_plane_bytes(n));
                b.blob[l] = bufs.take(infos[f].len_enc_vec[l]);
                b.work[l] = bufs.take(roi_batch_work_bytes(b.s.nseg[l], b.ids[l].size()));
                if (!b.plane[l] || !b.blob[l] || !b.work[l]) return fail_at("field", f, WR_ERR_HIP);
                if (b.s.brick && !(b.perms[l] = bufs.take(batch_perm_bytes(n, b.s.brick)))) return fail_at("field", f, WR_ERR_HIP);
            }
            if (b.used && b.s.brick && !(b.d_bricks = bufs.take(roi_batch_bricks_bytes(b.bricks.size())))) return fail_at("field", f, WR_ERR_HIP);
            if (b.has_mask()) {  // (the plane at the batch's pitch; the restore's counters are in its table)
                b.mask.bits = bufs.take(roi_batch_mask_plane_bytes(n));
                b.mask.d_blob = bufs.take(b.mask.blob_bytes());
                b.mask.work = bufs.take(b.mask.work_bytes());
                if (!b.mask.bits || !b.mask.d_blob || !b.mask.work) return fail_at("field", f, WR_ERR_HIP);
            }
        }
        if (nall) {
            if (!(d_once = bufs.take(roi_batch_once_bytes(nplain, nstranded)))) return WR_ERR_HIP;
            if (nmask && !(d_restore = bufs.take(roi_batch_restore_bytes((size_t)nroi, (size_t)nfields)))) return WR_ERR_HIP;
            if (int rc = bufs.pin(tables + (nmask ? roi_batch_restore_bytes((size_t)nroi, (size_t)nfields) : 0))) return rc;
            if (int rc = bufs.ev.create(0)) return rc;
            if (nmask) if (int rc = bufs.ev.create(1)) return rc;
        }
        if (nall && !fld.dev && !(d_host_out = bufs.take((size_t)nfields * T * elem))) return WR_ERR_HIP;
    }
    // ---- stage "up": only the listed segments' bytes
    size_t bytes_up = 0, segments = 0, mask_bytes_up = 0, mask_segments = 0;
    for (int f = 0; f < nfields; f++) {
        RoiBatchField& b = bf[f];
        if (b.used) {
            if (int rc = seg_upload_lists(c, b.s, b.used, data_encs[f], b.blob, b.work, b.d_bricks, b.ids, b.bricks, &local.h2d_ms, &bytes_up)) return fail_at("field", f, rc);
            for (int l = 0; l < b.used; l++) segments += b.ids[l].size();
        }
        if (b.has_mask()) {
            if (int rc = b.mask.upload(c, &local.h2d_ms, &mask_bytes_up)) return fail_at("field", f, rc);
            mask_segments += b.mask.ids.size();
        }
    }
    g_stat[WR_STAT_ROI_BYTES_UP] += bytes_up;
    if (nmask) g_stat[WR_STAT_MASK_ROI_BYTES_UP] += mask_bytes_up;
    const double t_coded = now();
    SlotLease slot;
    if (njobs)
        if (int rc = slot.acquire(c, need)) return rc;
    const double t_phase = now();
    uint8_t* const d_out = fld.dev ? reinterpret_cast<uint8_t*>(fld.dev) : d_host_out;
    int rc = WR_OK;
    std::vector<unsigned long long> restored((size_t)nfields, 0);  // (the masked call) per field the set bits among its regions
    if (nall) {
        StageLock cu(pool->cu_mu);
        if (njobs) clock_warmup(c, need.field_elems);
        // the jobs' failure counts lie behind the tables, in the order of the fields, a field's planes and then its mask
        unsigned int* const d_bad = reinterpret_cast<unsigned int*>(d_once + tables);
        HIPCHK(hipMemsetAsync(d_bad, 0, 4 * nall, c->stream));
        ListJobs jobs;
        int at = 0;
        for (int f = 0; f < nfields; f++) {
            RoiBatchField& b = bf[f];
            b.job0 = at;
            for (int l = 0; l < b.used; l++, at++) {
                wrk::SegJob job = seg_job(wrk::plane_ref(b.s.brick ? b.perms[l] : b.plane[l]), b.blob[l], infos[f].len_enc_vec[l], b.work[l], n, b.s.seg[l], b.s.nseg[l], b.s.brick);
                job.bad = d_bad + at;  // (the batch counts in one array, read back once)
                jobs.add(job, wrk::seg_decode_list_ids(b.work[l], b.s.nseg[l]), b.ids[l].size(), b.s.strands);
            }
            if (b.has_mask()) {
                wrk::SegJob job = b.mask.seg_job();
                job.bad = d_bad + at++;
                jobs.add(job, b.mask.seg_list());
            }
        }
        launch_note(c, "seg_decode_lists_batch", 0, d_once, n, bufs.pinned, wrk::plane_ref(d_once));
        HIPCHK(hipEventRecord(bufs.ev[0], c->stream));
        const int launches = jobs.launch(bufs.pinned, d_once, c->stream);
        HIPCHK(hipEventRecord(bufs.ev[1], c->stream));
        if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "batched segment decoder launch failed" + launch_describe(c));
        g_stat[WR_STAT_ROI_SEGMENTS] += segments;  // (behind the check: a launch that failed does not count as made)
        g_stat[WR_STAT_ROI_CODER_LAUNCHES] += (unsigned long)launches;
        if (nmask) g_stat[WR_STAT_MASK_ROI_SEGMENTS] += mask_segments;
        // no dequantiser runs unless every listed segment of every field and of every mask decoded: the counts come back once
        std::vector<unsigned int> bad(nall);
        HIPCHK(hipMemcpyAsync(bad.data(), d_bad, 4 * nall, hipMemcpyDeviceToHost, c->stream));
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(WR_ERR_HIP, "the batched segment decoder failed on the device" + launch_describe(c));
        for (int f = 0; f < nfields; f++) {
            for (int l = 0; l < bf[f].used; l++)
                if (const unsigned int k = bad[(size_t)bf[f].job0 + l])
                    return fail(WR_ERR_STREAM, "field " + std::to_string(f) + ": plane " + std::to_string(l) + ": " + bad_segments_text(k));
            if (bf[f].has_mask())
                if (const unsigned int k = bad[(size_t)bf[f].job0 + bf[f].used]) return fail(WR_ERR_STREAM, "field " + std::to_string(f) + ": mask blob: " + bad_segments_text(k));
        }
        fold_coder_seconds(bufs, 1, &local);
        // ---- every field in turn: its bricks back to their places, then its regions through the window stage
        for (int f = 0; f < nfields && rc == WR_OK; f++) {
            const RoiBatchField& b = bf[f];
            if (!b.used) continue;
            for (int l = 0; l < b.used; l++)
                if (b.s.brick && !wrk::plane_reorder(wrk::plane_ref(b.plane[l]), b.perms[l], b.s.od, true, reinterpret_cast<const uint32_t*>(b.d_bricks), b.bricks.size(), c->stream))
                    return fail(WR_ERR_ARG, "field " + std::to_string(f) + ": too many bricks");
            wrk::DequantParams p;
            if ((rc = dequant_params(&infos[f], b.used, n, [&](int l) { return wrk::plane_ref(b.plane[l]); }, &p)) != WR_OK) { rc = fail_at("field", f, rc); break; }
            launch_note(c, "dequant_window", b.used - 1, slot->field, need.field_elems, nullptr, p.q[b.used - 1]);
            rc = roi_multi_from_planes(c, slot.get(), d_out + (size_t)f * T * elem, nx, ny, b.pls, out_at, p, f32, tm ? &local : nullptr);
            if (rc) rc = fail_at("field", f, rc);
        }
        // ---- (the masked call) the constant fields that have a mask, then `fill` into every region of every masked field: one launch
        if (nmask && rc == WR_OK) {
            std::vector<const uint8_t*> planes_of((size_t)nfields, nullptr);
            for (int f = 0; f < nfields; f++) {
                const RoiBatchField& b = bf[f];
                if (!b.has_mask()) continue;
                planes_of[f] = b.mask.bits;
                if (!b.s.constant) continue;
                if (f32) wrk::fill_f32(reinterpret_cast<float*>(d_out) + (size_t)f * T, T, (float)infos[f].midval, c->stream);
                else wrk::fill(reinterpret_cast<double*>(d_out) + (size_t)f * T, T, infos[f].midval, c->stream);
            }
            uint8_t* const host_table = bufs.pinned + tables;
            HIPCHK(hipEventRecord(bufs.ev[2], c->stream));
            const int nfld = f32 ? wrk::mask_restore_boxes(reinterpret_cast<float*>(d_out), mregions.data(), out_at.data(), (size_t)nroi, planes_of.data(), (size_t)nfields, T,
                                                           (float)mb->fill, host_table, d_restore, c->stream)
                                 : wrk::mask_restore_boxes(reinterpret_cast<double*>(d_out), mregions.data(), out_at.data(), (size_t)nroi, planes_of.data(), (size_t)nfields, T,
                                                           mb->fill, host_table, d_restore, c->stream);
            HIPCHK(hipEventRecord(bufs.ev[3], c->stream));
            if (nfld != (int)nmask) rc = fail(WR_ERR_ARG, "too many turns: the restore launch of the call has 2^31 or more");
            else if (hipGetLastError() != hipSuccess) rc = fail(WR_ERR_HIP, "mask restore launch failed");
            else {
                std::vector<unsigned long long> counts(nmask);
                HIPCHK(hipMemcpyAsync(counts.data(), wrk::mask_boxes_counters(d_restore, (size_t)nroi, (size_t)nfields), nmask * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                size_t m = 0;
                for (int f = 0; f < nfields; f++) if (bf[f].has_mask()) restored[f] = counts[m++];
            }
        }
        rc = kernel_stage_end(c, rc);
    }
    if (rc) return rc;
    // constant fields: midval in every region (device callers here, host callers behind the one copy down); those that have
    // a mask were made in the kernel stage
    for (int f = 0; f < nfields; f++)
        if (bf[f].s.constant && fld.dev && !bf[f].has_mask())
            if (int rc2 = fill_constant(c, FieldRef{fld.dev + (size_t)f * T}, T, infos[f].midval)) return rc2;
    if (nall)  // (an all-constant call has nothing to bring down)
        if (int rc2 = finish_call(c, fld, d_host_out, d_host_out, (size_t)nfields * T, false, t0, t_coded, t_phase, &local, nullptr)) return rc2;
    for (int f = 0; f < nfields; f++) {
        if (!bf[f].s.constant || fld.dev || bf[f].has_mask()) continue;
        FieldRef part;
        if (f32) part.host_f32 = fld.host_f32 + (size_t)f * T;
        else part.host = fld.host + (size_t)f * T;
        if (int rc2 = fill_constant(c, part, T, infos[f].midval)) return rc2;
    }
    if (mb && mb->res) {
        const float fill_ms = nmask ? (float)(bufs.ev.seconds(1) * 1e3) : 0;
        for (int f = 0; f < nfields; f++) {
            wr_mask_result& r = mb->res[f];
            memset(&r, 0, sizeof r);
            if (!bf[f].has_mask()) continue;
            r.undefined = restored[f]; r.pad = bf[f].mask.info.pad; r.mask_len = bf[f].mask.len; r.fill_ms = fill_ms;
        }
    }
    local.total = now() - t0;
    if (tm) *tm = local;
    return WR_OK;
}

int decode_seg_roi_batch_masked(wr_ctx* c, FieldRef f, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm,
                                wr_mask_result* res)
{
    if (res && nfields > 0) memset(res, 0, (size_t)nfields * sizeof *res);
    const MaskBatch mb{fill, res};
    return decode_seg_roi_batch_impl(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, tm, &mb);
}

// wr_dev_mask_restore_boxes / _f32: the restore over the boxes alone, as a stage call
template <class T>
int dev_mask_restore_boxes(wr_ctx* c, T* d_out, int nfields, int nx, int ny, int nz, int level, const wr_box* rois, int nroi, const unsigned char* const* d_bits,
                           double fill, unsigned long long* undefined)
{
    if (int rc = ctx_bind(c)) return rc;
    if (!d_out || !d_bits) return fail(WR_ERR_ARG, "null pointer");
    if (nfields < 1) return fail(WR_ERR_ARG, "nfields must be at least 1");
    std::vector<size_t> offs((size_t)(nroi > 0 ? nroi : 0) + 1);
    const size_t T_elems = wr_roi_multi_elems(nx, ny, nz, level, rois, nroi, offs.data());
    if (!T_elems) return WR_ERR_ARG;  // (the message is wr_roi_multi_elems')
    std::vector<wrmask::Region> gs;
    for (int i = 0; i < nroi; i++) gs.push_back(mask_region(nx, ny, nz, level, &rois[i]));
    size_t nmask = 0;
    for (int f = 0; f < nfields; f++) nmask += d_bits[f] != nullptr;
    if (undefined) for (int f = 0; f < nfields; f++) undefined[f] = 0;
    const size_t turns = wrmask::boxes_turns(gs.data(), gs.size(), nullptr);
    if (!turns || (unsigned long long)nmask * turns >= wrmask::kTurnLimit) return fail(WR_ERR_ARG, "too many turns: the restore launch has 2^31 or more");
    if (!nmask) return WR_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    BatchBufs bufs(c);
    const size_t table = wrk::mask_boxes_table_bytes((size_t)nroi, (size_t)nfields);
    uint8_t* const d_table = bufs.take(table);
    if (!d_table) return WR_ERR_HIP;
    if (int rc = bufs.pin(table)) return rc;
    StageLock cu(c->pool->cu_mu);
    if (wrk::mask_restore_boxes(d_out, gs.data(), offs.data(), (size_t)nroi, d_bits, (size_t)nfields, T_elems, (T)fill, bufs.pinned, d_table, c->stream) != (int)nmask)
        return fail(WR_ERR_ARG, "too many turns: the restore launch has 2^31 or more");
    if (hipGetLastError() != hipSuccess) return fail(WR_ERR_HIP, "mask restore launch failed");
    std::vector<unsigned long long> counts(nmask);
    HIPCHK(hipMemcpyAsync(counts.data(), wrk::mask_boxes_counters(d_table, (size_t)nroi, (size_t)nfields), nmask * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (undefined) {
        size_t m = 0;
        for (int f = 0; f < nfields; f++) if (d_bits[f]) undefined[f] = counts[m++];
    }
    return WR_OK;
}

}  // namespace

extern "C" {

int wr_decode_host_seg_roi_batch_masked(wr_ctx* c, double* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                        const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm,
                                        wr_mask_result* res)
{
    FieldRef f; f.host = h_out;
    return decode_seg_roi_batch_masked(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, fill, tm, res);
}

int wr_decode_host_seg_roi_batch_masked_f32(wr_ctx* c, float* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                            const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm,
                                            wr_mask_result* res)
{
    FieldRef f; f.host_f32 = h_out;
    return decode_seg_roi_batch_masked(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, fill, tm, res);
}

int wr_decode_device_seg_roi_batch_masked(wr_ctx* c, double* d_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                          const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm,
                                          wr_mask_result* res)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    return decode_seg_roi_batch_masked(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, fill, tm, res);
}

int wr_dev_mask_restore_boxes(wr_ctx* c, double* d_out, int nfields, int nx, int ny, int nz, int level, const wr_box* rois, int nroi,
                              const unsigned char* const* d_bits, double fill, unsigned long long* undefined)
{
    return dev_mask_restore_boxes(c, d_out, nfields, nx, ny, nz, level, rois, nroi, d_bits, fill, undefined);
}
int wr_dev_mask_restore_boxes_f32(wr_ctx* c, float* d_out, int nfields, int nx, int ny, int nz, int level, const wr_box* rois, int nroi,
                                  const unsigned char* const* d_bits, double fill, unsigned long long* undefined)
{
    return dev_mask_restore_boxes(c, d_out, nfields, nx, ny, nz, level, rois, nroi, d_bits, fill, undefined);
}

size_t wr_seg_roi_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int planes, unsigned seg, unsigned brick, unsigned strands, unsigned mask_seg,
                                            size_t out_elems)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (!mask_seg) mask_seg = WR_SEG_DEFAULT;
    if (nfields < 1 || nmasked < 0 || nmasked > nfields || !n || planes < 0 || planes > WR_NLAYMAX || !wrseg::seg_ok(seg) || !wrseg::seg_ok(mask_seg) ||
        (brick && !wrblk::brick_ok(brick)))
        return 0;
    if (strands && !wrseg::strands_ok(strands, seg)) return 0;
    const size_t N = (size_t)nfields, M = (size_t)nmasked, jobs = N * (size_t)planes;
    if (jobs + M > WR_SEG_BATCH_MAX) return 0;
    if (!M) return wr_seg_roi_batch_device_bytes(nfields, n, planes, seg, brick, strands, out_elems);
    // the plain function's sum, with the masks' jobs in the table of the WRS1 / WRS2 launch
    const size_t nseg = wrseg::seg_count(n, seg);
    const size_t blob = ((strands ? wr_seg_bound_strands(n, seg, strands) : brick ? wr_seg_bound_blocked(n, seg) : wr_seg_bound(n, seg)) + 15) & ~(size_t)15;
    const size_t per_job = batch_plane_bytes(n) + up256(blob) + up256(roi_batch_work_bytes(nseg, nseg)) + batch_perm_bytes(n, brick);
    const size_t per_field = brick && planes ? up256(roi_batch_bricks_bytes(n)) : 0;
    // per masked field: the mask plane at its pitch, the blob at its bound, the offsets, flags and list of all its segments
    const size_t msym = wrmask::mask_bytes(n), mnseg = wrseg::seg_count(msym, mask_seg);
    const size_t per_mask = roi_batch_mask_plane_bytes(n) + up256(wr_mask_bound(n, mask_seg)) + up256(roi_batch_work_bytes(mnseg, mnseg));
    const size_t once = up256(roi_batch_once_bytes((strands ? 0 : jobs) + M, strands ? jobs : 0)) + up256(roi_batch_restore_bytes(WR_ROI_MULTI_MAX, N));
    return jobs * per_job + N * per_field + M * per_mask + once + up256(N * out_elems * sizeof(double));
}

size_t wr_seg_lists_lanes(int njobs, const size_t* nlist, const unsigned* strands, uint32_t* first)
{
    const unsigned long long lanes = wrsb::lists_lanes(njobs, nlist, strands, first);
    if (lanes) return (size_t)lanes;
    if (njobs < 1 || njobs > (int)wrsb::kBatchMax) { fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(wrsb::kBatchMax)); return 0; }
    if (!nlist) { fail(WR_ERR_ARG, "null array"); return 0; }
    unsigned long long any = 0;
    for (int j = 0; j < njobs; j++) {
        if (strands && !wrsb::strands_layout_ok(strands[j])) { fail(WR_ERR_ARG, "job " + std::to_string(j) + ": strands must be 0 or one of 1, 2, 4, 8, 16, 32"); return 0; }
        any |= nlist[j];
    }
    if (any) fail(WR_ERR_ARG, "too many segments: the launch has 2^31 lanes or more");
    return 0;  // (every list empty: no lanes, first[] is all zeros, nothing was refused)
}

size_t wr_seg_roi_batch_device_bytes(int nfields, size_t n, int planes, unsigned seg, unsigned brick, unsigned strands, size_t out_elems)
{
    if (!seg) seg = WR_SEG_DEFAULT;
    if (nfields < 1 || !n || planes < 0 || planes > WR_NLAYMAX || !wrseg::seg_ok(seg) || (brick && !wrblk::brick_ok(brick))) return 0;
    if (strands && !wrseg::strands_ok(strands, seg)) return 0;
    const size_t N = (size_t)nfields, jobs = N * (size_t)planes;
    if (jobs > WR_SEG_BATCH_MAX) return 0;
    const size_t nseg = wrseg::seg_count(n, seg);
    const size_t blob = ((strands ? wr_seg_bound_strands(n, seg, strands) : brick ? wr_seg_bound_blocked(n, seg) : wr_seg_bound(n, seg)) + 15) & ~(size_t)15;
    const size_t per_job = batch_plane_bytes(n) + up256(blob) + up256(roi_batch_work_bytes(nseg, nseg)) + batch_perm_bytes(n, brick);
    const size_t per_field = brick && planes ? up256(roi_batch_bricks_bytes(n)) : 0;  // (a brick holds a sample at least)
    return jobs * per_job + N * per_field + up256(roi_batch_once_bytes(strands ? 0 : jobs, strands ? jobs : 0)) + up256(N * out_elems * sizeof(double));
}

size_t wr_ctx_device_free_bytes(wr_ctx* c)
{
    if (ctx_bind(c)) return 0;
    size_t free_bytes = 0, total = 0;
    if (hipMemGetInfo(&free_bytes, &total) != hipSuccess) { (void)hipGetLastError(); fail(WR_ERR_HIP, "hipMemGetInfo failed"); return 0; }
    return free_bytes;
}

int wr_dev_seg_decode_lists_mixed(wr_ctx* c, int njobs, const unsigned char* const* d_blob, const size_t* blob_len, unsigned char* const* d_sym, const size_t* n,
                                  const uint32_t* const* ids, const size_t* nlist, size_t* bad_segments)
{
    if (njobs < 1 || njobs > WR_SEG_BATCH_MAX) return fail(WR_ERR_ARG, "njobs must be in 1.." + std::to_string(WR_SEG_BATCH_MAX));
    if (int rc = ctx_bind(c)) return rc;
    if (!d_blob || !blob_len || !d_sym || !n || !ids || !nlist) return fail(WR_ERR_ARG, "null array");
    for (int j = 0; j < njobs; j++) {
        const std::string who = "job " + std::to_string(j) + ": ";
        if (!d_blob[j] || (n[j] && !d_sym[j]) || (nlist[j] && !ids[j])) return fail(WR_ERR_ARG, who + "null pointer");
        if (((uintptr_t)d_sym[j] | (uintptr_t)d_blob[j]) & 15) return fail(WR_ERR_ARG, who + "plane and blob buffers must be 16-byte aligned");
        if (bad_segments) bad_segments[j] = 0;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    // every header, index and list is validated on the host before anything is launched for any job
    std::vector<Front> front(njobs);
    size_t nplain = 0, nstranded = 0, any = 0;
    for (int j = 0; j < njobs; j++) {
        const std::string who = "job " + std::to_string(j) + ": ";
        if (int rc = fetch_front(d_blob[j], blob_len[j], n[j], true, nullptr, who, &front[j])) return rc;
        if (nlist[j] > front[j].nseg) return fail(WR_ERR_ARG, who + "the list is longer than the plane has segments");
        for (size_t i = 0; i < nlist[j]; i++)
            if (ids[j][i] >= front[j].nseg || (i && ids[j][i] <= ids[j][i - 1])) return fail(WR_ERR_ARG, who + "the list must be ascending, every id below the segment count");
        (front[j].strands ? nstranded : nplain)++;
        any += nlist[j];
    }
    if (!any) return WR_OK;
    BatchBufs bufs(c);
    ListJobs jobs;
    std::vector<uint8_t*> works(njobs, nullptr);
    for (int j = 0; j < njobs; j++) {
        const Front& f = front[j];
        const uint32_t* d_ids = nullptr;
        if (nlist[j]) {
            uint8_t* const work = works[j] = bufs.take(roi_batch_work_bytes(f.nseg, nlist[j]));
            if (!work) return WR_ERR_HIP;
            if (int rc = seg_upload_offsets(f.bytes.data(), wrseg::header_bytes(f.brick, f.strands), f.nseg, work)) return rc;
            HIPCHK(hipMemcpy(wrk::seg_decode_list_ids(work, f.nseg), ids[j], nlist[j] * sizeof(uint32_t), hipMemcpyHostToDevice));
            d_ids = wrk::seg_decode_list_ids(work, f.nseg);
        }
        jobs.add(seg_job(wrk::plane_ref(d_sym[j]), d_blob[j], blob_len[j], works[j], n[j], f.seg, f.nseg, f.brick), d_ids, nlist[j], f.strands);
    }
    if (!jobs.lanes_ok()) return fail(WR_ERR_ARG, "too many segments: a launch has 2^31 lanes or more");
    const size_t table = roi_batch_tables_bytes(nplain, nstranded);
    uint8_t* const d_table = bufs.take(table);
    if (!d_table) return WR_ERR_HIP;
    if (int rc = bufs.pin(table)) return rc;
    StageLock cu(c->pool->cu_mu);
    for (int j = 0; j < njobs; j++) if (works[j]) HIPCHK(hipMemsetAsync(wrk::seg_work_bad(works[j]), 0, sizeof(unsigned int), c->stream));
    jobs.launch(bufs.pinned, d_table, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<unsigned int> bad(njobs, 0);
    for (int j = 0; j < njobs; j++) if (works[j]) HIPCHK(hipMemcpyAsync(&bad[j], wrk::seg_work_bad(works[j]), sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = WR_OK;
    for (int j = 0; j < njobs; j++) {
        if (bad_segments) bad_segments[j] = bad[j];
        if (bad[j] && !rc) rc = fail(WR_ERR_STREAM, "job " + std::to_string(j) + ": segmented plane: " + bad_segments_text(bad[j]));
    }
    return rc;
}

int wr_decode_host_seg_roi_batch(wr_ctx* c, double* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                 const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    FieldRef f; f.host = h_out;
    return decode_seg_roi_batch_impl(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, tm);
}

int wr_decode_host_seg_roi_batch_f32(wr_ctx* c, float* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                     const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    FieldRef f; f.host_f32 = h_out;
    return decode_seg_roi_batch_impl(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, tm);
}

int wr_decode_device_seg_roi_batch(wr_ctx* c, double* d_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                   const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm)
{
    FieldRef f; f.dev = d_out;
    if (!d_out) return fail(WR_ERR_ARG, "null device output pointer");
    return decode_seg_roi_batch_impl(c, f, nfields, nx, ny, nz, level, max_planes, rois, nroi, infos, data_encs, data_lens, tm);
}

}  // extern "C"
