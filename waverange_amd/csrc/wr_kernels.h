// wr_kernels.h -- launchers for the gfx950 kernels of the WaveRange hot path.
//
// Everything here works on DEVICE pointers and enqueues on the given HIP stream; nothing
// synchronises.  Canonical arithmetic is strict IEEE double without FMA contraction
// (the library is compiled with -ffp-contract=off; see DESIGN.md "Arithmetic").
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wr_blocked.h"

namespace wrk {

// ---- 3-D CDF-9/7 lifting transform (reference src/waveletcdf97_3d/waveletcdf97_3d.c:38-468)
// In place on `fld` (nx*ny*nz doubles, x fastest); `scratch` is a second buffer of the same
// size.  lvl > 0 forward, lvl < 0 inverse, 0 identity.
void transform(double* fld, double* scratch, int nx, int ny, int nz, int lvl, hipStream_t st);
// one level of the above: the box ceil(n / 2^k), in place on `fld`
void transform_level(double* fld, double* scratch, int nx, int ny, int nz, int k, bool inverse, hipStream_t st);

// ---- reductions (reference src/core/wrappers.cpp:244-250, 308-314)
// partial[] needs 2*minmax_partials() doubles; result (min, max) lands in result[0..1] (device).
int minmax_partials();
void minmax(const double* x, size_t n, double* partial, double* result, hipStream_t st);
void minmax(const float* x, size_t n, double* partial, double* result, hipStream_t st);  // of an fp32 field (8-byte aligned)
// sign bit of the LAST element equal to zero (the reference's fmin scan keeps the last of
// equal values): out[0] = index+1 of that element (0 if none).  Rare path (min == 0 only).
void last_zero_index(const double* x, size_t n, unsigned long long* out, hipStream_t st);
void last_zero_index(const float* x, size_t n, unsigned long long* out, hipStream_t st);

// ---- fp32 fields on the paths that do not run the fused kernels (general transform, wtflag = 0): one pass each way.
// dst[i] = (double)src[i] (exact) / dst[i] = (float)src[i] (round to nearest even, as the C cast).  Not in place.
void widen_f32(const float* src, double* dst, size_t n, hipStream_t st);
void narrow_f64(const double* src, float* dst, size_t n, hipStream_t st);

// A quantized plane as the kernels see it: one array, or up to kPlaneChunks chunks of 2^shift bytes each (a large plane
// of a call in flight lives in chunks that come and go as the host coder drains or fills it: wr_pipeline.cpp).  Byte i of
// the plane is chunk[i >> shift][i & (2^shift - 1)]; a chunk is a multiple of 4096 bytes, so the 4096-element groups the
// kernels work in, and their 16-byte loads, never straddle two chunks.
constexpr int kPlaneChunks = 16;
struct PlaneRef {
    uint8_t* chunk[kPlaneChunks];
    unsigned shift;
    __host__ __device__ uint8_t* at(size_t i) const { return chunk[i >> shift] + (i & (((size_t)1 << shift) - 1)); }
};
// every chunk that the bytes [0, n) of the plane fall into is there (host-side check in front of a launch: a kernel handed
// a table with a hole in it would write through a null or stale pointer)
inline bool plane_ref_covers(const PlaneRef& r, size_t n)
{
    if (!n) return true;
    const size_t last = r.shift >= 8 * sizeof(size_t) - 1 ? 0 : (n - 1) >> r.shift;
    if (last >= (size_t)kPlaneChunks) return false;
    for (size_t k = 0; k <= last; k++) if (!r.chunk[k]) return false;
    return true;
}
inline PlaneRef plane_ref(const uint8_t* base)  // a plane that is one array
{
    PlaneRef r;
    for (int k = 0; k < kPlaneChunks; k++) r.chunk[k] = const_cast<uint8_t*>(base);
    r.shift = 63;
    return r;
}

// ---- quantizer plane (wrappers.cpp:339-340, 384-398) fused with the min/max of the residual
// q[j] = (uchar)(aopt*x[j] + bopt); if write_resid: x[j] -= q[j]*deps + minval and
// result[0..1] = min/max of the new residual.
void quantize_plane(double* x, size_t n, double aopt, double bopt, double deps, double minval,
                    const PlaneRef& q, bool write_resid, double* partial, double* result, hipStream_t st);

// ---- the same plane without a residual array (k_quant_blk): x holds the COEFFICIENTS and stays as it is; the residual this
// plane is cut from is recomputed from them and the scalars of the planes before (prev, in order); want_minmax: result[0..1]
// = min/max of the residual after this plane; write_resid: x := that residual (the last plane of a caller who wants it);
// hist != nullptr: the per-60000-symbol-block byte histograms of the plane (block_histograms' output) are written too.
// quantize_plane_blk_ok: the pointers are 16-byte aligned (and WR_QUANT_INPLACE is not set).
constexpr int kQuantPrevMax = 7;
struct QuantPrev {
    int n = 0;
    double aopt[kQuantPrevMax], bopt[kQuantPrevMax], deps[kQuantPrevMax], minval[kQuantPrevMax];
    void push(double a, double b, double d, double m) { aopt[n] = a; bopt[n] = b; deps[n] = d; minval[n] = m; n++; }
};
bool quantize_plane_blk_ok(const double* x, const PlaneRef& q);
void quantize_plane_blk(double* x, size_t n, const QuantPrev& prev, double aopt, double bopt, double deps, double minval, const PlaneRef& q,
                        bool write_resid, bool want_minmax, uint16_t* hist, double* partial, double* result, hipStream_t st);
// x := the residual after the planes in prev
void residual_apply(double* x, size_t n, const QuantPrev& prev, hipStream_t st);

// ---- the size probe of an encode to a byte budget (k_quant_probe; the bound and its table: wr_budget.h).  x holds the
// COEFFICIENTS (16-byte aligned, read only); the plane in question is cut from the residual after the planes in prev.  For
// each of the cd.n <= kProbeK candidate steps (aopt, bopt) totals[k] becomes the sum over the plane's segments of the bound
// of the segment stream that step would give (the blob's header and index are not in it).  Nothing else is written.
// want_minmax: result[0..1] = min/max of the residual that candidate 0 (step cd.deps0, offset cd.minval0) would leave.
// tab: wrbud::kTabWords words of device memory, the host's table; fixed: its Tables::fixed.  totals: kProbeK words of
// device memory, zeroed here.  seg: wrseg::seg_ok.
constexpr int kProbeK = 8;
struct ProbeCands {
    int n = 0;
    double aopt[kProbeK], bopt[kProbeK];
    double deps0 = 0, minval0 = 0;
};
void quant_probe(const double* x, size_t n, unsigned seg, const QuantPrev& prev, const ProbeCands& cd, bool want_minmax, const uint32_t* tab,
                 unsigned long long fixed, unsigned long long* totals, double* partial, double* result, hipStream_t st);
// the same sum for a plane of symbols that exists (16-byte aligned, one array): totals[0]
void plane_bound(const uint8_t* sym, size_t n, unsigned seg, const uint32_t* tab, unsigned long long fixed, unsigned long long* totals, hipStream_t st);

// ---- the trial of an encode to an error bound (k_requant_accum).  x holds the COEFFICIENTS (read only); acc[j] becomes what
// dequant_accum gives from the planes quantize_plane_blk would write for the full planes in prev, in order, and then a last
// plane cut with (aopt, bopt, deps, minval), bit for bit.  No plane is written.  acc must not overlap x.  Both pointers
// 16-byte aligned: 16-byte loads and stores; otherwise an element-wise form of the same arithmetic.
void requant_accum(const double* x, size_t n, const QuantPrev& prev, double aopt, double bopt, double deps, double minval, double* acc, hipStream_t st);
// ---- its compare: result[0] = max |a[j] - b[j]| over the differences that are finite (both operands widened to fp64, one
// subtraction each; 0 if there is none), result[1] = the count of those that are not.  partial: 2 * minmax_partials() doubles.
void linf_count(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st);
void linf_count(const float* a, const float* b, size_t n, double* partial, double* result, hipStream_t st);
// ---- the compare of an encode to an RMS or PSNR target (k_err_stats): result[0], result[1] as linf_count gives them, and
// result[2] = S, the fp64 sum of fl(d * d) over the finite differences d = fl(a[j] - b[j]) in a summation order that n and the
// alignment of the pointers fix: the same bits on every run, within 2^-38 S* of the real sum of those squares for n <= 2^33
// (the derivation is next to the kernel).  +inf when a square overflows.  partial: 3 * minmax_partials() doubles.
void err_stats(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st);
void err_stats(const float* a, const float* b, size_t n, double* partial, double* result, hipStream_t st);

// ---- quantizer plane with the non-uniform (local) cutoff mask (wrappers.cpp:343-379, 397-398):
// loops over PHYSICAL positions, maps each to its wavelet-space index (ind_p2w_3d,
// waveletcdf97_3d.c:473-553) and quantizes there; coefficients of the finest level whose plane
// range is below the local precision are zeroed.  Residual update and its min/max are fused.
struct LocalCutoff {
    int nx, ny, nz, wlev;
    int mx, my, mz;
    const double* cutoff;  // device array, mx*my*mz entries
    double tol_scale;      // tolabs / tolrel
    double tolabs, span;   // span = maxval - minval of the plane
};
void quantize_plane_local(double* x, size_t n, double aopt, double bopt, double deps, double minval,
                          uint8_t* q, const LocalCutoff& lc, double* partial, double* result, hipStream_t st);

// ---- decoder accumulation (wrappers.cpp:480, 513-514): acc = 0; acc += q_l*deps_l + min_l, l in order
struct DequantParams {
    PlaneRef q[8];
    double deps[8];
    double minval[8];
    int nlay;
};
void dequant_accum(double* acc, size_t n, const DequantParams& p, hipStream_t st);

// ---- helpers
// result[0] = max|a-b|, result[1] = max|a|  (partial: 2*minmax_partials() doubles)
void linf_diff(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st);
void fill(double* x, size_t n, double v, hipStream_t st);
// synthetic field of waverange_amd/synth.py, planes z0..z1-1, written at out[0..]
void synth_field(double* out, int nx, int ny, int nz, unsigned long long seed, int z0, int z1,
                 hipStream_t st);
// per-60000-symbol-block byte histograms of a plane (feeds the host range coder's model):
// hist[b*256 + v] = count of value v in block b (uint16, block size < 65536)
void block_histograms(const PlaneRef& q, size_t n, uint16_t* hist, hipStream_t st);
// keeps `workgroups` workgroups of 256 lanes on the device for `ms` milliseconds (mode 0: fp64 arithmetic, 1: asleep)
void burn(double ms, int mode, int workgroups, double* sink, hipStream_t st);
// bytes (a multiple of 16, 16-byte aligned pointers) copied by `workgroups` workgroups; src / dst may be pinned host memory
void copy_kernel(void* dst, const void* src, size_t bytes, int workgroups, hipStream_t st);

// ---- segmented plane streams (wr_segcoder.hip; the format and the coder step: wr_segcoder.h).  One lane codes one segment.
// Encode: the plane's blob (header, index, segment streams) lands in blob[0, cap) -- 16-byte aligned -- unless it is longer than
// cap; result_host (pinned, as the device sees it; may be null) and the first two words of `stage` take {the blob's length,
// segments that failed}.  `stage`: seg_stage_bytes(n, seg) of device memory, 256-byte aligned (the uncompacted streams, one
// region of the segment bound per segment, and the scan's arrays).  The symbols' plane is 16-byte aligned.
size_t seg_stage_bytes(size_t n, unsigned seg);
// brick != 0 (here and in the decoders): the blob is a WRS2 blob with that brick edge in its header -- `sym` is then the plane in
// the blocked order (plane_reorder below); the coder does not care.
void seg_encode(const PlaneRef& sym, size_t n, unsigned seg, uint8_t* stage, uint8_t* blob, size_t cap, unsigned long long* result_host,
                hipStream_t st, unsigned brick = 0);
// Decode: `work` is seg_decode_work_bytes(nseg) of device memory, 256-byte aligned: {u32 bad segments} at 0 (zeroed here), at
// 256 the nseg + 1 byte offsets of the segment streams behind the index (u64, put there by the caller from the index it
// has VALIDATED on the host), then a u32 flag per segment (0: decoded).  A lane writes only its segment's symbols.
// The layout is written here and nowhere else: the launchers and every caller that fills `work` or a SegJob go through these.
inline size_t seg_work_flags_at(size_t nseg) { return 256 + ((8 * (nseg + 1) + 255) & ~(size_t)255); }
inline unsigned int* seg_work_bad(uint8_t* work) { return reinterpret_cast<unsigned int*>(work); }
inline unsigned long long* seg_work_offs(uint8_t* work) { return reinterpret_cast<unsigned long long*>(work + 256); }
inline uint32_t* seg_work_flags(uint8_t* work, size_t nseg) { return reinterpret_cast<uint32_t*>(work + seg_work_flags_at(nseg)); }
size_t seg_decode_work_bytes(size_t nseg);
// strands != 0 (here and in seg_decode_list): the blob is a WRS3 blob of that many strands per segment (its brick may be 0);
// `work` is laid out the same, the launch is `strands` times as wide.
void seg_decode(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, hipStream_t st, unsigned brick = 0,
                unsigned strands = 0);
// The same over a subset of the segments: `work` is seg_decode_list_work_bytes(nseg, nlist) bytes laid out as above, followed
// by the nlist segment ids at seg_decode_list_ids(work, nseg) (u32, ascending, every one below nseg, put there by the
// caller).  Lane j of the grid decodes segment ids[j]; only the bytes of those segments' streams are read from the blob,
// only their symbols are written, flags[] is set for them alone.
size_t seg_decode_list_work_bytes(size_t nseg, size_t nlist);
uint32_t* seg_decode_list_ids(uint8_t* work, size_t nseg);
void seg_decode_list(const uint8_t* blob, size_t blob_len, const PlaneRef& sym, size_t n, unsigned seg, uint8_t* work, size_t nlist, hipStream_t st,
                     unsigned brick = 0, unsigned strands = 0);
// Stranded segments ("WRS3"): seg_encode with `strands` lanes per segment.  `stage`: strand_stage_bytes(n, seg, strands) bytes,
// 256-byte aligned (a region of the record's bound per segment, the lengths and the scan's arrays).  brick goes into the header
// as it is (0: `sym` is in natural order).
size_t strand_stage_bytes(size_t n, unsigned seg, unsigned strands);
void strand_encode(const PlaneRef& sym, size_t n, unsigned seg, unsigned strands, unsigned brick, uint8_t* stage, uint8_t* blob, size_t cap,
                   unsigned long long* result_host, hipStream_t st);

// ---- the segment coder over the planes of a batch of fields (wr_segbatch.hip): one launch sequence codes `njobs` planes, one
// lane per segment of any of them (the locator: wr_segbatch.h).  A job is one (field, plane); every blob is byte for byte what
// seg_encode / the single-plane decoder make of that plane alone.
struct SegJob {
    PlaneRef sym;               // the plane's symbols (the blocked order for a WRS2 blob), 16-byte aligned
    unsigned long long n;       // symbols of the plane
    uint8_t* blob;              // encode: where the blob lands (16-byte aligned); decode: the blob
    unsigned long long cap;     // encode: the room at blob; decode: the blob's length
    unsigned long long* offs;   // nseg + 1 byte offsets of the segment streams behind the index (encode: set by seg_encode_batch)
    uint32_t* flags;            // decode: a flag per segment (0: decoded)
    unsigned int* bad;          // decode: the job's count of segments that did not decode (zeroed by the caller)
    uint32_t seg, nseg, brick;  // brick != 0: a WRS2 blob with that brick edge in its header (a WRS3 blob: the edge, or 0)
    uint32_t strands;           // 0: a WRS1 / WRS2 job; K: a WRS3 job of K strands per segment (the strand launchers below)
};
// The table of a launch sequence as it lies in device memory: the jobs, then first[njobs + 1], each 256-byte aligned.
size_t seg_batch_table_bytes(size_t njobs);
// host_table := the table of jobs[0, njobs); returns the segments of the launch (the caller keeps them below 2^31)
size_t seg_batch_table_fill(uint8_t* host_table, const SegJob* jobs, size_t njobs);
// Encode: all jobs share n and seg.  `stage`: seg_batch_stage_bytes(njobs, n, seg) of device memory, 256-byte aligned: the table,
// {length, failed segments} per job (u64 pairs, at seg_batch_results(stage, njobs)), every job's offs and lens, and one region
// of the segment bound per segment of the launch.  jobs[j].offs is set here; host_table (seg_batch_table_bytes(njobs) bytes of
// host memory) is filled and copied up, and has to stay alive until the stream has drained.  result_host: njobs u64 pairs of
// pinned memory as the device sees it, written like the pairs in `stage`.
size_t seg_batch_stage_bytes(size_t njobs, size_t n, unsigned seg);
unsigned long long* seg_batch_results(uint8_t* stage, size_t njobs);
void seg_encode_batch(SegJob* jobs, size_t njobs, size_t n, unsigned seg, uint8_t* host_table, uint8_t* stage, unsigned long long* result_host,
                      hipStream_t st);
// Decode: jobs may differ in n, seg and brick.  `table`: seg_batch_table_bytes(njobs) of device memory, 256-byte aligned;
// host_table as above.  Every job's offs come from an index the caller has VALIDATED on the host.
void seg_decode_batch(const SegJob* jobs, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st);
// The same over a subset of every job's segments (k_seg_decode_list_batch): job j decodes the segments lists[j].ids[0, nlist)
// -- u32 in DEVICE memory, ascending, every one below the job's nseg, put there by the caller -- and nothing else of its blob
// is read, nothing else of its plane written, flags[] set for those segments alone.  A lane per listed segment of any job; a
// job with nlist == 0 owns none.  `table`: seg_lists_table_bytes(njobs) of device memory, 256-byte aligned (the table of
// seg_decode_batch with first[] the prefix of the list lengths, then the lists' records); host_table: as many bytes of host
// memory, alive until the stream has drained.  Every job's `bad` is zeroed by the caller.  Returns the lanes of the launch
// (the caller keeps them below 2^31); 0: nothing was launched.
struct SegList {
    const uint32_t* ids;
    uint32_t nlist;
    uint32_t pad;
};
size_t seg_lists_table_bytes(size_t njobs);
size_t seg_decode_lists(const SegJob* jobs, const SegList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st);
// The same for WRS3 blobs (k_strand_decode_list_batch): job j decodes its listed segments with K lanes each, as
// k_strand_decode<true> launched for the job alone would.  The record stands next to SegList; SegJob is as above (its brick is
// not looked at: the header of a WRS3 blob has one length).  first[] is the prefix of the jobs' lanes, each job's rounded up to
// a whole wave (wrsb::lists_lanes in wr_segbatch.h).  `table`: strand_lists_table_bytes(njobs) of device memory, 256-byte
// aligned; host_table as above.  Returns the lanes of the launch (a multiple of 64; the caller keeps them below 2^31).
struct StrandList {
    const uint32_t* ids;
    uint32_t nlist;
    uint32_t K, kshift, L;  // strands per segment, log2(K), strand_len(seg, K)
    uint32_t pad[2];
};
size_t strand_lists_table_bytes(size_t njobs);
size_t strand_decode_lists(const SegJob* jobs, const StrandList* lists, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st);
// Stranded (WRS3) jobs through whole-plane launches.  Encode (k_strand_encode_batch, k_seg_scan_batch, k_strand_gather_batch):
// seg_encode_batch with `strands` lanes per segment; all jobs share n, seg and strands, jobs[j].strands is set here and
// jobs[j].brick goes into the header as it is.  `stage`: strand_batch_stage_bytes(njobs, n, seg, strands) of device memory laid
// out as seg_encode_batch's, with tlens and slens behind lens and one region of the record's staging stride (kModelBound +
// strands * strand_bound(L)) per segment of the launch.  Every blob is byte for byte strand_encode's.
size_t strand_batch_stage_bytes(size_t njobs, size_t n, unsigned seg, unsigned strands);
void strand_encode_batch(SegJob* jobs, size_t njobs, size_t n, unsigned seg, unsigned strands, uint8_t* host_table, uint8_t* stage,
                         unsigned long long* result_host, hipStream_t st);
// Decode (k_strand_decode_batch): every job has strands != 0; they may differ in n, seg, strands and brick.  first[] is the
// prefix of wrsb::job_lanes(nseg_j, strands_j): a job's lanes rounded up to whole waves.  `table`, host_table: as
// seg_decode_batch's.  Returns the lanes of the launch (a multiple of 64; the caller keeps them below 2^31).
size_t strand_decode_batch(const SegJob* jobs, size_t njobs, uint8_t* host_table, uint8_t* table, hipStream_t st);

// ---- the blocked symbol order of WRS2 (wr_blocked.hip; the order itself and its host geometry: wr_blocked.h).  `nat` is the
// plane in natural order, `blk` the same n bytes in the blocked order, one array.  Forward: blk := nat permuted; inverse:
// nat := blk permuted back.  ids == nullptr: the whole plane.  Otherwise ids[0, nlist) are ascending brick ids in device
// memory (every one below od.nbricks: the host made the list) and the grid is the list: nothing outside those bricks is read
// or written.  The box table travels in the kernel's arguments.
constexpr int kReorderBoxes = 29;  // as kWindowBoxes
struct ReorderBox {
    uint32_t ox, oy, oz, ex, ey, ez;
    uint32_t first;  // the first work item of the box
    uint32_t wide;   // 16-byte accesses on both sides
    unsigned long long start;
};
struct ReorderMap {
    int nbox;
    uint32_t nx, ny, brick, group, items;  // group: bricks along x per work item
    ReorderBox box[kReorderBoxes];
};
// Bricks along x per work item: a row of the group is 128 bytes of the natural plane; with a list an item is one brick.
inline uint32_t reorder_group(uint32_t B, bool list) { return list || B >= 128 ? 1 : 128 / B; }
inline uint64_t reorder_box_items(const wrblk::Box& b, uint32_t group) { return (uint64_t)((b.t[0] + group - 1) / group) * b.t[1] * b.t[2]; }
// Whether k_plane_reorder moves box b of the order 16 bytes per lane or byte by byte: B >= 16, and the box's origin and extent in
// x, nx and the box's start in the stream are multiples of 16 (then every brick offset is one too).  `aligned`: both arrays
// are 16-byte aligned and every plane chunk a multiple of 4096 bytes long, which the library's own planes always are.  Host
// only; plane_reorder and wr_reorder_plan both decide here.
inline bool reorder_box_wide(bool aligned, const wrblk::Order& od, const wrblk::Box& b)
{
    return aligned && od.B >= 16 && od.nx % 16 == 0 && b.o[0] % 16 == 0 && b.e[0] % 16 == 0 && b.start % 16 == 0;
}
// false: the plane has more work items than a grid has blocks, nothing was launched.
bool plane_reorder(const PlaneRef& nat, uint8_t* blk, const wrblk::Order& od, bool inverse, const uint32_t* ids, size_t nlist, hipStream_t st);

// ---- low-resolution decode (wr_lowres.hip): the corner box [0,bx) x [0,by) x [0,bz) of the coefficient array, gathered out
// of the planes.  box[(z*by + y)*bx + x] = sum over the planes, in order, of q_l[(y + ny*z)*nx + x] * deps_l + minval_l (the
// arithmetic of dequant_accum).  Nothing of a plane outside those by*bz runs of bx bytes is read.
void dequant_box(double* box, int bx, int by, int bz, int nx, int ny, const DequantParams& p, hipStream_t st);
// dst[i] = src[i] * s (one multiply, one rounding), narrowed to fp32 as the C cast in the second form.  The fp64 form may run
// in place; 16-byte aligned src, 8-byte aligned dst.
void scale_f64(const double* src, double* dst, size_t n, double s, hipStream_t st);
void scale_narrow_f64(const double* src, float* dst, size_t n, double s, hipStream_t st);

// ---- region decode (wr_roi.hip): the coefficient array of a window (wr_roi.h), wx*wy*wz doubles in the Mallat layout of its
// own extents, gathered out of the planes.  Box b of the map copies lx*ly*lz coefficients: win[((oz + z)*wy + oy + y)*wx + ox
// + x] = sum over the planes, in order, of q_l[(sy + y + ny*(sz + z))*nx + sx + x] * deps_l + minval_l (the arithmetic of
// dequant_accum); nx, ny are the extents of the field.  The boxes tile the window; nothing of a plane outside their x-runs is
// read.  The map travels in the kernel's arguments.
constexpr int kWindowBoxes = 29;  // the low-pass box and seven detail octants of each of four levels
struct WindowBox { uint32_t sx, sy, sz, ox, oy, oz, lx, ly, lz; };
struct WindowMap {
    int nbox;
    uint32_t wx, wy, nx, ny;
    WindowBox box[kWindowBoxes];
};
void dequant_window(double* win, const WindowMap& m, const DequantParams& p, hipStream_t st);
// Whether k_dequant_window gathers box x of the map 4 symbols at a time (one 4-byte load per plane, two 16-byte stores) or
// byte by byte: a run's offsets in the plane and in the window and its length must be multiples of 4.  `aligned`: the window
// array is 16-byte aligned and every plane chunk 4-byte aligned and a multiple of 4096 bytes long, which the library's own
// slots and planes always are.  Host only; dequant_window and wr_roi_plan both decide here.
inline bool window_box_wide(bool aligned, const WindowMap& m, const WindowBox& x)
{
    return aligned && m.nx % 4 == 0 && m.wx % 4 == 0 && x.sx % 4 == 0 && x.ox % 4 == 0 && x.lx % 4 == 0;
}
// out[(z*cy + y)*cx + x] = win[((z + oz)*wy + y + oy)*wx + x + ox] * s (one multiply, one rounding; s == 1: the bits as they
// are), narrowed to fp32 as the C cast in the second form.  Not in place.
struct CropBox { uint32_t wx, wy, ox, oy, oz, cx, cy, cz; };
void crop_scale_f64(const double* win, double* out, const CropBox& c, double s, hipStream_t st);
void crop_scale_narrow_f64(const double* win, float* out, const CropBox& c, double s, hipStream_t st);

}  // namespace wrk

namespace wrk {
// ---- fused single-pass-per-level transform (wr_fused.hip).  The finest levels whose boxes are even
// in all three directions (and, for the inverse, whose x extent is a multiple of 4) run fused, the
// remaining coarser levels on the general kernels: fused_levels().  A 1024^3 field runs all four
// levels fused, 1000^3 three forward / two inverse, 500^3 two / one.
// Out of place: the result lands in `dst`; `src` is CONSUMED (the general levels use the forward's
// input array as scratch, the inverse rewrites the coarse corner of its coefficient array);
// `lowbuf` holds the compact low-pass boxes between fused levels (fused_lowbuf_elems() doubles).
int fused_levels(int nx, int ny, int nz, bool inverse);
bool fused_ok(int nx, int ny, int nz, int lvl);
size_t fused_lowbuf_elems(int nx, int ny, int nz);
// Launch geometry of one fused level: tiles in x and y (gridDim.x = tiles_x * tiles_y), z-pairs per segment, z segments
// (gridDim.y) and the z-pairs of the last segment.  fused_plan() fills levels[0 .. return value) (room for 4), finest level
// first, from the function the launches take their grids from; host only.
struct FusedGrid { int tiles_x, tiles_y, zps, zsegs, zlast; };
FusedGrid fused_grid(int n1, int n2, int n3, bool inverse);
int fused_plan(int nx, int ny, int nz, bool inverse, FusedGrid* levels);
// one-time set-up of the fused kernels (their dynamic LDS limit); nullptr, or why they cannot run on this device
const char* fused_prepare();
// mm_partial (fused_minmax_records() x 4 doubles, device) and mm_result (4 doubles, device): when given -- and all
// four levels run fused -- the forward kernels also reduce min/max of the field read and of the coefficient array
// written; mm_result = {field min, field max, coefficient min, coefficient max} (NaNs skipped, the sign of a zero
// minimum is not defined here: see read_minmax in wr_pipeline.cpp).
size_t fused_minmax_records(int nx, int ny, int nz);
void transform_fwd_fused(double* src, double* dst, double* lowbuf, int nx, int ny, int nz, hipStream_t st,
                         double* mm_partial = nullptr, double* mm_result = nullptr);
void transform_inv_fused(double* src, double* dst, double* lowbuf, int nx, int ny, int nz, hipStream_t st);
// The same with an fp32 field: level 0 reads (forward) / writes (inverse) 4 bytes per sample and widens / narrows in the
// kernel (k_fwd_fused_f32, k_inv_fused_f32); every other level and all arithmetic are those of the fp64 path, so the
// coefficients are bit for bit those of the widened field and the reconstruction is (float) of the fp64 one.  src / dst
// are 8-byte aligned.  `scratch` (n doubles) takes the general levels' ping-pong traffic that the fp64 forms put into
// their fp64 src / dst; it may be the memory the fp32 src (forward) or dst (inverse) lies in.
void transform_fwd_fused_f32(const float* src, double* scratch, double* dst, double* lowbuf, int nx, int ny, int nz, hipStream_t st,
                             double* mm_partial = nullptr, double* mm_result = nullptr);
void transform_inv_fused_f32(double* src, float* dst, double* scratch, double* lowbuf, int nx, int ny, int nz, hipStream_t st);
}  // namespace wrk
