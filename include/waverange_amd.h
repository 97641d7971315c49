/*
 * waverange_amd.h -- C ABI of libwaverange_amd.so: the MI355X (gfx950) implementation of
 * WaveRange's encode/decode hot path (3-D CDF-9/7 transform + bit-plane quantizer on the
 * GPU, rngcod13 range coder on the host).
 *
 * Part 1 are the drop-in entry points: the SAME unmangled symbols, argument order and
 * meaning as the reference's libwaverange (src/core/wrappers.h:53,70,75,95,111,119).  The
 * reference declares the scalar outputs as C++ references; at the SysV ABI level a
 * reference is a pointer, so the declarations below are call-compatible with code compiled
 * against the reference header.
 *
 * Part 2 is the device-resident API used by the tests, bench.py and multi-field callers:
 * plain pointers and sizes only, HIP stream handles passed as void*.
 *
 * Error convention: Part 1 keeps the reference's "void + fatal" behaviour (a message on
 * stderr and abort(); the reference throws through the extern "C" frame, wrappers.cpp:425,
 * or exit(1)s, :170).  Part 2 functions return 0 on success and a negative code on error;
 * wr_last_error() returns the message.  There is NO CPU fallback: without a usable GPU
 * every compute entry point fails loudly.
 */
#ifndef WAVERANGE_AMD_H
#define WAVERANGE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Everything declared here -- and nothing else -- is exported by libwaverange_amd.so (built with -fvisibility=hidden):
 * the 24 symbols of the reference's libwaverange.so plus the wr_* functions. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ----------------------------------------------------------------------------------- */
/* Part 1: libwaverange drop-in symbols                                                 */
/* ----------------------------------------------------------------------------------- */

/* replaces setup_wr, reference src/core/wrappers.cpp:531-541 (wrappers.h:75) */
void setup_wr(int nx, int ny, int nz, unsigned char *nlaymax, unsigned long *ntot_enc_max);

/* replaces encoding_wrap, reference src/core/wrappers.cpp:228-452 (wrappers.h:53).
 * Writes the reference's stream unless wr_set_stream_format / WR_STREAM_FORMAT (Part 2) select a segmented format.
 * fld_1d: host double[nx*ny*nz], x fastest.  data_enc: host buffer of ntot_enc_max bytes.
 * mx*my*mz > 1 selects the reference's non-uniform (local) cutoff branch, wrappers.cpp:343-379.
 * As in the reference (wrappers.cpp:397-398, README.md:197) fld_1d is overwritten with the residual
 * in wavelet space; WR_WRITEBACK_RESIDUAL=0 or wr_set_writeback_residual(0) skips that download.
 * Thread safety: like the reference, encoding_wrap / decoding_wrap / waveletcdf97_3d may be called
 * concurrently from several threads on distinct buffers (every call borrows its own context). */
void encoding_wrap(int nx, int ny, int nz, double *fld_1d, int wtflag, int mx, int my, int mz,
                   double *cutoffvec, double *tolabs, double *midval, double *halfspanval,
                   unsigned char *wlev, unsigned char *nlay, unsigned long *ntot_enc,
                   double *deps_vec, double *minval_vec, unsigned long *len_enc_vec,
                   unsigned char *data_enc);

/* replaces decoding_wrap, reference src/core/wrappers.cpp:456-527 (wrappers.h:70) */
void decoding_wrap(int nx, int ny, int nz, double *fld_1d, double *tolabs, double *midval,
                   double *halfspanval, unsigned char *wlev, unsigned char *nlay,
                   unsigned long *ntot_enc, double *deps_vec, double *minval_vec,
                   unsigned long *len_enc_vec, unsigned char *data_enc);

/* Fortran shims, reference src/core/wrappers.cpp:545-594 (wrappers.h:95,111,119) */
void setup_wr_f(int *nx, int *ny, int *nz, int *nlaymax, long *ntot_enc_max);
void encoding_wrap_f(int *nx, int *ny, int *nz, double *fld, int *wtflag, double *tolrel,
                     double *tolabs, double *midval, double *halfspanval, unsigned char *wlev,
                     unsigned char *nlay, long *ntot_enc, double *deps_vec, double *minval_vec,
                     long *len_enc_vec, unsigned char *data_enc);
void decoding_wrap_f(int *nx, int *ny, int *nz, double *fld, double *midval, double *halfspanval,
                     unsigned char *wlev, unsigned char *nlay, long *ntot_enc, double *deps_vec,
                     double *minval_vec, long *len_enc_vec, unsigned char *data_enc);

/* replaces waveletcdf97_3d, reference src/waveletcdf97_3d/waveletcdf97_3d.c:38 (exported by
 * the reference's .so; host buffer, in place; lvl>0 forward, lvl<0 inverse) */
void waveletcdf97_3d(int n1, int n2, int n3, int lvl, double *x);

/* Part 1b: the other symbols the reference's .so exports (host-only integer code) */
/* rangecoder state, layout of reference src/rangecod/rangecod.h:110-131 */
typedef struct {
    unsigned int low, range, help;
    unsigned char buffer;
    unsigned int bytecount;
    unsigned char *databuf;
    unsigned long datalen, datapos;
} rangecoder;
extern char coderversion[];
/* replace the rngcod13 primitives of reference src/rangecod/rangecod.c:170-404 */
void start_encoding(rangecoder *rc, char c, unsigned long initlength);
void encode_freq(rangecoder *rc, unsigned int sy_f, unsigned int lt_f, unsigned int tot_f);
void encode_shift(rangecoder *rc, unsigned int sy_f, unsigned int lt_f, unsigned int shift);
unsigned int done_encoding(rangecoder *rc);
int start_decoding(rangecoder *rc);
unsigned int decode_culfreq(rangecoder *rc, unsigned int tot_f);
unsigned int decode_culshift(rangecoder *rc, unsigned int shift);
void decode_update(rangecoder *rc, unsigned int sy_f, unsigned int lt_f, unsigned int tot_f);
unsigned char decode_byte(rangecoder *rc);
unsigned short decode_short(rangecoder *rc);
void done_decoding(rangecoder *rc);
void init_databuf(rangecoder *rc, unsigned long maxlen);
void free_databuf(rangecoder *rc);
void countblock(int *buffer, unsigned int length, unsigned int *counters);
void readcounts(rangecoder *rc, unsigned int *counters);
/* replaces ind_p2w_3d, reference src/waveletcdf97_3d/waveletcdf97_3d.c:473-553 */
void ind_p2w_3d(int lvlin, int n1, int n2, int n3, int i1in, int i2in, int i3in, int *lvl, int *i1,
                int *i2, int *i3);

/* ----------------------------------------------------------------------------------- */
/* Part 2: device-resident API                                                          */
/* ----------------------------------------------------------------------------------- */

#define WR_NLAYMAX 8 /* reference src/core/defs.h:38 */
#define WR_OK 0
#define WR_ERR_ARG (-1)
#define WR_ERR_HIP (-2)
#define WR_ERR_UNSUPPORTED (-3)
#define WR_ERR_STREAM (-4)
#define WR_ERR_OVERFLOW (-5)
#define WR_ERR_BUDGET (-6) /* an encode to a byte budget: no tolerance of the grid fits the budget */
#define WR_ERR_BOUND (-7)  /* an encode to an error bound: the finest tolerance allowed does not meet the bound */

typedef struct wr_ctx wr_ctx;

/* outputs of one encode = the header record of a field (reference .wrh fields) */
typedef struct wr_enc_info {
    double tolabs, midval, halfspanval;
    unsigned char wlev, nlay;
    unsigned long ntot_enc;
    double deps_vec[WR_NLAYMAX];
    double minval_vec[WR_NLAYMAX];
    unsigned long len_enc_vec[WR_NLAYMAX];
} wr_enc_info;

/* per-call stage timings in seconds (host wall clock around the stages) */
typedef struct wr_timings {
    double total;      /* whole call */
    double gpu;        /* the call's device phase: from getting a work-space slot to its last copy (upload,
                          min/max + transform + quantizer or dequant + inverse, downloads) */
    double transfer;   /* host time outside the range coder and the device phase (stream concatenation etc.) */
    double rangecoder; /* host range coder, wall time of the slowest plane thread */
    /* HIP-event durations on the context's stream, milliseconds */
    float transform_ms; /* all launches of the forward or inverse transform */
    float quant_ms;     /* all quantizer-plane (or the dequantise-accumulate) launches */
    float minmax_ms;    /* stand-alone min/max reductions */
    double wait;        /* waiting for a free work-space slot of the device */
    float h2d_ms;       /* host entry points: upload of the field (encode) / the planes (decode) */
    float d2h_ms;       /* host entry points: sum of the plane downloads (encode) / download of the field
                           (decode); engine timestamps for DMA copies */
    double plane_coder_s[WR_NLAYMAX]; /* host range coder, per plane: from the moment a coder took the plane's stream to its end (a
                           call is as long as its SLOWEST plane stream: `rangecoder` is the maximum of these) */
} wr_timings;

const char *wr_last_error(void);
int wr_device_count(void);
/* 0 = silent, 1 = the reference's progress lines on stdout (default; WR_QUIET=1 silences) */
void wr_set_verbosity(int level);
/* host range-coder threads per encode / decode call (default: one per plane; WR_THREADS=k in the
 * environment sets the default).  With fewer threads than planes a thread codes several planes
 * with interleaved symbol loops: less CPU time per field, more wall time for a single field. */
void wr_set_threads(int nthreads);
/* a different count for the encoder alone (0 = follow wr_set_threads, which also resets this): the
 * encoder interleaves 2 planes as efficiently as 3-4, the decoder is at its best with 4 per thread */
void wr_set_encoder_threads(int nthreads);
/* Process-wide coder pool for callers that keep several fields in flight: nthreads > 0 starts that many worker
 * threads which code the plane streams of ALL concurrent encode / decode calls (wr_set_threads is then
 * ignored); 0 stops it (default: every call runs its own coder threads).  A worker interleaves up to 3 encoder
 * or decoder_streams (1..4, default 4; < 1 keeps the setting) decoder streams in one symbol loop, whichever
 * fields they belong to, so a decoder loop is not limited to the 3-4 planes of one field, and the number of
 * running coder threads never exceeds nthreads.  Same bytes either way. */
void wr_set_coder_pool(int nthreads, int decoder_streams);
/* whether the drop-in encoding_wrap leaves the residual in fld_1d as the reference does (default 1,
 * WR_WRITEBACK_RESIDUAL in the environment): callers that discard the array save a field download */
void wr_set_writeback_residual(int on);
/* Work-space slots of a device (1..4, default 3 or WR_SLOTS): how many device phases may be in
 * flight at once -- one uploading, one in its kernels, one downloading.  A slot holds a staging
 * field, the coefficient array and the low-pass boxes of the transform (2.2 x the field size) and is
 * only populated when concurrent callers need it; if the device runs out of memory the library keeps
 * to the slots it has.  The quantized planes are not in the slot: see wr_ctx_create. */
int wr_set_device_slots(int device, int nslots);
/* process-wide event counters (diagnostics and tests) */
#define WR_STAT_EARLY_DECODES 0   /* decode calls whose planes went to the device window by window under the decoder */
#define WR_STAT_SLOTS_POPULATED 1 /* work-space slots that received device buffers */
#define WR_STAT_DEVICE_PLANE_BYTES 2 /* device memory of quantized planes allocated right now (in use + idle), all devices */
#define WR_STAT_POOL_IDLE_MS 3  /* milliseconds the coder pool's workers have waited for a job, summed over the workers */
#define WR_STAT_POOL_STREAMS_MOVED 4  /* plane streams that changed pool workers between two blocks: an idle worker takes over half
                                        of the streams of the fullest running session */
#define WR_STAT_POOL_QUEUE_MS 5  /* milliseconds plane jobs have waited in the coder pool's queues before a worker took them, summed over jobs */
#define WR_STAT_PLANE_WAIT_MS 6  /* milliseconds calls have waited for device memory for their quantized planes (a decoder also: for its turn
                                    to gather them), summed over calls */
#define WR_STAT_HANDOVER_ERRORS 7  /* window requests of a host coder that were refused: the plane stream they named had moved on to another
                                      call, they came out of order, or two coders were inside one stream (always 0 in a correct run; the
                                      call concerned fails) */
#define WR_STAT_CLOCK_WARMUP_MS 8  /* milliseconds of clock warm-up load put in front of kernel stages (WR_CLOCK_WARMUP_MS, a measurement
                                      hook that is off by default: always 0 then) */
#define WR_STAT_WINDOW_WAIT_MS 10  /* milliseconds host coders have waited inside their window requests for a window's DMA copy (a worker of the
                                    * coder pool is blocked then, not idle), summed over coders */
#define WR_STAT_DECODE_GATE_MS 9   /* milliseconds decode calls have waited for admission to the coder pool, holding no device memory yet
                                      (before: the same time in the pool's queues with their planes allocated), summed over calls */
#define WR_STAT_LOWRES_SEGMENTS 11 /* segments the low-resolution decodes (wr_decode_*_seg_lowres) have launched, summed over planes */
#define WR_STAT_LOWRES_BYTES_UP 12 /* coded payload bytes those calls have copied to the device (the offsets tables are not counted) */
#define WR_STAT_ROI_SEGMENTS 13 /* segments the region decodes (wr_decode_*_seg_roi) have launched, summed over planes */
#define WR_STAT_ROI_BYTES_UP 14 /* coded payload bytes those calls have copied to the device (the offsets tables are not counted) */
#define WR_STAT_ROI_CODER_LAUNCHES 15 /* coder kernel launches of the region decodes: one per used plane of a single-region call and
                                       * of a multi-region call on a WRS3 stream, one per multi-region call on a WRS1 / WRS2 stream */
#define WR_STAT_BUDGET_CODER_RUNS 16 /* planes the encodes to a byte budget (wr_encode_*_seg_budget) have handed to the segment coder:
                                      info->nlay per call, however many tolerances the search looked at */
#define WR_STAT_BOUNDED_CODER_RUNS 17 /* the same for the encodes to an error bound (wr_encode_*_seg_bounded) */
#define WR_STAT_BATCH_CODER_LAUNCHES 18 /* coder kernel launches (k_*_encode_batch, k_*_decode_batch) of the batch calls, whole path
                                          and stage level: one per plane index of an encode and of wr_decode_*_seg_batch, at most two
                                          per wr_decode_*_seg_batch_mixed while neither kind of job exceeds WR_SEG_BATCH_MAX */
#define WR_STAT_QUALITY_CODER_RUNS 19 /* planes the encodes to an RMS / PSNR target (wr_encode_*_seg_quality, any norm) have handed to
                                        the segment coder: info->nlay per call */
#define WR_STAT_MASK_ROI_SEGMENTS 20 /* mask-plane segments the masked region / low-resolution decodes (wr_decode_*_seg_roi_masked) have launched */
#define WR_STAT_MASK_ROI_BYTES_UP 21 /* coded bytes of the mask plane those calls have copied to the device (the offsets tables are not counted) */
unsigned long wr_stat(int what);
/* Hands the idle buffers of the device's plane pool back to the device (the pool keeps the plane memory of finished calls for
 * the next ones: after a burst of concurrent calls that can be most of the HBM).  Buffers in use are not touched. */
int wr_ctx_trim(wr_ctx *c);
/* coder pool, per loop kind {scalar encoder, scalar decoder, 16-lane decoder for dominant-symbol planes, 16-lane encoder}
 * -- WR_POOL_LOOP_KINDS entries each: seconds the workers have spent in block steps of that loop and stream-blocks (60000
 * symbols) advanced: symbols per worker-second in the pipeline */
#define WR_POOL_LOOP_KINDS 4
void wr_pool_loop_stats(double *seconds, double *blocks);

/* One context per concurrent caller: (device, kernel stream, coded-stream buffers, and per plane a ring
 * of two 15 MB pinned chunks), grown on demand and kept.  The device work space (wr_set_device_slots)
 * and the device buffers of the quantized planes are shared between the contexts of a GPU: the planes
 * stay in device memory -- a call borrows one buffer per plane while the plane exists and returns it
 * -- and the host coder reads or writes them through the ring, chunk by chunk, so no whole plane is
 * ever staged in host memory.  stream == NULL makes the context create its own. */
int wr_ctx_create(wr_ctx **ctx, int device, void *hip_stream);
void wr_ctx_destroy(wr_ctx *ctx);
int wr_ctx_sync(wr_ctx *ctx);
/* keep_residual != 0: also apply the residual update on the last plane, so that the device
 * field ends up bit-identical to what the reference leaves in fld_1d (wrappers.cpp:397-398) */
void wr_ctx_set_keep_residual(wr_ctx *ctx, int keep_residual);

/* device memory helpers (thin hipMalloc/hipMemcpy wrappers so callers need no HIP headers) */
int wr_dev_alloc(wr_ctx *ctx, void **ptr, size_t bytes);
int wr_dev_free(wr_ctx *ctx, void *ptr);
int wr_dev_upload(wr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int wr_dev_download(wr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* pinned host memory: field and coded-stream buffers allocated here move over PCIe by DMA without
 * a staging copy (pageable buffers work everywhere too, at roughly half the rate) */
int wr_host_alloc(void **ptr, size_t bytes);
int wr_host_free(void *ptr);
/* Pin a buffer the caller already owns (hipHostRegister): its copies then move by DMA without the runtime's staging
 * copy.  They go through hipMemcpyAsync, not through the library's own SDMA path (the GPU sees registered memory at
 * another address than the host does, which only HIP's copy translates): under many concurrent calls wr_host_alloc'd
 * buffers are the faster choice.  Unregister before freeing the buffer. */
int wr_host_register(void *ptr, size_t bytes);
int wr_host_unregister(void *ptr);

int wr_dev_copy(wr_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes); /* ctx stream, waits */
/* measurement hook: copies through the compute units with `workgroups` workgroups on the context's stream, without
 * waiting (either side may be pinned host memory; 16-byte granularity) */
int wr_dev_copy_kernel(wr_ctx *ctx, void *dst, const void *src, size_t bytes, int workgroups);
/* measurement hook: `workgroups` workgroups stay on the device for `ms` milliseconds on the context's stream, without waiting
 * (mode 0: a chain of fp64 arithmetic, 1: asleep) -- what it takes to bring the shader clock up before a kernel stage */
int wr_dev_burn(wr_ctx *ctx, double ms, int mode, int workgroups);
/* max|a-b| and max|a| over n doubles (accuracy check of a reconstruction, "L-inf vs tol") */
int wr_dev_linf(wr_ctx *ctx, const double *d_a, const double *d_b, size_t n, double *max_abs_diff,
                double *max_abs_a);

/* --- stage-level entry points on device pointers (d_ prefix = device memory, 16-B aligned) */
/* transform in place: a1/a2 of SURVEY.md 8a */
int wr_dev_transform(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int lvl);
/* min/max with the reference's scan semantics incl. the sign of a zero minimum: a4/a5 */
int wr_dev_minmax(wr_ctx *ctx, const double *d_x, size_t n, double *mn, double *mx);
/* one quantizer plane + residual update; next_min/next_max = extrema of the new residual */
int wr_dev_quantize_plane(wr_ctx *ctx, double *d_x, size_t n, double deps, double minval,
                          unsigned char *d_q, double *next_min, double *next_max);
/* acc = sum over planes of (q*deps + minval), planes are nlay device arrays of n bytes */
int wr_dev_dequant_accum(wr_ctx *ctx, double *d_acc, size_t n, int nlay,
                         const unsigned char *const *d_planes, const double *deps,
                         const double *minval);
/* synthetic field generator (waverange_amd/synth.py) straight into device memory */
int wr_dev_synth_field(wr_ctx *ctx, double *d_out, int nx, int ny, int nz,
                       unsigned long long seed);

/* --- device-only part of the codec (no range coder): transform + all quantizer planes.
 * d_fld is CONSUMED: with wr_ctx_set_keep_residual(ctx, 1) it holds the residual in wavelet space afterwards (what the
 * reference leaves in fld_1d, wrappers.cpp:397-398); without, its contents are unspecified (since round 4 the planes are cut
 * from residuals recomputed from the coefficient array, which nobody writes back: the array then holds the coefficients).
 * The same goes for d_fld of wr_encode_device.  d_planes receives nlay planes at a pitch of wr_plane_pitch(n) bytes.
 * Fills tolabs/midval/halfspanval/wlev/nlay/deps/minval. */
size_t wr_plane_pitch(size_t n);
int wr_dev_encode_planes(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag,
                         double tolrel, unsigned char *d_planes, wr_enc_info *info);
int wr_dev_decode_planes(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz,
                         const unsigned char *d_planes, const wr_enc_info *info);

/* --- whole hot path with the field resident in HBM: encode -> host byte stream, and back.
 * data_enc: host buffer of at least setup_wr()'s ntot_enc_max bytes (cap is checked). */
int wr_encode_device(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag,
                     double tolrel, wr_enc_info *info, unsigned char *data_enc, size_t cap,
                     wr_timings *tm);
/* same with the reference's local cutoff vector (mx*my*mz entries, host memory) */
int wr_encode_device_local(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx,
                           int my, int mz, const double *cutoffvec, wr_enc_info *info,
                           unsigned char *data_enc, size_t cap, wr_timings *tm);
/* data_len: bytes readable at data_enc (0 = trust info->ntot_enc, as the reference does) */
int wr_decode_device(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz,
                     const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                     wr_timings *tm);

/* --- whole hot path host buffer to host buffer: what encoding_wrap / decoding_wrap run on, with an
 * explicit context (one per concurrent caller), error codes and timings.  The field is staged through
 * the device's work-space slot: upload on the device's upload stream, kernels, planes / field back on
 * the download stream, so that concurrent calls overlap their copies with one another's kernels and
 * host range coding.  h_fld may be pinned (wr_host_alloc) or pageable.  Encode leaves h_fld untouched
 * unless wr_ctx_set_keep_residual(ctx, 1) asks for the reference's residual write-back. */
int wr_encode_host(wr_ctx *ctx, double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                   int mz, const double *cutoffvec, wr_enc_info *info, unsigned char *data_enc,
                   size_t cap, wr_timings *tm);
int wr_decode_host(wr_ctx *ctx, double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                   const unsigned char *data_enc, size_t data_len, wr_timings *tm);
/* Decode in two calls, for callers that want to bound their output buffers: the host range decoding takes seconds
 * and needs no field buffer -- wr_decode_begin runs it, every decoded window going straight to the planes' device
 * buffers, which stay parked in the context -- the field buffer is only touched by the ~0.2 s of kernels and
 * download that wr_decode_finish_host / _device run.  (A streaming decoder with many fields in flight holds one
 * output field per finish in progress instead of one per field.)  One begin may be pending per context (another
 * begin, a whole decode or an encode on the context discards it); data_enc is not needed after begin has returned. */
int wr_decode_begin(wr_ctx *ctx, int nx, int ny, int nz, const wr_enc_info *info,
                    const unsigned char *data_enc, size_t data_len, wr_timings *tm);
int wr_decode_finish_host(wr_ctx *ctx, double *h_fld, wr_timings *tm);
int wr_decode_finish_device(wr_ctx *ctx, double *d_fld, wr_timings *tm);
/* The same for single-precision fields (fp32 host buffers, pinned or pageable): 4 bytes per sample cross the bus and
 * the field is widened / narrowed on the device, inside the first / last transform kernel where the fused transform
 * runs.  The arithmetic is the fp64 path's: the header, coded bytes and len_enc_vec are those wr_encode_host gives for
 * the field widened to double, and the decoded field is, bit for bit, (float) of what wr_decode_host returns (round to
 * nearest even; -0.0 and fp32 subnormals kept; inf where the reconstruction exceeds FLT_MAX).  h_fld of an encode is never
 * written: with wr_ctx_set_keep_residual(ctx, 1) the encode returns WR_ERR_UNSUPPORTED. */
int wr_encode_host_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                       int mz, const double *cutoffvec, wr_enc_info *info, unsigned char *data_enc,
                       size_t cap, wr_timings *tm);
int wr_decode_host_f32(wr_ctx *ctx, float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                       const unsigned char *data_enc, size_t data_len, wr_timings *tm);
int wr_decode_finish_host_f32(wr_ctx *ctx, float *h_fld, wr_timings *tm); /* after wr_decode_begin */
/* ---- Segmented plane streams ("WRS1"): an opt-in second stream format, coded and decoded on the GPU.
 * Transform, quantizer and header scalars are those of wr_encode_host for the same field; only the bytes of every plane in
 * data_enc differ.  A plane of n symbols is cut into segments of `seg` symbols, each coded as a complete stream of its own
 * (byte for byte wr_range_encode of those symbols), so that a field is tens of thousands of independent chains instead
 * of one per plane:
 *   plane blob := 'W','R','S','1' | u32 seg | u32 nseg = ceil(n / seg) | u32 len[nseg] | the segment streams, in order
 * (little endian; 16 <= seg <= 59999, a multiple of 16).  len_enc_vec[l] is the length of plane l's blob, ntot_enc their
 * sum.  The reference's tools and the other wr_decode_* entry points do NOT read this format (a reference stream starts
 * with byte 0x00).  seg = 0 means WR_SEG_DEFAULT everywhere. */
#define WR_SEG_DEFAULT 59904
size_t wr_seg_bound(size_t n, unsigned seg); /* worst-case blob bytes of one plane; 0 if seg is refused */
/* stage level, device pointers (16-byte aligned): code / decode one plane of n symbols.  bad_segments: segments whose
 * stream did not decode to their symbols (WR_ERR_STREAM then); a malformed index is refused before anything is launched. */
int wr_dev_seg_encode(wr_ctx *ctx, const unsigned char *d_sym, size_t n, unsigned seg, unsigned char *d_blob,
                      size_t cap, size_t *blob_len);
int wr_dev_seg_decode(wr_ctx *ctx, const unsigned char *d_blob, size_t blob_len, unsigned char *d_sym, size_t n,
                      size_t *bad_segments);
/* whole path: as wr_encode_host / wr_decode_host (and the fp32 and device-field forms), the planes coded by the GPU.
 * No coder pool, no host coder threads.  wr_timings: `rangecoder` is the time of the coder kernels and the compaction,
 * plane_coder_s[l] plane l's.  cap too small: WR_ERR_OVERFLOW; a malformed blob: WR_ERR_STREAM. */
int wr_encode_host_seg(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                       const double *cutoffvec, unsigned seg, wr_enc_info *info, unsigned char *data_enc, size_t cap,
                       wr_timings *tm);
int wr_decode_host_seg(wr_ctx *ctx, double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                       const unsigned char *data_enc, size_t data_len, wr_timings *tm);
int wr_encode_host_seg_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                           const double *cutoffvec, unsigned seg, wr_enc_info *info, unsigned char *data_enc,
                           size_t cap, wr_timings *tm);
int wr_decode_host_seg_f32(wr_ctx *ctx, float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                           const unsigned char *data_enc, size_t data_len, wr_timings *tm);
int wr_encode_device_seg(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                         const double *cutoffvec, unsigned seg, wr_enc_info *info, unsigned char *data_enc, size_t cap,
                         wr_timings *tm);
int wr_decode_device_seg(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, const wr_enc_info *info,
                         const unsigned char *data_enc, size_t data_len, wr_timings *tm);
/* ---- Encode to a byte budget: the call picks the tolerance, and codes every plane once.
 * The grid.  Relative tolerances are searched on the exact doubles
 *   t(g) = ldexp(64 + (g & 63), (g >> 6) - 66),  0 <= g <= WR_BUDGET_GMAX:  t(0) = 2^-60, t(3840) = 1,
 * neighbours at most a factor 65/64 apart.  wr_budget_tol(g) is t(g) (g clamped to the grid); wr_budget_index(tolrel) the
 * smallest g with t(g) >= tolrel, clamped to the grid.
 * The bound.  wr_seg_size_bound_host_ref(sym, n, seg) is an upper bound on wr_seg_encode_host_ref(sym, n, seg, ...) computed
 * from the segments' histograms alone: 12 + 4 nseg bytes of header and index, and per segment
 *   floor(bits / 8) + 5,  bits = 2 (1 + loss(2)) + 256 (16 + loss(2^16)) + bs (log2(bs) + loss(bs)) - sum c_s log2(c_s)
 * with bs the segment's symbols, c_s the count of symbol s and loss(t) = -log2(1 - t / 2^23), the rounding loss of a coder
 * step.  The arithmetic is integer (bits in units of 2^-12, from a table rounded in the safe direction), so the GPU gives
 * the same number.  0: seg refused.  B(g), the bound of a field at t(g), is the sum of this over the planes the quantizer
 * loop produces for cutoffvec = { t(g) }.
 * The call.  wr_encode_*_seg_budget take the arguments of wr_encode_host_seg / _f32 / wr_encode_device_seg with the cutoff
 * vector replaced by max_bytes and tol_min, and a result record.  With g_min = wr_budget_index(tol_min) they return a g in
 * [g_min, WR_BUDGET_GMAX] and a stream such that
 *   it fits          B(g) <= max_bytes, hence info->ntot_enc <= res->bound = B(g) <= max_bytes;
 *   it is tight      g == g_min or B(g - 1) > max_bytes (B is not proven monotone: this local property is the contract, not
 *                    "the smallest g of all");
 *   it is the same   info and data_enc are bit for bit what wr_encode_host_seg returns for cutoffvec = { t(g) } and this seg;
 *   coded once       WR_STAT_BUDGET_CODER_RUNS grows by info->nlay; res->probe_passes counts the launches of the size probe,
 *                    a pass over the coefficients that writes nothing.
 * A constant field gives nlay = 0, g = g_min, bound = 0.  WR_ERR_BUDGET: B(WR_BUDGET_GMAX) > max_bytes -- the floor is the
 * headers, about 520 bytes per segment; wr_last_error() names the smallest budget that would do, and data_enc is not written.
 * WR_ERR_UNSUPPORTED: a local cutoff (mx * my * mz > 1) and wr_ctx_set_keep_residual(ctx, 1).  WR_ERR_ARG: tol_min that is
 * not a positive number, and what wr_encode_host_seg refuses.  The stream is WRS1; for WRS2 / WRS3 recut it with
 * wr_transcode_host, which is lossless and runs no transform. */
#define WR_BUDGET_GMAX 3840
double wr_budget_tol(int g);
int wr_budget_index(double tolrel);
size_t wr_seg_size_bound_host_ref(const unsigned char *sym, size_t n, unsigned seg);
typedef struct wr_budget_result {
    int g;            /* the grid point chosen */
    double tolrel;    /* t(g) */
    size_t bound;     /* B(g) */
    int probe_passes; /* launches of the size probe */
} wr_budget_result;
#define WR_BUDGET_PROBE_MAX 8 /* candidate steps one pass of the size probe takes */
/* stage level, device pointers (16-byte aligned).  wr_dev_plane_size_bound: the bound of a plane of symbols, equal to
 * wr_seg_size_bound_host_ref of them.  wr_dev_quant_size_probe: for each of the ncand <= WR_BUDGET_PROBE_MAX steps deps[k],
 * bounds[k] = the bound of the plane (unsigned char)((d_resid[j] - minval) / deps[k] + 0.5) in the quantizer's own arithmetic
 * (aopt = 1 / deps, bopt = -minval * aopt + 0.5); d_resid is only read and no plane is written.  ncand outside
 * 1..WR_BUDGET_PROBE_MAX: WR_ERR_ARG. */
int wr_dev_plane_size_bound(wr_ctx *ctx, const unsigned char *d_sym, size_t n, unsigned seg, size_t *bound);
int wr_dev_quant_size_probe(wr_ctx *ctx, const double *d_resid, size_t n, double minval, int ncand, const double *deps,
                            unsigned seg, size_t *bounds);
int wr_encode_host_seg_budget(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                              size_t max_bytes, double tol_min, unsigned seg, wr_enc_info *info, unsigned char *data_enc,
                              size_t cap, wr_timings *tm, wr_budget_result *res);
int wr_encode_host_seg_budget_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                  int mz, size_t max_bytes, double tol_min, unsigned seg, wr_enc_info *info,
                                  unsigned char *data_enc, size_t cap, wr_timings *tm, wr_budget_result *res);
int wr_encode_device_seg_budget(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                size_t max_bytes, double tol_min, unsigned seg, wr_enc_info *info, unsigned char *data_enc,
                                size_t cap, wr_timings *tm, wr_budget_result *res);
/* ---- Encode to a pointwise error bound: the call picks the tolerance, and codes every plane once.
 * The relative tolerance of the plain calls steps the wavelet coefficients; what the samples end up with is only roughly
 * tolrel * max|f|.  These calls take the bound on the samples itself.
 * E(g).  For a field f and a point g of the grid above, E(g) = max_j |f[j] - r_g[j]|, r_g being bit for bit what
 * wr_decode_host_seg returns for the stream wr_encode_host_seg makes at cutoffvec = { wr_budget_tol(g) }.  One IEEE fp64
 * subtraction per sample; the maximum of such values is exact, so E(g) is a well-defined double.  For an fp32 field r_g is
 * the fp32 reconstruction of wr_decode_host_seg_f32 and both operands are widened to fp64 first.  The reconstruction does
 * not depend on the segmented format, seg, brick or strands, so E does not either.
 * The start.  wr_bounded_start(max_abs_err, absmax) is the largest g with wr_budget_tol(g) * absmax <= max_abs_err (one fp64
 * multiply, found by comparison over the grid, no libm), clamped to the grid; -1 when even t(0) is too coarse or an
 * argument is not a positive finite number.  absmax is max(|lo|, |hi|) of the field.
 * The call.  wr_encode_*_seg_bounded take the arguments of wr_encode_host_seg_strands / _f32 / wr_encode_device_seg_strands
 * with the cutoff vector replaced by max_abs_err and tol_min, and a result record.  brick = 0, strands = 0: WRS1; brick > 0:
 * WRS2; strands > 0: WRS3 (with or without a brick edge).  With g_min = wr_budget_index(tol_min) they return a g in
 * [g_min, WR_BUDGET_GMAX] such that
 *   it holds         E(g) <= max_abs_err, and res->err == E(g);
 *   it is tight      g == WR_BUDGET_GMAX or E(g + 1) > max_abs_err (E is not monotone: this local property is the contract,
 *                    not "the largest g of all");
 *   it is the same   info and data_enc are bit for bit what the plain call of the chosen format returns at cutoffvec = { t(g) };
 *   coded once       WR_STAT_BOUNDED_CODER_RUNS grows by info->nlay; res->trials counts the tolerances whose reconstruction
 *                    was formed.  A trial is a pass over the coefficients that writes the decoder's coefficient sum (no plane,
 *                    no coder), the decoder's inverse transform and a compare against the field, all on the device.
 * A constant field gives nlay = 0, g = WR_BUDGET_GMAX, err = 0, trials = 0.  WR_ERR_BOUND: E(g_min) > max_abs_err;
 * wr_last_error() names E(g_min) and data_enc is not written.  WR_ERR_ARG: a field holding a NaN or an infinity (the message
 * counts such samples; from these calls only), a max_abs_err or tol_min that is not a positive finite number, and what the
 * plain calls refuse.  WR_ERR_UNSUPPORTED: a local cutoff (mx * my * mz > 1) and wr_ctx_set_keep_residual(ctx, 1).
 * wtflag = 0 is supported (a trial then has no inverse).
 * Device memory.  Next to what the plain call takes, the trials take two work arrays of nx * ny * nz doubles and, where the
 * forward transform does not leave the field intact (any shape whose four levels do not all run on the fused kernels, and
 * wtflag = 0), a copy of the field (8 bytes per sample, 4 for an fp32 field).  They come from the plane pool and go back when
 * the call ends; a device that cannot give them returns the pool's usual error.
 * wr_seg_error_host / _f32: the measuring half on its own.  *err = max_j |h_fld[j] - r[j]| for the reconstruction r of an
 * existing segmented stream (WRS1, WRS2 or WRS3), formed and compared on the device; h_fld is only read.  WR_ERR_ARG when a
 * difference is not finite. */
typedef struct wr_bounded_result {
    int g;         /* the grid point chosen */
    double tolrel; /* t(g) */
    double err;    /* E(g) */
    int trials;    /* tolerances whose reconstruction was formed */
} wr_bounded_result;
int wr_bounded_start(double max_abs_err, double absmax);
/* stage level: d_acc[j] = the decoder's coefficient sum (what wr_dev_decode_planes accumulates before its inverse) of the nlay
 * planes the quantizer loop cuts from d_coef with the steps deps[l] and offsets minval[l], l = 0 .. nlay - 1, in its own
 * arithmetic (aopt = 1 / deps, bopt = -minval * aopt + 0.5); no plane is written, d_coef is only read and must not overlap
 * d_acc.  Pointers that are not 16-byte aligned take an element-wise form.  nlay outside 1 .. WR_NLAYMAX: WR_ERR_ARG. */
int wr_dev_requant_accum(wr_ctx *ctx, const double *d_coef, size_t n, int nlay, const double *deps, const double *minval,
                         double *d_acc);
int wr_encode_host_seg_bounded(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                               double max_abs_err, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                               wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_bounded_result *res);
int wr_encode_host_seg_bounded_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                   double max_abs_err, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                                   wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm,
                                   wr_bounded_result *res);
int wr_encode_device_seg_bounded(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                 double max_abs_err, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                                 wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_bounded_result *res);
int wr_seg_error_host(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                      const unsigned char *data_enc, size_t data_len, double *err);
int wr_seg_error_host_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                          const unsigned char *data_enc, size_t data_len, double *err);
/* measurement hook: HIP-event milliseconds of the three stages of a trial -- the coefficient sum, the inverse, the compare --
 * summed over the trials of the context's last encode to an error bound or to a quality target (null pointers are skipped) */
int wr_ctx_bounded_trial_ms(wr_ctx *ctx, double *requant_ms, double *inverse_ms, double *compare_ms);
/* ---- Encode to an RMS error or a PSNR target: the same search in the L2 norm, every plane coded once.
 * Definitions.  For a field f of n samples and a grid point g, r_g is as above (bit for bit the decoder's reconstruction of the
 * plain call's stream at t(g); for an fp32 field the fp32 reconstruction).  d_j = fl(f_j - r_j) in fp64, both operands widened
 * first for fp32; q_j = fl(d_j * d_j), ONE rounding (the library is built with -ffp-contract=off: this is not an FMA);
 * S*(g) = sum_j q_j, the real-number sum over the finite d_j; R*(g) = sqrt(S*(g) / n).  What the library computes is S(g), an
 * fp64 summation of the same q_j, and R(g) = fl(sqrt(fl(S / n))).  Two guarantees:
 *   reproducible   the same n, the same alignment class of the two pointers (both aligned for two-sample loads -- 16 bytes
 *                  fp64, 8 bytes fp32 -- or not) and the same library give the same bits on every run: per-thread partial sums
 *                  in index order, then a fixed tree over lanes, waves and blocks; no floating-point atomics, nothing depends
 *                  on the order in which blocks finish.  (Inside the calls below both arrays are always aligned.)
 *   accurate       |S - S*| <= 2^-36 * S* for every n <= 2^33 (the kernel's derivation gives 2^-38: csrc/wr_kernels.hip).
 * A q_j that overflows makes S = R = +inf, which holds no target.  range = hi - lo of the field, the values every encode's
 * prologue forms; PSNR = 20 log10(range / R), +inf for R = 0.
 * wr_psnr_rms(db, lo, hi) = (hi - lo) * pow(10, -db / 20): the RMS error that PSNR db means on a field of that range; NaN unless
 * db is finite and hi - lo is a positive finite number.  A PSNR target is converted with it once, on the host, and the value
 * is returned in res->max_rms: the contract is stated on R against THAT value, so nothing depends on libm's last bit.
 * The call.  wr_encode_*_seg_quality take the arguments of the _bounded calls with max_abs_err replaced by (norm, target):
 *   WR_NORM_MAX    target is max_abs_err: g, info and data_enc are the bounded call's; res->max_abs = E(g), res->range is
 *                  filled, res->rms, sumsq, psnr and max_rms are NaN (not measured)
 *   WR_NORM_RMS    target is max_rms, in the field's units
 *   WR_NORM_PSNR   target is in dB over the field's range; max_rms = wr_psnr_rms(target, lo, hi)
 * For WR_NORM_RMS and WR_NORM_PSNR, with g_min = wr_budget_index(tol_min), they return a g in [g_min, WR_BUDGET_GMAX] such that
 *   it holds         res->rms == R(g) <= res->max_rms; res->sumsq == S(g), res->max_abs == E(g), res->psnr from R(g) and range;
 *   it is tight      g == WR_BUDGET_GMAX, or the call formed R(g + 1) and it exceeds max_rms (R is not monotone: the local
 *                    property is the contract, as for E);
 *   it is the same   info and data_enc are bit for bit the plain call's of the chosen format at cutoffvec = { t(g) };
 *   coded once       WR_STAT_QUALITY_CODER_RUNS grows by info->nlay (for every norm; WR_STAT_BOUNDED_CODER_RUNS does not move).
 * The walk starts at wr_bounded_start(max_rms, absmax): R never exceeds E, so that point normally holds and the walk goes
 * coarser.  A constant field gives nlay = 0, g = WR_BUDGET_GMAX, rms = sumsq = max_abs = 0, trials = 0, psnr = +inf and
 * range = 2 * info->halfspanval.  WR_ERR_BOUND: R(g_min) > max_rms; wr_last_error() names R(g_min), data_enc is not written.
 * WR_ERR_ARG: an unknown norm, a target that is not a positive finite number, a PSNR target on a field with range == 0, and
 * everything the bounded calls refuse that way (a NaN or an infinity in the field among it); WR_ERR_UNSUPPORTED as there.
 * wtflag = 0 is supported.  Device memory as the bounded calls.
 * wr_seg_error_stats_host / _f32: the measuring half, as wr_seg_error_host, filling a record: max_abs, sumsq = S, rms = R (the
 * same kernel on arrays of the same alignment class: the bits the encode reported), lo and hi of h_fld (NaNs skipped, as the
 * prologue's), psnr, and the count of differences that are not finite.  WR_ERR_ARG when nonfinite > 0, the record still filled.
 * wr_dev_err_stats / _f32: the compare alone on two device arrays of n >= 1 samples, of any alignment; lo, hi and psnr are not
 * its business and come back as NaN.  It returns WR_OK whatever nonfinite is. */
enum { WR_NORM_MAX = 1, WR_NORM_RMS = 2, WR_NORM_PSNR = 3 };
typedef struct wr_quality_result {
    int g;          /* the grid point chosen */
    double tolrel;  /* t(g) */
    double max_abs; /* E(g) */
    double rms;     /* R(g) */
    double sumsq;   /* S(g) */
    double range;   /* hi - lo of the field */
    double psnr;    /* 20 log10(range / R(g)), +inf for R(g) = 0 */
    double max_rms; /* the RMS target R(g) was held against: `target`, or what a PSNR target was converted to */
    int trials;     /* tolerances whose reconstruction was formed */
} wr_quality_result;
typedef struct wr_error_stats {
    double max_abs, sumsq, rms, lo, hi, psnr;
    unsigned long long nonfinite;
} wr_error_stats;
double wr_psnr_rms(double db, double lo, double hi);
int wr_encode_host_seg_quality(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                               int norm, double target, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                               wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_quality_result *res);
int wr_encode_host_seg_quality_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                   int norm, double target, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                                   wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm,
                                   wr_quality_result *res);
int wr_encode_device_seg_quality(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                 int norm, double target, double tol_min, unsigned seg, unsigned brick, unsigned strands,
                                 wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_quality_result *res);
int wr_seg_error_stats_host(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                            const unsigned char *data_enc, size_t data_len, wr_error_stats *stats);
int wr_seg_error_stats_host_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                                const unsigned char *data_enc, size_t data_len, wr_error_stats *stats);
int wr_dev_err_stats(wr_ctx *ctx, const double *d_a, const double *d_b, size_t n, wr_error_stats *stats);
int wr_dev_err_stats_f32(wr_ctx *ctx, const float *d_a, const float *d_b, size_t n, wr_error_stats *stats);
/* ---- Masked fields: undefined samples travel as a bit mask, split from the field and put back on the GPU.
 * Semantics.  A sample x of the field (fp64, or fp32 widened exactly) is UNDEFINED if it is not finite, !(fabs(x) <= DBL_MAX),
 * or if x < below; `below` is the caller's threshold (-INFINITY switches it off, a NaN is WR_ERR_ARG).  All other samples are
 * defined.  A masked encode
 *   splits    finds the undefined samples, counts them (`undefined`, exact) and forms pad = S / count, the mean of the defined
 *             samples: S is an fp64 sum in an order that n alone fixes (a thread in index order, lanes by shuffles at distances
 *             32 .. 1, waves in order, partials in order; no floating-point atomics), so pad has the same bits on every run.  For
 *             an fp32 field pad is that mean rounded to float, and the rounded value is what is stored and returned;
 *   fills     every undefined sample with pad, in the device's work space: the caller's host buffer is only read (a
 *             device-resident field is consumed, as by wr_encode_device_seg);
 *   encodes   the padded field as the plain call of the chosen format does -- brick == 0 && strands == 0: WRS1
 *             (wr_encode_host_seg), brick != 0: WRS2 (_blocked), strands != 0: WRS3 (_strands, brick 0 or an edge); nothing is
 *             defaulted but seg -- so that info and the first info->ntot_enc bytes of data_enc are bit for bit what that call
 *             returns for the caller's field with its undefined samples replaced by the returned pad;
 *   appends   the mask blob at data_enc + info->ntot_enc, res->mask_len bytes.
 * undefined == 0: mask_len == 0 and the whole result is the plain call's.  No defined sample: WR_ERR_ARG, nothing written.  A
 * constant padded field (nlay == 0, ntot_enc == 0): the trivial record, and the mask blob at data_enc.  cap must hold the
 * field's planes plus wr_mask_bound(n, seg) bytes when a sample is undefined: WR_ERR_OVERFLOW otherwise, before data_enc is
 * written.  Every existing decoder, region decode, low-resolution decode and wr_transcode_host reads the field part as it is,
 * and returns the padded field; wr_decode_*_seg_roi_masked (further down) are the region and low-resolution decodes that
 * put `fill` back.
 * The mask blob ("WRM1", little endian):
 *   'W','R','M','1' | u32 0 | u64 n | u64 undefined | f64 pad | WRS1 plane blob of ceil(n / 8) symbols
 * Bit j & 7 (least significant first) of symbol j >> 3 is 1 iff sample j, in the field's memory order, is undefined; the unused
 * high bits of the last symbol are 0.  The WRS1 blob is exactly wr_seg_encode_host_ref of those symbols at the call's segment
 * length, whatever the field's format.  pad is informative: no decoder needs it.
 * A masked decode takes data_len = field planes + mask blob; data_len == info->ntot_enc (or 0) is an unmasked record and
 * decodes as wr_decode_host_seg.  Undefined samples come back as `fill` (any double, a NaN included; (float)fill for fp32).
 * WR_ERR_STREAM, before anything is written to the caller's field: a wrong magic, a nonzero reserved word, an n other than
 * nx * ny * nz, a truncated or overlong blob, a WRS1 blob that does not decode, a set bit beyond n, a population count other
 * than `undefined`.
 * wr_mask_bound: the worst-case mask_len (0: seg refused).  wr_mask_blob_host_ref / wr_mask_parse_host_ref: the blob's
 * definition on the calling thread, no device needed: from / to one flag byte (0 or 1) per sample; parse applies every refusal
 * above (null outputs are skipped).  wr_mask_sniff: 1 if data starts like a mask blob.
 * Stage level (device pointers of any alignment, n >= 1).  wr_dev_mask_split: d_bits[0, ceil(n / 8)) = the mask, *undefined and
 * *pad as above (pad is a NaN when no sample is defined; the call still succeeds).  wr_dev_mask_fill: d_fld[j] = value where bit
 * j is set, nothing else is touched.  wr_dev_mask_restore: the same with the mask checked: *undefined = its set bits,
 * WR_ERR_STREAM if one lies at or beyond n.
 * wr_mask_result: split_ms, fill_ms (a decode: the restore), mask_coder_ms are HIP-event milliseconds; the mask's coder kernels
 * run on a stream of their own under the field's transform and quantizer (a decode: under the field's coder stage). */
typedef struct wr_mask_result {
    unsigned long long undefined;
    double pad;
    size_t mask_len;
    float split_ms, fill_ms, mask_coder_ms;
} wr_mask_result;
size_t wr_mask_bound(size_t n, unsigned seg);
size_t wr_mask_blob_host_ref(const unsigned char *undef_flags, size_t n, unsigned seg, double pad, unsigned char *blob);
int wr_mask_parse_host_ref(const unsigned char *blob, size_t len, size_t n, unsigned char *undef_flags,
                           unsigned long long *undefined, double *pad);
int wr_mask_sniff(const unsigned char *data, size_t len);
int wr_dev_mask_split(wr_ctx *ctx, const double *d_fld, size_t n, double below, unsigned char *d_bits,
                      unsigned long long *undefined, double *pad);
int wr_dev_mask_split_f32(wr_ctx *ctx, const float *d_fld, size_t n, double below, unsigned char *d_bits,
                          unsigned long long *undefined, double *pad);
int wr_dev_mask_fill(wr_ctx *ctx, double *d_fld, size_t n, const unsigned char *d_bits, double value);
int wr_dev_mask_fill_f32(wr_ctx *ctx, float *d_fld, size_t n, const unsigned char *d_bits, double value);
int wr_dev_mask_restore(wr_ctx *ctx, double *d_fld, size_t n, const unsigned char *d_bits, double fill,
                        unsigned long long *undefined);
int wr_dev_mask_restore_f32(wr_ctx *ctx, float *d_fld, size_t n, const unsigned char *d_bits, double fill,
                            unsigned long long *undefined);
int wr_encode_host_seg_masked(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                              const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands, double below,
                              wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_mask_result *res);
int wr_encode_host_seg_masked_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                  const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands, double below,
                                  wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_mask_result *res);
int wr_encode_device_seg_masked(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands, double below,
                                wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm, wr_mask_result *res);
int wr_decode_host_seg_masked(wr_ctx *ctx, double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                              const unsigned char *data_enc, size_t data_len, double fill, wr_timings *tm, wr_mask_result *res);
int wr_decode_host_seg_masked_f32(wr_ctx *ctx, float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                                  const unsigned char *data_enc, size_t data_len, double fill, wr_timings *tm,
                                  wr_mask_result *res);
int wr_decode_device_seg_masked(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, const wr_enc_info *info,
                                const unsigned char *data_enc, size_t data_len, double fill, wr_timings *tm,
                                wr_mask_result *res);
/* ---- Masked fields in the tolerance searches: the error is taken over the defined samples only.
 * Definitions.  Let D be the set of defined samples of the field f under `below` (above), nd = |D| = n - undefined, pad the
 * split's mean, f_pad the padded field, and r_g the reconstruction of the plain call's stream of f_pad at t(g), formed exactly
 * as a trial of the bounded and quality calls forms it (the fp32 reconstruction for an fp32 field).  Then
 *   E_D(g) = max over j in D of |f_j - r_g[j]|           (one fp64 subtraction per sample: exact, whatever the order)
 *   S_D(g) = the fp64 sum over j in D of fl(d_j * d_j), d_j = fl(f_j - r_g[j])      (finite d_j only)
 *   R_D(g) = fl(sqrt(fl(S_D / nd)))                      (the division is by nd, not by n)
 * lo, hi and range = hi - lo are those of the defined samples.  They equal the values the prologue forms for f_pad, because the
 * mean of the defined samples -- and, for an fp32 field, that mean rounded to float, rounding being monotone -- lies in
 * [lo, hi]; the calls rely on this: the start point of the walk and the conversion of a PSNR target use the prologue's lo and
 * hi of f_pad.  The two guarantees of the quality calls hold as stated there: reproducible (the same n, the same mask, the same
 * alignment class and the same library give the same bits: per-thread sums in index order, a fixed tree over lanes, waves and
 * blocks, no floating-point atomics) and accurate (|S_D - S_D*| <= 2^-36 * S_D* for every n <= 2^33, S_D* the real sum of the
 * same rounded squares; the kernel's derivation gives 2^-38: csrc/wr_mask.hip).  A difference at a DEFINED sample that is not
 * finite is counted in `nonfinite`; nothing at an undefined position is ever looked at, whatever the two arrays hold there.
 * wr_encode_*_seg_quality_masked take the arguments of the _quality calls plus `below`, and fill a wr_quality_result and a
 * wr_mask_result (mres may be null).  The contract is that of the quality calls with E_D, S_D, R_D in the place of E, S, R:
 *   it holds / it is tight / coded once   as there; WR_NORM_MAX is the masked pointwise bound, E_D(g) <= target (rms, sumsq, psnr
 *                    and max_rms NaN, as there); WR_STAT_QUALITY_CODER_RUNS grows by info->nlay;
 *   it is the same   info and the first info->ntot_enc bytes of data_enc are bit for bit the plain call's stream of f_pad at
 *                    t(g) in the chosen format; the mask blob behind them, mres->mask_len bytes, and mres are what
 *                    wr_encode_*_seg_masked gives at that tolerance.
 * undefined == 0: the plain compare runs, and the whole result is bit for bit the plain quality call's.  A sample that is not
 * finite is undefined by definition, so the quality calls' refusal of such a field does not apply.
 * wr_encode_*_seg_budget_masked take the arguments of the _budget calls plus `below`.  The budget holds the whole record:
 *   it fits          B(g) + mask_len <= max_bytes, mask_len the blob's exact length (the search waits for the mask's coder
 *                    before its first probe); res->bound = B(g);
 *   it is the same   g, res->bound, res->probe_passes, info and the first info->ntot_enc bytes are bit for bit what
 *                    wr_encode_host_seg_budget returns for f_pad with max_bytes - mask_len; the blob is the masked call's.
 * WR_ERR_BUDGET: max_bytes <= mask_len on a field that is not constant, or B(WR_BUDGET_GMAX) + mask_len > max_bytes;
 * wr_last_error() names mask_len + B(WR_BUDGET_GMAX), the smallest budget that would do, and data_enc is not written.  WRS1 only.
 * Common to both: cap must hold the planes plus wr_mask_bound(n, seg); no defined sample and a NaN `below`: WR_ERR_ARG; a
 * constant f_pad: nlay = 0, g = WR_BUDGET_GMAX (budget: g_min), errors 0, trials = 0, the blob at data_enc; a local cutoff and
 * wr_ctx_set_keep_residual(ctx, 1): WR_ERR_UNSUPPORTED.
 * wr_seg_error_stats_host_masked / _f32: the measuring half.  data_len = the planes plus the mask blob of a masked record (the
 * blob validated as wr_decode_host_seg_masked validates it: WR_ERR_STREAM; data_len == info->ntot_enc: an unmasked record,
 * every sample defined).  The record is filled over the RECORD's defined samples -- max_abs = E_D, sumsq = S_D, rms = R_D, the
 * bits the encode reported; lo and hi of the defined samples of h_fld -- and *defined = nd.  h_fld may hold anything at the
 * undefined positions.  WR_ERR_ARG when nonfinite > 0, with the record still filled.
 * wr_dev_err_stats_masked / _f32: the masked compare alone on two device arrays of n >= 1 samples and a packed mask d_bits (bit
 * j & 7 of byte j >> 3), all of any alignment; no mask byte at or beyond ceil(n / 8) and no sample at or beyond n is read, and what a
 * sample whose bit is set holds never matters.
 * *defined = the clear bits below n, rms = sqrt(sumsq / *defined) (a NaN when there is none); lo, hi and psnr come back as
 * NaN.  It returns WR_OK whatever nonfinite is. */
int wr_encode_host_seg_quality_masked(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                      int mz, int norm, double target, double tol_min, unsigned seg, unsigned brick,
                                      unsigned strands, double below, wr_enc_info *info, unsigned char *data_enc, size_t cap,
                                      wr_timings *tm, wr_quality_result *res, wr_mask_result *mres);
int wr_encode_host_seg_quality_masked_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                          int mz, int norm, double target, double tol_min, unsigned seg, unsigned brick,
                                          unsigned strands, double below, wr_enc_info *info, unsigned char *data_enc,
                                          size_t cap, wr_timings *tm, wr_quality_result *res, wr_mask_result *mres);
int wr_encode_device_seg_quality_masked(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                        int norm, double target, double tol_min, unsigned seg, unsigned brick,
                                        unsigned strands, double below, wr_enc_info *info, unsigned char *data_enc, size_t cap,
                                        wr_timings *tm, wr_quality_result *res, wr_mask_result *mres);
int wr_encode_host_seg_budget_masked(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                     int mz, size_t max_bytes, double tol_min, unsigned seg, double below, wr_enc_info *info,
                                     unsigned char *data_enc, size_t cap, wr_timings *tm, wr_budget_result *res,
                                     wr_mask_result *mres);
int wr_encode_host_seg_budget_masked_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                         int mz, size_t max_bytes, double tol_min, unsigned seg, double below,
                                         wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm,
                                         wr_budget_result *res, wr_mask_result *mres);
int wr_encode_device_seg_budget_masked(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                       size_t max_bytes, double tol_min, unsigned seg, double below, wr_enc_info *info,
                                       unsigned char *data_enc, size_t cap, wr_timings *tm, wr_budget_result *res,
                                       wr_mask_result *mres);
int wr_seg_error_stats_host_masked(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                                   const unsigned char *data_enc, size_t data_len, wr_error_stats *stats,
                                   unsigned long long *defined);
int wr_seg_error_stats_host_masked_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, const wr_enc_info *info,
                                       const unsigned char *data_enc, size_t data_len, wr_error_stats *stats,
                                       unsigned long long *defined);
int wr_dev_err_stats_masked(wr_ctx *ctx, const double *d_a, const double *d_b, size_t n, const unsigned char *d_bits,
                            wr_error_stats *stats, unsigned long long *defined);
int wr_dev_err_stats_masked_f32(wr_ctx *ctx, const float *d_a, const float *d_b, size_t n, const unsigned char *d_bits,
                                wr_error_stats *stats, unsigned long long *defined);
/* ---- Low-resolution decode of segmented streams: a coarse version of the field without decoding the field.
 * The transform is a Mallat decomposition (waveletcdf97_3d.c:73-78): after level r the low-pass coefficients of an nx*ny*nz
 * field sit in the corner box [0,bx) x [0,by) x [0,bz) of the coefficient array.  With h(n) = (n + 1) / 2 in integer
 * arithmetic, for a header record `info` and a level r, 0 <= r <= info->wlev:
 *   box       bx = h^r(nx), likewise by, bz
 *   exponent  e = the sum over the three axes and the levels j = 1..r of [h^(j-1)(n_axis) > 1] (an axis of extent 1 at a level
 *             is not transformed there and adds nothing: the DC gain of a level is sqrt(2) per transformed axis)
 *   scale     s = 2^(-e/2) as a double: ldexp(e odd ? 0x1.6a09e667f3bcdp-1 : 1.0, -(e / 2))
 *   planes    p planes are used, 1 <= p <= info->nlay; max_planes == 0 means all of them
 * The result D(r, p) is an array of bx*by*bz doubles, x fastest:
 *   1. C[j] = 0; for l = 0..p-1 in order: C[j] += q_l[j] * deps_vec[l] + minval_vec[l]   (no contraction, this order)
 *   2. A = the contiguous copy of C over z < bz, y < by, x < bx
 *   3. if wlev - r > 0: waveletcdf97_3d(bx, by, bz, -(wlev - r), A)
 *   4. out = A * s, one multiply and one rounding (s = 1 at r = 0)
 *   5. for fp32 output (float)out, rounded as wr_decode_host_seg_f32 rounds
 * D(0, nlay) is the full decode, bit for bit.  A constant field (info->ntot_enc == 0) gives midval at the box's size.
 * wlev == 0 with r > 0, r > wlev, r outside [0, 4] or p > nlay: WR_ERR_ARG.
 * Segments: for a plane cut at `seg`, run (y, z) of the box needs the segments floor(row*nx / seg) .. floor((row*nx + bx - 1)
 * / seg), row = y + ny*z; the union over the box's runs is decoded, and only those segments' bytes go to the device.  Every
 * plane's header and index are validated as by wr_decode_host_seg before anything is launched. */
int wr_lowres_dims(int nx, int ny, int nz, int level, int *bx, int *by, int *bz); /* host only */
double wr_lowres_scale(int nx, int ny, int nz, int level); /* s above; host only; 0 for a refused argument */
/* ascending ids of the segments a level needs; returns their number (ids may be NULL to count; at most cap are written),
 * 0 if seg or another argument is refused */
size_t wr_seg_lowres_segments(int nx, int ny, int nz, int level, unsigned seg, uint32_t *ids, size_t cap);
/* stage level: from nlay full planes at a pitch of wr_plane_pitch(n) in device memory (any format decoded them); d_out
 * receives bx*by*bz doubles */
int wr_dev_decode_planes_lowres(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                                const unsigned char *d_planes, const wr_enc_info *info);
/* whole path, as wr_decode_host_seg / _f32 / wr_decode_device_seg; the output holds bx*by*bz elements.  wr_timings as there:
 * h2d_ms the copies of the needed streams, rangecoder / plane_coder_s the decoder launches, quant_ms the box dequantiser,
 * transform_ms the inverse on the box and the scaling. */
int wr_decode_host_seg_lowres(wr_ctx *ctx, double *h_out, int nx, int ny, int nz, int level, int max_planes,
                              const wr_enc_info *info, const unsigned char *data_enc, size_t data_len, wr_timings *tm);
int wr_decode_host_seg_lowres_f32(wr_ctx *ctx, float *h_out, int nx, int ny, int nz, int level, int max_planes,
                                  const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                                  wr_timings *tm);
int wr_decode_device_seg_lowres(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                                const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                                wr_timings *tm);
/* ---- Region decode of segmented streams: a sub-box of the field (or of a low-resolution box) without decoding the field.
 * D(r, p) is the low-resolution decode above before its fp32 narrowing; D(0, nlay) is the full decode.  For a level
 * 0 <= r <= wlev, p planes (max_planes, 0 = all) and a half-open box roi = [x0,x1) x [y0,y1) x [z0,z1) in the coordinates of
 * D(r, p), 0 <= lo < hi <= b_axis, b = h^r(n):
 *   R(r, p, roi) is the contiguous copy of D(r, p) over the box, bit for bit, x fastest;
 *   for fp32 output (float) of that, rounded as wr_decode_host_seg_f32 rounds;
 *   a constant field (info->ntot_enc == 0) gives midval at the box's size;
 *   an empty or out-of-range box and every argument the low-resolution decode refuses: WR_ERR_ARG.
 * Lifting is local: with d = wlev - r levels still to invert an output sample depends on coefficients within a bounded
 * distance, so the region is inverted inside a window.  Per axis, n the extent of the level-r box, [lo, hi) the region:
 *   d = 0:  a = lo, b = hi
 *   else    m(0) = 0, m(k) = 2 (m(k-1) + 2)   (4, 12, 28, 60);  A = 2^d
 *           a = floor(max(0, lo - m(d)) / A) * A
 *           b = ceil((hi + m(d)) / A) * A, replaced by n when it reaches or passes n
 * A window starts on a multiple of 2^d (pair parity is the field's at every level) and ends on one or on the field's true end
 * (its level extents w_l = ceil(b / 2^l) - a / 2^l follow the field's ceil chain, so the odd-length step of
 * waveletcdf97_3d.c:314 happens where the field's does); each inverse level spoils at most 2 pairs beyond what a cut edge had
 * already spoilt (the stages at waveletcdf97_3d.c:316-330), which is the recursion for m.
 * The window's coefficient array W is wx*wy*wz doubles in the Mallat layout of its own extents;
 * waveletcdf97_3d(wx, wy, wz, -d, W) inverts it as it stands.  It is filled from the coefficient array C of step 1 above: for a
 * window point c = (cx, cy, cz),
 *   lambda = the number of l in 1..d with c_axis < w_l(axis) on all three axes;  ell = min(lambda + 1, d)
 *   per axis, with n_ell = h^ell(n) and a_ell = a >> ell:  f = a_ell + c  when c < w_ell,  n_ell + a_ell + (c - w_ell) otherwise
 *   W[c] = C[fx + nx * (fy + ny * fz)]          (nx, ny: the extents of the FIELD, not of the level-r box)
 * i.e. the low-pass box of level d plus up to seven detail octants per level, at most 29 source boxes.  The map is not
 * separable per axis: a point that is a level-1 detail in x takes its y and z at level-1 granularity.
 * The result is W inverted, cropped to [lo - a, hi - a) per axis and multiplied by s = wr_lowres_scale(nx, ny, nz, r), one
 * multiply and one rounding.
 * Segments: a plane cut at `seg` needs the segments the x-runs of those source boxes touch, and no others; only their bytes go
 * to the device.  Every plane's header and index are validated as by wr_decode_host_seg before anything is launched. */
typedef struct wr_box { int x0, y0, z0, x1, y1, z1; } wr_box;
/* the window of a region, in the coordinates of the level's box; wlev is 0 or 4 (the stream's); host only */
int wr_roi_window(int nx, int ny, int nz, int level, int wlev, const wr_box *roi, wr_box *win);
/* which kernels a region decode runs (host only: no device call, no context; the refusals of wr_roi_window, and out == NULL:
 * WR_ERR_ARG).  `inverse` = wlev - level levels are still to invert on the window `win`; `fused` says whether they run on the
 * fused inverse (out of place, as wr_fused_plan's `used` for the window's extents, after the WR_NO_FUSED switch) and
 * `fused_levels` how many of them it takes itself (0 when it does not run), the rest and every window with inverse < 4 run on
 * the general kernels.  box[0, nbox) are the source boxes of the gather in launch order, x, y, z: len coefficients per axis
 * from src of the field's array land at dst of the window; `wide`: the box is gathered 4 symbols at a time, otherwise byte by
 * byte (planes and work space aligned as the library's own always are). */
typedef struct wr_roi_plan_t {
    wr_box win;
    int inverse;
    int fused, fused_levels;
    int nbox;
    struct { int src[3], dst[3], len[3]; int wide; } box[29];
} wr_roi_plan_t;
int wr_roi_plan(int nx, int ny, int nz, int level, int wlev, const wr_box *roi, wr_roi_plan_t *out);
/* ascending ids of the segments a region needs; conventions of wr_seg_lowres_segments */
size_t wr_seg_roi_segments(int nx, int ny, int nz, int level, int wlev, const wr_box *roi, unsigned seg, uint32_t *ids,
                           size_t cap);
/* stage level, as wr_dev_decode_planes_lowres; d_out receives the region's elements */
int wr_dev_decode_planes_roi(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                             const wr_box *roi, const unsigned char *d_planes, const wr_enc_info *info);
/* whole path, as wr_decode_host_seg_lowres / _f32 / wr_decode_device_seg_lowres; the output holds the region's elements.
 * wr_timings: quant_ms is the window dequantiser, transform_ms the inverse on the window, the crop and the scaling. */
int wr_decode_host_seg_roi(wr_ctx *ctx, double *h_out, int nx, int ny, int nz, int level, int max_planes,
                           const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                           wr_timings *tm);
int wr_decode_host_seg_roi_f32(wr_ctx *ctx, float *h_out, int nx, int ny, int nz, int level, int max_planes,
                               const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                               wr_timings *tm);
int wr_decode_device_seg_roi(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                             const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                             wr_timings *tm);
/* ---- Masked region and low-resolution decode: the two partial decodes above with the mask of a masked record cropped on the
 * GPU.  No new format: the record is what wr_encode_*_seg_masked wrote (field part WRS1, WRS2 or WRS3; the mask blob behind
 * it, always a WRS1 plane in natural order).  b = h^r(n) per axis, r in 0 .. wlev; roi is a half-open box in the coordinates
 * of the level-r box, roi == NULL means the whole box of the level (the low-resolution decode); p = max_planes.
 * R(r, p, roi) is what wr_decode_host_seg_roi returns for the field part (wr_decode_host_seg_lowres for roi == NULL).
 * The coarse mask.  Sample (i, j, k) of the level-r box is undefined iff sample (i << r, j << r, k << r) of the field is: mask
 * bit J = (i << r) + nx * ((j << r) + ny * (k << r)), formed in size_t.  i << r <= n_axis - 1 always holds (i < ceil(n / 2^r));
 * it is the position the level-r low-pass sample sits at, since lifting keeps the even samples.  No bit at or beyond n is ever
 * read.  At r = 0 this is the mask itself.
 * The masked result.  M(r, p, roi, fill)[x, y, z] = fill where coarse sample (x0 + x, y0 + y, z0 + z) is undefined, and
 * R(r, p, roi)[x, y, z] otherwise; (float)fill for fp32 output; a NaN fill is allowed.  So
 *   M(0, nlay, roi, fill) is bit for bit the crop of what wr_decode_host_seg_masked returns with the same fill;
 *   M(r, ...) is where(und[::2^r, ::2^r, ::2^r][roi], fill, R(r, ...));
 *   a record without a blob (data_len == info->ntot_enc, or 0) decodes as the plain call, and res is zeroed;
 *   a constant padded field (nlay == 0, the blob at data_enc) gives midval with fill restored.
 * Mask segments.  For a run (y, z) of the region the bits J(x0, y, z) .. J(x1 - 1, y, z) lie in symbols J >> 3, a symbol in
 * segment (J >> 3) / seg, seg being read from the blob's own WRS1 header, not from the field part.  The ascending union over
 * the region's runs (wr_mask_roi_segments) is all that is uploaded and decoded of the mask.
 * Refusals.  Every argument the plain region / low-resolution call refuses: WR_ERR_ARG.  The blob's header and its whole
 * segment index are validated on the host as by the full masked decode: a wrong magic, a nonzero reserved word, another n, a
 * truncated or overlong blob: WR_ERR_STREAM, nothing launched.  A LISTED mask segment that does not decode: WR_ERR_STREAM
 * before a byte of the caller's output is written.  Two checks of the full decode are NOT made by a partial decode: the
 * population count against the header's `undefined`, and the unused high bits of the last symbol.  Damage inside a segment the
 * region does not list does not fail the call: that segment is not decoded.
 * res: undefined = the number of undefined samples INSIDE THE RETURNED BOX, counted by the restore kernel; pad and mask_len as
 * in the full decode; fill_ms the box restore, mask_coder_ms the mask's list-decoder launch, split_ms 0.
 * WR_STAT_MASK_ROI_SEGMENTS moves by the listed mask segments, WR_STAT_MASK_ROI_BYTES_UP by their stream bytes.
 * wr_mask_roi_segments: host only, no device and no context; conventions of wr_seg_roi_segments (seg == 0: WR_SEG_DEFAULT).
 * wr_dev_mask_restore_box: stage level, device pointers of any alignment: d_out is the contiguous region, x fastest; d_bits
 * the full-length mask plane of ceil(n / 8) bytes, of which only the bytes that hold a bit of the region are read;
 * *undefined = the set bits among the region's. */
size_t wr_mask_roi_segments(int nx, int ny, int nz, int level, const wr_box *roi, unsigned seg, uint32_t *ids, size_t cap);
int wr_dev_mask_restore_box(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, const wr_box *roi,
                            const unsigned char *d_bits, double fill, unsigned long long *undefined);
int wr_dev_mask_restore_box_f32(wr_ctx *ctx, float *d_out, int nx, int ny, int nz, int level, const wr_box *roi,
                                const unsigned char *d_bits, double fill, unsigned long long *undefined);
int wr_decode_host_seg_roi_masked(wr_ctx *ctx, double *h_out, int nx, int ny, int nz, int level, int max_planes,
                                  const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc, size_t data_len,
                                  double fill, wr_timings *tm, wr_mask_result *res);
int wr_decode_host_seg_roi_masked_f32(wr_ctx *ctx, float *h_out, int nx, int ny, int nz, int level, int max_planes,
                                      const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc,
                                      size_t data_len, double fill, wr_timings *tm, wr_mask_result *res);
int wr_decode_device_seg_roi_masked(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                                    const wr_box *roi, const wr_enc_info *info, const unsigned char *data_enc,
                                    size_t data_len, double fill, wr_timings *tm, wr_mask_result *res);
/* host reference of the WRS1 format (its definition further up, on the calling thread): for tests and for readers without a GPU.
 * blob holds wr_seg_bound(n, seg) bytes; returns the blob's length (0: seg refused, wr_last_error says why). */
size_t wr_seg_encode_host_ref(const unsigned char *sym, size_t n, unsigned seg, unsigned char *blob);
int wr_seg_decode_host_ref(const unsigned char *blob, size_t len, unsigned char *sym, size_t n);

/* ---- Blocked symbol order for segmented streams ("WRS2"): an opt-in third stream format.  Everything is WRS1's -- transform,
 * quantizer, header scalars, the segment coder, the rules for `seg` -- except the ORDER in which a plane's symbols are cut
 * into segments: subband by subband, and inside a subband in bricks of B^3, so that the low-pass box of every level is a
 * prefix of the plane and a region of the field is a few bricks of every subband.
 * For a field nx*ny*nz, wlev levels (the stream's: 0 or 4), h(n) = (n + 1) / 2, level extents e_0 = n, e_l = h(e_{l-1}) per
 * axis, and a brick edge B:
 *   boxes    first the low-pass box [0, e_wlev)^3; then for l = wlev, ..., 1 the seven octants o = 1..7, bit 0 / 1 / 2 of o
 *            saying whether x / y / z takes the high part [e_l, e_{l-1}) or the low part [0, e_l) of level l.  A box with an
 *            empty axis (the high part of an axis of extent 1) contributes nothing.  wlev = 0: one box, the field.
 *   bricks   inside a box in (tz, ty, tx) order, tx fastest; brick (tx, ty, tz) covers [tx*B, min((tx+1)*B, ex)) and likewise
 *            in y and z.  Partial bricks at the high edges hold exactly their hx*hy*hz symbols, no padding.
 *   symbols  inside a brick x fastest, then y, then z.
 * This is a permutation pi of [0, n): stream position -> coefficient index fx + nx * (fy + ny * fz).  The boxes of the levels
 * above r tile the box of level r (the low-resolution decode's), so that box is the first bx*by*bz stream positions, for
 * every r <= wlev.
 *   plane blob := 'W','R','S','2' | u32 seg | u32 nseg | u32 brick | u32 len[nseg] | the segment streams, in order
 * Segment k is byte for byte wr_range_encode of the stream positions [k*seg, ...) of the permuted plane.  B is one of 8, 16,
 * 32, 64; brick = 0 means WR_BRICK_DEFAULT everywhere.  Every plane of a stream has the same format and the same brick:
 * anything else is WR_ERR_STREAM, as is a brick that is not one of the four, before anything is launched.
 * The wr_decode_*_seg, _seg_lowres and _seg_roi entry points above read the magic of every plane and decode either format;
 * their results are bit for bit those of the WRS1 stream of the same field.  A low-resolution decode of a blocked stream
 * needs the segments 0 .. ceil(bx*by*bz / seg) - 1; a region decode the segments that the x-runs of its source boxes fall
 * into under pi. */
#define WR_BRICK_DEFAULT 32
int wr_blocked_order(int nx, int ny, int nz, int wlev, unsigned brick, uint64_t *pi); /* pi[n]; host only */
size_t wr_seg_bound_blocked(size_t n, unsigned seg); /* worst-case blob bytes of one plane; 0 if seg is refused */
/* ascending ids of the segments a level / a region needs of a blocked plane; conventions of wr_seg_lowres_segments and
 * wr_seg_roi_segments */
size_t wr_seg_lowres_segments_blocked(int nx, int ny, int nz, int level, int wlev, unsigned brick, unsigned seg,
                                      uint32_t *ids, size_t cap);
size_t wr_seg_roi_segments_blocked(int nx, int ny, int nz, int level, int wlev, const wr_box *roi, unsigned brick,
                                   unsigned seg, uint32_t *ids, size_t cap);
/* stage level, device pointers (16-byte aligned), n = nx*ny*nz bytes each, not in place.  inverse == 0: d_dst[p] =
 * d_src[pi[p]] (natural order to blocked); otherwise d_dst[pi[p]] = d_src[p]. */
int wr_dev_plane_reorder(wr_ctx *ctx, unsigned char *d_dst, const unsigned char *d_src, int nx, int ny, int nz, int wlev,
                         unsigned brick, int inverse);
/* the same over a subset of the bricks: only the stream positions of the listed bricks (and the coefficients they map to) are
 * read and written, so what d_dst held everywhere else is still there afterwards -- d_dst is NOT cleared.  Brick ids count the
 * bricks of the boxes in stream order (box after box, inside a box tz, ty, tx with tx fastest).  ids[0, nlist) is in HOST
 * memory, strictly ascending, every id below the plane's number of bricks (wr_reorder_plan's nbricks): anything else, a null
 * ids with nlist > 0 and what wr_dev_plane_reorder refuses is WR_ERR_ARG before any copy or launch.  nlist == 0: WR_OK,
 * nothing is launched. */
int wr_dev_plane_reorder_list(wr_ctx *ctx, unsigned char *d_dst, const unsigned char *d_src, int nx, int ny, int nz, int wlev,
                              unsigned brick, int inverse, const uint32_t *ids, size_t nlist);
/* how the reorder kernel walks a plane (host only: no device call, no context; the refusals of wr_dev_plane_reorder, and
 * out == NULL: WR_ERR_ARG; a refused call leaves *out alone).  A work item is `group` bricks that follow each other along x in
 * one box (128 / B of them; list != 0, a launch over a brick list: 1), `items` of them in all, over the `nbricks` bricks of
 * the plane's nbox boxes.  box[0, nbox) are the boxes in stream order, x, y, z: origin and extent in the coefficient array,
 * bricks per axis, `first` the box's first work item, `first_brick` the id of its first brick, `start` the stream position
 * of its first symbol; `wide`: the box moves 16 bytes per lane, otherwise a byte (planes aligned as the library's own always
 * are: B >= 16 and the box's origin and extent in x, nx and start all multiples of 16). */
typedef struct wr_reorder_plan_t {
    int group;
    uint32_t items, nbricks;
    int nbox;
    struct { int origin[3], extent[3], bricks[3]; uint32_t first, first_brick; uint64_t start; int wide; } box[29];
} wr_reorder_plan_t;
int wr_reorder_plan(int nx, int ny, int nz, int wlev, unsigned brick, int list, wr_reorder_plan_t *out);
/* whole path: wr_encode_host_seg / _f32 / wr_encode_device_seg with every plane as a WRS2 blob */
int wr_encode_host_seg_blocked(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                               int mz, const double *cutoffvec, unsigned seg, unsigned brick, wr_enc_info *info,
                               unsigned char *data_enc, size_t cap, wr_timings *tm);
int wr_encode_host_seg_blocked_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                   int mz, const double *cutoffvec, unsigned seg, unsigned brick, wr_enc_info *info,
                                   unsigned char *data_enc, size_t cap, wr_timings *tm);
int wr_encode_device_seg_blocked(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                 const double *cutoffvec, unsigned seg, unsigned brick, wr_enc_info *info,
                                 unsigned char *data_enc, size_t cap, wr_timings *tm);
/* host reference of the WRS2 format, on the calling thread: sym is the plane in NATURAL order (nx*ny*nz symbols), the
 * permutation is done here.  blob holds wr_seg_bound_blocked(n, seg) bytes; returns the blob's length (0: an argument was
 * refused).  The decoder reads a WRS1 blob too (wlev and brick are then not looked at). */
size_t wr_seg_encode_host_ref_blocked(const unsigned char *sym, int nx, int ny, int nz, int wlev, unsigned brick,
                                      unsigned seg, unsigned char *blob);
int wr_seg_decode_host_ref_blocked(const unsigned char *blob, size_t len, unsigned char *sym, int nx, int ny, int nz,
                                   int wlev);

/* ---- Stranded segments ("WRS3"): an opt-in fourth stream format -- short coder chains that share one model.
 * Everything is WRS1's (or, with a brick edge, WRS2's) -- transform, quantizer, header scalars, the rules for `seg`, the
 * symbol order -- except how a segment is coded.  A WRS1 segment is one chain of up to 59 999 dependent coder steps and carries
 * its own model of 256 counts (about 512 bytes), so a shorter chain used to mean a shorter segment and a model per chain.
 * WRS3 keeps the MODEL per segment and cuts the CHAIN: the segment's symbols are coded as K independent strands, each a complete
 * coder run over a contiguous K-th of the segment, all with the segment's one table.  A strand costs about ten bytes (a length
 * word, the start byte, the five bytes of the finish).  All fields little endian:
 *   plane blob := 'W','R','S','3' | u32 seg | u32 nseg | u32 brick | u32 strands | u32 len[nseg] | segment records, in order
 *   seg      as WRS1: a multiple of 16 in [16, 59999]; nseg = ceil(n / seg)
 *   brick    0: the natural (WRS1) symbol order; 8 / 16 / 32 / 64: the blocked (WRS2) order with that brick edge
 *   strands  K, one of 1, 2, 4, 8, 16, 32 with 16 * K <= seg.  strands = 0 in a call means WR_STRANDS_DEFAULT.
 *   L        the strand length, 16 * ceil(seg / (16 * K))
 * Segment k holds the bs stream positions [k*seg, k*seg + bs) of the (possibly permuted) plane, bs = min(seg, n - k*seg).
 * Strand j of it covers the segment's positions [j*L, min((j+1)*L, bs)); the first Kk = ceil(bs / L) strands are non-empty.
 *   record k := u32 tlen | u32 slen[K] | T | S_0 | ... | S_{Kk-1} | 0-3 zero bytes up to a multiple of 4
 * In terms of the range coder's calls (rangecod.c; csrc/wr_segcoder.h holds them as wrseg::Enc), with count_s the number of
 * times symbol s occurs in the whole segment and cum_s the sum of the counts below s:
 *   T    start_encoding(0); encode_short(count_s) for s = 0..255; done_encoding                       tlen bytes
 *   S_j  start_encoding(0); encode_freq(count_s, cum_s, bs) for each symbol s of strand j in order;
 *        encode_freq(1, 0, 2); done_encoding                                                            slen[j] bytes
 * slen[j] = 0 and no bytes for j >= Kk.  len[k] is the record's length including the padding; the header and the index are
 * 4-byte aligned, so every record and every slen array is.
 * Bounds (derived in csrc/wr_segcoder.h from the coder step): tlen <= 520, slen[j] <= 2 * L + 8, a record is at most
 * 4 * (K + 1) + 520 + K * (2 * L + 8) bytes.  WRS1's bound of about 1.03 bytes per symbol does NOT hold for a strand: a symbol
 * that is rare in its segment costs up to 16 bits wherever it stands.
 * Refused before anything is launched (WR_ERR_STREAM): what WRS1 / WRS2 refuse in a header or index, a strand count or brick
 * outside the lists above, a len[k] above the record bound or not a multiple of 4, planes of one stream that differ in
 * format, brick or strand count.  Refused per record, before a symbol of it is written, and counted in bad_segments:
 * len[k] < 4 * (K + 1); a slen[j] above its bound or non-zero for j >= Kk; tlen above its bound; round_up4(4 * (K + 1) + tlen
 * + sum slen) != len[k]; counts in T that do not sum to bs.  A strand whose run does not end with the zero flag is refused
 * after its symbols.  A strand decoder runs exactly its strand's symbol count of steps, reads zeros past slen[j], and writes
 * nothing outside its strand.
 * The wr_decode_*_seg, _seg_lowres and _seg_roi entry points and wr_dev_seg_decode read the magic and decode this format too
 * (wr_dev_seg_decode gives the symbols in stream order: permuted if brick != 0); segment lists, byte ranges and WR_STAT_*
 * counters are per segment exactly as for the same seg and order in WRS1 / WRS2.  Results are bit for bit those of the WRS1
 * stream of the same field. */
#define WR_STRANDS_DEFAULT 8
size_t wr_seg_bound_strands(size_t n, unsigned seg, unsigned strands); /* worst-case blob bytes of one plane; 0 if refused */
/* stage level, as wr_dev_seg_encode: the plane as it stands, brick = 0 in the header */
int wr_dev_seg_encode_strands(wr_ctx *ctx, const unsigned char *d_sym, size_t n, unsigned seg, unsigned strands,
                              unsigned char *d_blob, size_t cap, size_t *blob_len);
/* whole path: wr_encode_host_seg / _f32 / wr_encode_device_seg with every plane as a WRS3 blob.  brick = 0: the natural
 * order (no reorder pass); 8 / 16 / 32 / 64: the blocked order. */
int wr_encode_host_seg_strands(wr_ctx *ctx, const double *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                               int mz, const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands,
                               wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm);
int wr_encode_host_seg_strands_f32(wr_ctx *ctx, const float *h_fld, int nx, int ny, int nz, int wtflag, int mx, int my,
                                   int mz, const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands,
                                   wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm);
int wr_encode_device_seg_strands(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                 const double *cutoffvec, unsigned seg, unsigned brick, unsigned strands,
                                 wr_enc_info *info, unsigned char *data_enc, size_t cap, wr_timings *tm);
/* host reference of the WRS3 format, on the calling thread: sym is the plane in NATURAL order (nx*ny*nz symbols; with
 * brick = 0 only the product matters and wlev is not looked at, and a dimension may be 0).  blob holds
 * wr_seg_bound_strands(n, seg, strands) bytes; returns the blob's length (0: an argument was refused).
 * wr_seg_decode_host_ref_blocked reads WRS3 blobs too; wr_seg_decode_host_ref stays WRS1-only. */
size_t wr_seg_encode_host_ref_strands(const unsigned char *sym, int nx, int ny, int nz, int wlev, unsigned brick,
                                      unsigned seg, unsigned strands, unsigned char *blob);

/* ---- Batched segmented streams: plane l of N same-shaped fields in ONE coder launch.  No new format.
 * A plane's coder kernels take as long as one segment's chain, however few segments the plane has: a 128^3 plane is 36 lanes
 * of a device that holds tens of thousands.  A batch call codes plane index l of all its fields in one launch sequence, one
 * lane per segment of any field, so N small fields cost about one field's coder time.
 *   For every field of a batch, the header record and every byte of data_enc are exactly what the single-field call returns for
 *   that field alone -- wr_encode_host_seg with brick == 0, wr_encode_host_seg_blocked otherwise (brick != 0; there is no
 *   default here) -- whatever the other fields of the batch are and whatever their order.  A batched decode gives, bit for bit,
 *   what wr_decode_host_seg gives per field.  Either side may be mixed freely with the single-field calls.
 * All fields of a batch share nx, ny, nz, wtflag, mx, my, mz, seg and brick; each has its own cutoff vector (mx*my*mz entries),
 * its own wr_enc_info and its own output buffer of caps[i] bytes.  A decode batch may mix WRS1 and WRS2 fields.
 * Refused with WR_ERR_ARG: nfields outside 1..WR_SEG_BATCH_MAX, null arrays or entries, and a batch whose segments of one plane
 * index number 2^31 or more.  WR_ERR_UNSUPPORTED: a WRS3 field in a decode batch (strands are not batched), and a context with
 * wr_ctx_set_keep_residual(ctx, 1).  The first failing field decides the return code; wr_last_error() starts with
 * "field <index>: " and names the plane where there is one; the other fields' outputs are then unspecified.  On decode every
 * field's lengths, headers and indices are validated on the host BEFORE anything is copied or launched for any field, and no
 * dequantizer runs unless every segment of every field decoded.  Constant fields (nlay == 0) take part with no job.
 * wr_timings is one record for the call: `rangecoder` is the sum of the batched coder launches, plane_coder_s[l] the launch
 * sequence of plane index l; h2d_ms, d2h_ms, quant_ms and transform_ms are summed over the fields.
 * Device memory: beside one work-space slot a batch takes, from the plane pool (its accounting, cap and reserve),
 *   per (field, plane)   wr_plane_pitch(n) for the plane, the blob (encode: its bound rounded up to 16; decode: its length),
 *                        decode: the offsets and flags of its segments
 *   per field            brick != 0: wr_plane_pitch(n) for the plane in stream order
 *   once                 encode: the staging of one plane index (a region of the segment bound per segment of every field, the
 *                        scan's arrays, the job table); decode: a job table per plane index and the failure counts
 * wr_seg_batch_device_bytes is that sum for nfields fields of n samples and nlay planes each (host only; 0 for a refused
 * argument: nfields, n == 0, nlay outside 0..WR_NLAYMAX, seg, brick); it is the arithmetic the drivers allocate by, with every
 * blob at its bound.  A batch the pool cannot hold fails with the pool's error before the first coder launch. */
#define WR_SEG_BATCH_MAX 1024
size_t wr_seg_batch_device_bytes(int nfields, size_t n, int nlay, unsigned seg, unsigned brick, int decode);
/* the locator of the batched kernels (csrc/wr_segbatch.h), for tests: first[0 .. njobs] is the exclusive prefix of the jobs'
 * segment counts; lane g < first[njobs] is segment *k of job *job.  WR_ERR_ARG: a prefix that does not start at 0 or
 * decreases, njobs outside 1..WR_SEG_BATCH_MAX, g past the end. */
int wr_seg_batch_locate(const uint32_t *first, uint32_t njobs, uint32_t g, uint32_t *job, uint32_t *k);
/* stage level, device pointers (16-byte aligned): njobs planes of n symbols each in one launch sequence.  Every blob equals
 * wr_dev_seg_encode's for that plane; errors as in the single-plane calls, the first failing job deciding ("job <index>: ").
 * blob_len[j] is set for every job that was coded, bad_segments[j] (may be NULL) for every job that was decoded. */
int wr_dev_seg_encode_batch(wr_ctx *ctx, int njobs, const unsigned char *const *d_sym, size_t n, unsigned seg,
                            unsigned char *const *d_blob, const size_t *cap, size_t *blob_len);
int wr_dev_seg_decode_batch(wr_ctx *ctx, int njobs, const unsigned char *const *d_blob, const size_t *blob_len,
                            unsigned char *const *d_sym, size_t n, size_t *bad_segments);
/* whole path */
int wr_encode_host_seg_batch(wr_ctx *ctx, int nfields, const double *const *h_flds, int nx, int ny, int nz, int wtflag,
                             int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg, unsigned brick,
                             wr_enc_info *infos, unsigned char *const *data_encs, const size_t *caps, wr_timings *tm);
int wr_decode_host_seg_batch(wr_ctx *ctx, int nfields, double *const *h_flds, int nx, int ny, int nz,
                             const wr_enc_info *infos, const unsigned char *const *data_encs, const size_t *data_lens,
                             wr_timings *tm);
int wr_encode_host_seg_batch_f32(wr_ctx *ctx, int nfields, const float *const *h_flds, int nx, int ny, int nz, int wtflag,
                                 int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg, unsigned brick,
                                 wr_enc_info *infos, unsigned char *const *data_encs, const size_t *caps,
                                 wr_timings *tm);
int wr_decode_host_seg_batch_f32(wr_ctx *ctx, int nfields, float *const *h_flds, int nx, int ny, int nz,
                                 const wr_enc_info *infos, const unsigned char *const *data_encs,
                                 const size_t *data_lens, wr_timings *tm);
/* device fields (consumed by an encode, as wr_encode_device_seg's) */
int wr_encode_device_seg_batch(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz, int wtflag,
                               int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg, unsigned brick,
                               wr_enc_info *infos, unsigned char *const *data_encs, const size_t *caps, wr_timings *tm);
int wr_decode_device_seg_batch(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz,
                               const wr_enc_info *infos, const unsigned char *const *data_encs,
                               const size_t *data_lens, wr_timings *tm);

/* ---- Batch calls for WRS3: stranded fields in the batched coder launches.  No new format.
 * The calls above keep their contract (a WRS3 field is WR_ERR_UNSUPPORTED there); the ones here take strands.
 * Encode: wr_encode_*_seg_batch_strands is wr_encode_*_seg_batch with `strands` after `brick`, in the place it has in
 *   wr_encode_host_seg_strands: strands = 0 means WR_STRANDS_DEFAULT, brick = 0 the natural order.  For every field, the header
 *   record and every byte of data_enc are exactly what wr_encode_host_seg_strands (_f32, wr_encode_device_seg_strands) returns
 *   for that field alone with the same seg, brick and strands.  Plane index l of all fields is one launch sequence, strands
 *   lanes per segment of any field.  Refused with WR_ERR_ARG beside the refusals above: a seg / brick / strands combination
 *   the single call refuses, and a batch whose strands of one plane index number 2^31 or more.
 * Decode: wr_decode_*_seg_batch_mixed is wr_decode_*_seg_batch for any mix of WRS1, WRS2 and WRS3 fields; brick edge, seg,
 *   strands, tolerance and plane count may differ per field, constant fields take part without a job.  Every reconstruction is
 *   bit for bit wr_decode_host_seg's.  Every (field, plane) of the call is a job of its own: the WRS1 / WRS2 jobs go into one
 *   coder launch and the WRS3 jobs into another -- at most two launches per call while neither kind has more than
 *   WR_SEG_BATCH_MAX jobs, further launches of at most WR_SEG_BATCH_MAX jobs each beyond that.  Validation, refusals and error
 *   texts are those of wr_decode_host_seg_batch (every stream is parsed on the host before anything is copied or launched; a
 *   failed segment is WR_ERR_STREAM naming field and plane before any dequantizer runs), except that a launch, not a plane
 *   index, is what must stay below 2^31 lanes.  wr_timings: `rangecoder` and plane_coder_s[0] are the call's coder launches.
 * Device memory: as above, with the blob at wr_seg_bound_strands, and
 *   encode, once         the staging of one plane index at the record's stride: 520 + K (2 L + 8) bytes per segment of every
 *                        field (L = the strand length), about 2.0 n per plane where WRS1 takes 1.07 n
 *   decode, per job      brick != 0: wr_plane_pitch(n) for the plane in stream order (all jobs are in flight at once)
 *   decode, once         a job table per launch and the failure counts
 * wr_seg_batch_device_bytes_strands is that sum (strands = 0: WR_STRANDS_DEFAULT; 0 for a refused argument: those of
 * wr_seg_batch_device_bytes, and strands not one of 1, 2, 4, 8, 16, 32 or 16 * strands > seg); it never decreases when
 * nfields, n or nlay grows. */
size_t wr_seg_batch_device_bytes_strands(int nfields, size_t n, int nlay, unsigned seg, unsigned brick, unsigned strands,
                                         int decode);
/* the lane layout of the batched strand ENCODER (csrc/wr_segbatch.h), for tests: all jobs share `strands` (one of 1, 2, 4, 8,
 * 16, 32), first[0 .. njobs] is the exclusive prefix of the jobs' segment counts, and lane g of the grid is strand
 * g & (strands - 1) of launch segment g / strands, which is segment *segment of job *job.  Returns 1, or 0 for a lane past the
 * end (g / strands >= first[njobs]: nothing is written, and it is no error); WR_ERR_ARG for refused arguments (a null pointer,
 * njobs outside 1..WR_SEG_BATCH_MAX, such a strand count, a prefix that does not start at 0 or decreases).
 * The batched strand DECODER's layout is wr_seg_lists_lanes with nlist[j] = the segments of job j. */
int wr_seg_batch_strand_lane(const uint32_t *first, uint32_t njobs, unsigned strands, unsigned long long g, uint32_t *job,
                             uint32_t *segment, uint32_t *strand);
/* stage level, device pointers (16-byte aligned).  Encode: njobs planes of n symbols each as WRS3 blobs in the natural order
 * (strands = 0: WR_STRANDS_DEFAULT) in one launch sequence; every blob equals wr_dev_seg_encode_strands' for that plane.  A
 * blob buffer too small for its blob is WR_ERR_OVERFLOW naming the job, with the other jobs complete.  Decode: njobs WRS1, WRS2
 * and WRS3 blobs of planes of n symbols, the plain jobs in one launch and the stranded ones in another; the symbols come out
 * in stream order, as with wr_dev_seg_decode_lists_mixed.  Every header and index is validated on the host first: a malformed
 * one in job j is WR_ERR_STREAM with "job j" and nothing is launched.  A segment or record that does not decode on the device
 * is counted in bad_segments[j] (may be NULL) and the call returns WR_ERR_STREAM naming the first such job. */
int wr_dev_seg_encode_batch_strands(wr_ctx *ctx, int njobs, const unsigned char *const *d_sym, size_t n, unsigned seg,
                                    unsigned strands, unsigned char *const *d_blob, const size_t *cap, size_t *blob_len);
int wr_dev_seg_decode_batch_mixed(wr_ctx *ctx, int njobs, const unsigned char *const *d_blob, const size_t *blob_len,
                                  unsigned char *const *d_sym, size_t n, size_t *bad_segments);
/* whole path */
int wr_encode_host_seg_batch_strands(wr_ctx *ctx, int nfields, const double *const *h_flds, int nx, int ny, int nz,
                                     int wtflag, int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg,
                                     unsigned brick, unsigned strands, wr_enc_info *infos, unsigned char *const *data_encs,
                                     const size_t *caps, wr_timings *tm);
int wr_encode_host_seg_batch_strands_f32(wr_ctx *ctx, int nfields, const float *const *h_flds, int nx, int ny, int nz,
                                         int wtflag, int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg,
                                         unsigned brick, unsigned strands, wr_enc_info *infos,
                                         unsigned char *const *data_encs, const size_t *caps, wr_timings *tm);
int wr_encode_device_seg_batch_strands(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz, int wtflag,
                                       int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg,
                                       unsigned brick, unsigned strands, wr_enc_info *infos,
                                       unsigned char *const *data_encs, const size_t *caps, wr_timings *tm);
int wr_decode_host_seg_batch_mixed(wr_ctx *ctx, int nfields, double *const *h_flds, int nx, int ny, int nz,
                                   const wr_enc_info *infos, const unsigned char *const *data_encs,
                                   const size_t *data_lens, wr_timings *tm);
int wr_decode_host_seg_batch_mixed_f32(wr_ctx *ctx, int nfields, float *const *h_flds, int nx, int ny, int nz,
                                       const wr_enc_info *infos, const unsigned char *const *data_encs,
                                       const size_t *data_lens, wr_timings *tm);
int wr_decode_device_seg_batch_mixed(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz,
                                     const wr_enc_info *infos, const unsigned char *const *data_encs,
                                     const size_t *data_lens, wr_timings *tm);

/* ---- Masked batch encode and decode: N masked fields per call, their N masks in one coder launch.  No new format.
 * A loop of wr_encode_*_seg_masked pays, per field, a coder launch per plane and one more for the mask, each as long as one
 * segment's chain; here the planes go as in the batch calls above and all masks as one launch more.
 * Encode.  wr_encode_*_seg_batch_masked take the arguments of wr_encode_*_seg_batch_strands, `below` (one threshold per call;
 *   a NaN is WR_ERR_ARG) behind `strands`, and results[0, nfields) (may be NULL) at the end.  The format is chosen as the single
 *   masked call chooses it and nothing is defaulted but seg: brick == 0 && strands == 0: WRS1; brick != 0: WRS2; strands != 0:
 *   WRS3.  For every field f, infos[f], every byte of data_encs[f] -- the field part, then the WRM1 blob at infos[f].ntot_enc --
 *   and results[f].undefined, .pad, .mask_len are exactly what wr_encode_*_seg_masked returns for that field alone with the
 *   same seg, brick, strands and below, whatever the other fields are and whatever their order.  A field without an undefined
 *   sample gives the plain batch record (mask_len == 0); a padded field that is constant gives the trivial record with the
 *   blob at data_enc.  Device fields are split by one launch and filled by one launch before the first transform (the fields
 *   are consumed); a host field is split and filled in the slot as it passes through.  Before a field's transform is queued:
 *   no defined sample is WR_ERR_ARG "field f: no defined sample: ...", a mean that is not finite WR_ERR_ARG likewise.  The masks
 *   of all fields that have an undefined sample are coded by ONE launch of the batched WRS1 coder, ceil(n / 8) symbols each at
 *   the call's seg, on a stream of their own under the fields' plane launches: WR_STAT_BATCH_CODER_LAUNCHES grows by the plane
 *   launches plus 1 (plus 0 when no field has an undefined sample).  caps[f] must hold the field part plus the blob's exact
 *   length: WR_ERR_OVERFLOW naming the field otherwise, before data_encs[f] is written (earlier fields are complete).
 *   results[f].mask_coder_ms is the one mask launch's time in every masked field; split_ms and fill_ms are the field's own for
 *   host fields and the batched launches' for device fields.
 * Decode.  wr_decode_*_seg_batch_masked take the arguments of wr_decode_*_seg_batch_mixed (data_lens is required), `fill` and
 *   results[0, nfields) (may be NULL).  data_lens[f] is the field part plus the blob; data_lens[f] == infos[f].ntot_enc, or 0, is
 *   an unmasked record.  WRS1, WRS2 and WRS3 field parts, masked, unmasked and constant records (a constant with or without a
 *   blob) may share a call; every reconstruction is bit for bit wr_decode_*_seg_masked's for that record alone, a NaN `fill`
 *   included.  Every blob is validated on the host before anything is copied or launched; each mask is one more WRS1 job of
 *   the call's plain launch, so the call still makes at most two coder launches; one launch behind the coder stage counts every
 *   mask.  WR_ERR_STREAM naming "field f: ", before any dequantizer runs and before any caller's field is written: a malformed
 *   blob, a segment that does not decode, a set bit at or beyond n, a population count other than the header's.  results[f]:
 *   undefined, pad and mask_len as the single call gives them, mask_coder_ms the call's coder launches; the fills are not timed.
 * Stage level (device pointers of any alignment, n >= 1, 1..WR_SEG_BATCH_MAX fields or masks).  Field f's results are those of
 *   wr_dev_mask_split / wr_dev_mask_fill for that field alone, bit for bit (pad is a NaN for a field with no defined sample; the
 *   call still succeeds); a NULL d_flds[f] of a fill is skipped.  wr_dev_mask_check_batch reads no field: undefined[m] = the set
 *   bits of mask m's ceil(n / 8) bytes, beyond[m] = 1 if one lies at or beyond n.  WR_ERR_ARG: null arrays or entries, n == 0,
 *   a count out of range, a NaN `below`.
 * Device memory: wr_seg_batch_device_bytes_masked is wr_seg_batch_device_bytes_strands (an encode with strands == 0:
 *   wr_seg_batch_device_bytes, the WRS1 / WRS2 planes that call makes) plus
 *   per masked field     the bit plane; the blob, at its bound (encode) or at wr_mask_bound with the decoder's work buffer (decode)
 *   once, encode         the mask launch's staging, and the split partials of nfields fields
 *   once, decode         the masks' share of the job tables and failure counts, and the check's counters
 *   An encode cannot know nmasked in advance and holds a bit plane for every field: callers pass nfields.  0 for a refused
 *   argument (those of the base, nmasked outside 0..nfields); it never decreases when nfields, nmasked, n or nlay grows (seg,
 *   brick, strands and decode choose a layout; they are no measure of the work). */
size_t wr_seg_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int nlay, unsigned seg, unsigned brick,
                                        unsigned strands, int decode);
int wr_dev_mask_split_batch(wr_ctx *ctx, int nfields, const double *const *d_flds, size_t n, double below,
                            unsigned char *const *d_bits, unsigned long long *undefined, double *pad);
int wr_dev_mask_split_batch_f32(wr_ctx *ctx, int nfields, const float *const *d_flds, size_t n, double below,
                                unsigned char *const *d_bits, unsigned long long *undefined, double *pad);
int wr_dev_mask_fill_batch(wr_ctx *ctx, int nfields, double *const *d_flds, size_t n, const unsigned char *const *d_bits,
                           const double *values);
int wr_dev_mask_fill_batch_f32(wr_ctx *ctx, int nfields, float *const *d_flds, size_t n,
                               const unsigned char *const *d_bits, const double *values);
int wr_dev_mask_check_batch(wr_ctx *ctx, int nmasks, const unsigned char *const *d_bits, size_t n,
                            unsigned long long *undefined, unsigned char *beyond);
int wr_encode_host_seg_batch_masked(wr_ctx *ctx, int nfields, const double *const *h_flds, int nx, int ny, int nz, int wtflag,
                                    int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg, unsigned brick,
                                    unsigned strands, double below, wr_enc_info *infos, unsigned char *const *data_encs,
                                    const size_t *caps, wr_timings *tm, wr_mask_result *results);
int wr_encode_host_seg_batch_masked_f32(wr_ctx *ctx, int nfields, const float *const *h_flds, int nx, int ny, int nz,
                                        int wtflag, int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg,
                                        unsigned brick, unsigned strands, double below, wr_enc_info *infos,
                                        unsigned char *const *data_encs, const size_t *caps, wr_timings *tm,
                                        wr_mask_result *results);
int wr_encode_device_seg_batch_masked(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz, int wtflag,
                                      int mx, int my, int mz, const double *const *cutoffvecs, unsigned seg, unsigned brick,
                                      unsigned strands, double below, wr_enc_info *infos, unsigned char *const *data_encs,
                                      const size_t *caps, wr_timings *tm, wr_mask_result *results);
int wr_decode_host_seg_batch_masked(wr_ctx *ctx, int nfields, double *const *h_flds, int nx, int ny, int nz,
                                    const wr_enc_info *infos, const unsigned char *const *data_encs, const size_t *data_lens,
                                    double fill, wr_timings *tm, wr_mask_result *results);
int wr_decode_host_seg_batch_masked_f32(wr_ctx *ctx, int nfields, float *const *h_flds, int nx, int ny, int nz,
                                        const wr_enc_info *infos, const unsigned char *const *data_encs,
                                        const size_t *data_lens, double fill, wr_timings *tm, wr_mask_result *results);
int wr_decode_device_seg_batch_masked(wr_ctx *ctx, int nfields, double *const *d_flds, int nx, int ny, int nz,
                                      const wr_enc_info *infos, const unsigned char *const *data_encs, const size_t *data_lens,
                                      double fill, wr_timings *tm, wr_mask_result *results);

/* ---- Region decode, many regions per call: Q regions of one stream, and all used planes in ONE coder launch.  No new format.
 * A single-region call launches the coder once per used plane, back to back, and each launch lasts one segment's chain however
 * few lanes it has; Q probes of one snapshot pay that Q times.  Here the segments that any of the regions needs -- per plane the
 * ascending UNION of the regions' lists for that plane's `seg` -- are uploaded and decoded once, on a WRS1 / WRS2 stream by one
 * launch over all used planes (a job per plane, a lane per listed segment: csrc/wr_segbatch.hip), on a WRS3 stream by one
 * launch per plane over the union.  Then the regions are finished one after another as the single-region call finishes its
 * one: window dequantiser, inverse on the window, crop and scale.
 *   rois[0, nroi), 1 <= nroi <= WR_ROI_MULTI_MAX, are boxes in the coordinates of D(r, p) as above; one level and one
 *   max_planes hold for the call; regions may overlap or repeat.  The output is ONE contiguous buffer: region i lies at element
 *   offset offs[i] of wr_roi_multi_elems (the exclusive prefix of the regions' element counts) and is, bit for bit, what
 *   wr_decode_host_seg_roi (the _f32 form: wr_decode_host_seg_roi_f32) returns for rois[i] alone.
 * Order of validation: the plan of every region first -- the first bad region gives WR_ERR_ARG and wr_last_error() starts with
 * "region <index>: " --, then every plane's header and index, used or not, as by wr_decode_host_seg; nothing is copied or
 * launched before both have passed.  A constant field gives midval in every region.  The per-plane counts of segments that did
 * not decode come back once; any non-zero count is WR_ERR_STREAM naming the plane, before a dequantiser runs.
 * A blocked stream takes one stream-order scratch plane per used plane from the plane pool (the single-region call reuses one);
 * a host caller's crops are gathered in one pool buffer of the total size and come down in one copy.
 * WR_STAT_ROI_SEGMENTS moves by the union's size summed over the used planes, WR_STAT_ROI_BYTES_UP by the union's stream bytes,
 * WR_STAT_ROI_CODER_LAUNCHES by 1 (WRS1 / WRS2) or by the used planes (WRS3).  wr_timings: `rangecoder` is the coder launch(es);
 * on the one-launch path plane_coder_s[0] is that time and the other entries are 0; quant_ms and transform_ms are summed over
 * the regions (the call then waits for every region's kernels before it queues the next one's).
 * The single-region entry points are unchanged; a caller who wants one launch for one region passes nroi = 1. */
#define WR_ROI_MULTI_MAX 1024
/* host only.  offs[0 .. nroi] (may be NULL): the exclusive prefix of the regions' element counts; returns the total, or 0 for a
 * refused argument (nroi outside 1..WR_ROI_MULTI_MAX, null rois, a level outside [0, 4], an empty or out-of-range box). */
size_t wr_roi_multi_elems(int nx, int ny, int nz, int level, const wr_box *rois, int nroi, size_t *offs);
/* host only.  The ascending union of what wr_seg_roi_segments (brick == 0) or wr_seg_roi_segments_blocked (brick != 0) lists
 * per region; their conventions (the count of the whole union is returned, at most cap ids are written, 0: refused). */
size_t wr_seg_roi_segments_multi(int nx, int ny, int nz, int level, int wlev, const wr_box *rois, int nroi,
                                 unsigned brick, unsigned seg, uint32_t *ids, size_t cap);
/* stage level, as wr_dev_decode_planes_roi (the window stage only): d_out receives wr_roi_multi_elems elements */
int wr_dev_decode_planes_roi_multi(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                                   const wr_box *rois, int nroi, const unsigned char *d_planes, const wr_enc_info *info);
/* stage level, for tests of the kernel: njobs (1..WR_SEG_BATCH_MAX) WRS1 / WRS2 blobs in device memory, job j a plane of n[j]
 * symbols of which the segments ids[j][0, nlist[j]) -- HOST arrays, ascending, below the blob's segment count; nlist[j] may be
 * 0 -- are decoded by one launch into d_sym[j] (stream order for a WRS2 blob).  Device pointers are 16-byte aligned.  Every
 * header, index and list is validated on the host before the launch (WR_ERR_STREAM / WR_ERR_ARG, "job <index>: "); only listed
 * segments are read and written.  bad_segments[j] (may be NULL): the job's segments that did not decode (WR_ERR_STREAM). */
int wr_dev_seg_decode_lists(wr_ctx *ctx, int njobs, const unsigned char *const *d_blob, const size_t *blob_len,
                            unsigned char *const *d_sym, const size_t *n, const uint32_t *const *ids, const size_t *nlist,
                            size_t *bad_segments);
/* whole path: wr_decode_host_seg_roi / _f32 / wr_decode_device_seg_roi with rois, nroi in place of roi */
int wr_decode_host_seg_roi_multi(wr_ctx *ctx, double *h_out, int nx, int ny, int nz, int level, int max_planes,
                                 const wr_box *rois, int nroi, const wr_enc_info *info, const unsigned char *data_enc,
                                 size_t data_len, wr_timings *tm);
int wr_decode_host_seg_roi_multi_f32(wr_ctx *ctx, float *h_out, int nx, int ny, int nz, int level, int max_planes,
                                     const wr_box *rois, int nroi, const wr_enc_info *info, const unsigned char *data_enc,
                                     size_t data_len, wr_timings *tm);
int wr_decode_device_seg_roi_multi(wr_ctx *ctx, double *d_out, int nx, int ny, int nz, int level, int max_planes,
                                   const wr_box *rois, int nroi, const wr_enc_info *info, const unsigned char *data_enc,
                                   size_t data_len, wr_timings *tm);

/* ---- Region decode across a batch of fields: the regions of N same-shaped fields, and at most TWO coder launches per call.
 * The many-region call above works on one coded field; a probe's time history or the same slice of every snapshot loops over
 * the fields and pays one coder launch -- one segment's chain -- per field (WRS3: per field and plane).  Here a job is one
 * (non-constant field, used plane) with the union of the segments the regions need, as the many-region call lists it; the
 * jobs of all WRS1 / WRS2 fields go into one launch and those of all WRS3 fields into a second one (csrc/wr_segbatch.hip:
 * k_seg_decode_list_batch, k_strand_decode_list_batch).  Then every field's regions are finished as the many-region call
 * finishes them.  No new format.
 *   All fields have the shape nx, ny, nz; one level, one max_planes and one region list rois[0, nroi), 1 <= nroi <=
 *   WR_ROI_MULTI_MAX, hold for the call.  The fields may differ in tolerance, plane count, wlev, seg, brick and strands, and
 *   WRS1, WRS2 and WRS3 fields may be mixed.  With T = wr_roi_multi_elems(nx, ny, nz, level, rois, nroi, offs) the output is
 *   ONE contiguous buffer of nfields * T elements: region i of field f lies at element f * T + offs[i] and is, bit for bit,
 *   what wr_decode_host_seg_roi_multi (the _f32 form: ..._f32) returns for field f alone with the same arguments.  A region
 *   that is the whole box of the level makes this the batched low-resolution decode.  Constant fields take part with no job;
 *   as in the per-field call, max_planes may not exceed a field's plane count, so a constant field (no planes) together with
 *   max_planes > 0 is WR_ERR_ARG ("field <f>: region 0: ").
 * Refused with WR_ERR_ARG before anything is copied or launched: nfields < 1, a null array, more than WR_SEG_BATCH_MAX jobs,
 * a launch of 2^31 lanes or more.  Order of validation: every field's region plans against that field's own record -- the
 * first failure gives its code and a text starting "field <f>: region <i>: " --, then every field's stream, every plane's
 * header and index, used or not ("field <f>: ").  The first failing field decides the return code.  The per-job counts of
 * segments that did not decode come back once; a non-zero count is WR_ERR_STREAM naming field and plane, before any
 * dequantiser runs, and the output buffer is then untouched.
 * WR_STAT_ROI_SEGMENTS moves by the listed segments summed over all jobs, WR_STAT_ROI_BYTES_UP by the stream bytes uploaded,
 * WR_STAT_ROI_CODER_LAUNCHES by the launches made: 0, 1 or 2.  wr_timings is one record for the call: `rangecoder` is the
 * coder launches, plane_coder_s[0] carries that time and the other entries are 0; quant_ms and transform_ms are summed over
 * fields and regions.
 * Device memory, from the plane pool beside one work-space slot:
 *   per job     wr_plane_pitch(n) for the plane (full pitch, sparsely filled), the blob's length, the offsets, flags and list
 *               of its segments; a WRS2 job: wr_plane_pitch(n) for the plane in stream order
 *   per field   WRS2: its brick list
 *   once        the two job tables, a failure count per job; a host caller: the output, nfields * T elements, one copy down
 * wr_seg_roi_batch_device_bytes is an upper bound of that sum for nfields fields of n samples with `planes` used planes each
 * (host only; every blob at its bound, every list at the plane's segment count, the brick list at n entries; strands != 0:
 * WRS3 fields; out_elems: T for a host caller, 0 for a device caller).  0 for a refused argument: nfields < 1, n == 0, planes
 * outside 0..WR_NLAYMAX, seg, brick, strands, nfields * planes above WR_SEG_BATCH_MAX.  The call does not split a batch: one
 * that does not get its memory fails with the pool's error before the coder launch. */
size_t wr_seg_roi_batch_device_bytes(int nfields, size_t n, int planes, unsigned seg, unsigned brick, unsigned strands,
                                     size_t out_elems);
/* the free memory of the context's device in bytes, as the runtime reports it now (0: it could not be asked); what a caller
 * holds wr_seg_roi_batch_device_bytes against when it cuts a long series of fields into calls.  Idle buffers of the library's
 * own pools count as used, so it is a lower bound of what a call can get. */
size_t wr_ctx_device_free_bytes(wr_ctx *ctx);
/* host only: the lane layout of a launch over lists (csrc/wr_segbatch.h).  Job j decodes nlist[j] segments; strands[j] == 0: a
 * WRS1 / WRS2 job of nlist[j] lanes, no padding; strands[j] == K: a WRS3 job of nlist[j] * K lanes ROUNDED UP to a multiple
 * of 64, lane r of it being strand r & (K - 1) of list position r / K (a position >= nlist[j]: padding).  first[0 .. njobs]
 * (may be NULL): the exclusive prefix of the jobs' lanes, as wr_seg_batch_locate takes it.  strands == NULL: all 0.  Returns
 * the lanes of the launch, or 0 if refused (njobs outside 1..WR_SEG_BATCH_MAX, null nlist, a strand count that is not 0, 1, 2,
 * 4, 8, 16 or 32, 2^31 lanes or more; wr_last_error() says which) -- and 0 with first[] all zeros if every list is empty. */
size_t wr_seg_lists_lanes(int njobs, const size_t *nlist, const unsigned *strands, uint32_t *first);
/* stage level, for tests of the kernels: wr_dev_seg_decode_lists that also accepts WRS3 blobs (strands and brick are read from
 * each header after host validation; a WRS3 blob's symbols come out in stream order).  The WRS1 / WRS2 jobs go through one
 * kernel and the WRS3 jobs through the other, whatever their order in the call. */
int wr_dev_seg_decode_lists_mixed(wr_ctx *ctx, int njobs, const unsigned char *const *d_blob, const size_t *blob_len,
                                  unsigned char *const *d_sym, const size_t *n, const uint32_t *const *ids,
                                  const size_t *nlist, size_t *bad_segments);
/* whole path: h_out / d_out receive nfields * T elements */
int wr_decode_host_seg_roi_batch(wr_ctx *ctx, double *h_out, int nfields, int nx, int ny, int nz, int level, int max_planes,
                                 const wr_box *rois, int nroi, const wr_enc_info *infos,
                                 const unsigned char *const *data_encs, const size_t *data_lens, wr_timings *tm);
int wr_decode_host_seg_roi_batch_f32(wr_ctx *ctx, float *h_out, int nfields, int nx, int ny, int nz, int level,
                                     int max_planes, const wr_box *rois, int nroi, const wr_enc_info *infos,
                                     const unsigned char *const *data_encs, const size_t *data_lens, wr_timings *tm);
int wr_decode_device_seg_roi_batch(wr_ctx *ctx, double *d_out, int nfields, int nx, int ny, int nz, int level,
                                   int max_planes, const wr_box *rois, int nroi, const wr_enc_info *infos,
                                   const unsigned char *const *data_encs, const size_t *data_lens, wr_timings *tm);

/* ---- Masked region decode across a batch of fields: the call above on records that wr_encode_*_seg_masked wrote, the
 * undefined samples of every region coming back as `fill`.  No new format and no new error code.  Arguments and output layout
 * are those of wr_decode_host_seg_roi_batch; data_lens[f] is the length of field f's planes PLUS its mask blob, as for
 * wr_decode_host_seg_roi_masked, and data_lens[f] == infos[f].ntot_enc (or 0) marks an unmasked record.  Masked and unmasked
 * records, WRS1 / WRS2 / WRS3 field parts and constant fields may be mixed; nfields = 1 is the masked many-region call.
 *   Region i of field f is bit for bit what wr_decode_host_seg_roi_masked (_f32, the device form) returns for rois[i] of that
 *   record alone with the same level, max_planes and fill ((float)fill for fp32 output; a NaN fill is allowed); for an
 *   unmasked record it is the plain batch call's, and res[f] is zeroed.  A constant padded field with a blob (nlay == 0, the
 *   blob at data_encs[f]) gives midval with fill restored, for a host caller too.
 * Coder launches.  A masked field adds ONE job to the call's WRS1 / WRS2 launch, whatever the format of its field part: its
 * blob, a plane of ceil(n / 8) symbols cut at the seg of the blob's own header, with the ascending union over the regions of
 * wr_mask_roi_segments listed (wr_mask_roi_segments_multi).  The call still makes at most two launches (a batch of WRS3 fields
 * with masks makes two: strands and masks) and nothing runs on a second stream.  Then the window stage as above, and ONE
 * launch of k_mask_restore_boxes (csrc/wr_mask.hip) over every (masked field, region) box of the output buffer.
 * res (nfields records, may be NULL): undefined = the set bits among field f's regions, summed over the regions (a sample in
 * two overlapping regions counts twice: the sum of the single calls' values); pad and mask_len as in the full masked decode;
 * fill_ms the call's one restore launch (HIP events; the same value in every masked record); mask_coder_ms and split_ms 0: the
 * mask jobs ride in the fields' launch and their time is in tm->rangecoder.
 * Validation, all of it before anything is copied or launched: every field's region plans ("field <f>: region <i>: "), every
 * field's stream, every plane's header and index, then every blob's header and whole segment index as the single masked call
 * validates them ("field <f>: mask blob: ...", WR_ERR_STREAM).  WR_ERR_ARG: more than WR_SEG_BATCH_MAX jobs, mask jobs
 * counted; a coder launch of 2^31 lanes or more; a restore launch of 2^31 turns or more.  After the launch a listed segment of
 * a field part ("field <f>: plane <l>: ") or of a mask ("field <f>: mask blob: ") that did not decode is WR_ERR_STREAM before
 * any dequantiser runs, the caller's output untouched.  As in the single call, the population count against the header and the
 * unused high bits of the last symbol are not checked, and damage in an unlisted mask segment does not fail the call.
 * WR_STAT_MASK_ROI_SEGMENTS moves by the listed mask segments summed over the fields, WR_STAT_MASK_ROI_BYTES_UP by their
 * stream bytes; WR_STAT_ROI_SEGMENTS / _BYTES_UP count the field parts only; WR_STAT_ROI_CODER_LAUNCHES moves by 0, 1 or 2.
 * wr_seg_roi_batch_device_bytes_masked: wr_seg_roi_batch_device_bytes plus, per masked field, a job on ceil(n / 8) symbols (the
 * plane at its pitch, the blob at wr_mask_bound(n, mask_seg), the job's offsets, flags and list) and once the restore's table
 * (sized for WR_ROI_MULTI_MAX regions); 0 for a refused argument, also nmasked outside 0..nfields and nfields * planes +
 * nmasked above WR_SEG_BATCH_MAX; with nmasked == 0 it is the plain function.  An upper bound of what the driver takes from the
 * plane pool, which allocates by the same arithmetic.
 * wr_mask_roi_segments_multi (host only): the ascending union of wr_mask_roi_segments over the regions, with its conventions.
 * wr_mask_boxes_turns (host only): the turns of the restore launch for one field's regions -- a turn is 64 consecutive x of one
 * region row, region i has ceil(cx / 64) * cy * cz --, first[0 .. nroi] (may be NULL) their exclusive prefix; 0 for an argument
 * that wr_roi_multi_elems refuses and for 2^31 turns or more.
 * wr_dev_mask_restore_boxes (stage level; device pointers of any alignment): wr_dev_mask_restore_box on d_out + f * T + offs[i]
 * for every f with d_bits[f] != NULL (a HOST array of nfields device pointers) and every i, in one launch; a field without a
 * plane is left untouched and its count is 0.  undefined: nfields counts, may be NULL. */
size_t wr_seg_roi_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int planes, unsigned seg, unsigned brick,
                                            unsigned strands, unsigned mask_seg, size_t out_elems);
size_t wr_mask_roi_segments_multi(int nx, int ny, int nz, int level, const wr_box *rois, int nroi, unsigned seg,
                                  uint32_t *ids, size_t cap);
size_t wr_mask_boxes_turns(int nx, int ny, int nz, int level, const wr_box *rois, int nroi, uint32_t *first);
int wr_dev_mask_restore_boxes(wr_ctx *ctx, double *d_out, int nfields, int nx, int ny, int nz, int level,
                              const wr_box *rois, int nroi, const unsigned char *const *d_bits, double fill,
                              unsigned long long *undefined);
int wr_dev_mask_restore_boxes_f32(wr_ctx *ctx, float *d_out, int nfields, int nx, int ny, int nz, int level,
                                  const wr_box *rois, int nroi, const unsigned char *const *d_bits, double fill,
                                  unsigned long long *undefined);
int wr_decode_host_seg_roi_batch_masked(wr_ctx *ctx, double *h_out, int nfields, int nx, int ny, int nz, int level,
                                        int max_planes, const wr_box *rois, int nroi, const wr_enc_info *infos,
                                        const unsigned char *const *data_encs, const size_t *data_lens, double fill,
                                        wr_timings *tm, wr_mask_result *res);
int wr_decode_host_seg_roi_batch_masked_f32(wr_ctx *ctx, float *h_out, int nfields, int nx, int ny, int nz, int level,
                                            int max_planes, const wr_box *rois, int nroi, const wr_enc_info *infos,
                                            const unsigned char *const *data_encs, const size_t *data_lens, double fill,
                                            wr_timings *tm, wr_mask_result *res);
int wr_decode_device_seg_roi_batch_masked(wr_ctx *ctx, double *d_out, int nfields, int nx, int ny, int nz, int level,
                                          int max_planes, const wr_box *rois, int nroi, const wr_enc_info *infos,
                                          const unsigned char *const *data_encs, const size_t *data_lens, double fill,
                                          wr_timings *tm, wr_mask_result *res);

/* ---- The stream format of the drop-in symbols: which of the four formats the implicit-context ENCODERS write.
 * encoding_wrap, encoding_wrap_f and wr_encoding_wrap_f32 write the reference's stream unless this process-wide setting says
 * otherwise; then they run wr_encode_host_seg / _seg_blocked / _seg_strands (the _f32 forms) with the setting's parameters.
 * Header scalars, the residual write-back of an fp64 field and setup_wr are unchanged; a stream that outgrows setup_wr's
 * bound is fatal with the reference's message (only the bytes actually produced count, also for WRS3, whose worst case is
 * larger).  The DECODERS -- decoding_wrap, decoding_wrap_f, wr_decoding_wrap_f32 -- do not look at the setting: a coded field
 * of four bytes or more that starts with "WRS1" / "WRS2" / "WRS3" goes through wr_decode_host_seg (_f32), anything else through
 * wr_decode_host (every plane of a reference stream starts with byte 0x00).  The explicit-context entry points (wr_encode_host,
 * wr_decode_host, ...) neither change nor look at the setting.
 * Grammar of the text form:  ref | wrs1 | wrs2 | wrs3, then :seg=N, :brick=B, :strands=K in any order, each at most once,
 *   e.g. "wrs3:seg=4096:brick=16:strands=8".  Missing values are the defaults: WR_SEG_DEFAULT; WR_BRICK_DEFAULT for wrs2 and
 *   0 (the natural order) for wrs3; WR_STRANDS_DEFAULT.  Refused (WR_ERR_ARG, wr_last_error() quotes the offending token): an
 *   unknown name or key, a key given twice, any key with ref, brick with wrs1, strands without wrs3, a value the _seg encoders
 *   refuse, anything else after the name.
 * The environment variable WR_STREAM_FORMAT holds the same grammar.  It is read once, by the first implicit-context encode (or
 * the first wr_get_stream_format); a value that does not parse is fatal at that encode, with the parser's message -- there is
 * no silent fall back to the reference's stream.  wr_set_stream_format overrides it, before or after.
 * All four functions are host only: no device call, no context. */
#define WR_FORMAT_REF 0
#define WR_FORMAT_WRS1 1
#define WR_FORMAT_WRS2 2
#define WR_FORMAT_WRS3 3
/* text -> the four values, defaults filled in (ref: 0, 0, 0, 0); outputs may be NULL and are untouched on an error */
int wr_stream_format_parse(const char *text, int *format, unsigned *seg, unsigned *brick, unsigned *strands);
/* 0 for seg, brick (wrs2) or strands (wrs3) means the default, as in the _seg calls; WR_ERR_ARG on what those calls refuse,
 * on a non-zero brick with WRS1, non-zero strands without WRS3 and any non-zero parameter with WR_FORMAT_REF */
int wr_set_stream_format(int format, unsigned seg, unsigned brick, unsigned strands);
/* the setting in force, defaults filled in; WR_ERR_ARG (the parser's message) if WR_STREAM_FORMAT decides and does not parse */
int wr_get_stream_format(int *format, unsigned *seg, unsigned *brick, unsigned *strands);
/* WR_FORMAT_* of a coded field's first bytes; -1: neither (fewer than four bytes of a magic, an unknown magic, no bytes) */
int wr_stream_sniff(const unsigned char *data, size_t len);

/* ---- Transcoding: a coded field from one of the four stream formats to another, on its planes.  No new format.
 * A coded field is nlay planes of byte symbols plus its header record, and all four formats code the SAME planes under the same
 * header scalars; only the bytes of every plane differ.  A transcode decodes the planes with the source format's decoder and
 * codes them with the target's coder: no transform, no quantizer, no tolerance, and nothing is quantized a second time (a
 * decode followed by an encode codes the RECONSTRUCTION, whose min / max and therefore plane scalars are its own).
 *   source   whatever wr_stream_sniff says of the first plane; the planes of a stream must agree
 *   target   format is one of WR_FORMAT_*; seg, brick, strands are normalised and refused as by wr_set_stream_format (0 = the
 *            format's default, a parameter the format does not have must be 0).  All 16 pairs take the same path, same-format
 *            pairs included (a new seg, brick or strand count; ref -> ref is a check of the stream)
 *   result   *info_out is *info_in with only len_enc_vec and ntot_enc changed (info_out may be info_in); data_out is, byte for
 *            byte, what the target format's encoder -- wr_encode_host, or wr_encode_host_seg / _seg_blocked / _seg_strands with
 *            the same seg / brick / strands -- returns for the field the source stream was made from
 *   trivial  a constant field (info_in->ntot_enc == 0) passes through: the header is copied, no device work
 *   bound    wr_transcode_bound = nlay times the per-plane bound of the target (wr_range_encode_bound, wr_seg_bound,
 *            wr_seg_bound_blocked, wr_seg_bound_strands); any cap that holds the bytes actually produced succeeds
 *   len_in   bytes readable at data_in (0 = trust info_in->ntot_enc)
 * Refusals, in this order; *info_out is written only on success, and the context keeps working after every one of them:
 *   WR_ERR_ARG       null pointers, non-positive dimensions, a target the format setting refuses; then, for a field that is not
 *                    trivial, nlay outside 1..WR_NLAYMAX, wlev not 0 or 4, null buffers, data_out[0, cap) overlapping the input
 *   WR_ERR_STREAM    lengths that do not fit ntot_enc or len_in; first bytes that are no stream; planes that differ in format;
 *                    for a segmented source every header and index as by wr_decode_host_seg -- all of this on the host, before
 *                    anything is copied or launched; then a plane that does not decode (segments flagged by the kernels, or
 *                    "stream does not decode to nx*ny*nz symbols" from the host decoder).  The message starts "plane <l>: "
 *   WR_ERR_OVERFLOW  cap below the bytes produced, with the encoders' message
 * wr_transcode_host runs on a context: a segmented side is decoded / coded by the GPU's segment coders (with the inverse /
 * forward plane reorder of a blocked stream), a reference side by the host coder as in wr_decode_host / wr_encode_host -- the
 * coder pool, per-plane threads or wr_set_threads groups -- through the planes' pinned windows, the block histograms counted on
 * the device.  It takes no work-space slot; planes, blobs (the target's at their bound), one staging buffer and one stream-order
 * plane come from the plane pool.  A wr_decode_begin pending on the context is discarded.
 * wr_timings: plane_coder_s[l] is plane l's decoder time plus its coder time; `rangecoder` is the sum of the two halves' figures,
 * each as its own driver defines it (host coder: the slowest plane; segment coders: the sum over the planes); h2d_ms the blobs
 * or decoded windows going up, d2h_ms the histograms and windows or the blobs coming down; gpu the wall time of the kernel
 * stages; transfer = total - rangecoder; the transform and quantizer fields stay 0.
 * wr_transcode_host_ref is the definition on the calling thread (no context, no GPU): wr_range_decode / wr_range_encode and the
 * wr_seg_*_host_ref* functions, plane by plane; the same refusals in the same order, the same bytes. */
size_t wr_transcode_bound(size_t n, int nlay, int format, unsigned seg, unsigned brick, unsigned strands); /* host only; 0: refused */
int wr_transcode_host(wr_ctx *ctx, int nx, int ny, int nz, const wr_enc_info *info_in, const unsigned char *data_in,
                      size_t len_in, int format, unsigned seg, unsigned brick, unsigned strands, wr_enc_info *info_out,
                      unsigned char *data_out, size_t cap, wr_timings *tm);
int wr_transcode_host_ref(int nx, int ny, int nz, const wr_enc_info *info_in, const unsigned char *data_in, size_t len_in,
                          int format, unsigned seg, unsigned brick, unsigned strands, wr_enc_info *info_out,
                          unsigned char *data_out, size_t cap);

/* encoding_wrap / decoding_wrap for fp32 fields: the same arguments but the field, an implicit context per call and
 * the reference's "void + fatal" errors.  fld_1d of an encode is never overwritten (no residual write-back). */
void wr_encoding_wrap_f32(int nx, int ny, int nz, const float *fld_1d, int wtflag, int mx, int my, int mz,
                          double *cutoffvec, double *tolabs, double *midval, double *halfspanval,
                          unsigned char *wlev, unsigned char *nlay, unsigned long *ntot_enc, double *deps_vec,
                          double *minval_vec, unsigned long *len_enc_vec, unsigned char *data_enc);
void wr_decoding_wrap_f32(int nx, int ny, int nz, float *fld_1d, double *tolabs, double *midval,
                          double *halfspanval, unsigned char *wlev, unsigned char *nlay,
                          unsigned long *ntot_enc, double *deps_vec, double *minval_vec,
                          unsigned long *len_enc_vec, unsigned char *data_enc);
/* waveletcdf97_3d on a host array, in place */
int wr_transform_host(wr_ctx *ctx, double *h_fld, int nx, int ny, int nz, int lvl);

/* --- which kernels a transform of this shape runs on (host only: no device call, no context).  The finest `levels` levels
 * of a four-level forward (inverse != 0: inverse) transform can run on the fused single-pass kernels, the coarser ones run on
 * the general kernels; `used` says whether wr_dev_transform(.., +-4) and the codec take the fused path for this shape at all
 * (two fused levels, or one of a field of 2^21 samples or more), before the WR_NO_FUSED environment switch is looked at.
 * level[l], l < levels, finest first, is the launch of fused level l on its box (nx >> l) x (ny >> l) x (nz >> l), from the
 * function the launch itself takes its grid from: tiles_x * tiles_y workgroup columns, each cut along z into zsegs segments
 * of zps z-pairs, the last one of zlast.  Entries from `levels` on are zero.  A non-positive dimension or out == NULL:
 * WR_ERR_ARG. */
typedef struct wr_fused_level {
    int tiles_x, tiles_y, zps, zsegs, zlast;
} wr_fused_level;
typedef struct wr_fused_plan_t {
    int levels, used;
    wr_fused_level level[4];
} wr_fused_plan_t;
int wr_fused_plan(int nx, int ny, int nz, int inverse, wr_fused_plan_t *out);

/* --- host range coder alone (one plane stream), rows a6/a7/a10 of SURVEY.md 8a */
size_t wr_range_encode_bound(size_t n);
/* the same for a plane whose byte histograms per 60000-symbol block are known (unsigned short[256] per block, n/60000+1
 * blocks): block entropies + headers + the coder's worst-case rounding loss (0.0104 bit per symbol), a rigorous bound
 * within ~0.2 % of the stream's length.  wr_encode_* use it to code the planes of a field side by side straight into
 * data_enc (the reference codes each plane into a buffer of its own and copies, wrappers.cpp:412-427). */
size_t wr_range_encode_bound_hist(const unsigned short *hists, size_t n);
size_t wr_range_encode(const unsigned char *sym, size_t n, unsigned char *out);
size_t wr_range_decode(const unsigned char *in, size_t len, unsigned char *sym, size_t n);
/* `count` planes of n symbols each coded on the calling thread, their symbol loops interleaved
 * (up to 4 at a time): the same bytes as `count` calls of the functions above, at a fraction of
 * the CPU time, because one plane's coder is a serial dependency chain that leaves most of a
 * core idle.  out[k] holds wr_range_encode_bound(n) bytes; produced[k] as wr_range_decode. */
void wr_range_encode_multi(int count, const unsigned char *const *sym, size_t n,
                           unsigned char *const *out, size_t *lens);
void wr_range_decode_multi(int count, const unsigned char *const *in, const size_t *len,
                           unsigned char *const *sym, size_t n, size_t *produced);

/* the same through the coder pool (wr_set_coder_pool must have started it): `count` planes of their own lengths
 * n[k], coded by the pool's workers next to whatever else is queued; returns when all of them are done */
int wr_range_encode_pool(int count, const unsigned char *const *sym, const size_t *n,
                         unsigned char *const *out, size_t *lens);
int wr_range_decode_pool(int count, const unsigned char *const *in, const size_t *len,
                         unsigned char *const *sym, const size_t *n, size_t *produced);

/* `count` planes on the calling thread through the 16-lane AVX-512 loops: the encoder's takes planes of any kind,
 * the decoder's gains on dominant-symbol planes (any plane decodes correctly, the others just gain nothing);
 * WR_ERR_UNSUPPORTED on a CPU without AVX-512.  The coder pool routes all encoder planes and the decoder planes
 * below 2 bits per symbol there by itself. */
int wr_range_encode_vec(int count, const unsigned char *const *sym, const size_t *n,
                        unsigned char *const *out, size_t *lens);
int wr_range_decode_vec(int count, const unsigned char *const *in, const size_t *len,
                        unsigned char *const *sym, const size_t *n, size_t *produced);

/* Test hooks for the windowed symbol path: planes that live in device memory reach the host coder through a small
 * pinned ring, window by window (wr_encode_host / wr_decode_*); here the windows are `chunk` symbols (a multiple of
 * 60000) of plain host buffers.  mode 0: interleaved loops on the calling thread, 1: the coder pool, 2: the 16-lane
 * loops.  Same bytes / symbols as the whole-plane functions above. */
int wr_range_encode_windowed(int mode, int count, const unsigned char *const *sym, size_t n, size_t chunk,
                             unsigned char *const *out, size_t *lens);
int wr_range_decode_windowed(int mode, int count, const unsigned char *const *in, const size_t *len,
                             unsigned char *const *sym, size_t n, size_t chunk, size_t *produced);

/* Test hook for the plane hand-over (wr_handover.h): replays the window handle of a finished call against the plane of the
 * next call on the same context; 0 if the request was refused and left that plane untouched. */
int wr_test_stale_window(wr_ctx *ctx, size_t n);

/* --- for callers with a batch of independent fields (the wrenc / wrdec / FluSI tools): starts the coder pool with one
 * worker per CPU this process may use (affinity mask, cgroup quota) when nfields > 1, and returns how many
 * encoding_wrap / decoding_wrap (or wr_*_host) calls on fields of field_elems elements to keep in flight at once:
 * 1.5 per CPU, fewer if host memory or device memory are short, never more than nfields.  The calls themselves are
 * unchanged (same bytes); this only sizes the concurrency around them. */
int wr_autotune_batch(size_t field_elems, int nfields);

/* --- measurement hook for bench.py: runs `reps` forward (lvl>0) or inverse transforms of an
 * nx*ny*nz field back to back on the context's stream and returns the average duration of
 * one transform in milliseconds measured with HIP events on that stream. */
int wr_bench_transform(wr_ctx *ctx, double *d_fld, int nx, int ny, int nz, int lvl, int reps,
                       double *ms_per_transform);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
