// wr_kernels.hip -- hand-written gfx950 (CDNA4) kernels for the WaveRange hot path.
//
// What is here (round 1):
//   k_line_x      x-axis lifting of whole lines staged in LDS (in place)
//   k_stream      y-/z-axis lifting as a streaming register pipeline, one thread per x
//                 (coalesced along x), out of place (ping-pong)
//   k_minmax*     min/max reductions
//   k_quant       bit-plane quantizer fused with the residual update and its min/max
//   k_dequant     fused multi-plane dequantise-accumulate
//   k_synth       synthetic field generator, k_hist per-block histograms
//
// Arithmetic contract: every floating-point expression below is written exactly as the
// reference evaluates it (one rounding per * and per +); the translation unit is compiled
// with -ffp-contract=off and additionally pins it with the pragma below.  No MFMA: this is
// a 9-tap stencil + byte packing, HBM-bound.
#include "wr_kernels.h"
#include "wr_budget.h"

#include <stdlib.h>

#pragma clang fp contract(off)

namespace wrk {

// ---- constants: reference src/waveletcdf97_3d/waveletcdf97_3d.c:41-45,55-58 (values as
// hex doubles from SURVEY.md A.1; 2*c is exact so (c*2)*v is written with a folded constant)
#define WR_ALPHA (-0x1.960ce676401a2p+0)
#define WR_BETA (-0x1.b2035c9357a96p-5)
#define WR_GAMMA (0x1.c40ceba5738p-1)
#define WR_DELTA (0x1.c626a904721eep-2)
#define WR_ZETA (0x1.264c795071464p+0)
#define WR_IZETA (0x1.bd5edf975ce17p-1)
#define WR_EXT0 (-0x1.4f43b88aa31b3p-3)
#define WR_EXT1 (0x1.a6be82e3706b1p-4)
#define WR_EXT2 (0x1.0f7c8ee31b63bp+0)

static_assert(WR_ALPHA == -1.5861343420693648 && WR_BETA == -0.0529801185718856 &&
                  WR_GAMMA == 0.8829110755411875 && WR_DELTA == 0.4435068520511142 &&
                  WR_ZETA == 1.1496043988602418,
              "lifting constants");
static_assert(WR_IZETA == 1.0 / 1.1496043988602418, "1/zeta is the compile-time quotient");
static_assert(WR_EXT0 == -2 * WR_ALPHA * WR_BETA * WR_GAMMA / (1 + 2 * WR_BETA * WR_GAMMA), "ext0");
static_assert(WR_EXT1 == -2 * WR_BETA * WR_GAMMA / (1 + 2 * WR_BETA * WR_GAMMA), "ext1");
static_assert(WR_EXT2 == -2 * (WR_ALPHA + WR_GAMMA + 3 * WR_ALPHA * WR_BETA * WR_GAMMA) /
                             (1 + 2 * WR_BETA * WR_GAMMA),
              "ext2");

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// =====================================================================================
// x-axis pass: R whole lines per workgroup staged in LDS, four lifting sweeps with a
// workgroup barrier between them, in place.  (waveletcdf97_3d.c:82-142 fwd, :410-465 inv)
// =====================================================================================
template <bool INV>
__global__ __launch_bounds__(256) void k_line_x(double* __restrict__ X, int n, int n2, int n3,
                                                size_t sy, size_t sz, int R)
{
    extern __shared__ double lds[];
    const int m = (n + 1) >> 1;  // low-pass length
    const int mp = m + 1;        // row pitch (+1: keeps S/D rows off the same bank phase)
    double* S = lds;
    double* D = lds + (size_t)R * mp;
    const long long nlines = (long long)n2 * n3;
    const long long line0 = (long long)blockIdx.x * R;
    const int tid = threadIdx.x, nt = blockDim.x;
    const bool odd = n & 1;
    int rows = R;  // lines of this workgroup that exist
    if (line0 + rows > nlines) rows = (int)(nlines - line0);

    // ---- load (coalesced over the line), de-interleave (fwd) or scale (inv).  Loops are
    // (line, position) nests: no per-element division.
    for (int r = 0; r < rows; r++) {
        const long long line = line0 + r;
        const double* src = X + (size_t)(line % n2) * sy + (size_t)(line / n2) * sz;
        double* s = S + r * mp; double* d = D + r * mp;
        for (int j = tid; j < n; j += nt) {
            const double v = src[j];
            if (!INV) { if (j & 1) d[j >> 1] = v; else s[j >> 1] = v; }
            else { if (j < m) s[j] = v * WR_IZETA; else d[j - m] = v * WR_ZETA; }
        }
    }
    __syncthreads();
    if (odd) {
        // fwd: synthesise the missing last odd sample (:109); inv: it is zero (:314)
        for (int r = tid; r < rows; r += nt) {
            double* s = S + r * mp; double* d = D + r * mp;
            if (!INV) d[m - 1] = (s[m - 2] * WR_EXT0 + d[m - 2] * WR_EXT1) + s[m - 1] * WR_EXT2;
            else d[m - 1] = 0.0;
        }
        __syncthreads();
    }
    // one lifting sweep over all staged lines: ODD updates d from s, else s from d; SGN = +1 / -1
    auto sweep = [&](bool upd_d, double c, double sgn) {
        for (int r = 0; r < rows; r++) {
            double* s = S + r * mp; double* d = D + r * mp;
            for (int i = tid; i < m; i += nt) {
                if (upd_d) {
                    const double t = (i < m - 1) ? c * (s[i + 1] + s[i]) : (c * 2) * s[i];
                    d[i] = (sgn > 0) ? d[i] + t : d[i] - t;
                } else {
                    const double t = (i > 0) ? c * (d[i] + d[i - 1]) : (c * 2) * d[i];
                    s[i] = (sgn > 0) ? s[i] + t : s[i] - t;
                }
            }
        }
        __syncthreads();
    };
    if (!INV) {
        sweep(true, WR_ALPHA, 1.0); sweep(false, WR_BETA, 1.0); sweep(true, WR_GAMMA, 1.0); sweep(false, WR_DELTA, 1.0);
    } else {
        sweep(false, WR_DELTA, -1.0); sweep(true, WR_GAMMA, -1.0); sweep(false, WR_BETA, -1.0); sweep(true, WR_ALPHA, -1.0);
    }
    // ---- store (coalesced): fwd = [low | high] with scaling, inv = interleave
    for (int r = 0; r < rows; r++) {
        const long long line = line0 + r;
        double* dst = X + (size_t)(line % n2) * sy + (size_t)(line / n2) * sz;
        const double* s = S + r * mp; const double* d = D + r * mp;
        for (int j = tid; j < n; j += nt) {
            double v;
            if (!INV) v = (j < m) ? s[j] * WR_ZETA : d[j - m] * WR_IZETA;
            else v = (j & 1) ? d[j >> 1] : s[j >> 1];
            dst[j] = v;
        }
    }
}

// =====================================================================================
// y-/z-axis pass: one thread per x (coalesced), marching along the axis with the four
// lifting stages held as a register pipeline ("streaming lifting"); src -> dst.
//   forward  reads rows 2t, 2t+1          writes rows j (low) and m+j (high), j = t-2
//   inverse  reads rows t (low), q+t (high) writes rows 2j, 2j+1
// (waveletcdf97_3d.c:146-270 fwd, :292-406 inv)
// =====================================================================================
template <bool INV>
__global__ __launch_bounds__(64) void k_stream(const double* __restrict__ src, double* __restrict__ dst,
                                               int n, size_t sa, int n1, size_t st, int nb, size_t sb)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n1) return;
    const int m = (n + 1) >> 1;
    // batch index b: a grid-stride loop, so that nb is not bound by the 65535 limit of gridDim.y
    for (int b = blockIdx.y; b < nb; b += gridDim.y) {
    const size_t base = (size_t)x * st + (size_t)b * sb;
    const double* in = src + base;
    double* out = dst + base;

    if (!INV) {
        double sr1 = 0, dr1 = 0, p1 = 0, q1 = 0, p2 = 0;
        double s0 = in[0];
        double d0 = (1 < n) ? in[sa] : 0.0;  // n >= 2 always (caller skips shorter axes)
        for (int t = 0; t <= m + 1; t++) {
            // prefetch pair t+1 while pair t is being consumed
            double s_nx = 0, d_nx = 0;
            if (t + 1 < m) {
                s_nx = in[(size_t)(2 * t + 2) * sa];
                if (2 * t + 3 < n) d_nx = in[(size_t)(2 * t + 3) * sa];
            }
            if (t == m - 1 && (n & 1)) d0 = (sr1 * WR_EXT0 + dr1 * WR_EXT1) + s0 * WR_EXT2;
            double D1 = 0, S1 = 0;
            if (t >= 1 && t <= m) {
                const int j = t - 1;
                D1 = (j < m - 1) ? dr1 + WR_ALPHA * (s0 + sr1) : dr1 + (WR_ALPHA * 2) * sr1;
                S1 = (j > 0) ? sr1 + WR_BETA * (D1 + p1) : sr1 + (WR_BETA * 2) * D1;
            }
            if (t >= 2) {
                const int j = t - 2;
                double D2 = (j < m - 1) ? p1 + WR_GAMMA * (S1 + q1) : p1 + (WR_GAMMA * 2) * q1;
                double S2 = (j > 0) ? q1 + WR_DELTA * (D2 + p2) : q1 + (WR_DELTA * 2) * D2;
                out[(size_t)j * sa] = S2 * WR_ZETA;
                if (2 * j + 1 < n) out[(size_t)(m + j) * sa] = D2 * WR_IZETA;
                p2 = D2;
            }
            p1 = D1; q1 = S1; sr1 = s0; dr1 = d0;
            s0 = s_nx; d0 = d_nx;
        }
    } else {
        const int q = m;          // number of low-pass rows
        const int nh = n - q;     // number of high-pass rows
        double dprev = 0, s1prev = 0, d1prev = 0, s2prev = 0;
        double lo = in[0];
        double hi = (0 < nh) ? in[(size_t)q * sa] : 0.0;
        for (int t = 0; t <= q + 1; t++) {
            double lo_nx = 0, hi_nx = 0;
            if (t + 1 < q) {
                lo_nx = in[(size_t)(t + 1) * sa];
                if (t + 1 < nh) hi_nx = in[(size_t)(q + t + 1) * sa];
            }
            double d0 = 0, S1 = 0, D1 = 0, S2 = 0;
            if (t < q) {
                double s0 = lo * WR_IZETA;
                d0 = (t < nh) ? hi * WR_ZETA : 0.0;
                S1 = (t > 0) ? s0 - WR_DELTA * (d0 + dprev) : s0 - (WR_DELTA * 2) * d0;
            }
            if (t >= 1 && t <= q) {
                const int j = t - 1;
                D1 = (j < q - 1) ? dprev - WR_GAMMA * (S1 + s1prev) : dprev - (WR_GAMMA * 2) * s1prev;
                S2 = (j > 0) ? s1prev - WR_BETA * (D1 + d1prev) : s1prev - (WR_BETA * 2) * D1;
            }
            if (t >= 2) {
                const int j = t - 2;
                double DD = (j < q - 1) ? d1prev - WR_ALPHA * (S2 + s2prev) : d1prev - (WR_ALPHA * 2) * s2prev;
                out[(size_t)(2 * j) * sa] = s2prev;
                if (2 * j + 1 < n) out[(size_t)(2 * j + 1) * sa] = DD;
            }
            dprev = d0; s1prev = S1; d1prev = D1; s2prev = S2;
            lo = lo_nx; hi = hi_nx;
        }
    }
    }
}

// box copy src -> dst (only needed when exactly one of the y/z passes was skipped)
__global__ void k_copy_box(const double* __restrict__ src, double* __restrict__ dst, int n1, int n2, int n3,
                           size_t sy, size_t sz)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n1) return;
    for (int z = blockIdx.z; z < n3; z += gridDim.z)
        for (int y = blockIdx.y; y < n2; y += gridDim.y) {
            size_t o = (size_t)x + (size_t)y * sy + (size_t)z * sz;
            dst[o] = src[o];
        }
}

static inline unsigned grid_cap(int n) { return (unsigned)(n < 65535 ? n : 65535); }
static void launch_copy_box(const double* src, double* dst, int n1, int n2, int n3, size_t sy, size_t sz, hipStream_t st)
{
    hipLaunchKernelGGL(k_copy_box, dim3(cdiv(n1, 64), grid_cap(n2), grid_cap(n3)), dim3(64), 0, st, src, dst, n1, n2, n3, sy, sz);
}

// longest line the LDS-staged x pass takes (two half-lines of doubles + padding in 160 KiB)
constexpr int kMaxLdsLine = 10200;

static void launch_line_x(bool inv, double* X, int n, int n2, int n3, size_t sy, size_t sz, hipStream_t st)
{
    const int m = (n + 1) / 2;
    const size_t per_line = (size_t)2 * (m + 1) * sizeof(double);
    int R = (int)((48 * 1024) / per_line);  // <= 48 KiB of LDS per workgroup: 3 workgroups per CU
    if (R < 1) R = 1;                       // lines up to 10239 samples fit the 160 KiB LDS
    if (R > 64) R = 64;
    const long long nlines = (long long)n2 * n3;
    if (R > nlines) R = (int)nlines;
    const size_t lds = per_line * R;
    const int grid = cdiv(nlines, R);
    if (inv) {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)k_line_x<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_line_x<true>, dim3(grid), dim3(256), lds, st, X, n, n2, n3, sy, sz, R);
    } else {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)k_line_x<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_line_x<false>, dim3(grid), dim3(256), lds, st, X, n, n2, n3, sy, sz, R);
    }
}

// one streaming pass over the box (n1 x n2 x n3): axis 1 = y, 2 = z (threads along x, coalesced);
// axis 0 = x for lines too long for the LDS-staged kernel (threads along y: slow, but any length)
static void launch_stream(bool inv, const double* src, double* dst, int axis, int n1, int n2, int n3,
                          size_t sy, size_t sz, hipStream_t st)
{
    const int n = axis == 0 ? n1 : axis == 1 ? n2 : n3;          // marching axis
    const int nt = axis == 0 ? n2 : n1;                           // threads
    const int nb = axis == 1 ? n3 : axis == 2 ? n2 : n3;          // batches
    const size_t sa = axis == 0 ? 1 : axis == 1 ? sy : sz;
    const size_t tstride = axis == 0 ? sy : 1;
    const size_t sb = axis == 2 ? sy : sz;
    dim3 grid(cdiv(nt, 64), grid_cap(nb));
    if (inv) hipLaunchKernelGGL(k_stream<true>, grid, dim3(64), 0, st, src, dst, n, sa, nt, tstride, nb, sb);
    else hipLaunchKernelGGL(k_stream<false>, grid, dim3(64), 0, st, src, dst, n, sa, nt, tstride, nb, sb);
}

void transform(double* fld, double* scratch, int nx, int ny, int nz, int lvl, hipStream_t st)
{
    const int nl = lvl >= 0 ? lvl : -lvl;
    // forward visits boxes ceil(n/1), ceil(n/2), ...; inverse visits them coarsest first
    for (int step = 0; step < nl; step++) transform_level(fld, scratch, nx, ny, nz, lvl >= 0 ? step : nl - 1 - step, lvl < 0, st);
}

void transform_level(double* fld, double* scratch, int nx, int ny, int nz, int k, bool inverse, hipStream_t st)
{
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    auto up = [](int v, int p) { return v / p + (v % p ? 1 : 0); };
    const int lvl = inverse ? -1 : 1;
    {
        const int n1 = up(nx, 1 << k), n2 = up(ny, 1 << k), n3 = up(nz, 1 << k);
        double* cur = fld;
        double* oth = scratch;
        auto stream_pass = [&](int axis) {
            launch_stream(lvl < 0, cur, oth, axis, n1, n2, n3, sy, sz, st);
            double* t = cur; cur = oth; oth = t;
        };
        const bool long_x = n1 > kMaxLdsLine;
        if (lvl >= 0) {
            if (n1 > 1) { if (long_x) stream_pass(0); else launch_line_x(false, cur, n1, n2, n3, sy, sz, st); }
            if (n2 > 1) stream_pass(1);
            if (n3 > 1) stream_pass(2);
        } else {
            if (n3 > 1) stream_pass(2);
            if (n2 > 1) stream_pass(1);
            if (n1 > 1 && long_x) stream_pass(0);
            else {
                if (cur != fld) {  // bring the box home before the in-place x pass
                    launch_copy_box(cur, fld, n1, n2, n3, sy, sz, st);
                    cur = fld;
                }
                if (n1 > 1) launch_line_x(true, cur, n1, n2, n3, sy, sz, st);
            }
        }
        if (cur != fld) launch_copy_box(cur, fld, n1, n2, n3, sy, sz, st);
    }
}

// =====================================================================================
// reductions
// =====================================================================================
#define WR_RED_BLOCKS 2048
#define WR_RED_THREADS 256

int minmax_partials() { return WR_RED_BLOCKS; }

// NaNs are skipped, as the reference's fmin/fmax scan does (wrappers.cpp:246-249)
__device__ inline void mm_acc(double v, double& lo, double& hi)
{
    lo = fmin(lo, v);
    hi = fmax(hi, v);
}

__device__ inline void block_minmax(double lo, double hi, double* __restrict__ partial)
{
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_down(lo, o, 64));
        hi = fmax(hi, __shfl_down(hi, o, 64));
    }
    __shared__ double slo[WR_RED_THREADS / 64], shi[WR_RED_THREADS / 64];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[w] = lo; shi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WR_RED_THREADS / 64; i++) { lo = fmin(lo, slo[i]); hi = fmax(hi, shi[i]); }
        partial[2 * blockIdx.x] = lo;
        partial[2 * blockIdx.x + 1] = hi;
    }
}

template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2; };
template <> struct Pair<float> { using type = float2; };

// (fp32: the samples widened, which changes no minimum, maximum or NaN)
template <typename T>
__global__ __launch_bounds__(WR_RED_THREADS) void k_minmax(const T* __restrict__ x, size_t n,
                                                           double* __restrict__ partial)
{
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    const size_t n2 = n >> 1;
    const typename Pair<T>::type* x2 = reinterpret_cast<const typename Pair<T>::type*>(x);  // hipMalloc'd base: aligned
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        const typename Pair<T>::type v = x2[i];
        mm_acc((double)v.x, lo, hi);
        mm_acc((double)v.y, lo, hi);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) mm_acc((double)x[n - 1], lo, hi);
    block_minmax(lo, hi, partial);
}

__global__ __launch_bounds__(WR_RED_THREADS) void k_minmax_final(const double* __restrict__ partial, int np,
                                                                 double* __restrict__ result)
{
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        lo = fmin(lo, partial[2 * i]);
        hi = fmax(hi, partial[2 * i + 1]);
    }
    block_minmax(lo, hi, result);  // single block: lands in result[0], result[1]
}

static int red_grid(size_t n, int per_thread)
{
    long long g = cdiv((long long)n, (long long)WR_RED_THREADS * per_thread);
    if (g < 1) g = 1;
    if (g > WR_RED_BLOCKS) g = WR_RED_BLOCKS;
    return (int)g;
}

template <typename T>
static void minmax_t(const T* x, size_t n, double* partial, double* result, hipStream_t st)
{
    const int g = red_grid(n, 2);
    hipLaunchKernelGGL(k_minmax<T>, dim3(g), dim3(WR_RED_THREADS), 0, st, x, n, partial);
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
}
void minmax(const double* x, size_t n, double* partial, double* result, hipStream_t st) { minmax_t(x, n, partial, result, st); }
void minmax(const float* x, size_t n, double* partial, double* result, hipStream_t st) { minmax_t(x, n, partial, result, st); }

template <typename T>
__global__ void k_last_zero(const T* __restrict__ x, size_t n, unsigned long long* out)
{
    unsigned long long best = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (x[i] == (T)0) best = i + 1;  // grid-stride: i only grows, so the last hit is the largest
    if (best) atomicMax(out, best);
}

template <typename T>
static void last_zero_index_t(const T* x, size_t n, unsigned long long* out, hipStream_t st)
{
    (void)hipMemsetAsync(out, 0, sizeof(unsigned long long), st);
    hipLaunchKernelGGL(k_last_zero<T>, dim3(red_grid(n, 1)), dim3(WR_RED_THREADS), 0, st, x, n, out);
}
void last_zero_index(const double* x, size_t n, unsigned long long* out, hipStream_t st) { last_zero_index_t(x, n, out, st); }
void last_zero_index(const float* x, size_t n, unsigned long long* out, hipStream_t st) { last_zero_index_t(x, n, out, st); }

// fp32 fields where the fused kernels do not run (wr_codec.cpp): widened before the encoder, narrowed after the decoder
__global__ void k_widen_f32(const float* __restrict__ src, double* __restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}
__global__ void k_narrow_f64(const double* __restrict__ src, float* __restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}
void widen_f32(const float* src, double* dst, size_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_widen_f32, dim3(red_grid(n, 1)), dim3(WR_RED_THREADS), 0, st, src, dst, n);
}
void narrow_f64(const double* src, float* dst, size_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_narrow_f64, dim3(red_grid(n, 1)), dim3(WR_RED_THREADS), 0, st, src, dst, n);
}

// =====================================================================================
// quantizer plane, fused: q = (uchar)(aopt*x + bopt); r = x - (q*deps + minval); min/max(r)
// Each lane handles 2 adjacent elements per step (16-B load, 2-B plane store, 16-B store).
// =====================================================================================
// (unsigned char)(double) as the reference's x86-64 builds perform it: cvttsd2si to 32 bits, then the low byte.  For the values
// a quantizer plane is made of, [0.5, 255.5], that is C's truncation toward zero.  Outside the int range and for a NaN C leaves
// the cast undefined, and a field can get there: with a residual of subnormals deps falls below 2^-1024, aopt = 1 / deps is
// infinite and aopt * x + bopt is +inf or NaN.  cvttsd2si then gives 0x80000000 ("integer indefinite"): byte 0, where
// v_cvt_i32_f64 saturates +inf to 0x7fffffff: byte 255.  The oracle and the compiled reference code such planes as zeros.
__device__ inline unsigned char quant_byte(double fq) { return (unsigned char)(fabs(fq) < 0x1p31 ? (int)fq : 0); }

template <bool RESID>
__global__ __launch_bounds__(WR_RED_THREADS) void k_quant(double* __restrict__ x, size_t n, double aopt,
                                                          double bopt, double deps, double minval,
                                                          uint8_t* __restrict__ q, double* __restrict__ partial)
{
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    const size_t n2 = n >> 1;
    double2* x2 = reinterpret_cast<double2*>(x);
    uchar2* q2 = reinterpret_cast<uchar2*>(q);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        double2 v = x2[i];
        // (unsigned char)(double): quant_byte
        const unsigned char qa = quant_byte(aopt * v.x + bopt);
        const unsigned char qb = quant_byte(aopt * v.y + bopt);
        q2[i] = make_uchar2(qa, qb);
        if (RESID) {
            v.x = v.x - ((double)qa * deps + minval);
            v.y = v.y - ((double)qb * deps + minval);
            x2[i] = v;
            mm_acc(v.x, lo, hi);
            mm_acc(v.y, lo, hi);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double v = x[n - 1];
        const unsigned char qa = quant_byte(aopt * v + bopt);
        q[n - 1] = qa;
        if (RESID) {
            v = v - ((double)qa * deps + minval);
            x[n - 1] = v;
            mm_acc(v, lo, hi);
        }
    }
    if (RESID) block_minmax(lo, hi, partial);
}

// The same plane in chunks of 4096 elements per workgroup, the quantized bytes staged through LDS: the direct
// form stores 2 bytes per lane (128 B per wave instruction: 8.4 M store instructions for a 1024^3 plane), here
// every lane stores 16 bytes of the plane after the chunk's 8 loads per lane have been issued back to back.
constexpr int Q_CHUNK = 4096;
template <bool RESID>
__global__ __launch_bounds__(WR_RED_THREADS) void k_quant_lds(double* __restrict__ x, size_t nchunks, double aopt, double bopt,
                                                              double deps, double minval, PlaneRef q,
                                                              double* __restrict__ partial)
{
    __shared__ uchar2 sq[Q_CHUNK / 2];
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    const int t = threadIdx.x;
    for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        double2* x2 = reinterpret_cast<double2*>(x + ch * Q_CHUNK);
        double2 v[Q_CHUNK / 512];
#pragma unroll
        for (int j = 0; j < Q_CHUNK / 512; j++) v[j] = x2[j * 256 + t];
#pragma unroll
        for (int j = 0; j < Q_CHUNK / 512; j++) {
            const unsigned char qa = quant_byte(aopt * v[j].x + bopt);
            const unsigned char qb = quant_byte(aopt * v[j].y + bopt);
            sq[j * 256 + t] = make_uchar2(qa, qb);
            if (RESID) {
                v[j].x = v[j].x - ((double)qa * deps + minval);
                v[j].y = v[j].y - ((double)qb * deps + minval);
                x2[j * 256 + t] = v[j];
                mm_acc(v[j].x, lo, hi);
                mm_acc(v[j].y, lo, hi);
            }
        }
        __syncthreads();
        reinterpret_cast<uint4*>(q.at(ch * Q_CHUNK))[t] = reinterpret_cast<const uint4*>(sq)[t];
        __syncthreads();
    }
    if (RESID) block_minmax(lo, hi, partial);
}

// merges the partials of the chunked kernel (first g1) and of the tail kernel (g2 more)
void quantize_plane(double* x, size_t n, double aopt, double bopt, double deps, double minval, const PlaneRef& q,
                    bool write_resid, double* partial, double* result, hipStream_t st)
{
    const bool aligned = (((uintptr_t)x | (uintptr_t)q.chunk[0]) & 15) == 0;
    const bool chunked = q.shift < 63;  // (chunks are device allocations: aligned; the direct form below wants one array)
    if (chunked && !aligned) {  // the callers check this (wr_codec.cpp); the direct form would run past the first chunk
        fprintf(stderr, "libwaverange_amd: internal error: chunked plane with unaligned pointers (x=%p chunk0=%p)\n", (void*)x, (void*)q.chunk[0]);
        abort();
    }
    const size_t nchunks = aligned ? n / Q_CHUNK : 0;
    int g1 = 0;
    if (nchunks) {
        g1 = (int)(nchunks < (size_t)WR_RED_BLOCKS / 2 ? nchunks : (size_t)WR_RED_BLOCKS / 2);
        if (write_resid) hipLaunchKernelGGL(k_quant_lds<true>, dim3(g1), dim3(WR_RED_THREADS), 0, st, x, nchunks, aopt, bopt, deps, minval, q, partial);
        else hipLaunchKernelGGL(k_quant_lds<false>, dim3(g1), dim3(WR_RED_THREADS), 0, st, x, nchunks, aopt, bopt, deps, minval, q, partial);
    }
    const size_t done = nchunks * Q_CHUNK;
    int g2 = 0;
    if (done < n) {  // remainder (or everything, for unaligned pointers): direct form
        g2 = red_grid(n - done, 2);
        if (g2 > WR_RED_BLOCKS / 2) g2 = WR_RED_BLOCKS / 2;
        // (a chunked plane: the remainder is shorter than a group of 4096 and lies in one chunk)
        uint8_t* const qd = q.at(done);
        if (write_resid) hipLaunchKernelGGL(k_quant<true>, dim3(g2), dim3(WR_RED_THREADS), 0, st, x + done, n - done, aopt, bopt, deps, minval, qd, partial + 2 * g1);
        else hipLaunchKernelGGL(k_quant<false>, dim3(g2), dim3(WR_RED_THREADS), 0, st, x + done, n - done, aopt, bopt, deps, minval, qd, partial + 2 * g1);
    }
    if (write_resid) hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g1 + g2, result);
}

// =====================================================================================
// Quantizer plane WITHOUT a residual array: the residual a plane is cut from is recomputed from the coefficient array.
// The reference keeps the residual in memory (wrappers.cpp:397-398: fld_1d[j] -= iqfld*deps + minval after every plane), 17 B
// per element and plane here: 8 read, 8 written, 1 of plane.  But the residual after plane l is a fixed expression of the
// coefficient and of the scalars of planes 0 .. l, so a lane that holds the coefficient can redo the subtractions of the
// planes before (7 instructions each) instead of reading what the pass before wrote: 9 B per element and plane (8 read, 1
// of plane), whatever the plane, and the same bits -- every residual is produced by the same operations on the same
// operands, a register instead of a store and a load between them.  The array is written once, by the last plane, and only
// if the caller wants the residual (encoding_wrap leaves it in fld_1d).
// One workgroup works through whole coding blocks (60000 symbols, wrappers.cpp:68: the host coder's model blocks), so it
// also leaves the block's byte histogram (k_hist's job: one pass over the plane less); within a block, 4096 elements at a
// time, the plane bytes staged through LDS for 16-byte stores as in k_quant_lds.
// =====================================================================================
constexpr int QB = 60000;
constexpr int QW = 1024;  // elements a wave takes at a time: 8 x 16-byte loads per lane, 16 plane bytes per lane
// Between one wave's LDS stores and its own loads of the same bytes through another type (wave-private staging, no other
// wave involved): the hardware runs a wave's LDS instructions in order, so no s_barrier is needed -- but the compiler must
// be told that the type-punned loads depend on the stores.  A wavefront-scope release/acquire fence pair and the wave barrier
// (a scheduling barrier, zero instructions) say exactly that and nothing more.
__device__ inline void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool WRITE, bool MM, bool HIST>
__global__ __launch_bounds__(WR_RED_THREADS) void k_quant_blk(double* __restrict__ x, size_t n, QuantPrev prev, double aopt, double bopt,
                                                              double deps, double minval, PlaneRef q, uint16_t* __restrict__ hist,
                                                              double* __restrict__ partial)
{
    constexpr int COPIES = 8;
    constexpr int NW = WR_RED_THREADS / 64;
    __shared__ unsigned int h[HIST ? COPIES : 1][256 + 1];  // +1: the copies start in different banks
    // wave-private staging of the plane bytes: written as byte pairs, read back as 16-byte pieces by the same wave (LDS runs
    // a wave's instructions in order), so the waves of a workgroup never wait for one another inside a coding block
    __shared__ uchar2 sq[NW][QW / 2];
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    unsigned int* const mine = h[HIST ? (t & (COPIES - 1)) : 0];
    const size_t nb = n / QB + 1;  // includes the (possibly empty) final block, as the host coder's block count does
    for (size_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const size_t b0 = b * QB, b1 = (b0 + QB < n) ? b0 + QB : n;
        if (HIST) {
#pragma unroll
            for (int c = 0; c < COPIES; c++) h[c][t] = 0;
            __syncthreads();
        }
        // a block may straddle two chunks of the plane (never more); 60000 b and the chunk size are multiples of 16, so a
        // 16-byte piece lies in one of them
        const size_t c0 = (b0 < n ? b0 : (n ? n - 1 : 0)) >> q.shift, edge = (c0 + 1) << q.shift;
        uint8_t* const p0 = q.chunk[c0] + (b0 - (c0 << q.shift));
        uint8_t* const p1 = edge < b1 ? q.chunk[c0 + 1] : p0;
        for (size_t g0 = b0 + (size_t)w * QW; g0 < b1; g0 += (size_t)NW * QW) {
            const bool full = g0 + QW <= b1;  // wave-uniform
            double2* const x2 = reinterpret_cast<double2*>(x + g0);
            double2 v[QW / 128];
            if (full) {
#pragma unroll
                for (int j = 0; j < QW / 128; j++) v[j] = x2[j * 64 + lane];
            } else {
#pragma unroll
                for (int j = 0; j < QW / 128; j++) {
                    const size_t e = g0 + 2 * (size_t)(j * 64 + lane);
                    v[j] = make_double2(0.0, 0.0);
                    if (e + 1 < b1) v[j] = x2[j * 64 + lane];
                    else if (e < b1) v[j].x = x[e];
                }
            }
            // the planes before this one, in order: v becomes the residual this plane is cut from
#pragma unroll
            for (int p = 0; p < kQuantPrevMax; p++) {
                if (p < prev.n) {
                    const double pa = prev.aopt[p], pb = prev.bopt[p], pd = prev.deps[p], pm = prev.minval[p];
#pragma unroll
                    for (int j = 0; j < QW / 128; j++) {
                        const unsigned char qa = quant_byte(pa * v[j].x + pb);
                        const unsigned char qb = quant_byte(pa * v[j].y + pb);
                        v[j].x = v[j].x - ((double)qa * pd + pm);
                        v[j].y = v[j].y - ((double)qb * pd + pm);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < QW / 128; j++) {
                // (unsigned char)(double): quant_byte
                const unsigned char qa = quant_byte(aopt * v[j].x + bopt);
                const unsigned char qb = quant_byte(aopt * v[j].y + bopt);
                sq[w][j * 64 + lane] = make_uchar2(qa, qb);
                if (WRITE || MM) {
                    v[j].x = v[j].x - ((double)qa * deps + minval);
                    v[j].y = v[j].y - ((double)qb * deps + minval);
                    if (full) {
                        if (WRITE) x2[j * 64 + lane] = v[j];
                        if (MM) { mm_acc(v[j].x, lo, hi); mm_acc(v[j].y, lo, hi); }
                    } else {
                        const size_t e = g0 + 2 * (size_t)(j * 64 + lane);
                        if (e + 1 < b1) {
                            if (WRITE) x2[j * 64 + lane] = v[j];
                            if (MM) { mm_acc(v[j].x, lo, hi); mm_acc(v[j].y, lo, hi); }
                        } else if (e < b1) {
                            if (WRITE) x[e] = v[j].x;
                            if (MM) mm_acc(v[j].x, lo, hi);
                        }
                    }
                }
            }
            const size_t i = g0 + 16 * (size_t)lane;  // this lane's 16 symbols
            wave_lds_fence();  // the byte pairs above -> the 16-byte pieces below
            const uint4 wq = reinterpret_cast<const uint4*>(&sq[w][0])[lane];
            wave_lds_fence();  // ... and the next round's stores stay behind these loads
            if (i < b1) {
                uint8_t* const dstq = i < edge ? p0 + (i - b0) : p1 + (i - edge);
                const int cnt = (b1 - i < 16) ? (int)(b1 - i) : 16;
                const unsigned int words[4] = {wq.x, wq.y, wq.z, wq.w};
                if (cnt == 16) *reinterpret_cast<uint4*>(dstq) = wq;
                else
                    for (int k = 0; k < cnt; k++) dstq[k] = (uint8_t)(words[k >> 2] >> (8 * (k & 3)));
                if (HIST) {  // a run of equal symbols is one add (bit planes of a smooth field are dominated by one value)
                    unsigned int prevs = words[0] & 0xff, run = 0;
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const unsigned int sb = (words[k >> 2] >> (8 * (k & 3))) & 0xff;
                        if (k < cnt) {
                            if (sb != prevs) { atomicAdd(&mine[prevs], run); prevs = sb; run = 0; }
                            run++;
                        }
                    }
                    atomicAdd(&mine[prevs], run);
                }
            }
        }
        if (HIST) {
            __syncthreads();
            unsigned int tot = 0;
#pragma unroll
            for (int c = 0; c < COPIES; c++) tot += h[c][t];
            hist[b * 256 + t] = (uint16_t)tot;
            __syncthreads();  // before the next block zeroes the bins
        }
    }
    if (MM) block_minmax(lo, hi, partial);
}

// x := the residual after the planes in `prev` (the rare paths that want the residual in memory between two planes)
__global__ __launch_bounds__(WR_RED_THREADS) void k_resid_apply(double* __restrict__ x, size_t n, QuantPrev prev)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double v = x[i];
#pragma unroll
        for (int p = 0; p < kQuantPrevMax; p++)
            if (p < prev.n) {
                const unsigned char qa = quant_byte(prev.aopt[p] * v + prev.bopt[p]);
                v = v - ((double)qa * prev.deps[p] + prev.minval[p]);
            }
        x[i] = v;
    }
}

void residual_apply(double* x, size_t n, const QuantPrev& prev, hipStream_t st)
{
    if (!prev.n || !n) return;
    hipLaunchKernelGGL(k_resid_apply, dim3(red_grid(n, 1)), dim3(WR_RED_THREADS), 0, st, x, n, prev);
}

bool quantize_plane_blk_ok(const double* x, const PlaneRef& q)
{
    static const bool on = !(getenv("WR_QUANT_INPLACE") && atoi(getenv("WR_QUANT_INPLACE")));
    return on && (((uintptr_t)x | (uintptr_t)q.chunk[0]) & 15) == 0;
}

void quantize_plane_blk(double* x, size_t n, const QuantPrev& prev, double aopt, double bopt, double deps, double minval, const PlaneRef& q,
                        bool write_resid, bool want_minmax, uint16_t* hist, double* partial, double* result, hipStream_t st)
{
    const size_t nb = n / QB + 1;
    // one round of resident workgroups (8 per CU at most), each with a dozen blocks or more to stream through
    constexpr size_t gmax = (size_t)WR_RED_BLOCKS / 2;
    const int g = (int)(nb < gmax ? nb : gmax);
#define WR_QB_LAUNCH(W, M, H) hipLaunchKernelGGL((k_quant_blk<W, M, H>), dim3(g), dim3(WR_RED_THREADS), 0, st, x, n, prev, aopt, bopt, deps, minval, q, hist, partial)
    if (hist) {
        if (write_resid) { if (want_minmax) WR_QB_LAUNCH(true, true, true); else WR_QB_LAUNCH(true, false, true); }
        else { if (want_minmax) WR_QB_LAUNCH(false, true, true); else WR_QB_LAUNCH(false, false, true); }
    } else {
        if (write_resid) { if (want_minmax) WR_QB_LAUNCH(true, true, false); else WR_QB_LAUNCH(true, false, false); }
        else { if (want_minmax) WR_QB_LAUNCH(false, true, false); else WR_QB_LAUNCH(false, false, false); }
    }
#undef WR_QB_LAUNCH
    if (want_minmax) hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
}

// =====================================================================================
// The size probe of an encode to a byte budget (wr_budget.h): what WOULD the WRS1 blob of this plane take at most, for up to
// kProbeK quantizer steps at once?  The pass of k_quant_blk -- the coefficients in 16-byte loads, the planes before redone in
// registers -- but nothing is written: every candidate's bytes go through the wave's staging into one LDS histogram per
// candidate, and at the end of a segment 256 lanes turn each histogram into the segment's bound by table look-ups.  One
// workgroup takes one segment at a time.  The bounds are integers added up with integer atomics: the totals do not depend
// on the order the segments finish in.  MM: min/max of the residual candidate 0 would leave (the next plane's range).
// The histograms keep k_quant_blk's two answers to the one dominant symbol of a smooth plane: several copies that start
// in different banks, and one add per run of equal symbols among a lane's 16.
// =====================================================================================
constexpr int kProbeCopies = 4;

// the histograms of one segment of bs symbols -> acc (lane k < ncand: candidate k's bytes).  All 256 lanes, between barriers.
template <int K>
__device__ inline void probe_segment_end(unsigned int (*h)[kProbeCopies][256 + 1], unsigned long long (*wsum)[WR_RED_THREADS / 64], int ncand, uint32_t bs,
                                         const uint32_t* __restrict__ tab, unsigned long long fixed, unsigned long long& acc)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    __syncthreads();
    for (int k = 0; k < K; k++) {
        if (k >= ncand) break;
        unsigned int c = 0;
#pragma unroll
        for (int j = 0; j < kProbeCopies; j++) c += h[k][j][t];
        unsigned long long d = tab[c < wrbud::kTabN ? c : 0];  // (c <= bs < kTabN: the clamp never acts, it keeps the look-up in the table whatever happens)
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned int lo32 = __shfl_down((unsigned int)d, o, 64), hi32 = __shfl_down((unsigned int)(d >> 32), o, 64);
            d += (unsigned long long)hi32 << 32 | lo32;
        }
        if (lane == 0) wsum[k][w] = d;
    }
    __syncthreads();
    if (t < ncand) {
        unsigned long long sum = 0;
        for (int i = 0; i < WR_RED_THREADS / 64; i++) sum += wsum[t][i];
        acc += wrbud::segment_bytes(fixed, tab[wrbud::kTabN + (bs < wrbud::kTabN ? bs : 0)], sum);
    }
    __syncthreads();  // before the next segment zeroes the bins
}

// a lane's 16 symbols (cnt of them count) into its copy of a histogram, one add per run
__device__ inline void probe_count16(unsigned int* mine, const uint4& wq, int cnt)
{
    const unsigned int words[4] = {wq.x, wq.y, wq.z, wq.w};
    unsigned int prevs = words[0] & 0xff, run = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned int sb = (words[k >> 2] >> (8 * (k & 3))) & 0xff;
        if (k < cnt) {
            if (sb != prevs) { atomicAdd(&mine[prevs], run); prevs = sb; run = 0; }
            run++;
        }
    }
    atomicAdd(&mine[prevs], run);
}

template <int K, bool MM>
__global__ __launch_bounds__(WR_RED_THREADS) void k_quant_probe(const double* __restrict__ x, size_t n, unsigned seg, QuantPrev prev, ProbeCands cd,
                                                                const uint32_t* __restrict__ tab, unsigned long long fixed,
                                                                unsigned long long* __restrict__ totals, double* __restrict__ partial)
{
    constexpr int NW = WR_RED_THREADS / 64;
    __shared__ unsigned int h[K][kProbeCopies][256 + 1];
    __shared__ unsigned long long wsum[K][NW];
    __shared__ uchar2 sq[NW][QW / 2];  // wave-private staging, as in k_quant_blk
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ncand = cd.n < K ? cd.n : K;
    unsigned long long acc = 0;
    const size_t nseg = (n + seg - 1) / seg;
    for (size_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const size_t s0 = s * seg, s1 = (s0 + seg < n) ? s0 + seg : n;
        for (int i = t; i < K * kProbeCopies * 257; i += WR_RED_THREADS) (&h[0][0][0])[i] = 0;
        __syncthreads();
        for (size_t g0 = s0 + (size_t)w * QW; g0 < s1; g0 += (size_t)NW * QW) {
            const bool full = g0 + QW <= s1;  // wave-uniform
            const double2* const x2 = reinterpret_cast<const double2*>(x + g0);  // (seg is a multiple of 16: 128-byte aligned)
            double2 v[QW / 128];
            if (full) {
#pragma unroll
                for (int j = 0; j < QW / 128; j++) v[j] = x2[j * 64 + lane];
            } else {
#pragma unroll
                for (int j = 0; j < QW / 128; j++) {
                    const size_t e = g0 + 2 * (size_t)(j * 64 + lane);
                    v[j] = make_double2(0.0, 0.0);
                    if (e + 1 < s1) v[j] = x2[j * 64 + lane];
                    else if (e < s1) v[j].x = x[e];
                }
            }
#pragma unroll
            for (int p = 0; p < kQuantPrevMax; p++) {
                if (p < prev.n) {
                    const double pa = prev.aopt[p], pb = prev.bopt[p], pd = prev.deps[p], pm = prev.minval[p];
#pragma unroll
                    for (int j = 0; j < QW / 128; j++) {
                        const unsigned char qa = quant_byte(pa * v[j].x + pb);
                        const unsigned char qb = quant_byte(pa * v[j].y + pb);
                        v[j].x = v[j].x - ((double)qa * pd + pm);
                        v[j].y = v[j].y - ((double)qb * pd + pm);
                    }
                }
            }
            const size_t i = g0 + 16 * (size_t)lane;  // this lane's 16 symbols
            const int cnt = i < s1 ? ((s1 - i < 16) ? (int)(s1 - i) : 16) : 0;
            for (int k = 0; k < K; k++) {
                if (k >= ncand) break;
                const double aopt = cd.aopt[k], bopt = cd.bopt[k];
#pragma unroll
                for (int j = 0; j < QW / 128; j++) {
                    const unsigned char qa = quant_byte(aopt * v[j].x + bopt);
                    const unsigned char qb = quant_byte(aopt * v[j].y + bopt);
                    sq[w][j * 64 + lane] = make_uchar2(qa, qb);
                    if (MM && k == 0) {
                        const double ra = v[j].x - ((double)qa * cd.deps0 + cd.minval0);
                        const double rb = v[j].y - ((double)qb * cd.deps0 + cd.minval0);
                        const size_t e = g0 + 2 * (size_t)(j * 64 + lane);
                        if (full || e + 1 < s1) { mm_acc(ra, lo, hi); mm_acc(rb, lo, hi); }
                        else if (e < s1) mm_acc(ra, lo, hi);
                    }
                }
                wave_lds_fence();  // the byte pairs above -> the 16-byte piece below
                const uint4 wq = reinterpret_cast<const uint4*>(&sq[w][0])[lane];
                wave_lds_fence();  // ... and the next candidate's stores stay behind these loads
                if (cnt) probe_count16(h[k][t & (kProbeCopies - 1)], wq, cnt);
            }
        }
        probe_segment_end<K>(h, wsum, ncand, (uint32_t)(s1 - s0), tab, fixed, acc);
    }
    if (t < ncand && acc) atomicAdd(&totals[t], acc);
    if (MM) block_minmax(lo, hi, partial);
}

// the same bound for a plane of symbols that exists (one candidate, no arithmetic)
__global__ __launch_bounds__(WR_RED_THREADS) void k_plane_bound(const uint8_t* __restrict__ sym, size_t n, unsigned seg, const uint32_t* __restrict__ tab,
                                                                unsigned long long fixed, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned int h[1][kProbeCopies][256 + 1];
    __shared__ unsigned long long wsum[1][WR_RED_THREADS / 64];
    const int t = threadIdx.x;
    unsigned long long acc = 0;
    const size_t nseg = (n + seg - 1) / seg;
    for (size_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const size_t s0 = s * seg, s1 = (s0 + seg < n) ? s0 + seg : n;
        for (int i = t; i < kProbeCopies * 257; i += WR_RED_THREADS) (&h[0][0][0])[i] = 0;
        __syncthreads();
        for (size_t i = s0 + 16 * (size_t)t; i < s1; i += 16 * (size_t)WR_RED_THREADS) {  // (s0 and the plane are 16-byte aligned)
            const int cnt = (s1 - i < 16) ? (int)(s1 - i) : 16;
            uint4 wq = make_uint4(0, 0, 0, 0);
            if (cnt == 16) wq = *reinterpret_cast<const uint4*>(sym + i);
            else {
                unsigned int words[4] = {0, 0, 0, 0};
                for (int k = 0; k < cnt; k++) words[k >> 2] |= (unsigned int)sym[i + k] << (8 * (k & 3));
                wq = make_uint4(words[0], words[1], words[2], words[3]);
            }
            probe_count16(h[0][t & (kProbeCopies - 1)], wq, cnt);
        }
        probe_segment_end<1>(h, wsum, 1, (uint32_t)(s1 - s0), tab, fixed, acc);
    }
    if (t == 0 && acc) atomicAdd(&totals[0], acc);
}

static int probe_grid(size_t n, unsigned seg)
{
    const size_t nseg = (n + seg - 1) / seg;
    constexpr size_t gmax = (size_t)WR_RED_BLOCKS / 2;  // (one round of resident workgroups; the partials of MM fit d_partial)
    return (int)(nseg < gmax ? (nseg ? nseg : 1) : gmax);
}

void quant_probe(const double* x, size_t n, unsigned seg, const QuantPrev& prev, const ProbeCands& cd, bool want_minmax, const uint32_t* tab,
                 unsigned long long fixed, unsigned long long* totals, double* partial, double* result, hipStream_t st)
{
    (void)hipMemsetAsync(totals, 0, kProbeK * sizeof(unsigned long long), st);
    const int g = probe_grid(n, seg);
    if (want_minmax) {
        hipLaunchKernelGGL((k_quant_probe<kProbeK, true>), dim3(g), dim3(WR_RED_THREADS), 0, st, x, n, seg, prev, cd, tab, fixed, totals, partial);
        hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
    } else
        hipLaunchKernelGGL((k_quant_probe<kProbeK, false>), dim3(g), dim3(WR_RED_THREADS), 0, st, x, n, seg, prev, cd, tab, fixed, totals, partial);
}

void plane_bound(const uint8_t* sym, size_t n, unsigned seg, const uint32_t* tab, unsigned long long fixed, unsigned long long* totals, hipStream_t st)
{
    (void)hipMemsetAsync(totals, 0, sizeof(unsigned long long), st);
    hipLaunchKernelGGL(k_plane_bound, dim3(probe_grid(n, seg)), dim3(WR_RED_THREADS), 0, st, sym, n, seg, tab, fixed, totals);
}

// local-cutoff variant: one thread per physical position (a bijection onto wavelet space)
__global__ __launch_bounds__(WR_RED_THREADS) void k_quant_local(double* __restrict__ x, size_t n, double aopt,
                                                                double bopt, double deps, double minval,
                                                                uint8_t* __restrict__ q, LocalCutoff lc,
                                                                double* __restrict__ partial)
{
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    for (size_t jp = (size_t)blockIdx.x * blockDim.x + threadIdx.x; jp < n; jp += (size_t)gridDim.x * blockDim.x) {
        const int px = (int)(jp % (size_t)lc.nx), py = (int)((jp / (size_t)lc.nx) % (size_t)lc.ny);
        const int pz = (int)(jp / (size_t)lc.nx / (size_t)lc.ny);
        // ind_p2w_3d (waveletcdf97_3d.c:473-553); the "touched" flag is sticky across levels there
        int c1 = lc.nx, c2 = lc.ny, c3 = lc.nz, i1 = px, i2 = py, i3 = pz, lvl = 0, touched = 0;
        for (int k = 0; k < lc.wlev; k++) {
            const int m1 = c1 / 2 + (c1 % 2 > 0), m2 = c2 / 2 + (c2 % 2 > 0), m3 = c3 / 2 + (c3 % 2 > 0);
            if (c1 > 1 && i3 < c3 && i2 < c2 && i1 < c1) { i1 = (i1 % 2) ? i1 / 2 + m1 : i1 / 2; touched = 1; }
            if (c2 > 1 && i3 < c3 && i2 < c2 && i1 < c1) { i2 = (i2 % 2) ? i2 / 2 + m2 : i2 / 2; touched = 1; }
            if (c3 > 1 && i3 < c3 && i2 < c2 && i1 < c1) { i3 = (i3 % 2) ? i3 / 2 + m3 : i3 / 2; touched = 1; }
            c1 = m1; c2 = m2; c3 = m3;
            if (touched) lvl += 1;
        }
        double mask = lc.tolabs;
        if (lvl <= 1) {  // LOC_CUTOFF_LVL (defs.h:42); lcl_prec (wrappers.cpp:55-64)
            const int kx = (int)((double)px / (double)lc.nx * (double)lc.mx);
            const int ky = (int)((double)py / (double)lc.ny * (double)lc.my);
            const int kz = (int)((double)pz / (double)lc.nz * (double)lc.mz);
            mask = lc.tol_scale * lc.cutoff[kx + lc.mx * ky + lc.mx * lc.my * kz];
        }
        const size_t jw = (size_t)i1 + (size_t)lc.nx * (size_t)i2 + (size_t)lc.nx * (size_t)lc.ny * (size_t)i3;
        double v = x[jw];
        unsigned char qq;
        if (lc.span < mask) { qq = 0; v = minval; }
        else qq = quant_byte(aopt * v + bopt);
        q[jw] = qq;
        v = v - ((double)qq * deps + minval);
        x[jw] = v;
        mm_acc(v, lo, hi);
    }
    block_minmax(lo, hi, partial);
}

void quantize_plane_local(double* x, size_t n, double aopt, double bopt, double deps, double minval, uint8_t* q,
                          const LocalCutoff& lc, double* partial, double* result, hipStream_t st)
{
    const int g = red_grid(n, 1);
    hipLaunchKernelGGL(k_quant_local, dim3(g), dim3(WR_RED_THREADS), 0, st, x, n, aopt, bopt, deps, minval, q, lc, partial);
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
}

// =====================================================================================
// decoder: acc = 0; for l in order: acc = acc + (q_l*deps_l + min_l)   (wrappers.cpp:480,513-514)
// =====================================================================================
__global__ __launch_bounds__(WR_RED_THREADS) void k_dequant(double* __restrict__ acc, size_t n, DequantParams p)
{
    const size_t n2 = n >> 1;
    double2* a2 = reinterpret_cast<double2*>(acc);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        double2 a = make_double2(0.0, 0.0);
#pragma unroll
        for (int l = 0; l < 8; l++) {
            if (l < p.nlay) {
                uchar2 qq = reinterpret_cast<const uchar2*>(p.q[l].chunk[0])[i];  // (this form works on plain arrays: dequant_accum)
                a.x = a.x + ((double)qq.x * p.deps[l] + p.minval[l]);
                a.y = a.y + ((double)qq.y * p.deps[l] + p.minval[l]);
            }
        }
        a2[i] = a;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double a = 0.0;
        for (int l = 0; l < p.nlay; l++) a = a + ((double)p.q[l].chunk[0][n - 1] * p.deps[l] + p.minval[l]);
        acc[n - 1] = a;
    }
}

// Same sums, with the byte planes staged through LDS: a workgroup takes 4096 consecutive elements,
// reads each plane's 4 KB with 16-byte loads, and every store instruction of a wave then covers
// 1 KB of consecutive doubles (the direct form above moves 2 bytes per lane and load).
constexpr int DQ_CHUNK = 4096;
constexpr int DQW = 1024;  // elements a wave takes at a time; the staging is wave-private (no workgroup barrier: LDS runs a
                           // wave's instructions in order), so the waves of a workgroup stream independently
__global__ __launch_bounds__(256) void k_dequant_lds(double* __restrict__ acc, size_t nchunks, DequantParams p)
{
    __shared__ uint4 sq[4][8][DQW / 16];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t nsub = nchunks * (DQ_CHUNK / DQW);
    for (size_t sc = (size_t)blockIdx.x * 4 + w; sc < nsub; sc += (size_t)gridDim.x * 4) {
        const size_t base = sc * DQW;
#pragma unroll
        for (int l = 0; l < 8; l++)
            if (l < p.nlay) sq[w][l][lane] = reinterpret_cast<const uint4*>(p.q[l].at(base))[lane];
        wave_lds_fence();  // the 16-byte pieces above -> the byte pairs below (same wave; see k_quant_blk)
        double2* a2 = reinterpret_cast<double2*>(acc + base);
#pragma unroll
        for (int j = 0; j < DQW / 128; j++) {
            double2 a = make_double2(0.0, 0.0);
#pragma unroll
            for (int l = 0; l < 8; l++) {
                if (l < p.nlay) {
                    const uchar2 qq = reinterpret_cast<const uchar2*>(&sq[w][l][0])[j * 64 + lane];
                    a.x = a.x + ((double)qq.x * p.deps[l] + p.minval[l]);
                    a.y = a.y + ((double)qq.y * p.deps[l] + p.minval[l]);
                }
            }
            a2[j * 64 + lane] = a;
        }
        wave_lds_fence();  // the next round's stores stay behind this round's loads
    }
}

void dequant_accum(double* acc, size_t n, const DequantParams& p, hipStream_t st)
{
    bool aligned = ((uintptr_t)acc & 15) == 0;
    bool chunked = false;
    for (int l = 0; l < p.nlay; l++) { aligned = aligned && ((uintptr_t)p.q[l].chunk[0] & 15) == 0; chunked = chunked || p.q[l].shift < 63; }
    if (chunked && !aligned) {  // the direct form reads chunk[0][i] for the whole plane
        fprintf(stderr, "libwaverange_amd: internal error: chunked plane with unaligned pointers (acc=%p)\n", (void*)acc);
        abort();
    }
    const size_t nchunks = aligned ? n / DQ_CHUNK : 0;
    if (nchunks) {
        const size_t g = nchunks < 256 * 8 ? nchunks : 256 * 8;
        hipLaunchKernelGGL(k_dequant_lds, dim3((unsigned)g), dim3(256), 0, st, acc, nchunks, p);
    }
    const size_t done = nchunks * DQ_CHUNK;
    if (done < n) {  // remainder (or everything, for unaligned plane pointers): direct form
        DequantParams r = p;  // the remainder of every plane as a plain array (a chunked plane: shorter than a group, in one chunk)
        for (int l = 0; l < p.nlay; l++) r.q[l] = plane_ref(p.q[l].at(done));
        hipLaunchKernelGGL(k_dequant, dim3(red_grid(n - done, 2)), dim3(WR_RED_THREADS), 0, st, acc + done, n - done, r);
    }
}

// =====================================================================================
// helpers
// =====================================================================================
__global__ __launch_bounds__(WR_RED_THREADS) void k_linf(const double* __restrict__ a, const double* __restrict__ b,
                                                         size_t n, double* __restrict__ partial)
{
    // reuses the min/max plumbing: "lo" carries -max|a-b| so that fmin keeps the largest diff
    const double nan = __builtin_nan("");
    double lo = nan, hi = nan;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        lo = fmin(lo, -fabs(a[i] - b[i]));
        hi = fmax(hi, fabs(a[i]));
    }
    block_minmax(lo, hi, partial);
}

__global__ void k_neg0(double* r) { r[0] = -r[0]; }

void linf_diff(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st)
{
    const int g = red_grid(n, 1);
    hipLaunchKernelGGL(k_linf, dim3(g), dim3(WR_RED_THREADS), 0, st, a, b, n, partial);
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
    hipLaunchKernelGGL(k_neg0, dim3(1), dim3(1), 0, st, result);
}

// The compare of an encode to an error bound: max |a - b| over the differences that are finite, and the count of those that
// are not (a NaN or an infinity on either side).  Both operands widened to fp64, one subtraction per sample; the maximum of
// such values is exact, whatever the order of the reduction.  partial[2b] = block b's maximum, partial[2b + 1] its count
// (an integer below 2^53 in a double: the sums are exact).
__device__ inline void linf_cnt_acc(double a, double b, double& mx, double& cnt)
{
    const double d = fabs(a - b);
    if (d <= DBL_MAX) mx = fmax(mx, d);
    else cnt += 1.0;
}

__device__ inline void block_max_sum(double mx, double cnt, double* __restrict__ out)
{
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_down(mx, o, 64));
        cnt += __shfl_down(cnt, o, 64);
    }
    __shared__ double smx[WR_RED_THREADS / 64], scn[WR_RED_THREADS / 64];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smx[w] = mx; scn[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WR_RED_THREADS / 64; i++) { mx = fmax(mx, smx[i]); cnt += scn[i]; }
        out[0] = mx;
        out[1] = cnt;
    }
}

// PAIRS: both arrays are aligned for the two-sample loads of k_minmax (16 bytes fp64, 8 bytes fp32)
template <typename T, bool PAIRS>
__global__ __launch_bounds__(WR_RED_THREADS) void k_linf_cnt(const T* __restrict__ a, const T* __restrict__ b, size_t n, double* __restrict__ partial)
{
    double mx = 0.0, cnt = 0.0;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if (PAIRS) {
        const size_t n2 = n >> 1;
        const typename Pair<T>::type* a2 = reinterpret_cast<const typename Pair<T>::type*>(a);
        const typename Pair<T>::type* b2 = reinterpret_cast<const typename Pair<T>::type*>(b);
        for (size_t i = tid; i < n2; i += nthr) {
            const typename Pair<T>::type va = a2[i], vb = b2[i];
            linf_cnt_acc((double)va.x, (double)vb.x, mx, cnt);
            linf_cnt_acc((double)va.y, (double)vb.y, mx, cnt);
        }
        if ((n & 1) && tid == 0) linf_cnt_acc((double)a[n - 1], (double)b[n - 1], mx, cnt);
    } else {
        for (size_t i = tid; i < n; i += nthr) linf_cnt_acc((double)a[i], (double)b[i], mx, cnt);
    }
    block_max_sum(mx, cnt, partial + 2 * blockIdx.x);
}

__global__ __launch_bounds__(WR_RED_THREADS) void k_linf_cnt_final(const double* __restrict__ partial, int np, double* __restrict__ result)
{
    double mx = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        mx = fmax(mx, partial[2 * i]);
        cnt += partial[2 * i + 1];
    }
    block_max_sum(mx, cnt, result);  // single block: lands in result[0], result[1]
}

template <typename T>
static void linf_count_t(const T* a, const T* b, size_t n, double* partial, double* result, hipStream_t st)
{
    const bool pairs = (((uintptr_t)a | (uintptr_t)b) & (2 * sizeof(T) - 1)) == 0;
    const int g = red_grid(n, 2);
    if (pairs) hipLaunchKernelGGL((k_linf_cnt<T, true>), dim3(g), dim3(WR_RED_THREADS), 0, st, a, b, n, partial);
    else hipLaunchKernelGGL((k_linf_cnt<T, false>), dim3(g), dim3(WR_RED_THREADS), 0, st, a, b, n, partial);
    hipLaunchKernelGGL(k_linf_cnt_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
}
void linf_count(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st) { linf_count_t(a, b, n, partial, result, st); }
void linf_count(const float* a, const float* b, size_t n, double* partial, double* result, hipStream_t st) { linf_count_t(a, b, n, partial, result, st); }

// The compare of an encode to an RMS or PSNR target: in one pass what k_linf_cnt gives -- the maximum of the finite |a - b| and
// the count of differences that are not finite -- and S, the sum of q = fl(d * d) over the finite d = fl(a - b) (operands
// widened to fp64; the product is rounded once, nothing here contracts to an FMA).  partial[3b .. 3b + 2] = block b's maximum,
// count and sum.
// The order of the sum is fixed by n and by which load form runs, never by the order in which blocks or waves finish: a thread
// adds its terms in index order (the two-sample form keeps one sum per sample of the pair and adds the second to the first,
// then the odd tail), the lanes of a wave combine by shuffles at distances 32 .. 1, thread 0 adds the waves' sums in wave
// order, the final block's thread t adds the partials t, t + 256, .. in that order and reduces the same way.  No atomics.
// Accuracy.  Every term is >= 0, so a sum that passes through k roundings lies within k u / (1 - k u) of the real sum of the
// same q, u = 2^-53.  The grid is red_grid(n, 2) blocks of WR_RED_THREADS, at most WR_RED_BLOCKS x WR_RED_THREADS = 2^19
// threads: a thread of the element-wise form adds at most ceil(n / 2^19) terms (2^14 at n = 2^33), a sum of the two-sample
// form ceil(n / 2^20) and one addition joins the two; then 6 shuffle steps, 3 waves, and in the final block at most 8 partials,
// 6 steps, 3 waves: k <= 2^14 + 26, |S - S*| < 2^-38 S* for every n <= 2^33.
__device__ inline void err_stats_acc(double a, double b, double& mx, double& cnt, double& s)
{
    const double d = a - b, m = fabs(d);
    if (m <= DBL_MAX) { mx = fmax(mx, m); s = s + d * d; }
    else cnt += 1.0;
}

__device__ inline void block_max_sum_sum(double mx, double cnt, double s, double* __restrict__ out)
{
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_down(mx, o, 64));
        cnt += __shfl_down(cnt, o, 64);
        s = s + __shfl_down(s, o, 64);
    }
    __shared__ double smx[WR_RED_THREADS / 64], scn[WR_RED_THREADS / 64], ssq[WR_RED_THREADS / 64];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smx[w] = mx; scn[w] = cnt; ssq[w] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WR_RED_THREADS / 64; i++) { mx = fmax(mx, smx[i]); cnt += scn[i]; s = s + ssq[i]; }
        out[0] = mx;
        out[1] = cnt;
        out[2] = s;
    }
}

// PAIRS: as k_linf_cnt
template <typename T, bool PAIRS>
__global__ __launch_bounds__(WR_RED_THREADS) void k_err_stats(const T* __restrict__ a, const T* __restrict__ b, size_t n, double* __restrict__ partial)
{
    double mx = 0.0, cnt = 0.0, s = 0.0;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if (PAIRS) {
        double s1 = 0.0;
        const size_t n2 = n >> 1;
        const typename Pair<T>::type* a2 = reinterpret_cast<const typename Pair<T>::type*>(a);
        const typename Pair<T>::type* b2 = reinterpret_cast<const typename Pair<T>::type*>(b);
        for (size_t i = tid; i < n2; i += nthr) {
            const typename Pair<T>::type va = a2[i], vb = b2[i];
            err_stats_acc((double)va.x, (double)vb.x, mx, cnt, s);
            err_stats_acc((double)va.y, (double)vb.y, mx, cnt, s1);
        }
        s = s + s1;
        if ((n & 1) && tid == 0) err_stats_acc((double)a[n - 1], (double)b[n - 1], mx, cnt, s);
    } else {
        for (size_t i = tid; i < n; i += nthr) err_stats_acc((double)a[i], (double)b[i], mx, cnt, s);
    }
    block_max_sum_sum(mx, cnt, s, partial + 3 * blockIdx.x);
}

__global__ __launch_bounds__(WR_RED_THREADS) void k_err_stats_final(const double* __restrict__ partial, int np, double* __restrict__ result)
{
    double mx = 0.0, cnt = 0.0, s = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        mx = fmax(mx, partial[3 * i]);
        cnt += partial[3 * i + 1];
        s = s + partial[3 * i + 2];
    }
    block_max_sum_sum(mx, cnt, s, result);  // single block: lands in result[0 .. 2]
}

template <typename T>
static void err_stats_t(const T* a, const T* b, size_t n, double* partial, double* result, hipStream_t st)
{
    const bool pairs = (((uintptr_t)a | (uintptr_t)b) & (2 * sizeof(T) - 1)) == 0;
    const int g = red_grid(n, 2);
    if (pairs) hipLaunchKernelGGL((k_err_stats<T, true>), dim3(g), dim3(WR_RED_THREADS), 0, st, a, b, n, partial);
    else hipLaunchKernelGGL((k_err_stats<T, false>), dim3(g), dim3(WR_RED_THREADS), 0, st, a, b, n, partial);
    hipLaunchKernelGGL(k_err_stats_final, dim3(1), dim3(WR_RED_THREADS), 0, st, partial, g, result);
}
void err_stats(const double* a, const double* b, size_t n, double* partial, double* result, hipStream_t st) { err_stats_t(a, b, n, partial, result, st); }
void err_stats(const float* a, const float* b, size_t n, double* partial, double* result, hipStream_t st) { err_stats_t(a, b, n, partial, result, st); }

// =====================================================================================
// The trial of an encode to an error bound: what would the decoder's coefficient sum be, had the planes been cut with these
// steps?  acc[j] is what k_dequant / k_dequant_lds give from the planes k_quant_blk would have written -- the full planes in
// `prev`, then the last one -- formed straight from the coefficient: per plane q = quant_byte(aopt * r + bopt),
// t = (double)q * deps + minval, acc = acc + t, r = r - t, the operations of those kernels on the same operands (the term t is
// the one value both of them form), so every bit agrees.  No plane, residual or histogram is written: 8 bytes read and 8
// written per sample, no LDS.  A wave takes RQW elements at a time, 8 x 16-byte loads per lane in flight, as k_quant_blk; the
// waves stride over the whole tiles, the elements behind the last whole tile go one by one.  ntiles = 0 (unaligned pointers):
// everything goes one by one.
// =====================================================================================
constexpr int RQW = 1024;
__device__ inline double requant_one(double v, const QuantPrev& prev, double aopt, double bopt, double deps, double minval)
{
    double a = 0.0;
#pragma unroll
    for (int p = 0; p < kQuantPrevMax; p++) {
        if (p < prev.n) {
            const unsigned char q = quant_byte(prev.aopt[p] * v + prev.bopt[p]);
            const double t = (double)q * prev.deps[p] + prev.minval[p];
            a = a + t;
            v = v - t;
        }
    }
    const unsigned char q = quant_byte(aopt * v + bopt);
    return a + ((double)q * deps + minval);
}

__global__ __launch_bounds__(WR_RED_THREADS) void k_requant_accum(const double* __restrict__ x, size_t n, size_t ntiles, QuantPrev prev, double aopt,
                                                                  double bopt, double deps, double minval, double* __restrict__ acc)
{
    constexpr int NW = WR_RED_THREADS / 64;
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * NW + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * NW;
    for (size_t tile = wave; tile < ntiles; tile += nwaves) {
        const double2* const x2 = reinterpret_cast<const double2*>(x + tile * RQW);
        double2* const a2 = reinterpret_cast<double2*>(acc + tile * RQW);
        double2 v[RQW / 128], a[RQW / 128];
#pragma unroll
        for (int j = 0; j < RQW / 128; j++) { v[j] = x2[j * 64 + lane]; a[j] = make_double2(0.0, 0.0); }
#pragma unroll
        for (int p = 0; p < kQuantPrevMax; p++) {
            if (p < prev.n) {
                const double pa = prev.aopt[p], pb = prev.bopt[p], pd = prev.deps[p], pm = prev.minval[p];
#pragma unroll
                for (int j = 0; j < RQW / 128; j++) {
                    const unsigned char qa = quant_byte(pa * v[j].x + pb);
                    const unsigned char qb = quant_byte(pa * v[j].y + pb);
                    const double ta = (double)qa * pd + pm, tb = (double)qb * pd + pm;
                    a[j].x = a[j].x + ta; a[j].y = a[j].y + tb;
                    v[j].x = v[j].x - ta; v[j].y = v[j].y - tb;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RQW / 128; j++) {
            const unsigned char qa = quant_byte(aopt * v[j].x + bopt);
            const unsigned char qb = quant_byte(aopt * v[j].y + bopt);
            a[j].x = a[j].x + ((double)qa * deps + minval);
            a[j].y = a[j].y + ((double)qb * deps + minval);
            a2[j * 64 + lane] = a[j];
        }
    }
    for (size_t i = ntiles * RQW + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        acc[i] = requant_one(x[i], prev, aopt, bopt, deps, minval);
}

void requant_accum(const double* x, size_t n, const QuantPrev& prev, double aopt, double bopt, double deps, double minval, double* acc, hipStream_t st)
{
    if (!n) return;
    const bool aligned = (((uintptr_t)x | (uintptr_t)acc) & 15) == 0;
    const size_t ntiles = aligned ? n / RQW : 0;
    constexpr size_t NW = WR_RED_THREADS / 64;
    // one round of resident workgroups over the whole tiles; without any, the grid of an element-wise pass
    size_t g = ntiles ? (ntiles + NW - 1) / NW : (size_t)red_grid(n, 1);
    if (g > (size_t)WR_RED_BLOCKS) g = WR_RED_BLOCKS;
    hipLaunchKernelGGL(k_requant_accum, dim3((unsigned)g), dim3(WR_RED_THREADS), 0, st, x, n, ntiles, prev, aopt, bopt, deps, minval, acc);
}

__global__ void k_fill(double* x, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = v;
}

void fill(double* x, size_t n, double v, hipStream_t st)
{
    hipLaunchKernelGGL(k_fill, dim3(red_grid(n, 1)), dim3(WR_RED_THREADS), 0, st, x, n, v);
}

__device__ inline double tent(double t) { return 1.0 - fabs(2.0 * t - 1.0); }

// bit-identical to waverange_amd/synth.py::field (IEEE + - * / floor only)
__global__ void k_synth(double* __restrict__ out, int nx, int ny, int nz, unsigned long long seed, int z0, int z1)
{
    const size_t total = (size_t)nx * ny * (size_t)(z1 - z0);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e % nx);
        const int j = (int)((e / nx) % ny);
        const int k = z0 + (int)(e / ((size_t)nx * ny));
        const double u = (double)i / (double)nx, v = (double)j / (double)ny, w = (double)k / (double)nz;
        const double tv = tent(v);
        const double a = 10.0 * (4.0 * u * (1.0 - u)) * (tv * tv) * (1.0 - 2.0 * w);
        const double u8 = 8.0 * u, v8 = 8.0 * v, w8 = 8.0 * w;
        const double b = 0.1 * tent(u8 - floor(u8)) * tent(v8 - floor(v8)) * tent(w8 - floor(w8));
        const unsigned long long lin = ((unsigned long long)k * ny + j) * nx + i;
        unsigned long long z = seed + (lin + 1ull) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        const double r = (double)(z >> 11) * (1.0 / 9007199254740992.0);
        const double c = 0.01 * (r - 0.5);
        out[e] = (a + b) + c;
    }
}

void synth_field(double* out, int nx, int ny, int nz, unsigned long long seed, int z0, int z1, hipStream_t st)
{
    const size_t total = (size_t)nx * ny * (size_t)(z1 - z0);
    hipLaunchKernelGGL(k_synth, dim3(red_grid(total, 1)), dim3(WR_RED_THREADS), 0, st, out, nx, ny, nz, seed, z0, z1);
}

// one workgroup per 60000-symbol coding block: LDS histogram -> uint16[256].  Bit planes of a smooth
// field are dominated by one value, so (a) a lane reads 16 symbols at once and adds a run of equal
// ones with a single atomic, and (b) the lanes spread over 8 copies of the histogram, which bounds the
// same-address serialisation of the LDS atomics.  (60000 = 16 * 3750; the plane base is 256-B aligned.)
__global__ __launch_bounds__(256) void k_hist(PlaneRef q, size_t n, uint16_t* __restrict__ hist)
{
    constexpr int COPIES = 8;
    __shared__ unsigned int h[COPIES][256 + 1];  // +1: the copies start in different banks
    for (int c = 0; c < COPIES; c++) h[c][threadIdx.x] = 0;
    __syncthreads();
    const size_t b0 = (size_t)blockIdx.x * 60000;
    const size_t b1 = (b0 + 60000 < n) ? b0 + 60000 : n;
    unsigned int* mine = h[threadIdx.x & (COPIES - 1)];
    const size_t nvec = (b1 - b0) / 16;
    // a block of 60000 symbols may straddle two chunks of the plane (never more: a chunk is megabytes); 60000 b and the
    // chunk size are multiples of 16, so a 16-byte load lies in one of them
    const size_t c0 = (b0 < n ? b0 : (n ? n - 1 : 0)) >> q.shift, edge = (c0 + 1) << q.shift;  // (the empty final block reads nothing)
    const uint8_t* const p0 = q.chunk[c0] + (b0 - (c0 << q.shift));
    const uint8_t* const p1 = edge < b1 ? q.chunk[c0 + 1] : p0;
    auto sym_ptr = [&](size_t i) -> const uint8_t* { return i < edge ? p0 + (i - b0) : p1 + (i - edge); };
    for (size_t v = threadIdx.x; v < nvec; v += 256) {
        const uint4 w = *reinterpret_cast<const uint4*>(sym_ptr(b0 + 16 * v));
        const unsigned int words[4] = {w.x, w.y, w.z, w.w};
        unsigned int prev = words[0] & 0xff, run = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned int b = (words[k >> 2] >> (8 * (k & 3))) & 0xff;
            if (b != prev) { atomicAdd(&mine[prev], run); prev = b; run = 0; }
            run++;
        }
        atomicAdd(&mine[prev], run);
    }
    for (size_t i = b0 + nvec * 16 + threadIdx.x; i < b1; i += 256) atomicAdd(&mine[*sym_ptr(i)], 1u);
    __syncthreads();
    unsigned int tot = 0;
    for (int c = 0; c < COPIES; c++) tot += h[c][threadIdx.x];
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = (uint16_t)tot;
}

// Plain copy by a handful of workgroups: moves host <-> device data through the compute units instead of an SDMA
// engine (pinned host memory is device-visible).  8-16 workgroups reach the PCIe rate (profiles/r02/c_d2h_probe.txt).
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
    }
    for (; i < n16; i += stride) dst[i] = src[i];
}

void copy_kernel(void* dst, const void* src, size_t bytes, int workgroups, hipStream_t st)
{
    hipLaunchKernelGGL(k_copy16, dim3(workgroups), dim3(256), 0, st, static_cast<const uint4*>(src), static_cast<uint4*>(dst), bytes / 16);
}

// Clock keeper: occupies every CU for `ticks` of the 100 MHz wall clock and leaves -- mode 0 with a chain of fp64 multiply-adds
// (real load), mode 1 asleep (s_sleep between looks at the clock).  Every wave leaves by the clock, whatever it computed.
__global__ __launch_bounds__(256) void k_burn(long long ticks, int mode, double* sink)
{
    const long long t0 = wall_clock64();
    double a = 1.0 + threadIdx.x * 1e-9, b = 0.999999;
    while (wall_clock64() - t0 < ticks) {
        if (mode == 0) {
#pragma unroll
            for (int i = 0; i < 64; i++) a = a * b + 1e-9;
        } else
            __builtin_amdgcn_s_sleep(64);
    }
    if (a == 123.456) sink[0] = a;  // (never: keeps the chain alive)
}

void burn(double ms, int mode, int workgroups, double* sink, hipStream_t st)
{
    hipLaunchKernelGGL(k_burn, dim3(workgroups), dim3(256), 0, st, (long long)(ms * 1e5), mode, sink);
}

void block_histograms(const PlaneRef& q, size_t n, uint16_t* hist, hipStream_t st)
{
    const int nb = (int)(n / 60000 + 1);  // includes the (possibly empty) final block
    hipLaunchKernelGGL(k_hist, dim3(nb), dim3(256), 0, st, q, n, hist);
}

}  // namespace wrk
