// wr_lowres.hip -- the kernels of a low-resolution decode next to the list form of the segment decoder (wr_segcoder.hip):
//
//   k_dequant_box   the corner box of the coefficient array gathered out of the quantized planes: for every run (y, z) of the
//                   box, bx bytes of each plane at (y + ny*z)*nx -> bx doubles, contiguous.  Nothing else of a plane is read:
//                   outside the segments a low-resolution decode has launched the plane buffers hold whatever was there.
//   k_scale         the finish: out = in * s, fp64 or narrowed to fp32
//
// Strict IEEE, no contraction (-ffp-contract=off): the sums are dequant_accum's, term by term.
#include "wr_kernels.h"

namespace wrk {

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 8192;

// a / b where a fits 32 bits almost always (a 64-bit division is a long subroutine on this hardware)
__device__ inline size_t div_small(size_t a, uint32_t b) { return (a >> 32) ? a / b : (size_t)((uint32_t)a / b); }

unsigned grid_for(size_t items)
{
    const size_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

// One item is V consecutive symbols of one run: item g is group g % gpr of run g / gpr, and -- the box being contiguous with
// bx = gpr * V -- its doubles start at box[g * V], so runs shorter than a wave share it.  V = 4: one 4-byte load per plane and
// two 16-byte stores; needs nx, bx multiples of 4 and 4-byte aligned chunks (a chunk is a multiple of 4096 bytes: a group never
// straddles two).  V = 1: the byte path, any shape.
template <int V>
__global__ __launch_bounds__(kThreads) void k_dequant_box(double* __restrict__ box, size_t items, uint32_t gpr, uint32_t by, uint32_t nx, uint32_t ny,
                                                          DequantParams p)
{
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < items; g += (size_t)gridDim.x * kThreads) {
        const size_t run = div_small(g, gpr);
        const uint32_t xg = (uint32_t)(g - run * gpr);
        const size_t z = div_small(run, by);
        const size_t y = run - z * by;
        const size_t at = (y + (size_t)ny * z) * nx + (size_t)xg * V;
        if constexpr (V == 4) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int l = 0; l < 8; l++) {
                if (l < p.nlay) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(p.q[l].at(at));
                    a0 = a0 + ((double)(w & 0xff) * p.deps[l] + p.minval[l]);
                    a1 = a1 + ((double)((w >> 8) & 0xff) * p.deps[l] + p.minval[l]);
                    a2 = a2 + ((double)((w >> 16) & 0xff) * p.deps[l] + p.minval[l]);
                    a3 = a3 + ((double)(w >> 24) * p.deps[l] + p.minval[l]);
                }
            }
            double2* const o = reinterpret_cast<double2*>(box + g * 4);
            o[0] = make_double2(a0, a1);
            o[1] = make_double2(a2, a3);
        } else {
            double a = 0.0;
#pragma unroll
            for (int l = 0; l < 8; l++)
                if (l < p.nlay) a = a + ((double)*p.q[l].at(at) * p.deps[l] + p.minval[l]);
            box[g] = a;
        }
    }
}

template <typename T>
struct Pair;
template <>
struct Pair<double> { using type = double2; };
template <>
struct Pair<float> { using type = float2; };

// (src and dst may be the same array in the fp64 form: every element is read and written by one lane)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_scale(const double* src, T* dst, size_t n, double s)
{
    using T2 = typename Pair<T>::type;
    const size_t n2 = n >> 1;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n2; i += (size_t)gridDim.x * kThreads) {
        const double2 v = reinterpret_cast<const double2*>(src)[i];
        T2 o;
        o.x = (T)(v.x * s);
        o.y = (T)(v.y * s);
        reinterpret_cast<T2*>(dst)[i] = o;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = (T)(src[n - 1] * s);
}

}  // namespace

void dequant_box(double* box, int bx, int by, int bz, int nx, int ny, const DequantParams& p, hipStream_t st)
{
    bool wide = nx % 4 == 0 && bx % 4 == 0 && ((uintptr_t)box & 15) == 0;
    for (int l = 0; l < p.nlay; l++) {
        if (p.q[l].shift < 12) wide = false;
        for (int k = 0; k < kPlaneChunks; k++) wide = wide && ((uintptr_t)p.q[l].chunk[k] & 3) == 0;
    }
    const size_t elems = (size_t)bx * by * bz;
    if (!elems) return;
    if (wide)
        hipLaunchKernelGGL(k_dequant_box<4>, dim3(grid_for(elems / 4)), dim3(kThreads), 0, st, box, elems / 4, (uint32_t)(bx / 4), (uint32_t)by, (uint32_t)nx,
                           (uint32_t)ny, p);
    else
        hipLaunchKernelGGL(k_dequant_box<1>, dim3(grid_for(elems)), dim3(kThreads), 0, st, box, elems, (uint32_t)bx, (uint32_t)by, (uint32_t)nx, (uint32_t)ny,
                           p);
}

void scale_f64(const double* src, double* dst, size_t n, double s, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_scale<double>, dim3(grid_for((n + 1) / 2)), dim3(kThreads), 0, st, src, dst, n, s);
}

void scale_narrow_f64(const double* src, float* dst, size_t n, double s, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_scale<float>, dim3(grid_for((n + 1) / 2)), dim3(kThreads), 0, st, src, dst, n, s);
}

}  // namespace wrk
