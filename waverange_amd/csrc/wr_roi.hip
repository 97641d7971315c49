// wr_roi.hip -- the kernels of a region decode (include/waverange_amd.h, "region decode"; the geometry: wr_roi.h):
//
//   k_dequant_window  the window's coefficient array gathered out of the quantized planes: the low-pass box of the coarsest
//                     level and up to seven detail octants per level, each a box of x-runs of the field's array that lands
//                     as a box of the window (WindowMap).  Items are numbered through all boxes, so the short runs of the
//                     coarse levels share waves.  Nothing outside those runs is read: outside the segments a region decode has
//                     launched the plane buffers hold whatever was there.
//   k_crop_scale      the finish: out = (T)(window[crop] * s), the crop stored contiguously
//
// Strict IEEE, no contraction (-ffp-contract=off): the sums are dequant_accum's, term by term.
#include <string.h>

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

// How the items are dealt out: box b owns the items [first[b], first[b + 1]); item i of a box is group i % gpr of its run
// i / gpr, run j is row (j % ly, j / ly) of the box.  A group is 4 consecutive symbols (one 4-byte load per plane, two 16-byte
// stores) where the box is `wide`: the run's offsets in the plane and in the window and its length are multiples of 4 (a
// chunk of a plane is a multiple of 4096 bytes: a group never straddles two).  Otherwise it is one symbol: the byte path.
struct WindowItems {
    size_t first[kWindowBoxes + 1];
    uint32_t gpr[kWindowBoxes];
    uint8_t wide[kWindowBoxes];
};

__global__ __launch_bounds__(kThreads) void k_dequant_window(double* __restrict__ win, WindowMap m, WindowItems it, DequantParams p)
{
    const size_t items = it.first[m.nbox];
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < items; g += (size_t)gridDim.x * kThreads) {
        int b = 0;
        while (b + 1 < m.nbox && g >= it.first[b + 1]) b++;
        const WindowBox bx = m.box[b];
        const size_t i = g - it.first[b];
        const size_t run = div_small(i, it.gpr[b]);
        const uint32_t xg = (uint32_t)(i - run * it.gpr[b]);
        const size_t z = div_small(run, bx.ly);
        const size_t y = run - z * bx.ly;
        const uint32_t v = it.wide[b] ? 4 : 1;
        const size_t at = ((bx.sy + y) + (size_t)m.ny * (bx.sz + z)) * m.nx + bx.sx + (size_t)xg * v;
        const size_t to = ((bx.oz + z) * m.wy + (bx.oy + y)) * m.wx + bx.ox + (size_t)xg * v;
        if (it.wide[b]) {
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
            double2* const o = reinterpret_cast<double2*>(win + to);
            o[0] = make_double2(a0, a1);
            o[1] = make_double2(a2, a3);
        } else {
            double a = 0.0;
#pragma unroll
            for (int l = 0; l < 8; l++)
                if (l < p.nlay) a = a + ((double)*p.q[l].at(at) * p.deps[l] + p.minval[l]);
            win[to] = a;
        }
    }
}

// out[(z * cy + y) * cx + x] = (T)(win[((z + oz) * wy + (y + oy)) * wx + (x + ox)] * s); s == 1 copies the bits
template <typename T>
__global__ __launch_bounds__(kThreads) void k_crop_scale(const double* __restrict__ win, T* __restrict__ out, size_t n, uint32_t wx, uint32_t wy,
                                                        uint32_t ox, uint32_t oy, uint32_t oz, uint32_t cx, uint32_t cy, double s)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const size_t row = div_small(i, cx);
        const uint32_t x = (uint32_t)(i - row * cx);
        const size_t z = div_small(row, cy);
        const size_t y = row - z * cy;
        const double v = win[((z + oz) * wy + (y + oy)) * wx + (x + ox)];
        out[i] = (T)(s == 1.0 ? v : v * s);
    }
}

template <typename T>
void crop_scale(const double* win, T* out, const CropBox& c, double s, hipStream_t st)
{
    const size_t n = (size_t)c.cx * c.cy * c.cz;
    if (n)
        hipLaunchKernelGGL(k_crop_scale<T>, dim3(grid_for(n)), dim3(kThreads), 0, st, win, out, n, c.wx, c.wy, c.ox, c.oy, c.oz, c.cx, c.cy, s);
}

}  // namespace

void dequant_window(double* win, const WindowMap& m, const DequantParams& p, hipStream_t st)
{
    bool aligned = ((uintptr_t)win & 15) == 0;
    for (int l = 0; l < p.nlay; l++) {
        if (p.q[l].shift < 12) aligned = false;
        for (int k = 0; k < kPlaneChunks; k++) aligned = aligned && ((uintptr_t)p.q[l].chunk[k] & 3) == 0;
    }
    WindowItems it;
    memset(&it, 0, sizeof it);
    for (int b = 0; b < m.nbox; b++) {
        const WindowBox& x = m.box[b];
        it.wide[b] = window_box_wide(aligned, m, x);
        it.gpr[b] = it.wide[b] ? x.lx / 4 : x.lx;
        it.first[b + 1] = it.first[b] + (size_t)it.gpr[b] * x.ly * x.lz;
    }
    const size_t items = it.first[m.nbox];
    if (items) hipLaunchKernelGGL(k_dequant_window, dim3(grid_for(items)), dim3(kThreads), 0, st, win, m, it, p);
}

void crop_scale_f64(const double* win, double* out, const CropBox& c, double s, hipStream_t st) { crop_scale<double>(win, out, c, s, st); }

void crop_scale_narrow_f64(const double* win, float* out, const CropBox& c, double s, hipStream_t st) { crop_scale<float>(win, out, c, s, st); }

}  // namespace wrk
