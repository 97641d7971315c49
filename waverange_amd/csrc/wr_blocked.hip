// wr_blocked.hip -- the permutation between a plane's natural order and the blocked order of a WRS2 stream (wr_blocked.h).
//
//   k_plane_reorder<inverse, list>   forward: blocked[p] = natural[pi(p)]; inverse: natural[pi(p)] = blocked[p]
//
// The kernel is pure traffic (n bytes in, n bytes out), so the access shape is the design.  A work item is a GROUP of bricks
// that follow each other along x in one box: 128 / B of them (4 at B = 32), so a row of the group is 128 consecutive bytes of
// the natural plane -- one line where the box's origin and nx are multiples of 128, as in a 1024^3 field -- and B consecutive
// bytes of each brick on the blocked side, where the rows of a brick follow each other.  A workgroup of 256 lanes takes one
// item.  On the wide path a lane moves 16 bytes; 8 neighbouring lanes cover a row of the group and a wave 8 rows, so one wave
// instruction touches 8 whole lines on the natural side and, per brick, 8 * B consecutive bytes (two whole lines at B = 32) on
// the blocked side: one line request per 128 payload bytes on either side, none of it partial.  With a list the items are
// single bricks (nothing outside a listed brick may be touched): B / 16 lanes cover a row, a wave 1 KiB of consecutive
// blocked bytes and 64 / (B / 16) pieces of B bytes of the natural plane (at B = 32 a quarter of each line it requests).
// A box goes the wide way when B >= 16 and its origin in x, its extent in x, nx and its start in the stream are multiples of
// 16 (then every brick offset is one too); otherwise lane by lane, a byte each, in the same shape (the byte path).
#include <string.h>

#include "wr_blocked.h"
#include "wr_kernels.h"

namespace wrk {

namespace {

constexpr int kThreads = 256;

// Moves the rows of one item.  U: bytes per lane (16 or 1); cs: log2 of the lanes that cover a row of the item; W: the row's
// length in bytes (a multiple of U); hy, hz: the bricks' extents; at0: the natural index of the item's first byte; pos0: the
// stream position of its first brick.
template <bool kInverse, int U>
__device__ inline void move_rows(const PlaneRef& nat, uint8_t* blk, uint32_t cs, uint32_t W, uint32_t B, uint32_t lb, uint32_t hy, uint32_t hz,
                                 size_t at0, size_t pitch_y, size_t pitch_z, unsigned long long pos0)
{
    const uint32_t x = (threadIdx.x & ((1u << cs) - 1)) * U;  // the lane's place in the row
    if (x >= W) return;
    const uint32_t rr = threadIdx.x >> cs, rows = kThreads >> cs;  // the lane's row in a step, rows per step
    // rows of a step: yb consecutive y (a power of two), then the next z
    const uint32_t yb = B < rows ? B : rows, lyb = B < rows ? lb : 31 - __clz(rows);
    const uint32_t y0 = rr & (yb - 1), z0 = rr >> lyb, zstep = rows >> lyb;
    const uint32_t t = x >> lb, lx = x & (B - 1);        // the brick of the group and the place in its row
    const uint32_t left = W - (t << lb), hx = left < B ? left : B;
    const unsigned long long brick0 = pos0 + (unsigned long long)hy * hz * (t << lb) + lx;
    // four rows in flight per lane: the loads of a batch are issued before its stores
    for (uint32_t y = y0; y < hy; y += yb)
        for (uint32_t z = z0; z < hz; z += 4 * zstep) {
            uint4 v[4];
            uint8_t b1[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t zk = z + k * zstep;
                if (zk >= hz) break;
                const uint8_t* const pn = nat.at(at0 + zk * pitch_z + y * pitch_y + x);
                const uint8_t* const pb = blk + brick0 + (unsigned long long)hx * (y + (unsigned long long)hy * zk);
                if (U == 16) v[k] = *reinterpret_cast<const uint4*>(kInverse ? pb : pn);
                else b1[k] = *(kInverse ? pb : pn);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t zk = z + k * zstep;
                if (zk >= hz) break;
                uint8_t* const pn = nat.at(at0 + zk * pitch_z + y * pitch_y + x);
                uint8_t* const pb = blk + brick0 + (unsigned long long)hx * (y + (unsigned long long)hy * zk);
                if (U == 16) *reinterpret_cast<uint4*>(kInverse ? pn : pb) = v[k];
                else *(kInverse ? pn : pb) = b1[k];
            }
        }
}

// kList: item = brick ids[blockIdx.x] (the map's `first` then counts bricks, group == 1); otherwise item = blockIdx.x.
template <bool kInverse, bool kList>
__global__ __launch_bounds__(kThreads) void k_plane_reorder(PlaneRef nat, uint8_t* blk, ReorderMap m, const uint32_t* ids)
{
    uint32_t item = blockIdx.x;
    if (kList) item = ids[item];
    if (item >= m.items) return;
    int b = 0;
    while (b + 1 < m.nbox && item >= m.box[b + 1].first) b++;
    const ReorderBox bx = m.box[b];
    const uint32_t B = m.brick, lb = 31 - __clz(B), G = kList ? 1 : m.group;
    const uint32_t ntx = (bx.ex + B - 1) >> lb, nty = (bx.ey + B - 1) >> lb, ngx = (ntx + G - 1) / G;
    uint32_t r = item - bx.first;
    const uint32_t gx = r % ngx;
    r /= ngx;
    const uint32_t ty = r % nty, tz = r / nty;
    if (((size_t)tz << lb) >= bx.ez) return;
    const uint32_t hz = bx.ez - (tz << lb) < B ? bx.ez - (tz << lb) : B, hy = bx.ey - (ty << lb) < B ? bx.ey - (ty << lb) : B;
    const uint32_t x0 = gx * G * B, W = bx.ex - x0 < G * B ? bx.ex - x0 : G * B;
    const unsigned long long pos0 = bx.start + (unsigned long long)(tz << lb) * bx.ex * bx.ey +
                                    (unsigned long long)hz * ((unsigned long long)(ty << lb) * bx.ex + (unsigned long long)hy * x0);
    const size_t at0 = ((size_t)(bx.oy + (ty << lb)) + (size_t)m.ny * (bx.oz + (tz << lb))) * m.nx + bx.ox + x0;
    const uint32_t lgb = 31 - __clz(G * B);  // a row of the item is at most 2^lgb bytes
    if (bx.wide) move_rows<kInverse, 16>(nat, blk, lgb - 4, W, B, lb, hy, hz, at0, m.nx, (size_t)m.nx * m.ny, pos0);
    else move_rows<kInverse, 1>(nat, blk, lgb, W, B, lb, hy, hz, at0, m.nx, (size_t)m.nx * m.ny, pos0);
}

}  // namespace

bool plane_reorder(const PlaneRef& nat, uint8_t* blk, const wrblk::Order& od, bool inverse, const uint32_t* ids, size_t nlist, hipStream_t st)
{
    const bool list = ids != nullptr;
    ReorderMap m;
    memset(&m, 0, sizeof m);
    m.nbox = od.nbox;
    m.nx = (uint32_t)od.nx; m.ny = (uint32_t)od.ny; m.brick = od.B;
    m.group = reorder_group(od.B, list);
    bool aligned = ((uintptr_t)blk & 15) == 0 && nat.shift >= 12;
    for (int k = 0; k < kPlaneChunks; k++) aligned = aligned && ((uintptr_t)nat.chunk[k] & 15) == 0;
    uint64_t first = 0;
    for (int i = 0; i < od.nbox; i++) {
        const wrblk::Box& b = od.box[i];
        ReorderBox& r = m.box[i];
        r.ox = (uint32_t)b.o[0]; r.oy = (uint32_t)b.o[1]; r.oz = (uint32_t)b.o[2];
        r.ex = (uint32_t)b.e[0]; r.ey = (uint32_t)b.e[1]; r.ez = (uint32_t)b.e[2];
        r.first = (uint32_t)first;
        r.wide = reorder_box_wide(aligned, od, b);
        r.start = b.start;
        first += reorder_box_items(b, m.group);
    }
    if (first > 0x7fffffffu || nlist > 0x7fffffffu) return false;  // more work items than a grid has blocks: nothing is launched
    m.items = (uint32_t)first;
    const size_t grid = list ? nlist : (size_t)first;
    if (!grid) return true;
    if (inverse) {
        if (list) hipLaunchKernelGGL((k_plane_reorder<true, true>), dim3((unsigned)grid), dim3(kThreads), 0, st, nat, blk, m, ids);
        else hipLaunchKernelGGL((k_plane_reorder<true, false>), dim3((unsigned)grid), dim3(kThreads), 0, st, nat, blk, m, ids);
    } else {
        if (list) hipLaunchKernelGGL((k_plane_reorder<false, true>), dim3((unsigned)grid), dim3(kThreads), 0, st, nat, blk, m, ids);
        else hipLaunchKernelGGL((k_plane_reorder<false, false>), dim3((unsigned)grid), dim3(kThreads), 0, st, nat, blk, m, ids);
    }
    return true;
}

}  // namespace wrk
