// wr_blocked.h -- the blocked symbol order of a segmented plane stream ("WRS2", include/waverange_amd.h), host only.
//
// A plane is written subband by subband and inside a subband in bricks of B^3: first the low-pass box [0, e_wlev)^3, then for
// l = wlev .. 1 the seven detail octants of level l (bit 0 / 1 / 2 of the octant: x / y / z takes the high part [e_l, e_{l-1})),
// e_0 = n, e_l = h(e_{l-1}), h(n) = (n + 1) / 2.  A box with an empty axis contributes nothing.  The bricks of a box come in
// (tz, ty, tx) order, tx fastest; a partial brick at a high edge holds exactly its hx*hy*hz symbols; inside a brick x is fastest,
// then y, then z.  This is a permutation pi of [0, n): stream position -> coefficient index fx + nx * (fy + ny * fz).
//
// The boxes of the levels above r tile the box of level r, so that box is a prefix of the stream, for every r <= wlev.
//
// The stream position of a point has a closed form.  In a box of extents (ex, ey, ez) that starts at stream position `start`,
// brick (tx, ty, tz) with hy, hz its extents in y and z begins at
//   start + tz*B*ex*ey + hz * (ty*B*ex + hy * tx*B)
// (whole slabs of bricks below it, whole rows of bricks in front of it in its slab, whole bricks -- all of width B -- in front
// of it in its row), and the point (lx, ly, lz) of a brick that is hx wide sits lx + hx * (ly + hy * lz) behind that.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wr_roi.h"

namespace wrblk {

constexpr int kMaxBoxes = 1 + 7 * wrlow::kMaxLevel;
constexpr uint32_t kBrickDefault = 32;

inline bool brick_ok(uint32_t b) { return b == 8 || b == 16 || b == 32 || b == 64; }

struct Box {
    int o[3], e[3];        // origin and extents in the coefficient array (x, y, z)
    int level;             // the level whose octant it is; wlev + 1 for the low-pass box
    uint32_t t[3];         // bricks per axis
    uint64_t start;        // stream position of its first symbol
    uint64_t first_brick;  // id of its first brick
    size_t elems() const { return (size_t)e[0] * e[1] * e[2]; }
    uint64_t bricks() const { return (uint64_t)t[0] * t[1] * t[2]; }
};

struct Order {
    int nx, ny, nz, wlev;
    uint32_t B;
    int nbox;
    Box box[kMaxBoxes];
    uint64_t nbricks;
    size_t n() const { return (size_t)nx * ny * nz; }
};

// nx, ny, nz >= 1; wlev in [0, kMaxLevel]; brick_ok(B)
inline Order order_of(int nx, int ny, int nz, int wlev, uint32_t B)
{
    Order od{};
    od.nx = nx; od.ny = ny; od.nz = nz; od.wlev = wlev; od.B = B;
    int e[wrlow::kMaxLevel + 1][3] = {{nx, ny, nz}};
    for (int l = 1; l <= wlev; l++)
        for (int k = 0; k < 3; k++) e[l][k] = wrlow::half_up(e[l - 1][k]);
    uint64_t start = 0, brick = 0;
    auto add = [&](const int* o, const int* x, int level) {
        if (x[0] <= 0 || x[1] <= 0 || x[2] <= 0) return;
        Box& b = od.box[od.nbox++];
        for (int k = 0; k < 3; k++) { b.o[k] = o[k]; b.e[k] = x[k]; b.t[k] = ((uint32_t)x[k] + B - 1) / B; }
        b.level = level; b.start = start; b.first_brick = brick;
        start += b.elems();
        brick += b.bricks();
    };
    const int zero[3] = {0, 0, 0};
    add(zero, e[wlev], wlev + 1);
    for (int l = wlev; l >= 1; l--)
        for (int oct = 1; oct < 8; oct++) {
            int o[3], x[3];
            for (int k = 0; k < 3; k++) {
                if (oct >> k & 1) { o[k] = e[l][k]; x[k] = e[l - 1][k] - e[l][k]; }
                else { o[k] = 0; x[k] = e[l][k]; }
            }
            add(o, x, l);
        }
    od.nbricks = brick;
    return od;
}

// the boxes that make up the box of level r (r <= wlev): the first prefix_boxes(od, r) of them
inline int prefix_boxes(const Order& od, int r)
{
    int k = 0;
    while (k < od.nbox && od.box[k].level > r) k++;
    return k;
}

inline uint32_t brick_extent(int e, uint32_t t, uint32_t B) { const uint32_t left = (uint32_t)e - t * B; return left < B ? left : B; }

// stream position of the first symbol of brick (tx, ty, tz) of a box
inline uint64_t brick_start(const Box& b, uint32_t B, uint32_t tx, uint32_t ty, uint32_t tz)
{
    const uint64_t hy = brick_extent(b.e[1], ty, B), hz = brick_extent(b.e[2], tz, B);
    return b.start + (uint64_t)tz * B * b.e[0] * b.e[1] + hz * ((uint64_t)ty * B * b.e[0] + hy * ((uint64_t)tx * B));
}

// Every x-run of every brick, in stream order: f(stream position, coefficient index, length).
template <class F>
inline void for_each_run(const Order& od, F f)
{
    const uint32_t B = od.B;
    for (int i = 0; i < od.nbox; i++) {
        const Box& b = od.box[i];
        uint64_t pos = b.start;
        for (uint32_t tz = 0; tz < b.t[2]; tz++)
            for (uint32_t ty = 0; ty < b.t[1]; ty++)
                for (uint32_t tx = 0; tx < b.t[0]; tx++) {
                    const uint32_t hx = brick_extent(b.e[0], tx, B), hy = brick_extent(b.e[1], ty, B), hz = brick_extent(b.e[2], tz, B);
                    for (uint32_t z = 0; z < hz; z++)
                        for (uint32_t y = 0; y < hy; y++) {
                            const size_t at = ((size_t)(b.o[1] + ty * B + y) + (size_t)od.ny * (b.o[2] + tz * B + z)) * od.nx + b.o[0] + tx * B;
                            f(pos, at, hx);
                            pos += hx;
                        }
                }
    }
}

// pi[stream position] = coefficient index; n() entries
inline void fill_order(const Order& od, uint64_t* pi)
{
    for_each_run(od, [&](uint64_t pos, size_t at, uint32_t len) {
        for (uint32_t x = 0; x < len; x++) pi[pos + x] = at + x;
    });
}

// forward: blocked[p] = natural[pi[p]]; inverse: natural[pi[p]] = blocked[p].  n() bytes each, not in place.
inline void reorder_host(const Order& od, const uint8_t* src, uint8_t* dst, bool inverse)
{
    for_each_run(od, [&](uint64_t pos, size_t at, uint32_t len) {
        if (inverse) memcpy(dst + at, src + pos, len);
        else memcpy(dst + pos, src + at, len);
    });
}

// the segments of the box of level r: the prefix
inline size_t lowres_segments(int nx, int ny, int nz, int level, uint32_t seg, uint32_t* ids, size_t cap)
{
    const size_t count = (wrlow::box_of(nx, ny, nz, level).elems() + seg - 1) / seg;
    for (size_t k = 0; ids && k < count && k < cap; k++) ids[k] = (uint32_t)k;
    return count;
}

// What a region needs of a blocked plane: the bricks the source boxes of the window (wrroi::geometry_of) meet, and -- seg != 0
// -- the segments that the parts of those boxes' x-runs inside each brick fall into.  Both marks are indexed by id; either may
// be nullptr.  A source box is an octant of a level cut to the window, so it lies inside one box of the order; the
// intersection is taken with all of them all the same.
inline void region_touch(const Order& od, const wrroi::Geometry& g, uint32_t seg, std::vector<bool>* need_seg, std::vector<bool>* need_brick)
{
    const uint32_t B = od.B;
    for (int i = 0; i < g.nbox; i++) {
        const wrroi::SrcBox& s = g.box[i];
        for (int j = 0; j < od.nbox; j++) {
            const Box& b = od.box[j];
            uint32_t lo[3], hi[3];  // the intersection, in the box's own coordinates
            bool empty = false;
            for (int k = 0; k < 3; k++) {
                const int a = s.src[k] > b.o[k] ? s.src[k] : b.o[k];
                const int e = s.src[k] + s.len[k] < b.o[k] + b.e[k] ? s.src[k] + s.len[k] : b.o[k] + b.e[k];
                if (a >= e) { empty = true; break; }
                lo[k] = (uint32_t)(a - b.o[k]); hi[k] = (uint32_t)(e - b.o[k]);
            }
            if (empty) continue;
            for (uint32_t tz = lo[2] / B; tz <= (hi[2] - 1) / B; tz++)
                for (uint32_t ty = lo[1] / B; ty <= (hi[1] - 1) / B; ty++)
                    for (uint32_t tx = lo[0] / B; tx <= (hi[0] - 1) / B; tx++) {
                        if (need_brick) (*need_brick)[b.first_brick + ((uint64_t)tz * b.t[1] + ty) * b.t[0] + tx] = true;
                        if (!need_seg) continue;
                        const uint32_t hx = brick_extent(b.e[0], tx, B), hy = brick_extent(b.e[1], ty, B), hz = brick_extent(b.e[2], tz, B);
                        const uint32_t c0[3] = {tx * B, ty * B, tz * B}, h[3] = {hx, hy, hz};
                        uint32_t a[3], e[3];  // the part inside the brick, in the brick's coordinates
                        for (int k = 0; k < 3; k++) {
                            a[k] = lo[k] > c0[k] ? lo[k] - c0[k] : 0;
                            e[k] = hi[k] - c0[k] < h[k] ? hi[k] - c0[k] : h[k];
                        }
                        const uint64_t at = brick_start(b, B, tx, ty, tz);
                        for (uint32_t z = a[2]; z < e[2]; z++)
                            for (uint32_t y = a[1]; y < e[1]; y++) {
                                const uint64_t p0 = at + a[0] + (uint64_t)hx * (y + (uint64_t)hy * z), p1 = p0 + (e[0] - a[0]) - 1;
                                for (uint64_t k = p0 / seg; k <= p1 / seg; k++) (*need_seg)[k] = true;
                            }
                    }
        }
    }
}

using wrroi::list_marks;

// The ascending ids of the segments of length `seg` that a region needs of a blocked plane; conventions of wrlow::segments_of.
inline size_t region_segments(const Order& od, const wrroi::Geometry& g, uint32_t seg, uint32_t* ids, size_t cap)
{
    std::vector<bool> need((od.n() + seg - 1) / seg, false);
    region_touch(od, g, seg, &need, nullptr);
    return list_marks(need, ids, cap);
}

// the ascending ids of the bricks it needs
inline void region_bricks(const Order& od, const wrroi::Geometry& g, std::vector<uint32_t>* ids)
{
    std::vector<bool> need(od.nbricks, false);
    region_touch(od, g, 0, nullptr, &need);
    ids->resize(list_marks(need, nullptr, 0));
    list_marks(need, ids->data(), ids->size());
}

// the ascending unions of region_segments / region_bricks over the regions g[0, ng)
inline size_t region_segments_multi(const Order& od, const wrroi::Geometry* g, size_t ng, uint32_t seg, uint32_t* ids, size_t cap)
{
    std::vector<bool> need((od.n() + seg - 1) / seg, false);
    for (size_t i = 0; i < ng; i++) region_touch(od, g[i], seg, &need, nullptr);
    return list_marks(need, ids, cap);
}

inline void region_bricks_multi(const Order& od, const wrroi::Geometry* g, size_t ng, std::vector<uint32_t>* ids)
{
    std::vector<bool> need(od.nbricks, false);
    for (size_t i = 0; i < ng; i++) region_touch(od, g[i], 0, nullptr, &need);
    ids->resize(list_marks(need, nullptr, 0));
    list_marks(need, ids->data(), ids->size());
}

}  // namespace wrblk
