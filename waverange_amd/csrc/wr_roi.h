// wr_roi.h -- the geometry of a region-of-interest decode (include/waverange_amd.h, "region decode"), host only.
//
// Lifting is local: with d levels still to invert, a sample of the result depends on coefficients within a bounded distance
// only, so a region [lo, hi) can be inverted inside a window [a, b) of the level-r box.  Per axis (n the box's extent):
//   d = 0: a = lo, b = hi
//   else   m(0) = 0, m(k) = 2 (m(k-1) + 2)   (every inverse level spoils at most 2 pairs beyond what a cut edge had spoilt)
//          a = floor(max(0, lo - m(d)) / 2^d) * 2^d,  b = ceil((hi + m(d)) / 2^d) * 2^d, n where that reaches or passes n
// A window starts on a multiple of 2^d and ends on one or on the field's true end, so its level extents
// w_l = ceil(b / 2^l) - a / 2^l follow the field's ceil chain and pair parity is the field's at every level:
// waveletcdf97_3d(wx, wy, wz, -d) inverts the window's coefficients, in the Mallat layout of the window's own extents, as
// it stands.  Those coefficients are the low-pass box of level d plus up to seven detail octants per level of the field's
// array, cut to the window: at most 1 + 7 * 4 source boxes (`Geometry::box`).  The map is not separable per axis: a point that
// is a level-l detail in one direction takes its other two coordinates at level-l granularity too.
#pragma once
#include <vector>

#include "../../include/waverange_amd.h"
#include "wr_lowres.h"

namespace wrroi {

constexpr int kMaxBoxes = 1 + 7 * wrlow::kMaxLevel;

inline int margin(int d)
{
    int m = 0;
    for (int k = 0; k < d; k++) m = 2 * (m + 2);
    return m;
}

inline int ceil_shift(int v, int l) { return (int)(((long long)v + ((1ll << l) - 1)) >> l); }

struct Axis {
    int n;       // extent of the level-r box
    int lo, hi;  // the region
    int a, b;    // the window
    int w[wrlow::kMaxLevel + 1];   // w_l, l = 0..d: the window's extent at level l
    int nl[wrlow::kMaxLevel + 1];  // h^l(n)
};

inline Axis axis_of(int n, int lo, int hi, int d)
{
    Axis ax{};
    ax.n = n; ax.lo = lo; ax.hi = hi;
    if (d == 0) {
        ax.a = lo; ax.b = hi;
    } else {
        const long long m = margin(d), A = 1ll << d;
        ax.a = (int)((lo - m > 0 ? lo - m : 0) / A * A);
        const long long b = (hi + m + A - 1) / A * A;
        ax.b = b >= n ? n : (int)b;
    }
    for (int l = 0; l <= d; l++) {
        ax.w[l] = ceil_shift(ax.b, l) - (ax.a >> l);
        ax.nl[l] = ceil_shift(n, l);
    }
    return ax;
}

// one source box: `len` coefficients per axis from `src` of the field's array land at `dst` of the window (x, y, z)
struct SrcBox { int src[3], dst[3], len[3]; };

struct Geometry {
    int d;       // levels still to invert
    Axis ax[3];  // x, y, z
    int nbox;
    SrcBox box[kMaxBoxes];
    int w(int axis) const { return ax[axis].w[0]; }
    size_t elems() const { return (size_t)w(0) * w(1) * w(2); }
    size_t out_elems() const { return (size_t)(ax[0].hi - ax[0].lo) * (ax[1].hi - ax[1].lo) * (ax[2].hi - ax[2].lo); }
};

inline bool roi_ok(const wrlow::Box& b, const wr_box& r)
{
    return r.x0 >= 0 && r.x0 < r.x1 && r.x1 <= b.bx && r.y0 >= 0 && r.y0 < r.y1 && r.y1 <= b.by && r.z0 >= 0 && r.z0 < r.z1 && r.z1 <= b.bz;
}

// b: the box of level r; d = wlev - r; roi inside the box (roi_ok)
inline Geometry geometry_of(const wrlow::Box& b, int d, const wr_box& roi)
{
    Geometry g{};
    g.d = d;
    g.ax[0] = axis_of(b.bx, roi.x0, roi.x1, d);
    g.ax[1] = axis_of(b.by, roi.y0, roi.y1, d);
    g.ax[2] = axis_of(b.bz, roi.z0, roi.z1, d);
    SrcBox low{};
    for (int k = 0; k < 3; k++) { low.src[k] = g.ax[k].a >> d; low.dst[k] = 0; low.len[k] = g.ax[k].w[d]; }
    g.box[g.nbox++] = low;
    for (int l = d; l >= 1; l--)
        for (int oct = 1; oct < 8; oct++) {  // bit k set: the high half in direction k
            SrcBox s{};
            bool empty = false;
            for (int k = 0; k < 3; k++) {
                const Axis& ax = g.ax[k];
                if (oct >> k & 1) { s.src[k] = ax.nl[l] + (ax.a >> l); s.dst[k] = ax.w[l]; s.len[k] = ax.w[l - 1] - ax.w[l]; }
                else { s.src[k] = ax.a >> l; s.dst[k] = 0; s.len[k] = ax.w[l]; }
                empty = empty || s.len[k] <= 0;
            }
            if (!empty) g.box[g.nbox++] = s;
        }
    return g;
}

// need[k] = true for every segment of length `seg` that the source boxes' x-runs touch in a plane of an nx * ny * nz field
// (need has one entry per segment of the plane; marks that are set stay set, so several regions can share one array)
inline void mark_segments(int nx, int ny, const Geometry& g, uint32_t seg, std::vector<bool>* need)
{
    for (int i = 0; i < g.nbox; i++) {
        const SrcBox& s = g.box[i];
        for (int z = s.src[2]; z < s.src[2] + s.len[2]; z++)
            for (int y = s.src[1]; y < s.src[1] + s.len[1]; y++) {
                const size_t at = ((size_t)y + (size_t)ny * z) * nx + s.src[0];
                for (size_t k = at / seg; k <= (at + s.len[0] - 1) / seg; k++) (*need)[k] = true;
            }
    }
}

// the marked ids, ascending: the first `cap` of them go to ids (if it is not null), the count of all of them is returned
inline size_t list_marks(const std::vector<bool>& need, uint32_t* ids, size_t cap)
{
    size_t count = 0;
    for (size_t k = 0; k < need.size(); k++)
        if (need[k]) {
            if (ids && count < cap) ids[count] = (uint32_t)k;
            count++;
        }
    return count;
}

// The ascending ids of the segments of length `seg` that the source boxes' x-runs touch in a plane of an nx * ny * nz field;
// conventions of wrlow::segments_of.
inline size_t segments_of(int nx, int ny, int nz, const Geometry& g, uint32_t seg, uint32_t* ids, size_t cap)
{
    std::vector<bool> need(((size_t)nx * ny * nz + seg - 1) / seg, false);
    mark_segments(nx, ny, g, seg, &need);
    return list_marks(need, ids, cap);
}

// the ascending union of segments_of over the regions g[0, ng)
inline size_t segments_of_multi(int nx, int ny, int nz, const Geometry* g, size_t ng, uint32_t seg, uint32_t* ids, size_t cap)
{
    std::vector<bool> need(((size_t)nx * ny * nz + seg - 1) / seg, false);
    for (size_t i = 0; i < ng; i++) mark_segments(nx, ny, g[i], seg, &need);
    return list_marks(need, ids, cap);
}

}  // namespace wrroi
