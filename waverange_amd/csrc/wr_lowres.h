// wr_lowres.h -- the geometry of a reduced-resolution decode (include/waverange_amd.h, "low-resolution decode"), host only.
//
// The transform (waveletcdf97_3d.c:73-78) is a Mallat decomposition: after level r the low-pass coefficients of an
// nx*ny*nz field sit in the corner box [0,bx) x [0,by) x [0,bz) of the coefficient array, b = h^r(n), h(n) = (n + 1) / 2.
// With x fastest the box is by*bz runs of bx symbols of every plane, run (y, z) at offset (y + ny*z) * nx; a plane cut into
// segments of `seg` symbols needs the segments those runs touch and no others.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace wrlow {

constexpr int kMaxLevel = 4;  // the codec's transform depth (defs.h: WAV_LVL)

inline int half_up(int n) { return (n + 1) / 2; }

struct Box {
    int bx, by, bz;
    int e;  // transformed axes summed over the levels 1..r: the box carries a gain of 2^(e/2)
    size_t elems() const { return (size_t)bx * by * bz; }
    size_t rows() const { return (size_t)by * bz; }
};

inline bool level_ok(int level) { return level >= 0 && level <= kMaxLevel; }

// the box of level r (0 <= r <= kMaxLevel) of a field with positive extents
inline Box box_of(int nx, int ny, int nz, int level)
{
    Box b{nx, ny, nz, 0};
    for (int j = 0; j < level; j++) {
        b.e += (b.bx > 1) + (b.by > 1) + (b.bz > 1);  // an axis of extent 1 is not transformed at this level
        b.bx = half_up(b.bx); b.by = half_up(b.by); b.bz = half_up(b.bz);
    }
    return b;
}

// 2^(-e/2): what brings the box back to the field's range
inline double scale_of(const Box& b) { return ldexp((b.e & 1) ? 0x1.6a09e667f3bcdp-1 : 1.0, -(b.e / 2)); }

// The ascending ids of the segments of length `seg` that the box's runs touch; at most `cap` of them are written to ids
// (nullptr: none), the number of all of them is returned.  The runs ascend in the plane, so do the segments they touch.
inline size_t segments_of(int nx, int ny, const Box& b, uint32_t seg, uint32_t* ids, size_t cap)
{
    size_t count = 0, next = 0;  // next: the first segment not yet listed
    for (int z = 0; z < b.bz; z++)
        for (int y = 0; y < b.by; y++) {
            const size_t at = ((size_t)y + (size_t)ny * z) * nx;
            size_t k = at / seg;
            const size_t last = (at + b.bx - 1) / seg;
            if (k < next) k = next;
            for (; k <= last; k++) {
                if (ids && count < cap) ids[count] = (uint32_t)k;
                count++;
            }
            next = last + 1;
        }
    return count;
}

}  // namespace wrlow
