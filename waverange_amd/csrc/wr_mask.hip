// Masked fields on the device (wr_mask.h): split a field into a packed bit mask and the sum and count of its defined samples,
// fill the undefined ones, and put a value back where a decoded mask says so.  gfx950, wave64.
//
// All three kernels walk the field the same way: a wave takes 64 consecutive samples per turn (chunk `ch`: samples 64 ch ..
// 64 ch + 63, mask bytes 8 ch .. 8 ch + 7), lane l sample 64 ch + l, so a wave's loads are one coalesced line and __ballot of
// the undefined predicate IS the chunk's 8 mask bytes.  Chunks go round the grid's waves: wave w takes ch = w, w + W, ...
#include "wr_mask.h"

#include <float.h>

namespace wrk {

#define WR_MASK_BLOCKS 2048
#define WR_MASK_THREADS 256
#define WR_MASK_WAVES (WR_MASK_THREADS / 64)

int mask_partials() { return WR_MASK_BLOCKS; }

static int mask_grid(size_t n)
{
    const size_t nchunk = (n + 63) >> 6;
    size_t g = (nchunk + WR_MASK_WAVES - 1) / WR_MASK_WAVES;
    if (g < 1) g = 1;
    if (g > WR_MASK_BLOCKS) g = WR_MASK_BLOCKS;
    return (int)g;
}

// the block's sum and count into out[0], out[1]: shuffles 32 .. 1, then thread 0 adds the waves in order (block_max_sum_sum's scheme)
__device__ inline void block_sum_count(double s, unsigned long long cnt, double* __restrict__ out)
{
    for (int o = 32; o > 0; o >>= 1) {
        s = s + __shfl_down(s, o, 64);
        cnt += __shfl_down(cnt, o, 64);
    }
    __shared__ double ssum[WR_MASK_WAVES];
    __shared__ unsigned long long scnt[WR_MASK_WAVES];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ssum[w] = s; scnt[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WR_MASK_WAVES; i++) { s = s + ssum[i]; cnt += scnt[i]; }
        out[0] = s;
        reinterpret_cast<unsigned long long*>(out)[1] = cnt;
    }
}

// the 8 mask bytes of chunk ch as one word: bytes at and beyond nbytes read as 0
__device__ inline unsigned long long mask_word(const uint8_t* __restrict__ bits, size_t nbytes, size_t ch, bool wide)
{
    const size_t b0 = ch << 3;
    if (wide && b0 + 8 <= nbytes) return *reinterpret_cast<const unsigned long long*>(bits + b0);
    unsigned long long m = 0;
    for (int k = 0; k < 8; k++)
        if (b0 + k < nbytes) m |= (unsigned long long)bits[b0 + k] << (8 * k);
    return m;
}

// WIDE: `bits` is 8-byte aligned
template <typename T, bool WIDE>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_split(const T* __restrict__ x, size_t n, double below, uint8_t* __restrict__ bits,
                                                                  double* __restrict__ partial)
{
    double s = 0.0;
    unsigned long long cnt = 0;
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    // kTurns turns at a time: their loads are issued together (a load per lane and turn is too little in flight to fill the
    // memory pipe), the samples then go into the sum in turn order, as they would one turn at a time
    constexpr int kTurns = 4;
    for (size_t ch0 = wave; ch0 < nchunk; ch0 += kTurns * nwaves) {
        T v[kTurns];
        bool have[kTurns];
#pragma unroll
        for (int u = 0; u < kTurns; u++) {
            const size_t ch = ch0 + u * nwaves, i = (ch << 6) + lane;
            have[u] = ch < nchunk && i < n;
            v[u] = have[u] ? x[i] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < kTurns; u++) {
            const size_t ch = ch0 + u * nwaves;
            if (ch >= nchunk) break;  // (the whole wave)
            const double w = (double)v[u];
            const bool undef = have[u] && (!(fabs(w) <= DBL_MAX) || w < below);
            if (have[u] && !undef) { s = s + w; cnt++; }
            const unsigned long long m = __ballot(undef);
            if (lane == 0) {
                const size_t b0 = ch << 3;
                if (WIDE && b0 + 8 <= nbytes) *reinterpret_cast<unsigned long long*>(bits + b0) = m;
                else
                    for (int k = 0; k < 8; k++)
                        if (b0 + k < nbytes) bits[b0 + k] = (uint8_t)(m >> (8 * k));
            }
        }
    }
    block_sum_count(s, cnt, partial + 2 * blockIdx.x);
}

__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_split_final(const double* __restrict__ partial, int np, double* __restrict__ result)
{
    double s = 0.0;
    unsigned long long cnt = 0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        s = s + partial[2 * i];
        cnt += reinterpret_cast<const unsigned long long*>(partial)[2 * i + 1];
    }
    block_sum_count(s, cnt, result);  // single block: lands in result[0], result[1]
}

template <typename T>
static void mask_split_t(const T* x, size_t n, double below, uint8_t* bits, double* partial, double* result, hipStream_t st)
{
    const int g = mask_grid(n);
    if (((uintptr_t)bits & 7) == 0) hipLaunchKernelGGL((k_mask_split<T, true>), dim3(g), dim3(WR_MASK_THREADS), 0, st, x, n, below, bits, partial);
    else hipLaunchKernelGGL((k_mask_split<T, false>), dim3(g), dim3(WR_MASK_THREADS), 0, st, x, n, below, bits, partial);
    hipLaunchKernelGGL(k_mask_split_final, dim3(1), dim3(WR_MASK_THREADS), 0, st, partial, g, result);
}
void mask_split(const double* x, size_t n, double below, uint8_t* bits, double* partial, double* result, hipStream_t st) { mask_split_t(x, n, below, bits, partial, result, st); }
void mask_split(const float* x, size_t n, double below, uint8_t* bits, double* partial, double* result, hipStream_t st) { mask_split_t(x, n, below, bits, partial, result, st); }

template <typename T>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_fill(T* __restrict__ x, size_t n, const uint8_t* __restrict__ bits, bool wide, T v)
{
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    for (size_t ch = wave; ch < nchunk; ch += nwaves) {
        const unsigned long long m = mask_word(bits, nbytes, ch, wide);
        if (!m) continue;  // (the whole wave: m is the same in every lane)
        const size_t i = (ch << 6) + lane;
        if (i < n && ((m >> lane) & 1)) x[i] = v;
    }
}

template <typename T>
static void mask_fill_t(T* x, size_t n, const uint8_t* bits, T v, hipStream_t st)
{
    hipLaunchKernelGGL((k_mask_fill<T>), dim3(mask_grid(n)), dim3(WR_MASK_THREADS), 0, st, x, n, bits, ((uintptr_t)bits & 7) == 0, v);
}
void mask_fill(double* x, size_t n, const uint8_t* bits, double v, hipStream_t st) { mask_fill_t(x, n, bits, v, st); }
void mask_fill(float* x, size_t n, const uint8_t* bits, float v, hipStream_t st) { mask_fill_t(x, n, bits, v, st); }

template <typename T>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_restore(T* __restrict__ x, size_t n, const uint8_t* __restrict__ bits, bool wide, T v,
                                                                    unsigned long long* __restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    unsigned long long pop = 0, beyond = 0;  // (of the wave: every lane holds the same values)
    for (size_t ch = wave; ch < nchunk; ch += nwaves) {
        const unsigned long long m = mask_word(bits, nbytes, ch, wide);
        if (!m) continue;
        const size_t left = n - (ch << 6);
        const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1;
        pop += (unsigned long long)__popcll(m);
        beyond |= m & ~valid;
        const size_t i = (ch << 6) + lane;
        if (x && i < n && ((m >> lane) & 1)) x[i] = v;
    }
    if (lane == 0) {
        if (pop) atomicAdd(&counters[0], pop);
        if (beyond) atomicOr(&counters[1], 1ull);
    }
}

template <typename T>
static void mask_restore_t(T* x, size_t n, const uint8_t* bits, T v, unsigned long long* counters, hipStream_t st)
{
    (void)hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), st);
    hipLaunchKernelGGL((k_mask_restore<T>), dim3(mask_grid(n)), dim3(WR_MASK_THREADS), 0, st, x, n, bits, ((uintptr_t)bits & 7) == 0, v, counters);
}
void mask_restore(double* x, size_t n, const uint8_t* bits, double v, unsigned long long* counters, hipStream_t st) { mask_restore_t(x, n, bits, v, counters, st); }
void mask_restore(float* x, size_t n, const uint8_t* bits, float v, unsigned long long* counters, hipStream_t st) { mask_restore_t(x, n, bits, v, counters, st); }

// ---- the restore on a region of a level's box (wrmask::Region).  A wave takes 64 consecutive x of one region row per turn;
// the turns of a row, then the rows, go round the grid's waves: wave w takes turn t = w, w + W, ...  (turn, y, z) are kept as
// counters that advance by W's digits with carries, so the walk has no division after its first step.
struct MaskBox {
    unsigned long long nx, ny;  // the field's
    uint32_t r;
    uint32_t x0, y0, z0;
    uint32_t cx, cy, cz;  // the region's extents
};

// The word of a turn at level 0: bits J0 .. J0 + cnt - 1 (cnt in 1 .. 64) as bits 0 .. cnt - 1, from the 1 .. 9 bytes that hold
// them and no others (bits above cnt - 1: whatever those bytes hold).  Every lane of the wave passes the same J0 and cnt.
__device__ inline unsigned long long mask_word_at(const uint8_t* __restrict__ bits, size_t J0, uint32_t cnt)
{
    const size_t b0 = J0 >> 3;
    const uint32_t sh = (uint32_t)(J0 & 7), nb = (uint32_t)(((J0 + cnt - 1) >> 3) - b0) + 1;
    unsigned long long lo = 0;
    if (nb >= 8 && (reinterpret_cast<uintptr_t>(bits + b0) & 7) == 0) lo = *reinterpret_cast<const unsigned long long*>(bits + b0);
    else
        for (uint32_t k = 0; k < 8; k++)
            if (k < nb) lo |= (unsigned long long)bits[b0 + k] << (8 * k);
    unsigned long long m = lo >> sh;
    if (nb == 9) m |= (unsigned long long)bits[b0 + 8] << (64 - sh);  // (nine bytes: sh != 0)
    return m;
}

// One turn of a box restore, written once for k_mask_restore_box and k_mask_restore_boxes: the 64 consecutive x from xs of row
// (y, z) of a region at (x0, y0, z0) with the extents (cx, cy, .), in the level-r box of a field of nx * ny * . samples.  o: the
// region's elements; `v` goes where a bit is set, and the set bits among the turn's are added to pop.  Everything but `lane` is
// the same in every lane of the wave.
template <typename T>
__device__ __forceinline__ void mask_box_turn(T* o, const uint8_t* bits, unsigned long long nx, unsigned long long ny, uint32_t r,
                                              uint32_t x0, uint32_t y0, uint32_t z0, uint32_t cx, uint32_t cy, uint32_t xs, uint32_t y, uint32_t z, uint32_t lane, T v,
                                              unsigned long long& pop)
{
    const uint32_t left = cx - xs, cnt = left < 64 ? left : 64;
    const unsigned long long valid = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
    const size_t row = (size_t)nx * (((size_t)(y0 + y) << r) + (size_t)ny * ((size_t)(z0 + z) << r));
    unsigned long long m;
    if (r == 0) {
        m = mask_word_at(bits, row + x0 + xs, cnt) & valid;
    } else {
        const size_t J = row + ((size_t)(x0 + xs + lane) << r);
        m = __ballot(lane < cnt && ((bits[J >> 3] >> (J & 7)) & 1));
    }
    if (m) {  // (the whole wave: m is the same in every lane)
        pop += (unsigned long long)__popcll(m);
        if ((m >> lane) & 1) o[((size_t)z * cy + y) * cx + xs + lane] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_restore_box(T* __restrict__ out, MaskBox g, const uint8_t* __restrict__ bits, T v,
                                                                        unsigned long long* __restrict__ counters)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6)));
    const uint32_t nwaves = gridDim.x * WR_MASK_WAVES;
    const uint32_t tpr = (g.cx + 63) >> 6;  // turns per row
    // the step W = nwaves as digits (dt, dy, dz) in the bases (tpr, cy, .), and where the wave starts
    const uint32_t dt = nwaves % tpr, drow = nwaves / tpr, dy = drow % g.cy, dz = drow / g.cy;
    uint32_t turn = wave % tpr, y = (wave / tpr) % g.cy, z = (wave / tpr) / g.cy;
    unsigned long long pop = 0;  // (of the wave: every lane holds the same value)
    while (z < g.cz) {
        mask_box_turn(out, bits, g.nx, g.ny, g.r, g.x0, g.y0, g.z0, g.cx, g.cy, turn << 6, y, z, lane, v, pop);
        turn += dt;
        const uint32_t carry = turn >= tpr;
        if (carry) turn -= tpr;
        y += dy + carry;
        if (y >= g.cy) { y -= g.cy; z++; }
        z += dz;
    }
    if (lane == 0 && pop) atomicAdd(&counters[0], pop);
}

template <typename T>
static void mask_restore_box_t(T* out, const wrmask::Region& g, const uint8_t* bits, T v, unsigned long long* counters, hipStream_t st)
{
    MaskBox b;
    b.nx = (unsigned long long)g.nx; b.ny = (unsigned long long)g.ny;
    b.r = (uint32_t)g.r;
    b.x0 = (uint32_t)g.x0; b.y0 = (uint32_t)g.y0; b.z0 = (uint32_t)g.z0;
    b.cx = (uint32_t)(g.x1 - g.x0); b.cy = (uint32_t)(g.y1 - g.y0); b.cz = (uint32_t)(g.z1 - g.z0);
    const size_t turns = (size_t)((b.cx + 63) >> 6) * b.cy * b.cz;
    size_t grid = (turns + WR_MASK_WAVES - 1) / WR_MASK_WAVES;
    if (grid > WR_MASK_BLOCKS) grid = WR_MASK_BLOCKS;
    (void)hipMemsetAsync(counters, 0, sizeof(unsigned long long), st);
    hipLaunchKernelGGL((k_mask_restore_box<T>), dim3((unsigned)grid), dim3(WR_MASK_THREADS), 0, st, out, b, bits, v, counters);
}
void mask_restore_box(double* out, const wrmask::Region& g, const uint8_t* bits, double v, unsigned long long* counters, hipStream_t st) { mask_restore_box_t(out, g, bits, v, counters, st); }
void mask_restore_box(float* out, const wrmask::Region& g, const uint8_t* bits, float v, unsigned long long* counters, hipStream_t st) { mask_restore_box_t(out, g, bits, v, counters, st); }

// ---- the restore on the boxes of a region decode across a batch of fields: every (field that has a mask, region) in ONE
// launch.  An item is such a pair, in the order of the fields, then the regions.  The regions are the same for every field, so
// the item table is kept in two parts: a record per region (its box, its turns per row, its element offset offs[i]) with
// first[0 .. nroi], the exclusive prefix of the regions' turns (wrmask::boxes_turns), and a record per field with a mask (its
// plane, its element offset f * T, its counter).  Item (m, i) -- m counts the fields that have a mask -- owns the turns
// m * tpf + first[i] .. m * tpf + first[i + 1] - 1 of the launch, tpf = first[nroi]; a turn is 64 consecutive x of one region
// row, exactly k_mask_restore_box's.  The launch's turns go round the grid's waves: wave w takes t = w, w + W, ...
// The walk.  (m, u) = (t / tpf, t % tpf) are kept as counters that advance by W's digits with a carry, so the field costs no
// division after the first step.  The region of u is found by bisection in first[] and kept with its range [lo, hi): a wave
// searches again only when u has left the range (a step into the same region of the next field keeps it).  Inside the region
// the turn's (turn, y, z) come from u - lo by two divisions, one where the rows have a single turn (cx <= 64: every probe):
// the digits of W in a region's bases, which is how k_mask_restore_box avoids dividing, would have to be formed anew, by the
// same divisions, each time the region changes.  Everything but the lane's own bit is uniform in the wave (the wave index is
// made so) and lives in scalar registers.
// The count: a wave adds up the set bits of its turns of one item and puts them into the field's counter with one integer
// atomic when it leaves the item.  Nothing depends on where a block ends: a wave only knows its own index in the grid.
struct MaskBoxRegion {
    uint32_t x0, y0, z0;
    uint32_t cx, cy, cz;  // the region's extents
    uint32_t tpr, pad;    // turns per row
    unsigned long long off;  // where the region starts in a field's part of the output, elements
};
struct MaskBoxField {
    const uint8_t* bits;
    unsigned long long off;  // where the field's part starts in the output, elements
};
struct MaskBoxes {
    unsigned long long nx, ny;  // the fields'
    uint32_t r, nroi, tpf, nfld;
    const MaskBoxRegion* reg;
    const uint32_t* first;
    const MaskBoxField* fld;
    unsigned long long* counters;  // one per field with a mask
};

template <typename T>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_restore_boxes(T* __restrict__ out, MaskBoxes g, T v)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6)));
    const uint32_t nwaves = gridDim.x * WR_MASK_WAVES;
    const uint32_t du = nwaves % g.tpf, dm = nwaves / g.tpf;
    uint32_t u = wave % g.tpf, m = wave / g.tpf;
    uint32_t lo = 0, hi = 0, item_m = 0;  // the item at hand: field item_m, the region whose turns are [lo, hi); hi == 0: none yet
    MaskBoxRegion b = {};
    const uint8_t* bits = nullptr;
    T* o = nullptr;
    unsigned long long pop = 0;  // (of the wave and the item: every lane holds the same value)
    while (m < g.nfld) {
        if (u < lo || u >= hi || m != item_m) {
            if (lane == 0 && pop) atomicAdd(&g.counters[item_m], pop);
            pop = 0;
            if (u < lo || u >= hi) {
                uint32_t i = 0, end = g.nroi;  // first[i] <= u < first[end]
                while (end - i > 1) {
                    const uint32_t mid = (i + end) >> 1;
                    if (g.first[mid] <= u) i = mid;
                    else end = mid;
                }
                b = g.reg[i];
                lo = g.first[i];
                hi = g.first[i + 1];
            }
            item_m = m;
            bits = g.fld[m].bits;
            o = out + g.fld[m].off + b.off;
        }
        const uint32_t q = u - lo;
        uint32_t turn = 0, rowi = q;
        if (b.tpr != 1) { rowi = q / b.tpr; turn = q - rowi * b.tpr; }
        const uint32_t z = rowi / b.cy, y = rowi - z * b.cy;
        mask_box_turn(o, bits, g.nx, g.ny, g.r, b.x0, b.y0, b.z0, b.cx, b.cy, turn << 6, y, z, lane, v, pop);
        u += du;
        const uint32_t carry = u >= g.tpf;
        if (carry) u -= g.tpf;
        m += dm + carry;
    }
    if (lane == 0 && pop) atomicAdd(&g.counters[item_m], pop);
}

namespace {
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
size_t boxes_first_at(size_t nroi) { return nroi * sizeof(MaskBoxRegion); }
size_t boxes_fields_at(size_t nroi) { return boxes_first_at(nroi) + up8((nroi + 1) * sizeof(uint32_t)); }
size_t boxes_counters_at(size_t nroi, size_t nfields) { return boxes_fields_at(nroi) + nfields * sizeof(MaskBoxField); }
}  // namespace

size_t mask_boxes_table_bytes(size_t nroi, size_t nfields) { return (boxes_counters_at(nroi, nfields) + nfields * sizeof(unsigned long long) + 255) & ~(size_t)255; }
unsigned long long* mask_boxes_counters(uint8_t* table, size_t nroi, size_t nfields) { return reinterpret_cast<unsigned long long*>(table + boxes_counters_at(nroi, nfields)); }

template <typename T>
static int mask_restore_boxes_t(T* out, const wrmask::Region* gs, const size_t* offs, size_t nroi, const uint8_t* const* bits, size_t nfields, size_t field_elems,
                                T v, uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    MaskBoxRegion* const reg = reinterpret_cast<MaskBoxRegion*>(host_table);
    uint32_t* const first = reinterpret_cast<uint32_t*>(host_table + boxes_first_at(nroi));
    MaskBoxField* const fld = reinterpret_cast<MaskBoxField*>(host_table + boxes_fields_at(nroi));
    const size_t tpf = wrmask::boxes_turns(gs, nroi, first);
    if (!tpf) return -1;
    for (size_t i = 0; i < nroi; i++) {
        MaskBoxRegion& b = reg[i];
        memset(&b, 0, sizeof b);
        b.x0 = (uint32_t)gs[i].x0; b.y0 = (uint32_t)gs[i].y0; b.z0 = (uint32_t)gs[i].z0;
        b.cx = (uint32_t)(gs[i].x1 - gs[i].x0); b.cy = (uint32_t)(gs[i].y1 - gs[i].y0); b.cz = (uint32_t)(gs[i].z1 - gs[i].z0);
        b.tpr = (b.cx + 63) >> 6;
        b.off = offs[i];
    }
    size_t nfld = 0;
    for (size_t f = 0; f < nfields; f++)
        if (bits[f]) { fld[nfld].bits = bits[f]; fld[nfld].off = (unsigned long long)f * field_elems; nfld++; }
    if (!nfld) return 0;
    const unsigned long long turns = (unsigned long long)nfld * tpf;
    if (turns >= wrmask::kTurnLimit) return -1;
    MaskBoxes g;
    g.nx = (unsigned long long)gs[0].nx; g.ny = (unsigned long long)gs[0].ny;
    g.r = (uint32_t)gs[0].r; g.nroi = (uint32_t)nroi; g.tpf = (uint32_t)tpf; g.nfld = (uint32_t)nfld;
    g.reg = reinterpret_cast<const MaskBoxRegion*>(table);
    g.first = reinterpret_cast<const uint32_t*>(table + boxes_first_at(nroi));
    g.fld = reinterpret_cast<const MaskBoxField*>(table + boxes_fields_at(nroi));
    g.counters = mask_boxes_counters(table, nroi, nfields);
    size_t grid = (size_t)((turns + WR_MASK_WAVES - 1) / WR_MASK_WAVES);
    if (grid > WR_MASK_BLOCKS) grid = WR_MASK_BLOCKS;
    (void)hipMemcpyAsync(table, host_table, boxes_counters_at(nroi, nfields), hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(g.counters, 0, nfld * sizeof(unsigned long long), st);
    hipLaunchKernelGGL((k_mask_restore_boxes<T>), dim3((unsigned)grid), dim3(WR_MASK_THREADS), 0, st, out, g, v);
    return (int)nfld;
}
int mask_restore_boxes(double* out, const wrmask::Region* gs, const size_t* offs, size_t nroi, const uint8_t* const* bits, size_t nfields, size_t field_elems, double v,
                       uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    return mask_restore_boxes_t(out, gs, offs, nroi, bits, nfields, field_elems, v, host_table, table, st);
}
int mask_restore_boxes(float* out, const wrmask::Region* gs, const size_t* offs, size_t nroi, const uint8_t* const* bits, size_t nfields, size_t field_elems, float v,
                       uint8_t* host_table, uint8_t* table, hipStream_t st)
{
    return mask_restore_boxes_t(out, gs, offs, nroi, bits, nfields, field_elems, v, host_table, table, st);
}

// x[0, n) = v: the constant fp32 field of a host caller of the masked batch call, made where the restore will find it
__global__ __launch_bounds__(WR_MASK_THREADS) void k_fill_f32(float* __restrict__ x, size_t n, float v)
{
    for (size_t i = (size_t)blockIdx.x * WR_MASK_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * WR_MASK_THREADS) x[i] = v;
}
void fill_f32(float* x, size_t n, float v, hipStream_t st)
{
    size_t g = (n + WR_MASK_THREADS - 1) / WR_MASK_THREADS;
    if (g < 1) g = 1;
    if (g > WR_MASK_BLOCKS) g = WR_MASK_BLOCKS;
    hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)g), dim3(WR_MASK_THREADS), 0, st, x, n, v);
}

// ---- the masked compare of an encode to an error bound or a quality target on a masked field (include/waverange_amd.h,
// "Masked fields in the tolerance searches"): what k_err_stats gives (wr_kernels.hip) over the samples whose mask bit is clear
// -- the maximum of the finite |a - b|, the count of differences that are not finite, S_D = the fp64 sum of q = fl(d * d) over
// the finite d = fl(a - b), operands widened to fp64 first -- and the number of samples compared, the clear bits below n, as
// an integer.  Nothing at a position whose bit is set is looked at: such a sample is loaded only as the other half of a pair
// that has a defined sample, and a select puts 0 in its place.
// The walk.  PAIRS (both arrays aligned for two-sample loads, 16 bytes fp64, 8 bytes fp32): a wave takes 128 consecutive
// samples per turn, lane l the pair 128 t + 2 l, 128 t + 2 l + 1 in one load per array, and the turn's 16 mask bytes as two
// words every lane holds (the wave index is made uniform, so the words are read once per wave, not once per sample); turns go
// round the grid's waves, wave w takes t = w, w + W, ...  A turn whose 128 bits are all set costs those 16 bytes only.  The
// element-wise form (any alignment): a turn is 64 samples and one word, lane l sample 64 t + l.  The mask words are read as
// 8-byte words where `bits` is 8-byte aligned and all 8 bytes lie below ceil(n / 8), byte by byte otherwise (mask_word); no byte
// at or beyond ceil(n / 8) and no sample at or beyond n is read: the bits at and beyond n count as set (cmp_word).
// The order of the sum is fixed by n, by which of the two forms runs and by the mask, never by the order in which blocks or
// waves finish: a thread adds its terms in index order (the two-sample form keeps one sum per sample of the pair and adds the
// second to the first, then the odd last sample, which the grid's first thread takes), the lanes of a wave combine by shuffles
// at distances 32 .. 1, thread 0 adds the waves' sums in wave order, the final block's thread t adds the partials t, t + 256,
// .. in that order and reduces the same way.  No atomics.
// Accuracy.  Every term is >= 0, so a sum that passes through k roundings lies within k u / (1 - k u) of the real sum of the
// same q, u = 2^-53.  The grid is at most WR_MASK_BLOCKS x WR_MASK_THREADS = 2^19 threads and covers ceil(n / 512) blocks'
// worth of samples before it wraps: a thread of the element-wise form adds at most ceil(n / 2^19) terms (2^14 at n = 2^33), a
// sum of the two-sample form ceil(n / 2^20) and one addition joins the two, one more takes the odd sample; then 6 shuffle
// steps, 3 waves, and in the final block at most 8 partials, 6 steps, 3 waves: k <= 2^14 + 27, |S_D - S_D*| < 2^-38 S_D* for
// every n <= 2^33.  A mask only removes terms.
// partial[4b .. 4b + 3] = block b's maximum, count, sum and (as an unsigned 64-bit integer) compared samples.
template <typename T> struct CmpPair;
template <> struct CmpPair<double> { using type = double2; };
template <> struct CmpPair<float> { using type = float2; };

__device__ inline void cmp_acc(double a, double b, double& mx, double& cnt, double& s)  // (err_stats_acc, wr_kernels.hip)
{
    const double d = a - b, m = fabs(d);
    if (m <= DBL_MAX) { mx = fmax(mx, m); s = s + d * d; }
    else cnt += 1.0;
}

// mask_word of chunk ch with the bits of the samples at and beyond n set
__device__ inline unsigned long long cmp_word(const uint8_t* __restrict__ bits, size_t nbytes, size_t n, size_t ch, bool wide)
{
    const size_t base = ch << 6;
    if (base >= n) return ~0ull;
    unsigned long long m = mask_word(bits, nbytes, ch, wide);
    if (n - base < 64) m |= ~0ull << (n - base);
    return m;
}

// def: the caller's share of the compared samples (summed over the block's threads)
__device__ inline void block_cmp_reduce(double mx, double cnt, double s, unsigned long long def, double* __restrict__ out,
                                        unsigned long long* __restrict__ out_def)
{
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_down(mx, o, 64));
        cnt += __shfl_down(cnt, o, 64);
        s = s + __shfl_down(s, o, 64);
        def += __shfl_down(def, o, 64);
    }
    __shared__ double smx[WR_MASK_WAVES], scn[WR_MASK_WAVES], ssq[WR_MASK_WAVES];
    __shared__ unsigned long long sdf[WR_MASK_WAVES];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smx[w] = mx; scn[w] = cnt; ssq[w] = s; sdf[w] = def; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WR_MASK_WAVES; i++) { mx = fmax(mx, smx[i]); cnt += scn[i]; s = s + ssq[i]; def += sdf[i]; }
        out[0] = mx;
        out[1] = cnt;
        out[2] = s;
        *out_def = def;
    }
}

// wide: `bits` is 8-byte aligned
template <typename T, bool PAIRS>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_err_stats_masked(const T* __restrict__ a, const T* __restrict__ b, size_t n,
                                                                        const uint8_t* __restrict__ bits, bool wide, double* __restrict__ partial)
{
    double mx = 0.0, cnt = 0.0, s = 0.0;
    unsigned long long def = 0;  // (of the wave: every lane holds the same value)
    const uint32_t lane = threadIdx.x & 63;
    const size_t wave = (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6)));
    const size_t nwaves = (size_t)gridDim.x * WR_MASK_WAVES, nbytes = (n + 7) >> 3;
    if (PAIRS) {
        double s1 = 0.0;
        const size_t n2 = n >> 1, nturn = (n + 127) >> 7;
        const typename CmpPair<T>::type* a2 = reinterpret_cast<const typename CmpPair<T>::type*>(a);
        const typename CmpPair<T>::type* b2 = reinterpret_cast<const typename CmpPair<T>::type*>(b);
        for (size_t t = wave; t < nturn; t += nwaves) {
            const unsigned long long m0 = cmp_word(bits, nbytes, n, 2 * t, wide), m1 = cmp_word(bits, nbytes, n, 2 * t + 1, wide);
            def += (unsigned long long)(__popcll(~m0) + __popcll(~m1));
            if ((m0 & m1) == ~0ull) continue;  // (the whole wave: the words are the same in every lane)
            const size_t i = (t << 6) + lane;  // the lane's pair
            const uint32_t und = (uint32_t)((lane < 32 ? m0 >> (2 * lane) : m1 >> (2 * (lane - 32))) & 3);
            if (i < n2 && und != 3) {
                // one load per array for the pair.  The undefined sample of a half-defined pair goes in as 0 - 0: the maximum and
                // the count do not move and s + 0 is s, bit for bit, so the sum is the one of the defined samples in index
                // order.  (Selects, not branches: with a branch per sample the compiler sinks the loads into the branches
                // and splits each 16-byte load into two of 8.)
                const typename CmpPair<T>::type va = a2[i], vb = b2[i];
                const bool ux = und & 1, uy = und & 2;
                cmp_acc(ux ? 0.0 : (double)va.x, ux ? 0.0 : (double)vb.x, mx, cnt, s);
                cmp_acc(uy ? 0.0 : (double)va.y, uy ? 0.0 : (double)vb.y, mx, cnt, s1);
            }
        }
        s = s + s1;
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0 && !((bits[(n - 1) >> 3] >> ((n - 1) & 7)) & 1))
            cmp_acc((double)a[n - 1], (double)b[n - 1], mx, cnt, s);
    } else {
        const size_t nchunk = (n + 63) >> 6;
        for (size_t ch = wave; ch < nchunk; ch += nwaves) {
            const unsigned long long m = cmp_word(bits, nbytes, n, ch, wide);
            def += (unsigned long long)__popcll(~m);
            if (m == ~0ull) continue;  // (the whole wave)
            const size_t i = (ch << 6) + lane;
            if (!((m >> lane) & 1)) cmp_acc((double)a[i], (double)b[i], mx, cnt, s);  // (a clear bit: i < n)
        }
    }
    block_cmp_reduce(mx, cnt, s, lane == 0 ? def : 0ull, partial + 4 * blockIdx.x,
                     reinterpret_cast<unsigned long long*>(partial) + 4 * blockIdx.x + 3);
}

__global__ __launch_bounds__(WR_MASK_THREADS) void k_err_stats_masked_final(const double* __restrict__ partial, int np, double* __restrict__ result,
                                                                              unsigned long long* __restrict__ defined)
{
    double mx = 0.0, cnt = 0.0, s = 0.0;
    unsigned long long def = 0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        mx = fmax(mx, partial[4 * i]);
        cnt += partial[4 * i + 1];
        s = s + partial[4 * i + 2];
        def += reinterpret_cast<const unsigned long long*>(partial)[4 * i + 3];
    }
    block_cmp_reduce(mx, cnt, s, def, result, defined);  // single block: lands in result[0 .. 2] and *defined
}

template <typename T>
static void err_stats_masked_t(const T* a, const T* b, size_t n, const uint8_t* bits, double* partial, double* result, unsigned long long* defined,
                               hipStream_t st)
{
    const bool pairs = (((uintptr_t)a | (uintptr_t)b) & (2 * sizeof(T) - 1)) == 0, wide = ((uintptr_t)bits & 7) == 0;
    size_t g = (n + 2 * WR_MASK_THREADS - 1) / (2 * WR_MASK_THREADS);  // (the grid of k_err_stats)
    if (g < 1) g = 1;
    if (g > WR_MASK_BLOCKS) g = WR_MASK_BLOCKS;
    if (pairs) hipLaunchKernelGGL((k_err_stats_masked<T, true>), dim3((unsigned)g), dim3(WR_MASK_THREADS), 0, st, a, b, n, bits, wide, partial);
    else hipLaunchKernelGGL((k_err_stats_masked<T, false>), dim3((unsigned)g), dim3(WR_MASK_THREADS), 0, st, a, b, n, bits, wide, partial);
    hipLaunchKernelGGL(k_err_stats_masked_final, dim3(1), dim3(WR_MASK_THREADS), 0, st, partial, (int)g, result, defined);
}
void err_stats_masked(const double* a, const double* b, size_t n, const uint8_t* bits, double* partial, double* result, unsigned long long* defined,
                      hipStream_t st)
{
    err_stats_masked_t(a, b, n, bits, partial, result, defined, st);
}
void err_stats_masked(const float* a, const float* b, size_t n, const uint8_t* bits, double* partial, double* result, unsigned long long* defined,
                      hipStream_t st)
{
    err_stats_masked_t(a, b, n, bits, partial, result, defined, st);
}

// ---- split, fill and check across a batch of fields of n samples each, one launch per stage.  The grid is two-dimensional:
// gridDim.x = mask_grid(n), gridDim.y = the fields; block (x, y) finds field y's pointers in a table in device-visible memory
// (pinned host memory: 1024 entries do not fit in kernel arguments) and then does for that field exactly what block x of the
// single kernel does for it alone -- the same chunks per wave, the same kTurns, the same order of additions, block_sum_count's
// shuffles and wave order -- so that S and the count of every field have the bits the single kernel gives.  The single
// kernels above are not touched: these are bodies of their own.
// k_mask_split_batch: partial[y * 2 * gridDim.x + 2x .. + 1] = the sum and count of block (x, y); k_mask_split_final_batch's
// block y reduces field y's gridDim.x partials in k_mask_split_final's order into result[2y], result[2y + 1].
// WIDE: every field's `bits` is 8-byte aligned
template <typename T, bool WIDE>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_split_batch(const MaskSplitItem* __restrict__ items, size_t n, double below,
                                                                        double* __restrict__ partial)
{
    const MaskSplitItem it = items[blockIdx.y];
    const T* __restrict__ x = static_cast<const T*>(it.x);
    uint8_t* __restrict__ bits = it.bits;
    double s = 0.0;
    unsigned long long cnt = 0;
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    constexpr int kTurns = 4;  // (k_mask_split's)
    for (size_t ch0 = wave; ch0 < nchunk; ch0 += kTurns * nwaves) {
        T v[kTurns];
        bool have[kTurns];
#pragma unroll
        for (int u = 0; u < kTurns; u++) {
            const size_t ch = ch0 + u * nwaves, i = (ch << 6) + lane;
            have[u] = ch < nchunk && i < n;
            v[u] = have[u] ? x[i] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < kTurns; u++) {
            const size_t ch = ch0 + u * nwaves;
            if (ch >= nchunk) break;  // (the whole wave)
            const double w = (double)v[u];
            const bool undef = have[u] && (!(fabs(w) <= DBL_MAX) || w < below);
            if (have[u] && !undef) { s = s + w; cnt++; }
            const unsigned long long m = __ballot(undef);
            if (lane == 0) {
                const size_t b0 = ch << 3;
                if (WIDE && b0 + 8 <= nbytes) *reinterpret_cast<unsigned long long*>(bits + b0) = m;
                else
                    for (int k = 0; k < 8; k++)
                        if (b0 + k < nbytes) bits[b0 + k] = (uint8_t)(m >> (8 * k));
            }
        }
    }
    block_sum_count(s, cnt, partial + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_split_final_batch(const double* __restrict__ partial, int np, double* __restrict__ result)
{
    const double* __restrict__ p = partial + 2 * (size_t)blockIdx.x * np;
    double s = 0.0;
    unsigned long long cnt = 0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        s = s + p[2 * i];
        cnt += reinterpret_cast<const unsigned long long*>(p)[2 * i + 1];
    }
    block_sum_count(s, cnt, result + 2 * blockIdx.x);
}

size_t mask_split_batch_partials(size_t n) { return 2 * (size_t)mask_grid(n); }

void mask_split_batch(const MaskSplitItem* host_items, const MaskSplitItem* d_items, int nfields, bool f32, size_t n, double below, double* partial, double* result,
                      hipStream_t st)
{
    const int g = mask_grid(n);
    bool wide = true;
    for (int f = 0; f < nfields; f++) wide = wide && ((uintptr_t)host_items[f].bits & 7) == 0;
    const dim3 grid((unsigned)g, (unsigned)nfields), block(WR_MASK_THREADS);
    if (f32) {
        if (wide) hipLaunchKernelGGL((k_mask_split_batch<float, true>), grid, block, 0, st, d_items, n, below, partial);
        else hipLaunchKernelGGL((k_mask_split_batch<float, false>), grid, block, 0, st, d_items, n, below, partial);
    } else {
        if (wide) hipLaunchKernelGGL((k_mask_split_batch<double, true>), grid, block, 0, st, d_items, n, below, partial);
        else hipLaunchKernelGGL((k_mask_split_batch<double, false>), grid, block, 0, st, d_items, n, below, partial);
    }
    hipLaunchKernelGGL(k_mask_split_final_batch, dim3((unsigned)nfields), block, 0, st, partial, g, result);
}

// k_mask_fill_batch: k_mask_fill on field blockIdx.y of the table; the value travels as the bits of a T
template <typename T> __device__ inline T mask_value_of(unsigned long long v);
template <> __device__ inline double mask_value_of<double>(unsigned long long v) { return __longlong_as_double((long long)v); }
template <> __device__ inline float mask_value_of<float>(unsigned long long v) { return __uint_as_float((unsigned)v); }

template <typename T>
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_fill_batch(const MaskFillItem* __restrict__ items, size_t n)
{
    const MaskFillItem it = items[blockIdx.y];
    T* __restrict__ x = static_cast<T*>(it.x);
    const uint8_t* __restrict__ bits = it.bits;
    const bool wide = (reinterpret_cast<uintptr_t>(bits) & 7) == 0;
    const T v = mask_value_of<T>(it.value);
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    for (size_t ch = wave; ch < nchunk; ch += nwaves) {
        const unsigned long long m = mask_word(bits, nbytes, ch, wide);
        if (!m) continue;  // (the whole wave: m is the same in every lane)
        const size_t i = (ch << 6) + lane;
        if (i < n && ((m >> lane) & 1)) x[i] = v;
    }
}

unsigned long long mask_fill_value(double v, bool f32)
{
    unsigned long long out = 0;
    if (f32) { const float w = (float)v; memcpy(&out, &w, sizeof w); }
    else memcpy(&out, &v, sizeof v);
    return out;
}

void mask_fill_batch(const MaskFillItem* d_items, int nitems, bool f32, size_t n, hipStream_t st)
{
    const dim3 grid((unsigned)mask_grid(n), (unsigned)nitems), block(WR_MASK_THREADS);
    if (f32) hipLaunchKernelGGL((k_mask_fill_batch<float>), grid, block, 0, st, d_items, n);
    else hipLaunchKernelGGL((k_mask_fill_batch<double>), grid, block, 0, st, d_items, n);
}

// k_mask_check_batch: the count-only k_mask_restore on mask blockIdx.y: counters[2y] += its set bits, counters[2y + 1] |= 1 if
// one lies at or beyond n; one integer atomic per wave and mask.  No field is read.
__global__ __launch_bounds__(WR_MASK_THREADS) void k_mask_check_batch(const uint8_t* const* __restrict__ masks, size_t n, unsigned long long* __restrict__ counters)
{
    const uint8_t* __restrict__ bits = masks[blockIdx.y];
    const bool wide = (reinterpret_cast<uintptr_t>(bits) & 7) == 0;
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * WR_MASK_WAVES + (threadIdx.x >> 6), nwaves = (size_t)gridDim.x * WR_MASK_WAVES;
    const size_t nchunk = (n + 63) >> 6, nbytes = (n + 7) >> 3;
    unsigned long long pop = 0, beyond = 0;  // (of the wave: every lane holds the same values)
    for (size_t ch = wave; ch < nchunk; ch += nwaves) {
        const unsigned long long m = mask_word(bits, nbytes, ch, wide);
        if (!m) continue;
        const size_t left = n - (ch << 6);
        const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1;
        pop += (unsigned long long)__popcll(m);
        beyond |= m & ~valid;
    }
    if (lane == 0) {
        if (pop) atomicAdd(&counters[2 * blockIdx.y], pop);
        if (beyond) atomicOr(&counters[2 * blockIdx.y + 1], 1ull);
    }
}

void mask_check_batch(const uint8_t* const* d_masks, int nmasks, size_t n, unsigned long long* counters, hipStream_t st)
{
    (void)hipMemsetAsync(counters, 0, 2 * (size_t)nmasks * sizeof(unsigned long long), st);
    hipLaunchKernelGGL(k_mask_check_batch, dim3((unsigned)mask_grid(n), (unsigned)nmasks), dim3(WR_MASK_THREADS), 0, st, d_masks, n, counters);
}

}  // namespace wrk
