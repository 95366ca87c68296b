// What the kernels of the device-side sample path (sample_aug.hip K15, sample_aug2.hip K15b, sample_aug3.hip K15c) agree
// on, defined once: the words of a view's op row, the segment record the host cuts a row into (hiast_hip.h, K15b), the
// 12-byte form of four HWC pixels and the grid of a pass over pixels.  gfx950 only.  The words and kinds of a sample's
// record row are host-safe and live in aug_records.h.
#pragma once
#include "aug_records.h"
#include "common.h"

namespace hiast {

// a view's op row: kind, blob offset of the finished view, n_ops, 0, then (type, parameter) x HIAST_AUG_MAX_OPS
constexpr int OPS = HIAST_AUG_OPS_WORDS;
__device__ __forceinline__ int64_t op_type(const int64_t* o, int i) { return o[4 + 2 * i]; }
__device__ __forceinline__ int64_t op_par(const int64_t* o, int i) { return o[5 + 2 * i]; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one sample's segment of one launch round, every index clamped into the row before it addresses an op: ops [from, to),
// the table op among them (stat | -1), the op that closes the segment (blur | -1: a blur or an FDA); live: a planned
// sample (a finished one has no ops)
enum { S_FROM, S_TO, S_STAT, S_BLUR };
struct Seg {
    int from, to, stat, blur;
    bool live;
};
__device__ __forceinline__ Seg seg_of(const int64_t* o, const int32_t* sg)
{
    Seg s;
    const int n = o[0] != 0 ? 0 : clampi((int)o[2], 0, HIAST_AUG_MAX_OPS);
    s.from = clampi(sg[S_FROM], 0, n);
    s.to = clampi(sg[S_TO], s.from, n);
    s.stat = (sg[S_STAT] >= s.from && sg[S_STAT] < s.to) ? sg[S_STAT] : -1;
    s.blur = (sg[S_BLUR] >= 0 && sg[S_BLUR] < n) ? sg[S_BLUR] : -1;
    s.live = o[0] == 0;
    return s;
}

// four HWC pixels = 12 bytes = three 32-bit words at a 4-byte aligned p: v[j] is byte j, pixel i is v[3 i .. 3 i + 2]
__device__ __forceinline__ void unpack12(const uint32_t* p, unsigned (&v)[12])
{
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = (w0 >> (8 * i)) & 255u;
        v[4 + i] = (w1 >> (8 * i)) & 255u;
        v[8 + i] = (w2 >> (8 * i)) & 255u;
    }
}
__device__ __forceinline__ void pack12(const unsigned (&v)[12], uint32_t* p)
{
    uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w0 |= v[i] << (8 * i);
        w1 |= v[4 + i] << (8 * i);
        w2 |= v[8 + i] << (8 * i);
    }
    p[0] = w0;
    p[1] = w1;
    p[2] = w2;
}

}  // namespace hiast

// blocks of 256 threads along x for a grid-stride pass over HW pixels, four pixels per thread and step
static inline int aug_pixel_blocks(int64_t HW)
{
    const int64_t nb = (HW / 4 + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}
