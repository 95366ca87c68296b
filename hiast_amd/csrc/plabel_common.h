// What the pseudo-label and validator kernels (plabel.hip, plabel2.hip, plabel_tta.hip) are bit-exact about, defined once:
// the per-view arithmetic of the multi-scale + flip average with its argument record and checks, and the counters of the
// per-class fp16-bin confidence histogram [C][HIAST_NBINS] with the scattered workspace they count into.  gfx950 only.
#pragma once
#include "common.h"

namespace hiast {

// ---- views ---------------------------------------------------------------------------------------------------------------
// Per scale s (image resized to Hs x Ws, low-res head map hs x ws) a native pixel reads the <= 4 bilinear taps of the size-s
// probability map; a tap's probabilities are softmax(bilinear(z_s)) at that size-s pixel, plus the same of the mirror image's
// forward read at the mirrored column: "HIAST-A arithmetic" for the logit interpolation and the softmax, so the label map is
// bit-reproducible against the oracle's restatement.
struct ViewScale {
    const float* z;       // [B,C,hs,ws] head output of the resized image
    const float* zf;      // the same of its mirror image, or null
    int hs, ws, Hs, Ws;
    float rh, rw;         // native pixel -> size-s grid
    float sh, sw;         // size-s pixel -> low-res head map
};
struct ViewArgs {
    ViewScale s[HIAST_TTA_MAX_SCALES];
    int n;
};

// The view arrays of the C ABI (hiast_tta_fused, hiast_plabel_pass1_tta) -> a, or the code of the first check that fails
static inline int view_args_fill(ViewArgs& a, const float* const* z, const float* const* zf, const int* hs, const int* ws,
                                 const int* Hs, const int* Ws, int n_scales, int B, int C, int H, int W)
{
    if (!z || !hs || !ws || !Hs || !Ws) return HIAST_E_ARG;
    if (n_scales <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    if (n_scales > HIAST_TTA_MAX_SCALES || B > 65535 || H > 65535) return HIAST_E_RANGE;
    a.n = n_scales;
    for (int i = 0; i < n_scales; ++i) {
        if (!z[i] || (zf && !zf[i]) || hs[i] <= 0 || ws[i] <= 0 || Hs[i] < hs[i] || Ws[i] < ws[i]) return HIAST_E_ARG;
        ViewScale& s = a.s[i];
        s.z = z[i];
        s.zf = zf ? zf[i] : nullptr;
        s.hs = hs[i];
        s.ws = ws[i];
        s.Hs = Hs[i];
        s.Ws = Ws[i];
        // native pixel -> size-s grid (the second F.interpolate, validator.py:52)
        s.rh = H > 1 ? (float)(s.Hs - 1) / (float)(H - 1) : 0.0f;
        s.rw = W > 1 ? (float)(s.Ws - 1) / (float)(W - 1) : 0.0f;
        // size-s grid -> low-res head map (the segmentor's interpolate, self_training_segmentor.py:27)
        s.sh = s.Hs > 1 ? (float)(s.hs - 1) / (float)(s.Hs - 1) : 0.0f;
        s.sw = s.Ws > 1 ? (float)(s.ws - 1) / (float)(s.Ws - 1) : 0.0f;
    }
    return 0;
}

// v[c] = softmax(bilinear(z))[c] at size-s pixel (Y, X)
template <int C>
__device__ __forceinline__ void view_softmax(const float* __restrict__ z, int hs, int ws, float sh, float sw, int Y, int X, float* v)
{
    const Src sy = src_of(sh, Y, hs), sx = src_of(sw, X, ws);
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* p = z + (size_t)c * hs * ws;
        const float top = lerp_h(p[sy.i0 * ws + sx.i0], p[sy.i0 * ws + sx.i1], sx.l0, sx.l1);
        const float bot = lerp_h(p[sy.i1 * ws + sx.i0], p[sy.i1 * ws + sx.i1], sx.l0, sx.l1);
        v[c] = lerp_v(top, bot, sy.l0, sy.l1);
        if (c == 0 || v[c] > m) m = v[c];
    }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = a_expf(v[c] - m);
        s = s + v[c];
    }
    const float inv = 1.0f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = v[c] * inv;
}

// q[c] = p(view)[c] (+ p(mirror view)[c], read at the mirrored column) at size-s pixel (Y, X): p, and the once-rounded p + pf
template <int C>
__device__ __forceinline__ void view_pair(const ViewScale& sc, const float* __restrict__ z, const float* __restrict__ zf, int Y,
                                          int X, float* q)
{
    view_softmax<C>(z, sc.hs, sc.ws, sc.sh, sc.sw, Y, X, q);
    if (zf) {
        float f[C];
        view_softmax<C>(zf, sc.hs, sc.ws, sc.sh, sc.sw, Y, sc.Ws - 1 - X, f);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = q[c] + f[c];
    }
}

// tot[c] += the size-s map resampled at native pixel (Y, X), every tap evaluated by this thread.  The value is built as
// lerp_v(lerp_h(p00, p01), lerp_h(p10, p11)) per class, the oracle's rounding order (the sum of four weighted taps is not
// associative).
template <int C>
__device__ __forceinline__ void view_scale_direct(const ViewScale& sc, const float* __restrict__ z, const float* __restrict__ zf,
                                                  int Y, int X, float* tot)
{
    const Src ty = src_of(sc.rh, Y, sc.Hs), tx = src_of(sc.rw, X, sc.Ws);
    float p00[C], p01[C], p10[C], p11[C];
    view_pair<C>(sc, z, zf, ty.i0, tx.i0, p00);
    // a tap with weight 0 (scale == native size: every pixel) contributes fmaf(0, p, .) = nothing: its softmaxes are skipped and
    // p00 (p10) stands in its place
    const bool dx = tx.i1 != tx.i0 && tx.l1 != 0.0f, dy = ty.i1 != ty.i0 && ty.l1 != 0.0f;
    if (dx) view_pair<C>(sc, z, zf, ty.i0, tx.i1, p01);
    if (dy) view_pair<C>(sc, z, zf, ty.i1, tx.i0, p10);
    if (dx && dy) view_pair<C>(sc, z, zf, ty.i1, tx.i1, p11);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float q01 = dx ? p01[c] : p00[c];
        const float q10 = dy ? p10[c] : p00[c];
        const float q11 = dx ? (dy ? p11[c] : p01[c]) : (dy ? p10[c] : p00[c]);
        const float top = lerp_h(p00[c], q01, tx.l0, tx.l1);
        const float bot = lerp_h(q10, q11, tx.l0, tx.l1);
        tot[c] = tot[c] + lerp_v(top, bot, ty.l0, ty.l1);
    }
}

// ---- histogram counters --------------------------------------------------------------------------------------------------
// A counter is named by its key = class * HIAST_NBINS + fp16 bin, the word of the caller's hist; NOKEY: nothing to count.
constexpr unsigned NOKEY = 0xFFFFFFFFu;

// Scattered layout of the counting workspace.  On real maps a few classes and the confidences 0.5 .. 1 take nearly all pixels:
// in the natural [class][bin] layout their ~2000 counters are ~60 lines of 128 B, and integer atomics on one line execute one
// after the other at the memory side (tools/micro/int_atomics.hip: 3.1 M adds inside 60 lines 0.42 ms, over >= 240 lines
// 0.12 ms = the chip's rate of 26 G atomics/s).  The workspace stores counter (class c, bin) at word
// ((bin & 255) * C + c) * 61 + (bin >> 8): neighbouring bins are 256 planes apart, the hot counters lie on several hundred lines.
constexpr int HIST_PLANE = (HIAST_NBINS + 255) / 256;                 // 61 words per (low byte, class)
template <int C>
__device__ __forceinline__ unsigned hist_slot(unsigned key)
{
    const unsigned c = key / HIAST_NBINS, bin = key - c * HIAST_NBINS;
    return ((bin & 255u) * C + c) * HIST_PLANE + (bin >> 8);
}
// the word of `key` in the scattered workspace (SCATTER) or in hist itself
template <int C, bool SCATTER>
__device__ __forceinline__ unsigned hist_word(unsigned key) { return SCATTER ? hist_slot<C>(key) : key; }

// The workspace protocol (host; plabel.hip): its size (0 for C outside 1 .. HIAST_MAX_CLASSES), zeroing it before a counting
// launch, and the launch that adds it into hist [C][HIAST_NBINS] after one (C: a class count of for_class_count, else
// HIAST_E_RANGE).  All on `st`; -> 0 or an error code.
size_t hist_ws_bytes(int C);
int hist_ws_clear(uint32_t* ws, int C, hipStream_t st);
int hist_ws_merge(const uint32_t* ws, uint32_t* hist, int C, hipStream_t st);

// Wave-aggregated add of one count per lane with a key (all 64 lanes call): lanes holding the same key elect a leader that issues
// ONE atomic of the popcount (flat regions: 64 same-address atomics would serialise).  ROUNDS = 0: until no key is left.
// ROUNDS > 0: that many rounds take out the keys many lanes share, then the lanes that are left add their own count — on
// realistic confidences nearly every lane of a wave holds a different (class, fp16 bin) key, and the fully aggregated loop then
// ran 64 ballot / shuffle rounds per wave row (1.85 ms per 8-image batch; the integer sums are the same in any order).
template <int ROUNDS, int C = 0, bool SCATTER = false>
__device__ __forceinline__ void wave_add(unsigned* cnt, unsigned key)
{
    unsigned long long todo = __ballot(key != NOKEY);
    const auto round = [&] {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        if (lane_id() == leader) atomicAdd(&cnt[hist_word<C, SCATTER>(k)], (unsigned)__popcll(same));
        todo &= ~same;
    };
    if constexpr (ROUNDS == 0) {
        while (todo) round();
    } else {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (!todo) break;
            round();
        }
        if ((todo >> lane_id()) & 1ull) atomicAdd(&cnt[hist_word<C, SCATTER>(key)], 1u);
    }
}

// The TOP fp16 bins (confidence >= 1 - 128 * 2^-11 ~ 0.94) of every class are counted in LDS first (s_top = unsigned [C * TOPB],
// 256 threads) and flushed once per block: on confident predictions most pixels of the whole batch fall into a handful of
// (class, bin) counters (0.99 ms per 8-image batch with every lane adding to global memory).
constexpr int TOPB = 128;
template <int C>
__device__ __forceinline__ void top_zero(unsigned* s_top)
{
    for (int i = threadIdx.x; i < C * TOPB; i += 256) s_top[i] = 0u;
}
// counts (class am, bin) in s_top, or -> its key for the caller to add elsewhere (NOKEY for a bin past the histogram)
__device__ __forceinline__ unsigned top_count(unsigned* s_top, int am, unsigned bin)
{
    if (bin >= HIAST_NBINS - TOPB && bin < HIAST_NBINS) {
        atomicAdd(&s_top[am * TOPB + (int)(bin - (HIAST_NBINS - TOPB))], 1u);
        return NOKEY;
    }
    return bin < HIAST_NBINS ? (unsigned)am * HIAST_NBINS + bin : NOKEY;
}
template <int C, bool SCATTER>
__device__ __forceinline__ void top_flush(const unsigned* s_top, uint32_t* __restrict__ cnt)
{
    for (int i = threadIdx.x; i < C * TOPB; i += 256) {
        const unsigned v = s_top[i];
        const unsigned k = (unsigned)(i / TOPB) * HIAST_NBINS + (HIAST_NBINS - TOPB) + (unsigned)(i % TOPB);
        if (v) atomicAdd(&cnt[hist_word<C, SCATTER>(k)], v);
    }
}

}  // namespace hiast
