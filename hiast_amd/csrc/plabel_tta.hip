// K3c — pseudo-label pass 1 over several views (multi-scale + flip): hiast_plabel_pass1_tta.  gfx950 only.
//
// The validator's view averaging (K16, plabel2.hip) with pass 1's outputs (K3, plabel.hip): from the LOW-RES head outputs of
// every (scale, flip) forward to (maxprob, argmax, hist) in one kernel.  Per native pixel
//   tot[c]  = Σ_scales resample_to_native( softmax(up(z_s)) + flip(softmax(up(zf_s))) )[c]      — K16's operations in K16's order
//   argmax  = first c with the largest tot[c]
//   maxprob = fminf(tot[argmax] / n_views, 1)                                                    — IEEE division
//   hist[argmax][fp16 bits of maxprob] += 1
// Neither full-resolution logits nor per-view probability maps are stored; pass 2, the strided sample and the threshold
// recursion read (maxprob, argmax, hist) as they do behind the single-view pass 1.
//
// Two forms of the per-scale sum, same additions on the same operands (same bits):
//   tiled   a block owns PT_TH x PT_TW native pixels.  Per scale it computes q = p(view) + p(mirror view at column Ws-1-x) ONCE
//           for every size-s pixel a tap of the tile reads (the tile's footprint plus one row and one column) into LDS, then
//           every native pixel interpolates its four taps from LDS: about Hs Ws / (H W) softmaxes per pixel and flip where
//           K16 evaluates up to four.
//   direct  K16's thread-per-pixel form (each pixel evaluates its own taps): taken when a scale's footprint does not fit
//           the LDS patch (size ratios above ~1.5 at 19 classes).
// Histogram: as pass 1's one-block-per-item form — the top PT_TOPB fp16 bins of every class in LDS (flushed once per block,
// a block works through many tiles), two wave-aggregated rounds + one atomic per remaining lane for the rest, into the
// scattered workspace (layout of plabel.hip) that a merge launch adds into hist, or straight into hist without one.
#include <stdlib.h>

#include "common.h"

namespace hiast {

constexpr int PT_TH = 8, PT_TW = 32;              // native pixels per tile: 256 threads, one each
constexpr int PT_PATCH = 12288;                   // floats of LDS for a scale's probability patch (48 KiB)
constexpr int PT_TOPB = 128;                      // top fp16 bins (confidence >= ~0.94) counted in LDS
constexpr int PT_PLANE = (HIAST_NBINS + 255) / 256;

// plabel.hip's scattered counter layout: (class c, bin) at word ((bin & 255) * C + c) * 61 + (bin >> 8)
template <int C>
__device__ __forceinline__ unsigned pt_slot(unsigned key)
{
    const unsigned c = key / HIAST_NBINS, bin = key - c * HIAST_NBINS;
    return ((bin & 255u) * C + c) * PT_PLANE + (bin >> 8);
}
template <int C>
__global__ __launch_bounds__(256) void pt_merge_kernel(const uint32_t* __restrict__ ws, uint32_t* __restrict__ hist)
{
    const unsigned key = blockIdx.x * 256u + threadIdx.x;
    if (key >= (unsigned)C * HIAST_NBINS) return;
    const unsigned v = ws[pt_slot<C>(key)];
    if (v) hist[key] += v;                       // (one thread per counter; calls on one stream are ordered)
}

struct PtScale {
    const float* z;       // [B,C,hs,ws] head output of the resized image
    const float* zf;      // the same of its mirror image, or null
    int hs, ws, Hs, Ws;
    float rh, rw;         // native pixel -> size-s grid
    float sh, sw;         // size-s pixel -> low-res head map
};
struct PtArgs {
    PtScale s[HIAST_TTA_MAX_SCALES];
    int n;
};

// v[c] = softmax(bilinear(z))[c] at size-s pixel (Y, X): K16's tap_probs
template <int C>
__device__ __forceinline__ void pt_softmax(const float* __restrict__ z, int hs, int ws, float sh, float sw, int Y, int X, float* v)
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

// q[c] = p(view)[c] (+ p(mirror view)[c] read at the mirrored column) at size-s pixel (Y, X): K16 accumulates fmaf(1, p, 0) and
// then fmaf(1, pf, p), which are p and the once-rounded p + pf
template <int C>
__device__ __forceinline__ void pt_pair(const PtScale& sc, const float* __restrict__ z, const float* __restrict__ zf, int Y, int X,
                                        float* q)
{
    pt_softmax<C>(z, sc.hs, sc.ws, sc.sh, sc.sw, Y, X, q);
    if (zf) {
        float f[C];
        pt_softmax<C>(zf, sc.hs, sc.ws, sc.sh, sc.sw, Y, sc.Ws - 1 - X, f);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = q[c] + f[c];
    }
}

// K16's per-scale value of native pixel (Y, X), every tap evaluated by this thread
template <int C>
__device__ __forceinline__ void pt_scale_direct(const PtScale& sc, const float* __restrict__ z, const float* __restrict__ zf, int Y,
                                                int X, float* tot)
{
    const Src ty = src_of(sc.rh, Y, sc.Hs), tx = src_of(sc.rw, X, sc.Ws);
    float p00[C], p01[C], p10[C], p11[C];
    pt_pair<C>(sc, z, zf, ty.i0, tx.i0, p00);
    // a tap with weight 0 (scale == native size: every pixel) contributes nothing: its softmaxes are skipped, as in K16
    const bool dx = tx.i1 != tx.i0 && tx.l1 != 0.0f, dy = ty.i1 != ty.i0 && ty.l1 != 0.0f;
    if (dx) pt_pair<C>(sc, z, zf, ty.i0, tx.i1, p01);
    if (dy) pt_pair<C>(sc, z, zf, ty.i1, tx.i0, p10);
    if (dx && dy) pt_pair<C>(sc, z, zf, ty.i1, tx.i1, p11);
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

// One block works through the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (x tile fastest, then y tile, then image).
// cnt: the scattered workspace (SCATTER) or the caller's hist.
template <int C, bool TILED, bool SCATTER>
__global__ __launch_bounds__(256) void plabel_tta_kernel(PtArgs a, int H, int W, int ntx, int nty, long long ntiles, float nviews,
                                                         float* __restrict__ maxprob, uint8_t* __restrict__ argmax,
                                                         uint32_t* __restrict__ cnt)
{
    constexpr int CS = C | 1;                     // odd row stride of the patch: lanes on consecutive pixels hit different banks
    __shared__ unsigned s_top[C * PT_TOPB];
    __shared__ float s_patch[TILED ? PT_PATCH : 1];
    const int tid = threadIdx.x;
    for (int i = tid; i < C * PT_TOPB; i += 256) s_top[i] = 0u;
    __syncthreads();

    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {          // block-uniform trip count
        const int xt = (int)(t % ntx);
        const long long r = t / ntx;
        const int yt = (int)(r % nty), b = (int)(r / nty);
        const int X0 = xt * PT_TW, Y0 = yt * PT_TH;
        const int X = X0 + (tid & (PT_TW - 1)), Y = Y0 + (tid / PT_TW);
        const bool live = X < W && Y < H;
        const int Xc = X < W ? X : W - 1, Yc = Y < H ? Y : H - 1;

        float tot[C];
#pragma unroll
        for (int c = 0; c < C; ++c) tot[c] = 0.0f;
        for (int si = 0; si < a.n; ++si) {
            const PtScale sc = a.s[si];
            const float* z = sc.z + (size_t)b * C * sc.hs * sc.ws;
            const float* zf = sc.zf ? sc.zf + (size_t)b * C * sc.hs * sc.ws : nullptr;
            if (TILED) {
                // the size-s pixels the tile's taps read: rows ybase .. ylast, columns xbase .. xlast (src_of is monotonic)
                const int Yl = Y0 + PT_TH - 1 < H ? Y0 + PT_TH - 1 : H - 1, Xl = X0 + PT_TW - 1 < W ? X0 + PT_TW - 1 : W - 1;
                const int ybase = src_of(sc.rh, Y0, sc.Hs).i0, xbase = src_of(sc.rw, X0, sc.Ws).i0;
                const int nr = src_of(sc.rh, Yl, sc.Hs).i1 - ybase + 1, nc = src_of(sc.rw, Xl, sc.Ws).i1 - xbase + 1;
                for (int i = tid; i < nr * nc; i += 256) {                 // (host: nr * nc * CS <= PT_PATCH for every tile)
                    const int pr = i / nc, pc = i - pr * nc;
                    float q[C];
                    pt_pair<C>(sc, z, zf, ybase + pr, xbase + pc, q);
#pragma unroll
                    for (int c = 0; c < C; ++c) s_patch[i * CS + c] = q[c];
                }
                __syncthreads();
                // lerp_v(lerp_h(q00, q01), lerp_h(q10, q11)): where K16 skips a tap (weight 0, or i1 == i0) it puts q00 (q10) in its
                // place and fmaf(0, q00, 1 * q00) = fmaf(0, q01, 1 * q00) for any finite q01
                const Src ty = src_of(sc.rh, Yc, sc.Hs), tx = src_of(sc.rw, Xc, sc.Ws);
                const float* q00 = s_patch + ((ty.i0 - ybase) * nc + (tx.i0 - xbase)) * CS;
                const float* q01 = s_patch + ((ty.i0 - ybase) * nc + (tx.i1 - xbase)) * CS;
                const float* q10 = s_patch + ((ty.i1 - ybase) * nc + (tx.i0 - xbase)) * CS;
                const float* q11 = s_patch + ((ty.i1 - ybase) * nc + (tx.i1 - xbase)) * CS;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float top = lerp_h(q00[c], q01[c], tx.l0, tx.l1);
                    const float bot = lerp_h(q10[c], q11[c], tx.l0, tx.l1);
                    tot[c] = tot[c] + lerp_v(top, bot, ty.l0, ty.l1);
                }
                __syncthreads();                                           // the next scale overwrites the patch
            } else {
                pt_scale_direct<C>(sc, z, zf, Yc, Xc, tot);
            }
        }

        float m = tot[0];
        int am = 0;
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (tot[c] > m) { m = tot[c]; am = c; }                         // first max wins ties
        const float prob = fminf(m / nviews, 1.0f);                         // IEEE division; the sum can exceed n_views by rounding

        unsigned key = 0xFFFFFFFFu;
        if (live) {
            const size_t o = ((size_t)b * H + Y) * W + X;
            maxprob[o] = prob;
            argmax[o] = (uint8_t)am;
            const unsigned bin = __half_as_ushort(__float2half_rn(prob));
            if (bin >= HIAST_NBINS - PT_TOPB && bin < HIAST_NBINS)
                atomicAdd(&s_top[am * PT_TOPB + (int)(bin - (HIAST_NBINS - PT_TOPB))], 1u);
            else if (bin < HIAST_NBINS) key = (unsigned)am * HIAST_NBINS + bin;
        }
        // the keys not counted in LDS: two wave-aggregated rounds take out the keys many lanes share, the lanes that are left
        // add their own count (pass 1's scheme; integer sums are the same in any order)
        unsigned long long todo = __ballot(key != 0xFFFFFFFFu);
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            if (!todo) break;
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned k = __shfl(key, leader, 64);
            const unsigned long long same = __ballot(key == k);
            if (lane_id() == leader) atomicAdd(&cnt[SCATTER ? pt_slot<C>(k) : k], (unsigned)__popcll(same));
            todo &= ~same;
        }
        if ((todo >> lane_id()) & 1ull) atomicAdd(&cnt[SCATTER ? pt_slot<C>(key) : key], 1u);
    }

    __syncthreads();
    for (int i = tid; i < C * PT_TOPB; i += 256) {
        const unsigned v = s_top[i];
        const unsigned k = (unsigned)(i / PT_TOPB) * HIAST_NBINS + (HIAST_NBINS - PT_TOPB) + (unsigned)(i % PT_TOPB);
        if (v) atomicAdd(&cnt[SCATTER ? pt_slot<C>(k) : k], v);
    }
}

// src_of's indices on the host (the same single fp32 product)
static inline void pt_host_src(float scale, int dst, int in, int* i0, int* i1)
{
    const float f = scale * (float)dst;
    int a = (int)f;
    a = a > in - 1 ? in - 1 : a;
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
}
// most size-s rows (columns) a tile of `tile` native rows (columns) reads taps from
static int pt_host_extent(float scale, int n, int in, int tile)
{
    int most = 0;
    for (int d0 = 0; d0 < n; d0 += tile) {
        const int dl = d0 + tile - 1 < n ? d0 + tile - 1 : n - 1;
        int a0, a1, b0, b1;
        pt_host_src(scale, d0, in, &a0, &a1);
        pt_host_src(scale, dl, in, &b0, &b1);
        if (b1 - a0 + 1 > most) most = b1 - a0 + 1;
    }
    return most;
}

template <int C>
static int launch_pass1_tta(const PtArgs& a, int B, int H, int W, int n_views, float* maxprob, uint8_t* argmax, uint32_t* hist,
                            uint32_t* ws, hipStream_t st)
{
    constexpr int CS = C | 1;
    // HIAST_PLTTA_FORM (tuning override, for A/B timing): "direct" = never the tiled form
    const char* form = getenv("HIAST_PLTTA_FORM");
    bool tiled = !(form && form[0] == 'd');
    for (int i = 0; i < a.n && tiled; ++i) {
        const long long nr = pt_host_extent(a.s[i].rh, H, a.s[i].Hs, PT_TH), nc = pt_host_extent(a.s[i].rw, W, a.s[i].Ws, PT_TW);
        if (nr * nc * CS > PT_PATCH) tiled = false;
    }
    const int ntx = (W + PT_TW - 1) / PT_TW, nty = (H + PT_TH - 1) / PT_TH;
    const long long ntiles = (long long)ntx * nty * B;
    // the tiled form's LDS leaves two blocks per CU; the direct form is bounded by its registers
    const long long want = (long long)hiast_grid_cus() * (tiled ? 2 : 4);
    const unsigned blocks = (unsigned)(ntiles < want ? ntiles : want);
    if (ws) {
        const hipError_t e0 = hipMemsetAsync(ws, 0, (size_t)256 * C * PT_PLANE * sizeof(uint32_t), st);
        if (e0 != hipSuccess) return (int)e0;
    }
#define HIAST_PT(T, S)                                                                                                       \
    hipLaunchKernelGGL((plabel_tta_kernel<C, T, S>), dim3(blocks), dim3(256), 0, st, a, H, W, ntx, nty, ntiles, (float)n_views, \
                       maxprob, argmax, S ? ws : hist)
    if (ws) { if (tiled) HIAST_PT(true, true); else HIAST_PT(false, true); }
    else    { if (tiled) HIAST_PT(true, false); else HIAST_PT(false, false); }
#undef HIAST_PT
    HIAST_CHECK_LAUNCH();
    if (ws) {
        hipLaunchKernelGGL(pt_merge_kernel<C>, dim3((C * HIAST_NBINS + 255) / 256), dim3(256), 0, st, ws, hist);
        HIAST_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace hiast

extern "C" size_t hiast_plabel_pass1_tta_workspace_bytes(int C)
{
    return (C == 19 || C == 16 || C == 9 || C == 2) ? (size_t)256 * C * hiast::PT_PLANE * sizeof(uint32_t) : 0;
}

extern "C" int hiast_plabel_pass1_tta(const float* const* z, const float* const* zf, const int* hs, const int* ws, const int* Hs,
                                      const int* Ws, int n_scales, int B, int C, int H, int W, float* maxprob, uint8_t* argmax,
                                      uint32_t* hist, void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    if (!z || !hs || !ws || !Hs || !Ws || !maxprob || !argmax || !hist) return HIAST_E_ARG;
    if (n_scales <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    if (n_scales > HIAST_TTA_MAX_SCALES || B > 65535 || H > 65535) return HIAST_E_RANGE;
    hiast::PtArgs a;
    a.n = n_scales;
    for (int i = 0; i < n_scales; ++i) {
        if (!z[i] || (zf && !zf[i]) || hs[i] <= 0 || ws[i] <= 0 || Hs[i] < hs[i] || Ws[i] < ws[i]) return HIAST_E_ARG;
        hiast::PtScale& s = a.s[i];
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
    if (!(C == 19 || C == 16 || C == 9 || C == 2)) return HIAST_E_RANGE;
    if (workspace && (workspace_bytes < hiast_plabel_pass1_tta_workspace_bytes(C) || (((uintptr_t)workspace) & 3))) return HIAST_E_WS;
    const int n_views = n_scales * (zf ? 2 : 1);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* wsp = (uint32_t*)workspace;
    uint32_t* h32 = hist;
    switch (C) {
        case 19: return hiast::launch_pass1_tta<19>(a, B, H, W, n_views, maxprob, argmax, h32, wsp, st);
        case 16: return hiast::launch_pass1_tta<16>(a, B, H, W, n_views, maxprob, argmax, h32, wsp, st);
        case 9: return hiast::launch_pass1_tta<9>(a, B, H, W, n_views, maxprob, argmax, h32, wsp, st);
        default: return hiast::launch_pass1_tta<2>(a, B, H, W, n_views, maxprob, argmax, h32, wsp, st);
    }
}
