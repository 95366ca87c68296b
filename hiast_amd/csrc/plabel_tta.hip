// K3c — pseudo-label pass 1 over several views (multi-scale + flip): hiast_plabel_pass1_tta.  gfx950 only.
//
// The validator's view averaging with pass 1's outputs, both through plabel_common.h: from the LOW-RES head outputs of every
// (scale, flip) forward to (maxprob, argmax, hist) in one kernel.  Per native pixel
//   tot[c]  = Σ_scales resample_to_native( softmax(up(z_s)) + flip(softmax(up(zf_s))) )[c]      — view_scale_direct's operations
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
//           the direct form evaluates up to four.
//   direct  the thread-per-pixel form (each pixel evaluates its own taps): taken when a scale's footprint does not fit
//           the LDS patch (size ratios above ~1.5 at 19 classes).
// Histogram: the shared counters — the top bins of every class in LDS (flushed once per block, a block works through many
// tiles), two wave-aggregated rounds + one atomic per remaining lane for the rest, into the scattered workspace that a merge
// launch adds into hist, or straight into hist without one.
#include <stdlib.h>

#include "plabel_common.h"

namespace hiast {

constexpr int PT_TH = 8, PT_TW = 32;              // native pixels per tile: 256 threads, one each
constexpr int PT_PATCH = 12288;                   // floats of LDS for a scale's probability patch (48 KiB)

// One block works through the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (x tile fastest, then y tile, then image).
// cnt: the scattered workspace (SCATTER) or the caller's hist.
template <int C, bool TILED, bool SCATTER>
__global__ __launch_bounds__(256) void plabel_tta_kernel(ViewArgs a, int H, int W, int ntx, int nty, long long ntiles, float nviews,
                                                         float* __restrict__ maxprob, uint8_t* __restrict__ argmax,
                                                         uint32_t* __restrict__ cnt)
{
    constexpr int CS = C | 1;                     // odd row stride of the patch: lanes on consecutive pixels hit different banks
    __shared__ unsigned s_top[C * TOPB];
    __shared__ float s_patch[TILED ? PT_PATCH : 1];
    const int tid = threadIdx.x;
    top_zero<C>(s_top);
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
            const ViewScale sc = a.s[si];
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
                    view_pair<C>(sc, z, zf, ybase + pr, xbase + pc, q);
#pragma unroll
                    for (int c = 0; c < C; ++c) s_patch[i * CS + c] = q[c];
                }
                __syncthreads();
                // lerp_v(lerp_h(q00, q01), lerp_h(q10, q11)): where the direct form skips a tap (weight 0, or i1 == i0) it puts q00
                // (q10) in its place and fmaf(0, q00, 1 * q00) = fmaf(0, q01, 1 * q00) for any finite q01
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
                view_scale_direct<C>(sc, z, zf, Yc, Xc, tot);
            }
        }

        float m = tot[0];
        int am = 0;
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (tot[c] > m) { m = tot[c]; am = c; }                         // first max wins ties
        const float prob = fminf(m / nviews, 1.0f);                         // IEEE division; the sum can exceed n_views by rounding

        unsigned key = NOKEY;
        if (live) {
            const size_t o = ((size_t)b * H + Y) * W + X;
            maxprob[o] = prob;
            argmax[o] = (uint8_t)am;
            key = top_count(s_top, am, __half_as_ushort(__float2half_rn(prob)));
        }
        wave_add<2, C, SCATTER>(cnt, key);                                  // the keys not counted in LDS
    }

    __syncthreads();
    top_flush<C, SCATTER>(s_top, cnt);
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
static int launch_pass1_tta(const ViewArgs& a, int B, int H, int W, int n_views, float* maxprob, uint8_t* argmax, uint32_t* hist,
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
        const int e0 = hist_ws_clear(ws, C, st);
        if (e0) return e0;
    }
#define HIAST_PT(T, S)                                                                                                       \
    hipLaunchKernelGGL((plabel_tta_kernel<C, T, S>), dim3(blocks), dim3(256), 0, st, a, H, W, ntx, nty, ntiles, (float)n_views, \
                       maxprob, argmax, S ? ws : hist)
    if (ws) { if (tiled) HIAST_PT(true, true); else HIAST_PT(false, true); }
    else    { if (tiled) HIAST_PT(true, false); else HIAST_PT(false, false); }
#undef HIAST_PT
    HIAST_CHECK_LAUNCH();
    return ws ? hist_ws_merge(ws, hist, C, st) : 0;
}

}  // namespace hiast

extern "C" size_t hiast_plabel_pass1_tta_workspace_bytes(int C)
{
    return hiast::for_class_count(C, [](auto) {}) ? hiast::hist_ws_bytes(C) : 0;
}

extern "C" int hiast_plabel_pass1_tta(const float* const* z, const float* const* zf, const int* hs, const int* ws, const int* Hs,
                                      const int* Ws, int n_scales, int B, int C, int H, int W, float* maxprob, uint8_t* argmax,
                                      uint32_t* hist, void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    if (!maxprob || !argmax || !hist) return HIAST_E_ARG;
    hiast::ViewArgs a;
    const int bad = hiast::view_args_fill(a, z, zf, hs, ws, Hs, Ws, n_scales, B, C, H, W);
    if (bad) return bad;
    const size_t need = hiast_plabel_pass1_tta_workspace_bytes(C);
    if (!need) return HIAST_E_RANGE;
    if (workspace && (workspace_bytes < need || (((uintptr_t)workspace) & 3))) return HIAST_E_WS;
    const int n_views = n_scales * (zf ? 2 : 1);
    int rc = HIAST_E_RANGE;
    hiast::for_class_count(C, [&](auto cc) {
        rc = hiast::launch_pass1_tta<decltype(cc)::value>(a, B, H, W, n_views, maxprob, argmax, hist, (uint32_t*)workspace,
                                                          (hipStream_t)stream);
    });
    return rc;
}
