// K3b / K16 — the generator policies and the validator either side of the IAS path.  gfx950 only.
//
// K3b  hiast_plabel_strided_hist: the CBST policy's confidence sample
//      (workflows/pseudo_label_generator.py:142-158): per class, every `interval`-th element of
//      `probs_pred[lbls_pred == c]` — i.e. of the class's pixels in raster order over the batch — enters the
//      per-class fp16 list.  Here: the rank of a pixel within its class comes from a block-count + scan + in-block
//      ballot ranking, the kept pixels go into the same [C, NBINS] integer histogram pass 1 uses.
// K16  hiast_tta_fused: Validator.get_multi_scale_and_flip_logits + argmax (workflows/validator.py:34-55,92):
//      Σ_scales resample_to_native( softmax(up(z_s)) + flip(softmax(up(z_s,flipped))) ) from the LOW-RES head outputs
//      of every (scale, flip) forward in one kernel: neither the full-resolution logits nor the per-scale probability
//      maps (39.8 MB/img each at 512x1024) are ever stored; the output is the uint8 label map (+ optionally the
//      summed probabilities for the API that returns them).  The per-view arithmetic, the view arguments and their
//      checks are those of plabel_common.h.
#include "plabel_common.h"

namespace hiast {

constexpr int SH_TILE = 4096;     // pixels per block (16 rounds of 256)

// rank of every lane's pixel among the pixels of ITS class within the 256-pixel round, and the per-class totals of
// the round; s_w[4][MAX_CLASSES] is scratch.  Returns -1 for lanes without a class.
__device__ __forceinline__ int round_rank(int cls, unsigned* s_w, unsigned* s_tot)
{
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x < 4 * HIAST_MAX_CLASSES) s_w[threadIdx.x] = 0;
    __syncthreads();
    int rk = -1;
    unsigned long long todo = __ballot(cls >= 0);
    const unsigned long long lt = (1ull << lane_id()) - 1ull;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(cls, leader, 64);
        const unsigned long long same = __ballot(cls == k);
        if (cls == k) rk = __popcll(same & lt);
        if (lane_id() == leader) s_w[wave * HIAST_MAX_CLASSES + k] = (unsigned)__popcll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (cls >= 0)
        for (int w = 0; w < wave; ++w) rk += (int)s_w[w * HIAST_MAX_CLASSES + cls];
    if (threadIdx.x < HIAST_MAX_CLASSES)
        s_tot[threadIdx.x] = s_w[threadIdx.x] + s_w[HIAST_MAX_CLASSES + threadIdx.x] +
                             s_w[2 * HIAST_MAX_CLASSES + threadIdx.x] + s_w[3 * HIAST_MAX_CLASSES + threadIdx.x];
    __syncthreads();
    return rk;
}

// MODE 0: per-block class counts -> cnt[nblk][C];  MODE 1: histogram of the kept pixels, base[nblk][C] = rank of the
// block's first pixel of each class (mod interval)
template <int MODE>
__global__ __launch_bounds__(256) void strided_hist_kernel(const float* __restrict__ maxprob,
                                                           const uint8_t* __restrict__ argmax, long long N, int C,
                                                           int interval, unsigned* __restrict__ blk,
                                                           uint32_t* __restrict__ hist)
{
    __shared__ unsigned s_w[4 * HIAST_MAX_CLASSES];
    __shared__ unsigned s_tot[HIAST_MAX_CLASSES];
    __shared__ unsigned s_run[HIAST_MAX_CLASSES];
    const long long t0 = (long long)blockIdx.x * SH_TILE;
    if (threadIdx.x < HIAST_MAX_CLASSES)
        s_run[threadIdx.x] = (MODE == 1 && (int)threadIdx.x < C) ? blk[(size_t)blockIdx.x * C + threadIdx.x] : 0u;
    __syncthreads();
    for (int r = 0; r < SH_TILE / 256; ++r) {
        const long long i = t0 + r * 256 + threadIdx.x;
        int cls = -1;
        if (i < N) {
            const int a = argmax[i];
            cls = a < C ? a : -1;
        }
        if (MODE == 0) {
            wave_add<0>(s_run, (unsigned)cls);                 // counts only, in LDS; cls -1 is NOKEY
        } else {
            const int rk = round_rank(cls, s_w, s_tot);
            unsigned key = NOKEY;
            if (cls >= 0 && ((s_run[cls] + (unsigned)rk) % (unsigned)interval) == 0u) {
                const unsigned bin = __half_as_ushort(__float2half_rn(maxprob[i]));
                if (bin < HIAST_NBINS) key = (unsigned)cls * HIAST_NBINS + bin;
            }
            wave_add<0>(hist, key);
            __syncthreads();       // every lane has read s_run before it moves on
            if ((int)threadIdx.x < C) s_run[threadIdx.x] = (s_run[threadIdx.x] + s_tot[threadIdx.x]) % (unsigned)interval;
            __syncthreads();
        }
    }
    if (MODE == 0) {
        __syncthreads();
        if ((int)threadIdx.x < C) blk[(size_t)blockIdx.x * C + threadIdx.x] = s_run[threadIdx.x];
    }
}

// exclusive scan over blocks per class (mod interval), seeded with the ranks' offset; also the batch totals
__global__ void strided_scan_kernel(unsigned* __restrict__ blk, int nblk, int C, int interval,
                                    const long long* __restrict__ rank_offset, long long* __restrict__ class_total)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    unsigned run = rank_offset ? (unsigned)(rank_offset[c] % interval) : 0u;
    long long tot = 0;
    for (int b = 0; b < nblk; ++b) {
        const unsigned n = blk[(size_t)b * C + c];
        blk[(size_t)b * C + c] = run;
        run = (run + n) % (unsigned)interval;
        tot += n;
    }
    if (class_total) class_total[c] = tot;
}

// ---------------------------------------------------------------------------------------------------------------
// K16.  One thread per native pixel, every tap of every scale evaluated by that thread (view_scale_direct).
template <int C>
__global__ __launch_bounds__(256) void tta_fused_kernel(ViewArgs a, int B, int H, int W, float* __restrict__ probsum,
                                                        uint8_t* __restrict__ label)
{
    const int X = blockIdx.x * 256 + threadIdx.x;
    const int Y = blockIdx.y, b = blockIdx.z;
    if (X >= W) return;
    float tot[C];
#pragma unroll
    for (int c = 0; c < C; ++c) tot[c] = 0.0f;
    for (int si = 0; si < a.n; ++si) {
        const ViewScale sc = a.s[si];
        const float* z = sc.z + (size_t)b * C * sc.hs * sc.ws;
        const float* zf = sc.zf ? sc.zf + (size_t)b * C * sc.hs * sc.ws : nullptr;
        view_scale_direct<C>(sc, z, zf, Y, X, tot);
    }
    const size_t pix = ((size_t)b * H + Y) * W + X;
    if (probsum) {
#pragma unroll
        for (int c = 0; c < C; ++c) probsum[((size_t)b * C + c) * H * W + (size_t)Y * W + X] = tot[c];
    }
    if (label) {
        float m = tot[0];
        int am = 0;
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (tot[c] > m) { m = tot[c]; am = c; }
        label[pix] = (uint8_t)am;
    }
}

}  // namespace hiast

extern "C" size_t hiast_plabel_strided_hist_workspace_bytes(int64_t N, int C)
{
    if (N <= 0 || C <= 0) return 0;
    const long long nblk = (N + hiast::SH_TILE - 1) / hiast::SH_TILE;
    return (size_t)nblk * C * sizeof(unsigned);
}

extern "C" int hiast_plabel_strided_hist(const float* maxprob, const uint8_t* argmax, int64_t N, int C, int interval,
                                         const int64_t* rank_offset, int64_t* class_total, uint32_t* hist,
                                         void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    if (!maxprob || !argmax || !hist || !workspace) return HIAST_E_ARG;
    if (N <= 0 || C <= 0 || interval <= 0) return HIAST_E_ARG;
    if (C > HIAST_MAX_CLASSES) return HIAST_E_RANGE;
    const long long nblk = (N + hiast::SH_TILE - 1) / hiast::SH_TILE;
    if (nblk > 0x7fffffffLL) return HIAST_E_RANGE;
    if (workspace_bytes < (size_t)nblk * C * sizeof(unsigned)) return HIAST_E_WS;
    hipStream_t st = (hipStream_t)stream;
    unsigned* blk = (unsigned*)workspace;
    hipLaunchKernelGGL(hiast::strided_hist_kernel<0>, dim3((unsigned)nblk), dim3(256), 0, st, maxprob, argmax,
                       (long long)N, C, interval, blk, hist);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::strided_scan_kernel, dim3(1), dim3(64), 0, st, blk, (int)nblk, C, interval,
                       (const long long*)rank_offset, (long long*)class_total);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::strided_hist_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, st, maxprob, argmax,
                       (long long)N, C, interval, blk, hist);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_tta_fused(const float* const* z, const float* const* zf, const int* hs, const int* ws,
                               const int* Hs, const int* Ws, int n_scales, int B, int C, int H, int W, float* probsum,
                               uint8_t* label, hiast_stream_t stream)
{
    if (!probsum && !label) return HIAST_E_ARG;
    hiast::ViewArgs a;
    const int bad = hiast::view_args_fill(a, z, zf, hs, ws, Hs, Ws, n_scales, B, C, H, W);
    if (bad) return bad;
    const bool known = hiast::for_class_count(C, [&](auto cc) {
        hipLaunchKernelGGL(hiast::tta_fused_kernel<decltype(cc)::value>, dim3((W + 255) / 256, H, B), dim3(256), 0,
                           (hipStream_t)stream, a, B, H, W, probsum, label);
    });
    if (!known) return HIAST_E_RANGE;
    HIAST_CHECK_LAUNCH();
    return 0;
}
