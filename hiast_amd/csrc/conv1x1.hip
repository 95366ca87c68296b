// K9a — 1x1 bottleneck projections of the ResNet trunk for the fp32 (pseudo-label) forward, as ONE
// fused kernel: GEMM + BatchNorm(eval) + residual add + ReLU
// (reference: Bottleneck.forward, sseg/models/modules/resnet.py:78-98: conv1 -> bn1 -> relu and
//  conv3 -> bn3 -> += identity -> relu, each a separate cuDNN / ATen pass there).
//
//   Y[m][n] = act( (Σ_k X[m][k] * W[n][k]) * scale_n + shift_n (+ R[m][n]) )
//   X: [M = B*H*W pixels][K = Cin]  fp32, NHWC (channels-last) activations
//   W: [N = Cout][K]                fp32 (the conv weight [Cout,Cin,1,1] as stored)
//
// Arithmetic: "split-bf16": every fp32 operand is split on the fly into hi = bf16(v) and
// lo = bf16(v - hi); the product is accumulated in fp32 as hi*hi + hi*lo + lo*hi on
// v_mfma_f32_32x32x16_bf16 (the dropped lo*lo term is 2^-16 relative).  Measured |err| vs fp64 is
// ~5e-6 of max|Y| (fp32 MFMA: ~2e-6; plain bf16: 2e-3), well inside the 1e-3 logits contract, at
// 3/16 of the fp32-MFMA cost: gfx950 has no TF32/xf32 path, this is the fast exact-class option.
//
// Structure: 128 x BN block tile (BN = 128 or 64), BK = 32, 4 waves as 2 x 2 (wave tile 64 x BN/2),
// register-staged global loads (fp32 -> hi/lo happens between the load and the LDS write), LDS double
// buffered with one barrier per k-step, rows padded to 80 B so ds_read_b128 fragments are conflict free.
#include <hip/hip_bf16.h>

#include "common.h"

namespace hiast {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int C1_BM = 128;
constexpr int C1_BK = 32;
constexpr int C1_PITCH = 32;      // bf16 elements per LDS row: 64 bytes, no padding

// LDS image of a [rows][32 bf16] tile: 64-byte rows whose four 16-byte chunks are XOR-swizzled with
// (row >> 2) & 3.  A ds_read_b128 fragment read (16 lanes = 16 rows, same logical chunk) then touches
// 16 distinct 4-bank columns and a ds_write_b64 staging store (16 lanes = 2 whole rows) 32 distinct banks:
// both conflict free (the padded 80-byte rows measured 33 % of LDS cycles as bank conflicts on the stores).
__device__ __forceinline__ int lds_off(int row, int chunk16) { return row * 64 + ((chunk16 ^ ((row >> 2) & 3)) << 4); }

__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& lo)
{
    const float f[4] = {v.x, v.y, v.z, v.w};
    unsigned short h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __hip_bfloat16 hb = __float2bfloat16(f[i]);
        const float hf = __bfloat162float(hb);
        const __hip_bfloat16 lb = __float2bfloat16(f[i] - hf);
        h[i] = __bfloat16_as_ushort(hb);
        l[i] = __bfloat16_as_ushort(lb);
    }
    hi = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    lo = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
}

// geometry of the 3x3 variant (TAPS == 9): input H x W, output Ho x Wo, stride, dilation (padding = dilation);
// K is then the number of input channels and the GEMM reduction runs over 9 taps x K
struct ConvGeo {
    int H, W, Ho, Wo, stride, dil;
};

// TA = float : fp32 activations, split-bf16 arithmetic (3 MFMAs per operand pair)   [pseudo-label forward]
// TA = bf16  : bf16 activations in/out, plain bf16 MFMA (fp32 accumulate), weights converted from the fp32
//              master copy while staging                                           [teacher forward under AMP]
// TO = output (and residual) element type: TA, or float for a bf16 GEMM whose result is consumed in fp32
// (the ASPP tap GEMM of aspp2.hip).  mean == nullptr: no BatchNorm (scale 1, shift 0) — a plain GEMM.
template <typename TA, typename TO, int BN, int TAPS, bool RES, bool RELU>
__global__ __launch_bounds__(256) void conv1x1_bn_act_kernel(
    const TA* __restrict__ X, const float* __restrict__ W, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, float eps,
    const TO* __restrict__ R, TO* __restrict__ Y, int M, int K, int N, ConvGeo geo)
{
    constexpr bool SPLIT = sizeof(TA) == 4;
    constexpr int TN = BN / 64;                       // 32-wide column tiles per wave (2 or 1)
    constexpr int A_F4 = SPLIT ? C1_BM * C1_BK / 4 / 256 : C1_BM * C1_BK / 8 / 256;   // 16-byte loads per thread (4 | 2)
    constexpr int B_F4 = BN * C1_BK / 4 / 256;        // 4 or 2 (weights are always fp32)
    // [buf][A_hi | A_lo | B_hi | B_lo]   (the *_lo planes exist only in split mode)
    constexpr int A_BYTES = C1_BM * C1_PITCH * 2, B_BYTES = BN * C1_PITCH * 2;
    constexpr int BUF_BYTES = (SPLIT ? 2 : 1) * (A_BYTES + B_BYTES);
    constexpr int A_LO = A_BYTES, B_HI = (SPLIT ? 2 : 1) * A_BYTES, B_LO = B_HI + B_BYTES;
    constexpr int EPI_BYTES = C1_BM * (BN + 4) * 4;
    constexpr int SMEM_BYTES = 2 * BUF_BYTES > EPI_BYTES ? 2 * BUF_BYTES : EPI_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware tile order: work items are numbered with the channel tile fastest, and XCD k (workgroup ids
    // k, k+8, ... under round-robin dispatch) takes the k-th contiguous eighth of them, so the column blocks
    // that re-read one 128-row activation tile run back to back on ONE L2 instead of on eight.
    int bm, bn_;
    {
        const int gx = gridDim.x, gy = gridDim.y, total = gx * gy;
        int lid = blockIdx.x + gx * blockIdx.y;
        if ((total & 7) == 0) lid = (lid & 7) * (total >> 3) + (lid >> 3);
        bn_ = lid % gy;
        bm = lid / gy;
    }
    const int m0 = bm * C1_BM, n0 = bn_ * BN;
    const int kchunks = K / C1_BK;
    const int nk = TAPS * kchunks;

    f32x16 acc[2][TN];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // global -> register staging: float4 index f = tid + 256*i; row = f / 8, c4 = f % 8.  A thread's rows are
    // the same for every k-step; for the 3x3 variant their (image, y, x) is decoded once and each tap only
    // shifts it (out-of-image taps load a valid address and are zeroed by a select: no conditional loads).
    constexpr int A_ROW_SHIFT = SPLIT ? 3 : 2;        // 16-byte loads per 32-element row: 8 (fp32) | 4 (bf16)
    constexpr int A_PER = SPLIT ? 4 : 8;              // elements per 16-byte load
    uint4 ra[A_F4];
    float4 rb[B_F4];
    int rn[A_F4], ry[A_F4], rx[A_F4];
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
        int m = m0 + ((tid + 256 * i) >> A_ROW_SHIFT);
        m = m < M ? m : M - 1;                                       // tail rows: valid address, never stored
        if (TAPS == 1) {
            rn[i] = m; ry[i] = 0; rx[i] = 0;
        } else {
            const int hw = geo.Ho * geo.Wo;
            rn[i] = m / hw;
            const int r = m - rn[i] * hw;
            ry[i] = (r / geo.Wo) * geo.stride;
            rx[i] = (r - (r / geo.Wo) * geo.Wo) * geo.stride;
        }
    }
    // Raw buffer loads: a lane whose tap falls outside the image gets a byte offset beyond num_records and
    // the hardware returns zeros — zero padding without a select, which the optimiser turns back into a
    // branch around the load (and a branchy load costs an s_waitcnt vmcnt(0) each).
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const unsigned x_bytes = (unsigned)(((TAPS == 1) ? (size_t)M : (size_t)(M / (geo.Ho * geo.Wo)) * geo.H * geo.W) *
                                        K * sizeof(TA));
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)x_bytes, 0x00020000);
    constexpr int OOB = (int)0x80000000;
    auto gload = [&](int kt) {
        const int tap = TAPS == 1 ? 0 : kt / kchunks;
        const int k0 = (TAPS == 1 ? kt : kt - tap * kchunks) * C1_BK;
        const int oy = TAPS == 1 ? 0 : (tap / 3 - 1) * geo.dil, ox = TAPS == 1 ? 0 : (tap % 3 - 1) * geo.dil;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) {
            const int cc = (tid + 256 * i) & ((1 << A_ROW_SHIFT) - 1);
            if (TAPS == 1) {
                ra[i] = *reinterpret_cast<const uint4*>(X + (size_t)rn[i] * K + k0 + cc * A_PER);
            } else {
                const int yy = ry[i] + oy, xx = rx[i] + ox;
                const bool ok = yy >= 0 && yy < geo.H && xx >= 0 && xx < geo.W;
                const int pix = (rn[i] * geo.H + yy) * geo.W + xx;
                const int voff = ok ? (int)(((size_t)pix * K + k0 + cc * A_PER) * sizeof(TA)) : OOB;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, 0, 0);
                ra[i] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }
#pragma unroll
        for (int i = 0; i < B_F4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
            rb[i] = *reinterpret_cast<const float4*>(W + (size_t)(n0 + row) * (TAPS * K) + kt * C1_BK + c4 * 4);
        }
    };
    auto lds_store = [&](int buf) {
        unsigned char* base = smem + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) {
            const int f = tid + 256 * i, row = f >> A_ROW_SHIFT, cc = f & ((1 << A_ROW_SHIFT) - 1);
            if (SPLIT) {
                uint2 hi, lo;
                const float4 v = make_float4(__uint_as_float(ra[i].x), __uint_as_float(ra[i].y),
                                             __uint_as_float(ra[i].z), __uint_as_float(ra[i].w));
                split4(v, hi, lo);
                *reinterpret_cast<uint2*>(base + lds_off(row, cc >> 1) + (cc & 1) * 8) = hi;
                *reinterpret_cast<uint2*>(base + A_LO + lds_off(row, cc >> 1) + (cc & 1) * 8) = lo;
            } else {
                *reinterpret_cast<uint4*>(base + lds_off(row, cc)) = ra[i];
            }
        }
#pragma unroll
        for (int i = 0; i < B_F4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
            uint2 hi, lo;
            split4(rb[i], hi, lo);
            *reinterpret_cast<uint2*>(base + B_HI + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = hi;
            if (SPLIT) *reinterpret_cast<uint2*>(base + B_LO + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = lo;
        }
    };

    gload(0);
    lds_store(0);
    __syncthreads();

    const int frow = lane & 31, fchunk = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const unsigned char* base = smem + buf * BUF_BYTES;
#pragma unroll
        for (int kk = 0; kk < C1_BK / 16; ++kk) {
            bf16x8 ah[2], al[2], bh[TN], bl[TN];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int off = lds_off(wm * 64 + a * 32 + frow, kk * 2 + fchunk);
                ah[a] = *reinterpret_cast<const bf16x8*>(base + off);
                if (SPLIT) al[a] = *reinterpret_cast<const bf16x8*>(base + A_LO + off);
            }
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int off = lds_off(wn * (BN / 2) + b * 32 + frow, kk * 2 + fchunk);
                bh[b] = *reinterpret_cast<const bf16x8*>(base + B_HI + off);
                if (SPLIT) bl[b] = *reinterpret_cast<const bf16x8*>(base + B_LO + off);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    if (SPLIT) {
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
                    }
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
                }
        }
        if (kt + 1 < nk) lds_store(buf ^ 1);
        __syncthreads();
    }

    // epilogue through LDS (the staging buffers are free now): accumulators -> fp32 tile [128][BN+4] with
    // the BN scale/shift applied, then every thread moves float4s along the channel axis, so the
    // residual read and the output write are whole 512-byte row segments (16 B per lane) instead of
    // 4-byte accesses (the K <= 256 "expanding" convs are bound by exactly this traffic).
    constexpr int CP = BN + 4;
    float* sC = reinterpret_cast<float*>(smem);
    __syncthreads();          // (the last k-step's barrier already passed; keeps the reuse of smem explicit)
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int nl = wn * (BN / 2) + b * 32 + (lane & 31);
        const int n = n0 + nl;
        float sc = 1.0f, sh = 0.0f;
        if (mean) {
            const float invstd = 1.0f / sqrtf(var[n] + eps);
            sc = (gamma ? gamma[n] : 1.0f) * invstd;
            sh = fmaf(-mean[n], sc, beta ? beta[n] : 0.0f);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                sC[ml * CP + nl] = fmaf(acc[a][b][r], sc, sh);
            }
    }
    __syncthreads();
    if (sizeof(TO) == 4) {
        constexpr int F4_PER_ROW = BN / 4;
#pragma unroll 4
        for (int f = tid; f < C1_BM * F4_PER_ROW; f += 256) {
            const int ml = f / F4_PER_ROW, c4 = f - ml * F4_PER_ROW;
            const int m = m0 + ml;
            if (m >= M) continue;
            float4 o = *reinterpret_cast<const float4*>(sC + ml * CP + c4 * 4);
            const size_t g = (size_t)m * N + n0 + c4 * 4;
            if (RES) {
                const float4 rr = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(R) + g);
                o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w;
            }
            if (RELU) {
                o.x = o.x > 0.f ? o.x : 0.f; o.y = o.y > 0.f ? o.y : 0.f;
                o.z = o.z > 0.f ? o.z : 0.f; o.w = o.w > 0.f ? o.w : 0.f;
            }
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(Y) + g) = o;
        }
    } else {
        constexpr int V8_PER_ROW = BN / 8;
#pragma unroll 4
        for (int f = tid; f < C1_BM * V8_PER_ROW; f += 256) {
            const int ml = f / V8_PER_ROW, c8 = f - ml * V8_PER_ROW;
            const int m = m0 + ml;
            if (m >= M) continue;
            float o[8];
            const float4 o0 = *reinterpret_cast<const float4*>(sC + ml * CP + c8 * 8);
            const float4 o1 = *reinterpret_cast<const float4*>(sC + ml * CP + c8 * 8 + 4);
            o[0] = o0.x; o[1] = o0.y; o[2] = o0.z; o[3] = o0.w; o[4] = o1.x; o[5] = o1.y; o[6] = o1.z; o[7] = o1.w;
            const size_t g = (size_t)m * N + n0 + c8 * 8;
            if (RES) {
                const uint4 rr = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(R) + g);
                const unsigned wds[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[2 * q] += __uint_as_float(wds[q] << 16);
                    o[2 * q + 1] += __uint_as_float(wds[q] & 0xFFFF0000u);
                }
            }
            unsigned pk[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a0 = o[2 * q], a1 = o[2 * q + 1];
                if (RELU) { a0 = a0 > 0.f ? a0 : 0.f; a1 = a1 > 0.f ? a1 : 0.f; }
                pk[q] = (unsigned)__bfloat16_as_ushort(__float2bfloat16(a0)) |
                        ((unsigned)__bfloat16_as_ushort(__float2bfloat16(a1)) << 16);
            }
            *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(Y) + g) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
    }
}

// NHWC BatchNorm(eval) (+ReLU) for the activations that come out of the library 3x3 / 7x7 convolutions:
// y[m][c] = act(x[m][c]*scale_c + shift_c), VEC channels per thread (one 16-byte word), C % VEC == 0.
// A thread's channels do not change along its grid-stride walk when the stride is a multiple of C (the launcher picks the
// grid that way whenever C divides 256 * VEC * k): scale / shift are then derived ONCE per thread, and four words are
// requested before the first is used.  (The first form derived 1/sqrt(var + eps) per element and kept one word in flight:
// the 268 MB stem activation of the pseudo-label forward moved at 2.0 TB/s, the bf16 one of the teacher at 1.1.)
template <int VEC>
__device__ __forceinline__ void bna_params(const float* gamma, const float* beta, const float* mean, const float* var,
                                           float eps, int c, float (&sc)[VEC], float (&sh)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float invstd = 1.0f / sqrtf(var[c + k] + eps);
        sc[k] = (gamma ? gamma[c + k] : 1.0f) * invstd;
        sh[k] = fmaf(-mean[c + k], sc[k], beta ? beta[c + k] : 0.0f);
    }
}

template <bool RELU>
__device__ __forceinline__ float4 bna_apply4(const float4 v, const float (&sc)[4], const float (&sh)[4])
{
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = fmaf(o[k], sc[k], sh[k]);
        o[k] = RELU ? ((t > 0.f || t != t) ? t : 0.f) : t;      // a NaN stays (the rule of hiast_hip.h)
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

template <bool RELU>
__device__ __forceinline__ uint4 bna_apply8(const uint4 v, const float (&sc)[8], const float (&sh)[8])
{
    const unsigned wds[4] = {v.x, v.y, v.z, v.w};
    unsigned pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float o[2] = {__uint_as_float(wds[q] << 16), __uint_as_float(wds[q] & 0xFFFF0000u)};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float t = fmaf(o[k], sc[2 * q + k], sh[2 * q + k]);
            o[k] = RELU ? ((t > 0.f || t != t) ? t : 0.f) : t;      // a NaN stays (the rule of hiast_hip.h)
        }
        pk[q] = (unsigned)__bfloat16_as_ushort(__float2bfloat16(o[0])) |
                ((unsigned)__bfloat16_as_ushort(__float2bfloat16(o[1])) << 16);
    }
    return make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

template <bool RELU>
__global__ __launch_bounds__(256) void bn_act_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ var, float eps,
                                                          long long total4, int C)
{
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float sc[4], sh[4];
    if ((stride * 4) % C == 0) {            // block-uniform: this thread's channels are fixed
        if (i < total4) bna_params<4>(gamma, beta, mean, var, eps, (int)((i * 4) % C), sc, sh);
        for (; i + 3 * stride < total4; i += 4 * stride) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4*>(x)[i + u * stride];
#pragma unroll
            for (int u = 0; u < 4; ++u) reinterpret_cast<float4*>(y)[i + u * stride] = bna_apply4<RELU>(v[u], sc, sh);
        }
        for (; i < total4; i += stride)
            reinterpret_cast<float4*>(y)[i] = bna_apply4<RELU>(reinterpret_cast<const float4*>(x)[i], sc, sh);
        return;
    }
    for (; i < total4; i += stride) {
        bna_params<4>(gamma, beta, mean, var, eps, (int)((i * 4) % C), sc, sh);
        reinterpret_cast<float4*>(y)[i] = bna_apply4<RELU>(reinterpret_cast<const float4*>(x)[i], sc, sh);
    }
}

// bf16 flavour: 8 channels per thread (C % 8 == 0)
template <bool RELU>
__global__ __launch_bounds__(256) void bn_act_nhwc_bf16_kernel(const unsigned short* __restrict__ x,
                                                               unsigned short* __restrict__ y,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ var, float eps,
                                                               long long total8, int C)
{
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float sc[8], sh[8];
    if ((stride * 8) % C == 0) {
        if (i < total8) bna_params<8>(gamma, beta, mean, var, eps, (int)((i * 8) % C), sc, sh);
        for (; i + 3 * stride < total8; i += 4 * stride) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const uint4*>(x)[i + u * stride];
#pragma unroll
            for (int u = 0; u < 4; ++u) reinterpret_cast<uint4*>(y)[i + u * stride] = bna_apply8<RELU>(v[u], sc, sh);
        }
        for (; i < total8; i += stride)
            reinterpret_cast<uint4*>(y)[i] = bna_apply8<RELU>(reinterpret_cast<const uint4*>(x)[i], sc, sh);
        return;
    }
    for (; i < total8; i += stride) {
        bna_params<8>(gamma, beta, mean, var, eps, (int)((i * 8) % C), sc, sh);
        reinterpret_cast<uint4*>(y)[i] = bna_apply8<RELU>(reinterpret_cast<const uint4*>(x)[i], sc, sh);
    }
}

}  // namespace hiast

// Since round 5 the only caller of the register-staged kernel is the plain GEMM below (the fp32-row form of the ASPP tap GEMM,
// hiast_aspp2_fwd): the round-1 C-ABI entries hiast_conv1x1_bn_act_nhwc / hiast_conv3x3_bn_act_nhwc had no product caller left
// (every trunk convolution runs on hiast_igemm_bn_act) and were removed from the ABI; the BN / residual / ReLU / 3x3 variants of
// the kernel template are no longer instantiated.
template <typename TA, typename TO>
static int launch_gemm_t(const void* x, const float* w, void* y, int64_t M, int K, int N, hipStream_t st)
{
    const int BN = (N % 128 == 0) ? 128 : 64;
    dim3 grid((unsigned)((M + hiast::C1_BM - 1) / hiast::C1_BM), N / BN);
    const hiast::ConvGeo geo = {0, 0, 0, 0, 1, 1};
#define L(BNV)                                                                                                     \
    hipLaunchKernelGGL((hiast::conv1x1_bn_act_kernel<TA, TO, BNV, 1, false, false>), grid, dim3(256), 0, st,       \
                       (const TA*)x, w, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,       \
                       (const float*)nullptr, 0.f, (const TO*)nullptr, (TO*)y, (int)M, K, N, geo)
    if (BN == 128) L(128); else L(64);
#undef L
    HIAST_CHECK_LAUNCH();
    return 0;
}

// plain GEMM entry for other translation units (aspp2.hip): Y[M][N] = X[M][K] * W[N][K]^T, no BN / residual / ReLU.
// dtype: 0 = fp32 in (split-bf16 arithmetic) / fp32 out, 1 = bf16 in / bf16 out, 2 = bf16 in / fp32 out.
int hiast_gemm_nt_launch(const void* x, const float* w, void* y, int64_t M, int K, int N, int dtype, hipStream_t st)
{
    if (!x || !w || !y) return HIAST_E_ARG;
    if (M <= 0 || K <= 0 || N <= 0) return HIAST_E_ARG;
    if (K % hiast::C1_BK != 0 || N % 64 != 0 || M > (1ll << 31) - 256 || dtype < 0 || dtype > 2) return HIAST_E_RANGE;
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y)) & 15) return HIAST_E_RANGE;
    if (dtype == 0) return launch_gemm_t<float, float>(x, w, y, M, K, N, st);
    if (dtype == 2) return launch_gemm_t<__hip_bfloat16, float>(x, w, y, M, K, N, st);
    return launch_gemm_t<__hip_bfloat16, __hip_bfloat16>(x, w, y, M, K, N, st);
}

extern "C" int hiast_bn_act_nhwc_infer(const void* x, void* y, const float* gamma, const float* beta,
                                       const float* mean, const float* var, float eps, int relu, int64_t M,
                                       int C, int dtype, hiast_stream_t stream)
{
    if (!x || !y || !mean || !var) return HIAST_E_ARG;
    if (M <= 0 || C <= 0) return HIAST_E_ARG;
    const int vec = dtype ? 8 : 4;
    if ((dtype != 0 && dtype != 1) || C % vec != 0 || ((((uintptr_t)x) | ((uintptr_t)y)) & 15)) return HIAST_E_RANGE;
    const long long totalv = (long long)M * C / vec;
    long long nb = (totalv + 256 * 4 - 1) / (256 * 4);
    int grid = (int)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb));
    // a grid-stride that is a multiple of C keeps a thread's channels fixed (parameters derived once per thread): round the
    // grid down to a multiple of C / gcd(C, 256 * vec) when that leaves at least one block
    {
        long long a = 256LL * vec, g = C;
        while (a) { const long long t = g % a; g = a; a = t; }          // g = gcd(C, 256 * vec)
        const int need = (int)(C / g);
        if (grid >= need) grid -= grid % need;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) {
        if (relu)
            hipLaunchKernelGGL(hiast::bn_act_nhwc_kernel<true>, dim3(grid), dim3(256), 0, st, (const float*)x, (float*)y,
                               gamma, beta, mean, var, eps, totalv, C);
        else
            hipLaunchKernelGGL(hiast::bn_act_nhwc_kernel<false>, dim3(grid), dim3(256), 0, st, (const float*)x, (float*)y,
                               gamma, beta, mean, var, eps, totalv, C);
    } else {
        if (relu)
            hipLaunchKernelGGL(hiast::bn_act_nhwc_bf16_kernel<true>, dim3(grid), dim3(256), 0, st,
                               (const unsigned short*)x, (unsigned short*)y, gamma, beta, mean, var, eps, totalv, C);
        else
            hipLaunchKernelGGL(hiast::bn_act_nhwc_bf16_kernel<false>, dim3(grid), dim3(256), 0, st,
                               (const unsigned short*)x, (unsigned short*)y, gamma, beta, mean, var, eps, totalv, C);
    }
    HIAST_CHECK_LAUNCH();
    return 0;
}
