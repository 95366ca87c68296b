// What is left of K9a, the round-1 fused 1x1 convolution of the trunk (every trunk convolution runs on hiast_igemm_bn_act
// now): the plain fp32 GEMM behind the fp32-row form of the ASPP tap GEMM (hiast_aspp2_fwd, aspp2.hip), and the NHWC
// BatchNorm(eval) (+ReLU) pass hiast_bn_act_nhwc_infer.
//
//   Y[m][n] = Σ_k X[m][k] * W[n][k]
//   X: [M = B*h*w pixels][K = Cin]  fp32, NHWC (channels-last) activation rows
//   W: [N][K]                       fp32 (the tap weights, N = 9 taps x padded classes: a multiple of 128)
//
// Arithmetic: "split-bf16": every fp32 operand is split on the fly into hi = bf16(v) and
// lo = bf16(v - hi); the product is accumulated in fp32 as hi*hi + hi*lo + lo*hi on
// v_mfma_f32_32x32x16_bf16 (the dropped lo*lo term is 2^-16 relative).  Measured |err| vs fp64 is
// ~5e-6 of max|Y| (fp32 MFMA: ~2e-6; plain bf16: 2e-3), well inside the 1e-3 logits contract, at
// 3/16 of the fp32-MFMA cost: gfx950 has no TF32/xf32 path, this is the fast exact-class option.
//
// Structure: 128 x 128 block tile, BK = 32, 4 waves as 2 x 2 (wave tile 64 x 64), register-staged global loads
// (fp32 -> hi/lo happens between the load and the LDS write), LDS double buffered with one barrier per k-step,
// 64-byte rows whose 16-byte chunks are XOR-swizzled so fragment reads and staging stores are conflict free.
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

constexpr int C1_BN = 128;
constexpr int C1_TN = C1_BN / 64;                                    // 32-wide column tiles per wave
constexpr int C1_A_F4 = C1_BM * C1_BK / 4 / 256;                     // 16-byte loads per thread and k-step: 4
constexpr int C1_B_F4 = C1_BN * C1_BK / 4 / 256;                     // 4
// [buf][A_hi | A_lo | B_hi | B_lo]
constexpr int C1_A_BYTES = C1_BM * C1_PITCH * 2, C1_B_BYTES = C1_BN * C1_PITCH * 2;
constexpr int C1_BUF_BYTES = 2 * (C1_A_BYTES + C1_B_BYTES);
constexpr int C1_A_LO = C1_A_BYTES, C1_B_HI = 2 * C1_A_BYTES, C1_B_LO = C1_B_HI + C1_B_BYTES;
constexpr int C1_CP = C1_BN + 4;                                     // floats per row of the epilogue tile
constexpr int C1_EPI_BYTES = C1_BM * C1_CP * 4;
constexpr int C1_SMEM_BYTES = 2 * C1_BUF_BYTES > C1_EPI_BYTES ? 2 * C1_BUF_BYTES : C1_EPI_BYTES;

__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                          float* __restrict__ Y, int M, int K, int N)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[C1_SMEM_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware tile order: work items are numbered with the column tile fastest, and XCD k (workgroup ids
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
    const int m0 = bm * C1_BM, n0 = bn_ * C1_BN;
    const int nk = K / C1_BK;

    f32x16 acc[2][C1_TN];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < C1_TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // global -> register staging: float4 index f = tid + 256*i; row = f / 8, c4 = f % 8.  A thread's rows are
    // the same for every k-step.
    float4 ra[C1_A_F4], rb[C1_B_F4];
    int rm[C1_A_F4];
#pragma unroll
    for (int i = 0; i < C1_A_F4; ++i) {
        const int m = m0 + ((tid + 256 * i) >> 3);
        rm[i] = m < M ? m : M - 1;                                   // tail rows: valid address, never stored
    }
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < C1_A_F4; ++i) {
            const int c4 = (tid + 256 * i) & 7;
            ra[i] = *reinterpret_cast<const float4*>(X + (size_t)rm[i] * K + kt * C1_BK + c4 * 4);
        }
#pragma unroll
        for (int i = 0; i < C1_B_F4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
            rb[i] = *reinterpret_cast<const float4*>(W + (size_t)(n0 + row) * K + kt * C1_BK + c4 * 4);
        }
    };
    auto lds_store = [&](int buf) {
        unsigned char* base = smem + buf * C1_BUF_BYTES;
#pragma unroll
        for (int i = 0; i < C1_A_F4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
            uint2 hi, lo;
            split4(ra[i], hi, lo);
            *reinterpret_cast<uint2*>(base + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = hi;
            *reinterpret_cast<uint2*>(base + C1_A_LO + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = lo;
        }
#pragma unroll
        for (int i = 0; i < C1_B_F4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
            uint2 hi, lo;
            split4(rb[i], hi, lo);
            *reinterpret_cast<uint2*>(base + C1_B_HI + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = hi;
            *reinterpret_cast<uint2*>(base + C1_B_LO + lds_off(row, c4 >> 1) + (c4 & 1) * 8) = lo;
        }
    };

    gload(0);
    lds_store(0);
    __syncthreads();

    const int frow = lane & 31, fchunk = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const unsigned char* base = smem + buf * C1_BUF_BYTES;
#pragma unroll
        for (int kk = 0; kk < C1_BK / 16; ++kk) {
            bf16x8 ah[2], al[2], bh[C1_TN], bl[C1_TN];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int off = lds_off(wm * 64 + a * 32 + frow, kk * 2 + fchunk);
                ah[a] = *reinterpret_cast<const bf16x8*>(base + off);
                al[a] = *reinterpret_cast<const bf16x8*>(base + C1_A_LO + off);
            }
#pragma unroll
            for (int b = 0; b < C1_TN; ++b) {
                const int off = lds_off(wn * (C1_BN / 2) + b * 32 + frow, kk * 2 + fchunk);
                bh[b] = *reinterpret_cast<const bf16x8*>(base + C1_B_HI + off);
                bl[b] = *reinterpret_cast<const bf16x8*>(base + C1_B_LO + off);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < C1_TN; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
                }
        }
        if (kt + 1 < nk) lds_store(buf ^ 1);
        __syncthreads();
    }

    // epilogue through LDS (the staging buffers are free now): accumulators -> fp32 tile [128][128 + 4], then
    // every thread moves float4s along the column axis, so the output write is whole 512-byte row segments
    // (16 B per lane) instead of 4-byte accesses.
    float* sC = reinterpret_cast<float*>(smem);
    __syncthreads();          // (the last k-step's barrier already passed; keeps the reuse of smem explicit)
#pragma unroll
    for (int b = 0; b < C1_TN; ++b) {
        const int nl = wn * (C1_BN / 2) + b * 32 + (lane & 31);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                // + 0.0f, not the bare accumulator: a -0 sum is stored as +0, as the kernel always has (it was
                // fmaf(acc, scale 1, shift 0) when it still carried a BatchNorm)
                sC[ml * C1_CP + nl] = fmaf(acc[a][b][r], 1.0f, 0.0f);
            }
    }
    __syncthreads();
    constexpr int F4_PER_ROW = C1_BN / 4;
#pragma unroll 4
    for (int f = tid; f < C1_BM * F4_PER_ROW; f += 256) {
        const int ml = f / F4_PER_ROW, c4 = f - ml * F4_PER_ROW;
        const int m = m0 + ml;
        if (m >= M) continue;
        const float4 o = *reinterpret_cast<const float4*>(sC + ml * C1_CP + c4 * 4);
        *reinterpret_cast<float4*>(Y + (size_t)m * N + n0 + c4 * 4) = o;
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

// The fp32-row form of the ASPP tap GEMM (hiast_aspp2_fwd, aspp2.hip: its only caller): Y[M][N] = X[M][K] * W[N][K]^T on fp32
// rows and fp32 weights, split-bf16 arithmetic, fp32 out.  N is the padded tap width (aspp2_np), a multiple of 128.
int hiast_gemm_nt_launch(const float* x, const float* w, float* y, int64_t M, int K, int N, hipStream_t st)
{
    if (!x || !w || !y) return HIAST_E_ARG;
    if (M <= 0 || K <= 0 || N <= 0) return HIAST_E_ARG;
    if (K % hiast::C1_BK != 0 || N % hiast::C1_BN != 0 || M > (1ll << 31) - 256) return HIAST_E_RANGE;
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y)) & 15) return HIAST_E_RANGE;
    const dim3 grid((unsigned)((M + hiast::C1_BM - 1) / hiast::C1_BM), N / hiast::C1_BN);
    hipLaunchKernelGGL(hiast::gemm_nt_f32_kernel, grid, dim3(256), 0, st, x, w, y, (int)M, K, N);
    HIAST_CHECK_LAUNCH();
    return 0;
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
