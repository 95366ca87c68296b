// K19: the warm-up discriminator's convolutions — 4x4 window, stride 2, padding 1, fp32 NCHW (FCDiscriminator,
// sseg/models/modules/discriminator.py:7-33: C -> 64 -> 128 -> 256 -> 512 -> 1, LeakyReLU(0.2) between them).
//
// Three operations, each an implicit GEMM on ONE tile kernel (64 x 64 outputs per block of 256 threads, K walked in steps of 16
// through two LDS buffers, a 4 x 4 register tile per thread, fp32 fmaf accumulation — DESIGN §9 says why not the split-bf16
// MFMA form):
//   forward   M = (b, ho, wo)            N = co                  K = (ci, kh, kw)      epilogue: + bias, LeakyReLU
//   dgrad     M = (b, h2, w2) of a class N = ci                  K = (co, 2 x 2 taps)  one launch plane per output-parity class
//   wgrad     M = co                     N = (ci, kh, kw) | bias K = (b, ho, wo)       split over K, fixed-order second stage
// The operands are never padded in memory: a loader returns 0.0f for a coordinate outside its tensor (the padding ring, the
// tail of a tile, the tail of K) WITHOUT forming the address, so odd H / W, Cin = 19 / 9 / 2 and Cout = 1 need no special case.
// The LeakyReLU backward is the prologue of dgrad and wgrad: g = dy * (y > 0 ? 1 : 0.2) from the saved OUTPUT y (slope > 0:
// sign(y) = sign of the pre-activation; y == 0 takes 0.2, as at::leaky_relu_backward does).
// hiast_disc_conv16_*: the same three operations with the operands rounded to fp16 / bf16 on the matrix cores, a second tile
// kernel (dc_gemm16_kernel, below) over the same loaders and stores.
#include "common.h"

namespace hiast {
namespace {

constexpr int DT = 64;    // tile edge, M and N
constexpr int DK = 16;    // K step
constexpr int DFLUSH = 8;  // K steps per first-level sum
constexpr int DLD = 68;   // LDS row stride in floats: 16-byte aligned rows, and the 16 k x 4 m stores of a wave hit 64 banks

struct DcGeo {
    int B, Cin, Cout, H, W, Ho, Wo;
};

__device__ __forceinline__ float dc_gate(const float* dy, const float* y, long long idx, int leaky)
{
    float g = dy[idx];
    if (leaky) g = y[idx] > 0.0f ? g : 0.2f * g;
    return g;
}

// thread -> the 4 tile elements it fetches per K step.  KFAST: k = tid % 16, row = tid / 16 + 16 i (global addresses run along
// k); otherwise row = tid % 64, k = tid / 64 + 4 i (addresses run along the tile row)
template <bool KFAST>
__device__ __forceinline__ void dc_put(float (*S)[DLD], int tid, const float r[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (KFAST) S[tid & 15][(tid >> 4) + 16 * i] = r[i];
        else S[(tid >> 6) + 4 * i][tid & 63] = r[i];
    }
}

// ------------------------------------------------------------------------------------------------------------ forward
struct FwdOp {
    const float* x; const float* w; const float* bias; float* y;
    DcGeo g;
    int M, K, leaky;
    static constexpr bool A_KFAST = false, B_KFAST = true;
    __device__ int mrows(int) const { return M; }
    __device__ void krange(int, int& kb, int& ke) const { kb = 0; ke = K; }
    struct Ctx {
        const FwdOp& o;
        const float* xb;
        int ih0, iw0, n0, tid;
        bool mv;
        __device__ Ctx(const FwdOp& op, int, int m0, int n0_, int tid_) : o(op), n0(n0_), tid(tid_)
        {
            const int m = m0 + (tid & 63), hw = o.g.Ho * o.g.Wo;
            mv = m < o.M;
            const int b = mv ? m / hw : 0, p = mv ? m % hw : 0;
            ih0 = 2 * (p / o.g.Wo) - 1;
            iw0 = 2 * (p % o.g.Wo) - 1;
            xb = o.x + (long long)b * o.g.Cin * o.g.H * o.g.W;
        }
        __device__ void fetch(int k0, int ke, float ra[4], float rb[4]) const
        {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + (tid >> 6) + 4 * i;
                const int ci = k >> 4, ih = ih0 + ((k >> 2) & 3), iw = iw0 + (k & 3);
                const bool ok = mv && k < ke && ih >= 0 && ih < o.g.H && iw >= 0 && iw < o.g.W;
                ra[i] = ok ? xb[((long long)ci * o.g.H + ih) * o.g.W + iw] : 0.0f;
            }
            const int k = k0 + (tid & 15);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + (tid >> 4) + 16 * i;
                rb[i] = (n < o.g.Cout && k < ke) ? o.w[(long long)n * o.K + k] : 0.0f;
            }
        }
    };
    __device__ void store(int, int m, int n, float v) const
    {
        if (m >= M || n >= g.Cout) return;
        const int hw = g.Ho * g.Wo, b = m / hw, p = m % hw;
        if (bias) v += bias[n];
        if (leaky) v = v > 0.0f ? v : 0.2f * v;
        y[((long long)b * g.Cout + n) * hw + p] = v;
    }
};

// ------------------------------------------------------------------------------------------------------ input gradient
// dx pixel (h, w) = (2 h2 + ph, 2 w2 + pw) receives, from every output channel, the 2 x 2 taps kh = 1 - ph + 2 th, kw = 1 - pw + 2 tw
// of output pixel (h2 + ph - th, w2 + pw - tw): a gather, one launch plane (blockIdx.z) per parity class (ph, pw).
// wt: the weights repacked per class, [4][Cout * 4][Cin] (dc_pack_wt_kernel), so the B tile's rows are contiguous.
struct DgradOp {
    const float* dy; const float* y; const float* wt; float* dx;
    DcGeo g;
    int K, leaky;                                    // K = Cout * 4
    static constexpr bool A_KFAST = false, B_KFAST = false;
    __device__ int hc(int z) const { return (g.H - (z >> 1) + 1) >> 1; }
    __device__ int wc(int z) const { return (g.W - (z & 1) + 1) >> 1; }
    __device__ int mrows(int z) const { return g.B * hc(z) * wc(z); }
    __device__ void krange(int, int& kb, int& ke) const { kb = 0; ke = K; }
    struct Ctx {
        const DgradOp& o;
        int b, hb, wb, n0, tid, z;                  // hb = h2 + ph, wb = w2 + pw
        bool mv;
        __device__ Ctx(const DgradOp& op, int z_, int m0, int n0_, int tid_) : o(op), n0(n0_), tid(tid_), z(z_)
        {
            const int m = m0 + (tid & 63), H2 = o.hc(z), W2 = o.wc(z), hw = H2 * W2;
            mv = m < o.g.B * hw;
            b = mv ? m / hw : 0;
            const int p = mv ? m % hw : 0;
            hb = p / W2 + (z >> 1);
            wb = p % W2 + (z & 1);
        }
        __device__ void fetch(int k0, int ke, float ra[4], float rb[4]) const
        {
            const int n = n0 + (tid & 63);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + (tid >> 6) + 4 * i;
                const int co = k >> 2, ho = hb - ((k >> 1) & 1), wo = wb - (k & 1);
                const bool ok = mv && k < ke && ho >= 0 && ho < o.g.Ho && wo >= 0 && wo < o.g.Wo;
                ra[i] = ok ? dc_gate(o.dy, o.y, (((long long)b * o.g.Cout + co) * o.g.Ho + ho) * o.g.Wo + wo, o.leaky) : 0.0f;
                rb[i] = (n < o.g.Cin && k < ke) ? o.wt[((long long)z * o.K + k) * o.g.Cin + n] : 0.0f;
            }
        }
    };
    __device__ void store(int z, int m, int n, float v) const
    {
        const int H2 = hc(z), W2 = wc(z), hw = H2 * W2;
        if (m >= g.B * hw || n >= g.Cin) return;
        const int b = m / hw, p = m % hw, h = 2 * (p / W2) + (z >> 1), w = 2 * (p % W2) + (z & 1);
        dx[(((long long)b * g.Cin + n) * g.H + h) * g.W + w] = v;
    }
};

__global__ __launch_bounds__(256) void dc_pack_wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cin, int Cout)
{
    const long long total = 16ll * Cin * Cout;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int ci = (int)(t % Cin);
        const long long r = t / Cin;
        const int K = Cout * 4, k = (int)(r % K), z = (int)(r / K);
        const int co = k >> 2, kh = 1 - (z >> 1) + 2 * ((k >> 1) & 1), kw = 1 - (z & 1) + 2 * (k & 1);
        wt[t] = w[(((long long)co * Cin + ci) * 4 + kh) * 4 + kw];
    }
}

// ------------------------------------------------------------------------------------------- weight and bias gradient
// N has one column more than the weights of an output channel: the "input" of the bias is 1 at every output pixel, so its
// gradient is column Cin * 16 of the same product.  blockIdx.z = a range of kper output pixels; partial sums go to
// P[z][n][co]; dc_wgrad_reduce_kernel adds the ranges in ascending z (fixed order: two runs give the same bits).
struct WgradOp {
    const float* x; const float* dy; const float* y; float* P;
    DcGeo g;
    int N, K, kper, leaky;                           // N = Cin * 16 + 1, K = B * Ho * Wo
    static constexpr bool A_KFAST = true, B_KFAST = true;
    __device__ int mrows(int) const { return g.Cout; }
    __device__ void krange(int z, int& kb, int& ke) const
    {
        kb = z * kper;
        ke = kb + kper < K ? kb + kper : K;
    }
    struct Ctx {
        const WgradOp& o;
        int m0, tid;
        int ci[4], kh[4], kw[4];                     // of this thread's 4 columns; ci = -1: the bias column, -2: past N
        __device__ Ctx(const WgradOp& op, int, int m0_, int n0, int tid_) : o(op), m0(m0_), tid(tid_)
        {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + (tid >> 4) + 16 * i;
                ci[i] = n < o.N - 1 ? n >> 4 : (n == o.N - 1 ? -1 : -2);
                kh[i] = (n >> 2) & 3;
                kw[i] = n & 3;
            }
        }
        __device__ void fetch(int k0, int ke, float ra[4], float rb[4]) const
        {
            const int k = k0 + (tid & 15), hw = o.g.Ho * o.g.Wo;
            const bool kv = k < ke;
            const int b = kv ? k / hw : 0, p = kv ? k % hw : 0;
            const int ih0 = 2 * (p / o.g.Wo) - 1, iw0 = 2 * (p % o.g.Wo) - 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = m0 + (tid >> 4) + 16 * i;
                ra[i] = (kv && co < o.g.Cout) ? dc_gate(o.dy, o.y, ((long long)b * o.g.Cout + co) * hw + p, o.leaky) : 0.0f;
                const int ih = ih0 + kh[i], iw = iw0 + kw[i];
                float v = 0.0f;
                if (kv && ci[i] >= 0 && ih >= 0 && ih < o.g.H && iw >= 0 && iw < o.g.W)
                    v = o.x[(((long long)b * o.g.Cin + ci[i]) * o.g.H + ih) * o.g.W + iw];
                if (kv && ci[i] == -1) v = 1.0f;
                rb[i] = v;
            }
        }
    };
    __device__ void store(int z, int m, int n, float v) const
    {
        if (m >= g.Cout || n >= N) return;
        P[((long long)z * N + n) * g.Cout + m] = v;
    }
};

__global__ __launch_bounds__(256) void dc_wgrad_reduce_kernel(const float* __restrict__ P, float* __restrict__ dw,
                                                              float* __restrict__ db, int N, int Cout, int nsplit)
{
    const long long total = (long long)N * Cout;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    float s = 0.0f;
    for (int z = 0; z < nsplit; ++z) s += P[(long long)z * total + t];
    const int n = (int)(t / Cout), co = (int)(t % Cout);
    if (n < N - 1) dw[(long long)co * (N - 1) + n] = s;
    else if (db) db[co] = s;
}

// --------------------------------------------------------------------------------------------------- the tile kernel
template <class Op>
__global__ __launch_bounds__(256) void dc_gemm_kernel(const Op op)
{
    __shared__ __attribute__((aligned(16))) float As[2][DK][DLD];
    __shared__ __attribute__((aligned(16))) float Bs[2][DK][DLD];
    const int tid = (int)threadIdx.x, z = (int)blockIdx.z;
    const int m0 = (int)blockIdx.x * DT, n0 = (int)blockIdx.y * DT;
    if (m0 >= op.mrows(z)) return;                   // a smaller parity class of dgrad: block-uniform
    int kb, ke;
    op.krange(z, kb, ke);
    const typename Op::Ctx ctx(op, z, m0, n0, tid);
    const int tx = tid & 15, ty = tid >> 4;          // rows m0 + 4 tx .. + 3 (lanes run along M), columns n0 + 4 ty .. + 3
    // two-level sum: acc takes DFLUSH steps (128 terms) and is then added into tot — over the 8192 terms of the classifier a
    // single fmaf chain's rounding error grows like n, this like sqrt(n) twice
    float acc[4][4], tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = 0.0f;
    int step = 0;
    float ra[4], rb[4];
    if (kb < ke) ctx.fetch(kb, ke, ra, rb);
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += DK) {
        dc_put<Op::A_KFAST>(As[buf], tid, ra);
        dc_put<Op::B_KFAST>(Bs[buf], tid, rb);
        __syncthreads();                             // one barrier per step: the buffer written two steps on was read before the
        if (k0 + DK < ke) ctx.fetch(k0 + DK, ke, ra, rb);   // barrier of the step in between
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
            const float4 a = *reinterpret_cast<const float4*>(&As[buf][kk][tx * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&Bs[buf][kk][ty * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        buf ^= 1;
        if (++step == DFLUSH) {
            step = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    tot[i][j] += acc[i][j];
                    acc[i][j] = 0.0f;
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) op.store(z, m0 + tx * 4 + i, n0 + ty * 4 + j, tot[i][j] + acc[i][j]);
}

// ------------------------------------------------------------------------------- the 16-bit matrix-core tile kernel
// The same three Ops, the same 64 x 64 block on 256 threads, the same two LDS buffers and one barrier per step; the arithmetic
// is v_mfma_f32_16x16x32_{f16,bf16}: every fetched fp32 value (in the backward: the fp32 gate product) is rounded to the 16-bit
// type (nearest even; an fp16 overflow becomes inf) when it goes to LDS, products are summed in fp32.  K advances 32 per step
// = two fetches (k0, k0 + 16); a range whose length is an odd multiple of 16 ends in a half step of zeros.
//
// LDS: [row][32 positions] of 16-bit values, a row = 64 B of data in DLD16 * 2 = 96 B.  The sum over k does not care about
// the order of k as long as both operands agree, so k = 16 kh + kl (kh = which fetch) sits at position
//     p(k) = 8 (kl & 3) + 4 kh + (kl >> 2)
// for both tiles.  A non-KFAST thread (row = tid % 64, kl = tid / 64 + 4 i) then owns the eight positions 8 (tid / 64) .. + 7
// of its row: one 16-byte store instead of eight 2-byte ones.  A KFAST thread (kl = tid % 16, rows tid / 16 + 16 i) stores 2
// bytes at p and p + 4.  Lane l of a wave reads positions 8 (l >> 4) .. + 7 of row (l & 15) as one 16-byte fragment.
// Banks with rows 24 dwords apart:
//   fragment read (ds_read_b128, 16-lane groups {0-3, 12-15, 20-27}, ...; 16-byte slot = 6 row + (l >> 4) mod 16): the
//       rows 0-3, 12-15 of one quarter give the even slots 0 6 12 2 | 8 14 4 10, rows 4-11 of the next quarter the odd
//       slots 9 15 5 11 1 7 13 3 (the other groups likewise): conflict-free;
//   16-byte store (8-lane groups, 32 banks): rows r .. r + 7 at 24 r mod 32 = 0 24 16 8 0 ...: 2-way;
//   2-byte store (32-lane halves: rows r, r + 1, kl = 0 .. 15 at dwords 4 (kl & 3) + (kl >> 3) = 0 1 4 5 8 9 12 13, two
//       lanes per dword): row r + 1 at + 24 meets row r in 4 of the 8 dwords: 2-way.
// (64-byte rows would put a group's fragments on 4 slots: 4-way; 80-byte rows make the 16-byte store conflict-free and the
// fragment read 2-way — the reads are the larger number.)
//
// Orientation: in all three Ops M is the index that is contiguous (or stride 2) in memory, so the M tile is the MFMA's B
// operand and the N tile its A operand: D[n][m] has m = lane & 15 on the lanes and n = 4 (lane >> 4) + reg in the registers,
// and the 16 lanes of a group store 16 neighbouring m.  Wave w owns the quadrant m 32 (w & 1) .. + 31, n 32 (w >> 1) .. + 31
// as 2 x 2 MFMA tiles.  Every 4 steps (128 terms, as DFLUSH x DK above) the accumulators are added into a second level.
constexpr int DK16 = 2 * DK;      // K step of the 16-bit kernel
constexpr int DFLUSH16 = DFLUSH / 2;
constexpr int DLD16 = 48;         // LDS row stride in 16-bit values (96 B)

template <bool F16, bool KFAST>
__device__ __forceinline__ void dc_put16(unsigned short (*S)[DLD16], int tid, const float r0[4], const float r1[4])
{
    typedef H16<F16> HT;
    if (KFAST) {
        const int kl = tid & 15, p = 8 * (kl & 3) + (kl >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            S[(tid >> 4) + 16 * i][p] = HT::enc(r0[i]);
            S[(tid >> 4) + 16 * i][p + 4] = HT::enc(r1[i]);
        }
    } else {
        *reinterpret_cast<uint4*>(&S[tid & 63][8 * (tid >> 6)]) =
            make_uint4(HT::pack(r0[0], r0[1]), HT::pack(r0[2], r0[3]), HT::pack(r1[0], r1[1]), HT::pack(r1[2], r1[3]));
    }
}

template <class Op, bool F16>
__global__ __launch_bounds__(256) void dc_gemm16_kernel(const Op op)
{
    typedef H16<F16> HT;
    __shared__ __attribute__((aligned(16))) unsigned short Ms[2][DT][DLD16];
    __shared__ __attribute__((aligned(16))) unsigned short Ns[2][DT][DLD16];
    const int tid = (int)threadIdx.x, z = (int)blockIdx.z;
    const int m0 = (int)blockIdx.x * DT, n0 = (int)blockIdx.y * DT;
    if (m0 >= op.mrows(z)) return;                   // block-uniform, as above
    int kb, ke;
    op.krange(z, kb, ke);
    const typename Op::Ctx ctx(op, z, m0, n0, tid);
    const int lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wm = ((tid >> 6) & 1) * 32, wn = (tid >> 7) * 32;
    h_f32x4 acc[2][2], tot[2][2];                    // [n tile][m tile]
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[u][t] = tot[u][t] = (h_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    int step = 0;
    float ra[2][4], rb[2][4];
    if (kb < ke) {
        ctx.fetch(kb, ke, ra[0], rb[0]);
        ctx.fetch(kb + DK, ke, ra[1], rb[1]);        // past ke: zeros, no address formed
    }
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += DK16) {
        dc_put16<F16, Op::A_KFAST>(Ms[buf], tid, ra[0], ra[1]);
        dc_put16<F16, Op::B_KFAST>(Ns[buf], tid, rb[0], rb[1]);
        __syncthreads();                             // one barrier per step, as in dc_gemm_kernel
        if (k0 + DK16 < ke) {
            ctx.fetch(k0 + DK16, ke, ra[0], rb[0]);
            ctx.fetch(k0 + DK16 + DK, ke, ra[1], rb[1]);
        }
        uint4 fm[2], fn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            fm[t] = *reinterpret_cast<const uint4*>(&Ms[buf][wm + 16 * t + fr][8 * fq]);
            fn[t] = *reinterpret_cast<const uint4*>(&Ns[buf][wn + 16 * t + fr][8 * fq]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[u][t] = HT::mfma16(fn[u], fm[t], acc[u][t]);
        buf ^= 1;
        if (++step == DFLUSH16) {
            step = 0;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    tot[u][t] += acc[u][t];
                    acc[u][t] = (h_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const h_f32x4 v = tot[u][t] + acc[u][t];
#pragma unroll
            for (int r = 0; r < 4; ++r) op.store(z, m0 + wm + 16 * t + fr, n0 + wn + 16 * u + 4 * fq + r, v[r]);
        }
}

// fmt = 0: the fp32 kernel; HIAST_FMT_FP16 / HIAST_FMT_BF16: the matrix-core kernel in that operand type
template <class Op>
void dc_launch(int fmt, dim3 grid, hipStream_t st, const Op& op)
{
    if (fmt == HIAST_FMT_FP16) hipLaunchKernelGGL((dc_gemm16_kernel<Op, true>), grid, dim3(256), 0, st, op);
    else if (fmt == HIAST_FMT_BF16) hipLaunchKernelGGL((dc_gemm16_kernel<Op, false>), grid, dim3(256), 0, st, op);
    else hipLaunchKernelGGL(dc_gemm_kernel<Op>, grid, dim3(256), 0, st, op);
}

inline bool dc_fmt16_ok(int fmt) { return fmt == HIAST_FMT_FP16 || fmt == HIAST_FMT_BF16; }

// ----------------------------------------------------------------------------------------------------------- host side
struct DcPlan {
    int ok;
    DcGeo g;
    int smax;            // upper bound of the wgrad split (sizes the workspace; monotone in B * Ho * Wo)
    int nsplit, kper;    // the split the launch uses (nsplit <= smax)
    size_t bytes;
};

DcPlan dc_plan(int B, int Cin, int Cout, int H, int W)
{
    DcPlan p = {};
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H < 2 || W < 2) return p;
    if (Cin > 4096 || Cout > 4096) return p;
    const int Ho = (H + 2 - 4) / 2 + 1, Wo = (W + 2 - 4) / 2 + 1;
    const long long lim = 1ll << 31;
    if ((long long)B * Cin * H * W >= lim || (long long)B * Cout * Ho * Wo >= lim || (long long)B * H * W >= lim - DT) return p;
    p.g = {B, Cin, Cout, H, W, Ho, Wo};
    const long long K = (long long)B * Ho * Wo, N = (long long)Cin * 16 + 1;
    const long long tiles = ((Cout + DT - 1) / DT) * ((N + DT - 1) / DT);
    long long s = 1024 / tiles;                      // about four blocks per CU; a constant: the summation order (hence the
    s = s < 1 ? 1 : s;                               // bits of dw) does not depend on the device
    const long long cap = (K + 255) / 256;           // at least 16 K steps per range
    s = s > cap ? cap : s;
    p.smax = (int)s;
    long long kper = (K + s - 1) / s;
    kper = (kper + DK - 1) / DK * DK;
    p.kper = (int)kper;
    p.nsplit = (int)((K + kper - 1) / kper);
    const size_t wg = (size_t)p.smax * (size_t)N * Cout * 4, dg = (size_t)16 * Cin * Cout * 4;
    p.bytes = ((wg > dg ? wg : dg) + 255) / 256 * 256;
    p.ok = 1;
    return p;
}

}  // namespace
}  // namespace hiast

using namespace hiast;

extern "C" size_t hiast_disc_conv_workspace_bytes(int B, int Cin, int Cout, int H, int W)
{
    const DcPlan p = dc_plan(B, Cin, Cout, H, W);
    return p.ok ? p.bytes : 0;
}

// the three operations; fmt = 0 (fp32) or a checked 16-bit format
static int dc_fwd(int fmt, const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                  int leaky, hiast_stream_t stream)
{
    if (!x || !w || !y) return HIAST_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    const DcPlan p = dc_plan(B, Cin, Cout, H, W);
    if (!p.ok) return HIAST_E_RANGE;
    FwdOp op;
    op.x = x; op.w = w; op.bias = bias; op.y = y;
    op.g = p.g;
    op.M = B * p.g.Ho * p.g.Wo;
    op.K = Cin * 16;
    op.leaky = leaky != 0;
    const dim3 grid((unsigned)((op.M + DT - 1) / DT), (unsigned)((Cout + DT - 1) / DT), 1);
    dc_launch(fmt, grid, (hipStream_t)stream, op);
    HIAST_CHECK_LAUNCH();
    return 0;
}

static int dc_dgrad(int fmt, const float* dy, const float* y, const float* w, float* dx, int B, int Cin, int Cout, int H, int W,
                    int leaky, void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    if (!dy || !w || !dx || !workspace || (leaky && !y)) return HIAST_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    const DcPlan p = dc_plan(B, Cin, Cout, H, W);
    if (!p.ok) return HIAST_E_RANGE;
    if (workspace_bytes < p.bytes) return HIAST_E_WS;
    if ((uintptr_t)workspace & 3) return HIAST_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    float* wt = (float*)workspace;
    const long long total = 16ll * Cin * Cout;
    const long long pb = (total + 255) / 256;
    hipLaunchKernelGGL(dc_pack_wt_kernel, dim3((unsigned)(pb > 4096 ? 4096 : pb)), dim3(256), 0, st, w, wt, Cin, Cout);
    HIAST_CHECK_LAUNCH();
    DgradOp op;
    op.dy = dy; op.y = y; op.wt = wt; op.dx = dx;
    op.g = p.g;
    op.K = Cout * 4;
    op.leaky = leaky != 0;
    const int Mc = B * ((H + 1) / 2) * ((W + 1) / 2);        // the largest class (ph = pw = 0)
    const dim3 grid((unsigned)((Mc + DT - 1) / DT), (unsigned)((Cin + DT - 1) / DT), 4);
    dc_launch(fmt, grid, st, op);
    HIAST_CHECK_LAUNCH();
    return 0;
}

static int dc_wgrad(int fmt, const float* x, const float* dy, const float* y, float* dw, float* db, int B, int Cin, int Cout,
                    int H, int W, int leaky, void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    if (!x || !dy || !dw || !workspace || (leaky && !y)) return HIAST_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    const DcPlan p = dc_plan(B, Cin, Cout, H, W);
    if (!p.ok) return HIAST_E_RANGE;
    if (workspace_bytes < p.bytes) return HIAST_E_WS;
    if ((uintptr_t)workspace & 3) return HIAST_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    WgradOp op;
    op.x = x; op.dy = dy; op.y = y; op.P = (float*)workspace;
    op.g = p.g;
    op.N = Cin * 16 + 1;
    op.K = B * p.g.Ho * p.g.Wo;
    op.kper = p.kper;
    op.leaky = leaky != 0;
    const dim3 grid((unsigned)((Cout + DT - 1) / DT), (unsigned)((op.N + DT - 1) / DT), (unsigned)p.nsplit);
    dc_launch(fmt, grid, st, op);
    HIAST_CHECK_LAUNCH();
    const long long total = (long long)op.N * Cout;
    hipLaunchKernelGGL(dc_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const float*)workspace, dw, db, op.N, Cout, p.nsplit);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_disc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout,
                                   int H, int W, int leaky, hiast_stream_t stream)
{
    return dc_fwd(0, x, w, bias, y, B, Cin, Cout, H, W, leaky, stream);
}

extern "C" int hiast_disc_conv_dgrad(const float* dy, const float* y, const float* w, float* dx, int B, int Cin, int Cout,
                                     int H, int W, int leaky, void* workspace, size_t workspace_bytes, hiast_stream_t stream)
{
    return dc_dgrad(0, dy, y, w, dx, B, Cin, Cout, H, W, leaky, workspace, workspace_bytes, stream);
}

extern "C" int hiast_disc_conv_wgrad(const float* x, const float* dy, const float* y, float* dw, float* db, int B, int Cin,
                                     int Cout, int H, int W, int leaky, void* workspace, size_t workspace_bytes,
                                     hiast_stream_t stream)
{
    return dc_wgrad(0, x, dy, y, dw, db, B, Cin, Cout, H, W, leaky, workspace, workspace_bytes, stream);
}

extern "C" int hiast_disc_conv16_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout,
                                     int H, int W, int leaky, int fmt, hiast_stream_t stream)
{
    if (!dc_fmt16_ok(fmt)) return HIAST_E_ARG;
    return dc_fwd(fmt, x, w, bias, y, B, Cin, Cout, H, W, leaky, stream);
}

extern "C" int hiast_disc_conv16_dgrad(const float* dy, const float* y, const float* w, float* dx, int B, int Cin, int Cout,
                                       int H, int W, int leaky, int fmt, void* workspace, size_t workspace_bytes,
                                       hiast_stream_t stream)
{
    if (!dc_fmt16_ok(fmt)) return HIAST_E_ARG;
    return dc_dgrad(fmt, dy, y, w, dx, B, Cin, Cout, H, W, leaky, workspace, workspace_bytes, stream);
}

extern "C" int hiast_disc_conv16_wgrad(const float* x, const float* dy, const float* y, float* dw, float* db, int B, int Cin,
                                       int Cout, int H, int W, int leaky, int fmt, void* workspace, size_t workspace_bytes,
                                       hiast_stream_t stream)
{
    if (!dc_fmt16_ok(fmt)) return HIAST_E_ARG;
    return dc_wgrad(fmt, x, dy, y, dw, db, B, Cin, Cout, H, W, leaky, workspace, workspace_bytes, stream);
}
