// K15c — level 3 of the device-side sample path (cfg.dataset.device_aug_level: 3): FDA (Fourier domain adaptation) as a
// plan op, in its sparse-DFT form.  augmentations.fourier_domain_adaptation replaces the amplitudes of the centre
// (2 border + 1)^2 bins of the view's spectrum by the target's and transforms back; the FFT is linear and every other bin
// is untouched, so the output is the view plus the real part of the inverse DFT of those few modified bins.  The datasets
// build the transform with beta_limit = 0.001: border = floor(min(H, W) * beta) is 0 or 1 there, 0..2 here.
// device_aug.fda_u8 is the float64 numpy restatement these kernels are tested against (equal bytes except where the
// pre-truncation value is within 1e-6 of an integer: the order of the float64 sums differs).
//
// With e(y) = (1, cos ty, sin ty, cos 2ty, sin 2ty), ty = 2 pi y / H, and r(x) likewise over W (the first 1 + 2 border
// entries of each), every bin sum is a signed pair of entries of the real matrix
//     G[i][j] = sum_y e_i(y) * (sum_x v[y][x] * r_j(x))                    (per channel; launch 1, separable)
// and the correction is sum_ij C[i][j] e_i(y) r_j(x) with C built from the modified bins (launch 2); launch 3 folds
// C with e(y) once per row and applies 1 + 2 border products per byte.  cos / sin come from a host-built float64 table
// (trig = cos[H], sin[H], cos[W], sin[W] of 2 pi j / n), the angle reduced by integer mod first.
// Everything is float64 in a fixed order: no floating-point atomics, the same call returns the same bytes.
// A sample whose segment is not closed by an FDA op (seg[b][3], K15b) is skipped by all three launches.
#include "aug_common.h"

namespace hiast {

constexpr int FDA_NC = 1 + 2 * HIAST_AUG_FDA_MAX_BORDER;      // entries of e(y) / r(x)
constexpr int FDA_NG = 3 * FDA_NC * FDA_NC;                   // doubles of one G / C record: [3][NC][NC]
constexpr int FDA_ROWS = 32;                                  // rows of one launch-1 block
constexpr long long FDA_OFF_MASK = (1ll << HIAST_AUG_FDA_BORDER_SHIFT) - 1;

// the FDA op that closes this sample's segment: its border (-1: none) and the blob offset of its target view
__device__ __forceinline__ int fda_of(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg, int b, long long& off)
{
    const int64_t* o = ops + (size_t)b * OPS;
    const Seg s = seg_of(o, seg + b * 4);
    if (!s.live || s.blur < 0 || op_type(o, s.blur) != HIAST_AUG_OP_FDA) return -1;
    const long long par = op_par(o, s.blur);
    const long long border = par >> HIAST_AUG_FDA_BORDER_SHIFT;
    if (par < 0 || border > HIAST_AUG_FDA_MAX_BORDER) return -1;
    off = par & FDA_OFF_MASK;
    return (int)border;
}

// 4 pixels (12 bytes) of an HWC row from pixel x0: whole words where the row allows it; pixels >= n read as 0
__device__ __forceinline__ void load4(const uint8_t* __restrict__ row, bool words, int x0, int n, unsigned (&v)[12])
{
    if (words && n == 4) {
        unpack12(reinterpret_cast<const uint32_t*>(row + (size_t)x0 * 3), v);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = i < 3 * n ? row[(size_t)x0 * 3 + i] : 0u;
    }
}

// r(x) of the first 1 + 2 NB entries
template <int NB>
__device__ __forceinline__ void basis(const double* __restrict__ cs, const double* __restrict__ sn, int x, int n,
                                      double (&r)[1 + 2 * NB])
{
    r[0] = 1.0;
    int a = 0;
#pragma unroll
    for (int k = 1; k <= NB; ++k) {
        a += x;                                               // (k x) mod n, x < n
        a = a >= n ? a - n : a;
        r[2 * k - 1] = cs[a];
        r[2 * k] = sn[a];
    }
}

template <int NB>
__device__ __forceinline__ void fda_sum_band(const uint8_t* __restrict__ src, const double* __restrict__ trig, int H, int W,
                                             int y0, double* __restrict__ out, double (*s_red)[FDA_NG])
{
    constexpr int NC = 1 + 2 * NB;
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
    const double *cy = trig, *sy = trig + H, *cx = trig + 2 * (size_t)H, *sx = cx + W;
    double acc[3][NC][NC];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[c][i][j] = 0.0;
    const int y1 = min(y0 + FDA_ROWS, H);
    for (int y = y0 + wave; y < y1; y += 4) {
        const uint8_t* row = src + (size_t)y * W * 3;
        const bool words = (reinterpret_cast<uintptr_t>(row) & 3) == 0;
        double col[3][NC];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < NC; ++j) col[c][j] = 0.0;
        for (int x0 = lane * 4; x0 < W; x0 += 256) {
            unsigned v[12];
            load4(row, words, x0, min(4, W - x0), v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double r[NC];
                basis<NB>(cx, sx, min(x0 + i, W - 1), W, r);  // (a pixel past the row holds 0s: any in-range angle)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double d = (double)v[3 * i + c];
#pragma unroll
                    for (int j = 0; j < NC; ++j) col[c][j] = col[c][j] + d * r[j];
                }
            }
        }
        double e[NC];
        basis<NB>(cy, sy, y, H, e);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < NC; ++i)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[c][i][j] = acc[c][i][j] + e[i] * col[c][j];
    }
    // in the wave (fixed butterfly), then the four waves through LDS in their order
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double s = wave_sum_f64(acc[c][i][j]);
                if (lane == 0) s_red[wave][(c * FDA_NC + i) * FDA_NC + j] = s;
            }
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * NC * NC; t += 256) {
        const int c = t / (NC * NC), i = (t / NC) % NC, j = t % NC;
        const int q = (c * FDA_NC + i) * FDA_NC + j;
        double s = s_red[0][q];
        s = s + s_red[1][q];
        s = s + s_red[2][q];
        s = s + s_red[3][q];
        out[q] = s;
    }
}

// launch 1: block (band, image 0 view | 1 target, sample) -> ws partial [B][2][bands][3][NC][NC]
__global__ __launch_bounds__(256) void aug3_fda_sums_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                            const uint8_t* __restrict__ blob, const double* __restrict__ trig,
                                                            const uint8_t* __restrict__ img, double* __restrict__ ws, int H, int W)
{
    __shared__ double s_red[4][FDA_NG];
    const int b = blockIdx.z, which = blockIdx.y, band = blockIdx.x;
    long long off = 0;
    const int border = fda_of(ops, seg, b, off);
    if (border < 0) return;
    const uint8_t* src = which ? blob + off : img + (size_t)b * H * W * 3;
    double* out = ws + (((size_t)b * 2 + which) * gridDim.x + band) * FDA_NG;
    if (border == 0) fda_sum_band<0>(src, trig, H, W, band * FDA_ROWS, out, s_red);
    else if (border == 1) fda_sum_band<1>(src, trig, H, W, band * FDA_ROWS, out, s_red);
    else fda_sum_band<2>(src, trig, H, W, band * FDA_ROWS, out, s_red);
}

// launch 2: block = sample: the partials in band order, then per channel the modified bins D / (H W) as the
// coefficient matrix C of the correction -> coef [B][3][NC][NC]
__global__ __launch_bounds__(64) void aug3_fda_coef_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                           const double* __restrict__ part, double* __restrict__ coef,
                                                           int bands, int H, int W)
{
    __shared__ double s_g[2][FDA_NG];
    __shared__ double s_cf[3][FDA_NC * FDA_NC];
    const int b = blockIdx.x;
    long long off = 0;
    const int nb = fda_of(ops, seg, b, off);
    if (nb < 0) return;
    const int nc = 1 + 2 * nb;
    for (int t = threadIdx.x; t < 2 * 3 * nc * nc; t += 64) {
        const int which = t / (3 * nc * nc), u = t % (3 * nc * nc);
        const int q = ((u / (nc * nc)) * FDA_NC + (u / nc) % nc) * FDA_NC + u % nc;
        const double* p = part + ((size_t)b * 2 + which) * bands * FDA_NG + q;
        double s = 0.0;
        for (int k = 0; k < bands; ++k) s = s + p[(size_t)k * FDA_NG];
        s_g[which][q] = s;
    }
    __syncthreads();
    if (threadIdx.x >= 3) return;
    const int c = threadIdx.x;
    const double* gs = s_g[0] + c * FDA_NC * FDA_NC;
    const double* gt = s_g[1] + c * FDA_NC * FDA_NC;
    double* cf = s_cf[c];
    for (int q = 0; q < FDA_NC * FDA_NC; ++q) cf[q] = 0.0;
    const double hw = (double)H * (double)W;
    for (int ky = 0; ky <= nb; ++ky)
        for (int kx = ky ? -nb : 0; kx <= nb; ++kx) {
            const int ax = kx < 0 ? -kx : kx;
            const double sg = kx < 0 ? -1.0 : 1.0;
            const int ci = ky ? 2 * ky - 1 : 0, si = 2 * ky, cj = ax ? 2 * ax - 1 : 0, sj = 2 * ax;     // si / sj unused at 0
            // S = sum v exp(-i (ky ty + kx tx)):  Re = G[c][c] - sg G[s][s],  Im = -(G[s][c] + sg G[c][s])
            double sr = gs[ci * FDA_NC + cj], sim = 0.0, tr = gt[ci * FDA_NC + cj], tim = 0.0;
            if (ky && ax) {
                sr = sr - sg * gs[si * FDA_NC + sj];
                tr = tr - sg * gt[si * FDA_NC + sj];
            }
            if (ky) {
                sim = sim + gs[si * FDA_NC + cj];
                tim = tim + gt[si * FDA_NC + cj];
            }
            if (ax) {
                sim = sim + sg * gs[ci * FDA_NC + sj];
                tim = tim + sg * gt[ci * FDA_NC + sj];
            }
            sim = -sim;
            tim = -tim;
            const double ms = sqrt(sr * sr + sim * sim), mt = sqrt(tr * tr + tim * tim);
            const double pr = ms == 0.0 ? 1.0 : sr / ms, pi = ms == 0.0 ? 0.0 : sim / ms;
            const double w = (ky || ax) ? 2.0 : 1.0;          // the bin and its conjugate partner
            const double dr = w * ((mt - ms) * pr / hw), di = w * ((mt - ms) * pi / hw);
            // Re(D exp(+i (ky ty + kx tx))) = dr (cy cx - sg sy sx) - di (sy cx + sg cy sx)
            cf[ci * FDA_NC + cj] = cf[ci * FDA_NC + cj] + dr;
            if (ky && ax) cf[si * FDA_NC + sj] = cf[si * FDA_NC + sj] - sg * dr;
            if (ky) cf[si * FDA_NC + cj] = cf[si * FDA_NC + cj] - di;
            if (ax) cf[ci * FDA_NC + sj] = cf[ci * FDA_NC + sj] - sg * di;
        }
    double* out = coef + ((size_t)b * 3 + c) * FDA_NC * FDA_NC;
    for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nc; ++j) out[i * FDA_NC + j] = cf[i * FDA_NC + j];
}

template <int NB>
__device__ __forceinline__ void fda_apply_row(uint8_t* __restrict__ row, const double* __restrict__ cx,
                                              const double* __restrict__ sx, const double (*rc)[FDA_NC], int W)
{
    constexpr int NC = 1 + 2 * NB;
    const bool words = (reinterpret_cast<uintptr_t>(row) & 3) == 0;
    for (int x0 = threadIdx.x * 4; x0 < W; x0 += 1024) {
        const int n = min(4, W - x0);
        unsigned v[12];
        load4(row, words, x0, n, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double r[NC];
            basis<NB>(cx, sx, min(x0 + i, W - 1), W, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double f = (double)v[3 * i + c];
#pragma unroll
                for (int j = 0; j < NC; ++j) f = f + rc[c][j] * r[j];
                f = f < 0.0 ? 0.0 : (f > 255.0 ? 255.0 : f);  // (NaN cannot arise: finite coefficients)
                v[3 * i + c] = (unsigned)(int)f;              // truncation
            }
        }
        if (words && n == 4) {
            pack12(v, reinterpret_cast<uint32_t*>(row + (size_t)x0 * 3));
        } else {
            for (int i = 0; i < 3 * n; ++i) row[(size_t)x0 * 3 + i] = (uint8_t)v[i];
        }
    }
}

// launch 3: block (row, sample), in place; each thread reads its 12 bytes before it writes them
__global__ __launch_bounds__(256) void aug3_fda_apply_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                             const double* __restrict__ trig, const double* __restrict__ coef,
                                                             uint8_t* __restrict__ img, int H, int W)
{
    __shared__ double s_rc[3][FDA_NC];
    const int b = blockIdx.y, y = blockIdx.x;
    long long off = 0;
    const int nb = fda_of(ops, seg, b, off);
    if (nb < 0) return;
    const int nc = 1 + 2 * nb;
    if ((int)threadIdx.x < 3 * nc) {                          // C folded with e(y): the row's 1 + 2 border coefficients
        const int c = threadIdx.x / nc, j = threadIdx.x % nc;
        const double* cf = coef + ((size_t)b * 3 + c) * FDA_NC * FDA_NC;
        double s = cf[j];
        int a = 0;
        for (int k = 1; k <= nb; ++k) {
            a += y;
            a = a >= H ? a - H : a;
            s = s + cf[(2 * k - 1) * FDA_NC + j] * trig[a];
            s = s + cf[(2 * k) * FDA_NC + j] * trig[H + a];
        }
        s_rc[c][j] = s;
    }
    __syncthreads();
    uint8_t* row = img + ((size_t)b * H + y) * W * 3;
    const double *cx = trig + 2 * (size_t)H, *sx = cx + W;
    if (nb == 0) fda_apply_row<0>(row, cx, sx, s_rc, W);
    else if (nb == 1) fda_apply_row<1>(row, cx, sx, s_rc, W);
    else fda_apply_row<2>(row, cx, sx, s_rc, W);
}

}  // namespace hiast

static int fda_bands(int H) { return (H + hiast::FDA_ROWS - 1) / hiast::FDA_ROWS; }

extern "C" size_t hiast_aug3_fda_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * (2 * (size_t)fda_bands(H) + 1) * hiast::FDA_NG * sizeof(double);
}

extern "C" int hiast_aug3_fda_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const double* trig, uint8_t* img,
                                 double* ws, int B, int H, int W, hiast_stream_t stream)
{
    if (!ops || !seg || !blob || !trig || !img || !ws) return HIAST_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    if (B > 65535 || H < 8 || W < 8 || H > (1 << 20) || W > (1 << 20)) return HIAST_E_RANGE;
    const int bands = fda_bands(H);
    double* coef = ws + (size_t)B * 2 * bands * hiast::FDA_NG;
    hipLaunchKernelGGL(hiast::aug3_fda_sums_kernel, dim3(bands, 2, B), dim3(256), 0, (hipStream_t)stream, ops, seg, blob, trig,
                       img, ws, H, W);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::aug3_fda_coef_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ops, seg, ws, coef, bands, H, W);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::aug3_fda_apply_kernel, dim3(H, B), dim3(256), 0, (hipStream_t)stream, ops, seg, trig, coef, img,
                       H, W);
    HIAST_CHECK_LAUNCH();
    return 0;
}
