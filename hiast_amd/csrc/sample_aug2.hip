// K15b — the colour ops of the device-side sample path at every level, BYTE FOR BYTE what
// hiast_amd/sseg/datasets/augmentations.py computes on the host (device_aug.py holds the numpy restatements the kernels
// are tested against).  Level 1 (the default):
//   LUT         the 256-entry table the host code builds (neighbours composed on the host)
//   gray        OpenCV's fixed point
//   Equalize    cv2.equalizeHist: per-channel histogram -> float64 table, rint (half to even)
// Level 2 (cfg.dataset.device_aug_level: 2), ColorJitter and GaussianBlur as plan ops:
//   contrast    a 256-entry table built on the device from the gray mean of the image AT THAT POINT of the chain (the
//               gray histogram -> an exact integer sum -> float64 mean), float32 multiply + add, truncated
//   saturation  c * f32(f) + gray * f32(1 - f), each operation rounded to float32, truncated
//   hue         Pillow's C RGB -> HSV -> RGB round trip (float32 quotients, float64 wrap, C round()), H shifted mod 256
//   blur        scipy.ndimage.correlate1d's symmetric loop, axis 0 then axis 1, reflect-101: float64
//               o = x[c] w[s]; o += (x[c-j] + x[c+j]) w[s-j] for j = s..1, rounded to float32 per pass, rint at the end
// A view's op row (hiast_hip.h) is cut into SEGMENTS by the host: ops [from, to) are pointwise except for at most one
// table op (Equalize / contrast) at index `stat`, whose table is built from the image after ops [from, stat); a blur at
// index `blur` (== to) closes the segment.  seg int32 [B][4] = (from, to, stat | -1, blur | -1) per sample and launch
// round; a sample with an empty segment is skipped by its record, as finished samples are.  A row of level-1 ops is one
// segment (0, n_ops, index of its Equalize | -1, -1): one round, the table launches only if some row equalises.
// The float32 quotients go through a float64 division (53 >= 2 * 24 + 2 bits: the double rounding is innocuous), so
// they are correctly rounded whatever the compiler's float32 division is.  Built with -ffp-contract=off.
#include "aug_common.h"

namespace hiast {

__device__ __forceinline__ unsigned trunc8(float v) { return (unsigned)(int)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v)); }
__device__ __forceinline__ float div32(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ unsigned gray8(unsigned r, unsigned g, unsigned b) { return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14; }
__device__ __forceinline__ unsigned round8(double v)
{
    v = round(v);                                            // C round(): half away from zero
    return (unsigned)(int)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

__device__ __forceinline__ void hue_shift(unsigned& r, unsigned& g, unsigned& b, unsigned shift)
{
    const unsigned maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    if (maxc == minc) return;                                // (0, 0, v) -> S == 0 -> (v, v, v): the pixel unchanged
    const float cr = (float)(maxc - minc);
    const float s = div32(cr, (float)maxc);
    const float rc = div32((float)(maxc - r), cr), gc = div32((float)(maxc - g), cr), bc = div32((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double hd = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6]: fmod(hd, 1.0) == hd - floor(hd), exact
    h = (float)(hd - floor(hd));
    unsigned H = (unsigned)clampi((int)((double)h * 255.0), 0, 255);
    const unsigned S = (unsigned)clampi((int)((double)s * 255.0), 0, 255), V = maxc;
    H = (H + shift) & 255u;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double h6 = (double)H * 6.0 / 255.0;
    const double fl = floor(h6);
    const float f = (float)(h6 - fl);
    const float fs = (float)((double)S / 255.0);
    const double v = (double)V;
    const unsigned p = round8(v * (1.0 - (double)fs));
    const unsigned q = round8(v * (1.0 - (double)fs * (double)f));
    const unsigned t = round8(v * (1.0 - (double)fs * (1.0 - (double)f)));
    switch ((int)fl % 6) {
    case 0: r = V, g = t, b = p; break;
    case 1: r = q, g = V, b = p; break;
    case 2: r = p, g = V, b = t; break;
    case 3: r = p, g = q, b = V; break;
    case 4: r = t, g = p, b = V; break;
    default: r = V, g = p, b = q; break;
    }
}

// ops [from, to) of one view's op row on one pixel; tab: the sample's [3][256] table of this segment's table op
__device__ __forceinline__ void aug2_apply_ops(const int64_t* __restrict__ o, int from, int to, const uint8_t* __restrict__ blob,
                                               const uint8_t* __restrict__ tab, unsigned& r, unsigned& g, unsigned& b)
{
    for (int i = from; i < to; ++i) {
        const int type = (int)op_type(o, i);
        const int64_t par = op_par(o, i);
        if (type == HIAST_AUG_OP_LUT) {
            const uint8_t* lut = blob + par;
            r = lut[r];
            g = lut[g];
            b = lut[b];
        } else if (type == HIAST_AUG_OP_GRAY) {
            r = g = b = gray8(r, g, b);
        } else if (type == HIAST_AUG_OP_EQUALIZE || type == HIAST_AUG_OP_CONTRAST) {
            if (tab) {
                r = tab[r];
                g = tab[256 + g];
                b = tab[512 + b];
            }
        } else if (type == HIAST_AUG_OP_SAT) {
            const double fd = __longlong_as_double(par);
            const float f = (float)fd, f1 = (float)(1.0 - fd);
            const float gg = (float)gray8(r, g, b) * f1;
            float vr = (float)r * f, vg = (float)g * f, vb = (float)b * f;
            vr = vr + gg;
            vg = vg + gg;
            vb = vb + gg;
            r = trunc8(vr);
            g = trunc8(vg);
            b = trunc8(vb);
        } else if (type == HIAST_AUG_OP_HUE) {
            hue_shift(r, g, b, (unsigned)par & 255u);
        }
    }
}

// histogram of the image a segment's table op meets: per channel (Equalize) or of the gray value (contrast, bins
// 0..255 of the sample's 768): LDS integer atomics, then one global integer atomic per non-empty bin
__global__ __launch_bounds__(256) void aug2_hist_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                        const uint8_t* __restrict__ blob, const uint8_t* __restrict__ in,
                                                        unsigned* __restrict__ hist, long long HW)
{
    const int b = blockIdx.y;
    const int64_t* o = ops + (size_t)b * OPS;
    const Seg s = seg_of(o, seg + b * 4);
    if (!s.live || s.stat < 0) return;
    const bool contrast = op_type(o, s.stat) == HIAST_AUG_OP_CONTRAST;
    __shared__ unsigned s_h[768];
    for (int i = threadIdx.x; i < 768; i += 256) s_h[i] = 0;
    __syncthreads();
    const uint8_t* src = in + (size_t)b * HW * 3;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
        unsigned r = src[p * 3], g = src[p * 3 + 1], bl = src[p * 3 + 2];
        aug2_apply_ops(o, s.from, s.stat, blob, nullptr, r, g, bl);
        if (contrast) {
            atomicAdd(&s_h[gray8(r, g, bl)], 1u);
        } else {
            atomicAdd(&s_h[r], 1u);
            atomicAdd(&s_h[256 + g], 1u);
            atomicAdd(&s_h[512 + bl], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 768; i += 256)
        if (s_h[i]) atomicAdd(&hist[(size_t)b * 768 + i], s_h[i]);
}

// the segment's table from its histogram, one thread per (sample, channel): cv2.equalizeHist's (float64, rint) or
// ColorJitter's contrast table (the same 256 entries for the three channels)
__global__ __launch_bounds__(64) void aug2_table_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                        const unsigned* __restrict__ hist, uint8_t* __restrict__ tab, long long HW)
{
    if (threadIdx.x >= 3) return;
    const int b = blockIdx.x;
    const int64_t* o = ops + (size_t)b * OPS;
    const Seg s = seg_of(o, seg + b * 4);
    if (!s.live || s.stat < 0) return;
    uint8_t* lut = tab + (size_t)b * 768 + threadIdx.x * 256;
    if (op_type(o, s.stat) == HIAST_AUG_OP_CONTRAST) {
        const unsigned* h = hist + (size_t)b * 768;
        long long sum = 0;
        for (int i = 0; i < 256; ++i) sum += (long long)i * (long long)h[i];
        const double fd = __longlong_as_double(op_par(o, s.stat));
        const double mean = (double)sum / (double)HW;
        const float f = (float)fd, add = (float)(mean * (1.0 - fd));
        for (int i = 0; i < 256; ++i) {
            float v = (float)i * f;
            v = v + add;
            lut[i] = (uint8_t)trunc8(v);
        }
        return;
    }
    const unsigned* h = hist + (size_t)b * 768 + threadIdx.x * 256;
    int first = 0;
    while (first < 256 && h[first] == 0) ++first;
    if (first == 256) return;
    if ((long long)h[first] == HW) {                       // constant channel: the image unchanged
        for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)first;
        return;
    }
    const double scale = 255.0 / (double)(HW - (long long)h[first]);
    long long acc = 0;
    for (int i = 0; i < 256; ++i) {
        if (i <= first) {
            lut[i] = 0;
            continue;
        }
        acc += h[i];
        const double v = rint((double)acc * scale);
        lut[i] = (uint8_t)(v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v));
    }
}

// a segment's ops on uint8 HWC.  in != out: every sample is written (a finished view is copied from the blob, an empty
// segment copies); in == out: a sample without ops in this segment is not touched.  Each thread reads its pixels
// before it writes them, so in place is safe.
__global__ __launch_bounds__(256) void aug2_colour_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                          const uint8_t* __restrict__ blob, const uint8_t* __restrict__ tab,
                                                          const uint8_t* in, uint8_t* out, long long HW)
{
    const int b = blockIdx.y;
    const int64_t* o = ops + (size_t)b * OPS;
    const Seg s = seg_of(o, seg + b * 4);
    const bool inplace = in == out;
    if (inplace && (!s.live || s.to <= s.from)) return;
    const uint8_t* src = !s.live ? blob + o[1] : in + (size_t)b * HW * 3;
    uint8_t* dst = out + (size_t)b * HW * 3;
    const uint8_t* t = tab + (size_t)b * 768;
    const long long step = (long long)gridDim.x * 256;
    if ((HW & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < HW / 4; q += step) {
            unsigned c[12];
            unpack12(s4 + q * 3, c);
#pragma unroll
            for (int i = 0; i < 4; ++i) aug2_apply_ops(o, s.from, s.to, blob, t, c[3 * i], c[3 * i + 1], c[3 * i + 2]);
            pack12(c, d4 + q * 3);
        }
    } else {
        for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += step) {
            unsigned r = src[p * 3], g = src[p * 3 + 1], bl = src[p * 3 + 2];
            aug2_apply_ops(o, s.from, s.to, blob, t, r, g, bl);
            dst[p * 3] = (uint8_t)r;
            dst[p * 3 + 1] = (uint8_t)g;
            dst[p * 3 + 2] = (uint8_t)bl;
        }
    }
}

// ---- blur -----------------------------------------------------------------------------------------------------------
constexpr int MAX_K = HIAST_AUG_MAX_KSIZE;
constexpr int MAX_S = MAX_K / 2;

__device__ __forceinline__ int mirror(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return clampi(i, 0, n - 1);                              // (s < n, checked by the host: the clamp never acts)
}

// the blur of this sample's segment: half width (0 = none) and its weights as float64 in LDS; block-uniform
__device__ __forceinline__ int blur_of(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                       const int32_t* __restrict__ tabs, int b, int H, int W, double* s_w)
{
    const int64_t* o = ops + (size_t)b * OPS;
    const Seg sg = seg_of(o, seg + b * 4);
    if (!sg.live || sg.blur < 0 || op_type(o, sg.blur) != HIAST_AUG_OP_BLUR) return 0;
    const int64_t par = op_par(o, sg.blur);
    const int ks = (int)(par >> 32), s = ks >> 1;
    if (ks < 3 || ks > MAX_K || !(ks & 1) || s >= H || s >= W) return 0;
    if ((int)threadIdx.x < ks) s_w[threadIdx.x] = (double)__int_as_float(tabs[(par & 0xffffffffll) + threadIdx.x]);
    __syncthreads();
    return s;
}

// pass 1, axis 0 (down the rows; channel-agnostic over the W*3 bytes of a row): uint8 -> float32 tmp [B][H][W*3]
template <int VEC>
__global__ __launch_bounds__(256) void aug2_blur_rows_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ tabs, const uint8_t* __restrict__ img,
                                                             float* __restrict__ tmp, int H, int W)
{
    __shared__ double s_w[MAX_K];
    const int b = blockIdx.z, y = blockIdx.y;
    const int s = blur_of(ops, seg, tabs, b, H, W, s_w);
    if (s == 0) return;
    const int rowb = W * 3;
    const int q = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (q >= rowb) return;
    const uint8_t* base = img + (size_t)b * H * rowb + q;
    double acc[VEC];
    unsigned a[VEC], c[VEC];
    auto load = [&](int row, unsigned* v) {
        const uint8_t* p = base + (size_t)row * rowb;
        if (VEC == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = (w >> (8 * i)) & 255u;
        } else {
            v[0] = p[0];
        }
    };
    load(y, a);
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = (double)a[i] * s_w[s];
    for (int j = s; j >= 1; --j) {
        load(mirror(y - j, H), a);
        load(mirror(y + j, H), c);
        const double w = s_w[s - j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const double pair = (double)a[i] + (double)c[i];
            const double prod = pair * w;
            acc[i] = acc[i] + prod;
        }
    }
    float* d = tmp + ((size_t)b * H + y) * rowb + q;
    if (VEC == 4) {
        *reinterpret_cast<float4*>(d) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
        d[0] = (float)acc[0];
    }
}

// pass 2, axis 1 (along a row, neighbours 3 elements apart): 256 outputs per block, their row segment + the 3*s halo
// on either side staged in LDS with the border already reflected; float32 -> rint -> uint8, in place over the image
__global__ __launch_bounds__(256) void aug2_blur_cols_kernel(const int64_t* __restrict__ ops, const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ tabs, const float* __restrict__ tmp,
                                                             uint8_t* __restrict__ img, int H, int W)
{
    __shared__ double s_w[MAX_K];
    __shared__ float s_x[256 + 6 * MAX_S];
    const int b = blockIdx.z, y = blockIdx.y;
    const int s = blur_of(ops, seg, tabs, b, H, W, s_w);
    if (s == 0) return;
    const int rowb = W * 3;
    const int e0 = blockIdx.x * 256;
    const float* row = tmp + ((size_t)b * H + y) * rowb;
    for (int l = threadIdx.x; l < 256 + 6 * s; l += 256) {
        const int e = e0 + l - 3 * s;
        const int p = e >= 0 ? e / 3 : -((2 - e) / 3);       // floor(e / 3)
        const int ch = e - 3 * p;
        s_x[l] = row[mirror(p, W) * 3 + ch];
    }
    __syncthreads();
    const int e = e0 + threadIdx.x;
    if (e >= rowb) return;
    const int l = threadIdx.x + 3 * s;
    double acc = (double)s_x[l] * s_w[s];
    for (int j = s; j >= 1; --j) {
        const double pair = (double)s_x[l - 3 * j] + (double)s_x[l + 3 * j];
        const double prod = pair * s_w[s - j];
        acc = acc + prod;
    }
    float v = rintf((float)acc);                             // half to even
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    img[((size_t)b * H + y) * rowb + e] = (uint8_t)(int)v;
}

}  // namespace hiast

extern "C" int hiast_aug2_table_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const uint8_t* in,
                                   uint32_t* hist, uint8_t* table, int B, int64_t HW, hiast_stream_t stream)
{
    if (!ops || !seg || !blob || !in || !hist || !table) return HIAST_E_ARG;
    if (B <= 0 || HW <= 0) return HIAST_E_ARG;
    if (B > 65535 || HW >= (1ll << 31)) return HIAST_E_RANGE;            // 32-bit bins
    if (hipMemsetAsync(hist, 0, (size_t)B * 768 * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return HIAST_E_ARG;
    hipLaunchKernelGGL(hiast::aug2_hist_kernel, dim3(aug_pixel_blocks(HW), B), dim3(256), 0, (hipStream_t)stream, ops, seg,
                       blob, in, hist, (long long)HW);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::aug2_table_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ops, seg, hist, table,
                       (long long)HW);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_aug2_colour_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const uint8_t* table,
                                    const uint8_t* in, uint8_t* out, int B, int64_t HW, hiast_stream_t stream)
{
    if (!ops || !seg || !blob || !table || !in || !out) return HIAST_E_ARG;
    if (B <= 0 || HW <= 0) return HIAST_E_ARG;
    if (B > 65535) return HIAST_E_RANGE;
    hipLaunchKernelGGL(hiast::aug2_colour_kernel, dim3(aug_pixel_blocks(HW), B), dim3(256), 0, (hipStream_t)stream, ops, seg,
                       blob, table, in, out, (long long)HW);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_aug2_blur_u8(const int64_t* ops, const int32_t* seg, const int32_t* tabs, uint8_t* img, float* tmp,
                                  int B, int H, int W, hiast_stream_t stream)
{
    if (!ops || !seg || !tabs || !img || !tmp) return HIAST_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    if (B > 65535 || H > 65535 || W > (1 << 20)) return HIAST_E_RANGE;
    const int rowb = W * 3;
    if (rowb % 4 == 0 && ((((uintptr_t)img) | ((uintptr_t)tmp)) & 15) == 0)
        hipLaunchKernelGGL(hiast::aug2_blur_rows_kernel<4>, dim3((rowb / 4 + 255) / 256, H, B), dim3(256), 0,
                           (hipStream_t)stream, ops, seg, tabs, img, tmp, H, W);
    else
        hipLaunchKernelGGL(hiast::aug2_blur_rows_kernel<1>, dim3((rowb + 255) / 256, H, B), dim3(256), 0, (hipStream_t)stream,
                           ops, seg, tabs, img, tmp, H, W);
    HIAST_CHECK_LAUNCH();
    hipLaunchKernelGGL(hiast::aug2_blur_cols_kernel, dim3((rowb + 255) / 256, H, B), dim3(256), 0, (hipStream_t)stream, ops,
                       seg, tabs, tmp, img, H, W);
    HIAST_CHECK_LAUNCH();
    return 0;
}
