// K15 for the mixing preprocessors (PREPROCESSOR['ClassMix'] / ['CutMix'], hiast_amd/sseg/datasets/preprocessor.py): the
// geometry pass of sample_aug.hip — the same two launches, the same integer arithmetic — with a select on load that also
// knows a rectangle, and the copy_paste_mask of a batch of device-resident frames in one launch.
//   record kind 3 = kind 0 (window bytes in the blob), kind 4 = kind 2 (window read in place from the store), each with a
//   rectangle: the record's paste_table word points at 256 table bytes followed by ry0, ry1, rx0, rx1 (little-endian
//   int32, WINDOW coordinates of the unflipped window, half-open, clipped by the host; empty: ry0 == ry1).
//   select: ptab[plbl[col]] && ry0 <= row < ry1 && rx0 <= col < rx1.  Kinds 0 and 2 select on the table alone, as before.
// The row test is uniform per block row: a row outside the rectangle takes the no-paste pointers and never reads the source;
// the column test comes before the source label is read, so no byte of the source outside the rectangle is ever loaded.
// The rectangle is clamped to the window again here: the host wrapper rejects a wrong one (aug_mix_host.h), the clamp keeps
// it from mattering.  hiast_aug_geometry_u8 / _store_u8 (sample_aug.hip) keep their kernels: kinds 0..2 only.
#include "aug_common.h"
#include "aug_mix_host.h"

namespace hiast {

enum { R_KIND, R_IMG, R_LBL, R_PIMG, R_PLBL, R_PTAB, R_CH, R_CW, R_FLIP, R_HLO, R_HN, R_HK, R_HT, R_VLO, R_VN, R_VK, R_VT,
       R_NX, R_NY, R_STRIDE };
enum { KIND_PLAN = 0, KIND_FINISHED = 1, KIND_STORE = HIAST_STORE_KIND, KIND_PLAN_RECT = HIAST_MIX_KIND_PLAN_RECT,
       KIND_STORE_RECT = HIAST_MIX_KIND_STORE_RECT };
static_assert(R_STRIDE == HIAST_STORE_REC_STRIDE && R_STRIDE < HIAST_AUG_REC_WORDS, "the stride is the record's spare word");
constexpr int REC = HIAST_AUG_REC_WORDS;
constexpr int PBITS = 22;

__device__ __forceinline__ unsigned mix_clip8(int v) { return (unsigned)clampi(v >> PBITS, 0, 255); }

// where a sample's window lies (sample_aug.hip's Window) and what its paste is confined to.  live: a planned sample this
// launch can read (a store kind needs a store); finished: kind 1; anything else is left alone
struct MixWindow {
    const uint8_t* base;
    size_t stride;
    bool live, finished, paste, boxed;
    int ry0, ry1, rx0, rx1;
};
__device__ __forceinline__ MixWindow mix_window_of(const int64_t* r, const uint8_t* blob, const uint8_t* store)
{
    MixWindow w;
    const int64_t kind = r[R_KIND];
    const bool in_store = kind == KIND_STORE || kind == KIND_STORE_RECT;
    const bool rect = kind == KIND_PLAN_RECT || kind == KIND_STORE_RECT;
    const int64_t cw = r[R_CW];
    w.finished = kind == KIND_FINISHED;
    w.live = in_store ? store != nullptr : (kind == KIND_PLAN || kind == KIND_PLAN_RECT);
    w.base = in_store ? store : blob;
    w.stride = (size_t)(in_store && r[R_STRIDE] > cw ? r[R_STRIDE] : cw);
    w.paste = r[R_PIMG] >= 0 && r[R_PLBL] >= 0 && r[R_PTAB] >= 0;
    w.ry0 = 0, w.ry1 = (int)r[R_CH], w.rx0 = 0, w.rx1 = (int)cw;
    w.boxed = rect;
    if (rect && w.paste && w.live) {
        const int32_t* q = reinterpret_cast<const int32_t*>(blob + r[R_PTAB] + 256);
        w.ry0 = clampi(q[0], 0, (int)r[R_CH]);
        w.ry1 = clampi(q[1], w.ry0, (int)r[R_CH]);
        w.rx0 = clampi(q[2], 0, (int)cw);
        w.rx1 = clampi(q[3], w.rx0, (int)cw);
    } else if (rect) {
        w.paste = false;
    }
    return w;
}

// horizontal pass: one thread per (output column, source row) of a planned sample -> tmp [B][max_ch][ow][3]
__global__ __launch_bounds__(256) void mix_hpass_kernel(const int64_t* __restrict__ recs, const uint8_t* __restrict__ blob,
                                                        const uint8_t* __restrict__ store, const int32_t* __restrict__ tabs,
                                                        uint8_t* __restrict__ tmp, int max_ch, int ow)
{
    const int64_t* r = recs + (size_t)blockIdx.z * REC;
    const MixWindow win = mix_window_of(r, blob, store);
    if (!win.live) return;
    const int ch = (int)r[R_CH], cw = (int)r[R_CW], row = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (row >= ch || x >= ow) return;
    const bool flip = r[R_FLIP] != 0;
    const bool paste = win.paste && row >= win.ry0 && row < win.ry1;         // uniform per block row
    const int rx0 = win.rx0, rx1 = win.rx1;
    const uint8_t* img = win.base + r[R_IMG] + (size_t)row * win.stride * 3;
    const uint8_t* pimg = paste ? win.base + r[R_PIMG] + (size_t)row * win.stride * 3 : img;
    const uint8_t* plbl = paste ? win.base + r[R_PLBL] + (size_t)row * win.stride : img;
    const uint8_t* ptab = paste ? blob + r[R_PTAB] : img;
    const int T = (int)r[R_HT], lo = tabs[r[R_HLO] + x], n = tabs[r[R_HN] + x];
    const int32_t* k = tabs + r[R_HK] + (size_t)x * T;
    int a0 = 1 << (PBITS - 1), a1 = a0, a2 = a0;
    if (win.boxed) {                        // uniform per sample: kinds 0 and 2 keep the loop of sample_aug.hip
        const unsigned rxn = (unsigned)(rx1 - rx0);
        for (int t = 0; t < n && t < T; ++t) {
            const int j = clampi(lo + t, 0, cw - 1);
            const int col = flip ? cw - 1 - j : j;
            const uint8_t* p = (paste && (unsigned)(col - rx0) < rxn && ptab[plbl[col]]) ? pimg + col * 3 : img + col * 3;
            const int w = k[t];
            a0 += w * p[0];
            a1 += w * p[1];
            a2 += w * p[2];
        }
    } else {
        for (int t = 0; t < n && t < T; ++t) {
            const int j = clampi(lo + t, 0, cw - 1);
            const int col = flip ? cw - 1 - j : j;
            const uint8_t* p = (paste && ptab[plbl[col]]) ? pimg + col * 3 : img + col * 3;
            const int w = k[t];
            a0 += w * p[0];
            a1 += w * p[1];
            a2 += w * p[2];
        }
    }
    uint8_t* d = tmp + (((size_t)blockIdx.z * max_ch + row) * ow + x) * 3;
    d[0] = (uint8_t)mix_clip8(a0);
    d[1] = (uint8_t)mix_clip8(a1);
    d[2] = (uint8_t)mix_clip8(a2);
}

// vertical pass (VEC = 4 bytes per thread when ow*3 is a multiple of 4) + the label gather through the same select + the
// copy of finished (host-augmented) samples
template <int VEC>
__global__ __launch_bounds__(256) void mix_vpass_kernel(const int64_t* __restrict__ recs, const uint8_t* __restrict__ blob,
                                                        const uint8_t* __restrict__ store, const int32_t* __restrict__ tabs,
                                                        const uint8_t* __restrict__ tmp,
                                                        uint8_t* __restrict__ img_out, uint8_t* __restrict__ lbl_out,
                                                        int max_ch, int oh, int ow)
{
    const int b = blockIdx.z, y = blockIdx.y;
    const int64_t* r = recs + (size_t)b * REC;
    const int rowb = ow * 3;
    const int q = (blockIdx.x * 256 + threadIdx.x) * VEC;
    uint8_t* dimg = img_out + ((size_t)b * oh + y) * rowb;
    uint8_t* dlbl = lbl_out + ((size_t)b * oh + y) * ow;
    const int stride = gridDim.x * 256;
    const MixWindow win = mix_window_of(r, blob, store);
    if (win.finished) {                     // finished view 0 + label of a host-augmented sample
        const uint8_t* s = blob + r[R_IMG] + (size_t)y * rowb;
        if (q < rowb) {
            if (VEC == 4) *reinterpret_cast<uint32_t*>(dimg + q) = *reinterpret_cast<const uint32_t*>(s + q);
            else dimg[q] = s[q];
        }
        const uint8_t* sl = blob + r[R_LBL] + (size_t)y * ow;
        for (int x = blockIdx.x * 256 + threadIdx.x; x < ow; x += stride) dlbl[x] = sl[x];
        return;
    }
    if (!win.live) return;
    const int ch = (int)r[R_CH], cw = (int)r[R_CW];
    if (q < rowb) {
        const int T = (int)r[R_VT], lo = tabs[r[R_VLO] + y], n = tabs[r[R_VN] + y];
        const int32_t* k = tabs + r[R_VK] + (size_t)y * T;
        int a[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) a[i] = 1 << (PBITS - 1);
        for (int t = 0; t < n && t < T; ++t) {
            const int row = clampi(lo + t, 0, ch - 1);
            const uint8_t* s = tmp + ((size_t)b * max_ch + row) * rowb + q;
            const int w = k[t];
            if (VEC == 4) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(s);
#pragma unroll
                for (int i = 0; i < VEC; ++i) a[i] += w * (int)((v >> (8 * i)) & 255u);
            } else {
                a[0] += w * s[0];
            }
        }
        if (VEC == 4) {
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) v |= mix_clip8(a[i]) << (8 * i);
            *reinterpret_cast<uint32_t*>(dimg + q) = v;
        } else {
            dimg[q] = (uint8_t)mix_clip8(a[0]);
        }
    }
    const bool flip = r[R_FLIP] != 0;
    const int sy = clampi(tabs[r[R_NY] + y], 0, ch - 1);
    const bool paste = win.paste && sy >= win.ry0 && sy < win.ry1;           // uniform per block row
    const int rx0 = win.rx0, rx1 = win.rx1;
    const uint8_t* lbl = win.base + r[R_LBL] + (size_t)sy * win.stride;
    const uint8_t* plbl = paste ? win.base + r[R_PLBL] + (size_t)sy * win.stride : lbl;
    const uint8_t* ptab = paste ? blob + r[R_PTAB] : lbl;
    const unsigned rxn = (unsigned)(rx1 - rx0);        // (kinds 0 and 2: [0, cw), every column passes)
    for (int x = blockIdx.x * 256 + threadIdx.x; x < ow; x += stride) {
        const int sx = clampi(tabs[r[R_NX] + x], 0, cw - 1);
        const int col = flip ? cw - 1 - sx : sx;
        uint8_t l = lbl[col];
        if (paste && (unsigned)(col - rx0) < rxn) {
            const uint8_t pl = plbl[col];
            if (ptab[pl]) l = pl;
        }
        dlbl[x] = l;
    }
}

// copy_paste_mask: one block row per record of prm [n][8] = (source label offset in the store | -1, table offset in the
// blob, y0, y1, x0, x1 in FRAME coordinates, frame of `out`, 0): out[frame][y][x] = (table[src] && in rect) ? src : 255.
// A frame is walked as HW flat bytes, 16 per lane where both the source label and the output frame start on a 16-byte
// boundary (frames of the store do), one byte per lane over the tail (or over everything otherwise).  A 16-byte piece whose
// rows all miss the rectangle is written without reading the source.
__device__ __forceinline__ uint32_t mask_word(uint32_t v, const uint8_t* tab, int& y, int& x, int W, int y0, int y1, int x0,
                                              int x1)
{
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (v >> (8 * i)) & 255u;
        const bool in = y >= y0 && y < y1 && x >= x0 && x < x1;
        o |= ((in && tab[s]) ? s : 255u) << (8 * i);
        if (++x == W) {
            x = 0;
            ++y;
        }
    }
    return o;
}

__global__ __launch_bounds__(256) void paste_mask_kernel(const int64_t* __restrict__ prm, const uint8_t* __restrict__ store,
                                                         const uint8_t* __restrict__ blob, uint8_t* __restrict__ out,
                                                         long long HW, int H, int W)
{
    __shared__ uint8_t tab[256];
    const int64_t* p = prm + (size_t)blockIdx.y * 8;
    const int64_t soff = p[0];
    const int y0 = clampi((int)p[2], 0, H), y1 = clampi((int)p[3], 0, H);
    const int x0 = clampi((int)p[4], 0, W), x1 = clampi((int)p[5], 0, W);
    const bool any = soff >= 0 && y0 < y1 && x0 < x1;
    tab[threadIdx.x] = any ? blob[p[1] + threadIdx.x] : (uint8_t)0;
    __syncthreads();
    const uint8_t* src = any ? store + soff : out;
    uint8_t* dst = out + (size_t)p[6] * HW;
    const bool wide = ((((uintptr_t)dst) | (any ? (uintptr_t)src : (uintptr_t)0)) & 15) == 0;
    const long long nvec = wide ? HW / 16 : 0;
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x, gs = (long long)gridDim.x * 256;
    for (long long c = gt; c < nvec; c += gs) {
        const long long i = c * 16;
        int y = (int)(i / W), x = (int)(i - (long long)y * W);
        const int ylast = (int)((i + 15) / W);
        uint4 o;
        if (!any || ylast < y0 || y >= y1) {
            o.x = o.y = o.z = o.w = 0xFFFFFFFFu;
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(src + i);
            o.x = mask_word(v.x, tab, y, x, W, y0, y1, x0, x1);
            o.y = mask_word(v.y, tab, y, x, W, y0, y1, x0, x1);
            o.z = mask_word(v.z, tab, y, x, W, y0, y1, x0, x1);
            o.w = mask_word(v.w, tab, y, x, W, y0, y1, x0, x1);
        }
        *reinterpret_cast<uint4*>(dst + i) = o;
    }
    for (long long i = nvec * 16 + gt; i < HW; i += gs) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        uint8_t o = 255;
        if (any && y >= y0 && y < y1 && x >= x0 && x < x1) {
            const uint8_t s = src[i];
            if (tab[s]) o = s;
        }
        dst[i] = o;
    }
}

}  // namespace hiast

extern "C" int hiast_aug_records_check(const int64_t* recs, const uint8_t* blob, int64_t blob_bytes, int B, int max_kind)
{
    return hiast_mix_host::check_records(recs, blob, blob_bytes, B, max_kind);
}

extern "C" int hiast_aug_geometry_mix_u8(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs,
                                         uint8_t* tmp, uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                                         hiast_stream_t stream)
{
    if (!recs || !blob || !tabs || !tmp || !img_out || !lbl_out) return HIAST_E_ARG;         // (store may be null)
    if (B <= 0 || max_ch <= 0 || oh <= 0 || ow <= 0) return HIAST_E_ARG;
    if (B > 65535 || max_ch > 65535 || oh > 65535 || ow > (1 << 20)) return HIAST_E_RANGE;
    if ((((uintptr_t)blob) & 3) != 0) return HIAST_E_ARG;                                    // (the rectangle is read as int32)
    hipLaunchKernelGGL(hiast::mix_hpass_kernel, dim3((ow + 255) / 256, max_ch, B), dim3(256), 0, (hipStream_t)stream, recs,
                       blob, store, tabs, tmp, max_ch, ow);
    HIAST_CHECK_LAUNCH();
    const int rowb = ow * 3;
    if (rowb % 4 == 0 && ((((uintptr_t)tmp) | ((uintptr_t)img_out)) & 3) == 0)
        hipLaunchKernelGGL(hiast::mix_vpass_kernel<4>, dim3((rowb / 4 + 255) / 256, oh, B), dim3(256), 0, (hipStream_t)stream,
                           recs, blob, store, tabs, tmp, img_out, lbl_out, max_ch, oh, ow);
    else
        hipLaunchKernelGGL(hiast::mix_vpass_kernel<1>, dim3((rowb + 255) / 256, oh, B), dim3(256), 0, (hipStream_t)stream,
                           recs, blob, store, tabs, tmp, img_out, lbl_out, max_ch, oh, ow);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_aug_paste_mask_u8(const int64_t* prm, const uint8_t* store, const uint8_t* blob, uint8_t* out, int n, int H,
                                       int W, hiast_stream_t stream)
{
    if (!prm || !store || !blob || !out) return HIAST_E_ARG;
    if (n <= 0 || H <= 0 || W <= 0) return HIAST_E_ARG;
    if (n > 65535 || (long long)H * W > (1ll << 31) - 16) return HIAST_E_RANGE;
    const long long HW = (long long)H * W;
    long long nb = (HW / 16 + 255) / 256;
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    hipLaunchKernelGGL(hiast::paste_mask_kernel, dim3((unsigned)nb, n), dim3(256), 0, (hipStream_t)stream, prm, store, blob, out,
                       HW, H, W);
    HIAST_CHECK_LAUNCH();
    return 0;
}
