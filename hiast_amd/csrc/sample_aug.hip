// K15 — the per-sample data path on the device (reference: sseg/datasets/augmentations.py + preprocessor.py, executed in
// DataLoader workers through albumentations / OpenCV; here hiast_amd/sseg/datasets/augmentations.py is the host form).
// A worker hands over bytes + a PLAN (hiast_amd/sseg/datasets/device_aug.py): every random decision is drawn on the
// host, the kernels are pure functions of bytes + plan and reproduce the host code BYTE FOR BYTE.  This file is the
// geometry: CopyPaste select on load, flipped read, Pillow's two-pass 8-bit bilinear resample (22-bit fixed-point
// weights, the horizontal pass rounded to uint8 before the vertical one), nearest gather of the label, all in integers.
// The colour ops of every level (256-entry LUTs, OpenCV's fixed-point gray, cv2.equalizeHist, ...) are sample_aug2.hip.
// One launch covers the whole batch: per sample one int64 record row of offsets into ONE uint8 blob and ONE int32 table
// blob (hiast_hip.h), as hiast_ema_update / hiast_multi_copy do with pointers.
// Table indices are clamped to the sample's extent before they address memory: the host wrapper rejects a table that
// points outside, the clamp keeps a wrong table from leaving the buffers.
// Device-resident frames (hiast_amd/sseg/datasets/device_store.py): a record of kind 2 addresses its window, and its
// CopyPaste source window, in place in the STORE of decoded frames instead of the blob: the same reads with the frame's
// width as the row stride (record word 19) instead of cw.  The paste table and all tap tables stay in blob / tabs.
// The mixing preprocessors (PREPROCESSOR['ClassMix'] / ['CutMix'], hiast_amd/sseg/datasets/preprocessor.py) confine the
// paste to a rectangle:
//   record kind 3 = kind 0 (window bytes in the blob), kind 4 = kind 2 (window read in place from the store), each with a
//   rectangle: the record's paste_table word points at 256 table bytes followed by ry0, ry1, rx0, rx1 (little-endian
//   int32, WINDOW coordinates of the unflipped window, half-open, clipped by the host; empty: ry0 == ry1).
//   select: ptab[plbl[col]] && ry0 <= row < ry1 && rx0 <= col < rx1.  Kinds 0 and 2 select on the table alone.
// The row test is uniform per block row: a row outside the rectangle takes the no-paste pointers and never reads the source;
// the column test comes before the source label is read, so no byte of the source outside the rectangle is ever loaded.
// The rectangle is clamped to the window again here: the host wrapper rejects a wrong one (aug_records.h), the clamp keeps
// it from mattering.
// ONE kernel pair serves the three entries hiast_aug_geometry_u8 / _store_u8 / _mix_u8: they differ in the highest kind
// they know (max_kind 1 / 2 / 4), in whether a store is required, and in what they ask of the blob's alignment.  A record
// whose kind is above the entry's max_kind, or is a store kind while the store is null, is LEFT ALONE by both launches:
// nothing is read through its offsets, and its rows of tmp, img_out and lbl_out are not written.  (The first two entries
// used to copy such a record as if it were a finished sample, reading the blob at what may be a store offset.)
#include "aug_common.h"

namespace hiast {

constexpr int PBITS = 22;

__device__ __forceinline__ unsigned clip8(int v) { return (unsigned)clampi(v >> PBITS, 0, 255); }

// where a sample's window lies: the bytes handed over in the blob (row stride cw) or, for a store kind, a window of a
// resident frame (row stride = the frame's width, never below cw), and what its paste is confined to.  live: a planned
// sample this launch knows and can read (a store kind needs a store); finished: kind 1; anything else is left alone
struct Window {
    const uint8_t* base;
    size_t stride;
    bool live, finished, paste, boxed;
    int ry0, ry1, rx0, rx1;
};
__device__ __forceinline__ Window window_of(const int64_t* r, const uint8_t* blob, const uint8_t* store, int max_kind)
{
    Window w;
    const int64_t kind = r[R_KIND];
    const bool in_store = kind == KIND_STORE || kind == KIND_STORE_RECT;
    const bool rect = kind == KIND_PLAN_RECT || kind == KIND_STORE_RECT;
    const int64_t cw = r[R_CW];
    w.finished = kind == KIND_FINISHED;     // (every entry knows kinds 0 and 1)
    w.live = kind <= max_kind && (in_store ? store != nullptr : (kind == KIND_PLAN || kind == KIND_PLAN_RECT));
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
__global__ __launch_bounds__(256) void aug_hpass_kernel(const int64_t* __restrict__ recs, const uint8_t* __restrict__ blob,
                                                        const uint8_t* __restrict__ store, const int32_t* __restrict__ tabs,
                                                        uint8_t* __restrict__ tmp, int max_ch, int ow, int max_kind)
{
    const int64_t* r = recs + (size_t)blockIdx.z * REC;
    const Window win = window_of(r, blob, store, max_kind);
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
    if (win.boxed) {                        // uniform per sample: kinds 0 and 2 keep the loop without the column test
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
    d[0] = (uint8_t)clip8(a0);
    d[1] = (uint8_t)clip8(a1);
    d[2] = (uint8_t)clip8(a2);
}

// vertical pass (channel-agnostic: byte i of an output row is a weighted sum of byte i of the tmp rows; VEC = 4 bytes per
// thread when ow*3 is a multiple of 4) + the label gather through the same select + the copy of finished (host-augmented)
// samples
template <int VEC>
__global__ __launch_bounds__(256) void aug_vpass_kernel(const int64_t* __restrict__ recs, const uint8_t* __restrict__ blob,
                                                        const uint8_t* __restrict__ store, const int32_t* __restrict__ tabs,
                                                        const uint8_t* __restrict__ tmp,
                                                        uint8_t* __restrict__ img_out, uint8_t* __restrict__ lbl_out,
                                                        int max_ch, int oh, int ow, int max_kind)
{
    const int b = blockIdx.z, y = blockIdx.y;
    const int64_t* r = recs + (size_t)b * REC;
    const int rowb = ow * 3;
    const int q = (blockIdx.x * 256 + threadIdx.x) * VEC;
    uint8_t* dimg = img_out + ((size_t)b * oh + y) * rowb;
    uint8_t* dlbl = lbl_out + ((size_t)b * oh + y) * ow;
    const int stride = gridDim.x * 256;
    const Window win = window_of(r, blob, store, max_kind);
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
            for (int i = 0; i < VEC; ++i) v |= clip8(a[i]) << (8 * i);
            *reinterpret_cast<uint32_t*>(dimg + q) = v;
        } else {
            dimg[q] = (uint8_t)clip8(a[0]);
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

// B frames of HW pixels at offsets[b] of the store -> out float32 [B][3][HW]: K14's arithmetic (common.h)
__global__ __launch_bounds__(256) void normalize_gather_u8_kernel(const uint8_t* __restrict__ store,
                                                                  const int64_t* __restrict__ offsets, float* __restrict__ out,
                                                                  long long HW, float m0, float m1, float m2, float s0, float s1,
                                                                  float s2)
{
    const int b = blockIdx.y;
    const int64_t off = offsets[b];
    normalize_image_u8(store + (off < 0 ? 0 : off), out + (size_t)b * 3 * HW, HW, m0, m1, m2, s0, s1, s2);
}

}  // namespace hiast

// the two launches of the geometry pass for records of kinds 0..max_kind (store kinds only with a store); blob_align: 1, or 4
// for an entry that reads rectangles (int32) from the blob
static int aug_geometry_launch(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs, uint8_t* tmp,
                               uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow, int max_kind,
                               int blob_align, hiast_stream_t stream)
{
    if (!recs || !blob || !tabs || !tmp || !img_out || !lbl_out) return HIAST_E_ARG;
    if (B <= 0 || max_ch <= 0 || oh <= 0 || ow <= 0) return HIAST_E_ARG;
    if (B > 65535 || max_ch > 65535 || oh > 65535 || ow > (1 << 20)) return HIAST_E_RANGE;
    if ((((uintptr_t)blob) & (uintptr_t)(blob_align - 1)) != 0) return HIAST_E_ARG;
    hipLaunchKernelGGL(hiast::aug_hpass_kernel, dim3((ow + 255) / 256, max_ch, B), dim3(256), 0, (hipStream_t)stream, recs,
                       blob, store, tabs, tmp, max_ch, ow, max_kind);
    HIAST_CHECK_LAUNCH();
    const int rowb = ow * 3;
    if (rowb % 4 == 0 && ((((uintptr_t)tmp) | ((uintptr_t)img_out) | ((uintptr_t)blob)) & 3) == 0)
        hipLaunchKernelGGL(hiast::aug_vpass_kernel<4>, dim3((rowb / 4 + 255) / 256, oh, B), dim3(256), 0, (hipStream_t)stream,
                           recs, blob, store, tabs, tmp, img_out, lbl_out, max_ch, oh, ow, max_kind);
    else
        hipLaunchKernelGGL(hiast::aug_vpass_kernel<1>, dim3((rowb + 255) / 256, oh, B), dim3(256), 0, (hipStream_t)stream,
                           recs, blob, store, tabs, tmp, img_out, lbl_out, max_ch, oh, ow, max_kind);
    HIAST_CHECK_LAUNCH();
    return 0;
}

extern "C" int hiast_aug_geometry_u8(const int64_t* recs, const uint8_t* blob, const int32_t* tabs, uint8_t* tmp,
                                     uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                                     hiast_stream_t stream)
{
    return aug_geometry_launch(recs, blob, nullptr, tabs, tmp, img_out, lbl_out, B, max_ch, oh, ow, hiast::KIND_FINISHED, 1, stream);
}

extern "C" int hiast_aug_geometry_store_u8(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs,
                                           uint8_t* tmp, uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                                           hiast_stream_t stream)
{
    if (!store) return HIAST_E_ARG;
    return aug_geometry_launch(recs, blob, store, tabs, tmp, img_out, lbl_out, B, max_ch, oh, ow, hiast::KIND_STORE, 1, stream);
}

extern "C" int hiast_aug_geometry_mix_u8(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs,
                                         uint8_t* tmp, uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                                         hiast_stream_t stream)
{
    return aug_geometry_launch(recs, blob, store, tabs, tmp, img_out, lbl_out, B, max_ch, oh, ow, hiast::KIND_STORE_RECT, 4,
                               stream);      // (store may be null)
}

extern "C" int hiast_normalize_gather_u8(const uint8_t* store, const int64_t* offsets, float* out, int B, int64_t HW,
                                         const float* mean, const float* std, hiast_stream_t stream)
{
    if (!store || !offsets || !out || !mean || !std) return HIAST_E_ARG;
    if (B <= 0 || HW <= 0) return HIAST_E_ARG;
    if (B > 65535) return HIAST_E_RANGE;
    long long nb = (HW + 256 * 4 - 1) / (256 * 4);
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    hipLaunchKernelGGL(hiast::normalize_gather_u8_kernel, dim3((unsigned)nb, B), dim3(256), 0, (hipStream_t)stream, store,
                       offsets, out, (long long)HW, mean[0], mean[1], mean[2], std[0], std[1], std[2]);
    HIAST_CHECK_LAUNCH();
    return 0;
}
