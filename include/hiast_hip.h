/*
 * hiast_hip.h — C ABI of libhiast_hip.so, the MI355X (gfx950) kernels behind HIAST's
 * self-training hot path.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into caller-owned memory unless marked "host";
 *     the library never allocates, frees or keeps a pointer after the call returns;
 *   - head-side tensors (logits, probabilities, ASPP I/O of K1, fp32 BN of K10, K2-K8, K15, K16) are contiguous
 *     NCHW fp32; the trunk kernels (K1b, K9, K9c, K9d, K10b) take CHANNELS-LAST rows [B,H,W,C] in fp32, bf16 or
 *     bf16 split planes (hi|lo slabs) as stated per entry point; label maps are uint8 or int64 (is_i64 flag);
 *   - calls only ENQUEUE work on `stream` (a hipStream_t passed as void*); they never
 *     synchronise the device, so a caller's DDP/compute overlap is preserved;
 *   - return value: 0 = ok, <0 = argument error (HIAST_E_*), >0 = a hipError_t;
 *   - thread-safe for distinct streams; the only state is the tuning environment (read once), the thread-local
 *     co-scheduling hint (hiast_igemm_set_cosched) and the process-wide CU reserve (hiast_set_reserve_cus).
 *
 * Each entry point cites the reference call it stands in for (paths under
 * bupt-ai-cz/HIAST `code/`).  The reference has no native code: these replace
 * torch/cuDNN/numpy calls made from its Python.
 */
#ifndef HIAST_HIP_H
#define HIAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIAST_ABI_VERSION 6

#define HIAST_E_ARG   (-1) /* null pointer / non-positive extent */
#define HIAST_E_RANGE (-2) /* extent outside what the kernels are built for */
#define HIAST_E_WS    (-3) /* workspace too small */

/* fp16 bit patterns 0x0000..0x3C00 (0.0 .. 1.0): one histogram bin per representable
 * fp16 confidence value; reproduces `probs.astype(np.float16)` exactly
 * (workflows/pseudo_label_generator.py:201). */
#define HIAST_NBINS 15361
/* Σ max-prob is accumulated exactly as an integer: prob * 2^30 (prob >= 2^-7). */
#define HIAST_PROB_FX_SHIFT 30
#define HIAST_MAX_CLASSES 32
/* Operand formats of the 16-bit channels-last kernels (K9c-K9e, K10b, K1b, K18; the `fmt` arguments below):
 *   HIAST_FMT_BF16        rows of bf16 values (slab = 64 channels)
 *   HIAST_FMT_SPLIT_BF16  fp32-class values as bf16 hi|lo planes (slab = 32 channels; inference only)
 *   HIAST_FMT_FP16        rows of IEEE fp16 values — the type the reference trains in under apex O1
 *                         (code/utils/default_config.py:109, code/utils/utils.py:126-132)
 * bf16 and fp16 rows share every layout and kernel structure; the matrix cores run both at the same rate. */
#define HIAST_FMT_BF16 1
#define HIAST_FMT_SPLIT_BF16 2
#define HIAST_FMT_FP16 3
#define HIAST_IGNORE 255

typedef void* hiast_stream_t;

int hiast_version(void);
/* host: static string for a negative HIAST_E_* code, "hip error" otherwise */
const char* hiast_error_string(int code);

/* ---- device geometry and the CU reserve (ABI 6; host) -------------------------------------------------------------------
 * Stands in for nothing in the reference (apex / NCCL on NVSwitch hardware has no such knob): under DDP + SyncBN
 * (code/workflows/trainer/base_trainer.py:43-56, code/utils/utils.py:103-105) 208 chained [C,2] all-reduces per step each need a
 * free compute unit for RCCL's kernel while the side streams keep every CU busy with 60-160 us tile-kernel blocks.
 * hiast_device_cus(): compute units of the current device (hipDeviceGetAttribute; 0 when no device is visible).
 * hiast_set_reserve_cus(n): from now on every one-block-per-CU / persistent launch of this library (xconv*, stem*, pass 1,
 *   weight-gradient work splits) sizes its grid to CUs - n (n is rounded up to a multiple of 8, one per XCD; n <= CUs / 2);
 *   returns the previous value.  Process-wide; call it once before the first launch (work splits, i.e. partial-sum row counts
 *   and summation orders, depend on it).
 * hiast_stream_create_reserved(&s, n): a stream on which NO kernel (ours or torch's) can be placed on n of the CUs (queue CU
 *   mask, hipExtStreamCreateWithCUMask; n / 8 CUs of every XCD) — what keeps the non-persistent tile kernels off them.
 *   Destroy with hiast_stream_destroy. */
int hiast_device_cus(void);
int hiast_set_reserve_cus(int n);
int hiast_get_reserve_cus(void);
int hiast_stream_create_reserved(hiast_stream_t* out, int reserve);
int hiast_stream_destroy(hiast_stream_t s);

/* ---- K2: bilinear upsample, align_corners=True ------------------------------------
 * F.interpolate(logits, size, mode='bilinear', align_corners=True):
 *   sseg/models/segmentors/self_training_segmentor.py:27, source_only_segmentor.py:19,
 *   workflows/validator.py:45,52, workflows/trainer/base_trainer.py:169,171.
 * in [B,C,h,w] -> out [B,C,H,W].  bwd is the exact adjoint (gin overwritten). */
int hiast_upsample_bilinear_ac_fwd(const float* in, float* out, int B, int C, int h, int w,
                                   int H, int W, hiast_stream_t stream);
int hiast_upsample_bilinear_ac_bwd(const float* gout, float* gin, int B, int C, int h, int w,
                                   int H, int W, hiast_stream_t stream);

/* ---- K3: pseudo-label pass 1 -------------------------------------------------------
 * F.softmax(logits,1).max(1) on the upsampled logits + the per-class fp16 confidence
 * lists of workflows/pseudo_label_generator.py:192-201, as one fused kernel:
 * logits_lr [B,C,h,w] (low-res head output; h==H,w==W accepted) ->
 *   maxprob f32 [B,H,W], argmax u8 [B,H,W] (first max on ties),
 *   hist u32 [C,HIAST_NBINS] += count of pixels of class c whose fp16(maxprob) has
 *   bit pattern `bin` (caller zeroes hist; bins accumulate across calls).
 * workspace (optional, hiast_plabel_pass1_workspace_bytes(C) bytes, 4-byte aligned, private to
 * the call until the stream has passed it): the kernel counts into a scattered copy of the
 * histogram there (hot counters on different memory lines) and a second launch adds it into
 * hist; NULL = count straight into hist (same sums, slower on peaked class distributions). */
size_t hiast_plabel_pass1_workspace_bytes(int C);
int hiast_plabel_pass1(const float* logits_lr, int B, int C, int h, int w, int H, int W,
                       float* maxprob, uint8_t* argmax, uint32_t* hist, void* workspace,
                       size_t workspace_bytes, hiast_stream_t stream);

/* ---- K4: pseudo-label pass 2 -------------------------------------------------------
 * BasePseudoGenerator.select_and_save_confident_label, pseudo_label_generator.py:67-105:
 *   plbl = argmax; plbl[maxprob < thr[argmax]] = 255; per-image per-class pixel counts;
 *   per-class Σ maxprob over kept pixels.
 * thr_up f32 [C] = smallest float32 >= the float64 threshold (so the fp32 compare equals
 * the reference's float32<float64 compare); NULL = no threshold ('NT' policy).
 * count i64 [B,C] and sumprob_fx u64 [C] (Σ prob*2^30, exact) are ACCUMULATED (caller zeroes). */
int hiast_plabel_pass2(const float* maxprob, const uint8_t* argmax, const float* thr_up,
                       int B, int C, int64_t HW, uint8_t* plbl, int64_t* count,
                       uint64_t* sumprob_fx, hiast_stream_t stream);

/* ---- K3b: CBST confidence sample -------------------------------------------------------
 * CBSTPseudoGenerator.get_constant_threshold, workflows/pseudo_label_generator.py:142-158:
 *   for c: tmp = probs_pred[lbls_pred == c].astype(float16); list_c.extend(tmp[0:len(tmp):interval])
 * over ONE batch: maxprob f32 [N], argmax u8 [N] (N = B*H*W, raster order) -> hist u32 [C,HIAST_NBINS] += the
 * kept pixels' fp16 bins (pixel kept iff (rank_offset[c] + its rank among the batch's class-c pixels) % interval == 0).
 * rank_offset i64 [C] or NULL (= 0): class-c pixels of this global batch held by lower ranks (sharded generation);
 * class_total i64 [C] or NULL: out, the batch's per-class pixel counts.  workspace: device scratch of
 * hiast_plabel_strided_hist_workspace_bytes(N, C). */
size_t hiast_plabel_strided_hist_workspace_bytes(int64_t N, int C);
int hiast_plabel_strided_hist(const float* maxprob, const uint8_t* argmax, int64_t N, int C, int interval,
                              const int64_t* rank_offset, int64_t* class_total, uint32_t* hist,
                              void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K16: multi-scale + flip test-time augmentation, fused tail -------------------------
 * Validator.get_multi_scale_and_flip_logits + argmax, workflows/validator.py:34-55,92, from the LOW-RES head outputs:
 *   out = sum_s interp( softmax(interp(z[s] -> Hs[s] x Ws[s])) + flip_w(softmax(interp(zf[s] -> ...))) -> H x W )
 * z, zf: HOST arrays of n_scales device pointers to [B,C,hs[s],ws[s]] fp32 (zf NULL = no flip; a zf with a NULL
 * entry is HIAST_E_ARG); hs, ws, Hs, Ws: host int arrays.  probsum f32 [B,C,H,W] and/or label u8 [B,H,W] (either may be NULL):
 * neither full-resolution logits nor per-scale probability maps are stored. */
#define HIAST_TTA_MAX_SCALES 8
int hiast_tta_fused(const float* const* z, const float* const* zf, const int* hs, const int* ws, const int* Hs,
                    const int* Ws, int n_scales, int B, int C, int H, int W, float* probsum, uint8_t* label,
                    hiast_stream_t stream);

/* ---- K3c: pseudo-label pass 1 over several views (multi-scale + flip) -------------------
 * K16's view averaging with K3's outputs, from the LOW-RES head outputs of every (scale, flip) forward.
 * z, zf, hs, ws, Hs, Ws as for hiast_tta_fused (zf NULL = no mirror views; a zf with a NULL entry is HIAST_E_ARG).
 * Per native pixel:
 *   tot[c]  = the per-class probability sum of hiast_tta_fused (same operations in the same order)
 *   argmax  = the first class with the largest tot[c]                      (the validator's label)
 *   n_views = n_scales * (zf ? 2 : 1)
 *   maxprob = fminf(tot[argmax] / (float)n_views, 1.0f)                    (IEEE fp32 division: the mean probability over the
 *             views; the sum can exceed n_views by rounding — the clamp keeps the fp16 bin at most 0x3C00, the last one)
 *   hist[argmax][fp16 bits of maxprob] += 1                                (bins < HIAST_NBINS, as pass 1)
 * -> maxprob f32 [B,H,W], argmax u8 [B,H,W], hist u32 [C,HIAST_NBINS] accumulated.  C in {19, 16, 9, 2}.
 * workspace (optional, hiast_plabel_pass1_tta_workspace_bytes(C) bytes, 4-byte aligned, zeroed by the call): the scattered
 * counting copy of pass 1 plus a merge launch; NULL = count straight into hist. */
size_t hiast_plabel_pass1_tta_workspace_bytes(int C);
int hiast_plabel_pass1_tta(const float* const* z, const float* const* zf, const int* hs, const int* ws, const int* Hs,
                           const int* Ws, int n_scales, int B, int C, int H, int W, float* maxprob, uint8_t* argmax,
                           uint32_t* hist, void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K5-K8: fused self-training loss ------------------------------------------------
 * SelfTrainingSegmentor.compute_loss, self_training_segmentor.py:30-53 with
 * losses.py:32-36 (CE), :39-65,75-89 (SoftCE on a region), _kld :153-163, _entropy :140-150,
 * consuming LOW-RES student logits (and low-res teacher logits; the bilinear upsample of
 * forward() and the teacher softmax of consistency_self_training_trainer.py:113-119 are
 * recomputed in-kernel, never materialised).
 *
 * sums f64 [8] (overwritten): 0 Σ_conf -logp[y]   1 Σ_conf Σ_c -logp_c/C   2 Σ_ign Σ_c -p_c logp_c
 *   3 Σ_region Σ_c -q_c logp_c   4 N_conf   5 N_ign   6 #(q_c * -logp_c != 0 in region)   7 unused
 * The reference's losses are then  w_t*s0/s4, w_k*s1/(C*s4), w_e*s2/(C*s5), w_c*s3/s6
 * (0/0 = NaN, as in the reference).
 * region: 0 'ignored' (plbl==255), 1 'confident', 2 'all' (losses.py:77-82).
 * teacher_lr may be NULL (no consistency term; s3 = s6 = 0).
 * plbl: uint8 or int64 [B,H,W] (is_i64).  A label outside [0, C) + {255} is NOT detected: it counts as confident (slot 4)
 *   and matches no class (its -logp[y] is lse, its CE gradient p_c).
 * workspace: hiast_st_loss_workspace_bytes(...) bytes of scratch.
 * Geometry: the entries upsample, H >= h and W >= w are required (HIAST_E_RANGE otherwise), B <= 65535 and h <= 65535 (grid
 *   limits).  The backward gives every output column of a block of TI low-res cells one of its 256 threads, so each block
 *   must stay within 256 columns: with sw = (w - 1) / (W - 1) in float32, TI = min(max(int(253 sw), 1), 253, w) and
 *   TI / sw + 2 <= 256 (w = 1: W <= 256) — about W - 1 <= 254 (w - 1), the largest W for w = 1 .. 9 being 256, 255, 509, 763,
 *   1017, 1271, 1525, 1779, 2033.  hiast_st_loss_workspace_bytes(...) == 0 IS the test: it returns 0 exactly for the
 *   geometries both entries refuse with HIAST_E_RANGE (H < h and W < w among them), never for positive extents they accept.  Class counts
 *   other than 19, 16, 9, 2 are HIAST_E_RANGE.  A refused call launches nothing and writes nothing.
 *
 * The consistency term is pluggable, as cfg.cst_training.cst_loss.type of the reference (losses.py:9-41): the
 * hiast_st_loss_cst_* entries take cst_kind; hiast_st_loss_fwd / _bwd are their cst_kind = 0 call.  With z the upsampled
 * student logits, logp their log-softmax, zt the upsampled teacher logits, q1 = softmax(zt) in fp32, slots 3 and 6 hold
 *   HIAST_CST_SOFTCE 0: s3 = Σ_region Σ_c -q1_c logp_c, s6 = #(non-zero products)                      (as above)
 *   HIAST_CST_CE     1: l = lse(z) - z[yt] per pixel, yt = arg-max_c zt (the first maximum); s3 = Σ_pixels l M,
 *                       s6 = Σ_pixels (l != 0 ? M : 0), M = the number of images of the batch whose region mask holds at
 *                       this pixel position.  This is the reference's behaviour: it multiplies the [B,H,W] per-pixel loss
 *                       by the [B,1,H,W] mask, which broadcasts to [B,B,H,W] (out[i,j] = l[j] mask[i], losses.py:86-87),
 *                       so image j contributes wherever M > 0, whether or not its own pixel is in the region.
 *   HIAST_CST_KLDIV  2: s3 = Σ_region Σ_c q_c (log q_c - logp_c) with q = softmax(q1), s6 = #(non-zero products).  The
 *                       double softmax is the reference's behaviour: its trainer hands over probabilities and
 *                       LOSS['KLDIV'] applies a softmax to its target again (losses.py:21-23).
 *   HIAST_CST_MSE    3: s3 = Σ_region Σ_c (z_c - q1_c)^2 on the RAW student logits (the reference applies no softmax to
 *                       the student, losses.py:9-13), s6 = #(non-zero squares).
 * Slots 0-2, 4, 5 do not depend on the kind; the loss is w_c*s3/s6 for every kind.  The gradients of the term are
 * A4 (p_c Σq1 - q1_c), A4 M (p_c - [c == yt]), A4 (p_c Σq - q_c), A4 2 (z_c - q1_c) with A4 = coef[3] / s6.
 * cst_kind outside 0..3: HIAST_E_RANGE; a kind other than 0 with teacher_lr == NULL: HIAST_E_ARG (nothing is launched). */
#define HIAST_CST_SOFTCE 0
#define HIAST_CST_CE 1
#define HIAST_CST_KLDIV 2
#define HIAST_CST_MSE 3
size_t hiast_st_loss_workspace_bytes(int B, int C, int h, int w, int H, int W);
int hiast_st_loss_fwd(const float* logits_lr, const float* teacher_lr, const void* plbl,
                      int plbl_is_i64, int B, int C, int h, int w, int H, int W, int region,
                      double* sums, void* workspace, size_t workspace_bytes,
                      hiast_stream_t stream);
/* d(Σ_i coef_i * loss_i)/d logits_lr, with the loss_i normalised as above.
 * coef f32 [4] (device) = grad_output_i * weight_i for (CE, KLD, ENT, CST).
 * dlogits_lr [B,C,h,w] is overwritten.
 * The factor of term i is A_i = (float)((double)coef_i / denominator_i), and exactly 0 when coef_i == 0 — so a loss whose
 * denominator is 0 (no confident pixel: s4; no ignored pixel: s5; an empty region: s6) leaves the gradient finite as long as
 * its coef is 0.  A zero denominator with a non-zero coef gives A_i = ±inf: every cell the term reaches is then NaN (0 · inf)
 * or ±inf, as the reference's 0/0 loss would make it. */
int hiast_st_loss_bwd(const float* logits_lr, const float* teacher_lr, const void* plbl,
                      int plbl_is_i64, int B, int C, int h, int w, int H, int W, int region,
                      const double* sums, const float* coef, float* dlogits_lr,
                      void* workspace, size_t workspace_bytes, hiast_stream_t stream);
/* the same pair with the consistency kind as an argument (HIAST_CST_*, see above) */
int hiast_st_loss_cst_fwd(const float* logits_lr, const float* teacher_lr, const void* plbl,
                          int plbl_is_i64, int B, int C, int h, int w, int H, int W, int region, int cst_kind,
                          double* sums, void* workspace, size_t workspace_bytes, hiast_stream_t stream);
int hiast_st_loss_cst_bwd(const float* logits_lr, const float* teacher_lr, const void* plbl,
                          int plbl_is_i64, int B, int C, int h, int w, int H, int W, int region, int cst_kind,
                          const double* sums, const float* coef, float* dlogits_lr,
                          void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K1: ASPP head, 4 dilated 3x3 convs summed --------------------------------------
 * ASPP_V2.forward, sseg/models/modules/seg_models/deeplab_v2.py:20-24 (+ autograd):
 *   y = Σ_{i<4} conv3x3(x; W_i, b_i, dilation=dil[i], padding=dil[i]).
 * x [B,Cin,h,w]; W_i [Cout,Cin,3,3]; b_i [Cout]; y [B,Cout,h,w]; Cin % 64 == 0, Cout <= 32.
 * The 36 taps collapse to 33 (the 4 centre taps share one input pixel and are pre-summed).
 * wpack: hiast_aspp_wpack_bytes() scratch written by hiast_aspp_pack_weights (repacked
 * [33][Cin][32] weights + summed bias) and read by fwd / bwd_data; dil: host int[4].
 * workspace: hiast_aspp_workspace_bytes() scratch (split-K partial sums, fixed-order reduce:
 * results are bitwise reproducible; no float atomics).
 * One image (Cin*h*w values) must stay below 2^31 elements; the forward with Cout <= 19 addresses it with 32-bit BYTE
 * offsets and refuses an image above 2^31 bytes (HIAST_E_RANGE, before the workspace is looked at). */
size_t hiast_aspp_wpack_bytes(int Cin, int Cout);
size_t hiast_aspp_workspace_bytes(int B, int Cin, int h, int w, int Cout);
int hiast_aspp_pack_weights(const float* w0, const float* w1, const float* w2, const float* w3,
                            const float* b0, const float* b1, const float* b2, const float* b3,
                            int Cin, int Cout, float* wpack, hiast_stream_t stream);
int hiast_aspp_fwd(const float* x, const float* wpack, float* y, int B, int Cin, int h, int w,
                   int Cout, const int* dil, void* workspace, size_t workspace_bytes,
                   hiast_stream_t stream);
/* dx [B,Cin,h,w] overwritten */
int hiast_aspp_bwd_data(const float* dy, const float* wpack, float* dx, int B, int Cin, int h,
                        int w, int Cout, const int* dil, hiast_stream_t stream);
/* dW_i [Cout,Cin,3,3] and db [Cout] (the same bias gradient for every branch) overwritten */
int hiast_aspp_bwd_weight(const float* x, const float* dy, float* dw0, float* dw1, float* dw2,
                          float* dw3, float* db, int B, int Cin, int h, int w, int Cout,
                          const int* dil, void* workspace, size_t workspace_bytes,
                          hiast_stream_t stream);

/* ---- K1b: the same ASPP head on CHANNELS-LAST activations, as one GEMM + a 33-tap shift-add ------------
 * (deeplab_v2.py:20-24 + autograd, as K1).  T[p][tap*Cout+co] = Σ_ci x[p][ci]*W[tap][co][ci] is a plain
 * [B*h*w x Cin] x [Cin x NP] GEMM on the bf16 matrix cores (NP = hiast_aspp2_np(Cout) = 33*Cout rounded up to
 * 128), y[co][q] = bias[co] + Σ_tap T[q+off(tap)][tap*Cout+co]: the feature map is read once instead of 33x.
 * x_nhwc [B,h,w,Cin]; dtype 0 = fp32 rows (split-bf16 arithmetic on the fly), 2 = split planes (K9c format; both
 * fp32-class: the pseudo-label forward), 1 = bf16 (training step under mixed precision; the reference trains under
 * apex O1).  y [B,Cout,h,w] fp32 (NCHW, what the loss / pseudo-label kernels read).  Cin % 128 == 0, Cout <= 32.
 * pack: wt [NP][Cin] fp32, wd [Cin][NP] fp32 (its transpose; may be NULL), bias [Cout].  fwd takes wt itself for
 * dtype 0 and hiast_pack_conv_weight(wt, NP, Cin, 1, planes = dtype) for dtype 1 | 2; bwd takes
 * hiast_pack_conv_weight(wd, Cin, NP, 1, 1).
 * bwd (bf16 x only): dy [B,Cout,h,w] fp32 -> dx_nhwc [B,h,w,Cin] bf16 (NULL = skip), dW_i [Cout,Cin,3,3] fp32 and
 * db [Cout] (all NULL = skip); fp32 accumulation, pixel-range split with a fixed-order reduce (bitwise
 * reproducible, no float atomics).  workspace: hiast_aspp2_workspace_bytes(..., backward) bytes. */
int hiast_aspp2_np(int Cout);
size_t hiast_aspp2_workspace_bytes(int B, int Cin, int h, int w, int Cout, int backward);
int hiast_aspp2_pack_weights(const float* w0, const float* w1, const float* w2, const float* w3,
                             const float* b0, const float* b1, const float* b2, const float* b3, int Cin,
                             int Cout, float* wt, float* wd, float* bias, hiast_stream_t stream);
int hiast_aspp2_fwd(const void* x_nhwc, int dtype, const void* wt, const float* bias, float* y, int B, int Cin,
                    int h, int w, int Cout, const int* dil, void* workspace, size_t workspace_bytes,
                    hiast_stream_t stream);
int hiast_aspp2_bwd(const void* x_nhwc, const float* dy, const void* wd, void* dx_nhwc, float* dw0, float* dw1,
                    float* dw2, float* dw3, float* db, int B, int Cin, int h, int w, int Cout, const int* dil,
                    int fmt /* HIAST_FMT_BF16 | HIAST_FMT_FP16: type of x, dx (and of the gathered dY) */,
                    void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K10: BatchNorm2d (+ residual) (+ ReLU), fused ----------------------------------------
 * The conv -> BN -> ReLU / conv -> BN -> (+identity) -> ReLU chains of Bottleneck.forward,
 * sseg/models/modules/resnet.py:78-98 (separate BN / add / ReLU passes in the reference).  "Frozen" BN still
 * uses BATCH statistics in train() mode (utils/utils.py:60-65).
 * x, res, y, dy, dx, dres: [B,C,HW] contiguous, dtype 0 = fp32, 1 = bf16; gamma/beta/statistics fp32 [C]
 * (gamma/beta may be NULL = 1/0).  `part` = per-plane partial sums, double [C][npart][2]; between the
 * stats call and the apply call the caller may sum `part` across ranks (SyncBN) — then pass the summed
 * buffer with npart planes and the GLOBAL element count.
 *   hiast_bn_stats        : part[c][n] = (Σx, Σx²) of plane (n,c)            (npart = B)
 *   hiast_bn_act_apply    : y = relu?(x*scale_c + shift_c (+res));  part == NULL -> inference (running
 *                           statistics), else training: mean/var from part/count, writes save_mean /
 *                           save_invstd [C] and updates running_mean/var (momentum, unbiased variance;
 *                           running_* may be NULL).
 *   hiast_bn_act_bwd_stats: g = dy*(y>0 if relu); part[c][n] = (Σg, Σ g*xhat)
 *   hiast_bn_act_bwd_apply: dx = gamma*invstd*(g - Σg/count - xhat*Σ(g*xhat)/count); dres = g (nullable);
 *                           dgamma = Σ g*xhat, dbeta = Σg (nullable). */
size_t hiast_bn_workspace_bytes(int B, int C);
int hiast_bn_stats(const void* x, int B, int C, int64_t HW, int dtype, double* part, hiast_stream_t stream);
int hiast_bn_act_apply(const void* x, const void* res, void* y, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, const double* part, int npart, double count,
                       float momentum, float eps, int relu, float* save_mean, float* save_invstd, int B, int C,
                       int64_t HW, int dtype, hiast_stream_t stream);
int hiast_bn_act_bwd_stats(const void* dy, const void* y, const void* x, const float* save_mean,
                           const float* save_invstd, int relu, int B, int C, int64_t HW, int dtype,
                           double* part, hiast_stream_t stream);
int hiast_bn_act_bwd_apply(const void* dy, const void* y, const void* x, const float* gamma,
                           const float* save_mean, const float* save_invstd, const double* part, int npart,
                           double count, int relu, void* dx, void* dres, float* dgamma, float* dbeta, int B,
                           int C, int64_t HW, int dtype, hiast_stream_t stream);

/* ---- K9 (round 1): BN(eval) (+ ReLU) on channels-last rows ------------------------------------------------------------
 * hiast_bn_act_nhwc_infer: y[m][c] = act(x[m][c]*scale_c + shift_c) behind the library 7x7 stem of the inference forwards
 * (sseg/models/modules/resnet.py:177-184) when the fused stem kernels do not apply.  dtype 0: fp32 rows, 1: bf16 rows.
 * (Round 5: the round-1 convolution entries this block used to declare, hiast_conv1x1_bn_act_nhwc / hiast_conv3x3_bn_act_nhwc,
 * had no product caller since hiast_igemm_bn_act (K9c) took every trunk convolution and were REMOVED from the ABI; their
 * translation unit keeps the fp32-row GEMM behind hiast_aspp2_fwd.) */
int hiast_bn_act_nhwc_infer(const void* x, void* y, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, int relu, int64_t M, int C, int dtype,
                            hiast_stream_t stream);

/* ---- K9c: the same fused trunk convolutions with operands pre-split into bf16 planes and staged by LDS-DMA ------
 * (resnet.py:78-98 as K9).  An fp32-class activation row of C values is stored as [hi_0..hi_{C-1} | lo_0..lo_{C-1}]
 * bf16 (hi = bf16(v), lo = bf16(v - hi); 4 bytes per value like fp32): x [B,H,W,planes,Cin], y [B,Ho,Wo,planes,Cout],
 * res like y.  planes = 2: hi*hi + lo*hi + hi*lo on the bf16 matrix cores (fp32-class, the pseudo-label forward);
 * planes = 1: plain bf16.  The split is done once by the producer's epilogue instead of by every consumer block.
 * wp: packed bf16 [Cout][taps][planes*Cin] from hiast_pack_conv_weight (w: torch layout [Cout][Cin][taps], taps = 1 | 9;
 * transpose = 1 packs the ADJOINT convolution's weight [Cin][taps flipped][planes*Cout] into wp: running the same kernel
 * on dY with it is the data gradient of a stride-1 convolution — autograd of nn.Conv2d in resnet.py:78-98;
 * transpose = 2 writes the forward weight to wp AND the adjoint to wpt in one pass; wpt is unused otherwise).
 * taps = 9: padding = dilation, stride 1 | 2.  out_f32 = 1: y is fp32 [B,Ho,Wo,Cout] (no residual).  mean == NULL: no
 * BatchNorm (plain GEMM).  Cin % 32 == 0, Cout % 64 == 0, every tensor < 2 GiB, 16-byte aligned.
 * hiast_split_planes: fp32 [M][C] <-> planes [M][2][C] (inverse = 1: x is written; hi + lo is exact in fp32).
 * stats (planes = 1, 16-bit output, no res, relu = 0; may be NULL): [ceil(B*Ho*Wo/256)][Cout][2] fp32, per 256-row block the sums
 * Σy and Σy² of the stored (bf16) outputs — the BatchNorm batch statistics of the training forward come out of the
 * convolution's epilogue (hiast_bn_nhwc_stats_from_partial reduces them) instead of another pass over y.
 * res_gate (planes = 1, 16-bit output, with res and relu = 0; may be NULL): like res; the residual is then added only where res_gate > 0 — the data
 * gradient of a bottleneck's first convolution takes the ReLU-masked gradient of the identity branch (dy of the block
 * output, gated by the block output) in its epilogue instead of a masked copy + a separate add.  gate_mask = 1:
 * res_gate is the [M][Cout/8] bit mask written by hiast_bn_nhwc_apply instead of a tensor of values. */
int hiast_igemm_bn_act(const void* x, const void* wp, const float* gamma, const float* beta, const float* mean,
                       const float* var, float eps, const void* res, int relu, void* y, int B, int H, int W, int Cin,
                       int Cout, int taps, int stride, int dil, int fmt /* HIAST_FMT_*: "planes" above = 2 for SPLIT_BF16, 1 otherwise;
                       FP16: everything said of planes = 1 with fp16 rows */, int out_f32, float* stats,
                       int stats_rows /* rows of `stats` the caller allocated = hiast_igemm_stats_rows(...) (ignored when stats is
                       NULL): the launch returns HIAST_E_ARG when the tile form it takes writes another number of rows (ABI 6;
                       never more than ceil(M / 128) rows) */,
                       const void* res_gate, int gate_mask, hiast_stream_t stream);
/* host: the co-scheduling hint of the CALLING THREAD (thread-local; ABI 6, replaces the HIAST_IGEMM_COSCHED environment
 * variable that round 5 set and unset around every forward): on != 0 = "this thread runs two launch sequences side by side
 * on two streams" — half-chip launches then keep the 256-row tile form (two of them fill the chip) instead of the 128 x 128 /
 * two-blocks-per-CU form.  on < 0 = back to the process default (HIAST_IGEMM_COSCHED, read once).  Returns the previous value
 * (-1 = default).  The hint enters hiast_igemm_stats_rows / hiast_igemm_dgrad_bn_stats_rows and the launches alike; a launch
 * checks the caller's row count against the form it takes. */
int hiast_igemm_set_cosched(int on);
/* host, A/B and tests: force the tile form of the calling thread's launches — 1 = the 128 x 128 form wherever it is instantiated,
 * 0 = never, < 0 = automatic (the HIAST_IGEMM_HALF environment variable, read once, else the measured rule).  Returns the
 * previous value. */
int hiast_igemm_set_half(int v);
/* host: number of partial-sum rows hiast_igemm_bn_act writes into `stats` [rows][Cout][2] for M = B*Ho*Wo output pixels
 * (one row per block of the kernel chosen for the shape) */
int hiast_igemm_stats_rows(int64_t M, int Cin, int Cout, int taps, int fmt);
/* Data gradient of a stride-1 trunk convolution, dA = conv(dy, adjoint weight) (wpt: hiast_pack_conv_weight with
 * transpose; Cin = channels of dy, Cout = channels of dA; bf16 channels-last rows), for the case that A = relu(bn(x)):
 * the epilogue also emits the per-block sums of that BatchNorm's backward pass, partial[rows][Cout][2] = (Σg, Σ g*xhat)
 * with g = dA where gamma*(x-mean)*invstd + beta > 0 (the stored bf16 dA), xhat = (x-mean)*invstd — what
 * hiast_bn_nhwc_bwd_stats(relu = 2) computes with one more read of dA and x.  rows = hiast_igemm_dgrad_bn_stats_rows(M, Cin, Cout, taps) (one row per block row of the tile form the launch takes);
 * hiast_bn_nhwc_stats_from_partial reduces them to the sums hiast_bn_nhwc_bwd_apply takes.  gamma / beta may be NULL
 * (1 / 0).  Replaces the autograd of conv -> bn -> relu (Bottleneck.forward, sseg/models/modules/resnet.py:78-98: cuDNN
 * data gradient + ATen batch_norm_backward reduce, each a pass of its own). */
int hiast_igemm_dgrad_bn_stats(const void* dy, const void* wpt, void* da, int B, int H, int W, int Cin, int Cout, int taps,
                               int dil, const void* bn_x, const float* gamma, const float* beta, const float* save_mean,
                               const float* save_invstd, float* partial, int partial_rows /* = hiast_igemm_dgrad_bn_stats_rows(...);
                               HIAST_E_ARG on a mismatch with the tile form the launch takes (ABI 6) */,
                               int fmt /* HIAST_FMT_BF16 | HIAST_FMT_FP16 */, hiast_stream_t stream);
int hiast_igemm_dgrad_bn_stats_rows(int64_t M, int Cin, int Cout, int taps);
/* Data gradient of the trunk's 3x3 / stride-2 / padding-1 convolution (layer2.0.conv2; autograd of nn.Conv2d in
 * Bottleneck.forward, resnet.py:78-98 — round 4, was the library's): dx [B,H,W,Cin] from dy [B,(H-1)/2+1,(W-1)/2+1,Cout]
 * and the adjoint-packed weight (hiast_pack_conv_weight, transpose = 1), 16-bit rows of format fmt. */
int hiast_igemm_dgrad_s2(const void* dy, const void* wpt, void* dx, int B, int H, int W, int Cin, int Cout, int fmt,
                         hiast_stream_t stream);
/* Data gradient of conv1 of an IDENTITY bottleneck (K = 256 -> N = 1024 in layer3) that also delivers the backward sums of the
 * PREVIOUS block's bn3 (round 4; autograd of `out = relu(bn3(conv3(out)) + identity)` followed by the next block's conv1,
 * resnet.py:78-98): dx [M][N] = dy [M][K] x wpt (adjoint packed) + res where the bit of res_gate is set (the identity
 * branch's gradient of THIS block: res = gradient of its output, res_gate = gate bits of its ReLU, [M][N/8] bytes); and
 * partial fp32 [hiast_xconv_dgrad_gated_bn_stats_rows][N][2] = per-block (Σg, Σ g*xhat) with g = stored dx where the bit of
 * bn_mask is set and xhat = (bn_x - save_mean) * save_invstd: what hiast_bn_nhwc_bwd_stats computes in a pass of its own
 * over (dx, bn_x, bn_mask).  K == 256, N % 256 == 0, M >= 4096 (else rows() returns 0: use hiast_igemm_bn_act + that pass). */
int hiast_xconv_dgrad_gated_bn_stats_rows(int64_t M, int K, int N);
int hiast_xconv_dgrad_gated_bn_stats(const void* dy, const void* wpt, const void* res, const void* res_gate, const void* bn_x,
                                     const void* bn_mask, const float* save_mean, const float* save_invstd, void* dx,
                                     float* partial, int64_t M, int K, int N, int fmt, hiast_stream_t stream);
/* hiast_pack_conv_weight: w fp32 [N][K][taps] (torch layout) -> wp [N][taps][planes*K] in operand format fmt (transpose = 0),
 * the adjoint [K][taps flipped][planes*N] (transpose = 1), or both (transpose = 2: forward in wp, adjoint in wpt; wpt is not
 * looked at otherwise).  Element (row, tap, reduction channel k) sits at ((row*taps + tap)*planes*KO) + k for one plane and at
 * + (k / 32)*64 + k % 32 for split planes, its lo half 32 elements further (KO = reduction channels of that form).  Any N, K,
 * taps > 0 and any alignment are taken; N % 64 == 0, K % 64 == 0, taps <= 9 and 16-byte aligned wp / wpt take the tiled kernel
 * (the same bits).  Split planes need whole 32-channel slabs of the reduction axis of every form written — K % 32 == 0 for
 * transpose 0 and 2, N % 32 == 0 for transpose 1 and 2 — else HIAST_E_RANGE before any launch (a ragged slab's lo half would
 * land in the next row, and behind wp for the last one). */
int hiast_pack_conv_weight(const float* w, int N, int K, int taps, int fmt, int transpose, void* wp, void* wpt,
                           hiast_stream_t stream);
int hiast_split_planes(float* x, void* planes, int64_t M, int C, int inverse, hiast_stream_t stream);
/* NaN rule of hiast_stem_eval, hiast_stem_tail, hiast_bn_act_nhwc_infer (relu = 1) and hiast_maxpool3x3s2_nhwc_fwd: a NaN
 * activation passes the ReLU (NaN < 0 is false) and takes a pooling window's maximum, as in ATen's relu and max_pool2d; every
 * other value keeps the bits it had (-0.0 behind a ReLU is +0.0). */
/* K9f hiast_stem_tail: bn1 (eval) -> ReLU -> MaxPool2d(3, stride 2, padding 1) of the stem convolution's output
 * (ResNet.forward, sseg/models/modules/resnet.py:180-184: x = conv1(x); bn1; relu; maxpool) in ONE pass, written in the
 * operand format of the trunk kernels.  x: channels-last [B,H,W,C] fp32 (dtype 0), bf16 (dtype 1) or fp16 (dtype 2); for the
 * 16-bit inputs the ReLU output is rounded to the input's type before the maximum, as a half-precision module path does.
 * out in format fmt: HIAST_FMT_SPLIT_BF16: split planes [B,Ho,Wo,2*C] (C % 32 == 0), HIAST_FMT_BF16 / HIAST_FMT_FP16: 16-bit
 * rows [B,Ho,Wo,C]; every dtype goes with every fmt.  Ho = (H-1)/2+1, Wo = (W-1)/2+1; C % 8 == 0; x and out 16-byte aligned;
 * B*H*W*C < 2^40; gamma / beta may be NULL (1 / 0).
 * Grid: ceil(B*Ho*Wo*(C/8) / 256) blocks in one pass whatever C is; above 16384 blocks the grid is capped and rounded down to
 * a multiple of need = (C/8) / gcd(256, C/8), so that a striding thread keeps its channel group.  HIAST_E_RANGE only for a C
 * whose need exceeds the cap (C/8 > 16384 with no factor of 2 to spare: no workload has one). */
int hiast_stem_tail(const void* x, int dtype /* 0 fp32 | 1 bf16 | 2 fp16 */, const float* gamma, const float* beta,
                    const float* mean, const float* var, float eps, void* out, int fmt /* HIAST_FMT_* of out */, int B, int H,
                    int W, int C, hiast_stream_t stream);
/* K9j hiast_stem_eval: the whole stem of an inference forward in ONE kernel — conv 7x7 / stride 2 / padding 3 (3 -> 64, no bias)
 * -> bn1 (eval) -> ReLU -> MaxPool2d(3, stride 2, padding 1) (ResNet.forward, sseg/models/modules/resnet.py:180-184), written in
 * the operand format of the trunk kernels; the full-resolution convolution output is never stored.
 * x: fp32 [B,3,H,W] contiguous (NCHW), w: fp32 [64,3,7,7] (nn.Conv2d layout), gamma / beta may be NULL (1 / 0);
 * out: [B,Hp,Wp,planes*64] in format fmt (HIAST_FMT_BF16 | _SPLIT_BF16 | _FP16), Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (same for W).
 * Arithmetic: fmt's 16-bit operands (split planes: hi*hi + lo*hi + hi*lo) with fp32 accumulation. */
int hiast_stem_eval(const float* x, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                    float eps, void* out, int fmt, int B, int H, int W, hiast_stream_t stream);

/* ---- K9k (round 4): the stem convolution of the TRAINING forward and its weight gradient -----------------------------------
 * `x = self.conv1(x)` of ResNet.forward in model.train() under apex O1 (sseg/models/modules/resnet.py:177-180: a half-
 * precision library convolution) and the autograd weight gradient of that nn.Conv2d (the image needs no data gradient).
 * x fp32 [B,3,H,W] NCHW contiguous, w fp32 [64,3,7,7] -> y [B,Hc,Wc,64] channels-last rows in format fmt (HIAST_FMT_BF16 |
 * HIAST_FMT_FP16; operands rounded to that type, fp32 accumulation), Hc = (H-1)/2+1, Wc = (W-1)/2+1, and partial fp32
 * [hiast_stem_train_blocks(B,H,W)][64][2]: per-block sums Σy, Σy² of the STORED values for the batch-statistics BatchNorm that
 * follows (hiast_bn_nhwc_apply_partial).  hiast_stem_wgrad: dw fp32 [64,3,7,7] from dy (rows like y) and the same x;
 * per-block partials in `workspace` (hiast_stem_wgrad_workspace_bytes), added in a fixed order: bitwise reproducible. */
int hiast_stem_train_blocks(int B, int H, int W);
int hiast_stem_train_fwd(const float* x, const float* w, void* y, float* partial, int fmt, int B, int H, int W,
                         hiast_stream_t stream);
size_t hiast_stem_wgrad_workspace_bytes(int B, int H, int W);
int hiast_stem_wgrad(const float* x, const void* dy, float* dw, int fmt, int B, int H, int W, void* workspace,
                     size_t workspace_bytes, hiast_stream_t stream);
/* hiast_pack_conv_weight for a list of weights in ONE launch (a trunk's 104 convolutions after every optimiser / EMA
 * update).  table: device array of records (mode = the `transpose` argument above; N, K multiples of 64, taps <= 9);
 * one block per 64 x 64 (n, k) tile of one weight: chunk_tensor[b] = record index, chunk_start[b] = index of the tile
 * within that weight, row-major over (N/64, K/64).  max_taps >= the largest `taps` of the records a block of this launch
 * may meet (sizes the LDS tile: list the 1x1 and the 3x3 weights in separate launches to keep the 1x1 blocks small). */
typedef struct { const float* w; void* wp; void* wpt; int32_t N, K, taps, planes /* = HIAST_FMT_* */, mode, pad; } hiast_pack_rec;
int hiast_pack_conv_weight_multi(const hiast_pack_rec* table, const int32_t* chunk_tensor, const int64_t* chunk_start,
                                 int n_chunks, int max_taps, hiast_stream_t stream);

/* ---- K9d: weight gradient of the trunk convolutions on channels-last bf16 activations -------------------------
 * autograd of nn.Conv2d in Bottleneck.forward (resnet.py:78-98) under mixed precision:
 *   dW[n][k][tap] = Σ_m dy[m][n] * x[m + off(tap)][k], bf16 operands, fp32 accumulation, fp32 result in torch's
 *   [Cout][Cin][kh][kw] layout.  dy [B,Ho,Wo,Cout], x [B,H,W,Cin] bf16; taps = 1 | 9 (padding = dilation, stride 1|2).
 * Cin % 256 == 0 and Cout % 256 == 0 (layer3 / layer4 of the trunk: 91 % of its FLOPs).  Pixel ranges are reduced in
 * a fixed order (bitwise reproducible).  workspace: hiast_conv_wgrad_workspace_bytes(...) (0 = unsupported shape). */
size_t hiast_conv_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int taps);
int hiast_conv_wgrad_nhwc(const void* dy, const void* x, float* dw, int B, int H, int W, int Cin, int Cout, int taps,
                          int stride, int dil, int fmt /* HIAST_FMT_BF16 | HIAST_FMT_FP16: type of dy and x */,
                          void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* Grouped form (round 4): the weight gradients of up to 4 convolutions — the three of one bottleneck, whose backward
 * (resnet.py:78-98 under autograd) produces their operands one after the other — in ONE launch + ONE reduction.  Each job
 * is a hiast_conv_wgrad_nhwc problem (same shape limits); the jobs share the pixel-range split, so the chip is filled
 * once (one 256 x 256 fp32 partial tile per CU) for all of them instead of once per convolution: a layer3 bottleneck
 * writes 64 MB of partials instead of 192 MB and needs 2 launches instead of 6.  `jobs` is a HOST array (read during the
 * call); results are bitwise reproducible (fixed-order reduction) but differ from the one-by-one form in summation order. */
typedef struct { const void* dy; const void* x; float* dw; int32_t B, H, W, Cin, Cout, taps, stride, dil; } hiast_wgrad_job;
size_t hiast_conv_wgrad_group_workspace_bytes(const hiast_wgrad_job* jobs, int njobs);
int hiast_conv_wgrad_group_nhwc(const hiast_wgrad_job* jobs, int njobs, int fmt, void* workspace, size_t workspace_bytes,
                                hiast_stream_t stream);

/* ---- K9h: the same weight gradient for the layers BELOW 256 channels (layer1 / layer2: Cin, Cout in {64, 128, 256, ...,
 * multiples of 128}; 1x1 (stride 1) and 3x3 (any stride, 'same' padding = dil)) — autograd of nn.Conv2d in
 * sseg/models/modules/resnet.py:78-98.  x [B,H,W,Cin], dy [B,Ho,Wo,Cout] (Ho = (H-1)/stride + 1) 16-bit channels-last rows;
 * hiast_conv_wgrad_small_workspace_bytes takes the OUTPUT map size (fmt = HIAST_FMT_BF16 /
 * _FP16), dw fp32 [Cout][Cin][kh][kw], fp32 accumulation, pixel ranges reduced in a fixed order (bitwise reproducible).
 * A strided 1x1 is this call on the subsampled input. */
size_t hiast_conv_wgrad_small_workspace_bytes(int B, int H, int W, int Cin, int Cout, int taps);
int hiast_conv_wgrad_small_nhwc(const void* dy, const void* x, float* dw, int B, int H, int W, int Cin, int Cout, int taps,
                                int stride, int dil, int fmt, void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K10b: BatchNorm2d (+ residual) (+ ReLU), TRAINING mode, on channels-last bf16 activations [M = B*H*W][C] ------
 * Same arithmetic and passes as K10 (resnet.py:78-98 in train(): batch statistics even with frozen affine
 * parameters, utils/utils.py:60-65) in the layout the convolution kernels of K9c produce / consume.
 * C a power of two in [8, 2048].  sums [C][2] double: (Σx, Σx²) forward, (Σg, Σ g*xhat) backward — all-reduce them
 * across ranks between the stats and the apply call for SyncBN.  workspace: hiast_bn_nhwc_workspace_bytes(C).
 * Every entry (hiast_bn_nhwc_stats_from_partial included) refuses any other C, 0 included, with HIAST_E_RANGE. */
size_t hiast_bn_nhwc_workspace_bytes(int C);
/* fmt (every call below): HIAST_FMT_BF16 | HIAST_FMT_FP16, the type of the activation tensors x, res, y, dy, dx, dres */
int hiast_bn_nhwc_stats(const void* x, int64_t M, int C, double* sums, void* workspace, size_t workspace_bytes, int fmt,
                        hiast_stream_t stream);
int hiast_bn_nhwc_stats_from_partial(const float* partial, int nblk, int C, double* sums, hiast_stream_t stream);
/* single-rank forward straight from the per-block partial sums (no all-reduce point): statistics + apply */
int hiast_bn_nhwc_apply_partial(const void* x, const void* res, void* y, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, const float* partial, int nblk, double count,
                                float momentum, float eps, int relu, float* save_mean, float* save_invstd, int64_t M,
                                int C, void* mask, int fmt, hiast_stream_t stream);
int hiast_bn_nhwc_apply(const void* x, const void* res, void* y, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, const double* sums, double count, float momentum,
                        float eps, int relu, float* save_mean, float* save_invstd, int64_t M, int C, void* mask, int fmt,
                        hiast_stream_t stream);
/* apply: mask (may be NULL) receives the bits y > 0, [M][C/8] bytes (bit k of byte (m, g) = channel 8g + k).
 * relu of the backward calls: 0 = no ReLU in the forward, 1 = gate y > 0 read from y, 2 = gate recomputed as
 * x*scale + shift > 0 (only when the forward had NO residual input; y may be NULL and is not read), 3 = y points to the
 * bit mask written by the forward (1/16 of y's bytes) */
int hiast_bn_nhwc_bwd_stats(const void* dy, const void* y, const void* x, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, int relu, int64_t M, int C, double* sums,
                            void* workspace, size_t workspace_bytes, int fmt, hiast_stream_t stream);
int hiast_bn_nhwc_bwd_apply(const void* dy, const void* y, const void* x, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, const double* sums, double count, int relu,
                            void* dx, void* dres, float* dgamma, float* dbeta, int64_t M, int C, int fmt,
                            hiast_stream_t stream);

/* ---- K11: EMA teacher update ---------------------------------------------------------
 * utils/utils.py:115-123 update_ema_model: ema = ema*gamma + p*(1-gamma) over a list of
 * tensors in ONE launch (gamma, one_minus_gamma: the float32 roundings of the Python
 * doubles, as torch's tensor*scalar does; mul, mul, add - no fma).  table: device array of n_tensors records
 * {float* ema; const float* p; int64 n}; chunk_tensor/chunk_start: device int32/int64
 * arrays of n_chunks entries mapping a 64Ki-element chunk to (tensor, first element). */
typedef struct { float* ema; const float* p; int64_t n; } hiast_ema_rec;
int hiast_ema_update(const hiast_ema_rec* table, const int32_t* chunk_tensor,
                     const int64_t* chunk_start, int n_chunks, float gamma,
                     float one_minus_gamma, hiast_stream_t stream);

/* ---- K18: MaxPool2d(3, stride 2, padding 1) on channels-last bf16 activations ------------------------------------
 * ResNet.forward, sseg/models/modules/resnet.py:184 (x = self.maxpool(x)) in the mixed-precision training forward, and
 * its autograd.  x, y, dy, dx: bf16 [B,H,W,C] / [B,Ho,Wo,C] (Ho = (H-1)/2+1, Wo = (W-1)/2+1), C % 8 == 0;
 * idx: one byte per output element, the position 3*dy + dx of the maximum inside its window (ATen keeps an int64 flat
 * index: 8x the bytes); first maximum in row-major window order, a NaN takes over, as ATen.  The backward gathers, for
 * every input pixel, the gradients of the <= 4 windows whose maximum it is (fp32 sum, one rounding). */
int hiast_maxpool3x3s2_nhwc_fwd(const void* x, void* y, uint8_t* idx, int B, int H, int W, int C,
                                int fmt /* HIAST_FMT_BF16 | HIAST_FMT_FP16 */, hiast_stream_t stream);
int hiast_maxpool3x3s2_nhwc_bwd(const void* dy, const uint8_t* idx, void* dx, int B, int H, int W, int C, int fmt,
                                hiast_stream_t stream);

/* ---- K14: ToTensor + Normalize on the device ------------------------------------------------------
 * transform (sseg/datasets/utils.py:37-55: torchvision ToTensor + Normalize in the DataLoader workers): img uint8
 * [B][H*W][3] (HWC as decoded) -> out float32 [B][3][H*W]; v = float(u8)/255, out = (v - mean[c])/std[c], torch's
 * operations in torch's order (bit-identical).  mean / std: HOST float[3]. */
int hiast_normalize_u8(const uint8_t* img, float* out, int B, int64_t HW, const float* mean, const float* std,
                       hiast_stream_t stream);

/* ---- K15: the per-sample data path on the device (cfg.dataset.device_aug) -----------------------------
 * augmentations.py / preprocessor.py of the reference run in DataLoader workers; here a worker hands over bytes and a
 * PLAN (every random decision, drawn on the host: hiast_amd/sseg/datasets/device_aug.py) and the device executes it,
 * byte-identical to the host code.  A batch is ONE uint8 blob, ONE int32 table blob and one int64 record row per
 * sample, all on the device; every offset counts elements of its blob:
 *   recs [B][HIAST_AUG_REC_WORDS]: kind (0 plan | 1 finished views: copied), img, lbl, paste_img, paste_lbl, paste_table
 *        (blob offsets; paste_* = -1 without CopyPaste), ch, cw (extent of the handed-over window), flip, then table
 *        offsets hlo, hn, hk, h_taps, vlo, vn, vk, v_taps (first tap / tap count / [out][taps] 22-bit fixed-point
 *        weights per output column / row: Pillow's 8-bit resample), nx, ny (nearest source index per output column / row)
 *   ops  [B][HIAST_AUG_OPS_WORDS] of ONE view: kind, blob offset of the finished view (kind 1), n_ops, 0, then
 *        (type, blob offset of a 256-entry table) x HIAST_AUG_MAX_OPS; at most one HIAST_AUG_OP_EQUALIZE per row of
 *        level-1 ops.  The rows of every level are executed by the K15b entries: a row of level-1 ops is the one segment
 *        (0, n_ops, index of its Equalize | -1, -1).
 * hiast_aug_geometry_u8: CopyPaste select on load (table[paste_lbl] ? paste : own), flipped read, horizontal pass into
 *   tmp [B][max_ch][ow][3] (rounded to uint8), vertical pass -> img_out uint8 [B][oh][ow][3]; label gather through the
 *   same select -> lbl_out uint8 [B][oh][ow].  Two launches.
 * The three geometry entries (hiast_aug_geometry_u8, _store_u8 and _mix_u8 below) run the SAME two kernels and differ in
 *   three things only: the highest record kind they know (max_kind 1, 2, 4), whether `store` may be null (no such argument,
 *   never, always) and what they ask of `blob` (any address, any address, 4-byte aligned).  A record whose kind is above
 *   the entry's max_kind, or is a store kind (2, 4) while `store` is null, is LEFT ALONE by both launches: nothing is read
 *   through its offsets, and its rows of tmp, img_out and lbl_out are not written.  The vertical pass moves 4 bytes per
 *   lane exactly when ow * 3 is a multiple of 4 and tmp, img_out and blob are 4-byte aligned, single bytes otherwise. */
#define HIAST_AUG_REC_WORDS 20
#define HIAST_AUG_MAX_OPS 8
#define HIAST_AUG_OPS_WORDS (4 + 2 * HIAST_AUG_MAX_OPS)
#define HIAST_AUG_OP_LUT 1
#define HIAST_AUG_OP_GRAY 2
#define HIAST_AUG_OP_EQUALIZE 3
int hiast_aug_geometry_u8(const int64_t* recs, const uint8_t* blob, const int32_t* tabs, uint8_t* tmp,
                          uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow, hiast_stream_t stream);

/* ---- K15 with device-resident frames (cfg.dataset.device_store_gb; hiast_amd/sseg/datasets/device_store.py) ---------
 * `store`: ONE uint8 device buffer of decoded frames (image [H][W][3] and label [H][W] each, every frame 16-byte
 * aligned), addressed by 64-bit element offsets from its base.
 * hiast_aug_geometry_store_u8: hiast_aug_geometry_u8 with a third record kind, HIAST_STORE_KIND (2): img / lbl
 *   (and paste_img / paste_lbl, or -1) are offsets INTO THE STORE of the window's first pixel — frame offset +
 *   (y1 * W + x1) * 3 for an image, + y1 * W + x1 for a label —, record word HIAST_STORE_REC_STRIDE (19, spare in the
 *   other kinds) is the frame's width W in pixels = the row stride (>= cw); paste_table and every tap / nearest table
 *   stay in blob / tabs.  The arithmetic is that of kind 0 (which reads the same window with row stride cw); kinds 0, 1
 *   and 2 may be mixed in one batch; a null `store` is HIAST_E_ARG.  hiast_aug_geometry_u8 itself knows kinds 0 and 1
 *   only (a record of kind 2 is left alone there, see K15).
 * hiast_normalize_gather_u8: hiast_normalize_u8 on B frames of HW pixels that start at store + offsets[b] (offsets:
 *   DEVICE int64 [B]) -> out float32 [B][3][HW], one launch, the same operations in the same order (bit-identical to
 *   hiast_normalize_u8 on the same bytes).  mean / std: HOST float[3].
 * Both refuse a null pointer (HIAST_E_ARG) and the extents their neighbours refuse (HIAST_E_RANGE) before any launch;
 * offsets are bounds-checked by the host wrappers (hiast_amd/kernels.py), table indices are clamped as in K15. */
#define HIAST_STORE_KIND 2
#define HIAST_STORE_REC_STRIDE 19
int hiast_aug_geometry_store_u8(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs,
                                uint8_t* tmp, uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                                hiast_stream_t stream);
int hiast_normalize_gather_u8(const uint8_t* store, const int64_t* offsets, float* out, int B, int64_t HW, const float* mean,
                              const float* std, hiast_stream_t stream);

/* ---- K15 for the mixing preprocessors (cfg.preprocessor.type: ClassMix | CutMix; hiast_amd/sseg/datasets/preprocessor.py) ---
 * Two more record kinds, a paste confined to a rectangle: HIAST_MIX_KIND_PLAN_RECT (3) = kind 0 and
 * HIAST_MIX_KIND_STORE_RECT (4) = kind 2 (HIAST_STORE_KIND), whose paste_table word points at HIAST_MIX_TABLE_BYTES
 * bytes of the blob: the 256 table bytes, then ry0, ry1, rx0, rx1 as little-endian int32 — the rectangle in the
 * coordinates of the record's (unflipped) window, half-open, clipped to [0, ch] x [0, cw]; empty: ry0 == ry1.  The offset
 * is a multiple of 4.  Kinds 0, 1 and 2 keep their bytes and their meaning.
 * hiast_aug_geometry_mix_u8: hiast_aug_geometry_store_u8 for every kind 0..4 — the same two launches, the same
 *   arithmetic; the select on load is table[paste_lbl] && ry0 <= row < ry1 && rx0 <= col < rx1 in the horizontal pass and
 *   in the label gather (kinds 0 and 2: the table alone).  A row outside the rectangle reads no byte of the paste source,
 *   a column outside it neither.  `store` may be NULL when no record is of kind 2 or 4 (such a record is then left
 *   alone).  `blob` must be 4-byte aligned (HIAST_E_ARG otherwise: the rectangle is read as int32).
 *   hiast_aug_geometry_u8 / hiast_aug_geometry_store_u8 know kinds 0..1 / 0..2 only and leave a record of a higher kind
 *   alone (K15: the unknown-kind rule).  Records live on the device, so no launch entry can REFUSE a kind: the refusal is
 *   hiast_aug_records_check on the HOST copy, which the wrappers (hiast_amd/kernels.py) call before every geometry entry
 *   with that entry's max_kind.
 * hiast_aug_records_check: HOST recs [B][HIAST_AUG_REC_WORDS] and HOST blob of blob_bytes -> 0, or HIAST_E_ARG for a kind
 *   outside 0..max_kind (max_kind: 1, 2 or 4), and for a record of kind 3 / 4 without paste offsets, whose table +
 *   rectangle is not inside the blob at a multiple of 4, or whose rectangle leaves [0, ch] x [0, cw] or has y0 > y1 or
 *   x0 > x1.  Launches nothing.
 * hiast_aug_paste_mask_u8: the copy_paste_mask of n frames of H x W in ONE launch.  prm: DEVICE int64 [n][8] = (offset
 *   of the source frame's label in the store | -1, blob offset of its 256-byte table, y0, y1, x0, x1 in FRAME
 *   coordinates, index of the frame of `out` to write, 0): out[frame][y][x] = (table[src] && y0 <= y < y1 && x0 <= x < x1)
 *   ? src : 255; a source of -1 gives 255 everywhere and reads nothing.  16 bytes per lane where the source label and
 *   the output frame are 16-byte aligned (frames of the store are), single bytes over the tail.  Offsets and frame
 *   indices are bounds-checked by the host wrapper; the rectangle is clamped to the frame.
 * The launch entries refuse a null pointer and a non-positive extent (HIAST_E_ARG) and the extents their neighbours refuse
 * (HIAST_E_RANGE) before any launch. */
#define HIAST_MIX_KIND_PLAN_RECT 3
#define HIAST_MIX_KIND_STORE_RECT 4
#define HIAST_MIX_TABLE_BYTES (256 + 16)
int hiast_aug_records_check(const int64_t* recs, const uint8_t* blob, int64_t blob_bytes, int B, int max_kind);
int hiast_aug_geometry_mix_u8(const int64_t* recs, const uint8_t* blob, const uint8_t* store, const int32_t* tabs,
                              uint8_t* tmp, uint8_t* img_out, uint8_t* lbl_out, int B, int max_ch, int oh, int ow,
                              hiast_stream_t stream);
int hiast_aug_paste_mask_u8(const int64_t* prm, const uint8_t* store, const uint8_t* blob, uint8_t* out, int n, int H, int W,
                            hiast_stream_t stream);

/* ---- K15b: the colour ops of the device-side sample path, every level -------------------------------------------
 * Level 1: LUT, OpenCV's fixed-point gray, cv2.equalizeHist (per-channel histogram -> float64 table, rint).  Level 2
 * (cfg.dataset.device_aug_level: 2): ColorJitter and GaussianBlur as plan ops.  All byte-identical to
 * hiast_amd/sseg/datasets/augmentations.py.  The level-2 op types of an ops row; the second word of the pair is
 *   HIAST_AUG_OP_CONTRAST  the bits of the float64 factor (the table is built on the device from the gray mean of the
 *                          image at that point of the chain)
 *   HIAST_AUG_OP_SAT       the bits of the float64 factor
 *   HIAST_AUG_OP_HUE       the hue shift, 0..255 (Pillow's 8-bit HSV round trip; 0 is NOT the identity)
 *   HIAST_AUG_OP_BLUR      tabs offset of the ksize float32 weights (as bits; symmetric) | ksize << 32, ksize odd in
 *                          3..HIAST_AUG_MAX_KSIZE, ksize / 2 < min(H, W)
 * The host cuts a row into segments, one launch round each: seg int32 [B][4] = (from, to, stat, blur): ops [from, to)
 * are pointwise except for at most one table op (Equalize / contrast) at index stat (-1: none); a blur at index
 * blur (-1: none) follows them.  A sample whose segment is empty is skipped.  Any number of table ops per row
 * that holds a level-2 op.  A batch of level-1 rows is one round: hiast_aug2_table_u8 only if some row has an Equalize,
 * then one hiast_aug2_colour_u8 (in != out).
 * hiast_aug2_table_u8: per sample with a table op, the histogram of `in` after ops [from, stat) (hist uint32
 *   [B][3][256], zeroed here; contrast: the gray histogram in bins 0..255) and the op's table (uint8 [B][3][256]).
 * hiast_aug2_colour_u8: ops [from, to) on in uint8 [B][HW][3] -> out.  in != out: every sample is written (finished
 *   views are copied from the blob); in == out: samples with an empty segment are not touched.
 * hiast_aug2_blur_u8: the segment's blur, in place on img uint8 [B][H][W][3] through tmp float32 [B][H][W][3]: scipy's
 *   symmetric correlate1d in float64 down the rows, then along them, reflect-101, rint.  Two launches. */
#define HIAST_AUG_OP_CONTRAST 4
#define HIAST_AUG_OP_SAT 5
#define HIAST_AUG_OP_HUE 6
#define HIAST_AUG_OP_BLUR 7
#define HIAST_AUG_MAX_KSIZE 41
int hiast_aug2_table_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const uint8_t* in, uint32_t* hist,
                        uint8_t* table, int B, int64_t HW, hiast_stream_t stream);
int hiast_aug2_colour_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const uint8_t* table,
                         const uint8_t* in, uint8_t* out, int B, int64_t HW, hiast_stream_t stream);
int hiast_aug2_blur_u8(const int64_t* ops, const int32_t* seg, const int32_t* tabs, uint8_t* img, float* tmp, int B,
                       int H, int W, hiast_stream_t stream);

/* ---- K15c: level 3 of the device-side sample path (cfg.dataset.device_aug_level: 3) ------------------------------
 * FDA (augmentations.fourier_domain_adaptation) as a plan op, in its sparse-DFT form: the output is the view plus the
 * real part of the inverse DFT of the (2 border + 1)^2 centre bins whose amplitude the target replaces,
 *   S = sum v exp(-2 pi i (ky y / H + kx x / W)),  D = (|T| - |S|) S / |S|  (phase 1 for S == 0),
 *   out = trunc(clip(v + sum_bins Re(D exp(+2 pi i ...)) / (H W), 0, 255)),
 * float64 throughout in a fixed order (device_aug.fda_u8 is the numpy restatement; bytes are equal except where the
 * value before truncation is within 1e-6 of an integer).  One further op type of an ops row:
 *   HIAST_AUG_OP_FDA       blob offset of the target view (uint8 [H][W][3], the reference image resized to the view)
 *                          | border << HIAST_AUG_FDA_BORDER_SHIFT, border 0..HIAST_AUG_FDA_MAX_BORDER, min(H, W) >= 8
 * An FDA op closes a segment as a blur does: its index stands in seg[b][3] and its launches follow the segment's
 * colour pass (hiast_aug2_blur_u8 skips a sample whose closing op is no blur, hiast_aug3_fda_u8 one whose closing op
 * is no FDA: its bytes are not touched).  Any number of FDA ops per row.
 * hiast_aug3_fda_u8: in place on img uint8 [B][H][W][3].  trig: float64 cos[H], sin[H], cos[W], sin[W] of
 *   2 pi j / n (built on the host).  ws: hiast_aug3_fda_workspace_bytes(B, H, W) bytes, 8-byte aligned.  Three launches:
 *   per (sample, view | target, band of 32 rows) the partial bin sums (rows reduced along x, then times the row factors;
 *   in the wave, then through LDS; no floating-point atomics), per sample the partials in band order and D / (H W),
 *   then the pointwise apply. */
#define HIAST_AUG_OP_FDA 8
#define HIAST_AUG_FDA_MAX_BORDER 2
#define HIAST_AUG_FDA_BORDER_SHIFT 40
size_t hiast_aug3_fda_workspace_bytes(int B, int H, int W);
int hiast_aug3_fda_u8(const int64_t* ops, const int32_t* seg, const uint8_t* blob, const double* trig, uint8_t* img,
                      double* ws, int B, int H, int W, hiast_stream_t stream);

/* K11b: copy n_tensors small tensors in one launch (the BatchNorm buffers update_ema_model copies from the student,
 * utils/utils.py:120-123).  table: device array of {dst, src, nbytes}; one block per tensor. */
typedef struct { void* dst; const void* src; int64_t nbytes; } hiast_copy_rec;
int hiast_multi_copy(const hiast_copy_rec* table, int n_tensors, hiast_stream_t stream);

/* ---- K13: Adam step ---------------------------------------------------------------------
 * torch.optim.Adam(betas, weight_decay) as built by utils/utils.py:135-154 and stepped by BaseTrainer.update_model
 * (workflows/trainer/base_trainer.py:127-141): every parameter tensor in ONE launch, torch's single-tensor
 * formulas in its operation order (L2 weight decay folded into the gradient, bias-corrected step).
 * table: device array of records {p, g, m (exp_avg), v (exp_avg_sq), n, lr, bc1 = 1-b1^t, bc2_sqrt = sqrt(1-b2^t)};
 * chunk tables as for K11. */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; float lr; float bc1; float bc2_sqrt; float step; } hiast_adam_rec;
/* ctl (may be NULL): device control block for mixed precision with dynamic loss scaling (apex amp.scale_loss /
 * torch GradScaler, base_trainer.py:129-131): a one-thread kernel ahead of the update reads the scaler's device scalars
 * grad_scale (may be NULL = 1) and found_inf (may be NULL = 0) and writes skip / 1/scale / the running count of SKIPPED
 * steps (hiast_adam_prepare: ONCE per optimiser step, before the hiast_adam_step launches of that step); the update multiplies every gradient by 1/scale and is skipped entirely (no moment update) when found_inf != 0 —
 * without the host ever reading found_inf.  With ctl the records' bc1 / bc2_sqrt are ignored: a record's `step` field is
 * the number of steps ATTEMPTED on that tensor (this one included, host-side count) and the bias corrections are formed
 * on the device from step - ctl->skipped.  Zero ctl once when the optimiser is created. */
typedef struct { float skipped; float skip; float inv_scale; float pad[5]; } hiast_adam_ctl;
int hiast_adam_prepare(hiast_adam_ctl* ctl, const float* grad_scale, const float* found_inf, hiast_stream_t stream);
int hiast_adam_step(const hiast_adam_rec* table, const int32_t* chunk_tensor, const int64_t* chunk_start,
                    int n_chunks, double beta1, double beta2, float eps, float weight_decay, const hiast_adam_ctl* ctl,
                    hiast_stream_t stream);

/* ---- K13b: SGD step ----------------------------------------------------------------------
 * torch.optim.SGD(momentum, dampening=0, nesterov=False, weight_decay) as built by utils/utils.py:140 (momentum 0.9,
 * weight decay 5e-4: the DeepLab-V2 warm-up recipe) and stepped by BaseTrainer.update_model (base_trainer.py:127-141):
 * every parameter tensor in ONE launch, torch's single-tensor formulas in its operation order, fp32, no contraction:
 *   g' = g * inv_scale;  if (wd != 0) g' = g' + wd * p;
 *   buf != NULL:  buf = buf * momentum + g';  p = p - lr * buf          buf == NULL (momentum 0):  p = p - lr * g'
 * table: device array of records {p, g, buf (momentum_buffer or NULL: no state is read or written), n, lr}; chunk tables
 * as for K11.  A new momentum buffer is zero-filled by the host: the first applied step leaves buf = g' (torch clones).
 * ctl (may be NULL): K13's control block, filled by hiast_adam_prepare once per optimiser step: inv_scale multiplies
 * every gradient, and with ctl->skip != 0 the launch returns before touching anything (SGD keeps no step count). */
typedef struct { float* p; const float* g; float* buf; int64_t n; float lr; float pad; } hiast_sgd_rec;
int hiast_sgd_step(const hiast_sgd_rec* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int n_chunks,
                   float momentum, float weight_decay, const hiast_adam_ctl* ctl, hiast_stream_t stream);

/* ---- K13c: AdamW step --------------------------------------------------------------------
 * torch.optim.AdamW(betas, eps, weight_decay) as built by utils/utils.py:144: K13 with DECOUPLED weight decay — the same
 * kernel body, instantiated with the other rule:
 *   g' = g * inv_scale;  p = p * decay;  m = m + (g' - m)*(1 - b1);  v = v*b2 + (1 - b2)*g'*g';
 *   p  = p - (lr / bc1) * (m / (sqrt(v) / bc2_sqrt + eps))
 * The record is hiast_adam_rec plus decay = float(1 - lr * weight_decay), formed in double on the host per tensor as
 * torch forms it (so the entry takes no weight_decay).  bc1 / bc2_sqrt / step and ctl: as for hiast_adam_step. */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; float lr; float bc1; float bc2_sqrt; float step; float decay; float pad; } hiast_adamw_rec;
int hiast_adamw_step(const hiast_adamw_rec* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int n_chunks,
                     double beta1, double beta2, float eps, const hiast_adam_ctl* ctl, hiast_stream_t stream);

/* ---- K15: discriminator input map (adversarial warm-up stage) -----------------------------
 * sseg/models/segmentors/adversarial_warmup_segmentor.py: F.interpolate(logits, size, bilinear,
 * align_corners=True) :36,:41 followed by D_preprocess_fun :26-29 — mode 0 = softmax(dim=1)
 * (AdaptSegNet), mode 1 = prob_2_entropy(softmax) :71-76 (AdvEnt):  -p log2(p + 1e-30) / log2(C).
 * logits_lr [B,C,h,w] -> out [B,C,H,W]; the full-resolution logits are never stored.
 * bwd: gout [B,C,H,W] -> dlogits_lr [B,C,h,w] (overwritten); scratch: B*C*H*W floats. */
int hiast_dinput_fwd(const float* logits_lr, int mode, float* out, int B, int C, int h, int w, int H, int W,
                     hiast_stream_t stream);
int hiast_dinput_bwd(const float* logits_lr, int mode, const float* gout, float* scratch, float* dlogits_lr,
                     int B, int C, int h, int w, int H, int W, hiast_stream_t stream);

/* ---- K19: the discriminator's 4x4 / stride-2 / padding-1 convolutions (adversarial warm-up stage) -----------
 * sseg/models/modules/discriminator.py:7-33 (FCDiscriminator: nn.Conv2d(kernel_size=4, stride=2, padding=1) x 5 with
 * LeakyReLU(0.2) between them) and what autograd derives from it.  fp32, contiguous NCHW, fp32 accumulation:
 *   x [B,Cin,H,W], w [Cout,Cin,4,4], bias [Cout] (NULL = none), y / dy [B,Cout,Ho,Wo], Ho = (H - 2) / 2 + 1, Wo likewise.
 * fwd:   y = conv(x, w) + bias, then LeakyReLU(0.2) when leaky != 0.
 * dgrad: dx (overwritten) from dy and w; with leaky != 0, dy is first multiplied by the activation's slope taken from the
 *        saved OUTPUT y (y > 0 ? 1 : 0.2), i.e. dy is the gradient w.r.t. the activation's output.  y may be NULL when leaky == 0.
 * wgrad: dw [Cout,Cin,4,4] and db [Cout] (NULL = not wanted), overwritten, from x and the same gated dy.  Pixel ranges are
 *        summed into workspace partials and added in a fixed order: two calls on the same inputs give the same bits.
 * workspace: hiast_disc_conv_workspace_bytes(B, Cin, Cout, H, W) bytes (0 = shape refused), 4-byte aligned, private to the
 *        call until the stream has passed it; one size serves dgrad and wgrad.  It never shrinks when B, H or W grow.
 * Refused (HIAST_E_RANGE): H or W < 2, more than 4096 channels, a tensor of 2^31 elements or more. */
size_t hiast_disc_conv_workspace_bytes(int B, int Cin, int Cout, int H, int W);
int hiast_disc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                        int leaky, hiast_stream_t stream);
int hiast_disc_conv_dgrad(const float* dy, const float* y, const float* w, float* dx, int B, int Cin, int Cout, int H, int W,
                          int leaky, void* workspace, size_t workspace_bytes, hiast_stream_t stream);
int hiast_disc_conv_wgrad(const float* x, const float* dy, const float* y, float* dw, float* db, int B, int Cin, int Cout,
                          int H, int W, int leaky, void* workspace, size_t workspace_bytes, hiast_stream_t stream);
/* The same three operations on the matrix cores: same tensors (fp32 NCHW in memory), same workspace, same checks and return
 * codes; fmt = HIAST_FMT_FP16 | HIAST_FMT_BF16 (anything else: HIAST_E_ARG, nothing launched).  Every operand value (x, w;
 * in the backward the fp32 product dy * slope, w and x) is rounded to fmt, nearest even, as it is staged — an fp16 overflow is
 * +-inf, not a clamp — and the products are summed in fp32.  Outputs are fp32.  wgrad keeps the split and the fixed-order
 * second stage of the fp32 entry: bit-reproducible. */
int hiast_disc_conv16_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                          int leaky, int fmt, hiast_stream_t stream);
int hiast_disc_conv16_dgrad(const float* dy, const float* y, const float* w, float* dx, int B, int Cin, int Cout, int H, int W,
                            int leaky, int fmt, void* workspace, size_t workspace_bytes, hiast_stream_t stream);
int hiast_disc_conv16_wgrad(const float* x, const float* dy, const float* y, float* dw, float* db, int B, int Cin, int Cout,
                            int H, int W, int leaky, int fmt, void* workspace, size_t workspace_bytes, hiast_stream_t stream);

/* ---- K12: IoU histograms --------------------------------------------------------------
 * utils/metrics.py:6-19 intersectionAndUnionGPU: pred/target int64 [N]; target==255 is
 * ignored; inter/area_pred/area_tgt i64 [K] ACCUMULATED (caller zeroes). */
int hiast_confusion_hist(const int64_t* pred, const int64_t* target, int64_t N, int K,
                         int64_t* inter, int64_t* area_pred, int64_t* area_tgt,
                         hiast_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HIAST_HIP_H */
