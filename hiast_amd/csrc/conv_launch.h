// Host side of the trunk convolutions: ONE record that describes a launch (ConvLaunch), ONE answer to "which kernel takes it,
// in which form, and how many block rows does it write" (ConvRoute, ig_route), and the only declarations of the functions that
// cross translation units on the way from the C ABI to hipLaunchKernelGGL.  Internal: not part of include/hiast_hip.h.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace hiast {

// geometry of a 3x3 launch: H x W is the operand map, Ho x Wo the output map (stride < 0: the transposed stride-2 convolution,
// igemm_kernel.h UPS).  A caller of hiast_igemm_launch fills H, W, stride and dil (for stride -2, H x W is the OUTPUT map); the
// launcher validates them and derives the rest.  1x1 launches ignore it.
struct IGeo {
    int H, W, Ho, Wo, stride, dil;
};

}  // namespace hiast

// One trunk-convolution launch: Y[M][N] = act((X * Wp^T) * scale + shift (+ res)).  Call sites start from the defaults and name
// the fields they set.
struct ConvLaunch {
    // operands (16-byte aligned): activation rows, packed weight (hiast_pack_conv_weight), output, residual rows, and the gate of
    // the residual (gate_mask: one bit per channel instead of values like res)
    const void* x = nullptr;
    const void* wp = nullptr;
    void* y = nullptr;
    const void* res = nullptr;
    const void* res_gate = nullptr;
    int gate_mask = 0;
    // folded BatchNorm (mean == nullptr: none); with stats_mode 2 the batch mean / invstd of the BN whose gradient the output is
    const float* gamma = nullptr;
    const float* beta = nullptr;
    const float* mean = nullptr;
    const float* var = nullptr;
    float eps = 0.0f;
    int relu = 0;
    int64_t M = 0;                       // output pixels
    int K = 0, N = 0, taps = 1;          // reduction channels, output channels, 1 | 9
    hiast::IGeo geo = {0, 0, 0, 0, 1, 1};
    int fmt = HIAST_FMT_BF16;            // operand format (HIAST_FMT_*)
    int out_f32 = 0;                     // fp32 [M][N] output instead of the operand format
    // per-block-row sums: stats[stats_rows][N][2].  stats_mode: 0 none | 1 forward BatchNorm sums of the output | 2 backward
    // BatchNorm sums of the activation whose gradient the output is (data-gradient launches: res = that BN's input).  Callers
    // set 2 only; hiast_igemm_launch derives 0 / 1 from `stats`.
    float* stats = nullptr;
    int stats_rows = 0;
    int stats_mode = 0;
    hipStream_t st = nullptr;

    int planes() const { return hiast_fmt_planes(fmt); }
    bool f16() const { return fmt == HIAST_FMT_FP16; }
};

enum class ConvFamily { XCONV, XCONV2, TILE_F16, TILE };

struct ConvRoute {
    ConvFamily family = ConvFamily::TILE;
    int BN = 0, BM = 0;                  // tile families: columns (256 | 128 | 64) and rows (256 | 128) of the block tile
    bool half9 = false;                  // tile families: the 128 x 128 form of the split-plane 3x3 + BN + ReLU launch
    int rows = 0;                        // block rows (xconv: panel streams) = rows of a statistics buffer; 0 for XCONV2
};

// Panel streams of the persistent 1x1 kernels (xconv.hip, xconv2.hip; their grid is streams x NG column groups): one block per
// CU (HIAST_XCONV_CUS: experiment, part of the chip) in whole rounds of the 8 XCDs, which the kernels' (slot, xcd) numbering
// wants, and no more than the panels need.
static inline int conv_panel_streams(int64_t M, int NG, int panel_rows)
{
    static const int env_cus = [] { const char* e = getenv("HIAST_XCONV_CUS"); const int v = e ? atoi(e) : 0; return v >= 8 && v <= 256 ? v : 0; }();
    const long long npanel = (M + panel_rows - 1) / panel_rows;
    long long streams = (env_cus ? env_cus : hiast_grid_cus()) / NG / 8 * 8;
    if (streams < 8) streams = 8;
    if (streams > npanel) streams = (npanel + 7) / 8 * 8;
    return (int)streams;
}

// igemm.hip.  ig_route reads the shape, the format, which operands are present and stats_mode (never stats or stats_rows), so the
// row-count entries of the ABI ask it about the launch they size without having its buffers.
ConvRoute ig_route(const ConvLaunch& c);
int hiast_igemm_launch(const ConvLaunch& c);                              // validates, routes, launches (also aspp2.hip's tap GEMMs)
// igemm_f16.hip: the fp16 instantiations of the tile kernel (a translation unit of its own: build time)
int hiast_igemm_launch_f16(const ConvLaunch& c, const ConvRoute& r);
// K9e (xconv.hip): register-resident-weight kernel for the HBM-bound expanding 1x1 shapes
int hiast_xconv_ok(const ConvLaunch& c);
int hiast_xconv_stats_rows(int64_t M, int N);
int hiast_xconv_launch(const ConvLaunch& c, const ConvRoute& r);
// K9g (xconv2.hip): the same idea for the split-plane 256 -> N launches with BatchNorm(eval) (+ residual + ReLU)
int hiast_xconv2_ok(const ConvLaunch& c);
int hiast_xconv2_launch(const ConvLaunch& c);
// conv1x1.hip: fp32 rows x fp32 weights (the ASPP tap GEMM on unpacked operands)
int hiast_gemm_nt_launch(const float* x, const float* w, float* y, int64_t M, int K, int N, hipStream_t st);
