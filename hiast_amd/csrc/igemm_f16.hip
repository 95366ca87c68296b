// K9c, fp16 instantiations: the implicit-GEMM tile kernel of igemm_kernel.h on IEEE fp16 rows (HIAST_FMT_FP16) — the
// reference's apex-O1 arithmetic (code/utils/default_config.py:109, utils/utils.py:126-132: half-precision convolutions,
// fp32 accumulation, fp32 master weights) for the teacher forward, the student forward and the data gradients.
// Same kernel text as the bf16 variants (LDS-DMA slabs, asm fragment reads, counted waits); only H16<true> differs.
#include "igemm_kernel.h"

int hiast_igemm_launch_f16(const ConvLaunch& c, const ConvRoute& r)
{
    return c.out_f32 ? launch_igemm_t<1, true, true>(c, r) : launch_igemm_t<1, false, true>(c, r);
}
