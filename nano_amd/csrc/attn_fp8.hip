// attn_fp8.hip -- the attention launches on FP8 (OCP e4m3fn) KV rows: the attention_body instantiations of element format 2 (attn_impl.h
// has the format, attn.hip the design and the planner).  A translation unit of its own so that the format's kernels compile next to
// the FP32 / FP16 ones, not behind them.
#include "attn_launch.h"

namespace nano {

hipError_t launch_attention_fp8(const AttnArgs &a, const AttnPlan &p, uint32_t nb, hipStream_t st) {
    return launch_attention_fmt<2>(a, p, nb, st);
}

}  // namespace nano
