// gemv.hip -- dispatcher of the fused decode GEMVs (out[d] = W[d,n] . act[n] for up to 8 sequences) by weight format:
//   FP32 matmul (reference infer/infer.c:637-651)            -> gemv_f32.hip
//   Q80  matmul_quant + quantize (infer.c:654-679, tensor.c:21-46) -> gemv_q80_impl.h (one translation unit per group size)
//   Q4K  matmul_q4k (tensor.c:438-471)                        -> gemv_q4k.hip
#include "kernels.h"

namespace nano {

hipError_t launch_gemv(uint32_t quant, GemvArgs &a, hipStream_t st) {
    if (quant == 0x80u) return launch_gemv_q80(a, st);
    return launch_gemv_f32(a, st);
}

// number of (max, row) arg-max partials launch_gemv() will write per sequence for these arguments (sizes tile_max;
// 0 = none written, the arg-max kernel scans the logits)
uint32_t gemv_tiles(uint32_t quant, const GemvArgs &a) {
    if (quant == 0x80u) return gemv_q80_partials(a);
    if (quant == 0x42u) { Q4kGemvPlan p; return gemv_q4k_plan(a, &p) ? p.partials : 0u; }
    return 0;
}

// ---- the fused q | k | v + attention launch: each format's pair lives with its kernel ----
#define NANO_FUSED_PAIR(F) bool qkv_attn_fused_##F##_plan(const GemvArgs &, const AttnArgs &, QkvAttnFusedPlan *); \
                           hipError_t launch_qkv_attn_fused_##F(const GemvArgs &, const AttnArgs &, unsigned long long *, uint32_t *, uint32_t, hipStream_t);
NANO_FUSED_PAIR(q80) NANO_FUSED_PAIR(q4k) NANO_FUSED_PAIR(f32)
#undef NANO_FUSED_PAIR

bool qkv_attn_fused_plan(uint32_t quant, const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan *p) {
    if (quant == 0x80u) return qkv_attn_fused_q80_plan(ga, aa, p);
    if (quant == 0x42u) return qkv_attn_fused_q4k_plan(ga, aa, p);
    return qkv_attn_fused_f32_plan(ga, aa, p);
}
hipError_t launch_qkv_attn_fused(uint32_t quant, const GemvArgs &ga, const AttnArgs &aa, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st) {
    if (quant == 0x80u) return launch_qkv_attn_fused_q80(ga, aa, hand, tick, layer1, st);
    if (quant == 0x42u) return launch_qkv_attn_fused_q4k(ga, aa, hand, tick, layer1, st);
    return launch_qkv_attn_fused_f32(ga, aa, hand, tick, layer1, st);
}

}  // namespace nano
