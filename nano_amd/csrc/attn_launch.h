// attn_launch.h -- from an attention plan to the kernel launch: the templates launch_attention() dispatches through, in a header so
// that the instantiations of one element format can be a translation unit of their own (attn.hip: FP32 and FP16 rows; attn_fp8.hip: FP8
// rows, compiled in parallel with the rest).
#pragma once
#include "attn_impl.h"

namespace nano {

namespace {

template <int LPR, int QV, int MODE, int KVH>
static hipError_t launch_mode_kv(const AttnArgs &a_in, const AttnPlan &p, uint32_t nb, hipStream_t st) {
    const uint32_t hd4 = (a_in.hd + 3) & ~3u;
    // (+ several heads per workgroup: the waves' transposition blocks of the sub-group combine, 4 waves x 64 / LPR sub-groups x LPR * QV * 4 floats)
    auto lds_for = [&](uint32_t kvm) { return (size_t)(kvm * hd4 + hd4 + 4 * kvm + 4 * kvm + (size_t)4 * kvm * hd4 + (kvm > 1 ? (size_t)4 * (64 / LPR) * (LPR * QV * 4) : 0)) * sizeof(float); };
    AttnArgs a = a_in;
    a.kv_log2 = p.kv_log2; a.kvmul_log2 = p.kvmul_log2;
    constexpr bool CAN16 = KVH == 1 && QV % 4 == 0;            // (FP8 rows have the narrow load form only: attention_plan() never sets w16 for them)
    const bool w16 = CAN16 && p.w16;
    const bool np4 = p.npt == 4u;
    // (a ragged step's launches -- a.row_slot -- run the attention_rows_kernel instantiation of the same plan)
#define ATTN_GO4(K_, KVM_, NP_, PG_) do { if constexpr (CAN16) { if (w16) { hipLaunchKernelGGL((K_<LPR, QV, KVM_, MODE, KVH, PG_, NP_, CAN16>), dim3(a.n_head / KVM_, nb, a.nsplit), dim3(256), lds_for(KVM_), st, a); break; } } \
                         hipLaunchKernelGGL((K_<LPR, QV, KVM_, MODE, KVH, PG_, NP_, false>), dim3(a.n_head / KVM_, nb, a.nsplit), dim3(256), lds_for(KVM_), st, a); } while (0)
#define ATTN_GO3(KVM_, NP_, PG_) do { if (a.row_slot) ATTN_GO4(attention_rows_kernel, KVM_, NP_, PG_); else ATTN_GO4(attention_kernel, KVM_, NP_, PG_); } while (0)
#define ATTN_GO2(KVM_, NP_) do { if (p.paged) ATTN_GO3(KVM_, NP_, true); else ATTN_GO3(KVM_, NP_, false); } while (0)
#define ATTN_GO(KVM_) do { if (np4) ATTN_GO2(KVM_, 4); else ATTN_GO2(KVM_, NP); } while (0)
    if (p.kvm == 4) {
        if constexpr (LPR == 16) return hipErrorInvalidValue;  // (attention_plan() caps head_dim > 128 at two heads: no such kernel)
        else ATTN_GO2(4, NP);
    } else if (p.kvm == 2) ATTN_GO(2); else ATTN_GO(1);
#undef ATTN_GO
#undef ATTN_GO2
#undef ATTN_GO3
#undef ATTN_GO4
    return hipGetLastError();
}
template <int LPR, int QV, int KVH>
static hipError_t launch_lpr(const AttnArgs &a, const AttnPlan &p, uint32_t nb, hipStream_t st) {
    // (FP8 rows: only what attention_plan() can ask for is built -- the Qwen3 decode mode needs head_dim % 64 == 0, never QV 1)
    if constexpr (!(KVH == 2 && QV == 1)) { if (p.mode == 1) return launch_mode_kv<LPR, QV, 1, KVH>(a, p, nb, st); }
    else if (p.mode == 1) return hipErrorInvalidValue;
    if (p.mode == 2) return launch_mode_kv<LPR, QV, 2, KVH>(a, p, nb, st);
    return launch_mode_kv<LPR, QV, 0, KVH>(a, p, nb, st);
}
// every launch of element format KVH (kernels.h KV_FMT_*)
template <int KVH>
static hipError_t launch_attention_fmt(const AttnArgs &a, const AttnPlan &p, uint32_t nb, hipStream_t st) {
    if (p.lpr == 16) return launch_lpr<16, 4, KVH>(a, p, nb, st);
    if (p.qv == 1) return launch_lpr<8, 1, KVH>(a, p, nb, st);
    if (p.qv == 2) return launch_lpr<8, 2, KVH>(a, p, nb, st);
    return launch_lpr<8, 4, KVH>(a, p, nb, st);
}

}  // namespace

}  // namespace nano
