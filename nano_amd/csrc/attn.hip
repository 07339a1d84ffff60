// attn.hip -- single-token GQA attention over the FP32 KV cache (reference infer/infer.c:810-879).
//
// One workgroup per (KV head group, sequence, split).  Like the GEMVs of a batch-1 decode step this kernel is
// LATENCY bound (a KV head's rows are at most a few hundred KB), so it is built as ONE memory round trip:
// at entry every thread issues the loads of q, the raw k row, the norm weights and ALL the K and V rows
// its workgroup will ever need (buffer descriptors: rows beyond the cache are out of range and read as 0
// without touching memory; rows beyond `range_hint`, the host's upper bound of pos+1 for this launch, are
// skipped the same way); position-dependent work (RoPE row, causal mask, the fresh k row) is applied
// afterwards, when pos[b] has arrived.
//   * the q heads of a KV group share every K/V row they read (GQA: kv_mul heads per workgroup);
//   * Qwen3 q/k rmsnorm (infer.c:824-835) and RoPE (rope_qwen3 infer.c:692-706 / rope infer.c:681-690) are
//     head-local and done here by one wave per vector (DPP reductions, no barrier);
//   * the finished k row is written to cache row `pos` by split 0; every workgroup uses its own LDS copy
//     for timestep pos, so nobody reads the row while it is being written; v went to the cache directly
//     from the QKV GEMV;
//   * timestep blocks are dealt round-robin to `nsplit` workgroups ("flash-decoding"); with nsplit == 1 the
//     kernel normalises and writes the final head outputs, otherwise UNNORMALISED partials
//     o_s = sum_t exp(s_t - m_s) v_t with (m_s, l_s) which the Wo GEMV's prologue combines (gemv_q80.hip).
// Softmax is algebraically the reference's (max-subtracted, infer.c:616-634); summation order differs and the
// q.k / weighted-V accumulations use fused multiply-adds (tolerance 1e-5).
#include "attn_launch.h"

namespace nano {

// timesteps one workgroup covers per round for this head size
static uint32_t steps_per_wg(uint32_t hd) { return NP * (256 / (hd > 128 ? 16 : 8)); }

// number of splits for an upper bound `range_hint` of the attended range: <= 8 up to attention_wide_from() positions (what the Wo
// GEMV's prologue combines); beyond, up to attention_split_cap() so that a long range still spreads over the chip (8 KV groups
// x 32 splits), combined by attn_combine_tokens_kernel -- a launch of its own, which pays from about four rounds per
// workgroup on (Qwen3-0.6B, tools/long_ctx_probe.py).
uint32_t attention_wide_from() {
    return 2048u;
}
uint32_t attention_split_cap() {
    return 32u;
}
uint32_t attention_nsplit(uint32_t range_hint, uint32_t hd) {
    const uint32_t per = steps_per_wg(hd), cap = range_hint > attention_wide_from() ? attention_split_cap() : 8u;
    uint32_t n = (range_hint + per - 1) / per;
    if (n < 1) n = 1;
    if (n > cap) n = cap;
    return n;
}

bool attention_plan(const AttnArgs &a, uint32_t nb, AttnPlan *out) {
    if (a.hd % 4 || a.hd > 256 || a.hd < 4 || a.nsplit == 0 || a.nsplit > ATTN_MAX_NSPLIT || !a.n_kv_head) return false;
    if (a.nsplit == 1 && !a.xba_out) return false;
    if (a.kv_half > KV_FMT_FP8) return false;
    AttnPlan p{};
    p.lpr = a.hd <= 128 ? 8u : 16u;                            // lanes per KV row and float4 slots per lane: the head fills a sub-group
    p.qv = a.hd <= 32 ? 1u : a.hd <= 64 ? 2u : 4u;
    // the decode modes index with shifts and masks: power-of-two head counts (every BASELINE shape: 16 / 8 and 32 / 8 heads)
    const uint32_t kv_mul = a.n_head / a.n_kv_head;
    const bool kv_pow2 = (a.n_kv_head & (a.n_kv_head - 1)) == 0, mul_pow2 = (kv_mul & (kv_mul - 1)) == 0;
    const bool decode = kv_pow2 && kv_mul && mul_pow2 && a.kraw && a.rope_cos && a.rope_cur && !a.fixed_range && a.is_causal && !a.q_out;
    p.mode = (decode && a.q_norm && a.rope_qwen3 && a.hd % 64 == 0 && a.hd == p.qv * p.lpr * 4u) ? 1u : (decode && !a.q_norm && !a.rope_qwen3) ? 2u : 0u;
    p.kv_log2 = 0xffffffffu; p.kvmul_log2 = 0;
    if (kv_pow2 && (p.mode != 0 || a.n_kv_head >= 8)) { uint32_t l2 = 0; while ((1u << l2) < a.n_kv_head) l2++; p.kv_log2 = l2; }
    if (mul_pow2) { uint32_t l2 = 0; while ((1u << l2) < kv_mul) l2++; p.kvmul_log2 = l2; }
    // q heads per workgroup (KVM; h0 = KVM grp, KV head h0 / kv_mul): fewer heads = more workgroups with less dependent work each,
    // the K/V rows' repeated reads come from L2 (and the KV head's fresh k row is written by each of its workgroups: same
    // bits).  Same per-head arithmetic whatever the choice.  One head per workgroup while that leaves at most one workgroup
    // per CU, two while at most two, else the whole KV group (measured: Qwen3-0.6B batch 1 6.15 -> 5.35 us per launch = +3.7 %
    // tokens/s; Qwen3-4B's kv_mul 4: 8.65 -> 6.03 us at batch 1, 10.05 -> 7.22 with two heads at 16 sequences, where one head
    // per workgroup costs 10.3; at 64 sequences the KV rows' bandwidth rules and four heads share them: 13.7 vs 16.4).
    const uint64_t head_wgs = (uint64_t)a.n_head * nb * a.nsplit;
    uint32_t kvm = (head_wgs <= 256u || kv_mul % 2 != 0) ? 1u : (head_wgs <= 1024u || kv_mul % 4 != 0) ? 2u : 4u;
    // A workgroup that would walk exactly two rounds of NP blocks (513 .. 1024 positions at 8 splits) keeps four blocks in flight
    // instead: every row of the launch requested at kernel entry (Qwen3-0.6B at position 1023: 639 -> 632 us per step).  Measured
    // and NOT taken beyond: four rounds -> two at 2047 positions 754 -> 759 us, two -> one at 4095 with 32 splits 819 -> 836 (the
    // issue phase grows from 3.1 to 5.9 us: `profiles/r04_long_ctx_np4.txt`).  Decided by the range and the split count alone --
    // never by the batch: a token's attention is the same expression in a decode step and in a prefill chunk (the four-head
    // workgroups of large batches give way to two heads).
    const uint32_t R = 256u / p.lpr;                           // timesteps per block
    const bool np4 = !a.prep_only && a.nsplit <= 8u && a.range_hint > a.nsplit * (uint32_t)NP * R && a.range_hint <= 2u * a.nsplit * (uint32_t)NP * R;
    if (np4 && kvm == 4) kvm = 2;
    // head_dim > 128: at most two heads.  The decode modes' shared q / k preparation (attention_body SHARE) gives wave 0's sub-groups one
    // vector each -- KVM q heads and the k row -- and a wave holds 64 / LPR = 4 sub-groups of 16 lanes: with four heads the k row had no
    // sub-group, was never stored, and every lane read stale LDS as the fresh k (tests/test_gpu_attention_decode.py).  No measured
    // configuration runs head_dim > 128, so the cap costs nothing known.
    if (p.lpr == 16 && kvm == 4) kvm = 2;
    p.kvm = kvm;
    p.npt = np4 ? 4u : (uint32_t)NP;
    // (FP8 rows: never.  Their wide form -- 8-byte loads with this slot map -- was measured 0.1 .. 0.8 % ahead of one 4-byte load per slot
    // at head_dim 128, no further than the controls drifted: not shown to earn its instantiations, not built.  profiles/kv_fp8.txt)
    p.w16 = (a.kv_half == KV_FMT_F16 && p.qv % 4 == 0 && a.hd % 8u == 0u) ? 1u : 0u;
    p.paged = a.pt_rows ? 1u : 0u;
    p.kv_half = a.kv_half;                                     // the element format (KV_FMT_*); w16 = the wide load form of FP16 rows
    p.nsplit = a.nsplit;
    *out = p;
    return true;
}

hipError_t launch_attention(const AttnArgs &a, uint32_t nb, hipStream_t st) {
    AttnPlan p;
    if (!attention_plan(a, nb, &p)) return hipErrorInvalidValue;
    if (a.kv_half == KV_FMT_FP8) return launch_attention_fp8(a, p, nb, st);      // (attn_fp8.hip)
    return a.kv_half ? launch_attention_fmt<1>(a, p, nb, st) : launch_attention_fmt<0>(a, p, nb, st);
}

// stand-alone combine (operator tests, state read-back; the forward folds this into the Wo GEMV's prologue)
__global__ void attn_combine_kernel(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit) {
    const uint32_t h = blockIdx.x, q_dim = n_head * hd;
    const float *mlh = ml + (size_t)h * nsplit * 2;
    float M = -INFINITY;
    for (uint32_t s = 0; s < nsplit; s++) if (mlh[2 * s + 1] > 0.0f) M = fmaxf(M, mlh[2 * s]);
    float L = 0.0f;
    for (uint32_t s = 0; s < nsplit; s++) L += mlh[2 * s + 1] * ((mlh[2 * s + 1] > 0.0f) ? expf(mlh[2 * s] - M) : 0.0f);
    for (uint32_t i = threadIdx.x; i < hd; i += blockDim.x) {
        float acc = 0.0f;
        for (uint32_t s = 0; s < nsplit; s++) {
            const float e = (mlh[2 * s + 1] > 0.0f) ? expf(mlh[2 * s] - M) : 0.0f;
            acc += part[(size_t)s * q_dim + (size_t)h * hd + i] * (e / L);
        }
        out[(size_t)h * hd + i] = acc;
    }
}
hipError_t launch_attn_combine(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit, hipStream_t st) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(n_head), dim3(128), 0, st, part, ml, out, n_head, hd, nsplit);
    return hipGetLastError();
}

// The combine of the Wo GEMV's prologue (gemv_common.h combine_weights / combine4) as a kernel of its own, for steps
// whose Wo cannot fold it in (batched prefill through the MFMA GEMM, ranges split more than 8 ways): same weights (8 slots,
// pairwise-tree sum of l_s * exp(m_s - M), e / L), same ascending accumulation -- the bits of x are those of the decode path; more
// than 8 splits: the 8-slot tree per block of 8, blocks added in order (combine_weights_lds above).  A thread owns ONE output
// element and asks for all its partials before the weights exist: one memory round trip.
template <int NS>
__global__ __launch_bounds__(128) void attn_combine_tokens_kernel(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit,
                                                                  int8_t *xf_out, float *xsf_out) {
    __shared__ float wsh[64];
    const uint32_t b = blockIdx.y, q_dim = n_head * hd;
    for (uint32_t i0 = 0; i0 < hd; i0 += 128u) {                 // (head_dim 256: two passes)
        const uint32_t hh = blockIdx.x, i = i0 + threadIdx.x;
        const bool live = i < hd;
        const float *pb = part + (size_t)b * nsplit * q_dim + (size_t)hh * hd + i;
        float o[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) o[s] = (live && (uint32_t)s < nsplit) ? pb[(size_t)s * q_dim] : 0.0f;
        if (i0 == 0) combine_weights_lds(ml + (((size_t)b * n_head + hh) * nsplit) * 2, nsplit, wsh);
        float acc = 0.0f;
#pragma unroll
        for (int s = 0; s < NS; s++) if ((uint32_t)s < nsplit) acc += o[s] * wsh[s];
        if (nsplit < (uint32_t)NS) acc += 0.0f;                  // (the empty slots' +0 of the register version: -0 becomes +0 as it always did)
        if (live) {
            out[(size_t)b * q_dim + (size_t)hh * hd + i] = acc;
            if (xf_out) {       // also as a Q80 group of 64 (= this wave's 64 lanes; head_dim % 64 == 0) in fragment order, see attention_kernel
                float mx = fabsf(acc);
#pragma unroll
                for (int o2 = 1; o2 < 64; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
                const float scale = div_const<127>(mx);
                const uint32_t el = hh * hd + i, g = el >> 6, jj = el & 63u, ng = q_dim >> 6;
                const size_t gb = (size_t)(b >> 4) * ng + g;
                xf_out[gb * 1024u + (size_t)((jj >> 4) * 16u + (b & 15u)) * 16u + (jj & 15u)] = (int8_t)q80_quant1(acc, scale);
                if (jj == 0) xsf_out[gb * 16u + (b & 15u)] = scale;
            }
        }
    }
}
hipError_t launch_attn_combine_tokens(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit, uint32_t nb,
                                      int8_t *xf_out, float *xsf_out, hipStream_t st) {
    if (xf_out && (hd % 64u || !xsf_out)) return hipErrorInvalidValue;
    if (nsplit == 0 || nsplit > ATTN_MAX_NSPLIT) return hipErrorInvalidValue;
    if (nsplit <= 8) hipLaunchKernelGGL(attn_combine_tokens_kernel<8>, dim3(n_head, nb), dim3(128), 0, st, part, ml, out, n_head, hd, nsplit, xf_out, xsf_out);
    else if (nsplit <= 32) hipLaunchKernelGGL(attn_combine_tokens_kernel<32>, dim3(n_head, nb), dim3(128), 0, st, part, ml, out, n_head, hd, nsplit, xf_out, xsf_out);
    else hipLaunchKernelGGL(attn_combine_tokens_kernel<64>, dim3(n_head, nb), dim3(128), 0, st, part, ml, out, n_head, hd, nsplit, xf_out, xsf_out);
    return hipGetLastError();
}

}  // namespace nano
