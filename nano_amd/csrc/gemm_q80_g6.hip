// gemm_q80_g6.hip -- G6: the split-K Q80 (W8A8) projection kernel of the FAST path, group size 64, 1..16 tokens per weight read.
//
// What it replaced and why (round 4).  Its predecessor G5 (since removed) kept the reference's ascending group order
// (infer/infer.c:668-674) for every output by handing a running value from wave to wave -- a serial chain through LDS (19 links for
// Qwen3-4B's W2) -- and its SwiGLU launch tied eight waves to one 64-row output group (152 of 256 CUs busy).  The fast path is held to the
// float bar of SURVEY 7 tier ii (<= 1e-5 relative; the integer group sums and both quantizers stay bit-exact) with ONE fixed,
// split-independent reduction shape -- the CANONICAL fold, shared with the GEMV kernels (gemv_q80_impl.h), G7 and G7K:
//     products   p_g   = ((float)ival_g * ws_g) * xs_g                          (infer.c:672, unchanged)
//     unit sums  S_u   = ((p_8u + p_8u+1) + ... ) + p_8u+7                      (8 groups = 512 bytes of the row, ascending)
//     row value        = ((S_0 + S_1) + S_2) + ...                              (units ascending)
// so a batch is still bit for bit its sequences alone and batched prefill is bit for bit token-by-token ingestion.  Strict mode
// (nano_hip_set_strict) keeps the reference's order in the older kernels and stays the bit-exact certificate.
//
// Structure (MI355X: 256 CUs, 8 waves of one workgroup per CU, LDS 160 KB):
//   * a TILE is up to 16 matrix rows = two halves of `hh` <= 8 rows (SwiGLU: half 0 = rows of W1, half 1 = the same rows of W3, so
//     the pair meets in one matrix-core tile and no 64-row grouping is needed); hh is fitted on the host so that the tiles spread
//     evenly over the CUs (a launch lasts as long as the CU with the most rows).  Workgroup b owns tiles b, b + grid, ...
//   * an ITEM is (tile, unit): 16 rows x 512 B = 8 KB of weights.  The items of a workgroup are dealt round-robin to its waves;
//     a wave keeps D items in flight in registers (every load of a Qwen3-4B launch is issued at kernel entry) -- TRUE split-K:
//     no wave waits for another one's result before it multiplies.
//   * per item: registers -> wave-private LDS transposition buffer (row pitch 528 B) -> MFMA A fragments (ds_read_b128); one
//     v_mfma_i32_16x16x64_i8 per group gives the exact int32 group sums of (16 rows x 16 tokens); products; the unit sum S_u goes
//     to an LDS table; the wave that owns the row's LAST unit waits for the tile's counter, adds the units in order and runs the
//     epilogue (store | residual add | SwiGLU).  One counter wait per tile, no chain.
//   * the activation comes first in every wave's load queue (loads return in issue order; round 3 measured the activation of a
//     52.9 MB launch "arriving" after the whole weight burst when it was issued behind it):
//       MODE S  (fragment-order activations that fit LDS: rows <= 4096 values, <= 16 tokens): the workgroup's copy is staged once;
//       MODE F  (fragment-order activations from quant_rows_frag_kernel / the attention kernel): each item's 8 KB of B fragments
//               are requested right before its weights.
// MFMA operand layout as in gemm_q80.hip (verified on gfx950, tools/kbench/mfma_probe.hip).
#include "gemm_q80_g6_impl.h"

namespace nano {

// ---- host side: every choice is the plan's (q80_gemm_plan_g6(), gemm_q80_host.h) -----------------------------------------------------
hipError_t launch_gemm_q80_g6(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st) {
    G6Dev d{};
    d.g = to_dev(a);
    d.g.nthr = p.threads;
    d.xf = a.xq_in; d.xsf = a.xs_in;
    d.hh = p.hh; d.nu = p.nu; d.magic_nu = p.magic;
    d.tts = p.tts; d.tts_log2 = p.tts == 4u ? 2u : p.tts == 2u ? 1u : 0u;
    d.ntiles = p.ntiles; d.tc0 = p.tc0; d.tc1 = p.tc1; d.grid = p.grid; d.tpw = p.tpw; d.nw = p.nw; d.full = p.full;
    const size_t lds = p.lds_bytes;
    if (p.kernel == Q80_GEMM_G6S) {
#define G6S_GO(NV_, R_) do { return p.ms ? g6_launch_t<G6_S, NV_, R_, true>(d, lds, st) : g6_launch_t<G6_S, NV_, R_, false>(d, lds, st); } while (0)
#define G6S_R(NV_) do { if (p.r == 1u) G6S_GO(NV_, 1); if (p.r == 2u) G6S_GO(NV_, 2); G6S_GO(NV_, 4); } while (0)
        if (p.nv == 5u) G6S_R(5);
        G6S_R(8);
#undef G6S_R
#undef G6S_GO
    }
#define G6F_GO(R_, T_) do { return p.ms ? g6_launch_t<G6_F, 1, R_, true, T_>(d, lds, st) : g6_launch_t<G6_F, 1, R_, false, T_>(d, lds, st); } while (0)
#define G6F_R(T_) do { if (p.r == 1u) G6F_GO(1, T_); if (p.r == 2u) G6F_GO(2, T_); if (p.r == 3u) G6F_GO(3, T_); G6F_GO(4, T_); } while (0)
    if (p.tt == 1u) G6F_R(1);
    if (p.tt == 2u) G6F_R(2);
    if (p.r == 1u) G6F_GO(1, 4);
    if (p.r == 2u) G6F_GO(2, 4);
    G6F_GO(3, 4);
#undef G6F_R
#undef G6F_GO
}

}  // namespace nano
