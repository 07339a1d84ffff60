// kernels.h -- host-visible argument blocks and launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nano_mi355x.h"
#include "device_common.h"

namespace nano {

enum : uint32_t { GEMV_EPI_STORE = 0, GEMV_EPI_RESID = 1, GEMV_EPI_SWIGLU = 2 };

// One weight tensor (or a run of them sharing the input vector) of a fused GEMV launch.
struct GemvSeg {
    const void *w;          // FP32: float[rows][n]; Q80: int8[rows][n]; Q4K: 160-byte blocks, 16-B aligned
    const float *ws;        // Q80: float[rows][n/gs]
    float *out;             // output base
    uint32_t rows;
    uint32_t out_bstride;   // floats between sequence slots
    uint32_t out_pstride;   // floats per position (KV-cache rows); 0 = not position indexed
    uint32_t _pad;
};

struct GemvArgs {
    GemvSeg seg[3];
    uint32_t nseg;
    uint32_t n;             // row length (input vector length)
    uint32_t gs;            // Q80 group size
    uint32_t nb;            // live sequences (<= template capacity)
    const float *xin;       // fp32 input vectors
    uint32_t xin_bstride;
    uint32_t epi;
    const float *norm_w;    // rmsnorm weight or nullptr
    const uint32_t *pos;    // device positions [nb] (for out_pstride)
    uint32_t tiles;         // filled by the launcher
    uint32_t frag_ready;    // batched GEMM path: 1 = the fragment-order activations already exist in the step's scratch (the attention kernel wrote them)
    // operator-test inputs: an already quantized activation (skips the quantizing prologue)
    const int8_t *xq_in;    // Q80 int8[n] (batched GEMM path with frag_ready: all tokens, MFMA B-fragment order)
    const float *xs_in;     // Q80 float[n/gs]
    const uint8_t *x4_in;   // Q4K blocks[ceil(n/256)*160]
    uint8_t *q4_scratch; size_t q4_scratch_bytes;   // Q4K, 2 .. 64 sequences: room for the staged groups of every sequence (nb * n bytes), or nullptr
    float *f32_scratch; size_t f32_scratch_floats;  // FP32, 9 .. 64 tokens: room for the operand-order activations of gemm_f32.hip (F32GemmPlan::xs_floats), or nullptr
    // input = combination of split attention partials (attn.hip) instead of xin:
    //   x[b][i] = sum_s part[b][s][i] * w[b][head(i)][s],  w from the (max, sum) pairs in attn_ml
    const float *attn_part; // [nb][nsplit][n] unnormalised partial outputs, or nullptr
    const float *attn_ml;   // [nb][n_head][nsplit][2] (running max, exp-sum) per split
    uint32_t attn_nsplit, attn_n_head, attn_hd;
    uint32_t attn_table;    // 1: the combine keeps its table form (weights through LDS) where the in-wave form would apply (gemv_q80_host.h combine_wave_shape())
    // residual epilogue only: an extra vector added to the GEMV result BEFORE the residual add, x += (W.act + resid_add)
    // (the LoRA o-branch, reference infer.c:898-908); [nb][resid_add_bstride] or nullptr
    const float *resid_add; uint32_t resid_add_bstride, _pad3;
    // optional per-tile arg-max partials of a STORE launch: tile_max[b][tile] = (max value, row index bits)
    float *tile_max;
    uint32_t cus;           // compute units of the device the launch goes to (0: assume 256); sizes the work split
    uint32_t ordered;       // 1: strict mode -- every fp32 group fold in the reference's ascending order (infer.c:668-674); 0: the fast
                            // path's CANONICAL fold where it applies (q80_canonical(): unit sums of 8 groups, units ascending)
    uint32_t *err;          // sticky error word of the model (device pointer to host-mapped memory), or nullptr: see NANO_DEVERR_*
    unsigned long long *stamps;   // measurement builds only (NANO_STAMPS): per-workgroup phase stamps, or nullptr
};

// Bounded waits inside kernels (G6's finisher on its tile counter, the fused launches' consumers on their granules) must not hang the device; a wait that gives up ORs its code (device_common.h NANO_DEVERR_*) into the model's
// sticky error word: the next synchronising C-ABI call re-issues the work through the plain launches (hand-offs) or returns NANO_HIP_ERUNTIME
// instead of results computed from whatever was there (round-4 / round-5 advice).

// The fast path's reduction shape of a Q80 projection (group size 64, row length a multiple of 256; not the classifier-like tall
// STORE launches, whose kernels hold whole rows per wave and keep the reference's order): row = ((S_0 + S_1) + ...), S_u = the 8
// group products of unit u added in ascending order.  Every kernel a launch can be routed to (SLAB GEMV, G6, G7) implements this
// one shape: given the same quantized activations, a batch's projections are bit for bit its sequences' alone whatever route each
// size takes.  What a batch shares beyond that: the rmsnorm sum-of-squares tree in front of the quantizer is 256 threads wide on
// every route of the small matrices (Qwen3-0.6B: batches ARE their sequences alone end to end, tests/test_gpu_fullsize.py::test_batch_equals_sequences_alone_and_runs_repeat asserts it);
// on the wide matrices (route_is_wide(), Qwen3-4B) the one- and two-sequence SLAB launches run the tree of their own thread count
// and the >= 3-sequence launches the 512-thread one (route_norm_order()), so a scale may differ in its last ulp between batch
// sizes there -- inside the fast path's stated tolerance, not a bit-for-bit promise.  Strict mode: never canonical.
inline bool q80_canonical(const GemvArgs &a) {
    if (a.ordered || a.gs != 64 || a.n % 256u) return false;
    if (a.nseg == 1 && a.epi == GEMV_EPI_STORE && a.seg[0].rows >= 16384u && a.seg[0].out_pstride == 0) return false;
    return true;
}
uint32_t gemv_tiles(uint32_t quant, const GemvArgs &a);   // tiles launch_gemv() will use (sizes tile_max)
hipError_t launch_gemv(uint32_t quant, GemvArgs &a, hipStream_t st);
// rows of a launch: the tensors of a STORE / residual launch one after the other (SwiGLU: the two matrices share theirs)
inline uint32_t gemv_total_rows(const GemvArgs &a) {
    if (a.epi == GEMV_EPI_SWIGLU) return a.seg[0].rows;
    uint32_t r = 0;
    for (uint32_t s = 0; s < a.nseg; s++) r += a.seg[s].rows;
    return r;
}
hipError_t launch_gemv_q4k(const GemvArgs &a, hipStream_t st);
// The launch launch_gemv_q4k() issues for `a` (nb <= 8): the item kernel gemv_q4k_slab_kernel<role, B, nv, ipt> (gemv_q4k.hip) or the chunk
// kernel gemv_q4k_chunk_kernel<role, nv, d, loop, B> (gemv_q4k_chunk.hip: whole 256-value blocks, n <= 16384; 2 .. 8 sequences with
// GemvArgs::q4_scratch, behind a q4k_quant_rows_kernel<., quant_nv> launch of quant_nthr threads per sequence), with its threads, rows per
// workgroup, workgroups and LDS bytes; the launchers take every choice from here.  false: the arguments are refused -- malformed, several
// weight tensors whose row counts are no multiples of 4 on the item kernel, more than 4 items per thread, or more LDS than a CU has
// (gemv_q4k_fit_batch() tells the router how many sequences fit).
constexpr uint32_t GEMV_Q4K_LDS_MAX = 160 * 1024;
constexpr uint32_t GEMV_Q4K_CHUNK_SEARCH_LDS = 150 * 1024;  // the chunk planner's search stops at slabs whose workgroups (k per CU) would ask for more
enum : uint32_t { Q4K_KERNEL_NONE = 0, Q4K_KERNEL_SLAB = 1, Q4K_KERNEL_CHUNK = 2 };
struct Q4kGemvPlan {
    uint32_t kernel, role, B;                   // B: the template capacity 1 | 2 | 4 | 8 (the chunk kernel's NB)
    uint32_t nv, ipt;                           // the NV template value (0 | 1 | 2 | 4; chunk: 1 | 2 | 4); slab: items per thread 1 | 2 | 4
    uint32_t d, loop, rounds, wg[3];            // chunk: wave-loads in flight per wave, the persistent (classifier) form and its rounds, workgroups per tensor
    uint32_t rw, nthr, grid, lds_bytes;         // rows per workgroup, threads, workgroups, dynamic LDS
    uint32_t pre;                               // the caller brings the quantized activation (F_PRE)
    uint32_t quant_rows, quant_nthr, quant_nv;  // 1: a q4k_quant_rows_kernel launch goes first, with the one-sequence chunk plan's threads and NV
    uint32_t partials;                          // (max, row) arg-max pairs per sequence the launch writes into tile_max, one per workgroup; 0: none
};
bool gemv_q4k_plan(const GemvArgs &a, Q4kGemvPlan *p);
uint32_t gemv_q4k_fit_batch(const GemvArgs &a);            // sequences per item-kernel launch that fit in LDS (8 | 4 | 2 | 1; 0: not even the one-sequence launch is taken)
// Q4K, 9..64 tokens per weight read on the int8 matrix cores (gemm_q4k.hip): the quantizer launch of the several-sequence chunk launches
// (one workgroup per token, a.q4_scratch = nb * n bytes) + one MFMA per (group, token tile), the reference's float order -- bit for bit
// the chunk GEMV's results.  Takes: whole blocks (n % 256 == 0, n <= 16384), segment rows in multiples of 16, no LoRA addend, no
// caller-quantized activation, no arg-max partials; split-attention partials where the one-sequence chunk launch takes them.
bool gemm_q4k_supports(const GemvArgs &a);                  // host predicate (shapes and features; the scratch is the router's question)
hipError_t launch_gemm_q4k(const GemvArgs &a, hipStream_t st);
hipError_t launch_gemv_q80(const GemvArgs &a, hipStream_t st);      // gemv_q80.hip
hipError_t launch_gemv_f32(const GemvArgs &a, hipStream_t st);      // gemv_f32.hip
// The kernel launch_gemv_q80() runs for `a` (nb <= 8) -- gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, EARLY, WF, WFC> or
// gemv_q80_stream_kernel<ROLE, GS, B, NV> (gemv_q80_impl.h) -- with its waves, rows per workgroup, workgroups and LDS bytes; the launchers
// take every choice from here.  false: the arguments are refused -- malformed, a SwiGLU launch without its two matrices, several weight
// tensors whose row counts are no multiples of 4, more than 4 work units per wave, or more LDS than a CU has (gemv_q80_fit_batch() tells
// the router how many sequences fit).
constexpr uint32_t GEMV_Q80_LDS_MAX = 160 * 1024;
enum : uint32_t { Q80_KERNEL_NONE = 0, Q80_KERNEL_SLAB = 1, Q80_KERNEL_STREAM = 2 };
// the special forms of the slab kernel: EARLY (the first unit of each wave before the activation is quantized), WF (in-wave fold of
// one-chunk rows), WFC2..4 (in-wave fold of the 2..4 chunks of a residual row)
enum : uint32_t { Q80_VAR_PLAIN = 0, Q80_VAR_EARLY = 1, Q80_VAR_WF = 2, Q80_VAR_WFC2 = 3, Q80_VAR_WFC3 = 4, Q80_VAR_WFC4 = 5 };
struct Q80GemvPlan {
    uint32_t kernel, role, gs, B, nv, upw;      // nv, upw: the NV and UPW template values (STREAM: upw = 0)
    uint32_t rw, nw, grid, lds_bytes;           // rows per workgroup (STREAM: the 16 rows of a wave's tile), waves, workgroups, dynamic LDS
    uint32_t variant, pre;                      // Q80_VAR_*; pre: the activation arrives quantized (F_PRE)
    uint32_t early, units, wg_c0, wg_c1;        // the launchers' device block: GemvDev::early, units, workgroups up to the end of segment 0 / 1
    uint32_t cw;                                // 1: gemv_q80_slab_cw_kernel<nv, upw, wfc> -- the combine role, one item per thread, with the splits' weights made inside each wave (variant plain | wfc2..4)
};
bool gemv_q80_plan(const GemvArgs &a, Q80GemvPlan *p);
uint32_t gemv_q80_fit_batch(const GemvArgs &a);            // sequences per Q80 GEMV launch that fit in LDS (8 | 4 | 2 | 1; 0: none -- the shape is refused)
// the gemv_f32_slab_kernel<ROLE, B, NV, UPW> launch_gemv_f32() runs for `a` (nb <= 8), its waves, workgroups and LDS bytes; the launcher
// takes every choice from here.  false: the arguments are refused -- malformed, more than 4 units per wave, or more LDS than a CU has.
constexpr uint32_t GEMV_F32_LDS_MAX = 160 * 1024;
struct F32GemvPlan { uint32_t role, B, nv, upw, rw, nw, grid, lds_bytes; };
bool gemv_f32_plan(const GemvArgs &a, F32GemvPlan *p);
uint32_t gemv_f32_fit_batch(const GemvArgs &a);            // sequences per FP32 launch that fit in LDS (8 | 4 | 2 | 1; 0: none -- the shape is refused)
// FP32, 9..64 tokens per weight read on the FP32 matrix cores (gemm_f32.hip): an activation prologue launch (one workgroup per token: the
// GEMV's own rmsnorm on the thread count of the sliced route's launch, the result in MFMA operand order in a.f32_scratch) + the GEMM, whose
// v_mfma_f32_16x16x4_f32 per float4 item, pairwise tree per 128-float unit and ascending chunk fold are the GEMV's reduction shape: bit for
// bit its results.  gemm_f32_plan() (gemm_f32_host.h) names the whole launch; the launcher takes every choice from it and cannot refuse.
// false: the shape is refused (nb outside 9..64, n % 4, a row the GEMV plan refuses, segment rows no multiple of 16, the LoRA addend,
// split-attention partials, arg-max partials, more LDS than a CU has, a tensor of 2^32 bytes or more) and the sliced route keeps it.
constexpr uint32_t GEMM_F32_LDS_MAX = 160 * 1024;
struct F32GemmPlan {
    uint32_t sw;                                // template value: 1 = the W1 and the W3 tile of the same rows in one workgroup (SwiGLU)
    uint32_t threads, grid, lds_bytes;          // 64 * nw threads x grid workgroups (one per row tile), dynamic LDS
    uint32_t rt, nw, nt, nu, upw, tp;           // rows of a tile (16), waves, token tiles of 16, units of 128 floats per row, units of a wave (max), floats between table rows
    uint32_t stage_bytes, tab_off;              // LDS: a wave's transposition buffer; byte offset of the unit-sum table [matrix][unit][row][tp]
    uint32_t pro_threads, pro_lds;              // the prologue launch: threads per token (the sliced route's launch of this shape), its LDS bytes
    uint32_t xs_floats;                         // floats of operand-order scratch the launch needs
};
bool gemm_f32_plan(const GemvArgs &a, F32GemmPlan *p);
inline bool gemm_f32_supports(const GemvArgs &a) { return gemm_f32_plan(a, nullptr); }
hipError_t launch_gemm_f32(const GemvArgs &a, hipStream_t st);
// 2..64 tokens per weight read on the int8 matrix cores, activations in MFMA B-fragment order (a.xq_in / a.xs_in = launch_quant_rows_frag's
// output, or the attention kernel's).  The canonical fold (q80_canonical()):
//   G6 (gemm_q80_g6.hip)   split-K over (tile, unit) items; MODE S: the activation staged in LDS once per workgroup (<= 16 tokens, rows of
//                          <= 4096 values), MODE F: fetched per item, 1 / 2 / 4 token tiles
//   G7 (gemm_q80_g7.hip)   17..64 tokens, several row tiles per CU or very short rows: LDS-DMA loader waves stream the weights through an
//                          LDS ring, consumer waves own (row tile, token tile) pairs for the whole row length
//   G7K (gemm_q80_g7.hip)  3..48 tokens, one row tile per CU and rows of >= 2048 values: the waves split the row length by units
// The reference's ascending group order (strict mode, group sizes other than 64, rows that are no multiple of 256, the classifier):
//   GC (gemm_q80_cls.hip)  tall matrices with short rows (the classifier): persistent waves, activation fragments staged in LDS
//   G2 (gemm_q80.hip)      the general kernel
// gemm_q80_plan() names the whole launch of `a` -- the kernel in this order of preference: canonical launches G7K, G7, G6; the others
// GC, G2 -- with its template values, threads, workgroups, dynamic LDS bytes and the fields the kernel's device block is filled from;
// the launchers (gemm_q80_host.h) take every choice from it and cannot refuse.  false: no batched kernel takes the launch (a shape or
// feature none of them has, or more LDS than a CU has) and nothing is launched -- the router then cuts it into GEMV launches.
enum : uint32_t { Q80_GEMM_NONE, Q80_GEMM_G6S, Q80_GEMM_G6F, Q80_GEMM_G7, Q80_GEMM_G7K, Q80_GEMM_GC, Q80_GEMM_G2 };
struct Q80GemmPlan {
    uint32_t kernel;
    // template values -- G6: MODE (the kernel), NV, R, MS, TT; G7: TP, PP, MS; GC: TT; G2: GS, SW, TT
    uint32_t tt, nv, r, ms, tp, pp, gs, sw;
    uint32_t threads, grid, lds_bytes;
    uint32_t norm_order;                        // tree width of the quant_rows_frag launch in front (route_norm_order())
    // row tiles (G6, G7, G7K; GC: ntiles): live rows per half tile, tiles, tiles up to the end of segment 0 / 1, tiles per workgroup (max),
    // workgroups that own tpw tiles; units of 8 groups, steps of 256 B, live token tiles
    uint32_t hh, ntiles, tc0, tc1, tpw, full, nu, nk, ttl;
    uint32_t nw, rounds, tts;                   // G6: waves, the most items a wave owns, token tiles spread over the waves
    uint32_t magic;                             // G6: G6Dev::magic_nu; G2: G2Dev::magic_ng
    uint32_t nsa, pre, a_stage, a_ws, b_base, b_stage, b_xs;    // G7: ring stages, steps asked for before the first barrier, the LDS layout (G7Dev)
    uint32_t ks, ncw, nss, tab, ring, nl;       // G7K: phases, consumer waves, super-steps, LDS offset of the unit-sum table, ring super-steps, loader waves
    uint32_t waves, lt, nhc, nwaves;            // GC: waves per workgroup, token tiles staged in LDS, half chunks per row, waves of the launch
    uint32_t ng, npass;                         // GC, G2: groups per row; G2: passes of 512 B
};
bool gemm_q80_plan(const GemvArgs &a, Q80GemmPlan *p);
// order: threads of the rmsnorm sum-of-squares tree -- 256 (the SLAB GEMV prologue's of the small matrices) or 512 (the wide matrices' batched launches, route_norm_order())
hipError_t launch_quant_rows_frag(const float *x, uint32_t x_bstride, const float *norm_w, uint32_t n, uint32_t gs, uint32_t nb,
                                  int8_t *xf, float *xsf, hipStream_t st, uint32_t order = 256);
hipError_t launch_quant_rows(const float *x, uint32_t x_bstride, const float *norm_w, uint32_t n, uint32_t gs, uint32_t nb,
                             int8_t *xq, float *xs, hipStream_t st);
uint32_t gemv_q80_partials(const GemvArgs &a);

// ---- routing (route.hip): which kernel a projection launch goes to ------------------------------------------------------------
enum RouteKind : uint32_t {
    ROUTE_GEMV = 0,        // one GEMV launch (FP32 / Q80 SLAB or STREAM), activation quantized in its prologue
    ROUTE_GEMV_PREQ,       // Q80: row-major quantizer launch + GEMV reading the quantized rows (2..8 sequences on large inputs)
    ROUTE_GEMV_SLICED,     // more than 8 sequences through the GEMV kernels in groups of 8
    ROUTE_Q4K,
    ROUTE_RESERVED,        // (round 4's G6 MODE P; the value stays so that the route numbers the tests read do not move)
    // the batched Q80 routes: fragment-order activations (quantizer launch unless frag_ready) + the kernel gemm_q80_plan() names
    ROUTE_FRAG_G6,         // Q80_GEMM_G6S | Q80_GEMM_G6F
    ROUTE_FRAG_OLD,        // Q80_GEMM_GC | Q80_GEMM_G2: the reference's group order
    ROUTE_FRAG_G7,         // Q80_GEMM_G7 | Q80_GEMM_G7K
    ROUTE_Q4K_GEMM,        // Q4K, 9..64 tokens: the staged-group quantizer launch + the int8 MFMA GEMM (gemm_q4k.hip)
    ROUTE_F32_GEMM,        // FP32, 9..64 tokens: the activation prologue launch + the FP32 MFMA GEMM (gemm_f32.hip)
};
inline bool route_takes_fragments(RouteKind k) { return k == ROUTE_FRAG_G6 || k == ROUTE_FRAG_OLD || k == ROUTE_FRAG_G7; }
inline bool route_takes_attn_parts(RouteKind k) { return k == ROUTE_GEMV || k == ROUTE_Q4K || k == ROUTE_Q4K_GEMM; }     // (Q4K GEMM: its quantizer launch combines)
struct Q80Route {
    uint32_t quant; int cus;
    uint32_t mfma_min_nb;  // sequences from which the small Q80 matrices and every Q4K matrix take the batched (MFMA GEMM) route (9; NANO_MFMA_MIN_NB)
    int8_t *gq; float *gxs;  // fragment-order activation scratch (nullptr: no batched route)
    uint8_t *q4x; size_t q4x_bytes;   // Q4K: scratch for the staged groups of a launch's sequences (n bytes each: 2 .. 8 gemv_q4k_chunk.hip, 9 .. 64 gemm_q4k.hip), or nullptr
    uint32_t f32_min_nb;   // FP32: sequences from which a projection takes the MFMA GEMM (gemm_f32.hip); 0 or > 64: never
    float *f32x; size_t f32x_floats;  // FP32: scratch for the operand-order activations of a GEMM launch, or nullptr
};
RouteKind route_kind(const Q80Route &r, const GemvArgs &a, Q80GemmPlan *gp = nullptr);   // gp: the plan behind a ROUTE_FRAG_* answer
// The slices route_projection() cuts a GEMV launch of a.nb sequences into (FP32; Q4K; Q80, the routes that end in the GEMV kernels:
// ROUTE_GEMV, ROUTE_GEMV_PREQ, ROUTE_GEMV_SLICED): per = sequences of every slice but the last, launches = their number.  Every
// workgroup holds the activations of all its sequences in LDS, so groups of 8 wherever 8 fit a CU's LDS (gemv_*_fit_batch()), fewer per
// launch on long rows; Q4K: 8 where the chunk form takes min(nb, 8) sequences, whose activations are staged once.  Per sequence nothing
// changes: the kernels are bit for bit per sequence whatever the capacity.  false: not even one sequence fits, or the shape is refused
// (hipErrorInvalidValue before any launch)
bool route_gemv_slices(uint32_t quant, const GemvArgs &a, uint32_t *per, uint32_t *launches);
// the fields route_projection() itself writes into `a` before it asks route_kind() or launches (cus, the Q4K scratch): written here only
void route_fill(const Q80Route &r, GemvArgs &a);
// arg-max pairs per sequence the launch of `a` is asked for (a.tile_max) and writes, 0: not asked -- the one condition and the one count
// of the step's classifier and of the operator; a.tile_max null on entry
uint32_t route_partials(const Q80Route &r, GemvArgs a);
hipError_t route_projection(const Q80Route &r, GemvArgs &a, hipStream_t st);
uint32_t route_norm_order(const GemvArgs &a);
bool route_is_wide(const GemvArgs &a);

// ---- attention ------------------------------------------------------------------------------------
// up to attention_split_cap() (default 32, capacity 64) splits of a range beyond attention_wide_from() positions (default 2048; <= 8
// below, which the Wo GEMV's prologue combines: attention_nsplit())
constexpr uint32_t ATTN_MAX_NSPLIT = 64;
// the KV cache's element format (AttnArgs::kv_half, AttnPlan::kv_half, NanoAttnDecodeDesc::kv_half, NanoHipModel::kv_half): FP32 rows, or
// opt-in FP16 / FP8 (OCP e4m3fn, scale 1) rows -- 4, 2, 1 bytes per element
enum : uint32_t { KV_FMT_F32 = 0, KV_FMT_F16 = 1, KV_FMT_FP8 = 2 };
inline uint32_t kv_fmt_bytes(uint32_t fmt) { return fmt == KV_FMT_FP8 ? 1u : fmt == KV_FMT_F16 ? 2u : 4u; }
uint32_t attention_wide_from();
uint32_t attention_split_cap();
struct AttnArgs {
    const float *q;         // [nb][q_dim] raw q from the QKV GEMV (normed + roped in LDS, head-local)
    float *q_out;           // optional [nb][q_dim]: finished q written back (debug / traces), or nullptr
    const float *kraw;      // [nb][kv_dim] raw k of the current position (nullptr: k row already final in cache)
    float *kcache;          // [nb][L][S][kv_dim]
    float *vcache;
    const uint32_t *pos;    // [nb]
    const float *q_norm;    // [hd] for this layer or nullptr
    const float *k_norm;
    const float *rope_cos;  // [rows][hd/2] or nullptr (no rope)
    const float *rope_sin;
    const float *rope_cur;  // optional [nb][2][hd/2]: the rows of pos[b], staged by the embed kernel (else read from the tables)
    float *out;             // nsplit > 1: [nb][nsplit][q_dim] UNNORMALISED partial outputs  sum_t exp(s_t - m) v_t
    float *ml;              // nsplit > 1: [nb][n_head][nsplit][2]  (m = max score of the split, l = sum exp(s_t - m))
    float *xba_out;         // nsplit == 1: [nb][q_dim] final (normalised) head outputs
    uint32_t nsplit;        // timestep blocks are dealt round-robin to `nsplit` workgroups per (KV group, sequence)
    uint32_t range_hint;    // host's upper bound of the attended range (>= pos+1 of every sequence; S when not causal)
    uint32_t layer, n_layer, S, hd, n_head, n_kv_head, q_dim, kv_dim;
    uint32_t rope_qwen3;    // 1: (i, i+hd/2) pairs, 0: adjacent pairs
    uint32_t is_causal;
    uint32_t cache_bstride_rows;   // = L*S rows between slots (in units of kv_dim floats)
    uint32_t fixed_range;          // op-test mode: attend over rows [0, fixed_range) of an externally filled cache
    uint32_t prep_only;            // 1: finish and store the k row of pos[b] (norm + RoPE), then return (batched prefill, pass 1)
    uint32_t kv_half;              // KV_FMT_*: 1 / 2 = kcache / vcache hold FP16 / FP8 elements (opt-in); the fresh v row then comes from vraw
    const float *vraw;             // FP16 / FP8 cache: [nb][kv_dim] v of the current position from the QKV GEMV (FP32 scratch), else nullptr
    // single-split launches only, optional: the finished output also leaves as Q80 groups of 64 in MFMA B-fragment order (what
    // quant_rows_frag_kernel would make of xba_out), so the batched Wo GEMM needs no quantizer launch.  head_dim % 64 == 0.
    int8_t *xf_out; float *xsf_out;
    // filled by launch_attention(): workgroup x -> q heads so that the workgroups sharing a KV head run on ONE XCD (workgroup
    // index mod 8 = XCD, each XCD has its own L2): x = sub * n_kv_head + kv head, when n_kv_head is a power of two >= 8;
    // kv_log2 = log2(n_kv_head), else 0xffffffff = plain order (x = first head / heads per workgroup)
    uint32_t kv_log2, kvmul_log2;   // kvmul_log2 = log2(n_head / n_kv_head) (decode modes: both head counts are powers of two)
    // PAGED KV cache (opt-in): kcache / vcache are pools [layer][page][64 positions][kv_dim]; a sequence's 64-position
    // block j lives in the page whose first row (page * 64, rows counted inside a layer plane) is pt_rows[slot][j]
    const uint32_t *pt_rows;        // [slots][pt_stride], 0xffffffff = no page; nullptr = the contiguous cache
    const uint32_t *kvrow;          // [nb] pool row of position pos[b] (staged by the embed kernel next to the RoPE row)
    uint32_t pt_stride, pt_bstride; // entries per slot; entries between the sequences of this launch (0: batched prefill, one slot)
    uint32_t pool_rows, _pad6;      // rows of one layer plane = pages * 64
    uint32_t *err;          // sticky error word (as GemvArgs::err)
    unsigned long long *stamps;   // measurement builds only (NANO_STAMPS): per-workgroup phase stamps, or nullptr
    // RAGGED steps (nano_hip_step_rows): row b is position pos[b] of KV slot row_slot[b] -- its cache base is row_slot[b] *
    // cache_bstride_rows rows into kcache / vcache (paged: its table row pt_rows + row_slot[b] * pt_stride; pt_bstride is not read);
    // q / kraw / vraw / out / ml / xba_out / pos / kvrow / rope_cur stay indexed by the row.  On an FP32 cache vraw, where set, is stored
    // to the row's v row like the FP16 cache's.  nullptr: the two fixed maps above.  Set: launch_attention() runs the attention_rows_kernel
    // instantiations (the same body with the map compiled in); the attention_kernel ones never read the field.  Last in the block: no
    // other field's kernarg offset moved.
    const uint32_t *row_slot;
};
hipError_t launch_attention(const AttnArgs &a, uint32_t nb, hipStream_t st);
// the attention_kernel<LPR, QV, KVM, MODE, KVH, PG, NPT, W16> launch_attention() runs for `a` and nb sequences, and the workgroup order
// it fills in (kv_log2 / kvmul_log2 of AttnArgs); the launcher takes every choice from here.  false: the arguments are refused.
// kv_half: the element format (KV_FMT_*); w16: the wide load form ran (FP16 rows only: 16-byte loads, two float4 slots each).
struct AttnPlan { uint32_t mode, lpr, qv, kvm, npt, w16, paged, kv_half, nsplit, kv_log2, kvmul_log2; };
bool attention_plan(const AttnArgs &a, uint32_t nb, AttnPlan *p);
hipError_t launch_attention_fp8(const AttnArgs &a, const AttnPlan &p, uint32_t nb, hipStream_t st);   // launch_attention()'s FP8 half (attn_fp8.hip)
// q | k | v projection of one sequence + decode attention as ONE launch (gemv.hip dispatches on the weight format -- Q80 group size 64:
// gemv_q80_impl.h, Q4K: gemv_q4k_chunk.hip, round 6, both with Qwen3 attention; FP32: gemv_f32.hip, the plain mode): the attention workgroups
// wait for q / k / v as 8-byte {tag, value} granules in `hand` (q_dim + 2 kv_dim entries); tag = the step's tick * 128 + layer1 (device_common.h)
// The launch launch_qkv_attn_fused() issues: qkv_attn_fused_kernel<nv, upw> (Q80, the product-table body) | qkv_attn_fused_wf_kernel
// (Q80, rows of one chunk: the in-wave fold; nv = upw = 1) | q4k_qkv_attn_fused_kernel<d> (nv = 1) | f32_qkv_attn_fused_kernel<qv> (nv = upw = 1), on `threads` threads
// x (ngemv projection workgroups of rw rows -- wg[s] on tensor s -- followed by n_attn attention workgroups) with lds_bytes of dynamic LDS.
// qkv_attn_fused_plan() makes every choice, the launchers take them from it; false: the launch is refused (the step issues the two plain
// launches) -- a plan names a built instantiation or does not exist.  Host arithmetic on shape fields; of the pointers only null-or-not is read.
enum : uint32_t { FUSED_KERNEL_NONE = 0, FUSED_KERNEL_Q80_TABLE = 1, FUSED_KERNEL_Q80_WF = 2, FUSED_KERNEL_Q4K = 3, FUSED_KERNEL_F32 = 4 };
constexpr uint32_t FUSED_LDS_MAX = 64 * 1024;
struct QkvAttnFusedPlan {
    uint32_t kernel, nv;
    uint32_t upw, d, qv;                        // Q80: UPW, FP32: 1; Q4K: D; FP32: QV (1: head_dim <= 32, 2: above); the others 0
    uint32_t threads, n_attn, ngemv, lds_bytes;
    uint32_t rw, wg[3], rounds;                 // rows of a projection workgroup, its workgroups per tensor (FP32: all in wg[0]); Q4K: the chunk plan's rounds
};
bool qkv_attn_fused_plan(uint32_t quant, const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan *p);
inline bool qkv_attn_fused_supports(uint32_t quant, const GemvArgs &ga, const AttnArgs &aa) { return qkv_attn_fused_plan(quant, ga, aa, nullptr); }
hipError_t launch_qkv_attn_fused(uint32_t quant, const GemvArgs &ga, const AttnArgs &aa, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st);
// Wo + W1|W3 of one sequence in ONE launch (gemv_q80_impl.h wo_w13_fused_kernel): x reaches W1|W3 as granules of the same launch.
// The launch: wo_w13_fused_kernel<role, wf, wfc> on wb workgroups (the first wa also run Wo's rows: rw_a and rw_b rows each) of 512 threads,
// one float4 item per thread and one unit per wave in both bodies; role R_RESID | R_RESID_COMBINE (gemv_common.h: 2 | 3); wf 1: W1|W3's rows
// of one chunk folded in the wave; wfc 2: Wo's rows of two chunks likewise, else 0; cw 1: wo_w13_fused_cw_kernel<wf, wfc>, the combine role with
// the splits' weights made inside each wave (gemv_q80_host.h combine_wave_shape()).  wo_w13_fused_plan() makes every choice; false: refused.
// sig, threads, nv_a .. upw_b are the constants 3, 512, 1, 1, 1, 1 of that one form: words of the plan queries (nano_mi355x.h).
struct WoW13FusedPlan {
    uint32_t sig, threads, role, wf, wfc;
    uint32_t nv_a, upw_a, nv_b, upw_b;
    uint32_t wa, wb, lds_bytes;
    uint32_t rw_a, rw_b;
    uint32_t cw;                                // 1: wo_w13_fused_cw_kernel<wf, wfc> -- Wo's split combine with in-wave weights, live splits only (role R_RESID_COMBINE)
};
bool wo_w13_fused_plan(const GemvArgs &wo, const GemvArgs &w13, WoW13FusedPlan *p);
inline bool wo_w13_fused_supports(const GemvArgs &wo, const GemvArgs &w13) { return wo_w13_fused_plan(wo, w13, nullptr); }
hipError_t launch_wo_w13_fused(const GemvArgs &wo, const GemvArgs &w13, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st);
// the attention side of the fused one-sequence launches: decode attention on an FP32 contiguous cache, one head per workgroup, two timestep
// blocks in flight -- Qwen3's at head_dim 128 (Q80, Q4K), or `plain` (FP32 models): no q / k norm, adjacent-pair RoPE (Nano), head_dim <= 64;
// qr / kr / vr = rows of the q | k | v segments
inline bool fused_attn_side_ok(const AttnArgs &aa, uint32_t qr, uint32_t kr, uint32_t vr, bool plain) {
    if (plain ? (aa.hd < 4u || aa.hd > 64u || aa.hd % 4u || aa.q_norm || aa.k_norm || aa.rope_qwen3) : (aa.hd != 128u || !aa.q_norm || !aa.k_norm || !aa.rope_qwen3)) return false;
    if (!aa.rope_cos || !aa.rope_cur || !aa.kraw || aa.fixed_range || !aa.is_causal || aa.q_out) return false;
    if (aa.kv_half || aa.pt_rows || aa.prep_only || aa.xf_out || aa.nsplit == 0 || aa.nsplit > 8u) return false;
    const uint32_t kv_mul = aa.n_kv_head ? aa.n_head / aa.n_kv_head : 0u;
    if (!aa.n_kv_head || (aa.n_kv_head & (aa.n_kv_head - 1u)) || !kv_mul || (kv_mul & (kv_mul - 1u))) return false;
    if ((uint64_t)aa.n_head * aa.nsplit > 256u) return false;                   // (beyond: the attention launcher puts several heads in a workgroup)
    if (aa.range_hint > aa.nsplit * 2u * 32u) return false;                     // (more than one round: the launcher may pick four blocks in flight)
    return aa.q_dim == qr && aa.kv_dim == kr && aa.kv_dim == vr && aa.q_dim == aa.n_head * aa.hd;
}
// the tick words and the zeroed granule buffers of the fused launches, for a model and for the operators alike (backend.hip)
hipError_t handoff_alloc(uint32_t **tick, unsigned long long **hand, size_t granules, unsigned long long **hand2, size_t granules2);
uint32_t attention_nsplit(uint32_t range_hint, uint32_t hd);
hipError_t launch_attn_combine(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit, hipStream_t st);
hipError_t launch_attn_combine_tokens(const float *part, const float *ml, float *out, uint32_t n_head, uint32_t hd, uint32_t nsplit, uint32_t nb,
                                      int8_t *xf_out, float *xsf_out, hipStream_t st);   // xf_out: also Q80 fragments (AttnArgs::xf_out), or nullptr

// ---- strict-parity kernels (strict.hip): every float reduction in the reference's own order --------------
struct StrictAttnArgs {
    float *q;               // [nb][q_dim] raw q, finished (norm + RoPE) in place
    const float *kraw;      // [nb][kv_dim] raw k of the current position
    float *kcache, *vcache; // [slots][L][S][kv_dim]
    const uint32_t *pos;    // [nb]
    const float *q_norm, *k_norm;          // [hd] of this layer or nullptr
    const float *rope_cos, *rope_sin;      // [rows][hd/2]
    float *att;             // [nb][n_head][S] scores -> probabilities
    float *xba;             // [nb][q_dim] head outputs
    uint32_t n_head, n_kv_head, hd, q_dim, kv_dim, layer, n_layer, S;
    uint32_t slot0;         // KV slot of sequence 0 of this step (sequence b lives in slot0 + b)
    uint32_t rope_qwen3, is_causal;
    uint32_t fold_prep;     // exact.hip's one-launch attention only: 1 = it also does launch_strict_qk's work (q / k [norm] + RoPE, k row store)
};
hipError_t launch_strict_rmsnorm(float *o, const float *x, const float *w, uint32_t n, uint32_t nvec, uint32_t x_stride, uint32_t o_stride, hipStream_t st);
hipError_t launch_strict_qk(const StrictAttnArgs &a, uint32_t nb, hipStream_t st);
hipError_t launch_strict_attention(const StrictAttnArgs &a, uint32_t nb, hipStream_t st);
hipError_t launch_strict_swiglu(float *hb, const float *hb2, uint32_t n, uint32_t nb, uint32_t bstride, hipStream_t st);
hipError_t launch_strict_matmul_f32(float *out, const float *x, const float *w, uint32_t n, uint32_t d, uint32_t nb, uint32_t x_bstride,
                                    uint32_t out_bstride, uint32_t out_pstride, const uint32_t *pos, int resid, hipStream_t st);

// ---- exact-mode kernels (exact.hip): strict.hip's bits from kernels made to be replayed -----------------
// rmsnorm with the sum of squares in index order (the terms staged in LDS); scores + softmax + weighted V of one layer in ONE launch
// with att[range] in LDS.  exact_attention_fits(): att[max_range] fits that launch's LDS -- where it does not, the step keeps
// launch_strict_attention (att in global memory).  StrictAttnArgs as for strict.hip (att is not read by the one-launch kernel).
hipError_t launch_exact_rmsnorm(float *o, const float *x, const float *w, uint32_t n, uint32_t nvec, uint32_t x_stride, uint32_t o_stride, hipStream_t st);
bool exact_attention_fits(uint32_t hd, uint32_t max_range);
hipError_t launch_exact_attention(const StrictAttnArgs &a, uint32_t nb, hipStream_t st);

// ---- LoRA side branches (lora.hip) -------------------------------------------------------------------
// what the two launches cannot run, or nullptr: E % 4 (float4 loads of the A rows and of the LDS copy), rank 0, and dynamic LDS beyond the
// 64 KiB a launch may ask for (qkv: E + 3 rank + 32 floats).  Asked by nano_hip_lora_attach / _table_set and by the operators; the launches refuse too.
const char *lora_shape_error(uint32_t E, uint32_t rank);
// One kernel pair.  A row's "module" is the descriptor of its KV slot: row b belongs to slot slot0 + b * slot_stride (1: a decode step,
// 0: a prefill chunk) and takes its pointers, rank and alpha from that slot's descriptor in device memory -- read when the kernel runs,
// so a captured launch follows a rebinding.  An attached module (nano_hip_lora_attach) is the same descriptor in every slot; a table binds
// one per slot.  rank 0 = no module: the qkv launch returns before its first barrier and writes nothing, the o launch stores -0.0f into
// its o1 row (r + (-0.0f) has r's bits for every float r: the Wo epilogue then leaves x += Wo xba).
struct LoraSlotDesc {
    const float *t[8];      // qa qb ka kb va vb oa ob of the module, each [L][...] (the layout of nano_hip_lora_attach's parameter block)
    uint32_t rank, alpha;   // rank 0: no module
};
struct LoraRowsArgs {
    const LoraSlotDesc *desc;                      // [slots]
    const float *x;         // qkv: residual stream x [nb][E]; o: attention output xba [nb][E]
    const float *norm_w;    // qkv: rms_attn weight of the layer
    float *q, *kraw, *v;    // qkv: in-place targets (v = cache base of slot 0 / of the prefill slot); o: q = o1 out
    const uint32_t *pos;
    uint32_t E, KD, layer, slot0, slot_stride, v_bstride, max_rank, _pad;   // max_rank sizes the launch's LDS: the largest rank a descriptor may name
};
hipError_t launch_lora_qkv_rows(const LoraRowsArgs &a, uint32_t nb, hipStream_t st);
hipError_t launch_lora_o_rows(const LoraRowsArgs &a, uint32_t nb, hipStream_t st);

// ---- small kernels ----------------------------------------------------------------------------------
struct EmbedArgs {
    const void *tok;        // FP32 float[V][E] | Q80 int8[V][E] | Q4K blocks
    const float *tok_s;     // Q80 scales
    const uint32_t *tokens; // [nb]
    float *x;               // [nb][E]
    uint32_t E, gs, quant, x_bstride;
    // the step's first kernel also stages the RoPE row of each sequence's position at a FIXED address, so that
    // the attention kernels need no pos-dependent load: rope_cur[b] = { cos[pos[b]][0..half), sin[pos[b]][0..half) }
    const float *rope_cos; const float *rope_sin; const uint32_t *pos; float *rope_cur; uint32_t half, _pad;
    // paged KV cache: kvrow[b] = pt_rows[b * pt_bstride + pos[b] / 64] + pos[b] % 64 (the pool row the step writes), or nullptr
    const uint32_t *pt_rows; uint32_t *kvrow; uint32_t pt_bstride, pt_entries;   // pt_entries: table entries per slot (a position beyond them stages nothing)
    // the step's first kernel also advances the model's hand-off epoch (device_common.h: tick[0] += 1, workgroup 0), or nullptr
    uint32_t *tick;
    // ragged steps: row b belongs to KV slot row_slot[b] -- kvrow[b] = pt_rows[row_slot[b] * pt_entries + pos[b] / 64] + pos[b] % 64
    // (pt_bstride is not read); nullptr: row b is slot b (x pt_bstride)
    const uint32_t *row_slot;
};
hipError_t launch_embed(const EmbedArgs &a, uint32_t nb, hipStream_t st);

// argmax over logits[b][V] -> out[b]; optionally advances the decode loop state:
// tokens[b] = argmax, pos[b] += 1, trace[step*nb + b] = argmax
struct ArgmaxArgs {
    const float *logits; uint32_t V, bstride;
    uint32_t *out;
    uint32_t *tokens; uint32_t *pos; uint32_t *trace; const uint32_t *pos0; uint32_t nb;   // trace[(pos-pos0)*nb + b]
    const float *tile_max; uint32_t ntiles;     // optional (max, row) partials from the classifier GEMV
    // greedy loop only (tokens != nullptr): the SAME kernel then embeds the token it picked at its next position -- the next
    // step's first kernel (embed) and its launch boundary are gone.  emb.x == nullptr: not fused.  rope_rows: rows of the RoPE
    // tables (the position after the last one has no row: nothing is staged for it)
    EmbedArgs emb; uint32_t rope_rows, _pade;
};
hipError_t launch_argmax(const ArgmaxArgs &a, uint32_t nb, hipStream_t st);

// ---- row statistics of logits for given targets (score.hip): one NanoHipTokenScore per row ----
constexpr uint32_t SCORE_TILE = 4096;                      // logits per tile: the reduction shape is a function of V alone
struct ScorePartial { float m, s; uint32_t idx, cnt; };    // of one tile: maximum, sum of expf(l - m), first index of m, the tile's share of rank
struct ScoreArgs {
    const float *logits; uint32_t V, ntiles;               // [rows][V], row stride V; ntiles = score_tiles(V)
    const uint32_t *targets;                               // [rows], every one < V; nullptr: each row's own arg-max
    ScorePartial *part;                                    // scratch [rows][ntiles]
    NanoHipTokenScore *out;                                // [rows]
};
uint32_t score_tiles(uint32_t V);
// two launches: the tiles, then one wave per row
hipError_t launch_score_rows(const ScoreArgs &a, uint32_t rows, hipStream_t st);

// ---- the k most probable tokens of every row, with their log-probs (topk.hip): k NanoHipTopEntry per row ----
struct TopkArgs {
    const float *logits; uint32_t V, ntiles, k;            // [rows][V], row stride V; ntiles = score_tiles(V); 1 <= k <= min(NANO_TOPK_MAX, V)
    unsigned long long *part;                              // scratch [rows][ntiles][k]: every tile's best keys, in order (0: none)
    const NanoHipTokenScore *scores;                       // [rows]: launch_score_rows' records of the same rows (queued first on the same stream): lse
    NanoHipTopEntry *out;                                  // [rows][k]
};
// two launches: the tiles (score.hip's tiles), then one workgroup per row; rows <= 65535
hipError_t launch_topk_rows(const TopkArgs &a, uint32_t rows, hipStream_t st);

// ---- text embeddings: a pass's final-norm rows pooled per segment (pool.hip) ----
constexpr uint32_t POOL_THREADS = 256, POOL_MAX_ROWS = 256;  // threads of a workgroup; the most rows a pass may hold (the inverse RMS of each in LDS)
// a workgroup's 4 words: { segment, first entry of its row list in `lists`, rows in the list | POOL_BEGUN | POOL_ENDS, the segment's row count }
constexpr uint32_t POOL_GROUP_WORDS = 4, POOL_N_MASK = 0x3fffffffu, POOL_BEGUN = 0x40000000u, POOL_ENDS = 0x80000000u;
struct PoolArgs {
    const float *x; uint32_t x_stride, rows_max;           // the pass's rows (residual rows; w == nullptr: rows already normed); rows_max: rows of the pass
    const float *w;                                        // [n_embd] the final norm's weights, or nullptr: the ordered form (pool.hip)
    const uint32_t *groups, *lists;                        // [workgroups][POOL_GROUP_WORDS]; pass rows, each list ascending (= ascending position)
    float *acc;                                            // [n_segs][dim rounded up to 4] running sums of segments that straddle passes
    float *out;                                            // [n_segs][dim]
    uint32_t n_embd, dim, mean, normalize;                 // dim: 1 .. n_embd; mean: 0 the (one) listed row itself, 1 sum / count
};
// one launch: one workgroup per entry of groups
hipError_t launch_pool_rows(const PoolArgs &a, uint32_t n_groups, hipStream_t st);

hipError_t launch_rmsnorm(float *out, const float *x, const float *w, uint32_t n, hipStream_t st);
hipError_t launch_quantize_q80(const float *x, uint32_t n, uint32_t gs, int8_t *q, float *s, hipStream_t st);
hipError_t launch_quantize_q4k(const float *x, uint32_t n, uint8_t *blocks, hipStream_t st);
hipError_t launch_swiglu(float *hb, const float *hb2, uint32_t n, hipStream_t st);
hipError_t launch_rope(float *head, uint32_t hd, const float *fcr, const float *fci, int qwen3, hipStream_t st);
hipError_t launch_stream_read(const void *buf, size_t bytes, float *sink, hipStream_t st);
hipError_t launch_stream_read_masked(const void *buf, size_t bytes, float *sink, uint32_t xcd_mask, uint32_t wgs, hipStream_t st);

// ---- KV-cache row copies (kv_copy.hip): the contiguous fork, the partial block of a paged fork, copy-on-write of a shared page ----
// A job moves `rows` cache rows inside every layer plane of K and of V from src_row to dst_row; the trailing rows - keep_rows rows of the
// destination are written as zero.  gstart[0 .. n_groups] cuts the job list into groups that share src_row / rows / keep_rows: a
// workgroup loads the source once and stores it to every destination of its group.  Layer plane l starts l * plane_bytes into k / v.
struct KvCopyJob { uint32_t src_row, dst_row, rows, keep_rows; };
struct KvCopyArgs {
    void *k, *v;
    uint64_t plane_bytes;
    uint32_t row_bytes;                          // a multiple of 8; 16-byte vectors when a multiple of 16
    uint32_t n_groups, cx, _pad;                 // cx: workgroups per group and plane (set by the launcher)
    const KvCopyJob *jobs; const uint32_t *gstart;            // device memory
};
hipError_t launch_kv_copy(KvCopyArgs a, uint32_t n_layer, uint32_t max_rows, uint32_t cus, bool nt_stores, hipStream_t st);

// ---- KV images (kv_image.hip): a slot's rows to / from a staging buffer in image order (kv_image.h) ----
// A job starts at a 64-position block boundary and covers `rows` positions: cache rows cache_row .. (counted inside a layer plane, the
// slot's base folded in) on one side, the blocks at staging_off .. on the other -- block i of the job at staging_off + i * 64 * n_layer
// * 2 * row_bytes, its runs holding min(64, rows - 64 i) rows each.  Pack (cache -> staging): the job's trailing zero_rows rows are not
// read but staged as zero (a block the slot has not mapped: zero_rows == rows, cache_row is not used).  Unpack (staging -> cache): the
// zero_rows cache rows behind the job's `rows` are written as zero (the rest of a partial last page).  job_blocks: blocks of the
// longest job (contiguous cache: one job per staging chunk; paged: one job per block).
struct KvImageJob { uint32_t cache_row, staging_off, rows, zero_rows; };
struct KvImageArgs {
    void *k, *v, *staging;
    uint64_t plane_bytes;
    uint32_t row_bytes, n_layer;
    uint32_t n_jobs, job_blocks, cx, _pad;       // cx: workgroups per block and plane (set by the launcher)
    const KvImageJob *jobs;                      // device memory
};
hipError_t launch_kv_image(KvImageArgs a, bool pack, uint32_t cus, hipStream_t st);

// ---- device-side sampler (sampler.hip) ----
constexpr uint32_t SAMPLE_CHUNK = 256;            // softmax numerators per chunk function (one wave x float4)
constexpr uint32_t SAMPLE_MAX_CHUNKS = 1024;      // vocabularies up to 262144
constexpr uint32_t SAMPLE_MAX_CANDIDATES = NANO_SAMPLE_MAX_CANDIDATES;
constexpr uint32_t SAMPLE_BINS = 256;             // histogram of the softmax numerators: 8 bins per binade, 2^0 .. 2^-31
struct SampleArgs {
    const float *logits; uint32_t V;
    uint32_t nch;                                 // chunks, rounded up to a multiple of 4; y/e hold nch*256 floats
    float *y, *e;                                 // penalised+tempered logits, softmax numerators
    const uint8_t *seen;                          // null when the penalty is 1
    float penalty, temperature, top_p, cutoff, coin;
    uint32_t top_k;                               // 0 = off; else the sorted list is cut to its first top_k entries (nano_mi355x.h)
    // the row's logit edit (nano_mi355x.h "logit edits"), device memory: allow = ceil(V / 32) mask words, null = every token allowed;
    // bias = n_bias entries of distinct tokens, any order.  Both enter the prep kernel's y only; the logits stay as they are.
    const uint32_t *allow; const NanoHipLogitBias *bias; uint32_t n_bias;
    float *pmax;                                  // [nch/4] workgroup maxima of the prep kernel
    uint32_t *ncand, *ndrop, *dropmax, *bstar;    // accumulators, left at 0 by the last kernel (bstar: set by propagate)
    uint32_t *bin_cnt; unsigned long long *bin_mass;      // [SAMPLE_BINS], likewise
    float *approx; uint32_t *spec; uint2 *fn;     // per chunk: approximate sum, guessed exponent field, chunk function
    float *sum;
    unsigned long long *cand; uint32_t cap;
    NanoHipSample *res;
    // second phase, wide nuclei (sampler_wide.hip): every candidate as a key, the sorted keys, the sorted probabilities
    unsigned long long *wide_in, *wide_out; float *wide_p; uint32_t wide_cap;
};
// The sampler's rows (a one-row call is a batch of one): `a` is row 0's view -- its scratch pointers (y, e, seen, pmax, cells, bins,
// approx, spec, fn, cand) are row 0's, and row r's lie `rstride` bytes further per row; row r's logits are `lstride` floats further,
// its result is res[r], its parameters rp[r].  The wide-phase pointers of `a` are not used.
struct SampleRowParams {
    float penalty, temperature, top_p, cutoff, coin; uint32_t top_k;
    const uint32_t *allow; const NanoHipLogitBias *bias; uint32_t n_bias, _pad;      // the row's edit (device pointers; null / 0 = none)
};
struct SampleRows {
    SampleArgs a;
    const SampleRowParams *rp;
    uint64_t rstride;
    uint32_t lstride, _pad;
};
// row r's own view, a SampleArgs (device: the kernels; host: the wide phase of one row); the seen plane only when the penalty is not 1
__host__ __device__ inline SampleArgs sample_row(const SampleRows &b, uint32_t r, const SampleRowParams &p) {
    SampleArgs a = b.a;
    const uint64_t o = (uint64_t)r * b.rstride;
    // offset as a byte pointer, not through an integer: the compiler then still sees a global pointer (global_*, not flat_* accesses)
    auto mv = [o](auto *ptr) { return reinterpret_cast<decltype(ptr)>(const_cast<char *>(reinterpret_cast<const char *>(ptr)) + o); };
    a.logits = b.a.logits + (size_t)r * b.lstride;
    a.y = mv(a.y); a.e = mv(a.e); a.pmax = mv(a.pmax);
    a.ncand = mv(a.ncand); a.ndrop = mv(a.ndrop); a.dropmax = mv(a.dropmax); a.bstar = mv(a.bstar); a.sum = mv(a.sum);
    a.bin_cnt = mv(a.bin_cnt); a.bin_mass = mv(a.bin_mass);
    a.approx = mv(a.approx); a.spec = mv(a.spec); a.fn = mv(a.fn); a.cand = mv(a.cand);
    a.seen = p.penalty != 1.0f ? mv(b.a.seen) : nullptr;
    a.res = b.a.res + r;
    a.penalty = p.penalty; a.temperature = p.temperature; a.top_p = p.top_p; a.cutoff = p.cutoff; a.coin = p.coin; a.top_k = p.top_k;
    a.allow = p.allow; a.bias = p.bias; a.n_bias = p.n_bias;
    return a;
}
// The mask bits of tokens i0 .. i0 + 3 (i0 a multiple of 4: one nibble of one word), 0xF for a row without a mask.  Nothing is read for
// i0 >= V, so the last word read is word ceil(V / 32) - 1; bits of tokens >= V inside the nibble are the caller's to ignore (i < V).
// The prep kernel, the candidate filter and the wide phase's candidate test all ask this one function: the branch is row-uniform.
__device__ __forceinline__ uint32_t sample_allow_nibble(const SampleArgs &a, uint32_t i0) {
    if (!a.allow) return 0xFu;
    return i0 < a.V ? (a.allow[i0 >> 5] >> (i0 & 31u)) & 0xFu : 0u;
}
hipError_t launch_sample_rows(const SampleRows &b, uint32_t rows, bool softmax, bool edited, hipStream_t st);      // edited: some row has an edit
hipError_t launch_seen_set(const uint32_t *ids, uint32_t n, uint8_t *seen, hipStream_t st);
size_t sample_wide_temp_bytes(uint32_t n);                            // scratch of the device sort of n keys
hipError_t launch_sample_wide(const SampleArgs &a, void *temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_sample_wide_cut(const SampleArgs &a, hipStream_t st);   // (its last three kernels: sampler.hip)   // after the row's pick reported NANO_SAMPLE_FALLBACK

// ---- greedy decode with lookup drafts (lookup.hip): what happens between two steps of the loop, one workgroup ----
// Behind a step that fed fed[0..nb) at positions n-1 .. n-2+nb and left the row arg-maxes amax[0..nb): accept the draft rows the
// arg-maxes confirm, clip to the ids still wanted, stop at the stop token, append to the history, look the new suffix up in the history
// and stage the next step's rows (DESIGN.md section 10 has the definitions; tests/lookup_ref.py restates them).  nb = 0: no step has
// run yet -- lookup, gate and staging only.
constexpr uint32_t LOOKUP_MAX_ROWS = 16;          // rows of a verify chunk: the fed id + at most 15 drafted ones
constexpr uint32_t LOOKUP_MAX_NGRAM = 4;
enum { LOOKUP_REC_EMITTED = 0, LOOKUP_REC_ACCEPTED, LOOKUP_REC_NB_NEXT, LOOKUP_REC_N, LOOKUP_REC_MATCH_LEN, LOOKUP_REC_MATCH_END,
       LOOKUP_REC_DONE, LOOKUP_REC_LEFT, LOOKUP_REC_WORDS };
struct LookupArgs {
    uint32_t *hist; uint32_t cap;                 // the sequence's ids, device memory, 16-byte aligned; cap a multiple of 4: nothing is written at or beyond it
    uint32_t *state;                              // [0] n = ids in hist, [1] left = ids still to emit, [2] ids emitted so far (the cursor into trace)
    const uint32_t *fed, *amax; uint32_t nb;      // the step this launch follows (<= LOOKUP_MAX_ROWS rows)
    uint32_t max_draft, ngram_max, ngram_min, stop_token;
    uint32_t seq_limit;                           // min(max_seq_len, RoPE rows): a chunk's last position stays below it
    uint32_t *next_tokens, *next_pos;             // [LOOKUP_MAX_ROWS] the next step's rows (next_tokens may be fed: the fed ids are read first)
    uint32_t *trace; uint32_t trace_cap;          // the call's emitted ids (nullptr: not kept)
    uint32_t *record;                             // [LOOKUP_REC_WORDS]
};
hipError_t launch_lookup_step(const LookupArgs &a, hipStream_t st);

// ---- lookup drafts for several sequences (lookup_rows.hip): what happens between two ragged passes of nano_hip_decode_lookup_rows ----
// Two launches.  lookup_rows_seq_kernel, one workgroup of 256 threads per sequence: lookup.hip's accept / emit / lookup / draft / gate on
// the sequence's own history, its record and its next rows' tokens into stage[i][LOOKUP_MAX_ROWS].  lookup_rows_pack_kernel, one
// workgroup: the live sequences (nb_next > 0) ordered stably by the range hint of position n - 1, the prefix sum of their row counts,
// and the next pass's tokens, positions and row -> slot map in pass order, plus every sequence's first row and row count for the next
// accept (nano_hip_lookup_rows_plan is the host's copy of the same rule).
enum { LOOKUP_ST_N = 0, LOOKUP_ST_LEFT, LOOKUP_ST_CURSOR, LOOKUP_ST_DONE, LOOKUP_ST_WORDS };
constexpr uint32_t LOOKUP_ROW_NONE = 0xffffffffu;  // row_start of a sequence without rows in the pass
struct LookupRowsArgs {
    uint32_t n_seqs;
    uint32_t *hist; uint32_t cap;                 // sequence i's ids: hist + seq_slot[i] * cap (16-byte aligned rows; cap a multiple of 4)
    const uint32_t *seq_slot;                     // [n_seqs] the KV slot of sequence i
    uint32_t *state;                              // [n_seqs][LOOKUP_ST_WORDS] n | ids still to emit | ids emitted so far | finished
    const uint32_t *fed, *amax;                   // the pass these launches follow, in pass order: its tokens and row arg-maxes
    uint32_t *row_start, *nb;                     // [n_seqs] sequence i's first row and row count in that pass (nb 0: none); the pack launch writes the next pass's
    uint32_t max_draft, ngram_max, ngram_min, stop_token;
    uint32_t seq_limit, max_seq_len;              // min(max_seq_len, RoPE rows) | max_seq_len: a range hint is clipped to it
    uint32_t *stage;                              // [n_seqs][LOOKUP_MAX_ROWS] the next rows' tokens of every sequence
    uint32_t *record;                             // [n_seqs][LOOKUP_REC_WORDS]
    uint32_t *trace; const uint32_t *trace_base; uint32_t trace_cap;   // the emitted ids: sequence i's from trace_base[i] on (trace nullptr: not kept)
    uint32_t *next_tokens, *next_pos, *next_slot; // the next pass in pass order (at most n_seqs * (max_draft + 1) rows; never fed / amax's rows before they are read: the pack launch runs behind the sequences')
};
__host__ __device__ inline uint32_t lookup_rows_hint(uint32_t n, uint32_t max_seq_len) {      // nano_hip_rows_plan's row_hint of position n - 1
    const uint32_t h = ((n - 1u + 64u) / 64u) * 64u;
    return h > max_seq_len ? max_seq_len : h;
}
hipError_t launch_lookup_rows_round(const LookupRowsArgs &a, hipStream_t st);

// ---- greedy decode with a draft model (draft.hip): what happens between the two models' steps of a round, one workgroup ----
// A round feeds the target [hist[n-1], d1 .. dD'] at positions n-1 .. n-1+D' (tests/draft_ref.py restates the
// definitions).  One kernel, three roles:
//   STAGE    behind the draft's D' MODE_LOOP steps: their ids (the draft's trace) become rows 1 .. D' of the target's tokens
//   ACCEPT   behind the target's step: accept / clip / stop / append as lookup.hip's, the new dn (positions the draft holds), the next
//            round's row count by the bucket rule, row 0 and the positions of the next round for the target, row 0 for the draft
//   BEGIN    behind a catch-up chunk of the draft (which used its token / position rows): the draft's row 0 once more
enum { DRAFT_ROLE_STAGE = 0, DRAFT_ROLE_ACCEPT = 1, DRAFT_ROLE_BEGIN = 2 };
enum { DRAFT_REC_EMITTED = 0, DRAFT_REC_ACCEPTED, DRAFT_REC_NB_NEXT, DRAFT_REC_N, DRAFT_REC_DN, DRAFT_REC_CURSOR, DRAFT_REC_DONE, DRAFT_REC_LEFT, DRAFT_REC_WORDS };
struct DraftArgs {
    uint32_t role;
    uint32_t *hist; uint32_t cap;                 // as LookupArgs
    uint32_t *state;                              // as LookupArgs
    const uint32_t *fed, *amax; uint32_t nb;      // ACCEPT: the step this launch follows.  STAGE: nb - 1 ids are staged
    const uint32_t *ids;                          // STAGE: the draft's ids [nb - 1]
    uint32_t max_draft, stop_token;
    uint32_t seq_limit;                           // min over both models of (max_seq_len, RoPE rows)
    uint32_t dn;                                  // ACCEPT: positions of the history the draft held before this round
    uint32_t *next_tokens, *next_pos;             // [LOOKUP_MAX_ROWS] the target's rows of the next round
    uint32_t *d_tokens, *d_pos, *d_pos0;          // the draft's row 0, and where its loop's trace index starts (nullptr: there is no draft to stage)
    uint32_t *trace; uint32_t trace_cap;          // as LookupArgs
    uint32_t *record;                             // [DRAFT_REC_WORDS]
};
// rows of the round that starts at a history of n ids with `left` ids to emit (0: none -- left == 0): 1 + D'
__host__ __device__ inline uint32_t draft_round_rows(uint32_t n, uint32_t left, uint32_t max_draft, uint32_t seq_limit) {
    if (left == 0 || n == 0) return 0;
    uint32_t d = max_draft < LOOKUP_MAX_ROWS - 1 ? max_draft : LOOKUP_MAX_ROWS - 1;
    const uint32_t bucket = 63u - (n - 1u) % 64u, room = seq_limit > n ? seq_limit - n : 0u;    // the chunk inside one 64-position bucket; n - 1 + D' < seq_limit
    d = d < bucket ? d : bucket; d = d < left - 1u ? d : left - 1u; d = d < room ? d : room;
    return d + 1u;
}
hipError_t launch_draft_round(const DraftArgs &a, hipStream_t st);

}  // namespace nano
