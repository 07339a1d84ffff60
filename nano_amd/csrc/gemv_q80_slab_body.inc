// gemv_q80_slab_body.inc -- the statements of the SLAB GEMV kernel (gemv_q80_impl.h), included TEXTUALLY into each kernel that runs them:
// the plain gemv_q80_slab_kernel and the fused q | k | v + attention and Wo + W1|W3 kernels.  Textual, not a function taking the argument block by
// reference: routed through a reference the compiler copied the block to scratch in the multi-segment roles and fetched its fields
// late (296 bytes of private memory, the step 25 % slower; tests/test_isa_hygiene.py).  The includer defines
//   SLAB_A      the GemvDev (a by-value kernel parameter, or a member of one)
//   SLAB_BID    the workgroup's index among the GEMV workgroups
//   SLAB_HAND   0 | 1: also store every result as an 8-byte {tag, value} granule (SLAB_HANDV: the SlabHand; SLAB_PTAG: the tag the
//               producers of this launch write -- hand_tag_producer(), unique per (step, layer): a granule of an earlier launch never matches)
//   SLAB_XHAND  0 | 1: the activation arrives as granules written by other workgroups of the SAME launch (SLAB_XHANDV: the SlabHand of
//               that buffer, one entry per activation value; SLAB_CTAG: the tag to wait for): polled after the weight loads are out,
//               instead of loaded at kernel entry
//               (Measured against it and dropped, round 5: two sweeps in flight -- the polls compete with the producers, -2 %; one counter
//               the producers add to -- device-scope read-modify-writes on one address serialise at ~50 ns each: +6 us per layer with 128
//               producers, +12 with 256; one flag per producer polled by one wave per workgroup, then the values by agent-scope loads --
//               the extra round trip costs more than the polls it saves: +1.7 us per layer.  profiles/r05_wo_w13_fused.txt)
//   SLAB_EARLY  (optional, default 0; SLAB_PART 0 only) units of a wave's weights asked for before the activation is quantized, the rest
//               after (0 = all before)
//   SLAB_PART   0: the whole body; 1: declarations + every load of the launch (sections 0-3) only; 2: the rest (sections 4-6) -- a kernel
//               that runs two bodies issues the second one's weight loads (part 1) before it computes the first (wo_w13_fused_kernel)
//   SLAB_WF     (optional, default 0) a compile-time 0 | 1: rows of ONE chunk (n == 1024, group size 64, one sequence, the rmsnorm roles, canonical
//               launches -- the host selects it): every wave folds the rows of its units itself (wave_fold_canon16, gemv_q80_impl.h) and stores
//               them; no product table in LDS, no workgroup barrier after the dots, waves end independently.  R_NORM_SWIGLU: a unit is two rows
//               of W1 plus the same two rows of W3 (the host passes units = ceil(rw / 2)), so the wave has both halves of its SwiGLU pairs
//   SLAB_WFC   (optional, default 0) a compile-time 0 | 2 | 3 | 4: rows of that many WHOLE chunks (n == 1024 SLAB_WFC, group size 64, one sequence,
//               the residual roles -- Wo, W2 --, one weight segment, canonical launches -- the host selects it).  Units, loads and fold threads
//               are the table form's; but every wave folds the chunk of its unit itself to the chunk's two unit sums (wave_fold_canon16_units)
//               and leaves 8 floats (4 rows x 2 sums) in LDS instead of 64 products: behind the barrier the fold thread of a row reads its
//               2 SLAB_WFC unit sums (one or two LDS reads) and adds them in ascending order -- 2 SLAB_WFC - 1 adds where the table's fold
//               has 16 SLAB_WFC - 1 behind 4 SLAB_WFC reads.  (A wave per tile with ALL of its chunks -- no barrier at all -- was built first and
//               lost: the dots and folds of two or three chunks in ONE wave cost more than the barrier, profiles/wave_fold_chunks.txt.)
//   SLAB_CW    (optional, default 0) a compile-time 0 | 1: the split-attention combine with in-wave weights and live splits only (role
//               R_RESID_COMBINE, one sequence, a wave's items cover whole heads -- the host selects it: gemv_q80_host.h combine_wave_shape(),
//               gemv_common.h cw_issue / cw_combine): no weight table in the LDS carve-up, no barrier in front of the quantizer
// and has ROLE, GS, B, NV, UPW, smem, in scope.
#ifndef SLAB_WF
#define SLAB_WF 0
#define SLAB_WF_DEFAULTED 1
#endif
#ifndef SLAB_WFC
#define SLAB_WFC 0
#define SLAB_WFC_DEFAULTED 1
#endif
#ifndef SLAB_EARLY
#define SLAB_EARLY 0
#define SLAB_EARLY_DEFAULTED 1
#endif
#ifndef SLAB_CW
#define SLAB_CW 0
#define SLAB_CW_DEFAULTED 1
#endif
#ifndef SLAB_XHAND_WAIT
#define SLAB_XHAND_WAIT 0u
#define SLAB_XHAND_NAP 0
#define SLAB_XHAND_WAIT_DEFAULTED 1
#endif
// (a unit's weight and scale loads; used by section 2 and -- SLAB_EARLY -- by section 4)
#define SLAB_ISSUE_UNIT(k) do { \
      if constexpr (WFPAIR_) { \
        /* pair unit u: rows 2u, 2u + 1 of W1 (r = 0, 1) and of W3 (r = 2, 3); the lane's scale comes from ONE of the two arrays: both are */ \
        /* asked for, the other one out of range (no traffic, reads as 0), and the bit patterns are OR-ed -- no divergent descriptor */ \
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW; \
        const bool live = u < SLAB_A.units; \
        const __amdgpu_buffer_rsrc_t rw0_ = mkrsrc(w0, live ? rows0 * n : 0u), rw1_ = mkrsrc(SLAB_A.w[1], live ? rows0 * n : 0u); \
        const __amdgpu_buffer_rsrc_t rs0_ = mkrsrc(ws0, live ? rows0 * ng * 4u : 0u), rs1_ = mkrsrc(SLAB_A.ws[1], live ? rows0 * ng * 4u : 0u); \
        const uint32_t lrow = lrow0 + u * 2u, base = lrow * n + (uint32_t)lane * 16u; \
        _Pragma("unroll") \
        for (int r = 0; r < TR; r++) wv[k][r] = bload_w(r < 2 ? rw0_ : rw1_, (u * 2u + (uint32_t)(r & 1) < RW) ? base + (uint32_t)(r & 1) * n : OOB); \
        const uint32_t r_ = (uint32_t)lane & 3u, rr_ = r_ & 1u; \
        const uint32_t so_ = (u * 2u + rr_ < RW) ? ((lrow + rr_) * ng + ((uint32_t)lane >> 2)) * 4u : OOB; \
        const float s0_ = bload_f(rs0_, r_ < 2u ? so_ : OOB), s1_ = bload_f(rs1_, r_ < 2u ? OOB : so_); \
        sv[k][0] = __uint_as_float(__float_as_uint(s0_) | __float_as_uint(s1_)); \
      } else { \
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW; \
        const uint32_t t = (u * SLAB_A.magic_nchunk) >> 16; \
        const uint32_t c = u - t * SLAB_A.nchunk; \
        const uint32_t mat = t >= TPW ? 1u : 0u, tl = t - mat * TPW; \
        const bool live = u < SLAB_A.units; \
        const __amdgpu_buffer_rsrc_t rw_ = mkrsrc(mat ? SLAB_A.w[1] : w0, live ? rows0 * n : 0u); \
        const __amdgpu_buffer_rsrc_t rs_ = mkrsrc(mat ? SLAB_A.ws[1] : ws0, live ? rows0 * ng * 4u : 0u); \
        const uint32_t lrow = lrow0 + tl * TR; \
        const uint32_t col = (c << 10) + (uint32_t)lane * 16u; \
        const uint32_t base = (col < n) ? lrow * n + col : OOB; \
        _Pragma("unroll") \
        for (int r = 0; r < TR; r++) wv[k][r] = bload_w(rw_, base + ((tl * TR + (uint32_t)r < RW) ? (uint32_t)r * n : OOB)); \
        const uint32_t g = c * GC + (uint32_t)lane / LPG; \
        _Pragma("unroll") \
        for (int s = 0; s < NS; s++) { \
            const uint32_t r = ((uint32_t)lane % LPG) + s * LPG; \
            sv[k][s] = bload_f(rs_, (r < TR && tl * TR + r < RW && g < ng) ? ((lrow + r) * ng + g) * 4u : OOB); \
        } \
      } \
    } while (0)
#if SLAB_PART != 2
    constexpr int TR = 4;
    constexpr int LPG = GS / 16, GC = 1024 / GS;
    constexpr int NS = (TR + LPG - 1) / LPG;               // rows a lane owns after the group reduction
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = (int)(SLAB_A.nthr >> 6);
    constexpr bool WF_ = (SLAB_WF) != 0, WFPAIR_ = WF_ && ROLE == R_NORM_SWIGLU;
    static_assert(!WF_ || (GS == 64 && B == 1 && (SLAB_EARLY) == 0 && (ROLE == R_NORM_STORE || ROLE == R_NORM_SWIGLU)), "SLAB_WF: one-chunk rows of the rmsnorm roles");
    constexpr int NCH_ = (SLAB_WFC);                                  // SLAB_WFC: chunks of a row
    constexpr bool WFC_ = NCH_ != 0;
    constexpr uint32_t UP_ = NCH_ <= 2 ? 4u : 8u;                     // ... floats per row of the unit-sum table (a row's sums: one or two 16-byte reads)
    static_assert(!WFC_ || (!WF_ && NCH_ >= 2 && NCH_ <= 4 && GS == 64 && B == 1 && (SLAB_EARLY) == 0 && (ROLE == R_RESID || ROLE == R_RESID_COMBINE)), "SLAB_WFC: whole-chunk rows of the residual roles");
    const uint32_t n = WF_ ? 1024u : WFC_ ? (uint32_t)NCH_ * 1024u : SLAB_A.n, ng = WF_ ? 16u : WFC_ ? (uint32_t)NCH_ * 16u : SLAB_A.ng;
    const uint32_t n16 = (n + 15) & ~15u, ng4 = (ng + 3) & ~3u;
    const uint32_t PITCH = (GC == 16) ? (((ng + 47) / 64) * 64 + 16) : (ng4 + 4);
    const uint32_t RW = SLAB_A.rw, TPW = SLAB_A.tpw, RWP = TPW * TR;         // rows of this workgroup, its four-row tiles, rows of the product table
    const uint32_t epi = role_epi<ROLE>(SLAB_A);
    const bool swiglu = epi == GEMV_EPI_SWIGLU;
    const uint32_t nmat = swiglu ? 2 : 1;
    int8_t *xq = reinterpret_cast<int8_t *>(smem);                 // [B][n16]
    float *xs = reinterpret_cast<float *>(smem + B * n16);         // [B][ng4]
    float *red = xs + B * ng4;                                     // [B][16] (+ combine weights [B][n_head][8])
    constexpr bool CW_ = (SLAB_CW) != 0;
    static_assert(!CW_ || (ROLE == R_RESID_COMBINE && B == 1 && NV >= 1 && !(SLAB_XHAND)), "SLAB_CW: the one-sequence combine role, items in registers");
    float *P = red + B * 16 + (!CW_ && has_flag<ROLE>(SLAB_A, F_COMBINE) ? B * SLAB_A.attn_n_head * 8 : 0);   // [B][nmat][RWP][PITCH] (SLAB_WFC: unit sums [RWP][UP_])

    // every argument the chain below reads late (output slots, strides, positions, the residual addend) is fetched NOW, with
    // the first ones (karg_touch, gemv_common.h)
    karg_touch(SLAB_A.out[0]); karg_touch(SLAB_A.out_bstride[0]); karg_touch(SLAB_A.out_pstride[0]); karg_touch(SLAB_A.rows[0]); karg_touch(SLAB_A.magic_rw); karg_touch(SLAB_A.nb);
    if (!(ROLE == R_RESID || ROLE == R_RESID_COMBINE || ROLE == R_NORM_SWIGLU)) {
        karg_touch(SLAB_A.out[1]); karg_touch(SLAB_A.out[2]); karg_touch(SLAB_A.out_bstride[1]); karg_touch(SLAB_A.out_bstride[2]);
        karg_touch(SLAB_A.out_pstride[1]); karg_touch(SLAB_A.out_pstride[2]); karg_touch(SLAB_A.rows[1]); karg_touch(SLAB_A.rows[2]);
    }
    karg_touch(SLAB_A.pos); karg_touch(SLAB_A.canon);
    if (ROLE == R_GENERIC || ROLE == R_RESID || ROLE == R_RESID_COMBINE) { karg_touch(SLAB_A.resid_add); karg_touch(SLAB_A.resid_add_bstride); }
    NANO_STAMP(SLAB_A.stamps, 0, tid);
    // ---- 1. activation loads (critical path) ------------------------------------------------------------
    Staged<B, NV> sx;
    if constexpr (SLAB_XHAND) stage_issue_nw<ROLE, B, NV>(SLAB_A, sx);          // (the norm weights only: the values come as granules, below)
    else if (!(NANO_STAMPS && (SLAB_A.dbg & 2u))) stage_issue<ROLE, B, NV, (SLAB_CW)>(SLAB_A, sx);

    // ---- 2. all weight / scale loads of this wave; the workgroup's rows lie inside ONE segment ------------
    // (the residual and SwiGLU launches of a decode step have ONE weight segment: their roles skip the selection chains)
    constexpr bool ONESEG = ROLE == R_RESID || ROLE == R_RESID_COMBINE || ROLE == R_NORM_SWIGLU;
    const int sel = (ONESEG || swiglu) ? 0 : (int)(SLAB_BID >= SLAB_A.wg_c0) + (int)(SLAB_BID >= SLAB_A.wg_c1);
    const int8_t *w0 = sel == 0 ? SLAB_A.w[0] : sel == 1 ? SLAB_A.w[1] : SLAB_A.w[2];
    const float *ws0 = sel == 0 ? SLAB_A.ws[0] : sel == 1 ? SLAB_A.ws[1] : SLAB_A.ws[2];
    float *out0 = sel == 0 ? SLAB_A.out[0] : sel == 1 ? SLAB_A.out[1] : SLAB_A.out[2];
    const uint32_t rows0 = sel == 0 ? SLAB_A.rows[0] : sel == 1 ? SLAB_A.rows[1] : SLAB_A.rows[2];
    const uint32_t obs = sel == 0 ? SLAB_A.out_bstride[0] : sel == 1 ? SLAB_A.out_bstride[1] : SLAB_A.out_bstride[2];
    const uint32_t ops = sel == 0 ? SLAB_A.out_pstride[0] : sel == 1 ? SLAB_A.out_pstride[1] : SLAB_A.out_pstride[2];
    const uint32_t lrow0 = (SLAB_BID - (sel == 0 ? 0u : sel == 1 ? SLAB_A.wg_c0 : SLAB_A.wg_c1)) * RW;

    int4 wv[UPW][TR];
    float sv[UPW][NS];
    // Round 6, the matrices of >= 8 M weights: a CU's share of those (65-207 KB) does not fit the memory pipeline's queue, a wave's load
    // instructions BLOCK at issue until earlier ones have returned, and every wave of the workgroup reached the activation only after the
    // whole burst (stamps, W2 of Qwen3-4B: 4.0 us in issue, THEN 1.9 us of quantization, with nothing in flight).  Such launches ask for
    // the first `early` units of every wave here and for the rest after the activation is in LDS: the first units stream while it is
    // normalised and quantized.  (early = 0: everything here -- the small matrices, whose loads all leave at once.)
    constexpr uint32_t early_ = (uint32_t)(SLAB_EARLY);      // (compile time: a run-time choice in these kernels cost the small launches 1.3 %)
    static_assert(SLAB_PART == 0 || early_ == 0u, "SLAB_EARLY: the whole body only");
    // (a macro, not a lambda: as a lambda the fused kernels' schedules changed and the one-sequence step lost 0.8 %.  Unit u = wave + k NW ->
    //  (tile, chunk); rows of the tile beyond the workgroup's RW belong to the next workgroup (RW % 4 != 0): a wave-uniform select)
#pragma unroll
    for (int k = 0; k < UPW; k++) { if (early_ == 0u || (uint32_t)k < early_) SLAB_ISSUE_UNIT(k); }
    if (!SLAB_XHAND && NANO_STAMPS && (SLAB_A.dbg & 2u)) stage_issue<ROLE, B, NV, (SLAB_CW)>(SLAB_A, sx);          // (experiment: the activation behind the weights)
    // ---- 3. the fold thread's output slot (residual: old value) -----------------------------------------------
    const int fb = (int)(((uint32_t)tid * SLAB_A.magic_rw) >> 16);          // tid / RW: fold thread -> (sequence, local row)
    const int frl = tid - fb * (int)RW;
    const bool fold_live = tid < (int)(RW * B) && fb < (int)SLAB_A.nb && lrow0 + frl < rows0;
    // the position of a pos-indexed output (v-cache row) is fetched now and used only by the final store: no wait
    // here (a wait on it would also wait for every weight load issued above -- vmcnt counts in order)
    uint32_t opos = 0;
    if constexpr (WF_) {        // (the lanes that will hold the row results ask; a buffer load: in order behind the weights, no traffic elsewhere)
        if constexpr (ROLE == R_NORM_STORE) opos = __float_as_uint(bload_f(mkrsrc(SLAB_A.pos, ops ? 4u : 0u), ((uint32_t)lane & ~3u) == (uint32_t)WF_LANE0 ? 0u : OOB));
    } else
    if (ops && fold_live) opos = SLAB_A.pos[fb];
    float oldv = 0.0f;
    if (epi == GEMV_EPI_RESID && fold_live) oldv = out0[(size_t)fb * obs + lrow0 + frl];      // residual stream: never pos-indexed
    float addv = 0.0f;                                              // LoRA o-branch: x += (W.act + addv), reference order
    const bool has_add = epi == GEMV_EPI_RESID && SLAB_A.resid_add != nullptr;
    if (has_add && fold_live) addv = SLAB_A.resid_add[(size_t)fb * SLAB_A.resid_add_bstride + lrow0 + frl];

    NANO_STAMP(SLAB_A.stamps, 1, oldv);                                  // every load issued
#endif   // SLAB_PART != 2
#if SLAB_PART != 1
    // ---- 4. rmsnorm + quantization from registers (weights in flight) ----------------------------------------
    if constexpr (SLAB_XHAND) {
        // The activation as 8-byte {tag, value} granules from the workgroups that produce it in this same launch (an all-gather by
        // polling: every thread waits for the granules of its own float4 items).  Relaxed agent-scope loads, the tag and the value
        // arrive together (guide, Guideline 16 R2).  Bounded; giving up is reported through the sticky error word.
        static_assert(!SLAB_XHAND || B == 1, "granule activations: one sequence");
        const unsigned long long *hb_ = SLAB_XHANDV.buf;
        const uint32_t ctag_ = SLAB_CTAG;
        bool got_ = false;                  // (one sweep at a time: two in flight measured SLOWER here -- the polls compete with the producers)
        for (uint32_t w_ = 0; w_ < SLAB_XHAND_WAIT; w_++) __builtin_amdgcn_s_sleep(16);      // (workgroups that produce nothing: the first granules are ~3 us away)
        for (uint32_t spin_ = 0; spin_ < (1u << 14) && !got_; spin_++) {
            if (spin_) __builtin_amdgcn_s_sleep(SLAB_XHAND_NAP);
            // somebody in this step already gave up (the abort word next to the tick): the call is lost, do not sit out the bound again
            if ((spin_ & 63u) == 63u && hand_aborted(SLAB_XHANDV)) break;
            got_ = true;
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const uint32_t i = ((uint32_t)tid + (uint32_t)j * SLAB_A.nthr) * 4u;
                if (i < n) {
                    const unsigned long long g0_ = __hip_atomic_load(hb_ + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long g1_ = __hip_atomic_load(hb_ + i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long g2_ = __hip_atomic_load(hb_ + i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long g3_ = __hip_atomic_load(hb_ + i + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    got_ = got_ && (uint32_t)(g0_ >> 32) == ctag_ && (uint32_t)(g1_ >> 32) == ctag_ && (uint32_t)(g2_ >> 32) == ctag_ && (uint32_t)(g3_ >> 32) == ctag_;
                    sx.x[0][j] = make_float4(__uint_as_float((uint32_t)g0_), __uint_as_float((uint32_t)g1_), __uint_as_float((uint32_t)g2_), __uint_as_float((uint32_t)g3_));
                } else sx.x[0][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (!got_) hand_give_up(SLAB_XHANDV, SLAB_A.err);
    }
    stage_finish<ROLE, GS, B, NV, (SLAB_CW)>(SLAB_A, sx, xq, xs, red, n16, ng4);
    if constexpr (early_ != 0u) {
#pragma unroll
        for (int k = 1; k < UPW; k++) { if ((uint32_t)k >= early_) SLAB_ISSUE_UNIT(k); }
    }
    NANO_STAMP(SLAB_A.stamps, 3, xs[0]);                                 // activation normalised + quantized in LDS (stamp 2: inside, the activation arrived)

    if constexpr (WF_) {
    // ---- 5 + 6, rows of one chunk (SLAB_WF): integer dots, the product stays in its lane, the wave folds and stores its own rows --------
    float pw_[UPW];
    const int4 xv_ = *reinterpret_cast<const int4 *>(xq + lane * 16);
    const float xsc_ = xs[lane >> 2];
    asm volatile("" :: "v"(xsc_));                                       // (read next to the activation bytes, not behind the dots: one LDS round trip)
#pragma unroll
    for (int k = 0; k < UPW; k++) {
        int iv[TR];
#pragma unroll
        for (int r = 0; r < TR; r++) {
            int d = __builtin_amdgcn_sdot4(wv[k][r].x, xv_.x, 0, false);
            d = __builtin_amdgcn_sdot4(wv[k][r].y, xv_.y, d, false);
            d = __builtin_amdgcn_sdot4(wv[k][r].z, xv_.z, d, false);
            d = __builtin_amdgcn_sdot4(wv[k][r].w, xv_.w, d, false);
            iv[r] = dpp_group_sum<LPG>(d);
        }
        int v = iv[0];
#pragma unroll
        for (int q = 1; q < TR; q++) v = (q == (lane & 3)) ? iv[q] : v;
        pw_[k] = ((float)v * sv[k][0]) * xsc_;                                                  // infer.c:672 (units beyond the last, rows beyond RW: weights and scales read as 0)
    }
    NANO_STAMP(SLAB_A.stamps, 4, pw_[UPW - 1]);                          // this wave's weights arrived, its dots are done
    NANO_STAMP(SLAB_A.stamps, 5, pw_[UPW - 1]);                          // (no table, no barrier: the same moment)
#pragma unroll
    for (int k = 0; k < UPW; k++) {
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW;
        if (u < SLAB_A.units) {
            const float v0 = wave_fold_canon16(pw_[k]);                                       // lanes WF_LANE0 + r: row r of the unit
            const float v1 = WFPAIR_ ? DPP_F(v0, 0x102) : 0.0f;                               // (row_shl:2: W3's row next to W1's)
            const uint32_t rl_ = WFPAIR_ ? u * 2u + ((uint32_t)lane & 1u) : u * (uint32_t)TR + ((uint32_t)lane & 3u);
            const bool mine_ = WFPAIR_ ? ((uint32_t)lane & ~1u) == (uint32_t)WF_LANE0 : ((uint32_t)lane & ~3u) == (uint32_t)WF_LANE0;
            if (mine_ && rl_ < RW && lrow0 + rl_ < rows0) {
                float *dst = out0 + (size_t)opos * ops + lrow0 + rl_;
                const float val = finish_epi(epi, v0, v1, 0.0f);
                if constexpr (SLAB_HAND == 1)                             // (the granule first: a waiting workgroup sits behind it)
                    __hip_atomic_store(SLAB_HANDV.buf + (sel == 0 ? SLAB_HANDV.base[0] : sel == 1 ? SLAB_HANDV.base[1] : SLAB_HANDV.base[2]) + lrow0 + rl_,
                                       ((unsigned long long)(SLAB_PTAG) << 32) | (unsigned long long)__float_as_uint(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (NANO_STAMPS && (SLAB_A.dbg & 4u)) *dst = val; else __hip_atomic_store(dst, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // write-through, as below
            }
        }
    }
    } else {
    // ---- 5. integer dots, group products into the LDS table ----------------------------------------------------
#pragma unroll
    for (int k = 0; k < UPW; k++) {
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW;
        if (u < SLAB_A.units) {
            const uint32_t t = (u * SLAB_A.magic_nchunk) >> 16;
            const uint32_t c = u - t * SLAB_A.nchunk;
            const uint32_t mat = t >= TPW ? 1u : 0u, tl = t - mat * TPW;
            const uint32_t col = (c << 10) + (uint32_t)lane * 16u;
            const uint32_t g = c * GC + (uint32_t)lane / LPG;
            if constexpr (WFC_) {
                // the product stays in the lane that formed it (lane 4 g + r: row r, group g of the chunk); the wave folds the chunk to its two
                // unit sums and lanes WF_LANE0 + r leave them in the row's slots 2 c, 2 c + 1 (rows beyond RW: weights and scales read as 0)
                const int4 xv = *reinterpret_cast<const int4 *>(xq + col);
                const float xsc = xs[g];
                int iv[TR];
#pragma unroll
                for (int r = 0; r < TR; r++) {
                    int d = __builtin_amdgcn_sdot4(wv[k][r].x, xv.x, 0, false);
                    d = __builtin_amdgcn_sdot4(wv[k][r].y, xv.y, d, false);
                    d = __builtin_amdgcn_sdot4(wv[k][r].z, xv.z, d, false);
                    d = __builtin_amdgcn_sdot4(wv[k][r].w, xv.w, d, false);
                    iv[r] = dpp_group_sum<LPG>(d);
                }
                int v = iv[0];
#pragma unroll
                for (int q = 1; q < TR; q++) v = (q == (lane & 3)) ? iv[q] : v;
                float s0_, s1_;
                wave_fold_canon16_units(((float)v * sv[k][0]) * xsc, s0_, s1_);                                    // infer.c:672
                if (((uint32_t)lane & ~3u) == (uint32_t)WF_LANE0)
                    *reinterpret_cast<float2 *>(P + (tl * TR + ((uint32_t)lane & 3u)) * UP_ + 2u * c) = make_float2(s0_, s1_);
            } else {
#pragma unroll
            for (int b = 0; b < B; b++) {
                if (b < (int)SLAB_A.nb) {
                    const int4 xv = (col < n) ? *reinterpret_cast<const int4 *>(xq + b * n16 + col) : make_int4(0, 0, 0, 0);
                    int iv[TR];
#pragma unroll
                    for (int r = 0; r < TR; r++) {
                        int d = __builtin_amdgcn_sdot4(wv[k][r].x, xv.x, 0, false);
                        d = __builtin_amdgcn_sdot4(wv[k][r].y, xv.y, d, false);
                        d = __builtin_amdgcn_sdot4(wv[k][r].z, xv.z, d, false);
                        d = __builtin_amdgcn_sdot4(wv[k][r].w, xv.w, d, false);
                        iv[r] = dpp_group_sum<LPG>(d);
                    }
                    const float xsc = (g < ng) ? xs[b * ng4 + g] : 0.0f;
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        const uint32_t r = ((uint32_t)lane % LPG) + s * LPG;
                        int v = iv[0];
#pragma unroll
                        for (int q = 1; q < TR; q++) v = (q == (int)r) ? iv[q] : v;
                        if (r < TR && g < ng)                                                   // infer.c:672
                            P[(((size_t)b * nmat + mat) * RWP + tl * TR + r) * PITCH + g] = ((float)v * sv[k][s]) * xsc;
                    }
                }
            }
            }   // !SLAB_WFC
        }
    }
    NANO_STAMP(SLAB_A.stamps, 4, wv[UPW - 1][TR - 1].w);                 // this wave's weights arrived, its products are in the table
    __syncthreads();
    NANO_STAMP(SLAB_A.stamps, 5, P[0]);                                  // every wave's products are in the table

    // ---- 6. ordered fold (infer.c:668-674) + epilogue -------------------------------------------------------------
    // The wide matrices (SLAB_EARLY instantiations, canonical launches of whole units): the unit sums first, ONE THREAD PER (row, unit) -- each
    // adds its 8 group products in order and leaves S_u in the unit's first slot of the table -- then the thread of a row adds the units in
    // ascending order.  A row of Qwen3-4B's W2 is 152 groups: one thread walking it paid ten dependent LDS round trips (~0.8 us of a ~9 us launch).
    constexpr bool PFOLD = early_ != 0u && GS == 64;
    bool pfold_ = false;
    if constexpr (PFOLD) {
        pfold_ = (ROLE != R_GENERIC || SLAB_A.canon) && (ng & 7u) == 0u;
        if (pfold_) {
            const uint32_t nu_ = ng >> 3, rows_ = RW * (uint32_t)B * nmat, items_ = rows_ * nu_;
            for (uint32_t it = (uint32_t)tid; it < items_; it += SLAB_A.nthr) {
                const uint32_t rr_ = it / nu_, u_ = it - rr_ * nu_;                 // rr_ = (sequence * nmat + matrix) * RW + row
                const uint32_t bm_ = rr_ / RW, rl_ = rr_ - bm_ * RW;
                float *pu_ = P + ((size_t)bm_ * RWP + rl_) * PITCH + 8u * u_;
                const float4 t0_ = *reinterpret_cast<const float4 *>(pu_), t1_ = *reinterpret_cast<const float4 *>(pu_ + 4);
                pu_[0] = unit_sum(t0_, t1_);
            }
            __syncthreads();
        }
    }
    if (tid < (int)(RW * B)) {
        // all LDS reads of a 16-group batch are issued before the dependent add chain; groups beyond ng add
        // +0.0f (exact: the running value is never -0.0f)
        float v0 = 0.0f, v1 = 0.0f;
        const float *p0 = P + (((size_t)fb * nmat) * RWP + frl) * PITCH;
        const float *p1 = p0 + (size_t)RWP * PITCH;
        // The role kernels of group size 64 are launched for CANONICAL launches only (launch_slab_b): the canonical fold alone, no run-time
        // choice and no ordered chain in their code (round 4 left both folds behind a run-time flag in every kernel: the one-sequence step
        // of Qwen3-0.6B went 1880 -> 1826 tok/s with it, bisected in round 5: profiles/r05_headline_bisect.txt).
        constexpr bool ROLE_CANON = ROLE != R_GENERIC && GS == 64;
        if constexpr (WFC_) {                                        // the row's unit sums, ascending: ((S_0 + S_1) + S_2) + ...
            const float4 a_ = *reinterpret_cast<const float4 *>(P + (uint32_t)frl * UP_);
            float4 b_ = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (NCH_ > 2) b_ = *reinterpret_cast<const float4 *>(P + (uint32_t)frl * UP_ + 4u);
            v0 = fadd(fadd(fadd(a_.x, a_.y), a_.z), a_.w);
            if constexpr (NCH_ > 2) v0 = fadd(fadd(v0, b_.x), b_.y);
            if constexpr (NCH_ > 3) v0 = fadd(fadd(v0, b_.z), b_.w);
        } else
        if (PFOLD && pfold_) {                                       // units ascending; the first unit is the row's starting value
            const uint32_t nu_ = ng >> 3;
            v0 = p0[0];
            for (uint32_t u_ = 1; u_ < nu_; u_++) v0 = fadd(v0, p0[8u * u_]);
            if (swiglu) { v1 = p1[0]; for (uint32_t u_ = 1; u_ < nu_; u_++) v1 = fadd(v1, p1[8u * u_]); }
        } else
        if constexpr (ROLE_CANON) {
            if constexpr (ROLE == R_NORM_SWIGLU) fold_row2_canon_ng(p0, p1, ng, v0, v1); else v0 = fold_row_canon_ng(p0, ng);
        } else
        if (GS == 64 && SLAB_A.canon) {                              // the fast path's canonical fold (strict mode: the reference's order below)
            v0 = fold_row_canon_ng(p0, ng);
            if (swiglu) v1 = fold_row_canon_ng(p1, ng);
        } else
        if (!swiglu && ng == 48u) v0 = fold_row<12>(p0);        // the row lengths of Qwen3-0.6B at group size 64 (3072 / 2048 / 1024): every
        else if (!swiglu && ng == 32u) v0 = fold_row<8>(p0);    // LDS read of the row goes out before the dependent add chain starts (round 3:
        else if (ng == 16u) {                                   // the batch-by-batch loop below exposes one LDS round trip per 16 groups)
            if (swiglu) fold_row2<4>(p0, p1, v0, v1); else v0 = fold_row<4>(p0);
        } else if ((ng & 15u) == 0) {       // whole 16-group batches (every BASELINE shape): no per-element selects
            for (uint32_t g0 = 0; g0 < ng; g0 += 16) {
                float4 t[4], u[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { t[q] = *reinterpret_cast<const float4 *>(p0 + g0 + 4 * q); if (swiglu) u[q] = *reinterpret_cast<const float4 *>(p1 + g0 + 4 * q); }
#pragma unroll
                for (int q = 0; q < 4; q++) { v0 += t[q].x; v0 += t[q].y; v0 += t[q].z; v0 += t[q].w; }
                if (swiglu) {
#pragma unroll
                    for (int q = 0; q < 4; q++) { v1 += u[q].x; v1 += u[q].y; v1 += u[q].z; v1 += u[q].w; }
                }
            }
        } else {
        for (uint32_t g0 = 0; g0 < ng; g0 += 16) {
                float4 t[4], u[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    t[q] = (g0 + 4 * q < ng4) ? *reinterpret_cast<const float4 *>(p0 + g0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
                    if (swiglu) u[q] = (g0 + 4 * q < ng4) ? *reinterpret_cast<const float4 *>(p1 + g0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t g = g0 + 4 * q;
                    v0 += (g < ng) ? t[q].x : 0.0f; v0 += (g + 1 < ng) ? t[q].y : 0.0f; v0 += (g + 2 < ng) ? t[q].z : 0.0f; v0 += (g + 3 < ng) ? t[q].w : 0.0f;
                }
                if (swiglu) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t g = g0 + 4 * q;
                        v1 += (g < ng) ? u[q].x : 0.0f; v1 += (g + 1 < ng) ? u[q].y : 0.0f; v1 += (g + 2 < ng) ? u[q].z : 0.0f; v1 += (g + 3 < ng) ? u[q].w : 0.0f;
                    }
                }
            }
        }
        if (fold_live) {
            float *dst = out0 + (size_t)fb * obs + (size_t)opos * ops + lrow0 + frl;
            const float val = finish_epi(epi, has_add ? v0 + addv : v0, v1, oldv);
            // WRITE-THROUGH (sc1) store: the result leaves the XCD's L2 now instead of in the write-back at the end of the kernel, which
            // the next kernel's start waits for (round 3, measured: 1807 -> 1836 tok/s at positions 20..39, 1681 -> 1718 over 31..510;
            // measurement builds: NANO_DBG bit 4 restores the plain store for A/B runs)
            if constexpr (SLAB_HAND == 1)                             // (the granule first: a waiting workgroup sits behind it)
                __hip_atomic_store(SLAB_HANDV.buf + (sel == 0 ? SLAB_HANDV.base[0] : sel == 1 ? SLAB_HANDV.base[1] : SLAB_HANDV.base[2]) + lrow0 + (uint32_t)frl,
                                   ((unsigned long long)(SLAB_PTAG) << 32) | (unsigned long long)__float_as_uint(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (NANO_STAMPS && (SLAB_A.dbg & 4u)) *dst = val; else __hip_atomic_store(dst, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    }   // !SLAB_WF
    NANO_STAMP_END(SLAB_A.stamps, 6);                                    // folded and stored: the workgroup's last wave ends
#endif   // SLAB_PART != 1
#undef SLAB_ISSUE_UNIT
#ifdef SLAB_WF_DEFAULTED
#undef SLAB_WF
#undef SLAB_WF_DEFAULTED
#endif
#ifdef SLAB_WFC_DEFAULTED
#undef SLAB_WFC
#undef SLAB_WFC_DEFAULTED
#endif
#ifdef SLAB_EARLY_DEFAULTED
#undef SLAB_EARLY
#undef SLAB_EARLY_DEFAULTED
#endif
#ifdef SLAB_CW_DEFAULTED
#undef SLAB_CW
#undef SLAB_CW_DEFAULTED
#endif
#ifdef SLAB_XHAND_WAIT_DEFAULTED
#undef SLAB_XHAND_WAIT
#undef SLAB_XHAND_NAP
#undef SLAB_XHAND_WAIT_DEFAULTED
#endif
