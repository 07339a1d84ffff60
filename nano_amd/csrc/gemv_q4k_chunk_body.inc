// gemv_q4k_chunk_body.inc -- the statements of the Q4K chunk GEMV kernel (gemv_q4k_chunk.hip), included TEXTUALLY into each kernel that runs
// them: the plain gemv_q4k_chunk_kernel and (round 6) the fused q | k | v + attention launch -- the same arrangement, for the same reason, as
// gemv_q80_slab_body.inc (a by-value kernel-argument block routed through a reference ended up in scratch).  The includer defines
//   CHUNK_A      the GemvDev (a by-value kernel parameter, or a member of one)
//   CHUNK_BID    the workgroup's index among this body's workgroups
//   CHUNK_HAND   0 | 1: the fold threads also store every result as an 8-byte {tag, value} granule (CHUNK_HANDV: the SlabHand, CHUNK_PTAG: the
//                producers' tag of this step and layer -- device_common.h)
// and has ROLE, NV, D, LOOP, NB and smem in scope.
    const uint32_t tid = threadIdx.x, nthr = CHUNK_A.nthr, lane = tid & 63u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), NW = nthr >> 6;
    const uint32_t n = CHUNK_A.n, bpl = n >> 8, GT = bpl * 8u, BP = bpl | 1u;    // BP: pitch of the block-sum table (odd: rows on different banks)
    const uint32_t RW = CHUNK_A.rw;
    const uint32_t epi = role_epi<ROLE>(CHUNK_A);
    const bool swiglu = epi == GEMV_EPI_SWIGLU;
    const uint32_t nmat = swiglu ? 2u : 1u;
    // LDS: xg[NB][GT] | red[16 (+ combine weights)] | scr[NW][SL][64] (SL = D lines per wave; looping launches: 1; NB > 1: one per sequence)
    //      | am[2 NW] | Dt[nmat][NB][RW][BP]
    XGroup *xg = reinterpret_cast<XGroup *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)NB * GT * sizeof(XGroup));
    float *scr = red + 16 + (has_flag<ROLE>(CHUNK_A, F_COMBINE) ? CHUNK_A.attn_n_head * 8u : 0u);
    constexpr uint32_t SL = NB > 1 ? (uint32_t)NB : LOOP ? 1u : (uint32_t)D;
    float *am = scr + NW * SL * 64u;
    float *Dt = am + 2u * NW;

    // late-read arguments are fetched with the first ones (karg_touch, gemv_common.h)
    karg_touch(CHUNK_A.out[0]); karg_touch(CHUNK_A.out_pstride[0]); karg_touch(CHUNK_A.magic_nchunk); karg_touch(CHUNK_A.tile_max); karg_touch(CHUNK_A.ntiles); karg_touch(CHUNK_A.units);
    if (!swiglu) { karg_touch(CHUNK_A.out[1]); karg_touch(CHUNK_A.out[2]); karg_touch(CHUNK_A.out_pstride[1]); karg_touch(CHUNK_A.out_pstride[2]); }
    karg_touch(CHUNK_A.pos);
    if (ROLE == R_GENERIC || ROLE == R_RESID || ROLE == R_RESID_COMBINE) { karg_touch(CHUNK_A.resid_add); karg_touch(CHUNK_A.resid_add_bstride); }
    NANO_STAMP(CHUNK_A.stamps, 0, tid);
    Staged<1, NV> sx;
    if constexpr (NB == 1) stage_issue<ROLE, 1, NV>(CHUNK_A, sx);

    // this workgroup's rows: inside one segment (the last workgroup of a segment may hold fewer than RW)
    const uint32_t bid = CHUNK_BID;
    const int sel = swiglu ? 0 : (int)(bid >= CHUNK_A.wg_c0) + (int)(bid >= CHUNK_A.wg_c1);
    const uint8_t *w0 = reinterpret_cast<const uint8_t *>(sel == 0 ? CHUNK_A.w[0] : sel == 1 ? CHUNK_A.w[1] : CHUNK_A.w[2]);
    float *out0 = sel == 0 ? CHUNK_A.out[0] : sel == 1 ? CHUNK_A.out[1] : CHUNK_A.out[2];
    const uint32_t rows0 = sel == 0 ? CHUNK_A.rows[0] : sel == 1 ? CHUNK_A.rows[1] : CHUNK_A.rows[2];
    const uint32_t ops = sel == 0 ? CHUNK_A.out_pstride[0] : sel == 1 ? CHUNK_A.out_pstride[1] : CHUNK_A.out_pstride[2];
    const uint32_t lrow0 = (bid - (sel == 0 ? 0u : sel == 1 ? CHUNK_A.wg_c0 : CHUNK_A.wg_c1)) * RW;
    const uint32_t rwl = rows0 - lrow0 < RW ? rows0 - lrow0 : RW;
    const uint32_t nblk = rwl * bpl;                                   // blocks of this workgroup, per matrix
    const uint32_t T = ((nblk + 5u) * 43691u) >> 18;                   // wave-loads per matrix: ceil(nblk / 6) (nblk < 2^16)
    const uint32_t TT = nmat * T;
    const size_t run0 = (size_t)lrow0 * bpl * 160u;
    const __amdgpu_buffer_rsrc_t rw0 = mkrsrc(w0 + run0, nblk * 160u);
    const __amdgpu_buffer_rsrc_t rw1 = mkrsrc(swiglu ? reinterpret_cast<const uint8_t *>(CHUNK_A.w[1]) + run0 : nullptr, swiglu ? nblk * 160u : 0u);

    const uint32_t cl = (lane * 26u) >> 8, c = lane - cl * 10u;        // lane / 10, lane % 10
    const bool live = lane < 60u;
    const uint32_t loff = live ? lane * 16u : OOB;

    uint4 ring[D];
    auto issue = [&](const uint32_t t) __attribute__((always_inline)) -> uint4 {
        const bool m1 = swiglu && t >= T;                               // wave-uniform
        const uint32_t tl = t - (m1 ? T : 0u);
        const uint32_t off = (t < TT && live) ? tl * 960u + loff : OOB;
        return m1 ? bload_u4(rw1, off, true) : bload_u4(rw0, off, true);
    };
#pragma unroll
    for (int k = 0; k < D; k++) ring[k] = issue(wid + (uint32_t)k * NW);

    // the fold threads (one per row of the workgroup): the position of a pos-indexed output (v-cache row), the old residual value
    // and the LoRA addend are fetched now and used only by the final store
    const bool fold_live = NB == 1 && tid < rwl;                                   // (several sequences: the fold loop below fetches its own)
    uint32_t opos = 0;
    if (ops && fold_live) opos = CHUNK_A.pos[0];
    float oldv = 0.0f;
    if (epi == GEMV_EPI_RESID && fold_live) oldv = out0[lrow0 + tid];              // residual stream: never pos-indexed
    float addv = 0.0f;                                                             // LoRA o-branch: x += (W.act + addv), reference order
    const bool has_add = epi == GEMV_EPI_RESID && CHUNK_A.resid_add != nullptr;
    if (has_add && fold_live) addv = CHUNK_A.resid_add[lrow0 + tid];

    NANO_STAMP(CHUNK_A.stamps, 1, tid);                                   // every load of the first ring issued

    // ---- a wave-load in two halves: what needs only the weights (pre), what needs the staged activation (post) ----------------------
    float *scw = scr + wid * SL * 64u;                              // this wave's lines: group values of the six blocks of a wave-load
    const int ha0 = (int)(cl * 40u), ha1 = ha0 + 4;                 // byte addresses (ds_bpermute) of this lane's two header lanes
    const uint32_t g = (c - 2u) & 7u;                               // group of the block (lanes with c >= 2; the header lanes compute along, unused)
    struct Pre { float sp, bp, su; };
    auto pre = [&](const uint4 v) __attribute__((always_inline)) -> Pre {
        // the block's header words: s_scale (chunk 0, word 3), s_bias and the 12 packed 6-bit bytes (chunk 1)
        const float s_scale = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(ha0, (int)v.w));
        const float s_bias = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(ha1, (int)v.x));
        const uint32_t sb0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ha1, (int)v.y);
        const uint32_t sb1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ha1, (int)v.z);
        const uint32_t sb2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ha1, (int)v.w);
        uint32_t s6, b6;
        q4k_unpack6(sb0, sb1, sb2, (int)g, s6, b6);
        const uint32_t wn[4] = { v.x, v.y, v.z, v.w };
        uint32_t sump = 0;                                              // v_dot8_u32_u4: the weight nibbles against eight ones
#pragma unroll
        for (int m = 0; m < 4; m++) sump = __builtin_amdgcn_udot8(wn[m], 0x11111111u, sump, false);
        return Pre{(float)s6 * s_scale, (float)b6 * s_bias, (float)(int)sump};
    };
    // post, step A: the group values of wave-load t into line `ln` of this wave's scratch; step B: the block's first lane adds the
    // eight in order and files the block sum.  Straight-line launches run A for all their wave-loads, then B for all (the LDS round
    // trips of D independent wave-loads overlap instead of queueing up behind one another).
    auto post_a = [&](const uint4 v, const Pre q, const uint32_t t, float *ln, const uint32_t sq_ = 0u) __attribute__((always_inline)) {
        const bool m1 = swiglu && t >= T;
        const uint32_t tl = t - (m1 ? T : 0u);
        const uint32_t b = tl * 6u + cl;                                // block of the workgroup's run
        const bool bv = t < TT && live && b < nblk;
        const uint32_t rl = bpl == 1u ? b : __umulhi(b, CHUNK_A.magic_nchunk), blk = b - rl * bpl;   // b / bpl, b % bpl (magic_nchunk = ceil(2^32 / bpl) here; 2^32 does not fit)
        if (bv && c >= 2u) {
            const uint32_t wn[4] = { v.x, v.y, v.z, v.w };
            const XGroup &xq = xg[sq_ * GT + blk * 8u + g];
            uint32_t spq = 0;                                           // ... against the activation nibbles
#pragma unroll
            for (int m = 0; m < 4; m++) spq = __builtin_amdgcn_udot8(wn[m], xq.pk[m], spq, false);
            const float sp = q.sp, bp = q.bp, sq = xq.sq, bq = xq.bq;
            // reference tensor.c:425-428, same association (whole blocks: every group has 32 values)
            ln[cl * 8u + g] = sp * sq * (float)(int)spq - sp * bq * q.su - sq * bp * (float)xq.sumq + 32 * bp * bq;
        }
    };
    auto post_b = [&](const uint32_t t, const float *ln, const uint32_t sq_ = 0u) __attribute__((always_inline)) {
        const bool m1 = swiglu && t >= T;
        const uint32_t tl = t - (m1 ? T : 0u);
        const uint32_t b = tl * 6u + cl;
        const bool bv = t < TT && live && b < nblk;
        const uint32_t rl = bpl == 1u ? b : __umulhi(b, CHUNK_A.magic_nchunk), blk = b - rl * bpl;
        if (bv && c == 0u) {
            const float4 v0 = *reinterpret_cast<const float4 *>(ln + cl * 8u), v1 = *reinterpret_cast<const float4 *>(ln + cl * 8u + 4u);
            float d = 0.0f;                                             // the 8 groups of a block in order (tensor.c:359-434)
            d += v0.x; d += v0.y; d += v0.z; d += v0.w; d += v1.x; d += v1.y; d += v1.z; d += v1.w;
            Dt[(((m1 ? (uint32_t)NB : 0u) + sq_) * RW + rl) * BP + blk] = d;
        }
    };

    // The activation: normalised from registers, block-quantized wave-locally into LDS.  A wave that is done with its blocks (or has
    // none) works through the weight-only half of its wave-loads while the others still quantize; the barrier after that publishes xg.
    Pre pq[D];
    if constexpr (NB > 1) {
        // the staged groups of every sequence, as q4k_quant_rows_kernel left them: [sequence][GT] x 32 bytes, copied as they are
        const uint4 *src = reinterpret_cast<const uint4 *>(CHUNK_A.xq_in);
        uint4 *dst = reinterpret_cast<uint4 *>(xg);
        const uint32_t cnt = CHUNK_A.nb * GT * 2u;
        for (uint32_t i = tid; i < cnt; i += nthr) dst[i] = src[i];
    } else
    if (has_flag<ROLE>(CHUNK_A, F_PRE)) unpack_q4k_wg(CHUNK_A, xg);
    else {
        stage_xn<ROLE, 1, NV>(CHUNK_A, sx, nullptr, red, (n + 3u) & ~3u, true);
        NANO_STAMP(CHUNK_A.stamps, 2, red[0]);                            // the activation arrived and is normalised
        quantize_q4k_regs<1, NV, false>(CHUNK_A, sx, xg);
    }
    if constexpr (!LOOP) {
#pragma unroll
        for (int k = 0; k < D; k++) pq[k] = pre(ring[k]);
    }
    __syncthreads();
    NANO_STAMP(CHUNK_A.stamps, 3, xg[0].sq);                              // block-quantized activation staged in LDS

    if constexpr (NB > 1 && !LOOP) {
        // several sequences: a wave-load at a time, its activation half once per sequence (one scratch line each)
#pragma unroll
        for (int k = 0; k < D; k++) {
            const uint32_t t = wid + (uint32_t)k * NW;
#pragma unroll
            for (int b = 0; b < NB; b++) if ((uint32_t)b < CHUNK_A.nb) post_a(ring[k], pq[k], t, scw + b * 64, (uint32_t)b);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int b = 0; b < NB; b++) if ((uint32_t)b < CHUNK_A.nb) post_b(t, scw + b * 64, (uint32_t)b);
            __builtin_amdgcn_wave_barrier();
        }
    } else if constexpr (NB > 1) {
        for (uint32_t r = 0; r < CHUNK_A.units; r++) {
#pragma unroll
            for (int k = 0; k < D; k++) {
                const uint32_t t = wid + (r * (uint32_t)D + (uint32_t)k) * NW;
                const Pre q = pre(ring[k]);
#pragma unroll
                for (int b = 0; b < NB; b++) if ((uint32_t)b < CHUNK_A.nb) post_a(ring[k], q, t, scw + b * 64, (uint32_t)b);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int b = 0; b < NB; b++) if ((uint32_t)b < CHUNK_A.nb) post_b(t, scw + b * 64, (uint32_t)b);
                __builtin_amdgcn_wave_barrier();
                ring[k] = issue(t + (uint32_t)D * NW);
            }
        }
    } else
    if constexpr (!LOOP) {
#pragma unroll
        for (int k = 0; k < D; k++) post_a(ring[k], pq[k], wid + (uint32_t)k * NW, scw + k * 64);
        __builtin_amdgcn_wave_barrier();                                // (the LDS queue of a wave is in order: the reads below see the writes above)
#pragma unroll
        for (int k = 0; k < D; k++) post_b(wid + (uint32_t)k * NW, scw + k * 64);
    } else {
        // persistent: `CHUNK_A.units` rounds of D wave-loads; a consumed slot is asked for again at once (loads past the end: out of range, no traffic)
        for (uint32_t r = 0; r < CHUNK_A.units; r++) {
#pragma unroll
            for (int k = 0; k < D; k++) {
                const uint32_t t = wid + (r * (uint32_t)D + (uint32_t)k) * NW;
                post_a(ring[k], pre(ring[k]), t, scw);
                __builtin_amdgcn_wave_barrier();
                post_b(t, scw);
                __builtin_amdgcn_wave_barrier();
                ring[k] = issue(t + (uint32_t)D * NW);
            }
        }
    }
    NANO_STAMP(CHUNK_A.stamps, 4, (float)ring[D - 1].x);                 // this wave's weights arrived, its block sums are in the table
    __syncthreads();
    NANO_STAMP(CHUNK_A.stamps, 5, Dt[0]);

    // ---- one thread per row: the blocks of the row in order (tensor.c:438-471), epilogue --------------------------------------------
    if constexpr (NB > 1) {
        // a thread per (sequence, row): the blocks of the row in order, the epilogue of its sequence
        const uint32_t obs = sel == 0 ? CHUNK_A.out_bstride[0] : sel == 1 ? CHUNK_A.out_bstride[1] : CHUNK_A.out_bstride[2];
        for (uint32_t idx = tid; idx < CHUNK_A.nb * rwl; idx += nthr) {
            const uint32_t b = idx / rwl, r = idx - b * rwl;
            float res[2] = {0.0f, 0.0f};
            for (uint32_t mat = 0; mat < nmat; mat++) {
                const float *f = Dt + (((size_t)mat * NB + b) * RW + r) * BP;
                float line = 0.0f;
                uint32_t blk = 0;
                for (; blk + 4 <= bpl; blk += 4) {
                    const float d0 = f[blk], d1 = f[blk + 1], d2 = f[blk + 2], d3 = f[blk + 3];
                    line += d0; line += d1; line += d2; line += d3;
                }
                for (; blk < bpl; blk++) line += f[blk];
                res[mat] = line;
            }
            float *o = out0 + (size_t)b * obs + (ops ? (size_t)CHUNK_A.pos[b] * ops : 0u) + lrow0 + r;
            const float old = epi == GEMV_EPI_RESID ? *o : 0.0f;
            const float add = has_add ? CHUNK_A.resid_add[(size_t)b * CHUNK_A.resid_add_bstride + lrow0 + r] : 0.0f;
            const float v = finish_epi(epi, has_add ? res[0] + add : res[0], res[1], old);
            __hip_atomic_store(o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        NANO_STAMP_END(CHUNK_A.stamps, 6);
        return;
    }
    float val = 0.0f;
    if (fold_live) {
        float res[2] = {0.0f, 0.0f};
        for (uint32_t mat = 0; mat < nmat; mat++) {
            const float *f = Dt + ((size_t)mat * RW + tid) * BP;
            float line = 0.0f;
            uint32_t blk = 0;
            for (; blk + 4 <= bpl; blk += 4) {                          // four reads go out together; the sum itself is serial (the reference's order)
                const float d0 = f[blk], d1 = f[blk + 1], d2 = f[blk + 2], d3 = f[blk + 3];
                line += d0; line += d1; line += d2; line += d3;
            }
            for (; blk < bpl; blk++) line += f[blk];
            res[mat] = line;
        }
        val = finish_epi(epi, has_add ? res[0] + addv : res[0], res[1], oldv);
        if constexpr (CHUNK_HAND == 1)                                  // (the granule first: a waiting workgroup sits behind it)
            __hip_atomic_store(CHUNK_HANDV.buf + (sel == 0 ? CHUNK_HANDV.base[0] : sel == 1 ? CHUNK_HANDV.base[1] : CHUNK_HANDV.base[2]) + lrow0 + tid,
                               ((unsigned long long)(CHUNK_PTAG) << 32) | (unsigned long long)__float_as_uint(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // write-through (sc1) store, see gemv_q80_impl.h: nothing is left for the write-back at the end of the kernel
        __hip_atomic_store(out0 + (size_t)opos * ops + lrow0 + tid, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // classifier launches (one STORE segment): this workgroup's (max, first row) arg-max partial, so that the arg-max kernel scans
    // gridDim.x pairs instead of every logit
    if (CHUNK_A.tile_max) {
        float bvv = fold_live ? val : -INFINITY;
        uint32_t bi = fold_live ? lrow0 + tid : 0xffffffffu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bvv, o, 64);
            const uint32_t oi = __shfl_xor(bi, o, 64);
            if (oi != 0xffffffffu && (bi == 0xffffffffu || ov > bvv || (ov == bvv && oi < bi))) { bvv = ov; bi = oi; }
        }
        if (lane == 0u) { am[2u * wid] = bvv; am[2u * wid + 1u] = __uint_as_float(bi); }
        __syncthreads();
        if (tid == 0u) {
            for (uint32_t w = 1; w < NW; w++) {
                const float ov = am[2u * w];
                const uint32_t oi = __float_as_uint(am[2u * w + 1u]);
                if (oi != 0xffffffffu && (bi == 0xffffffffu || ov > bvv || (ov == bvv && oi < bi))) { bvv = ov; bi = oi; }
            }
            float *tm = CHUNK_A.tile_max + (size_t)bid * 2;
            tm[0] = bvv; tm[1] = __uint_as_float(bi);
        }
    }
    NANO_STAMP_END(CHUNK_A.stamps, 6);
