// gemv_f32_slab_body.inc -- the statements of the FP32 SLAB GEMV kernel (gemv_f32.hip), included TEXTUALLY into the plain kernel and (round 6)
// into the fused q | k | v + attention launch of FP32 models -- the arrangement of gemv_q80_slab_body.inc, for the same reason.  The includer
// defines F32_A (the GemvDev), F32_BID (the workgroup's index among the GEMV workgroups) and F32_HAND 0 | 1 (the fold threads also store every
// result as an 8-byte {tag, value} granule: F32_HANDV the SlabHand, F32_PTAG the producers' tag), and has ROLE, B, NV, UPW and smem in scope.
    constexpr int TR = 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = (int)(F32_A.nthr >> 6);
    const uint32_t n = F32_A.n, n4 = (n + 3) & ~3u;
    const uint32_t nchunk = F32_A.nchunk, PC = (nchunk + 3) & ~3u;      // F32_A.nchunk: 256-float chunks per row
    const uint32_t RW = F32_A.rw;
    const uint32_t epi = role_epi<ROLE>(F32_A);
    const bool swiglu = epi == GEMV_EPI_SWIGLU;
    const uint32_t nmat = swiglu ? 2 : 1;
    float *xf = reinterpret_cast<float *>(smem);                   // [B][n4]
    float *red = xf + B * n4;                                      // [B][16] (+ combine weights [B][n_head][8])
    float *P = red + B * 16 + (has_flag<ROLE>(F32_A, F_COMBINE) ? B * F32_A.attn_n_head * 8 : 0);   // [B][nmat][RW][PC]

    Staged<B, NV> sx;
    stage_issue<ROLE, B, NV>(F32_A, sx);

    const uint32_t grow0 = (F32_BID) * RW;
    const uint32_t b0 = F32_A.rows[0], b1 = b0 + F32_A.rows[1];
    const int sel = swiglu ? 0 : (int)(grow0 >= b0) + (int)(grow0 >= b1);
    const float *w0 = reinterpret_cast<const float *>(sel == 0 ? F32_A.w[0] : sel == 1 ? F32_A.w[1] : F32_A.w[2]);
    float *out0 = sel == 0 ? F32_A.out[0] : sel == 1 ? F32_A.out[1] : F32_A.out[2];
    const uint32_t rows0 = sel == 0 ? F32_A.rows[0] : sel == 1 ? F32_A.rows[1] : F32_A.rows[2];
    const uint32_t obs = sel == 0 ? F32_A.out_bstride[0] : sel == 1 ? F32_A.out_bstride[1] : F32_A.out_bstride[2];
    const uint32_t ops = sel == 0 ? F32_A.out_pstride[0] : sel == 1 ? F32_A.out_pstride[1] : F32_A.out_pstride[2];
    const uint32_t lrow0 = grow0 - (sel == 0 ? 0u : sel == 1 ? b0 : b1);
    const uint32_t tmask = (1u << F32_A.log2_tiles) - 1u;

    float4 wv[UPW][TR];
#pragma unroll
    for (int k = 0; k < UPW; k++) {
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW;
        const uint32_t t = (u * F32_A.magic_nchunk) >> 16;                 // u / nchunk
        const uint32_t c = u - t * nchunk;
        const uint32_t tl = t & tmask, mat = t >> F32_A.log2_tiles;
        const bool live = u < F32_A.units;
        // (byte offsets and the descriptor's size are 32-bit: a weight tensor of rows * n * 4 >= 2^32 bytes is beyond this kernel)
        const __amdgpu_buffer_rsrc_t rw_ = mkrsrc(mat ? reinterpret_cast<const float *>(F32_A.w[1]) : w0, live ? rows0 * n * 4u : 0u);
        const uint32_t lrow = lrow0 + tl * TR;
        const uint32_t col = (c << 8) + (uint32_t)lane * 4u;
        const uint32_t base = (col < n) ? (lrow * n + col) * 4u : OOB;
#pragma unroll
        for (int r = 0; r < TR; r++) wv[k][r] = bload_wf(rw_, base + (uint32_t)r * n * 4u);
    }
    const int lrw = (int)F32_A.log2_tiles + 2;
    const int fb = tid >> lrw, frl = tid & ((int)RW - 1);
    const bool fold_live = tid < (int)(RW * B) && fb < (int)F32_A.nb && lrow0 + frl < rows0;
    // the position of a pos-indexed output (v-cache row) is fetched now and used only by the final store: no wait
    // here (a wait on it would also wait for every weight load issued above -- vmcnt counts in order)
    uint32_t opos = 0;
    if (ops && fold_live) opos = F32_A.pos[fb];
    float oldv = 0.0f;
    if (epi == GEMV_EPI_RESID && fold_live) oldv = out0[(size_t)fb * obs + lrow0 + frl];      // residual stream: never pos-indexed
    float addv = 0.0f;                                              // LoRA o-branch: x += (W.act + addv), reference order
    const bool has_add = epi == GEMV_EPI_RESID && F32_A.resid_add != nullptr;
    if (has_add && fold_live) addv = F32_A.resid_add[(size_t)fb * F32_A.resid_add_bstride + lrow0 + frl];

    stage_finish_f32<ROLE, B, NV>(F32_A, sx, xf, red, n4);

#pragma unroll
    for (int k = 0; k < UPW; k++) {
        const uint32_t u = (uint32_t)wid + (uint32_t)k * NW;
        if (u < F32_A.units) {
            const uint32_t t = (u * F32_A.magic_nchunk) >> 16;
            const uint32_t c = u - t * nchunk;
            const uint32_t tl = t & tmask, mat = t >> F32_A.log2_tiles;
            const uint32_t col = (c << 8) + (uint32_t)lane * 4u;
#pragma unroll
            for (int b = 0; b < B; b++) {
                if (b < (int)F32_A.nb) {
                    const float4 xv = (col < n) ? *reinterpret_cast<const float4 *>(xf + b * n4 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int r = 0; r < TR; r++) {
                        float p = wv[k][r].x * xv.x;
                        p = __builtin_fmaf(wv[k][r].y, xv.y, p); p = __builtin_fmaf(wv[k][r].z, xv.z, p); p = __builtin_fmaf(wv[k][r].w, xv.w, p);
                        p = dpp_wave_sum(p);
                        if (lane == 0) P[(((size_t)b * nmat + mat) * RW + tl * TR + r) * PC + c] = p;
                    }
                }
            }
        }
    }
    __syncthreads();

    if (tid < (int)(RW * B)) {
        float v0 = 0.0f, v1 = 0.0f;
        const float *p0 = P + (((size_t)fb * nmat) * RW + frl) * PC;
        const float *p1 = p0 + (size_t)RW * PC;
        for (uint32_t c = 0; c < nchunk; c++) { v0 += p0[c]; if (swiglu) v1 += p1[c]; }
        // write-through (sc1) store, see gemv_q80_impl.h: nothing is left for the write-back at the end of the kernel
        if constexpr (F32_HAND == 1) {
            if (fold_live) {
                const float val = finish_epi(epi, has_add ? v0 + addv : v0, v1, oldv);
                // (the granule first: a waiting workgroup sits behind it)
                __hip_atomic_store(F32_HANDV.buf + (sel == 0 ? F32_HANDV.base[0] : sel == 1 ? F32_HANDV.base[1] : F32_HANDV.base[2]) + lrow0 + (uint32_t)frl,
                                   ((unsigned long long)(F32_PTAG) << 32) | (unsigned long long)__float_as_uint(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(out0 + (size_t)fb * obs + (size_t)opos * ops + lrow0 + frl, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else
        if (fold_live) __hip_atomic_store(out0 + (size_t)fb * obs + (size_t)opos * ops + lrow0 + frl, finish_epi(epi, has_add ? v0 + addv : v0, v1, oldv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
