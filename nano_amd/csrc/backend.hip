// backend.hip -- the C-ABI device backend declared in include/nano_mi355x.h: create / destroy / layout, the forward / prefill / greedy
// entry points, the sticky error word and the re-issue policy (backend_model.h lists the other translation units).
//
// Owns: the device copy of the model's parameter blob (each tensor re-based to a 256-byte aligned address; Q4K tensors lose their
// 44-byte frame prefix so that 160-byte blocks are 16-byte aligned; otherwise the row-major weight blocks stay byte-for-byte as in the
// model file), the KV cache and the per-sequence scratch, and the HIP graphs of one decode step (backend_step.hip):
//   embed -> L x [ QKV GEMV | attention | Wo GEMV(+residual) | W1/W3 GEMV(+SwiGLU) | W2 GEMV(+residual) ] -> classifier GEMV -> arg-max
// all on one stream, captured once per (batch, mode, range) and replayed.  Attention is split over the sequence; its partials are
// combined in the Wo GEMV's prologue (no extra launch).
#include "backend_model.h"

static thread_local std::string g_err;
extern "C" const char *nano_hip_last_error(void) { return g_err.c_str(); }
extern "C" void nano_hip_set_error_(const char *msg) { g_err = msg ? msg : ""; }

// ---- device info ----
extern "C" int nano_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int nano_hip_device_info(int device, char *name, size_t cap, uint64_t *total_mem) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (name && cap) { strncpy(name, p.gcnArchName, cap - 1); name[cap - 1] = 0; }
    if (total_mem) *total_mem = p.totalGlobalMem;
    return p.multiProcessorCount;
}

// ---- parameter blob layout (reference infer/infer.c:100-217) ----
struct Piece { size_t src_off, bytes, dst_off; };

static void shapes(const NanoModelDesc &d, uint32_t &hd, uint32_t &QD, uint32_t &KD) {
    if (d.arch == NANO_ARCH_QWEN3) { hd = d.head_dim; QD = hd * d.n_head; KD = hd * d.n_kv_head; }
    else { hd = d.n_embd / d.n_head; QD = d.n_embd; KD = (d.n_embd * d.n_kv_head) / d.n_head; }
}

extern "C" size_t nano_hip_params_bytes(const NanoModelDesc *d) {
    if (!d || d->quant_type == NANO_QUANT_Q4K) return 0;
    uint32_t hd, QD, KD; shapes(*d, hd, QD, KD);
    const size_t L = d->n_layer, E = d->n_embd, H = d->n_hidden, V = d->vocab_size;
    const size_t P = V * E + L * (2 * (size_t)QD * E + 2 * (size_t)KD * E + 3 * H * E);
    size_t sz = 4 * (2 * L * E + E);
    sz += weight_bytes(d->quant_type, d->group_size, P);
    if (d->arch == NANO_ARCH_QWEN2) sz += 4 * L * ((size_t)QD + 2 * KD);
    if (d->arch == NANO_ARCH_QWEN3) sz += 8 * L * hd;
    sz += 8 * ((size_t)d->block_size * hd / 2);
    if (!d->is_shared_classifier) sz += weight_bytes(d->quant_type, d->group_size, V * E);
    return sz;
}

static int copy_in(void *dst, const void *src, size_t bytes, int src_on_device) {
    HIP_TRY(hipMemcpy(dst, src, bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return 0;
}
static int peek(void *host_dst, const uint8_t *src, size_t bytes, int src_on_device) {
    if (src_on_device) { HIP_TRY(hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost)); }
    else memcpy(host_dst, src, bytes);
    return 0;
}

static void destroy(NanoHipModel *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->st) (void)hipStreamSynchronize(m->st);
    for (auto &kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
    void *dev[] = { m->arena, m->x, m->q, m->kraw, m->xba, m->hb, m->logits, m->kcache, m->vcache,
                    m->tokens, m->pos, m->amax, m->trace, m->pos0, m->attn_part, m->attn_ml, m->tile_max, m->rope_cur, m->gq, m->gxs, m->lt.at.buf, m->lora_o1,
                    m->xn, m->hb2, m->att, m->vraw, m->stamp.buf, m->kv.pt, m->kv.kvrow, m->ho.hand, m->ho.hand2, m->ho.tick, m->kv.jobs, m->q4x, m->f32x, m->rows.vraw };
    for (void *p : dev) if (p) (void)hipFree(p);
    for (auto &en : m->lt.e) if (en.buf) (void)hipFree(en.buf);
    if (m->lt.desc) (void)hipFree(m->lt.desc);
    void *host[] = { m->h_tokens, m->h_pos, m->h_amax, m->h_logits, m->kv.h_pt, m->h_err };
    for (void *p : host) if (p) (void)hipHostFree(p);
    sampler_free(m->smp);
    lookup_free(m);
    lookup_rows_free(m);
    draft_free(m);
    rows_free(m);
    kv_image_free(m);
    for (hipEvent_t ev : { m->ev0, m->ev1, m->ev2 }) if (ev) (void)hipEventDestroy(ev);
    if (m->st) (void)hipStreamDestroy(m->st);
    delete m;
}

extern "C" void nano_hip_model_destroy(NanoHipModel *m) { destroy(m); }

extern "C" int nano_hip_model_create(NanoHipModel **out, const NanoModelDesc *desc, const void *params, size_t params_bytes,
                                     int params_on_device, int device, uint32_t max_seq_len, uint32_t max_batch) {
    uint32_t flags = 0;
    if (const char *kv = getenv("NANO_KV_F16")) if (*kv && *kv != '0') flags |= NANO_HIP_KV_F16;
    if (const char *k8 = getenv("NANO_KV_FP8")) if (*k8 && *k8 != '0') flags |= NANO_HIP_KV_FP8;      // (with NANO_KV_F16: refused below)
    if (const char *kp = getenv("NANO_KV_PAGED")) if (*kp && *kp != '0') flags |= NANO_HIP_KV_PAGED;
    return nano_hip_model_create_ex(out, desc, params, params_bytes, params_on_device, device, max_seq_len, max_batch, flags);
}

extern "C" int nano_hip_model_create_ex(NanoHipModel **out, const NanoModelDesc *desc, const void *params, size_t params_bytes,
                                        int params_on_device, int device, uint32_t max_seq_len, uint32_t max_batch, uint32_t flags) {
    if (!out || !desc || !params) FAIL(NANO_HIP_EINVAL, "null argument");
    if (flags & ~(NANO_HIP_KV_F16 | NANO_HIP_KV_PAGED | NANO_HIP_KV_FP8)) FAIL(NANO_HIP_EINVAL, "unknown flags 0x%x", flags);
    if ((flags & NANO_HIP_KV_F16) && (flags & NANO_HIP_KV_FP8)) FAIL(NANO_HIP_EINVAL, "NANO_HIP_KV_F16 and NANO_HIP_KV_FP8 (NANO_KV_F16 / NANO_KV_FP8) both set: the KV cache has one element format");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FAIL(NANO_HIP_ENODEV, "no HIP device visible (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev) FAIL(NANO_HIP_EINVAL, "device %d out of range (%d devices)", device, ndev);
    const NanoModelDesc &d = *desc;
    if (d.quant_type != NANO_QUANT_F32 && d.quant_type != NANO_QUANT_Q80 && d.quant_type != NANO_QUANT_Q4K)
        FAIL(NANO_HIP_EINVAL, "unknown quant type 0x%x", d.quant_type);
    if (max_batch == 0 || max_batch > NANO_MAX_BATCH || max_seq_len == 0) FAIL(NANO_HIP_EINVAL, "bad max_batch/max_seq_len");
    uint32_t hd, QD, KD; shapes(d, hd, QD, KD);
    if (d.n_head == 0 || d.n_kv_head == 0 || d.n_head % d.n_kv_head) FAIL(NANO_HIP_EINVAL, "bad head counts");
    if (hd == 0 || hd % 4 || hd > 256) FAIL(NANO_HIP_EINVAL, "head_dim %u unsupported (needs %%4==0, <=256)", hd);
    if (d.n_embd % 16 || QD % 16 || d.n_hidden % 16) FAIL(NANO_HIP_EINVAL, "n_embd/q_dim/n_hidden must be multiples of 16");
    if (d.quant_type == NANO_QUANT_Q80) {
        const uint32_t gs = d.group_size;
        if (!(gs == 32 || gs == 64 || gs == 128 || gs == 256)) FAIL(NANO_HIP_EINVAL, "Q80 group size %u unsupported (32/64/128/256)", gs);
        if (d.n_embd % gs || QD % gs || d.n_hidden % gs) FAIL(NANO_HIP_EINVAL, "group size must divide n_embd, q_dim, n_hidden");
    }
    if (!d.is_shared_classifier && d.quant_type == NANO_QUANT_Q4K) FAIL(NANO_HIP_EINVAL, "Q4K classifier is always shared (reference infer.c:211)");

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        FAIL(NANO_HIP_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);

    NanoHipModel *m = new NanoHipModel();
    m->d = d; m->device = device; m->cus = prop.multiProcessorCount;
    m->S = max_seq_len; m->maxB = max_batch; m->hd = hd; m->QD = QD; m->KD = KD;
    m->kv_half = (flags & NANO_HIP_KV_FP8) ? KV_FMT_FP8 : (flags & NANO_HIP_KV_F16) ? KV_FMT_F16 : KV_FMT_F32;
    m->kv.paged = (flags & NANO_HIP_KV_PAGED) != 0;
    m->params_bytes = params_bytes;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(params);
    const size_t L = d.n_layer, E = d.n_embd, H = d.n_hidden, V = d.vocab_size;
    const size_t each[WCOUNT] = { (size_t)QD * E, (size_t)KD * E, (size_t)KD * E, E * QD, H * E, E * H, H * E };
    const size_t rows_of[WCOUNT] = { QD, KD, KD, E, H, E, H };
    const size_t cols_of[WCOUNT] = { E, E, E, QD, E, H, E };

    // ---- pass 1: walk the blob, record pieces -----------------------------------------------------
    std::vector<Piece> pieces;
    size_t so = 0, doff = 0;
    auto add = [&](size_t bytes, size_t skip_prefix = 0) -> size_t {
        doff = align_up(doff, 256);
        Piece p{ so + skip_prefix, bytes - skip_prefix, doff };
        pieces.push_back(p);
        so += bytes; doff += bytes - skip_prefix;
        return p.dst_off;
    };
    size_t o_rms_attn = add(4 * L * E), o_rms_ffn = add(4 * L * E), o_rms_final = add(4 * E);
    size_t o_tok_w = 0, o_tok_s = 0, o_cls_w = 0, o_cls_s = 0;
    std::vector<size_t> o_w[WCOUNT], o_s[WCOUNT];
    int rc = 0;
    if (d.quant_type == NANO_QUANT_Q80) {
        o_tok_w = add(V * E); o_tok_s = add(4 * (V * E / d.group_size));
        for (int k = 0; k < WCOUNT; k++)
            for (size_t l = 0; l < L; l++) { o_w[k].push_back(add(each[k])); o_s[k].push_back(add(4 * (each[k] / d.group_size))); }
    } else if (d.quant_type == NANO_QUANT_Q4K) {
        for (int k = -1; k < WCOUNT; k++) {
            uint64_t frame = 0;
            if (so + 8 > params_bytes) { destroy(m); FAIL(NANO_HIP_EINVAL, "parameter blob truncated (Q4K frame)"); }
            if ((rc = peek(&frame, src + so, 8, params_on_device))) { destroy(m); return rc; }
            const size_t rows = (k < 0) ? V : L * rows_of[k], cols = (k < 0) ? E : cols_of[k];
            const size_t expect = 44 + rows * ((cols + 255) / 256) * 160;
            if (frame != expect) { destroy(m); FAIL(NANO_HIP_EINVAL, "Q4K tensor %d: frame %llu bytes, expected %zu", k, (unsigned long long)frame, expect); }
            size_t o = add(frame, 44);
            if (k < 0) o_tok_w = o; else o_w[k].push_back(o);
        }
    } else {
        o_tok_w = add(4 * V * E);
        for (int k = 0; k < WCOUNT; k++) o_w[k].push_back(add(4 * L * each[k]));
    }
    size_t o_qn = 0, o_kn = 0;
    if (d.arch == NANO_ARCH_QWEN2) so += 4 * L * ((size_t)QD + 2 * KD);        // biases: mapped, never applied (infer.c:788-790)
    if (d.arch == NANO_ARCH_QWEN3) { o_qn = add(4 * L * hd); o_kn = add(4 * L * hd); }
    const size_t rope_file_n = (size_t)d.block_size * hd / 2;
    const size_t rope_rows = (d.block_size < max_seq_len) ? d.block_size : max_seq_len;   // rows actually indexable
    size_t o_cos = 0, o_sin = 0;
    if (d.arch == NANO_ARCH_QWEN3) {
        so += 8 * rope_file_n;                                                   // skipped and recomputed (infer.c:189-204)
        doff = align_up(doff, 256); o_cos = doff; doff += 4 * rope_rows * hd / 2;
        doff = align_up(doff, 256); o_sin = doff; doff += 4 * rope_rows * hd / 2;
    } else {
        o_cos = add(4 * rope_file_n); o_sin = add(4 * rope_file_n);
    }
    if (!d.is_shared_classifier) {
        if (d.quant_type == NANO_QUANT_Q80) { o_cls_w = add(V * E); o_cls_s = add(4 * (V * E / d.group_size)); }
        else if (d.quant_type == NANO_QUANT_F32) {
            // FP32 un-shared: the reference's classifier pointer is the stale START of the parameter blob (infer.c:215):
            // it reads vocab x n_embd floats from there (norm weights, then the embedding table).  The tensors are re-based
            // individually in the arena, so the aliased view gets a contiguous copy of its own.
            doff = align_up(doff, 256);
            pieces.push_back(Piece{ 0, 4 * V * E, doff });
            o_cls_w = doff; doff += 4 * V * E;
        }
    }
    if (so > params_bytes) { destroy(m); FAIL(NANO_HIP_EINVAL, "parameter blob too small: need %zu bytes, got %zu", so, params_bytes); }

    // ---- pass 2: allocate + upload -------------------------------------------------------------------
    m->arena_bytes = align_up(doff, 256) + 256;
    if (hipMalloc(&m->arena, m->arena_bytes) != hipSuccess) { destroy(m); FAIL(NANO_HIP_ENOMEM, "hipMalloc(%zu) for weights failed", m->arena_bytes); }
    for (const Piece &p : pieces)
        if ((rc = copy_in(m->arena + p.dst_off, src + p.src_off, p.bytes, params_on_device))) { destroy(m); return rc; }
    if (d.arch == NANO_ARCH_QWEN3) {
        // same libm calls as the reference loader (infer.c:193-201), host side
        std::vector<float> c(rope_rows * hd / 2), s(rope_rows * hd / 2);
        for (uint32_t pos = 0; pos < rope_rows; pos++)
            for (uint32_t i = 0; i < hd / 2; i++) {
                float freq = 1.0f / powf(1000000.0f, (float)(i * 2) / (float)hd);
                c[(size_t)pos * hd / 2 + i] = cosf(pos * freq);
                s[(size_t)pos * hd / 2 + i] = sinf(pos * freq);
            }
        if ((rc = copy_in(m->arena + o_cos, c.data(), c.size() * 4, 0)) || (rc = copy_in(m->arena + o_sin, s.data(), s.size() * 4, 0))) { destroy(m); return rc; }
    }
    auto F = [&](size_t o) { return reinterpret_cast<const float *>(m->arena + o); };
    m->rms_attn = F(o_rms_attn); m->rms_ffn = F(o_rms_ffn); m->rms_final = F(o_rms_final);
    m->rope_cos = F(o_cos); m->rope_sin = F(o_sin);
    m->rope_rows = (d.arch == NANO_ARCH_QWEN3) ? (uint32_t)rope_rows : d.block_size;
    if (d.arch == NANO_ARCH_QWEN3) { m->q_norm = F(o_qn); m->k_norm = F(o_kn); }
    m->tok.w = m->arena + o_tok_w; m->tok.s = (d.quant_type == NANO_QUANT_Q80) ? F(o_tok_s) : nullptr;
    for (int k = 0; k < WCOUNT; k++) {
        m->W[k].resize(L);
        for (size_t l = 0; l < L; l++) {
            if (d.quant_type == NANO_QUANT_Q80) { m->W[k][l].w = m->arena + o_w[k][l]; m->W[k][l].s = F(o_s[k][l]); }
            else if (d.quant_type == NANO_QUANT_Q4K) m->W[k][l].w = m->arena + o_w[k][0] + l * rows_of[k] * ((cols_of[k] + 255) / 256) * 160;
            else m->W[k][l].w = m->arena + o_w[k][0] + 4 * l * each[k];
        }
    }
    if (d.is_shared_classifier) m->cls = m->tok;
    else if (d.quant_type == NANO_QUANT_Q80) { m->cls.w = m->arena + o_cls_w; m->cls.s = F(o_cls_s); }
    else m->cls.w = m->arena + o_cls_w;      /* FP32: the copy of the blob's first vocab x n_embd floats (see above) */

    {   // algorithmic weight bytes per decode step
        const uint64_t P = (uint64_t)V * E + L * (2 * (uint64_t)QD * E + 2 * (uint64_t)KD * E + 3 * (uint64_t)H * E);
        m->weight_bytes_per_step = weight_bytes(d.quant_type, d.group_size, P);
    }

    // ---- state ---------------------------------------------------------------------------------------
    const size_t B = max_batch;
    if (const char *mm = getenv("NANO_MFMA_MIN_NB")) { const uint32_t v = (uint32_t)strtoul(mm, nullptr, 0); if (v >= 2) m->mfma_min_nb = v; }
    // FP32's own minimum for its MFMA GEMM (gemm_f32.hip); NANO_MFMA_MIN_NB can only raise it (65: the slices of 8, the A/B switch)
    if (m->mfma_min_nb > m->f32_min_nb) m->f32_min_nb = m->mfma_min_nb;
    // per-token scratch also serves batched prefill: up to 64 (Q80, and Q4K / FP32 where gemm_q4k.hip / gemm_f32.hip takes all seven
    // per-layer projections: MFMA GEMMs) / 8 prompt tokens per pass.  Decided here, once, from the shapes and the minimum.
    m->pf_chunk = d.quant_type == NANO_QUANT_Q80 ? 64u : 8u;
    const bool f32 = d.quant_type == NANO_QUANT_F32;
    if ((d.quant_type == NANO_QUANT_Q4K && m->mfma_min_nb <= 64u) || (f32 && m->f32_min_nb <= 64u)) {
        auto takes = [&](uint32_t n, uint32_t epi, uint32_t r0, uint32_t r1, uint32_t r2) {
            GemvArgs a{};
            a.n = n; a.nb = 64; a.epi = epi; a.cus = (uint32_t)m->cus;
            const uint32_t rows[3] = { r0, r1, r2 };
            for (uint32_t s = 0; s < 3 && rows[s]; s++) { a.seg[s].rows = rows[s]; a.nseg = s + 1; }
            if (epi != GEMV_EPI_RESID) a.norm_w = m->rms_attn;                  // (a flag here: q | k | v and W1|W3 normalise in their prologue)
            return f32 ? gemm_f32_supports(a) : gemm_q4k_supports(a);
        };
        if (takes((uint32_t)E, GEMV_EPI_STORE, QD, KD, KD) && takes(QD, GEMV_EPI_RESID, (uint32_t)E, 0, 0) &&
            takes((uint32_t)E, GEMV_EPI_SWIGLU, (uint32_t)H, (uint32_t)H, 0) && takes((uint32_t)H, GEMV_EPI_RESID, (uint32_t)E, 0, 0)) m->pf_chunk = 64u;
    }
    const size_t PF = m->pf_chunk;
    const size_t Bs = B > PF ? B : PF;
    m->Bs = (uint32_t)Bs;
    size_t kvn = B * L * max_seq_len * KD;
    if (m->kv.paged) {
        m->kv.pt_stride = (max_seq_len + 63) / 64;
        m->kv.pages = (uint32_t)B * m->kv.pt_stride;
        // a layer plane is addressed with 32-bit byte offsets (buffer descriptors): pages x 64 rows x kv_dim x element size < 4 GB.  The
        // DEFAULT pool (every slot's whole context) is clamped to that with a log line; an explicit NANO_KV_PAGES beyond it is refused.
        const uint64_t esz_kv = kv_esz(m), page_b = 64ull * KD * esz_kv, max_pages = (((1ull << 32) - (1u << 20)) / page_b);
        if (m->kv.pages > max_pages) {
            fprintf(stderr, "nano_hip: paged KV cache: default pool of %u pages clamped to %llu (a layer plane is limited to 4 GB: 64 rows x %u x %llu B per page); set NANO_KV_PAGES to choose\n",
                    m->kv.pages, (unsigned long long)max_pages, KD, (unsigned long long)esz_kv);
            m->kv.pages = (uint32_t)max_pages;
        }
        if (const char *np = getenv("NANO_KV_PAGES")) { const unsigned long v = strtoul(np, nullptr, 0); if (v >= 1 && v <= (1ul << 24)) m->kv.pages = (uint32_t)v; }
        if ((uint64_t)m->kv.pages > max_pages) { destroy(m); FAIL(NANO_HIP_EINVAL, "paged KV cache: %u pages x 64 rows x %u elements of %llu B exceed a 4 GB layer plane (at most %llu pages)", m->kv.pages, KD, (unsigned long long)esz_kv, (unsigned long long)max_pages); }
        kvn = L * (size_t)m->kv.pages * 64 * KD;
    }
    m->trace_cap = max_seq_len * max_batch;
    m->nsplit_cap = max_seq_len > attention_wide_from() ? attention_split_cap() : 8;     // partial buffers are sized for the maximum
    bool ok = hipMalloc(&m->x, Bs * E * 4) == hipSuccess && hipMalloc(&m->q, Bs * QD * 4) == hipSuccess &&
              hipMalloc(&m->kraw, Bs * KD * 4) == hipSuccess && hipMalloc(&m->xba, Bs * QD * 4) == hipSuccess &&
              hipMalloc(&m->hb, Bs * H * 4) == hipSuccess && hipMalloc(&m->logits, B * V * 4) == hipSuccess &&
              hipMalloc(&m->kcache, kvn * kv_esz(m)) == hipSuccess && hipMalloc(&m->vcache, kvn * kv_esz(m)) == hipSuccess &&
              (!m->kv_half || hipMalloc(&m->vraw, Bs * KD * 4) == hipSuccess) &&
              hipMalloc(&m->tokens, Bs * 4) == hipSuccess && hipMalloc(&m->pos, Bs * 4) == hipSuccess &&
              hipMalloc(&m->amax, B * 4) == hipSuccess && hipMalloc(&m->trace, (size_t)m->trace_cap * 4) == hipSuccess &&
              hipMalloc(&m->pos0, B * 4) == hipSuccess &&
              hipMalloc(&m->attn_part, Bs * m->nsplit_cap * QD * 4) == hipSuccess &&
              hipMalloc(&m->attn_ml, Bs * d.n_head * m->nsplit_cap * 2 * 4) == hipSuccess &&
              hipMalloc(&m->tile_max, B * V * 2 * 4) == hipSuccess &&
              hipMalloc(&m->rope_cur, Bs * m->hd * 4 + 64) == hipSuccess;
    if (ok && Bs > 8 && d.quant_type == NANO_QUANT_Q80) {
        size_t nmax = E > QD ? E : QD; if (H > nmax) nmax = H;
        ok = hipMalloc(&m->gq, Bs * ((nmax + 15) & ~(size_t)15)) == hipSuccess && hipMalloc(&m->gxs, Bs * (nmax / d.group_size) * 4) == hipSuccess;
    }
    if (ok && Bs > 1 && d.quant_type == NANO_QUANT_Q4K) {
        size_t nmax = E > QD ? E : QD; if (H > nmax) nmax = H;
        // 32 bytes per 32-value group: up to 8 sequences per chunk launch, up to 64 per GEMM launch (gemm_q4k.hip)
        m->q4x_bytes = (Bs > 8 ? (Bs < 64 ? Bs : (size_t)64) : (size_t)8) * ((nmax + 255) & ~(size_t)255);
        ok = hipMalloc(&m->q4x, m->q4x_bytes) == hipSuccess;
    }
    if (ok && Bs > 8 && f32 && m->f32_min_nb <= 64u) {
        size_t nmax = E > QD ? E : QD; if (H > nmax) nmax = H;
        // up to 64 tokens per GEMM launch, every row padded to whole 128-float units (gemm_f32.hip)
        m->f32x_floats = (size_t)64 * ((nmax + 127) & ~(size_t)127);
        ok = hipMalloc(&m->f32x, m->f32x_floats * 4) == hipSuccess;
    }
    if (ok && m->kv.paged) {
        const size_t ptn = B * m->kv.pt_stride;
        ok = hipMalloc(&m->kv.pt, ptn * 4) == hipSuccess && hipMalloc(&m->kv.kvrow, Bs * 4) == hipSuccess && hipHostMalloc(&m->kv.h_pt, ptn * 4) == hipSuccess &&
             hipMemset(m->kv.pt, 0xff, ptn * 4) == hipSuccess && hipMemset(m->kv.kvrow, 0, Bs * 4) == hipSuccess;
        if (ok) {
            memset(m->kv.h_pt, 0xff, ptn * 4);
            for (uint32_t pg = m->kv.pages; pg-- > 0;) m->kv.free_pages.push_back(pg);           // pages are handed out in ascending order
            m->kv.page_owners.assign(m->kv.pages, 0u);
        }
    }
    if (!ok) { destroy(m); FAIL(NANO_HIP_ENOMEM, "hipMalloc for KV cache / scratch failed (batch %zu, seq %u)", B, max_seq_len); }
    // calloc semantics of the reference (infer.c:33,47): non-causal attention reads unwritten rows
    if (hipMemset(m->kcache, 0, kvn * kv_esz(m)) != hipSuccess || hipMemset(m->vcache, 0, kvn * kv_esz(m)) != hipSuccess ||
        hipMemset(m->x, 0, Bs * E * 4) != hipSuccess || hipMemset(m->logits, 0, B * V * 4) != hipSuccess ||
        hipMemset(m->tokens, 0, Bs * 4) != hipSuccess || hipMemset(m->pos, 0, Bs * 4) != hipSuccess ||
        hipMemset(m->pos0, 0, B * 4) != hipSuccess) { destroy(m); FAIL(NANO_HIP_ERUNTIME, "hipMemset failed"); }
    ok = hipHostMalloc(&m->h_tokens, Bs * 4) == hipSuccess && hipHostMalloc(&m->h_pos, Bs * 4) == hipSuccess &&
         hipHostMalloc(&m->h_amax, (size_t)m->trace_cap * 4) == hipSuccess && hipHostMalloc(&m->h_logits, B * V * 4) == hipSuccess;
    if (!ok) { destroy(m); FAIL(NANO_HIP_ENOMEM, "hipHostMalloc failed"); }
    if (hipHostMalloc(reinterpret_cast<void **>(&m->h_err), 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&m->dev_err), m->h_err, 0) != hipSuccess) { destroy(m); FAIL(NANO_HIP_ENOMEM, "hipHostMalloc (mapped) failed"); }
    *m->h_err = 0;
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&m->ev0) != hipSuccess ||
        hipEventCreate(&m->ev1) != hipSuccess || hipEventCreate(&m->ev2) != hipSuccess) { destroy(m); FAIL(NANO_HIP_ERUNTIME, "stream/event creation failed"); }
    if (getenv("NANO_HIP_NO_GRAPH")) m->use_graph = false;
    if (const char *nt = getenv("NANO_KV_COPY_NT")) m->kv.copy_nt = *nt && *nt != '0';
    // NANO_FUSE_LAUNCHES: bit 0 = q | k | v + attention in one launch, bit 1 = Wo + W1|W3 in one launch (higher bits are ignored).
    // Default 3; 0 = the five launches per layer; same bits in every setting
    if (const char *fz = getenv("NANO_FUSE_LAUNCHES")) { const uint32_t v = (uint32_t)strtoul(fz, nullptr, 0); m->ho.fuse_qkv_attn = (v & 1u) != 0; m->ho.fuse_wo_w13 = (v & 2u) != 0; }
    if (const char *cwv = getenv("NANO_COMBINE_WAVE")) m->ho.combine_wave = *cwv != '0';
    {
        // granule buffers of the fused one-sequence launches (hand2: the Wo + W1|W3 launch, Q80 only)
        const bool gran = (m->d.quant_type == NANO_QUANT_Q80 && m->d.group_size == 64) || m->d.quant_type == NANO_QUANT_Q4K || m->d.quant_type == NANO_QUANT_F32;
        const size_t g1 = gran ? (size_t)m->QD + 2 * (size_t)m->KD : 0, g2 = (gran && m->d.quant_type == NANO_QUANT_Q80) ? (size_t)m->d.n_embd : 0;
        if (handoff_alloc(&m->ho.tick, &m->ho.hand, g1, &m->ho.hand2, g2) != hipSuccess) { destroy(m); FAIL(NANO_HIP_ENOMEM, "hipMalloc of the hand-off words and granules failed"); }
    }
    HIP_TRY(hipDeviceSynchronize());
    *out = m;
    if (const char *xm = getenv("NANO_EXACT")) if (*xm && *xm != '0') { const int rc = nano_hip_set_exact(m, 1); if (rc) return rc; }
    if (const char *sm = getenv("NANO_STRICT")) if (*sm && *sm != '0') return nano_hip_set_strict(m, 1);
    return NANO_HIP_OK;
}

extern "C" int nano_hip_model_device(const NanoHipModel *m) { return m ? m->device : -1; }
extern "C" uint64_t nano_hip_weight_bytes_per_step(const NanoHipModel *m) { return m ? m->weight_bytes_per_step : 0; }
// The hand-off state of the fused one-sequence launches (device_common.h): the three tick words (64 bytes) and the granule buffers of
// `granules` / `granules2` 8-byte {tag, value} entries (0: none, and then hand / hand2 may be null), all zeroed -- tag 0 (the memset) is no epoch: the first step's tick is 1.
// A model's (above) and the fused-launch operators' (ops.hip) come from here.  On failure whatever was allocated stays with the caller.
hipError_t nano::handoff_alloc(uint32_t **tick, unsigned long long **hand, size_t granules, unsigned long long **hand2, size_t granules2) {
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void **>(tick), 64)) != hipSuccess || (e = hipMemset(*tick, 0, 64)) != hipSuccess) return e;
    if (granules && ((e = hipMalloc(reinterpret_cast<void **>(hand), granules * 8)) != hipSuccess || (e = hipMemset(*hand, 0, granules * 8)) != hipSuccess)) return e;
    if (granules2 && ((e = hipMalloc(reinterpret_cast<void **>(hand2), granules2 * 8)) != hipSuccess || (e = hipMemset(*hand2, 0, granules2 * 8)) != hipSuccess)) return e;
    return hipSuccess;
}
// A kernel gave up a bounded wait since the last check (G6's finisher, a fused launch's hand-off):
// the results of the call are not valid.  Read after a stream synchronisation; the word lives in host-mapped memory, so the check
// is one load.  dev_err_take() returns the code bits and clears the word (m->ho.last_dev_err keeps them); dev_err_check() turns
// them into NANO_HIP_ERUNTIME.  Every public entry point that synchronises ends with one of the two (round-5 advice: the
// arg-max sampling path and an allocation-failure exit of the sampler returned without looking).
uint32_t dev_err_take(NanoHipModel *m) {
    const uint32_t c = m->h_err ? *reinterpret_cast<volatile uint32_t *>(m->h_err) : 0u;
    if (!c) return 0u;
    *reinterpret_cast<volatile uint32_t *>(m->h_err) = 0;
    m->ho.last_dev_err = c;
    if (m->ho.tick) (void)hipMemsetAsync(m->ho.tick + 2, 0, 4, m->st);         // the abort flag of the lost step (device_common.h)
    return c;
}
int dev_err_fail(uint32_t c) {
    FAIL(NANO_HIP_ERUNTIME, "a kernel gave up waiting for its producers (code %u: 1 = G6 tile counter, 2 = in-launch hand-off of a fused launch): the results of this call are not valid", c);
}
int dev_err_check(NanoHipModel *m) {
    const uint32_t c = dev_err_take(m);
    return c ? dev_err_fail(c) : 0;
}
// The in-launch hand-offs of the fused one-sequence launches are an optimisation over launches that need nothing from each other but
// stream order.  When one gives up -- the chip shared with other work that kept its producers off the CUs for longer than the bound -- the
// engine switches them off for this model, drops the graphs that contain them and re-issues the call (backend_model.h with_reissue).
void drop_graphs(NanoHipModel *m) {
    for (auto &kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
    m->graphs.clear(); m->pf_graph_keys.clear(); m->exact_nodes.clear();
}
void handoff_fallback(NanoHipModel *m) {
    (void)hipStreamSynchronize(m->st);
    m->ho.fuse_qkv_attn = m->ho.fuse_wo_w13 = false;
    drop_graphs(m);
    m->ho.fallbacks++;
}

extern "C" int nano_hip_sync(NanoHipModel *m) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    return dev_err_check(m);
}

int check_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, uint32_t extra_steps) {
    if (!m || !tokens || !pos) FAIL(NANO_HIP_EINVAL, "null argument");
    const uint32_t cap = NANO_MAX_BATCH;               // > 8 sequences: Q80, Q4K and FP32 through their MFMA GEMMs, shapes a GEMM refuses through the GEMV kernels in groups
    if (batch == 0 || batch > m->maxB || batch > cap) FAIL(NANO_HIP_EINVAL, "batch %u out of range (max %u, kernel capacity %u)", batch, m->maxB, cap);
    for (uint32_t i = 0; i < batch; i++) {
        if (tokens[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "token %u out of vocabulary", tokens[i]);
        if ((uint64_t)pos[i] + (extra_steps ? extra_steps - 1 : 0) >= (uint64_t)m->S) FAIL(NANO_HIP_EINVAL, "position %u (+%u steps) exceeds max_seq_len %u", pos[i], extra_steps, m->S);
        if ((uint64_t)pos[i] + (extra_steps ? extra_steps - 1 : 0) >= (uint64_t)m->rope_rows) FAIL(NANO_HIP_EINVAL, "position %u (+%u steps) exceeds the model's RoPE table (%u rows = block_size)", pos[i], extra_steps, m->rope_rows);
    }
    return 0;
}
// nano_hip_forward in two halves: _begin queues the step and the copies back on the model's stream and returns; _end waits
// and hands the results over.  Several models (replicas on several GPUs, host/nano_engine.c nano_context_replicate) run
// their steps concurrently between the two.
extern "C" int nano_hip_forward_begin(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                      uint32_t is_causal, int want_logits, int want_argmax) {
    int rc;
    if ((rc = check_batch(m, tokens, pos, batch, 0))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = kv_ensure_batch(m, pos, batch, 0, !is_causal))) return rc;
    if (tokens != m->fw_tokens.data()) { m->fw_tokens.assign(tokens, tokens + batch); m->fw_pos.assign(pos, pos + batch); }    // (what a re-issue needs)
    m->fw_causal = is_causal; m->fw_logits = want_logits; m->fw_argmax = want_argmax;
    uint32_t max_pos = 0;
    if ((rc = stage_batch(m, tokens, pos, batch, false, &max_pos))) return rc;
    const uint32_t mode = want_argmax ? MODE_ARGMAX : (want_logits ? MODE_LOGITS : MODE_NOCLS);
    if ((rc = run_step(m, batch, is_causal ? 1u : 0u, mode, max_pos))) return rc;
    const size_t V = m->d.vocab_size;
    if (want_logits) HIP_TRY(hipMemcpyAsync(m->h_logits, m->logits, batch * V * 4, hipMemcpyDeviceToHost, m->st));
    if (want_argmax) HIP_TRY(hipMemcpyAsync(m->h_amax, m->amax, batch * 4, hipMemcpyDeviceToHost, m->st));
    m->pending_batch = batch;
    return 0;
}

extern "C" int nano_hip_forward_end(NanoHipModel *m, float *logits_out, uint32_t *argmax_out) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    if (!m->pending_batch) return nano_hip_sync(m);                         // (no step queued: nothing to hand over, nothing to re-issue)
    const size_t V = m->d.vocab_size, batch = m->pending_batch;
    const int rc = with_reissue(m, [&](bool again) {                        // the first attempt is what nano_hip_forward_begin queued
        if (again) { const int rb = nano_hip_forward_begin(m, m->fw_tokens.data(), m->fw_pos.data(), (uint32_t)batch, m->fw_causal, m->fw_logits, m->fw_argmax); if (rb) return rb; }
        HIP_TRY(hipStreamSynchronize(m->st));
        return 0;
    });
    m->pending_batch = 0;
    if (rc) return rc;
    if (logits_out) memcpy(logits_out, m->h_logits, batch * V * 4);
    if (argmax_out) memcpy(argmax_out, m->h_amax, batch * 4);
    return 0;
}

extern "C" int nano_hip_forward(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                uint32_t is_causal, float *logits_out, uint32_t *argmax_out) {
    int rc;
    if ((rc = nano_hip_forward_begin(m, tokens, pos, batch, is_causal, logits_out != nullptr, argmax_out != nullptr))) return rc;
    return nano_hip_forward_end(m, logits_out, argmax_out);
}

// ---- LoRA: one attached module, or a table of modules with one bound to each KV slot (lora.hip) ------------------------
// `params` = the floats of a LoRA module file after its 256-byte header, in file order (reference infer.c:476-497):
// wq_a[L][r][E] wq_b[L][E][r] wk_a[L][r][E] wk_b[L][KD][r] wv_a[L][r][E] wv_b[L][KD][r] wo_a[L][r][E] wo_b[L][E][r].
static size_t lora_layout(size_t L, size_t E, size_t KD, size_t r, size_t off[8]) {
    const size_t len[8] = { L * r * E, L * E * r, L * r * E, L * KD * r, L * r * E, L * KD * r, L * r * E, L * E * r };
    size_t total = 0;
    for (int i = 0; i < 8; i++) { off[i] = total; total += len[i]; }
    return total;
}
extern "C" size_t nano_hip_lora_param_floats(uint32_t n_layer, uint32_t n_embd, uint32_t kv_dim, uint32_t rank) {
    size_t off[8];
    return lora_layout(n_layer, n_embd, kv_dim, rank, off);
}
// A module on the device: its buffer, and the o1 scratch and the descriptor array (rank 0 in every slot) where the model has none yet.
// every_slot: the module goes into every slot's descriptor (an attached module).  Everything is allocated and uploaded before the model
// changes: a failure leaves it as it was.  The stream is idle (queued steps read the descriptors).
static int lora_entry_make(NanoHipModel *m, uint32_t rank, uint32_t alpha, const float *params, bool every_slot, NanoHipModel::LoraTable::Entry *out) {
    size_t off[8];
    const size_t total = lora_layout(m->d.n_layer, m->d.n_embd, m->KD, rank, off);
    NanoHipModel::LoraTable::Entry en;
    float *o1 = m->lora_o1; LoraSlotDesc *desc = m->lt.desc;
    HIP_TRY(hipMalloc(&en.buf, total * 4));
    for (int i = 0; i < 8; i++) en.d.t[i] = en.buf + off[i];
    en.d.rank = rank; en.d.alpha = alpha;
    hipError_t e = hipMemcpy(en.buf, params, total * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !o1) e = hipMalloc(&o1, (size_t)m->Bs * m->d.n_embd * 4);
    if (e == hipSuccess && !desc) {
        e = hipMalloc(&desc, (size_t)m->maxB * sizeof(LoraSlotDesc));
        if (e == hipSuccess) e = hipMemset(desc, 0, (size_t)m->maxB * sizeof(LoraSlotDesc));      // rank 0: no slot has a module
    }
    if (e == hipSuccess && every_slot) {
        const std::vector<LoraSlotDesc> all(m->maxB, en.d);
        e = hipMemcpy(desc, all.data(), all.size() * sizeof(LoraSlotDesc), hipMemcpyHostToDevice);     // at most 64 x 72 bytes
    }
    if (e != hipSuccess) {
        (void)hipFree(en.buf); if (o1 != m->lora_o1) (void)hipFree(o1); if (desc != m->lt.desc) (void)hipFree(desc);
        HIP_TRY(e);
    }
    m->lora_o1 = o1; m->lt.desc = desc;
    *out = en;
    return 0;
}
extern "C" int nano_hip_lora_attach(NanoHipModel *m, uint32_t rank, uint32_t alpha, const float *params, size_t n_floats) {
    if (!m || !params || !rank) FAIL(NANO_HIP_EINVAL, "bad argument");
    if (m->d.arch != NANO_ARCH_NANO) FAIL(NANO_HIP_EINVAL, "LoRA side branches exist for the Nano architecture only (reference infer.c:792)");
    // (n_embd % 16 == 0 is the model's own check; rank is the caller's: a module whose t vectors do not fit the launches' LDS is refused here)
    if (const char *msg = lora_shape_error(m->d.n_embd, rank)) FAIL(NANO_HIP_EINVAL, "%s (n_embd %u, rank %u)", msg, m->d.n_embd, rank);
    if (m->lt.n) FAIL(NANO_HIP_EINVAL, "a LoRA table is stored (nano_hip_lora_table_set); the table and an attached module exclude each other");
    HIP_TRY(hipSetDevice(m->device));
    const size_t total = nano_hip_lora_param_floats(m->d.n_layer, m->d.n_embd, m->KD, rank);
    if (n_floats < total) FAIL(NANO_HIP_EINVAL, "LoRA parameter block too small: %zu floats, need %zu", n_floats, total);
    HIP_TRY(hipStreamSynchronize(m->st));
    NanoHipModel::LoraTable::Entry en;
    int rc; if ((rc = lora_entry_make(m, rank, alpha, params, true, &en))) return rc;
    drop_graphs(m);                                          // graphs captured with the previous module carry its rank as their LDS size
    if (m->lt.at.buf) (void)hipFree(m->lt.at.buf);
    m->lt.at = en; m->lt.max_rank = rank; m->lora_on = true;
    return 0;
}
// use_lora of the reference's forward (lora != NULL): switch the attached module on / off per call
extern "C" int nano_hip_lora_enable(NanoHipModel *m, int on) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (on && !m->lt.at.buf && !m->lt.n) FAIL(NANO_HIP_EINVAL, "no LoRA module attached and no LoRA table entry stored");
    if (m->lt.n && m->lora_on != (on != 0)) {              // the table switched: drop the graphs, as every change of the table does
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipStreamSynchronize(m->st));
        drop_graphs(m);
    }
    m->lora_on = on != 0;
    return 0;
}

static LoraSlotDesc lora_slot_desc(const NanoHipModel *m, uint32_t id) { return id == NANO_LORA_NONE ? LoraSlotDesc{} : m->lt.e[id].d; }
static bool lora_entry_bound(const NanoHipModel *m, uint32_t id) {
    for (const uint32_t b : m->lt.bound) if (b == id) return true;
    return false;
}
static void lora_table_summary(NanoHipModel *m) {
    m->lt.n = 0; m->lt.max_rank = 0;
    for (const auto &en : m->lt.e) if (en.buf) { m->lt.n++; if (en.d.rank > m->lt.max_rank) m->lt.max_rank = en.d.rank; }
}
extern "C" int nano_hip_lora_table_set(NanoHipModel *m, uint32_t id, uint32_t rank, uint32_t alpha, const float *params, size_t n_floats) {
    if (!m || !params) FAIL(NANO_HIP_EINVAL, "LoRA table: null argument");
    if (id >= NANO_LORA_TABLE_MAX) FAIL(NANO_HIP_EINVAL, "LoRA table: entry %u beyond the %u entries of the table", id, NANO_LORA_TABLE_MAX);
    if (m->d.arch != NANO_ARCH_NANO) FAIL(NANO_HIP_EINVAL, "LoRA side branches exist for the Nano architecture only (reference infer.c:792)");
    if (m->lt.at.buf) FAIL(NANO_HIP_EINVAL, "LoRA table: a module is attached (nano_hip_lora_attach); the table and an attached module exclude each other");
    if (const char *msg = lora_shape_error(m->d.n_embd, rank)) FAIL(NANO_HIP_EINVAL, "%s (n_embd %u, rank %u)", msg, m->d.n_embd, rank);
    const size_t total = nano_hip_lora_param_floats(m->d.n_layer, m->d.n_embd, m->KD, rank);
    if (n_floats < total) FAIL(NANO_HIP_EINVAL, "LoRA parameter block too small: %zu floats, need %zu", n_floats, total);
    if (!m->lt.e.empty() && m->lt.e[id].buf && lora_entry_bound(m, id)) FAIL(NANO_HIP_EINVAL, "LoRA table: entry %u is bound to a slot (bind the slot elsewhere first)", id);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    NanoHipModel::LoraTable::Entry en;
    int rc; if ((rc = lora_entry_make(m, rank, alpha, params, false, &en))) return rc;
    if (m->lt.e.empty()) { m->lt.e.resize(NANO_LORA_TABLE_MAX); m->lt.bound.assign(m->maxB, NANO_LORA_NONE); }
    drop_graphs(m);                                          // their LDS size (the largest rank) and their launch choice may have changed
    if (m->lt.e[id].buf) (void)hipFree(m->lt.e[id].buf);
    m->lt.e[id] = en;
    lora_table_summary(m);
    m->lora_on = true;
    return 0;
}
extern "C" int nano_hip_lora_table_clear(NanoHipModel *m, uint32_t id) {
    if (!m) FAIL(NANO_HIP_EINVAL, "LoRA table: null model");
    if (id >= NANO_LORA_TABLE_MAX) FAIL(NANO_HIP_EINVAL, "LoRA table: entry %u beyond the %u entries of the table", id, NANO_LORA_TABLE_MAX);
    if (m->lt.e.empty() || !m->lt.e[id].buf) FAIL(NANO_HIP_EINVAL, "LoRA table: entry %u is empty", id);
    if (lora_entry_bound(m, id)) FAIL(NANO_HIP_EINVAL, "LoRA table: entry %u is bound to a slot (bind the slot elsewhere first)", id);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    drop_graphs(m);
    (void)hipFree(m->lt.e[id].buf);
    m->lt.e[id] = NanoHipModel::LoraTable::Entry{};
    lora_table_summary(m);
    if (!m->lt.n) m->lora_on = false;                        // an empty table is no table: the model steps as one that never had a module
    return 0;
}
// Rebinding is a small upload into the descriptor array; captured launches read it when they replay, so no graph is dropped.
extern "C" int nano_hip_lora_bind(NanoHipModel *m, const uint32_t *slots, const uint32_t *ids, uint32_t n) {
    if (!m || !slots || !ids) FAIL(NANO_HIP_EINVAL, "LoRA bind: null argument");
    if (m->d.arch != NANO_ARCH_NANO) FAIL(NANO_HIP_EINVAL, "LoRA side branches exist for the Nano architecture only (reference infer.c:792)");
    if (m->lt.at.buf) FAIL(NANO_HIP_EINVAL, "LoRA bind: a module is attached (nano_hip_lora_attach); the table and an attached module exclude each other");
    std::vector<bool> listed(m->maxB, false);
    for (uint32_t i = 0; i < n; i++) {
        if (slots[i] >= m->maxB) FAIL(NANO_HIP_EINVAL, "LoRA bind: slot %u out of range (max_batch %u)", slots[i], m->maxB);
        if (listed[slots[i]]) FAIL(NANO_HIP_EINVAL, "LoRA bind: slot %u listed twice", slots[i]);
        listed[slots[i]] = true;
        if (ids[i] == NANO_LORA_NONE) continue;
        if (ids[i] >= NANO_LORA_TABLE_MAX) FAIL(NANO_HIP_EINVAL, "LoRA bind: entry %u beyond the %u entries of the table", ids[i], NANO_LORA_TABLE_MAX);
        if (m->lt.e.empty() || !m->lt.e[ids[i]].buf) FAIL(NANO_HIP_EINVAL, "LoRA bind: entry %u is empty", ids[i]);
    }
    if (m->lt.e.empty() || n == 0) return 0;                 // (no table yet: only NANO_LORA_NONE passed the checks, which every slot already is)
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));                    // queued steps read the descriptors
    std::vector<LoraSlotDesc> all(m->maxB);
    std::vector<uint32_t> bound = m->lt.bound;
    for (uint32_t i = 0; i < n; i++) bound[slots[i]] = ids[i];
    for (uint32_t s = 0; s < m->maxB; s++) all[s] = lora_slot_desc(m, bound[s]);
    HIP_TRY(hipMemcpy(m->lt.desc, all.data(), all.size() * sizeof(LoraSlotDesc), hipMemcpyHostToDevice));      // at most 64 x 72 bytes
    m->lt.bound = std::move(bound);
    return 0;
}
extern "C" int nano_hip_lora_binding(const NanoHipModel *m, uint32_t slot, uint32_t *id_out) {
    if (!m || !id_out) FAIL(NANO_HIP_EINVAL, "LoRA binding: null argument");
    if (slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "LoRA binding: slot %u out of range (max_batch %u)", slot, m->maxB);
    *id_out = m->lt.bound.empty() ? NANO_LORA_NONE : m->lt.bound[slot];
    return 0;
}
// One prefill chunk: nb rows of `slot`, their tokens and positions in m->tokens / m->pos, the last at last_pos.  replay: through a HIP graph per
// (KV slot, range bucket, nb, key_kind) -- positions and tokens are device data, the slot's cache addresses are baked into the nodes.  The chunk
// that meets a key first runs eagerly and is captured for the next one that reaches it; a failed capture only costs the replays (r.capture
// is not looked at).  The cache of chunk graphs is bounded (oldest out).  Chunks of different kinds have different nodes: the key carries
// RowWant::key_kind (step_key), so none ever replays another's graph.
hipError_t enqueue_chunk(NanoHipModel *m, uint32_t slot, uint32_t nb, const RowWant &want, uint32_t last_pos, bool replay) {
    // (the range hint of the chunk's last token's own decode step)
    const StepSpec s = StepSpec::chunk(slot, nb, want.mode_pass(), range_hint_of(m, 1, 1, last_pos), want.use_targets());
    const uint64_t key = replay ? step_key(m, s, want.key_kind()) : STEP_NO_KEY;
    m->nsplit = xba_nsplit(m, s);                                      // 1: a prefill chunk leaves xba final (single split or the combine kernel), replayed or not
    if (key == STEP_NO_KEY) return enqueue_step(m, s);                 // eager: one pass per chunk
    const GraphRun r = graph_step(m, key, [&, s] { return enqueue_step(m, s); });
    if (r.stored) {
        if (m->pf_graph_keys.size() >= PF_GRAPH_CAP) {
            auto old = m->graphs.find(m->pf_graph_keys.front());
            if (old != m->graphs.end()) { (void)hipGraphExecDestroy(old->second); m->graphs.erase(old); }
            m->pf_graph_keys.erase(m->pf_graph_keys.begin());
        }
        m->pf_graph_keys.push_back(key);
    }
    return r.step;
}
// Batched prefill: feeds `count` prompt tokens at positions pos0 .. pos0+count-1 of sequence `slot` in
// passes of up to 64 (Q80, Q4K and FP32 through their MFMA GEMMs: m->pf_chunk) / 8 tokens per weight read instead of one decode step per token; no
// logits (the reference computes and discards them for prompt positions, infer.c:1146-1149).  The KV rows and every
// later logit are the ones token-by-token feeding produces, bit for bit (same kernels and the same attention split per token).
// want (RowWant, backend_model.h) says what comes back per fed row; nothing else differs.
//   scores (nano_hip_prefill_score): every chunk goes on into the classifier for all its rows and the row statistics (enqueue_step MODE_SCORE);
//     scores_out[i] scores the logits of tokens[i] for targets[i] (no targets: for the row's own arg-max).  k >= 1 (nano_hip_prefill_score_topk):
//     the selection's two launches (topk.hip) are queued eagerly behind every scored chunk, so the chunk graphs and their keys are nano_hip_prefill_score's.
//   arg-maxes (nano_hip_verify_draft): every chunk goes on into the classifier and the arg-max of all its rows (MODE_VERIFY); argmax_out[i] is row i's.
// Strict and exact mode feed token by token through rows_run_ordered: the prompt is staged once and the host waits once per prompt in both
// (no wait per token: a token comes from the staged prompt by a device-to-device copy, not through stage_batch's pinned row; the phase hook waits itself).
int prefill_run(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count, const RowWant &want) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    if (const int rc = rows_check(m, want)) return rc;
    if (!tokens) FAIL(NANO_HIP_EINVAL, "null argument");
    if (slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "slot %u out of range (max_batch %u)", slot, m->maxB);
    if ((uint64_t)pos0 + count > m->S) FAIL(NANO_HIP_EINVAL, "positions %u..%u exceed max_seq_len %u", pos0, pos0 + count, m->S);
    if ((uint64_t)pos0 + count > m->rope_rows) FAIL(NANO_HIP_EINVAL, "positions %u..%u exceed the model's RoPE table (%u rows = block_size)", pos0, pos0 + count, m->rope_rows);
    for (uint32_t i = 0; i < count; i++) if (tokens[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "token %u out of vocabulary", tokens[i]);
    if (want.use_targets()) for (uint32_t i = 0; i < count; i++) if (want.targets[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "target %u out of vocabulary", want.targets[i]);
    if (want.kind == RowWant::SCORE && !count) return 0;
    HIP_TRY(hipSetDevice(m->device));
    if (count) { const int rc = step_served(m, true); if (rc) return rc; }     // (an empty prompt queues nothing: there is nothing to refuse)
    const bool ordered = strict_serves(m) || exact_serves(m);                 // one reference-order step per prompt token (exact mode: each a replay)
    if (const int rc = rows_begin(m, want, !ordered, C_FEED, count, want.targets)) return rc;
    if (m->kv.paged && count) {
        const uint32_t need = pos0 + count - 1;
        int rc = kv_ensure(m, &slot, &pos0, &need, 1);
        if (rc) return rc;
    }
    // the whole prompt's tokens and positions go to the device ONCE; a chunk takes its share by device-to-device copies on the stream, the host waits only at the end
    if (count) {
        std::vector<uint32_t> hp(count);
        for (uint32_t i = 0; i < count; i++) hp[i] = pos0 + i;
        if (const int rc = rows_feed(m, count, tokens, hp.data(), nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(m->st));                              // hp leaves scope; one wait per prompt
    }
    if (ordered) {
        if (const int rc = rows_run_ordered(m, want, count, slot, nullptr)) return rc;
        return rows_back(m, want, count, nullptr, true);
    }
    const uint32_t chunk_max = m->pf_chunk;
    for (uint32_t done = 0; done < count;) {
        uint32_t nb = (count - done < chunk_max) ? count - done : chunk_max;
        const uint32_t to_bucket_end = 64u - (pos0 + done) % 64u;          // one attention range bucket per chunk (see enqueue_step)
        if (nb > to_bucket_end) nb = to_bucket_end;
        HIP_TRY(hipMemcpyAsync(m->tokens, m->rb.tok + done, nb * 4, hipMemcpyDeviceToDevice, m->st));
        HIP_TRY(hipMemcpyAsync(m->pos, m->rb.pos + done, nb * 4, hipMemcpyDeviceToDevice, m->st));
        HIP_TRY(rows_pass_targets(m, want, done, nb));
        // a full 64-token chunk recurs in every long prompt: replayed.  Other chunk lengths run eagerly (a capture costs more than the ~300
        // launches it would save once).
        const bool replay = m->use_graph && nb == chunk_max && chunk_max == 64u;
        HIP_TRY(enqueue_chunk(m, slot, nb, want, pos0 + done + nb - 1, replay));
        HIP_TRY(rows_after_pass(m, want, done, nb));
        done += nb;
    }
    return rows_back(m, want, count, nullptr, true);
}
extern "C" int nano_hip_prefill(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count) {
    return prefill_run(m, slot, tokens, pos0, count, RowWant());
}
extern "C" int nano_hip_prefill_score(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                                      const uint32_t *targets, NanoHipTokenScore *out) {
    return prefill_run(m, slot, tokens, pos0, count, RowWant::scores(targets, 0, out, nullptr));
}
extern "C" int nano_hip_prefill_score_topk(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                                           const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    return prefill_run(m, slot, tokens, pos0, count, RowWant::scores(targets, k, scores_out, top_out));
}
extern "C" uint32_t nano_hip_prefill_chunk_tokens(const NanoHipModel *m) {
    if (!m) return 0u;
    return (strict_serves(m) || exact_serves(m)) ? 1u : m->pf_chunk;
}
// one pass of the greedy loop: queued, waited for, the ids handed over
static int decode_greedy_once(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, uint32_t steps, uint32_t *out_ids) {
    int rc;
    if ((rc = check_batch(m, tokens, pos, batch, steps))) return rc;
    if ((uint64_t)steps * batch > m->trace_cap) FAIL(NANO_HIP_EINVAL, "steps*batch exceeds trace capacity %u", m->trace_cap);
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = kv_ensure_batch(m, pos, batch, steps - 1, false))) return rc;          // every page the loop will enter, up front
    uint32_t max_pos = 0;
    if ((rc = stage_batch(m, tokens, pos, batch, true, &max_pos))) return rc;
    for (uint32_t s = 0; s < steps; s++) {
        // from the second step on the fast path's arg-max kernel of step s - 1 has embedded this step's token (misc.hip argmax_kernel): the
        // step then starts at layer 0's QKV launch (the reference-order step always embeds)
        if ((rc = run_step(m, batch, 1, MODE_LOOP, max_pos + s, s > 0))) return rc;
    }
    if (out_ids) HIP_TRY(hipMemcpyAsync(m->h_amax, m->trace, (size_t)steps * batch * 4, hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    if (out_ids) memcpy(out_ids, m->h_amax, (size_t)steps * batch * 4);
    return 0;
}
// A hand-off that gives up somewhere in the loop leaves every later step of it on garbage: the whole call again (with_reissue).
extern "C" int nano_hip_decode_greedy(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                      uint32_t steps, uint32_t *out_ids) {
    if (steps == 0) return 0;
    return with_reissue(m, [&](bool) { return decode_greedy_once(m, tokens, pos, batch, steps, out_ids); });
}
