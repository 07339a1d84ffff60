// backend_probe.hip -- measurement, state read-back, the hand-off switches and fault injection (tests; tools).
#include <array>
#include "backend_model.h"

// ---- the in-launch hand-offs: state, switches, fault injection (tests; tools) ----------------------------------------------------------
extern "C" int nano_hip_handoff_state(const NanoHipModel *m, uint32_t *fused_mask, uint32_t *fallbacks, uint32_t *last_code) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (fused_mask) *fused_mask = (m->ho.fuse_qkv_attn ? 1u : 0u) | (m->ho.fuse_wo_w13 ? 2u : 0u);
    if (fallbacks) *fallbacks = m->ho.fallbacks;
    if (last_code) *last_code = m->ho.last_dev_err;
    return 0;
}
extern "C" int nano_hip_set_fusion(NanoHipModel *m, uint32_t mask) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (mask & ~3u) FAIL(NANO_HIP_EINVAL, "unknown fusion bits 0x%x", mask);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    m->ho.fuse_qkv_attn = (mask & 1u) != 0; m->ho.fuse_wo_w13 = (mask & 2u) != 0;
    drop_graphs(m);                                                        // (graphs carry the launches of the setting they were captured under)
    return 0;
}
extern "C" int nano_hip_debug_fault(NanoHipModel *m, uint32_t flags) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (flags & ~3u) FAIL(NANO_HIP_EINVAL, "unknown fault bits 0x%x", flags);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    const uint32_t words[2] = { (flags & 1u) ? 0x5a5au : 0u, 0u };          // tick[1]: XORed into every producer's tag; tick[2]: the abort flag, cleared
    HIP_TRY(hipMemcpy(m->ho.tick + 1, words, 8, hipMemcpyHostToDevice));
    m->ho.reissue = (flags & 2u) == 0;
    return 0;
}

// ---- measurement ----
static uint64_t classifier_bytes(const NanoHipModel *m) { return weight_bytes(m->d.quant_type, m->d.group_size, (uint64_t)m->d.vocab_size * m->d.n_embd); }

extern "C" int nano_hip_time_classifier(NanoHipModel *m, uint32_t batch, uint32_t iters, float *ms_per_launch, uint64_t *bytes_per_launch) {
    if (!m || !iters || batch == 0 || batch > m->maxB || batch > NANO_MAX_BATCH) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(enqueue_classifier(m, batch));                               // warm
    HIP_TRY(hipEventRecord(m->ev0, m->st));
    for (uint32_t i = 0; i < iters; i++) HIP_TRY(enqueue_classifier(m, batch));
    HIP_TRY(hipEventRecord(m->ev1, m->st));
    HIP_TRY(hipEventSynchronize(m->ev1));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
    if (ms_per_launch) *ms_per_launch = ms / iters;
    if (bytes_per_launch) *bytes_per_launch = classifier_bytes(m);
    return 0;
}
// the batch the step probes time: `batch` sequences, each token 1 at position pos (their pages taken, tokens and positions queued)
static int stage_probe_batch(NanoHipModel *m, uint32_t batch, uint32_t pos) {
    for (uint32_t i = 0; i < batch; i++) { m->h_tokens[i] = 1 % m->d.vocab_size; m->h_pos[i] = pos; }
    const int rc = kv_ensure_batch(m, m->h_pos, batch, 0, false);
    return rc ? rc : stage_batch(m, m->h_tokens, m->h_pos, batch, false);
}
// The classifier launch timed INSIDE whole decode steps (its weights are cold: the layers' 468 MB went through the
// caches since the previous step), HIP events on the model's stream, eager launches.  *ms_per_launch is the raw
// event span (end of the previous kernel -> end of the classifier); *ms_empty_pair the span of an empty event pair.
extern "C" int nano_hip_time_classifier_in_step(NanoHipModel *m, uint32_t batch, uint32_t pos, uint32_t iters, float *ms_per_launch,
                                                uint64_t *bytes_per_launch, float *ms_empty_pair) {
    if (!m || !iters || batch == 0 || batch > m->maxB || batch > NANO_MAX_BATCH || pos >= m->S) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(m->device));
    { const int rc = stage_probe_batch(m, batch, pos); if (rc) return rc; }
    StepSpec s = StepSpec::seqs(batch, 1, MODE_ARGMAX, range_hint_of(m, 1, 1, pos));      // (this probe has always timed the step of the 64-position hint, whatever the batch)
    s.probe_cls = true;
    m->nsplit = xba_nsplit(m, s);
    double cls = 0.0, empty = 0.0;
    for (uint32_t i = 0; i < iters + 1; i++) {
        HIP_TRY(enqueue_step(m, s));
        HIP_TRY(hipEventSynchronize(m->ev2));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, m->ev0, m->ev1));
        HIP_TRY(hipEventElapsedTime(&b, m->ev1, m->ev2));
        if (i) { cls += a; empty += m->probe_ext ? 0.0f : b; }   // iteration 0 warms up; exact kernel timestamps carry no event overhead
    }
    HIP_TRY(hipStreamSynchronize(m->st));
    if (ms_per_launch) *ms_per_launch = (float)(cls / iters);          // raw span: includes the launch latency
    if (ms_empty_pair) *ms_empty_pair = (float)(empty / iters);
    if (bytes_per_launch) *bytes_per_launch = classifier_bytes(m);
    return 0;
}

extern "C" int nano_hip_time_step(NanoHipModel *m, uint32_t batch, uint32_t pos, uint32_t iters, float *ms_per_step) {
    if (!m || !iters || batch == 0 || batch > m->maxB || batch > NANO_MAX_BATCH || pos >= m->S) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(m->device));
    int rc;
    if ((rc = stage_probe_batch(m, batch, pos))) return rc;
    if ((rc = run_step(m, batch, 1, MODE_ARGMAX, pos))) return rc;       // warm / capture
    HIP_TRY(hipEventRecord(m->ev0, m->st));
    for (uint32_t i = 0; i < iters; i++) if ((rc = run_step(m, batch, 1, MODE_ARGMAX, pos))) return rc;
    HIP_TRY(hipEventRecord(m->ev1, m->st));
    HIP_TRY(hipEventSynchronize(m->ev1));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
    if (ms_per_step) *ms_per_step = ms / iters;
    return dev_err_check(m);                                             // (a step whose kernels gave up is no measurement)
}

extern "C" int nano_hip_membw(int device, size_t bytes, uint32_t iters, float *gbps) {
    if (!iters || bytes < (1u << 20)) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    void *buf = nullptr; float *sink = nullptr;
    HIP_TRY(hipMalloc(&buf, bytes));
    HIP_TRY(hipMalloc(&sink, 4));
    HIP_TRY(hipMemset(buf, 1, bytes));
    hipEvent_t e0, e1; HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(launch_stream_read(buf, bytes, sink, 0));
    HIP_TRY(hipEventRecord(e0, 0));
    for (uint32_t i = 0; i < iters; i++) HIP_TRY(launch_stream_read(buf, bytes, sink, 0));
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (gbps) *gbps = (float)((double)bytes * iters / (ms * 1e-3) / 1e9);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(buf); (void)hipFree(sink);
    return 0;
}
// Competing load for the hand-off tests: `iters` launches of a streaming reader of `bytes` on a stream of its own, on the workgroup slots of
// the XCDs in `xcd_mask` only (uneven load), `wgs` workgroups of 256 threads each launch.  Blocks until they are done: call it from a thread
// of its own while the model under test decodes.
extern "C" int nano_hip_background_load(int device, size_t bytes, uint32_t iters, uint32_t xcd_mask, uint32_t wgs) {
    if (!iters || bytes < (1u << 20) || !wgs || wgs > 65535u) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    void *buf = nullptr; float *sink = nullptr; hipStream_t st = nullptr;
    HIP_TRY(hipMalloc(&buf, bytes));
    HIP_TRY(hipMalloc(&sink, 4));
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipMemsetAsync(buf, 1, bytes, st));
    hipError_t e = hipSuccess;
    for (uint32_t i = 0; i < iters && e == hipSuccess; i++) e = launch_stream_read_masked(buf, bytes, sink, xcd_mask, wgs, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st); (void)hipFree(buf); (void)hipFree(sink);
    HIP_TRY(e); HIP_TRY(e2);
    return 0;
}

extern "C" int nano_hip_read_state(NanoHipModel *m, uint32_t slot, int which, uint32_t layer, uint32_t pos, float *out, size_t n) {
    if (!m || !out || slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    const float *src = nullptr; size_t cap = 0;
    const KvRows kv{ m, slot, true };
    if (which == 5 || which == 6) {                              // a cache row, FP32 or (widened on the way back) FP16 / FP8
        if (layer >= m->d.n_layer || pos >= m->S) FAIL(NANO_HIP_EINVAL, "bad layer/pos");
        if (n > m->KD) FAIL(NANO_HIP_EINVAL, "n too large");
        size_t row = 0;
        if (!kv.row(layer, pos, &row)) { memset(out, 0, n * 4); return 0; }     // paged, no page yet: a never-written (zero) row
        const float *rp = kv.at(which == 5 ? m->kcache : m->vcache, row);
        if (!m->kv_half) { HIP_TRY(hipMemcpy(out, rp, n * 4, hipMemcpyDeviceToHost)); return 0; }
        if (m->kv_half == KV_FMT_FP8) {                          // e4m3fn bytes (scale 1): widened through the 256 values of the format
            static const std::array<float, 256> e4m3 = [] {
                std::array<float, 256> t{};
                for (uint32_t c = 0; c < 256; c++) {
                    const uint32_t ex = (c >> 3) & 15u, mt = c & 7u;
                    const float mag = (ex == 15u && mt == 7u) ? NAN : ex ? ldexpf((float)(8u + mt), (int)ex - 10) : ldexpf((float)mt, -9);
                    t[c] = (c & 0x80u) ? -mag : mag;
                }
                return t;
            }();
            std::vector<uint8_t> b8(n);
            HIP_TRY(hipMemcpy(b8.data(), rp, n, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) out[i] = e4m3[b8[i]];
            return 0;
        }
        std::vector<__half> tmp(n);
        HIP_TRY(hipMemcpy(tmp.data(), rp, n * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) out[i] = __half2float(tmp[i]);
        return 0;
    }
    switch (which) {
    case 0: src = m->x + (size_t)slot * m->d.n_embd; cap = m->d.n_embd; break;
    case 1: src = m->q + (size_t)slot * m->QD; cap = m->QD; break;
    case 2:   // attention output: final when the last step ran unsplit, else combine the split partials on demand
        if (m->nsplit > 1) HIP_TRY(launch_attn_combine(m->attn_part + (size_t)slot * m->nsplit * m->QD, m->attn_ml + (size_t)slot * m->d.n_head * m->nsplit * 2,
                                    m->xba + (size_t)slot * m->QD, m->d.n_head, m->hd, m->nsplit, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        src = m->xba + (size_t)slot * m->QD; cap = m->QD; break;
    case 3: src = m->hb + (size_t)slot * m->d.n_hidden; cap = m->d.n_hidden; break;
    case 4: src = m->logits + (size_t)slot * m->d.vocab_size; cap = m->d.vocab_size; break;
    default: FAIL(NANO_HIP_EINVAL, "unknown state id %d", which);
    }
    if (n > cap) FAIL(NANO_HIP_EINVAL, "n too large");
    HIP_TRY(hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- phase stamps (measurement builds: make -C nano_amd/csrc stamps; in the product build the kernels ignore the buffer) ----
extern "C" int nano_hip_stamps_begin(NanoHipModel *m) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    const size_t bytes = (size_t)STAMP_MAX_LAUNCHES * STAMP_WGS * 8 * sizeof(unsigned long long);
    if (!m->stamp.buf) HIP_TRY(hipMalloc(&m->stamp.buf, bytes));
    HIP_TRY(hipStreamSynchronize(m->st));
    HIP_TRY(hipMemset(m->stamp.buf, 0, bytes));
    m->stamp.launches = 0; m->stamp.kinds.clear(); m->stamp.on = true;
    return 0;
}
extern "C" int nano_hip_stamps_read(NanoHipModel *m, unsigned long long *out, uint32_t *kinds, uint32_t cap_launches, uint32_t *n_launches) {
    if (!m || !out || !kinds || !n_launches) FAIL(NANO_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));
    m->stamp.on = false;
    const uint32_t n = m->stamp.launches < cap_launches ? m->stamp.launches : cap_launches;
    if (n) HIP_TRY(hipMemcpy(out, m->stamp.buf, (size_t)n * STAMP_WGS * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) kinds[i] = m->stamp.kinds[i];
    *n_launches = n;
    return 0;
}
