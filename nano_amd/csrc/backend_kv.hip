// backend_kv.hip -- the KV cache as the host sees it: where its rows are, the paged cache (pages on demand, copy-on-write, release),
// a prefix shared between slots (fork), a slot's rows in host memory and back (KV images: save / restore).
#include "backend_model.h"

// ---- where the KV cache's rows are (KvRows, backend_model.h) ----------------------------------------------------------------------------
KvRows::VTarget KvRows::v_target(uint32_t l) const {
    if (m->kv_half) return { m->vraw, m->KD, 0u, m->pos };                                     // FP16 / FP8 cache: the attention kernel rounds and stores the row
    if (m->kv.paged) return { m->vcache + l * plane_elems(), 0u, m->KD, m->kv.kvrow };            // paged: row kvrow[b] of this layer's plane (the one position-indexed output)
    // a ragged pass on the contiguous FP32 cache goes the FP16 cache's way: 64 slots of a 4B model are more v plane than a 32-bit offset
    // reaches, and not every projection epilogue multiplies in 64 bits; the attention kernel's prep pass copies the row (same bits)
    if (ragged) return { m->rows.vraw, m->KD, 0u, m->pos };
    return { v_flat(l), v_flat_bstride(), m->KD, m->pos };
}
// (batched prefill on the contiguous cache: the slot's own rows, no stride; on the paged cache the table row is the slot's and these stay)
void KvRows::attention(AttnArgs &a) const {
    const bool own = one_slot && !m->kv.paged;
    a.kcache = own ? at(m->kcache, (size_t)slot * slot_elems()) : m->kcache;
    a.vcache = own ? at(m->vcache, (size_t)slot * slot_elems()) : m->vcache;
    a.cache_bstride_rows = own ? 0u : m->d.n_layer * m->S;
}
bool KvRows::row(uint32_t layer, uint32_t pos, size_t *elems) const {
    if (!m->kv.paged) { *elems = (size_t)slot * slot_elems() + layer * layer_elems() + (size_t)pos * m->KD; return true; }
    const uint32_t rb = m->kv.h_pt[(size_t)slot * m->kv.pt_stride + (pos >> 6)];
    if (rb == KV_NO_PAGE) return false;
    *elems = layer * plane_elems() + (size_t)(rb + (pos & 63u)) * m->KD;
    return true;
}

// ---- row copies between slots / pages (kv_copy.hip) ---------------------------------------------------------------------------
// Queues ONE copy launch for `jobs` on the model's stream.  gstart cuts the list into groups that share a source (kernels.h KvCopyArgs);
// plane_rows = cache rows of one layer plane in the layout the rows are counted in (contiguous: max_seq_len, with slot s starting at row
// s * L * S of "plane 0"; paged: pages * 64).  The list goes to the device from a staging copy of its own, like the page-table rows.
static hipError_t kv_copy_enqueue(NanoHipModel *m, const std::vector<KvCopyJob> &jobs, const std::vector<uint32_t> &gstart, size_t plane_rows) {
    if (jobs.empty()) return hipSuccess;
    const size_t head = (gstart.size() + 3) & ~(size_t)3, words = head + jobs.size() * 4;       // jobs start 16-byte aligned
    if (words > m->kv.jobs_cap) {
        hipError_t e = hipStreamSynchronize(m->st);                        // (a queued launch may still read the old list)
        if (e != hipSuccess) return e;
        if (m->kv.jobs) { (void)hipFree(m->kv.jobs); m->kv.jobs = nullptr; m->kv.jobs_cap = 0; }
        const size_t cap = words < 1024 ? 1024 : 2 * words;
        if ((e = hipMalloc(reinterpret_cast<void **>(&m->kv.jobs), cap * 4)) != hipSuccess) return e;
        m->kv.jobs_cap = cap;
    }
    m->kv.pt_stage.emplace_back(words, 0u);
    std::vector<uint32_t> &stage = m->kv.pt_stage.back();
    memcpy(stage.data(), gstart.data(), gstart.size() * 4);
    memcpy(stage.data() + head, jobs.data(), jobs.size() * sizeof(KvCopyJob));
    hipError_t e = hipMemcpyAsync(m->kv.jobs, stage.data(), words * 4, hipMemcpyHostToDevice, m->st);
    if (e != hipSuccess) return e;
    uint32_t max_rows = 0;
    for (const KvCopyJob &j : jobs) if (j.rows > max_rows) max_rows = j.rows;
    KvCopyArgs a{};
    a.k = m->kcache; a.v = m->vcache;
    a.row_bytes = (uint32_t)(m->KD * kv_esz(m)); a.plane_bytes = (uint64_t)plane_rows * a.row_bytes;
    a.n_groups = (uint32_t)gstart.size() - 1;
    a.gstart = m->kv.jobs; a.jobs = reinterpret_cast<const KvCopyJob *>(m->kv.jobs + head);
    return launch_kv_copy(a, m->d.n_layer, max_rows, (uint32_t)m->cus, m->kv.copy_nt, m->st);
}
// staging rows of copies long done: drop them behind a sync
static int kv_stage_trim(NanoHipModel *m) {
    if (m->kv.pt_stage.size() > 256) {
        HIP_TRY(hipStreamSynchronize(m->st));
        m->kv.pt_stage.clear();
    }
    return 0;
}

// ---- changes of the paged cache (and the copies of a contiguous fork): planned, queued, and committed only when everything was queued ----
// A failing memset, copy or upload leaves the host table, the owner counts and the free list as they were (round-3 advice: pages leaked /
// host and device tables diverged).  Each changed table row goes to the device from a staging copy of its own: a later change may
// rewrite the pinned mirror before an earlier queued upload has run.
namespace {
struct KvPlan {
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> rows;          // (slot, its new table row)
    std::vector<uint32_t> zero;                                            // pages to zero-fill in every layer plane (the reference callocs its cache, infer.c:33,47)
    std::vector<KvCopyJob> jobs; std::vector<uint32_t> gstart{0u};         // row copies, cut into groups that share a source (kv_copy_enqueue)
    std::vector<std::pair<uint32_t, int32_t>> owners;                      // (page, change of its owner count)
    std::vector<uint32_t> free_pages;                                      // the free list once the pages drawn are gone and the pages given up are back
    uint64_t cow = 0;                                                      // copy-on-write copies among the jobs
};
}  // namespace
static int kv_apply(NanoHipModel *m, KvPlan &p, const char *what) {
    const size_t page_bytes = (size_t)64 * m->KD * kv_esz(m), plane_bytes = (size_t)m->kv.pages * page_bytes;
    hipError_t err = hipSuccess;
    for (const uint32_t page : p.zero) {
        if (err == hipSuccess) err = hipMemset2DAsync(reinterpret_cast<uint8_t *>(m->kcache) + (size_t)page * page_bytes, plane_bytes, 0, page_bytes, m->d.n_layer, m->st);
        if (err == hipSuccess) err = hipMemset2DAsync(reinterpret_cast<uint8_t *>(m->vcache) + (size_t)page * page_bytes, plane_bytes, 0, page_bytes, m->d.n_layer, m->st);
    }
    if (p.gstart.back() != p.jobs.size()) p.gstart.push_back((uint32_t)p.jobs.size());
    if (err == hipSuccess) err = kv_copy_enqueue(m, p.jobs, p.gstart, m->kv.paged ? (size_t)m->kv.pages * 64 : m->S);
    for (size_t i = 0; i < p.rows.size() && err == hipSuccess; i++) {
        m->kv.pt_stage.push_back(p.rows[i].second);
        err = hipMemcpyAsync(m->kv.pt + (size_t)p.rows[i].first * m->kv.pt_stride, m->kv.pt_stage.back().data(), (size_t)m->kv.pt_stride * 4, hipMemcpyHostToDevice, m->st);
    }
    if (err != hipSuccess) FAIL(NANO_HIP_ERUNTIME, "KV cache: queueing %s failed: %s (nothing committed)", what, hipGetErrorString(err));
    for (const auto &r : p.rows) memcpy(m->kv.h_pt + (size_t)r.first * m->kv.pt_stride, r.second.data(), (size_t)m->kv.pt_stride * 4);
    for (const auto &o : p.owners) m->kv.page_owners[o.first] += o.second;
    m->kv.cow_copies += p.cow;
    if (m->kv.paged) m->kv.free_pages.swap(p.free_pages);
    return kv_stage_trim(m);
}

// ---- paged KV cache: pages for the positions a call is about to touch ------------------------------------------------------
// first[i] / need[i] = first position slot slots[i] WRITES in the call / last position it will hold after it.  All or nothing: when the
// pool cannot cover every block the call fails before taking a page.  A block without a page gets one, zero-filled in every layer plane.
// A block the call writes into whose page has other owners as well (nano_hip_kv_fork) gets a page of this slot's own with the 64 rows
// copied in all planes -- copy-on-write, one launch for all such blocks of the call -- and the old page loses an owner; when several
// owners write in one call the last one keeps the page.  The slots' table rows go to the device behind everything queued so far.
int kv_ensure(NanoHipModel *m, const uint32_t *slots, const uint32_t *first, const uint32_t *need, uint32_t n) {
    if (!m->kv.paged) return 0;
    struct Take { uint32_t slot, blk, from; };                             // from: the shared page the new one is a copy of, or KV_NO_PAGE (zero-filled)
    std::vector<Take> takes;
    auto has = [&](uint32_t slot, uint32_t blk) { for (const Take &t : takes) if (t.slot == slot && t.blk == blk) return true; return false; };
    auto owners_left = [&](uint32_t page) { uint32_t c = m->kv.page_owners[page]; for (const Take &t : takes) if (t.from == page) c--; return c; };
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t blk = 0; blk <= need[i] >> 6 && blk < m->kv.pt_stride; blk++) {
            const uint32_t e = m->kv.h_pt[(size_t)slots[i] * m->kv.pt_stride + blk];
            if (has(slots[i], blk)) continue;                              // (the same slot twice in one call: its block once)
            if (e == KV_NO_PAGE) takes.push_back(Take{slots[i], blk, KV_NO_PAGE});
            else if (blk >= first[i] >> 6 && owners_left(e / 64u) > 1) takes.push_back(Take{slots[i], blk, e / 64u});
        }
    if (takes.empty()) return 0;
    if (takes.size() > m->kv.free_pages.size()) {
        size_t ncow = 0;
        for (const Take &t : takes) ncow += t.from != KV_NO_PAGE;
        FAIL(NANO_HIP_ENOMEM, "paged KV cache: %zu more pages needed (%zu of them copies of shared pages the call writes into), %zu free of %u (nano_hip_kv_release() returns a finished sequence's pages)",
             takes.size(), ncow, m->kv.free_pages.size(), m->kv.pages);
    }
    KvPlan p;
    p.free_pages = m->kv.free_pages;
    for (const Take &t : takes) {
        const uint32_t page = p.free_pages.back(); p.free_pages.pop_back();
        p.owners.emplace_back(page, 1);
        if (t.from == KV_NO_PAGE) p.zero.push_back(page);
        else { p.jobs.push_back(KvCopyJob{t.from * 64u, page * 64u, 64u, 64u}); p.gstart.push_back((uint32_t)p.jobs.size()); p.owners.emplace_back(t.from, -1); p.cow++; }
        auto row = p.rows.begin();
        while (row != p.rows.end() && row->first != t.slot) ++row;
        if (row == p.rows.end()) row = p.rows.emplace(row, t.slot, std::vector<uint32_t>(m->kv.h_pt + (size_t)t.slot * m->kv.pt_stride, m->kv.h_pt + (size_t)(t.slot + 1) * m->kv.pt_stride));
        row->second[t.blk] = page * 64u;
    }
    return kv_apply(m, p, "the pages of a step");
}
// sequences 0..batch-1 of a step live in slots 0..batch-1; each writes positions pos[i] .. pos[i] + extra and needs its pages up to there
// (whole_context: a non-causal step reads every row of the context, so every block is mapped; it still writes position pos[i] only)
int kv_ensure_batch(NanoHipModel *m, const uint32_t *pos, uint32_t batch, uint32_t extra, bool whole_context) {
    if (!m->kv.paged) return 0;
    uint32_t slots[NANO_MAX_BATCH], need[NANO_MAX_BATCH];
    for (uint32_t i = 0; i < batch; i++) { slots[i] = i; need[i] = whole_context ? m->S - 1 : pos[i] + extra; if (need[i] > m->S - 1) need[i] = m->S - 1; }
    return kv_ensure(m, slots, pos, need, batch);
}

// ---- paged KV cache: slot life cycle ----------------------------------------------------------------------------------------
extern "C" int nano_hip_kv_release(NanoHipModel *m, uint32_t slot) {
    if (!m || !m->kv.paged) FAIL(NANO_HIP_EINVAL, "not a paged-KV model");
    if (slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "slot %u out of range (max_batch %u)", slot, m->maxB);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->st));                                 // nothing queued may still read the pages
    uint32_t *row = m->kv.h_pt + (size_t)slot * m->kv.pt_stride;
    for (uint32_t blk = 0; blk < m->kv.pt_stride; blk++)
        if (row[blk] != KV_NO_PAGE) {                                    // a page goes back to the pool when its last owner leaves
            const uint32_t page = row[blk] / 64u;
            if (--m->kv.page_owners[page] == 0) m->kv.free_pages.push_back(page);
            row[blk] = KV_NO_PAGE;
        }
    HIP_TRY(hipMemcpyAsync(m->kv.pt + (size_t)slot * m->kv.pt_stride, row, (size_t)m->kv.pt_stride * 4, hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return 0;
}
extern "C" int nano_hip_kv_pages(const NanoHipModel *m, uint32_t *in_use, uint32_t *total) {
    if (!m || !m->kv.paged) FAIL(NANO_HIP_EINVAL, "not a paged-KV model");
    if (in_use) *in_use = m->kv.pages - (uint32_t)m->kv.free_pages.size();
    if (total) *total = m->kv.pages;
    return 0;
}
extern "C" int nano_hip_kv_sharing(const NanoHipModel *m, uint32_t *shared_pages, uint64_t *cow_copies) {
    if (!m || !m->kv.paged) FAIL(NANO_HIP_EINVAL, "not a paged-KV model");
    if (shared_pages) {
        uint32_t n = 0;
        for (uint32_t c : m->kv.page_owners) n += c > 1;
        *shared_pages = n;
    }
    if (cow_copies) *cow_copies = m->kv.cow_copies;
    return 0;
}

// ---- a prefix shared between slots ---------------------------------------------------------------------------------------------
// Contiguous cache: one copy launch, rows [0, n_pos) of the source slot to every destination in all 2 L planes (the source is read once).
// Paged cache: the destinations give back what they hold, take the source's FULL pages below n_pos as co-owners (no byte moves) and get
// a page of their own for a partial last block: its first n_pos % 64 rows copied, the rest zero (a fresh page is zero-filled, and
// non-causal attention reads unwritten rows).  Everything is planned first and committed after the queueing succeeded: a call that
// fails (arguments, pool) leaves tables, owner counts and the destinations' contents as they were.  The pages a fork can draw on are
// the free ones plus those only its destinations own.
// The rows a fork copies carry the deltas of the source slot's LoRA module: with a table, the destinations take its binding too.
static int fork_bindings(NanoHipModel *m, int rc, uint32_t src_slot, const uint32_t *dst_slots, uint32_t n_dst) {
    if (rc || m->lt.bound.empty()) return rc;
    const std::vector<uint32_t> ids(n_dst, m->lt.bound[src_slot]);
    return nano_hip_lora_bind(m, dst_slots, ids.data(), n_dst);
}
extern "C" int nano_hip_kv_fork(NanoHipModel *m, uint32_t src_slot, uint32_t n_pos, const uint32_t *dst_slots, uint32_t n_dst) {
    if (!m || !dst_slots) FAIL(NANO_HIP_EINVAL, "null argument");
    if (src_slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "source slot %u out of range (max_batch %u)", src_slot, m->maxB);
    if (n_pos > m->S) FAIL(NANO_HIP_EINVAL, "%u positions exceed max_seq_len %u", n_pos, m->S);
    {
        std::vector<bool> listed(m->maxB, false);
        for (uint32_t i = 0; i < n_dst; i++) {
            const uint32_t d = dst_slots[i];
            if (d >= m->maxB) FAIL(NANO_HIP_EINVAL, "destination slot %u out of range (max_batch %u)", d, m->maxB);
            if (d == src_slot) FAIL(NANO_HIP_EINVAL, "slot %u is the source and a destination", d);
            if (listed[d]) FAIL(NANO_HIP_EINVAL, "destination slot %u listed twice", d);
            listed[d] = true;
        }
    }
    HIP_TRY(hipSetDevice(m->device));
    if (n_dst == 0) return 0;
    KvPlan p;
    if (!m->kv.paged) {
        if (n_pos == 0) return 0;
        const uint32_t slot_rows = m->d.n_layer * m->S;                    // rows of one slot: [slot][layer][S][kv_dim]
        if ((uint64_t)m->maxB * slot_rows > 0xffffffffull) FAIL(NANO_HIP_EINVAL, "cache of %u slots x %u rows is beyond the copy kernel's 32-bit row index", m->maxB, slot_rows);
        for (uint32_t i = 0; i < n_dst; i++) p.jobs.push_back(KvCopyJob{src_slot * slot_rows, dst_slots[i] * slot_rows, n_pos, n_pos});
        return fork_bindings(m, kv_apply(m, p, "the fork"), src_slot, dst_slots, n_dst);
    }
    const uint32_t P = m->kv.pt_stride, nfull = n_pos >> 6, part = n_pos & 63u;
    const uint32_t *srow = m->kv.h_pt + (size_t)src_slot * P;
    const bool copy_part = part && srow[nfull] != KV_NO_PAGE;              // (part != 0 implies nfull < P: n_pos <= max_seq_len)
    // what the destinations' own release returns: pages that lose their last owner, in release order
    std::map<uint32_t, uint32_t> leaving;
    p.free_pages = m->kv.free_pages;
    for (uint32_t i = 0; i < n_dst; i++)
        for (uint32_t blk = 0; blk < P; blk++) {
            const uint32_t e = m->kv.h_pt[(size_t)dst_slots[i] * P + blk];
            if (e != KV_NO_PAGE && ++leaving[e / 64u] == m->kv.page_owners[e / 64u]) p.free_pages.push_back(e / 64u);
        }
    const size_t wanted = copy_part ? n_dst : 0;
    if (wanted > p.free_pages.size())
        FAIL(NANO_HIP_ENOMEM, "paged KV cache: a fork of %u positions into %u slots needs %zu pages for the partial block, %zu available (%zu free + the destinations' own) of %u",
             n_pos, n_dst, wanted, p.free_pages.size(), m->kv.free_pages.size(), m->kv.pages);
    for (const auto &lv : leaving) p.owners.emplace_back(lv.first, -(int32_t)lv.second);
    for (uint32_t i = 0; i < n_dst; i++) {
        std::vector<uint32_t> row(P, KV_NO_PAGE);
        for (uint32_t blk = 0; blk < nfull && blk < P; blk++) row[blk] = srow[blk];
        if (copy_part) {
            const uint32_t page = p.free_pages.back(); p.free_pages.pop_back();
            row[nfull] = page * 64u;
            p.jobs.push_back(KvCopyJob{srow[nfull], page * 64u, 64u, part});
        }
        for (const uint32_t e : row) if (e != KV_NO_PAGE) p.owners.emplace_back(e / 64u, 1);
        p.rows.emplace_back(dst_slots[i], std::move(row));
    }
    return fork_bindings(m, kv_apply(m, p, "the fork"), src_slot, dst_slots, n_dst);
}

// ---- KV images: a slot's rows in host memory and back (kv_image.h the layout, kv_image.hip the kernel) ---------------------------
// Host-only queries: no device call, no model state.
extern "C" int nano_hip_kv_image_plan(uint32_t n_layer, uint32_t kv_dim, uint32_t elem_bytes, uint32_t n_pos, uint64_t *out) {
    KvImagePlan p;
    if (!out) FAIL(NANO_HIP_EINVAL, "null argument");
    if (!kvi_plan(n_layer, kv_dim, elem_bytes, n_pos, &p)) FAIL(NANO_HIP_EINVAL, "KV image plan: %u layers, kv_dim %u, %u-byte elements describe no cache (elements of 4, 2 or 1 bytes; kv_dim a multiple of 4)", n_layer, kv_dim, elem_bytes);
    const uint64_t w[NANO_KV_IMAGE_PLAN_WORDS] = { KVI_HEADER_BYTES, p.payload_bytes, p.total_bytes, p.blocks, p.last_rows, p.block_stride, p.vec_bytes, 0 };
    memcpy(out, w, sizeof w);
    return 0;
}
extern "C" size_t nano_hip_kv_image_bytes(const NanoHipModel *m, uint32_t n_pos) {
    KvImagePlan p;
    return m && kvi_plan(m->d.n_layer, m->KD, (uint32_t)kv_esz(m), n_pos, &p) ? (size_t)p.total_bytes : 0;
}
extern "C" int nano_hip_kv_image_check(const void *image, size_t bytes, NanoKvImageHeader *out_header) {
    char msg[320];
    if (kvi_check(image, bytes, out_header, msg, sizeof msg)) FAIL(NANO_HIP_EINVAL, "%s", msg);
    return 0;
}

// The transport.  A chunk is a whole number of 64-position blocks in image order; the device staging buffer and the pinned host buffer
// each hold two, so the pack of one chunk (the model's stream) runs beside the copy of the previous one (kvi.cp) and the host's memcpy
// of the one before, and unpack the same way round.  Chunk size, measured with tools/kv_park_probe.py on Qwen3-0.6B at 4095 positions
// (profiles/kv_park.txt; NANO_KV_IMAGE_CHUNK_MB overrides the constant for such a run), save | restore, medians of 5:
//   FP32 rows (939 MB; a block is 14.7 MB):  4 MiB 46.3 | 30.0 ms   16 MiB 46.0 | 30.5   64 MiB 46.5 | 33.9   256 MiB 49.7 | 33.5
//   FP8 rows  (235 MB; a block is 3.7 MB):   4 MiB 12.5 |  9.1 ms   16 MiB 12.5 |  8.8   64 MiB 13.2 |  8.7   256 MiB 15.9 | 12.2
// 4 .. 64 MiB are inside each other's spread, 256 MiB is slower (fewer chunks, less overlap): 16 MiB, the smallest staging memory among
// the sizes that were not slower.  A chunk is never less than one block.
constexpr size_t KVI_CHUNK_BYTES = (size_t)16 << 20;
void kv_image_free(NanoHipModel *m) {
    NanoHipModel::KvImageIo &io = m->kvi;
    if (io.cp) (void)hipStreamSynchronize(io.cp);
    if (io.dev) (void)hipFree(io.dev);
    if (io.host) (void)hipHostFree(io.host);
    if (io.jobs) (void)hipFree(io.jobs);
    for (int h = 0; h < 2; h++) { if (io.staged[h]) (void)hipEventDestroy(io.staged[h]); if (io.freed[h]) (void)hipEventDestroy(io.freed[h]); }
    if (io.cp) (void)hipStreamDestroy(io.cp);
    io = NanoHipModel::KvImageIo{};
}
// the buffers, on first use; NANO_HIP_ENOMEM leaves none of them and the model as it was
static int kv_image_io(NanoHipModel *m, const KvImagePlan &p) {
    NanoHipModel::KvImageIo &io = m->kvi;
    if (io.dev) return 0;
    size_t target = KVI_CHUNK_BYTES;
    if (const char *mb = getenv("NANO_KV_IMAGE_CHUNK_MB")) { const unsigned long v = strtoul(mb, nullptr, 0); if (v >= 1 && v <= 1024) target = (size_t)v << 20; }
    const uint32_t all = (m->S + 63) / 64;                                  // blocks of a whole slot
    uint64_t nb = target / p.block_stride;
    if (nb < 1) nb = 1;
    if (nb > all) nb = all;
    const uint64_t half = nb * p.block_stride;
    if (half > 0x7fffffffull) FAIL(NANO_HIP_EINVAL, "KV image: a block of %llu bytes is beyond the staging buffer's 32-bit offsets", (unsigned long long)p.block_stride);
    bool ok = hipMalloc(reinterpret_cast<void **>(&io.dev), 2 * half) == hipSuccess && hipHostMalloc(reinterpret_cast<void **>(&io.host), 2 * half) == hipSuccess &&
              hipStreamCreateWithFlags(&io.cp, hipStreamNonBlocking) == hipSuccess;
    for (int h = 0; h < 2 && ok; h++)
        ok = hipEventCreateWithFlags(&io.staged[h], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&io.freed[h], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        kv_image_free(m);
        FAIL(NANO_HIP_ENOMEM, "KV image: staging buffers of 2 x %llu bytes on the device and in pinned host memory could not be allocated", (unsigned long long)half);
    }
    io.half = (size_t)half; io.chunk_blocks = (uint32_t)nb;
    return 0;
}
// The jobs of every chunk of a call, chunk after chunk (chunk c's are jobs cstart[c] .. cstart[c + 1] - 1): row[b] = the cache row of
// block b's first position (paged: the page-table entry, KV_NO_PAGE = none), or -- contiguous -- one job per chunk from base_row on.
namespace {
struct KvImageCall {
    std::vector<KvImageJob> jobs; std::vector<uint32_t> cstart{0u};
    uint32_t n_pos = 0, blocks = 0, chunk_blocks = 0;
    uint32_t chunks() const { return (uint32_t)cstart.size() - 1u; }
    uint32_t first_block(uint32_t c) const { return c * chunk_blocks; }
    uint32_t rows_of(uint32_t c) const { const uint32_t r0 = first_block(c) * 64u, r1 = r0 + chunk_blocks * 64u; return (r1 < n_pos ? r1 : n_pos) - r0; }
};
}  // namespace
static KvImageCall kv_image_jobs(const NanoHipModel *m, uint32_t n_pos, bool pack, uint64_t block_stride, uint32_t base_row, const uint32_t *row) {
    KvImageCall c;
    c.n_pos = n_pos; c.blocks = (n_pos + 63) / 64; c.chunk_blocks = m->kvi.chunk_blocks;
    for (uint32_t b0 = 0; b0 < c.blocks; b0 += c.chunk_blocks) {
        const uint32_t b1 = b0 + c.chunk_blocks < c.blocks ? b0 + c.chunk_blocks : c.blocks;
        const uint32_t rows = (b1 * 64u < n_pos ? b1 * 64u : n_pos) - b0 * 64u;
        if (!row) c.jobs.push_back(KvImageJob{ base_row + b0 * 64u, 0u, rows, 0u });
        else
            for (uint32_t b = b0; b < b1; b++) {
                const uint32_t r = (b * 64u + 64u < n_pos ? b * 64u + 64u : n_pos) - b * 64u;
                const bool none = row[b] == KV_NO_PAGE;
                c.jobs.push_back(KvImageJob{ none ? 0u : row[b], (uint32_t)((b - b0) * block_stride), r, pack ? (none ? r : 0u) : 64u - r });
            }
        c.cstart.push_back((uint32_t)c.jobs.size());
    }
    return c;
}
// the call's job list to the device, on the model's stream (from a staging copy of its own, like the copy jobs of a fork)
static int kv_image_upload(NanoHipModel *m, const KvImageCall &c) {
    NanoHipModel::KvImageIo &io = m->kvi;
    const size_t words = c.jobs.size() * 4;
    if (words > io.jobs_cap) {
        HIP_TRY(hipStreamSynchronize(m->st));                              // (a queued launch may still read the old list)
        if (io.jobs) { (void)hipFree(io.jobs); io.jobs = nullptr; io.jobs_cap = 0; }
        const size_t cap = words < 1024 ? 1024 : 2 * words;
        if (hipMalloc(reinterpret_cast<void **>(&io.jobs), cap * 4) != hipSuccess) { (void)hipGetLastError(); FAIL(NANO_HIP_ENOMEM, "KV image: a job list of %zu bytes could not be allocated", cap * 4); }
        io.jobs_cap = cap;
    }
    if (!words) return 0;
    m->kv.pt_stage.emplace_back(words, 0u);
    memcpy(m->kv.pt_stage.back().data(), c.jobs.data(), words * 4);
    HIP_TRY(hipMemcpyAsync(io.jobs, m->kv.pt_stage.back().data(), words * 4, hipMemcpyHostToDevice, m->st));
    return 0;
}
static hipError_t kv_image_launch(NanoHipModel *m, const KvImageCall &c, uint32_t chunk, int h, bool pack) {
    KvImageArgs a{};
    a.k = m->kcache; a.v = m->vcache; a.staging = m->kvi.dev + (size_t)h * m->kvi.half;
    a.row_bytes = (uint32_t)(m->KD * kv_esz(m)); a.n_layer = m->d.n_layer;
    a.plane_bytes = (uint64_t)(m->kv.paged ? (size_t)m->kv.pages * 64 : m->S) * a.row_bytes;
    a.n_jobs = c.cstart[chunk + 1] - c.cstart[chunk];
    a.job_blocks = m->kv.paged ? 1u : (c.rows_of(chunk) + 63u) / 64u;
    a.jobs = reinterpret_cast<const KvImageJob *>(m->kvi.jobs) + c.cstart[chunk];
    return launch_kv_image(a, pack, (uint32_t)m->cus, m->st);
}
static int kv_image_slot_check(const NanoHipModel *m, uint32_t slot) {
    if (slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "slot %u out of range (max_batch %u)", slot, m->maxB);
    if (!m->kv.paged && (uint64_t)m->maxB * m->d.n_layer * m->S > 0xffffffffull)
        FAIL(NANO_HIP_EINVAL, "cache of %u slots x %u rows is beyond the image kernel's 32-bit row index", m->maxB, m->d.n_layer * m->S);
    return 0;
}

extern "C" int nano_hip_kv_save(NanoHipModel *m, uint32_t slot, uint32_t n_pos, void *image, size_t cap, size_t *bytes) {
    if (!m || !image || !bytes) FAIL(NANO_HIP_EINVAL, "null argument");
    if (const int rc = kv_image_slot_check(m, slot)) return rc;
    if (n_pos > m->S) FAIL(NANO_HIP_EINVAL, "%u positions exceed max_seq_len %u", n_pos, m->S);
    KvImagePlan p;
    if (!kvi_plan(m->d.n_layer, m->KD, (uint32_t)kv_esz(m), n_pos, &p)) FAIL(NANO_HIP_EINVAL, "the model's cache has no image (kv_dim %u)", m->KD);
    *bytes = (size_t)p.total_bytes;
    if (cap < p.total_bytes) FAIL(NANO_HIP_EINVAL, "KV image of %u positions needs %llu bytes, the buffer has %zu", n_pos, (unsigned long long)p.total_bytes, cap);
    HIP_TRY(hipSetDevice(m->device));
    NanoKvImageHeader hd;
    kvi_header(&hd, m->kv_half, m->d.n_layer, m->KD, n_pos, kvi_model_tag(m->d, m->params_bytes), p);
    uint8_t *out = static_cast<uint8_t *>(image);
    if (n_pos) {
        if (const int rc = kv_image_io(m, p)) return rc;
        NanoHipModel::KvImageIo &io = m->kvi;
        const KvImageCall c = kv_image_jobs(m, n_pos, true, p.block_stride, slot * m->d.n_layer * m->S, m->kv.paged ? m->kv.h_pt + (size_t)slot * m->kv.pt_stride : nullptr);
        if (const int rc = kv_image_upload(m, c)) return rc;
        auto chunk_bytes = [&](uint32_t ch) { return (size_t)c.rows_of(ch) * m->d.n_layer * 2 * p.row_bytes; };
        // a failure past this point waits for what was queued (the caller's buffer and the pinned halves must not be written behind its back)
        hipError_t e = hipSuccess;
        auto drain = [&](uint32_t ch) {
            const int h = (int)(ch & 1u);
            if ((e = hipEventSynchronize(io.freed[h])) != hipSuccess) return;
            memcpy(out + KVI_HEADER_BYTES + (size_t)c.first_block(ch) * p.block_stride, io.host + (size_t)h * io.half, chunk_bytes(ch));
        };
        for (uint32_t ch = 0; ch < c.chunks() && e == hipSuccess; ch++) {
            const int h = (int)(ch & 1u);
            if ((e = hipStreamWaitEvent(m->st, io.freed[h], 0)) != hipSuccess) break;          // the half's earlier chunk has been copied out
            if ((e = kv_image_launch(m, c, ch, h, true)) != hipSuccess) break;
            if ((e = hipEventRecord(io.staged[h], m->st)) != hipSuccess) break;
            if ((e = hipStreamWaitEvent(io.cp, io.staged[h], 0)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(io.host + (size_t)h * io.half, io.dev + (size_t)h * io.half, chunk_bytes(ch), hipMemcpyDeviceToHost, io.cp)) != hipSuccess) break;
            if ((e = hipEventRecord(io.freed[h], io.cp)) != hipSuccess) break;
            if (ch) drain(ch - 1);                                         // ... while this chunk is packed and copied
        }
        if (e == hipSuccess) drain(c.chunks() - 1);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(m->st); (void)hipStreamSynchronize(io.cp);
            FAIL(NANO_HIP_ERUNTIME, "KV image: saving slot %u failed: %s", slot, hipGetErrorString(e));
        }
    }
    HIP_TRY(hipStreamSynchronize(m->st));                                 // (n_pos == 0 too: the call runs behind everything queued)
    memcpy(out, &hd, sizeof hd);
    return kv_stage_trim(m);
}

extern "C" int nano_hip_kv_restore(NanoHipModel *m, uint32_t slot, const void *image, size_t bytes, uint32_t n_pos) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    NanoKvImageHeader hd;
    if (const int rc = nano_hip_kv_image_check(image, bytes, &hd)) return rc;
    if (const int rc = kv_image_slot_check(m, slot)) return rc;
    if (n_pos == 0xffffffffu) n_pos = hd.n_pos;
    if (n_pos > hd.n_pos) FAIL(NANO_HIP_EINVAL, "%u positions asked of a KV image of %u", n_pos, hd.n_pos);
    if (n_pos > m->S) FAIL(NANO_HIP_EINVAL, "%u positions exceed max_seq_len %u", n_pos, m->S);
    if (hd.format != m->kv_half) FAIL(NANO_HIP_EINVAL, "KV image of element format %u, the model's cache has format %u (0 FP32, 1 FP16, 2 FP8; formats are not converted)", hd.format, m->kv_half);
    if (hd.n_layer != m->d.n_layer || hd.kv_dim != m->KD) FAIL(NANO_HIP_EINVAL, "KV image of %u layers x kv_dim %u, the model has %u x %u", hd.n_layer, hd.kv_dim, m->d.n_layer, m->KD);
    if (hd.model_tag != kvi_model_tag(m->d, m->params_bytes)) FAIL(NANO_HIP_EINVAL, "KV image with model tag %016llx, this model's is %016llx (another model file)", (unsigned long long)hd.model_tag, (unsigned long long)kvi_model_tag(m->d, m->params_bytes));
    HIP_TRY(hipSetDevice(m->device));
    KvImagePlan p, pi;                                                     // of the n_pos positions restored | of the image
    kvi_plan(hd.n_layer, hd.kv_dim, (uint32_t)kv_esz(m), n_pos, &p);
    kvi_plan(hd.n_layer, hd.kv_dim, (uint32_t)kv_esz(m), hd.n_pos, &pi);
    // paged: the slot's new table row, planned before anything is queued (the fork's rule for a destination)
    KvPlan plan;
    std::vector<uint32_t> row;
    if (m->kv.paged) {
        const uint32_t P = m->kv.pt_stride;
        std::map<uint32_t, uint32_t> leaving;
        plan.free_pages = m->kv.free_pages;
        for (uint32_t blk = 0; blk < P; blk++) {
            const uint32_t e = m->kv.h_pt[(size_t)slot * P + blk];
            if (e != KV_NO_PAGE && ++leaving[e / 64u] == m->kv.page_owners[e / 64u]) plan.free_pages.push_back(e / 64u);
        }
        if (p.blocks > plan.free_pages.size())
            FAIL(NANO_HIP_ENOMEM, "paged KV cache: restoring %u positions needs %u pages, %zu available (%zu free + the slot's own) of %u (nano_hip_kv_release() returns a finished sequence's pages)",
                 n_pos, p.blocks, plan.free_pages.size(), m->kv.free_pages.size(), m->kv.pages);
        for (const auto &lv : leaving) plan.owners.emplace_back(lv.first, -(int32_t)lv.second);
        row.assign(P, KV_NO_PAGE);
        for (uint32_t blk = 0; blk < p.blocks; blk++) {
            const uint32_t page = plan.free_pages.back(); plan.free_pages.pop_back();
            row[blk] = page * 64u;
            plan.owners.emplace_back(page, 1);
        }
        plan.rows.emplace_back(slot, row);
    }
    if (n_pos) {
        if (const int rc = kv_image_io(m, p)) return rc;
        NanoHipModel::KvImageIo &io = m->kvi;
        const KvImageCall c = kv_image_jobs(m, n_pos, false, p.block_stride, slot * m->d.n_layer * m->S, m->kv.paged ? row.data() : nullptr);
        if (const int rc = kv_image_upload(m, c)) return rc;
        const uint8_t *in = static_cast<const uint8_t *>(image);
        const uint32_t img_rows_cut = p.blocks == pi.blocks ? pi.last_rows : 64u;      // rows per run, in the image, of the block the restore ends in
        hipError_t e = hipSuccess;
        for (uint32_t ch = 0; ch < c.chunks() && e == hipSuccess; ch++) {
            const int h = (int)(ch & 1u);
            if ((e = hipEventSynchronize(io.staged[h])) != hipSuccess) break;                   // the pinned half's earlier chunk is on the device
            uint8_t *pin = io.host + (size_t)h * io.half;
            const uint32_t b0 = c.first_block(ch), rows = c.rows_of(ch), nfull = rows / 64u, part = rows % 64u;
            const size_t chunk_bytes = (size_t)rows * m->d.n_layer * 2 * p.row_bytes;
            // whole blocks are a byte range of the image; a partial last block is one too unless the image's block holds more rows (the row cut)
            const bool cut = part && img_rows_cut != part;
            memcpy(pin, in + KVI_HEADER_BYTES + (size_t)b0 * p.block_stride, cut ? (size_t)nfull * p.block_stride : chunk_bytes);
            if (cut)
                for (uint32_t run = 0; run < m->d.n_layer * 2u; run++)
                    memcpy(pin + (size_t)nfull * p.block_stride + (size_t)run * part * p.row_bytes,
                           in + kvi_offset(pi, b0 + nfull, img_rows_cut, run / 2u, run % 2u, 0), (size_t)part * p.row_bytes);
            if ((e = hipStreamWaitEvent(io.cp, io.freed[h], 0)) != hipSuccess) break;           // the device half's earlier chunk has been unpacked
            if ((e = hipMemcpyAsync(io.dev + (size_t)h * io.half, pin, chunk_bytes, hipMemcpyHostToDevice, io.cp)) != hipSuccess) break;
            if ((e = hipEventRecord(io.staged[h], io.cp)) != hipSuccess) break;
            if ((e = hipStreamWaitEvent(m->st, io.staged[h], 0)) != hipSuccess) break;
            if ((e = kv_image_launch(m, c, ch, h, false)) != hipSuccess) break;
            e = hipEventRecord(io.freed[h], m->st);
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(io.cp); (void)hipStreamSynchronize(m->st);
            FAIL(NANO_HIP_ERUNTIME, "KV image: queueing the restore into slot %u failed: %s (nothing committed)", slot, hipGetErrorString(e));
        }
    }
    return kv_apply(m, plan, "the restore");
}
