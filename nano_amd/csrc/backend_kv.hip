// backend_kv.hip -- the KV cache as the host sees it: where its rows are, the paged cache (pages on demand, copy-on-write, release),
// a prefix shared between slots (fork).
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
        return kv_apply(m, p, "the fork");
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
    return kv_apply(m, p, "the fork");
}
