// kv_image.h -- the arithmetic of a KV image (include/nano_mi355x.h "KV images"): the 64-byte header, the block-major payload and how a
// sequence's rows are cut into staging chunks.  Host only, no device call: nano_hip_kv_image_plan / _bytes / _check (backend_kv.hip)
// answer from it without a GPU, and nano_hip_kv_save / _restore lay their staging chunks out with the same functions.
//   payload: block b = positions 64 b .. min(64 b + 63, n_pos - 1); inside a block the layers ascending, per layer the block's K rows
//   (one contiguous run) and then its V rows, every row the cache's own bytes.  Block b starts 64 b * n_layer * 2 * row_bytes into the
//   payload: every block but the last is full, and the last holds runs of n_pos % 64 rows (64 when that is 0).
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/nano_mi355x.h"

namespace nano {

#pragma GCC visibility push(hidden)
constexpr uint32_t KVI_MAGIC = 0x31564b4eu;               // "NKV1" as a little-endian word
constexpr uint32_t KVI_VERSION = 1, KVI_HEADER_BYTES = 64, KVI_BLOCK_ROWS = 64;
static_assert(sizeof(NanoKvImageHeader) == KVI_HEADER_BYTES, "the header is 64 bytes");

struct KvImagePlan {
    uint64_t payload_bytes, total_bytes, block_stride;    // block_stride: bytes of a full block = 64 * n_layer * 2 * row_bytes
    uint32_t row_bytes, blocks, last_rows, vec_bytes;     // last_rows: rows per run of the last block (0: no block); vec_bytes: 16 | 8 | 4 (launch_kv_copy's rule)
};
inline uint32_t kvi_vec_bytes(uint32_t row_bytes) { return row_bytes % 16 == 0 ? 16u : row_bytes % 8 == 0 ? 8u : 4u; }
// false: elem_bytes is not 4, 2 or 1, n_layer is 0, or kv_dim is 0 / no multiple of 4 (head_dim % 4 == 0 makes every model's one)
inline bool kvi_plan(uint32_t n_layer, uint32_t kv_dim, uint32_t elem_bytes, uint32_t n_pos, KvImagePlan *p) {
    if ((elem_bytes != 4 && elem_bytes != 2 && elem_bytes != 1) || !n_layer || !kv_dim || kv_dim % 4) return false;
    if ((uint64_t)kv_dim * elem_bytes > 0xffffffffull) return false;
    p->row_bytes = kv_dim * elem_bytes;
    p->block_stride = (uint64_t)KVI_BLOCK_ROWS * n_layer * 2 * p->row_bytes;
    p->payload_bytes = (uint64_t)n_pos * n_layer * 2 * p->row_bytes;
    p->total_bytes = KVI_HEADER_BYTES + p->payload_bytes;
    p->blocks = n_pos / KVI_BLOCK_ROWS + (n_pos % KVI_BLOCK_ROWS != 0);
    p->last_rows = !n_pos ? 0u : n_pos % KVI_BLOCK_ROWS ? n_pos % KVI_BLOCK_ROWS : KVI_BLOCK_ROWS;
    p->vec_bytes = kvi_vec_bytes(p->row_bytes);
    return true;
}
// byte offset, from the start of the image, of row `row` of the K (kv = 0) or V (kv = 1) run of `layer` in block `block` whose runs hold
// block_rows rows
inline uint64_t kvi_offset(const KvImagePlan &p, uint32_t block, uint32_t block_rows, uint32_t layer, uint32_t kv, uint32_t row) {
    return KVI_HEADER_BYTES + block * p.block_stride + ((uint64_t)(layer * 2 + kv) * block_rows + row) * p.row_bytes;
}
inline uint32_t kvi_fmt_bytes(uint32_t fmt) { return fmt == 0 ? 4u : fmt == 1 ? 2u : fmt == 2 ? 1u : 0u; }
// FNV-1a (64 bit) over the twelve NanoModelDesc words and params_bytes, each as little-endian bytes.  A guard against mixing up
// shapes: two files of one shape and size get one tag whatever their weights are.
inline uint64_t kvi_model_tag(const NanoModelDesc &d, uint64_t params_bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto eat = [&](uint64_t v, int n) { for (int i = 0; i < n; i++) { h ^= (v >> (8 * i)) & 0xffu; h *= 0x100000001b3ull; } };
    const uint32_t w[12] = { d.arch, d.block_size, d.vocab_size, d.n_layer, d.n_embd, d.n_head, d.n_kv_head, d.n_hidden,
                             d.is_shared_classifier, d.head_dim, d.quant_type, d.group_size };
    for (uint32_t x : w) eat(x, 4);
    eat(params_bytes, 8);
    return h;
}
inline void kvi_header(NanoKvImageHeader *h, uint32_t fmt, uint32_t n_layer, uint32_t kv_dim, uint32_t n_pos, uint64_t tag, const KvImagePlan &p) {
    memset(h, 0, sizeof *h);
    h->magic = KVI_MAGIC; h->version = KVI_VERSION; h->header_bytes = KVI_HEADER_BYTES; h->format = fmt;
    h->n_layer = n_layer; h->kv_dim = kv_dim; h->n_pos = n_pos; h->block_rows = KVI_BLOCK_ROWS; h->row_bytes = p.row_bytes;
    h->payload_bytes = p.payload_bytes; h->model_tag = tag;
}
// what nano_hip_kv_image_check refuses: null on success, else the message (written into msg)
inline const char *kvi_check(const void *image, size_t bytes, NanoKvImageHeader *out, char *msg, size_t cap) {
    if (!image) { snprintf(msg, cap, "KV image: null buffer"); return msg; }
    if (bytes < KVI_HEADER_BYTES) { snprintf(msg, cap, "KV image: %zu bytes are less than the %u-byte header", bytes, KVI_HEADER_BYTES); return msg; }
    NanoKvImageHeader h;
    memcpy(&h, image, sizeof h);
    if (h.magic != KVI_MAGIC) { snprintf(msg, cap, "KV image: bad magic 0x%08x (\"NKV1\" expected)", h.magic); return msg; }
    if (h.version != KVI_VERSION || h.header_bytes != KVI_HEADER_BYTES) { snprintf(msg, cap, "KV image: version %u with a %u-byte header (version %u, %u bytes expected)", h.version, h.header_bytes, KVI_VERSION, KVI_HEADER_BYTES); return msg; }
    if (h.block_rows != KVI_BLOCK_ROWS) { snprintf(msg, cap, "KV image: blocks of %u rows (%u expected)", h.block_rows, KVI_BLOCK_ROWS); return msg; }
    KvImagePlan p;
    if (!kvi_plan(h.n_layer, h.kv_dim, kvi_fmt_bytes(h.format), h.n_pos, &p)) { snprintf(msg, cap, "KV image: element format %u, %u layers, kv_dim %u describe no cache", h.format, h.n_layer, h.kv_dim); return msg; }
    if (h.row_bytes != p.row_bytes) { snprintf(msg, cap, "KV image: row_bytes %u, but kv_dim %u x %u-byte elements are %u", h.row_bytes, h.kv_dim, kvi_fmt_bytes(h.format), p.row_bytes); return msg; }
    if (h.payload_bytes != p.payload_bytes) { snprintf(msg, cap, "KV image: payload of %llu bytes, but %u positions x %u layers x 2 x %u bytes are %llu", (unsigned long long)h.payload_bytes, h.n_pos, h.n_layer, p.row_bytes, (unsigned long long)p.payload_bytes); return msg; }
    if (h.reserved0 || h.reserved1[0] || h.reserved1[1]) { snprintf(msg, cap, "KV image: reserved header words are not zero"); return msg; }
    if (bytes < p.total_bytes) { snprintf(msg, cap, "KV image: %zu bytes, but header and payload are %llu", bytes, (unsigned long long)p.total_bytes); return msg; }
    if (out) *out = h;
    return nullptr;
}
#pragma GCC visibility pop

}  // namespace nano
