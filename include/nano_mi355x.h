/*
 * nano_mi355x.h -- C-ABI of the MI355X (gfx950) device backend for Nano's decode hot path.
 *
 * This is the boundary the reference's host code binds to: plain C, plain pointers and sizes,
 * no C++ or framework types.  It replaces the *inside* of the reference's
 *
 *     float *llm_forward(Nano_Context*, uint32_t token, uint32_t pos, uint32_t max_seq_len,
 *                        uint32_t is_causal, LLM*, LoRA*)              (reference infer/infer.c:971)
 *
 * and of the operators it is built from (reference infer/infer.c:589-706, infer/tensor.c:15-471):
 * weights, KV cache and scratch become device resident; (token, pos) go in; logits[vocab] (or
 * the arg-max index) come out.  The engine API above it (llm_context_init, generate_next_token,
 * llm_session_step ... reference infer/infer.h:253-282) is declared in nano_infer_abi.h and
 * implemented in host C on top of the entry points below.
 *
 * All functions return 0 on success or a negative NANO_HIP_E* code; nano_hip_last_error() gives
 * the text.  There is NO CPU fallback: if no gfx950 device / HIP runtime is usable the create
 * call fails.  Not thread-safe per model (the reference engine is single-caller).
 */
#ifndef NANO_MI355X_H
#define NANO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NANO_ARCH_NANO  0u     /* reference infer/infer.h:45-47 */
#define NANO_ARCH_QWEN2 2u
#define NANO_ARCH_QWEN3 3u

#define NANO_QUANT_F32 0x00u   /* reference infer/tensor.h:73-77 */
#define NANO_QUANT_Q80 0x80u
#define NANO_QUANT_Q4K 0x42u

#define NANO_HIP_OK        0
#define NANO_HIP_EINVAL   -1   /* bad argument / unsupported shape */
#define NANO_HIP_ERUNTIME -2   /* HIP runtime error (text in nano_hip_last_error) */
#define NANO_HIP_ENODEV   -3   /* no usable device */
#define NANO_HIP_ENOMEM   -4

#define NANO_MAX_BATCH 64u

/* Model hyper-parameters = header words 4..16 of the .bin file (reference infer/infer.c:231-251),
 * i.e. LLM_Config + arch/quant_type/group_size of the reference's LLM struct (infer/infer.h:89-99,167-180). */
typedef struct NanoModelDesc {
    uint32_t arch;
    uint32_t block_size;
    uint32_t vocab_size;
    uint32_t n_layer;
    uint32_t n_embd;
    uint32_t n_head;
    uint32_t n_kv_head;
    uint32_t n_hidden;
    uint32_t is_shared_classifier;
    uint32_t head_dim;        /* header word 14; used for Qwen3 only */
    uint32_t quant_type;
    uint32_t group_size;
} NanoModelDesc;

typedef struct NanoHipModel NanoHipModel;   /* opaque: device weights + KV cache + scratch + graphs */

/* ---- device / errors ------------------------------------------------------------------------- */
int         nano_hip_device_count(void);
const char *nano_hip_last_error(void);
/* fills name[0..cap) with the device's gcnArchName ("gfx950..."), returns CU count or <0 */
int         nano_hip_device_info(int device, char *name, size_t cap, uint64_t *total_mem_bytes);

/* ---- model lifetime ---------------------------------------------------------------------------
 * `params` is the parameter blob exactly as it sits in the model file after the header and the
 * tokenizer section (what the reference's memory_map_params() walks, infer/infer.c:100-217); it
 * may be unaligned.  params_on_device != 0 means `params` is a DEVICE pointer on `device` (e.g. a
 * buffer filled by an RCCL broadcast); the backend then copies device-to-device.
 * max_batch independent sequences get their own FP32 KV cache [L][max_seq_len][kv_dim] x2
 * (reference infer/infer.c:46-51) and scratch; the weights are shared.
 * Replaces: memory_map_params + malloc_fwd_buffer (reference infer/infer.c:15-85,100-217). */
int  nano_hip_model_create(NanoHipModel **out, const NanoModelDesc *desc, const void *params, size_t params_bytes,
                           int params_on_device, int device, uint32_t max_seq_len, uint32_t max_batch);
/* The same with option flags.  NANO_HIP_KV_F16 (opt-in because it changes results): the KV cache holds FP16
 * rows instead of the reference's FP32 (infer/infer.c:46-51) -- half the cache memory and half the bytes attention reads
 * per position; every row is rounded once (to nearest even) when it is written, the current token attends to its own
 * rounded row, all arithmetic stays FP32.  Logits stay within the Q80 noise floor of the FP32-cache path (stated and
 * tested in tests/test_gpu_kv16.py).  Not combinable with strict mode or LoRA.  nano_hip_model_create() applies it when
 * NANO_KV_F16=1 is set in the environment. */
#define NANO_HIP_KV_F16 1u
/* NANO_HIP_KV_PAGED (opt-in; results are BIT-IDENTICAL to the contiguous cache): the KV cache is a pool of pages
 * of 64 positions ([layer][page][64][kv_dim] x2) instead of max_batch fixed slots of max_seq_len rows (the reference sizes its
 * cache statically, infer/infer.c:46-51, and reads it linearly, :850-878).  A sequence slot takes a page when its position
 * enters a new 64-position block -- taken zero-filled, like the reference's calloc'd rows -- and gives its pages back with
 * nano_hip_kv_release(); a step that finds no free page fails with NANO_HIP_ENOMEM and changes nothing.  The pool holds
 * NANO_KV_PAGES pages (environment; default max_batch * ceil(max_seq_len / 64) = what the slots would have held), so more
 * slots than the memory for full-length sequences can be open when most are short.  Combinable with NANO_HIP_KV_F16; not with
 * strict mode or LoRA.  nano_hip_model_create() applies it when NANO_KV_PAGED=1 is set in the environment.
 * Pages can have several owners: nano_hip_kv_fork() below points the destinations' table entries at the source's full pages (no byte
 * moves) and every page keeps an owner count.  A page with more than one owner is read-only: a step that is about to write into one
 * first gives the writing slot a copy of its own (copy-on-write: one free page per such block, NANO_HIP_ENOMEM and nothing changed when
 * the pool has none), and nano_hip_kv_release() returns a page to the pool only when its last owner leaves. */
#define NANO_HIP_KV_PAGED 2u
/* NANO_HIP_KV_FP8 (opt-in because it changes results): the KV cache holds one-byte OCP e4m3fn elements (bias 7, largest
 * finite +-448, smallest subnormal 2^-9, no infinities; not the MI300 fnuz encoding) with scale 1 -- a stored byte decodes to the value
 * itself.  A quarter of the FP32 cache's memory and of the bytes attention reads per position.  Every row is rounded once when it is
 * written, byte = e4m3_rne(clamp(x, -448, 448)): to nearest even, subnormals included, the sign of zero kept; out-of-range values and
 * +-Inf saturate and never become a NaN code (NaN inputs are outside the contract).  The current token attends to its own rounded k
 * and v row, all arithmetic stays FP32, and a zero byte is +0, so a fresh cache or page reads as the reference's calloc'd rows -- the
 * FP16 cache's rules.  e4m3 keeps 3 mantissa bits: the logits move further from the FP32-cache path than with FP16 rows (measured in
 * tests/test_gpu_kv8.py, stated in DESIGN.md).  Combinable with NANO_HIP_KV_PAGED; together with NANO_HIP_KV_F16 creation fails with
 * NANO_HIP_EINVAL (also when the two arrive through the environment); not with strict mode, exact mode or LoRA.
 * nano_hip_model_create() applies it when NANO_KV_FP8=1 is set in the environment. */
#define NANO_HIP_KV_FP8 4u
int  nano_hip_model_create_ex(NanoHipModel **out, const NanoModelDesc *desc, const void *params, size_t params_bytes,
                              int params_on_device, int device, uint32_t max_seq_len, uint32_t max_batch, uint32_t flags);
void nano_hip_model_destroy(NanoHipModel *m);
/* Paged KV cache only: give the pages of sequence slot `slot` back to the pool (the slot's next position is 0 again); pages in
 * use / in the pool.  Both fail with NANO_HIP_EINVAL on a model without NANO_HIP_KV_PAGED. */
int  nano_hip_kv_release(NanoHipModel *m, uint32_t slot);
int  nano_hip_kv_pages(const NanoHipModel *m, uint32_t *in_use, uint32_t *total);
/* Share a prefix between slots.  Make positions 0 .. n_pos-1 of every slot in dst_slots[0..n_dst) hold the K / V rows that
 * src_slot holds there, in every layer.  Afterwards each destination behaves exactly like a slot that was fed the same n_pos tokens
 * itself (bit for bit: batched prefill does not depend on the slot).  Both cache layouts, FP32 and FP16 rows, every mode.
 * Contiguous cache: the rows are copied (one launch for all destinations; the source is read once); rows >= n_pos of a destination
 * stay as they are.  Paged cache: a destination first gives back what it holds; every full 64-position block below n_pos is SHARED
 * (the destination's table entry points at the source's page, see NANO_HIP_KV_PAGED); a partial last block is copied into a page of
 * the destination's own whose rows from n_pos % 64 on are zero; blocks the source has not mapped stay unmapped.
 * NANO_HIP_EINVAL: null model / list, a slot >= max_batch, n_pos > max_seq_len, the source or a duplicate in dst_slots.
 * n_pos == 0 is valid (paged: the destinations end up empty).  NANO_HIP_ENOMEM: the pool cannot supply the partial-block pages
 * from its free pages plus the pages only the destinations own; nothing has changed then.  The work is queued on the model's
 * stream behind what is already there.  The reference has no counterpart (one cache per context, infer/infer.c:46-51).
 * With a LoRA table (below) a fork that copies rows also binds every destination to the source slot's entry: the rows carry that
 * module's deltas. */
int  nano_hip_kv_fork(NanoHipModel *m, uint32_t src_slot, uint32_t n_pos, const uint32_t *dst_slots, uint32_t n_dst);
/* paged models: pages that currently have more than one owner; page copies made so far because a slot wrote into a page it
 * shared (copy-on-write), since the model was created.  NANO_HIP_EINVAL on a model without NANO_HIP_KV_PAGED. */
int  nano_hip_kv_sharing(const NanoHipModel *m, uint32_t *shared_pages, uint64_t *cow_copies);

/* ---- KV images: a slot's rows in host memory and back ---------------------------------------------
 * A KV image is a self-describing byte string holding positions 0 .. n_pos-1 of one sequence slot, bit for bit as the cache holds
 * them; the caller keeps it in RAM, a file or another process.  The rows of a position do not depend on the slot, so an image
 * comes back into any slot, and into any model -- of this process or another -- opened from the same model file with the same
 * element format; decoding then continues with exactly the bits it would have had.  The reference has no counterpart (one cache per
 * context, infer/infer.c:46-51).
 * Header (64 bytes, little-endian): NanoKvImageHeader below.  model_tag is an FNV-1a (64 bit) of the twelve NanoModelDesc words and
 * params_bytes: a guard against mixing up shapes, NOT a proof of equal weights (two files of one shape and size share a tag).
 * Payload, block-major: block b covers positions 64 b .. min(64 b + 63, n_pos - 1) and starts at byte 64 + 64 b n_layer 2 row_bytes;
 * inside a block the layers ascend, and each layer holds the block's K rows (one contiguous run) and then its V rows, every row the
 * cache's own bytes (FP32, FP16 or e4m3).  The payload is n_pos n_layer 2 row_bytes bytes.  A block is a page of the paged cache, the
 * image streams in whole blocks, and the image of the first n' <= n_pos positions is a prefix of the bytes plus a row cut inside one
 * block.  The bytes are the same whether the slot was contiguous or paged: an image of one layout restores into the other.
 * Not offered: conversion between element formats (an FP32 image does not restore into an FP16 or FP8 cache), ranges that do not
 * start at position 0, an asynchronous call, file I/O or compression, replicas (the engine entries refuse a replicated context), and
 * restoring into several slots at once (restore into one, then nano_hip_kv_fork). */
typedef struct NanoKvImageHeader {
    uint32_t magic;            /* "NKV1" */
    uint32_t version;          /* 1 */
    uint32_t header_bytes;     /* 64 */
    uint32_t format;           /* element format: 0 FP32, 1 FP16, 2 FP8 e4m3 */
    uint32_t n_layer, kv_dim, n_pos;
    uint32_t block_rows;       /* 64 */
    uint32_t row_bytes;        /* kv_dim x element bytes */
    uint32_t reserved0;        /* 0 */
    uint64_t payload_bytes;    /* n_pos * n_layer * 2 * row_bytes */
    uint64_t model_tag;
    uint32_t reserved1[2];     /* 0 */
} NanoKvImageHeader;
/* Host-only (no device is touched, they answer on a machine without a GPU).
 * _plan: out[0..8) = header bytes, payload bytes, total bytes, blocks, rows per run of the last block (0 when n_pos is 0), bytes of a
 * full block (the block stride), the byte width of the vectors the pack kernel moves the rows in (16, 8 or 4, from row_bytes), 0.
 * NANO_HIP_EINVAL: null out, elem_bytes not 4 / 2 / 1, n_layer 0, kv_dim 0 or no multiple of 4.
 * _bytes: the size of the image of n_pos positions of model m (0 for a null model).
 * _check: 0 and *out_header (may be NULL) for a well-formed image; NANO_HIP_EINVAL with a message for a null or short buffer (shorter
 * than the header, or than header + payload), bad magic or version, block_rows != 64, a format / n_layer / kv_dim that describe no
 * cache, row_bytes != kv_dim x element bytes, payload_bytes that are not the plan's, non-zero reserved words. */
#define NANO_KV_IMAGE_PLAN_WORDS 8
int    nano_hip_kv_image_plan(uint32_t n_layer, uint32_t kv_dim, uint32_t elem_bytes, uint32_t n_pos, uint64_t *out);
size_t nano_hip_kv_image_bytes(const NanoHipModel *m, uint32_t n_pos);
int    nano_hip_kv_image_check(const void *image, size_t bytes, NanoKvImageHeader *out_header);
/* Save: the image of positions 0 .. n_pos-1 of `slot` into image[0..cap), any host memory; *bytes = its size.  Runs behind everything
 * queued on the model's stream and returns when `image` holds the header and all rows.  The slot, its pages and the owner counts are
 * unchanged (a shared page is read, not copied); a block the slot has not mapped (paged cache) is written as zeros, which is what
 * attention reads there.  n_pos == 0 is valid: the image is the header alone.  Every mode, layout and element format.
 * NANO_HIP_EINVAL: null model / image / bytes, slot >= max_batch, n_pos > max_seq_len, cap below the image's size (*bytes still gets
 * the size needed).  NANO_HIP_ENOMEM: the staging buffers (allocated on first use, freed with the model) could not be had; the model
 * stays usable.
 * Restore: positions 0 .. n_pos-1 of the image into `slot`; n_pos <= the header's n_pos, UINT32_MAX = all of it.  Fewer positions
 * read the byte prefix plus the row cut: a rollback to an earlier turn.  `image` is reusable at return; the device work is queued on
 * the model's stream behind what is already there.  Contiguous cache: rows 0 .. n_pos-1 of the slot are overwritten, rows >= n_pos
 * stay as they are (as with a fork).  Paged cache, the fork's contract for a destination: the slot first gives back what it holds and
 * takes ceil(n_pos / 64) pages of its own, drawn from the free pages plus those only this slot owns; rows n_pos % 64 .. 63 of a partial
 * last page are zero; other owners of pages the slot shared keep their rows.  Everything is planned first and committed after it was
 * queued: NANO_HIP_ENOMEM (pool, or staging buffers) leaves tables, owner counts and contents as they were.
 * NANO_HIP_EINVAL, before anything is queued: whatever nano_hip_kv_image_check refuses, slot >= max_batch, n_pos beyond the image or
 * max_seq_len, an element format, n_layer, kv_dim or model tag that is not the model's.
 * Neither touches the sampler's per-slot records or the lookup loop's history: those are keyed by the caller's history.
 * Neither touches the slot's LoRA table binding (nano_hip_lora_bind): an image does not know the adapter its rows were written
 * under, so the caller binds the slot as it was when the image was saved before stepping it. */
int  nano_hip_kv_save(NanoHipModel *m, uint32_t slot, uint32_t n_pos, void *image, size_t cap, size_t *bytes);
int  nano_hip_kv_restore(NanoHipModel *m, uint32_t slot, const void *image, size_t bytes, uint32_t n_pos);
/* number of parameter-blob bytes the backend expects for `desc` (0 if it cannot be derived
 * without reading the blob, i.e. Q4K whose tensor frames carry their own sizes) */
size_t nano_hip_params_bytes(const NanoModelDesc *desc);
/* algorithmic weight bytes streamed per decode step: P*(1+4/gs), P*160/256 or 4P */
uint64_t nano_hip_weight_bytes_per_step(const NanoHipModel *m);

/* ---- the forward ------------------------------------------------------------------------------
 * One decode step for `batch` independent sequences (slot i = sequence i): feeds tokens[i] at
 * position pos[i].  Positions of a slot must arrive strictly increasing from 0 within a session
 * (a new session restarts at 0 and overwrites the cache, no reset call -- reference semantics).
 * is_causal = 0 attends over all max_seq_len cache rows (only used by seq2seq, infer.c:849).
 * logits_out: NULL or host buffer of batch*vocab floats.  argmax_out: NULL or host buffer of
 * batch uint32 (first maximum, strict '>' scan order = reference sample_argmax, infer.c:1026-1037).
 * If want_logits == 0 && argmax_out == NULL the classifier GEMV is skipped (prefill positions
 * whose logits the reference computes and discards, infer.c:1146-1149).
 * Replaces: llm_forward (reference infer/infer.c:971-1018) and, for batch > 1, adds the batch
 * entry SURVEY 8b asks for. */
int nano_hip_forward(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                     uint32_t is_causal, float *logits_out, uint32_t *argmax_out);

/* The same step in two halves: _begin queues it (and the copies back) on the model's stream and returns, _end waits and
 * fills the caller's buffers (NULL = not wanted; what _begin was told to produce).  Between the two the caller may
 * begin steps on OTHER models: replicas of one model on several GPUs of a node decode their shares of a prompt batch
 * concurrently from one process (host/nano_engine.c nano_context_replicate; SURVEY 8e's "one process, 8 streams"). */
int nano_hip_forward_begin(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                           uint32_t is_causal, int want_logits, int want_argmax);
int nano_hip_forward_end(NanoHipModel *m, float *logits_out, uint32_t *argmax_out);

/* Greedy on-device decode: starting from tokens[i] at pos[i], run `steps` steps feeding each
 * slot's arg-max back in, without host round trips (tokens/positions live on the device, each
 * step is one HIP-graph replay).  out_ids: host buffer [steps][batch].  Equivalent to calling
 * generate_next_token() `steps` times with temperature 0 and repetition_penalty 1
 * (reference infer/infer.c:1135-1193). */
int nano_hip_decode_greedy(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                           uint32_t steps, uint32_t *out_ids);

/* Batched prefill: feed `count` prompt tokens at positions pos0 .. pos0+count-1 of sequence `slot`, up
 * to nano_hip_prefill_chunk_tokens() tokens per weight read instead of one forward per token; no logits are produced (the reference
 * computes and discards them for prompt positions, infer.c:1146-1149, 1258-1260).  KV rows and all later outputs equal
 * those of `count` nano_hip_forward() calls.  Replaces the prompt loop around llm_forward (infer.c:1258-1260). */
int nano_hip_prefill(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count);
/* Prompt tokens nano_hip_prefill() feeds per weight read in the model's current mode -- what a caller sizing prompt pieces needs:
 * 64 for Q80 and for a Q4K model whose seven per-layer projections all go to the int8 MFMA GEMM (whole 256-value blocks, row counts in
 * multiples of 16; NANO_MFMA_MIN_NB <= 64), 8 for every other Q4K model and for FP32, 1 in strict or exact mode (one reference-order
 * forward per token), 0 for a null model. */
uint32_t nano_hip_prefill_chunk_tokens(const NanoHipModel *m);

/* ---- scoring prefill: the log-probability of given tokens, from batched prefill -------------------------------
 * What the model thought of one fed position, reduced on the device from that position's V logits (score.hip):
 * the logits never leave the device.  The reduction shape depends on V only, so a position's six words are the same
 * bits however the prompt was cut into calls and chunks.  -inf logits add 0 to the sum and count in `rank` like any
 * float; a -inf target has logprob -inf.  Rows with NaN or +inf, and rows of -inf only, are unspecified. */
typedef struct NanoHipTokenScore {
    float    logprob;       /* target_logit - lse, that one float32 subtraction */
    float    target_logit;  /* logits[target], the stored float */
    float    max_logit;     /* the row's maximum, the stored float */
    float    lse;           /* max_logit + logf(sum_j expf(logits[j] - max_logit)) */
    uint32_t argmax;        /* first maximum, strict '>' in index order: what nano_hip_forward's argmax_out holds */
    uint32_t rank;          /* #{j : l_j > l_t} + #{j < t : l_j == l_t}; 0 exactly when target == argmax */
} NanoHipTokenScore;        /* 24 bytes */
/* Everything nano_hip_prefill(m, slot, tokens, pos0, count) does -- same chunking, same KV rows, same later outputs, bit for
 * bit -- and out[i] = the logits produced by feeding tokens[i] at pos0 + i, scored for targets[i] (targets == NULL: for
 * each row's own arg-max, so rank is 0).  Perplexity of ids[0..n): tokens = ids, targets = ids + 1, count = n - 1.
 * A chunk runs the classifier over all its rows into a buffer of chunk x V floats (allocated on the first scoring call;
 * NANO_HIP_ENOMEM leaves the model usable) and the statistics kernel behind it; the scores come back in one copy behind
 * the call's final wait.  Strict and exact mode feed token by token as nano_hip_prefill does there: each token is a
 * reference-order step with logits, so the selections are the reference's bits.  LoRA, FP16 rows and the paged cache as
 * in nano_hip_prefill.  NANO_HIP_EINVAL before anything is queued (a refused call feeds nothing): null m / tokens / out,
 * slot or position range, a token or target >= vocab.  count == 0 returns 0 and touches nothing. */
int nano_hip_prefill_score(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                           const uint32_t *targets, NanoHipTokenScore *out);
/* The statistics kernel alone on caller logits [rows][V] (host pointers; targets may be NULL); NANO_HIP_EINVAL: a null
 * logits / out pointer, rows or V of 0, a target >= V. */
int nano_hip_op_score_rows(int device, const float *logits, uint32_t rows, uint32_t V,
                           const uint32_t *targets, NanoHipTokenScore *out);

/* ---- top-k alternatives: the k most probable tokens of a row, with their log-probs (topk.hip) ---------------------
 * For a row of V float32 logits and 1 <= k <= min(NANO_TOPK_MAX, V) the row's k entries, selected on the device behind the
 * statistics above (the logits never leave the device):
 *   order    float comparison, descending; equal floats: the smaller index first.  -0.0f == +0.0f is such a tie.  Denormals
 *            compare by value (nothing is flushed).  -inf is a float like any other: a row with fewer than k finite logits goes
 *            on with its -inf entries in index order, logprob -inf.
 *   so       entry j is the token whose NanoHipTokenScore.rank would be j; top[0].token is the record's argmax.
 *   logit    the stored float, bit for bit (a -0.0f stays -0.0f);  logprob = logit - lse, that one float32 subtraction with the
 *            lse of the row's score record: a target among the k entries has the record's logprob, bit for bit.
 * Rows with NaN or +inf, and rows of -inf only, are unspecified, as above.  The selection is exact, so the entries do not depend
 * on how a prompt is cut into calls, chunks or passes, on the row's index or alignment, or on the launch that produced the logits. */
#define NANO_TOPK_MAX 32u
typedef struct NanoHipTopEntry { uint32_t token; float logit; float logprob; } NanoHipTopEntry;   /* 12 bytes */
/* In the three model entry points below k == 0 means scores only (top_out may be NULL); k >= 1 requires top_out with rows * k
 * entries in caller order, and scores_out may then be NULL.  k > NANO_TOPK_MAX, k > vocab, a null top_out with k >= 1, a null
 * scores_out with k == 0 and a target >= vocab are NANO_HIP_EINVAL before anything is queued.  The selection's scratch is allocated on the
 * first such call with k >= 1 (NANO_HIP_ENOMEM leaves the model usable); k == 0 and callers of the other entry points allocate none of it.
 *
 * nano_hip_prefill_score_topk: everything nano_hip_prefill_score does -- same chunks and chunk graphs, same KV rows, same later
 * outputs, the same score records bit for bit -- plus the k entries of every fed position (top_out[i * k + j]).  The two selection
 * launches are queued eagerly behind each chunk (strict / exact mode: behind each token's reference-order step). */
int nano_hip_prefill_score_topk(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                                const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out);
/* One causal decode step of the sequences in slots 0 .. batch-1, queued exactly as nano_hip_forward queues it with logits wanted
 * (same graphs, same re-issue after a hand-off gave up, strict / exact mode alike) -- but no logits are copied to the host: the
 * statistics and the selection run on the step's rows on the device and the records come back in one copy behind the call's
 * wait.  targets (may be NULL: each row's own arg-max) as in nano_hip_prefill_score.  The logits stay where nano_hip_forward
 * leaves them: nano_hip_read_state(m, i, 4, ...) returns the row the entries of sequence i were taken from. */
int nano_hip_forward_topk(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                          const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out);
/* The statistics and the selection alone on caller logits [rows][V] (host pointers; targets and scores_out may be NULL; top_out
 * [rows][k]).  NANO_HIP_EINVAL before a device is asked for: null logits / top_out, rows, V or k of 0, k > NANO_TOPK_MAX, k > V,
 * a target >= V. */
int nano_hip_op_topk_rows(int device, const float *logits, uint32_t rows, uint32_t V, uint32_t k,
                          const uint32_t *targets, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out);

/* ---- greedy decode with lookup drafts: several ids per weight read (opt-in) -----------------
 * Greedy decode of sequence slot 0 in which a step may be a prefill chunk of K = max_draft + 1 rows: the last id plus a
 * continuation guessed by looking the last ngram_min .. ngram_max ids up in the sequence's own history (longest suffix match, then
 * the most recent; what followed it last time, extended periodically), verified by the chunk's own row arg-maxes.  Row i's arg-max is
 * the id that follows row i's id; rows are accepted while the next row's fed id equals it, so a chunk emits 1 .. K ids and every
 * emitted id is the arg-max of a row whose whole prefix is emitted ids.  Accept, append, lookup and the staging of the next step run on
 * the device behind each step (lookup.hip); the host reads one 32-byte record per step.  A chunk never crosses a 64-position attention
 * bucket (the rule of nano_hip_prefill's chunks): positions whose chunk would take a plain one-row step, and so does a step with
 * no match, with fewer than 2 ids left, or whose chunk would pass max_seq_len / the RoPE table.
 * What the ids are: wherever a prefill chunk's rows carry the bits of token-by-token feeding (the guarantee of nano_hip_prefill; every
 * small-matrix route) they are exactly nano_hip_decode_greedy's.  On wide matrices (Qwen3-4B's shapes) launches of >= 3 rows
 * normalise through a different reduction tree, a chunk row may differ from the one-row step in the last ulp, and the promise is the one
 * batched prefill gives there: every emitted id is the arg-max of a fast-path chunk row, not necessarily decode_greedy's id at a near-tie.
 * Strict and exact mode run the loop with max_draft treated as 0: plain reference-order steps, that mode's ids.  max_draft is also
 * clipped to nano_hip_prefill_chunk_tokens() - 1 (a chunk holds no more rows than the per-token scratch).  LoRA, FP16 rows and the
 * paged cache as in nano_hip_prefill.  is_causal = 0 is not offered. */
typedef struct NanoHipLookupParams {
    uint32_t max_draft;     /* 0 .. 15 drafted ids per verify chunk; 0 = plain steps only */
    uint32_t ngram_max;     /* 1 .. 4: the longest suffix looked up */
    uint32_t ngram_min;     /* 1 .. ngram_max: the shortest match that drafts */
    uint32_t stop_token;    /* the loop ends after emitting it; UINT32_MAX = none */
    uint32_t max_steps;     /* steps (plain or verify) after which the call returns; 0 = no limit */
} NanoHipLookupParams;
typedef struct NanoHipLookupStats {
    uint32_t steps_plain, steps_verify;
    uint32_t drafted;       /* steps_verify * (the clipped) max_draft */
    uint32_t accepted;      /* draft rows confirmed, summed over the verify steps (before clipping to max_new / the stop token) */
    uint32_t emitted;       /* = *n_out */
} NanoHipLookupStats;
/* Slot 0 holds positions 0 .. n_history-2 of history[0..n_history); history[n_history-1] is fed first.  Emits at most max_new ids
 * into out_ids (host, max_new words), *n_out of them; stats may be NULL.  Afterwards slot 0 holds valid rows for positions
 * 0 .. n_history + *n_out - 2, as after nano_hip_decode_greedy; rows beyond may hold rejected drafts' K / V and are rewritten before any
 * causal step reads them.  The history lives on the device between calls: a history that extends the previous call's (its ids plus
 * what that call emitted) uploads only the new ids.
 * NANO_HIP_EINVAL before anything is queued: null m / history / p / out_ids / n_out, n_history == 0, an id >= vocab, max_draft > 15,
 * ngram_max outside 1 .. 4, ngram_min outside 1 .. ngram_max, n_history - 1 + max_new beyond max_seq_len or the RoPE table, max_new
 * beyond the trace capacity (max_seq_len * max_batch).  max_new == 0 returns 0 and touches nothing (*n_out = 0).
 * A record the host cannot accept (nb_next not 1 or K, n not grown by the emitted count, n beyond the limit) ends the call with
 * NANO_HIP_ERUNTIME.  The whole call is re-issued once after a hand-off gave up, as nano_hip_decode_greedy is. */
int nano_hip_decode_lookup(NanoHipModel *m, const uint32_t *history, uint32_t n_history, uint32_t max_new,
                           const NanoHipLookupParams *p, uint32_t *out_ids, uint32_t *n_out, NanoHipLookupStats *stats);
/* For callers with a drafter of their own: nano_hip_prefill(m, slot, tokens, pos0, count) -- same chunking, same KV rows -- that also
 * returns argmax_out[i] = the arg-max of row i's logits (the value nano_hip_prefill_score(...)[i].argmax holds) and *n_accepted = the
 * largest a <= count-1 with tokens[i] == argmax_out[i-1] for all 1 <= i <= a (tokens[0] is the last committed id, tokens[1..] the
 * draft).  Rows beyond pos0 + a hold the rejected ids' K / V: feed on from position pos0 + a + 1 with argmax_out[a].
 * NANO_HIP_EINVAL as nano_hip_prefill, and for count == 0 or a null argmax_out; n_accepted may be NULL. */
int nano_hip_verify_draft(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                          uint32_t *argmax_out, uint32_t *n_accepted);
/* The between-steps kernel alone (lookup.hip; host pointers; operator tests).  history[0..n) in, room for n + 16 ids: the emitted ids are
 * appended in place.  fed / amax [nb] describe the step it follows (nb = 0 .. 16; 0: none has run).  params as above (max_steps unused),
 * left = ids still to emit, seq_limit = min(max_seq_len, RoPE rows).  record_out[8] = {emitted, accepted, nb_next, n, match_len,
 * match_end, done, left}; next_tokens_out / next_pos_out [16] = the next step's rows (entries from nb_next on are UINT32_MAX).
 * NANO_HIP_EINVAL: null pointers, n == 0 or n > 65536, nb > 16, parameters out of their ranges. */
int nano_hip_op_lookup_step(int device, uint32_t *history, uint32_t n, const uint32_t *fed, const uint32_t *amax, uint32_t nb,
                            const NanoHipLookupParams *params, uint32_t left, uint32_t seq_limit, uint32_t *record_out,
                            uint32_t *next_tokens_out, uint32_t *next_pos_out);

/* ---- lookup drafts for several sequences: one ragged verify pass per round (opt-in) ----------
 * nano_hip_decode_lookup's contract for n_seqs sequences at once, sequence i in KV slot seqs[i].slot: the slot holds positions
 * 0 .. n_history-2 of histories[i], histories[i][n_history-1] is fed first, at most max_new ids go to out_ids[i] (host, max_new words)
 * and their count to n_out[i]; afterwards the slot holds valid rows for positions 0 .. n_history + n_out[i] - 2.  p->stop_token applies
 * to every sequence, p->max_steps bounds the call's rounds (0 = no limit).  stats (optional) holds n_seqs records, rounds (optional)
 * receives the number of rounds run.
 * A round is ONE ragged pass (as nano_hip_step_rows runs them) over the live sequences' rows: each sequence takes one row or a verify
 * chunk of D_eff + 1 rows by the one-sequence loop's own gate (a draft exists, at least 2 ids left, the chunk inside one 64-position
 * bucket and below max_seq_len / the RoPE table).  Behind the pass the definitions of the one-sequence loop run for every sequence on the
 * device (accept, emit, lookup, draft, gate) and the next pass's tokens, positions and row -> slot map are staged there; the host
 * waits once per round for n_seqs 32-byte records.  A finished sequence contributes no rows to later rounds.
 * D_eff is fixed for the call: min(p->max_draft, nano_hip_prefill_chunk_tokens(m) / n_seqs - 1), so a round is always exactly one
 * pass; in strict and exact mode it is 0 and a round is one reference-order step per live sequence in its slot (that mode's ids).
 * What the ids are: sequence i's ids and its NanoHipLookupStats are those of nano_hip_decode_lookup for that sequence alone with
 * max_draft = D_eff (with the caveat stated there for wide matrices): a sequence's rounds do not depend on what shares the pass.
 * NANO_HIP_EINVAL before anything is queued (a refused call feeds nothing): null m / seqs / histories / p / out_ids / n_out or a
 * null entry of histories / out_ids; per sequence whatever nano_hip_decode_lookup refuses; LoRA switched on or a cache the row map
 * cannot address (as nano_hip_step_rows); two sequences in one slot; a slot >= max_batch; reserved != 0; the sum of max_new beyond the
 * trace capacity (max_seq_len * max_batch); outside strict and exact mode n_seqs beyond nano_hip_prefill_chunk_tokens(m).
 * n_seqs == 0 or every max_new == 0 returns 0 and touches nothing.  A record the host cannot accept (the check of
 * nano_hip_decode_lookup, per sequence) ends the call with NANO_HIP_ERUNTIME.  No in-launch hand-off runs in an eager ragged pass, so
 * none can give up and the call is never re-issued.
 * Paged cache: the pages of positions n_history-1 .. n_history-2+max_new of every sequence are taken up front, all or nothing; shared
 * pages (nano_hip_kv_fork) are copied on write.  FP32, FP16, FP8 and the paged cache are served, as for ragged steps.
 * The histories live on the device between calls, one per KV slot (apart from nano_hip_decode_lookup's): a history that extends what
 * the slot's previous call left uploads only the new ids.  They are allocated on the first call; NANO_HIP_ENOMEM leaves the model usable.
 * NOT offered: a draft model for several sequences, sampling, logit edits, LoRA, replicas. */
typedef struct NanoHipLookupSeq { uint32_t slot, n_history, max_new, reserved; } NanoHipLookupSeq;   /* 16 bytes */
int nano_hip_decode_lookup_rows(NanoHipModel *m, const NanoHipLookupSeq *seqs, uint32_t n_seqs,
                                const uint32_t *const *histories, const NanoHipLookupParams *p,
                                uint32_t *const *out_ids, uint32_t *n_out, NanoHipLookupStats *stats, uint32_t *rounds);
/* The pass of a round, device-free (the host's copy of what the pack launch of lookup_rows.hip does).  n[i] = ids in sequence i's
 * history, nb_next[i] = its rows in the pass (0: it has none -- a dead sequence).  The live sequences are ordered stably by the range
 * hint of position n[i] - 1 (nano_hip_rows_plan's row_hint); each sequence's rows are contiguous and ascending.  order[0 .. live) =
 * the live sequences in pass order, row_start[i] = sequence i's first row (UINT32_MAX: dead), group_hint / group_rows [*n_groups] =
 * the runs of equal hints and their row counts.  Every output may be NULL; the arrays hold n_seqs entries.
 * NANO_HIP_EINVAL: null n / nb_next with n_seqs > 0, max_seq_len == 0, nb_next[i] > 16, a live sequence with n[i] == 0 or whose rows
 * end beyond max_seq_len. */
int nano_hip_lookup_rows_plan(const uint32_t *n, const uint32_t *nb_next, uint32_t n_seqs, uint32_t max_seq_len,
                              uint32_t *order, uint32_t *row_start, uint32_t *group_hint, uint32_t *group_rows, uint32_t *n_groups);
/* The two between-rounds launches alone (lookup_rows.hip; host pointers; operator tests).  Sequence i: histories[i][0 .. n[i]) in, room
 * for n[i] + 16 ids (the emitted ids are appended in place), left[i] ids still to emit, KV slot slots[i] (distinct, < 64).  fed / amax
 * [n_rows] are the previous pass in pass order, row_start[i] / nb[i] sequence i's rows there (nb[i] = 0: none; 0 .. 16).  params and
 * seq_limit as nano_hip_op_lookup_step, max_seq_len clips the range hints.  records_out [n_seqs][8] as nano_hip_op_lookup_step's;
 * next_tokens_out / next_pos_out / next_slot_out [n_seqs * 16] = the next pass in pass order (entries beyond its rows are UINT32_MAX);
 * row_start_out [n_seqs] (UINT32_MAX: no rows).
 * NANO_HIP_EINVAL before a device is asked for: null pointers, n_seqs outside 1 .. 64, n[i] == 0 or > 65536, rows outside the pass,
 * a slot >= 64 or named twice, parameters out of their ranges, max_seq_len == 0. */
int nano_hip_op_lookup_rows_round(int device, uint32_t n_seqs, uint32_t *const *histories, const uint32_t *n, const uint32_t *left,
                                  const uint32_t *slots, const uint32_t *fed, const uint32_t *amax, uint32_t n_rows,
                                  const uint32_t *row_start, const uint32_t *nb, const NanoHipLookupParams *params,
                                  uint32_t seq_limit, uint32_t max_seq_len, uint32_t *records_out, uint32_t *next_tokens_out,
                                  uint32_t *next_pos_out, uint32_t *next_slot_out, uint32_t *row_start_out);

/* ---- greedy decode with a draft model: several ids per read of the target's weights (opt-in) ----
 * Two resident models with one vocabulary on one device.  A round: the draft model runs D' one-row greedy loop steps from the last id,
 * the target verifies [last id, d1 .. dD'] as one chunk of D' + 1 rows and accepts rows exactly as nano_hip_decode_lookup does, so every
 * emitted id is the arg-max of a target row whose whole prefix is emitted ids: the output is nano_hip_decode_lookup's -- and, with the
 * caveat stated there for wide matrices, nano_hip_decode_greedy's -- for ANY draft model; only the number of rounds depends on it.
 * D' = min(max_draft, 63 - (n-1) % 64, left - 1, room below both models' max_seq_len and RoPE tables), n the history's length: a chunk
 * stays inside one 64-position bucket.  D' = 0 is a plain one-row target step (the draft falls behind and catches up later).
 * The draft holds `draft_held` leading positions of the history in ITS slot 0; the call feeds it what it lacks (hist[dn .. n-2], from
 * the device history, batched prefill without outputs) before it drafts: a caller never ingests the prompt into the draft by hand.
 * Between the models' steps runs draft.hip's kernel; the models' streams are ordered by events; the host waits once per round, for
 * the 32-byte record.  max_draft is clipped to the target's nano_hip_prefill_chunk_tokens() - 1.  A target in strict or exact mode
 * runs plain reference-order steps (max_draft treated as 0, the draft untouched).  The draft may use any quantisation and any KV cache. */
typedef struct NanoHipDraftParams {
    uint32_t max_draft;   /* 0 .. 15 drafted ids per round; 0 = plain target steps only */
    uint32_t stop_token;  /* UINT32_MAX = none */
    uint32_t max_rounds;  /* 0 = no limit */
    uint32_t draft_held;  /* leading positions of `history` that the draft's slot 0 already holds (0 = none) */
} NanoHipDraftParams;
typedef struct NanoHipDraftStats {
    uint32_t rounds_plain, rounds_verify;
    uint32_t drafted, accepted, emitted;
    uint32_t draft_rows_fed;   /* catch-up rows fed to the draft, prompt included */
    uint32_t draft_held;       /* what to pass as draft_held when the call is continued */
} NanoHipDraftStats;
/* The target's contract is nano_hip_decode_lookup's: slot 0 holds positions 0 .. n_history-2, history[n_history-1] is fed first, the
 * device history is kept between calls (and shared with nano_hip_decode_lookup), the same state is left behind.  Afterwards the draft's
 * slot 0 holds valid rows for stats->draft_held positions of history + out_ids.
 * NANO_HIP_EINVAL before anything is queued in either model: everything nano_hip_decode_lookup refuses (its n-gram parameters aside),
 * a null draft, draft == target, different devices, different vocab_size, max_draft > 15, draft_held > n_history - 1 or beyond the
 * draft's max_seq_len, a draft in strict or exact mode or with LoRA on.  max_new == 0 returns 0 and touches nothing.
 * A hand-off that gave up in either model re-issues the whole call once, the draft fed from position 0 again. */
int nano_hip_decode_draft(NanoHipModel *target, NanoHipModel *draft, const uint32_t *history, uint32_t n_history,
                          uint32_t max_new, const NanoHipDraftParams *p, uint32_t *out_ids, uint32_t *n_out, NanoHipDraftStats *stats);
/* Measurement (tools/draft_probe.py): with NANO_DRAFT_TIMING=1 in the environment at the target's first nano_hip_decode_draft call, every
 * drafted round is bracketed by timing events; this returns the summed milliseconds of {catch-up, the draft's steps, stage + verify chunk
 * + accept} and the number of rounds since the last query, and resets them.  Without the switch: zeros. */
int nano_hip_draft_phase_ms(NanoHipModel *target, double out_ms[3], uint32_t *rounds);
/* The between-steps kernel alone (draft.hip; host pointers; operator tests): its STAGE role on fed[1 .. nb), then its ACCEPT role.
 * history[0..n) in, room for n + 16 ids; the device history's capacity is min(n + 16, seq_limit + 1) rounded up to 4.  fed / amax [nb]
 * describe the round it follows (nb = 0 .. 16; 0: none has run), dn = positions the draft held before it.  record_out[8] = {emitted,
 * accepted, nb_next, n, dn, cursor, done, left}; next_tokens_out / next_pos_out [16] = row 0 and the positions of the next round
 * (next_tokens_out[1 .. nb) are what STAGE put there; untouched entries are UINT32_MAX).  NANO_HIP_EINVAL: null pointers, n == 0 or n > 65536, nb > 16, max_draft > 15, dn > n - 1. */
int nano_hip_op_draft_round(int device, uint32_t *history, uint32_t n, const uint32_t *fed, const uint32_t *amax, uint32_t nb,
                            const NanoHipDraftParams *params, uint32_t left, uint32_t seq_limit, uint32_t dn, uint32_t *record_out,
                            uint32_t *next_tokens_out, uint32_t *next_pos_out);

/* ---- ragged steps: rows of several KV slots share one weight read --------------------------------------------------
 * A step whose rows each carry their own (slot, position): several prompts in one chunk, a new prompt joining running sequences, one
 * greedy step for sequences in ANY slots, drafts of several sequences verified at once.  A segment names positions
 * pos0 .. pos0 + count - 1 of `slot`; tokens holds sum(count) ids, segment after segment.
 * Contract: the K / V rows and every later output of every slot are those of nano_hip_prefill(m, slot, ...) called per segment, bit for
 * bit (with the wide-matrix caveat stated at nano_hip_decode_lookup above), and argmax_out (optional, sum(count) words, caller order)
 * holds what nano_hip_verify_draft returns for the same rows.  A segment of count 1 is a decode row: with argmax_out one call is a
 * greedy step of the running sequences plus a piece of a newcomer's prompt.  Sampled rows follow with nano_hip_forward_sample_batch,
 * as after nano_hip_prefill.
 * How: the rows are cut into passes of up to nano_hip_prefill_chunk_tokens() rows in caller order (nano_hip_rows_plan below); a pass
 * is one embed launch and per layer one q|k|v launch, one Wo, W1|W3 and W2 launch over ALL its rows.  Each row's attention is split
 * exactly as that token's own one-sequence decode step (64 positions per split at head_dim <= 128), which is what makes the bits
 * hold: inside a pass the rows are ordered by range bucket and every bucket gets its own attention (and combine) launch.  Passes run
 * eagerly (no graphs); the call's tokens, positions and slots are staged once and the host waits once.  Paged cache: the pages of all
 * segments are ensured before anything is queued, all or nothing, shared pages copied on write as for nano_hip_prefill.  Contiguous
 * FP32 cache: the fresh v rows travel through scratch and are stored by the attention kernel's row-preparation pass, as on the FP16
 * cache (a copy: the same bits).  Strict and exact mode feed token by token, each a reference-order step in the row's slot.
 * NANO_HIP_EINVAL before anything is queued (a refused call feeds nothing): null m / segs / tokens, a slot >= max_batch, two segments
 * with the same slot, positions beyond max_seq_len or the RoPE table, a token >= vocab, reserved != 0, LoRA switched on (its v branch
 * addresses the cache by a flat stride), a cache the row map cannot address (nano_hip_rows_addressable), and whatever
 * nano_hip_prefill refuses for the model's switches.  n_segs == 0, or all counts 0, returns 0 and touches nothing.  is_causal = 0 is
 * not offered. */
typedef struct NanoHipRowSeg { uint32_t slot, pos0, count, reserved; } NanoHipRowSeg;   /* positions pos0 .. pos0+count-1 of `slot` */
int nano_hip_step_rows(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens, uint32_t *argmax_out);
/* The scoring form of a ragged step: everything nano_hip_step_rows promises for the cache, and for every row (caller order, sum(count)
 * rows) the score record and the k entries that nano_hip_prefill_score_topk returns for the same rows called per segment, bit for
 * bit.  targets (may be NULL: each row's own arg-max), k, scores_out and top_out as described at nano_hip_prefill_score_topk.  A pass
 * goes on into the classifier for all its rows and the statistics; the selection's two launches follow it.  Strict and exact mode:
 * per row a reference-order step with logits, then the statistics and the selection on that row.
 * NANO_HIP_EINVAL as nano_hip_step_rows, plus the k and target checks. */
int nano_hip_step_rows_score(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens,
                             const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out);
/* Device-free: how nano_hip_step_rows cuts its rows into passes of at most `cap` rows (cap = nano_hip_prefill_chunk_tokens()).  For
 * row r in caller order (all outputs optional, sum(count) words): row_pass[r] = its pass, row_index[r] = its row inside the pass,
 * row_hint[r] = min((pos / 64 + 1) * 64, max_seq_len), the range hint of its own decode step.  Passes fill in caller order, so a slot's
 * rows ascend over (pass, position) and there are ceil(rows / cap) passes; inside a pass rows are ordered by hint, stably.
 * NANO_HIP_EINVAL: null segs with n_segs > 0, cap or max_seq_len of 0, reserved != 0, two segments with the same slot, positions beyond
 * max_seq_len. */
int nano_hip_rows_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len,
                       uint32_t *row_pass, uint32_t *row_index, uint32_t *row_hint, uint32_t *n_passes);
/* Device-free: 1 when a contiguous cache of these dimensions can be indexed by a row map (a slot's n_layer x max_seq_len rows counted in
 * 32 bits, a layer of one slot within a 32-bit byte offset), else 0.  The paged pool is checked when the model is created. */
int nano_hip_rows_addressable(uint32_t n_layer, uint32_t max_seq_len, uint32_t kv_dim, uint32_t elem_bytes);

/* ---- text embeddings: pooled final-norm hidden states from a ragged step ---------------------
 * nano_hip_step_rows_pool feeds the rows of its segments exactly as nano_hip_step_rows does -- same passes, the same K / V rows left
 * behind bit for bit, so a caller may go on decoding from the slots -- stops every pass in front of the classifier and returns ONE
 * vector of dim floats per segment (out[n_segs][dim ? dim : n_embd], caller order).  The quantity, as float chains:
 *   per-row vector  y_r[i] = w_final[i] * (x_r[i] * (1 / sqrtf(mean(x_r^2) + 1e-5f))), x_r the row's residual after the last layer: what
 *                   the reference holds in s->x after llm_forward (its final rmsnorm).  Fast path: the sum of x^2 in ONE fixed order of the
 *                   pool kernel's own (pool.hip states it), which does not depend on the pass the row landed in, its row inside the
 *                   pass, or the other rows of the call.  Strict and exact mode: that mode's ordered rmsnorm, the reference's bits.
 *   pooling         NANO_POOL_LAST: v = y of the segment's last fed row.  NANO_POOL_MEAN: v = (((y_0 + y_1) + y_2) + ...) / (float)count,
 *                   plain FP32 adds in ascending position and one division; count == 1 gives y_0 / 1.0f, LAST's bits.  v does not depend
 *                   on how the call's rows were cut into passes.
 *   truncation      components 0 .. dim-1 are kept (dim == 0: n_embd), BEFORE normalisation.
 *   normalisation   normalize = 1: out = v * (1 / sqrtf(sum_{i<dim} v[i]^2)); fast path: a fixed order of the kernel's own; strict / exact
 *                   mode: ascending FP32.  A sum of 0 returns zeros, never NaN.  normalize = 0: out = v.
 * A segment of count 0 gets a row of zeros and touches nothing.  How: one launch behind each pass (strict / exact mode: behind each
 * pooled row's reference-order step, which LAST needs for one row per segment only), one workgroup per segment present in the pass; a
 * call whose texts fit one pass costs one extra launch, the vectors come back in one copy behind the call's one wait.
 * NANO_HIP_EINVAL before anything is queued: whatever nano_hip_step_rows refuses (LoRA included), a null p or out, pooling > 1,
 * normalize > 1, dim > n_embd, reserved != 0.  n_segs == 0 returns 0 and touches nothing.
 * Not offered: is_causal = 0 (bidirectional encoders), CLS pooling, a text longer than one call's positions (max_seq_len / the RoPE
 * table), LoRA. */
#define NANO_POOL_LAST 0u
#define NANO_POOL_MEAN 1u
typedef struct NanoHipPoolParams { uint32_t pooling, normalize, dim, reserved; } NanoHipPoolParams;   /* 16 bytes; reserved must be 0 */
int nano_hip_step_rows_pool(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens,
                            const NanoHipPoolParams *p, float *out /* [n_segs][dim ? dim : n_embd] */);
/* Device-free: the row map nano_hip_step_rows_pool builds for its kernel, from the function it builds it with.  Per FED row, in the order
 * the call feeds them (pass after pass, a pass's rows by row_index of nano_hip_rows_plan; all outputs optional, sum(count) words):
 * row_seg = its segment, row_ordinal = its ordinal among the segment's pooled rows, 0xffffffff where the row is not pooled (LAST: every
 * row but the segment's last, which is ordinal 0; MEAN: row j of a segment is ordinal j).  NANO_HIP_EINVAL as nano_hip_rows_plan, and
 * for pooling > 1. */
int nano_hip_rows_pool_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len, uint32_t pooling,
                            uint32_t *row_seg, uint32_t *row_ordinal);
/* The pool kernel alone on caller rows (host pointers; the fast form: it norms the rows itself).  x[rows][n_embd] holds the residual
 * rows segment after segment, seg_count[n_segs] their counts (sum = rows); the rows are cut into passes of at most pass_cap rows
 * exactly as a model with that chunk size would cut them (positions from 0) and one launch runs per pass.  out[n_segs][dim ? dim :
 * n_embd].  NANO_HIP_EINVAL before a device is asked for: null x / w_final / seg_count / p / out, n_segs or n_embd of 0, rows not the
 * sum of the counts, pass_cap of 0 or above 256, and the parameter checks above. */
int nano_hip_op_pool_rows(int device, const float *x, uint32_t rows, uint32_t n_embd, const float *w_final, const uint32_t *seg_count,
                          uint32_t n_segs, const NanoHipPoolParams *p, uint32_t pass_cap, float *out);

/* LoRA side branches of the Nano architecture (reference infer.c:434-498 loader, 792-808 / 898-903 forward).
 * `params` = the floats that follow the 256-byte header of a LoRA module file, in file order; rank / alpha = header words
 * 6 / 7.  Attaching enables the module (every KV slot's rows take it; a call that fails leaves the model as it was);
 * nano_hip_lora_enable(m, 0/1) is the reference's per-call `lora != NULL`.
 * Replaces: load_lora / parse_lora_file's device side and the use_lora branches of transformer_block_forward. */
int nano_hip_lora_attach(NanoHipModel *m, uint32_t rank, uint32_t alpha, const float *params, size_t n_floats);
int nano_hip_lora_enable(NanoHipModel *m, int on);

/* LoRA table: up to NANO_LORA_TABLE_MAX modules resident on the device and a binding KV slot -> entry.  Every step that runs the LoRA
 * launches then applies to each row the module of that row's slot (slot0 + b in a decode step, the chunk's slot for every row of a prefill /
 * scoring / verify chunk), or none: one base model, one weight read per step, each running sequence with its own adapter.  The binding
 * belongs to the slot, not to a call: the slot's K / V rows carry that module's deltas for as long as the sequence lives.
 *   nano_hip_lora_param_floats  floats of a module's parameter block (what follows a module file's 256-byte header): device-free.
 *   nano_hip_lora_table_set     stores `params` (layout and meaning as nano_hip_lora_attach) as entry id and switches the table on.
 *                               Overwriting an entry is allowed while no slot is bound to it.
 *   nano_hip_lora_table_clear   empties an entry; NANO_HIP_EINVAL while a slot is bound to it.  An empty table is no table.
 *   nano_hip_lora_bind          slots[i] takes entry ids[i], or none (NANO_LORA_NONE).  A small upload: captured graphs read the
 *                               bindings when they replay and are kept.  (Storing or clearing an entry and switching the table on or
 *                               off drop the graphs.)
 *   nano_hip_lora_binding       *id_out = the entry of `slot`, or NANO_LORA_NONE.
 * A row with module i is bit for bit what a model with module i attached (nano_hip_lora_attach) gives that row; a row without a module
 * keeps q, k and v as the projections left them and adds -0.0f in Wo's epilogue, which changes no bit.  A model with a stored, enabled
 * table is a model "with LoRA on" wherever this header says so: one attention split, the gates of nano_hip_lora_attach.
 * nano_hip_lora_enable switches whichever is present.  nano_hip_kv_fork copies the source slot's binding to its destinations;
 * nano_hip_kv_restore leaves bindings alone (an image does not know its adapter: bind the slot before stepping it).
 * NANO_HIP_EINVAL before anything is allocated or queued, the model unchanged: a null pointer, an id >= NANO_LORA_TABLE_MAX, a slot >=
 * max_batch, a bind to an empty entry, a slot named twice in one call, an architecture other than Nano, a rank the launches cannot run
 * (as nano_hip_lora_attach), a parameter block shorter than nano_hip_lora_param_floats, a set or clear of a bound entry, and a table
 * call on a model with an attached module (nano_hip_lora_attach on a model with a stored entry likewise).
 * Not offered: LoRA for the Qwen architectures (the reference has none); a table on the FP16, FP8 or paged cache, in strict or exact
 * mode, in ragged steps or pooling; more than one attention split with a module on; adapters in quantized form; bindings inside KV
 * images. */
#define NANO_LORA_TABLE_MAX 64u
#define NANO_LORA_NONE      0xffffffffu
size_t nano_hip_lora_param_floats(uint32_t n_layer, uint32_t n_embd, uint32_t kv_dim, uint32_t rank);
int nano_hip_lora_table_set(NanoHipModel *m, uint32_t id, uint32_t rank, uint32_t alpha, const float *params, size_t n_floats);
int nano_hip_lora_table_clear(NanoHipModel *m, uint32_t id);
int nano_hip_lora_bind(NanoHipModel *m, const uint32_t *slots, const uint32_t *ids, uint32_t n);
int nano_hip_lora_binding(const NanoHipModel *m, uint32_t slot, uint32_t *id_out);

/* ---- device-side sampling ------------------------------------------------------------------
 * One decode step of sequence slot 0 followed by the reference's sampler, run on the device: repetition penalty over
 * `history[0..n_history)` (the reference marks output_ids[0..pos), infer.c:1158-1166), temperature, softmax, top-p
 * nucleus, one draw with `coin` (the caller's xorshift64* float, infer/utils.c:959-970).  temperature == 0 gives the
 * penalised arg-max (infer.c:1169-1171).  The sampled token is the one the host code returns for the same logits
 * (expf, the index-order float sum, the stable sort and the cut are evaluated in the reference's order).
 * A nucleus that does not fit the LDS sorter (more than NANO_SAMPLE_MAX_CANDIDATES tokens down to the bin of the cut: near-uniform
 * distributions) is sampled by a second device phase (every candidate through a device radix sort, the same sequential cut and draw):
 * n_sorted == n_candidates then.  status NANO_SAMPLE_FALLBACK is left for the cases the device declines (no candidate at all, or no memory
 * for the second phase's scratch): `token` is not valid and the caller samples on the host from the logits of this step
 * (nano_hip_read_state(m, 0, 4, ...)); nothing else has to be redone.
 * Replaces: the D2H copy of V logits plus the host loops of generate_next_token (infer.c:1156-1189). */
#define NANO_SAMPLE_OK        0u
#define NANO_SAMPLE_FALLBACK  1u
#define NANO_SAMPLE_MAX_CANDIDATES 8192u
typedef struct NanoHipSample {
    uint32_t token;            /* sampled token id */
    uint32_t status;           /* NANO_SAMPLE_* */
    uint32_t n_candidates;     /* tokens with p >= (1-top_p)/(V-1) */
    uint32_t n_sorted;         /* of those, how many the device sorted (a superset of the nucleus) */
    uint32_t nucleus;          /* tokens kept by the top-p cut */
    uint32_t top[6];           /* the six most probable tokens (the reference's sampling observation, infer.c:1085-1094) */
    uint32_t sum_bits;         /* bits of the softmax denominator */
    uint32_t walked_chunks;    /* diagnostic: 256-element chunks the denominator was added element by element */
} NanoHipSample;
int nano_hip_forward_sample(NanoHipModel *m, uint32_t token, uint32_t pos, const uint32_t *history, uint32_t n_history,
                            float repetition_penalty, float temperature, float top_p, float coin, NanoHipSample *out);
/* The sampler alone on caller-provided logits (host pointer, V floats): operator parity tests. */
int nano_hip_op_sample(NanoHipModel *m, const float *logits, const uint32_t *history, uint32_t n_history,
                       float repetition_penalty, float temperature, float top_p, float coin, NanoHipSample *out);

/* ---- device-side sampling of a batched step -------------------------------------------------------------
 * The sampler above over rows; the one-row calls above are a batch of one (slot 0).  Row i gets its own penalty, temperature,
 * top_p, coin and history, and its result equals what a batch of that row alone returns for its logits, field by field.  The six
 * kernels run once for all rows; temperature-0 rows take the penalised arg-max; a row whose nucleus does not fit the LDS sorter goes
 * through the wide phase (rows one after another); NANO_SAMPLE_FALLBACK means the same as above (the row's logits:
 * nano_hip_read_state(m, i, 4, ...)).
 * Each slot keeps its own record of the ids already marked (slot 0's serves one-row and batched calls alike): when row i's history
 * extends slot i's last one only the new ids are uploaded, otherwise the slot's set starts over.  The scratch, about 1.5 MB per row
 * at V = 151 936, is sized to max_batch rows and allocated on the first sampled call of any kind, one-row calls included: small next
 * to one sequence's KV cache, and one row for a model opened with max_batch = 1 (the engine's default).  NANO_HIP_ENOMEM if it
 * cannot be allocated, and the model stays usable.  batch <= max_batch; every row's history is checked before anything is queued
 * (null pointers, length <= max_seq_len + 1, ids < V). */
typedef struct NanoHipSampleParams {
    float repetition_penalty, temperature, top_p, coin;
    const uint32_t *history; uint32_t n_history;     /* the ids the penalty marks (reference infer.c:1158-1166) */
} NanoHipSampleParams;
/* one decode step of slots 0..batch-1 (as nano_hip_forward), then row i sampled with params[i] into out[i] */
int nano_hip_forward_sample_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                  const NanoHipSampleParams *params, NanoHipSample *out);
/* the sampler alone on caller logits [batch][V] (host pointer; operator parity tests) */
int nano_hip_op_sample_batch(NanoHipModel *m, const float *logits, uint32_t batch,
                             const NanoHipSampleParams *params, NanoHipSample *out);

/* ---- top-k truncation in front of the top-p cut -----------------------------------------------------------
 * The calls above with one more row parameter; they are these calls with top_k = 0, and top_k == 0 is that sampler field for field.
 * For top_k >= 1 the result is that of sample_top_p (reference infer/infer.c:1062-1109) with one statement added behind its qsort:
 *     if (top_k > 0 && (uint32_t)n0 > top_k) n0 = top_k;
 * The softmax denominator runs over all V tokens and the candidates are p >= cutoff as before; the stable descending sort (equal
 * probabilities in index order) is cut to its first min(n0, top_k) entries, and the cut loop and the draw run on that list: `last` is
 * the first running sum above top_p, else the list's last entry; r = coin * cdf[last]; the pick is the first running sum above r, else
 * `last`.  So:
 *   - n_candidates stays the count of p >= cutoff;
 *   - nucleus = last + 1 <= top_k;
 *   - top[i] is 0 for i >= min(n0, top_k);
 *   - sum_bits and walked_chunks do not depend on top_k;
 *   - temperature 0 ignores top_k;
 *   - n_sorted is a diagnostic (>= nucleus) and otherwise unspecified for top_k >= 1;
 *   - any top_k >= 1 is accepted, and a top_k of V or more changes nothing.
 * With more candidates than the LDS sorter holds, only the histogram bins down to the one in which the count reaches top_k are sorted
 * (or down to the bin of the top-p cut, whichever comes first), so a flat distribution with a small top_k stays out of the wide phase;
 * a row whose leading bin alone exceeds the sorter (all logits equal) still goes there and is truncated in the same way.
 * NANO_HIP_EINVAL before anything is queued for a non-zero reserved word, and for everything the calls above refuse. */
typedef struct NanoHipSampleParamsEx {
    NanoHipSampleParams p;
    uint32_t top_k;
    uint32_t reserved[3];
} NanoHipSampleParamsEx;   /* top_k 0 = off; reserved must be 0 */
int nano_hip_forward_sample_batch_ex(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                     const NanoHipSampleParamsEx *params, NanoHipSample *out);
int nano_hip_op_sample_batch_ex(NanoHipModel *m, const float *logits, uint32_t batch,
                                const NanoHipSampleParamsEx *params, NanoHipSample *out);

/* ---- logit edits: allowed-token masks and logit bias in front of the pick ---------------------------------
 * The _ex calls above with a per-row edit; they are these calls with no edit, and a row without an edit is the _ex row field for field.
 * Let V be the vocabulary and W = ceil(V / 32).  A row may carry
 *   - a mask: W words; token j is allowed when bit (j & 31) of word (j >> 5) is set.  Bits of tokens >= V in the last word are ignored,
 *     whatever they hold.  Given per call (`allow`, host memory, uploaded with the call) or by id from the model's mask table
 *     (`mask_id`, 1-based; nano_hip_mask_table_set uploads the table once: ban lists, fixed answer sets, a grammar's per-state masks);
 *   - a bias list: n_bias <= NANO_BIAS_MAX entries {token, bias}; the tokens are distinct and may come in any order.
 * The edited row is
 *     x_j  = l_j + b_j                      one float32 add, only for a token that has an entry; a token without one keeps its stored bits
 *     l'_j = allowed(j) ? x_j : -INFINITY
 * and the result is the sampler's result on l' as the _ex call defines it: penalty, temperature, softmax over all V, candidates, stable
 * sort, top-k cut, top-p cut, draw; temperature 0 gives the first maximum of the penalised l'.  So y = ((l + b) / penalty) / temperature.
 * ONE difference from the reference sampler run on l': a disallowed token is never a candidate -- the candidate test is
 *     allowed(j) && p_j >= cutoff.
 * For top_p < 1 that changes nothing (p = 0 < cutoff).  For top_p >= 1 the cutoff is <= 0 and the reference on l' counts the p = 0
 * tokens as candidates, lists them in top[] and returns the sorted list's last entry when coin * sum is not below the sum; with the filter
 * n_candidates and top[] hold allowed tokens only.
 * GUARANTEE: a result with NANO_SAMPLE_OK names an allowed token, for every top_p, top_k, coin and temperature.
 *   - sum_bits and walked_chunks are those of the _ex call on l';
 *   - a -inf bias is allowed and bans that one token;
 *   - an edited row whose allowed tokens are all -inf after the bias is unspecified, as rows of -inf only are elsewhere;
 *   - the step's logits are NOT modified: nano_hip_read_state(m, i, 4, ...) still returns what nano_hip_forward leaves; the edit enters
 *     only the sampler's y.
 * NANO_HIP_EINVAL before anything is queued (a failed table call leaves the old table in place) for: `allow` and `mask_id` both given;
 * a mask_id beyond the table; a mask (per call or in the table) with no allowed token among its first V bits; n_bias > NANO_BIAS_MAX;
 * n_bias > 0 with a null list; a bias token >= V; a token listed twice; a NaN or +inf bias; and everything the _ex calls refuse.
 * The staging of per-call masks and bias lists -- pinned plus device memory of max_batch x (W x 4 + NANO_BIAS_MAX x 8) bytes -- is
 * allocated on the first call that carries an edit (NANO_HIP_ENOMEM leaves the model usable); callers that never edit allocate nothing
 * new.  Masks and lists go up in the same single copy as the rows' parameters and new history ids; a table mask costs no upload.
 * NOT offered here: edits for nano_hip_decode_greedy's device loop, nano_hip_decode_lookup and nano_hip_verify_draft; for the scoring
 * and top-k entry points (log-probs renormalised over an allowed set are another reduction); inside nano_hip_step_rows; and deriving
 * masks from a grammar -- that is the caller's library, this is the hook it needs. */
#define NANO_BIAS_MAX 1024u
typedef struct NanoHipLogitBias { uint32_t token; float bias; } NanoHipLogitBias;
typedef struct NanoHipSampleParamsEdit {
    NanoHipSampleParamsEx ex;            /* reserved words still 0 */
    const uint32_t *allow;               /* host, W words, or NULL */
    const NanoHipLogitBias *bias;        /* host, n_bias entries, or NULL */
    uint32_t mask_id;                    /* 0 = none, else 1-based index into the model's mask table */
    uint32_t n_bias;
} NanoHipSampleParamsEdit;
/* n_masks x W words (host); replaces the table; n_masks = 0 frees it */
int nano_hip_mask_table_set(NanoHipModel *m, const uint32_t *words, uint32_t n_masks);
int nano_hip_forward_sample_batch_edit(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                       const NanoHipSampleParamsEdit *params, NanoHipSample *out);
int nano_hip_op_sample_batch_edit(NanoHipModel *m, const float *logits, uint32_t batch,
                                  const NanoHipSampleParamsEdit *params, NanoHipSample *out);

/* ---- strict-parity / per-phase mode -------------------------------------------------------------------------
 * nano_hip_set_strict(m, 1): every later forward / prefill runs eagerly, one kernel per reference operator, with
 * every float reduction (rmsnorm, q.k, softmax sum, weighted V, FP32 matmul) in the reference's sequential order
 * and the pinned libm's expf: the logits equal the reference CPU engine's BIT FOR BIT for F32, Q80 and Q4K models
 * (tests/test_gpu_strict.py).  Slow (a thread walks each chain); it exists as the parity proof and as the
 * un-fused replay behind the per-phase observation hook.  Also switched on by NANO_STRICT=1 in the environment
 * at model creation.  LoRA side branches are not covered (the call fails with NANO_HIP_EINVAL).
 * nano_hip_set_phase_hook: in strict mode fn(env, layer, phase) is called on the caller's thread at the twelve
 * points the reference fires ctx->observation from inside its forward (reference infer/infer.c:755-949, 985-1003;
 * phase = NANO_LLM_PHASE_* 1..11, layer = -1 / 0..L-1 / L), after all device work queued before that point has
 * finished, so nano_hip_read_state() inside the hook sees the tensors of that phase.  fn = NULL removes it. */
typedef void (*nano_hip_phase_fn)(void *env, int32_t layer, int32_t phase);
int nano_hip_set_strict(NanoHipModel *m, int on);
int nano_hip_set_phase_hook(NanoHipModel *m, nano_hip_phase_fn fn, void *env);

/* ---- exact mode: the reference's bits from graph-replayed steps --------------------------------------------------
 * nano_hip_set_exact(m, 1): every later step (forward, forward_begin/_end, decode_greedy, prefill, forward_sample[_batch],
 * time_step) returns what strict mode returns -- the reference CPU engine's logits, arg-max ids and sampled tokens, bit for bit,
 * for F32, Q80 and Q4K models -- from a step that is captured once per (batch, mode, is_causal) and replayed as a HIP graph,
 * the on-device greedy loop included.  Its float chains are exact.hip's: rmsnorm with the sum of squares in index order out of
 * LDS; q / k preparation + scores + softmax + weighted V of a layer in ONE launch with att[range] in LDS.  That launch needs att[max_seq_len] to fit
 * its 64 KiB of LDS: models created with max_seq_len > 7168 keep strict mode's three attention launches (att in global memory)
 * inside the captured step -- same bits, no context length is refused.  Prefill runs token by token (MODE_NOCLS replays).
 * Also switched on by NANO_EXACT=1 in the environment at model creation.
 * Interplay: strict mode wins when both are on; with a phase hook installed an exact-mode step is served by the strict step
 * (same bits; the hook needs the eager per-operator replay); LoRA side branches, the FP16 and the paged KV cache are refused with
 * NANO_HIP_EINVAL as in strict mode; the in-launch hand-offs (NANO_FUSE_LAUNCHES) are not used, so the mode has no give-up path.
 * nano_hip_exact_state: *on = the switch, *graphs = exact-mode graphs instantiated, *launches_per_step = kernel nodes of the
 * last enqueued exact step (0 before the first one, and with NANO_HIP_NO_GRAPH).  Any pointer may be NULL. */
int nano_hip_set_exact(NanoHipModel *m, int on);
int nano_hip_exact_state(const NanoHipModel *m, uint32_t *on, uint32_t *graphs, uint32_t *launches_per_step);

/* Blocks until all work queued on the model's stream has finished. */
int nano_hip_sync(NanoHipModel *m);

/* ---- measurement -------------------------------------------------------------------------------
 * Launches the classifier GEMV (the dominant kernel: vocab x n_embd rows) `iters` times back to
 * back on the model's stream between two HIP events and returns the average milliseconds per
 * launch and the algorithmic bytes one launch streams. */
int nano_hip_time_classifier(NanoHipModel *m, uint32_t batch, uint32_t iters, float *ms_per_launch, uint64_t *bytes_per_launch);
/* The same launch timed where it runs: inside `iters` whole decode steps at position `pos` (eager launches, HIP
 * events on the model's stream right before / after the classifier launch).  Its weights are cold there -- the
 * layers' bytes went through the caches since the previous step -- which back-to-back launches of
 * nano_hip_time_classifier() do not guarantee.  *ms_per_launch is the raw event span, *ms_empty_pair (optional)
 * the span of an empty event pair recorded right after it (event overhead, reported, not subtracted). */
int nano_hip_time_classifier_in_step(NanoHipModel *m, uint32_t batch, uint32_t pos, uint32_t iters, float *ms_per_launch,
                                     uint64_t *bytes_per_launch, float *ms_empty_pair);
/* Same for one whole decode step (graph replay), `iters` replays between two events. */
int nano_hip_time_step(NanoHipModel *m, uint32_t batch, uint32_t pos, uint32_t iters, float *ms_per_step);
/* Device read-bandwidth microbenchmark: streams `bytes` of device memory `iters` times; GB/s out. */
int nano_hip_membw(int device, size_t bytes, uint32_t iters, float *gbps);

/* ---- in-launch hand-offs: state, switches, fault injection -----------------------------------------
 * One-sequence Q80 steps fuse launches whose workgroups hand results to each other INSIDE a launch (q|k|v -> attention, Wo -> W1|W3;
 * DESIGN.md section 3).  Every such wait is
 * bounded; when one gives up (the chip shared with work that kept the producers off the CUs) the engine switches the fusions off for
 * this model and RE-ISSUES the call through the plain launches -- the caller gets the results, `fallbacks` counts the event.
 * nano_hip_handoff_state: fused_mask = the NANO_FUSE_LAUNCHES bits in force (1 q|k|v + attention, 2 Wo + W1|W3), fallbacks = re-issues
 * so far, last_code = code bits of the last give-up.
 * nano_hip_set_fusion: set those bits (drops the captured graphs); other bits: NANO_HIP_EINVAL.
 * nano_hip_debug_fault (tests): bit 0 = the producers of every hand-off publish with a wrong tag, so each consumer gives up (the
 * give-up path on demand); bit 1 = no re-issue: the call returns NANO_HIP_ERUNTIME.  0 restores both.
 * nano_hip_background_load (tests): a competing streaming reader on the XCDs of `xcd_mask`, see backend.hip. */
int nano_hip_handoff_state(const NanoHipModel *m, uint32_t *fused_mask, uint32_t *fallbacks, uint32_t *last_code);
int nano_hip_set_fusion(NanoHipModel *m, uint32_t mask);
int nano_hip_debug_fault(NanoHipModel *m, uint32_t flags);
int nano_hip_background_load(int device, size_t bytes, uint32_t iters, uint32_t xcd_mask, uint32_t wgs);

/* ---- debugging / parity access -----------------------------------------------------------------
 * Copy a scratch tensor of slot `slot` to the host after a forward.  which: 0=x 1=q 2=xba 3=hb
 * 4=logits 5=k cache row (layer,pos) 6=v cache row (layer,pos).  n floats are copied. */
int nano_hip_read_state(NanoHipModel *m, uint32_t slot, int which, uint32_t layer, uint32_t pos, float *out, size_t n);

/* ---- single operators (host pointers in/out; same device kernels as the forward) ---------------
 * These exist so that every kernel can be checked against the oracle on oracle-fed inputs.
 * Replaces, in order: rmsnorm (infer.c:601), matmul (infer.c:637), quantize (tensor.c:21),
 * matmul_quant (infer.c:654), quantize_tensor_q4k_in_situ (tensor.c:281, 1-D), matmul_q4k
 * (tensor.c:438), rope / rope_qwen3 (infer.c:681/692), the attention loop (infer.c:842-879). */
int nano_hip_op_rmsnorm(int device, float *out, const float *x, const float *w, uint32_t n);
int nano_hip_op_matmul_f32(int device, float *out, const float *x, const float *w, uint32_t n, uint32_t d);
int nano_hip_op_quantize_q80(int device, const float *x, uint32_t n, uint32_t gs, int8_t *q, float *s);
int nano_hip_op_matmul_q80(int device, float *out, const int8_t *xq, const float *xs, const int8_t *wq,
                           const float *ws, uint32_t n, uint32_t d, uint32_t gs);
/* blocks_out: ceil(n/256)*160 bytes (the block array of a 1-D Q4k_Tensor, frame prefix excluded) */
int nano_hip_op_quantize_q4k(int device, const float *x, uint32_t n, uint8_t *blocks_out);
/* w_blocks: d*ceil(n/256)*160 bytes; x_blocks: ceil(n/256)*160 bytes */
int nano_hip_op_matmul_q4k(int device, float *out, const uint8_t *x_blocks, const uint8_t *w_blocks, uint32_t n, uint32_t d);
int nano_hip_op_rope(int device, float *head, uint32_t head_dim, const float *fcr, const float *fci, int qwen3_style);
/* q[n_head*hd] (already normed+roped), k/v caches [range][kv_dim]; out[n_head*hd] */
int nano_hip_op_attention(int device, float *out, const float *q, const float *k_cache, const float *v_cache,
                          uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t range);
/* One decode attention launch exactly as a step issues it (the non-fused path of a decode step, or with `chunk` the two passes of a
 * batched prefill chunk): q / k rmsnorm and RoPE of the raw rows, the finished k row (FP16 cache: and the v row) stored at pos, causal
 * attention over rows 0..pos, split partials combined by the batched / prefill combine.  Replaces infer/infer.c:810-879.  The op stages
 * each sequence's RoPE row (and, paged, its pool row) as the step's embed kernel does.  All pointers are host pointers; the caches are
 * copied in and back whole, so the caller sees every element the launch wrote. */
typedef struct NanoAttnDecodeDesc {
    uint32_t nb;                /* sequences (1..NANO_MAX_BATCH); chunk: tokens of the one sequence */
    uint32_t n_head, n_kv_head, hd, n_layer, layer, S;     /* S: cache rows per layer of a slot, and rows of the RoPE tables */
    uint32_t range_hint;        /* max(pos) + 1 <= range_hint <= S */
    uint32_t nsplit;            /* 0: attention_nsplit(range_hint, hd); else forced (<= 64) */
    uint32_t rope_qwen3;        /* 1: (i, i + hd/2) pairs, 0: adjacent pairs */
    uint32_t kv_half;           /* the cache's element format: 0 FP32, 1 FP16 (k_cache / v_cache hold uint16 bit patterns), 2 FP8 e4m3fn (bytes) */
    uint32_t chunk;             /* 1: the nb rows are consecutive positions of ONE sequence: pass 1 (prep_only), then pass 2 */
    uint32_t want_frag;         /* 1: also the Q80 groups of 64 in fragment order (nsplit == 1, hd % 64 == 0 only) */
    uint32_t pool_rows;         /* paged cache: rows of one layer plane (a multiple of 64); 0: contiguous cache */
    uint32_t pt_stride;         /* paged: page-table entries per sequence */
    const float *q;             /* [nb][n_head * hd] raw q */
    const float *k;             /* [nb][n_kv_head * hd] raw k of pos */
    const float *vraw;          /* FP16 / FP8 cache: [nb][kv_dim] v of pos (FP32), or NULL; FP32 cache: the v rows of pos are in v_cache already */
    const uint32_t *pos;        /* [nb] */
    const float *q_norm, *k_norm;          /* [hd] (Qwen3) or NULL */
    const float *rope_cos, *rope_sin;      /* [S][hd / 2] */
    const uint32_t *pt_rows;    /* paged: [sequences (chunk: 1)][pt_stride] first pool row of each 64-position page, 0xffffffff = none */
    void *k_cache, *v_cache;    /* in / out: contiguous [sequences (chunk: 1)][n_layer][S][kv_dim], paged [n_layer][pool_rows][kv_dim] */
    float *out;                 /* [nb][n_head * hd] head outputs */
    int8_t *xf;                 /* want_frag: [ceil(nb / 16)][n_head * hd / 64][1024] */
    float *xsf;                 /* want_frag: [ceil(nb / 16)][n_head * hd / 64][16] */
    uint32_t *plan;             /* optional [2][10]: {mode, lpr, qv, kvm, npt, w16, paged, kv_half, nsplit, xcd} of the launch (chunk: pass 1, pass 2) */
} NanoAttnDecodeDesc;
int nano_hip_op_attention_decode(int device, const NanoAttnDecodeDesc *d);
int nano_hip_op_swiglu(int device, float *hb, const float *hb2, uint32_t n);
/* exact mode's two kernels on caller inputs (exact.hip).  rmsnorm: infer.c:601-614.  Attention: infer.c:842-879 for one sequence and
 * one layer -- q finished (norm + RoPE), caches [S][kv_dim]; is_causal: rows 0 .. range - 1, else all S rows; long_form = 1 runs the
 * three strict-mode launches an exact step keeps where att[S] does not fit the one-launch kernel's LDS. */
int nano_hip_op_exact_rmsnorm(int device, float *out, const float *x, const float *w, uint32_t n);
typedef struct NanoExactAttnDesc {
    uint32_t n_head, n_kv_head, hd, S;
    uint32_t range;             /* is_causal: positions attended (1 .. S) */
    uint32_t is_causal;
    uint32_t long_form;         /* 1: scores / softmax / weighted V as three launches, att in global memory */
    uint32_t _pad;
    const float *q;             /* [n_head * hd] */
    const float *k_cache, *v_cache;        /* [S][n_kv_head * hd] */
    float *out;                 /* [n_head * hd] */
} NanoExactAttnDesc;
int nano_hip_op_exact_attention(int device, const NanoExactAttnDesc *d);

int nano_hip_op_argmax(int device, const float *x, uint32_t n, uint32_t *idx);

/* One FUSED decode GEMV launch exactly as a decode step issues it (the role-specialised kernels: rmsnorm + activation
 * quantization prologue, optional split-attention combine, store / residual / SwiGLU epilogue), for operator tests of those
 * kernels on caller-chosen inputs.  What it replaces in the reference: rmsnorm + quantize + matmul(_quant | _q4k) (+ the
 * residual add / SwiGLU) of one projection, infer/infer.c:758-786 (kind 0), 885-908 and 950-965 (kind 1), 914-944 (kind 2).
 * With tile_max the launch is also asked for the arg-max partials exactly where a step's classifier launch is, and with argmax_out
 * the arg-max kernel of a greedy step (sample_argmax, infer.c:1026-1037) runs behind it.  All pointers are host pointers. */
typedef struct NanoFusedGemvDesc {
    uint32_t quant;             /* NANO_QUANT_F32 / _Q80 / _Q4K */
    uint32_t gs;                /* Q80 group size */
    uint32_t kind;              /* 0: out = W act (up to 3 weight tensors, e.g. q | k | v); 1: out += W act; 2: out = silu(W0 act) * (W1 act) */
    uint32_t n, nb, nseg;       /* row length, sequences (1..64), weight tensors (kind 2: 2) */
    uint32_t rows[3];
    const void *w[3];           /* F32: float[rows][n]; Q80: int8[rows][n]; Q4K: 160-byte blocks, no frame prefix */
    const float *ws[3];         /* Q80: float[rows][n/gs] */
    const float *x;             /* [nb][n] fp32 activation (NULL when attn_part is given) */
    const float *norm_w;        /* rmsnorm weight [n], or NULL: no norm */
    const float *attn_part;     /* optional, kind 1: [nb][nsplit][n] unnormalised attention partials, combined in the prologue */
    const float *attn_ml;       /* [nb][n_head][nsplit][2] (max, exp-sum) per split */
    uint32_t attn_nsplit, attn_n_head, attn_hd;
    uint32_t use_gemm;          /* 1 (Q80): the batched route of a step -- activation quantizer launch + int8 MFMA GEMM; 1 (FP32, 9..64 sequences):
                                 * the activation prologue launch + the FP32 MFMA GEMM where it takes the shape, else the sliced GEMV route */
    uint32_t ordered;           /* 1: strict mode -- the reference's ascending group order in every kernel (bit-exact fp32); 0: the fast path */
    uint32_t *route_out;        /* optional: the route the launch took (RouteKind of nano_amd/csrc/kernels.h), or NULL */
    float *out;                 /* [nb][sum of rows] (kind 2: [nb][rows[0]]); kind 1: holds the residual stream on entry */
    uint32_t out_slots;         /* 0: nb.  Else out holds out_slots >= nb sequence slots; a launch must leave those beyond nb alone */
    uint32_t out_stride;        /* 0: sum of rows.  Else floats between the slots of out (>= sum of rows; the rest are guard elements) */
    /* optional, for tests of the arg-max partials a step's classifier launch writes (all NULL / 0: a launch without them) */
    float *tile_max;            /* float[tile_slots][tile_pairs][2], or NULL.  It goes to the device whole and comes back whole, and stands for
                                 * the step's partials buffer: the launch is asked for partials exactly where the step's classifier is (one STORE
                                 * tensor, at most 8 sequences, a route that takes no fragments, Q4K: a batch that runs as one launch) and then writes,
                                 * as in a step, nb x ntiles (max value, bits of its first row | 0xffffffff: no row) pairs densely from the start of
                                 * the buffer -- pair t of sequence b at float (b * ntiles + t) * 2 -- and nothing else */
    uint32_t tile_slots;        /* capacity of tile_max: >= nb, */
    uint32_t tile_pairs;        /* ... and >= the pairs per sequence the launch writes (else an error, before any launch) */
    uint32_t *ntiles_out;       /* optional: pairs per sequence the launch was asked for and the arg-max kernel reads; 0: the launch was not asked */
    uint32_t *argmax_out;       /* optional uint32_t[nb]: behind the launch, the arg-max kernel as a greedy step builds it -- over out[b][: sum of
                                 * rows], from the partials where the launch was asked for them, scanning the result otherwise */
    const float *resid_add;     /* optional, kind 1 only: [nb][resid_add_stride] -- the addend of the residual epilogue, out += (W act + resid_add)
                                 * (the LoRA o-branch's o1, infer.c:898-908); NULL: out += W act.  The plan queries read it as a flag */
    uint32_t resid_add_stride;  /* floats between the sequences of resid_add (>= rows[0]) */
} NanoFusedGemvDesc;
int nano_hip_op_fused_gemv(int device, const NanoFusedGemvDesc *d);

/* The two LoRA side-branch launches of a layer (nano_amd/csrc/lora.hip) exactly as a decode step issues them, on caller-chosen inputs:
 *   nano_hip_op_lora_qkv   q[b] += s B_q (A_q xb),  kraw[b] += s B_k (A_k xb),  v[b * v_bstride + pos[b] * KD ...] += s B_v (A_v xb)
 *                          with xb = rmsnorm(x[b], norm_w) and s = (float)alpha / (float)rank     (reference infer/infer.c:792-808)
 *   nano_hip_op_lora_o     q[b] = s B (A x[b]) -- x = the attention output, q = o1, a[0] / b[0] = the o pair    (infer.c:898-903)
 * q, kraw and v go to the device whole (q_floats / k_floats / v_floats floats) and come back whole, so the caller sees every element a
 * launch wrote: q holds nb rows of E floats from its start, kraw nb rows of KD; v is a whole cache plane [slots][S][KD] and v_bstride the
 * floats between the sequences' slots -- S * KD for a decode step, 0 for a prefill chunk (every sequence is a position of one slot).
 * Refused before any launch (NANO_HIP_EINVAL): a null pointer, nb of 0 or above NANO_MAX_BATCH, E % 4 != 0, rank of 0, E + 3 rank + 32
 * floats beyond the 64 KiB of LDS a launch may ask for, a buffer smaller than its rows, pos[b] >= S, a v row beyond v_floats.
 * All pointers are host pointers. */
typedef struct NanoLoraOpDesc {
    uint32_t E, KD, rank, alpha, nb, S;
    uint32_t v_bstride, _pad;
    const float *x;             /* [nb][E] */
    const float *norm_w;        /* qkv: [E] */
    const float *a[3], *b[3];   /* qkv: the q, k, v pairs -- a[i] [rank][E], b[i] [E | KD | KD][rank]; o: a[0] / b[0] [E][rank] */
    const uint32_t *pos;        /* qkv: [nb] */
    float *q, *kraw, *v;        /* in-place targets (o: q alone, overwritten) */
    uint64_t q_floats, k_floats, v_floats;
} NanoLoraOpDesc;
int nano_hip_op_lora_qkv(int device, const NanoLoraOpDesc *d);
int nano_hip_op_lora_o(int device, const NanoLoraOpDesc *d);
/* The same two launches with a module per row (a LoRA table: each row takes the module of its KV slot, or none; the operators above are
 * one adapter with every row bound to it), one launch on caller arrays:
 * the fields of NanoLoraOpDesc that do not depend on the module, n_adapters adapters {rank, alpha, a[3], b[3]} (o: a[0] / b[0] = the o
 * pair), and row_adapter[nb] = each row's adapter or NANO_LORA_NONE.  A row without an adapter: nano_hip_op_lora_qkv_rows leaves its q,
 * kraw and v rows untouched, nano_hip_op_lora_o_rows stores -0.0f into its row of q.  The launch's LDS is sized by the largest rank.
 * Refused before any launch, before a device is asked for (NANO_HIP_EINVAL): what the operators above refuse (each adapter's rank), n_adapters
 * of 0 or above NANO_LORA_TABLE_MAX, a null adapters / row_adapter, a row_adapter entry that is neither an adapter nor
 * NANO_LORA_NONE.  No host path: without a device NANO_HIP_ENODEV. */
typedef struct NanoLoraAdapter {
    uint32_t rank, alpha;
    const float *a[3], *b[3];
} NanoLoraAdapter;
typedef struct NanoLoraRowsOpDesc {
    uint32_t E, KD, nb, S;
    uint32_t v_bstride, n_adapters;
    const float *x;             /* [nb][E] */
    const float *norm_w;        /* qkv: [E] */
    const NanoLoraAdapter *adapters;    /* [n_adapters] */
    const uint32_t *row_adapter;        /* [nb] */
    const uint32_t *pos;        /* qkv: [nb] */
    float *q, *kraw, *v;        /* in-place targets (o: q alone, overwritten) */
    uint64_t q_floats, k_floats, v_floats;
} NanoLoraRowsOpDesc;
int nano_hip_op_lora_qkv_rows(int device, const NanoLoraRowsOpDesc *d);
int nano_hip_op_lora_o_rows(int device, const NanoLoraRowsOpDesc *d);
/* The FP32 launch the router issues for descriptor d (quant = NANO_QUANT_F32), from the functions the launcher and the router follow:
 * out = {role, B, nv, upw, rw, nw, grid, lds_bytes, launches, seqs_per_launch, takes, 0} -- gemv_f32_slab_kernel<role, B, nv, upw> on
 * nw waves x grid workgroups owning rw rows each, of the first of `launches` slices of seqs_per_launch sequences.  takes = 0: the
 * shape is refused before any launch (a row of more than 16384 floats, 8192 with SwiGLU; one sequence that does not fit a CU's LDS).
 * Host arithmetic on the shape fields: works without a device, and no pointer of d is followed (norm_w / attn_part: null or not). */
#define NANO_F32_GEMV_PLAN_WORDS 12
int nano_hip_f32_gemv_plan(const NanoFusedGemvDesc *d, uint32_t cus, uint32_t out[NANO_F32_GEMV_PLAN_WORDS]);
/* The FP32 MFMA GEMM launch (9..64 sequences per weight read) the router issues for descriptor d (quant = NANO_QUANT_F32) in a model, or
 * through nano_hip_op_fused_gemv with use_gemm = 1: out = {route, sw, threads, grid, lds_bytes, rt, nw, nt, nu, upw, tp, stage_bytes, tab_off,
 * pro_threads, pro_lds, xs_floats, takes}.  route 9: gemm_f32_kernel<sw> (sw = 1: the W1 and W3 tiles of SwiGLU in one workgroup) on
 * threads = 64 nw threads x grid workgroups of one rt = 16 row tile each and lds_bytes of dynamic LDS; nt token tiles of 16; a row is nu
 * units of 128 floats, unit u belongs to wave u % nw (at most upw per wave); LDS = nw transposition buffers of stage_bytes, then at tab_off
 * the unit-sum table [sw + 1][nu][rt][tp] floats; in front of it the activation prologue launch of pro_threads threads (the thread count
 * of the sliced route's launch for the shape: its rmsnorm tree) x nb workgroups with pro_lds bytes, which writes xs_floats floats of
 * operand-order scratch.  A descriptor the GEMM refuses (nb outside 9..64, a row the GEMV plan refuses, segment rows no multiple of 16,
 * split-attention partials, more LDS than a CU has, a tensor of 2^32 bytes or more): the route of the sliced GEMV launches
 * (nano_hip_f32_gemv_plan reports them), takes = 1 and zeros for the plan.  Same promises as nano_hip_f32_gemv_plan. */
#define NANO_F32_GEMM_PLAN_WORDS 17
int nano_hip_f32_gemm_plan(const NanoFusedGemvDesc *d, uint32_t cus, uint32_t out[NANO_F32_GEMM_PLAN_WORDS]);
/* The Q80 launch the router issues for descriptor d (quant = NANO_QUANT_Q80), likewise: out = {route, kernel, role, gs, B, nv, upw, rw, nw,
 * grid, lds_bytes, variant, pre, launches, seqs_per_launch, takes, cw}.  cw = 1 (the new 17th word; words 0 .. 15 are what they were):
 * the residual launch behind split attention runs gemv_q80_slab_cw_kernel<nv, upw, wfc>, the splits' weights made inside each wave (the
 * environment's NANO_COMBINE_WAVE=0 refuses that form).  route: the router's choice with the step's scratch present (the value
 * route_out of nano_hip_op_fused_gemv reports).  Routes that end in the Q80 GEMV: kernel 1 = gemv_q80_slab_kernel<role, gs, B, nv, upw>
 * in its form `variant` (0 plain, 1 early, 2 wf, 3..5 wfc2..4), 2 = gemv_q80_stream_kernel<role, gs, B, nv>; nw waves x grid workgroups,
 * rw rows per workgroup, lds_bytes of dynamic LDS; pre = 1: the activation reaches the kernel quantized; the plan is that of the first
 * of `launches` slices of seqs_per_launch sequences.  The batched routes (G6 / G7 / G2 / GC): the route, launches = 1,
 * seqs_per_launch = nb, zeros for the kernel fields.  takes = 0: the shape is refused before any launch (a SLAB row of more than 65536
 * values, 32768 with SwiGLU; one sequence that does not fit a CU's LDS) and every other entry is 0.  Host arithmetic on the shape fields:
 * works without a device, and no pointer of d is followed (norm_w / attn_part: null or not). */
#define NANO_Q80_GEMV_PLAN_WORDS 17
int nano_hip_q80_gemv_plan(const NanoFusedGemvDesc *d, uint32_t cus, uint32_t out[NANO_Q80_GEMV_PLAN_WORDS]);
/* The batched Q80 launch the router issues for descriptor d (quant = NANO_QUANT_Q80), likewise: out = {route, kernel, tt, nv, r, ms, tp, pp,
 * gs, sw, threads, grid, lds_bytes, norm_order, hh, ntiles, tc0, tc1, tpw, full, nu, nk, ttl, nw, rounds, tts, magic, nsa, pre, a_stage, a_ws,
 * b_base, b_stage, b_xs, ks, ncw, nss, tab, ring, nl, waves, lt, nhc, nwaves, ng, npass, takes}.  kernel: 1 G6 MODE S, 2 G6 MODE F, 3 G7,
 * 4 G7K, 5 GC, 6 G2 with its template values (G6: nv, r, ms, tt; G7: tp, pp, ms; GC: tt; G2: gs, sw, tt), threads x grid workgroups,
 * lds_bytes of dynamic LDS, norm_order = the tree width of the activation quantizer launch in front, and the fields the kernel's
 * argument block is filled from (fields of other kernels: 0).  A descriptor whose route ends in the GEMV kernels: the route, takes = 1,
 * zeros for the rest (nano_hip_q80_gemv_plan reports that launch).  Same assumptions, flags and promises as nano_hip_q80_gemv_plan. */
#define NANO_Q80_GEMM_PLAN_WORDS 47
int nano_hip_q80_gemm_plan(const NanoFusedGemvDesc *d, uint32_t cus, uint32_t out[NANO_Q80_GEMM_PLAN_WORDS]);
/* The Q4K launch the router issues for descriptor d (quant = NANO_QUANT_Q4K), likewise: out = {route, kernel, role, B, nv, ipt, d, loop,
 * rounds, wg[3], rw, nthr, grid, lds_bytes, pre, quant_rows, quant_nthr, quant_nv, partials, launches, seqs_per_launch, takes}.  route: the
 * router's choice with the step's scratch present.  The GEMV route: kernel 1 = gemv_q4k_slab_kernel<role, B, nv, ipt>, 2 =
 * gemv_q4k_chunk_kernel<role, nv, d, loop, B> (whole 256-value blocks; `rounds` passes of the looping form, wg[s] workgroups on tensor s);
 * nthr threads x grid workgroups of rw rows, lds_bytes of dynamic LDS; pre = 1: the activation reaches the kernel quantized; quant_rows = 1:
 * a q4k_quant_rows_kernel<., quant_nv> launch of quant_nthr threads per sequence goes first (the chunk kernel's 2..8 sequences); partials:
 * arg-max pairs per sequence the launch writes when asked (a launch of one STORE tensor is planned with the request, as the step's
 * classifier makes it); the plan is that of the first of `launches` slices of seqs_per_launch sequences.  The GEMM route (9..64 tokens):
 * the route, launches = 1, seqs_per_launch = nb, zeros for the kernel fields.  takes = 0: the shape is refused before any launch (several
 * tensors whose rows are no multiples of 4 or more than 4 items per thread on the slab kernel; one sequence that does not fit a CU's LDS)
 * and every other entry is 0.  Host arithmetic on the shape fields: works without a device, and no pointer of d is followed. */
#define NANO_Q4K_GEMV_PLAN_WORDS 24
int nano_hip_q4k_gemv_plan(const NanoFusedGemvDesc *d, uint32_t cus, uint32_t out[NANO_Q4K_GEMV_PLAN_WORDS]);

/* ---- the two fused one-sequence launches of a decode step: their plans, and each launch alone on caller inputs ----
 * nano_hip_qkv_attn_fused_plan: the q | k | v + attention launch a step issues for the projection `qkv` (kind 0, three tensors, one
 * sequence, norm_w) and the attention `attn` (nb = 1; its nsplit, 0: the step's own choice for range_hint, and range_hint), from the function
 * the launcher follows: out = {kernel, nv, upw, d, qv, threads, n_attn, ngemv, lds_bytes, rw, wg[3], rounds, 0, takes}.  kernel 1 =
 * qkv_attn_fused_kernel<nv, upw> (Q80, product table), 2 = qkv_attn_fused_wf_kernel<1, upw> (Q80, rows of one chunk folded in the wave),
 * 3 = q4k_qkv_attn_fused_kernel<nv, d>, 4 = f32_qkv_attn_fused_kernel<1, upw, qv>; `threads` threads x (ngemv projection workgroups of rw
 * rows, wg[s] on tensor s (FP32: all in wg[0]), then n_attn attention workgroups), lds_bytes of dynamic LDS.  takes = 0: the step issues the
 * two plain launches -- the shape is refused, or the projection's route is not the one GEMV / Q4K launch -- and every other entry is 0.
 * nano_hip_wo_w13_fused_plan: the Wo + W1|W3 launch (Q80) for `wo` (kind 1, optional attn_part) and `w13` (kind 2, norm_w; n = wo's rows):
 * out = {sig, threads, role, wf, wfc, nv_a, upw_a, nv_b, upw_b, wa, wb, lds_bytes, rw_a, rw_b, 0, takes, cw} -- wo_w13_fused_kernel<role, nv_a,
 * upw_a, nv_b, upw_b, threads, wf, wfc> on wb workgroups, the first wa of which also run Wo's rows (rw_a and rw_b rows per workgroup); role
 * 2 = residual, 3 = residual behind the split combine; cw 1 = the combine's weights are made inside each wave and only the live splits
 * are read (wo_w13_fused_cw_kernel<wf, wfc>; the environment's NANO_COMBINE_WAVE=0 refuses that form).  takes = 0 likewise.
 * LAYOUT: the array GREW from 16 to 17 words -- words 0 .. 15 are what they were, cw is the new last word; a caller built against
 * the 16-word header must be rebuilt (its buffer is one word short).  The same holds for nano_hip_q80_gemv_plan, below.
 * Both are host arithmetic on the shape fields: they work without a device and follow no pointer (norm_w, q_norm / k_norm and attn_part
 * are read as null or not; every other pointer of the descriptors is not looked at). */
#define NANO_QKV_ATTN_FUSED_PLAN_WORDS 16
#define NANO_WO_W13_FUSED_PLAN_WORDS 17
int nano_hip_qkv_attn_fused_plan(const NanoFusedGemvDesc *qkv, const NanoAttnDecodeDesc *attn, uint32_t cus, uint32_t out[NANO_QKV_ATTN_FUSED_PLAN_WORDS]);
int nano_hip_wo_w13_fused_plan(const NanoFusedGemvDesc *wo, const NanoFusedGemvDesc *w13, uint32_t cus, uint32_t out[NANO_WO_W13_FUSED_PLAN_WORDS]);
/* One q | k | v + attention launch exactly as a step issues it (replaces infer/infer.c:758-786 and 810-879 of one layer).  The op stages
 * the RoPE row of pos as the embed kernel does, takes the granule buffer and the tick words from the code a model takes them from, sets
 * tick[0] = tick0 + 1 (the embed kernel opens a new epoch) and issues the launch with layer1 (1..127; the tag is tick * 128 + layer1).
 * qkv: x [n], norm_w, the three tensors; its out, if not NULL, receives the raw q | raw k rows the launch stored ([q_dim + kv_dim]).  attn: nb = 1, contiguous FP32 cache; q and k are not read (the launch's own
 * projection feeds the attention); k_cache / v_cache go in and come back whole; out = the head outputs (nsplit > 1: the partials combined
 * as a step combines them).  A shape the plan refuses: NANO_HIP_EINVAL before any launch.  A consumer that gave up its wait
 * (NANO_DEVERR_HANDOFF in the error word): NANO_HIP_ERUNTIME, and no result is handed back. */
typedef struct NanoQkvAttnFusedDesc {
    const NanoFusedGemvDesc *qkv;
    const NanoAttnDecodeDesc *attn;
    uint32_t layer1, tick0;
    const unsigned long long *hand_init;   /* optional: the granule buffer's content before the launch, q_dim + 2 kv_dim entries (tag << 32 | value bits); NULL: zeros */
    float *part_out;            /* optional, nsplit > 1: [nsplit][q_dim] raw partials */
    float *ml_out;              /* optional, nsplit > 1: [n_head][nsplit][2] */
    uint32_t *plan_out;         /* optional [NANO_QKV_ATTN_FUSED_PLAN_WORDS]: the plan that ran */
    uint32_t *err_out;          /* optional: the model-style sticky error word after the launch */
} NanoQkvAttnFusedDesc;
int nano_hip_op_qkv_attn_fused(int device, const NanoQkvAttnFusedDesc *d);
/* One Wo + W1|W3 launch exactly as a step issues it (replaces infer/infer.c:885-944 of one layer).  wo: kind 1, x = the attention output
 * [n] or attn_part / attn_ml; its out holds the residual stream on entry and on return.  w13: kind 2 with norm_w; its x is not read -- the
 * launch's input is the residual stream Wo leaves, as in a step; its out receives hb.  tick0, layer1, hand_init (w13->n entries), refusal
 * and give-up as for nano_hip_op_qkv_attn_fused. */
typedef struct NanoWoW13FusedDesc {
    const NanoFusedGemvDesc *wo, *w13;
    uint32_t layer1, tick0;
    const unsigned long long *hand_init;
    uint32_t *plan_out;         /* optional [NANO_WO_W13_FUSED_PLAN_WORDS] */
    uint32_t *err_out;
} NanoWoW13FusedDesc;
int nano_hip_op_wo_w13_fused(int device, const NanoWoW13FusedDesc *d);

/* One device-resident copy of a model's parameter bytes per GPU from ONE host upload (replicate.hip; SURVEY 8e "broadcast(weights) at
 * load"): the bytes go to `root_device` over PCIe once and from there to the other devices over xGMI -- an RCCL broadcast (librccl.so
 * is dlopen()ed on first use) or, when RCCL is unavailable / NANO_REPLICATE_VIA=peer, hipMemcpyPeer; NANO_REPLICATE_VIA=host uploads
 * per device; NANO_REPLICATE_VIA=rccl insists on RCCL, =peer on hipMemcpyPeer (also with one device: a 1-rank communicator / a copy whose
 * source device is its destination).  devices[i]'s copy is nano_hip_blob_ptr(share, i), to be handed to
 * nano_hip_model_create[_ex] with params_on_device = 1; nano_hip_blob_done(share, i) says replica i is built (the copy is freed once no
 * later entry of `devices` shares it: the transient footprint is ONE extra copy of the parameters per device); release frees what is left.
 * Errors name the device. */
typedef struct NanoBlobShare NanoBlobShare;
int nano_hip_blob_share(NanoBlobShare **out, const void *host_params, size_t bytes, int root_device, const int *devices, int n_devices);
const void *nano_hip_blob_ptr(const NanoBlobShare *s, int i);
void nano_hip_blob_stats(const NanoBlobShare *s, double *upload_s, double *share_s, char *how, size_t how_cap);
void nano_hip_blob_done(NanoBlobShare *s, int i);
void nano_hip_blob_release(NanoBlobShare *s);
int nano_hip_model_device(const NanoHipModel *m);

/* Phase stamps -- measurement only.  The library built with `make -C nano_amd/csrc stamps` (libnano_mi355x_stamps.so) has its
 * GEMV and attention kernels write shader-clock stamps per workgroup: [launch][2048 workgroups][8 stamps], stamp 0 = kernel
 * entry ... (tools/stamp_probe.py names them).  _begin arms the buffer; the steps that follow run eagerly and number their
 * launches; _read returns them with the launch kinds (1 QKV, 2 attention, 3 Wo, 4 W1|W3, 5 W2).  In the product library the
 * kernels ignore the buffer and every stamp reads 0. */
int nano_hip_stamps_begin(NanoHipModel *m);
int nano_hip_stamps_read(NanoHipModel *m, unsigned long long *out, uint32_t *kinds, uint32_t cap_launches, uint32_t *n_launches);

#ifdef __cplusplus
}
#endif
#endif /* NANO_MI355X_H */
