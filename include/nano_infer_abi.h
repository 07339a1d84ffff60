/*
 * nano_infer_abi.h -- the engine-level C API of the MI355X drop-in, i.e. what a Nano front-end
 * (main_cli.c, main_wss.c, main_wasm.c, ui_llm.c ...) includes instead of the reference's
 * infer/infer.h.  Same exported symbols, same argument meaning, same struct field names and
 * layout (the front-ends read ctx->llm->config.*, ->arch, ->quant_type, ->group_size,
 * ctx->tokenizer->vocab[id] and the Nano_Session fields directly: reference infer/main_cli.c:146-240,
 * infer/main_wss.c:65-101), same status codes and error behaviour (loader failures print to stderr
 * and exit(EXIT_FAILURE), reference infer/infer.c:81-84,332,341-343).
 *
 * What is different underneath: llm_forward() and everything below it run on the GPU through the
 * C-ABI of nano_mi355x.h.  The host-side weight pointers of LLM_Param and the scratch pointers of
 * FwdBuffer stay NULL (the tensors live in HBM), except state.logits which is the host buffer
 * llm_forward() returns (callers mutate it in place, reference infer/infer.c:1163,1175,1178).
 *
 * Tokenizers are not part of the accelerated path: the text-level entry points call the
 * reference's own tokenizer.c / utils.c functions (build_bpe_tokenizer, encode_nano, decode_nano,
 * apply_qwen_chat_template, decode_bpe, new_map, new_trie, ...) which a front-end keeps linking
 * unchanged; they are WEAK references here, so the library also loads stand-alone for the
 * id-level API (generate_next_token, llm_forward, nano_forward_batch).
 */
#ifndef NANO_INFER_ABI_H
#define NANO_INFER_ABI_H

#include <stddef.h>
#include <stdint.h>
#include <wchar.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants (reference infer/infer.h:45-76) --------------------------------------------------- */
#define LLM_ARCH_NANO  (0)
#define LLM_ARCH_QWEN2 (2)
#define LLM_ARCH_QWEN3 (3)

#define LLM_RUNNING_IN_PREFILLING (11)
#define LLM_RUNNING_IN_DECODING   (12)
#define LLM_STOPPED_NORMALLY      (-10)
#define LLM_STOPPED_IN_PREFILLING (-11)
#define LLM_STOPPED_IN_DECODING   (-12)
#define LLM_STOPPED_WITH_ERROR    (-20)
#define IS_LLM_RUNNING(x) ((x) > 0)

#define NANO_LLM_PHASE_EMBEDDING  (1)
#define NANO_LLM_PHASE_ATTN_NORM  (2)
#define NANO_LLM_PHASE_QKV        (3)
#define NANO_LLM_PHASE_QK_ROPE    (4)
#define NANO_LLM_PHASE_MHA        (5)
#define NANO_LLM_PHASE_O          (6)
#define NANO_LLM_PHASE_FFN_NORM   (7)
#define NANO_LLM_PHASE_W1W3       (8)
#define NANO_LLM_PHASE_W2         (9)
#define NANO_LLM_PHASE_FINAL_NORM (10)
#define NANO_LLM_PHASE_CLASSIFY   (11)
#define NANO_LLM_PHASE_SAMPLE     (12)

#ifndef QUANT_TYPE_F32               /* reference infer/tensor.h:73-77 */
#define QUANT_TYPE_F32  (0x00)
#define QUANT_TYPE_Q80  (0x80)
#define QUANT_TYPE_Q4K  (0x42)
#endif

/* ---- tensor views (reference infer/tensor.h:84-90,116-117,142-146) -------------------------------- */
typedef struct { int8_t *q; float *s; } Q80_Tensor;
typedef uint8_t Q4k_Tensor;
typedef union { Q4k_Tensor *tensor_q4k; Q80_Tensor tensor_q80; float *tensor_f32; } Typed_Tensor;

/* ---- tokenizer (reference infer/tokenizer.h:17-38); owned by the front-end's tokenizer.c ----------- */
typedef struct { char *str; int id; } TokenIndex;
struct Trie;
struct Map;
typedef struct {
    uint32_t vocab_size;
    wchar_t *unicode_charset;
    wchar_t **token_list;
    struct Trie *vocab_trie;
    struct Map *unicode_to_id_map;
    struct Map *token_to_id_map;
    char **vocab;
    float *vocab_scores;
    TokenIndex *sorted_vocab;
    unsigned int max_token_length;
    unsigned char byte_pieces[512];
} Tokenizer;

/* ---- model (reference infer/infer.h:78-180) --------------------------------------------------------- */
typedef struct Nano_Observation {
    int32_t layer;
    int32_t phase;
    uint32_t token_0, token_1, token_2, token_3, token_4, token_5;
} Nano_Observation;

typedef struct {
    uint32_t block_size, vocab_size, n_layer, n_embd, n_head, n_kv_head, n_hidden;
    uint32_t is_shared_classifier;
    uint32_t head_dim;
} LLM_Config;

typedef struct {                 /* host views: NULL in this implementation (weights live in HBM) */
    Typed_Tensor *q_tokens;
    float *token_embedding;
    float *rms_norm_attn, *rms_norm_ffn, *rms_norm_final;
    Typed_Tensor *wq, *wk, *wv, *wo;
    float *bq, *bk, *bv;
    float *q_norm, *k_norm;
    Typed_Tensor *w1, *w2, *w3;
    float *freq_cis_real, *freq_cis_imag;
    Typed_Tensor *token_classifier;
} LLM_Param;

typedef struct {                 /* only `logits` is a live host buffer here */
    float *xbuf; int8_t *qvbuf; float *qsbuf; float *kvcache;
    float *x, *xb, *xba, *xb2, *hb, *hb2;
    Typed_Tensor xq, xbaq, hq;
    float *q, *k, *v, *k_cache, *v_cache, *att;
    float *logits;
    float *q0, *k0, *v0, *o0, *q1, *k1, *v1, *o1;
} FwdBuffer;

typedef struct {
    LLM_Config config;
    LLM_Param params;
    FwdBuffer state;
    uint32_t arch;
    uint32_t quant_type;
    uint32_t group_size;
    int fd;
    uint8_t *buffer;
    size_t file_size;
} LLM;

typedef struct { uint32_t lora_rank, lora_alpha, n_layer, n_embd, n_head, n_kv_head, n_hidden, lora_config; } LoRA_Config;
typedef struct { float *wq_lora_a, *wq_lora_b, *wk_lora_a, *wk_lora_b, *wv_lora_a, *wv_lora_b, *wo_lora_a, *wo_lora_b; } LoRA_Param;
typedef struct { LoRA_Config config; LoRA_Param params; float *data; } LoRA;

typedef struct { float prob; int index; } ProbIndex;

typedef struct {
    int vocab_size;
    ProbIndex *probindex;
    float repetition_penalty;
    float temperature;
    float top_p;
    uint32_t top_k;
    uint64_t rng_state;
} Sampler;

typedef struct Nano_Context {
    LLM *llm;
    LoRA *lora;
    Tokenizer *tokenizer;
    Sampler *sampler;
    uint32_t max_seq_len;
    uint64_t random_seed;
    void (*observation)(Nano_Observation obs, void *env);   /* may be NULL here (the reference requires non-NULL) */
    void *observation_env;
} Nano_Context;

typedef struct Nano_Session {
    wchar_t *prompt;
    uint32_t num_prompt_tokens;
    uint32_t max_seq_len;
    uint32_t *output_ids;
    uint32_t output_count;
    wchar_t *output_text;
    uint32_t next_token;
    uint32_t pos;
    int32_t is_prefilling;
    uint64_t t_0, t_1;
    float tps;
} Nano_Session;

/* ---- the reference's exported engine API (reference infer/infer.h:253-282), same semantics ---------- */
void load_llm_from_buffer(LLM *llm, Tokenizer *tk, uint8_t *buffer, uint32_t max_seq_len);
void load_llm(LLM *llm, Tokenizer *tk, char *model_path, uint32_t max_seq_len);
Sampler *build_sampler(int vocab_size, float repetition_penalty, float temperature, float top_p, uint32_t top_k, uint64_t rng_seed);
LoRA *load_lora_from_buffer(LLM *llm, uint8_t *buffer);
LoRA *load_lora(LLM *llm, char *lora_path);

Nano_Context *llm_context_init_from_buffer(uint8_t *buffer, uint32_t max_seq_len, float repetition_penalty, float temperature, float top_p, uint32_t top_k, uint64_t random_seed);
Nano_Context *llm_context_init(char *model_path, char *lora_path, uint32_t max_seq_len, float repetition_penalty, float temperature, float top_p, uint32_t top_k, uint64_t random_seed);
void llm_context_free(Nano_Context *ctx);

uint32_t generate_next_token(Nano_Context *ctx, uint32_t *output_ids, uint32_t pos, int is_prefilling);

Nano_Session *llm_session_init(Nano_Context *ctx, wchar_t *prompt, uint32_t max_seq_len, int32_t is_thinking_enabled);
int32_t llm_session_step(Nano_Context *ctx, Nano_Session *session);
void llm_session_free(Nano_Session *session);

int32_t generate_sync(Nano_Context *ctx, wchar_t *prompt, uint32_t max_seq_len,
                      int32_t (*on_prefilling)(Nano_Session *), int32_t (*on_decoding)(Nano_Session *),
                      int32_t (*on_finished)(Nano_Session *));
void seq2seq(Nano_Context *ctx, wchar_t *input_list, wchar_t *output_list, uint32_t max_seq_len);

void free_lora(LLM *llm, LoRA *lora);
void free_llm(LLM *llm, Tokenizer *tk);
void free_sampler(Sampler *sampler);

/* exported by the reference without a prototype (infer/infer.c:971) -- the inner seam */
float *llm_forward(Nano_Context *ctx, uint32_t token, uint32_t pos, uint32_t max_seq_len, uint32_t is_causal, LLM *llm, LoRA *lora);

/* ---- new surface (absent in the reference; SURVEY 8b "New surface needed") -------------------------- */
/* GPU used by contexts created afterwards (default 0, or env NANO_HIP_DEVICE). */
void nano_set_device(int device);
/* Number of independent sequence slots (KV caches) contexts created afterwards get (default 1). */
void nano_set_max_batch(uint32_t max_batch);
/* One decode step for `batch` independent sequences of one context: slot i feeds tokens[i] at pos[i].
 * logits (batch*vocab floats) and argmax (batch ids) may each be NULL.  Returns 0 or a negative
 * NANO_HIP_E* code (nano_mi355x.h). */
int nano_forward_batch(Nano_Context *ctx, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                       float *logits, uint32_t *argmax);
/* One decode step of `batch` sequences (slot i = sequence i, as nano_forward_batch) sampled with each sequence's
 * own Sampler: out_ids[i] is the token generate_next_token would return for that sequence's logits.  histories[i] holds the
 * n_history[i] ids the repetition penalty marks (histories / n_history may be NULL: no history).  Each sampler's coin comes from its
 * own rng_state, drawn only when its temperature is not 0.  The rows are sampled on the device; rows it declines, and every row under
 * NANO_HOST_SAMPLER=1, go through the host loops.  With replicas, each replica's share is served by its own batched call, one replica
 * after another (not concurrently).  Returns 0 or a negative NANO_HIP_E* code.
 * Sampler.top_k is stored and ignored here and in generate_next_token, as in the reference.  With NANO_SAMPLE_TOP_K=1 in the
 * environment (read once) both pass it to the device sampler and the host loops apply the same truncation: the sorted candidates are
 * cut to the first top_k in front of the top-p cut (nano_mi355x.h, "top-k truncation"); top_k == 0 stays off. */
int nano_forward_batch_sample(Nano_Context *ctx, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                              Sampler *const *samplers, const uint32_t *const *histories, const uint32_t *n_history,
                              uint32_t *out_ids);
/* Logit edits (nano_mi355x.h, "logit edits"): an allowed-token mask (ceil(V / 32) words, bit (j & 31) of word (j >> 5) allows token j,
 * NULL = every token) and a bias list (n_bias <= NANO_BIAS_MAX distinct tokens with their biases), applied in front of the pick:
 * l' = allowed ? l + bias : -inf, and a disallowed token is never a candidate, so the returned id is always an allowed one.
 * nano_set_logit_edit copies `edit` into the context (NULL clears it); it then applies to the decode branch of generate_next_token,
 * and therefore to sessions and generate_sync; prompt positions are unaffected.  With an edit set the greedy branch (temperature 0,
 * penalty 1) goes through the device sampler as a temperature-0 row, not through the arg-max of the forward or the lookup-draft loop.
 * The host loops (per-phase observation, NANO_HOST_SAMPLER=1, rows the device declines) apply the same edit and the same candidate
 * filter: device and host agree id for id.  Without an edit every path is what it was.  Returns 0, or NANO_HIP_EINVAL for an edit the
 * device sampler would refuse (no allowed token, too many / duplicate / out-of-vocabulary bias tokens, a NaN or +inf bias).
 * nano_forward_batch_sample_edit is nano_forward_batch_sample with edits[i] for sequence i (`edits` NULL: no edits; an entry with a
 * NULL mask and n_bias 0: none for that sequence); nano_forward_batch_sample is this call with edits = NULL. */
typedef struct NanoLogitEdit { const uint32_t *allow; const uint32_t *bias_tokens; const float *bias_values; uint32_t n_bias; } NanoLogitEdit;
int nano_set_logit_edit(Nano_Context *ctx, const NanoLogitEdit *edit);
int nano_forward_batch_sample_edit(Nano_Context *ctx, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                   Sampler *const *samplers, const uint32_t *const *histories, const uint32_t *n_history,
                                   const NanoLogitEdit *edits, uint32_t *out_ids);
/* Ingest prefix_ids[0..n_prefix) once per device and make it the first n_prefix positions of sequences 0..batch-1 of the
 * context (the sequences nano_forward_batch addresses): N continuations of one prompt, or N questions behind one instruction
 * prefix, pay the prompt once.  With replicas (sequence i -> replica i mod G, slot i / G) each replica ingests the prefix into
 * its slot 0 and forks it into the other slots of its share (nano_hip_kv_fork, nano_mi355x.h: a copy, or shared pages on a paged
 * cache).  Applies the context's LoRA selection as nano_forward_batch does.  Returns 0 or a NANO_HIP_E* code. */
int nano_prefill_shared(Nano_Context *ctx, const uint32_t *prefix_ids, uint32_t n_prefix, uint32_t batch);
/* Park a sequence's KV rows in host memory and bring them back (KV images, nano_mi355x.h: the format, and what save and restore
 * promise, are stated there).  `slot` is a slot of the context's device model -- sequence i of nano_forward_batch lives in slot i, a
 * session in slot 0.  nano_kv_image_bytes = the size of the image of n_pos positions (0 for a context without a device model);
 * nano_kv_save writes it into buf[0..cap) and its size into *bytes; nano_kv_restore makes positions 0 .. n_pos-1 of `slot` those of
 * the image (n_pos = UINT32_MAX: all of it), in this process or in another that opened the same model file: the continuation is bit
 * for bit the uninterrupted one.  Contexts with replicas are not offered: both return NANO_HIP_EINVAL there (a sequence's slot is on
 * one of several devices).  Not offered either: format conversion, ranges that do not start at position 0, an asynchronous call, file
 * I/O or compression, several slots at once (restore, then nano_hip_kv_fork).  Returns 0 or a NANO_HIP_E* code. */
size_t nano_kv_image_bytes(Nano_Context *ctx, uint32_t n_pos);
int nano_kv_save(Nano_Context *ctx, uint32_t slot, uint32_t n_pos, void *buf, size_t cap, size_t *bytes);
int nano_kv_restore(Nano_Context *ctx, uint32_t slot, const void *buf, size_t bytes, uint32_t n_pos);
/* LoRA table (nano_mi355x.h, "LoRA table"): several modules of one base model resident at once and a binding sequence -> module, so that
 * one nano_forward_batch* step (or nano_prefill_shared, nano_forward_batch_sample*, nano_forward_batch_topk) serves sequences with
 * different adapters from ONE read of the base weights.  nano_lora_table_load reads a module file of load_lora's format into entry id (<
 * 64) and applies load_lora's check that the module fits the base model; _from_buffer takes the file's bytes (copied: the buffer may go).
 * nano_lora_table_free empties an entry (refused while a slot is bound to it).  nano_lora_bind: slots[i] -- sequence i of
 * nano_forward_batch lives in slot i, a session in slot 0 -- takes entry ids[i], or none (0xffffffff, NANO_LORA_NONE).  Bind a slot
 * before its sequence's first token and keep the binding while the sequence lives: its K / V rows carry that module's deltas.
 * The reference's load_lora / free_lora / llm_forward(..., lora) keep their single-module meaning and do not mix with a table: on a
 * model with a loaded module the table calls return NANO_HIP_EINVAL, and load_lora on a model with a table fails as every load_lora
 * failure does.  llm_forward with lora = NULL on a model with a table applies slot 0's binding.  Not offered: replicas (with replicas
 * attached the table calls return NANO_HIP_EINVAL, and nano_context_replicate refuses a context with a table), the ragged calls
 * (nano_prefill_batch, nano_embed_batch: NANO_HIP_EINVAL as with a module), Qwen architectures.  Returns 0 or a NANO_HIP_E* code: an
 * unreadable file and a module that does not fit are NANO_HIP_EINVAL. */
int nano_lora_table_load(Nano_Context *ctx, uint32_t id, const char *path);
int nano_lora_table_load_from_buffer(Nano_Context *ctx, uint32_t id, const uint8_t *buffer, size_t bytes);
int nano_lora_table_free(Nano_Context *ctx, uint32_t id);
int nano_lora_bind(Nano_Context *ctx, const uint32_t *slots, const uint32_t *ids, uint32_t n);
/* Ingest `batch` prompts at once: sequence i (the sequences nano_forward_batch addresses) takes prompts[i][0..n_tokens[i]) from position
 * 0, and first_ids[i] (optional, batch words) is the arg-max behind its last token -- the first id of a greedy continuation (an empty
 * prompt leaves first_ids[i] untouched).  One ragged step per device (nano_hip_step_rows, nano_mi355x.h): the prompts share the weight
 * reads, and each sequence's rows are those of its own batched prefill.  With replicas (sequence i -> replica i mod G, slot i / G) each
 * replica's share is one call, one replica after another.  The ragged step has no LoRA branches: with a module selected the call
 * returns NANO_HIP_EINVAL.  Returns 0 or a NANO_HIP_E* code; a refused call feeds nothing on the device that refused. */
int nano_prefill_batch(Nano_Context *ctx, const uint32_t *const *prompts, const uint32_t *n_tokens, uint32_t batch, uint32_t *first_ids);
/* Text embeddings of `batch` texts in one ragged step (nano_hip_step_rows_pool, nano_mi355x.h: the float chains, the order of every sum
 * and what strict / exact mode return are stated there): sequence i takes texts[i][0..n_tokens[i]) from position 0, as in
 * nano_prefill_batch, and out[i * d .. (i + 1) * d) with d = dim ? dim : n_embd is its vector: the final-norm hidden state of its last
 * token (pooling = NANO_POOL_LAST, what an embedding checkpoint of the Qwen3 family is trained for) or the mean over its tokens
 * (NANO_POOL_MEAN), cut to its leading dim components, then -- normalize = 1 -- scaled to unit length.  An empty text gets zeros.  No
 * classifier runs and no logit exists.  The sequences are left ingested: a caller may go on decoding from them with nano_forward_batch.
 * Runs on the context's own device: with replicas attached the call returns NANO_HIP_EINVAL, as it does with a LoRA module selected
 * (the ragged step has no LoRA branches), for batch == 0 or beyond the device's slots, and for whatever the backend call refuses.
 * Not offered: bidirectional attention (is_causal = 0), CLS pooling, texts longer than max_seq_len.  Returns 0 or a NANO_HIP_E* code. */
int nano_embed_batch(Nano_Context *ctx, const uint32_t *const *texts, const uint32_t *n_tokens, uint32_t batch, uint32_t pooling,
                     uint32_t normalize, uint32_t dim, float *out);
/* Greedy decode of `batch` sequences with lookup drafts, one ragged verify pass per round (nano_hip_decode_lookup_rows, nano_mi355x.h:
 * what the ids are and how a round is built are stated there).  Sequence i lives in slot i, as in nano_forward_batch: the slot holds
 * positions 0 .. n_history[i]-2 of histories[i], the history's last id is fed first, at most max_new[i] ids go to out_ids[i] and their
 * count to n_out[i].  max_draft 0 .. 15 (clipped by the device entry's rule), n-grams of 1 .. 3 ids as nano_set_lookup_draft uses,
 * stop_token UINT32_MAX = none.  Runs on the context's own device: with replicas attached or a LoRA module selected the call returns
 * NANO_HIP_EINVAL, as it does for whatever the device entry refuses.  Not offered: a draft model, sampling, logit edits.  Returns 0
 * or a NANO_HIP_E* code. */
int nano_decode_batch_lookup(Nano_Context *ctx, const uint32_t *const *histories, const uint32_t *n_history, const uint32_t *max_new,
                             uint32_t batch, int max_draft, uint32_t stop_token, uint32_t *const *out_ids, uint32_t *n_out);
/* Feed ids[0..n_ids-1) into sequence 0 from position 0 and score ids[1..n_ids): logprobs / argmax hold n_ids-1 entries (either may be NULL),
 * *nll_sum = -(sum of the logprobs), added in double in index order.  Applies the context's LoRA selection as nano_forward_batch does.
 * logprobs[i] = log p(ids[i + 1] | ids[0..i]) and argmax[i] = the model's own choice there, both taken on the device from a batched
 * prefill whose logits never reach the host (nano_hip_prefill_score, nano_mi355x.h); perplexity = exp(nll_sum / (n_ids - 1)).
 * Uses the context's own device, not its replicas; n_ids < 2 scores nothing and returns 0.  Returns 0 or a NANO_HIP_E* code. */
int nano_score_ids(Nano_Context *ctx, const uint32_t *ids, uint32_t n_ids, float *logprobs, uint32_t *argmax, double *nll_sum);
/* nano_score_ids plus the alternatives the model weighed at every scored position: top_ids / top_logprobs hold (n_ids - 1) * k entries
 * (either may be NULL, not both), position after position, most probable first -- the `top_logprobs` of a serving front end, selected on the
 * device (nano_hip_prefill_score_topk, nano_mi355x.h: order, ties and bits are stated there).  1 <= k <= min(32, vocab), else
 * NANO_HIP_EINVAL.  logprobs, argmax and *nll_sum are nano_score_ids's, bit for bit. */
int nano_score_ids_topk(Nano_Context *ctx, const uint32_t *ids, uint32_t n_ids, uint32_t k, float *logprobs, uint32_t *argmax,
                        uint32_t *top_ids, float *top_logprobs, double *nll_sum);
/* One decode step for `batch` sequences as nano_forward_batch (same sequence -> (replica, slot) map), handing back per sequence its k
 * most probable next ids and their log-probs (batch * k entries each; either may be NULL, not both) and its arg-max (may be NULL) instead
 * of batch * vocab logits (nano_hip_forward_topk).  With replicas, each replica's share is served by its own call, one replica after
 * another (not concurrently, unlike nano_forward_batch).  1 <= k <= min(32, vocab).  Returns 0 or a negative NANO_HIP_E* code. */
int nano_forward_batch_topk(Nano_Context *ctx, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, uint32_t k,
                            uint32_t *top_ids, float *top_logprobs, uint32_t *argmax);
/* Replicas of the context's model on the listed further GPUs of the node, in this process: nano_forward_batch then serves
 * sequence i from replica i mod (1 + n_devices) (replica 0 = the context's own device) and the replicas decode their
 * shares concurrently -- independent sequences shard trivially, no collective.  The one-process-per-GPU
 * route with an RCCL broadcast of the weights is nano_amd/dist.py + bench.py.  Returns 0 or a NANO_HIP_E* code. */
int nano_context_replicate(Nano_Context *ctx, const int *devices, int n_devices);
/* how the last nano_context_replicate moved the weights (one host upload + an RCCL broadcast / peer copies over xGMI, replicate.hip) */
int nano_replicate_stats(Nano_Context *ctx, double *upload_s, double *share_s, char *how, size_t how_cap);
/* Session over token ids (no tokenizer needed): like llm_session_init but the prompt is given as ids. */
Nano_Session *nano_session_init_ids(Nano_Context *ctx, const uint32_t *prompt_ids, uint32_t n_prompt, uint32_t max_seq_len);
/* Like llm_session_step but never touches the tokenizer (output_text stays NULL). */
int32_t nano_session_step_ids(Nano_Context *ctx, Nano_Session *session);
/* Per-phase observation (debug aid).  The reference fires ctx->observation eight times per layer and three times per
 * token from inside llm_forward (infer/infer.c:755-949, 985-1003; consumer infer/ui_llm.c:695-706).  The fused device
 * forward has no host boundary between phases, so by default the hook fires at token granularity (EMBEDDING,
 * FINAL_NORM, CLASSIFY, SAMPLE).  nano_set_phase_observation(1) (or NANO_OBSERVE_PHASES=1 in the environment) makes
 * the forwards of contexts that have a hook installed run the backend's eager per-operator replay (strict mode of
 * nano_mi355x.h): all twelve phases fire in the reference's order with that phase's tensors finished on the device,
 * the sampler runs in host C on the returned logits.  Slow; never on a timed path. */
void nano_set_phase_observation(int on);
/* Greedy decode with lookup drafts (nano_mi355x.h nano_hip_decode_lookup), opt-in: with max_draft = 1 .. 15 (or NANO_LOOKUP_DRAFT=n in the
 * environment, read once) the greedy branch of generate_next_token (temperature 0, repetition penalty 1, no per-phase observation) runs
 * one step of that loop per call with ngram 1 .. 3: a verify chunk's confirmed ids beyond the returned one are queued, and the following
 * calls whose (pos, output_ids[pos]) continue them return from the queue without device work.  Any other call drops the queue.  The
 * ids are nano_hip_decode_lookup's (see there for what that promises on wide matrices).  0 = today's path. */
void nano_set_lookup_draft(int max_draft);
/* Greedy decode with a draft model (nano_mi355x.h nano_hip_decode_draft), opt-in: with a model file's path and max_draft = 1 .. 15 (or
 * NANO_DRAFT_MODEL=<path> together with NANO_DRAFT_LEN=n in the environment, read once) the greedy branch of generate_next_token runs one
 * round of that loop per call: the draft model's ids are verified by one chunk of the model, and the confirmed ids beyond the returned one
 * go into the queue of the lookup drafts above, with the same rules.  Where both switches are set the draft model is used.  The draft is
 * opened on the first such call of each model, on that model's device and with its max_seq_len; the engine remembers which ids the draft
 * holds and feeds it the rest of output_ids itself.  A draft whose vocabulary size differs is refused when it is opened, with a message
 * on stderr (generate_next_token then exits, as it does when an upload fails).  The ids are nano_hip_decode_draft's: the model's own
 * greedy ids whatever the draft is.  path = NULL or max_draft = 0 switches it off.  Returns 0, or NANO_HIP_EINVAL for a max_draft outside
 * 1 .. 15 or an unusable path (the switch is then off). */
int nano_set_draft_model(const char *path, int max_draft);
/* Opens ctx's model's draft now instead of on first use: 0, or the NANO_HIP_E* code of what refused it (message on stderr). */
int nano_draft_model_open(Nano_Context *ctx);
/* Opaque device model behind an LLM (NanoHipModel*, nano_mi355x.h) for measurement tools. */
void *nano_device_model(const LLM *llm);

#ifdef __cplusplus
}
#endif
#endif /* NANO_INFER_ABI_H */
