/*
 * reprover_hip.h — C ABI of libreprover_hip.so, the MI355X (gfx950) premise-retrieval engine.
 *
 * Drop-in boundary for the hot path of lean-dojo/ReProver named by BASELINE.json:north_star:
 *   retrieval/model.py::PremiseRetriever (_encode :92-114, reindex_corpus :183-210,
 *   retrieve :338-375, predict hooks :274-336), common.py::Corpus.get_nearest_premises :299-326,
 *   retrieval/index.py :13-41.
 * The reference has no native code and no FFI of its own: it calls HuggingFace `transformers`
 * (T5EncoderModel) and torch ops from Python.  These entry points are what a ctypes/cffi stub
 * on the reference side binds instead (INTEGRATION.md shows the stub); the Python package
 * `reprover_amd` is exactly such a stub plus the host-side mirror of the reference classes.
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs; no torch / HIP C++ types.  `stream` is a
 *     hipStream_t passed as void* (NULL = the legacy default stream).
 *   - every pointer documented "device" must be a HIP device pointer valid on the current device.
 *   - every call returns an RpStatus (0 = OK, < 0 = error); rp_last_error() gives the message
 *     of the last failing call on the calling thread.
 *   - launches are asynchronous on `stream`; no call synchronises the device unless documented.
 *   - no hidden allocations after rp_encoder_create(); scratch comes from caller workspaces sized
 *     by the matching *_workspace_bytes() function.
 *   - a workspace's contents on entry are arbitrary: no call reads a workspace byte that the same call has not written
 *     (the two documented hand-overs aside: rp_train_backward reads what rp_train_forward left, the decoder steps
 *     read the cross K/V and the cache rows that earlier calls wrote).  workspace_bytes smaller than the matching
 *     *_workspace_bytes() returns RP_E_WORKSPACE and nothing is launched or written.
 *   - nothing outside [workspace, workspace + workspace_bytes) and the documented outputs is written, and nothing
 *     outside the documented extent of an input is read.  Where an output is written only in part (the padding gaps
 *     of the flat gradient buffers), its description says so.
 */
#ifndef REPROVER_HIP_H
#define REPROVER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t RpStatus;
enum {
  RP_OK = 0,
  RP_E_INVALID = -1,      /* bad argument / unsupported shape                                   */
  RP_E_HIP = -2,          /* a HIP runtime call failed                                          */
  RP_E_WORKSPACE = -3,    /* caller workspace too small                                         */
  RP_E_UNSUPPORTED = -4,  /* model configuration outside what the kernels implement             */
  RP_E_COMM = -5          /* RCCL could not be bound, or one of its calls failed                */
};

enum { RP_DT_F32 = 0, RP_DT_BF16 = 1 };

/* ABI / build identification; bumps when a signature changes. */
int32_t rp_abi_version(void);   /* 7 */
/* Message of the last error returned on this thread ("" if none). */
const char* rp_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Encoder: T5EncoderModel forward + masked mean-pool + L2 normalise
 *   replaces retrieval/model.py:92-114 (_encode) and, beneath it, transformers
 *   models/t5/modeling_t5.py T5Stack.forward :663-750 (what model.py:44-45,101-105 invoke).
 * ------------------------------------------------------------------------------------------- */
typedef struct RpT5Config {
  int32_t vocab_size;      /* rows of the embedding table (384 for ByT5)                        */
  int32_t d_model;         /* 1472 (small) / 1536 (base); must be a multiple of 32              */
  int32_t d_kv;            /* per-head width; kernels implement 64                              */
  int32_t num_heads;       /* 6 / 12                                                            */
  int32_t d_ff;            /* 3584 / 3968; multiple of 32; feed_forward_proj = gated-gelu       */
  int32_t num_layers;      /* 12 / 18                                                           */
  int32_t rel_num_buckets; /* 32                                                                */
  int32_t rel_max_distance;/* 128                                                               */
  float   layer_norm_eps;  /* 1e-6                                                              */
} RpT5Config;

/* Weights in HuggingFace layout (nn.Linear = [out, in] row-major), all device pointers of dtype
 * `weight_dtype` (RP_DT_F32 or RP_DT_BF16); key names: SURVEY.md App. B.5.  The engine packs its
 * own bf16 copies (fused QKV, gate/up-interleaved wi, padded) at create time; the caller may free
 * the originals afterwards. */
typedef struct RpT5LayerWeights {
  const void* ln_attn;   /* encoder.block.i.layer.0.layer_norm.weight          [d_model]         */
  const void* q;         /* ...layer.0.SelfAttention.q.weight                  [H*d_kv, d_model] */
  const void* k;         /* ...k.weight                                        [H*d_kv, d_model] */
  const void* v;         /* ...v.weight                                        [H*d_kv, d_model] */
  const void* o;         /* ...o.weight                                        [d_model, H*d_kv] */
  const void* ln_ff;     /* ...layer.1.layer_norm.weight                       [d_model]         */
  const void* wi_0;      /* ...layer.1.DenseReluDense.wi_0.weight              [d_ff, d_model]   */
  const void* wi_1;      /* ...wi_1.weight                                     [d_ff, d_model]   */
  const void* wo;        /* ...wo.weight                                       [d_model, d_ff]   */
} RpT5LayerWeights;

typedef struct RpT5Weights {
  const void* embed;            /* shared.weight                               [vocab, d_model]  */
  const void* rel_bias;         /* block.0 relative_attention_bias.weight      [buckets, H]      */
  const void* final_ln;         /* encoder.final_layer_norm.weight             [d_model]         */
  const RpT5LayerWeights* layers; /* host array of num_layers entries                           */
} RpT5Weights;

typedef struct RpEncoder RpEncoder;

/* Allocates and packs device weights (synchronises the device once). */
RpStatus rp_encoder_create(const RpT5Config* cfg, const RpT5Weights* weights, int32_t weight_dtype,
                           RpEncoder** out);
void     rp_encoder_destroy(RpEncoder* enc);

/* Scratch needed by rp_encode_varlen for `total_tokens` packed tokens in `batch` sequences. */
size_t   rp_encoder_workspace_bytes(const RpEncoder* enc, int32_t total_tokens, int32_t batch);

/* Encode `batch` sequences given as packed token ids (varlen, no padding):
 *   ids        device int32 [total_tokens]  — ByT5 ids (byte+3, EOS=1 last), sequence b occupies
 *                                             [cu_seqlens[b], cu_seqlens[b+1])
 *   cu_seqlens device int32 [batch+1], cu_seqlens[0] = 0, cu_seqlens[batch] = total_tokens
 *   max_len    longest sequence (host value; sizes the attention grid)
 *   out        device [batch, d_model] of out_dtype (RP_DT_F32 / RP_DT_BF16): unit-norm rows,
 *              = F.normalize(masked_mean(last_hidden_state))  (model.py:108-114)
 * Equivalent to PremiseRetriever._encode(input_ids, attention_mask) with right-padded inputs:
 * padding never influences a row, so it is not materialised. */
RpStatus rp_encode_varlen(RpEncoder* enc, const int32_t* ids, const int32_t* cu_seqlens,
                          int32_t batch, int32_t total_tokens, int32_t max_len,
                          void* out, int32_t out_dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The reference's own call form: PremiseRetriever._encode(input_ids, attention_mask) (retrieval/model.py:92-114)
 * on a right-padded batch as the tokenizer / datamodule.py:130-144 collate produce it.
 *   input_ids       device int64 [batch, padded_len]
 *   attention_mask  device int64 [batch, padded_len]   1 on real tokens, then 0
 *   out             device [batch, d_model] of out_dtype, as rp_encode_varlen
 *   meta            device int32 [4], written asynchronously: meta[0] = total real tokens, meta[1] = longest
 *                   sequence, meta[2] != 0 when some row is NOT right-padded (ones after a zero) or is empty -
 *                   `out` is then meaningless and the caller must raise (read it at its next synchronisation).
 * Lengths, cu_seqlens and the packed ids are derived on the device (no host round trip, no torch kernels); the
 * encoder pass is launched for the upper bound batch * padded_len tokens and skips, on the device, every tile
 * beyond the real count.  Results are bit-identical to rp_encode_varlen on the packed form of the same batch. */
size_t   rp_encode_padded_workspace_bytes(const RpEncoder* enc, int32_t batch, int32_t padded_len);
RpStatus rp_encode_padded(RpEncoder* enc, const int64_t* input_ids, const int64_t* attention_mask,
                          int32_t batch, int32_t padded_len, void* out, int32_t out_dtype, int32_t* meta,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Host-only helper, exact restatement of T5Attention._relative_position_bucket (bidirectional)
 * — modeling_t5.py:216-262; exported so the bucket table can be checked without a GPU. */
int32_t  rp_relative_position_bucket(int32_t relative_position, int32_t num_buckets,
                                     int32_t max_distance);

/* ---------------------------------------------------------------------------------------------
 * Retrieval: similarity GEMM + accessibility mask + exact top-k
 *   replaces common.py:299-326 (Corpus.get_nearest_premises): `Q @ E.T`, full argsort, and the
 *   per-query Python walk over accessible premises.
 *
 * Accessibility in array form (common.py:280-289; derivation SURVEY.md §8 a6'):
 *   premise i is accessible to query j  iff
 *       bit j of file_bits_t[file_of[i]]                       (file imported, transitively)
 *    or (file_of[i] == own_file[j] and end_key[i] <= q_key[j]) (earlier in the same file)
 *   with key = (line_nb << 20) | column_nb.  Passing file_of == NULL disables the mask.
 * Ordering: (score descending, id ascending) — the reference's argsort leaves ties unspecified.
 * ------------------------------------------------------------------------------------------- */
enum { RP_TOPK_AUTO = 0, RP_TOPK_DENSE = 1 /* force the single-pass dense path */ };

/* D = the embedding width for BOTH entry points (the e4m3 one plans with half the 2-byte units per row; its plan can
 * only differ by taking the first-generation filter kernel, which needs no more workspace than this returns; it
 * still asks for this size, so that one rule - workspace_bytes >= what this returns - holds for all four calls). */
size_t   rp_sim_topk_workspace_bytes(int32_t B, int32_t N, int32_t D, int32_t k, int32_t flags);

/*   Q            device bf16 [B, D]   query embeddings (unit norm)
 *   E            device bf16 [N, D]   this rank's rows of the premise-embedding matrix
 *   file_of      device int32 [N]     file index of each premise           (NULL = no mask)
 *   end_key      device int64 [N]     end position key of each premise
 *   file_bits_t  device uint32 [F, ceil(B/32)]  bit j of row f = query j may use file f
 *   own_file     device int32 [B];  q_key device int64 [B]
 *   id_offset    added to local row numbers to form the ids written (row-sharded corpus)
 *   out_scores   device f32 [B, k];  out_ids device int32 [B, k]  (rows sorted best-first;
 *                entries past out_count[j] are -inf / -1)
 *   out_count    device int32 [B]: min(k, #accessible premises on this rank); the caller maps
 *                a global count < k to the reference's ValueError (common.py:323-324).
 *                -1 = "internal candidate overflow: call again with RP_TOPK_DENSE".  The two-pass plan keeps at most
 *                max(8192, 8 k stride) + k candidate keys per query (about k * stride lie above the sampled bound); a
 *                query that would need more - adversarial score distributions, or a sample with fewer than k accessible
 *                rows, which yields no bound - reports -1 and every caller repeats the search with the dense plan.
 *   k <= 1024 per call (the final selection sorts in LDS).  The reference accepts any k (common.py:299-326):
 *   rp_sim_topk_after continues the same ranking page by page, which is how the host shim serves k > 1024.    */
RpStatus rp_sim_topk(const void* Q, const void* E, int32_t B, int32_t N, int32_t D,
                     const int32_t* file_of, const int64_t* end_key,
                     const uint32_t* file_bits_t, int32_t F,
                     const int32_t* own_file, const int64_t* q_key,
                     int32_t id_offset, int32_t k, int32_t flags,
                     float* out_scores, int32_t* out_ids, int32_t* out_count,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The next page of rp_sim_topk's ranking: identical arguments plus, per query, the LAST entry of what the caller already
 * holds - after_score device f32 [B], after_id device int32 [B] (the id as written by the previous call, id_offset
 * included; after_id[j] < 0: no bound for query j).  Only premises that come strictly after (after_score[j], after_id[j])
 * in the (score descending, id ascending) order qualify; out_count counts those (min(k, remaining accessible)).  Pages
 * concatenate to exactly what one call with a larger k would return: the order is total (ids break ties).          */
RpStatus rp_sim_topk_after(const void* Q, const void* E, int32_t B, int32_t N, int32_t D,
                           const int32_t* file_of, const int64_t* end_key,
                           const uint32_t* file_bits_t, int32_t F,
                           const int32_t* own_file, const int64_t* q_key,
                           int32_t id_offset, const float* after_score, const int32_t* after_id,
                           int32_t k, int32_t flags,
                           float* out_scores, int32_t* out_ids, int32_t* out_count,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * e4m3 index (BASELINE.json configs[4]: fp8 similarity).  No reference counterpart: the reference
 * keeps the index in the model dtype (retrieval/model.py:190-194).  Rows are quantised one by one,
 *   scale[r] = max|x[r,:]| / 448 (1.0 for an all-zero row),
 *   q[r,c]   = round-to-nearest-even to OCP e4m3fn of x[r,c] * (448 / max|x[r,:]|),
 * and the score of (query j, premise i) is  (sum_c q8[j,c] * e8[i,c]) * q_scale[j] * e_scale[i]
 * with the sum accumulated in fp32 by the block-scaled MFMA (all block scales 2^0).  Mask, ordering,
 * outputs, workspace (rp_sim_topk_workspace_bytes) and flags are exactly rp_sim_topk's; D % 64 == 0.
 * ------------------------------------------------------------------------------------------- */
RpStatus rp_quantize_rows_e4m3(const void* X, int32_t x_dtype /* RP_DT_F32 | RP_DT_BF16 */, int64_t rows,
                               int32_t D, void* out_fp8 /* u8 [rows, D] */, float* out_scale /* [rows] */,
                               void* stream);
RpStatus rp_sim_topk_fp8(const void* Q8, const float* q_scale, const void* E8, const float* e_scale,
                         int32_t B, int32_t N, int32_t D,
                         const int32_t* file_of, const int64_t* end_key,
                         const uint32_t* file_bits_t, int32_t F,
                         const int32_t* own_file, const int64_t* q_key,
                         int32_t id_offset, int32_t k, int32_t flags,
                         float* out_scores, int32_t* out_ids, int32_t* out_count,
                         void* workspace, size_t workspace_bytes, void* stream);

RpStatus rp_sim_topk_fp8_after(const void* Q8, const float* q_scale, const void* E8, const float* e_scale,
                               int32_t B, int32_t N, int32_t D,
                               const int32_t* file_of, const int64_t* end_key,
                               const uint32_t* file_bits_t, int32_t F,
                               const int32_t* own_file, const int64_t* q_key,
                               int32_t id_offset, const float* after_score, const int32_t* after_id,
                               int32_t k, int32_t flags,
                               float* out_scores, int32_t* out_ids, int32_t* out_count,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Merge R per-rank results (as gathered by an RCCL all-gather) into the global top-k.
 *   scores device f32 [R, B, k], ids device int32 [R, B, k], counts device int32 [R, B]
 *   workspace: rp_topk_merge_workspace_bytes(R, B, k) bytes.                                   */
size_t   rp_topk_merge_workspace_bytes(int32_t R, int32_t B, int32_t k);
RpStatus rp_topk_merge(const float* scores, const int32_t* ids, const int32_t* counts,
                       int32_t R, int32_t B, int32_t k,
                       float* out_scores, int32_t* out_ids, int32_t* out_count,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same merge reading an all-gather's receive buffer as it lies: every rank sent ONE packed block
 *   [ scores f32 [Bt, k] | ids int32 [Bt, k] | counts int32 [Bt] ]      (Bt = all queries of the step)
 * so rank r's element [q, i] sits at base + r * rank_stride + q * k + i (4-byte units; rank_stride = Bt * (2 k + 1)) and
 * a rank merges only its own queries by passing pointers advanced to its first query (scores + q0 * k, ids + q0 * k,
 * counts + q0) with B = its number of queries.  No copy, no re-layout between the collective and the merge. */
RpStatus rp_topk_merge_strided(const float* scores, const int32_t* ids, const int32_t* counts, int64_t rank_stride,
                               int32_t R, int32_t B, int32_t k,
                               float* out_scores, int32_t* out_ids, int32_t* out_count,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The collective of the sharded retrieve step (one all-gather of the per-rank lists, then the
 * per-query merge).  The reference has no counterpart - it replicates the whole index per process
 * (retrieval/model.py:274-279, prover/proof_search.py:438-447); this is the exchange its row-sharded replacement needs,
 * behind the ABI so that a caller without torch.distributed can run it.
 *
 * RCCL is bound at run time (dlopen: a copy the process already holds, else librccl.so.1 on the search path, else
 * /opt/rocm/lib; RP_RCCL_LIB overrides); without it these calls return RP_E_COMM and everything else keeps working.
 * One communicator per (rank, GPU): rank 0 calls rp_comm_unique_id, the caller carries the 128 bytes to the other ranks
 * by whatever channel it has (a file, a socket, torch.distributed's store), every rank calls rp_comm_init with its
 * device current.  Calls are enqueued on `stream`; nothing synchronises; no allocation after rp_comm_init.
 * ------------------------------------------------------------------------------------------- */
#define RP_COMM_ID_BYTES 128
typedef struct RpComm RpComm;
RpStatus rp_comm_unique_id(void* id_out /* host, RP_COMM_ID_BYTES */);
RpStatus rp_comm_init(const void* unique_id, int32_t rank, int32_t world, RpComm** out);
RpStatus rp_comm_destroy(RpComm* comm);
int32_t  rp_comm_world(const RpComm* comm);
int32_t  rp_comm_rank(const RpComm* comm);
/* ncclAllGather of bytes_per_rank bytes (a multiple of 4) from every rank: recv = [world, bytes_per_rank], rank order.
 * Used as it stands for the query embeddings ([B, D] bf16 per rank) and for persisting a sharded index. */
RpStatus rp_comm_allgather(RpComm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
/* The step's exchange in one call: all-gather of this rank's packed block
 *   send_block  [ scores f32 [Bt, k] | ids int32 [Bt, k] | counts int32 [Bt] ]   (rp_sim_topk wrote into it in place)
 *   recv_blocks [world, Bt (2 k + 1)] 4-byte units
 * followed by rp_topk_merge_strided over queries [q0, q0 + B) read from recv_blocks as they lie -> out_* [B, k] / [B].
 * A rank whose count is -1 (candidate overflow, see rp_sim_topk) contributes nothing to the merge: the caller reads the
 * gathered counts (recv_blocks[r, 2 Bt k + q], identical on every rank) and, if any is negative, all ranks redo the step
 * with RP_TOPK_DENSE - what dist.PendingShardedSearch.finish does.
 * workspace: rp_topk_merge_workspace_bytes(world, B, k). */
RpStatus rp_allgather_topk(RpComm* comm, const void* send_block, void* recv_blocks, int32_t Bt, int32_t k,
                           int32_t q0, int32_t B, float* out_scores, int32_t* out_ids, int32_t* out_count,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Per-batch accessibility operand built on the device (replaces the host-side bit transposition of
 * common.py:280-289's closure for a batch): file_bits_t [F, ceil(B/32)] (as rp_sim_topk takes it) from
 *   reach     device uint64 [F, ceil(F/64)]   bit g of row f = file f imports file g (transitive closure, resident)
 *   own_file  device int32 [B]                the file each query's theorem lives in
 * so a search uploads 12 bytes per query (own_file, q_key). */
RpStatus rp_build_file_bits(const uint64_t* reach, int32_t F, const int32_t* own_file, int32_t B,
                            uint32_t* file_bits_t, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training forward, loss part: replaces retrieval/model.py:133-139
 *   similarity = torch.mm(context_emb, all_premise_embs.t());  loss = F.mse_loss(similarity, label)
 * (the embeddings come from rp_encode_padded / rp_encode_varlen with out_dtype RP_DT_F32).
 *   context_emb    device f32 [B, D];  premise_embs device f32 [P, D]  (P = B * (1 + num_negatives))
 *   label          device f32 [B, P]   (datamodule.py:160-175)
 *   out_loss       device f32 [1]: mean over the B x P entries of (similarity - label)^2, summed in index order
 *   out_similarity device f32 [B, P] or NULL
 * The encoder's backward is not part of this library; the two ends of the training step around it are:
 * ------------------------------------------------------------------------------------------- */
size_t   rp_contrastive_mse_workspace_bytes(int32_t B, int32_t P);
RpStatus rp_contrastive_mse(const float* context_emb, const float* premise_embs, const float* label,
                            int32_t B, int32_t P, int32_t D, float* out_loss, float* out_similarity,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Backward of that loss (what autograd does behind retrieval/model.py:137-139): with S = out_similarity of the forward,
 * dS = 2 (S - label) / (B P);  d_context_emb [B, D] = dS premise_embs;  d_premise_embs [P, D] = dS^T context_emb. */
RpStatus rp_contrastive_mse_backward(const float* context_emb, const float* premise_embs, const float* similarity,
                                     const float* label, int32_t B, int32_t P, int32_t D, float* d_context_emb,
                                     float* d_premise_embs, void* stream);
/* One torch.optim.AdamW update (/root/reference/common.py:395: `torch.optim.AdamW(parameters, lr=lr)`; decoupled
 * weight decay, bias-corrected moments) of n fp32 parameters, in place:  param, exp_avg, exp_avg_sq device f32 [n],
 * 16-byte aligned;  step = 1, 2, ...;  lr = base rate x the schedule's factor for this step
 * (get_constant_schedule_with_warmup: min(1, (step - 1) / warmup_steps)).  torch defaults: betas (0.9, 0.999),
 * eps 1e-8, weight_decay 1e-2.  The update is AdamW for exactly the C floats it receives (beta2 = 0.999 arrives as
 * 0.99900001287, and 1 - beta2, the bias corrections and 1 - lr * weight_decay are formed from that float); torch keeps
 * the betas in double and rounds 1 - beta2 on its own, so its exp_avg_sq differs from this one by 1.3e-5 relative at the
 * defaults - the bias correction absorbs it, the parameters agree to fp32 rounding (tests/test_step_ends_gpu.py). */
RpStatus rp_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                       float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step: replaces what autograd + Lightning do behind retrieval/model.py:155-181 (`training_step` differentiating
 * `forward` :116-140 through `_encode` :92-114 and transformers' T5Stack) and common.py:381-405 (`get_optimizers`).
 * Parameters, gradients and optimizer moments are FLAT fp32 device buffers in one canonical layout:
 *   embed [V, D] | rel_bias [buckets, H] | final_ln [D] | per layer: ln_attn [D], q, k, v [H*d_kv, D], o [D, H*d_kv],
 *   ln_ff [D], wi_0, wi_1 [d_ff, D], wo [D, d_ff]      (HF shapes; every tensor starts at a multiple of 64 elements)
 * rp_train_param_layout writes the rp_train_param_tensors(cfg) + 1 element offsets (last = total length incl. padding).
 * One step = rp_train_forward (all sequences of the batch - contexts, positives, negatives - packed as ONE varlen pass)
 *  -> rp_contrastive_mse (+ _backward) on the [batch, D] embeddings -> rp_train_backward -> rp_grad_norm (optional
 * clipping) -> rp_adamw_step over the flat buffers -> rp_trainer_load_params.  Dropout: rp_trainer_set_dropout (off by
 * default).  d_model and d_ff must be multiples of 64.
 * ------------------------------------------------------------------------------------------- */
typedef struct RpTrainer RpTrainer;
int32_t  rp_train_param_tensors(const RpT5Config* cfg);                 /* 3 + 9 * num_layers */
RpStatus rp_train_param_layout(const RpT5Config* cfg, int64_t* offsets /* [tensors + 1] */);
/* `params`: device f32 flat buffer in the layout above.  Allocates the bf16 compute copies (synchronises once). */
RpStatus rp_trainer_create(const RpT5Config* cfg, const float* params, RpTrainer** out);
void     rp_trainer_destroy(RpTrainer* tr);
/* The inference engine on the trainer's current weights (for rp_encode_varlen / rp_encode_padded: validation re-indexes
 * with the model being trained, retrieval/model.py:212-225); owned by the trainer. */
RpEncoder* rp_trainer_encoder(RpTrainer* tr);
/* Dropout of the following rp_train_forward / rp_train_backward pairs (T5's dropout_rate, 0.1 in the reference's training:
 * transformers modeling_t5.py :725 embeddings, :168/:360 attention probabilities, :400 / :140 the two residual branches, :110
 * inside the gated FFN, :745 after the final norm).  Counter-based: element (site, row, column) is kept iff the 16-bit field
 * (column & 1) of hash(seed, site, row, column >> 1) is >= round(p * 2^16), and scaled by 1 / (1 - p); the backward
 * regenerates the masks of the forward that ran with the same seed, nothing is stored.  p = 0 (the default) switches it off;
 * pass a fresh seed per step. */
RpStatus rp_trainer_set_dropout(RpTrainer* tr, float p, uint32_t seed);
/* Refresh every compute copy from the fp32 masters (call after each optimizer step); launch-only. */
RpStatus rp_trainer_load_params(RpTrainer* tr, const float* params, void* stream);
size_t   rp_train_workspace_bytes(const RpTrainer* tr, int32_t total_tokens, int32_t batch);
/* Forward over `batch` packed sequences (ids / cu_seqlens as rp_encode_varlen); out_emb device f32 [batch, d_model] =
 * _encode's unit-norm rows; the activations the backward needs stay in `workspace`, which must be handed unchanged to
 * rp_train_backward. */
RpStatus rp_train_forward(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                          int32_t total_tokens, float* out_emb, void* workspace, size_t workspace_bytes, void* stream);
/* d_emb device f32 [batch, d_model] = d loss / d out_emb;  grads: flat f32 buffer, every element overwritten with
 * d loss / d parameter (padding gaps untouched: zero them once).  Deterministic: no floating-point atomics on HBM. */
RpStatus rp_train_backward(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens,
                           int32_t batch, int32_t total_tokens, const float* d_emb, float* grads,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The same forward and backward with last_hidden_state as the hand-over instead of the pooled embedding: the encoder half
 * of the seq2seq loss's gradient (generation/model.py:117-121 through T5ForConditionalGeneration; the decoder half is
 * rp_decoder_loss_grad, whose d_enc is this pair's d_hidden).  The layer loops are the pooled pair's; only the head differs
 * (the final RMSNorm alone).  Same workspace (rp_train_workspace_bytes), same determinism.
 * rp_train_forward_hidden: the trainer's forward up to and including the final RMSNorm.  out_hidden: device bf16
 * [total_tokens, d_model] = bf16(final_ln * (x * rs)), fp32 arithmetic and one rounding; the activations stay in `workspace`
 * for rp_train_backward_hidden.  cu_seqlens is read back once before anything is launched (the one synchronisation of
 * `stream` in this pair): it must run 0 .. total_tokens and an empty sequence is RP_E_INVALID.
 * rp_train_backward_hidden: d_hidden: device f32 [total_tokens, d_model] = d loss / d out_hidden, unrounded (e.g.
 * rp_decoder_loss_grad's d_enc); grads: the trainer's flat layout, every element overwritten, gaps untouched; ids and
 * cu_seqlens are the forward's (not checked again).
 * Both return RP_E_INVALID while rp_trainer_set_dropout holds p > 0 (what follows them must drop too: a half-dropped
 * model is neither the reference's training mode nor its eval mode), for a null pointer and for batch <= 0;
 * RP_E_WORKSPACE for a workspace one byte short.  Nothing is launched or written then.
 * rp_train_forward_hidden_dropout / rp_train_backward_hidden_dropout: the same pair, same arguments, honouring
 * rp_trainer_set_dropout: the layer loops drop at HF's sites as rp_train_forward does, and the final site
 * (RP_DROP_SITE_FINAL) masks out_hidden = bf16(mask * final_ln * (x * rs)) and, in the backward, d_hidden before anything
 * else.  The decoder half is then rp_decoder_loss_grad_dropout with the same (p, seed).  With dropout unset they give the
 * plain pair's bits. */
RpStatus rp_train_forward_hidden(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                                 int32_t total_tokens, void* out_hidden_bf16, void* workspace, size_t workspace_bytes,
                                 void* stream);
RpStatus rp_train_backward_hidden(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens,
                                  int32_t batch, int32_t total_tokens, const float* d_hidden, float* grads,
                                  void* workspace, size_t workspace_bytes, void* stream);
RpStatus rp_train_forward_hidden_dropout(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                                         int32_t total_tokens, void* out_hidden_bf16, void* workspace,
                                         size_t workspace_bytes, void* stream);
RpStatus rp_train_backward_hidden_dropout(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens,
                                          int32_t batch, int32_t total_tokens, const float* d_hidden, float* grads,
                                          void* workspace, size_t workspace_bytes, void* stream);
/* out_norm[0] (device) = ||grads||_2 over n floats (Lightning's gradient_clip_val, confs/cli_lean4_random.yaml:19, clips
 * on it); scratch: 1024 device floats.  Pair with rp_adamw_step_clipped. */
RpStatus rp_grad_norm(const float* grads, int64_t n, float* out_norm, float* scratch, void* stream);
/* rp_adamw_step with the gradient scaled by min(1, max_norm / (total_norm[0] + 1e-6)) (torch.nn.utils.clip_grad_norm_);
 * total_norm: device f32 [1] from rp_grad_norm, or NULL for no clipping. */
RpStatus rp_adamw_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                               float lr, float beta1, float beta2, float eps, float weight_decay,
                               const float* total_norm, float max_norm, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-kernel timing with HIP events on the launch stream (used by bench.py for the roofline
 * object).  While enabled, every kernel launch of the engine is bracketed by an event pair.
 * ------------------------------------------------------------------------------------------- */
enum {
  RP_K_EMBED = 0, RP_K_RMSNORM = 1, RP_K_GEMM_QKV = 2, RP_K_ATTENTION = 3, RP_K_GEMM_O = 4,
  RP_K_GEMM_WI = 5, RP_K_GEMM_WO = 6, RP_K_POOL = 7, RP_K_SCAN = 8 /* dense / filter pass */, RP_K_SELECT = 9,
  RP_K_SCAN_SAMPLE = 10 /* sample pass of the two-pass plan */,
  /* training step (rp_train_*) */
  RP_K_BWD_DGRAD = 11 /* dY W GEMMs (+ fused GELU / RMSNorm backward) */, RP_K_BWD_WGRAD = 12 /* dY^T X GEMMs */,
  RP_K_BWD_ATTENTION = 13, RP_K_BWD_OTHER = 14 /* pooling, embedding, row statistics, gradient finishing */,
  RP_K_OPTIMIZER = 15 /* AdamW, gradient norm, weight re-packing */,
  RP_K_COLLECTIVE = 16 /* the all-gather of rp_comm_allgather / rp_allgather_topk */,
  RP_K_HIDDEN_HEAD = 17 /* rp_train_forward_hidden's final-norm rows */,
  RP_K_BWD_HIDDEN_HEAD = 18 /* rp_train_backward_hidden's final-norm backward (the row pass) */,
  RP_K_COUNT = 19
};
RpStatus rp_profile_enable(int32_t on);   /* on != 0: start collecting (clears previous records) */
/* Synchronises the recorded events; total_ms = sum of launch durations, launches = their number. */
RpStatus rp_profile_read(int32_t kernel_class, double* total_ms, int64_t* launches);

/* ---------------------------------------------------------------------------------------------
 * Kernel-level entry points used by the parity tests (tests/test_kernels_gpu.py) to check each
 * HIP kernel against the oracle in isolation.  Same conventions as above.
 * ------------------------------------------------------------------------------------------- */
enum { RP_EPI_STORE_BF16 = 0, RP_EPI_RESID = 1, RP_EPI_GEGLU_BF16 = 2,
       RP_EPI_RESID8 = 3 /* the inference pass's residual stream: out = bf16 plane [M, n_valid], then one-byte extension plane [M, n_valid] */ };
/* C = A[M,K] (bf16) x W[N,K]^T (bf16); M, N multiples of 128 (N may exceed n_valid: only the
 * first n_valid columns are written), K multiple of 32.
 *   STORE_BF16: out bf16 [M, n_valid]
 *   RESID:      out = the residual stream's two bf16 planes [2, M, n_valid] (hi = bf16(x), lo = bf16(x - hi));
 *               x += C, re-split (n_valid multiple of 8) - the training step's form
 *   RESID8:     out = bf16 plane [M, n_valid] followed by a uint8 plane [M, n_valid]: x = float(((hi << 16) | (ext << 8)) -
 *               0x8000), the fp32 word of x rounded to its top 24 bits (hi = that word rounded to 16 bits, half away from
 *               zero; ext = the signed remainder stored biased by 128 = bits 8..15 of (the rounded word + 0x8000); ABI 6);
 *               x += C, re-split - the inference pass's form
 *   GEGLU_BF16: W rows interleaved 32 gate / 32 up; out bf16 [M, n_valid/2] = gelu_new(g)*u  */
RpStatus rp_dbg_gemm(const void* A, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                     int32_t n_valid, int32_t epilogue, void* stream);
/* The same GEMM with the fused T5-RMSNorm pieces (rp_encoder.hip "RMSNorm folded into the GEMMs"):
 *   STORE / GEGLU: accumulators are scaled by rs[row] = rsqrt(sum_p ssp_in[p, row] * inv_d + eps), ssp slot-major [np, M] (ssp_in NULL = 1);
 *   RESID: additionally writes ssp_out[p, row] = sum of x^2 over features [64p, 64p+64) (x as stored: hi + lo); xb_out is
 *          unused (the hi plane IS the next projection's operand) and may be NULL. */
RpStatus rp_dbg_gemm_fused(const void* A, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                           int32_t n_valid, int32_t epilogue, const float* ssp_in, int32_t np_in, float inv_d,
                           float eps, void* xb_out, float* ssp_out, int32_t np_out, void* stream);
/* The T5 RMSNorm statistic as the product computes it (there is no separate normalisation pass): rs[row] =
 * rsqrt(sum_p ssp[p, row] * inv_d + eps) from the slot-major partial sums of squares the residual epilogues emit. */
/* Box calibration for the bench line: `waves_per_cu` x 256 CUs waves each issue `mfmas` v_mfma_f32_32x32x16_bf16 from
 * registers (pseudo-random bf16 operands, eight accumulators per wave, no memory traffic): 32768 FLOP per instruction.
 * The achieved rate is what THIS box's matrix pipes sustain under load (the chip clocks to its power budget: boxes of one
 * pool differ by several per cent), against which a step time can be read.  `sink` (>= 4 bytes) keeps the result live. */
RpStatus rp_dbg_mfma_probe(int32_t waves_per_cu, int32_t mfmas, float* sink, void* stream);
RpStatus rp_dbg_rowscale(const float* ssp /* [np, rows] */, float* rs /* [rows] */, int32_t rows, int32_t np,
                         float inv_d, float eps, void* stream);
RpStatus rp_dbg_attention(const void* qkv_bf16, const int32_t* cu_seqlens, const float* bias_tab,
                          void* out_bf16, int32_t batch, int32_t max_len, int32_t num_heads,
                          int32_t rows_total, void* stream);
/* The encoder's forward kernels in isolation with every launch option reachable (tests/test_encoder_forward_kernels_gpu.py).
 * Each runs the launch code of the encoder pass; arguments are checked before anything is launched (RP_E_INVALID, nothing
 * written); no output is zeroed first.
 *   rp_dbg_gemm_ex: rp_dbg_gemm_fused with the operands' geometry free: A bf16 [M, lda] (lda % 8 == 0), W bf16 [n_rows_w, K] (exactly that many
 *     rows: the operand's row clamp serves the last feature tile), out with leading dimension ldo (RESID: planes [2, M, ldo];
 *     RESID8: bf16 plane [M, ldo] then byte plane [M, ldo]; GEGLU: [M, ldo], n_valid / 2 columns written), the first n_valid
 *     features written.  tokens_valid (0: all M) and t_dev (device int32 or NULL) as encode_pass passes them; prof_class one
 *     of RP_K_GEMM_QKV / O / WI / WO (the class's tile and launch-form options apply).  rs_form 0: no row scale; 1: rs_buf
 *     f32 [M] = rowscale_kernel(ssp_in [np_in, M]), then the RowScale epilogue; 2: the RowScaleFromSlots epilogue on ssp_in
 *     (STORE / GEGLU on the small tiles only).  ssp_out f32 [np_out, M] (RESID / RESID8, optional).  plan: HOST int32 [6] =
 *     what was launched: tile configuration, form (0 one workgroup per tile, 1 persistent, 2 mixed full + half tiles),
 *     feature tiles, token tiles, prefetch helpers, full token rows of the mixed plan.
 *   rp_dbg_attention_ex: rp_dbg_attention with the table's max_distance (bias_tab f32 [H, ntab], ntab = 2 max_distance + 1;
 *     refused when the table with its padding exceeds the kernel's, as rp_encoder_create refuses it).
 *   rp_dbg_encoder_rows (launch only): mode 0 the embedding table into the 24-bit form (a = table f32 [vocab, n]; o0 bf16
 *     [vocab, n], o1 u8 [vocab, n], o2 f32 [vocab]); mode 1 the pass's embedding rows (a / b / c = mode 0's outputs, ia = ids
 *     [T], rows = Tp, a multiple of 256; o0 bf16 [Tp, n], o1 u8 [Tp, n], and o3 = rs f32 [Tp] when given, else o2 = ssp f32
 *     [np, Tp]; the kernel form by n <= 1536 and Tp < 8192 as the pass picks it); mode 2 the last_hidden_state rows (a / b =
 *     planes [rows, n], c = rs [rows], d = final norm weight f32 [n]; o0 bf16 [rows, n]). */
RpStatus rp_dbg_gemm_ex(const void* A, int32_t lda, const void* W, int32_t n_rows_w, void* out, int32_t ldo, int32_t M, int32_t K,
                        int32_t n_valid, int32_t epilogue, int32_t prof_class, int32_t tokens_valid, const int32_t* t_dev,
                        int32_t rs_form, const float* ssp_in, int32_t np_in, float inv_d, float eps, float* rs_buf, float* ssp_out,
                        int32_t np_out, int32_t* plan, void* stream);
/* The current value of an option rp_set_option knows by a variable of its own (not the compound gemm_variant_all). */
RpStatus rp_dbg_get_option(const char* name, int32_t* value);
/* The similarity scan's plan, without a GPU call (tests/test_scan_plan_cpu.py, tests/test_scan_tiles_gpu.py): what
 * rp_sim_topk[_fp8][_after] would launch for (B, N, D, k, flags) under the current options - fp8 != 0: the e4m3 entry points,
 * paged != 0: the _after ones.  The arguments are checked as those calls check them (same status, same message).
 * out: HOST int64 [RP_SIM_PLAN_FIELDS], indexed by RpSimPlanField.  Pass 0 is the dense pass or the sample pass, pass 1 the
 * filter pass (tile -1, 0 workgroups when dense-only); stage 0 is the select behind pass 0, stage 1 the per-query stage behind
 * pass 1 (-1 when dense-only). */
typedef enum {
  /* first-generation kernel (queries are the MFMA rows): dense, sample and fallback filter passes */
  RP_SIM_TILE_Q256 = 0, RP_SIM_TILE_Q128W8, RP_SIM_TILE_Q128K32W8, RP_SIM_TILE_Q64, RP_SIM_TILE_Q32,
  RP_SIM_TILE_SAMPLE, RP_SIM_TILE_SAMPLE_K64W8, RP_SIM_TILE_SAMPLE_Q32, RP_SIM_TILE_SAMPLE_BIG,
  RP_SIM_TILE_8Q256, RP_SIM_TILE_8Q128W8, RP_SIM_TILE_8Q64, RP_SIM_TILE_8Q64_TAIL, RP_SIM_TILE_8Q32, RP_SIM_TILE_8Q32_TAIL,
  RP_SIM_TILE_8SAMPLE, RP_SIM_TILE_8SAMPLE_K64W8, RP_SIM_TILE_8SAMPLE_K64_TAILW8, RP_SIM_TILE_8SAMPLE_Q32,
  RP_SIM_TILE_8SAMPLE_Q32_TAIL,
  /* second-generation filter kernel (premises are the MFMA rows); each has a paged twin */
  RP_SIM_TILE_FILTER_NT8, RP_SIM_TILE_8FILTER_W8, RP_SIM_TILE_8FILTER_TAILW8,
  RP_SIM_TILE_COUNT
} RpSimTile;
typedef enum {
  RP_SIM_STAGE_SELECT = 0,   /* select_kernel, 1024 threads */
  RP_SIM_STAGE_SELECT_SMALL, /* select_kernel, 256 threads */
  RP_SIM_STAGE_GATHER,       /* gather_select_kernel, 1024 threads */
  RP_SIM_STAGE_GATHER_MID,   /* gather_select_kernel, 512 threads */
  RP_SIM_STAGE_GATHER_SMALL  /* gather_select_kernel, 256 threads */
} RpSimStage;
typedef enum {
  RP_SIM_PLAN_DENSE_ONLY = 0, RP_SIM_PLAN_NEW_FILTER, RP_SIM_PLAN_STRIDE, RP_SIM_PLAN_SAMPLE_BLOCKS, RP_SIM_PLAN_FILTER_BLOCKS,
  RP_SIM_PLAN_CAP, RP_SIM_PLAN_BYTES, RP_SIM_PLAN_TILE0, RP_SIM_PLAN_WGS0, RP_SIM_PLAN_TILE1, RP_SIM_PLAN_WGS1,
  RP_SIM_PLAN_PAGED_FILTER /* pass 1 runs the paged twin of its filter tile */, RP_SIM_PLAN_STAGE0, RP_SIM_PLAN_STAGE1,
  RP_SIM_PLAN_FIELDS
} RpSimPlanField;
RpStatus rp_dbg_sim_plan(int32_t B, int32_t N, int32_t D, int32_t k, int32_t flags, int32_t fp8, int32_t paged, int64_t* out);
RpStatus rp_dbg_attention_ex(const void* qkv_bf16, const int32_t* cu_seqlens, const float* bias_tab, void* out_bf16, int32_t batch,
                             int32_t num_heads, int32_t rows_total, int32_t max_distance, int32_t ntab, void* stream);
RpStatus rp_dbg_encoder_rows(int32_t mode, const void* a, const void* b, const void* c, const void* d, const int32_t* ia,
                             const int32_t* t_dev, int32_t T, int32_t rows, int32_t n, int32_t vocab, int32_t np, float inv_d,
                             float eps, void* o0, void* o1, void* o2, void* o3, void* stream);
/* Training kernels in isolation (tests/test_train_kernels_gpu.py).
 *   rp_dbg_wgrad: out f32 [|splits|, ny, nx], partial s = Y[rows of split s]^T X;  Y bf16 [T, ny], X bf16 [T, nx], T % 64 == 0;
 *     splits > 0: 256 x 256 tiles, splits < 0: 128 x 128 tiles.
 *   rp_dbg_attention_bwd: runs the forward (att_out, lse_out [H, rows_total]) and both backward kernels on packed qkv;
 *     att = the O the backward uses for delta (NULL: att_out); dqkv bf16 [rows_total, 3*H*64] (rows of real tokens written);
 *     dtab f32 [2*128+1, H]: gradient of the [H, 257] bias table, transposed.  Synchronises.
 *   rp_dbg_dgrad: mode 0 = gated-GELU backward epilogue (A = dx [M, K], W = Wo2^T [N = d_ff, K]; aux0 = gu bf16 [M, 2N],
 *     aux1 = rs [M]; out0 = dzs bf16 [M, 2N], out1 = row dots f32 [M]); mode 1 = RMSNorm-backward residual epilogue
 *     (A = dzs [M, K], W [N, K]; aux0 = x bf16 [M, N], aux1 = rcoef [M]; out0 = planes [2, M, N] updated in place).
 *     variant: tile configuration (0 = 128x128x32, 26 = 256x256x64 pipelined). */
RpStatus rp_dbg_wgrad(const void* Y, const void* X, float* out, int32_t T, int32_t ny, int32_t nx, int32_t splits,
                      void* stream);
/* two products over the same T token rows in ONE launch of 256 x 256 tiles with a common split count (the training step's
 * weight-gradient pairs): out0 f32 [splits, ny0, nx0], out1 f32 [splits, ny1, nx1] as rp_dbg_wgrad writes them. */
RpStatus rp_dbg_wgrad_pair(const void* Y0, const void* X0, float* out0, int32_t ny0, int32_t nx0, const void* Y1,
                           const void* X1, float* out1, int32_t ny1, int32_t nx1, int32_t T, int32_t splits, void* stream);
/* rp_dbg_wgrad with everything the launch functions take left free (tests/test_train_mfma_kernels_gpu.py): one product, or two
 * (Y1 != NULL) over the same T token rows in one launch; Y bf16 [T, ldy] with ny live columns, X bf16 [T, ldx] with nx, both
 * pitches multiples of 8 and the pointers 16-byte aligned; out f32 [splits, ny, nx] per product.  cfg: 0 = 256 x 256 tiles,
 * 1 = 128 x 128 (one product only), -1 = plan_wgrad's choice; 1 <= splits <= T / 64.  g1 .. dln_part all non-NULL: the
 * finishing epilogue on product 0 (rows of Y0 in the packed [32 gate | 32 up] order, ny0 % 64 == 0, splits == 1, else
 * refused): out0 = d wi_0 [ny0 / 2, nx0], g1 = d wi_1, w0 / w1 the masters [ny0 / 2, nx0], ln [nx0], dln_part f32
 * [ny0 / 32, nx0].  plan_out[2] = the tile configuration and split count that ran.  Everything is checked before the launch;
 * no output is zeroed first.  Launch only.
 * rp_dbg_wgrad_plan (no GPU call): out[4] = (cfg, splits) of plan_wgrad(rows0, cols0, nk), then of plan_wgrad_pair(rows0,
 * cols0, rows1, cols1, nk) (splits 0: separate launches preferred; -1, -1 when rows1 == 0). */
RpStatus rp_dbg_wgrad_ex(const void* Y0, int32_t ldy0, int32_t ny0, const void* X0, int32_t ldx0, int32_t nx0, float* out0,
                         const void* Y1, int32_t ldy1, int32_t ny1, const void* X1, int32_t ldx1, int32_t nx1, float* out1,
                         int32_t T, int32_t cfg, int32_t splits, float* g1, const float* w0, const float* w1, const float* ln,
                         float* dln_part, int32_t* plan_out, void* stream);
/* The training attention alone at any max_distance and under the trainer's dropout: forward (att_out bf16 [rows_total, H * 64],
 * lse_out f32 [H, rows_total], log2 domain), both backward launches (delta_out f32 [H, rows_total], dqkv bf16 [rows_total, 3 * H *
 * 64]: rows of real tokens written) and the table gradient dtab f32 [2 * maxd + 1, H].  qkv / datt bf16, cu_seqlens int32 [batch + 1]
 * on the device (0 .. T <= rows_total, no empty sequence), bias_tab f32 [H, 2 * maxd + 1], rows_total % 256 == 0; att: the O the
 * backward reads for delta (NULL: att_out).  Mask: rp_dbg_dropout_mask(p, seed, site, s0 + i, (h << 20) | j).  Synchronises. */
RpStatus rp_dbg_attention_train(const void* qkv, const void* att, const void* datt, const int32_t* cu_seqlens, const float* bias_tab,
                                int32_t batch, int32_t num_heads, int32_t rows_total, int32_t max_distance, float p, uint32_t seed,
                                uint32_t site, float* lse_out, void* att_out, float* delta_out, void* dqkv, float* dtab, void* stream);
RpStatus rp_dbg_wgrad_plan(int32_t rows0, int32_t cols0, int32_t rows1, int32_t cols1, int32_t nk, int32_t* out);
/* One launch_gemm with a training epilogue and its dropout: A bf16 [M, K], W bf16 [N, K] (exactly N rows), M % 256 == 0; the
 * mask is rp_dbg_dropout_mask(p, seed, site, ..)'s.  mode 0 = the gated-GELU backward over N = d_ff rows (aux0 = gu bf16 [M, ld]
 * with 2 N packed columns, aux1 = rs [M]; out0 = dzs bf16 [M, ld], out1 = the row dot's slots f32 [ceil(N / 64), M], out2 =
 * rcoef f32 [M] = rs^2 (sum of the slots) / K; p > 0: dff masked; variant 0 or 26).  mode 1 = the RMSNorm-backward residual (aux0 = x bf16 [M, ld], aux1 = rcoef
 * [M]; out0 / out1 = the hi / lo planes [M, ld] updated in place; p > 0: also out2 = dxm bf16 [M, ld] = bf16(mask (hi + lo)) of
 * the planes just stored; variant 0 or 26).  mode 2 = the training forward's FFN-in epilogue over N = 2 d_ff packed rows (aux1 =
 * rs [M] or NULL; out0 = gu bf16 [M, N], out1 = ff bf16 [M, ld], masked when p > 0; variant -1 = the forward's choice).
 * mode 3 = the training forward's residual projections (aux0 = the old hi plane bf16 [M, ld], read only; out0 = the new hi
 * plane, out1 = the lo plane updated in place, out2 = ssp f32 [ceil(N / 64), M] or NULL; p > 0: the projection's output is
 * masked before it is added; variant -1 = the forward's choice).
 * plan[6] as rp_dbg_gemm_ex's.  Everything is checked before the launch; no output is zeroed first.  Launch only. */
RpStatus rp_dbg_train_gemm(int32_t mode, const void* A, const void* W, int32_t M, int32_t N, int32_t K, const void* aux0,
                           const float* aux1, void* out0, void* out1, void* out2, int32_t ld, float p, uint32_t seed, uint32_t site,
                           int32_t variant, int32_t* plan, void* stream);
RpStatus rp_dbg_attention_bwd(const void* qkv, const void* att, const void* datt, const int32_t* cu_seqlens,
                              const float* bias_tab, int32_t batch, int32_t num_heads, int32_t rows_total, void* lse_out,
                              void* att_out, void* dqkv, float* dtab, void* stream);
/* out u8 [rows, cols]: 1 where element (site, row0 + r, col0 + c) is kept.  Sites: 0 embeddings, 1 final norm output,
 * 16 + 8 i + {0 attention probabilities (row = the query's packed token index, col = (head << 20) | key offset in its
 * sequence), 1 attention residual branch, 2 gated product inside the FFN, 3 FFN residual branch} (row = packed token
 * index, col = feature).  The decoder's sites (rp_decoder_loss_grad_dropout; rows are packed TARGET token indices): 2
 * embeddings, 3 final norm output, 0x4000 + 8 i + {0 self-attention probabilities, 1 self-attention residual branch, 2
 * cross-attention probabilities (key offset inside the pair's source), 3 cross-attention residual branch, 4 gated product
 * inside the FFN, 5 FFN residual branch}.  Element (site, row, col) is kept iff the 16-bit field (col & 1) of
 * hash(seed, site, row, col >> 1) is >= round(p * 65536): one hash per column pair (rp_encoder_kernels.h::drop_mul2). */
enum {
  RP_DROP_SITE_EMBED = 0, RP_DROP_SITE_FINAL = 1, RP_DROP_SITE_LAYER0 = 16, /* encoder layer i: 16 + 8 i + {0 .. 3} */
  RP_DROP_SITE_DEC_EMBED = 2, RP_DROP_SITE_DEC_FINAL = 3, RP_DROP_SITE_DEC_LAYER0 = 0x4000 /* decoder layer i: + 8 i + {0 .. 5} */
};
RpStatus rp_dbg_dropout_mask(float p, uint32_t seed, uint32_t site, uint32_t row0, uint32_t col0, int32_t rows,
                             int32_t cols, uint8_t* out, void* stream);
RpStatus rp_dbg_dgrad(const void* A, const void* W, int32_t M, int32_t N, int32_t K, int32_t mode, const void* aux0,
                      const float* aux1, void* out0, float* out1, int32_t variant, void* stream);
/* The seq2seq training path's kernels in isolation (tests/test_decoder_kernels_gpu.py; test-only).
 * Each runs the launch functions rp_decoder_loss_grad / rp_train_*_hidden run; scratch is allocated inside, every call
 * synchronises, and no output is zeroed first (rows a kernel does not write keep what the caller put there).
 *   rp_dbg_decoder_attention: dec_flash_kernel, then dec_flash_bwd_kernel<0>, <1> and (causal) bias_grad_kernel, inner = H * 64,
 *     Tp / Sp = the query / key row totals rounded up to 128.  q_cu / k_cu / bucket_of are HOST arrays, the rest device.
 *       causal != 0: q = the fused bf16 [Tp, 3 inner] (q | k | v), kv / k_cu / dkv unused (k_cu = q_cu), dq = the fused
 *                    gradient bf16 [Tp, 3 inner] (dq | dk | dv); bias_tab f32 [H, nbias]; bucket_of int32 [nbias] in
 *                    [0, nbuckets): dtab f32 [nbuckets, H] = the table gradient folded through it (identity: raw).
 *       causal == 0: q bf16 [Tp, inner], kv bf16 [Sp, 2 inner] (k | v), dq bf16 [Tp, inner], dkv bf16 [Sp, 2 inner]; key
 *                    blocks of pairs with no query are not launched; the table arguments are unused.
 *     d_o bf16 [Tp, inner]; out bf16 [Tp, inner]; lse2, delta f32 [H, Tp].
 *   rp_dbg_decoder_attention_dropout: the same with the probabilities dropped at (p, seed, site) - the dropout forms of the
 *     three kernels through the same launch functions; p = 0 gives rp_dbg_decoder_attention's bits.  lse2 is the undropped one.
 *   rp_dbg_decoder_rows: mode 0 bwd_dlogits_kernel (a = logits f32 [rows_pad, n], ia = labels [n_tok], b = loss_sum_count
 *     f64 [2]; o0 bf16 [rows_pad, n]); 1 bwd_cast_kernel (a f32 [rows_pad, n]; o0 bf16); 2 bwd_rmsnorm_kernel<flag> +
 *     colsum_kernel (a = x f32 [n_tok, n], b = ln f32 [n], o0 = dh f32 in / row terms of d ln out, o1 = dx f32 (flag: added
 *     to), o2 = d ln f32 [n]; eps, scale); 3 bwd_geglu_kernel (a = gate | up f32 [rows_pad, 2 n] interleaved by 32, b = dff
 *     f32 [rows_pad, n]; o0 bf16 [rows_pad, 2 n] = dg | du); 4 bwd_embed_kernel<flag> (ia = ids [n_tok], a = dx f32
 *     [n_tok, n]; o0 f32 [vocab, n], flag: added to).  Launch only (stream-ordered).
 *   rp_dbg_hidden_head: hidden_head_kernel, then hidden_head_bwd_kernel + colsum_kernel: xhi / xlo bf16 [T, D], rs f32 [T],
 *     ln f32 [D], d_hidden f32 [T, D]; out_hidden, dxhi, dxlo bf16 [T, D], dln f32 [D].  D % 8 == 0, D <= 2048. */
RpStatus rp_dbg_decoder_attention(int32_t causal, const void* q, const void* kv, const void* d_o, const int32_t* q_cu,
                                  const int32_t* k_cu, int32_t batch, int32_t num_heads, const float* bias_tab, int32_t nbias,
                                  const int32_t* bucket_of, int32_t nbuckets, void* out, float* lse2, float* delta, void* dq,
                                  void* dkv, float* dtab, void* stream);
RpStatus rp_dbg_decoder_attention_dropout(int32_t causal, const void* q, const void* kv, const void* d_o, const int32_t* q_cu,
                                          const int32_t* k_cu, int32_t batch, int32_t num_heads, const float* bias_tab,
                                          int32_t nbias, const int32_t* bucket_of, int32_t nbuckets, float p, uint32_t seed,
                                          uint32_t site, void* out, float* lse2, float* delta, void* dq, void* dkv,
                                          float* dtab, void* stream);
/* The decoder's embedding site alone, fp32 end to end (device pointers): x f32 [n_tok, n] = mask * embed[ids] and dtable f32
 * [vocab, n] = per-id sum of mask * dx, mask = (RP_DROP_SITE_DEC_EMBED, row = token, column = feature).  On a table of ones
 * x is the multiplier itself: exactly 0 or fp32 1 / (1 - p).  Launch only. */
RpStatus rp_dbg_decoder_embed_dropout(const int32_t* ids, int32_t n_tok, const float* embed, int32_t vocab, int32_t n, float p,
                                      uint32_t seed, const float* dx, float* x, float* dtable, void* stream);
RpStatus rp_dbg_decoder_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t n_tok, int32_t rows_pad,
                             int32_t n, int32_t vocab, int32_t flag, float eps, float scale, void* o0, void* o1, void* o2,
                             void* stream);
RpStatus rp_dbg_hidden_head(const void* xhi, const void* xlo, const float* rs, const float* ln, const float* d_hidden,
                            int32_t T, int32_t D, void* out_hidden, void* dxhi, void* dxlo, float* dln, void* stream);
/* The encoder's pooling head, its training row kernels and the weight pack / unpack kernels in isolation
 * (tests/test_encoder_train_kernels_gpu.py; test-only).  Device pointers; each runs the launch functions
 * the encoder pass and the trainer run, with the same grids and in the same order; arguments are checked before anything is
 * launched (RP_E_INVALID: nothing launched, nothing written) and no output is zeroed first.
 *   rp_dbg_train_rows (launch only): one kernel per mode; (p, seed) = the dropout of modes 1, 2, 5 (p = 0: off).
 *     0 embed_kernel<false>, 1 embed_train_kernel (p > 0): ia = ids [T], a = table f32 [vocab, n]; o0 / o1 = the planes bf16
 *       [rows, n] (rows = Tp >= T; rows T .. Tp get token 0), o2 = ssp f32 [np, rows] (slot 0 = the row's sum of squares).  Ids
 *       are clamped to [0, vocab).
 *     2 mask_dx_kernel: a / b = dxhi / dxlo bf16 [rows, n]; o0 = bf16((hi + lo) * mask(site)) [rows, n].
 *     3 qkv_scale_dot_kernel: o0 = dqkv bf16 [rows, n] IN PLACE (rows < T scaled by rs, rows T .. rows zeroed), a = qkv bf16
 *       [rows, n], b = rs f32 [rows]; o1 = rcoef f32 [rows] = rs^2 (dqkv . qkv) inv_d (0 on rows >= T).
 *     4 rowdot_finish_kernel: a = rdp f32 [np, ld], b = rs f32 [rows]; o0 = rcoef f32 [rows] = rs^2 (sum_p rdp[p]) inv_d.
 *     5 embed_bwd_kernel: ia = ids [T], a / b = dxhi / dxlo bf16 [T, n]; o0 = d table f32 [vocab, n], every row written; an
 *       id is clamped to [0, vocab) exactly as the forward's gather clamps it (a negative id lands in row 0).
 *   rp_dbg_pool_head (synchronises; the lists' scratch is allocated inside): worklist_kernel, the forward head, and with
 *     d_emb != NULL pool_bwd_seq_kernel + colsum_kernel + pool_bwd_tok_kernel.  xhi bf16 [>= T, D]; xlo: the bf16 lo plane, or
 *     with lo8 the uint8 extension plane of the 24-bit form; rs f32 [T]; cu int32 [batch + 1]; w f32 [D]; chunk 32 / 64 / 128.
 *     p > 0: pool_partial_train_kernel (the mask of RP_DROP_SITE_FINAL).  Dropout and the backward take the trainer's form only
 *     (chunk 128, fuse 0, bf16 lo plane, fp32 out).  out [batch, D] f32 / bf16; partial f32 [T / chunk + batch, D]: chunk c of
 *     sequence b at row cu[b] / chunk + b + c, gap rows untouched, and with fuse the rows of one-chunk sequences untouched;
 *     pwork int32 [T / chunk + batch, 4] = {first token, length, chunk, sequence}, gap entries zero; ds, dwf f32 [batch, D];
 *     d_final_ln f32 [D]; dxhi / dxlo bf16 [>= T, D] (rows < T written).  Every sequence holds at least its EOS: cu must run
 *     0 .. T strictly increasing - an empty sequence is outside the pooling head's contract (rp_encode_varlen and
 *     rp_train_forward launch no chunk for it, so its `out` row is not written, and the pooled backward divides by its length)
 *     and is RP_E_INVALID here.
 *   rp_dbg_repack (launch only): ONE repack_layer_kernel launch over 1 .. 4 matrices.  Per matrix: mode 0 = q | k | v rows
 *     (s0, s1, s2 f32 [n, cols], rows = 3 n), 1 = 32 rows of s0 then the same 32 of s1 (f32 [rows / 2, cols]), 2 = copy of s0;
 *     colscale f32 [cols] or NULL; dst bf16 [rows, cols] = bf16(master * colscale), dst_t bf16 [cols, rows] = its transpose.
 *     rows and cols are multiples of 64.
 *   rp_dbg_bias_table (launch only): tab f32 [H, ntab], tab[h, o] = rel_bias[bucket_of[o], h] (rel_bias f32 [buckets, H]).
 *   rp_dbg_unfold (launch only): ONE unfold_kernel launch, then (modes 1, 2) the colsum_kernel over dln_part the trainer
 *     runs.  part f32 [splits] x [rows, C] at split_stride elements; mode 0: g0 [rows, C] = the sum over the splits; 1: rows
 *     [k n, (k + 1) n) -> g_k [n, C] (rows = 3 n); 2: rows 64 j + {0 .. 31} -> g0 rows 32 j .., 64 j + {32 .. 63} -> g1 (rows %
 *     64 == 0), each times ln [C]; w0 / w1 / w2: the masters, shaped as g; dln_part f32 [ceil(rows / 32), C]; dln f32 [C] =
 *     sum_r (sum over the splits)[r, c] * master[r, c].  C % 4 == 0. */
typedef struct RpDbgRepackMat {
  const float* s0;
  const float* s1;
  const float* s2;
  const float* colscale;
  void* dst;
  void* dst_t;
  int32_t rows, cols, n, mode;
} RpDbgRepackMat;
RpStatus rp_dbg_train_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t T, int32_t rows, int32_t n,
                           int32_t vocab, int32_t np, int32_t ld, float inv_d, float p, uint32_t seed, uint32_t site, void* o0,
                           void* o1, void* o2, void* stream);
RpStatus rp_dbg_pool_head(const void* xhi, const void* xlo, int32_t lo8, const float* rs, const int32_t* cu_seqlens,
                          int32_t batch, int32_t T, int32_t D, const float* w, int32_t chunk, int32_t fuse, int32_t out_bf16,
                          const float* d_emb, float p, uint32_t seed, void* out, float* partial, void* pwork, float* ds,
                          float* dwf, float* d_final_ln, void* dxhi, void* dxlo, void* stream);
RpStatus rp_dbg_repack(const RpDbgRepackMat* mats, int32_t n_mats, void* stream);
RpStatus rp_dbg_bias_table(const float* rel_bias, const int32_t* bucket_of, int32_t H, int32_t ntab, float* tab, void* stream);
RpStatus rp_dbg_unfold(const float* part, int64_t split_stride, int32_t splits, int32_t rows, int32_t C, int32_t mode, int32_t n,
                       float* g0, float* g1, float* g2, const float* w0, const float* w1, const float* w2, const float* ln,
                       float* dln_part, float* dln, void* stream);
/* The decode step's kernels in isolation (tests/test_decode_step_kernels_gpu.py; test-only).  Device
 * pointers unless said otherwise, launch only (stream-ordered), through the launch code rp_decoder_batch_step / _pool_step run.
 *   rp_dbg_dec_gemm: dec_gemm_kernel<ceil(K / 512), epi>: out[m, n] = sum_k A[m, k] W[n, k], A bf16 [M, lda], W bf16 [N, K]
 *     ([2 N, K] for epi 3), K % 8 == 0; epi 0: out bf16 [M, ldo]; 1: out f32, added to; 2: out f32; 3: out bf16 =
 *     gelu_new(A W[n]) * (A W[n + N]).  K > 4096: RP_E_UNSUPPORTED, nothing launched.
 *   rp_dbg_dec_rows: mode 0 dec_embed_kernel (ia = tokens [rows], a = table f32 [vocab, n]; o0 f32 [rows, n]); 1
 *     dec_rmsnorm_kernel (a = x f32 [rows, n], b = ln f32 [n]; o0 bf16 [rows, n]; eps, scale); 2 dec_log_softmax_kernel (o0 f32
 *     [rows, n], in place); 3 dec_store_kv_kernel<DecSlots> (a = qkv bf16 [n_active * nb, 3 n], n = inner; o0 = the caches, state s at
 *     s * state_stride elements, max_len * nb rows of 2 n; row pos[slot] * nb + beam of state[slot] <- k | v of its qkv row).
 *   rp_dbg_dec_attention: dec_attention_kernel<cross != 0, DecSlots> over the n_active * nb rows of a slot table.  self: kv = the caches
 *     (state s at s * state_stride elements, rows = max_len * nb rows of ldkv), keys 0 .. pos[slot] through anc int32
 *     [n_active * nb, astride] (entries clamped to [0, rows)), bias tab f32 [H, nbias] by distance (clamped at nbias - 1).
 *     cross: kv = `rows` rows of ldkv, slot a reads rows [src_off[a], src_off[a] + src_len[a]), no bias.  K at column
 *     koff + 64 h, V at voff + 64 h; q bf16 [rows, ldq], out bf16 [rows, ldo].
 *   state / src_off / src_len / pos are HOST arrays of n_active entries, checked as rp_decoder_pool_step checks its own
 *   (counts, distinct states in [0, n_states), pos in [0, max_len), anc_stride > pos). */
RpStatus rp_dbg_dec_gemm(int32_t epi, const void* A, int32_t lda, int32_t M, const void* W, int32_t N, int32_t K, void* out,
                         int32_t ldo, void* stream);
RpStatus rp_dbg_dec_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t rows, int32_t n, int32_t vocab,
                         float eps, float scale, const int32_t* state, const int32_t* pos, int32_t n_active, int32_t n_states,
                         int32_t nb, int32_t max_len, int64_t state_stride, void* o0, void* stream);
RpStatus rp_dbg_dec_attention(int32_t cross, const void* q, int32_t ldq, const void* kv, int32_t ldkv, int32_t koff, int32_t voff,
                              int32_t rows, int64_t state_stride, int32_t n_states, const int32_t* anc, int32_t anc_stride,
                              const float* bias_tab, int32_t nbias, int32_t nb, int32_t num_heads, const int32_t* state,
                              const int32_t* src_off, const int32_t* src_len, const int32_t* pos, int32_t n_active,
                              int32_t max_len, void* out, int32_t ldo, void* stream);
/* Tuning knobs (integers), e.g. "gemm_variant"; returns RP_E_INVALID for unknown names. */
RpStatus rp_set_option(const char* name, int32_t value);


/* ---------------------------------------------------------------------------------------------
 * Tactic generator: the T5 decoder of T5ForConditionalGeneration, one beam-search step at a time
 *   (transformers modeling_t5.py T5Stack.forward as a decoder with a KV cache; generation/utils.py
 *   _beam_search's top-2nb selection).  reprover_amd/generation.py drives it; DESIGN.md section 9.
 * ------------------------------------------------------------------------------------------- */

/* T5's unidirectional bucket (bidirectional=False) of rel = key position - query position (<= 0). */
int32_t rp_relative_position_bucket_causal(int32_t rel, int32_t num_buckets, int32_t max_distance);

/* The encoder's last_hidden_state (final RMSNorm applied) instead of the pooled embedding: same
 * arguments and workspace as rp_encode_varlen; out = device bf16 [total_tokens, d_model]. */
RpStatus rp_encode_hidden(RpEncoder* enc, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                          int32_t total_tokens, int32_t max_len, void* out_bf16, void* workspace,
                          size_t workspace_bytes, void* stream);

typedef struct RpT5DecoderLayerWeights {
  const void* ln_self;   /* decoder.block.i.layer.0.layer_norm.weight          [d_model]         */
  const void* q;         /* ...layer.0.SelfAttention.{q,k,v}.weight            [H*d_kv, d_model] */
  const void* k;
  const void* v;
  const void* o;         /* ...layer.0.SelfAttention.o.weight                  [d_model, H*d_kv] */
  const void* ln_cross;  /* ...layer.1.layer_norm.weight                       [d_model]         */
  const void* cq;        /* ...layer.1.EncDecAttention.{q,k,v}.weight          [H*d_kv, d_model] */
  const void* ck;
  const void* cv;
  const void* co;        /* ...layer.1.EncDecAttention.o.weight                [d_model, H*d_kv] */
  const void* ln_ff;     /* ...layer.2.layer_norm.weight                       [d_model]         */
  const void* wi_0;      /* ...layer.2.DenseReluDense.wi_0.weight              [d_ff, d_model]   */
  const void* wi_1;
  const void* wo;        /* ...layer.2.DenseReluDense.wo.weight                [d_model, d_ff]   */
} RpT5DecoderLayerWeights;

typedef struct RpT5DecoderWeights {
  const void* embed;            /* shared.weight                               [vocab, d_model]  */
  const void* rel_bias;         /* decoder.block.0 SelfAttention relative_attention_bias [buckets, H] */
  const void* final_ln;         /* decoder.final_layer_norm.weight             [d_model]         */
  const void* lm_head;          /* lm_head.weight (shared.weight when tied)    [vocab, d_model]  */
  const RpT5DecoderLayerWeights* layers; /* host array, cfg->num_layers (= num_decoder_layers)   */
  int32_t tie_word_embeddings;  /* 1: hidden * d_model^-0.5 before lm_head (HF's scale_decoder_outputs) */
} RpT5DecoderWeights;

typedef struct RpDecoder RpDecoder;

/* cfg->num_layers is the number of DECODER layers.  Packs bf16 weights (synchronises once). */
RpStatus rp_decoder_create(const RpT5Config* cfg, const RpT5DecoderWeights* weights, int32_t weight_dtype,
                           RpDecoder** out);
void     rp_decoder_destroy(RpDecoder* dec);
/* Workspace of one generate call: cross K/V of a src_len source, the self-attention cache of
 * max_len * num_beams rows per layer, activations of num_beams rows.  0 on bad arguments. */
size_t   rp_decoder_workspace_bytes(const RpDecoder* dec, int32_t num_beams, int32_t max_len, int32_t src_len);
/* Cross-attention K/V of every layer from the encoder states enc_bf16 [src_len, d_model] (one
 * GEMM against the concatenated [layers*2*H*d_kv, d_model] weight), into the workspace. */
RpStatus rp_decoder_cross_kv(RpDecoder* dec, const void* enc_bf16, int32_t src_len, int32_t num_beams,
                             int32_t max_len, void* workspace, size_t workspace_bytes, void* stream);
/* One decode step at position t for nb beams (same workspace as rp_decoder_cross_kv):
 *   tokens    device int32 [nb], the beams' tokens at position t
 *   ancestry  device int32 [nb, anc_stride]: cache row read by beam b at position p <= t; row
 *             t*nb + b is the one this step writes for beam b (entries are clamped to the cache)
 *   logprobs  device fp32 [nb, vocab]: log_softmax of the lm_head logits
 * A row's output does not depend on the other rows of the launch. */
RpStatus rp_decoder_step(RpDecoder* dec, const int32_t* tokens, const int32_t* ancestry, int32_t anc_stride,
                         int32_t nb, int32_t t, int32_t max_len, int32_t src_len, float* logprobs,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Top k (<= 128, <= nb*vocab) of logprobs[b, v] + running[b] over the flattened [nb*vocab], in
 * descending order, ties to the lower flat index (torch.topk): score, token (v), parent (b).
 * workspace: nb * min(k, vocab) * 8 bytes of device memory. */
RpStatus rp_beam_select(const float* logprobs, const float* running, int32_t nb, int32_t vocab, int32_t k,
                        float* scores, int32_t* tokens, int32_t* parents, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Batched generation: one decode loop for the beams of n proof states ("One step,
 * 1 - 32 states").  All states start together and sit at the same position t; a state that has finished
 * is left out of the step's active list and costs nothing (states that join a running search, each at
 * its own position: the slot pool below).  For every state the outputs are the bits
 * that rp_decoder_cross_kv / rp_decoder_step / rp_beam_select give that state alone, whichever other
 * states share the call and in whatever order: those three are the one-state calls of the functions
 * below (n = 1, src_cu = {0, src_len}, active = {0}), one implementation.
 * Caps: 1 <= n <= 32 states, n * num_beams <= 1024 rows (16 states of 64 beams), num_beams <= 64, max_len <= 8192, every source
 * 1..8192 tokens, vocab <= 512.
 *   src_cu  HOST int32 [n + 1] prefix sums (start at 0): source b is rows src_cu[b] .. src_cu[b+1] of
 *           enc_bf16 [src_cu[n], d_model] (rp_encode_hidden over the packed sources)
 * Workspace (each part rounded up to 256 bytes; L = decoder layers, inner = H * d_kv):
 *   cross K/V   src_cu[n] * L * 2 * inner * 2 bytes
 *   cache       n * L * max_len * num_beams * 2 * inner * 2 bytes: per state and layer
 *               [max_len * num_beams, 2 * inner], row t * num_beams + b, as rp_decoder_step lays it out
 *               (ByT5-small, 64 beams x 512 positions: ~200 MB per state)
 *   activations n * num_beams * (4 d_model + 2 (d_model + d_ff) + 6 inner + 2 inner) bytes
 * rp_decoder_batch_workspace_bytes returns 0 on bad arguments (rp_last_error says why). */
size_t   rp_decoder_batch_workspace_bytes(const RpDecoder* dec, const int32_t* src_cu, int32_t n,
                                          int32_t num_beams, int32_t max_len);
/* Cross-attention K/V of every layer for all n sources in one GEMM over the src_cu[n] packed rows. */
RpStatus rp_decoder_batch_cross_kv(RpDecoder* dec, const void* enc_bf16, const int32_t* src_cu, int32_t n,
                                   int32_t num_beams, int32_t max_len, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* One decode step at position t for the n_active states still searching; row a * nb + b is beam b of the
 * state in slot a:
 *   active    HOST int32 [n_active]: distinct state indices in [0, n), the state each slot carries (host
 *             memory, so that it is checked here: two slots naming one state would share cache rows)
 *   tokens    device int32 [n_active * nb]
 *   ancestry  device int32 [n_active * nb, anc_stride]: as rp_decoder_step, entries local to the state's
 *             own cache (row t * nb + b is the one written for beam b; entries are clamped to that cache)
 *   logprobs  device fp32 [n_active * nb, vocab]
 * One launch per kernel over all rows (12 per layer + 4); the attentions size their LDS for the longest
 * key list of the call. */
RpStatus rp_decoder_batch_step(RpDecoder* dec, const int32_t* src_cu, int32_t n, const int32_t* active,
                               int32_t n_active, const int32_t* tokens, const int32_t* ancestry,
                               int32_t anc_stride, int32_t nb, int32_t t, int32_t max_len, float* logprobs,
                               void* workspace, size_t workspace_bytes, void* stream);
/* rp_beam_select for n_active (<= 32) states in one launch pair: per state a, the top k of
 * logprobs[a * nb + b, v] + running[a * nb + b] over its own [nb * vocab] block, in rp_beam_select's
 * order; scores / tokens / parents are [n_active, k], parents local to the state.
 * workspace: n_active * nb * min(k, vocab) * 8 bytes of device memory. */
RpStatus rp_beam_select_batch(const float* logprobs, const float* running, int32_t n_active, int32_t nb,
                              int32_t vocab, int32_t k, float* scores, int32_t* tokens, int32_t* parents,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The slot pool: continuous batching ("Continuous batching").  A workspace of n_slots
 * places, each able to carry one proof state's search; a state is admitted into a free slot between two
 * steps and leaves it when it stops, so the states of one step stand at different positions.  The step is
 * rp_decoder_batch_step's launch sequence with a position per slot instead of one t: a slot's beams store
 * cache row pos * nb + b and attend over ancestry columns 0 .. pos.  For every state the log-probs are the
 * bits rp_decoder_step gives it alone at that position, whichever states share the call, wherever they
 * stand and in whatever slot order.  rp_beam_select_batch serves the pool as it is (selection reads no
 * position).
 * Layout: rp_decoder_batch_workspace_bytes' with n = n_slots and a cross K/V part of n_slots * src_cap rows.
 * Slot s owns cross-K/V rows s * src_cap .. (s + 1) * src_cap and cache state s.
 * Caps: 1 <= n_slots <= 32, n_slots * num_beams <= 1024, num_beams <= 64, max_len and src_cap in 1..8192.
 * rp_decoder_pool_workspace_bytes returns 0 on bad arguments (rp_last_error says why).
 *
 * rp_decoder_pool_admit writes the cross K/V of m newly encoded sources into their slots' regions, one GEMM
 * per source against the weight rp_decoder_batch_cross_kv uses (a GEMM row depends on no other row: the same
 * bits):
 *   slots     HOST int32 [m]: distinct slots in [0, n_slots), the place each source takes
 *   enc_bf16  device bf16 [src_cu[m], d_model]: rp_encode_hidden over the packed newcomers
 *   src_cu    HOST int32 [m + 1] prefix sums (start at 0), every source 1..src_cap rows
 * A re-used slot needs no clearing: every cache row a state reads at position p was written by that state
 * at a position <= p (its ancestry names only rows of its own earlier steps), and every cross key it reads
 * lies below its own src_len, which its own admission wrote.  Nothing a previous tenant left is read.
 *
 * rp_decoder_pool_step: one decode step for the n_active slots listed; row a * nb + b is beam b of slot
 * active[a]:
 *   active    HOST int32 [n_active]: distinct slots in [0, n_slots)
 *   pos       HOST int32 [n_active]: the position each slot's beams stand at, 0 <= pos < max_len
 *   src_len   HOST int32 [n_active]: the source length each slot was admitted with, 1 .. src_cap
 *   tokens    device int32 [n_active * nb]
 *   ancestry  device int32 [n_active * nb, anc_stride]: row r's columns 0 .. pos[r / nb] are read (entries
 *             local to the slot's cache, clamped to it); anc_stride >= the largest pos + 1
 *   logprobs  device fp32 [n_active * nb, vocab]
 * The self-attention sizes its LDS for the largest pos + 1 of the call.
 * RP_E_INVALID (nothing is launched, rp_last_error says which): a null pointer, a slot outside
 * [0, n_slots), a slot named twice, pos outside [0, max_len), src_len outside 1..src_cap, anc_stride below
 * a pos + 1, the caps above.  RP_E_WORKSPACE (nothing is launched): workspace_bytes below
 * rp_decoder_pool_workspace_bytes. */
size_t   rp_decoder_pool_workspace_bytes(const RpDecoder* dec, int32_t n_slots, int32_t num_beams, int32_t max_len,
                                         int32_t src_cap);
RpStatus rp_decoder_pool_admit(RpDecoder* dec, int32_t n_slots, int32_t num_beams, int32_t max_len, int32_t src_cap,
                               const int32_t* slots, const void* enc_bf16, const int32_t* src_cu, int32_t m,
                               void* workspace, size_t workspace_bytes, void* stream);
RpStatus rp_decoder_pool_step(RpDecoder* dec, int32_t n_slots, int32_t num_beams, int32_t max_len, int32_t src_cap,
                              const int32_t* active, const int32_t* pos, const int32_t* src_len, int32_t n_active,
                              const int32_t* tokens, const int32_t* ancestry, int32_t anc_stride, float* logprobs,
                              void* workspace, size_t workspace_bytes, void* stream);

/* rp_decoder_batch_step with a position per listed state: pos HOST int32 [n_active] in place of t, each checked as t
 * is (0 <= pos < max_len, anc_stride >= pos + 1).  The same launch sequence; with every pos = t the same bits. */
RpStatus rp_decoder_batch_step_pos(RpDecoder* dec, const int32_t* src_cu, int32_t n, const int32_t* active,
                                   int32_t n_active, const int32_t* tokens, const int32_t* ancestry,
                                   int32_t anc_stride, int32_t nb, const int32_t* pos, int32_t max_len,
                                   float* logprobs, void* workspace, size_t workspace_bytes, void* stream);

/* Prompt prefill ("Tactic prefix").  A decoder prompt [start, b_1 .. b_P] is shared by
 * all beams of its state, so one cache row per prompt position serves them all: beam 0's, row p * nb.  The
 * prefill carries the first R = P prompt tokens (the prompt without its last token, which the search feeds
 * itself at t = R) through the layers, all positions of all listed states in one launch sequence, and writes
 * in every layer cache rows p * nb, p = 0 .. R - 1, of each listed state - nothing else of the cache, no
 * lm_head, no log-softmax.  The rows are, bit for bit, those that R calls of rp_decoder_batch_step write for
 * beam 0 when fed the prompt's tokens with identity ancestry.  Runs between steps: the activation block is its
 * scratch, and it takes the rows in passes of at most n * nb (pool: n_slots * nb) rows, lower positions first.
 *   states / slots  HOST int32 [m]: distinct, 1 <= m <= n (n_slots)
 *   src_len         (pool) HOST int32 [m]: as rp_decoder_pool_step takes it
 *   prompt_cu       HOST int32 [m + 1] prefix sums (start at 0): listed state j has R_j = prompt_cu[j+1] -
 *                   prompt_cu[j] rows, 1 <= R_j, R_j + 1 < max_len
 *   tokens          device int32 [prompt_cu[m]]: row prompt_cu[j] + p is position p of listed state j
 *                   (clamped to the vocabulary on the device, as the step's)
 *   anc             device int32 [anc_len]: the prompt ancestry anc[p] = p * nb, one vector for every row
 *                   (entries are clamped to the state's cache); anc_len >= every R_j
 * RP_E_INVALID (nothing is launched): a null pointer, a state or slot out of range or named twice,
 * prompt_cu[0] != 0, an R_j outside the above, anc_len below an R_j, the caps of the step.  RP_E_WORKSPACE
 * (nothing is launched): a workspace below rp_decoder_batch_workspace_bytes / rp_decoder_pool_workspace_bytes. */
RpStatus rp_decoder_batch_prefill(RpDecoder* dec, const int32_t* src_cu, int32_t n, const int32_t* states,
                                  const int32_t* prompt_cu, int32_t m, const int32_t* tokens, const int32_t* anc,
                                  int32_t anc_len, int32_t nb, int32_t max_len, void* workspace,
                                  size_t workspace_bytes, void* stream);
RpStatus rp_decoder_pool_prefill(RpDecoder* dec, int32_t n_slots, int32_t num_beams, int32_t max_len, int32_t src_cap,
                                 const int32_t* slots, const int32_t* src_len, const int32_t* prompt_cu, int32_t m,
                                 const int32_t* tokens, const int32_t* anc, int32_t anc_len, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Beam books ("Per-step host sync, and device books"): beam search's bookkeeping -
 * what generation.py's _BeamState keeps on the host - in one caller-owned device block for n states, and one launch per
 * position that updates it from rp_beam_select_batch's outputs, so the host loop reads nothing back per
 * step.  The block, every part starting at a multiple of 16 bytes, in this order (tables are int32 with
 * max_len columns per row; a pair [2] is read at member t & 1 and written at the other by the step at t):
 *   run_seq [2][n][nb][max_len]  running sequences          anc [2][n][nb][max_len]  their ancestry rows
 *   fin_seq [2][n][nb][max_len]  finished hypotheses        run_scores, beam_scores fp32 [n][nb]
 *   fin_flag, fin_len int32 [n][nb]  is_sent_finished; generated tokens of the hypothesis
 *   heur, done, steps int32 [n]      heuristic_unsatisfied; stopped; advances taken (steps & 1 = the
 *                                    current member of the state's pairs)
 *   tokens int32 [n * nb], running fp32 [n * nb], anc_rows int32 [n * nb][max_len]: BY ROW (slot * nb + b),
 *     the next rp_decoder_batch_step's tokens / ancestry (anc_stride = max_len) and the next
 *     rp_beam_select_batch's running scores for the active list of the advance that wrote them
 * rp_beam_books_bytes returns 0 on bad arguments (rp_last_error says why).
 * rp_beam_books_init: _BeamState.__init__ for all n states (sequences eos with the start token in column
 * 0, run_scores {0, -1e9, ..}, beam_scores -1e9, nothing finished, heur 1, done 0, identity ancestry
 * c * nb + b, by-row inputs for the active list 0 .. n - 1).
 * rp_beam_advance: _BeamState.advance for the states of `active` (HOST int32 [n_active], as
 * rp_decoder_batch_step takes it) at position t, one workgroup per slot, in fp32 with one rounding per
 * operation.  scores / tokens / parents are [n_active, 2 nb].  With idx the candidate's index:
 *   1. hits = token == eos || t + 2 >= max_len;  run_lp = score + (hits ? -1e9 : -0.0)
 *   2. the next running beams are the top nb of run_lp, descending, ties (-0.0 == +0.0) to the lower idx;
 *      beam r takes run_seq / anc row parents[c] with token / (t + 1) * nb + r in column t + 1
 *   3. fin = score / fin_div + (heur ? 0 : -1e9) + (hits && idx < nb ? -0.0 : -1e9); the new hypotheses are
 *      the top nb of [the nb kept beam_scores, fin] in the same order
 *   4. heur &= any(run_scores[0] / run_div > (fin_flag ? min(beam_scores) : -1e9));  done = !heur || all(hits)
 *   5. the by-row inputs of the next step for the slot
 *   6. a state whose done is set is left exactly as it is, whatever triples arrive
 * fin_div, run_div: (t + 1) ** length_penalty, rounded to fp32 by the caller.
 * RP_E_INVALID (nothing is launched): null pointers, nb outside 1..64, n outside 1..32, more than 1024
 * rows, max_len outside 2..8192, active not distinct or outside [0, n), t + 1 >= max_len, bytes below
 * rp_beam_books_bytes.
 *
 * The slot pool's books (rp_decoder_pool_*: state index = slot place, n = n_slots), a position per slot.  `active` /
 * `pos` are HOST int32 [n_active]: the slots in use in listing order (row a * nb + b of the by-row parts is beam b of
 * slot active[a]) and the position each stands at; `states` is HOST int32 [m].
 * rp_beam_books_admit: rp_beam_books_init's values for the listed states only (one device routine serves both): every
 * by-state part of those states over all max_len columns in both pair members (the previous tenant wrote them, and the
 * 16-byte gathers of an advance copy up to three columns past t + 1), scores, flags, heur 1, done 0, steps 0.  Nothing
 * of another state and nothing by row is touched.
 * rp_beam_pool_advance: rp_beam_advance with slot a's t = pos[a] throughout (the pair member read, the column written,
 * the ancestry entry (pos[a] + 1) * nb + r, the max_len test, fin_len, steps) and its own divisors fin_div[a] /
 * run_div[a] (HOST float [n_active], the caller's (pos[a] + 1) ** length_penalty).  One kernel: rp_beam_advance is the
 * call in which every slot has pos = t.
 * rp_beam_books_rows: the by-row inputs (tokens, running, anc_rows) of rows a * nb + b from the by-state parts of
 * state active[a]: its current pair member pos[a] & 1, the token in column pos[a] of run_seq, the whole ancestry row.
 * Needed whenever the active list changes (admission, departure); by-state and by-row parts are disjoint.
 * RP_E_INVALID (nothing is launched): as above, and states / active not distinct or outside [0, n), m or n_active
 * outside 1..n, a pos outside [0, max_len - 2]. */
size_t   rp_beam_books_bytes(int32_t n, int32_t nb, int32_t max_len);
RpStatus rp_beam_books_init(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, int32_t eos,
                            int32_t start_token, void* stream);
RpStatus rp_beam_advance(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, const int32_t* active,
                         int32_t n_active, int32_t t, const float* scores, const int32_t* tokens,
                         const int32_t* parents, float fin_div, float run_div, int32_t eos, void* stream);
RpStatus rp_beam_books_admit(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, const int32_t* states,
                             int32_t m, int32_t eos, int32_t start_token, void* stream);
RpStatus rp_beam_pool_advance(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, const int32_t* active,
                              const int32_t* pos, int32_t n_active, const float* scores, const int32_t* tokens,
                              const int32_t* parents, const float* fin_div, const float* run_div, int32_t eos,
                              void* stream);
RpStatus rp_beam_books_rows(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, const int32_t* active,
                            const int32_t* pos, int32_t n_active, void* stream);

/* Sampled generation ("Sampling"): after rp_decoder_batch_step, one launch draws one
 * token per row (row = slot * nb + sample, the step's layout) from logprobs [n_active * nb, vocab] and
 * keeps the rows' books, so the host loop needs no readback.  HF's TemperatureLogitsWarper ->
 * TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial, per row and in fp32:
 *   1. s[v] = logprobs[v] / temperature
 *   2. top-k (0 < top_k < vocab): drop s[v] < the k-th largest value; ties with it stay
 *   3. top-p (top_p < 1), over e[v] = exp(s[v] - max) of what 2 kept: in ascending order of probability,
 *      equal ones by descending id, drop every token whose inclusive cumulative mass is
 *      <= (1 - top_p) * sum(e); the most probable token (the lowest id among equals) always stays
 *   4. over the kept ids in ascending order, C(v) = inclusive prefix sum of e, Z = its total: the token
 *      is the smallest kept v of non-zero mass with C(v) > u * Z, else the last kept v of non-zero mass
 *   5. u = rp_sample_uniform(seeds[state], sample, t)
 * Arrays indexed by state (not slot), all device memory, n = the states of the call:
 *   seeds        uint32 [n]
 *   seq          int32 [n, nb, max_len]: the token goes to position t + 1
 *   cum_logprob  fp32  [n, nb]: += logprobs[token], the model's log-prob (untempered, unfiltered)
 *   n_generated  int32 [n, nb]: += 1
 *   finished     int32 [n, nb]: set when token == eos.  A row already finished writes pad to seq and
 *                tokens_next and changes nothing else.
 *   tokens_next  int32 [n_active * nb], by row: the next step's tokens
 *   active       HOST int32 [n_active]: distinct states in [0, n), as rp_decoder_batch_step takes it
 * RP_E_INVALID (nothing is launched): temperature <= 0 or not finite, top_p outside (0, 1], top_k < 0,
 * vocab outside 1..512, nb outside 1..64, n outside 1..32, more than 1024 rows, t + 1 >= max_len. */
RpStatus rp_sample_step(const float* logprobs, int32_t vocab, const int32_t* active, int32_t n_active, int32_t n,
                        int32_t nb, const uint32_t* seeds, int32_t t, int32_t max_len, float temperature,
                        int32_t top_k, float top_p, int32_t eos, int32_t pad, int32_t* seq, int32_t* tokens_next,
                        float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream);
/* The sampler's uniform in [0, 1), host only: (h >> 8) * 2^-24 with
 *   h = fmix32(fmix32(seed ^ 0x53414D50) + sample * 0x85EBCA77 + position * 0x27D4EB2F)   (mod 2^32)
 * fmix32 = murmur3's 32-bit finaliser (the training dropout's hash ends in it too).  seed is the state's,
 * sample the row's index inside its state, position the step's t: nothing else enters. */
float    rp_sample_uniform(uint32_t seed, uint32_t sample, uint32_t position);

/* The slot pool's sampler ("Continuous batching for sampling"): rp_sample_step's books for
 * rp_decoder_pool_*, state index = slot place and n = n_slots, a position per slot.  The books stay the separate
 * caller-owned device arrays above (seeds, seq, cum_logprob, n_generated, finished by state; tokens_next by row).
 * `active` / `pos` are HOST int32 [n_active]: the slots in use in listing order (row a * nb + b is sample b of slot
 * active[a]) and the position each stands at; `states` is HOST int32 [m] and `new_seeds` HOST uint32 [m] (both travel
 * as kernel arguments).  None of the three takes a workspace.
 * rp_sample_pool_step: rp_sample_step with slot a's t = pos[a] throughout: u = rp_sample_uniform(seeds[state], sample,
 * pos[a]), the token goes to column pos[a] + 1.  One kernel: rp_sample_step is the call in which every slot has pos = t.
 * rp_sample_pool_admit: a slot's next tenant.  For the listed states only: seeds[s] = new_seeds[i]; every seq row of the
 * state pad over ALL max_len columns with the start token in column 0 (the previous tenant wrote them, and a result is
 * trimmed by n_generated, not by content); cum_logprob 0, n_generated 0, finished 0.  Nothing of another state and
 * nothing by row is touched.
 * rp_sample_pool_rows: tokens_next[a * nb + b] = seq[active[a], b, pos[a]], the by-row input of the next
 * rp_decoder_pool_step.  Needed whenever the active list changes (admission, departure).  That step's ancestry is the
 * identity table [n_slots * nb, max_len] with entry [r, p] = p * nb + r % nb, built once: it depends on r % nb only, so
 * its first n_active * nb rows serve any active list.
 * RP_E_INVALID (nothing is launched): everything rp_sample_step refuses (max_len < 2 included), and a null pos, a
 * pos[a] outside [0, max_len - 2], states / active not distinct or outside [0, n), m or n_active outside 1..n, more
 * than 1024 listed rows. */
RpStatus rp_sample_pool_step(const float* logprobs, int32_t vocab, const int32_t* active, const int32_t* pos,
                             int32_t n_active, int32_t n, int32_t nb, const uint32_t* seeds, int32_t max_len,
                             float temperature, int32_t top_k, float top_p, int32_t eos, int32_t pad, int32_t* seq,
                             int32_t* tokens_next, float* cum_logprob, int32_t* n_generated, int32_t* finished,
                             void* stream);
RpStatus rp_sample_pool_admit(const int32_t* states, const uint32_t* new_seeds, int32_t m, int32_t n, int32_t nb,
                              int32_t max_len, int32_t start_token, int32_t pad, uint32_t* seeds, int32_t* seq,
                              float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream);
RpStatus rp_sample_pool_rows(const int32_t* active, const int32_t* pos, int32_t n_active, int32_t n, int32_t nb,
                             int32_t max_len, const int32_t* seq, int32_t* tokens_next, void* stream);

/* Constrained decoding ("Constrained decoding"): one launch between a decode step and its selection
 * or sampler launch that overwrites the forbidden entries of the step's log-probs with -inf and leaves every other bit
 * of them as it was.  The constraint is a deterministic automaton over token ids:
 *   next  device int16 [n_q, vocab], contiguous: next[s][v] is the state after token v in state s, < 0 = forbidden.
 * rp_constraint_mask: row r of logprobs [rows, vocab] is masked by state q_rows[r] (device int32 [rows], by launch row:
 * the host-books loops upload it with the step's tokens).
 * rp_constraint_mask_step: the form for loops that read nothing back.  q is device int32 [n, nb] by (state, sample) like
 * the sampler's books; `active` / `pos` are HOST int32 [n_active] and travel as kernel arguments; tokens_in is the step's
 * by-row input (the sampler's tokens_next).  For row a * nb + b of slot active[a]: pos[a] == 0 sets q = 0 (which is
 * also how an admitted slot's next tenant starts clean); else q moves to next[q][tokens_in[row]] where that is >= 0 and
 * stays where it is not (a finished row that is fed pad); then the row is masked by the new q, which is stored.  q of
 * a state that is not listed is not touched.
 * q, q_rows, tokens_in and the table are device memory, so their VALUES cannot be checked here: a state is clamped into
 * [0, n_q) and a token into [0, vocab) before either indexes anything, so no value reaches an address outside the
 * buffers (a wrong value masks its own row by the clamped state and harms nothing else).
 * Neither takes a workspace.  RP_E_INVALID (nothing is launched): a null pointer, logprobs / next not aligned to their
 * element type, vocab outside 1..512, rows outside 1..1024, n_q outside 1..4096, nb outside 1..64, n outside 1..32,
 * n_active outside 1..n, more than 1024 listed rows, active not distinct or outside [0, n), a negative pos. */
RpStatus rp_constraint_mask(float* logprobs, int32_t vocab, int32_t rows, const int32_t* q_rows, const int16_t* next,
                            int32_t n_q, void* stream);
RpStatus rp_constraint_mask_step(float* logprobs, int32_t vocab, const int32_t* active, const int32_t* pos,
                                 int32_t n_active, int32_t n, int32_t nb, const int32_t* tokens_in, int32_t* q,
                                 const int16_t* next, int32_t n_q, void* stream);

/* Sampling parameters per row ("Sampling parameters per request"): rp_sample_step and
 * rp_sample_pool_step with a parameter table in place of temperature / top_k / top_p, and rp_sample_pool_admit with a
 * count of live rows per admitted state.  The same kernels; none of the three takes a workspace.
 *   params  device int32 [n, nb, 4], 16-byte aligned, indexed by (state, sample) like the other books.  Block
 *           (state, sample) = { the bits of fp32 temperature, top_k, the bits of fp32 top_p, 0 }.
 * Two statements hold for every row:
 *   - a row whose block holds (T, k, p) draws what rp_sample_step / rp_sample_pool_step with (T, k, p) draws for it, bit
 *     for bit in every book: 1 - top_p is formed on the device by the expression the by-value call evaluates on the
 *     host, (float)(1.0 - (double)top_p), and s[v] = logprobs[v] / temperature is the same fp32 division;
 *   - a row depends on its own block only: the workgroup of row (state, sample) reads those 16 bytes and no other part
 *     of the table, and the step writes none of it.  A finished row reads nothing of it.
 * The table is device memory, so its VALUES cannot be checked here: the caller validates them (reprover_amd:
 * generation.check_sampling, before the upload).  A block outside rp_sample_step's domain (temperature <= 0 or not
 * finite, top_k < 0, top_p outside (0, 1]) makes that row draw an unspecified token in [0, vocab) and nothing else:
 * no access leaves the buffers, because top_k is used as an index only inside 0 < top_k < vocab, temperature and
 * top_p enter arithmetic alone, and the token is clamped to [0, vocab) before it addresses logprobs; the row's other
 * books are updated as for any token, and no other row is affected.
 * rp_sample_pool_admit_rows: rp_sample_pool_admit, except that rows b >= n_live[i] of admitted state states[i] start
 * with finished = 1 (they write pad, keep n_generated = 0 and cum_logprob = 0, and count as finished when the state's
 * flags are reduced).  n_live is HOST int32 [m] and travels as a kernel argument.  rp_sample_pool_admit is the call with
 * every n_live[i] = nb.
 * RP_E_INVALID (nothing is launched; rp_last_error says which): everything rp_sample_step / rp_sample_pool_step /
 * rp_sample_pool_admit refuse apart from the three by-value parameter checks, a null params, a params that is not
 * 16-byte aligned, a null n_live, an n_live[i] outside 1..nb. */
RpStatus rp_sample_step_rows(const float* logprobs, int32_t vocab, const int32_t* active, int32_t n_active, int32_t n,
                             int32_t nb, const uint32_t* seeds, int32_t t, int32_t max_len, const void* params,
                             int32_t eos, int32_t pad, int32_t* seq, int32_t* tokens_next, float* cum_logprob,
                             int32_t* n_generated, int32_t* finished, void* stream);
RpStatus rp_sample_pool_step_rows(const float* logprobs, int32_t vocab, const int32_t* active, const int32_t* pos,
                                  int32_t n_active, int32_t n, int32_t nb, const uint32_t* seeds, int32_t max_len,
                                  const void* params, int32_t eos, int32_t pad, int32_t* seq, int32_t* tokens_next,
                                  float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream);
RpStatus rp_sample_pool_admit_rows(const int32_t* states, const uint32_t* new_seeds, const int32_t* n_live, int32_t m,
                                   int32_t n, int32_t nb, int32_t max_len, int32_t start_token, int32_t pad,
                                   uint32_t* seeds, int32_t* seq, float* cum_logprob, int32_t* n_generated,
                                   int32_t* finished, void* stream);

/* Teacher-forced seq2seq forward (T5ForConditionalGeneration(input_ids, attention_mask, labels)) over
 * `batch` (source, target) pairs packed varlen; DESIGN.md section 10.  src_cu / tgt_cu are HOST int32
 * [batch + 1] prefix sums (start at 0): source b is rows src_cu[b] .. src_cu[b+1] of enc_bf16, target b
 * positions tgt_cu[b] .. tgt_cu[b+1] of tokens / labels.  Every source and target holds at most 8192
 * tokens; a pair may be empty (0 target tokens), a non-empty target needs a non-empty source.
 *   enc_bf16        device bf16 [src_cu[batch], d_model]: rp_encode_hidden over the sources
 *   tokens          device int32 [tgt_cu[batch]]: decoder input ids (labels shifted right, start token first)
 *   labels          device int32 [tgt_cu[batch]]: target ids; < 0 (HF's -100) is ignored
 *   label_logprobs  device fp32 [tgt_cu[batch]]: log p(label), 0 where ignored
 *   loss_sum_count  device fp64 [2]: sum of -log p over the counted labels, their count (a fixed-order sum)
 *   logprob_rows    NULL or device fp32 [tgt_cu[batch], vocab]: every position's log_softmax row
 * labels >= vocab are outside the contract (the host layer rejects them); they come out as ignored.
 * A pair's outputs do not depend on the other pairs of the launch.  It reads a second, interleaved copy
 * of the FFN-in weights that rp_decoder_create packs (2 * layers * d_ff * d_model bf16 bytes).
 * Workspace: rp_decoder_forward_workspace_bytes (0 on bad arguments, rp_last_error says why). */
size_t   rp_decoder_forward_workspace_bytes(const RpDecoder* dec, const int32_t* src_cu, const int32_t* tgt_cu,
                                            int32_t batch);
RpStatus rp_decoder_forward(RpDecoder* dec, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                            const int32_t* labels, const int32_t* tgt_cu, int32_t batch, float* label_logprobs,
                            double* loss_sum_count, float* logprob_rows, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Gradients of the teacher-forced seq2seq loss (HF's: the mean of -log p over the counted labels) with respect to the
 * decoder's parameters and to the encoder output; DESIGN.md section 11.  Arguments and bounds are rp_decoder_forward's;
 * label_logprobs and loss_sum_count come out as rp_decoder_forward's bits.  Additionally vocab_size must be a multiple
 * of 64 (RP_E_UNSUPPORTED otherwise).
 *
 * Flat gradient buffer (fp32): rp_decoder_grad_layout writes the rp_decoder_grad_tensors(dec) + 1 element offsets
 * (last = total length incl. padding); every tensor starts at a multiple of 64 elements.  Order, HF shapes:
 *   shared [V, D] | lm_head [V, D] (absent when the decoder was created with tie_word_embeddings: the head's gradient
 *   is then added into shared) | rel_bias [buckets, H] | final_ln [D] | per layer: ln_self, q, k, v, o, ln_cross, cq,
 *   ck, cv, co, ln_ff, wi_0, wi_1, wo
 *   grads   device fp32 [layout total]: every element of every tensor is overwritten with d loss / d parameter; the
 *           padding gaps are left untouched
 *   d_enc   NULL or device fp32 [src_cu[batch], d_model]: d loss / d enc_bf16
 *           (the layers' cross K | V terms are added one after another in the backward's order, last layer first)
 * If no label is counted every gradient is 0 and the count comes back as 0.  No floating-point atomic touches device
 * memory: two calls with the same arguments give the same bits; a pair's d_enc rows times the count do not depend on
 * the other pairs of the call.
 * Choices: the transposed bf16 weights of the input-gradient GEMMs are made per call, one at a time, in a workspace
 * matrix of max(3 H d_kv d_model, 2 d_ff d_model, V d_model) bf16 (no second resident copy of the decoder); the gate /
 * up pre-activations and the RMSNorm statistics are recomputed, everything else the backward reads is saved.
 * Workspace, with Tp / Sp the target / source token totals rounded up to 128, I = H d_kv, L layers, all rounded to 256 B:
 *   (3L+1) Tp D 6 + L (Tp (3I + 3I + F) 2 + Sp 2I 2 + 2 H Tp 4) + Tp V 6 + Tp D 10 + Tp F 16 + Tp 5I 2 + Sp 2I 2
 *   + H Tp 4 + blocks H (2 max_distance + 1) 4 + transposed weight + Sp D 2 + the cu arrays and work lists
 * (rp_decoder_loss_grad_workspace_bytes; 0 on bad arguments, rp_last_error says why).  Bad arguments return
 * RP_E_INVALID / RP_E_UNSUPPORTED / RP_E_WORKSPACE and nothing is launched or written. */
int32_t  rp_decoder_grad_tensors(const RpDecoder* dec);                  /* 3 (+ 1 untied) + 14 * layers */
RpStatus rp_decoder_grad_layout(const RpDecoder* dec, int64_t* offsets /* [tensors + 1] */);
size_t   rp_decoder_loss_grad_workspace_bytes(const RpDecoder* dec, const int32_t* src_cu, const int32_t* tgt_cu,
                                              int32_t batch);
RpStatus rp_decoder_loss_grad(RpDecoder* dec, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                              const int32_t* labels, const int32_t* tgt_cu, int32_t batch, float* label_logprobs,
                              double* loss_sum_count, float* grads, float* d_enc, void* workspace,
                              size_t workspace_bytes, void* stream);
/* rp_decoder_loss_grad in T5's training mode: dropout with probability p in [0, 1) at HF's decoder
 * sites - the embeddings, both attentions' probabilities, the three residual branches and the gated product of every layer,
 * the final norm's output (the RP_DROP_SITE_DEC_* sites of rp_dbg_dropout_mask above).  Counter-based masks from `seed`:
 * the backward regenerates them, nothing is stored, the same (inputs, p, seed) give the same bits.  Each mask multiplies the
 * fp32 value before its rounding; the probabilities are masked after the row sum (the normaliser is the undropped one).
 * label_logprobs / loss_sum_count are the DROPPED model's.  d_enc carries no mask of its own: the encoder's final site
 * belongs to rp_train_backward_hidden_dropout; hand both halves the same seed (the site numbers are disjoint).
 * p = 0 gives rp_decoder_loss_grad's bits.  The workspace function returns rp_decoder_loss_grad_workspace_bytes' size: the
 * masked bf16 gradient of a residual branch is written by the cast that precedes the branch either way. */
size_t   rp_decoder_loss_grad_dropout_workspace_bytes(const RpDecoder* dec, const int32_t* src_cu, const int32_t* tgt_cu,
                                                      int32_t batch);
RpStatus rp_decoder_loss_grad_dropout(RpDecoder* dec, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                                      const int32_t* labels, const int32_t* tgt_cu, int32_t batch, float p, uint32_t seed,
                                      float* label_logprobs, double* loss_sum_count, float* grads, float* d_enc,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* Refresh every resident copy of the decoder's weights from fp32 masters (after an optimizer step); DESIGN.md section 14.
 *   params  device fp32 [layout total], 16-byte aligned, in exactly rp_decoder_grad_layout's order and offsets (with the
 *           tied head, lm_head is taken from shared)
 * Afterwards the fp32 embedding and norm vectors, the bf16 operands (lm_head, the fused self QKV, o, cross q / o, the
 * cross K | V concatenation of all layers, wi_0 | wi_1, wo), the interleaved FFN-in copy and the expanded bias table hold
 * the bits rp_decoder_create(..., RP_DT_F32, ...) packs from the same values: every element is rounded once, from the
 * master.  One grid-stride launch over a device-resident descriptor table built at create; launch-only (no allocation,
 * host copy or synchronisation), everything on `stream`.  Profile class RP_K_OPTIMIZER.  A null dec or params returns
 * RP_E_INVALID and nothing is launched. */
RpStatus rp_decoder_load_params(RpDecoder* dec, const float* params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REPROVER_HIP_H */
