// libreprover_hip - the teacher-forced seq2seq forward of the tactic generator's T5 decoder (include/reprover_hip.h,
// DESIGN.md section 10): T5ForConditionalGeneration(input_ids, attention_mask, labels) over B (source, target) pairs
// packed varlen, the decoder side in one launch sequence (fwd_launch_layers, rp_decoder_forward_kernels.h; this file
// holds the entry point: checks, workspace, the one-buffer-per-kind filling of the sequence's buffer view).
//
// Per layer: RMSNorm -> fused self QKV GEMM -> causal varlen flash attention (bias by distance query - key) -> o GEMM +
// residual -> RMSNorm -> cross q GEMM -> varlen flash cross-attention over the pair's own source (cross K/V: one GEMM per
// layer over every source, into a buffer reused layer by layer) -> co GEMM + residual -> RMSNorm -> gated-GELU FFN (two
// GEMMs, the second + residual); then the final norm, lm_head, per-row log-softmax + label gather and one fixed-order
// reduction of the loss.  The GEMMs run on the encoder's MFMA tiles (rp_encoder_kernels.h launch_gemm_cfg, 64 x 128 x 64)
// with the decoder's own epilogues.
//
// Every output element is computed by a reduction whose order depends only on its own pair's lengths (GEMM: K ascending;
// attention: 64-key tiles counted from the pair's first key; rows: fixed butterflies), never on which other pairs share
// the launch or where the pair sits in it: a pair's log-probs are the same bits alone, batched or permuted.
#include "rp_decoder_forward_kernels.h"

extern "C" size_t rp_decoder_forward_workspace_bytes(const RpDecoder* d, const int32_t* src_cu, const int32_t* tgt_cu,
                                                     int32_t batch) {
  int n_src = 0, n_tgt = 0;
  if (fwd_check_model(d) != RP_OK || fwd_check_cu(src_cu, tgt_cu, batch, n_src, n_tgt) != RP_OK) return 0;
  return fwd_carve(d, batch, n_src, n_tgt, nullptr).bytes;
}

extern "C" RpStatus rp_decoder_forward(RpDecoder* d, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                                       const int32_t* labels, const int32_t* tgt_cu, int32_t batch,
                                       float* label_logprobs, double* loss_sum_count, float* logprob_rows, void* ws,
                                       size_t ws_bytes, void* stream_) {
  RpStatus st = fwd_check_model(d);
  if (st) return st;
  int n_src = 0, n_tgt = 0;
  if ((st = fwd_check_cu(src_cu, tgt_cu, batch, n_src, n_tgt))) return st;
  RP_REQUIRE(loss_sum_count, "null loss_sum_count");
  RP_REQUIRE(n_tgt == 0 || (enc_bf16 && tokens && labels && label_logprobs), "null argument");
  const FwdWs w = fwd_carve(d, batch, n_src, n_tgt, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream_;
  if (n_tgt == 0) {
    const double zero[2] = {0.0, 0.0};
    RP_HIP(hipMemcpyWithStream(loss_sum_count, zero, sizeof zero, hipMemcpyHostToDevice, s));
    return RP_OK;
  }
  std::vector<int32_t> meta;
  const int n_work = fwd_build_meta(src_cu, tgt_cu, batch, meta);
  RP_HIP(hipMemcpyWithStream(w.meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s));
  // one buffer per kind, reused by every layer: the stream is updated in place, nothing is kept for a backward
  const FwdLayerBufs one{w.x, w.x, w.x, w.x, w.h, w.h, w.h, w.qkv, w.qkv, w.ckv, w.att, w.att, w.ff, nullptr, nullptr, 0};
  const std::vector<FwdLayerBufs> bufs(d->cfg.num_layers, one);
  return fwd_launch_layers(d, enc_bf16, tokens, labels, batch, n_src, n_tgt, w.meta, n_work, bufs.data(),
                           FwdFinalBufs{w.x, w.h, w.logits}, label_logprobs, loss_sum_count, logprob_rows, s);
}
