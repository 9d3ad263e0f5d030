// libreprover_hip - the teacher-forced seq2seq forward of the tactic generator's T5 decoder (include/reprover_hip.h,
// DESIGN.md section 10): T5ForConditionalGeneration(input_ids, attention_mask, labels) over B (source, target) pairs
// packed varlen, the decoder side in one launch sequence.
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
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  if (n_tgt == 0) {
    const double zero[2] = {0.0, 0.0};
    RP_HIP(hipMemcpyWithStream(loss_sum_count, zero, sizeof zero, hipMemcpyHostToDevice, s));
    return RP_OK;
  }
  // metadata: the cu arrays and the attention work list {pair, first query} (128-query blocks of non-empty targets)
  std::vector<int32_t> meta(2 * (batch + 1));
  std::copy(src_cu, src_cu + batch + 1, meta.begin());
  std::copy(tgt_cu, tgt_cu + batch + 1, meta.begin() + batch + 1);
  for (int b = 0; b < batch; ++b)
    for (int q0 = 0; q0 < tgt_cu[b + 1] - tgt_cu[b]; q0 += FA_Q) {
      meta.push_back(b);
      meta.push_back(q0);
    }
  const int n_work = (int)(meta.size() - 2 * (batch + 1)) / 2;
  RP_HIP(hipMemcpyWithStream(w.meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s));
  const int32_t* d_src_cu = w.meta;
  const int32_t* d_tgt_cu = w.meta + batch + 1;
  const int2* d_work = reinterpret_cast<const int2*>(w.meta + 2 * (batch + 1));

  const int Tp = (int)align_up(n_tgt, FWD_BN), Sp = (int)align_up(n_src, FWD_BN);
  const dim3 att_grid(H * n_work);
  hipLaunchKernelGGL(dec_embed_kernel, dim3(n_tgt), dim3(256), 0, s, tokens, d->embed, w.x, D, V);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    // self-attention: x += o(attn(rmsnorm(x))), causal inside each pair
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(n_tgt), dim3(256), 0, s, w.x, l.ln_self, w.h, D, eps, 1.f);
    if ((st = fwd_gemm(w.h, n_tgt, Tp, l.wqkv, 3 * inner, D, EpiDecBf16{w.qkv, 3 * inner, 3 * inner, n_tgt}, s,
                       RP_K_GEMM_QKV)))
      return st;
    hipLaunchKernelGGL(dec_flash_kernel<true>, att_grid, dim3(256), 0, s, w.qkv, 3 * inner, w.qkv, 3 * inner, inner,
                       2 * inner, d_tgt_cu, d_tgt_cu, d_work, d->bias_tab, d->nbias, w.att, inner, (float*)nullptr, 0);
    if ((st = fwd_gemm(w.att, n_tgt, Tp, l.wo, D, inner, EpiDecF32<true>{w.x, D, D, n_tgt}, s, RP_K_GEMM_O))) return st;
    // cross-attention: the pair's queries over its own source's K / V (this layer's, from one GEMM over all sources)
    if ((st = fwd_gemm((const bf16_t*)enc_bf16, n_src, Sp, d->cross_kv_w + (size_t)2 * i * inner * D, 2 * inner, D,
                       EpiDecBf16{w.ckv, 2 * inner, 2 * inner, n_src}, s, RP_K_GEMM_QKV)))
      return st;
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(n_tgt), dim3(256), 0, s, w.x, l.ln_cross, w.h, D, eps, 1.f);
    if ((st = fwd_gemm(w.h, n_tgt, Tp, l.cq, inner, D, EpiDecBf16{w.qkv, inner, inner, n_tgt}, s, RP_K_GEMM_QKV)))
      return st;
    hipLaunchKernelGGL(dec_flash_kernel<false>, att_grid, dim3(256), 0, s, w.qkv, inner, w.ckv, 2 * inner, 0, inner,
                       d_tgt_cu, d_src_cu, d_work, (const float*)nullptr, 1, w.att, inner, (float*)nullptr, 0);
    if ((st = fwd_gemm(w.att, n_tgt, Tp, l.co, D, inner, EpiDecF32<true>{w.x, D, D, n_tgt}, s, RP_K_GEMM_O))) return st;
    // gated-GELU FFN
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(n_tgt), dim3(256), 0, s, w.x, l.ln_ff, w.h, D, eps, 1.f);
    if ((st = fwd_gemm(w.h, n_tgt, Tp, d->wi_il + (size_t)i * 2 * F * D, 2 * F, D, EpiDecGeglu{w.ff, F, F, n_tgt}, s,
                       RP_K_GEMM_WI)))
      return st;
    if ((st = fwd_gemm(w.ff, n_tgt, Tp, l.wo2, D, F, EpiDecF32<true>{w.x, D, D, n_tgt}, s, RP_K_GEMM_WO))) return st;
  }
  const float scale = d->tied ? 1.f / sqrtf((float)D) : 1.f;
  hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(n_tgt), dim3(256), 0, s, w.x, d->final_ln, w.h, D, eps, scale);
  if ((st = fwd_gemm(w.h, n_tgt, Tp, d->lm_head, V, D, EpiDecF32<false>{w.logits, V, V, n_tgt}, s, RP_K_GEMM_O))) return st;
  hipLaunchKernelGGL(fwd_loss_row_kernel, dim3(n_tgt), dim3(256), 0, s, w.logits, V, labels, label_logprobs, logprob_rows);
  hipLaunchKernelGGL(fwd_loss_reduce_kernel, dim3(1), dim3(256), 0, s, label_logprobs, labels, n_tgt, V, loss_sum_count);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
