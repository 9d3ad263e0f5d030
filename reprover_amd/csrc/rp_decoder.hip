// libreprover_hip - the tactic generator's T5 decoder (include/reprover_hip.h).
//
// One beam-search step for nb <= 64 beams: per layer RMSNorm -> fused self QKV -> causal self-attention over the
// ancestry-addressed cache -> o + residual -> RMSNorm -> cross q -> cross-attention over the source -> o + residual ->
// gated-GELU FFN; then the final norm, lm_head and log_softmax.  Precision: bf16 weights and GEMM operands, fp32
// accumulation, statistics, softmax and residual stream, fp32 log-probs.
//
// Every output element of every kernel here is computed by a reduction whose order depends only on the shapes (K, the
// key count), never on which other rows share the launch or where the row sits in it: a row's log-probs are the same
// bits batched or alone.
#include <algorithm>
#include <vector>

#include "rp_decoder_common.h"

using namespace rp;

namespace {

template <typename T>
__global__ void dec_to_bf16_kernel(bf16_t* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = f2bf((float)src[i]);
}
template <>
__global__ void dec_to_bf16_kernel<bf16_t>(bf16_t* __restrict__ dst, const bf16_t* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
template <typename T>
__global__ void dec_to_f32_kernel(float* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = (float)src[i];
}
template <>
__global__ void dec_to_f32_kernel<bf16_t>(float* __restrict__ dst, const bf16_t* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = bf2f(src[i]);
}

// One (head, beam) per workgroup: dec_attention_row (rp_decoder_common.h) over the beam's q row, ancestry row and out row.
__global__ __launch_bounds__(256) void dec_attention_kernel(const bf16_t* __restrict__ q, int ldq,
                                                            const bf16_t* __restrict__ kv, int ldkv, int koff, int voff,
                                                            int rows, const int32_t* __restrict__ anc, int astride,
                                                            const float* __restrict__ tab, int nbias, int len,
                                                            bf16_t* __restrict__ out, int ldo) {
  extern __shared__ float s_sc[];
  const int h = blockIdx.x, b = blockIdx.y;
  dec_attention_row(s_sc, q + (size_t)b * ldq, kv, ldkv, koff, voff, rows, anc ? anc + (size_t)b * astride : nullptr, tab,
                    nbias, len, out + (size_t)b * ldo, h);
}

// cache row t * nb + b of layer l <- the k, v columns of qkv[b]
__global__ __launch_bounds__(256) void dec_store_kv_kernel(const bf16_t* __restrict__ qkv, int inner,
                                                           bf16_t* __restrict__ cache, int row0) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < 2 * inner; c += 256)
    cache[(size_t)(row0 + b) * 2 * inner + c] = qkv[(size_t)b * 3 * inner + inner + c];
}

// ---- beam selection ---------------------------------------------------------------------------------------------------
// per beam row: the top kr keys of logprobs[b, :] + running[b]
__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ lp, const float* __restrict__ running,
                                                            int V, int kr, uint64_t* __restrict__ cand) {
  __shared__ uint64_t s[DEC_SELECT_ROW];
  const int b = blockIdx.x;
  const float rb = running[b];
  for (int i = threadIdx.x; i < DEC_SELECT_ROW; i += 256)
    s[i] = (i < V) ? sel_key(lp[(size_t)b * V + i] + rb, (uint32_t)(b * V + i)) : 0ull;
  bitonic_desc(s, DEC_SELECT_ROW);
  for (int i = threadIdx.x; i < kr; i += 256) cand[(size_t)b * kr + i] = s[i];
}

__global__ __launch_bounds__(1024) void beam_merge_kernel(const uint64_t* __restrict__ cand, int n, int V, int k,
                                                          float* __restrict__ scores, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ parents) {
  __shared__ uint64_t s[DEC_MERGE];
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = threadIdx.x; i < np2; i += 1024) s[i] = (i < n) ? cand[i] : 0ull;
  bitonic_desc(s, np2);
  for (int i = threadIdx.x; i < k; i += 1024) {
    const uint32_t idx = ~(uint32_t)s[i];
    scores[i] = key_score(s[i]);
    tokens[i] = (int32_t)(idx % (uint32_t)V);
    parents[i] = (int32_t)(idx / (uint32_t)V);
  }
}

}  // namespace

namespace {
struct DecWs {
  bf16_t* ckv;    // [S, L * 2 * inner]
  bf16_t* cache;  // [L][max_len * nb, 2 * inner]
  float* x;       // [nb, D]
  bf16_t* h;      // [nb, D] + [nb, F]
  bf16_t* qkv;    // [nb, 3 * inner]
  bf16_t* att;    // [nb, inner]
  size_t bytes;
};
DecWs dec_carve(const RpDecoder* d, int nb, int max_len, int S, char* base) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, L = d->cfg.num_layers;
  DecWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  w.ckv = (bf16_t*)take((size_t)S * L * 2 * inner * 2);
  w.cache = (bf16_t*)take(L * (size_t)max_len * nb * 2 * inner * 2);
  w.x = (float*)take((size_t)nb * D * 4);
  w.h = (bf16_t*)take((size_t)nb * (D + F) * 2);  // the normed rows, then the FFN's inner rows
  w.qkv = (bf16_t*)take((size_t)nb * 3 * inner * 2);
  w.att = (bf16_t*)take((size_t)nb * inner * 2);
  w.bytes = off;
  return w;
}

template <typename T>
RpStatus dec_pack(RpDecoder* d, const RpT5DecoderWeights* w) {
  const RpT5Config& c = d->cfg;
  const size_t D = c.d_model, F = c.d_ff, inner = d->inner, V = c.vocab_size, L = c.num_layers;
  auto alloc = [&](size_t bytes, void** p) -> RpStatus {
    RP_HIP(hipMalloc(p, bytes));
    d->allocs.push_back(*p);
    return RP_OK;
  };
  auto bf = [&](bf16_t* dst, const void* src, size_t n) {
    hipLaunchKernelGGL((dec_to_bf16_kernel<T>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, 0, dst,
                       (const T*)src, (int64_t)n);
  };
  auto f32 = [&](float* dst, const void* src, size_t n) {
    hipLaunchKernelGGL((dec_to_f32_kernel<T>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, 0, dst,
                       (const T*)src, (int64_t)n);
  };
  RpStatus st;
  if ((st = alloc(V * D * 4, (void**)&d->embed))) return st;
  f32(d->embed, w->embed, V * D);
  if ((st = alloc(D * 4, (void**)&d->final_ln))) return st;
  f32(d->final_ln, w->final_ln, D);
  if ((st = alloc(V * D * 2, (void**)&d->lm_head))) return st;
  bf(d->lm_head, w->lm_head, V * D);
  if ((st = alloc(L * 2 * inner * D * 2, (void**)&d->cross_kv_w))) return st;
  d->layers.resize(L);
  for (size_t i = 0; i < L; ++i) {
    const RpT5DecoderLayerWeights& s = w->layers[i];
    RpDecoder::Layer& l = d->layers[i];
    if ((st = alloc(D * 4, (void**)&l.ln_self)) || (st = alloc(D * 4, (void**)&l.ln_cross)) ||
        (st = alloc(D * 4, (void**)&l.ln_ff)) || (st = alloc(3 * inner * D * 2, (void**)&l.wqkv)) ||
        (st = alloc(D * inner * 2, (void**)&l.wo)) || (st = alloc(inner * D * 2, (void**)&l.cq)) ||
        (st = alloc(D * inner * 2, (void**)&l.co)) || (st = alloc(2 * F * D * 2, (void**)&l.wi)) ||
        (st = alloc(D * F * 2, (void**)&l.wo2)))
      return st;
    f32(l.ln_self, s.ln_self, D);
    f32(l.ln_cross, s.ln_cross, D);
    f32(l.ln_ff, s.ln_ff, D);
    bf(l.wqkv, s.q, inner * D);
    bf(l.wqkv + inner * D, s.k, inner * D);
    bf(l.wqkv + 2 * inner * D, s.v, inner * D);
    bf(l.wo, s.o, D * inner);
    bf(l.cq, s.cq, inner * D);
    bf(l.co, s.co, D * inner);
    bf(d->cross_kv_w + (2 * i) * inner * D, s.ck, inner * D);
    bf(d->cross_kv_w + (2 * i + 1) * inner * D, s.cv, inner * D);
    bf(l.wi, s.wi_0, F * D);
    bf(l.wi + F * D, s.wi_1, F * D);
    bf(l.wo2, s.wo, D * F);
    RP_CHECK_LAUNCH();
  }
  // the teacher-forced forward's FFN-in operand (rp_decoder_forward.hip): 2 L d_ff d_model bf16 bytes more
  if (F % 32 == 0) {
    if ((st = alloc(L * 2 * F * D * 2, (void**)&d->wi_il))) return st;
    for (size_t i = 0; i < L; ++i)
      hipLaunchKernelGGL(dec_interleave_kernel, dim3((unsigned)(2 * F)), dim3(256), 0, 0, d->wi_il + i * 2 * F * D,
                         d->layers[i].wi, (int)F, (int)D);
    RP_CHECK_LAUNCH();
  }
  // relative-position bias by distance j = query - key in [0, nbias): beyond 2 * max_distance every bucket is the last
  const int nbk = c.rel_num_buckets, H = c.num_heads;
  d->nbias = 2 * c.rel_max_distance + 1;
  std::vector<float> raw((size_t)nbk * H);
  {
    float* tmp;
    RP_HIP(hipMalloc((void**)&tmp, raw.size() * 4));
    hipLaunchKernelGGL((dec_to_f32_kernel<T>), dim3((nbk * H + 255) / 256), dim3(256), 0, 0, tmp, (const T*)w->rel_bias,
                       (int64_t)nbk * H);
    RP_HIP(hipMemcpy(raw.data(), tmp, raw.size() * 4, hipMemcpyDeviceToHost));
    RP_HIP(hipFree(tmp));
  }
  std::vector<float> tab((size_t)H * d->nbias);
  for (int j = 0; j < d->nbias; ++j) {
    const int bk = rp_relative_position_bucket_causal(-j, nbk, c.rel_max_distance);
    for (int h = 0; h < H; ++h) tab[(size_t)h * d->nbias + j] = raw[(size_t)bk * H + h];
  }
  if ((st = alloc(tab.size() * 4, (void**)&d->bias_tab))) return st;
  RP_HIP(hipMemcpy(d->bias_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  RP_HIP(hipDeviceSynchronize());
  return RP_OK;
}
}  // namespace

// modeling_t5.py _relative_position_bucket, bidirectional=False: n = -min(rel, 0); exact below num_buckets / 2, then
// logarithmic up to max_distance; float32 arithmetic as torch evaluates it.
extern "C" int32_t rp_relative_position_bucket_causal(int32_t rel, int32_t num_buckets, int32_t max_distance) {
  const int n = rel < 0 ? -rel : 0;
  const int max_exact = num_buckets / 2;
  if (n < max_exact) return n;
  float ratio = (float)n / (float)max_exact;
  float t = logf(ratio) / (float)log((double)max_distance / (double)max_exact) * (float)(num_buckets - max_exact);
  int large = max_exact + (int)t;
  return large > num_buckets - 1 ? num_buckets - 1 : large;
}

extern "C" RpStatus rp_decoder_create(const RpT5Config* cfg, const RpT5DecoderWeights* weights, int32_t weight_dtype,
                                      RpDecoder** out) {
  RP_REQUIRE(cfg && weights && out && weights->layers && weights->embed && weights->lm_head, "null argument");
  if (cfg->d_kv != 64) return fail(RP_E_UNSUPPORTED, "d_kv=%d: the decoder kernels implement d_kv=64", cfg->d_kv);
  if (cfg->num_layers < 1) return fail(RP_E_INVALID, "num_layers (decoder layers) = %d", cfg->num_layers);
  if (cfg->d_model % 8 || cfg->d_ff % 8 || cfg->d_model > DEC_MAX_KIT * 512 || cfg->d_ff > DEC_MAX_KIT * 512)
    return fail(RP_E_UNSUPPORTED, "d_model=%d / d_ff=%d: multiples of 8, at most %d", cfg->d_model, cfg->d_ff,
                DEC_MAX_KIT * 512);
  if (cfg->vocab_size < 1 || cfg->vocab_size > DEC_SELECT_ROW)
    return fail(RP_E_UNSUPPORTED, "vocab_size=%d: the beam selection implements vocab <= %d", cfg->vocab_size,
                DEC_SELECT_ROW);
  RP_REQUIRE(cfg->rel_num_buckets >= 2 && cfg->rel_max_distance > cfg->rel_num_buckets / 2, "relative-position config");
  RP_REQUIRE(weight_dtype == RP_DT_F32 || weight_dtype == RP_DT_BF16, "weight_dtype");
  RpDecoder* d = new RpDecoder();
  d->cfg = *cfg;
  d->inner = cfg->num_heads * cfg->d_kv;
  d->tied = weights->tie_word_embeddings ? 1 : 0;
  RpStatus st = weight_dtype == RP_DT_F32 ? dec_pack<float>(d, weights) : dec_pack<bf16_t>(d, weights);
  if (st != RP_OK) {
    rp_decoder_destroy(d);
    return st;
  }
  *out = d;
  return RP_OK;
}

extern "C" void rp_decoder_destroy(RpDecoder* d) {
  if (!d) return;
  for (void* p : d->allocs) (void)hipFree(p);
  delete d;
}

static RpStatus dec_check_shape(const RpDecoder* d, int nb, int max_len, int S) {
  RP_REQUIRE(d, "null decoder");
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "num_beams=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(max_len >= 1 && max_len <= DEC_MAX_KEYS, "max_len=%d (1..%d)", max_len, DEC_MAX_KEYS);
  RP_REQUIRE(S >= 1 && S <= DEC_MAX_KEYS, "src_len=%d (1..%d)", S, DEC_MAX_KEYS);
  return RP_OK;
}

extern "C" size_t rp_decoder_workspace_bytes(const RpDecoder* d, int32_t nb, int32_t max_len, int32_t S) {
  if (!d || nb < 1 || nb > DEC_MAX_BEAMS || max_len < 1 || max_len > DEC_MAX_KEYS || S < 1 || S > DEC_MAX_KEYS) return 0;
  return dec_carve(d, nb, max_len, S, nullptr).bytes;
}

extern "C" RpStatus rp_decoder_cross_kv(RpDecoder* d, const void* enc, int32_t S, int32_t nb, int32_t max_len, void* ws,
                                        size_t ws_bytes, void* stream_) {
  RpStatus st = dec_check_shape(d, nb, max_len, S);
  if (st) return st;
  RP_REQUIRE(enc, "null encoder states");
  const DecWs w = dec_carve(d, nb, max_len, S, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  const int D = d->cfg.d_model, NKV = d->cfg.num_layers * 2 * d->inner;
  return launch_dec_gemm<EPI_BF16>((const bf16_t*)enc, D, S, d->cross_kv_w, NKV, D, w.ckv, NKV, (hipStream_t)stream_);
}

extern "C" RpStatus rp_decoder_step(RpDecoder* d, const int32_t* tokens, const int32_t* anc, int32_t astride, int32_t nb,
                                    int32_t t, int32_t max_len, int32_t S, float* logprobs, void* ws, size_t ws_bytes,
                                    void* stream_) {
  RpStatus st = dec_check_shape(d, nb, max_len, S);
  if (st) return st;
  RP_REQUIRE(tokens && anc && logprobs, "null argument");
  RP_REQUIRE(t >= 0 && t < max_len, "t=%d outside [0, max_len=%d)", t, max_len);
  RP_REQUIRE(astride >= t + 1, "anc_stride=%d < t + 1 = %d", astride, t + 1);
  const DecWs w = dec_carve(d, nb, max_len, S, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream_;
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  const int rows = max_len * nb, ldckv = L * 2 * inner;
  hipLaunchKernelGGL(dec_embed_kernel, dim3(nb), dim3(256), 0, s, tokens, d->embed, w.x, D, V);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    bf16_t* cache = w.cache + (size_t)i * rows * 2 * inner;
    // self-attention (modeling_t5.py T5LayerSelfAttention): x += o(attn(rmsnorm(x)))
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, w.x, l.ln_self, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_BF16>(w.h, D, nb, l.wqkv, 3 * inner, D, w.qkv, 3 * inner, s))) return st;
    hipLaunchKernelGGL(dec_store_kv_kernel, dim3(nb), dim3(256), 0, s, w.qkv, inner, cache, t * nb);
    hipLaunchKernelGGL(dec_attention_kernel, dim3(H, nb), dim3(256), (t + 1) * sizeof(float), s, w.qkv, 3 * inner,
                       cache, 2 * inner, 0, inner, rows, anc, astride, d->bias_tab, d->nbias, t + 1, w.att, inner);
    if ((st = launch_dec_gemm<EPI_RESID>(w.att, inner, nb, l.wo, D, inner, w.x, D, s))) return st;
    // cross-attention (T5LayerCrossAttention): no position bias, all S source keys
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, w.x, l.ln_cross, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_BF16>(w.h, D, nb, l.cq, inner, D, w.qkv, inner, s))) return st;
    hipLaunchKernelGGL(dec_attention_kernel, dim3(H, nb), dim3(256), S * sizeof(float), s, w.qkv, inner, w.ckv, ldckv,
                       2 * i * inner, (2 * i + 1) * inner, S, (const int32_t*)nullptr, 0, (const float*)nullptr, 1, S,
                       w.att, inner);
    if ((st = launch_dec_gemm<EPI_RESID>(w.att, inner, nb, l.co, D, inner, w.x, D, s))) return st;
    // gated-GELU FFN (T5LayerFF / T5DenseGatedActDense)
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, w.x, l.ln_ff, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_GEGLU>(w.h, D, nb, l.wi, F, D, w.h + (size_t)nb * D, F, s))) return st;
    if ((st = launch_dec_gemm<EPI_RESID>(w.h + (size_t)nb * D, F, nb, l.wo2, D, F, w.x, D, s))) return st;
  }
  const float scale = d->tied ? 1.f / sqrtf((float)D) : 1.f;
  hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, w.x, d->final_ln, w.h, D, eps, scale);
  if ((st = launch_dec_gemm<EPI_F32>(w.h, D, nb, d->lm_head, V, D, logprobs, V, s))) return st;
  hipLaunchKernelGGL(dec_log_softmax_kernel, dim3(nb), dim3(256), 0, s, logprobs, V);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_beam_select(const float* lp, const float* running, int32_t nb, int32_t V, int32_t k, float* scores,
                                   int32_t* tokens, int32_t* parents, void* ws, size_t ws_bytes, void* stream_) {
  RP_REQUIRE(lp && running && scores && tokens && parents, "null argument");
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(V >= 1 && V <= DEC_SELECT_ROW, "vocab=%d (1..%d)", V, DEC_SELECT_ROW);
  RP_REQUIRE(k >= 1 && k <= DEC_SELECT_MAX_K && k <= nb * V, "k=%d (1..min(%d, nb * vocab))", k, DEC_SELECT_MAX_K);
  const int kr = std::min(k, V);  // a row contributes at most k candidates
  const size_t need = (size_t)nb * kr * sizeof(uint64_t);
  if (!ws || ws_bytes < need) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream_;
  uint64_t* cand = (uint64_t*)ws;
  hipLaunchKernelGGL(beam_row_topk_kernel, dim3(nb), dim3(256), 0, s, lp, running, V, kr, cand);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(1024), 0, s, cand, nb * kr, V, k, scores, tokens, parents);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
