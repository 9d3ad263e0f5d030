// libreprover_hip - batched tactic generation: one decode step for the beams of several proof states at once
// (include/reprover_hip.h rp_decoder_batch_*, rp_beam_select_batch; DESIGN.md section 9 "Batched generation").
//
// The rows of a step are the n_active * nb beams of the states that are still searching, packed slot by slot.  Embed,
// RMSNorm, every projection, lm_head and log_softmax are row-wise and run over all rows in one launch each; the two
// attentions run as one launch over (head, row), each row finding its state's cache, cross K/V and source length through
// the slot table passed by value.  Every output element keeps the reduction chain of its per-state counterpart in
// rp_decoder.hip (the kernels are the same source, rp_decoder_common.h, or - the interleaved GEMM - the same chain per
// (m, n) with several rows in flight), so a row's log-probs are the bits rp_decoder_step gives that state alone.
#include <algorithm>

#include "rp_decoder_common.h"

using namespace rp;

namespace rp {
// rp_set_option "dec_batch_gemm": 1 = dec_gemm_kernel at a larger grid.y (the default: 7 % faster at 8 states x 64 beams),
// 0 = the interleaved-row GEMM below (the A/B of tools/gen_bench.py --states; the same bits either way)
int g_dec_batch_gemm = 1;
}  // namespace rp

namespace {

constexpr int DECB_MAX_STATES = 32;   // states per call (a 32-bit mask checks the active list)
constexpr int DECB_MAX_ROWS = 1024;   // n * nb: 16 states of 64 beams, 32 of 32 or fewer
constexpr int DECB_GEMM_ROWS = 128;   // activation rows one workgroup streams past its weight rows

// per active slot: the state it carries and where that state's source sits in the packed cross K/V
struct DecbSlots {
  int32_t state[DECB_MAX_STATES];
  int32_t src_off[DECB_MAX_STATES];
  int32_t src_len[DECB_MAX_STATES];
};

// dec_gemm_kernel with R activation rows in flight per wave: the weight row stays in registers across DECB_GEMM_ROWS rows,
// the R rows' loads are issued together and their fma chains and butterflies are independent, so one row's load and
// cross-lane latency hides behind the others'.  Each (m, n) runs exactly dec_gemm_kernel's chain: lane l over the
// 16-byte pieces l, l + 64, ... of K from 0.f (absent pieces as zeros), then wave_sum64.  After the xor butterfly every
// lane holds the sum (fp32 addition commutes, so the lanes agree bit for bit); lane r stores row m + r.
template <int KIT, int EPI, int R>
__global__ __launch_bounds__(256) void decb_gemm_kernel(const bf16_t* __restrict__ A, int lda, int M,
                                                        const bf16_t* __restrict__ W, int N, int K,
                                                        void* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int nk = K >> 3;
  uint4 w0[KIT], w1[KIT];
#pragma unroll
  for (int i = 0; i < KIT; ++i) {
    const int j = lane + 64 * i;
    w0[i] = (j < nk) ? reinterpret_cast<const uint4*>(W + (size_t)n * K)[j] : make_uint4(0u, 0u, 0u, 0u);
    if constexpr (EPI == EPI_GEGLU)
      w1[i] = (j < nk) ? reinterpret_cast<const uint4*>(W + (size_t)(n + N) * K)[j] : make_uint4(0u, 0u, 0u, 0u);
  }
  const int m1 = min(M, (int)(blockIdx.y + 1) * DECB_GEMM_ROWS);
  for (int m = blockIdx.y * DECB_GEMM_ROWS; m < m1; m += R) {
    uint4 av[R][KIT];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint4* a = reinterpret_cast<const uint4*>(A + (size_t)min(m + r, m1 - 1) * lda);  // past the end: a live row again
#pragma unroll
      for (int i = 0; i < KIT; ++i) {
        const int j = lane + 64 * i;
        av[r][i] = (j < nk) ? a[j] : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    float acc0[R], acc1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc0[r] = 0.f;
      acc1[r] = 0.f;
#pragma unroll
      for (int i = 0; i < KIT; ++i) {
        acc0[r] = dot8(av[r][i], w0[i], acc0[r]);
        if constexpr (EPI == EPI_GEGLU) acc1[r] = dot8(av[r][i], w1[i], acc1[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc0[r] = wave_sum64(acc0[r]);
      if constexpr (EPI == EPI_GEGLU) acc1[r] = wave_sum64(acc1[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (lane == r && m + r < m1) {
        const size_t o = (size_t)(m + r) * ldo + n;
        if constexpr (EPI == EPI_BF16) reinterpret_cast<bf16_t*>(out)[o] = f2bf(acc0[r]);
        if constexpr (EPI == EPI_RESID) reinterpret_cast<float*>(out)[o] += acc0[r];
        if constexpr (EPI == EPI_F32) reinterpret_cast<float*>(out)[o] = acc0[r];
        if constexpr (EPI == EPI_GEGLU) reinterpret_cast<bf16_t*>(out)[o] = f2bf(gelu_tanh(acc0[r]) * acc1[r]);
      }
    }
  }
}

template <int EPI>
RpStatus launch_decb_gemm(const bf16_t* A, int lda, int M, const bf16_t* W, int N, int K, void* out, int ldo,
                          hipStream_t s) {
  if (g_dec_batch_gemm == 1) return launch_dec_gemm<EPI>(A, lda, M, W, N, K, out, ldo, s);
  const int kit = (K / 8 + 63) / 64;
  const dim3 grid((N + 3) / 4, (M + DECB_GEMM_ROWS - 1) / DECB_GEMM_ROWS);
  // rows in flight: 8 while a row is at most 4 pieces per lane (16 VGPRs), else 4: at most 128 VGPRs of activations
#define DECB_GEMM_CASE(I, R) \
  case I: hipLaunchKernelGGL((decb_gemm_kernel<I, EPI, R>), grid, dim3(256), 0, s, A, lda, M, W, N, K, out, ldo); break;
  switch (kit) {
    DECB_GEMM_CASE(1, 8) DECB_GEMM_CASE(2, 8) DECB_GEMM_CASE(3, 8) DECB_GEMM_CASE(4, 8)
    DECB_GEMM_CASE(5, 4) DECB_GEMM_CASE(6, 4) DECB_GEMM_CASE(7, 4) DECB_GEMM_CASE(8, 4)
    default: return fail(RP_E_UNSUPPORTED, "decoder GEMM K=%d > %d", K, DEC_MAX_KIT * 512);
  }
#undef DECB_GEMM_CASE
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// One (head, row) per workgroup, row = slot * nb + beam.  Self-attention (CROSS = false): the state's own cache of
// `rows` = max_len * nb rows at kv + state * state_stride, keys through the row's ancestry entries (local to that cache),
// len keys.  Cross-attention: the state's source rows of the packed cross K/V, all src_len keys, no bias.
template <bool CROSS>
__global__ __launch_bounds__(256) void decb_attention_kernel(const bf16_t* __restrict__ q, int ldq,
                                                             const bf16_t* __restrict__ kv, int ldkv, int koff, int voff,
                                                             int rows, size_t state_stride,
                                                             const int32_t* __restrict__ anc, int astride,
                                                             const float* __restrict__ tab, int nbias, int len, int nb,
                                                             DecbSlots slots, bf16_t* __restrict__ out, int ldo) {
  extern __shared__ float s_sc[];
  const int h = blockIdx.x, row = blockIdx.y;
  const int slot = row / nb;
  if constexpr (CROSS)
    dec_attention_row(s_sc, q + (size_t)row * ldq, kv + (size_t)slots.src_off[slot] * ldkv, ldkv, koff, voff,
                      slots.src_len[slot], nullptr, nullptr, 1, slots.src_len[slot], out + (size_t)row * ldo, h);
  else
    dec_attention_row(s_sc, q + (size_t)row * ldq, kv + (size_t)slots.state[slot] * state_stride, ldkv, koff, voff, rows,
                      anc + (size_t)row * astride, tab, nbias, len, out + (size_t)row * ldo, h);
}

// cache row row0 + beam of the row's state <- the k, v columns of qkv[row]
__global__ __launch_bounds__(256) void decb_store_kv_kernel(const bf16_t* __restrict__ qkv, int inner,
                                                            bf16_t* __restrict__ cache, size_t state_stride, int row0,
                                                            int nb, DecbSlots slots) {
  const int row = blockIdx.x, slot = row / nb, b = row - slot * nb;
  bf16_t* dst = cache + (size_t)slots.state[slot] * state_stride + (size_t)(row0 + b) * 2 * inner;
  for (int c = threadIdx.x; c < 2 * inner; c += 256) dst[c] = qkv[(size_t)row * 3 * inner + inner + c];
}

// beam_row_topk_kernel per state: row = slot * nb + b, keyed by the flat index b * V + i inside the state's own block
__global__ __launch_bounds__(256) void decb_row_topk_kernel(const float* __restrict__ lp, const float* __restrict__ running,
                                                            int V, int kr, int nb, uint64_t* __restrict__ cand) {
  __shared__ uint64_t s[DEC_SELECT_ROW];
  const int row = blockIdx.x, b = row % nb;
  const float rb = running[row];
  for (int i = threadIdx.x; i < DEC_SELECT_ROW; i += 256)
    s[i] = (i < V) ? sel_key(lp[(size_t)row * V + i] + rb, (uint32_t)(b * V + i)) : 0ull;
  bitonic_desc(s, DEC_SELECT_ROW);
  for (int i = threadIdx.x; i < kr; i += 256) cand[(size_t)row * kr + i] = s[i];
}

// beam_merge_kernel per state: workgroup a sorts the state's n = nb * kr candidates and writes its k winners
__global__ __launch_bounds__(1024) void decb_merge_kernel(const uint64_t* __restrict__ cand, int n, int V, int k,
                                                          float* __restrict__ scores, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ parents) {
  __shared__ uint64_t s[DEC_MERGE];
  const int a = blockIdx.x;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = threadIdx.x; i < np2; i += 1024) s[i] = (i < n) ? cand[(size_t)a * n + i] : 0ull;
  bitonic_desc(s, np2);
  for (int i = threadIdx.x; i < k; i += 1024) {
    const uint32_t idx = ~(uint32_t)s[i];
    scores[(size_t)a * k + i] = key_score(s[i]);
    tokens[(size_t)a * k + i] = (int32_t)(idx % (uint32_t)V);
    parents[(size_t)a * k + i] = (int32_t)(idx / (uint32_t)V);
  }
}

struct DecbWs {
  bf16_t* ckv;    // [sum S, L * 2 * inner]
  bf16_t* cache;  // [n][L][max_len * nb, 2 * inner]
  float* x;       // [n * nb, D]
  bf16_t* h;      // [n * nb, D] then [n * nb, F]
  bf16_t* qkv;    // [n * nb, 3 * inner]
  bf16_t* att;    // [n * nb, inner]
  size_t bytes;
};
DecbWs decb_carve(const RpDecoder* d, int n, int total_src, int nb, int max_len, char* base) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, L = d->cfg.num_layers, M = (size_t)n * nb;
  DecbWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  w.ckv = (bf16_t*)take((size_t)total_src * L * 2 * inner * 2);
  w.cache = (bf16_t*)take((size_t)n * L * max_len * nb * 2 * inner * 2);
  w.x = (float*)take(M * D * 4);
  w.h = (bf16_t*)take(M * (D + F) * 2);
  w.qkv = (bf16_t*)take(M * 3 * inner * 2);
  w.att = (bf16_t*)take(M * inner * 2);
  w.bytes = off;
  return w;
}

// the caps of a batched call; total_src = src_cu[n]
RpStatus decb_check(const RpDecoder* d, const int32_t* src_cu, int n, int nb, int max_len, int& total_src) {
  RP_REQUIRE(d, "null decoder");
  RP_REQUIRE(src_cu, "null src_cu");
  RP_REQUIRE(n >= 1 && n <= DECB_MAX_STATES, "states=%d (1..%d)", n, DECB_MAX_STATES);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "num_beams=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n * nb <= DECB_MAX_ROWS, "rows = states * num_beams = %d > %d", n * nb, DECB_MAX_ROWS);
  RP_REQUIRE(max_len >= 1 && max_len <= DEC_MAX_KEYS, "max_len=%d (1..%d)", max_len, DEC_MAX_KEYS);
  RP_REQUIRE(src_cu[0] == 0, "src_cu[0]=%d, not 0", src_cu[0]);
  for (int b = 0; b < n; ++b) {
    const int64_t S = (int64_t)src_cu[b + 1] - src_cu[b];
    RP_REQUIRE(S >= 1 && S <= DEC_MAX_KEYS, "src_len of state %d = %lld (1..%d)", b, (long long)S, DEC_MAX_KEYS);
  }
  total_src = src_cu[n];
  return RP_OK;
}

}  // namespace

extern "C" size_t rp_decoder_batch_workspace_bytes(const RpDecoder* d, const int32_t* src_cu, int32_t n, int32_t nb,
                                                   int32_t max_len) {
  int total = 0;
  if (decb_check(d, src_cu, n, nb, max_len, total) != RP_OK) return 0;
  return decb_carve(d, n, total, nb, max_len, nullptr).bytes;
}

extern "C" RpStatus rp_decoder_batch_cross_kv(RpDecoder* d, const void* enc, const int32_t* src_cu, int32_t n, int32_t nb,
                                              int32_t max_len, void* ws, size_t ws_bytes, void* stream_) {
  int total = 0;
  RpStatus st = decb_check(d, src_cu, n, nb, max_len, total);
  if (st) return st;
  RP_REQUIRE(enc, "null encoder states");
  const DecbWs w = decb_carve(d, n, total, nb, max_len, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  const int D = d->cfg.d_model, NKV = d->cfg.num_layers * 2 * d->inner;
  return launch_decb_gemm<EPI_BF16>((const bf16_t*)enc, D, total, d->cross_kv_w, NKV, D, w.ckv, NKV, (hipStream_t)stream_);
}

extern "C" RpStatus rp_decoder_batch_step(RpDecoder* d, const int32_t* src_cu, int32_t n, const int32_t* active,
                                          int32_t n_active, const int32_t* tokens, const int32_t* anc, int32_t astride,
                                          int32_t nb, int32_t t, int32_t max_len, float* logprobs, void* ws,
                                          size_t ws_bytes, void* stream_) {
  int total = 0;
  RpStatus st = decb_check(d, src_cu, n, nb, max_len, total);
  if (st) return st;
  RP_REQUIRE(active && tokens && anc && logprobs, "null argument");
  RP_REQUIRE(n_active >= 1 && n_active <= n, "active states=%d (1..states=%d)", n_active, n);
  RP_REQUIRE(t >= 0 && t < max_len, "t=%d outside [0, max_len=%d)", t, max_len);
  RP_REQUIRE(astride >= t + 1, "anc_stride=%d < t + 1 = %d", astride, t + 1);
  DecbSlots slots = {};
  uint32_t seen = 0;
  int max_src = 0;
  for (int a = 0; a < n_active; ++a) {
    const int sidx = active[a];
    RP_REQUIRE(sidx >= 0 && sidx < n, "active[%d]=%d outside [0, states=%d)", a, sidx, n);
    RP_REQUIRE(!(seen & (1u << sidx)), "active[%d]=%d names a state twice", a, sidx);  // two slots would share cache rows
    seen |= 1u << sidx;
    slots.state[a] = sidx;
    slots.src_off[a] = src_cu[sidx];
    slots.src_len[a] = src_cu[sidx + 1] - src_cu[sidx];
    max_src = std::max(max_src, slots.src_len[a]);
  }
  const DecbWs w = decb_carve(d, n, total, nb, max_len, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream_;
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  const int M = n_active * nb, rows = max_len * nb, ldckv = L * 2 * inner;
  const size_t layer_stride = (size_t)rows * 2 * inner, state_stride = (size_t)L * layer_stride;
  bf16_t* ffn = w.h + (size_t)M * D;
  hipLaunchKernelGGL(dec_embed_kernel, dim3(M), dim3(256), 0, s, tokens, d->embed, w.x, D, V);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    bf16_t* cache = w.cache + (size_t)i * layer_stride;  // state 0's rows of layer i
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_self, w.h, D, eps, 1.f);
    if ((st = launch_decb_gemm<EPI_BF16>(w.h, D, M, l.wqkv, 3 * inner, D, w.qkv, 3 * inner, s))) return st;
    hipLaunchKernelGGL(decb_store_kv_kernel, dim3(M), dim3(256), 0, s, w.qkv, inner, cache, state_stride, t * nb, nb, slots);
    hipLaunchKernelGGL((decb_attention_kernel<false>), dim3(H, M), dim3(256), (t + 1) * sizeof(float), s, w.qkv, 3 * inner,
                       cache, 2 * inner, 0, inner, rows, state_stride, anc, astride, d->bias_tab, d->nbias, t + 1, nb, slots,
                       w.att, inner);
    if ((st = launch_decb_gemm<EPI_RESID>(w.att, inner, M, l.wo, D, inner, w.x, D, s))) return st;
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_cross, w.h, D, eps, 1.f);
    if ((st = launch_decb_gemm<EPI_BF16>(w.h, D, M, l.cq, inner, D, w.qkv, inner, s))) return st;
    hipLaunchKernelGGL((decb_attention_kernel<true>), dim3(H, M), dim3(256), max_src * sizeof(float), s, w.qkv, inner, w.ckv,
                       ldckv, 2 * i * inner, (2 * i + 1) * inner, 0, (size_t)0, (const int32_t*)nullptr, 0,
                       (const float*)nullptr, 1, 0, nb, slots, w.att, inner);
    if ((st = launch_decb_gemm<EPI_RESID>(w.att, inner, M, l.co, D, inner, w.x, D, s))) return st;
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_ff, w.h, D, eps, 1.f);
    if ((st = launch_decb_gemm<EPI_GEGLU>(w.h, D, M, l.wi, F, D, ffn, F, s))) return st;
    if ((st = launch_decb_gemm<EPI_RESID>(ffn, F, M, l.wo2, D, F, w.x, D, s))) return st;
  }
  const float scale = d->tied ? 1.f / sqrtf((float)D) : 1.f;
  hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, d->final_ln, w.h, D, eps, scale);
  if ((st = launch_decb_gemm<EPI_F32>(w.h, D, M, d->lm_head, V, D, logprobs, V, s))) return st;
  hipLaunchKernelGGL(dec_log_softmax_kernel, dim3(M), dim3(256), 0, s, logprobs, V);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_beam_select_batch(const float* lp, const float* running, int32_t n_active, int32_t nb, int32_t V,
                                         int32_t k, float* scores, int32_t* tokens, int32_t* parents, void* ws,
                                         size_t ws_bytes, void* stream_) {
  RP_REQUIRE(lp && running && scores && tokens && parents, "null argument");
  RP_REQUIRE(n_active >= 1 && n_active <= DECB_MAX_STATES, "states=%d (1..%d)", n_active, DECB_MAX_STATES);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(V >= 1 && V <= DEC_SELECT_ROW, "vocab=%d (1..%d)", V, DEC_SELECT_ROW);
  RP_REQUIRE(k >= 1 && k <= DEC_SELECT_MAX_K && k <= nb * V, "k=%d (1..min(%d, nb * vocab))", k, DEC_SELECT_MAX_K);
  const int kr = std::min(k, V);
  const size_t need = (size_t)n_active * nb * kr * sizeof(uint64_t);
  if (!ws || ws_bytes < need) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream_;
  uint64_t* cand = (uint64_t*)ws;
  hipLaunchKernelGGL(decb_row_topk_kernel, dim3(n_active * nb), dim3(256), 0, s, lp, running, V, kr, nb, cand);
  hipLaunchKernelGGL(decb_merge_kernel, dim3(n_active), dim3(1024), 0, s, cand, nb * kr, V, k, scores, tokens, parents);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
