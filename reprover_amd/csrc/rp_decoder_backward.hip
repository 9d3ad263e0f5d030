// libreprover_hip - gradients of the teacher-forced seq2seq loss with respect to the decoder's parameters and to the
// encoder output (include/reprover_hip.h): rp_decoder_loss_grad.
//
// Forward part: rp_decoder_forward's launch sequence itself (fwd_launch_layers, rp_decoder_forward_kernels.h), given a
// buffer view in which every layer's activations have slots of their own; the sequence then copies the residual stream
// forward before each residual GEMM adds into it.  label_logprobs / loss_sum_count are rp_decoder_forward's bits.
// Saved per layer: the residual stream at the three sub-layer inputs (fp32), the three normed rows, qkv, the cross q,
// the cross K | V, both attention outputs with their lse2, and the FFN inner rows.  Recomputed in the backward: the
// RMSNorm statistic rsqrt(mean x^2 + eps) (from the saved stream, in the row kernel that needs it) and the gate / up
// pre-activations (one GEMM on the interleaved FFN-in weight into an fp32 buffer reused by every layer: the forward's own
// accumulators, never rounded).
//
// Backward, per GEMM  y = x W^T:  dW = dY^T X  (wgrad_kernel, rp_train_kernels.h: token-major operands, split-free, so
// one fixed K order)  and  dX = dY W  (the forward's MFMA core on a transposed bf16 copy of W made per call by
// transpose_bf16_kernel into one scratch matrix of the largest weight's size: no second resident copy of the decoder, and
// never a stale one).  dY is rounded to bf16 before either MFMA; accumulation and the residual-stream gradient are fp32.
// Attention: dec_flash_bwd_kernel below.  No floating-point atomic touches HBM; every reduction runs in an order fixed
// by the shapes, so two runs give the same bits, and d_enc rows of a pair do not depend on the other pairs except through
// the 1 / count factor of the loss.
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "rp_decoder_forward_kernels.h"
#include "rp_train_kernels.h"

extern "C" int32_t rp_relative_position_bucket_causal(int32_t rel, int32_t num_buckets, int32_t max_distance);

namespace {

// ---- flat gradient layout ------------------------------------------------------------------------------------------------
enum { G_LN_SELF, G_Q, G_K, G_V, G_O, G_LN_CROSS, G_CQ, G_CK, G_CV, G_CO, G_LN_FF, G_WI0, G_WI1, G_WO, G_PER_LAYER };
struct GradLayout {
  std::vector<int64_t> off;    // tensors + 1: every tensor starts at a multiple of 64 elements
  std::vector<int64_t> elems;  // tensors: the real (unpadded) element counts
  int head = 0;
  int64_t shared() const { return off[0]; }
  int64_t lm_head() const { return off[1]; }  // untied only
  int64_t rel_bias() const { return off[1 + head]; }
  int64_t final_ln() const { return off[2 + head]; }
  int64_t layer(int i, int k) const { return off[3 + head + i * G_PER_LAYER + k]; }
};
GradLayout grad_layout(const RpDecoder* d) {
  const int64_t D = d->cfg.d_model, V = d->cfg.vocab_size, ID = (int64_t)d->inner * D, FD = (int64_t)d->cfg.d_ff * D;
  const int64_t per_layer[G_PER_LAYER] = {D, ID, ID, ID, ID, D, ID, ID, ID, ID, D, FD, FD, FD};  // G_* order
  GradLayout l;
  l.head = d->tied ? 0 : 1;
  l.off.push_back(0);
  auto add = [&](int64_t n) {
    l.elems.push_back(n);
    l.off.push_back(l.off.back() + (n + 63) / 64 * 64);
  };
  add(V * D);
  if (!d->tied) add(V * D);
  add((int64_t)d->cfg.rel_num_buckets * d->cfg.num_heads);
  add(D);
  for (int i = 0; i < d->cfg.num_layers; ++i)
    for (int64_t n : per_layer) add(n);
  return l;
}

// ---- row kernels ---------------------------------------------------------------------------------------------------------
// dlogits = (softmax - onehot) / count for counted rows, 0 for ignored rows and for the padding rows [n_tok, gridDim.x);
// the softmax is fwd_loss_row_kernel's (max, sum of __expf); count = loss_sum_count[1] on the device (0: every row 0).
__global__ __launch_bounds__(256) void bwd_dlogits_kernel(const float* __restrict__ logits, int V, int n_tok,
                                                          const int32_t* __restrict__ labels,
                                                          const double* __restrict__ sum_count, bf16_t* __restrict__ out) {
  __shared__ float red[4];
  const int t = blockIdx.x;
  const int c0 = threadIdx.x, c1 = threadIdx.x + 256;
  const int y = t < n_tok ? labels[t] : -1;
  const float cnt = (float)sum_count[1];
  if (y < 0 || y >= V || !(cnt > 0.f)) {  // block-uniform
    if (c0 < V) out[(size_t)t * V + c0] = f2bf(0.f);
    if (c1 < V) out[(size_t)t * V + c1] = f2bf(0.f);
    return;
  }
  const float* row = logits + (size_t)t * V;
  const float x0 = c0 < V ? row[c0] : -INFINITY, x1 = c1 < V ? row[c1] : -INFINITY;
  const float mx = block_max256(fmaxf(x0, x1), red);
  float s = (c0 < V ? __expf(x0 - mx) : 0.f) + (c1 < V ? __expf(x1 - mx) : 0.f);
  s = block_sum256(s, red);
  const float inv = 1.f / s, ic = 1.f / cnt;
  if (c0 < V) out[(size_t)t * V + c0] = f2bf((__expf(x0 - mx) * inv - (c0 == y ? 1.f : 0.f)) * ic);
  if (c1 < V) out[(size_t)t * V + c1] = f2bf((__expf(x1 - mx) * inv - (c1 == y ? 1.f : 0.f)) * ic);
}

// out = bf16(in) over rows < n_tok, 0 over the padding rows (the wgrad GEMM reads whole 64-row tiles)
__global__ __launch_bounds__(256) void bwd_cast_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int D,
                                                       int n_tok) {
  const int t = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) out[(size_t)t * D + c] = f2bf(t < n_tok ? in[(size_t)t * D + c] : 0.f);
}
// out = bf16(mask * in): what the branch behind a residual dropout reads as its dY (dgrad and wgrad); the stream's own
// gradient `in` passes the residual unmasked
__global__ __launch_bounds__(256) void bwd_cast_drop_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int D,
                                                            int n_tok, Drop drop, uint32_t site) {
  const int t = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256)
    out[(size_t)t * D + c] = f2bf(t < n_tok ? drop_mul(drop, site, (uint32_t)t, (uint32_t)c) * in[(size_t)t * D + c] : 0.f);
}

// T5 RMSNorm backward of h = scale * w * x * rs, rs = rsqrt(mean(x^2) + eps), one workgroup per token:
//   dx (+)= scale * (w * rs * dh - x * rs^3 * mean(dh * w * x));   dh <- scale * dh * x * rs   (the row's term of d w,
// summed over the tokens by colsum_kernel afterwards).  ADD = 0 writes dx (the final norm opens the backward).
// DROP (the final norm under dropout): the rows were h = mask * (...), so dh is read times the regenerated mask.
template <bool ADD, bool DROP = false>
__global__ __launch_bounds__(256) void bwd_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          float* __restrict__ dh, float* __restrict__ dx, int D, float eps,
                                                          float scale, Drop drop = Drop{0u, 0u, 1.f}) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * D;
  if constexpr (DROP)
    for (int c = threadIdx.x; c < D; c += 256) dh[base + c] *= drop_mul(drop, DROP_SITE_DEC_FINAL, blockIdx.x, (uint32_t)c);
  float ss = 0.f, dot = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) {
    const float xv = x[base + c];
    ss = fmaf(xv, xv, ss);
    dot = fmaf(dh[base + c] * w[c], xv, dot);
  }
  ss = block_sum256(ss, red);
  dot = block_sum256(dot, red);
  const float r = rsqrtf(ss / (float)D + eps);
  const float k = r * r * r * (dot / (float)D);
  for (int c = threadIdx.x; c < D; c += 256) {
    const float xv = x[base + c], g = dh[base + c];
    const float v = scale * (w[c] * r * g - xv * k);
    dx[base + c] = ADD ? dx[base + c] + v : v;
    dh[base + c] = scale * g * xv * r;
  }
}

// Backward of ff = gelu_new(g) * u:  dg = dff * u * gelu_new'(g), du = dff * gelu_new(g), written bf16 as [dg (F) | du (F)]
// per token (wi_0's rows then wi_1's: the order of the plain FFN-in weight).  gu is the recomputed fp32 pre-activation
// pair in the interleaved order of RpDecoder::wi_il (64-column blocks: 32 gate, the same 32 up).  Padding rows get 0.
// DROP: the forward stored ff = mask * gelu_new(g) * u (HF:110), so dff is read times the regenerated mask.
template <bool DROP>
__global__ __launch_bounds__(256) void bwd_geglu_kernel(const float* __restrict__ gu, const float* __restrict__ dff,
                                                        bf16_t* __restrict__ dgu, int F, int n_tok, Drop drop,
                                                        uint32_t drop_site) {
  const int t = blockIdx.x;
  for (int f = threadIdx.x; f < F; f += 256) {
    float dg = 0.f, du = 0.f;
    if (t < n_tok) {
      const size_t gi = (size_t)t * 2 * F + 64 * (f >> 5) + (f & 31);
      const float g = gu[gi], u = gu[gi + 32];
      float d = dff[(size_t)t * F + f];
      if constexpr (DROP) d *= drop_mul(drop, drop_site, (uint32_t)t, (uint32_t)f);
      const float c0 = 0.7978845608028654f, c1 = 0.044715f;
      const float th = tanhf(c0 * (g + c1 * g * g * g));
      const float dgelu = 0.5f * (1.f + th) + 0.5f * g * (1.f - th * th) * c0 * (1.f + 3.f * c1 * g * g);
      dg = d * u * dgelu;
      du = d * (0.5f * g * (1.f + th));
    }
    dgu[(size_t)t * 2 * F + f] = f2bf(dg);
    dgu[(size_t)t * 2 * F + F + f] = f2bf(du);
  }
}

// d embed[v] (+)= sum over the tokens t with clamp(tokens[t]) == v, in token order, of dx[t] (embed_bwd_kernel's pattern on
// the fp32 stream gradient: one owner per vocabulary row, no atomics).  ADD: the tied head's weight gradient is there.
// DROP: the forward's rows were mask * embed[id] (HF:725), so each dx row is read times the regenerated mask.
template <bool ADD, bool DROP = false>
__global__ __launch_bounds__(256) void bwd_embed_kernel(const int32_t* __restrict__ ids, int T, int vocab,
                                                        const float* __restrict__ dx, int D, float* __restrict__ dtable,
                                                        Drop drop = Drop{0u, 0u, 1.f}) {
  __shared__ unsigned long long masks[4];
  const int v = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  const int wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (int base = 0; base < T; base += 256) {
    const int t = base + threadIdx.x;
    const int id = (t < T) ? min(max(ids[t], 0), vocab - 1) : -1;
    const unsigned long long m = __ballot(id == v);
    if ((threadIdx.x & 63) == 0) masks[wave] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned long long mm = masks[w];
      while (mm) {
        const int bit = __builtin_ctzll(mm);
        mm &= mm - 1;
        if (col < D) {
          const int t = base + w * 64 + bit;
          if constexpr (DROP)
            acc += dx[(size_t)t * D + col] * drop_mul(drop, DROP_SITE_DEC_EMBED, (uint32_t)t, (uint32_t)col);
          else
            acc += dx[(size_t)t * D + col];
        }
      }
    }
    __syncthreads();
  }
  if (col < D) {
    float* p = dtable + (size_t)v * D + col;
    *p = ADD ? *p + acc : acc;
  }
}

// ---- attention backward --------------------------------------------------------------------------------------------------
// dec_flash_bwd_kernel: the backward of dec_flash_kernel, after the encoder's attn_bwd_kernel (rp_train_kernels.h: the same
// staging of the streamed tile for plain and transposing fragment reads, the same MFMA sequence) with the decoder's
// indexing: queries are rows q_cu[b] + i of q / o / d_o, keys rows k_cu[b] + j of kv, different lengths per pair.
//   P = 2^((s + bias) log2 e - lse2),  delta_i = sum_d dO_i O_i,  dP = dO V^T,  dS = P (dP - delta)
//   MODE 0 (dQ = dS K):  workgroup = 128 queries x head, keys / values streamed; writes delta and, CAUSAL, the workgroup's
//                        partial gradient of bias_tab[h, min(i - j, nbias - 1)] (accumulated over the layers in layer
//                        launch order into its own row of dtab_part; bias_grad_kernel reduces the rows in row order)
//   MODE 1 (dK = dS^T Q, dV = P^T dO):  workgroup = 128 keys x head, queries / dO streamed with their lse2 / delta
// Two passes, no atomics on HBM.  CAUSAL (self-attention, k_cu = q_cu): keys j <= i; MODE 0 stops at the key tile of the
// block's last query, MODE 1 starts at the query tile of the block's first key.  P and dS are rounded to bf16 for the
// second MFMAs.
// DROP (the forward masked P before P V, mask M of dec_flash_kernel's elements): dV = (P M)^T dO, dP = M (dO V^T),
// dS = P (dP - delta); delta = rowsum(dO O) is unchanged because O was built from P M.  MODE 0 walks keys (two column
// pairs per four rows), MODE 1 walks queries (the lane's key picks the 16-bit field): the hash counter is linear in both.
struct FlashBwdArgs {
  const bf16_t* q;
  int ldq;
  const bf16_t* kv;
  int ldkv, koff, voff;
  const int32_t *q_cu, *k_cu;
  const int2* work;  // {pair, first resident row}: 128-query blocks (MODE 0) or 128-key blocks (MODE 1)
  const float* bias_tab;
  int nbias;
  const bf16_t *o, *d_o;  // [*, ldo]
  int ldo;
  const float* lse2;  // [H, ld_stat]
  float* delta;       // [H, ld_stat]
  int ld_stat;
  bf16_t* dq;  // MODE 0 [*, lddq]
  int lddq;
  bf16_t* dkv;  // MODE 1 [*, lddkv]: dK at column dkoff, dV at dvoff
  int lddkv, dkoff, dvoff;
  float* dtab_part;  // MODE 0, CAUSAL: [entries, H, nbias]
  Drop drop = {0u, 0u, 1.f};  // thresh 0: no dropout
  uint32_t drop_site = 0;
};

template <int MODE, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256, 2) void dec_flash_bwd_kernel(FlashBwdArgs a) {
  constexpr bool TAB = MODE == 0 && CAUSAL;
  constexpr int WTAB = TAB ? 4 * FA_TAB_MAX * 4 : 0;
  __shared__ __attribute__((aligned(16))) char smem[2 * AB_STAGE + FA_TAB_MAX * 4 + WTAB];
  float* tab = reinterpret_cast<float*>(smem + 2 * AB_STAGE);
  float* wtab = reinterpret_cast<float*>(smem + 2 * AB_STAGE + FA_TAB_MAX * 4);  // TAB: one table per wave

  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, cl = lane & 31;
  const int nh = a.ldo >> 6;
  const int h = blockIdx.x % nh;
  const int entry = blockIdx.x / nh;
  const int2 wk = a.work[entry];
  const int b = wk.x, n0 = wk.y;
  const int qs = a.q_cu[b], qlen = a.q_cu[b + 1] - qs;
  const int ks = a.k_cu[b], klen = a.k_cu[b + 1] - ks;
  const int rlen = MODE == 0 ? qlen : klen;  // resident rows (on the lanes)
  const int slen = MODE == 0 ? klen : qlen;  // streamed rows
  if (rlen <= 0) return;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbias = a.nbias;
  if (CAUSAL)
    for (int i = tid; i < nbias; i += 256) tab[i] = a.bias_tab[(size_t)h * nbias + i];
  if (TAB)
    for (int i = tid; i < 4 * FA_TAB_MAX; i += 256) wtab[i] = 0.f;
  __syncthreads();  // the tables are filled by all waves and read / added to by each

  const int wn0 = n0 + wave * 32;
  const bool active = wn0 < rlen && slen > 0;  // wave-uniform
  const int ni = wn0 + cl;
  const bool n_real = ni < rlen;
  const int nc = min(ni, rlen - 1);
  bf16x8 r1f[4], r2f[4];
  float lse_n = 0.f, delta_n = 0.f;
  if (MODE == 0) {
    const size_t row = (size_t)(qs + nc);
    const bf16_t* qp = a.q + row * a.ldq + h * 64 + hi * 8;
    const bf16_t* dop = a.d_o + row * a.ldo + h * 64 + hi * 8;
    const bf16_t* op = a.o + row * a.ldo + h * 64 + hi * 8;
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      r1f[c] = *reinterpret_cast<const bf16x8*>(qp + c * 16);
      r2f[c] = *reinterpret_cast<const bf16x8*>(dop + c * 16);
      const bf16x8 of = *reinterpret_cast<const bf16x8*>(op + c * 16);
#pragma unroll
      for (int e = 0; e < 8; ++e) dl = __builtin_fmaf(bf2f((bf16_t)r2f[c][e]), bf2f((bf16_t)of[e]), dl);
    }
    delta_n = dl + __shfl_xor(dl, 32, 64);
    lse_n = a.lse2[(size_t)h * a.ld_stat + row];
    if (n_real && hi == 0) a.delta[(size_t)h * a.ld_stat + row] = delta_n;
  } else {
    const size_t row = (size_t)(ks + nc);
    const bf16_t* kp = a.kv + row * a.ldkv + a.koff + h * 64 + hi * 8;
    const bf16_t* vp = a.kv + row * a.ldkv + a.voff + h * 64 + hi * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      r1f[c] = *reinterpret_cast<const bf16x8*>(kp + c * 16);
      r2f[c] = *reinterpret_cast<const bf16x8*>(vp + c * 16);
    }
  }

  // streamed operands: MODE 0 keys (K, V); MODE 1 queries (Q, dO) with their statistics
  const bf16_t* x1 = (MODE == 0) ? a.kv + (size_t)ks * a.ldkv + a.koff + h * 64 : a.q + (size_t)qs * a.ldq + h * 64;
  const bf16_t* x2 = (MODE == 0) ? a.kv + (size_t)ks * a.ldkv + a.voff + h * 64 : a.d_o + (size_t)qs * a.ldo + h * 64;
  const int ld1 = (MODE == 0) ? a.ldkv : a.ldq, ld2 = (MODE == 0) ? a.ldkv : a.ldo;
  const float* st_lse = a.lse2 + (size_t)h * a.ld_stat + qs;
  const float* st_del = a.delta + (size_t)h * a.ld_stat + qs;
  const int smax = max(slen - 1, 0);
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * AB_STAGE;
    const int m0 = kt * 64;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = wave * 2 + e;  // piece: d half p / 4, rows 16 (p % 4) .. + 15
      const int row = 16 * (p & 3) + (lane >> 2);
      const int slot = (lane & 3) ^ ((row >> 2) & 3);
      const size_t r = (size_t)min(m0 + row, smax);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(x1 + r * ld1 + (p >> 2) * 32 + slot * 8), (lds_ptr_t)(base + p * 1024), 16,
                                       0, 0);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(x2 + r * ld2 + (p >> 2) * 32 + slot * 8),
                                       (lds_ptr_t)(base + AB_TILE + p * 1024), 16, 0, 0);
    }
    if (MODE == 1 && wave < 2) {
      const float* src = (wave == 0 ? st_lse : st_del) + min(m0 + lane, smax);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + 2 * AB_TILE + wave * 256), 4, 0, 0);
    }
  };

  int n_off[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int row = mb * 32 + cl;
      n_off[mb][c] = (c >> 1) * 4096 + row * 64 + (((2 * (c & 1) + hi) ^ ((row >> 2) & 3)) << 4);
    }
  const int g1 = (lane >> 4) & 1, q4 = (lane & 15) >> 2, l3 = lane & 3;
  const int cl16 = 2 * g1 + (l3 >> 1);
  const int t_lo = (4 * hi + q4) * 64 + ((cl16 ^ hi) << 4) + 8 * (l3 & 1);
  const int t_up = (4 * hi + q4 + 8) * 64 + ((cl16 ^ (hi ^ 2)) << 4) + 8 * (l3 & 1);

  f32x16 acc1[2], acc2[2];  // MODE 0: acc1 = dQ^T;  MODE 1: acc1 = dK^T, acc2 = dV^T   ([d half][d, n])
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[d][r] = acc2[d][r] = 0.f;

  const float LOG2E = 1.4426950408889634f;
  // streamed tiles [kt_lo, kt_hi): causal MODE 0 ends with the block's last query, causal MODE 1 begins with its first key
  const int kt_lo = (CAUSAL && MODE == 1) ? n0 / 64 : 0;
  const int kt_hi = slen > 0 ? ((CAUSAL && MODE == 0 ? min(slen, n0 + FA_Q) : slen) + 63) / 64 : 0;
  if (kt_lo < kt_hi) stage(kt_lo, 0);
  for (int kt = kt_lo; kt < kt_hi; ++kt) {
    const int it = kt - kt_lo;
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < kt_hi) stage(kt + 1, (it + 1) & 1);
    const int m0 = kt * 64;
    if (!active) continue;
    if (CAUSAL && MODE == 0 && m0 > wn0 + 31) continue;  // every key of the tile lies after every query of the wave
    if (CAUSAL && MODE == 1 && m0 + 63 < wn0) continue;  // every query of the tile lies before every key of the wave
    const char* sb = smem + (it & 1) * AB_STAGE;
    const float* sstat = reinterpret_cast<const float*>(sb + 2 * AB_TILE);
    f32x16 s[2], dp[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[mb][r] = dp[mb][r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 f1 = *reinterpret_cast<const bf16x8*>(sb + n_off[mb][c]);
        const bf16x8 f2 = *reinterpret_cast<const bf16x8*>(sb + AB_TILE + n_off[mb][c]);
        s[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, r1f[c], s[mb], 0, 0, 0);
        dp[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f2, r2f[c], dp[mb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int c0 = m0 + mb * 32;
      // table gradient: every accumulator row is rotated by its own row number, which brings the entries of a diagonal
      // (query - key constant) into one lane (attn_bwd_kernel's scheme); masked entries carry dS = 0
      float diag_a = 0.f, diag_b = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float lse_m[4], del_m[4];
        if (MODE == 1) {
          const float4 lv = *reinterpret_cast<const float4*>(sstat + mb * 32 + 8 * g + 4 * hi);
          const float4 dv = *reinterpret_cast<const float4*>(sstat + 64 + mb * 32 + 8 * g + 4 * hi);
          lse_m[0] = lv.x; lse_m[1] = lv.y; lse_m[2] = lv.z; lse_m[3] = lv.w;
          del_m[0] = dv.x; del_m[1] = dv.y; del_m[2] = dv.z; del_m[3] = dv.w;
        }
        float dmul[4];
        if constexpr (DROP) {
          const int jg = c0 + 8 * g + 4 * hi;  // even: the lane's four streamed indices are jg .. jg + 3
          const uint32_t hcol = (uint32_t)h << 20;
          if (MODE == 0) {  // streamed keys: two column pairs of the query's row
            drop_mul2(a.drop, a.drop_site, (uint32_t)(qs + ni), hcol | (uint32_t)jg, dmul[0], dmul[1]);
            drop_mul2(a.drop, a.drop_site, (uint32_t)(qs + ni), hcol | (uint32_t)(jg + 2), dmul[2], dmul[3]);
          } else {  // streamed queries: the lane's key picks the field, the row advances
#pragma unroll
            for (int e = 0; e < 4; ++e) dmul[e] = drop_mul(a.drop, a.drop_site, (uint32_t)(qs + jg + e), hcol | (uint32_t)ni);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const int j = c0 + 8 * g + 4 * hi + e;  // streamed index of this accumulator row
          const int dist = (MODE == 0) ? ni - j : j - ni;  // query - key
          const bool live = j < slen && n_real && (!CAUSAL || dist >= 0);
          const float bias = CAUSAL ? tab[min(max(dist, 0), nbias - 1)] : 0.f;
          const float lse = (MODE == 0) ? lse_n : lse_m[e];
          const float del = (MODE == 0) ? delta_n : del_m[e];
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[mb][r] + bias, LOG2E, -lse));
          if (!live) p = 0.f;
          float pm = p, dpv = dp[mb][r];
          if constexpr (DROP) {
            pm *= dmul[e];
            dpv *= dmul[e];
          }
          const float ds = live ? p * (dpv - del) : 0.f;
          s[mb][r] = pm;
          dp[mb][r] = ds;
          if (TAB) {
            const int kr = 8 * g + 4 * hi + e;
            const float w = __shfl(ds, (hi << 5) | ((cl + kr) & 31), 64);
            if (cl + kr < 32)
              diag_a += w;
            else
              diag_b += w;
          }
        }
      }
      if (TAB) {
        // the lane's diagonals: key - query = (c0 + kr) - (wn0 + column) = c0 - wn0 - cl and that + 32
        const int dist_a = wn0 + cl - c0, dist_b = dist_a - 32;
        atomicAdd(&wtab[wave * FA_TAB_MAX + min(max(dist_a, 0), nbias - 1)], diag_a);  // LDS, wave-private table
        atomicAdd(&wtab[wave * FA_TAB_MAX + min(max(dist_b, 0), nbias - 1)], diag_b);
      }
    }
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const int mb = sl >> 1, sub = sl & 1;
      bf16x8 pf, dsf;
      {
        uint32_t pw[4], dw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pw[e] = pack_bf2(s[mb][8 * sub + 2 * e], s[mb][8 * sub + 2 * e + 1]);
          dw[e] = pack_bf2(dp[mb][8 * sub + 2 * e], dp[mb][8 * sub + 2 * e + 1]);
        }
        uint4 t = make_uint4(pw[0], pw[1], pw[2], pw[3]);
        pf = *reinterpret_cast<bf16x8*>(&t);
        uint4 u = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        dsf = *reinterpret_cast<bf16x8*>(&u);
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const char* b1 = sb + d * 4096 + sl * 1024;
        const bf16x8 x1t = tr_read_pair(b1 + t_lo, b1 + t_up);
        acc1[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1t, dsf, acc1[d], 0, 0, 0);
        if (MODE == 1) {
          const bf16x8 x2t = tr_read_pair(b1 + AB_TILE + t_lo, b1 + AB_TILE + t_up);
          acc2[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2t, pf, acc2[d], 0, 0, 0);
        }
      }
    }
  }

  if (n_real) {  // (a wave with nothing to stream - an empty target over this source - writes zeros)
    auto store = [&](const f32x16 (&o)[2], bf16_t* op) {
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          uint2 v;
          v.x = pack_bf2(o[d][4 * g], o[d][4 * g + 1]);
          v.y = pack_bf2(o[d][4 * g + 2], o[d][4 * g + 3]);
          *reinterpret_cast<uint2*>(op + d * 32 + 8 * g + 4 * hi) = v;
        }
    };
    if (MODE == 0) {
      store(acc1, a.dq + (size_t)(qs + ni) * a.lddq + h * 64);
    } else {
      store(acc1, a.dkv + (size_t)(ks + ni) * a.lddkv + a.dkoff + h * 64);
      store(acc2, a.dkv + (size_t)(ks + ni) * a.lddkv + a.dvoff + h * 64);
    }
  }
  if (TAB) {
    __syncthreads();
    float* dst = a.dtab_part + ((size_t)entry * nh + h) * nbias;
    for (int i = tid; i < nbias; i += 256)
      dst[i] += (wtab[i] + wtab[FA_TAB_MAX + i]) + (wtab[2 * FA_TAB_MAX + i] + wtab[3 * FA_TAB_MAX + i]);
  }
}

// ---- workspace -----------------------------------------------------------------------------------------------------------
// bytes = meta + sum over the buffers below (each rounded up to 256), with Tp / Sp = the target / source token counts
// rounded up to 128, D = d_model, F = d_ff, I = H * 64, V = vocab, L = layers, W = the largest weight's element count:
//   saved    (3 L + 1) Tp D 4 (stream) + (3 L + 1) Tp D 2 (normed) + L [Tp 3I 2 + Tp I 2 + Sp 2I 2 + 2 Tp I 2 + 2 H Tp 4
//            + Tp F 2] + Tp V 4 (logits)
//   scratch  Tp D 4 (dx) + Tp D 4 (dh) + Tp D 2 + Tp V 2 + Tp F 4 + Tp 2F 4 (gate | up) + Tp 2F 2 + Tp I 2 + Tp 3I 2 + Tp I 2 (cross dq)
//            + Sp 2I 2 + H Tp 4 (delta) + entries H nbias 4 (table partials) + W 2 (transposed weight) + Sp D 2 (enc copy)
struct BwdWs {
  int32_t* meta;  // src_cu, tgt_cu, query work list, source-key work list (int2 each), bucket_of [nbias]
  float* xs;      // [3 L + 1][Tp, D]
  bf16_t* hs;     // [3 L + 1][Tp, D]
  bf16_t *qkv, *cq, *ckv, *att_s, *att_c, *ff;  // [L][...]
  float *lse_s, *lse_c;                         // [L][H, Tp]
  float* logits;
  float *dx, *dh, *dff, *gu, *delta, *dtab_part;
  bf16_t *dyb, *dlog, *dgu, *datt, *dqkv, *dcq, *dkv, *wt, *encp;
  size_t sz_x, sz_qkv, sz_cq, sz_ckv, sz_ff, sz_lse, dtab_bytes;
  int L, Tp;
  size_t bytes;
  // layer i's slots: the stream and the normed rows move on by one slot per sub-layer, so x3 is layer i + 1's x0
  FwdLayerBufs layer(int i) const {
    float* x = xs + 3 * (size_t)i * sz_x;
    bf16_t* h = hs + 3 * (size_t)i * sz_x;
    const size_t n = i;
    return {x, x + sz_x, x + 2 * sz_x, x + 3 * sz_x, h, h + sz_x, h + 2 * sz_x, qkv + n * sz_qkv, cq + n * sz_cq,
            ckv + n * sz_ckv, att_s + n * sz_cq, att_c + n * sz_cq, ff + n * sz_ff, lse_s + n * sz_lse, lse_c + n * sz_lse, Tp};
  }
  FwdFinalBufs last() const { return {xs + 3 * (size_t)L * sz_x, hs + 3 * (size_t)L * sz_x, logits}; }
};
int bwd_src_work(int batch, int n_src) { return n_src / FA_Q + batch; }
size_t bwd_max_weight(const RpDecoder* d) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, V = d->cfg.vocab_size;
  return std::max(std::max(3 * inner * D, 2 * F * D), V * D);
}
BwdWs bwd_carve(const RpDecoder* d, int batch, int n_src, int n_tgt, char* base) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, V = d->cfg.vocab_size, H = d->cfg.num_heads;
  const size_t L = d->cfg.num_layers;
  const size_t Tp = align_up((size_t)std::max(n_tgt, 1), FWD_BN), Sp = align_up((size_t)std::max(n_src, 1), FWD_BN);
  BwdWs w;
  Carver c{base};
  w.L = (int)L;
  w.Tp = (int)Tp;
  w.meta = (int32_t*)c.take((size_t)(2 * (batch + 1) + 2 * fwd_max_work(batch, n_tgt) + 2 * bwd_src_work(batch, n_src) +
                                     d->nbias) * 4);
  w.sz_x = Tp * D;
  w.sz_qkv = Tp * 3 * inner;
  w.sz_cq = Tp * inner;
  w.sz_ckv = Sp * 2 * inner;
  w.sz_ff = Tp * F;
  w.sz_lse = H * Tp;
  w.xs = (float*)c.take((3 * L + 1) * w.sz_x * 4);
  w.hs = (bf16_t*)c.take((3 * L + 1) * w.sz_x * 2);
  w.qkv = (bf16_t*)c.take(L * w.sz_qkv * 2);
  w.cq = (bf16_t*)c.take(L * w.sz_cq * 2);
  w.ckv = (bf16_t*)c.take(L * w.sz_ckv * 2);
  w.att_s = (bf16_t*)c.take(L * w.sz_cq * 2);
  w.att_c = (bf16_t*)c.take(L * w.sz_cq * 2);
  w.ff = (bf16_t*)c.take(L * w.sz_ff * 2);
  w.lse_s = (float*)c.take(L * w.sz_lse * 4);
  w.lse_c = (float*)c.take(L * w.sz_lse * 4);
  w.logits = (float*)c.take(Tp * V * 4);
  w.dx = (float*)c.take(Tp * D * 4);
  w.dh = (float*)c.take(Tp * D * 4);
  w.dyb = (bf16_t*)c.take(Tp * D * 2);
  w.dlog = (bf16_t*)c.take(Tp * V * 2);
  w.dff = (float*)c.take(Tp * F * 4);
  w.gu = (float*)c.take(Tp * 2 * F * 4);
  w.dgu = (bf16_t*)c.take(Tp * 2 * F * 2);
  w.datt = (bf16_t*)c.take(Tp * inner * 2);
  w.dqkv = (bf16_t*)c.take(Tp * 3 * inner * 2);
  w.dcq = (bf16_t*)c.take(Tp * inner * 2);
  w.dkv = (bf16_t*)c.take(Sp * 2 * inner * 2);
  w.delta = (float*)c.take(H * Tp * 4);
  w.dtab_bytes = (size_t)fwd_max_work(batch, n_tgt) * H * d->nbias * 4;
  w.dtab_part = (float*)c.take(w.dtab_bytes);
  w.wt = (bf16_t*)c.take(bwd_max_weight(d) * 2);
  w.encp = (bf16_t*)c.take(Sp * D * 2);
  w.bytes = c.off;
  return w;
}

RpStatus bwd_check_model(const RpDecoder* d) {
  RpStatus st = fwd_check_model(d);
  if (st) return st;
  if (d->cfg.vocab_size % 64)
    return fail(RP_E_UNSUPPORTED, "vocab_size=%d: the lm_head's backward GEMMs need a multiple of 64", d->cfg.vocab_size);
  return RP_OK;
}

// f(std::true_type) or f(std::false_type): the one place a run-time flag picks a template's ADD argument
template <class F>
auto with_bool(bool b, F f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// ---- launches on raw pointers (rp_decoder_loss_grad and the rp_dbg_decoder_* test entries run these) --------------------------
// the 128-key blocks {pair, first key} of the sources of non-empty targets, appended to meta; returns their number
int bwd_build_kwork(const int32_t* src_cu, const int32_t* tgt_cu, int batch, std::vector<int32_t>& meta) {
  const size_t at = meta.size();
  for (int b = 0; b < batch; ++b) {
    if (tgt_cu[b + 1] == tgt_cu[b]) continue;
    for (int k0 = 0; k0 < src_cu[b + 1] - src_cu[b]; k0 += FA_Q) {
      meta.push_back(b);
      meta.push_back(k0);
    }
  }
  return (int)(meta.size() - at) / 2;
}
void launch_dlogits(const float* logits, int V, int n_tok, int rows_pad, const int32_t* labels, const double* sum_count,
                    bf16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(bwd_dlogits_kernel, dim3(rows_pad), dim3(256), 0, s, logits, V, n_tok, labels, sum_count, out);
}
const Drop NO_DROP = {0u, 0u, 1.f};
// (site: the residual-branch site whose mask the cast applies; ignored without dropout)
void launch_cast(const float* in, bf16_t* out, int D, int n_tok, int rows_pad, hipStream_t s, const Drop& drop = NO_DROP,
                 uint32_t site = 0u) {
  if (drop.thresh)
    hipLaunchKernelGGL(bwd_cast_drop_kernel, dim3(rows_pad), dim3(256), 0, s, in, out, D, n_tok, drop, site);
  else
    hipLaunchKernelGGL(bwd_cast_kernel, dim3(rows_pad), dim3(256), 0, s, in, out, D, n_tok);
}
void launch_geglu_bwd(const float* gu, const float* dff, bf16_t* dgu, int F, int n_tok, int rows_pad, hipStream_t s,
                      const Drop& drop = NO_DROP, uint32_t site = 0u) {
  with_bool(drop.thresh != 0, [&](auto dr) {
    hipLaunchKernelGGL(bwd_geglu_kernel<decltype(dr)::value>, dim3(rows_pad), dim3(256), 0, s, gu, dff, dgu, F, n_tok, drop,
                       site);
  });
}
// dh -> dx through the norm whose input rows were x; the rows' terms of d ln are summed into dln.  drop (the final norm
// alone, which writes dx): its rows were masked at DROP_SITE_DEC_FINAL.
void launch_norm_bwd(const float* x, const float* ln, float* dh, float* dx, int n_tok, int D, float eps, float sc, bool add,
                     float* dln, hipStream_t s, const Drop& drop = NO_DROP) {
  if (drop.thresh && !add)
    hipLaunchKernelGGL((bwd_rmsnorm_kernel<false, true>), dim3(n_tok), dim3(256), 0, s, x, ln, dh, dx, D, eps, sc, drop);
  else
    with_bool(add, [&](auto a) {
      hipLaunchKernelGGL((bwd_rmsnorm_kernel<decltype(a)::value, false>), dim3(n_tok), dim3(256), 0, s, x, ln, dh, dx, D, eps,
                         sc, NO_DROP);
    });
  hipLaunchKernelGGL(colsum_kernel, dim3((D + 63) / 64), dim3(64 * COLSUM_WAVES), 0, s, (const float*)dh, n_tok, D, dln);
}
void launch_embed_bwd(bool add_, const int32_t* ids, int T, int V, const float* dx, int D, float* dtable, hipStream_t s,
                      const Drop& drop = NO_DROP) {
  with_bool(add_, [&](auto add) {
    with_bool(drop.thresh != 0, [&](auto dr) {
      hipLaunchKernelGGL((bwd_embed_kernel<decltype(add)::value, decltype(dr)::value>), dim3(V, (D + 255) / 256), dim3(256), 0,
                         s, ids, T, V, dx, D, dtable, drop);
    });
  });
}
// both passes of the attention backward: dQ (+ delta, + the table partials when causal) over the query blocks, then
// dK | dV over the key blocks (causal: the query blocks again)
void launch_flash_bwd(bool causal, FlashBwdArgs fa, int H, const int2* qwork, int n_qwork, const int2* kwork, int n_kwork,
                      hipStream_t s) {
  auto launch = [&](auto mode, int n) {
    constexpr int M = decltype(mode)::value;
    with_bool(causal, [&](auto c) {
      with_bool(fa.drop.thresh != 0, [&](auto dr) {
        hipLaunchKernelGGL((dec_flash_bwd_kernel<M, decltype(c)::value, decltype(dr)::value>), dim3(H * n), dim3(256), 0, s, fa);
      });
    });
  };
  fa.work = qwork;
  launch(std::integral_constant<int, 0>{}, n_qwork);
  fa.work = kwork;
  if (!n_kwork) return;
  launch(std::integral_constant<int, 1>{}, n_kwork);
}
void launch_bias_grad(const float* dtab_part, int n_work, int H, int nbias, const int32_t* bucket_of, int nbuckets,
                      float* d_rel_bias, hipStream_t s) {
  hipLaunchKernelGGL(bias_grad_kernel, dim3(H), dim3(256), 0, s, dtab_part, n_work, H, nbias, bucket_of, nbuckets, d_rel_bias);
}

// Backward of a projection  y = x W^T,  W [R, C] bf16, over n token rows (n_pad: rounded up to 128, the padding rows of dY
// and X zero).  First one weight-gradient launch per slice of W's rows, in the order given: dW[row0 : row0 + rows] =
// dY[:, row0 : row0 + rows]^T X  (wgrad_kernel, one split: K runs in ascending token order).  Then dX = dY W on the
// forward's GEMM core: W is transposed into the scratch matrix wt immediately before the GEMM that reads it (every call
// shares wt).
struct WgradSlice {
  int row0, rows;
  float* dW;
};
enum DxKind { DX_NONE, DX_F32, DX_F32_ADD, DX_BF16 };
RpStatus linear_bwd(const bf16_t* dY, const bf16_t* X, int n, int n_pad, const bf16_t* W, int R, int C,
                    std::initializer_list<WgradSlice> slices, DxKind kind, void* dX, bf16_t* wt, hipStream_t s) {
  RpStatus st;
  for (const WgradSlice& sl : slices)
    if ((st = launch_wgrad_cfg<WgradCfg<128, 128, 2, 2, 2>>(WgradOperands{dY + sl.row0, R, sl.rows, X, C, C, sl.dW}, nullptr,
                                                           n_pad / 64, 1, s)))
      return st;
  if (kind == DX_NONE) return RP_OK;
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, s, W, R, C, wt);
  if (kind == DX_BF16) return fwd_gemm(dY, n, n_pad, wt, C, R, EpiDecBf16{(bf16_t*)dX, C, C, n}, s, RP_K_GEMM_O);
  return with_bool(kind == DX_F32_ADD, [&](auto add) {
    return fwd_gemm(dY, n, n_pad, wt, C, R, EpiDecF32<decltype(add)::value>{(float*)dX, C, C, n}, s, RP_K_GEMM_O);
  });
}

}  // namespace

extern "C" int32_t rp_decoder_grad_tensors(const RpDecoder* d) {
  if (!d) return 0;
  return (int32_t)grad_layout(d).off.size() - 1;
}

extern "C" RpStatus rp_decoder_grad_layout(const RpDecoder* d, int64_t* offsets) {
  RP_REQUIRE(d && offsets, "null argument");
  const GradLayout l = grad_layout(d);
  std::copy(l.off.begin(), l.off.end(), offsets);
  return RP_OK;
}

extern "C" size_t rp_decoder_loss_grad_workspace_bytes(const RpDecoder* d, const int32_t* src_cu, const int32_t* tgt_cu,
                                                       int32_t batch) {
  int n_src = 0, n_tgt = 0;
  if (bwd_check_model(d) != RP_OK || fwd_check_cu(src_cu, tgt_cu, batch, n_src, n_tgt) != RP_OK) return 0;
  return bwd_carve(d, batch, n_src, n_tgt, nullptr).bytes;
}

// The dropout form needs no buffer of its own: the branch behind a residual mask reads bf16(mask * dx), and the fp32 stream
// gradient is cast into the bf16 operand buffer (dyb) in front of every branch anyway - the mask rides on that cast.
extern "C" size_t rp_decoder_loss_grad_dropout_workspace_bytes(const RpDecoder* d, const int32_t* src_cu, const int32_t* tgt_cu,
                                                               int32_t batch) {
  return rp_decoder_loss_grad_workspace_bytes(d, src_cu, tgt_cu, batch);
}

// rp_decoder_loss_grad (drop.thresh == 0) and rp_decoder_loss_grad_dropout: one body, the launches differ only where a mask
// is applied
static RpStatus loss_grad(RpDecoder* d, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                          const int32_t* labels, const int32_t* tgt_cu, int32_t batch, const Drop& drop, float* label_logprobs,
                          double* loss_sum_count, float* grads, float* d_enc, void* ws, size_t ws_bytes, void* stream_) {
  RpStatus st = bwd_check_model(d);
  if (st) return st;
  int n_src = 0, n_tgt = 0;
  if ((st = fwd_check_cu(src_cu, tgt_cu, batch, n_src, n_tgt))) return st;
  RP_REQUIRE(loss_sum_count, "null loss_sum_count");
  RP_REQUIRE(grads, "null grads");
  RP_REQUIRE(n_tgt == 0 || (enc_bf16 && tokens && labels && label_logprobs), "null argument");
  const BwdWs w = bwd_carve(d, batch, n_src, n_tgt, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream_;
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  const GradLayout lay = grad_layout(d);
  if (d_enc && n_src) RP_HIP(hipMemsetAsync(d_enc, 0, (size_t)n_src * D * 4, s));
  if (n_tgt == 0) {  // no label at all: the loss is 0 / 0, every gradient 0
    const double zero[2] = {0.0, 0.0};
    RP_HIP(hipMemcpyWithStream(loss_sum_count, zero, sizeof zero, hipMemcpyHostToDevice, s));
    for (size_t k = 0; k < lay.elems.size(); ++k) RP_HIP(hipMemsetAsync(grads + lay.off[k], 0, (size_t)lay.elems[k] * 4, s));
    return RP_OK;
  }

  // metadata: the forward's, then the 128-key blocks of the sources of non-empty targets (the cross dK | dV pass) and the
  // bucket of every bias distance
  std::vector<int32_t> meta;
  const int n_work = fwd_build_meta(src_cu, tgt_cu, batch, meta);
  const size_t kwork_at = meta.size();
  const int n_kwork = bwd_build_kwork(src_cu, tgt_cu, batch, meta);
  const size_t bucket_at = meta.size();
  for (int j = 0; j < d->nbias; ++j) meta.push_back(rp_relative_position_bucket_causal(-j, c.rel_num_buckets, c.rel_max_distance));
  RP_HIP(hipMemcpyWithStream(w.meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s));
  const int32_t* d_src_cu = w.meta;
  const int32_t* d_tgt_cu = w.meta + batch + 1;
  const int2* d_work = reinterpret_cast<const int2*>(w.meta + 2 * (batch + 1));
  const int2* d_kwork = reinterpret_cast<const int2*>(w.meta + kwork_at);
  const int32_t* d_bucket = w.meta + bucket_at;

  const int Tp = w.Tp, Sp = (int)align_up(n_src, FWD_BN);
  std::vector<FwdLayerBufs> bufs(L);
  for (int i = 0; i < L; ++i) bufs[i] = w.layer(i);
  const FwdFinalBufs fin = w.last();
  // the wgrad GEMM reads whole 64-row tiles of both operands: their padding rows are zeroed once (no kernel writes them;
  // the cast / dlogits / geglu row kernels write their own); the source rows of pairs with an empty target keep dK | dV = 0
  auto zero_tail = [&](void* p, size_t rows, size_t rows_pad, size_t row_bytes) {
    return rows_pad > rows ? hipMemsetAsync((char*)p + rows * row_bytes, 0, (rows_pad - rows) * row_bytes, s) : hipSuccess;
  };
  for (int i = 0; i <= 3 * L; ++i) RP_HIP(zero_tail(w.hs + (size_t)i * w.sz_x, n_tgt, Tp, (size_t)D * 2));
  for (const FwdLayerBufs& b : bufs) {
    RP_HIP(zero_tail(b.att_s, n_tgt, Tp, (size_t)inner * 2));
    RP_HIP(zero_tail(b.att_c, n_tgt, Tp, (size_t)inner * 2));
    RP_HIP(zero_tail(b.ff, n_tgt, Tp, (size_t)F * 2));
  }
  RP_HIP(zero_tail(w.dqkv, n_tgt, Tp, (size_t)3 * inner * 2));
  RP_HIP(zero_tail(w.dcq, n_tgt, Tp, (size_t)inner * 2));
  RP_HIP(hipMemsetAsync(w.dkv, 0, (size_t)Sp * 2 * inner * 2, s));
  RP_HIP(hipMemsetAsync(w.dtab_part, 0, w.dtab_bytes, s));
  RP_HIP(hipMemcpyAsync(w.encp, enc_bf16, (size_t)n_src * D * 2, hipMemcpyDeviceToDevice, s));
  RP_HIP(zero_tail(w.encp, n_src, Sp, (size_t)D * 2));

  // ---- forward: the shared sequence on the per-layer slots ----------------------------------------------------------------
  if ((st = fwd_launch_layers(d, enc_bf16, tokens, labels, batch, n_src, n_tgt, w.meta, n_work, bufs.data(), fin,
                              label_logprobs, loss_sum_count, nullptr, s, drop)))
    return st;

  // ---- backward --------------------------------------------------------------------------------------------------------------
  auto G = [&](int64_t off) { return grads + off; };
  auto lin = [&](const bf16_t* dY, const bf16_t* X, const bf16_t* W, int R, int C, std::initializer_list<WgradSlice> slices,
                 DxKind kind, void* dX) { return linear_bwd(dY, X, n_tgt, Tp, W, R, C, slices, kind, dX, w.wt, s); };
  // w.dh -> w.dx through the norm whose input rows were x
  auto norm_bwd = [&](const float* x, const float* ln, float sc, bool add, float* dln) {
    launch_norm_bwd(x, ln, w.dh, w.dx, n_tgt, D, eps, sc, add, dln, s, add ? NO_DROP : drop);
  };
  // dyb = bf16([mask *] dx): the dY of the residual branch that was dropped at `site`
  auto cast_dx = [&](uint32_t site) { launch_cast(w.dx, w.dyb, D, n_tgt, Tp, s, drop, site); };

  // loss and head
  launch_dlogits(w.logits, V, n_tgt, Tp, labels, loss_sum_count, w.dlog, s);
  if ((st = lin(w.dlog, fin.h, d->lm_head, V, D, {{0, V, G(d->tied ? lay.shared() : lay.lm_head())}}, DX_F32, w.dh)))
    return st;
  norm_bwd(fin.x, d->final_ln, fwd_head_scale(d), false, G(lay.final_ln()));

  FlashBwdArgs fa{};
  fa.q_cu = d_tgt_cu;
  fa.bias_tab = d->bias_tab;
  fa.nbias = d->nbias;
  fa.ldo = inner;
  fa.delta = w.delta;
  fa.ld_stat = Tp;
  fa.dtab_part = w.dtab_part;
  fa.drop = drop;
  for (int i = L - 1; i >= 0; --i) {
    const RpDecoder::Layer& l = d->layers[i];
    const FwdLayerBufs& b = bufs[i];
    const uint32_t site = DROP_SITE_DEC_LAYER0 + 8u * (uint32_t)i;  // + {0 .. 5}, as in fwd_launch_layers
    auto Gl = [&](int k) { return G(lay.layer(i, k)); };
    // gated-GELU FFN
    cast_dx(site + 5);
    if ((st = lin(w.dyb, b.ff, l.wo2, D, F, {{0, D, Gl(G_WO)}}, DX_F32, w.dff))) return st;
    if ((st = fwd_gemm(b.h2, n_tgt, Tp, d->wi_il + (size_t)i * 2 * F * D, 2 * F, D, EpiDecF32<false>{w.gu, 2 * F, 2 * F, n_tgt},
                       s, RP_K_GEMM_WI)))
      return st;
    launch_geglu_bwd(w.gu, w.dff, w.dgu, F, n_tgt, Tp, s, drop, site + 4);
    if ((st = lin(w.dgu, b.h2, l.wi, 2 * F, D, {{0, F, Gl(G_WI0)}, {F, F, Gl(G_WI1)}}, DX_F32, w.dh))) return st;
    norm_bwd(b.x2, l.ln_ff, 1.f, true, Gl(G_LN_FF));

    // cross-attention
    cast_dx(site + 3);
    if ((st = lin(w.dyb, b.att_c, l.co, D, inner, {{0, D, Gl(G_CO)}}, DX_BF16, w.datt))) return st;
    fa.q = b.cq; fa.ldq = inner;
    fa.kv = b.ckv; fa.ldkv = 2 * inner; fa.koff = 0; fa.voff = inner;
    fa.k_cu = d_src_cu;
    fa.o = b.att_c; fa.d_o = w.datt;
    fa.lse2 = b.lse_c;
    fa.dq = w.dcq; fa.lddq = inner;
    fa.dkv = w.dkv; fa.lddkv = 2 * inner; fa.dkoff = 0; fa.dvoff = inner;
    fa.drop_site = site + 2;
    launch_flash_bwd(false, fa, H, d_work, n_work, d_kwork, n_kwork, s);
    // the launch order of the two cross projections is kept: all three weight gradients, the K | V projection's dX (over
    // the source rows, added into d_enc), then the q projection's dX
    if ((st = lin(w.dcq, b.h1, l.cq, inner, D, {{0, inner, Gl(G_CQ)}}, DX_NONE, nullptr))) return st;
    if ((st = linear_bwd(w.dkv, w.encp, n_src, Sp, d->cross_kv_w + (size_t)2 * i * inner * D, 2 * inner, D,
                         {{0, inner, Gl(G_CK)}, {inner, inner, Gl(G_CV)}}, d_enc ? DX_F32_ADD : DX_NONE, d_enc, w.wt, s)))
      return st;
    if ((st = lin(w.dcq, b.h1, l.cq, inner, D, {}, DX_F32, w.dh))) return st;
    norm_bwd(b.x1, l.ln_cross, 1.f, true, Gl(G_LN_CROSS));

    // self-attention
    cast_dx(site + 1);
    if ((st = lin(w.dyb, b.att_s, l.wo, D, inner, {{0, D, Gl(G_O)}}, DX_BF16, w.datt))) return st;
    fa.q = b.qkv; fa.ldq = 3 * inner;
    fa.kv = b.qkv; fa.ldkv = 3 * inner; fa.koff = inner; fa.voff = 2 * inner;
    fa.k_cu = d_tgt_cu;
    fa.o = b.att_s; fa.d_o = w.datt;
    fa.lse2 = b.lse_s;
    fa.dq = w.dqkv; fa.lddq = 3 * inner;
    fa.dkv = w.dqkv; fa.lddkv = 3 * inner; fa.dkoff = inner; fa.dvoff = 2 * inner;
    fa.drop_site = site;
    launch_flash_bwd(true, fa, H, d_work, n_work, d_work, n_work, s);
    if ((st = lin(w.dqkv, b.h0, l.wqkv, 3 * inner, D,
                  {{0, inner, Gl(G_Q)}, {inner, inner, Gl(G_K)}, {2 * inner, inner, Gl(G_V)}}, DX_F32, w.dh)))
      return st;
    norm_bwd(b.x0, l.ln_self, 1.f, true, Gl(G_LN_SELF));
  }
  // the shared bias table (every layer added into the same partial rows) and the embedding
  launch_bias_grad(w.dtab_part, n_work, H, d->nbias, d_bucket, c.rel_num_buckets, G(lay.rel_bias()), s);
  launch_embed_bwd(d->tied, tokens, n_tgt, V, w.dx, D, G(lay.shared()), s, drop);  // tied: the head's weight gradient is already there
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_decoder_loss_grad(RpDecoder* d, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                                         const int32_t* labels, const int32_t* tgt_cu, int32_t batch,
                                         float* label_logprobs, double* loss_sum_count, float* grads, float* d_enc,
                                         void* ws, size_t ws_bytes, void* stream_) {
  return loss_grad(d, enc_bf16, src_cu, tokens, labels, tgt_cu, batch, NO_DROP, label_logprobs, loss_sum_count, grads, d_enc, ws,
                   ws_bytes, stream_);
}

extern "C" RpStatus rp_decoder_loss_grad_dropout(RpDecoder* d, const void* enc_bf16, const int32_t* src_cu, const int32_t* tokens,
                                                 const int32_t* labels, const int32_t* tgt_cu, int32_t batch, float p,
                                                 uint32_t seed, float* label_logprobs, double* loss_sum_count, float* grads,
                                                 float* d_enc, void* ws, size_t ws_bytes, void* stream_) {
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  return loss_grad(d, enc_bf16, src_cu, tokens, labels, tgt_cu, batch, make_drop(p, seed), label_logprobs, loss_sum_count, grads,
                   d_enc, ws, ws_bytes, stream_);
}

// ---- kernel-level test entry points (include/reprover_hip.h: tests/test_decoder_kernels_gpu.py) -----------------------------
// The attention kernels alone on caller-supplied operands in the product's layouts, through the product's work lists and
// launch functions.  Scratch (metadata, table partials) is allocated here; no output is zeroed.
static RpStatus dbg_attention(int32_t causal, const void* q, const void* kv, const void* d_o, const int32_t* q_cu,
                              const int32_t* k_cu, int32_t batch, int32_t H, const float* bias_tab, int32_t nbias,
                              const int32_t* bucket_of, int32_t nbuckets, const Drop& drop, uint32_t drop_site, void* out,
                              float* lse2, float* delta, void* dq, void* dkv, float* dtab, void* stream_) {
  RP_REQUIRE(q && d_o && q_cu && out && lse2 && delta && dq, "null argument");
  RP_REQUIRE(H >= 1 && H <= 64, "H=%d", H);
  if (causal) {
    RP_REQUIRE(bias_tab && bucket_of && dtab && nbias >= 1 && nbias <= FA_TAB_MAX && nbuckets >= 1, "causal: table arguments");
    for (int i = 0; i < nbias; ++i) RP_REQUIRE(bucket_of[i] >= 0 && bucket_of[i] < nbuckets, "bucket_of[%d]=%d", i, bucket_of[i]);
    k_cu = q_cu;
  } else {
    RP_REQUIRE(kv && k_cu && dkv, "cross: null argument");
  }
  int n_src = 0, n_tgt = 0;
  RpStatus st = fwd_check_cu(k_cu, q_cu, batch, n_src, n_tgt);
  if (st) return st;
  RP_REQUIRE(n_tgt > 0, "no query row");
  hipStream_t s = (hipStream_t)stream_;
  const int inner = H * 64, Tp = (int)align_up(n_tgt, FWD_BN);
  std::vector<int32_t> meta;
  const int n_work = fwd_build_meta(k_cu, q_cu, batch, meta);
  const size_t kwork_at = meta.size();
  const int n_kwork = causal ? n_work : bwd_build_kwork(k_cu, q_cu, batch, meta);
  const size_t bucket_at = meta.size();
  if (causal) meta.insert(meta.end(), bucket_of, bucket_of + nbias);
  int32_t* d_meta = nullptr;
  float* part = nullptr;
  const size_t part_bytes = causal ? (size_t)n_work * H * nbias * 4 : 0;
  RP_HIP(hipMalloc((void**)&d_meta, meta.size() * 4));
  if (part_bytes && hipMalloc((void**)&part, part_bytes) != hipSuccess) {
    (void)hipFree(d_meta);
    return fail(RP_E_HIP, "hipMalloc of the table partials failed");
  }
  auto done = [&](RpStatus r) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_meta);
    if (part) (void)hipFree(part);
    return r;
  };
  if (hipMemcpyAsync(d_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      (part && hipMemsetAsync(part, 0, part_bytes, s) != hipSuccess))
    return done(fail(RP_E_HIP, "metadata upload failed"));
  const int32_t* d_src_cu = d_meta;
  const int32_t* d_tgt_cu = d_meta + batch + 1;
  const int2* d_work = reinterpret_cast<const int2*>(d_meta + 2 * (batch + 1));
  const int2* d_kwork = causal ? d_work : reinterpret_cast<const int2*>(d_meta + kwork_at);
  FlashBwdArgs fa{};
  fa.q_cu = d_tgt_cu;
  fa.bias_tab = bias_tab;
  fa.nbias = causal ? nbias : 1;
  fa.ldo = inner;
  fa.delta = delta;
  fa.ld_stat = Tp;
  fa.dtab_part = part;
  fa.drop = drop;
  fa.drop_site = drop_site;
  fa.o = (const bf16_t*)out;
  fa.d_o = (const bf16_t*)d_o;
  fa.lse2 = lse2;
  fa.q = (const bf16_t*)q;
  if (causal) {
    fa.ldq = 3 * inner;
    fa.kv = (const bf16_t*)q; fa.ldkv = 3 * inner; fa.koff = inner; fa.voff = 2 * inner;
    fa.k_cu = d_tgt_cu;
    fa.dq = (bf16_t*)dq; fa.lddq = 3 * inner;
    fa.dkv = (bf16_t*)dq; fa.lddkv = 3 * inner; fa.dkoff = inner; fa.dvoff = 2 * inner;
  } else {
    fa.ldq = inner;
    fa.kv = (const bf16_t*)kv; fa.ldkv = 2 * inner; fa.koff = 0; fa.voff = inner;
    fa.k_cu = d_src_cu;
    fa.dq = (bf16_t*)dq; fa.lddq = inner;
    fa.dkv = (bf16_t*)dkv; fa.lddkv = 2 * inner; fa.dkoff = 0; fa.dvoff = inner;
  }
  launch_dec_flash(causal != 0, fa.q, fa.ldq, fa.kv, fa.ldkv, fa.koff, fa.voff, fa.q_cu, fa.k_cu, d_work, n_work, H, bias_tab,
                   fa.nbias, (bf16_t*)out, inner, lse2, Tp, s, drop, drop_site);
  launch_flash_bwd(causal != 0, fa, H, d_work, n_work, d_kwork, n_kwork, s);
  if (causal) launch_bias_grad(part, n_work, H, nbias, d_meta + bucket_at, nbuckets, dtab, s);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return done(fail(RP_E_HIP, "decoder attention launch failed: %s", hipGetErrorString(le)));
  return done(RP_OK);
}

extern "C" RpStatus rp_dbg_decoder_attention(int32_t causal, const void* q, const void* kv, const void* d_o,
                                             const int32_t* q_cu, const int32_t* k_cu, int32_t batch, int32_t H,
                                             const float* bias_tab, int32_t nbias, const int32_t* bucket_of, int32_t nbuckets,
                                             void* out, float* lse2, float* delta, void* dq, void* dkv, float* dtab,
                                             void* stream_) {
  return dbg_attention(causal, q, kv, d_o, q_cu, k_cu, batch, H, bias_tab, nbias, bucket_of, nbuckets, NO_DROP, 0u, out, lse2,
                       delta, dq, dkv, dtab, stream_);
}

// rp_dbg_decoder_attention with the probabilities dropped at (p, seed, site): the same launch functions in their dropout form
extern "C" RpStatus rp_dbg_decoder_attention_dropout(int32_t causal, const void* q, const void* kv, const void* d_o,
                                                     const int32_t* q_cu, const int32_t* k_cu, int32_t batch, int32_t H,
                                                     const float* bias_tab, int32_t nbias, const int32_t* bucket_of,
                                                     int32_t nbuckets, float p, uint32_t seed, uint32_t site, void* out,
                                                     float* lse2, float* delta, void* dq, void* dkv, float* dtab,
                                                     void* stream_) {
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  return dbg_attention(causal, q, kv, d_o, q_cu, k_cu, batch, H, bias_tab, nbias, bucket_of, nbuckets, make_drop(p, seed), site,
                       out, lse2, delta, dq, dkv, dtab, stream_);
}

// The embedding site's two kernels alone, both fp32 end to end: x [n_tok, n] = mask * embed[ids] (dec_embed_drop_kernel) and
// dtable [vocab, n] = the per-id sum of mask * dx (bwd_embed_kernel<false, true>), the mask of (DROP_SITE_DEC_EMBED, row =
// token, column = feature).  On a table of ones x IS the multiplier: exactly 0 or fp32 1 / (1 - p).
extern "C" RpStatus rp_dbg_decoder_embed_dropout(const int32_t* ids, int32_t n_tok, const float* embed, int32_t vocab, int32_t n,
                                                 float p, uint32_t seed, const float* dx, float* x, float* dtable, void* stream_) {
  RP_REQUIRE(ids && embed && dx && x && dtable && n_tok >= 1 && vocab >= 1 && n >= 1, "bad argument");
  RP_REQUIRE(p > 0.f && p < 1.f, "dropout probability %g", (double)p);
  hipStream_t s = (hipStream_t)stream_;
  const Drop drop = make_drop(p, seed);
  hipLaunchKernelGGL(dec_embed_drop_kernel, dim3(n_tok), dim3(256), 0, s, ids, embed, x, n, vocab, drop);
  launch_embed_bwd(false, ids, n_tok, vocab, dx, n, dtable, s, drop);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// The row kernels of the decoder backward, one per mode, through the product's launch functions:
//   0 dlogits   a = logits f32 [rows_pad, n], ia = labels [n_tok], b = loss_sum_count f64 [2]; o0 = bf16 [rows_pad, n]
//   1 cast      a = f32 [rows_pad, n]; o0 = bf16 [rows_pad, n]
//   2 rmsnorm   a = x f32 [n_tok, n], b = ln f32 [n], o0 = dh f32 [n_tok, n] (in: dh, out: the rows' terms of d ln),
//               o1 = dx f32 [n_tok, n] (flag: added to), o2 = d ln f32 [n]; eps, scale
//   3 geglu     a = gate | up f32 [rows_pad, 2 n] (interleaved by 32), b = dff f32 [rows_pad, n]; o0 = bf16 [rows_pad, 2 n]
//   4 embed     ia = ids [n_tok], a = dx f32 [n_tok, n]; o0 = table gradient f32 [vocab, n] (flag: added to)
extern "C" RpStatus rp_dbg_decoder_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t n_tok,
                                        int32_t rows_pad, int32_t n, int32_t vocab, int32_t flag, float eps, float scale,
                                        void* o0, void* o1, void* o2, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  RP_REQUIRE(a && o0 && n >= 1 && n_tok >= 0, "bad argument");
  switch (mode) {
    case 0:
      RP_REQUIRE(b && ia && n <= FWD_MAX_VOCAB && rows_pad >= n_tok && rows_pad >= 1, "dlogits: bad argument");
      launch_dlogits((const float*)a, n, n_tok, rows_pad, ia, (const double*)b, (bf16_t*)o0, s);
      break;
    case 1:
      RP_REQUIRE(rows_pad >= n_tok && rows_pad >= 1, "cast: bad argument");
      launch_cast((const float*)a, (bf16_t*)o0, n, n_tok, rows_pad, s);
      break;
    case 2:
      RP_REQUIRE(b && o1 && o2 && n_tok >= 1, "rmsnorm: bad argument");
      launch_norm_bwd((const float*)a, (const float*)b, (float*)o0, (float*)o1, n_tok, n, eps, scale, flag != 0, (float*)o2, s);
      break;
    case 3:
      RP_REQUIRE(b && n % 64 == 0 && rows_pad >= n_tok && rows_pad >= 1, "geglu: bad argument");
      launch_geglu_bwd((const float*)a, (const float*)b, (bf16_t*)o0, n, n_tok, rows_pad, s);
      break;
    case 4:
      RP_REQUIRE(ia && vocab >= 1 && n_tok >= 1, "embed: bad argument");
      launch_embed_bwd(flag != 0, ia, n_tok, vocab, (const float*)a, n, (float*)o0, s);
      break;
    default:
      return fail(RP_E_INVALID, "mode=%d", mode);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}
