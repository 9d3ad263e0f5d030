// Decoder state and the kernels shared by the decode step (rp_decoder.hip), its batched form (rp_decoder_batch.hip) and
// the teacher-forced forward (rp_decoder_forward.hip).  Every reduction here runs in a fixed order that depends only on the row length.
#pragma once
#include <vector>

#include "rp_util.h"

namespace {
using namespace rp;

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// 256-thread block reductions in a fixed order (wave butterflies, then the four waves in index order)
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max256(float v, float* red) {
  v = wave_max64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// x[b, :] = embed[tokens[b], :]   (fp32 residual stream)
__global__ __launch_bounds__(256) void dec_embed_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ embed,
                                                        float* __restrict__ x, int D, int V) {
  const int b = blockIdx.x;
  const int tok = min(max(tokens[b], 0), V - 1);
  for (int c = threadIdx.x; c < D; c += 256) x[(size_t)b * D + c] = embed[(size_t)tok * D + c];
}

// out[b, :] = bf16(w * (x * rsqrt(mean(x^2) + eps)) * scale)   (T5LayerNorm; scale = d_model^-0.5 on a tied lm_head)
__global__ __launch_bounds__(256) void dec_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          bf16_t* __restrict__ out, int D, float eps, float scale) {
  __shared__ float red[4];
  const float* row = x + (size_t)blockIdx.x * D;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) ss = fmaf(row[c], row[c], ss);
  ss = block_sum256(ss, red);
  const float r = rsqrtf(ss / (float)D + eps);
  for (int c = threadIdx.x; c < D; c += 256) out[(size_t)blockIdx.x * D + c] = f2bf(w[c] * (row[c] * r) * scale);
}

// dst rows [64 k, 64 k + 32) = wi rows [32 k, 32 k + 32) (wi_0), rows [64 k + 32, 64 k + 64) = wi rows [F + 32 k, ...)
// (wi_1): the gate and up rows of the same 32 features side by side (d_ff % 32 == 0)
__global__ void dec_interleave_kernel(bf16_t* __restrict__ dst, const bf16_t* __restrict__ wi, int F, int D) {
  const int r = blockIdx.x;  // destination row, < 2 F
  const int blk = r >> 6, in = r & 63;
  const int src = (in < 32 ? 0 : F) + 32 * blk + (in & 31);
  for (int c = threadIdx.x; c < D; c += blockDim.x) dst[(size_t)r * D + c] = wi[(size_t)src * D + c];
}

__device__ __forceinline__ float gelu_tanh(float u) {
  return 0.5f * u * (1.f + tanhf(0.7978845608028654f * (u + 0.044715f * u * u * u)));
}

// ---- the decode step's kernels, shared by the per-state step (rp_decoder.hip) and the batched one (rp_decoder_batch.hip)
constexpr int DEC_MAX_BEAMS = 64;
constexpr int DEC_MAX_KIT = 8;          // GEMM K <= 8 * 512 = 4096 (a wave holds its weight row in registers)
constexpr int DEC_MAX_KEYS = 8192;      // attention keys per launch (fp32 scores in dynamic LDS: 32 KB)
constexpr int DEC_SELECT_MAX_K = 128;   // 2 * DEC_MAX_BEAMS
constexpr int DEC_SELECT_ROW = 512;     // the per-row sort covers vocab <= 512
constexpr int DEC_MERGE = 8192;         // nb * min(k, vocab) candidates <= 64 * 128

enum DecEpi { EPI_BF16 = 0, EPI_RESID = 1, EPI_F32 = 2, EPI_GEGLU = 3 };

__device__ __forceinline__ float dot8(uint4 a, uint4 w, float acc) {
  const uint32_t av[4] = {a.x, a.y, a.z, a.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc = fmaf(__uint_as_float(av[i] << 16), __uint_as_float(wv[i] << 16), acc);
    acc = fmaf(__uint_as_float(av[i] & 0xffff0000u), __uint_as_float(wv[i] & 0xffff0000u), acc);
  }
  return acc;
}

// out[m, n] = sum_k A[m, k] W[n, k] for rows m in [m0, m0 + 64) of this workgroup row, one wave per output column n.  The
// wave keeps its weight row (KIT x 512 elements) in registers and streams the A rows past it; lane l covers the 16-byte
// pieces l, l + 64, ... of K, and the 64 lane sums are combined by one xor butterfly: the same chain for every (m, n).
// EPI_GEGLU: column n reads W rows n (wi_0) and n + N (wi_1), out = gelu_new(a0) * a1.
template <int KIT, int EPI>
__global__ __launch_bounds__(256) void dec_gemm_kernel(const bf16_t* __restrict__ A, int lda, int M,
                                                       const bf16_t* __restrict__ W, int N, int K,
                                                       void* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int nk = K >> 3;  // 16-byte pieces per row
  uint4 w0[KIT], w1[KIT];
#pragma unroll
  for (int i = 0; i < KIT; ++i) {
    const int j = lane + 64 * i;
    w0[i] = (j < nk) ? reinterpret_cast<const uint4*>(W + (size_t)n * K)[j] : make_uint4(0u, 0u, 0u, 0u);
    if constexpr (EPI == EPI_GEGLU)
      w1[i] = (j < nk) ? reinterpret_cast<const uint4*>(W + (size_t)(n + N) * K)[j] : make_uint4(0u, 0u, 0u, 0u);
  }
  const int m1 = min(M, (int)(blockIdx.y + 1) * 64);
  for (int m = blockIdx.y * 64; m < m1; ++m) {
    const uint4* a = reinterpret_cast<const uint4*>(A + (size_t)m * lda);
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int i = 0; i < KIT; ++i) {
      const int j = lane + 64 * i;
      const uint4 av = (j < nk) ? a[j] : make_uint4(0u, 0u, 0u, 0u);
      acc0 = dot8(av, w0[i], acc0);
      if constexpr (EPI == EPI_GEGLU) acc1 = dot8(av, w1[i], acc1);
    }
    acc0 = wave_sum64(acc0);
    if constexpr (EPI == EPI_GEGLU) acc1 = wave_sum64(acc1);
    if (lane == 0) {
      if constexpr (EPI == EPI_BF16) reinterpret_cast<bf16_t*>(out)[(size_t)m * ldo + n] = f2bf(acc0);
      if constexpr (EPI == EPI_RESID) reinterpret_cast<float*>(out)[(size_t)m * ldo + n] += acc0;
      if constexpr (EPI == EPI_F32) reinterpret_cast<float*>(out)[(size_t)m * ldo + n] = acc0;
      if constexpr (EPI == EPI_GEGLU) reinterpret_cast<bf16_t*>(out)[(size_t)m * ldo + n] = f2bf(gelu_tanh(acc0) * acc1);
    }
  }
}

template <int EPI>
RpStatus launch_dec_gemm(const bf16_t* A, int lda, int M, const bf16_t* W, int N, int K, void* out, int ldo,
                         hipStream_t s) {
  const int kit = (K / 8 + 63) / 64;
  const dim3 grid((N + 3) / 4, (M + 63) / 64);
#define DEC_GEMM_CASE(I) \
  case I: hipLaunchKernelGGL((dec_gemm_kernel<I, EPI>), grid, dim3(256), 0, s, A, lda, M, W, N, K, out, ldo); break;
  switch (kit) {
    DEC_GEMM_CASE(1) DEC_GEMM_CASE(2) DEC_GEMM_CASE(3) DEC_GEMM_CASE(4)
    DEC_GEMM_CASE(5) DEC_GEMM_CASE(6) DEC_GEMM_CASE(7) DEC_GEMM_CASE(8)
    default: return fail(RP_E_UNSUPPORTED, "decoder GEMM K=%d > %d", K, DEC_MAX_KIT * 512);
  }
#undef DEC_GEMM_CASE
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// One (head, row) of decoder attention: softmax(q k^T + bias) v over `len` keys, d_kv = 64, fp32 scores in s_sc (dynamic
// LDS, >= len floats), by one 256-thread workgroup.  q / out point at the row's own q and output row, anc at its ancestry
// row (or null).  Key p lives in row r(p) of kv (r = anc[p] clamped to [0, rows), or p); K at column koff + 64 h, V at
// voff + 64 h.  bias (self-attention): tab[h * nbias + min(len - 1 - p, nbias - 1)] (distance query - key).  The
// reductions (strided max / sum / PV loops, the 4-wave combine) depend on len alone.
__device__ __forceinline__ void dec_attention_row(float* __restrict__ s_sc, const bf16_t* __restrict__ q,
                                                  const bf16_t* __restrict__ kv, int ldkv, int koff, int voff, int rows,
                                                  const int32_t* __restrict__ anc, const float* __restrict__ tab,
                                                  int nbias, int len, bf16_t* __restrict__ out, int h) {
  __shared__ float s_q[64];
  __shared__ float red[4];
  __shared__ float s_part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 64) s_q[tid] = bf2f(q[h * 64 + tid]);
  __syncthreads();
  float mx = -INFINITY;
  for (int p = tid; p < len; p += 256) {
    int r = anc ? anc[p] : p;
    r = min(max(r, 0), rows - 1);
    const uint4* kr = reinterpret_cast<const uint4*>(kv + (size_t)r * ldkv + koff + h * 64);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint4 k8 = kr[i];
      const uint32_t kw[4] = {k8.x, k8.y, k8.z, k8.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc = fmaf(s_q[8 * i + 2 * e], __uint_as_float(kw[e] << 16), acc);
        acc = fmaf(s_q[8 * i + 2 * e + 1], __uint_as_float(kw[e] & 0xffff0000u), acc);
      }
    }
    if (tab) acc += tab[(size_t)h * nbias + min(len - 1 - p, nbias - 1)];
    s_sc[p] = acc;
    mx = fmaxf(mx, acc);
  }
  mx = block_max256(mx, red);
  float sum = 0.f;
  for (int p = tid; p < len; p += 256) {
    const float e = __expf(s_sc[p] - mx);
    s_sc[p] = e;
    sum += e;
  }
  sum = block_sum256(sum, red);  // (its leading barrier also publishes s_sc)
  float acc = 0.f;
  for (int p = wave; p < len; p += 4) {
    int r = anc ? anc[p] : p;
    r = min(max(r, 0), rows - 1);
    acc = fmaf(s_sc[p], bf2f(kv[(size_t)r * ldkv + voff + h * 64 + lane]), acc);
  }
  s_part[wave][lane] = acc;
  __syncthreads();
  if (tid < 64) {
    const float o = ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) / sum;
    out[h * 64 + tid] = f2bf(o);
  }
}

__global__ __launch_bounds__(256) void dec_log_softmax_kernel(float* __restrict__ x, int V) {
  __shared__ float red[4];
  float* row = x + (size_t)blockIdx.x * V;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, row[c]);
  mx = block_max256(mx, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) s += __expf(row[c] - mx);
  s = block_sum256(s, red);
  const float ls = logf(s);
  for (int c = threadIdx.x; c < V; c += 256) row[c] = (row[c] - mx) - ls;
}


// Keys sort descending: high 32 bits = the score made order-preserving as an unsigned integer, low 32 = ~flat index (a
// lower index ranks higher on equal scores, torch.topk's order).  -0.0 is keyed as +0.0: the two compare equal, so the
// index decides between them.  NaN scores are outside the contract.
__device__ __forceinline__ uint64_t sel_key(float v, uint32_t idx) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(~idx);
}
__device__ __forceinline__ float key_score(uint64_t k) {
  uint32_t u = (uint32_t)(k >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}
// bitonic sort, descending, of n (power of two) keys in LDS by the whole workgroup
__device__ void bitonic_desc(uint64_t* s, int n) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int j = i ^ stride;
        if (j > i) {
          const bool desc = (i & size) == 0;
          const uint64_t a = s[i], c = s[j];
          if (desc ? (a < c) : (a > c)) {
            s[i] = c;
            s[j] = a;
          }
        }
      }
    }
  __syncthreads();
}

}  // namespace

struct RpDecoder {
  RpT5Config cfg;
  int inner = 0, nbias = 0, tied = 0;
  float* embed = nullptr;     // [V, D] fp32
  float* final_ln = nullptr;  // [D]
  bf16_t* lm_head = nullptr;  // [V, D]
  bf16_t* cross_kv_w = nullptr;  // [L * 2 * inner, D]: layer l's k rows at 2 l inner, v rows at (2 l + 1) inner
  float* bias_tab = nullptr;     // [H, nbias] by distance query - key (clamped)
  struct Layer {
    float *ln_self, *ln_cross, *ln_ff;
    bf16_t *wqkv, *wo, *cq, *co, *wi, *wo2;
  };
  std::vector<Layer> layers;
  // rp_decoder_forward's FFN-in operand (packed at create time): per layer [wi_0; wi_1] re-ordered into 64-row blocks of
  // 32 gate rows then the same 32 up rows, [L][2 * d_ff, d_model] bf16
  bf16_t* wi_il = nullptr;
  std::vector<void*> allocs;
};
