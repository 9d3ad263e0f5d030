// Decoder state and the row kernels shared by the decode step (rp_decoder.hip) and the teacher-forced forward
// (rp_decoder_forward.hip).  Every reduction here runs in a fixed order that depends only on the row length.
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
  // rp_decoder_load_params (rp_decoder.hip): the device-resident descriptor table of every resident copy above, built once
  // at create, and the distance -> bucket index of bias_tab's columns (nbias int32)
  void* reload_tab = nullptr;
  int32_t* bias_bucket = nullptr;
  int reload_entries = 0, reload_chunks = 0;
  std::vector<void*> allocs;
};
