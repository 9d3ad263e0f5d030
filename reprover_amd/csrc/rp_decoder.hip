// libreprover_hip - the tactic generator's T5 decoder (include/reprover_hip.h).
//
// One beam-search step for the nb <= 64 beams of each of 1..32 proof states: per layer RMSNorm -> fused self QKV ->
// causal self-attention over the ancestry-addressed cache -> o + residual -> RMSNorm -> cross q -> cross-attention over
// the source -> o + residual -> gated-GELU FFN; then the final norm, lm_head and log_softmax.  Precision: bf16 weights and
// GEMM operands, fp32 accumulation, statistics, softmax and residual stream, fp32 log-probs.
//
// The rows of a step are the n_active * nb beams of the states that are still searching, packed slot by slot.  Embed,
// RMSNorm, every projection, lm_head and log_softmax are row-wise and run over all rows in one launch each; the two
// attentions run as one launch over (head, row), each row finding its state's cache, cross K/V and source length through
// the slot table passed by value.  rp_decoder_step / rp_decoder_cross_kv / rp_beam_select are the one-state calls of
// rp_decoder_batch_step / rp_decoder_batch_cross_kv / rp_beam_select_batch: there is one launch sequence.
// rp_decoder_pool_step is that sequence with a position per slot (the batched call: every slot at t), over a workspace
// whose slots states enter between steps (rp_decoder_pool_admit): continuous batching.
// rp_decoder_batch_step_pos is the batched call with a position per listed state.  rp_decoder_batch_prefill /
// rp_decoder_pool_prefill write a decoder prompt's cache rows - one per prompt position, beam 0's, shared by all beams of
// the state - for all positions of all listed states through the step's own launch sequence (dec_layers_launch) and
// kernels, the rows found through a segment table (DecSegs) instead of the slot table, so that the rows are the bits the
// step writes.  Behind the entries: one list check (dec_list), one geometry of the workspace (DecGeom, from src_cu or from
// the pool's slots), one step (dec_step) and one prefill (dec_prefill).
// rp_sample_step (sampling) and rp_beam_books_init / rp_beam_advance (beam search) keep a search's bookkeeping on the
// device, one more launch per step, so that the host loop reads nothing back per position.  rp_beam_pool_advance is
// rp_beam_advance with a position per slot (one kernel: the uniform call has every slot at t), and rp_beam_books_admit /
// rp_beam_books_rows give a slot's next tenant fresh books and rebuild the by-row inputs when the active list changes:
// the slot pool's books.  rp_sample_pool_step / rp_sample_pool_admit / rp_sample_pool_rows are the same three for the
// sampler's books (rp_sample_step: the call in which every slot has pos = t).
//
// Every output element of every kernel here is computed by a reduction whose order depends only on the shapes (K, the
// key count), never on which other rows share the launch or where the row sits in it: a row's log-probs are the same
// bits batched or alone.
#include <algorithm>
#include <vector>

#include "rp_decoder_common.h"

using namespace rp;

namespace {

constexpr int DEC_MAX_BEAMS = 64;
constexpr int DEC_MAX_KIT = 8;          // GEMM K <= 8 * 512 = 4096 (a wave holds its weight row in registers)
constexpr int DEC_MAX_KEYS = 8192;      // attention keys per launch (fp32 scores in dynamic LDS: 32 KB)
constexpr int DEC_SELECT_MAX_K = 128;   // 2 * DEC_MAX_BEAMS
constexpr int DEC_SELECT_ROW = 512;     // the per-row sort covers vocab <= 512
constexpr int DEC_MERGE = 8192;         // nb * min(k, vocab) candidates <= 64 * 128
constexpr int DEC_MAX_STATES = 32;      // states per call (a 32-bit mask checks the active list)
constexpr int DEC_MAX_ROWS = 1024;      // states * nb: 16 states of 64 beams, 32 of 32 or fewer

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

// per active slot: the state it carries, where that state's source sits in the cross K/V, and the position the slot's
// beams stand at (the decode step's: one value for the whole call from rp_decoder_batch_step, one per slot from
// rp_decoder_pool_step)
struct DecSlots {
  int32_t state[DEC_MAX_STATES];
  int32_t src_off[DEC_MAX_STATES];
  int32_t src_len[DEC_MAX_STATES];
  int32_t pos[DEC_MAX_STATES];
};

// ---- prompt prefill ("Tactic prefix") ---------------------------------------------------------------
// The rows of one prefill pass, by segment: segment g is rows row0[g] .. row0[g + 1] of the pass (row0 ascending, the
// last segment runs to the pass's end), the prompt positions pos0[g], pos0[g] + 1, ... of one state.  A prompt is shared
// by the state's beams: the row at position p is stored as cache row p * nb (beam 0's) and nowhere else.
struct DecSegs {
  int32_t n;
  int32_t state[DEC_MAX_STATES];
  int32_t src_off[DEC_MAX_STATES];
  int32_t src_len[DEC_MAX_STATES];
  int32_t pos0[DEC_MAX_STATES];
  int32_t row0[DEC_MAX_STATES];
};
__device__ __forceinline__ int dec_seg_of(const DecSegs& segs, int row) {
  int g = 0;
  for (int i = 1; i < segs.n; ++i)
    if (row >= segs.row0[i]) g = i;
  return g;
}

// What a row table (DecSlots: the rows of a step; DecSegs: the rows of a prefill pass) says of one row of its launch: the
// row's state, that state's source rows of the cross K/V, the row's position and beam - it is stored in row pos * nb + beam
// of the state's cache - and its ancestry row.  A step's row is beam row - slot * nb of its slot, with its own row of the
// ancestry table; a prompt row is beam 0's, and every prompt row reads the caller's one vector p' -> p' * nb.
struct DecRow {
  int state, src_off, src_len, pos, beam;
  const int32_t* anc;
  __device__ __forceinline__ int cache_row(int nb) const { return pos * nb + beam; }
};
__device__ __forceinline__ DecRow dec_row(const DecSlots& slots, int row, int nb, const int32_t* anc, int astride) {
  const int slot = row / nb, b = row - slot * nb;
  return {slots.state[slot], slots.src_off[slot], slots.src_len[slot], slots.pos[slot], b, anc + (size_t)row * astride};
}
__device__ __forceinline__ DecRow dec_row(const DecSegs& segs, int row, int, const int32_t* anc, int) {
  const int g = dec_seg_of(segs, row);
  return {segs.state[g], segs.src_off[g], segs.src_len[g], segs.pos0[g] + (row - segs.row0[g]), 0, anc};
}
// the longest self-attention key list and the longest source among the M rows of a launch (the dynamic LDS holds them)
int dec_max_keys(const DecSlots& slots, int M, int nb) {
  int keys = 0;
  for (int a = 0; a < M / nb; ++a) keys = std::max(keys, slots.pos[a] + 1);
  return keys;
}
int dec_max_keys(const DecSegs& segs, int M, int) {
  int keys = 0;  // the largest position the pass reaches, plus one
  for (int g = 0; g < segs.n; ++g) keys = std::max(keys, segs.pos0[g] + (g + 1 < segs.n ? segs.row0[g + 1] : M) - segs.row0[g]);
  return keys;
}
int dec_max_src(const DecSlots& slots, int M, int nb) { return *std::max_element(slots.src_len, slots.src_len + M / nb); }
int dec_max_src(const DecSegs& segs, int, int) { return *std::max_element(segs.src_len, segs.src_len + segs.n); }

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

// One (head, row) per workgroup, the row found through its table (dec_row).  Self-attention (CROSS = false): the state's
// own cache of `rows` = max_len * nb rows at kv + state * state_stride, keys through the row's ancestry entries (local to
// that cache), pos + 1 keys: entries 0 .. pos (the dynamic LDS holds the launch's largest pos + 1 scores).  Cross-attention:
// the state's source rows of the cross K/V, all src_len keys, no bias.  A prompt row (DecSegs) runs dec_attention_row as
// the step runs it, so its bits are those of the step at its position for beam 0.
template <bool CROSS, typename Rows>
__global__ __launch_bounds__(256) void dec_attention_kernel(const bf16_t* __restrict__ q, int ldq,
                                                            const bf16_t* __restrict__ kv, int ldkv, int koff, int voff,
                                                            int rows, size_t state_stride,
                                                            const int32_t* __restrict__ anc, int astride,
                                                            const float* __restrict__ tab, int nbias, int nb, Rows table,
                                                            bf16_t* __restrict__ out, int ldo) {
  extern __shared__ float s_sc[];
  const int h = blockIdx.x, row = blockIdx.y;
  const DecRow r = dec_row(table, row, nb, anc, astride);
  if constexpr (CROSS)
    dec_attention_row(s_sc, q + (size_t)row * ldq, kv + (size_t)r.src_off * ldkv, ldkv, koff, voff, r.src_len, nullptr,
                      nullptr, 1, r.src_len, out + (size_t)row * ldo, h);
  else
    dec_attention_row(s_sc, q + (size_t)row * ldq, kv + (size_t)r.state * state_stride, ldkv, koff, voff, rows, r.anc, tab,
                      nbias, r.pos + 1, out + (size_t)row * ldo, h);
}

// The two attention launches over the M rows of a row table (dec_layers_launch and the test entry rp_dbg_dec_attention
// both launch through here): one workgroup per (head, row), the dynamic LDS holds the launch's longest key list.
template <typename Rows>
void launch_dec_self_attention(const bf16_t* q, int ldq, const bf16_t* cache, int ldkv, int koff, int voff, int rows,
                               size_t state_stride, const int32_t* anc, int astride, const float* tab, int nbias, int nb,
                               int H, const Rows& table, int M, bf16_t* out, int ldo, hipStream_t s) {
  hipLaunchKernelGGL((dec_attention_kernel<false, Rows>), dim3(H, M), dim3(256), dec_max_keys(table, M, nb) * sizeof(float), s,
                     q, ldq, cache, ldkv, koff, voff, rows, state_stride, anc, astride, tab, nbias, nb, table, out, ldo);
}
template <typename Rows>
void launch_dec_cross_attention(const bf16_t* q, int ldq, const bf16_t* ckv, int ldkv, int koff, int voff, int nb, int H,
                                const Rows& table, int M, bf16_t* out, int ldo, hipStream_t s) {
  hipLaunchKernelGGL((dec_attention_kernel<true, Rows>), dim3(H, M), dim3(256), dec_max_src(table, M, nb) * sizeof(float), s, q,
                     ldq, ckv, ldkv, koff, voff, 0, (size_t)0, (const int32_t*)nullptr, 0, (const float*)nullptr, 1, nb, table,
                     out, ldo);
}

// the row's cache row of its state <- the k, v columns of qkv[row]
template <typename Rows>
__global__ __launch_bounds__(256) void dec_store_kv_kernel(const bf16_t* __restrict__ qkv, int inner,
                                                           bf16_t* __restrict__ cache, size_t state_stride, int nb,
                                                           Rows table) {
  const int row = blockIdx.x;
  const DecRow r = dec_row(table, row, nb, nullptr, 0);
  bf16_t* dst = cache + (size_t)r.state * state_stride + (size_t)r.cache_row(nb) * 2 * inner;
  for (int c = threadIdx.x; c < 2 * inner; c += 256) dst[c] = qkv[(size_t)row * 3 * inner + inner + c];
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

// ---- beam selection ---------------------------------------------------------------------------------------------------
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

// per beam row (row = slot * nb + b): the top kr keys of logprobs[row, :] + running[row], keyed by the flat index
// b * V + i inside the state's own block
__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ lp, const float* __restrict__ running,
                                                            int V, int kr, int nb, uint64_t* __restrict__ cand) {
  __shared__ uint64_t s[DEC_SELECT_ROW];
  const int row = blockIdx.x, b = row % nb;
  const float rb = running[row];
  for (int i = threadIdx.x; i < DEC_SELECT_ROW; i += 256)
    s[i] = (i < V) ? sel_key(lp[(size_t)row * V + i] + rb, (uint32_t)(b * V + i)) : 0ull;
  bitonic_desc(s, DEC_SELECT_ROW);
  for (int i = threadIdx.x; i < kr; i += 256) cand[(size_t)row * kr + i] = s[i];
}

// per state: workgroup a sorts the state's n = nb * kr candidates and writes its k winners
__global__ __launch_bounds__(1024) void beam_merge_kernel(const uint64_t* __restrict__ cand, int n, int V, int k,
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

// ---- sampling ---------------------------------------------------------------------------------------------------------
// The sampler's random number (include/reprover_hip.h, rp_sample_uniform): a counter-based hash of (the state's seed, the
// sample's index inside its state, the position t), drop_hash's form with the seed finalised first so that neighbouring
// seeds give unrelated streams.  Nothing else enters: not the row's slot in the launch, not the other states.
constexpr uint32_t SAMPLE_SITE = 0x53414D50u;
__host__ __device__ __forceinline__ float sample_uniform(uint32_t seed, uint32_t sample, uint32_t position) {
  const uint32_t h = fmix32(fmix32(seed ^ SAMPLE_SITE) + sample * 0x85EBCA77u + position * 0x27D4EB2Fu);
  return (float)(h >> 8) * 0x1p-24f;
}

// Inclusive prefix sums of a[0, 512) in place by 256 threads, in an order fixed by the index alone: thread i sums its pair
// (2 i, 2 i + 1), a Hillis-Steele scan runs over the wave's 64 pair sums, the four wave totals are added in index order.
// The caller has published a[]; the sums are published on return.
__device__ __forceinline__ void block_scan512(float* a, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float x0 = a[2 * tid], x1 = x0 + a[2 * tid + 1];
  float v = x1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  float before = __shfl_up(v, 1, 64);
  if (lane == 0) before = 0.f;
  if (lane == 63) red[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) before += red[w];
  a[2 * tid] = before + x0;
  a[2 * tid + 1] = before + x1;
  __syncthreads();
}

// One sampled token per row (row = slot * nb + sample) and the row's bookkeeping; one workgroup per row, vocab <= 512.
// HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial with a stated order:
//   s[v] = logprobs[v] / temperature, sorted descending with ties to the lower id (one bitonic sort serves both filters);
//   top-k keeps s[v] >= the k-th largest (ties with it stay);
//   top-p drops sorted position j > 0 when its tail mass sum_{i >= j} e_i <= drop_mass * sum_i e_i (e = exp(s - max) over
//     what top-k kept; drop_mass = 1 - top_p; read from the far end this is HF's ascending cumulative sum, equal
//     probabilities in descending id order);
//   the draw walks the kept ids in ascending order: the smallest v of non-zero mass with C(v) > u Z (C = the inclusive
//     prefix sum of e, Z its last value), else the last kept id of non-zero mass.
// State arrays are indexed by (state, sample): a finished row writes pad and changes nothing else.
// The row's position t = slots.pos[slot] (rp_sample_step: one t for every slot; rp_sample_pool_step: one per slot).
// params (rp_sample_step_rows / rp_sample_pool_step_rows; null: the three by-value parameters, for every row) is the
// table int32 [n, nb, 4] by (state, sample) of {temperature's bits, top_k, top_p's bits, 0}: the row's workgroup loads its
// own 16 bytes once, every thread the same address, so the values - and the top-p branch with its barriers - are uniform
// over the workgroup.  drop_mass is then the host's expression evaluated here, and the division below the same fp32
// division: a row whose block holds (T, k, p) draws the bits of the by-value call with (T, k, p).  A block outside the
// domain (the ABI cannot look into device memory) reaches no address outside the buffers: top_k indexes keys[] only
// inside 0 < top_k < V <= 512, temperature and drop_mass enter arithmetic alone, and the token is clamped to [0, V).
__global__ __launch_bounds__(256) void sample_step_kernel(const float* __restrict__ lp, int V, int nb, DecSlots slots,
                                                          const uint32_t* __restrict__ seeds, int max_len,
                                                          float temperature, int top_k, float drop_mass,
                                                          const int4* __restrict__ params, int eos, int pad,
                                                          int32_t* __restrict__ seq, int32_t* __restrict__ tokens_next,
                                                          float* __restrict__ cum, int32_t* __restrict__ ngen,
                                                          int32_t* __restrict__ finished) {
  __shared__ uint64_t keys[DEC_SELECT_ROW];
  __shared__ float sc[DEC_SELECT_ROW];  // tail masses by reversed sorted position, then masses / prefix sums by id
  __shared__ float red[4];
  __shared__ int s_first[4], s_last[4];
  const int tid = threadIdx.x, row = blockIdx.x, slot = row / nb, b = row - slot * nb;
  const int state = slots.state[slot], t = slots.pos[slot];
  const size_t idx = (size_t)state * nb + b;
  int32_t* next = seq + idx * max_len + min(t + 1, max_len - 1);
  if (finished[idx]) {  // the same value for the whole workgroup
    if (tid == 0) {
      *next = pad;
      tokens_next[row] = pad;
    }
    return;
  }
  if (params) {  // a kernel argument: the same for the whole grid
    const int4 own = params[idx];
    temperature = __int_as_float(own.x);
    top_k = own.y;
    drop_mass = (float)(1.0 - (double)__int_as_float(own.z));
  }
  const float* r = lp + (size_t)row * V;
  for (int i = tid; i < DEC_SELECT_ROW; i += 256) keys[i] = (i < V) ? sel_key(r[i] / temperature, (uint32_t)i) : 0ull;
  bitonic_desc(keys, DEC_SELECT_ROW);  // the V keys of the row (all non-zero) come first
  const float mx = key_score(keys[0]);
  // top-k on the keys' order-preserving high words (s[v] >= the k-th largest); off: the row's smallest, all stay
  const uint32_t thr = (uint32_t)(keys[(top_k > 0 && top_k < V) ? top_k - 1 : V - 1] >> 32);
  float e[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = tid + 256 * c;
    const float sj = key_score(keys[j]);
    e[c] = (j < V && (uint32_t)(keys[j] >> 32) >= thr) ? expf(sj - mx) : 0.f;
  }
  if (drop_mass > 0.f) {
    sc[DEC_SELECT_ROW - 1 - tid] = e[0];
    sc[DEC_SELECT_ROW - 1 - (tid + 256)] = e[1];
    __syncthreads();
    block_scan512(sc, red);
    const float cut = drop_mass * sc[DEC_SELECT_ROW - 1];
    const float t0 = sc[DEC_SELECT_ROW - 1 - tid], t1 = sc[DEC_SELECT_ROW - 1 - (tid + 256)];
    if (tid > 0 && t0 <= cut) e[0] = 0.f;  // sorted position 0, the most probable token, always stays
    if (t1 <= cut) e[1] = 0.f;
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = tid + 256 * c;
    if (j < V) sc[min(~(uint32_t)keys[j], (uint32_t)(V - 1))] = e[c];  // the ids of positions [0, V) are 0 .. V - 1
    else sc[j] = 0.f;
  }
  __syncthreads();
  const float w0 = sc[2 * tid], w1 = sc[2 * tid + 1];
  block_scan512(sc, red);
  const float target = sample_uniform(seeds[state], (uint32_t)b, (uint32_t)t) * sc[DEC_SELECT_ROW - 1];
  // the smallest id whose prefix sum passes the target, and the largest id of non-zero mass (its stand-in when rounding
  // leaves none): wave butterflies, then the four waves
  int first = DEC_SELECT_ROW, last = -1;
  if (w1 > 0.f) {
    last = 2 * tid + 1;
    if (sc[2 * tid + 1] > target) first = 2 * tid + 1;
  }
  if (w0 > 0.f) {
    last = max(last, 2 * tid);
    if (sc[2 * tid] > target) first = 2 * tid;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if ((tid & 63) == 0) {
    s_first[tid >> 6] = first;
    s_last[tid >> 6] = last;
  }
  __syncthreads();
  if (tid == 0) {
    first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
    last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
    int tok = first < DEC_SELECT_ROW ? first : last;
    if (tok < 0) tok = (int)~(uint32_t)keys[0];  // no mass anywhere (NaN rows, outside the contract): the first key's id
    tok = min(max(tok, 0), V - 1);
    *next = tok;
    tokens_next[row] = tok;
    cum[idx] += r[tok];  // the model's log-prob: untempered, unfiltered
    ngen[idx] += 1;
    if (tok == eos) finished[idx] = 1;
  }
}

// The sampler's books for a slot's next tenant (rp_sample_pool_admit): the states listed in slots.state[0 .. gridDim.x),
// one workgroup each, their seeds by value.  Every seq row of the state over all ld columns (the previous tenant wrote
// them), its scores, counts and flags, its seed; nothing of another state.  The tenant's live rows travel the same way
// (rp_sample_pool_admit_rows; rp_sample_pool_admit: nb for every state): rows b >= n_live start finished, so the step
// writes pad for them and nothing else, and their n_generated stays 0.
struct SampleSeeds {
  uint32_t seed[DEC_MAX_STATES];
};
struct SampleLive {
  int32_t n_live[DEC_MAX_STATES];
};

__global__ __launch_bounds__(256) void sample_admit_kernel(DecSlots slots, SampleSeeds fresh, SampleLive live, int nb, int ld,
                                                           int start, int pad, uint32_t* __restrict__ seeds,
                                                           int32_t* __restrict__ seq, float* __restrict__ cum,
                                                           int32_t* __restrict__ ngen, int32_t* __restrict__ finished) {
  const int tid = threadIdx.x, state = slots.state[blockIdx.x], n_live = live.n_live[blockIdx.x];
  for (int r = 0; r < nb; ++r) {
    int32_t* row = seq + ((size_t)state * nb + r) * ld;
    for (int c = tid; c < ld; c += 256) row[c] = c == 0 ? start : pad;
  }
  for (int r = tid; r < nb; r += 256) {
    const size_t at = (size_t)state * nb + r;
    cum[at] = 0.f;
    ngen[at] = 0;
    finished[at] = r >= n_live;
  }
  if (tid == 0) seeds[state] = fresh.seed[blockIdx.x];
}

// The next step's tokens of slot blockIdx.x, by row, from its state's seq: column slots.pos[slot] (rp_sample_pool_rows).
__global__ __launch_bounds__(64) void sample_rows_kernel(DecSlots slots, int nb, int ld, const int32_t* __restrict__ seq,
                                                         int32_t* __restrict__ tokens_next) {
  const int slot = blockIdx.x, state = slots.state[slot], t = slots.pos[slot];
  for (int r = threadIdx.x; r < nb; r += 64)
    tokens_next[(size_t)slot * nb + r] = seq[((size_t)state * nb + r) * ld + t];
}

// ---- beam books: beam search's bookkeeping on the device ------------------------------------------------------------------
// What generation.py's _BeamState keeps on the host, for n states, in one caller-owned block (include/reprover_hip.h,
// rp_beam_books_bytes).  Every part starts at a multiple of 16 bytes; the row tables have max_len int32 per row.  The
// three row tables are pairs: the step at position t reads pair member t & 1 and writes the other, so no row is gathered
// in place.  Columns a step has not reached hold their initial value in both members (eos / the identity entry).
struct BeamBooks {
  size_t bytes;
  int32_t *run_seq, *anc, *fin_seq;  // [2][n][nb][max_len]: running sequences, their ancestry rows, finished hypotheses
  float *run_scores, *beam_scores;   // [n][nb]
  int32_t *fin_flag, *fin_len;       // [n][nb]: is_sent_finished, generated tokens (beam_indices' non-negative count)
  int32_t *heur, *done, *steps;      // [n]: heuristic_unsatisfied, stopped, advances taken
  int32_t* tokens;                   // [n * nb] by row (slot * nb + b): the next step's tokens
  float* running;                    // [n * nb] by row: rp_beam_select_batch's running scores
  int32_t* anc_rows;                 // [n * nb][max_len] by row: the next step's ancestry table
};

BeamBooks books_carve(char* base, int n, int nb, int max_len) {
  BeamBooks b = {};
  size_t off = 0;
  auto take = [&](size_t words) {
    char* p = base ? base + off : nullptr;
    off += (words * 4 + 15) & ~(size_t)15;
    return p;
  };
  const size_t rows = (size_t)n * nb, table = rows * max_len;
  b.run_seq = (int32_t*)take(2 * table);
  b.anc = (int32_t*)take(2 * table);
  b.fin_seq = (int32_t*)take(2 * table);
  b.run_scores = (float*)take(rows);
  b.beam_scores = (float*)take(rows);
  b.fin_flag = (int32_t*)take(rows);
  b.fin_len = (int32_t*)take(rows);
  b.heur = (int32_t*)take(n);
  b.done = (int32_t*)take(n);
  b.steps = (int32_t*)take(n);
  b.tokens = (int32_t*)take(rows);
  b.running = (float*)take(rows);
  b.anc_rows = (int32_t*)take(table);
  b.bytes = off;
  return b;
}

constexpr float BEAM_NEG = -1.0e9f;  // generation.py's NEG (exact in fp32)

// _BeamState.__init__ for one state, by one workgroup: every by-state part over all ld columns, both pair members.  ROWS:
// the by-row inputs of slot = state as well (rp_beam_books_init: the first step's active list is 0 .. n - 1); without it
// nothing by row and nothing of another state is touched (rp_beam_books_admit: a slot's next tenant).
template <bool ROWS>
__device__ __forceinline__ void beam_state_init(const BeamBooks& bk, int n, int nb, int ld, int state, int eos, int start) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nb * ld; i += 256) {
    const int r = i / ld, c = i - r * ld;
    const int tok = c == 0 ? start : eos, id = c * nb + r;
    for (int buf = 0; buf < 2; ++buf) {
      const size_t at = ((size_t)(buf * n + state) * nb) * ld + i;
      bk.run_seq[at] = tok;
      bk.fin_seq[at] = tok;
      bk.anc[at] = id;
    }
    if (ROWS) bk.anc_rows[(size_t)state * nb * ld + i] = id;
  }
  for (int r = tid; r < nb; r += 256) {
    const size_t at = (size_t)state * nb + r;
    const float run = r == 0 ? 0.f : BEAM_NEG;
    bk.run_scores[at] = run;
    bk.beam_scores[at] = BEAM_NEG;
    bk.fin_flag[at] = 0;
    bk.fin_len[at] = 0;
    if (ROWS) {
      bk.running[at] = run;
      bk.tokens[at] = start;
    }
  }
  if (tid == 0) {
    bk.heur[state] = 1;
    bk.done[state] = 0;
    bk.steps[state] = 0;
  }
}

__global__ __launch_bounds__(256) void beam_books_init_kernel(BeamBooks bk, int n, int nb, int ld, int eos, int start) {
  beam_state_init<true>(bk, n, nb, ld, blockIdx.x, eos, start);
}

// the states listed in slots.state[0 .. gridDim.x), one workgroup each
__global__ __launch_bounds__(256) void beam_books_admit_kernel(BeamBooks bk, int n, int nb, int ld, DecSlots slots, int eos,
                                                               int start) {
  beam_state_init<false>(bk, n, nb, ld, slots.state[blockIdx.x], eos, start);
}

// W int32 moved as one access (W = 4: 16 bytes, rows of a multiple of 4 columns)
template <int W>
struct alignas(4 * W) BookPack {
  int32_t x[W];
};
template <int W>
__device__ __forceinline__ BookPack<W> book_patch(BookPack<W> p, int v, int col, int value) {
#pragma unroll
  for (int e = 0; e < W; ++e)
    if (v * W + e == col) p.x[e] = value;
  return p;
}

// The three row gathers of one advance, in units of W columns: columns 0 .. t come from the source rows, column t + 1 is
// the step's own (the candidate's token; the cache row (t + 1) * nb + r).  With W = 4 the last unit may carry up to three
// columns past t + 1: they hold their initial values in source and destination alike.
template <int W>
__device__ __forceinline__ void beam_gather(const BeamBooks& bk, size_t src, size_t dst, size_t row0, int nb, int ld, int t,
                                            const int* s_tok, const int* s_par, const int* s_nxt, const int* s_sel) {
  typedef BookPack<W> P;
  const int nv = (t + 2 + W - 1) / W, ldv = ld / W;
  const P* run_s = reinterpret_cast<const P*>(bk.run_seq + src);
  const P* anc_s = reinterpret_cast<const P*>(bk.anc + src);
  const P* fin_s = reinterpret_cast<const P*>(bk.fin_seq + src);
  P* run_d = reinterpret_cast<P*>(bk.run_seq + dst);
  P* anc_d = reinterpret_cast<P*>(bk.anc + dst);
  P* fin_d = reinterpret_cast<P*>(bk.fin_seq + dst);
  P* rows_d = reinterpret_cast<P*>(bk.anc_rows + row0);
  for (int i = threadIdx.x; i < nb * nv; i += 256) {
    const int r = i / nv, v = i - r * nv;
    const int c = s_nxt[r], p = s_par[c];
    run_d[(size_t)r * ldv + v] = book_patch<W>(run_s[(size_t)p * ldv + v], v, t + 1, s_tok[c]);
    const P a = book_patch<W>(anc_s[(size_t)p * ldv + v], v, t + 1, (t + 1) * nb + r);
    anc_d[(size_t)r * ldv + v] = a;
    rows_d[(size_t)r * ldv + v] = a;
    const int m = s_sel[r];  // < nb: a kept hypothesis; else candidate m - nb
    fin_d[(size_t)r * ldv + v] = m < nb ? fin_s[(size_t)m * ldv + v]
                                        : book_patch<W>(run_s[(size_t)s_par[m - nb] * ldv + v], v, t + 1, s_tok[m - nb]);
  }
}

// _BeamState.advance for the state in slot blockIdx.x, from the step's 2 nb selected triples (generation.py:92-130; the
// numbered comments are include/reprover_hip.h's).  fp32, one rounding per operation, the reference's order.  Both
// selections rank by counting in rp_beam_select's total order: descending, equal scores (-0.0 == +0.0) to the lower index.
// The slot's position t = slots.pos[slot] and its two divisors travel by value (rp_beam_advance: one t for every slot).
struct BeamDivs {
  float fin[DEC_MAX_STATES], run[DEC_MAX_STATES];
};

__global__ __launch_bounds__(256) void beam_advance_kernel(BeamBooks bk, int n, int nb, int ld, DecSlots slots, BeamDivs divs,
                                                           const float* __restrict__ scores,
                                                           const int32_t* __restrict__ tokens,
                                                           const int32_t* __restrict__ parents, int eos) {
  __shared__ float s_run[2 * DEC_MAX_BEAMS], s_m[3 * DEC_MAX_BEAMS], s_score[DEC_MAX_BEAMS];
  __shared__ int s_tok[2 * DEC_MAX_BEAMS], s_par[2 * DEC_MAX_BEAMS], s_hit[2 * DEC_MAX_BEAMS];
  __shared__ int s_nxt[DEC_MAX_BEAMS], s_sel[DEC_MAX_BEAMS], s_kflag[DEC_MAX_BEAMS], s_klen[DEC_MAX_BEAMS];
  __shared__ int s_flag[DEC_MAX_BEAMS], s_frozen;
  const int tid = threadIdx.x, slot = blockIdx.x, state = slots.state[slot], t = slots.pos[slot], K = 2 * nb;
  const float fin_div = divs.fin[slot], run_div = divs.run[slot];
  const size_t srow = (size_t)state * nb;
  if (tid == 0) s_frozen = bk.done[state];
  __syncthreads();
  if (s_frozen) return;  // 6. a stopped state takes nothing more (one value for the whole workgroup)
  if (tid < K) {
    const float val = scores[(size_t)slot * K + tid];
    const int tok = tokens[(size_t)slot * K + tid];
    const int hit = tok == eos || t + 2 >= ld;                             // 1.
    s_tok[tid] = tok;
    s_par[tid] = min(max(parents[(size_t)slot * K + tid], 0), nb - 1);     // (in range by contract)
    s_hit[tid] = hit;
    s_run[tid] = __fadd_rn(val, hit ? BEAM_NEG : -0.0f);
    float fin = __fdiv_rn(val, fin_div);                                   // 3.
    fin = __fadd_rn(fin, bk.heur[state] ? 0.0f : BEAM_NEG);
    fin = __fadd_rn(fin, (hit && tid < nb) ? -0.0f : BEAM_NEG);
    s_m[nb + tid] = fin;
  }
  if (tid < nb) {
    s_m[tid] = bk.beam_scores[srow + tid];
    s_kflag[tid] = bk.fin_flag[srow + tid];
    s_klen[tid] = bk.fin_len[srow + tid];
  }
  __syncthreads();
  if (tid < K) {  // 2. the next running beams: the candidates of rank < nb
    const float x = s_run[tid];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += (s_run[j] > x || (s_run[j] == x && j < tid)) ? 1 : 0;
    if (rank < nb) s_nxt[rank] = tid;
  }
  if (tid < 3 * nb) {  // 3. the kept hypotheses first, then the candidates: rank < nb stays
    const float x = s_m[tid];
    int rank = 0;
    for (int j = 0; j < 3 * nb; ++j) rank += (s_m[j] > x || (s_m[j] == x && j < tid)) ? 1 : 0;
    if (rank < nb) s_sel[rank] = tid;
  }
  __syncthreads();
  const int cur = t & 1;
  const size_t src = ((size_t)(cur * n + state) * nb) * ld, dst = ((size_t)((cur ^ 1) * n + state) * nb) * ld;
  if (ld % 4 == 0)
    beam_gather<4>(bk, src, dst, (size_t)slot * nb * ld, nb, ld, t, s_tok, s_par, s_nxt, s_sel);
  else
    beam_gather<1>(bk, src, dst, (size_t)slot * nb * ld, nb, ld, t, s_tok, s_par, s_nxt, s_sel);
  if (tid < nb) {
    const int c = s_nxt[tid], m = s_sel[tid];
    bk.run_scores[srow + tid] = s_run[c];
    bk.tokens[(size_t)slot * nb + tid] = s_tok[c];  // 5. the next step's inputs, by row
    bk.running[(size_t)slot * nb + tid] = s_run[c];
    const int flag = m < nb ? s_kflag[m] : (s_hit[m - nb] && m - nb < nb);
    s_score[tid] = s_m[m];
    s_flag[tid] = flag;
    bk.beam_scores[srow + tid] = s_m[m];
    bk.fin_flag[srow + tid] = flag;
    bk.fin_len[srow + tid] = m < nb ? s_klen[m] : t + 1;
  }
  __syncthreads();
  if (tid == 0) {  // 4.
    const float best = __fdiv_rn(s_run[s_nxt[0]], run_div);
    float worst = s_score[0];
    for (int r = 1; r < nb; ++r) worst = fminf(worst, s_score[r]);
    int any = 0, all = 1;
    for (int r = 0; r < nb; ++r) any |= best > (s_flag[r] ? worst : BEAM_NEG);
    for (int j = 0; j < K; ++j) all &= s_hit[j];
    const int heur = bk.heur[state] && any;
    bk.heur[state] = heur;
    bk.done[state] = !heur || all;
    bk.steps[state] = t + 1;
  }
}

// The by-row inputs of slot blockIdx.x from the by-state parts of its state: the state's current pair member
// (slots.pos[slot] & 1), the whole ancestry row, the token in column pos.  By-state and by-row parts are disjoint.
__global__ __launch_bounds__(256) void beam_books_rows_kernel(BeamBooks bk, int n, int nb, int ld, DecSlots slots) {
  const int tid = threadIdx.x, slot = blockIdx.x, state = slots.state[slot], t = slots.pos[slot];
  const size_t src = ((size_t)((t & 1) * n + state) * nb) * ld, dst = (size_t)slot * nb * ld;
  if (ld % 4 == 0) {
    typedef BookPack<4> P;
    const P* a = reinterpret_cast<const P*>(bk.anc + src);
    P* d = reinterpret_cast<P*>(bk.anc_rows + dst);
    for (int i = tid; i < nb * (ld / 4); i += 256) d[i] = a[i];
  } else {
    for (int i = tid; i < nb * ld; i += 256) bk.anc_rows[dst + i] = bk.anc[src + i];
  }
  for (int r = tid; r < nb; r += 256) {
    bk.tokens[(size_t)slot * nb + r] = bk.run_seq[src + (size_t)r * ld + t];
    bk.running[(size_t)slot * nb + r] = bk.run_scores[(size_t)state * nb + r];
  }
}

// ---- rp_decoder_load_params: every resident copy refreshed from one flat fp32 buffer -------------------------------------
// One table entry per (source tensor, resident copy): n source elements at params + src go to dst (and, for RL_BF16_IL,
// row-permuted to dst2 as well).  The table is cut into chunks of RL_CHUNK elements, chunk0 = the entry's first chunk; a
// workgroup finds the entry of its chunk by a binary search over chunk0, so small and large tensors share one grid evenly
// and no entry depends on another (each reads the fp32 master and rounds each element once).
enum { RL_F32 = 0, RL_BF16 = 1, RL_BF16_IL = 2, RL_BIAS = 3 };
constexpr int RL_CHUNK = 8192;      // elements: 256 threads x 4 rounds x 8 elements (32 B read, 16 B written per thread)
constexpr int RL_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the rest is grid-strided
struct DecReloadEntry {
  int64_t src;   // element offset into params (a multiple of 64)
  int64_t n;     // elements; a multiple of 8 except for RL_BIAS (dst elements: H * nbias)
  void* dst;
  void* dst2;    // RL_BF16_IL: wi_il's layer base
  int32_t chunk0, kind;
  int32_t cols;  // RL_BF16_IL: d_model; RL_BIAS: nbias
  int32_t aux;   // RL_BF16_IL: 0 (wi_0: the gate rows) or 32 (wi_1: the up rows); RL_BIAS: H
};

__global__ __launch_bounds__(256) void dec_reload_kernel(const DecReloadEntry* __restrict__ tab, int n_entries, int n_chunks,
                                                         const float* __restrict__ params,
                                                         const int32_t* __restrict__ bucket) {
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    int lo = 0, hi = n_entries - 1;  // the last entry with chunk0 <= ch (block-uniform)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].chunk0 <= ch) lo = mid;
      else hi = mid - 1;
    }
    const DecReloadEntry e = tab[lo];
    const int64_t base = (int64_t)(ch - e.chunk0) * RL_CHUNK;
    const float* __restrict__ src = params + e.src;
    if (e.kind == RL_BIAS) {  // dst[h, j] = rel_bias[bucket[j], h]: a gather, no arithmetic
      const int64_t end = base + RL_CHUNK < e.n ? base + RL_CHUNK : e.n;
      for (int64_t i = base + threadIdx.x; i < end; i += 256) {
        const int h = (int)(i / e.cols), j = (int)(i - (int64_t)h * e.cols);
        reinterpret_cast<float*>(e.dst)[i] = src[(int64_t)bucket[j] * e.aux + h];
      }
      continue;
    }
#pragma unroll
    for (int it = 0; it < RL_CHUNK / 2048; ++it) {
      const int64_t i = base + (int64_t)(it * 256 + threadIdx.x) * 8;
      if (i >= e.n) break;
      const float4 a = *reinterpret_cast<const float4*>(src + i), b = *reinterpret_cast<const float4*>(src + i + 4);
      if (e.kind == RL_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(e.dst) + i) = a;
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(e.dst) + i + 4) = b;
        continue;
      }
      const uint4 v = make_uint4(pack_bf2(a.x, a.y), pack_bf2(a.z, a.w), pack_bf2(b.x, b.y), pack_bf2(b.z, b.w));
      *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(e.dst) + i) = v;
      if (e.kind == RL_BF16_IL) {  // dec_interleave_kernel's row map, from the source side (cols % 8 == 0: one row)
        const int64_t r = i / e.cols, c = i - r * e.cols;
        const int64_t row = (r >> 5) * 64 + (r & 31) + e.aux;
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(e.dst2) + row * e.cols + c) = v;
      }
    }
  }
}

struct DecWs {
  bf16_t* ckv;    // [sum S, L * 2 * inner]
  bf16_t* cache;  // [n][L][max_len * nb, 2 * inner]
  float* x;       // [n * nb, D]
  bf16_t* h;      // [n * nb, D] then [n * nb, F]
  bf16_t* qkv;    // [n * nb, 3 * inner]
  bf16_t* att;    // [n * nb, inner]
  size_t bytes;
};
DecWs dec_carve(const RpDecoder* d, int n, int total_src, int nb, int max_len, char* base) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, L = d->cfg.num_layers, M = (size_t)n * nb;
  DecWs w;
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

// the descriptor table of rp_decoder_load_params and the bias table's bucket index, made once (dec_pack has run)
RpStatus dec_reload_table(RpDecoder* d) {
  const RpT5Config& c = d->cfg;
  const int64_t D = c.d_model, F = c.d_ff, ID = (int64_t)d->inner * D, V = c.vocab_size;
  const int L = c.num_layers, H = c.num_heads;
  std::vector<int64_t> off((size_t)rp_decoder_grad_tensors(d) + 1);
  RpStatus st = rp_decoder_grad_layout(d, off.data());
  if (st) return st;
  std::vector<DecReloadEntry> tab;
  int64_t chunks = 0;
  auto add = [&](int kind, int64_t src, int64_t n, void* dst, void* dst2 = nullptr, int cols = 0, int aux = 0) {
    tab.push_back(DecReloadEntry{src, n, dst, dst2, (int32_t)chunks, kind, cols, aux});
    chunks += (n + RL_CHUNK - 1) / RL_CHUNK;
  };
  int t = 0;  // the layout's tensor index, in rp_decoder_grad_layout's order
  add(RL_F32, off[t], V * D, d->embed);
  if (d->tied) add(RL_BF16, off[t], V * D, d->lm_head);
  ++t;
  if (!d->tied) add(RL_BF16, off[t++], V * D, d->lm_head);
  add(RL_BIAS, off[t++], (int64_t)H * d->nbias, d->bias_tab, nullptr, d->nbias, H);
  add(RL_F32, off[t++], D, d->final_ln);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    bf16_t* ckv = d->cross_kv_w + (size_t)2 * i * ID;
    bf16_t* il = d->wi_il ? d->wi_il + (size_t)i * 2 * F * D : nullptr;
    const int wi_kind = il ? RL_BF16_IL : RL_BF16;
    add(RL_F32, off[t++], D, l.ln_self);
    add(RL_BF16, off[t++], ID, l.wqkv);
    add(RL_BF16, off[t++], ID, l.wqkv + ID);
    add(RL_BF16, off[t++], ID, l.wqkv + 2 * ID);
    add(RL_BF16, off[t++], ID, l.wo);
    add(RL_F32, off[t++], D, l.ln_cross);
    add(RL_BF16, off[t++], ID, l.cq);
    add(RL_BF16, off[t++], ID, ckv);
    add(RL_BF16, off[t++], ID, ckv + ID);
    add(RL_BF16, off[t++], ID, l.co);
    add(RL_F32, off[t++], D, l.ln_ff);
    add(wi_kind, off[t++], F * D, l.wi, il, (int)D, 0);
    add(wi_kind, off[t++], F * D, l.wi + F * D, il, (int)D, 32);
    add(RL_BF16, off[t++], F * D, l.wo2);
  }
  if (t + 1 != (int)off.size() || chunks > INT32_MAX) return fail(RP_E_INVALID, "decoder reload table: %d tensors", t);
  for (const DecReloadEntry& e : tab)  // the vector path moves 8 elements at a time (d_model and d_ff are multiples of 8)
    if (e.kind != RL_BIAS && (e.n % 8 || e.src % 8)) return fail(RP_E_UNSUPPORTED, "decoder reload: tensor of %lld elements", (long long)e.n);
  std::vector<int32_t> bk((size_t)d->nbias);
  for (int j = 0; j < d->nbias; ++j) bk[j] = rp_relative_position_bucket_causal(-j, c.rel_num_buckets, c.rel_max_distance);
  RP_HIP(hipMalloc((void**)&d->bias_bucket, bk.size() * 4));
  d->allocs.push_back(d->bias_bucket);
  RP_HIP(hipMalloc(&d->reload_tab, tab.size() * sizeof(DecReloadEntry)));
  d->allocs.push_back(d->reload_tab);
  RP_HIP(hipMemcpy(d->bias_bucket, bk.data(), bk.size() * 4, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d->reload_tab, tab.data(), tab.size() * sizeof(DecReloadEntry), hipMemcpyHostToDevice));
  d->reload_entries = (int)tab.size();
  d->reload_chunks = (int)chunks;
  return RP_OK;
}

// The ids a call lists: n of them, each in [0, bound), none named twice (bound <= DEC_MAX_STATES: a 32-bit mask).  `list`
// is the argument's name in the messages and `what` the thing an id names ("state" or "slot").  each(index, id) checks
// what else the caller keeps per entry and fills its by-value table; its refusal ends the walk.
template <typename Each>
RpStatus dec_list(const int32_t* ids, int n, int bound, const char* list, const char* what, Each each) {
  uint32_t seen = 0;
  for (int a = 0; a < n; ++a) {
    const int id = ids[a];
    RP_REQUIRE(id >= 0 && id < bound, "%s[%d]=%d outside [0, %ss=%d)", list, a, id, what, bound);
    RP_REQUIRE(!(seen & (1u << id)), "%s[%d]=%d names a %s twice", list, a, id, what);  // two entries would share rows
    seen |= 1u << id;
    if (RpStatus st = each(a, id)) return st;
  }
  return RP_OK;
}

// Where the states of a workspace live: n caches and a cross K/V of total_src rows, state s's source in rows
// [off[s], off[s] + len[s]).  dec_check fills it from src_cu, pool_check with every slot's region src_cap rows long (the
// pool's calls say how much of a region is in use).
struct DecGeom {
  int n, total_src;
  int32_t off[DEC_MAX_STATES], len[DEC_MAX_STATES];
};

// the caps of a call over packed sources
RpStatus dec_check(const RpDecoder* d, const int32_t* src_cu, int n, int nb, int max_len, DecGeom& g) {
  RP_REQUIRE(d, "null decoder");
  RP_REQUIRE(src_cu, "null src_cu");
  RP_REQUIRE(n >= 1 && n <= DEC_MAX_STATES, "states=%d (1..%d)", n, DEC_MAX_STATES);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "num_beams=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n * nb <= DEC_MAX_ROWS, "rows = states * num_beams = %d > %d", n * nb, DEC_MAX_ROWS);
  RP_REQUIRE(max_len >= 1 && max_len <= DEC_MAX_KEYS, "max_len=%d (1..%d)", max_len, DEC_MAX_KEYS);
  RP_REQUIRE(src_cu[0] == 0, "src_cu[0]=%d, not 0", src_cu[0]);
  for (int b = 0; b < n; ++b) {
    const int64_t S = (int64_t)src_cu[b + 1] - src_cu[b];
    RP_REQUIRE(S >= 1 && S <= DEC_MAX_KEYS, "src_len of state %d = %lld (1..%d)", b, (long long)S, DEC_MAX_KEYS);
    g.off[b] = src_cu[b];
    g.len[b] = (int32_t)S;
  }
  g.n = n;
  g.total_src = src_cu[n];
  return RP_OK;
}

// the caps of a slot pool: dec_check's, with every slot's source region src_cap rows long
RpStatus pool_check(const RpDecoder* d, int n_slots, int nb, int max_len, int src_cap, DecGeom& g) {
  RP_REQUIRE(d, "null decoder");
  RP_REQUIRE(n_slots >= 1 && n_slots <= DEC_MAX_STATES, "slots=%d (1..%d)", n_slots, DEC_MAX_STATES);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "num_beams=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n_slots * nb <= DEC_MAX_ROWS, "rows = slots * num_beams = %d > %d", n_slots * nb, DEC_MAX_ROWS);
  RP_REQUIRE(max_len >= 1 && max_len <= DEC_MAX_KEYS, "max_len=%d (1..%d)", max_len, DEC_MAX_KEYS);
  RP_REQUIRE(src_cap >= 1 && src_cap <= DEC_MAX_KEYS, "src_cap=%d (1..%d)", src_cap, DEC_MAX_KEYS);
  for (int sl = 0; sl < n_slots; ++sl) {
    g.off[sl] = sl * src_cap;
    g.len[sl] = src_cap;
  }
  g.n = n_slots;
  g.total_src = n_slots * src_cap;
  return RP_OK;
}

// the workspace of a geometry, carved; refused when the caller's is absent or smaller
RpStatus dec_workspace(const RpDecoder* d, const DecGeom& g, int nb, int max_len, void* ws, size_t ws_bytes, DecWs& w) {
  w = dec_carve(d, g.n, g.total_src, nb, max_len, (char*)ws);
  if (!ws || ws_bytes < w.bytes) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, w.bytes);
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
  if (st == RP_OK) st = dec_reload_table(d);
  if (st != RP_OK) {
    rp_decoder_destroy(d);
    return st;
  }
  *out = d;
  return RP_OK;
}

// Refresh every resident copy of the weights (dec_pack's: the fp32 tables, the bf16 operands, the cross K/V
// concatenation, the interleaved FFN-in copy, the expanded bias table) from the fp32 masters in rp_decoder_grad_layout's
// order: one grid-stride launch over the descriptor table.  Launch-only.
extern "C" RpStatus rp_decoder_load_params(RpDecoder* d, const float* params, void* stream_) {
  RP_REQUIRE(d && params, "null argument");
  RP_REQUIRE(((uintptr_t)params & 15) == 0, "params is not 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope ps(stream, RP_K_OPTIMIZER);
  hipLaunchKernelGGL(dec_reload_kernel, dim3(std::min(d->reload_chunks, RL_MAX_BLOCKS)), dim3(256), 0, stream,
                     (const DecReloadEntry*)d->reload_tab, d->reload_entries, d->reload_chunks, params,
                     (const int32_t*)d->bias_bucket);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" void rp_decoder_destroy(RpDecoder* d) {
  if (!d) return;
  for (void* p : d->allocs) (void)hipFree(p);
  delete d;
}

extern "C" size_t rp_decoder_batch_workspace_bytes(const RpDecoder* d, const int32_t* src_cu, int32_t n, int32_t nb,
                                                   int32_t max_len) {
  DecGeom g;
  if (dec_check(d, src_cu, n, nb, max_len, g) != RP_OK) return 0;
  return dec_carve(d, g.n, g.total_src, nb, max_len, nullptr).bytes;
}

extern "C" RpStatus rp_decoder_batch_cross_kv(RpDecoder* d, const void* enc, const int32_t* src_cu, int32_t n, int32_t nb,
                                              int32_t max_len, void* ws, size_t ws_bytes, void* stream_) {
  DecGeom g;
  DecWs w;
  RpStatus st = dec_check(d, src_cu, n, nb, max_len, g);
  if (st) return st;
  RP_REQUIRE(enc, "null encoder states");
  if ((st = dec_workspace(d, g, nb, max_len, ws, ws_bytes, w))) return st;
  const int D = d->cfg.d_model, NKV = d->cfg.num_layers * 2 * d->inner;
  return launch_dec_gemm<EPI_BF16>((const bf16_t*)enc, D, g.total_src, d->cross_kv_w, NKV, D, w.ckv, NKV, (hipStream_t)stream_);
}

namespace {
// The launch sequence over the M rows of a row table: a decode step's (DecSlots: rp_decoder_batch_step, every slot at the
// call's t; rp_decoder_batch_step_pos and rp_decoder_pool_step, a position per slot) or a prefill pass's (DecSegs).  Only
// the cache store and the two attentions look at the table; everything else is row-wise.  All rows' K/V are stored before
// the self-attention reads them.  Without `logprobs` (a prefill pass) the last layer ends at its cache store - nothing
// after it reaches the cache - and there is no final norm, lm_head or log_softmax.
template <typename Rows>
RpStatus dec_layers_launch(RpDecoder* d, const DecWs& w, const Rows& table, int M, const int32_t* tokens, const int32_t* anc,
                           int astride, int nb, int max_len, float* logprobs, hipStream_t s) {
  RpStatus st;
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  const int rows = max_len * nb, ldckv = L * 2 * inner;
  const size_t layer_stride = (size_t)rows * 2 * inner, state_stride = (size_t)L * layer_stride;
  bf16_t* ffn = w.h + (size_t)M * D;
  hipLaunchKernelGGL(dec_embed_kernel, dim3(M), dim3(256), 0, s, tokens, d->embed, w.x, D, V);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    bf16_t* cache = w.cache + (size_t)i * layer_stride;  // state 0's rows of layer i
    // self-attention (modeling_t5.py T5LayerSelfAttention): x += o(attn(rmsnorm(x)))
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_self, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_BF16>(w.h, D, M, l.wqkv, 3 * inner, D, w.qkv, 3 * inner, s))) return st;
    hipLaunchKernelGGL(dec_store_kv_kernel<Rows>, dim3(M), dim3(256), 0, s, w.qkv, inner, cache, state_stride, nb, table);
    if (!logprobs && i == L - 1) break;
    launch_dec_self_attention(w.qkv, 3 * inner, cache, 2 * inner, 0, inner, rows, state_stride, anc, astride, d->bias_tab,
                              d->nbias, nb, H, table, M, w.att, inner, s);
    if ((st = launch_dec_gemm<EPI_RESID>(w.att, inner, M, l.wo, D, inner, w.x, D, s))) return st;
    // cross-attention (T5LayerCrossAttention): no position bias, all of the state's source keys
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_cross, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_BF16>(w.h, D, M, l.cq, inner, D, w.qkv, inner, s))) return st;
    launch_dec_cross_attention(w.qkv, inner, w.ckv, ldckv, 2 * i * inner, (2 * i + 1) * inner, nb, H, table, M, w.att, inner,
                               s);
    if ((st = launch_dec_gemm<EPI_RESID>(w.att, inner, M, l.co, D, inner, w.x, D, s))) return st;
    // gated-GELU FFN (T5LayerFF / T5DenseGatedActDense)
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, l.ln_ff, w.h, D, eps, 1.f);
    if ((st = launch_dec_gemm<EPI_GEGLU>(w.h, D, M, l.wi, F, D, ffn, F, s))) return st;
    if ((st = launch_dec_gemm<EPI_RESID>(ffn, F, M, l.wo2, D, F, w.x, D, s))) return st;
  }
  if (logprobs) {
    const float scale = d->tied ? 1.f / sqrtf((float)D) : 1.f;
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(M), dim3(256), 0, s, w.x, d->final_ln, w.h, D, eps, scale);
    if ((st = launch_dec_gemm<EPI_F32>(w.h, D, M, d->lm_head, V, D, logprobs, V, s))) return st;
    hipLaunchKernelGGL(dec_log_softmax_kernel, dim3(M), dim3(256), 0, s, logprobs, V);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// One decode step over a checked geometry: the one routine behind rp_decoder_batch_step (pos null: every listed state at
// t), rp_decoder_batch_step_pos (state active[a] at pos[a]) and rp_decoder_pool_step (src_len[a] rows of slot active[a]'s
// region in use).  `what` is what the list names, "state" or "slot".
RpStatus dec_step(RpDecoder* d, const DecGeom& g, const char* what, const int32_t* active, int n_active, const int32_t* pos,
                  int t, const int32_t* src_len, const int32_t* tokens, const int32_t* anc, int astride, int nb,
                  int max_len, float* logprobs, void* ws, size_t ws_bytes, void* stream_) {
  RP_REQUIRE(n_active >= 1 && n_active <= g.n, "active %ss=%d (1..%ss=%d)", what, n_active, what, g.n);
  if (!pos) {  // all states started together
    RP_REQUIRE(t >= 0 && t < max_len, "t=%d outside [0, max_len=%d)", t, max_len);
    RP_REQUIRE(astride >= t + 1, "anc_stride=%d < t + 1 = %d", astride, t + 1);
  }
  DecSlots slots = {};
  DecWs w;
  RpStatus st = dec_list(active, n_active, g.n, "active", what, [&](int a, int id) -> RpStatus {
    if (pos) {
      RP_REQUIRE(pos[a] >= 0 && pos[a] < max_len, "pos[%d]=%d outside [0, max_len=%d)", a, pos[a], max_len);
      if (src_len) RP_REQUIRE(src_len[a] >= 1 && src_len[a] <= g.len[id], "src_len[%d]=%d (1..src_cap=%d)", a, src_len[a], g.len[id]);
      RP_REQUIRE(astride >= pos[a] + 1, "anc_stride=%d < pos[%d] + 1 = %d", astride, a, pos[a] + 1);
    }
    slots.state[a] = id;
    slots.src_off[a] = g.off[id];
    slots.src_len[a] = src_len ? src_len[a] : g.len[id];
    slots.pos[a] = pos ? pos[a] : t;
    return RP_OK;
  });
  if (st || (st = dec_workspace(d, g, nb, max_len, ws, ws_bytes, w))) return st;
  return dec_layers_launch(d, w, slots, n_active * nb, tokens, anc, astride, nb, max_len, logprobs, (hipStream_t)stream_);
}
}  // namespace

extern "C" RpStatus rp_decoder_batch_step(RpDecoder* d, const int32_t* src_cu, int32_t n, const int32_t* active,
                                          int32_t n_active, const int32_t* tokens, const int32_t* anc, int32_t astride,
                                          int32_t nb, int32_t t, int32_t max_len, float* logprobs, void* ws,
                                          size_t ws_bytes, void* stream_) {
  DecGeom g;
  RpStatus st = dec_check(d, src_cu, n, nb, max_len, g);
  if (st) return st;
  RP_REQUIRE(active && tokens && anc && logprobs, "null argument");
  return dec_step(d, g, "state", active, n_active, nullptr, t, nullptr, tokens, anc, astride, nb, max_len, logprobs, ws,
                  ws_bytes, stream_);
}

// rp_decoder_batch_step with a position per listed state (the lockstep loop over states whose prompts differ in length)
extern "C" RpStatus rp_decoder_batch_step_pos(RpDecoder* d, const int32_t* src_cu, int32_t n, const int32_t* active,
                                              int32_t n_active, const int32_t* tokens, const int32_t* anc, int32_t astride,
                                              int32_t nb, const int32_t* pos, int32_t max_len, float* logprobs, void* ws,
                                              size_t ws_bytes, void* stream_) {
  DecGeom g;
  RpStatus st = dec_check(d, src_cu, n, nb, max_len, g);
  if (st) return st;
  RP_REQUIRE(active && pos && tokens && anc && logprobs, "null argument");
  return dec_step(d, g, "state", active, n_active, pos, 0, nullptr, tokens, anc, astride, nb, max_len, logprobs, ws, ws_bytes,
                  stream_);
}

// ---- the slot pool: states that join a running search between steps ("Continuous batching") ---------
extern "C" size_t rp_decoder_pool_workspace_bytes(const RpDecoder* d, int32_t n_slots, int32_t nb, int32_t max_len,
                                                  int32_t src_cap) {
  DecGeom g;
  if (pool_check(d, n_slots, nb, max_len, src_cap, g) != RP_OK) return 0;
  return dec_carve(d, g.n, g.total_src, nb, max_len, nullptr).bytes;
}

extern "C" RpStatus rp_decoder_pool_admit(RpDecoder* d, int32_t n_slots, int32_t nb, int32_t max_len, int32_t src_cap,
                                          const int32_t* slot_ids, const void* enc, const int32_t* src_cu, int32_t m,
                                          void* ws, size_t ws_bytes, void* stream_) {
  DecGeom g;
  DecWs w;
  RpStatus st = pool_check(d, n_slots, nb, max_len, src_cap, g);
  if (st) return st;
  RP_REQUIRE(slot_ids && enc && src_cu && ws, "null argument");
  RP_REQUIRE(m >= 1 && m <= n_slots, "admitted sources=%d (1..slots=%d)", m, n_slots);
  RP_REQUIRE(src_cu[0] == 0, "src_cu[0]=%d, not 0", src_cu[0]);
  st = dec_list(slot_ids, m, n_slots, "slots", "slot", [&](int j, int) -> RpStatus {
    const int64_t S = (int64_t)src_cu[j + 1] - src_cu[j];
    RP_REQUIRE(S >= 1 && S <= src_cap, "src_len of source %d = %lld (1..src_cap=%d)", j, (long long)S, src_cap);
    return RP_OK;
  });
  if (st || (st = dec_workspace(d, g, nb, max_len, ws, ws_bytes, w))) return st;
  const int D = d->cfg.d_model, NKV = d->cfg.num_layers * 2 * d->inner;
  for (int j = 0; j < m; ++j)  // one GEMM per newcomer, into its slot's region (a row depends on no other row)
    if ((st = launch_dec_gemm<EPI_BF16>((const bf16_t*)enc + (size_t)src_cu[j] * D, D, src_cu[j + 1] - src_cu[j],
                                        d->cross_kv_w, NKV, D, w.ckv + (size_t)g.off[slot_ids[j]] * NKV, NKV,
                                        (hipStream_t)stream_)))
      return st;
  return RP_OK;
}

extern "C" RpStatus rp_decoder_pool_step(RpDecoder* d, int32_t n_slots, int32_t nb, int32_t max_len, int32_t src_cap,
                                         const int32_t* active, const int32_t* pos, const int32_t* src_len,
                                         int32_t n_active, const int32_t* tokens, const int32_t* anc, int32_t astride,
                                         float* logprobs, void* ws, size_t ws_bytes, void* stream_) {
  DecGeom g;
  RpStatus st = pool_check(d, n_slots, nb, max_len, src_cap, g);
  if (st) return st;
  RP_REQUIRE(active && pos && src_len && tokens && anc && logprobs && ws, "null argument");
  return dec_step(d, g, "slot", active, n_active, pos, 0, src_len, tokens, anc, astride, nb, max_len, logprobs, ws, ws_bytes,
                  stream_);
}

// ---- prompt prefill: the prompt rows of the listed states through the layers, all positions in one launch sequence --------
namespace {
struct PrefillState {
  int state, src_off, src_len, rows;
};

// The prompt rows, state after state and position after position (the order of `tokens`), are cut into passes of at most
// `cap` rows - the activation block's - so a state's lower positions are stored, in every layer, before a later pass
// attends over them.  A pass is dec_layers_launch over its segments, without log-probs.
RpStatus dec_prefill_launch(RpDecoder* d, const DecWs& w, const PrefillState* ps, int m, const int32_t* tokens,
                            const int32_t* anc, int nb, int max_len, int cap, hipStream_t s) {
  RpStatus st;
  DecSegs segs = {};
  int used = 0, first = 0, row = 0;
  for (int j = 0; j < m; ++j) {
    int p = 0;
    while (p < ps[j].rows) {
      const int take = std::min(ps[j].rows - p, cap - used);
      const int g = segs.n++;
      segs.state[g] = ps[j].state;
      segs.src_off[g] = ps[j].src_off;
      segs.src_len[g] = ps[j].src_len;
      segs.pos0[g] = p;
      segs.row0[g] = used;
      used += take;
      p += take;
      row += take;
      if (used == cap || (j == m - 1 && p == ps[j].rows)) {
        if ((st = dec_layers_launch(d, w, segs, used, tokens + first, anc, 0, nb, max_len, nullptr, s))) return st;
        first = row;
        used = 0;
        segs = DecSegs{};
      }
    }
  }
  return RP_OK;
}

// The one routine behind rp_decoder_batch_prefill and rp_decoder_pool_prefill (src_len: the rows of each listed slot's
// region in use): prompt_cu[0] = 0, 1 <= R_j, R_j + 1 < max_len, anc_len >= every R_j, then the list.
RpStatus dec_prefill(RpDecoder* d, const DecGeom& g, const char* list, const char* what, const int32_t* ids,
                     const int32_t* src_len, const int32_t* prompt_cu, int m, const int32_t* tokens, const int32_t* anc,
                     int anc_len, int nb, int max_len, void* ws, size_t ws_bytes, void* stream_) {
  RP_REQUIRE(m >= 1 && m <= g.n, "listed %ss=%d (1..%ss=%d)", what, m, what, g.n);
  RP_REQUIRE(prompt_cu[0] == 0, "prompt_cu[0]=%d, not 0", prompt_cu[0]);
  for (int j = 0; j < m; ++j) {
    const int64_t R = (int64_t)prompt_cu[j + 1] - prompt_cu[j];
    RP_REQUIRE(R >= 1, "prompt %d has %lld rows (>= 1)", j, (long long)R);
    RP_REQUIRE(R + 1 < max_len, "prompt %d: %lld rows + 1 >= max_len=%d", j, (long long)R, max_len);
    RP_REQUIRE(anc_len >= R, "anc_len=%d < the %lld rows of prompt %d", anc_len, (long long)R, j);
  }
  PrefillState ps[DEC_MAX_STATES];
  DecWs w;
  RpStatus st = dec_list(ids, m, g.n, list, what, [&](int j, int id) -> RpStatus {
    if (src_len) RP_REQUIRE(src_len[j] >= 1 && src_len[j] <= g.len[id], "src_len[%d]=%d (1..src_cap=%d)", j, src_len[j], g.len[id]);
    ps[j] = PrefillState{id, g.off[id], src_len ? src_len[j] : g.len[id], prompt_cu[j + 1] - prompt_cu[j]};
    return RP_OK;
  });
  if (st || (st = dec_workspace(d, g, nb, max_len, ws, ws_bytes, w))) return st;
  return dec_prefill_launch(d, w, ps, m, tokens, anc, nb, max_len, g.n * nb, (hipStream_t)stream_);
}
}  // namespace

extern "C" RpStatus rp_decoder_batch_prefill(RpDecoder* d, const int32_t* src_cu, int32_t n, const int32_t* states,
                                             const int32_t* prompt_cu, int32_t m, const int32_t* tokens,
                                             const int32_t* anc, int32_t anc_len, int32_t nb, int32_t max_len, void* ws,
                                             size_t ws_bytes, void* stream_) {
  DecGeom g;
  RpStatus st = dec_check(d, src_cu, n, nb, max_len, g);
  if (st) return st;
  RP_REQUIRE(states && prompt_cu && tokens && anc, "null argument");
  return dec_prefill(d, g, "states", "state", states, nullptr, prompt_cu, m, tokens, anc, anc_len, nb, max_len, ws, ws_bytes,
                     stream_);
}

extern "C" RpStatus rp_decoder_pool_prefill(RpDecoder* d, int32_t n_slots, int32_t nb, int32_t max_len, int32_t src_cap,
                                            const int32_t* slot_ids, const int32_t* src_len, const int32_t* prompt_cu,
                                            int32_t m, const int32_t* tokens, const int32_t* anc, int32_t anc_len,
                                            void* ws, size_t ws_bytes, void* stream_) {
  DecGeom g;
  RpStatus st = pool_check(d, n_slots, nb, max_len, src_cap, g);
  if (st) return st;
  RP_REQUIRE(slot_ids && src_len && prompt_cu && tokens && anc && ws, "null argument");
  return dec_prefill(d, g, "slots", "slot", slot_ids, src_len, prompt_cu, m, tokens, anc, anc_len, nb, max_len, ws, ws_bytes,
                     stream_);
}

// ---- the decode step's kernels one at a time (test-only: tests/test_decode_step_kernels_gpu.py) ---------------------------
// Device pointers in, launch-only on the given stream, through the launch code dec_layers_launch runs.
extern "C" RpStatus rp_dbg_dec_gemm(int32_t epi, const void* A, int32_t lda, int32_t M, const void* W, int32_t N, int32_t K,
                                    void* out, int32_t ldo, void* stream_) {
  RP_REQUIRE(A && W && out, "null argument");
  RP_REQUIRE(M >= 1 && N >= 1 && K >= 8 && K % 8 == 0, "M=%d N=%d K=%d (K a multiple of 8)", M, N, K);
  RP_REQUIRE(lda >= K && lda % 8 == 0 && ldo >= N, "lda=%d (>= K, a multiple of 8), ldo=%d (>= N)", lda, ldo);
  RP_REQUIRE((((uintptr_t)A | (uintptr_t)W) & 15) == 0, "A / W not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream_;
  const bf16_t *a = (const bf16_t*)A, *w = (const bf16_t*)W;
  switch (epi) {
    case EPI_BF16: return launch_dec_gemm<EPI_BF16>(a, lda, M, w, N, K, out, ldo, s);
    case EPI_RESID: return launch_dec_gemm<EPI_RESID>(a, lda, M, w, N, K, out, ldo, s);
    case EPI_F32: return launch_dec_gemm<EPI_F32>(a, lda, M, w, N, K, out, ldo, s);
    case EPI_GEGLU: return launch_dec_gemm<EPI_GEGLU>(a, lda, M, w, N, K, out, ldo, s);
    default: return fail(RP_E_INVALID, "epi=%d", epi);
  }
}

namespace {
// a caller-supplied slot table under rp_decoder_pool_step's checks (state / pos are host arrays)
RpStatus dbg_slots(DecSlots& slots, const int32_t* state, const int32_t* pos, int n_active, int n_states, int nb,
                   int max_len) {
  RP_REQUIRE(state && pos, "null slot table");
  RP_REQUIRE(n_states >= 1 && n_states <= DEC_MAX_STATES, "states=%d (1..%d)", n_states, DEC_MAX_STATES);
  RP_REQUIRE(n_active >= 1 && n_active <= n_states, "active slots=%d (1..states=%d)", n_active, n_states);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "num_beams=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n_active * nb <= DEC_MAX_ROWS, "rows = slots * num_beams = %d > %d", n_active * nb, DEC_MAX_ROWS);
  RP_REQUIRE(max_len >= 1 && max_len <= DEC_MAX_KEYS, "max_len=%d (1..%d)", max_len, DEC_MAX_KEYS);
  return dec_list(state, n_active, n_states, "state", "state", [&](int a, int id) -> RpStatus {
    RP_REQUIRE(pos[a] >= 0 && pos[a] < max_len, "pos[%d]=%d outside [0, max_len=%d)", a, pos[a], max_len);
    slots.state[a] = id;
    slots.pos[a] = pos[a];
    return RP_OK;
  });
}
}  // namespace

// The step's row kernels, one per mode (rows = grid size):
//   0 embed        ia = tokens [rows], a = table f32 [vocab, n]; o0 = f32 [rows, n]
//   1 rmsnorm      a = x f32 [rows, n], b = ln f32 [n]; o0 = bf16 [rows, n]; eps, scale
//   2 log_softmax  o0 = f32 [rows, n], in place
//   3 store_kv     a = qkv bf16 [n_active * nb, 3 n] (n = inner); o0 = caches bf16, state s at s * state_stride elements,
//                  max_len * nb rows of 2 n each; the slot table (state, pos: host arrays) as rp_decoder_pool_step checks it
extern "C" RpStatus rp_dbg_dec_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t rows, int32_t n,
                                    int32_t vocab, float eps, float scale, const int32_t* state, const int32_t* pos,
                                    int32_t n_active, int32_t n_states, int32_t nb, int32_t max_len, int64_t state_stride,
                                    void* o0, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  RP_REQUIRE(o0 && n >= 1, "bad argument");
  switch (mode) {
    case 0:
      RP_REQUIRE(a && ia && rows >= 1 && vocab >= 1, "embed: bad argument");
      hipLaunchKernelGGL(dec_embed_kernel, dim3(rows), dim3(256), 0, s, ia, (const float*)a, (float*)o0, n, vocab);
      break;
    case 1:
      RP_REQUIRE(a && b && rows >= 1, "rmsnorm: bad argument");
      hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(rows), dim3(256), 0, s, (const float*)a, (const float*)b, (bf16_t*)o0, n, eps,
                         scale);
      break;
    case 2:
      RP_REQUIRE(rows >= 1, "log_softmax: bad argument");
      hipLaunchKernelGGL(dec_log_softmax_kernel, dim3(rows), dim3(256), 0, s, (float*)o0, n);
      break;
    case 3: {
      DecSlots slots = {};
      RpStatus st = dbg_slots(slots, state, pos, n_active, n_states, nb, max_len);
      if (st) return st;
      RP_REQUIRE(a && state_stride >= (int64_t)max_len * nb * 2 * n, "store_kv: state_stride=%lld < max_len * nb * 2 * inner",
                 (long long)state_stride);
      hipLaunchKernelGGL(dec_store_kv_kernel<DecSlots>, dim3(n_active * nb), dim3(256), 0, s, (const bf16_t*)a, n, (bf16_t*)o0,
                         (size_t)state_stride, nb, slots);
      break;
    }
    default:
      return fail(RP_E_INVALID, "mode=%d", mode);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// The step's self- (cross = 0) or cross-attention launch over a caller-supplied slot table (state, src_off, src_len, pos:
// host arrays of n_active entries), checked as rp_decoder_pool_step checks its own.
//   self:  kv = the caches (state s at s * state_stride elements, `rows` = max_len * nb rows of ldkv), keys 0 .. pos[slot]
//          through anc [n_active * nb, astride] (device), bias tab f32 [H, nbias]
//   cross: kv = the cross K/V of `rows` rows of ldkv; slot a reads rows [src_off[a], src_off[a] + src_len[a]); no bias
// K at column koff + 64 h, V at voff + 64 h; q [n_active * nb, ldq], out [n_active * nb, ldo], head h at column 64 h.
extern "C" RpStatus rp_dbg_dec_attention(int32_t cross, const void* q, int32_t ldq, const void* kv, int32_t ldkv, int32_t koff,
                                         int32_t voff, int32_t rows, int64_t state_stride, int32_t n_states,
                                         const int32_t* anc, int32_t astride, const float* tab, int32_t nbias, int32_t nb,
                                         int32_t H, const int32_t* state, const int32_t* src_off, const int32_t* src_len,
                                         const int32_t* pos, int32_t n_active, int32_t max_len, void* out, int32_t ldo,
                                         void* stream_) {
  RP_REQUIRE(q && kv && out && (!cross || (src_off && src_len)), "null argument");
  RP_REQUIRE(H >= 1 && ldq >= 64 * H && ldo >= 64 * H && ldq % 8 == 0, "H=%d ldq=%d ldo=%d", H, ldq, ldo);
  RP_REQUIRE(ldkv % 8 == 0 && koff >= 0 && koff % 8 == 0 && voff >= 0 && koff + 64 * H <= ldkv && voff + 64 * H <= ldkv,
             "ldkv=%d koff=%d voff=%d", ldkv, koff, voff);
  RP_REQUIRE((((uintptr_t)q | (uintptr_t)kv) & 15) == 0, "q / kv not 16-byte aligned");
  DecSlots slots = {};
  RpStatus st = dbg_slots(slots, state, pos, n_active, n_states, nb, max_len);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream_;
  if (cross) {
    for (int a = 0; a < n_active; ++a) {
      RP_REQUIRE(src_len[a] >= 1 && src_len[a] <= DEC_MAX_KEYS, "src_len[%d]=%d (1..%d)", a, src_len[a], DEC_MAX_KEYS);
      RP_REQUIRE(src_off[a] >= 0 && (int64_t)src_off[a] + src_len[a] <= rows, "src_off[%d]=%d + src_len outside [0, rows=%d]", a,
                 src_off[a], rows);
      slots.src_off[a] = src_off[a];
      slots.src_len[a] = src_len[a];
    }
    launch_dec_cross_attention((const bf16_t*)q, ldq, (const bf16_t*)kv, ldkv, koff, voff, nb, H, slots, n_active * nb,
                               (bf16_t*)out, ldo, s);
  } else {
    RP_REQUIRE(anc && tab && nbias >= 1, "self-attention: null ancestry / bias table");
    RP_REQUIRE(rows == max_len * nb && state_stride >= (int64_t)rows * ldkv && state_stride % 8 == 0,
               "rows=%d (max_len * nb), state_stride=%lld", rows, (long long)state_stride);
    for (int a = 0; a < n_active; ++a)
      RP_REQUIRE(astride >= pos[a] + 1, "anc_stride=%d < pos[%d] + 1 = %d", astride, a, pos[a] + 1);
    launch_dec_self_attention((const bf16_t*)q, ldq, (const bf16_t*)kv, ldkv, koff, voff, rows, (size_t)state_stride, anc,
                              astride, tab, nbias, nb, H, slots, n_active * nb, (bf16_t*)out, ldo, s);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_beam_select_batch(const float* lp, const float* running, int32_t n_active, int32_t nb, int32_t V,
                                         int32_t k, float* scores, int32_t* tokens, int32_t* parents, void* ws,
                                         size_t ws_bytes, void* stream_) {
  RP_REQUIRE(lp && running && scores && tokens && parents, "null argument");
  RP_REQUIRE(n_active >= 1 && n_active <= DEC_MAX_STATES, "states=%d (1..%d)", n_active, DEC_MAX_STATES);
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(V >= 1 && V <= DEC_SELECT_ROW, "vocab=%d (1..%d)", V, DEC_SELECT_ROW);
  RP_REQUIRE(k >= 1 && k <= DEC_SELECT_MAX_K && k <= nb * V, "k=%d (1..min(%d, nb * vocab))", k, DEC_SELECT_MAX_K);
  const int kr = std::min(k, V);  // a row contributes at most k candidates
  const size_t need = (size_t)n_active * nb * kr * sizeof(uint64_t);
  if (!ws || ws_bytes < need) return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream_;
  uint64_t* cand = (uint64_t*)ws;
  hipLaunchKernelGGL(beam_row_topk_kernel, dim3(n_active * nb), dim3(256), 0, s, lp, running, V, kr, nb, cand);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(n_active), dim3(1024), 0, s, cand, nb * kr, V, k, scores, tokens, parents);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" float rp_sample_uniform(uint32_t seed, uint32_t sample, uint32_t position) {
  return sample_uniform(seed, sample, position);
}

namespace {
// The slot list of a books launch: active[a] distinct and in [0, n), slot a at position pos[a] (null: t for all).
RpStatus books_slots(DecSlots* slots, const int32_t* active, const int32_t* pos, int t, int n_active, int n, int max_len) {
  RP_REQUIRE(n_active >= 1 && n_active <= n, "active states=%d (1..states=%d)", n_active, n);
  return dec_list(active, n_active, n, "active", "state", [&](int a, int id) -> RpStatus {
    const int p = pos ? pos[a] : t;
    RP_REQUIRE(p >= 0 && p + 1 < max_len, "pos[%d]=%d: position pos + 1 outside [1, max_len=%d)", a, p, max_len);
    slots->state[a] = id;
    slots->pos[a] = p;
    return RP_OK;
  });
}

// the caps the sampler's entry points share; `listed` = the states the call names (active, or admitted)
RpStatus sample_caps(int n, int nb, int listed, int max_len) {
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n >= 1 && n <= DEC_MAX_STATES, "states=%d (1..%d)", n, DEC_MAX_STATES);
  RP_REQUIRE(max_len >= 2, "max_len=%d < 2", max_len);
  RP_REQUIRE((int64_t)listed * nb <= DEC_MAX_ROWS, "rows = listed states * nb = %lld > %d", (long long)listed * nb,
             DEC_MAX_ROWS);
  return RP_OK;
}

// rp_sample_step (pos null: every slot at t) and rp_sample_pool_step (slot a at pos[a]), and their _rows forms (by_row:
// the parameters come from the table `params`, the three by-value ones are not looked at): one check list, one kernel
RpStatus sample_step_launch(const float* lp, int V, const int32_t* active, const int32_t* pos, int t, int n_active, int n,
                            int nb, const uint32_t* seeds, int max_len, float temperature, int top_k, float top_p,
                            bool by_row, const void* params, int eos, int pad, int32_t* seq, int32_t* tokens_next,
                            float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream_) {
  RP_REQUIRE(lp && active && seeds && seq && tokens_next && cum_logprob && n_generated && finished, "null argument");
  if (by_row) {
    RP_REQUIRE(params, "null argument (params)");
    RP_REQUIRE((uintptr_t)params % 16 == 0, "params=%p is not 16-byte aligned", params);
  } else {
    RP_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "temperature=%g, not a positive finite number",
               (double)temperature);
    RP_REQUIRE(top_p > 0.f && top_p <= 1.f, "top_p=%g outside (0, 1]", (double)top_p);
    RP_REQUIRE(top_k >= 0, "top_k=%d < 0", top_k);
  }
  RP_REQUIRE(V >= 1 && V <= DEC_SELECT_ROW, "vocab=%d (1..%d)", V, DEC_SELECT_ROW);
  RpStatus st = sample_caps(n, nb, n_active, max_len);
  if (st) return st;
  if (!pos) RP_REQUIRE(t >= 0 && t + 1 < max_len, "t=%d: position t + 1 outside [1, max_len=%d)", t, max_len);
  DecSlots slots = {};
  if ((st = books_slots(&slots, active, pos, t, n_active, n, max_len))) return st;
  const float drop_mass = by_row ? 0.f : (float)(1.0 - (double)top_p);
  hipLaunchKernelGGL(sample_step_kernel, dim3(n_active * nb), dim3(256), 0, (hipStream_t)stream_, lp, V, nb, slots, seeds,
                     max_len, by_row ? 1.f : temperature, by_row ? 0 : top_k, drop_mass, by_row ? (const int4*)params : nullptr,
                     eos, pad, seq, tokens_next, cum_logprob, n_generated, finished);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// rp_sample_pool_admit (n_live null: every row of every admitted state is live) and rp_sample_pool_admit_rows
RpStatus sample_admit_launch(const int32_t* states, const uint32_t* new_seeds, const int32_t* n_live, bool live_rows, int m,
                             int n, int nb, int max_len, int start_token, int pad, uint32_t* seeds, int32_t* seq,
                             float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream_) {
  RP_REQUIRE(states && new_seeds && seeds && seq && cum_logprob && n_generated && finished && (n_live || !live_rows),
             "null argument");
  RpStatus st = sample_caps(n, nb, m, max_len);
  if (st) return st;
  RP_REQUIRE(m >= 1 && m <= n, "admitted states=%d (1..states=%d)", m, n);
  DecSlots slots = {};
  SampleSeeds fresh = {};
  SampleLive live = {};
  st = dec_list(states, m, n, "states", "state", [&](int j, int id) -> RpStatus {
    if (live_rows) RP_REQUIRE(n_live[j] >= 1 && n_live[j] <= nb, "n_live[%d]=%d outside 1..nb=%d", j, n_live[j], nb);
    slots.state[j] = id;
    fresh.seed[j] = new_seeds[j];
    live.n_live[j] = live_rows ? n_live[j] : nb;
    return RP_OK;
  });
  if (st) return st;
  hipLaunchKernelGGL(sample_admit_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream_, slots, fresh, live, nb, max_len,
                     start_token, pad, seeds, seq, cum_logprob, n_generated, finished);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
}  // namespace

extern "C" RpStatus rp_sample_step(const float* lp, int32_t V, const int32_t* active, int32_t n_active, int32_t n,
                                   int32_t nb, const uint32_t* seeds, int32_t t, int32_t max_len, float temperature,
                                   int32_t top_k, float top_p, int32_t eos, int32_t pad, int32_t* seq, int32_t* tokens_next,
                                   float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream_) {
  return sample_step_launch(lp, V, active, nullptr, t, n_active, n, nb, seeds, max_len, temperature, top_k, top_p, false,
                            nullptr, eos, pad, seq, tokens_next, cum_logprob, n_generated, finished, stream_);
}

extern "C" RpStatus rp_sample_step_rows(const float* lp, int32_t V, const int32_t* active, int32_t n_active, int32_t n,
                                        int32_t nb, const uint32_t* seeds, int32_t t, int32_t max_len, const void* params,
                                        int32_t eos, int32_t pad, int32_t* seq, int32_t* tokens_next, float* cum_logprob,
                                        int32_t* n_generated, int32_t* finished, void* stream_) {
  return sample_step_launch(lp, V, active, nullptr, t, n_active, n, nb, seeds, max_len, 0.f, 0, 0.f, true, params, eos, pad,
                            seq, tokens_next, cum_logprob, n_generated, finished, stream_);
}

// ---- the slot pool's sampler ("Continuous batching for sampling"): state index = slot place ----------
extern "C" RpStatus rp_sample_pool_step(const float* lp, int32_t V, const int32_t* active, const int32_t* pos,
                                        int32_t n_active, int32_t n, int32_t nb, const uint32_t* seeds, int32_t max_len,
                                        float temperature, int32_t top_k, float top_p, int32_t eos, int32_t pad,
                                        int32_t* seq, int32_t* tokens_next, float* cum_logprob, int32_t* n_generated,
                                        int32_t* finished, void* stream_) {
  RP_REQUIRE(pos, "null argument");
  return sample_step_launch(lp, V, active, pos, 0, n_active, n, nb, seeds, max_len, temperature, top_k, top_p, false, nullptr,
                            eos, pad, seq, tokens_next, cum_logprob, n_generated, finished, stream_);
}

extern "C" RpStatus rp_sample_pool_step_rows(const float* lp, int32_t V, const int32_t* active, const int32_t* pos,
                                             int32_t n_active, int32_t n, int32_t nb, const uint32_t* seeds, int32_t max_len,
                                             const void* params, int32_t eos, int32_t pad, int32_t* seq,
                                             int32_t* tokens_next, float* cum_logprob, int32_t* n_generated,
                                             int32_t* finished, void* stream_) {
  RP_REQUIRE(pos, "null argument");
  return sample_step_launch(lp, V, active, pos, 0, n_active, n, nb, seeds, max_len, 0.f, 0, 0.f, true, params, eos, pad, seq,
                            tokens_next, cum_logprob, n_generated, finished, stream_);
}

extern "C" RpStatus rp_sample_pool_admit(const int32_t* states, const uint32_t* new_seeds, int32_t m, int32_t n, int32_t nb,
                                         int32_t max_len, int32_t start_token, int32_t pad, uint32_t* seeds, int32_t* seq,
                                         float* cum_logprob, int32_t* n_generated, int32_t* finished, void* stream_) {
  return sample_admit_launch(states, new_seeds, nullptr, false, m, n, nb, max_len, start_token, pad, seeds, seq, cum_logprob,
                             n_generated, finished, stream_);
}

extern "C" RpStatus rp_sample_pool_admit_rows(const int32_t* states, const uint32_t* new_seeds, const int32_t* n_live,
                                              int32_t m, int32_t n, int32_t nb, int32_t max_len, int32_t start_token,
                                              int32_t pad, uint32_t* seeds, int32_t* seq, float* cum_logprob,
                                              int32_t* n_generated, int32_t* finished, void* stream_) {
  return sample_admit_launch(states, new_seeds, n_live, true, m, n, nb, max_len, start_token, pad, seeds, seq, cum_logprob,
                             n_generated, finished, stream_);
}

extern "C" RpStatus rp_sample_pool_rows(const int32_t* active, const int32_t* pos, int32_t n_active, int32_t n, int32_t nb,
                                        int32_t max_len, const int32_t* seq, int32_t* tokens_next, void* stream_) {
  RP_REQUIRE(active && pos && seq && tokens_next, "null argument");
  RpStatus st = sample_caps(n, nb, n_active, max_len);
  if (st) return st;
  DecSlots slots = {};
  if ((st = books_slots(&slots, active, pos, 0, n_active, n, max_len))) return st;
  hipLaunchKernelGGL(sample_rows_kernel, dim3(n_active), dim3(64), 0, (hipStream_t)stream_, slots, nb, max_len, seq,
                     tokens_next);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// ---- constrained decoding ("Constrained decoding") -----------------------------------------------------
// (The kernels stand here, after every other kernel of the file, so that adding them moves no existing kernel inside
// the code object: a kernel's cycles shift by a few per cent with its placement.)
namespace {
// One wave per row, four rows per workgroup, no LDS: the row's V log-probs (as bits) and the V int16 of its automaton
// state's row of `next` are walked in vectors of W = 4, 2 or 1 elements, the widest for which one shared head of < W
// elements leaves both the log-prob pointer 4 W-byte aligned and the table pointer 2 W-byte aligned.  Rows of a width
// that is a multiple of 4 take W = 4 with no head (16-byte and 8-byte accesses, 256 elements per pass of the wave); other
// widths take what the two row starts allow.  An entry is rewritten to -inf where next < 0; every other word is stored
// back as the bits that were loaded.
template <int W>
__device__ __forceinline__ void mask_row(uint32_t* __restrict__ lp, const int16_t* __restrict__ nx, int V, int lane) {
  typedef uint32_t U __attribute__((ext_vector_type(W)));
  typedef int16_t S __attribute__((ext_vector_type(W)));
  constexpr uint32_t NEG_INF = 0xff800000u;
  int head = 0;
  if (W > 1) head = min(V, (int)((W - (((uintptr_t)lp >> 2) & (W - 1))) & (W - 1)));
  if (lane < head && nx[lane] < 0) lp[lane] = NEG_INF;
  const int nvec = (V - head) / W;
  for (int i = lane; i < nvec; i += 64) {
    const int at = head + i * W;
    if constexpr (W == 1) {
      if (nx[at] < 0) lp[at] = NEG_INF;
    } else {
      U x = *reinterpret_cast<const U*>(lp + at);
      const S s = *reinterpret_cast<const S*>(nx + at);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (s[j] < 0) x[j] = NEG_INF;
      *reinterpret_cast<U*>(lp + at) = x;
    }
  }
  const int tail = head + nvec * W + lane;
  if (tail < V && nx[tail] < 0) lp[tail] = NEG_INF;
}

// row `row` of logprobs masked by state q (already inside [0, n_q)) of the table
__device__ __forceinline__ void mask_row_any(float* __restrict__ logprobs, const int16_t* __restrict__ next, int V, int row,
                                             int q, int lane) {
  uint32_t* lp = reinterpret_cast<uint32_t*>(logprobs) + (size_t)row * V;
  const int16_t* nx = next + (size_t)q * V;
  const unsigned d = (unsigned)(((uintptr_t)lp >> 2) - ((uintptr_t)nx >> 1)) & 3u;  // the two starts, in elements, mod 4
  if (d == 0) mask_row<4>(lp, nx, V, lane);
  else if (d == 2) mask_row<2>(lp, nx, V, lane);
  else mask_row<1>(lp, nx, V, lane);
}

// rp_constraint_mask: row r by state q_rows[r].  q_rows is device memory, so its values are clamped into [0, n_q) here.
__global__ __launch_bounds__(256) void constraint_mask_kernel(float* __restrict__ logprobs, int V, int rows,
                                                              const int32_t* __restrict__ q_rows,
                                                              const int16_t* __restrict__ next, int n_q) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int q = min(max(q_rows[row], 0), n_q - 1);
  mask_row_any(logprobs, next, V, row, q, lane);
}

// rp_constraint_mask_step: the state of row a * nb + b lives in q[state, b] like the sampler's books.  It is advanced by
// the token the step was fed (pos 0: back to the start state, which is also how a slot's next tenant starts clean; a
// forbidden token - the pad a finished row is fed - leaves it), written back by lane 0, and the row is masked by it.
// Every value read from device memory (q, the token, the table's entry) is clamped before it indexes anything.
__global__ __launch_bounds__(256) void constraint_mask_step_kernel(float* __restrict__ logprobs, int V, int rows, int nb,
                                                                   DecSlots slots, const int32_t* __restrict__ tokens_in,
                                                                   int32_t* __restrict__ q, const int16_t* __restrict__ next,
                                                                   int n_q) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int slot = row / nb, b = row - slot * nb;
  const size_t idx = (size_t)slots.state[slot] * nb + b;
  int qn = 0;
  if (slots.pos[slot] != 0) {
    qn = min(max(q[idx], 0), n_q - 1);
    const int tok = min(max(tokens_in[row], 0), V - 1);
    const int to = next[(size_t)qn * V + tok];
    if (to >= 0) qn = min(to, n_q - 1);
  }
  if (lane == 0) q[idx] = qn;
  mask_row_any(logprobs, next, V, row, qn, lane);
}

// what the two entries ask of the log-probs and the table
RpStatus constraint_caps(const float* logprobs, int V, const int16_t* next, int n_q) {
  RP_REQUIRE((uintptr_t)logprobs % 4 == 0 && (uintptr_t)next % 2 == 0, "logprobs=%p / next=%p is not aligned to its type",
             (const void*)logprobs, (const void*)next);
  RP_REQUIRE(V >= 1 && V <= DEC_SELECT_ROW, "vocab=%d (1..%d)", V, DEC_SELECT_ROW);
  RP_REQUIRE(n_q >= 1 && n_q <= 4096, "n_q=%d (1..4096)", n_q);
  return RP_OK;
}
}  // namespace

extern "C" RpStatus rp_constraint_mask(float* logprobs, int32_t V, int32_t rows, const int32_t* q_rows, const int16_t* next,
                                       int32_t n_q, void* stream_) {
  RP_REQUIRE(logprobs && q_rows && next, "null argument");
  if (RpStatus st = constraint_caps(logprobs, V, next, n_q)) return st;
  RP_REQUIRE(rows >= 1 && rows <= DEC_MAX_ROWS, "rows=%d (1..%d)", rows, DEC_MAX_ROWS);
  hipLaunchKernelGGL(constraint_mask_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream_, logprobs, V, rows,
                     q_rows, next, n_q);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_constraint_mask_step(float* logprobs, int32_t V, const int32_t* active, const int32_t* pos,
                                            int32_t n_active, int32_t n, int32_t nb, const int32_t* tokens_in, int32_t* q,
                                            const int16_t* next, int32_t n_q, void* stream_) {
  RP_REQUIRE(logprobs && active && pos && tokens_in && q && next, "null argument");
  if (RpStatus st = constraint_caps(logprobs, V, next, n_q)) return st;
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n >= 1 && n <= DEC_MAX_STATES, "states=%d (1..%d)", n, DEC_MAX_STATES);
  RP_REQUIRE(n_active >= 1 && n_active <= n, "active states=%d (1..states=%d)", n_active, n);
  RP_REQUIRE((int64_t)n_active * nb <= DEC_MAX_ROWS, "rows = listed states * nb = %lld > %d", (long long)n_active * nb,
             DEC_MAX_ROWS);
  DecSlots slots = {};
  RpStatus st = dec_list(active, n_active, n, "active", "state", [&](int a, int id) -> RpStatus {
    RP_REQUIRE(pos[a] >= 0, "pos[%d]=%d < 0", a, pos[a]);
    slots.state[a] = id;
    slots.pos[a] = pos[a];
    return RP_OK;
  });
  if (st) return st;
  const int rows = n_active * nb;
  hipLaunchKernelGGL(constraint_mask_step_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream_, logprobs, V, rows,
                     nb, slots, tokens_in, q, next, n_q);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

namespace {
RpStatus books_check(int n, int nb, int max_len) {
  RP_REQUIRE(nb >= 1 && nb <= DEC_MAX_BEAMS, "nb=%d (1..%d)", nb, DEC_MAX_BEAMS);
  RP_REQUIRE(n >= 1 && n <= DEC_MAX_STATES, "states=%d (1..%d)", n, DEC_MAX_STATES);
  RP_REQUIRE(n * nb <= DEC_MAX_ROWS, "rows = states * nb = %d > %d", n * nb, DEC_MAX_ROWS);
  RP_REQUIRE(max_len >= 2 && max_len <= DEC_MAX_KEYS, "max_len=%d (2..%d)", max_len, DEC_MAX_KEYS);
  return RP_OK;
}
}  // namespace

extern "C" size_t rp_beam_books_bytes(int32_t n, int32_t nb, int32_t max_len) {
  if (books_check(n, nb, max_len) != RP_OK) return 0;
  return books_carve(nullptr, n, nb, max_len).bytes;
}

extern "C" RpStatus rp_beam_books_init(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len, int32_t eos,
                                       int32_t start_token, void* stream_) {
  RpStatus st = books_check(n, nb, max_len);
  if (st) return st;
  RP_REQUIRE(books, "null books");
  const BeamBooks bk = books_carve((char*)books, n, nb, max_len);
  RP_REQUIRE(bytes >= bk.bytes, "books %zu < required %zu bytes", bytes, bk.bytes);
  hipStream_t s = (hipStream_t)stream_;
  RP_HIP(hipMemsetAsync(books, 0, bk.bytes, s));  // the padding between the parts
  hipLaunchKernelGGL(beam_books_init_kernel, dim3(n), dim3(256), 0, s, bk, n, nb, max_len, eos, start_token);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

namespace {
RpStatus books_advance(void* books, size_t bytes, int n, int nb, int max_len, const DecSlots& slots, const BeamDivs& divs,
                       int n_active, const float* scores, const int32_t* tokens, const int32_t* parents, int eos,
                       void* stream_) {
  const BeamBooks bk = books_carve((char*)books, n, nb, max_len);
  RP_REQUIRE(bytes >= bk.bytes, "books %zu < required %zu bytes", bytes, bk.bytes);
  hipLaunchKernelGGL(beam_advance_kernel, dim3(n_active), dim3(256), 0, (hipStream_t)stream_, bk, n, nb, max_len, slots, divs,
                     scores, tokens, parents, eos);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
}  // namespace

extern "C" RpStatus rp_beam_advance(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len,
                                    const int32_t* active, int32_t n_active, int32_t t, const float* scores,
                                    const int32_t* tokens, const int32_t* parents, float fin_div, float run_div,
                                    int32_t eos, void* stream_) {
  RpStatus st = books_check(n, nb, max_len);
  if (st) return st;
  RP_REQUIRE(books && active && scores && tokens && parents, "null argument");
  RP_REQUIRE(n_active >= 1 && n_active <= n, "active states=%d (1..states=%d)", n_active, n);
  RP_REQUIRE(t >= 0 && t + 1 < max_len, "t=%d: position t + 1 outside [1, max_len=%d)", t, max_len);
  DecSlots slots = {};
  BeamDivs divs = {};
  if ((st = books_slots(&slots, active, nullptr, t, n_active, n, max_len))) return st;
  for (int a = 0; a < n_active; ++a) {
    divs.fin[a] = fin_div;
    divs.run[a] = run_div;
  }
  return books_advance(books, bytes, n, nb, max_len, slots, divs, n_active, scores, tokens, parents, eos, stream_);
}

extern "C" RpStatus rp_beam_pool_advance(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len,
                                         const int32_t* active, const int32_t* pos, int32_t n_active, const float* scores,
                                         const int32_t* tokens, const int32_t* parents, const float* fin_div,
                                         const float* run_div, int32_t eos, void* stream_) {
  RpStatus st = books_check(n, nb, max_len);
  if (st) return st;
  RP_REQUIRE(books && active && pos && scores && tokens && parents && fin_div && run_div, "null argument");
  DecSlots slots = {};
  BeamDivs divs = {};
  if ((st = books_slots(&slots, active, pos, 0, n_active, n, max_len))) return st;
  for (int a = 0; a < n_active; ++a) {
    divs.fin[a] = fin_div[a];
    divs.run[a] = run_div[a];
  }
  return books_advance(books, bytes, n, nb, max_len, slots, divs, n_active, scores, tokens, parents, eos, stream_);
}

extern "C" RpStatus rp_beam_books_admit(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len,
                                        const int32_t* states, int32_t m, int32_t eos, int32_t start_token, void* stream_) {
  RpStatus st = books_check(n, nb, max_len);
  if (st) return st;
  RP_REQUIRE(books && states, "null argument");
  RP_REQUIRE(m >= 1 && m <= n, "admitted states=%d (1..states=%d)", m, n);
  DecSlots slots = {};
  st = dec_list(states, m, n, "states", "state", [&](int j, int id) -> RpStatus {
    slots.state[j] = id;
    return RP_OK;
  });
  if (st) return st;
  const BeamBooks bk = books_carve((char*)books, n, nb, max_len);
  RP_REQUIRE(bytes >= bk.bytes, "books %zu < required %zu bytes", bytes, bk.bytes);
  hipLaunchKernelGGL(beam_books_admit_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream_, bk, n, nb, max_len, slots, eos,
                     start_token);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_beam_books_rows(void* books, size_t bytes, int32_t n, int32_t nb, int32_t max_len,
                                       const int32_t* active, const int32_t* pos, int32_t n_active, void* stream_) {
  RpStatus st = books_check(n, nb, max_len);
  if (st) return st;
  RP_REQUIRE(books && active && pos, "null argument");
  DecSlots slots = {};
  if ((st = books_slots(&slots, active, pos, 0, n_active, n, max_len))) return st;
  const BeamBooks bk = books_carve((char*)books, n, nb, max_len);
  RP_REQUIRE(bytes >= bk.bytes, "books %zu < required %zu bytes", bytes, bk.bytes);
  hipLaunchKernelGGL(beam_books_rows_kernel, dim3(n_active), dim3(256), 0, (hipStream_t)stream_, bk, n, nb, max_len, slots);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// ---- the per-state entry points: one state, its source at rows [0, S), alone in the active list --------------------------
extern "C" size_t rp_decoder_workspace_bytes(const RpDecoder* d, int32_t nb, int32_t max_len, int32_t S) {
  const int32_t cu[2] = {0, S};
  return rp_decoder_batch_workspace_bytes(d, cu, 1, nb, max_len);
}

extern "C" RpStatus rp_decoder_cross_kv(RpDecoder* d, const void* enc, int32_t S, int32_t nb, int32_t max_len, void* ws,
                                        size_t ws_bytes, void* stream) {
  const int32_t cu[2] = {0, S};
  return rp_decoder_batch_cross_kv(d, enc, cu, 1, nb, max_len, ws, ws_bytes, stream);
}

extern "C" RpStatus rp_decoder_step(RpDecoder* d, const int32_t* tokens, const int32_t* anc, int32_t astride, int32_t nb,
                                    int32_t t, int32_t max_len, int32_t S, float* logprobs, void* ws, size_t ws_bytes,
                                    void* stream) {
  const int32_t cu[2] = {0, S}, active = 0;
  return rp_decoder_batch_step(d, cu, 1, &active, 1, tokens, anc, astride, nb, t, max_len, logprobs, ws, ws_bytes, stream);
}

extern "C" RpStatus rp_beam_select(const float* lp, const float* running, int32_t nb, int32_t V, int32_t k, float* scores,
                                   int32_t* tokens, int32_t* parents, void* ws, size_t ws_bytes, void* stream) {
  return rp_beam_select_batch(lp, running, 1, nb, V, k, scores, tokens, parents, ws, ws_bytes, stream);
}
