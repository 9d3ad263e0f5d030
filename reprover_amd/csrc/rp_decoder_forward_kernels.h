// Device code and host helpers of the teacher-forced decoder forward.  fwd_launch_layers below is the one launch sequence;
// rp_decoder_forward.hip (the loss) runs it on one buffer per kind, rp_decoder_backward.hip (the loss and its gradients)
// on per-layer activation slots: two fillings of FwdLayerBufs, the same launches.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "rp_decoder_common.h"
#include "rp_encoder_kernels.h"

using namespace rp;

namespace {

constexpr int FWD_MAX_LEN = 8192;   // tokens of one source or one target
constexpr int FWD_MAX_VOCAB = 512;  // the loss row kernel keeps a row in registers: 2 values per lane of 256
constexpr int FWD_BN = 128;         // token tile of the GEMM configuration below
using FwdCfg = GemmCfg<64, 128, 64, 1, 4, 4>;  // features x tokens x K, 1 x 4 waves, 4 stages (launch_gemm variant 16)

// ---- GEMM epilogues (transposed issue: rows = output features, columns = tokens) ------------------------------------
// acc[i][j][4 g + e]  <->  feature m_base + 32 i + 8 g + 4 hi + e,  token n_base + 32 j + (lane & 31): a lane owns four
// consecutive features of one token per register group, stored as 8 (bf16) or 16 (fp32) bytes.
struct EpiDecBf16 {  // out[token, feature] = bf16(acc)
  bf16_t* out;
  int ldo, n_feat, n_tok;
  template <int FM, int FN>
  __device__ __forceinline__ void run(f32x16 (&acc)[FM][FN], int m_base, int n_base, int lane, char*) {
    const int hi = lane >> 5, cl = lane & 31;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int t = n_base + 32 * j + cl;
      if (t >= n_tok) continue;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = m_base + 32 * i + 8 * g + 4 * hi;
          if (f >= n_feat) continue;
          uint2 v;
          v.x = pack_bf2(acc[i][j][4 * g], acc[i][j][4 * g + 1]);
          v.y = pack_bf2(acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
          *reinterpret_cast<uint2*>(out + (size_t)t * ldo + f) = v;
        }
    }
  }
};
// Training dropout of an epilogue (rp_decoder_loss_grad_dropout): the mask of (site, row = token, column = feature)
// multiplies the fp32 accumulator before anything is rounded or added.  The <.., false> forms hold no such member.
struct DropSite {
  Drop d;
  uint32_t site;
};
struct NoDropSite {};
template <bool DROP>
using DropSiteIf = typename std::conditional<DROP, DropSite, NoDropSite>::type;
// multipliers of a lane's four consecutive features f .. f + 3 (f a multiple of 4) of token t
__device__ __forceinline__ void drop_mul4(const DropSite& ds, int t, int f, float (&m)[4]) {
  drop_mul2(ds.d, ds.site, (uint32_t)t, (uint32_t)f, m[0], m[1]);
  drop_mul2(ds.d, ds.site, (uint32_t)t, (uint32_t)f + 2u, m[2], m[3]);
}

template <bool ADD, bool DROP = false>
struct EpiDecF32 {  // out[token, feature] (+)= [mask *] acc: the fp32 residual stream (ADD) or the lm_head logits
  float* out;
  int ldo, n_feat, n_tok;
  [[no_unique_address]] DropSiteIf<DROP> drop;  // DROP: HF's dropout on the sub-layer's output before the add (:400, :431, :140)
  template <int FM, int FN>
  __device__ __forceinline__ void run(f32x16 (&acc)[FM][FN], int m_base, int n_base, int lane, char*) {
    const int hi = lane >> 5, cl = lane & 31;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int t = n_base + 32 * j + cl;
      if (t >= n_tok) continue;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = m_base + 32 * i + 8 * g + 4 * hi;
          if (f >= n_feat) continue;
          float* p = out + (size_t)t * ldo + f;
          if constexpr (DROP) {
            float m[4];
            drop_mul4(drop, t, f, m);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][4 * g + e] *= m[e];
          }
          if ((ldo & 3) == 0 && f + 4 <= n_feat) {  // 16-byte aligned and inside the row: one vector access
            float4 v = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
            if constexpr (ADD) {
              const float4 o = *reinterpret_cast<const float4*>(p);
              v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
            }
            *reinterpret_cast<float4*>(p) = v;
          } else {  // a vocabulary that is no multiple of 4: element by element, never past the row's end
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (f + e < n_feat) p[e] = ADD ? p[e] + acc[i][j][4 * g + e] : acc[i][j][4 * g + e];
          }
        }
    }
  }
};
// FFN-in on the interleaved weight (RpDecoder::wi_il): row fragment 2 k is the gate (wi_0) and 2 k + 1 the up (wi_1)
// projection of the same 32 features (m_base is a multiple of 64): out = bf16([mask *] gelu_new(a0) * a1), the decode
// step's form; DROP: HF's dropout inside the gated FFN (:110).
template <bool DROP = false>
struct EpiDecGeglu {
  bf16_t* out;
  int ldo, n_feat, n_tok;
  [[no_unique_address]] DropSiteIf<DROP> drop;
  template <int FM, int FN>
  __device__ __forceinline__ void run(f32x16 (&acc)[FM][FN], int m_base, int n_base, int lane, char*) {
    static_assert(FM % 2 == 0, "gate and up fragments in pairs");
    const int hi = lane >> 5, cl = lane & 31;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int t = n_base + 32 * j + cl;
      if (t >= n_tok) continue;
#pragma unroll
      for (int i = 0; i < FM; i += 2)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = (m_base + 32 * i) / 2 + 8 * g + 4 * hi;
          if (f >= n_feat) continue;
          float r[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = gelu_tanh(acc[i][j][4 * g + e]) * acc[i + 1][j][4 * g + e];
          if constexpr (DROP) {
            float m[4];
            drop_mul4(drop, t, f, m);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] *= m[e];
          }
          uint2 v;
          v.x = pack_bf2(r[0], r[1]);
          v.y = pack_bf2(r[2], r[3]);
          *reinterpret_cast<uint2*>(out + (size_t)t * ldo + f) = v;
        }
    }
  }
};

// out = act [tokens, K] x W[n_rows_w, K]^T through the encoder's tile machinery; rows beyond n_tok are never read
// (the operand clamps at tokens_valid) nor written (the epilogues)
template <class Epi>
RpStatus fwd_gemm(const bf16_t* act, int n_tok, int n_tok_pad, const bf16_t* W, int n_rows_w, int K, Epi epi,
                  hipStream_t s, int prof_class) {
  GemmOperand a{act, K, n_tok_pad}, w{W, K, n_rows_w};
  return launch_gemm_cfg<FwdCfg>(w, a, K, epi, s, prof_class, n_tok, nullptr);
}

// ---- attention ---------------------------------------------------------------------------------------------------------
// Varlen flash attention for the decoder, d_kv = 64, after the encoder's attention_kernel (rp_encoder_kernels.h: the same
// K/V LDS-DMA ring, S^T = K Q^T with one query per lane, O^T = V^T P^T from ds_read_b64_tr_b16 fragments, online softmax
// in the exp2 domain, P rounded to bf16 for the PV MFMA).  Workgroup = (work entry {pair b, first query q0}, head): 128
// queries, wave w owns 32.  Queries are rows q_cu[b] + i of q, keys / values rows k_cu[b] + j of kv.
//   CAUSAL (self-attention): k_cu = q_cu, keys j <= i, score += tab[h * nbias + min(i - j, nbias - 1)]; key tiles past the
//     workgroup's (or the wave's) last query are not visited.
//   else (cross-attention): every key of the pair's source, no bias.
// lse2 (optional, [H, lse_ld]): the row's log-sum-exp in the exp2 domain, what a backward recomputes P from.
constexpr int FA_Q = 128, FA_KV = 64, FA_TAB_MAX = 1024;
constexpr int FA_K_BYTES = 64 * 128, FA_V_BYTES = 64 * 128, FA_STAGE = FA_K_BYTES + FA_V_BYTES;

// DROP (training, rp_decoder_loss_grad_dropout): HF's dropout on the probabilities (:168).  P is masked after the row sum
// and before the PV MFMA, so the normaliser and lse2 are the undropped ones; mask element = (drop_site, row = the query's
// packed index q_cu[b] + i, column = (head << 20) | j).  A lane's keys r, r + 1 (r even) are neighbours, one hash each.
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void dec_flash_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kv,
                                                        int ldkv, int koff, int voff, const int32_t* __restrict__ q_cu,
                                                        const int32_t* __restrict__ k_cu, const int2* __restrict__ work,
                                                        const float* __restrict__ bias_tab, int nbias,
                                                        bf16_t* __restrict__ out, int ldo, float* __restrict__ lse2,
                                                        int lse_ld, Drop drop, uint32_t drop_site) {
  __shared__ __attribute__((aligned(16))) char smem[2 * FA_STAGE + FA_TAB_MAX * 4];
  float* tab = reinterpret_cast<float*>(smem + 2 * FA_STAGE);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, cl = lane & 31;
  const int nh = ldo >> 6;  // heads: blockIdx.x = entry * H + head (heads fastest: neighbours share q / kv rows)
  const int h = blockIdx.x % nh;
  const int2 wk = work[blockIdx.x / nh];
  const int b = wk.x, q0 = wk.y;
  const int qs = q_cu[b], qlen = q_cu[b + 1] - qs;
  const int ks = k_cu[b], klen = k_cu[b + 1] - ks;
  if (qlen <= 0 || klen <= 0) return;  // (the host builds entries for non-empty pairs only)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if constexpr (CAUSAL)
    for (int i = tid; i < nbias; i += 256) tab[i] = bias_tab[(size_t)h * nbias + i];

  const int wq0 = q0 + wave * 32;
  const bool active = wq0 < qlen;  // wave-uniform
  const int qi = wq0 + cl;
  bf16x8 qf[4];
  {
    const bf16_t* qp = q + (size_t)(qs + min(qi, qlen - 1)) * ldq + h * 64 + hi * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const bf16x8*>(qp + c * 16);
  }
  const bf16_t* k_base = kv + (size_t)ks * ldkv + koff + h * 64;
  const bf16_t* v_base = kv + (size_t)ks * ldkv + voff + h * 64;
  // DMA pieces of this wave: K pieces {2w, 2w+1} (8 keys x 128 B each), V pieces {2w, 2w+1} (d-half p >> 2, 16 keys x
  // 64 B each); key rows past the pair's last clamp to it (read, then masked)
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * FA_STAGE;
    const int k0 = kt * FA_KV;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = wave * 2 + e;
      {
        const int key = 8 * p + (lane >> 3);
        const int kc = (lane & 7) ^ ((key >> 1) & 7);
        const bf16_t* src = k_base + (size_t)min(k0 + key, klen - 1) * ldkv + kc * 8;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + p * 1024), 16, 0, 0);
      }
      {
        const int key = 16 * (p & 3) + (lane >> 2);
        const bf16_t* src = v_base + (size_t)min(k0 + key, klen - 1) * ldkv + (p >> 2) * 32 + (lane & 3) * 8;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + FA_K_BYTES + p * 1024), 16, 0, 0);
      }
    }
  };
  int k_off[2][4];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int key = kb * 32 + cl;
      k_off[kb][c] = key * 128 + (((c * 2 + hi) ^ ((key >> 1) & 7)) << 4);
    }
  const int v_off0 = FA_K_BYTES + (4 * hi + ((lane & 15) >> 2)) * 64 + (4 * (lane & 3) + 16 * ((lane >> 4) & 1)) * 2;

  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int kend = CAUSAL ? min(klen, q0 + FA_Q) : klen;
  const int n_tiles = (kend + FA_KV - 1) / FA_KV;
  stage(0, 0);
  for (int kt = 0; kt < n_tiles; ++kt) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // tile kt complete in LDS; tile kt-1's buffer free (and tab written)
    if (kt + 1 < n_tiles) stage(kt + 1, (kt + 1) & 1);
    const int k0 = kt * FA_KV;
    if (!active || (CAUSAL && k0 > wq0 + 31)) continue;  // (every key of the tile lies after every query of the wave)
    const char* sb = smem + (kt & 1) * FA_STAGE;
    // a 32-key block wholly beyond the pair's keys (or, causal, after the wave's last query) is skipped: p = +0 there
    const bool two = k0 + 32 < klen && (!CAUSAL || k0 + 32 <= wq0 + 31);
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (kb == 1 && !two) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16x8 kf = *reinterpret_cast<const bf16x8*>(sb + k_off[kb][c]);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[c], s[kb], 0, 0, 0);
      }
      const int c0 = k0 + kb * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = c0 + mfma32_row(r, hi);
        if constexpr (CAUSAL)
          s[kb][r] = (j < klen && j <= qi) ? s[kb][r] + tab[min(qi - j, nbias - 1)] : -INFINITY;
        else
          s[kb][r] = (j < klen) ? s[kb][r] : -INFINITY;
      }
    }
    float mx = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[0][r]);
    if (two) {
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[1][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);  // finite: key 0 of tile 0 is visible to every query
    const float LOG2E = 1.4426950408889634f;
    const float mneg = -m_new * LOG2E;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (kb == 1 && !two) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[kb][r], LOG2E, mneg));
        s[kb][r] = p;
        psum += p;
      }
    }
    if (__any(m_new != m_run)) {
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);  // m_run = -inf first -> 0
      l_run *= alpha;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    }
    l_run += psum;
    m_run = m_new;
    if constexpr (DROP) {
      const uint32_t row = (uint32_t)(qs + qi), col0 = ((uint32_t)h << 20) | (uint32_t)k0;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && !two) break;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          float m0, m1;
          drop_mul2(drop, drop_site, row, col0 + (uint32_t)(kb * 32 + mfma32_row(r, hi)), m0, m1);
          s[kb][r] *= m0;
          s[kb][r + 1] *= m1;
        }
      }
    }
    // O^T += V^T P^T over four 16-key slabs (P rounded to bf16: DESIGN.md section 10, rounding point R_P)
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      if (sl == 2 && !two) break;
      const int kb = sl >> 1, sub = sl & 1;
      bf16x8 pf;
      {
        uint32_t pw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) pw[e] = pack_bf2(s[kb][8 * sub + 2 * e], s[kb][8 * sub + 2 * e + 1]);
        uint4 t = make_uint4(pw[0], pw[1], pw[2], pw[3]);
        pf = *reinterpret_cast<bf16x8*>(&t);
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const char* vp = sb + v_off0 + d * 4096 + sl * 16 * 64;
        v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(vp));
        v4s16 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(vp + 8 * 64));
        bf16x8 vf;
        vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
        vf[4] = up[0]; vf[5] = up[1]; vf[6] = up[2]; vf[7] = up[3];
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[d], 0, 0, 0);
      }
    }
  }
  if (active && qi < qlen) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_tot;
    if (lse2 && hi == 0) lse2[(size_t)h * lse_ld + qs + qi] = fmaf(m_run, 1.4426950408889634f, __log2f(l_tot));
    bf16_t* op = out + (size_t)(qs + qi) * ldo + h * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 v;
        v.x = pack_bf2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv);
        v.y = pack_bf2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
        *reinterpret_cast<uint2*>(op + d * 32 + 8 * g + 4 * hi) = v;
      }
  }
}

// One forward attention launch over the work list {pair, first query}: the causal form reads q | k | v at koff / voff of
// one fused buffer (k_cu = q_cu) and the bias table, the cross form reads no table.  drop.thresh != 0: the dropout form.
inline void launch_dec_flash(bool causal, const bf16_t* q, int ldq, const bf16_t* kv, int ldkv, int koff, int voff,
                             const int32_t* q_cu, const int32_t* k_cu, const int2* work, int n_work, int H,
                             const float* bias_tab, int nbias, bf16_t* out, int ldo, float* lse2, int lse_ld, hipStream_t s,
                             const Drop& drop = Drop{0u, 0u, 1.f}, uint32_t drop_site = 0u) {
  const dim3 att_grid(H * n_work);
  auto launch = [&](auto kernel, const float* tab, int nb) {
    hipLaunchKernelGGL(kernel, att_grid, dim3(256), 0, s, q, ldq, kv, ldkv, koff, voff, q_cu, k_cu, work, tab, nb, out, ldo,
                       lse2, lse_ld, drop, drop_site);
  };
  if (causal)
    drop.thresh ? launch(dec_flash_kernel<true, true>, bias_tab, nbias) : launch(dec_flash_kernel<true, false>, bias_tab, nbias);
  else
    drop.thresh ? launch(dec_flash_kernel<false, true>, nullptr, 1) : launch(dec_flash_kernel<false, false>, nullptr, 1);
}

// ---- row kernels of the dropout form ---------------------------------------------------------------------------------------
// dec_embed_kernel with HF's dropout on the embeddings (:725): x[t, :] = mask * embed[tokens[t], :]
__global__ __launch_bounds__(256) void dec_embed_drop_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ embed,
                                                             float* __restrict__ x, int D, int V, Drop drop) {
  const int b = blockIdx.x;
  const int tok = min(max(tokens[b], 0), V - 1);
  for (int c = threadIdx.x; c < D; c += 256)
    x[(size_t)b * D + c] = embed[(size_t)tok * D + c] * drop_mul(drop, DROP_SITE_DEC_EMBED, (uint32_t)b, (uint32_t)c);
}
// dec_rmsnorm_kernel with HF's dropout after the final norm (:745): the mask multiplies the fp32 value, one rounding (the
// tied head's d_model^-1/2 in `scale` commutes with it)
__global__ __launch_bounds__(256) void dec_rmsnorm_drop_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               bf16_t* __restrict__ out, int D, float eps, float scale,
                                                               Drop drop) {
  __shared__ float red[4];
  const float* row = x + (size_t)blockIdx.x * D;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) ss = fmaf(row[c], row[c], ss);
  ss = block_sum256(ss, red);
  const float r = rsqrtf(ss / (float)D + eps);
  for (int c = threadIdx.x; c < D; c += 256)
    out[(size_t)blockIdx.x * D + c] =
        f2bf(drop_mul(drop, DROP_SITE_DEC_FINAL, blockIdx.x, (uint32_t)c) * (w[c] * (row[c] * r) * scale));
}

// ---- loss ---------------------------------------------------------------------------------------------------------------
// One workgroup per target row: log_softmax over V <= 512 in fp32 (the decode step's arithmetic: max, sum of __expf,
// (x - max) - log(sum)); lp[row] = the label's log-prob, 0 when the label is ignored (< 0, HF's -100) or out of range.
// rows (optional): the whole [V] row of log-probs.
__global__ __launch_bounds__(256) void fwd_loss_row_kernel(const float* __restrict__ logits, int V,
                                                           const int32_t* __restrict__ labels, float* __restrict__ lp,
                                                           float* __restrict__ rows) {
  __shared__ float red[4];
  const int t = blockIdx.x;
  const float* row = logits + (size_t)t * V;
  const int c0 = threadIdx.x, c1 = threadIdx.x + 256;
  const float x0 = c0 < V ? row[c0] : -INFINITY, x1 = c1 < V ? row[c1] : -INFINITY;
  const float mx = block_max256(fmaxf(x0, x1), red);
  float s = (c0 < V ? __expf(x0 - mx) : 0.f) + (c1 < V ? __expf(x1 - mx) : 0.f);
  s = block_sum256(s, red);
  const float ls = logf(s);
  if (rows) {
    if (c0 < V) rows[(size_t)t * V + c0] = (x0 - mx) - ls;
    if (c1 < V) rows[(size_t)t * V + c1] = (x1 - mx) - ls;
  }
  const int y = labels[t];  // (labels >= V are outside the contract; they are treated as ignored, never read past the row)
  if (threadIdx.x == 0) lp[t] = (y >= 0 && y < V) ? (row[y] - mx) - ls : 0.f;
}

// loss_sum_count[0] = sum over counted rows of -lp (fp64), [1] = their count; counted = label in [0, V).  One workgroup,
// thread i takes rows i, i + 256, ... in order, then a fixed tree: the same bits for the same rows on every run.
__global__ __launch_bounds__(256) void fwd_loss_reduce_kernel(const float* __restrict__ lp, const int32_t* __restrict__ labels,
                                                              int n, int V, double* __restrict__ out) {
  __shared__ double s_sum[256];
  __shared__ double s_cnt[256];
  double sum = 0.0, cnt = 0.0;
  for (int t = threadIdx.x; t < n; t += 256) {
    const int y = labels[t];
    if (y >= 0 && y < V) {
      sum -= (double)lp[t];
      cnt += 1.0;
    }
  }
  s_sum[threadIdx.x] = sum;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = s_sum[0];
    out[1] = s_cnt[0];
  }
}

// ---- workspace and metadata ----------------------------------------------------------------------------------------------
// Bump allocator over a caller's workspace, every buffer 256-byte aligned; base null: sizes only.
struct Carver {
  char* base;
  size_t off = 0;
  char* take(size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  }
};

struct FwdWs {
  int32_t* meta;  // src_cu [B + 1], tgt_cu [B + 1], work entries (int2)
  float* x;       // [Tp, D] residual stream
  bf16_t* h;      // [Tp, D] normed rows
  bf16_t* ff;     // [Tp, F] FFN inner rows
  bf16_t* qkv;    // [Tp, 3 inner]
  bf16_t* att;    // [Tp, inner]
  bf16_t* ckv;    // [Sp, 2 inner] one layer's cross K | V
  float* logits;  // [Tp, V]
  size_t bytes;
};
int fwd_max_work(int batch, int n_tgt) { return n_tgt / FA_Q + batch; }
FwdWs fwd_carve(const RpDecoder* d, int batch, int n_src, int n_tgt, char* base) {
  const size_t D = d->cfg.d_model, F = d->cfg.d_ff, inner = d->inner, V = d->cfg.vocab_size;
  const size_t Tp = align_up((size_t)std::max(n_tgt, 1), FWD_BN), Sp = align_up((size_t)std::max(n_src, 1), FWD_BN);
  FwdWs w;
  Carver c{base};
  w.meta = (int32_t*)c.take((size_t)(2 * (batch + 1) + 2 * fwd_max_work(batch, n_tgt)) * 4);
  w.x = (float*)c.take(Tp * D * 4);
  w.h = (bf16_t*)c.take(Tp * D * 2);
  w.ff = (bf16_t*)c.take(Tp * F * 2);
  w.qkv = (bf16_t*)c.take(Tp * 3 * inner * 2);
  w.att = (bf16_t*)c.take(Tp * inner * 2);
  w.ckv = (bf16_t*)c.take(Sp * 2 * inner * 2);
  w.logits = (float*)c.take(Tp * V * 4);
  w.bytes = c.off;
  return w;
}

// Host image of the metadata: src_cu [B + 1] | tgt_cu [B + 1] | the attention work list {pair, first query} (128-query
// blocks of non-empty targets).  Returns the number of work entries; a caller may append lists of its own.
int fwd_build_meta(const int32_t* src_cu, const int32_t* tgt_cu, int batch, std::vector<int32_t>& meta) {
  meta.assign(src_cu, src_cu + batch + 1);
  meta.insert(meta.end(), tgt_cu, tgt_cu + batch + 1);
  for (int b = 0; b < batch; ++b)
    for (int q0 = 0; q0 < tgt_cu[b + 1] - tgt_cu[b]; q0 += FA_Q) {
      meta.push_back(b);
      meta.push_back(q0);
    }
  return (int)(meta.size() - 2 * (batch + 1)) / 2;
}

// ---- the launch sequence ---------------------------------------------------------------------------------------------------
// Where one layer's activations go.  x0 .. x3: the residual stream at the layer's input and after each of its three
// sub-layers (x3 is the next layer's x0); h0 .. h2: the normed rows of the three sub-layers.  Pointers may coincide
// wherever the later value may overwrite the earlier one (the loss alone: one buffer per kind).  lse (optional,
// [H, lse_ld]): the attention rows' log-sum-exp, what a backward recomputes P from.
struct FwdLayerBufs {
  float *x0, *x1, *x2, *x3;
  bf16_t *h0, *h1, *h2, *qkv, *cq, *ckv, *att_s, *att_c, *ff;
  float *lse_s, *lse_c;
  int lse_ld;
};
struct FwdFinalBufs {
  float* x;  // the last layer's x3
  bf16_t* h;
  float* logits;
};
// scale of the final norm's rows: the tied head reads them times d_model^-1/2
float fwd_head_scale(const RpDecoder* d) { return d->tied ? 1.f / sqrtf((float)d->cfg.d_model) : 1.f; }

// The whole teacher-forced forward on the device copy `meta` of fwd_build_meta's image: embed, the layers, final norm,
// lm_head, the rows' log-softmax + label gather and the fixed-order reduction of the loss.  Where a residual GEMM's
// destination differs from the stream it adds to, the n_tgt * D floats are copied there just before that GEMM.
// drop (thresh 0 = off: the launches and kernels of the loss alone): the training dropout at HF's decoder sites.
RpStatus fwd_launch_layers(const RpDecoder* d, const void* enc_bf16, const int32_t* tokens, const int32_t* labels, int batch,
                           int n_src, int n_tgt, const int32_t* meta, int n_work, const FwdLayerBufs* bufs,
                           const FwdFinalBufs& fin, float* label_logprobs, double* loss_sum_count, float* logprob_rows,
                           hipStream_t s, const Drop& drop = Drop{0u, 0u, 1.f}) {
  const RpT5Config& c = d->cfg;
  const int D = c.d_model, F = c.d_ff, inner = d->inner, H = c.num_heads, V = c.vocab_size, L = c.num_layers;
  const float eps = c.layer_norm_eps;
  const int32_t* d_src_cu = meta;
  const int32_t* d_tgt_cu = meta + batch + 1;
  const int2* d_work = reinterpret_cast<const int2*>(meta + 2 * (batch + 1));
  const int Tp = (int)align_up(n_tgt, FWD_BN), Sp = (int)align_up(n_src, FWD_BN);
  RpStatus st;
  auto norm = [&](const float* x, const float* ln, bf16_t* h, float scale) {
    hipLaunchKernelGGL(dec_rmsnorm_kernel, dim3(n_tgt), dim3(256), 0, s, x, ln, h, D, eps, scale);
  };
  auto move_stream = [&](float* to, const float* from) {
    return to != from ? hipMemcpyAsync(to, from, (size_t)n_tgt * D * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
  };
  // x += [mask *] act W^T  and  ff = bf16([mask *] gelu(gate) * up): the residual and gated-GELU GEMMs in either form
  auto resid_gemm = [&](const bf16_t* act, const bf16_t* W, int K, float* x, uint32_t site, int prof_class) {
    return drop.thresh ? fwd_gemm(act, n_tgt, Tp, W, D, K, EpiDecF32<true, true>{x, D, D, n_tgt, {drop, site}}, s, prof_class)
                       : fwd_gemm(act, n_tgt, Tp, W, D, K, EpiDecF32<true>{x, D, D, n_tgt}, s, prof_class);
  };
  auto geglu_gemm = [&](const bf16_t* act, const bf16_t* W, bf16_t* ff, uint32_t site) {
    return drop.thresh ? fwd_gemm(act, n_tgt, Tp, W, 2 * F, D, EpiDecGeglu<true>{ff, F, F, n_tgt, {drop, site}}, s, RP_K_GEMM_WI)
                       : fwd_gemm(act, n_tgt, Tp, W, 2 * F, D, EpiDecGeglu<>{ff, F, F, n_tgt}, s, RP_K_GEMM_WI);
  };
  if (drop.thresh)
    hipLaunchKernelGGL(dec_embed_drop_kernel, dim3(n_tgt), dim3(256), 0, s, tokens, d->embed, L ? bufs[0].x0 : fin.x, D, V, drop);
  else
    hipLaunchKernelGGL(dec_embed_kernel, dim3(n_tgt), dim3(256), 0, s, tokens, d->embed, L ? bufs[0].x0 : fin.x, D, V);
  for (int i = 0; i < L; ++i) {
    const RpDecoder::Layer& l = d->layers[i];
    const FwdLayerBufs& b = bufs[i];
    const uint32_t site = DROP_SITE_DEC_LAYER0 + 8u * (uint32_t)i;  // + {0 .. 5}: rp_encoder_kernels.h
    // self-attention: x += o(attn(rmsnorm(x))), causal inside each pair
    norm(b.x0, l.ln_self, b.h0, 1.f);
    if ((st = fwd_gemm(b.h0, n_tgt, Tp, l.wqkv, 3 * inner, D, EpiDecBf16{b.qkv, 3 * inner, 3 * inner, n_tgt}, s,
                       RP_K_GEMM_QKV)))
      return st;
    launch_dec_flash(true, b.qkv, 3 * inner, b.qkv, 3 * inner, inner, 2 * inner, d_tgt_cu, d_tgt_cu, d_work, n_work, H,
                     d->bias_tab, d->nbias, b.att_s, inner, b.lse_s, b.lse_ld, s, drop, site);
    RP_HIP(move_stream(b.x1, b.x0));
    if ((st = resid_gemm(b.att_s, l.wo, inner, b.x1, site + 1, RP_K_GEMM_O))) return st;
    // cross-attention: the pair's queries over its own source's K / V (this layer's, from one GEMM over all sources)
    if ((st = fwd_gemm((const bf16_t*)enc_bf16, n_src, Sp, d->cross_kv_w + (size_t)2 * i * inner * D, 2 * inner, D,
                       EpiDecBf16{b.ckv, 2 * inner, 2 * inner, n_src}, s, RP_K_GEMM_QKV)))
      return st;
    norm(b.x1, l.ln_cross, b.h1, 1.f);
    if ((st = fwd_gemm(b.h1, n_tgt, Tp, l.cq, inner, D, EpiDecBf16{b.cq, inner, inner, n_tgt}, s, RP_K_GEMM_QKV)))
      return st;
    launch_dec_flash(false, b.cq, inner, b.ckv, 2 * inner, 0, inner, d_tgt_cu, d_src_cu, d_work, n_work, H, nullptr, 1,
                     b.att_c, inner, b.lse_c, b.lse_ld, s, drop, site + 2);
    RP_HIP(move_stream(b.x2, b.x1));
    if ((st = resid_gemm(b.att_c, l.co, inner, b.x2, site + 3, RP_K_GEMM_O))) return st;
    // gated-GELU FFN
    norm(b.x2, l.ln_ff, b.h2, 1.f);
    if ((st = geglu_gemm(b.h2, d->wi_il + (size_t)i * 2 * F * D, b.ff, site + 4))) return st;
    RP_HIP(move_stream(b.x3, b.x2));
    if ((st = resid_gemm(b.ff, l.wo2, F, b.x3, site + 5, RP_K_GEMM_WO))) return st;
  }
  if (drop.thresh)
    hipLaunchKernelGGL(dec_rmsnorm_drop_kernel, dim3(n_tgt), dim3(256), 0, s, (const float*)fin.x, (const float*)d->final_ln,
                       fin.h, D, eps, fwd_head_scale(d), drop);
  else
    norm(fin.x, d->final_ln, fin.h, fwd_head_scale(d));
  if ((st = fwd_gemm(fin.h, n_tgt, Tp, d->lm_head, V, D, EpiDecF32<false>{fin.logits, V, V, n_tgt}, s, RP_K_GEMM_O)))
    return st;
  hipLaunchKernelGGL(fwd_loss_row_kernel, dim3(n_tgt), dim3(256), 0, s, fin.logits, V, labels, label_logprobs, logprob_rows);
  hipLaunchKernelGGL(fwd_loss_reduce_kernel, dim3(1), dim3(256), 0, s, label_logprobs, labels, n_tgt, V, loss_sum_count);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

RpStatus fwd_check_model(const RpDecoder* d) {
  RP_REQUIRE(d, "null decoder");
  const RpT5Config& c = d->cfg;
  if (c.d_model % 64 || c.d_ff % 64 || d->inner % 64)
    return fail(RP_E_UNSUPPORTED, "d_model=%d, d_ff=%d, H*d_kv=%d: the forward's GEMMs need multiples of 64", c.d_model,
                c.d_ff, d->inner);
  if (!d->wi_il) return fail(RP_E_UNSUPPORTED, "the decoder holds no interleaved FFN-in weight");
  if (c.vocab_size > FWD_MAX_VOCAB) return fail(RP_E_UNSUPPORTED, "vocab_size=%d > %d", c.vocab_size, FWD_MAX_VOCAB);
  if (d->nbias > FA_TAB_MAX) return fail(RP_E_UNSUPPORTED, "relative_attention_max_distance=%d too large", c.rel_max_distance);
  return RP_OK;
}

// host totals from the cu arrays, with the per-pair bounds
RpStatus fwd_check_cu(const int32_t* src_cu, const int32_t* tgt_cu, int batch, int& n_src, int& n_tgt) {
  RP_REQUIRE(src_cu && tgt_cu, "null cu array");
  RP_REQUIRE(batch >= 1 && batch <= (1 << 20), "batch=%d", batch);
  RP_REQUIRE(src_cu[0] == 0 && tgt_cu[0] == 0, "cu arrays must start at 0");
  for (int b = 0; b < batch; ++b) {
    const int s = src_cu[b + 1] - src_cu[b], t = tgt_cu[b + 1] - tgt_cu[b];
    RP_REQUIRE(s >= 0 && s <= FWD_MAX_LEN, "source %d: %d tokens (0..%d)", b, s, FWD_MAX_LEN);
    RP_REQUIRE(t >= 0 && t <= FWD_MAX_LEN, "target %d: %d tokens (0..%d)", b, t, FWD_MAX_LEN);
    RP_REQUIRE(t == 0 || s >= 1, "pair %d: a non-empty target needs a non-empty source", b);
  }
  n_src = src_cu[batch];
  n_tgt = tgt_cu[batch];
  RP_REQUIRE(n_src < (1 << 28) && n_tgt < (1 << 28), "too many tokens");
  return RP_OK;
}

}  // namespace
