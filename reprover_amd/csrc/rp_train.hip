// Training step of the retriever on gfx950: encoder forward with saved activations, encoder backward, flat-buffer
// optimizer support.  Replaces what autograd does behind retrieval/model.py:155-181 (`training_step` differentiating
// `forward` :116-140 through `_encode` :92-114 and HuggingFace's T5Stack); common.py:381-405 (`get_optimizers`) is
// rp_adamw_step over the flat parameter buffer.  Device code: rp_train_kernels.h; oracle: oracle/train_ref.py (G11, G12).
//
// Parameters, gradients and moments are FLAT fp32 device buffers in one canonical layout (rp_train_param_layout):
//   embed [V, D] | rel_bias [buckets, H] | final_ln [D] | per layer: ln_attn [D], q, k, v [H*64, D], o [D, H*64],
//   ln_ff [D], wi_0, wi_1 [F, D], wo [D, F]        (each tensor starts at a multiple of 64 elements)
// so that the optimizer, the gradient norm and a checkpoint are one launch / one copy each, and the host views any
// tensor in place.  The engine keeps bf16 compute copies (the forward's packed weights and their transposes for the
// dgrad GEMMs), refreshed from the fp32 masters by rp_trainer_load_params after every optimizer step.
//
// What is saved for the backward (per layer, per token): bf16(x) entering each sub-layer, rs of both RMSNorms, qkv, the
// attention output and its log-sum-exp, the row-scaled gate/up pre-activations and their gated product: 30.5 KB per token
// and layer for ByT5-small (366 KB per token at 12 layers; 41 k tokens = 15 GB of the 288 GB).  Nothing is recomputed
// except the attention probabilities (flash-style, from q, k, the bias table and the log-sum-exp).
// Dropout: T5's dropout (0.1 in the reference's training) at HF's six sites, counter-based (rp_trainer_set_dropout): the
// backward regenerates the forward's masks.  p = 0 is the deterministic step fixtures G11 / G12 pin; either way the step is
// bit-reproducible run to run for a given seed.
// The same layer loops serve two hand-overs: the pooled embedding (rp_train_forward / rp_train_backward, the retriever) and
// last_hidden_state (rp_train_forward_hidden / rp_train_backward_hidden: the encoder half of the seq2seq loss's gradient,
// generation/model.py:117-121; without dropout).  Only the head around the final RMSNorm differs.
#include "rp_train_kernels.h"

using namespace rp;

namespace rp {
int g_train_dbg = 0;  // experiments (rp_set_option "train_dbg", probe builds): bit 0 = skip the bias-table gradient's LDS atomics
// rp_set_option "train_wgrad_form" (tests): bit 0 = the weight gradients of a sub-layer as separate launches (rounds 3-5),
// bit 1 = dWi' finished by unfold_kernel even when its launch has no split
int g_train_wgrad_form = 0;
}

namespace {

constexpr int N_GLOBAL = 3;       // embed, rel_bias, final_ln
constexpr int N_PER_LAYER = 9;    // ln_attn q k v o ln_ff wi_0 wi_1 wo
enum { P_LN_ATTN = 0, P_Q, P_K, P_V, P_O, P_LN_FF, P_WI0, P_WI1, P_WO };

struct Layout {
  std::vector<int64_t> off;  // [3 + 9 L + 1], last = total
  int64_t embed() const { return off[0]; }
  int64_t rel_bias() const { return off[1]; }
  int64_t final_ln() const { return off[2]; }
  int64_t layer(int i, int which) const { return off[N_GLOBAL + i * N_PER_LAYER + which]; }
  int64_t total() const { return off.back(); }
};

Layout make_layout(const RpT5Config& c) {
  const int64_t D = c.d_model, F = c.d_ff, inner = (int64_t)c.num_heads * c.d_kv;
  Layout l;
  int64_t o = 0;
  auto add = [&](int64_t n) {
    l.off.push_back(o);
    o += (n + 63) / 64 * 64;
  };
  add((int64_t)c.vocab_size * D);
  add((int64_t)c.rel_num_buckets * c.num_heads);
  add(D);
  for (int i = 0; i < c.num_layers; ++i) {
    add(D);
    add(inner * D);
    add(inner * D);
    add(inner * D);
    add(D * inner);
    add(D);
    add(F * D);
    add(F * D);
    add(D * F);
  }
  l.off.push_back(o);
  return l;
}

struct LayerT {  // transposed bf16 copies for the dgrad GEMMs
  bf16_t* wqkv_t;  // [D, 3 inner]   (Wqkv')^T
  bf16_t* wo_t;    // [inner, D]
  bf16_t* wi_t;    // [D, 2 F]       (Wi')^T, K in packed order
  bf16_t* wo2_t;   // [F, D]
};

}  // namespace

struct RpTrainer {
  RpEncoder* enc = nullptr;  // the forward's packed weights: also usable with rp_encode_varlen / rp_encode_padded
  Layout lay;
  std::vector<LayerT> lt;
  int32_t* bucket_of = nullptr;  // [2 maxd + 1] relative offset -> bucket
  Drop drop = {0u, 0u, 1.f};     // dropout of the next forward / backward (rp_trainer_set_dropout); thresh 0 = off
  std::vector<void*> allocs;
};

namespace {

struct TrainWs {
  // saved by the forward
  std::vector<bf16_t*> xa, xf, qkv, att, gu, ff;  // xa has L + 1 entries (xa[L] = the final hi plane)
  std::vector<float*> lse, rsa, rsf;
  bf16_t* xlo;
  float *ssp, *rs_final, *pool;
  int4 *work, *pwork;
  // backward scratch
  bf16_t *dxhi, *dxlo, *dzs, *datt, *dqkv, *dxm;
  float *delta, *rdp, *rcoef, *wpart, *dtab_part, *dln_part, *ds_seq, *dwf_seq, *norm_part, *dhead_part;
  size_t wpart_bytes;
  size_t bytes;
};

// How a wgrad GEMM [rows x cols] over nk token tiles is launched: tile configuration (0: 256 x 256, one 128-KiB
// workgroup per CU; 1: 128 x 128, two per CU) and split-K count, by a small cost model - rounds of workgroups x time of
// one workgroup's K range, plus the traffic of the fp32 partial matrices (written once, read once by the finishing
// kernel).  Deterministic in (rows, cols, nk): the same plan sizes the workspace and drives the launch.
struct WgradPlan {
  int cfg, splits;
  double t;  // modelled seconds
};
constexpr double WGRAD_CU_RATE = 1.0e15 / 256;  // sustained MFMA rate of one CU on these loops, FLOP/s
constexpr double WGRAD_PART_BW = 4.0e12;        // partial-matrix traffic, B/s
WgradPlan plan_wgrad(int rows, int cols, int nk) {
  WgradPlan best{0, 1, 1e30};
  for (int cfg = 0; cfg < 2; ++cfg) {
    const int b = cfg == 0 ? 256 : 128;
    const int slots = cfg == 0 ? 256 : 512;
    const double rate = cfg == 0 ? WGRAD_CU_RATE : WGRAD_CU_RATE * 0.7 / 2;  // per workgroup
    const int tiles = ((rows + b - 1) / b) * ((cols + b - 1) / b);
    for (int s = 1; s <= 32 && s * 4 <= std::max(nk, 4); ++s) {
      const int rounds = (tiles * s + slots - 1) / slots;
      const double t_wg = 2.0 * b * b * 64.0 * ((nk + s - 1) / s) / rate;
      const double t_part = s > 1 ? 2.0 * s * (double)rows * cols * 4 / WGRAD_PART_BW : 0.0;
      const double tt = rounds * t_wg + t_part + 3e-6;
      if (tt < best.t) best = WgradPlan{cfg, s, tt};
    }
  }
  return best;
}
// Two products over the same tokens in ONE launch of 256 x 256 tiles with a common split count (wgrad_kernel's second
// problem): the union of their tiles fills the rounds better than either alone - at the reference's training batch the two
// feed-forward gradients are 168 + 84 = 252 tiles, one round of 256 CUs with no split at all.  splits = 0: launch them
// separately (the model prefers it).  Same determinism as plan_wgrad.
WgradPlan plan_wgrad_pair(int rows0, int cols0, int rows1, int cols1, int nk) {
  const int tiles = ((rows0 + 255) / 256) * ((cols0 + 255) / 256) + ((rows1 + 255) / 256) * ((cols1 + 255) / 256);
  WgradPlan best{0, 0, plan_wgrad(rows0, cols0, nk).t + plan_wgrad(rows1, cols1, nk).t};
  for (int s = 1; s <= 32 && s * 4 <= std::max(nk, 4); ++s) {
    const int rounds = (tiles * s + 255) / 256;
    const double t_wg = 2.0 * 256 * 256 * 64.0 * ((nk + s - 1) / s) / WGRAD_CU_RATE;
    const double t_part = s > 1 ? 2.0 * s * ((double)rows0 * cols0 + (double)rows1 * cols1) * 4 / WGRAD_PART_BW : 0.0;
    const double tt = rounds * t_wg + t_part + 3e-6;
    if (tt < best.t) best = WgradPlan{0, s, tt};
  }
  return best;
}
int wgrad_splits(int rows, int cols, int nk) { return plan_wgrad(rows, cols, nk).splits; }

TrainWs carve_train(const RpTrainer* tr, int T, int batch, char* base) {
  const RpT5Config& c = tr->enc->cfg;
  const size_t Tp = align_up((size_t)T, GEMM_M_ALIGN);
  const size_t D = c.d_model, F = c.d_ff, inner = tr->enc->inner, H = c.num_heads, L = c.num_layers;
  TrainWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  w.xa.resize(L + 1);
  w.xf.resize(L); w.qkv.resize(L); w.att.resize(L); w.gu.resize(L); w.ff.resize(L);
  w.lse.resize(L); w.rsa.resize(L); w.rsf.resize(L);
  for (size_t i = 0; i <= L; ++i) w.xa[i] = (bf16_t*)take(Tp * D * 2);
  for (size_t i = 0; i < L; ++i) {
    w.xf[i] = (bf16_t*)take(Tp * D * 2);
    w.qkv[i] = (bf16_t*)take(Tp * 3 * inner * 2);
    w.att[i] = (bf16_t*)take(Tp * inner * 2);
    w.gu[i] = (bf16_t*)take(Tp * 2 * F * 2);
    w.ff[i] = (bf16_t*)take(Tp * F * 2);
    w.lse[i] = (float*)take(H * Tp * 4);
    w.rsa[i] = (float*)take(Tp * 4);
    w.rsf[i] = (float*)take(Tp * 4);
  }
  w.xlo = (bf16_t*)take(Tp * D * 2);
  w.ssp = (float*)take(Tp * ((D + 63) / 64) * 4);
  w.rs_final = (float*)take(Tp * 4);
  w.pool = (float*)take((Tp / POOL_CHUNK + (size_t)batch + 1) * D * 4);
  w.work = (int4*)take((Tp / ATT_Q + (size_t)batch + 1) * sizeof(int4));
  w.pwork = (int4*)take((Tp / POOL_CHUNK + (size_t)batch + 1) * sizeof(int4));
  w.dxhi = (bf16_t*)take(Tp * D * 2);
  w.dxlo = (bf16_t*)take(Tp * D * 2);
  w.dzs = (bf16_t*)take(Tp * 2 * F * 2);
  w.datt = (bf16_t*)take(Tp * inner * 2);
  w.dqkv = (bf16_t*)take(Tp * 3 * inner * 2);
  w.dxm = (bf16_t*)take(Tp * D * 2);  // mask * dx behind a residual-branch dropout (dropout on: else unused)
  w.delta = (float*)take(H * Tp * 4);
  w.rdp = (float*)take(((F + 63) / 64) * Tp * 4);
  w.rcoef = (float*)take(Tp * 4);
  const int nk = (int)(Tp / 64);
  size_t wp = 0;
  auto need = [&](size_t rows, size_t cols) { wp = std::max(wp, (size_t)wgrad_splits((int)rows, (int)cols, nk) * rows * cols * 4); };
  need(3 * inner, D);
  need(D, inner);
  need(2 * F, D);
  need(D, F);
  // the feed-forward pair in one launch: both partial sets live side by side
  wp = std::max(wp, (size_t)std::max(1, plan_wgrad_pair((int)(2 * F), (int)D, (int)D, (int)F, nk).splits) * (2 * F * D + D * F) * 4);
  wp = std::max(wp, (size_t)std::max(1, plan_wgrad_pair((int)(3 * inner), (int)D, (int)D, (int)inner, nk).splits) * (3 * inner * D + D * inner) * 4);
  w.wpart_bytes = wp;
  w.wpart = (float*)take(wp);
  w.dtab_part = (float*)take((Tp / ATT_Q + (size_t)batch + 1) * H * (2 * tr->enc->maxd + 1) * 4);
  w.dln_part = (float*)take(((std::max(2 * F, 3 * inner) + 31) / 32) * D * 4);  // row-block partials of d ln: wi (2F rows) / qkv (3 inner)
  w.ds_seq = (float*)take((size_t)batch * D * 4);
  w.dwf_seq = (float*)take((size_t)batch * D * 4);
  w.norm_part = (float*)take(1024 * 4);
  // rp_train_backward_hidden's partial rows of d final_ln, one per HIDDEN_BWD_ROWS token rows (last: the regions above are
  // where they were before this one existed)
  w.dhead_part = (float*)take(Tp / HIDDEN_BWD_ROWS * D * 4);
  w.bytes = off;
  return w;
}

// tile configuration of a backward dgrad GEMM: the pipelined 256 x 256 x 64 tile when it fills the chip, else 128 x 128
int bwd_variant(int n_rows_w, int K, int Tp) {
  if (K % 64 != 0) return 0;
  const int tiles = ((n_rows_w + 255) / 256) * (Tp / 256);
  return tiles >= 192 ? 26 : 0;
}

RpStatus launch_wgrad(const bf16_t* Y, int ldy, int ny, const bf16_t* X, int ldx, int nx, int Tp, int splits, float* out,
                      hipStream_t stream, int force_cfg = -1, const WgradFinish* fin = nullptr) {
  RP_REQUIRE(Tp % 64 == 0 && ny % 8 == 0 && nx % 8 == 0 && ny >= 8 && nx >= 8, "wgrad: Tp=%d ny=%d nx=%d", Tp, ny, nx);
  const int cfg = force_cfg >= 0 ? force_cfg : plan_wgrad(ny, nx, Tp / 64).cfg;
  WgradOperands a{Y, ldy, ny, X, ldx, nx, out};
  if (fin) a.fin = *fin;  // (rp_dbg_wgrad_ex: the product finishes dWi' on the pair's first product only)
  if (cfg == 1) return launch_wgrad_cfg<WgradCfg<128, 128, 2, 2, 2>>(a, nullptr, Tp / 64, splits, stream);
  return launch_wgrad_cfg<WgradCfg<256, 256, 4, 2, 2>>(a, nullptr, Tp / 64, splits, stream);
}
// two products over the same token rows in one launch of 256 x 256 tiles (plan_wgrad_pair)
RpStatus launch_wgrad_pair(const WgradOperands& a, const WgradOperands& b, int Tp, int splits, hipStream_t stream) {
  RP_REQUIRE(Tp % 64 == 0 && a.ny % 8 == 0 && a.nx % 8 == 0 && b.ny % 8 == 0 && b.nx % 8 == 0 && splits >= 1, "wgrad pair");
  return launch_wgrad_cfg<WgradCfg<256, 256, 4, 2, 2>>(a, &b, Tp / 64, splits, stream);
}

RpStatus run_unfold(const UnfoldArgs& a, hipStream_t stream) {
  ProfScope ps(stream, RP_K_BWD_OTHER);
  hipLaunchKernelGGL(unfold_kernel, dim3((a.C + 255) / 256, (a.rows + 31) / 32), dim3(256), 0, stream, a);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// ---- the memory-bound launches of the step, on raw pointers ------------------------------------------------
// The trainer and the kernel-level test entry points (rp_dbg_train_rows, rp_dbg_pool_head, rp_dbg_repack, rp_dbg_unfold) both
// launch through these: one grid rule per kernel.  No profiling scope and no launch check inside: the caller's.
void launch_embed(const int32_t* ids, const float* table, bf16_t* xhi, bf16_t* xlo, float* ssp, int np, int T, int Tp, int D,
                  int vocab, const Drop& drop, hipStream_t stream) {
  if (drop.thresh)
    hipLaunchKernelGGL(embed_train_kernel, dim3((Tp + 3) / 4), dim3(256), 0, stream, ids, table, xhi, xlo, ssp, np, T, Tp, D, vocab,
                       drop);
  else
    hipLaunchKernelGGL(embed_kernel<false>, dim3((Tp + 3) / 4), dim3(256), 0, stream, ids, table, xhi, xlo, ssp, np, T, Tp, D, vocab,
                       (const int32_t*)nullptr);
}
void launch_mask_dx(const bf16_t* dxhi, const bf16_t* dxlo, bf16_t* dxm, int rows, int D, const Drop& drop, uint32_t site,
                    hipStream_t stream) {
  hipLaunchKernelGGL(mask_dx_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, dxhi, dxlo, dxm, rows, D, drop, site);
}
void launch_rowdot_finish(const float* rdp, int np, int ld, const float* rs, float inv_d, float* rcoef, int rows,
                          hipStream_t stream) {
  hipLaunchKernelGGL(rowdot_finish_kernel, dim3((rows + 63) / 64), dim3(64), 0, stream, rdp, np, ld, rs, inv_d, rcoef, rows);
}
void launch_qkv_scale_dot(bf16_t* dqkv, const bf16_t* qkv, const float* rs, float* rcoef, int T, int rows, int width, float inv_d,
                          hipStream_t stream) {
  hipLaunchKernelGGL(qkv_scale_dot_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, dqkv, qkv, rs, rcoef, T, rows, width, inv_d);
}
void launch_embed_bwd(const int32_t* ids, int T, int vocab, const bf16_t* dxhi, const bf16_t* dxlo, int D, float* dtable,
                      const Drop& drop, hipStream_t stream) {
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(vocab, (D + 255) / 256), dim3(256), 0, stream, ids, T, vocab, dxhi, dxlo, D, dtable,
                     drop);
}
void launch_colsum(const float* part, int rows, int C, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64), dim3(64 * COLSUM_WAVES), 0, stream, part, rows, C, out);
}
void launch_bias_table(const float* rel_bias, const int32_t* bucket_of, int H, int ntab, float* tab, hipStream_t stream) {
  hipLaunchKernelGGL(bias_table_kernel, dim3((H * ntab + 255) / 256), dim3(256), 0, stream, rel_bias, bucket_of, H, ntab, tab);
}
// The training attention's three launches (the trainer and rp_dbg_attention_train): the forward with saved log-sum-exp, the two
// backward launches of one template (<0>: dQ, delta, the table gradient's partial rows; <1>: dK, dV), and the table gradient.
void launch_attention_train_fwd(dim3 grid, const bf16_t* qkv, const int4* work, const float* tab, bf16_t* att, int H, int maxd,
                                float* lse, int ld_stat, const Drop& drop, uint32_t site, hipStream_t stream) {
  if (drop.thresh)
    hipLaunchKernelGGL((attention_kernel<true, true>), grid, dim3(256), 0, stream, qkv, work, tab, att, H, maxd, lse, ld_stat, drop, site);
  else
    hipLaunchKernelGGL((attention_kernel<true, false>), grid, dim3(256), 0, stream, qkv, work, tab, att, H, maxd, lse, ld_stat, drop, site);
}
void launch_attention_bwd(dim3 grid, const bf16_t* qkv, const bf16_t* att, const bf16_t* datt, const float* lse, float* delta,
                          const int4* work, const float* tab, bf16_t* dqkv, float* dtab_part, int H, int maxd, int ld_stat,
                          int dbg_flags, const Drop& drop, uint32_t site, hipStream_t stream) {
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, qkv, att, datt, lse, delta, work, tab, dqkv, dtab_part, H, maxd, ld_stat,
                       dbg_flags, drop, site);
  };
  if (drop.thresh) {
    launch(attn_bwd_kernel<0, true>);
    launch(attn_bwd_kernel<1, true>);
  } else {
    launch(attn_bwd_kernel<0, false>);
    launch(attn_bwd_kernel<1, false>);
  }
}
void launch_bias_grad(const float* dtab_part, int nrows, int H, int ntab, const int32_t* bucket_of, int nbuckets, float* d_rel_bias,
                      hipStream_t stream) {
  hipLaunchKernelGGL(bias_grad_kernel, dim3(H), dim3(256), 0, stream, dtab_part, nrows, H, ntab, bucket_of, nbuckets, d_rel_bias);
}
// one repack_layer_kernel launch over up to four matrices: add() in order, then launch (an unused entry starts behind the
// last tile, so no workgroup selects it)
struct RepackPlan {
  RepackArgs a{};
  int count = 0, tiles = 0;
  void add(const float* s0, const float* s1, const float* s2, const float* cs, bf16_t* dst, bf16_t* dst_t, int rows, int cols,
           int n, int mode) {
    a.m[count++] = RepackMat{s0, s1, s2, cs, dst, dst_t, rows, cols, n, mode, tiles};
    tiles += (rows / 64) * (cols / 64);
  }
  void launch(hipStream_t stream) {
    for (int k = count; k < 4; ++k) a.m[k].tile0 = tiles;
    hipLaunchKernelGGL(repack_layer_kernel, dim3(tiles), dim3(256), 0, stream, a);
  }
};

// The pooling head's forward on raw pointers: the chunk sums (the inference kernel; under dropout the training one, which
// masks the final norm's output), then the per-sequence finish.  The trainer runs chunk = POOL_CHUNK, fuse = 0, bf16 lo plane.
void launch_pool_head(const bf16_t* xhi, const bf16_t* xlo, bool lo8, const float* rs, const int4* pwork, float* partial,
                      const int32_t* cu, int batch, int T, int D, int chunk, const float* w, void* out, int out_bf16, int fuse,
                      const Drop& drop, hipStream_t stream) {
  const dim3 pg(T / chunk + batch);
  if (!drop.thresh)
    launch_pool_partial(pg, stream, xhi, xlo, rs, pwork, partial, D, chunk, w, out, out_bf16, fuse, lo8);
  else if (D <= 3 * 512)
    hipLaunchKernelGGL(pool_partial_train_kernel<3>, pg, dim3(256), 0, stream, xhi, xlo, rs, pwork, partial, D, drop);
  else
    hipLaunchKernelGGL(pool_partial_train_kernel<4>, pg, dim3(256), 0, stream, xhi, xlo, rs, pwork, partial, D, drop);
  launch_pool_finish(batch, stream, partial, w, cu, out, out_bf16, D, chunk, fuse);
}
// ... and its backward: per sequence ds / dwf from the forward's chunk sums, d final_layer_norm.weight = the column sums of
// dwf, then per token the two planes of the residual gradient
void launch_pool_bwd_head(const bf16_t* xhi, const bf16_t* xlo, const float* rs, const int4* pwork, const float* partial,
                          const float* w, const int32_t* cu, int batch, int T, int D, const float* d_emb, float* ds, float* dwf,
                          float* d_final_ln, bf16_t* dxhi, bf16_t* dxlo, const Drop& drop, hipStream_t stream) {
  const float inv_d = 1.f / (float)D;
  hipLaunchKernelGGL(pool_bwd_seq_kernel, dim3(batch), dim3(256), 0, stream, partial, w, cu, d_emb, ds, dwf, D);
  launch_colsum(dwf, batch, D, d_final_ln, stream);
  const dim3 pg(T / POOL_CHUNK + batch);
  if (D <= 3 * 512)
    hipLaunchKernelGGL(pool_bwd_tok_kernel<3>, pg, dim3(256), 0, stream, xhi, xlo, rs, pwork, (const float*)ds, dxhi, dxlo, D, inv_d,
                       drop);
  else
    hipLaunchKernelGGL(pool_bwd_tok_kernel<4>, pg, dim3(256), 0, stream, xhi, xlo, rs, pwork, (const float*)ds, dxhi, dxlo, D, inv_d,
                       drop);
}

// ---- forward with saved activations -----------------------------------------------------------------------
// The shared body of rp_train_forward and rp_train_forward_hidden: embedding, every layer, the final RMSNorm's row
// statistic.  Leaves the final residual stream in xa[L] + xlo and rs_final; the entry point's head follows.
RpStatus forward_layers(RpTrainer* tr, const int32_t* ids, const int32_t* cu, int batch, int T, const TrainWs& w,
                        hipStream_t stream) {
  RpEncoder* e = tr->enc;
  const RpT5Config& c = e->cfg;
  const int D = c.d_model, F = c.d_ff, inner = e->inner, H = c.num_heads, L = c.num_layers;
  const int Tp = (int)align_up((size_t)T, GEMM_M_ALIGN);
  const int np = (D + 63) / 64;
  RpStatus st;
  auto rowscale = [&](float* rs) {
    ProfScope ps(stream, RP_K_RMSNORM);
    launch_rowscale_kernel(w.ssp, rs, Tp, np, 1.f / (float)D, c.layer_norm_eps, stream);
  };
  const Drop drop = tr->drop;
  {
    ProfScope ps(stream, RP_K_EMBED);
    launch_embed(ids, (const float*)e->embed, w.xa[0], w.xlo, w.ssp, np, T, Tp, D, c.vocab_size, drop, stream);
  }
  const dim3 att_grid(H, T / ATT_Q + batch);
  launch_worklist(cu, batch, w.work, (int)att_grid.y, w.pwork, T / POOL_CHUNK + batch, POOL_CHUNK, stream);
  RP_CHECK_LAUNCH();
  for (int i = 0; i < L; ++i) {
    const LayerPacked& Lw = e->layers[i];
    const uint32_t site = DROP_SITE_LAYER0 + 8u * (uint32_t)i;  // + {0 probs, 1 attention residual, 2 FFN inner, 3 FFN residual}
    rowscale(w.rsa[i]);
    if ((st = launch_gemm(w.xa[i], D, Tp, Lw.wqkv, D, 3 * inner, D,
                          EpiStoreBf16{w.qkv[i], 3 * inner, 3 * inner, RowScale{w.rsa[i]}}, stream, RP_K_GEMM_QKV)))
      return st;
    {
      ProfScope ps(stream, RP_K_ATTENTION);
      launch_attention_train_fwd(att_grid, (const bf16_t*)w.qkv[i], (const int4*)w.work, (const float*)e->bias_tab, w.att[i], H,
                                 e->maxd, w.lse[i], Tp, drop, site, stream);
    }
    // rows T .. Tp of every saved activation must stay finite: they are K rows of the wgrad GEMMs (against zero dY rows)
    if (Tp > T) RP_HIP(hipMemsetAsync(w.att[i] + (size_t)T * inner, 0, (size_t)(Tp - T) * inner * 2, stream));
    if ((st = launch_gemm(w.att[i], inner, Tp, Lw.wo, inner, D, inner,
                          EpiResidT<true>{w.xf[i], w.xlo, D, D, w.ssp, np, Tp, w.xa[i], drop, site + 1}, stream, RP_K_GEMM_O)))
      return st;
    rowscale(w.rsf[i]);
    const EpiStoreBf16 gu_store{w.gu[i], 2 * F, 2 * F, RowScale{w.rsf[i]}};
    st = drop.thresh ? launch_gemm(w.xf[i], D, Tp, Lw.wi, D, 2 * F, D,
                                   EpiGegluTrainT<true>{gu_store, w.ff[i], F, 2 * F, RowScale{w.rsf[i]}, drop, site + 2}, stream,
                                   RP_K_GEMM_WI)
                     : launch_gemm(w.xf[i], D, Tp, Lw.wi, D, 2 * F, D,
                                   EpiGegluTrainT<false>{gu_store, w.ff[i], F, 2 * F, RowScale{w.rsf[i]}, drop, site + 2}, stream,
                                   RP_K_GEMM_WI);
    if (st) return st;
    if ((st = launch_gemm(w.ff[i], F, Tp, Lw.wo2, F, D, F,
                          EpiResidT<true>{w.xa[i + 1], w.xlo, D, D, w.ssp, np, Tp, w.xf[i], drop, site + 3}, stream, RP_K_GEMM_WO)))
      return st;
  }
  rowscale(w.rs_final);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// head of rp_train_forward: final RMSNorm + mean pooling + normalisation -> out_emb [batch, D]
RpStatus pool_head(RpTrainer* tr, const int32_t* cu, int batch, int T, float* out_emb, const TrainWs& w, hipStream_t stream) {
  RpEncoder* e = tr->enc;
  const int D = e->cfg.d_model, L = e->cfg.num_layers;
  const Drop drop = tr->drop;
  {
    ProfScope ps(stream, RP_K_POOL);
    launch_pool_head(w.xa[L], w.xlo, false, w.rs_final, (const int4*)w.pwork, w.pool, cu, batch, T, D, POOL_CHUNK,
                     (const float*)e->final_ln, (void*)out_emb, 0, 0 /* the backward reads every chunk's sums from `pool` */, drop,
                     stream);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// head of rp_train_forward_hidden: the final RMSNorm's rows, last_hidden_state [T, D] bf16 (on raw pointers: the trainer
// and the rp_dbg_hidden_head test entry both launch through here)
// drop (thresh 0 = off): the final site's mask, rp_train_forward_hidden_dropout alone
RpStatus launch_hidden_head(const bf16_t* xhi, const bf16_t* xlo, const float* rs, const float* ln, bf16_t* out_hidden, int T,
                            int D, hipStream_t stream, const Drop& drop = Drop{0u, 0u, 1.f}) {
  ProfScope ps(stream, RP_K_HIDDEN_HEAD);
  const dim3 grid((T + HIDDEN_ROWS - 1) / HIDDEN_ROWS);
  if (drop.thresh)
    hipLaunchKernelGGL(hidden_head_kernel<true>, grid, dim3(256), 0, stream, xhi, xlo, rs, ln, out_hidden, T, D, drop);
  else
    hipLaunchKernelGGL(hidden_head_kernel<false>, grid, dim3(256), 0, stream, xhi, xlo, rs, ln, out_hidden, T, D, drop);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
RpStatus hidden_head(RpTrainer* tr, int T, bf16_t* out_hidden, const TrainWs& w, hipStream_t stream) {
  RpEncoder* e = tr->enc;
  return launch_hidden_head((const bf16_t*)w.xa[e->cfg.num_layers], (const bf16_t*)w.xlo, (const float*)w.rs_final,
                            (const float*)e->final_ln, out_hidden, T, e->cfg.d_model, stream, tr->drop);
}

// ---- backward ---------------------------------------------------------------------------------------------
// The residual gradient starts as zero planes (rows T .. Tp stay zero: they are K rows of the wgrad GEMMs) and the
// bias-table partials as zeros; then the entry point's head writes d loss / d x of the final residual stream and
// final_layer_norm.weight's gradient, and backward_layers does the rest.
RpStatus backward_zero(RpTrainer* tr, int batch, int T, const TrainWs& w, hipStream_t stream) {
  const RpT5Config& c = tr->enc->cfg;
  const int Tp = (int)align_up((size_t)T, GEMM_M_ALIGN);
  const size_t att_rows = (size_t)(T / ATT_Q + batch), ntab = 2 * tr->enc->maxd + 1;
  RP_HIP(hipMemsetAsync(w.dxhi, 0, (size_t)Tp * c.d_model * 2, stream));
  RP_HIP(hipMemsetAsync(w.dxlo, 0, (size_t)Tp * c.d_model * 2, stream));
  RP_HIP(hipMemsetAsync(w.dtab_part, 0, att_rows * c.num_heads * ntab * 4, stream));
  return RP_OK;
}

// head of rp_train_backward: normalisation + mean pooling + final RMSNorm, from d loss / d embedding [batch, D]
RpStatus pool_bwd_head(RpTrainer* tr, const int32_t* cu, int batch, int T, const float* d_emb, float* grads, const TrainWs& w,
                       hipStream_t stream) {
  RpEncoder* e = tr->enc;
  const int D = e->cfg.d_model, L = e->cfg.num_layers;
  ProfScope ps(stream, RP_K_BWD_OTHER);
  launch_pool_bwd_head((const bf16_t*)w.xa[L], (const bf16_t*)w.xlo, (const float*)w.rs_final, (const int4*)w.pwork,
                       (const float*)w.pool, (const float*)e->final_ln, cu, batch, T, D, d_emb, w.ds_seq, w.dwf_seq,
                       grads + tr->lay.final_ln(), w.dxhi, w.dxlo, tr->drop, stream);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// head of rp_train_backward_hidden: the final RMSNorm alone, from d loss / d last_hidden_state [T, D] fp32.  The partial
// rows of final_layer_norm.weight's gradient, one per workgroup, go through dhead_part to colsum_kernel.
// (on raw pointers, as launch_hidden_head; dhead_part: ceil(T / HIDDEN_BWD_ROWS) rows of D floats)
RpStatus launch_hidden_bwd_head(const bf16_t* xhi, const bf16_t* xlo, const float* rs, const float* ln, const float* d_hidden,
                                bf16_t* dxhi, bf16_t* dxlo, float* dhead_part, float* dln, int T, int D, hipStream_t stream,
                                const Drop& drop = Drop{0u, 0u, 1.f}) {
  const float inv_d = 1.f / (float)D;
  const int nblk = (T + HIDDEN_BWD_ROWS - 1) / HIDDEN_BWD_ROWS;
  {
    ProfScope ps(stream, RP_K_BWD_HIDDEN_HEAD);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), 0, stream, xhi, xlo, rs, ln, d_hidden, dxhi, dxlo, dhead_part, T, D, inv_d,
                         drop);
    };
    if (D <= 3 * 512)
      drop.thresh ? launch(hidden_head_bwd_kernel<3, true>) : launch(hidden_head_bwd_kernel<3, false>);
    else
      drop.thresh ? launch(hidden_head_bwd_kernel<4, true>) : launch(hidden_head_bwd_kernel<4, false>);
  }
  ProfScope ps(stream, RP_K_BWD_OTHER);
  launch_colsum(dhead_part, nblk, D, dln, stream);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
RpStatus hidden_bwd_head(RpTrainer* tr, int T, const float* d_hidden, float* grads, const TrainWs& w, hipStream_t stream) {
  RpEncoder* e = tr->enc;
  return launch_hidden_bwd_head((const bf16_t*)w.xa[e->cfg.num_layers], (const bf16_t*)w.xlo, (const float*)w.rs_final,
                                (const float*)e->final_ln, d_hidden, w.dxhi, w.dxlo, w.dhead_part, grads + tr->lay.final_ln(), T,
                                e->cfg.d_model, stream, tr->drop);
}

// The shared body of rp_train_backward and rp_train_backward_hidden: from the residual gradient of the final stream
// (dxhi + dxlo) through every layer to the embedding scatter and the bias table.
RpStatus backward_layers(RpTrainer* tr, const float* params, const int32_t* ids, int batch, int T, float* grads,
                         const TrainWs& w, hipStream_t stream) {
  RpEncoder* e = tr->enc;
  const RpT5Config& c = e->cfg;
  const Layout& lay = tr->lay;
  const int D = c.d_model, F = c.d_ff, inner = e->inner, H = c.num_heads, L = c.num_layers;
  const int Tp = (int)align_up((size_t)T, GEMM_M_ALIGN);
  const int nk = Tp / 64, ntab = 2 * e->maxd + 1;
  const float inv_d = 1.f / (float)D;
  RpStatus st;
  const Drop drop = tr->drop;
  const dim3 att_grid(H, T / ATT_Q + batch);
  // Behind a residual-branch dropout the branch sees mask * dx: one bf16 copy (dxm), the operand of its dgrad and wgrad
  // GEMMs.  The first branch's copy is a pass of its own (mask_first, behind the pooling backward); every later one is
  // written by the RMSNorm-backward epilogue that produces the gradient it masks (EpiRmsBwdResidT<true>, next_site).
  const bf16_t* const dxb = drop.thresh ? (const bf16_t*)w.dxm : (const bf16_t*)w.dxhi;
  auto mask_first = [&](uint32_t site) {
    if (!drop.thresh) return;
    ProfScope ps(stream, RP_K_BWD_OTHER);
    launch_mask_dx((const bf16_t*)w.dxhi, (const bf16_t*)w.dxlo, w.dxm, Tp, D, drop, site, stream);
  };
  // dx += A W - x rcoef (RMSNorm backward in the epilogue), and dxm for the branch whose backward comes next (0 = none)
  auto rms_bwd_gemm = [&](const bf16_t* A, int K, const bf16_t* Wt, const bf16_t* x_saved, uint32_t next_site) -> RpStatus {
    if (drop.thresh && next_site)
      return launch_gemm(A, K, Tp, Wt, K, D, K,
                         EpiRmsBwdResidT<true>{w.dxhi, w.dxlo, D, D, x_saved, w.rcoef, w.dxm, drop, next_site}, stream,
                         RP_K_BWD_DGRAD, 0, nullptr, bwd_variant(D, K, Tp));
    return launch_gemm(A, K, Tp, Wt, K, D, K, EpiRmsBwdResid{w.dxhi, w.dxlo, D, D, x_saved, w.rcoef}, stream, RP_K_BWD_DGRAD, 0,
                       nullptr, bwd_variant(D, K, Tp));
  };
  mask_first(DROP_SITE_LAYER0 + 8u * (uint32_t)(L - 1) + 3);
  for (int i = L - 1; i >= 0; --i) {
    const LayerT& Lt = tr->lt[i];
    const uint32_t site = DROP_SITE_LAYER0 + 8u * (uint32_t)i;
    // ---------------- feed-forward sub-layer:  x_out = x + ff Wo2^T,  ff = gelu(g) u,  [g | u] = rs (x Wi'^T)
    // dWo2 = dx^T ff  (dx: the hi plane of the residual gradient; mask * dx under dropout)
    const WgradPlan pair = (g_train_wgrad_form & 1) ? WgradPlan{0, 0, 0.0} : plan_wgrad_pair(2 * F, D, D, F, nk);
    auto wo_unfold = [&](int S) -> RpStatus {
      if (S == 1) return RP_OK;
      UnfoldArgs a{};
      a.part = w.wpart + (pair.splits ? (size_t)S * 2 * F * D : 0); a.split_stride = (size_t)D * F; a.splits = S; a.rows = D; a.C = F;
      a.mode = UNFOLD_PLAIN; a.g0 = grads + lay.layer(i, P_WO);
      return run_unfold(a, stream);
    };
    if (!pair.splits) {
      const int S = wgrad_splits(D, F, nk);
      if ((st = launch_wgrad(dxb, D, D, w.ff[i], F, F, Tp, S, S == 1 ? grads + lay.layer(i, P_WO) : w.wpart, stream))) return st;
      if ((st = wo_unfold(S))) return st;
    }
    // dff = dx Wo2 -> gated-GELU backward -> dzs = rs [dg | du] (packed order), row dots
    if ((st = launch_gemm(dxb, D, Tp, Lt.wo2_t, D, F, D,
                          EpiGegluBwd{w.gu[i], w.dzs, 2 * F, F, w.rsf[i], w.rdp, (F + 63) / 64, Tp, drop, site + 2}, stream,
                          RP_K_BWD_DGRAD, 0,
                          nullptr, bwd_variant(F, D, Tp))))
      return st;
    {
      ProfScope ps(stream, RP_K_BWD_OTHER);
      launch_rowdot_finish((const float*)w.rdp, (F + 63) / 64, Tp, (const float*)w.rsf[i], inv_d, w.rcoef, Tp, stream);
    }
    // dWi' = dzs^T x  -> unfold (de-interleave gate / up, x ln_ff, d ln_ff); with the pair plan dWo2 rides in the same launch
    // (dxb is still the branch's masked gradient: the epilogue that overwrites it comes below)
    {
      const int S = pair.splits ? pair.splits : wgrad_splits(2 * F, D, nk);
      // split-free pair: the epilogue finishes dWi' itself (WgradFinish: no partial matrix, no unfold pass); bit 1 of
      // train_wgrad_form keeps the separate pass
      const bool finish_in_epilogue = pair.splits == 1 && (2 * F) % 64 == 0 && !(g_train_wgrad_form & 2);
      if (pair.splits) {
        WgradOperands wi_ops{w.dzs, 2 * F, 2 * F, w.xf[i], D, D, w.wpart};
        if (finish_in_epilogue) {
          wi_ops.out = grads + lay.layer(i, P_WI0);
          wi_ops.fin = WgradFinish{1, grads + lay.layer(i, P_WI1), params + lay.layer(i, P_WI0), params + lay.layer(i, P_WI1),
                                   params + lay.layer(i, P_LN_FF), w.dln_part};
        }
        const WgradOperands wo_ops{dxb, D, D, w.ff[i], F, F, S == 1 ? grads + lay.layer(i, P_WO) : w.wpart + (size_t)S * 2 * F * D};
        if ((st = launch_wgrad_pair(wi_ops, wo_ops, Tp, S, stream))) return st;
        if ((st = wo_unfold(S))) return st;
      } else if ((st = launch_wgrad(w.dzs, 2 * F, 2 * F, w.xf[i], D, D, Tp, S, w.wpart, stream))) {
        return st;
      }
      if (!finish_in_epilogue) {
        UnfoldArgs a{};
        a.part = w.wpart; a.split_stride = (size_t)2 * F * D; a.splits = S; a.rows = 2 * F; a.C = D; a.mode = UNFOLD_GEGLU;
        a.g0 = grads + lay.layer(i, P_WI0); a.g1 = grads + lay.layer(i, P_WI1);
        a.w0 = params + lay.layer(i, P_WI0); a.w1 = params + lay.layer(i, P_WI1);
        a.ln = params + lay.layer(i, P_LN_FF); a.dln_part = w.dln_part;
        if ((st = run_unfold(a, stream))) return st;
      }
      ProfScope ps(stream, RP_K_BWD_OTHER);
      launch_colsum((const float*)w.dln_part, (2 * F + 31) / 32, D, grads + lay.layer(i, P_LN_FF), stream);
    }
    // dx += dzs Wi' - x rcoef   (RMSNorm backward in the epilogue)
    if ((st = rms_bwd_gemm(w.dzs, 2 * F, Lt.wi_t, w.xf[i], site + 1))) return st;

    // ---------------- attention sub-layer:  x_out = x + att Wo^T,  att = Attn(q, k, v),  [q | k | v] = rs (x Wqkv'^T)
    // the two weight gradients of the sub-layer (dWo = dx^T att, dWqkv' = dzs^T x) as one launch when the model prefers it
    // (30 + 12 tiles: a common split count fills the round)
    const WgradPlan apair = (g_train_wgrad_form & 1) ? WgradPlan{0, 0, 0.0} : plan_wgrad_pair(3 * inner, D, D, inner, nk);
    auto o_unfold = [&](int S) -> RpStatus {
      if (S == 1) return RP_OK;
      UnfoldArgs a{};
      a.part = w.wpart + (apair.splits ? (size_t)S * 3 * inner * D : 0); a.split_stride = (size_t)D * inner; a.splits = S; a.rows = D;
      a.C = inner; a.mode = UNFOLD_PLAIN; a.g0 = grads + lay.layer(i, P_O);
      return run_unfold(a, stream);
    };
    if (!apair.splits) {
      const int S = wgrad_splits(D, inner, nk);
      if ((st = launch_wgrad(dxb, D, D, w.att[i], inner, inner, Tp, S, S == 1 ? grads + lay.layer(i, P_O) : w.wpart, stream))) return st;
      if ((st = o_unfold(S))) return st;
    }
    if ((st = launch_gemm(dxb, D, Tp, Lt.wo_t, D, inner, D, EpiStoreBf16{w.datt, inner, inner, RowScale{nullptr}}, stream,
                          RP_K_BWD_DGRAD, 0, nullptr, bwd_variant(inner, D, Tp))))
      return st;
    {
      ProfScope ps(stream, RP_K_BWD_ATTENTION);
      launch_attention_bwd(att_grid, (const bf16_t*)w.qkv[i], (const bf16_t*)w.att[i], (const bf16_t*)w.datt, (const float*)w.lse[i],
                           w.delta, (const int4*)w.work, (const float*)e->bias_tab, w.dqkv, w.dtab_part, H, e->maxd, Tp, g_train_dbg,
                           drop, site, stream);
      RP_CHECK_LAUNCH();
    }
    {
      ProfScope ps(stream, RP_K_BWD_OTHER);
      launch_qkv_scale_dot(w.dqkv, (const bf16_t*)w.qkv[i], (const float*)w.rsa[i], w.rcoef, T, Tp, 3 * inner, inv_d, stream);
    }
    {
      const int S = apair.splits ? apair.splits : wgrad_splits(3 * inner, D, nk);
      if (apair.splits) {
        const WgradOperands qkv_ops{w.dqkv, 3 * inner, 3 * inner, w.xa[i], D, D, w.wpart};
        const WgradOperands o_ops{dxb, D, D, w.att[i], inner, inner,
                                  S == 1 ? grads + lay.layer(i, P_O) : w.wpart + (size_t)S * 3 * inner * D};
        if ((st = launch_wgrad_pair(qkv_ops, o_ops, Tp, S, stream))) return st;
        if ((st = o_unfold(S))) return st;
      } else if ((st = launch_wgrad(w.dqkv, 3 * inner, 3 * inner, w.xa[i], D, D, Tp, S, w.wpart, stream))) {
        return st;
      }
      UnfoldArgs a{};
      a.part = w.wpart; a.split_stride = (size_t)3 * inner * D; a.splits = S; a.rows = 3 * inner; a.C = D; a.mode = UNFOLD_QKV;
      a.n = inner;
      a.g0 = grads + lay.layer(i, P_Q); a.g1 = grads + lay.layer(i, P_K); a.g2 = grads + lay.layer(i, P_V);
      a.w0 = params + lay.layer(i, P_Q); a.w1 = params + lay.layer(i, P_K); a.w2 = params + lay.layer(i, P_V);
      a.ln = params + lay.layer(i, P_LN_ATTN); a.dln_part = w.dln_part;
      if ((st = run_unfold(a, stream))) return st;
      ProfScope ps(stream, RP_K_BWD_OTHER);
      launch_colsum((const float*)w.dln_part, (3 * inner + 31) / 32, D, grads + lay.layer(i, P_LN_ATTN), stream);
    }
    if ((st = rms_bwd_gemm(w.dqkv, 3 * inner, Lt.wqkv_t, w.xa[i], i > 0 ? site - 8u + 3u : 0u))) return st;
  }
  {
    ProfScope ps(stream, RP_K_BWD_OTHER);
    launch_embed_bwd(ids, T, c.vocab_size, (const bf16_t*)w.dxhi, (const bf16_t*)w.dxlo, D, grads + lay.embed(), drop, stream);
    launch_bias_grad((const float*)w.dtab_part, (int)att_grid.y, H, ntab, (const int32_t*)tr->bucket_of, c.rel_num_buckets,
                     grads + lay.rel_bias(), stream);
    RP_CHECK_LAUNCH();
  }
  return RP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
extern "C" int32_t rp_train_param_tensors(const RpT5Config* cfg) {
  return cfg ? N_GLOBAL + N_PER_LAYER * cfg->num_layers : 0;
}

extern "C" RpStatus rp_train_param_layout(const RpT5Config* cfg, int64_t* offsets) {
  RP_REQUIRE(cfg && offsets, "null argument");
  const Layout l = make_layout(*cfg);
  for (size_t i = 0; i < l.off.size(); ++i) offsets[i] = l.off[i];
  return RP_OK;
}

extern "C" void rp_trainer_destroy(RpTrainer* tr) {
  if (!tr) return;
  for (void* p : tr->allocs) (void)hipFree(p);
  if (tr->enc) rp_encoder_destroy(tr->enc);
  delete tr;
}

extern "C" RpStatus rp_trainer_create(const RpT5Config* cfg, const float* params, RpTrainer** out) {
  RP_REQUIRE(cfg && params && out, "null argument");
  RP_REQUIRE(cfg->d_model % 64 == 0 && cfg->d_ff % 64 == 0, "training kernels need d_model=%d and d_ff=%d to be multiples of 64",
             cfg->d_model, cfg->d_ff);
  RpTrainer* tr = new RpTrainer();
  tr->lay = make_layout(*cfg);
  // the inference encoder on the same weights (HF-layout pointers into the flat buffer)
  std::vector<RpT5LayerWeights> lw(cfg->num_layers);
  for (int i = 0; i < cfg->num_layers; ++i) {
    lw[i].ln_attn = params + tr->lay.layer(i, P_LN_ATTN);
    lw[i].q = params + tr->lay.layer(i, P_Q);
    lw[i].k = params + tr->lay.layer(i, P_K);
    lw[i].v = params + tr->lay.layer(i, P_V);
    lw[i].o = params + tr->lay.layer(i, P_O);
    lw[i].ln_ff = params + tr->lay.layer(i, P_LN_FF);
    lw[i].wi_0 = params + tr->lay.layer(i, P_WI0);
    lw[i].wi_1 = params + tr->lay.layer(i, P_WI1);
    lw[i].wo = params + tr->lay.layer(i, P_WO);
  }
  RpT5Weights wts{params + tr->lay.embed(), params + tr->lay.rel_bias(), params + tr->lay.final_ln(), lw.data()};
  RpStatus st = rp_encoder_create(cfg, &wts, RP_DT_F32, &tr->enc);
  if (st != RP_OK) {
    delete tr;
    return st;
  }
  const int D = cfg->d_model, F = cfg->d_ff, inner = tr->enc->inner;
  auto alloc = [&](size_t bytes, void** p) -> RpStatus {
    RP_HIP(hipMalloc(p, bytes));
    tr->allocs.push_back(*p);
    return RP_OK;
  };
  tr->lt.resize(cfg->num_layers);
  for (int i = 0; i < cfg->num_layers && st == RP_OK; ++i) {
    LayerT& t = tr->lt[i];
    if ((st = alloc((size_t)3 * inner * D * 2, (void**)&t.wqkv_t))) break;
    if ((st = alloc((size_t)D * inner * 2, (void**)&t.wo_t))) break;
    if ((st = alloc((size_t)2 * F * D * 2, (void**)&t.wi_t))) break;
    if ((st = alloc((size_t)D * F * 2, (void**)&t.wo2_t))) break;
  }
  const int ntab = 2 * tr->enc->maxd + 1;
  if (st == RP_OK) st = alloc((size_t)ntab * 4, (void**)&tr->bucket_of);
  if (st == RP_OK) {
    std::vector<int32_t> bk(ntab);
    for (int o = 0; o < ntab; ++o)
      bk[o] = rp_relative_position_bucket(o - tr->enc->maxd, cfg->rel_num_buckets, cfg->rel_max_distance);
    if (hipMemcpy(tr->bucket_of, bk.data(), (size_t)ntab * 4, hipMemcpyHostToDevice) != hipSuccess)
      st = fail(RP_E_HIP, "hipMemcpy of the bucket map failed");
  }
  if (st == RP_OK) st = rp_trainer_load_params(tr, params, nullptr);
  if (st == RP_OK && hipDeviceSynchronize() != hipSuccess) st = fail(RP_E_HIP, "hipDeviceSynchronize failed");
  if (st != RP_OK) {
    rp_trainer_destroy(tr);
    return st;
  }
  *out = tr;
  return RP_OK;
}

extern "C" RpEncoder* rp_trainer_encoder(RpTrainer* tr) { return tr ? tr->enc : nullptr; }

extern "C" RpStatus rp_trainer_set_dropout(RpTrainer* tr, float p, uint32_t seed) {
  RP_REQUIRE(tr && p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  tr->drop = make_drop(p, seed);
  return RP_OK;
}

extern "C" RpStatus rp_dbg_dropout_mask(float p, uint32_t seed, uint32_t site, uint32_t row0, uint32_t col0, int32_t rows,
                                        int32_t cols, uint8_t* out, void* stream_) {
  RP_REQUIRE(out && rows > 0 && cols > 0 && p > 0.f && p < 1.f, "bad argument");
  const Drop d = make_drop(p, seed);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, (hipStream_t)stream_, d, site, row0, col0,
                     rows, cols, out);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// Refresh every bf16 compute copy from the fp32 masters (after an optimizer step): the forward's packed weights, the
// embedding / norm / bias tables, and the transposed copies of the dgrad GEMMs.  Launch-only.
extern "C" RpStatus rp_trainer_load_params(RpTrainer* tr, const float* params, void* stream_) {
  RP_REQUIRE(tr && params, "null argument");
  hipStream_t stream = (hipStream_t)stream_;
  RpEncoder* e = tr->enc;
  const RpT5Config& c = e->cfg;
  const Layout& lay = tr->lay;
  const int D = c.d_model, F = c.d_ff, inner = e->inner, H = c.num_heads;
  ProfScope ps(stream, RP_K_OPTIMIZER);
  RP_HIP(hipMemcpyAsync(e->embed, params + lay.embed(), (size_t)c.vocab_size * D * 4, hipMemcpyDeviceToDevice, stream));
  embed_table_x24(e, stream);  // the inference pass's pre-encoded copy of the table follows the masters
  RP_HIP(hipMemcpyAsync(e->final_ln, params + lay.final_ln(), (size_t)D * 4, hipMemcpyDeviceToDevice, stream));
  const int ntab = 2 * e->maxd + 1;
  launch_bias_table(params + lay.rel_bias(), (const int32_t*)tr->bucket_of, H, ntab, e->bias_tab, stream);
  for (int i = 0; i < c.num_layers; ++i) {
    LayerPacked& L = e->layers[i];
    const LayerT& t = tr->lt[i];
    const float* ln_a = params + lay.layer(i, P_LN_ATTN);
    const float* ln_f = params + lay.layer(i, P_LN_FF);
    RepackPlan plan;
    plan.add(params + lay.layer(i, P_Q), params + lay.layer(i, P_K), params + lay.layer(i, P_V), ln_a, L.wqkv, t.wqkv_t,
             3 * inner, D, inner, (int)PACK_CONCAT3);
    plan.add(params + lay.layer(i, P_O), nullptr, nullptr, nullptr, L.wo, t.wo_t, D, inner, 0, (int)PACK_COPY);
    plan.add(params + lay.layer(i, P_WI0), params + lay.layer(i, P_WI1), nullptr, ln_f, L.wi, t.wi_t, 2 * F, D, 0,
             (int)PACK_GEGLU);
    plan.add(params + lay.layer(i, P_WO), nullptr, nullptr, nullptr, L.wo2, t.wo2_t, D, F, 0, (int)PACK_COPY);
    plan.launch(stream);
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" size_t rp_train_workspace_bytes(const RpTrainer* tr, int32_t total_tokens, int32_t batch) {
  if (!tr || total_tokens <= 0 || batch <= 0) return 0;
  return carve_train(tr, total_tokens, batch, nullptr).bytes;
}

// argument checks and the workspace carve shared by the four forward / backward entry points
static RpStatus train_entry(RpTrainer* tr, int32_t batch, int32_t T, void* workspace, size_t workspace_bytes, TrainWs* w) {
  RP_REQUIRE(batch > 0 && T > 0, "batch=%d total_tokens=%d", batch, T);
  *w = carve_train(tr, T, batch, (char*)workspace);
  if (!workspace || workspace_bytes < w->bytes)
    return fail(RP_E_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, w->bytes);
  return RP_OK;
}
// the plain hidden entry points run without dropout only: what follows them must drop too (rp_decoder_loss_grad_dropout), or
// the model is half-dropped, neither the reference's training mode nor its eval mode; the _dropout pair is the opt-in
static RpStatus hidden_entry(const RpTrainer* tr, const char* what, bool dropout_ok) {
  RP_REQUIRE(dropout_ok || !tr->drop.thresh,
             "%s: dropout is set (rp_trainer_set_dropout p > 0); this entry point takes p = 0 only, %s_dropout honours it", what,
             what);
  RP_REQUIRE(tr->enc->cfg.d_model <= 4 * 512, "%s: d_model=%d > 2048", what, tr->enc->cfg.d_model);
  return RP_OK;
}

extern "C" RpStatus rp_train_forward(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch, int32_t T,
                                     float* out_emb, void* workspace, size_t workspace_bytes, void* stream_) {
  RP_REQUIRE(tr && ids && cu_seqlens && out_emb, "null argument");
  TrainWs w;
  RpStatus st;
  if ((st = train_entry(tr, batch, T, workspace, workspace_bytes, &w))) return st;
  if ((st = forward_layers(tr, ids, cu_seqlens, batch, T, w, (hipStream_t)stream_))) return st;
  return pool_head(tr, cu_seqlens, batch, T, out_emb, w, (hipStream_t)stream_);
}

extern "C" RpStatus rp_train_backward(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens,
                                      int32_t batch, int32_t T, const float* d_emb, float* grads, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  RP_REQUIRE(tr && params && ids && cu_seqlens && d_emb && grads, "null argument");
  TrainWs w;
  RpStatus st;
  if ((st = train_entry(tr, batch, T, workspace, workspace_bytes, &w))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  if ((st = backward_zero(tr, batch, T, w, stream))) return st;
  if ((st = pool_bwd_head(tr, cu_seqlens, batch, T, d_emb, grads, w, stream))) return st;
  return backward_layers(tr, params, ids, batch, T, grads, w, stream);
}

// The sequence lengths are read on the device only (worklist_kernel); an empty sequence is refused here, where the pooled
// pair divides by its length.  cu_seqlens is a device array: one small copy, made before anything is launched.
static RpStatus check_no_empty_sequence(const int32_t* cu_dev, int32_t batch, int32_t T, hipStream_t stream) {
  std::vector<int32_t> cu((size_t)batch + 1);
  RP_HIP(hipMemcpyAsync(cu.data(), cu_dev, cu.size() * 4, hipMemcpyDeviceToHost, stream));
  RP_HIP(hipStreamSynchronize(stream));
  RP_REQUIRE(cu[0] == 0 && cu[batch] == T, "cu_seqlens runs %d .. %d for total_tokens=%d", cu[0], cu[batch], T);
  for (int b = 0; b < batch; ++b) RP_REQUIRE(cu[b + 1] > cu[b], "sequence %d is empty (cu_seqlens %d, %d)", b, cu[b], cu[b + 1]);
  return RP_OK;
}

static RpStatus forward_hidden(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch, int32_t T,
                               void* out_hidden_bf16, void* workspace, size_t workspace_bytes, void* stream_, bool dropout_ok) {
  RP_REQUIRE(tr && ids && cu_seqlens && out_hidden_bf16, "null argument");
  TrainWs w;
  RpStatus st;
  if ((st = hidden_entry(tr, "rp_train_forward_hidden", dropout_ok))) return st;
  if ((st = train_entry(tr, batch, T, workspace, workspace_bytes, &w))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  if ((st = check_no_empty_sequence(cu_seqlens, batch, T, stream))) return st;
  if ((st = forward_layers(tr, ids, cu_seqlens, batch, T, w, stream))) return st;
  return hidden_head(tr, T, (bf16_t*)out_hidden_bf16, w, stream);
}

extern "C" RpStatus rp_train_forward_hidden(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                                            int32_t T, void* out_hidden_bf16, void* workspace, size_t workspace_bytes,
                                            void* stream_) {
  return forward_hidden(tr, ids, cu_seqlens, batch, T, out_hidden_bf16, workspace, workspace_bytes, stream_, false);
}
extern "C" RpStatus rp_train_forward_hidden_dropout(RpTrainer* tr, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                                                    int32_t T, void* out_hidden_bf16, void* workspace, size_t workspace_bytes,
                                                    void* stream_) {
  return forward_hidden(tr, ids, cu_seqlens, batch, T, out_hidden_bf16, workspace, workspace_bytes, stream_, true);
}

static RpStatus backward_hidden(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens, int32_t batch,
                                int32_t T, const float* d_hidden, float* grads, void* workspace, size_t workspace_bytes,
                                void* stream_, bool dropout_ok) {
  RP_REQUIRE(tr && params && ids && cu_seqlens && d_hidden && grads, "null argument");
  TrainWs w;
  RpStatus st;
  if ((st = hidden_entry(tr, "rp_train_backward_hidden", dropout_ok))) return st;
  if ((st = train_entry(tr, batch, T, workspace, workspace_bytes, &w))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  if ((st = backward_zero(tr, batch, T, w, stream))) return st;
  if ((st = hidden_bwd_head(tr, T, d_hidden, grads, w, stream))) return st;
  return backward_layers(tr, params, ids, batch, T, grads, w, stream);
}
extern "C" RpStatus rp_train_backward_hidden(RpTrainer* tr, const float* params, const int32_t* ids, const int32_t* cu_seqlens,
                                             int32_t batch, int32_t T, const float* d_hidden, float* grads, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
  return backward_hidden(tr, params, ids, cu_seqlens, batch, T, d_hidden, grads, workspace, workspace_bytes, stream_, false);
}
extern "C" RpStatus rp_train_backward_hidden_dropout(RpTrainer* tr, const float* params, const int32_t* ids,
                                                     const int32_t* cu_seqlens, int32_t batch, int32_t T, const float* d_hidden,
                                                     float* grads, void* workspace, size_t workspace_bytes, void* stream_) {
  return backward_hidden(tr, params, ids, cu_seqlens, batch, T, d_hidden, grads, workspace, workspace_bytes, stream_, true);
}

// ||g||_2 of n floats -> out_norm[0] (device), deterministic; scratch = 1024 floats
extern "C" RpStatus rp_grad_norm(const float* grads, int64_t n, float* out_norm, float* scratch, void* stream_) {
  RP_REQUIRE(grads && out_norm && scratch && n > 0, "null argument");
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope ps(stream, RP_K_OPTIMIZER);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(1024), dim3(256), 0, stream, grads, (size_t)n, scratch);
  hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)scratch, 1024, out_norm);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// ---- kernel-level test entry points ------------------------------------------------------------------------
extern "C" RpStatus rp_dbg_wgrad(const void* Y, const void* X, float* out, int32_t T, int32_t ny, int32_t nx, int32_t splits,
                                 void* stream_) {
  RP_REQUIRE(Y && X && out && splits != 0, "bad argument");
  // splits < 0: |splits| partial matrices with the 128 x 128 tile configuration (> 0: the 256 x 256 one)
  return launch_wgrad((const bf16_t*)Y, ny, ny, (const bf16_t*)X, nx, nx, T, splits < 0 ? -splits : splits, out,
                      (hipStream_t)stream_, splits < 0 ? 1 : 0);
}

extern "C" RpStatus rp_dbg_wgrad_pair(const void* Y0, const void* X0, float* out0, int32_t ny0, int32_t nx0, const void* Y1,
                                      const void* X1, float* out1, int32_t ny1, int32_t nx1, int32_t T, int32_t splits,
                                      void* stream_) {
  RP_REQUIRE(Y0 && X0 && out0 && Y1 && X1 && out1 && splits > 0, "bad argument");
  const WgradOperands a{(const bf16_t*)Y0, ny0, ny0, (const bf16_t*)X0, nx0, nx0, out0};
  const WgradOperands b{(const bf16_t*)Y1, ny1, ny1, (const bf16_t*)X1, nx1, nx1, out1};
  return launch_wgrad_pair(a, b, T, splits, (hipStream_t)stream_);
}

// One or two products over the same T token rows with everything launch_wgrad / launch_wgrad_pair take left free: row
// pitches apart from the widths, the tile configuration forced or planned, the split count, the finishing epilogue on the
// first product.  Every argument is checked before anything is launched; no output is zeroed first.
extern "C" RpStatus rp_dbg_wgrad_ex(const void* Y0, int32_t ldy0, int32_t ny0, const void* X0, int32_t ldx0, int32_t nx0,
                                    float* out0, const void* Y1, int32_t ldy1, int32_t ny1, const void* X1, int32_t ldx1,
                                    int32_t nx1, float* out1, int32_t T, int32_t cfg, int32_t splits, float* g1, const float* w0,
                                    const float* w1, const float* ln, float* dln_part, int32_t* plan_out, void* stream_) {
  RP_REQUIRE(Y0 && X0 && out0 && plan_out, "null argument");
  RP_REQUIRE(T >= 64 && T % 64 == 0, "T=%d is no positive multiple of 64", T);
  RP_REQUIRE(splits >= 1 && splits <= T / 64, "splits=%d for %d token tiles", splits, T / 64);
  RP_REQUIRE(cfg >= -1 && cfg <= 1, "cfg=%d", cfg);
  auto operand_ok = [](const void* p, int ld, int n) {
    return n >= 8 && n % 8 == 0 && ld >= n && ld % 8 == 0 && ((uintptr_t)p & 15) == 0;  // 16-byte DMA pieces
  };
  RP_REQUIRE(operand_ok(Y0, ldy0, ny0) && operand_ok(X0, ldx0, nx0), "product 0: ny=%d ldy=%d nx=%d ldx=%d", ny0, ldy0, nx0, ldx0);
  const bool pair = Y1 != nullptr;
  if (pair) {
    RP_REQUIRE(X1 && out1, "null argument");
    RP_REQUIRE(operand_ok(Y1, ldy1, ny1) && operand_ok(X1, ldx1, nx1), "product 1: ny=%d ldy=%d nx=%d ldx=%d", ny1, ldy1, nx1, ldx1);
    RP_REQUIRE(cfg != 1, "a pair runs on 256 x 256 tiles only");
  }
  const bool finish = g1 || w0 || w1 || ln || dln_part;
  if (finish) RP_REQUIRE(g1 && w0 && w1 && ln && dln_part, "the finishing epilogue: null argument");
  const WgradFinish fin{1, g1, w0, w1, ln, dln_part};
  hipStream_t stream = (hipStream_t)stream_;
  plan_out[0] = pair ? 0 : cfg >= 0 ? cfg : plan_wgrad(ny0, nx0, T / 64).cfg;
  plan_out[1] = splits;
  if (!pair)
    return launch_wgrad((const bf16_t*)Y0, ldy0, ny0, (const bf16_t*)X0, ldx0, nx0, T, splits, out0, stream, cfg,
                        finish ? &fin : nullptr);
  WgradOperands a{(const bf16_t*)Y0, ldy0, ny0, (const bf16_t*)X0, ldx0, nx0, out0};
  if (finish) a.fin = fin;
  const WgradOperands b{(const bf16_t*)Y1, ldy1, ny1, (const bf16_t*)X1, ldx1, nx1, out1};
  return launch_wgrad_pair(a, b, T, splits, stream);
}

// No GPU call.  out[0], out[1] = (cfg, splits) of plan_wgrad(rows0, cols0, nk); out[2], out[3] = those of
// plan_wgrad_pair(rows0, cols0, rows1, cols1, nk) (splits 0: the model prefers separate launches), -1 when rows1 == 0.
extern "C" RpStatus rp_dbg_wgrad_plan(int32_t rows0, int32_t cols0, int32_t rows1, int32_t cols1, int32_t nk, int32_t* out) {
  RP_REQUIRE(out, "null argument");
  RP_REQUIRE(rows0 >= 1 && cols0 >= 1 && nk >= 1 && rows1 >= 0 && (rows1 == 0 || cols1 >= 1), "rows0=%d cols0=%d rows1=%d cols1=%d nk=%d",
             rows0, cols0, rows1, cols1, nk);
  const WgradPlan one = plan_wgrad(rows0, cols0, nk);
  out[0] = one.cfg;
  out[1] = one.splits;
  out[2] = out[3] = -1;
  if (rows1 > 0) {
    const WgradPlan two = plan_wgrad_pair(rows0, cols0, rows1, cols1, nk);
    out[2] = two.cfg;
    out[3] = two.splits;
  }
  return RP_OK;
}

extern "C" RpStatus rp_dbg_attention_bwd(const void* qkv, const void* att, const void* datt, const int32_t* cu,
                                         const float* bias_tab, int32_t batch, int32_t H, int32_t rows_total, void* lse_out,
                                         void* att_out, void* dqkv, float* dtab /* [H, 257] */, void* stream_) {
  // forward (writes att_out + lse) then both backward kernels; test entry only: scratch is allocated here
  const int maxd = 128, ntab = 2 * maxd + 1;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(H, rows_total / ATT_Q + batch);
  const int n_p = rows_total / POOL_CHUNK + batch;
  int4* work = nullptr;
  float *delta = nullptr, *part = nullptr;
  int32_t* bk = nullptr;
  RP_HIP(hipMalloc((void**)&work, ((size_t)grid.y + n_p) * sizeof(int4)));
  RP_HIP(hipMalloc((void**)&delta, (size_t)H * rows_total * 4));
  RP_HIP(hipMalloc((void**)&part, (size_t)grid.y * H * ntab * 4));
  RP_HIP(hipMalloc((void**)&bk, (size_t)ntab * 4));
  RP_HIP(hipMemsetAsync(part, 0, (size_t)grid.y * H * ntab * 4, stream));
  {
    std::vector<int32_t> ident(ntab);
    for (int i = 0; i < ntab; ++i) ident[i] = i;  // identity "buckets": the raw table gradient comes back
    RP_HIP(hipMemcpy(bk, ident.data(), (size_t)ntab * 4, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(worklist_kernel, dim3(1), dim3(1024), 0, stream, cu, batch, work, (int)grid.y, work + grid.y, n_p, POOL_CHUNK);
  hipLaunchKernelGGL((attention_kernel<true, false>), grid, dim3(256), 0, stream, (const bf16_t*)qkv, (const int4*)work, bias_tab,
                     (bf16_t*)att_out, H, maxd, (float*)lse_out, rows_total, Drop{0u, 0u, 1.f}, 0u);
  const bf16_t* o = att ? (const bf16_t*)att : (const bf16_t*)att_out;
  hipLaunchKernelGGL((attn_bwd_kernel<0, false>), grid, dim3(256), 0, stream, (const bf16_t*)qkv, o, (const bf16_t*)datt,
                     (const float*)lse_out, delta, (const int4*)work, bias_tab, (bf16_t*)dqkv, part, H, maxd, rows_total, 0,
                     Drop{0u, 0u, 1.f}, 0u);
  hipLaunchKernelGGL((attn_bwd_kernel<1, false>), grid, dim3(256), 0, stream, (const bf16_t*)qkv, o, (const bf16_t*)datt,
                     (const float*)lse_out, delta, (const int4*)work, bias_tab, (bf16_t*)dqkv, part, H, maxd, rows_total, 0,
                     Drop{0u, 0u, 1.f}, 0u);
  // [ntab "buckets", H] -> caller's [H, ntab] is the transposed view; the test reads it as [ntab, H]
  hipLaunchKernelGGL(bias_grad_kernel, dim3(H), dim3(256), 0, stream, (const float*)part, (int)grid.y, H, ntab,
                     (const int32_t*)bk, ntab, dtab);
  const hipError_t le = hipGetLastError();
  (void)hipStreamSynchronize(stream);
  (void)hipFree(work);
  (void)hipFree(delta);
  (void)hipFree(part);
  (void)hipFree(bk);
  if (le != hipSuccess) return fail(RP_E_HIP, "attention backward launch failed: %s", hipGetErrorString(le));
  return RP_OK;
}

// The training attention alone, as the trainer launches it: the forward (att_out + lse), both backward launches (delta, dqkv, the
// table gradient's partial rows) and bias_grad_kernel with identity buckets, at any max_distance and under the trainer's dropout
// (the mask is rp_dbg_dropout_mask(p, seed, site, row = s0 + i, col = (h << 20) | j)).  att != NULL: the O the backward reads for
// delta instead of att_out.  Scratch (work list, partial rows, buckets) is allocated here; synchronises.  Everything is checked
// before anything is launched; no output is zeroed first (rows T .. rows_total of att_out / dqkv / lse / delta are not written).
extern "C" RpStatus rp_dbg_attention_train(const void* qkv, const void* att, const void* datt, const int32_t* cu, const float* bias_tab,
                                           int32_t batch, int32_t H, int32_t rows_total, int32_t maxd, float p, uint32_t seed,
                                           uint32_t site, float* lse_out, void* att_out, float* delta_out, void* dqkv, float* dtab,
                                           void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RP_REQUIRE(qkv && datt && cu && bias_tab && lse_out && att_out && delta_out && dqkv && dtab, "null argument");
  RP_REQUIRE(batch >= 1 && H >= 1 && rows_total >= GEMM_M_ALIGN && rows_total % GEMM_M_ALIGN == 0, "batch=%d, H=%d, rows_total=%d", batch,
             H, rows_total);
  RP_REQUIRE(maxd >= 1 && 2 * maxd + 1 + 128 <= ATT_TAB_MAX, "max_distance=%d", maxd);  // as rp_encoder_create
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  int T = 0;
  {
    std::vector<int32_t> h((size_t)batch + 1);
    RP_HIP(hipMemcpyAsync(h.data(), cu, h.size() * 4, hipMemcpyDeviceToHost, stream));
    RP_HIP(hipStreamSynchronize(stream));
    T = h[batch];
    RP_REQUIRE(h[0] == 0 && T >= 1 && T <= rows_total, "cu_seqlens runs %d .. %d for rows_total=%d", h[0], T, rows_total);
    for (int i = 0; i < batch; ++i) RP_REQUIRE(h[i + 1] > h[i], "sequence %d is empty (cu_seqlens %d, %d)", i, h[i], h[i + 1]);
  }
  const Drop drop = make_drop(p, seed);
  const int ntab = 2 * maxd + 1;
  const dim3 grid(H, T / ATT_Q + batch);
  const int n_p = T / POOL_CHUNK + batch;
  int4* work = nullptr;
  float* part = nullptr;
  int32_t* bk = nullptr;
  RP_HIP(hipMalloc((void**)&work, ((size_t)grid.y + n_p) * sizeof(int4)));
  RP_HIP(hipMalloc((void**)&part, (size_t)grid.y * H * ntab * 4));
  RP_HIP(hipMalloc((void**)&bk, (size_t)ntab * 4));
  RP_HIP(hipMemsetAsync(part, 0, (size_t)grid.y * H * ntab * 4, stream));  // (the partial rows accumulate: backward_zero's part)
  {
    std::vector<int32_t> ident(ntab);
    for (int i = 0; i < ntab; ++i) ident[i] = i;  // identity "buckets": the raw table gradient comes back, [ntab, H]
    RP_HIP(hipMemcpy(bk, ident.data(), (size_t)ntab * 4, hipMemcpyHostToDevice));
  }
  launch_worklist(cu, batch, work, (int)grid.y, work + grid.y, n_p, POOL_CHUNK, stream);
  launch_attention_train_fwd(grid, (const bf16_t*)qkv, (const int4*)work, bias_tab, (bf16_t*)att_out, H, maxd, lse_out, rows_total, drop,
                             site, stream);
  const bf16_t* o = att ? (const bf16_t*)att : (const bf16_t*)att_out;
  launch_attention_bwd(grid, (const bf16_t*)qkv, o, (const bf16_t*)datt, lse_out, delta_out, (const int4*)work, bias_tab, (bf16_t*)dqkv,
                       part, H, maxd, rows_total, 0, drop, site, stream);
  launch_bias_grad(part, (int)grid.y, H, ntab, bk, ntab, dtab, stream);
  const hipError_t le = hipGetLastError();
  (void)hipStreamSynchronize(stream);
  (void)hipFree(work);
  (void)hipFree(part);
  (void)hipFree(bk);
  if (le != hipSuccess) return fail(RP_E_HIP, "attention launch failed: %s", hipGetErrorString(le));
  return RP_OK;
}

// The last_hidden_state head alone: the forward, then the backward with its colsum, on caller-supplied planes (rows T .. Tp of
// dxhi / dxlo are the caller's); the partial rows of d ln are allocated here.
extern "C" RpStatus rp_dbg_hidden_head(const void* xhi, const void* xlo, const float* rs, const float* ln, const float* d_hidden,
                                       int32_t T, int32_t D, void* out_hidden, void* dxhi, void* dxlo, float* dln,
                                       void* stream_) {
  RP_REQUIRE(xhi && xlo && rs && ln && d_hidden && out_hidden && dxhi && dxlo && dln, "null argument");
  RP_REQUIRE(T >= 1 && D >= 8 && D % 8 == 0 && D <= 4 * 512, "T=%d, D=%d", T, D);
  hipStream_t stream = (hipStream_t)stream_;
  float* part = nullptr;
  RP_HIP(hipMalloc((void**)&part, (size_t)((T + HIDDEN_BWD_ROWS - 1) / HIDDEN_BWD_ROWS) * D * 4));
  RpStatus st = launch_hidden_head((const bf16_t*)xhi, (const bf16_t*)xlo, rs, ln, (bf16_t*)out_hidden, T, D, stream);
  if (st == RP_OK)
    st = launch_hidden_bwd_head((const bf16_t*)xhi, (const bf16_t*)xlo, rs, ln, d_hidden, (bf16_t*)dxhi, (bf16_t*)dxlo, part, dln,
                                T, D, stream);
  (void)hipStreamSynchronize(stream);
  (void)hipFree(part);
  return st;
}

// dgrad epilogues in isolation.  mode 0: EpiGegluBwd (A = dx [M, K], W = Wo2^T [F, K]; aux0 = gu [M, 2F] bf16, aux1 = rs [M];
// out0 = dzs [M, 2F] bf16, out1 = row dot [M] f32 (slots summed)).  mode 1: EpiRmsBwdResid (A = dzs [M, K], W [N, K];
// aux0 = x [M, N] bf16, aux1 = rcoef [M]; out0 = the two planes [2, M, N], updated in place).
extern "C" RpStatus rp_dbg_dgrad(const void* A, const void* W, int32_t M, int32_t N, int32_t K, int32_t mode, const void* aux0,
                                 const float* aux1, void* out0, float* out1, int32_t variant, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bf16_t* a = (const bf16_t*)A;
  const bf16_t* w = (const bf16_t*)W;
  if (mode == 0) {
    const int np = (N + 63) / 64;
    float* rdp = nullptr;
    float* ones = nullptr;
    RP_HIP(hipMalloc((void**)&rdp, (size_t)np * M * 4));
    RP_HIP(hipMalloc((void**)&ones, (size_t)M * 4));
    std::vector<float> one(M, 1.f);
    RP_HIP(hipMemcpy(ones, one.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    RpStatus st = launch_gemm(a, K, M, w, K, N, K, EpiGegluBwd{(const bf16_t*)aux0, (bf16_t*)out0, 2 * N, N, aux1, rdp, np, M, Drop{0u, 0u, 1.f}, 0u},
                              stream, RP_K_BWD_DGRAD, 0, nullptr, variant);
    // out1 = sum of the slots (rs = 1, inv_d = 1 turns rowdot_finish into a plain slot sum)
    if (st == RP_OK)
      launch_rowdot_finish(rdp, np, M, ones, 1.f, out1, M, stream);
    (void)hipStreamSynchronize(stream);
    (void)hipFree(rdp);
    (void)hipFree(ones);
    return st;
  }
  return launch_gemm(a, K, M, w, K, N, K,
                     EpiRmsBwdResid{(bf16_t*)out0, (bf16_t*)out0 + (size_t)M * N, N, N, (const bf16_t*)aux0, aux1}, stream,
                     RP_K_BWD_DGRAD, 0, nullptr, variant);
}

// One launch_gemm with a training epilogue and its dropout (tests/test_train_mfma_kernels_gpu.py).  A bf16 [M, K], W bf16 [N, K]
// (exactly N rows), M % GEMM_M_ALIGN == 0.  The Drop is rp_trainer_set_dropout's and rp_dbg_dropout_mask's (make_drop), so the mask
// read back with rp_dbg_dropout_mask(p, seed, site, ..) is the one the launch used.
//   mode 0: the gated-GELU backward (EpiGegluBwd) over N = d_ff rows of W = Wo2^T.  aux0 = gu bf16 [M, ld] (2 N packed columns live),
//           aux1 = rs [M]; out0 = dzs bf16 [M, ld], out1 = the row dot's slots f32 [ceil(N / 64), M], out2 = rcoef f32 [M] from
//           launch_rowdot_finish over those slots with inv_d = 1 / K; p > 0: dff is masked at `site`.  variant 0 or 26.
//   mode 1: the RMSNorm-backward residual.  aux0 = x bf16 [M, ld], aux1 = rcoef [M]; out0 / out1 = the hi / lo planes [M, ld],
//           updated in place; p > 0: EpiRmsBwdResidT<true>, out2 = dxm bf16 [M, ld] under the mask of `site` (the trainer's
//           next_site), p == 0: EpiRmsBwdResid, out2 unused.  variant 0 or 26.
//   mode 2: the training forward's FFN-in epilogue, N = 2 d_ff packed rows.  aux1 = rs [M] (NULL: no row factor); out0 = gu bf16
//           [M, N], out1 = ff bf16 [M, ld]; p > 0: EpiGegluTrainT<true> with the mask of `site`, p == 0: <false>.  variant -1:
//           the forward's own choice (pick_gemm_variant).
//   mode 3: the training forward's residual projections (EpiResidT<true>).  aux0 = the old hi plane bf16 [M, ld] (read only);
//           out0 = the new hi plane [M, ld], out1 = the lo plane [M, ld], updated in place; out2 = ssp f32 [ceil(N / 64), M]
//           or NULL; p > 0: the projection's output is masked at `site` before it is added.  variant -1: the forward's choice.
// plan[6]: what launch_gemm_cfg launched, as rp_dbg_gemm_ex reports it.  Checked before anything is launched; nothing zeroed.
extern "C" RpStatus rp_dbg_train_gemm(int32_t mode, const void* A, const void* W, int32_t M, int32_t N, int32_t K, const void* aux0,
                                      const float* aux1, void* out0, void* out1, void* out2, int32_t ld, float p, uint32_t seed,
                                      uint32_t site, int32_t variant, int32_t* plan, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RP_REQUIRE(mode >= 0 && mode <= 3, "mode=%d", mode);
  RP_REQUIRE(A && W && out0 && out1 && plan, "null argument");
  RP_REQUIRE(M >= GEMM_M_ALIGN && M % GEMM_M_ALIGN == 0 && K >= 32 && K % 32 == 0 && N >= 8 && N % 8 == 0, "M=%d, N=%d, K=%d", M, N, K);
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  const Drop drop = make_drop(p, seed);
  const bf16_t* a = (const bf16_t*)A;
  const bf16_t* w = (const bf16_t*)W;
  auto gemm = [&]() -> RpStatus {
    if (mode == 0)
      return launch_gemm(a, K, M, w, K, N, K,
                         EpiGegluBwd{(const bf16_t*)aux0, (bf16_t*)out0, ld, N, aux1, (float*)out1, (N + 63) / 64, M, drop, site}, stream,
                         RP_K_BWD_DGRAD, 0, nullptr, variant);
    if (mode == 1) {
      if (drop.thresh)
        return launch_gemm(a, K, M, w, K, N, K,
                           EpiRmsBwdResidT<true>{(bf16_t*)out0, (bf16_t*)out1, ld, N, (const bf16_t*)aux0, aux1, (bf16_t*)out2, drop, site},
                           stream, RP_K_BWD_DGRAD, 0, nullptr, variant);
      return launch_gemm(a, K, M, w, K, N, K, EpiRmsBwdResid{(bf16_t*)out0, (bf16_t*)out1, ld, N, (const bf16_t*)aux0, aux1}, stream,
                         RP_K_BWD_DGRAD, 0, nullptr, variant);
    }
    if (mode == 3)
      return launch_gemm(a, K, M, w, K, N, K,
                         EpiResidT<true>{(bf16_t*)out0, (bf16_t*)out1, ld, N, (float*)out2, (N + 63) / 64, M, (const bf16_t*)aux0, drop, site},
                         stream, RP_K_GEMM_WO, 0, nullptr, variant);
    const EpiStoreBf16 gu_store{(bf16_t*)out0, N, N, RowScale{aux1}};
    if (drop.thresh)
      return launch_gemm(a, K, M, w, K, N, K, EpiGegluTrainT<true>{gu_store, (bf16_t*)out1, ld, N, RowScale{aux1}, drop, site}, stream,
                         RP_K_GEMM_WI, 0, nullptr, variant);
    return launch_gemm(a, K, M, w, K, N, K, EpiGegluTrainT<false>{gu_store, (bf16_t*)out1, ld, N, RowScale{aux1}, drop, site}, stream,
                       RP_K_GEMM_WI, 0, nullptr, variant);
  };
  if (mode == 0) {
    RP_REQUIRE(aux0 && aux1 && out2, "null argument");
    RP_REQUIRE(N % 64 == 0 && ld >= 2 * N && ld % 8 == 0, "gated GELU backward: N=%d, ld=%d", N, ld);
    RP_REQUIRE(variant == 0 || variant == 26, "variant=%d", variant);
  } else if (mode == 1) {
    RP_REQUIRE(aux0 && aux1, "null argument");
    RP_REQUIRE(ld >= N && ld % 8 == 0, "ld=%d, N=%d", ld, N);
    RP_REQUIRE(variant == 0 || variant == 26, "variant=%d", variant);
    RP_REQUIRE(!drop.thresh || (out2 && site != 0), "the masked form needs dxm and a site");
  } else if (mode == 3) {
    RP_REQUIRE(aux0, "null argument");
    RP_REQUIRE(ld >= N && ld % 8 == 0, "ld=%d, N=%d", ld, N);
    RP_REQUIRE(variant >= -1, "variant=%d", variant);
  } else {
    RP_REQUIRE(N % 64 == 0, "gated GELU: N=%d is not whole 32 / 32 row blocks", N);
    RP_REQUIRE(ld >= N / 2 && ld % 8 == 0, "ld=%d, N=%d", ld, N);
    RP_REQUIRE(variant >= -1, "variant=%d", variant);
  }
  g_gemm_check_only = true;  // launch_gemm's and launch_gemm_cfg's own requirements first, nothing launched
  RpStatus st = gemm();
  g_gemm_check_only = false;
  if (st) return st;
  st = gemm();
  if (mode == 0 && st == RP_OK) {
    launch_rowdot_finish((const float*)out1, (N + 63) / 64, M, aux1, 1.f / (float)K, (float*)out2, M, stream);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) st = fail(RP_E_HIP, "rowdot_finish launch failed: %s", hipGetErrorString(le));
  }
  const GemmLaunchPlan& lp = g_last_gemm_plan;
  plan[0] = lp.variant, plan[1] = lp.form, plan[2] = lp.tiles_f, plan[3] = lp.tiles_t, plan[4] = lp.n_helpers, plan[5] = lp.full_rows;
  return st;
}

// ---- the encoder's pooling head, training row kernels and weight pack / unpack kernels in isolation -------------------------
// (tests/test_encoder_train_kernels_gpu.py).  Device pointers, the launch functions the trainer and the
// encoder pass run, arguments checked before anything is launched, no output zeroed first.
extern "C" RpStatus rp_dbg_train_rows(int32_t mode, const void* a, const void* b, const int32_t* ia, int32_t T, int32_t rows,
                                      int32_t n, int32_t vocab, int32_t np, int32_t ld, float inv_d, float p, uint32_t seed,
                                      uint32_t site, void* o0, void* o1, void* o2, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RP_REQUIRE(mode >= 0 && mode <= 5, "mode=%d", mode);
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  RP_REQUIRE(rows >= 1 && n >= 8 && n % 8 == 0, "rows=%d, n=%d", rows, n);
  const Drop drop = make_drop(p, seed);
  switch (mode) {
    case 0:  // embed_kernel<false>
    case 1:  // embed_train_kernel
      RP_REQUIRE(ia && a && o0 && o1 && o2, "null argument");
      RP_REQUIRE(T >= 1 && T <= rows && vocab >= 1 && np >= 1, "T=%d, Tp=%d, vocab=%d, np=%d", T, rows, vocab, np);
      RP_REQUIRE((mode == 1) == (drop.thresh != 0), "mode %d %s p > 0", mode, mode == 1 ? "needs" : "takes no");
      launch_embed(ia, (const float*)a, (bf16_t*)o0, (bf16_t*)o1, (float*)o2, np, T, rows, n, vocab, drop, stream);
      break;
    case 2:  // mask_dx_kernel
      RP_REQUIRE(a && b && o0, "null argument");
      launch_mask_dx((const bf16_t*)a, (const bf16_t*)b, (bf16_t*)o0, rows, n, drop, site, stream);
      break;
    case 3:  // qkv_scale_dot_kernel (o0 = dqkv, in place)
      RP_REQUIRE(a && b && o0 && o1, "null argument");
      RP_REQUIRE(T >= 0 && T <= rows, "T=%d, rows=%d", T, rows);
      launch_qkv_scale_dot((bf16_t*)o0, (const bf16_t*)a, (const float*)b, (float*)o1, T, rows, n, inv_d, stream);
      break;
    case 4:  // rowdot_finish_kernel (n unused)
      RP_REQUIRE(a && b && o0, "null argument");
      RP_REQUIRE(np >= 1 && ld >= rows, "np=%d, ld=%d, rows=%d", np, ld, rows);
      launch_rowdot_finish((const float*)a, np, ld, (const float*)b, inv_d, (float*)o0, rows, stream);
      break;
    default:  // embed_bwd_kernel (rows = T)
      RP_REQUIRE(ia && a && b && o0, "null argument");
      RP_REQUIRE(T >= 1 && vocab >= 1, "T=%d, vocab=%d", T, vocab);
      launch_embed_bwd(ia, T, vocab, (const bf16_t*)a, (const bf16_t*)b, n, (float*)o0, drop, stream);
      break;
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_dbg_pool_head(const void* xhi, const void* xlo, int32_t lo8, const float* rs, const int32_t* cu,
                                     int32_t batch, int32_t T, int32_t D, const float* w, int32_t chunk, int32_t fuse,
                                     int32_t out_bf16, const float* d_emb, float p, uint32_t seed, void* out, float* partial,
                                     void* pwork, float* ds, float* dwf, float* d_final_ln, void* dxhi, void* dxlo,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RP_REQUIRE(xhi && xlo && rs && cu && w && out && partial && pwork, "null argument");
  RP_REQUIRE(batch >= 1 && T >= 1 && D >= 8 && D % 8 == 0 && D <= 4 * 512, "batch=%d, T=%d, D=%d", batch, T, D);
  RP_REQUIRE(chunk == 32 || chunk == 64 || chunk == 128, "chunk=%d", chunk);
  RP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability %g", (double)p);
  const Drop drop = make_drop(p, seed);
  const bool training_form = chunk == POOL_CHUNK && !fuse && !lo8 && !out_bf16;
  RP_REQUIRE(!drop.thresh || training_form, "dropout: the training form only (chunk 128, fuse 0, bf16 lo plane, fp32 out)");
  if (d_emb) {
    RP_REQUIRE(training_form, "the backward: the training form only (chunk 128, fuse 0, bf16 lo plane, fp32 out)");
    RP_REQUIRE(ds && dwf && d_final_ln && dxhi && dxlo, "null argument");
  }
  {  // every sequence holds at least its EOS: an empty one is outside the pooling head's contract and refused here
    std::vector<int32_t> h((size_t)batch + 1);
    RP_HIP(hipMemcpyAsync(h.data(), cu, h.size() * 4, hipMemcpyDeviceToHost, stream));
    RP_HIP(hipStreamSynchronize(stream));
    RP_REQUIRE(h[0] == 0 && h[batch] == T, "cu_seqlens runs %d .. %d for T=%d", h[0], h[batch], T);
    for (int i = 0; i < batch; ++i) RP_REQUIRE(h[i + 1] > h[i], "sequence %d is empty (cu_seqlens %d, %d)", i, h[i], h[i + 1]);
  }
  const int n_att = T / ATT_Q + batch;
  int4* work = nullptr;  // the attention list of the same launch
  RP_HIP(hipMalloc((void**)&work, (size_t)n_att * sizeof(int4)));
  launch_worklist(cu, batch, work, n_att, (int4*)pwork, T / chunk + batch, chunk, stream);
  launch_pool_head((const bf16_t*)xhi, (const bf16_t*)xlo, lo8 != 0, rs, (const int4*)pwork, partial, cu, batch, T, D, chunk, w, out,
                   out_bf16, fuse, drop, stream);
  if (d_emb)
    launch_pool_bwd_head((const bf16_t*)xhi, (const bf16_t*)xlo, rs, (const int4*)pwork, partial, w, cu, batch, T, D, d_emb, ds, dwf,
                         d_final_ln, (bf16_t*)dxhi, (bf16_t*)dxlo, drop, stream);
  const hipError_t le = hipGetLastError();
  (void)hipStreamSynchronize(stream);
  (void)hipFree(work);
  if (le != hipSuccess) return fail(RP_E_HIP, "pooling head launch failed: %s", hipGetErrorString(le));
  return RP_OK;
}

extern "C" RpStatus rp_dbg_repack(const RpDbgRepackMat* mats, int32_t n_mats, void* stream_) {
  RP_REQUIRE(mats && n_mats >= 1 && n_mats <= 4, "n_mats=%d", n_mats);
  RepackPlan plan;
  for (int k = 0; k < n_mats; ++k) {
    const RpDbgRepackMat& m = mats[k];
    RP_REQUIRE(m.s0 && m.dst && m.dst_t, "matrix %d: null argument", k);
    RP_REQUIRE(m.rows >= 64 && m.cols >= 64 && m.rows % 64 == 0 && m.cols % 64 == 0, "matrix %d: rows=%d, cols=%d", k, m.rows,
               m.cols);
    RP_REQUIRE(m.mode == PACK_CONCAT3 || m.mode == PACK_GEGLU || m.mode == PACK_COPY, "matrix %d: mode=%d", k, m.mode);
    if (m.mode == PACK_CONCAT3) RP_REQUIRE(m.s1 && m.s2 && m.n >= 1 && m.rows == 3 * m.n, "matrix %d: rows=%d, n=%d", k, m.rows, m.n);
    if (m.mode == PACK_GEGLU) RP_REQUIRE(m.s1, "matrix %d: null argument", k);
    plan.add(m.s0, m.s1, m.s2, m.colscale, (bf16_t*)m.dst, (bf16_t*)m.dst_t, m.rows, m.cols, m.n, m.mode);
  }
  plan.launch((hipStream_t)stream_);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_dbg_bias_table(const float* rel_bias, const int32_t* bucket_of, int32_t H, int32_t ntab, float* tab,
                                      void* stream_) {
  RP_REQUIRE(rel_bias && bucket_of && tab && H >= 1 && ntab >= 1, "bad argument");
  launch_bias_table(rel_bias, bucket_of, H, ntab, tab, (hipStream_t)stream_);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" RpStatus rp_dbg_unfold(const float* part, int64_t split_stride, int32_t splits, int32_t rows, int32_t C, int32_t mode,
                                  int32_t n, float* g0, float* g1, float* g2, const float* w0, const float* w1, const float* w2,
                                  const float* ln, float* dln_part, float* dln, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RP_REQUIRE(part && g0, "null argument");
  RP_REQUIRE(splits >= 1 && rows >= 1 && C >= 4 && C % 4 == 0, "splits=%d, rows=%d, C=%d", splits, rows, C);
  RP_REQUIRE(split_stride >= (int64_t)rows * C, "split_stride=%lld < rows * C", (long long)split_stride);
  RP_REQUIRE(mode == UNFOLD_PLAIN || mode == UNFOLD_QKV || mode == UNFOLD_GEGLU, "mode=%d", mode);
  if (mode == UNFOLD_QKV) RP_REQUIRE(n >= 1 && rows == 3 * n && g1 && g2 && w0 && w1 && w2, "QKV: rows=%d, n=%d", rows, n);
  if (mode == UNFOLD_GEGLU) RP_REQUIRE(rows % 64 == 0 && g1 && w0 && w1, "GEGLU: rows=%d", rows);
  if (mode != UNFOLD_PLAIN) RP_REQUIRE(ln && dln_part && dln, "null argument");
  UnfoldArgs a{};
  a.part = part; a.split_stride = (size_t)split_stride; a.splits = splits; a.rows = rows; a.C = C; a.mode = mode; a.n = n;
  a.g0 = g0; a.g1 = g1; a.g2 = g2; a.w0 = w0; a.w1 = w1; a.w2 = w2; a.ln = ln; a.dln_part = dln_part;
  RpStatus st = run_unfold(a, stream);
  if (st) return st;
  if (mode != UNFOLD_PLAIN) launch_colsum(dln_part, (rows + 31) / 32, C, dln, stream);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
