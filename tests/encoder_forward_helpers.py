"""Float64 restatements of the encoder's forward MFMA kernels and its embedding / output row kernels, one kernel at a time, for
tests/test_encoder_forward_kernels_gpu.py (the kernels, through rp_dbg_gemm_ex / rp_dbg_attention_ex / rp_dbg_encoder_rows /
rp_dbg_rowscale) and tests/test_encoder_forward_kernels_cpu.py (the restatements against torch float64, float32 stand-ins of
the kernels' schedules against every bar, planted bugs against the same bars).  numpy float64, no GPU; the 24-bit and two-plane
encodings are hip_helpers.split_x24 / merge_x24 / split_planes on CPU tensors.

GEMM  C[token, feature] = sum_k A[token, k] W[feature, k], operands bf16.  Every output element is ONE K-ascending chain of
K / 16 v_mfma_f32_32x32x16_bf16 steps (rp_gemm.h: "every output element is the same K-ascending chain of MFMA steps under every
layout", in the per-tile, persistent and mixed forms alike), each adding 16 exact bf16 products to the fp32 accumulator, so
    |acc - C| <= (K / 16 + 16) 2^-24 sum_k |a_k w_k|                                                            (acc_bar)
and the epilogues add (rp_encoder_kernels.h):
  STORE   bf16(acc * rs): one fp32 product (2^-24), the factor's own error (rs_rel), one bf16 rounding (half an ulp of bf16 at
          the value: bf16_half_ulp);
  RESID   v = (hi + lo) + acc in fp32 (2^-24 |v|), hi = bf16(v), lo = bf16(v - hi): |v - hi| <= 2^-9 ulp-binade, its rounding
          2^-17 |v|;  the hi plane alone is within one bf16 rounding;
  RESID8  v = x + acc in fp32, rounded to its top 24 bits half away from zero (2^-16 |v|; with an exact accumulator the planes
          are split_x24(v) to the bit);  ssp[slot, token] = the sum of squares of the 64 features of the slot AS STORED, an fma
          chain of 8 and a 3-step tree: 16 x 2^-24 of the sum;
  GEGLU   gelu_new(rs g) (rs u), bf16: both accumulators' terms propagated to first order + their product, one bf16 rounding,
          and FASTMATH_ENC_GEGLU for u * rcp(1 + exp2(..)) with the factor folded into its constants (rp_util.h geglu2), which
          cannot be derived: 2 x the largest excess over the derived terms measured on the MI355X (below).

Attention (attention_kernel<false>): s = q . k (four MFMA steps) + tab[h, clamp(j - i, -maxd, maxd) + maxd] in fp32, no
1 / sqrt(d); p = exp2((s - m) log2 e) in fp32 with the running maximum m; the row sum adds the UNROUNDED p (`psum += p` stands
before the pack), the P V product takes p ROUNDED to bf16 (`pack_bf2` of s[kb][..] in front of the second MFMA); the output is
bf16(o / l).  So per element
    |out - ref| <= 2^-8 sum_j p_j |v_j| / sum_j p_j                                (the rounding of every p_j)
                 + half a bf16 ulp of the result                                   (the store)
                 + sum_j p_j rel_ij (|v_j| + |ref|) / sum_j p_j + chain terms      (fp32: attention_fp32_bar)
with rel_ij the relative error of p_ij from its exponent's error (the score's accumulation and the fma's roundings, scaled by
ln 2) and one ulp of v_exp_f32, and the chains 5 steps per 64-key tile for o, 32 adds per tile for l."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import hip_helpers as hh
from decoder_kernel_helpers import bf16_round, rel_l2, worst_row  # noqa: F401  (re-exported)

U32 = 2.0 ** -24
EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_RESID8 = 0, 1, 2, 3  # RP_EPI_*
EPI_NAMES = {EPI_STORE: "store", EPI_RESID: "resid", EPI_GEGLU: "geglu", EPI_RESID8: "resid8"}
K_QKV, K_O, K_WI, K_WO = 2, 4, 5, 6  # RP_K_GEMM_*
CLASS_BIT = {K_QKV: 1, K_O: 4, K_WI: 8, K_WO: 16}  # the class's bit in the gemm_persist / gemm_mixed options
FORM_TILE, FORM_PERSIST, FORM_MIXED = 0, 1, 2
EPS = 1e-6

# tile configuration -> (feature tile BM, token tile BN, BK, ring stages, pipelined loop)   (launch_gemm's table)
VARIANTS = {26: (256, 256, 64, 2, 1), 9: (256, 256, 32, 3, 0), 30: (256, 128, 64, 2, 1), 0: (128, 128, 32, 3, 0),
            15: (64, 128, 32, 7, 0), 16: (64, 128, 64, 4, 0), 17: (64, 128, 64, 4, 1)}
SMALL_VARIANTS = (0, 15, 16, 17)
# k-tile counts 1, 2, 3, 4, 5, 7, 8 (+ a long one): one k-tile, and each ring (2, 3, 4, 7 stages) wrapping zero, one and
# several times
KS_BK64 = (64, 128, 192, 256, 320, 448, 512, 1472)
KS_BK32 = (32, 64, 96, 128, 224, 256, 1504)
KS_LONG = (3584, 7168)
# valid features of the last (here: only) feature tile: either side of the edge layouts' thresholds (128, 192); the last
# statistic slot full (64, 128, 192, 256), half full (96) and 8 wide (8, 136, 200)
N_VALIDS = (8, 64, 96, 128, 136, 192, 200, 256)
N_MAX = 256
PLACEMENT_ROWS = (0, 63, 64, 127, 128, 255)
PLACEMENT_FEATURES = (0, 31, 32, 63, 64, -1)  # -1: the last valid one
TOKENS_VALID = (1, 63, 64, 65, 101, 127, 128, 129, 255, 256, 257, 512)
GEGLU_GATE_STDS = (1.0, 3.0, 10.0, 30.0)  # std of the gate accumulator by output feature (f % 4): |g| from below 1 to beyond 100

# u * rcp(1 + exp2(..)) with the token's factor folded into the constants (rp_util.h geglu2): what the epilogue may miss float64
# by beyond one bf16 rounding and the propagated accumulator terms, absolute, = 2 x the largest excess measured on the MI355X
# over the K, gate-scale and row-scale sweep of tests/test_encoder_forward_kernels_gpu.py
# (profiles/encoder_forward_kernel_margins.json, "geglu_fastmath_excess").  The factor 2 covers box-to-box variation of a
# deterministic kernel whose only freedom is the operand sweep.
#   Measured: no excess.  Over all 7 tile configurations x 10 K x 4 widths, the row-scale forms, the token-count and the
#   persistent-form cases (gates from below 1 to beyond 100 in magnitude at every K >= 64) the largest |error| - derived terms
#   is negative everywhere: -4.6e-41 (results that are exactly zero, against the bar's floor of 2^-134), -3.3e-11 on the
#   nearest non-zero result (K = 64, persistent shape run per tile).  v_exp_f32 and v_rcp_f32 are 1 ulp each: their error stays
#   inside the bf16 rounding of the result and the propagated accumulator terms, so nothing is added.
GEGLU_EXCESS_MEASURED = 0.0
FASTMATH_ENC_GEGLU = 2.0 * GEGLU_EXCESS_MEASURED


def ks_of(variant: int) -> Tuple[int, ...]:
    return KS_BK64 if VARIANTS[variant][2] == 64 else KS_BK32


def expected_variant(forced: int, M: int, K: int, small_pipe: bool = True) -> int:
    """pick_gemm_variant with gemm_variant_all = ``forced`` and gemm_skinny off."""
    v = forced
    if v == 26 and K % 64:
        v = 9
    if v == 16 and K % 64:
        v = 15
    if v == 16 and small_pipe:
        v = 17
    if v >= 5 and M % 256:
        v = 0
    return v


def variant_admits(v: int, M: int, K: int) -> bool:
    bm, bn, bk, _, _ = VARIANTS[v]
    return K % bk == 0 and M % bn == 0 and (v < 5 or M % 256 == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# launch forms: plan_mixed and the persistent rule of launch_gemm_cfg, restated
# ---------------------------------------------------------------------------------------------------------------------------
def plan_mixed(tiles_f: int, tiles_t: int, n_cus: int) -> Tuple[int, int, int]:
    """-> (full_rows, half_first, half_last); full_rows = 0: no mixed launch."""
    unit = n_cus // math.gcd(tiles_f, n_cus)
    t1 = tiles_t // unit * unit
    rest = tiles_t - t1
    if t1 == 0 or rest == 0 or rest * tiles_f > (7 * n_cus) // 10 or 2 * rest * tiles_f > n_cus:
        return 0, 0, 0
    hf = min(2 * rest, (n_cus // 2) // tiles_f)
    return t1, hf, 2 * rest - hf


def expected_form(tiles_f: int, tiles_t: int, K: int, n_cus: int, prof_class: int, persist_opt: int, mixed_opt: int, epi: int,
                  t_dev: bool = False, variant: int = 26) -> Tuple[int, int]:
    """-> (form, full_rows) of launch_gemm_cfg for the pipelined 256 x 256 x 64 tile (helpers off)."""
    if variant != 26 or K < 128:
        return FORM_TILE, 0
    bit = CLASS_BIT[prof_class]
    if (mixed_opt & bit) and epi != EPI_GEGLU and not t_dev:  # (the gated-GELU epilogue takes no edge layouts: never mixed)
        full = plan_mixed(tiles_f, tiles_t, n_cus)[0]
        if full:
            return FORM_MIXED, full
    if (persist_opt & bit) and tiles_f * tiles_t > (n_cus & ~7):
        return FORM_PERSIST, 0
    return FORM_TILE, 0


def smallest_form_shapes(n_cus: int) -> Dict[str, Tuple[int, int]]:
    """The smallest (tiles_f, tiles_t) that give: a persistent launch in which workgroups walk two tiles (more tiles than
    workgroups; 16 feature tiles - under a class whose mixed option is on the same shape may take a mixed plan), and, tiles_f in
    {4, 8, 16}, a mixed plan with half_last = 0 and one with half_last > 0."""
    best: Dict[str, Tuple[int, int]] = {}
    for tf in (4, 8, 16):
        for tt in range(1, 4 * n_cus):
            full, _, hl = plan_mixed(tf, tt, n_cus)
            kinds = []
            if tf == 16 and tf * tt > (n_cus & ~7):
                kinds.append("persist")
            if full:
                kinds.append("mixed_tail" if hl > 0 else "mixed")
            for kind in kinds:
                if kind not in best or tf * tt < best[kind][0] * best[kind][1]:
                    best[kind] = (tf, tt)
            if tf * tt > 3 * n_cus:
                break
    return best


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM operands
# ---------------------------------------------------------------------------------------------------------------------------
def interleave_geglu(gate: np.ndarray, up: np.ndarray) -> np.ndarray:
    """[F, K] gate and up rows -> the packed operand [2 F, K]: blocks of 32 gate rows then the same 32 up rows (F % 32 == 0)."""
    F, K = gate.shape
    return np.stack([gate.reshape(F // 32, 32, K), up.reshape(F // 32, 32, K)], 1).reshape(2 * F, K)


@functools.lru_cache(maxsize=8)
def gemm_operands(M: int, N: int, K: int, kind: str, geglu: bool = False, seed: int = 0):
    """A [M, K], W [N, K] float64 arrays of bf16 values and x0 [M, N] (what the residual forms add to; fp32 values that the
    24-bit form holds exactly).  ``integer``: independent integers in [-4, 4], so that every partial sum in any order is an
    integer of magnitude <= 16 K <= 24064 < 2^24 and, with |x0| <= 1000, every residual result an integer below 2^15: exact in
    the accumulator, in both residual formats, and changed by any permutation of rows, columns or fragments.  ``normal``:
    N(0, 1) for A and N(0, 1 / K) for W; a gated-GELU operand has its gate rows scaled so that the gate accumulator has std
    GEGLU_GATE_STDS[f % 4]."""
    rng = np.random.default_rng([seed, M, N, K, int(geglu), 0 if kind == "integer" else 1])
    if kind == "integer":
        A = rng.integers(-4, 5, (M, K)).astype(np.float64)
        W = rng.integers(-4, 5, (N, K)).astype(np.float64)
        x0 = rng.integers(-1000, 1001, (M, N)).astype(np.float64)
    else:
        A = bf16_round(rng.standard_normal((M, K)))
        W = rng.standard_normal((N, K)) / np.sqrt(K)
        if geglu:
            F = N // 2
            std = np.asarray(GEGLU_GATE_STDS)[np.arange(F) % 4]
            W = interleave_geglu(W[:F] * std[:, None], W[F:])
        W = bf16_round(W)
        x0 = x24_round(rng.standard_normal((M, N)) * 3.0)
    for x in (A, W, x0):
        x.setflags(write=False)
    return A, W, x0


@functools.lru_cache(maxsize=8)
def gemm_products(M: int, N: int, K: int, kind: str, geglu: bool = False, seed: int = 0):
    """-> (P, S) = (A W^T, |A| |W|^T) of gemm_operands, float64 [M, N]."""
    A, W, _ = gemm_operands(M, N, K, kind, geglu, seed)
    P, S = A @ W.T, np.abs(A) @ np.abs(W).T
    P.setflags(write=False)
    S.setflags(write=False)
    return P, S


def x24_round(x) -> np.ndarray:
    """float64 -> the fp32 value the 24-bit form holds (the fp32 word rounded to its top 24 bits, half away from zero)."""
    _, hi, ext = hh.split_x24(torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(1, -1))
    return hh.merge_x24(hi, ext).numpy().astype(np.float64).reshape(np.shape(x))


def split_x24_np(x) -> Tuple[np.ndarray, np.ndarray]:
    """fp32 values [M, N] -> (bf16 plane as uint16 bits, biased extension bytes)."""
    _, hi, ext = hh.split_x24(torch.from_numpy(np.ascontiguousarray(x, np.float32)))
    return hi.view(torch.int16).numpy().view(np.uint16).copy(), ext.numpy().copy()


def merge_x24_np(hi_bits: np.ndarray, ext: np.ndarray) -> np.ndarray:
    hi = torch.from_numpy(np.ascontiguousarray(hi_bits).view(np.int16)).view(torch.bfloat16)
    return hh.merge_x24(hi, torch.from_numpy(np.ascontiguousarray(ext))).numpy().astype(np.float64)


def split_planes_np(x) -> Tuple[np.ndarray, np.ndarray]:
    """fp32 values -> (hi, lo) planes as float64 values of bf16."""
    pl = hh.split_planes(torch.from_numpy(np.ascontiguousarray(x, np.float32)))
    return pl[0].float().numpy().astype(np.float64), pl[1].float().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM references and bars
# ---------------------------------------------------------------------------------------------------------------------------
def acc_bar(S, K: int):
    return (K // 16 + 16) * U32 * S


def bf16_half_ulp(ref, err=0.0):
    """Half a bf16 ulp at a value within ``err`` of ``ref`` (8 significant bits; normal range)."""
    a = np.maximum(np.abs(ref) + err, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 8)


def rs_reference(ssp, inv_d: float, eps: float = EPS):
    """rowscale_kernel / RowScaleFromSlots / embed_copy_kernel's rs_out in float64: ssp [np, rows] -> rs [rows]."""
    return 1.0 / np.sqrt(np.asarray(ssp, np.float64).sum(0) * inv_d + eps)


def rs_rel_bar(np_: int) -> float:
    """Relative: np - 1 adds in index order, one fma, v_rsq_f32 (1 ulp)."""
    return (np_ + 3) * U32


def gelu_new(u):
    return 0.5 * u * (1.0 + np.tanh(0.7978845608028654 * (u + 0.044715 * u * u * u)))


def gelu_new_grad(u):
    c0, c1 = 0.7978845608028654, 0.044715
    th = np.tanh(c0 * (u + c1 * u ** 3))
    return 0.5 * (1.0 + th) + 0.5 * u * (1.0 - th * th) * c0 * (1.0 + 3.0 * c1 * u * u)


def geglu_split(P):
    """Accumulators [M, 2 F] over the interleaved rows -> (gate, up) [M, F]."""
    M, N2 = P.shape
    v = P.reshape(M, N2 // 64, 2, 32)
    return v[:, :, 0].reshape(M, N2 // 2), v[:, :, 1].reshape(M, N2 // 2)


def gemm_expected(epi: int, P, S, K: int, x0=None, rs=None, rs_rel: float = 0.0, extra: Optional[float] = None,
                  exact_acc: bool = False, mutant: Optional[str] = None, round_out: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ref, bar), float64 [M, n] (GEGLU: [M, n / 2]) from the products' first n columns.  rs: float64 [M] or None;
    ``rs_rel``: the relative error allowed to the kernel's own factor; exact_acc: the integer-operand cases (acc_bar = 0).
    round_out=False (STORE, GEGLU): the bar of the fp32 value in front of the bf16 rounding (a caller that scales it first).
    Mutants (the CPU test's planted bugs IN THE REFERENCE's place): "resid_overwrites", "geglu_up_row_plus_31",
    "rs_neighbour_row"."""
    e = np.zeros_like(S) if exact_acc else acc_bar(S, K)
    r = np.ones(P.shape[0]) if rs is None else np.asarray(rs, np.float64)
    if mutant == "rs_neighbour_row":
        r = np.roll(r, -1)
    r = r[:, None]
    if epi == EPI_STORE:
        ref = P * r
        pre = r * e + ((U32 + rs_rel) * np.abs(ref) if rs is not None else 0.0)  # (no factor: acc * 1 is exact)
        return ref, pre + (bf16_half_ulp(ref, pre) if round_out else 0.0)
    if epi in (EPI_RESID, EPI_RESID8):
        ref = P if mutant == "resid_overwrites" else x0 + P
        return ref, e + (U32 + (2.0 ** -17 if epi == EPI_RESID else 2.0 ** -16)) * (np.abs(ref) + e)
    g, u = geglu_split(P)
    eg, eu = geglu_split(e)
    if mutant == "geglu_up_row_plus_31":  # the up fragment taken 31 rows further on instead of 32
        u = np.concatenate([P[:, 31:], P[:, :31]], 1).reshape(P.shape[0], -1, 2, 32)[:, :, 0].reshape(u.shape)
    a0, a1 = g * r, u * r
    e0 = eg * r + (U32 + rs_rel) * np.abs(a0)
    e1 = eu * r + (U32 + rs_rel) * np.abs(a1)
    ref = gelu_new(a0) * a1
    d = np.maximum(np.abs(gelu_new_grad(a0 - e0)), np.abs(gelu_new_grad(a0 + e0)))
    d = np.maximum(d, np.abs(gelu_new_grad(a0)))
    pre = d * np.abs(a1) * e0 + np.abs(gelu_new(a0)) * e1 + 1.2 * e0 * e1 + (FASTMATH_ENC_GEGLU if extra is None else extra)
    return ref, pre + (bf16_half_ulp(ref, pre) if round_out else 0.0)


def ssp_reference(x_stored, np_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ssp [np, M], bar): per-64-feature sums of squares of x as stored; 8 fmas and a 3-step tree: 16 x 2^-24 of the sum."""
    M, n = x_stored.shape
    sq = np.zeros((M, np_out * 64))
    sq[:, :n] = np.asarray(x_stored, np.float64) ** 2
    s = sq.reshape(M, np_out, 64).sum(2).T
    return s, 16 * U32 * s


def findings(what: str, got, ref, bar, margins: Optional[Dict] = None) -> List[str]:
    """Every element within its bar; ``margins[what]`` keeps the worst |error| / bar met under that name."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    ok = np.isfinite(got) & (err <= bar)
    ratio = float(np.where(bar > 0, err / np.maximum(bar, 1e-300), np.where(err > 0, np.inf, 0.0)).max()) if err.size else 0.0
    if margins is not None:
        margins[what] = max(margins.get(what, 0.0), ratio if np.isfinite(got).all() else float("inf"))
    if ok.all():
        return []
    i = int(np.argmax(np.where(ok, -np.inf, np.where(np.isfinite(err), err - bar, np.inf))))
    return [f"{what}: {int((~ok).sum())} of {ok.size} elements beyond the bar; worst at {np.unravel_index(i, err.shape)}: got "
            f"{got.flat[i]:.6e}, ref {ref.flat[i]:.6e}, bar {np.broadcast_to(bar, err.shape).flat[i]:.3e}"]


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM stand-in: float32 where the kernel rounds (tests/test_encoder_forward_kernels_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def standin_acc(A, W, tokens_valid: int = 0, mutant: Optional[str] = None) -> np.ndarray:
    """The accumulators as the MFMA chain forms them: K / 16 steps, each the exact sum of 16 products added to the fp32
    accumulator with one rounding.  tokens_valid: rows from it on read the last valid row (the operand's row clamp).  Mutant
    "no_row_replication": they read their own rows."""
    A = np.asarray(A, np.float64)
    if 0 < tokens_valid < A.shape[0] and mutant != "no_row_replication":
        A = np.concatenate([A[:tokens_valid], np.repeat(A[tokens_valid - 1:tokens_valid], A.shape[0] - tokens_valid, 0)])
    acc = np.zeros((A.shape[0], W.shape[0]))
    for k in range(0, A.shape[1], 16):
        acc = _f32(acc + A[:, k:k + 16] @ W[:, k:k + 16].T)
    return acc


def standin_epilogue(epi: int, acc, x0=None, rs=None, np_out: int = 0, mutant: Optional[str] = None):
    """-> the values the kernel's store leaves (float64 of bf16 / of the decoded planes) and, for the residual forms, ssp.
    Mutants: "resid_overwrites", "geglu_up_row_plus_31", "rs_neighbour_row", "drop_last_half_slot"."""
    r = np.ones(acc.shape[0]) if rs is None else _f32(rs)
    if mutant == "rs_neighbour_row":
        r = np.roll(r, -1)
    r = r[:, None]
    if epi == EPI_STORE:
        return bf16_round(_f32(acc * r)), None
    if epi in (EPI_RESID, EPI_RESID8):
        v = _f32(acc if mutant == "resid_overwrites" else x0 + acc)
        if epi == EPI_RESID8:
            x = x24_round(v)
        else:
            hi, lo = split_planes_np(v)
            x = hi + lo
        ssp = None
        if np_out:
            ssp = _f32(ssp_reference(x, np_out)[0])
            if mutant == "drop_last_half_slot" and x.shape[1] % 64:
                ssp[-1] = 0.0
        return x, ssp
    g, u = geglu_split(acc)
    if mutant == "geglu_up_row_plus_31":
        u = np.concatenate([acc[:, 31:], acc[:, :31]], 1).reshape(acc.shape[0], -1, 2, 32)[:, :, 0].reshape(u.shape)
    a0, a1 = _f32(g * r), _f32(u * r)
    return bf16_round(_f32(_f32(gelu_new(a0)) * a1)), None


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
MIXED_LENS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 700)
SHORT_LENS = tuple(int(x) for x in np.random.default_rng(1).integers(1, 150, 1300))
# name -> (H, max_distance, std of the logits, lengths)
ATTENTION_CASES = {
    "h1-d8-std4-mixed": (1, 8, 4.0, MIXED_LENS),
    "h2-d32-std12-mixed": (2, 32, 12.0, MIXED_LENS),
    "h6-d128-std4-mixed": (6, 128, 4.0, MIXED_LENS),
    "h12-d447-std4-mixed": (12, 447, 4.0, MIXED_LENS),
    "h2-d128-std4-2048": (2, 128, 4.0, (2048, 33)),
    "h1-d447-std12-2048": (1, 447, 12.0, (2048,)),
    "h2-d32-std4-700": (2, 32, 4.0, (700,)),
    "h2-d8-std12-short": (2, 8, 12.0, SHORT_LENS),
}
ATT_TAB_MAX = 1024


@functools.lru_cache(maxsize=4)
def attention_case(name: str, seed: int = 5) -> Dict:
    """qkv [T, 3 H 64] float64 of bf16 values ([q | k | v], head-major), tab [H, 2 maxd + 1] fp32 values, one independent value
    per distance (a table expanded from buckets is constant from max_distance on and hides a clamp one entry early)."""
    H, maxd, std, lens = ATTENTION_CASES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    return make_attention_case(rng, H, maxd, std, lens, name)


def make_attention_case(rng, H, maxd, std, lens, name="") -> Dict:
    T, inner = int(sum(lens)), H * 64
    s = math.sqrt(std / 8.0)  # q . k over 64 dimensions of N(0, s^2) x N(0, s^2): std 8 s^2
    qkv = np.concatenate([rng.standard_normal((T, 2 * inner)) * s, rng.standard_normal((T, inner))], 1)
    tab = rng.standard_normal((H, 2 * maxd + 1)).astype(np.float32).astype(np.float64)
    return dict(name=name, H=H, maxd=maxd, lens=tuple(lens), cu=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                qkv=bf16_round(qkv), tab=tab, T=T)


def late_jump_case() -> Dict:
    """One query row whose running maximum jumps at a late key tile: key 300 of 320 dominates query 7 (logit 256)."""
    rng = np.random.default_rng(77)
    c = make_attention_case(rng, 1, 32, 0.7, (320,), "late-jump")
    qkv = c["qkv"].copy()
    qkv[7, :64] = 2.0
    qkv[300, 64:128] = 2.0
    c["qkv"] = qkv
    return c


def sub_attention_case(c: Dict, b: int) -> Dict:
    """Sequence b of a case alone."""
    s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
    return dict(c, lens=(s1 - s0,), cu=np.array([0, s1 - s0], np.int32), qkv=c["qkv"][s0:s1], T=s1 - s0)


def attention_reference(c: Dict, mutant: Optional[str] = None):
    """-> (ref, lead, fp32) float64 [T, H 64]: the exact result, the leading term of the bar 2^-8 sum_j p_j |v_j| / sum_j p_j,
    and the fp32 terms (module docstring).  Mutants: "bias_off_by_one" (tab index + 1), "clamp_one_early" (the distance clamped
    at maxd - 1), "mask_le_len" (key `len` admitted: the next row of the packed operand), "bias_sign" (i - j)."""
    H, maxd, qkv, tab, cu = c["H"], c["maxd"], c["qkv"], c["tab"], c["cu"]
    inner = H * 64
    T = qkv.shape[0]
    if mutant == "mask_le_len":  # (behind the last sequence: a row of ones where the GPU test keeps its NaN guard)
        qkv = np.concatenate([qkv, np.ones((1, qkv.shape[1]))])
    ref, lead, f32 = np.zeros((T, inner)), np.zeros((T, inner)), np.zeros((T, inner))
    LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
    for b in range(len(cu) - 1):
        s0, s1 = int(cu[b]), int(cu[b + 1])
        L = s1 - s0
        if L == 0:
            continue
        k1 = s1 + 1 if mutant == "mask_le_len" else s1
        i, j = np.arange(L)[:, None], np.arange(k1 - s0)[None, :]
        rel = (i - j) if mutant == "bias_sign" else (j - i)
        md = maxd - 1 if mutant == "clamp_one_early" else maxd
        idx = np.clip(rel, -md, md) + maxd + (1 if mutant == "bias_off_by_one" else 0)
        idx = np.minimum(idx, 2 * maxd)
        n_tiles = (L + 63) // 64
        heads = lambda part, rows: qkv[rows, part * inner:(part + 1) * inner].reshape(-1, H, 64).transpose(1, 0, 2)  # noqa: E731
        q, k, v = heads(0, slice(s0, s1)), heads(1, slice(s0, k1)), heads(2, slice(s0, k1))  # [H, rows, 64]
        s = q @ k.transpose(0, 2, 1) + tab[:, idx]
        m = s.max(2, keepdims=True)
        p = np.exp(s - m)
        l = p.sum(2, keepdims=True)
        o = (p @ v) / l
        av = (p @ np.abs(v)) / l
        # relative error of p_ij: ln 2 x the error of its exponent t = (s - m) log2 e - the score's chain of 4 MFMA steps and
        # the table add, the fma's and the maximum's roundings, the rescales on the way to the final maximum (bounded by |t|)
        # - and v_exp_f32's ulp per tile passed
        es = (4 + 16) * U32 * (np.abs(q) @ np.abs(k).transpose(0, 2, 1)) + U32 * np.abs(s)
        t = np.abs(s - m) * LOG2E
        relp = LN2 * (U32 * (3 * t + (2 * np.abs(m) + np.abs(s)) * LOG2E) + es * LOG2E) + (n_tiles + 2) * 2 * U32
        pr = p * relp
        chain = (5 * n_tiles + 16 + 3) * U32 * (1 + 2.0 ** -8) * av + (32 * n_tiles + 2) * U32 * np.abs(o)
        fp = (pr @ np.abs(v) + np.abs(o) * pr.sum(2, keepdims=True)) / l + chain
        back = lambda a: a.transpose(1, 0, 2).reshape(L, inner)  # noqa: E731
        ref[s0:s1], lead[s0:s1], f32[s0:s1] = back(o), 2.0 ** -8 * back(av), back(fp)
    return ref, lead, f32


def attention_bar(ref, lead, f32):
    pre = lead + f32
    return pre + bf16_half_ulp(ref, pre)


def attention_findings(name: str, got, ref, lead, f32, margins: Optional[Dict] = None) -> List[str]:
    """Per element within attention_bar; recorded: max |error|, relative L2, worst row, worst |error| / bar, and the excess
    beyond one rounding (|error| - lead - half an output ulp, at most) against the fp32 terms there."""
    got = np.asarray(got, np.float64)
    bar = attention_bar(ref, lead, f32)
    found = findings(name, got, ref, bar)
    err = np.abs(got - ref)
    exc = err - lead - bf16_half_ulp(ref, lead + f32)
    i = int(np.argmax(exc)) if exc.size else 0
    if margins is not None and err.size:
        margins[name] = dict(max_abs_error=float(err.max()), rel_l2=rel_l2(got, ref), worst_row=worst_row(got, ref),
                             worst_error_over_bar=float((err / bar).max()), excess_beyond_one_rounding=float(exc.flat[i]),
                             fp32_bar_there=float(f32.flat[i]))
    return found


def standin_attention(c: Dict, mutant: Optional[str] = None) -> np.ndarray:
    """The kernel's schedule in float32: 64-key tiles, the running maximum, p = exp2 in fp32, the row sum over the unrounded p,
    P V over p rounded to bf16, rescales by alpha, bf16(o / l).  Mutants as attention_reference's."""
    H, maxd, qkv, tab, cu = c["H"], c["maxd"], c["qkv"], c["tab"], c["cu"]
    inner = H * 64
    T = qkv.shape[0]
    if mutant == "mask_le_len":
        qkv = np.concatenate([qkv, np.ones((1, qkv.shape[1]))])
    out = np.zeros((T, inner))
    LOG2E = float(np.float32(1.4426950408889634))
    for b in range(len(cu) - 1):
        s0, s1 = int(cu[b]), int(cu[b + 1])
        L = s1 - s0
        k1 = s1 + 1 if mutant == "mask_le_len" else s1
        heads = lambda part, rows: qkv[rows, part * inner:(part + 1) * inner].reshape(-1, H, 64).transpose(1, 0, 2)  # noqa: E731
        q = heads(0, slice(s0, s1))
        m_run, l_run, o = np.full((H, L, 1), -np.inf), np.zeros((H, L, 1)), np.zeros((H, L, 64))
        md = maxd - 1 if mutant == "clamp_one_early" else maxd
        for k0 in range(s0, k1, 64):
            ke = min(k0 + 64, k1)
            k, v = heads(1, slice(k0, ke)), heads(2, slice(k0, ke))
            i, j = np.arange(L)[:, None], np.arange(k0 - s0, ke - s0)[None, :]
            rel = (i - j) if mutant == "bias_sign" else (j - i)
            idx = np.minimum(np.clip(rel, -md, md) + maxd + (1 if mutant == "bias_off_by_one" else 0), 2 * maxd)
            s = _f32(_f32(q @ k.transpose(0, 2, 1)) + tab[:, idx])
            m_new = np.maximum(m_run, s.max(2, keepdims=True))
            p = _f32(np.exp2(_f32(s * LOG2E - _f32(m_new * LOG2E))))
            alpha = _f32(np.exp2(_f32((m_run - m_new) * LOG2E)))
            l_run = _f32(_f32(l_run * alpha) + _f32(p.sum(2, keepdims=True)))
            o = _f32(_f32(o * alpha) + bf16_round(p) @ v)
            m_run = m_new
        out[s0:s1] = bf16_round(_f32(o * _f32(1.0 / l_run))).transpose(1, 0, 2).reshape(L, inner)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# embedding rows, last_hidden_state rows, rowscale
# ---------------------------------------------------------------------------------------------------------------------------
EMBED_DS = (64, 512, 1472, 1536, 1568, 2048)
EMBED_VOCAB = 384
ROWSCALE_ROWS = (1, 63, 64, 65, 260)
ROWSCALE_NPS = (1, 23, 24, 32)


def embed_table(D: int, V: int = EMBED_VOCAB, seed: int = 3) -> np.ndarray:
    """fp32 [V, D]: rows of differing scale, one zero row, one of magnitude 1e4."""
    rng = np.random.default_rng([seed, D])
    t = (rng.standard_normal((V, D)) * np.exp(rng.uniform(-2.0, 2.0, (V, 1)))).astype(np.float32)
    t[5] = 0.0
    t[6] *= np.float32(1e4) / np.abs(t[6]).max()
    return t


def embed_ids(T: int, V: int = EMBED_VOCAB, seed: int = 9) -> np.ndarray:
    """ids that repeat, and -1, V, V + 1000, -2^31 (clamped to [0, V - 1]) among them, the last row included."""
    rng = np.random.default_rng([seed, T])
    ids = rng.integers(0, V, T).astype(np.int64)
    for pos, bad in zip((0, T // 3, T // 2, T - 1), (-1, V, V + 1000, -2 ** 31)):
        ids[pos] = bad
    ids[min(1, T - 1)] = V - 1 if T > 4 else ids[min(1, T - 1)]
    return ids.astype(np.int32)


def embed_table_reference(table: np.ndarray):
    """The host's 24-bit encoding of the table: (hi bits uint16 [V, D], ext uint8 [V, D], x as stored float64)."""
    hi, ext = split_x24_np(table)
    return hi, ext, merge_x24_np(hi, ext)


def embed_ss_standin(x) -> np.ndarray:
    """embed_kernel<true>'s row statistic to the bit: lane l of the row's wave takes the 8-feature pieces l, l + 64, .. and
    chains ss = fma(x, x, ss) over their elements in order, then the xor butterfly 32, 16, .., 1.  x: the values as stored (16
    significant bits, so x^2 + ss is exact in float64 before its one rounding to fp32)."""
    V, D = x.shape
    nv = D // 8
    pieces = np.zeros((V, (nv + 63) // 64 * 64, 8))
    pieces[:, :nv] = np.asarray(x, np.float64).reshape(V, nv, 8)
    pieces = pieces.reshape(V, -1, 64, 8)
    ss = np.zeros((V, 64))
    for step in range(pieces.shape[1]):
        for e in range(8):
            ss = _f32(pieces[:, step, :, e] ** 2 + ss)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = _f32(ss + ss[:, lanes ^ o])
    return ss[:, 0].astype(np.float32)


def embed_rows_reference(ids, V: int, T: int, Tp: int, t_live: Optional[int] = None):
    """-> (row of the table per written output row [rows_written], rows_written): rows < T' take clamp(ids), rows T' ..
    rows_written token 0 (the kernel's contract); T' = t_live when the count is known on the device only, and then
    rows_written = min(Tp, t_live rounded up to 256)."""
    Tl = T if t_live is None else t_live
    rows = Tp if t_live is None else min(Tp, (t_live + 255) & ~255)
    src = np.zeros(rows, np.int64)
    n = min(Tl, rows)
    src[:n] = np.clip(np.asarray(ids[:n], np.int64), 0, V - 1)
    return src, rows


def hidden_out_reference(x, rs, w):
    """-> (ref, bar): w (x rs) in float64; two fp32 products and one bf16 rounding."""
    ref = np.asarray(w, np.float64)[None, :] * (np.asarray(x, np.float64) * np.asarray(rs, np.float64)[:, None])
    pre = 2 * U32 * np.abs(ref)
    return ref, pre + bf16_half_ulp(ref, pre)
