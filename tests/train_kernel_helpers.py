"""Float64 restatements of the encoder's training weight-gradient kernel (wgrad_kernel with its two epilogue forms, in one- and
two-product launches) and of four of the training step's GEMM epilogues (the RMSNorm-backward residual with its masked copy,
the gated-GELU backward, the training FFN-in epilogue, the training residual epilogue) and of the training attention forward and
backward (derivations in front of their sections below), for
tests/test_train_mfma_kernels_gpu.py (the kernels, through rp_dbg_wgrad_ex and rp_dbg_train_gemm) and
tests/test_train_mfma_kernels_cpu.py (the restatements against torch float64, a float32 stand-in of the kernel's schedule against
every bar, planted bugs against the same bars).  numpy float64, no GPU.  acc_bar, bf16_round and the finding / margin bookkeeping
are tests/encoder_forward_helpers.py's; the packed gate | up row map and the unfold restatement tests/encoder_kernel_helpers.py's.

wgrad  dW[o, c] = sum_t Y[t, o] X[t, c], operands bf16, read in rp_train_kernels.h (wgrad_kernel, wgrad_tile, EpiStoreF32):
  * split s of S reduces the token tiles [s nk / S, (s + 1) nk / S) (integer division, nk = T / 64) into a partial matrix of its
    own, out + s * ny * nx; nothing adds the partials (unfold_kernel does, later), so the comparison is per split: a boundary
    that moved by one tile leaves the sum of the partials unchanged;
  * element (o, c) of a partial is ONE token-ascending chain of v_mfma_f32_32x32x16_bf16 steps, four per 64-token tile, each
    adding 16 exact bf16 products to the fp32 accumulator, under both tile configurations (they differ in which wave holds
    the element, not in its chain), so with R = the rows of the split
        |acc - dW_s| <= (R / 16 + 16) 2^-24 sum_t |y x|                                      (encoder_forward_helpers.acc_bar)
    and the plain epilogue stores the accumulator as it stands;
  * integer operands in [-4, 4]: every partial sum in any order is an integer of magnitude <= 16 T <= 16384 < 2^24 at T <= 1024,
    exact in fp32, so the partial matrices equal float64 to the bit;
  * the operands' feature columns are fetched in 8-column pieces at min(piece, n - 8): a piece beyond the matrix edge repeats
    the last one and lands in accumulator rows / columns that are not stored.  Without the clamp the same accumulators would
    hold what lies behind column n instead - no stored element changes, the fault is the read itself - so the stand-in
    fetches through a loader that counts the columns read at or beyond n (StandinReads), and the GPU test fills the columns
    n .. ld with NaN and lets the arenas' guards stand behind the last row.

The finishing epilogue (EpiStoreF32 with WgradFinish: the first product of a split-free launch, ny % 64 == 0; the rows of Y are
the packed order of wi_0 / wi_1, blocks of 32 gate rows then the same 32 up rows):
  * g[sr, c] = acc * ln[c], ONE fp32 product on the accumulator, sr = (o >> 6) * 32 + (o & 31), gate rows to `out`, up rows to
    g1:   |g - ref| <= e |ln| + 2^-24 (|ref| + e |ln|)   with e the accumulator's bar.
    unfold_kernel's GEGLU mode on the plain launch's one partial computes s = 0 + v (exact; an accumulator is never -0: it
    starts at +0 and round-to-nearest sums give -0 only from two -0 terms) and then `s * ln`, the same single product: the
    finishing launch's g0 / g1 must have rp_dbg_unfold's BITS.  With an exact accumulator g = fp32(acc ln) to the bit (the
    product of two fp32 values is exact in float64);
  * dln_part[o >> 5][c] = sum over the block's 32 rows of acc w[sr, c]: each half-wave chains dl = fma(acc, w, dl) over its 16
    rows (one rounding per step), then one add across the half-waves: 17 roundings, each of a partial sum bounded by
    sum |acc w|, second-order terms under one more:
        |dln_part - ref| <= sum_r e_r |w_r| + 18 x 2^-24 sum_r (|acc_r| + e_r) |w_r|.
    unfold_kernel chains 8 rows per wave and adds four waves in a tree - another order, so only the bound is asserted.  Integer
    masters in [-4, 4]: |sum| <= 32 x 4 x 16 T < 2^24 at T <= 1024, so dln_part is exact too.

The launch plans (plan_wgrad / plan_wgrad_pair, rp_train.hip) are restated in plan_wgrad / plan_wgrad_pair below; the CPU test
holds rp_dbg_wgrad_plan to them over a grid and pins the forms at the ByT5-small / base training geometries."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import encoder_forward_helpers as ef
import encoder_kernel_helpers as ek
from encoder_forward_helpers import U32, acc_bar, bf16_round, findings  # noqa: F401  (re-exported)

CFG_TILE = {0: 256, 1: 128}  # tile configuration -> features per tile side
WGRAD_TS = (64, 128, 192, 256, 320, 512, 1024)  # 1, 2, 3, 4, 5, 8, 16 token tiles: the 2-stage ring wraps zero, one, several times
WGRAD_SPLITS = (1, 2, 3, 5)
WGRAD_NS = (8, 64, 72, 120, 128, 136, 200, 256, 264, 384)  # the n - 8 clamp one piece before, at and after a 64 / 128 / 256 edge
# (ny, nx, ldy - ny, ldx - nx) per token count: every width of WGRAD_NS is an ny and an nx somewhere, every pitch form both ways
WGRAD_SHAPES = {
    64: ((8, 384, 0, 8), (64, 264, 24, 0), (384, 8, 8, 24), (136, 200, 0, 0)),
    128: ((72, 256, 8, 0), (120, 136, 0, 24), (264, 64, 24, 8)),
    192: ((128, 120, 0, 0), (200, 72, 8, 8), (256, 128, 24, 24)),
    256: ((136, 128, 24, 0), (384, 264, 0, 8), (8, 8, 8, 24)),
    320: ((200, 200, 0, 24), (256, 72, 8, 0), (64, 120, 24, 8)),
    512: ((264, 136, 8, 8), (128, 384, 0, 0), (72, 64, 24, 24)),
    1024: ((120, 256, 24, 0), (384, 384, 0, 8), (264, 8, 8, 0)),
}
PLACEMENT_TOKENS = (0, 7, 8, 63, 64, -1)                 # -1: the last one
PLACEMENT_FEATURES = (0, 31, 32, 127, 128, 255, 256, -1)
FINISH_NYS = (64, 128, 320, 576)   # ny = 2 F
FINISH_NXS = (8, 72, 256, 264)
# (product 0, product 1) as (ny, nx): different shapes; the second smaller than one tile in the second case
PAIR_SHAPES = (((384, 264), (264, 200)), ((320, 136), (72, 120)), ((8, 264), (264, 8)))


def split_ranges(T: int, S: int, mutant: Optional[str] = None) -> List[Tuple[int, int]]:
    """Token rows [r0, r1) of every split.  Mutant "split_boundary_up": the boundaries rounded up instead of down."""
    nk = T // 64
    cut = (lambda s: -(-s * nk // S)) if mutant == "split_boundary_up" else (lambda s: s * nk // S)
    return [(cut(s) * 64, cut(s + 1) * 64) for s in range(S)]


@functools.lru_cache(maxsize=16)
def wgrad_operands(T: int, ny: int, nx: int, kind: str, seed: int = 0):
    """Y [T, ny], X [T, nx] float64 arrays of bf16 values: ``integer`` in [-4, 4], ``normal`` N(0, 1)."""
    rng = np.random.default_rng([seed, T, ny, nx, 0 if kind == "integer" else 1])
    if kind == "integer":
        Y, X = rng.integers(-4, 5, (T, ny)).astype(np.float64), rng.integers(-4, 5, (T, nx)).astype(np.float64)
    else:
        Y, X = bf16_round(rng.standard_normal((T, ny))), bf16_round(rng.standard_normal((T, nx)))
    Y.setflags(write=False)
    X.setflags(write=False)
    return Y, X


def wgrad_reference(Y, X, S: int, exact: bool = False, mutant: Optional[str] = None):
    """-> (ref, bar) float64 [S, ny, nx]: the partial matrix of every split and its accumulator bar (zero: exact)."""
    ref, bar = [], []
    for r0, r1 in split_ranges(Y.shape[0], S, mutant):
        ref.append(Y[r0:r1].T @ X[r0:r1])
        bar.append(np.zeros_like(ref[-1]) if exact else acc_bar(np.abs(Y[r0:r1]).T @ np.abs(X[r0:r1]), r1 - r0))
    return np.stack(ref), np.stack(bar)


@functools.lru_cache(maxsize=8)
def finish_operands(F: int, nx: int, kind: str, seed: int = 0):
    """w0, w1 fp32 [F, nx] (``integer``: in [-4, 4]) and ln fp32 [nx] (1 + 0.2 N(0, 1) in both kinds)."""
    rng = np.random.default_rng([seed, F, nx, 7])
    if kind == "integer":
        w0, w1 = (rng.integers(-4, 5, (F, nx)).astype(np.float32) for _ in range(2))
    else:
        w0, w1 = (rng.standard_normal((F, nx)).astype(np.float32) for _ in range(2))
    return w0, w1, (1.0 + 0.2 * rng.standard_normal(nx)).astype(np.float32)


def finish_reference(acc, e, w0, w1, ln):
    """acc, e float64 [2 F, nx] (the packed product and its accumulator bar) -> {name: (ref, bar)} for g0, g1 [F, nx] and
    dln_part [2 F / 32, nx]."""
    rows, nx = acc.shape
    w64 = [np.asarray(w0, np.float64), np.asarray(w1, np.float64)]
    ln64 = np.asarray(ln, np.float64)
    g, dln = ek.unfold_reference(acc[None], ek.UNFOLD_GEGLU, 0, w64, ln64)
    ge, _ = ek.unfold_reference(e[None], ek.UNFOLD_GEGLU, 0, w64, np.abs(ln64))
    out = {f"g{k}": (g[k], ge[k] + U32 * (np.abs(g[k]) + ge[k])) for k in range(2)}
    wp = np.abs(ek.repack_reference(ek.PACK_GEGLU, w64, rows, 0))
    signed = ek.repack_reference(ek.PACK_GEGLU, w64, rows, 0)
    ref = (acc * signed).reshape(rows // 32, 32, nx).sum(1)
    bar = (e * wp).reshape(rows // 32, 32, nx).sum(1) + 18 * U32 * ((np.abs(acc) + e) * wp).reshape(rows // 32, 32, nx).sum(1)
    out["dln_part"] = (ref, bar)
    assert np.abs(ref.sum(0) - dln).max() <= 1e-9 * max(1.0, np.abs(dln).max())  # the blocks add up to unfold_reference's d ln
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plans, restated (rp_train.hip: plan_wgrad, plan_wgrad_pair)
# ---------------------------------------------------------------------------------------------------------------------------
_CU_RATE, _PART_BW = 1.0e15 / 256, 4.0e12


def _plan_wgrad(rows: int, cols: int, nk: int) -> Tuple[int, int, float]:
    best = (0, 1, 1e30)
    for cfg in range(2):
        b, slots = (256, 256) if cfg == 0 else (128, 512)
        rate = _CU_RATE if cfg == 0 else _CU_RATE * 0.7 / 2
        tiles = ((rows + b - 1) // b) * ((cols + b - 1) // b)
        s = 1
        while s <= 32 and s * 4 <= max(nk, 4):
            rounds = (tiles * s + slots - 1) // slots
            t_wg = 2.0 * b * b * 64.0 * ((nk + s - 1) // s) / rate
            t_part = 2.0 * s * float(rows) * cols * 4 / _PART_BW if s > 1 else 0.0
            tt = rounds * t_wg + t_part + 3e-6
            if tt < best[2]:
                best = (cfg, s, tt)
            s += 1
    return best


def plan_wgrad(rows: int, cols: int, nk: int) -> Tuple[int, int]:
    """-> (cfg, splits)."""
    return _plan_wgrad(rows, cols, nk)[:2]


def plan_wgrad_pair(rows0: int, cols0: int, rows1: int, cols1: int, nk: int) -> Tuple[int, int]:
    """-> (cfg, splits); splits = 0: the model prefers separate launches."""
    tiles = ((rows0 + 255) // 256) * ((cols0 + 255) // 256) + ((rows1 + 255) // 256) * ((cols1 + 255) // 256)
    best = (0, 0, _plan_wgrad(rows0, cols0, nk)[2] + _plan_wgrad(rows1, cols1, nk)[2])
    s = 1
    while s <= 32 and s * 4 <= max(nk, 4):
        rounds = (tiles * s + 255) // 256
        t_wg = 2.0 * 256 * 256 * 64.0 * ((nk + s - 1) // s) / _CU_RATE
        t_part = 2.0 * s * (float(rows0) * cols0 + float(rows1) * cols1) * 4 / _PART_BW if s > 1 else 0.0
        tt = rounds * t_wg + t_part + 3e-6
        if tt < best[2]:
            best = (0, s, tt)
        s += 1
    return best[:2]


# ---------------------------------------------------------------------------------------------------------------------------
# stand-in: float32 where the kernel rounds (tests/test_train_mfma_kernels_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
_f32 = ef._f32


class StandinReads:
    """What the stand-in's loader fetched outside an operand's live columns (8-column pieces at or beyond n)."""

    def __init__(self):
        self.outside = 0


def _load(mem, n: int, rows: slice, feat0: int, width: int, clamp: bool, reads: Optional[StandinReads]):
    """The tile's operand image [rows, width] from the padded matrix ``mem`` [T, ld >= n] (NaN beyond column n and, behind the
    last row, nothing: a read there is counted and returns NaN), in 8-column pieces at min(piece, n - 8)."""
    T, ld = mem.shape
    flat = np.concatenate([mem.reshape(-1), np.full(width + 8, np.nan)])
    img = np.empty((rows.stop - rows.start, width))
    for p in range(0, width, 8):
        f = min(feat0 + p, n - 8) if clamp else feat0 + p
        if f + 8 > n and reads is not None:
            reads.outside += 1
        idx = (np.arange(rows.start, rows.stop) * ld + f)[:, None] + np.arange(8)[None, :]
        img[:, p:p + 8] = flat[np.minimum(idx, flat.size - 1)]
    return img


def standin_wgrad(Ym, ny: int, Xm, nx: int, S: int, cfg: int, mutant: Optional[str] = None,
                  reads: Optional[StandinReads] = None) -> np.ndarray:
    """The partial matrices [S, ny, nx] as wgrad_kernel forms them: per tile of CFG_TILE[cfg] features a side the operand images
    fetched in clamped 8-column pieces, the accumulator one chain of 16-token MFMA steps over the split's rows, elements inside
    the matrix stored.  Ym [T, ldy], Xm [T, ldx]: the padded operands.  Mutants: "split_boundary_up", "no_feature_clamp"."""
    B = CFG_TILE[cfg]
    out = np.full((S, ny, nx), np.nan)
    clamp = mutant != "no_feature_clamp"
    for s, (r0, r1) in enumerate(split_ranges(Ym.shape[0], S, mutant)):
        for m0 in range(0, ny, B):
            a = _load(Ym, ny, slice(r0, r1), m0, B, clamp, reads)
            for n0 in range(0, nx, B):
                w = _load(Xm, nx, slice(r0, r1), n0, B, clamp, reads)
                acc = np.zeros((B, B))
                for k in range(0, r1 - r0, 16):
                    acc = _f32(acc + a[k:k + 16].T @ w[k:k + 16])
                mo, nc = min(B, ny - m0), min(B, nx - n0)
                out[s, m0:m0 + mo, n0:n0 + nc] = acc[:mo, :nc]
    return out


def mfma32_row(r, hi):
    return (r & 3) + 8 * (r >> 2) + 4 * hi


def standin_finish(acc, w0, w1, ln, mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """EpiStoreF32's finishing branch on fp32 accumulators [2 F, nx] -> g0, g1 [F, nx], dln_part [2 F / 32, nx].  Mutants:
    "gate_up_swapped", "sr0_one_group_late" (wrapping at the last group), "dln_other_half_dropped"."""
    rows, nx = acc.shape
    F = rows // 2
    g = [np.full((F, nx), np.nan), np.full((F, nx), np.nan)]
    w = [np.asarray(w0, np.float64), np.asarray(w1, np.float64)]
    ln = np.asarray(ln, np.float64)
    dln = np.full((rows // 32, nx), np.nan)
    for ob in range(0, rows, 32):
        up = (ob >> 5) & 1
        if mutant == "gate_up_swapped":
            up ^= 1
        grp = ob >> 6
        if mutant == "sr0_one_group_late":
            grp = (grp + 1) % (rows // 64)
        sr0 = grp * 32
        halves = []
        for hi in range(2):
            dl = np.zeros(nx)
            for r in range(16):
                row = mfma32_row(r, hi)
                v = acc[ob + row]
                g[up][sr0 + row] = _f32(v * ln)
                dl = _f32(v * w[up][sr0 + row] + dl)
            halves.append(dl)
        dln[ob >> 5] = halves[0] if mutant == "dln_other_half_dropped" else _f32(halves[0] + halves[1])
    return dict(g0=g[0], g1=g[1], dln_part=dln)


def padded(a, ld: int) -> np.ndarray:
    """[rows, n] -> [rows, ld] with NaN in the columns beyond n."""
    out = np.full((a.shape[0], ld), np.nan)
    out[:, :a.shape[1]] = a
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the training step's GEMM epilogues (rp_dbg_train_gemm): RMSNorm-backward residual, training FFN-in, training residual
# ---------------------------------------------------------------------------------------------------------------------------
# The GEMM core is the forward's (one K-ascending chain of K / 16 MFMA steps per element in every tile configuration: acc_bar).
#
# RMSNorm-backward residual (EpiRmsBwdResidT, hilo_update2):  d = fma(-rc, x, acc) is ONE rounding of acc - rc x (|.| <= |P| + e +
# |rc x|); v = (hi + lo) + d is one fp32 add (hi + lo itself is exact: the planes are the split of an fp32 value); hi' =
# bf16(v), lo' = bf16(v - hi'): |v - hi' - lo'| <= 2^-17 |v| - the forward RESID bar on top of the fma:
#     pre = e + 2^-24 (|P| + e + |rc x|);   |hi' + lo' - ref| <= pre + (2^-24 + 2^-17)(|ref| + pre);   hi' alone: one bf16 rounding.
# Integer operands (A, W, x in [-4, 4], old dx in [-1000, 1000], rc a signed power of two in [1/2, 2]): every value is a multiple of
# 1/2 below 1000 + 16 K + 8 < 2^15, exact in fp32 and in 16 bits across the planes: the planes are the host's split of float64.
# dxm is computed from the words just stored: bf16((f32(hi') + f32(lo')) * m), m = 0 or fp32 1 / (1 - p) - the host recomputes it
# from the planes and the mask read back, BIT FOR BIT; mask_dx_kernel on the same planes gives the same bits.
#
# Training FFN-in (EpiGegluTrainT): gu is EpiStoreBf16's store, ff the inference epilogue's geglu2 on the same accumulators -
# without dropout both have rp_dbg_gemm_ex's bits.  With dropout y m is one more fp32 product in front of the bf16 rounding:
#     |ff - ref m| <= m pre + 2^-24 |ref m| + half a bf16 ulp there      (pre: the forward GEGLU bar in front of its rounding)
# and ff is +-0 wherever m = 0.
# Training residual (EpiResidT<true>): the projection's output is masked, d = acc m (one product), then hilo_update2 as in the
# forward: the RESID bar with P m for P and m e + 2^-24 |P m| for e.
TG_GEGLU_BWD, TG_RMS_BWD, TG_GEGLU_TRAIN, TG_RESID_TRAIN = 0, 1, 2, 3
TG_MS = (256, 512)
RMS_NS = (8, 64, 72, 136, 192, 200, 256, 264, 448)  # 192: the edge tile d_model 1472 leaves
RMS_KS = (128, 192, 384)
FWD_FS = (64, 128, 192, 256, 320, 448)  # d_ff: tiles of 64, 128, 192 valid features, one and a half 256-tiles (N = 2 d_ff packed rows)
FWD_KS = (64, 128, 1472)
DROP_PS = (0.0, 0.1, 0.5)
SITE, OTHER_SITE = 16 + 8 * 3 + 1, 16 + 8 * 3 + 3  # a residual-branch site of layer 3 and the one the trainer masks next


def tg_variants(K: int) -> Tuple[int, ...]:
    return (0, 26) if K % 64 == 0 else (0,)


def drop_scale(p: float) -> float:
    """make_drop's multiplier: fp32 1 / (1 - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


@functools.lru_cache(maxsize=8)
def rms_operands(M: int, N: int, K: int, kind: str, seed: int = 0):
    """A [M, K], W [N, K] (ef.gemm_operands'), the old gradient x0 [M, N] (fp32 values that are the sum of their two planes), the
    saved input xs [M, N] (bf16 values), rcoef [M] (fp32 values)."""
    A, W, _ = ef.gemm_operands(M, N, K, kind, False, seed)
    rng = np.random.default_rng([seed, M, N, K, 11, 0 if kind == "integer" else 1])
    if kind == "integer":
        x0 = rng.integers(-1000, 1001, (M, N)).astype(np.float64)
        xs = rng.integers(-4, 5, (M, N)).astype(np.float64)
        rc = rng.choice([0.5, 1.0, 2.0, -1.0, -0.5], M)
    else:
        hi, lo = ef.split_planes_np(rng.standard_normal((M, N)) * 3.0)
        x0 = hi + lo
        xs = bf16_round(rng.standard_normal((M, N)))
        rc = (rng.standard_normal(M) * 0.3).astype(np.float32).astype(np.float64)
    for a in (x0, xs, rc):
        a.setflags(write=False)
    return A, W, x0, xs, rc


def rms_bwd_expected(P, S, K: int, x0, xs, rc, exact_acc: bool = False, mutant: Optional[str] = None):
    """-> (ref, bar, bar_hi) float64 [M, n].  Mutants (in the reference's place): "plus_rc_x", "rc_neighbour_row"."""
    n = x0.shape[1]
    P, S = P[:, :n], S[:, :n]
    r = np.roll(rc, -1) if mutant == "rc_neighbour_row" else np.asarray(rc)
    t = r[:, None] * xs
    ref = x0 + (P + t if mutant == "plus_rc_x" else P - t)
    e = np.zeros_like(S) if exact_acc else acc_bar(S, K)
    pre = e + U32 * (np.abs(P) + e + np.abs(t))
    bar = pre + (U32 + 2.0 ** -17) * (np.abs(ref) + pre)
    hi_pre = pre + U32 * (np.abs(ref) + pre)
    return ref, bar, hi_pre + ef.bf16_half_ulp(ref, hi_pre)


def dxm_expected(hi, lo, m) -> np.ndarray:
    """bf16((f32(hi) + f32(lo)) * m) as the kernels compute it, to the bit (float64 values of bf16)."""
    import torch
    h, l, mm = (torch.from_numpy(np.ascontiguousarray(a, np.float32)) for a in (hi, lo, m))
    return ((h + l) * mm).to(torch.bfloat16).float().numpy().astype(np.float64)


def standin_rms_bwd(acc, x0, xs, rc, m=None, m_wrong=None, mutant: Optional[str] = None):
    """-> (hi, lo, dxm or None).  Mutants: "plus_rc_x", "rc_neighbour_row", "dxm_before_update", "site_for_next_site" (the mask
    of another site, m_wrong)."""
    n = x0.shape[1]
    r = np.roll(rc, -1) if mutant == "rc_neighbour_row" else np.asarray(rc)
    t = r[:, None] * xs
    d = _f32(acc[:, :n] + t if mutant == "plus_rc_x" else acc[:, :n] - t)
    hi, lo = ef.split_planes_np(_f32(x0 + d))
    if m is None:
        return hi, lo, None
    h0, l0 = ef.split_planes_np(x0)
    sh, sl = (h0, l0) if mutant == "dxm_before_update" else (hi, lo)
    return hi, lo, dxm_expected(sh, sl, m_wrong if mutant == "site_for_next_site" else m)


def geglu_train_expected(P, S, K: int, rs=None, rs_rel: float = 0.0, m=None, exact_acc: bool = False):
    """-> (ref, bar) float64 [M, F] of ff; m: the multipliers [M, F] (None: no dropout - the forward's bar)."""
    if m is None:
        return ef.gemm_expected(ef.EPI_GEGLU, P, S, K, rs=rs, rs_rel=rs_rel, exact_acc=exact_acc)
    ref0, pre = ef.gemm_expected(ef.EPI_GEGLU, P, S, K, rs=rs, rs_rel=rs_rel, exact_acc=exact_acc, round_out=False)
    ref = ref0 * m
    pre_m = m * pre + U32 * np.abs(ref)
    return ref, np.where(m == 0, 0.0, pre_m + ef.bf16_half_ulp(ref, pre_m))


def standin_geglu_train(acc, rs=None, m=None, mutant: Optional[str] = None) -> np.ndarray:
    """ff as the epilogue forms it: gelu_new(rs g) (rs u) in fp32, times m, rounded to bf16.  Mutant "mask_one_column_over"."""
    r = (np.ones(acc.shape[0]) if rs is None else _f32(rs))[:, None]
    g, u = ef.geglu_split(acc)
    y = _f32(_f32(ef.gelu_new(_f32(g * r))) * _f32(u * r))
    if m is not None:
        y = _f32(y * (np.roll(m, 1, axis=1) if mutant == "mask_one_column_over" else m))
    return bf16_round(y)


def resid_train_expected(P, S, K: int, x0, m=None, exact_acc: bool = False):
    """-> (ref, bar, bar_hi) float64 [M, n] of the updated stream x0 + m P."""
    n = x0.shape[1]
    P, S = P[:, :n], S[:, :n]
    e = np.zeros_like(S) if exact_acc else acc_bar(S, K)
    if m is not None:
        P, e = P * m, m * e + U32 * np.abs(P * m)
    ref = x0 + P
    bar = e + (U32 + 2.0 ** -17) * (np.abs(ref) + e)
    hi_pre = e + U32 * (np.abs(ref) + e)
    return ref, bar, hi_pre + ef.bf16_half_ulp(ref, hi_pre)


def standin_resid_train(acc, x0, m=None, mutant: Optional[str] = None):
    """-> (hi, lo).  Mutant "mask_one_column_over"."""
    d = acc[:, :x0.shape[1]]
    if m is not None:
        d = _f32(d * (np.roll(m, 1, axis=1) if mutant == "mask_one_column_over" else m))
    return ef.split_planes_np(_f32(x0 + d))


def cpu_mask(M: int, n: int, p: float, seed: int) -> np.ndarray:
    """A stand-in for the engine's mask on the build machine: 0 or drop_scale(p), independent per element."""
    keep = np.random.default_rng([seed, M, n, int(p * 1000)]).random((M, n)) >= p
    return keep * drop_scale(p)


# ---------------------------------------------------------------------------------------------------------------------------
# gated-GELU backward (EpiGegluBwd, rp_dbg_train_gemm mode 0)
# ---------------------------------------------------------------------------------------------------------------------------
# dff = acc (times m under dropout: one product), g / u the SAVED bf16 pre-activations (exact inputs), read in EpiGegluBwd::run:
#   sg = rcp(1 + exp2(g (K2 g^2 + K1))) = sigmoid(2 z);  gelu = g sg;  gelu' = fma(g t, d2z, sg), t = fma(-sg, sg, sg), d2z = fma(..)
#   dy_g = (dff u) gelu',  dy_u = dff (g sg);   dzs = bf16(dy rs) in the packed order;   dot += fma(dy_g, g, fma(dy_u, u, dot))
# The accumulator bar e goes through linearly: e |u gelu'| and e |gelu|.  The fp32 evaluation rounds g^2, d2z, t, g t, the fma, dff u
# and the product (7; 8 taken; the exponent a = g fma(K2, g^2, K1) carries three roundings, 3 x 2^-24 |a|, which exp2 turns into a
# relative error of 3 x 2^-24 |2 z| of e^(-2 z), i.e. sg (1 - sg) times that on sg - it matters in the tails, where gelu and gelu'
# are tiny - and goes on through d gelu / d sg = g and d gelu' / d sg = 1 + g (1 - 2 sg) d2z) at magnitudes bounded by |dff u| (sg + |g t d2z|), and g sg and its product with dff (3 with the
# margin) at |dy_u|; dzs adds the product with rs and half a bf16 ulp.  What v_exp_f32 / v_rcp_f32 and the exponent's own
# rounding (amplified by |a| ln 2 before sg saturates) add cannot be derived: FASTMATH_GEGLU_BWD_* below, measured.
# The row dot adds the UNROUNDED products: per lane 8 fmas in 2-vectors and their sum, three DPP adds (12 roundings on a
# partial sum bounded by the slot's sum of |terms|), then launch_rowdot_finish: np - 1 adds in index order and three products
# (np + 3).  Under dropout everything is the reference with dff m, and where m = 0 both outputs are +-0.
# The `dot = 0` of a feature block at or beyond n_valid is covered by the `slot < np` guard whenever np = ceil(d_ff / 64), which is
# what every caller passes (the trainer, rp_dbg_dgrad, rp_dbg_train_gemm): the planted bug "row dot kept beyond n_valid" changes no
# result at that np, and the CPU test says so instead of pretending to catch it.
GB_FS = FWD_FS
GB_KS = (64, 128, 192, 320, 1472)
# twice the worst excess of |error| over the derived bar measured on the MI355X over GB_FS x GB_KS x p = 0, 0.1, 0.5 x variants 0,
# 26, gates of std 1, 3, 10, 30 by feature (profiles/train_kernel_margins.json, "geglu_bwd_fastmath_excess"); 0: no excess.
#   Measured: no excess.  The largest |error| - derived bar over all 180 calls is negative for both outputs: -2.0e-41 on dzs
#   (elements whose result is a flushed denormal), -1.7e-6 on rcoef (0.033 of its bar at worst); dzs reaches 0.9991 of its bar,
#   which is the bf16 rounding being attained.  v_exp_f32 and v_rcp_f32 stay inside the derived terms, so nothing is added.
GEGLU_BWD_DZS_EXCESS_MEASURED = 0.0
GEGLU_BWD_RCOEF_EXCESS_MEASURED = 0.0
FASTMATH_GEGLU_BWD_DZS = 2.0 * GEGLU_BWD_DZS_EXCESS_MEASURED
FASTMATH_GEGLU_BWD_RCOEF = 2.0 * GEGLU_BWD_RCOEF_EXCESS_MEASURED


@functools.lru_cache(maxsize=4)
def geglu_bwd_operands(M: int, F: int, K: int, seed: int = 0):
    """dx [M, K], Wo2^T [F, K] (dff ~ N(0, 1)), the saved gate / up [M, F] (bf16 values; gate std 1, 3, 10, 30 by feature), rs."""
    A, W, _ = ef.gemm_operands(M, F, K, "normal", False, seed + 100)
    rng = np.random.default_rng([seed, M, F, K, 23])
    g = bf16_round(rng.standard_normal((M, F)) * np.asarray(ef.GEGLU_GATE_STDS)[np.arange(F) % 4])
    u = bf16_round(rng.standard_normal((M, F)))
    rs = rng.uniform(0.5, 1.5, M).astype(np.float32).astype(np.float64)
    for a in (g, u, rs):
        a.setflags(write=False)
    return A, W, g, u, rs


def pack_gu(g, u) -> np.ndarray:
    """[M, F] gate and up -> the packed [M, 2 F]: per 64 columns 32 gate then the same 32 up."""
    M, F = g.shape
    return np.stack([g.reshape(M, F // 32, 32), u.reshape(M, F // 32, 32)], 2).reshape(M, 2 * F)


def geglu_bwd_expected(P, S, K: int, g, u, rs, m=None, extra_dzs: Optional[float] = None, extra_rcoef: Optional[float] = None):
    """-> dict: dzs_g, dzs_u (ref, bar) [M, F] and rcoef (ref, bar) [M] = rs^2 sum_f (dy_g g + dy_u u) / K."""
    F = g.shape[1]
    dff, e = P[:, :F], acc_bar(S[:, :F], K)
    if m is not None:
        dff = dff * m
        e = m * e + U32 * np.abs(dff)
    c0, c1 = 0.7978845608028654, 0.044715
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-2.0 * c0 * (g + c1 * g ** 3)))
    d2z = 2.0 * c0 * (1.0 + 3.0 * c1 * g * g)
    mag = sg + np.abs(g * sg * (1.0 - sg) * d2z)
    dsg = sg * (1.0 - sg) * 3.0 * np.abs(2.0 * c0 * (g + c1 * g ** 3)) * U32  # the exponent's three roundings through exp2
    # (the sigmoid form: 0.5 (1 + tanh z) = sigmoid(2 z) exactly, and it keeps its relative accuracy in the negative tail, where
    # 1 + tanh cancels to nothing in float64)
    gl, gp = g * sg, sg + g * sg * (1.0 - sg) * d2z
    dyg, dyu = dff * u * gp, dff * gl
    pg = e * np.abs(u * gp) + np.abs(dff * u) * (8 * U32 * mag + (1.0 + np.abs(g * d2z)) * dsg)
    pu = e * np.abs(gl) + 3 * U32 * np.abs(dyu) + np.abs(dff * g) * dsg
    # sg below 2^-120: exp2 overflows beyond a = 128 and v_rcp_f32 returns a flushed denormal or 0 ("g -> -inf gives -0", rp_util.h):
    # the whole (tiny) value may be lost
    flushed = sg < 2.0 ** -120
    pg, pu = pg + flushed * np.abs(dyg), pu + flushed * np.abs(dyu)
    r = np.asarray(rs)[:, None]
    xd = FASTMATH_GEGLU_BWD_DZS if extra_dzs is None else extra_dzs
    out = {}
    for name, dy, pe in (("dzs_g", dyg, pg), ("dzs_u", dyu, pu)):
        ref = r * dy
        pre = r * pe + U32 * np.abs(ref) + xd
        bar = pre + ef.bf16_half_ulp(ref, pre)
        out[name] = (ref, bar if m is None else np.where(m == 0, 0.0, bar))
    np_ = (F + 63) // 64
    dot = (dyg * g + dyu * u).sum(1)
    tabs = (np.abs(dyg * g) + np.abs(dyu * u)).sum(1)
    dbar = (pg * np.abs(g) + pu * np.abs(u)).sum(1) + (12 + np_ + 3) * U32 * tabs
    # the slots alone (out1 [np, M]): each slot's own 64 features against its own 12-rounding chain - a bug in one feature block
    # stands against that block's bar, not the whole row's
    xr = FASTMATH_GEGLU_BWD_RCOEF if extra_rcoef is None else extra_rcoef
    per = lambda a: a.reshape(a.shape[0], np_, 64).sum(2).T  # noqa: E731
    out["slots"] = (per(dyg * g + dyu * u), per(pg * np.abs(g) + pu * np.abs(u)) + 12 * U32 * per(np.abs(dyg * g) + np.abs(dyu * u)) + xr)
    scale = np.asarray(rs) ** 2 / K
    out["rcoef"] = (scale * dot, scale * dbar + (FASTMATH_GEGLU_BWD_RCOEF if extra_rcoef is None else extra_rcoef))
    return out


def standin_geglu_bwd(acc, g, u, rs, K: int, m=None, mutant: Optional[str] = None):
    """-> (dzs_g, dzs_u [M, F] bf16 values, rcoef [M]) in float32 steps.  Mutants: "gelu_grad_without_sg", "mask_one_column_over",
    "rs_neighbour_row", "rowdot_beyond_n_valid" (the `dot = 0` of a block at or beyond n_valid dropped, the slot guard kept)."""
    F = g.shape[1]
    df = acc[:, :F]
    if m is not None:
        df = _f32(df * (np.roll(m, 1, axis=1) if mutant == "mask_one_column_over" else m))
    r = _f32(np.roll(rs, -1) if mutant == "rs_neighbour_row" else rs)[:, None]
    k1 = float(np.float32(-2.0 * 0.7978845608028654 * 1.4426950408889634))
    k2, d2 = float(np.float32(k1 * 0.044715)), float(np.float32(2.0 * 0.7978845608028654))
    d2c3 = float(np.float32(d2 * 3.0 * 0.044715))
    g2 = _f32(g * g)
    with np.errstate(over="ignore"):
        sg = _f32(1.0 / _f32(_f32(np.exp2(_f32(g * _f32(k2 * g2 + k1)))) + 1.0))
    d2z, gs, t = _f32(d2c3 * g2 + d2), _f32(g * sg), _f32(sg - sg * sg)
    dgelu = _f32(_f32(g * t) * d2z + (0.0 if mutant == "gelu_grad_without_sg" else sg))
    dyg, dyu = _f32(_f32(df * u) * dgelu), _f32(df * gs)
    np_ = (F + 63) // 64
    slots = np.zeros((np_, acc.shape[0]))
    for s in range(np_):
        c = slice(64 * s, 64 * s + 64)
        slots[s] = _f32(_f32(dyg[:, c] * g[:, c] + dyu[:, c] * u[:, c]).sum(1))
    # ("rowdot_beyond_n_valid": the blocks at or beyond n_valid have slot >= np_ and are never stored - nothing to add)
    dot = np.zeros(acc.shape[0])
    for s in range(np_):
        dot = _f32(dot + slots[s])
    rcoef = _f32(_f32(_f32(r[:, 0] * r[:, 0]) * dot) * np.float32(1.0 / K))
    return bf16_round(_f32(dyg * r)), bf16_round(_f32(dyu * r)), rcoef


# ---------------------------------------------------------------------------------------------------------------------------
# training attention: attention_kernel<true, DROP>, attn_bwd_kernel<0 | 1, DROP>, bias_grad_kernel (rp_dbg_attention_train)
# ---------------------------------------------------------------------------------------------------------------------------
# Forward: s = q . k + tab[h, clamp(j - i, -maxd, maxd) + maxd], P = softmax(s), att = bf16((m P) V) (the row sum uses the undropped
# P), lse2 = m_run log2 e + log2(l) (fp32, log2 domain).  Backward, read in attn_bwd_kernel: delta_i = sum_d dO_i O_i with O the bf16
# att the kernel reads - a 32-step fma chain per half-wave and one add of exact bf16 products; P is RECOMPUTED as exp2((s + b) log2 e
# - lse2) in fp32 from a four-step MFMA score; dP = dO V^T (four MFMA steps), times m under dropout; dS = P (dP - delta).  Both
# operands of the second MFMAs are rounded to bf16 in front of them (`pack_bf2` of s[mb] = m P and of dp[mb] = dS), so
#     dQ = dS K,  dK = dS^T Q:   |err| <= 2^-8 sum |dS| |K or Q|  +  sum |d dS| |K or Q|  +  chain  +  half a bf16 ulp of the result
#     dV = (m P)^T dO:           |err| <= 2^-8 sum m P |dO|       +  sum m P relp |dO|    +  chain  +  half a bf16 ulp
# with relp the relative error of the recomputed P (the score's chain, lse2's own fp32 bar, the fma, one ulp of v_exp_f32) and
# d dS = relp |dS| + P (e_dP + e_delta) + 2^-24 (3 |dS| + P (|dP| + |delta|)), chains of 4 steps per 64-row tile (+ 16).
# The table gradient adds the UNROUNDED dS of a diagonal: dtab[h][t] = sum over the pairs with clamp(j - i) = t, so per entry
#     |err| <= sum |d dS| + (pairs on the diagonal + 16) 2^-24 sum |dS|     - it grows with the number of pairs.
# Its order is NOT fixed: the lanes of a wave add their diagonals into the wave's LDS table with ds_add_f32, two half-waves (and, at
# the clamps, many lanes) to the same word in one instruction, in an order the hardware chooses; so dtab is held to the bound, not
# to bits, run to run and between a sequence alone and packed.  dq / dk / dv / att / lse of a sequence do not depend on its
# neighbours (each workgroup sees one sequence; every chain is in key- or query-tile order): bits, without dropout (the mask's
# row is the packed index).
ATT_TRAIN_CASES = {  # name -> (H, max_distance, std of the logits, lengths)
    "h1-d8-std4-mixed": (1, 8, 4.0, ef.MIXED_LENS),
    "h2-d32-std12-mixed": (2, 32, 12.0, ef.MIXED_LENS),
    "h6-d128-std4-mixed": (6, 128, 4.0, ef.MIXED_LENS),
    "h2-d8-std4-short": (2, 8, 4.0, tuple(int(x) for x in np.random.default_rng(2).integers(1, 6, 300))),
}
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


@functools.lru_cache(maxsize=4)
def attention_train_case(name: str, seed: int = 11) -> Dict:
    """ef.make_attention_case's qkv and table (a value of its own per distance; sequences longer than 2 maxd hit both clamps)
    + dO [T, H 64] bf16 values."""
    H, maxd, std, lens = ATT_TRAIN_CASES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    c = ef.make_attention_case(rng, H, maxd, std, lens, name)
    c["datt"] = bf16_round(rng.standard_normal((c["T"], H * 64)))
    return c


def _heads(a, H):
    return a.reshape(a.shape[0], H, 64).transpose(1, 0, 2)  # [H, rows, 64]


def _unheads(a):
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


def attention_train_compute(c: Dict, mask=None, att_used=None, mutant: Optional[str] = None, f32: bool = False, bars: bool = False):
    """Forward + backward of every sequence.  mask(b, s0, L) -> multipliers [H, L, L] or None.  att_used [T, H 64]: the O delta
    is formed from (None: this function's own att).  f32=True: the kernel's schedule in float32 with its two bf16 roundings (the
    stand-in).  bars=True: also the per-element bars (float64 path only).  Mutants: "bias_sign" (i - j), "clamp_one_early",
    "delta_neighbour_head", "ds_without_delta", "mask_on_p_only".  -> dict of att, lse2 [H, T], delta [H, T], dq, dk, dv [T, H 64],
    dtab [H, 2 maxd + 1] (+ bar_* when asked)."""
    H, maxd, qkv, tab, cu, dO = c["H"], c["maxd"], c["qkv"], c["tab"], c["cu"], c["datt"]
    inner, T, ntab = H * 64, qkv.shape[0], 2 * maxd + 1
    R = (lambda a: _f32(a)) if f32 else (lambda a: a)
    B = (lambda a: bf16_round(a)) if f32 else (lambda a: a)
    out = {k: np.zeros((T, inner)) for k in ("att", "dq", "dk", "dv")}
    out.update(lse2=np.zeros((H, T)), delta=np.zeros((H, T)), dtab=np.zeros((H, ntab)))
    if bars:
        out.update({f"bar_{k}": np.zeros((T, inner)) for k in ("att", "dq", "dk", "dv")})
        out.update(bar_lse2=np.zeros((H, T)), bar_delta=np.zeros((H, T)), bar_dtab=np.zeros((H, ntab)))
    for b in range(len(cu) - 1):
        s0, s1 = int(cu[b]), int(cu[b + 1])
        L = s1 - s0
        nt = (L + 63) // 64
        q, k, v = (_heads(qkv[s0:s1, o * inner:(o + 1) * inner], H) for o in range(3))
        do = _heads(dO[s0:s1], H)
        i, j = np.arange(L)[:, None], np.arange(L)[None, :]
        md = maxd - 1 if mutant == "clamp_one_early" else maxd
        idx = np.clip((i - j) if mutant == "bias_sign" else (j - i), -md, md) + maxd
        true_idx = np.clip(j - i, -maxd, maxd) + maxd
        s = R(R(q @ k.transpose(0, 2, 1)) + tab[:, idx])
        mx = s.max(2, keepdims=True)
        e = np.exp(s - mx)
        l = e.sum(2, keepdims=True)
        lse2 = R(mx * LOG2E + np.log2(l))
        P = R(np.exp2(R(s * LOG2E - lse2))) if f32 else e / l
        m = None if mask is None else mask(b, s0, L)
        Pm = P if m is None else R(P * m)
        att = B(R(Pm @ v)) if f32 else Pm @ v
        o_used = att if att_used is None else _heads(att_used[s0:s1], H)
        delta = R((do * o_used).sum(2, keepdims=True))
        if mutant == "delta_neighbour_head":
            delta = np.roll(delta, 1, axis=0)
        dP = R(do @ v.transpose(0, 2, 1))
        if m is not None and mutant != "mask_on_p_only":
            dP = R(dP * m)
        dS = R(P * (dP if mutant == "ds_without_delta" else R(dP - delta)))
        dSb, Pb = B(dS), B(Pm)
        out["att"][s0:s1], out["lse2"][:, s0:s1], out["delta"][:, s0:s1] = _unheads(att), lse2[:, :, 0], delta[:, :, 0]
        out["dq"][s0:s1], out["dk"][s0:s1] = _unheads(B(R(dSb @ k))), _unheads(B(R(dSb.transpose(0, 2, 1) @ q)))
        out["dv"][s0:s1] = _unheads(B(R(Pb.transpose(0, 2, 1) @ do)))
        flat = true_idx.reshape(-1)
        for h in range(H):
            out["dtab"][h] += np.bincount(flat, weights=dS[h].reshape(-1), minlength=ntab)
        if not bars:
            continue
        aq, ak, av, ado = np.abs(q), np.abs(k), np.abs(v), np.abs(do)
        es = (4 + 16) * U32 * (aq @ ak.transpose(0, 2, 1)) + U32 * np.abs(s)              # the score, natural units
        e_lse2 = LOG2E * (es.max(2, keepdims=True) + (34 * nt + 8) * U32) + 3 * U32 * np.abs(lse2) + 2 * U32 * (np.abs(np.log2(l)) + 1)
        relp = es + LN2 * (e_lse2 + 2 * U32 * (np.abs(s) * LOG2E + np.abs(lse2))) + 2 * U32
        e_delta = 34 * U32 * (ado * np.abs(o_used)).sum(2, keepdims=True)
        mm = 1.0 if m is None else m
        e_dp = mm * (4 + 16) * U32 * (ado @ av.transpose(0, 2, 1)) + (0.0 if m is None else U32 * np.abs(dP))
        aS = np.abs(dS)
        d_ds = relp * aS + P * (e_dp + e_delta) + U32 * (3 * aS + P * (np.abs(dP) + np.abs(delta)))
        chain = (4 * nt + 16) * U32
        half = lambda ref, pre: pre + ef.bf16_half_ulp(ref, pre)  # noqa: E731
        rq, rk, rv = dS @ k, dS.transpose(0, 2, 1) @ q, Pm.transpose(0, 2, 1) @ do
        out["bar_dq"][s0:s1] = _unheads(half(rq, (2.0 ** -8 + chain) * (aS @ ak) + d_ds @ ak))
        out["bar_dk"][s0:s1] = _unheads(half(rk, (2.0 ** -8 + chain) * (aS.transpose(0, 2, 1) @ aq) + d_ds.transpose(0, 2, 1) @ aq))
        aP = np.abs(Pm)
        out["bar_dv"][s0:s1] = _unheads(half(rv, (2.0 ** -8 + chain + 2 * U32) * (aP.transpose(0, 2, 1) @ ado)
                                             + (aP * relp).transpose(0, 2, 1) @ ado))
        # the forward: p (times m) rounded to bf16 in front of P V, the row sum's 32 adds per tile, o / l
        out["bar_att"][s0:s1] = _unheads(half(Pm @ v, (2.0 ** -8 + chain + (34 * nt + 4) * U32) * (aP @ av) + (aP * relp) @ av))
        out["bar_lse2"][:, s0:s1], out["bar_delta"][:, s0:s1] = e_lse2[:, :, 0], e_delta[:, :, 0]
        cnt = np.bincount(flat, minlength=ntab)
        for h in range(H):
            out["bar_dtab"][h] += (np.bincount(flat, weights=d_ds[h].reshape(-1), minlength=ntab)
                                   + (cnt + 16) * U32 * np.bincount(flat, weights=aS[h].reshape(-1), minlength=ntab))
    return out


def sub_attention_train_case(c: Dict, b: int) -> Dict:
    """Sequence b of a case alone."""
    s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
    return dict(ef.sub_attention_case(c, b), datt=c["datt"][s0:s1])


def cpu_attention_mask(c: Dict, p: float, seed: int = 3):
    """A stand-in for the engine's probability mask on the build machine: mask(b, s0, L) -> [H, L, L] of 0 / drop_scale(p)."""
    def mask(b, s0, L):
        return (np.random.default_rng([seed, b, L]).random((c["H"], L, L)) >= p) * drop_scale(p)
    return mask
