"""Float64 restatements of the decode step's kernels (rp_decoder.hip: dec_gemm_kernel<KIT, EPI>, dec_attention_kernel<CROSS>,
dec_embed / dec_rmsnorm / dec_log_softmax / dec_store_kv), one kernel at a time, for tests/test_decode_step_kernels_gpu.py
(the kernels, through rp_dbg_dec_gemm / rp_dbg_dec_rows / rp_dbg_dec_attention) and tests/test_decode_step_kernels_cpu.py
(that the GPU tests' bars separate planted bugs on the GPU tests' own shapes).  numpy only (the fp32 yardsticks are torch's);
every reference starts from the bf16 / fp32 values the kernel is handed.

Each restatement takes ``dtype`` and ``mutant``: float64 is the reference; float32 with the output rounded where the kernel
rounds is the CPU test's stand-in for the kernel; a mutant is one planted bug."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import numpy as np

from decoder_kernel_helpers import bf16_round, bf16_row_findings, rel_l2, worst_row, yardstick_bar  # noqa: F401
from gen_helpers import simulated_search, unidirectional_bucket

U32 = 2.0 ** -24
EPI_BF16, EPI_RESID, EPI_F32, EPI_GEGLU = 0, 1, 2, 3
EPI_NAMES = {EPI_BF16: "bf16", EPI_RESID: "resid", EPI_F32: "f32", EPI_GEGLU: "geglu"}

# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
# K -> what of launch_dec_gemm's KIT = ceil(K / 512) it reaches (a lane covers the 16-byte pieces l, l + 64, ...)
GEMM_KS = (8, 504, 512, 520, 1024, 1472, 1536, 2040, 2048, 2560, 3072, 3584, 3968, 4096)
GEMM_MS = (1, 63, 64, 65, 130)
GEMM_NS = (1, 3, 4, 5, 130)
GEMM_MAX_M, GEMM_MAX_N = 130, 130
GEMM_PLACEMENT_ROWS = (0, 63, 64, 129)
GEMM_PLACEMENT_COLS = (0, 3, 129)
GEGLU_GATE_STDS = (1.0, 3.0, 10.0, 15.0)  # std of a0 by weight row (row % 4): the gate rows of the GEGLU operand are scaled so
# that gate values cover the unsaturated range and reach magnitude 30 and more at every K

# tanhf (and the fp32 arithmetic of gelu_new around it) in dec_gemm_kernel<., EPI_GEGLU>: what the kernel may miss float64 by
# beyond 2^-8 |ref| and the propagated fp32 terms of its two accumulators, absolute, = 2 x the largest excess measured on the
# MI355X over the K sweep (profiles/decode_step_kernel_margins.json, "gemm" / "geglu_fastmath_excess"):
#   7.311690373561346e-06 at K = 3584 (3.1e-6 .. 5.7e-6 at the other K from 504 on, 3.7e-7 at K = 8), where 1 + tanh cancels
#   (a0 near -5) and the up value is large: results of magnitude 1e-5 and below
GEGLU_EXCESS_MEASURED = 7.311690373561346e-06
FASTMATH_DEC_GEGLU = 2.0 * GEGLU_EXCESS_MEASURED
# __expf in dec_attention_kernel: the same rule over every attention case ("attention_expf_excess": the largest |error| beyond
# 2^-8 |ref|, less the fp32 bar).  Measured: negative in all twelve cases (-2.0e-6 .. -1.2e-5): nothing is added.
FASTMATH_DEC_ATTENTION = 0.0


def kit_of(K: int) -> int:
    return (K // 8 + 63) // 64


@functools.lru_cache(maxsize=None)
def gemm_operands(K: int, kind: str = "normal"):
    """A [130, K], W [260, K] as float64 arrays holding bf16 values, and out0 [130, 130] (what EPI_RESID adds to).
    ``normal``: N(0, 1) (W's first 130 rows, the gate rows of a GEGLU call at N = 130, scaled in the GEGLU operand: see
    gemm_w).  ``integer``: operands in [-8, 8] that identify their row, their element, their 16-byte piece and their
    512-element group, so that every partial sum is an integer below 2^24 (exact in fp32) and a dropped, doubled or
    misplaced piece changes the result."""
    M, N = GEMM_MAX_M, 2 * GEMM_MAX_N
    if kind == "integer":
        k = np.arange(K)
        pos = k * 3 + (k >> 3) * 7 + (k >> 9) * 11
        A = ((np.arange(M)[:, None] * 5 + pos[None]) % 17 - 8).astype(np.float64)
        pos = k * 10 + (k >> 3) * 2 + (k >> 9) * 5
        W = ((np.arange(N)[:, None] * 6 + pos[None]) % 17 - 8).astype(np.float64)
        out0 = ((np.arange(M)[:, None] * 37 + np.arange(GEMM_MAX_N)[None] * 101) % 2001 - 1000).astype(np.float64)
    else:
        rng = np.random.default_rng(1000 + K)
        A = bf16_round(rng.standard_normal((M, K)))
        W = bf16_round(rng.standard_normal((N, K)))
        out0 = rng.standard_normal((M, GEMM_MAX_N)).astype(np.float32).astype(np.float64) * 3.0
    for x in (A, W, out0):
        x.setflags(write=False)
    return A, W, out0


def gemm_w(W: np.ndarray, N: int, epi: int, K: int, cols: Optional[List[int]] = None) -> np.ndarray:
    """The weight operand of an N-column call cut from the 260-row W: rows [0, N) (``cols``: those rows), and for
    EPI_GEGLU the up rows 130 + the same behind them, gate row r scaled to std(a0) = GEGLU_GATE_STDS[r % 4] (and rounded to
    bf16 again)."""
    rows = np.arange(N) if cols is None else np.asarray(cols)
    if epi != EPI_GEGLU:
        return W[rows]
    std = np.asarray(GEGLU_GATE_STDS)[rows % len(GEGLU_GATE_STDS)]
    return np.concatenate([bf16_round(W[rows] * (std / np.sqrt(K))[:, None]), W[rows + GEMM_MAX_N]])


def gelu_new(u):
    return 0.5 * u * (1.0 + np.tanh(0.7978845608028654 * (u + 0.044715 * u * u * u)))


def gelu_new_grad(u):
    c0, c1 = 0.7978845608028654, 0.044715
    th = np.tanh(c0 * (u + c1 * u ** 3))
    return 0.5 * (1.0 + th) + 0.5 * u * (1.0 - th * th) * c0 * (1.0 + 3.0 * c1 * u * u)


GEMM_MUTANTS = {
    # name -> the epilogues it applies to (None: all)
    "drop_last_partial_group": None,   # the last, partly filled 64-piece group of K is not accumulated
    "w_piece_plus_one": None,          # lane j reads piece j + 1 of W (the last piece: zero)
    "geglu_up_row_n_plus_1": (EPI_GEGLU,),
    "geglu_swap": (EPI_GEGLU,),
    "resid_overwrites": (EPI_RESID,),
}


def _lane_sums(A, W, dtype, mutant=None):
    """[M, N] = sum_k A W^T.  float64: a matmul.  float32: the kernel's order - lane l's fma chain over its pieces l, l + 64,
    ... (8 elements each, in order), then the xor butterfly 32, 16, ..., 1, lane 0's value."""
    K = A.shape[1]
    nk = K // 8
    if mutant == "w_piece_plus_one":
        W = np.concatenate([W[:, 8:], np.zeros((W.shape[0], 8))], 1)
    if mutant == "drop_last_partial_group" and nk % 64:
        keep = (nk // 64) * 64 * 8
        A, W = A[:, :keep], W[:, :keep]
        K, nk = keep, keep // 8
    if dtype == np.float64:
        return A @ W.T
    kit = (nk + 63) // 64
    Ap = np.zeros((A.shape[0], kit * 512), np.float32)
    Wp = np.zeros((W.shape[0], kit * 512), np.float32)
    Ap[:, :K], Wp[:, :K] = A, W
    Ap, Wp = Ap.reshape(-1, kit, 64, 8), Wp.reshape(-1, kit, 64, 8)
    acc = np.zeros((A.shape[0], W.shape[0], 64), np.float32)
    for i in range(kit):
        for e in range(8):
            acc += Ap[:, None, i, :, e] * Wp[None, :, i, :, e]  # bf16 x bf16 is exact in fp32: the fma rounds once
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ o]
    return acc[:, :, 0]


def gemm_standin_sums(A, W) -> np.ndarray:
    """[M, rows of W]: the accumulators as the kernel forms them, in float32 (the CPU test's stand-in for the main loop)."""
    return _lane_sums(A, W, np.float32).astype(np.float64)


def gemm_reference(A, W, N, epi, out0=None, dtype=np.float64, mutant: Optional[str] = None, sums=None) -> np.ndarray:
    """out [M, N] of rp_dbg_dec_gemm(epi) on A [M, K], W [N or 2 N, K] (float64 arrays of bf16 values), out0 [M, N] for
    EPI_RESID; unrounded (``gemm_store`` rounds as the kernel's store does).  ``sums``: the accumulators to start from
    instead of the float64 products (gemm_standin_sums); ``dtype``: the epilogue's arithmetic."""
    assert mutant is None or mutant in GEMM_MUTANTS, mutant
    P = (_lane_sums(A, W, np.float64, mutant) if sums is None else sums).astype(dtype)
    if epi == EPI_GEGLU:
        a0, a1 = P[:, :N], P[:, N:2 * N]
        if mutant == "geglu_up_row_n_plus_1":
            a1 = P[:, 1:N + 1]
        if mutant == "geglu_swap":
            a0, a1 = a1, a0
        out = gelu_new(a0) * a1
    elif epi == EPI_RESID:
        out = P[:, :N] if mutant == "resid_overwrites" else np.asarray(out0, dtype) + P[:, :N]
    else:
        out = P[:, :N]
    return out.astype(np.float64)


def gemm_store(out, epi) -> np.ndarray:
    """The value the kernel's store leaves: bf16 (EPI_BF16, EPI_GEGLU) or fp32."""
    return bf16_round(out) if epi in (EPI_BF16, EPI_GEGLU) else np.asarray(out, np.float32).astype(np.float64)


def gemm_bar(A, W, N, epi, out0=None, extra: float = 0.0):
    """-> (ref, bar) [M, N]: the exact float64 result and the element-wise bar of the module docstring of the GPU test:
    an fp32 chain of at most 8 KIT fmas of exact products and 6 butterfly adds, (8 KIT + 6) 2^-24 sum |a w|; + 2^-24
    |result| for EPI_RESID's add; + 2^-8 |ref| for a bf16 store; EPI_GEGLU: 2^-8 |ref| + the two accumulators' terms
    propagated through gelu_new(a0) a1 (first order + the product of the two) + ``extra`` (FASTMATH_DEC_GEGLU)."""
    c = (8 * kit_of(A.shape[1]) + 6) * U32
    P, S = A @ W.T, np.abs(A) @ np.abs(W).T
    if epi == EPI_GEGLU:
        a0, a1, e0, e1 = P[:, :N], P[:, N:2 * N], c * S[:, :N], c * S[:, N:2 * N]
        ref = gelu_new(a0) * a1
        g = np.maximum(np.abs(gelu_new_grad(a0 - e0)), np.abs(gelu_new_grad(a0 + e0)))
        g = np.maximum(g, np.abs(gelu_new_grad(a0)))
        return ref, 2.0 ** -8 * np.abs(ref) + g * np.abs(a1) * e0 + np.abs(gelu_new(a0)) * e1 + 1.2 * e0 * e1 + extra
    ref, bar = P, c * S
    if epi == EPI_RESID:
        ref = out0 + P
        bar = bar + U32 * np.abs(ref)
    if epi == EPI_BF16:
        bar = bar + 2.0 ** -8 * np.abs(ref)
    return ref, bar


def gemm_exact_expected(A, W, N, epi, out0=None) -> np.ndarray:
    """The integer-operand cases: every partial sum is an integer below 2^24, so the fp32 result IS the float64 one, bit for
    bit (EPI_BF16: its bf16 rounding)."""
    return gemm_store(gemm_reference(A, W, N, epi, out0), epi)


def gemm_max_partial_sum(A, W) -> float:
    """An upper bound on |any partial sum in any order| of every output: max over (m, n) of sum_k |a w|."""
    return float((np.abs(A) @ np.abs(W).T).max())


def gemm_findings(what, got, ref, bar, margins: Optional[Dict] = None) -> List[str]:
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / np.maximum(bar, 1e-300)).max())
    if margins is not None:
        margins[what] = max(margins.get(what, 0.0), ratio)
    if not np.isfinite(got).all() or not (err <= bar).all():
        i = int(np.argmax(err - bar))
        return [f"{what}: {int((~(err <= bar)).sum())} elements beyond the bar; worst |error| {err.flat[i]:.3e} at "
                f"{np.unravel_index(i, err.shape)} (ref {ref.flat[i]:.6e}, bar {bar.flat[i]:.3e})"]
    return []


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
# self-attention: name -> (H, nb, table, positions per slot, states per slot, q / k scale).  table: (num_buckets, max_distance)
# = T5's buckets expanded by distance as the product expands them (nbias = 2 max_distance + 1: 257 or 33; constant from
# max_distance on), or nbias alone = a value of its own per distance (the clamped entry differs from its neighbour, so a
# clamp one entry early shows).  Key counts pos + 1 cover {1, 2, 255, 256, 257, 258, 300, 1025} and the cap 8192; the 33-wide table's
# clamp is crossed from 34 keys on.  "mixed": four slots at {0, 256, 40, 299} carrying states [2, 0, 3, 1].
SELF_CASES = {
    "h3-nb3-n257": (3, 3, 257, (0, 1, 254, 255, 256, 257, 299), (3, 0, 6, 2, 5, 1, 4), 0.6),
    "h6-nb1-n33": (6, 1, 33, (0, 32, 33, 34, 299, 1024), (5, 4, 3, 2, 1, 0), 0.6),
    "h12-nb3-n257": (12, 3, (32, 128), (1, 256, 257), (0, 1, 2), 0.6),
    "h1-nb64-n33": (1, 64, (8, 16), (0, 40, 33), (2, 0, 1), 0.6),
    "h1-nb1-n257-big": (1, 1, (32, 128), (255, 299, 1024), (1, 2, 0), 1.1),
    "h3-nb3-n33-mixed": (3, 3, 33, (0, 256, 40, 299), (2, 0, 3, 1), 0.6),
    "h1-nb1-n257-cap": (1, 1, (32, 128), (8191,), (0,), 0.6),
}
HAND_MADE_ROW = "h3-nb3-n257"  # its last slot's beam 1 holds ancestry entries -1, rows, rows + 1000 and -2^31: they clamp
# cross-attention: name -> (H, nb, src_len per slot, memory order of the slots' sources, scale)
CROSS_CASES = {
    "h3-nb3": (3, 3, (1, 257, 64), (2, 0, 1), 0.6),
    "h6-nb1": (6, 1, (63, 65, 255), (1, 2, 0), 0.6),
    "h12-nb3": (12, 3, (256, 1, 65), (2, 1, 0), 0.6),
    "h1-nb64": (1, 64, (64, 255, 63), (1, 0, 2), 0.6),
    "h1-nb1-big": (1, 1, (2048, 256, 257), (2, 0, 1), 1.1),
}
CROSS_GAP = 2  # NaN rows between two sources


@functools.lru_cache(maxsize=None)
def self_case(name: str) -> Dict:
    """q [R, inner]; cache [n_states, rows, 2 inner] (k | v; rows no ancestry entry names hold NaN); anc [R, astride] int64;
    tab [H, nbias] (fp32 values); state / pos per slot.  float64 arrays of bf16 values."""
    H, nb, table, pos, state, scale = SELF_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    inner, n, max_len = 64 * H, len(pos), max(pos) + 1
    nbias = table if isinstance(table, int) else 2 * table[1] + 1
    rows, astride = max_len * nb, max_len + 3
    n_states = max(state) + 1
    cache = np.full((n_states, rows, 2 * inner), np.nan)
    anc = np.zeros((n * nb, astride), np.int64)
    for a in range(n):
        used = (pos[a] + 1) * nb
        # every state's region is filled distinctly: its own draws
        cache[state[a], :used, :inner] = bf16_round(rng.standard_normal((used, inner)) * scale)
        cache[state[a], :used, inner:] = bf16_round(rng.standard_normal((used, inner)))
        for _, _, last in simulated_search(nb, pos[a] + 1, 500 + 31 * a + len(name)):
            pass
        anc[a * nb:(a + 1) * nb, :pos[a] + 1] = last.numpy()
        anc[a * nb:(a + 1) * nb, pos[a] + 1:] = used if used < rows else 0  # never read: a NaN row where there is one
    if name == HAND_MADE_ROW:
        r = (n - 1) * nb + 1
        anc[r, [5, 7, 9, 11]] = [-1, rows, rows + 1000, -2 ** 31]
    if isinstance(table, int):
        tab = rng.standard_normal((H, nbias)).astype(np.float32).astype(np.float64)
    else:
        raw = rng.standard_normal((H, table[0])).astype(np.float32).astype(np.float64)
        tab = raw[:, unidirectional_bucket(-np.arange(nbias), table[0], table[1])]
    q = bf16_round(rng.standard_normal((n * nb, inner)) * scale)
    return dict(name=name, cross=False, H=H, nb=nb, nbias=nbias, pos=list(pos), state=list(state), n_states=n_states,
                max_len=max_len, rows=rows, astride=astride, q=q, kv=cache, anc=anc, tab=tab, koff=0, voff=inner,
                ldkv=2 * inner, scale=scale)


@functools.lru_cache(maxsize=None)
def cross_case(name: str) -> Dict:
    """q [R, inner]; kv [rows, 4 inner]: a two-layer cross K/V whose layer 1 the call reads (koff = 2 inner, voff = 3 inner;
    layer 0's columns and the rows between two sources hold NaN); src_off / src_len per slot."""
    H, nb, lens, order, scale = CROSS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    inner, n = 64 * H, len(lens)
    off, at = [0] * n, CROSS_GAP
    for a in order:
        off[a] = at
        at += lens[a] + CROSS_GAP
    kv = np.full((at, 4 * inner), np.nan)
    for a in range(n):
        kv[off[a]:off[a] + lens[a], 2 * inner:3 * inner] = bf16_round(rng.standard_normal((lens[a], inner)) * scale)
        kv[off[a]:off[a] + lens[a], 3 * inner:] = bf16_round(rng.standard_normal((lens[a], inner)))
    q = bf16_round(rng.standard_normal((n * nb, inner)) * scale)
    return dict(name=name, cross=True, H=H, nb=nb, src_off=off, src_len=list(lens), state=list(range(n)), pos=[0] * n,
                n_states=n, max_len=1, rows=at, q=q, kv=kv, koff=2 * inner, voff=3 * inner, ldkv=4 * inner, scale=scale)


def one_slot(c: Dict, a: int) -> Dict:
    """The call that holds slot ``a`` of ``c`` alone (the same buffers)."""
    nb = c["nb"]
    out = dict(c, q=c["q"][a * nb:(a + 1) * nb], state=[c["state"][a]], pos=[c["pos"][a]], slot_of=a)
    if c["cross"]:
        out.update(src_off=[c["src_off"][a]], src_len=[c["src_len"][a]])
    else:
        out["anc"] = c["anc"][a * nb:(a + 1) * nb]
    return out


ATTENTION_MUTANTS = {
    # name -> the form it applies to
    "bias_distance_plus_one": "self",
    "clamp_at_nbias_minus_2": "self",
    "ancestry_ignored": "self",        # key p read from row p * nb + beam
    "pos_of_slot_0": "self",           # slot 0's position gives every slot's key count
    "drop_last_key_mod_256": "self",   # the last key dropped when len % 256 == 1 (len > 1)
    "src_off_of_slot_0": "cross",
    "v_at_koff": "both",
}


def attention_reference(c: Dict, dtype=np.float64, rounded: bool = False, mutant: Optional[str] = None) -> np.ndarray:
    """out [R, inner]: per row and head softmax(q k^T + tab[h, min(len - 1 - p, nbias - 1)]) v over keys p = 0 .. pos[slot]
    read through the row's ancestry entries clamped to [0, rows) (cross: no bias, the slot's src_len rows from src_off).
    ``rounded``: out rounded to bf16 (the kernel's store).  dtype float32 + rounded: the CPU test's stand-in."""
    assert mutant is None or mutant in ATTENTION_MUTANTS, mutant
    H, nb, koff, voff = c["H"], c["nb"], c["koff"], c["voff"]
    if mutant == "v_at_koff":
        voff = koff
    R = c["q"].shape[0]
    out = np.zeros((R, 64 * H))
    for row in range(R):
        slot, b = divmod(row, nb)
        if c["cross"]:
            off = c["src_off"][0 if mutant == "src_off_of_slot_0" else slot]
            n = c["src_len"][slot]
            keys = c["kv"][off:off + n]
            bias_idx = None
        else:
            n = c["pos"][0 if mutant == "pos_of_slot_0" else slot] + 1
            r = np.arange(n) * nb + b if mutant == "ancestry_ignored" else c["anc"][row, :n]
            keys = c["kv"][c["state"][slot]][np.clip(r, 0, c["rows"] - 1)]
            dist = n - 1 - np.arange(n) + (1 if mutant == "bias_distance_plus_one" else 0)
            bias_idx = np.minimum(dist, c["nbias"] - (2 if mutant == "clamp_at_nbias_minus_2" else 1))
            if mutant == "drop_last_key_mod_256" and n > 1 and n % 256 == 1:
                keys, bias_idx = keys[:-1], bias_idx[:-1]
        keys = keys.astype(dtype)
        for h in range(H):
            s = keys[:, koff + 64 * h:koff + 64 * h + 64] @ c["q"][row, 64 * h:64 * h + 64].astype(dtype)
            if bias_idx is not None:
                s = s + c["tab"][h][bias_idx].astype(dtype)
            e = np.exp(s - s.max())
            out[row, 64 * h:64 * h + 64] = (e @ keys[:, voff + 64 * h:voff + 64 * h + 64]) / e.sum()
    return bf16_round(out) if rounded else out


def attention_yardstick(c: Dict, device="cpu") -> np.ndarray:
    """The same computation in torch fp32 on the same inputs (test_step_ends_gpu's kind of yardstick), unrounded."""
    import torch

    H, nb, koff, voff = c["H"], c["nb"], c["koff"], c["voff"]
    f = lambda x: torch.from_numpy(np.nan_to_num(np.asarray(x, np.float64)).astype(np.float32)).to(device)  # noqa: E731
    q, kv = f(c["q"]), f(c["kv"])
    tab = None if c["cross"] else f(c["tab"])
    out = torch.zeros((q.shape[0], 64 * H), dtype=torch.float32, device=device)
    for row in range(q.shape[0]):
        slot = row // nb
        if c["cross"]:
            keys = kv[c["src_off"][slot]:c["src_off"][slot] + c["src_len"][slot]]
            n = keys.shape[0]
        else:
            n = c["pos"][slot] + 1
            r = torch.from_numpy(np.clip(c["anc"][row, :n], 0, c["rows"] - 1)).to(device)
            keys = kv[c["state"][slot]][r]
            idx = torch.from_numpy(np.minimum(n - 1 - np.arange(n), c["nbias"] - 1)).to(device)
        k = keys[:, koff:koff + 64 * H].reshape(n, H, 64)
        v = keys[:, voff:voff + 64 * H].reshape(n, H, 64)
        s = torch.einsum("nhd,hd->hn", k, q[row].reshape(H, 64))
        if tab is not None:
            s = s + tab[:, idx]
        out[row] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v).reshape(-1)
    return out.cpu().numpy().astype(np.float64)


def attention_findings(name, got, exact, yard, margins: Optional[Dict] = None) -> List[str]:
    """out against the exact float64 form: one bf16 rounding (2^-8 |ref|) + the fp32 bar (2 x the torch fp32 restatement's
    error + one fp32 ulp of the largest value) + FASTMATH_DEC_ATTENTION; relative L2 and worst row are reported."""
    m = {} if margins is None else margins
    found = bf16_row_findings(name, got, exact, yard, FASTMATH_DEC_ATTENTION, m)
    m[name].update(rel_l2=rel_l2(got, exact), worst_row=worst_row(got, exact))
    return found


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
LOG_SOFTMAX_VS = (1, 3, 255, 256, 257, 384, 512)
LOG_SOFTMAX_ROWS = (1, 130)
RMSNORM_DS = (8, 128, 264, 1472, 1536, 4096)
EMBED_CASES = ((1, 8), (1, 1472), (384, 8), (300, 1472))  # (V, D)
RMS_EPS = 1e-6


def log_softmax_inputs(V: int, rows: int) -> np.ndarray:
    """fp32 logits ~ N(0, 4^2); with 130 rows: row 5 = +-80, row 6 all equal, row 7 = row 5 + 40 (120 / -40: the same
    log-probs; e^120 is beyond fp32)."""
    rng = np.random.default_rng(17 * V + rows)
    x = (rng.standard_normal((rows, V)) * 4.0).astype(np.float32)
    if rows > 7:
        x[5] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0)
        x[6] = 1.25
        x[7] = x[5] + 40.0
    return x


def log_softmax_reference(x, dtype=np.float64, mutant: Optional[str] = None) -> np.ndarray:
    """mutants: ``sum_stops_at_256`` (columns from 256 on left out of the sum), ``no_max`` (the maximum not subtracted)."""
    x = np.asarray(x, dtype)
    mx = np.zeros((x.shape[0], 1), dtype) if mutant == "no_max" else x.max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - mx)
        if mutant == "sum_stops_at_256":
            e = e[:, :256]
        return ((x - mx) - np.log(e.sum(1, keepdims=True, dtype=dtype))).astype(np.float64)


def fp32_findings(what, got, ref, yard, margins: Optional[Dict] = None) -> List[str]:
    """An fp32 output under tests/test_step_ends_gpu.py's bar: 2 x a torch fp32 restatement's error + one fp32 ulp of the
    largest value."""
    got = np.asarray(got, np.float64)
    bar = yardstick_bar(ref, yard)
    err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")
    if margins is not None:
        margins[what] = dict(max_abs_error=err, bar=bar)
    return [] if err <= bar else [f"{what}: max |error| {err:.3e} beyond the bar {bar:.3e}"]


def rmsnorm_inputs(D: int):
    """x fp32 [5, D] ~ 3 N(0, 1) with row 1 all zero and row 2 of magnitude 1e4; w fp32 [D] ~ 1 + 0.2 N(0, 1)."""
    rng = np.random.default_rng(29 * D)
    x = (rng.standard_normal((5, D)) * 3.0).astype(np.float32)
    x[1] = 0.0
    x[2] = rng.choice([-1.0, 1.0], D) * rng.uniform(1e4, 3e4, D)
    return x, (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)


def rmsnorm_reference(x, w, eps, scale, dtype=np.float64, rounded: bool = False, mutant: Optional[str] = None) -> np.ndarray:
    """w (x rsqrt(mean(x^2) + eps)) scale.  mutants: ``mean_over_padded_d`` (D rounded up to 256), ``scale_dropped``."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    D = x.shape[1]
    den = (D + 255) // 256 * 256 if mutant == "mean_over_padded_d" else D
    r = 1.0 / np.sqrt((x * x).sum(1, keepdims=True, dtype=dtype) / dtype(den) + dtype(eps))
    out = (w * (x * r) * dtype(1.0 if mutant == "scale_dropped" else scale)).astype(np.float64)
    return bf16_round(out) if rounded else out


def embed_reference(ids, table) -> np.ndarray:
    """table[clip(ids, 0, V - 1)]"""
    return table[np.clip(ids, 0, table.shape[0] - 1)]


def embed_ids(V: int) -> np.ndarray:
    rng = np.random.default_rng(V)
    return np.concatenate([[-1, V, 0, V - 1, V + 1000, -2 ** 31], rng.integers(0, V, size=64)]).astype(np.int32)


def store_kv_reference(qkv, cache, state, pos, nb, mutant: Optional[str] = None) -> np.ndarray:
    """The caches [n_states, rows, 2 inner] after the store: rows pos[slot] * nb + b of state[slot] <- columns [inner,
    3 inner) of qkv row slot * nb + b; everything else as it was.  mutants: ``pos_of_slot_0``, ``v_not_stored``.  Works on
    any dtype (the GPU test passes the raw 16-bit patterns)."""
    out = cache.copy()
    inner = qkv.shape[1] // 3
    for a in range(len(state)):
        p = pos[0 if mutant == "pos_of_slot_0" else a]
        src = qkv[a * nb:(a + 1) * nb, inner:2 * inner if mutant == "v_not_stored" else 3 * inner]
        out[state[a], p * nb:(p + 1) * nb, :src.shape[1]] = src
    return out


# the whole-step run off the two product geometries (tests/test_decode_step_kernels_gpu.py): KIT 2 (d_model 520: one live
# lane in group 2) and 5 (d_ff 2056), a 33-wide table whose clamp the 60 steps cross, V below 384
STEP_CONFIG = dict(d_model=520, d_ff=2056, num_heads=3, vocab_size=300, num_decoder_layers=2,
                   relative_attention_num_buckets=8, relative_attention_max_distance=16)
STEP_CASE = "step-d520-f2056-h3-v300/nb5"
