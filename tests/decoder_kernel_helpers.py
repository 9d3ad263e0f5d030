"""Float64 restatements of the seq2seq training path's kernels, one kernel at a time, for tests/test_decoder_kernels_gpu.py
(the kernels, through rp_dbg_decoder_attention / rp_dbg_decoder_rows / rp_dbg_hidden_head) and tests/test_decoder_kernels_cpu.py
(that the GPU tests' bars separate planted bugs on the GPU tests' own shapes).  numpy only; every reference starts from the
bf16 / fp32 values the kernel is handed.

Attention comes in two forms.  ``rounded=False``: float64 throughout.  ``rounded=True``: float64 with a bf16 rounding at the
kernel's documented points and nowhere else: P before the PV product, ``out``, P and dS before the
second products of the backward, and dq / dk / dv at the store.  The distance of the rounded form from the exact one is what
bf16 operand rounding costs on a tensor; the GPU test allows the kernel GRAD_TOL_FACTOR times that, on relative L2 and on
the worst row (max |error| / max |reference|)."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from gen_helpers import unidirectional_bucket
from seq2seq_grad_helpers import GRAD_TOL_FACTOR

LOG2E = 1.4426950408889634
U32 = 2.0 ** -24

# ---- shapes of the GPU tests (the smallest that reach every edge: 128-row resident block, 32 rows per wave, 64-row streamed
# tiles, 16-row DMA pieces; length 300 passes the 257-entry table's clamp on 43 diagonals) --------------------------------
CAUSAL_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 256, 257, 300)
CROSS_PAIRS = ((1, 1), (1, 300), (33, 63), (0, 70), (64, 64), (65, 129), (127, 128), (128, 127), (129, 65), (130, 257), (257, 1))
# name -> (causal, H, nbias, bucket map, operand scale).  "sharp": q, k ~ 0.6 N(0, 1), scores of std 2.9 (the largest of 300
# probabilities is about 0.2); "big": 1.1 N(0, 1), scores of std 9.7 and magnitude 30.  Bucket maps: None = identity (the raw
# table gradient), (num_buckets, max_distance) = T5's unidirectional buckets (nbias = 2 max_distance + 1).
ATTENTION_CASES = {
    "causal-h6-n257-identity": (True, 6, 257, None, 0.6),
    "causal-h2-n33-buckets": (True, 2, 33, (8, 16), 0.6),
    "causal-h1-n257-buckets-big": (True, 1, 257, (32, 128), 1.1),
    "causal-h1-n33-identity": (True, 1, 33, None, 0.6),
    "cross-h6": (False, 6, 0, None, 0.6),
    "cross-h2": (False, 2, 0, None, 0.6),
    "cross-h1-big": (False, 1, 0, None, 1.1),
}
BF16_TENSORS = ("out", "dq", "dk", "dv")

# Bars that are not GRAD_TOL_FACTOR x the rounded reference's error, by (case, tensor): (relative L2, worst row), each 2 x the
# value measured on the MI355X (profiles/decoder_kernel_margins.json), none above test_attention_backward's 2e-2.
DEC_KERNEL_TOL: Dict[Tuple[str, str], Tuple[float, float]] = {}
DEC_KERNEL_TOL_CAP = 2e-2
LSE2_BAR = 1e-3  # test_attention_backward's

# __expf / tanhf in bwd_dlogits_kernel and bwd_geglu_kernel: what the kernel may miss float64 by beyond one bf16 rounding of
# the result and the fp32 yardstick's own error, absolute, = 2 x the largest excess of |error| over 2^-8 |ref| measured on
# the MI355X (profiles/decoder_kernel_margins.json, "rows").
#   dlogits: no excess at V = 64 / 320 / 384 / 512 (at most 7e-74, on the e^-160 entries of the +-80 row): __expf's error
#            stays inside the rounding term, so nothing is added
#   geglu:   1.21e-5 at F = 3584 (4.6e-6 at 256, 2.6e-6 at 64), on results of magnitude up to 30
FASTMATH_DLOGITS = 0.0
FASTMATH_GEGLU = 2.42e-5


def bf16_round(x) -> np.ndarray:
    """float64 values rounded to the nearest bf16 (ties to even), returned as float64."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).reshape(f.shape).astype(np.float64)


def rel_l2(got, ref) -> float:
    den = float(np.sqrt((np.asarray(ref, np.float64) ** 2).sum()))
    num = float(np.sqrt(((np.asarray(got, np.float64) - ref) ** 2).sum()))
    return num / den if den else num


def worst_row(got, ref) -> float:
    """The largest per-row max |error| over the tensor's max |reference|."""
    den = float(np.abs(ref).max()) if np.size(ref) else 0.0
    num = float(np.abs(np.asarray(got, np.float64) - ref).max()) if np.size(ref) else 0.0
    return num / den if den else num


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def attention_case(name: str, seed: int = 11) -> Dict:
    """The operands of one packed call as float64 arrays holding bf16 values (tab: fp32 values)."""
    causal, H, nbias, buckets, scale = ATTENTION_CASES[name]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    pairs = [(n, n) for n in CAUSAL_LENS] if causal else list(CROSS_PAIRS)
    return make_attention_case(rng, causal, H, pairs, nbias, buckets, scale, name)


def make_attention_case(rng, causal, H, pairs, nbias, buckets, scale, name="") -> Dict:
    inner = H * 64
    T, S = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    draw = lambda n, s: bf16_round(rng.standard_normal((n, inner)) * s)  # noqa: E731
    c = dict(name=name, causal=causal, H=H, pairs=list(pairs), q=draw(T, scale), k=draw(S, scale), v=draw(S, 1.0),
             d_o=draw(T, 1.0), nbias=nbias)
    if causal:
        c["tab"] = rng.standard_normal((H, nbias)).astype(np.float32).astype(np.float64)
        if buckets is None:
            c["bucket_of"], c["nbuckets"] = np.arange(nbias, dtype=np.int32), nbias
        else:
            c["bucket_of"] = unidirectional_bucket(-np.arange(nbias), buckets[0], buckets[1]).astype(np.int32)
            c["nbuckets"] = buckets[0]
    return c


def subcase(c: Dict, order: List[int], heads: Optional[List[int]] = None) -> Dict:
    """The packed call that holds pairs ``order`` of ``c`` (in that order) and, optionally, only ``heads``."""
    qcu = np.concatenate([[0], np.cumsum([p[0] for p in c["pairs"]])])
    kcu = np.concatenate([[0], np.cumsum([p[1] for p in c["pairs"]])])
    qrows = np.concatenate([np.arange(qcu[b], qcu[b + 1]) for b in order]).astype(np.int64)
    krows = np.concatenate([np.arange(kcu[b], kcu[b + 1]) for b in order]).astype(np.int64)
    heads = list(range(c["H"])) if heads is None else heads
    cols = np.concatenate([np.arange(h * 64, h * 64 + 64) for h in heads])
    out = dict(c, pairs=[c["pairs"][b] for b in order], H=len(heads), q=c["q"][qrows][:, cols], k=c["k"][krows][:, cols],
               v=c["v"][krows][:, cols], d_o=c["d_o"][qrows][:, cols], qrows=qrows, krows=krows, cols=cols)
    if c["causal"]:
        out["tab"] = c["tab"][heads]
    return out


ATTENTION_MUTANTS = {
    # name -> the form it applies to
    "last_key_twice": "cross",       # key klen - 1 counted twice when klen % 64 != 0 (mask off by one over the clamped row)
    "causal_strict": "causal",       # the causal mask as j < i (row 0 keeps its only key)
    "no_table_clamp": "causal",      # the table read at the unclamped distance (runs on into the next head's row, then 0)
    "dtab_plus_one": "causal",       # the table gradient lands at distance + 1
    "delta_neighbour": "both",       # delta taken from the neighbouring row
    "drop_block_last_row": "both",   # the last row of a 128-row block dropped from dK and dV
    "swap_dk_dv": "both",
    "prev_head_bias": "causal",      # head h reads head h - 1's bias row
}


def attention_reference(c: Dict, rounded: bool = False, mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """out [T, inner], lse2 / delta [H, T], dq [T, inner], dk / dv [S, inner] and, causal, dtab [nbuckets, H], pair by pair
    and head by head."""
    assert mutant is None or mutant in ATTENTION_MUTANTS, mutant
    r = bf16_round if rounded else (lambda x: x)
    H, causal, nbias = c["H"], c["causal"], c["nbias"]
    T, S = c["q"].shape[0], c["k"].shape[0]
    res = dict(out=np.zeros((T, H * 64)), lse2=np.zeros((H, T)), delta=np.zeros((H, T)), dq=np.zeros((T, H * 64)),
               dk=np.zeros((S, H * 64)), dv=np.zeros((S, H * 64)))
    raw = np.zeros((H, max(nbias, 1)))
    flat_tab = np.concatenate([c["tab"].reshape(-1), np.zeros(8192)]) if causal else None
    qs = ks = 0
    for Tq, Tk in c["pairs"]:
        if Tq == 0:
            ks += Tk
            continue
        for h in range(H):
            cs = slice(h * 64, h * 64 + 64)
            q, d_o = c["q"][qs : qs + Tq, cs], c["d_o"][qs : qs + Tq, cs]
            k, v = c["k"][ks : ks + Tk, cs], c["v"][ks : ks + Tk, cs]
            twice = mutant == "last_key_twice" and Tk % 64 != 0
            if twice:
                k, v = np.concatenate([k, k[-1:]]), np.concatenate([v, v[-1:]])
            s = q @ k.T
            live = np.ones(s.shape, bool)
            if causal:
                dist = np.arange(Tq)[:, None] - np.arange(k.shape[0])[None]
                live = (dist > 0) | ((dist == 0) & (np.arange(Tq)[:, None] == 0)) if mutant == "causal_strict" else dist >= 0
                idx = np.minimum(np.maximum(dist, 0), nbias - 1)
                hb = h - 1 if (mutant == "prev_head_bias" and h > 0) else h
                bias = flat_tab[hb * nbias + np.maximum(dist, 0)] if mutant == "no_table_clamp" else c["tab"][hb][idx]
                s = s + bias
            s = np.where(live, s, -np.inf)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(1, keepdims=True)
            p = e / l
            out = r((r(e) @ v) / l)
            delta = (d_o * out).sum(1)
            if mutant == "delta_neighbour":
                delta = np.roll(delta, 1)
            ds = p * (d_o @ v.T - delta[:, None])
            dq, dk, dv = r(r(ds) @ k), r(r(ds).T @ q), r(r(p).T @ d_o)
            if twice:
                dk, dv = dk[:Tk], dv[:Tk]
            if mutant == "drop_block_last_row":
                dk[127::128] = 0.0
                dv[127::128] = 0.0
            if mutant == "swap_dk_dv":
                dk, dv = dv, dk
            res["out"][qs : qs + Tq, cs] = out
            res["lse2"][h, qs : qs + Tq] = (m[:, 0] + np.log(l[:, 0])) * LOG2E
            res["delta"][h, qs : qs + Tq] = delta
            res["dq"][qs : qs + Tq, cs] = dq
            res["dk"][ks : ks + Tk, cs] = dk
            res["dv"][ks : ks + Tk, cs] = dv
            if causal:
                at = np.minimum(idx + 1, nbias - 1) if mutant == "dtab_plus_one" else idx
                np.add.at(raw[h], at[live], ds[live])
        qs += Tq
        ks += Tk
    if causal:
        dtab = np.zeros((c["nbuckets"], H))
        np.add.at(dtab, c["bucket_of"], raw.T)
        res["dtab"] = dtab
    return res


def delta_bar(d_o: np.ndarray, out: np.ndarray, H: int) -> np.ndarray:
    """[H, T]: 33 x 2^-24 x sum |dO O| per row and head: a 32-term fp32 fma chain and one add over exact bf16 products."""
    T = d_o.shape[0]
    return 33 * U32 * np.abs(d_o * out).reshape(T, H, 64).sum(2).T


def delta_of(d_o: np.ndarray, out: np.ndarray, H: int) -> np.ndarray:
    T = d_o.shape[0]
    return (d_o * out).reshape(T, H, 64).sum(2).T


def attention_bounds(name: str, exact: Dict, rounded: Dict) -> Dict[str, Tuple[float, float]]:
    """tensor -> (relative L2 bound, worst-row bound): GRAD_TOL_FACTOR x the rounded reference's own error, or the named
    DEC_KERNEL_TOL entry.  Computed from the references alone."""
    out = {}
    for t in BF16_TENSORS + (("dtab",) if "dtab" in exact else ()):
        b = (GRAD_TOL_FACTOR * rel_l2(rounded[t], exact[t]), GRAD_TOL_FACTOR * worst_row(rounded[t], exact[t]))
        if (name, t) in DEC_KERNEL_TOL:
            b = DEC_KERNEL_TOL[(name, t)]
            assert max(b) <= DEC_KERNEL_TOL_CAP, (name, t, b)
        out[t] = b
    return out


def real_rows(c: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """(query rows, key rows whose pair has a query): the rows the kernels write."""
    krows, ks = [], 0
    for Tq, Tk in c["pairs"]:
        if Tq:
            krows.append(np.arange(ks, ks + Tk))
        ks += Tk
    return np.arange(c["q"].shape[0]), np.concatenate(krows)


def attention_findings(c: Dict, got: Dict, exact: Dict, bounds: Dict, margins: Optional[Dict] = None) -> List[str]:
    """What of ``got`` (float64 arrays shaped as the reference's; delta against the float64 sum over got's own ``out``)
    misses its bar, one line each; ``margins`` receives every measured value with its bound."""
    bad = []
    _, krows = real_rows(c)
    for t, (b2, bm) in bounds.items():
        rows = krows if t in ("dk", "dv") else slice(None)
        e2, em = rel_l2(got[t][rows], exact[t][rows]), worst_row(got[t][rows], exact[t][rows])
        if margins is not None:
            margins[t] = dict(rel_l2=e2, rel_l2_bound=b2, worst_row=em, worst_row_bound=bm)
        if not np.isfinite(got[t][rows]).all() or not (e2 <= b2 and em <= bm):
            bad.append(f"{t}: rel L2 {e2:.3e} (bound {b2:.3e}), worst row {em:.3e} (bound {bm:.3e})")
    e = float(np.abs(got["lse2"] - exact["lse2"]).max())
    if margins is not None:
        margins["lse2"] = dict(max_abs=e, bound=LSE2_BAR)
    if not e <= LSE2_BAR:
        bad.append(f"lse2: max |error| {e:.3e} (bar {LSE2_BAR})")
    err = np.abs(got["delta"] - delta_of(c["d_o"], got["out"], c["H"]))
    bar = delta_bar(c["d_o"], got["out"], c["H"])
    ratio = float((err / np.maximum(bar, 1e-300)).max())
    if margins is not None:
        margins["delta"] = dict(worst_error_over_bar=ratio)
    if not (err <= bar).all():
        bad.append(f"delta: {int((err > bar).sum())} rows beyond 33 x 2^-24 x sum |dO O| (worst {ratio:.2f} x)")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(x)))


def yardstick_bar(ref: np.ndarray, yard: np.ndarray) -> float:
    """tests/test_step_ends_gpu.py's bar: 2 x the error of a torch fp32 restatement + one fp32 ulp of the largest value."""
    return 2.0 * float(np.abs(np.asarray(yard, np.float64) - ref).max()) + ulp32(float(np.abs(ref).max()))


def bf16_row_findings(what: str, got: np.ndarray, ref: np.ndarray, yard: np.ndarray, extra: float = 0.0,
                      margins: Optional[Dict] = None) -> List[str]:
    """A bf16 output: per element 2^-8 |ref| (one bf16 rounding) + the yardstick's bar + ``extra`` (the fast-math term)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    yb = yardstick_bar(ref, yard)
    bar = 2.0 ** -8 * np.abs(ref) + yb + extra
    excess = float((err - 2.0 ** -8 * np.abs(ref)).max())  # what the rounding term leaves over, absolute
    if margins is not None:
        margins[what] = dict(max_abs_error=float(err.max()), excess_over_rounding=excess, yardstick_bar=yb, extra=extra)
    if not np.isfinite(got).all() or not (err <= bar).all():
        i = int(np.argmax(err - bar))
        return [f"{what}: {int((err > bar).sum())} elements beyond the bar; worst |error| {err.flat[i]:.3e} at {i} "
                f"(ref {ref.flat[i]:.3e}, bar {bar.flat[i]:.3e}; yardstick {yb:.3e}, extra {extra:.3e})"]
    return []


def dlogits_reference(logits: np.ndarray, labels: np.ndarray, n_tok: int, count: float, mutant: Optional[str] = None):
    """(softmax - onehot) / count over the counted rows < n_tok, 0 elsewhere.  logits [rows_pad, V] float64."""
    rows, V = logits.shape
    out = np.zeros((rows, V))
    valid = (labels >= 0) & (labels < V)
    if mutant == "count_all":
        count = float(n_tok)
    if not count > 0:
        return out
    for t in np.flatnonzero(valid[:n_tok]):
        x = logits[t] - logits[t].max()
        p = np.exp(x) / np.exp(x).sum()
        p[(labels[t] + 1) % V if mutant == "onehot_plus_one" else labels[t]] -= 1.0
        out[t] = p / count
    return out


def dlogits_yardstick(logits32, labels, n_tok, count):
    """torch fp32 restatement (any device) -> fp32 tensor."""
    import torch

    rows, V = logits32.shape
    out = torch.zeros_like(logits32)
    lab = torch.as_tensor(labels[:n_tok], device=logits32.device).long()
    valid = (lab >= 0) & (lab < V)
    if count > 0 and bool(valid.any()):
        idx = torch.nonzero(valid)[:, 0]
        p = torch.softmax(logits32[idx], dim=-1)
        p[torch.arange(len(idx), device=p.device), lab[idx]] -= 1.0
        out[idx] = p / np.float32(count)
    return out


def dlogits_inputs(V: int, seed: int = 3):
    """130 real rows in a 256-row grid: labels valid, -100 and >= V; a row of +-80 logits; a row of equal logits."""
    rng = np.random.default_rng(seed + V)
    n_tok, rows = 130, 256
    logits = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    logits[5] = np.where(rng.random(V) < 0.5, 80.0, -80.0).astype(np.float32)
    logits[5, 7] = 80.0
    logits[6] = 1.25
    labels = rng.integers(0, V, size=n_tok).astype(np.int32)
    labels[5], labels[6] = 7, V - 1
    labels[[3, 64, 129]] = -100
    labels[[10, 128]] = [V, V + 1000]
    return logits, labels, n_tok, rows


C0, C1 = 0.7978845608028654, 0.044715


def split_gate_up(gu: np.ndarray, F: int):
    """[rows, 2 F] interleaved in 64-column blocks (32 gate, the same 32 up) -> gate, up [rows, F]."""
    b = gu.reshape(gu.shape[0], F // 32, 2, 32)
    return b[:, :, 0].reshape(-1, F), b[:, :, 1].reshape(-1, F)


def geglu_bwd_reference(gu: np.ndarray, dff: np.ndarray, n_tok: int, mutant: Optional[str] = None) -> np.ndarray:
    """[rows, 2 F] = dg | du of ff = gelu_new(g) u, rows >= n_tok zero.  numpy float64, or torch fp32 tensors (the
    yardstick: the same formula in the same order)."""
    rows, F = dff.shape
    g, u = split_gate_up(gu, F)
    if mutant == "swap_gate_up":
        g, u = u, g
    xp = np if isinstance(gu, np.ndarray) else __import__("torch")
    th = xp.tanh(C0 * (g + C1 * g * g * g))
    dgelu = 0.5 * (1.0 + th) + 0.5 * g * (1.0 - th * th) * C0 * (1.0 + 3.0 * C1 * g * g)
    dg, du = dff * u * dgelu, dff * (0.5 * g * (1.0 + th))
    dg[n_tok:] = 0
    du[n_tok:] = 0
    return np.concatenate([dg, du], 1) if xp is np else xp.cat([dg, du], 1)


def geglu_inputs(F: int, seed: int = 5):
    """130 real rows of 256; gate values from -12 to 12 (test_gemm_geglu_wide_range_of_gate_values' range)."""
    rng = np.random.default_rng(seed + F)
    n_tok, rows = 130, 256
    gate = rng.uniform(-12.0, 12.0, size=(rows, F))
    gate[0, : min(F, 25)] = np.linspace(-12.0, 12.0, min(F, 25))
    up = rng.standard_normal((rows, F)) * 2.0
    gu = np.stack([gate.reshape(rows, F // 32, 32), up.reshape(rows, F // 32, 32)], 2).reshape(rows, 2 * F).astype(np.float32)
    dff = rng.standard_normal((rows, F)).astype(np.float32)
    return gu, dff, n_tok, rows


def rmsnorm_bwd_reference(x, w, dh, eps, scale, dx0=None):
    """-> (dx, the rows' terms of d w, d w) of h = scale w x rs."""
    D = x.shape[1]
    rs = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + eps)
    dot = (dh * w * x).sum(1, keepdims=True) / D
    dx = scale * (w * rs * dh - x * rs ** 3 * dot)
    terms = scale * dh * x * rs
    return (dx if dx0 is None else dx0 + dx), terms, terms.sum(0)


def embed_bwd_reference(ids, dx, V, base=None, mutant: Optional[str] = None):
    """d table [V, D]: the rows of dx summed per clamped id, added to ``base`` if given."""
    out = np.zeros((V, dx.shape[1])) if base is None else base.astype(np.float64).copy()
    idc = np.clip(ids, 0, V - 1)
    keep = (ids >= 0) & (ids < V) if mutant == "no_id_clamp" else np.ones(len(ids), bool)
    np.add.at(out, idc[keep], dx[keep])
    return out


def embed_inputs(T: int, V: int, D: int, seed: int = 7):
    """ids that repeat, that never occur (33, 34 and V - 2 are kept free) and that lie outside [0, V)."""
    rng = np.random.default_rng(seed + T + D)
    ids = rng.integers(0, 24, size=T).astype(np.int32) * 16  # multiples of 16: heavy repeats
    ids[rng.random(T) < 0.3] = V - 1
    if T > 2:
        ids[T // 2], ids[T - 1] = -5, V + 7  # clamp to rows 0 and V - 1
    else:
        ids[0] = V + 7
    dx = rng.standard_normal((T, D)).astype(np.float32)
    return ids, dx


def hidden_head_reference(xhi, xlo, rs, w, d_hidden):
    """-> (out, dx, d w): out = w (x rs), dx = w rs dh - x rs^3 (dh w . x) / D, d w = sum_t dh x rs; x = hi + lo."""
    x = xhi.astype(np.float64) + xlo.astype(np.float64)
    D = x.shape[1]
    r = rs.astype(np.float64)[:, None]
    out = w * (x * r)
    dot = (d_hidden * w * x).sum(1, keepdims=True) / D
    return out, w * r * d_hidden - x * r ** 3 * dot, (d_hidden * x * r).sum(0)
