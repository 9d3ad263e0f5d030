"""Float64 restatements of the encoder's pooling head, training row kernels and weight pack / unpack kernels, one kernel at a
time, for tests/test_encoder_train_kernels_gpu.py (the kernels, through rp_dbg_pool_head / rp_dbg_train_rows / rp_dbg_repack /
rp_dbg_unfold / rp_dbg_bias_table) and tests/test_encoder_train_kernels_cpu.py (the references against torch float64 autograd,
and that the GPU tests' bars separate planted bugs on the GPU tests' own shapes).  numpy only; every reference starts from the
values the kernel is handed: the decoded planes, rs as fp32, the dropout mask read back from the device.

Pooling head (rp_train_kernels.h, the comment above pool_bwd_seq_kernel):
  forward   s = sum_t mask x_t rs_t,  m = w s / len,  e = m / max(|m|, 1e-12)
  backward  dm = (de - e (e . de)) / |m|  (|m| <= 1e-12: dm = de / 1e-12),  ds = dm w / len,  dwf = dm s / len,
            dx_t = rs_t (mask ds) - x_t rs_t^3 ((mask ds) . x_t) / D

Bars of fp32 outputs: tests/test_step_ends_gpu.py's (2 x a torch fp32 restatement's error + one fp32 ulp of the largest value,
decoder_kernel_helpers.yardstick_bar); where a kernel's fixed summation order is a longer chain than torch's tree, the derived
first-order bound (longest sequential chain + tree depth) x 2^-24 x sum |terms| per element (chain_bound)."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from decoder_kernel_helpers import U32, embed_bwd_reference, embed_inputs, ulp32, yardstick_bar  # noqa: F401  (re-exported)

# one packed call per D, in this order: the offsets are not chunk-aligned; the edges are 4 waves, two rows in flight x 4 waves
# = 8, four rows in flight x 4 waves = 16, chunks of 32 / 64 / 128
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
# 128: 16 pieces, most lanes clamped; 1472: the third piece partly clamped; 1536: NV = 3 full; 1600: NV = 4 partly; 2048: the limit
DS = (128, 1472, 1536, 1600, 2048)
EPS_NORM = 1e-12
SITE_EMBED, SITE_FINAL, SITE_LAYER0 = 0, 1, 16


def cu_of(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def n_slots(T: int, batch: int, chunk: int) -> int:
    return T // chunk + batch


def chunks_of(cu, chunk: int):
    """(slot, b, c, first row, end row) of every chunk: slot = cu[b] / chunk + b + c (worklist_kernel)."""
    out = []
    for b in range(len(cu) - 1):
        s0, ln = int(cu[b]), int(cu[b + 1] - cu[b])
        for c in range((ln + chunk - 1) // chunk):
            out.append((s0 // chunk + b + c, b, c, s0 + c * chunk, s0 + min(ln, (c + 1) * chunk)))
    return out


def pwork_reference(cu, T: int, chunk: int) -> np.ndarray:
    """int32 [n_slots, 4]: {first token, length, chunk, sequence}; a gap entry is all zero (length 0)."""
    batch = len(cu) - 1
    out = np.zeros((n_slots(T, batch, chunk), 4), np.int32)
    for slot, b, c, _, _ in chunks_of(cu, chunk):
        out[slot] = (cu[b], cu[b + 1] - cu[b], c, b)
    return out


def pool_terms(x, rs, mask=None):
    t = x * np.asarray(rs, np.float64)[:, None]
    return t if mask is None else t * mask


def partial_reference(x, rs, cu, chunk: int, mask=None):
    """-> (slots, sums [n, D], sums of |terms| [n, D]) over the chunks in slot order."""
    t = pool_terms(x, rs, mask)
    ch = chunks_of(cu, chunk)
    return (np.array([c[0] for c in ch]), np.stack([t[a:b].sum(0) for _, _, _, a, b in ch]),
            np.stack([np.abs(t[a:b]).sum(0) for _, _, _, a, b in ch]))


def finish_reference(s, length: int, w):
    """-> (e, m, |m|) of one sequence's column sums."""
    m = w * s / length
    nrm = float(np.sqrt((m * m).sum()))
    return m / max(nrm, EPS_NORM), m, nrm


def head_reference(x, rs, cu, w, mask=None):
    """-> (e [batch, D], s [batch, D]) from the planes."""
    t = pool_terms(x, rs, mask)
    s = np.stack([t[cu[b] : cu[b + 1]].sum(0) for b in range(len(cu) - 1)])
    e = np.stack([finish_reference(s[b], int(cu[b + 1] - cu[b]), w)[0] for b in range(len(cu) - 1)])
    return e, s


def bwd_seq_reference(s, length: int, w, de, mutant: Optional[str] = None, chunk: int = 128):
    """-> (ds, dwf) of one sequence.  Mutants: "no_projection", "len_from_chunk" (ds scaled by the chunk's 1 / len)."""
    e, m, nrm = finish_reference(s, length, w)
    if nrm > EPS_NORM:
        dm = (de - (0.0 if mutant == "no_projection" else e * (e * de).sum())) / nrm
    else:
        dm = de / EPS_NORM
    ln_ds = min(length, chunk) if mutant == "len_from_chunk" else length
    return dm * w / ln_ds, dm * s / length


def bwd_tok_reference(x, rs, ds_rows, mask=None, mutant: Optional[str] = None):
    """dx [n, D] of token rows x with their sequences' ds (one row per token).  Mutant: "rs_squared"."""
    D = x.shape[1]
    r = np.asarray(rs, np.float64)[:, None]
    dsm = ds_rows if mask is None else ds_rows * mask
    dot = (dsm * x).sum(1, keepdims=True) / D
    return r * dsm - x * (r ** 2 if mutant == "rs_squared" else r ** 3) * dot


def seq_rows(cu) -> np.ndarray:
    """The sequence of every token row."""
    return np.repeat(np.arange(len(cu) - 1), np.diff(cu))


def chain_bound(abs_terms, chain: int):
    return chain * U32 * abs_terms


# ---------------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------------
def fp32_findings(what: str, got, ref, yard, bound=None, margins: Optional[Dict] = None) -> List[str]:
    """An fp32 output: max |error| within the yardstick's bar; failing that (a fixed summation order longer than torch's tree)
    every element within the derived ``bound``.  ``margins`` records both figures and which bar was needed."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    yb = yardstick_bar(ref, yard)
    e = float(err.max()) if err.size else 0.0
    rec = dict(max_abs_error=e, yardstick_bar=yb, bar="yardstick")
    ok = bool(np.isfinite(got).all()) and e <= yb
    if not ok and bound is not None and np.isfinite(got).all():
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        rec.update(bar="chain", worst_error_over_chain_bound=ratio)
        ok = bool((err <= bound).all())
    if margins is not None:
        margins[what] = rec
    return [] if ok else [f"{what}: max |error| {e:.3e}, yardstick bar {yb:.3e}" + (
        f", worst error / chain bound {rec.get('worst_error_over_chain_bound', float('nan')):.2f}" if bound is not None else "")]


def planes_findings(what: str, hi, lo, ref, fp32_bar: float, margins: Optional[Dict] = None) -> List[str]:
    """Two-plane outputs: per element |hi + lo - ref| <= 2^-16 |ref| + the fp32 bar (one rounding of the lo plane) and
    |hi - ref| <= 2^-8 |ref| + the same; the coarser per-tensor bars of test_rmsnorm_backward_residual_epilogue recorded."""
    hi, lo, ref = np.asarray(hi, np.float64), np.asarray(lo, np.float64), np.asarray(ref, np.float64)
    es, eh = np.abs(hi + lo - ref), np.abs(hi - ref)
    bs, bh = 2.0 ** -16 * np.abs(ref) + fp32_bar, 2.0 ** -8 * np.abs(ref) + fp32_bar
    ref_max = float(np.abs(ref).max())
    rec = dict(sum_worst_error_over_bar=float((es / bs).max()), hi_worst_error_over_bar=float((eh / bh).max()), fp32_bar=fp32_bar,
               ref_max=ref_max, sum_err=float(es.max()), sum_bar_coarse=2.0 ** -15 * ref_max + 1e-4, hi_err=float(eh.max()),
               hi_bar_coarse=2.0 ** -8 * ref_max)
    if margins is not None:
        margins[what] = rec
    bad = []
    if not (np.isfinite(hi).all() and np.isfinite(lo).all()):
        bad.append(f"{what}: not finite")
    if not (es <= bs).all():
        bad.append(f"{what}: hi + lo misses 2^-16 |ref| + {fp32_bar:.2e} on {int((es > bs).sum())} elements, worst {rec['sum_worst_error_over_bar']:.2f} x")
    if not (eh <= bh).all():
        bad.append(f"{what}: hi misses 2^-8 |ref| + {fp32_bar:.2e} on {int((eh > bh).sum())} elements, worst {rec['hi_worst_error_over_bar']:.2f} x")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def pool_inputs(D: int, lens=LENGTHS, seed: int = 0):
    """x fp32 [T, D] (rows of differing scale), w fp32 [D], d_emb fp32 [batch, D]."""
    rng = np.random.default_rng(seed + D)
    T = int(sum(lens))
    x = (rng.standard_normal((T, D)) * np.exp(rng.uniform(-1.0, 1.5, (T, 1)))).astype(np.float32)
    w = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    de = rng.standard_normal((len(lens), D)).astype(np.float32)
    return x, w, de


def embed_ids(T: int, V: int, seed: int = 7) -> np.ndarray:
    """ids that repeat, that never occur, -5 and V + 7 (decoder_kernel_helpers.embed_inputs')."""
    return embed_inputs(T, V, 8, seed)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# weight pack / unpack
# ---------------------------------------------------------------------------------------------------------------------------
PACK_CONCAT3, PACK_GEGLU, PACK_COPY = 0, 1, 2
UNFOLD_PLAIN, UNFOLD_QKV, UNFOLD_GEGLU = 0, 1, 2


def pack_row_map(mode: int, rows: int, n: int, mutant: Optional[str] = None):
    """(source index, source row) of every packed row: CONCAT3 / QKV rows [k n, (k + 1) n) from source k; GEGLU 32 rows of
    s0 then the same 32 of s1; COPY / PLAIN the row itself.  Mutant "geglu_block_off": the row map off by one 32-row block."""
    r = np.arange(rows)
    if mode == PACK_CONCAT3:
        return r // n, r % n
    if mode == PACK_GEGLU:
        rr = (r + 32) % rows if mutant == "geglu_block_off" else r
        return (rr >> 5) & 1, (rr >> 6) * 32 + (rr & 31)
    return np.zeros(rows, np.int64), r


def repack_reference(mode: int, sources, rows: int, n: int) -> np.ndarray:
    """The packed matrix's fp32 master values [rows, cols] before the column scale (a permutation of the sources' rows)."""
    which, sr = pack_row_map(mode, rows, n)
    return np.stack([sources[k][i] for k, i in zip(which, sr)])


def unfold_reference(part, mode: int, n: int, masters=None, ln=None, mutant: Optional[str] = None):
    """part [splits, rows, C] float64 -> (g list, d ln or None): g_k[sr] = sum_splits part[r] * ln, d ln[c] = sum_r s[r, c]
    master_k[sr, c].  Mutants: "splits_minus_one", "geglu_block_off"."""
    S, rows, C = part.shape
    s = part[: S - 1 if (mutant == "splits_minus_one" and S > 1) else S].sum(0)
    if mode == UNFOLD_PLAIN:
        return [s], None
    pm = PACK_CONCAT3 if mode == UNFOLD_QKV else PACK_GEGLU
    which, sr = pack_row_map(pm, rows, n, mutant)
    nsrc = 3 if mode == UNFOLD_QKV else 2
    per = n if mode == UNFOLD_QKV else rows // 2
    g = [np.zeros((per, C)) for _ in range(nsrc)]
    dln = np.zeros(C)
    for r in range(rows):
        g[which[r]][sr[r]] = s[r] * ln
        dln += s[r] * masters[which[r]][sr[r]]
    return g, dln


def bias_table_reference(rel_bias, bucket_of):
    """tab [H, ntab] from relative_attention_bias.weight [buckets, H]."""
    return np.ascontiguousarray(rel_bias[np.asarray(bucket_of)].T)


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins: float64 code that rounds to fp32 where the kernels round, with planted bugs (tests/test_encoder_train_kernels_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def standin_partial(x, rs, cu, chunk: int, mask=None, mutant: Optional[str] = None):
    """pool_partial_kernel's order: wave w adds tokens t0 + w, t0 + w + 4, .. one fused multiply-add each, then
    (w0 + w1) + (w2 + w3).  Mutants: "drop_last_odd" (the last token of an odd-length chunk), "clamped_piece" (the clamped
    lanes of the last 16-byte piece accumulated into columns D - 8 ..), "mask_next_row" (the mask of row t + 1)."""
    T, D = x.shape
    r = np.asarray(rs, np.float64)
    if mask is not None and mutant == "mask_next_row":
        mask = np.roll(mask, -1, axis=0)
    nv = D // 8
    clamped = (-nv) % 64 if mutant == "clamped_piece" else 0
    out = []
    for _, _, _, a, b in chunks_of(cu, chunk):
        if mutant == "drop_last_odd" and (b - a) % 2 == 1 and b - a > 1:
            b -= 1
        waves = []
        for wv in range(4):
            acc = np.zeros(D)
            for t in range(a + wv, b, 4):
                xt = x[t] if mask is None else _f32(x[t] * mask[t])
                acc = _f32(xt * r[t] + acc)
            waves.append(acc)
        s = _f32(_f32(waves[0] + waves[1]) + _f32(waves[2] + waves[3]))
        if clamped:
            s[D - 8 :] = s[D - 8 :] * (1 + clamped)
        out.append(s)
    return np.stack(out)


def standin_seq_sums(partial, cu, chunk: int):
    """pool_finish_kernel / pool_bwd_seq_kernel: a sequence's chunk rows added in chunk order."""
    out, i = [], 0
    for b in range(len(cu) - 1):
        n = (int(cu[b + 1] - cu[b]) + chunk - 1) // chunk
        s = np.zeros(partial.shape[1])
        for c in range(n):
            s = _f32(s + partial[i + c])
        out.append(s)
        i += n
    return np.stack(out)


def standin_scatter(ids, dx, V: int, mutant: Optional[str] = None):
    """embed_bwd_kernel: per id, its token rows added in token order in fp32.  Mutant "negative_ignored"."""
    out = np.zeros((V, dx.shape[1]))
    for t, i in enumerate(ids):
        if i < 0 and mutant == "negative_ignored":
            continue
        v = min(max(int(i), 0), V - 1)
        out[v] = _f32(out[v] + dx[t])
    return out
