"""The sampler's reference for the tests: a float64 restatement of ``rp_sample_step``'s five steps (temperature, top-k,
top-p, the draw, the uniform from ``rp_sample_uniform``), vectorised over rows, with each row's decision margins; and a
CPU ``sample_step`` for ``sample_search_batch`` built on it.  It never launches anything.
"""
from __future__ import annotations

import numpy as np
import torch

GRID = [(T, k, p) for T in (0.7, 1.0, 1.5) for k in (0, 1, 5, "vocab") for p in (1.0, 0.9, 0.1)]


def margin_bound(vocab: int) -> float:
    """A row is compared only when every margin exceeds this: the worst-case fp32 prefix-sum error of ``vocab`` terms
    summing to 1 (vocab * 2^-24), doubled for the exp."""
    return vocab * 2.0 ** -23


def uniforms(lib, seeds, samples, position: int) -> np.ndarray:
    """``rp_sample_uniform(seed, sample, position)`` per row (float32)."""
    return np.array([lib.rp_sample_uniform(int(s) & 0xFFFFFFFF, int(b), int(position)) for s, b in zip(seeds, samples)],
                    dtype=np.float32)


def reference_sample(lp, u, temperature: float, top_k: int, top_p: float):
    """lp [R, V] float32 log-probs, u [R] float32 -> (tokens int64 [R], kept bool [R, V] by id, margins float64 [R], the
    two filters' part of the margins [R]).

    The parameters enter as the float32 values the kernel receives; everything after that is float64.  ``margins`` is
    the smallest of: |u - C(v) / Z| over the CDF's inner boundaries; |cumulative probability - (1 - top_p)| over the
    ascending cumulative sums that decide something; |s[v] - threshold| over the scores not exactly tied with the
    top-k threshold."""
    lp = np.asarray(lp, dtype=np.float32)
    R, V = lp.shape
    inf = np.inf
    s = lp.astype(np.float64) / np.float64(np.float32(temperature))
    order = np.argsort(-s, axis=1, kind="stable")  # descending, equal scores by ascending id
    ss = np.take_along_axis(s, order, 1)
    keep = np.ones((R, V), dtype=bool)
    m_topk = np.full(R, inf)
    if 0 < top_k < V:
        thr = ss[:, top_k - 1 : top_k]
        keep = ss >= thr
        with np.errstate(invalid="ignore"):
            d = np.abs(ss - thr)
        d[(ss == thr) | np.isnan(d)] = inf
        m_topk = d.min(1)
    with np.errstate(invalid="ignore"):
        e = np.where(keep, np.exp(ss - ss[:, :1]), 0.0)
    m_topp = np.full(R, inf)
    if top_p < 1.0:
        drop = np.float64(np.float32(1.0 - np.float64(np.float32(top_p))))
        # read from the far end, the descending order is HF's ascending one with equal probabilities by descending id
        tail = np.cumsum(e[:, ::-1], axis=1)[:, ::-1] / e.sum(1, keepdims=True)
        dropped = tail <= drop
        dropped[:, 0] = False
        d = np.abs(tail - drop)
        d[e == 0.0] = inf
        d[:, 0] = inf  # the most probable token stays whatever its cumulative sum
        m_topp = d.min(1)
        keep &= ~dropped
        e = np.where(keep, e, 0.0)
    w = np.zeros((R, V))
    np.put_along_axis(w, order, e, 1)
    kept = np.zeros((R, V), dtype=bool)
    np.put_along_axis(kept, order, keep, 1)
    C = np.cumsum(w, axis=1)
    Z = C[:, -1:]
    u64 = np.asarray(u, dtype=np.float64)[:, None]
    mass = w > 0.0
    last = V - 1 - np.argmax(mass[:, ::-1], axis=1)
    hit = mass & (C > u64 * Z)
    tokens = np.where(hit.any(1), hit.argmax(1), last)
    d = np.abs(u64 - C / Z)
    d[~mass] = inf
    d[np.arange(R), last] = inf  # C = Z there: past it the stand-in is the same token
    m_cdf = d.min(1)
    return tokens.astype(np.int64), kept, np.minimum(np.minimum(m_topk, m_topp), m_cdf), np.minimum(m_topk, m_topp)


class CpuSampler:
    """``sample_search_batch``'s ``sample_step`` on the host: the reference sampler and ``rp_sample_step``'s bookkeeping."""

    def __init__(self, lib, temperature=1.0, top_k=0, top_p=1.0, eos=1, pad=0):
        self.lib, self.T, self.k, self.p, self.eos, self.pad = lib, temperature, top_k, top_p, eos, pad
        self.min_margin = np.inf

    def __call__(self, log_probs: torch.Tensor, active, t: int, st) -> None:
        n, nb, _ = st.seq.shape
        lp = log_probs.detach().cpu().numpy().astype(np.float32)
        seeds = [int(st.seeds[i]) for i in active for _ in range(nb)]
        u = uniforms(self.lib, seeds, list(range(nb)) * len(active), t)
        toks, _, margins, _ = reference_sample(lp, u, self.T, self.k, self.p)
        for a, i in enumerate(active):
            for b in range(nb):
                r = a * nb + b
                if int(st.finished[i, b]):
                    st.seq[i, b, t + 1] = self.pad
                    st.tokens[r] = self.pad
                    continue
                self.min_margin = min(self.min_margin, float(margins[r]))
                tok = int(toks[r])
                st.seq[i, b, t + 1] = tok
                st.tokens[r] = tok
                st.cum_logprob[i, b] += float(lp[r, tok])
                st.n_generated[i, b] += 1
                if tok == self.eos:
                    st.finished[i, b] = 1


def hand_rows(rows: int, vocab: int, seed: int) -> np.ndarray:
    """Hand-built float32 log-prob rows [rows, vocab]: seeded log-softmax rows of mixed sharpness, then (cycling over the
    row index) a one-hot row, a row with -inf entries, a row with exact ties around every top-k threshold of the grid,
    and a flat row."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((rows, vocab)) * g.choice([0.5, 2.0, 6.0], size=(rows, 1))
    for r in range(rows):
        kind = r % 8
        if kind == 1:  # one-hot
            x[r] = -np.inf
            x[r, g.integers(vocab)] = 0.0
        elif kind == 3:  # -inf entries
            x[r, g.random(vocab) < 0.3] = -np.inf
            x[r, g.integers(vocab)] = 1.0
        elif kind == 5:  # the six largest values: one alone, a pair, a tie of three across rank 5
            x[r] = np.round(x[r])
            top = g.permutation(vocab)[:6]
            x[r, top] = x[r].max() + np.array([3.0, 2.0, 2.0, 1.0, 1.0, 1.0])[: len(top)]
        elif kind == 7:  # flat
            x[r] = 0.0
    x = x.astype(np.float32)
    mx = x.max(1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.exp(x - mx).sum(1, keepdims=True, dtype=np.float64)).astype(np.float32)
    return (x - lse).astype(np.float32)


KERNEL_T = 5  # the position of the kernel test's step


def kernel_case(lib, V: int, rows: int):
    """The kernel test's inputs for one shape: rows laid out as states of min(rows, 64) samples, the states in the slots in
    descending order.  Returns (lp [rows, V], seeds [n], active, row_state [rows], row_sample [rows], u [rows]).  The
    rows' seed, V + 2, is one at which the reference alone leaves at most 10 % of the rows of every grid point out, for
    every shape of the test (tests/test_sample_cpu.py checks exactly these inputs)."""
    nb = min(rows, 64)
    n = rows // nb
    seeds = 1000 + 7 * np.arange(n)
    active = list(range(n))[::-1]  # slot a carries state n - 1 - a
    row_state = np.repeat(active, nb)
    row_sample = np.tile(np.arange(nb), n)
    u = uniforms(lib, seeds[row_state], row_sample, KERNEL_T)
    return hand_rows(rows, V, seed=V + 2), seeds, active, row_state, row_sample, u
