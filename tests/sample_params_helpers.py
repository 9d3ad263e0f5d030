"""Sampling parameters per row, for the tests: the reference sampler with a parameter table (``CpuRowSampler``:
tests/sample_pool_helpers.py's bookkeeping, the parameters of every launch row looked up through
``generation.sample_row_params_host``, ``reference_sample`` once per distinct parameter set), the assignment of grid
points to rows that the kernel tests share, and the tickets of the pool / stream scenario.  It never launches anything.
"""
from __future__ import annotations

import numpy as np
import torch

from sample_helpers import GRID, reference_sample, uniforms
from reprover_amd.generation import BeamSearchOutput, SamplingParams, sample_row_params_host

EOS = 1


def grid_point(state: int, sample: int, nb: int, V: int):
    """Row (state, sample)'s ``(temperature, top_k, top_p)``: a walk through the 36 grid points in steps of 5 (coprime
    to 36: neighbouring rows differ in all three values, every point is reached)."""
    T, k, p = GRID[(5 * (state * nb + sample) + 1) % 36]
    return T, (V if k == "vocab" else k), p


def grid_table(n: int, nb: int, V: int) -> torch.Tensor:
    """int32 ``[n, nb, 4]``: every row's block at its grid point."""
    return torch.stack([SamplingParams(*map(list, zip(*(grid_point(s, b, nb, V) for b in range(nb))))).rows(nb)
                        for s in range(n)])


def uniform_table(n: int, nb: int, T, k, p) -> torch.Tensor:
    return SamplingParams(T, k, p).rows(nb)[None].repeat(n, 1, 1).contiguous()


def reference_by_row(lp, u, row_params):
    """``reference_sample`` with a parameter set per row: (tokens int64 [R], margins float64 [R])."""
    lp = np.asarray(lp, dtype=np.float32)
    toks = np.zeros(lp.shape[0], dtype=np.int64)
    margins = np.full(lp.shape[0], np.inf)
    for key in sorted(set(row_params)):
        rows = np.array([r for r, q in enumerate(row_params) if q == key])
        toks[rows], _, margins[rows], _ = reference_sample(lp[rows], np.asarray(u)[rows], *key)
    return toks, margins


class CpuRowSampler:
    """``SamplePool``'s ``sample_step`` on the host with the parameters of ``st.params`` (and, through ``at``,
    ``sample_search``'s).  ``mutant`` is ``sample_row_params_host``'s."""

    def __init__(self, lib, eos=EOS, pad=0, mutant=None):
        self.lib, self.eos, self.pad, self.mutant = lib, eos, pad, mutant
        self.min_margin = np.inf
        self.calls = []

    def __call__(self, log_probs: torch.Tensor, active, pos, st) -> None:
        n, nb, max_len = st.seq.shape
        assert len(active) == len(pos) and all(0 <= p <= max_len - 2 for p in pos), (pos, max_len)
        self.calls.append((list(active), list(pos)))
        lp = log_probs.detach().cpu().numpy().astype(np.float32)
        u = np.concatenate([uniforms(self.lib, [int(st.seeds[i])] * nb, range(nb), p) for i, p in zip(active, pos)])
        toks, margins = reference_by_row(lp, u, sample_row_params_host(st, active, self.mutant))
        for a, (i, p) in enumerate(zip(active, pos)):
            for b in range(nb):
                r = a * nb + b
                if int(st.finished[i, b]):
                    st.seq[i, b, p + 1] = self.pad
                    st.tokens[r] = self.pad
                    continue
                self.min_margin = min(self.min_margin, float(margins[r]))
                tok = int(toks[r])
                st.seq[i, b, p + 1] = tok
                st.tokens[r] = tok
                st.cum_logprob[i, b] += float(lp[r, tok])
                st.n_generated[i, b] += 1
                if tok == self.eos:
                    st.finished[i, b] = 1

    def at(self, log_probs: torch.Tensor, active, t: int, st) -> None:
        self(log_probs, active, [t] * len(active), st)


# ---- the pool / stream scenario: seven tickets, four parameter sets, four live counts -----------------------------------------
STREAM_KW = dict(temperature=1.2, top_k=50, top_p=0.95)  # the pool's own parameters: what a ticket without any gets
LIVE = (4, 1, 3, 2)


def ticket_params(i: int):
    """Ticket ``i``'s ``SamplingParams`` (None: the pool's own) for its ``LIVE[i % 4]`` samples: a ladder over four
    samples, greedy-like ``top_k = 1``, scalars, the pool's own."""
    return (SamplingParams(temperature=[0.7, 1.0, 1.5, 1.2], top_k=[0, 5, 50, 0], top_p=[1.0, 0.9, 0.95, 0.5]),
            SamplingParams(0.8, 1, 1.0), SamplingParams(1.5, 0, 0.9), None)[i % 4]


def ticket_block(i: int, nb: int) -> torch.Tensor:
    """Ticket ``i``'s parameters as a block of ``nb >= LIVE[i % 4]`` rows (the rows past its samples: the defaults)."""
    q = ticket_params(i) or SamplingParams(**STREAM_KW)
    k = LIVE[i % 4]
    return torch.cat([q.rows(k), SamplingParams().rows(nb)[k:]])


def first_rows(out: BeamSearchOutput, k: int, eos: int = EOS) -> BeamSearchOutput:
    """The output of the same search with only its first ``k`` samples: their rows, trimmed to the longest of them."""
    seq = out.sequences[:k]
    n_tok = [(row[1:].tolist().index(eos) + 1) if eos in row[1:].tolist() else seq.shape[1] - 1 for row in seq]
    return BeamSearchOutput(seq[:, : 1 + max(n_tok)].clone(), out.sequences_scores[:k].clone())
