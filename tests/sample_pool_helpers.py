"""The sampled pool's reference sampler: tests/sample_helpers.py's ``CpuSampler`` with a position per slot - the same
``reference_sample`` and ``uniforms``, ``rp_sample_pool_step``'s bookkeeping.  With every ``pos = t`` it is ``CpuSampler``
at ``t``.  It never launches anything.
"""
from __future__ import annotations

import numpy as np
import torch

from sample_helpers import reference_sample, uniforms


class CpuPoolSampler:
    """``SamplePool``'s ``sample_step`` on the host (and, through ``at``, ``sample_search``'s): slot ``active[a]`` draws
    at ``pos[a]`` and writes column ``pos[a] + 1``.  ``min_margin`` is the smallest decision margin of any live row it
    drew; ``calls`` the ``(active, pos)`` lists it was handed."""

    def __init__(self, lib, temperature=1.0, top_k=0, top_p=1.0, eos=1, pad=0):
        self.lib, self.T, self.k, self.p, self.eos, self.pad = lib, temperature, top_k, top_p, eos, pad
        self.min_margin = np.inf
        self.calls = []

    def __call__(self, log_probs: torch.Tensor, active, pos, st) -> None:
        n, nb, max_len = st.seq.shape
        assert len(active) == len(pos) and all(0 <= p <= max_len - 2 for p in pos), (pos, max_len)
        self.calls.append((list(active), list(pos)))
        lp = log_probs.detach().cpu().numpy().astype(np.float32)
        u = np.concatenate([uniforms(self.lib, [int(st.seeds[i])] * nb, range(nb), p) for i, p in zip(active, pos)])
        toks, _, margins, _ = reference_sample(lp, u, self.T, self.k, self.p)
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
        """``sample_search_batch``'s ``sample_step``: every slot at ``t``."""
        self(log_probs, active, [t] * len(active), st)
