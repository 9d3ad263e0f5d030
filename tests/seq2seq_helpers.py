"""Float64 teacher-forced reference of ``rp_decoder_forward`` (the batched seq2seq forward) for the seq2seq tests.

``T5ForwardEmu`` runs a whole target at once with a causal mask.  It rounds to bf16 where the forward's kernels round:
every point ``T5DecodeEmu`` lists (tests/gen_helpers.py) plus one the flash attention adds.

- R_P: the attention probabilities ``exp(s - max)`` are rounded to bf16 before they multiply V (the PV MFMA).  The
  normaliser ``sum(exp(s - max))`` stays unrounded.  This holds for self- and cross-attention.

The kernel's online softmax rounds ``exp(s - running max)`` and rescales in fp32.  The reference uses the final row max
instead; the two differ by at most one bf16 rounding per probability.  With ``rounding=False`` nothing is rounded and the
weights are the fp32 ones: HF fp32 computed in float64.

``mutant`` plants one bug (``MUTANTS``) so that a test can show the comparisons notice it.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from gen_helpers import T5DecodeEmu, _gelu, unidirectional_bucket

MUTANTS = ("future_key", "next_source", "labels_shifted", "count_ignored", "mean_all")


class T5ForwardEmu(T5DecodeEmu):
    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device="cpu", dtype=torch.float64, rounding: bool = True,
                 mutant: Optional[str] = None):
        assert mutant is None or mutant in MUTANTS, mutant
        super().__init__(cfg, sd, device, dtype, rounding)
        self.fmutant = mutant

    def _flash(self, q, k, v, bias=None, causal=False):
        """q [H, T, dk], k / v [H, S, dk] -> [T, H * dk]: bf16(sum(bf16(p) v) / sum(p))"""
        s = torch.einsum("htd,hsd->hts", q, k)
        if bias is not None:
            s = s + bias
        if causal:
            T = q.shape[1]
            allowed = torch.ones(T, T, dtype=torch.bool, device=s.device).tril()
            if self.fmutant == "future_key":
                allowed = allowed | torch.eye(T, dtype=torch.bool, device=s.device).roll(1, dims=1).triu()
            s = s.masked_fill(~allowed, float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("hts,hsd->htd", self.r(e), v) / e.sum(-1)[..., None]
        return self.r(o).transpose(0, 1).reshape(q.shape[1], -1)

    def pair_log_probs(self, enc: torch.Tensor, tokens: np.ndarray) -> torch.Tensor:
        """log-probs [T, V] of one pair: enc [S, D] (the encoder output), tokens [T] (the decoder inputs)."""
        enc = enc.to(device=self.device, dtype=self.dtype)
        T, S, H, dk = len(tokens), enc.shape[0], self.H, self.dk
        x = self.embed[torch.as_tensor(np.asarray(tokens, dtype=np.int64), device=self.device)]
        dist = np.arange(T)[:, None] - np.arange(T)[None]  # query - key
        bk = unidirectional_bucket(-np.maximum(dist, 0), self.cfg["relative_attention_num_buckets"],
                                   self.cfg["relative_attention_max_distance"])
        bias = self.tab[torch.from_numpy(bk).to(self.device)].permute(2, 0, 1)  # [H, T, T]
        for l in self.layers:
            h = self._norm(x, l["ln_self"])
            q, k, v = (self.r(h @ l[n].T).view(T, H, dk).transpose(0, 1) for n in ("q", "k", "v"))
            x = x + self._flash(q, k, v, bias, causal=True) @ l["o"].T
            h = self._norm(x, l["ln_cross"])
            q = self.r(h @ l["cq"].T).view(T, H, dk).transpose(0, 1)
            ck = self.r(enc @ l["ck"].T).view(S, H, dk).transpose(0, 1)
            cv = self.r(enc @ l["cv"].T).view(S, H, dk).transpose(0, 1)
            x = x + self._flash(q, ck, cv) @ l["co"].T
            h = self._norm(x, l["ln_ff"])
            x = x + self.r(_gelu(h @ l["wi_0"].T) * (h @ l["wi_1"].T)) @ l["wo"].T
        h = self._norm(x, self.final_ln, self.out_scale)
        return torch.log_softmax(h @ self.lm.T, dim=-1)

    def forward(self, encs, tactic_ids, rows: bool = False):
        """(loss, label log-probs [B, T] (0 where ignored)[, per-pair log-prob rows]) for padded labels ``tactic_ids``
        [B, T] (-100 = ignored) and one encoder output per pair (``encs[b]`` [S_b, D])."""
        from reprover_amd.decoder import shift_and_segment

        y = np.asarray(tactic_ids, dtype=np.int64)
        tokens, labels, cu = shift_and_segment(y)
        B, Tmax = y.shape
        out = torch.zeros((B, Tmax), dtype=self.dtype)
        all_rows = []
        total, count = 0.0, 0
        for b in range(B):
            n = int(cu[b + 1] - cu[b])
            if n == 0:
                all_rows.append(None)
                if self.fmutant in ("count_ignored", "mean_all"):
                    count += Tmax if self.fmutant == "mean_all" else int((y[b] == -100).sum())
                continue
            src = b if self.fmutant != "next_source" else (b + 1) % B
            if self.fmutant == "next_source" and encs[src] is None:
                src = b
            lp = self.pair_log_probs(encs[src], tokens[cu[b] : cu[b + 1]]).cpu()
            all_rows.append(lp)
            lab = labels[cu[b] : cu[b + 1]].astype(np.int64)
            if self.fmutant == "labels_shifted":
                lab = np.concatenate([lab[1:], lab[-1:]])
            keep = lab >= 0
            g = lp[torch.arange(n), torch.from_numpy(np.where(keep, lab, 0))]
            g = torch.where(torch.from_numpy(keep), g, torch.zeros((), dtype=g.dtype))
            out[b, :n] = g
            total -= float(g.sum())
            count += int(keep.sum())
            if self.fmutant == "count_ignored":
                count += int((~keep).sum()) + int((y[b, n:] == -100).sum())
            elif self.fmutant == "mean_all":
                count += Tmax - int(keep.sum())
        loss = total / count if count else float("nan")
        return (loss, out, all_rows) if rows else (loss, out)


def g23_inputs(tmp):
    """(split path, preds dict) of G23, rebuilt identically by the tests: 20 corpus files, 8 theorems; every state gets
    the first 6 premises of its own file, in reverse order."""
    import json
    import os

    from reprover_amd import synth
    from reprover_amd.common import Corpus

    files = synth.synth_corpus_records(20, 200, seed=231, max_imports=4)
    cpath = os.path.join(tmp, "corpus.jsonl")
    synth.write_corpus_jsonl(cpath, files)
    split = synth.synth_split(files, 8, seed=232, min_file=8)
    path = os.path.join(tmp, "val.json")
    with open(path, "w") as fh:
        json.dump(split, fh)
    corpus = Corpus(cpath)
    preds = {}
    for thm in split:
        prem = list(corpus.get_premises(thm["file_path"]))[:6][::-1]
        for tac in thm["traced_tactics"]:
            preds[(thm["file_path"], thm["full_name"], tac["state_before"])] = {"retrieved_premises": prem}
    return path, preds


# Tolerances of rp_decoder_forward against T5ForwardEmu: case -> (max |d log-prob|, rms over all counted labels);
# measured on the MI355X with headroom (tests/test_seq2seq_gpu.py prints the margins).
FORWARD_TOL = {  # measured: max, rms
    "tiny-sharp": (0.4, 0.05),          # 0.19, 0.032 (B = 8, targets up to 520)
    "byt5-small-sharp": (0.8, 0.1),     # 0.40, 0.071 (B = 64, sources 1 - 2300 bytes, targets 1 - 512)
}
STEP_TOL = 0.4  # rp_decoder_forward against the rp_decoder_step loop (other reduction orders, R_P): measured 0.16
