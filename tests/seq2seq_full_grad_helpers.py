"""Float64 reference gradients of the seq2seq loss for the WHOLE model (``HipSeq2SeqGradients``):
a float64 restatement of the T5 encoder (``Enc64``) composed with the decoder reference of tests/seq2seq_grad_helpers.py
through autograd, every weight a leaf.

The composition is the implementation's: the decoder reference differentiates the loss with the encoder rows as leaves
(``reference_grads``: decoder gradients + d_enc), then d_enc is pushed back through the encoder graph.  ``shared.weight``
is the encoder's embedding gradient + the decoder's entry.

``rounding=False`` is HF fp32 computed in float64 (the reference).  ``rounding=True`` keeps the bf16 rounding points of the
training forward (differentiated through the casts, as HF's bf16 autograd does): the GEMM A operand ``bf16(x)``, the
norm weight folded into the bf16 projection weights, q / k / v, the attention probabilities and output, the gated FFN's
inner rows, and the bf16 hidden rows of the hand-over.  The residual stream itself is not rounded (two bf16 planes)."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from gen_helpers import _gelu, bf16_round
from oracle.t5_ref import relative_position_bucket
from seq2seq_grad_helpers import G25_SRC, reference_grads

ENC_KEYS = {
    "ln_attn": "layer.0.layer_norm.weight", "q": "layer.0.SelfAttention.q.weight", "k": "layer.0.SelfAttention.k.weight",
    "v": "layer.0.SelfAttention.v.weight", "o": "layer.0.SelfAttention.o.weight", "ln_ff": "layer.1.layer_norm.weight",
    "wi_0": "layer.1.DenseReluDense.wi_0.weight", "wi_1": "layer.1.DenseReluDense.wi_1.weight",
    "wo": "layer.1.DenseReluDense.wo.weight",
}
ENC_REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
ENC_FINAL_LN = "encoder.final_layer_norm.weight"

# The G26 batch: G25's shapes with byte sources instead of given encoder rows.  564 source tokens pad to 640 rows; 129
# and 300 cross the 128-row tiles; the fourth pair has no label (an all-zero block of d_enc).
G26_SRC = G25_SRC


def g26_sources(seed: int = 26) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.integers(3, 259, size=s - 1), [1]]).astype(np.int64) for s in G26_SRC]


def padded_sources(srcs: List[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    S = max(len(s) for s in srcs)
    ids, mask = np.zeros((len(srcs), S), np.int64), np.zeros((len(srcs), S), np.int64)
    for b, s in enumerate(srcs):
        ids[b, : len(s)] = s
        mask[b, : len(s)] = 1
    return ids, mask


# Planted bugs of the whole-model gradient -> the tensor each is aimed at
# (the last two change the residual gradient entering the top layer - tiny has two.  The dropped term is the part of that
# gradient along x, which the top layer's norm-weight gradient, a sum of dh x rs, feels most; misrouted rows move every
# tensor, the top FFN-out weight first.)
FULL_MUTANTS = {
    "embed_not_added": "shared.weight",  # the encoder's embedding gradient is not added into shared.weight
    # the - x rs^3 mean(dh w x) term of the final norm's backward is dropped
    "final_norm_mean_dropped": "encoder.block.1.layer.1.layer_norm.weight",
    "next_source": "encoder.block.1.layer.1.DenseReluDense.wo.weight",  # pair b's d_enc rows go to pair b + 1's source
}


class Enc64:
    """The T5 encoder of one unpadded sequence in float64 (HF modeling_t5.py T5Stack, eval mode), weights as leaves."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], rounding: bool = False, mutant: Optional[str] = None):
        self.cfg, self.mutant = cfg, mutant
        self.r = bf16_round if rounding else (lambda t: t)
        self.rounding = rounding
        self.H, self.dk, self.eps = cfg["num_heads"], cfg["d_kv"], cfg.get("layer_norm_epsilon", 1e-6)
        w = lambda k: sd[k].detach().to(torch.float64).clone().requires_grad_(True)  # noqa: E731
        self.leaves = {"shared.weight": w("shared.weight"), ENC_REL_BIAS: w(ENC_REL_BIAS), ENC_FINAL_LN: w(ENC_FINAL_LN)}
        for i in range(cfg["num_layers"]):
            for key in ENC_KEYS.values():
                self.leaves[f"encoder.block.{i}.{key}"] = w(f"encoder.block.{i}.{key}")

    def _rs(self, x, detach=False):
        x = x.detach() if detach else x
        return torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)

    def _proj(self, x, ln, W):
        """RMSNorm + projection as the trainer runs it: rs * (bf16(x) @ bf16(W * ln)^T); unrounded: the same product."""
        return (self.r(x) @ self.r(W * ln[None, :]).T) * self._rs(x)

    def forward(self, ids: np.ndarray) -> torch.Tensor:
        g = self.leaves
        S, H, dk = len(ids), self.H, self.dk
        x = g["shared.weight"][torch.from_numpy(np.asarray(ids, dtype=np.int64))]
        rel = np.arange(S)[None, :] - np.arange(S)[:, None]  # key - query
        bk = relative_position_bucket(rel, self.cfg["relative_attention_num_buckets"], self.cfg["relative_attention_max_distance"])
        bias = g[ENC_REL_BIAS][torch.from_numpy(bk)].permute(2, 0, 1)  # [H, S, S]
        for i in range(self.cfg["num_layers"]):
            L = {f: g[f"encoder.block.{i}.{key}"] for f, key in ENC_KEYS.items()}
            q, k, v = (self.r(self._proj(x, L["ln_attn"], L[n])).view(S, H, dk).transpose(0, 1) for n in ("q", "k", "v"))
            s = torch.einsum("htd,hsd->hts", q, k) + bias
            e = torch.exp(s - s.amax(-1, keepdim=True))
            a = self.r(torch.einsum("hts,hsd->htd", self.r(e), v) / e.sum(-1)[..., None]).transpose(0, 1).reshape(S, H * dk)
            x = x + a @ self.r(L["o"]).T
            ff = self.r(_gelu(self._proj(x, L["ln_ff"], L["wi_0"])) * self._proj(x, L["ln_ff"], L["wi_1"]))
            x = x + ff @ self.r(L["wo"]).T
        rs = self._rs(x, detach=self.mutant == "final_norm_mean_dropped")  # detached: no - x rs^3 mean(dh w x) term
        return self.r(g[ENC_FINAL_LN] * (x * rs))


def reference_full_grads(cfg: Dict, sd: Dict[str, torch.Tensor], sources: List[np.ndarray], tactic_ids,
                         rounding: bool = False, mutant: Optional[str] = None, want_hidden: bool = False):
    """(loss, {HF parameter name: d loss / d parameter}, d_enc packed[, hidden rows per pair]) in float64 for the model of
    ``sd`` on (sources, padded labels).  ``lm_head.weight`` appears when the head is untied."""
    assert mutant is None or mutant in FULL_MUTANTS, mutant
    tied = bool(cfg["tie_word_embeddings"])
    enc = Enc64(cfg, sd, rounding, mutant)
    hidden = [enc.forward(s) for s in sources]
    loss, grads, d_enc = reference_grads(cfg, sd, [h.detach() for h in hidden], tactic_ids, rounding=rounding, tied=tied,
                                         mutant="next_source" if mutant == "next_source" else None)
    torch.autograd.backward(hidden, [torch.from_numpy(d) for d in d_enc])
    grads = dict(grads)
    for k, t in enc.leaves.items():
        ge = (torch.zeros_like(t) if t.grad is None else t.grad).numpy()
        if k == "shared.weight":
            grads[k] = grads[k] if mutant == "embed_not_added" else ge + grads[k]
        else:
            grads[k] = ge
    out = (loss, grads, np.concatenate(d_enc))
    return out + ([h.detach().numpy() for h in hidden],) if want_hidden else out


G26_STRIDE = 8       # every 8th element of the tensors this fixture is the first to pin: shared.weight and encoder.*
G26_STRIDE_DEC = 32  # decoder-only tensors (pinned at stride 8 by G25 already): every 32nd, which keeps the file below G25's size


def g26_stride(name: str) -> int:
    return G26_STRIDE if (name == "shared.weight" or name.startswith("encoder.")) else G26_STRIDE_DEC


def load_g26(golden_dir: str, name: str) -> Dict:
    """One configuration of tests/golden/g26_seq2seq_full_grad.npz (make_golden_seq2seq_full_grad.py), in load_g25's form."""
    import json
    import os

    z = np.load(os.path.join(golden_dir, "g26_seq2seq_full_grad.npz"))
    meta = json.loads(bytes(z["meta"]).decode())[name]
    out = dict(labels=z[f"{name}_labels"].astype(np.int64), loss=z[f"{name}_loss"], tensors={})
    for i, k in enumerate(meta["tensors"]):
        n2, mx, e2, em = z[f"{name}_figures"][i]
        out["tensors"][k] = dict(sample=z[f"{name}_s{i}"], norm=float(n2), max=float(mx), bf16_l2=float(e2),
                                 bf16_max=float(em))
    return out


# HipSeq2SeqGradients.loss_and_grads against reference_full_grads(rounding=False) on G26, per tensor: no worse than
# HF-bf16 autograd's own error on that tensor (the fixture's figures), on both metrics.  Exceptions by (config, tensor) ->
# (relative L2 bound, max / max bound), each 2 x the figure measured on the MI355X (in the comment), allowed only where the
# other metric is inside its bar.  Measured: every tensor of both configurations is inside HF-bf16's figures on both
# metrics (worst 0.75 of the bar on relative L2, 0.86 on max / max), so the table is empty.
FULL_GRAD_TOL: Dict[Tuple[str, str], Tuple[float, float]] = {}
