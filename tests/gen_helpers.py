"""Pure-torch fp32 restatement of T5ForConditionalGeneration for the generator tests (CPU or any device).

Encoder: RMSNorm / bidirectional-bias self-attention / gated-GELU blocks (modeling_t5.py).  Decoder: one step at a time
through a flat key/value cache addressed by the beam driver's ancestry table (reprover_amd/generation.py): causal
self-attention with the unidirectional bucket bias, cross-attention over the source without bias, gated-GELU FFN, final
norm, optional ``d_model ** -0.5`` rescale when embeddings are tied, ``lm_head``, ``log_softmax``.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import t5_ref


def unidirectional_bucket(d, num_buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """``T5Attention._relative_position_bucket(key - query, bidirectional=False)`` for ``d = key - query`` (int array)."""
    rel = -np.minimum(np.asarray(d, dtype=np.int64), 0)
    max_exact = num_buckets // 2
    with np.errstate(divide="ignore"):
        ratio = torch.from_numpy(rel.astype(np.float32)) / max_exact
        large = max_exact + (torch.log(ratio) / math.log(max_distance / max_exact)
                             * (num_buckets - max_exact)).to(torch.long).numpy()
    large = np.minimum(large, num_buckets - 1)
    return np.where(rel < max_exact, rel, large)


def _rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _gelu(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * torch.pow(u, 3.0))))


class T5Fp32:
    """fp32 T5 seq2seq over an HF-keyed state dict."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device="cpu"):
        self.cfg = cfg
        self.w = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in sd.items()}
        self.device = torch.device(device)
        self.H, self.dk = cfg["num_heads"], cfg["d_kv"]
        self.eps = cfg.get("layer_norm_epsilon", 1e-6)
        self.L = cfg["num_decoder_layers"]
        self.lm = self.w["lm_head.weight"] if "lm_head.weight" in self.w else self.w["shared.weight"]
        self.tied = bool(cfg.get("tie_word_embeddings", False))

    # -- encoder ---------------------------------------------------------------------------------
    def encode(self, ids: np.ndarray) -> torch.Tensor:
        """last_hidden_state [S, D] of one source (final RMSNorm applied)."""
        ids2 = np.asarray(ids, dtype=np.int64)[None]
        w = {k: v.cpu() for k, v in self.w.items() if k.startswith("encoder.") or k == "shared.weight"}
        return t5_ref._encoder_forward(self.cfg, w, ids2, np.ones_like(ids2))[0].to(self.device)

    # -- decoder ---------------------------------------------------------------------------------
    def start(self, enc: torch.Tensor, num_beams: int, max_len: int) -> None:
        """Cross K/V of the source (shared by all beams) and an empty self-attention cache of ``max_len * nb`` rows."""
        S = enc.shape[0]
        self.nb = num_beams
        self.ck, self.cv = [], []
        for i in range(self.L):
            p = f"decoder.block.{i}.layer.1.EncDecAttention."
            self.ck.append((enc @ self.w[p + "k.weight"].T).view(S, self.H, self.dk).transpose(0, 1))
            self.cv.append((enc @ self.w[p + "v.weight"].T).view(S, self.H, self.dk).transpose(0, 1))
        inner = self.H * self.dk
        self.kc = torch.zeros(self.L, max_len * num_beams, inner, device=self.device)
        self.vc = torch.zeros_like(self.kc)
        tab = self.w["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        d = -np.arange(max_len)  # key - query for key = query - j
        bk = unidirectional_bucket(d, self.cfg["relative_attention_num_buckets"],
                                   self.cfg["relative_attention_max_distance"])
        self.bias = tab[torch.from_numpy(bk).to(self.device)].T.contiguous()  # [H, max_len] by distance j = q - k

    def step(self, tokens: torch.Tensor, ancestry: torch.Tensor) -> torch.Tensor:
        """One decode step (the beam driver's ``step``): log-probs [nb, V]."""
        nb, T = ancestry.shape
        t = T - 1
        H, dk = self.H, self.dk
        x = self.w["shared.weight"][tokens.to(self.device)]
        dist = t - torch.arange(T, device=self.device)
        bias = self.bias[:, dist]  # [H, T]
        rows = ancestry.to(self.device)
        for i in range(self.L):
            p = f"decoder.block.{i}.layer."
            h = _rms(x, self.w[p + "0.layer_norm.weight"], self.eps)
            q = h @ self.w[p + "0.SelfAttention.q.weight"].T
            self.kc[i, t * nb : (t + 1) * nb] = h @ self.w[p + "0.SelfAttention.k.weight"].T
            self.vc[i, t * nb : (t + 1) * nb] = h @ self.w[p + "0.SelfAttention.v.weight"].T
            k = self.kc[i][rows].view(nb, T, H, dk).transpose(1, 2)  # [nb, H, T, dk]
            v = self.vc[i][rows].view(nb, T, H, dk).transpose(1, 2)
            s = torch.einsum("bhd,bhtd->bht", q.view(nb, H, dk), k) + bias[None]
            a = torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), v).reshape(nb, H * dk)
            x = x + a @ self.w[p + "0.SelfAttention.o.weight"].T
            h = _rms(x, self.w[p + "1.layer_norm.weight"], self.eps)
            q = (h @ self.w[p + "1.EncDecAttention.q.weight"].T).view(nb, H, dk)
            s = torch.einsum("bhd,hsd->bhs", q, self.ck[i])
            a = torch.einsum("bhs,hsd->bhd", torch.softmax(s, -1), self.cv[i]).reshape(nb, H * dk)
            x = x + a @ self.w[p + "1.EncDecAttention.o.weight"].T
            h = _rms(x, self.w[p + "2.layer_norm.weight"], self.eps)
            g = _gelu(h @ self.w[p + "2.DenseReluDense.wi_0.weight"].T) * (h @ self.w[p + "2.DenseReluDense.wi_1.weight"].T)
            x = x + g @ self.w[p + "2.DenseReluDense.wo.weight"].T
        x = _rms(x, self.w["decoder.final_layer_norm.weight"], self.eps)
        if self.tied:
            x = x * self.cfg["d_model"] ** -0.5
        return Fn.log_softmax(x @ self.lm.T, dim=-1)

    def teacher_forced(self, enc: torch.Tensor, target: np.ndarray) -> torch.Tensor:
        """log-probs [len(target), V] of one sequence fed token by token (target[0] = the start token)."""
        T = len(target)
        self.start(enc, 1, T)
        out = []
        for t in range(T):
            anc = torch.arange(t + 1, dtype=torch.int64)[None]
            out.append(self.step(torch.tensor([int(target[t])]), anc)[0])
        return torch.stack(out)
