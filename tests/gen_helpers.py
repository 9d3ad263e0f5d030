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
        # the d_model^-0.5 output rescale: transformers 5's scale_decoder_outputs, else (transformers 4) the tie flag
        self.tied = bool(cfg.get("scale_decoder_outputs", cfg.get("tie_word_embeddings", False)))

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


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """x rounded to bf16 (nearest even), returned in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def _keep(x: torch.Tensor) -> torch.Tensor:
    return x


class T5DecodeEmu:
    """The decoder step of ``rp_decoder_step`` restated in torch at ``dtype`` (float64 by default), rounding to bf16 at
    exactly the points the HIP kernels do (``rounding=False``: none, i.e. fp32 weights computed in ``dtype``):

    - GEMM weights (self q / k / v / o, cross q / k / v / o, wi_0 / wi_1, wo, lm_head) are bf16; the embedding, the norm
      weights and the relative-position table stay fp32;
    - every RMSNorm output is rounded (on a scaled lm_head after the d_model^-0.5 factor); q, k, v, the self-attention
      cache and the cross K/V are rounded;
    - attention: scores (+ bias) unrounded, ``sum(e v) / sum(e)`` rounded; each o-projection adds to the unrounded
      residual; the FFN's inner rows are ``bf16(gelu_new(a0) a1)``; the lm_head output and log_softmax are unrounded.

    Addressing is ``T5Fp32``'s: a flat cache of ``max_len * nb`` rows read through the beam driver's ancestry table, the
    bias indexed by the distance query - key.  The source is the engine's bf16 ``encode_hidden`` output (or any [S, D]
    tensor), so encoder error stays out of a decoder comparison.  It never calls the HIP library.

    ``mutant`` plants one known bug (``MUTANTS``) so that tests can show a comparison would notice it."""

    MUTANTS = ("bias_off_by_one", "drop_last_key", "cross_short", "ancestry_identity", "tied_scale_missing")

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device="cpu", dtype=torch.float64, rounding: bool = True,
                 mutant=None):
        assert mutant is None or mutant in self.MUTANTS, mutant
        self.cfg, self.mutant, self.dtype = cfg, mutant, dtype
        self.device = torch.device(device)
        self.r = bf16_round if rounding else _keep
        self.H, self.dk = cfg["num_heads"], cfg["d_kv"]
        self.eps = cfg.get("layer_norm_epsilon", 1e-6)
        self.L = cfg["num_decoder_layers"]

        def gemm_w(k):
            w = sd[k].detach().to(torch.float32)
            return (w.to(torch.bfloat16) if rounding else w).to(device=self.device, dtype=dtype)

        def fp32_w(k):
            return sd[k].detach().to(torch.float32).to(device=self.device, dtype=dtype)

        self.embed = fp32_w("shared.weight")
        self.tab = fp32_w("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")
        self.final_ln = fp32_w("decoder.final_layer_norm.weight")
        tied = bool(cfg.get("tie_word_embeddings", False))
        self.lm = gemm_w("lm_head.weight" if "lm_head.weight" in sd else "shared.weight")
        scaled = bool(cfg.get("scale_decoder_outputs", tied)) and mutant != "tied_scale_missing"
        self.out_scale = cfg["d_model"] ** -0.5 if scaled else 1.0
        self.layers = []
        for i in range(self.L):
            p = f"decoder.block.{i}.layer."
            self.layers.append(dict(
                ln_self=fp32_w(p + "0.layer_norm.weight"), ln_cross=fp32_w(p + "1.layer_norm.weight"),
                ln_ff=fp32_w(p + "2.layer_norm.weight"),
                **{n: gemm_w(p + k) for n, k in (
                    ("q", "0.SelfAttention.q.weight"), ("k", "0.SelfAttention.k.weight"),
                    ("v", "0.SelfAttention.v.weight"), ("o", "0.SelfAttention.o.weight"),
                    ("cq", "1.EncDecAttention.q.weight"), ("ck", "1.EncDecAttention.k.weight"),
                    ("cv", "1.EncDecAttention.v.weight"), ("co", "1.EncDecAttention.o.weight"),
                    ("wi_0", "2.DenseReluDense.wi_0.weight"), ("wi_1", "2.DenseReluDense.wi_1.weight"),
                    ("wo", "2.DenseReluDense.wo.weight"))}))

    def _norm(self, x, w, scale=1.0):
        return self.r(w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)) * scale)

    def _attend(self, q, k, v, bias=None):
        """q [nb, H, dk], k / v [nb or 1, H, n, dk] -> bf16(softmax(q k^T + bias) v) [nb, H * dk]"""
        s = torch.einsum("bhd,bhnd->bhn", q, k)
        if bias is not None:
            s = s + bias
        e = torch.exp(s - s.amax(-1, keepdim=True))
        return self.r(torch.einsum("bhn,bhnd->bhd", e, v) / e.sum(-1)[..., None]).reshape(q.shape[0], -1)

    def start(self, enc: torch.Tensor, num_beams: int, max_len: int) -> None:
        """Cross K/V of one source [S, d_model] (shared by all beams) and an empty cache of ``max_len * nb`` rows."""
        enc = enc.to(device=self.device, dtype=self.dtype)
        if self.mutant == "cross_short":
            enc = enc[:-1]
        S, H, dk = enc.shape[0], self.H, self.dk
        self.nb = num_beams
        self.ck = [self.r(enc @ l["ck"].T).view(S, H, dk).transpose(0, 1)[None] for l in self.layers]
        self.cv = [self.r(enc @ l["cv"].T).view(S, H, dk).transpose(0, 1)[None] for l in self.layers]
        inner = H * dk
        self.kc = torch.zeros(self.L, max_len * num_beams, inner, device=self.device, dtype=self.dtype)
        self.vc = torch.zeros_like(self.kc)
        j = np.arange(max_len + 1)  # distance query - key
        bk = unidirectional_bucket(-j, self.cfg["relative_attention_num_buckets"],
                                   self.cfg["relative_attention_max_distance"])
        self.bias = self.tab[torch.from_numpy(bk).to(self.device)].T.contiguous()  # [H, max_len + 1]

    def step(self, tokens: torch.Tensor, ancestry: torch.Tensor) -> torch.Tensor:
        """One decode step (the beam driver's ``step``): log-probs [nb, V] in ``dtype``."""
        nb, T = ancestry.shape
        t = T - 1
        H, dk = self.H, self.dk
        x = self.embed[tokens.to(self.device).long()]
        dist = t - torch.arange(T, device=self.device)
        rows = ancestry.to(self.device).long()
        if self.mutant == "bias_off_by_one":
            dist = dist + 1
        if self.mutant == "ancestry_identity":
            rows = torch.arange(T, device=self.device)[None] * nb + torch.arange(nb, device=self.device)[:, None]
        n = T - 1 if (self.mutant == "drop_last_key" and t > 256) else T
        bias = self.bias[:, dist[:n]][None]  # [1, H, n]
        for i, l in enumerate(self.layers):
            h = self._norm(x, l["ln_self"])
            q = self.r(h @ l["q"].T)
            self.kc[i, t * nb : (t + 1) * nb] = self.r(h @ l["k"].T)
            self.vc[i, t * nb : (t + 1) * nb] = self.r(h @ l["v"].T)
            k = self.kc[i][rows[:, :n]].view(nb, n, H, dk).transpose(1, 2)
            v = self.vc[i][rows[:, :n]].view(nb, n, H, dk).transpose(1, 2)
            x = x + self._attend(q.view(nb, H, dk), k, v, bias) @ l["o"].T
            h = self._norm(x, l["ln_cross"])
            q = self.r(h @ l["cq"].T).view(nb, H, dk)
            x = x + self._attend(q, self.ck[i], self.cv[i]) @ l["co"].T
            h = self._norm(x, l["ln_ff"])
            x = x + self.r(_gelu(h @ l["wi_0"].T) * (h @ l["wi_1"].T)) @ l["wo"].T
        h = self._norm(x, self.final_ln, self.out_scale)
        return torch.log_softmax(h @ self.lm.T, dim=-1)

    def teacher_forced(self, enc: torch.Tensor, target: np.ndarray, max_len=None) -> torch.Tensor:
        """log-probs [len(target), V] of one sequence fed token by token (target[0] = the start token)."""
        T = len(target)
        self.start(enc, 1, max_len or T)
        tgt = torch.as_tensor(np.asarray(target, dtype=np.int64))
        out = [self.step(tgt[t : t + 1], torch.arange(t + 1)[None])[0] for t in range(T)]
        return torch.stack(out)


def source_ids(n_bytes: int, seed: int) -> np.ndarray:
    """A synthetic source of ``n_bytes`` byte ids (ByT5: byte + 3) whose last id is EOS; one byte is EOS alone."""
    if n_bytes == 1:
        return np.array([1], dtype=np.int32)
    from reprover_amd import synth

    text = synth.synth_text(np.random.default_rng(seed), n_bytes + 8)
    ids = np.frombuffer(text.encode("utf-8"), dtype=np.uint8).astype(np.int32)[: n_bytes - 1] + 3
    return np.concatenate([ids, [1]]).astype(np.int32)


def simulated_search(nb: int, steps: int, seed: int, tokens_range=(3, 259)):
    """A seeded stand-in for beam search: yields ``(t, tokens [nb], ancestry [nb, t + 1])`` per step, the table built as
    ``generation.beam_search`` builds it (column t = rows ``t * nb + b``, then rows reordered by the parents of the kept
    beams).  Parents are drawn with repeats, skewed towards low slots as the best beams' children are, so rows of the
    table are shared (a many-to-one reorder, not a permutation)."""
    rng = np.random.default_rng(seed)
    anc = np.zeros((nb, 0), dtype=np.int64)
    for t in range(steps):
        anc = np.concatenate([anc, (t * nb + np.arange(nb))[:, None]], axis=1)
        tok = rng.integers(*tokens_range, size=nb) if t else np.zeros(nb, dtype=np.int64)
        yield t, torch.from_numpy(tok), torch.from_numpy(anc.copy())
        src = np.minimum(rng.geometric(0.25, size=nb) - 1, nb - 1)
        if nb > 1 and t % 7 == 3:
            src = rng.permutation(nb)  # now and then a plain permutation as well
        anc = anc[src]


# Tolerances of the HIP decoder against T5DecodeEmu: case -> (max |d log-prob| over every step and entry, rms over all);
# measured on the MI355X (tests/test_decoder_parity_gpu.py prints the margins) with headroom.
DECODER_TOL = {  # measured: max, rms, top-2nb candidates max
    "tiny-sharp/nb1": (0.3, 0.03),                  # 0.15, 0.018
    "tiny-sharp/nb3": (0.35, 0.025, 0.15),          # 0.19, 0.013, 0.079
    "tiny-sharp/nb64": (0.45, 0.025, 0.2),          # 0.28, 0.012, 0.13
    "tiny-sharp/nb3/src1": (0.1, 0.006, 0.04),      # 0.041, 0.0029, 0.017
    "byt5-small-sharp/nb64": (0.8, 0.08, 0.5),      # 0.53, 0.054, 0.31
    "byt5-small-sharp/nb8": (1.0, 0.09, 0.55),      # 0.66, 0.061, 0.35
    "tiny-tied": (0.05, 0.006, 0.025),              # 0.022, 0.0031, 0.0087
    "g21b": (0.025, 0.0012),                        # 0.011, 0.00053
    "g21c": (0.4, 0.06),                            # 0.19, 0.030
    "g21b/hf": (0.05,),                             # 0.023 (against HF fp32)
    "g21c/hf": (0.8,),                              # 0.39 (against HF fp32)
    "generate/rescore": (0.8,),                     # 0.42 (sums over up to 127 tokens)
    # tests/test_decode_step_kernels_gpu.py's whole step (d_model 520, d_ff 2056, H 3, V 300, buckets (8, 16)): 2 x measured,
    # the rms capped at tiny-sharp/nb3's
    "step-d520-f2056-h3-v300/nb5": (0.28, 0.025),   # 0.14, 0.014
}
# running scores per beam row in the selection checks (nats between rows): candidates then mix many rows
SELECT_SPREAD = {"tiny-sharp": 0.2, "byt5-small-sharp": 1.0, "tiny-tied": 0.025}


# rp_encode_hidden against the fp32 encoder reference (HF-scale weights), element-wise |d| <= a |ref| + b: config -> (a, b)
ENCODER_TOL = {"tiny": (2 ** -6, 0.04), "byt5-small": (2 ** -6, 0.08)}  # HF scale; measured b: 0.025, 0.057
