"""Float64 reference of the whole seq2seq model UNDER GIVEN DROPOUT MASKS, for
tests/test_seq2seq_dropout_cpu.py (pinned to HF's train mode, planted mutants) and the GPU tests (the masks a step used,
read back with ``rp_dbg_dropout_mask``).

``DropEnc64`` extends ``Enc64`` (tests/seq2seq_full_grad_helpers.py) and ``DropDecEmu`` the decoder reference
(tests/seq2seq_grad_helpers.py) with one multiplier tensor per (site, pair); ``reference_full_grads_dropout`` composes them
as ``reference_full_grads`` does.  ``rounding=False`` is HF fp32 in float64; ``rounding=True`` keeps the engine's rounding
points, each mask applied where the engine applies it: on the fp32 value BEFORE the rounding, on the probabilities after
the row sum (the normaliser stays undropped).

Masks come from a provider ``masks(half, kind, layer, pair, shape) -> float64 multipliers`` (0 or 1 / (1 - p)):
half "enc": kinds embed, probs, attn_resid, ff_inner, ff_resid, final; half "dec": embed, self_probs, self_resid,
cross_probs, cross_resid, ff_inner, ff_resid, final.  Probabilities have shape (H, queries, keys), the rest (tokens,
features).  ``layer`` is None for embed / final."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from gen_helpers import _gelu, unidirectional_bucket
from oracle.t5_ref import relative_position_bucket
from seq2seq_full_grad_helpers import ENC_FINAL_LN, ENC_KEYS, ENC_REL_BIAS, Enc64
from seq2seq_grad_helpers import LAYER_KEYS, REL_BIAS, _GradEmu

ENC_KINDS = {"probs": 0, "attn_resid": 1, "ff_inner": 2, "ff_resid": 3}
DEC_KINDS = {"self_probs": 0, "self_resid": 1, "cross_probs": 2, "cross_resid": 3, "ff_inner": 4, "ff_resid": 5}

# Planted bugs of the dropout path -> the tensor each is aimed at (tiny: two layers per stack)
DROP_MUTANTS = {
    "renormalised": "decoder.block.0.layer.0.SelfAttention.v.weight",  # probabilities renormalised after the mask
    "scale_missing": "decoder.block.0.layer.0.SelfAttention.o.weight",  # 1 / (1 - p) missing at layer 0's self residual site
    "cross_reads_self": "decoder.block.0.layer.1.EncDecAttention.v.weight",  # cross probs read the self-probs site's masks
    "resid_forward_only": "decoder.block.1.layer.2.DenseReluDense.wo.weight",  # a residual mask not applied to the branch's dx
    "ff_inner_bwd_missing": "decoder.block.1.layer.2.DenseReluDense.wi_0.weight",  # no FFN-inner mask in the gated-GELU backward
    "enc_final_bwd_missing": "encoder.final_layer_norm.weight",  # the encoder's final mask missing from d_hidden
    "delta_undropped": "decoder.block.0.layer.0.SelfAttention.q.weight",  # delta = rowsum(dO . O) from the UNDROPPED output
}


def ones_masks(half, kind, layer, pair, shape):
    return torch.ones(shape, dtype=torch.float64)


class RandomMasks:
    """Bernoulli(1 - p) / (1 - p) multipliers, a fixed table per (half, kind, layer, pair) cut to the asked shape: the
    same element for the same (row, column) whatever shape asks for it, as a counter-based mask behaves."""

    def __init__(self, p: float, seed: int, rows: int = 320, keys: int = 320, features: int = 1024):
        self.p, self.seed, self.rows, self.keys, self.features = p, seed, rows, keys, features
        self._tabs: Dict = {}

    def __call__(self, half, kind, layer, pair, shape):
        key = (half, kind, layer, pair)
        probs = len(shape) == 3
        if key not in self._tabs:
            order = sorted(list(ENC_KINDS) + list(DEC_KINDS) + ["embed", "final"])
            s = [self.seed, 0 if half == "enc" else 1, order.index(kind), -1 if layer is None else layer, pair]
            rng = np.random.default_rng([x + 2 for x in s])
            full = (shape[0], self.rows, self.keys) if probs else (self.rows, self.features)
            self._tabs[key] = rng.random(full) >= self.p
        t = self._tabs[key]
        assert all(a <= b for a, b in zip(shape, t.shape)), (key, shape, t.shape)
        cut = t[:, : shape[1], : shape[2]] if probs else t[: shape[0], : shape[1]]
        return torch.from_numpy(cut.astype(np.float64) / (1.0 - self.p))


class _MutantSoftmax(torch.autograd.Function):
    """softmax(s) * m whose backward takes delta from the UNDROPPED output: dS = P (M dP - rowsum(P dP))."""

    @staticmethod
    def forward(ctx, s, m):
        p = torch.softmax(s, dim=-1)
        ctx.save_for_backward(p, m)
        return p * m

    @staticmethod
    def backward(ctx, g):
        p, m = ctx.saved_tensors
        return p * (m * g - (p * g).sum(-1, keepdim=True)), None


def _fwd_only(value, unmasked):
    """`value` in the forward, the gradient of `unmasked` in the backward (a mask the backward forgot)"""
    return value.detach() + (unmasked - unmasked.detach())


def drop_attention(r, q, k, v, bias, causal, m, mutant=None):
    """q [H, T, dk], k / v [H, S, dk], m [H, T, S] -> [T, H * dk]: r(sum(r(e m) v) / sum(e)), the normaliser undropped"""
    s = torch.einsum("htd,hsd->hts", q, k)
    if bias is not None:
        s = s + bias
    if causal:
        T = q.shape[1]
        s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = (e * m).sum(-1) if mutant == "renormalised" else e.sum(-1)
    if mutant == "delta_undropped":
        pm = _MutantSoftmax.apply(s, m)
        pm = pm + (r(e * m) / den[..., None] - pm).detach()  # the stand-in's values, the mutant's gradient
        o = torch.einsum("hts,hsd->htd", pm, v)
    else:
        o = torch.einsum("hts,hsd->htd", r(e * m), v) / den[..., None]
    return r(o).transpose(0, 1).reshape(q.shape[1], -1)


class DropEnc64(Enc64):
    """``Enc64`` in T5's training mode under given masks (HF's six encoder sites)."""

    def __init__(self, cfg, sd, rounding=False, masks=ones_masks, mutant: Optional[str] = None, p: float = 0.0):
        super().__init__(cfg, sd, rounding, None)
        self.masks, self.dmutant, self.p = masks, mutant, p

    def forward(self, ids: np.ndarray, pair: int = 0) -> torch.Tensor:
        g, M = self.leaves, (lambda kind, layer, shape: self.masks("enc", kind, layer, pair, shape))
        S, H, dk, D, F = len(ids), self.H, self.dk, self.cfg["d_model"], self.cfg["d_ff"]
        x = M("embed", None, (S, D)) * g["shared.weight"][torch.from_numpy(np.asarray(ids, dtype=np.int64))]
        rel = np.arange(S)[None, :] - np.arange(S)[:, None]  # key - query
        bk = relative_position_bucket(rel, self.cfg["relative_attention_num_buckets"], self.cfg["relative_attention_max_distance"])
        bias = g[ENC_REL_BIAS][torch.from_numpy(bk)].permute(2, 0, 1)  # [H, S, S]
        for i in range(self.cfg["num_layers"]):
            L = {f: g[f"encoder.block.{i}.{key}"] for f, key in ENC_KEYS.items()}
            q, k, v = (self.r(self._proj(x, L["ln_attn"], L[n])).view(S, H, dk).transpose(0, 1) for n in ("q", "k", "v"))
            a = drop_attention(self.r, q, k, v, bias, False, M("probs", i, (H, S, S)))
            x = x + M("attn_resid", i, (S, D)) * (a @ self.r(L["o"]).T)
            ff = self.r(M("ff_inner", i, (S, F)) * (_gelu(self._proj(x, L["ln_ff"], L["wi_0"])) * self._proj(x, L["ln_ff"], L["wi_1"])))
            x = x + M("ff_resid", i, (S, D)) * (ff @ self.r(L["wo"]).T)
        h = g[ENC_FINAL_LN] * (x * self._rs(x))
        m = M("final", None, (S, D))
        return self.r(_fwd_only(m * h, h) if self.dmutant == "enc_final_bwd_missing" else m * h)


class DropDecEmu(_GradEmu):
    """The decoder reference in T5's training mode under given masks (HF's decoder sites)."""

    masks, dmutant, p = staticmethod(ones_masks), None, 0.0

    def pair_log_probs_dropout(self, enc, tokens, pair: int):
        enc = enc.to(device=self.device, dtype=self.dtype)
        T, S, H, dk, D, F = len(tokens), enc.shape[0], self.H, self.dk, self.cfg["d_model"], self.cfg["d_ff"]
        mut = self.dmutant
        M = lambda kind, layer, shape: self.masks("dec", kind, layer, pair, shape)  # noqa: E731
        x = M("embed", None, (T, D)) * self.embed[torch.as_tensor(np.asarray(tokens, dtype=np.int64))]
        dist = np.arange(T)[:, None] - np.arange(T)[None]  # query - key
        bk = unidirectional_bucket(-np.maximum(dist, 0), self.cfg["relative_attention_num_buckets"],
                                   self.cfg["relative_attention_max_distance"])
        bias = self.tab[torch.from_numpy(bk)].permute(2, 0, 1)  # [H, T, T]
        last = len(self.layers) - 1
        for i, l in enumerate(self.layers):
            h = self._norm(x, l["ln_self"])
            q, k, v = (self.r(h @ l[n].T).view(T, H, dk).transpose(0, 1) for n in ("q", "k", "v"))
            a = drop_attention(self.r, q, k, v, bias, True, M("self_probs", i, (H, T, T)), mut if i == 0 else None)
            m = M("self_resid", i, (T, D))
            if mut == "scale_missing" and i == 0:
                m = m * (1.0 - self.p)
            x = x + m * (a @ l["o"].T)
            h = self._norm(x, l["ln_cross"])
            q = self.r(h @ l["cq"].T).view(T, H, dk).transpose(0, 1)
            ck = self.r(enc @ l["ck"].T).view(S, H, dk).transpose(0, 1)
            cv = self.r(enc @ l["cv"].T).view(S, H, dk).transpose(0, 1)
            a = drop_attention(self.r, q, ck, cv, None, False,
                               M("self_probs" if mut == "cross_reads_self" else "cross_probs", i, (H, T, S)))
            x = x + M("cross_resid", i, (T, D)) * (a @ l["co"].T)
            h = self._norm(x, l["ln_ff"])
            inner = _gelu(h @ l["wi_0"].T) * (h @ l["wi_1"].T)
            m = M("ff_inner", i, (T, F))
            ff = self.r(_fwd_only(m * inner, inner) if (mut == "ff_inner_bwd_missing" and i == last) else m * inner)
            branch, m = ff @ l["wo"].T, M("ff_resid", i, (T, D))
            x = x + (_fwd_only(m * branch, branch) if (mut == "resid_forward_only" and i == last) else m * branch)
        h = self.final_ln * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)) * self.out_scale
        h = self.r(M("final", None, (T, D)) * h)
        return torch.log_softmax(h @ self.lm.T, dim=-1)


def reference_decoder_grads_dropout(cfg: Dict, sd: Dict[str, torch.Tensor], encs, tactic_ids, masks=ones_masks,
                                    rounding: bool = False, mutant: Optional[str] = None, p: float = 0.0, tied: bool = False):
    """``reference_grads`` (tests/seq2seq_grad_helpers.py) under ``masks``: (loss, {HF name: d loss / d decoder parameter},
    [d loss / d enc_b]) in float64 with the encoder rows ``encs`` as leaves."""
    from reprover_amd.decoder import shift_and_segment

    emu = DropDecEmu(cfg, sd, rounding=rounding)
    emu.masks, emu.dmutant, emu.p = masks, mutant, p
    leaves = {"shared.weight": emu.embed, "lm_head.weight": emu.lm, REL_BIAS: emu.tab,
              "decoder.final_layer_norm.weight": emu.final_ln}
    for i, l in enumerate(emu.layers):
        for fld, key in LAYER_KEYS.items():
            leaves[f"decoder.block.{i}.{key}"] = l[fld]
    for t in leaves.values():
        t.requires_grad_(True)
    encs = [e.detach().to(torch.float64).clone().requires_grad_(True) for e in encs]
    y = np.asarray(tactic_ids, dtype=np.int64)
    tokens, labels, cu = shift_and_segment(y)
    total, count = torch.zeros((), dtype=torch.float64), 0
    for b in range(y.shape[0]):
        n = int(cu[b + 1] - cu[b])
        if n == 0:
            continue
        lp = emu.pair_log_probs_dropout(encs[b], tokens[cu[b] : cu[b + 1]], b)
        lab = labels[cu[b] : cu[b + 1]].astype(np.int64)
        keep = lab >= 0
        g = lp[torch.arange(n), torch.from_numpy(np.where(keep, lab, 0))]
        total = total - g[torch.from_numpy(keep)].sum()
        count += int(keep.sum())
    if count:
        (total / count).backward()
    grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).numpy().astype(np.float64)  # noqa: E731
    grads = {k: grad(t) for k, t in leaves.items()}
    if tied:
        grads["shared.weight"] = grads["shared.weight"] + grads.pop("lm_head.weight")
    return (float(total.detach()) / count if count else float("nan")), grads, [grad(e) for e in encs]


def reference_full_grads_dropout(cfg: Dict, sd: Dict[str, torch.Tensor], sources: List[np.ndarray], tactic_ids,
                                 masks=ones_masks, rounding: bool = False, mutant: Optional[str] = None, p: float = 0.0):
    """(loss, {HF parameter name: d loss / d parameter}, d_enc packed) in float64 under ``masks``, composed as
    ``reference_full_grads``: the decoder's gradients and d_enc with the hidden rows as leaves, then d_enc through the
    encoder graph.  ``mutant`` plants one of ``DROP_MUTANTS`` (``p`` is what "scale_missing" removes)."""
    assert mutant is None or mutant in DROP_MUTANTS, mutant
    enc = DropEnc64(cfg, sd, rounding, masks, mutant, p)
    hidden = [enc.forward(s, b) for b, s in enumerate(sources)]
    loss, grads, d_enc = reference_decoder_grads_dropout(cfg, sd, [h.detach() for h in hidden], tactic_ids, masks, rounding,
                                                         mutant, p, tied=bool(cfg["tie_word_embeddings"]))
    torch.autograd.backward(hidden, [torch.from_numpy(d) for d in d_enc])
    for k, t in enc.leaves.items():
        ge = (torch.zeros_like(t) if t.grad is None else t.grad).numpy()
        grads[k] = ge + grads[k] if k == "shared.weight" else ge
    return loss, grads, np.concatenate(d_enc)


class DeviceMasks:
    """The multipliers a step of the engine used, read back with ``rp_dbg_dropout_mask`` (needs the GPU): pair b's rows
    start at src_cu[b] (encoder sites) or tgt_cu[b] (decoder sites); probabilities per head with col0 = h << 20."""

    def __init__(self, p: float, seed: int, src_cu, tgt_cu):
        self.p, self.seed, self.src_cu, self.tgt_cu = float(p), int(seed), np.asarray(src_cu), np.asarray(tgt_cu)
        self.scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))  # the engine's fp32 1 / (1 - p)

    def read(self, site, row0, col0, rows, cols) -> torch.Tensor:
        from reprover_amd import _lib

        out = torch.empty((rows, cols), dtype=torch.uint8, device="cuda:0")
        with torch.cuda.device(out.device):
            _lib.check(_lib.load().rp_dbg_dropout_mask(self.p, self.seed, site, int(row0), int(col0), rows, cols,
                                                       _lib.ptr(out), _lib.current_stream()), "rp_dbg_dropout_mask")
        return out.cpu().to(torch.float64)

    @staticmethod
    def site(half, kind, layer):
        from reprover_amd import decoder as D

        if half == "enc":
            return {"embed": D.DROP_SITE_EMBED, "final": D.DROP_SITE_FINAL}.get(kind, None) if layer is None else \
                D.DROP_SITE_LAYER0 + 8 * layer + ENC_KINDS[kind]
        return {"embed": D.DROP_SITE_DEC_EMBED, "final": D.DROP_SITE_DEC_FINAL}.get(kind, None) if layer is None else \
            D.DROP_SITE_DEC_LAYER0 + 8 * layer + DEC_KINDS[kind]

    def __call__(self, half, kind, layer, pair, shape):
        site = self.site(half, kind, layer)
        row0 = (self.src_cu if half == "enc" else self.tgt_cu)[pair]
        if len(shape) == 3:
            m = torch.stack([self.read(site, row0, h << 20, shape[1], shape[2]) for h in range(shape[0])])
        else:
            m = self.read(site, row0, 0, shape[0], shape[1])
        return m * self.scale


# ---- the attention kernels alone (tests/test_decoder_dropout_kernels_gpu.py) ------------------------------------------------
def attention_masks(c: Dict, p: float, seed: int, site: int) -> List[Optional[np.ndarray]]:
    """Per pair of case ``c`` (tests/decoder_kernel_helpers.py): the multipliers [H, Tq, Tk] the kernels used, read back at
    the pair's PACKED query rows (``c["row0"]``: first packed row per pair, default the call's own prefix sums)."""
    dm = DeviceMasks(p, seed, [0], [0])
    q_cu = np.concatenate([[0], np.cumsum([q for q, _ in c["pairs"]])])
    row0 = c.get("row0", q_cu[:-1])
    return [None if Tq == 0 else np.stack([dm.read(site, row0[b], h << 20, Tq, Tk).numpy() for h in range(c["H"])]) * dm.scale
            for b, (Tq, Tk) in enumerate(c["pairs"])]


def attention_reference_dropout(c: Dict, masks: List[Optional[np.ndarray]], rounded: bool = False) -> Dict[str, np.ndarray]:
    """``decoder_kernel_helpers.attention_reference`` with the probabilities dropped: out = (P M) V with the undropped
    normaliser and lse2; dV = (P M)^T dO, dP = M (dO V^T), dS = P (dP - delta), delta = rowsum(dO O) over the dropped O."""
    import decoder_kernel_helpers as dk

    r = dk.bf16_round if rounded else (lambda x: x)
    H, causal, nbias = c["H"], c["causal"], c["nbias"]
    T, S = c["q"].shape[0], c["k"].shape[0]
    res = dict(out=np.zeros((T, H * 64)), lse2=np.zeros((H, T)), delta=np.zeros((H, T)), dq=np.zeros((T, H * 64)),
               dk=np.zeros((S, H * 64)), dv=np.zeros((S, H * 64)))
    raw = np.zeros((H, max(nbias, 1)))
    qs = ks = 0
    for b, (Tq, Tk) in enumerate(c["pairs"]):
        for h in range(H if Tq else 0):
            cs = slice(h * 64, h * 64 + 64)
            q, d_o = c["q"][qs : qs + Tq, cs], c["d_o"][qs : qs + Tq, cs]
            k, v = c["k"][ks : ks + Tk, cs], c["v"][ks : ks + Tk, cs]
            M = masks[b][h]
            s = q @ k.T
            live = np.ones(s.shape, bool)
            if causal:
                dist = np.arange(Tq)[:, None] - np.arange(Tk)[None]
                live = dist >= 0
                idx = np.minimum(np.maximum(dist, 0), nbias - 1)
                s = s + c["tab"][h][idx]
            s = np.where(live, s, -np.inf)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(1, keepdims=True)
            p = e / l
            out = r((r(e * M) @ v) / l)
            delta = (d_o * out).sum(1)
            ds = p * (M * (d_o @ v.T) - delta[:, None])
            res["out"][qs : qs + Tq, cs] = out
            res["lse2"][h, qs : qs + Tq] = (m[:, 0] + np.log(l[:, 0])) * dk.LOG2E
            res["delta"][h, qs : qs + Tq] = delta
            res["dq"][qs : qs + Tq, cs] = r(r(ds) @ k)
            res["dk"][ks : ks + Tk, cs] = r(r(ds).T @ q)
            res["dv"][ks : ks + Tk, cs] = r(r(p * M).T @ d_o)
            if causal:
                np.add.at(raw[h], idx[live], ds[live])
        qs += Tq
        ks += Tk
    if causal:
        dtab = np.zeros((c["nbuckets"], H))
        np.add.at(dtab, c["bucket_of"], raw.T)
        res["dtab"] = dtab
    return res
