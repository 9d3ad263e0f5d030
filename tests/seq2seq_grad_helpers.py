"""Float64 reference gradients of the teacher-forced seq2seq loss for the ``rp_decoder_loss_grad`` tests: autograd through
``T5ForwardEmu`` (tests/seq2seq_helpers.py) with the encoder outputs and every decoder weight as leaves.

``rounding=False`` is HF fp32 computed in float64 (the reference); ``rounding=True`` keeps the forward's bf16 rounding
points (differentiated straight through the casts, as HF's bf16 autograd does): the baseline whose distance from the
reference sizes the tolerances (``GRAD_TOL``)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from seq2seq_helpers import T5ForwardEmu

LAYER_KEYS = {
    "ln_self": "layer.0.layer_norm.weight", "q": "layer.0.SelfAttention.q.weight", "k": "layer.0.SelfAttention.k.weight",
    "v": "layer.0.SelfAttention.v.weight", "o": "layer.0.SelfAttention.o.weight", "ln_cross": "layer.1.layer_norm.weight",
    "cq": "layer.1.EncDecAttention.q.weight", "ck": "layer.1.EncDecAttention.k.weight",
    "cv": "layer.1.EncDecAttention.v.weight", "co": "layer.1.EncDecAttention.o.weight",
    "ln_ff": "layer.2.layer_norm.weight", "wi_0": "layer.2.DenseReluDense.wi_0.weight",
    "wi_1": "layer.2.DenseReluDense.wi_1.weight", "wo": "layer.2.DenseReluDense.wo.weight",
}
REL_BIAS = "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"

# The G25 batch shapes: 129 crosses the 128-query block, 260 passes the 256-key mark and the bias clamp (max_distance
# 128), 1 and 0 are the edges; the 40-label target holds interior -100s.
G25_SRC = (1, 70, 300, 129, 64)
G25_TGT = (1, 129, 260, 0, 40)


def g25_labels(seed: int = 25) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    out = []
    for n in G25_TGT:
        y = np.concatenate([rng.integers(3, 259, size=max(n - 1, 0)), [1]])[:n].astype(np.int64)
        if n == 40:
            y[5:7] = -100
            y[20] = -100
        out.append(y)
    return out


def padded_labels(labels: List[np.ndarray]) -> np.ndarray:
    T = max(max(len(y) for y in labels), 1)
    out = np.full((len(labels), T), -100, np.int64)
    for b, y in enumerate(labels):
        out[b, : len(y)] = y
    return out


def g25_encs(cfg: Dict) -> List[torch.Tensor]:
    """The G25 encoder outputs: bf16 values from the project's Philox normals (the fixture's generator and the tests
    rebuild the same tensors, so they are not stored)."""
    from reprover_amd import synth

    D = cfg["d_model"]
    return [torch.from_numpy((synth._philox_normal(f"g25.enc.{b}", s * D, 25) * 0.5).astype(np.float32).reshape(s, D))
            .to(torch.bfloat16) for b, s in enumerate(G25_SRC)]


# Planted bugs of the gradient (not of the loss value): each is the kind of index or bookkeeping error a hand-written
# backward is prone to.  -> the tensor the bug is aimed at
GRAD_MUTANTS = {
    "bias_off_by_one": REL_BIAS,        # the table gradient lands at distance + 1
    "clamp_dropped": REL_BIAS,          # distances >= 2 * max_distance (the clamped table entry) get no gradient
    "next_source": "d_enc",             # a pair's d_enc rows are written to the next pair's source
    "tied_head_missing": "shared.weight",  # tied head: the lm_head gradient is not added into shared
    "mean_all": "decoder.final_layer_norm.weight",  # division by every label position instead of the counted ones
    "final_scale_missing": "decoder.final_layer_norm.weight",  # d_model^-0.5 left out of the final norm's backward
}


class _GradEmu(T5ForwardEmu):
    """T5ForwardEmu whose self-attention bias can route its gradient to other table entries (same values)."""

    gmutant = None

    def pair_log_probs(self, enc, tokens):
        if self.gmutant not in ("bias_off_by_one", "clamp_dropped"):
            return super().pair_log_probs(enc, tokens)
        from gen_helpers import _gelu, unidirectional_bucket

        enc = enc.to(device=self.device, dtype=self.dtype)
        T, S, H, dk = len(tokens), enc.shape[0], self.H, self.dk
        nb, md = self.cfg["relative_attention_num_buckets"], self.cfg["relative_attention_max_distance"]
        x = self.embed[torch.as_tensor(np.asarray(tokens, dtype=np.int64), device=self.device)]
        dist = np.maximum(np.arange(T)[:, None] - np.arange(T)[None], 0)
        look = lambda d: self.tab[torch.from_numpy(unidirectional_bucket(-d, nb, md))].permute(2, 0, 1)  # noqa: E731
        bias = look(dist)
        if self.gmutant == "bias_off_by_one":
            wrong = look(dist + 1)
            bias = bias.detach() + (wrong - wrong.detach())
        else:
            live = torch.from_numpy(dist < 2 * md).to(bias.dtype)
            bias = bias.detach() + live * (bias - bias.detach())
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


def reference_grads(cfg: Dict, sd: Dict[str, torch.Tensor], encs, tactic_ids, rounding: bool = False,
                    tied: bool = False, mutant: str = None) -> Tuple[float, Dict[str, np.ndarray], List[np.ndarray]]:
    """(loss, {HF name: d loss / d parameter}, [d loss / d enc_b]) in float64.  ``tied``: the head's gradient is added
    into ``shared.weight`` and no ``lm_head.weight`` entry is returned.  With no counted label: NaN loss, zero gradients.
    ``mutant`` plants one of ``GRAD_MUTANTS``."""
    from reprover_amd.decoder import shift_and_segment

    assert mutant is None or mutant in GRAD_MUTANTS, mutant
    emu = _GradEmu(cfg, sd, rounding=rounding)
    emu.gmutant = mutant
    leaves = {"shared.weight": emu.embed, "lm_head.weight": emu.lm, REL_BIAS: emu.tab,
              "decoder.final_layer_norm.weight": emu.final_ln}
    for i, l in enumerate(emu.layers):
        for fld, key in LAYER_KEYS.items():
            leaves[f"decoder.block.{i}.{key}"] = l[fld]
    for t in leaves.values():
        t.requires_grad_(True)
    encs = [None if e is None else e.detach().to(torch.float64).clone().requires_grad_(True) for e in encs]
    y = np.asarray(tactic_ids, dtype=np.int64)
    tokens, labels, cu = shift_and_segment(y)
    total, count = torch.zeros((), dtype=torch.float64), 0
    for b in range(y.shape[0]):
        n = int(cu[b + 1] - cu[b])
        if n == 0:
            continue
        lp = emu.pair_log_probs(encs[b], tokens[cu[b] : cu[b + 1]])
        lab = labels[cu[b] : cu[b + 1]].astype(np.int64)
        keep = lab >= 0
        g = lp[torch.arange(n), torch.from_numpy(np.where(keep, lab, 0))]
        total = total - g[torch.from_numpy(keep)].sum()
        count += int(keep.sum())
    if count:
        (total / (y.size if mutant == "mean_all" else count)).backward()
    grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).numpy().astype(np.float64)  # noqa: E731
    grads = {k: grad(t) for k, t in leaves.items()}
    if mutant == "final_scale_missing" and emu.out_scale != 1.0:
        # the final norm's backward without the factor: everything below the head is 1 / scale too large
        for k in grads:
            if k != "lm_head.weight":
                grads[k] = grads[k] / emu.out_scale
    if tied:
        head = grads.pop("lm_head.weight")
        if mutant != "tied_head_missing":
            grads["shared.weight"] = grads["shared.weight"] + head
    d_enc = [None if e is None else grad(e) for e in encs]
    if mutant == "final_scale_missing" and emu.out_scale != 1.0:
        d_enc = [None if e is None else e / emu.out_scale for e in d_enc]
    if mutant == "next_source":
        moved = [None if e is None else np.zeros_like(e) for e in d_enc]
        B = len(d_enc)
        for b in range(B):
            src, dst = d_enc[b], moved[(b + 1) % B]
            if src is not None and dst is not None:
                n = min(len(src), len(dst))
                dst[:n] += src[:n]
        d_enc = moved
    return (float(total.detach()) / count if count else float("nan")), grads, d_enc


def packed(d_enc) -> np.ndarray:
    return np.concatenate([e for e in d_enc if e is not None])


def rel_l2(got: np.ndarray, ref: np.ndarray) -> float:
    den = float(np.sqrt((ref.astype(np.float64) ** 2).sum()))
    return float(np.sqrt(((got.astype(np.float64) - ref) ** 2).sum())) / den if den else float(np.abs(got).max())


def rel_max(got: np.ndarray, ref: np.ndarray) -> float:
    den = float(np.abs(ref).max())
    return float(np.abs(got.astype(np.float64) - ref).max()) / den if den else float(np.abs(got).max())


G25_STRIDE = 8  # the fixture keeps every 8th element of each HF fp32 gradient (flattened), plus whole-tensor figures


def load_g25(golden_dir: str, name: str) -> Dict:
    """One configuration of tests/golden/g25_seq2seq_grad.npz (make_golden_seq2seq_grad.py): labels, HF fp32 / bf16
    losses, and per tensor (HF names + "d_enc"): the strided sample and the L2 norm / max of HF fp32's gradient, and
    HF-bf16 autograd's error against it (relative L2, max error / max)."""
    import json
    import os

    z = np.load(os.path.join(golden_dir, "g25_seq2seq_grad.npz"))
    meta = json.loads(bytes(z["meta"]).decode())[name]
    out = dict(labels=z[f"{name}_labels"].astype(np.int64), loss=z[f"{name}_loss"], tensors={})
    for i, k in enumerate(meta["tensors"]):
        n2, mx, e2, em = z[f"{name}_figures"][i]
        out["tensors"][k] = dict(sample=z[f"{name}_s{i}"], norm=float(n2), max=float(mx), bf16_l2=float(e2),
                                 bf16_max=float(em))
    return out


# rp_decoder_loss_grad against reference_grads(rounding=False) on G25, per tensor: no worse than HF-bf16 autograd's own
# error on that tensor (the fixture's figures), on both metrics.  Exceptions by name - (config, tensor) -> (relative L2
# bound, max / max bound), each 2 x the figure measured on the MI355X (in the comment), where HF-bf16's errors cancel or
# it keeps more precision than a bf16 GEMM operand can.
GRAD_TOL: Dict[Tuple[str, str], Tuple[float, float]] = {
    # max / max measured 3.852e-2 where HF-bf16 has 3.454e-2 (relative L2: 2.24e-2 against HF-bf16's 3.19e-2, kept as the
    # bound): the largest error of a 128-element norm-weight gradient is one element's; HF-bf16's happens to be smaller
    ("tiny", "decoder.block.1.layer.2.layer_norm.weight"): (3.185e-2, 7.704e-2),
}
# ByT5-small widths (no fixture: the tensors are too big to commit): at most GRAD_TOL_FACTOR times the error of the
# rounded reference (reference_grads(rounding=True): the forward's bf16 rounding points, exact backward) on the same
# tensor: the backward additionally rounds dY, dS and P to bf16 before its MFMAs.  Measured on the MI355X: relative L2
# 0.77 % - 1.64 % per tensor, each within 2 % of the rounded reference's own error.
GRAD_TOL_FACTOR = 2.0
