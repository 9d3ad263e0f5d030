"""The float64 reference of the tactic generator's training step (``HipSeq2SeqTrainer``): the
whole-model gradient of tests/seq2seq_full_grad_helpers.py stepped by oracle/train_ref.py's AdamW.  ``shared.weight`` is
updated once, with the summed gradient (the encoder's embedding part + the decoder's, which holds the tied head's).

The parameters are stored in fp32 between steps, as the engine's masters are (``train_ref.adamw_step``); the arithmetic of a
step and both moments are float64.  Hyper-parameters are used as given: a caller comparing with the GPU passes the values
a C float of the ABI receives (``f32``)."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import train_ref
from seq2seq_full_grad_helpers import reference_full_grads

ALIASES = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight")
# Planted bug of the step -> the tensor it is aimed at
STEP_MUTANTS = {
    # each half updates its own copy of the embedding with its own part of the gradient and its own moments, one after
    # the other: two AdamW updates of shared.weight per step
    "shared_twice": "shared.weight",
}


def f32(x) -> float:
    """The value a C float parameter of the ABI receives."""
    return float(np.float32(x))


def parameter_names(cfg: Dict, sd: Dict[str, torch.Tensor]) -> List[str]:
    """Every parameter of the HF model once: no embed_tokens alias, no lm_head when it is tied to shared."""
    tied = bool(cfg["tie_word_embeddings"])
    return [k for k in sd if "embed_tokens" not in k and not (tied and k == "lm_head.weight")]


def with_aliases(cfg: Dict, params: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}
    for a in ALIASES:
        sd[a] = sd["shared.weight"]
    return sd


class RefTrainer64:
    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], lr: float, warmup_steps: int = 0, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, rounding: bool = False, mutant: Optional[str] = None):
        assert mutant is None or mutant in STEP_MUTANTS, mutant
        self.cfg, self.rounding, self.mutant = cfg, rounding, mutant
        self.lr, self.warmup_steps, self.betas, self.eps, self.weight_decay = lr, warmup_steps, betas, eps, weight_decay
        self.p = {k: sd[k].detach().numpy().astype(np.float32).copy() for k in parameter_names(cfg, sd)}
        self.m = {k: np.zeros(v.shape) for k, v in self.p.items()}
        self.v = {k: np.zeros(v.shape) for k, v in self.p.items()}
        self.m2, self.v2 = np.zeros(self.p["shared.weight"].shape), np.zeros(self.p["shared.weight"].shape)  # shared_twice
        self.t = 0

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return with_aliases(self.cfg, self.p)

    def gradients(self, sources, y, rounding: Optional[bool] = None):
        """(loss, {name: float64 gradient}) at the current parameters"""
        loss, grads, _ = reference_full_grads(self.cfg, self.state_dict(), sources, y,
                                              rounding=self.rounding if rounding is None else rounding)
        return loss, grads

    def apply(self, grads: Dict[str, np.ndarray], split_shared=None) -> None:
        """One AdamW update of every parameter from ``grads``.  ``split_shared`` = (encoder part, decoder part) of
        shared.weight's gradient for the shared_twice mutant."""
        lr = self.lr * train_ref.warmup_factor(self.t, self.warmup_steps)
        self.t += 1
        hyper = (self.t, lr, self.betas, self.eps, self.weight_decay)
        for k in self.p:
            if k == "shared.weight" and self.mutant == "shared_twice":
                ge, gd = split_shared
                self.p[k], self.m[k], self.v[k] = train_ref.adamw_step(self.p[k], ge, self.m[k], self.v[k], *hyper)
                self.p[k], self.m2, self.v2 = train_ref.adamw_step(self.p[k], gd, self.m2, self.v2, *hyper)
            else:
                self.p[k], self.m[k], self.v[k] = train_ref.adamw_step(self.p[k], grads[k], self.m[k], self.v[k], *hyper)

    def step(self, sources, y) -> float:
        loss, grads = self.gradients(sources, y)
        split = None
        if self.mutant == "shared_twice":
            _, gdec, _ = reference_full_grads(self.cfg, self.state_dict(), sources, y, rounding=self.rounding,
                                              mutant="embed_not_added")  # shared.weight = the decoder's part alone
            split = (grads["shared.weight"] - gdec["shared.weight"], gdec["shared.weight"])
        self.apply(grads, split)
        return loss
