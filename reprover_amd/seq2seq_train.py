"""The tactic generator's training step on libreprover_hip.

Reference: ``generation/model.py:117-146`` (``training_step`` / ``configure_optimizers``) differentiated by autograd through
``T5ForConditionalGeneration`` and stepped by ``common.py::get_optimizers`` (AdamW under a constant schedule after a linear
warm-up).  Here ``HipSeq2SeqTrainer`` is ``HipSeq2SeqGradients`` (the loss and every gradient, section 13) plus the optimizer
end: the encoder's masters, gradients and moments live in its ``HipT5Trainer`` (flat, ``rp_train_param_layout``), the
decoder's in four flat buffers of ``rp_decoder_grad_layout``'s form owned here.  ``shared.weight`` has one master, one
gradient and one pair of moments: the trainer's ``embed`` slot.  The decoder's ``shared`` slot receives a copy of the updated
master and carries no optimizer state.  After the update both halves re-pack their compute copies
(``rp_trainer_load_params`` / ``rp_decoder_load_params``).  ``dropout_rate > 0`` is T5's training mode (DESIGN.md section
15): one seed per step drives both halves' masks; the seed base and the number of forwards taken travel with the training
state, so a resumed run draws the masks the uninterrupted run would.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .decoder import (HipSeq2SeqGradients, HipT5Decoder, HipT5Generator, decoder_grad_names, decoder_grad_shapes,
                      lm_head_source)
from .encoder import _require_gpu
from .train import HipT5Trainer

ALIASES = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight")  # HF's other names of shared.weight


def decoder_param_layout(cfg: Dict, tied: bool) -> Tuple[List[str], List[Tuple[int, ...]], np.ndarray]:
    """(names, shapes, element offsets [n + 1]) of the decoder's flat layout as ``rp_decoder_grad_layout`` reports it for a
    created decoder: every tensor starts at a multiple of 64 elements.  Needs no decoder (the masters are laid out before
    the decoder is created from them; the constructor checks the two against each other)."""
    names = decoder_grad_names(cfg, tied)
    shapes = [decoder_grad_shapes(cfg)[n] for n in names]
    off = np.zeros(len(names) + 1, dtype=np.int64)
    for i, sh in enumerate(shapes):
        off[i + 1] = off[i] + (int(np.prod(sh)) + 63) // 64 * 64
    return names, shapes, off


def hf_seq2seq_config(cfg: Dict) -> Dict:
    """``config.json`` of a T5ForConditionalGeneration with this geometry (what ``load_seq2seq_checkpoint`` and
    ``transformers`` read)."""
    tied = bool(cfg.get("tie_word_embeddings", False))
    return dict(
        model_type="t5", architectures=["T5ForConditionalGeneration"], is_encoder_decoder=True,
        vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], num_heads=cfg["num_heads"],
        d_ff=cfg["d_ff"], num_layers=cfg["num_layers"], num_decoder_layers=cfg.get("num_decoder_layers") or cfg["num_layers"],
        relative_attention_num_buckets=cfg.get("relative_attention_num_buckets", 32),
        relative_attention_max_distance=cfg.get("relative_attention_max_distance", 128),
        layer_norm_epsilon=float(cfg.get("layer_norm_epsilon", 1e-6)),
        feed_forward_proj=cfg.get("feed_forward_proj", "gated-gelu"), dropout_rate=cfg.get("dropout_rate", 0.1),
        tie_word_embeddings=tied, scale_decoder_outputs=bool(cfg.get("scale_decoder_outputs", tied)),
        decoder_start_token_id=cfg.get("decoder_start_token_id", 0), eos_token_id=cfg.get("eos_token_id", 1),
        pad_token_id=cfg.get("pad_token_id", 0))


def write_seq2seq_checkpoint(path: str, cfg: Dict, sd: Dict[str, torch.Tensor]) -> None:
    """``<path>/config.json`` + ``<path>/model.safetensors`` of a T5ForConditionalGeneration state dict (any device; written
    as fp32).  Every key of ``sd`` is stored, aliases of ``shared.weight`` included, each as a tensor of its own."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(hf_seq2seq_config(cfg), fh, indent=1)
    save_file({k: v.detach().to(torch.float32).cpu().contiguous().clone() for k, v in sd.items()},
              os.path.join(path, "model.safetensors"), metadata={"format": "pt"})


class HipSeq2SeqTrainer(HipSeq2SeqGradients):
    """Masters, gradients and AdamW moments of a whole T5ForConditionalGeneration on one GPU; ``loss_and_grads`` is
    ``HipSeq2SeqGradients``' (the same calls in the same order, the same bits), ``optimizer_step`` the update."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device, lr: float = 0.0, warmup_steps: int = 0,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 gradient_clip_val: Optional[float] = None, dropout_rate: float = 0.0, dropout_seed: Optional[int] = None):
        self.cfg = dict(cfg)
        self.device = _require_gpu(device)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.gradient_clip_val = gradient_clip_val
        head, scaled = lm_head_source(cfg, sd)
        self.tied = bool(scaled)  # the decoder's notion: the scaled head reads shared.weight and has no slot of its own
        if self.tied and head != "shared.weight" and not torch.equal(sd[head].cpu(), sd["shared.weight"].cpu()):
            raise ValueError("the checkpoint scales the decoder output as a tied head does, but its lm_head.weight differs "
                             "from shared.weight: such a model cannot be trained with one embedding master")
        enc_sd = {k: v for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
        self.trainer = HipT5Trainer(cfg, enc_sd, self.device, lr=lr, warmup_steps=warmup_steps, betas=betas, eps=eps,
                                    weight_decay=weight_decay, gradient_clip_val=gradient_clip_val, dropout_rate=dropout_rate,
                                    dropout_seed=dropout_seed)
        names, shapes, off = decoder_param_layout(cfg, self.tied)
        self.dec_names, self.dec_shapes, self.dec_off = names, shapes, off
        total, self._opt0 = int(off[-1]), int(off[1])  # the optimizer runs over [off[1], total): everything but shared
        with torch.cuda.device(self.device):
            self.dec_params = torch.zeros(total, dtype=torch.float32, device=self.device)
            for n, sh, o in zip(names, shapes, off):
                src = sd[head if n == "lm_head.weight" else n].detach()
                assert tuple(src.shape) == tuple(sh), (n, tuple(src.shape), sh)
                self.dec_params[int(o) : int(o) + src.numel()] = src.reshape(-1).to(device=self.device, dtype=torch.float32)
            self.dec_grads = torch.zeros(total, dtype=torch.float32, device=self.device)
            self.dec_exp_avg = torch.zeros(total - self._opt0, dtype=torch.float32, device=self.device)
            self.dec_exp_avg_sq = torch.zeros_like(self.dec_exp_avg)
            self._norm_dec = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        # the decoder is created from views of the master buffer: create and reload read the same floats
        view = dict(self._dec_views(self.dec_params))
        if self.tied:
            view["lm_head.weight"] = view["shared.weight"]
        self.decoder = HipT5Decoder(cfg, view, self.device)
        got_names, got_off = self.decoder.grad_layout()
        if got_names != names or not np.array_equal(got_off, off):
            raise _lib.HipLibraryError("the decoder's flat layout differs from decoder_param_layout's")
        self.last_d_enc: Optional[torch.Tensor] = None

    # -- views -------------------------------------------------------------------------------------------------------------
    def _dec_views(self, flat: torch.Tensor) -> Iterator[Tuple[str, torch.Tensor]]:
        for n, sh, o in zip(self.dec_names, self.dec_shapes, self.dec_off):
            yield n, flat[int(o) : int(o) + int(np.prod(sh))].view(*sh)

    def named_parameters(self) -> Iterator[Tuple[str, torch.Tensor]]:
        """(HF name, fp32 view of its master) of every parameter once: ``shared.weight`` is the trainer's."""
        yield from self.trainer.named_parameters()
        for n, v in self._dec_views(self.dec_params):
            if n != "shared.weight":
                yield n, v

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Host fp32 copies under HF's names and shapes, with the aliases HF writes for ``shared.weight``."""
        sd = {k: v.detach().cpu().clone() for k, v in self.named_parameters()}
        for a in ALIASES:
            sd[a] = sd["shared.weight"]
        if self.tied:
            sd["lm_head.weight"] = sd["shared.weight"]
        return sd

    @property
    def steps(self) -> int:
        return self.trainer.steps

    # -- the step ----------------------------------------------------------------------------------------------------------
    def optimizer_step(self) -> None:
        """One AdamW update of every parameter from the gradients of the last ``loss_and_grads`` and a refresh of every
        compute copy; launches on the current stream only.  Consumes the gradients: the decoder's ``shared`` gradient is
        added into the trainer's embedding gradient in place."""
        tr, lib = self.trainer, self.trainer._lib
        lr = tr.current_lr()
        tr.steps += 1
        e0, VD = int(tr.layout[0][2]), self.cfg["vocab_size"] * self.cfg["d_model"]
        n_enc, n_dec, o = tr.params.numel(), self.dec_params.numel() - self._opt0, self._opt0 * 4
        clip = self.gradient_clip_val is not None and self.gradient_clip_val > 0
        with torch.cuda.device(self.device):
            s = _lib.current_stream()
            tr.grads[e0 : e0 + VD].add_(self.dec_grads[:VD])  # encoder part + decoder part (which holds the tied head's)
            if clip:  # one global norm; shared is counted once, in the encoder buffer
                _lib.check(lib.rp_grad_norm(_lib.ptr(tr.grads), n_enc, _lib.ptr(tr.grad_norm), _lib.ptr(tr._norm_scratch), s),
                           "rp_grad_norm")
                _lib.check(lib.rp_grad_norm(self.dec_grads.data_ptr() + o, n_dec, _lib.ptr(self._norm_dec),
                                            _lib.ptr(tr._norm_scratch), s), "rp_grad_norm")
                torch.hypot(tr.grad_norm, self._norm_dec, out=self.grad_norm)
            norm = _lib.ptr(self.grad_norm) if clip else None
            hyper = (tr.steps, lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, norm,
                     float(self.gradient_clip_val or 0.0), s)
            _lib.check(lib.rp_adamw_step_clipped(_lib.ptr(tr.params), _lib.ptr(tr.grads), _lib.ptr(tr.exp_avg),
                                                 _lib.ptr(tr.exp_avg_sq), n_enc, *hyper), "rp_adamw_step_clipped")
            _lib.check(lib.rp_adamw_step_clipped(self.dec_params.data_ptr() + o, self.dec_grads.data_ptr() + o,
                                                 _lib.ptr(self.dec_exp_avg), _lib.ptr(self.dec_exp_avg_sq), n_dec, *hyper),
                       "rp_adamw_step_clipped")
            self.dec_params[:VD].copy_(tr.params[e0 : e0 + VD])
        self.load_params()

    def load_params(self) -> None:
        """Re-pack both halves' compute copies from the masters."""
        self.trainer.load_params()
        self.decoder.load_params(self.dec_params)

    # -- checkpoints -------------------------------------------------------------------------------------------------------
    def save_pretrained(self, path: str) -> None:
        """A HuggingFace checkpoint directory of the current masters (``load_seq2seq_checkpoint``,
        ``HipT5Generator.from_pretrained`` and ``transformers`` read it)."""
        write_seq2seq_checkpoint(path, self.cfg, self.state_dict())

    def save_training_state(self, path: str) -> None:
        """Everything a resumed run needs, in directory ``path``: ``encoder_state.safetensors`` (``HipT5Trainer``'s:
        masters, moments, the step counter, the dropout seed base and the number of forwards drawn from it) and
        ``decoder_state.safetensors`` (the decoder's masters and moments)."""
        from safetensors.torch import save_file

        os.makedirs(path, exist_ok=True)
        self.trainer.save_training_state(os.path.join(path, "encoder_state.safetensors"))
        save_file({"params": self.dec_params.cpu(), "exp_avg": self.dec_exp_avg.cpu(), "exp_avg_sq": self.dec_exp_avg_sq.cpu(),
                   "steps": torch.tensor([self.trainer.steps], dtype=torch.int64)},
                  os.path.join(path, "decoder_state.safetensors"))

    def load_training_state(self, path: str) -> None:
        from safetensors.torch import load_file

        dpath = os.path.join(path, "decoder_state.safetensors")
        st = load_file(dpath)
        for key, mine in (("params", self.dec_params), ("exp_avg", self.dec_exp_avg), ("exp_avg_sq", self.dec_exp_avg_sq)):
            if key not in st or st[key].numel() != mine.numel():
                raise ValueError(f"{dpath}: '{key}' has {st[key].numel() if key in st else 'no'} elements, this decoder's flat "
                                 f"layout has {mine.numel()} (the state belongs to another geometry)")
        self.trainer.load_training_state(os.path.join(path, "encoder_state.safetensors"))
        if int(st["steps"][0]) != self.trainer.steps:
            raise ValueError(f"{path}: the two halves were saved at different steps ({self.trainer.steps}, {int(st['steps'][0])})")
        self.dec_params.copy_(st["params"])
        self.dec_exp_avg.copy_(st["exp_avg"])
        self.dec_exp_avg_sq.copy_(st["exp_avg_sq"])
        self.load_params()

    def generator(self) -> HipT5Generator:
        """The inference view of this model: the trainer's encoder engine and this decoder, both refreshed by
        ``optimizer_step``.  No second copy of any weight."""
        return HipT5Generator.from_parts(self.cfg, self.trainer.encoder, self.decoder, self.device)
