"""``RetrievalAugmentedGenerator`` and ``TopkAccuracy``: the reference's ``generation/model.py`` without Lightning, on the
HIP engine (``HipT5Generator``).  ``forward`` is the teacher-forced loss (``rp_decoder_forward``); ``validation_step``
computes what the reference logs, ``loss_val`` and ``top{k}_acc_val`` for k = 1..num_beams, and accumulates the epoch
values (``epoch_metrics``: the loss as the mean over batches weighted by batch size, the accuracies over all states).

Generation follows the reference's call: ``max_length=max_oup_seq_len``, ``num_return_sequences=num_beams``,
``early_stopping=False`` and no ``length_penalty`` argument, so HF's default 1.0 applies (not ``self.length_penalty``).
With ``num_beams == 1`` HF runs greedy search, and so does this (``HipT5Generator.greedy_many``).  A validation batch is one
batched call (``generate_many``: one decode loop for all its states, the bits of one state at a time).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

from ..common import remove_marks
from ..tokenizer import ByT5Tokenizer, batch_decode


class TopkAccuracy:
    """generation/model.py:25-46: a state counts when its ground-truth tactic (marks removed) is among the first k
    predictions (marks removed)."""

    def __init__(self, k: int) -> None:
        self.k = k
        self.correct = 0
        self.total = 0

    def update(self, batch_preds: List[List[str]], batch_gt: List[str]) -> None:
        assert len(batch_preds) == len(batch_gt)
        for preds, gt in zip(batch_preds, batch_gt):
            gt = remove_marks(gt)
            preds = [remove_marks(p) for p in preds]
            self.correct += gt in preds[: self.k]
        self.total += len(batch_gt)

    def compute(self) -> float:
        return float(self.correct) / self.total if self.total else float("nan")

    def reset(self) -> None:
        self.correct = self.total = 0


class RetrievalAugmentedGenerator:
    def __init__(self, model_name: str, lr: float, warmup_steps: int, num_beams: int, eval_num_retrieved: int,
                 eval_num_workers: int, eval_num_gpus: int, eval_num_theorems: int, max_inp_seq_len: int,
                 max_oup_seq_len: int, length_penalty: float = 0.0, ret_ckpt_path: Optional[str] = None,
                 device="cuda:0", dropout_rate: float = 0.0, dropout_seed: Optional[int] = None) -> None:
        from ..decoder import HipT5Generator

        self.lr, self.warmup_steps = lr, warmup_steps
        # T5's dropout of the TRAINING step (the reference's checkpoints carry dropout_rate 0.1); generation and validation
        # never drop
        self.dropout_rate, self.dropout_seed = float(dropout_rate), dropout_seed
        self.num_beams = num_beams
        self.length_penalty = length_penalty
        self.eval_num_retrieved, self.eval_num_workers = eval_num_retrieved, eval_num_workers
        self.eval_num_gpus, self.eval_num_theorems = eval_num_gpus, eval_num_theorems
        self.max_inp_seq_len, self.max_oup_seq_len = max_inp_seq_len, max_oup_seq_len
        self.ret_ckpt_path = ret_ckpt_path  # (the retriever only serves Pass@1 through the prover: not run here)
        self.tokenizer = ByT5Tokenizer()
        self.model_name, self.device = model_name, device
        self.train_engine = None  # HipSeq2SeqTrainer, once configure_optimizers has run
        self.generator = HipT5Generator.from_pretrained(model_name, device)
        self.topk_accuracies = {k: TopkAccuracy(k) for k in range(1, num_beams + 1)}
        self._loss_sum, self._loss_n = 0.0, 0

    def forward(self, state_ids, state_mask, tactic_ids) -> float:
        return self.generator.forward(state_ids, state_mask, tactic_ids)

    def configure_optimizers(self, weight_decay: float = 1e-2, gradient_clip_val: Optional[float] = None):
        """generation/model.py:134-146 (``get_optimizers``: AdamW under a constant schedule after ``warmup_steps``): builds
        the ``HipSeq2SeqTrainer`` from the checkpoint with this model's ``lr`` and ``warmup_steps`` and re-points
        ``self.generator`` at its inference view; the inference-only copies made by the constructor are released.
        ``weight_decay``: 1e-2 is ``torch.optim.AdamW``'s default."""
        from ..decoder import load_seq2seq_checkpoint
        from ..seq2seq_train import HipSeq2SeqTrainer

        cfg, sd = load_seq2seq_checkpoint(self.model_name)
        self.generator = None  # (released before the training buffers are taken)
        self.train_engine = HipSeq2SeqTrainer(cfg, sd, self.device, lr=self.lr, warmup_steps=self.warmup_steps,
                                              weight_decay=weight_decay, gradient_clip_val=gradient_clip_val,
                                              dropout_rate=self.dropout_rate, dropout_seed=self.dropout_seed)
        self.generator = self.train_engine.generator()
        return self.train_engine

    def training_step(self, batch: Dict[str, Any], batch_idx: int = 0) -> float:
        """generation/model.py:117-132: the loss of the batch (``loss_train``), and here also the update it leads to (the
        optimizer and the scheduler are the engine's: gradients, AdamW, re-packing of the compute copies)."""
        if self.train_engine is None:
            raise RuntimeError("training_step needs configure_optimizers() first")
        loss, _ = self.train_engine.loss_and_grads(batch["state_ids"], batch["state_mask"], batch["tactic_ids"])
        self.train_engine.optimizer_step()
        return float(loss)

    def generate_batch(self, state_ids, state_mask) -> List[List[str]]:
        """num_beams decoded candidates per state (skip_special_tokens=True)."""
        ids = np.asarray(state_ids.cpu() if hasattr(state_ids, "cpu") else state_ids)
        n = np.asarray(state_mask.cpu() if hasattr(state_mask, "cpu") else state_mask).sum(1)
        srcs = [ids[b, : int(n[b])] for b in range(ids.shape[0])]
        out: List[List[str]] = []
        cap = self.generator.decoder.max_states(self.num_beams)  # the engine's cap on states per call
        for i in range(0, len(srcs), cap):
            chunk = srcs[i : i + cap]
            if self.num_beams == 1:
                res = self.generator.greedy_many(chunk, self.max_oup_seq_len)
            else:
                res = self.generator.generate_many(chunk, self.num_beams, self.max_oup_seq_len, length_penalty=1.0)
            out.extend(batch_decode(r.sequences.tolist(), skip_special_tokens=True) for r in res)
        return out

    def validation_step(self, batch: Dict[str, Any], _=None) -> Dict[str, float]:
        loss = self.forward(batch["state_ids"], batch["state_mask"], batch["tactic_ids"])
        bs = int(batch["state_ids"].shape[0])
        self._loss_sum += loss * bs
        self._loss_n += bs
        preds = self.generate_batch(batch["state_ids"], batch["state_mask"])
        logs = {"loss_val": loss}
        for k, acc in self.topk_accuracies.items():
            batch_acc = TopkAccuracy(k)
            batch_acc.update(preds, batch["tactic"])
            acc.update(preds, batch["tactic"])
            logs[f"top{k}_acc_val"] = batch_acc.compute()
        self.last_preds = preds
        return logs

    def epoch_metrics(self) -> Dict[str, float]:
        out = {"loss_val": self._loss_sum / self._loss_n if self._loss_n else float("nan")}
        for k, acc in self.topk_accuracies.items():
            out[f"top{k}_acc_val"] = acc.compute()
        return out
