"""Data module for the tactic generator: the reference's ``generation/datamodule.py`` without Lightning.

``GeneratorDataset`` reads LeanDojo ``traced_tactics`` (``remove_marks`` on the tactic), optionally prepends retrieved
premises to the state (``format_augmented_state``, ``p_drop`` in training only), then removes the marks from the state.
``collate`` tokenises with ``padding="longest"``, truncates to ``max_inp_seq_len`` / ``max_oup_seq_len`` and turns pad
ids of the tactic into ``-100``.  ``preds_path`` is a ``predictions.pickle`` (the reference's, or the one
``reprover_amd.retrieval.main predict`` writes), keyed by (context path, theorem full name, state).  Tokenisation is the
package's ByT5 byte tokenizer (the reference's ``AutoTokenizer`` of a ByT5 checkpoint); any tokenizer with the same call
form can be passed in.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import Any, Dict, Iterator, List, Optional

from ..common import Corpus, format_augmented_state, remove_marks
from ..tokenizer import ByT5Tokenizer

Example = Dict[str, Any]


class GeneratorDataset:
    def __init__(self, data_path: str, corpus: Optional[Corpus], preds: Optional[Dict], max_inp_seq_len: int,
                 max_oup_seq_len: int, p_drop: float, tokenizer, is_train: bool) -> None:
        self.corpus = corpus
        self.preds = preds
        self.max_inp_seq_len = max_inp_seq_len
        self.max_oup_seq_len = max_oup_seq_len
        self.p_drop = p_drop
        self.tokenizer = tokenizer
        self.is_train = is_train
        self.data = self._load_data(data_path)

    def _load_data(self, data_path: str) -> List[Example]:
        data = []
        with open(data_path) as fh:
            theorems = json.load(fh)
        for thm in theorems:
            for tac in thm["traced_tactics"]:
                data.append({"url": thm["url"], "commit": thm["commit"], "file_path": thm["file_path"],
                             "full_name": thm["full_name"], "state": tac["state_before"],
                             "tactic": remove_marks(tac["tactic"])})
        return data

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, idx: int) -> Example:
        # (a copy: the reference rewrites the stored example, so a second access would augment an augmented state)
        ex = dict(self.data[idx])
        if self.preds is not None:
            pred = self.preds[(ex["file_path"], ex["full_name"], ex["state"])]
            ex["state"] = format_augmented_state(ex["state"], pred["retrieved_premises"], self.max_inp_seq_len,
                                                 self.p_drop if self.is_train else 0.0)
        ex["state"] = remove_marks(ex["state"])
        return ex

    def collate(self, examples: List[Example]) -> Dict[str, Any]:
        state = [ex["state"] for ex in examples]
        tok_state = self.tokenizer(state, padding="longest", max_length=self.max_inp_seq_len, truncation=True,
                                   return_tensors="pt")
        tactic = [ex["tactic"] for ex in examples]
        tok_tactic = self.tokenizer(tactic, padding="longest", max_length=self.max_oup_seq_len, truncation=True,
                                    return_tensors="pt")
        tactic_ids = tok_tactic.input_ids
        tactic_ids[tactic_ids == self.tokenizer.pad_token_id] = -100
        batch = {"state": state, "state_ids": tok_state.input_ids, "state_mask": tok_state.attention_mask,
                 "tactic": tactic, "tactic_ids": tactic_ids, "tactic_mask": tok_tactic.attention_mask}
        for k in examples[0]:
            if k not in batch:
                batch[k] = [ex[k] for ex in examples]
        return batch


def load_preds(preds_path: str) -> Dict:
    """(context path, theorem full name, state) -> prediction record of a ``predictions.pickle``.  The file is read with
    plain ``pickle.load``, as the reference reads it: a file the reference wrote needs its ``common`` module importable."""
    with open(preds_path, "rb") as fh:
        records = pickle.load(fh)
    preds = {}
    for pred in records:
        ctx = pred["context"]
        preds[ctx.path, ctx.theorem_full_name, ctx.state] = pred
    return preds


def epoch_seed(base_seed: int, epoch: int) -> int:
    """The seed of one epoch's shuffle and premise drops: the retriever's (``retrieval/main.py::_epoch_seed``)."""
    return (int(base_seed) * 1_000_003 + 7919 * int(epoch) + 12345) % (2 ** 63)


class GeneratorDataModule:
    def __init__(self, data_path: str, model_name: str, batch_size: int, eval_batch_size: int, max_inp_seq_len: int,
                 max_oup_seq_len: int, p_drop: float, num_workers: int = 0, corpus_path: Optional[str] = None,
                 preds_path: Optional[str] = None, tokenizer=None) -> None:
        self.data_path = data_path
        self.corpus = Corpus(corpus_path) if corpus_path is not None else None
        self.batch_size = batch_size
        self.eval_batch_size = eval_batch_size
        self.max_inp_seq_len = max_inp_seq_len
        self.max_oup_seq_len = max_oup_seq_len
        self.p_drop = p_drop
        self.num_workers = num_workers
        self.tokenizer = tokenizer or ByT5Tokenizer()  # ByT5's byte tokenizer: model_name needs no download
        self.preds = None if preds_path is None else load_preds(preds_path)
        self.ds_train: Optional[GeneratorDataset] = None
        self.ds_val: Optional[GeneratorDataset] = None

    def setup(self, stage: Optional[str] = None) -> None:
        args = (self.corpus, self.preds, self.max_inp_seq_len, self.max_oup_seq_len, self.p_drop, self.tokenizer)
        if stage in (None, "fit"):
            self.ds_train = GeneratorDataset(os.path.join(self.data_path, "train.json"), *args, is_train=True)
        if stage in (None, "fit", "validate"):
            self.ds_val = GeneratorDataset(os.path.join(self.data_path, "val.json"), *args, is_train=False)

    def train_dataloader(self, skip: int = 0, seed: Optional[int] = None, epoch: int = 0) -> Iterator[Dict[str, Any]]:
        """One epoch of the train split as the reference's DataLoader yields it (generation/datamodule.py:184-193:
        ``shuffle=True, drop_last=True``), examples fetched with ``is_train=True`` so that ``p_drop`` applies.  The order
        and the premise drops draw from ``random``; with ``seed`` given it is seeded first with ``epoch_seed(seed, epoch)``
        (the caller's stream is its own to restore).  ``skip``: the first ``skip`` batches are consumed at the index level,
        their examples fetched (the draws advance as in an uninterrupted epoch) but neither collated nor yielded."""
        import random

        if seed is not None:
            random.seed(epoch_seed(seed, epoch))
        ds = self.ds_train
        order = list(range(len(ds)))
        random.shuffle(order)
        for n, i in enumerate(range(0, len(order) - self.batch_size + 1, self.batch_size)):
            examples = [ds[j] for j in order[i : i + self.batch_size]]
            if n >= skip:
                yield ds.collate(examples)

    def val_dataloader(self) -> Iterator[Dict[str, Any]]:
        """Batches of ``eval_batch_size`` in order, the last one short (shuffle=False, drop_last=False)."""
        ds = self.ds_val
        for i in range(0, len(ds), self.eval_batch_size):
            yield ds.collate([ds[j] for j in range(i, min(i + self.eval_batch_size, len(ds)))])
