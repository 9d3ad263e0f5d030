"""Generate the teacher-forced seq2seq fixture G22 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data files are committed.  Usage:
    python tests/golden/make_golden_seq2seq.py [g22 g23]   (default: both)

G22  T5ForConditionalGeneration(input_ids, attention_mask, labels) in fp32 and bf16 on padded batches, for tiny and
     ByT5-small at HF init scales and tiny at scale="sharp" (synth.synth_seq2seq_state_dict).  Batch "mix" holds a 1-byte
     source and sources of 300, 2047 and 2300 bytes; targets of 1 token (EOS only), typical lengths and 512; a row with
     interior -100 labels; an all-ignored row.  Batch "none" has only ignored labels (NaN loss).  Stored per model and
     batch: the padded inputs, .loss (fp32; bf16 from the bf16 logits in fp32), the per-token label log-probs (0 where
     ignored) and full rows at a few positions.
G23  the reference's own GeneratorDataset (generation/datamodule.py through ref_harness, a transformers ByT5Tokenizer
     passed in) over a synth.synth_split theorem file, without and with a preds dict (g23_preds below): the collate
     output (strings and ids) of the whole split, and the augmented states of p_drop = 0 (validation) and of a seeded
     p_drop = 0.5 training item.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_generate import hf_model, source_ids  # noqa: E402

from reprover_amd import synth  # noqa: E402

OUT = HERE
MIX = [  # (source bytes, target: number of labels incl. the final EOS | "interior" | "ignored")
    (1, 1), (300, 41), (2047, 512), (2300, "interior"), (300, "ignored"), (80, 64),
]
ROWS = ((1, (0, 5, 40)), (2, (0, 255, 511)))  # (batch row, positions) whose full fp32 rows are stored
MODELS = {"tiny": ("tiny", "hf"), "byt5-small": ("byt5-small", "hf"), "tiny-sharp": ("tiny", "sharp")}


def padded_batch(spec, seed):
    rng = np.random.default_rng(seed)
    srcs, labs = [], []
    for j, (n_src, tgt) in enumerate(spec):
        srcs.append(source_ids(n_src, 220 + 7 * j + seed)[0] if n_src > 1 else np.array([1], dtype=np.int64))
        if tgt == "interior":
            y = np.concatenate([rng.integers(3, 259, size=29), [1]])
            y[5:7] = -100
        elif tgt == "ignored":
            y = np.full(12, -100)
        else:
            y = np.concatenate([rng.integers(3, 259, size=tgt - 1), [1]])
        labs.append(y.astype(np.int64))
    S, T = max(map(len, srcs)), max(map(len, labs))
    ids = np.zeros((len(spec), S), np.int64)
    mask = np.zeros((len(spec), S), np.int64)
    y = np.full((len(spec), T), -100, np.int64)
    for b, (s, l) in enumerate(zip(srcs, labs)):
        ids[b, : len(s)] = s
        mask[b, : len(s)] = 1
        y[b, : len(l)] = l
    return ids, mask, y


def label_lp(model, ids, mask, y):
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(y))
    lp = torch.log_softmax(out.logits.float(), -1)
    keep = torch.from_numpy(y != -100)
    lab = torch.from_numpy(np.where(y == -100, 0, y))
    per = torch.where(keep, lp.gather(-1, lab[..., None])[..., 0], torch.zeros(()))
    n = int(keep.sum())
    loss = float(-per.sum() / n) if n else float("nan")
    return per.numpy().astype(np.float32), loss, float(out.loss.float()), lp


def g22_model(name, arrays, meta):
    cname, scale = MODELS[name]
    cfg = synth.seq2seq_config(cname)
    sd = synth.synth_seq2seq_state_dict(cfg, scale=scale)
    m32, m16 = hf_model(cfg, sd), hf_model(cfg, sd, torch.bfloat16)
    for batch, spec in (("mix", MIX), ("none", [(40, "ignored"), (7, "ignored")])):
        ids, mask, y = padded_batch(spec, 22)
        p32, l32, hf32, lp = label_lp(m32, ids, mask, y)
        p16, l16, _, _ = label_lp(m16, ids, mask, y)
        assert (np.isnan(l32) and np.isnan(hf32)) or abs(l32 - hf32) <= 1e-5 * max(1.0, abs(l32)), (l32, hf32)
        key = f"{name}_{batch}"
        arrays[f"{key}_ids"] = ids.astype(np.int32)
        arrays[f"{key}_mask"] = mask.astype(np.int8)
        arrays[f"{key}_labels"] = y.astype(np.int32)
        arrays[f"{key}_lp32"] = p32
        arrays[f"{key}_lp16"] = p16
        arrays[f"{key}_loss"] = np.array([l32, l16], dtype=np.float64)
        if batch == "mix":
            for b, pos in ROWS:
                arrays[f"{key}_rows{b}"] = lp[b, list(pos)].numpy().astype(np.float32)
        meta[key] = dict(config=cname, scale=scale, positions=[list(p) for _, p in ROWS])
        print(f"g22 {key}: loss fp32 {l32:.6f} bf16 {l16:.6f}, max |lp bf16 - fp32| {float(np.abs(p16 - p32).max()):.3e}")


G23_MAX_INP, G23_MAX_OUP, G23_SEED = 700, 40, 23


def g23():
    import random
    import tempfile

    import ref_harness as H
    from transformers import ByT5Tokenizer

    H.install()
    H._mod("tqdm", tqdm=lambda x, **k: x)
    from generation.datamodule import GeneratorDataset

    tok = ByT5Tokenizer()
    from seq2seq_helpers import g23_inputs

    path, preds = g23_inputs(tempfile.mkdtemp())
    out = {}
    for tag, pr in (("plain", None), ("preds", preds)):
        ds = GeneratorDataset(path, None, pr, G23_MAX_INP, G23_MAX_OUP, 0.5, tok, is_train=False)
        batch = ds.collate([ds[i] for i in range(len(ds))])
        out[tag] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in batch.items()}
    train = GeneratorDataset(path, None, preds, G23_MAX_INP, G23_MAX_OUP, 0.5, tok, is_train=True)
    random.seed(G23_SEED)
    out["train_p_drop"] = [train[i]["state"] for i in range(3)]
    out["config"] = dict(max_inp_seq_len=G23_MAX_INP, max_oup_seq_len=G23_MAX_OUP, p_drop=0.5, seed=G23_SEED)
    with open(os.path.join(OUT, "g23_generator_data.json"), "w") as fh:
        json.dump(out, fh, ensure_ascii=False)
    print("g23:", len(out["plain"]["state"]), "examples")


def main():
    which = sys.argv[1:] or ["g22", "g23"]
    if "g22" in which:
        arrays, meta = {}, {}
        for name in MODELS:
            g22_model(name, arrays, meta)
        arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(OUT, "g22_seq2seq.npz"), **arrays)
    if "g23" in which:
        g23()


if __name__ == "__main__":
    main()
