"""Generate fixture G24 (the sampler's kept sets) with HuggingFace transformers' logits warpers on CPU.

Authoring container only; only the resulting data file is committed.  Usage:
    python tests/golden/make_golden_sample.py

G24  For vocab 3 / 384 / 512: float32 log-softmax rows (seeded random rows of mixed sharpness, then rows of small
     integers, i.e. with many exact ties) and, for every point of the grid temperature {0.7, 1, 1.5} x top_k {0, 1, 5,
     vocab} x top_p {1, 0.9, 0.1}, the tokens that TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper
     leave finite (bit-packed masks).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

HERE = os.path.dirname(os.path.abspath(__file__))
VOCABS = (3, 384, 512)
RANDOM_ROWS, TIED_ROWS = 24, 8


def rows(vocab: int, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    x = g.standard_normal((RANDOM_ROWS + TIED_ROWS, vocab)) * g.choice([0.5, 2.0, 6.0], size=(RANDOM_ROWS + TIED_ROWS, 1))
    x[RANDOM_ROWS:] = np.round(x[RANDOM_ROWS:])
    return torch.log_softmax(torch.from_numpy(x.astype(np.float32)), -1).numpy()


def main() -> None:
    out, grid = {}, []
    for vocab in VOCABS:
        lp = rows(vocab, 2400 + vocab)
        out[f"v{vocab}_lp"] = lp
        masks = []
        for T in (0.7, 1.0, 1.5):
            for k in (0, 1, 5, vocab):
                for p in (1.0, 0.9, 0.1):
                    s = torch.from_numpy(lp.copy())
                    if T != 1.0:
                        s = TemperatureLogitsWarper(T)(None, s)
                    if k:
                        s = TopKLogitsWarper(k)(None, s)
                    if p < 1.0:
                        s = TopPLogitsWarper(p)(None, s)
                    masks.append(torch.isfinite(s).numpy())
                    if vocab == VOCABS[0]:
                        grid.append([T, 0 if k == 0 else ("vocab" if k == vocab else k), p])
        out[f"v{vocab}_kept"] = np.packbits(np.stack(masks), axis=-1)
    import transformers

    out["meta"] = np.frombuffer(json.dumps({"grid": grid, "vocabs": list(VOCABS), "random_rows": RANDOM_ROWS,
                                            "tied_rows": TIED_ROWS, "transformers": transformers.__version__}).encode(),
                                dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g24_sample_warp.npz"), **out)


if __name__ == "__main__":
    main()
