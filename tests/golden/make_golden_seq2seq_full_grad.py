"""Generate the whole-model seq2seq gradient fixture G26 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data file is committed.  Usage:
    python tests/golden/make_golden_seq2seq_full_grad.py

G26  autograd of T5ForConditionalGeneration(input_ids, attention_mask, labels).loss in fp32 and in bf16 for the tiny and
     tiny-tied configurations (synthetic weights, scale="hf": with the sharp family HF-bf16's own error on the encoder
     tensors is 13 - 22 % relative L2, too loose a bar), on the batch of tests/seq2seq_full_grad_helpers.py: B = 5 pairs,
     sources of 1, 70, 300, 129 and 64 byte ids (g26_sources, rebuilt by the tests), G25's labels.  Per parameter the
     file keeps, in G25's form: a strided sample of the fp32 gradient (every 8th element of shared.weight and the
     encoder's tensors, every 32nd of the decoder's, which G25 pins at stride 8), its L2 norm and max, and HF-bf16's error
     against it (relative L2, max error / max) over the whole tensor; and both losses.
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

from make_golden_generate import hf_model  # noqa: E402
from seq2seq_full_grad_helpers import g26_sources, g26_stride, padded_sources  # noqa: E402
from seq2seq_grad_helpers import g25_labels, padded_labels, rel_l2, rel_max  # noqa: E402

from reprover_amd import synth  # noqa: E402


def hf_grads(model, ids, mask, y):
    model.zero_grad()
    out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(y))
    out.loss.backward()
    g = {k: p.grad.detach().float().double().numpy() for k, p in model.named_parameters()}
    return float(out.loss.float()), g


def main():
    arrays, meta = {}, {}
    for name in ("tiny", "tiny-tied"):
        cfg = synth.seq2seq_config(name)
        sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
        (ids, mask), y = padded_sources(g26_sources()), padded_labels(g25_labels())
        l32, g32 = hf_grads(hf_model(cfg, sd), ids, mask, y)
        l16, g16 = hf_grads(hf_model(cfg, sd, torch.bfloat16), ids, mask, y)
        assert set(g32) == set(g16)
        want = {k for k in sd if "embed_tokens" not in k}
        assert set(g32) == want, set(g32) ^ want
        tensors = sorted(g32)
        figs = []
        for i, k in enumerate(tensors):
            arrays[f"{name}_s{i}"] = g32[k].reshape(-1)[:: g26_stride(k)].astype(np.float32)
            figs.append([np.sqrt((g32[k] ** 2).sum()), np.abs(g32[k]).max(), rel_l2(g16[k], g32[k]), rel_max(g16[k], g32[k])])
            print(f"g26 {name} {k}: |g| {figs[-1][0]:.3e}, HF-bf16 rel L2 {figs[-1][2]:.3e}, max/max {figs[-1][3]:.3e}")
        arrays[f"{name}_figures"] = np.array(figs, dtype=np.float64)
        arrays[f"{name}_labels"] = y.astype(np.int32)
        arrays[f"{name}_loss"] = np.array([l32, l16], dtype=np.float64)
        meta[name] = dict(config=name, scale="hf", tensors=tensors)
        print(f"g26 {name}: loss fp32 {l32:.6f} bf16 {l16:.6f}")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g26_seq2seq_full_grad.npz"), **arrays)


if __name__ == "__main__":
    main()
