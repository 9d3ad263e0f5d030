"""Generate the seq2seq gradient fixture G25 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data file is committed.  Usage:
    python tests/golden/make_golden_seq2seq_grad.py

G25  autograd of T5ForConditionalGeneration(encoder_outputs, attention_mask, labels).loss in fp32 and in bf16 for the
     tiny and tiny-tied decoder configurations (synthetic weights, scale="sharp"), on the batch of
     tests/seq2seq_grad_helpers.py: B = 5 pairs, sources of 1, 70, 300, 129 and 64 rows (g25_encs, rebuilt by the tests),
     targets of 1, 129, 260, 0 and 40 labels, the last with interior -100s.  Full gradients of both precisions are about
     9 MB, so per tensor (every decoder parameter and d loss / d encoder_last_hidden_state, packed) the file keeps: every
     8th element of the fp32 gradient, its L2 norm and max, and HF-bf16's error against it (relative L2, max error / max)
     computed here over the whole tensor.  A variant with every label ignored gives HF a NaN loss and is not stored.
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
from seq2seq_grad_helpers import (G25_STRIDE, LAYER_KEYS, REL_BIAS, g25_encs, g25_labels, padded_labels, rel_l2,  # noqa: E402
                                  rel_max)

from reprover_amd import synth  # noqa: E402


def hf_grads(model, encs, y, dtype):
    from transformers.modeling_outputs import BaseModelOutput

    B, S = len(encs), max(e.shape[0] for e in encs)
    enc = torch.zeros((B, S, encs[0].shape[1]), dtype=dtype)
    mask = torch.zeros((B, S), dtype=torch.long)
    for b, e in enumerate(encs):
        enc[b, : len(e)] = e.to(dtype)
        mask[b, : len(e)] = 1
    enc.requires_grad_(True)
    model.zero_grad()
    out = model(encoder_outputs=BaseModelOutput(last_hidden_state=enc), attention_mask=mask, labels=torch.from_numpy(y))
    out.loss.backward()
    names = {"shared.weight": model.shared.weight, REL_BIAS: None, "decoder.final_layer_norm.weight": None}
    params = dict(model.named_parameters())
    g = {"shared.weight": model.shared.weight.grad}
    if model.lm_head.weight is not model.shared.weight:
        g["lm_head.weight"] = model.lm_head.weight.grad
    for k in (REL_BIAS, "decoder.final_layer_norm.weight"):
        g[k] = params[k].grad
    for i in range(model.config.num_decoder_layers):
        for key in LAYER_KEYS.values():
            g[f"decoder.block.{i}.{key}"] = params[f"decoder.block.{i}.{key}"].grad
    del names
    g["d_enc"] = torch.cat([enc.grad[b, : len(e)] for b, e in enumerate(encs)])
    return float(out.loss.float()), {k: v.detach().float().double().numpy() for k, v in g.items()}


def main():
    arrays, meta = {}, {}
    for name in ("tiny", "tiny-tied"):
        cfg = synth.seq2seq_config(name)
        sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
        encs, y = g25_encs(cfg), padded_labels(g25_labels())
        l32, g32 = hf_grads(hf_model(cfg, sd), encs, y, torch.float32)
        l16, g16 = hf_grads(hf_model(cfg, sd, torch.bfloat16), encs, y, torch.bfloat16)
        assert set(g32) == set(g16)
        tensors = sorted(g32)
        figs = []
        for i, k in enumerate(tensors):
            arrays[f"{name}_s{i}"] = g32[k].reshape(-1)[::G25_STRIDE].astype(np.float32)
            figs.append([np.sqrt((g32[k] ** 2).sum()), np.abs(g32[k]).max(), rel_l2(g16[k], g32[k]), rel_max(g16[k], g32[k])])
            print(f"g25 {name} {k}: |g| {figs[-1][0]:.3e}, HF-bf16 rel L2 {figs[-1][2]:.3e}, max/max {figs[-1][3]:.3e}")
        arrays[f"{name}_figures"] = np.array(figs, dtype=np.float64)
        arrays[f"{name}_labels"] = y.astype(np.int32)
        arrays[f"{name}_loss"] = np.array([l32, l16], dtype=np.float64)
        meta[name] = dict(config=name, scale="sharp", stride=G25_STRIDE, tensors=tensors)
        print(f"g25 {name}: loss fp32 {l32:.6f} bf16 {l16:.6f}")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g25_seq2seq_grad.npz"), **arrays)


if __name__ == "__main__":
    main()
