"""Generate the tactic-prefix fixture G27 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data file is committed.  Usage:
    python tests/golden/make_golden_prefix.py

G27  generate(input_ids, decoder_input_ids=[0] + prefix, num_beams, num_return_sequences=num_beams, length_penalty,
     max_length, early_stopping=False, do_sample=False) in fp32 and bf16 on the G20 weights and the G20 source, over
     P = len(prefix) in {1, 5, 17} x num_beams in {2, 4, 8} x length_penalty in {0, 1, -0.5} x max_length in
     {P + 2, P + 6, P + 20} (81 cases), plus greedy (num_beams=1) cases at P in {1, 5}.  Stored per case: HF's fp32
     sequences (they hold the prompt) and sequences_scores, whether HF-bf16 returns the same sequences, the prefix, and the
     per-step top-2nb candidates of the fp32 driver (generation.beam_search over gen_helpers.T5Fp32 with
     prefill_by_steps), which is asserted equal to HF while generating.
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

from make_golden_generate import G20_EOS_BOOST, G20_SOURCE_BYTES, g20_weights, hf_model, source_ids  # noqa: E402

G27_PREFIX_TEXT = "simp only [foo] at h"  # its first P bytes are the prefix (ByT5 ids: byte + 3, no EOS)
G27_GRID = [(P, nb, lp, P + extra) for P in (1, 5, 17) for nb in (2, 4, 8) for lp in (0.0, 1.0, -0.5)
            for extra in (2, 6, 20)]
G27_GREEDY = [(P, 1, 0.0, P + extra) for P in (1, 5) for extra in (6, 20)]
G27_MIN_FLAGGED, G27_MIN_EOS_ROWS = 24, 8


def g27():
    from gen_helpers import T5Fp32
    from reprover_amd.generation import beam_search, greedy_search

    cfg, sd = g20_weights()
    m32, m16 = hf_model(cfg, sd), hf_model(cfg, sd, torch.bfloat16)
    src, _ = source_ids(G20_SOURCE_BYTES, 20)
    inp = torch.from_numpy(src)[None]
    arrays = {"src": src.astype(np.int32)}
    meta = []
    ref = T5Fp32(cfg, sd)
    enc = ref.encode(src)
    text = G27_PREFIX_TEXT.encode("utf-8")
    for ci, (P, nb, lp, ml) in enumerate(G27_GRID + G27_GREEDY):
        prefix = [b + 3 for b in text[:P]]
        assert len(prefix) == P
        dec = torch.tensor([[0] + prefix], dtype=torch.long)
        kw = dict(decoder_input_ids=dec, num_beams=nb, num_return_sequences=nb, length_penalty=lp, max_length=ml,
                  early_stopping=False, do_sample=False, return_dict_in_generate=True, output_scores=True)
        with torch.no_grad():
            o32 = m32.generate(inp, **kw)
            o16 = m16.generate(inp, **kw)
        s32 = o32.sequences.numpy()
        assert (s32[:, : P + 1] == np.array([0] + prefix)).all()
        sc32 = o32.sequences_scores.numpy() if nb > 1 else np.zeros(1, np.float32)
        agree = s32.shape == o16.sequences.shape and bool((o16.sequences.numpy() == s32).all())
        arrays[f"c{ci}_prefix"] = np.array(prefix, dtype=np.int32)
        arrays[f"c{ci}_seq"] = s32.astype(np.int32)
        arrays[f"c{ci}_score"] = sc32.astype(np.float32)
        ref.start(enc, nb, ml)
        steps = 0
        if nb > 1:
            trace = []
            mine = beam_search(ref.step, nb, ml, lp, trace=trace, prompt=prefix)
            assert mine.sequences.shape == s32.shape and (mine.sequences.numpy() == s32).all(), (ci, mine.sequences, s32)
            assert np.allclose(mine.sequences_scores.numpy(), sc32, rtol=1e-5, atol=1e-5), (ci, mine.sequences_scores, sc32)
            arrays[f"c{ci}_trace_score"] = np.stack([t[0].numpy() for t in trace]).astype(np.float32)
            arrays[f"c{ci}_trace_token"] = np.stack([t[1].numpy() for t in trace]).astype(np.int16)
            arrays[f"c{ci}_trace_parent"] = np.stack([t[2].numpy() for t in trace]).astype(np.int16)
            steps = len(trace)
        else:
            mine = greedy_search(ref.step, ml, prompt=prefix)
            assert mine.sequences.shape == s32.shape and (mine.sequences.numpy() == s32).all(), (ci, mine.sequences, s32)
        n_eos = int((s32[:, P + 1 :] == 1).any(1).sum())
        meta.append(dict(prefix_len=P, num_beams=nb, length_penalty=lp, max_length=ml, bf16_agrees=agree, steps=steps,
                         n_finished_on_eos=n_eos))
        print(f"g27 case {ci}: P={P} nb={nb} lp={lp} max_length={ml} -> {s32.shape}, eos-finished {n_eos}, "
              f"bf16 agrees {agree}")
    beam = meta[: len(G27_GRID)]
    flagged, eos_rows = sum(c["bf16_agrees"] for c in beam), sum(c["n_finished_on_eos"] for c in beam)
    print(f"g27: {flagged} of {len(beam)} beam cases flagged bf16_agrees, {eos_rows} rows finished on EOS")
    assert flagged >= G27_MIN_FLAGGED and eos_rows >= G27_MIN_EOS_ROWS, (flagged, eos_rows)
    arrays["meta"] = np.frombuffer(json.dumps(dict(cases=meta, n_beam_cases=len(G27_GRID), eos_boost=G20_EOS_BOOST,
                                                   source_bytes=G20_SOURCE_BYTES, prefix_text=G27_PREFIX_TEXT)).encode(),
                                   dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g27_generate_prefix.npz"), **arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    g27()
