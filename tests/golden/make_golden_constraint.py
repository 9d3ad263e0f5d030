"""Generate the constrained-decoding fixture G30 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data file is committed.  Usage:
    python tests/golden/make_golden_constraint.py

G30  generate(input_ids, prefix_allowed_tokens_fn=fn, num_beams, num_return_sequences=num_beams, length_penalty,
     max_length, early_stopping=False, do_sample=False) in fp32 and bf16 on the G20 weights and the G20 source, fn walking
     a reprover_amd.constraint.ByteAutomaton, over automaton in {utf8, utf8 & ban(G30_BANNED)} x num_beams in
     {1 (greedy), 2, 4, 8} x length_penalty in {0, 1, -0.5} x max_length in {6, 24} (48 cases), plus cases whose decoder
     prompt ends inside the 3-byte character of G30_PREFIX_TEXT.  Stored per case: HF's fp32 sequences and
     sequences_scores, whether HF-bf16 returns the same sequences, the prefix, and (beams) the per-step top-2nb candidates
     of the fp32 driver (generation.beam_search / greedy_search over gen_helpers.T5Fp32 with the host mask).  Asserted
     while generating: the driver equals HF (sequences exactly, scores to 1e-5); every step of every case has at least
     2 * num_beams finite candidates (torch.topk orders dead -inf ties in an unspecified way: the inputs keep them out of
     the comparison); the unconstrained HF output of every case violates the automaton.
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

# "sorry", and two byte strings the unconstrained HF output on these weights contains (ids 72 4 and 58 58)
G30_BANNED = [b"sorry", b"E\x01", b"77"]
G30_AUTOMATA = ("utf8", "utf8_ban")
G30_GRID = [(a, nb, lp, ml) for a in G30_AUTOMATA for nb in (1, 2, 4, 8) for lp in (0.0, 1.0, -0.5) for ml in (6, 24)]
G30_PREFIX_TEXT = "rw [←"  # "←" is E2 86 90: a prefix cut after E2 or after E2 86 ends inside it
# (automaton, bytes of the text kept, num_beams, length_penalty, tokens generated at most)
G30_PREFIXED = [("utf8", 5, 1, 0.0, 8), ("utf8", 5, 4, 1.0, 8), ("utf8", 6, 2, 0.0, 5), ("utf8_ban", 6, 4, -0.5, 12),
                ("utf8_ban", 5, 8, 1.0, 8)]
G30_MIN_FLAGGED, G30_MIN_EOS_ROWS = 40, 26  # what HF gives on these weights (of 53 cases; rows over all cases)


def automaton(name: str, vocab: int):
    from reprover_amd.constraint import ByteAutomaton

    u = ByteAutomaton.utf8(vocab)
    return u if name == "utf8" else u & ByteAutomaton.ban(G30_BANNED, vocab)


def g30():
    from constraint_helpers import obeys
    from gen_helpers import T5Fp32
    from reprover_amd.generation import beam_search, constraint_mask_host, greedy_search

    cfg, sd = g20_weights()
    m32, m16 = hf_model(cfg, sd), hf_model(cfg, sd, torch.bfloat16)
    src, _ = source_ids(G20_SOURCE_BYTES, 20)
    inp = torch.from_numpy(src)[None]
    arrays = {"src": src.astype(np.int32)}
    meta = []
    free_rows = []  # every unconstrained HF row, as a string of ids: G30_BANNED's two byte strings must occur in them
    ref = T5Fp32(cfg, sd)
    enc = ref.encode(src)
    auts = {name: automaton(name, cfg["vocab_size"]) for name in G30_AUTOMATA}
    text = G30_PREFIX_TEXT.encode("utf-8")
    cases = [(a, 0, nb, lp, ml) for a, nb, lp, ml in G30_GRID] + [(a, P, nb, lp, 1 + P + g) for a, P, nb, lp, g in G30_PREFIXED]
    for ci, (name, P, nb, lp, ml) in enumerate(cases):
        aut = auts[name]
        prefix = [b + 3 for b in text[:P]]
        kw = dict(num_beams=nb, num_return_sequences=nb, length_penalty=lp, max_length=ml, early_stopping=False,
                  do_sample=False, return_dict_in_generate=True, output_scores=True)
        if P:
            kw["decoder_input_ids"] = torch.tensor([[0] + prefix], dtype=torch.long)
        fn = aut.prefix_allowed_tokens_fn()
        with torch.no_grad():
            free = m32.generate(inp, **kw)
            o32 = m32.generate(inp, prefix_allowed_tokens_fn=fn, **kw)
            o16 = m16.generate(inp, prefix_allowed_tokens_fn=fn, **kw)
        s32 = o32.sequences.numpy()
        free_rows.extend("," + ",".join(str(int(t)) for t in row) + "," for row in free.sequences.numpy())
        assert not all(obeys(aut, row) for row in free.sequences.numpy()), (ci, "the constraint has no effect", free.sequences)
        assert all(obeys(aut, row) for row in s32), (ci, s32)
        sc32 = o32.sequences_scores.numpy() if nb > 1 else np.zeros(1, np.float32)
        agree = s32.shape == o16.sequences.shape and bool((o16.sequences.numpy() == s32).all())
        arrays[f"c{ci}_prefix"] = np.array(prefix, dtype=np.int32)
        arrays[f"c{ci}_seq"] = s32.astype(np.int32)
        arrays[f"c{ci}_score"] = sc32.astype(np.float32)
        ref.start(enc, nb, ml)
        least = [10 ** 9]

        def mask(lp_rows, q_rows, aut=aut, least=least):
            out = constraint_mask_host(lp_rows, q_rows, aut)
            least[0] = min(least[0], int(torch.isfinite(out).sum(1).min()))
            return out

        steps = 0
        if nb > 1:
            trace = []
            mine = beam_search(ref.step, nb, ml, lp, trace=trace, prompt=prefix or None, constraint=aut, mask=mask)
            assert mine.sequences.shape == s32.shape and (mine.sequences.numpy() == s32).all(), (ci, mine.sequences, s32)
            assert np.allclose(mine.sequences_scores.numpy(), sc32, rtol=1e-5, atol=1e-5), (ci, mine.sequences_scores, sc32)
            assert all(bool(torch.isfinite(t[0]).all()) for t in trace), (ci, "fewer than 2 nb finite candidates")
            arrays[f"c{ci}_trace_score"] = np.stack([t[0].numpy() for t in trace]).astype(np.float32)
            arrays[f"c{ci}_trace_token"] = np.stack([t[1].numpy() for t in trace]).astype(np.int16)
            arrays[f"c{ci}_trace_parent"] = np.stack([t[2].numpy() for t in trace]).astype(np.int16)
            steps = len(trace)
        else:
            mine = greedy_search(ref.step, ml, prompt=prefix or None, constraint=aut, mask=mask)
            assert mine.sequences.shape == s32.shape and (mine.sequences.numpy() == s32).all(), (ci, mine.sequences, s32)
            assert least[0] >= 2, (ci, least)
        n_eos = int((s32[:, P + 1 :] == 1).any(1).sum())
        meta.append(dict(automaton=name, prefix_len=P, num_beams=nb, length_penalty=lp, max_length=ml, bf16_agrees=agree,
                         steps=steps, n_finished_on_eos=n_eos))
        print(f"g30 case {ci}: {name} P={P} nb={nb} lp={lp} max_length={ml} -> {s32.shape}, eos-finished {n_eos}, "
              f"bf16 agrees {agree}, least allowed per row {least[0]}")
    for banned in G30_BANNED[1:]:
        ids = "," + ",".join(str(b + 3) for b in banned) + ","
        assert any(ids in row for row in free_rows), (banned, "no unconstrained HF output contains it")
    flagged, eos_rows = sum(c["bf16_agrees"] for c in meta), sum(c["n_finished_on_eos"] for c in meta)
    print(f"g30: {flagged} of {len(meta)} cases flagged bf16_agrees, {eos_rows} rows finished on EOS")
    assert flagged >= G30_MIN_FLAGGED and eos_rows >= G30_MIN_EOS_ROWS, (flagged, eos_rows)
    arrays["meta"] = np.frombuffer(json.dumps(dict(
        cases=meta, n_grid_cases=len(G30_GRID), eos_boost=G20_EOS_BOOST, source_bytes=G20_SOURCE_BYTES,
        prefix_text=G30_PREFIX_TEXT, banned=[list(b) for b in G30_BANNED])).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g30_generate_constrained.npz"), **arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    g30()
