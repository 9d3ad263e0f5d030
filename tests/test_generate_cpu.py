"""Tactic generator, host side: unidirectional buckets and ByT5 decode (G18), and the beam-search driver against
HuggingFace generate (G20) through the fp32 CPU restatement of the T5 decoder (tests/gen_helpers.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, unidirectional_bucket  # noqa: E402
from reprover_amd import synth, tokenizer  # noqa: E402
from reprover_amd.generation import beam_search  # noqa: E402


def test_unidirectional_bucket_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g18_buckets_causal.npz"))
    assert np.array_equal(unidirectional_bucket(g["rel"], 32, 128), g["bucket"])


def test_unidirectional_bucket_library_golden(golden_dir):
    from reprover_amd import _lib

    lib = _lib.load()
    g = np.load(os.path.join(golden_dir, "g18_buckets_causal.npz"))
    mine = np.array([lib.rp_relative_position_bucket_causal(int(r), 32, 128) for r in g["rel"]])
    assert np.array_equal(mine, g["bucket"])


def test_batch_decode_golden(golden_dir):
    with open(os.path.join(golden_dir, "g18_decode.json")) as fh:
        g = json.load(fh)
    assert tokenizer.batch_decode(g["ids"], skip_special_tokens=True) == g["text"]
    tok = tokenizer.ByT5Tokenizer()
    assert [tok.decode(torch.tensor(i, dtype=torch.long)) for i in g["ids"]] == g["text"]


def _g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def _g20_model(meta):
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    return cfg, sd


@pytest.fixture(scope="module")
def g20_setup(golden_dir):
    z, meta = _g20(golden_dir)
    cfg, sd = _g20_model(meta)
    ref = T5Fp32(cfg, sd)
    return z, meta, ref, ref.encode(z["src"])


@pytest.mark.parametrize("case", range(24))
def test_beam_search_matches_hf_generate(g20_setup, case):
    z, meta, ref, enc = g20_setup
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    ref.start(enc, nb, ml)
    trace = []
    out = beam_search(ref.step, nb, ml, lp, trace=trace)
    assert len(trace) == c["steps"]
    assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
    if nb > 1:  # HF's num_beams=1 is greedy search: no sequences_scores
        np.testing.assert_allclose(out.sequences_scores.numpy(), z[f"c{case}_score"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(np.stack([t[1].numpy() for t in trace]), z[f"c{case}_trace_token"])
    assert np.array_equal(np.stack([t[2].numpy() for t in trace]), z[f"c{case}_trace_parent"])


def test_g20_grid_covers_eos_and_cap(golden_dir):
    _, meta = _g20(golden_dir)
    cases = meta["cases"]
    assert {c["num_beams"] for c in cases} == {1, 4, 8, 64}
    assert {c["length_penalty"] for c in cases} == {0.0, 1.0, -0.5}
    assert any(c["n_finished_on_eos"] for c in cases) and any(c["steps"] == c["max_length"] - 1 for c in cases)


def test_beam_search_rejects_max_length_one():
    with pytest.raises(ValueError):
        beam_search(lambda t, a: torch.zeros(len(t), 384), 4, 1)


def test_seq2seq_synth_keeps_encoder_bytes():
    cfg = synth.seq2seq_config("tiny")
    enc = synth.synth_state_dict(synth.t5_config("tiny"), scale="hf")
    s2s = synth.synth_seq2seq_state_dict(cfg)
    for k, v in enc.items():
        assert torch.equal(s2s[k], v), k
    assert s2s["decoder.block.1.layer.1.EncDecAttention.k.weight"].shape == (128, 128)
    assert "lm_head.weight" in s2s and "lm_head.weight" not in synth.synth_seq2seq_state_dict(synth.seq2seq_config("tiny-tied"))
