"""The teacher-forced seq2seq path on the host: label shifting and segmentation (HF ``_shift_right``), the mask check,
the float64 reference (tests/seq2seq_helpers.py) against HF fp32 (G22), how far planted reference bugs move the loss
and log-probs, and the greedy driver against HF greedy generate (G22)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32  # noqa: E402
from seq2seq_helpers import FORWARD_TOL, MUTANTS, T5ForwardEmu  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.decoder import shift_and_segment, source_lengths  # noqa: E402
from reprover_amd.generation import greedy_search  # noqa: E402

G22 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_seq2seq.npz")
MODELS = {"tiny": ("tiny", "hf"), "tiny-sharp": ("tiny", "sharp")}


def _hf_shift_right(labels, start=0, pad=0):
    """modeling_t5.py T5PreTrainedModel._shift_right"""
    shifted = labels.new_zeros(labels.shape)
    shifted[..., 1:] = labels[..., :-1].clone()
    shifted[..., 0] = start
    return shifted.masked_fill(shifted == -100, pad)


def test_shift_and_segment_match_hf_shift_right():
    y = torch.tensor([[5, 6, 1, -100, -100], [-100, -100, -100, -100, -100], [7, -100, -100, 9, 1], [1, -100, 3, -100, -100],
                      [4, 4, 4, 4, 1]])
    tokens, labels, cu = shift_and_segment(y)
    assert cu.tolist() == [0, 3, 3, 8, 11, 16]
    ref = _hf_shift_right(y)
    for b in range(y.shape[0]):
        n = cu[b + 1] - cu[b]
        assert tokens[cu[b] : cu[b + 1]].tolist() == ref[b, :n].tolist()
        assert labels[cu[b] : cu[b + 1]].tolist() == y[b, :n].tolist()
    # the interior -100 is fed as token 0 and stays an ignored label inside the segment
    assert tokens[cu[2] + 2] == 0 and labels[cu[2] + 1] == -100
    with pytest.raises(ValueError):
        shift_and_segment(np.array([[3, -5, 1]]))


def test_source_lengths_accept_right_padding_only():
    assert source_lengths(np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]])).tolist() == [2, 1, 3]
    for bad in ([[0, 1, 1]], [[1, 0, 1]], [[1, 2, 0]]):
        with pytest.raises(ValueError):
            source_lengths(np.array(bad))
    with pytest.raises(ValueError):
        source_lengths(np.array([1, 1]))


def _g22(name, batch="mix"):
    z = np.load(G22)
    k = f"{name}_{batch}"
    return (z[f"{k}_ids"].astype(np.int64), z[f"{k}_mask"].astype(np.int64), z[f"{k}_labels"].astype(np.int64),
            z[f"{k}_lp32"], z[f"{k}_lp16"], z[f"{k}_loss"], z)


def _encs(cfg, sd, ids, mask):
    ref = T5Fp32(cfg, sd)
    n = source_lengths(mask)
    return [ref.encode(ids[b, : n[b]]) if n[b] else None for b in range(len(n))]


@pytest.mark.parametrize("name", list(MODELS))
def test_reference_without_rounding_matches_hf_fp32(name):
    cname, scale = MODELS[name]
    cfg = synth.seq2seq_config(cname)
    sd = synth.synth_seq2seq_state_dict(cfg, scale=scale)
    ids, mask, y, lp32, _, loss, z = _g22(name)
    emu = T5ForwardEmu(cfg, sd, rounding=False)
    got_loss, got, rows = emu.forward(_encs(cfg, sd, ids, mask), y, rows=True)
    d = np.abs(got.numpy() - lp32)
    print(f"{name}: max |d lp| {d.max():.2e}, |d loss| {abs(got_loss - loss[0]):.2e}")
    assert d.max() < 2e-4 and abs(got_loss - loss[0]) < 2e-5 * max(1.0, abs(loss[0]))
    for b, pos in ((1, (0, 5, 40)), (2, (0, 255, 511))):
        assert np.abs(rows[b][list(pos)].numpy() - z[f"{name}_mix_rows{b}"]).max() < 2e-4
    nan_loss, nan_lp = emu.forward(_encs(cfg, sd, *_g22(name, "none")[:2]), _g22(name, "none")[2])
    assert np.isnan(nan_loss) and np.isnan(_g22(name, "none")[5][0]) and not nan_lp.abs().sum()


def test_planted_bugs_move_loss_or_log_probs():
    """Each planted bug moves the label log-probs (or, for the counting bugs, the loss) well beyond the GPU tolerance."""
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    ids, mask, y, *_ = _g22("tiny-sharp")
    encs = [e.to(torch.bfloat16) if e is not None else None for e in _encs(cfg, sd, ids, mask)]
    clean_loss, clean = T5ForwardEmu(cfg, sd).forward(encs, y)
    tol_max, tol_rms = FORWARD_TOL["tiny-sharp"]
    for m in MUTANTS:
        loss, lp = T5ForwardEmu(cfg, sd, mutant=m).forward(encs, y)
        d_lp = float((lp - clean).abs().max())
        d_loss = abs(loss - clean_loss)
        print(f"{m}: max |d lp| {d_lp:.3f} (tolerance {tol_max}), |d loss| {d_loss:.3f} (loss tolerance {tol_rms})")
        if m in ("count_ignored", "mean_all"):
            assert d_loss > 10 * tol_rms, m
        else:
            assert d_lp > 4 * tol_max, m


def test_greedy_driver_reproduces_g20_one_beam_points():
    """HF's generate(num_beams=1) is greedy search; G20's nb=1 grid points are its outputs."""
    z = np.load(os.path.join(os.path.dirname(G22), "g20_generate.npz"))
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= 1.6  # make_golden_generate.G20_EOS_BOOST
    ref = T5Fp32(cfg, sd)
    enc = ref.encode(z["src"])
    for c, ml in enumerate((6, 20, 6, 20, 6, 20)):  # G20_GRID's nb = 1 points: length penalties 0, 1, -0.5
        ref.start(enc, 1, ml)
        got = greedy_search(ref.step, ml).sequences[0].numpy()
        assert got.tolist() == z[f"c{c}_seq"][0].tolist(), c


def _toy_step(table):
    """A model whose log-probs depend only on the position: table [positions, V] of logits."""
    def step(tokens, ancestry):
        return torch.log_softmax(torch.as_tensor(table[ancestry.shape[1] - 1], dtype=torch.float32), -1)[None]
    return step


def test_greedy_search_stops_at_eos_and_breaks_ties_low():
    V, eos = 6, 1
    flat = np.zeros((8, V))
    flat[0, [3, 4]] = 2.0  # a tie: the lower id wins
    flat[1, eos] = 1.0
    flat[1, 5] = 0.999
    g = greedy_search(_toy_step(flat), 8, eos_token_id=eos)
    assert g.sequences[0].tolist() == [0, 3, eos]
    lp = torch.log_softmax(torch.tensor(flat[:2], dtype=torch.float32), -1)
    assert abs(float(g.sequences_scores[0]) - float(lp[0, 3] + lp[1, eos])) < 1e-6
    no_eos = np.zeros((8, V))
    no_eos[:, 2] = 1.0
    assert greedy_search(_toy_step(no_eos), 5, eos_token_id=eos).sequences[0].tolist() == [0, 2, 2, 2, 2]


def test_generator_dataset_and_collate_match_reference_g23(tmp_path):
    """The reference's GeneratorDataset / collate (G23) without and with retrieval predictions, and a seeded p_drop = 0.5
    training item."""
    import json
    import random

    from seq2seq_helpers import g23_inputs
    from reprover_amd.generator.datamodule import GeneratorDataset

    g = json.load(open(os.path.join(os.path.dirname(G22), "g23_generator_data.json"), encoding="utf-8"))
    c = g["config"]
    path, preds = g23_inputs(str(tmp_path))
    for tag, pr in (("plain", None), ("preds", preds)):
        ds = GeneratorDataset(path, None, pr, c["max_inp_seq_len"], c["max_oup_seq_len"], c["p_drop"], _tokenizer(),
                              is_train=False)
        batch = ds.collate([ds[i] for i in range(len(ds))])
        for k, v in g[tag].items():
            got = batch[k].tolist() if hasattr(batch[k], "tolist") else batch[k]
            assert got == v, (tag, k)
    train = GeneratorDataset(path, None, preds, c["max_inp_seq_len"], c["max_oup_seq_len"], c["p_drop"], _tokenizer(),
                             is_train=True)
    random.seed(c["seed"])
    assert [train[i]["state"] for i in range(3)] == g["train_p_drop"]
    assert g["train_p_drop"][0] != g["preds"]["state"][0]  # the seeded draw dropped premises


def _tokenizer():
    from reprover_amd.tokenizer import ByT5Tokenizer

    return ByT5Tokenizer()


def test_topk_accuracy_semantics():
    from reprover_amd.generator.model import TopkAccuracy

    preds = [["rw [h]", "<a>simp</a>", "exact h"], ["intro x", "ring", "linarith"], ["norm_num", "omega", "simp"]]
    gt = ["simp", "linarith", "<a>norm_num</a>"]  # marks removed on both sides
    got = []
    for k in (1, 2, 3):
        acc = TopkAccuracy(k)
        acc.update(preds[:2], gt[:2])
        acc.update(preds[2:], gt[2:])
        got.append((acc.correct, acc.total, acc.compute()))
    assert got == [(1, 3, 1 / 3), (2, 3, 2 / 3), (3, 3, 1.0)]
    assert np.isnan(TopkAccuracy(1).compute())


def test_generator_fit_exits_with_a_message():
    from reprover_amd.generator import main as gmain

    with pytest.raises(SystemExit, match="decoder backward"):
        gmain.main(["fit", "--config", "unused.yaml"])
