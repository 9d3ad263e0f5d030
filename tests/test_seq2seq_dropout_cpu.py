"""T5's dropout on the seq2seq training path without a GPU: the float64 reference under given masks
(tests/seq2seq_dropout_helpers.py) is ``reference_full_grads`` at all-ones masks, is HF's train mode given the same masks
(the site list and the placement against the normaliser are HF's), and the GPU tests' bar separates planted bugs of the
dropout path; the command line, the training state's seed stream and the site constants."""
import functools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seq2seq_dropout_helpers import (DEC_KINDS, DROP_MUTANTS, ENC_KINDS, RandomMasks, ones_masks,  # noqa: E402
                                     reference_full_grads_dropout)
from seq2seq_full_grad_helpers import g26_sources, padded_sources, reference_full_grads  # noqa: E402
from seq2seq_grad_helpers import GRAD_TOL_FACTOR, g25_labels, padded_labels, rel_l2, rel_max  # noqa: E402
from reprover_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0.1
HF_FP32_REL = 2.2e-5  # tests/test_seq2seq_grad_cpu.py's bound on the reference against HF fp32, of each tensor's largest


def _model(name):
    cfg = synth.seq2seq_config(name)
    return cfg, synth.synth_seq2seq_state_dict(cfg, scale="hf")


def _y():
    return padded_labels(g25_labels())


@functools.lru_cache(maxsize=None)
def _refs(name, seed=5):
    """(unrounded, rounded) reference of the G26 batch under one set of Bernoulli(0.9) / 0.9 masks, d_enc as a tensor"""
    cfg, sd = _model(name)
    masks = RandomMasks(P, seed)
    out = []
    for rounding in (False, True):
        loss, g, d_enc = reference_full_grads_dropout(cfg, sd, g26_sources(), _y(), masks, rounding=rounding)
        out.append((loss, dict(g, d_enc=d_enc)))
    return masks, out[0], out[1]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_all_ones_masks_give_reference_full_grads(name, rounding):
    cfg, sd = _model(name)
    loss0, g0, d0 = reference_full_grads(cfg, sd, g26_sources(), _y(), rounding=rounding)
    loss1, g1, d1 = reference_full_grads_dropout(cfg, sd, g26_sources(), _y(), ones_masks, rounding=rounding)
    assert abs(loss1 - loss0) <= 1e-12 * abs(loss0) and set(g0) == set(g1)
    for k in g0:
        assert np.abs(g1[k] - g0[k]).max() <= 1e-12 * np.abs(g0[k]).max(), k
    assert np.abs(d1 - d0).max() <= 1e-12 * np.abs(d0).max()


def test_masks_move_the_loss_and_every_gradient():
    _, (loss, g), _ = _refs("tiny")
    cfg, sd = _model("tiny")
    loss0, g0, _ = reference_full_grads(cfg, sd, g26_sources(), _y())
    assert abs(loss - loss0) > 1e-3 * abs(loss0)
    assert all(rel_l2(g[k], g0[k]) > 1e-2 for k in g0)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_reference_equals_hf_train_mode_given_the_same_masks(name, tmp_path, monkeypatch):
    """HF's T5ForConditionalGeneration in train() mode, fp32, eager attention (so that nn.functional.dropout is called on
    the attention weights), on the G26 batch; torch.nn.functional.dropout is replaced by a multiplication with the test's
    own masks in HF's call order.  Loss and every gradient match the float64 reference under the same masks within
    HF_FP32_REL of each tensor's largest: the sites, their order and the placement against the softmax normaliser are HF's."""
    transformers = pytest.importorskip("transformers")
    from reprover_amd.decoder import shift_and_segment
    from reprover_amd.seq2seq_train import ALIASES, write_seq2seq_checkpoint

    cfg, sd = _model(name)
    masks, (ref_loss, gref), _ = _refs(name)
    full = dict(sd)
    for a in ALIASES:
        full[a] = full["shared.weight"]
    if cfg["tie_word_embeddings"]:
        full["lm_head.weight"] = full["shared.weight"]
    write_seq2seq_checkpoint(str(tmp_path / "ckpt"), cfg, full)
    model = transformers.T5ForConditionalGeneration.from_pretrained(str(tmp_path / "ckpt"), attn_implementation="eager",
                                                                    torch_dtype=torch.float32)
    model.train()
    assert model.config.dropout_rate == 0.1
    srcs, y = g26_sources(), _y()
    ids, amask = padded_sources(srcs)
    _, _, tgt_cu = shift_and_segment(y)
    B, S, T = len(srcs), ids.shape[1], y.shape[1]
    slen, tlen = [len(s) for s in srcs], np.diff(tgt_cu)
    H, Dm, F = cfg["num_heads"], cfg["d_model"], cfg["d_ff"]

    def batch(half, kind, layer):
        rows, n = (S, slen) if half == "enc" else (T, tlen)
        if "probs" in kind:
            keys, k = (S, slen) if (half == "enc" or kind == "cross_probs") else (T, tlen)
            m = torch.ones(B, H, rows, keys, dtype=torch.float64)
            for b in range(B):
                if n[b]:
                    m[b, :, : n[b], : k[b]] = masks(half, kind, layer, b, (H, int(n[b]), int(k[b])))
            return m
        width = F if kind == "ff_inner" else Dm
        m = torch.ones(B, rows, width, dtype=torch.float64)
        for b in range(B):
            if n[b]:
                m[b, : n[b]] = masks(half, kind, layer, b, (int(n[b]), width))
        return m

    order = []
    for half, kinds, L in (("enc", ENC_KINDS, cfg["num_layers"]), ("dec", DEC_KINDS, cfg["num_decoder_layers"])):
        order.append((half, "embed", None))
        order += [(half, kind, i) for i in range(L) for kind in sorted(kinds, key=kinds.get)]
        order.append((half, "final", None))
    calls = []

    def fake_dropout(x, p=0.5, training=True, inplace=False):
        assert training and abs(p - P) < 1e-12
        site = order[len(calls)]
        calls.append(site)
        m = batch(*site)
        assert tuple(m.shape) == tuple(x.shape), (site, tuple(m.shape), tuple(x.shape))
        return x * m.to(x.dtype)

    monkeypatch.setattr(torch.nn.functional, "dropout", fake_dropout)
    out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(amask), labels=torch.from_numpy(y))
    out.loss.backward()
    assert calls == order
    assert abs(float(out.loss.detach()) - ref_loss) <= HF_FP32_REL * abs(ref_loss)
    hf = {k: p.grad.double().numpy() for k, p in model.named_parameters()}
    worst = 0.0
    for k, g in gref.items():
        if k == "d_enc":
            continue
        e = np.abs(hf[k] - g).max() / np.abs(g).max()
        worst = max(worst, e)
        assert e <= HF_FP32_REL, (k, e)
    print(f"{name}: reference vs HF train mode under the same masks, worst max error / max {worst:.2e}")


# ---- planted bugs ----------------------------------------------------------------------------------------------------------------
def _over_bar(got, ref, base):
    """per tensor: (relative L2, max / max) of ``got`` against the unrounded reference, each over the GPU tests' bar
    (GRAD_TOL_FACTOR x the rounded reference's own error under the same masks)"""
    return {k: (rel_l2(got[k], ref[k]) / (GRAD_TOL_FACTOR * rel_l2(base[k], ref[k])),
                rel_max(got[k], ref[k]) / (GRAD_TOL_FACTOR * rel_max(base[k], ref[k]))) for k in ref}


def test_the_unmutated_stand_in_meets_the_gpu_bar():
    _, (_, ref), (_, base) = _refs("tiny")
    assert all(max(v) <= 1.0 / GRAD_TOL_FACTOR + 1e-12 for v in _over_bar(base, ref, base).values())


@pytest.mark.parametrize("mutant", sorted(DROP_MUTANTS))
def test_the_gpu_bar_separates_planted_bugs(mutant):
    """The rounded reference stands in for the engine (as in tests/test_decoder_kernels_cpu.py).  Each planted bug of the
    dropout path misses the GPU tests' bar on the tensor it is aimed at, on both metrics, by at least 4 x (measured: 5.0 x
    (scale_missing, relative L2) to 13.5 x (cross_reads_self); no mutant stays below the bar, so none is asserted at a floor)."""
    cfg, sd = _model("tiny")
    masks, (_, ref), (_, base) = _refs("tiny")
    _, g, d_enc = reference_full_grads_dropout(cfg, sd, g26_sources(), _y(), masks, rounding=True, mutant=mutant, p=P)
    over = _over_bar(dict(g, d_enc=d_enc), ref, base)
    e2, em = over[DROP_MUTANTS[mutant]]
    print(f"{mutant}: {DROP_MUTANTS[mutant]} at {e2:.2f} x (relative L2) and {em:.2f} x (max / max) of the bar; "
          f"{sum(max(v) > 1 for v in over.values())} of {len(over)} tensors past it")
    assert e2 >= 4.0 and em >= 4.0


# ---- host checks -----------------------------------------------------------------------------------------------------------------
def test_fit_parser_dropout_rate_flag(tmp_path):
    import json

    from reprover_amd.generator import fit

    ap = fit.build_parser()
    assert ap.parse_args(["--config", "c.yaml"]).dropout_rate == 0.0
    assert ap.parse_args(["--config", "c.yaml", "--dropout-rate", "0.1"]).dropout_rate == 0.1
    assert ap.parse_args(["--config", "c.yaml", "--dropout-rate", "config"]).dropout_rate == "config"
    for bad in ("1.0", "-0.1", "half"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--config", "c.yaml", "--dropout-rate", bad])
    ck = tmp_path / "ckpt"
    ck.mkdir()
    (ck / "config.json").write_text(json.dumps({"dropout_rate": 0.25}))
    assert fit.resolve_dropout_rate("config", str(ck)) == 0.25 and fit.resolve_dropout_rate(0.1, str(ck)) == 0.1
    (ck / "config.json").write_text(json.dumps({"d_model": 8}))
    assert fit.resolve_dropout_rate("config", str(ck)) == 0.1  # T5Config's default
    with pytest.raises(SystemExit, match="--ckpt_path"):  # a hub name (the reference yaml's model_name) is not a directory
        fit.resolve_dropout_rate("config", "google/byt5-small")


def test_training_state_carries_the_seed_base_and_the_forward_count(tmp_path):
    """HipT5Trainer's state file (HipSeq2SeqTrainer's encoder_state.safetensors) records (dropout_seed, forwards drawn); a
    file without the field loads as before and leaves the stream where it is.  Run on a stand-in with host tensors."""
    from safetensors.torch import load_file, save_file

    from reprover_amd.train import HipT5Trainer

    def stand_in(seed, forwards):
        z = torch.zeros(8)
        return types.SimpleNamespace(params=z.clone(), exp_avg=z.clone(), exp_avg_sq=z.clone(), steps=3, dropout_seed=seed,
                                     _forwards=forwards, load_params=lambda: None)

    path = str(tmp_path / "state.safetensors")
    HipT5Trainer.save_training_state(stand_in(7, 41), path)
    assert load_file(path)["dropout"].tolist() == [7, 41]
    fresh = stand_in(3407, 0)
    HipT5Trainer.load_training_state(fresh, path)
    assert (fresh.dropout_seed, fresh._forwards, fresh.steps) == (7, 41, 3)
    old = {k: v for k, v in load_file(path).items() if k != "dropout"}
    save_file(old, path)
    fresh = stand_in(11, 5)
    HipT5Trainer.load_training_state(fresh, path)
    assert (fresh.dropout_seed, fresh._forwards, fresh.steps) == (11, 5, 3)


def test_site_constants_agree_and_are_disjoint():
    from reprover_amd import decoder as D

    def enum_values(path):
        text = open(os.path.join(ROOT, path)).read()
        return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"\b(?:RP_)?(DROP_SITE_\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", text)}

    py = {k: getattr(D, k) for k in dir(D) if k.startswith("DROP_SITE_")}
    assert len(py) == 6
    assert enum_values("include/reprover_hip.h") == py
    assert enum_values("reprover_amd/csrc/rp_encoder_kernels.h") == py
    assert [D.DEC_SELF_PROBS, D.DEC_SELF_RESID, D.DEC_CROSS_PROBS, D.DEC_CROSS_RESID, D.DEC_FF_INNER, D.DEC_FF_RESID] == \
        [DEC_KINDS[k] for k in ("self_probs", "self_resid", "cross_probs", "cross_resid", "ff_inner", "ff_resid")] == list(range(6))
    L = 64
    enc = {D.DROP_SITE_EMBED, D.DROP_SITE_FINAL} | {D.DROP_SITE_LAYER0 + 8 * i + k for i in range(L) for k in range(4)}
    dec = {D.DROP_SITE_DEC_EMBED, D.DROP_SITE_DEC_FINAL} | {D.DROP_SITE_DEC_LAYER0 + 8 * i + k for i in range(L) for k in range(6)}
    assert len(enc) == 2 + 4 * L and len(dec) == 2 + 6 * L and not (enc & dec)
