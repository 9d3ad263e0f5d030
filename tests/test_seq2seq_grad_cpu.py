"""The decoder-gradient reference (tests/seq2seq_grad_helpers.py) and the flat gradient layout of rp_decoder_loss_grad,
without a GPU."""
import ctypes as C
import os
import sys

import functools

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seq2seq_grad_helpers import (G25_STRIDE, GRAD_MUTANTS, GRAD_TOL, LAYER_KEYS, g25_encs, g25_labels, load_g25,  # noqa: E402
                                  packed, padded_labels, reference_grads, rel_l2)
from reprover_amd import _lib, synth  # noqa: E402


def _small():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    rng = np.random.default_rng(3)
    encs = [torch.from_numpy(rng.standard_normal((s, cfg["d_model"])) * 0.3) for s in (3, 5)]
    y = padded_labels([np.array([7, 9, 1]), np.array([4, -100, 250, 1])])
    return cfg, sd, encs, y


def test_reference_gradient_matches_finite_differences():
    """Central differences of the float64 loss along random directions agree with the autograd gradient to 1e-6 relative
    (float64 truncation at step 1e-5 is ~1e-10; the bound leaves room for the curvature term)."""
    cfg, sd, encs, y = _small()
    loss, grads, d_enc = reference_grads(cfg, sd, encs, y)
    assert np.isfinite(loss)
    rng = np.random.default_rng(4)
    names = ["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", "decoder.final_layer_norm.weight",
             "decoder.block.1.layer.1.EncDecAttention.k.weight", "decoder.block.0.layer.2.DenseReluDense.wi_0.weight",
             "shared.weight", "lm_head.weight"]
    for name in names:
        u = rng.standard_normal(sd[name].shape)
        h = 1e-5
        vals = []
        for sgn in (+1, -1):
            sd2 = dict(sd)
            sd2[name] = sd[name].double() + sgn * h * torch.from_numpy(u)
            vals.append(_loss64(cfg, sd2, encs, y))
        fd = (vals[0] - vals[1]) / (2 * h)
        an = float((grads[name] * u).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (name, fd, an)
    u = rng.standard_normal(encs[1].shape)
    e2 = [[encs[0], encs[1] + s * 1e-5 * torch.from_numpy(u)] for s in (+1, -1)]
    fd = (_loss64(cfg, sd, e2[0], y) - _loss64(cfg, sd, e2[1], y)) / 2e-5
    an = float((d_enc[1] * u).sum())
    assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (fd, an)


def _loss64(cfg, sd, encs, y):
    """the reference's loss with float64 weights (T5ForwardEmu casts through fp32, which would swallow a 1e-5 step)"""
    from seq2seq_helpers import T5ForwardEmu

    emu = T5ForwardEmu(cfg, {k: v.float() for k, v in sd.items()}, rounding=False)
    emu.embed, emu.tab = sd["shared.weight"].double(), sd[
        "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].double()
    emu.final_ln, emu.lm = sd["decoder.final_layer_norm.weight"].double(), sd["lm_head.weight"].double()
    for i, l in enumerate(emu.layers):
        for fld, key in LAYER_KEYS.items():
            l[fld] = sd[f"decoder.block.{i}.{key}"].double()
    return emu.forward(encs, y)[0]


def test_reference_ignored_labels_and_tied_sum():
    cfg, sd, encs, y = _small()
    loss, grads, d_enc = reference_grads(cfg, sd, encs, np.full_like(y, -100))
    assert np.isnan(loss) and not any(g.any() for g in grads.values()) and not any(e.any() for e in d_enc)
    _, g_untied, _ = reference_grads(cfg, sd, encs, y)
    _, g_tied, _ = reference_grads(cfg, sd, encs, y, tied=True)
    assert "lm_head.weight" not in g_tied
    assert np.array_equal(g_tied["shared.weight"], g_untied["shared.weight"] + g_untied["lm_head.weight"])


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Measured distance of the float64 reference from HF fp32 autograd on G25, relative L2 over the stored sample: at most
# 1.1e-5 on any tensor of either configuration (7.1e-6 tiny, 1.1e-5 tiny-tied: the fp32 rounding of HF's own pass); the
# issue's bar is 1e-4, tightened to twice the observed value.
HF_FP32_REL = 2.2e-5


@functools.lru_cache(maxsize=None)
def _g25(name, mutant=None):
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    fx = load_g25(GOLDEN, name)
    assert np.array_equal(fx["labels"], padded_labels(g25_labels()))
    loss, g, de = reference_grads(cfg, sd, [e.float() for e in g25_encs(cfg)], fx["labels"],
                                  tied=bool(cfg["tie_word_embeddings"]), mutant=mutant)
    g = dict(g)
    g["d_enc"] = packed(de)
    return fx, loss, g


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_reference_equals_hf_fp32_on_g25(name):
    fx, loss, g = _g25(name)
    assert abs(loss - fx["loss"][0]) <= 1e-5 * abs(loss)
    assert set(g) == set(fx["tensors"])
    worst = 0.0
    for k, t in fx["tensors"].items():
        e = rel_l2(t["sample"], g[k].reshape(-1)[::G25_STRIDE])
        n = abs(np.sqrt((g[k] ** 2).sum()) / t["norm"] - 1.0)
        m = abs(np.abs(g[k]).max() / t["max"] - 1.0)
        worst = max(worst, e, n, m)
        assert e <= HF_FP32_REL and n <= HF_FP32_REL and m <= HF_FP32_REL, (k, e, n, m)
    print(f"G25 {name}: reference vs HF fp32, worst relative figure {worst:.2e}")


def _tol(name, fx, k):
    return GRAD_TOL.get((name, k), (fx["tensors"][k]["bf16_l2"], fx["tensors"][k]["bf16_max"]))[0]


# mutant -> (configuration it is run on, measured move of its target tensor / that tensor's GPU bound).  A ratio below 10
# is a documented floor: the bug is real but small on G25 (see the comment), and the assertion holds the measured ratio.
MUTANT_CASES = {
    "bias_off_by_one": "tiny", "clamp_dropped": "tiny", "next_source": "tiny", "tied_head_missing": "tiny-tied",
    "mean_all": "tiny", "final_scale_missing": "tiny-tied",
}
# Mutants that separate by less than 10 x their tensor's bound on G25, with the measured ratio (asserted as a floor):
# clamp_dropped: only distances 256 .. 259 of the 260-label target are clamped (10 of its 33930 causal pairs), and they
#   share bucket 31 with every distance from 113 up: the table gradient moves by 3.7e-3, 0.055 x its bound.  No batch
#   within the fixture's size separates it; the GPU test's clamp coverage is the parity of rel_bias itself.
# tied_head_missing: the head's part is 28 % of shared's gradient on G25: 5.8 x the bound (HF-bf16's 4.9 % on shared).
MUTANT_FLOOR = {"clamp_dropped": 0.05, "tied_head_missing": 5.0}


@pytest.mark.parametrize("mutant", sorted(GRAD_MUTANTS))
def test_planted_gradient_mutants_are_separated(mutant):
    name = MUTANT_CASES[mutant]
    fx, _, g = _g25(name)
    _, _, gm = _g25(name, mutant)
    target = GRAD_MUTANTS[mutant]
    moves = {k: rel_l2(gm[k], g[k]) for k in g}
    ratio = moves[target] / _tol(name, fx, target)
    best = max(moves[k] / _tol(name, fx, k) for k in g)
    print(f"mutant {mutant} ({name}): moves {target} by {moves[target]:.3e} = {ratio:.1f} x its bound "
          f"{_tol(name, fx, target):.3e}; best tensor {best:.1f} x")
    if mutant in MUTANT_FLOOR:
        assert MUTANT_FLOOR[mutant] < ratio <= 10, "measured floor; above 10 the mutant belongs to the separated ones"
    else:
        assert ratio > 10  # i.e. no bound exceeds one tenth of what the mutant moves its tensor by


def test_grad_layout_symbols_and_alignment():
    """The new ABI symbols exist with the documented order: the layout functions need the library but no GPU (a null
    decoder is rejected without touching the device)."""
    lib = _lib.load()
    for name in ("rp_decoder_grad_tensors", "rp_decoder_grad_layout", "rp_decoder_loss_grad_workspace_bytes",
                 "rp_decoder_loss_grad"):
        assert hasattr(lib, name), name
    assert lib.rp_abi_version() == 7
    assert lib.rp_decoder_grad_tensors(None) == 0
    off = np.zeros(4, dtype=np.int64)
    assert lib.rp_decoder_grad_layout(None, off.ctypes.data_as(C.c_void_p)) == -1  # RP_E_INVALID
    assert lib.rp_decoder_loss_grad_workspace_bytes(None, None, None, 1) == 0
