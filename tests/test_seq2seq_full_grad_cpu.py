"""The whole-model gradient reference (tests/seq2seq_full_grad_helpers.py) against HF fp32 autograd (fixture G26), against
central differences, and its planted mutants, without a GPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seq2seq_full_grad_helpers import (ENC_FINAL_LN, ENC_REL_BIAS, FULL_GRAD_TOL, FULL_MUTANTS, Enc64, g26_sources,  # noqa: E402
                                       g26_stride, load_g26, reference_full_grads)
from seq2seq_grad_helpers import g25_labels, padded_labels, rel_l2  # noqa: E402
from seq2seq_helpers import T5ForwardEmu  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The bound test_seq2seq_grad_cpu.py holds the decoder reference to on G25 (HF_FP32_REL).  Measured here on G26 over every
# tensor of both configurations: at most 7.5e-6 (the fp32 rounding of HF's own pass), so the bound stays.
HF_FP32_REL = 2.2e-5


@functools.lru_cache(maxsize=None)
def _g26(name, mutant=None):
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    fx = load_g26(GOLDEN, name)
    assert np.array_equal(fx["labels"], padded_labels(g25_labels()))
    loss, g, _ = reference_full_grads(cfg, sd, g26_sources(), fx["labels"], mutant=mutant)
    return fx, loss, g


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_reference_equals_hf_fp32_on_g26(name):
    fx, loss, g = _g26(name)
    assert abs(loss - fx["loss"][0]) <= 1e-5 * abs(loss)
    assert set(g) == set(fx["tensors"])
    worst = 0.0
    for k, t in fx["tensors"].items():
        e = rel_l2(t["sample"], g[k].reshape(-1)[:: g26_stride(k)])
        n = abs(np.sqrt((g[k] ** 2).sum()) / t["norm"] - 1.0)
        m = abs(np.abs(g[k]).max() / t["max"] - 1.0)
        worst = max(worst, e, n, m)
        assert e <= HF_FP32_REL and n <= HF_FP32_REL and m <= HF_FP32_REL, (k, e, n, m)
    print(f"G26 {name}: reference vs HF fp32, worst relative figure {worst:.2e}")


def _small():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    srcs = [np.array([7, 200, 31, 1]), np.array([90, 4, 17, 250, 66, 1])]
    y = padded_labels([np.array([7, 9, 1]), np.array([4, -100, 250, 1])])
    return cfg, sd, srcs, y


def test_encoder_gradient_matches_central_differences():
    """Central differences of the float64 loss along random directions of a handful of encoder tensors agree with the
    composed gradient to 1e-6 relative.  Step 1e-6: the float64 truncation is ~3e-9 absolute; at 1e-5 the third-order
    term of a random direction of a q matrix (HF's scale: std 0.011) is 2e-6 relative and falls 100 x with the step."""
    cfg, sd, srcs, y = _small()
    loss, grads, _ = reference_full_grads(cfg, sd, srcs, y)
    assert np.isfinite(loss)
    dec = T5ForwardEmu(cfg, sd, rounding=False)

    def loss64(sd2):
        enc = Enc64(cfg, sd2)
        with torch.no_grad():
            return dec.forward([enc.forward(s) for s in srcs], y)[0]

    assert abs(loss64(sd) - loss) <= 1e-12 * abs(loss)
    rng = np.random.default_rng(5)
    for name in (ENC_REL_BIAS, ENC_FINAL_LN, "encoder.block.0.layer.0.SelfAttention.q.weight",
                 "encoder.block.1.layer.0.SelfAttention.o.weight", "encoder.block.0.layer.1.DenseReluDense.wi_1.weight",
                 "encoder.block.1.layer.1.layer_norm.weight"):
        u = rng.standard_normal(sd[name].shape)
        h = 1e-6
        vals = [loss64(dict(sd, **{name: sd[name].double() + sgn * h * torch.from_numpy(u)})) for sgn in (+1, -1)]
        fd = (vals[0] - vals[1]) / (2 * h)
        an = float((grads[name] * u).sum())
        print(f"{name}: central difference {fd:.9e}, gradient {an:.9e}")
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (name, fd, an)


def test_shared_is_the_sum_and_ignored_labels_give_zero():
    cfg, sd, srcs, y = _small()
    _, g, _ = reference_full_grads(cfg, sd, srcs, y)
    _, g_dec, _ = reference_full_grads(cfg, sd, srcs, y, mutant="embed_not_added")
    assert rel_l2(g_dec["shared.weight"], g["shared.weight"]) > 0.1
    used = np.unique(np.concatenate(srcs))
    diff = g["shared.weight"] - g_dec["shared.weight"]  # the encoder's part: rows of the source ids only
    assert diff[used].any() and not np.delete(diff, used, axis=0).any()
    loss, g0, d_enc = reference_full_grads(cfg, sd, srcs, np.full_like(y, -100))
    assert np.isnan(loss) and not any(t.any() for t in g0.values()) and not d_enc.any()
    want = {k for k in sd if "embed_tokens" not in k}
    assert set(g) == want


def _tol(name, fx, k):
    return FULL_GRAD_TOL.get((name, k), (fx["tensors"][k]["bf16_l2"], fx["tensors"][k]["bf16_max"]))[0]


# mutant -> configuration; every one moves its target tensor by more than 10 x that tensor's GPU bound (measured:
# embed_not_added 31 x, final_norm_mean_dropped 64 x, next_source 40 x)
MUTANT_CASES = {"embed_not_added": "tiny-tied", "final_norm_mean_dropped": "tiny-tied", "next_source": "tiny"}


@pytest.mark.parametrize("mutant", sorted(FULL_MUTANTS))
def test_planted_full_gradient_mutants_are_separated(mutant):
    name = MUTANT_CASES[mutant]
    fx, _, g = _g26(name)
    _, _, gm = _g26(name, mutant)
    target = FULL_MUTANTS[mutant]
    move = rel_l2(gm[target], g[target])
    ratio = move / _tol(name, fx, target)
    print(f"mutant {mutant} ({name}): moves {target} by {move:.3e} = {ratio:.1f} x its bound {_tol(name, fx, target):.3e}")
    assert ratio > 10


def test_hidden_entry_symbols():
    """The two additive entry points exist, the ABI version did not move, and a null trainer is refused without touching
    a device."""
    lib = _lib.load()
    assert lib.rp_abi_version() == 7
    for name in ("rp_train_forward_hidden", "rp_train_backward_hidden"):
        assert hasattr(lib, name), name
    assert lib.rp_train_forward_hidden(None, None, None, 1, 1, None, None, 0, None) == -1  # RP_E_INVALID
    assert lib.rp_train_backward_hidden(None, None, None, None, 1, 1, None, None, None, 0, None) == -1
    assert b"null" in lib.rp_last_error()
