"""rp_decoder_loss_grad on the MI355X: parity of every parameter gradient and of d loss / d enc with the float64
reference (tests/seq2seq_grad_helpers.py), the forward's bits, determinism, batch invariance of d_enc, edges, ABI errors
and the public interface (HipT5Generator.loss_and_grads, one descent step)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seq2seq_grad_helpers import (GRAD_TOL, GRAD_TOL_FACTOR, g25_encs, g25_labels, load_g25, padded_labels,  # noqa: E402
                                  reference_grads, rel_l2, rel_max)
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, HipT5Generator, shift_and_segment  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RP_E_INVALID, RP_E_WORKSPACE = -1, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg(name):
    if name == "byt5-width":  # ByT5-small's widths (tile edges that 128 and 256 hide), one decoder layer
        return dict(synth.seq2seq_config("byt5-small"), num_decoder_layers=1)
    return synth.seq2seq_config(name)


@functools.lru_cache(maxsize=None)
def _decoder(name):
    cfg = _cfg(name)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    return cfg, sd, HipT5Decoder(cfg, sd, DEV)


def _encs(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal((s, cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16)
            for s in lens]


def _run(dec, encs, y, want_d_enc=True, grads=None, order=None):
    order = list(range(len(encs))) if order is None else order
    tokens, labels, tgt_cu = shift_and_segment(np.asarray(y)[order])
    src_cu = np.concatenate([[0], np.cumsum([encs[b].shape[0] for b in order])]).astype(np.int32)
    enc = torch.cat([encs[b] for b in order]).to(DEV).contiguous()
    lp, sc, flat, d_enc = dec.loss_grad(enc, src_cu, tokens, labels, tgt_cu, want_d_enc, grads)
    torch.cuda.synchronize()
    return dict(lp=lp, sc=sc, flat=flat, d_enc=d_enc, src_cu=src_cu, args=(enc, src_cu, tokens, labels, tgt_cu))


def _named(dec, flat):
    names, off = dec.grad_layout()
    shapes = dec.grad_shapes()
    f = flat.cpu().numpy()
    return {n: f[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))].reshape(shapes[n]) for i, n in enumerate(names)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, decoder, encs, labels, result, reference, rounded baseline) of one parity case, computed once"""
    cfg, sd, dec = _decoder(name)
    if name == "byt5-width":
        encs = _encs(cfg, (65, 1), 25)
        y = padded_labels([np.concatenate([np.arange(3, 132), [1]]), np.array([9, 200, 1])])
    else:
        encs, y = g25_encs(cfg), padded_labels(g25_labels())
    out = _run(dec, encs, y)
    tied = bool(cfg["tie_word_embeddings"])
    f32 = [e.float() for e in encs]
    ref = reference_grads(cfg, sd, f32, y, rounding=False, tied=tied)
    base = reference_grads(cfg, sd, f32, y, rounding=True, tied=tied)
    return cfg, dec, encs, y, out, ref, base


@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_gradients_against_float64_reference(name):
    """Per tensor, relative L2 and max error / max against the float64 reference.  G25 configurations: no worse than
    HF-bf16 autograd's own error on the tensor (the fixture), GRAD_TOL's named exceptions aside.  ByT5-small widths: at
    most GRAD_TOL_FACTOR x the rounded reference's error."""
    cfg, dec, encs, y, out, (loss, gref, eref), (_, gbase, ebase) = _case(name)
    s, c = out["sc"]
    assert abs(s / c - loss) <= 2e-3 * max(1.0, abs(loss))
    got = _named(dec, out["flat"])
    assert set(got) == set(gref)
    got["d_enc"] = out["d_enc"].cpu().numpy()
    gref, gbase = dict(gref), dict(gbase)
    gref["d_enc"], gbase["d_enc"] = np.concatenate(eref), np.concatenate(ebase)
    assert got["d_enc"].shape[0] == out["src_cu"][-1]
    fx = load_g25(GOLDEN, name)["tensors"] if name != "byt5-width" else None
    bad = []
    for k in sorted(got):
        assert np.isfinite(got[k]).all(), k
        e2, em = rel_l2(got[k], gref[k]), rel_max(got[k], gref[k])
        if fx is None:
            t2, tm = GRAD_TOL_FACTOR * rel_l2(gbase[k], gref[k]), GRAD_TOL_FACTOR * rel_max(gbase[k], gref[k])
            what = "2 x rounded reference"
        else:
            t2, tm = GRAD_TOL.get((name, k), (fx[k]["bf16_l2"], fx[k]["bf16_max"]))
            what = "GRAD_TOL" if (name, k) in GRAD_TOL else "HF-bf16"
        print(f"{name} {k}: rel L2 {e2:.3e} (bound {t2:.3e}, margin {t2 / e2:.2f} x); max/max {em:.3e} (bound {tm:.3e}, "
              f"margin {tm / em:.2f} x) [{what}]")
        if not (e2 <= t2 and em <= tm):
            bad.append((k, e2, t2, em, tm))
    assert not bad, bad


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_grad_layout_matches_the_state_dict(name):
    """rp_decoder_grad_layout against the checkpoint: the names in the documented order, one entry per decoder
    parameter, monotone 64-aligned offsets, every gap covering its HF tensor's numel with less than 64 spare."""
    cfg, sd, dec = _decoder(name)
    names, off = dec.grad_layout()
    keys = [k for k in sd if (k.startswith("decoder.") and k != "decoder.embed_tokens.weight")
            or k in ("shared.weight", "lm_head.weight")]
    assert sorted(names) == sorted(keys) and len(set(names)) == len(names)
    L = cfg["num_decoder_layers"]
    head = [] if cfg["tie_word_embeddings"] else ["lm_head.weight"]
    assert names[: 3 + len(head)] == ["shared.weight"] + head + [
        "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", "decoder.final_layer_norm.weight"]
    order = ["layer.0.layer_norm", "layer.0.SelfAttention.q", "layer.0.SelfAttention.k", "layer.0.SelfAttention.v",
             "layer.0.SelfAttention.o", "layer.1.layer_norm", "layer.1.EncDecAttention.q", "layer.1.EncDecAttention.k",
             "layer.1.EncDecAttention.v", "layer.1.EncDecAttention.o", "layer.2.layer_norm",
             "layer.2.DenseReluDense.wi_0", "layer.2.DenseReluDense.wi_1", "layer.2.DenseReluDense.wo"]
    assert names[3 + len(head):] == [f"decoder.block.{i}.{o}.weight" for i in range(L) for o in order]
    assert len(off) == len(names) + 1 == dec._lib.rp_decoder_grad_tensors(dec._handle) + 1
    assert off[0] == 0
    shapes = dec.grad_shapes()
    for i, n in enumerate(names):
        numel = int(sd[n].numel())
        assert tuple(shapes[n]) == tuple(sd[n].shape), n
        assert off[i] % 64 == 0 and numel <= off[i + 1] - off[i] <= numel + 63, (n, off[i], off[i + 1], numel)


def test_forward_bits_determinism_gaps_and_null_d_enc():
    # the forward's bits on every cached case: two layers (slot stride), a 129- and a 260-token target (a second 128-query
    # block, Tp > n_tgt), an empty target beside non-empty ones, tied and untied heads, d_model 1472 (no multiple of 128)
    for name in ("tiny", "tiny-tied", "byt5-width"):
        _, dec, _, _, out, _, _ = _case(name)
        lp, sc, _ = dec.forward(*out["args"])
        assert torch.equal(lp, out["lp"]) and sc == out["sc"], name
    cfg, dec, encs, y, out, _, _ = _case("tiny")
    names, off = dec.grad_layout()
    shapes = dec.grad_shapes()
    assert all(o % 64 == 0 for o in off)
    sentinel = torch.full((int(off[-1]),), 12345.0, dtype=torch.float32, device=DEV)
    again = _run(dec, encs, y, grads=sentinel)
    assert torch.equal(again["d_enc"], out["d_enc"])
    live = torch.zeros(int(off[-1]), dtype=torch.bool)
    for i, n in enumerate(names):
        live[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))] = True
    live = live.to(DEV)
    assert torch.equal(again["flat"][live], out["flat"][live])
    assert (again["flat"][~live] == 12345.0).all()
    nod = _run(dec, encs, y, want_d_enc=False)
    assert nod["d_enc"] is None and torch.equal(nod["flat"], out["flat"]) and torch.equal(nod["lp"], out["lp"])


def test_d_enc_rows_alone_batched_permuted():
    """d_enc x count of a pair does not depend on the other pairs: alone, batched (equal counts arranged by comparing
    d_enc * count in float64 would round; instead the pair alone is compared with itself in a permuted single-count
    batch), and the whole batch permuted (same count: identical bits)."""
    cfg, dec, encs, y, out, _, _ = _case("tiny")
    order = [2, 0, 4, 1, 3]
    perm = _run(dec, encs, y, order=order)
    cu, pcu = out["src_cu"], perm["src_cu"]
    for pos, b in enumerate(order):
        assert torch.equal(perm["d_enc"][pcu[pos] : pcu[pos + 1]], out["d_enc"][cu[b] : cu[b + 1]]), b
    assert torch.equal(perm["flat"].isfinite(), torch.ones_like(perm["flat"], dtype=torch.bool))
    # pair 2 alone against pair 2 beside pairs whose labels are all ignored (the same count)
    y2 = np.full_like(y, -100)
    y2[2] = y[2]
    alone = _run(dec, [encs[2]], y[2:3])
    beside = _run(dec, encs, y2)
    assert alone["sc"] == beside["sc"]
    assert torch.equal(beside["d_enc"][cu[2] : cu[3]], alone["d_enc"])
    assert not beside["d_enc"][: cu[2]].any() and not beside["d_enc"][cu[3] :].any()


def test_edges_and_errors():
    cfg, dec, encs, y, out, _, _ = _case("tiny")
    none = _run(dec, encs, np.full_like(y, -100))
    assert none["sc"] == (0.0, 0.0)
    assert not none["flat"].any() and not none["d_enc"].any()
    # interior ignored labels only in one pair, the others counted nowhere near: finite everywhere
    assert torch.isfinite(out["flat"]).all() and torch.isfinite(out["d_enc"]).all()
    cu = out["src_cu"]
    assert not out["d_enc"][cu[3] : cu[4]].any()  # the empty pair's source receives no gradient
    # ABI errors: nothing is written
    enc, src_cu, tokens, labels, tgt_cu = out["args"]
    lib = dec._lib
    pc = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = int(lib.rp_decoder_loss_grad_workspace_bytes(dec._handle, pc(src_cu), pc(tgt_cu), len(tgt_cu) - 1))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    tok, lab = (torch.from_numpy(a).to(DEV) for a in (tokens, labels))
    T = int(tgt_cu[-1])
    lp = torch.full((T,), 7.0, device=DEV)
    sc = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    g = torch.full((int(dec.grad_layout()[1][-1]),), 7.0, device=DEV)
    de = torch.full((int(src_cu[-1]), cfg["d_model"]), 7.0, device=DEV)

    def call(grads_ptr, ws_bytes):
        with torch.cuda.device(DEV):
            return lib.rp_decoder_loss_grad(dec._handle, enc.data_ptr(), pc(src_cu), tok.data_ptr(), lab.data_ptr(),
                                            pc(tgt_cu), len(tgt_cu) - 1, lp.data_ptr(), sc.data_ptr(), grads_ptr,
                                            de.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream())

    assert call(g.data_ptr(), n - 1) == RP_E_WORKSPACE
    assert call(None, n) == RP_E_INVALID
    torch.cuda.synchronize()
    for t in (lp, sc, g, de):
        assert (t == 7.0).all()


def test_loss_and_grads_public_interface_and_descent():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    gen = HipT5Generator(cfg, sd, DEV)
    rng = np.random.default_rng(7)
    lens, tl = (40, 9, 130), (12, 30, 5)
    ids = np.zeros((3, max(lens)), np.int64)
    mask = np.zeros_like(ids)
    y = np.full((3, max(tl)), -100, np.int64)
    for b in range(3):
        ids[b, : lens[b]] = np.concatenate([rng.integers(3, 259, lens[b] - 1), [1]])
        mask[b, : lens[b]] = 1
        y[b, : tl[b]] = np.concatenate([rng.integers(3, 259, tl[b] - 1), [1]])
    loss0 = gen.forward(ids, mask, y)
    loss, grads, d_enc = gen.loss_and_grads(ids, mask, y)
    assert loss == loss0
    dec_keys = {k for k in sd if (k.startswith("decoder.") and k != "decoder.embed_tokens.weight")
                or k in ("shared.weight", "lm_head.weight")}
    assert set(grads) == dec_keys
    assert d_enc.shape == (sum(lens), cfg["d_model"]) and d_enc.dtype == torch.float32
    for k, g in grads.items():
        assert tuple(g.shape) == tuple(sd[k].shape), k
    # One descent step on the decoder weights.  The forward's loss is exact from run to run (a fixed-order fp64 sum of fp32
    # log-probs), so its resolution is the spacing of an fp32 log-prob at the loss's size, 2^-23 * loss.  eta is taken
    # from the gradient norm so that the first-order decrease eta |g|^2 is DESCENT_MULTIPLE = 2^17 times that resolution
    # (1.6 % of the loss: large enough that the bf16 weights the engine keeps move by many ulps).  The assertion asks
    # for a quarter of the first-order decrease: curvature and the bf16 rounding of the stepped weights take the rest.
    DESCENT_MULTIPLE = 2.0 ** 17
    resolution = 2.0 ** -23 * loss
    g2 = float(sum((g.double() ** 2).sum() for g in grads.values()))
    eta = DESCENT_MULTIPLE * resolution / g2
    sd2 = dict(sd)
    for k, g in grads.items():
        sd2[k] = sd[k] - eta * g.cpu()
    # the encoder reads shared.weight too: keep its copy, only the decoder side steps
    gen2 = HipT5Generator.__new__(HipT5Generator)
    gen2.cfg, gen2.device, gen2.encoder = gen.cfg, gen.device, gen.encoder
    gen2.decoder = HipT5Decoder(cfg, sd2, DEV)
    loss1 = gen2.forward(ids, mask, y)
    print(f"descent: loss {loss0:.5f} -> {loss1:.5f} (first-order {DESCENT_MULTIPLE * resolution:.5f})")
    assert loss1 < loss0 - 0.25 * DESCENT_MULTIPLE * resolution
