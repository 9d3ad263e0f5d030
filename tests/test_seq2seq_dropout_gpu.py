"""T5's dropout through the whole seq2seq training path on the MI355X: the new entry points give
the old ones' bits at p = 0; at p = 0.1 the loss and every gradient equal the float64 reference GIVEN THE SAME MASKS (read
back with rp_dbg_dropout_mask, tests/seq2seq_dropout_helpers.py) within section 11's rule; mask statistics, seeds and
reproducibility; workspace hygiene of the three new hot entry points; the training step, its resume and the fit loop."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hip_helpers import Arena, guard_bytes, hygiene_findings  # noqa: E402
from seq2seq_dropout_helpers import DEC_KINDS, ENC_KINDS, DeviceMasks, reference_full_grads_dropout  # noqa: E402
from seq2seq_full_grad_helpers import g26_sources, padded_sources  # noqa: E402
from seq2seq_grad_helpers import GRAD_TOL_FACTOR, g25_labels, padded_labels, rel_l2, rel_max  # noqa: E402
from seq2seq_train_helpers import RefTrainer64, f32  # noqa: E402
import test_step_ends_gpu as step_ends  # noqa: E402  (the optimizer-end bar: its derivation, not a copy)
from oracle import train_ref  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd import decoder as D  # noqa: E402
from reprover_amd.decoder import HipSeq2SeqGradients, HipT5Decoder, HipT5Generator, packed_pairs, shift_and_segment  # noqa: E402
from reprover_amd.seq2seq_train import HipSeq2SeqTrainer  # noqa: E402
from reprover_amd.train import HipT5Trainer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, SEED = 0.1, 7

# Tensors past GRAD_TOL_FACTOR x the rounded reference's own error under the same masks -> (relative L2 bound, max / max
# bound, reason), each bound 2 x the figure measured on the MI355X (in the comment); None keeps the rule's bound on that
# metric.  Keys: (case, tensor).  The whole-model cases (tiny, tiny-tied on G26) need none.
_SELF = "decoder.block.0.layer.0."
_ONE_KEY = ("T = 1: one key per query, so softmax is constant and d q, d k and the bias-table gradient are IDENTICALLY ZERO in both "
            "references (their metrics fall back to the absolute figure).  The engine's dS = P (M dP - delta) takes delta from the "
            "bf16-rounded out, a residue of 2^-8 |dO . out| that does not cancel; it reaches these three tensors and, through "
            "the q / k paths, the self-attention norm weight.  Every other tensor of the case is inside the rule.")
DROP_GRAD_TOL = {
    ("d128-f64-T1", _SELF + "SelfAttention.q.weight"): (2 * 9.031e-2, 2 * 9.031e-2, _ONE_KEY),       # absolute, measured 9.031e-2
    ("d128-f64-T1", _SELF + "SelfAttention.k.weight"): (2 * 3.157e-2, 2 * 3.157e-2, _ONE_KEY),       # absolute, 3.157e-2
    ("d128-f64-T1", _SELF + "SelfAttention.relative_attention_bias.weight"): (2 * 8.605e-3, 2 * 8.605e-3, _ONE_KEY),  # 8.605e-3
    ("d128-f64-T1", _SELF + "layer_norm.weight"): (2 * 1.520e-2, None, _ONE_KEY),  # rel L2 1.520e-2 (rule: 1.496e-2)
    ("d1472-f3584-T1", _SELF + "SelfAttention.q.weight"): (2 * 7.923e-2, 2 * 7.923e-2, _ONE_KEY),    # absolute, 7.923e-2
    ("d1472-f3584-T1", _SELF + "SelfAttention.k.weight"): (2 * 5.374e-2, 2 * 5.374e-2, _ONE_KEY),    # absolute, 5.374e-2
    ("d1472-f3584-T1", _SELF + "SelfAttention.relative_attention_bias.weight"): (2 * 7.496e-3, 2 * 7.496e-3, _ONE_KEY),  # 7.496e-3
    ("d1472-f3584-T1", _SELF + "layer_norm.weight"): (2 * 1.781e-2, None, _ONE_KEY),  # rel L2 1.781e-2 (rule: 1.526e-2)
}
# the same for a loss: case -> (bound on |loss - reference loss|, the reason)
_ONE_SCALAR = ("the rounded reference's loss deviates by ONE realisation of bf16 rounding noise summed into a scalar (4.8e-4 and "
               "2.5e-4 here; 3.7e-3 and 1.7e-3 on the neighbouring T = 129); the engine's is another realisation, 1e-4 of the loss, "
               "and every gradient of the case is inside the rule (TRAIN_TOL of tests/test_seq2seq_train_gpu.py: the same finding)")
DROP_LOSS_TOL = {
    "d128-f64-T127": (2 * 1.462e-3, _ONE_SCALAR),     # measured 1.462e-3 (rule: 9.54e-4)
    "d1472-f3584-T127": (2 * 8.420e-4, _ONE_SCALAR),  # measured 8.420e-4 (rule: 5.05e-4)
}


def _bounds(key, rule_l2, rule_max):
    """(relative L2 bound, max / max bound) of a tensor: the rule's, or DROP_GRAD_TOL's named entry"""
    t2, tm = DROP_GRAD_TOL.get(key, (None, None, ""))[:2]
    return (rule_l2 if t2 is None else t2), (rule_max if tm is None else tm)


def _batch():
    (ids, mask), y = padded_sources(g26_sources()), padded_labels(g25_labels())
    return ids, mask, y


def _model(name):
    cfg = synth.seq2seq_config(name)
    return cfg, synth.synth_seq2seq_state_dict(cfg, scale="hf")


def _views(dec, flat):
    names, off = dec.grad_layout()
    shapes = dec.grad_shapes()
    return {n: flat[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))] for i, n in enumerate(names)}


# ---- a. p = 0: the old entry points' bits ---------------------------------------------------------------------------------------
def _dec_case(name):
    if name == "byt5-width":  # tests/test_seq2seq_grad_gpu.py's one-layer ByT5-small-width case
        cfg = dict(synth.seq2seq_config("byt5-small"), num_decoder_layers=1)
        rng = np.random.default_rng(25)
        encs = [torch.from_numpy(rng.standard_normal((s, cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16)
                for s in (65, 1)]
        y = padded_labels([np.concatenate([np.arange(3, 132), [1]]), np.array([9, 200, 1])])
    else:
        from seq2seq_grad_helpers import g25_encs

        cfg = synth.seq2seq_config(name)
        encs, y = g25_encs(cfg), padded_labels(g25_labels())
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    tokens, labels, tgt_cu = shift_and_segment(np.asarray(y))
    src_cu = np.concatenate([[0], np.cumsum([e.shape[0] for e in encs])]).astype(np.int32)
    return cfg, sd, (torch.cat(encs).to(DEV).contiguous(), src_cu, tokens, labels, tgt_cu)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_decoder_dropout_entry_at_p0_gives_loss_grads_bits(name):
    cfg, sd, args = _dec_case(name)
    dec = HipT5Decoder(cfg, sd, DEV)
    lp0, sc0, flat0, de0 = dec.loss_grad(*args)
    lp1, sc1, flat1, de1 = dec.loss_grad(*args, dropout=(0.0, 12345))
    torch.cuda.synchronize()
    assert sc0 == sc1 and torch.equal(lp0, lp1) and torch.equal(de0, de1)
    v0, v1 = _views(dec, flat0), _views(dec, flat1)
    for k in v0:
        assert torch.equal(v0[k], v1[k]), k
    lib = _lib.load()
    B = len(args[1]) - 1
    cu = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data  # noqa: E731
    assert lib.rp_decoder_loss_grad_dropout_workspace_bytes(dec._handle, cu(args[1]), cu(args[4]), B) == \
        lib.rp_decoder_loss_grad_workspace_bytes(dec._handle, cu(args[1]), cu(args[4]), B) > 0


@pytest.mark.parametrize("name", ["tiny", "byt5-small-1-layer"])
def test_hidden_dropout_pair_with_dropout_unset_gives_the_plain_pairs_bits(name):
    cfg = synth.t5_config("tiny") if name == "tiny" else dict(synth.t5_config("byt5-small"), num_layers=1)
    sd = synth.synth_state_dict(cfg, scale="hf")
    tr = HipT5Trainer(cfg, sd, DEV)  # dropout_rate 0: the opt-in runs the _dropout entry points with dropout unset
    rng = np.random.default_rng(31)
    lens = (1, 129, 70)
    ids = np.concatenate([np.concatenate([rng.integers(3, 259, n - 1), [1]]) for n in lens]).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    d_hidden = torch.from_numpy(rng.standard_normal((int(cu[-1]), cfg["d_model"])).astype(np.float32)).to(DEV)
    h0 = tr.forward_hidden(ids, cu).clone()
    g0 = tr.backward_hidden(d_hidden).clone()
    h1 = tr.forward_hidden(ids, cu, dropout=True).clone()
    g1 = tr.backward_hidden(d_hidden, dropout=True).clone()
    torch.cuda.synchronize()
    assert tr.last_dropout_seed is None
    assert torch.equal(h0, h1) and torch.equal(g0, g1)


# ---- b. the whole model under masks -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full(name):
    cfg, sd = _model(name)
    model = HipSeq2SeqGradients(cfg, sd, DEV, dropout_rate=P, dropout_seed=SEED)
    loss, grads = model.loss_and_grads(*_batch())
    torch.cuda.synchronize()
    return cfg, sd, model, loss, {k: v.detach().clone() for k, v in grads.items()}, model.last_d_enc.clone(), model.last_dropout_seed


def _cus(cfg):
    ids, mask, y = _batch()
    _, src_cu, _, _, tgt_cu = packed_pairs(cfg, ids, mask, y)
    return src_cu, tgt_cu


def margins(name):
    """per tensor: relative L2 and max / max against the unrounded reference under the step's masks, and the rounded
    reference's own figures; the loss row.  What profiles/seq2seq_dropout_margins.json and DESIGN.md section 15 quote."""
    cfg, sd, _, loss, grads, d_enc, seed = _full(name)
    masks = DeviceMasks(P, seed, *_cus(cfg))
    y = _batch()[2]
    ref_loss, gref, dref = reference_full_grads_dropout(cfg, sd, g26_sources(), y, masks)
    base_loss, gbase, dbase = reference_full_grads_dropout(cfg, sd, g26_sources(), y, masks, rounding=True)
    assert set(grads) == set(gref)
    got = {k: v.cpu().numpy() for k, v in grads.items()}
    got["d_enc"], gref["d_enc"], gbase["d_enc"] = d_enc.cpu().numpy(), dref, dbase
    rows = []
    for k in sorted(got):
        assert np.isfinite(got[k]).all(), k
        b2, bm = GRAD_TOL_FACTOR * rel_l2(gbase[k], gref[k]), GRAD_TOL_FACTOR * rel_max(gbase[k], gref[k])
        t2, tm = _bounds((name, k), b2, bm)
        rows.append(dict(tensor=k, rel_l2=rel_l2(got[k], gref[k]), bound_l2=t2, rel_max=rel_max(got[k], gref[k]), bound_max=tm,
                         rounded_l2=b2 / GRAD_TOL_FACTOR, rounded_max=bm / GRAD_TOL_FACTOR,
                         bound="DROP_GRAD_TOL" if (name, k) in DROP_GRAD_TOL else f"{GRAD_TOL_FACTOR} x rounded"))
    return dict(loss=loss, reference_loss=ref_loss, loss_error=abs(loss - ref_loss),
                loss_bound=GRAD_TOL_FACTOR * abs(base_loss - ref_loss), tensors=rows)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_gradients_equal_the_float64_reference_under_the_same_masks(name):
    """HipSeq2SeqGradients(dropout_rate=0.1, dropout_seed=7) on the G26 batch.  Every site's mask of the step is read back
    (encoder and decoder sites, probabilities per head) and handed to the float64 reference.  Per tensor (d_enc included),
    relative L2 and max / max against the unrounded reference are at most GRAD_TOL_FACTOR x the rounded reference's own
    error under the same masks (section 11's rule), DROP_GRAD_TOL's named entries aside; the loss within the same factor
    of the rounded reference's loss error.  profiles/seq2seq_dropout_margins.json holds margins() of both configurations."""
    m = margins(name)
    bad = []
    for r in m["tensors"]:
        print(f"{name} {r['tensor']}: rel L2 {r['rel_l2']:.3e} (bound {r['bound_l2']:.3e}, {r['rel_l2'] / r['bound_l2']:.2f} of "
              f"it); max/max {r['rel_max']:.3e} (bound {r['bound_max']:.3e}, {r['rel_max'] / r['bound_max']:.2f} of it) "
              f"[{r['bound']}]")
        if not (r["rel_l2"] <= r["bound_l2"] and r["rel_max"] <= r["bound_max"]):
            bad.append((r["tensor"], r["rel_l2"], r["bound_l2"], r["rel_max"], r["bound_max"]))
    print(f"{name}: loss {m['loss']:.6f}, reference {m['reference_loss']:.6f}, error {m['loss_error']:.3e} "
          f"(bound {m['loss_bound']:.3e})")
    assert m["loss_error"] <= m["loss_bound"]
    assert not bad, bad
    cfg, sd, _, loss, _, d_enc, _ = _full(name)
    plain = HipSeq2SeqGradients(cfg, sd, DEV)
    loss0, _ = plain.loss_and_grads(*_batch())
    assert plain.last_dropout_seed is None and loss0 != loss
    src_cu, _ = _cus(cfg)
    assert not d_enc[src_cu[3] : src_cu[4]].any() and d_enc[src_cu[2] : src_cu[3]].any()


# ---- c. the masks ---------------------------------------------------------------------------------------------------------------
def test_mask_statistics_and_site_separation():
    """Per site (every encoder and decoder site, a second layer and layer 63): the kept fraction within 5 sqrt(q (1 - q) / n)
    of q = 1 - 6554 / 65536; any two sites' masks differ, so a decoder site's mask differs from the encoder site's on the same
    rows; another seed gives another mask."""
    m = DeviceMasks(P, 99, [0], [0])
    q = 1.0 - 6554.0 / 65536.0
    sites = [("enc", "embed", None), ("enc", "final", None), ("dec", "embed", None), ("dec", "final", None)]
    sites += [("enc", k, 1) for k in ENC_KINDS] + [("dec", k, 1) for k in DEC_KINDS] + [("dec", "self_probs", 63)]
    seen = {}
    for half, kind, layer in sites:
        site = m.site(half, kind, layer)
        col0 = (1 << 20) if "probs" in kind else 0
        got = m.read(site, 130, col0, 300, 256).numpy()
        n = got.size
        assert set(np.unique(got)) == {0.0, 1.0}
        assert abs(got.mean() - q) <= 5 * np.sqrt(q * (1 - q) / n), (half, kind, layer, got.mean())
        for other, arr in seen.items():
            assert not np.array_equal(arr, got), (other, (half, kind, layer))
        seen[(half, kind, layer)] = got
    other_seed = DeviceMasks(P, 100, [0], [0]).read(m.site("dec", "embed", None), 130, 0, 300, 256).numpy()
    assert not np.array_equal(other_seed, seen[("dec", "embed", None)])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.3])
@pytest.mark.parametrize("T,n", [(1, 128), (130, 1472)])
def test_kept_values_are_exactly_the_fp32_multiplier_on_the_device(T, n, p):
    """The decoder's embedding site through its two fp32 kernels alone (rp_dbg_decoder_embed_dropout: dec_embed_drop_kernel
    and bwd_embed_kernel<false, true>), T = 1 and 130 rows.  On a table of ones every element of x is, bit for bit, 0 or
    fp32 1 / (1 - p), and it is kept exactly where rp_dbg_dropout_mask says; on a random table x = mask * embed[id] in fp32,
    bit for bit; with distinct ids the table gradient's row id is mask * dx of that token, bit for bit, every other row 0."""
    lib = _lib.load()
    rng = np.random.default_rng(T + n)
    V = 200
    ids = rng.permutation(V)[:T].astype(np.int32)
    kept = DeviceMasks(p, 77, [0], [0]).read(D.DROP_SITE_DEC_EMBED, 0, 0, T, n).to(DEV) != 0
    scale = torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p)), device=DEV)  # fp32 1.f / (1.f - p)
    want_m = torch.where(kept, scale, torch.zeros((), device=DEV))
    dx = torch.from_numpy(rng.standard_normal((T, n)).astype(np.float32)).to(DEV)
    for table in (torch.ones((V, n), device=DEV), torch.from_numpy(rng.standard_normal((V, n)).astype(np.float32)).to(DEV)):
        x = torch.full((T, n), 7.0, device=DEV)
        dtab = torch.full((V, n), 7.0, device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(lib.rp_dbg_decoder_embed_dropout(_dev(ids).data_ptr(), T, table.data_ptr(), V, n, p, 77, dx.data_ptr(),
                                                        x.data_ptr(), dtab.data_ptr(), _lib.current_stream()),
                       "rp_dbg_decoder_embed_dropout")
        torch.cuda.synchronize()
        assert torch.equal(x, want_m * table[torch.from_numpy(ids.astype(np.int64)).to(DEV)])
        want_tab = torch.zeros((V, n), device=DEV)
        want_tab[torch.from_numpy(ids.astype(np.int64)).to(DEV)] = want_m * dx
        assert torch.equal(dtab, want_tab)
    assert 0 < int(kept.sum()) < kept.numel() or T == 1


def test_same_seed_same_bits_next_call_another_seed():
    cfg, sd, model, loss, grads, d_enc, seed = _full("tiny-tied")
    batch = _batch()
    loss2, grads2 = model.loss_and_grads(*batch)
    torch.cuda.synchronize()
    assert model.last_dropout_seed not in (None, seed)
    assert loss2 != loss and any(not torch.equal(grads2[k], grads[k]) for k in grads)
    other = HipSeq2SeqGradients(cfg, sd, DEV, dropout_rate=P, dropout_seed=SEED)
    loss3, grads3 = other.loss_and_grads(*batch)
    torch.cuda.synchronize()
    assert other.last_dropout_seed == seed and loss3 == loss and torch.equal(other.last_d_enc, d_enc)
    for k in grads:
        assert torch.equal(grads3[k], grads[k]), k
    # the parts with the step's seed give the step's bits; the default calls on a dropping trainer still refuse
    packed, src_cu, tokens, labels, tgt_cu = packed_pairs(cfg, *batch)
    with pytest.raises(ValueError):
        other.trainer.forward_hidden(packed, src_cu)
    with pytest.raises(ValueError):
        other.trainer.backward_hidden(d_enc)
    # inference through the same weights never drops
    gen = HipT5Generator.from_parts(cfg, other.trainer.encoder, other.decoder, DEV)
    assert gen.forward(*batch) == HipT5Generator(cfg, sd, DEV).forward(*batch)


# ---- c2. the row sites at tile edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 127, 129, 130])
@pytest.mark.parametrize("name", ["d128-f64", "d1472-f3584"])
def test_row_sites_at_tile_edges_through_a_one_layer_decoder(name, T):
    """The row sites at the launch's row counts that decide the 128-token tile tail and the `t >= n_tok` guards: the residual
    epilogue at T = 1, 127, 129 (and 130: embeddings and the final norm) with D = 128 and 1472, the gated-GELU epilogue at
    F = 64 and 3584.  Each T is a call of its own: rp_decoder_loss_grad_dropout on a ONE-layer decoder over given encoder
    rows, one pair of T target tokens, so n_tok = T.  Every decoder tensor and d_enc against the float64 decoder reference
    under the read-back masks, section 11's rule as above; DROP_GRAD_TOL / DROP_LOSS_TOL name what is past it (the T = 1
    tensors whose exact gradient is identically zero, and the loss at T = 127)."""
    from seq2seq_dropout_helpers import reference_decoder_grads_dropout

    base = synth.seq2seq_config("tiny" if name == "d128-f64" else "byt5-small")
    cfg = dict(base, num_decoder_layers=1, **({"d_ff": 64} if name == "d128-f64" else {}))
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    rng = np.random.default_rng(41 + T)
    S = 70
    encs = [torch.from_numpy(rng.standard_normal((S, cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16)]
    y = padded_labels([np.concatenate([rng.integers(3, 259, size=T - 1), [1]]).astype(np.int64)])
    tokens, labels, tgt_cu = shift_and_segment(y)
    assert tuple(tgt_cu) == (0, T)
    src_cu = np.array([0, S], dtype=np.int32)
    dec = HipT5Decoder(cfg, sd, DEV)
    _, (s, c), flat, d_enc = dec.loss_grad(encs[0].to(DEV).contiguous(), src_cu, tokens, labels, tgt_cu, dropout=(P, SEED))
    torch.cuda.synchronize()
    shapes = dec.grad_shapes()
    got = {k: v.cpu().numpy().reshape(shapes[k]) for k, v in _views(dec, flat).items()}
    got["d_enc"] = d_enc.cpu().numpy()
    masks = DeviceMasks(P, SEED, src_cu, tgt_cu)
    tied = bool(cfg["tie_word_embeddings"])
    f32 = [e.float() for e in encs]
    ref_loss, gref, dref = reference_decoder_grads_dropout(cfg, sd, f32, y, masks, tied=tied)
    base_loss, gbase, dbase = reference_decoder_grads_dropout(cfg, sd, f32, y, masks, rounding=True, tied=tied)
    gref["d_enc"], gbase["d_enc"] = np.concatenate(dref), np.concatenate(dbase)
    assert set(got) == set(gref)
    bad = []
    for k in sorted(got):
        assert np.isfinite(got[k]).all(), k
        e2, em = rel_l2(got[k], gref[k]), rel_max(got[k], gref[k])
        t2, tm = GRAD_TOL_FACTOR * rel_l2(gbase[k], gref[k]), GRAD_TOL_FACTOR * rel_max(gbase[k], gref[k])
        t2, tm = _bounds((f"{name}-T{T}", k), t2, tm)
        print(f"{name} T={T} {k}: rel L2 {e2:.3e} (bound {t2:.3e}); max/max {em:.3e} (bound {tm:.3e})")
        if not (e2 <= t2 and em <= tm):
            bad.append((k, e2, t2, em, tm))
    loss = s / c
    lb = DROP_LOSS_TOL.get(f"{name}-T{T}", (GRAD_TOL_FACTOR * abs(base_loss - ref_loss),))[0]
    print(f"{name} T={T}: loss {loss:.6f}, reference {ref_loss:.6f} (error {abs(loss - ref_loss):.3e}, bound {lb:.3e})")
    if not abs(loss - ref_loss) <= lb:
        bad.append(("loss", abs(loss - ref_loss), lb))
    assert not bad, bad


# ---- d. workspace hygiene of the three new hot entry points ---------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_hidden_dropout_entry_points_workspace_hygiene():
    """tests/test_workspace_hygiene_gpu.py's recipe on rp_train_forward_hidden_dropout + rp_train_backward_hidden_dropout
    (p = 0.1) as one sequence: an exactly-sized workspace poisoned with 0x00 / 0xFF / 0x7F gives the same output bits, the
    guards stay intact, one byte less is refused with nothing written."""
    cfg = synth.t5_config("tiny")
    tr = HipT5Trainer(cfg, synth.synth_state_dict(cfg, scale="hf"), DEV)
    lib, g, Dm = tr._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"]
    rng = np.random.default_rng(11)
    lens = (1, 129, 70)
    ids = np.concatenate([np.concatenate([rng.integers(3, 259, n - 1), [1]]) for n in lens]).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    batch, T = len(lens), int(cu[-1])
    a_ids, a_cu = Arena.of("ids", _dev(ids), g), Arena.of("cu_seqlens", _dev(cu), g)
    d_hidden = Arena.of("d_hidden", _dev(rng.standard_normal((T, Dm)).astype(np.float32)), g)
    ws = Arena("workspace", lib.rp_train_workspace_bytes(tr._handle, T, batch), g, DEV)
    hid = Arena("out_hidden", T * Dm * 2, g, DEV, dtype=torch.bfloat16)
    grads = Arena.of("grads", torch.full((int(tr.layout[-1][2]),), 12345.0, dtype=torch.float32, device=DEV), g)
    _lib.check(lib.rp_trainer_set_dropout(tr._handle, P, SEED), "rp_trainer_set_dropout")

    def call(n):
        st = lib.rp_train_forward_hidden_dropout(tr._handle, a_ids.ptr, a_cu.ptr, batch, T, hid.ptr, ws.ptr, n,
                                                 _lib.current_stream())
        if st:
            return st
        return lib.rp_train_backward_hidden_dropout(tr._handle, tr.params.data_ptr(), a_ids.ptr, a_cu.ptr, batch, T,
                                                    d_hidden.ptr, grads.ptr, ws.ptr, n, _lib.current_stream())

    results = {}
    try:
        with torch.cuda.device(DEV):
            found = hygiene_findings(call, ws, [hid, grads], [a_ids, a_cu, d_hidden], results=results)
    finally:
        lib.rp_trainer_set_dropout(tr._handle, 0.0, 0)
    assert not found, "\n".join(found)
    out = results["out_hidden"].float()
    assert torch.isfinite(out).all() and 0.05 < float((out == 0).float().mean()) < 0.15  # the final site dropped a tenth


def test_decoder_dropout_entry_point_workspace_hygiene():
    """The same recipe on rp_decoder_loss_grad_dropout (p = 0.1) with the workspace of its own size function."""
    cfg, sd, (enc, src_cu, tokens, labels, tgt_cu) = _dec_case("tiny-tied")
    dec = HipT5Decoder(cfg, sd, DEV)
    lib, g = _lib.load(), guard_bytes(cfg["d_ff"])
    src_h, tgt_h = np.ascontiguousarray(src_cu, dtype=np.int32), np.ascontiguousarray(tgt_cu, dtype=np.int32)
    B, S, T = len(src_h) - 1, int(src_h[-1]), int(tgt_h[-1])
    a_enc = Arena.of("enc", enc, g)
    a_tok, a_lab = Arena.of("tokens", _dev(tokens.astype(np.int32)), g), Arena.of("labels", _dev(labels.astype(np.int32)), g)
    ws = Arena("workspace", lib.rp_decoder_loss_grad_dropout_workspace_bytes(dec._handle, src_h.ctypes.data, tgt_h.ctypes.data, B),
               g, DEV)
    lp, sc = Arena("label_logprobs", T * 4, g, DEV, dtype=torch.float32), Arena("loss_sum_count", 16, g, DEV, dtype=torch.float64)
    grads = Arena.of("grads", torch.full((int(dec.grad_layout()[1][-1]),), 12345.0, dtype=torch.float32, device=DEV), g)
    d_enc = Arena("d_enc", S * cfg["d_model"] * 4, g, DEV, dtype=torch.float32)

    def call(n):
        return lib.rp_decoder_loss_grad_dropout(dec._handle, a_enc.ptr, src_h.ctypes.data, a_tok.ptr, a_lab.ptr, tgt_h.ctypes.data,
                                                B, P, SEED, lp.ptr, sc.ptr, grads.ptr, d_enc.ptr, ws.ptr, n, _lib.current_stream())

    results = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, ws, [lp, sc, grads, d_enc], [a_enc, a_tok, a_lab], results=results)
    assert not found, "\n".join(found)
    assert torch.isfinite(results["d_enc"]).all() and torch.isfinite(results["label_logprobs"]).all()


# ---- e. the training step ---------------------------------------------------------------------------------------------------------
def _state(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in dict(
        enc_p=tr.trainer.params, enc_m=tr.trainer.exp_avg, enc_v=tr.trainer.exp_avg_sq, dec_p=tr.dec_params,
        dec_m=tr.dec_exp_avg, dec_v=tr.dec_exp_avg_sq).items()}


class MaskedRefTrainer64(RefTrainer64):
    """tests/seq2seq_train_helpers.py's float64 step with the gradient taken under ``self.masks`` (set before every step)"""

    masks = None

    def gradients(self, sources, y, rounding=None):
        loss, grads, _ = reference_full_grads_dropout(self.cfg, self.state_dict(), sources, y, self.masks,
                                                      rounding=self.rounding if rounding is None else rounding)
        return loss, grads


# Figures of test_two_training_steps_against_reftrainer64_and_a_resume past GRAD_TOL_FACTOR x the rounded reference
# trajectory's own deviation -> (bound = 2 x the figure measured on the MI355X, the reason), as TRAIN_TOL of
# tests/test_seq2seq_train_gpu.py.  Keys: ("loss", step) or ("update", step, tensor).
TRAIN_DROP_TOL = {
    # measured 1.459e-2 where the rounded trajectory deviates by 7.27e-3 (2.007 x)
    ("update", 2, "decoder.block.0.layer.0.layer_norm.weight"): (
        2 * 1.459e-2, "the engine's backward rounds as well (dY, P and dS to bf16), the rounded reference's is exact; Adam's "
        "normalised update m / sqrt(v) turns relative gradient noise on small-gradient elements into update differences of "
        "the order of lr, and this tensor has 128 elements; step 1 and every other tensor of step 2 are inside the rule"),
}


def test_two_training_steps_against_reftrainer64_and_a_resume(tmp_path):
    """HipSeq2SeqTrainer(dropout_rate=0.1, dropout_seed=7), two steps on tiny-tied, beside RefTrainer64 driven with each
    step's read-back masks (an unrounded trajectory and a bf16-rounded one, each at its own weights).
      * the optimizer end: tests/test_seq2seq_train_gpu.py's bar - float64 AdamW applied to copies of this call's own
        gradients, masters and moments, the yardstick torch's fp32 AdamW on the same copies (2 x its error + one ulp);
      * each step's loss and, per tensor, the relative L2 of the accumulated update (masters - initial masters) against the
        unrounded reference trajectory: at most GRAD_TOL_FACTOR x the rounded trajectory's own deviation + one fp32 ulp of
        the tensor's largest master per element (the masters are fp32 on both sides but the engine's AdamW arithmetic is
        fp32 where the reference's is float64: tests/test_step_ends_gpu.py's ulp term; on a norm weight, 1.2e-7 against an
        update of 1e-3), TRAIN_DROP_TOL's named entries aside;
      * step 1 is HipSeq2SeqGradients' of the same seed bit for bit; a trainer resumed from the state saved after step 1
        (constructed with another seed base: the state carries it) takes step 2 with the uninterrupted run's bits."""
    name, lr = "tiny-tied", 1e-3
    betas, eps, wd = (0.9, 0.999), 1e-8, 1e-2
    cfg, sd = _model(name)
    tr = HipSeq2SeqTrainer(cfg, sd, DEV, lr=lr, weight_decay=wd, dropout_rate=P, dropout_seed=SEED)
    ids, mask, y = _batch()
    src_cu, tgt_cu = _cus(cfg)
    fb = (f32(betas[0]), f32(betas[1]))
    refs = [MaskedRefTrainer64(cfg, sd, f32(lr), 0, fb, f32(eps), f32(wd), rounding=r) for r in (False, True)]
    p0 = {k: v.copy() for k, v in refs[0].p.items()}
    e0, VD, o1 = int(tr.trainer.layout[0][2]), cfg["vocab_size"] * cfg["d_model"], int(tr.dec_off[1])
    cat = lambda enc, dec_tail: torch.cat([enc, dec_tail])  # noqa: E731
    _, _, _, loss1, grads1, _, seed1 = _full(name)
    bad, seeds = [], []
    for step in (1, 2):
        loss, grads = tr.loss_and_grads(ids, mask, y)
        torch.cuda.synchronize()
        seeds.append(tr.last_dropout_seed)
        if step == 1:
            assert seeds[0] == seed1 and loss == loss1 and all(torch.equal(grads[k], grads1[k]) for k in grads1)
        # the optimizer end on this call's own gradients
        g_enc = tr.trainer.grads.clone()
        g_enc[e0 : e0 + VD] = tr.trainer.grads[e0 : e0 + VD] + tr.dec_grads[:VD]
        g = cat(g_enc, tr.dec_grads[o1:].clone())
        p_in = cat(tr.trainer.params.clone(), tr.dec_params[o1:].clone())
        m_in = cat(tr.trainer.exp_avg.clone(), tr.dec_exp_avg.clone())
        v_in = cat(tr.trainer.exp_avg_sq.clone(), tr.dec_exp_avg_sq.clone())
        step_lr = f32(tr.trainer.current_lr())
        tr.optimizer_step()
        torch.cuda.synchronize()
        want = train_ref.adamw_step64(p_in.cpu().numpy(), g.cpu().numpy(), m_in.cpu().numpy(), v_in.cpu().numpy(), step, step_lr,
                                      fb, f32(eps), f32(wd))
        par = torch.nn.Parameter(p_in.clone())
        opt = torch.optim.AdamW([par], lr=step_lr, betas=fb, eps=f32(eps), weight_decay=f32(wd))
        opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m_in.clone(), "exp_avg_sq": v_in.clone()}
        par.grad = g.clone()
        opt.step()
        got = (cat(tr.trainer.params, tr.dec_params[o1:]), cat(tr.trainer.exp_avg, tr.dec_exp_avg),
               cat(tr.trainer.exp_avg_sq, tr.dec_exp_avg_sq))
        step_ends._compare_with_yardstick(f"dropout step {step}", "seq2seq_dropout", got,
                                          (par.detach(), opt.state[par]["exp_avg"], opt.state[par]["exp_avg_sq"]), want)
        # beside the reference trajectories under this step's masks
        masks = DeviceMasks(P, seeds[-1], src_cu, tgt_cu)
        ref_losses = []
        for r in refs:
            r.masks = masks
            ref_losses.append(r.step(g26_sources(), y))
        err, dev = abs(loss - ref_losses[0]), abs(ref_losses[1] - ref_losses[0])
        bound = TRAIN_DROP_TOL.get(("loss", step), (GRAD_TOL_FACTOR * dev,))[0]
        print(f"step {step}: loss {loss:.6f}, reference {ref_losses[0]:.6f}: error {err:.3e}, rounded trajectory's {dev:.3e}, "
              f"bound {bound:.3e}")
        if not err <= bound:
            bad.append(("loss", step, err, bound))
        mine = {k: v.cpu().numpy().astype(np.float64) for k, v in tr.state_dict().items() if k in p0}
        for k in sorted(p0):
            upd_ref = refs[0].p[k].astype(np.float64) - p0[k]
            e = rel_l2(mine[k] - p0[k], upd_ref)
            d = rel_l2(refs[1].p[k].astype(np.float64) - p0[k], upd_ref)
            floor = np.sqrt(upd_ref.size) * float(np.spacing(np.float32(np.abs(refs[0].p[k]).max()))) / np.sqrt((upd_ref ** 2).sum())
            bound = TRAIN_DROP_TOL.get(("update", step, k), (GRAD_TOL_FACTOR * d + floor,))[0]
            print(f"step {step} update of {k}: rel L2 {e:.3e}, rounded trajectory's {d:.3e}, bound {bound:.3e}")
            if not e <= bound:
                bad.append(("update", step, k, e, bound))
        if step == 1:
            tr.save_training_state(str(tmp_path / "state"))
    assert seeds[1] not in (None, seeds[0])
    end = _state(tr)
    fresh = HipSeq2SeqTrainer(cfg, sd, DEV, lr=lr, weight_decay=wd, dropout_rate=P, dropout_seed=SEED + 1000)
    fresh.load_training_state(str(tmp_path / "state"))
    fresh.loss_and_grads(ids, mask, y)
    assert fresh.last_dropout_seed == seeds[1]
    fresh.optimizer_step()
    got = _state(fresh)
    for k in end:
        assert torch.equal(end[k], got[k]), k
    assert not bad, bad


def test_run_fit_with_dropout_trains_and_validates_without_masks(tmp_path):
    from reprover_amd.generator.fit import run_fit
    from reprover_amd.generator.model import RetrievalAugmentedGenerator
    from test_seq2seq_train_gpu import LR, _fit_parts

    model, dm = _fit_parts(tmp_path)
    plain = model()
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_generator_data.json"),
                       encoding="utf-8"))["config"]
    dropping = RetrievalAugmentedGenerator(plain.model_name, LR, 0, 1, 100, 1, 1, 0, g["max_inp_seq_len"], g["max_oup_seq_len"],
                                           device=DEV, dropout_rate=P, dropout_seed=SEED)
    logs = []
    ck = str(tmp_path / "ck")
    out = run_fit(dropping, dm(), 3, ckpt_dir=ck, log=logs.append)
    assert out["steps"] == 3 and all(np.isfinite(out["losses"]))
    assert "dropout" in str(logs[0]) and "0.1" in str(logs[0])
    assert f"seed base {SEED}, 0 forwards" in str(logs[1])
    logs0 = []
    out0 = run_fit(plain, dm(), 3, log=logs0.append)
    assert "without T5's dropout" in str(logs0[0]) and out0["losses"] != out["losses"]
    d = dm()
    d.setup("validate")
    batch = next(iter(d.val_dataloader()))
    got = dropping.validation_step(batch)
    again = model(ck)
    want = again.validation_step(batch)
    assert got["loss_val"] == want["loss_val"] and dropping.last_preds == again.last_preds
    assert dropping.validation_step(batch)["loss_val"] == got["loss_val"]
