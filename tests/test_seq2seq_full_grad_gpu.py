"""Gradients of the seq2seq loss for the whole model on the MI355X: rp_train_forward_hidden /
rp_train_backward_hidden and HipSeq2SeqGradients against the float64 reference (tests/seq2seq_full_grad_helpers.py) and
fixture G26, consistency bit for bit with their parts, workspace hygiene, ABI errors, one descent step."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hip_helpers import Arena, guard_bytes, hygiene_findings  # noqa: E402
from seq2seq_full_grad_helpers import (FULL_GRAD_TOL, Enc64, g26_sources, load_g26, padded_sources,  # noqa: E402
                                       reference_full_grads)
from seq2seq_grad_helpers import GRAD_TOL_FACTOR, g25_labels, padded_labels, rel_l2, rel_max  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipSeq2SeqGradients, HipT5Generator, packed_pairs  # noqa: E402
from reprover_amd.train import HipT5Trainer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RP_E_INVALID, RP_E_WORKSPACE = -1, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 12345.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ids(rng, lens):
    ids = np.concatenate([np.concatenate([rng.integers(3, 259, n - 1), [1]]) for n in lens]).astype(np.int32)
    return ids, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ---- a. the forward hand-over ------------------------------------------------------------------------------------------------
def _enc_cfg(name):
    if name == "tiny":
        return synth.t5_config("tiny")
    return dict(synth.t5_config(name[: -len("-1-layer")]), num_layers=1)  # a one-layer cut of ByT5-small / -base


@functools.lru_cache(maxsize=None)
def _trainer(name):
    cfg = _enc_cfg(name)
    sd = synth.synth_state_dict(cfg, scale="hf")
    return cfg, sd, HipT5Trainer(cfg, sd, DEV)


def _encode_hidden(enc, ids, cu):
    """rp_encode_hidden rows (the inference pass) of the packed sequences"""
    B, T = len(cu) - 1, int(cu[-1])
    out = torch.empty((T, enc.cfg["d_model"]), dtype=torch.bfloat16, device=DEV)
    ws = enc._workspace(enc._lib.rp_encoder_workspace_bytes(enc._handle, T, B))
    ids_d, cu_d = _t(ids), _t(cu)
    with torch.cuda.device(DEV):
        _lib.check(enc._lib.rp_encode_hidden(enc._handle, ids_d.data_ptr(), cu_d.data_ptr(), B, T, int(np.diff(cu).max()),
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                   "rp_encode_hidden")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["tiny", "byt5-small-1-layer", "byt5-base-1-layer"])
def test_forward_hidden_rows_against_float64_and_the_inference_pass(name):
    """rp_train_forward_hidden's rows are no further from the float64 encoder than 2 x rp_encode_hidden's rows on the same
    input (the inference stream carries 24 bits per element, the training stream two bf16 planes; both round the GEMM
    operands to bf16), on relative L2 and on max error / max; d_model 1472 and 1536 are the two sides of the D <= 3 * 512
    template split.  A sequence's rows are the same bits alone or packed with others.

    Measured on the MI355X, forward_hidden / encode_hidden: relative L2 4.34e-3 / 4.40e-3 (tiny), 3.153e-3 / 3.152e-3
    (D = 1472), 3.17e-3 / 3.17e-3 (D = 1536); max / max 4.58e-3 / 4.77e-3, 4.72e-3 / 4.10e-3, 3.35e-3 / 3.80e-3."""
    cfg, sd, tr = _trainer(name)
    lens = (1, 129, 70)
    ids, cu = _ids(np.random.default_rng(31), lens)
    got = tr.forward_hidden(ids, cu)
    torch.cuda.synchronize()
    assert got.shape == (int(cu[-1]), cfg["d_model"]) and got.dtype == torch.bfloat16
    inf = _encode_hidden(tr.encoder, ids, cu)
    enc = Enc64(cfg, sd)
    with torch.no_grad():
        ref = torch.cat([enc.forward(ids[cu[b] : cu[b + 1]]) for b in range(len(lens))]).numpy()
    g, i = got.float().cpu().numpy(), inf.float().cpu().numpy()
    assert np.isfinite(g).all()
    e_tr, e_inf = (rel_l2(g, ref), rel_max(g, ref)), (rel_l2(i, ref), rel_max(i, ref))
    print(f"{name}: forward_hidden rel L2 {e_tr[0]:.3e} max/max {e_tr[1]:.3e}; encode_hidden rel L2 {e_inf[0]:.3e} "
          f"max/max {e_inf[1]:.3e}")
    assert e_tr[0] <= 2 * e_inf[0] and e_tr[1] <= 2 * e_inf[1]
    for b in range(len(lens)):
        alone = tr.forward_hidden(ids[cu[b] : cu[b + 1]], np.array([0, lens[b]], dtype=np.int32))
        assert torch.equal(alone, got[cu[b] : cu[b + 1]]), b


# ---- b. gradients on G26 -----------------------------------------------------------------------------------------------------
def _batch():
    (ids, mask), y = padded_sources(g26_sources()), padded_labels(g25_labels())
    return ids, mask, y


@functools.lru_cache(maxsize=None)
def _full(name):
    """(cfg, sd, model, loss, gradients as float64 numpy, d_enc) of one G26 configuration, computed once"""
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    model = HipSeq2SeqGradients(cfg, sd, DEV)
    loss, grads = model.loss_and_grads(*_batch())
    torch.cuda.synchronize()
    return cfg, sd, model, loss, {k: v.detach().clone() for k, v in grads.items()}, model.last_d_enc.clone()


def margins(name):
    """per tensor of a G26 configuration: (tensor, relative L2, its bound, max / max, its bound, which bound), and the loss
    row; the figures profiles/seq2seq_full_grad_margins.json and DESIGN.md section 13 quote"""
    cfg, sd, _, loss, grads, _ = _full(name)
    fx = load_g26(GOLDEN, name)
    ref_loss, gref, _ = reference_full_grads(cfg, sd, g26_sources(), fx["labels"])
    assert set(grads) == set(gref) == set(fx["tensors"])
    rows = []
    for k in sorted(grads):
        got = grads[k].cpu().numpy()
        assert np.isfinite(got).all(), k
        t2, tm = FULL_GRAD_TOL.get((name, k), (fx["tensors"][k]["bf16_l2"], fx["tensors"][k]["bf16_max"]))
        rows.append(dict(tensor=k, rel_l2=rel_l2(got, gref[k]), bound_l2=t2, rel_max=rel_max(got, gref[k]), bound_max=tm,
                         hf_bf16_l2=fx["tensors"][k]["bf16_l2"], hf_bf16_max=fx["tensors"][k]["bf16_max"],
                         bound="FULL_GRAD_TOL" if (name, k) in FULL_GRAD_TOL else "HF-bf16"))
    return dict(loss=loss, reference_loss=ref_loss, loss_error=abs(loss - ref_loss),
                loss_bound=abs(float(fx["loss"][1]) - float(fx["loss"][0])), tensors=rows)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_gradients_against_float64_reference_on_g26(name):
    """Every parameter's gradient: relative L2 and max error / max against the float64 reference, each no worse than
    HF-bf16 autograd's own error on that tensor (fixture G26), FULL_GRAD_TOL's named exceptions aside; the loss within
    |HF-bf16 loss - HF-fp32 loss|.

    Measured on the MI355X (profiles/seq2seq_full_grad_margins.json): our error is 0.12 - 0.75 of HF-bf16's on relative
    L2 and 0.08 - 0.86 on max / max over all 103 tensors of both configurations; loss error 7.1e-3 (bar 8.3e-2) and
    3.7e-4 (bar 3.1e-2).  FULL_GRAD_TOL has no entry."""
    m = margins(name)
    bad = []
    for r in m["tensors"]:
        print(f"{name} {r['tensor']}: rel L2 {r['rel_l2']:.3e} (bound {r['bound_l2']:.3e}, {r['rel_l2'] / r['bound_l2']:.2f} "
              f"of it); max/max {r['rel_max']:.3e} (bound {r['bound_max']:.3e}, {r['rel_max'] / r['bound_max']:.2f} of it) "
              f"[{r['bound']}]")
        if not (r["rel_l2"] <= r["bound_l2"] and r["rel_max"] <= r["bound_max"]):
            bad.append((r["tensor"], r["rel_l2"], r["bound_l2"], r["rel_max"], r["bound_max"]))
    print(f"{name}: loss {m['loss']:.6f}, reference {m['reference_loss']:.6f}, error {m['loss_error']:.3e} "
          f"(bound {m['loss_bound']:.3e})")
    assert m["loss_error"] <= m["loss_bound"]
    assert not bad, bad


def test_full_grad_tol_exceptions_are_one_sided():
    """an exception widens one metric only: the other stays at HF-bf16's figure or below"""
    for (name, k), (t2, tm) in FULL_GRAD_TOL.items():
        fx = load_g26(GOLDEN, name)["tensors"][k]
        assert t2 <= fx["bf16_l2"] or tm <= fx["bf16_max"], (name, k)


# ---- c. consistency, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_parts_and_repeat_bit_for_bit(name):
    cfg, sd, model, loss, grads, d_enc = _full(name)
    ids, mask, y = _batch()
    packed, src_cu, tokens, labels, tgt_cu = packed_pairs(cfg, ids, mask, y)
    hidden = model.trainer.forward_hidden(packed, src_cu)
    _, (s, c), flat, de = model.decoder.loss_grad(hidden, src_cu, tokens, labels, tgt_cu, want_d_enc=True)
    assert loss == s / c and torch.equal(de, d_enc)
    names, off = model.decoder.grad_layout()
    shapes = model.decoder.grad_shapes()
    dec = {n: flat[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))].view(shapes[n]) for i, n in enumerate(names)}
    enc = dict(model.trainer._views(model.trainer.backward_hidden(de)))
    assert set(grads) == set(dec) | set(enc) == {k for k in sd if "embed_tokens" not in k}
    for k, g in grads.items():
        assert tuple(g.shape) == tuple(sd[k].shape) and g.dtype == torch.float32 and g.is_cuda, k
        if k == "shared.weight":
            assert torch.equal(g, enc[k] + dec[k])
            assert bool(enc[k].any()) and bool(dec[k].any())
        else:
            assert torch.equal(g, dec[k] if k in dec else enc[k]), k
    loss2, grads2 = model.loss_and_grads(ids, mask, y)
    assert loss2 == loss and all(torch.equal(grads2[k], grads[k]) for k in grads)
    assert torch.equal(model.last_d_enc, d_enc)
    # d_enc of the pair without labels is an all-zero block; only that pair: NaN loss, every gradient zero
    assert not d_enc[src_cu[3] : src_cu[4]].any()
    loss0, g0 = model.loss_and_grads(ids[3:4], mask[3:4], y[3:4])
    assert np.isnan(loss0) and not any(bool(g.any()) for g in g0.values())
    with pytest.raises(ValueError):
        model.loss_and_grads(ids[:2], np.array([mask[0], np.zeros_like(mask[1])]), y[:2])  # an empty source


# ---- d. ByT5-small widths ----------------------------------------------------------------------------------------------------
def test_byt5_small_widths_against_the_rounded_reference():
    """ByT5-small's widths (tile edges that 128 and 256 hide), two encoder layers and one decoder layer, the G26 batch: every
    encoder tensor and shared.weight at most GRAD_TOL_FACTOR x the error of the bf16-rounded float64 reference on the same
    tensor (reference_full_grads(rounding=True): the forward's rounding points, exact backward), as section 11 holds the
    decoder's tensors.

    Measured on the MI355X: relative L2 1.88 % - 2.14 % per tensor where the rounded reference is at 1.99 % - 2.31 %."""
    cfg = dict(synth.seq2seq_config("byt5-small"), num_layers=2, num_decoder_layers=1)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    ids, mask, y = _batch()
    model = HipSeq2SeqGradients(cfg, sd, DEV)
    loss, grads = model.loss_and_grads(ids, mask, y)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in grads.items() if k.startswith("encoder.") or k == "shared.weight"}
    del model, grads
    ref_loss, gref, _ = reference_full_grads(cfg, sd, g26_sources(), y)
    _, gbase, _ = reference_full_grads(cfg, sd, g26_sources(), y, rounding=True)
    assert abs(loss - ref_loss) <= 2e-3 * max(1.0, abs(ref_loss))
    bad = []
    for k in sorted(got):
        assert np.isfinite(got[k]).all(), k
        e2, em = rel_l2(got[k], gref[k]), rel_max(got[k], gref[k])
        t2, tm = GRAD_TOL_FACTOR * rel_l2(gbase[k], gref[k]), GRAD_TOL_FACTOR * rel_max(gbase[k], gref[k])
        print(f"byt5-width {k}: rel L2 {e2:.3e} (bound {t2:.3e}); max/max {em:.3e} (bound {tm:.3e})")
        if not (e2 <= t2 and em <= tm):
            bad.append((k, e2, t2, em, tm))
    assert not bad, bad


# ---- e. workspace hygiene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "byt5-small-1-layer"])
def test_hidden_entry_points_workspace_hygiene(name):
    """rp_train_forward_hidden + rp_train_backward_hidden as one sequence on an exactly-sized workspace poisoned before the
    forward: the same bits under all three fills and both input-tail fills, every guard intact, one byte less refused with
    nothing written; the gradient buffer's padding gaps keep their sentinel."""
    cfg, _, tr = _trainer(name)
    lib, g, D = tr._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"]
    lens = (1, 129, 70)
    ids, cu = _ids(np.random.default_rng(11), lens)
    batch, T = len(lens), int(cu[-1])
    a_ids, a_cu = Arena.of("ids", _t(ids), g), Arena.of("cu_seqlens", _t(cu), g)
    d_hidden = Arena.of("d_hidden", _t(np.random.default_rng(12).standard_normal((T, D)).astype(np.float32)), g)
    ws = Arena("workspace", lib.rp_train_workspace_bytes(tr._handle, T, batch), g, DEV)
    hid = Arena("out_hidden", T * D * 2, g, DEV, dtype=torch.bfloat16)
    total = int(tr.layout[-1][2])
    grads = Arena.of("grads", torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV), g)
    _lib.check(lib.rp_trainer_set_dropout(tr._handle, 0.0, 0), "rp_trainer_set_dropout")

    def call(n):
        st = lib.rp_train_forward_hidden(tr._handle, a_ids.ptr, a_cu.ptr, batch, T, hid.ptr, ws.ptr, n, _lib.current_stream())
        if st:
            return st
        return lib.rp_train_backward_hidden(tr._handle, tr.params.data_ptr(), a_ids.ptr, a_cu.ptr, batch, T, d_hidden.ptr,
                                            grads.ptr, ws.ptr, n, _lib.current_stream())

    results = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, ws, [hid, grads], [a_ids, a_cu, d_hidden], results=results)
    assert not found, "\n".join(found)
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for _, shape, off in tr.layout[:-1]:
        live[int(off) : int(off) + int(np.prod(shape))] = True
    assert (results["grads"][~live] == SENTINEL).all(), "a padding gap was written"
    assert torch.isfinite(results["grads"][live]).all() and bool((results["grads"][live] != SENTINEL).any())
    assert torch.isfinite(results["out_hidden"].float()).all()


# ---- f. ABI errors -----------------------------------------------------------------------------------------------------------
def test_abi_errors_leave_everything_untouched():
    cfg, _, tr = _trainer("tiny")
    lib, D = tr._lib, cfg["d_model"]
    lens = (3, 130)
    ids, cu = _ids(np.random.default_rng(13), lens)
    batch, T = len(lens), int(cu[-1])
    ids_d, cu_d = _t(ids), _t(cu)
    cu_empty = _t(np.array([0, 0, T], dtype=np.int32))
    n = lib.rp_train_workspace_bytes(tr._handle, T, batch)
    ws = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    hid = torch.full((T, D), 7.0, dtype=torch.bfloat16, device=DEV)
    dh = torch.full((T, D), 0.5, dtype=torch.float32, device=DEV)
    grads = torch.full((int(tr.layout[-1][2]),), 7.0, dtype=torch.float32, device=DEV)
    s = _lib.current_stream()
    P = tr.params.data_ptr()

    def fwd(tr_=tr._handle, ids_=ids_d.data_ptr(), cu_=cu_d.data_ptr(), b=batch, out=hid.data_ptr(), w=ws.data_ptr(), nb=n):
        with torch.cuda.device(DEV):
            return lib.rp_train_forward_hidden(tr_, ids_, cu_, b, T, out, w, nb, s)

    def bwd(tr_=tr._handle, p=P, ids_=ids_d.data_ptr(), cu_=cu_d.data_ptr(), b=batch, d=dh.data_ptr(), g=grads.data_ptr(),
            w=ws.data_ptr(), nb=n):
        with torch.cuda.device(DEV):
            return lib.rp_train_backward_hidden(tr_, p, ids_, cu_, b, T, d, g, w, nb, s)

    _lib.check(lib.rp_trainer_set_dropout(tr._handle, 0.0, 0), "rp_trainer_set_dropout")
    for kw in (dict(tr_=None), dict(ids_=None), dict(cu_=None), dict(out=None), dict(b=0), dict(b=-1), dict(cu_=cu_empty.data_ptr())):
        assert fwd(**kw) == RP_E_INVALID, kw
    assert b"empty" in lib.rp_last_error()
    assert fwd(w=None) == RP_E_WORKSPACE and fwd(nb=n - 1) == RP_E_WORKSPACE
    for kw in (dict(tr_=None), dict(p=None), dict(ids_=None), dict(cu_=None), dict(d=None), dict(g=None), dict(b=0)):
        assert bwd(**kw) == RP_E_INVALID, kw
    assert bwd(w=None) == RP_E_WORKSPACE and bwd(nb=n - 1) == RP_E_WORKSPACE
    _lib.check(lib.rp_trainer_set_dropout(tr._handle, 0.1, 5), "rp_trainer_set_dropout")
    try:
        assert fwd() == RP_E_INVALID and b"dropout" in lib.rp_last_error()
        assert bwd() == RP_E_INVALID and b"dropout" in lib.rp_last_error()
    finally:
        _lib.check(lib.rp_trainer_set_dropout(tr._handle, 0.0, 0), "rp_trainer_set_dropout")
    torch.cuda.synchronize()  # no GPU error follows, and nothing was written
    assert (ws == 7).all() and (hid == 7.0).all() and (grads == 7.0).all()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(hid.float()).all() and not (hid == 7.0).all()
    # the Python layer: dropout and an empty sequence raise before anything is launched
    drop = HipT5Trainer(cfg, synth.synth_state_dict(cfg, scale="hf"), DEV, dropout_rate=0.1)
    with pytest.raises(ValueError):
        drop.forward_hidden(ids, cu)
    with pytest.raises(ValueError):
        drop.backward_hidden(dh)
    with pytest.raises(ValueError):
        tr.forward_hidden(ids, np.array([0, 0, T], dtype=np.int32))


# ---- g. one descent step -----------------------------------------------------------------------------------------------------
def test_one_descent_step_lowers_the_loss():
    """sd - eta * gradient for every parameter, HipT5Generator rebuilt from it: ``forward`` on the batch is lower.  The
    forward's loss is exact from run to run, with the resolution of an fp32 log-prob at the loss's size, 2^-23 * loss.  eta
    is taken from the gradient norm so that the first-order decrease eta |g|^2 is 2^17 times that resolution (1.6 % of the
    loss: the bf16 weights the engine keeps move by many ulps); the assertion asks for a quarter of the first-order
    decrease: curvature and the bf16 rounding of the stepped weights take the rest (as test_seq2seq_grad_gpu.py does for
    the decoder alone)."""
    cfg, sd, _, _, grads, _ = _full("tiny")
    ids, mask, y = _batch()
    loss0 = HipT5Generator(cfg, sd, DEV).forward(ids, mask, y)
    DESCENT_MULTIPLE = 2.0 ** 17
    resolution = 2.0 ** -23 * loss0
    g2 = float(sum((g.double() ** 2).sum() for g in grads.values()))
    eta = DESCENT_MULTIPLE * resolution / g2
    sd2 = dict(sd)
    for k, g in grads.items():
        sd2[k] = sd[k] - eta * g.cpu()
    for alias in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
        if alias in sd2:
            sd2[alias] = sd2["shared.weight"]
    loss1 = HipT5Generator(cfg, sd2, DEV).forward(ids, mask, y)
    print(f"descent: loss {loss0:.5f} -> {loss1:.5f} (first-order {DESCENT_MULTIPLE * resolution:.5f})")
    assert loss1 < loss0 - 0.25 * DESCENT_MULTIPLE * resolution
