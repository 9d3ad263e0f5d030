"""rp_decoder_load_params on the MI355X: a decoder created from weights W1 and reloaded with W2 computes
the bits of a decoder created from W2, on every entry point that reads a resident copy: rp_decoder_forward's log-prob rows
(the fp32 embedding and norms, the bf16 operands, the interleaved FFN-in copy, the bias table), rp_decoder_step over three
positions with two beams (the cross K/V concatenation, the plain FFN-in copy) and rp_decoder_loss_grad's gradients and
d_enc.  Everything is an equality of bits: the reload rounds each element once from the fp32 master, as create does."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Decoder  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RP_E_INVALID, RP_E_UNSUPPORTED = -1, -2
NB, STEPS = 2, 3


def _cfg(name):
    if name == "d_ff-40":  # no interleaved FFN-in copy (d_ff % 32 != 0): the table builder's other branch
        return dict(synth.seq2seq_config("tiny"), d_ff=40, num_decoder_layers=1)
    if name == "byt5-width":  # D 1472, F 3584, V 384: wi_0 has 5.3 M elements = 644 chunks of 8192; with the other 13
        # tensors the table has more chunks than the 2048 workgroups of the launch: the grid-stride tail runs
        return dict(synth.seq2seq_config("byt5-small"), num_layers=1, num_decoder_layers=1)
    return synth.seq2seq_config(name)


@functools.lru_cache(maxsize=None)
def _weights(name, seed):
    return synth.synth_seq2seq_state_dict(_cfg(name), seed=seed, scale="sharp")


def _flat(dec, sd):
    """sd's decoder tensors in rp_decoder_grad_layout's flat form; the padding gaps hold a value no copy may pick up"""
    names, off = dec.grad_layout()
    flat = torch.full((int(off[-1]),), float("nan"), dtype=torch.float32)
    for i, n in enumerate(names):
        flat[int(off[i]) : int(off[i]) + sd[n].numel()] = sd[n].reshape(-1)
    return flat.to(DEV)


def _inputs(cfg):
    rng = np.random.default_rng(14)
    lens = (70, 3)
    enc = torch.from_numpy(rng.standard_normal((sum(lens), cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16).to(DEV)
    src_cu = np.array([0, lens[0], sum(lens)], dtype=np.int32)
    labels = [np.concatenate([rng.integers(3, 259, 129), [1]]), np.array([9, 200, 1])]
    tokens = np.concatenate([np.concatenate([[0], y[:-1]]) for y in labels]).astype(np.int32)
    tgt_cu = np.array([0, 130, 133], dtype=np.int32)
    return enc, src_cu, tokens, np.concatenate(labels).astype(np.int32), tgt_cu


def _outputs(dec, teacher_forced=True):
    """every output that reads a resident copy, as host tensors"""
    cfg = dec.cfg
    enc, src_cu, tokens, labels, tgt_cu = _inputs(cfg)
    out = {}
    if teacher_forced:
        _, sc, rows = dec.forward(enc, src_cu, tokens, labels, tgt_cu, rows=True)
        out["rows"], out["sum_count"] = rows.cpu(), sc
        _, _, grads, d_enc = dec.loss_grad(enc, src_cu, tokens, labels, tgt_cu, want_d_enc=True)
        out["grads"], out["d_enc"] = grads.cpu(), d_enc.cpu()
    dec.start(enc[:70].contiguous(), NB, STEPS)
    for t in range(STEPS):
        anc = (torch.arange(t + 1)[None] * NB + torch.tensor([[0], [1]])) if t < 2 else torch.tensor([[0, 3, 4], [1, 2, 5]])
        out[f"step{t}"] = dec.step(torch.tensor([5 + t, 77]), anc).cpu()
    torch.cuda.synchronize()
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.isfinite(a[k]).all(), k
            assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "d_ff-40", "byt5-width"])
def test_reloaded_decoder_equals_a_fresh_one(name):
    cfg = _cfg(name)
    w1, w2 = _weights(name, 1), _weights(name, 2)
    tf = name != "d_ff-40"  # the teacher-forced entry points take d_ff % 64 == 0 only: the step is the path that exists there
    a, b = HipT5Decoder(cfg, w1, DEV), HipT5Decoder(cfg, w2, DEV)
    if not tf:
        with pytest.raises(_lib.HipLibraryError):
            b.forward(*_inputs(cfg))
    want = _outputs(b, tf)
    before = _outputs(a, tf)
    assert not torch.equal(before["step0"], want["step0"]), "the two weight sets must differ in the output"
    flat2 = _flat(a, w2)
    a.load_params(flat2)
    _same(_outputs(a, tf), want)
    # the same weights again: nothing moves
    a.load_params(flat2)
    _same(_outputs(a, tf), want)
    # ... and back: W1's bits return (no copy is left behind from W2)
    a.load_params(_flat(a, w1))
    _same(_outputs(a, tf), before)


def test_two_reloads_back_to_back_on_a_stream_then_a_forward():
    """W1 then W2 with no synchronisation in between, then the outputs, on a side stream: the second reload's bits"""
    cfg = _cfg("tiny")
    a, b = HipT5Decoder(cfg, _weights("tiny", 3), DEV), HipT5Decoder(cfg, _weights("tiny", 2), DEV)
    want = _outputs(b)
    f1, f2 = _flat(a, _weights("tiny", 1)), _flat(a, _weights("tiny", 2))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        a.load_params(f1)
        a.load_params(f2)
        got = _outputs(a)
    _same(got, want)


def test_null_arguments_are_refused_and_nothing_is_launched():
    cfg = _cfg("tiny")
    a = HipT5Decoder(cfg, _weights("tiny", 1), DEV)
    before = _outputs(a)
    flat = _flat(a, _weights("tiny", 2))
    lib, s = a._lib, _lib.current_stream()
    assert lib.rp_decoder_load_params(None, flat.data_ptr(), s) == RP_E_INVALID
    assert lib.rp_decoder_load_params(a._handle, None, s) == RP_E_INVALID
    assert lib.rp_decoder_load_params(a._handle, flat.data_ptr() + 4, s) == RP_E_INVALID  # not 16-byte aligned
    assert lib.rp_last_error()
    with pytest.raises(ValueError):
        a.load_params(flat[:-64])
    _same(_outputs(a), before)
