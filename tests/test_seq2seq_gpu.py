"""rp_decoder_forward (the batched teacher-forced seq2seq forward) on the MI355X: against HF fp32 / bf16 (G19, G21, G22),
against the float64 reference (tests/seq2seq_helpers.py) at the reference's validation shapes, against the decode step
loop, same bits alone / batched / permuted, generate's scores, edge cases and ABI errors."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from seq2seq_helpers import FORWARD_TOL, STEP_TOL, T5ForwardEmu  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G22_LOSS_REL = 4e-4  # measured 2.2e-4 (tiny), 1.9e-4 (ByT5-small) at HF scale; tiny-sharp meets the absolute bound
G21_TOL = (1.2, 0.2)  # G21 (a), tiny-sharp over 520 positions against HF fp32: measured max 0.82, rms 0.14
RP_E_WORKSPACE = -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _model(cname: str, scale: str):
    cfg = synth.seq2seq_config(cname)
    sd = synth.synth_seq2seq_state_dict(cfg, scale=scale)
    return cfg, sd, HipT5Generator(cfg, sd, DEV)


def _padded(srcs, labels):
    S, T = max(len(s) for s in srcs), max(max(len(y) for y in labels), 1)
    ids = np.zeros((len(srcs), S), np.int64)
    mask = np.zeros((len(srcs), S), np.int64)
    y = np.full((len(srcs), T), -100, np.int64)
    for b, (s, l) in enumerate(zip(srcs, labels)):
        ids[b, : len(s)], mask[b, : len(s)], y[b, : len(l)] = s, 1, l
    return ids, mask, y


def _err(got, ref, keep):
    d = np.abs(got - ref)[keep]
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


@pytest.mark.parametrize("name,cname,scale", [("tiny", "tiny", "hf"), ("byt5-small", "byt5-small", "hf"),
                                              ("tiny-sharp", "tiny", "sharp")])
def test_forward_against_hf_g22(name, cname, scale):
    z = np.load(os.path.join(GOLDEN, "g22_seq2seq.npz"))
    _, _, gen = _model(cname, scale)
    k = f"{name}_mix"
    ids, mask, y = z[f"{k}_ids"].astype(np.int64), z[f"{k}_mask"].astype(np.int64), z[f"{k}_labels"].astype(np.int64)
    loss32, loss16 = z[f"{k}_loss"]
    loss = gen.forward(ids, mask, y)
    lp = gen.label_log_probs(ids, mask, y).cpu().numpy()
    keep = y != -100
    e = _err(lp, z[f"{k}_lp32"], keep)
    e16 = _err(z[f"{k}_lp16"], z[f"{k}_lp32"], keep)
    print(f"G22 {name}: |loss - fp32| {abs(loss - loss32):.2e} [HF-bf16 {abs(loss16 - loss32):.2e}]; label lp max / rms "
          f"{e[0]:.3e} / {e[1]:.3e} [HF-bf16 {e16[0]:.3e} / {e16[1]:.3e}]")
    # per-token: no further from fp32 than HF-bf16 (the step path's contract).  The loss: within HF-bf16's loss error or
    # 1e-3; at HF scale (only) also 4e-4 relative, where losses are 34 - 119 nats and HF-bf16's per-token errors (2-3x ours)
    # happen to cancel in its mean
    assert e[0] <= e16[0] and e[1] <= e16[1]
    rel = G22_LOSS_REL * abs(loss32) if scale == "hf" else 0.0
    assert abs(loss - loss32) <= max(abs(loss16 - loss32), 1e-3, rel)
    assert not lp[~keep].any()
    nz = z[f"{name}_none_ids"].astype(np.int64), z[f"{name}_none_mask"].astype(np.int64), z[f"{name}_none_labels"]
    assert np.isnan(gen.forward(*nz))


def test_forward_against_hf_g19_g21():
    """Per-token log-probs along the step tests' sources and targets: no further from HF fp32 than HF-bf16 (G19), and
    within the step path's margins on G21."""
    z = np.load(os.path.join(GOLDEN, "g19_decoder_step.npz"))
    for key, cname in (("tiny_0", "tiny"), ("tiny_1", "tiny"), ("byt5-small_0", "byt5-small")):
        _, _, gen = _model(cname, "hf")
        src, tgt = z[f"{key}_src"].astype(np.int64), z[f"{key}_tgt"].astype(np.int64)
        lab = np.concatenate([tgt[1:], [1]])  # decoder inputs are tgt (starts with 0): labels are tgt shifted left
        ids, mask, y = _padded([src], [lab])
        lp = gen.label_log_probs(ids, mask, y).cpu().numpy()[0]
        ref32 = z[f"{key}_lp32"][np.arange(len(lab)), lab]
        ref16 = z[f"{key}_lp16"][np.arange(len(lab)), lab]
        e, e16 = _err(lp, ref32, slice(None)), _err(ref16, ref32, slice(None))
        print(f"G19 {key}: max / rms {e[0]:.3e} / {e[1]:.3e} [HF-bf16 {e16[0]:.3e} / {e16[1]:.3e}]")
        assert e[0] <= max(e16[0], 2e-3) and e[1] <= max(e16[1], 1e-3)
    z = np.load(os.path.join(GOLDEN, "g21_decoder_long.npz"))
    import json

    meta = json.loads(bytes(z["meta"]).decode())
    name = "a"
    m = meta[name]
    _, _, gen = _model(m["config"], m["scale"])
    tgt = z[f"{name}_tgt"].astype(np.int64)
    ids, mask, y = _padded([z[f"{name}_src"].astype(np.int64)], [tgt[1:]])
    lp = gen.label_log_probs(ids, mask, y).cpu().numpy()[0]
    e = _err(lp, z[f"{name}_lp_label"], slice(None))
    print(f"G21 {name}: max / rms {e[0]:.3e} / {e[1]:.3e}")
    assert e[0] < G21_TOL[0] and e[1] < G21_TOL[1]


def _random_pairs(rng, B, src_range, tgt_range, long_tgt=()):
    srcs, labs = [], []
    for b in range(B):
        n = int(rng.integers(*src_range)) if b else 1
        srcs.append(source_ids(n, 500 + b).astype(np.int64))
        t = long_tgt[b] if b < len(long_tgt) else int(rng.integers(*tgt_range))
        labs.append(np.concatenate([rng.integers(3, 259, size=t - 1), [1]]).astype(np.int64))
    return srcs, labs


@pytest.mark.parametrize("cname,B,src_range,tgt_range,long_tgt", [
    ("tiny", 8, (2, 700), (1, 80), (1, 520, 300)),
    ("byt5-small", 64, (2, 2301), (1, 65), (1, 512, 2, 511, 300)),
])
def test_forward_against_float64_reference(cname, B, src_range, tgt_range, long_tgt):
    cfg, sd, gen = _model(cname, "sharp")
    rng = np.random.default_rng(7)
    srcs, labs = _random_pairs(rng, B, src_range, tgt_range, long_tgt)
    if cname == "byt5-small":
        srcs[1] = source_ids(2300, 77).astype(np.int64)
    ids, mask, y = _padded(srcs, labs)
    loss = gen.forward(ids, mask, y)
    lp = gen.label_log_probs(ids, mask, y).double()
    emu = T5ForwardEmu(cfg, sd, device=DEV)
    encs = [gen.encode_hidden_packed(s, np.array([0, len(s)], np.int32)) for s in srcs]
    ref_loss, ref = emu.forward(encs, y)
    keep = torch.from_numpy(y != -100).to(DEV)
    d = (lp - ref.to(DEV))[keep].abs()
    mx, rms = float(d.max()), float(d.pow(2).mean().sqrt())
    tol = FORWARD_TOL[f"{cname}-sharp"]
    print(f"{cname}-sharp B={B}: max {mx:.3e} rms {rms:.3e} (tolerance {tol}), |d loss| {abs(loss - ref_loss):.3e}")
    assert mx < tol[0] and rms < tol[1] and abs(loss - ref_loss) < tol[1]


def test_forward_against_step_loop():
    """A few short pairs through rp_decoder_step one token at a time: the same model, other reduction orders."""
    _, _, gen = _model("tiny", "sharp")
    rng = np.random.default_rng(3)
    srcs, labs = _random_pairs(rng, 3, (2, 400), (2, 40))
    ids, mask, y = _padded(srcs, labs)
    _, tgt_cu, _, rows = gen._teacher_forced(ids, mask, y, rows=True)
    worst = 0.0
    for b, (s, l) in enumerate(zip(srcs, labs)):
        enc = gen.encode_hidden(s)
        inp = np.concatenate([[0], l[:-1]])
        gen.decoder.start(enc, 1, len(inp))
        for t in range(len(inp)):
            step = gen.decoder.step(torch.tensor([int(inp[t])]), torch.arange(t + 1)[None])[0]
            worst = max(worst, float((step - rows[int(tgt_cu[b]) + t]).abs().max()))
    print(f"forward vs step loop: max |d log-prob| {worst:.3e} (tolerance {STEP_TOL})")
    assert worst < STEP_TOL


def test_same_bits_alone_batched_permuted():
    _, _, gen = _model("tiny", "sharp")
    rng = np.random.default_rng(11)
    srcs, labs = _random_pairs(rng, 6, (2, 900), (1, 300), (1, 260))
    ids, mask, y = _padded(srcs, labs)
    # the decode step's log-probs on this decoder, before and after forward calls
    enc = gen.encode_hidden(srcs[2])
    gen.decoder.start(enc, 1, 4)
    before = gen.decoder.step(torch.tensor([0]), torch.arange(1)[None]).clone()
    batched = gen.label_log_probs(ids, mask, y).cpu()
    loss = gen.forward(ids, mask, y)
    for _ in range(2):
        assert gen.forward(ids, mask, y) == loss
    for b in range(len(srcs)):
        alone = gen.label_log_probs(*_padded([srcs[b]], [labs[b]])).cpu()[0]
        n = len(labs[b])
        assert torch.equal(alone[:n], batched[b, :n]), b
    perm = rng.permutation(len(srcs))
    permuted = gen.label_log_probs(ids[perm], mask[perm], y[perm]).cpu()
    assert torch.equal(permuted, batched[perm])
    gen.decoder.start(enc, 1, 4)
    after = gen.decoder.step(torch.tensor([0]), torch.arange(1)[None])
    assert torch.equal(before, after)


def test_generate_scores_equal_label_log_prob_sums():
    _, _, gen = _model("tiny", "sharp")
    src = source_ids(300, 42).astype(np.int64)
    lp_pen = 1.0
    out = gen.generate(src, num_beams=4, max_length=24, length_penalty=lp_pen)
    labs = []
    for s in out.sequences.numpy():
        s = s[1:]
        end = np.nonzero(s == 1)[0]
        labs.append(s[: end[0] + 1] if len(end) else s)
    ids, mask, y = _padded([src] * len(labs), labs)
    lp = gen.label_log_probs(ids, mask, y).double().cpu()
    for j, l in enumerate(labs):
        score = float(lp[j, : len(l)].sum()) / len(l) ** lp_pen
        assert abs(score - float(out.sequences_scores[j])) < 0.05, (j, score, float(out.sequences_scores[j]))


def test_edge_cases_and_abi_errors():
    _, _, gen = _model("tiny", "hf")
    src = source_ids(30, 1).astype(np.int64)
    # B = 1, T = 1 (EOS only)
    ids, mask, y = _padded([src], [np.array([1])])
    lp = gen.label_log_probs(ids, mask, y)
    assert lp.shape == (1, 1) and float(lp[0, 0]) < 0 and abs(gen.forward(ids, mask, y) + float(lp[0, 0])) < 1e-6
    # all ignored: NaN, zeros
    ids, mask, y = _padded([src, src], [np.array([-100, -100]), np.array([-100])])
    assert np.isnan(gen.forward(ids, mask, y)) and not gen.label_log_probs(ids, mask, y).any()
    with pytest.raises(ValueError):
        gen.forward(ids, np.array([[0] + [1] * (ids.shape[1] - 1)] * 2), y)
    # over-limit shapes and inconsistent pairs through rp_last_error, never a fault
    lib, dec = gen.decoder._lib, gen.decoder._handle
    arr = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    pc = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for s_cu, t_cu, msg in (([0, 10], [0, 8193], "target 0"), ([0, 8193], [0, 4], "source 0"), ([0, 0], [0, 3], "empty source"),
                            ([1, 3], [0, 3], "start at 0")):
        s_cu, t_cu = arr(s_cu), arr(t_cu)
        assert lib.rp_decoder_forward_workspace_bytes(dec, pc(s_cu), pc(t_cu), 1) == 0
        sc = torch.empty(2, dtype=torch.float64, device=DEV)
        st = lib.rp_decoder_forward(dec, None, pc(s_cu), None, None, pc(t_cu), 1, None, sc.data_ptr(), None, None, 0,
                                    _lib.current_stream())
        assert st != _lib.RP_OK
        assert msg in lib.rp_last_error().decode(), lib.rp_last_error()
    # workspace too small
    s_cu, t_cu = arr([0, 10]), arr([0, 4])
    n = lib.rp_decoder_forward_workspace_bytes(dec, pc(s_cu), pc(t_cu), 1)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    sc = torch.empty(2, dtype=torch.float64, device=DEV)
    enc = torch.zeros((10, gen.cfg["d_model"]), dtype=torch.bfloat16, device=DEV)
    t = torch.zeros(4, dtype=torch.int32, device=DEV)
    lp = torch.empty(4, dtype=torch.float32, device=DEV)
    st = lib.rp_decoder_forward(dec, enc.data_ptr(), pc(s_cu), t.data_ptr(), t.data_ptr(), pc(t_cu), 1, lp.data_ptr(),
                                sc.data_ptr(), None, ws.data_ptr(), n - 1, _lib.current_stream())
    assert st == RP_E_WORKSPACE


def test_vocab_not_a_multiple_of_four():
    """V = 259: the logits epilogue stores the row's last group element by element.  Targets of 128 tokens in all put the
    last row at the end of the workspace; rows must match the decode step loop and the neighbours' first logits."""
    cfg = dict(synth.seq2seq_config("tiny"), vocab_size=259)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    gen = HipT5Generator(cfg, sd, DEV)
    rng = np.random.default_rng(5)
    srcs = [source_ids(90, 61).astype(np.int64), source_ids(300, 62).astype(np.int64)]
    labs = [np.concatenate([rng.integers(3, 259, size=99), [1]]), np.concatenate([rng.integers(3, 259, size=27), [1]])]
    ids, mask, y = _padded(srcs, labs)
    _, tgt_cu, _, rows = gen._teacher_forced(ids, mask, y, rows=True)
    assert int(tgt_cu[-1]) == 128
    worst = 0.0
    for b, (s, l) in enumerate(zip(srcs, labs)):
        gen.decoder.start(gen.encode_hidden(s), 1, len(l))
        inp = np.concatenate([[0], l[:-1]])
        for t in range(len(inp)):
            step = gen.decoder.step(torch.tensor([int(inp[t])]), torch.arange(t + 1)[None])[0]
            worst = max(worst, float((step - rows[int(tgt_cu[b]) + t]).abs().max()))
    print(f"V = 259, forward vs step loop: max |d log-prob| {worst:.3e}")
    assert worst < STEP_TOL
    with pytest.raises(ValueError):
        gen.forward(ids, mask, np.where(y == 1, 259, y))
