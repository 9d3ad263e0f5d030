"""The tactic generator's HIP decoder against the bf16-emulating float64 reference (tests/gen_helpers.py T5DecodeEmu)
at the shapes the prover runs: teacher-forced and ancestry-driven runs up to 512 positions, 64 beams, 2047 / 2048-byte
and 1-byte sources, the sharp weight family, the tied and the transformers-5 (scale_decoder_outputs=False) heads, the
RP_DT_BF16 create path, decoder reuse across shapes, rp_beam_select over a vocab / beam / k sweep, rp_encode_hidden over
source lengths, and generate at prover shape.

Tolerances (DECODER_TOL) are measured MI355X margins with headroom; tests/test_decoder_ref_cpu.py shows how far each
planted reference bug moves the log-probs beyond them."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import (DECODER_TOL, ENCODER_TOL, SELECT_SPREAD, T5DecodeEmu, simulated_search,  # noqa: E402
                         source_ids)
from oracle import t5_ref  # noqa: E402
from oracle.parity_margins import gap_rule_ids  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import _DEC_KEYS, HipT5Decoder, HipT5Generator  # noqa: E402
from reprover_amd.generation import beam_search  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _model(cname: str, scale: str, scale_decoder_outputs=None):
    cfg = synth.seq2seq_config(cname)
    if scale_decoder_outputs is not None:
        cfg["scale_decoder_outputs"] = scale_decoder_outputs
    sd = synth.synth_seq2seq_state_dict(cfg, scale=scale)
    return cfg, sd, HipT5Generator(cfg, sd, DEV), T5DecodeEmu(cfg, sd, device=DEV)


def _compare(gen, emu, enc, nb, max_len, runs, select=False, seed=0, spread=0.0):
    """Run the HIP step and the reference in lockstep over ``runs`` (tuples (t, tokens, ancestry)).  Returns (max error
    per step, rms over all, and with ``select``: the max error on the reference's top-2nb candidates of log-probs +
    running scores, and the gap-rule (checked, mismatched) of the device selection against that top-2nb)."""
    gen.decoder.start(enc, nb, max_len)
    emu.start(enc, nb, max_len)
    rng = np.random.default_rng(seed)
    step_max, sq, n, cand, sel = [], torch.zeros((), dtype=torch.float64, device=DEV), 0, [], [0, 0]
    for t, tok, anc in runs:
        got = gen.decoder.step(tok, anc).double()
        ref = emu.step(tok, anc)
        d = (got - ref).abs()
        step_max.append(d.max())
        sq += d.pow(2).sum()
        n += d.numel()
        if select:
            # running scores ``spread`` apart: the top-2nb candidates mix many rows
            run = torch.from_numpy(-spread * (np.arange(nb) + rng.uniform(0, 1, nb))).float()
            k = 2 * nb
            rs, ri = torch.sort((ref + run.to(DEV).double()[:, None]).reshape(-1), descending=True, stable=True)
            cand.append(d.reshape(-1)[ri[:k]].max())
            s, tk, par = gen.decoder.select(got.float(), run, k)
            ours = (par.long() * ref.shape[1] + tk.long()).cpu().numpy()
            c, b = gap_rule_ids([ours], [ri[:k].cpu().numpy()], [rs[:k].cpu().numpy()], select)
            sel = [sel[0] + c, sel[1] + b]
    cand_max = float(torch.stack(cand).max()) if cand else None
    return torch.stack(step_max).cpu().numpy(), float((sq / n).sqrt()), cand_max, tuple(sel)


def _teacher(target):
    for t in range(len(target)):
        yield t, torch.tensor([int(target[t])]), torch.arange(t + 1)[None]


def _check(case, step_max, rms, cand=None, sel=None):
    tol = DECODER_TOL[case]
    print(f"decoder parity {case}: max |d lp| {step_max.max():.3e} (step {int(step_max.argmax())}), rms {rms:.3e}; "
          f"tol {tol[0]:.1e} / {tol[1]:.1e}" +
          (f"; top-2nb candidates max |d| {cand:.3e} (tol {tol[2]:.1e}), selection gap-rule ranks {sel[0]} checked / "
           f"{sel[1]} mismatched" if sel else ""))
    assert step_max.max() <= tol[0], (case, step_max.max(), int(step_max.argmax()))
    assert rms <= tol[1], (case, rms)
    if sel is not None:
        assert cand <= tol[2], (case, cand)
        assert sel[0] > 0 and sel[1] == 0, (case, sel)


G21 = "g21_decoder_long.npz"


def test_tiny_sharp_teacher_forced_520(golden_dir):
    """One beam along G21(a)'s 520-position target; max_len = 520 so the last step is t = max_len - 1."""
    g = np.load(os.path.join(golden_dir, G21))
    cfg, sd, gen, emu = _model("tiny", "sharp")
    tgt = g["a_tgt"][:-1]
    enc = gen.encode_hidden(g["a_src"])
    step_max, rms, _, _ = _compare(gen, emu, enc, 1, len(tgt), _teacher(tgt))
    _check("tiny-sharp/nb1", step_max, rms)
    assert len(step_max) == 520


@pytest.mark.parametrize("nb,steps,max_len,src", [(3, 512, 4096, 300), (64, 512, 512, 700), (3, 64, 64, 1)])
def test_tiny_sharp_ancestry(nb, steps, max_len, src):
    """Simulated searches with repeated parents; max_len far above the steps, or equal to them (t = max_len - 1); a
    1-byte source."""
    cfg, sd, gen, emu = _model("tiny", "sharp")
    enc = gen.encode_hidden(source_ids(src, 40 + nb))
    case = f"tiny-sharp/nb{nb}" + ("/src1" if src == 1 else "")
    step_max, rms, cand, sel = _compare(gen, emu, enc, nb, max_len, simulated_search(nb, steps, 100 + nb),
                                        select=DECODER_TOL[case][2], seed=nb, spread=SELECT_SPREAD["tiny-sharp"])
    _check(case, step_max, rms, cand, sel)


@pytest.mark.parametrize("nb,steps,src", [(64, 300, 2048), (8, 512, 2047)])
def test_byt5_small_sharp_ancestry(nb, steps, src):
    cfg, sd, gen, emu = _model("byt5-small", "sharp")
    enc = gen.encode_hidden(source_ids(src, 50 + nb))
    case = f"byt5-small-sharp/nb{nb}"
    step_max, rms, cand, sel = _compare(gen, emu, enc, nb, steps, simulated_search(nb, steps, 200 + nb),
                                        select=DECODER_TOL[case][2], seed=nb, spread=SELECT_SPREAD["byt5-small-sharp"])
    _check(case, step_max, rms, cand, sel)


def test_tiny_tied_ancestry(golden_dir):
    g = np.load(os.path.join(golden_dir, G21))
    cfg, sd, gen, emu = _model("tiny-tied", "hf")
    enc = gen.encode_hidden(g["b_src"])
    step_max, rms, cand, sel = _compare(gen, emu, enc, 4, 200, simulated_search(4, 160, 7),
                                        select=DECODER_TOL["tiny-tied"][2], seed=4,
                                        spread=SELECT_SPREAD["tiny-tied"])
    _check("tiny-tied", step_max, rms, cand, sel)


def _save_dir(path, cfg, sd, hf_extra):
    os.makedirs(path, exist_ok=True)
    hf = dict(model_type="t5", is_encoder_decoder=True, decoder_start_token_id=0, eos_token_id=1,
              **{k: cfg[k] for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                     "num_decoder_layers", "relative_attention_num_buckets",
                                     "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj")},
              **hf_extra)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(hf, fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items() if "embed_tokens" not in k},
              os.path.join(path, "model.safetensors"))


@pytest.mark.parametrize("name,hf_extra", [("b", dict(tie_word_embeddings=True)),
                                           ("c", dict(tie_word_embeddings=True, scale_decoder_outputs=False))])
def test_checkpoint_heads_against_g21(golden_dir, tmp_path, name, hf_extra):
    """G21(b) (tied, transformers-4 config) and G21(c) (transformers-5 config: lm_head = shared, no d_model^-0.5) loaded
    from a checkpoint directory: teacher-forced log-probs against HF fp32 and against the reference."""
    g = np.load(os.path.join(golden_dir, G21))
    cfg = synth.seq2seq_config("tiny-tied")
    sd = synth.synth_seq2seq_state_dict(cfg)
    _save_dir(str(tmp_path), cfg, sd, hf_extra)
    gen = HipT5Generator.from_pretrained(str(tmp_path), DEV)
    emu = T5DecodeEmu(gen.cfg, sd, device=DEV)
    tgt = g[f"{name}_tgt"]
    T = len(tgt) - 1
    enc = gen.encode_hidden(g[f"{name}_src"])
    step_max, rms, _, _ = _compare(gen, emu, enc, 1, T, _teacher(tgt[:T]))
    _check(f"g21{name}", step_max, rms)
    gen.decoder.start(enc, 1, T)
    lp = torch.stack([gen.decoder.step(tok, anc)[0] for _, tok, anc in _teacher(tgt[:T])]).double().cpu()
    lab = lp[torch.arange(T), torch.from_numpy(tgt[1:].astype(np.int64))].numpy()
    d_lab = np.abs(lab - g[f"{name}_lp_label"]).max()
    d_rows = np.abs(lp[g[f"{name}_rows"]].numpy() - g[f"{name}_lp_rows"]).max()
    print(f"decoder vs HF fp32 G21({name}): label max {d_lab:.3e}, rows max {d_rows:.3e}")
    assert max(d_lab, d_rows) <= DECODER_TOL[f"g21{name}/hf"][0], (d_lab, d_rows)


def _bf16_decoder(cfg, sd_bf16):
    """A decoder created through rp_decoder_create(RP_DT_BF16) from bf16 weights, wrapped as a HipT5Decoder."""
    lib = _lib.load()
    L = cfg["num_decoder_layers"]
    c = _lib.RpT5Config(cfg["vocab_size"], cfg["d_model"], cfg["d_kv"], cfg["num_heads"], cfg["d_ff"], L,
                        cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"],
                        float(cfg["layer_norm_epsilon"]))
    keep = {k: v.to(DEV).contiguous() for k, v in sd_bf16.items()}
    layers = (_lib.RpT5DecoderLayerWeights * L)()
    for i in range(L):
        for fld, key in _DEC_KEYS.items():
            setattr(layers[i], fld, keep[f"decoder.block.{i}.{key}"].data_ptr())
    w = _lib.RpT5DecoderWeights(keep["shared.weight"].data_ptr(),
                                keep["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].data_ptr(),
                                keep["decoder.final_layer_norm.weight"].data_ptr(), keep["lm_head.weight"].data_ptr(),
                                layers, 0)
    handle = C.c_void_p()
    torch.cuda.synchronize()
    _lib.check(lib.rp_decoder_create(C.byref(c), C.byref(w), _lib.RP_DT_BF16, C.byref(handle)), "rp_decoder_create(bf16)")
    return HipT5Decoder.from_handle(lib, handle, cfg, DEV)


def _steps(dec, enc, nb, max_len, steps, seed):
    dec.start(enc, nb, max_len)
    return [dec.step(tok, anc).clone().cpu() for _, tok, anc in simulated_search(nb, steps, seed)]


def test_bf16_create_path_same_bits():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd.items() if k.startswith("decoder.") or k in ("shared.weight",
                                                                                                   "lm_head.weight")}
    ref = HipT5Decoder(cfg, {k: v.float() for k, v in sd16.items()}, DEV)
    dec = _bf16_decoder(cfg, sd16)
    enc = _model("tiny", "sharp")[2].encode_hidden(source_ids(300, 3))
    for a, b in zip(_steps(ref, enc, 5, 300, 260, 9), _steps(dec, enc, 5, 300, 260, 9)):
        assert torch.equal(a, b)


def test_decoder_reuse_across_shapes_same_bits():
    """One decoder driven big -> small -> big (beams, max_len, source) gives the bits of a fresh decoder each time."""
    cfg, sd, gen, _ = _model("tiny", "sharp")
    shapes = [(64, 300, 700, 280), (2, 20, 1, 20), (33, 400, 2048, 270)]
    encs = {S: gen.encode_hidden(source_ids(S, S)) for _, _, S, _ in shapes}
    shared = HipT5Decoder(cfg, sd, DEV)
    for nb, max_len, S, steps in shapes:
        got = _steps(shared, encs[S], nb, max_len, steps, nb)
        fresh = _steps(HipT5Decoder(cfg, sd, DEV), encs[S], nb, max_len, steps, nb)
        assert all(torch.equal(a, b) for a, b in zip(got, fresh)), (nb, max_len, S)


# ---- rp_beam_select ---------------------------------------------------------------------------------------------------

def _selector():
    return HipT5Decoder.from_handle(_lib.load(), None, None, DEV)


def _select_data(kind, nb, V, g):
    if kind == "quantised":  # few levels: ties inside rows, across rows and across the row -> merge boundary
        lp = torch.randint(-3, 1, (nb, V), generator=g).float() * 0.5
        run = torch.randint(-1, 1, (nb,), generator=g).float() * 0.5
    elif kind == "neg_inf":
        lp = torch.randn(nb, V, generator=g)
        lp[torch.rand(nb, V, generator=g) < 0.6] = -float("inf")
        run = torch.randn(nb, generator=g)
    elif kind == "running_neg1e9":  # HF's first step: rows 1.. at -1e9 collapse to exact ties
        lp = torch.log_softmax(torch.randn(nb, V, generator=g) * 3, -1)
        run = torch.zeros(nb)
        run[1:] = -1e9
    else:  # signed zeros
        lp = torch.tensor([0.0, -0.0, -1.0])[torch.randint(0, 3, (nb, V), generator=g)]
        run = torch.tensor([0.0, -0.0])[torch.randint(0, 2, (nb,), generator=g)]
    return lp, run


SEL_NB = (1, 2, 3, 5, 31, 32, 33, 63, 64)
SEL_V = (1, 2, 7, 100, 127, 128, 129, 255, 256, 257, 384, 511, 512)


@pytest.mark.parametrize("kind", ["quantised", "neg_inf", "running_neg1e9", "signed_zero"])
def test_beam_select_sweep_equals_stable_sort(kind):
    """rp_beam_select against torch.sort(stable=True) on the same fp32 sums: scores, tokens and parents exactly equal."""
    sel = _selector()
    g = torch.Generator().manual_seed(len(kind))
    n = 0
    for nb in SEL_NB:
        for V in SEL_V:
            lp, run = _select_data(kind, nb, V, g)
            acc = (lp.to(DEV) + run.to(DEV)[:, None]).reshape(-1).cpu()  # the sums the device forms
            rs, ri = torch.sort(acc, descending=True, stable=True)
            for k in sorted({1, nb, 2 * nb, min(128, nb * V)}):
                if k > min(128, nb * V):
                    continue
                s, t, p = sel.select(lp.to(DEV), run.to(DEV), k)
                assert torch.equal(s.cpu(), rs[:k]), (kind, nb, V, k)
                assert torch.equal(t.cpu().long(), ri[:k] % V), (kind, nb, V, k)
                assert torch.equal(p.cpu().long(), ri[:k] // V), (kind, nb, V, k)
                n += 1
    assert n >= 400


# ---- rp_encode_hidden -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname", ["tiny", "byt5-small"])
def test_encode_hidden_lengths_elementwise(cname):
    """|hidden - fp32 reference| <= a |ref| + b element-wise over source lengths 1 .. 2048 (ENCODER_TOL), on HF-scale
    weights (where bf16 keeps the encoder within cosine 0.9999 of fp32).  Teeth: the reference with its last key
    masked out (a dropped key) breaks the bound on the rows before it, at every length from 2 to 300."""
    cfg, sd, gen, _ = _model(cname, "hf")
    a, b = ENCODER_TOL[cname]
    use, teeth = {}, {}
    for S in (1, 2, 63, 64, 65, 300, 2047, 2048):
        src = source_ids(S, 60 + S)
        ids = src[None].astype(np.int64)
        hid = gen.encode_hidden(src).double().cpu()
        ref = t5_ref._encoder_forward(cfg, sd, ids, np.ones((1, S), np.int64))[0].double()
        use[S] = ((hid - ref).abs() / (a * ref.abs() + b)).max().item()
        if 2 <= S <= 300:
            mask = np.ones((1, S), np.int64)
            mask[0, -1] = 0
            mut = t5_ref._encoder_forward(cfg, sd, ids, mask)[0].double()[: S - 1]
            teeth[S] = ((mut - ref[: S - 1]).abs() / (a * ref[: S - 1].abs() + b)).max().item()
        need = ((hid - ref).abs() - a * ref.abs()).max().item()
        print(f"encode_hidden {cname} S={S}: max |d| {(hid - ref).abs().max():.3e}, b needed {need:.2e}, bound use "
              f"{use[S]:.2f}" + (f", last-key-dropped reference uses {teeth[S]:.1f}x the bound" if S in teeth else ""))
    assert max(use.values()) <= 1.0, (cname, use)
    assert min(teeth.values()) > 1.0, (cname, teeth)


# ---- generate at prover shape -----------------------------------------------------------------------------------------

def _hypotheses(trace, nb, eos=1):
    """Per step of a beam-search trace: the candidates as prefix hashes in rank order, their scores, and the running
    hypotheses {prefix: score} that generation.beam_search keeps (the top nb candidates not ending in EOS)."""
    seqs = [(0,)] * nb
    for vals, toks, parents in trace:
        cand = [seqs[int(p)] + (int(t),) for p, t in zip(parents, toks)]
        run_lp = vals + (toks == eos).float() * -1.0e9
        nxt = torch.topk(run_lp, k=nb)[1].tolist()
        seqs = [cand[i] for i in nxt]
        yield dict(cand=[hash(c) for c in cand], scores=vals.double().numpy(),
                   running={cand[i]: float(run_lp[i]) for i in nxt})


def _strip(seq):
    seq = list(seq)
    return seq[: seq.index(1, 1) + 1] if 1 in seq[1:] else seq


def test_generate_prover_shape_against_reference():
    """ByT5-small-sharp, 64 beams, max_length 128, a 2048-byte source, length_penalty 0 (the prover's call).

    1. HIP generate with the reference evaluated on every step's own (tokens, ancestry): the device selection agrees with
       the reference's top-2nb at every rank the gap rule covers, on every step.
    2. Every returned HIP sequence, rescored by the reference, matches its sequences_scores.
    3. HIP generate and the host beam search over the reference: while they hold the same running hypotheses, their
       candidates agree at every gap-rule rank (tol: the candidate tolerance, times the step count for the running
       sums).  At this shape the reference's top-128 has gaps far below the candidate error, so the searches part early:
       the count is printed, not asserted; checks 1 and 2 carry the weight."""
    cfg, sd, gen, emu = _model("byt5-small", "sharp")
    tol = sel_tol = DECODER_TOL["byt5-small-sharp/nb64"][2]
    src = source_ids(2048, 66)
    nb, ml = 64, 128
    enc = gen.encode_hidden(src)
    dec = gen.decoder
    seen = {"checked": 0, "bad": 0, "steps": 0}

    def step(tokens, ancestry):
        if ancestry.shape[1] == 1:
            emu.start(enc, nb, ml)
        seen["ref"] = emu.step(tokens, ancestry)
        return type(dec).step(dec, tokens, ancestry)

    def select(lp, running, k):
        s, t, p = type(dec).select(dec, lp, running, k)
        rs, ri = torch.sort((seen["ref"] + running.double()[:, None]).reshape(-1), descending=True, stable=True)
        ours = (p.long() * lp.shape[1] + t.long()).cpu().numpy()
        c, b = gap_rule_ids([ours], [ri[:k].cpu().numpy()], [rs[:k].cpu().numpy()], sel_tol)
        seen["checked"], seen["bad"], seen["steps"] = seen["checked"] + c, seen["bad"] + b, seen["steps"] + 1
        return s, t, p

    dec.step, dec.select = step, select
    trace = []
    try:
        out = gen.generate(src, nb, ml, 0.0, trace=trace)
    finally:
        del dec.step, dec.select
    counts = {k: seen[k] for k in ("steps", "checked", "bad")}
    assert counts["steps"] == len(trace) and counts["checked"] > 0 and counts["bad"] == 0, counts

    emu.start(enc, nb, ml)
    rtrace = []
    beam_search(emu.step, nb, ml, 0.0, device=DEV, trace=rtrace)
    # the two searches hold the same running hypotheses (prefix -> score, slot order aside) until a candidate crosses the
    # rank-nb boundary differently; on each such step the candidates (as prefixes) must agree at every gap-rule rank
    compared = checked = 0
    for s, (h, r) in enumerate(zip(_hypotheses(trace, nb), _hypotheses(rtrace, nb))):
        c, b = gap_rule_ids([h["cand"]], [r["cand"]], [r["scores"]], tol * (s + 1))
        assert b == 0, s
        checked += c
        if h["running"].keys() != r["running"].keys():
            break
        assert max(abs(h["running"][k] - r["running"][k]) for k in r["running"]) <= tol * (s + 1), s
        compared += 1
    # rescoring: every returned sequence teacher-forced through the reference in one 64-row batch
    seqs = [_strip(r.tolist()) for r in out.sequences]
    T = max(len(q) for q in seqs) - 1
    emu.start(enc, nb, T)
    pad = torch.tensor([q + [1] * (T + 1 - len(q)) for q in seqs])
    total = torch.zeros(nb, dtype=torch.float64)
    for t in range(T):
        anc = torch.arange(t + 1)[None] * nb + torch.arange(nb)[:, None]
        lp = emu.step(pad[:, t], anc).cpu()
        live = torch.tensor([t + 1 < len(q) for q in seqs])
        total += torch.where(live, lp[torch.arange(nb), pad[:, t + 1]], torch.zeros(nb, dtype=torch.float64))
    d = (total - out.sequences_scores.double()).abs()
    gaps = [float((rs[:-1] - rs[1:]).min()) for rs, _, _ in rtrace[:4]]
    print(f"generate prover shape: {len(trace)} steps; selection along the HIP search: gap-rule ranks {seen['checked']} "
          f"checked / {seen['bad']} mismatched; {compared} steps of the reference search compared "
          f"({checked} gap-rule ranks; its first min gaps {gaps}); rescored sequences max |d score| {d.max():.3e} (lengths {min(map(len, seqs))}-{max(map(len, seqs))})")
    assert checked > 0, (compared, checked)
    assert d.max() <= DECODER_TOL["generate/rescore"][0], d.max()
