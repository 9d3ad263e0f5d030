"""Time the teacher-forced seq2seq forward (rp_decoder_forward) at the reference's generator-validation shape.

ByT5-small (synthetic weights), B pairs with sources of --src-bytes bytes and targets of each --tgt length.  Reports the
encoder pass (rp_encode_hidden over the B sources) and the decoder side (cross K/V, layers, loss: one rp_decoder_forward)
separately, the decoder side's GEMM FLOPs over its whole pass time (a lower bound of the GEMMs' own rate: the pass also
holds attention, norms, the loss and the metadata copy), and the same pairs' per-token cost through the rp_decoder_step loop
(a few pairs and positions only).  Prints one JSON object; --out also writes it.

    python tools/seq2seq_bench.py [--batch 64] [--src-bytes 2300] [--tgt 64 512] [--iters 5] [--out FILE]

--grad times the loss with its gradients (rp_decoder_loss_grad) instead: at the same shapes
rp_decoder_forward and rp_decoder_loss_grad alternate in one process, and the result holds both medians and their ratio.

    python tools/seq2seq_bench.py --grad --out profiles/seq2seq_grad_bench.json

--full-grad times the whole model's gradient (HipSeq2SeqGradients) at the reference's training
batch (generation/confs/cli_lean4_random.yaml: batch 8, 2300-byte sources, 512-label targets): the full call and the
decoder-only HipT5Generator.loss_and_grads alternate in one process; a separate profiled pass (rp_profile_read) gives the two
head kernels' times, turned into bytes/s from the bytes their shapes need.  No threshold: figures only.

    python tools/seq2seq_bench.py --full-grad --out profiles/seq2seq_full_grad_bench.json

--step times the whole training step (HipSeq2SeqTrainer: the same gradient, then AdamW over both halves and the re-packing
of every compute copy) at the same batch: the full step and the --full-grad call alternate in one
process, median of --iters (9), host clock around synchronised calls.  Separate profiled passes (rp_profile_read) give the
RP_K_OPTIMIZER class of one step and rp_decoder_load_params alone, the latter turned into bytes/s from the bytes its table
moves.  No threshold: figures only.

    python tools/seq2seq_bench.py --step --iters 9 --out profiles/seq2seq_train_bench.json

--step --dropout P prices T5's dropout instead: two HipSeq2SeqTrainer of the same weights, one at
p = 0 and one at p = P, alternate in one process at the same batch; the result holds both medians, their ratio and, from
one profiled step of each (rp_profile_read), the time per kernel class, which says where the masks' share goes.

    python tools/seq2seq_bench.py --step --dropout 0.1 --iters 9 --out profiles/seq2seq_dropout_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reprover_amd import synth  # noqa: E402
from reprover_amd import _lib  # noqa: E402
from reprover_amd.decoder import HipSeq2SeqGradients, HipT5Generator, shift_and_segment  # noqa: E402

HBM_PEAK = 8.0e12       # MI355X HBM3E, bytes/s (spec)
HBM_MEASURED = 6.29e12  # a float4 copy on the same part: the achievable ceiling


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _source(n, seed):
    text = synth.synth_text(np.random.default_rng(seed), n + 8)
    ids = np.frombuffer(text.encode("utf-8"), dtype=np.uint8).astype(np.int32)[: n - 1] + 3
    return np.concatenate([ids, [1]]).astype(np.int32)


def _grad_leg(a, gen, enc, src_cu, rng):
    B, S = a.batch, a.src_bytes
    result = dict(metric="seq2seq_grad_bench", measured=True, model="byt5-small (synthetic, sharp)", batch=B, source_bytes=S,
                  targets={})
    grads = torch.zeros(int(gen.decoder.grad_layout()[1][-1]), dtype=torch.float32, device=enc.device)
    for T in a.tgt:
        y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)
        tokens, labels, tgt_cu = shift_and_segment(y)
        fwd = lambda: gen.decoder.forward(enc, src_cu, tokens, labels, tgt_cu)  # noqa: E731
        bwd = lambda: gen.decoder.loss_grad(enc, src_cu, tokens, labels, tgt_cu, True, grads)  # noqa: E731
        fwd(), bwd()
        torch.cuda.synchronize()
        ts = {"f": [], "g": []}
        for _ in range(a.iters):  # alternating: both see the same clocks and the same neighbours
            for k, fn in (("f", fwd), ("g", bwd)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1))
        f_ms, g_ms = float(np.median(ts["f"])), float(np.median(ts["g"]))
        result["targets"][str(T)] = dict(forward_ms=round(f_ms, 3), loss_grad_ms=round(g_ms, 3),
                                         ratio=round(g_ms / f_ms, 3), forward_ms_all=[round(x, 3) for x in ts["f"]],
                                         loss_grad_ms_all=[round(x, 3) for x in ts["g"]])
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def _full_grad_leg(a, dev):
    B, S, T = 8, 2300, 512
    cfg = synth.seq2seq_config("byt5-small")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    full, dec_only = HipSeq2SeqGradients(cfg, sd, dev), HipT5Generator(cfg, sd, dev)
    rng = np.random.default_rng(0)
    ids = np.stack([_source(S, 100 + b) for b in range(B)]).astype(np.int64)
    mask = np.ones_like(ids)
    y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)
    legs = (("full", lambda: full.loss_and_grads(ids, mask, y)), ("decoder_only", lambda: dec_only.loss_and_grads(ids, mask, y)))
    for _ in range(2):  # warm-up of every shape the timed window uses
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _ in legs}
    for _ in range(a.iters):  # alternating: both see the same clocks and the same neighbours
        for k, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # ends in a device-to-host copy of the loss sums: host clock around synchronised work
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    f_ms, d_ms = float(np.median(ts["full"])), float(np.median(ts["decoder_only"]))
    # the encoder's share: the full call's forward_hidden + backward_hidden against the decoder-only call's inference pass
    _lib.profile_enable(True)
    legs[0][1]()
    torch.cuda.synchronize()
    prof = _lib.profile_read(heads=True)
    _lib.profile_enable(False)
    Tn, D = B * S, cfg["d_model"]
    heads = {}
    for name, nbytes in (("hidden_head", Tn * D * (2 + 2 + 2)), ("bwd_hidden_head", Tn * D * (2 + 2 + 4 + 2 + 2))):
        ms, n = prof[name]
        rate = nbytes / (ms * 1e-3) if ms > 0 else float("nan")
        heads[name] = dict(ms=round(ms, 4), launches=int(n), bytes=int(nbytes), tb_per_s=round(rate / 1e12, 3),
                           of_hbm_peak=round(rate / HBM_PEAK, 3), of_measured_copy_rate=round(rate / HBM_MEASURED, 3))
    result = dict(metric="seq2seq_full_grad_bench", measured=True, model="byt5-small (synthetic, hf)", batch=B, source_bytes=S,
                  target_labels=T, source_tokens=Tn, iters=a.iters, full_ms=round(f_ms, 3), decoder_only_ms=round(d_ms, 3),
                  encoder_backward_share=round((f_ms - d_ms) / f_ms, 4), full_ms_per_1k_source_tokens=round(f_ms / Tn * 1e3, 3),
                  full_ms_all=[round(x, 3) for x in ts["full"]], decoder_only_ms_all=[round(x, 3) for x in ts["decoder_only"]],
                  head_kernels=heads,
                  profiled_pass_ms_by_class={k: round(v[0], 3) for k, v in prof.items() if v[1]},
                  note="full = trainer forward with saved activations + decoder loss_grad + encoder backward + the shared sum; "
                       "decoder_only = inference encoder pass + decoder loss_grad; encoder_backward_share = what the full call "
                       "adds over it; head kernel rates = bytes their shapes need (both planes, d_hidden, outputs) / profiled time")
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def reload_bytes(cfg, tied):
    """bytes rp_decoder_load_params reads + writes: 4 B read per master element and table entry, 2 B written per bf16 copy
    (4 B for the FFN-in tensors, which have a second, interleaved copy), 4 B per fp32 copy"""
    D, F, V, L, H = cfg["d_model"], cfg["d_ff"], cfg["vocab_size"], cfg["num_decoder_layers"], cfg["num_heads"]
    ID = H * cfg["d_kv"] * D
    nbias = 2 * cfg.get("relative_attention_max_distance", 128) + 1
    il = 2 if F % 32 == 0 else 0
    total = V * D * (4 + 4) + V * D * (4 + 2) + H * nbias * (4 + 4 + 4) + D * 8
    total += L * (3 * D * 8 + 8 * ID * 6 + 2 * F * D * (6 + il) + F * D * 6)
    return total


def _step_dropout_leg(a, dev):
    from reprover_amd.seq2seq_train import HipSeq2SeqTrainer

    B, S, T = 8, 2300, 512
    cfg = synth.seq2seq_config("byt5-small")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    make = lambda p: HipSeq2SeqTrainer(cfg, sd, dev, lr=5e-4, warmup_steps=2000, dropout_rate=p, dropout_seed=7)  # noqa: E731
    trainers = {"p0": make(0.0), "dropout": make(a.dropout)}
    rng = np.random.default_rng(0)
    ids = np.stack([_source(S, 100 + b) for b in range(B)]).astype(np.int64)
    mask = np.ones_like(ids)
    y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)

    def step(tr):
        tr.loss_and_grads(ids, mask, y)
        tr.optimizer_step()

    for _ in range(2):
        for tr in trainers.values():
            step(tr)
    torch.cuda.synchronize()
    ts = {k: [] for k in trainers}
    for _ in range(a.iters):  # alternating: both see the same clocks and the same neighbours
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(tr)
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    prof = {}
    for k, tr in trainers.items():  # one profiled step each (events around every launch group: slower host, classes apart)
        _lib.profile_enable(True)
        step(tr)
        torch.cuda.synchronize()
        prof[k] = {c: round(v[0], 3) for c, v in _lib.profile_read(heads=True).items() if v[1]}
        _lib.profile_enable(False)
    result = dict(metric="seq2seq_dropout_bench", measured=True, model="byt5-small (synthetic, hf)", batch=B, source_bytes=S,
                  target_labels=T, iters=a.iters, dropout_rate=a.dropout, step_ms_p0=round(med["p0"], 3),
                  step_ms_dropout=round(med["dropout"], 3), dropout_over_p0=round(med["dropout"] / med["p0"], 4),
                  step_ms_p0_all=[round(x, 3) for x in ts["p0"]], step_ms_dropout_all=[round(x, 3) for x in ts["dropout"]],
                  profiled_step_ms_by_class_p0=prof["p0"], profiled_step_ms_by_class_dropout=prof["dropout"],
                  profiled_class_difference_ms={c: round(prof["dropout"].get(c, 0.0) - prof["p0"].get(c, 0.0), 3)
                                                for c in sorted(set(prof["p0"]) | set(prof["dropout"]))},
                  note="step = HipSeq2SeqTrainer.loss_and_grads + optimizer_step, median of iters alternating calls, host clock "
                       "around synchronised calls; the class split is one profiled step of each trainer (decoder row kernels "
                       "and attention launches carry no class of their own); one box, one run")
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def _step_leg(a, dev):
    from reprover_amd.seq2seq_train import HipSeq2SeqTrainer

    B, S, T = 8, 2300, 512
    cfg = synth.seq2seq_config("byt5-small")
    sd = synth.synth_seq2seq_state_dict(cfg, scale="hf")
    trainer = HipSeq2SeqTrainer(cfg, sd, dev, lr=5e-4, warmup_steps=2000)  # the reference's generator config
    grad_only = HipSeq2SeqGradients(cfg, sd, dev)
    rng = np.random.default_rng(0)
    ids = np.stack([_source(S, 100 + b) for b in range(B)]).astype(np.int64)
    mask = np.ones_like(ids)
    y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)

    def step():
        trainer.loss_and_grads(ids, mask, y)
        trainer.optimizer_step()

    legs = (("step", step), ("full_grad", lambda: grad_only.loss_and_grads(ids, mask, y)))
    for _ in range(2):  # warm-up of every shape the timed window uses
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _ in legs}
    for _ in range(a.iters):  # alternating: both see the same clocks and the same neighbours
        for k, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    s_ms, g_ms = float(np.median(ts["step"])), float(np.median(ts["full_grad"]))
    # the optimizer end alone, unprofiled: device events around back-to-back calls
    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    reload_ms = events(lambda: trainer.decoder.load_params(trainer.dec_params), 20)
    opt_ms = events(trainer.optimizer_step, 5)
    # profiled passes (events around every launch group: slower host, kernel classes apart)
    _lib.profile_enable(True)
    step()
    torch.cuda.synchronize()
    prof = _lib.profile_read(heads=True)
    _lib.profile_enable(False)
    _lib.profile_enable(True)
    for _ in range(10):
        trainer.decoder.load_params(trainer.dec_params)
    torch.cuda.synchronize()
    rl_ms, rl_n = _lib.profile_read()["optimizer"]
    _lib.profile_enable(False)
    nbytes = reload_bytes(cfg, trainer.tied)

    def rate(ms):
        r = nbytes / (ms * 1e-3) if ms > 0 else float("nan")
        return dict(ms=round(ms, 4), tb_per_s=round(r / 1e12, 3), of_hbm_peak=round(r / HBM_PEAK, 3),
                    of_measured_copy_rate=round(r / HBM_MEASURED, 3))

    n_enc, n_dec = trainer.trainer.params.numel(), trainer.dec_params.numel()
    opt_class_ms, opt_class_n = prof["optimizer"]
    result = dict(metric="seq2seq_train_bench", measured=True, model="byt5-small (synthetic, hf)", batch=B, source_bytes=S,
                  target_labels=T, iters=a.iters, step_ms=round(s_ms, 3), full_grad_ms=round(g_ms, 3),
                  step_over_full_grad=round(s_ms / g_ms, 4), step_ms_all=[round(x, 3) for x in ts["step"]],
                  full_grad_ms_all=[round(x, 3) for x in ts["full_grad"]],
                  optimizer_step_ms_back_to_back=round(opt_ms, 4),
                  optimizer_and_reload_share_of_step=round(opt_ms / s_ms, 4),
                  profiled_step_optimizer_class=dict(ms=round(opt_class_ms, 4), launch_groups=int(opt_class_n)),
                  profiled_step_ms_by_class={k: round(v[0], 3) for k, v in prof.items() if v[1]},
                  decoder_reload=dict(bytes=int(nbytes), table_elements=int(n_dec), back_to_back=rate(reload_ms),
                                      profiled=rate(rl_ms / max(rl_n, 1)), profiled_launches=int(rl_n)),
                  parameters=dict(encoder_flat=int(n_enc), decoder_flat=int(n_dec)),
                  note="step = HipSeq2SeqTrainer.loss_and_grads + optimizer_step (shared-gradient sum, AdamW over both flat "
                       "buffers, copy of the embedding master, rp_trainer_load_params, rp_decoder_load_params); full_grad = "
                       "HipSeq2SeqGradients.loss_and_grads, the protocol of profiles/seq2seq_full_grad_bench.json; "
                       "optimizer_step_ms_back_to_back = device events around 5 consecutive optimizer steps; decoder_reload "
                       "rates = bytes its table moves (4 B read per element, 2 B written per bf16 copy, 4 B per fp32 copy) / "
                       "time; one box, one run")
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--src-bytes", type=int, default=2300)
    ap.add_argument("--tgt", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-pairs", type=int, default=2)
    ap.add_argument("--step-tokens", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--grad", action="store_true", help="time rp_decoder_loss_grad against rp_decoder_forward")
    ap.add_argument("--full-grad", action="store_true", help="time HipSeq2SeqGradients against the decoder-only gradients")
    ap.add_argument("--step", action="store_true", help="time the whole training step against the --full-grad call")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P",
                    help="with --step: time the step at p = 0 against the step at p = P (T5's dropout) instead")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.step:
        return _step_dropout_leg(a, dev) if a.dropout > 0 else _step_leg(a, dev)
    if a.full_grad:
        return _full_grad_leg(a, dev)
    cfg = synth.seq2seq_config("byt5-small")
    gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg, scale="sharp"), dev)
    B, S = a.batch, a.src_bytes
    srcs = [_source(S, 100 + b) for b in range(B)]
    ids = np.concatenate(srcs)
    src_cu = np.arange(B + 1, dtype=np.int32) * S
    D, F, inner, V, L = cfg["d_model"], cfg["d_ff"], cfg["num_heads"] * cfg["d_kv"], cfg["vocab_size"], cfg["num_decoder_layers"]
    enc_ms = _time(lambda: gen.encode_hidden_packed(ids, src_cu), a.iters)
    enc = gen.encode_hidden_packed(ids, src_cu)
    rng = np.random.default_rng(0)
    if a.grad:
        return _grad_leg(a, gen, enc, src_cu, rng)
    result = dict(model="byt5-small (synthetic, sharp)", batch=B, source_bytes=S, encoder_ms=round(enc_ms, 3), targets={})
    for T in a.tgt:
        y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)
        tokens, labels, tgt_cu = shift_and_segment(y)
        dec_ms = _time(lambda: gen.decoder.forward(enc, src_cu, tokens, labels, tgt_cu), a.iters)
        Tt, St = B * T, B * S
        layer_flop = 2 * Tt * D * (3 * inner + inner + inner + inner + 2 * F + F) * L + 2 * Tt * D * V
        cross_flop = 2 * St * D * 2 * inner * L
        attn_flop = 4 * L * cfg["num_heads"] * cfg["d_kv"] * B * (T * (T + 1) / 2 + T * S)
        # the step loop: per-token cost of rp_decoder_step over the first tokens of a few pairs
        n_tok = min(a.step_tokens, T)
        t0 = time.perf_counter()
        for b in range(a.step_pairs):
            gen.decoder.start(enc[src_cu[b] : src_cu[b + 1]], 1, T)
            for t in range(n_tok):
                gen.decoder.step(torch.tensor([int(tokens[tgt_cu[b] + t])]), torch.arange(t + 1)[None])
        torch.cuda.synchronize()
        step_ms_per_token = (time.perf_counter() - t0) * 1e3 / (a.step_pairs * n_tok)
        loop_ms = step_ms_per_token * Tt
        result["targets"][str(T)] = dict(
            decoder_ms=round(dec_ms, 3), decoder_vs_encoder=round(dec_ms / enc_ms, 4),
            gemm_tflop=dict(layers_and_head=round(layer_flop / 1e12, 3), cross_kv=round(cross_flop / 1e12, 3)),
            attention_tflop=round(attn_flop / 1e12, 3),
            decoder_pass_gemm_tflops_per_s_lower_bound=round((layer_flop + cross_flop) / dec_ms / 1e9, 1),
            step_loop_ms_per_token=round(step_ms_per_token, 4), step_loop_ms_estimated=round(loop_ms, 1),
            speedup_vs_step_loop=round(loop_ms / dec_ms, 1))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
