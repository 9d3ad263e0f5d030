"""Tactic-generator timings on one GPU: decode-step microseconds at cache lengths 1 / 128 / 511 for 1, 8 and 64 beams
(ByT5-small-shaped synthetic weights, a 2048-byte source), the whole generate call at the prover shape (64 beams,
max_length 512, length_penalty 0), and the decoder weight bytes per step against HBM bandwidth.  One JSON line.

    python tools/gen_bench.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reprover_amd import synth  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def step_us(gen, enc, nb, t, max_len, reps=20):
    dec = gen.decoder
    dec.start(enc, nb, max_len)
    tok = torch.full((nb,), 7, dtype=torch.int32, device=gen.device)
    anc = (torch.arange(t + 1, device=gen.device)[None, :] * nb + torch.arange(nb, device=gen.device)[:, None]).int()
    out = torch.empty((nb, gen.cfg["vocab_size"]), dtype=torch.float32, device=gen.device)
    for _ in range(3):
        dec.step(tok, anc, out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dec.step(tok, anc, out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    cfg = synth.seq2seq_config("byt5-small")
    sd = synth.synth_seq2seq_state_dict(cfg)
    gen = HipT5Generator(cfg, sd, "cuda:0")
    rng = np.random.default_rng(0)
    src = np.concatenate([rng.integers(3, 259, size=2047), [1]]).astype(np.int32)
    enc = gen.encode_hidden(src)
    res = {"metric": "gen_bench", "config": "byt5-small (4 decoder layers), source 2048 bytes", "step_us": {}}
    for nb in (1, 8, 64):
        for t in (0, 127, 510):
            res["step_us"][f"beams{nb}_cache{t + 1}"] = round(step_us(gen, enc, nb, t, 512), 1)
    D, F, inner, L, V = cfg["d_model"], cfg["d_ff"], cfg["num_heads"] * cfg["d_kv"], cfg["num_decoder_layers"], cfg["vocab_size"]
    wbytes = 2 * (L * (3 * inner * D + D * inner + inner * D + D * inner + 2 * F * D + D * F) + V * D)
    res["weight_bytes_per_step"] = wbytes
    res["weight_floor_us"] = round(wbytes / HBM_BYTES_PER_S * 1e6, 1)
    for k, v in list(res["step_us"].items()):
        res.setdefault("roofline_fraction", {})[k] = round(res["weight_floor_us"] / v, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = []
    gen.generate(src, 64, 512, 0.0, trace=steps)
    torch.cuda.synchronize()
    res["prover_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["prover_call_steps"] = len(steps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
