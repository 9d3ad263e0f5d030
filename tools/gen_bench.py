"""Tactic-generator timings on one GPU: decode-step microseconds at cache lengths 1 / 128 / 511 for 1, 8 and 64 beams
(ByT5-small-shaped synthetic weights, a 2048-byte source), the whole generate call at the prover shape (64 beams,
max_length 512, length_penalty 0), and the decoder weight bytes per step against HBM bandwidth.  One JSON line.

    python tools/gen_bench.py [--out FILE]

``--states B [B ...]``: batched generation instead.  For each B, ``generate_many`` over B distinct 2048-byte sources (64
beams, max_length 512, length_penalty 0) against the loop of B ``generate`` calls, in one process, the two alternating;
and the validation shape (greedy, largest B).  Times, ratio (loop / batched), per-step milliseconds and kernel launches
per step, as one JSON line.

    python tools/gen_bench.py --states 1 4 8 [--reps 2] [--out FILE]

``--sample``: the sampled call beside the beam-search prover call, in one process, the two alternating: 64 samples
(temperature 1, top_k 0, top_p 0.95) against 64 beams, a 2048-byte source, max_length 512.  Whole-call and per-step
milliseconds of both, as one JSON line.

    python tools/gen_bench.py --sample [--reps 3] [--out FILE]

``--states B [B ...] --sync-every K [K ...]``: the beam search with its books on the device
(``generate_many(sync_every=K)``) beside the host-books call of the same tree, in one process, alternating: per
repetition the host-books call twice (the difference of its own two runs is the spread), then one call per K.  Whole-call
and per-step milliseconds of each, and whether every device-books output equals the host-books one.

    python tools/gen_bench.py --states 1 8 --sync-every 1 4 16 [--reps 2] [--out FILE]

``--stream``: continuous batching.  16 queued sources of mixed lengths (64 beams, max_length 512) served by
``generate_many`` in chunks of 8 and by a ``generate_stream`` of 8 slots, in one process, alternating: whole-call
milliseconds of both, every search's own step count, the stream's finish step per source, and whether the outputs are
equal.  Where every search runs to ``max_length`` the two do the same work and the figure says nothing about admission.

    python tools/gen_bench.py --stream [--reps 2] [--out FILE]

``--stream --sync-every K [K ...]``: the stream with its books on the device (``generate_stream(sync_every=K)``) beside
the host-books stream of the same tree, in one process, alternating: per repetition the host-books stream twice (the
difference of its own two runs is the spread), then one device-books stream per K.  Whole-call milliseconds, decode steps
and sync points of each, whether every output equals the host-books one, and per K whether a speed-up may be claimed
(every device-books run below the host-books stream's fastest run minus its largest spread).  As above: where every search
runs to ``max_length`` the run measures the per-step host cost and says nothing about admission.

    python tools/gen_bench.py --stream --sync-every 1 4 16 [--reps 2] [--out FILE]

``--stream --sample``: continuous batching for sampling.  The same 16 queued sources, 64 samples each (temperature 1,
top_k 0, top_p 0.95, max_length 512), served by ``sample_many`` in chunks of 8 and by a ``sample_stream`` of 8 slots, in
one process, alternating; every stream output is checked equal to the chunked one.  The EOS row of ``lm_head.weight`` is
multiplied by ``--eos-boost`` so that the states end at different lengths; the length of every state is recorded.  With
plain synthetic weights everything runs to ``max_length`` and the comparison says nothing about admission.

    python tools/gen_bench.py --stream --sample [--eos-boost 4.0] [--reps 2] [--out FILE]

``--stream --sample --per-request``: sampling parameters per request.  The same 16 sources through a ``sample_stream`` of
8 slots twice in one process, alternating: once with the stream's scalars (``rp_sample_pool_step``, the parameters by
value) and once on a stream opened ``per_request`` with the same values handed in per ticket
(``rp_sample_pool_step_rows``, the parameter table).  Milliseconds per decode step of both, the table form as a ratio to
the scalar form beside the scalar form's own spread over the repetitions, and whether the outputs are equal (they are the
same bits by contract).  No threshold: the scalar form measured in the same run is the bar.

    python tools/gen_bench.py --stream --sample --per-request [--reps 3] [--out profiles/gen_sample_params_bench.json]

``--prefix-bytes N [N ...]``: the tactic prefix.  At 64 and at 8 beams, for every N: the one-pass prefill of an N-byte
prefix (``rp_decoder_batch_prefill``) against the same cache rows written by N ordinary decode steps
(``prefill_by_steps`` through ``rp_decoder_batch_step``), alternating in one process, device time per call; and in a
host-books ``generate_stream`` of 8 slots with 7 searches running, the wall time of the step that admits an eighth
source without a prefix, with an N-byte prefix prefilled in one pass, and with the prefix fed through steps, beside the
ordinary steps around it.  No threshold: the by-steps path measured in the same run is the bar.

    python tools/gen_bench.py --prefix-bytes 4 16 64 [--reps 5] [--out FILE]
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


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _same(a, b):
    return all(torch.equal(x.sequences, y.sequences) and torch.equal(x.sequences_scores, y.sequences_scores)
               for x, y in zip(a, b))


def states_bench(gen, cfg, states, reps, nb=64, max_len=512, src_bytes=2048):
    rng = np.random.default_rng(0)
    srcs = [np.concatenate([rng.integers(3, 259, size=src_bytes - 1), [1]]).astype(np.int32) for _ in range(max(states))]
    L = cfg["num_decoder_layers"]
    launches = 12 * L + 4  # per decode step: embed, 12 per layer, final norm, lm_head, log_softmax; + 2 for the selection
    res = {"metric": "gen_batch_bench", "beams": nb, "max_length": max_len, "length_penalty": 0.0,
           "config": f"byt5-small ({L} decoder layers), distinct sources of {src_bytes} bytes", "reps": reps, "states": {}}
    gen.generate_many(srcs[:2], nb, 8, 0.0)  # warm-up: code objects
    gen.generate(srcs[0], nb, 8, 0.0)

    def pair(B, greedy=False):
        loop_ms, many_ms, steps_loop, steps_many, same = [], [], 0, 0, True
        for _ in range(reps):
            tr_loop = [[] for _ in range(B)]
            if greedy:
                ms, a = _timed(lambda: [gen.greedy(s, max_len) for s in srcs[:B]])
                steps_loop = sum(o.sequences.shape[1] - 1 for o in a)
            else:
                ms, a = _timed(lambda: [gen.generate(s, nb, max_len, 0.0, trace=tr_loop[i]) for i, s in enumerate(srcs[:B])])
                steps_loop = sum(len(t) for t in tr_loop)
            loop_ms.append(ms)
            tr = []
            if greedy:
                ms, b = _timed(lambda: gen.greedy_many(srcs[:B], max_len))
                steps_many = max(o.sequences.shape[1] - 1 for o in b)
            else:
                ms, b = _timed(lambda: gen.generate_many(srcs[:B], nb, max_len, 0.0, traces=tr))
                steps_many = max(len(t) for t in tr)
            many_ms.append(ms)
            same = same and _same(a, b)
        lo, ma = min(loop_ms), min(many_ms)
        sel = 0 if greedy else 2
        return {"loop_ms": [round(x, 1) for x in loop_ms], "batched_ms": [round(x, 1) for x in many_ms],
                "ratio_loop_over_batched": round(lo / ma, 3), "loop_steps": steps_loop, "batched_steps": steps_many,
                "loop_ms_per_step": round(lo / steps_loop, 3), "batched_ms_per_step": round(ma / steps_many, 3),
                "launches_per_step": {"loop": (launches + sel) * B, "batched": launches + sel},
                "outputs_identical": same}

    for B in states:
        res["states"][str(B)] = pair(B)
    B = max(states)
    res["greedy_validation_shape"] = dict(pair(B, greedy=True), states=B)
    return res


def books_bench(gen, cfg, states, sync_every, reps, nb=64, max_len=512, src_bytes=2048):
    rng = np.random.default_rng(0)
    srcs = [np.concatenate([rng.integers(3, 259, size=src_bytes - 1), [1]]).astype(np.int32) for _ in range(max(states))]
    L = cfg["num_decoder_layers"]
    res = {"metric": "gen_device_books_bench", "beams": nb, "max_length": max_len, "length_penalty": 0.0,
           "config": f"byt5-small ({L} decoder layers), distinct sources of {src_bytes} bytes", "reps": reps,
           "launches_per_step": {"host_books": 12 * L + 4 + 2, "device_books": 12 * L + 4 + 3}, "states": {}}
    gen.generate_many(srcs[:2], nb, 8, 0.0)  # warm-up: code objects
    gen.generate_many(srcs[:2], nb, 8, 0.0, sync_every=2)
    for B in states:
        host_ms, dev_ms, same, steps = [], {k: [] for k in sync_every}, True, 0
        for _ in range(reps):
            pair = []
            for _ in range(2):
                tr = []
                ms, want = _timed(lambda: gen.generate_many(srcs[:B], nb, max_len, 0.0, traces=tr))
                pair.append(ms)
                steps = max(len(t) for t in tr)
            host_ms.append(pair)
            for k in sync_every:
                ms, got = _timed(lambda: gen.generate_many(srcs[:B], nb, max_len, 0.0, sync_every=k))
                dev_ms[k].append(ms)
                same = same and _same(got, want)
        best = min(min(p) for p in host_ms)
        res["states"][str(B)] = {
            "steps": steps, "host_books_ms": [[round(x, 1) for x in p] for p in host_ms],
            "host_books_spread_ms": [round(abs(p[0] - p[1]), 1) for p in host_ms],
            "host_books_ms_per_step": round(best / steps, 3),
            "device_books_ms": {str(k): [round(x, 1) for x in v] for k, v in dev_ms.items()},
            "device_books_ms_per_step": {str(k): round(min(v) / steps, 3) for k, v in dev_ms.items()},
            "ratio_host_over_device": {str(k): round(best / min(v), 3) for k, v in dev_ms.items()},
            "outputs_identical": same}
    return res


def sample_bench(gen, cfg, reps, nb=64, max_len=512, src_bytes=2048):
    rng = np.random.default_rng(0)
    src = np.concatenate([rng.integers(3, 259, size=src_bytes - 1), [1]]).astype(np.int32)
    kw = dict(temperature=1.0, top_k=0, top_p=0.95)
    gen.generate(src, nb, 8, 0.0)  # warm-up: code objects
    gen.sample(src, nb, 8, **kw)
    beam_ms, sample_ms, beam_steps, sample_steps = [], [], 0, 0
    for r in range(reps):
        steps = []
        ms, _ = _timed(lambda: gen.generate(src, nb, max_len, 0.0, trace=steps))
        beam_ms.append(ms)
        beam_steps = len(steps)
        ms, out = _timed(lambda: gen.sample(src, nb, max_len, seed=r, **kw))
        sample_ms.append(ms)
        sample_steps = out.sequences.shape[1] - 1  # an upper bound when every sample stops inside one sync interval
    L = cfg["num_decoder_layers"]
    return {"metric": "gen_sample_bench", "rows": nb, "max_length": max_len, "length_penalty": 0.0, "sampling": kw,
            "sync_every": 16, "config": f"byt5-small ({L} decoder layers), source {src_bytes} bytes", "reps": reps,
            "beam_ms": [round(x, 1) for x in beam_ms], "sample_ms": [round(x, 1) for x in sample_ms],
            "beam_steps": beam_steps, "sample_steps": sample_steps,
            "beam_ms_per_step": [round(x / beam_steps, 3) for x in beam_ms],
            "sample_ms_per_step": [round(x / sample_steps, 3) for x in sample_ms],
            "launches_per_step": {"beam": 12 * L + 4 + 2, "sample": 12 * L + 4 + 1}}


def stream_bench(gen, cfg, reps, nb=64, max_len=512, n_src=16, n_slots=8):
    """16 queued sources of mixed lengths served (a) by ``generate_many`` in chunks of ``n_slots`` and (b) by a stream of
    ``n_slots`` slots, alternating in one process; the per-source finish step beside the times.  The stream can only win
    where states stop at different steps: ``finish_steps_differ`` says whether they did."""
    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(64, 2049, size=n_src)]
    srcs = [np.concatenate([rng.integers(3, 259, size=n - 1), [1]]).astype(np.int32) for n in lens]
    L = cfg["num_decoder_layers"]
    gen.generate_many(srcs[:2], nb, 8, 0.0)  # warm-up: code objects
    warm = gen.generate_stream(nb, 8, 0.0, n_slots=2, src_cap=2048)
    warm.submit(srcs[0])
    warm.drain()

    def chunks():
        outs, steps = [], []
        for i in range(0, n_src, n_slots):
            tr = []
            outs += gen.generate_many(srcs[i : i + n_slots], nb, max_len, 0.0, traces=tr)
            steps += [len(t) for t in tr]
        return outs, steps

    def stream():
        st = gen.generate_stream(nb, max_len, 0.0, n_slots=n_slots, src_cap=2048)
        tickets = [st.submit(s) for s in srcs]
        got, finish = {}, {}
        while st.queued or st.in_flight:
            for ticket, out in st.step():
                got[ticket], finish[ticket] = out, st.steps
        return [got[t] for t in tickets], [finish[t] for t in tickets], st.steps

    chunk_ms, stream_ms, same = [], [], True
    for _ in range(reps):
        ms, (a, own_steps) = _timed(chunks)
        chunk_ms.append(ms)
        ms, (b, finish, total) = _timed(stream)
        stream_ms.append(ms)
        same = same and _same(a, b)
    chunk_steps = sum(max(own_steps[i : i + n_slots]) for i in range(0, n_src, n_slots))
    return {"metric": "gen_stream_bench", "beams": nb, "max_length": max_len, "length_penalty": 0.0, "sources": n_src,
            "slots": n_slots, "config": f"byt5-small ({L} decoder layers), sources of {min(lens)}..{max(lens)} bytes",
            "source_bytes": lens, "reps": reps, "chunked_generate_many_ms": [round(x, 1) for x in chunk_ms],
            "stream_ms": [round(x, 1) for x in stream_ms],
            "ratio_chunked_over_stream": round(min(chunk_ms) / min(stream_ms), 3),
            "steps_of_each_search": own_steps, "stream_finish_step": finish, "chunked_decode_steps": chunk_steps,
            "stream_decode_steps": total, "finish_steps_differ": len(set(own_steps)) > 1, "outputs_identical": same}


def stream_books_bench(gen, cfg, sync_every, reps, nb=64, max_len=512, n_src=16, n_slots=8):
    """``stream_bench``'s 16 queued sources through a stream of ``n_slots`` slots with host books (the baseline, twice per
    repetition) and with device books at every ``sync_every``, alternating in one process."""
    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(64, 2049, size=n_src)]
    srcs = [np.concatenate([rng.integers(3, 259, size=n - 1), [1]]).astype(np.int32) for n in lens]
    L = cfg["num_decoder_layers"]

    def stream(n, length, sources, **kw):
        st = gen.generate_stream(nb, length, 0.0, n_slots=n, src_cap=2048, **kw)
        tickets = [st.submit(s) for s in sources]
        got = dict(st.drain())
        return [got[t] for t in tickets], st.steps, getattr(st.pool, "sync_points", None)

    stream(2, 8, srcs[:1])  # warm-up: code objects
    stream(2, 8, srcs[:1], sync_every=2)
    host_ms, dev_ms, same, host_steps = [], {k: [] for k in sync_every}, True, 0
    dev_steps, dev_syncs = {}, {}
    for _ in range(reps):
        pair = []
        for _ in range(2):
            ms, (want, host_steps, _) = _timed(lambda: stream(n_slots, max_len, srcs))
            pair.append(ms)
        host_ms.append(pair)
        for k in sync_every:
            ms, (got, dev_steps[k], dev_syncs[k]) = _timed(lambda: stream(n_slots, max_len, srcs, sync_every=k))
            dev_ms[k].append(ms)
            same = same and _same(got, want)
    best = min(min(p) for p in host_ms)
    spread = max(abs(p[0] - p[1]) for p in host_ms)
    return {"metric": "gen_stream_books_bench", "beams": nb, "max_length": max_len, "length_penalty": 0.0, "sources": n_src,
            "slots": n_slots, "config": f"byt5-small ({L} decoder layers), sources of {min(lens)}..{max(lens)} bytes",
            "reps": reps, "host_books_stream_ms": [[round(x, 1) for x in p] for p in host_ms],
            "host_books_spread_ms": [round(abs(p[0] - p[1]), 1) for p in host_ms], "host_books_decode_steps": host_steps,
            "device_books_stream_ms": {str(k): [round(x, 1) for x in v] for k, v in dev_ms.items()},
            "device_books_decode_steps": {str(k): v for k, v in dev_steps.items()},
            "device_books_sync_points": {str(k): v for k, v in dev_syncs.items()},
            "ratio_host_over_device": {str(k): round(best / min(v), 3) for k, v in dev_ms.items()},
            "speedup_claimed": {str(k): bool(max(v) < best - spread) for k, v in dev_ms.items()},
            "outputs_identical": same}


def sample_stream_bench(gen, cfg, reps, eos_boost, nb=64, max_len=512, n_src=16, n_slots=8):
    """``stream_bench``'s 16 queued sources, sampled: (a) ``sample_many`` in chunks of ``n_slots`` and (b) a
    ``sample_stream`` of ``n_slots`` slots, alternating in one process, every stream output checked equal to the chunked
    one.  The generator's EOS row is boosted so that the states end at different lengths (recorded: the stream can only
    win where they do)."""
    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(64, 2049, size=n_src)]
    srcs = [np.concatenate([rng.integers(3, 259, size=n - 1), [1]]).astype(np.int32) for n in lens]
    seeds = list(range(100, 100 + n_src))
    kw = dict(temperature=1.0, top_k=0, top_p=0.95)
    L = cfg["num_decoder_layers"]

    def chunks():
        outs = []
        for i in range(0, n_src, n_slots):
            outs += gen.sample_many(srcs[i : i + n_slots], nb, max_len, seeds=seeds[i : i + n_slots], **kw)
        return outs

    def stream(n=n_slots, length=max_len, sources=srcs):
        st = gen.sample_stream(nb, length, n_slots=n, src_cap=2048, **kw)
        tickets = [st.submit(s, seed) for s, seed in zip(sources, seeds)]
        got = dict(st.drain())
        return [got[t] for t in tickets], st.steps, st.pool.sync_points

    gen.sample_many(srcs[:2], nb, 8, seeds=seeds[:2], **kw)  # warm-up: code objects
    stream(2, 8, srcs[:1])
    chunk_ms, stream_ms, same, steps, syncs = [], [], True, 0, 0
    for _ in range(reps):
        ms, a = _timed(chunks)
        chunk_ms.append(ms)
        ms, (b, steps, syncs) = _timed(stream)
        stream_ms.append(ms)
        same = same and _same(a, b)
    own = [o.sequences.shape[1] - 1 for o in a]  # a state's length: its longest sample
    # the chunked call looks at the flags every 16 positions: a chunk runs to its longest member's next look
    chunk_steps = sum(min(-(-max(own[i : i + n_slots]) // 16) * 16, max_len - 1) for i in range(0, n_src, n_slots))
    return {"metric": "gen_sample_stream_bench", "measured": True, "rows": nb, "max_length": max_len, "length_penalty": 0.0,
            "sampling": kw, "sync_every": 16, "eos_boost": eos_boost, "sources": n_src, "slots": n_slots,
            "config": f"byt5-small ({L} decoder layers), sources of {min(lens)}..{max(lens)} bytes", "source_bytes": lens,
            "reps": reps, "chunked_sample_many_ms": [round(x, 1) for x in chunk_ms],
            "stream_ms": [round(x, 1) for x in stream_ms],
            "ratio_chunked_over_stream": round(min(chunk_ms) / min(stream_ms), 3), "length_of_each_state": own,
            "lengths_differ": len(set(own)) > 1, "states_ended_by_length": sum(n == max_len - 1 for n in own),
            "chunked_decode_steps_upper_bound": chunk_steps, "stream_decode_steps": steps, "stream_sync_points": syncs,
            "outputs_identical": same}


def sample_params_bench(gen, cfg, reps, eos_boost, nb=64, max_len=512, n_src=16, n_slots=8):
    """``sample_stream_bench``'s sources through (a) a stream with the parameters by value and (b) a stream opened
    ``per_request`` with the same values per ticket, alternating in one process: ms per decode step of both."""
    from reprover_amd.generation import SamplingParams

    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(64, 2049, size=n_src)]
    srcs = [np.concatenate([rng.integers(3, 259, size=n - 1), [1]]).astype(np.int32) for n in lens]
    seeds = list(range(100, 100 + n_src))
    kw = dict(temperature=1.0, top_k=0, top_p=0.95)
    L = cfg["num_decoder_layers"]

    def stream(per_request, n=n_slots, length=max_len, sources=srcs):
        st = gen.sample_stream(nb, length, n_slots=n, src_cap=2048, per_request=per_request, **kw)
        extra = dict(params=SamplingParams(**kw), num_samples=nb) if per_request else {}
        tickets = [st.submit(s, seed, **extra) for s, seed in zip(sources, seeds)]
        got = dict(st.drain())
        return [got[t] for t in tickets], st.steps

    for per_request in (False, True):  # warm-up: code objects
        stream(per_request, 2, 8, srcs[:1])
    scalar_ms, table_ms, same, steps = [], [], True, 0
    for _ in range(reps):
        ms, (a, steps) = _timed(lambda: stream(False))
        scalar_ms.append(ms / steps)
        ms, (b, steps_b) = _timed(lambda: stream(True))
        table_ms.append(ms / steps_b)
        same = same and _same(a, b) and steps == steps_b
    base = min(scalar_ms)
    return {"metric": "gen_sample_params_bench", "measured": True, "rows": nb, "max_length": max_len, "sampling": kw,
            "sync_every": 16, "eos_boost": eos_boost, "sources": n_src, "slots": n_slots,
            "config": f"byt5-small ({L} decoder layers), sources of {min(lens)}..{max(lens)} bytes", "reps": reps,
            "decode_steps": steps, "scalar_ms_per_step": [round(x, 4) for x in scalar_ms],
            "table_ms_per_step": [round(x, 4) for x in table_ms],
            "scalar_spread": round(max(scalar_ms) / base - 1.0, 4),
            "ratio_table_over_scalar": round(min(table_ms) / base, 4),
            "ratio_table_over_scalar_by_rep": [round(t / s_, 4) for t, s_ in zip(table_ms, scalar_ms)],
            "outputs_identical": same}


def prefix_bench(gen, cfg, prefix_bytes, reps, max_len=512, src_bytes=2048, n_slots=8):
    """One-pass prefill against ``prefill_by_steps`` (device milliseconds, alternating), and the admission step of a
    host-books stream with and without a prefixed newcomer (wall milliseconds), at 64 and 8 beams."""
    from reprover_amd.generation import prefill_by_steps

    rng = np.random.default_rng(0)
    srcs = [np.concatenate([rng.integers(3, 259, size=src_bytes - 1), [1]]).astype(np.int32) for _ in range(n_slots)]
    text = rng.integers(3 + 32, 3 + 127, size=max(prefix_bytes)).astype(np.int32)
    enc = gen.encode_hidden(srcs[0])
    dec = gen.decoder
    L = cfg["num_decoder_layers"]
    res = {"metric": "gen_prefix_bench", "config": f"byt5-small ({L} decoder layers), sources of {src_bytes} bytes",
           "max_length": max_len, "reps": reps, "slots": n_slots, "beams": {}}

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def admission(nb, prefix, by_steps):
        """(the admitting step's wall ms, the other steps' wall ms): 7 searches run 6 steps, the eighth joins."""
        st = gen.generate_stream(nb, max_len, 0.0, n_slots=n_slots, src_cap=src_bytes)
        if by_steps:
            st.pool._prefill = None  # BeamSearchPool's default: the prompt through ordinary steps
        for s in srcs[:-1]:
            st.submit(s)
        plain = []
        for _ in range(6):
            plain.append(_timed(st.step)[0])
        st.submit(srcs[-1], prefix=prefix)
        admit = _timed(st.step)[0]
        for _ in range(4):
            plain.append(_timed(st.step)[0])
        return admit, plain[1:]  # (the first step admitted the seven)

    for nb in (64, 8):
        dec.start(enc, nb, max_len)
        rows_warm = [0] + text[:3].tolist()
        dec.prefill_many([0], [rows_warm])
        prefill_by_steps(dec.step, nb, rows_warm, gen.device)
        admission(nb, text[:2], False)
        admission(nb, text[:2], True)
        per = {}
        for N in prefix_bytes:
            rows = [0] + text[: N - 1].tolist()  # the N prompt rows: [start] + the prefix without its last byte
            dec.start(enc, nb, max_len)
            one, steps = [], []
            for _ in range(reps):
                one.append(device_ms(lambda: dec.prefill_many([0], [rows])))
                steps.append(device_ms(lambda: prefill_by_steps(dec.step, nb, rows, gen.device)))
            none_ms, pass_ms, step_ms, plain = [], [], [], []
            for _ in range(max(2, reps // 2)):
                for kind, prefix, by_steps in ((none_ms, None, False), (pass_ms, text[:N], False), (step_ms, text[:N], True)):
                    a, p = admission(nb, prefix, by_steps)
                    kind.append(a)
                    plain += p
            per[str(N)] = {
                "one_pass_ms": [round(x, 3) for x in one], "by_steps_ms": [round(x, 3) for x in steps],
                "ratio_by_steps_over_one_pass": round(min(steps) / min(one), 2),
                "one_pass_faster": max(one) < min(steps),
                "stream_admission_step_ms": {"no_prefix": [round(x, 2) for x in none_ms],
                                             "prefix_one_pass": [round(x, 2) for x in pass_ms],
                                             "prefix_by_steps": [round(x, 2) for x in step_ms]},
                "stream_plain_step_ms_median": round(float(np.median(plain)), 2),
            }
        res["beams"][str(nb)] = per
    return res


def constraint_bench(gen, cfg, reps, max_len=512, src_bytes=2048):
    """The same call with and without ``constraint=ByteAutomaton.utf8`` (one ``rp_constraint_mask`` /
    ``rp_constraint_mask_step`` launch more per step), alternating in one process: greedy, 8 and 64 beams, 64 samples.
    Device milliseconds between two events round the whole call, and per decode step (the two searches need not take
    the same number of steps)."""
    from reprover_amd.constraint import ByteAutomaton

    aut = ByteAutomaton.utf8(cfg["vocab_size"])
    rng = np.random.default_rng(0)
    src = np.concatenate([rng.integers(3, 259, size=src_bytes - 1), [1]]).astype(np.int32)
    calls = {
        "greedy": lambda kw: gen.greedy(src, max_len, **kw),
        "beams8": lambda kw: gen.generate(src, 8, max_len, 0.0, **kw),
        "beams64": lambda kw: gen.generate(src, 64, max_len, 0.0, **kw),
        "samples64": lambda kw: gen.sample(src, 64, max_len, 1.0, 0, 1.0, seed=1, **kw),
    }
    res = {"metric": "gen_constraint_bench", "config": f"byt5-small, source {src_bytes} bytes, max_length {max_len}, utf8 "
           f"automaton of {aut.n_states} states", "reps": reps, "rows": {}}
    for name, call in calls.items():
        for kw in ({}, {"constraint": aut}):  # warm-up: code objects, the table's upload
            call(kw)
        ms = {"free": [], "utf8": []}
        steps = {}
        for _ in range(reps):
            for arm, kw in (("free", {}), ("utf8", {"constraint": aut})):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out = call(kw)
                e1.record()
                torch.cuda.synchronize()
                ms[arm].append(round(e0.elapsed_time(e1), 2))
                steps[arm] = int(out.sequences.shape[1]) - 1
        res["rows"][name] = {"free_ms": ms["free"], "utf8_ms": ms["utf8"], "steps": steps,
                             "free_us_per_step": round(1e3 * float(np.median(ms["free"])) / steps["free"], 1),
                             "utf8_us_per_step": round(1e3 * float(np.median(ms["utf8"])) / steps["utf8"], 1)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--states", type=int, nargs="+", default=None, help="batched generation against the per-state loop")
    ap.add_argument("--sync-every", type=int, nargs="+", default=None,
                    help="with --states: device-books generate_many at these sync_every values against the host books; "
                         "with --stream: the device-books stream against the host-books stream")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sample", action="store_true", help="the sampled call beside the beam-search prover call")
    ap.add_argument("--stream", action="store_true", help="a stream of 8 slots against generate_many in chunks of 8")
    ap.add_argument("--eos-boost", type=float, default=4.0,
                    help="with --stream --sample: the factor on the EOS row of lm_head.weight (states end at different lengths)")
    ap.add_argument("--per-request", action="store_true",
                    help="with --stream --sample: the stream's scalars against the same values per ticket (the parameter table)")
    ap.add_argument("--prefix-bytes", type=int, nargs="+", default=None,
                    help="the one-pass prompt prefill against prefill_by_steps, and a stream's admission step with a prefix")
    ap.add_argument("--constraint", choices=["utf8"], default=None,
                    help="the same calls with and without the constraint, alternating (goes alone)")
    args = ap.parse_args(argv)
    if args.constraint:
        if args.prefix_bytes or args.states or args.stream or args.sample or args.sync_every:
            ap.error("--constraint goes alone")
        cfg = synth.seq2seq_config("byt5-small")
        gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg), "cuda:0")
        line = json.dumps(constraint_bench(gen, cfg, max(args.reps, 5)))
        print(line)
        args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                            "gen_constraint_bench.json")
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
        return
    if args.prefix_bytes:
        if min(args.prefix_bytes) < 1 or max(args.prefix_bytes) > 500 or args.states or args.stream or args.sample:
            ap.error("--prefix-bytes takes values in 1..500 and goes alone")
        cfg = synth.seq2seq_config("byt5-small")
        gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg), "cuda:0")
        line = json.dumps(prefix_bench(gen, cfg, sorted(args.prefix_bytes), max(args.reps, 3)))
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    if args.per_request and not (args.stream and args.sample):
        ap.error("--per-request goes with --stream --sample")
    if args.sync_every and (not (args.states or args.stream) or args.sample or min(args.sync_every) < 1):
        ap.error("--sync-every takes values >= 1 and goes with --states or --stream")
    if args.sample or args.stream:
        cfg = synth.seq2seq_config("byt5-small")
        sd = synth.synth_seq2seq_state_dict(cfg)
        if args.stream and args.sample:  # as tests/test_sample_gpu.py's _gen boosts it
            sd["lm_head.weight"] = sd["lm_head.weight"].clone()
            sd["lm_head.weight"][1] *= args.eos_boost
        gen = HipT5Generator(cfg, sd, "cuda:0")
        if args.per_request:
            line = json.dumps(sample_params_bench(gen, cfg, max(args.reps, 3), args.eos_boost))
            args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                "gen_sample_params_bench.json")
        elif args.stream and args.sample:
            line = json.dumps(sample_stream_bench(gen, cfg, args.reps, args.eos_boost))
        elif args.stream and args.sync_every:
            line = json.dumps(stream_books_bench(gen, cfg, args.sync_every, args.reps))
        else:
            line = json.dumps(stream_bench(gen, cfg, args.reps) if args.stream else sample_bench(gen, cfg, max(args.reps, 2)))
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    if args.states:
        cfg = synth.seq2seq_config("byt5-small")
        gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg), "cuda:0")
        if args.sync_every:
            line = json.dumps(books_bench(gen, cfg, sorted(args.states), args.sync_every, args.reps))
        else:
            line = json.dumps(states_bench(gen, cfg, sorted(args.states), args.reps))
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
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
