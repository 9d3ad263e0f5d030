"""Tactic-prefix beam search, host side: the beam-search driver with a decoder prompt against HuggingFace
``generate(decoder_input_ids=[start] + prefix)`` (G27) through the fp32 CPU restatement of the T5 decoder
(tests/gen_helpers.py) with the prompt rows written by ``prefill_by_steps``; a planted divisor mutant the fixture tells
apart; empty and None prompts on the G20 grid; the lockstep loop and the slot pool over prompts of different lengths; the
refused combinations; the product classes over a stub engine."""
import asyncio
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.generation import (BeamBooksPool, BeamSearchOutput, BeamSearchPool, SamplePool, _BeamState,  # noqa: E402
                                     beam_search, beam_search_batch, beam_search_batch_device, greedy_search,
                                     greedy_search_batch, prefill_by_steps, sample_search, sample_search_batch)
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402

N_BEAM_CASES = 81


def _model(meta):
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    return cfg, sd


@pytest.fixture(scope="module")
def g27(golden_dir):
    z = np.load(os.path.join(golden_dir, "g27_generate_prefix.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg, sd = _model(meta)
    ref = T5Fp32(cfg, sd)
    return z, meta, cfg, sd, ref, ref.encode(z["src"])


def test_g27_grid(g27):
    z, meta = g27[:2]
    beam = meta["cases"][:N_BEAM_CASES]
    assert meta["n_beam_cases"] == N_BEAM_CASES and len(meta["cases"]) == N_BEAM_CASES + 4
    assert {c["prefix_len"] for c in beam} == {1, 5, 17} and {c["num_beams"] for c in beam} == {2, 4, 8}
    assert {c["length_penalty"] for c in beam} == {0.0, 1.0, -0.5}
    assert {c["max_length"] - c["prefix_len"] for c in beam} == {2, 6, 20}
    assert sum(c["bf16_agrees"] for c in beam) >= 24 and sum(c["n_finished_on_eos"] for c in beam) >= 8
    assert [(c["num_beams"], c["prefix_len"]) for c in meta["cases"][N_BEAM_CASES:]] == [(1, 1), (1, 1), (1, 5), (1, 5)]
    for ci, c in enumerate(meta["cases"]):  # HF's sequences hold the prompt
        assert np.array_equal(z[f"c{ci}_seq"][:, : 1 + c["prefix_len"]],
                              np.tile(np.concatenate([[0], z[f"c{ci}_prefix"]]), (c["num_beams"], 1)))


@pytest.mark.parametrize("case", range(N_BEAM_CASES))
def test_prompted_beam_search_matches_hf_generate(g27, case):
    z, meta, cfg, sd, ref, enc = g27
    c = meta["cases"][case]
    nb, lp, ml, prefix = c["num_beams"], c["length_penalty"], c["max_length"], z[f"c{case}_prefix"]
    ref.start(enc, nb, ml)
    trace = []
    out = beam_search(ref.step, nb, ml, lp, trace=trace, prompt=prefix,
                      prefill=lambda rows: prefill_by_steps(ref.step, nb, rows))
    assert len(trace) == c["steps"]
    assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
    np.testing.assert_allclose(out.sequences_scores.numpy(), z[f"c{case}_score"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(np.stack([t[1].numpy() for t in trace]), z[f"c{case}_trace_token"])
    assert np.array_equal(np.stack([t[2].numpy() for t in trace]), z[f"c{case}_trace_parent"])
    np.testing.assert_allclose(np.stack([t[0].numpy() for t in trace]), z[f"c{case}_trace_score"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", range(N_BEAM_CASES, N_BEAM_CASES + 4))
def test_prompted_greedy_matches_hf_generate(g27, case):
    z, meta, cfg, sd, ref, enc = g27
    c = meta["cases"][case]
    prefix = z[f"c{case}_prefix"]
    ref.start(enc, 1, c["max_length"])
    out = greedy_search(ref.step, c["max_length"], prompt=prefix)
    assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
    assert out.sequences[0, : 1 + len(prefix)].tolist() == [0] + prefix.tolist()


def test_divisors_that_count_the_prompt_are_told_apart(g27):
    """prompt_len left at 1 in the two divisors: every ``length_penalty != 0`` case moves by more than the fixture's
    tolerance (sequences or scores), and the ``length_penalty == 0`` cases do not move at all."""
    z, meta, cfg, sd, ref, enc = g27
    for case, c in enumerate(meta["cases"][:N_BEAM_CASES]):
        if c["max_length"] - c["prefix_len"] != 6:  # one max_length per (P, nb, lp): 27 searches
            continue
        nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
        ref.start(enc, nb, ml)
        bad = beam_search(ref.step, nb, ml, lp, prompt=z[f"c{case}_prefix"], mutant="divisors_count_prompt")
        same = (bad.sequences.shape == z[f"c{case}_seq"].shape and np.array_equal(bad.sequences.numpy(), z[f"c{case}_seq"])
                and np.allclose(bad.sequences_scores.numpy(), z[f"c{case}_score"], rtol=1e-5, atol=1e-5))
        assert same == (lp == 0.0), (case, c)


# ---- empty and None prompts: today's objects, outputs and traces -------------------------------------------------------
def test_empty_and_none_prompts_are_the_same_books():
    a = _BeamState(4, 12, 1.0, 1, 0, None)
    for prompt in (None, [], np.zeros(0, dtype=np.int32)):
        b = _BeamState(4, 12, 1.0, 1, 0, None, prompt)
        assert set(vars(a)) == set(vars(b))
        for k, v in vars(a).items():
            w = getattr(b, k)
            if isinstance(v, torch.Tensor):
                assert v.dtype == w.dtype and v.shape == w.shape and torch.equal(v, w), k
            else:
                assert v == w, k
    assert a.prompt_len == 1 and a.ancestry.shape == (4, 0) and a.running_bi.shape == (4, 11)


@pytest.fixture(scope="module")
def g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg, sd = _model(meta)
    ref = T5Fp32(cfg, sd)
    return z, meta, ref, ref.encode(z["src"])


@pytest.mark.parametrize("case", range(24))
def test_empty_and_none_prompts_on_the_g20_grid(g20, case):
    z, meta, ref, enc = g20
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    outs = []
    for kw in ({}, {"prompt": None}, {"prompt": []}):
        calls = []

        def step(tokens, ancestry):
            calls.append((tokens.clone(), ancestry.clone()))
            return ref.step(tokens, ancestry)

        ref.start(enc, nb, ml)
        trace = []
        out = beam_search(step, nb, ml, lp, trace=trace, **kw)
        outs.append((out, trace, calls))
        assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
        assert np.array_equal(np.stack([t[1].numpy() for t in trace]), z[f"c{case}_trace_token"])
        assert np.array_equal(np.stack([t[2].numpy() for t in trace]), z[f"c{case}_trace_parent"])
    for out, trace, calls in outs[1:]:  # the same bits and the same calls into the model
        assert torch.equal(out.sequences_scores, outs[0][0].sequences_scores)
        assert all(torch.equal(x, y) for t, u in zip(trace, outs[0][1]) for x, y in zip(t, u))
        assert len(calls) == len(outs[0][2])
        assert all(torch.equal(x, y) for t, u in zip(calls, outs[0][2]) for x, y in zip(t, u))
    if nb == 1:
        ref.start(enc, 1, ml)
        g0 = greedy_search(ref.step, ml)
        ref.start(enc, 1, ml)
        g1 = greedy_search(ref.step, ml, prompt=[])
        assert torch.equal(g0.sequences, g1.sequences) and torch.equal(g0.sequences_scores, g1.sequences_scores)
        assert np.array_equal(g0.sequences.numpy(), z[f"c{case}_seq"])


# ---- the lockstep loop and the slot pool over prompts of different lengths -----------------------------------------------
class ManyRef:
    """``step_many`` (with or without ``pos``) / ``admit`` / pool ``step`` over one fp32 decoder and cache per state."""

    def __init__(self, cfg, sd, encs, nb, max_len, start=True):
        self.nb, self.max_len = nb, max_len
        self.refs = [T5Fp32(cfg, sd) for _ in encs]
        self.pos_seen = []
        if start:
            for r, enc in zip(self.refs, encs):
                r.start(enc, nb, max_len)

    def step_many(self, active, tokens, ancestry, pos=None):
        nb = self.nb
        if pos is None:
            pos = [ancestry.shape[1] - 1] * len(active)
        else:
            assert ancestry.shape == (len(active) * nb, max(pos) + 1)
        self.pos_seen.append(list(pos))
        return torch.cat([self.refs[s].step(tokens[a * nb : (a + 1) * nb], ancestry[a * nb : (a + 1) * nb, : pos[a] + 1])
                          for a, s in enumerate(active)])

    def admit(self, slots, sources):
        for s, enc in zip(slots, sources):
            self.refs[s].start(enc, self.nb, self.max_len)

    def step(self, active, pos, tokens, ancestry):
        return self.step_many(active, tokens, ancestry, pos)


@pytest.fixture(scope="module")
def mixed(g27):
    """Four sources with prompts of 0, 1, 5 and 17 tokens, and every search alone (computed once, left unchanged)."""
    z, meta, cfg, sd, ref, enc0 = g27
    src = z["src"]
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    encs = [enc0, ref.encode(cut(40)), ref.encode(source_ids(120, 11)), ref.encode(cut(7))]
    long_prefix = z["c80_prefix"]
    assert len(long_prefix) == 17
    prompts = [None, long_prefix[:1], long_prefix[:5], long_prefix]
    alone = {}

    def alone_for(nb, ml, lp):
        if (nb, ml, lp) not in alone:
            outs = []
            for enc, p in zip(encs, prompts):
                ref.start(enc, nb, ml)
                trace = []
                outs.append((beam_search(ref.step, nb, ml, lp, trace=trace, prompt=p), trace))
            alone[(nb, ml, lp)] = outs
        return alone[(nb, ml, lp)]

    return cfg, sd, encs, prompts, alone_for


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits, not a tolerance


@pytest.mark.parametrize("nb,lp,ml", [(4, 1.0, 24), (2, -0.5, 40), (8, 0.0, 20)])
@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2)])
@pytest.mark.parametrize("prefilled", ["default", "callable"])
def test_batch_with_prompts_of_different_lengths_gives_each_search_alone(mixed, nb, lp, ml, order, prefilled):
    cfg, sd, encs, prompts, alone_for = mixed
    want = alone_for(nb, ml, lp)
    eng = ManyRef(cfg, sd, [encs[i] for i in order], nb, ml)
    seen = []

    def prefill_many(states, rows):
        seen.append((list(states), [list(r) for r in rows]))
        for s, r in zip(states, rows):
            prefill_by_steps(eng.refs[s].step, nb, r)

    traces = []
    kw = {"prefill_many": prefill_many} if prefilled == "callable" else {}
    outs = beam_search_batch(eng.step_many, 4, nb, ml, lp, traces=traces, prompts=[prompts[i] for i in order], **kw)
    for j, i in enumerate(order):
        _same(outs[j], want[i][0])
        assert len(traces[j]) == len(want[i][1])
        assert all(torch.equal(x, y) for t, u in zip(traces[j], want[i][1]) for x, y in zip(t, u))
        P = 0 if prompts[i] is None else len(prompts[i])
        assert outs[j].sequences[:, 1 : 1 + P].tolist() == [[int(x) for x in (prompts[i] if P else [])]] * nb
    if prefilled == "callable":  # one call: the states with a prompt, rows = [start] + prompt[:-1]
        (states, rows), = seen
        assert states == [j for j, i in enumerate(order) if prompts[i] is not None]
        assert rows == [[0] + [int(x) for x in prompts[order[j]][:-1]] for j in states]
    loop = [p for p in eng.pos_seen if len(p) > 1]
    assert loop and loop[0] == [0 if prompts[i] is None else len(prompts[i]) for i in order]  # a position per state


def test_greedy_batch_with_prompts_gives_each_search_alone(mixed):
    cfg, sd, encs, prompts, _ = mixed
    ml = 24
    eng = ManyRef(cfg, sd, encs, 1, ml)
    outs = greedy_search_batch(eng.step_many, 4, ml, prompts=prompts)
    for enc, p, out in zip(encs, prompts, outs):
        ref = T5Fp32(cfg, sd)
        ref.start(enc, 1, ml)
        _same(out, greedy_search(ref.step, ml, prompt=p))
        P = 0 if p is None else len(p)
        assert out.sequences[0, 1 : 1 + P].tolist() == ([] if p is None else [int(x) for x in p])
        assert out.sequences.shape[1] <= ml


def _run_pool(mixed, nb, ml, lp, mutant=None, prefill=False):
    """Six tickets (the four sources, then sources 1 and 3 with each other's prompts) through 2 slots, a newcomer
    queued every two steps: ({ticket: output}, [(source, prompt)] by ticket, the engine)."""
    cfg, sd, encs, prompts, _ = mixed
    jobs = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (3, 1)]
    eng = ManyRef(cfg, sd, encs[:2], nb, ml, start=False)
    kw = {}
    if prefill:
        kw["prefill"] = lambda slots, rows: [prefill_by_steps(eng.refs[s].step, nb, r) for s, r in zip(slots, rows)]
    pool = BeamSearchPool(eng.admit, eng.step, 2, nb, ml, lp, mutant=mutant, **kw)
    got = {}
    for si, pi in jobs:
        pool.submit(encs[si], prompt=prompts[pi]) if prompts[pi] is not None else pool.submit(encs[si])
        for _ in range(2):
            got.update(pool.step())
    got.update(pool.drain())
    assert sorted(got) == list(range(len(jobs))) and pool.in_flight == 0 and pool.queued == 0
    return got, jobs, eng


@pytest.mark.parametrize("nb,lp,ml", [(4, 1.0, 24), (2, -0.5, 40)])
@pytest.mark.parametrize("prefill", [False, True])
def test_pool_tickets_with_different_prompts_equal_their_search_alone(mixed, g27, nb, lp, ml, prefill):
    cfg, sd, encs, prompts, alone_for = mixed
    ref = g27[4]
    got, jobs, eng = _run_pool(mixed, nb, ml, lp, prefill=prefill)
    assert any(len(set(p)) > 1 for p in eng.pos_seen), eng.pos_seen  # slots of one step at different positions
    for ticket, (si, pi) in enumerate(jobs):
        if si == pi:
            want = alone_for(nb, ml, lp)[si][0]
        else:
            ref.start(encs[si], nb, ml)
            want = beam_search(ref.step, nb, ml, lp, prompt=prompts[pi])
        _same(got[ticket], want)


def test_pool_shared_position_mutant_is_noticed_with_prompts(mixed, g27):
    cfg, sd, encs, prompts, alone_for = mixed
    nb, lp, ml = 4, 1.0, 24
    want = alone_for(nb, ml, lp)
    bad, jobs, _ = _run_pool(mixed, nb, ml, lp, mutant="shared_position")
    differs = [not (bad[t].sequences.shape == want[si][0].sequences.shape
                    and torch.equal(bad[t].sequences, want[si][0].sequences)
                    and torch.equal(bad[t].sequences_scores, want[si][0].sequences_scores))
               for t, (si, pi) in enumerate(jobs) if si == pi]
    assert any(differs), "the shared-position mutant changed no output: the comparison would not notice it"


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_value_errors():
    nothing = lambda *a, **k: None  # noqa: E731
    step = lambda t, a: torch.zeros(len(t), 384)  # noqa: E731
    with pytest.raises(ValueError):
        _BeamState(4, 6, 1.0, 1, 0, None, [5, 6, 7, 8, 9])  # max_length <= 1 + len(prompt)
    _BeamState(4, 7, 1.0, 1, 0, None, [5, 6, 7, 8, 9])
    with pytest.raises(ValueError):
        beam_search(step, 4, 4, prompt=[5, 6, 7])
    with pytest.raises(ValueError):
        greedy_search(step, 4, prompt=[5, 6, 7])
    with pytest.raises(ValueError):
        beam_search_batch(nothing, 2, 4, 8, prompts=[[5]])  # one entry per state
    with pytest.raises(ValueError):
        greedy_search_batch(nothing, 2, 8, prompts=[[5], None, None])
    pool = BeamSearchPool(nothing, nothing, 2, 4, 6)
    with pytest.raises(ValueError):
        pool.submit("src", prompt=[5, 6, 7, 8, 9])
    assert pool.queued == 0
    # the device books and sampling: not built yet
    with pytest.raises(ValueError, match="not built yet"):
        beam_search_batch_device(nothing, nothing, nothing, 1, 4, 8, prompts=[[5]])
    books = BeamBooksPool(nothing, nothing, 2, 4, 8)
    with pytest.raises(ValueError, match="not built yet"):
        books.submit("src", prompt=[5])
    assert books.submit("src") == 0 and books.submit("src", prompt=[]) == 1
    with pytest.raises(ValueError, match="not built yet"):
        sample_search_batch(nothing, nothing, 1, 4, 8, [0], prompts=[[5]])
    with pytest.raises(ValueError, match="not built yet"):
        sample_search(nothing, nothing, 4, 8, prompt=[5])
    sp = SamplePool(nothing, nothing, nothing, 2, 4, 8)
    with pytest.raises(ValueError, match="not built yet"):
        sp.submit("src", 0, prompt=[5])
    assert sp.submit("src", 0) == 0


# ---- the product classes over a stub engine ---------------------------------------------------------------------------
def stub_output(ids, nb, prefix):
    body = [int(x) for x in np.asarray(ids)[:4] if x >= 3]
    rows = [[0] + list(prefix or []) + body + [3 + ord("0") + r, 1] for r in range(nb)]
    scores = [-0.25 * r - 0.001 * len(ids) for r in range(nb)]
    return BeamSearchOutput(torch.tensor(rows, dtype=torch.int64), torch.tensor(scores, dtype=torch.float32))


class StubStream:
    def __init__(self, engine, nb):
        self.engine, self.nb, self.waiting, self.tickets = engine, nb, [], 0

    queued = property(lambda self: len(self.waiting))
    in_flight = property(lambda self: 0)

    def submit(self, ids, **kw):
        self.engine.calls.append(("submit", kw))
        self.tickets += 1
        self.waiting.append((self.tickets, ids, kw.get("prefix")))
        return self.tickets

    def step(self):
        done, self.waiting = [(t, stub_output(ids, self.nb, p)) for t, ids, p in self.waiting], []
        return done


class StubEngine:
    def __init__(self):
        self.decoder = SimpleNamespace(max_states=lambda nb: 2)
        self.calls = []

    def generate(self, ids, nb, max_len, lp, **kw):
        self.calls.append(("generate", kw))
        return stub_output(ids, nb, kw.get("prefix"))

    def generate_many(self, sources, nb, max_len, lp, **kw):
        self.calls.append(("generate_many", kw))
        prefixes = kw.get("prefixes") or [None] * len(sources)
        return [stub_output(ids, nb, p) for ids, p in zip(sources, prefixes)]

    def generate_stream(self, nb, max_len, lp, n_slots=None, src_cap=None):
        return StubStream(self, nb)


def stub_generator(**kw):
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, **kw)
    gen.generator, gen.tokenizer = StubEngine(), ByT5Tokenizer()
    return gen


ARGS = ("f.lean", "thm", Pos(1, 0))
STATE = "h : x = y ⊢ y = x"


def test_generate_sync_prefix_bytes_and_strings():
    gen = stub_generator()
    out = gen.generate_sync(STATE, *ARGS, 4, prefix="rw [")
    assert gen.generator.calls == [("generate", {"prefix": [b + 3 for b in b"rw ["]})]
    assert len(out) == 4 and all(t.startswith("rw [") for t, _ in out)
    assert [s for _, s in out] == stub_output(np.zeros(len(STATE.encode()) + 1), 4, None).sequences_scores.tolist()
    gen.generator.calls.clear()
    uni = gen.generate_sync(STATE, *ARGS, 2, prefix="∀ x")  # UTF-8 bytes, no EOS
    assert gen.generator.calls[0][1]["prefix"] == [b + 3 for b in "∀ x".encode("utf-8")]
    assert all(t.startswith("∀ x") for t, _ in uni)


def test_empty_prefix_is_none_with_the_same_engine_calls():
    gen = stub_generator()
    a = gen.generate_sync(STATE, *ARGS, 4)
    b = gen.generate_sync(STATE, *ARGS, 4, prefix=None)
    c = gen.generate_sync(STATE, *ARGS, 4, prefix="")
    assert a == b == c and gen.generator.calls == [("generate", {})] * 3
    gen.generator.calls.clear()
    x = gen.batch_generate_sync([STATE, "⊢ True"], [ARGS[0]] * 2, [ARGS[1]] * 2, [ARGS[2]] * 2, 4)
    y = gen.batch_generate_sync([STATE, "⊢ True"], [ARGS[0]] * 2, [ARGS[1]] * 2, [ARGS[2]] * 2, 4, prefixes=[None, ""])
    assert x == y and gen.generator.calls == [("generate_many", {})] * 2
    assert asyncio.run(gen.generate(STATE, *ARGS, 4, prefix="")) == a


def test_batch_generate_sync_prefixes():
    gen = stub_generator()
    states = [STATE, "⊢ True", "a : Nat"]
    lists = ([ARGS[0]] * 3, [ARGS[1]] * 3, [ARGS[2]] * 3)
    out = gen.batch_generate_sync(states, *lists, 4, prefixes=["rw [", None, "exact "])
    want = [gen.generate_sync(s, *ARGS, 4, prefix=p) for s, p in zip(states, ["rw [", None, "exact "])]
    assert out == want
    assert all(t.startswith("rw [") for t, _ in out[0]) and all(t.startswith("exact ") for t, _ in out[2])
    many = [kw for name, kw in gen.generator.calls if name == "generate_many"]  # chunks of max_states = 2
    assert many == [{"prefixes": [[b + 3 for b in b"rw ["], None]}, {"prefixes": [[b + 3 for b in b"exact "]]}]
    with pytest.raises(ValueError):
        gen.batch_generate_sync(states, *lists, 4, prefixes=["rw ["])


def test_continuous_path_hands_the_prefix_over_with_the_ticket():
    gen = stub_generator(continuous=True)

    async def main():
        return await asyncio.gather(gen.generate(STATE, *ARGS, 4, prefix="simp only"), gen.generate(STATE, *ARGS, 4))

    with_prefix, without = asyncio.run(main())
    assert all(t.startswith("simp only") for t, _ in with_prefix) and without == gen.generate_sync(STATE, *ARGS, 4)
    submits = [kw for name, kw in gen.generator.calls if name == "submit"]
    assert submits == [{"prefix": [b + 3 for b in b"simp only"]}, {}]


def test_product_refusals():
    with pytest.raises(ValueError, match="not built yet"):
        stub_generator(do_sample=True).generate_sync(STATE, *ARGS, 4, prefix="rw")
    with pytest.raises(ValueError, match="not built yet"):
        stub_generator(beam_sync_every=4).generate_sync(STATE, *ARGS, 4, prefix="rw")
    with pytest.raises(ValueError, match="not built yet"):
        stub_generator(beam_sync_every=4).batch_generate_sync([STATE], [ARGS[0]], [ARGS[1]], [ARGS[2]], 4, prefixes=["rw"])
    with pytest.raises(ValueError, match="not built yet"):
        asyncio.run(stub_generator(continuous=True, beam_sync_every=2).generate(STATE, *ARGS, 4, prefix="rw"))
    gen = stub_generator()  # max_oup_seq_len = 16: the start token + 15 bytes leave no room
    with pytest.raises(ValueError, match="no room"):
        gen.generate_sync(STATE, *ARGS, 4, prefix="x" * 15)
    assert gen.generator.calls == []
    gen.generate_sync(STATE, *ARGS, 4, prefix="x" * 14)
    # the refused engines still serve the call without a prefix
    assert stub_generator(beam_sync_every=4).generate_sync(STATE, *ARGS, 4, prefix="") \
        == stub_generator().generate_sync(STATE, *ARGS, 4)


def test_retrieval_augmented_generator_passes_the_prefix_through():
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10)
    rag.hf_gen.generator, rag.hf_gen.tokenizer = StubEngine(), ByT5Tokenizer()
    seen = []
    rag.retriever = SimpleNamespace(retrieve=lambda state, *a: (seen.append(state), ([], []))[1])
    out = rag.generate_sync(STATE, *ARGS, 4, prefix="exact ")
    assert all(t.startswith("exact ") for t, _ in out) and seen == [STATE]
    assert asyncio.run(rag.generate(STATE, *ARGS, 4, prefix="exact ")) == out
    both = rag.batch_generate_sync([STATE, STATE], [ARGS[0]] * 2, [ARGS[1]] * 2, [ARGS[2]] * 2, 4, prefixes=["exact ", None])
    assert both[0] == out and both[1] == rag.generate_sync(STATE, *ARGS, 4)
    with pytest.raises(ValueError, match="no room"):
        rag.generate_sync(STATE, *ARGS, 4, prefix="x" * 40)
    assert len(seen) == 5  # the refused call retrieved nothing
