"""Continuous batching, host side: ``BeamSearchPool`` over the fp32 CPU decoder step (tests/gen_helpers.py) returns, for
every ticket, exactly what ``beam_search`` returns for that source alone - on every G20 grid point, whether the sources
are all there at the start, arrive one every three steps, or outnumber the slots.  A planted mutant (every slot handed the
step's largest position) must change an output.  The async front of ``HuggingFaceGenerator(continuous=True)`` is driven
with a fake engine: every call gets its own result, the driver stops when the stream is idle, a raising step fails every
waiter."""
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
from reprover_amd.generation import BeamSearchOutput, BeamSearchPool, beam_search  # noqa: E402
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402

SCHEDULES = ("all_at_once", "one_every_3_steps", "5_sources_2_slots")


class PoolRef:
    """``admit`` / ``step`` over one fp32 reference decoder (and cache) per slot; a source is its encoder output."""

    def __init__(self, cfg, sd, n_slots, nb, max_len):
        self.nb, self.max_len = nb, max_len
        self.refs = [T5Fp32(cfg, sd) for _ in range(n_slots)]
        self.admitted, self.pos_seen = [], []

    def admit(self, slots, sources):
        assert len(slots) == len(sources) == len(set(slots))
        self.admitted.append(list(slots))
        for s, enc in zip(slots, sources):
            self.refs[s].start(enc, self.nb, self.max_len)

    def step(self, active, pos, tokens, ancestry):
        nb = self.nb
        assert list(active) == sorted(set(active)) and len(pos) == len(active)
        assert tokens.shape[0] == len(active) * nb and ancestry.shape == (len(active) * nb, max(pos) + 1)
        self.pos_seen.append(list(pos))
        return torch.cat([self.refs[s].step(tokens[a * nb : (a + 1) * nb], ancestry[a * nb : (a + 1) * nb, : pos[a] + 1])
                          for a, s in enumerate(active)])


def run_schedule(schedule, cfg, sd, encs, nb, ml, lp, mutant=None):
    """({ticket: output}, tickets in submission order, the engine) of one schedule over ``encs``."""
    n_slots = 2 if schedule == "5_sources_2_slots" else len(encs)
    eng = PoolRef(cfg, sd, n_slots, nb, ml)
    pool = BeamSearchPool(eng.admit, eng.step, n_slots, nb, ml, lp, mutant=mutant)
    got, tickets = {}, []
    if schedule == "one_every_3_steps":
        for enc in encs:
            tickets.append(pool.submit(enc))
            for _ in range(3):
                got.update(pool.step())
    else:
        tickets = [pool.submit(enc) for enc in encs]
        assert pool.queued == len(encs) and pool.in_flight == 0
    got.update(pool.drain())
    assert pool.queued == 0 and pool.in_flight == 0 and pool.step() == []
    assert sorted(got) == sorted(tickets) and pool.steps == len(eng.pos_seen)
    return got, tickets, eng


@pytest.fixture(scope="module")
def setup(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    ref = T5Fp32(cfg, sd)
    src = z["src"]
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    srcs = [np.asarray(src, dtype=np.int32), cut(40), cut(7), source_ids(120, 11), source_ids(33, 12)]
    alone = {}  # (nb, ml, lp) -> beam_search of every source by itself, computed once and left unchanged

    def alone_for(nb, ml, lp):
        if (nb, ml, lp) not in alone:
            outs = []
            for enc in encs:
                ref.start(enc, nb, ml)
                outs.append(beam_search(ref.step, nb, ml, lp))
            alone[(nb, ml, lp)] = outs
        return alone[(nb, ml, lp)]

    encs = [ref.encode(s) for s in srcs]
    return z, meta, cfg, sd, encs, alone_for


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits, not a tolerance


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", range(24))
def test_pool_equals_beam_search_on_the_g20_grid(setup, case, schedule):
    z, meta, cfg, sd, encs, alone_for = setup
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    got, tickets, eng = run_schedule(schedule, cfg, sd, encs, nb, ml, lp)
    for ticket, want in zip(tickets, alone_for(nb, ml, lp)):
        _same(got[ticket], want)
    # ticket 0 is the G20 source: the committed HuggingFace sequences
    assert np.array_equal(got[tickets[0]].sequences.numpy(), z[f"c{case}_seq"])
    if schedule == "5_sources_2_slots":  # first in, first out into the lowest free slot; slots are taken again
        assert eng.admitted[0] == [0, 1] and sum(len(a) for a in eng.admitted) == 5
        assert all(len(p) <= 2 for p in eng.pos_seen)
    if schedule == "all_at_once":
        assert eng.admitted == [list(range(len(encs)))]


@pytest.mark.parametrize("nb,lp,ml", [(4, 0.0, 64), (8, 1.0, 64)])
def test_staggered_states_stand_at_different_positions_and_the_shared_position_mutant_is_noticed(setup, nb, lp, ml):
    """With a newcomer every three steps the slots of one step stand at different positions (else the schedule shows
    nothing); the pool still equals the lone searches, and handing every slot the largest position does not."""
    z, meta, cfg, sd, encs, alone_for = setup
    want = alone_for(nb, ml, lp)
    got, tickets, eng = run_schedule("one_every_3_steps", cfg, sd, encs, nb, ml, lp)
    assert any(len(set(p)) > 1 for p in eng.pos_seen), eng.pos_seen
    for ticket, w in zip(tickets, want):
        _same(got[ticket], w)
    bad, bad_tickets, _ = run_schedule("one_every_3_steps", cfg, sd, encs, nb, ml, lp, mutant="shared_position")
    differs = [not (b.sequences.shape == w.sequences.shape and torch.equal(b.sequences, w.sequences)
                    and torch.equal(b.sequences_scores, w.sequences_scores))
               for b, w in zip((bad[t] for t in bad_tickets), want)]
    assert any(differs), "the shared-position mutant changed no output: the comparison would not notice it"


def test_pool_arguments(setup):
    z, meta, cfg, sd, encs, alone_for = setup
    nothing = lambda *a: None  # noqa: E731
    with pytest.raises(ValueError):
        BeamSearchPool(nothing, nothing, 2, 4, 1)
    with pytest.raises(ValueError):
        BeamSearchPool(nothing, nothing, 0, 4, 8)
    pool = BeamSearchPool(nothing, nothing, 2, 4, 8)
    assert pool.step() == [] and pool.drain() == [] and pool.steps == 0


# ---- the async front over a fake engine -----------------------------------------------------------------------------------
def fake_output(ids, nb):
    """A stand-in for a beam search's output that depends on the source alone: ``nb`` rows spelling the source's first
    bytes and the row's number (rows 0 and 1 alike, so that de-duplication has work), descending scores."""
    body = [int(x) for x in np.asarray(ids)[:6] if x >= 3]
    rows = [[0] + body + [3 + ord("0") + max(r, 1), 1] for r in range(nb)]
    scores = [-0.25 * r - 0.001 * len(ids) for r in range(nb)]
    return BeamSearchOutput(torch.tensor(rows, dtype=torch.int64), torch.tensor(scores, dtype=torch.float32))


class FakeStream:
    def __init__(self, engine, nb, n_slots, src_cap):
        self.engine, self.nb, self.n_slots, self.src_cap = engine, nb, n_slots, src_cap
        self.waiting, self.running, self.tickets, self.steps = [], [], 0, 0

    queued = property(lambda self: len(self.waiting))
    in_flight = property(lambda self: len(self.running))

    def submit(self, ids):
        assert len(ids) <= self.src_cap
        self.tickets += 1
        self.waiting.append([self.tickets, ids, 1 + len(ids) % 4])  # ticket, source, steps until it stops
        return self.tickets

    def step(self):
        if self.engine.fail_at_step is not None and self.steps == self.engine.fail_at_step:
            raise RuntimeError("the engine fell over")
        while self.waiting and len(self.running) < self.n_slots:
            self.running.append(self.waiting.pop(0))
        self.steps += 1
        self.engine.in_flight_seen.append(len(self.running))
        for r in self.running:
            r[2] -= 1
        done = [(t, fake_output(ids, self.nb)) for t, ids, left in self.running if left == 0]
        self.running = [r for r in self.running if r[2] > 0]
        return done


class FakeEngine:
    def __init__(self):
        self.decoder = SimpleNamespace(max_states=lambda nb: 4)
        self.streams, self.in_flight_seen, self.fail_at_step = [], [], None

    def generate(self, ids, nb, max_len, lp):
        return fake_output(ids, nb)

    def generate_stream(self, nb, max_len, lp, n_slots=None, src_cap=None):
        self.streams.append(FakeStream(self, nb, n_slots or self.decoder.max_states(nb), src_cap))
        return self.streams[-1]


def fake_generator(**kw):
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, **kw)
    gen.generator, gen.tokenizer = FakeEngine(), ByT5Tokenizer()
    return gen


STATES = ["a : Nat", "h : x = y ⊢ y = x", "⊢ True", "n m : Nat ⊢ n + m = m + n", "p q : Prop"]
ARGS = ("f.lean", "thm", Pos(1, 0))


def test_gather_gives_every_call_its_own_result_and_the_driver_stops():
    gen = fake_generator(continuous_slots=2)
    want = [gen.generate_sync(s, *ARGS, 4) for s in STATES]
    assert len({tuple(w) for w in want}) == len(STATES) and all(len(w) == 3 for w in want)  # distinct; de-duplicated

    async def main():
        got = await asyncio.gather(*(gen.generate(s, *ARGS, 4) for s in STATES))
        assert gen._driver is None and not gen._waiters  # the driver ended with the stream idle
        again = await gen.generate(STATES[0], *ARGS, 4)  # ... and a later call starts it anew on the same stream
        assert gen._driver is None
        return got, again

    got, again = asyncio.run(main())
    assert got == want and again == want[0]
    eng = gen.generator
    assert len(eng.streams) == 1 and eng.streams[0].n_slots == 2 and eng.streams[0].src_cap == 64
    assert max(eng.in_flight_seen) == 2  # the calls shared the loop, two slots at a time
    assert eng.streams[0].queued == 0 and eng.streams[0].in_flight == 0


def test_another_num_samples_waits_for_the_drain_then_reopens():
    gen = fake_generator()

    async def main():
        return await asyncio.gather(gen.generate(STATES[0], *ARGS, 4), gen.generate(STATES[1], *ARGS, 2),
                                    gen.generate(STATES[2], *ARGS, 4), gen.generate(STATES[3], *ARGS, 2))

    got = asyncio.run(main())
    assert got == [gen.generate_sync(s, *ARGS, n) for s, n in zip(STATES, (4, 2, 4, 2))]
    streams = gen.generator.streams
    assert len(streams) >= 2 and {s.nb for s in streams} == {2, 4}
    assert all(s.queued == 0 and s.in_flight == 0 for s in streams) and gen._driver is None


def test_a_raising_step_fails_every_waiter_and_the_next_call_gets_a_fresh_stream():
    gen = fake_generator(continuous_slots=2)
    gen.generator.fail_at_step = 1

    async def main():
        res = await asyncio.gather(*(gen.generate(s, *ARGS, 4) for s in STATES), return_exceptions=True)
        assert gen._driver is None and not gen._waiters
        return res

    res = asyncio.run(main())
    # the states that stopped in the one step taken have their results; every other waiter has the exception
    failed = [r for r in res if isinstance(r, Exception)]
    assert len(failed) >= 3 and all(isinstance(r, RuntimeError) and "fell over" in str(r) for r in failed)
    assert all(r == gen.generate_sync(s, *ARGS, 4) for r, s in zip(res, STATES) if not isinstance(r, Exception))
    gen.generator.fail_at_step = None
    assert asyncio.run(gen.generate(STATES[0], *ARGS, 4)) == gen.generate_sync(STATES[0], *ARGS, 4)
    assert len(gen.generator.streams) == 2


def test_retrieval_augmented_generate_retrieves_then_submits():
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, continuous=True, continuous_slots=2)
    rag.hf_gen.generator, rag.hf_gen.tokenizer = FakeEngine(), ByT5Tokenizer()
    seen = []
    rag.retriever = SimpleNamespace(retrieve=lambda state, *a: (seen.append(state), ([], []))[1])

    async def main():
        return await asyncio.gather(*(rag.generate(s, *ARGS, 4) for s in STATES))

    got = asyncio.run(main())
    assert seen == STATES  # every call retrieved before it submitted, in call order
    assert got == [rag.generate_sync(s, *ARGS, 4) for s in STATES]
    assert len(rag.hf_gen.generator.streams) == 1 and max(rag.hf_gen.generator.in_flight_seen) == 2


def test_construction():
    with pytest.raises(ValueError):
        HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, do_sample=True)
    with pytest.raises(ValueError):
        HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, continuous_slots=0)
    with pytest.raises(ValueError):
        RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, continuous=True, do_sample=True)
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0)  # the default: generate() is generate_sync, no stream
    gen.generator, gen.tokenizer = FakeEngine(), ByT5Tokenizer()
    assert asyncio.run(gen.generate(STATES[0], *ARGS, 4)) == gen.generate_sync(STATES[0], *ARGS, 4)
    assert gen.generator.streams == [] and not gen.continuous
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, continuous=True, continuous_slots=3)
    assert rag.hf_gen.continuous and rag.hf_gen.continuous_slots == 3
