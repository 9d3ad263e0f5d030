"""Continuous batching for the sampled search, host side: ``SamplePool`` over the fp32 CPU decoder step
(tests/test_generate_pool_cpu.py's ``PoolRef``) with the float64 reference sampler at a position per slot
(tests/sample_pool_helpers.py) returns, for every ticket, exactly what ``sample_search`` returns for that source alone
with the same step and the same sampler at that ticket's seed - 6 sources through 2 and 3 slots, 1 and 4 samples,
``max_length`` 12 and 3, ``sync_every`` 1, 3 and 16.  The pool's behaviour (positions, slot re-use, admission and delivery
order, the forced sync point at ``max_length - 1``, the copies) is checked on those runs, three planted mutants must be
noticed, the arguments are checked, and the tactic generators' ``sample_stream`` layer is driven over a fake engine.
Every comparison is equality."""
import asyncio
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from sample_helpers import margin_bound  # noqa: E402
from sample_pool_helpers import CpuPoolSampler  # noqa: E402
from test_generate_pool_cpu import ARGS, STATES, PoolRef  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.generation import (SAMPLE_POOL_MUTANTS, BeamSearchOutput, SamplePool, SampleState,  # noqa: E402
                                     sample_books_admit_host, sample_books_rows_host, sample_search)
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402

KW = dict(temperature=1.2, top_k=50, top_p=0.95)
SEEDS = [41, 42, 43, 44, 0xFFFFFFF5, 46]  # one per source (one with its top bit set)
EOS_BOOST = 4.0
EOS = 1


@pytest.fixture(scope="module")
def setup(hip_lib):
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][EOS] *= EOS_BOOST  # some samples stop early: the states end at different lengths
    ref = T5Fp32(cfg, sd)
    srcs = [source_ids(60, 3), source_ids(7, 4), source_ids(33, 5), source_ids(120, 6), source_ids(1, 7), source_ids(20, 8)]
    encs = [ref.encode(s) for s in srcs]
    alone = {}  # (nb, ml) -> (sample_search of every source by itself, the smallest margin): once, left unchanged

    def alone_for(nb, ml):
        if (nb, ml) not in alone:
            outs, margin = [], np.inf
            for enc, seed in zip(encs, SEEDS):
                ref.start(enc, nb, ml)
                sampler = CpuPoolSampler(hip_lib, **KW)
                outs.append(sample_search(lambda tok, anc, t: ref.step(tok.long(), anc[:, : t + 1].long()), sampler.at, nb,
                                          ml, seed))
                margin = min(margin, sampler.min_margin)
            alone[(nb, ml)] = (outs, margin)
        return alone[(nb, ml)]

    return cfg, sd, encs, alone_for


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits, not a tolerance


def _differs(a, b):
    return not (a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences)
                and torch.equal(a.sequences_scores, b.sequences_scores))


def _ends(out, ml):
    """(generated length of the state, "eos" when every sample drew EOS else "length")"""
    rows = [r[1:].tolist() for r in out.sequences]
    return out.sequences.shape[1] - 1, "eos" if all(EOS in r for r in rows) else "length"


def run_pool(hip_lib, cfg, sd, encs, seeds, n_slots, nb, ml, k, schedule="all_at_once", mutant=None, on_step=None):
    """({ticket: output}, tickets in submission order, the engine, the pool, the sampler, a log) of one run: ``log`` holds
    to_host's copy sizes, the free slots seen at every admission and the per-step deliveries."""
    eng = PoolRef(cfg, sd, n_slots, nb, ml)
    sampler = CpuPoolSampler(hip_lib, **KW)
    log = SimpleNamespace(copies=[], free_at_admit=[], admitted_sources=[], delivered=[])

    def to_host(x):
        log.copies.append(tuple(x.shape))
        return x.cpu()

    def admit(slots, sources):
        log.free_at_admit.append([s for s in range(n_slots) if pool._ticket[s] is None])
        log.admitted_sources.extend(next(i for i, e in enumerate(encs) if e is src) for src in sources)
        eng.admit(slots, sources)

    def step(active, pos, tokens, ancestry):
        assert tokens.dtype == torch.int32 and ancestry.dtype == torch.int32
        assert tokens.shape == (len(active) * nb,) and ancestry.shape == (len(active) * nb, ml)
        assert all(0 <= p and p + 1 < ml for p in pos), pos  # no step carries pos + 1 >= max_length
        return eng.step(active, pos, tokens.long(), ancestry[:, : max(pos) + 1].long())

    pool = SamplePool(admit, step, sampler, n_slots, nb, ml, sync_every=k, to_host=to_host, mutant=mutant)
    got, tickets = {}, []

    def one_step():
        before = pool.sync_points
        pairs = pool.step()
        assert not set(t for t, _ in pairs) & set(got)  # a ticket is delivered once
        got.update(pairs)
        log.delivered.append([t for t, _ in pairs])
        if on_step is not None:
            on_step(pool, pairs, before, sampler)

    if schedule == "one_every_2_steps":
        for enc, seed in zip(encs, seeds):
            tickets.append(pool.submit(enc, seed))
            for _ in range(2):
                one_step()
    else:
        tickets = [pool.submit(enc, seed) for enc, seed in zip(encs, seeds)]
        assert pool.queued == len(encs) and pool.in_flight == 0
    while pool.queued or pool.in_flight:
        one_step()
    assert pool.step() == [] and pool.drain() == []
    assert sorted(got) == sorted(tickets) and pool.steps == len(eng.pos_seen) == len(sampler.calls)
    return got, tickets, eng, pool, sampler, log


# ---- the pool against the lockstep search ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("ml", [12, 3])
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("n_slots", [2, 3])
def test_pool_equals_sample_search_alone(hip_lib, setup, n_slots, nb, ml, k):
    cfg, sd, encs, alone_for = setup
    want, margin = alone_for(nb, ml)
    ends = [_ends(w, ml) for w in want]
    print("ends:", ends, "smallest margin alone:", margin)
    # the runs alone show what the comparison needs: different lengths, and at max_length 12 both kinds of end
    if ml == 12:
        assert len({n for n, _ in ends}) > 1, ends
        assert any(how == "eos" and n < ml - 1 for n, how in ends) and any(how == "length" for _, how in ends), ends
    else:
        assert any(how == "length" for _, how in ends), ends  # two positions: states end by length
    got, tickets, eng, pool, sampler, log = run_pool(hip_lib, cfg, sd, encs, SEEDS, n_slots, nb, ml, k)
    for ticket, w in zip(tickets, want):
        _same(got[ticket], w)
    # no decision of the sampler on these inputs lies inside the fp32 bound: nothing had to be left out
    V = cfg["vocab_size"]
    print("smallest margin in the pool:", sampler.min_margin, "bound:", margin_bound(V))
    assert margin > margin_bound(V) and sampler.min_margin > margin_bound(V)
    assert len(log.copies) <= 2 * pool.sync_points
    assert sum(len(a) for a in eng.admitted) == len(encs) and all(len(p) <= n_slots for p in eng.pos_seen)


# ---- the pool's behaviour ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,schedule", [(1, "all_at_once"), (3, "all_at_once"), (16, "one_every_2_steps")])
def test_positions_slots_order_and_copies(hip_lib, setup, k, schedule):
    """(With everything there at the start and ``sync_every`` 16 two slots run in lockstep to ``max_length``: that
    interval gets the staggered arrivals.)"""
    cfg, sd, encs, alone_for = setup
    n_slots, nb, ml = 2, 4, 12
    want, _ = alone_for(nb, ml)
    got, tickets, eng, pool, sampler, log = run_pool(hip_lib, cfg, sd, encs, SEEDS, n_slots, nb, ml, k, schedule=schedule)
    print("positions per step:", eng.pos_seen, "admitted:", eng.admitted, "delivered:", log.delivered)
    assert any(len(set(p)) > 1 for p in eng.pos_seen), eng.pos_seen       # some step carries two different positions
    assert [c[1] for c in sampler.calls] == eng.pos_seen                   # ... and the sampler is handed the step's own
    slots = [s for a in eng.admitted for s in a]
    assert len(slots) == len(encs) > len(set(slots))                       # a slot is reused
    assert log.admitted_sources == list(range(len(encs)))                  # first in, first out
    assert eng.admitted[0] == ([0, 1] if schedule == "all_at_once" else [0])
    for taken, free in zip(eng.admitted, log.free_at_admit):               # the lowest free slots, ascending
        assert taken == free[: len(taken)]
    slot_of = {}
    for taken, first in zip(eng.admitted, np.cumsum([0] + [len(a) for a in eng.admitted[:-1]])):
        slot_of.update({tickets[first + j]: s for j, s in enumerate(taken)})
    for pairs in log.delivered:
        assert [slot_of[t] for t in pairs] == sorted(slot_of[t] for t in pairs)  # within a sync point, by slot
    for ticket, w in zip(tickets, want):
        _same(got[ticket], w)
    assert len(log.copies) <= 2 * pool.sync_points, (log.copies, pool.sync_points)
    row = nb * ml + 2 * nb
    for shape in log.copies:  # the reduced flags, or one result buffer of the stopped states: never the books
        assert shape == (n_slots,) or (len(shape) == 2 and 1 <= shape[0] <= n_slots and shape[1] == row), shape
    assert sum(s[0] for s in log.copies if len(s) == 2) == len(encs)  # every state read once


def test_with_k_1_a_state_is_delivered_in_the_step_where_it_ended(hip_lib, setup):
    cfg, sd, encs, alone_for = setup
    nb, ml = 4, 12
    want, _ = alone_for(nb, ml)
    got, tickets, eng, pool, sampler, log = run_pool(hip_lib, cfg, sd, encs, SEEDS, len(encs), nb, ml, 1)
    assert eng.admitted == [list(range(len(encs)))]
    for i, t in enumerate(tickets):  # all admitted at step 0: delivered at the step that is the state's own length
        at = next(step for step, pairs in enumerate(log.delivered) if t in pairs)
        assert at + 1 == _ends(want[i], ml)[0], (i, at)
    assert pool.steps == max(_ends(w, ml)[0] for w in want)


@pytest.mark.parametrize("ml", [3, 12])
def test_the_forced_sync_point_at_max_length(hip_lib, setup, ml):
    """``sync_every`` 16 never comes due here: a state that ran to ``max_length`` leaves at the sync point forced after
    the step that took its slot to ``max_length - 1``, and is not stepped again."""
    cfg, sd, encs, alone_for = setup
    nb, n_slots = 4, 2
    want, _ = alone_for(nb, ml)
    forced = []

    def on_step(pool, pairs, syncs_before, sampler):
        act, pos = sampler.calls[-1]
        if any(p + 2 >= ml for p in pos):  # this step took a slot to max_length - 1
            assert pool._since == 0 and pool.sync_points > syncs_before
            forced.append(pool.steps)
            assert all(pool._ticket[s] is None or pool._pos[s] + 1 < ml for s in range(n_slots))

    got, tickets, eng, pool, sampler, log = run_pool(hip_lib, cfg, sd, encs, SEEDS, n_slots, nb, ml, 16, on_step=on_step)
    assert forced, "no slot reached max_length - 1: the run shows nothing"
    assert all(p + 1 < ml for ps in eng.pos_seen for p in ps)
    if ml == 3:
        assert pool.steps < 16  # sync_every never came due: every departure was at a forced sync point
    for ticket, w in zip(tickets, want):
        _same(got[ticket], w)


@pytest.mark.parametrize("mutant", SAMPLE_POOL_MUTANTS)
def test_the_planted_mutants_are_noticed(hip_lib, setup, mutant):
    cfg, sd, encs, alone_for = setup
    nb, ml = 4, 12
    want, _ = alone_for(nb, ml)
    assert SAMPLE_POOL_MUTANTS == ("shared_position", "admit_not_reset", "stale_tokens")
    # staggered arrivals through two slots: different positions in one step, slots taken again, lists that change
    good, tickets, _, _, _, _ = run_pool(hip_lib, cfg, sd, encs, SEEDS, 2, nb, ml, 1, schedule="one_every_2_steps")
    for ticket, w in zip(tickets, want):
        _same(good[ticket], w)
    bad, bad_tickets, _, _, _, _ = run_pool(hip_lib, cfg, sd, encs, SEEDS, 2, nb, ml, 1, schedule="one_every_2_steps",
                                            mutant=mutant)
    assert any(_differs(bad[t], w) for t, w in zip(bad_tickets, want)), \
        f"the {mutant} mutant changed no output: the comparison would not notice it"


def test_the_host_restatements_touch_their_own_parts_only():
    n, nb, L = 3, 2, 5
    st = SampleState(seeds=torch.full((n,), 7, dtype=torch.int32), seq=torch.full((n, nb, L), 9, dtype=torch.int32),
                     cum_logprob=torch.full((n, nb), -3.0), n_generated=torch.full((n, nb), 4, dtype=torch.int32),
                     finished=torch.ones((n, nb), dtype=torch.int32), tokens=torch.full((n * nb,), 5, dtype=torch.int32))
    sample_books_admit_host(st, [2, 0], [0xFFFFFFFF, 11], decoder_start_token_id=8, pad_token_id=6)
    assert st.seeds.tolist() == [11, 7, -1]
    for s in (0, 2):
        assert st.seq[s].tolist() == [[8, 6, 6, 6, 6]] * nb
        assert st.cum_logprob[s].tolist() == [0.0] * nb and st.n_generated[s].tolist() == [0] * nb
        assert st.finished[s].tolist() == [0] * nb
    assert (st.seq[1] == 9).all() and (st.finished[1] == 1).all() and (st.n_generated[1] == 4).all()
    assert (st.cum_logprob[1] == -3.0).all() and (st.tokens == 5).all()  # nothing by row
    st.seq[1, :, 3] = torch.tensor([21, 22], dtype=torch.int32)
    sample_books_rows_host(st, [1, 2], [3, 0])
    assert st.tokens.tolist() == [21, 22, 8, 8, 5, 5]


def test_pool_arguments():
    nothing = lambda *a: None  # noqa: E731
    for bad in (dict(n_slots=0), dict(num_samples=0), dict(max_length=1), dict(sync_every=0), dict(sync_every=-1),
                dict(sync_every=1.5)):
        kw = dict(n_slots=2, num_samples=4, max_length=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            SamplePool(nothing, nothing, nothing, **kw)
    pool = SamplePool(nothing, nothing, nothing, 2, 4, 8, sync_every=2)
    assert pool.step() == [] and pool.drain() == [] and pool.steps == 0 and pool.sync_points == 0
    assert pool.queued == 0 and pool.in_flight == 0
    assert pool.ancestry.tolist() == [[p * 4 + r % 4 for p in range(8)] for r in range(8)]


# ---- the tactic generators' layer over a fake engine ------------------------------------------------------------------------
def fake_sampled(ids, seed, nb):
    """A stand-in for a sampled search's output that depends on (source, seed): ``nb`` rows spelling the source's first
    bytes and a digit drawn from the seed (rows 0 and 1 alike, so that de-duplication has work), scores in an order the
    seed decides (so that the sort has work)."""
    body = [int(x) for x in np.asarray(ids)[:6] if x >= 3]
    rows = [[0] + body + [3 + ord("0") + (seed + max(r, 1)) % 10, 1] for r in range(nb)]
    scores = [-0.25 * ((r + seed) % nb) - 0.001 * len(ids) - 1e-6 * (seed % 97) for r in range(nb)]
    return BeamSearchOutput(torch.tensor(rows, dtype=torch.int64), torch.tensor(scores, dtype=torch.float32))


class FakeSampleStream:
    def __init__(self, engine, nb, n_slots, src_cap, sync_every):
        self.engine, self.nb, self.n_slots, self.src_cap, self.sync_every = engine, nb, n_slots, src_cap, sync_every
        self.waiting, self.running, self.tickets, self.steps, self.failed = [], [], 0, 0, False

    queued = property(lambda self: len(self.waiting))
    in_flight = property(lambda self: len(self.running))

    def submit(self, ids, seed):
        assert len(ids) <= self.src_cap
        self.tickets += 1
        self.waiting.append([self.tickets, ids, seed, 1 + len(ids) % 4])  # ticket, source, seed, steps until it stops
        return self.tickets

    def step(self):
        if self.engine.fail_at_step is not None and self.steps == self.engine.fail_at_step:
            self.failed = True
            raise RuntimeError("the engine fell over")
        while self.waiting and len(self.running) < self.n_slots:
            self.running.append(self.waiting.pop(0))
        self.steps += 1
        self.engine.in_flight_seen.append(len(self.running))
        for r in self.running:
            r[3] -= 1
        done = [(t, fake_sampled(ids, seed, self.nb)) for t, ids, seed, left in self.running if left == 0]
        self.running = [r for r in self.running if r[3] > 0]
        return done


class FakeSampleEngine:
    def __init__(self):
        self.decoder = SimpleNamespace(max_states=lambda nb: 4)
        self.streams, self.stream_args, self.in_flight_seen, self.fail_at_step = [], [], [], None

    def sample_many(self, sources, nb, max_len, temperature, top_k, top_p, seeds, lp):
        return [fake_sampled(ids, seed, nb) for ids, seed in zip(sources, seeds)]

    def sample_stream(self, nb, max_len, temperature, top_k, top_p, lp, n_slots=None, src_cap=None, sync_every=16):
        assert all(s.failed or (s.queued == 0 and s.in_flight == 0) for s in self.streams)  # the last one has drained
        self.stream_args.append((nb, max_len, temperature, top_k, top_p, lp, n_slots, src_cap, sync_every))
        self.streams.append(FakeSampleStream(self, nb, n_slots or self.decoder.max_states(nb), src_cap, sync_every))
        return self.streams[-1]


def fake_generator(seed=5, **kw):
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.5, do_sample=True, temperature=0.8, top_k=40, top_p=0.9,
                               seed=seed, **kw)
    gen.generator, gen.tokenizer = FakeSampleEngine(), ByT5Tokenizer()
    return gen


def test_gather_equals_sequential_generate_sync_on_a_fresh_object():
    gen = fake_generator(sample_stream=True, sample_stream_slots=2, sample_sync_every=3)
    fresh = fake_generator()
    want = [fresh.generate_sync(s, *ARGS, 4) for s in STATES]
    assert len({tuple(w) for w in want}) == len(STATES) and all(len(w) == 3 for w in want)  # distinct; de-duplicated
    assert all([sc for _, sc in w] == sorted((sc for _, sc in w), reverse=True) for w in want)  # best first
    assert want != [fake_generator().generate_sync(s, *ARGS, 4) for s in STATES[::-1]][::-1]  # the seeds follow call order

    async def main():
        got = await asyncio.gather(*(gen.generate(s, *ARGS, 4) for s in STATES))
        assert gen._driver is None and not gen._waiters  # the driver ended with the stream idle
        return got

    assert asyncio.run(main()) == want
    eng = gen.generator
    assert eng.stream_args == [(4, 16, 0.8, 40, 0.9, 0.5, 2, 64, 3)]
    assert max(eng.in_flight_seen) == 2 and eng.streams[0].queued == 0 and eng.streams[0].in_flight == 0
    assert gen.states_served == fresh.states_served == len(STATES)
    # generate_sync / batch_generate_sync stay as they are: sample_many, the next seeds
    assert gen.generate_sync(STATES[0], *ARGS, 4) == fresh.generate_sync(STATES[0], *ARGS, 4)
    assert gen.batch_generate_sync(STATES[:2], [ARGS[0]] * 2, [ARGS[1]] * 2, [ARGS[2]] * 2, 4) == \
        fresh.batch_generate_sync(STATES[:2], [ARGS[0]] * 2, [ARGS[1]] * 2, [ARGS[2]] * 2, 4)
    assert len(eng.streams) == 1


def test_another_num_samples_waits_for_the_drain_then_reopens():
    gen = fake_generator(sample_stream=True)

    async def main():
        return await asyncio.gather(gen.generate(STATES[0], *ARGS, 4), gen.generate(STATES[1], *ARGS, 2),
                                    gen.generate(STATES[2], *ARGS, 4), gen.generate(STATES[3], *ARGS, 2))

    got = asyncio.run(main())
    streams = gen.generator.streams
    assert len(streams) >= 2 and {s.nb for s in streams} == {2, 4}
    assert all(s.queued == 0 and s.in_flight == 0 for s in streams) and gen._driver is None
    # (the fake engine asserts that a stream is opened only after the one before it has drained)
    assert [len(r) for r in got] == [3, 1, 3, 1]  # every call got an output of its own num_samples, de-duplicated
    assert gen.states_served == 4


def test_a_raising_step_fails_every_waiter_and_the_next_call_gets_a_fresh_stream():
    gen = fake_generator(sample_stream=True, sample_stream_slots=2)
    gen.generator.fail_at_step = 1

    async def main():
        res = await asyncio.gather(*(gen.generate(s, *ARGS, 4) for s in STATES), return_exceptions=True)
        assert gen._driver is None and not gen._waiters
        return res

    res = asyncio.run(main())
    failed = [r for r in res if isinstance(r, Exception)]
    assert len(failed) >= 3 and all(isinstance(r, RuntimeError) and "fell over" in str(r) for r in failed)
    fresh = fake_generator()
    want = [fresh.generate_sync(s, *ARGS, 4) for s in STATES]
    assert all(r == w for r, w in zip(res, want) if not isinstance(r, Exception))
    gen.generator.fail_at_step = None
    assert asyncio.run(gen.generate(STATES[0], *ARGS, 4)) == fresh.generate_sync(STATES[0], *ARGS, 4)
    assert len(gen.generator.streams) == 2


def test_retrieval_augmented_generator_forwards_the_keywords():
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.5, 10, do_sample=True, temperature=0.8, top_k=40,
                                      top_p=0.9, seed=5, sample_stream=True, sample_stream_slots=2, sample_sync_every=3)
    hf = rag.hf_gen
    assert hf.sample_stream and hf.sample_stream_slots == 2 and hf.sample_sync_every == 3 and not hf.continuous
    hf.generator, hf.tokenizer = FakeSampleEngine(), ByT5Tokenizer()
    seen = []
    rag.retriever = SimpleNamespace(retrieve=lambda state, *a: (seen.append(state), ([], []))[1])

    async def main():
        return await asyncio.gather(*(rag.generate(s, *ARGS, 4) for s in STATES))

    got = asyncio.run(main())
    assert seen == STATES  # every call retrieved before it submitted, in call order
    fresh = fake_generator()
    assert got == [fresh.generate_sync(s, *ARGS, 4) for s in STATES]
    assert len(hf.generator.streams) == 1 and max(hf.generator.in_flight_seen) == 2


def test_construction():
    base = ("unused", "cpu", 64, 16, 0.0)
    with pytest.raises(ValueError):  # sampling stays refused with continuous=True
        HuggingFaceGenerator(*base, continuous=True, do_sample=True)
    with pytest.raises(ValueError):
        RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, continuous=True, do_sample=True)
    with pytest.raises(ValueError, match="sample_stream"):
        HuggingFaceGenerator(*base, sample_stream=True)  # without do_sample
    with pytest.raises(ValueError, match="sample_stream"):
        HuggingFaceGenerator(*base, sample_stream=True, continuous=True)
    with pytest.raises(ValueError):
        HuggingFaceGenerator(*base, sample_stream=True, continuous=True, do_sample=True)
    with pytest.raises(ValueError, match="sample_stream"):
        RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, sample_stream=True)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sample_stream_slots"):
            HuggingFaceGenerator(*base, do_sample=True, sample_stream=True, sample_stream_slots=bad)
        with pytest.raises(ValueError, match="sample_sync_every"):
            HuggingFaceGenerator(*base, do_sample=True, sample_stream=True, sample_sync_every=bad)
    gen = HuggingFaceGenerator(*base, do_sample=True)  # the default: generate() is generate_sync, no stream
    gen.generator, gen.tokenizer = FakeSampleEngine(), ByT5Tokenizer()
    assert asyncio.run(gen.generate(STATES[0], *ARGS, 4)) == fake_generator(seed=0).generate_sync(STATES[0], *ARGS, 4)
    assert gen.generator.streams == [] and not gen.sample_stream
