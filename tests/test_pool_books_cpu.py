"""Continuous batching with the books in a ``BeamBooks`` block, host side: ``BeamBooksPool`` over the fp32 CPU decoder
step with the host restatements of the three pool-books kernels (``beam_books_admit_host``, ``beam_pool_advance_host``,
``beam_books_rows_host``) returns, for every ticket, exactly what ``beam_search`` returns for that source alone - on every
G20 grid point, under the three schedules of tests/test_generate_pool_cpu.py, for ``sync_every`` 1, 3 and 16.  Two planted
mutants must be noticed; a stopped state is delivered at the next sync point and frozen meanwhile; the device-to-host
copies are counted; the arguments are checked.  Everything is compared bit for bit."""
import asyncio
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32  # noqa: E402
from test_generate_pool_cpu import ARGS, SCHEDULES, STATES, FakeStream, _same, fake_output, setup  # noqa: E402, F401
from reprover_amd.generation import (POOL_BOOKS_MUTANTS, BeamBooks, BeamBooksPool, beam_advance_host,  # noqa: E402
                                     beam_books_admit_host, beam_books_init_host, beam_books_rows_host,
                                     beam_pool_advance_host)
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402

BY_STATE = ("run_seq", "anc", "fin_seq", "run_scores", "beam_scores", "fin_flag", "fin_len", "heur", "done", "steps")


class BooksRef:
    """``admit`` / ``step`` over one fp32 reference decoder (and cache) per slot, fed from the books' by-row views."""

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
        assert all(0 <= p <= self.max_len - 2 for p in pos)  # no launch carries pos + 1 >= max_len
        assert tokens.dtype == torch.int32 and ancestry.dtype == torch.int32
        assert tokens.shape == (len(active) * nb,) and ancestry.shape == (len(active) * nb, self.max_len)
        self.pos_seen.append(list(pos))
        return torch.cat([self.refs[s].step(tokens[a * nb : (a + 1) * nb].long(),
                                            ancestry[a * nb : (a + 1) * nb, : pos[a] + 1].long())
                          for a, s in enumerate(active)])


def run_books(schedule, cfg, sd, encs, nb, ml, lp, k, mutant=None, n_slots=None, on_step=None):
    """({ticket: output}, tickets in submission order, the engine, the pool, to_host's copy sizes) of one schedule."""
    if n_slots is None:
        n_slots = 2 if schedule == "5_sources_2_slots" else len(encs)
    eng = BooksRef(cfg, sd, n_slots, nb, ml)
    copies = []

    def to_host(x):
        copies.append(tuple(x.shape))
        return x.cpu()

    pool = BeamBooksPool(eng.admit, eng.step, n_slots, nb, ml, lp, sync_every=k, to_host=to_host, mutant=mutant)
    got, tickets = {}, []

    def step():
        pairs = pool.step()
        assert not set(t for t, _ in pairs) & set(got)  # a ticket is delivered once
        got.update(pairs)
        if on_step is not None:
            on_step(pool, pairs)

    if schedule == "one_every_3_steps":
        for enc in encs:
            tickets.append(pool.submit(enc))
            for _ in range(3):
                step()
    else:
        tickets = [pool.submit(enc) for enc in encs]
        assert pool.queued == len(encs) and pool.in_flight == 0
    while pool.queued or pool.in_flight:
        step()
    assert pool.step() == [] and pool.drain() == []
    assert sorted(got) == sorted(tickets) and pool.steps == len(eng.pos_seen)
    return got, tickets, eng, pool, copies


def _check_copies(pool, eng, copies, k, nb, ml):
    """At most two copies per sync point (the ``n_slots`` flags, one result buffer of the stopped states only), and at
    most ceil(steps / K) + admissions + 1 sync points."""
    assert len(copies) <= 2 * pool.sync_points, (copies, pool.sync_points)
    assert pool.sync_points <= -(-pool.steps // k) + len(eng.admitted) + 1, (pool.sync_points, pool.steps, k)
    row = nb * ml + 2 * nb + 1
    for shape in copies:
        assert shape == (pool.n_slots,) or (len(shape) == 2 and 1 <= shape[0] <= pool.n_slots and shape[1] == row), shape
    assert sum(s[0] for s in copies if len(s) == 2) == sum(len(a) for a in eng.admitted)  # every state read once


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", range(24))
def test_books_pool_equals_beam_search_on_the_g20_grid(setup, case, schedule, k):  # noqa: F811
    z, meta, cfg, sd, encs, alone_for = setup
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    got, tickets, eng, pool, copies = run_books(schedule, cfg, sd, encs, nb, ml, lp, k)
    for ticket, want in zip(tickets, alone_for(nb, ml, lp)):
        _same(got[ticket], want)
    _check_copies(pool, eng, copies, k, nb, ml)
    if schedule == "5_sources_2_slots":  # first in, first out into the lowest free slot; slots are taken again
        assert eng.admitted[0] == [0, 1] and sum(len(a) for a in eng.admitted) == 5
        assert all(len(p) <= 2 for p in eng.pos_seen)
    if schedule == "all_at_once":
        assert eng.admitted == [list(range(len(encs)))]


def _differs(a, b):
    return not (a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences)
                and torch.equal(a.sequences_scores, b.sequences_scores))


@pytest.mark.parametrize("nb,lp,ml", [(4, 0.0, 64), (8, 1.0, 64)])
def test_the_shared_position_mutant_is_noticed(setup, nb, lp, ml):  # noqa: F811
    """With a newcomer every three steps the slots of one step stand at different positions, of both parities; handing
    every slot's advance the largest of them changes an output."""
    z, meta, cfg, sd, encs, alone_for = setup
    want = alone_for(nb, ml, lp)
    got, tickets, eng, _, _ = run_books("one_every_3_steps", cfg, sd, encs, nb, ml, lp, 1)
    assert any(len({p & 1 for p in ps}) > 1 for ps in eng.pos_seen), eng.pos_seen
    for ticket, w in zip(tickets, want):
        _same(got[ticket], w)
    bad, bad_tickets, _, _, _ = run_books("one_every_3_steps", cfg, sd, encs, nb, ml, lp, 1, mutant="shared_position")
    assert any(_differs(bad[t], w) for t, w in zip(bad_tickets, want)), \
        "the shared-position mutant changed no output: the comparison would not notice it"


def test_the_admit_not_reset_mutant_is_noticed(setup):  # noqa: F811
    """One slot, taken a second time by a source whose search stops earlier than its predecessor's: without the reset
    of the row tables the block (or an output) differs from the sound pool's."""
    z, meta, cfg, sd, encs, alone_for = setup
    nb, lp, ml = 4, 0.0, 64
    want = alone_for(nb, ml, lp)
    _, _, _, pool, _ = run_books("all_at_once", cfg, sd, encs, nb, ml, lp, 1)
    stops = pool.books.steps.tolist()  # all admitted at step 0 into slots 0 .. 4: the searches' own lengths
    print("stop steps:", stops)
    long, short = max(range(len(encs)), key=lambda i: stops[i]), min(range(len(encs)), key=lambda i: stops[i])
    assert stops[long] > stops[short] + 3, stops
    pair = [encs[long], encs[short]]
    good, tickets, _, good_pool, _ = run_books("all_at_once", cfg, sd, pair, nb, ml, lp, 1, n_slots=1)
    _same(good[tickets[0]], want[long])
    _same(good[tickets[1]], want[short])
    bad, bad_tickets, eng, bad_pool, _ = run_books("all_at_once", cfg, sd, pair, nb, ml, lp, 1, n_slots=1,
                                                   mutant="admit_not_reset")
    assert eng.admitted == [[0], [0]]
    assert (not torch.equal(bad_pool.books.block, good_pool.books.block)
            or any(_differs(bad[t], good[g]) for t, g in zip(bad_tickets, tickets))), \
        "the admit-not-reset mutant changed neither the block nor an output"
    assert "admit_not_reset" in POOL_BOOKS_MUTANTS and "shared_position" in POOL_BOOKS_MUTANTS


@pytest.mark.parametrize("k", [3, 4])
def test_a_stopped_state_is_delivered_at_the_next_sync_point_and_frozen_meanwhile(setup, k):  # noqa: F811
    z, meta, cfg, sd, encs, alone_for = setup
    nb, lp, ml = 4, 0.0, 64
    stopped_at, snapshot, delivered_at, frozen = {}, {}, {}, []
    slot_of = {}

    def parts(bk, s):
        return [getattr(bk, f)[:, s].clone() if f in ("run_seq", "anc", "fin_seq") else getattr(bk, f)[s].clone()
                for f in BY_STATE]

    def on_step(pool, pairs):
        bk = pool.books
        for ticket, _ in pairs:
            s = slot_of[ticket]
            delivered_at[ticket] = pool.steps
            if ticket in snapshot:  # it stopped in an earlier step
                frozen.append(all(torch.equal(a, b) for a, b in zip(parts(bk, s), snapshot[ticket])))
        for s, ticket in enumerate(pool._ticket):
            if ticket is not None:
                slot_of[ticket] = s
                if int(bk.done[s]) and ticket not in stopped_at:
                    stopped_at[ticket], snapshot[ticket] = pool.steps, parts(bk, s)
        for ticket, _ in pairs:  # (delivered in the step it stopped in: the step's own sync point)
            stopped_at.setdefault(ticket, pool.steps)

    got, tickets, eng, pool, copies = run_books("all_at_once", cfg, sd, encs, nb, ml, lp, k, on_step=on_step)
    for ticket, want in zip(tickets, alone_for(nb, ml, lp)):
        _same(got[ticket], want)
    print("stopped at", stopped_at, "delivered at", delivered_at)
    assert len(set(stopped_at.values())) > 1  # the states stop at different steps
    late = [delivered_at[t] - stopped_at[t] for t in tickets]
    assert all(0 <= d <= k - 1 for d in late) and max(late) > 0, late
    # all were admitted at step 0 and nothing was queued afterwards: the sync points are the multiples of K
    assert all(delivered_at[t] == -(-stopped_at[t] // k) * k for t in tickets)
    assert frozen and all(frozen)
    _check_copies(pool, eng, copies, k, nb, ml)


def test_the_uniform_restatement_is_the_pool_restatement_with_one_position():
    """``beam_advance_host`` (its callers and tests/test_beam_books_*.py keep their behaviour) and
    ``beam_pool_advance_host`` with every ``pos = t`` leave the same block; ``beam_books_admit_host`` of every state is
    ``beam_books_init_host``'s by-state part, and ``beam_books_rows_host`` its by-row part."""
    n, nb, ml = 3, 3, 8
    g = torch.Generator().manual_seed(5)
    a, b = beam_books_init_host(n, nb, ml, 1, 0), BeamBooks(n, nb, ml)
    b.block.fill_(0x5A5A5A5A)
    beam_books_admit_host(b, [2, 0, 1], 1, 0)
    beam_books_rows_host(b, [0, 1, 2], [0, 0, 0])
    for f in BY_STATE + ("tokens", "running", "anc_rows"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    b = BeamBooks(n, nb, ml, block=a.block.clone())
    for t in range(ml - 1):
        active = [[0, 1, 2], [2, 0], [1, 2, 0]][t % 3]
        sc = torch.sort(-9.0 * torch.rand((len(active), 2 * nb), generator=g), descending=True)[0]
        tk = torch.randint(1, 9, (len(active), 2 * nb), generator=g, dtype=torch.int32)
        pr = torch.randint(0, nb, (len(active), 2 * nb), generator=g, dtype=torch.int32)
        beam_advance_host(a, active, t, sc, tk, pr, float(t + 1), float(t + 1), 1)
        k = len(active)
        beam_pool_advance_host(b, active, [t] * k, sc, tk, pr, [float(t + 1)] * k, [float(t + 1)] * k, 1)
        assert torch.equal(a.block, b.block), t


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_sync_every_is_checked():
    nothing = lambda *a: None  # noqa: E731
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sync_every"):
            BeamBooksPool(nothing, nothing, 2, 4, 8, sync_every=bad)
        with pytest.raises(ValueError, match="beam_sync_every"):
            HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, beam_sync_every=bad)
    with pytest.raises(ValueError):
        BeamBooksPool(nothing, nothing, 2, 4, 1, sync_every=2)
    with pytest.raises(ValueError):
        BeamBooksPool(nothing, nothing, 0, 4, 8, sync_every=2)
    with pytest.raises(ValueError):  # sampling stays refused with continuous=True
        HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, beam_sync_every=4, do_sample=True)
    pool = BeamBooksPool(nothing, nothing, 2, 4, 8, sync_every=2)
    assert pool.step() == [] and pool.drain() == [] and pool.steps == 0 and pool.sync_points == 0


class FakeEngine:
    """tests/test_generate_pool_cpu.py's fake engine; ``generate_stream`` records the keywords it was opened with."""

    def __init__(self):
        self.decoder = SimpleNamespace(max_states=lambda nb: 4)
        self.streams, self.stream_kw, self.in_flight_seen, self.fail_at_step = [], [], [], None

    def generate(self, ids, nb, max_len, lp, **kw):
        return fake_output(ids, nb)

    def generate_stream(self, nb, max_len, lp, n_slots=None, src_cap=None, **kw):
        self.stream_kw.append(kw)
        self.streams.append(FakeStream(self, nb, n_slots or self.decoder.max_states(nb), src_cap))
        return self.streams[-1]


@pytest.mark.parametrize("rag", [False, True])
@pytest.mark.parametrize("k", [None, 4])
def test_beam_sync_every_reaches_the_stream(k, rag):
    if rag:
        top = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, continuous=True, continuous_slots=2,
                                          beam_sync_every=k)
        top.retriever = SimpleNamespace(retrieve=lambda state, *a: ([], []))
        gen = top.hf_gen
    else:
        top = gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, continuous=True, continuous_slots=2,
                                         beam_sync_every=k)
    gen.generator, gen.tokenizer = FakeEngine(), ByT5Tokenizer()

    async def main():
        return await asyncio.gather(*(top.generate(s, *ARGS, 4) for s in STATES))

    got = asyncio.run(main())
    assert got == [top.generate_sync(s, *ARGS, 4) for s in STATES]
    assert gen.generator.stream_kw == ([{}] if k is None else [{"sync_every": 4}])
