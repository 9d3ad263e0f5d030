"""Sampling parameters per request, host side: ``SamplingParams`` (broadcast, ladder, the bits of the table, every
refusal), the share of rows the float64 reference leaves out on the mixed-table kernel test's inputs, ``SamplePool`` with
``per_request=True`` over the fp32 CPU decoder step against the search of every source alone (seven tickets of four
parameter sets and four live-row counts through three slots; three planted mutants must be noticed), the default pool
calling its callbacks exactly as before, and the tactic generators' ``sampling`` / ``per_request_sampling`` layer over a
fake engine.  Every comparison of outputs is equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from sample_helpers import kernel_case, margin_bound  # noqa: E402
from sample_params_helpers import (LIVE, STREAM_KW, CpuRowSampler, first_rows, grid_point, grid_table,  # noqa: E402
                                   reference_by_row, ticket_block, ticket_params)
from test_generate_pool_cpu import PoolRef  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.generation import (SAMPLE_PARAMS_MUTANTS, SAMPLE_POOL_MUTANTS, SamplePool, SampleState,  # noqa: E402
                                     SamplingParams, sample_books_admit_host, sample_row_params_host, sample_search)

EOS = 1
SEEDS = [41, 42, 43, 44, 0xFFFFFFF5, 46, 47]


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


# ---- C1: SamplingParams -------------------------------------------------------------------------------------------------------
def test_sampling_params_broadcast_ladder_and_bits():
    assert SamplingParams().rows(3).tolist() == [[_bits(1.0), 0, _bits(1.0), 0]] * 3
    rows = SamplingParams(0.7, 5, 0.9).rows(2)
    assert rows.dtype == torch.int32 and rows.shape == (2, 4)
    assert rows.tolist() == [[_bits(0.7), 5, _bits(0.9), 0]] * 2  # word 0 and word 2: fp32 bits; word 3: 0
    assert rows[:, 0].view(torch.float32).tolist() == [float(np.float32(0.7))] * 2
    ladder = SamplingParams(temperature=[0.5, 1.0, 3.0e38], top_k=7, top_p=(1.0, 0.25, 2.0 ** -149))
    assert ladder.rows(3).tolist() == [[_bits(0.5), 7, _bits(1.0), 0], [_bits(1.0), 7, _bits(0.25), 0],
                                       [_bits(3.0e38), 7, 1, 0]]
    assert SamplingParams(top_k=np.array([0, 1, 512])).rows(3)[:, 1].tolist() == [0, 1, 512]
    assert ladder.values(3)[1] == (1.0, 7, 0.25)


@pytest.mark.parametrize("bad", [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
                                 dict(temperature=float("inf")), dict(temperature=1e-50), dict(temperature=3.5e38),
                                 dict(top_k=-1), dict(top_k=1.5), dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=1.01),
                                 dict(top_p=float("nan")), dict(top_p=-0.5), dict(top_p=1e-50)])
def test_sampling_params_refuses_what_check_sampling_refuses_in_any_row(bad):
    with pytest.raises(ValueError):
        SamplingParams(**bad).rows(2)
    (name, value), = bad.items()
    good = dict(temperature=1.0, top_k=0, top_p=1.0)[name]
    for ladder in ([good, value], [value, good]):  # ... in whichever row it stands
        with pytest.raises(ValueError):
            SamplingParams(**{name: ladder}).rows(2)
    assert SamplingParams(**{name: [good, good]}).rows(2).shape == (2, 4)


def test_sampling_params_refuses_a_ladder_of_the_wrong_length():
    for kw in (dict(temperature=[1.0, 2.0]), dict(top_k=[1, 2, 3, 4]), dict(top_p=[]), dict(temperature=[1.0] * 3, top_k=[1] * 2)):
        with pytest.raises(ValueError):
            SamplingParams(**kw).rows(3)
    with pytest.raises(ValueError):
        SamplingParams().rows(0)
    with pytest.raises(ValueError):
        SamplingParams(temperature="1.0").rows(1)


# ---- C2: what the reference leaves out on the mixed-table kernel test's inputs ----------------------------------------------
@pytest.mark.parametrize("rows", [1, 64, 1024])
@pytest.mark.parametrize("V", [1, 3, 384, 512])
def test_the_reference_leaves_out_at_most_a_tenth_of_the_mixed_rows(hip_lib, V, rows):
    lp, seeds, active, row_state, row_sample, u = kernel_case(hip_lib, V, rows)
    nb = min(rows, 64)
    params = [grid_point(int(s), int(b), nb, V) for s, b in zip(row_state, row_sample)]
    if rows >= 64:  # every grid point stands in some row, and neighbouring rows stand at different ones
        assert len({(5 * (int(s) * nb + int(b)) + 1) % 36 for s, b in zip(row_state, row_sample)}) == 36
        assert V < 384 or all(a != b for a, b in zip(params[:63], params[1:64]))
    _, margins = reference_by_row(lp, u, params)
    out = int((margins <= margin_bound(V)).sum())
    print(f"V={V} rows={rows}: {out} rows left out of {rows}")
    assert out <= 0.1 * rows


# ---- C3: the pool with parameters and live rows per ticket ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(hip_lib):
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][EOS] *= 4.0  # some samples stop early: the states end at different lengths
    ref = T5Fp32(cfg, sd)
    srcs = [source_ids(60, 3), source_ids(7, 4), source_ids(33, 5), source_ids(120, 6), source_ids(1, 7), source_ids(20, 8),
            source_ids(64, 9)]
    encs = [ref.encode(s) for s in srcs]
    alone = {}

    def alone_for(nb, ml):
        """Per ticket the search of its source alone at its seed and its block (``nb`` rows: a row's log-probs depend
        on no other row, but the fp32 CPU GEMM's bits may depend on the row count), its first LIVE rows: computed once."""
        if (nb, ml) not in alone:
            outs = []
            for i, (enc, seed) in enumerate(zip(encs, SEEDS)):
                ref.start(enc, nb, ml)
                full = sample_search(lambda tok, anc, t: ref.step(tok.long(), anc[:, : t + 1].long()),
                                     CpuRowSampler(hip_lib).at, nb, ml, seed, params=ticket_block(i, nb))
                outs.append(first_rows(full, LIVE[i % 4]))
            alone[(nb, ml)] = outs
        return alone[(nb, ml)]

    return cfg, sd, encs, alone_for


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits


def _differs(a, b):
    return not (a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences)
                and torch.equal(a.sequences_scores, b.sequences_scores))


def run_pool(hip_lib, cfg, sd, encs, n_slots, nb, ml, k, staggered=False, mutant=None):
    eng = PoolRef(cfg, sd, n_slots, nb, ml)
    sampler = CpuRowSampler(hip_lib, mutant=mutant if mutant == "params_by_row" else None)
    admits = []

    def step(active, pos, tokens, ancestry):
        return eng.step(active, pos, tokens.long(), ancestry[:, : max(pos) + 1].long())

    pool = SamplePool(eng.admit, step, sampler, n_slots, nb, ml, sync_every=k, mutant=mutant, per_request=True,
                      params=SamplingParams(**STREAM_KW))
    admit_host = pool._books_admit
    pool._books_admit = lambda st, states, seeds, start, pad, **kw: (admits.append((list(states), kw)),
                                                                     admit_host(st, states, seeds, start, pad, **kw))[1]
    got, tickets = {}, []
    for i, (enc, seed) in enumerate(zip(encs, SEEDS)):
        tickets.append(pool.submit(enc, seed, params=ticket_params(i), num_samples=LIVE[i % 4]))
        if staggered:
            for _ in range(2):
                got.update(pool.step())
    got.update(pool.drain())
    assert sorted(got) == sorted(tickets) and pool.queued == 0 and pool.in_flight == 0
    return got, tickets, eng, pool, admits


@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("ml", [4, 12])
def test_pool_with_parameters_and_live_rows_per_ticket_equals_the_search_alone(hip_lib, setup, ml, k):
    cfg, sd, encs, alone_for = setup
    n_slots, nb = 3, 4
    want = alone_for(nb, ml)
    got, tickets, eng, pool, admits = run_pool(hip_lib, cfg, sd, encs, n_slots, nb, ml, k)
    for i, (t, w) in enumerate(zip(tickets, want)):
        assert got[t].sequences.shape[0] == LIVE[i % 4] == got[t].sequences_scores.shape[0]  # the ticket's own rows
        _same(got[t], w)
    slots = [s for a in eng.admitted for s in a]
    assert len(slots) == 7 > len(set(slots))  # slots are taken again, under other parameters and live counts
    # every admission carried the tenants' live counts and blocks; the table was written there and nowhere else
    assert [s for a, _ in admits for s in a] == slots
    assert [n for _, kw in admits for n in kw["n_live"]] == [LIVE[i % 4] for i in range(7)]
    blocks = torch.cat([kw["params"] for _, kw in admits])
    assert torch.equal(blocks, torch.stack([ticket_block(i, nb) for i in range(7)]))
    if ml == 12:
        lens = [w.sequences.shape[1] - 1 for w in want]
        assert len(set(lens)) > 1, lens
        # the ladder is one: its rows' parameters differ, and so do its rows' tokens
        assert len({tuple(r.tolist()) for r in want[0].sequences}) > 1


@pytest.mark.parametrize("mutant", SAMPLE_PARAMS_MUTANTS)
def test_the_planted_mutants_are_noticed(hip_lib, setup, mutant):
    cfg, sd, encs, alone_for = setup
    assert SAMPLE_PARAMS_MUTANTS == ("stale_params", "params_by_row", "dead_rows_live")
    assert SAMPLE_POOL_MUTANTS == ("shared_position", "admit_not_reset", "stale_tokens")  # ... and that tuple as it was
    nb, ml = 4, 12
    want = alone_for(nb, ml)
    good, tickets, _, _, _ = run_pool(hip_lib, cfg, sd, encs, 3, nb, ml, 1, staggered=True)
    for t, w in zip(tickets, want):
        _same(good[t], w)
    bad, bad_tickets, _, _, _ = run_pool(hip_lib, cfg, sd, encs, 3, nb, ml, 1, staggered=True, mutant=mutant)
    assert any(_differs(bad[t], w) for t, w in zip(bad_tickets, want)), \
        f"the {mutant} mutant changed no output: the comparison would not notice it"


def test_the_host_restatements_of_the_two_device_routines():
    n, nb, L = 3, 4, 5
    st = SampleState(seeds=torch.full((n,), 7, dtype=torch.int32), seq=torch.full((n, nb, L), 9, dtype=torch.int32),
                     cum_logprob=torch.full((n, nb), -3.0), n_generated=torch.full((n, nb), 4, dtype=torch.int32),
                     finished=torch.full((n, nb), 2, dtype=torch.int32), tokens=torch.full((n * nb,), 5, dtype=torch.int32),
                     params=grid_table(n, nb, 384))
    before = st.params.clone()
    blocks = torch.stack([SamplingParams(0.5, 3, 0.25).rows(nb), SamplingParams([1.0, 2.0, 3.0, 4.0]).rows(nb)])
    sample_books_admit_host(st, [2, 0], [1, 2], 8, 6, n_live=[1, 4], params=blocks)
    assert st.finished.tolist() == [[0, 0, 0, 0], [2, 2, 2, 2], [0, 1, 1, 1]]
    assert torch.equal(st.params[2], blocks[0]) and torch.equal(st.params[0], blocks[1])
    assert torch.equal(st.params[1], before[1]) and (st.seq[1] == 9).all() and (st.tokens == 5).all()
    assert (st.cum_logprob[[0, 2]] == 0).all() and (st.n_generated[[0, 2]] == 0).all()
    # the lookup: launch row a * nb + b takes block (active[a], b)
    got = sample_row_params_host(st, [2, 1])
    assert got[:nb] == [(0.5, 3, 0.25)] * nb
    assert got[nb:] == [(float(np.float32(T)), k, float(np.float32(p))) for T, k, p in (grid_point(1, b, nb, 384) for b in range(nb))]
    assert sample_row_params_host(st, [2, 1], "params_by_row")[:nb] == [(float(T), 0, 1.0) for T in (1.0, 2.0, 3.0, 4.0)]
    # the mutants of the admission
    sample_books_admit_host(st, [1], [3], 8, 6, n_live=[2], params=blocks[:1], mutant="stale_params")
    assert torch.equal(st.params[1], before[1]) and st.finished[1].tolist() == [0, 0, 1, 1]
    sample_books_admit_host(st, [1], [3], 8, 6, n_live=[2], params=blocks[:1], mutant="dead_rows_live")
    assert torch.equal(st.params[1], blocks[0]) and st.finished[1].tolist() == [0, 0, 0, 0]


def test_submit_arguments():
    nothing = lambda *a, **k: None  # noqa: E731
    plain = SamplePool(nothing, nothing, nothing, 2, 4, 8)
    assert plain.state.params is None and not plain.per_request
    for kw in (dict(params=SamplingParams()), dict(num_samples=4), dict(num_samples=1)):
        with pytest.raises(ValueError, match="per_request"):
            plain.submit(object(), 1, **kw)
    pool = SamplePool(nothing, nothing, nothing, 2, 4, 8, per_request=True)
    assert pool.state.params.tolist() == [SamplingParams().rows(4).tolist()] * 2
    for kw in (dict(num_samples=0), dict(num_samples=5), dict(num_samples=1.5), dict(num_samples=-1),
               dict(params=SamplingParams(temperature=0.0)), dict(params=SamplingParams(top_k=[1, 2]), num_samples=3),
               dict(params=SamplingParams(top_p=[0.5] * 4), num_samples=2)):
        with pytest.raises(ValueError):
            pool.submit(object(), 1, **kw)
    assert pool.queued == 0
    assert pool.submit(object(), 1, SamplingParams(top_k=[1, 2]), 2) == 0 and pool.queued == 1


# ---- C4: the default pool is called as before ------------------------------------------------------------------------------------
def test_the_default_pool_calls_its_callbacks_with_the_arguments_it_always_did(hip_lib, setup):
    cfg, sd, encs, _ = setup
    n_slots, nb, ml = 2, 4, 6
    eng = PoolRef(cfg, sd, n_slots, nb, ml)
    seen = {"sample_step": [], "books_admit": [], "rows": []}

    def sample_step(lp, active, pos, state):  # today's signature: anything more is a TypeError
        seen["sample_step"].append((tuple(lp.shape), list(active), list(pos), state))
        state.finished[list(active)] = 1  # every state stops after its first step

    def books_admit(state, states, seeds, start, pad):  # likewise
        seen["books_admit"].append((state, list(states), list(seeds), start, pad))

    def rows(state, active, pos):
        seen["rows"].append((state, list(active), list(pos)))

    pool = SamplePool(eng.admit, lambda a, p, tok, anc: eng.step(a, p, tok.long(), anc[:, : max(p) + 1].long()), sample_step,
                      n_slots, nb, ml, decoder_start_token_id=3, pad_token_id=2, sync_every=1, books_admit=books_admit,
                      rows=rows)
    tickets = [pool.submit(e, s) for e, s in zip(encs[:3], SEEDS)]
    out = pool.drain()
    assert [t for t, _ in out] == tickets and all(o.sequences.shape[0] == nb for _, o in out)
    st = pool.state
    assert st.params is None  # no table: the decoder's sample_pool_step takes the scalar entry point
    assert seen["books_admit"] == [(st, [0, 1], SEEDS[:2], 3, 2), (st, [0], SEEDS[2:3], 3, 2)]
    V = cfg["vocab_size"]
    assert seen["sample_step"] == [((2 * nb, V), [0, 1], [0, 0], st), ((nb, V), [0], [0], st)]
    assert seen["rows"] == [(st, [0, 1], [0, 0]), (st, [0], [0])]


# ---- the tactic generators' layer over a fake engine --------------------------------------------------------------------------------
class _FakeStream:
    def __init__(self, engine, nb, per_request):
        self.engine, self.nb, self.per_request, self.waiting, self.steps = engine, nb, per_request, [], 0

    queued = property(lambda self: len(self.waiting))
    in_flight = 0

    def submit(self, ids, seed, params=None, num_samples=None):
        assert self.per_request and 1 <= num_samples <= self.nb
        self.engine.submitted.append((len(self.engine.streams) - 1, seed, params, num_samples))
        self.waiting.append((len(self.engine.submitted), seed, num_samples))
        return len(self.engine.submitted)

    def step(self):
        self.steps += 1
        done, self.waiting = self.waiting[:1], self.waiting[1:]  # one ticket per step: later calls find the stream busy
        return [(t, _fake_out(seed, k)) for t, seed, k in done]


def _fake_out(seed, k):
    from reprover_amd.generation import BeamSearchOutput
    rows = [[0, 3 + ord("a") + (seed + r) % 26, 1] for r in range(k)]
    return BeamSearchOutput(torch.tensor(rows, dtype=torch.int64), torch.tensor([-0.5 * r for r in range(k)]))


class _FakeEngine:
    def __init__(self):
        from types import SimpleNamespace
        self.decoder = SimpleNamespace(max_states=lambda nb: 2)
        self.streams, self.opened, self.submitted, self.many = [], [], [], []

    def sample_many(self, sources, nb, max_len, temperature, top_k, top_p, seeds, lp, **kw):
        self.many.append((len(sources), nb, kw))
        return [_fake_out(seed, nb) for seed in seeds]

    def sample_stream(self, nb, max_len, temperature, top_k, top_p, lp, n_slots=None, src_cap=None, sync_every=16,
                      per_request=False):
        assert all(s.queued == 0 for s in self.streams)  # opened only once the last one has drained
        self.opened.append((nb, per_request))
        self.streams.append(_FakeStream(self, nb, per_request))
        return self.streams[-1]


def _fake_generator(**kw):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator
    from reprover_amd.tokenizer import ByT5Tokenizer
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, do_sample=True, temperature=0.8, top_k=40, top_p=0.9, seed=5, **kw)
    gen.generator, gen.tokenizer = _FakeEngine(), ByT5Tokenizer()
    return gen


def test_tactic_generator_joins_the_running_stream_with_its_own_rows_and_parameters():
    import asyncio
    from reprover_amd.common import Pos
    args = ("f.lean", "thm", Pos(1, 0))
    hot, ladder = SamplingParams(1.5, 0, 0.9), SamplingParams([0.7, 1.3], 5, 1.0)
    calls = [("s0", 4, hot), ("s1", 2, ladder), ("s2", 4, None), ("s3", 1, None), ("s4", 8, hot)]
    gen = _fake_generator(sample_stream=True, per_request_sampling=True)

    async def main():
        return await asyncio.gather(*(gen.generate(s, *args, n, sampling=q) for s, n, q in calls))

    got = asyncio.run(main())
    eng = gen.generator
    assert eng.opened == [(4, True), (8, True)]  # the first call's rows; only the call asking for more re-opened
    assert [(s, q, k) for s, _, q, k in eng.submitted] == [(0, hot, 4), (0, ladder, 2), (0, None, 4), (0, None, 1), (1, hot, 8)]
    fresh = _fake_generator()
    want = [fresh.generate_sync(s, *args, n, sampling=q) for s, n, q in calls]  # the seeds follow call order
    assert got == want and [len(g) for g in got] == [4, 2, 4, 1, 8]
    assert [kw for _, _, kw in fresh.generator.many] == [{"params": [hot]}, {"params": [ladder]}, {}, {}, {"params": [hot]}]
    assert gen._driver is None and not gen._waiters
    # batch_generate_sync: a sequence with one entry per state, chunked with the states; all None is the call as it was
    fresh.generator.many.clear()
    fresh.batch_generate_sync(["a", "b", "c"], [args[0]] * 3, [args[1]] * 3, [args[2]] * 3, 4, sampling=[hot, None, ladder.__class__(1.0)])
    assert [(n, set(kw)) for n, _, kw in fresh.generator.many] == [(2, {"params"}), (1, {"params"})]
    assert fresh.generator.many[0][2]["params"] == [hot, None]
    fresh.generator.many.clear()
    fresh.batch_generate_sync(["a"], [args[0]], [args[1]], [args[2]], 4, sampling=[None])
    assert fresh.generator.many == [(1, 4, {})]
    # sample_stream_samples: the stream's rows whatever the first call asks for
    wide = _fake_generator(sample_stream=True, per_request_sampling=True, sample_stream_samples=8)
    asyncio.run(wide.generate("s", *args, 2))
    assert wide.generator.opened == [(8, True)] and wide.generator.submitted[0][3] == 2


def test_tactic_generator_refusals():
    import asyncio
    from reprover_amd.common import Pos
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator
    args = ("f.lean", "thm", Pos(1, 0))
    base = ("unused", "cpu", 64, 16, 0.0)
    beam = HuggingFaceGenerator(*base)
    with pytest.raises(ValueError, match="do_sample"):
        beam.generate_sync("s", *args, 4, sampling=SamplingParams())
    with pytest.raises(ValueError, match="do_sample"):
        asyncio.run(beam.generate("s", *args, 4, sampling=SamplingParams()))
    with pytest.raises(ValueError, match="do_sample"):
        beam.batch_generate_sync(["s"], [args[0]], [args[1]], [args[2]], 4, sampling=[SamplingParams()])
    with pytest.raises(ValueError, match="sample_stream"):
        HuggingFaceGenerator(*base, do_sample=True, per_request_sampling=True)
    with pytest.raises(ValueError, match="sample_stream_samples"):
        HuggingFaceGenerator(*base, do_sample=True, sample_stream=True, sample_stream_samples=4)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sample_stream_samples"):
            HuggingFaceGenerator(*base, do_sample=True, sample_stream=True, per_request_sampling=True, sample_stream_samples=bad)
    plain = _fake_generator(sample_stream=True)
    with pytest.raises(ValueError, match="per_request_sampling"):
        asyncio.run(plain.generate("s", *args, 4, sampling=SamplingParams()))
    gen = _fake_generator(sample_stream=True, per_request_sampling=True)
    served = gen.states_served
    for q in (SamplingParams(top_k=[1, 2, 3]), SamplingParams(temperature=0.0)):  # refused before a seed is taken
        with pytest.raises(ValueError):
            asyncio.run(gen.generate("s", *args, 4, sampling=q))
    assert gen.states_served == served and gen.generator.opened == []
    with pytest.raises(ValueError):
        gen.batch_generate_sync(["a", "b"], [args[0]] * 2, [args[1]] * 2, [args[2]] * 2, 4, sampling=[None])
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, do_sample=True, sample_stream=True,
                                      per_request_sampling=True, sample_stream_samples=6)
    assert rag.hf_gen.per_request_sampling and rag.hf_gen.sample_stream_samples == 6
