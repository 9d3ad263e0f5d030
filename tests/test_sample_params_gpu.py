"""Sampling parameters per request on the MI355X (rp_sample_step_rows / rp_sample_pool_step_rows /
rp_sample_pool_admit_rows, ``sample_many(params=...)``, ``sample_stream(per_request=True)``, the tactic generators'
``sampling``): a uniform table against the scalar entry point, a mixed table row by row against scalar calls and the
float64 reference, the neighbours of a step and of an admission between guards, the admission with live rows, the
property the live-row contract rests on, whole searches and streams against ``sample`` alone, and the refusals.  Every
comparison of books and outputs is equality of bits."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from hip_helpers import guard_intact, guarded  # noqa: E402
from sample_helpers import GRID, KERNEL_T, kernel_case, margin_bound  # noqa: E402
from sample_params_helpers import (LIVE, STREAM_KW, first_rows, grid_point, grid_table, reference_by_row,  # noqa: E402
                                   ticket_params, uniform_table)
from test_generate_batch_gpu import _save_generator_dir  # noqa: E402
from test_sample_gpu import _gen  # noqa: E402
from test_sample_pool_gpu import _arena_state, _arenas, _case, _host_state, _same_books, _to_dev  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Decoder  # noqa: E402
from reprover_amd.generation import SamplePool, SampleState, SamplingParams  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, PAD = 1, 0
C = _lib.C
FIELDS = ("seeds", "seq", "cum_logprob", "n_generated", "finished", "tokens")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _kernel_states(lib, V, rows):
    """``test_kernel_equals_the_reference_sampler``'s inputs and books: (lp on the device, a maker of fresh books,
    kernel_case's lists)."""
    lp, seeds, active, row_state, row_sample, u = kernel_case(lib, V, rows)
    nb = min(rows, 64)
    n = rows // nb
    start = np.linspace(-3, 3, n * nb, dtype=np.float32).reshape(n, nb)
    was_finished = (np.arange(n * nb).reshape(n, nb) % 5) == 2

    def fresh(params=None):
        st = _to_dev(_host_state(n, nb, 9, seeds, start, was_finished))
        st.params = None if params is None else params.to(DEV).contiguous()
        return st

    return torch.from_numpy(lp).to(DEV), fresh, (lp, n, nb, active, row_state, row_sample, u, was_finished)


def _host(st):
    return {f: (getattr(st, f).cpu().view(torch.int32) if f == "cum_logprob" else getattr(st, f).cpu()).numpy() for f in FIELDS}


# ---- G1: a uniform table is the scalar entry point ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 64, 1024])
@pytest.mark.parametrize("V", [1, 3, 384, 512])
def test_a_uniform_table_equals_the_scalar_entry_point(V, rows):
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    lp_d, fresh, (_, n, nb, active, *_rest) = _kernel_states(lib, V, rows)
    for T, k, p in GRID:
        k = V if k == "vocab" else k
        one, two = fresh(), fresh(uniform_table(n, nb, T, k, p))
        dec.sample_step(lp_d, active, KERNEL_T, one, T, k, p, EOS, PAD)
        dec.sample_step(lp_d, active, KERNEL_T, two, 1.0, 0, 1.0, EOS, PAD)  # (the table's values, not these)
        _same_books(one, two)
        assert int(one.n_generated.sum()) > 0 or rows == 1


# ---- G2: a mixed table, row by row -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 64, 1024])
@pytest.mark.parametrize("V", [1, 3, 384, 512])
def test_a_mixed_table_equals_the_scalar_call_of_every_row_and_the_reference(V, rows):
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    lp_d, fresh, (lp, n, nb, active, row_state, row_sample, u, was_finished) = _kernel_states(lib, V, rows)
    t = KERNEL_T
    mixed = fresh(grid_table(n, nb, V))
    dec.sample_step(lp_d, active, t, mixed, 1.0, 0, 1.0, EOS, PAD)
    got = _host(mixed)
    params = [grid_point(int(s), int(b), nb, V) for s, b in zip(row_state, row_sample)]
    launch_row = np.arange(rows)
    for point in sorted(set(params)):
        scalar = fresh()
        dec.sample_step(lp_d, active, t, scalar, *point, EOS, PAD)
        want = _host(scalar)
        mine = np.array([q == point for q in params])
        s, b = row_state[mine], row_sample[mine]
        for f in ("seq", "cum_logprob", "n_generated", "finished"):
            assert np.array_equal(got[f][s, b], want[f][s, b]), (point, f)
        assert np.array_equal(got["tokens"][launch_row[mine]], want["tokens"][launch_row[mine]]), point
    assert np.array_equal(got["seeds"], _host(fresh())["seeds"])
    # ... and the float64 reference at every row's own grid point
    tokens = got["seq"][row_state, row_sample, t + 1]
    want_tok, margins = reference_by_row(lp, u, params)
    ok = margins > margin_bound(V)
    left_out = int((~ok).sum())
    print(f"V={V} rows={rows}: {left_out} rows left out")
    assert left_out <= 0.1 * rows
    cmp = ok & ~was_finished[row_state, row_sample]
    assert np.array_equal(tokens[cmp], want_tok[cmp]), np.nonzero(cmp & (tokens != want_tok))[0][:8]
    assert (tokens[was_finished[row_state, row_sample]] == PAD).all()


def test_a_mixed_table_at_mixed_positions_equals_single_slot_scalar_calls():
    """Four states of three samples, each slot at its own position, the active list permuted: every row holds what the
    scalar ``rp_sample_step`` of its slot alone, at the slot's position and the row's grid point, leaves in that row."""
    lib = _lib.load()
    V, n, nb, max_len = 384, 4, 3, 9
    lp, seeds, _, cum, finished = _case(lib, V, n, nb)
    P = {0: 0, 1: 5, 2: max_len - 2, 3: 2}
    active = [2, 0, 3, 1]
    pos = [P[s] for s in active]
    table = grid_table(n, nb, V).to(DEV)
    one = _to_dev(_host_state(n, nb, max_len, seeds, cum, finished))
    _lib.check(lib.rp_sample_pool_step_rows(lp.data_ptr(), V, _p(_i32(*active)), _p(_i32(*pos)), n, n, nb,
                                            one.seeds.data_ptr(), max_len, table.data_ptr(), EOS, PAD, one.seq.data_ptr(),
                                            one.tokens.data_ptr(), one.cum_logprob.data_ptr(), one.n_generated.data_ptr(),
                                            one.finished.data_ptr(), None), "rp_sample_pool_step_rows")
    got = _host(one)
    for a, s in enumerate(active):
        for b in range(nb):
            two = _to_dev(_host_state(n, nb, max_len, seeds, cum, finished))
            T, k, p = grid_point(s, b, nb, V)
            _lib.check(lib.rp_sample_step(lp.data_ptr() + a * nb * V * 4, V, _p(_i32(s)), 1, n, nb, two.seeds.data_ptr(),
                                          P[s], max_len, T, k, p, EOS, PAD, two.seq.data_ptr(),
                                          two.tokens.data_ptr() + a * nb * 4, two.cum_logprob.data_ptr(),
                                          two.n_generated.data_ptr(), two.finished.data_ptr(), None), "rp_sample_step")
            want = _host(two)
            for f in ("seq", "cum_logprob", "n_generated", "finished"):
                assert np.array_equal(got[f][s, b], want[f][s, b]), (s, b, f)
            assert got["tokens"][a * nb + b] == want["tokens"][a * nb + b]
    seq = got["seq"]
    for s in range(n):  # column pos + 1 of every state, and no other
        assert (np.delete(seq[s], P[s] + 1, axis=1) == -7).all() and (seq[s, :, P[s] + 1] != -7).all()
    assert torch.equal(table.cpu(), grid_table(n, nb, V))


# ---- G3: the neighbours of a step and of an admission -------------------------------------------------------------------------------
POISON = 0x5A5A5A5A
NAN_BITS = 0x7FC00000  # a poisoned parameter block: NaN temperature and top_p, a top_k of NaN's bits


def test_a_step_and_an_admission_leave_their_neighbours_and_the_guards_alone():
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    V, n, nb, max_len = 384, 4, 3, 9
    lp, seeds, _, cum, finished = _case(lib, V, n, nb)
    sizes = dict(seeds=n, seq=n * nb * max_len, cum_logprob=n * nb, n_generated=n * nb, finished=n * nb, tokens=n * nb,
                 params=n * nb * 4)
    shapes = dict(seeds=(n,), seq=(n, nb, max_len), cum_logprob=(n, nb), n_generated=(n, nb), finished=(n, nb),
                  tokens=(n * nb,), params=(n, nb, 4))
    bufs = {f: guarded(w, POISON, POISON, device=DEV, dtype=torch.int32) for f, w in sizes.items()}
    view = {f: bufs[f][1].view(*shapes[f]) for f in sizes}
    good = _host_state(n, nb, max_len, seeds, cum, finished)
    listed, others = [2, 0], [1, 3]
    for s in listed:  # the listed states hold real books and real blocks; the others stay poisoned, blocks included
        for f in ("seeds", "seq", "n_generated", "finished"):
            view[f][s] = getattr(good, f)[s].to(DEV)
        view["cum_logprob"][s] = good.cum_logprob[s].view(torch.int32).to(DEV)
        view["params"][s] = grid_table(n, nb, V)[s].to(DEV)
    for s in others:
        view["params"][s] = NAN_BITS
    assert view["params"].data_ptr() % 16 == 0
    st = SampleState(seeds=view["seeds"], seq=view["seq"], cum_logprob=view["cum_logprob"].view(torch.float32),
                     n_generated=view["n_generated"], finished=view["finished"], tokens=view["tokens"],
                     params=view["params"])

    def snapshot():
        torch.cuda.synchronize()
        return {f: view[f].cpu().clone() for f in sizes}

    def guards_intact():
        return all(guard_intact(bufs[f][0], sizes[f], POISON) for f in sizes)

    before = snapshot()
    dec.sample_pool_step(lp[: 2 * nb].contiguous(), listed, [0, 5], st, 1.0, 0, 1.0, EOS, PAD)
    after = snapshot()
    assert guards_intact()
    for f in ("seeds", "seq", "cum_logprob", "n_generated", "finished"):
        assert torch.equal(after[f][others], before[f][others]), f
    assert torch.equal(after["params"], before["params"])  # the step writes no block, the listed states' included
    assert torch.equal(after["tokens"][2 * nb :], before["tokens"][2 * nb :])
    assert not torch.equal(after["seq"][listed], before["seq"][listed])  # ... and it did run
    assert (after["seq"][2, :, 1] != -7).all() and (after["seq"][0, :, 6] != -7).all()
    # the admission at the ABI: state 2 with two live rows
    _lib.check(lib.rp_sample_pool_admit_rows(_p(_i32(2)), _p(np.array([77], dtype=np.uint32)), _p(_i32(2)), 1, n, nb, max_len,
                                             5, PAD, st.seeds.data_ptr(), st.seq.data_ptr(), st.cum_logprob.data_ptr(),
                                             st.n_generated.data_ptr(), st.finished.data_ptr(), None),
               "rp_sample_pool_admit_rows")
    admitted = snapshot()
    assert guards_intact()
    for f in ("seeds", "seq", "cum_logprob", "n_generated", "finished"):
        assert torch.equal(admitted[f][[0, 1, 3]], after[f][[0, 1, 3]]), f
    assert torch.equal(admitted["params"], after["params"]) and torch.equal(admitted["tokens"], after["tokens"])
    assert admitted["finished"][2].tolist() == [0, 0, 1] and admitted["seeds"][2].item() == 77
    assert admitted["seq"][2].tolist() == [[5] + [PAD] * (max_len - 1)] * nb
    # the Python layer's admission: the tenant's block, and no other block
    block = SamplingParams([0.5, 2.0, 1.0], 3, 0.25).rows(nb)[None]
    dec.sample_books_admit(st, [0], [78], 5, PAD, n_live=[1], params=block)
    last = snapshot()
    assert guards_intact()
    assert torch.equal(last["params"][0], block[0]) and torch.equal(last["params"][1:], admitted["params"][1:])
    for f in ("seeds", "seq", "cum_logprob", "n_generated", "finished"):
        assert torch.equal(last[f][[1, 2, 3]], admitted[f][[1, 2, 3]]), f
    assert last["finished"][0].tolist() == [0, 1, 1] and torch.equal(last["tokens"], admitted["tokens"])


# ---- G4: the admission with live rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 64])
@pytest.mark.parametrize("max_len", [2, 9])
def test_admission_with_live_rows(max_len, nb):
    lib = _lib.load()
    n, start, pad, fill = 4, 5, 9, 0x7F
    states, seeds = [3, 1], [0xDEADBEEF, 7]
    word = int(np.frombuffer(bytes([fill] * 4), dtype=np.int32)[0])
    plain = _arenas(n, nb, max_len, fill)
    _lib.check(lib.rp_sample_pool_admit(_p(_i32(*states)), _p(np.array(seeds, dtype=np.uint32)), 2, n, nb, max_len, start,
                                        pad, plain["seeds"].ptr, plain["seq"].ptr, plain["cum_logprob"].ptr,
                                        plain["n_generated"].ptr, plain["finished"].ptr, None), "rp_sample_pool_admit")
    torch.cuda.synchronize()
    want = _arena_state(plain, n, nb, max_len)
    for live in sorted({1, nb, (nb + 1) // 2}):
        for counts in ([live, nb], [nb, live], [live, live]):
            ar = _arenas(n, nb, max_len, fill)
            _lib.check(lib.rp_sample_pool_admit_rows(_p(_i32(*states)), _p(np.array(seeds, dtype=np.uint32)),
                                                     _p(_i32(*counts)), 2, n, nb, max_len, start, pad, ar["seeds"].ptr,
                                                     ar["seq"].ptr, ar["cum_logprob"].ptr, ar["n_generated"].ptr,
                                                     ar["finished"].ptr, None), "rp_sample_pool_admit_rows")
            torch.cuda.synchronize()
            got = _arena_state(ar, n, nb, max_len)
            assert not any(a.broken_guards() for a in ar.values())
            for s, k in zip(states, counts):
                assert got.finished[s].tolist() == [0] * k + [1] * (nb - k), (counts, s)
            for s in (0, 2):  # the other states: untouched
                assert (got.finished[s] == word).all() and (got.seq[s] == word).all() and got.seeds[s].item() == word
            got.finished[states] = 0
            _same_books(got, want)  # everything else - and, at n_live = nb, everything - is rp_sample_pool_admit's
            if counts == [nb, nb]:
                _same_books(_arena_state(ar, n, nb, max_len), want)


# ---- end to end: the tiny generator ---------------------------------------------------------------------------------------------------
LENGTHS = (60, 7, 33, 300, 1, 120, 64)
SEEDS = (21, 22, 23, 0xFFFFFFF0, 25, 26, 27)


@pytest.fixture(scope="module")
def tiny_gen():
    return _gen("tiny", eos_boost=4.0)  # EOS boosted: samples and states end at different lengths


def _same(a, b):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)  # bits


# G5
def test_the_first_rows_of_a_wider_search_are_the_narrower_search(tiny_gen):
    """What the live-row contract rests on: rows 0..1 of ``sample(ids, 4)`` are ``sample(ids, 2)``, bit for bit."""
    cfg, gen = tiny_gen
    for n, seed in zip(LENGTHS[:3], SEEDS):
        src = source_ids(n, 30)
        four = gen.sample(src, 4, 12, seed=seed, **STREAM_KW)
        _same(first_rows(four, 2), gen.sample(src, 2, 12, seed=seed, **STREAM_KW))
        _same(first_rows(four, 1), gen.sample(src, 1, 12, seed=seed, **STREAM_KW))


# G6
def test_sample_many_with_parameters_per_source(tiny_gen):
    cfg, gen = tiny_gen
    nb, ml = 4, 12
    srcs = [source_ids(n, 30 + i) for i, n in enumerate(LENGTHS[:3])]
    seeds = list(SEEDS[:3])
    ladder = ticket_params(0)
    params = [ladder, None, SamplingParams(0.8, 1, 1.0)]
    alone = [gen.sample(s, nb, ml, seed=sd, params=q, **STREAM_KW) for s, sd, q in zip(srcs, seeds, params)]
    _same(alone[1], gen.sample(srcs[1], nb, ml, seed=seeds[1], **STREAM_KW))  # None: the call's scalars
    _same(alone[2], gen.sample(srcs[2], nb, ml, 0.8, 1, 1.0, seed=seeds[2]))  # scalars as a table: the scalar call
    for order in ([0, 1, 2], [2, 1, 0]):
        outs = gen.sample_many([srcs[i] for i in order], nb, ml, seeds=[seeds[i] for i in order],
                               params=[params[i] for i in order], **STREAM_KW)
        for o, i in zip(outs, order):
            _same(o, alone[i])
    # every row of the ladder is that row of the uniform call at the row's own values
    width = alone[0].sequences.shape[1]
    for b, (T, k, p) in enumerate(ladder.values(nb)):
        uni = gen.sample(srcs[0], nb, ml, T, k, p, seed=seeds[0])
        row = torch.full((ml,), PAD, dtype=torch.int64)
        row[: uni.sequences.shape[1]] = uni.sequences[b]
        mine = torch.full((ml,), PAD, dtype=torch.int64)
        mine[:width] = alone[0].sequences[b]
        assert torch.equal(mine, row), b
        assert torch.equal(alone[0].sequences_scores[b], uni.sequences_scores[b]), b
    assert len({tuple(r.tolist()) for r in alone[0].sequences}) > 1
    with pytest.raises(ValueError):
        gen.sample_many(srcs, nb, ml, params=params[:2])
    with pytest.raises(ValueError):
        gen.sample(srcs[0], nb, ml, params=SamplingParams(top_k=[1, 2]))  # a ladder of the wrong length


# G7
@pytest.mark.parametrize("sync_every", [1, 16])
@pytest.mark.parametrize("ml", [4, 12])
def test_stream_with_parameters_and_live_rows_per_ticket_equals_sample_alone(tiny_gen, ml, sync_every):
    cfg, gen = tiny_gen
    nb, n_slots = 4, 3
    srcs = [source_ids(n, 30 + i) for i, n in enumerate(LENGTHS)]
    want = [gen.sample(s, LIVE[i % 4], ml, seed=seed, params=ticket_params(i), **STREAM_KW)
            for i, (s, seed) in enumerate(zip(srcs, SEEDS))]
    stream = gen.sample_stream(nb, ml, n_slots=n_slots, src_cap=512, sync_every=sync_every, per_request=True, **STREAM_KW)
    assert isinstance(stream.pool, SamplePool) and stream.pool.per_request and stream.pool.state.params.is_cuda
    admitted = []
    pool_admit = gen.decoder.pool_admit
    gen.decoder.pool_admit = lambda slots, *a, **k: (admitted.extend(int(s) for s in slots), pool_admit(slots, *a, **k))[1]
    try:
        tickets = [stream.submit(s, seed, params=ticket_params(i), num_samples=LIVE[i % 4])
                   for i, (s, seed) in enumerate(zip(srcs, SEEDS))]
        got = dict(stream.drain())
    finally:
        del gen.decoder.pool_admit
    assert sorted(got) == sorted(tickets)
    for i, (t, w) in enumerate(zip(tickets, want)):
        assert got[t].sequences.shape[0] == LIVE[i % 4]
        _same(got[t], w)
    assert len(admitted) == 7 > len(set(admitted))  # slots served again, under other parameters and live counts
    if ml == 12:
        assert len({w.sequences.shape[1] for w in want}) > 1


# G8
def test_gathered_generate_with_sampling_per_call_equals_generate_sync_in_order(tmp_path):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= 4.0
    gdir = str(tmp_path / "gen")
    _save_generator_dir(gdir, cfg, sd)
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900)]
    counts = (4, 2, 4, 1)
    sampling = (ticket_params(0), SamplingParams([0.9, 1.4], 0, 0.9), None, SamplingParams(0.8, 1, 1.0))
    kw = dict(do_sample=True, temperature=1.2, top_k=50, top_p=0.95, seed=11)
    hf = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, sample_stream=True, sample_stream_slots=4, sample_sync_every=4,
                              per_request_sampling=True, **kw)
    hf.initialize()
    fresh = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, **kw)
    fresh.initialize()
    args = ("f.lean", "thm", Pos(1, 0))
    opened = []
    open_stream = hf.generator.sample_stream
    hf.generator.sample_stream = lambda *a, **k: (opened.append((a, k)), open_stream(*a, **k))[1]

    async def main():
        return await asyncio.gather(*(hf.generate(s, *args, n, sampling=q) for s, n, q in zip(states, counts, sampling)))

    got = asyncio.run(main())
    assert got == [fresh.generate_sync(s, *args, n, sampling=q) for s, n, q in zip(states, counts, sampling)]
    assert all(got) and [len(g) <= n for g, n in zip(got, counts)] == [True] * 4
    # one stream, opened per request with the first call's rows; every call joined it while it ran: four states in 31
    # steps at the most, where a drain between two calls would have cost a second stream
    assert len(opened) == 1 and opened[0][0][0] == 4 and opened[0][1]["per_request"] is True
    assert hf._stream.pool.per_request and hf._stream.pool.nb == 4 and 1 <= hf._stream.steps <= 31
    assert hf._driver is None and not hf._waiters and hf._stream.in_flight == 0 and hf._stream.queued == 0
    with pytest.raises(ValueError, match="do_sample"):
        HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0).generate_sync(states[0], *args, 4, sampling=SamplingParams())
    plain = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, sample_stream=True, **kw)
    with pytest.raises(ValueError, match="per_request_sampling"):
        asyncio.run(plain.generate(states[0], *args, 4, sampling=SamplingParams()))


# ---- G9: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_poisoned_outputs_untouched(tiny_gen):
    lib = _lib.load()
    buf = torch.full((1 << 16,), 123, dtype=torch.int32, device=DEV)
    d, *parts = (buf.data_ptr() + i * 0x8000 for i in range(8))  # the log-probs, the six arrays, the table: 32 KiB apart
    d_seeds, d_seq, d_tok, d_cum, d_ngen, d_fin, d_par = parts
    ids = np.arange(32, dtype=np.int32)
    zeros = np.zeros(32, dtype=np.int32)
    fours = np.full(32, 4, dtype=np.int32)
    useeds = np.arange(32, dtype=np.uint32)

    def step(V=384, na=2, n=2, nb=4, t=0, ml=8, par=d_par, lp=d, a=ids, seeds=d_seeds, seq=d_seq, tok=d_tok, cum=d_cum,
             ngen=d_ngen, fin=d_fin):
        return lib.rp_sample_step_rows(lp, V, _p(a), na, n, nb, seeds, t, ml, par, EOS, PAD, seq, tok, cum, ngen, fin, None)

    def pool_step(V=384, na=2, n=2, nb=4, ml=8, par=d_par, lp=d, a=ids, pos=zeros, seeds=d_seeds, seq=d_seq, tok=d_tok,
                  cum=d_cum, ngen=d_ngen, fin=d_fin):
        return lib.rp_sample_pool_step_rows(lp, V, _p(a), _p(pos), na, n, nb, seeds, ml, par, EOS, PAD, seq, tok, cum, ngen,
                                            fin, None)

    def admit(s=ids, new=useeds, live=fours, m=2, n=2, nb=4, ml=8, seeds=d_seeds, seq=d_seq, cum=d_cum, ngen=d_ngen,
              fin=d_fin):
        return lib.rp_sample_pool_admit_rows(_p(s), _p(new), _p(live), m, n, nb, ml, 5, PAD, seeds, seq, cum, ngen, fin, None)

    def refused(fn, word, **kw):
        assert fn(**kw) == -1, (fn.__name__, kw)
        msg = lib.rp_last_error()
        assert msg and word in msg, (fn.__name__, kw, msg)

    shared = ((dict(V=513), b"vocab"), (dict(V=0), b"vocab"), (dict(nb=65), b"nb=65"), (dict(nb=0), b"nb=0"),
              (dict(na=17, n=17, nb=64), b"rows"), (dict(n=33, na=33), b"states=33"), (dict(n=0, na=0), b"states=0"),
              (dict(na=3), b"active states=3"), (dict(na=0), b"active states=0"), (dict(ml=1), b"max_len=1"),
              (dict(lp=None), b"null"), (dict(a=None), b"null"), (dict(seeds=None), b"null"), (dict(seq=None), b"null"),
              (dict(tok=None), b"null"), (dict(cum=None), b"null"), (dict(ngen=None), b"null"), (dict(fin=None), b"null"),
              (dict(a=_i32(1, 1)), b"twice"), (dict(a=_i32(0, 2)), b"active[1]=2"), (dict(a=_i32(-1, 0)), b"active[0]=-1"),
              # ... and the table itself
              (dict(par=None), b"params"), (dict(par=d_par + 4), b"aligned"), (dict(par=d_par + 8), b"aligned"))
    for kw, word in shared + ((dict(t=7), b"t=7"), (dict(t=-1), b"t=-1")):
        refused(step, word, **kw)
    for kw, word in shared + ((dict(pos=None), b"null"), (dict(pos=_i32(0, 7)), b"pos[1]=7"), (dict(pos=_i32(-1, 0)), b"pos[0]=-1")):
        refused(pool_step, word, **kw)
    for kw, word in ((dict(s=None), b"null"), (dict(new=None), b"null"), (dict(live=None), b"null"), (dict(seeds=None), b"null"),
                     (dict(seq=None), b"null"), (dict(cum=None), b"null"), (dict(ngen=None), b"null"), (dict(fin=None), b"null"),
                     (dict(m=0), b"admitted states=0"), (dict(m=3), b"admitted states=3"), (dict(s=_i32(1, 1)), b"twice"),
                     (dict(s=_i32(0, 2)), b"states[1]=2"), (dict(s=_i32(-1, 0)), b"states[0]=-1"), (dict(nb=0), b"nb=0"),
                     (dict(nb=65), b"nb=65"), (dict(n=0), b"states=0"), (dict(n=33), b"states=33"),
                     (dict(m=17, n=17, nb=64), b"rows"), (dict(ml=1), b"max_len=1"),
                     (dict(live=_i32(0, 4)), b"n_live[0]=0"), (dict(live=_i32(4, 5)), b"n_live[1]=5"),
                     (dict(live=_i32(-1, 4)), b"n_live[0]=-1")):
        refused(admit, word, **kw)
    torch.cuda.synchronize()
    assert bool((buf == 123).all())  # nothing was launched
    # the accepted calls do write (the table: valid blocks first; the refusals above never read it)
    buf[0x8000 * 7 // 4 : 0x8000 * 7 // 4 + 2 * 4 * 4] = uniform_table(2, 4, 1.0, 0, 1.0).reshape(-1).to(DEV)
    for fn, kw in ((step, dict(t=6)), (pool_step, dict(pos=_i32(0, 6))), (admit, dict(live=_i32(1, 4)))):
        before = buf.clone()
        assert fn(**kw) == 0, fn.__name__
        torch.cuda.synchronize()
        assert not torch.equal(buf, before), fn.__name__
    # the Python layer
    cfg, gen = tiny_gen
    src = source_ids(7, 4)
    plain = gen.sample_stream(4, 8, src_cap=16)
    for kw in (dict(params=SamplingParams()), dict(num_samples=2), dict(num_samples=4)):
        with pytest.raises(ValueError, match="per_request"):
            plain.submit(src, 1, **kw)
    stream = gen.sample_stream(4, 8, src_cap=16, per_request=True)
    for kw in (dict(num_samples=5), dict(num_samples=0), dict(params=SamplingParams(top_p=0.0)),
               dict(params=SamplingParams(temperature=[1.0] * 4), num_samples=3)):
        with pytest.raises(ValueError):
            stream.submit(src, 1, **kw)
    assert stream.queued == 0 and stream.step() == []


# ---- G10: ByT5-small dimensions -----------------------------------------------------------------------------------------------------
def test_byt5_small_dimensions():
    """Sources of 300, 2048 and 1 bytes through 2 slots, 8 rows, max_length 32, with 8, 3 and 1 live rows."""
    cfg, gen = _gen("byt5-small")
    srcs = [source_ids(300, 8), source_ids(2048, 9), source_ids(1, 10)]
    kw = dict(temperature=0.9, top_k=0, top_p=0.9)
    live = (8, 3, 1)
    params = (SamplingParams(temperature=[0.6 + 0.2 * b for b in range(8)], top_k=[0, 5] * 4, top_p=0.95),
              SamplingParams(1.3, 40, [1.0, 0.9, 0.5]), None)
    alone = [gen.sample(s, k, 32, seed=70 + i, params=q, **kw) for i, (s, k, q) in enumerate(zip(srcs, live, params))]
    stream = gen.sample_stream(8, 32, n_slots=2, per_request=True, **kw)
    tickets = [stream.submit(s, 70 + i, params=q, num_samples=k) for i, (s, k, q) in enumerate(zip(srcs, live, params))]
    got = dict(stream.drain())
    for t, a in zip(tickets, alone):
        _same(got[t], a)
