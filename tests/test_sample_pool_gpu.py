"""Continuous batching for sampling on the MI355X (rp_sample_pool_step / rp_sample_pool_admit / rp_sample_pool_rows,
``sample_stream``, ``HuggingFaceGenerator(sample_stream=True)``): the uniform call against ``rp_sample_step``, mixed
positions against single-state calls, the admission and the row rebuild against their host restatements between guards,
the refusals, whole streams against ``sample`` alone, the stream's device-to-host copies counted, the retirement rule.
Every comparison is equality."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from hip_helpers import Arena  # noqa: E402
from sample_helpers import KERNEL_T, kernel_case  # noqa: E402
from test_generate_batch_gpu import _save_generator_dir  # noqa: E402
from test_sample_gpu import _gen  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, SampleStream  # noqa: E402
from reprover_amd.generation import SamplePool, SampleState, sample_books_admit_host, sample_books_rows_host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, PAD = 1, 0
GUARD = 1 << 20
C = _lib.C
FIELDS = ("seeds", "seq", "cum_logprob", "n_generated", "finished", "tokens")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _host_state(n, nb, max_len, seeds, cum, finished, fill=-7):
    bits = np.asarray(seeds, dtype=np.uint32).view(np.int32)
    return SampleState(seeds=torch.from_numpy(bits.copy()), seq=torch.full((n, nb, max_len), fill, dtype=torch.int32),
                       cum_logprob=torch.from_numpy(np.asarray(cum, dtype=np.float32).reshape(n, nb).copy()),
                       n_generated=torch.zeros((n, nb), dtype=torch.int32),
                       finished=torch.from_numpy(np.asarray(finished, dtype=np.int32).reshape(n, nb).copy()),
                       tokens=torch.full((n * nb,), fill, dtype=torch.int32))


def _to_dev(st):
    return SampleState(**{f: getattr(st, f).to(DEV).contiguous() for f in FIELDS})


def _bits(x):
    x = x.cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same_books(a, b):
    for f in FIELDS:
        assert torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))), f


def _case(lib, V, n, nb):
    """``kernel_case``'s rows for n * nb rows, laid out as n states of nb samples, the states in the slots in descending
    order; a fifth of the rows finished on entry; scores that are not zero."""
    lp = kernel_case(lib, V, n * nb)[0]
    seeds = 1000 + 7 * np.arange(n)
    active = list(range(n))[::-1]
    cum = np.linspace(-3, 3, n * nb, dtype=np.float32)
    finished = (np.arange(n * nb) % 5) == 2
    return torch.from_numpy(lp).to(DEV).contiguous(), seeds, active, cum, finished


# ---- the uniform call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nb", [(1, 1), (3, 5), (16, 64)])
@pytest.mark.parametrize("V", [3, 384, 512])
def test_the_uniform_call_is_rp_sample_step(V, n, nb):
    """With every ``pos = t`` the pool's step leaves ``rp_sample_step(t)``'s bits in all six arrays."""
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    lp, seeds, active, cum, finished = _case(lib, V, n, nb)
    t, max_len = KERNEL_T, 9
    for T, k, p in ((1.0, 0, 1.0), (0.7, 5, 0.9), (1.5, V, 0.1), (1.0, 1, 1.0)):
        one, two = (_to_dev(_host_state(n, nb, max_len, seeds, cum, finished)) for _ in range(2))
        dec.sample_step(lp, active, t, one, T, k, p, EOS, PAD)
        dec.sample_pool_step(lp, active, [t] * n, two, T, k, p, EOS, PAD)
        _same_books(one, two)
        seq = one.seq.cpu().numpy()
        assert (np.delete(seq, t + 1, axis=2) == -7).all() and (seq[:, :, t + 1] != -7).all()  # ... and something was drawn
        assert int(one.n_generated.sum()) == int((~finished).sum())


def test_mixed_positions_equal_single_state_calls():
    """Three states at positions (0, 5, max_len - 2) in one call, the active list permuted: what three single-state
    ``rp_sample_step`` calls leave, each at its own ``t``."""
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    V, n, nb, max_len = 384, 3, 5, 9
    lp, seeds, _, cum, finished = _case(lib, V, n, nb)
    P = {0: 0, 1: 5, 2: max_len - 2}
    active = [2, 0, 1]
    pos = [P[s] for s in active]
    for T, k, p in ((1.0, 0, 1.0), (1.2, 50, 0.95)):
        one, two = (_to_dev(_host_state(n, nb, max_len, seeds, cum, finished)) for _ in range(2))
        dec.sample_pool_step(lp, active, pos, one, T, k, p, EOS, PAD)
        for a, s in enumerate(active):  # slot a alone: its rows of lp, its rows of tokens_next
            _lib.check(lib.rp_sample_step(lp.data_ptr() + a * nb * V * 4, V, _p(_i32(s)), 1, n, nb, two.seeds.data_ptr(),
                                          P[s], max_len, T, k, p, EOS, PAD, two.seq.data_ptr(),
                                          two.tokens.data_ptr() + a * nb * 4, two.cum_logprob.data_ptr(),
                                          two.n_generated.data_ptr(), two.finished.data_ptr(), None), "rp_sample_step")
        _same_books(one, two)
        seq = one.seq.cpu().numpy()
        for s in range(n):  # column pos + 1 of every state, and no other
            assert (np.delete(seq[s], P[s] + 1, axis=1) == -7).all() and (seq[s, :, P[s] + 1] != -7).all()
    # a shared position is another result: the position enters the random number and the column
    shared = _to_dev(_host_state(n, nb, max_len, seeds, cum, finished))
    dec.sample_pool_step(lp, active, [pos[0]] * n, shared, 1.2, 50, 0.95, EOS, PAD)
    assert not torch.equal(shared.seq.cpu(), one.seq.cpu())


# ---- admission and the row rebuild ------------------------------------------------------------------------------------------
def _arenas(n, nb, max_len, fill):
    sizes = dict(seeds=n, seq=n * nb * max_len, cum_logprob=n * nb, n_generated=n * nb, finished=n * nb, tokens=n * nb)
    return {f: Arena(f, 4 * words, GUARD, DEV, init=fill) for f, words in sizes.items()}


def _arena_state(ar, n, nb, max_len):
    """Host copies of the arenas' payloads as a ``SampleState``."""
    shape = dict(seeds=(n,), seq=(n, nb, max_len), cum_logprob=(n, nb), n_generated=(n, nb), finished=(n, nb),
                 tokens=(n * nb,))
    return SampleState(**{f: ar[f].view(*shape[f], dtype=torch.float32 if f == "cum_logprob" else torch.int32).cpu().clone()
                          for f in FIELDS})


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x7F])
@pytest.mark.parametrize("max_len", [2, 9, 40])
def test_admit_resets_the_listed_states_over_all_columns_and_nothing_else(max_len, fill):
    lib = _lib.load()
    n, nb, start, pad = 4, 3, 5, 9
    ar = _arenas(n, nb, max_len, fill)
    want = _arena_state(ar, n, nb, max_len)
    states, seeds = [3, 1], [0xDEADBEEF, 7]
    _lib.check(lib.rp_sample_pool_admit(_p(_i32(*states)), _p(np.array(seeds, dtype=np.uint32)), 2, n, nb, max_len, start,
                                        pad, ar["seeds"].ptr, ar["seq"].ptr, ar["cum_logprob"].ptr, ar["n_generated"].ptr,
                                        ar["finished"].ptr, None), "rp_sample_pool_admit")
    torch.cuda.synchronize()
    sample_books_admit_host(want, states, seeds, start, pad)
    got = _arena_state(ar, n, nb, max_len)
    _same_books(got, want)  # every byte of every array: the listed states as specified, the others the fill
    for s in states:
        assert got.seq[s].tolist() == [[start] + [pad] * (max_len - 1)] * nb
        assert got.cum_logprob[s].tolist() == [0.0] * nb and got.n_generated[s].tolist() == [0] * nb
        assert got.finished[s].tolist() == [0] * nb
    assert got.seeds[3].item() == np.array(0xDEADBEEF, dtype=np.uint32).view(np.int32) and got.seeds[1].item() == 7
    word = int(np.frombuffer(bytes([fill] * 4), dtype=np.int32)[0])
    assert (got.seq[0] == word).all() and (got.seq[2] == word).all() and (got.tokens == word).all()  # nothing by row
    assert not any(a.broken_guards() for a in ar.values())


def test_rows_equal_the_host_restatement_on_a_permuted_shrunken_list():
    lib = _lib.load()
    n, nb, max_len = 4, 3, 9
    ar = _arenas(n, nb, max_len, 0x5A)
    g = torch.Generator().manual_seed(3)
    ar["seq"].view(n, nb, max_len, dtype=torch.int32).copy_(torch.randint(2, 300, (n, nb, max_len), generator=g,
                                                                         dtype=torch.int32))
    want = _arena_state(ar, n, nb, max_len)
    for active, pos in (([3, 0, 2, 1], [0, 7, 3, 5]), ([2, 0], [max_len - 2, 4]), ([1], [0])):
        _lib.check(lib.rp_sample_pool_rows(_p(_i32(*active)), _p(_i32(*pos)), len(active), n, nb, max_len, ar["seq"].ptr,
                                           ar["tokens"].ptr, None), "rp_sample_pool_rows")
        torch.cuda.synchronize()
        sample_books_rows_host(want, active, pos)
        got = _arena_state(ar, n, nb, max_len)
        _same_books(got, want)  # the listed rows; the rows past them and every other array as they were
        assert got.tokens[: nb].tolist() == want.seq[active[0], :, pos[0]].tolist()
    assert not any(a.broken_guards() for a in ar.values())


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_poisoned_outputs_untouched():
    lib = _lib.load()
    buf = torch.full((1 << 16,), 123, dtype=torch.int32, device=DEV)
    d, *parts = (buf.data_ptr() + i * 0x8000 for i in range(7))  # the log-probs, then the six arrays: 32 KiB apart
    d_seeds, d_seq, d_tok, d_cum, d_ngen, d_fin = parts
    ids = np.arange(32, dtype=np.int32)
    zeros = np.zeros(32, dtype=np.int32)
    useeds = np.arange(32, dtype=np.uint32)

    def step(V=384, na=2, n=2, nb=4, ml=8, T=1.0, k=0, p=1.0, lp=d, a=ids, pos=zeros, seeds=d_seeds, seq=d_seq, tok=d_tok,
             cum=d_cum, ngen=d_ngen, fin=d_fin):
        return lib.rp_sample_pool_step(lp, V, _p(a), _p(pos), na, n, nb, seeds, ml, T, k, p, EOS, PAD, seq, tok, cum, ngen,
                                       fin, None)

    def admit(s=ids, new=useeds, m=2, n=2, nb=4, ml=8, seeds=d_seeds, seq=d_seq, cum=d_cum, ngen=d_ngen, fin=d_fin):
        return lib.rp_sample_pool_admit(_p(s), _p(new), m, n, nb, ml, 5, PAD, seeds, seq, cum, ngen, fin, None)

    def rows(a=ids, pos=zeros, na=2, n=2, nb=4, ml=8, seq=d_seq, tok=d_tok):
        return lib.rp_sample_pool_rows(_p(a), _p(pos), na, n, nb, ml, seq, tok, None)

    def refused(fn, word, **kw):
        assert fn(**kw) == -1, (fn.__name__, kw)
        msg = lib.rp_last_error()
        assert msg and word in msg, (fn.__name__, kw, msg)

    # everything rp_sample_step refuses
    for kw, word in ((dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(T=float("nan")), b"temperature"),
                     (dict(T=float("inf")), b"temperature"), (dict(p=0.0), b"top_p"), (dict(p=1.5), b"top_p"),
                     (dict(k=-1), b"top_k"), (dict(V=513), b"vocab"), (dict(V=0), b"vocab"), (dict(nb=65), b"nb=65"),
                     (dict(nb=0), b"nb=0"), (dict(na=17, n=17, nb=64), b"rows"), (dict(n=33, na=33), b"states=33"),
                     (dict(n=0, na=0), b"states=0"), (dict(na=3), b"active states=3"), (dict(na=0), b"active states=0"),
                     (dict(ml=1), b"max_len=1"), (dict(lp=None), b"null"), (dict(a=None), b"null"),
                     (dict(seeds=None), b"null"), (dict(seq=None), b"null"), (dict(tok=None), b"null"),
                     (dict(cum=None), b"null"), (dict(ngen=None), b"null"), (dict(fin=None), b"null"),
                     (dict(a=_i32(1, 1)), b"twice"), (dict(a=_i32(0, 2)), b"active[1]=2"), (dict(a=_i32(-1, 0)), b"active[0]=-1"),
                     # ... and a null pos or a pos outside [0, max_len - 2]
                     (dict(pos=None), b"null"), (dict(pos=_i32(0, 7)), b"pos[1]=7"), (dict(pos=_i32(-1, 0)), b"pos[0]=-1")):
        refused(step, word, **kw)
    for kw, word in ((dict(s=None), b"null"), (dict(new=None), b"null"), (dict(seeds=None), b"null"), (dict(seq=None), b"null"),
                     (dict(cum=None), b"null"), (dict(ngen=None), b"null"), (dict(fin=None), b"null"),
                     (dict(m=0), b"admitted states=0"), (dict(m=3), b"admitted states=3"), (dict(s=_i32(1, 1)), b"twice"),
                     (dict(s=_i32(0, 2)), b"states[1]=2"), (dict(s=_i32(-1, 0)), b"states[0]=-1"), (dict(nb=0), b"nb=0"),
                     (dict(nb=65), b"nb=65"), (dict(n=0), b"states=0"), (dict(n=33), b"states=33"),
                     (dict(m=17, n=17, nb=64), b"rows"), (dict(ml=1), b"max_len=1")):
        refused(admit, word, **kw)
    for kw, word in ((dict(a=None), b"null"), (dict(pos=None), b"null"), (dict(seq=None), b"null"), (dict(tok=None), b"null"),
                     (dict(na=0), b"active states=0"), (dict(na=3), b"active states=3"), (dict(a=_i32(1, 1)), b"twice"),
                     (dict(a=_i32(0, 2)), b"active[1]=2"), (dict(a=_i32(-1, 0)), b"active[0]=-1"),
                     (dict(pos=_i32(0, 7)), b"pos[1]=7"), (dict(pos=_i32(-1, 0)), b"pos[0]=-1"), (dict(nb=0), b"nb=0"),
                     (dict(nb=65), b"nb=65"), (dict(n=0), b"states=0"), (dict(n=33), b"states=33"),
                     (dict(na=17, n=17, nb=64), b"rows"), (dict(ml=1), b"max_len=1")):
        refused(rows, word, **kw)
    torch.cuda.synchronize()
    assert bool((buf == 123).all())  # nothing was launched
    for fn, kw in ((step, dict(pos=_i32(0, 6))), (admit, {}), (rows, dict(pos=_i32(0, 6)))):  # the accepted calls do write
        before = buf.clone()
        assert fn(**kw) == 0, fn.__name__
        torch.cuda.synchronize()
        assert not torch.equal(buf, before), fn.__name__


# ---- whole streams ----------------------------------------------------------------------------------------------------------
KW = dict(temperature=1.2, top_k=50, top_p=0.95)
LENGTHS = (60, 7, 33, 300, 1, 120, 64)
SEEDS = (21, 22, 23, 0xFFFFFFF0, 25, 26, 27)
_ALONE = {}


@pytest.fixture(scope="module")
def tiny_gen():
    return _gen("tiny", eos_boost=4.0)  # EOS boosted: the states end at different lengths


def _same(a, b):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)  # bits


def _alone(gen, nb, ml):
    """``sample`` of every source by itself, once per shape and left unchanged."""
    if (nb, ml) not in _ALONE:
        _ALONE[(nb, ml)] = [gen.sample(source_ids(n, 30 + i), nb, ml, seed=s, **KW)
                            for i, (n, s) in enumerate(zip(LENGTHS, SEEDS))]
    return _ALONE[(nb, ml)]


@pytest.mark.parametrize("sync_every", [1, 3, 16])
@pytest.mark.parametrize("ml", [40, 4])
def test_tiny_stream_equals_sample_alone(tiny_gen, ml, sync_every):
    """Seven sources through three slots: every ticket is ``sample`` alone, bit for bit.  At ``max_length`` 4 every
    state ends by length, at the forced sync point."""
    cfg, gen = tiny_gen
    dec = gen.decoder
    nb, n_slots = 6, 3
    want = _alone(gen, nb, ml)
    srcs = [source_ids(n, 30 + i) for i, n in enumerate(LENGTHS)]
    stream = gen.sample_stream(nb, ml, n_slots=n_slots, src_cap=512, sync_every=sync_every, **KW)
    assert isinstance(stream, SampleStream) and isinstance(stream.pool, SamplePool) and stream.pool.state.seq.is_cuda
    steps, admitted, copies = [], [], []
    pool_step, pool_admit, to_host = dec.pool_step, dec.pool_admit, stream.pool._to_host

    def counted(x):
        copies.append(tuple(x.shape))
        return to_host(x)

    stream.pool._to_host = counted
    dec.pool_step = lambda active, pos, *a, **k: (steps.append((list(active), list(pos))), pool_step(active, pos, *a, **k))[1]
    dec.pool_admit = lambda slots, *a, **k: (admitted.extend(int(s) for s in slots), pool_admit(slots, *a, **k))[1]
    try:
        tickets = [stream.submit(s, seed) for s, seed in zip(srcs, SEEDS)]
        assert stream.queued == len(srcs) and stream.in_flight == 0
        got = dict(stream.drain())
    finally:
        del dec.pool_step, dec.pool_admit
    assert sorted(got) == sorted(tickets) and stream.queued == 0 and stream.in_flight == 0
    for t, w in zip(tickets, want):
        _same(got[t], w)
    lens = [w.sequences.shape[1] - 1 for w in want]
    print("lengths alone:", lens, "steps", stream.steps, "sync points", stream.pool.sync_points, "copies", copies)
    assert all(0 <= p <= ml - 2 for _, pos in steps for p in pos) and len(steps) == stream.steps
    assert len(admitted) == len(srcs) > len(set(admitted)) and set(admitted) <= set(range(n_slots))  # a slot served twice
    assert len(copies) <= 2 * stream.pool.sync_points
    row = nb * ml + 2 * nb
    assert all(c == (n_slots,) or (len(c) == 2 and c[1] == row) for c in copies)
    assert sum(c[0] for c in copies if len(c) == 2) == len(srcs)
    if ml == 40:
        assert len(set(lens)) > 1 and any(n < ml - 1 for n in lens), lens  # the states end at different lengths, some by EOS
        if sync_every < 16:  # (at 16 the slots fall into step; the ticket test below staggers the arrivals)
            assert any(len(set(pos)) > 1 for _, pos in steps), "no call carried two distinct positions"
    else:
        assert max(lens) == ml - 1  # ended by length, at the forced sync point


def test_staggered_arrivals_then_a_beam_stream_retires_the_sample_stream(tiny_gen):
    cfg, gen = tiny_gen
    nb, ml = 6, 40
    want = _alone(gen, nb, ml)
    srcs = [source_ids(n, 30 + i) for i, n in enumerate(LENGTHS)]
    stream = gen.sample_stream(nb, ml, n_slots=3, src_cap=512, sync_every=16, **KW)
    steps = []
    pool_step = gen.decoder.pool_step
    gen.decoder.pool_step = lambda active, pos, *a, **k: (steps.append(list(pos)), pool_step(active, pos, *a, **k))[1]
    got, tickets = {}, []
    try:
        for s, seed in zip(srcs, SEEDS):
            tickets.append(stream.submit(s, seed))
            for _ in range(2):
                got.update(stream.step())
        got.update(stream.drain())
    finally:
        del gen.decoder.pool_step
    for t, w in zip(tickets, want):
        _same(got[t], w)
    assert any(len(set(pos)) > 1 for pos in steps)
    # the decoder carries one stream at a time, of either kind
    t = stream.submit(srcs[0], 1)
    beam = gen.generate_stream(4, 8, 1.0, n_slots=2, src_cap=512)
    with pytest.raises(RuntimeError, match="retired"):
        stream.step()
    ticket = beam.submit(srcs[1])
    assert [tk for tk, _ in beam.drain()] == [ticket]
    again = gen.sample_stream(nb, ml, n_slots=3, src_cap=512, **KW)  # ... and a sample stream retires the beam stream
    beam.submit(srcs[1])
    with pytest.raises(RuntimeError, match="retired"):
        beam.step()
    t = again.submit(srcs[2], SEEDS[2])
    _same(dict(again.drain())[t], want[2])


def test_stream_arguments(tiny_gen):
    cfg, gen = tiny_gen
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1), dict(num_samples=0), dict(max_length=1),
               dict(sync_every=0), dict(sync_every=1.5), dict(n_slots=0)):
        args = dict(num_samples=2, max_length=8)
        args.update(kw)
        with pytest.raises(ValueError):
            gen.sample_stream(**args)
    stream = gen.sample_stream(2, 8, src_cap=16)
    with pytest.raises(ValueError):
        stream.submit(source_ids(17, 1), 0)
    assert stream.step() == [] and stream.steps == 0


def test_byt5_small_dimensions():
    """ByT5-small dimensions, sources of 300, 2048 and 1 bytes through 2 slots, 8 samples, max_length 32."""
    cfg, gen = _gen("byt5-small")
    srcs = [source_ids(300, 8), source_ids(2048, 9), source_ids(1, 10)]
    kw = dict(temperature=0.9, top_k=0, top_p=0.9)
    alone = [gen.sample(s, 8, 32, seed=70 + i, **kw) for i, s in enumerate(srcs)]
    stream = gen.sample_stream(8, 32, n_slots=2, **kw)
    tickets = [stream.submit(s, 70 + i) for i, s in enumerate(srcs)]
    got = dict(stream.drain())
    for t, a in zip(tickets, alone):
        _same(got[t], a)


# ---- product ----------------------------------------------------------------------------------------------------------------
def test_gathered_generate_equals_a_fresh_objects_generate_sync(tmp_path):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= 4.0
    gdir = str(tmp_path / "gen")
    _save_generator_dir(gdir, cfg, sd)
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900, 33)]
    kw = dict(do_sample=True, temperature=1.2, top_k=50, top_p=0.95, seed=11)
    hf = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, sample_stream=True, sample_stream_slots=2, sample_sync_every=4, **kw)
    hf.initialize()
    fresh = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, **kw)
    fresh.initialize()
    args = ("f.lean", "thm", Pos(1, 0), 8)

    async def main():
        return await asyncio.gather(*(hf.generate(s, *args) for s in states))

    got = asyncio.run(main())
    assert got == [fresh.generate_sync(s, *args) for s in states]  # tactics, scores (exact floats), order
    assert all(got)
    assert hf._driver is None and not hf._waiters and hf._stream.in_flight == 0 and hf._stream.queued == 0
    assert isinstance(hf._stream.pool, SamplePool) and hf._stream.pool.n_slots == 2 and hf._stream.pool.sync_every == 4
