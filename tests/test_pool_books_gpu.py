"""The slot pool's books on the MI355X (rp_beam_books_admit / rp_beam_pool_advance / rp_beam_books_rows,
generate_stream(sync_every=...), HuggingFaceGenerator(continuous=True, beam_sync_every=...)): the three kernels alone
against their host restatements on a scripted pool, bit for bit over the whole block; the uniform call against
rp_beam_advance; their refusals; whole streams against ``generate`` and against the host-books stream; the stream's
device-to-host copies counted; a slot taken again over poisoned memory.  Every comparison is equality."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from hip_helpers import Arena  # noqa: E402
from test_beam_books_gpu import _divs, _script  # noqa: E402
from test_generate_batch_gpu import _g20, _same_output, _save_generator_dir, _sources  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402
from reprover_amd.generation import (BeamBooks, BeamBooksPool, beam_advance_host, beam_books_admit_host,  # noqa: E402
                                     beam_books_bytes, beam_books_init_host, beam_books_rows_host,
                                     beam_pool_advance_host)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, START = 1, 0
GUARD = 1 << 20
C = _lib.C
PARTS = ("run_seq", "anc", "fin_seq", "run_scores", "beam_scores", "fin_flag", "fin_len", "heur", "done", "steps", "tokens",
         "running", "anc_rows")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _f32(*v):
    return np.array(v, dtype=np.float32)


def _differing_parts(n, nb, ml, got, ref):
    view = BeamBooks(n, nb, ml, block=got)
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x  # noqa: E731
    return [f for f in PARTS if not torch.equal(bits(getattr(view, f)), bits(getattr(ref, f)))]


# ---- the kernels alone -----------------------------------------------------------------------------------------------------
LP = 0.7  # the divisors (pos + 1) ** LP differ between the slots of a step


def _pool_script(nb, ml, seed):
    """A pool of three slots as a list of calls: ("admit", states), ("rows", active, pos), ("advance", active, pos,
    scores, tokens, parents).  Slot 0 is taken at step 0 by a tenant that stops by the heuristic after position
    min(2, ml - 2), is fed on, and is taken again at step 6 by one that stops at its first step (earlier than its
    predecessor, whose columns the admission must reset).  Slot 1 is taken at step 1 and runs to max_len: EOS among its
    first nb candidates at position 1 (nb > 1), only among the second nb at position 2, exact ties (the two best, the
    two worst) at odd positions from 3 on, signed zeros at position 4.  Slot 2 is taken at step 3 - so the three stand at
    positions of both parities - and stops at its first step.  The active lists are permuted, shrink and keep feeding
    stopped states (their host position goes on, held at ml - 2); ``rows`` follows every change of the list."""
    g = torch.Generator().manual_seed(seed)
    K = 2 * nb
    lists = {0: [0], 1: [0, 1], 2: [1, 0], 3: [2, 0, 1], 4: [1, 2, 0], 5: [0, 1], 6: [0, 1], 7: [1, 0]}
    admits = {0: [0], 1: [1], 3: [2], 6: [0]}
    kind = {0: "heuristic", 1: "runner", 2: "first"}
    pos, calls, prev = {}, [], None
    for step in range(max(ml, 9)):
        active = lists.get(step, [1, 0] if step % 5 == 0 else [1])
        if step in admits:
            calls.append(("admit", admits[step]))
            for s in admits[step]:
                pos[s] = 0
            if step == 6:
                kind[0] = "first"
        if active != prev or step in admits:
            calls.append(("rows", active, [pos[s] for s in active]))
        sc, tk, pr = [], [], []
        for s in active:
            p = pos[s]
            vals = torch.sort(-30.0 * torch.rand(K, generator=g), descending=True)[0]
            toks = torch.randint(2, 20, (K,), generator=g, dtype=torch.int32)
            pars = torch.randint(0, nb, (K,), generator=g, dtype=torch.int32)
            if (kind[s] == "heuristic" and p == min(2, ml - 2)) or (kind[s] == "first" and p == 0):
                toks[:nb] = EOS
                vals[nb:] -= 50.0
            if kind[s] == "runner":
                if p == 1 and nb > 1:
                    toks[0] = EOS
                if p == 2:
                    toks[nb] = EOS
                if p >= 3 and p % 2 == 1:
                    vals[1 % K] = vals[0]
                    vals[K - 1] = vals[K - 2]
                if p == 4:
                    vals[0], vals[1 % K] = -0.0, 0.0
            sc.append(vals)
            tk.append(toks)
            pr.append(pars)
        calls.append(("advance", active, [pos[s] for s in active], torch.stack(sc), torch.stack(tk), torch.stack(pr)))
        for s in active:
            pos[s] = min(pos[s] + 1, ml - 2)
        prev = active
    return calls


def _pool_divs(pos):
    return [float((p + 1) ** LP) for p in pos], [float((p + 1) ** LP) for p in pos]


def _run_pool_kernels(lib, nb, ml, calls, fill):
    """The calls through the three entry points on a block of exactly rp_beam_books_bytes between guards, poisoned with
    ``fill`` and then initialised; after every call the whole block equals the restatement's.  The first call of each
    kind is first made with one byte less and refused.  Returns (final block, the restatement's books, what
    (steps, heur, done) were before every admission)."""
    n = 3
    need = lib.rp_beam_books_bytes(n, nb, ml)
    assert need == beam_books_bytes(n, nb, ml) and need % 16 == 0
    arena = Arena("books", need, GUARD, DEV, init=fill)
    ref = beam_books_init_host(n, nb, ml, EOS, START)
    _lib.check(lib.rp_beam_books_init(arena.ptr, need, n, nb, ml, EOS, START, None), "rp_beam_books_init")
    block = lambda: arena.view(dtype=torch.int32).cpu()  # noqa: E731
    assert torch.equal(block(), ref.block), "init"
    seen, history = set(), []
    for i, call in enumerate(calls):
        kind = call[0]
        if kind == "admit":
            history.append((ref.steps.tolist(), ref.heur.tolist(), ref.done.tolist()))
            st = _i32(*call[1])
            run = lambda nbytes: lib.rp_beam_books_admit(arena.ptr, nbytes, n, nb, ml, _p(st), len(st), EOS, START,  # noqa: E731
                                                         None)
            host = lambda: beam_books_admit_host(ref, call[1], EOS, START)  # noqa: E731
        elif kind == "rows":
            act, ps = _i32(*call[1]), _i32(*call[2])
            run = lambda nbytes: lib.rp_beam_books_rows(arena.ptr, nbytes, n, nb, ml, _p(act), _p(ps), len(act), None)  # noqa: E731
            host = lambda: beam_books_rows_host(ref, call[1], call[2])  # noqa: E731
        else:
            act, ps = _i32(*call[1]), _i32(*call[2])
            fd, rd = _pool_divs(call[2])
            fda, rda = _f32(*fd), _f32(*rd)
            d_sc, d_tk, d_pr = (x.to(DEV).contiguous() for x in call[3:6])
            run = lambda nbytes: lib.rp_beam_pool_advance(arena.ptr, nbytes, n, nb, ml, _p(act), _p(ps), len(act),  # noqa: E731
                                                          d_sc.data_ptr(), d_tk.data_ptr(), d_pr.data_ptr(), _p(fda),
                                                          _p(rda), EOS, None)
            host = lambda: beam_pool_advance_host(ref, call[1], call[2], *call[3:6], fd, rd, EOS)  # noqa: E731
        if kind not in seen:  # one byte less is refused, nothing written
            seen.add(kind)
            before = block()
            assert run(need - 1) == -1 and b"books" in lib.rp_last_error(), kind
            torch.cuda.synchronize()
            assert torch.equal(block(), before), kind
        _lib.check(run(need), kind)
        host()
        got = block()
        if not torch.equal(got, ref.block):
            raise AssertionError(f"call {i} {call[:3]}: parts {_differing_parts(n, nb, ml, got, ref)} differ from the "
                                 "restatement")
    assert not arena.broken_guards()
    assert seen == {"admit", "rows", "advance"}
    return block(), ref, history


@pytest.mark.parametrize("nb", [1, 2, 3, 64])
@pytest.mark.parametrize("ml", [2, 3, 5, 40])
def test_pool_kernels_alone_equal_the_restatements(nb, ml):
    """max_len 5 takes the one-column gather, 40 the 16-byte one."""
    lib = _lib.load()
    calls = _pool_script(nb, ml, seed=1000 * nb + ml)
    pos_lists = [c[2] for c in calls if c[0] == "advance"]
    assert any(len({p & 1 for p in ps}) > 1 for ps in pos_lists) or ml == 2  # slots of one call at both parities
    a, ref, history = _run_pool_kernels(lib, nb, ml, calls, 0x5A)
    b, _, _ = _run_pool_kernels(lib, nb, ml, calls, 0xFF)
    assert torch.equal(a, b)  # nothing depends on what the block held
    steps, heur, done = ref.steps.tolist(), ref.heur.tolist(), ref.done.tolist()
    before_retake = history[3]  # (steps, heur, done) when slot 0 was taken again
    print("before slot 0 was taken again", before_retake, "final steps", steps, "heur", heur, "done", done)
    assert done == [1, 1, 1] and before_retake[2][0] == 1  # the first tenant had stopped
    assert steps[0] == 1 and steps[2] == 1 and steps[1] == ml - 1  # the first step (twice); max_len
    if ml == 40:  # the three kinds of stop: the heuristic after position 2, max_len, the first step
        assert before_retake[0][0] == 3 and before_retake[1][0] == 0  # ... later than its successor reaches
        assert heur[0] == 0 and heur[2] == 0
    assert before_retake[0][0] >= steps[0]


def test_admit_and_rows_touch_nothing_else():
    """On a block that was never initialised (0x5A everywhere) an admission writes the by-state parts of its states and a
    ``rows`` the by-row parts of its rows: every other byte keeps the fill, as in the restatement."""
    lib = _lib.load()
    n, nb, ml = 4, 3, 12
    need = lib.rp_beam_books_bytes(n, nb, ml)
    arena = Arena("books", need, GUARD, DEV, init=0x5A)
    ref = BeamBooks(n, nb, ml)
    ref.block.view(torch.uint8).fill_(0x5A)
    block = lambda: arena.view(dtype=torch.int32).cpu()  # noqa: E731
    st = _i32(3, 1)
    _lib.check(lib.rp_beam_books_admit(arena.ptr, need, n, nb, ml, _p(st), 2, EOS, START, None), "rp_beam_books_admit")
    beam_books_admit_host(ref, [3, 1], EOS, START)
    assert torch.equal(block(), ref.block), _differing_parts(n, nb, ml, block(), ref)
    assert int(ref.done[0]) == 0x5A5A5A5A and int(ref.tokens[0]) == 0x5A5A5A5A  # another state; the by-row parts
    act, ps = _i32(3, 1), _i32(0, 0)
    _lib.check(lib.rp_beam_books_rows(arena.ptr, need, n, nb, ml, _p(act), _p(ps), 2, None), "rp_beam_books_rows")
    beam_books_rows_host(ref, [3, 1], [0, 0])
    assert torch.equal(block(), ref.block), _differing_parts(n, nb, ml, block(), ref)
    assert int(ref.tokens[0]) == START and int(ref.tokens[2 * nb]) == 0x5A5A5A5A  # rows 0 .. 2 nb - 1 only
    assert not arena.broken_guards()


@pytest.mark.parametrize("nb,ml", [(1, 2), (3, 5), (2, 40), (64, 40)])
def test_the_uniform_call_is_rp_beam_advance(nb, ml):
    """tests/test_beam_books_gpu.py's script through rp_beam_advance and through rp_beam_pool_advance with every
    pos = t: the same block after every call (and the restatement's)."""
    lib = _lib.load()
    n = 3
    need = lib.rp_beam_books_bytes(n, nb, ml)
    one, two = (Arena(name, need, GUARD, DEV, init=0x5A) for name in ("books_t", "books_pos"))
    ref = beam_books_init_host(n, nb, ml, EOS, START)
    for a in (one, two):
        _lib.check(lib.rp_beam_books_init(a.ptr, need, n, nb, ml, EOS, START, None), "rp_beam_books_init")
    for t, (active, triples) in enumerate(_script(nb, ml, seed=1000 * nb + ml)):
        sc, tk, pr = (torch.stack([triples[s][j] for s in active]) for j in range(3))
        d = [x.to(DEV).contiguous() for x in (sc, tk, pr)]
        ptrs = [x.data_ptr() for x in d]
        act, k = _i32(*active), len(active)
        fd, rd = _divs(t)
        _lib.check(lib.rp_beam_advance(one.ptr, need, n, nb, ml, _p(act), k, t, *ptrs, fd, rd, EOS, None), "rp_beam_advance")
        _lib.check(lib.rp_beam_pool_advance(two.ptr, need, n, nb, ml, _p(act), _p(_i32(*[t] * k)), k, *ptrs,
                                            _p(_f32(*[fd] * k)), _p(_f32(*[rd] * k)), EOS, None), "rp_beam_pool_advance")
        beam_advance_host(ref, active, t, sc, tk, pr, fd, rd, EOS)
        x, y = one.view(dtype=torch.int32).cpu(), two.view(dtype=torch.int32).cpu()
        assert torch.equal(x, y), (t, _differing_parts(n, nb, ml, y, BeamBooks(n, nb, ml, block=x)))
        assert torch.equal(x, ref.block), t
    assert not one.broken_guards() and not two.broken_guards()


def test_pool_books_refusals_leave_the_books_untouched():
    lib = _lib.load()
    n, nb, ml = 3, 4, 9
    need = lib.rp_beam_books_bytes(n, nb, ml)
    arena = Arena("books", need, GUARD, DEV, init=0x5A)
    _lib.check(lib.rp_beam_books_init(arena.ptr, need, n, nb, ml, EOS, START, None), "rp_beam_books_init")
    K = 2 * nb
    sc = torch.zeros((n, K), dtype=torch.float32, device=DEV)
    tk = torch.full((n, K), 5, dtype=torch.int32, device=DEV)
    pr = torch.zeros((n, K), dtype=torch.int32, device=DEV)
    d = (sc.data_ptr(), tk.data_ptr(), pr.data_ptr())
    torch.cuda.synchronize()
    before = arena.payload().clone()
    ones = _f32(1, 1, 1)

    def adv(books=arena.ptr, nbytes=need, n=n, nb=nb, ml=ml, a=_i32(0, 1, 2), p=_i32(0, 3, 7), na=3, ptrs=d, fd=ones,
            rd=ones):
        return lib.rp_beam_pool_advance(books, nbytes, n, nb, ml, _p(a), _p(p), na, *ptrs, _p(fd), _p(rd), EOS, None)

    def rows(books=arena.ptr, nbytes=need, n=n, nb=nb, ml=ml, a=_i32(0, 1, 2), p=_i32(0, 3, 7), na=3):
        return lib.rp_beam_books_rows(books, nbytes, n, nb, ml, _p(a), _p(p), na, None)

    def admit(books=arena.ptr, nbytes=need, n=n, nb=nb, ml=ml, s=_i32(2, 0), m=2):
        return lib.rp_beam_books_admit(books, nbytes, n, nb, ml, _p(s), m, EOS, START, None)

    def refused(fn, word, **kw):
        assert fn(**kw) == -1, (fn.__name__, kw)
        msg = lib.rp_last_error()
        assert msg and word in msg, (fn.__name__, kw, msg)

    for fn in (adv, rows):
        refused(fn, b"null", books=None)
        refused(fn, b"null", a=None)
        refused(fn, b"null", p=None)
        refused(fn, b"twice", a=_i32(1, 1, 2))
        refused(fn, b"active[1]=3", a=_i32(0, 3, 2))
        refused(fn, b"active[1]=-1", a=_i32(0, -1, 2))
        refused(fn, b"active states=0", na=0)
        refused(fn, b"active states=4", na=4)
        refused(fn, b"pos[2]=8", p=_i32(0, 3, ml - 1))
        refused(fn, b"pos[0]=-1", p=_i32(-1, 3, 7))
    refused(adv, b"null", ptrs=(None, d[1], d[2]))
    refused(adv, b"null", ptrs=(d[0], None, d[2]))
    refused(adv, b"null", ptrs=(d[0], d[1], None))
    refused(adv, b"null", fd=None)
    refused(adv, b"null", rd=None)
    refused(admit, b"null", books=None)
    refused(admit, b"null", s=None)
    refused(admit, b"twice", s=_i32(2, 2))
    refused(admit, b"states[1]=3", s=_i32(2, 3))
    refused(admit, b"states[0]=-1", s=_i32(-1, 0))
    refused(admit, b"admitted states=0", m=0)
    refused(admit, b"admitted states=4", s=_i32(0, 1, 2, 2), m=4)
    for fn in (adv, rows, admit):
        refused(fn, b"nb=0", nb=0)
        refused(fn, b"nb=65", nb=65)
        refused(fn, b"states=0", n=0)
        refused(fn, b"states=33", n=33)
        refused(fn, b"rows", n=17, nb=64)
        refused(fn, b"max_len=1", ml=1)
        refused(fn, b"max_len=8193", ml=8193)
        refused(fn, b"books", nbytes=need - 1)
    torch.cuda.synchronize()
    assert torch.equal(arena.payload(), before) and not arena.broken_guards()
    for fn in (adv, admit, rows):  # and the accepted calls do change them (rows: after the admission reset run_scores)
        assert fn() == 0, fn.__name__
        torch.cuda.synchronize()
        now = arena.payload().clone()
        assert not torch.equal(now, before), fn.__name__
        before = now
    assert not arena.broken_guards()


# ---- whole streams ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_gen(golden_dir):
    z, cfg, sd = _g20(golden_dir)
    return z, cfg, sd, HipT5Generator(cfg, sd, DEV)


_ALONE, _HOST_STREAM = {}, {}


def _alone(gen, key, src, nb, ml, lp):
    """(generate(src), the position it stopped after) once per (source, shape)"""
    k = (key, nb, ml, lp)
    if k not in _ALONE:
        trace = []
        _ALONE[k] = (gen.generate(src, nb, ml, lp, trace=trace), len(trace))
    return _ALONE[k]


def _run_stream(gen, srcs, nb, ml, lp, n_slots, schedule, **kw):
    stream = gen.generate_stream(nb, ml, lp, n_slots=n_slots, src_cap=512, **kw)
    got, tickets = {}, []
    if schedule == "one_every_3_steps":
        for s in srcs:
            tickets.append(stream.submit(s))
            for _ in range(3):
                got.update(stream.step())
    else:
        tickets = [stream.submit(s) for s in srcs]
    while stream.queued or stream.in_flight:
        got.update(stream.step())
    assert sorted(got) == sorted(tickets)
    return [got[t] for t in tickets], stream


@pytest.mark.parametrize("k", [1, 4, 100])
@pytest.mark.parametrize("schedule", ["all_at_once", "one_every_3_steps", "a_slot_each"])
@pytest.mark.parametrize("lp", [0.0, 1.0])
@pytest.mark.parametrize("nb,n_src,n_slots,ml", [(4, 5, 2, 64), (64, 4, 3, 128)])
def test_stream_with_device_books_equals_generate(tiny_gen, nb, n_src, n_slots, ml, lp, schedule, k):
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])[:n_src]
    slots = None if schedule == "a_slot_each" else n_slots
    hk = (nb, ml, lp, schedule)
    if hk not in _HOST_STREAM:  # the host-books stream, once per shape and schedule
        _HOST_STREAM[hk] = _run_stream(gen, srcs, nb, ml, lp, slots, schedule)[0]
    outs, stream = _run_stream(gen, srcs, nb, ml, lp, slots, schedule, sync_every=k)
    pool = stream.pool
    assert isinstance(pool, BeamBooksPool) and pool.books.block.is_cuda and pool.sync_every == k
    stops = [_alone(gen, i, s, nb, ml, lp)[1] for i, s in enumerate(srcs)]
    print("stop positions:", stops, "steps", pool.steps, "sync points", pool.sync_points)
    for i, s in enumerate(srcs):
        _same_output(outs[i], _alone(gen, i, s, nb, ml, lp)[0])
        _same_output(outs[i], _HOST_STREAM[hk][i])
    if nb == 4 and lp == 0.0:  # departures and re-admission at different positions are really exercised
        assert len(set(stops)) >= 2, stops


def test_stream_sync_every_arguments(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sync_every"):
            gen.generate_stream(4, 8, 1.0, n_slots=2, src_cap=16, sync_every=bad)
    with pytest.raises(ValueError):
        gen.generate_stream(4, 1, 1.0, n_slots=2, src_cap=16, sync_every=2)
    stream = gen.generate_stream(4, 2, 0.0, n_slots=2, src_cap=16, sync_every=3)  # max_length 2: one position
    tickets = [stream.submit(source_ids(n, n)) for n in (16, 3, 5)]
    got = dict(stream.drain())
    for t, n in zip(tickets, (16, 3, 5)):
        _same_output(got[t], gen.generate(source_ids(n, n), 4, 2, 0.0))


@pytest.mark.parametrize("k", [1, 4, 100])
def test_the_stream_makes_no_per_step_transfer(tiny_gen, k):
    """The test's own ``BeamBooksPool`` over the engine's callables: every tensor handed to and returned by ``step`` /
    ``select`` / ``advance`` / ``rows`` is on the device and int32 / fp32; every device-to-host copy goes through
    ``to_host``: at most two per sync point, the ``n_slots`` flags or one result buffer of the states that stopped,
    never the block."""
    z, cfg, sd, gen = tiny_gen
    dec = gen.decoder
    srcs = _sources(z["src"])[:5]
    nb, L, lp, n_slots = 4, 64, 0.0, 2
    stream = gen.generate_stream(nb, L, lp, n_slots=n_slots, src_cap=512, sync_every=k)  # opens the decoder's slot pool
    calls = {"step": 0, "select": 0, "advance": 0, "rows": 0, "admit": 0}
    copies = []

    def on_device(*xs):
        assert all(x.is_cuda and x.dtype in (torch.int32, torch.float32) for x in xs)

    def admit(slots, sources):
        calls["admit"] += 1
        stream._admit(slots, sources)

    def step(active, pos, tokens, ancestry):
        calls["step"] += 1
        on_device(tokens, ancestry)
        assert tokens.dtype == torch.int32 and ancestry.dtype == torch.int32 and ancestry.shape == (len(active) * nb, L)
        assert all(0 <= p <= L - 2 for p in pos)
        out = stream._step(active, pos, tokens, ancestry)
        on_device(out)
        return out

    def select(log_probs, running, nb_, k_):
        calls["select"] += 1
        on_device(log_probs, running)
        outs = dec.select_many(log_probs, running, nb_, k_)
        on_device(*outs)
        return outs

    def advance(books, active, pos, *rest):
        calls["advance"] += 1
        on_device(books.block, *rest[:3])
        assert all(isinstance(x, float) for x in rest[3] + rest[4])  # the divisors travel by value
        dec.beam_pool_advance(books, active, pos, *rest)

    def rows(books, active, pos):
        calls["rows"] += 1
        on_device(books.block)
        dec.beam_books_rows(books, active, pos)

    def to_host(x):
        copies.append(tuple(x.shape))
        return x.cpu()

    pool = BeamBooksPool(admit, step, n_slots, nb, L, lp, EOS, START, select_many=select, device=gen.device, sync_every=k,
                         books_admit=dec.beam_books_admit, advance=advance, rows=rows, to_host=to_host)
    tickets = [pool.submit(s) for s in srcs]
    got = dict(pool.drain())
    for i, (t, s) in enumerate(zip(tickets, srcs)):
        _same_output(got[t], _alone(gen, i, s, nb, L, lp)[0])
    steps = calls["step"]
    print("steps", steps, "sync points", pool.sync_points, "admissions", calls["admit"], "copies", copies)
    assert steps == calls["select"] == calls["advance"] == pool.steps
    assert len(copies) <= 2 * pool.sync_points
    assert pool.sync_points <= -(-steps // k) + calls["admit"] + 1
    assert calls["rows"] <= pool.sync_points
    row = nb * L + 2 * nb + 1
    for shape in copies:  # the flags, or the stopped states' results: never the block
        assert shape == (n_slots,) or (len(shape) == 2 and 1 <= shape[0] <= n_slots and shape[1] == row), shape
    assert sum(s[0] for s in copies if len(s) == 2) == len(srcs)
    assert max(int(np.prod(s)) for s in copies) * 4 < beam_books_bytes(n_slots, nb, L)


def test_a_slot_taken_again_over_poisoned_memory(tiny_gen):
    """One slot: a 300-token source runs in it to position 40 at the most (max_length 42), then a 3-token source takes
    it.  Both outputs are ``generate``'s bits with the pool workspace and the books block pre-filled with 0x00, 0xFF and
    0x7F."""
    z, cfg, sd, gen = tiny_gen
    nb, ml, lp = 4, 42, 0.0
    old, new = source_ids(300, 41), source_ids(3, 42)
    want = [gen.generate(s, nb, ml, lp) for s in (old, new)]
    for fill in (0x00, 0xFF, 0x7F):
        stream = gen.generate_stream(nb, ml, lp, n_slots=1, src_cap=300, sync_every=4)
        gen.decoder._pool_ws.fill_(fill)
        stream.pool.books.block.view(torch.uint8).fill_(fill)
        tickets = [stream.submit(old), stream.submit(new)]
        got = dict(stream.drain())
        for t, w in zip(tickets, want):
            _same_output(got[t], w)
        assert stream._src_len == [3] and stream.pool.sync_points >= 2


# ---- product ---------------------------------------------------------------------------------------------------------------
def test_continuous_generate_with_beam_sync_every_equals_generate_sync(golden_dir, tmp_path):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    z, cfg, sd = _g20(golden_dir)
    gdir = str(tmp_path / "gen")
    _save_generator_dir(gdir, cfg, sd)
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900, 33)]
    hf = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, continuous=True, continuous_slots=2, beam_sync_every=4)
    hf.initialize()
    plain = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0)
    plain.initialize()
    args = ("f.lean", "thm", Pos(1, 0), 8)

    async def main():
        return await asyncio.gather(*(hf.generate(s, *args) for s in states))

    got = asyncio.run(main())
    assert got == [plain.generate_sync(s, *args) for s in states]  # tactics, scores (exact floats), de-duplication order
    assert got == [hf.generate_sync(s, *args) for s in states]
    assert hf._driver is None and not hf._waiters and hf._stream.in_flight == 0 and hf._stream.queued == 0
    assert isinstance(hf._stream.pool, BeamBooksPool) and hf._stream.pool.sync_every == 4 and hf._stream.pool.n_slots == 2
