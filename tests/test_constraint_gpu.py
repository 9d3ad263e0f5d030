"""Constrained decoding on the MI355X ("Constrained decoding"): rp_constraint_mask against numpy bit
for bit with guards round every buffer; rp_constraint_mask_step against its host emulation over a two-slot pool; the
ABI's refusals; HipT5Generator's constrained searches against the same engine step followed by a torch mask and the
same selection or sampler, against HuggingFace (G30), alone, batched and streamed; a narrow trie."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from constraint_helpers import EOS, g30_automata, g30_model, load_g30, obeys, tokens_of  # noqa: E402
from reprover_amd import _lib  # noqa: E402
from reprover_amd.constraint import ByteAutomaton  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402
from reprover_amd.generation import (beam_search, beam_search_batch, constraint_mask_step_host,  # noqa: E402
                                     greedy_search, sample_search_batch)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RP_E_INVALID = -1
GUARD = 64  # words before and after every buffer
NEG_INF_BITS = np.uint32(0xFF800000)


def _pc(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _guarded(payload: np.ndarray, fill: int):
    """``payload`` (any 2- or 4-byte dtype) on the device between two guards of 64 four-byte words: (whole, view)."""
    raw = payload.reshape(-1).view(np.uint8)
    pad = (-len(raw)) % 4
    host = np.concatenate([np.full(GUARD * 4, fill, np.uint8), raw, np.full(pad + GUARD * 4, fill, np.uint8)])
    whole = torch.from_numpy(host).to(DEV)
    return whole, whole[GUARD * 4 : GUARD * 4 + len(raw)]


def _guards_intact(whole: torch.Tensor, nbytes: int, fill: int) -> bool:
    host = whole.cpu().numpy()
    return bool((host[: GUARD * 4] == fill).all() and (host[GUARD * 4 + nbytes :] == fill).all())


def _random_table(rng, n_q: int, vocab: int) -> np.ndarray:
    """int16 [n_q, vocab]: about a third forbidden, -1 and other negative values, targets anywhere in [0, n_q)."""
    nxt = rng.integers(0, n_q, size=(n_q, vocab)).astype(np.int16)
    kind = rng.random((n_q, vocab))
    nxt[kind < 0.3] = -1
    nxt[kind < 0.05] = -32768
    return nxt


def _random_bits(rng, rows: int, vocab: int) -> np.ndarray:
    """uint32 [rows, vocab] float bit patterns: random words (NaNs of every payload among them), -0.0, denormals, -inf."""
    bits = rng.integers(0, 2 ** 32, size=(rows, vocab), dtype=np.uint64).astype(np.uint32)
    kind = rng.random((rows, vocab))
    bits[kind < 0.05] = 0x80000000
    bits[(kind >= 0.05) & (kind < 0.10)] &= np.uint32(0x807FFFFF)  # denormals of both signs
    bits[(kind >= 0.10) & (kind < 0.15)] = NEG_INF_BITS
    return bits


# ---- rp_constraint_mask alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 2, 4096])
@pytest.mark.parametrize("rows", [1, 2, 255, 257, 1024])
@pytest.mark.parametrize("vocab", [1, 5, 300, 384, 512])
def test_mask_against_numpy(hip_lib, vocab, rows, n_q):
    rng = np.random.default_rng(vocab * 7 + rows * 3 + n_q)
    table = _random_table(rng, n_q, vocab)
    bits = _random_bits(rng, rows, vocab)
    q = rng.integers(0, n_q, size=rows).astype(np.int32)
    lp_all, lp = _guarded(bits, 0xA5)
    q_all, qd = _guarded(q, 0x3C)
    t_all, td = _guarded(table, 0x7E)
    st = hip_lib.rp_constraint_mask(lp.data_ptr(), vocab, rows, qd.data_ptr(), td.data_ptr(), n_q, _lib.current_stream())
    assert st == 0, hip_lib.rp_last_error()
    torch.cuda.synchronize()
    got = lp.cpu().numpy().view(np.uint32).reshape(rows, vocab)
    want = np.where(table[q] < 0, NEG_INF_BITS, bits)
    assert np.array_equal(got, want)  # every forbidden entry -inf, every other entry the same bits
    assert _guards_intact(lp_all, bits.nbytes, 0xA5) and _guards_intact(q_all, q.nbytes, 0x3C)
    assert _guards_intact(t_all, table.nbytes, 0x7E)
    assert np.array_equal(qd.cpu().numpy().view(np.int32), q) and np.array_equal(td.cpu().numpy().view(np.int16).reshape(n_q, vocab), table)


def test_mask_clamps_states_it_cannot_check(hip_lib):
    rng = np.random.default_rng(1)
    vocab, rows, n_q = 301, 9, 5
    table, bits = _random_table(rng, n_q, vocab), _random_bits(rng, rows, vocab)
    q = _i32([0, 4, 5, -1, 2 ** 31 - 1, -2 ** 31, 70000, 3, 1])
    lp_all, lp = _guarded(bits, 0xA5)
    t_all, td = _guarded(table, 0x7E)
    qd = torch.from_numpy(q).to(DEV)
    assert hip_lib.rp_constraint_mask(lp.data_ptr(), vocab, rows, qd.data_ptr(), td.data_ptr(), n_q, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    want = np.where(table[np.clip(q, 0, n_q - 1)] < 0, NEG_INF_BITS, bits)
    assert np.array_equal(lp.cpu().numpy().view(np.uint32).reshape(rows, vocab), want)
    assert _guards_intact(lp_all, bits.nbytes, 0xA5) and _guards_intact(t_all, table.nbytes, 0x7E)


# ---- rp_constraint_mask_step alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,nb", [(384, 4), (259, 3)])
def test_mask_step_against_the_host_emulation(hip_lib, vocab, nb):
    """Eight positions of a two-slot pool inside books of three states: the slots at different positions, slot 1
    re-admitted mid-run (its position back to 0), finished rows fed pad, and out-of-range values planted in q and the
    tokens.  q and the masked rows equal the emulation at every position; the unlisted state's q is never touched."""
    rng = np.random.default_rng(vocab + nb)
    aut = ByteAutomaton.utf8(vocab) & ByteAutomaton.ban(["ab", "←"], vocab)
    table = torch.from_numpy(aut.next).to(DEV)
    n, n_q = 3, aut.n_states
    q_dev = torch.tensor(rng.integers(0, n_q, size=(n, nb)), dtype=torch.int32, device=DEV)
    q_host = q_dev.cpu().clone()
    active, pos = [2, 0], [3, 0]
    for stepno in range(8):
        if stepno == 4:
            pos[0] = 0  # state 2's next tenant
        if stepno == 6:
            active, pos = [0], [pos[1]]  # state 2 left: one listed state, at launch row 0
        rows = len(active) * nb
        tokens = np.array([int(rng.choice(np.nonzero(aut.allowed(0))[0])) for _ in range(rows)], dtype=np.int32)
        tokens[rng.random(rows) < 0.3] = 0  # pad: a finished row
        if stepno == 2:  # values the ABI cannot check
            tokens[0], tokens[-1] = -7, 10 ** 6
            q_dev[2, 0], q_dev[0, nb - 1] = 9999, -3
            q_host[2, 0], q_host[0, nb - 1] = 9999, -3
        bits = _random_bits(rng, rows, vocab)
        lp_all, lp = _guarded(bits, 0xA5)
        lp = lp.view(torch.float32).view(rows, vocab)
        tok_dev = torch.from_numpy(tokens).to(DEV)
        st = hip_lib.rp_constraint_mask_step(lp.data_ptr(), vocab, _pc(_i32(active)), _pc(_i32(pos)), len(active), n, nb,
                                             tok_dev.data_ptr(), q_dev.data_ptr(), table.data_ptr(), n_q,
                                             _lib.current_stream())
        assert st == 0, hip_lib.rp_last_error()
        torch.cuda.synchronize()
        want = constraint_mask_step_host(torch.from_numpy(bits.view(np.float32).copy()), active, pos,
                                         torch.from_numpy(tokens), q_host, aut)
        assert torch.equal(q_dev.cpu(), q_host), stepno
        assert np.array_equal(lp.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32)), stepno
        assert _guards_intact(lp_all, bits.nbytes, 0xA5)
        pos = [p + 1 for p in pos]
    assert torch.equal(q_dev[1].cpu(), q_host[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(hip_lib, status, text):
    assert status == RP_E_INVALID
    assert text in hip_lib.rp_last_error().decode(), hip_lib.rp_last_error()


def test_refusals(hip_lib):
    lp = torch.zeros((8, 384), dtype=torch.float32, device=DEV)
    before = lp.clone()
    q = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    tok = torch.zeros(8, dtype=torch.int32, device=DEV)
    table = torch.zeros((2, 384), dtype=torch.int16, device=DEV)
    s = _lib.current_stream()

    def mask(lp_=lp.data_ptr(), vocab=384, rows=8, q_=q.data_ptr(), t=table.data_ptr(), n_q=2):
        return hip_lib.rp_constraint_mask(lp_, vocab, rows, q_, t, n_q, s)

    def step(lp_=lp.data_ptr(), vocab=384, active=(0, 1), pos=(0, 3), n=4, nb=2, tok_=tok.data_ptr(), q_=q.data_ptr(),
             t=table.data_ptr(), n_q=2, n_active=None, null_active=False, null_pos=False):
        a, p = _i32(active), _i32(pos)
        return hip_lib.rp_constraint_mask_step(lp_, vocab, None if null_active else _pc(a), None if null_pos else _pc(p),
                                               len(a) if n_active is None else n_active, n, nb, tok_, q_, t, n_q, s)

    assert mask() == 0 and step() == 0 and mask(vocab=1) == 0 and mask(vocab=512, rows=6) == 0 and mask(rows=1) == 0
    assert mask(n_q=1) == 0 and step(n_q=1) == 0 and step(nb=1) == 0 and step(n=2) == 0
    for kw in (dict(lp_=None), dict(q_=None), dict(t=None)):
        _refused(hip_lib, mask(**kw), "null argument")
    for kw in (dict(lp_=None), dict(q_=None), dict(t=None), dict(tok_=None), dict(null_active=True), dict(null_pos=True)):
        _refused(hip_lib, step(**kw), "null argument")
    for call in (mask, step):
        _refused(hip_lib, call(vocab=0), "vocab=0 (1..512)")
        _refused(hip_lib, call(vocab=513), "vocab=513 (1..512)")
        _refused(hip_lib, call(n_q=0), "n_q=0 (1..4096)")
        _refused(hip_lib, call(n_q=4097), "n_q=4097 (1..4096)")
    _refused(hip_lib, mask(rows=0), "rows=0 (1..1024)")
    _refused(hip_lib, mask(rows=1025), "rows=1025 (1..1024)")
    _refused(hip_lib, step(nb=0), "nb=0 (1..64)")
    _refused(hip_lib, step(nb=65), "nb=65 (1..64)")
    _refused(hip_lib, step(n=0), "states=0 (1..32)")
    _refused(hip_lib, step(n=33), "states=33 (1..32)")
    _refused(hip_lib, step(n_active=0), "active states=0")
    _refused(hip_lib, step(active=(0, 1, 2), pos=(0, 0, 0), n=2), "active states=3")
    _refused(hip_lib, step(active=tuple(range(17)), pos=(0,) * 17, n=32, nb=64), "> 1024")
    _refused(hip_lib, step(active=(1, 1)), "names a state twice")
    _refused(hip_lib, step(active=(0, 4)), "outside [0, states=4)")
    _refused(hip_lib, step(active=(0, -1)), "outside [0, states=4)")
    _refused(hip_lib, step(pos=(0, -1)), "pos[1]=-1")
    for call in (mask, step):  # a pointer that is not aligned to its element type (the vector accesses start from it)
        _refused(hip_lib, call(lp_=lp.data_ptr() + 2), "is not aligned to its type")
        _refused(hip_lib, call(t=table.data_ptr() + 1), "is not aligned to its type")
    torch.cuda.synchronize()
    assert torch.equal(lp, before)  # an all-allowed table and refused calls: nothing was written
    assert hip_lib.rp_abi_version() == 7


# ---- end to end on the G20 weights ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup():
    z, meta = load_g30()
    cfg, sd = g30_model(meta)
    return z, meta, cfg, HipT5Generator(cfg, sd, DEV), g30_automata(meta, cfg["vocab_size"])


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits, not a tolerance


def _torch_mask(aut):
    """The host-side reference of the launch: ``torch.where`` over the engine's own log-probs."""
    def mask(lp, q_rows):
        forbidden = aut.device_table(lp.device)[q_rows.long()] < 0
        return torch.where(forbidden, torch.full_like(lp, float("-inf")), lp)
    return mask


@pytest.mark.parametrize("name", ["utf8", "utf8_ban"])
def test_searches_equal_the_engine_step_with_a_torch_mask(name):
    z, meta, cfg, gen, auts = _setup()
    aut, dec, src, ml = auts[name], _setup()[3].decoder, z["src"], 24
    cut = np.concatenate([src[:40], [1]]).astype(np.int32)
    prefix = tokens_of("rw [←".encode()[:6])
    # greedy
    got = gen.greedy(src, ml, constraint=aut)
    dec.start(gen.encode_hidden(src), 1, ml)
    _same(got, greedy_search(dec.step, ml, device=DEV, constraint=aut, mask=_torch_mask(aut)))
    assert obeys(aut, got.sequences[0].numpy())
    # beams, with the per-step triples
    trace, want_trace = [], []
    got = gen.generate(src, 4, ml, 1.0, trace=trace, constraint=aut)
    dec.start(gen.encode_hidden(src), 4, ml)
    want = beam_search(dec.step, 4, ml, 1.0, select=dec.select, device=DEV, trace=want_trace, constraint=aut,
                       mask=_torch_mask(aut))
    _same(got, want)
    assert all(torch.equal(x, y) for t, u in zip(trace, want_trace) for x, y in zip(t, u))
    # three states, one with a prefix that ends inside a character: each equals its search alone and the torch mask's
    sources, prefixes = [src, cut, src[:120]], [None, prefix, None]
    many = gen.generate_many(sources, 4, ml, 1.0, prefixes=prefixes, constraint=aut)
    gen._start_many(sources, 4, ml)
    want = beam_search_batch(dec.step_many, 3, 4, ml, 1.0, select_many=dec.select_many, device=DEV, prompts=prefixes,
                             prefill_many=dec.prefill_many, constraint=aut, mask=_torch_mask(aut))
    for i, (a, b) in enumerate(zip(many, want)):
        _same(a, b)
        _same(a, gen.generate(sources[i], 4, ml, 1.0, prefix=prefixes[i], constraint=aut))
        assert all(obeys(aut, row) for row in a.sequences.numpy())
    assert many[1].sequences[:, 1:7].tolist() == [prefix] * 4
    # the stream: 2 slots, a newcomer between steps
    stream = gen.generate_stream(4, ml, 1.0, n_slots=2, src_cap=512, constraint=aut)
    got, tickets = {}, []
    for s, p in zip(sources, prefixes):
        tickets.append(stream.submit(s, prefix=p))
        got.update(stream.step())
    got.update(stream.drain())
    for t, b in zip(tickets, many):
        _same(got[t], b)


# Flagged cases left out of the sequence comparison: in each the engine's candidates first leave the fp32 driver's at two
# candidates whose fp32 scores lie closer than HF-bf16's own rms log-prob error on this model (G19, 0.15), so bf16
# arithmetic may order them either way; test_g30_cases_return_hf_sequences asserts exactly that for every listed case.
# The figures: the fp32 gap of the two candidates, measured on the MI355X.
_TAIL = "2 beams, max_length 24: at step 14 the last of the 4 kept candidates is token 71, not 239 (fp32 gap 2.2e-2)"
G30_NEAR_TIES = {
    7: _TAIL, 9: _TAIL, 11: _TAIL, 31: _TAIL, 33: _TAIL, 35: _TAIL,  # one search: utf8 / utf8 & ban, three penalties
    50: "prefix cut after E2 86, 2 beams: at step 4 the two best candidates, tokens 223 and 213, swap (fp32 gap 3.6e-2)",
    51: "prefix cut after E2 86, 4 beams: at step 3 the last of the 8 kept candidates is (beam 1, token 137), not "
        "(beam 3, token 18) (fp32 gap 8.7e-2)",
}


@functools.lru_cache(maxsize=None)
def _hf_bf16_rms_error() -> float:
    """HF-bf16's own rms log-prob error against HF-fp32 on the tiny model (fixture G19; the smaller of its two sources):
    what "near-tied" is measured with.  The engine's contract is to err no more (test_decode_step_no_worse_than_hf_bf16)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_decoder_step.npz"))
    return min(float(np.sqrt(((g[f"{k}_lp16"] - g[f"{k}_lp32"]) ** 2).mean())) for k in ("tiny_0", "tiny_1"))


def _first_departure_gap(ci, engine_trace):
    """(step, fp32 gap) where the engine's selected (parent, token) pairs first leave the fp32 driver's: the largest
    difference between the fp32 scores of the candidates that are picked by one side only or stand at another rank.  The
    fp32 scores of all ``nb * vocab`` candidates of that step come from a replay of the fp32 driver on the host."""
    from gen_helpers import T5Fp32
    from reprover_amd.generation import topk_select

    z, meta, cfg, gen, auts = _setup()
    c = meta["cases"][ci]
    zt, zp = z[f"c{ci}_trace_token"], z[f"c{ci}_trace_parent"]
    step = next(t for t, (_, tok, par) in enumerate(engine_trace)
                if not (np.array_equal(tok.numpy(), zt[t]) and np.array_equal(par.numpy(), zp[t])))
    rows = []

    def select(lp, running, k):
        rows.append((lp + running[:, None]).reshape(-1).clone())
        return topk_select(lp, running, k)

    ref = T5Fp32(cfg, g30_model(meta)[1])
    ref.start(ref.encode(z["src"]), c["num_beams"], c["max_length"])
    replay = []
    beam_search(ref.step, c["num_beams"], c["max_length"], c["length_penalty"], select=select, trace=replay,
                prompt=[int(x) for x in z[f"c{ci}_prefix"]] or None, constraint=auts[c["automaton"]])
    assert np.array_equal(np.stack([t[1].numpy() for t in replay]), zt)  # the replay is the fixture's driver
    V = cfg["vocab_size"]
    mine = [int(p) * V + int(k) for p, k in zip(engine_trace[step][2], engine_trace[step][1])]
    theirs = [int(p) * V + int(k) for p, k in zip(zp[step], zt[step])]
    moved = [a for a, b in zip(mine, theirs) if a != b] + [b for a, b in zip(mine, theirs) if a != b]
    scores = rows[step][moved]
    assert bool(torch.isfinite(scores).all())
    return step, float(scores.max() - scores.min())


def test_g30_cases_return_hf_sequences():
    """Every ``bf16_agrees`` case of G30 returns HF's sequences, but for the cases of ``G30_NEAR_TIES``: those must leave
    the fp32 driver at candidates that lie within HF-bf16's own rms log-prob error of each other, and nowhere earlier."""
    z, meta, cfg, gen, auts = _setup()
    bound = _hf_bf16_rms_error()
    print(f"near-tie bound (HF-bf16 rms log-prob error, G19 tiny): {bound:.4f}")
    assert 0.05 < bound < 0.5  # (the fixture's figure is 0.152)
    flagged = [ci for ci, c in enumerate(meta["cases"]) if c["bf16_agrees"]]
    assert set(G30_NEAR_TIES) <= set(flagged) and len(flagged) - len(G30_NEAR_TIES) >= 32
    for ci in flagged:
        c = meta["cases"][ci]
        aut = auts[c["automaton"]]
        prefix = [int(x) for x in z[f"c{ci}_prefix"]] or None
        trace = []
        if c["num_beams"] == 1:
            out = gen.greedy(z["src"], c["max_length"], prefix=prefix, constraint=aut)
        else:
            out = gen.generate(z["src"], c["num_beams"], c["max_length"], c["length_penalty"], prefix=prefix, constraint=aut,
                               trace=trace)
        assert all(obeys(aut, row) for row in out.sequences.numpy()), ci
        if ci not in G30_NEAR_TIES:
            assert np.array_equal(out.sequences.cpu().numpy(), z[f"c{ci}_seq"]), ci
            continue
        step, gap = _first_departure_gap(ci, trace)
        print(f"case {ci}: leaves the fp32 driver at step {step}, fp32 gap {gap:.3e} ({G30_NEAR_TIES[ci]})")
        assert gap <= bound, (ci, step, gap, bound)


def test_null_automaton_gives_the_unconstrained_bits():
    z, meta, cfg, gen, auts = _setup()
    null, src = ByteAutomaton.null(cfg["vocab_size"]), z["src"]
    _same(gen.greedy(src, 16, constraint=null), gen.greedy(src, 16))
    _same(gen.generate(src, 4, 16, 1.0, constraint=null), gen.generate(src, 4, 16, 1.0))
    _same(gen.sample(src, 4, 16, 1.1, 40, 0.9, seed=5, constraint=null), gen.sample(src, 4, 16, 1.1, 40, 0.9, seed=5))
    with pytest.raises(ValueError, match="not built yet"):
        gen.generate(src, 4, 16, 1.0, sync_every=4, constraint=null)
    with pytest.raises(ValueError, match="not built yet"):
        gen.generate_stream(4, 16, sync_every=4, constraint=null)
    from reprover_amd.decoder import GenerateStream
    with pytest.raises(ValueError, match="not built yet"):  # the stream's own constructor refuses it too
        GenerateStream(gen, 4, 16, 1.0, 2, 512, sync_every=4, constraint=null)
    with pytest.raises(ValueError):
        gen.generate(src, 4, 16, constraint=ByteAutomaton.null(300))
    with pytest.raises(ValueError, match="forbids"):
        gen.generate(src, 4, 16, prefix=tokens_of(bytes([0xC0, 0x80])), constraint=auts["utf8"])


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def _sampled_rows_obey(aut, out):
    assert bool(torch.isfinite(out.sequences_scores).all())  # a forbidden token's masked log-prob would be -inf
    for row in out.sequences.cpu().numpy():
        toks = [int(t) for t in row[1:]]
        toks = toks[: toks.index(EOS) + 1] if EOS in toks else toks
        assert aut.accepts_row(toks) if toks[-1] == EOS else aut.viable(toks), toks


def test_sampling_alone_batched_streamed_and_against_the_host_mask():
    z, meta, cfg, gen, auts = _setup()
    aut, dec, src, ml, nb = auts["utf8"], _setup()[3].decoder, z["src"], 20, 8
    kw = dict(temperature=1.2, top_k=50, top_p=0.95)
    sources = [src, np.concatenate([src[:40], [1]]).astype(np.int32), src[:120]]
    seeds = [41, 0xFFFFFFF5, 43]
    alone = [gen.sample(s, nb, ml, seed=sd_, constraint=aut, **kw) for s, sd_ in zip(sources, seeds)]
    free = [gen.sample(s, nb, ml, seed=sd_, **kw) for s, sd_ in zip(sources, seeds)]
    assert any(not torch.equal(a.sequences, f.sequences) for a, f in zip(alone, free))
    for out in alone:
        _sampled_rows_obey(aut, out)
    for k in (1, 16):
        for a, b in zip(gen.sample_many(sources, nb, ml, seeds=seeds, sync_every=k, constraint=aut, **kw), alone):
            _same(a, b)
    # the same engine step and sampler with the emulation's torch mask in place of the launch
    gen._start_many(sources, nb, ml)
    want = sample_search_batch(
        lambda active, tokens, ancestry, t: dec.step_many(active, tokens, ancestry, t=t),
        lambda lp, active, t, state: dec.sample_step(lp, active, t, state, kw["temperature"], kw["top_k"], kw["top_p"], 1, 0),
        3, nb, ml, seeds, device=DEV, constraint=aut,
        mask=lambda lp, active, pos, tok, q: constraint_mask_step_host(lp, active, pos, tok, q, aut))
    for a, b in zip(want, alone):
        _same(a, b)
    # streamed through 2 slots, and per-request parameters
    stream = gen.sample_stream(nb, ml, n_slots=2, src_cap=512, sync_every=3, constraint=aut, **kw)
    got, tickets = {}, []
    for s, sd_ in zip(sources + sources[:1], seeds + seeds[:1]):
        tickets.append(stream.submit(s, sd_))
        got.update(stream.step())
    got.update(stream.drain())
    for t, b in zip(tickets, alone + alone[:1]):
        _same(got[t], b)
    from reprover_amd.generation import SamplingParams
    params = SamplingParams(temperature=[0.7, 1.0, 1.5, 1.2] * 2, top_k=[0, 5, 50, 1] * 2, top_p=0.9)
    per = gen.sample(src, nb, ml, seed=7, params=params, constraint=aut)
    _sampled_rows_obey(aut, per)
    stream = gen.sample_stream(nb, ml, n_slots=2, src_cap=512, per_request=True, constraint=aut, **kw)
    t0 = stream.submit(src, 7, params=params)
    _same(dict(stream.drain())[t0], per)


def test_sampled_rows_equal_the_reference_sampler_on_the_masked_log_probs(hip_lib):
    """Step by step along the engine's own path: the tokens ``rp_sample_step`` draws from the masked log-probs equal
    tests/sample_helpers.py's float64 sampler on those log-probs with ``rp_sample_uniform``'s numbers, wherever that
    file's margin rule lets a row be compared; no forbidden entry keeps any mass."""
    from sample_helpers import margin_bound, reference_sample, uniforms

    z, meta, cfg, gen, auts = _setup()
    aut, dec, ml, nb = auts["utf8_ban"], _setup()[3].decoder, 20, 8
    T, k, p = 1.2, 50, 0.95
    sources, seeds = [z["src"], z["src"][:120]], [41, 0xFFFFFFF5]
    V = cfg["vocab_size"]
    seen = dict(compared=0, skipped=0)
    table = aut.device_table(DEV)

    def sample_step(lp, active, t, state):
        host = lp.cpu().numpy()
        was_finished = state.finished.cpu().numpy().copy()
        q = states["q"].cpu().numpy()
        u = np.concatenate([uniforms(hip_lib, [int(state.seeds[i])] * nb, range(nb), t) for i in active])
        want, kept, margins, _ = reference_sample(host, u, T, k, p)
        dec.sample_step(lp, active, t, state, T, k, p, 1, 0)
        got = state.tokens[: len(active) * nb].cpu().numpy()
        for a, i in enumerate(active):
            for b in range(nb):
                r = a * nb + b
                forbidden = (table[int(q[i, b])] < 0).cpu().numpy()
                assert np.isneginf(host[r][forbidden]).all() and not kept[r][forbidden].any()
                if was_finished[i, b]:
                    assert got[r] == 0
                elif margins[r] > margin_bound(V):
                    seen["compared"] += 1
                    assert int(got[r]) == int(want[r]) and not forbidden[int(got[r])], (i, b, t)
                else:
                    seen["skipped"] += 1

    states = {}

    def mask(lp, active, pos, tokens, q):
        states["q"] = q
        return dec.constraint_mask_step(lp, active, pos, tokens, q, aut)

    gen._start_many(sources, nb, ml)
    outs = sample_search_batch(lambda active, tokens, ancestry, t: dec.step_many(active, tokens, ancestry, t=t), sample_step,
                               2, nb, ml, seeds, device=DEV, constraint=aut, mask=mask)
    print("rows compared / left out by the margin rule:", seen)
    assert seen["compared"] > 100 and seen["skipped"] <= 0.1 * (seen["compared"] + seen["skipped"])
    for out, want in zip(outs, gen.sample_many(sources, nb, ml, T, k, p, seeds=seeds, constraint=aut)):
        _same(out, want)
        _sampled_rows_obey(aut, out)


# ---- a narrow automaton ------------------------------------------------------------------------------------------------------------
def test_a_trie_of_three_strings_at_four_beams_runs_to_the_end():
    z, meta, cfg, gen, auts = _setup()
    words = ["simp", "rw [←h]", "exact h"]
    aut = ByteAutomaton.trie(words, cfg["vocab_size"])
    out = gen.generate(z["src"], 4, 16, 1.0, constraint=aut)
    scores = out.sequences_scores.cpu()
    assert not bool(torch.isnan(scores).any())
    finite = [bytes(t - 3 for t in row[1:].tolist() if t >= 3).decode() for row, s in zip(out.sequences.cpu(), scores)
              if float(s) > -1.0e9 / 16]  # an unfilled row keeps -1e9 / its length <= -1e9 / 15; -inf: a dead beam
    assert sorted(finite) == sorted(words)
