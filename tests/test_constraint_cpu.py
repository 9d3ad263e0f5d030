"""Constrained decoding, host side ("Constrained decoding"): the automata of
``reprover_amd.constraint`` against Python's own UTF-8 decoder, ``in`` and set membership; the constructor's refusals; the
host loops of ``generation`` with the host mask against HuggingFace's ``prefix_allowed_tokens_fn`` (fixture G30); many
states, the slot pools and the sampled loops against each state alone; a null automaton against the unconstrained loops;
the planted mutants; the tactic generators' ``valid_utf8`` / ``banned`` over a stub engine.  Nothing here needs a GPU."""
import asyncio
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from constraint_helpers import EOS, g30_automata, g30_model, load_g30, obeys, tokens_of  # noqa: E402
from gen_helpers import T5Fp32, source_ids  # noqa: E402
from sample_pool_helpers import CpuPoolSampler  # noqa: E402
from test_generate_pool_cpu import PoolRef  # noqa: E402
from test_generate_prefix_cpu import ManyRef  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.constraint import MAX_STATES, ByteAutomaton  # noqa: E402
from reprover_amd.generation import (CONSTRAINT_MUTANTS, BeamBooksPool, BeamSearchOutput, BeamSearchPool,  # noqa: E402
                                     SamplePool, beam_search, beam_search_batch, beam_search_batch_device,
                                     constraint_mask_host, constraint_mask_step_host, greedy_search, greedy_search_batch,
                                     sample_search, sample_search_batch)
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402

V = 384
UTF8 = ByteAutomaton.utf8(V)


# ---- utf8 against Python's decoder ---------------------------------------------------------------------------------------
def _strict(data: bytes) -> bool:
    try:
        data.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _char_prefixes():
    """Every proper prefix (1..3 bytes) of the encoding of a code point, from Python's encoder: one code point per
    block of 64 gives every prefix, because only the last byte varies inside a block."""
    out = set()
    for cp in itertools.chain(range(0x80, 0xD800, 64), range(0xE000, 0x110000, 64)):
        enc = chr(cp).encode("utf-8")
        out.update(enc[:k] for k in range(1, len(enc)))
    return out


CHAR_PREFIXES = _char_prefixes()


def _prefix_of_valid(data: bytes) -> bool:
    """Whether some continuation makes ``data`` valid: valid characters, then nothing or a proper prefix of one.
    (CPython's incremental decoder is no reference here: it holds ED A0 back until the third byte.)"""
    return any(_strict(data[: len(data) - k]) and (k == 0 or data[len(data) - k :] in CHAR_PREFIXES)
               for k in range(min(3, len(data)) + 1))


def _walk(aut: ByteAutomaton, strings: np.ndarray) -> np.ndarray:
    """The automaton's state after every row of ``strings`` (uint8 [N, L]), -1 where a prefix was rejected: vectorised."""
    state = np.zeros(len(strings), dtype=np.int64)
    for j in range(strings.shape[1]):
        to = aut.next[np.maximum(state, 0), strings[:, j].astype(np.int64) + 3].astype(np.int64)
        state = np.where(state >= 0, to, -1)
    return state


def _check_utf8(strings: np.ndarray) -> None:
    state = _walk(UTF8, strings)
    viable = state >= 0
    accepted = viable & (UTF8.next[np.maximum(state, 0), EOS] >= 0)
    rows = [bytes(r) for r in strings]
    want_ok = np.array([_strict(r) for r in rows])
    want_viable = np.array([_prefix_of_valid(r) for r in rows])
    bad = np.nonzero((accepted != want_ok) | (viable != want_viable))[0]
    assert len(bad) == 0, [(rows[i].hex(), bool(accepted[i]), bool(want_ok[i]), bool(viable[i]), bool(want_viable[i]))
                           for i in bad[:5]]


def test_utf8_shape_and_fixed_ids():
    assert UTF8.n_states <= 9 and UTF8.next.dtype == np.int16 and UTF8.next.shape == (UTF8.n_states, V)
    for s in range(UTF8.n_states):  # pad, unk and the sentinels never; EOS only between characters
        allowed = UTF8.allowed(s)
        assert not allowed[0] and not allowed[2] and not allowed[259:].any()
        assert bool(allowed[EOS]) == (s == 0)
    assert UTF8.state_after([]) == 0 and UTF8.accepts(0)


def test_utf8_all_strings_of_one_and_two_bytes():
    one = np.arange(256, dtype=np.uint8)[:, None]
    _check_utf8(one)
    _check_utf8(np.stack(np.meshgrid(one[:, 0], one[:, 0], indexing="ij"), -1).reshape(-1, 2))


@pytest.mark.parametrize("lead", range(0xE0, 0x100, 4))
def test_utf8_every_three_byte_string_from_e0_up(lead):
    b = np.arange(256, dtype=np.uint8)
    grid = np.stack(np.meshgrid(np.arange(lead, lead + 4, dtype=np.uint8), b, b, indexing="ij"), -1).reshape(-1, 3)
    _check_utf8(grid)


def test_utf8_four_byte_strings_at_the_lead_and_second_byte_boundaries():
    b = np.arange(256, dtype=np.uint8)
    edge = np.array([0x00, 0x7F, 0x80, 0xBF, 0xC0, 0xFF], dtype=np.uint8)
    pairs = [(lead, second) for lead in (0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xF7, 0xF8, 0xFF)
             for second in (0x7F, 0x80, 0x8F, 0x90, 0xBF, 0xC0)]
    rows = []
    for lead, second in pairs:
        for third, fourth in ((b, edge), (edge, b)):
            t, f = np.meshgrid(third, fourth, indexing="ij")
            rows.append(np.stack([np.full(t.size, lead, np.uint8), np.full(t.size, second, np.uint8), t.reshape(-1),
                                  f.reshape(-1)], -1))
    _check_utf8(np.concatenate(rows))


def _encodings(lo: int, hi: int, width: int) -> np.ndarray:
    """The UTF-8 encodings of the code points lo .. hi - 1 (all ``width`` bytes long, no surrogates among them) from
    Python's encoder, each as one integer."""
    raw = np.frombuffer("".join(map(chr, range(lo, hi))).encode("utf-8"), dtype=np.uint8).reshape(-1, width)
    return (raw.astype(np.int64) << (8 * np.arange(width - 1, -1, -1))).sum(1)


@pytest.mark.parametrize("lead", (0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xF7, 0xF8, 0xFF))
def test_utf8_every_four_byte_string_of_the_boundary_lead_and_second_byte_pairs(lead):
    """All 65536 strings of every (lead, second byte) pair at the boundaries.  The reference is vectorised and comes from
    Python's encoder: a string that starts with a byte >= EF is valid exactly when it is one 4-byte character, or one
    3-byte character and an ASCII byte; it is a prefix of a valid string when it is valid, or one 3-byte character and a
    lead byte (a 1-byte proper prefix of a character).  The per-string reference of the test above agrees with this one
    on its subset (checked here on a sample)."""
    valid4 = _encodings(0x10000, 0x110000, 4)
    valid3 = np.concatenate([_encodings(0x800, 0xD800, 3), _encodings(0xE000, 0x10000, 3)])
    leads = np.array(sorted(p[0] for p in CHAR_PREFIXES if len(p) == 1), dtype=np.int64)
    b = np.arange(256, dtype=np.uint8)
    for second in (0x7F, 0x80, 0x8F, 0x90, 0xBF, 0xC0):
        t, f = np.meshgrid(b, b, indexing="ij")
        strings = np.stack([np.full(t.size, lead, np.uint8), np.full(t.size, second, np.uint8), t.reshape(-1),
                            f.reshape(-1)], -1)
        s = strings.astype(np.int64)
        first3 = np.isin((s[:, 0] << 16) | (s[:, 1] << 8) | s[:, 2], valid3)
        want_ok = np.isin((s[:, 0] << 24) | (s[:, 1] << 16) | (s[:, 2] << 8) | s[:, 3], valid4) | (first3 & (s[:, 3] < 0x80))
        want_viable = want_ok | (first3 & np.isin(s[:, 3], leads))
        state = _walk(UTF8, strings)
        viable = state >= 0
        accepted = viable & (UTF8.next[np.maximum(state, 0), EOS] >= 0)
        assert np.array_equal(accepted, want_ok) and np.array_equal(viable, want_viable), (hex(lead), hex(second))
        for i in np.random.default_rng(lead + second).integers(0, len(strings), size=200):  # the two references agree
            assert _strict(bytes(strings[i])) == bool(want_ok[i]) and _prefix_of_valid(bytes(strings[i])) == bool(want_viable[i])


def test_utf8_code_point_boundaries_and_overlongs():
    def enc(cp):
        return chr(cp).encode("utf-8", "surrogatepass")

    for cp in (0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF):
        assert UTF8.accepts_row(tokens_of(enc(cp)) + [EOS]), hex(cp)
        assert all(UTF8.viable(tokens_of(enc(cp)[:k])) for k in range(5)), hex(cp)
    for raw in (enc(0xD800), enc(0xDFFF), bytes([0xF4, 0x90, 0x80, 0x80]),  # surrogates, U+110000
                bytes([0xC0, 0x80]), bytes([0xE0, 0x80, 0x80]), bytes([0xF0, 0x80, 0x80, 0x80]), bytes([0xC1, 0xBF])):
        assert not _strict(raw)
        assert not UTF8.viable(tokens_of(raw)), raw.hex()
    assert not UTF8.accepts_row(tokens_of("←".encode()[:2]) + [EOS])  # EOS inside a character
    assert UTF8.viable(tokens_of("←".encode()[:2])) and not UTF8.viable(tokens_of("←".encode()[:2]) + [EOS])
    with pytest.raises(ValueError):
        UTF8.state_after(tokens_of(b"a") + [300])
    with pytest.raises(ValueError):
        UTF8.state_after([0])


# ---- ban, trie, product ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patterns", [["ab"], ["abc", "bc"], ["aa", "aab", "ba"], ["abab", "bab", "c"], ["abcabc", "cab", "bca"]])
def test_ban_equals_python_in_on_a_three_letter_alphabet(patterns):
    aut = ByteAutomaton.ban(patterns, V)
    rng = np.random.default_rng(len(patterns) + len(patterns[0]))
    texts = ["".join(t) for k in range(1, 6) for t in itertools.product("abc", repeat=k)]
    texts += ["".join(rng.choice(list("abc"), size=int(rng.integers(6, 30)))) for _ in range(400)]
    for text in texts:
        clean = not any(p in text for p in patterns)
        assert aut.viable(tokens_of(text.encode())) == clean, (patterns, text)
        assert aut.accepts_row(tokens_of(text.encode()) + [EOS]) == clean
    assert not aut.allowed(0)[0] and not aut.allowed(0)[2] and not aut.allowed(0)[259:].any()


def test_product_is_the_conjunction():
    ban = ByteAutomaton.ban(["sorry", "←", "x∀"], V)
    both = UTF8 & ban
    assert both.n_states <= UTF8.n_states * ban.n_states
    rng = np.random.default_rng(5)
    pieces = ["sorry", "sor", "ry", "←", "∀", "x", " ", "ℕ", "∀", "a"]
    for _ in range(300):
        text = "".join(rng.choice(pieces, size=int(rng.integers(1, 8)))).encode()
        cut = text[: int(rng.integers(1, len(text) + 1))]  # may end inside a character
        toks = tokens_of(cut)
        assert both.viable(toks) == (UTF8.viable(toks) and ban.viable(toks)), cut
        assert both.accepts_row(toks + [EOS]) == (UTF8.accepts_row(toks + [EOS]) and ban.accepts_row(toks + [EOS])), cut
    with pytest.raises(ValueError):
        UTF8 & ByteAutomaton.utf8(300)


def test_trie_is_membership():
    words = ["simp", "simp only [h]", "rw [←h]", "exact h"]
    aut = ByteAutomaton.trie(words, V)
    for w in words + ["sim", "simp o", "rw", "exact h ", "x", "rw [←", "simp only [h]]"]:
        toks = tokens_of(w.encode())
        assert aut.viable(toks) == any(x.startswith(w) for x in words), w
        assert aut.accepts_row(toks + [EOS]) == (w in words), w
    cut = tokens_of("rw [←".encode()[:-1])
    assert aut.viable(cut) and not aut.accepts_row(cut + [EOS])


def test_constructor_refusals():
    ok = np.full((2, 8), -1, dtype=np.int16)
    ok[0, 3], ok[1, EOS] = 1, 1
    ByteAutomaton(ok)
    stuck = ok.copy()
    stuck[1, EOS] = -1  # state 1 is reachable and allows nothing
    with pytest.raises(ValueError, match="allows no token"):
        ByteAutomaton(stuck)
    loop = ok.copy()
    loop[1, EOS], loop[1, 4] = -1, 1  # state 1 goes round for ever
    with pytest.raises(ValueError, match="EOS cannot be reached"):
        ByteAutomaton(loop)
    unreachable = np.concatenate([ok, np.full((1, 8), -1, dtype=np.int16)])  # a dead state nobody reaches is no refusal
    ByteAutomaton(unreachable)
    big = np.zeros((MAX_STATES + 1, 8), dtype=np.int16)
    with pytest.raises(ValueError, match="states"):
        ByteAutomaton(big)
    ByteAutomaton(np.zeros((MAX_STATES, 8), dtype=np.int16))
    with pytest.raises(ValueError):
        ByteAutomaton(np.full((2, 8), 2, dtype=np.int16))  # an entry names no state
    with pytest.raises(ValueError):
        ByteAutomaton.ban([""], V)
    with pytest.raises(ValueError):
        ByteAutomaton.trie([], V)
    table = UTF8.device_table("cpu")
    assert table.dtype == torch.int16 and table.is_contiguous() and UTF8.device_table("cpu") is table


# ---- the host emulations of the two entry points ---------------------------------------------------------------------------
def test_mask_host_touches_only_forbidden_entries():
    rng = np.random.default_rng(0)
    lp = torch.from_numpy(rng.standard_normal((6, V)).astype(np.float32))
    lp[0, 5], lp[1, 70] = float("-inf"), -0.0
    q = torch.tensor([0, 1, 2, 7, 99, -4], dtype=torch.int32)  # the last two are clamped into the table
    out = constraint_mask_host(lp.clone(), q, UTF8)
    for r, s in enumerate([0, 1, 2, 7, 7, 0]):
        allowed = torch.from_numpy(UTF8.allowed(s))
        assert torch.equal(out[r][allowed].view(torch.int32), lp[r][allowed].view(torch.int32))
        assert bool(torch.isneginf(out[r][~allowed]).all())


def _step_scenario(mutant=None):
    """Slot 0 carries state 2 at position 4, slot 1 state 0 at position 0 (its rows start over); state 1 is not listed."""
    arrow = tokens_of("←".encode())
    q = torch.tensor([[3, 3], [5, 5], [1, 2]], dtype=torch.int32)
    tokens = torch.tensor([arrow[1], 0, 7, 7], dtype=torch.int32)  # continuation byte; pad (forbidden: stays); anything
    out = constraint_mask_step_host(torch.zeros((4, V)), [2, 0], [4, 0], tokens, q, UTF8, mutant=mutant)
    return q.tolist(), [[bool(x) for x in torch.isneginf(r)] for r in out]


def _step_scenario_expected():
    rows = [0, 2, 0, 0]
    return [[0, 0], [5, 5], [0, 2]], [[not bool(x) for x in UTF8.allowed(s)] for s in rows]


def test_mask_step_host_advances_resets_and_keeps():
    assert _step_scenario() == _step_scenario_expected()


# ---- the host loops against HuggingFace (G30) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g30():
    z, meta = load_g30()
    cfg, sd = g30_model(meta)
    ref = T5Fp32(cfg, sd)
    return z, meta, cfg, sd, ref, ref.encode(z["src"]), g30_automata(meta, cfg["vocab_size"])


def _replay(g30, ci, **kw):
    z, meta, cfg, sd, ref, enc, auts = g30
    c = meta["cases"][ci]
    prefix = [int(x) for x in z[f"c{ci}_prefix"]] or None
    ref.start(enc, c["num_beams"], c["max_length"])
    if c["num_beams"] == 1:
        return greedy_search(ref.step, c["max_length"], prompt=prefix, constraint=auts[c["automaton"]], **kw)
    return beam_search(ref.step, c["num_beams"], c["max_length"], c["length_penalty"], prompt=prefix,
                       constraint=auts[c["automaton"]], **kw)


def _case_ids():
    _, meta = load_g30()
    return list(range(len(meta["cases"])))


@pytest.mark.parametrize("ci", _case_ids())
def test_g30_replay_gives_hf_rows(g30, ci):
    z, meta, _, _, _, _, auts = g30
    c = meta["cases"][ci]
    trace = [] if c["num_beams"] > 1 else None
    out = _replay(g30, ci, **({} if trace is None else {"trace": trace}))
    assert np.array_equal(out.sequences.numpy(), z[f"c{ci}_seq"])
    aut = auts[c["automaton"]]
    assert all(obeys(aut, row) for row in out.sequences.numpy())
    if trace is not None:
        assert np.allclose(out.sequences_scores.numpy(), z[f"c{ci}_score"], rtol=1e-5, atol=1e-5)
        assert np.array_equal(np.stack([t[1].numpy() for t in trace]), z[f"c{ci}_trace_token"])
        assert np.array_equal(np.stack([t[2].numpy() for t in trace]), z[f"c{ci}_trace_parent"])
        assert all(bool(torch.isfinite(t[0]).all()) for t in trace)  # no dead -inf tie enters a comparison


def test_g30_fixture_says_what_it_should(g30):
    z, meta, _, _, _, _, auts = g30
    cases = meta["cases"]
    assert meta["n_grid_cases"] == 48 and len(cases) > 48
    grid = {(c["automaton"], c["num_beams"], c["length_penalty"], c["max_length"]) for c in cases[:48]}
    assert grid == {(a, nb, lp, ml) for a in auts for nb in (1, 2, 4, 8) for lp in (0.0, 1.0, -0.5) for ml in (6, 24)}
    arrow = "←".encode()
    for ci, c in enumerate(cases[48:], 48):  # the prompts end inside the 3-byte character
        prefix = bytes(int(t) - 3 for t in z[f"c{ci}_prefix"])
        assert prefix.endswith(arrow[:1]) or prefix.endswith(arrow[:2])
        assert not _strict(prefix) and _prefix_of_valid(prefix)
    assert sum(c["bf16_agrees"] for c in cases) >= 40 and sum(c["n_finished_on_eos"] for c in cases) >= 26


# ---- many states, the pools and the sampled loops: each state's own bits ---------------------------------------------------
@pytest.fixture(scope="module")
def many(g30):
    """Three sources (one with a prompt that ends inside a character) and every constrained search alone, computed once."""
    z, meta, cfg, sd, ref, enc0, auts = g30
    src = z["src"]
    encs = [enc0, ref.encode(np.concatenate([src[:40], [1]]).astype(np.int32)), ref.encode(source_ids(120, 11))]
    prompts = [None, tokens_of("rw [←".encode()[:6]), None]
    cache = {}

    def alone(nb, ml, lp, name):
        key = (nb, ml, lp, name)
        if key not in cache:
            outs = []
            for enc, p in zip(encs, prompts):
                ref.start(enc, nb, ml)
                trace = []
                outs.append((beam_search(ref.step, nb, ml, lp, trace=trace, prompt=p, constraint=auts[name]), trace))
            cache[key] = outs
        return cache[key]

    return cfg, sd, encs, prompts, alone, auts


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores, want.sequences_scores)  # the same bits, not a tolerance


def _differs(a, b):
    return not (a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences)
                and torch.equal(a.sequences_scores, b.sequences_scores))


@pytest.mark.parametrize("nb,lp,ml,name", [(4, 1.0, 24, "utf8"), (2, -0.5, 16, "utf8_ban")])
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_batch_gives_each_constrained_search_alone(many, nb, lp, ml, name, order):
    cfg, sd, encs, prompts, alone, auts = many
    want = alone(nb, ml, lp, name)
    eng = ManyRef(cfg, sd, [encs[i] for i in order], nb, ml)
    traces = []
    outs = beam_search_batch(eng.step_many, 3, nb, ml, lp, traces=traces, prompts=[prompts[i] for i in order],
                             constraint=auts[name])
    for j, i in enumerate(order):
        _same(outs[j], want[i][0])
        assert all(torch.equal(x, y) for t, u in zip(traces[j], want[i][1]) for x, y in zip(t, u))
        assert all(obeys(auts[name], row) for row in outs[j].sequences.numpy())


def test_greedy_batch_gives_each_constrained_search_alone(many, g30):
    cfg, sd, encs, prompts, _, auts = many
    ref, ml = g30[4], 24
    eng = ManyRef(cfg, sd, encs, 1, ml)
    outs = greedy_search_batch(eng.step_many, 3, ml, prompts=prompts, constraint=auts["utf8_ban"])
    for enc, p, out in zip(encs, prompts, outs):
        ref.start(enc, 1, ml)
        _same(out, greedy_search(ref.step, ml, prompt=p, constraint=auts["utf8_ban"]))
        assert obeys(auts["utf8_ban"], out.sequences[0].numpy())


def _run_beam_pool(many, nb, ml, lp, name, mutant=None):
    """Five tickets (the three sources, then sources 0 and 2 again) through 2 slots, a newcomer every two steps."""
    cfg, sd, encs, prompts, _, auts = many
    jobs = [0, 1, 2, 0, 2]
    eng = PoolRef(cfg, sd, 2, nb, ml)
    pool = BeamSearchPool(eng.admit, eng.step, 2, nb, ml, lp, constraint=auts[name], mutant=mutant)
    got = {}
    for i in jobs:
        pool.submit(encs[i], prompt=prompts[i]) if prompts[i] is not None else pool.submit(encs[i])
        for _ in range(2):
            got.update(pool.step())
    got.update(pool.drain())
    assert sorted(got) == list(range(len(jobs)))
    return got, jobs


@pytest.mark.parametrize("nb,lp,ml,name", [(4, 1.0, 24, "utf8"), (2, -0.5, 16, "utf8_ban")])
def test_pool_tickets_equal_their_constrained_search_alone(many, nb, lp, ml, name):
    want = many[4](nb, ml, lp, name)
    got, jobs = _run_beam_pool(many, nb, ml, lp, name)
    for ticket, i in enumerate(jobs):
        _same(got[ticket], want[i][0])


SAMPLE_KW = dict(temperature=1.2, top_k=50, top_p=0.95)
SAMPLE_SEEDS = [41, 0xFFFFFFF5, 43]


@pytest.fixture(scope="module")
def sampled_alone(hip_lib, many, g30):
    """``sample_search`` of every source alone under each automaton: once, left unchanged."""
    cfg, sd, encs, _, _, auts = many
    ref = g30[4]
    cache = {}

    def alone(nb, ml, name):
        if (nb, ml, name) not in cache:
            outs = []
            for enc, seed in zip(encs, SAMPLE_SEEDS):
                ref.start(enc, nb, ml)
                sampler = CpuPoolSampler(hip_lib, **SAMPLE_KW)
                outs.append(sample_search(lambda tok, anc, t: ref.step(tok.long(), anc[:, : t + 1].long()), sampler.at, nb,
                                          ml, seed, constraint=None if name is None else auts[name]))
            cache[(nb, ml, name)] = outs
        return cache[(nb, ml, name)]

    return alone


def _sampled_rows_obey(aut, out):
    assert bool(torch.isfinite(out.sequences_scores).all())  # no forbidden token was drawn: its log-prob is the model's
    for row in out.sequences.numpy():
        toks = [int(t) for t in row[1:]]
        toks = toks[: toks.index(EOS) + 1] if EOS in toks else toks
        assert aut.accepts_row(toks) if toks[-1] == EOS else aut.viable(toks), toks


@pytest.mark.parametrize("name", ["utf8", "utf8_ban"])
@pytest.mark.parametrize("k", [1, 4])
def test_sampled_batch_gives_each_state_alone(hip_lib, many, sampled_alone, name, k):
    cfg, sd, encs, _, _, auts = many
    nb, ml = 4, 14
    want = sampled_alone(nb, ml, name)
    free = sampled_alone(nb, ml, None)
    assert any(_differs(a, b) for a, b in zip(want, free))  # the constraint changes what is drawn
    order = [2, 0, 1]
    eng = ManyRef(cfg, sd, [encs[i] for i in order], nb, ml)
    sampler = CpuPoolSampler(hip_lib, **SAMPLE_KW)
    outs = sample_search_batch(lambda active, tok, anc, t: eng.step_many(active, tok.long(), anc[:, : t + 1].long()),
                               sampler.at, 3, nb, ml, [SAMPLE_SEEDS[i] for i in order], sync_every=k,
                               constraint=auts[name])
    for j, i in enumerate(order):
        _same(outs[j], want[i])
        _sampled_rows_obey(auts[name], outs[j])


def _run_sample_pool(hip_lib, many, nb, ml, k, name, mutant=None):
    cfg, sd, encs, _, _, auts = many
    jobs = [0, 1, 2, 1, 0]
    eng = PoolRef(cfg, sd, 2, nb, ml)
    sampler = CpuPoolSampler(hip_lib, **SAMPLE_KW)
    pool = SamplePool(eng.admit, lambda active, pos, tok, anc: eng.step(active, pos, tok.long(), anc[:, : max(pos) + 1].long()),
                      sampler, 2, nb, ml, sync_every=k, constraint=auts[name], mutant=mutant)
    got = {}
    for i in jobs:
        pool.submit(encs[i], SAMPLE_SEEDS[i])
        got.update(pool.step())
    got.update(pool.drain())
    assert sorted(got) == list(range(len(jobs)))
    return got, jobs


@pytest.mark.parametrize("k", [1, 3])
def test_sample_pool_tickets_equal_their_state_alone(hip_lib, many, sampled_alone, k):
    nb, ml, name = 4, 14, "utf8"
    want = sampled_alone(nb, ml, name)
    got, jobs = _run_sample_pool(hip_lib, many, nb, ml, k, name)
    for ticket, i in enumerate(jobs):
        _same(got[ticket], want[i])
        _sampled_rows_obey(many[5][name], got[ticket])


# ---- the null automaton is the unconstrained loop ----------------------------------------------------------------------------
def test_null_automaton_gives_the_unconstrained_outputs(hip_lib, many, g30, sampled_alone):
    cfg, sd, encs, prompts, _, _ = many
    ref = g30[4]
    null = ByteAutomaton.null(cfg["vocab_size"])
    assert null.n_states == 1 and null.allowed(0).all()
    for constraint in (None, null):
        outs = []
        ref.start(encs[0], 4, 16)
        trace = []
        outs.append((beam_search(ref.step, 4, 16, 1.0, trace=trace, **({} if constraint is None else {"constraint": null})),
                     trace))
        ref.start(encs[1], 1, 16)
        outs.append((greedy_search(ref.step, 16, prompt=prompts[1], **({} if constraint is None else {"constraint": null})),
                     []))
        if constraint is None:
            base = outs
    for (a, ta), (b, tb) in zip(base, outs):
        _same(a, b)
        assert len(ta) == len(tb) and all(torch.equal(x, y) for t, u in zip(ta, tb) for x, y in zip(t, u))
    free = sampled_alone(4, 14, None)
    ref.start(encs[0], 4, 14)
    sampler = CpuPoolSampler(hip_lib, **SAMPLE_KW)
    _same(sample_search(lambda tok, anc, t: ref.step(tok.long(), anc[:, : t + 1].long()), sampler.at, 4, 14,
                        SAMPLE_SEEDS[0], constraint=null), free[0])


# ---- the planted mutants -------------------------------------------------------------------------------------------------------
def test_every_mutant_is_noticed(hip_lib, many, g30, sampled_alone):
    z, meta = g30[0], g30[1]
    assert set(CONSTRAINT_MUTANTS) == {"state_by_row", "admit_not_reset", "mask_wrong_row", "eos_anywhere"}
    beam_cases = [ci for ci, c in enumerate(meta["cases"]) if c["num_beams"] >= 4 and c["max_length"] >= 14]
    for mutant in ("state_by_row", "mask_wrong_row"):  # the host-books loop against HF's rows
        missed = [ci for ci in beam_cases
                  if not np.array_equal(_replay(g30, ci, mutant=mutant).sequences.numpy(), z[f"c{ci}_seq"])]
        assert missed, f"{mutant} changed no row of {beam_cases}: the fixture would not notice it"
    # EOS inside a character never wins a beam on these weights, so HF's rows do not notice "eos_anywhere" in the beam
    # loop: the mask's own check (test_mask_host_touches_only_forbidden_entries) does, and the sampled pool below
    inside = constraint_mask_host(torch.zeros((1, V)), torch.tensor([2], dtype=torch.int32), UTF8, mutant="eos_anywhere")
    assert not bool(torch.isneginf(inside[0][torch.from_numpy(~UTF8.allowed(2))]).all())
    nb, ml, name = 4, 14, "utf8"
    want = sampled_alone(nb, ml, name)
    for mutant in CONSTRAINT_MUTANTS:  # the fused form's own scenario
        assert _step_scenario(mutant) != _step_scenario_expected(), mutant
    # ... and in the pool (with both slots in use a launch row is its (state, sample) entry: "state_by_row" passes there)
    for mutant in ("admit_not_reset", "mask_wrong_row", "eos_anywhere"):
        got, jobs = _run_sample_pool(hip_lib, many, nb, ml, 3, name, mutant=mutant)
        assert any(_differs(got[t], want[i]) for t, i in enumerate(jobs)), mutant
    # not reset at admission: the slots' second tenants start where the first ones stood
    got, jobs = _run_sample_pool(hip_lib, many, nb, ml, 3, name, mutant="admit_not_reset")
    assert not any(_differs(got[t], want[i]) for t, i in list(enumerate(jobs))[:2])
    assert any(_differs(got[t], want[i]) for t, i in list(enumerate(jobs))[2:])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_value_errors(g30):
    nothing = lambda *a, **k: None  # noqa: E731
    step = lambda t, a: torch.zeros(len(t), V)  # noqa: E731
    bad = tokens_of(bytes([0xC0, 0x80]))
    with pytest.raises(ValueError, match="forbids"):
        beam_search(step, 4, 12, prompt=bad, constraint=UTF8)
    with pytest.raises(ValueError, match="forbids"):
        greedy_search(step, 12, prompt=bad, constraint=UTF8)
    pool = BeamSearchPool(nothing, nothing, 2, 4, 12, constraint=UTF8)
    with pytest.raises(ValueError, match="forbids"):
        pool.submit("src", prompt=bad)
    assert pool.queued == 0 and pool.submit("src", prompt=tokens_of("←".encode()[:2])) == 0
    with pytest.raises(ValueError, match="not built yet"):
        beam_search_batch_device(nothing, nothing, nothing, 1, 4, 8, constraint=UTF8)
    with pytest.raises(ValueError, match="not built yet"):
        BeamBooksPool(nothing, nothing, 2, 4, 8, constraint=UTF8)
    with pytest.raises(ValueError):
        beam_search(step, 4, 12, mask=nothing)  # a mask without a constraint
    with pytest.raises(ValueError):
        beam_search(lambda t, a: torch.zeros(len(t), 300), 4, 12, constraint=UTF8)  # another vocabulary


# ---- the product classes over a stub engine ------------------------------------------------------------------------------------
def _stub_output(nb):
    rows = [[0, 3 + ord("a"), 3 + ord("0") + r, 1] for r in range(nb)]
    return BeamSearchOutput(torch.tensor(rows, dtype=torch.int64), torch.tensor([-0.25 * r for r in range(nb)]))


class StubStream:
    def __init__(self, engine, nb):
        self.engine, self.nb, self.waiting, self.tickets = engine, nb, [], 0

    queued = property(lambda self: len(self.waiting))
    in_flight = property(lambda self: 0)

    def submit(self, ids, *a, **kw):
        self.tickets += 1
        self.waiting.append(self.tickets)
        return self.tickets

    def step(self):
        done, self.waiting = [(t, _stub_output(self.nb)) for t in self.waiting], []
        return done


class StubEngine:
    cfg = {"vocab_size": V}

    def __init__(self):
        self.decoder = SimpleNamespace(max_states=lambda nb: 2)
        self.calls = []

    def _note(self, name, kw):
        self.calls.append((name, kw.get("constraint")))

    def generate(self, ids, nb, max_len, lp, **kw):
        self._note("generate", kw)
        return _stub_output(nb)

    def generate_many(self, sources, nb, max_len, lp, **kw):
        self._note("generate_many", kw)
        return [_stub_output(nb) for _ in sources]

    def sample_many(self, sources, nb, max_len, *a, **kw):
        self._note("sample_many", kw)
        return [_stub_output(nb) for _ in sources]

    def generate_stream(self, nb, max_len, lp, **kw):
        self._note("generate_stream", kw)
        return StubStream(self, nb)

    def sample_stream(self, nb, max_len, *a, **kw):
        self._note("sample_stream", kw)
        return StubStream(self, nb)


def stub_generator(**kw):
    gen = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, **kw)
    gen.generator, gen.tokenizer = StubEngine(), ByT5Tokenizer()
    return gen


ARGS = ("f.lean", "thm", Pos(1, 0))
STATE = "h : x = y ⊢ y = x"
LISTS = ([ARGS[0]] * 3, [ARGS[1]] * 3, [ARGS[2]] * 3)


@pytest.mark.parametrize("opts", [dict(valid_utf8=True), dict(banned=["sorry"]), dict(valid_utf8=True, banned=["sorry", "admit"])])
def test_options_reach_every_call_form(opts):
    def constraints(gen):
        seen = [c for _, c in gen.generator.calls]
        assert seen and all(c is seen[0] and isinstance(c, ByteAutomaton) for c in seen), gen.generator.calls
        return seen[0], [name for name, _ in gen.generator.calls]

    gen = stub_generator(**opts)
    gen.generate_sync(STATE, *ARGS, 4)
    gen.generate_sync(STATE, *ARGS, 4, prefix="rw [")
    gen.batch_generate_sync([STATE] * 3, *LISTS, 4)
    gen.batch_generate_sync([STATE] * 3, *LISTS, 4, prefixes=["rw [", None, None])
    aut, names = constraints(gen)
    assert names == ["generate"] * 2 + ["generate_many"] * 4
    sorry, broken = tokens_of(b"sorry"), tokens_of("←".encode()[:1]) + [EOS]
    assert aut.viable(sorry) == ("banned" not in opts)
    assert aut.accepts_row(broken) == ("valid_utf8" not in opts)
    assert aut.accepts_row(tokens_of("rw [←h]".encode()) + [EOS])
    for kw, want in ((dict(continuous=True), "generate_stream"), (dict(do_sample=True), "sample_many"),
                     (dict(do_sample=True, sample_stream=True), "sample_stream"),
                     (dict(do_sample=True, sample_stream=True, per_request_sampling=True), "sample_stream")):
        gen = stub_generator(**opts, **kw)
        asyncio.run(gen.generate(STATE, *ARGS, 4))
        if "continuous" in kw:
            asyncio.run(gen.generate(STATE, *ARGS, 4, prefix="rw ["))
        assert constraints(gen)[1][0] == want
    rag = RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, **opts)
    rag.hf_gen.generator, rag.hf_gen.tokenizer = StubEngine(), ByT5Tokenizer()
    rag.retriever = SimpleNamespace(retrieve=lambda state, *a: ([], []))
    rag.generate_sync(STATE, *ARGS, 4)
    rag.batch_generate_sync([STATE] * 3, *LISTS, 4)
    assert constraints(rag.hf_gen)[1] == ["generate", "generate_many", "generate_many"]


def test_defaults_keep_the_engine_calls_and_sync_every_is_refused():
    gen = stub_generator()
    gen.generate_sync(STATE, *ARGS, 4)
    gen.batch_generate_sync([STATE] * 3, *LISTS, 4)
    assert all(c is None for _, c in gen.generator.calls) and gen._constraint() == {}
    for opts in (dict(valid_utf8=True), dict(banned=["sorry"])):
        with pytest.raises(ValueError, match="not built yet"):
            stub_generator(beam_sync_every=4, **opts)
        with pytest.raises(ValueError, match="not built yet"):
            RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, beam_sync_every=4, **opts)
    with pytest.raises(ValueError):
        stub_generator(banned="sorry")
    with pytest.raises(ValueError):
        stub_generator(banned=[""])
