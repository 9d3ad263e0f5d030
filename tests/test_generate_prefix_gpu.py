"""Tactic-prefix beam search on the MI355X: the one-pass prompt prefill (rp_decoder_batch_prefill /
rp_decoder_pool_prefill) against the same rows written by ordinary decode steps, byte for byte; rp_decoder_batch_step_pos
against rp_decoder_batch_step; the prefixed searches of HipT5Generator against the same searches prefilled by steps, alone,
batched and streamed; against HuggingFace (G27); the ABI's refusals; workspace hygiene."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hip_helpers import Arena, guard_bytes, hygiene_findings  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, HipT5Generator  # noqa: E402
from reprover_amd.generation import beam_search, greedy_search  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A  # what a workspace holds before the first call
RP_E_INVALID, RP_E_WORKSPACE = -1, -3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pc(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _stream():
    return _lib.current_stream()


def _cfg(name):
    if name == "byt5-width":  # ByT5-small's widths (6 heads, d_model 1472, d_ff 3584), two decoder layers
        return dict(synth.seq2seq_config("byt5-small"), num_decoder_layers=2)
    return synth.seq2seq_config(name)


@functools.lru_cache(maxsize=None)
def _decoder(name):
    cfg = _cfg(name)
    return cfg, HipT5Decoder(cfg, synth.synth_seq2seq_state_dict(cfg, scale="sharp"), DEV)


def _enc_rows(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return _t(rng.standard_normal((n, cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16)


def _align(x):
    return (x + 255) // 256 * 256


def _cache_view(cfg, ws, total_src, n, nb, max_len):
    """The cache part of a workspace (include/reprover_hip.h: cross K/V, then the cache) as int16
    [n, L, max_len, nb, 2 * inner], and its byte range."""
    L, inner = cfg["num_decoder_layers"], cfg["num_heads"] * cfg["d_kv"]
    lo = _align(total_src * L * 2 * inner * 2)
    nbytes = n * L * max_len * nb * 2 * inner * 2
    return ws[lo : lo + nbytes].view(torch.int16).view(n, L, max_len, nb, 2 * inner), lo, lo + _align(nbytes)


def _identity(nb, t):
    return (np.arange(t + 1)[None] * nb + np.arange(nb)[:, None]).astype(np.int32)


def _beam0(nb, t):
    """The ancestry of a prompted search's first step at position ``t``: prompt rows p * nb, then the beams' own."""
    anc = np.tile((np.arange(t + 1) * nb).astype(np.int32), (nb, 1))
    anc[:, t] = t * nb + np.arange(nb)
    return anc


class Batch:
    """Raw calls on one exactly-sized batch workspace."""

    def __init__(self, name, n, nb, src, max_len, seed=3):
        self.cfg, self.dec = _decoder(name)
        self.lib, self.n, self.nb, self.max_len, self.V = self.dec._lib, n, nb, max_len, self.cfg["vocab_size"]
        self.src_cu = _i32(np.concatenate([[0], np.cumsum(src)]))
        self.enc = _enc_rows(self.cfg, int(self.src_cu[-1]), seed)
        self.bytes = int(self.lib.rp_decoder_batch_workspace_bytes(self.dec._handle, _pc(self.src_cu), n, nb, max_len))
        assert self.bytes > 0

    def fresh(self):
        ws = torch.full((self.bytes,), FILL, dtype=torch.uint8, device=DEV)
        st = self.lib.rp_decoder_batch_cross_kv(self.dec._handle, self.enc.data_ptr(), _pc(self.src_cu), self.n, self.nb,
                                                self.max_len, ws.data_ptr(), self.bytes, _stream())
        assert st == 0, _lib.load().rp_last_error()
        return ws

    def step(self, ws, active, tokens, anc, t):
        act, tok, a = _i32(active), _t(_i32(tokens)), _t(_i32(anc))
        lp = torch.full((len(act) * self.nb, self.V), float("nan"), dtype=torch.float32, device=DEV)
        st = self.lib.rp_decoder_batch_step(self.dec._handle, _pc(self.src_cu), self.n, _pc(act), len(act), tok.data_ptr(),
                                            a.data_ptr(), a.shape[1], self.nb, t, self.max_len, lp.data_ptr(), ws.data_ptr(),
                                            self.bytes, _stream())
        assert st == 0, self.lib.rp_last_error()
        return lp

    def step_pos(self, ws, active, tokens, anc, pos, nbytes=None, lp=None):
        act, tok, a, p = _i32(active), _t(_i32(tokens)), _t(_i32(anc)), _i32(pos)
        if lp is None:
            lp = torch.full((len(act) * self.nb, self.V), float("nan"), dtype=torch.float32, device=DEV)
        st = self.lib.rp_decoder_batch_step_pos(self.dec._handle, _pc(self.src_cu), self.n, _pc(act), len(act),
                                                tok.data_ptr(), a.data_ptr(), a.shape[1], self.nb, _pc(p), self.max_len,
                                                lp.data_ptr(), ws.data_ptr(), self.bytes if nbytes is None else nbytes,
                                                _stream())
        return st, lp

    def prefill(self, ws, states, rows, nbytes=None, anc_len=None, prompt_cu=None, n=None, nb=None, max_len=None,
                m=None, null=None):
        st_, rows = _i32(states), [_i32(r) for r in rows]
        pcu = _i32(np.concatenate([[0], np.cumsum([len(r) for r in rows])])) if prompt_cu is None else _i32(prompt_cu)
        tok = _t(np.concatenate(rows))
        longest = max(len(r) for r in rows)
        anc = _t((np.arange(longest) * self.nb).astype(np.int32))
        args = dict(states=_pc(st_), prompt_cu=_pc(pcu), tokens=tok.data_ptr(), anc=anc.data_ptr(), ws=ws.data_ptr())
        if null:
            args[null] = None
        return self.lib.rp_decoder_batch_prefill(
            self.dec._handle, _pc(self.src_cu), self.n if n is None else n, args["states"], args["prompt_cu"],
            len(st_) if m is None else m, args["tokens"], args["anc"], longest if anc_len is None else anc_len,
            self.nb if nb is None else nb, self.max_len if max_len is None else max_len, args["ws"],
            self.bytes if nbytes is None else nbytes, _stream())


def _prompts(rng, lens):
    return [np.concatenate([[0], rng.integers(3, 259, size=R - 1)]).astype(np.int32) for R in lens]


PREFILL_SHAPES = (
    [("tiny", 1, 1, (R,), None) for R in (1, 2, 257)]            # one row per pass; the 256-key pass and the bias clamp
    + [("tiny", 1, 3, (R,), None) for R in (2, 3, 4)]            # pass capacity 3: below, at, above
    + [("tiny", 2, 3, (7, 2), None), ("tiny", 2, 3, (7, 2), (1,)), ("tiny-tied", 2, 3, (7, 2), None)]
    + [("tiny", 1, 64, (R,), None) for R in (63, 64, 65, 130)]   # the pass edges at 64 rows
    + [("tiny-tied", 1, 3, (4,), None), ("byt5-width", 1, 8, (9,), None)]
)


@pytest.mark.parametrize("name,n,nb,lens,subset", PREFILL_SHAPES,
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batch_prefill_equals_steps_byte_for_byte(name, n, nb, lens, subset):
    rng = np.random.default_rng(sum(lens) + nb)
    listed = list(range(n)) if subset is None else list(subset)
    max_len = max(lens) + 3
    b = Batch(name, n, nb, (5, 130)[:n] if n == 2 else (37,), max_len)
    rows = _prompts(rng, lens)
    A, B = b.fresh(), b.fresh()
    assert torch.equal(A, B)
    # A: the prompt tokens through ordinary steps, repeated over the beams, identity ancestry
    for t in range(max(lens[j] for j in listed)):
        act = [j for j in listed if lens[j] > t]
        b.step(A, act, np.concatenate([np.full(nb, rows[j][t]) for j in act]), np.tile(_identity(nb, t), (len(act), 1)), t)
    # B: one prefill call
    st = b.prefill(B, listed, [rows[j] for j in listed])
    assert st == 0, b.lib.rp_last_error()
    torch.cuda.synchronize()
    total = int(b.src_cu[-1])
    cA, lo, hi = _cache_view(b.cfg, A, total, n, nb, max_len)
    cB, _, _ = _cache_view(b.cfg, B, total, n, nb, max_len)
    assert torch.equal(A[:lo], B[:lo])  # the cross K/V: untouched
    written = torch.zeros(cB.shape[:4], dtype=torch.bool, device=DEV)
    for j in listed:
        written[j, :, : lens[j], 0] = True
        assert torch.equal(cA[j, :, : lens[j], 0], cB[j, :, : lens[j], 0]), f"state {j}: prompt rows differ"
    fill16 = torch.tensor(FILL * 257, dtype=torch.int16, device=DEV)
    assert bool((cB[~written] == fill16).all()), "the prefill wrote a cache row other than p * nb"
    assert bool((cB[written] != fill16).any())
    # one further step at t = R_j with beam-0 ancestry: the same log-prob bits from both
    for j in listed:
        tok = rng.integers(0, 259, nb)
        lpA = b.step(A, [j], tok, _beam0(nb, lens[j]), lens[j])
        lpB = b.step(B, [j], tok, _beam0(nb, lens[j]), lens[j])
        assert torch.isfinite(lpA).all() and torch.equal(lpA.view(torch.int32), lpB.view(torch.int32))


class Pool:
    def __init__(self, name, n_slots, nb, max_len, src_cap):
        self.cfg, self.dec = _decoder(name)
        self.lib, self.shape, self.nb, self.V = self.dec._lib, (n_slots, nb, max_len, src_cap), nb, self.cfg["vocab_size"]
        self.bytes = int(self.lib.rp_decoder_pool_workspace_bytes(self.dec._handle, *self.shape))
        assert self.bytes > 0

    def admit(self, ws, slot, enc):
        cu = _i32([0, enc.shape[0]])
        st = self.lib.rp_decoder_pool_admit(self.dec._handle, *self.shape, _pc(_i32([slot])), enc.data_ptr(), _pc(cu), 1,
                                            ws.data_ptr(), self.bytes, _stream())
        assert st == 0, self.lib.rp_last_error()

    def step(self, ws, active, pos, src_len, tokens, anc):
        act, p, sl, tok, a = _i32(active), _i32(pos), _i32(src_len), _t(_i32(tokens)), _t(_i32(anc))
        lp = torch.full((len(act) * self.nb, self.V), float("nan"), dtype=torch.float32, device=DEV)
        st = self.lib.rp_decoder_pool_step(self.dec._handle, *self.shape, _pc(act), _pc(p), _pc(sl), len(act),
                                           tok.data_ptr(), a.data_ptr(), a.shape[1], lp.data_ptr(), ws.data_ptr(),
                                           self.bytes, _stream())
        assert st == 0, self.lib.rp_last_error()
        return lp

    def prefill(self, ws, slots, src_len, rows, nbytes=None, anc_len=None, shape=None, null=None, prompt_cu=None):
        sl, ln, rows = _i32(slots), _i32(src_len), [_i32(r) for r in rows]
        pcu = _i32(np.concatenate([[0], np.cumsum([len(r) for r in rows])])) if prompt_cu is None else _i32(prompt_cu)
        tok = _t(np.concatenate(rows))
        longest = max(len(r) for r in rows)
        anc = _t((np.arange(longest) * self.nb).astype(np.int32))
        args = dict(slots=_pc(sl), src_len=_pc(ln), prompt_cu=_pc(pcu), tokens=tok.data_ptr(), anc=anc.data_ptr(),
                    ws=ws.data_ptr())
        if null:
            args[null] = None
        return self.lib.rp_decoder_pool_prefill(self.dec._handle, *(self.shape if shape is None else shape), args["slots"],
                                                args["src_len"], args["prompt_cu"], len(sl), args["tokens"], args["anc"],
                                                longest if anc_len is None else anc_len, args["ws"],
                                                self.bytes if nbytes is None else nbytes, _stream())


@pytest.mark.parametrize("name,nb,R", [("tiny", 3, 7), ("tiny", 3, 12), ("tiny-tied", 3, 7), ("tiny", 1, 5)])
def test_pool_prefill_into_a_slot_beside_a_running_search(name, nb, R):
    """Slot 1 of 3 is prefilled while slot 0 stands mid-search at position 5: slot 1's rows are the steps', nothing else
    of the cache changes, and slot 0's next step gives the bits it gives without the admission."""
    rng = np.random.default_rng(R)
    max_len, src_cap = R + 3 if R > 5 else 9, 40
    pl = Pool(name, 3, nb, max_len, src_cap)
    enc0, enc1 = _enc_rows(pl.cfg, 33, 5), _enc_rows(pl.cfg, 17, 6)
    ws = torch.full((pl.bytes,), FILL, dtype=torch.uint8, device=DEV)
    pl.admit(ws, 0, enc0)
    for t in range(5):
        pl.step(ws, [0], [t], [33], rng.integers(0, 259, nb), _identity(nb, t))
    tok5 = rng.integers(0, 259, nb)
    alone = ws.clone()
    lp_alone = pl.step(alone, [0], [5], [33], tok5, _identity(nb, 5))  # slot 0's next step with no admission
    rows = _prompts(rng, (R,))[0]
    A, B = ws.clone(), ws.clone()
    pl.admit(A, 1, enc1)
    for p in range(R):
        pl.step(A, [1], [p], [17], np.full(nb, rows[p]), _identity(nb, p))
    pl.admit(B, 1, enc1)
    before = B.clone()
    st = pl.prefill(B, [1], [17], [rows])
    assert st == 0, pl.lib.rp_last_error()
    torch.cuda.synchronize()
    cA, lo, hi = _cache_view(pl.cfg, A, 3 * src_cap, 3, nb, max_len)
    cB, _, _ = _cache_view(pl.cfg, B, 3 * src_cap, 3, nb, max_len)
    c0, _, _ = _cache_view(pl.cfg, before, 3 * src_cap, 3, nb, max_len)
    assert torch.equal(B[:lo], before[:lo])
    written = torch.zeros(cB.shape[:4], dtype=torch.bool, device=DEV)
    written[1, :, :R, 0] = True
    assert torch.equal(cA[1, :, :R, 0], cB[1, :, :R, 0])
    assert torch.equal(cB[~written], c0[~written]), "the prefill wrote a cache row other than slot 1's p * nb"
    lp0 = pl.step(B, [0], [5], [33], tok5, _identity(nb, 5))
    assert torch.equal(lp0.view(torch.int32), lp_alone.view(torch.int32))
    tok = rng.integers(0, 259, nb)
    lpA = pl.step(A, [1], [R], [17], tok, _beam0(nb, R))
    lpB = pl.step(B, [1], [R], [17], tok, _beam0(nb, R))
    assert torch.isfinite(lpA).all() and torch.equal(lpA.view(torch.int32), lpB.view(torch.int32))


# ---- rp_decoder_batch_step_pos ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_step_pos_with_equal_positions_is_batch_step(name):
    rng = np.random.default_rng(1)
    n, nb = 2, 3
    b = Batch(name, n, nb, (5, 130), 8)
    X, Y = b.fresh(), b.fresh()
    for t in range(4):
        tok = rng.integers(0, 259, n * nb)
        anc = np.tile(_identity(nb, t), (n, 1))
        anc[:, :t] = (anc[:, :t] // nb) * nb + (anc[:, :t] % nb + 1) % nb  # the neighbouring beam's history
        lpX = b.step(X, [1, 0], tok, anc, t)
        st, lpY = b.step_pos(Y, [1, 0], tok, anc, [t, t])
        assert st == 0, b.lib.rp_last_error()
        assert torch.equal(lpX.view(torch.int32), lpY.view(torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(X, Y)  # the whole workspace, cache and scratch


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_step_pos_with_unequal_positions_is_each_state_alone(name):
    rng = np.random.default_rng(2)
    n, nb, pos = 2, 3, (2, 5)
    b = Batch(name, n, nb, (5, 130), 8)
    toks = rng.integers(0, 259, (n, 6, nb))
    X, Y = b.fresh(), b.fresh()
    alone = []
    for s in range(n):
        for t in range(pos[s] + 1):
            lp = b.step(X, [s], toks[s, t], _identity(nb, t), t)
        alone.append(lp)
        for t in range(pos[s]):
            b.step(Y, [s], toks[s, t], _identity(nb, t), t)
    anc = np.zeros((n * nb, max(pos) + 1), np.int32)
    for s in range(n):
        anc[s * nb : (s + 1) * nb, : pos[s] + 1] = _identity(nb, pos[s])
    st, lp = b.step_pos(Y, [0, 1], np.concatenate([toks[s, pos[s]] for s in range(n)]), anc, pos)
    assert st == 0, b.lib.rp_last_error()
    for s in range(n):
        assert torch.equal(lp[s * nb : (s + 1) * nb].view(torch.int32), alone[s].view(torch.int32))
    st, lp_rev = b.step_pos(Y, [1, 0], np.concatenate([toks[s, pos[s]] for s in (1, 0)]),
                            np.concatenate([anc[nb:], anc[:nb]]), pos[::-1])
    assert st == 0 and torch.equal(lp_rev[:nb].view(torch.int32), alone[1].view(torch.int32))
    assert torch.equal(lp_rev[nb:].view(torch.int32), alone[0].view(torch.int32))


# ---- the searches ---------------------------------------------------------------------------------------------------------
def _g27(golden_dir):
    z = np.load(os.path.join(golden_dir, "g27_generate_prefix.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def _weights(name, meta):
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg)
    if "lm_head.weight" in sd:
        sd["lm_head.weight"] = sd["lm_head.weight"].clone()
        sd["lm_head.weight"][1] *= meta["eos_boost"]
    return cfg, sd


@pytest.fixture(scope="module")
def gens(golden_dir):
    z, meta = _g27(golden_dir)
    made = {}

    def get(name):
        if name not in made:
            cfg, sd = _weights(name, meta)
            made[name] = HipT5Generator(cfg, sd, DEV)
        return made[name]

    return z, meta, get


def _sources(z):
    from gen_helpers import source_ids

    src = z["src"]
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    return [np.asarray(src, dtype=np.int32), cut(40), source_ids(120, 11), cut(7)]


def _by_steps(gen, ids, nb, ml, lp, prefix, trace=None):
    """The prefixed search over existing entry points only: the prompt rows through ``rp_decoder_batch_step``."""
    enc = gen.encode_hidden(ids)
    gen.decoder.start(enc, nb, ml)
    return beam_search(gen.decoder.step, nb, ml, lp, select=gen.decoder.select, device=gen.device, trace=trace,
                       prompt=prefix)


def _same(out, want):
    assert torch.equal(out.sequences, want.sequences)
    assert torch.equal(out.sequences_scores.view(torch.int32), want.sequences_scores.view(torch.int32))


def _same_trace(a, b):
    assert len(a) == len(b) and all(torch.equal(x, y) for t, u in zip(a, b) for x, y in zip(t, u))


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
@pytest.mark.parametrize("nb,lp,ml,P", [(4, 1.0, 24, 5), (8, -0.5, 40, 17), (2, 0.0, 8, 1), (64, 1.0, 24, 5)])
def test_generate_with_prefix_equals_the_search_prefilled_by_steps(gens, name, nb, lp, ml, P):
    z, meta, get = gens
    gen = get(name)
    prefix = z["c80_prefix"][:P]
    t0, t1 = [], []
    out = gen.generate(z["src"], nb, ml, lp, trace=t0, prefix=prefix)
    want = _by_steps(gen, z["src"], nb, ml, lp, prefix, trace=t1)
    _same(out, want)
    _same_trace(t0, t1)
    assert out.sequences[:, : P + 1].tolist() == [[0] + prefix.tolist()] * nb and out.sequences.shape[1] <= ml
    # no prefix: the call as it was
    _same(gen.generate(z["src"], nb, ml, lp, prefix=[]), gen.generate(z["src"], nb, ml, lp))


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2)])
def test_generate_many_with_prefixes_equals_generate_alone(gens, name, order):
    z, meta, get = gens
    gen = get(name)
    nb, lp, ml = 4, 1.0, 24
    srcs, long_prefix = _sources(z), z["c80_prefix"]
    prefixes = [None, long_prefix[:1], long_prefix[:5], long_prefix]
    traces = []
    outs = gen.generate_many([srcs[i] for i in order], nb, ml, lp, traces=traces, prefixes=[prefixes[i] for i in order])
    for j, i in enumerate(order):
        t = []
        _same(outs[j], gen.generate(srcs[i], nb, ml, lp, trace=t, prefix=prefixes[i]))
        _same_trace(traces[j], t)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_stream_tickets_with_prefixes_equal_generate_alone(gens, name):
    z, meta, get = gens
    gen = get(name)
    nb, lp, ml = 4, 1.0, 24
    srcs, long_prefix = _sources(z), z["c80_prefix"]
    jobs = [(0, None), (1, long_prefix[:1]), (2, long_prefix[:5]), (3, long_prefix), (1, long_prefix), (3, long_prefix[:1])]
    want = [gen.generate(srcs[i], nb, ml, lp, prefix=p) for i, p in jobs]
    stream = gen.generate_stream(nb, ml, lp, n_slots=2, src_cap=512)
    got = {}
    for i, p in jobs:
        stream.submit(srcs[i], prefix=p)
        for _ in range(2):
            got.update(stream.step())
    got.update(stream.drain())
    assert sorted(got) == list(range(len(jobs)))
    for ticket, w in enumerate(want):
        _same(got[ticket], w)
    with pytest.raises(ValueError, match="not built yet"):
        gen.generate_stream(nb, ml, lp, n_slots=2, src_cap=512, sync_every=4).submit(srcs[0], prefix=long_prefix[:1])
    with pytest.raises(ValueError, match="not built yet"):
        gen.sample_stream(nb, ml, n_slots=2, src_cap=512).submit(srcs[0], 0, prefix=long_prefix[:1])
    with pytest.raises(ValueError, match="not built yet"):
        gen.generate_many(srcs[:1], nb, ml, lp, sync_every=4, prefixes=[long_prefix[:1]])
    with pytest.raises(ValueError):
        gen.generate(srcs[0], nb, 6, lp, prefix=long_prefix[:5])


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_greedy_with_prefix(gens, name):
    z, meta, get = gens
    gen = get(name)
    ml = 24
    srcs, long_prefix = _sources(z), z["c80_prefix"]
    prefixes = [None, long_prefix[:1], long_prefix[:5], long_prefix]
    alone = []
    for s, p in zip(srcs, prefixes):
        out = gen.greedy(s, ml, prefix=p)
        enc = gen.encode_hidden(s)
        gen.decoder.start(enc, 1, ml)
        _same(out, greedy_search(gen.decoder.step, ml, device=gen.device, prompt=p))  # prefilled by steps
        P = 0 if p is None else len(p)
        assert out.sequences[0, : P + 1].tolist() == [0] + ([] if p is None else p.tolist())
        alone.append(out)
    for order in ((0, 1, 2, 3), (2, 3, 1, 0)):
        outs = gen.greedy_many([srcs[i] for i in order], ml, prefixes=[prefixes[i] for i in order])
        for j, i in enumerate(order):
            _same(outs[j], alone[i])


# ---- against HuggingFace (G27) ----------------------------------------------------------------------------------------------
# Flagged cases left out of the sequence comparison: each only because the by-steps path (existing entry points only)
# returns the same differing sequences (asserted below) - the engine's bf16 arithmetic, not the prefill.
_NEAR_TIE = ("P=5, 8 beams, max_length=7 (one generated token): the 6th and 7th candidates of the first step, tokens 257 "
             "and 212, lie closer than the engine's bf16 error and come out in the other order; the by-steps path "
             "returns the same rows")
G27_LEFT_OUT: dict = {45: _NEAR_TIE + ", length_penalty 0.0", 48: _NEAR_TIE + ", length_penalty 1.0",
                      51: _NEAR_TIE + ", length_penalty -0.5"}


def _teacher_forced(gen, enc, target):
    T = len(target)
    gen.decoder.start(enc, 1, T)
    out = []
    for t in range(T):
        anc = torch.arange(t + 1, dtype=torch.int64)[None]
        out.append(gen.decoder.step(torch.tensor([int(target[t])]), anc).clone())
    return torch.cat(out).cpu()


def _strip(seq, P):
    seq = list(seq)
    if 1 in seq[P + 1 :]:
        seq = seq[: seq.index(1, P + 1) + 1]
    return seq


@pytest.mark.parametrize("case", range(81))
def test_generate_with_prefix_matches_g27_and_own_scores(gens, case):
    z, meta, get = gens
    gen = get("tiny")
    c = meta["cases"][case]
    nb, lp_, ml, P, prefix = c["num_beams"], c["length_penalty"], c["max_length"], c["prefix_len"], z[f"c{case}_prefix"]
    out = gen.generate(z["src"], nb, ml, lp_, prefix=prefix)
    if c["bf16_agrees"]:
        if case in G27_LEFT_OUT:
            assert np.array_equal(_by_steps(gen, z["src"], nb, ml, lp_, prefix).sequences.numpy(), out.sequences.numpy())
        else:
            assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
    enc = gen.encode_hidden(z["src"])
    for j in range(nb):
        seq = _strip(out.sequences[j].tolist(), P)
        tf = _teacher_forced(gen, enc, np.array(seq[:-1]))
        n_gen = len(seq) - 1 - P
        total = float(sum(tf[i, seq[i + 1]] for i in range(P, len(seq) - 1)))  # the generated tokens only
        expect = total / (n_gen ** lp_)
        assert abs(expect - float(out.sequences_scores[j])) <= 1e-4 * max(1.0, abs(expect)), (j, expect, out.sequences_scores[j])


def test_g27_compared_cases(golden_dir):
    _, meta = _g27(golden_dir)
    flagged = [i for i, c in enumerate(meta["cases"][:81]) if c["bf16_agrees"]]
    assert set(G27_LEFT_OUT) <= set(flagged) and len(flagged) - len(G27_LEFT_OUT) >= 24
    for case in G27_LEFT_OUT:
        c = meta["cases"][case]
        assert (c["prefix_len"], c["num_beams"], c["max_length"]) == (5, 8, 7)


def test_generate_sync_with_prefix_end_to_end(gens, tmp_path):
    """``HuggingFaceGenerator.generate_sync(state, ..., prefix="rw [")`` over the real engine: every tactic begins with the
    prefix, the scores are the engine's ``generate(prefix=bytes + 3)`` scores, and the continuous path and the batched
    call return the same pairs."""
    import asyncio

    from test_generate_gpu import _save_generator_dir
    from reprover_amd.common import Pos
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator
    from reprover_amd.tokenizer import encode_one

    z, meta, get = gens
    cfg, sd = _weights("tiny", meta)
    path = str(tmp_path / "gen")
    _save_generator_dir(path, cfg, sd)
    args, state, nb = ("f.lean", "thm", Pos(1, 0)), "h : x = y ⊢ y = x", 4
    hf = HuggingFaceGenerator(path, DEV, 256, 24, 1.0)
    hf.initialize()
    out = hf.generate_sync(state, *args, nb, prefix="rw [")
    assert out and all(t.startswith("rw [") for t, _ in out)
    want = hf.generator.generate(encode_one(state, 256), nb, 24, 1.0, prefix=[b + 3 for b in b"rw ["])
    assert want.sequences[:, :5].tolist() == [[0] + [b + 3 for b in b"rw ["]] * nb
    assert [s for _, s in out] == want.sequences_scores.tolist()[: len(out)] or len(out) < nb  # (de-duplication drops rows)
    assert set(s for _, s in out) <= set(want.sequences_scores.tolist())
    assert hf.generate_sync(state, *args, nb, prefix="") == hf.generate_sync(state, *args, nb)
    both = hf.batch_generate_sync([state, state], [args[0]] * 2, [args[1]] * 2, [args[2]] * 2, nb, prefixes=["rw [", None])
    assert both[0] == out and both[1] == hf.generate_sync(state, *args, nb)
    cont = HuggingFaceGenerator(path, DEV, 256, 24, 1.0, continuous=True, continuous_slots=2)
    cont.initialize()

    async def main():
        return await asyncio.gather(cont.generate(state, *args, nb, prefix="rw ["), cont.generate(state, *args, nb))

    a, b = asyncio.run(main())
    assert a == out and b == both[1]


# ---- the ABI's refusals --------------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing():
    lib = _lib.load()
    assert lib.rp_abi_version() == _lib.ABI_VERSION == 7
    n, nb, max_len = 2, 3, 8
    b = Batch("tiny", n, nb, (5, 130), max_len)
    ws = b.fresh()
    keep = ws.clone()
    rows = [_i32([0, 5, 6]), _i32([0, 9])]
    bad = {
        "null states": dict(null="states"), "null prompt_cu": dict(null="prompt_cu"), "null tokens": dict(null="tokens"),
        "null anc": dict(null="anc"), "m = 0": dict(m=0), "m > n": dict(m=3),
        "prompt_cu[0] != 0": dict(prompt_cu=[1, 3, 5]), "an empty prompt": dict(prompt_cu=[0, 3, 3]),
        "R + 1 >= max_len": dict(prompt_cu=[0, 7, 9]), "anc_len below R": dict(anc_len=2),
        "num_beams cap": dict(nb=65), "states cap": dict(n=33), "max_len cap": dict(max_len=8193),
    }
    for what, kw in bad.items():
        assert b.prefill(ws, [0, 1], rows, **kw) == RP_E_INVALID, what
    assert b.prefill(ws, [0, 2], rows) == RP_E_INVALID and b.prefill(ws, [1, 1], rows) == RP_E_INVALID
    assert b.prefill(ws, [0, -1], rows) == RP_E_INVALID
    assert b.prefill(ws, [0, 1], rows, null="ws") == RP_E_WORKSPACE
    assert b.prefill(ws, [0, 1], rows, nbytes=b.bytes - 1) == RP_E_WORKSPACE
    # rp_decoder_batch_step_pos
    lp = torch.full((n * nb, b.V), 7.0, dtype=torch.float32, device=DEV)
    tok, anc = np.zeros(n * nb, np.int32), np.zeros((n * nb, 3), np.int32)
    for pos in ([0, 8], [-1, 0], [3, 0]):  # outside [0, max_len); anc_stride < pos + 1
        assert b.step_pos(ws, [0, 1], tok, anc, pos, lp=lp)[0] == RP_E_INVALID, pos
    assert b.step_pos(ws, [0, 0], tok, anc, [0, 0], lp=lp)[0] == RP_E_INVALID
    assert b.step_pos(ws, [0, 2], tok, anc, [0, 0], lp=lp)[0] == RP_E_INVALID
    assert b.step_pos(ws, [0, 1], tok, anc, [0, 0], lp=lp, nbytes=b.bytes - 1)[0] == RP_E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(ws, keep) and bool((lp == 7.0).all())
    # the pool's
    pl = Pool("tiny", 3, nb, max_len, 40)
    pws = torch.full((pl.bytes,), FILL, dtype=torch.uint8, device=DEV)
    for what, kw in {"null slots": dict(null="slots"), "null src_len": dict(null="src_len"), "null ws": dict(null="ws"),
                     "null anc": dict(null="anc"), "prompt_cu[0]": dict(prompt_cu=[1, 3, 5]),
                     "empty": dict(prompt_cu=[0, 0, 3]), "too long": dict(prompt_cu=[0, 7, 9]),
                     "anc_len": dict(anc_len=1), "slots cap": dict(shape=(33, nb, max_len, 40)),
                     "src_cap": dict(shape=(3, nb, max_len, 0))}.items():
        assert pl.prefill(pws, [0, 2], [17, 40], rows, **kw) == RP_E_INVALID, what
    assert pl.prefill(pws, [0, 3], [17, 40], rows) == RP_E_INVALID and pl.prefill(pws, [2, 2], [17, 40], rows) == RP_E_INVALID
    assert pl.prefill(pws, [0, 2], [17, 41], rows) == RP_E_INVALID and pl.prefill(pws, [0, 2], [0, 40], rows) == RP_E_INVALID
    assert pl.prefill(pws, [0, 2], [17, 40], rows, nbytes=pl.bytes - 1) == RP_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((pws == FILL).all())


# ---- workspace hygiene -------------------------------------------------------------------------------------------------------
def _out(name, shape, dtype, guard):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return Arena(name, n, guard, DEV, dtype=dtype)


@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_batch_prefill_and_step_pos_hygiene(name):
    """Cross K/V, a prefill of two states (7 and 2 rows: three passes of at most 6), then one rp_decoder_batch_step_pos at
    positions (7, 2), on an exactly-sized workspace poisoned before the cross K/V: the same log-prob bits under every
    fill, every guard intact, one byte less refused."""
    cfg, dec = _decoder(name)
    lib, g, V = dec._lib, guard_bytes(cfg["d_ff"]), cfg["vocab_size"]
    n, nb, max_len, lens = 2, 3, 10, (7, 2)
    src_cu = _i32([0, 5, 135])
    rng = np.random.default_rng(7)
    enc = Arena.of("enc_bf16", _enc_rows(cfg, 135, 3), g)
    ws = Arena("workspace", lib.rp_decoder_batch_workspace_bytes(dec._handle, _pc(src_cu), n, nb, max_len), g, DEV)
    rows = _prompts(rng, lens)
    prompt_cu, states, pos = _i32([0, 7, 9]), _i32([0, 1]), _i32(lens)
    a_ptok = Arena.of("prompt tokens", _t(np.concatenate(rows)), g)
    a_panc = Arena.of("prompt ancestry", _t((np.arange(7) * nb).astype(np.int32)), g)
    anc = np.zeros((n * nb, 8), np.int32)
    for s in range(n):
        anc[s * nb : (s + 1) * nb, : lens[s] + 1] = _beam0(nb, lens[s])
    a_tok = Arena.of("tokens", _t(rng.integers(0, 259, n * nb).astype(np.int32)), g)
    a_anc = Arena.of("ancestry", _t(anc), g)
    lp = _out("logprobs", (n * nb, V), torch.float32, g)

    def call(nbytes):
        st = lib.rp_decoder_batch_cross_kv(dec._handle, enc.ptr, _pc(src_cu), n, nb, max_len, ws.ptr, nbytes, _stream())
        if st:
            return st
        st = lib.rp_decoder_batch_prefill(dec._handle, _pc(src_cu), n, _pc(states), _pc(prompt_cu), 2, a_ptok.ptr, a_panc.ptr,
                                          7, nb, max_len, ws.ptr, nbytes, _stream())
        if st:
            return st
        return lib.rp_decoder_batch_step_pos(dec._handle, _pc(src_cu), n, _pc(states), 2, a_tok.ptr, a_anc.ptr, 8, nb,
                                             _pc(pos), max_len, lp.ptr, ws.ptr, nbytes, _stream())

    res = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, ws, [lp], [enc, a_ptok, a_panc, a_tok, a_anc], results=res)
    assert not found, "\n".join(found)
    out = res["logprobs"].view(-1, V)
    assert torch.isfinite(out).all() and bool((out <= 0).all())
    # each entry point alone refuses one byte less and writes nothing
    for one in (lambda nbytes: lib.rp_decoder_batch_prefill(dec._handle, _pc(src_cu), n, _pc(states), _pc(prompt_cu), 2,
                                                            a_ptok.ptr, a_panc.ptr, 7, nb, max_len, ws.ptr, nbytes, _stream()),
                lambda nbytes: lib.rp_decoder_batch_step_pos(dec._handle, _pc(src_cu), n, _pc(states), 2, a_tok.ptr,
                                                             a_anc.ptr, 8, nb, _pc(pos), max_len, lp.ptr, ws.ptr, nbytes,
                                                             _stream())):
        ws.fill(0xA5)
        lp.reset()
        assert one(ws.nbytes - 1) == RP_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((ws.payload() == 0xA5).all()) and lp.at_rest() and not ws.broken_guards()


@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_pool_prefill_hygiene(name):
    """Admission of slots 2 and 0, a prefill of both (2 and 7 rows) and one pool step at positions (7, 2) in slot order,
    on an exactly-sized pool workspace poisoned before the admission."""
    cfg, dec = _decoder(name)
    lib, g, V = dec._lib, guard_bytes(cfg["d_ff"]), cfg["vocab_size"]
    n_slots, nb, max_len, src_cap = 3, 2, 10, 40
    shape = (n_slots, nb, max_len, src_cap)
    rng = np.random.default_rng(8)
    enc = Arena.of("enc_bf16", _enc_rows(cfg, 57, 4), g)
    src_cu, slots, src_len = _i32([0, 17, 57]), _i32([2, 0]), _i32([17, 40])
    ws = Arena("workspace", lib.rp_decoder_pool_workspace_bytes(dec._handle, *shape), g, DEV)
    rows = _prompts(rng, (2, 7))
    prompt_cu = _i32([0, 2, 9])
    a_ptok = Arena.of("prompt tokens", _t(np.concatenate(rows)), g)
    a_panc = Arena.of("prompt ancestry", _t((np.arange(7) * nb).astype(np.int32)), g)
    active, pos, act_len = _i32([0, 2]), _i32([7, 2]), _i32([40, 17])
    anc = np.zeros((2 * nb, 8), np.int32)
    anc[:nb] = _beam0(nb, 7)
    anc[nb:, :3] = _beam0(nb, 2)
    a_tok = Arena.of("tokens", _t(rng.integers(0, 259, 2 * nb).astype(np.int32)), g)
    a_anc = Arena.of("ancestry", _t(anc), g)
    lp = _out("logprobs", (2 * nb, V), torch.float32, g)

    def call(nbytes):
        st = lib.rp_decoder_pool_admit(dec._handle, *shape, _pc(slots), enc.ptr, _pc(src_cu), 2, ws.ptr, nbytes, _stream())
        if st:
            return st
        st = lib.rp_decoder_pool_prefill(dec._handle, *shape, _pc(slots), _pc(src_len), _pc(prompt_cu), 2, a_ptok.ptr,
                                         a_panc.ptr, 7, ws.ptr, nbytes, _stream())
        if st:
            return st
        return lib.rp_decoder_pool_step(dec._handle, *shape, _pc(active), _pc(pos), _pc(act_len), 2, a_tok.ptr, a_anc.ptr, 8,
                                        lp.ptr, ws.ptr, nbytes, _stream())

    res = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, ws, [lp], [enc, a_ptok, a_panc, a_tok, a_anc], results=res)
    assert not found, "\n".join(found)
    out = res["logprobs"].view(-1, V)
    assert torch.isfinite(out).all() and bool((out <= 0).all())
    ws.fill(0xA5)
    st = lib.rp_decoder_pool_prefill(dec._handle, *shape, _pc(slots), _pc(src_len), _pc(prompt_cu), 2, a_ptok.ptr,
                                     a_panc.ptr, 7, ws.ptr, ws.nbytes - 1, _stream())
    torch.cuda.synchronize()
    assert st == RP_E_WORKSPACE and bool((ws.payload() == 0xA5).all()) and not ws.broken_guards()
