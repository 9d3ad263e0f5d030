"""Continuous batching on the MI355X (rp_decoder_pool_*, HipT5Decoder.pool_*, HipT5Generator.generate_stream,
HuggingFaceGenerator(continuous=True)): slots of one step stand at different positions and give, row for row and cache
row for cache row, the bytes of the per-state rp_decoder_step; a slot taken again needs no clearing; whole searches that
join a running loop equal ``generate`` bit for bit.  Every comparison is equality against entry points that exist
already; there is no tolerance."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import simulated_search, source_ids  # noqa: E402
from hip_helpers import Arena, guard_bytes, hygiene_findings  # noqa: E402  (the guard-page harness of the hygiene tests)
from test_generate_batch_gpu import _g20, _same_output, _save_generator_dir, _sources  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = _lib.C


def _pc(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _up(n, to=256):
    return (n + to - 1) // to * to


@pytest.fixture(scope="module")
def tiny_gen(golden_dir):
    z, cfg, sd = _g20(golden_dir)
    return z, cfg, sd, HipT5Generator(cfg, sd, DEV)


def _dims(cfg):
    L, inner = cfg["num_decoder_layers"], cfg["num_heads"] * cfg["d_kv"]
    return L, inner, L * 2 * inner  # layers, H * d_kv, elements of one cross-K/V row


# ---- step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 4, 64])
def test_pool_step_rows_and_cache_rows_equal_the_per_state_step(tiny_gen, nb):
    """Slots at positions 0, 5 and 257 (past the attention's 256-wide key pass) over sources of 1, 257 and 300 tokens in
    one rp_decoder_pool_step.  Each state's cache comes from running it alone through rp_decoder_step up to its position
    with a simulated search's ancestry; the pool's log-prob rows and the slot's whole cache after the step (the rows it
    wrote included) are the per-state call's bytes.  Then again with the states in other slots, listed in another order."""
    z, cfg, sd, gen = tiny_gen
    dec, lib, h = gen.decoder, _lib.load(), gen.decoder._handle
    L, inner, nkv = _dims(cfg)
    V, T, cap = cfg["vocab_size"], 258, 300
    positions, lens = [0, 5, 257], [1, 257, 300]
    srcs = [source_ids(n, 90 + i) for i, n in enumerate(lens)]
    encs = [gen.encode_hidden(s) for s in srcs]
    cache_bytes = L * T * nb * 2 * inner * 2  # one state's self-attention cache
    before, after, want, inputs = [], [], [], []
    for i, (pos, e) in enumerate(zip(positions, encs)):
        need = lib.rp_decoder_workspace_bytes(h, nb, T, lens[i])
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        off = _up(lens[i] * nkv * 2)
        _lib.check(lib.rp_decoder_cross_kv(h, e.data_ptr(), lens[i], nb, T, ws.data_ptr(), need, None), "rp_decoder_cross_kv")
        lp = torch.empty((nb, V), dtype=torch.float32, device=DEV)
        for t, tok, anc in simulated_search(nb, pos + 1, seed=200 + 10 * nb + i):
            tok, anc = tok.to(DEV, torch.int32), anc.to(DEV, torch.int32).contiguous()
            if t == pos:
                before.append(ws[off : off + cache_bytes].clone())
                inputs.append((tok, anc))
            _lib.check(lib.rp_decoder_step(h, tok.data_ptr(), anc.data_ptr(), t + 1, nb, t, T, lens[i], lp.data_ptr(),
                                           ws.data_ptr(), need, None), "rp_decoder_step")
        after.append(ws[off : off + cache_bytes].clone())
        want.append(lp.clone())
        assert not torch.equal(before[i], after[i])  # the step at `pos` wrote its rows
    n_slots = 3
    need = lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, T, cap)
    assert need > 0
    cache0 = _up(n_slots * cap * nkv * 2)
    W = max(positions) + 1
    for place, order in (([0, 1, 2], [0, 1, 2]), ([2, 0, 1], [1, 2, 0])):  # state i sits in slot place[i]; listing order
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        enc = torch.cat(encs).contiguous()
        _lib.check(lib.rp_decoder_pool_admit(h, n_slots, nb, T, cap, _pc(_i32(*place)), enc.data_ptr(), _pc(cu), 3,
                                             ws.data_ptr(), need, None), "rp_decoder_pool_admit")
        for i in range(3):
            at = cache0 + place[i] * cache_bytes
            ws[at : at + cache_bytes] = before[i]
        tok = torch.cat([inputs[i][0] for i in order]).contiguous()
        anc = torch.zeros((3 * nb, W), dtype=torch.int32, device=DEV)
        for a, i in enumerate(order):
            anc[a * nb : (a + 1) * nb, : positions[i] + 1] = inputs[i][1]
        lp = torch.full((3 * nb, V), 7.0, dtype=torch.float32, device=DEV)
        _lib.check(lib.rp_decoder_pool_step(h, n_slots, nb, T, cap, _pc(_i32(*[place[i] for i in order])),
                                            _pc(_i32(*[positions[i] for i in order])), _pc(_i32(*[lens[i] for i in order])),
                                            3, tok.data_ptr(), anc.data_ptr(), W, lp.data_ptr(), ws.data_ptr(), need, None),
                   "rp_decoder_pool_step")
        for a, i in enumerate(order):
            assert torch.equal(lp[a * nb : (a + 1) * nb].view(torch.int32), want[i].view(torch.int32)), (place, i)
            at = cache0 + place[i] * cache_bytes
            assert torch.equal(ws[at : at + cache_bytes], after[i]), (place, i)


# ---- admission -----------------------------------------------------------------------------------------------------------
def test_admitted_cross_kv_rows_equal_batch_cross_kv(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    dec, lib, h = gen.decoder, _lib.load(), gen.decoder._handle
    L, inner, nkv = _dims(cfg)
    srcs = [source_ids(n, 300 + n) for n in (300, 1, 129)]
    cu = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.int32)
    enc = gen.encode_hidden_packed(np.concatenate(srcs), cu)
    nb, T, cap, n_slots = 4, 8, 300, 4
    dec.start_many(enc, cu, nb, T)  # rp_decoder_batch_cross_kv
    want = dec._ws[: int(cu[-1]) * nkv * 2].clone().view(int(cu[-1]), nkv * 2)
    dec.pool_open(n_slots, nb, T, cap)
    dec._pool_ws.fill_(0x5A)
    slots = [3, 0, 2]
    dec.pool_admit(slots, enc, cu)
    region = dec._pool_ws[: n_slots * cap * nkv * 2].view(n_slots, cap, nkv * 2)
    for j, s in enumerate(slots):
        n = len(srcs[j])
        assert torch.equal(region[s, :n], want[int(cu[j]) : int(cu[j + 1])]), j
        assert bool((region[s, n:] == 0x5A).all())  # nothing past the source's rows
    assert bool((region[1] == 0x5A).all())  # a slot that was not named
    assert bool((dec._pool_ws[_up(n_slots * cap * nkv * 2) :] == 0x5A).all())  # admission writes cross K/V only


def test_a_slot_taken_again_needs_no_clearing(tiny_gen):
    """A 300-token source runs in slot 0 up to position 40; then a 3-token source is admitted into slot 0 and takes three
    steps (beside a second slot that keeps stepping).  Its log-probs are those of a pool that never held anyone else,
    with the workspace pre-filled with 0x00, 0xFF and 0x7F, every guard intact, the workspace exactly
    rp_decoder_pool_workspace_bytes long and one byte less refused with nothing written."""
    z, cfg, sd, gen = tiny_gen
    lib, h = _lib.load(), gen.decoder._handle
    g, V = guard_bytes(cfg["d_ff"]), cfg["vocab_size"]
    nb, T, cap, n_slots = 4, 48, 300, 2
    old, new, other = source_ids(300, 41), source_ids(3, 42), source_ids(33, 43)
    a_old, a_new, a_other = (Arena.of(n, gen.encode_hidden(s), g) for n, s in (("enc_old", old), ("enc_new", new),
                                                                               ("enc_other", other)))
    ws = Arena("workspace", lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, T, cap), g, DEV)
    run_old = list(simulated_search(nb, 41, seed=7))
    run_other = list(simulated_search(nb, 44, seed=8))
    run_new = list(simulated_search(nb, 3, seed=9))
    dev = lambda x: x.to(DEV, torch.int32).contiguous()  # noqa: E731
    scratch = torch.empty((2 * nb, V), dtype=torch.float32, device=DEV)
    lps = [Arena(f"logprobs{t}", 2 * nb * V * 4, g, DEV, dtype=torch.float32) for t in range(3)]
    steps = []  # (active, pos, src_len, tokens arena, ancestry arena, width, output pointer)
    ins = [a_old, a_new, a_other]
    for t in range(44):
        first = run_old[t] if t <= 40 else run_new[t - 41]
        p0 = t if t <= 40 else t - 41
        W = t + 1
        anc = torch.zeros((2 * nb, W), dtype=torch.int64)
        anc[:nb, : p0 + 1] = first[2]
        anc[nb:] = run_other[t][2]
        a_tok = Arena.of(f"tokens{t}", dev(torch.cat([first[1], run_other[t][1]])), g)
        a_anc = Arena.of(f"ancestry{t}", dev(anc), g)
        ins += [a_tok, a_anc]
        steps.append((_i32(0, 1), _i32(p0, t), _i32(len(old) if t <= 40 else len(new), len(other)), a_tok, a_anc, W,
                      scratch.data_ptr() if t <= 40 else lps[t - 41].ptr))

    def admit(slots, arena, n, nbytes):
        return lib.rp_decoder_pool_admit(h, n_slots, nb, T, cap, _pc(_i32(*slots)), arena.ptr, _pc(_i32(0, n)), 1, ws.ptr,
                                         nbytes, _lib.current_stream())

    def run_steps(which, nbytes):
        for act, pos, sl, a_tok, a_anc, W, out in which:
            st = lib.rp_decoder_pool_step(h, n_slots, nb, T, cap, _pc(act), _pc(pos), _pc(sl), len(act), a_tok.ptr, a_anc.ptr,
                                          W, out, ws.ptr, nbytes, _lib.current_stream())
            if st:
                return st
        return 0

    def call(nbytes):
        st = admit([0], a_old, len(old), nbytes) or admit([1], a_other, len(other), nbytes)
        st = st or run_steps(steps[:41], nbytes)
        st = st or admit([0], a_new, len(new), nbytes)  # slot 0 again, as the old tenant left it
        return st or run_steps(steps[41:], nbytes)

    res = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, ws, lps, ins, results=res)
    assert not found, "\n".join(found)

    def fresh(nbytes):  # the newcomer in a pool nobody used: the other slot still has to reach its positions
        st = admit([1], a_other, len(other), nbytes)
        for act, pos, sl, a_tok, a_anc, W, out in steps[:41]:  # slot 1 alone (its rows are the table's second half)
            tok1 = a_tok.view()[nb:].contiguous()
            anc1 = a_anc.view(2 * nb, W)[nb:].contiguous()
            st = st or lib.rp_decoder_pool_step(h, n_slots, nb, T, cap, _pc(act[1:]), _pc(pos[1:]), _pc(sl[1:]), 1,
                                                tok1.data_ptr(), anc1.data_ptr(), W, scratch.data_ptr(), ws.ptr, nbytes,
                                                _lib.current_stream())
        st = st or admit([0], a_new, len(new), nbytes)
        return st or run_steps(steps[41:], nbytes)

    for a in lps + ins:
        a.reset()
    ws.fill(0x00)
    with torch.cuda.device(DEV):
        assert fresh(ws.nbytes) == 0
    torch.cuda.synchronize()
    for t in range(3):
        got = lps[t].payload().view(torch.float32)
        assert torch.equal(got.view(torch.int32), res[f"logprobs{t}"].view(torch.int32)), t
        assert torch.isfinite(got).all() and bool((got <= 0).all())  # log-softmax rows, not the fill


# ---- whole searches ------------------------------------------------------------------------------------------------------
_ALONE = {}


def _alone(gen, key, src, nb, ml, lp):
    """generate(src) once per (source, shape): the reference the stream's tickets are compared with"""
    k = (key, nb, ml, lp)
    if k not in _ALONE:
        _ALONE[k] = gen.generate(src, nb, ml, lp)
    return _ALONE[k]


def _run_stream(gen, srcs, nb, ml, lp, n_slots, schedule):
    stream = gen.generate_stream(nb, ml, lp, n_slots=n_slots, src_cap=512)
    got, tickets, finish = {}, [], {}

    def take(pairs):
        for ticket, out in pairs:
            got[ticket], finish[ticket] = out, stream.steps
    if schedule == "one_every_3_steps":
        for s in srcs:
            tickets.append(stream.submit(s))
            for _ in range(3):
                take(stream.step())
    else:
        tickets = [stream.submit(s) for s in srcs]
    while stream.queued or stream.in_flight:
        take(stream.step())
    assert sorted(got) == sorted(tickets)
    return [got[t] for t in tickets], [finish[t] for t in tickets]


@pytest.mark.parametrize("schedule", ["all_at_once", "one_every_3_steps", "a_slot_each"])
@pytest.mark.parametrize("lp", [0.0, 1.0])
@pytest.mark.parametrize("nb,n_src,n_slots,ml", [(4, 5, 2, 64), (64, 4, 3, 128)])
def test_stream_equals_generate(tiny_gen, nb, n_src, n_slots, ml, lp, schedule):
    """More sources than slots (slots are taken again), all there at the start or one newcomer every three steps, and
    once with a slot for everyone: every ticket's sequences and scores are generate(source)'s bits.  The max_length
    values are those at which these sources' searches stop at different steps (4 beams: 27 .. 63 of 63; 64 beams at
    length_penalty 0: 70 .. 127 of 127); at 64 beams and length_penalty 1 every search runs to max_length at any
    max_length tried up to 128, so there only the schedules stagger the states."""
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])[:n_src]
    outs, finish = _run_stream(gen, srcs, nb, ml, lp, None if schedule == "a_slot_each" else n_slots, schedule)
    print("finish steps:", finish)
    for i, s in enumerate(srcs):
        _same_output(outs[i], _alone(gen, i, s, nb, ml, lp))
    if (nb == 4 or lp == 0.0) and schedule == "a_slot_each":  # all admitted at step 0: the finish step is the search's own
        assert len(set(finish)) > 1 and min(finish) <= max(finish) - 3, finish


def test_stream_refuses_a_source_longer_than_src_cap(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    stream = gen.generate_stream(4, 8, 0.0, n_slots=2, src_cap=16)
    with pytest.raises(ValueError):
        stream.submit(source_ids(17, 1))
    with pytest.raises(ValueError):
        stream.submit(np.zeros(0, dtype=np.int32))
    t = stream.submit(source_ids(16, 1))
    (ticket, out), = stream.drain()
    assert ticket == t
    _same_output(out, gen.generate(source_ids(16, 1), 4, 8, 0.0))
    gen.generate_stream(4, 8, 0.0, n_slots=2, src_cap=16)  # the decoder carries one stream: the first is retired
    stream.submit(source_ids(5, 2))
    with pytest.raises(RuntimeError):
        stream.step()


def test_stream_byt5_small_width_64_beams():
    """ByT5-small dimensions, 64 beams, 2 slots, 3 sources of about 300 bytes."""
    cfg = synth.seq2seq_config("byt5-small")
    gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg), DEV)
    srcs = [source_ids(300, 51), source_ids(287, 52), source_ids(311, 53)]
    outs, finish = _run_stream(gen, srcs, 64, 24, 0.0, 2, "all_at_once")
    print("finish steps:", finish)
    for o, s in zip(outs, srcs):
        _same_output(o, gen.generate(s, 64, 24, 0.0))


# ---- product -------------------------------------------------------------------------------------------------------------
def test_continuous_generate_equals_generate_sync(golden_dir, tmp_path):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    z, cfg, sd = _g20(golden_dir)
    gdir = str(tmp_path / "gen")
    _save_generator_dir(gdir, cfg, sd)
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900, 33)]
    hf = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, continuous=True, continuous_slots=2)
    hf.initialize()
    args = ("f.lean", "thm", Pos(1, 0), 8)

    async def main():
        return await asyncio.gather(*(hf.generate(s, *args) for s in states))

    got = asyncio.run(main())
    assert got == [hf.generate_sync(s, *args) for s in states]  # tactics, scores (exact floats), de-duplication order
    assert hf._driver is None and not hf._waiters and hf._stream.in_flight == 0 and hf._stream.queued == 0
    assert hf._stream.pool.n_slots == 2


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_pool_refusals_carry_messages_and_launch_nothing(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    lib, h = _lib.load(), gen.decoder._handle
    V = cfg["vocab_size"]
    n_slots, nb, T, cap = 3, 4, 8, 16
    need = lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, T, cap)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    tok = torch.zeros(2 * nb, dtype=torch.int32, device=DEV)
    anc = torch.zeros((2 * nb, 4), dtype=torch.int32, device=DEV)
    lp = torch.full((2 * nb, V), 123.5, dtype=torch.float32, device=DEV)
    enc = torch.zeros((8, cfg["d_model"]), dtype=torch.bfloat16, device=DEV)
    ok = dict(active=_i32(0, 2), pos=_i32(3, 0), src_len=_i32(16, 1), n=2, tokens=tok.data_ptr(), anc=anc.data_ptr(),
              stride=4, lp=lp.data_ptr(), ws=ws.data_ptr(), bytes=need)

    def step(**kw):
        a = dict(ok, **kw)
        ptr = lambda x: None if x is None else _pc(x)  # noqa: E731
        st = lib.rp_decoder_pool_step(h, n_slots, nb, T, cap, ptr(a["active"]), ptr(a["pos"]), ptr(a["src_len"]), a["n"],
                                      a["tokens"], a["anc"], a["stride"], a["lp"], a["ws"], a["bytes"], None)
        torch.cuda.synchronize()
        return st, lib.rp_last_error()

    def refused(status, word, **kw):
        st, msg = step(**kw)
        assert st == status and msg and word in msg, (kw, st, msg)
        assert bool((lp == 123.5).all()) and not bool(ws.any())  # nothing was launched

    for name in ("active", "pos", "src_len", "tokens", "anc", "lp", "ws"):
        refused(-1, b"null", **{name: None})
    refused(-1, b"active[1]=3", active=_i32(0, 3))
    refused(-1, b"active[0]=-1", active=_i32(-1, 2))
    refused(-1, b"twice", active=_i32(2, 2))
    refused(-1, b"pos[0]=8", pos=_i32(8, 0))
    refused(-1, b"pos[1]=-1", pos=_i32(3, -1))
    refused(-1, b"src_len[0]=17", src_len=_i32(17, 1))
    refused(-1, b"src_len[1]=0", src_len=_i32(16, 0))
    refused(-1, b"anc_stride", stride=3)
    refused(-1, b"active slots=0", n=0)
    refused(-1, b"active slots=4", n=4)
    refused(-3, b"workspace", bytes=need - 1)
    st, _ = step()
    assert st == 0 and torch.isfinite(lp).all() and bool((lp <= 0).all())  # the accepted call does write
    # the workspace size and the admission
    err = lib.rp_last_error
    assert lib.rp_decoder_pool_workspace_bytes(None, n_slots, nb, T, cap) == 0 and b"null" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, 33, 4, T, cap) == 0 and b"slots=33" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, 17, 64, T, cap) == 0 and b"rows" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, 16, 64, T, cap) > 0
    assert lib.rp_decoder_pool_workspace_bytes(h, n_slots, 65, T, cap) == 0 and b"num_beams=65" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, 8193, cap) == 0 and b"max_len" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, T, 0) == 0 and b"src_cap" in err()
    assert lib.rp_decoder_pool_workspace_bytes(h, n_slots, nb, T, 8193) == 0 and b"src_cap" in err()
    ws.zero_()

    def admit(slots, cu, m, e=enc.data_ptr(), w=ws.data_ptr(), n=need):
        st = lib.rp_decoder_pool_admit(h, n_slots, nb, T, cap, None if slots is None else _pc(slots), e,
                                       None if cu is None else _pc(cu), m, w, n, None)
        torch.cuda.synchronize()
        return st
    for word, args, kw in ((b"null", (None, _i32(0, 8), 1), {}), (b"null", (_i32(0), None, 1), {}),
                           (b"null", (_i32(0), _i32(0, 8), 1), dict(e=None)), (b"null", (_i32(0), _i32(0, 8), 1), dict(w=None)),
                           (b"slots[0]=3", (_i32(3), _i32(0, 8), 1), {}), (b"twice", (_i32(1, 1), _i32(0, 4, 8), 2), {}),
                           (b"src_len of source 0", (_i32(0), _i32(0, 17), 1), {}),
                           (b"src_len of source 1", (_i32(0, 1), _i32(0, 8, 8), 2), {}),
                           (b"src_cu[0]", (_i32(0), _i32(1, 8), 1), {}), (b"admitted sources=0", (_i32(0), _i32(0, 8), 0), {})):
        assert admit(*args, **kw) == -1 and word in err(), (word, err())
    assert admit(_i32(0), _i32(0, 8), 1, n=need - 1) == -3 and b"workspace" in err()
    assert not bool(ws.any())  # no refused admission wrote anything
    assert admit(_i32(2), _i32(0, 8), 1) == 0
