"""Generate fixture G29: what every entry point of reprover_amd/csrc/rp_decoder.hip answers to a refused call.

Usage:
    python tests/golden/make_golden_decoder_refusals.py cpu     # the section that needs no GPU
    python tests/golden/make_golden_decoder_refusals.py gpu     # the section that needs a decoder handle (MI355X)

G29  ``g29_decoder_refusals.json``: two sections, each a table ``"entry(overrides)" -> [status, rp_last_error text]``.  A
     case is the entry's accepted call with the named arguments replaced.  Every ``RP_REQUIRE`` / ``fail`` of an entry is
     hit, every range is crossed on both sides (the inside value together with a fault that is checked later, so the call
     is still refused and shows that the earlier check let it through), and calls with two faults pin which is reported
     first.  The one message that prints a pointer (``params=%p``) is recorded with the pointer replaced by ``<ptr>``.
     Accepted size queries (``rp_beam_books_bytes``, the three ``*_workspace_bytes``) are recorded as ``[bytes, ""]``.

     ``cpu``  the entries that take no decoder handle - ``rp_beam_select_batch``, the seven ``rp_sample_*`` entries, the
              six ``rp_beam_books_*`` / ``rp_beam_*advance`` entries - and the null-decoder call of every decoder entry.
              Every call is a refusal, so nothing is launched and no GPU is needed; the pointers that would be device
              pointers name a host buffer that no refused call reads.
     ``gpu``  the entries that need a handle (batch / pool / prefill / per-state, ``rp_dbg_dec_rows`` mode 3,
              ``rp_dbg_dec_attention``) on the ``tiny`` seq2seq configuration with 3 slots, 4 beams, ``max_len`` 8,
              ``src_cap`` 16.  ``after`` is called after every refused call (the replaying test checks there that the
              workspace and every output buffer still hold their fill pattern); one accepted call per entry closes the
              section, recorded as ``[0, ""]``.

     The fixture was written on the commit before the decoder file's entry points were folded onto one list check, one
     geometry and one layer walk.  tests/test_decoder_refusals_cpu.py and tests/test_decoder_refusals_gpu.py record again
     and compare.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

G29_FILE = "g29_decoder_refusals.json"
N, NB, T, CAP = 3, 4, 8, 16  # states / slots, beams, max_len, src_cap
FILL_BYTE, FILL_F32 = 0xA5, 123.5
_PTR = re.compile(r"=0x[0-9a-fA-F]+|=\(nil\)")


def I(*v):  # noqa: E743
    return np.array(v, dtype=np.int32)


def R(n):
    return np.arange(n, dtype=np.int32)


class Off:
    """The address of ``buf`` plus ``by`` bytes (a misaligned pointer)."""

    def __init__(self, buf, by):
        self.buf, self.by = buf, by


def _ptr(v):
    if v is None or isinstance(v, (int, float)):
        return v
    if isinstance(v, C.c_void_p):  # a handle
        return v.value
    if isinstance(v, Off):
        return _ptr(v.buf) + v.by
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    return v.data_ptr()  # a torch tensor


def _show(v):
    if v is None:
        return "null"
    if isinstance(v, np.ndarray):
        s = v.tolist()
        return str(s).replace(" ", "") if len(s) <= 6 else f"[{s[0]},{s[1]},..,{s[-2]},{s[-1]}]x{len(s)}"
    if isinstance(v, Off):
        return f"+{v.by}"
    return repr(v)


class Entry:
    def __init__(self, name, params, ok, size=False, tag=""):
        self.name, self.params, self.ok, self.size, self.tag = name, params.split(), ok, size, tag
        assert set(self.params) == set(ok), (name, set(self.params) ^ set(ok))

    def call(self, lib, kw):
        assert set(kw) <= set(self.ok), (self.name, kw)
        a = dict(self.ok, **kw)
        return getattr(lib, self.name)(*[_ptr(a[p]) for p in self.params])


def _run(lib, table, entry, cases, after=None):
    for kw in cases:
        key = f"{entry.name}{entry.tag}({', '.join(f'{k}={_show(v)}' for k, v in kw.items())})"
        assert key not in table, key
        st = int(entry.call(lib, kw))
        refused = st == 0 if entry.size else st != 0
        msg = _PTR.sub("=<ptr>", lib.rp_last_error().decode()) if refused else ""
        assert refused or entry.size, f"{key} was accepted: every case but a size query is a refusal"
        table[key] = [st, msg]
        if after is not None:
            after(key)


def _nulls(*names):
    return [{n: None} for n in names]


# ---- the section without a GPU ------------------------------------------------------------------------------------------------
def record_cpu(lib) -> dict:
    out = {}
    raw = np.zeros((1 << 16) + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 64:][: 1 << 16]  # 64-byte aligned; stands for every device pointer: no refused call reads it
    run = lambda e, cases: _run(lib, out, e, cases)  # noqa: E731

    # rp_beam_select_batch
    e = Entry("rp_beam_select_batch", "lp running n_active nb V k scores tokens parents ws ws_bytes stream",
              dict(lp=buf, running=buf, n_active=2, nb=NB, V=16, k=8, scores=buf, tokens=buf, parents=buf, ws=buf,
                   ws_bytes=2 * NB * 8 * 8, stream=None))
    run(e, _nulls("lp", "running", "scores", "tokens", "parents") + [
        dict(n_active=0), dict(n_active=33), dict(nb=0), dict(nb=65), dict(V=0), dict(V=513), dict(k=0), dict(k=129),
        dict(nb=1, V=4, k=5), dict(ws=None), dict(ws_bytes=2 * NB * 8 * 8 - 1),
        dict(n_active=1, nb=1, V=1, k=1, ws_bytes=7), dict(n_active=32, nb=64, V=512, k=128, ws_bytes=0),
        dict(nb=2, V=4, k=8, ws_bytes=0),
        dict(lp=None, n_active=0), dict(n_active=0, nb=0), dict(nb=0, V=0), dict(V=0, k=0), dict(k=0, ws=None)])

    # the sampler's four steps
    step_ok = dict(lp=buf, V=16, active=I(0, 2), n_active=2, n=N, nb=NB, seeds=buf, max_len=T, eos=1, pad=0, seq=buf,
                   tokens_next=buf, cum=buf, ngen=buf, fin=buf, stream=None)
    scalars = dict(temperature=1.0, top_k=0, top_p=1.0)
    tail = "eos pad seq tokens_next cum ngen fin stream"
    steps = [
        Entry("rp_sample_step", "lp V active n_active n nb seeds t max_len temperature top_k top_p " + tail,
              dict(step_ok, t=3, **scalars)),
        Entry("rp_sample_step_rows", "lp V active n_active n nb seeds t max_len params " + tail,
              dict(step_ok, t=3, params=buf)),
        Entry("rp_sample_pool_step", "lp V active pos n_active n nb seeds max_len temperature top_k top_p " + tail,
              dict(step_ok, pos=I(3, 0), **scalars)),
        Entry("rp_sample_pool_step_rows", "lp V active pos n_active n nb seeds max_len params " + tail,
              dict(step_ok, pos=I(3, 0), params=buf)),
    ]
    for e in steps:
        pool, rows = "pos" in e.ok, "params" in e.ok
        cases = _nulls("lp", "active", "seeds", "seq", "tokens_next", "cum", "ngen", "fin")
        if pool:
            cases += [dict(pos=None), dict(pos=None, lp=None), dict(pos=None, V=0)]
        if rows:
            cases += [dict(params=None), dict(params=Off(buf, 4)), dict(params=Off(buf, 8)), dict(lp=None, params=None),
                      dict(params=None, V=0), dict(params=Off(buf, 4), V=0)]
        else:
            cases += [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
                      dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                      dict(top_k=-1), dict(lp=None, temperature=0.0), dict(temperature=0.0, top_p=0.0),
                      dict(top_p=0.0, top_k=-1), dict(top_k=-1, V=0),
                      dict(temperature=3.0e38, top_p=1e-30, top_k=1 << 30, V=0)]
        cases += [dict(V=0), dict(V=513), dict(nb=0), dict(nb=65), dict(n=0), dict(n=33), dict(max_len=1),
                  dict(n_active=17, n=17, nb=64), dict(n_active=33, n=3, nb=32), dict(V=0, nb=0), dict(nb=0, n=0),
                  dict(n=0, max_len=1), dict(max_len=1, n_active=300), dict(n_active=0), dict(n_active=4),
                  dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)), dict(active=I(3, 3)),
                  dict(n_active=300, nb=1), dict(V=512, nb=64, n=16, n_active=16, active=np.append(R(15), 14).astype(np.int32),
                                                **(dict(pos=np.zeros(16, np.int32)) if pool else dict(t=0))),
                  dict(V=1, nb=1, n=32, n_active=32, active=np.append(R(31), 32).astype(np.int32),
                       **(dict(pos=np.full(32, 6, np.int32)) if pool else dict(t=6)))]
        if pool:
            cases += [dict(pos=I(-1, 0)), dict(pos=I(3, 7)), dict(pos=I(7, -1)), dict(max_len=2, pos=I(0, 1)),
                      dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)), dict(active=I(0, 3), pos=I(0, 9)),
                      dict(n_active=0, pos=I(9, 9))]
        else:
            cases += [dict(t=-1), dict(t=7), dict(t=6, active=I(2, 2)), dict(max_len=2, t=1), dict(t=-1, n_active=0),
                      dict(t=7, active=I(2, 2)), dict(max_len=1, t=-1)]
        run(e, cases)

    # the sampler's admission and row rebuild
    admit_ok = dict(states=I(0, 2), new_seeds=np.array([7, 9], np.uint32), m=2, n=N, nb=NB, max_len=T, start=0, pad=0,
                    seeds=buf, seq=buf, cum=buf, ngen=buf, fin=buf, stream=None)
    atail = "m n nb max_len start pad seeds seq cum ngen fin stream"
    for e in (Entry("rp_sample_pool_admit", "states new_seeds " + atail, admit_ok),
              Entry("rp_sample_pool_admit_rows", "states new_seeds n_live " + atail, dict(admit_ok, n_live=I(4, 1)))):
        cases = _nulls("states", "new_seeds", "seeds", "seq", "cum", "ngen", "fin") + [
            dict(nb=0), dict(nb=65), dict(n=0), dict(n=33), dict(max_len=1), dict(m=17, n=17, nb=64), dict(m=0), dict(m=4),
            dict(states=I(0, 3)), dict(states=I(-1, 2)), dict(states=I(2, 2)), dict(states=I(3, 3)),
            dict(states=None, nb=0), dict(nb=0, n=0), dict(n=0, max_len=1), dict(max_len=1, m=0), dict(m=0, states=I(9, 9)),
            dict(m=300, nb=64), dict(m=300, nb=1), dict(max_len=2, states=I(1, 1)),
            dict(nb=64, n=16, m=16, states=np.append(R(15), 16).astype(np.int32), new_seeds=np.zeros(16, np.uint32),
                 **(dict(n_live=np.full(16, 64, np.int32)) if "n_live" in e.ok else {})),
            dict(nb=1, n=32, m=32, states=np.append(R(31), 0).astype(np.int32), new_seeds=np.zeros(32, np.uint32),
                 **(dict(n_live=np.full(32, 1, np.int32)) if "n_live" in e.ok else {}))]
        if "n_live" in e.ok:
            cases += [dict(n_live=None), dict(n_live=I(0, 1)), dict(n_live=I(4, 5)), dict(n_live=I(4, -1)),
                      dict(states=I(2, 2), n_live=I(4, 0)), dict(states=I(0, 3), n_live=I(9, 9)),
                      dict(states=I(0, 2), n_live=I(9, 9)), dict(n_live=None, nb=0)]
        run(e, cases)
    e = Entry("rp_sample_pool_rows", "active pos n_active n nb max_len seq tokens_next stream",
              dict(active=I(0, 2), pos=I(3, 0), n_active=2, n=N, nb=NB, max_len=T, seq=buf, tokens_next=buf, stream=None))
    run(e, _nulls("active", "pos", "seq", "tokens_next") + [
        dict(nb=0), dict(nb=65), dict(n=0), dict(n=33), dict(max_len=1), dict(n_active=17, n=17, nb=64), dict(n_active=0),
        dict(n_active=4), dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)), dict(pos=I(-1, 0)),
        dict(pos=I(3, 7)), dict(max_len=2, pos=I(0, 1)), dict(active=None, nb=0), dict(nb=0, n=0), dict(max_len=1, n_active=0),
        dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)), dict(n_active=0, active=I(9, 9)),
        dict(nb=64, n=16, n_active=16, active=np.append(R(15), 14).astype(np.int32), pos=np.full(16, 6, np.int32)),
        dict(nb=1, n=32, n_active=32, active=R(32), pos=np.append(np.zeros(31, np.int32), 7).astype(np.int32))])

    # the beam books
    e = Entry("rp_beam_books_bytes", "n nb max_len", dict(n=N, nb=NB, max_len=T), size=True)
    run(e, [dict(), dict(n=1, nb=1, max_len=2), dict(n=16, nb=64, max_len=8192), dict(n=32, nb=32, max_len=7), dict(nb=0),
            dict(nb=65), dict(n=0), dict(n=33), dict(n=17, nb=64), dict(max_len=1), dict(max_len=8193), dict(nb=0, n=0),
            dict(n=0, max_len=1), dict(n=33, nb=64), dict(n=17, nb=64, max_len=1)])
    need = int(lib.rp_beam_books_bytes(N, NB, T))
    caps = [dict(nb=0), dict(nb=65), dict(n=0), dict(n=33), dict(n=17, nb=64), dict(max_len=1), dict(max_len=8193),
            dict(nb=0, n=0), dict(n=0, max_len=1)]
    books = dict(books=buf, bytes=need, n=N, nb=NB, max_len=T)
    e = Entry("rp_beam_books_init", "books bytes n nb max_len eos start stream", dict(books, eos=1, start=0, stream=None))
    run(e, caps + [dict(books=None), dict(bytes=need - 1), dict(bytes=0), dict(nb=0, books=None), dict(books=None, bytes=0),
                   dict(n=32, nb=32, max_len=8192, bytes=need), dict(n=1, nb=1, max_len=2, bytes=15)])
    adv = dict(books, active=I(0, 2), n_active=2, scores=buf, tokens=buf, parents=buf, eos=1, stream=None)
    e = Entry("rp_beam_advance", "books bytes n nb max_len active n_active t scores tokens parents fin_div run_div eos stream",
              dict(adv, t=3, fin_div=1.0, run_div=1.0))
    run(e, caps + _nulls("books", "active", "scores", "tokens", "parents") + [
        dict(n_active=0), dict(n_active=4), dict(t=-1), dict(t=7), dict(active=I(0, 3)), dict(active=I(-1, 2)),
        dict(active=I(2, 2)), dict(bytes=need - 1), dict(max_len=2, t=1), dict(max_len=2, t=0, bytes=0),
        dict(t=6, bytes=0), dict(nb=0, books=None), dict(books=None, n_active=0), dict(n_active=0, t=-1),
        dict(t=7, active=I(2, 2)), dict(active=I(3, 3), bytes=0), dict(active=I(2, 2), bytes=0),
        dict(n=32, nb=32, n_active=32, active=R(32), bytes=need)])
    e = Entry("rp_beam_pool_advance",
              "books bytes n nb max_len active pos n_active scores tokens parents fin_div run_div eos stream",
              dict(adv, pos=I(3, 0), fin_div=np.ones(2, np.float32), run_div=np.ones(2, np.float32)))
    run(e, caps + _nulls("books", "active", "pos", "scores", "tokens", "parents", "fin_div", "run_div") + [
        dict(n_active=0), dict(n_active=4), dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)),
        dict(pos=I(-1, 0)), dict(pos=I(3, 7)), dict(pos=I(6, 0), bytes=0), dict(bytes=need - 1), dict(nb=0, pos=None),
        dict(pos=None, n_active=0), dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)),
        dict(active=I(0, 3), pos=I(0, 9)), dict(pos=I(3, 7), bytes=0), dict(max_len=2, pos=I(0, 0), bytes=0),
        dict(n=32, nb=32, n_active=32, active=R(32), pos=np.zeros(32, np.int32), fin_div=np.ones(32, np.float32),
             run_div=np.ones(32, np.float32), bytes=need)])
    e = Entry("rp_beam_books_admit", "books bytes n nb max_len states m eos start stream",
              dict(books, states=I(0, 2), m=2, eos=1, start=0, stream=None))
    run(e, caps + _nulls("books", "states") + [
        dict(m=0), dict(m=4), dict(states=I(0, 3)), dict(states=I(-1, 2)), dict(states=I(2, 2)), dict(states=I(3, 3)),
        dict(bytes=need - 1), dict(nb=0, states=None), dict(states=None, m=0), dict(m=0, bytes=0), dict(states=I(2, 2), bytes=0),
        dict(n=32, nb=32, m=32, states=R(32), bytes=need), dict(m=3, states=I(2, 1, 0), bytes=0)])
    e = Entry("rp_beam_books_rows", "books bytes n nb max_len active pos n_active stream",
              dict(books, active=I(0, 2), pos=I(3, 0), n_active=2, stream=None))
    run(e, caps + _nulls("books", "active", "pos") + [
        dict(n_active=0), dict(n_active=4), dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)),
        dict(pos=I(-1, 0)), dict(pos=I(3, 7)), dict(pos=I(6, 6), bytes=0), dict(bytes=need - 1), dict(nb=0, active=None),
        dict(active=None, n_active=0), dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)),
        dict(pos=I(3, 7), bytes=0)])

    # a null decoder, every decoder entry (a second fault after it: the handle is looked at first)
    for e, more in decoder_entries(None, buf, buf, buf, buf, buf, 1 << 16).values():
        if "d" in e.ok:
            run(e, [dict(), dict(ws_bytes=0)] if "ws_bytes" in e.ok else [dict()])
    cfgp = Entry("rp_decoder_load_params", "d params stream", dict(d=None, params=buf, stream=None))
    run(cfgp, [dict()])
    return out


# ---- the section with a decoder handle ------------------------------------------------------------------------------------
SRC_CU = I(0, 16, 17, 25)  # sources of 16, 1 and 8 rows


def decoder_entries(h, ws, enc, tokens, anc, lp, need_batch, need_pool=None, need_one=None):
    """name -> (Entry, its refused cases): the entries that take a decoder handle, their accepted call over the given
    buffers (device tensors with a handle; with ``h`` None any non-null pointer)."""
    need_pool = need_batch if need_pool is None else need_pool
    need_one = need_batch if need_one is None else need_one
    E = {}
    wide = dict(n=32, src_cu=R(33), nb=32, max_len=8192)  # the caps' far side, refused later for its workspace
    dec_caps = [dict(src_cu=None), dict(n=0), dict(n=33, src_cu=R(34)), dict(nb=0), dict(nb=65),
                dict(n=17, nb=64, src_cu=R(18)), dict(max_len=0), dict(max_len=8193), dict(src_cu=I(1, 16, 17, 25)),
                dict(src_cu=I(0, 0, 17, 25)), dict(src_cu=I(0, 16, 16, 25)), dict(src_cu=I(0, 8193, 8194, 8200)),
                dict(src_cu=I(0, 16, 17, 5)), dict(src_cu=None, n=0), dict(n=0, nb=0), dict(nb=0, max_len=0),
                dict(nb=65, n=17, src_cu=R(18)), dict(max_len=0, src_cu=I(1, 16, 17, 25)),
                dict(src_cu=I(1, 0, 17, 25))]
    pool_caps = [dict(n_slots=0), dict(n_slots=33), dict(nb=0), dict(nb=65), dict(n_slots=17, nb=64), dict(max_len=0),
                 dict(max_len=8193), dict(src_cap=0), dict(src_cap=8193), dict(n_slots=0, nb=0), dict(nb=0, max_len=0),
                 dict(n_slots=17, nb=65), dict(max_len=0, src_cap=0)]
    batch = dict(d=h, src_cu=SRC_CU, n=N, nb=NB, max_len=T, ws=ws, ws_bytes=need_batch, stream=None)
    pool = dict(d=h, n_slots=N, nb=NB, max_len=T, src_cap=CAP, ws=ws, ws_bytes=need_pool, stream=None)
    sizes = lambda d: {k: v for k, v in d.items() if k not in ("ws", "ws_bytes", "stream")}  # noqa: E731

    E["batch_ws"] = (Entry("rp_decoder_batch_workspace_bytes", "d src_cu n nb max_len", sizes(batch), size=True),
                     [dict(), dict(n=1, src_cu=I(0, 1), nb=1, max_len=1), dict(n=2, src_cu=I(0, 8192, 8200), nb=64, max_len=300)]
                     + dec_caps)
    E["pool_ws"] = (Entry("rp_decoder_pool_workspace_bytes", "d n_slots nb max_len src_cap", sizes(pool), size=True),
                    [dict(), dict(n_slots=1, nb=1, max_len=1, src_cap=1), dict(n_slots=16, nb=64, max_len=32, src_cap=8192)]
                    + pool_caps)
    E["one_ws"] = (Entry("rp_decoder_workspace_bytes", "d nb max_len S", dict(d=h, nb=NB, max_len=T, S=16), size=True),
                   [dict(), dict(nb=1, max_len=1, S=1), dict(nb=64, max_len=300, S=8192), dict(nb=0), dict(nb=65),
                    dict(max_len=0), dict(max_len=8193), dict(S=0), dict(S=8193), dict(S=-1), dict(nb=0, S=0)])

    E["batch_cross_kv"] = (Entry("rp_decoder_batch_cross_kv", "d enc src_cu n nb max_len ws ws_bytes stream", dict(batch, enc=enc)),
                           dec_caps + [dict(enc=None), dict(ws=None), dict(ws_bytes=need_batch - 1), dict(n=0, enc=None),
                                       dict(enc=None, ws=None), dict(wide, ws_bytes=0)])
    step = dict(batch, active=I(0, 2), n_active=2, tokens=tokens, anc=anc, astride=T, lp=lp)
    lists = [dict(n_active=0), dict(n_active=4), dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)),
             dict(active=I(3, 3)), dict(ws_bytes=need_batch - 1), dict(active=I(2, 2), ws_bytes=0)]
    E["batch_step"] = (
        Entry("rp_decoder_batch_step", "d src_cu n active n_active tokens anc astride nb t max_len lp ws ws_bytes stream",
              dict(step, t=3)),
        dec_caps + _nulls("active", "tokens", "anc", "lp") + lists + [
            dict(ws=None), dict(t=-1), dict(t=8), dict(astride=3), dict(astride=4, ws_bytes=0), dict(t=7, ws_bytes=0),
            dict(t=0, astride=1, ws_bytes=0), dict(n=0, active=None), dict(lp=None, n_active=0), dict(n_active=0, t=-1),
            dict(t=8, astride=0), dict(t=8, active=I(2, 2)), dict(astride=3, active=I(0, 3)), dict(ws=None, ws_bytes=0),
            dict(wide, t=8191, astride=8192, n_active=32, active=R(32), ws_bytes=0)])
    E["batch_step_pos"] = (
        Entry("rp_decoder_batch_step_pos", "d src_cu n active n_active tokens anc astride nb pos max_len lp ws ws_bytes stream",
              dict(step, pos=I(3, 0))),
        dec_caps + _nulls("active", "pos", "tokens", "anc", "lp") + lists + [
            dict(ws=None), dict(pos=I(8, 0)), dict(pos=I(3, -1)), dict(astride=3), dict(pos=I(0, 3), astride=3),
            dict(pos=I(7, 0), ws_bytes=0), dict(astride=4, ws_bytes=0), dict(n=0, pos=None), dict(pos=None, n_active=0),
            dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)), dict(active=I(0, 3), pos=I(0, 9)),
            dict(pos=I(8, 0), astride=0), dict(pos=I(3, 8), astride=3),
            dict(wide, pos=np.full(32, 8191, np.int32), astride=8192, n_active=32, active=R(32), ws_bytes=0)])
    E["pool_admit"] = (
        Entry("rp_decoder_pool_admit", "d n_slots nb max_len src_cap slot_ids enc src_cu m ws ws_bytes stream",
              dict(pool, slot_ids=I(2), enc=enc, src_cu=I(0, 8), m=1)),
        pool_caps + _nulls("slot_ids", "enc", "src_cu", "ws") + [
            dict(m=0), dict(m=4), dict(src_cu=I(1, 8)), dict(slot_ids=I(3)), dict(slot_ids=I(-1)),
            dict(slot_ids=I(1, 1), src_cu=I(0, 4, 8), m=2), dict(src_cu=I(0, 17)), dict(src_cu=I(0, 0)),
            dict(slot_ids=I(0, 1), src_cu=I(0, 8, 8), m=2), dict(src_cu=I(0, 16), ws_bytes=0), dict(src_cu=I(0, 1), ws_bytes=0),
            dict(ws_bytes=need_pool - 1), dict(n_slots=0, slot_ids=None), dict(ws=None, m=0), dict(m=0, src_cu=I(1, 8)),
            dict(src_cu=I(1, 8), slot_ids=I(3)), dict(slot_ids=I(3), src_cu=I(0, 17)),
            dict(slot_ids=I(1, 1), src_cu=I(0, 4, 40), m=2), dict(src_cu=I(0, 17), ws_bytes=0),
            dict(n_slots=32, nb=32, max_len=8192, src_cap=8192, m=32, slot_ids=R(32), src_cu=(R(33) * 8192).astype(np.int32),
                 ws_bytes=0)])
    E["pool_step"] = (
        Entry("rp_decoder_pool_step",
              "d n_slots nb max_len src_cap active pos src_len n_active tokens anc astride lp ws ws_bytes stream",
              dict(pool, active=I(0, 2), pos=I(3, 0), src_len=I(16, 1), n_active=2, tokens=tokens, anc=anc, astride=T, lp=lp)),
        pool_caps + _nulls("active", "pos", "src_len", "tokens", "anc", "lp", "ws") + [
            dict(n_active=0), dict(n_active=4), dict(active=I(0, 3)), dict(active=I(-1, 2)), dict(active=I(2, 2)),
            dict(pos=I(8, 0)), dict(pos=I(3, -1)), dict(src_len=I(17, 1)), dict(src_len=I(16, 0)), dict(astride=3),
            dict(pos=I(0, 3), astride=3), dict(ws_bytes=need_pool - 1), dict(pos=I(7, 0), ws_bytes=0),
            dict(astride=4, ws_bytes=0), dict(n_slots=0, active=None), dict(ws=None, n_active=0),
            dict(n_active=0, active=I(9, 9)), dict(active=I(2, 2), pos=I(9, 9)), dict(active=I(0, 0), pos=I(0, 9)),
            dict(pos=I(8, 0), src_len=I(17, 1)), dict(src_len=I(17, 1), astride=3), dict(pos=I(3, 8), astride=3),
            dict(astride=3, ws_bytes=0), dict(active=I(2, 2), ws_bytes=0),
            dict(n_slots=32, nb=32, max_len=8192, src_cap=8192, n_active=32, active=R(32), pos=np.full(32, 8191, np.int32),
                 src_len=np.full(32, 8192, np.int32), astride=8192, ws_bytes=0)])
    prompts = [dict(m=0), dict(m=4), dict(prompt_cu=I(1, 3, 5)), dict(prompt_cu=I(0, 0, 2)), dict(prompt_cu=I(0, 3, 3)),
               dict(prompt_cu=I(0, 3, 1)), dict(prompt_cu=I(0, 7, 9)), dict(prompt_cu=I(0, 3, 10)), dict(anc_len=2),
               dict(prompt_cu=I(0, 2, 5), anc_len=2), dict(prompt_cu=I(0, 6, 8), anc_len=6, ws_bytes=0),
               dict(prompt_cu=I(0, 1, 2), anc_len=1, ws_bytes=0), dict(m=0, prompt_cu=I(1, 3, 5)),
               dict(prompt_cu=I(1, 0, 5)), dict(prompt_cu=I(0, 7, 9), anc_len=2), dict(prompt_cu=I(0, 3, 10), anc_len=2)]
    E["batch_prefill"] = (
        Entry("rp_decoder_batch_prefill", "d src_cu n states prompt_cu m tokens anc anc_len nb max_len ws ws_bytes stream",
              dict(batch, states=I(0, 2), prompt_cu=I(0, 3, 5), m=2, tokens=tokens, anc=anc, anc_len=3)),
        dec_caps + _nulls("states", "prompt_cu", "tokens", "anc") + prompts + [
            dict(states=I(0, 3)), dict(states=I(-1, 2)), dict(states=I(2, 2)), dict(ws=None), dict(ws_bytes=need_batch - 1),
            dict(n=0, states=None), dict(anc=None, m=0), dict(prompt_cu=I(0, 0, 2), states=I(2, 2)),
            dict(anc_len=2, states=I(0, 3)), dict(states=I(3, 3)), dict(states=I(2, 2), ws_bytes=0), dict(ws=None, ws_bytes=0),
            dict(wide, m=32, states=R(32), prompt_cu=(R(33) * 8190).astype(np.int32), anc_len=8190, ws_bytes=0)])
    E["pool_prefill"] = (
        Entry("rp_decoder_pool_prefill",
              "d n_slots nb max_len src_cap slot_ids src_len prompt_cu m tokens anc anc_len ws ws_bytes stream",
              dict(pool, slot_ids=I(0, 2), src_len=I(16, 1), prompt_cu=I(0, 3, 5), m=2, tokens=tokens, anc=anc, anc_len=3)),
        pool_caps + _nulls("slot_ids", "src_len", "prompt_cu", "tokens", "anc", "ws") + prompts + [
            dict(slot_ids=I(0, 3)), dict(slot_ids=I(-1, 2)), dict(slot_ids=I(2, 2)), dict(src_len=I(17, 1)),
            dict(src_len=I(16, 0)), dict(ws_bytes=need_pool - 1), dict(n_slots=0, slot_ids=None), dict(ws=None, m=0),
            dict(prompt_cu=I(0, 0, 2), slot_ids=I(2, 2)), dict(anc_len=2, slot_ids=I(0, 3)),
            dict(slot_ids=I(2, 2), src_len=I(17, 1)), dict(slot_ids=I(0, 0), src_len=I(16, 0)),
            dict(slot_ids=I(0, 3), src_len=I(16, 0)), dict(src_len=I(16, 0), ws_bytes=0), dict(slot_ids=I(2, 2), ws_bytes=0),
            dict(n_slots=32, nb=32, max_len=8192, src_cap=8192, m=32, slot_ids=R(32), src_len=np.full(32, 8192, np.int32),
                 prompt_cu=(R(33) * 8190).astype(np.int32), anc_len=8190, ws_bytes=0)])
    one = dict(d=h, nb=NB, max_len=T, S=16, ws=ws, ws_bytes=need_one, stream=None)
    one_caps = [dict(nb=0), dict(nb=65), dict(max_len=0), dict(max_len=8193), dict(S=0), dict(S=8193), dict(nb=0, S=0)]
    E["cross_kv"] = (Entry("rp_decoder_cross_kv", "d enc S nb max_len ws ws_bytes stream", dict(one, enc=enc)),
                     one_caps + [dict(enc=None), dict(ws=None), dict(ws_bytes=need_one - 1), dict(S=0, enc=None),
                                 dict(enc=None, ws_bytes=0), dict(nb=64, max_len=8192, S=8192, ws_bytes=0)])
    E["step"] = (
        Entry("rp_decoder_step", "d tokens anc astride nb t max_len S lp ws ws_bytes stream",
              dict(one, tokens=tokens, anc=anc, astride=T, t=3, lp=lp)),
        one_caps + _nulls("tokens", "anc", "lp", "ws") + [
            dict(t=-1), dict(t=8), dict(astride=3), dict(ws_bytes=need_one - 1), dict(t=7, ws_bytes=0),
            dict(astride=4, ws_bytes=0), dict(S=0, tokens=None), dict(lp=None, t=8), dict(t=8, astride=0),
            dict(astride=3, ws_bytes=0), dict(nb=64, max_len=8192, S=8192, t=8191, astride=8192, ws_bytes=0)])
    return E


def record_gpu(lib, after=None, accepted=None) -> dict:
    """The section with a handle.  ``after(key, bufs)`` runs after every refused call, ``accepted(name, bufs)`` after every
    accepted one; ``bufs`` names the workspace and the output buffers."""
    import torch

    from reprover_amd import synth
    from reprover_amd.decoder import HipT5Decoder

    dev = "cuda:0"
    cfg = synth.seq2seq_config("tiny")
    dec = HipT5Decoder(cfg, synth.synth_seq2seq_state_dict(cfg), dev)
    h = dec._handle
    D, V, H = cfg["d_model"], cfg["vocab_size"], cfg["num_heads"]
    inner, L = H * cfg["d_kv"], cfg["num_decoder_layers"]
    need_batch = int(lib.rp_decoder_batch_workspace_bytes(h, SRC_CU.ctypes.data, N, NB, T))
    need_pool = int(lib.rp_decoder_pool_workspace_bytes(h, N, NB, T, CAP))
    need_one = int(lib.rp_decoder_workspace_bytes(h, NB, T, 16))
    assert min(need_batch, need_pool, need_one) > 0
    bufs = dict(ws=torch.full((max(need_batch, need_pool, need_one),), FILL_BYTE, dtype=torch.uint8, device=dev),
                lp=torch.full((N * NB, V), FILL_F32, dtype=torch.float32, device=dev))
    enc = torch.zeros((int(SRC_CU[-1]), D), dtype=torch.bfloat16, device=dev)
    tokens = torch.zeros(N * NB, dtype=torch.int32, device=dev)
    anc = torch.zeros((N * NB, T), dtype=torch.int32, device=dev)
    out = {}
    hook = None if after is None else (lambda key: (torch.cuda.synchronize(), after(key, bufs)))
    E = decoder_entries(h, bufs["ws"], enc, tokens, anc, bufs["lp"], need_batch, need_pool, need_one)
    for e, cases in E.values():
        _run(lib, out, e, cases, hook)

    # the two test entries that take a slot table
    rows, stride = T * NB, T * NB * 2 * inner
    bufs["cache"] = torch.full((N * stride,), FILL_F32, dtype=torch.bfloat16, device=dev)
    bufs["att"] = torch.full((2 * NB, inner), FILL_F32, dtype=torch.bfloat16, device=dev)
    qkv = torch.zeros((2 * NB, 3 * inner), dtype=torch.bfloat16, device=dev)
    ckv = torch.zeros((int(SRC_CU[-1]), L * 2 * inner), dtype=torch.bfloat16, device=dev)
    tab = torch.zeros((H, 5), dtype=torch.float32, device=dev)
    table = dict(state=I(0, 2), pos=I(3, 0), n_active=2, n_states=N, nb=NB, max_len=T)
    slot_cases = [dict(state=None), dict(pos=None), dict(n_states=0), dict(n_states=33), dict(n_active=0), dict(n_active=4),
                  dict(nb=0), dict(nb=65), dict(n_active=17, n_states=17, nb=64, state=R(17), pos=np.zeros(17, np.int32)),
                  dict(max_len=0), dict(max_len=8193), dict(state=I(0, 3)), dict(state=I(-1, 2)), dict(state=I(2, 2)),
                  dict(pos=I(8, 0)), dict(pos=I(3, -1)), dict(state=None, n_states=0), dict(n_states=0, n_active=0),
                  dict(n_active=0, nb=0), dict(nb=0, max_len=0), dict(max_len=0, state=I(9, 9)),
                  dict(state=I(2, 2), pos=I(9, 9)), dict(state=I(0, 0), pos=I(0, 9)), dict(state=I(0, 3), pos=I(0, 9))]
    e_rows = Entry("rp_dbg_dec_rows",
                   "mode a b ia rows n vocab eps scale state pos n_active n_states nb max_len state_stride o0 stream",
                   dict(table, mode=3, a=qkv, b=None, ia=None, rows=0, n=inner, vocab=0, eps=0.0, scale=0.0, state_stride=stride,
                        o0=bufs["cache"], stream=None))
    _run(lib, out, e_rows, slot_cases + [dict(o0=None), dict(n=0), dict(mode=4), dict(mode=-1), dict(a=None),
                                         dict(state_stride=stride - 1), dict(o0=None, mode=4), dict(n=0, state=None),
                                         dict(pos=I(8, 0), a=None), dict(a=None, state_stride=0),
                                         dict(n_states=32, n_active=32, nb=32, max_len=8192, state=R(32),
                                              pos=np.full(32, 8191, np.int32))], hook)
    att = dict(table, q=qkv, ldq=3 * inner, koff=0, voff=inner, nb=NB, H=H, out=bufs["att"], ldo=inner, stream=None)
    e_self = Entry("rp_dbg_dec_attention",
                   "cross q ldq kv ldkv koff voff rows state_stride n_states anc astride tab nbias nb H state src_off src_len pos "
                   "n_active max_len out ldo stream",
                   dict(att, cross=0, kv=bufs["cache"], ldkv=2 * inner, rows=rows, state_stride=stride, anc=anc, astride=T,
                        tab=tab, nbias=5, src_off=None, src_len=None), tag="[self]")
    _run(lib, out, e_self, slot_cases + _nulls("q", "kv", "out", "anc", "tab") + [
        dict(H=0), dict(ldq=64 * H - 8), dict(ldo=64 * H - 1), dict(ldq=3 * inner + 4), dict(ldkv=2 * inner + 4), dict(koff=-8),
        dict(koff=4), dict(voff=-1), dict(koff=2 * inner - 8), dict(voff=2 * inner - 63), dict(q=Off(qkv, 2)),
        dict(kv=Off(bufs["cache"], 8)), dict(nbias=0), dict(rows=rows - 1), dict(state_stride=rows * 2 * inner - 8),
        dict(state_stride=stride + 4), dict(astride=3), dict(pos=I(0, 3), astride=3), dict(q=None, H=0), dict(H=0, ldkv=4),
        dict(ldkv=4, q=Off(qkv, 2)), dict(q=Off(qkv, 2), state=None), dict(pos=I(8, 0), anc=None), dict(anc=None, rows=0),
        dict(rows=0, astride=0)], hook)
    e_cross = Entry("rp_dbg_dec_attention", " ".join(e_self.params),
                    dict(att, cross=1, kv=ckv, ldkv=L * 2 * inner, rows=int(SRC_CU[-1]), state_stride=0, anc=None, astride=0,
                         tab=None, nbias=0, src_off=I(0, 17), src_len=I(16, 8)), tag="[cross]")
    _run(lib, out, e_cross, _nulls("src_off", "src_len", "q", "state") + [
        dict(src_len=I(0, 8)), dict(src_len=I(16, 8193)), dict(src_off=I(-1, 17)), dict(src_off=I(0, 18)),
        dict(src_off=I(10, 17)), dict(src_len=I(0, 8), src_off=I(-1, 17)), dict(src_len=I(16, 0), src_off=I(-1, 17)),
        dict(state=I(2, 2), src_len=I(0, 0)), dict(pos=I(8, 0), src_off=I(-1, -1))], hook)

    # one accepted call per entry: the handle works
    ok = lambda name: (torch.cuda.synchronize(), accepted(name, bufs)) if accepted is not None else None  # noqa: E731
    bufs["ws"].zero_()
    for key in ("batch_cross_kv", "batch_prefill", "batch_step", "batch_step_pos", "cross_kv", "step", "pool_admit",
                "pool_prefill", "pool_step"):
        e = E[key][0]
        st = int(e.call(lib, {}))
        out[f"{e.name}()"] = [st, ""]
        ok(e.name)
    for e in (e_rows, e_self, e_cross):
        st = int(e.call(lib, {}))
        out[f"{e.name}{e.tag}()"] = [st, ""]
        ok(e.name + e.tag)
    torch.cuda.synchronize()
    return out


def main():
    from reprover_amd import _lib, build

    section = sys.argv[1] if len(sys.argv) > 1 else ""
    assert section in ("cpu", "gpu"), __doc__
    build.build()
    lib = _lib.load()
    got = record_cpu(lib) if section == "cpu" else record_gpu(lib)
    assert got == (record_cpu(lib) if section == "cpu" else record_gpu(lib)), "the record is not repeatable"
    path = os.path.join(os.environ.get("RP_G29_DIR", HERE), G29_FILE)
    whole = {}
    if os.path.exists(path):
        with open(path) as fh:
            whole = json.load(fh)
    whole[section] = got
    with open(path, "w") as fh:
        json.dump(whole, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"wrote {path}: section {section}, {len(got)} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
