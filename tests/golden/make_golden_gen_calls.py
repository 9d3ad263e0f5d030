"""Generate the call-trace fixture G28 of the generation drivers (no GPU, no HuggingFace).

Usage:
    python tests/golden/make_golden_gen_calls.py

G28  Every search function and pool of ``reprover_amd.generation`` run through its public API over a scripted host
     model, with a logging wrapper around every callable it is handed (``admit``, ``step`` / ``step_many``,
     ``select_many``, ``advance``, ``books_admit``, ``rows``, ``sample_step``, ``prefill`` / ``prefill_many``,
     ``to_host``).  Per call the fixture holds the structure only - the callable's name, ``active``, ``pos`` or ``t`` or
     that neither was passed, the other list arguments, every tensor's dtype and shape - and per pool ``step`` the
     tickets it returned.  No token and no score is recorded, so the file does not depend on the CPU it was written on:
     the model's EOS logit is -40 before a scripted position per source and +40 from it on (one source never stops
     before ``max_length``), which leaves no stop to a near-tie.

     5 sources, 2 beams / samples, vocabulary 9, ``max_length`` 8; the pools with all 5 submitted into 2 slots and with
     one newcomer every 3 steps into 3 slots.  tests/test_generation_calls_cpu.py records again and compares.
"""
from __future__ import annotations

import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sample_params_helpers import CpuRowSampler  # noqa: E402
from sample_pool_helpers import CpuPoolSampler  # noqa: E402
from reprover_amd import generation as G  # noqa: E402

G28_FILE = "g28_gen_calls.json"
EOS, START = 1, 0
NB, V, ML, LP = 2, 9, 8, 1.0
N_SRC = 5
EOS_FROM = (3, 5, 99, 2, 6)     # source i's EOS logit turns from -BOOST to +BOOST at this position; source 2 never stops
BOOST = 40.0
PROMPTS = (None, [4, 5], [3], None, [6, 7, 8])  # unequal lengths; source 4 starts at position 3
SEEDS = (41, 42, 43, 0xFFFFFFF5, 45)
SCHEDULES = ("5_sources_2_slots", "one_every_3_steps")


def _sig(x):
    """The structure of one argument: a tensor as dtype and shape, anything else as it is."""
    if isinstance(x, torch.Tensor):
        return str(x.dtype).replace("torch.", "") + str(list(x.shape)).replace(" ", "")
    if isinstance(x, (list, tuple)):
        return "[" + ",".join(_sig(y) for y in x) + "]"
    if isinstance(x, (G.BeamBooks, G.SampleState)):
        return type(x).__name__
    return repr(x)


class Recorder:
    def __init__(self):
        self.calls = []

    def note(self, name, *args, **kw):
        self.calls.append(" ".join([name] + [_sig(a) for a in args] + [f"{k}={_sig(v)}" for k, v in kw.items()]))

    def wrap(self, name, fn):
        def logged(*args, **kw):
            self.note(name, *args, **kw)
            return fn(*args, **kw)
        return logged

    def to_host(self, x):
        self.note("to_host", x)
        return x.cpu()


def log_probs(sources, positions, tokens, nb):
    """fp32 ``[len(sources) * nb, V]``: row ``a * nb + b`` from (source, position, the row's token) alone."""
    out = []
    for a, (i, t) in enumerate(zip(sources, positions)):
        for b in range(nb):
            g = torch.Generator().manual_seed((i * 64 + int(t)) * 1024 + int(tokens[a * nb + b]))
            logits = torch.randn(V, generator=g)
            logits[EOS] = BOOST if t >= EOS_FROM[i] else -BOOST
            out.append(torch.log_softmax(logits, -1))
    return torch.stack(out)


class Scripted:
    """The model behind every protocol; ``rec`` receives every call."""

    def __init__(self, rec, nb=NB, only=None):
        self.rec, self.nb, self.only, self.slot_src = rec, nb, only, {}

    def step_one(self, tokens, ancestry):  # beam_search / greedy_search
        self.rec.note("step", tokens, ancestry)
        return log_probs([self.only], [ancestry.shape[1] - 1], tokens, self.nb)

    def step_many(self, active, tokens, ancestry, **kw):  # the host-books loops: pos= only with prompts
        self.rec.note("step_many", active, tokens, ancestry, **kw)
        pos = kw["pos"] if "pos" in kw else [ancestry.shape[1] - 1] * len(active)
        return log_probs(active, pos, tokens, self.nb)

    def step_many_t(self, active, tokens, ancestry, t):  # the device-books loops
        self.rec.note("step_many", active, tokens, ancestry, t=t)
        return log_probs(active, [t] * len(active), tokens, self.nb)

    def admit(self, slots, sources):
        self.rec.note("admit", slots, sources)
        for s, src in zip(slots, sources):
            self.slot_src[s] = src

    def pool_step(self, active, pos, tokens, ancestry):
        self.rec.note("step", active, pos, tokens, ancestry)
        return log_probs([self.slot_src[s] for s in active], pos, tokens, self.nb)


def _drive(rec, pool, submit, schedule):
    """Run ``pool`` over the 5 sources by ``schedule``; every ``step``'s tickets go to ``rec``."""
    def one_step():
        rec.note("-> step returned", [t for t, _ in pool.step()])

    if schedule == "one_every_3_steps":
        for i in range(N_SRC):
            submit(i)
            for _ in range(3):
                one_step()
    else:
        for i in range(N_SRC):
            submit(i)
    while pool.queued or pool.in_flight:
        one_step()
    one_step()  # an idle pool: nothing is called
    rec.note("-> steps", pool.steps, getattr(pool, "sync_points", None))


def _slots(schedule):
    return 2 if schedule == "5_sources_2_slots" else 3


def record(lib) -> dict:
    """case name -> the list of its calls, in order."""
    cases = {}

    def case(name):
        rec = cases[name] = Recorder()
        return rec, Scripted(rec)

    select_many = lambda rec: rec.wrap("select_many", G.topk_select_many)  # noqa: E731

    for prompt in (None, PROMPTS[4]):
        rec, m = case("beam_search" + ("" if prompt is None else " prompt"))
        m.only = 4
        G.beam_search(m.step_one, NB, ML, LP, select=rec.wrap("select", G.topk_select), prompt=prompt)
        rec, m = case("greedy_search" + ("" if prompt is None else " prompt"))
        m.only, m.nb = 4, 1
        G.greedy_search(m.step_one, ML, prompt=prompt)

    for prompts in (None, PROMPTS):
        tag = "" if prompts is None else " prompts"
        rec, m = case("beam_search_batch" + tag)
        G.beam_search_batch(m.step_many, N_SRC, NB, ML, LP, select_many=select_many(rec), prompts=prompts)
        rec, m = case("greedy_search_batch" + tag)
        m.nb = 1
        G.greedy_search_batch(m.step_many, N_SRC, ML, prompts=prompts)
    rec, m = case("beam_search_batch prompts prefill_many")
    G.beam_search_batch(m.step_many, N_SRC, NB, ML, LP, select_many=select_many(rec), prompts=PROMPTS,
                        prefill_many=rec.wrap("prefill_many", lambda states, rows: None))
    rec, m = case("greedy_search_batch prompts prefill_many")
    m.nb = 1
    G.greedy_search_batch(m.step_many, N_SRC, ML, prompts=PROMPTS,
                          prefill_many=rec.wrap("prefill_many", lambda states, rows: None))

    for k in (1, 3):
        rec, m = case(f"beam_search_batch_device sync_every={k}")
        G.beam_search_batch_device(m.step_many_t, select_many(rec), rec.wrap("advance", G.beam_advance_host), N_SRC, NB,
                                   ML, LP, sync_every=k, init=rec.wrap("init", G.beam_books_init_host),
                                   to_host=rec.to_host)

    table = torch.stack([G.SamplingParams([0.8, 1.5], [0, 1], [1.0, 0.9]).rows(NB) if i % 2 else
                         G.SamplingParams().rows(NB) for i in range(N_SRC)])
    for params in (None, table):
        for k in (1, 3):
            rec, m = case(f"sample_search_batch sync_every={k}" + ("" if params is None else " params"))
            sampler = CpuPoolSampler(lib) if params is None else CpuRowSampler(lib)
            G.sample_search_batch(m.step_many_t, rec.wrap("sample_step", sampler.at), N_SRC, NB, ML, list(SEEDS),
                                  sync_every=k, params=params)

    for schedule in SCHEDULES:
        for prefill in (False, True):
            rec, m = case(f"BeamSearchPool {schedule}" + (" prefill" if prefill else ""))
            pool = G.BeamSearchPool(m.admit, m.pool_step, _slots(schedule), NB, ML, LP, select_many=select_many(rec),
                                    prefill=rec.wrap("prefill", lambda slots, rows: None) if prefill else None)
            _drive(rec, pool, lambda i: pool.submit(i, prompt=PROMPTS[i]), schedule)
        for k in (1, 3):
            rec, m = case(f"BeamBooksPool {schedule} sync_every={k}")
            pool = G.BeamBooksPool(m.admit, m.pool_step, _slots(schedule), NB, ML, LP, select_many=select_many(rec),
                                   sync_every=k, books_admit=rec.wrap("books_admit", G.beam_books_admit_host),
                                   advance=rec.wrap("advance", G.beam_pool_advance_host),
                                   rows=rec.wrap("rows", G.beam_books_rows_host), to_host=rec.to_host)
            _drive(rec, pool, lambda i: pool.submit(i), schedule)
            rec, m = case(f"SamplePool {schedule} sync_every={k}")
            pool = G.SamplePool(m.admit, m.pool_step, rec.wrap("sample_step", CpuPoolSampler(lib)), _slots(schedule),
                                NB, ML, sync_every=k, books_admit=rec.wrap("books_admit", G.sample_books_admit_host),
                                rows=rec.wrap("rows", G.sample_books_rows_host), to_host=rec.to_host)
            _drive(rec, pool, lambda i: pool.submit(i, SEEDS[i]), schedule)
            rec, m = case(f"SamplePool {schedule} sync_every={k} per_request")
            pool = G.SamplePool(m.admit, m.pool_step, rec.wrap("sample_step", CpuRowSampler(lib)), _slots(schedule),
                                NB, ML, sync_every=k, books_admit=rec.wrap("books_admit", G.sample_books_admit_host),
                                rows=rec.wrap("rows", G.sample_books_rows_host), to_host=rec.to_host, per_request=True,
                                params=G.SamplingParams(1.2, 0, 0.95))
            tickets = (dict(params=G.SamplingParams([0.8, 1.5], [0, 1], [1.0, 0.9])), dict(num_samples=1),
                       dict(params=G.SamplingParams(0.8, 1, 1.0), num_samples=1), dict(), dict(num_samples=2))
            _drive(rec, pool, lambda i: pool.submit(i, SEEDS[i], **tickets[i]), schedule)
    return {name: rec.calls for name, rec in cases.items()}


def main():
    from reprover_amd import _lib, build

    build.build()
    lib = _lib.load()
    got = record(lib)
    torch.set_num_threads(1)
    assert record(lib) == got, "the trace depends on the thread count"
    path = os.path.join(HERE, G28_FILE)
    with open(path, "w") as fh:
        json.dump(got, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"wrote {path}: {len(got)} cases, {sum(len(v) for v in got.values())} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
