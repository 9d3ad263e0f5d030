"""Batched beam-search drivers, host side: ``beam_search_batch`` / ``greedy_search_batch`` over the fp32 CPU decoder step
(tests/gen_helpers.py) return, per source, exactly what ``beam_search`` / ``greedy_search`` return for it alone: on every
G20 grid point, with states that stop at different steps, for one state, identical states and a permuted batch."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.generation import beam_search, beam_search_batch, greedy_search, greedy_search_batch  # noqa: E402


def batch_sources(src):
    """The G20 source, two truncations of it (EOS re-appended) and two seeded sources of other lengths."""
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    return [np.asarray(src, dtype=np.int32), cut(40), cut(7), source_ids(120, 11), source_ids(33, 12)]


class ManyRef:
    """``step_many`` over one fp32 reference decoder (and cache) per state."""

    def __init__(self, cfg, sd, encs, nb, max_len):
        self.nb = nb
        self.refs = [T5Fp32(cfg, sd) for _ in encs]
        for r, e in zip(self.refs, encs):
            r.start(e, nb, max_len)
        self.calls = []

    def step_many(self, active, tokens, ancestry):
        nb = self.nb
        assert list(active) == sorted(set(active)) and tokens.shape[0] == ancestry.shape[0] == len(active) * nb
        self.calls.append(list(active))
        return torch.cat([self.refs[i].step(tokens[a * nb : (a + 1) * nb], ancestry[a * nb : (a + 1) * nb])
                          for a, i in enumerate(active)])


@pytest.fixture(scope="module")
def setup(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    ref = T5Fp32(cfg, sd)
    srcs = batch_sources(z["src"])
    return z, meta, cfg, sd, ref, [ref.encode(s) for s in srcs]


def _alone(ref, enc, nb, ml, lp):
    ref.start(enc, nb, ml)
    trace = []
    return beam_search(ref.step, nb, ml, lp, trace=trace), trace


def _same(out, trace, ref_out, ref_trace):
    assert torch.equal(out.sequences, ref_out.sequences)
    assert torch.equal(out.sequences_scores, ref_out.sequences_scores)  # the same bits, not a tolerance
    assert len(trace) == len(ref_trace)
    for got, want in zip(trace, ref_trace):
        assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", range(24))
def test_batched_driver_equals_beam_search_on_the_g20_grid(setup, case):
    z, meta, cfg, sd, ref, encs = setup
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    many = ManyRef(cfg, sd, encs, nb, ml)
    traces = []
    outs = beam_search_batch(many.step_many, len(encs), nb, ml, lp, traces=traces)
    assert len(outs) == len(traces) == len(encs)
    for i, enc in enumerate(encs):
        _same(outs[i], traces[i], *_alone(ref, enc, nb, ml, lp))
    # entry 0 is the G20 source: the committed HuggingFace sequences and step count
    assert np.array_equal(outs[0].sequences.numpy(), z[f"c{case}_seq"])
    assert len(traces[0]) == c["steps"]
    # a state is in the active list exactly for the steps its own search runs
    for i in range(len(encs)):
        assert sum(i in act for act in many.calls) == len(traces[i])
    assert len(many.calls) == max(len(t) for t in traces)


@pytest.mark.parametrize("nb,lp,ml", [(4, 0.0, 64), (8, 0.0, 64), (1, 0.0, 20)])
def test_states_stop_at_different_steps(setup, nb, lp, ml):
    """The early-exit path: the states of one batch stop at different steps, one of them at least 3 steps before the
    last, and every one still equals its own search."""
    z, meta, cfg, sd, ref, encs = setup
    many = ManyRef(cfg, sd, encs, nb, ml)
    traces = []
    outs = beam_search_batch(many.step_many, len(encs), nb, ml, lp, traces=traces)
    stops = [len(t) for t in traces]
    assert len(set(stops)) > 1 and min(stops) <= max(stops) - 3, stops
    assert [len(a) for a in many.calls][-1] < len(encs)  # the last step ran fewer states than the first
    for i, enc in enumerate(encs):
        _same(outs[i], traces[i], *_alone(ref, enc, nb, ml, lp))


def test_one_state_identical_states_and_permutation(setup):
    z, meta, cfg, sd, ref, encs = setup
    nb, lp, ml = 4, 0.0, 64
    alone = [_alone(ref, e, nb, ml, lp) for e in encs]
    # B = 1
    for i in (0, 2):
        tr = []
        out = beam_search_batch(ManyRef(cfg, sd, [encs[i]], nb, ml).step_many, 1, nb, ml, lp, traces=tr)
        _same(out[0], tr[0], *alone[i])
    # identical sources
    tr = []
    outs = beam_search_batch(ManyRef(cfg, sd, [encs[2]] * 3, nb, ml).step_many, 3, nb, ml, lp, traces=tr)
    for o, t in zip(outs, tr):
        _same(o, t, *alone[2])
    # a permuted batch, one state twice
    perm = [4, 2, 0, 3, 2, 1]
    tr = []
    outs = beam_search_batch(ManyRef(cfg, sd, [encs[i] for i in perm], nb, ml).step_many, len(perm), nb, ml, lp, traces=tr)
    for o, t, i in zip(outs, tr, perm):
        _same(o, t, *alone[i])


def test_num_return_sequences_and_max_length_one(setup):
    z, meta, cfg, sd, ref, encs = setup
    outs = beam_search_batch(ManyRef(cfg, sd, encs[:2], 4, 12).step_many, 2, 4, 12, 1.0, num_return_sequences=2)
    for i, o in enumerate(outs):
        ref.start(encs[i], 4, 12)
        want = beam_search(ref.step, 4, 12, 1.0, num_return_sequences=2)
        assert torch.equal(o.sequences, want.sequences) and torch.equal(o.sequences_scores, want.sequences_scores)
    with pytest.raises(ValueError):
        beam_search_batch(lambda a, t, c: torch.zeros(len(t), 384), 2, 4, 1)
    with pytest.raises(ValueError):
        greedy_search_batch(lambda a, t, c: torch.zeros(len(t), 384), 2, 1)


@pytest.mark.parametrize("ml", [6, 40])
def test_greedy_batch_equals_greedy_search(setup, ml):
    z, meta, cfg, sd, ref, encs = setup
    many = ManyRef(cfg, sd, encs, 1, ml)
    outs = greedy_search_batch(many.step_many, len(encs), ml)
    lens = []
    for i, enc in enumerate(encs):
        ref.start(enc, 1, ml)
        want = greedy_search(ref.step, ml)
        assert torch.equal(outs[i].sequences, want.sequences)
        assert torch.equal(outs[i].sequences_scores, want.sequences_scores)
        lens.append(want.sequences.shape[1])
    assert len(many.calls) == max(lens) - 1
    if ml == 40:  # EOS at different steps: the early finishers leave the list
        assert min(lens) <= max(lens) - 3, lens
        assert len(many.calls[-1]) < len(encs)
