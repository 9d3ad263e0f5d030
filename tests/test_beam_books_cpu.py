"""Beam search with device books, host side (no GPU): ``beam_advance_host`` - the restatement of ``rp_beam_advance`` with
the stated stable order - against ``_BeamState`` on scripted triples, its tie rule against hand-written expectations,
planted mutants, and ``beam_search_batch_device`` over it against ``beam_search_batch`` on the G20 grid."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.generation import (NEG, BeamBooks, _BeamState, beam_advance_host, beam_books_bytes,  # noqa: E402
                                     beam_books_init_host, beam_search_batch, beam_search_batch_device,
                                     topk_select_many)

EOS, START = 1, 0


# ---- a toy model: log-probs that depend on (seed, state, position, the row's token) alone ----------------------------------
class Toy:
    """``step_many`` of both loops over seeded log-probs; ``eos_boost[i]`` is added to state ``i``'s EOS logit from
    position ``eos_from[i]`` on, so that the states of one call stop at different steps."""

    def __init__(self, seed, nb, eos_boost, eos_from, vocab=None):
        self.seed, self.nb, self.eos_boost, self.eos_from = seed, nb, eos_boost, eos_from
        self.V = vocab or 2 * nb + 5
        self.calls = []

    def rows(self, active, tokens, t):
        out = []
        for a, i in enumerate(active):
            for b in range(self.nb):
                tok = int(tokens[a * self.nb + b])
                g = torch.Generator().manual_seed(((self.seed * 64 + i) * 64 + t) * 1024 + tok)
                logits = torch.randn(self.V, generator=g) * 2.0
                if t >= self.eos_from[i]:
                    logits[EOS] += self.eos_boost[i]
                out.append(torch.log_softmax(logits, -1))
        return torch.stack(out)

    def host(self, active, tokens, ancestry):  # beam_search_batch's protocol: the position is the table's last column
        self.calls.append(list(active))
        return self.rows(active, tokens, ancestry.shape[1] - 1)

    def device(self, active, tokens, ancestry, t):  # beam_search_batch_device's
        self.calls.append(list(active))
        return self.rows(active, tokens, t)


def _toy(seed, nb):
    return Toy(seed, nb, eos_boost=(6.0, -4.0, 9.0), eos_from=(2, 0, 0))


def _divs(t, lp):
    """The two divisors as ``_BeamState.advance`` writes them (generation.py:110 and :126), at position t."""
    prompt_len, cur_len = 1, t + 1
    fin_div = float((cur_len + 1 - prompt_len) ** lp)
    cur_len = cur_len + 1
    run_div = float((cur_len - prompt_len) ** lp)
    return fin_div, run_div


def test_divisors_are_the_reference_expressions():
    for lp in (0.0, 1.0, 0.7, 2.0, 1):
        for t in range(20):
            assert _divs(t, lp) == (float((t + 1) ** lp), float((t + 1) ** lp))


def _same_out(got, want):
    assert torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.sequences_scores.view(torch.int32), want.sequences_scores.view(torch.int32))  # bits


def _live_distinct(vals):
    live = vals[vals > NEG / 2]
    return len(set(live.tolist())) == len(live)


def _replay(trace, nb, ml, lp, fields=True):
    """Feed one state's scripted triples to a ``_BeamState`` and to the restatement (one state, slot 0); compare the live
    book fields after every step; return (restatement's result, reference result, restatement's stop step)."""
    ref = _BeamState(nb, ml, lp, EOS, START, None)
    bk = beam_books_init_host(1, nb, ml, EOS, START)
    stop = None
    for t, (vals, toks, pars) in enumerate(trace):
        ref.inputs()
        ref_done = ref.advance(vals, toks, pars)
        beam_advance_host(bk, [0], t, vals[None], toks[None], pars[None], *_divs(t, lp), EOS)
        assert int(bk.steps[0]) == t + 1
        cur = (t + 1) & 1
        assert bool(bk.done[0]) == ref_done and bool(bk.heur[0]) == ref.heuristic_unsatisfied, t
        if fields and _live_distinct(vals):
            live = ref.running_scores > NEG / 2
            assert torch.equal(bk.run_scores[0][live].view(torch.int32), ref.running_scores[live].view(torch.int32))
            assert torch.equal(bk.run_seq[cur, 0][live].long(), ref.running_seq[live])
            assert torch.equal(bk.anc[cur, 0][live, : t + 1].long(), ref.ancestry[live])
            assert torch.equal(bk.tokens[:nb][live].long(), ref.running_seq[live, t + 1])
            fin = ref.is_sent_finished
            assert torch.equal(bk.fin_flag[0].bool(), fin)
            assert torch.equal(bk.beam_scores[0][fin].view(torch.int32), ref.beam_scores[fin].view(torch.int32))
            assert torch.equal(bk.fin_seq[cur, 0][fin].long(), ref.sequences[fin])
            assert torch.equal(bk.fin_len[0][fin].long(), ((ref.beam_indices + 1).bool()).sum(1)[fin])
        if ref_done:
            stop = t + 1
            break
    assert stop == len(trace)  # the script ends where the reference stops
    return bk.result(0), ref.result(), stop


# ---- the restatement against _BeamState ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 3, 8])
@pytest.mark.parametrize("ml", [2, 3, 17])
def test_restatement_equals_beam_state_on_seeded_scripts(nb, ml):
    stops = set()
    for lp in (0.0, 1.0, 0.7, 2.0):
        for seed in (1, 2):
            toy = _toy(seed, nb)
            traces = []
            outs = beam_search_batch(toy.host, 3, nb, ml, lp, EOS, START, traces=traces)
            for i in range(3):
                assert all(_live_distinct(v) for v, _, _ in traces[i])  # the scripts hold no live ties
                got, want, stop = _replay(traces[i], nb, ml, lp)
                _same_out(got, want)
                _same_out(got, outs[i])
                stops.add(stop)
    if ml == 17:
        assert min(stops) < 16, stops  # some script stops by the heuristic
        assert 16 in stops, stops      # and some at max_length
        assert len(stops) >= 3, stops


class ManyRef:
    """``step_many`` over one fp32 reference decoder (and cache) per state (tests/gen_helpers.py)."""

    def __init__(self, cfg, sd, encs, nb, max_len):
        self.nb = nb
        self.refs = [T5Fp32(cfg, sd) for _ in encs]
        for r, e in zip(self.refs, encs):
            r.start(e, nb, max_len)
        self.calls = []

    def host(self, active, tokens, ancestry):
        nb = self.nb
        self.calls.append(list(active))
        return torch.cat([self.refs[i].step(tokens[a * nb : (a + 1) * nb].long(), ancestry[a * nb : (a + 1) * nb].long())
                          for a, i in enumerate(active)])

    def device(self, active, tokens, ancestry, t):
        return self.host(active, tokens, ancestry[:, : t + 1])


@pytest.fixture(scope="module")
def g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    ref = T5Fp32(cfg, sd)
    src = z["src"]
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    srcs = [np.asarray(src, dtype=np.int32), cut(7), source_ids(33, 12)]
    return z, meta, cfg, sd, [ref.encode(s) for s in srcs]


def _device_loop(many, n, nb, ml, lp, k, advance=beam_advance_host, counter=None):
    def to_host(x):
        if counter is not None:
            counter.append(x.numel())
        return x.cpu()

    return beam_search_batch_device(many.device, topk_select_many, advance, n, nb, ml, lp, EOS, START, sync_every=k,
                                    to_host=to_host)


@pytest.mark.parametrize("case", range(24))
def test_device_loop_over_the_restatement_equals_beam_search_batch_on_the_g20_grid(g20, case):
    """The 24 G20 grid points through the fp32 model, three states that stop at different steps: the reference loop's
    traces replayed into the restatement give its results, and the new loop gives them for sync_every 1, 3 and 1000."""
    z, meta, cfg, sd, encs = g20
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    traces = []
    want = beam_search_batch(ManyRef(cfg, sd, encs, nb, ml).host, len(encs), nb, ml, lp, traces=traces)
    assert np.array_equal(want[0].sequences.numpy(), z[f"c{case}_seq"]) and len(traces[0]) == c["steps"]
    for i in range(len(encs)):
        got, ref_out, _ = _replay(traces[i], nb, ml, lp)
        _same_out(got, ref_out)
        _same_out(got, want[i])
    longest = max(len(t) for t in traces)
    for k in (1, 3, 1000):
        many = ManyRef(cfg, sd, encs, nb, ml)
        reads = []
        outs = _device_loop(many, len(encs), nb, ml, lp, k, counter=reads)
        for o, w in zip(outs, want):
            _same_out(o, w)
        steps = len(many.calls)
        assert steps >= longest and (k > 1 or steps == longest)  # sync_every = 1 stops where the host loop stops
        assert len(reads) <= -(-steps // k) + 1, (reads, steps, k)
        if k == 1:  # a state is stepped exactly as long as its own search runs
            for i in range(len(encs)):
                assert sum(i in act for act in many.calls) == len(traces[i])


def test_device_loop_arguments():
    toy = _toy(1, 2)
    with pytest.raises(ValueError):
        beam_search_batch_device(toy.device, topk_select_many, beam_advance_host, 3, 2, 1)
    with pytest.raises(ValueError):
        beam_search_batch_device(toy.device, topk_select_many, beam_advance_host, 3, 2, 8, sync_every=0)
    outs = beam_search_batch_device(toy.device, topk_select_many, beam_advance_host, 3, 2, 8, 1.0, num_return_sequences=1)
    want = beam_search_batch(_toy(1, 2).host, 3, 2, 8, 1.0, num_return_sequences=1)
    for o, w in zip(outs, want):
        _same_out(o, w)
    assert BeamBooks(3, 2, 8).nbytes == beam_books_bytes(3, 2, 8) and beam_books_bytes(3, 2, 8) % 16 == 0


# ---- the tie rule: hand-written expectations -------------------------------------------------------------------------------
def _f(*v):
    return torch.tensor(v, dtype=torch.float32)


def _i(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_tie_rule_running_ties_go_to_the_lower_index_and_kept_hypotheses_come_first():
    """nb = 2, position 0: the two best candidates tie at -1, the next two at -2; no EOS.  The running beams are
    candidates 0 and 1 in that order.  Every finished score is -1e9 exactly (-1 - 1e9 rounds to -1e9), tying with the two
    kept entries: the kept ones stay, so no generated length appears."""
    bk = beam_books_init_host(1, 2, 8, EOS, START)
    beam_advance_host(bk, [0], 0, _f(-1.0, -1.0, -2.0, -2.0)[None], _i(5, 6, 7, 8)[None], _i(0, 0, 0, 0)[None], 1.0, 1.0, EOS)
    assert bk.run_seq[1, 0, :, :3].tolist() == [[0, 5, 1], [0, 6, 1]]
    assert bk.run_scores[0].tolist() == [-1.0, -1.0] and bk.tokens[:2].tolist() == [5, 6]
    assert bk.anc[1, 0, :, :2].tolist() == [[0, 2], [0, 3]] and bk.anc_rows[:2, :2].tolist() == [[0, 2], [0, 3]]
    assert bk.beam_scores[0].tolist() == [NEG, NEG] and bk.fin_len[0].tolist() == [0, 0]
    assert bk.fin_flag[0].tolist() == [0, 0] and bk.fin_seq[1, 0, :, :2].tolist() == [[0, 1], [0, 1]]
    assert (int(bk.heur[0]), int(bk.done[0]), int(bk.steps[0])) == (1, 0, 1)


def test_tie_rule_signed_zeros_tie():
    """-0.0 and +0.0 are equal scores: candidate 0 (-0.0) stays ahead of candidate 1 (+0.0)."""
    bk = beam_books_init_host(1, 2, 8, EOS, START)
    beam_advance_host(bk, [0], 0, _f(-0.0, 0.0, -2.0, -2.0)[None], _i(5, 6, 7, 8)[None], _i(0, 0, 0, 0)[None], 1.0, 1.0, EOS)
    assert bk.tokens[:2].tolist() == [5, 6]
    assert bk.run_scores[0].view(torch.int32).tolist() == [-2 ** 31, 0]  # -0.0 + -0.0 = -0.0; +0.0 + -0.0 = +0.0


def test_tie_rule_finished_ties_keep_candidate_order():
    """nb = 2, length_penalty 1.  Position 0 keeps tokens 5 and 6.  At position 1 candidates 0 and 1 are EOS with the same
    score -2, from parents 1 and 0: the finished hypotheses are [0, 6, 1] then [0, 5, 1], both -2 / 2 = -1.  The best
    running score is -5 / 2 = -2.5, not above the worst finished -1: the heuristic stops the search."""
    bk = beam_books_init_host(1, 2, 8, EOS, START)
    beam_advance_host(bk, [0], 0, _f(-1.0, -1.5, -2.0, -2.5)[None], _i(5, 6, 7, 8)[None], _i(0, 0, 0, 0)[None], 1.0, 1.0, EOS)
    beam_advance_host(bk, [0], 1, _f(-2.0, -2.0, -5.0, -6.0)[None], _i(1, 1, 7, 8)[None], _i(1, 0, 0, 1)[None], 2.0, 2.0, EOS)
    assert bk.fin_seq[0, 0, :, :3].tolist() == [[0, 6, 1], [0, 5, 1]]
    assert bk.beam_scores[0].tolist() == [-1.0, -1.0] and bk.fin_flag[0].tolist() == [1, 1]
    assert bk.fin_len[0].tolist() == [2, 2]
    assert bk.run_seq[0, 0, :, :3].tolist() == [[0, 5, 7], [0, 6, 8]] and bk.run_scores[0].tolist() == [-5.0, -6.0]
    assert (int(bk.heur[0]), int(bk.done[0]), int(bk.steps[0])) == (0, 1, 2)
    out = bk.result(0)
    assert out.sequences.tolist() == [[0, 6, 1], [0, 5, 1]] and out.sequences_scores.tolist() == [-1.0, -1.0]
    # a stopped state is frozen: further triples change nothing
    before = bk.block.clone()
    beam_advance_host(bk, [0], 2, _f(-0.1, -0.2, -0.3, -0.4)[None], _i(9, 1, 9, 9)[None], _i(1, 1, 0, 0)[None], 3.0, 3.0, EOS)
    assert torch.equal(bk.block, before)


# ---- planted mutants of the restatement: each changes a result on a named case ---------------------------------------------
def _differs(outs, want):
    return any(not torch.equal(o.sequences, w.sequences) or not torch.equal(o.sequences_scores, w.sequences_scores)
               for o, w in zip(outs, want))


def _toy_case(seed, nb, ml, lp, k, advance):
    want = beam_search_batch(_toy(seed, nb).host, 3, nb, ml, lp, EOS, START)
    base = _device_loop(_toy(seed, nb), 3, nb, ml, lp, k)
    assert not _differs(base, want)  # the unmutated restatement passes the same case
    return _differs(_device_loop(_toy(seed, nb), 3, nb, ml, lp, k, advance=advance), want)


def _mutant(name):
    return lambda *a: beam_advance_host(*a, mutant=name)


def test_mutant_late_candidates_finish_changes_a_result():
    """Toy case (seed 2, nb 3, max_length 17, length_penalty 0.0), sync_every 1."""
    assert _toy_case(2, 3, 17, 0.0, 1, advance=_mutant("late_candidates_finish"))


def test_mutants_not_frozen_and_not_sticky_change_a_result_together_and_guard_each_other():
    """Toy case (seed 1, nb 3, max_length 17, length_penalty 2.0), sync_every 1000, so that stopped states are fed on.

    Neither mutant can change ``result()`` alone, by the reference's own construction: a state stops at the step its
    heuristic flag drops, so a frozen state never evaluates the flag again (stickiness is never exercised), and a state
    that is fed on with the flag down adds -1e9 to every new finished score, so its hypotheses stay (the freeze protects
    only the rest of the books).  Together they let a stopped state take new hypotheses: the result changes.  The
    freeze alone is seen in the books: without it a stopped state's block changes under further triples."""
    case = (1, 3, 17, 2.0, 1000)
    assert _toy_case(*case, advance=_mutant("done_not_frozen+heuristic_not_sticky"))
    assert not _toy_case(*case, advance=_mutant("done_not_frozen"))
    assert not _toy_case(*case, advance=_mutant("heuristic_not_sticky"))
    bk = beam_books_init_host(1, 2, 8, EOS, START)
    beam_advance_host(bk, [0], 0, _f(-1.0, -1.5, -2.0, -2.5)[None], _i(5, 6, 7, 8)[None], _i(0, 0, 0, 0)[None], 1.0, 1.0, EOS)
    beam_advance_host(bk, [0], 1, _f(-2.0, -2.0, -5.0, -6.0)[None], _i(1, 1, 7, 8)[None], _i(1, 0, 0, 1)[None], 2.0, 2.0, EOS)
    assert int(bk.done[0]) == 1
    before = bk.block.clone()
    more = (_f(-0.1, -0.2, -0.3, -0.4)[None], _i(9, 1, 9, 9)[None], _i(1, 1, 0, 0)[None], 3.0, 3.0, EOS)
    beam_advance_host(bk, [0], 2, *more)
    assert torch.equal(bk.block, before)
    beam_advance_host(bk, [0], 2, *more, mutant="done_not_frozen")
    assert not torch.equal(bk.block, before)


def test_mutant_fin_div_one_position_late_changes_a_result():
    """Toy case (seed 1, nb 3, max_length 17, length_penalty 1.0): the finished scores divided by (t + 2) ** lp."""
    lp = 1.0

    def late(books, active, t, vals, toks, pars, fin_div, run_div, eos):
        beam_advance_host(books, active, t, vals, toks, pars, float((t + 2) ** lp), run_div, eos)

    assert _toy_case(1, 3, 17, lp, 1, advance=late)


def test_mutant_ancestry_not_reordered_changes_a_result(g20):
    """G20 case 12 through the fp32 model: the ancestry rows not gathered by ``parents[nxt]`` feed the model another
    history."""
    z, meta, cfg, sd, encs = g20
    case = 12
    c = meta["cases"][case]
    nb, lp, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    assert nb > 1
    want = beam_search_batch(ManyRef(cfg, sd, encs, nb, ml).host, len(encs), nb, ml, lp)
    outs = _device_loop(ManyRef(cfg, sd, encs, nb, ml), len(encs), nb, ml, lp, 3, advance=_mutant("ancestry_not_reordered"))
    assert _differs(outs, want)
