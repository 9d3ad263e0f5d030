"""Sampled tactic generation, host side: the sampler's uniform (``rp_sample_uniform``), the reference sampler's kept sets
against HuggingFace's logits warpers (G24), ``sample_search_batch`` over the fp32 CPU decoder step with the reference
sampler standing in for the kernel, and the tactic generators' ``do_sample`` layer over a stub engine."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import T5Fp32, source_ids  # noqa: E402
from sample_helpers import GRID, CpuSampler, kernel_case, margin_bound, reference_sample  # noqa: E402
from reprover_amd import synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.generation import BeamSearchOutput, sample_search, sample_search_batch  # noqa: E402
from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator  # noqa: E402
from reprover_amd.tokenizer import ByT5Tokenizer  # noqa: E402


# ---- the uniform -----------------------------------------------------------------------------------------------------------
def test_uniform_range_grid_and_bins(hip_lib):
    for seed in (0, 1, 0xDEADBEEF):
        u = np.array([hip_lib.rp_sample_uniform(seed, s, p) for s in range(64) for p in range(1024)], dtype=np.float64)
        assert u.size == 65536 and (u >= 0).all() and (u < 1).all()
        assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))  # multiples of 2^-24
        counts = np.bincount((u * 16).astype(int), minlength=16)
        sigma = np.sqrt(65536 * (1 / 16) * (15 / 16))
        assert np.abs(counts - 4096).max() <= 5 * sigma, counts


def test_uniform_depends_on_seed_sample_and_position(hip_lib):
    f = hip_lib.rp_sample_uniform
    base = f(7, 3, 11)
    assert f(7, 3, 11) == base
    assert f(8, 3, 11) != base and f(7, 4, 11) != base and f(7, 3, 12) != base
    # neighbouring seeds do not give shifted copies of one stream
    a = np.array([f(0, 0, p) for p in range(256)])
    for other in (np.array([f(1, 0, p) for p in range(256)]), np.array([f(0, 1, p) for p in range(256)])):
        assert len(np.intersect1d(a, other)) <= 2


# ---- kept sets against HuggingFace's warpers ---------------------------------------------------------------------------
def test_reference_kept_sets_equal_hf_warpers(golden_dir):
    """Rows without ties: the same mask.  Rows with ties: HF leaves the order of equal probabilities to its sort, so a
    top-p boundary inside a tie group may keep other members of the group: the kept VALUES are the same multiset.  Rows
    whose decision margins are inside the fp32 bound are left out, at most 10 % per case."""
    z = np.load(os.path.join(golden_dir, "g24_sample_warp.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    assert [tuple(g) for g in meta["grid"]] == GRID
    nrand = meta["random_rows"]
    for V in meta["vocabs"]:
        lp = z[f"v{V}_lp"]
        R = lp.shape[0]
        want = np.unpackbits(z[f"v{V}_kept"], axis=-1)[..., :V].astype(bool)
        u = np.full(R, 0.5, dtype=np.float32)
        for gi, (T, k, p) in enumerate(GRID):
            k = V if k == "vocab" else k
            _, kept, _, margins = reference_sample(lp, u, T, k, p)  # the draw's margin does not bear on the kept set
            ok = margins > margin_bound(V)
            assert (~ok).sum() <= 0.1 * R, (V, T, k, p, int((~ok).sum()))
            for r in np.nonzero(ok)[0]:
                if r < nrand and len(np.unique(lp[r])) == V:
                    assert np.array_equal(kept[r], want[gi, r]), (V, T, k, p, r)
                else:
                    assert np.array_equal(np.sort(lp[r][kept[r]]), np.sort(lp[r][want[gi, r]])), (V, T, k, p, r)
            assert kept.any(1).all()


def test_reference_tie_rules():
    lp = np.log(np.array([[0.25, 0.25, 0.25, 0.25], [0.1, 0.4, 0.4, 0.1]], dtype=np.float32))
    u = np.zeros(2, dtype=np.float32)
    # top-k: ties with the k-th stay
    assert reference_sample(lp, u, 1.0, 1, 1.0)[1].tolist() == [[True] * 4, [False, True, True, False]]
    # top-p: equal probabilities are dropped from the highest id down
    assert reference_sample(lp, u, 1.0, 0, 0.5)[1][0].tolist() == [True, True, False, False]
    assert reference_sample(lp, u, 1.0, 0, 0.3)[1][1].tolist() == [False, True, False, False]
    # the draw walks ascending ids
    toks = [int(reference_sample(lp[:1], np.array([x], dtype=np.float32), 1.0, 0, 1.0)[0][0]) for x in (0.0, 0.3, 0.6, 0.99)]
    assert toks == [0, 1, 2, 3]


@pytest.mark.parametrize("rows", [1, 64, 1024])
@pytest.mark.parametrize("V", [1, 3, 384, 512])
def test_kernel_test_inputs_stay_inside_the_skip_cap(hip_lib, V, rows):
    """The GPU kernel test's inputs (every shape, the same rows and uniforms), judged by the reference alone: at most
    10 % of the rows of any grid point are left out."""
    lp, _, _, _, _, u = kernel_case(hip_lib, V, rows)
    for T, k, p in GRID:
        _, _, margins, _ = reference_sample(lp, u, T, V if k == "vocab" else k, p)
        assert (margins <= margin_bound(V)).sum() <= 0.1 * rows, (V, rows, T, k, p)


# ---- the loop ---------------------------------------------------------------------------------------------------------------
class ManyRef:
    """``sample_search_batch``'s ``step_many`` over one fp32 reference decoder (and cache) per state."""

    def __init__(self, cfg, sd, encs, nb, max_len):
        self.nb = nb
        self.refs = [T5Fp32(cfg, sd) for _ in encs]
        for r, e in zip(self.refs, encs):
            r.start(e, nb, max_len)
        self.calls = []

    def step_many(self, active, tokens, ancestry, t):
        nb = self.nb
        assert list(active) == sorted(set(active)) and tokens.shape[0] == ancestry.shape[0] == len(active) * nb
        assert all(int(ancestry[r, p]) == p * nb + r % nb for r in (0, len(active) * nb - 1) for p in (0, t))
        self.calls.append(list(active))
        return torch.cat([self.refs[i].step(tokens[a * nb : (a + 1) * nb].long(), ancestry[a * nb : (a + 1) * nb, : t + 1].long())
                          for a, i in enumerate(active)])


@pytest.fixture(scope="module")
def setup():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= 4.0  # EOS boosted: some samples stop early, one state long before the others
    ref = T5Fp32(cfg, sd)
    srcs = [source_ids(60, 3), source_ids(7, 4), source_ids(33, 5)]
    return cfg, sd, [ref.encode(s) for s in srcs]


def _run(hip_lib, cfg, sd, encs, seeds, nb, ml, sync_every=16, lp=0.0, **kw):
    many = ManyRef(cfg, sd, encs, nb, ml)
    sampler = CpuSampler(hip_lib, **kw)
    outs = sample_search_batch(many.step_many, sampler, len(encs), nb, ml, seeds, lp, sync_every=sync_every)
    return outs, many, sampler


def _same(a: BeamSearchOutput, b: BeamSearchOutput):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)


def test_loop_eos_padding_trim_and_score(hip_lib, setup):
    cfg, sd, encs = setup
    nb, ml = 6, 24
    outs, many, _ = _run(hip_lib, cfg, sd, encs, [11, 12, 13], nb, ml, sync_every=4, lp=0.0, temperature=1.0)
    stopped_early = 0
    for i, o in enumerate(outs):
        seq = o.sequences
        assert seq.dtype == torch.int64 and seq.shape[0] == nb and 2 <= seq.shape[1] <= ml and (seq[:, 0] == 0).all()
        lens = []
        for b in range(nb):
            row = seq[b, 1:].tolist()
            n = row.index(1) + 1 if 1 in row else len(row)
            assert all(x == 0 for x in row[n:])  # pad after EOS
            assert 1 in row or n == ml - 1 or n == seq.shape[1] - 1
            lens.append(n)
            # the score is the sum of the model's log-probs of the drawn tokens: replay the row alone
            ref = T5Fp32(cfg, sd)
            ref.start(encs[i], 1, ml)
            tot = np.float32(0)
            for t in range(n):
                lp_row = ref.step(seq[b, t : t + 1], torch.arange(t + 1)[None])[0]
                tot = np.float32(tot + np.float32(lp_row[seq[b, t + 1]]))
            assert abs(float(o.sequences_scores[b]) - float(tot)) <= 1e-4 * max(1.0, abs(float(tot)))
        assert seq.shape[1] == 1 + max(lens)  # trimmed to the longest
        stopped_early += sum(n < ml - 1 for n in lens)
    assert stopped_early > 0
    assert many.calls[3] == [0, 1, 2] and many.calls[4] == [0, 2]  # state 1 left at the first look, finished rows were fed pad until then
    # length_penalty: the finished-beam formula over the same tokens
    outs2, _, _ = _run(hip_lib, cfg, sd, encs, [11, 12, 13], nb, ml, sync_every=4, lp=1.0, temperature=1.0)
    for o, o2 in zip(outs, outs2):
        assert torch.equal(o.sequences, o2.sequences)
        n = (o.sequences[:, 1:] != 0).sum(1).float()
        n = torch.where((o.sequences[:, 1:] == 1).any(1), n, torch.full_like(n, o.sequences.shape[1] - 1.0))
        assert torch.allclose(o2.sequences_scores, o.sequences_scores / n, rtol=1e-6, atol=0)


def test_loop_max_length_stop(hip_lib, setup):
    cfg, sd, encs = setup
    outs, many, _ = _run(hip_lib, cfg, sd, encs[:1], [5], 3, 4, temperature=0.7, top_k=5)
    assert outs[0].sequences.shape[1] <= 4 and len(many.calls) <= 3
    with pytest.raises(ValueError):
        sample_search_batch(None, None, 1, 2, 1, [0])
    with pytest.raises(ValueError):
        sample_search_batch(None, None, 2, 2, 8, [0])


def test_batch_equals_alone_in_any_order_for_any_sync_interval(hip_lib, setup):
    cfg, sd, encs = setup
    nb, ml, kw = 4, 20, dict(temperature=1.2, top_k=50, top_p=0.95)
    seeds = [21, 22, 23]
    alone = []
    for e, s in zip(encs, seeds):
        ref = T5Fp32(cfg, sd)
        ref.start(e, nb, ml)
        alone.append(sample_search(lambda tok, anc, t: ref.step(tok.long(), anc[:, : t + 1].long()), CpuSampler(hip_lib, **kw),
                                   nb, ml, s))
    calls = {}
    for sync_every in (1, 16, 64):
        outs, many, _ = _run(hip_lib, cfg, sd, encs, seeds, nb, ml, sync_every=sync_every, **kw)
        calls[sync_every] = many.calls
        for o, a in zip(outs, alone):
            _same(o, a)
    assert len(set(o.sequences.shape[1] for o in alone)) > 1  # the states stop at different positions
    assert len(calls[1][-1]) < len(encs)  # sync_every = 1: the early finishers left the list
    assert all(len(c) == len(encs) for c in calls[64])  # never looked: all states stepped to the end
    perm = [2, 0, 1, 2]
    outs, _, _ = _run(hip_lib, cfg, sd, [encs[i] for i in perm], [seeds[i] for i in perm], nb, ml, sync_every=3, **kw)
    for o, i in zip(outs, perm):
        _same(o, alone[i])
    # another seed gives other samples
    other, _, _ = _run(hip_lib, cfg, sd, encs[:1], [99], nb, ml, **kw)
    assert not torch.equal(other[0].sequences, alone[0].sequences)


# ---- the tactic generators ---------------------------------------------------------------------------------------------
class StubEngine:
    """Records the calls of a ``HipT5Generator``; ``sample_many`` answers from the seeds alone."""

    class decoder:  # noqa: N801
        @staticmethod
        def max_states(nb):
            return 2

    def __init__(self):
        self.calls = []

    @staticmethod
    def _beams():
        return BeamSearchOutput(torch.tensor([[0, 100, 1], [0, 101, 1]]), torch.tensor([-1.0, -2.0]))

    def generate(self, *a):
        self.calls.append(("generate", a))
        return self._beams()

    def generate_many(self, ids, *a):
        self.calls.append(("generate_many", a))
        return [self._beams()] * len(ids)

    def sample_many(self, sources, num_samples, max_length, temperature, top_k, top_p, seeds, length_penalty):
        self.calls.append(("sample_many", (len(sources), num_samples, max_length, temperature, top_k, top_p, list(seeds),
                                           length_penalty)))
        outs = []
        for s in seeds:
            toks = [100 + (s >> (4 * j)) % 3 for j in range(num_samples)]
            scores = [-float((s >> (3 * j)) % 5) for j in range(num_samples)]
            outs.append(BeamSearchOutput(torch.tensor([[0, t, 1] for t in toks]), torch.tensor(scores)))
        return outs


def _gen(**kw):
    g = HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, **kw)
    g.generator, g.tokenizer = StubEngine(), ByT5Tokenizer()
    return g


POS = Pos(1, 1)


def test_defaults_leave_the_beam_search_call_untouched():
    g = _gen()
    out = g.generate_sync("a b", "f", "t", POS, 2)
    (name, args), = g.generator.calls
    assert name == "generate" and args[1:] == (2, 16, 0.0) and out == [("a", -1.0), ("b", -2.0)]
    g.batch_generate_sync(["a", "b", "c"], ["f"] * 3, ["t"] * 3, [POS] * 3, 2)
    assert [c[0] for c in g.generator.calls[1:]] == ["generate_many", "generate_many"]
    assert g.states_served == 0


def test_do_sample_sorts_dedups_and_counts_states():
    g = _gen(do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=3)
    a1 = g.generate_sync("s", "f", "t", POS, 4)
    a2 = g.generate_sync("s", "f", "t", POS, 4)
    name, args = g.generator.calls[0]
    assert name == "sample_many" and args[:6] == (1, 4, 16, 0.8, 40, 0.95) and args[7] == 0.0
    seeds = [c[1][6][0] for c in g.generator.calls]
    assert seeds[0] != seeds[1] and all(0 <= s < 2 ** 32 for s in seeds) and g.states_served == 2
    for res in (a1, a2):
        scores = [s for _, s in res]
        assert scores == sorted(scores, reverse=True) and len(set(t for t, _ in res)) == len(res) >= 1
    # a batch serves its states from the same counter values as single calls, across the engine's cap of 2 states
    h = _gen(do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=3)
    batch = h.batch_generate_sync(["s", "s", "s"], ["f"] * 3, ["t"] * 3, [POS] * 3, 4)
    assert batch[:2] == [a1, a2] and [c[1][0] for c in h.generator.calls] == [2, 1]
    assert [s for c in h.generator.calls for s in c[1][6]][:2] == seeds and h.states_served == 3
    assert _gen(do_sample=True, seed=4).generate_sync("s", "f", "t", POS, 4) is not None
    assert _gen(do_sample=True, seed=4)._next_seeds(1) != _gen(do_sample=True, seed=3)._next_seeds(1)


def test_bad_sampling_parameters_raise():
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_p=0.0),
               dict(top_p=1.5), dict(top_k=-1), dict(top_k=2.5)):
        with pytest.raises(ValueError):
            HuggingFaceGenerator("unused", "cpu", 64, 16, 0.0, do_sample=True, **kw)
        with pytest.raises(ValueError):
            RetrievalAugmentedGenerator("g", "r", "c", "cpu", 64, 16, 0.0, 10, do_sample=True, **kw)
