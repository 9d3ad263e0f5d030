"""That the bars of tests/test_decoder_kernels_gpu.py mean something (no GPU): on the GPU tests' own shapes, with the rounded
float64 reference (tests/decoder_kernel_helpers.py) standing in for the kernel, every planted bug misses a bar the GPU test
applies, and the unmutated stand-in meets every one of them.  The bars are computed as the GPU test computes them: from the
two references alone."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_kernel_helpers as dk  # noqa: E402


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = dk.attention_case(name)
    exact, rounded = dk.attention_reference(c), dk.attention_reference(c, rounded=True)
    return c, exact, rounded, dk.attention_bounds(name, exact, rounded)


def test_bf16_round_is_torchs_cast():
    x = np.random.default_rng(0).standard_normal(4096) * np.exp(np.random.default_rng(1).uniform(-30, 30, 4096))
    x = np.concatenate([x, [0.0, -0.0, 1.00390625, 1.01171875, 3.3895e38]])  # ties to even, both ways; the largest bf16
    want = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)
    assert np.array_equal(dk.bf16_round(x), want)


def test_exact_reference_is_autograd():
    """The exact form against torch autograd in float64 on a small causal and a small cross call."""
    rng = np.random.default_rng(4)
    for causal, pairs in ((True, [(5, 5), (70, 70)]), (False, [(3, 9), (0, 4), (66, 2)])):
        c = dk.make_attention_case(rng, causal, 2, pairs, 33 if causal else 0, None, 0.6)
        ref = dk.attention_reference(c)
        q, k, v = (torch.from_numpy(c[n]).requires_grad_(True) for n in ("q", "k", "v"))
        tab = torch.from_numpy(c["tab"]).requires_grad_(True) if causal else None
        outs, qs, ks = [], 0, 0
        for Tq, Tk in pairs:
            if Tq:
                heads = []
                for h in range(2):
                    cs = slice(64 * h, 64 * h + 64)
                    s = q[qs : qs + Tq, cs] @ k[ks : ks + Tk, cs].T
                    if causal:
                        dist = torch.arange(Tq)[:, None] - torch.arange(Tk)[None]
                        s = (s + tab[h][dist.clamp(0, c["nbias"] - 1)]).masked_fill(dist < 0, -np.inf)
                    heads.append(torch.softmax(s, -1) @ v[ks : ks + Tk, cs])
                outs.append(torch.cat(heads, 1))
            qs, ks = qs + Tq, ks + Tk
        out = torch.cat(outs)
        (out * torch.from_numpy(c["d_o"])).sum().backward()
        for name, t in (("out", out.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
            assert np.abs(ref[name] - t.numpy()).max() <= 1e-11 * max(1.0, np.abs(t.numpy()).max()), name
        if causal:
            assert np.abs(ref["dtab"] - tab.grad.numpy().T).max() <= 1e-11
        assert np.abs(ref["delta"] - dk.delta_of(c["d_o"], ref["out"], 2)).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(dk.ATTENTION_CASES))
def test_rounded_reference_meets_every_attention_bar(name):
    c, exact, rounded, bounds = _refs(name)
    margins = {}
    assert dk.attention_findings(c, rounded, exact, bounds, margins) == []
    for t, (b2, bm) in bounds.items():
        print(f"{name} {t}: bounds rel L2 {b2:.3e}, worst row {bm:.3e}")
        assert 0 < b2 <= dk.DEC_KERNEL_TOL_CAP and 0 < bm <= dk.DEC_KERNEL_TOL_CAP, "no bar above test_attention_backward's"
    # sharp rows: the largest probability of a 300-key row is well above 1 / 300; the "big" cases reach scores of 30
    big = dk.ATTENTION_CASES[name][4] > 1.0
    if c["causal"]:
        i = c["q"].shape[0] - 1  # the last query of the 300-token pair sees its 300 keys
        s = c["q"][i, :64] @ c["k"][i - 299 : i + 1, :64].T + c["tab"][0][np.minimum(np.arange(299, -1, -1), c["nbias"] - 1)]
    else:
        s = c["q"][1, :64] @ c["k"][1:301, :64].T  # pair (1, 300)
    pmax = float(np.exp(s - s.max()).max() / np.exp(s - s.max()).sum())
    print(f"{name}: largest probability of a 300-key row {pmax:.3f}, largest |score| {np.abs(s).max():.1f}")
    assert pmax > 10.0 / 300
    assert not big or np.abs(s).max() > 20.0


def _applies(mutant, name):
    causal, H = dk.ATTENTION_CASES[name][0], dk.ATTENTION_CASES[name][1]
    form = dk.ATTENTION_MUTANTS[mutant]
    return (form == "both" or form == ("causal" if causal else "cross")) and not (mutant == "prev_head_bias" and H == 1)


@pytest.mark.parametrize("mutant", sorted(dk.ATTENTION_MUTANTS))
def test_planted_attention_bugs_miss_a_bar(mutant):
    cases = [n for n in sorted(dk.ATTENTION_CASES) if _applies(mutant, n)]
    assert cases
    for name in cases:
        c, exact, _, bounds = _refs(name)
        found = dk.attention_findings(c, dk.attention_reference(c, rounded=True, mutant=mutant), exact, bounds)
        print(f"{mutant} on {name}: {found}")
        assert found, f"{mutant} passes every bar on {name}"


# ---- row kernels: the stand-in is the float64 reference rounded to the output's format -------------------------------------
@pytest.mark.parametrize("V", [64, 320, 384, 512])
def test_dlogits_bars_and_planted_bugs(V):
    logits, labels, n_tok, rows = dk.dlogits_inputs(V)
    count = float(((labels >= 0) & (labels < V)).sum())
    ref = dk.dlogits_reference(logits.astype(np.float64), labels, n_tok, count)
    yard = dk.dlogits_yardstick(torch.from_numpy(logits), labels, n_tok, count).numpy()
    assert dk.bf16_row_findings("dlogits", dk.bf16_round(ref), ref, yard, dk.FASTMATH_DLOGITS) == []
    assert not ref[n_tok:].any() and not ref[[3, 64, 129, 10, 128]].any() and ref[5].any() and ref[6].any()
    for mutant in ("onehot_plus_one", "count_all"):
        bad = dk.bf16_round(dk.dlogits_reference(logits.astype(np.float64), labels, n_tok, count, mutant))
        assert dk.bf16_row_findings("dlogits", bad, ref, yard, dk.FASTMATH_DLOGITS), mutant


@pytest.mark.parametrize("F", [64, 256, 3584])
def test_geglu_bars_and_planted_bug(F):
    gu, dff, n_tok, rows = dk.geglu_inputs(F)
    ref = dk.geglu_bwd_reference(gu.astype(np.float64), dff.astype(np.float64), n_tok)
    yard = dk.geglu_bwd_reference(torch.from_numpy(gu), torch.from_numpy(dff), n_tok).numpy()
    assert dk.bf16_row_findings("geglu", dk.bf16_round(ref), ref, yard, dk.FASTMATH_GEGLU) == []
    bad = dk.bf16_round(dk.geglu_bwd_reference(gu.astype(np.float64), dff.astype(np.float64), n_tok, "swap_gate_up"))
    assert dk.bf16_row_findings("geglu", bad, ref, yard, dk.FASTMATH_GEGLU)
    g, _ = dk.split_gate_up(gu, F)
    assert g.min() <= -11.9 and g.max() >= 11.9


@pytest.mark.parametrize("T", [1, 255, 256, 257, 600])
def test_embed_reference_and_planted_bug(T):
    V, D = 384, 128
    ids, dx = dk.embed_inputs(T, V, D)
    ref = dk.embed_bwd_reference(ids, dx.astype(np.float64), V)
    yard = torch.zeros(V, D).index_add_(0, torch.from_numpy(np.clip(ids, 0, V - 1)).long(), torch.from_numpy(dx)).numpy()
    bar = dk.yardstick_bar(ref, yard)
    assert np.abs(yard - ref).max() <= bar
    assert ((ids < 0) | (ids >= V)).any() and not ref[[33, 34, V - 2]].any()
    bad = dk.embed_bwd_reference(ids, dx.astype(np.float64), V, mutant="no_id_clamp")
    assert np.abs(bad - ref).max() > bar
    if T > 2:
        assert len(set(ids.tolist())) < T, "ids repeat"
