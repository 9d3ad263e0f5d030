"""tests/encoder_forward_helpers.py on the build machine, on the shapes tests/test_encoder_forward_kernels_gpu.py runs: the
float64 restatements equal torch float64 (matmul, softmax, HF's gelu_new) within 1e-11; a float32 stand-in of each kernel's
schedule meets every bar; each planted bug IN THE STAND-IN misses at least one; the integer-operand cases are exact (largest
possible partial sum below 2^24, results representable in the output formats)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_forward_helpers as ef  # noqa: E402

ALL_KS = tuple(sorted(set(ef.KS_BK64) | set(ef.KS_BK32)))
EPIS = (ef.EPI_STORE, ef.EPI_RESID, ef.EPI_GEGLU, ef.EPI_RESID8)


def _n_of(epi, n):
    return n if epi != ef.EPI_GEGLU else (n if n % 64 == 0 else None)


def _rs(M, np_=23, D=1472, seed=0):
    rng = np.random.default_rng([seed, M, np_])
    ssp = (rng.uniform(0.2, 3.0, (np_, M)) * 64).astype(np.float32)
    return ssp, ef.rs_reference(ssp, 1.0 / D)


def _standin_rs(ssp, inv_d):
    s = np.zeros(ssp.shape[1])
    for i in range(ssp.shape[0]):
        s = ef._f32(s + ssp[i])
    return ef._f32(1.0 / np.sqrt(ef._f32(ef._f32(s * np.float32(inv_d)) + np.float32(ef.EPS))))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against torch float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_gemm_restatement_equals_torch_float64():
    for K in (64, 1504):
        A, W, x0 = ef.gemm_operands(256, 256, K, "normal", True)
        P, S = ef.gemm_products(256, 256, K, "normal", True)
        tA, tW = torch.from_numpy(A.copy()), torch.from_numpy(W.copy())
        tP = tA @ tW.T
        assert np.abs(P - tP.numpy()).max() <= 1e-11
        _, rs = _rs(256)
        r = torch.from_numpy(rs)[:, None]
        assert np.abs(ef.gemm_expected(ef.EPI_STORE, P, S, K, rs=rs)[0] - (tP * r).numpy()).max() <= 1e-11
        assert np.abs(ef.gemm_expected(ef.EPI_RESID8, P, S, K, x0=x0)[0] - (torch.from_numpy(x0.copy()) + tP).numpy()).max() <= 1e-11
        # HF NewGELUActivation on the un-interleaved rows
        Wv = tW.view(256 // 64, 2, 32, K)
        g, u = (tA @ Wv[:, 0].reshape(-1, K).T) * r, (tA @ Wv[:, 1].reshape(-1, K).T) * r
        hf = 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * torch.pow(g, 3.0)))) * u
        ref = ef.gemm_expected(ef.EPI_GEGLU, P, S, K, rs=rs)[0]
        assert np.abs(ref - hf.numpy()).max() <= 1e-11 * max(1.0, float(hf.abs().max()))


@pytest.mark.parametrize("name", ["h2-d32-std12-mixed", "h1-d8-std4-mixed", "h2-d32-std4-700"])
def test_attention_restatement_equals_torch_float64(name):
    c = ef.attention_case(name)
    ref = ef.attention_reference(c)[0]
    H, maxd, inner = c["H"], c["maxd"], c["H"] * 64
    qkv, tab = torch.from_numpy(c["qkv"].copy()), torch.from_numpy(c["tab"].copy())
    for b in range(len(c["lens"])):
        s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
        pos = torch.arange(s1 - s0)
        rel = (pos[None, :] - pos[:, None]).clamp(-maxd, maxd) + maxd
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            q, k, v = (qkv[s0:s1, o * inner:(o + 1) * inner][:, sl] for o in range(3))
            want = torch.softmax(q @ k.T + tab[h][rel], dim=-1) @ v
            assert np.abs(ref[s0:s1, sl] - want.numpy()).max() <= 1e-11


def test_plan_mixed_restatement_on_256_cus():
    assert ef.plan_mixed(8, 33, 256) == (32, 2, 0)
    assert ef.plan_mixed(16, 22, 256) == (16, 8, 4)
    assert ef.plan_mixed(16, 17, 256) == (16, 2, 0)
    assert ef.plan_mixed(16, 16, 256) == (0, 0, 0) and ef.plan_mixed(6, 274, 256)[0] == 256
    shapes = ef.smallest_form_shapes(256)
    assert set(shapes) == {"persist", "mixed", "mixed_tail"}
    tf, tt = shapes["persist"]
    assert (tf, tt) == (16, 17) and shapes["mixed"] == (4, 65)
    assert ef.plan_mixed(*shapes["mixed"], 256)[2] == 0 and ef.plan_mixed(*shapes["mixed_tail"], 256)[2] > 0
    assert ef.expected_form(16, 17, 128, 256, ef.K_QKV, 9, 20, ef.EPI_STORE) == (ef.FORM_PERSIST, 0)
    assert ef.expected_form(16, 17, 64, 256, ef.K_QKV, 9, 20, ef.EPI_STORE) == (ef.FORM_TILE, 0)
    assert ef.expected_form(16, 22, 128, 256, ef.K_WO, 9, 20, ef.EPI_RESID8) == (ef.FORM_MIXED, 16)
    assert ef.expected_form(16, 22, 128, 256, ef.K_WI, 9, 28, ef.EPI_GEGLU) == (ef.FORM_PERSIST, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: stand-in against the bars, planted bugs, exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ALL_KS + ef.KS_LONG)
def test_gemm_standin_meets_every_bar(K):
    M = 256
    ssp, rs = _rs(M)
    rs32 = _standin_rs(ssp, 1.0 / 1472)
    assert np.abs(rs32 / rs - 1).max() <= ef.rs_rel_bar(ssp.shape[0])
    for epi in EPIS:
        geglu = epi == ef.EPI_GEGLU
        A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", geglu)
        P, S = ef.gemm_products(M, ef.N_MAX, K, "normal", geglu)
        acc = ef.standin_acc(A, W)
        assert (np.abs(acc - P) <= ef.acc_bar(S, K)).all()
        for n in ef.N_VALIDS:
            if _n_of(epi, n) is None:
                continue
            use_rs = rs if epi in (ef.EPI_STORE, ef.EPI_GEGLU) else None
            ref, bar = ef.gemm_expected(epi, P[:, :n], S[:, :n], K, x0[:, :n], use_rs, ef.rs_rel_bar(23), extra=0.0)
            np_out = (n + 63) // 64
            got, s = ef.standin_epilogue(epi, acc[:, :n], x0[:, :n], None if use_rs is None else rs32, np_out)
            assert ef.findings(f"{ef.EPI_NAMES[epi]} K={K} n={n}", got, ref, bar) == []
            if s is not None:
                sref, sbar = ef.ssp_reference(got, np_out)
                assert ef.findings("ssp", s, sref, sbar) == []
    if K >= 64:
        g = ef.geglu_split(ef.gemm_products(M, ef.N_MAX, K, "normal", True)[0])[0]
        assert np.abs(g).max() > 100 and np.abs(g[:, 0::4]).std() < 1.5, "the gate sweep covers the whole range"


@pytest.mark.parametrize("K", (64, 256, 1472))
def test_gemm_planted_bugs_miss_a_bar(K):
    M, n = 256, 96
    ssp, rs = _rs(M)
    rs32 = _standin_rs(ssp, 1.0 / 1472)
    for epi, mutant in ((ef.EPI_RESID, "resid_overwrites"), (ef.EPI_RESID8, "resid_overwrites"),
                        (ef.EPI_GEGLU, "geglu_up_row_plus_31"), (ef.EPI_STORE, "rs_neighbour_row"),
                        (ef.EPI_GEGLU, "rs_neighbour_row")):
        geglu = epi == ef.EPI_GEGLU
        nn = 128 if geglu else n
        A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", geglu)
        P, S = ef.gemm_products(M, ef.N_MAX, K, "normal", geglu)
        use = rs if epi in (ef.EPI_STORE, ef.EPI_GEGLU) else None
        ref, bar = ef.gemm_expected(epi, P[:, :nn], S[:, :nn], K, x0[:, :nn], use, ef.rs_rel_bar(23))
        got, _ = ef.standin_epilogue(epi, ef.standin_acc(A, W)[:, :nn], x0[:, :nn], None if use is None else rs32, 0, mutant)
        assert ef.findings(mutant, got, ref, bar), (mutant, ef.EPI_NAMES[epi])
        # and the same bug in the reference's place is as far from the reference
        bad = ef.gemm_expected(epi, P[:, :nn], S[:, :nn], K, x0[:, :nn], use, ef.rs_rel_bar(23), mutant=mutant)[0]
        assert ef.findings(mutant, bad, ref, bar)
    # the last, half-full statistic slot dropped
    A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal")
    acc = ef.standin_acc(A, W)[:, :n]
    got, s = ef.standin_epilogue(ef.EPI_RESID8, acc, x0[:, :n], None, 2, "drop_last_half_slot")
    sref, sbar = ef.ssp_reference(got, 2)
    assert ef.findings("ssp", s, sref, sbar)
    # the last valid row not replicated under tokens_valid: the reference of a call under a count has the last valid row's
    # products in every row from the count on (each with its own old x), as the GPU test's padding rows of the last tile do
    tv = 101
    P, S = ef.gemm_products(M, ef.N_MAX, K, "normal")
    Pr, Sr = P.copy(), S.copy()
    Pr[tv:], Sr[tv:] = P[tv - 1], S[tv - 1]
    for epi in (ef.EPI_STORE, ef.EPI_RESID8):
        ref, bar = ef.gemm_expected(epi, Pr[:, :n], Sr[:, :n], K, x0[:, :n])
        good = ef.standin_epilogue(epi, ef.standin_acc(A, W, tv)[:, :n], x0[:, :n])[0]
        bad = ef.standin_epilogue(epi, ef.standin_acc(A, W, tv, "no_row_replication")[:, :n], x0[:, :n])[0]
        assert ef.findings("tokens_valid", good, ref, bar) == []
        found = ef.findings("no_row_replication", bad, ref, bar)
        assert found, ef.EPI_NAMES[epi]
        assert ef.findings("rows below the count", bad[:tv], ref[:tv], bar[:tv]) == [], "only the padding rows miss"


@pytest.mark.parametrize("K", ALL_KS)
def test_integer_operand_cases_are_exact(K):
    M = 256
    for geglu in (False, True):
        A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "integer", geglu)
        P, S = ef.gemm_products(M, ef.N_MAX, K, "integer", geglu)
        assert S.max() <= 16 * K <= 24064 < 2 ** 24, "every partial sum in any order is an integer below 2^24"
        acc = ef.standin_acc(A, W)
        assert (acc == P).all() and (P == np.round(P)).all()
        if geglu:
            continue
        v = x0 + P
        assert np.abs(v).max() < 2 ** 15
        assert (ef.x24_round(v) == v).all(), "exact in the 24-bit form (16 significant bits)"
        hi, lo = ef.split_planes_np(v)
        assert (hi + lo == v).all(), "exact on the two bf16 planes"
        ref, bar = ef.gemm_expected(ef.EPI_RESID8, P, S, K, x0, exact_acc=True)
        assert (ef.standin_epilogue(ef.EPI_RESID8, acc, x0)[0] == ref).all()
        # (the statistic of these planes - sums of 64 squares of up to 2^30 - is not exact in fp32: it keeps its bar)
        ref, bar = ef.gemm_expected(ef.EPI_STORE, P, S, K, exact_acc=True)
        assert (ref == P).all() and (bar == ef.bf16_half_ulp(P)).all(), "the store's bar is the one rounding: the GPU test asserts bf16(P)"


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
ATT_CPU = ["h1-d8-std4-mixed", "h2-d32-std12-mixed", "h6-d128-std4-mixed", "h2-d32-std4-700", "h2-d8-std12-short"]


@pytest.mark.parametrize("name", ATT_CPU)
def test_attention_standin_meets_the_bar_and_planted_bugs_miss_it(name):
    c = ef.attention_case(name)
    ref, lead, f32 = ef.attention_reference(c)
    m = {}
    assert ef.attention_findings(name, ef.standin_attention(c), ref, lead, f32, m) == [], m
    assert m[name]["worst_error_over_bar"] <= 1.0
    # (the 1300 short sequences: the one planted bug they are there for - every sequence has a neighbour's row behind it)
    for mutant in ("mask_le_len",) if name.endswith("short") else ("bias_off_by_one", "clamp_one_early", "mask_le_len", "bias_sign"):
        assert ef.attention_findings(mutant, ef.standin_attention(c, mutant), ref, lead, f32), (name, mutant)
        if not name.endswith("short"):
            assert ef.findings(mutant, ef.attention_reference(c, mutant)[0], ref, ef.attention_bar(ref, lead, f32)), (name, mutant)


def test_attention_late_jump_row_and_table_limit():
    c = ef.late_jump_case()
    ref, lead, f32 = ef.attention_reference(c)
    assert ef.attention_findings("late-jump", ef.standin_attention(c), ref, lead, f32) == []
    assert np.abs(ref[7] - c["qkv"][300, 128:192]).max() < 1e-6, "row 7 is v[300]"
    assert 2 * 447 + 1 + 128 <= ef.ATT_TAB_MAX < 2 * 448 + 1 + 128, "447 is the largest max_distance the table admits"


# ---------------------------------------------------------------------------------------------------------------------------
# embedding rows, last_hidden_state rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ef.EMBED_DS)
def test_embed_encoding_and_hidden_out_bar(D):
    table = ef.embed_table(D)
    hi, ext, x = ef.embed_table_reference(table)
    assert (np.abs(x - table) <= 2.0 ** -16 * np.abs(table)).all() and not x[5].any()
    ss = ef.embed_ss_standin(x)
    exact = (x ** 2).sum(1)
    assert (np.abs(ss - exact) <= (D // 512 * 8 + 8 + 6) * ef.U32 * exact).all()
    ids = ef.embed_ids(300)
    src, rows = ef.embed_rows_reference(ids, ef.EMBED_VOCAB, 300, 512)
    assert rows == 512 and src.min() == 0 and src.max() == ef.EMBED_VOCAB - 1 and not src[300:].any()
    assert src[0] == 0 and src[100] == ef.EMBED_VOCAB - 1 and src[299] == 0
    src, rows = ef.embed_rows_reference(ids, ef.EMBED_VOCAB, 300, 512, t_live=255)
    assert rows == 256 and not src[255:].any()
    assert ef.embed_rows_reference(ids, ef.EMBED_VOCAB, 300, 512, t_live=257)[1] == 512
    rs = 1.0 / np.sqrt(exact / D + ef.EPS)
    w = 1.0 + 0.2 * np.random.default_rng(D).standard_normal(D)
    ref, bar = ef.hidden_out_reference(x, rs.astype(np.float32), w.astype(np.float32))
    got = ef.bf16_round(ef._f32(w.astype(np.float32)[None] * ef._f32(x * rs.astype(np.float32).astype(np.float64)[:, None])))
    assert ef.findings("hidden_out", got, ref, bar) == [] and not got[5].any()
    assert ef.findings("row + 1", np.roll(got, 1, 0), ref, bar)
