"""That the bars of tests/test_decode_step_kernels_gpu.py mean something (no GPU): on the GPU tests' own shapes a numpy stand-in
for each kernel - bf16 operands, float32 accumulation in the kernel's documented order, rounding where the kernel rounds -
meets every bar the GPU test applies, and every planted bug (tests/decode_step_helpers.py: the float64 restatement with one
line changed, rounded as the kernel's store rounds) misses at least one.  The bars are computed by the functions the GPU file
imports.  Also here: the float64 restatements against torch float64 (matmul, softmax, log_softmax, T5DecodeEmu._attend) within
1e-11, and that the integer-operand GEMM cases are exact in fp32 (every partial sum below 2^24)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_step_helpers as ds  # noqa: E402
from gen_helpers import T5DecodeEmu  # noqa: E402

EPIS = (ds.EPI_BF16, ds.EPI_RESID, ds.EPI_F32, ds.EPI_GEGLU)


# ---- the restatements against torch float64 ---------------------------------------------------------------------------------
def test_gemm_reference_is_torchs_matmul():
    A, W, out0 = ds.gemm_operands(520)
    P = (torch.from_numpy(A.copy()) @ torch.from_numpy(W.copy()).T).numpy()
    gelu = lambda u: 0.5 * u * (1.0 + torch.tanh(0.7978845608028654 * (u + 0.044715 * u ** 3)))  # noqa: E731
    want = {ds.EPI_BF16: P[:, :130], ds.EPI_F32: P[:, :130], ds.EPI_RESID: out0 + P[:, :130],
            ds.EPI_GEGLU: (gelu(torch.from_numpy(P[:, :130])) * torch.from_numpy(P[:, 130:])).numpy()}
    for epi in EPIS:
        got = ds.gemm_reference(A, W, 130, epi, out0)
        assert np.abs(got - want[epi]).max() <= 1e-11 * max(1.0, np.abs(want[epi]).max()), epi


def _attend(c, row):
    """T5DecodeEmu._attend (float64, unrounded) on one row of a case."""
    emu = T5DecodeEmu.__new__(T5DecodeEmu)
    emu.r = lambda x: x
    H, nb = c["H"], c["nb"]
    slot = row // nb
    if c["cross"]:
        keys = c["kv"][c["src_off"][slot]:c["src_off"][slot] + c["src_len"][slot]]
        bias = None
    else:
        n = c["pos"][slot] + 1
        keys = c["kv"][c["state"][slot]][np.clip(c["anc"][row, :n], 0, c["rows"] - 1)]
        bias = torch.from_numpy(c["tab"][:, np.minimum(n - 1 - np.arange(n), c["nbias"] - 1)])[None]
    n = keys.shape[0]
    k = torch.from_numpy(keys[:, c["koff"]:c["koff"] + 64 * H].reshape(n, H, 64)).transpose(0, 1)[None]
    v = torch.from_numpy(keys[:, c["voff"]:c["voff"] + 64 * H].reshape(n, H, 64)).transpose(0, 1)[None]
    return emu._attend(torch.from_numpy(c["q"][row].reshape(1, H, 64)), k, v, bias)[0].numpy()


@pytest.mark.parametrize("kind,name", [("self", "h3-nb3-n257"), ("self", "h6-nb1-n33"), ("cross", "h3-nb3"), ("cross", "h6-nb1")])
def test_attention_reference_is_the_emulators_attend(kind, name):
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    ref = ds.attention_reference(c)
    for row in range(c["q"].shape[0]):
        assert np.abs(ref[row] - _attend(c, row)).max() <= 1e-11, (name, row)


def test_row_references_are_torchs():
    for V in (3, 257, 512):
        x = ds.log_softmax_inputs(V, 130).astype(np.float64)
        want = torch.log_softmax(torch.from_numpy(x), -1).numpy()
        assert np.abs(ds.log_softmax_reference(x) - want).max() <= 1e-11
        assert np.abs(np.exp(ds.log_softmax_reference(x)) - torch.softmax(torch.from_numpy(x), -1).numpy()).max() <= 1e-11
    x, w = ds.rmsnorm_inputs(264)
    xt, wt = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    want = (wt * (xt * torch.rsqrt(xt.pow(2).mean(-1, keepdim=True) + ds.RMS_EPS)) * 0.25).numpy()
    assert np.abs(ds.rmsnorm_reference(x, w, ds.RMS_EPS, 0.25) - want).max() <= 1e-11
    table = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(ds.embed_reference(np.array([-1, 4, 2, -2 ** 31]), table), table[[0, 3, 2, 0]])


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
def test_every_gemm_instantiation_is_reached():
    assert sorted({ds.kit_of(K) for K in ds.GEMM_KS}) == list(range(1, 9))
    nk = {K: K // 8 for K in ds.GEMM_KS}
    assert nk[8] == 1 and nk[520] % 64 == 1 and nk[2040] % 64 == 63  # one live lane; one idle lane in the last group
    assert ds.kit_of(4096) == 8 and ds.kit_of(4104) == 9


@pytest.mark.parametrize("K", ds.GEMM_KS)
def test_integer_operands_are_exact_in_fp32(K):
    """Every partial sum, in any order, is an integer of magnitude below 2^24; the stand-in's fp32 chain therefore equals
    the float64 result, and a dropped or misplaced piece changes it."""
    A, W, out0 = ds.gemm_operands(K, "integer")
    assert np.array_equal(A, np.round(A)) and np.abs(A).max() <= 8 and np.abs(W).max() <= 8
    assert ds.gemm_max_partial_sum(A, W) + np.abs(out0).max() < 2 ** 24
    sums = ds.gemm_standin_sums(A[:33], W[:130])
    for epi in (ds.EPI_BF16, ds.EPI_RESID, ds.EPI_F32):
        want = ds.gemm_exact_expected(A[:33], W[:130], 130, epi, out0[:33])
        standin = ds.gemm_store(ds.gemm_reference(A[:33], W[:130], 130, epi, out0[:33], np.float32, sums=sums), epi)
        assert np.array_equal(standin, want), (K, epi)
        for mutant in ("w_piece_plus_one", "drop_last_partial_group", "resid_overwrites"):
            if mutant == "drop_last_partial_group" and (K // 8) % 64 == 0:
                continue
            if ds.GEMM_MUTANTS[mutant] and epi not in ds.GEMM_MUTANTS[mutant]:
                continue
            bad = ds.gemm_store(ds.gemm_reference(A[:33], W[:130], 130, epi, out0[:33], mutant=mutant), epi)
            assert (bad != want).mean() > 0.5, (K, epi, mutant)


@pytest.mark.parametrize("K", ds.GEMM_KS)
def test_gemm_standin_meets_the_bars_and_planted_bugs_miss_them(K):
    A, W, out0 = ds.gemm_operands(K)
    M, N = 33, ds.GEMM_MAX_N
    a, o0 = A[:M], out0[:M]
    sums = ds.gemm_standin_sums(a, W)  # [M, 260]
    for epi in EPIS:
        w = ds.gemm_w(W, N, epi, K)
        s = sums[:, :N]
        if epi == ds.EPI_GEGLU:
            s = np.concatenate([ds.gemm_standin_sums(a, w[:N]), sums[:, N:]], 1)  # (the gate rows are scaled)
        ref, bar = ds.gemm_bar(a, w, N, epi, o0, ds.FASTMATH_DEC_GEGLU)
        standin = ds.gemm_store(ds.gemm_reference(a, w, N, epi, o0, np.float32, sums=s), epi)
        assert ds.gemm_findings("stand-in", standin, ref, bar) == [], (K, epi)
        for mutant, epis in ds.GEMM_MUTANTS.items():
            if (epis and epi not in epis) or (mutant == "drop_last_partial_group" and (K // 8) % 64 == 0):
                continue
            bad = ds.gemm_store(ds.gemm_reference(a, w, N, epi, o0, mutant=mutant), epi)
            assert ds.gemm_findings(mutant, bad, ref, bar), (K, epi, mutant)
        if epi == ds.EPI_GEGLU:
            a0 = (a @ w.T)[:, :N]
            assert np.abs(a0).max() > 30.0 and (np.abs(a0) < 3.0).mean() > 0.3, (K, np.abs(a0).max())


# ---- attention --------------------------------------------------------------------------------------------------------------
ATT = [("self", n) for n in sorted(ds.SELF_CASES)] + [("cross", n) for n in sorted(ds.CROSS_CASES)]


@functools.lru_cache(maxsize=None)
def _att(kind, name):
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    return c, ds.attention_reference(c), ds.attention_yardstick(c)


def test_attention_cases_cover_the_issue():
    counts = {p + 1 for n in ds.SELF_CASES for p in ds.SELF_CASES[n][3]}
    assert counts >= {1, 2, 255, 256, 257, 258, 300, 1025, 8192}
    assert {ds.SELF_CASES[n][0] for n in ds.SELF_CASES} >= {1, 3, 6, 12} and {ds.SELF_CASES[n][1] for n in ds.SELF_CASES} == {1, 3, 64}
    assert {ds.self_case(n)["nbias"] for n in ds.SELF_CASES} == {33, 257}
    assert {s for n in ds.CROSS_CASES for s in ds.CROSS_CASES[n][2]} >= {1, 63, 64, 65, 255, 256, 257, 2048}
    for n in ds.CROSS_CASES:
        c = ds.cross_case(n)
        assert c["src_off"] != sorted(c["src_off"]), "the sources are not placed in slot order"
    c = ds.self_case("h3-nb3-n33-mixed")
    assert c["pos"] == [0, 256, 40, 299] and c["state"] == [2, 0, 3, 1]
    c = ds.self_case(ds.HAND_MADE_ROW)
    r = c["anc"][(len(c["pos"]) - 1) * c["nb"] + 1]
    assert r.min() < 0 and r.max() >= c["rows"]
    assert len({tuple(x[:200]) for x in c["anc"][-3:]}) > 1
    anc = ds.self_case("h1-nb64-n33")["anc"][64:128, :41]
    assert len(np.unique(anc[:, 20])) < 64, "parents repeat: beams share ancestors"


@pytest.mark.parametrize("kind,name", ATT, ids=[f"{k}-{n}" for k, n in ATT])
def test_attention_standin_meets_the_bar(kind, name):
    c, exact, yard = _att(kind, name)
    m = {}
    standin = ds.attention_reference(c, np.float32, rounded=True)
    assert ds.attention_findings(name, standin, exact, yard, m) == []
    if not c["cross"]:  # sharp rows: at 300 keys the largest probability is far above 1 / 300; "big" scores reach 30
        big = c["scale"] > 1.0
        for a, p in enumerate(c["pos"]):
            if p + 1 >= 300:
                row = a * c["nb"]
                k = c["kv"][c["state"][a]][np.clip(c["anc"][row, :p + 1], 0, c["rows"] - 1)][:, :64]
                s = k @ c["q"][row, :64] + c["tab"][0][np.minimum(p - np.arange(p + 1), c["nbias"] - 1)]
                e = np.exp(s - s.max())
                assert e.max() / e.sum() > 10.0 / (p + 1) and (not big or np.abs(s).max() > 20.0), (name, a)


@pytest.mark.parametrize("mutant", sorted(ds.ATTENTION_MUTANTS))
def test_planted_attention_bugs_miss_the_bar(mutant):
    form = ds.ATTENTION_MUTANTS[mutant]
    cases = [(k, n) for k, n in ATT if form in ("both", k)]
    if mutant == "ancestry_ignored":
        cases = [(k, n) for k, n in cases if ds.SELF_CASES[n][1] > 1]  # one beam: the ancestry IS the identity
    if mutant == "pos_of_slot_0":
        cases = [(k, n) for k, n in cases if len(set(ds.SELF_CASES[n][3])) > 1]
    if mutant == "drop_last_key_mod_256":
        # (not the "big" case: among scores of magnitude 30 the last of 1025 keys weighs nothing)
        cases = [(k, n) for k, n in cases if any(p > 0 and p % 256 == 0 for p in ds.SELF_CASES[n][3]) and ds.SELF_CASES[n][5] < 1]
    if mutant == "clamp_at_nbias_minus_2":  # a table by buckets is constant from max_distance on: only a table with a value
        # per distance shows where the clamp sits
        cases = [(k, n) for k, n in cases if isinstance(ds.SELF_CASES[n][2], int)]
    assert len(cases) >= 2, mutant
    for kind, name in cases:
        c, exact, yard = _att(kind, name)
        bad = ds.attention_reference(c, rounded=True, mutant=mutant)
        found = ds.attention_findings(name, bad, exact, yard)
        print(f"{mutant} on {kind}-{name}: {found}")
        assert found, f"{mutant} passes the bar on {kind}-{name}"


# ---- row kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", ds.LOG_SOFTMAX_VS)
def test_log_softmax_standin_and_planted_bugs(V):
    for rows in ds.LOG_SOFTMAX_ROWS:
        x = ds.log_softmax_inputs(V, rows)
        ref = ds.log_softmax_reference(x)
        yard = torch.log_softmax(torch.from_numpy(x), -1).numpy()
        assert ds.fp32_findings("stand-in", ds.log_softmax_reference(x, np.float32), ref, yard) == [], (V, rows)
        if V == 1:
            assert not ref.any()
        if V > 256:
            assert ds.fp32_findings("m", ds.log_softmax_reference(x, np.float32, "sum_stops_at_256"), ref, yard), (V, rows)
        if rows > 7 and V > 1:
            assert np.abs(ref[5] - ref[7]).max() <= 1e-12 and ref[5].min() < -159.0 and np.abs(ref[6] + np.log(V)).max() < 1e-12
            assert ds.fp32_findings("m", ds.log_softmax_reference(x, np.float32, "no_max"), ref, yard), (V, rows)


@pytest.mark.parametrize("D", ds.RMSNORM_DS)
def test_rmsnorm_standin_and_planted_bugs(D):
    x, w = ds.rmsnorm_inputs(D)
    assert not x[1].any() and np.abs(x[2]).max() > 1e4
    xt, wt = torch.from_numpy(x), torch.from_numpy(w)
    for scale in (1.0, float(np.float32(D ** -0.5))):
        ref = ds.rmsnorm_reference(x, w, ds.RMS_EPS, scale)
        yard = (wt * (xt * torch.rsqrt((xt * xt).mean(1, keepdim=True) + ds.RMS_EPS)) * scale).numpy()
        standin = ds.rmsnorm_reference(x, w, ds.RMS_EPS, scale, np.float32, rounded=True)
        assert ds.bf16_row_findings("stand-in", standin, ref, yard) == [] and not standin[1].any(), (D, scale)
        if D % 256:
            bad = ds.rmsnorm_reference(x, w, ds.RMS_EPS, scale, rounded=True, mutant="mean_over_padded_d")
            assert ds.bf16_row_findings("m", bad, ref, yard), (D, scale)
        if scale != 1.0:
            bad = ds.rmsnorm_reference(x, w, ds.RMS_EPS, scale, rounded=True, mutant="scale_dropped")
            assert ds.bf16_row_findings("m", bad, ref, yard), (D, scale)


def test_store_kv_reference_and_planted_bugs():
    nb, inner = 3, 64
    state, pos = [2, 0, 3], [8, 0, 5]
    rng = np.random.default_rng(0)
    qkv = rng.integers(-2 ** 15, 2 ** 15, size=(9, 3 * inner)).astype(np.int16)
    before = np.full((4, 27, 2 * inner), 0x5A5A, np.int16)
    want = ds.store_kv_reference(qkv, before, state, pos, nb)
    changed = np.argwhere((want != before).any(2))
    assert sorted(map(tuple, changed)) == sorted((s, p * nb + b) for s, p in zip(state, pos) for b in range(nb))
    assert np.array_equal(want[3, 15:18], qkv[6:9, inner:])
    for mutant in ("pos_of_slot_0", "v_not_stored"):
        assert not np.array_equal(ds.store_kv_reference(qkv, before, state, pos, nb, mutant), want), mutant
