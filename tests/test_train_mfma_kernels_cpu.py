"""tests/train_kernel_helpers.py on the build machine, on the shapes tests/test_train_mfma_kernels_gpu.py runs: the float64
restatements equal torch float64 (matmul; autograd through the folded RMSNorm weight, gelu_new, RMSNorm and softmax) within
1e-11; a float32 stand-in of wgrad_kernel's schedule, of the four GEMM epilogues and of the attention kernels meets every bar;
each planted bug IN THE STAND-IN misses one; the integer-operand cases are exact by the stated magnitude argument; the launch
plans rp_dbg_wgrad_plan reports (no GPU call) are the restated cost model's, pinned at the ByT5-small / base training geometries."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_forward_helpers as ef  # noqa: E402
import train_kernel_helpers as tk  # noqa: E402


def _splits(T):
    return [s for s in tk.WGRAD_SPLITS if s <= T // 64]


def _within(got, ref, bar):
    return bool((np.isfinite(got) & (np.abs(got - ref) <= bar)).all())


def test_case_lists_cover_what_they_claim():
    nys = {s[0] for v in tk.WGRAD_SHAPES.values() for s in v}
    nxs = {s[1] for v in tk.WGRAD_SHAPES.values() for s in v}
    assert nys == set(tk.WGRAD_NS) and nxs == set(tk.WGRAD_NS)
    pads = {(s[2], s[3]) for v in tk.WGRAD_SHAPES.values() for s in v}
    assert {p[0] for p in pads} == {0, 8, 24} and {p[1] for p in pads} == {0, 8, 24}
    assert [T // 64 for T in tk.WGRAD_TS] == [1, 2, 3, 4, 5, 8, 16]
    # uneven ranges: 5 tiles in 2 and 3, 8 in 3 and 5
    assert tk.split_ranges(320, 2) == [(0, 128), (128, 320)] and tk.split_ranges(512, 3) == [(0, 128), (128, 320), (320, 512)]
    assert all(ny % 64 == 0 for ny in tk.FINISH_NYS)
    (a, b) = tk.PAIR_SHAPES[1]
    assert b[0] < 256 and b[1] < 256 and all(p[0] != p[1] for p in tk.PAIR_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against torch float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tk.WGRAD_TS)
def test_wgrad_restatement_equals_torch_float64(T):
    for ny, nx, _, _ in tk.WGRAD_SHAPES[T]:
        Y, X = tk.wgrad_operands(T, ny, nx, "normal")
        tY, tX = torch.from_numpy(Y.copy()), torch.from_numpy(X.copy())
        for S in _splits(T):
            ref, _ = tk.wgrad_reference(Y, X, S)
            assert np.abs(ref.sum(0) - (tY.T @ tX).numpy()).max() <= 1e-11 * T
            bounds = [s * (T // 64) // S * 64 for s in range(S + 1)]
            for s in range(S):
                want = tY[bounds[s]:bounds[s + 1]].T @ tX[bounds[s]:bounds[s + 1]]
                assert np.abs(ref[s] - want.numpy()).max() <= 1e-11


@pytest.mark.parametrize("ny,nx", [(64, 8), (320, 72), (576, 264)])
def test_finish_restatement_equals_torch_autograd(ny, nx):
    """y = x W'^T with W' the packed [32 gate | 32 up] rows of wi_0 / wi_1 times ln; loss = sum(dzs * y): autograd's gradients of
    wi_0, wi_1 and ln are g0, g1 and the column sums of dln_part."""
    T, F = 128, ny // 2
    Y, X = tk.wgrad_operands(T, ny, nx, "normal")
    w0, w1, ln = tk.finish_operands(F, nx, "normal")
    t0, t1, tl = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (w0, w1, ln))
    packed = torch.stack([t0.view(F // 32, 32, nx), t1.view(F // 32, 32, nx)], 1).reshape(ny, nx) * tl
    (torch.from_numpy(Y.copy()) * (torch.from_numpy(X.copy()) @ packed.T)).sum().backward()
    ref, bar = tk.wgrad_reference(Y, X, 1)
    fin = tk.finish_reference(ref[0], bar[0], w0, w1, ln)
    for name, grad in (("g0", t0.grad), ("g1", t1.grad)):
        assert np.abs(fin[name][0] - grad.numpy()).max() <= 1e-11 * T
    assert np.abs(fin["dln_part"][0].sum(0) - tl.grad.numpy()).max() <= 1e-11 * T * F


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-in against the bars, planted bugs, exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("T", tk.WGRAD_TS)
def test_wgrad_standin_meets_the_bar_and_reads_inside(T, cfg):
    for ny, nx, py, px in tk.WGRAD_SHAPES[T][:2]:
        Y, X = tk.wgrad_operands(T, ny, nx, "normal")
        for S in _splits(T):
            reads = tk.StandinReads()
            got = tk.standin_wgrad(tk.padded(Y, ny + py), ny, tk.padded(X, nx + px), nx, S, cfg, reads=reads)
            ref, bar = tk.wgrad_reference(Y, X, S)
            assert _within(got, ref, bar), (T, ny, nx, S)
            assert reads.outside == 0


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("T", tk.WGRAD_TS)
def test_wgrad_integer_cases_are_exact(T, cfg):
    """|partial sums| <= 16 T <= 16384 < 2^24: the stand-in's fp32 chain equals float64 to the bit, in every split."""
    assert 16 * max(tk.WGRAD_TS) < 2 ** 24
    ny, nx, py, px = tk.WGRAD_SHAPES[T][-1]
    Y, X = tk.wgrad_operands(T, ny, nx, "integer")
    assert np.abs(Y).max() <= 4 and np.abs(X).max() <= 4
    for S in _splits(T):
        got = tk.standin_wgrad(tk.padded(Y, ny + py), ny, tk.padded(X, nx + px), nx, S, cfg)
        ref, bar = tk.wgrad_reference(Y, X, S, exact=True)
        assert not bar.any() and np.array_equal(got, ref)


def test_planted_split_boundary_rounded_up_misses_the_per_split_bar():
    """5 token tiles in 2 splits: [0, 2), [2, 5) - rounded up [0, 3), [3, 5).  The SUM of the partials does not notice."""
    T, (ny, nx, py, px) = 320, tk.WGRAD_SHAPES[320][0]
    Y, X = tk.wgrad_operands(T, ny, nx, "normal")
    ref, bar = tk.wgrad_reference(Y, X, 2)
    bad = tk.standin_wgrad(tk.padded(Y, ny + py), ny, tk.padded(X, nx + px), nx, 2, 0, mutant="split_boundary_up")
    assert not _within(bad[0], ref[0], bar[0]) and not _within(bad[1], ref[1], bar[1])
    assert _within(bad.sum(0), ref.sum(0), bar.sum(0) + 2 * tk.U32 * np.abs(ref).sum(0))
    # even ranges hide it: the case list must hold uneven ones
    even = tk.standin_wgrad(tk.padded(Y[:256], ny), ny, tk.padded(X[:256], nx), nx, 2, 0, mutant="split_boundary_up")
    assert _within(even, *tk.wgrad_reference(Y[:256], X[:256], 2))


@pytest.mark.parametrize("cfg", [0, 1])
def test_planted_feature_clamp_dropped_reads_outside_the_matrix(cfg):
    """No stored element changes without the clamp (the pieces beyond the edge feed accumulators that are not stored): what goes
    wrong is the read.  The loader counts it; widths that are multiples of the tile never leave the matrix either way."""
    T = 64
    for ny, nx, py, px in tk.WGRAD_SHAPES[T]:
        Y, X = tk.wgrad_operands(T, ny, nx, "normal")
        ref, bar = tk.wgrad_reference(Y, X, 1)
        reads = tk.StandinReads()
        bad = tk.standin_wgrad(tk.padded(Y, ny + py), ny, tk.padded(X, nx + px), nx, 1, cfg, mutant="no_feature_clamp", reads=reads)
        assert _within(bad, ref, bar)
        assert (reads.outside > 0) == (ny % tk.CFG_TILE[cfg] != 0 or nx % tk.CFG_TILE[cfg] != 0)
    assert any(ny % 256 or nx % 256 for v in tk.WGRAD_SHAPES.values() for ny, nx, _, _ in v)


def _finish_case(ny, nx, kind, T=128):
    Y, X = tk.wgrad_operands(T, ny, nx, kind)
    w0, w1, ln = tk.finish_operands(ny // 2, nx, kind)
    ref, bar = tk.wgrad_reference(Y, X, 1, exact=kind == "integer")
    acc = tk.standin_wgrad(tk.padded(Y, ny), ny, tk.padded(X, nx), nx, 1, 0)[0]
    return acc, ref[0], bar[0], w0, w1, ln


@pytest.mark.parametrize("ny", tk.FINISH_NYS)
def test_finish_standin_meets_every_bar(ny):
    for nx in tk.FINISH_NXS:
        acc, ref, bar, w0, w1, ln = _finish_case(ny, nx, "normal")
        fin = tk.finish_reference(ref, bar, w0, w1, ln)
        got = tk.standin_finish(acc, w0, w1, ln)
        for name, (r, b) in fin.items():
            assert _within(got[name], r, b), (ny, nx, name)


@pytest.mark.parametrize("ny", tk.FINISH_NYS)
def test_finish_integer_cases_are_exact(ny):
    """Exact accumulators: g = fp32(acc ln) to the bit; integer masters: |dln_part| <= 32 x 4 x 16 T < 2^24, exact."""
    assert 32 * 4 * 16 * max(tk.WGRAD_TS) < 2 ** 24
    nx = 72
    acc, ref, bar, w0, w1, ln = _finish_case(ny, nx, "integer")
    assert np.array_equal(acc, ref)
    got = tk.standin_finish(acc, w0, w1, ln)
    fin = tk.finish_reference(ref, bar, w0, w1, ln)
    for k in range(2):
        assert np.array_equal(got[f"g{k}"].astype(np.float32), fin[f"g{k}"][0].astype(np.float32))
    assert np.array_equal(got["dln_part"], fin["dln_part"][0])


@pytest.mark.parametrize("mutant,misses", [("gate_up_swapped", ("g0", "g1", "dln_part")), ("sr0_one_group_late", ("g0", "g1", "dln_part")),
                                           ("dln_other_half_dropped", ("dln_part",))])
def test_planted_finish_bugs_miss_a_bar(mutant, misses):
    """(ny = 64 has one 64-row group: "one group late" wraps onto itself there, so the case list holds more than one group.)"""
    acc, ref, bar, w0, w1, ln = _finish_case(320, 72, "normal")
    fin = tk.finish_reference(ref, bar, w0, w1, ln)
    bad = tk.standin_finish(acc, w0, w1, ln, mutant=mutant)
    for name, (r, b) in fin.items():
        assert _within(bad[name], r, b) == (name not in misses), (mutant, name)
    assert any(ny > 64 for ny in tk.FINISH_NYS)


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plans
# ---------------------------------------------------------------------------------------------------------------------------
def _lib_plan(r0, c0, r1, c1, nk):
    from reprover_amd import _lib
    out = (ctypes.c_int32 * 4)(-9, -9, -9, -9)
    _lib.check(_lib.load().rp_dbg_wgrad_plan(r0, c0, r1, c1, nk, out), "rp_dbg_wgrad_plan")
    return tuple(out)


def test_wgrad_plan_is_the_restated_cost_model():
    for nk in (1, 2, 3, 4, 5, 8, 16, 64, 129, 640):
        for r0, c0, r1, c1 in ((7168, 1472, 1472, 3584), (1152, 1472, 1472, 384), (7936, 1536, 1536, 3968), (2304, 1536, 1536, 768),
                               (384, 264, 264, 200), (8, 8, 0, 0), (1472, 3584, 0, 0), (320, 136, 72, 120)):
            want = tk.plan_wgrad(r0, c0, nk) + (tk.plan_wgrad_pair(r0, c0, r1, c1, nk) if r1 else (-1, -1))
            assert _lib_plan(r0, c0, r1, c1, nk) == want, (r0, c0, r1, c1, nk)
    from reprover_amd import _lib
    out = (ctypes.c_int32 * 4)()
    for bad in ((0, 8, 0, 0, 1), (8, 8, 8, 0, 1), (8, 8, 0, 0, 0), (8, 8, -1, 8, 1)):
        assert _lib.load().rp_dbg_wgrad_plan(*bad, out) == -1
    assert _lib.load().rp_dbg_wgrad_plan(8, 8, 0, 0, 1, None) == -1


# model -> (d_model, d_ff, inner); nk = token tiles of the step's packed batch
GEOMETRY = {"byt5-small": (1472, 3584, 384), "byt5-base": (1536, 3968, 768)}
PINNED = {
    # (model, nk): (feed-forward pair (cfg, splits), attention pair (cfg, splits))
    # (164 token tiles = the reference's training batch: 40 sequences, 10.4 k tokens padded to 41 x 256)
    ("byt5-small", 64): ((0, 1), (0, 5)), ("byt5-small", 164): ((0, 1), (0, 6)), ("byt5-small", 256): ((0, 1), (0, 6)),
    ("byt5-small", 640): ((0, 1), (0, 6)), ("byt5-base", 164): ((0, 0), (0, 3)),
    # base: 31 x 6 + 6 x 16 = 282 tiles do not fit one round of 256: separate launches, no finishing epilogue
    ("byt5-base", 64): ((0, 0), (0, 3)), ("byt5-base", 256): ((0, 0), (0, 3)), ("byt5-base", 640): ((0, 0), (0, 7)),
}


@pytest.mark.parametrize("model", sorted(GEOMETRY))
def test_wgrad_plan_at_the_training_geometries(model):
    """Which form the sub-layers' weight gradients take: pair splits 1 = one split-free launch, dWi' finished in the epilogue
    (2 F % 64 == 0 at both models); > 1 = one launch + unfold passes; 0 = separate launches."""
    D, F, inner = GEOMETRY[model]
    assert (2 * F) % 64 == 0
    for nk in (64, 164, 256, 640):
        ff = _lib_plan(2 * F, D, D, F, nk)[2:]
        at = _lib_plan(3 * inner, D, D, inner, nk)[2:]
        assert (ff, at) == PINNED[(model, nk)], (model, nk, ff, at)


# ---------------------------------------------------------------------------------------------------------------------------
# the training step's GEMM epilogues
# ---------------------------------------------------------------------------------------------------------------------------
def _hf_gelu_new(g):
    return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * torch.pow(g, 3.0))))


def test_rms_bwd_restatement_equals_torch_autograd():
    """y = rs (x W'^T), rs = rsqrt(mean x^2 + eps), loss = sum(dy y): autograd's dx is P - rc x with the GEMM's A = dzs = rs dy,
    W = W'^T and rc = rs^2 (sum_o dy y) / D - what qkv_scale_dot_kernel / rowdot_finish_kernel hand the epilogue."""
    M, D, O = 16, 64, 96
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((M, D)), requires_grad=True)
    Wp, dy = torch.tensor(rng.standard_normal((O, D)) / 8), torch.tensor(rng.standard_normal((M, O)))
    rs = torch.rsqrt((x * x).mean(1) + 1e-6)
    y = rs[:, None] * (x @ Wp.T)
    (dy * y).sum().backward()
    with torch.no_grad():
        dzs = (rs[:, None] * dy).numpy()
        rc = (rs * rs * (dy * y).sum(1) / D).numpy()
    P, S = dzs @ Wp.numpy(), np.abs(dzs) @ np.abs(Wp.numpy())
    ref, _, _ = tk.rms_bwd_expected(P, S, O, np.zeros((M, D)), x.detach().numpy(), rc)
    assert np.abs(ref - x.grad.numpy()).max() <= 1e-11


def _rms_case(N, K, kind, M=256):
    A, W, x0, xs, rc = tk.rms_operands(M, N, K, kind)
    P, S = ef.gemm_products(M, N, K, kind)
    return ef.standin_acc(A, W), P, S, x0, xs, rc


@pytest.mark.parametrize("N", tk.RMS_NS)
def test_rms_bwd_standin_meets_every_bar(N):
    for K in tk.RMS_KS:
        acc, P, S, x0, xs, rc = _rms_case(N, K, "normal")
        ref, bar, bar_hi = tk.rms_bwd_expected(P, S, K, x0, xs, rc)
        m = tk.cpu_mask(256, N, 0.1, 1)
        hi, lo, dxm = tk.standin_rms_bwd(acc, x0, xs, rc, m)
        assert _within(hi + lo, ref, bar) and _within(hi, ref, bar_hi), (N, K)
        assert (dxm[m == 0] == 0).all() and np.array_equal(dxm, tk.dxm_expected(hi, lo, m))


@pytest.mark.parametrize("K", tk.RMS_KS)
def test_rms_bwd_integer_cases_are_exact(K):
    """Multiples of 1/2 below 1000 + 16 K + 8 < 2^15: exact in fp32 and in the two planes' 16 bits."""
    assert 2 * (1000 + 16 * max(tk.RMS_KS) + 8) < 2 ** 16
    acc, P, S, x0, xs, rc = _rms_case(200, K, "integer")
    assert np.array_equal(acc, P)
    ref, bar, _ = tk.rms_bwd_expected(P, S, K, x0, xs, rc, exact_acc=True)
    hi, lo, _ = tk.standin_rms_bwd(acc, x0, xs, rc)
    want_hi, want_lo = ef.split_planes_np(ref)
    assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo) and np.array_equal(hi + lo, ref)


@pytest.mark.parametrize("mutant", ["plus_rc_x", "rc_neighbour_row"])
def test_planted_rms_bwd_value_bugs_miss_the_bar(mutant):
    acc, P, S, x0, xs, rc = _rms_case(136, 192, "normal")
    ref, bar, bar_hi = tk.rms_bwd_expected(P, S, 192, x0, xs, rc)
    hi, lo, _ = tk.standin_rms_bwd(acc, x0, xs, rc, mutant=mutant)
    assert not _within(hi + lo, ref, bar) and not _within(hi, ref, bar_hi)
    # ... and the same bug in the reference's place is as far from the sound stand-in
    wrong, wbar, _ = tk.rms_bwd_expected(P, S, 192, x0, xs, rc, mutant=mutant)
    good = tk.standin_rms_bwd(acc, x0, xs, rc)
    assert not _within(good[0] + good[1], wrong, wbar)


@pytest.mark.parametrize("mutant", ["dxm_before_update", "site_for_next_site"])
def test_planted_dxm_bugs_change_its_bits(mutant):
    acc, P, S, x0, xs, rc = _rms_case(136, 192, "normal")
    m, other = tk.cpu_mask(256, 136, 0.1, 1), tk.cpu_mask(256, 136, 0.1, 2)
    assert (m != other).any()
    hi, lo, dxm = tk.standin_rms_bwd(acc, x0, xs, rc, m, other, mutant=mutant)
    assert not np.array_equal(dxm, tk.dxm_expected(hi, lo, m))


def _geglu_case(F, K, kind="normal", M=256):
    A, W, _ = ef.gemm_operands(M, 2 * F, K, kind, True)
    P, S = ef.gemm_products(M, 2 * F, K, kind, True)
    rs = np.random.default_rng([F, K]).uniform(0.5, 1.5, M).astype(np.float32).astype(np.float64)
    return ef.standin_acc(A, W), A, W, P, S, rs


def test_geglu_train_restatement_equals_torch_float64():
    acc, A, W, P, S, rs = _geglu_case(192, 128)
    m = tk.cpu_mask(256, 192, 0.5, 3)
    tA, tW = torch.from_numpy(A.copy()), torch.from_numpy(W.copy()).view(192 // 32, 2, 32, 128)
    r = torch.from_numpy(rs)[:, None]
    g, u = (tA @ tW[:, 0].reshape(-1, 128).T) * r, (tA @ tW[:, 1].reshape(-1, 128).T) * r
    want = (_hf_gelu_new(g) * u * torch.from_numpy(m)).numpy()
    assert np.abs(tk.geglu_train_expected(P, S, 128, rs, m=m)[0] - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("F", tk.FWD_FS)
def test_geglu_train_standin_meets_the_bar(F):
    for K in tk.FWD_KS:
        acc, A, W, P, S, rs = _geglu_case(F, K)
        for p in tk.DROP_PS:
            m = tk.cpu_mask(256, F, p, 4) if p else None
            ref, bar = tk.geglu_train_expected(P, S, K, rs, m=m)
            got = tk.standin_geglu_train(acc, rs, m)
            assert _within(got, ref, bar), (F, K, p)
            if p:
                assert (got[m == 0] == 0).all() and (bar[m == 0] == 0).all()


def test_planted_geglu_mask_one_column_over_misses_the_bar():
    acc, A, W, P, S, rs = _geglu_case(128, 128)
    m = tk.cpu_mask(256, 128, 0.1, 4)
    ref, bar = tk.geglu_train_expected(P, S, 128, rs, m=m)
    assert not _within(tk.standin_geglu_train(acc, rs, m, mutant="mask_one_column_over"), ref, bar)


def test_resid_train_restatement_equals_torch_float64():
    acc, P, S, x0, xs, rc = _rms_case(200, 192, "normal")
    A, W = tk.rms_operands(256, 200, 192, "normal")[:2]
    m = tk.cpu_mask(256, 200, 0.1, 5)
    want = torch.from_numpy(x0.copy()) + torch.from_numpy(m) * (torch.from_numpy(A.copy()) @ torch.from_numpy(W.copy()).T)
    assert np.abs(tk.resid_train_expected(P, S, 192, x0, m)[0] - want.numpy()).max() <= 1e-11


@pytest.mark.parametrize("N", tk.RMS_NS)
def test_resid_train_standin_meets_every_bar(N):
    for K in (128, 192):
        acc, P, S, x0, _, _ = _rms_case(N, K, "normal")
        for p in tk.DROP_PS:
            m = tk.cpu_mask(256, N, p, 6) if p else None
            ref, bar, bar_hi = tk.resid_train_expected(P, S, K, x0, m)
            hi, lo = tk.standin_resid_train(acc, x0, m)
            assert _within(hi + lo, ref, bar) and _within(hi, ref, bar_hi), (N, K, p)
            if p:
                bad = tk.standin_resid_train(acc, x0, m, mutant="mask_one_column_over")
                assert not _within(bad[0] + bad[1], ref, bar), "planted: the mask one column over"


def test_resid_train_integer_case_is_exact():
    """Integers below 1000 + 16 K < 2^15 at K <= 1472: exact in fp32 and in the two planes' 16 bits."""
    assert 1000 + 16 * max(tk.FWD_KS) < 2 ** 15
    acc, P, S, x0, _, _ = _rms_case(200, 192, "integer")
    ref, _, _ = tk.resid_train_expected(P, S, 192, x0, exact_acc=True)
    hi, lo = tk.standin_resid_train(acc, x0)
    assert np.array_equal(hi + lo, ref) and np.array_equal(hi, ef.split_planes_np(ref)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# gated-GELU backward
# ---------------------------------------------------------------------------------------------------------------------------
def _gb_case(F, K, M=256):
    A, W, g, u, rs = tk.geglu_bwd_operands(M, F, K)
    P, S = A @ W.T, np.abs(A) @ np.abs(W).T
    return ef.standin_acc(A, W), P, S, g, u, rs


def test_geglu_bwd_restatement_equals_torch_autograd():
    """ff = gelu_new(g) u (HF's NewGELUActivation), loss = sum(m dff ff): autograd's dg, du times rs are dzs; the row dot."""
    acc, P, S, g, u, rs = _gb_case(128, 64)
    m = tk.cpu_mask(256, 128, 0.1, 9)
    tg, tu = (torch.tensor(a, requires_grad=True) for a in (g, u))
    (torch.from_numpy(P * m) * _hf_gelu_new(tg) * tu).sum().backward()
    exp = tk.geglu_bwd_expected(P, S, 64, g, u, rs, m)
    r = rs[:, None]
    assert np.abs(exp["dzs_g"][0] - r * tg.grad.numpy()).max() <= 1e-11 * max(1.0, np.abs(tg.grad.numpy()).max())
    assert np.abs(exp["dzs_u"][0] - r * tu.grad.numpy()).max() <= 1e-11 * max(1.0, np.abs(tu.grad.numpy()).max())
    dot = (tg.grad.numpy() * g + tu.grad.numpy() * u).sum(1)
    assert np.abs(exp["rcoef"][0] - rs ** 2 * dot / 64).max() <= 1e-11 * max(1.0, np.abs(dot).max())


@pytest.mark.parametrize("F", tk.GB_FS)
def test_geglu_bwd_standin_meets_every_bar(F):
    """(with no fast-math allowance: numpy's exp2 and division are correctly rounded to well within the derived terms)"""
    for K in (64, 192):
        acc, P, S, g, u, rs = _gb_case(F, K)
        for p in tk.DROP_PS:
            m = tk.cpu_mask(256, F, p, 9) if p else None
            exp = tk.geglu_bwd_expected(P, S, K, g, u, rs, m, extra_dzs=0.0, extra_rcoef=0.0)
            dg, du, rc = tk.standin_geglu_bwd(acc, g, u, rs, K, m)
            for name, got in (("dzs_g", dg), ("dzs_u", du), ("rcoef", rc)):
                assert _within(got, *exp[name]), (F, K, p, name)
            assert exp["slots"][0].shape == ((F + 63) // 64, 256) and np.abs(exp["slots"][0].sum(0) * rs ** 2 / K - exp["rcoef"][0]).max() < 1e-9
            if p:
                assert (dg[m == 0] == 0).all() and (du[m == 0] == 0).all()


@pytest.mark.parametrize("mutant,misses", [("gelu_grad_without_sg", ("dzs_g", "rcoef")), ("mask_one_column_over", ("dzs_g", "dzs_u", "rcoef")),
                                           ("rs_neighbour_row", ("dzs_g", "dzs_u", "rcoef"))])
def test_planted_geglu_bwd_bugs_miss_a_bar(mutant, misses):
    acc, P, S, g, u, rs = _gb_case(192, 128)
    m = tk.cpu_mask(256, 192, 0.1, 9)
    exp = tk.geglu_bwd_expected(P, S, 128, g, u, rs, m, extra_dzs=0.0, extra_rcoef=0.0)
    got = dict(zip(("dzs_g", "dzs_u", "rcoef"), tk.standin_geglu_bwd(acc, g, u, rs, 128, m, mutant=mutant)))
    for name in got:
        assert _within(got[name], *exp[name]) == (name not in misses), (mutant, name)


def test_planted_rowdot_beyond_n_valid_is_hidden_by_the_slot_guard():
    """At np = ceil(d_ff / 64) - every caller's - a block at or beyond n_valid has slot >= np and is not stored either way."""
    acc, P, S, g, u, rs = _gb_case(192, 128)
    good = tk.standin_geglu_bwd(acc, g, u, rs, 128)
    bad = tk.standin_geglu_bwd(acc, g, u, rs, 128, mutant="rowdot_beyond_n_valid")
    assert all(np.array_equal(a, b) for a, b in zip(good, bad))


# ---------------------------------------------------------------------------------------------------------------------------
# training attention
# ---------------------------------------------------------------------------------------------------------------------------
ATT_OUTPUTS = ("att", "dq", "dk", "dv", "lse2", "delta", "dtab")


@pytest.mark.parametrize("name", ["h1-d8-std4-mixed", "h2-d8-std4-short"])
def test_attention_train_restatement_equals_torch_autograd(name):
    """loss = sum(dO . ((m softmax(q k^T + tab[clamp(j - i)])) v)): autograd's gradients of q, k, v and of the table."""
    c = tk.attention_train_case(name)
    H, maxd, inner = c["H"], c["maxd"], c["H"] * 64
    mk = tk.cpu_attention_mask(c, 0.5)
    ref = tk.attention_train_compute(c, mk)
    tab = torch.tensor(c["tab"], requires_grad=True)
    dtab = np.zeros_like(c["tab"])
    for b in list(range(len(c["lens"])))[:40]:
        s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
        pos = torch.arange(s1 - s0)
        rel = (pos[None, :] - pos[:, None]).clamp(-maxd, maxd) + maxd
        m = torch.from_numpy(mk(b, s0, s1 - s0))
        x = torch.tensor(c["qkv"][s0:s1], requires_grad=True)
        loss = 0.0
        for h in range(H):
            q, k, v = (x[:, o * inner + h * 64:o * inner + (h + 1) * 64] for o in range(3))
            P = torch.softmax(q @ k.T + tab[h][rel], dim=-1)
            o = (P * m[h]) @ v
            assert np.abs(ref["att"][s0:s1, h * 64:(h + 1) * 64] - o.detach().numpy()).max() <= 1e-11
            lse = torch.logsumexp(q @ k.T + tab[h][rel], dim=-1)
            assert np.abs(ref["lse2"][h, s0:s1] - (lse * tk.LOG2E).detach().numpy()).max() <= 1e-10
            loss = loss + (torch.from_numpy(c["datt"][s0:s1, h * 64:(h + 1) * 64]) * o).sum()
        g = torch.autograd.grad(loss, [x, tab])
        got = np.concatenate([ref["dq"][s0:s1], ref["dk"][s0:s1], ref["dv"][s0:s1]], 1)
        assert np.abs(got - g[0].numpy()).max() <= 1e-10 * max(1.0, float(g[0].abs().max()))
        dtab += g[1].numpy()
    if len(c["lens"]) <= 40:
        assert np.abs(ref["dtab"] - dtab).max() <= 1e-9 * max(1.0, np.abs(dtab).max())


@pytest.mark.parametrize("name", sorted(tk.ATT_TRAIN_CASES))
def test_attention_train_standin_meets_every_bar(name):
    c = tk.attention_train_case(name)
    for p in (0.0, 0.5) if c["H"] < 6 else (0.1,):
        mk = tk.cpu_attention_mask(c, p) if p else None
        st = tk.attention_train_compute(c, mk, f32=True)
        ref = tk.attention_train_compute(c, mk, att_used=st["att"], bars=True)
        for k in ATT_OUTPUTS:
            assert _within(st[k], ref[k], ref["bar_" + k]), (name, p, k)


@pytest.mark.parametrize("mutant,misses", [
    ("bias_sign", {"att", "dq", "dk", "dv", "lse2", "dtab"}), ("clamp_one_early", {"att", "dq", "dk", "dv", "lse2", "dtab"}),
    ("delta_neighbour_head", {"delta", "dq", "dk", "dtab"}), ("ds_without_delta", {"dq", "dk", "dtab"}),
    ("mask_on_p_only", {"dq", "dk", "dtab"})])
def test_planted_attention_bugs_miss_a_bar(mutant, misses):
    """(the table holds a value of its own per distance and the sequences are longer than 2 maxd: a diagonal off by one, a
    mirrored table and a clamp one entry early all change the logits)"""
    c = tk.attention_train_case("h2-d32-std12-mixed")
    assert max(c["lens"]) > 2 * c["maxd"] and len(set(c["tab"][0].tolist())) == 2 * c["maxd"] + 1
    mk = tk.cpu_attention_mask(c, 0.5)
    st = tk.attention_train_compute(c, mk, f32=True, mutant=mutant)
    ref = tk.attention_train_compute(c, mk, att_used=st["att"], bars=True)
    missed = {k for k in ATT_OUTPUTS if not _within(st[k], ref[k], ref["bar_" + k])}
    assert missed == misses, (mutant, missed)
