"""The encoder's forward MFMA kernels (the GEMM tiles with their four epilogues in every launch form, attention_kernel) and its
embedding / last_hidden_state / rowscale kernels alone on the MI355X, each against the float64 restatement of the same operation
(tests/encoder_forward_helpers.py: derivation of every bar in its docstring), through the test-only entry points
rp_dbg_gemm_ex, rp_dbg_attention_ex, rp_dbg_encoder_rows and rp_dbg_rowscale, which run the launch code encode_pass runs
(DESIGN.md section 11).  tests/test_encoder_forward_kernels_cpu.py shows on the same shapes that the bars hold for a float32
stand-in and separate planted bugs.

Every operand has NaN guard rows behind its last row (an over-read shows as a NaN in the result, not as a fault); every output
is pre-filled with a sentinel (bf16 0xFFFF, bytes 0x5A, fp32 NaN) and has guard rows of its own.  Every GEMM case asserts the
`plan` rp_dbg_gemm_ex reports: the tile configuration and the launch form it names are the ones that ran.

Token rows under tokens_valid / t_dev, as read in launch_gemm_cfg, gemm_kernel_body and the epilogues: only the token tiles up
to the count are launched; inside the last one the rows from the count on are READ as copies of the last valid row (the
operand's row clamp), go through the epilogue with their OWN row's factor and old x, and are WRITTEN.  So: rows below the count
carry the bits of the full call; a padding row of the last tile carries the last valid row's bits wherever its own inputs
(old x; no row factor) equal that row's; rows from the end of the last launched tile on keep the sentinel.

RP_ENC_FWD_MARGINS_OUT=<path>: every measured value and bar is written there as JSON
(profiles/encoder_forward_kernel_margins.json)."""
import contextlib
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_forward_helpers as ef  # noqa: E402
import hip_helpers as hh  # noqa: E402
from reprover_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGINS = {}
RP_E_INVALID = -1
GUARD_ROWS = 8
ALL_VARIANTS = (0, 9, 15, 16, 17, 26, 30)
EPIS = (ef.EPI_STORE, ef.EPI_RESID, ef.EPI_GEGLU, ef.EPI_RESID8)
OPTIONS = ("gemm_variant_o", "gemm_skinny", "gemm_small_pipe", "gemm_helpers", "gemm_persist", "gemm_mixed", "gemm_edge_layout")
CLASS_OF = {ef.EPI_STORE: ef.K_QKV, ef.EPI_GEGLU: ef.K_WI, ef.EPI_RESID: ef.K_WO, ef.EPI_RESID8: ef.K_WO}
VE = [pytest.param(v, e, id=f"v{v}-{ef.EPI_NAMES[e]}") for v in ALL_VARIANTS for e in EPIS]


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("RP_ENC_FWD_MARGINS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def defaults():
    """The options' values as the library holds them when this module first asks (no test has changed one yet: every change
    goes through options() below, which puts them back), + gemm_variant_all = -1, the compound option's "all four at their
    defaults"."""
    lib, out = _lib.load(), dict(gemm_variant_all=-1)
    for name in OPTIONS:
        v = ctypes.c_int32(-12345)
        _lib.check(lib.rp_dbg_get_option(name.encode(), ctypes.byref(v)), name)
        out[name] = v.value
    assert out["gemm_variant_o"] == -1 and out["gemm_skinny"] == 1, out  # (what gemm_variant_all = -1 and forced() rely on)
    return out


@contextlib.contextmanager
def options(**kw):
    """Options for the calls inside, every one of them back at the value the library held afterwards."""
    lib = _lib.load()
    saved = defaults()
    try:
        for k, v in kw.items():
            _lib.check(lib.rp_set_option(k.encode(), v), k)
        yield
    finally:
        for k in kw:
            if k == "gemm_variant_o":  # (its own option takes tile ids only: "by pass size" comes back with the defaults of all four)
                assert "gemm_variant_all" not in kw
                k = "gemm_variant_all"
            _lib.check(lib.rp_set_option(k.encode(), saved[k]), k)


def forced(variant):
    """One tile configuration for every class, the few-token switch off; 16 stays 16 only with the pipelined small tile off."""
    return options(gemm_skinny=0, gemm_variant_all=variant, gemm_small_pipe=0 if variant == 16 else 1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cached operands are read-only)
    return t if dtype is None else t.to(dtype)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _operand(a64, ld=None):
    """bf16 [rows + GUARD_ROWS, ld]: the values, NaN in the columns beyond them and in the guard rows behind the last row."""
    rows, cols = a64.shape
    t = torch.full((rows + GUARD_ROWS, ld or cols), float("nan"), dtype=torch.bfloat16, device=DEV)
    t[:rows, :cols] = _dev(a64, torch.bfloat16)
    return t


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Gemm:
    """One rp_dbg_gemm_ex call: buffers with sentinels and guards, the call, the decoded outputs."""

    def __init__(self, epi, A, W, n_valid, x0=None, lda=None, ldo=None, prof_class=None, tokens_valid=0, t_dev=None,
                 rs_form=0, ssp_in=None, inv_d=0.0, np_out=0):
        self.epi, self.M, self.K, self.n = epi, A.shape[0], A.shape[1], n_valid
        self.cols = n_valid // 2 if epi == ef.EPI_GEGLU else n_valid
        self.ldo = ldo or (self.cols + 7) // 8 * 8
        self.lda = lda or self.K
        M, ldo = self.M, self.ldo
        self.A, self.W = _operand(A, self.lda), _operand(W)
        x0 = None if x0 is None else x0[:, :n_valid]
        self.n_rows_w = W.shape[0]
        rows = M + GUARD_ROWS
        if epi in (ef.EPI_STORE, ef.EPI_GEGLU):
            self.buf = torch.full((rows, ldo), -1, dtype=torch.int16, device=DEV)
        elif epi == ef.EPI_RESID:
            self.buf = torch.full((2 * M + GUARD_ROWS, ldo), -1, dtype=torch.int16, device=DEV)
            pl = hh.split_planes(_dev(x0, torch.float32))
            self.buf[:M, :n_valid] = pl[0].view(torch.int16)
            self.buf[M:2 * M, :n_valid] = pl[1].view(torch.int16)
        else:
            self.buf = torch.full(((3 * M + GUARD_ROWS) * ldo,), 0x5A, dtype=torch.uint8, device=DEV)
            self.buf[:2 * M * ldo].view(torch.int16).fill_(-1)
            _, hi, ext = hh.split_x24(_dev(x0, torch.float32))
            self.hi_view()[:, :n_valid] = hi.view(torch.int16)
            self.ext_view()[:, :n_valid] = ext
        self.before = self.buf.clone()
        self.ssp = torch.full((np_out + 1, M), float("nan"), dtype=torch.float32, device=DEV) if np_out else None
        self.np_out = np_out
        self.ssp_in = None if ssp_in is None else _dev(ssp_in, torch.float32)
        self.rs_buf = torch.full((M + 1,), float("nan"), dtype=torch.float32, device=DEV) if rs_form == 1 else None
        self.plan = (ctypes.c_int32 * 6)(*([-7] * 6))
        self.t_dev = None if t_dev is None else torch.tensor([t_dev], dtype=torch.int32, device=DEV)
        self.args = (prof_class or CLASS_OF[epi], tokens_valid, rs_form, inv_d)

    def hi_view(self):
        return self.buf[:2 * self.M * self.ldo].view(torch.int16).view(self.M, self.ldo)

    def ext_view(self):
        return self.buf[2 * self.M * self.ldo:3 * self.M * self.ldo].view(self.M, self.ldo)

    def call(self):
        prof_class, tokens_valid, rs_form, inv_d = self.args
        st = _lib.load().rp_dbg_gemm_ex(
            _lib.ptr(self.A), self.lda, _lib.ptr(self.W), self.n_rows_w, _lib.ptr(self.buf), self.ldo, self.M, self.K, self.n,
            self.epi, prof_class, tokens_valid, _lib.ptr(self.t_dev), rs_form, _lib.ptr(self.ssp_in),
            0 if self.ssp_in is None else self.ssp_in.shape[0], inv_d, ef.EPS, _lib.ptr(self.rs_buf), _lib.ptr(self.ssp),
            self.np_out, self.plan, _lib.current_stream())
        torch.cuda.synchronize()
        return st

    def run(self):
        _lib.check(self.call(), "rp_dbg_gemm_ex")
        return self

    @property
    def variant(self):
        return self.plan[0]

    @property
    def form(self):
        return self.plan[1]

    def planes(self):
        """The written region as raw planes: a list of 2-D integer tensors [M, cols]."""
        M, c = self.M, self.cols
        if self.epi in (ef.EPI_STORE, ef.EPI_GEGLU):
            return [self.buf[:M, :c]]
        if self.epi == ef.EPI_RESID:
            return [self.buf[:M, :c], self.buf[M:2 * M, :c]]
        return [self.hi_view()[:, :c], self.ext_view()[:, :c]]

    def values(self, rows=None):
        """float64 [rows, cols]: the bf16 output, or x decoded from the planes."""
        r = slice(0, self.M) if rows is None else rows
        pl = [p[r] for p in self.planes()]
        if self.epi in (ef.EPI_STORE, ef.EPI_GEGLU):
            return _f64(pl[0].contiguous().view(torch.bfloat16))
        if self.epi == ef.EPI_RESID:
            return _f64(pl[0].contiguous().view(torch.bfloat16)) + _f64(pl[1].contiguous().view(torch.bfloat16))
        return hh.merge_x24(pl[0].contiguous().view(torch.bfloat16), pl[1].contiguous()).cpu().numpy().astype(np.float64)

    def outside_untouched(self, rows_written=None):
        """Everything but rows [0, rows_written) x the valid columns holds what it held before the call."""
        now, was = self.buf.clone(), self.before.clone()
        rw = self.M if rows_written is None else rows_written

        def blank(t):
            if self.epi in (ef.EPI_STORE, ef.EPI_GEGLU):
                t[:rw, :self.cols] = 0
            elif self.epi == ef.EPI_RESID:
                t[:rw, :self.cols] = 0
                t[self.M:self.M + rw, :self.cols] = 0
            else:
                M, ldo = self.M, self.ldo
                t[:2 * M * ldo].view(torch.int16).view(M, ldo)[:rw, :self.cols] = 0
                t[2 * M * ldo:3 * M * ldo].view(M, ldo)[:rw, :self.cols] = 0
        blank(now)
        blank(was)
        ok = torch.equal(now, was)
        if self.ssp is not None:
            ok = ok and bool(torch.isnan(self.ssp[self.np_out]).all()) and bool(torch.isnan(self.ssp[:, rw:]).all())
        return ok

    def all_written(self, rows_written=None):
        rw = self.M if rows_written is None else rows_written
        p = self.planes()[0][:rw]
        return not bool((p == -1).any())


def _check(g, P, S, x0, rs, rs_rel, what, margins, rows=None, exact=False):
    """The call's values (and statistic) against the float64 reference, per element."""
    r = slice(0, g.M) if rows is None else rows
    n = g.n
    ref, bar = ef.gemm_expected(g.epi, P[r, :n], S[r, :n], g.K, None if x0 is None else x0[r, :n], None if rs is None else rs[r],
                                rs_rel, exact_acc=exact)
    got = g.values(r)
    found = ef.findings(what, got, ref, bar, margins)
    if g.epi == ef.EPI_GEGLU:
        exc = float((np.abs(got - ref) - (bar - ef.FASTMATH_ENC_GEGLU)).max())
        e = MARGINS.setdefault("geglu_fastmath_excess", {})
        e[what] = max(e.get(what, -1.0), exc)
    if g.epi == ef.EPI_RESID:  # the hi plane alone: the next projection's operand, one bf16 rounding of x
        hi = _f64(g.planes()[0][r].contiguous().view(torch.bfloat16))
        found += ef.findings(what + " hi", hi, ref, bar + ef.bf16_half_ulp(ref, bar), margins)
    if g.ssp is not None:
        sref, sbar = ef.ssp_reference(got, g.np_out)
        found += ef.findings(what + " ssp", g.ssp[:g.np_out, r].cpu().numpy(), sref, sbar, margins)
    return found


def _ssp_in(M, np_, seed=0):
    rng = np.random.default_rng([seed, M, np_])
    return (rng.uniform(0.2, 3.0, (np_, M)) * 64).astype(np.float32)


def _np_out(epi, n):
    return (n + 63) // 64 if epi in (ef.EPI_RESID, ef.EPI_RESID8) else 0


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: integer operands, every tile configuration x every epilogue x every k-tile count
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,epi", VE)
def test_gemm_integer_operands_are_exact(variant, epi):
    M, N = 256, ef.N_MAX
    geglu = epi == ef.EPI_GEGLU
    m = MARGINS.setdefault("gemm_integer", {})
    found = []
    with forced(variant):
        for K in ef.ks_of(variant):
            A, W, x0 = ef.gemm_operands(M, N, K, "integer", geglu)
            P, S = ef.gemm_products(M, N, K, "integer", geglu)
            g = Gemm(epi, A, W, N, x0, np_out=_np_out(epi, N)).run()
            assert (g.variant, g.form) == (ef.expected_variant(variant, M, K, variant != 16), ef.FORM_TILE), list(g.plan)
            assert g.outside_untouched() and g.all_written()
            pl = g.planes()
            if epi == ef.EPI_STORE:
                assert np.array_equal(_f64(pl[0].contiguous().view(torch.bfloat16)), ef.bf16_round(P)), K
            elif epi == ef.EPI_RESID:
                want = hh.split_planes(torch.from_numpy((x0 + P).astype(np.float32)))
                assert np.array_equal(_bf16_bits(pl[0]), _bf16_bits(want[0])) and np.array_equal(_bf16_bits(pl[1]), _bf16_bits(want[1])), K
            elif epi == ef.EPI_RESID8:
                hi, ext = ef.split_x24_np(x0 + P)
                assert np.array_equal(_bf16_bits(pl[0]), hi) and np.array_equal(pl[1].cpu().numpy(), ext), K
            if epi in (ef.EPI_RESID, ef.EPI_RESID8):
                assert np.array_equal(g.values(), x0 + P)
            found += _check(g, P, S, x0, None, 0.0, f"v{variant}-{ef.EPI_NAMES[epi]}", m, exact=True)
    assert not found, found


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: N(0, 1) operands within the derived bar, per element
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,epi", VE)
def test_gemm_random_operands_within_the_derived_bar(variant, epi):
    """K over the family's list + 3584, 7168; the last feature tile holding 8 .. 256 valid features with a weight operand of
    exactly that many rows; lda > K and ldo > n on every other case; the row factor through rowscale_kernel on every other."""
    M = 256
    geglu = epi == ef.EPI_GEGLU
    m = MARGINS.setdefault("gemm_random", {})
    found = []
    ssp_in = _ssp_in(M, 23)
    rs = ef.rs_reference(ssp_in, 1.0 / 1472)
    with forced(variant):
        for ik, K in enumerate(ef.ks_of(variant) + ef.KS_LONG):
            A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", geglu)
            P, S = ef.gemm_products(M, ef.N_MAX, K, "normal", geglu)
            for i_n, n in enumerate(ef.N_VALIDS):
                if geglu and n % 64:
                    continue
                odd = (ik + i_n) % 2 == 1
                use_rs = odd and epi in (ef.EPI_STORE, ef.EPI_GEGLU)
                g = Gemm(epi, A, W[:n], n, x0, lda=K + 8 if odd else None, ldo=n + 8 if odd else None, rs_form=1 if use_rs else 0,
                         ssp_in=ssp_in if use_rs else None, inv_d=1.0 / 1472, np_out=_np_out(epi, n)).run()
                assert (g.variant, g.form, g.plan[3]) == (ef.expected_variant(variant, M, K, variant != 16), ef.FORM_TILE,
                                                         M // ef.VARIANTS[g.variant][1]), list(g.plan)
                assert g.plan[2] == -(-n // ef.VARIANTS[g.variant][0])
                assert g.outside_untouched() and g.all_written(), (K, n)
                found += _check(g, P, S, x0, rs if use_rs else None, ef.rs_rel_bar(23) if use_rs else 0.0,
                                f"v{variant}-{ef.EPI_NAMES[epi]}", m)
    assert not found, found


@pytest.mark.parametrize("M,variant", [(128, 0), (384, 0), (512, 0), (512, 17), (512, 26), (768, 9), (768, 15), (768, 30)])
def test_gemm_token_extents(M, variant):
    """M = 128 and 384 admit the 128 x 128 tile only (pick_gemm_variant sends every other request there); 512 and 768 are
    two and three token tiles of 256."""
    K = 256
    m = MARGINS.setdefault("gemm_token_extents", {})
    found = []
    for epi in EPIS:
        geglu = epi == ef.EPI_GEGLU
        A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", geglu)
        P, S = ef.gemm_products(M, ef.N_MAX, K, "normal", geglu)
        with forced(variant if M % 256 == 0 else 26):
            g = Gemm(epi, A, W[:192], 192, x0, np_out=_np_out(epi, 192)).run()
        assert (g.variant, g.form, g.plan[3]) == (variant, ef.FORM_TILE, M // ef.VARIANTS[variant][1]), list(g.plan)
        assert g.outside_untouched() and g.all_written()
        found += _check(g, P, S, x0, None, 0.0, f"M{M}-v{variant}-{ef.EPI_NAMES[epi]}", m)
    assert not found, found


@pytest.mark.parametrize("variant", ef.SMALL_VARIANTS)
@pytest.mark.parametrize("epi", [ef.EPI_STORE, ef.EPI_GEGLU], ids=["store", "geglu"])
def test_gemm_row_scale_from_slots(variant, epi):
    """launch_gemm<true>: the epilogue sums the statistic slots itself (np = 1, 2, 23, 24, 32), and gives the bits of the
    rowscale_kernel + RowScale form."""
    M, n = 256, 192
    m = MARGINS.setdefault("gemm_row_scale_from_slots", {})
    found = []
    with forced(variant):
        for K in (ef.ks_of(variant)[1], ef.ks_of(variant)[-1]):
            A, W, _ = ef.gemm_operands(M, ef.N_MAX, K, "normal", epi == ef.EPI_GEGLU)
            P, S = ef.gemm_products(M, ef.N_MAX, K, "normal", epi == ef.EPI_GEGLU)
            for np_ in (1, 2, 23, 24, 32):
                ssp_in = _ssp_in(M, np_, seed=K)
                rs = ef.rs_reference(ssp_in, 1.0 / (64 * np_))
                g = Gemm(epi, A, W[:n], n, rs_form=2, ssp_in=ssp_in, inv_d=1.0 / (64 * np_)).run()
                assert (g.variant, g.form) == (ef.expected_variant(variant, M, K, variant != 16), ef.FORM_TILE), list(g.plan)
                assert g.outside_untouched() and g.all_written()
                found += _check(g, P, S, None, rs, ef.rs_rel_bar(np_), f"v{variant}-{ef.EPI_NAMES[epi]}", m)
                g1 = Gemm(epi, A, W[:n], n, rs_form=1, ssp_in=ssp_in, inv_d=1.0 / (64 * np_)).run()
                assert list(g1.plan) == list(g.plan), (list(g1.plan), list(g.plan))
                assert torch.equal(g.buf, g1.buf), "the bits of the rowscale_kernel + RowScale form"
                rsk = g1.rs_buf[:M].cpu().numpy().astype(np.float64)
                found += ef.findings(f"rowscale np={np_}", rsk, rs, ef.rs_rel_bar(np_) * rs, m)
                assert bool(torch.isnan(g1.rs_buf[M:]).all())
    assert not found, found


def test_gemm_row_scale_from_slots_is_refused_on_the_big_tiles():
    A, W, _ = ef.gemm_operands(256, ef.N_MAX, 128, "normal")
    with forced(26):
        g = Gemm(ef.EPI_STORE, A, W, 256, rs_form=2, ssp_in=_ssp_in(256, 23), inv_d=1.0 / 1472)
        assert g.call() == RP_E_INVALID and torch.equal(g.buf, g.before) and list(g.plan) == [-7] * 6


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: placement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,epi", VE)
def test_gemm_one_live_row_and_one_live_feature(variant, epi):
    """One token row of A alone non-zero, then one feature of W alone (a gated-GELU feature: its gate and its up row): the live
    row / column carries the bits it has in the full call, everything else written is exactly zero (STORE / GEGLU) or keeps its
    old value to the bit (the residual forms); beyond the valid columns and rows the sentinel stays."""
    M, n = 256, 200 if epi != ef.EPI_GEGLU else 192
    K = ef.ks_of(variant)[2]
    geglu = epi == ef.EPI_GEGLU
    A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", geglu)
    W = W[:n]
    with forced(variant):
        full = Gemm(epi, A, W, n, x0).run()
        assert full.variant == ef.expected_variant(variant, M, K, variant != 16)
        for row in ef.PLACEMENT_ROWS:
            A1 = np.zeros_like(A)
            A1[row] = A[row]
            g = Gemm(epi, A1, W, n, x0).run()
            assert (g.variant, g.form) == (full.variant, ef.FORM_TILE) and g.outside_untouched()
            for p, pf, p0 in zip(g.planes(), full.planes(), Gemm(epi, A1, W, n, x0).planes()):
                assert torch.equal(p[row], pf[row]), (row, "the live row has the bits of the full call")
                rest = torch.ones(M, dtype=torch.bool, device=DEV)
                rest[row] = False
                if epi in (ef.EPI_STORE, ef.EPI_GEGLU):
                    assert not bool(p[rest].any()), (row, "every other row is +0")
                else:
                    assert torch.equal(p[rest], p0[rest]), (row, "every other row keeps its old value to the bit")
        cols = g.cols
        for f in ef.PLACEMENT_FEATURES:
            f = cols - 1 if f < 0 else f
            W1 = np.zeros_like(W)
            live = [64 * (f // 32) + f % 32, 64 * (f // 32) + 32 + f % 32] if geglu else [f]
            W1[live] = W[live]
            g = Gemm(epi, A, W1, n, x0).run()
            assert (g.variant, g.form) == (full.variant, ef.FORM_TILE) and g.outside_untouched()
            for p, pf, p0 in zip(g.planes(), full.planes(), Gemm(epi, A, W1, n, x0).planes()):
                assert torch.equal(p[:, f], pf[:, f]), (f, "the live feature has the bits of the full call")
                rest = torch.ones(cols, dtype=torch.bool, device=DEV)
                rest[f] = False
                if epi in (ef.EPI_STORE, ef.EPI_GEGLU):
                    assert not bool(p[:, rest].any()), (f, "every other feature is +0")
                else:
                    assert torch.equal(p[:, rest], p0[:, rest]), (f, "every other feature keeps its old value to the bit")


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: tokens_valid and t_dev
# ---------------------------------------------------------------------------------------------------------------------------
def _x0_with_copied_tail(x0, tv):
    x = x0.copy()
    x[tv:] = x[tv - 1]
    return x


def _token_count_case(epi, A, W, n, x0, tv, full, variant, helpers, t_dev=False, K=None):
    """One call under a token count (host side, or on the device with the grid sized for all M rows): see the module docstring."""
    M = A.shape[0]
    bn = ef.VARIANTS[variant][1]
    g = Gemm(epi, A, W, n, _x0_with_copied_tail(x0, tv), tokens_valid=0 if t_dev else tv, t_dev=tv if t_dev else None,
             np_out=_np_out(epi, n)).run()
    tiles_t = -(-tv // bn)
    end = min(M, tiles_t * bn)
    assert g.variant == variant and g.form == ef.FORM_TILE and g.plan[3] == (M // bn if t_dev else tiles_t), list(g.plan)
    assert (g.plan[4] > 0) == helpers, list(g.plan)
    assert g.outside_untouched(end) and g.all_written(end), tv
    for p, pf in zip(g.planes(), full.planes()):
        assert torch.equal(p[:tv], pf[:tv]), (tv, "rows below the count: the bits of the full call")
        assert torch.equal(p[tv:end], p[tv - 1:tv].expand(end - tv, -1)), (tv, "padding rows of the last tile: the last valid row's bits")
    if g.ssp is not None:
        assert torch.equal(g.ssp[:g.np_out, :tv], full.ssp[:g.np_out, :tv])
        assert torch.equal(g.ssp[:g.np_out, tv:end], g.ssp[:g.np_out, tv - 1:tv].expand(-1, end - tv))
    return g


@pytest.mark.parametrize("variant", [0, 17, 26])
@pytest.mark.parametrize("helpers", [False, True], ids=["plain", "helpers"])
def test_gemm_tokens_valid(variant, helpers):
    """helpers: a weight operand of 2 MiB (N = K = 1024) in a launch of at most half the chip: the surplus workgroups prefetch
    it (plan.n_helpers > 0) and change no bit."""
    M = 512
    N, K = (1024, 1024) if helpers else (ef.N_MAX, 256)
    m = MARGINS.setdefault("gemm_tokens_valid", {})
    found = []
    with forced(variant), options(gemm_helpers=64 if helpers else 0):
        for epi in EPIS:
            geglu = epi == ef.EPI_GEGLU
            A, W, x0 = ef.gemm_operands(M, N, K, "normal", geglu)
            n = N if helpers else 192
            full = Gemm(epi, A, W[:n], n, x0, np_out=_np_out(epi, n)).run()
            assert full.variant == variant and (full.plan[4] > 0) == helpers, list(full.plan)
            P, S = ef.gemm_products(M, N, K, "normal", geglu)
            found += _check(full, P, S, x0, None, 0.0, f"v{variant}-{ef.EPI_NAMES[epi]}-{'helpers' if helpers else 'plain'}", m)
            for tv in ef.TOKENS_VALID:
                if tv < M:
                    _token_count_case(epi, A, W[:n], n, x0, tv, full, variant, helpers)
    assert not found, found


@pytest.mark.parametrize("variant", [17, 26])
def test_gemm_device_side_token_count_per_tile_form(variant):
    """t_dev (rp_encode_padded): the grid covers all M rows, the kernel re-numbers the live tiles; rows below the count carry the
    bits of the host-side tokens_valid call, everything past the last live tile is untouched."""
    M, K, n = 768, 256, 192
    bn = ef.VARIANTS[variant][1]
    with forced(variant), options(gemm_helpers=0):
        for epi in EPIS:
            A, W, x0 = ef.gemm_operands(M, ef.N_MAX, K, "normal", epi == ef.EPI_GEGLU)
            full = Gemm(epi, A, W[:n], n, x0, np_out=_np_out(epi, n)).run()
            for tv in (1, bn - 1, bn, bn + 1, M):
                if tv == M:
                    g = Gemm(epi, A, W[:n], n, x0, t_dev=M, np_out=_np_out(epi, n)).run()
                    assert torch.equal(g.buf, full.buf) and list(g.plan) == list(full.plan), list(g.plan)
                    assert (g.variant, g.form) == (variant, ef.FORM_TILE)
                    continue
                host = _token_count_case(epi, A, W[:n], n, x0, tv, full, variant, False)
                dev = _token_count_case(epi, A, W[:n], n, x0, tv, full, variant, False, t_dev=True)
                assert torch.equal(host.buf, dev.buf), (tv, "the bits of the host-side tokens_valid call")


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: the persistent and the mixed launch forms against float64
# ---------------------------------------------------------------------------------------------------------------------------
def _form_shape(kind):
    return ef.smallest_form_shapes(n_cus())[kind]


def _big_check(g, A, W, x0, what, margins, block=1024):
    found = []
    for r0 in range(0, g.M, block):
        r = slice(r0, min(g.M, r0 + block))
        P, S = A[r] @ W.T, np.abs(A[r]) @ np.abs(W).T
        ref, bar = ef.gemm_expected(g.epi, P[:, :g.n], S[:, :g.n], g.K, None if x0 is None else x0[r, :g.n])
        got = g.values(r)
        found += ef.findings(what, got, ref, bar, margins)
        if g.epi == ef.EPI_GEGLU:
            e = MARGINS.setdefault("geglu_fastmath_excess", {})
            e[what] = max(e.get(what, -1.0), float((np.abs(got - ref) - (bar - ef.FASTMATH_ENC_GEGLU)).max()))
        if g.ssp is not None:
            sref, sbar = ef.ssp_reference(got, g.np_out)
            found += ef.findings(what + " ssp", g.ssp[:g.np_out, r].cpu().numpy(), sref, sbar, margins)
    return found


# (kind of shape, epilogue, class, options over the defaults, valid features of the last feature tile); the attention-out class
# picks the 128 x 128 tile below 57344 tokens unless gemm_variant_o names the big one
FORM_CASES = [
    ("persist", ef.EPI_STORE, ef.K_QKV, {}, 256), ("persist", ef.EPI_STORE, ef.K_QKV, {}, 128),
    ("persist", ef.EPI_STORE, ef.K_QKV, {}, 192), ("persist", ef.EPI_GEGLU, ef.K_WI, {}, 256),
    ("persist", ef.EPI_GEGLU, ef.K_WI, {}, 128), ("persist", ef.EPI_RESID8, ef.K_WO, dict(gemm_persist=16, gemm_mixed=0), 192),
    ("persist", ef.EPI_RESID, ef.K_WO, dict(gemm_persist=16, gemm_mixed=0), 128),
    ("mixed", ef.EPI_RESID8, ef.K_WO, {}, 256), ("mixed", ef.EPI_RESID8, ef.K_O, dict(gemm_variant_o=26), 128),
    ("mixed", ef.EPI_RESID8, ef.K_WO, {}, 192), ("mixed", ef.EPI_RESID, ef.K_WO, {}, 192),
    ("mixed", ef.EPI_STORE, ef.K_QKV, dict(gemm_mixed=1, gemm_persist=0), 128),
    ("mixed_tail", ef.EPI_RESID8, ef.K_WO, {}, 256), ("mixed_tail", ef.EPI_RESID8, ef.K_O, dict(gemm_variant_o=26), 128),
    ("mixed_tail", ef.EPI_RESID8, ef.K_WO, {}, 192), ("mixed_tail", ef.EPI_RESID, ef.K_O, dict(gemm_variant_o=26), 256),
    ("mixed_tail", ef.EPI_STORE, ef.K_QKV, dict(gemm_mixed=1, gemm_persist=0), 192),
]


@pytest.mark.parametrize("kind,epi,cls,opts,last", [pytest.param(*c, id=f"{c[0]}-{ef.EPI_NAMES[c[1]]}-c{c[2]}-last{c[4]}")
                                                    for c in FORM_CASES])
def test_gemm_persistent_and_mixed_forms_against_float64(kind, epi, cls, opts, last):
    """Shapes from the device's CU count (plan_mixed and the n_grid > slots rule restated in the helpers): the smallest with
    more tiles than persistent workgroups, with a mixed plan without and with half tiles handed out last.  K = 128 (192 for the
    first case of each kind); the same shape at K = 64 must fall back to one workgroup per tile."""
    tf, tt = _form_shape(kind)
    M, n = 256 * tt, 256 * (tf - 1) + last
    K = 192 if last == 256 and opts == {} and epi != ef.EPI_GEGLU and epi != ef.EPI_RESID else 128
    A, W, x0 = ef.gemm_operands(M, n, K, "normal", epi == ef.EPI_GEGLU, seed=1)
    x0 = x0 if epi in (ef.EPI_RESID, ef.EPI_RESID8) else None
    po, mo = opts.get("gemm_persist", defaults()["gemm_persist"]), opts.get("gemm_mixed", defaults()["gemm_mixed"])
    want = ef.expected_form(tf, tt, K, n_cus(), cls, po, mo, epi)
    assert want[0] == (ef.FORM_PERSIST if kind == "persist" else ef.FORM_MIXED)
    m = MARGINS.setdefault("gemm_forms", {})
    with options(gemm_skinny=0, gemm_helpers=0, **opts):
        g = Gemm(epi, A, W, n, x0, prof_class=cls, np_out=_np_out(epi, n)).run()
        assert (g.variant, g.form, g.plan[2], g.plan[3], g.plan[5]) == (26, want[0], tf, tt, want[1]), list(g.plan)
        assert g.outside_untouched() and g.all_written()
        found = _big_check(g, A, W, x0, f"{kind}-{ef.EPI_NAMES[epi]}-c{cls}-last{last}", m)
        if last == 256:  # one k-tile: the launch must fall back to one workgroup per tile (both forms need K >= 2 BK)
            g64 = Gemm(epi, A[:, :64], W[:, :64], n, x0, prof_class=cls, np_out=_np_out(epi, n)).run()
            assert (g64.variant, g64.form) == (26, ef.FORM_TILE), list(g64.plan)
            found += _big_check(g64, A[:, :64], W[:, :64], x0, f"{kind}-{ef.EPI_NAMES[epi]}-K64-per-tile", m)
    assert not found, found


def test_gemm_device_side_token_count_persistent_form():
    tf, tt = _form_shape("persist")
    M, n, K, bn = 256 * tt, 256 * (tf - 1) + 192, 128, 256
    A, W, _ = ef.gemm_operands(M, n, K, "normal", False, seed=1)
    with options(gemm_skinny=0, gemm_helpers=0):
        full = Gemm(ef.EPI_STORE, A, W, n).run()
        assert full.form == ef.FORM_PERSIST
        for tv in (1, bn - 1, bn, bn + 1, M):
            g = Gemm(ef.EPI_STORE, A, W, n, t_dev=tv).run()
            assert (g.variant, g.form, g.plan[3]) == (26, ef.FORM_PERSIST, tt), list(g.plan)
            end = min(M, -(-tv // bn) * bn)
            assert g.outside_untouched(end) and g.all_written(end)
            host = Gemm(ef.EPI_STORE, A, W, n, tokens_valid=tv).run()
            assert host.form == (ef.FORM_PERSIST if tv == M else ef.FORM_TILE)
            assert torch.equal(g.buf, host.buf), (tv, "the bits of the host-side tokens_valid call")
            assert torch.equal(g.planes()[0][:tv], full.planes()[0][:tv])


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_gemm_ex_checks_its_arguments_before_it_launches():
    A, W, x0 = ef.gemm_operands(256, ef.N_MAX, 128, "normal")
    for kw, epi in ((dict(lda=120), ef.EPI_STORE), (dict(lda=132), ef.EPI_STORE), (dict(ldo=128), ef.EPI_STORE), (dict(prof_class=3), ef.EPI_STORE),
                    (dict(tokens_valid=257), ef.EPI_STORE), (dict(rs_form=1), ef.EPI_STORE),
                    (dict(rs_form=1, ssp_in=_ssp_in(256, 4)), ef.EPI_RESID8), (dict(np_out=4), ef.EPI_STORE)):
        g = Gemm(epi, A, W, 256, x0, **{k: v for k, v in kw.items() if k != "lda"})
        g.lda = kw.get("lda", g.lda)  # (lda < K: the operand keeps its K columns, the call names fewer)
        if "rs_form" in kw and "ssp_in" not in kw:
            g.rs_buf = None
        assert g.call() == RP_E_INVALID, kw
        assert torch.equal(g.buf, g.before) and list(g.plan) == [-7] * 6, kw
    g = Gemm(ef.EPI_GEGLU, A, W[:96], 96)
    assert g.call() == RP_E_INVALID and torch.equal(g.buf, g.before)
    with forced(30):  # K = 96 is no multiple of this tile's 64: refused before the row-scale launch
        g = Gemm(ef.EPI_STORE, A[:, :96], W[:, :96], 256, rs_form=1, ssp_in=_ssp_in(256, 4), inv_d=1 / 256)
        assert g.call() == RP_E_INVALID and torch.equal(g.buf, g.before) and bool(torch.isnan(g.rs_buf).all())


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def run_attention(c, rows_extra=130):
    """-> out bf16 [T + rows_extra, H 64] as int16 bits (sentinel -1 where nothing was written); qkv has NaN rows behind T."""
    T, H = c["T"], c["H"]
    rows_total = T + rows_extra
    qkv = torch.full((rows_total + GUARD_ROWS, 3 * H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    qkv[:T] = _dev(c["qkv"], torch.bfloat16)
    out = torch.full((rows_total + GUARD_ROWS, H * 64), -1, dtype=torch.int16, device=DEV)
    tab, cu = _dev(c["tab"], torch.float32), _dev(c["cu"])
    _lib.check(_lib.load().rp_dbg_attention_ex(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(tab), _lib.ptr(out), len(c["lens"]), H,
                                               rows_total, c["maxd"], 2 * c["maxd"] + 1, _lib.current_stream()),
               "rp_dbg_attention_ex")
    torch.cuda.synchronize()
    return out


def _attention_check(c, out, name):
    T = c["T"]
    assert bool((out[T:] == -1).all()), "rows past the last sequence keep the sentinel"
    got = _f64(out[:T].contiguous().view(torch.bfloat16))
    ref, lead, f32 = ef.attention_reference(c)
    m = MARGINS.setdefault("attention", {})
    found = ef.attention_findings(name, got, ref, lead, f32, m)
    print(name, m[name])
    assert not found, found


@pytest.mark.parametrize("name", list(ef.ATTENTION_CASES))
def test_attention_against_float64(name):
    c = ef.attention_case(name)
    _attention_check(c, run_attention(c), name)


def test_attention_running_maximum_jumps_at_a_late_key_tile():
    c = ef.late_jump_case()
    out = run_attention(c)
    _attention_check(c, out, "late-jump")
    row7 = _f64(out[7:8].contiguous().view(torch.bfloat16))[0]
    assert np.abs(row7 - c["qkv"][300, 128:192]).max() < 1e-2, "row 7 is v[300]"


@pytest.mark.parametrize("name", ["h2-d32-std12-mixed", "h12-d447-std4-mixed", "h2-d128-std4-2048"])
def test_a_sequence_alone_has_the_bits_it_has_in_the_mixed_call(name):
    c = ef.attention_case(name)
    mixed = run_attention(c)
    for b in range(len(c["lens"])):
        s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
        alone = run_attention(ef.sub_attention_case(c, b), rows_extra=3)
        assert torch.equal(alone[:s1 - s0], mixed[s0:s1]), c["lens"][b]
        assert bool((alone[s1 - s0:] == -1).all())


def test_attention_ex_refuses_a_table_beyond_the_kernels():
    c = ef.make_attention_case(np.random.default_rng(0), 1, 448, 4.0, (64,))
    with pytest.raises(_lib.HipLibraryError):
        run_attention(c)
    lib = _lib.load()
    out = torch.full((64, 64), -1, dtype=torch.int16, device=DEV)
    qkv, tab, cu = _dev(c["qkv"], torch.bfloat16), _dev(c["tab"], torch.float32), _dev(c["cu"])
    for maxd, ntab in ((448, 897), (32, 64), (0, 1)):
        assert lib.rp_dbg_attention_ex(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(tab), _lib.ptr(out), 1, 1, 64, maxd, ntab,
                                       _lib.current_stream()) == RP_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == -1).all())


# ---------------------------------------------------------------------------------------------------------------------------
# embedding rows, last_hidden_state rows, rowscale
# ---------------------------------------------------------------------------------------------------------------------------
def rows_call(mode, a=None, b=None, c=None, d=None, ia=None, t_dev=None, T=0, rows=1, n=8, vocab=0, np_=0, inv_d=0.0,
              o0=None, o1=None, o2=None, o3=None):
    st = _lib.load().rp_dbg_encoder_rows(mode, _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(d), _lib.ptr(ia), _lib.ptr(t_dev),
                                         T, rows, n, vocab, np_, inv_d, ef.EPS, _lib.ptr(o0), _lib.ptr(o1), _lib.ptr(o2),
                                         _lib.ptr(o3), _lib.current_stream())
    torch.cuda.synchronize()
    return st


@pytest.fixture(scope="module")
def tables():
    """D -> the table encoded on the device (mode 0), checked once against the host's encoding, with NaN guard rows."""
    out = {}
    V = ef.EMBED_VOCAB
    for D in ef.EMBED_DS:
        table = ef.embed_table(D)
        src = torch.full((V + GUARD_ROWS, D), float("nan"), dtype=torch.float32, device=DEV)
        src[:V] = _dev(table)
        hi = torch.full((V + GUARD_ROWS, D), -1, dtype=torch.int16, device=DEV)
        lo = torch.full((V + GUARD_ROWS, D), 0x5A, dtype=torch.uint8, device=DEV)
        ss = torch.full((V + GUARD_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
        assert rows_call(0, a=src, rows=V, n=D, vocab=V, o0=hi, o1=lo, o2=ss) == 0
        out[D] = (table, hi, lo, ss)
    return out


@pytest.mark.parametrize("D", ef.EMBED_DS)
def test_embed_table_is_the_hosts_24_bit_encoding_bit_for_bit(tables, D):
    table, hi, lo, ss = tables[D]
    V = ef.EMBED_VOCAB
    hi_ref, ext_ref, x = ef.embed_table_reference(table)
    assert np.array_equal(_bf16_bits(hi[:V]), hi_ref) and np.array_equal(lo[:V].cpu().numpy(), ext_ref)
    assert np.array_equal(ss[:V].cpu().numpy().view(np.uint32), ef.embed_ss_standin(x).view(np.uint32)), "embed_ss, bit for bit"
    assert bool((hi[V:] == -1).all()) and bool((lo[V:] == 0x5A).all()) and bool(torch.isnan(ss[V:]).all())


@pytest.mark.parametrize("D", ef.EMBED_DS)
@pytest.mark.parametrize("Tp", [512, 8192], ids=["few", "many"])
def test_embed_copy_rows(tables, D, Tp):
    """The four template forms (NV by D <= 1536, R by Tp < 8192): planes are table rows bit for bit, ids clamped to [0, V - 1],
    rows T .. Tp token 0; the statistic in slot 0 with slots 1 .. np - 1 zero, or rs = rowscale_kernel's bits on those slots;
    the device-side count at 1, 255, 256, 257, T."""
    table, thi, tlo, tss = tables[D]
    V, np_ = ef.EMBED_VOCAB, (D + 63) // 64
    T = Tp - 57
    ids = ef.embed_ids(T)
    ids_d = torch.full((Tp + GUARD_ROWS,), 2 ** 31 - 1, dtype=torch.int32, device=DEV)  # (a read past T would clamp to V - 1)
    ids_d[:T] = _dev(ids)
    slots = torch.zeros((np_, Tp), dtype=torch.float32, device=DEV)
    for rs_on in (False, True):
        for t_live in (None, 1, 255, 256, 257, T):
            xhi = torch.full((Tp + GUARD_ROWS, D), -1, dtype=torch.int16, device=DEV)
            xlo = torch.full((Tp + GUARD_ROWS, D), 0x5A, dtype=torch.uint8, device=DEV)
            ssp = torch.full((np_ + 1, Tp), float("nan"), dtype=torch.float32, device=DEV)
            rs = torch.full((Tp + GUARD_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
            td = None if t_live is None else torch.tensor([t_live], dtype=torch.int32, device=DEV)
            assert rows_call(1, a=thi, b=tlo, c=tss, ia=ids_d, t_dev=td, T=T, rows=Tp, n=D, vocab=V, np_=np_, inv_d=1.0 / D,
                             o0=xhi, o1=xlo, o2=ssp, o3=rs if rs_on else None) == 0
            src, rows = ef.embed_rows_reference(ids, V, T, Tp, t_live)
            src_d = _dev(src)
            what = (D, Tp, rs_on, t_live)
            assert torch.equal(xhi[:rows], thi[src_d]) and torch.equal(xlo[:rows], tlo[src_d]), what
            assert bool((xhi[rows:] == -1).all()) and bool((xlo[rows:] == 0x5A).all()), what
            if rs_on:
                slots.zero_()
                slots[0, :rows] = tss[src_d]
                want = hh.rowscale(slots, 1.0 / D)
                assert torch.equal(rs[:rows].view(torch.int32), want[:rows].view(torch.int32)), what
                assert bool(torch.isnan(rs[rows:]).all()) and bool(torch.isnan(ssp).all()), what
            else:
                assert torch.equal(ssp[0, :rows].view(torch.int32), tss[src_d].view(torch.int32)), what
                assert not bool(ssp[1:np_, :rows].view(torch.int32).any()), "slots 1 .. np - 1 are +0"
                assert bool(torch.isnan(ssp[:, rows:]).all()) and bool(torch.isnan(ssp[np_]).all()) and bool(torch.isnan(rs).all())


@pytest.mark.parametrize("D", ef.EMBED_DS)
def test_hidden_out_rows(tables, D):
    """bf16(w (x rs)) within one rounding of float64; the zero row (token 5) exactly zero, the row of magnitude 1e4 (6) in."""
    table, thi, tlo, tss = tables[D]
    V = ef.EMBED_VOCAB
    x = ef.merge_x24_np(_bf16_bits(thi[:V]), tlo[:V].cpu().numpy())
    rng = np.random.default_rng(D)
    rs = (1.0 / np.sqrt((x ** 2).mean(1) + ef.EPS)).astype(np.float32)
    w = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    rs_d = torch.full((V + GUARD_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
    rs_d[:V] = _dev(rs)
    out = torch.full((V + GUARD_ROWS, D), -1, dtype=torch.int16, device=DEV)
    assert rows_call(2, a=thi, b=tlo, c=rs_d, d=_dev(w), rows=V, n=D, o0=out) == 0
    assert bool((out[V:] == -1).all())
    got = _f64(out[:V].contiguous().view(torch.bfloat16))
    ref, bar = ef.hidden_out_reference(x, rs, w)
    m = MARGINS.setdefault("hidden_out", {})
    found = ef.findings(f"D={D}", got, ref, bar, m)
    assert not found, found
    assert not got[5].any() and np.abs(x[6]).max() > 9e3


@pytest.mark.parametrize("rows", ef.ROWSCALE_ROWS)
@pytest.mark.parametrize("np_", ef.ROWSCALE_NPS)
def test_rowscale(rows, np_):
    ssp = _ssp_in(rows, np_, seed=3)
    ssp[:, 0] = 0.0  # a zero row: rs = eps^-1/2
    buf = torch.full((np_ + 1, rows), float("nan"), dtype=torch.float32, device=DEV)
    buf[:np_] = _dev(ssp)
    rs = torch.full((rows + 3,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().rp_dbg_rowscale(_lib.ptr(buf), _lib.ptr(rs), rows, np_, 1.0 / (64 * np_), ef.EPS, _lib.current_stream()),
               "rp_dbg_rowscale")
    torch.cuda.synchronize()
    ref = ef.rs_reference(ssp, 1.0 / (64 * np_))
    m = MARGINS.setdefault("rowscale", {})
    found = ef.findings(f"rows={rows} np={np_}", rs[:rows].cpu().numpy(), ref, ef.rs_rel_bar(np_) * ref, m)
    assert not found, found
    assert bool(torch.isnan(rs[rows:]).all())


def test_encoder_rows_checks_its_arguments():
    t = torch.zeros(8, 64, device=DEV)
    assert rows_call(3, a=t, rows=8, n=64) == RP_E_INVALID
    assert rows_call(0, a=t, rows=8, n=60, vocab=8, o0=t, o1=t, o2=t) == RP_E_INVALID
    assert rows_call(1, a=t, b=t, c=t, ia=t, T=8, rows=300, n=64, vocab=8, np_=1, o0=t, o1=t, o2=t) == RP_E_INVALID  # Tp % 256
    assert rows_call(1, a=t, b=t, c=t, ia=t, T=600, rows=512, n=64, vocab=8, np_=1, o0=t, o1=t, o2=t) == RP_E_INVALID
    assert rows_call(2, a=t, b=t, c=None, d=t, rows=8, n=64, o0=t) == RP_E_INVALID
