"""The encoder's training weight-gradient kernel (wgrad_kernel: both tile configurations, split-K, one- and two-product launches,
row pitches apart from the widths, the finishing epilogue) and four of the training step's GEMM epilogues (EpiRmsBwdResidT
with and without MASK, EpiGegluBwd with dropout, EpiGegluTrainT<false | true>, EpiResidT<true> with a dropout site) alone on the MI355X against the
float64 restatement of the same operation (tests/train_kernel_helpers.py: derivation of every bar there), through the test-only
entry points rp_dbg_wgrad_ex and rp_dbg_train_gemm, which run launch_wgrad / launch_wgrad_pair / launch_gemm as the trainer does.
The training attention (attention_kernel<true, *>, attn_bwd_kernel<0 | 1, *>, bias_grad_kernel) runs through
rp_dbg_attention_train (docs/HISTORY.md section 21).  tests/test_train_mfma_kernels_cpu.py shows on the same shapes that the bars hold for a float32 stand-in and separate planted bugs.

Every operand and output lives in a guarded arena (hip_helpers.Arena): operands hold NaN in the columns n .. ld the kernel must
not read, outputs the sentinel byte; after every call the guards are intact, the operands unchanged, every live output element
written.  Every case asserts the tile configuration and split count rp_dbg_wgrad_ex reports.

RP_TRAIN_MARGINS_OUT=<path>: every measured value and bar is written there as JSON (profiles/train_kernel_margins.json)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_forward_helpers as ef  # noqa: E402
import encoder_kernel_helpers as ek  # noqa: E402
import hip_helpers as hh  # noqa: E402
import train_kernel_helpers as tk  # noqa: E402
from reprover_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGINS = {}
RP_E_INVALID = -1
GUARD = hh.MIN_GUARD
SENTINEL32 = np.uint32(0x5A5A5A5A)
assert hh.OUTPUT_BYTE == 0x5A


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("RP_TRAIN_MARGINS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


def _operand(name, a64, ld):
    """bf16 [T, ld] in an arena: the values, NaN in the columns beyond them."""
    t = torch.from_numpy(tk.padded(a64, ld)).to(torch.bfloat16)
    return hh.Arena.of(name, t.to(DEV), GUARD)


def _f32_arena(name, *shape, init=None):
    if init is not None:
        return hh.Arena.of(name, torch.from_numpy(np.ascontiguousarray(init, np.float32)).to(DEV), GUARD)
    return hh.Arena(name, int(np.prod(shape)) * 4, GUARD, DEV, dtype=torch.float32)


def _read(arena, *shape):
    return arena.view(*shape).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _equals_float64(got, ref):
    """An fp32 result against a float64 one, as numbers (no NaN equals anything; the sign of a zero is not a number's bit: a
    float64 sum of +-0 products and the MFMA's may differ in it)."""
    return np.array_equal(np.asarray(got, np.float64), ref)


class Product:
    """One product's buffers: Y [T, ldy], X [T, ldx] (float64 arrays of bf16 values), out [splits, ny, nx]."""

    def __init__(self, tag, Y, X, S, py=0, px=0):
        self.T, self.ny, self.nx, self.S = Y.shape[0], Y.shape[1], X.shape[1], S
        self.ldy, self.ldx = self.ny + py, self.nx + px
        self.Y, self.X = _operand(f"Y{tag}", Y, self.ldy), _operand(f"X{tag}", X, self.ldx)
        self.out = _f32_arena(f"out{tag}", S, self.ny, self.nx)

    def args(self):
        return (self.Y.ptr, self.ldy, self.ny, self.X.ptr, self.ldx, self.nx, self.out.ptr)

    def arenas(self):
        return [self.Y, self.X, self.out]

    def result(self):
        return _read(self.out, self.S, self.ny, self.nx)


class Finish:
    """The finishing epilogue's buffers for a product of ny = 2 F rows: `out` holds d wi_0 [F, nx] in its first half."""

    def __init__(self, F, nx, w0, w1, ln):
        self.F, self.nx = F, nx
        self.w0, self.w1, self.ln = _f32_arena("w0", init=w0), _f32_arena("w1", init=w1), _f32_arena("ln", init=ln)
        self.g1, self.dln = _f32_arena("g1", F, nx), _f32_arena("dln_part", 2 * F // 32, nx)

    def args(self):
        return (self.g1.ptr, self.w0.ptr, self.w1.ptr, self.ln.ptr, self.dln.ptr)

    def arenas(self):
        return [self.w0, self.w1, self.ln, self.g1, self.dln]


def launch(p0, p1=None, cfg=0, fin=None, splits=None, expect=0, want_cfg=None):
    """rp_dbg_wgrad_ex; then: the guards intact and the operands unchanged; refused (expect != 0): every output at rest; else the
    reported plan is (want_cfg, splits) and every live output element is written.  -> the reported plan."""
    plan = (ctypes.c_int32 * 2)(-7, -7)
    a1 = p1.args() if p1 is not None else (None, 0, 0, None, 0, 0, None)
    fa = fin.args() if fin is not None else (None,) * 5
    S = p0.S if splits is None else splits
    st = _lib.load().rp_dbg_wgrad_ex(*p0.args(), *a1, p0.T, cfg, S, *fa, plan, _lib.current_stream())
    torch.cuda.synchronize()
    arenas = p0.arenas() + (p1.arenas() if p1 is not None else []) + (fin.arenas() if fin is not None else [])
    outputs = [p0.out] + ([p1.out] if p1 is not None else []) + ([fin.g1, fin.dln] if fin is not None else [])
    for a in arenas:
        assert a.broken_guards() == [], a.name
        if a not in outputs:
            assert a.at_rest(), f"{a.name} was written"
    if expect:
        assert st == expect, (st, hh.last_error())
        assert all(a.at_rest() for a in outputs)
        return None
    _lib.check(st, "rp_dbg_wgrad_ex")
    assert (plan[0], plan[1]) == ((cfg if want_cfg is None else want_cfg), S), tuple(plan)
    if fin is None:
        assert not (_bits(p0.result()) == SENTINEL32).any(), "out0: a live element was not written"
    else:  # the first F * nx floats are d wi_0; the rest of out0's arena keeps its byte
        flat = _read(p0.out)
        assert not (_bits(flat[: fin.F * fin.nx]) == SENTINEL32).any() and (_bits(flat[fin.F * fin.nx:]) == SENTINEL32).all()
        assert not (_bits(_read(fin.g1)) == SENTINEL32).any() and not (_bits(_read(fin.dln)) == SENTINEL32).any()
    if p1 is not None:
        assert not (_bits(p1.result()) == SENTINEL32).any(), "out1: a live element was not written"
    return tuple(plan)


def _splits(T):
    return [s for s in tk.WGRAD_SPLITS if s <= T // 64]


def _note(name, **kw):
    MARGINS.setdefault(name, {}).update(kw)


# ---------------------------------------------------------------------------------------------------------------------------
# one product
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("T", tk.WGRAD_TS)
def test_wgrad_against_float64(T, cfg):
    """Every split's partial matrix: integer operands to the bit, N(0, 1) operands within the accumulator bar."""
    found, worst = [], {}
    for ny, nx, py, px in tk.WGRAD_SHAPES[T]:
        for kind in ("integer", "normal"):
            Y, X = tk.wgrad_operands(T, ny, nx, kind)
            for S in _splits(T):
                p = Product("", Y, X, S, py, px)
                launch(p, cfg=cfg)
                got = p.result()
                ref, bar = tk.wgrad_reference(Y, X, S, exact=kind == "integer")
                tag = f"wgrad cfg={cfg} T={T} {ny}x{nx} ld+{py}/{px} S={S} {kind}"
                if kind == "integer":
                    if not _equals_float64(got, ref):
                        found.append(f"{tag}: {int((got != ref).sum())} elements differ from float64")
                else:
                    found += tk.findings(tag, got, ref, bar, worst)
    _note(f"wgrad_normal_cfg{cfg}_T{T}", worst_error_over_bar=max(worst.values()))
    assert not found, "\n".join(found)


@pytest.mark.parametrize("T", [128, 320])
@pytest.mark.parametrize("cfg", [0, 1])
def test_wgrad_one_hot_placement(cfg, T):
    """Y and X hold one non-zero each, at (token t, feature o / c): exactly one element of exactly one split's partial is
    non-zero, and it is the product.  t over 0, 7, 8, 63, 64, T - 1; o, c over 0, 31, 32, 127, 128, 255, 256, last."""
    n, S = 264, 2
    zero = np.zeros((T, n))
    p = Product("", zero, zero, S, 8, 24)
    yv, xv = p.Y.view(T, p.ldy, dtype=torch.bfloat16), p.X.view(T, p.ldx, dtype=torch.bfloat16)
    feats = [f % n for f in tk.PLACEMENT_FEATURES]
    tokens = [t % T for t in tk.PLACEMENT_TOKENS] + ([127, 128, 191, 192] if T == 320 else [])  # (320: either side of the uneven cut)
    owner = {t: next(i for i, (r0, r1) in enumerate(tk.split_ranges(T, S)) if r0 <= t < r1) for t in tokens}
    cases = [(tokens[(i + j) % len(tokens)], o, c) for i, o in enumerate(feats) for j, c in enumerate(feats)]
    cases += [(t, 255, 256) for t in tokens] + [(t, n - 1, 0) for t in tokens]
    for t, o, c in cases:
        yv[t, o], xv[t, c] = 3.0, -1.5
        p.Y._init, p.X._init = p.Y.payload().clone(), p.X.payload().clone()  # (what "unchanged" is compared with)
        p.out.reset()
        launch(p, cfg=cfg)
        got = p.result()
        want = np.zeros((S, n, n))
        want[owner[t], o, c] = -4.5
        assert _equals_float64(got, want), (cfg, t, o, c, np.argwhere(got != want)[:4])
        yv[t, o], xv[t, c] = 0.0, 0.0


def test_wgrad_planned_configuration():
    """cfg = -1: plan_wgrad picks the tile configuration; the report names it (rp_dbg_wgrad_plan's answer, the restated cost
    model's) and the partials have the bits of the forced launch of that configuration."""
    seen = set()
    # (2560 x 3328 over one token tile: the smallest multiple-of-256 shape at which the cost model prefers the 256 x 256 tile)
    for T, (ny, nx) in ((64, (384, 384)), (1024, (384, 384)), (256, (136, 128)), (1024, (8, 8)), (64, (2560, 3328))):
        out = (ctypes.c_int32 * 4)()
        _lib.check(_lib.load().rp_dbg_wgrad_plan(ny, nx, 0, 0, T // 64, out), "rp_dbg_wgrad_plan")
        assert (out[0], out[1]) == tk.plan_wgrad(ny, nx, T // 64)
        Y, X = tk.wgrad_operands(T, ny, nx, "normal")
        S = min(out[1], T // 64)
        planned, forced = Product("", Y, X, S), Product("", Y, X, S)
        launch(planned, cfg=-1, want_cfg=out[0])
        launch(forced, cfg=out[0])
        assert np.array_equal(_bits(planned.result()), _bits(forced.result()))
        seen.add(out[0])
    assert seen == {0, 1}, "both tile configurations are reached through the plan"
    _note("wgrad_planned", configurations_seen=sorted(seen))


# ---------------------------------------------------------------------------------------------------------------------------
# two products in one launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 320, 512])
def test_wgrad_pair(T):
    """Two products of different shapes over the same token rows (the second smaller than one tile in one case): the bits of
    the single launches, and each within the float64 bar."""
    found, worst = [], {}
    for (s0, s1) in tk.PAIR_SHAPES:
        for S in _splits(T):
            ops = [tk.wgrad_operands(T, ny, nx, "normal", seed=k + 1) for k, (ny, nx) in enumerate((s0, s1))]
            a, b = Product("0", *ops[0], S, 8, 0), Product("1", *ops[1], S, 0, 24)
            launch(a, b, cfg=0)
            for k, (p, (Y, X)) in enumerate(zip((a, b), ops)):
                alone = Product("", Y, X, S, p.ldy - p.ny, p.ldx - p.nx)
                launch(alone, cfg=0)
                assert np.array_equal(_bits(p.result()), _bits(alone.result())), (T, s0, s1, S, k)
                found += tk.findings(f"pair T={T} {s0}+{s1} S={S} product {k}", p.result(), *tk.wgrad_reference(Y, X, S), worst)
    _note(f"wgrad_pair_T{T}", worst_error_over_bar=max(worst.values()))
    assert not found, "\n".join(found)


# ---------------------------------------------------------------------------------------------------------------------------
# the finishing epilogue
# ---------------------------------------------------------------------------------------------------------------------------
def run_unfold_geglu(part, w0, w1, ln):
    """rp_dbg_unfold, GEGLU mode, on one partial [rows, C] (host fp32) -> g0, g1 [rows / 2, C]."""
    rows, C = part.shape
    pd, d0, d1, dl = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (part, w0, w1, ln))
    g = [_f32_arena(f"u{k}", rows // 2, C) for k in range(2)]
    dpart, dln = _f32_arena("udp", rows // 32, C), _f32_arena("udl", C)
    _lib.check(_lib.load().rp_dbg_unfold(_lib.ptr(pd), rows * C, 1, rows, C, ek.UNFOLD_GEGLU, 0, g[0].ptr, g[1].ptr, None, _lib.ptr(d0),
                                         _lib.ptr(d1), None, _lib.ptr(dl), dpart.ptr, dln.ptr, _lib.current_stream()), "rp_dbg_unfold")
    torch.cuda.synchronize()
    return [_read(x, rows // 2, C) for x in g]


@pytest.mark.parametrize("form", ["alone-cfg0", "alone-cfg1", "pair"])
@pytest.mark.parametrize("ny", tk.FINISH_NYS)
def test_wgrad_finish(ny, form):
    """g0 / g1: the bits of unfold_kernel's GEGLU mode on the plain launch's partial, within the float64 bar, and with integer
    operands fp32(acc ln) to the bit; dln_part within its chain bound, exact with integer masters."""
    found, worst = [], {}
    cfg = 1 if form == "alone-cfg1" else 0
    F = ny // 2
    for nx in tk.FINISH_NXS:
        for kind, T in (("integer", 192), ("normal", 64), ("normal", 320)):
            Y, X = tk.wgrad_operands(T, ny, nx, kind)
            w0, w1, ln = tk.finish_operands(F, nx, kind)
            p, fin = Product("", Y, X, 1, 24, 8), Finish(F, nx, w0, w1, ln)
            other = None
            if form == "pair":
                Y1, X1 = tk.wgrad_operands(T, 72, 264, kind, seed=3)
                other = Product("1", Y1, X1, 1)
            launch(p, other, cfg=cfg, fin=fin)
            got = dict(g0=_read(p.out)[: F * nx].reshape(F, nx), g1=_read(fin.g1, F, nx), dln_part=_read(fin.dln, ny // 32, nx))
            plain = Product("", Y, X, 1, 24, 8)
            launch(plain, cfg=cfg)
            acc = plain.result()[0]
            ref, bar = tk.wgrad_reference(Y, X, 1, exact=kind == "integer")
            want = tk.finish_reference(ref[0], bar[0], w0, w1, ln)
            tag = f"finish {form} ny={ny} nx={nx} T={T} {kind}"
            ug = run_unfold_geglu(acc, w0, w1, ln)
            for k in range(2):
                assert np.array_equal(_bits(got[f"g{k}"]), _bits(ug[k])), f"{tag}: g{k} differs from rp_dbg_unfold in bits"
            if kind == "integer":
                assert _equals_float64(acc, ref[0]), tag
                for k in range(2):
                    assert _equals_float64(got[f"g{k}"], want[f"g{k}"][0].astype(np.float32)), f"{tag}: g{k} is not fp32(acc ln)"
                assert _equals_float64(got["dln_part"], want["dln_part"][0]), f"{tag}: dln_part is not exact"
            else:
                for name, (r, b) in want.items():
                    found += tk.findings(f"{tag} {name}", got[name], r, b, worst)
            if other is not None:
                found += tk.findings(f"{tag} product 1", other.result(), *tk.wgrad_reference(Y1, X1, 1, exact=kind == "integer"))
    for name in ("g0", "g1", "dln_part"):
        _note(f"wgrad_finish_{form}_ny{ny}", **{name: max(v for k, v in worst.items() if k.endswith(name))})
    assert not found, "\n".join(found)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: bad VALUES only; every pointer is a valid buffer of the stated size
# ---------------------------------------------------------------------------------------------------------------------------
def test_wgrad_refusals():
    T, ny, nx = 128, 64, 72
    Y, X = tk.wgrad_operands(T, ny, nx, "integer")
    w0, w1, ln = tk.finish_operands(ny // 2, nx, "integer")
    lib = _lib.load()

    def refused(mut, fin_splits=None, **kw):
        p = Product("", Y, X, 2, 8, 8)
        fin = Finish(ny // 2, nx, w0, w1, ln) if fin_splits else None
        mut(p)
        launch(p, cfg=kw.get("cfg", 0), fin=fin, splits=fin_splits or kw.get("splits"), expect=RP_E_INVALID)

    refused(lambda p: None, fin_splits=2)                       # a finishing epilogue on a split launch
    refused(lambda p: setattr(p, "ny", 56), fin_splits=1)       # ... on ny % 64 != 0 (8-row pieces of the same matrix)
    refused(lambda p: setattr(p, "T", 96))
    refused(lambda p: setattr(p, "T", 0))
    refused(lambda p: None, splits=0)
    refused(lambda p: None, splits=3)                           # more splits than token tiles
    refused(lambda p: None, cfg=2)
    refused(lambda p: None, cfg=-2)
    refused(lambda p: setattr(p, "ny", 60))
    refused(lambda p: setattr(p, "nx", 0))
    refused(lambda p: setattr(p, "ldy", 60))                    # ld < n
    refused(lambda p: setattr(p, "ldx", 76))                    # ld % 8 != 0
    # a pair on the 128 x 128 tiles; a pair whose second product has a bad width; a finishing epilogue with a pointer missing
    a, b = Product("0", Y, X, 1), Product("1", Y, X, 1)
    launch(a, b, cfg=1, expect=RP_E_INVALID)
    b.nx = 12
    launch(a, b, cfg=0, expect=RP_E_INVALID)
    p, fin = Product("", Y, X, 1), Finish(ny // 2, nx, w0, w1, ln)
    plan = (ctypes.c_int32 * 2)()
    st = lib.rp_dbg_wgrad_ex(*p.args(), None, 0, 0, None, 0, 0, None, T, 0, 1, fin.g1.ptr, fin.w0.ptr, None, fin.ln.ptr, fin.dln.ptr, plan,
                             _lib.current_stream())
    torch.cuda.synchronize()
    assert st == RP_E_INVALID and p.out.at_rest() and fin.g1.at_rest() and fin.dln.at_rest()
    # and the same buffers are accepted with the values put right
    launch(p, cfg=0, fin=fin)


# ---------------------------------------------------------------------------------------------------------------------------
# the training step's GEMM epilogues (rp_dbg_train_gemm)
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 0x5EED1234
VARIANT_TILE = {v: (t[0], t[1]) for v, t in ef.VARIANTS.items()}  # tile configuration -> (feature tile, token tile)


def _bf16_arena(name, a64=None, rows=0, ld=0):
    """bf16 [rows, ld]: the values of a64 with NaN in the columns beyond them, or (a64 None) an output full of the sentinel."""
    if a64 is None:
        return hh.Arena(name, rows * ld * 2, GUARD, DEV, dtype=torch.bfloat16)
    return _operand(name, a64, ld)


def _bf16_bits(arena, rows, ld):
    return arena.view(rows, ld, dtype=torch.int16).cpu().numpy().view(np.uint16)


def _bf16_values(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _to_bf16_bits(a64):
    return torch.from_numpy(np.ascontiguousarray(a64)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def mask_of(p, site, rows, cols, seed=SEED):
    """The multipliers the launch used at (site, rows 0 .., columns 0 ..): 0 or fp32 1 / (1 - p), as float64."""
    out = torch.zeros(rows, cols, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().rp_dbg_dropout_mask(p, seed, site, 0, 0, rows, cols, _lib.ptr(out), _lib.current_stream()), "rp_dbg_dropout_mask")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64) * tk.drop_scale(p)


class TrainGemm:
    """One rp_dbg_train_gemm call: arenas, the call, the checks every call gets (guards, inputs unchanged, the columns beyond the
    live ones unchanged, the reported tile configuration)."""

    def __init__(self, mode, A, W, ld, p=0.0, site=tk.SITE, variant=0, x0=None, xs=None, rc=None, rs=None, want_ssp=False):
        self.mode, self.M, self.K, self.N, self.ld, self.p, self.site, self.variant = mode, A.shape[0], A.shape[1], W.shape[0], ld, p, site, variant
        M, N = self.M, self.N
        self.A, self.W = _operand("A", A, self.K), _operand("W", W, self.K)
        self.inputs, self.outputs, self.inout = [self.A, self.W], [], []
        self.aux0 = self.aux1 = self.out2 = None
        if mode == tk.TG_GEGLU_BWD:  # N = d_ff; xs = the packed gu [M, 2 N]
            self.aux0, self.aux1 = _bf16_arena("gu_saved", xs, ld=ld), _f32_arena("rs", init=rs)
            self.inputs += [self.aux0, self.aux1]
            self.out0 = _bf16_arena("dzs", rows=M, ld=ld)
            self.out1, self.out2 = _f32_arena("rdp", (N + 63) // 64, M), _f32_arena("rcoef", M)
            self.outputs += [self.out0, self.out1, self.out2]
            self.n = 2 * N
        elif mode == tk.TG_RMS_BWD:
            hi, lo = ef.split_planes_np(x0)
            self.hi, self.lo, self.aux0 = _bf16_arena("dxhi", hi, ld=ld), _bf16_arena("dxlo", lo, ld=ld), _bf16_arena("x", xs, ld=ld)
            self.aux1 = _f32_arena("rcoef", init=rc)
            self.inputs += [self.aux0, self.aux1]
            self.inout += [self.hi, self.lo]
            if p > 0:
                self.out2 = _bf16_arena("dxm", rows=M, ld=ld)
                self.outputs.append(self.out2)
            self.out0, self.out1, self.n = self.hi, self.lo, N
        elif mode == tk.TG_GEGLU_TRAIN:
            if rs is not None:
                self.aux1 = _f32_arena("rs", init=rs)
                self.inputs.append(self.aux1)
            self.out0, self.out1 = _bf16_arena("gu", rows=M, ld=N), _bf16_arena("ff", rows=M, ld=ld)
            self.outputs += [self.out0, self.out1]
            self.n = N // 2
        else:
            hi, lo = ef.split_planes_np(x0)
            self.aux0, self.lo = _bf16_arena("xhi_in", hi, ld=ld), _bf16_arena("xlo", lo, ld=ld)
            self.out0, self.out1 = _bf16_arena("xhi", rows=M, ld=ld), self.lo
            self.inputs.append(self.aux0)
            self.outputs.append(self.out0)
            self.inout.append(self.lo)
            if want_ssp:
                self.out2 = _f32_arena("ssp", (N + 63) // 64, M)
                self.outputs.append(self.out2)
            self.n = N
        self.before = {a.name: a.payload().clone() for a in self.inout}

    def call(self, expect=0, **override):
        kw = dict(mode=self.mode, M=self.M, N=self.N, K=self.K, ld=self.ld, p=self.p, site=self.site, variant=self.variant)
        kw.update(override)
        plan = (ctypes.c_int32 * 6)(*([-7] * 6))
        ptr = lambda a: None if a is None else a.ptr  # noqa: E731
        st = _lib.load().rp_dbg_train_gemm(kw["mode"], self.A.ptr, self.W.ptr, kw["M"], kw["N"], kw["K"], ptr(self.aux0), ptr(self.aux1),
                                           self.out0.ptr, self.out1.ptr, ptr(self.out2), kw["ld"], kw["p"], SEED, kw["site"], kw["variant"],
                                           plan, _lib.current_stream())
        torch.cuda.synchronize()
        for a in self.inputs + self.outputs + self.inout:
            assert a.broken_guards() == [], a.name
        for a in self.inputs:
            assert a.at_rest(), f"{a.name} was written"
        if expect:
            assert st == expect, (st, hh.last_error())
            assert all(a.at_rest() for a in self.outputs + self.inout)
            return self
        _lib.check(st, "rp_dbg_train_gemm")
        # (variant -1: the forward's own choice - any tile configuration of the table; the tile counts below follow from it)
        assert (plan[0] == self.variant if self.variant >= 0 else plan[0] in VARIANT_TILE) and plan[1] == 0, tuple(plan)
        assert (plan[2], plan[3]) == (-(-self.N // VARIANT_TILE[plan[0]][0]), self.M // VARIANT_TILE[plan[0]][1]), tuple(plan)
        M, ld = self.M, self.ld
        for a in self.inout:  # the columns beyond the live ones keep their (NaN) bits
            now, was = _bf16_bits(a, M, ld), self.before[a.name].view(torch.int16).view(M, ld).cpu().numpy().view(np.uint16)
            assert np.array_equal(now[:, self.n:], was[:, self.n:]), f"{a.name}: a column beyond n changed"
        for a in self.outputs:
            if a.dtype == torch.float32:
                assert not (_bits(_read(a)) == SENTINEL32).any(), f"{a.name}: a live element was not written"
                continue
            lda = self.N if a.name == "gu" else ld
            live = self.N if a.name == "gu" else self.n
            b = _bf16_bits(a, M, lda)
            assert not (b[:, :live] == 0x5A5A).any(), f"{a.name}: a live element was not written"
            assert (b[:, live:] == 0x5A5A).all(), f"{a.name}: a column beyond n was written"
        return self

    def bits(self, arena, cols=None):
        lda = self.N if arena.name == "gu" else self.ld
        return _bf16_bits(arena, self.M, lda)[:, : (self.n if cols is None else cols)]


def mask_dx_launch(hi_bits, lo_bits, p, site):
    """mask_dx_kernel (rp_dbg_train_rows mode 2) on contiguous copies of the planes -> dxm bits."""
    rows, n = hi_bits.shape
    h, l = (torch.from_numpy(b.view(np.int16).copy()).to(DEV) for b in (hi_bits, lo_bits))
    out = hh.Arena("dxm_rows", rows * n * 2, GUARD, DEV, dtype=torch.bfloat16)
    st = _lib.load().rp_dbg_train_rows(2, _lib.ptr(h), _lib.ptr(l), None, 0, rows, n, 0, 0, 0, 0.0, p, SEED, site, out.ptr, None, None,
                                       _lib.current_stream())
    _lib.check(st, "rp_dbg_train_rows(2)")
    torch.cuda.synchronize()
    assert out.broken_guards() == []
    return _bf16_bits(out, rows, n)


@pytest.mark.parametrize("variant", [0, 26])
@pytest.mark.parametrize("N", tk.RMS_NS)
def test_rms_bwd_residual(N, variant):
    """dx += A W^T - rc x on the two planes, with and without the next branch's mask: integer operands the host's split of
    float64 bit for bit, N(0, 1) operands within the bar; dxm = bf16((hi + lo) m) of the planes just stored, bit for bit against
    the host and against mask_dx_kernel; the planes do not depend on the mask."""
    found, worst = [], {}
    for i, K in enumerate(tk.RMS_KS):
        M = tk.TG_MS[(i + N // 8) % 2]
        ld = N + (0, 8, 24)[(i + N // 8) % 3]
        for kind in ("integer", "normal"):
            A, W, x0, xs, rc = tk.rms_operands(M, N, K, kind)
            P, S = ef.gemm_products(M, N, K, kind)
            ref, bar, bar_hi = tk.rms_bwd_expected(P, S, K, x0, xs, rc, exact_acc=kind == "integer")
            tag = f"rms_bwd v{variant} M={M} N={N} K={K} ld={ld} {kind}"
            planes = {}
            for p in (0.0, 0.1):
                g = TrainGemm(tk.TG_RMS_BWD, A, W, ld, p=p, site=tk.OTHER_SITE, variant=variant, x0=x0, xs=xs, rc=rc).call()
                hb, lb = g.bits(g.hi), g.bits(g.lo)
                planes[p] = (hb, lb)
                hi, lo = _bf16_values(hb), _bf16_values(lb)
                if kind == "integer":
                    wh, wl = ef.split_planes_np(ref)
                    assert np.array_equal(hi, wh) and np.array_equal(lo, wl), f"{tag} p={p}: the planes are not the split of float64"
                else:
                    found += tk.findings(f"{tag} p={p} hi+lo", hi + lo, ref, bar, worst)
                    found += tk.findings(f"{tag} p={p} hi", hi, ref, bar_hi, worst)
                if p:
                    m = mask_of(p, tk.OTHER_SITE, M, N)
                    assert 0.05 < (m == 0).mean() < 0.15 or N == 8
                    assert (m != mask_of(p, tk.SITE, M, N)).any()
                    dxm = g.bits(g.out2)
                    assert np.array_equal(dxm, _to_bf16_bits(tk.dxm_expected(hi, lo, m))), f"{tag}: dxm is not bf16((hi + lo) m)"
                    assert np.array_equal(dxm, mask_dx_launch(hb, lb, p, tk.OTHER_SITE)), f"{tag}: dxm differs from mask_dx_kernel"
            assert all(np.array_equal(a, b) for a, b in zip(planes[0.0], planes[0.1])), f"{tag}: the planes depend on the mask"
    _note(f"rms_bwd_v{variant}_N{N}", **{k.strip(): max(v for t, v in worst.items() if t.endswith(k)) for k in ("hi+lo", " hi")})
    assert not found, "\n".join(found)


def _unpack(packed):
    """[M, 2 F] packed columns -> (gate, up) [M, F]."""
    M, n2 = packed.shape
    v = packed.reshape(M, n2 // 64, 2, 32)
    return v[:, :, 0].reshape(M, n2 // 2), v[:, :, 1].reshape(M, n2 // 2)


@pytest.mark.parametrize("variant", [0, 26])
@pytest.mark.parametrize("F", tk.GB_FS)
def test_geglu_backward(F, variant):
    """dzs = rs [dy_g | dy_u] (packed) and rcoef = rs^2 (row dot) / K against float64 on the saved bf16 g, u (gate std 1, 3, 10, 30
    by feature), p = 0, 0.1, 0.5; under dropout the reference with dff m, and +-0 where m = 0.  The excess over the derived bars
    (what the fast-math constants stand for) is measured with the constants at 0 and recorded before the assertion."""
    found, worst, excess = [], {}, MARGINS.setdefault("geglu_bwd_fastmath_excess", dict(dzs=-1e30, rcoef=-1e30))  # (rcoef: it and the slots)
    for i, K in enumerate(tk.GB_KS):
        M = tk.TG_MS[(i + F // 64) % 2]
        ld = 2 * F + (0, 8, 24)[(i + F // 64) % 3]
        A, W, g, u, rs = tk.geglu_bwd_operands(M, F, K)
        P, S = A @ W.T, np.abs(A) @ np.abs(W).T
        for p in tk.DROP_PS:
            tag = f"geglu_bwd v{variant} M={M} F={F} K={K} ld={ld} p={p}"
            t = TrainGemm(tk.TG_GEGLU_BWD, A, W, ld, p=p, site=tk.SITE + 1, variant=variant, xs=tk.pack_gu(g, u), rs=rs).call()
            bits = t.bits(t.out0)
            dg, du = _unpack(_bf16_values(bits))
            m = mask_of(p, tk.SITE + 1, M, F) if p else None
            if p:
                zg, zu = _unpack(bits)
                assert ((zg[m == 0] & 0x7FFF) == 0).all() and ((zu[m == 0] & 0x7FFF) == 0).all(), f"{tag}: a dropped element is not +-0"
            got = dict(dzs_g=dg, dzs_u=du, rcoef=_read(t.out2, M).astype(np.float64), slots=_read(t.out1, (F + 63) // 64, M).astype(np.float64))
            bare = tk.geglu_bwd_expected(P, S, K, g, u, rs, m, extra_dzs=0.0, extra_rcoef=0.0)
            for name, key in (("dzs_g", "dzs"), ("dzs_u", "dzs"), ("rcoef", "rcoef"), ("slots", "rcoef")):
                live = bare[name][1] > 0
                excess[key] = max(excess[key], float((np.abs(got[name] - bare[name][0]) - bare[name][1])[live].max()))
            for name, (ref, bar) in tk.geglu_bwd_expected(P, S, K, g, u, rs, m).items():
                found += tk.findings(f"{tag} {name}", got[name], ref, bar, worst)
    print(f"  geglu backward F={F} v{variant}: excess over the derived bars so far {excess}")
    _note(f"geglu_bwd_v{variant}_F{F}", **{k: max(v for t, v in worst.items() if t.endswith(k)) for k in ("dzs_g", "dzs_u", "rcoef", "slots")})
    assert not found, "\n".join(found)


def gemm_ex(A, W, epi, prof_class, ssp=None, inv_d=0.0):
    """rp_dbg_gemm_ex on the same operands (default options) -> (bits [M, cols], rs bits or None)."""
    M, K, N = A.shape[0], A.shape[1], W.shape[0]
    cols = N // 2 if epi == ef.EPI_GEGLU else N
    a, w = _operand("A", A, K), _operand("W", W, K)
    out = _bf16_arena("out", rows=M, ld=cols)
    sspd = None if ssp is None else torch.from_numpy(np.ascontiguousarray(ssp, np.float32)).to(DEV)
    rs = None if ssp is None else _f32_arena("rs", M)
    plan = (ctypes.c_int32 * 6)()
    st = _lib.load().rp_dbg_gemm_ex(a.ptr, K, w.ptr, N, out.ptr, cols, M, K, N, epi, prof_class, 0, None, 0 if ssp is None else 1,
                                    _lib.ptr(sspd), 0 if ssp is None else ssp.shape[0], inv_d, ef.EPS, None if rs is None else rs.ptr, None, 0,
                                    plan, _lib.current_stream())
    _lib.check(st, "rp_dbg_gemm_ex")
    torch.cuda.synchronize()
    return _bf16_bits(out, M, cols), (None if rs is None else _read(rs, M))


@pytest.mark.parametrize("variant", [-1, 0, 26])
@pytest.mark.parametrize("F", tk.FWD_FS)
def test_geglu_train(F, variant):
    """gu: rp_dbg_gemm_ex STORE's bits with the same row factor; ff without dropout: rp_dbg_gemm_ex GEGLU's bits ("the same bits
    as it"); with dropout: float64 gelu_new(rs g)(rs u) m within the forward bar scaled by m + one product + half a bf16 ulp,
    and +-0 where m = 0."""
    found, worst = [], {}
    for i, K in enumerate(tk.FWD_KS):
        M = tk.TG_MS[(i + F // 64) % 2]
        ld = F + (0, 8, 24)[(i + F // 64) % 3]
        A, W, _ = ef.gemm_operands(M, 2 * F, K, "normal", True)
        P, S = ef.gemm_products(M, 2 * F, K, "normal", True)
        ssp = rs32 = rs64 = None
        if (i + F // 64) % 3 != 2:  # two cases of three run with a row factor in [0.5, 1.5]: rowscale_kernel's, as the trainer's
            want = np.random.default_rng([F, K]).uniform(0.5, 1.5, M)
            ssp = np.zeros((2, M), np.float32)
            ssp[0] = ssp[1] = (0.5 * (1.0 / want ** 2 - ef.EPS) * 64).astype(np.float32)
            rs32 = hh.rowscale(torch.from_numpy(ssp).to(DEV), 1.0 / 64).cpu().numpy()
            rs64 = rs32.astype(np.float64)
            assert 0.49 < rs64.min() and rs64.max() < 1.51
        tag = f"geglu_train v{variant} M={M} F={F} K={K} ld={ld} rs={'yes' if ssp is not None else 'no'}"
        gu_ref, rs_ref = gemm_ex(A, W, ef.EPI_STORE, ef.K_WI, ssp, 1.0 / 64)
        ff_ref, _ = gemm_ex(A, W, ef.EPI_GEGLU, ef.K_WI, ssp, 1.0 / 64)
        if ssp is not None:
            assert np.array_equal(_bits(rs_ref), _bits(rs32))
        for p in tk.DROP_PS:
            g = TrainGemm(tk.TG_GEGLU_TRAIN, A, W, ld, p=p, site=tk.SITE + 1, variant=variant, rs=rs32).call()
            assert np.array_equal(g.bits(g.out0, 2 * F), gu_ref), f"{tag} p={p}: gu differs from rp_dbg_gemm_ex STORE in bits"
            ffb = g.bits(g.out1)
            m = mask_of(p, tk.SITE + 1, M, F) if p else None
            if not p:
                assert np.array_equal(ffb, ff_ref), f"{tag}: ff differs from rp_dbg_gemm_ex GEGLU in bits"
            else:
                assert ((ffb[m == 0] & 0x7FFF) == 0).all(), f"{tag} p={p}: a dropped element is not +-0"
            ref, bar = tk.geglu_train_expected(P, S, K, rs64, m=m)
            found += tk.findings(f"{tag} p={p} ff", _bf16_values(ffb), ref, bar, worst)
    _note(f"geglu_train_v{variant}_F{F}", worst_error_over_bar=max(worst.values()))
    assert not found, "\n".join(found)


@pytest.mark.parametrize("variant", [-1, 0, 26])
@pytest.mark.parametrize("N", tk.RMS_NS)
def test_resid_train(N, variant):
    """x += m (A W^T) with the old hi plane read from its own buffer: integer operands without dropout the host's split of
    float64 bit for bit; else within the forward RESID bar with the masked product; ssp = the sums of squares of x as stored."""
    found, worst = [], {}
    for i, K in enumerate(tk.FWD_KS):
        M = tk.TG_MS[(i + N // 8) % 2]
        ld = N + (0, 8, 24)[(i + N // 8) % 3]
        for kind in ("integer", "normal"):
            A, W, x0, _, _ = tk.rms_operands(M, N, K, kind)
            P, S = ef.gemm_products(M, N, K, kind)
            for p in tk.DROP_PS:
                if kind == "integer" and p:
                    continue
                tag = f"resid_train v{variant} M={M} N={N} K={K} ld={ld} {kind} p={p}"
                want_ssp = (i + int(p * 10)) % 2 == 0
                g = TrainGemm(tk.TG_RESID_TRAIN, A, W, ld, p=p, site=tk.SITE, variant=variant, x0=x0, want_ssp=want_ssp).call()
                hi, lo = _bf16_values(g.bits(g.out0)), _bf16_values(g.bits(g.lo))
                m = mask_of(p, tk.SITE, M, N) if p else None
                ref, bar, bar_hi = tk.resid_train_expected(P, S, K, x0, m, exact_acc=kind == "integer")
                if kind == "integer":
                    wh, wl = ef.split_planes_np(ref)
                    assert np.array_equal(hi, wh) and np.array_equal(lo, wl), f"{tag}: the planes are not the split of float64"
                else:
                    found += tk.findings(f"{tag} hi+lo", hi + lo, ref, bar, worst)
                    found += tk.findings(f"{tag} hi", hi, ref, bar_hi, worst)
                if want_ssp:
                    np_ = (N + 63) // 64
                    sref, sbar = ef.ssp_reference(hi + lo, np_)
                    found += tk.findings(f"{tag} ssp", _read(g.out2, np_, M), sref, sbar, worst)
    _note(f"resid_train_v{variant}_N{N}", **{k.strip(): max(v for t, v in worst.items() if t.endswith(k)) for k in ("hi+lo", " hi", " ssp")})
    assert not found, "\n".join(found)


def test_train_gemm_refusals():
    M, N, K = 256, 64, 128
    A, W, x0, xs, rc = tk.rms_operands(M, N, K, "integer")
    g = TrainGemm(tk.TG_RMS_BWD, A, W, N, p=0.1, variant=0, x0=x0, xs=xs, rc=rc)
    for bad in (dict(mode=-1), dict(mode=4), dict(M=128), dict(M=0), dict(K=16), dict(K=144), dict(N=60), dict(N=0), dict(ld=56), dict(ld=68),
                dict(p=1.0), dict(p=-0.1), dict(variant=9), dict(variant=-1), dict(site=0)):
        g.call(expect=RP_E_INVALID, **bad)
    g.call(expect=RP_E_INVALID, variant=26, K=96)  # launch_gemm_cfg's own requirement (K % 64), before anything is launched
    g.call()
    A2, W2, _ = ef.gemm_operands(M, 128, K, "integer", True)
    f = TrainGemm(tk.TG_GEGLU_TRAIN, A2, W2, 64, variant=0)
    for bad in (dict(N=96), dict(ld=56), dict(variant=-2), dict(variant=5)):
        f.call(expect=RP_E_INVALID, **bad)
    f.call()
    A3, W3, gg, uu, rs3 = tk.geglu_bwd_operands(M, 64, K)
    b = TrainGemm(tk.TG_GEGLU_BWD, A3, W3, 128, variant=0, xs=tk.pack_gu(gg, uu), rs=rs3)
    for bad in (dict(N=96), dict(ld=120), dict(ld=132), dict(variant=-1), dict(variant=17)):
        b.call(expect=RP_E_INVALID, **bad)
    b.call()
    r = TrainGemm(tk.TG_RESID_TRAIN, A, W, N, variant=0, x0=x0)
    for bad in (dict(ld=56), dict(variant=-2), dict(M=384)):
        r.call(expect=RP_E_INVALID, **bad)
    r.call()


# ---------------------------------------------------------------------------------------------------------------------------
# training attention (rp_dbg_attention_train)
# ---------------------------------------------------------------------------------------------------------------------------
ATT_SITE = 16 + 8 * 2  # the probabilities' site of layer 2


def _rows_arena(name, a64, rows_total, dtype=torch.bfloat16):
    """[rows_total, cols]: the values in rows 0 .. T, NaN behind them (rows the kernels must not read)."""
    t = torch.full((rows_total, a64.shape[1]), float("nan"), dtype=dtype)
    t[: a64.shape[0]] = torch.from_numpy(np.ascontiguousarray(a64)).to(dtype)
    return hh.Arena.of(name, t.to(DEV), GUARD)


class AttnTrain:
    """One rp_dbg_attention_train call on a case: arenas, the call, guards, inputs unchanged, rows T .. rows_total untouched."""

    def __init__(self, c, p=0.0, att_in=None, rows_total=None):
        self.c, self.p, self.H, self.T = c, p, c["H"], c["T"]
        H, T = self.H, self.T
        self.rows = rows_total or (T + 256) // 256 * 256  # (at least one NaN row behind the last token)
        inner, ntab = H * 64, 2 * c["maxd"] + 1
        self.qkv, self.datt = _rows_arena("qkv", c["qkv"], self.rows), _rows_arena("datt", c["datt"], self.rows)
        self.att_in = None if att_in is None else _rows_arena("att", att_in, self.rows)
        self.cu = hh.Arena.of("cu", torch.from_numpy(np.asarray(c["cu"], np.int32)).to(DEV), GUARD)
        self.tab = _f32_arena("tab", init=c["tab"])
        self.lse, self.delta = _f32_arena("lse", H, self.rows), _f32_arena("delta", H, self.rows)
        self.att, self.dqkv = _bf16_arena("att_out", rows=self.rows, ld=inner), _bf16_arena("dqkv", rows=self.rows, ld=3 * inner)
        self.dtab = _f32_arena("dtab", ntab, H)
        self.inputs = [a for a in (self.qkv, self.datt, self.att_in, self.cu, self.tab) if a is not None]
        self.outputs = [self.lse, self.delta, self.att, self.dqkv, self.dtab]

    def call(self, expect=0, **override):
        c = self.c
        kw = dict(batch=len(c["cu"]) - 1, H=self.H, rows_total=self.rows, maxd=c["maxd"], p=self.p, site=ATT_SITE)
        kw.update(override)
        st = _lib.load().rp_dbg_attention_train(self.qkv.ptr, None if self.att_in is None else self.att_in.ptr, self.datt.ptr, self.cu.ptr,
                                                self.tab.ptr, kw["batch"], kw["H"], kw["rows_total"], kw["maxd"], kw["p"], SEED, kw["site"],
                                                self.lse.ptr, self.att.ptr, self.delta.ptr, self.dqkv.ptr, self.dtab.ptr, _lib.current_stream())
        torch.cuda.synchronize()
        for a in self.inputs + self.outputs:
            assert a.broken_guards() == [], a.name
        for a in self.inputs:
            assert a.at_rest(), f"{a.name} was written"
        if expect:
            assert st == expect, (st, hh.last_error())
            assert all(a.at_rest() for a in self.outputs)
            return self
        _lib.check(st, "rp_dbg_attention_train")
        H, T, inner = self.H, self.T, self.H * 64
        self.att_bits, self.dqkv_bits = _bf16_bits(self.att, self.rows, inner), _bf16_bits(self.dqkv, self.rows, 3 * inner)
        self.lse_v, self.delta_v = _read(self.lse, H, self.rows), _read(self.delta, H, self.rows)
        for name, b in (("att_out", self.att_bits), ("dqkv", self.dqkv_bits)):
            assert not (b[:T] == 0x5A5A).any(), f"{name}: a live element was not written"
            assert (b[T:] == 0x5A5A).all(), f"{name}: a row beyond the last token was written"
        for name, v in (("lse", self.lse_v), ("delta", self.delta_v)):
            assert not (_bits(v[:, :T]) == SENTINEL32).any() and (_bits(v[:, T:]) == SENTINEL32).all(), name
        assert not (_bits(_read(self.dtab)) == SENTINEL32).any()
        return self

    def results(self):
        inner, T = self.H * 64, self.T
        d = _bf16_values(self.dqkv_bits[:T])
        return dict(att=_bf16_values(self.att_bits[:T]), dq=d[:, :inner], dk=d[:, inner:2 * inner], dv=d[:, 2 * inner:],
                    lse2=self.lse_v[:, :T].astype(np.float64), delta=self.delta_v[:, :T].astype(np.float64),
                    dtab=_read(self.dtab, 2 * self.c["maxd"] + 1, self.H).T.astype(np.float64))


def engine_attention_mask(c, p):
    """mask(b, s0, L) -> [H, L, L]: the multipliers the kernels used, row = s0 + i, column = (h << 20) | j."""
    def mask(b, s0, L):
        out = torch.zeros(c["H"], L, L, dtype=torch.uint8, device=DEV)
        for h in range(c["H"]):
            _lib.check(_lib.load().rp_dbg_dropout_mask(p, SEED, ATT_SITE, s0, h << 20, L, L, _lib.ptr(out[h]), _lib.current_stream()),
                       "rp_dbg_dropout_mask")
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.float64) * tk.drop_scale(p)
    return mask


ATT_OUTPUTS = ("att", "dq", "dk", "dv", "lse2", "delta", "dtab")


@pytest.mark.parametrize("p", tk.DROP_PS)
@pytest.mark.parametrize("name", sorted(tk.ATT_TRAIN_CASES))
def test_attention_train_against_float64(name, p):
    """Forward (att, lse) and backward (delta, dq, dk, dv, the table gradient) against float64 with per-element bars; delta is
    formed from the bf16 att the kernel reads, so the reference reads the same one."""
    c = tk.attention_train_case(name)
    got = AttnTrain(c, p).call().results()
    ref = tk.attention_train_compute(c, engine_attention_mask(c, p) if p else None, att_used=got["att"], bars=True)
    found, worst = [], {}
    for k in ATT_OUTPUTS:
        found += tk.findings(f"attention_train {name} p={p} {k}", got[k], ref[k], ref["bar_" + k], worst)
    _note(f"attention_train_{name}_p{p}", **{k: max(v for t, v in worst.items() if t.endswith(" " + k)) for k in ATT_OUTPUTS})
    assert not found, "\n".join(found)


@pytest.mark.parametrize("name", ["h2-d32-std12-mixed", "h6-d128-std4-mixed"])
def test_attention_train_sequence_alone_has_its_bits(name):
    """Without dropout every sequence alone has the bits of its rows in the packed call for att / lse / delta / dq / dk / dv; its
    table gradient (LDS float adds in an order the hardware chooses: not bit-stable) is within the float64 bound of its share."""
    c = tk.attention_train_case(name)
    packed = AttnTrain(c).call()
    inner = c["H"] * 64
    for b in range(len(c["lens"])):
        s0, s1 = int(c["cu"][b]), int(c["cu"][b + 1])
        sub = tk.sub_attention_train_case(c, b)
        alone = AttnTrain(sub).call()
        assert np.array_equal(alone.att_bits[: s1 - s0], packed.att_bits[s0:s1]), (name, b, "att")
        assert np.array_equal(alone.dqkv_bits[: s1 - s0], packed.dqkv_bits[s0:s1]), (name, b, "dqkv")
        assert np.array_equal(_bits(alone.lse_v[:, : s1 - s0]), _bits(packed.lse_v[:, s0:s1])), (name, b, "lse")
        assert np.array_equal(_bits(alone.delta_v[:, : s1 - s0]), _bits(packed.delta_v[:, s0:s1])), (name, b, "delta")
        got = alone.results()
        ref = tk.attention_train_compute(sub, att_used=got["att"], bars=True)
        assert not tk.findings(f"{name} sequence {b} alone dtab", got["dtab"], ref["dtab"], ref["bar_dtab"])


def test_attention_train_supplied_att_and_padding():
    """att supplied by the caller is the O delta is formed from (and only that: dq / dk follow delta, dv does not change); a
    larger rows_total changes nothing in the live rows."""
    c = tk.attention_train_case("h2-d32-std12-mixed")
    base = AttnTrain(c).call()
    other = tk.bf16_round(np.random.default_rng(5).standard_normal((c["T"], c["H"] * 64)))
    sup = AttnTrain(c, att_in=other, rows_total=base.rows + 512).call()
    got = sup.results()
    ref = tk.attention_train_compute(c, att_used=other, bars=True)
    found = []
    for k in ("dq", "dk", "dv", "delta", "dtab"):
        found += tk.findings(f"supplied att {k}", got[k], ref[k], ref["bar_" + k])
    assert not found, "\n".join(found)
    inner = c["H"] * 64
    assert np.array_equal(sup.att_bits[: c["T"]], base.att_bits[: c["T"]])
    assert np.array_equal(sup.dqkv_bits[: c["T"], 2 * inner:], base.dqkv_bits[: c["T"], 2 * inner:]), "dv does not depend on att"
    assert not np.array_equal(sup.dqkv_bits[: c["T"], :inner], base.dqkv_bits[: c["T"], :inner])


def test_attention_train_refusals():
    c = tk.attention_train_case("h1-d8-std4-mixed")
    a = AttnTrain(c)
    for bad in (dict(rows_total=a.rows - 128), dict(rows_total=0), dict(rows_total=a.rows - 256 * 3), dict(H=0), dict(batch=0), dict(maxd=0),
                dict(maxd=448), dict(p=1.0), dict(p=-0.5)):
        a.call(expect=RP_E_INVALID, **bad)
    for cu in ([0, 5, 5, 9], [1, 5, 9], [0, 5, 3]):  # an empty sequence; not starting at 0; descending
        e = AttnTrain(dict(c, cu=np.asarray(cu, np.int32)))
        e.call(expect=RP_E_INVALID, batch=len(cu) - 1)
    a.call()
