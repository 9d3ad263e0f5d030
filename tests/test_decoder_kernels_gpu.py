"""The seq2seq training path's kernels alone on the MI355X, each against the float64 restatement of the same operation
(tests/decoder_kernel_helpers.py), through the test-only entry points rp_dbg_decoder_attention, rp_dbg_decoder_rows and
rp_dbg_hidden_head, which run the launch functions rp_decoder_loss_grad and rp_train_*_hidden run.

Shapes: lengths on, one below and one above 32 / 64 / 128 / 256, a long target over a one-token source and the reverse, an
empty target between two others, H = 6 (no power of two), tables of 257 and 33 entries, scores of magnitude 30.  Bars
(tests/test_decoder_kernels_cpu.py shows that each separates planted bugs on these shapes):
  * out, dq, dk, dv, dtab: relative L2 and worst row (max |error| / max |reference|) against exact float64, at most
    GRAD_TOL_FACTOR x the same figure of the float64 reference that rounds to bf16 where the kernels do; computed here from
    the two references, named exceptions in DEC_KERNEL_TOL;
  * lse2: 1e-3; delta: 33 x 2^-24 x sum |dO O| per row against the float64 sum over the kernel's own bf16 out;
  * fp32 row-kernel outputs: tests/test_step_ends_gpu.py's bar (2 x a torch fp32 restatement's error + one fp32 ulp of the
    largest value); bf16 ones: one bf16 rounding (2^-8 |ref|) + that bar (+ the measured fast-math constant for the two
    kernels that call __expf / tanhf);
  * hidden head backward: test_rmsnorm_backward_residual_epilogue's 2^-15 ref_max + 1e-4 on hi + lo, 2^-8 ref_max on hi.
Everything else is compared bit for bit: a pair alone / packed / in a permuted packing, a head of the H = 6 call against
an H = 1 call on its columns, two runs of one call, a row of the hidden head at any position in any T; outputs lie in
guarded arenas pre-filled with a sentinel, and exactly the rows of real tokens are written.

RP_DEC_MARGINS_OUT=<path>: every measured value and bound is written there as JSON (profiles/decoder_kernel_margins.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_kernel_helpers as dk  # noqa: E402
import hip_helpers as hh  # noqa: E402
import test_step_ends_gpu as step_ends  # noqa: E402  (the fp32 bar: its derivation, not a copy)
from reprover_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = hh.MIN_GUARD
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    if "decoder_kernels" in step_ends._worst:
        MARGINS["fp32_outputs_worst_kernel_over_bar"] = list(step_ends._worst["decoder_kernels"])
    path = os.environ.get("RP_DEC_MARGINS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _pad(n, to=128):
    return max((n + to - 1) // to * to, to)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == hh.OUTPUT_BYTE).all())


def _all_written(t):
    """No element still holds the sentinel pattern (0x5A5A = 1.5e13 in bf16, 1.5e16 in fp32: no result is near it)."""
    s = torch.full((t.element_size(),), hh.OUTPUT_BYTE, dtype=torch.uint8).view(t.dtype)[0].item()
    return not bool((t == s).any())


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def run_attention(c):
    """One rp_dbg_decoder_attention call on case ``c`` -> (arenas by name, Tp, Sp).  Operand rows beyond the real ones hold
    NaN (they are never to be read); every output is an Arena pre-filled with the sentinel byte."""
    H, causal, inner = c["H"], c["causal"], c["H"] * 64
    T, S = c["q"].shape[0], c["k"].shape[0]
    Tp, Sp = _pad(T), _pad(S)
    nan = float("nan")
    d_o = torch.full((Tp, inner), nan, dtype=torch.bfloat16, device=DEV)
    d_o[:T] = _bf16(c["d_o"])
    q_cu = np.concatenate([[0], np.cumsum([p[0] for p in c["pairs"]])]).astype(np.int32)
    k_cu = np.concatenate([[0], np.cumsum([p[1] for p in c["pairs"]])]).astype(np.int32)
    if causal:
        q = torch.full((Tp, 3 * inner), nan, dtype=torch.bfloat16, device=DEV)
        q[:T] = torch.cat([_bf16(c["q"]), _bf16(c["k"]), _bf16(c["v"])], 1)
        kv = None
        tab = torch.from_numpy(c["tab"].astype(np.float32)).to(DEV).contiguous()
        bucket = np.ascontiguousarray(c["bucket_of"], dtype=np.int32)
    else:
        q = torch.full((Tp, inner), nan, dtype=torch.bfloat16, device=DEV)
        q[:T] = _bf16(c["q"])
        kv = torch.full((Sp, 2 * inner), nan, dtype=torch.bfloat16, device=DEV)
        kv[:S] = torch.cat([_bf16(c["k"]), _bf16(c["v"])], 1)
        tab, bucket = None, None
    A = {
        "out": hh.Arena("out", Tp * inner * 2, GUARD, DEV, dtype=torch.bfloat16),
        "lse2": hh.Arena("lse2", H * Tp * 4, GUARD, DEV, dtype=torch.float32),
        "delta": hh.Arena("delta", H * Tp * 4, GUARD, DEV, dtype=torch.float32),
        "dq": hh.Arena("dq", Tp * (3 if causal else 1) * inner * 2, GUARD, DEV, dtype=torch.bfloat16),
    }
    if causal:
        A["dtab"] = hh.Arena("dtab", c["nbuckets"] * H * 4, GUARD, DEV, dtype=torch.float32)
    else:
        A["dkv"] = hh.Arena("dkv", Sp * 2 * inner * 2, GUARD, DEV, dtype=torch.bfloat16)
    lib = _lib.load()
    st = lib.rp_dbg_decoder_attention(
        1 if causal else 0, _lib.ptr(q), _lib.ptr(kv), _lib.ptr(d_o), q_cu.ctypes.data, k_cu.ctypes.data, len(c["pairs"]), H,
        _lib.ptr(tab), c["nbias"] if causal else 0, bucket.ctypes.data if causal else None, c["nbuckets"] if causal else 0,
        A["out"].ptr, A["lse2"].ptr, A["delta"].ptr, A["dq"].ptr, A["dkv"].ptr if not causal else None,
        A["dtab"].ptr if causal else None, _lib.current_stream())
    _lib.check(st, "rp_dbg_decoder_attention")
    torch.cuda.synchronize()
    return A, Tp, Sp


def attention_tensors(c, A, Tp, Sp):
    """The arenas as device tensors in the reference's shapes (real rows only): out, dq [T, inner], dk, dv [S, inner],
    lse2, delta [H, T], dtab [nbuckets, H]."""
    H, inner = c["H"], c["H"] * 64
    T, S = c["q"].shape[0], c["k"].shape[0]
    t = dict(out=A["out"].view(Tp, inner)[:T], lse2=A["lse2"].view(H, Tp)[:, :T], delta=A["delta"].view(H, Tp)[:, :T])
    if c["causal"]:
        g = A["dq"].view(Tp, 3 * inner)[:T]
        t.update(dq=g[:, :inner], dk=g[:, inner : 2 * inner], dv=g[:, 2 * inner :], dtab=A["dtab"].view(c["nbuckets"], H))
    else:
        g = A["dkv"].view(Sp, 2 * inner)[:S]
        t.update(dq=A["dq"].view(Tp, inner)[:T], dk=g[:, :inner], dv=g[:, inner:])
    return {k: v.clone() for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _gpu(name):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = dk.attention_case(name)
    A, Tp, Sp = run_attention(c)
    return c, A, Tp, Sp, attention_tensors(c, A, Tp, Sp)


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = dk.attention_case(name)
    exact, rounded = dk.attention_reference(c), dk.attention_reference(c, rounded=True)
    return exact, dk.attention_bounds(name, exact, rounded)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", sorted(dk.ATTENTION_CASES))
def test_attention_against_float64(name):
    c, _, _, _, t = _gpu(name)
    exact, bounds = _refs(name)
    if c["causal"]:
        lib = _lib.load()
        nb, md = c["nbuckets"], (c["nbias"] - 1) // 2
        if not np.array_equal(c["bucket_of"], np.arange(c["nbias"])):  # the map is the product's
            assert [lib.rp_relative_position_bucket_causal(-j, nb, md) for j in range(c["nbias"])] == c["bucket_of"].tolist()
    got = {k: _f64(v) for k, v in t.items()}
    margins = MARGINS.setdefault("attention", {}).setdefault(name, {})
    found = dk.attention_findings(c, got, exact, bounds, margins)
    for k, m in sorted(margins.items()):
        print(f"{name} {k}: {m}")
    assert not found, found


@pytest.mark.parametrize("name", sorted(dk.ATTENTION_CASES))
def test_attention_writes_exactly_the_real_rows(name):
    c, A, Tp, Sp, t = _gpu(name)
    H, inner = c["H"], c["H"] * 64
    T, S = c["q"].shape[0], c["k"].shape[0]
    for a in A.values():
        assert a.broken_guards() == [], a.name
    assert _untouched(A["out"].view(Tp, inner)[T:]) and _all_written(t["out"])
    for n in ("lse2", "delta"):
        assert _untouched(A[n].view(H, Tp)[:, T:]) and _all_written(t[n]), n
    assert all(bool(torch.isfinite(v.float()).all()) for v in t.values()), "a padding row (NaN) was read"
    if c["causal"]:
        assert _untouched(A["dq"].view(Tp, 3 * inner)[T:]) and _all_written(A["dq"].view(Tp, 3 * inner)[:T])
        assert _all_written(t["dtab"])
    else:
        assert _untouched(A["dq"].view(Tp, inner)[T:]) and _all_written(t["dq"])
        _, krows = dk.real_rows(c)
        rest = np.setdiff1d(np.arange(Sp), krows)  # S .. Sp and the source whose target is empty
        assert len(rest) == Sp - S + 70
        g = A["dkv"].view(Sp, 2 * inner)
        assert _untouched(g[torch.from_numpy(rest).to(DEV)]) and _all_written(g[torch.from_numpy(krows).to(DEV)])


BITWISE = ("out", "lse2", "delta", "dq", "dk", "dv")


def _rows_of(t, name, qrows, krows, cols=None):
    """Tensor ``name`` of the whole call restricted to a sub-call's rows (and columns / heads)."""
    x = t[name]
    if name in ("lse2", "delta"):
        x = x[:, torch.from_numpy(qrows).to(DEV)]
        return x if cols is None else x[torch.from_numpy(cols[::64] // 64).to(DEV)]
    x = x[torch.from_numpy(krows if name in ("dk", "dv") else qrows).to(DEV)]
    return x if cols is None else x[:, torch.from_numpy(cols).to(DEV)]


@pytest.mark.parametrize("name", ["causal-h2-n33-buckets", "cross-h2"])
def test_a_pair_has_the_same_bits_alone_packed_and_permuted(name):
    c, _, _, _, t = _gpu(name)
    n = len(c["pairs"])
    orders = [[b] for b in range(n) if c["pairs"][b][0]] + [list(np.random.default_rng(2).permutation(n))]
    assert orders[-1] != list(range(n))
    for order in orders:
        sub = dk.subcase(c, order)
        ts = attention_tensors(sub, *run_attention(sub))
        for k in BITWISE:
            assert _same_bits(ts[k], _rows_of(t, k, sub["qrows"], sub["krows"])), (name, order, k)


@pytest.mark.parametrize("name", ["causal-h6-n257-identity", "cross-h6"])
def test_a_head_of_six_has_the_bits_of_a_one_head_call(name):
    c, _, _, _, t = _gpu(name)
    for h in range(c["H"]):
        sub = dk.subcase(c, list(range(len(c["pairs"]))), heads=[h])
        ts = attention_tensors(sub, *run_attention(sub))
        for k in BITWISE:
            assert _same_bits(ts[k], _rows_of(t, k, sub["qrows"], sub["krows"], sub["cols"])), (name, h, k)
        if c["causal"]:  # one head's table gradient: its own workgroups' partial rows in the same order
            assert _same_bits(ts["dtab"][:, 0], t["dtab"][:, h]), (name, h)


@pytest.mark.parametrize("name", sorted(dk.ATTENTION_CASES))
def test_attention_is_bit_reproducible(name):
    c, A, Tp, Sp, _ = _gpu(name)
    B, _, _ = run_attention(c)
    for k in A:
        assert torch.equal(A[k].payload(), B[k].payload()), (name, k)


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
def rows_call(mode, a, b=None, ia=None, n_tok=0, rows_pad=0, n=0, vocab=0, flag=0, eps=0.0, scale=1.0, o0=None, o1=None, o2=None):
    p = lambda x: None if x is None else (x.ptr if isinstance(x, hh.Arena) else _lib.ptr(x))  # noqa: E731
    st = _lib.load().rp_dbg_decoder_rows(mode, p(a), p(b), p(ia), n_tok, rows_pad, n, vocab, flag, eps, scale, p(o0), p(o1),
                                         p(o2), _lib.current_stream())
    _lib.check(st, f"rp_dbg_decoder_rows({mode})")
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fp32_check(tag, got, yard, want):
    """tests/test_step_ends_gpu.py's bar on up to three fp32 outputs (device tensors / float64 arrays)."""
    step_ends._compare_with_yardstick(tag, "decoder_kernels", tuple(got), tuple(yard), tuple(want))


@pytest.mark.parametrize("V", [64, 320, 384, 512])
def test_bwd_dlogits(V):
    logits, labels, n_tok, rows = dk.dlogits_inputs(V)
    count = float(((labels >= 0) & (labels < V)).sum())
    lg, lab = _dev(logits), _dev(labels)
    ref = dk.dlogits_reference(logits.astype(np.float64), labels, n_tok, count)
    yard = _f64(dk.dlogits_yardstick(lg, labels, n_tok, count))
    out = hh.Arena("dlogits", rows * V * 2, GUARD, DEV, dtype=torch.bfloat16)
    rows_call(0, lg, torch.tensor([123.0, count], dtype=torch.float64, device=DEV), lab, n_tok, rows, V, o0=out)
    first = out.payload().clone()
    got = out.view(rows, V)
    assert out.broken_guards() == [] and _all_written(got)
    zero = np.concatenate([np.arange(n_tok, rows), np.flatnonzero((labels < 0) | (labels >= V))])
    assert not bool(got[_dev(zero)].view(torch.int16).any()), "padding and ignored rows are exactly zero"
    m = MARGINS.setdefault("rows", {})
    found = dk.bf16_row_findings(f"dlogits V={V}", _f64(got), ref, yard, dk.FASTMATH_DLOGITS, m)
    print(m[f"dlogits V={V}"])
    assert not found, found
    rows_call(0, lg, torch.tensor([123.0, count], dtype=torch.float64, device=DEV), lab, n_tok, rows, V, o0=out)
    assert torch.equal(first, out.payload())
    out.reset()
    rows_call(0, lg, torch.zeros(2, dtype=torch.float64, device=DEV), lab, n_tok, rows, V, o0=out)
    assert not bool(out.view(rows, V).view(torch.int16).any()), "count 0: every row is zero"


@pytest.mark.parametrize("D", [128, 1472])
def test_bwd_cast_is_torchs_cast(D):
    rng = np.random.default_rng(D)
    n_tok, rows = 130, 256
    x = (rng.standard_normal((rows, D)) * np.exp(rng.uniform(-60, 60, (rows, D)))).astype(np.float32)
    x[0, :8] = [0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, 1e-40, 65280.0, 3.0e38]  # ties both ways, a subnormal
    xd = _dev(x)
    out = hh.Arena("cast", rows * D * 2, GUARD, DEV, dtype=torch.bfloat16)
    rows_call(1, xd, n_tok=n_tok, rows_pad=rows, n=D, o0=out)
    got = out.view(rows, D)
    assert out.broken_guards() == []
    assert _same_bits(got[:n_tok], torch.from_numpy(x[:n_tok]).to(torch.bfloat16).to(DEV))
    assert np.array_equal(_f64(got[:n_tok]), dk.bf16_round(x[:n_tok]))
    assert not bool(got[n_tok:].view(torch.int16).any())


@pytest.mark.parametrize("D", [128, 1472, 1536])
def test_bwd_rmsnorm_and_colsum(D):
    eps = 1e-6
    for n_tok in (1, 63, 65, 130):
        for add in (0, 1):
            for scale in (1.0, float(np.float32(D ** -0.5))):
                rng = np.random.default_rng(D + 7 * n_tok + add)
                x = (rng.standard_normal((n_tok, D)) * 3.0).astype(np.float32)
                w = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
                dh = rng.standard_normal((n_tok, D)).astype(np.float32)
                dx0 = rng.standard_normal((n_tok, D)).astype(np.float32)
                want = dk.rmsnorm_bwd_reference(x.astype(np.float64), w.astype(np.float64), dh.astype(np.float64), eps, scale,
                                                dx0.astype(np.float64) if add else None)
                xd, wd, dhd, dx0d = _dev(x), _dev(w), _dev(dh), _dev(dx0)
                rs = torch.rsqrt((xd * xd).mean(1, keepdim=True) + eps)
                ydx = scale * (wd * rs * dhd - xd * rs ** 3 * ((dhd * wd * xd).sum(1, keepdim=True) / D))
                yterms = scale * dhd * xd * rs
                yard = (dx0d + ydx if add else ydx, yterms, yterms.sum(0))
                a_dh = hh.Arena.of("dh", dhd, GUARD)
                a_dx = hh.Arena.of("dx", dx0d, GUARD) if add else hh.Arena("dx", n_tok * D * 4, GUARD, DEV, dtype=torch.float32)
                a_dw = hh.Arena("dln", D * 4, GUARD, DEV, dtype=torch.float32)
                rows_call(2, xd, wd, n_tok=n_tok, n=D, flag=add, eps=eps, scale=scale, o0=a_dh, o1=a_dx, o2=a_dw)
                got = (a_dx.view(n_tok, D), a_dh.view(n_tok, D), a_dw.view(D))
                for a in (a_dh, a_dx, a_dw):
                    assert a.broken_guards() == [], a.name
                assert all(_all_written(g) for g in got)
                _fp32_check(f"bwd_rmsnorm D={D} rows={n_tok} add={add} scale={scale:.4f} (dx, dh, d ln)", got, yard, want)
    print("worst kernel / bar:", step_ends._worst.get("decoder_kernels"))


@pytest.mark.parametrize("F", [64, 256, 3584])
def test_bwd_geglu(F):
    gu, dff, n_tok, rows = dk.geglu_inputs(F)
    gud, dffd = _dev(gu), _dev(dff)
    ref = dk.geglu_bwd_reference(gu.astype(np.float64), dff.astype(np.float64), n_tok)
    yard = _f64(dk.geglu_bwd_reference(gud, dffd, n_tok))
    out = hh.Arena("dgu", rows * 2 * F * 2, GUARD, DEV, dtype=torch.bfloat16)
    rows_call(3, gud, dffd, n_tok=n_tok, rows_pad=rows, n=F, o0=out)
    got = out.view(rows, 2 * F)
    assert out.broken_guards() == [] and _all_written(got)
    assert not bool(got[n_tok:].view(torch.int16).any()), "padding rows are exactly zero"
    m = MARGINS.setdefault("rows", {})
    found = dk.bf16_row_findings(f"geglu F={F}", _f64(got), ref, yard, dk.FASTMATH_GEGLU, m)
    print(m[f"geglu F={F}"])
    assert not found, found


@pytest.mark.parametrize("D", [128, 1472])
def test_bwd_embed(D):
    V = 384
    for T in (1, 255, 256, 257, 600):
        for add in (0, 1):
            ids, dx = dk.embed_inputs(T, V, D)
            base = np.random.default_rng(T + add).standard_normal((V, D)).astype(np.float32)
            want = dk.embed_bwd_reference(ids, dx.astype(np.float64), V, base if add else None)
            start = torch.from_numpy(base) if add else torch.zeros(V, D)
            yard = start.clone().index_add_(0, torch.from_numpy(np.clip(ids, 0, V - 1)).long(), torch.from_numpy(dx))
            idd, dxd = _dev(ids), _dev(dx)
            tab = hh.Arena.of("dtable", _dev(base), GUARD) if add else hh.Arena("dtable", V * D * 4, GUARD, DEV, dtype=torch.float32)
            rows_call(4, dxd, ia=idd, n_tok=T, n=D, vocab=V, flag=add, o0=tab)
            got = tab.view(V, D).clone()
            assert tab.broken_guards() == [] and _all_written(got)
            never = np.setdiff1d(np.arange(V), np.clip(ids, 0, V - 1))
            assert len(never) > 300 and {33, 34, V - 2} <= set(never.tolist())
            if add:
                assert _same_bits(got[_dev(never)], _dev(base)[_dev(never)]), "rows of ids that never occur are untouched"
            else:
                assert not bool(got[_dev(never)].view(torch.int32).any()), "rows of ids that never occur are exactly zero"
            _fp32_check(f"bwd_embed D={D} T={T} add={add}", (got,), (yard.to(DEV),), (want,))
            tab.reset()
            rows_call(4, dxd, ia=idd, n_tok=T, n=D, vocab=V, flag=add, o0=tab)
            assert _same_bits(tab.view(V, D), got), "bit-reproducible"


# ---------------------------------------------------------------------------------------------------------------------------
# the last_hidden_state head
# ---------------------------------------------------------------------------------------------------------------------------
def run_hidden_head(planes, rs, w, dh, T, D):
    Tp = _pad(T, 256)
    A = {n: hh.Arena(n, Tp * D * 2, GUARD, DEV, dtype=torch.bfloat16) for n in ("out", "dxhi", "dxlo")}
    A["dln"] = hh.Arena("dln", D * 4, GUARD, DEV, dtype=torch.float32)
    st = _lib.load().rp_dbg_hidden_head(_lib.ptr(planes[0]), _lib.ptr(planes[1]), _lib.ptr(rs), _lib.ptr(w), _lib.ptr(dh), T, D,
                                        A["out"].ptr, A["dxhi"].ptr, A["dxlo"].ptr, A["dln"].ptr, _lib.current_stream())
    _lib.check(st, "rp_dbg_hidden_head")
    torch.cuda.synchronize()
    for n, a in A.items():
        assert a.broken_guards() == [], n
        if n != "dln":
            assert _untouched(a.view(Tp, D)[T:]), f"rows T .. Tp of {n} are untouched"
            assert _all_written(a.view(Tp, D)[:T]), n
    return {n: (a.view(Tp, D)[:T] if n != "dln" else a.view(D)).clone() for n, a in A.items()}


@pytest.mark.parametrize("D", [128, 1472, 1536, 2048])
def test_hidden_head(D):
    rng = np.random.default_rng(D)
    N = 65
    x = _dev((rng.standard_normal((N, D)) * 4.0).astype(np.float32))
    planes = hh.split_planes(x)
    xs = planes[0].float() + planes[1].float()
    rs = torch.rsqrt((xs * xs).mean(1) + 1e-6).contiguous()
    w = _dev((1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32))
    dh = _dev(rng.standard_normal((N, D)).astype(np.float32))
    full = None
    m = MARGINS.setdefault("hidden_head", {})
    for T in (65, 1, 2, 7, 8, 9, 31, 32, 33):
        pl = planes[:, :T].contiguous()
        got = run_hidden_head(pl, rs[:T].contiguous(), w, dh[:T].contiguous(), T, D)
        r_out, r_dx, r_dw = dk.hidden_head_reference(_f64(pl[0]), _f64(pl[1]), _f64(rs[:T]), _f64(w), _f64(dh[:T]))
        r = rs[:T, None]
        y_out = w * (xs[:T] * r)
        found = dk.bf16_row_findings(f"hidden_head D={D} T={T}", _f64(got["out"]), r_out, _f64(y_out), 0.0, m)
        assert not found, found
        ref_max = float(np.abs(r_dx).max())
        e_sum = float(np.abs(_f64(got["dxhi"]) + _f64(got["dxlo"]) - r_dx).max())
        e_hi = float(np.abs(_f64(got["dxhi"]) - r_dx).max())
        m[f"hidden_head_bwd D={D} T={T}"] = dict(sum_err=e_sum, sum_bar=2 ** -15 * ref_max + 1e-4, hi_err=e_hi,
                                                 hi_bar=2 ** -8 * ref_max)
        print(f"hidden_head_bwd D={D} T={T}:", m[f"hidden_head_bwd D={D} T={T}"])
        assert e_sum <= 2 ** -15 * ref_max + 1e-4 and e_hi <= 2 ** -8 * ref_max
        _fp32_check(f"hidden_head D={D} T={T} (d ln)", (got["dln"],), ((dh[:T] * xs[:T] * r).sum(0),), (r_dw,))
        if full is None:
            full = got
        else:  # the per-row parts do not depend on T (the weight gradient does)
            for n in ("out", "dxhi", "dxlo"):
                assert _same_bits(got[n], full[n][:T]), (D, T, n)
    # ... nor on the row's position: 33 rows in reverse order
    perm = torch.arange(32, -1, -1, device=DEV)
    got = run_hidden_head(planes[:, perm].contiguous(), rs[perm].contiguous(), w, dh[perm].contiguous(), 33, D)
    for n in ("out", "dxhi", "dxlo"):
        assert _same_bits(got[n], full[n][perm]), (D, "reversed", n)
