"""The decode step's kernels alone on the MI355X (rp_decoder.hip: the code behind beam search, batched search, the slot pool
and sampling), each against the float64 restatement of the same operation (tests/decode_step_helpers.py), through the
test-only entry points rp_dbg_dec_gemm, rp_dbg_dec_rows and rp_dbg_dec_attention, which run the launch code dec_step_launch
runs.

GEMM: every K that reaches another KIT = ceil(K / 512) or leaves one lane / all but one lane of the last 64-piece group idle,
x the four epilogues (the parametrisation ids name the dec_gemm_kernel<KIT, EPI> instantiation), M in {1, 63, 64, 65, 130} x
N in {1, 3, 4, 5, 130}; N = 384 / 512; the cross-K/V shape M = 8193 (129 row blocks); lda > K and ldo > N.
  * integer operands that identify their indices: EPI_F32 / EPI_RESID equal float64 bit for bit, EPI_BF16 its rounding;
  * N(0, 1) operands: |err| <= (8 KIT + 6) 2^-24 sum |a w| (+ 2^-24 |result| for RESID's add, + 2^-8 |ref| for a bf16
    store; GEGLU: 2^-8 |ref| + both accumulators' terms propagated + FASTMATH_DEC_GEGLU, measured);
  * placement: a row alone has the bits it has at rows 0, 63, 64, 129 of the M = 130 call, a column those of the N = 130 call.
Attention: H in {1, 3, 6, 12}, nb in {1, 3, 64}, key counts {1, 2, 255, 256, 257, 258, 300, 1025, 8192}, tables of 257 and 33
entries, ancestry rows with repeated parents and out-of-range entries, slots at mixed positions, sources placed out of slot
order: out within one bf16 rounding + the fp32 bar (2 x a torch fp32 restatement's error + one ulp) of exact float64; a slot
alone has the bits it has in the mixed call; exactly the real rows are written.  Row kernels: log_softmax / rmsnorm against
float64 under the same bars, embed / store_kv bit for bit.  One whole-step run at d_model 520 / d_ff 2056 / H 3 / V 300 ties
the kernels back to the product's launch sequence.  tests/test_decode_step_kernels_cpu.py shows that the bars separate planted
bugs on these shapes.

RP_DEC_STEP_MARGINS_OUT=<path>: every measured value is written there as JSON (profiles/decode_step_kernel_margins.json)."""
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_step_helpers as ds  # noqa: E402
import hip_helpers as hh  # noqa: E402
from reprover_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = hh.MIN_GUARD
MARGINS = {}
NAN = float("nan")
RP_E_INVALID, RP_E_UNSUPPORTED = -1, -4  # include/reprover_hip.h


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("RP_DEC_STEP_MARGINS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == hh.OUTPUT_BYTE).all())


def _all_written(t):
    s = torch.full((t.element_size(),), hh.OUTPUT_BYTE, dtype=torch.uint8).view(t.dtype)[0].item()
    return not bool((t == s).any())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _nan_tail(x, extra=2):
    """x with ``extra`` NaN rows behind it (rows no kernel may read)."""
    out = torch.full((x.shape[0] + extra,) + tuple(x.shape[1:]), NAN, dtype=x.dtype, device=x.device)
    out[: x.shape[0]] = x
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_call(epi, A, W, N, out, lda=None, ldo=None, M=None, K=None, check=True):
    M = A.shape[0] if M is None else M
    K = A.shape[1] if K is None else K
    st = _lib.load().rp_dbg_dec_gemm(epi, _lib.ptr(A), K if lda is None else lda, M, _lib.ptr(W), N, K,
                                     out.ptr if isinstance(out, hh.Arena) else _lib.ptr(out), N if ldo is None else ldo,
                                     _lib.current_stream())
    torch.cuda.synchronize()
    if check:
        _lib.check(st, "rp_dbg_dec_gemm")
    return st


def run_gemm(epi, A, W, N, out0=None):
    """One call on float64 operands A [M, K], W [N or 2 N, K] -> the [M, N] output as a device tensor (an Arena pre-filled
    with the sentinel, or with out0 for EPI_RESID); NaN rows behind A and W; guards checked."""
    M = A.shape[0]
    dt = torch.bfloat16 if epi in (ds.EPI_BF16, ds.EPI_GEGLU) else torch.float32
    if epi == ds.EPI_RESID:
        out = hh.Arena.of("out", _f32(out0), GUARD)
    else:
        out = hh.Arena("out", M * N * (2 if dt == torch.bfloat16 else 4), GUARD, DEV, dtype=dt)
    gemm_call(epi, _nan_tail(_bf16(A)), _nan_tail(_bf16(W), 4), N, out, M=M)
    assert out.broken_guards() == []
    got = out.view(M, N).clone()
    assert _all_written(got)
    return got


def _gemm_id(K, epi):
    return f"K{K}-kit{ds.kit_of(K)}-{ds.EPI_NAMES[epi]}"


GEMM_PARAMS = [pytest.param(K, epi, id=_gemm_id(K, epi)) for K in ds.GEMM_KS for epi in range(4)]


@pytest.mark.parametrize("K,epi", GEMM_PARAMS)
def test_gemm_random_operands_within_the_derived_bar(K, epi):
    A, W, out0 = ds.gemm_operands(K)
    m = MARGINS.setdefault("gemm", {})
    found, excess = [], -np.inf
    for M in ds.GEMM_MS:
        for N in ds.GEMM_NS:
            a, w, o0 = A[:M], ds.gemm_w(W, N, epi, K), out0[:M, :N]
            got = _f64(run_gemm(epi, a, w, N, o0))
            extra = ds.FASTMATH_DEC_GEGLU if epi == ds.EPI_GEGLU else 0.0
            ref, bar = ds.gemm_bar(a, w, N, epi, o0, extra)
            found += ds.gemm_findings(f"{_gemm_id(K, epi)} worst |error| / bar", got, ref, bar, m)
            if epi == ds.EPI_GEGLU:
                excess = max(excess, float((np.abs(got - ref) - (bar - extra)).max()))
    print(_gemm_id(K, epi), "worst |error| / bar:", m[f"{_gemm_id(K, epi)} worst |error| / bar"])
    if epi == ds.EPI_GEGLU:  # what the derived part leaves over, absolute (<= 0: nothing)
        e = m.setdefault("geglu_fastmath_excess", {})
        e[f"K{K}"] = excess
        print(f"GEGLU K={K}: largest excess over the derived part {excess:.3e} (FASTMATH_DEC_GEGLU {ds.FASTMATH_DEC_GEGLU:.3e})")
    assert not found, found


@pytest.mark.parametrize("K,epi", [p for p in GEMM_PARAMS if p.values[1] != ds.EPI_GEGLU])
def test_gemm_integer_operands_are_exact(K, epi):
    A, W, out0 = ds.gemm_operands(K, "integer")
    for M, N in ((130, 130), (65, 5), (1, 1), (63, 3), (64, 4)):
        a, w, o0 = A[:M], ds.gemm_w(W, N, epi, K), out0[:M, :N]
        got = _f64(run_gemm(epi, a, w, N, o0))
        want = ds.gemm_exact_expected(a, w, N, epi, o0)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (_gemm_id(K, epi), M, N, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("K,epi", GEMM_PARAMS)
def test_gemm_a_row_and_a_column_have_the_same_bits_alone(K, epi):
    A, W, out0 = ds.gemm_operands(K)
    N = ds.GEMM_MAX_N
    full = run_gemm(epi, A, ds.gemm_w(W, N, epi, K), N, out0)
    for r in ds.GEMM_PLACEMENT_ROWS:
        alone = run_gemm(epi, A[r:r + 1], ds.gemm_w(W, N, epi, K), N, out0[r:r + 1])
        assert _same_bits(alone[0], full[r]), (_gemm_id(K, epi), "row", r)
    for c in ds.GEMM_PLACEMENT_COLS:
        alone = run_gemm(epi, A, ds.gemm_w(W, 1, epi, K, cols=[c]), 1, out0[:, c:c + 1])
        assert _same_bits(alone[:, 0], full[:, c]), (_gemm_id(K, epi), "column", c)


@pytest.mark.parametrize("K", [520, 1472])
def test_gemm_resid_adds_and_leaves_the_rest_untouched(K):
    """A 65 x 5 call into the middle of a 70 x 8 fp32 matrix (ldo = 8): the block gains the product, every other element
    keeps its bits."""
    A, W, _ = ds.gemm_operands(K)
    M, N, ldo = 65, 5, 8
    base = np.random.default_rng(K).standard_normal((70, ldo)).astype(np.float32)
    out = hh.Arena.of("out", _f32(base), GUARD)
    st = _lib.load().rp_dbg_dec_gemm(ds.EPI_RESID, _lib.ptr(_nan_tail(_bf16(A[:M]))), K, M, _lib.ptr(_nan_tail(_bf16(W[:N]))), N,
                                     K, out.ptr + 4 * (2 * ldo + 1), ldo, _lib.current_stream())
    _lib.check(st, "rp_dbg_dec_gemm")
    torch.cuda.synchronize()
    assert out.broken_guards() == []
    got = out.view(70, ldo).clone()
    inside = torch.zeros((70, ldo), dtype=torch.bool, device=DEV)
    inside[2:2 + M, 1:1 + N] = True
    assert _same_bits(got[~inside], _f32(base)[~inside]), "elements outside the block keep their bits"
    o0 = base[2:2 + M, 1:1 + N].astype(np.float64)
    ref, bar = ds.gemm_bar(A[:M], W[:N], N, ds.EPI_RESID, o0)
    assert ds.gemm_findings("resid block", _f64(got[2:2 + M, 1:1 + N]), ref, bar) == []
    assert float(np.abs(ref - o0).min()) > 0, "the block changed"


@pytest.mark.parametrize("epi", range(4), ids=[ds.EPI_NAMES[e] for e in range(4)])
def test_gemm_strides_wider_than_the_rows(epi):
    """lda > K and ldo > N: the gap columns of A hold NaN (never read), those of out keep the sentinel."""
    K, lda, M, N, ldo = 520, 528, 65, 5, 8
    A, W, out0 = ds.gemm_operands(K)
    a, w = A[:M], ds.gemm_w(W, N, epi, K)
    Ad = torch.full((M + 1, lda), NAN, dtype=torch.bfloat16, device=DEV)
    Ad[:M, :K] = _bf16(a)
    f32 = epi in (ds.EPI_RESID, ds.EPI_F32)
    out = hh.Arena("out", M * ldo * (4 if f32 else 2), GUARD, DEV, dtype=torch.float32 if f32 else torch.bfloat16)
    o0 = out0[:M, :N]
    if epi == ds.EPI_RESID:
        out.view(M, ldo)[:, :N] = _f32(o0)
    gemm_call(epi, Ad, _nan_tail(_bf16(w), 4), N, out, lda=lda, ldo=ldo, M=M, K=K)
    assert out.broken_guards() == []
    got = out.view(M, ldo)
    assert _untouched(got[:, N:]) and _all_written(got[:, :N])
    ref, bar = ds.gemm_bar(a, w, N, epi, o0, ds.FASTMATH_DEC_GEGLU)
    assert ds.gemm_findings("strided", _f64(got[:, :N]), ref, bar) == []
    assert _same_bits(got[:, :N], run_gemm(epi, a, w, N, o0)), "the same bits as the dense call"


@pytest.mark.parametrize("N,epi", [(384, ds.EPI_F32), (512, ds.EPI_F32), (384, ds.EPI_BF16), (512, ds.EPI_GEGLU)],
                         ids=["N384-f32", "N512-f32", "N384-bf16", "N512-geglu"])
def test_gemm_wide_outputs_at_k_1472(N, epi):
    K, M = 1472, 65
    rng = np.random.default_rng(N + epi)
    A = ds.bf16_round(rng.standard_normal((M, K)))
    W = ds.bf16_round(rng.standard_normal((2 * N if epi == ds.EPI_GEGLU else N, K)))
    if epi == ds.EPI_GEGLU:
        W[:N] *= 0.25
    got = _f64(run_gemm(epi, A, W, N))
    ref, bar = ds.gemm_bar(A, W, N, epi, None, ds.FASTMATH_DEC_GEGLU)
    found = ds.gemm_findings(f"N{N}-{ds.EPI_NAMES[epi]} worst |error| / bar", got, ref, bar, MARGINS.setdefault("gemm", {}))
    if epi == ds.EPI_GEGLU:
        MARGINS["gemm"].setdefault("geglu_fastmath_excess_other_calls", {})[f"N{N}"] = float(
            (np.abs(got - ref) - (bar - ds.FASTMATH_DEC_GEGLU)).max())
    assert not found, found


def test_gemm_cross_kv_shape_129_row_blocks():
    """rp_decoder_batch_cross_kv's shape: M = 8193 source rows (129 blocks in grid.y), N = 8, K = 1472, bf16 out."""
    K, M, N = 1472, 8193, 8
    rng = np.random.default_rng(8193)
    A = ds.bf16_round(rng.standard_normal((M, K)))
    W = ds.bf16_round(rng.standard_normal((N, K)))
    got = run_gemm(ds.EPI_BF16, A, W, N)
    ref, bar = ds.gemm_bar(A, W, N, ds.EPI_BF16)
    found = ds.gemm_findings("cross-kv M8193 worst |error| / bar", _f64(got), ref, bar, MARGINS.setdefault("gemm", {}))
    assert not found, found
    for r in (0, 64, 8191, 8192):  # the first row of a block, the last block's only row
        assert _same_bits(run_gemm(ds.EPI_BF16, A[r:r + 1], W, N)[0], got[r]), r


def test_gemm_refuses_k_above_4096_without_launching():
    K = 4104
    A = torch.full((2, K), NAN, dtype=torch.bfloat16, device=DEV)
    W = torch.full((2, K), NAN, dtype=torch.bfloat16, device=DEV)
    for epi in range(4):
        out = hh.Arena("out", 64, GUARD, DEV)
        assert gemm_call(epi, A, W, 1, out, check=False) == RP_E_UNSUPPORTED
        assert out.at_rest() and out.broken_guards() == []
    out = hh.Arena("out", 64, GUARD, DEV)
    assert gemm_call(0, A, W, 1, out, K=12, lda=16, check=False) == RP_E_INVALID  # K % 8 != 0 is outside the contract
    assert gemm_call(4, A, W, 1, out, K=8, check=False) == RP_E_INVALID
    assert out.at_rest()


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_operands(kind, name):
    """The case's buffers on the device, shared by the whole call and its one-slot calls."""
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    kv = _bf16(c["kv"].reshape(-1, c["ldkv"]))
    anc = None if c["cross"] else torch.from_numpy(c["anc"].astype(np.int32)).to(DEV)
    tab = None if c["cross"] else _f32(c["tab"])
    return kv, anc, tab


def run_attention(kind, name, c=None):
    """One rp_dbg_dec_attention call -> (Arena, R).  q: self-attention reads it from a [R, 3 inner] buffer whose k | v columns
    hold NaN (the product's qkv), cross from [R, inner]; two NaN rows behind; out: [R + 2, inner], sentinel-filled."""
    full = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    c = full if c is None else c
    kv, anc, tab = _device_operands(kind, name)
    H, nb, inner = c["H"], c["nb"], 64 * c["H"]
    R = c["q"].shape[0]
    ldq = inner if c["cross"] else 3 * inner
    q = torch.full((R + 2, ldq), NAN, dtype=torch.bfloat16, device=DEV)
    q[:R, :inner] = _bf16(c["q"])
    out = hh.Arena("out", (R + 2) * inner * 2, GUARD, DEV, dtype=torch.bfloat16)
    if not c["cross"] and "slot_of" in c:
        anc = anc[c["slot_of"] * nb:(c["slot_of"] + 1) * nb].contiguous()
    state, pos = _i32(c["state"]), _i32(c["pos"])
    off, ln = (_i32(c["src_off"]), _i32(c["src_len"])) if c["cross"] else (None, None)
    st = _lib.load().rp_dbg_dec_attention(
        1 if c["cross"] else 0, _lib.ptr(q), ldq, _lib.ptr(kv), c["ldkv"], c["koff"], c["voff"], c["rows"],
        0 if c["cross"] else c["rows"] * c["ldkv"], c["n_states"], _lib.ptr(anc), 0 if c["cross"] else c["astride"], _lib.ptr(tab),
        0 if c["cross"] else c["nbias"], nb, H, state.ctypes.data, off.ctypes.data if c["cross"] else None,
        ln.ctypes.data if c["cross"] else None, pos.ctypes.data, len(c["state"]), c["max_len"], out.ptr, inner,
        _lib.current_stream())
    _lib.check(st, "rp_dbg_dec_attention")
    torch.cuda.synchronize()
    return out, R


@functools.lru_cache(maxsize=None)
def _gpu(kind, name):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return run_attention(kind, name)


ATT_PARAMS = [("self", n) for n in sorted(ds.SELF_CASES)] + [("cross", n) for n in sorted(ds.CROSS_CASES)]
ATT_IDS = [f"{k}-{n}" for k, n in ATT_PARAMS]


@pytest.mark.parametrize("kind,name", ATT_PARAMS, ids=ATT_IDS)
def test_attention_against_float64(kind, name):
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    out, R = _gpu(kind, name)
    got = _f64(out.view(R + 2, 64 * c["H"])[:R])
    exact = ds.attention_reference(c)
    yard = ds.attention_yardstick(c, DEV)
    m = MARGINS.setdefault("attention", {})
    found = ds.attention_findings(f"{kind}-{name}", got, exact, yard, m)
    print(f"{kind}-{name}:", m[f"{kind}-{name}"])
    e = MARGINS.setdefault("attention_expf_excess", {})
    e[f"{kind}-{name}"] = m[f"{kind}-{name}"]["excess_over_rounding"] - m[f"{kind}-{name}"]["yardstick_bar"]
    assert not found, found


@pytest.mark.parametrize("kind,name", ATT_PARAMS, ids=ATT_IDS)
def test_attention_writes_exactly_its_rows_and_is_reproducible(kind, name):
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    out, R = _gpu(kind, name)
    v = out.view(R + 2, 64 * c["H"])
    assert out.broken_guards() == []
    assert _untouched(v[R:]) and _all_written(v[:R])
    assert bool(torch.isfinite(v[:R].float()).all()), "a NaN row or column (never to be read) was read"
    again, _ = run_attention(kind, name)
    assert torch.equal(out.payload(), again.payload())


@pytest.mark.parametrize("kind,name", [("self", "h3-nb3-n33-mixed"), ("self", "h6-nb1-n33"), ("cross", "h3-nb3"),
                                       ("cross", "h1-nb1-big")], ids=lambda x: x)
def test_a_slot_alone_has_the_bits_it_has_in_the_mixed_call(kind, name):
    """The LDS is sized by the call's longest key list; a short row must see its own keys only."""
    c = ds.cross_case(name) if kind == "cross" else ds.self_case(name)
    out, R = _gpu(kind, name)
    nb, inner = c["nb"], 64 * c["H"]
    full = out.view(R + 2, inner)
    for a in range(len(c["state"])):
        alone, r = run_attention(kind, name, ds.one_slot(c, a))
        assert r == nb and alone.broken_guards() == []
        assert _same_bits(alone.view(nb + 2, inner)[:nb], full[a * nb:(a + 1) * nb]), (kind, name, a)


def test_attention_refuses_a_bad_slot_table():
    c = ds.self_case("h3-nb3-n33-mixed")
    for change in (dict(pos=[0, 256, 40, 300]), dict(pos=[0, -1, 40, 299]), dict(state=[2, 0, 2, 1]), dict(state=[2, 0, 4, 1]),
                   dict(astride=299)):
        with pytest.raises(_lib.HipLibraryError):
            run_attention("self", "h3-nb3-n33-mixed", dict(c, **change))


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
def rows_call(mode, a=None, b=None, ia=None, rows=0, n=0, vocab=0, eps=0.0, scale=1.0, state=None, pos=None, n_states=0, nb=0,
              max_len=0, state_stride=0, o0=None):
    p = lambda x: None if x is None else (x.ptr if isinstance(x, hh.Arena) else _lib.ptr(x))  # noqa: E731
    st = _lib.load().rp_dbg_dec_rows(mode, p(a), p(b), p(ia), rows, n, vocab, eps, scale,
                                     None if state is None else state.ctypes.data, None if pos is None else pos.ctypes.data,
                                     0 if state is None else len(state), n_states, nb, max_len, state_stride, p(o0),
                                     _lib.current_stream())
    _lib.check(st, f"rp_dbg_dec_rows({mode})")
    torch.cuda.synchronize()


@pytest.mark.parametrize("V", ds.LOG_SOFTMAX_VS)
@pytest.mark.parametrize("rows", ds.LOG_SOFTMAX_ROWS)
def test_log_softmax(V, rows):
    x = ds.log_softmax_inputs(V, rows)
    ref = ds.log_softmax_reference(x)
    xd = _nan_tail(_f32(x))
    yard = _f64(torch.log_softmax(xd[:rows], -1))
    out = hh.Arena.of("lp", xd, GUARD)
    rows_call(2, rows=rows, n=V, o0=out)
    assert out.broken_guards() == []
    v = out.view(rows + 2, V)
    assert bool(torch.isnan(v[rows:]).all()), "rows beyond the grid are untouched"
    got = _f64(v[:rows])
    m = MARGINS.setdefault("rows", {})
    found = ds.fp32_findings(f"log_softmax V={V} rows={rows}", got, ref, yard, m)
    print(m[f"log_softmax V={V} rows={rows}"])
    assert not found, found
    if V == 1:
        assert not got.any(), "V = 1: exactly 0"
    lse = np.log(np.exp(got).sum(1))  # |d logsumexp| <= max |d x|: the same bar
    assert np.abs(lse).max() <= ds.yardstick_bar(ref, yard), lse
    first = out.payload().clone()
    out.reset()
    rows_call(2, rows=rows, n=V, o0=out)
    assert torch.equal(first, out.payload())


@pytest.mark.parametrize("D", ds.RMSNORM_DS)
def test_rmsnorm(D):
    x, w = ds.rmsnorm_inputs(D)
    xd, wd = _nan_tail(_f32(x)), _f32(w)
    for scale in (1.0, float(np.float32(D ** -0.5))):
        ref = ds.rmsnorm_reference(x, w, ds.RMS_EPS, scale)
        xs = xd[:5]
        yard = _f64(wd * (xs * torch.rsqrt((xs * xs).mean(1, keepdim=True) + ds.RMS_EPS)) * scale)
        out = hh.Arena("h", 7 * D * 2, GUARD, DEV, dtype=torch.bfloat16)
        rows_call(1, xd, wd, rows=5, n=D, eps=ds.RMS_EPS, scale=scale, o0=out)
        v = out.view(7, D)
        assert out.broken_guards() == [] and _untouched(v[5:]) and _all_written(v[:5])
        got = _f64(v[:5])
        assert not got[1].any(), "the all-zero row gives exactly 0"
        m = MARGINS.setdefault("rows", {})
        found = ds.bf16_row_findings(f"rmsnorm D={D} scale={scale:.4f}", got, ref, yard, 0.0, m)
        print(m[f"rmsnorm D={D} scale={scale:.4f}"])
        assert not found, found


@pytest.mark.parametrize("V,D", ds.EMBED_CASES)
def test_embed_is_bit_exact(V, D):
    table = np.random.default_rng(V + D).standard_normal((V, D)).astype(np.float32)
    ids = ds.embed_ids(V)
    n = len(ids)
    out = hh.Arena("x", (n + 2) * D * 4, GUARD, DEV, dtype=torch.float32)
    rows_call(0, _nan_tail(_f32(table)), ia=torch.from_numpy(ids).to(DEV), rows=n, n=D, vocab=V, o0=out)
    v = out.view(n + 2, D)
    assert out.broken_guards() == [] and _untouched(v[n:])
    assert _same_bits(v[:n], _f32(ds.embed_reference(ids, table)))


@pytest.mark.parametrize("H,nb", [(1, 1), (3, 3), (6, 64)])
def test_store_kv_writes_exactly_its_rows(H, nb):
    inner, max_len = 64 * H, 9
    state, pos = _i32([2, 0, 3]), _i32([8, 0, 5])
    n_states, rows = 4, max_len * nb
    rng = np.random.default_rng(H + nb)
    qkv = rng.integers(-2 ** 15, 2 ** 15, size=(3 * nb, 3 * inner)).astype(np.int16)  # bit patterns: every one must survive
    qd = torch.full((3 * nb + 2, 3 * inner), 0x7FC0, dtype=torch.int16, device=DEV)
    qd[: 3 * nb] = torch.from_numpy(qkv).to(DEV)
    out = hh.Arena("cache", n_states * rows * 2 * inner * 2, GUARD, DEV, dtype=torch.int16)
    before = out.view(n_states, rows, 2 * inner).cpu().numpy().copy()
    rows_call(3, qd, rows=3 * nb, n=inner, state=state, pos=pos, n_states=n_states, nb=nb, max_len=max_len,
              state_stride=rows * 2 * inner, o0=out)
    assert out.broken_guards() == []
    want = ds.store_kv_reference(qkv, before, state.tolist(), pos.tolist(), nb)
    got = out.view(n_states, rows, 2 * inner).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got != before).sum() > 0.99 * 3 * nb * 2 * inner


# ---------------------------------------------------------------------------------------------------------------------------
# the whole step off the two product geometries
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_step_at_kit_2_and_5_a_33_wide_table_and_v_300():
    """HipT5Decoder alone (no encoder) at d_model 520 / d_ff 2056 / H 3 / V 300, buckets (8, 16): 60 steps of a simulated
    search of 5 beams over a random bf16 [70, 520] source, in lockstep with T5DecodeEmu."""
    import test_decoder_parity_gpu as parity
    from gen_helpers import DECODER_TOL, T5DecodeEmu, simulated_search
    from reprover_amd import synth
    from reprover_amd.decoder import HipT5Decoder

    cfg = dict(synth.seq2seq_config("tiny"), **ds.STEP_CONFIG)
    sd = synth.synth_seq2seq_state_dict(cfg, scale="sharp")
    gen = types.SimpleNamespace(decoder=HipT5Decoder(cfg, sd, DEV))
    emu = T5DecodeEmu(cfg, sd, device=DEV)
    enc = torch.from_numpy(np.random.default_rng(70).standard_normal((70, cfg["d_model"])).astype(np.float32)).to(torch.bfloat16)
    step_max, rms, _, _ = parity._compare(gen, emu, enc.to(DEV).contiguous(), 5, 60, simulated_search(5, 60, 105, (3, 300)))
    MARGINS["whole_step"] = {ds.STEP_CASE: dict(max=float(step_max.max()), rms=rms, step_of_max=int(step_max.argmax()))}
    print(f"decode step {ds.STEP_CASE}: max |d lp| {step_max.max():.3e} (step {int(step_max.argmax())}), rms {rms:.3e}")
    assert len(step_max) == 60
    tol = DECODER_TOL[ds.STEP_CASE]
    assert step_max.max() <= tol[0] and rms <= tol[1], (step_max.max(), rms, tol)
