"""The decoder's attention kernels in their dropout form, alone on the MI355X, through
rp_dbg_decoder_attention_dropout: dec_flash_kernel<.., true>, both passes of dec_flash_bwd_kernel<.., true> and (causal)
bias_grad_kernel through the launch functions rp_decoder_loss_grad_dropout runs.

out, dq, dk, dv and dtab against the exact float64 form of tests/decoder_kernel_helpers.py extended with the mask the
kernels used (read back with rp_dbg_dropout_mask at the packed rows): relative L2 and worst row at most GRAD_TOL_FACTOR x
the rounded form's own error under the same mask.  lse2 is the UNDROPPED row's, within 1e-3.  p = 0 through this entry
gives rp_dbg_decoder_attention's bits; a pair alone equals the pair packed once the mask is read at the packed rows (the
mask's rows are packed indices); outputs lie in guarded arenas pre-filled with a sentinel and exactly the real rows are
written.  With one key per query (a pair's first query, or a one-token source) P = 1 and out is exactly 0 where the mask
dropped, else v times the fp32 multiplier 1 / (1 - p) rounded to bf16 at R_P (the P V operand: 1.109375 at p = 0.1, 2 at
p = 0.5) to one bf16 rounding (the row's own exp2 and 1 / l are within an fp32 ulp of 1, which can move a tie).

The row sites (the residual, gated-GELU, embedding and final-norm masks at tile edges) are held through a one-layer decoder
by tests/test_seq2seq_dropout_gpu.py::test_row_sites_at_tile_edges_through_a_one_layer_decoder."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_kernel_helpers as dk  # noqa: E402
import hip_helpers as hh  # noqa: E402
import seq2seq_dropout_helpers as sdh  # noqa: E402
from reprover_amd import _lib  # noqa: E402
from reprover_amd import decoder as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = hh.MIN_GUARD
SEED = 20241
CAUSAL_LENS = (1, 63, 64, 65, 128, 129, 257)
CROSS_PAIRS = ((1, 300), (65, 129), (129, 65), (257, 1), (0, 70))
# name -> (causal, H, p, site)
CASES = {
    "causal-h1": (True, 1, 0.1, D.DROP_SITE_DEC_LAYER0 + D.DEC_SELF_PROBS),
    "causal-h2": (True, 2, 0.1, D.DROP_SITE_DEC_LAYER0 + 8 + D.DEC_SELF_PROBS),
    "cross-h1": (False, 1, 0.1, D.DROP_SITE_DEC_LAYER0 + D.DEC_CROSS_PROBS),
    "cross-h2": (False, 2, 0.1, D.DROP_SITE_DEC_LAYER0 + 8 + D.DEC_CROSS_PROBS),
    "causal-h2-p0.5": (True, 2, 0.5, D.DROP_SITE_DEC_LAYER0 + D.DEC_SELF_PROBS),
}


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _pad(n, to=128):
    return max((n + to - 1) // to * to, to)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == hh.OUTPUT_BYTE).all())


def _all_written(t):
    s = torch.full((t.element_size(),), hh.OUTPUT_BYTE, dtype=torch.uint8).view(t.dtype)[0].item()
    return not bool((t == s).any())


def make_case(name):
    causal, H, p, site = CASES[name]
    rng = np.random.default_rng(17 + sum(map(ord, name)))
    pairs = [(n, n) for n in CAUSAL_LENS] if causal else list(CROSS_PAIRS)
    return dk.make_attention_case(rng, causal, H, pairs, 33 if causal else 0, (8, 16) if causal else None, 0.6, name), p, site


def run_attention(c, p=None, seed=SEED, site=0):
    """tests/test_decoder_kernels_gpu.py's run_attention through rp_dbg_decoder_attention_dropout (p None: the plain entry)"""
    H, causal, inner = c["H"], c["causal"], c["H"] * 64
    T, S = c["q"].shape[0], c["k"].shape[0]
    Tp, Sp = _pad(T), _pad(S)
    nan = float("nan")
    d_o = torch.full((Tp, inner), nan, dtype=torch.bfloat16, device=DEV)
    d_o[:T] = _bf16(c["d_o"])
    q_cu = np.concatenate([[0], np.cumsum([x[0] for x in c["pairs"]])]).astype(np.int32)
    k_cu = np.concatenate([[0], np.cumsum([x[1] for x in c["pairs"]])]).astype(np.int32)
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
    head = (1 if causal else 0, _lib.ptr(q), _lib.ptr(kv), _lib.ptr(d_o), q_cu.ctypes.data, k_cu.ctypes.data, len(c["pairs"]), H,
            _lib.ptr(tab), c["nbias"] if causal else 0, bucket.ctypes.data if causal else None, c["nbuckets"] if causal else 0)
    tail = (A["out"].ptr, A["lse2"].ptr, A["delta"].ptr, A["dq"].ptr, A["dkv"].ptr if not causal else None,
            A["dtab"].ptr if causal else None, _lib.current_stream())
    if p is None:
        _lib.check(lib.rp_dbg_decoder_attention(*head, *tail), "rp_dbg_decoder_attention")
    else:
        _lib.check(lib.rp_dbg_decoder_attention_dropout(*head, p, seed, site, *tail), "rp_dbg_decoder_attention_dropout")
    torch.cuda.synchronize()
    return A, Tp, Sp


def attention_tensors(c, A, Tp, Sp):
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
    c, p, site = make_case(name)
    A, Tp, Sp = run_attention(c, p, SEED, site)
    return c, p, site, A, Tp, Sp, attention_tensors(c, A, Tp, Sp)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", sorted(CASES))
def test_dropout_attention_against_float64_under_the_read_back_mask(name):
    c, p, site, _, _, _, t = _gpu(name)
    masks = sdh.attention_masks(c, p, SEED, site)
    exact = sdh.attention_reference_dropout(c, masks)
    rounded = sdh.attention_reference_dropout(c, masks, rounded=True)
    bounds = dk.attention_bounds("dropout-" + name, exact, rounded)
    got = {k: _f64(v) for k, v in t.items()}
    margins = {}
    found = dk.attention_findings(c, got, exact, bounds, margins)
    for k, m in sorted(margins.items()):
        print(f"{name} {k}: {m}")
    assert not found, found
    plain = dk.attention_reference(c)
    assert float(np.abs(got["lse2"] - plain["lse2"]).max()) <= dk.LSE2_BAR  # the undropped row's
    assert dk.rel_l2(got["out"], plain["out"]) > 0.05  # and the output is not the undropped one
    kept = np.concatenate([m.reshape(-1) for m in masks if m is not None])
    q = 1.0 - round(p * 65536) / 65536.0
    assert abs((kept != 0).mean() - q) <= 5 * np.sqrt(q * (1 - q) / kept.size)


@pytest.mark.parametrize("name", ["causal-h2", "cross-h2", "causal-h2-p0.5"])
def test_a_single_key_row_is_v_times_the_kept_multiplier_or_zero(name):
    """the first query of a causal pair and every query over a one-token source see one key: P = 1, so the P V operand is
    bf16(M) and out = bf16(bf16(M) v) with M = 0 (exactly 0) or fp32 1 / (1 - p) (to one bf16 rounding, 2^-8 relative)"""
    c, p, site, _, _, _, t = _gpu(name)
    masks = sdh.attention_masks(c, p, SEED, site)
    scale = torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p))).to(torch.bfloat16).float().numpy()
    assert float(scale) == {0.1: 1.109375, 0.5: 2.0}[p]
    qs = ks = n = 0
    for b, (Tq, Tk) in enumerate(c["pairs"]):
        rows = [0] if (c["causal"] and Tq) else (range(Tq) if Tk == 1 else [])
        for i in rows:
            for h in range(c["H"]):
                m = masks[b][h][i, 0]
                got = _f64(t["out"][qs + i, h * 64 : h * 64 + 64])
                want = c["v"][ks, h * 64 : h * 64 + 64] * float(scale)
                if m == 0:
                    assert not got.any(), (b, i, h)
                else:
                    assert (np.abs(got - want) <= 2.0 ** -8 * np.abs(want)).all() and got.any(), (b, i, h)
                n += 1
        qs += Tq
        ks += Tk
    assert n >= 14


@pytest.mark.parametrize("name", ["causal-h2", "cross-h2"])
def test_p0_through_the_dropout_entry_gives_the_plain_entrys_bits(name):
    c, _, site = make_case(name)
    A, _, _ = run_attention(c)
    B, _, _ = run_attention(c, 0.0, SEED, site)
    for k in A:
        assert torch.equal(A[k].payload(), B[k].payload()), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dropout_attention_writes_exactly_the_real_rows_and_is_reproducible(name):
    c, p, site, A, Tp, Sp, t = _gpu(name)
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
    B, _, _ = run_attention(c, p, SEED, site)
    for k in A:
        assert torch.equal(A[k].payload(), B[k].payload()), (name, k)
    other, _, _ = run_attention(c, p, SEED + 1, site)
    assert not torch.equal(A["out"].payload(), other["out"].payload())


@pytest.mark.parametrize("name", ["causal-h2", "cross-h2"])
def test_a_pair_alone_equals_the_pair_packed_up_to_the_mask(name):
    """The mask's rows are packed query indices, so a pair run alone draws the mask of rows 0 .. Tq - 1, not its packed
    rows': alone it is held to the float64 form under the mask read at ITS rows, and it differs from its packed self."""
    c, p, site, _, _, _, t = _gpu(name)
    b = 3  # (128, 128) causal; (257, 1) cross
    sub = dk.subcase(c, [b])
    ts = attention_tensors(sub, *run_attention(sub, p, SEED, site))
    masks = sdh.attention_masks(sub, p, SEED, site)
    exact = sdh.attention_reference_dropout(sub, masks)
    bounds = dk.attention_bounds("dropout-alone-" + name, exact, sdh.attention_reference_dropout(sub, masks, rounded=True))
    found = dk.attention_findings(sub, {k: _f64(v) for k, v in ts.items()}, exact, bounds)
    assert not found, found
    # the same pair inside the packed call: its rows of the packed outputs are held to the same bar under the mask read at
    # its PACKED rows, which is another mask than the one it drew alone
    q0 = int(sub["qrows"][0])
    packed_masks = sdh.attention_masks(dict(sub, row0=[q0]), p, SEED, site)
    assert not np.array_equal(packed_masks[0], masks[0])
    exact_p = sdh.attention_reference_dropout(sub, packed_masks)
    rounded_p = sdh.attention_reference_dropout(sub, packed_masks, rounded=True)
    bounds_p = {k: v for k, v in dk.attention_bounds("dropout-packed-" + name, exact_p, rounded_p).items() if k != "dtab"}
    qr, kr = torch.from_numpy(sub["qrows"]).to(DEV), torch.from_numpy(sub["krows"]).to(DEV)
    got_p = {k: _f64(t[k][:, qr] if k in ("lse2", "delta") else t[k][kr if k in ("dk", "dv") else qr]) for k in
             ("out", "lse2", "delta", "dq", "dk", "dv")}
    found = dk.attention_findings(sub, got_p, exact_p, bounds_p)
    assert not found, found
    assert dk.rel_l2(_f64(ts["out"]), exact_p["out"]) > 0.05  # (alone, under the other mask, it is another output)
