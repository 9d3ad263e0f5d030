"""The encoder's pooling head, its training row kernels and the weight pack / unpack kernels alone on the MI355X, each against
the float64 restatement of the same operation (tests/encoder_kernel_helpers.py), through the test-only entry points
rp_dbg_pool_head, rp_dbg_train_rows, rp_dbg_repack, rp_dbg_bias_table and rp_dbg_unfold, which run the launch functions the
encoder pass and the trainer run.

Shapes: d_model 128 / 1472 / 1536 / 1600 / 2048 (16 pieces, so most lanes clamped / the third 16-byte piece partly clamped /
NV = 3 full / NV = 4 partly / the limit); one packed call of 24 sequences of 1 .. 300 tokens whose offsets are not
chunk-aligned (edges: 4 waves, 8 and 16 rows in flight, chunks of 32 / 64 / 128).  Operand rows T .. Tp hold NaN; outputs lie in
guarded arenas pre-filled with a sentinel.  Bars (tests/test_encoder_train_kernels_cpu.py shows that each separates planted bugs
on these shapes; none is a measured number):
  * fp32 outputs: tests/test_step_ends_gpu.py's bar (2 x a torch fp32 restatement's error on the same inputs + one fp32 ulp of
    the largest reference value).  `partial` and `out` may fall back on the derived first-order bound (longest sequential chain
    + tree depth) x 2^-24 x sum |terms| per element where the kernel's fixed order is a longer chain than torch's tree: chunk / 4
    + 2 for a chunk's sums (+ 1 under dropout: the mask product is a rounding of its own), + the number of chunks through the
    finish; np + 3 for rowdot_finish_kernel (its slots are added in index order), 8 per 512 columns + 6 + 3 for
    qkv_scale_dot_kernel's row dot, the largest number of tokens sharing an id for the scatter, splits + 8 + row blocks for
    unfold_kernel's d ln.  Which bar an output needed is recorded in the margins file; measured on the MI355X, three did: rcoef
    of rowdot_finish_kernel at np = 56, rows = 65 (error 2.43e-8, yardstick bar 1.74e-8, 0.026 of the chain bound) and np = 65,
    rows = 1 (4.4e-10 / 2.9e-10 / 0.003), rcoef of qkv_scale_dot_kernel at width 1152, T = 1 (1.8e-10 / 7.6e-11 / 0.002).
  * two-plane outputs: per element |hi + lo - ref| <= 2^-16 |ref| + the fp32 bar, |hi - ref| <= 2^-8 |ref| + the same.
  * bf16 outputs that are one fp32 operation and a cast, permutations, and every alone / packed / reversed / run-to-run
    comparison: bit for bit.

RP_ENC_MARGINS_OUT=<path>: every measured value and bound is written there as JSON (profiles/encoder_train_kernel_margins.json)."""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_kernel_helpers as dk  # noqa: E402
import encoder_kernel_helpers as ek  # noqa: E402
import hip_helpers as hh  # noqa: E402
import test_step_ends_gpu as step_ends  # noqa: E402  (the fp32 bar: its derivation, not a copy)
from oracle import t5_ref  # noqa: E402
from reprover_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = hh.MIN_GUARD
GROUP = "encoder_train_kernels"
MARGINS = {}
RP_E_INVALID = -1
U = ek.U32


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    if GROUP in step_ends._worst:
        MARGINS["fp32_outputs_worst_kernel_over_bar"] = list(step_ends._worst[GROUP])
    path = os.environ.get("RP_ENC_MARGINS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _untouched(t):
    return bool((_bits(t) == hh.OUTPUT_BYTE).all())


def _all_written(t):
    s = torch.full((t.element_size(),), hh.OUTPUT_BYTE, dtype=torch.uint8).view(t.dtype)[0].item()
    return not bool((t == s).any())


def _fp32(what, got, ref, yard, bound=None, group="fp32"):
    """tests/test_step_ends_gpu.py's bar on one fp32 output (its own comparison, under this module's group name); where it
    misses and a derived chain bound is given, every element within that bound instead."""
    got64 = _f64(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    yard64 = _f64(yard) if torch.is_tensor(yard) else np.asarray(yard, np.float64)
    m = MARGINS.setdefault(group, {})
    found = ek.fp32_findings(what, got64, ref, yard64, bound, m)
    if m[what]["bar"] == "yardstick" and not found:
        step_ends._compare_with_yardstick(what, GROUP, (torch.from_numpy(got64),), (torch.from_numpy(yard64),), (ref,))
    else:
        MARGINS.setdefault("needed_chain_bound", {})[what] = m[what]
        print(f"  {what}: {m[what]}")
    assert not found, found
    return m[what]["yardstick_bar"]


def mask_of(p, seed, site, rows, cols):
    """The multipliers the kernels use at (site, rows 0 .., columns 0 ..), read back once: 0 or fp32 1 / (1 - p)."""
    out = torch.zeros(rows, cols, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().rp_dbg_dropout_mask(p, seed, site, 0, 0, rows, cols, _lib.ptr(out), _lib.current_stream()),
               "rp_dbg_dropout_mask")
    torch.cuda.synchronize()
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    return out.float() * scale.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# pooling head
# ---------------------------------------------------------------------------------------------------------------------------
def _pad(n, to=256):
    return (n + to - 1) // to * to


class Planes:
    """The residual stream of a packed call in one of the two formats, rows T .. Tp NaN; ``x``: the decoded values (fp32)."""

    def __init__(self, x32, lo8):
        T, D = x32.shape
        Tp = _pad(T + 1)
        self.lo8, self.T, self.Tp, self.D = lo8, T, Tp, D
        self.hi = torch.full((Tp, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        if lo8:
            _, hi, ext = hh.split_x24(x32)
            self.lo = torch.full((Tp, D), 0xFF, dtype=torch.uint8, device=DEV)
            self.hi[:T], self.lo[:T] = hi, ext
            self.x = hh.merge_x24(self.hi[:T], self.lo[:T]).contiguous()
        else:
            pl = hh.split_planes(x32)
            self.lo = torch.full((Tp, D), float("nan"), dtype=torch.bfloat16, device=DEV)
            self.hi[:T], self.lo[:T] = pl[0], pl[1]
            self.x = hh.merge_planes(torch.stack([self.hi[:T], self.lo[:T]])).contiguous()
        self.rs = torch.full((Tp,), float("nan"), dtype=torch.float32, device=DEV)
        self.rs[:T] = torch.rsqrt((self.x * self.x).mean(1) + 1e-6)

    def rows(self, idx):
        """The same token rows (bits and rs) as a call of their own."""
        new = object.__new__(Planes)
        T = len(idx)
        new.lo8, new.T, new.Tp, new.D = self.lo8, T, _pad(T + 1), self.D
        new.hi = torch.full((new.Tp, self.D), float("nan"), dtype=torch.bfloat16, device=DEV)
        new.lo = torch.full((new.Tp, self.D), 0xFF if self.lo8 else float("nan"), dtype=self.lo.dtype, device=DEV)
        new.rs = torch.full((new.Tp,), float("nan"), dtype=torch.float32, device=DEV)
        new.hi[:T], new.lo[:T], new.rs[:T], new.x = self.hi[idx], self.lo[idx], self.rs[idx], self.x[idx].contiguous()
        return new


def run_pool(pl, lens, w, chunk=128, fuse=0, out_bf16=0, d_emb=None, p=0.0, seed=0, expect=0):
    """One rp_dbg_pool_head call -> arenas by name.  Guards are checked here."""
    T, D, batch = pl.T, pl.D, len(lens)
    assert T == sum(lens)
    cu = _dev(ek.cu_of(lens))
    ns = ek.n_slots(T, batch, chunk)
    A = {
        "out": hh.Arena("out", batch * D * (2 if out_bf16 else 4), GUARD, DEV, dtype=torch.bfloat16 if out_bf16 else torch.float32),
        "partial": hh.Arena("partial", ns * D * 4, GUARD, DEV, dtype=torch.float32),
        "pwork": hh.Arena("pwork", ns * 16, GUARD, DEV, dtype=torch.int32),
    }
    if d_emb is not None:
        A["ds"] = hh.Arena("ds", batch * D * 4, GUARD, DEV, dtype=torch.float32)
        A["dwf"] = hh.Arena("dwf", batch * D * 4, GUARD, DEV, dtype=torch.float32)
        A["dln"] = hh.Arena("dln", D * 4, GUARD, DEV, dtype=torch.float32)
        A["dxhi"] = hh.Arena("dxhi", pl.Tp * D * 2, GUARD, DEV, dtype=torch.bfloat16)
        A["dxlo"] = hh.Arena("dxlo", pl.Tp * D * 2, GUARD, DEV, dtype=torch.bfloat16)
    g = lambda n: A[n].ptr if n in A else None  # noqa: E731
    st = _lib.load().rp_dbg_pool_head(_lib.ptr(pl.hi), _lib.ptr(pl.lo), 1 if pl.lo8 else 0, _lib.ptr(pl.rs), _lib.ptr(cu), batch, T,
                                      D, _lib.ptr(w), chunk, fuse, out_bf16, _lib.ptr(d_emb), p, seed, g("out"), g("partial"),
                                      g("pwork"), g("ds"), g("dwf"), g("dln"), g("dxhi"), g("dxlo"), _lib.current_stream())
    torch.cuda.synchronize()
    for n, a in A.items():
        assert a.broken_guards() == [], n
    if expect:
        assert st == expect and hh.last_error(), st
        assert all(a.at_rest() for a in A.values()), "a refused call writes nothing"
        return A
    _lib.check(st, "rp_dbg_pool_head")
    return A


@functools.lru_cache(maxsize=None)
def _case(D):
    """The packed call of ek.LENGTHS at width D: fp32 x, w, and d_emb scaled so that the reference's max |dx| is >= 1."""
    x, w, de = ek.pool_inputs(D)
    xd, wd = _dev(x), _dev(w)
    pl = Planes(xd, False)
    cu = ek.cu_of(ek.LENGTHS)
    x64, rs64, w64 = _f64(pl.x), _f64(pl.rs[: pl.T]), w.astype(np.float64)
    _, s = ek.head_reference(x64, rs64, cu, w64)
    ds = np.stack([ek.bwd_seq_reference(s[b], ek.LENGTHS[b], w64, de[b].astype(np.float64))[0] for b in range(len(ek.LENGTHS))])
    dx = ek.bwd_tok_reference(x64, rs64, ds[ek.seq_rows(cu)])
    de = (de * np.float32(2.0 ** np.ceil(np.log2(1.0 / np.abs(dx).max())))).astype(np.float32)  # a power of two: exact
    return dict(D=D, x=xd, w=wd, w64=w64, de=_dev(de), de64=de.astype(np.float64), cu=cu, lens=ek.LENGTHS,
                pl={False: pl, True: Planes(xd, True)})


def _partial_bound(abs_terms, chunk, dropout=False):
    return ek.chain_bound(abs_terms, chunk // 4 + 2 + (1 if dropout else 0))


def _out_bound(ds_bound, s, length, w64):
    """First-order bound of e = m / |m| from a bound on the sums: |de_i| <= (|dm_i| + |e_i| |dm|) / |m| + 16 roundings of the
    finish itself on e_i (the norm's 8-term run + wave and block trees, the square root, the products)."""
    e, m, nrm = ek.finish_reference(s, length, w64)
    dm = np.abs(w64) * ds_bound / length
    return (dm + np.abs(e) * np.sqrt((dm * dm).sum())) / max(nrm, ek.EPS_NORM) + 16 * U * np.abs(e)


def _torch_finish(s32, lens, w):
    m = w * s32 / torch.tensor(lens, dtype=torch.float32, device=DEV)[:, None]
    return m / m.norm(dim=1, keepdim=True).clamp_min(1e-12)


@pytest.mark.parametrize("D", ek.DS)
def test_pool_forward(D):
    """Every chunk / fuse / plane format / output type: pwork, every column sum of every chunk, out from the kernel's own
    partial bits and from the planes; fuse against no fuse, bf16 against torch's cast, two runs: bit for bit."""
    c = _case(D)
    lens, cu, w, w64, batch = c["lens"], c["cu"], c["w"], c["w64"], len(c["lens"])
    lens_t = np.array(lens)
    for lo8 in (False, True):
        pl = c["pl"][lo8]
        x64, rs64 = _f64(pl.x), _f64(pl.rs[: pl.T])
        terms32 = pl.x * pl.rs[: pl.T, None]
        e_ref, s_ref = ek.head_reference(x64, rs64, cu, w64)
        abs_seq = np.stack([np.abs(x64[cu[b] : cu[b + 1]] * rs64[cu[b] : cu[b + 1], None]).sum(0) for b in range(batch)])
        s32 = torch.stack([terms32[cu[b] : cu[b + 1]].sum(0) for b in range(batch)])
        e_yard = _torch_finish(s32, lens, w)
        for chunk in (32, 64, 128):
            tag = f"D={D} lo8={int(lo8)} chunk={chunk}"
            ch = ek.chunks_of(cu, chunk)
            slots, p_ref, p_abs = ek.partial_reference(x64, rs64, cu, chunk)
            p_yard = torch.stack([terms32[a:b].sum(0) for _, _, _, a, b in ch])
            nchunk = (lens_t + chunk - 1) // chunk
            outs = {}
            for fuse in (0, 1):
                for out_bf16 in (0, 1):
                    A = run_pool(pl, lens, w, chunk, fuse, out_bf16)
                    assert np.array_equal(A["pwork"].view(len(A["pwork"].view()) // 4, 4).cpu().numpy(),
                                          ek.pwork_reference(cu, pl.T, chunk)), (tag, "pwork; gap entries are zero length")
                    part = A["partial"].view(ek.n_slots(pl.T, batch, chunk), D)
                    written = np.array([not (fuse and nchunk[b] == 1) for _, b, _, _, _ in ch])
                    rest = np.setdiff1d(np.arange(part.shape[0]), slots[written])
                    assert _untouched(part[_dev(rest)]), (tag, fuse, "gap rows and fused sequences' rows of partial are untouched")
                    got_p = part[_dev(slots[written])]
                    assert _all_written(got_p)
                    if not out_bf16:
                        _fp32(f"partial {tag} fuse={fuse}", got_p, p_ref[written], p_yard[_dev(np.flatnonzero(written))],
                              _partial_bound(p_abs[written], chunk), "pool_forward")
                    out = A["out"].view(batch, D).clone()
                    assert _all_written(out), (tag, "exactly batch rows of out are written")
                    outs[(fuse, out_bf16)] = out
                    if not fuse and not out_bf16:
                        # out from the kernel's own partial bits: the float64 finish of the float64 sum of those rows
                        p64 = _f64(part)
                        s_own = np.stack([p64[cu[b] // chunk + b : cu[b] // chunk + b + nchunk[b]].sum(0) for b in range(batch)])
                        a_own = np.stack([np.abs(p64[cu[b] // chunk + b : cu[b] // chunk + b + nchunk[b]]).sum(0) for b in range(batch)])
                        e_own = np.stack([ek.finish_reference(s_own[b], lens[b], w64)[0] for b in range(batch)])
                        s_own32 = torch.stack([part[cu[b] // chunk + b : cu[b] // chunk + b + nchunk[b]].sum(0) for b in range(batch)])
                        bound = np.stack([_out_bound(nchunk[b] * U * a_own[b], s_own[b], lens[b], w64) for b in range(batch)])
                        _fp32(f"out from partial {tag}", out, e_own, _torch_finish(s_own32, lens, w), bound, "pool_forward")
                        bound = np.stack([_out_bound((chunk // 4 + 2 + nchunk[b]) * U * abs_seq[b], s_ref[b], lens[b], w64)
                                          for b in range(batch)])
                        _fp32(f"out from planes {tag}", out, e_ref, e_yard, bound, "pool_forward")
                        B = run_pool(pl, lens, w, chunk, fuse, out_bf16)
                        assert all(torch.equal(A[k].payload(), B[k].payload()) for k in A), (tag, "two runs")
            assert _same_bits(outs[(1, 0)], outs[(0, 0)]), (tag, "fuse = 1 gives fuse = 0's bits")
            assert _same_bits(outs[(1, 1)], outs[(0, 1)]), (tag, "fuse = 1 gives fuse = 0's bits (bf16)")
            assert _same_bits(outs[(0, 1)], outs[(0, 0)].to(torch.bfloat16)), (tag, "the bf16 out is torch's cast of the fp32 out")


def _gather_rows(cu, order):
    return torch.from_numpy(np.concatenate([np.arange(cu[b], cu[b + 1]) for b in order])).to(DEV)


@pytest.mark.parametrize("D", [128, 1472, 2048])
def test_pool_rows_do_not_depend_on_the_packing(D):
    """A sequence alone, inside the packed call, and inside the packed call in reversed order: the same bits of its out row
    (every chunk size, both formats) and of its tokens' dx rows."""
    c = _case(D)
    lens, cu, w, batch = c["lens"], c["cu"], c["w"], len(c["lens"])
    rev = list(range(batch))[::-1]
    for lo8, chunk, fuse, bwd in ((False, 128, 0, True), (True, 32, 1, False), (True, 64, 1, False), (False, 64, 0, False)):
        pl = c["pl"][lo8]
        de = c["de"] if bwd else None
        A = run_pool(pl, lens, w, chunk, fuse, 0, de)
        R = run_pool(pl.rows(_gather_rows(cu, rev)), [lens[b] for b in rev], w, chunk, fuse, 0, de[rev].contiguous() if bwd else None)
        out, out_r = A["out"].view(batch, D), R["out"].view(batch, D)
        assert _same_bits(out_r, out[rev]), (D, lo8, chunk, "reversed packing")
        if bwd:
            ridx = _gather_rows(cu, rev)
            for n in ("dxhi", "dxlo"):
                assert _same_bits(R[n].view(pl.Tp, D)[: pl.T], A[n].view(pl.Tp, D)[ridx]), (D, n, "reversed packing")
        for b in range(batch):
            rows = torch.arange(cu[b], cu[b + 1], device=DEV)
            S = run_pool(pl.rows(rows), [lens[b]], w, chunk, fuse, 0, de[b : b + 1].contiguous() if bwd else None)
            assert _same_bits(S["out"].view(1, D)[0], out[b]), (D, lo8, chunk, b, "alone")
            if bwd:
                for n in ("dxhi", "dxlo"):
                    assert _same_bits(S[n].view(_pad(lens[b] + 1), D)[: lens[b]], A[n].view(pl.Tp, D)[rows]), (D, n, b, "alone")


def _check_backward(tag, c, pl, lens, A, de, de64, mask=None, zero_seqs=()):
    """ds / dwf / d final_ln from the partial bits as they lie in memory, dx from the kernel's own ds bits, and the whole
    backward from the planes."""
    D, w, w64 = pl.D, c["w"], c["w64"]
    batch, cu = len(lens), ek.cu_of(lens)
    T, Tp = pl.T, pl.Tp
    part = A["partial"].view(ek.n_slots(T, batch, 128), D)
    nchunk = [(n + 127) // 128 for n in lens]
    base = [int(cu[b]) // 128 + b for b in range(batch)]
    p64 = _f64(part)
    s_own = np.stack([p64[base[b] : base[b] + nchunk[b]].sum(0) for b in range(batch)])
    ref = [ek.bwd_seq_reference(s_own[b], lens[b], w64, de64[b]) for b in range(batch)]
    ds_ref, dwf_ref = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    # torch fp32 restatement on the same bits
    s32 = torch.stack([part[base[b] : base[b] + nchunk[b]].sum(0) for b in range(batch)])
    ln = torch.tensor(lens, dtype=torch.float32, device=DEV)[:, None]
    m32 = w * s32 / ln
    nrm = m32.norm(dim=1, keepdim=True)
    e32 = m32 / nrm.clamp_min(1e-12)
    dm32 = torch.where(nrm > 1e-12, (de - e32 * (e32 * de).sum(1, keepdim=True)) / nrm.clamp_min(1e-12), de / 1e-12)
    ds, dwf = A["ds"].view(batch, D), A["dwf"].view(batch, D)
    assert _all_written(ds) and _all_written(dwf)
    live = np.array([b not in zero_seqs for b in range(batch)])
    for rows, kind in ((live, ""), (~live, " (eps branch)")):
        if rows.any():
            r = _dev(np.flatnonzero(rows))
            _fp32(f"ds {tag}{kind}", ds[r], ds_ref[rows], (dm32 * w / ln)[r], None, "pool_backward")
            _fp32(f"dwf {tag}{kind}", dwf[r], dwf_ref[rows], (dm32 * s32 / ln)[r], None, "pool_backward")
    _fp32(f"d final_ln {tag}", A["dln"].view(D), _f64(dwf).sum(0), dwf.sum(0), None, "pool_backward")
    # dx from the kernel's own ds bits
    x64, rs64 = _f64(pl.x), _f64(pl.rs[:T])
    seq = ek.seq_rows(cu)
    m64 = None if mask is None else _f64(mask)
    dx_ref = ek.bwd_tok_reference(x64, rs64, _f64(ds)[seq], m64)
    seq_d = _dev(seq)
    r32 = pl.rs[:T, None]
    dsm32 = ds[seq_d] if mask is None else ds[seq_d] * mask
    dx_yard = r32 * dsm32 - pl.x * r32 ** 3 * ((dsm32 * pl.x).sum(1, keepdim=True) / D)
    hi, lo = A["dxhi"].view(Tp, D), A["dxlo"].view(Tp, D)
    assert _untouched(hi[T:]) and _untouched(lo[T:]), (tag, "rows T .. Tp of dxhi / dxlo are untouched")
    assert _all_written(hi[:T]) and _all_written(lo[:T])
    m = MARGINS.setdefault("pool_backward_planes", {})
    bar = dk.yardstick_bar(dx_ref, _f64(dx_yard))
    found = ek.planes_findings(f"dx from ds {tag}", _f64(hi[:T]), _f64(lo[:T]), dx_ref, bar, m)
    assert not found, found
    # the whole backward from the planes
    _, s_ref = ek.head_reference(x64, rs64, cu, w64, m64)
    ds_whole = np.stack([ek.bwd_seq_reference(s_ref[b], lens[b], w64, de64[b])[0] for b in range(batch)])
    dx_whole = ek.bwd_tok_reference(x64, rs64, ds_whole[seq], m64)
    t32 = pl.x * r32 if mask is None else pl.x * r32 * mask
    s32w = torch.stack([t32[cu[b] : cu[b + 1]].sum(0) for b in range(batch)])
    m32 = w * s32w / ln
    nrm = m32.norm(dim=1, keepdim=True)
    e32 = m32 / nrm.clamp_min(1e-12)
    dm32 = torch.where(nrm > 1e-12, (de - e32 * (e32 * de).sum(1, keepdim=True)) / nrm.clamp_min(1e-12), de / 1e-12)
    dsw = (dm32 * w / ln)[seq_d]
    dsw = dsw if mask is None else dsw * mask
    dxw_yard = r32 * dsw - pl.x * r32 ** 3 * ((dsw * pl.x).sum(1, keepdim=True) / D)
    bar = dk.yardstick_bar(dx_whole, _f64(dxw_yard))
    found = ek.planes_findings(f"dx from planes {tag}", _f64(hi[:T]), _f64(lo[:T]), dx_whole, bar, m)
    assert not found, found
    return float(np.abs(dx_whole).max())


@pytest.mark.parametrize("D", ek.DS)
def test_pool_backward(D):
    c = _case(D)
    pl = c["pl"][False]
    A = run_pool(pl, c["lens"], c["w"], 128, 0, 0, c["de"])
    ref_max = _check_backward(f"D={D}", c, pl, c["lens"], A, c["de"], c["de64"])
    assert ref_max >= 1.0, "d_emb is scaled so that the absolute term of the bar stays small against the reference"
    B = run_pool(pl, c["lens"], c["w"], 128, 0, 0, c["de"])
    assert all(torch.equal(A[k].payload(), B[k].payload()) for k in A), "two runs give the same bits"


@pytest.mark.parametrize("D", [128, 1472, 2048])
def test_pool_head_with_dropout(D):
    """pool_partial_train_kernel and the backward's regenerated mask: the same mask, read back once per (p, seed)."""
    c = _case(D)
    pl, lens, cu, w = c["pl"][False], c["lens"], c["cu"], c["w"]
    x64, rs64 = _f64(pl.x), _f64(pl.rs[: pl.T])
    for p in (0.1, 0.5):
        for seed in (1, 0x9E3779B9):
            tag = f"D={D} p={p} seed={seed}"
            mask = mask_of(p, seed, ek.SITE_FINAL, pl.T, D)
            frac = float((mask == 0).float().mean())
            assert abs(frac - p) < 0.01, (tag, frac)
            A = run_pool(pl, lens, w, 128, 0, 0, c["de"], p, seed)
            slots, p_ref, p_abs = ek.partial_reference(x64, rs64, cu, 128, _f64(mask))
            part = A["partial"].view(ek.n_slots(pl.T, len(lens), 128), D)
            t32 = pl.x * mask * pl.rs[: pl.T, None]
            p_yard = torch.stack([t32[a:b].sum(0) for _, _, _, a, b in ek.chunks_of(cu, 128)])
            assert _untouched(part[_dev(np.setdiff1d(np.arange(part.shape[0]), slots))])
            _fp32(f"partial {tag}", part[_dev(slots)], p_ref, p_yard, _partial_bound(p_abs, 128, True), "pool_dropout")
            e_ref, _ = ek.head_reference(x64, rs64, cu, c["w64"], _f64(mask))
            s32 = torch.stack([t32[cu[b] : cu[b + 1]].sum(0) for b in range(len(lens))])
            _fp32(f"out {tag}", A["out"].view(len(lens), D), e_ref, _torch_finish(s32, lens, w), None, "pool_dropout")
            _check_backward(tag, c, pl, lens, A, c["de"], c["de64"], mask)


def test_pool_head_all_zero_sequences_take_the_eps_branch():
    """Sequences whose planes are all zero (5 and 200 tokens) between two ordinary ones: |m| = 0 <= 1e-12, so e = m / 1e-12 =
    0 exactly, no NaN, and the backward is the clamped branch dm = de / 1e-12."""
    D = 1472
    c = _case(D)
    lens = [7, 5, 200, 33]
    x = c["x"][: sum(lens)].clone()
    x[7 : 7 + 205] = 0.0
    for lo8 in (False, True):
        pl = Planes(x, lo8)
        assert not bool(pl.x[7:212].any())
        for chunk, fuse in ((128, 0), (64, 1), (32, 1)):
            A = run_pool(pl, lens, c["w"], chunk, fuse, 0)
            out = A["out"].view(4, D)
            assert bool((out[1:3] == 0).all()), "exactly zero rows"
            assert bool(torch.isfinite(out).all())
            assert torch.allclose(out[[0, 3]].norm(dim=1), torch.ones(2, device=DEV), atol=1e-5)
    pl = Planes(x, False)
    de, de64 = c["de"][:4].contiguous(), c["de64"][:4]
    A = run_pool(pl, lens, c["w"], 128, 0, 0, de)
    assert bool((A["out"].view(4, D)[1:3] == 0).all())
    assert bool((A["dwf"].view(4, D)[1:3] == 0).all()), "dwf = dm s / len with s = 0"
    _check_backward("zero sequences", c, pl, lens, A, de, de64, None, zero_seqs=(1, 2))


def test_pool_head_refuses_what_it_cannot_run():
    """An empty sequence is outside the pooling head's contract (reprover_hip.h) and refused; so are dropout or a backward in
    an inference form, a width past 2048 and a chunk that is none of 32 / 64 / 128.  Nothing is written."""
    c = _case(128)
    pl, w = c["pl"][False], c["w"]
    small = pl.rows(torch.arange(12, device=DEV))
    run_pool(small, [5, 0, 7], w, expect=RP_E_INVALID)
    run_pool(small, [12], w, chunk=48, expect=RP_E_INVALID)
    run_pool(small, [12], w, chunk=64, p=0.1, expect=RP_E_INVALID)
    run_pool(small, [12], w, chunk=128, fuse=1, d_emb=c["de"][:1].contiguous(), expect=RP_E_INVALID)
    run_pool(c["pl"][True].rows(torch.arange(12, device=DEV)), [12], w, d_emb=c["de"][:1].contiguous(), expect=RP_E_INVALID)


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
def rows_call(mode, a=None, b=None, ia=None, T=0, rows=0, n=0, vocab=0, np_=0, ld=0, inv_d=0.0, p=0.0, seed=0, site=0, o0=None,
              o1=None, o2=None, expect=0):
    ptr = lambda x: None if x is None else (x.ptr if isinstance(x, hh.Arena) else _lib.ptr(x))  # noqa: E731
    st = _lib.load().rp_dbg_train_rows(mode, ptr(a), ptr(b), ptr(ia), T, rows, n, vocab, np_, ld, inv_d, p, seed, site, ptr(o0),
                                       ptr(o1), ptr(o2), _lib.current_stream())
    torch.cuda.synchronize()
    if expect:
        assert st == expect and hh.last_error()
        assert all(o.at_rest() and o.broken_guards() == [] for o in (o0, o1, o2) if isinstance(o, hh.Arena))
        return
    _lib.check(st, f"rp_dbg_train_rows({mode})")


@pytest.mark.parametrize("D", [128, 1472, 2048])
def test_embed_forward_kernels(D):
    """embed_kernel<false> and embed_train_kernel: the planes bit for bit against split_planes(mask * table[clip(id)]) (one fp32
    multiply), slot 0 of ssp against float64 of the stored values, the other slots exactly zero, rows T .. Tp = token 0's row."""
    V = 384
    table = _dev((np.random.default_rng(D).standard_normal((V, D)) * 2.0).astype(np.float32))
    for T, np_ in ((1, 1), (3, 2), (4, 65), (5, 1), (255, 2), (257, 65)):
        Tp = 256 if T <= 256 else 512
        ids = ek.embed_ids(T, V)
        assert (ids >= V).any() and (T <= 2 or (ids < 0).any())
        idd = _dev(ids)
        idc = torch.cat([idd.long().clamp(0, V - 1), torch.zeros(Tp - T, dtype=torch.long, device=DEV)])
        for mode, p, seed in ((0, 0.0, 0), (1, 0.1, 5), (1, 0.5, 77)):
            tag = f"embed D={D} T={T} np={np_} mode={mode} p={p}"
            want = table[idc]
            if mode:
                want = want * mask_of(p, seed, ek.SITE_EMBED, Tp, D)
            planes = hh.split_planes(want + 0.0)  # the kernel adds the value to a zero stream: a dropped -x is +0, not -0
            A = [hh.Arena("xhi", Tp * D * 2, GUARD, DEV, dtype=torch.bfloat16), hh.Arena("xlo", Tp * D * 2, GUARD, DEV, dtype=torch.bfloat16),
                 hh.Arena("ssp", np_ * Tp * 4, GUARD, DEV, dtype=torch.float32)]
            rows_call(mode, table, ia=idd, T=T, rows=Tp, n=D, vocab=V, np_=np_, p=p, seed=seed, o0=A[0], o1=A[1], o2=A[2])
            assert all(a.broken_guards() == [] for a in A), tag
            assert _same_bits(A[0].view(Tp, D), planes[0]) and _same_bits(A[1].view(Tp, D), planes[1]), tag
            ssp = A[2].view(np_, Tp)
            assert not bool(ssp[1:].view(torch.int32).any()), (tag, "slots 1 .. np - 1 are exactly zero")
            stored = hh.merge_planes(planes)
            _fp32(f"ssp {tag}", ssp[0], (_f64(stored) ** 2).sum(1), (stored * stored).sum(1), None, "rows")
    out = hh.Arena("xhi", 256 * D * 2, GUARD, DEV, dtype=torch.bfloat16)
    rows_call(1, table, ia=idd, T=4, rows=256, n=D, vocab=V, np_=1, p=0.0, o0=out, o1=out, o2=out, expect=RP_E_INVALID)
    rows_call(0, table, ia=idd, T=300, rows=256, n=D, vocab=V, np_=1, o0=out, o1=out, o2=out, expect=RP_E_INVALID)


@pytest.mark.parametrize("D", [128, 1472])
def test_mask_dx(D):
    """Bit for bit against ((hi + lo) * m) in torch fp32 cast to bf16."""
    for rows in (1, 4, 5, 256):
        planes = hh.split_planes(_dev((np.random.default_rng(rows + D).standard_normal((rows, D)) * 3.0).astype(np.float32)))
        for site in (ek.SITE_LAYER0 + 3, ek.SITE_LAYER0 + 8 * 5 + 1):
            for seed in (3, 0xDEADBEEF):
                m = mask_of(0.1, seed, site, rows, D)
                out = hh.Arena("dxm", rows * D * 2, GUARD, DEV, dtype=torch.bfloat16)
                rows_call(2, planes[0], planes[1], rows=rows, n=D, p=0.1, seed=seed, site=site, o0=out)
                assert out.broken_guards() == []
                assert _same_bits(out.view(rows, D), (hh.merge_planes(planes) * m).to(torch.bfloat16)), (D, rows, site, seed)


@pytest.mark.parametrize("width", [384, 1152, 3072])
def test_qkv_scale_dot(width):
    rows = 256
    for T in (1, 5, 130):
        rng = np.random.default_rng(width + T)
        d = _dev(rng.standard_normal((rows, width)).astype(np.float32)).to(torch.bfloat16)
        y = _dev(rng.standard_normal((rows, width)).astype(np.float32)).to(torch.bfloat16)
        d[T:], y[T:] = float("nan"), float("nan")
        rs = torch.full((rows,), float("nan"), device=DEV)
        rs[:T] = _dev(rng.uniform(0.3, 3.0, T).astype(np.float32))
        inv_d = float(np.float32(1.0 / 1472))
        a_d = hh.Arena.of("dqkv", d, GUARD)
        a_r = hh.Arena("rcoef", rows * 4, GUARD, DEV, dtype=torch.float32)
        rows_call(3, y, rs, T=T, rows=rows, n=width, inv_d=inv_d, o0=a_d, o1=a_r)
        assert a_d.broken_guards() == [] and a_r.broken_guards() == []
        got, rc = a_d.view(rows, width), a_r.view(rows)
        assert _same_bits(got[:T], (d[:T].float() * rs[:T, None]).to(torch.bfloat16)), (width, T)
        assert not bool(got[T:].view(torch.int16).any()) and not bool(rc[T:].view(torch.int32).any()), "rows T .. rows are zero"
        r64 = _f64(rs[:T])
        ref = r64 * r64 * (_f64(d[:T]) * _f64(y[:T])).sum(1) * inv_d
        yard = rs[:T] * rs[:T] * (d[:T].float() * y[:T].float()).sum(1) * inv_d
        # a lane's run of 8 fused multiply-adds per 512 columns, the wave's 6-step tree, three products
        chain = 8 * ((width // 8 + 63) // 64) + 6 + 3
        bound = chain * U * (r64 * r64 * np.abs(_f64(d[:T]) * _f64(y[:T])).sum(1) * inv_d)
        _fp32(f"rcoef qkv width={width} T={T}", rc[:T], ref, yard, bound, "rows")


@pytest.mark.parametrize("np_", [1, 31, 32, 33, 56, 64, 65])
def test_rowdot_finish(np_):
    for rows in (1, 63, 64, 65, 130):
        ld = rows + 62
        rng = np.random.default_rng(np_ * 1000 + rows)
        rdp = _dev(rng.standard_normal((np_, ld)).astype(np.float32))
        rs = torch.full((ld,), float("nan"), device=DEV)
        rs[:rows] = _dev(rng.uniform(0.3, 3.0, rows).astype(np.float32))
        inv_d = float(np.float32(1.0 / 1472))
        out = hh.Arena("rcoef", ld * 4, GUARD, DEV, dtype=torch.float32)
        rows_call(4, rdp, rs, rows=rows, n=8, np_=np_, ld=ld, inv_d=inv_d, o0=out)
        got = out.view(ld)
        assert out.broken_guards() == [] and _untouched(got[rows:]), "entries past rows are untouched"
        r64 = _f64(rs[:rows])
        ref = r64 * r64 * _f64(rdp[:, :rows]).sum(0) * inv_d
        yard = rs[:rows] * rs[:rows] * rdp[:, :rows].sum(0) * inv_d
        bound = (np_ + 3) * U * (r64 * r64 * np.abs(_f64(rdp[:, :rows])).sum(0) * inv_d)  # the slots in index order: one chain
        _fp32(f"rcoef rowdot np={np_} rows={rows}", got[:rows], ref, yard, bound, "rows")
    out.reset()
    rows_call(4, rdp, rs, rows=rows, n=8, np_=np_, ld=rows - 1, inv_d=inv_d, o0=out, expect=RP_E_INVALID)


@pytest.mark.parametrize("D", [128, 1472])
def test_embed_backward(D):
    """The scatter agrees with the forward's gather on every id: -5 lands in row 0 and V + 7 in row V - 1 (the forward reads
    those rows); rows of ids that never occur are exactly zero; with and without the embedding site's dropout."""
    V = 384
    for T in (1, 255, 256, 257, 600):
        ids, dx = dk.embed_inputs(T, V, D)
        planes = hh.split_planes(_dev(dx))
        g = hh.merge_planes(planes)
        idd = _dev(ids)
        for p, seed in ((0.0, 0), (0.1, 9)):
            tag = f"embed_bwd D={D} T={T} p={p}"
            gm = g if p == 0 else g * mask_of(p, seed, ek.SITE_EMBED, T, D)
            want = ek.embed_bwd_reference(ids, _f64(gm), V)
            yard = torch.zeros(V, D, device=DEV).index_add_(0, idd.long().clamp(0, V - 1), gm)
            tab = hh.Arena("dtable", V * D * 4, GUARD, DEV, dtype=torch.float32)
            rows_call(5, planes[0], planes[1], ia=idd, T=T, rows=T, n=D, vocab=V, p=p, seed=seed, o0=tab)
            got = tab.view(V, D).clone()
            assert tab.broken_guards() == [] and _all_written(got)
            never = np.setdiff1d(np.arange(V), np.clip(ids, 0, V - 1))
            assert len(never) > 300 and {33, 34, V - 2} <= set(never.tolist())
            assert not bool(got[_dev(never)].view(torch.int32).any()), (tag, "rows of ids that never occur are exactly zero")
            if T > 2:  # token T // 2 holds id -5: the forward read table row 0 for it
                neg = np.flatnonzero(ids < 0)
                only_neg = ek.embed_bwd_reference(ids[neg], _f64(gm)[neg], V)[0]
                assert np.abs(only_neg).max() > 0 and np.abs(_f64(got[0]) - want[0]).max() < 1e-3 * np.abs(only_neg).max(), \
                    (tag, "the negative id's gradient lands in row 0")
            chain = np.bincount(np.clip(ids, 0, V - 1), minlength=V).max()
            bound = np.zeros((V, D))
            np.add.at(bound, np.clip(ids, 0, V - 1), np.abs(_f64(gm)))
            _fp32(tag, got, want, yard, chain * U * bound, "rows")
            tab.reset()
            rows_call(5, planes[0], planes[1], ia=idd, T=T, rows=T, n=D, vocab=V, p=p, seed=seed, o0=tab)
            assert _same_bits(tab.view(V, D), got), (tag, "bit-reproducible")


# ---------------------------------------------------------------------------------------------------------------------------
# weight pack / unpack
# ---------------------------------------------------------------------------------------------------------------------------
def _repack_specs(D):
    """The four matrices of one launch: (mode, rows, cols, n, number of sources, rows per source)."""
    return [(ek.PACK_CONCAT3, 3 * 128, D, 128, 3, 128), (ek.PACK_GEGLU, 2 * 64, D, 0, 2, 64), (ek.PACK_COPY, D, 128, 0, 1, D),
            (ek.PACK_CONCAT3, 3 * 384, D, 384, 3, 384), (ek.PACK_GEGLU, 2 * 192, D, 0, 2, 192), (ek.PACK_COPY, D, 192, 0, 1, D)]


def run_repack(specs, sources, colscales):
    mats = (_lib.RpDbgRepackMat * len(specs))()
    A = []
    for k, ((mode, rows, cols, n, nsrc, _), src, cs) in enumerate(zip(specs, sources, colscales)):
        dst = hh.Arena(f"dst{k}", rows * cols * 2, GUARD, DEV, dtype=torch.bfloat16)
        dst_t = hh.Arena(f"dst_t{k}", rows * cols * 2, GUARD, DEV, dtype=torch.bfloat16)
        A.append((dst, dst_t))
        s = [_lib.ptr(t) for t in src] + [None] * (3 - nsrc)
        mats[k] = _lib.RpDbgRepackMat(s[0], s[1], s[2], _lib.ptr(cs), dst.ptr, dst_t.ptr, rows, cols, n, mode)
    _lib.check(_lib.load().rp_dbg_repack(ctypes.addressof(mats), len(specs), _lib.current_stream()), "rp_dbg_repack")
    torch.cuda.synchronize()
    out = []
    for (mode, rows, cols, *_), (dst, dst_t) in zip(specs, A):
        assert dst.broken_guards() == [] and dst_t.broken_guards() == [], "nothing is written outside the matrices"
        out.append((dst.view(rows, cols).clone(), dst_t.view(cols, rows).clone()))
    return out


@pytest.mark.parametrize("D", [128, 192])
def test_repack_layer(D):
    """Distinct small integers times a power-of-two column scale (exact in bf16): dst against the host permutation, dst_t against
    dst's transpose; then random masters: dst = torch's cast of master * colscale (one fp32 multiply)."""
    for specs in (_repack_specs(D)[:3] + _repack_specs(D)[5:], _repack_specs(D)[3:5] + _repack_specs(D)[2:3] + _repack_specs(D)[:1]):
        for kind in ("integers", "random"):
            rng = np.random.default_rng(D + len(kind))
            sources, scales, want = [], [], []
            for k, (mode, rows, cols, n, nsrc, per) in enumerate(specs):
                if kind == "integers":  # 1 .. 255 by (source, row, column): no two rows of a matrix alike, exact in bf16
                    rr, cc = np.arange(per)[:, None], np.arange(cols)[None]
                    src = [((rr * 37 + cc * 11 + j * 101 + k * 53) % 255 + 1).astype(np.float32) for j in range(nsrc)]
                    cs = (2.0 ** rng.integers(-3, 4, cols)).astype(np.float32) if mode != ek.PACK_COPY else None
                else:
                    src = [rng.standard_normal((per, cols)).astype(np.float32) for _ in range(nsrc)]
                    cs = (1.0 + 0.2 * rng.standard_normal(cols)).astype(np.float32) if mode != ek.PACK_COPY else None
                packed = torch.from_numpy(ek.repack_reference(mode, src, rows, n)).to(DEV)
                if cs is not None:
                    packed = packed * _dev(cs)
                want.append(packed.to(torch.bfloat16))
                if kind == "integers":
                    assert torch.equal(want[-1].float(), packed), "exact in bf16"
                sources.append([_dev(s) for s in src])
                scales.append(None if cs is None else _dev(cs))
            got = run_repack(specs, sources, scales)
            for k, ((dst, dst_t), w) in enumerate(zip(got, want)):
                assert _same_bits(dst, w), (D, kind, k, "dst")
                assert _same_bits(dst_t, w.t().contiguous()), (D, kind, k, "dst_t is dst's transpose")
    one = hh.Arena("dst", 64 * 64 * 2, GUARD, DEV, dtype=torch.bfloat16)
    src = torch.zeros(64, 64, device=DEV)
    for rows, cols, mode, n in ((64, 96, ek.PACK_COPY, 0), (96, 64, ek.PACK_COPY, 0), (64, 64, 3, 0), (64, 64, ek.PACK_CONCAT3, 64)):
        mats = (_lib.RpDbgRepackMat * 1)(_lib.RpDbgRepackMat(_lib.ptr(src), _lib.ptr(src), _lib.ptr(src), None, one.ptr, one.ptr, rows, cols, n, mode))
        assert _lib.load().rp_dbg_repack(ctypes.addressof(mats), 1, _lib.current_stream()) == RP_E_INVALID
    torch.cuda.synchronize()
    assert one.at_rest() and one.broken_guards() == []


def run_unfold(part, mode, n, masters=None, ln=None, expect=0):
    """part fp32 device [splits, rows, C] -> (g list, d ln or None) as device tensors."""
    S, rows, C = part.shape
    nsrc = {ek.UNFOLD_PLAIN: 1, ek.UNFOLD_QKV: 3, ek.UNFOLD_GEGLU: 2}[mode]
    per = rows if mode == ek.UNFOLD_PLAIN else (n if mode == ek.UNFOLD_QKV else rows // 2)
    G = [hh.Arena(f"g{k}", per * C * 4, GUARD, DEV, dtype=torch.float32) for k in range(nsrc)]
    nblk = (rows + 31) // 32
    dpart = hh.Arena("dln_part", nblk * C * 4, GUARD, DEV, dtype=torch.float32)
    dln = hh.Arena("dln", C * 4, GUARD, DEV, dtype=torch.float32)
    gp = [g.ptr for g in G] + [None] * (3 - nsrc)
    wp = [_lib.ptr(m) for m in (masters or [])] + [None] * (3 - len(masters or []))
    plain = mode == ek.UNFOLD_PLAIN
    st = _lib.load().rp_dbg_unfold(_lib.ptr(part), rows * C, S, rows, C, mode, n, gp[0], gp[1], gp[2], wp[0], wp[1], wp[2],
                                   _lib.ptr(ln), None if plain else dpart.ptr, None if plain else dln.ptr, _lib.current_stream())
    torch.cuda.synchronize()
    for a in G + [dpart, dln]:
        assert a.broken_guards() == [], a.name
    if expect:
        assert st == expect and all(a.at_rest() for a in G + [dpart, dln])
        return None, None
    _lib.check(st, "rp_dbg_unfold")
    assert all(_all_written(g.view(per, C)) for g in G)
    return [g.view(per, C).clone() for g in G], (None if plain else dln.view(C).clone())


UNFOLD_ROWS = {ek.UNFOLD_PLAIN: ((32, 0), (40, 0), (392, 0)), ek.UNFOLD_QKV: ((24, 8), (39, 13), (393, 131)),
               ek.UNFOLD_GEGLU: ((64, 0), (128, 0), (448, 0))}  # (rows, n): QKV rows = 3 n, GEGLU rows % 64 == 0 - the kernel's layout rule


@pytest.mark.parametrize("mode", [ek.UNFOLD_PLAIN, ek.UNFOLD_QKV, ek.UNFOLD_GEGLU])
def test_unfold(mode):
    """Integer partials: g0 / g1 / g2 and d ln exact; random partials against float64."""
    for rows, n in UNFOLD_ROWS[mode]:
        for C in (128, 200, 260):
            for S in (1, 2, 5):
                rng = np.random.default_rng(rows * 7 + C + S)
                nsrc = {ek.UNFOLD_PLAIN: 0, ek.UNFOLD_QKV: 3, ek.UNFOLD_GEGLU: 2}[mode]
                per = n if mode == ek.UNFOLD_QKV else rows // 2
                for kind in ("integers", "random"):
                    tag = f"unfold mode={mode} rows={rows} C={C} S={S} {kind}"
                    if kind == "integers":
                        part = rng.integers(-8, 9, (S, rows, C)).astype(np.float32)
                        masters = [rng.integers(-4, 5, (per, C)).astype(np.float32) for _ in range(nsrc)]
                        ln = (2.0 ** rng.integers(-2, 3, C)).astype(np.float32)
                    else:
                        part = rng.standard_normal((S, rows, C)).astype(np.float32)
                        masters = [rng.standard_normal((per, C)).astype(np.float32) for _ in range(nsrc)]
                        ln = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
                    g_ref, dln_ref = ek.unfold_reference(part.astype(np.float64), mode, n, [m.astype(np.float64) for m in masters],
                                                         ln.astype(np.float64))
                    pd, md, lnd = _dev(part), [_dev(m) for m in masters], _dev(ln)
                    g, dln = run_unfold(pd, mode, n, md, lnd if nsrc else None)
                    # torch fp32 restatement: the same sums in torch's order
                    s32 = pd.sum(0)
                    pm = ek.PACK_COPY if mode == ek.UNFOLD_PLAIN else (ek.PACK_CONCAT3 if mode == ek.UNFOLD_QKV else ek.PACK_GEGLU)
                    which, sr = ek.pack_row_map(pm, rows, n)
                    for k in range(max(nsrc, 1)):
                        sel = _dev(np.flatnonzero(which == k))
                        order = _dev(np.argsort(sr[which == k]))
                        y = s32[sel][order] * (lnd if nsrc else 1.0)
                        if kind == "integers":
                            assert np.array_equal(_f64(g[k]), g_ref[k]), (tag, k)
                        else:
                            _fp32(f"{tag} g{k}", g[k], g_ref[k], y, None, "unfold")
                    if nsrc:
                        wfull = torch.stack([md[k][i] for k, i in zip(which, sr)])
                        if kind == "integers":
                            assert np.array_equal(_f64(dln), dln_ref), tag
                        else:
                            bound = (S + 8 + (rows + 31) // 32) * U * (np.abs(part.astype(np.float64)).sum(0) * np.abs(_f64(wfull))).sum(0)
                            _fp32(f"{tag} d ln", dln, dln_ref, (s32 * wfull).sum(0), bound, "unfold")
    part = torch.zeros(1, 64, 128, device=DEV)
    run_unfold(part[:, :, :126].contiguous(), ek.UNFOLD_PLAIN, 0, expect=RP_E_INVALID)
    run_unfold(part, ek.UNFOLD_QKV, 20, [part[0]] * 3, part[0, 0], expect=RP_E_INVALID)
    run_unfold(part[:, :40].contiguous(), ek.UNFOLD_GEGLU, 0, [part[0]] * 2, part[0, 0], expect=RP_E_INVALID)


@pytest.mark.parametrize("mode", [ek.UNFOLD_QKV, ek.UNFOLD_GEGLU])
def test_unfold_of_repacked_weights_is_the_round_trip(mode):
    """The row maps of repack_layer_kernel and unfold_kernel as one property: unfolding the packed form (colscale = ln, one
    split, partial = the packed matrix as fp32) gives back bf16(master) * ln^2 bit for bit (ln: powers of two)."""
    D = 192
    rng = np.random.default_rng(mode)
    n = 128 if mode == ek.UNFOLD_QKV else 0
    nsrc, per = (3, 128) if mode == ek.UNFOLD_QKV else (2, 192)
    rows = nsrc * per
    masters = [_dev(rng.integers(-100, 101, (per, D)).astype(np.float32) + 1000.0 * k) for k in range(nsrc)]
    ln = _dev((2.0 ** rng.integers(-2, 3, D)).astype(np.float32))
    spec = (ek.PACK_CONCAT3 if mode == ek.UNFOLD_QKV else ek.PACK_GEGLU, rows, D, n, nsrc, per)
    (dst, _), = run_repack([spec], [masters], [ln])
    g, _ = run_unfold(dst.float().unsqueeze(0).contiguous(), mode, n, masters, ln)
    for k in range(nsrc):
        want = masters[k].to(torch.bfloat16).float() * ln * ln
        assert _same_bits(g[k], want), (mode, k)
        assert k == 0 or not torch.equal(g[k], g[0])


@pytest.mark.parametrize("ntab,H", [(33, 1), (33, 6), (257, 1), (257, 6)])
def test_bias_table(ntab, H):
    """T5's bucket map at both table sizes: bit for bit against host indexing."""
    maxd = (ntab - 1) // 2
    buckets = 32
    bucket_of = t5_ref.relative_position_bucket(np.arange(ntab) - maxd, buckets, maxd).astype(np.int32)
    assert bucket_of.min() >= 0 and bucket_of.max() < buckets and len(set(bucket_of.tolist())) > 8
    rel = np.random.default_rng(ntab + H).standard_normal((buckets, H)).astype(np.float32)
    out = hh.Arena("tab", H * ntab * 4, GUARD, DEV, dtype=torch.float32)
    rel_d, bucket_d = _dev(rel), _dev(bucket_of)
    st = _lib.load().rp_dbg_bias_table(_lib.ptr(rel_d), _lib.ptr(bucket_d), H, ntab, out.ptr, _lib.current_stream())
    _lib.check(st, "rp_dbg_bias_table")
    torch.cuda.synchronize()
    assert out.broken_guards() == []
    assert np.array_equal(out.view(H, ntab).cpu().numpy(), ek.bias_table_reference(rel, bucket_of))
