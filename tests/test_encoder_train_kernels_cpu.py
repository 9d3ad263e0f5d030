"""The references of tests/test_encoder_train_kernels_gpu.py pinned without a GPU, and that its bars mean something.

1. The float64 restatements of tests/encoder_kernel_helpers.py against torch float64 autograd on the GPU tests' shapes: the
   pooling head forward and backward (eps branch and dropout mask included), the embedding scatter, the unfold / repack
   permutations with the folded norm weight.
2. With a float64 stand-in that rounds to fp32 where the kernels round (per-wave fused multiply-add runs, the four-wave tree,
   the chunk sums in order) in the kernel's place, every planted bug misses a bar the GPU test applies, and the unmutated
   stand-in meets every one of them.  The bars are computed as the GPU test computes them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_kernel_helpers as dk  # noqa: E402
import encoder_kernel_helpers as ek  # noqa: E402

U = ek.U32


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the references against torch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [False, True])
def test_pool_head_reference_is_autograd(dropout):
    """Forward and backward of the whole head, with an all-zero sequence (F.normalize's eps branch) among the others."""
    rng = np.random.default_rng(3)
    D, lens = 64, [1, 5, 4, 130, 33]
    cu = ek.cu_of(lens)
    T = int(cu[-1])
    x = rng.standard_normal((T, D)) * 2.0
    x[cu[2] : cu[3]] = 0.0
    w = 1.0 + 0.2 * rng.standard_normal(D)
    de = rng.standard_normal((len(lens), D))
    mask = (rng.random((T, D)) >= 0.3) / 0.7 if dropout else None
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    rs_t = torch.rsqrt((xt * xt).mean(1, keepdim=True) + 1e-6)
    y = xt * rs_t * wt  # the final RMSNorm, then HF's dropout, then the masked mean and F.normalize
    if dropout:
        y = y * torch.from_numpy(mask)
    e = torch.stack([torch.nn.functional.normalize(y[cu[b] : cu[b + 1]].mean(0), dim=0, eps=1e-12) for b in range(len(lens))])
    (e * torch.from_numpy(de)).sum().backward()
    rs = rs_t.detach().numpy()[:, 0]
    e_ref, s = ek.head_reference(x, rs, cu, w, mask)
    assert np.abs(e_ref - e.detach().numpy()).max() < 1e-13
    assert not e_ref[2].any() and np.allclose(np.linalg.norm(e_ref[[0, 1, 3, 4]], axis=1), 1.0)
    ref = [ek.bwd_seq_reference(s[b], lens[b], w, de[b]) for b in range(len(lens))]
    ds = np.stack([r[0] for r in ref])
    dx = ek.bwd_tok_reference(x, rs, ds[ek.seq_rows(cu)], mask)
    live = np.ones(T, bool)
    live[cu[2] : cu[3]] = False
    gx = xt.grad.numpy()
    assert np.abs(dx[live] - gx[live]).max() <= 1e-12 * np.abs(gx).max()
    # the clamped branch: dm = de / 1e-12 and no norm term (x = 0: rs = 1e3, the second term of dx vanishes)
    assert np.allclose(dx[~live], gx[~live], rtol=1e-12, atol=0) and np.abs(gx[~live]).max() > 1e9
    assert np.abs(sum(r[1] for r in ref) - wt.grad.numpy()).max() <= 1e-12 * np.abs(wt.grad.numpy()).max()


def test_partial_and_pwork_layout():
    """Chunk c of sequence b sits at slot cu[b] / chunk + b + c: strictly increasing, inside T / chunk + batch."""
    cu = ek.cu_of(ek.LENGTHS)
    T = int(cu[-1])
    for chunk in (32, 64, 128):
        slots = [c[0] for c in ek.chunks_of(cu, chunk)]
        assert slots == sorted(set(slots)) and slots[-1] < ek.n_slots(T, len(ek.LENGTHS), chunk)
        pw = ek.pwork_reference(cu, T, chunk)
        assert (pw[slots, 1] > 0).all() and pw[:, 1].astype(bool).sum() == len(slots)
        assert sum(min(chunk, ln - c * chunk) for _, ln, c, _ in pw[slots]) == T


def test_embed_scatter_reference_is_autograd():
    V, D = 384, 24
    for T in (1, 255, 600):
        ids, dx = ek.embed_inputs(T, V, D)
        table = torch.zeros(V, D, dtype=torch.float64, requires_grad=True)
        x = table[torch.from_numpy(np.clip(ids, 0, V - 1)).long()]  # the forward's gather clamps every id
        (x * torch.from_numpy(dx.astype(np.float64))).sum().backward()
        assert np.array_equal(ek.embed_bwd_reference(ids, dx.astype(np.float64), V), table.grad.numpy()) or \
            np.abs(ek.embed_bwd_reference(ids, dx.astype(np.float64), V) - table.grad.numpy()).max() < 1e-12


@pytest.mark.parametrize("mode", [ek.UNFOLD_QKV, ek.UNFOLD_GEGLU])
def test_unfold_and_repack_references_are_autograd(mode):
    """W' = pack(masters) * ln as torch builds it; for a gradient G of W', autograd's d master and d ln are unfold's."""
    rng = np.random.default_rng(mode)
    C = 20
    n, nsrc, per = (13, 3, 13) if mode == ek.UNFOLD_QKV else (0, 2, 64)
    rows = nsrc * per
    masters = [torch.from_numpy(rng.standard_normal((per, C))).requires_grad_(True) for _ in range(nsrc)]
    ln = torch.from_numpy(1.0 + 0.2 * rng.standard_normal(C)).requires_grad_(True)
    if mode == ek.UNFOLD_QKV:
        packed = torch.cat(masters)
    else:  # 32 rows of wi_0, the same 32 of wi_1
        packed = torch.stack([masters[0].view(per // 32, 32, C), masters[1].view(per // 32, 32, C)], 1).reshape(rows, C)
    pm = ek.PACK_CONCAT3 if mode == ek.UNFOLD_QKV else ek.PACK_GEGLU
    assert np.array_equal(ek.repack_reference(pm, [m.detach().numpy() for m in masters], rows, n), packed.detach().numpy())
    part = rng.standard_normal((3, rows, C))
    ((packed * ln) * torch.from_numpy(part.sum(0))).sum().backward()
    g, dln = ek.unfold_reference(part, mode, n, [m.detach().numpy() for m in masters], ln.detach().numpy())
    for k in range(nsrc):
        assert np.abs(g[k] - masters[k].grad.numpy()).max() < 1e-12
    assert np.abs(dln - ln.grad.numpy()).max() < 1e-12


def test_bias_table_reference():
    rel = np.arange(12.0).reshape(4, 3)
    tab = ek.bias_table_reference(rel, [3, 0, 0, 2])
    assert tab.shape == (3, 4) and np.array_equal(tab[1], [10.0, 1.0, 1.0, 7.0])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. planted bugs against the GPU tests' bars
# ---------------------------------------------------------------------------------------------------------------------------
def _bf16(a):
    return dk.bf16_round(a)


@functools.lru_cache(maxsize=None)
def _case(D):
    """The GPU test's packed call at width D as float64 arrays holding the values the kernel is handed."""
    x, w, de = ek.pool_inputs(D)
    hi = _bf16(x)
    xs = (hi + _bf16(x.astype(np.float64) - hi)).astype(np.float32)  # the two planes, decoded
    rs = (1.0 / np.sqrt((xs.astype(np.float64) ** 2).mean(1) + 1e-6)).astype(np.float32)
    cu = ek.cu_of(ek.LENGTHS)
    mask = ((np.random.default_rng(D).random(xs.shape) >= 0.1) * np.float32(1.0 / 0.9)).astype(np.float64)
    return dict(x=xs.astype(np.float64), x32=torch.from_numpy(xs), rs=rs.astype(np.float64), rs32=torch.from_numpy(rs), cu=cu,
                w=w.astype(np.float64), w32=torch.from_numpy(w), de=de.astype(np.float64), de32=torch.from_numpy(de), mask=mask)


def _partial_findings(c, chunk, mask, mutant):
    m64 = c["mask"] if mask else None
    got = ek.standin_partial(c["x"], c["rs"], c["cu"], chunk, m64, mutant)
    _, ref, abs_terms = ek.partial_reference(c["x"], c["rs"], c["cu"], chunk, m64)
    t32 = c["x32"] * c["rs32"][:, None] if not mask else c["x32"] * torch.from_numpy(c["mask"]).float() * c["rs32"][:, None]
    yard = torch.stack([t32[a:b].sum(0) for _, _, _, a, b in ek.chunks_of(c["cu"], chunk)]).numpy()
    return ek.fp32_findings("partial", got, ref, yard, ek.chain_bound(abs_terms, chunk // 4 + 2 + (1 if mask else 0)))


@pytest.mark.parametrize("D", [128, 1472])
def test_partial_bars_separate_planted_bugs(D):
    c = _case(D)
    for chunk in (32, 64, 128):
        assert not _partial_findings(c, chunk, False, None), "the clean stand-in meets the bar"
        assert _partial_findings(c, chunk, False, "drop_last_odd"), "the last token of an odd-length chunk dropped"
        assert _partial_findings(c, chunk, False, "clamped_piece"), "a clamped piece accumulated into columns D - 8 .."
    assert not _partial_findings(c, 128, True, None)
    assert _partial_findings(c, 128, True, "mask_next_row"), "the dropout mask of row t + 1"


def _seq_findings(c, mutant):
    """ds per sequence from the stand-in's own chunk sums, under the fp32 bar."""
    lens, cu, w, de = ek.LENGTHS, c["cu"], c["w"], c["de"]
    partial = ek.standin_partial(c["x"], c["rs"], cu, 128)
    s = ek.standin_seq_sums(partial, cu, 128)
    i, s_exact = 0, []
    for b, ln in enumerate(lens):
        n = (ln + 127) // 128
        s_exact.append(partial[i : i + n].sum(0))
        i += n
    ref = np.stack([ek.bwd_seq_reference(s_exact[b], lens[b], w, de[b])[0] for b in range(len(lens))])
    got = ek._f32(np.stack([ek.bwd_seq_reference(s[b], lens[b], w, de[b], mutant)[0] for b in range(len(lens))]))
    s32 = torch.from_numpy(np.stack(s_exact)).float()
    ln32 = torch.tensor(lens, dtype=torch.float32)[:, None]
    m32 = c["w32"] * s32 / ln32
    nrm = m32.norm(dim=1, keepdim=True)
    e32 = m32 / nrm
    yard = ((c["de32"] - e32 * (e32 * c["de32"]).sum(1, keepdim=True)) / nrm * c["w32"] / ln32).numpy()
    return ek.fp32_findings("ds", got, ref, yard)


@pytest.mark.parametrize("D", [128, 1472])
def test_pool_backward_bars_separate_planted_bugs(D):
    c = _case(D)
    assert not _seq_findings(c, None), "the clean stand-in meets the bar"
    assert _seq_findings(c, "len_from_chunk"), "1 / len taken from the chunk instead of the sequence"
    assert _seq_findings(c, "no_projection"), "the - e (e . de) term missing"
    # dx of every token row from ds, as two bf16 planes
    cu, seq = c["cu"], ek.seq_rows(c["cu"])
    _, s = ek.head_reference(c["x"], c["rs"], cu, c["w"])
    ds = ek._f32(np.stack([ek.bwd_seq_reference(s[b], ek.LENGTHS[b], c["w"], c["de"][b])[0] for b in range(len(ek.LENGTHS))]))
    ds = ds / np.abs(ek.bwd_tok_reference(c["x"], c["rs"], ds[seq])).max()  # as the GPU test scales d_emb
    ref = ek.bwd_tok_reference(c["x"], c["rs"], ds[seq])
    ds32, r32 = torch.from_numpy(ds[seq]).float(), c["rs32"][:, None]
    yard = (r32 * ds32 - c["x32"] * r32 ** 3 * ((ds32 * c["x32"]).sum(1, keepdim=True) / D)).numpy()
    bar = ek.yardstick_bar(ref, yard)
    for mutant in (None, "rs_squared"):
        v = ek._f32(ek.bwd_tok_reference(c["x"], c["rs"], ds[seq], None, mutant))
        hi = _bf16(v)
        found = ek.planes_findings("dx", hi, _bf16(v - hi), ref, bar)
        assert bool(found) == (mutant is not None), (mutant, found)


def test_unfold_bars_separate_planted_bugs():
    rng = np.random.default_rng(0)
    for mode, rows, n in ((ek.UNFOLD_GEGLU, 128, 0), (ek.UNFOLD_GEGLU, 448, 0), (ek.UNFOLD_QKV, 39, 13), (ek.UNFOLD_PLAIN, 40, 0)):
        for S in (2, 5):
            nsrc = {ek.UNFOLD_PLAIN: 0, ek.UNFOLD_QKV: 3, ek.UNFOLD_GEGLU: 2}[mode]
            per = n if mode == ek.UNFOLD_QKV else rows // 2
            part = rng.integers(-8, 9, (S, rows, 128)).astype(np.float64)
            masters = [rng.integers(-4, 5, (per, 128)).astype(np.float64) for _ in range(nsrc)]
            ln = 2.0 ** rng.integers(-2, 3, 128)
            g_ref, dln_ref = ek.unfold_reference(part, mode, n, masters, ln)
            mutants = ["splits_minus_one"] + (["geglu_block_off"] if mode == ek.UNFOLD_GEGLU else [])
            for mutant in mutants:  # the integer partials' comparison is exact equality
                g, dln = ek.unfold_reference(part, mode, n, masters, ln, mutant)
                assert not all(np.array_equal(a, b) for a, b in zip(g, g_ref)), (mode, mutant)
                assert dln_ref is None or mutant == "geglu_block_off" or not np.array_equal(dln, dln_ref)


@pytest.mark.parametrize("D", [128, 1472])
def test_embed_scatter_bar_separates_a_negative_id_that_is_ignored(D):
    V = 384
    for T in (255, 256, 257, 600):
        ids, dx = ek.embed_inputs(T, V, D)
        hi = _bf16(dx)
        g = (hi + _bf16(dx.astype(np.float64) - hi)).astype(np.float32)
        want = ek.embed_bwd_reference(ids, g.astype(np.float64), V)
        idc = np.clip(ids, 0, V - 1)
        yard = torch.zeros(V, D).index_add_(0, torch.from_numpy(idc).long(), torch.from_numpy(g)).numpy()
        bound = np.zeros((V, D))
        np.add.at(bound, idc, np.abs(g.astype(np.float64)))
        bound *= np.bincount(idc, minlength=V).max() * U
        assert not ek.fp32_findings("dtable", ek.standin_scatter(ids, g.astype(np.float64), V), want, yard, bound)
        assert ek.fp32_findings("dtable", ek.standin_scatter(ids, g.astype(np.float64), V, "negative_ignored"), want, yard, bound)
