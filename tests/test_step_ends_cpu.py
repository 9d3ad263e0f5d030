"""The references of tests/test_step_ends_gpu.py and tests/test_merge_gpu.py pinned without a GPU: the float64
restatements in oracle/train_ref.py (grad_norm, clipped adamw_step / adamw_step64, contrastive_mse) against torch's own
``clip_grad_norm_`` + ``torch.optim.AdamW`` and autograd in float64 on the CPU, and oracle/common_ref.py::merge_topk
against ``masked_topk`` of the unsplit ranking.

Tolerance: both sides compute in float64 with a different but equivalent operation order (torch's lerp / addcdiv against
the oracle's plain expressions), a handful of roundings per element and step: 1e-12 relative to the largest magnitude
compared (2^-53 = 1.1e-16 per rounding; five steps of ~10 roundings stay four orders of magnitude below the bar)."""
import numpy as np
import torch

from oracle import common_ref, train_ref

REL = 1e-12  # float64 rounding, see the module docstring


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max(initial=0.0) <= REL * max(np.abs(b).max(initial=0.0), 1e-300)


def test_grad_norm_and_clipped_adamw_equal_torch_in_float64():
    rng = np.random.default_rng(11)
    n, max_norm, lr = 1003, 1.0, 1e-3
    unit = [rng.standard_normal(n) for _ in range(5)]
    # gradient norms below max_norm, just below it outside and inside the band where the + 1e-6 of the factor's denominator
    # already clips, far above it, and very far above it
    targets = [0.25, 1.0 - 1e-5, 1.0 - 1e-7, 40.0, 3e4]
    grads = [(u / np.linalg.norm(u) * t).astype(np.float32) for u, t in zip(unit, targets)]
    for betas, eps, wd in (((0.9, 0.999), 1e-8, 1e-2), ((0.8, 0.95), 1e-6, 0.0)):
        p0 = rng.standard_normal(n).astype(np.float32)
        ref_p = torch.nn.Parameter(torch.from_numpy(p0).double())
        opt = torch.optim.AdamW([ref_p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
        p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
        coefs = []
        for t, g in enumerate(grads):
            ref_p.grad = torch.from_numpy(g).double()
            total = torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
            norm = train_ref.grad_norm(g)
            assert abs(norm - float(total)) <= REL * float(total)
            # the factor torch applied, read back from the gradient it scaled in place
            k = int(np.abs(g).argmax())
            coefs.append(float(ref_p.grad[k]) / float(g[k]))
            assert abs(train_ref.clip_coef(norm, max_norm) - coefs[-1]) <= 1e-12
            opt.step()
            p, m, v = train_ref.adamw_step64(p, g, m, v, t + 1, lr, betas, eps, wd, clip=(norm, max_norm))
            st = opt.state[ref_p]
            assert _close(p, ref_p.detach().numpy()), t
            assert _close(m, st["exp_avg"].numpy()) and _close(v, st["exp_avg_sq"].numpy()), t
        assert coefs[0] == 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0 and coefs[4] < 1e-4  # both sides of the clip
    # adamw_step (parameters rounded to fp32 per step, as the fixtures store them) is the same update
    p32, m32, v32 = train_ref.adamw_step(p0, grads[3], np.zeros(n), np.zeros(n), 1, lr, clip=(40.0, 1.0))
    p64, m64, v64 = train_ref.adamw_step64(p0, grads[3], np.zeros(n), np.zeros(n), 1, lr, clip=(40.0, 1.0))
    assert np.array_equal(p32, p64.astype(np.float32)) and np.array_equal(m32, m64) and np.array_equal(v32, v64)
    # no clip argument = the unclipped update; an all-zero gradient clips by min(1, max_norm / 1e-6) = 1
    assert train_ref.clip_coef(0.0, 1.0) == 1.0 and train_ref.grad_norm(np.zeros(7, np.float32)) == 0.0
    assert train_ref.grad_norm([np.array([3.0]), np.array([[4.0]])]) == 5.0


def test_contrastive_mse_equals_autograd_in_float64():
    rng = np.random.default_rng(12)
    for B, P, D, scale in ((1, 1, 4, 1.0), (3, 9, 7, 1.0), (8, 32, 1472, 1.0), (5, 10, 64, 30.0)):
        C = rng.standard_normal((B, D)) * scale
        Pm = rng.standard_normal((P, D)) * scale
        label = rng.uniform(-2, 2, size=(B, P))
        tc, tp = torch.from_numpy(C).requires_grad_(True), torch.from_numpy(Pm).requires_grad_(True)
        sim = tc @ tp.T
        loss = torch.nn.functional.mse_loss(sim, torch.from_numpy(label))
        loss.backward()
        got = train_ref.contrastive_mse(C, Pm, label)
        assert abs(got[0] - loss.item()) <= REL * loss.item()
        at = train_ref.contrastive_mse(C, Pm, label, similarity=got[1])  # the same point, handed in
        assert at[0] == got[0] and np.array_equal(at[2], got[2]) and np.array_equal(at[3], got[3])
        assert _close(got[1], sim.detach().numpy()) and _close(got[2], tc.grad.numpy()) and _close(got[3], tp.grad.numpy())


def test_merge_topk_of_a_split_ranking_equals_masked_topk_of_the_whole():
    rng = np.random.default_rng(13)
    B, N, R, k = 9, 400, 4, 25
    # few distinct values: ties within and across the shards, broken by id
    sims = rng.choice(np.array([-1.5, -0.25, 0.0, 0.125, 0.5, 0.75], dtype=np.float32), size=(B, N))
    acc = rng.random((B, N)) < 0.6
    acc[0] = False
    acc[0, :7] = True  # fewer than k in total
    acc[1] = False     # nothing at all
    bounds = [0, 50, 51, 300, N]  # uneven shards, one of a single row
    scores = np.full((R, B, k), np.inf, dtype=np.float32)  # stale data behind the counts
    ids = np.full((R, B, k), 12345, dtype=np.int32)
    counts = np.zeros((R, B), dtype=np.int32)
    for r in range(R):
        lo, hi = bounds[r], bounds[r + 1]
        for b in range(B):
            kk = min(k, int(acc[b, lo:hi].sum()))
            if kk:
                i, s = common_ref.masked_topk(sims[b : b + 1, lo:hi], acc[b : b + 1, lo:hi], kk)
                scores[r, b, :kk], ids[r, b, :kk] = s[0], i[0] + lo
            counts[r, b] = kk
    counts[2, 1] = -1  # "contributes nothing" (it had nothing anyway)
    mi, ms, mc = common_ref.merge_topk(scores, ids, counts, k)
    assert mi.dtype == np.int32 and ms.dtype == np.float32 and mc.dtype == np.int32
    for b in range(B):
        n = min(k, int(acc[b].sum()))
        assert mc[b] == n
        assert np.all(mi[b, n:] == -1) and np.all(np.isneginf(ms[b, n:]))
        if n:
            wi, ws = common_ref.masked_topk(sims[b : b + 1], acc[b : b + 1], n)
            assert np.array_equal(mi[b, :n], wi[0]) and np.array_equal(ms[b, :n].view(np.int32), ws[0].view(np.int32))
    assert mc[0] == 7 and mc[1] == 0
    # a negative count drops a rank that HAD entries
    counts2 = counts.copy()
    counts2[3, 2] = -1
    mi2, _, mc2 = common_ref.merge_topk(scores, ids, counts2, k)
    assert not np.any(mi2[2, : mc2[2]] >= bounds[3])
    # k smaller than the lists' width, and k = 1
    mi3, ms3, mc3 = common_ref.merge_topk(scores, ids, counts, 1)
    assert np.array_equal(mi3[2:, 0], mi[2:, 0]) and np.array_equal(mc3, np.minimum(mc, 1))
