"""rp_topk_merge / rp_topk_merge_strided on hand-built rank lists (not scan output), compared EXACTLY - ids, score bits,
counts, the -1 / -inf padding - with oracle/common_ref.py::merge_topk (a lexsort of the union; pinned against masked_topk
of the unsplit ranking by tests/test_step_ends_cpu.py).  No tolerance anywhere: a merge moves bits, it computes nothing.

What the lists are made of: scores from a dozen bf16-exact values (positive, negative, zero, subnormal) so that most
neighbours tie, within a rank and across ranks, and the id order decides; rank r owns ids [r 2^20, (r + 1) 2^20) as
``id_offset`` gives them; per (rank, query) counts from {-1 ("contributes nothing"), 0, 1, k - 1, k, uniform}; behind the
count stale garbage (+inf and NaN scores, ids of another rank) that must never surface.  No NaN and no -0.0 among the live
scores (the order of signed zeros is the scan's key order, pinned with the beam selection)."""
import time

import numpy as np
import pytest
import torch

import hip_helpers as hh
from oracle import common_ref
from reprover_amd import _lib

pytestmark = pytest.mark.gpu

RP_E_INVALID, RP_E_WORKSPACE = -1, -3
RANKS, QUERIES, KS = (1, 2, 3, 8, 16), (1, 5, 64, 257, 2048), (1, 2, 7, 100, 333, 1024)
ID_SPAN = 1 << 20
# descending; every value has at most 8 significant bits (bf16-exact), two are subnormal in fp32
VALUES = np.array([96.0, 1.0, 0.75, 0.4375, 0.25, 2.0 ** -130, 0.0, -(2.0 ** -130), -0.125, -0.5, -3.0], dtype=np.float32)
WORKSPACE_LIMIT = 2 << 30


def make_case(rng, R, B, k):
    """(scores f32 [R, B, k], ids i32 [R, B, k], counts i32 [R, B]): rows sorted best-first over their live prefix."""
    assert np.all(np.diff(VALUES) < 0) and not np.any(np.signbit(VALUES[VALUES == 0]))
    nv = int(rng.integers(2, len(VALUES) + 1))  # how many distinct scores this case uses: few = nearly everything ties
    pick = np.sort(rng.choice(len(VALUES), size=nv, replace=False))
    v_idx = pick[rng.integers(0, nv, size=(R, B, k))]
    # distinct ids per (rank, query): an arithmetic progression with an odd step, modulo the rank's span
    base = rng.integers(0, ID_SPAN, size=(R, B, 1))
    step = rng.integers(0, ID_SPAN // 2, size=(R, B, 1)) * 2 + 1
    local = (base + step * np.arange(k)[None, None, :]) % ID_SPAN
    order = np.argsort(v_idx.astype(np.int64) * ID_SPAN + local, axis=2, kind="stable")  # (score descending, id ascending)
    v_idx, local = np.take_along_axis(v_idx, order, 2), np.take_along_axis(local, order, 2)
    scores = VALUES[v_idx]
    ids = (local + np.arange(R)[:, None, None] * ID_SPAN).astype(np.int32)
    kind = rng.integers(0, 6, size=(R, B))
    counts = np.choose(kind, [np.full((R, B), -1), np.zeros((R, B), int), np.ones((R, B), int), np.full((R, B), k - 1),
                              np.full((R, B), k), rng.integers(0, k + 1, size=(R, B))]).astype(np.int32)
    counts = np.minimum(counts, k)
    if B >= 3:
        counts[:, B - 1] = rng.choice([-1, 0], size=R)  # one query where every rank is -1 or 0 -> count 0, all padding
        if k > 1:                                        # and one with fewer than k in total
            counts[:, B - 2] = rng.choice([-1, 0], size=R)
            counts[int(rng.integers(0, R)), B - 2] = 1
    # stale data behind the live prefix
    dead = np.arange(k)[None, None, :] >= np.maximum(counts, 0)[:, :, None]
    garbage = np.where(rng.random((R, B, k)) < 0.5, np.float32(np.inf), np.float32(np.nan)).astype(np.float32)
    scores = np.where(dead, garbage, scores).astype(np.float32)
    other = ((np.arange(R)[:, None, None] + 1) % max(R, 2)) * ID_SPAN + local
    ids = np.where(dead, other, ids).astype(np.int32)
    return scores, ids, counts


def pack_blocks(scores, ids, counts, Bt, q0, rank_stride, rng):
    """The all-gather's receive buffer: R blocks [scores Bt*k | ids Bt*k | counts Bt] (4-byte units) rank_stride apart, the
    case's B queries at rows q0 .. q0 + B of each; every other row and every gap is poison (full rows of +inf scores with
    low ids: a merge that reads a neighbour's row or a wrong stride unit returns them first)."""
    R, B, k = scores.shape
    block = Bt * (2 * k + 1)
    flat = np.empty((R - 1) * rank_stride + block, dtype=np.int32)
    flat[:] = np.float32(np.inf).view(np.int32)  # as a score +inf, as an id or a count a huge positive number
    for r in range(R):
        o = r * rank_stride
        s = flat[o : o + Bt * k].reshape(Bt, k)
        i = flat[o + Bt * k : o + 2 * Bt * k].reshape(Bt, k)
        c = flat[o + 2 * Bt * k : o + block]
        i[:] = rng.integers(0, 1000, size=(Bt, k))
        c[:] = k
        s[q0 : q0 + B] = scores[r].view(np.int32)
        i[q0 : q0 + B] = ids[r]
        c[q0 : q0 + B] = counts[r]
    return flat


def assert_same(got, want, what):
    gi, gs, gc = (t.cpu().numpy() for t in got)
    wi, ws, wc = want
    assert np.array_equal(gc, wc), (what, "counts", gc[:8], wc[:8])
    assert np.array_equal(gi, wi), (what, "ids", np.argwhere(gi != wi)[:4])
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), (what, "score bits", np.argwhere(gs.view(np.int32) != ws.view(np.int32))[:4])


def sweep_cases():
    """40 seeded draws + the corners the draws need not hit (R = 16 with k = 1024 at B = 64 and 2048, R * k = 16,384 keys per
    query; a single rank; a single query)."""
    rng = np.random.default_rng(20240)
    drawn = [(int(rng.choice(RANKS)), int(rng.choice(QUERIES)), int(rng.choice(KS))) for _ in range(40)]
    return drawn + [(16, 64, 1024), (16, 2048, 1024), (1, 1, 1), (8, 2048, 100), (3, 257, 333)]


def test_merge_sweep_plain_and_strided_exact():
    lib = _lib.load()
    cases = sweep_cases()
    ran, skipped, saw_empty, saw_short = [], 0, 0, 0
    t0 = time.time()
    for n, (R, B, k) in enumerate(cases):
        if lib.rp_topk_merge_workspace_bytes(R, B, k) > WORKSPACE_LIMIT:
            skipped += 1
            continue
        rng = np.random.default_rng(7000 + n)
        scores, ids, counts = make_case(rng, R, B, k)
        want = common_ref.merge_topk(scores, ids, counts, k)
        total = np.maximum(counts, 0).sum(0)
        assert np.array_equal(want[2], np.minimum(total, k))
        saw_empty += int((total == 0).any())
        saw_short += int(((total > 0) & (total < k)).any())
        d_s, d_i, d_c = (torch.from_numpy(a).cuda() for a in (scores, ids, counts))
        plain = hh.topk_merge(d_s, d_i, d_c)
        assert_same(plain, want, f"plain R={R} B={B} k={k}")
        again = hh.topk_merge(d_s, d_i, d_c)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, again))
        del d_s, d_i, d_c, again
        # the strided form: Bt > B queries per block, this rank merging its own [q0, q0 + B)
        Bt = B + 5
        tight = Bt * (2 * k + 1)
        for q0, stride in ((0, tight), (3, tight), (Bt - B, tight), (3, tight + 13)):
            packed = torch.from_numpy(pack_blocks(scores, ids, counts, Bt, q0, stride, rng)).cuda()
            got = hh.topk_merge_strided(packed, R, Bt, k, q0, B, stride)
            for a, b, name in zip(got, plain, ("ids", "scores", "counts")):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (f"strided R={R} B={B} k={k} q0={q0} stride={stride}", name)
            del packed, got
        del plain
        torch.cuda.empty_cache()
        ran.append((R, B, k))
        print(f"merge R={R} B={B} k={k}: exact (plain + 4 strided layouts); counts 0..{int(want[2].max())}")
    print(f"merge sweep: {len(ran)} cases run, {skipped} skipped, {time.time() - t0:.1f} s")
    assert len(ran) >= 40 and skipped * 4 < len(cases)
    assert any(R == 16 and k == 1024 and B >= 64 for R, B, k in ran)
    assert saw_empty >= 1 and saw_short >= 1


def test_merge_cross_rank_ties_take_the_lower_id():
    """Every live entry of every rank has the SAME score: the output is the k lowest ids of the union, i.e. rank 0's list
    first, then rank 1's - and with k larger than a rank's list the merge crosses ranks inside one tie."""
    R, B, k = 4, 3, 7
    scores = np.full((R, B, k), 0.25, dtype=np.float32)
    ids = (np.arange(R)[:, None, None] * ID_SPAN + np.arange(B)[None, :, None] * 16 + np.arange(k)[None, None, :] * 2).astype(np.int32)
    counts = np.full((R, B), 3, dtype=np.int32)
    counts[0, 1] = -1  # rank 0 drops out of query 1: rank 1's ids lead there
    want = common_ref.merge_topk(scores, ids, counts, k)
    assert want[0][0].tolist() == [0, 2, 4, ID_SPAN, ID_SPAN + 2, ID_SPAN + 4, 2 * ID_SPAN]
    assert want[0][1, 0] == ID_SPAN + 16
    got = hh.topk_merge(*(torch.from_numpy(a).cuda() for a in (scores, ids, counts)))
    assert_same(got, want, "all tied")


def test_merge_rejects_bad_arguments():
    lib = _lib.load()
    R, B, k = 2, 4, 8
    s = torch.zeros((R, B, k), dtype=torch.float32, device="cuda")
    i = torch.arange(R * B * k, dtype=torch.int32, device="cuda").view(R, B, k).contiguous()  # distinct ids, as the contract asks
    c = torch.full((R, B), k, dtype=torch.int32, device="cuda")
    out_s = torch.full((B, 1025), 7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((B, 1025), 7, dtype=torch.int32, device="cuda")
    out_c = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((R * B * 1025 * 8 + 256,), 7, dtype=torch.uint8, device="cuda")
    need = lib.rp_topk_merge_workspace_bytes(R, B, k)
    assert need >= R * B * k * 8
    outs = (_lib.ptr(out_s), _lib.ptr(out_i), _lib.ptr(out_c))
    stream = _lib.current_stream()

    def strided(stride, R_=R, k_=k, nbytes=ws.numel()):
        return lib.rp_topk_merge_strided(_lib.ptr(s), _lib.ptr(i), _lib.ptr(c), stride, R_, B, k_, *outs, _lib.ptr(ws), nbytes, stream)

    def plain(R_=R, k_=k, nbytes=ws.numel()):
        return lib.rp_topk_merge(_lib.ptr(s), _lib.ptr(i), _lib.ptr(c), R_, B, k_, *outs, _lib.ptr(ws), nbytes, stream)

    for call, text in ((lambda: strided(0), "rank_stride"), (lambda: strided(-5), "rank_stride"),
                       (lambda: strided(B * k, k_=1025), "k=1025"), (lambda: plain(k_=1025), "k=1025"), (lambda: plain(R_=0), "R=0"),
                       (lambda: strided(B * k, R_=0), "R=0"), (lambda: plain(k_=0), "k=0")):
        st = call()
        assert st == RP_E_INVALID and text in hh.last_error(), (st, text, hh.last_error())
    for call in (lambda: plain(nbytes=need - 1), lambda: strided(B * k, nbytes=need - 1), lambda: plain(nbytes=0)):
        assert call() == RP_E_WORKSPACE and "workspace" in hh.last_error()
    torch.cuda.synchronize()
    assert bool((out_s == 7.0).all()) and bool((out_i == 7).all()) and bool((out_c == 7).all()) and bool((ws == 7).all()), \
        "nothing was launched"
    assert plain() == 0  # the same arguments, whole: runs
    torch.cuda.synchronize()
    assert out_c.tolist() == [k] * B
