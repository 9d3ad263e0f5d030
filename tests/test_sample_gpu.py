"""Sampled tactic generation on the MI355X: ``rp_sample_step`` against the float64 reference sampler
(tests/sample_helpers.py) on hand-built rows, its distribution, ``sample`` / ``sample_many`` end to end, and the ABI's
argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from sample_helpers import GRID, KERNEL_T, kernel_case, margin_bound, reference_sample, uniforms  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, HipT5Generator  # noqa: E402
from reprover_amd.generation import SampleState  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, PAD = 1, 0


def _state(n, nb, max_len, seeds):
    bits = np.asarray(seeds, dtype=np.uint32).view(np.int32)
    return SampleState(seeds=torch.from_numpy(bits.copy()).to(DEV),
                       seq=torch.full((n, nb, max_len), -7, dtype=torch.int32, device=DEV),
                       cum_logprob=torch.zeros((n, nb), dtype=torch.float32, device=DEV),
                       n_generated=torch.zeros((n, nb), dtype=torch.int32, device=DEV),
                       finished=torch.zeros((n, nb), dtype=torch.int32, device=DEV),
                       tokens=torch.full((n * nb,), -7, dtype=torch.int32, device=DEV))


# ---- the kernel against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 64, 1024])
@pytest.mark.parametrize("V", [1, 3, 384, 512])
def test_kernel_equals_the_reference_sampler(V, rows):
    """Every grid point over hand-built rows (one-hot, -inf entries, ties at the top-k threshold, flat, random): the token
    of every compared row, the exact score increment, pad and an unchanged score on finished rows, the EOS flag.  Rows
    are laid out as states of min(rows, 64) samples; the states sit in the slots in descending order."""
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    lp, seeds, active, row_state, row_sample, u = kernel_case(lib, V, rows)
    nb = min(rows, 64)
    n = rows // nb
    t, max_len = KERNEL_T, 9
    lp_d = torch.from_numpy(lp).to(DEV)
    start = np.linspace(-3, 3, n * nb, dtype=np.float32).reshape(n, nb)
    was_finished = (np.arange(n * nb).reshape(n, nb) % 5) == 2
    for T, k, p in GRID:
        k = V if k == "vocab" else k
        want, _, margins, _ = reference_sample(lp, u, T, k, p)
        st = _state(n, nb, max_len, seeds)
        st.cum_logprob.copy_(torch.from_numpy(start))
        st.finished.copy_(torch.from_numpy(was_finished.astype(np.int32)))
        dec.sample_step(lp_d, active, t, st, T, k, p, EOS, PAD)
        seq, tok_next = st.seq.cpu().numpy(), st.tokens.cpu().numpy()
        cum, ngen, fin = st.cum_logprob.cpu().numpy(), st.n_generated.cpu().numpy(), st.finished.cpu().numpy()
        assert (np.delete(seq, t + 1, axis=2) == -7).all()  # only position t + 1 is written
        got = seq[row_state, row_sample, t + 1]
        assert np.array_equal(tok_next, got)
        done = was_finished[row_state, row_sample]
        assert (got[done] == PAD).all()
        assert np.array_equal(cum[was_finished], start[was_finished]) and (ngen[was_finished] == 0).all()
        assert (fin[was_finished] == 1).all()
        live = ~done
        assert ((got[live] >= 0) & (got[live] < V)).all()
        inc = (start[row_state, row_sample] + lp[np.arange(rows), np.clip(got, 0, V - 1)]).astype(np.float32)
        assert np.array_equal(cum[row_state, row_sample][live], inc[live])  # exactly logprobs[token]
        assert (ngen[row_state, row_sample][live] == 1).all()
        assert np.array_equal(fin[row_state, row_sample][live], (got[live] == EOS).astype(np.int32))
        ok = margins > margin_bound(V)
        assert (~ok).sum() <= 0.1 * rows, (T, k, p, int((~ok).sum()))
        cmp = ok & live
        assert np.array_equal(got[cmp], want[cmp]), (T, k, p, np.nonzero(cmp & (got != want))[0][:8])


def test_distribution_of_one_fixed_row():
    """One 8-token row drawn for 1024 rows x 64 positions: every token's count within 5 binomial sigma."""
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    probs = np.array([0.3, 0.02, 0.15, 0.08, 0.25, 0.005, 0.095, 0.1])
    lp = torch.from_numpy(np.log(probs).astype(np.float32)).to(DEV)[None].repeat(1024, 1).contiguous()
    n, nb, T = 16, 64, 64
    st = _state(n, nb, T + 1, 31 + np.arange(n))
    for t in range(T):
        dec.sample_step(lp, list(range(n)), t, st, 1.0, 0, 1.0, -1, PAD)  # eos = -1: no row ever finishes
    toks = st.seq[:, :, 1:].cpu().numpy().reshape(-1)
    N = toks.size
    assert N == 65536 and int(st.n_generated.min()) == T
    counts = np.bincount(toks, minlength=8)
    p32 = np.exp(np.log(probs).astype(np.float32).astype(np.float64))
    p32 /= p32.sum()
    assert (np.abs(counts - N * p32) <= 5 * np.sqrt(N * p32 * (1 - p32))).all(), counts


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _gen(name, eos_boost=None):
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg)
    if eos_boost:
        sd["lm_head.weight"] = sd["lm_head.weight"].clone()
        sd["lm_head.weight"][1] *= eos_boost
    return cfg, HipT5Generator(cfg, sd, DEV)


@pytest.fixture(scope="module")
def tiny_gen():
    return _gen("tiny", eos_boost=4.0)  # EOS boosted: some samples stop early


def _same(a, b):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)  # bits


def _replay(gen, src, out, seed, nb, max_length, T, k, p):
    """Teacher-force every returned row through ``step`` with identity ancestry (all rows at once): the reference sampler
    on the replayed rows reproduces every compared token, the score is the sum of the replayed log-probs."""
    lib = _lib.load()
    dec = gen.decoder
    dec.start(gen.encode_hidden(src), nb, max_length)
    seq = out.sequences
    V = gen.cfg["vocab_size"]
    n_tok = [(row[1:].tolist().index(EOS) + 1) if EOS in row[1:].tolist() else seq.shape[1] - 1 for row in seq]
    total = np.zeros(nb)
    compared = skipped = 0
    argmax_rows = []
    for t in range(seq.shape[1] - 1):
        anc = torch.arange(t + 1)[None] * nb + torch.arange(nb)[:, None]
        lp = dec.step(seq[:, t], anc).cpu().numpy()
        u = uniforms(lib, [seed] * nb, range(nb), t)
        want, _, margins, _ = reference_sample(lp, u, T, k, p)
        for b in range(nb):
            if t >= n_tok[b]:
                assert int(seq[b, t + 1]) == PAD
                continue
            total[b] += lp[b, int(seq[b, t + 1])]
            srt = np.sort(lp[b])
            argmax_rows.append((b, t, int(lp[b].argmax()), srt[-1] > srt[-2]))
            if margins[b] > margin_bound(V):
                compared += 1
                assert int(seq[b, t + 1]) == int(want[b]), (b, t)
            else:
                skipped += 1
    assert skipped <= 0.1 * (compared + skipped)
    sc = out.sequences_scores.numpy().astype(np.float64)
    assert (np.abs(sc - total) <= 1e-4 * np.maximum(1.0, np.abs(total))).all(), (sc, total)
    return n_tok, argmax_rows


def test_tiny_sample_many_equals_sample_replay_and_early_finish(tiny_gen):
    cfg, gen = tiny_gen
    srcs = [source_ids(60, 3), source_ids(7, 4), source_ids(33, 5), source_ids(300, 6)]
    seeds = [21, 22, 23, 0xFFFFFFF0]
    nb, ml, kw = 6, 40, dict(temperature=1.2, top_k=50, top_p=0.95)
    alone = [gen.sample(s, nb, ml, seed=sd_, **kw) for s, sd_ in zip(srcs, seeds)]
    for sync_every in (1, 16, 64):
        for o, a in zip(gen.sample_many(srcs, nb, ml, seeds=seeds, sync_every=sync_every, **kw), alone):
            _same(o, a)
    perm = [2, 0, 3, 1]
    for o, i in zip(gen.sample_many([srcs[i] for i in perm], nb, ml, seeds=[seeds[i] for i in perm], sync_every=3, **kw), perm):
        _same(o, alone[i])
    for o, i in zip(gen.sample_many([srcs[3], srcs[1]], nb, ml, seeds=[seeds[3], seeds[1]], **kw), (3, 1)):  # another batch
        _same(o, alone[i])
    assert not torch.equal(gen.sample(srcs[0], nb, ml, seed=99, **kw).sequences, alone[0].sequences)
    lens = []
    for src, a, s in zip(srcs, alone, seeds):
        assert a.sequences.shape[0] == nb and (a.sequences[:, 0] == 0).all() and a.sequences.dtype == torch.int64
        n_tok, _ = _replay(gen, src, a, s, nb, ml, kw["temperature"], kw["top_k"], kw["top_p"])
        assert a.sequences.shape[1] == 1 + max(n_tok)  # trimmed to the longest sample
        lens.append(n_tok)
    assert any(n < ml - 1 for ns in lens for n in ns)  # some samples stopped at EOS before max_length
    assert len({max(ns) for ns in lens}) > 1  # the states end at different positions
    # a state whose samples have all finished leaves the active list at the next look
    calls = []
    step_many = gen.decoder.step_many
    gen.decoder.step_many = lambda active, *a, **k: (calls.append(list(active)), step_many(active, *a, **k))[1]
    try:
        outs = gen.sample_many(srcs, nb, ml, seeds=seeds, sync_every=2, **kw)
    finally:
        del gen.decoder.step_many
    for o, a in zip(outs, alone):
        _same(o, a)
    assert len(calls[0]) == len(srcs) and len(calls[-1]) < len(srcs)
    # length_penalty: the finished-beam formula over the same tokens
    pen = gen.sample(srcs[2], nb, ml, seed=seeds[2], length_penalty=1.0, **kw)
    assert torch.equal(pen.sequences, alone[2].sequences)
    assert torch.allclose(pen.sequences_scores, alone[2].sequences_scores / torch.tensor(lens[2], dtype=torch.float32),
                          rtol=1e-6, atol=0)


def test_top_k_one_is_greedy(tiny_gen):
    cfg, gen = tiny_gen
    src = source_ids(60, 3)
    ml = 24
    out = gen.sample(src, 3, ml, temperature=0.7, top_k=1, seed=5)
    n_tok, argmax_rows = _replay(gen, src, out, 5, 3, ml, 0.7, 1, 1.0)
    for b, t, am, unique in argmax_rows:
        if unique:
            assert int(out.sequences[b, t + 1]) == am
    greedy = gen.greedy(src, ml)
    if all(u for b, _, _, u in argmax_rows if b == 0):
        g = greedy.sequences[0]
        assert torch.equal(out.sequences[0, : len(g)], g) and (out.sequences[0, len(g):] == PAD).all()


def test_byt5_small_dimensions():
    """ByT5-small dimensions, a 300-byte source, 8 samples, max_length 32: batch = alone, and the replay."""
    cfg, gen = _gen("byt5-small")
    srcs = [source_ids(300, 8), source_ids(41, 9)]
    kw = dict(temperature=0.9, top_k=0, top_p=0.9)
    alone = [gen.sample(s, 8, 32, seed=70 + i, **kw) for i, s in enumerate(srcs)]
    for sync_every in (1, 16, 64):
        for o, a in zip(gen.sample_many(srcs, 8, 32, seeds=[70, 71], sync_every=sync_every, **kw), alone):
            _same(o, a)
    for o, i in zip(gen.sample_many(srcs[::-1], 8, 32, seeds=[71, 70], **kw), (1, 0)):
        _same(o, alone[i])
    _replay(gen, srcs[0], alone[0], 70, 8, 32, 0.9, 0, 0.9)


def test_python_layer_rejects_bad_parameters(tiny_gen):
    cfg, gen = tiny_gen
    src = source_ids(7, 4)
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.01), dict(top_k=-1), dict(num_samples=0),
               dict(max_length=1), dict(sync_every=0)):
        args = dict(num_samples=2, max_length=8)
        args.update(kw)
        with pytest.raises(ValueError):
            gen.sample(src, **args)
    with pytest.raises(ValueError):
        gen.sample_many([src] * 3, 2, 8, seeds=[1, 2])
    with pytest.raises(ValueError):
        gen.sample_many([src] * 17, 64, 8)  # generate_many's cap: 16 states of 64 rows


# ---- ABI errors -----------------------------------------------------------------------------------------------------------
def test_abi_rejects_invalid_parameters_without_launching():
    lib = _lib.load()
    err = lambda: lib.rp_last_error()  # noqa: E731
    buf = torch.full((4096,), 123, dtype=torch.int32, device=DEV)
    d = buf.data_ptr()
    act = np.arange(32, dtype=np.int32)
    a = act.ctypes.data_as(C.c_void_p)

    def call(V=384, n_active=2, n=2, nb=4, t=0, max_len=8, T=1.0, k=0, p=1.0, lp=d, active=a):
        return lib.rp_sample_step(lp, V, active, n_active, n, nb, d, t, max_len, T, k, p, 1, 0, d, d, d, d, d, None)

    for kw, word in ((dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(T=float("nan")), b"temperature"),
                     (dict(p=0.0), b"top_p"), (dict(p=1.5), b"top_p"), (dict(k=-1), b"top_k"), (dict(V=513), b"vocab"),
                     (dict(V=0), b"vocab"), (dict(nb=65), b"nb=65"), (dict(n_active=17, n=17, nb=64), b"rows"),
                     (dict(n=33, n_active=33), b"states"), (dict(n_active=3), b"active states=3"),
                     (dict(t=7), b"t=7"), (dict(lp=None), b"null"), (dict(active=None), b"null")):
        assert call(**kw) == -1 and word in err(), (kw, err())
    twice = np.array([1, 1], dtype=np.int32)
    assert call(active=twice.ctypes.data_as(C.c_void_p)) == -1 and b"twice" in err()
    torch.cuda.synchronize()
    assert bool((buf == 123).all())  # nothing was launched
