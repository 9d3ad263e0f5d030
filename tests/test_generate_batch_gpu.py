"""Batched tactic generation on the MI355X (rp_decoder_batch_*, rp_beam_select_batch, generate_many / greedy_many): for
every state the batched entry points give the bits of the per-state ones - step rows, cross K/V, selection, whole
searches with their traces, and the product classes built on them - whichever other states share the call."""
import asyncio
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import simulated_search, source_ids  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, HipT5Generator  # noqa: E402
from reprover_amd.tokenizer import batch_decode  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    return z, cfg, sd


@pytest.fixture(scope="module")
def tiny_gen(golden_dir):
    z, cfg, sd = _g20(golden_dir)
    return z, cfg, sd, HipT5Generator(cfg, sd, DEV)


def _sources(src):
    """Eight distinct sources: the G20 source, truncations of it (EOS re-appended) and seeded ones of other lengths."""
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    return [np.asarray(src, dtype=np.int32), cut(40), cut(7), source_ids(120, 11), source_ids(33, 12), source_ids(1, 0),
            source_ids(257, 13), cut(150)]


def _pack(srcs):
    cu = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.int32)
    return np.concatenate(srcs).astype(np.int32), cu


def _same_output(got, want):
    assert torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.sequences_scores, want.sequences_scores)  # bits, not a tolerance


def _same_trace(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))


# ---- step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 4, 64])
def test_step_many_rows_and_cross_kv_equal_the_per_state_step(tiny_gen, nb):
    """Sources of 1, 300 and 2048 bytes in one batch; the ancestry tables of seeded simulated searches (rows reordered
    with repeats, one search per state); all states active, then strict subsets."""
    z, cfg, sd, gen = tiny_gen
    dec = gen.decoder
    srcs = [source_ids(1, 0), np.asarray(z["src"], dtype=np.int32), source_ids(2048, 21)]
    assert [len(s) for s in srcs] == [1, 300, 2048]
    T = 9
    ids, cu = _pack(srcs)
    enc = gen.encode_hidden_packed(ids, cu)
    nkv = cfg["num_decoder_layers"] * 2 * cfg["num_heads"] * cfg["d_kv"]
    runs = [list(simulated_search(nb, T, seed=40 + i)) for i in range(len(srcs))]
    ref, ref_ckv = [], []
    for i in range(len(srcs)):
        e = enc[int(cu[i]) : int(cu[i + 1])].contiguous()
        assert torch.equal(e, gen.encode_hidden(srcs[i]))  # packed encoder rows are the per-source bits
        dec.start(e, nb, T)
        ref_ckv.append(dec._ws[: e.shape[0] * nkv * 2].clone())
        ref.append([dec.step(tok, anc).clone() for _, tok, anc in runs[i]])
    dec.start_many(enc, cu, nb, T)
    got_ckv = dec._ws[: int(cu[-1]) * nkv * 2]
    assert torch.equal(got_ckv, torch.cat(ref_ckv))  # one GEMM over all rows = rp_decoder_cross_kv per source
    for t in range(T):
        active = [0, 1, 2] if t < 4 else ([0, 2] if t < 7 else [1])
        if t == 7:  # state 1 sat out steps 4-6: give it its rows for those positions (alone in the list)
            for tt in range(4, 7):
                one = dec.step_many([1], runs[1][tt][1], runs[1][tt][2])
                assert torch.equal(one, ref[1][tt])
        tok = torch.cat([runs[i][t][1] for i in active])
        anc = torch.cat([runs[i][t][2] for i in active])
        lp = dec.step_many(active, tok, anc)
        for a, i in enumerate(active):
            assert torch.equal(lp[a * nb : (a + 1) * nb], ref[i][t]), (t, i)


def test_step_many_does_not_depend_on_slot_order(tiny_gen):
    """The active list in another order (slots permuted): every state's rows keep their bits."""
    z, cfg, sd, gen = tiny_gen
    dec = gen.decoder
    srcs = _sources(z["src"])[:4]
    ids, cu = _pack(srcs)
    enc = gen.encode_hidden_packed(ids, cu)
    nb, T = 4, 5
    runs = [list(simulated_search(nb, T, seed=60 + i)) for i in range(4)]
    outs = {}
    for order in ([0, 1, 2, 3], [2, 0, 3, 1]):
        dec.start_many(enc, cu, nb, T)
        for t in range(T):
            lp = dec.step_many(order, torch.cat([runs[i][t][1] for i in order]), torch.cat([runs[i][t][2] for i in order]))
        outs[tuple(order)] = {i: lp[a * nb : (a + 1) * nb].clone() for a, i in enumerate(order)}
    for i in range(4):
        assert torch.equal(outs[(0, 1, 2, 3)][i], outs[(2, 0, 3, 1)][i])


# ---- select --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,V,k", [(1, 384, 2), (4, 384, 8), (64, 384, 128), (64, 512, 128), (4, 512, 128), (3, 37, 100),
                                    (1, 1, 1), (64, 5, 128)])
def test_select_batch_equals_select_per_state_and_stable_sort(nb, V, k):
    lib = _lib.load()
    dec = HipT5Decoder.from_handle(lib, None, None, DEV)
    g = torch.Generator().manual_seed(100 * nb + V)
    n = 5
    lp = torch.log_softmax(torch.randn(n * nb, V, generator=g) * 3, -1)
    run = torch.randn(n * nb, generator=g)
    # state 0: plain.  state 1: only beam 0 live (-1e9 rows), an exact tie inside a row
    run[nb + 1 : 2 * nb] = -1e9
    if V > 9:
        lp[nb, 7] = lp[nb, 9] = lp[nb].max() + 1
    # state 2: exact ties across rows (equal rows, equal running scores)
    lp[2 * nb : 3 * nb] = lp[2 * nb].clone()
    run[2 * nb : 3 * nb] = 0.25
    # state 3: -inf entries and signed zeros
    lp[3 * nb : 4 * nb, ::3] = float("-inf")
    lp[3 * nb : 4 * nb, 1::3] = torch.where(torch.arange(len(lp[0, 1::3])) % 2 == 0, 0.0, -0.0)
    run[3 * nb : 4 * nb] = -0.0  # keeps the sign of a zero log-prob
    # state 4: every running score -1e9 except the last beam
    run[4 * nb : 5 * nb - 1] = -1e9
    s, t, p = dec.select_many(lp.to(DEV), run.to(DEV), nb, k)
    assert s.shape == t.shape == p.shape == (n, k)
    for a in range(n):
        blk, rb = lp[a * nb : (a + 1) * nb], run[a * nb : (a + 1) * nb]
        s1, t1, p1 = dec.select(blk.to(DEV), rb.to(DEV), k)
        assert torch.equal(s[a].view(torch.int32), s1.view(torch.int32))  # the same bits, signed zeros included
        assert torch.equal(t[a], t1) and torch.equal(p[a], p1)
        rs, ri = torch.sort((blk + rb[:, None]).reshape(-1), descending=True, stable=True)
        assert torch.equal(s[a].cpu(), rs[:k])
        assert torch.equal(t[a].cpu().long(), ri[:k] % V) and torch.equal(p[a].cpu().long(), ri[:k] // V)


# ---- generate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("nb", [4, 64])
@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_generate_many_equals_generate(tiny_gen, B, nb, lp):
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])[:B]
    ml = 64 if nb == 4 else 24
    traces = []
    outs = gen.generate_many(srcs, nb, ml, lp, traces=traces)
    assert len(outs) == len(traces) == B
    for i, s in enumerate(srcs):
        tr = []
        _same_output(outs[i], gen.generate(s, nb, ml, lp, trace=tr))
        _same_trace(traces[i], tr)


def test_generate_many_states_stop_at_different_steps(tiny_gen):
    """The early-exit path on the device: the states of one batch stop at different steps, one at least 3 steps before
    the last; the states that go on keep their bits after the others have left the active list."""
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])
    nb, ml, lp = 4, 64, 0.0
    traces = []
    outs = gen.generate_many(srcs, nb, ml, lp, traces=traces)
    stops = [len(t) for t in traces]
    print("stop steps:", stops)
    assert len(set(stops)) > 1 and min(stops) <= max(stops) - 3, stops
    for i, s in enumerate(srcs):
        tr = []
        _same_output(outs[i], gen.generate(s, nb, ml, lp, trace=tr))
        _same_trace(traces[i], tr)
        assert len(tr) == stops[i]


def test_generate_many_permuted_and_duplicated(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])
    nb, ml, lp = 4, 64, 0.0
    base_tr = []
    base = gen.generate_many(srcs, nb, ml, lp, traces=base_tr)
    perm = [5, 2, 7, 0, 2, 6, 1, 4, 3, 2]  # a permutation with state 2 three times
    tr = []
    outs = gen.generate_many([srcs[i] for i in perm], nb, ml, lp, traces=tr)
    for o, t, i in zip(outs, tr, perm):
        _same_output(o, base[i])
        _same_trace(t, base_tr[i])


def test_greedy_many_equals_greedy(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    srcs = _sources(z["src"])
    for ml in (6, 40):
        outs = gen.greedy_many(srcs, ml)
        alone = [gen.greedy(s, ml) for s in srcs]
        for o, w in zip(outs, alone):
            _same_output(o, w)
        again = gen.greedy_many(srcs[::-1] + srcs[:1], ml)
        for o, w in zip(again, alone[::-1] + alone[:1]):
            _same_output(o, w)
    lens = [a.sequences.shape[1] for a in alone]
    print("greedy lengths:", lens)
    assert min(lens) <= max(lens) - 3, lens  # EOS at different steps at max_length 40


def test_generate_many_byt5_small_64_beams():
    """ByT5-small dimensions (d_model 1472, d_ff 3584: the 3- and 7-piece GEMM forms), 4 states, 64 beams, sources of up to
    2048 bytes."""
    cfg = synth.seq2seq_config("byt5-small")
    gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg), DEV)
    srcs = [source_ids(2048, 31), source_ids(700, 32), source_ids(1, 0), source_ids(1999, 33)]
    nb, ml, lp = 64, 40, 0.0
    traces = []
    outs = gen.generate_many(srcs, nb, ml, lp, traces=traces)
    for i, s in enumerate(srcs):
        tr = []
        _same_output(outs[i], gen.generate(s, nb, ml, lp, trace=tr))
        _same_trace(traces[i], tr)


# ---- product -------------------------------------------------------------------------------------------------------------
def _save_generator_dir(path, cfg, sd):
    os.makedirs(path, exist_ok=True)
    hf = dict(model_type="t5", architectures=["T5ForConditionalGeneration"], is_encoder_decoder=True,
              decoder_start_token_id=0, eos_token_id=1, pad_token_id=0,
              **{k: cfg[k] for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                     "num_decoder_layers", "relative_attention_num_buckets",
                                     "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj",
                                     "tie_word_embeddings")})
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(hf, fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()
               if k not in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight")},
              os.path.join(path, "model.safetensors"))


@pytest.fixture(scope="module")
def gen_dir(golden_dir):
    z, cfg, sd = _g20(golden_dir)
    d = os.path.join(tempfile.mkdtemp(), "gen")
    _save_generator_dir(d, cfg, sd)
    return z, d


@pytest.mark.parametrize("num_beams", [1, 4])
def test_validation_generate_batch_equals_per_state_loop(gen_dir, num_beams):
    from reprover_amd.generator.model import RetrievalAugmentedGenerator

    z, d = gen_dir
    model = RetrievalAugmentedGenerator(d, 5e-4, 2000, num_beams, 100, 1, 1, 250, 2048, 40, device=DEV)
    srcs = _sources(z["src"])
    S = max(len(s) for s in srcs)
    ids = torch.zeros((len(srcs), S), dtype=torch.int64)
    mask = torch.zeros((len(srcs), S), dtype=torch.int64)
    for b, s in enumerate(srcs):
        ids[b, : len(s)] = torch.from_numpy(s.astype(np.int64))
        mask[b, : len(s)] = 1
    got = model.generate_batch(ids, mask)
    g = model.generator
    want = []
    for s in srcs:
        seqs = (g.greedy(s, 40) if num_beams == 1 else g.generate(s, num_beams, 40, length_penalty=1.0)).sequences
        want.append(batch_decode(seqs.tolist(), skip_special_tokens=True))
    assert got == want and all(len(p) == num_beams for p in got)


def test_prover_batch_generate_equals_generate_sync(gen_dir):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator, RetrievalAugmentedGenerator
    from reprover_amd.retrieval import index as index_cli

    z, gdir = gen_dir
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900, 60)]
    states[4] = states[0]  # a repeated state
    hf = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0)
    hf.initialize()
    n = len(states)
    paths, names, poses = ["f.lean"] * n, ["thm"] * n, [Pos(1, 0)] * n
    got = hf.batch_generate_sync(states, paths, names, poses, 8)
    want = [hf.generate_sync(s, "f.lean", "thm", Pos(1, 0), 8) for s in states]
    assert got == want  # tactics, scores (exact floats) and the de-duplication order
    assert got[4] == got[0]
    assert asyncio.run(hf.batch_generate(states[:2], paths[:2], names[:2], poses[:2], 8)) == want[:2]
    # retrieval-augmented: retrieve per state, then one batched generate
    d = tempfile.mkdtemp()
    rcfg = synth.t5_config("tiny")
    ret_dir = os.path.join(d, "ret")
    os.makedirs(ret_dir)
    json.dump({k: rcfg[k] for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                    "relative_attention_num_buckets", "relative_attention_max_distance",
                                    "layer_norm_epsilon", "feed_forward_proj")}, open(os.path.join(ret_dir, "config.json"), "w"))
    save_file({k: v.clone().contiguous() for k, v in synth.synth_state_dict(rcfg).items()
               if k != "encoder.embed_tokens.weight"}, os.path.join(ret_dir, "model.safetensors"))
    files = synth.synth_corpus_records(10, 200, seed=31, max_imports=4)
    cpath = os.path.join(d, "corpus.jsonl")
    synth.write_corpus_jsonl(cpath, files)
    ipath = os.path.join(d, "indexed.pickle")
    index_cli.main(["--ckpt_path", ret_dir, "--corpus-path", cpath, "--output-path", ipath, "--batch-size", "32"])
    rag = RetrievalAugmentedGenerator(gdir, ret_dir, ipath, DEV, max_inp_seq_len=512, max_oup_seq_len=32,
                                      length_penalty=0.0, max_num_retrieved=20)
    rag.initialize()
    fpaths = [files[5]["path"], files[7]["path"], files[5]["path"]]
    fposes = [Pos(150, 0), Pos(90, 0), Pos(20, 0)]
    got = rag.batch_generate_sync(states[:3], fpaths, names[:3], fposes, 4)
    want = [rag.generate_sync(s, p, "thm", q, 4) for s, p, q in zip(states[:3], fpaths, fposes)]
    assert got == want
    assert asyncio.run(rag.batch_generate(states[:3], fpaths, names[:3], fposes, 4)) == want


# ---- ABI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,S", [(1, 1), (3, 257), (64, 300)])
def test_per_state_entry_points_are_the_one_state_batched_call(tiny_gen, nb, S):
    """Through the C ABI: rp_decoder_cross_kv + rp_decoder_step on one zero-filled workspace, rp_decoder_batch_cross_kv +
    rp_decoder_batch_step (n = 1, active = {0}) on another.  After every step the log-probs and the whole workspaces are
    equal byte for byte, and rp_beam_select / rp_beam_select_batch(n_active = 1) pick the same candidates.  nb = 1 and 3:
    the row / nb arithmetic and a merge that is no power of two; nb = 64 with k = 128 fills the merge; S = 257 crosses
    one 256-thread trip of the attention loops."""
    z, cfg, sd, gen = tiny_gen
    lib = _lib.load()
    h = gen.decoder._handle
    C = _lib.C
    T, V, k = 3, cfg["vocab_size"], 2 * nb
    enc = gen.encode_hidden(source_ids(S, 70 + nb))
    cu = np.array([0, S], dtype=np.int32)
    act = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    need = lib.rp_decoder_workspace_bytes(h, nb, T, S)
    assert need > 0 and need == lib.rp_decoder_batch_workspace_bytes(h, p(cu), 1, nb, T)
    ws1 = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ws2 = torch.zeros(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rp_decoder_cross_kv(h, enc.data_ptr(), S, nb, T, ws1.data_ptr(), need, None), "rp_decoder_cross_kv")
    _lib.check(lib.rp_decoder_batch_cross_kv(h, enc.data_ptr(), p(cu), 1, nb, T, ws2.data_ptr(), need, None),
               "rp_decoder_batch_cross_kv")
    assert torch.equal(ws1, ws2)
    sel_need = nb * min(k, V) * 8
    sel_ws = torch.empty(sel_need, dtype=torch.uint8, device=DEV)
    run = torch.randn(nb, generator=torch.Generator().manual_seed(nb)).to(DEV)
    new = lambda dt: torch.empty(k, dtype=dt, device=DEV)  # noqa: E731
    for t, tok, anc in simulated_search(nb, T, seed=80 + nb):
        tok, anc = tok.to(DEV, torch.int32), anc.to(DEV, torch.int32).contiguous()
        lp1 = torch.empty((nb, V), dtype=torch.float32, device=DEV)
        lp2 = torch.empty_like(lp1)
        _lib.check(lib.rp_decoder_step(h, tok.data_ptr(), anc.data_ptr(), t + 1, nb, t, T, S, lp1.data_ptr(),
                                       ws1.data_ptr(), need, None), "rp_decoder_step")
        _lib.check(lib.rp_decoder_batch_step(h, p(cu), 1, p(act), 1, tok.data_ptr(), anc.data_ptr(), t + 1, nb, t, T,
                                             lp2.data_ptr(), ws2.data_ptr(), need, None), "rp_decoder_batch_step")
        assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)), t
        assert torch.equal(ws1, ws2), t
        s1, t1, p1, s2, t2, p2 = new(torch.float32), new(torch.int32), new(torch.int32), new(torch.float32), \
            new(torch.int32), new(torch.int32)
        # the two select workspace requirements are the same number: both take sel_need bytes and refuse one fewer
        assert lib.rp_beam_select(lp1.data_ptr(), run.data_ptr(), nb, V, k, s1.data_ptr(), t1.data_ptr(), p1.data_ptr(),
                                  sel_ws.data_ptr(), sel_need - 1, None) == -3
        assert lib.rp_beam_select_batch(lp2.data_ptr(), run.data_ptr(), 1, nb, V, k, s2.data_ptr(), t2.data_ptr(),
                                        p2.data_ptr(), sel_ws.data_ptr(), sel_need - 1, None) == -3
        _lib.check(lib.rp_beam_select(lp1.data_ptr(), run.data_ptr(), nb, V, k, s1.data_ptr(), t1.data_ptr(),
                                      p1.data_ptr(), sel_ws.data_ptr(), sel_need, None), "rp_beam_select")
        _lib.check(lib.rp_beam_select_batch(lp2.data_ptr(), run.data_ptr(), 1, nb, V, k, s2.data_ptr(), t2.data_ptr(),
                                            p2.data_ptr(), sel_ws.data_ptr(), sel_need, None), "rp_beam_select_batch")
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(t1, t2) and torch.equal(p1, p2)
        assert torch.isfinite(lp1).all() and int(p1.max()) < nb  # a real step ran, not two empty buffers


def test_batch_argument_errors_carry_messages(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    lib = _lib.load()
    h = gen.decoder._handle
    C = _lib.C
    err = lambda: lib.rp_last_error()  # noqa: E731
    cu = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ws = torch.empty(1, dtype=torch.uint8, device=DEV)
    d = ws.data_ptr()
    ok = cu(0, 8, 16)
    act = cu(0, 1)
    assert lib.rp_decoder_batch_workspace_bytes(h, p(ok), 2, 4, 8) > 0
    # zero states
    assert lib.rp_decoder_batch_workspace_bytes(h, p(ok), 0, 4, 8) == 0 and b"states=0" in err()
    assert lib.rp_decoder_batch_cross_kv(h, d, p(ok), 0, 4, 8, d, 1, None) == -1 and b"states=0" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 0, d, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"active states=0" in err()
    assert lib.rp_beam_select_batch(d, d, 0, 4, 384, 8, d, d, d, d, 1, None) == -1 and b"states=0" in err()
    # too many states, rows over the cap (17 states of 64 beams = 1088 rows), 65 beams
    big = np.arange(34, dtype=np.int32)
    assert lib.rp_decoder_batch_workspace_bytes(h, p(big), 33, 4, 8) == 0 and b"states=33" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, p(big), 17, 64, 8) == 0 and b"rows" in err() and b"1088" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, p(big), 16, 64, 8) > 0
    assert lib.rp_decoder_batch_workspace_bytes(h, p(ok), 2, 65, 8) == 0 and b"num_beams=65" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 2, d, d, 1, 65, 0, 8, d, d, 1, None) == -1 and b"num_beams" in err()
    assert lib.rp_beam_select_batch(d, d, 2, 65, 384, 8, d, d, d, d, 1, None) == -1 and b"nb=65" in err()
    assert lib.rp_beam_select_batch(d, d, 2, 4, 384, 129, d, d, d, d, 1, None) == -1 and b"k=" in err()
    assert lib.rp_beam_select_batch(d, d, 2, 4, 513, 8, d, d, d, d, 1, None) == -1 and b"vocab" in err()
    # source lengths and max_len
    assert lib.rp_decoder_batch_workspace_bytes(h, p(cu(0, 8, 8)), 2, 4, 8) == 0 and b"src_len of state 1" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, p(cu(0, 8193, 8200)), 2, 4, 8) == 0 and b"src_len of state 0" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, p(cu(1, 8, 16)), 2, 4, 8) == 0 and b"src_cu[0]" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, p(ok), 2, 4, 8193) == 0 and b"max_len" in err()
    # a short workspace
    assert lib.rp_decoder_batch_cross_kv(h, d, p(ok), 2, 4, 8, d, 1, None) == -3 and b"workspace" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 2, d, d, 1, 4, 0, 8, d, d, 1, None) == -3 and b"workspace" in err()
    assert lib.rp_beam_select_batch(d, d, 2, 4, 384, 8, d, d, d, d, 1, None) == -3 and b"workspace" in err()
    # null arguments
    assert lib.rp_decoder_batch_workspace_bytes(None, p(ok), 2, 4, 8) == 0 and b"null" in err()
    assert lib.rp_decoder_batch_workspace_bytes(h, None, 2, 4, 8) == 0 and b"null" in err()
    assert lib.rp_decoder_batch_cross_kv(h, None, p(ok), 2, 4, 8, d, 1, None) == -1 and b"null" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, None, 2, d, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"null" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 2, None, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"null" in err()
    assert lib.rp_beam_select_batch(None, d, 2, 4, 384, 8, d, d, d, d, 1, None) == -1 and b"null" in err()
    # the step's position, ancestry stride and active list
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 2, d, d, 2, 4, 3, 8, d, d, 1, None) == -1 and b"anc_stride" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 2, d, d, 9, 4, 8, 8, d, d, 1, None) == -1 and b"t=8" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(act), 3, d, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"active states=3" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(cu(0, 2)), 2, d, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"active[1]=2" in err()
    assert lib.rp_decoder_batch_step(h, p(ok), 2, p(cu(1, 1)), 2, d, d, 1, 4, 0, 8, d, d, 1, None) == -1 and b"twice" in err()
    # the host layer: too many beams, no sources
    with pytest.raises(_lib.HipLibraryError, match="num_beams=65"):
        gen.generate_many([z["src"]], 65, 8, 1.0)
    with pytest.raises(ValueError):
        gen.generate_many([], 4, 8, 1.0)
    # the per-state entry points keep their limits
    assert lib.rp_decoder_workspace_bytes(h, 65, 8, 8) == 0
