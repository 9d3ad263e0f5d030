"""Tactic generator on the MI355X: rp_encode_hidden, the decoder step (G19 parity, same bits, ancestry reorder), the
device beam selection, generate against HF (G20), the prover-shaped run and RetrievalAugmentedGenerator end to end."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import t5_ref  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402
from reprover_amd.generation import topk_select  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g20_weights(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    return z, meta, cfg, sd


@pytest.fixture(scope="module")
def tiny_gen(golden_dir):
    z, meta, cfg, sd = _g20_weights(golden_dir)
    return z, meta, cfg, sd, HipT5Generator(cfg, sd, DEV)


def _teacher_forced(gen, enc, target):
    T = len(target)
    gen.decoder.start(enc, 1, T)
    out = []
    for t in range(T):
        anc = torch.arange(t + 1, dtype=torch.int64)[None]
        out.append(gen.decoder.step(torch.tensor([int(target[t])]), anc).clone())
    return torch.cat(out).cpu()


def test_encode_hidden_matches_fp32_and_pool_unchanged(tiny_gen):
    z, meta, cfg, sd, gen = tiny_gen
    src = z["src"]
    cu = np.array([0, len(src)], dtype=np.int32)
    pooled0 = gen.encoder.encode_packed(src, cu).clone()
    hid = gen.encode_hidden(src).float().cpu()
    pooled1 = gen.encoder.encode_packed(src, cu).clone()
    assert torch.equal(pooled0, pooled1)
    ref = t5_ref._encoder_forward(cfg, sd, src[None].astype(np.int64), np.ones((1, len(src)), np.int64))[0]
    cos = torch.nn.functional.cosine_similarity(hid, ref, dim=1)
    assert cos.min() > 0.999, cos.min()
    pool = torch.nn.functional.normalize(hid.mean(0), dim=0)
    assert torch.nn.functional.cosine_similarity(pool, pooled0.float().cpu()[0], dim=0) > 0.999


@pytest.mark.parametrize("key", ["tiny_0", "tiny_1", "byt5-small_0"])
def test_decode_step_no_worse_than_hf_bf16(golden_dir, key):
    g = np.load(os.path.join(golden_dir, "g19_decoder_step.npz"))
    name = key.rsplit("_", 1)[0]
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg)
    gen = HipT5Generator(cfg, sd, DEV)
    enc = gen.encode_hidden(g[f"{key}_src"])
    lp = _teacher_forced(gen, enc, g[f"{key}_tgt"]).numpy()
    lp32, lp16 = g[f"{key}_lp32"], g[f"{key}_lp16"]
    err, err_hf = np.abs(lp - lp32), np.abs(lp16 - lp32)
    # metric style of oracle/parity_margins.py: max and rms error against the fp32 reference, HF-bf16 beside it
    assert err.max() <= err_hf.max(), (err.max(), err_hf.max())
    assert np.sqrt((err ** 2).mean()) <= np.sqrt((err_hf ** 2).mean())


def test_same_bits_batched_permuted_and_reordered(tiny_gen):
    """A row's log-probs are the same bits alone, batched, permuted, and read through a reordered ancestry table (no
    cache row moved) as through a cache that holds each beam's history in place (an explicit gather)."""
    z, meta, cfg, sd, gen = tiny_gen
    enc = gen.encode_hidden(z["src"])
    rng = np.random.default_rng(5)
    nb, T = 4, 6
    hist = rng.integers(3, 259, size=(nb, T))
    hist[:, 0] = 0
    # 1. in place: beam b's history in its own rows, identity ancestry
    gen.decoder.start(enc, nb, T)
    for t in range(T):
        anc = (torch.arange(t + 1)[None, :] * nb + torch.arange(nb)[:, None]).long()
        ref = gen.decoder.step(torch.from_numpy(hist[:, t]), anc).clone().cpu()
    # 2. each beam alone
    for b in range(nb):
        gen.decoder.start(enc, 1, T)
        for t in range(T):
            one = gen.decoder.step(torch.tensor([int(hist[b, t])]), torch.arange(t + 1)[None].long()).clone().cpu()
        assert torch.equal(one[0], ref[b])
    # 3. permuted rows: row p carries beam perm[p]
    perm = np.array([2, 0, 3, 1])
    gen.decoder.start(enc, nb, T)
    for t in range(T):
        anc = (torch.arange(t + 1)[None, :] * nb + torch.arange(nb)[:, None]).long()
        got = gen.decoder.step(torch.from_numpy(hist[perm, t]), anc).clone().cpu()
    assert torch.equal(got, ref[perm])
    # 4. ancestry reorder: at step t slot s (row t * nb + s) takes the token of beam owner[t][s]; the table points each
    # slot at the rows of its beam's history, wherever earlier steps wrote them
    gen.decoder.start(enc, nb, T)
    owner = [rng.permutation(nb) for _ in range(T)]
    inv = [np.argsort(o) for o in owner]
    for t in range(T):
        anc = torch.tensor([[p * nb + inv[p][owner[t][s]] for p in range(t + 1)] for s in range(nb)]).long()
        lp = gen.decoder.step(torch.from_numpy(hist[owner[t], t]), anc).clone().cpu()
    assert torch.equal(lp, ref[owner[T - 1]])


def test_device_select_matches_torch_topk():
    lib = _lib.load()
    assert lib.rp_abi_version() == _lib.ABI_VERSION == 7
    from reprover_amd.decoder import HipT5Decoder

    g = torch.Generator().manual_seed(3)
    for nb in (1, 4, 64):
        lp = torch.log_softmax(torch.randn(nb, 384, generator=g) * 3, -1)
        lp[0, 7] = lp[0, 9] = lp[0].max() + 1  # an exact tie: the lower index first
        run = torch.randn(nb, generator=g)
        if nb > 1:
            run[1:] = -1e9
        dec = HipT5Decoder.__new__(HipT5Decoder)
        dec._lib, dec._sel_ws, dec.device = lib, None, torch.device(DEV)
        s, t, p = dec.select(lp.to(DEV), run.to(DEV), 2 * nb)
        # the stated order: descending score, ties to the lower flat index (a stable sort; CPU torch.topk itself does
        # not promise an order among exact ties)
        acc = (lp + run[:, None]).reshape(-1)
        rs, ri = torch.sort(acc, descending=True, stable=True)
        rs, ri = rs[: 2 * nb], ri[: 2 * nb]
        rt, rp = ri % 384, ri // 384
        vals, _, _ = topk_select(lp, run, 2 * nb)
        assert torch.equal(vals, rs)
        assert torch.equal(s.cpu(), rs) and torch.equal(t.cpu().long(), rt) and torch.equal(p.cpu().long(), rp)


def _strip(seq):
    seq = list(seq)
    if 1 in seq[1:]:
        seq = seq[: seq.index(1, 1) + 1]
    return seq


@pytest.mark.parametrize("case", range(24))
def test_generate_matches_g20_and_own_scores(tiny_gen, case):
    z, meta, cfg, sd, gen = tiny_gen
    c = meta["cases"][case]
    nb, lp_, ml = c["num_beams"], c["length_penalty"], c["max_length"]
    out = gen.generate(z["src"], nb, ml, lp_)
    if c["bf16_agrees"]:
        assert np.array_equal(out.sequences.numpy(), z[f"c{case}_seq"])
    enc = gen.encode_hidden(z["src"])
    for j in range(min(nb, 8)):
        seq = _strip(out.sequences[j].tolist())
        tf = _teacher_forced(gen, enc, np.array(seq[:-1]))
        total = float(sum(tf[i, seq[i + 1]] for i in range(len(seq) - 1)))
        expect = total / ((len(seq) - 1) ** lp_)
        assert abs(expect - float(out.sequences_scores[j])) <= 1e-4 * max(1.0, abs(expect)), (j, expect, out.sequences_scores[j])


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


def test_prover_shaped_run_and_retrieval_augmented_generator():
    """ByT5-small dims, 64 beams, a 2048-byte source, max_length 512 through RetrievalAugmentedGenerator."""
    from reprover_amd.prover.tactic_generator import RetrievalAugmentedGenerator
    from reprover_amd.retrieval import index as index_cli

    d = tempfile.mkdtemp()
    cfg = synth.seq2seq_config("byt5-small")
    gen_dir = os.path.join(d, "gen")
    _save_generator_dir(gen_dir, cfg, synth.synth_seq2seq_state_dict(cfg))
    rcfg = synth.t5_config("tiny")
    rsd = synth.synth_state_dict(rcfg)
    ret_dir = os.path.join(d, "ret")
    os.makedirs(ret_dir)
    json.dump({k: rcfg[k] for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                    "relative_attention_num_buckets", "relative_attention_max_distance",
                                    "layer_norm_epsilon", "feed_forward_proj")}, open(os.path.join(ret_dir, "config.json"), "w"))
    save_file({k: v.clone().contiguous() for k, v in rsd.items() if k != "encoder.embed_tokens.weight"},
              os.path.join(ret_dir, "model.safetensors"))
    files = synth.synth_corpus_records(10, 200, seed=31, max_imports=4)
    cpath = os.path.join(d, "corpus.jsonl")
    synth.write_corpus_jsonl(cpath, files)
    ipath = os.path.join(d, "indexed.pickle")
    index_cli.main(["--ckpt_path", ret_dir, "--corpus-path", cpath, "--output-path", ipath, "--batch-size", "32"])
    rag = RetrievalAugmentedGenerator(gen_dir, ret_dir, ipath, DEV, max_inp_seq_len=2048, max_oup_seq_len=512,
                                      length_penalty=0.0, max_num_retrieved=100)
    rag.initialize()
    state = synth.synth_state(np.random.default_rng(7), 2400)  # with the premises: truncated to 2048 bytes
    trace = []
    import asyncio

    g = rag.hf_gen.generator
    orig = g.generate
    g.generate = lambda *a, **k: orig(*a, trace=trace, **k)
    res = asyncio.run(rag.generate(state, files[5]["path"], "thm", Pos(150, 0), 64))
    assert 1 <= len(res) <= 64 and len({t for t, _ in res}) == len(res)
    assert all(isinstance(t, str) and isinstance(s, float) for t, s in res)
    assert all(a >= b for (_, a), (_, b) in zip(res, res[1:]))
    assert len(trace) <= 511
    g.generate = orig


def test_decoder_only_checkpoint_is_refused(tmp_path):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    json.dump({"model_type": "gpt2", "is_encoder_decoder": False}, open(tmp_path / "config.json", "w"))
    g = HuggingFaceGenerator(str(tmp_path), DEV, 2048, 512, 0.0)
    with pytest.raises(ValueError, match="decoder-only"):
        g.initialize()


def test_argument_errors_carry_messages(tiny_gen):
    z, meta, cfg, sd, gen = tiny_gen
    lib = _lib.load()
    h = gen.decoder._handle
    assert lib.rp_decoder_workspace_bytes(h, 65, 8, 8) == 0
    ws = torch.empty(1, dtype=torch.uint8, device=DEV)
    st = lib.rp_decoder_cross_kv(h, ws.data_ptr(), 8, 4, 8, ws.data_ptr(), 1, None)
    assert st == -3 and b"workspace" in lib.rp_last_error()
    st = lib.rp_decoder_step(h, ws.data_ptr(), ws.data_ptr(), 1, 65, 0, 8, 8, ws.data_ptr(), ws.data_ptr(), 1, None)
    assert st == -1 and b"num_beams" in lib.rp_last_error()
    st = lib.rp_decoder_step(h, ws.data_ptr(), ws.data_ptr(), 2, 4, 3, 8, 8, ws.data_ptr(), ws.data_ptr(), 1, None)
    assert st == -1 and b"anc_stride" in lib.rp_last_error()
    st = lib.rp_beam_select(ws.data_ptr(), ws.data_ptr(), 4, 384, 129, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(),
                            ws.data_ptr(), 1, None)
    assert st == -1 and b"k=" in lib.rp_last_error()
    with pytest.raises(_lib.HipLibraryError):
        gen.generate(z["src"], 65, 8, 1.0)
