"""Generate the tactic-generator fixtures G18 - G21 with HuggingFace transformers on CPU.

Authoring container only; only the resulting data files are committed.  Usage:
    python tests/golden/make_golden_generate.py [g18 g19 g20 g21]   (default: all)

G18  unidirectional relative-position buckets (T5Attention._relative_position_bucket(bidirectional=False)) over
     key - query in [-2200, 0], and ByT5Tokenizer.batch_decode(skip_special_tokens=True) cases.
G19  teacher-forced decoder log-probs of T5ForConditionalGeneration in fp32 and bf16 along fixed targets, for the tiny
     and the ByT5-small-shaped synthetic seq2seq weights (synth.synth_seq2seq_state_dict, HF init scales).
G20  generate(num_beams, num_return_sequences=num_beams, length_penalty, max_length, early_stopping=False,
     do_sample=False) in fp32 and bf16 over a grid, with the per-step top-2nb candidates of the fp32 run.
G21  teacher-forced fp32 decoder log-probs for three tiny models: (a) the sharp family (synth_seq2seq_state_dict
     scale="sharp") along a 520-position target, (b) tiny-tied at HF scale, (c) a transformers-5-style checkpoint:
     lm_head = shared, scale_decoder_outputs=False.  Stored: the log-prob of the next target token at every position, and
     full rows at a few positions (self-attention bucket edges, the 256-key boundaries of the attention kernel).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from transformers import ByT5Tokenizer, T5Config, T5ForConditionalGeneration  # noqa: E402
from transformers.models.t5.modeling_t5 import T5Attention  # noqa: E402

from reprover_amd import synth  # noqa: E402

OUT = HERE
G20_SOURCE_BYTES = 300
G20_EOS_BOOST = 1.6  # lm_head's EOS row scaled so that some grid points finish on EOS before max_length
G20_GRID = [(nb, lp, ml) for nb in (1, 4, 8, 64) for lp in (0.0, 1.0, -0.5) for ml in (6, 20)]


def hf_model(cfg, sd, dtype=torch.float32, scale_decoder_outputs=None):
    c = T5Config(vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"],
                 num_layers=cfg["num_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
                 feed_forward_proj="gated-gelu", tie_word_embeddings=cfg["tie_word_embeddings"], dropout_rate=0.0,
                 decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    m = T5ForConditionalGeneration(c).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("embed_tokens" in k or k == "lm_head.weight" for k in missing), missing
    # transformers 5 forces tie_word_embeddings=True on T5Config and keeps the flag's old meaning in
    # scale_decoder_outputs; an untied checkpoint (ByT5's) gets its own lm_head back here.
    if not cfg["tie_word_embeddings"]:
        m.lm_head.weight = torch.nn.Parameter(sd["lm_head.weight"].clone())
    with torch.no_grad():
        m.shared.weight.copy_(sd["shared.weight"])
    assert m.encoder.embed_tokens.weight is m.shared.weight and m.decoder.embed_tokens.weight is m.shared.weight
    m.config.scale_decoder_outputs = bool(cfg["tie_word_embeddings"] if scale_decoder_outputs is None
                                          else scale_decoder_outputs)
    return m.to(dtype)


def source_ids(n_bytes, seed):
    rng = np.random.default_rng(seed)
    text = synth.synth_text(rng, n_bytes)
    ids = np.frombuffer(text.encode("utf-8"), dtype=np.uint8).astype(np.int64) + 3
    return np.concatenate([ids[: n_bytes - 1], [1]]), text


def g18():
    d = torch.arange(-2200, 1, dtype=torch.long)
    b = T5Attention._relative_position_bucket(d, bidirectional=False, num_buckets=32, max_distance=128).numpy()
    np.savez_compressed(os.path.join(OUT, "g18_buckets_causal.npz"), rel=d.numpy().astype(np.int32),
                        bucket=b.astype(np.int8))
    tok = ByT5Tokenizer()
    rng = np.random.default_rng(18)
    cases = [
        [0, 3 + ord("a"), 3 + ord("b"), 1, 0, 0],
        list(np.array(list("exact".encode())) + 3) + [1],
        [3 + c for c in "∀ n : ℕ, n = n".encode()] + [1],
        [3 + c for c in "→ ⊢".encode()][:-1] + [1],  # a truncated 3-byte sequence: dropped by errors="ignore"
        [3 + 0xFF, 3 + ord("x"), 3 + 0xC3, 1],  # invalid UTF-8 bytes
        [259, 3 + ord("y"), 383, 300, 2, 1],  # extra ids and unk
        [0, 0, 0],
        [],
    ]
    for _ in range(8):
        cases.append(rng.integers(0, 384, size=int(rng.integers(1, 40))).tolist())
    cases = [[int(x) for x in c] for c in cases]
    out = tok.batch_decode(cases, skip_special_tokens=True)
    with open(os.path.join(OUT, "g18_decode.json"), "w") as fh:
        json.dump({"ids": cases, "text": out}, fh, ensure_ascii=False, indent=0)
    print("g18 ok:", len(d), "offsets,", len(cases), "decode cases")


def g19():
    arrays = {}
    for name, src_bytes, tlen in (("tiny", (300, 700), 48), ("byt5-small", (2048,), 24)):
        cfg = synth.seq2seq_config(name)
        sd = synth.synth_seq2seq_state_dict(cfg)
        m32, m16 = hf_model(cfg, sd), hf_model(cfg, sd, torch.bfloat16)
        rng = np.random.default_rng(19)
        for j, n in enumerate(src_bytes):
            src, _ = source_ids(n, 190 + j)
            tgt = np.concatenate([[0], rng.integers(3, 259, size=tlen - 1)]).astype(np.int64)
            with torch.no_grad():
                inp = torch.from_numpy(src)[None]
                dec = torch.from_numpy(tgt)[None]
                l32 = torch.log_softmax(m32(input_ids=inp, decoder_input_ids=dec).logits[0].float(), -1)
                l16 = torch.log_softmax(m16(input_ids=inp, decoder_input_ids=dec).logits[0].float(), -1)
            key = f"{name}_{j}"
            arrays[f"{key}_src"] = src.astype(np.int32)
            arrays[f"{key}_tgt"] = tgt.astype(np.int32)
            arrays[f"{key}_lp32"] = l32.numpy().astype(np.float32)
            arrays[f"{key}_lp16"] = l16.numpy().astype(np.float32)
            print(f"g19 {key}: src {n} bytes, target {tlen}, max |bf16 - fp32| {float((l16 - l32).abs().max()):.3e}")
    np.savez_compressed(os.path.join(OUT, "g19_decoder_step.npz"), **arrays)


def g20_weights():
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= G20_EOS_BOOST
    return cfg, sd


def g20():
    from reprover_amd.generation import beam_search
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gen_helpers import T5Fp32

    cfg, sd = g20_weights()
    m32, m16 = hf_model(cfg, sd), hf_model(cfg, sd, torch.bfloat16)
    src, _ = source_ids(G20_SOURCE_BYTES, 20)
    inp = torch.from_numpy(src)[None]
    arrays = {"src": src.astype(np.int32)}
    meta = []
    ref = T5Fp32(cfg, sd)
    enc = ref.encode(src)
    for ci, (nb, lp, ml) in enumerate(G20_GRID):
        kw = dict(num_beams=nb, num_return_sequences=nb, length_penalty=lp, max_length=ml, early_stopping=False,
                  do_sample=False, return_dict_in_generate=True, output_scores=True)
        with torch.no_grad():
            o32 = m32.generate(inp, **kw)
            o16 = m16.generate(inp, **kw)
        s32 = o32.sequences.numpy()
        sc32 = (o32.sequences_scores.numpy() if nb > 1 else np.zeros(1, np.float32))
        agree = s32.shape == o16.sequences.shape and bool((o16.sequences.numpy() == s32).all())
        arrays[f"c{ci}_seq"] = s32.astype(np.int32)
        arrays[f"c{ci}_score"] = sc32.astype(np.float32)
        # the driver over the fp32 restatement: the per-step candidates, and a cross-check while generating
        trace = []
        ref.start(enc, nb, ml)
        mine = beam_search(ref.step, nb, ml, lp, trace=trace)
        assert mine.sequences.shape == s32.shape and (mine.sequences.numpy() == s32).all(), (ci, mine.sequences, s32)
        if nb > 1:
            assert np.allclose(mine.sequences_scores.numpy(), sc32, rtol=1e-5, atol=1e-5), (ci, mine.sequences_scores, sc32)
        arrays[f"c{ci}_trace_score"] = np.stack([t[0].numpy() for t in trace]).astype(np.float32)
        arrays[f"c{ci}_trace_token"] = np.stack([t[1].numpy() for t in trace]).astype(np.int16)
        arrays[f"c{ci}_trace_parent"] = np.stack([t[2].numpy() for t in trace]).astype(np.int16)
        n_eos = int((s32[:, 1:] == 1).any(1).sum())
        meta.append(dict(num_beams=nb, length_penalty=lp, max_length=ml, bf16_agrees=agree, steps=len(trace),
                         n_finished_on_eos=n_eos))
        print(f"g20 case {ci}: nb={nb} lp={lp} max_length={ml} -> {s32.shape}, eos-finished {n_eos}, bf16 agrees {agree}")
    arrays["meta"] = np.frombuffer(json.dumps(dict(cases=meta, eos_boost=G20_EOS_BOOST,
                                                   source_bytes=G20_SOURCE_BYTES)).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "g20_generate.npz"), **arrays)


# name -> (seq2seq config, weight scale, scale_decoder_outputs, source bytes, target positions, full-row positions)
G21_MODELS = {
    "a": ("tiny", "sharp", False, 300, 520,
          [0, 1, 2, 15, 16, 17, 31, 32, 63, 64, 100, 127, 128, 129, 200, 255, 256, 257, 258, 300, 400, 510, 511, 519]),
    "b": ("tiny-tied", "hf", True, 200, 160, [0, 15, 16, 17, 127, 128, 129, 159]),
    "c": ("tiny-tied", "hf", False, 200, 160, [0, 15, 16, 17, 127, 128, 129, 159]),
}


def g21():
    arrays, meta = {}, {}
    for name, (cname, scale, sdo, n_src, T, rows) in G21_MODELS.items():
        cfg = synth.seq2seq_config(cname)
        sd = synth.synth_seq2seq_state_dict(cfg, scale=scale)
        m = hf_model(cfg, sd, scale_decoder_outputs=sdo)
        src, _ = source_ids(n_src, 210 + ord(name))
        rng = np.random.default_rng(21 + ord(name))
        tgt = np.concatenate([[0], rng.integers(3, 259, size=T)]).astype(np.int64)  # inputs tgt[:T], labels tgt[1:]
        with torch.no_grad():
            lp = torch.log_softmax(m(input_ids=torch.from_numpy(src)[None],
                                     decoder_input_ids=torch.from_numpy(tgt[:T])[None]).logits[0].float(), -1)
        arrays[f"{name}_src"] = src.astype(np.int32)
        arrays[f"{name}_tgt"] = tgt.astype(np.int32)
        arrays[f"{name}_lp_label"] = lp[torch.arange(T), torch.from_numpy(tgt[1:])].numpy().astype(np.float32)
        arrays[f"{name}_rows"] = np.array(rows, dtype=np.int32)
        arrays[f"{name}_lp_rows"] = lp[rows].numpy().astype(np.float32)
        meta[name] = dict(config=cname, scale=scale, scale_decoder_outputs=sdo, source_bytes=n_src, positions=T)
        print(f"g21 {name}: {cname} {scale} scale_decoder_outputs={sdo}, src {n_src}, positions {T}, "
              f"label lp range [{float(arrays[f'{name}_lp_label'].min()):.2f}, {float(arrays[f'{name}_lp_label'].max()):.2f}]")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "g21_decoder_long.npz"), **arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    for name in sys.argv[1:] or ["g18", "g19", "g20", "g21"]:
        {"g18": g18, "g19": g19, "g20": g20, "g21": g21}[name]()
