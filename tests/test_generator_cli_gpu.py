"""End to end: ``reprover_amd.generator.main validate`` on a synthetic split, a synthetic seq2seq checkpoint directory and
a ``predictions.pickle`` written by ``reprover_amd.retrieval.main predict``.  The printed ``loss_val`` is the batch-size
weighted mean of per-batch ``forward`` and every ``top{k}_acc_val`` is TopkAccuracy over the engine's own generations."""
import json
import os

import numpy as np
import pytest
import yaml
from safetensors.torch import save_file

from reprover_amd import synth
from reprover_amd.common import Corpus, Pos
from reprover_amd.decoder import HipT5Generator
from reprover_amd.generator import main as gen_main
from reprover_amd.generator.datamodule import GeneratorDataModule
from reprover_amd.generator.model import TopkAccuracy
from reprover_amd.retrieval import main as ret_main
from reprover_amd.tokenizer import batch_decode

pytestmark = pytest.mark.gpu
KEYS = ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers", "relative_attention_num_buckets",
        "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj")


def _ckpt(path, cfg, sd, extra):
    os.makedirs(path)
    json.dump(dict({k: cfg[k] for k in KEYS if k in cfg}, **extra), open(os.path.join(path, "config.json"), "w"))
    save_file({k: v.clone().contiguous() for k, v in sd.items() if "embed_tokens" not in k},
              os.path.join(path, "model.safetensors"))


def test_generator_validate_end_to_end(tmp_path, capsys):
    d = str(tmp_path)
    files = synth.synth_corpus_records(30, 500, seed=91, max_imports=6)
    cpath = os.path.join(d, "corpus.jsonl")
    synth.write_corpus_jsonl(cpath, files)
    corpus = Corpus(cpath)
    enough = lambda path, start: corpus.accessible_mask(path, Pos(*start)).sum() >= 12  # noqa: E731
    sdir = os.path.join(d, "split")
    os.makedirs(sdir)
    for name, n, seed in (("train", 4, 92), ("val", 6, 93), ("test", 3, 94)):
        json.dump(synth.synth_split(files, n, seed=seed, min_file=15, accept=enough), open(os.path.join(sdir, f"{name}.json"), "w"))
    # retriever checkpoint + predictions.pickle
    rcfg = synth.t5_config("tiny")
    _ckpt(os.path.join(d, "ret"), dict(rcfg, feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
                                       relative_attention_max_distance=128, layer_norm_epsilon=1e-6),
          synth.synth_state_dict(rcfg), {})
    rconf = {"model": {"model_name": os.path.join(d, "ret"), "num_retrieved": 10},
             "data": {"data_path": sdir, "corpus_path": cpath, "eval_batch_size": 16, "max_seq_len": 256}}
    yaml.safe_dump(rconf, open(os.path.join(d, "ret.yaml"), "w"))
    ret_main.main(["predict", "--config", os.path.join(d, "ret.yaml"), "--log-dir", os.path.join(d, "logs")])
    preds_path = os.path.join(d, "logs", "predictions.pickle")
    # seq2seq checkpoint + the reference's generation config layout
    gcfg = synth.seq2seq_config("tiny")
    gsd = synth.synth_seq2seq_state_dict(gcfg, scale="sharp")
    gdir = os.path.join(d, "gen")
    _ckpt(gdir, dict(gcfg, feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
                     relative_attention_max_distance=128, layer_norm_epsilon=1e-6),
          gsd, dict(model_type="t5", is_encoder_decoder=True, decoder_start_token_id=0, eos_token_id=1,
                    num_decoder_layers=gcfg["num_decoder_layers"], tie_word_embeddings=False))
    for num_beams in (1, 2):
        conf = {"model": {"model_name": gdir, "lr": 5e-4, "warmup_steps": 2000, "num_beams": num_beams, "length_penalty": 0.0,
                          "ret_ckpt_path": None, "eval_num_retrieved": 100, "eval_num_workers": 1, "eval_num_gpus": 1,
                          "eval_num_theorems": 250},
                "data": {"data_path": sdir, "corpus_path": cpath, "preds_path": preds_path, "batch_size": 8,
                         "eval_batch_size": 4, "max_inp_seq_len": 600, "max_oup_seq_len": 12, "p_drop": 0.5,
                         "num_workers": 2}}
        yaml.safe_dump(conf, open(os.path.join(d, "gen.yaml"), "w"))
        capsys.readouterr()
        gen_main.main(["validate", "--config", os.path.join(d, "gen.yaml"), "--limit-batches", "2"])
        out = capsys.readouterr().out
        printed = dict(line.split(": ", 1) for line in out.splitlines() if line.startswith(("loss_val", "top")))
        assert "Pass@1" in out and "skipped" in out
        # independently: the engine's forward and generate over the same batches
        dm = GeneratorDataModule(sdir, gdir, 8, 4, 600, 12, 0.5, 0, cpath, preds_path)
        dm.setup("validate")
        gen = HipT5Generator.from_pretrained(gdir, "cuda:0")
        losses, sizes, accs = [], [], {k: TopkAccuracy(k) for k in range(1, num_beams + 1)}
        for i, batch in enumerate(dm.val_dataloader()):
            if i == 2:
                break
            assert all("\n\n" in s for s in batch["state"])  # retrieved premises in front of every state
            losses.append(gen.forward(batch["state_ids"], batch["state_mask"], batch["tactic_ids"]))
            sizes.append(len(batch["state"]))
            preds = []
            for b in range(len(batch["state"])):
                src = batch["state_ids"][b, : int(batch["state_mask"][b].sum())].numpy()
                seqs = (gen.greedy(src, 12) if num_beams == 1 else gen.generate(src, num_beams, 12)).sequences
                preds.append(batch_decode(seqs.tolist()))
            for acc in accs.values():
                acc.update(preds, batch["tactic"])
        loss = float(np.dot(losses, sizes) / np.sum(sizes))
        assert np.isfinite(loss) and float(printed["loss_val"]) == loss
        assert sorted(printed) == ["loss_val"] + [f"top{k}_acc_val" for k in range(1, num_beams + 1)]
        for k, acc in accs.items():
            assert float(printed[f"top{k}_acc_val"]) == acc.compute()
