"""``python -m reprover_amd.generator.main validate --config <generation yaml> [--ckpt_path DIR] [--limit-batches N]``:
the reference's generator validation (generation/main.py through Lightning's ``validate``) on the HIP engine.  It reads
the reference's ``model:`` / ``data:`` keys and prints ``loss_val`` (the epoch mean weighted by batch size) and every
``top{k}_acc_val``.  ``eval_num_theorems > 0`` asks for Pass@1 through the prover, which needs Lean: it is skipped with
a message.  ``fit`` needs the decoder backward, which is not implemented."""
from __future__ import annotations

import argparse
from typing import Dict, Optional

import yaml

from .datamodule import GeneratorDataModule
from .model import RetrievalAugmentedGenerator


def run_validate(model: RetrievalAugmentedGenerator, dm: GeneratorDataModule,
                 limit_batches: Optional[int] = None) -> Dict[str, float]:
    dm.setup("validate")
    for i, batch in enumerate(dm.val_dataloader()):
        if limit_batches is not None and i >= limit_batches:
            break
        model.validation_step(batch, i)
    return model.epoch_metrics()


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Tactic generator: validate on MI355X.")
    ap.add_argument("subcommand", choices=["fit", "validate"])
    ap.add_argument("--config", required=True, help="YAML with `model:` and `data:` sections (reference layout)")
    ap.add_argument("--ckpt_path", default=None, help="HF checkpoint dir (overrides model.model_name)")
    ap.add_argument("--limit-batches", type=int, default=None, help="validate: at most N batches")
    args = ap.parse_args(argv)
    if args.subcommand == "fit":
        raise SystemExit("generator fit needs the decoder backward (not implemented); validate is available")
    with open(args.config) as fh:
        cfg = yaml.safe_load(fh)
    m, d = cfg["model"], cfg["data"]
    model = RetrievalAugmentedGenerator(
        args.ckpt_path or m["model_name"], float(m.get("lr", 0.0)), int(m.get("warmup_steps", 0)), int(m["num_beams"]),
        int(m.get("eval_num_retrieved", 100)), int(m.get("eval_num_workers", 1)), int(m.get("eval_num_gpus", 1)),
        int(m.get("eval_num_theorems", 0)), int(d["max_inp_seq_len"]), int(d["max_oup_seq_len"]),
        float(m.get("length_penalty", 0.0)), m.get("ret_ckpt_path"))
    if model.eval_num_theorems > 0:
        print(f"eval_num_theorems={model.eval_num_theorems}: Pass@1 through the prover needs Lean; skipped", flush=True)
    dm = GeneratorDataModule(d["data_path"], m["model_name"], int(d.get("batch_size", 1)), int(d["eval_batch_size"]),
                             int(d["max_inp_seq_len"]), int(d["max_oup_seq_len"]), float(d.get("p_drop", 0.0)),
                             int(d.get("num_workers", 0)), d.get("corpus_path"), d.get("preds_path"))
    for k, v in run_validate(model, dm, args.limit_batches).items():
        print(f"{k}: {v}")


if __name__ == "__main__":
    main()
