"""``python -m reprover_amd.generator.fit --config <generation yaml> [--ckpt_path DIR] [--max-steps N] [--val-every N]
[--log-dir DIR] [--ckpt-every N] [--resume-from DIR] [--dropout-rate RATE|config]``: the reference's generator training
(generation/main.py ``fit`` through Lightning) on the HIP engine, one GPU.  It reads the reference's ``model:`` / ``data:`` keys and
``trainer.max_steps``, and mirrors ``reprover_amd.retrieval.main.run_fit``: per batch ``training_step`` (loss, gradients,
AdamW, re-packing), epochs until ``max_steps``, a checkpoint directory swapped in atomically (a HuggingFace checkpoint of
the current weights + the training state + ``loop_state.json``), and a resume that skips the batches already trained on at
the index level.

By default the step runs WITHOUT T5's dropout; the reference trains with the checkpoint's ``dropout_rate`` (0.1), which
``--dropout-rate config`` selects.  ``reprover_amd.generator.main fit`` is deliberately left as it is
and does not route here."""
from __future__ import annotations

import argparse
import json
import os
import shutil
from typing import Any, Dict, Optional

import yaml

from .datamodule import GeneratorDataModule
from .main import run_validate
from .model import RetrievalAugmentedGenerator

TRAINING_STATE = "training_state"


def weight_decay_for(trainer_cfg: Optional[Dict]) -> float:
    """The weight decay the reference's ``get_optimizers`` (common.py:381-405) ends up with: ``torch.optim.AdamW(lr)``
    (default 1e-2), except under a ``DeepSpeedStrategy``, where it picks DeepSpeed's ``FusedAdam(adam_w_mode=True)`` (or
    ``DeepSpeedCPUAdam``), whose default weight decay is 0 (from its published signature; not verified here against an
    installed DeepSpeed)."""
    strategy = (trainer_cfg or {}).get("strategy")
    path = strategy.get("class_path", "") if isinstance(strategy, dict) else (strategy or "")
    return 0.0 if str(path).endswith("DeepSpeedStrategy") else 1e-2


def save_fit_checkpoint(model: RetrievalAugmentedGenerator, ckpt_dir: str, loop: Optional[Dict[str, int]] = None) -> str:
    """``<ckpt_dir>/`` = a HuggingFace checkpoint of the current weights, ``<ckpt_dir>/training_state/`` the masters and
    moments of both halves, ``<ckpt_dir>/loop_state.json`` the loop's position.  Written to ``<ckpt_dir>.tmp`` and renamed
    into place: a crash in the middle leaves the previous checkpoint (or ``<ckpt_dir>.old``) intact."""
    tmp, old = ckpt_dir.rstrip("/") + ".tmp", ckpt_dir.rstrip("/") + ".old"
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    model.train_engine.save_pretrained(tmp)
    model.train_engine.save_training_state(os.path.join(tmp, TRAINING_STATE))
    with open(os.path.join(tmp, "loop_state.json"), "w") as fh:
        json.dump(loop or {}, fh)
    shutil.rmtree(old, ignore_errors=True)
    if os.path.exists(ckpt_dir):
        os.replace(ckpt_dir, old)
    os.replace(tmp, ckpt_dir)
    shutil.rmtree(old, ignore_errors=True)
    return ckpt_dir


def run_fit(model: RetrievalAugmentedGenerator, dm: GeneratorDataModule, max_steps: int, val_every: int = 0,
            ckpt_dir: Optional[str] = None, ckpt_every: int = 0, resume_from: Optional[str] = None, seed: int = 3407,
            log=print, weight_decay: float = 1e-2) -> Dict[str, Any]:
    """The loop Lightning runs for the reference: ``configure_optimizers`` (unless the model already has its engine), then
    per batch ``training_step``; epochs until ``max_steps``; validation every ``val_every`` steps (0: never).  With
    ``ckpt_dir`` a checkpoint is written at the end (and every ``ckpt_every`` steps); ``resume_from`` = such a directory.
    Every epoch's shuffle and premise drops are seeded with a function of (``seed``, epoch) and a checkpoint records (epoch,
    batches done): a resumed run continues the data where it stopped."""
    import random

    if getattr(dm, "batch_size", 0) <= 0:
        raise ValueError(f"fit needs data.batch_size > 0 (got {dm.batch_size})")
    if dm.ds_train is None:
        dm.setup("fit")
    if model.train_engine is None:
        model.configure_optimizers(weight_decay=weight_decay)
    engine = model.train_engine
    if engine.dropout_rate > 0:
        log(f"fit: the step runs with T5's dropout, rate {engine.dropout_rate:g}")
    else:
        log("fit: the step runs without T5's dropout (the reference trains with dropout_rate 0.1)")
    step, losses, epoch, skip = 0, [], 0, 0
    if resume_from:
        if not os.path.isdir(resume_from) and os.path.isdir(resume_from.rstrip("/") + ".old"):
            log(f"fit: {resume_from} is missing, resuming from {resume_from.rstrip('/')}.old")
            resume_from = resume_from.rstrip("/") + ".old"
        engine.load_training_state(os.path.join(resume_from, TRAINING_STATE))
        step = engine.steps
        lpath = os.path.join(resume_from, "loop_state.json")
        if os.path.exists(lpath):
            with open(lpath) as fh:
                st = json.load(fh)
            epoch, skip = int(st.get("epoch", 0)), int(st.get("batches_done", 0))
            if int(st.get("seed", seed)) != int(seed):
                log(f"fit: the checkpoint's data seed {st['seed']} overrides the configured {seed}")
            seed = int(st.get("seed", seed))
    if engine.dropout_rate > 0:  # (after the resume: a loaded training state replaces the seed base and the forward count)
        log(f"fit: dropout seed base {engine.trainer.dropout_seed}, {engine.trainer._forwards} forwards drawn so far")
    caller_rng = random.getstate()  # the data draws from the global `random`, as upstream; the caller gets its stream back
    try:
        while step < max_steps:
            n_epoch = skip
            for batch in dm.train_dataloader(skip=skip, seed=seed, epoch=epoch):
                n_epoch += 1
                losses.append(model.training_step(batch, step))
                step += 1
                if val_every and step % val_every == 0:
                    rng_state = random.getstate()
                    log(f"step {step}: {run_validate(model, dm)}")
                    random.setstate(rng_state)
                if ckpt_dir and ckpt_every and step % ckpt_every == 0 and step < max_steps:
                    save_fit_checkpoint(model, ckpt_dir, {"epoch": epoch, "batches_done": n_epoch, "seed": seed, "step": step})
                if step >= max_steps:
                    break
            if n_epoch == 0:
                raise ValueError("the training split yields no full batch (drop_last=True)")
            if step < max_steps:
                epoch, skip = epoch + 1, 0
            else:
                skip = n_epoch
    finally:
        random.setstate(caller_rng)
    if ckpt_dir:
        save_fit_checkpoint(model, ckpt_dir, {"epoch": epoch, "batches_done": skip, "seed": seed, "step": step})
    return {"steps": step, "losses": [float(x) for x in losses], "checkpoint": ckpt_dir, "epoch": epoch,
            "weight_decay": engine.weight_decay}


def dropout_rate_arg(text: str):
    """``--dropout-rate``: a float in [0, 1), or ``config`` = the checkpoint's ``config.json`` ``dropout_rate``."""
    if text == "config":
        return text
    try:
        rate = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is neither a number nor 'config'")
    if not 0.0 <= rate < 1.0:
        raise argparse.ArgumentTypeError(f"dropout rate {rate} outside [0, 1)")
    return rate


def resolve_dropout_rate(value, checkpoint: str) -> float:
    """The rate ``--dropout-rate`` asks for: a number as given, ``config`` from ``<checkpoint>/config.json`` (HF's default
    of 0.1 when the key is absent)."""
    if value != "config":
        return float(value)
    path = os.path.join(checkpoint, "config.json")
    if not os.path.exists(path):
        raise SystemExit(f"fit: --dropout-rate config reads {path}, which does not exist: pass --ckpt_path with a local "
                         "HuggingFace checkpoint directory (a hub name is not resolved), or give the rate as a number")
    with open(path) as fh:
        return float(json.load(fh).get("dropout_rate", 0.1))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Tactic generator: fit on MI355X (one GPU; dropout off unless --dropout-rate).")
    ap.add_argument("--config", required=True, help="YAML with `model:`, `data:` and `trainer:` sections (reference layout)")
    ap.add_argument("--ckpt_path", default=None, help="HF checkpoint dir (overrides model.model_name)")
    ap.add_argument("--max-steps", type=int, default=None, help="overrides trainer.max_steps")
    ap.add_argument("--val-every", type=int, default=0, help="validate every N steps (0: never)")
    ap.add_argument("--log-dir", default=None, help="the checkpoint is written to <log-dir>/checkpoint")
    ap.add_argument("--ckpt-every", type=int, default=0, help="also checkpoint every N steps (0: only at the end)")
    ap.add_argument("--resume-from", default=None, help="a checkpoint directory written by an earlier fit")
    ap.add_argument("--dropout-rate", type=dropout_rate_arg, default=0.0, metavar="RATE",
                    help="T5's dropout in the training step: a rate in [0, 1), or 'config' for the checkpoint's "
                         "config.json dropout_rate (the reference's mode); default 0")
    return ap


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    with open(args.config) as fh:
        cfg = yaml.safe_load(fh)
    m, d, tcfg = cfg["model"], cfg["data"], cfg.get("trainer") or {}
    if int(d.get("batch_size", 0)) <= 0:
        raise SystemExit("fit: the config's data.batch_size must be a positive integer")
    wd = weight_decay_for(tcfg)
    seed = cfg.get("seed_everything")
    print(f"fit: weight decay {wd} ("
          + ("DeepSpeedStrategy: FusedAdam(adam_w_mode=True)'s default" if wd == 0.0 else "torch.optim.AdamW's default") + ")",
          flush=True)
    model = RetrievalAugmentedGenerator(
        args.ckpt_path or m["model_name"], float(m.get("lr", 0.0)), int(m.get("warmup_steps", 0)), int(m["num_beams"]),
        int(m.get("eval_num_retrieved", 100)), int(m.get("eval_num_workers", 1)), int(m.get("eval_num_gpus", 1)),
        int(m.get("eval_num_theorems", 0)), int(d["max_inp_seq_len"]), int(d["max_oup_seq_len"]),
        float(m.get("length_penalty", 0.0)), m.get("ret_ckpt_path"),
        dropout_rate=resolve_dropout_rate(args.dropout_rate, args.ckpt_path or m["model_name"]),
        dropout_seed=int(seed) if seed is not None else None)
    model.configure_optimizers(weight_decay=wd, gradient_clip_val=tcfg.get("gradient_clip_val"))
    dm = GeneratorDataModule(d["data_path"], m["model_name"], int(d["batch_size"]), int(d["eval_batch_size"]),
                             int(d["max_inp_seq_len"]), int(d["max_oup_seq_len"]), float(d.get("p_drop", 0.0)),
                             int(d.get("num_workers", 0)), d.get("corpus_path"), d.get("preds_path"))
    log_dir = args.log_dir or tcfg.get("default_root_dir") or os.path.join(os.getcwd(), "lightning_logs")
    print(f"fit: checkpoints go to {os.path.join(log_dir, 'checkpoint')}", flush=True)
    out = run_fit(model, dm, args.max_steps or int(tcfg.get("max_steps", 1)), args.val_every,
                  ckpt_dir=os.path.join(log_dir, "checkpoint"), ckpt_every=args.ckpt_every, resume_from=args.resume_from,
                  seed=int(seed) if seed is not None else 3407, weight_decay=wd)
    first = f"{out['losses'][0]:.6f} -> {out['losses'][-1]:.6f}" if out["losses"] else "(no step taken)"
    print(f"fit: {out['steps']} steps, loss {first}; checkpoint {out['checkpoint']}")


if __name__ == "__main__":
    main()
