"""The tactic generator's training step without a GPU: the two flat layouts against HF's parameter
list, the train dataloader on G23's data, the checkpoint writer, the command line, and the float64 reference step
(tests/seq2seq_train_helpers.py) pinned to torch.optim.AdamW on HF's model, with one planted bug."""
import ctypes as C
import json
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from oracle import train_ref  # noqa: E402
from seq2seq_full_grad_helpers import g26_sources, padded_sources  # noqa: E402
from seq2seq_grad_helpers import g25_labels, padded_labels  # noqa: E402
from seq2seq_helpers import g23_inputs  # noqa: E402
from seq2seq_train_helpers import ALIASES, RefTrainer64, parameter_names  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import load_seq2seq_checkpoint  # noqa: E402
from reprover_amd.seq2seq_train import decoder_param_layout, write_seq2seq_checkpoint  # noqa: E402
from reprover_amd.train import param_layout  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-12  # float64 against float64 in another operation order (tests/test_step_ends_cpu.py's bar and derivation)


# ---- layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_the_two_flat_layouts_name_every_hf_parameter_once(name):
    cfg = synth.seq2seq_config(name)
    sd = synth.synth_seq2seq_state_dict(cfg)
    tied = bool(cfg["tie_word_embeddings"])
    enc = [(k, tuple(sh)) for k, sh, _ in param_layout(cfg)[:-1]]
    names, shapes, off = decoder_param_layout(cfg, tied)
    assert names[0] == "shared.weight" and all(o % 64 == 0 for o in off)
    assert all(off[i + 1] - off[i] >= int(np.prod(sh)) for i, sh in enumerate(shapes))
    union = enc + list(zip(names, shapes))[1:]  # minus the decoder's shared slot
    assert len({k for k, _ in union}) == len(union), "a parameter is named twice"
    want = {k: tuple(sd[k].shape) for k in parameter_names(cfg, sd)}
    assert dict(union) == want
    assert ("lm_head.weight" in dict(union)) == (not tied)


def test_reload_symbol_and_abi_version():
    lib = _lib.load()
    assert hasattr(lib, "rp_decoder_load_params")
    assert lib.rp_abi_version() == 7
    buf = np.zeros(64, dtype=np.float32)
    assert lib.rp_decoder_load_params(None, buf.ctypes.data_as(C.c_void_p), None) == -1  # RP_E_INVALID, nothing launched
    assert lib.rp_decoder_grad_tensors(None) == 0


# ---- the train dataloader ----------------------------------------------------------------------------------------------------
def _datamodule(tmp, batch_size=4):
    from reprover_amd.generator.datamodule import GeneratorDataModule

    g = json.load(open(os.path.join(GOLDEN, "g23_generator_data.json"), encoding="utf-8"))
    c = g["config"]
    path, preds = g23_inputs(str(tmp))
    shutil.copy(path, os.path.join(str(tmp), "train.json"))
    dm = GeneratorDataModule(str(tmp), "unused", batch_size, 64, c["max_inp_seq_len"], c["max_oup_seq_len"], c["p_drop"])
    dm.preds = preds
    dm.setup("fit")
    return dm, g


def _epoch(dm, **kw):
    return [(b["state"], b["tactic"], b["state_ids"].tolist(), b["tactic_ids"].tolist()) for b in dm.train_dataloader(**kw)]


def test_train_dataloader_shuffles_drops_and_resumes(tmp_path):
    dm, g = _datamodule(tmp_path)
    n = len(dm.ds_train)
    assert n == 21 and n % dm.batch_size
    a, b, other = _epoch(dm, seed=5, epoch=0), _epoch(dm, seed=5, epoch=0), _epoch(dm, seed=5, epoch=1)
    assert a == b, "one (seed, epoch) is one sequence of batches"
    assert a != other and _epoch(dm, seed=6, epoch=0) != a
    assert len(a) == n // dm.batch_size and all(len(x[0]) == dm.batch_size for x in a), "the incomplete batch is dropped"
    # p_drop acts in training: the epoch holds states that lost premises; validation keeps every premise (G23's 'preds')
    assert dm.ds_train.is_train and not dm.ds_val.is_train
    full = set(g["preds"]["state"])
    train_states = [s for x in a for s in x[0]]
    assert any(s not in full for s in train_states), "p_drop = 0.5 dropped nothing"
    assert {s[-20:] for s in train_states} <= {s[-20:] for s in full}, "the states themselves are the split's"
    got_val = [s for batch in dm.val_dataloader() for s in batch["state"]]
    assert got_val == g["preds"]["state"], "no drop outside training"
    # index-level skip: the remaining batches are the uninterrupted epoch's
    assert _epoch(dm, skip=2, seed=5, epoch=0) == a[2:]
    # without a seed the caller's `random` stream decides
    random.seed(77)
    x = _epoch(dm)
    random.seed(77)
    assert _epoch(dm) == x


# ---- checkpoints -------------------------------------------------------------------------------------------------------------
def _full_state_dict(cfg):
    sd = dict(synth.synth_seq2seq_state_dict(cfg))
    for a in ALIASES:
        sd[a] = sd["shared.weight"]
    if cfg["tie_word_embeddings"]:
        sd["lm_head.weight"] = sd["shared.weight"]
    return sd


@pytest.mark.parametrize("name", ["tiny", "tiny-tied"])
def test_checkpoint_round_trip_bit_for_bit(name, tmp_path):
    cfg = synth.seq2seq_config(name)
    sd = _full_state_dict(cfg)
    write_seq2seq_checkpoint(str(tmp_path / "ckpt"), cfg, sd)
    cfg2, sd2 = load_seq2seq_checkpoint(str(tmp_path / "ckpt"))
    assert set(sd2) == set(sd)
    for k in sd:
        assert sd2[k].dtype == torch.float32 and torch.equal(sd2[k], sd[k]), k
    for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers", "num_decoder_layers", "tie_word_embeddings"):
        assert cfg2[k] == cfg[k], k
    assert cfg2["scale_decoder_outputs"] == cfg["tie_word_embeddings"] and cfg2["feed_forward_proj"] == "gated-gelu"
    transformers = pytest.importorskip("transformers")
    model, info = transformers.T5ForConditionalGeneration.from_pretrained(str(tmp_path / "ckpt"), output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info.get("mismatched_keys")
    head = sd["lm_head.weight"]
    assert torch.equal(model.lm_head.weight, head) and torch.equal(model.shared.weight, sd["shared.weight"])
    assert torch.equal(model.decoder.block[1].layer[1].EncDecAttention.k.weight,
                       sd["decoder.block.1.layer.1.EncDecAttention.k.weight"])


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_fit_parser_and_weight_decay_choice():
    import yaml

    from reprover_amd.generator import fit

    args = fit.build_parser().parse_args(["--config", "c.yaml", "--ckpt_path", "ck", "--max-steps", "7", "--val-every", "3",
                                          "--log-dir", "logs", "--ckpt-every", "2", "--resume-from", "logs/checkpoint"])
    assert (args.config, args.ckpt_path, args.max_steps, args.val_every, args.log_dir, args.ckpt_every, args.resume_from) == \
        ("c.yaml", "ck", 7, 3, "logs", 2, "logs/checkpoint")
    deepspeed = yaml.safe_load("""
trainer:
  strategy:
    class_path: pytorch_lightning.strategies.DeepSpeedStrategy
    init_args: {stage: 2, offload_optimizer: false}
  max_steps: 500000
""")
    assert fit.weight_decay_for(deepspeed["trainer"]) == 0.0
    assert fit.weight_decay_for({"max_steps": 5}) == 1e-2 and fit.weight_decay_for(None) == 1e-2
    assert fit.weight_decay_for({"strategy": "ddp"}) == 1e-2
    assert fit.weight_decay_for({"strategy": {"class_path": "pytorch_lightning.strategies.DDPStrategy"}}) == 1e-2


# ---- the reference step ------------------------------------------------------------------------------------------------------
def _g26():
    return g26_sources(), padded_labels(g25_labels())


# HF evaluates every RMSNorm's variance in fp32 whatever the model's dtype (modeling_t5.py T5LayerNorm), so its float64
# model is float64 except for one fp32 rounding of the variance (relative 2^-24, 2^-25 on the rsqrt) at each of the 12 norms
# of tiny (2 per encoder layer + 1, 3 per decoder layer + 1), seen by the forward and again by the backward through the
# saved value: 24 x 2^-25 if the errors add linearly; x 16 for what the layers after a norm make of a perturbation of its
# output.  Relative to the largest element of a tensor's gradient.
HF_GRAD_REL = 24 * 16 * 2.0 ** -25


def test_reference_step_is_torch_adamw_on_hf_for_two_steps():
    """tiny-tied, two steps at lr 1e-3.  (a) The reference's gradients are HF's (shared.weight: autograd's sum over the
    three uses) within HF_GRAD_REL.  (b) The reference's update is torch.optim.AdamW's: both are given HF's gradient, both
    carry their own moments over the two steps, and the parameters after each step agree within REL of the largest (both
    float64).  Each step starts both sides from the reference's fp32-stored parameters, as the engine stores its masters:
    elementwise agreement of a whole trajectory is not asked, a near-zero gradient element moves by lr either way."""
    from make_golden_generate import hf_model

    cfg = synth.seq2seq_config("tiny-tied")
    sd = synth.synth_seq2seq_state_dict(cfg)
    srcs, y = _g26()
    ids, mask = padded_sources(srcs)
    lr = 1e-3
    ref = RefTrainer64(cfg, sd, lr)
    model = hf_model(cfg, sd).double()
    params = dict(model.named_parameters())
    assert set(params) == set(ref.p)
    opt = torch.optim.AdamW(model.parameters(), lr=lr)  # the reference's get_optimizers outside DeepSpeed
    worst_g = worst_p = 0.0
    for step in (1, 2):
        loss, grads = ref.gradients(srcs, y)
        opt.zero_grad()
        out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(y))
        out.loss.backward()
        assert abs(float(out.loss.detach()) - loss) <= HF_GRAD_REL * abs(loss)
        hf_g = {k: p.grad.detach().numpy().copy() for k, p in params.items()}
        for k in grads:
            e = np.abs(hf_g[k] - grads[k]).max() / np.abs(grads[k]).max()
            worst_g = max(worst_g, e)
            assert e <= HF_GRAD_REL, (step, k, e)
        p0, m0, v0 = dict(ref.p), dict(ref.m), dict(ref.v)
        opt.step()
        ref.apply(hf_g)
        for k, p in params.items():
            want, _, _ = train_ref.adamw_step64(p0[k], hf_g[k], m0[k], v0[k], step, lr)
            e = np.abs(p.detach().numpy() - want).max() / np.abs(want).max()
            worst_p = max(worst_p, e)
            assert e <= REL, (step, k, e)
            assert np.array_equal(ref.p[k], want.astype(np.float32)), k
            with torch.no_grad():
                p.copy_(torch.from_numpy(ref.p[k]).double())
    assert not np.array_equal(ref.p["shared.weight"], sd["shared.weight"].numpy())
    print(f"gradients: worst {worst_g:.2e} of the tensor's max (bound {HF_GRAD_REL:.2e}); parameters: worst {worst_p:.2e} "
          f"relative (bound {REL:.0e})")


def test_planted_double_update_of_shared_moves_it_far_beyond_the_gpu_bar():
    """shared.weight updated once per half (the encoder's part, then the decoder's, each with its own moments) instead of
    once with the sum.  The GPU test holds a step's masters to 2 x torch-fp32 AdamW's own error against the float64 oracle
    + one fp32 ulp of the largest value (tests/test_step_ends_gpu.py); that bar, evaluated here with torch's fp32 AdamW on
    the CPU for the same step, is what the mutant's movement is measured in.

    Measured: the mutant moves shared.weight by 1.04e-3 (= lr: an element both parts push the same way moves twice) where
    the bar is 1.02e-6 (torch fp32 2.7e-7), 1.0e+03 x."""
    cfg = synth.seq2seq_config("tiny-tied")
    sd = synth.synth_seq2seq_state_dict(cfg)
    srcs, y = _g26()
    lr = 1e-3
    clean, bad = RefTrainer64(cfg, sd, lr), RefTrainer64(cfg, sd, lr, mutant="shared_twice")
    _, grads = clean.gradients(srcs, y)
    clean.apply(grads)
    bad.step(srcs, y)
    k = "shared.weight"
    moved = float(np.abs(bad.p[k].astype(np.float64) - clean.p[k]).max())
    # the GPU bar for this tensor and step
    w0 = sd[k].numpy()
    want, _, _ = train_ref.adamw_step64(w0, grads[k], np.zeros(w0.shape), np.zeros(w0.shape), 1, lr)
    p = torch.nn.Parameter(sd[k].clone())
    opt = torch.optim.AdamW([p], lr=lr)
    p.grad = torch.from_numpy(grads[k].astype(np.float32))
    opt.step()
    e_torch = float(np.abs(p.detach().numpy().astype(np.float64) - want).max())
    bar = 2.0 * e_torch + float(np.spacing(np.float32(np.abs(want).max())))
    print(f"shared_twice moves {k} by {moved:.3e}; GPU bar {bar:.3e} (torch fp32 {e_torch:.3e}): {moved / bar:.1e} x")
    assert moved > 100 * bar
    for other in clean.p:
        if other != k:
            assert np.array_equal(bad.p[other], clean.p[other]), other
