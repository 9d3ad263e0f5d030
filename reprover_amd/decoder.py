"""HipT5Generator: T5ForConditionalGeneration.generate (beam search) on libreprover_hip.

The encoder is ``HipT5Encoder`` (``rp_encode_hidden``: last_hidden_state instead of the pool); the decoder is
``rp_decoder_*`` (one launch sequence per beam-search step for 1..32 states); the beam bookkeeping
is ``reprover_amd.generation.beam_search_batch`` with the device top-2nb selection ``rp_beam_select_batch``.
``generate_many`` / ``greedy_many`` run the beams of several sources through that loop and return, per source, the bits
of ``generate`` / ``greedy``, which are its one-state calls.  With ``sync_every=K`` the beam search keeps its books on the
device instead (``rp_beam_books_init`` / ``rp_beam_advance``, ``generation.beam_search_batch_device``).
``generate_stream`` is the same search with admission: sources join a running loop between steps (``rp_decoder_pool_*``,
``generation.BeamSearchPool``) and each returns, when it stops, the bits of ``generate``; with ``sync_every=K`` the
stream's books live on the device too (``rp_beam_books_admit`` / ``rp_beam_pool_advance`` / ``rp_beam_books_rows``,
``generation.BeamBooksPool``).  The
teacher-forced loss (``forward`` / ``label_log_probs``) is ``rp_decoder_forward`` over all pairs of a batch at once.
PyTorch tensors are containers only.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .encoder import HipT5Encoder, _require_gpu
from .generation import (BeamBooks, BeamBooksPool, BeamSearchOutput, BeamSearchPool, SamplePool, SampleState, SamplingParams,
                         _check_count, _check_prompts, _check_room, _prompt_tokens, beam_search, beam_search_batch,
                         beam_search_batch_device, check_sampling, greedy_search, greedy_search_batch, sample_search_batch)

IGNORE_INDEX = -100  # the label HF's CrossEntropyLoss(ignore_index=-100) skips
# Dropout sites of the training step (include/reprover_hip.h RP_DROP_SITE_*; ``rp_dbg_dropout_mask`` reads a site's mask).
# Encoder: embeddings, final norm output, layer i at 16 + 8 i + {0 probs, 1 attention residual, 2 FFN inner, 3 FFN residual}.
DROP_SITE_EMBED, DROP_SITE_FINAL, DROP_SITE_LAYER0 = 0, 1, 16
# Decoder (rows = packed target token indices): embeddings, final norm output, layer i at 0x4000 + 8 i + the offsets below
DROP_SITE_DEC_EMBED, DROP_SITE_DEC_FINAL, DROP_SITE_DEC_LAYER0 = 2, 3, 0x4000
DEC_SELF_PROBS, DEC_SELF_RESID, DEC_CROSS_PROBS, DEC_CROSS_RESID, DEC_FF_INNER, DEC_FF_RESID = range(6)
_STATE_0 = np.zeros(1, dtype=np.int32)  # the active list of a one-state step

_DEC_KEYS = {
    "ln_self": "layer.0.layer_norm.weight",
    "q": "layer.0.SelfAttention.q.weight",
    "k": "layer.0.SelfAttention.k.weight",
    "v": "layer.0.SelfAttention.v.weight",
    "o": "layer.0.SelfAttention.o.weight",
    "ln_cross": "layer.1.layer_norm.weight",
    "cq": "layer.1.EncDecAttention.q.weight",
    "ck": "layer.1.EncDecAttention.k.weight",
    "cv": "layer.1.EncDecAttention.v.weight",
    "co": "layer.1.EncDecAttention.o.weight",
    "ln_ff": "layer.2.layer_norm.weight",
    "wi_0": "layer.2.DenseReluDense.wi_0.weight",
    "wi_1": "layer.2.DenseReluDense.wi_1.weight",
    "wo": "layer.2.DenseReluDense.wo.weight",
}


def load_seq2seq_checkpoint(path: str) -> Tuple[Dict, Dict[str, torch.Tensor]]:
    """(cfg, state dict) of a HuggingFace T5ForConditionalGeneration directory (config.json + model.safetensors or
    pytorch_model.bin).  A decoder-only checkpoint raises ``ValueError``."""
    if not os.path.isdir(path):
        raise FileExistsError(f"Checkpoint {path} does not exist.")
    with open(os.path.join(path, "config.json")) as fh:
        hf = json.load(fh)
    if not hf.get("is_encoder_decoder", hf.get("model_type") in ("t5", "mt5", "umt5")):
        raise ValueError(f"{path} is not an encoder-decoder (T5ForConditionalGeneration) checkpoint; decoder-only "
                         "generators (the reference's AutoModelForCausalLM fallback) are not implemented")
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file

        sd = load_file(st)
    else:
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    if not any(k.startswith("decoder.block.") for k in sd):
        raise ValueError(f"{path} holds no decoder.* weights: not a T5ForConditionalGeneration checkpoint")
    cfg = dict(
        vocab_size=hf["vocab_size"], d_model=hf["d_model"], d_kv=hf["d_kv"], num_heads=hf["num_heads"], d_ff=hf["d_ff"],
        num_layers=hf["num_layers"], num_decoder_layers=hf.get("num_decoder_layers") or hf["num_layers"],
        relative_attention_num_buckets=hf.get("relative_attention_num_buckets", 32),
        relative_attention_max_distance=hf.get("relative_attention_max_distance", 128),
        layer_norm_epsilon=hf.get("layer_norm_epsilon", 1e-6), feed_forward_proj=hf.get("feed_forward_proj", "relu"),
        tie_word_embeddings=bool(hf.get("tie_word_embeddings", True)),
        decoder_start_token_id=hf.get("decoder_start_token_id", 0), eos_token_id=hf.get("eos_token_id", 1),
    )
    # transformers 5 writes tie_word_embeddings=true for every T5 and keeps the d_model^-0.5 output rescale in
    # scale_decoder_outputs; transformers 4 has no such key and rescales exactly when the embeddings are tied
    cfg["scale_decoder_outputs"] = bool(hf.get("scale_decoder_outputs", cfg["tie_word_embeddings"]))
    return cfg, sd


def lm_head_source(cfg: Dict, sd: Dict[str, torch.Tensor]) -> Tuple[str, bool]:
    """(state-dict key of the lm_head, whether the final hidden state is scaled by d_model^-0.5 before it).  The head is
    ``lm_head.weight`` whenever the checkpoint holds one, else ``shared.weight`` (a tied checkpoint saves only that); the
    scale follows ``scale_decoder_outputs`` when the config has it, else ``tie_word_embeddings``."""
    tied = bool(cfg.get("tie_word_embeddings", False))
    if "lm_head.weight" in sd:
        key = "lm_head.weight"
    elif tied:
        key = "shared.weight"
    else:
        raise ValueError("untied checkpoint without lm_head.weight")
    return key, bool(cfg.get("scale_decoder_outputs", tied))


def source_lengths(state_mask) -> np.ndarray:
    """Per-row token counts of a right-padded 0/1 attention mask (what the tokenizer produces); anything else raises
    ``ValueError``: the packed encoder reads the first ``n`` ids of a row."""
    m = np.asarray(state_mask.cpu() if isinstance(state_mask, torch.Tensor) else state_mask).astype(np.int64)
    if m.ndim != 2:
        raise ValueError(f"state_mask must be [B, S], got shape {m.shape}")
    if not np.isin(m, (0, 1)).all():
        raise ValueError("state_mask must hold only 0 and 1")
    n = m.sum(1)
    if not (m == (np.arange(m.shape[1])[None] < n[:, None])).all():
        raise ValueError("state_mask must be right-padded (ones, then zeros)")
    return n


def shift_and_segment(tactic_ids, decoder_start_token_id: int = 0, pad_token_id: int = 0):
    """The decoder side of ``T5ForConditionalGeneration(labels=tactic_ids)`` as packed segments.

    Row b's segment ends at its last non-ignored label (causality makes later positions irrelevant; a row with no
    counted label is empty).  Inputs are HF's ``_shift_right(labels)``: the start token, then the labels shifted by one
    with ``-100`` replaced by the pad id, so an interior ``-100`` is fed as 0 and excluded from the loss.
    Returns (tokens int32 [sum T_b], labels int32 [sum T_b], cu int32 [B + 1])."""
    y = np.asarray(tactic_ids.cpu() if isinstance(tactic_ids, torch.Tensor) else tactic_ids).astype(np.int64)
    if y.ndim != 2:
        raise ValueError(f"tactic_ids must be [B, T], got shape {y.shape}")
    keep = y != IGNORE_INDEX
    if (y[keep] < 0).any():
        raise ValueError("tactic_ids holds negative ids other than -100")
    lens = np.where(keep.any(1), y.shape[1] - np.argmax(keep[:, ::-1], axis=1), 0)
    toks, labs = [], []
    for b, n in enumerate(lens):
        lab = y[b, :n]
        inp = np.concatenate([[decoder_start_token_id], lab[:-1]]) if n else lab
        toks.append(np.where(inp == IGNORE_INDEX, pad_token_id, inp))
        labs.append(lab)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cat = (lambda a: np.concatenate(a).astype(np.int32)) if len(lens) else (lambda a: np.zeros(0, np.int32))
    return cat(toks), cat(labs), cu


def _pc(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


REL_BIAS_KEY_DEC = "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def decoder_grad_names(cfg: Dict, tied: bool) -> List[str]:
    """HF state-dict names of the decoder's flat layout (``rp_decoder_grad_layout``), in buffer order; ``tied``: the
    decoder was created with the tied head and has no ``lm_head.weight`` slot."""
    names = ["shared.weight"] + ([] if tied else ["lm_head.weight"]) + [REL_BIAS_KEY_DEC, "decoder.final_layer_norm.weight"]
    for i in range(cfg["num_decoder_layers"]):
        names += [f"decoder.block.{i}.{key}" for key in _DEC_KEYS.values()]
    return names


def decoder_grad_shapes(cfg: Dict) -> Dict[str, Tuple[int, ...]]:
    """HF shape of every tensor ``decoder_grad_names`` can name."""
    c = cfg
    D, F, inner, V = c["d_model"], c["d_ff"], c["num_heads"] * c["d_kv"], c["vocab_size"]
    sh = {"ln_self": (D,), "q": (inner, D), "k": (inner, D), "v": (inner, D), "o": (D, inner), "ln_cross": (D,),
          "cq": (inner, D), "ck": (inner, D), "cv": (inner, D), "co": (D, inner), "ln_ff": (D,), "wi_0": (F, D),
          "wi_1": (F, D), "wo": (D, F)}
    out = {"shared.weight": (V, D), "lm_head.weight": (V, D), "decoder.final_layer_norm.weight": (D,),
           REL_BIAS_KEY_DEC: (c.get("relative_attention_num_buckets", 32), c["num_heads"])}
    for i in range(c["num_decoder_layers"]):
        for fld, key in _DEC_KEYS.items():
            out[f"decoder.block.{i}.{key}"] = sh[fld]
    return out


class HipT5Decoder:
    """The decoder weights resident on one GPU + the per-step launch sequence."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device):
        if cfg.get("feed_forward_proj", "gated-gelu") != "gated-gelu":
            raise _lib.HipLibraryError(f"feed_forward_proj={cfg.get('feed_forward_proj')!r} is not implemented")
        self.device = _require_gpu(device)
        self.cfg = dict(cfg)
        self.V = cfg["vocab_size"]
        L = cfg["num_decoder_layers"]
        lib = _lib.load()
        c = _lib.RpT5Config(cfg["vocab_size"], cfg["d_model"], cfg["d_kv"], cfg["num_heads"], cfg["d_ff"], L,
                            cfg.get("relative_attention_num_buckets", 32), cfg.get("relative_attention_max_distance", 128),
                            float(cfg.get("layer_norm_epsilon", 1e-6)))
        head, scaled = lm_head_source(cfg, sd)
        with torch.cuda.device(self.device):
            keep = []

            def dev(name: str) -> int:
                t = sd[name].detach().to(device=self.device, dtype=torch.float32).contiguous()
                keep.append(t)
                return t.data_ptr()

            layers = (_lib.RpT5DecoderLayerWeights * L)()
            for i in range(L):
                for fld, key in _DEC_KEYS.items():
                    setattr(layers[i], fld, dev(f"decoder.block.{i}.{key}"))
            w = _lib.RpT5DecoderWeights(
                dev("shared.weight"), dev("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"),
                dev("decoder.final_layer_norm.weight"), dev(head), layers, int(scaled))
            handle = C.c_void_p()
            torch.cuda.synchronize(self.device)
            _lib.check(lib.rp_decoder_create(C.byref(c), C.byref(w), _lib.RP_DT_F32, C.byref(handle)), "rp_decoder_create")
            del keep
        self._lib = lib
        self._handle = handle
        self._ws: Optional[torch.Tensor] = None
        self._sel_ws: Optional[torch.Tensor] = None

    @classmethod
    def from_handle(cls, lib, handle, cfg: Optional[Dict], device) -> "HipT5Decoder":
        """Wrap a decoder made by ``rp_decoder_create`` elsewhere (the wrapper owns it and destroys it).  With ``handle``
        None and ``cfg`` None the object only serves ``select`` (``rp_beam_select`` needs no decoder)."""
        self = cls.__new__(cls)
        self._lib, self._handle, self.device = lib, handle, torch.device(device)
        self.cfg = dict(cfg) if cfg else {}
        self.V = self.cfg.get("vocab_size")
        self._ws: Optional[torch.Tensor] = None
        self._sel_ws: Optional[torch.Tensor] = None
        return self

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                self._lib.rp_decoder_destroy(h)
            except Exception:
                pass
            self._handle = None

    # -- one state: the one-state calls of start_many / step_many / select_many below -------------------------------------
    def workspace_bytes(self, nb: int, max_len: int, src_len: int) -> int:
        return self._many_workspace_bytes(np.array([0, src_len], dtype=np.int32), nb, max_len)

    def start(self, enc_bf16: torch.Tensor, nb: int, max_len: int) -> None:
        """Cross K/V of one source [S, d_model] bf16 for a search of ``nb`` beams and ``max_len`` positions."""
        self.start_many(enc_bf16, np.array([0, enc_bf16.shape[0]], dtype=np.int32), nb, max_len)

    def step(self, tokens: torch.Tensor, ancestry: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """log-probs [nb, V] of one step (``beam_search``'s ``step``; ancestry int [nb, t + 1])."""
        return self.step_many(_STATE_0, tokens, ancestry, out)

    def _teacher_forced_args(self, entry: str, src_cu, tokens, labels, tgt_cu):
        """What ``rp_decoder_forward`` and ``rp_decoder_loss_grad`` share: int32 cu arrays, (B, T, S), the device tokens /
        labels, the lp / sc outputs, and the entry's own workspace, kept between calls and grown to
        ``<entry>_workspace_bytes``."""
        src_cu = np.ascontiguousarray(src_cu, dtype=np.int32)
        tgt_cu = np.ascontiguousarray(tgt_cu, dtype=np.int32)
        B, T, S = len(tgt_cu) - 1, int(tgt_cu[-1]), int(src_cu[-1])
        n = int(getattr(self._lib, entry + "_workspace_bytes")(self._handle, _pc(src_cu), _pc(tgt_cu), B))
        if n == 0:
            raise _lib.HipLibraryError(f"{entry}: " + self._lib.rp_last_error().decode(errors="replace"))
        kept = self.__dict__.setdefault("_teacher_forced_ws", {})
        if kept.get(entry) is None or kept[entry].numel() < n:
            kept[entry] = None  # (released before the larger one is taken)
            kept[entry] = torch.empty(n, dtype=torch.uint8, device=self.device)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)  # noqa: E731
        tok, lab = dev(tokens), dev(labels)
        lp = torch.empty(T, dtype=torch.float32, device=self.device)
        sc = torch.empty(2, dtype=torch.float64, device=self.device)
        return kept[entry], src_cu, tgt_cu, B, T, S, tok, lab, lp, sc

    def forward(self, enc_bf16: torch.Tensor, src_cu: np.ndarray, tokens: np.ndarray, labels: np.ndarray,
                tgt_cu: np.ndarray, rows: bool = False):
        """Teacher-forced pass over packed pairs (``rp_decoder_forward``): enc_bf16 [sum S_b, d_model] device bf16,
        host cu arrays, host int tokens / labels [sum T_b].  Returns (label log-probs [sum T_b] fp32 on the device,
        (sum of -log p, count) as floats, the full log-prob rows [sum T_b, V] or None)."""
        ws, src_cu, tgt_cu, B, T, _, tok, lab, lp, sc = self._teacher_forced_args("rp_decoder_forward", src_cu, tokens,
                                                                                  labels, tgt_cu)
        ptr = lambda t: t.data_ptr() if T else None  # noqa: E731  (no target token: the entry point takes nulls)
        out_rows = torch.empty((T, self.V), dtype=torch.float32, device=self.device) if rows else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_decoder_forward(self._handle, ptr(enc_bf16), _pc(src_cu), ptr(tok), ptr(lab),
                                                    _pc(tgt_cu), B, ptr(lp), sc.data_ptr(), ptr(out_rows) if rows else None,
                                                    ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "rp_decoder_forward")
        s, c = sc.cpu().tolist()
        return lp, (s, c), out_rows

    def grad_layout(self) -> Tuple[List[str], np.ndarray]:
        """(HF state-dict names, element offsets [n + 1]) of ``rp_decoder_loss_grad``'s flat fp32 gradient buffer, in
        buffer order.  A decoder created with the tied head has no ``lm_head.weight`` entry (``shared.weight`` carries
        both gradients)."""
        n = int(self._lib.rp_decoder_grad_tensors(self._handle))
        off = np.zeros(n + 1, dtype=np.int64)
        _lib.check(self._lib.rp_decoder_grad_layout(self._handle, off.ctypes.data_as(C.c_void_p)), "rp_decoder_grad_layout")
        names = decoder_grad_names(self.cfg, tied=n != 4 + 14 * self.cfg["num_decoder_layers"])
        assert len(names) == n, (len(names), n)
        return names, off

    def grad_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """HF shape of every tensor of ``grad_layout``."""
        return decoder_grad_shapes(self.cfg)

    def load_params(self, flat: torch.Tensor) -> None:
        """Refresh every resident copy of the weights from fp32 masters in ``grad_layout``'s flat form
        (``rp_decoder_load_params``: one launch on the current stream, nothing else)."""
        assert flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous()
        if flat.numel() != int(self.grad_layout()[1][-1]):
            raise ValueError(f"load_params: {flat.numel()} floats for a layout of {int(self.grad_layout()[1][-1])}")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_decoder_load_params(self._handle, flat.data_ptr(), _lib.current_stream()),
                       "rp_decoder_load_params")

    def loss_grad(self, enc_bf16: torch.Tensor, src_cu: np.ndarray, tokens: np.ndarray, labels: np.ndarray,
                  tgt_cu: np.ndarray, want_d_enc: bool = True, grads: Optional[torch.Tensor] = None,
                  dropout: Optional[Tuple[float, int]] = None):
        """``rp_decoder_loss_grad`` over packed pairs (arguments as ``forward``).  Returns (label log-probs [sum T_b],
        (sum of -log p, count), the flat fp32 gradient buffer of ``grad_layout``, d loss / d enc [sum S_b, d_model] fp32
        or None).  ``grads``: a buffer to write into (its padding gaps are left as they are).  ``dropout=(p, seed)``: T5's
        training mode (``rp_decoder_loss_grad_dropout``), masks at the ``DROP_SITE_DEC_*`` sites drawn from ``seed``."""
        entry = "rp_decoder_loss_grad" if dropout is None else "rp_decoder_loss_grad_dropout"
        extra = () if dropout is None else (float(dropout[0]), int(dropout[1]) & 0xFFFFFFFF)
        ws, src_cu, tgt_cu, B, T, S, tok, lab, lp, sc = self._teacher_forced_args(entry, src_cu, tokens, labels, tgt_cu)
        ptr = lambda t: t.data_ptr() if T else None  # noqa: E731
        if grads is None:
            grads = torch.zeros(int(self.grad_layout()[1][-1]), dtype=torch.float32, device=self.device)
        d_enc = torch.empty((S, self.cfg["d_model"]), dtype=torch.float32, device=self.device) if want_d_enc else None
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, entry)(self._handle, ptr(enc_bf16), _pc(src_cu), ptr(tok), ptr(lab), _pc(tgt_cu), B,
                                                 *extra, ptr(lp), sc.data_ptr(), grads.data_ptr(),
                                                 d_enc.data_ptr() if (want_d_enc and S) else None, ws.data_ptr(), ws.numel(),
                                                 _lib.current_stream()), entry)
        s, c = sc.cpu().tolist()
        return lp, (s, c), grads, d_enc

    def select(self, log_probs: torch.Tensor, running: torch.Tensor, k: int):
        """Device top-k of log_probs + running[:, None] (``rp_beam_select``): (scores, tokens, parents), each ``[k]``."""
        scores, toks, par = self.select_many(log_probs, running, log_probs.shape[0], k)
        return scores[0], toks[0], par[0]

    @staticmethod
    def max_states(nb: int) -> int:
        """States one batched call takes at ``nb`` beams (include/reprover_hip.h: 32 states, 1024 rows)."""
        return max(1, min(32, 1024 // max(1, int(nb))))

    # -- 1..max_states states (rp_decoder_batch_*): a state's rows are the same bits alone or with others ----------------
    def _many_workspace_bytes(self, cu: np.ndarray, nb: int, max_len: int) -> int:
        return int(self._lib.rp_decoder_batch_workspace_bytes(self._handle, cu.ctypes.data_as(C.c_void_p), len(cu) - 1, nb,
                                                              max_len))

    def start_many(self, enc_bf16: torch.Tensor, src_cu: np.ndarray, nb: int, max_len: int) -> None:
        """Cross K/V of ``n`` sources packed varlen (enc_bf16 [sum S_b, d_model] bf16, host ``src_cu [n + 1]``) for a
        search of ``nb`` beams and ``max_len`` positions per state, in one GEMM."""
        assert enc_bf16.dtype == torch.bfloat16 and enc_bf16.is_contiguous()
        cu = np.ascontiguousarray(src_cu, dtype=np.int32)
        n = len(cu) - 1
        if n < 1 or enc_bf16.shape[0] != int(cu[-1]):
            raise _lib.HipLibraryError(f"start_many: {n} states, src_cu[-1]={int(cu[-1]) if len(cu) else None} for "
                                       f"{enc_bf16.shape[0]} encoder rows")
        need = self._many_workspace_bytes(cu, nb, max_len)
        if need == 0:
            raise _lib.HipLibraryError("unsupported generate shape: " + self._lib.rp_last_error().decode(errors="replace"))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._many = (cu, n, nb, max_len)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_decoder_batch_cross_kv(self._handle, enc_bf16.data_ptr(), cu.ctypes.data_as(C.c_void_p),
                                                           n, nb, max_len, self._ws.data_ptr(), self._ws.numel(),
                                                           _lib.current_stream()),
                       "rp_decoder_batch_cross_kv")

    def step_many(self, active, tokens: torch.Tensor, ancestry: torch.Tensor, out: Optional[torch.Tensor] = None,
                  t: Optional[int] = None, pos=None) -> torch.Tensor:
        """log-probs [n_active * nb, V] of one step for the states ``active`` (distinct indices into ``start_many``'s
        sources): row ``a * nb + b`` is beam ``b`` of state ``active[a]`` (``beam_search_batch``'s ``step_many``).
        The position is the table's last column; with ``t`` given it is ``t`` and ``ancestry`` a wider table of which
        columns ``0..t`` are read (``sample_search_batch`` passes one table for the whole search).  With ``pos`` (one
        position per active state, in place of ``t``) the call is ``rp_decoder_batch_step_pos``: state ``active[a]`` at
        ``pos[a]``, columns ``0..pos[a]`` of its rows read (``beam_search_batch`` over prompts of different lengths)."""
        T = ancestry.shape[1]
        if pos is not None and t is not None:
            raise _lib.HipLibraryError("step_many: t= and pos= exclude each other")
        if t is not None and not 0 <= t < T:
            raise _lib.HipLibraryError(f"step_many: t={t} outside the {T} columns of the ancestry table")
        return self._step("step_many", active, tokens, ancestry, out, t=t, pos=pos)

    def _step(self, what: str, active, tokens: torch.Tensor, ancestry: torch.Tensor, out: Optional[torch.Tensor],
              t: Optional[int] = None, pos=None, src_len=None) -> torch.Tensor:
        """The one caller of the decoder step's three entries.  ``src_len`` given: the slot pool's
        (``rp_decoder_pool_step``, ``active`` its slots at ``pos``).  Else ``start_many``'s states: at ``pos`` where it is
        given (``rp_decoder_batch_step_pos``), otherwise all at ``t``, None standing for the table's last column
        (``rp_decoder_batch_step``)."""
        pool = src_len is not None
        nb = self._pool[1] if pool else self._many[2]
        act = np.ascontiguousarray(active, dtype=np.int32)
        by_state = [np.ascontiguousarray(x, dtype=np.int32) for x in (pos, src_len) if x is not None]
        rows, T = ancestry.shape
        if rows != len(act) * nb or tokens.numel() != rows or any(len(x) != len(act) for x in by_state):
            raise _lib.HipLibraryError(f"{what}: {rows} ancestry rows, {tokens.numel()} tokens, "
                                       f"{[len(x) for x in by_state]} positions / source lengths for {len(act)} states "
                                       f"of {nb} beams")
        tok = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        anc = ancestry.to(device=self.device, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty((rows, self.V), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if pool:
                p, sl = by_state
                _lib.check(self._lib.rp_decoder_pool_step(self._handle, *self._pool, _pc(act), _pc(p), _pc(sl), len(act),
                                                          tok.data_ptr(), anc.data_ptr(), T, out.data_ptr(),
                                                          self._pool_ws.data_ptr(), self._pool_ws.numel(),
                                                          _lib.current_stream()), "rp_decoder_pool_step")
                return out
            cu, n, _, max_len = self._many
            entry, where = ("rp_decoder_batch_step", T - 1 if t is None else t) if pos is None else (
                "rp_decoder_batch_step_pos", _pc(by_state[0]))
            _lib.check(getattr(self._lib, entry)(self._handle, _pc(cu), n, _pc(act), len(act), tok.data_ptr(),
                                                 anc.data_ptr(), T, nb, where, max_len, out.data_ptr(),
                                                 self._ws.data_ptr(), self._ws.numel(), _lib.current_stream()), entry)
        return out

    def _prefill(self, what: str, states, rows, src_len=None) -> None:
        """The one caller of the two prefill entries: the prompt rows ``rows[j]`` (tokens of positions ``0 .. R_j - 1``)
        of ``start_many``'s state ``states[j]`` (``rp_decoder_batch_prefill``) or, with ``src_len``, of the pool's slot
        ``states[j]`` (``rp_decoder_pool_prefill``).  Cache row ``p * nb`` of every layer is written, nothing else."""
        pool = src_len is not None
        nb = self._pool[1] if pool else self._many[2]
        st = np.ascontiguousarray(states, dtype=np.int32)
        ln = np.ascontiguousarray(src_len, dtype=np.int32) if pool else None
        if len(st) != len(rows) or not len(st) or (pool and len(ln) != len(st)):
            raise _lib.HipLibraryError(f"{what}: {len(rows)} prompts" + (f", {len(ln)} source lengths" if pool else "")
                                       + f" for {len(st)} " + ("slots" if pool else "states"))
        rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in rows]
        pcu = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        tok = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(self.device)
        longest = int(max(len(r) for r in rows))
        anc = (torch.arange(longest, dtype=torch.int32) * int(nb)).to(self.device)  # prompt position p -> cache row p * nb
        with torch.cuda.device(self.device):
            if pool:
                _lib.check(self._lib.rp_decoder_pool_prefill(self._handle, *self._pool, _pc(st), _pc(ln), _pc(pcu), len(st),
                                                             tok.data_ptr(), anc.data_ptr(), longest,
                                                             self._pool_ws.data_ptr(), self._pool_ws.numel(),
                                                             _lib.current_stream()), "rp_decoder_pool_prefill")
                return
            cu, n, _, max_len = self._many
            _lib.check(self._lib.rp_decoder_batch_prefill(self._handle, _pc(cu), n, _pc(st), _pc(pcu), len(st),
                                                          tok.data_ptr(), anc.data_ptr(), longest, nb, max_len,
                                                          self._ws.data_ptr(), self._ws.numel(), _lib.current_stream()),
                       "rp_decoder_batch_prefill")

    def prefill_many(self, states, rows) -> None:
        """The prompt rows of ``states`` (distinct indices into ``start_many``'s sources) in one pass
        (``rp_decoder_batch_prefill``, ``beam_search_batch``'s ``prefill_many``): ``rows[j]`` are the tokens of positions
        ``0 .. R_j - 1`` of state ``states[j]``; cache row ``p * nb`` of every layer is written, nothing else."""
        self._prefill("prefill_many", states, rows)

    # -- the slot pool (rp_decoder_pool_*): states join between steps, each slot at its own position ---------------------
    def pool_open(self, n_slots: int, nb: int, max_len: int, src_cap: int) -> None:
        """A workspace of ``n_slots`` places for searches of ``nb`` beams and ``max_len`` positions over sources of at
        most ``src_cap`` tokens (its own allocation: ``start`` / ``start_many`` calls in between leave it alone)."""
        need = int(self._lib.rp_decoder_pool_workspace_bytes(self._handle, n_slots, nb, max_len, src_cap))
        if need == 0:
            raise _lib.HipLibraryError("unsupported pool shape: " + self._lib.rp_last_error().decode(errors="replace"))
        self._pool_ws = None  # (released before the next one is taken)
        self._pool_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._pool = (int(n_slots), int(nb), int(max_len), int(src_cap))

    def pool_admit(self, slots, enc_bf16: torch.Tensor, src_cu: np.ndarray) -> None:
        """Cross K/V of the newcomers (enc_bf16 [sum S_j, d_model] bf16 packed, host ``src_cu [m + 1]``) into the
        regions of ``slots`` (distinct, one per source)."""
        assert enc_bf16.dtype == torch.bfloat16 and enc_bf16.is_contiguous()
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        cu = np.ascontiguousarray(src_cu, dtype=np.int32)
        if len(cu) != len(sl) + 1 or enc_bf16.shape[0] != int(cu[-1]):
            raise _lib.HipLibraryError(f"pool_admit: {len(sl)} slots, {len(cu)} src_cu entries, {enc_bf16.shape[0]} "
                                       "encoder rows")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_decoder_pool_admit(self._handle, *self._pool, _pc(sl), enc_bf16.data_ptr(), _pc(cu),
                                                       len(sl), self._pool_ws.data_ptr(), self._pool_ws.numel(),
                                                       _lib.current_stream()), "rp_decoder_pool_admit")

    def pool_prefill(self, slots, src_len, rows) -> None:
        """``prefill_many`` for the slot pool (``rp_decoder_pool_prefill``, ``BeamSearchPool``'s ``prefill``): the prompt
        rows ``rows[j]`` of slot ``slots[j]``, admitted with a source of ``src_len[j]`` tokens."""
        self._prefill("pool_prefill", slots, rows, src_len)

    def pool_step(self, active, pos, src_len, tokens: torch.Tensor, ancestry: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """log-probs [n_active * nb, V] of one step for the slots ``active`` (distinct), slot ``active[a]`` at position
        ``pos[a]`` over a source of ``src_len[a]`` tokens; row ``a * nb + b`` is its beam ``b``, of whose ancestry row
        columns ``0..pos[a]`` are read (``BeamSearchPool``'s ``step``)."""
        return self._step("pool_step", active, tokens, ancestry, out, pos=pos, src_len=src_len)

    def sample_step(self, log_probs: torch.Tensor, active, t: int, state: SampleState, temperature: float = 1.0,
                    top_k: int = 0, top_p: float = 1.0, eos_token_id: int = 1, pad_token_id: int = 0) -> None:
        """One token per row of ``log_probs [n_active * nb, V]`` and the rows' books in ``state``, on the device
        (``rp_sample_step``; ``sample_search_batch``'s ``sample_step``).  Nothing is read back.  With ``state.params``
        set, every row takes its parameters from its own block of that table (``rp_sample_step_rows``) and the three
        arguments are not looked at."""
        self._sample("sample_step", log_probs, active, int(t), state, temperature, top_k, top_p, eos_token_id, pad_token_id)

    def _sample(self, what: str, log_probs: torch.Tensor, active, where, state: SampleState, temperature: float,
                top_k: int, top_p: float, eos_token_id: int, pad_token_id: int) -> None:
        """The one caller of the sampler's four entries: ``where`` an int, every state at that position
        (``rp_sample_step``), or a position per slot (``rp_sample_pool_step``); with ``state.params`` set the ``_rows``
        entry of either, which takes the table in place of the three scalars."""
        pool = not isinstance(where, int)
        entry = ("rp_sample_pool_step" if pool else "rp_sample_step") + ("" if state.params is None else "_rows")
        act = np.ascontiguousarray(active, dtype=np.int32)
        p = np.ascontiguousarray(where, dtype=np.int32) if pool else None
        n, nb, max_len = self._sample_books(state, entry)
        rows, V = log_probs.shape
        if rows != len(act) * nb or state.tokens.numel() < rows or (pool and len(p) != len(act)):
            raise _lib.HipLibraryError(f"{what}: {rows} rows" + (f", {len(p)} positions" if pool else "")
                                       + f" for {len(act)} states of {nb} samples")
        assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dtype == torch.float32
        head = (_pc(p), len(act), n, nb, state.seeds.data_ptr()) if pool else (len(act), n, nb, state.seeds.data_ptr(), where)
        how = (temperature, top_k, top_p) if state.params is None else (self._sample_table(state, entry),)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, entry)(log_probs.data_ptr(), V, _pc(act), *head, max_len, *how, eos_token_id,
                                                 pad_token_id, state.seq.data_ptr(), state.tokens.data_ptr(),
                                                 state.cum_logprob.data_ptr(), state.n_generated.data_ptr(),
                                                 state.finished.data_ptr(), _lib.current_stream()), entry)

    def beam_books(self, n: int, nb: int, max_len: int, eos_token_id: int = 1,
                   decoder_start_token_id: int = 0) -> BeamBooks:
        """Device books of a beam search over ``n`` states, initialised (``rp_beam_books_init``;
        ``beam_search_batch_device``'s ``init``)."""
        need = int(self._lib.rp_beam_books_bytes(n, nb, max_len))
        if need == 0:
            raise _lib.HipLibraryError("beam_books: " + self._lib.rp_last_error().decode(errors="replace"))
        books = BeamBooks(n, nb, max_len, block=torch.empty(need // 4, dtype=torch.int32, device=self.device))
        assert books.nbytes == need, (books.nbytes, need)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_beam_books_init(books.block.data_ptr(), need, n, nb, max_len, eos_token_id,
                                                    decoder_start_token_id, _lib.current_stream()), "rp_beam_books_init")
        return books

    def beam_advance(self, books: BeamBooks, active, t: int, scores: torch.Tensor, tokens: torch.Tensor,
                     parents: torch.Tensor, fin_div: float, run_div: float, eos_token_id: int = 1) -> None:
        """The books' update from one step's selected triples ``[n_active, 2 nb]``, on the device (``rp_beam_advance``;
        ``beam_search_batch_device``'s ``advance``).  Nothing is read back."""
        self._advance("beam_advance", books, active, int(t), scores, tokens, parents, float(fin_div), float(run_div),
                      eos_token_id)

    def _advance(self, what: str, books: BeamBooks, active, where, scores: torch.Tensor, tokens: torch.Tensor,
                 parents: torch.Tensor, fin_div, run_div, eos_token_id: int) -> None:
        """The one caller of the books' two update entries: ``where`` an int and the divisors floats
        (``rp_beam_advance``: every state at that position), or a position and a pair of divisors per slot
        (``rp_beam_pool_advance``)."""
        pool = not isinstance(where, int)
        entry = "rp_beam_pool_advance" if pool else "rp_beam_advance"
        act = np.ascontiguousarray(active, dtype=np.int32)
        want = (len(act), 2 * books.nb)
        for x, dt in ((scores, torch.float32), (tokens, torch.int32), (parents, torch.int32)):
            assert x.is_cuda and x.is_contiguous() and x.dtype == dt, f"{entry} takes contiguous device tensors"
            if tuple(x.shape) != want:
                raise _lib.HipLibraryError(f"{what}: triples of shape {tuple(x.shape)} for {want}")
        assert books.block.is_cuda
        if pool:
            p = np.ascontiguousarray(where, dtype=np.int32)
            fd, rd = (np.ascontiguousarray(x, dtype=np.float32) for x in (fin_div, run_div))
            if not len(p) == len(fd) == len(rd) == len(act):
                raise _lib.HipLibraryError(f"{what}: {len(p)} positions, {len(fd)} / {len(rd)} divisors for "
                                           f"{len(act)} slots")
            where, fin_div, run_div = (_pc(p), len(act)), _pc(fd), _pc(rd)
        else:
            where = (len(act), where)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, entry)(books.block.data_ptr(), books.nbytes, books.n, books.nb, books.max_len,
                                                 _pc(act), *where, scores.data_ptr(), tokens.data_ptr(),
                                                 parents.data_ptr(), fin_div, run_div, eos_token_id,
                                                 _lib.current_stream()), entry)

    # -- the slot pool's books: a position per slot (``generation.BeamBooksPool``'s callables) ---------------------------
    def beam_books_admit(self, books: BeamBooks, states, eos_token_id: int = 1, decoder_start_token_id: int = 0) -> None:
        """``_BeamState.__init__``'s values in the by-state parts of ``states`` only (``rp_beam_books_admit``)."""
        st = np.ascontiguousarray(states, dtype=np.int32)
        assert books.block.is_cuda
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_beam_books_admit(books.block.data_ptr(), books.nbytes, books.n, books.nb,
                                                     books.max_len, _pc(st), len(st), eos_token_id,
                                                     decoder_start_token_id, _lib.current_stream()), "rp_beam_books_admit")

    def beam_pool_advance(self, books: BeamBooks, active, pos, scores: torch.Tensor, tokens: torch.Tensor,
                          parents: torch.Tensor, fin_div, run_div, eos_token_id: int = 1) -> None:
        """``beam_advance`` with slot ``active[a]`` at its own position ``pos[a]`` and its own divisors
        (``rp_beam_pool_advance``).  Nothing is read back."""
        self._advance("beam_pool_advance", books, active, list(pos), scores, tokens, parents, fin_div, run_div, eos_token_id)

    def beam_books_rows(self, books: BeamBooks, active, pos) -> None:
        """The by-row inputs of the slots ``active`` (in that order) from their by-state parts (``rp_beam_books_rows``)."""
        act, p = (np.ascontiguousarray(x, dtype=np.int32) for x in (active, pos))
        if len(act) != len(p):
            raise _lib.HipLibraryError(f"beam_books_rows: {len(p)} positions for {len(act)} slots")
        assert books.block.is_cuda
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_beam_books_rows(books.block.data_ptr(), books.nbytes, books.n, books.nb,
                                                    books.max_len, _pc(act), _pc(p), len(act), _lib.current_stream()),
                       "rp_beam_books_rows")

    # -- the slot pool's sampler: a position per slot (``generation.SamplePool``'s callables) -----------------------------
    @staticmethod
    def _sample_books(state: SampleState, entry: str):
        for x in (state.seeds, state.seq, state.cum_logprob, state.n_generated, state.finished, state.tokens):
            assert x.is_cuda and x.is_contiguous(), f"{entry} takes contiguous device tensors"
        assert state.seeds.dtype == state.seq.dtype == state.tokens.dtype == torch.int32
        assert state.n_generated.dtype == state.finished.dtype == torch.int32 and state.cum_logprob.dtype == torch.float32
        return state.seq.shape

    @staticmethod
    def _sample_table(state: SampleState, entry: str) -> int:
        """The address of ``state.params``, the parameter table int32 ``[n, nb, 4]`` by (state, sample)."""
        n, nb, _ = state.seq.shape
        t = state.params
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int32, f"{entry} takes a contiguous int32 device table"
        if tuple(t.shape) != (n, nb, 4):
            raise _lib.HipLibraryError(f"{entry}: a parameter table of shape {tuple(t.shape)} for {(n, nb, 4)}")
        return t.data_ptr()

    def sample_pool_step(self, log_probs: torch.Tensor, active, pos, state: SampleState, temperature: float = 1.0,
                         top_k: int = 0, top_p: float = 1.0, eos_token_id: int = 1, pad_token_id: int = 0) -> None:
        """``sample_step`` with slot ``active[a]`` at its own position ``pos[a]`` (``rp_sample_pool_step``;
        ``SamplePool``'s ``sample_step``).  Nothing is read back.  With ``state.params`` set:
        ``rp_sample_pool_step_rows``, as in ``sample_step``."""
        self._sample("sample_pool_step", log_probs, active, list(pos), state, temperature, top_k, top_p, eos_token_id,
                     pad_token_id)

    def sample_books_admit(self, state: SampleState, states, seeds, decoder_start_token_id: int = 0,
                           pad_token_id: int = 0, n_live=None, params: Optional[torch.Tensor] = None) -> None:
        """Fresh books for the next tenants of ``states`` with their 32-bit ``seeds`` (``rp_sample_pool_admit``).
        ``n_live`` (a count in ``1..nb`` per state): the rows from there on start finished
        (``rp_sample_pool_admit_rows``).  ``params`` (host int32 ``[len(states), nb, 4]``): the tenants' blocks of
        ``state.params``, written in one host-to-device copy - the blocks travel with their state indices in one buffer
        and are scattered on the device - and no other block."""
        st = np.ascontiguousarray(states, dtype=np.int32)
        sd = np.array([int(x) & 0xFFFFFFFF for x in seeds], dtype=np.uint32)
        n, nb, max_len = self._sample_books(state, "rp_sample_pool_admit")
        if len(sd) != len(st):
            raise _lib.HipLibraryError(f"sample_books_admit: {len(sd)} seeds for {len(st)} states")
        if params is not None:
            self._sample_table(state, "sample_books_admit")
            m = len(st)
            if tuple(params.shape) != (m, nb, 4) or params.dtype != torch.int32 or params.is_cuda:
                raise _lib.HipLibraryError(f"sample_books_admit: host int32 blocks of shape {(m, nb, 4)} expected, got "
                                           f"{tuple(params.shape)} {params.dtype}")
            if not all(0 <= int(s) < n for s in st) or len(set(st.tolist())) != m:
                raise _lib.HipLibraryError(f"sample_books_admit: states {st.tolist()} not distinct in [0, {n})")
            packed = torch.cat([params.reshape(m, nb * 4), torch.from_numpy(st).reshape(m, 1)], dim=1)
            dev = packed.to(state.params.device)  # the admission's one upload
            state.params.index_copy_(0, dev[:, -1].long(), dev[:, :-1].reshape(m, nb, 4))
        if n_live is not None:
            nl = np.ascontiguousarray(n_live, dtype=np.int32)
            if len(nl) != len(st):
                raise _lib.HipLibraryError(f"sample_books_admit: {len(nl)} live-row counts for {len(st)} states")
            with torch.cuda.device(self.device):
                _lib.check(self._lib.rp_sample_pool_admit_rows(_pc(st), _pc(sd), _pc(nl), len(st), n, nb, max_len,
                                                               decoder_start_token_id, pad_token_id,
                                                               state.seeds.data_ptr(), state.seq.data_ptr(),
                                                               state.cum_logprob.data_ptr(), state.n_generated.data_ptr(),
                                                               state.finished.data_ptr(), _lib.current_stream()),
                           "rp_sample_pool_admit_rows")
            return
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_sample_pool_admit(_pc(st), _pc(sd), len(st), n, nb, max_len, decoder_start_token_id,
                                                      pad_token_id, state.seeds.data_ptr(), state.seq.data_ptr(),
                                                      state.cum_logprob.data_ptr(), state.n_generated.data_ptr(),
                                                      state.finished.data_ptr(), _lib.current_stream()),
                       "rp_sample_pool_admit")

    def sample_books_rows(self, state: SampleState, active, pos) -> None:
        """The next step's tokens of the slots ``active`` (in that order) from their ``seq`` rows (``rp_sample_pool_rows``)."""
        act, p = (np.ascontiguousarray(x, dtype=np.int32) for x in (active, pos))
        n, nb, max_len = self._sample_books(state, "rp_sample_pool_rows")
        if len(act) != len(p) or state.tokens.numel() < len(act) * nb:
            raise _lib.HipLibraryError(f"sample_books_rows: {len(p)} positions for {len(act)} slots of {nb} samples")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_sample_pool_rows(_pc(act), _pc(p), len(act), n, nb, max_len, state.seq.data_ptr(),
                                                     state.tokens.data_ptr(), _lib.current_stream()),
                       "rp_sample_pool_rows")

    # -- constrained decoding (``generation``'s ``mask`` callables) ------------------------------------------------------
    def _constraint_table(self, constraint, log_probs: torch.Tensor) -> torch.Tensor:
        assert log_probs.is_cuda and log_probs.is_contiguous() and log_probs.dtype == torch.float32
        table = constraint.device_table(self.device)
        if table.shape[1] != log_probs.shape[1]:
            raise ValueError(f"a constraint over {table.shape[1]} ids for a model of {log_probs.shape[1]}")
        return table

    def constraint_mask(self, log_probs: torch.Tensor, q_rows: torch.Tensor, constraint) -> torch.Tensor:
        """``-inf`` (in place) into the entries of ``log_probs [rows, V]`` that ``constraint`` forbids in state
        ``q_rows[r]`` (device int32 ``[rows]``), every other bit as it was (``rp_constraint_mask``; the host-books
        loops' ``mask``).  Returns ``log_probs``."""
        table = self._constraint_table(constraint, log_probs)
        rows, V = log_probs.shape
        q = q_rows.to(device=self.device, dtype=torch.int32).contiguous()
        if q.numel() != rows:
            raise _lib.HipLibraryError(f"constraint_mask: {q.numel()} states for {rows} rows")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_constraint_mask(log_probs.data_ptr(), V, rows, q.data_ptr(), table.data_ptr(),
                                                    table.shape[0], _lib.current_stream()), "rp_constraint_mask")
        return log_probs

    def constraint_mask_step(self, log_probs: torch.Tensor, active, pos, tokens_in: torch.Tensor, q: torch.Tensor,
                             constraint) -> torch.Tensor:
        """The sampled loops' ``mask`` (``rp_constraint_mask_step``): the automaton states ``q`` (device int32
        ``[n, nb]`` by (state, sample)) of the slots ``active`` advance by the tokens the step was fed (``tokens_in``, by
        row; slot ``active[a]`` at ``pos[a]``, position 0 starting over) and mask the rows.  Nothing is read back."""
        table = self._constraint_table(constraint, log_probs)
        act, p = (np.ascontiguousarray(x, dtype=np.int32) for x in (active, pos))
        n, nb = q.shape
        rows, V = log_probs.shape
        for x in (q, tokens_in):
            assert x.is_cuda and x.is_contiguous() and x.dtype == torch.int32, "rp_constraint_mask_step takes int32 device tensors"
        if rows != len(act) * nb or len(p) != len(act) or tokens_in.numel() < rows:
            raise _lib.HipLibraryError(f"constraint_mask_step: {rows} rows, {len(p)} positions, {tokens_in.numel()} tokens "
                                       f"for {len(act)} states of {nb} samples")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_constraint_mask_step(log_probs.data_ptr(), V, _pc(act), _pc(p), len(act), n, nb,
                                                         tokens_in.data_ptr(), q.data_ptr(), table.data_ptr(),
                                                         table.shape[0], _lib.current_stream()),
                       "rp_constraint_mask_step")
        return log_probs

    def select_many(self, log_probs: torch.Tensor, running: torch.Tensor, nb: int, k: int):
        """Per state the device top-k of its own ``[nb * V]`` block (``rp_beam_select_batch``): scores, tokens, parents,
        each ``[n_active, k]``, parents local to the state."""
        rows, V = log_probs.shape
        na = rows // nb
        need = rows * min(k, V) * 8
        if self._sel_ws is None or self._sel_ws.numel() < need:
            self._sel_ws = torch.empty(max(need, 64 * 128 * 8), dtype=torch.uint8, device=self.device)
        run = running.to(device=self.device, dtype=torch.float32).contiguous()
        lp = log_probs.contiguous()
        scores = torch.empty((na, k), dtype=torch.float32, device=self.device)
        toks = torch.empty((na, k), dtype=torch.int32, device=self.device)
        par = torch.empty((na, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rp_beam_select_batch(lp.data_ptr(), run.data_ptr(), na, nb, V, k, scores.data_ptr(),
                                                      toks.data_ptr(), par.data_ptr(), self._sel_ws.data_ptr(),
                                                      self._sel_ws.numel(), _lib.current_stream()),
                       "rp_beam_select_batch")
        return scores, toks, par


def packed_pairs(cfg: Dict, state_ids, state_mask, tactic_ids):
    """The reference's padded (state_ids, state_mask, tactic_ids) batch as packed pairs: (source ids [sum S_b], src_cu,
    decoder input tokens, labels, tgt_cu), the form the encoder passes and ``rp_decoder_forward`` /
    ``rp_decoder_loss_grad`` take."""
    ids = np.asarray(state_ids.cpu() if isinstance(state_ids, torch.Tensor) else state_ids).astype(np.int64)
    n_src = source_lengths(state_mask)
    if ids.shape != tuple(state_mask.shape):
        raise ValueError(f"state_ids {ids.shape} and state_mask {tuple(state_mask.shape)} disagree")
    tokens, labels, tgt_cu = shift_and_segment(tactic_ids, cfg.get("decoder_start_token_id", 0), 0)
    if len(tgt_cu) - 1 != len(n_src):
        raise ValueError("state_ids and tactic_ids hold different batch sizes")
    if (labels >= cfg["vocab_size"]).any():
        raise ValueError(f"tactic_ids holds ids >= vocab_size={cfg['vocab_size']}")
    if ((np.diff(tgt_cu) > 0) & (n_src == 0)).any():
        raise ValueError("a pair with counted labels has an empty source")
    src_cu = np.concatenate([[0], np.cumsum(n_src)]).astype(np.int32)
    packed = np.concatenate([ids[b, :n] for b, n in enumerate(n_src)]) if len(n_src) else np.zeros(0)
    return packed, src_cu, tokens, labels, tgt_cu


class HipT5Generator:
    """Encoder + decoder of one T5ForConditionalGeneration checkpoint on one GPU."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device):
        self.cfg = dict(cfg)
        self.device = _require_gpu(device)
        enc_sd = {k: v for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
        self.encoder = HipT5Encoder(cfg, enc_sd, self.device, keep_master_weights=False)
        self.decoder = HipT5Decoder(cfg, sd, self.device)

    @classmethod
    def from_pretrained(cls, path: str, device) -> "HipT5Generator":
        cfg, sd = load_seq2seq_checkpoint(path)
        return cls(cfg, sd, device)

    @classmethod
    def from_parts(cls, cfg: Dict, encoder: HipT5Encoder, decoder: "HipT5Decoder", device) -> "HipT5Generator":
        """A generator over engines that live elsewhere (``HipSeq2SeqTrainer.generator``: the trainer's inference
        encoder and its decoder): no second copy of any weight; whoever refreshes those engines refreshes this."""
        self = cls.__new__(cls)
        self.cfg, self.device = dict(cfg), _require_gpu(device)
        self.encoder, self.decoder = encoder, decoder
        return self

    def encode_hidden(self, ids: np.ndarray) -> torch.Tensor:
        """last_hidden_state [S, d_model] bf16 of one source (int ids including the final EOS)."""
        ids = np.asarray(ids, dtype=np.int32)
        S = int(ids.size)
        enc = self.encoder
        ids_d = torch.from_numpy(ids).to(self.device)
        cu = torch.tensor([0, S], dtype=torch.int32, device=self.device)
        out = torch.empty((S, self.cfg["d_model"]), dtype=torch.bfloat16, device=self.device)
        n = enc._lib.rp_encoder_workspace_bytes(enc._handle, S, 1)
        ws = enc._workspace(n)
        with torch.cuda.device(self.device):
            _lib.check(enc._lib.rp_encode_hidden(enc._handle, ids_d.data_ptr(), cu.data_ptr(), 1, S, S, out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "rp_encode_hidden")
        return out

    def encode_hidden_packed(self, ids: np.ndarray, cu: np.ndarray) -> torch.Tensor:
        """last_hidden_state [sum S_b, d_model] bf16 of several sources packed varlen (``rp_encode_hidden``)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        cu = np.ascontiguousarray(cu, dtype=np.int32)
        B, S = len(cu) - 1, int(cu[-1])
        enc = self.encoder
        out = torch.empty((S, self.cfg["d_model"]), dtype=torch.bfloat16, device=self.device)
        if S == 0:
            return out
        ids_d = torch.from_numpy(ids).to(self.device)
        cu_d = torch.from_numpy(cu).to(self.device)
        max_len = int(np.diff(cu).max())
        ws = enc._workspace(enc._lib.rp_encoder_workspace_bytes(enc._handle, S, B))
        with torch.cuda.device(self.device):
            _lib.check(enc._lib.rp_encode_hidden(enc._handle, ids_d.data_ptr(), cu_d.data_ptr(), B, S, max_len,
                                                 out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "rp_encode_hidden")
        return out

    def loss_and_grads(self, state_ids, state_mask, tactic_ids):
        """(loss, gradients, d_enc) of ``forward``'s loss (``rp_decoder_loss_grad``; no dropout).
        ``gradients`` maps the HF state-dict names of the decoder's parameters (``shared.weight``, ``lm_head.weight``
        when the head is untied, ``decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight``,
        ``decoder.final_layer_norm.weight``, ``decoder.block.i.layer...``) to fp32 views of one flat device buffer;
        ``d_enc`` is d loss / d encoder_last_hidden_state packed ``[sum S_b, d_model]`` fp32.  With no counted label the
        loss is NaN and every gradient 0."""
        packed, src_cu, tokens, labels, tgt_cu = packed_pairs(self.cfg, state_ids, state_mask, tactic_ids)
        S = int(src_cu[-1])
        enc = self.encode_hidden_packed(packed, src_cu) if S else torch.empty((0, self.cfg["d_model"]),
                                                                              dtype=torch.bfloat16, device=self.device)
        _, (s, c), flat, d_enc = self.decoder.loss_grad(enc, src_cu, tokens, labels, tgt_cu, want_d_enc=True)
        names, off = self.decoder.grad_layout()
        shapes = self.decoder.grad_shapes()
        grads = {n: flat[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))].view(shapes[n]) for i, n in enumerate(names)}
        return (s / c if c else float("nan")), grads, d_enc

    def _teacher_forced(self, state_ids, state_mask, tactic_ids, rows: bool = False):
        packed, src_cu, tokens, labels, tgt_cu = packed_pairs(self.cfg, state_ids, state_mask, tactic_ids)
        enc = self.encode_hidden_packed(packed, src_cu) if int(tgt_cu[-1]) else None
        lp, sc, lp_rows = self.decoder.forward(enc, src_cu, tokens, labels, tgt_cu, rows)
        return lp, tgt_cu, sc, lp_rows

    def forward(self, state_ids, state_mask, tactic_ids) -> float:
        """``T5ForConditionalGeneration(input_ids, attention_mask, labels=tactic_ids).loss``: the mean of -log p over the
        labels that are not -100 (NaN when there are none).  Padded int tensors as the reference's collate makes them."""
        _, _, (s, c), _ = self._teacher_forced(state_ids, state_mask, tactic_ids)
        return s / c if c else float("nan")

    def label_log_probs(self, state_ids, state_mask, tactic_ids) -> torch.Tensor:
        """Per-token log p(label) [B, T] fp32 (on the device), 0 where the label is -100."""
        lp, tgt_cu, _, _ = self._teacher_forced(state_ids, state_mask, tactic_ids)
        B, T = np.asarray(tactic_ids.shape if isinstance(tactic_ids, torch.Tensor) else np.shape(tactic_ids))
        out = torch.zeros((int(B), int(T)), dtype=torch.float32, device=self.device)
        for b in range(int(B)):
            n = int(tgt_cu[b + 1] - tgt_cu[b])
            out[b, :n] = lp[int(tgt_cu[b]) : int(tgt_cu[b]) + n]
        return out

    @property
    def _eos(self) -> int:
        return self.cfg.get("eos_token_id", 1)

    @property
    def _start(self) -> int:
        return self.cfg.get("decoder_start_token_id", 0)

    @staticmethod
    def _prefix(prefix) -> Optional[List[int]]:
        """A prefix (token ids after the start token; None or empty: none) as a list, or None."""
        return _prompt_tokens(prefix) or None

    @staticmethod
    def _check_prefixes(prefixes, n: int, max_length: int):
        """``prefixes`` (None, or one entry or None per source) as lists; None when no source has one."""
        return _check_prompts(prefixes, n, max_length, "prefixes", "sources")

    def _constrained(self, constraint, fused: bool = False) -> Dict:
        """The loops' ``constraint=`` / ``mask=`` keywords for ``constraint`` (None: none): the decoder's
        ``rp_constraint_mask`` launch, or with ``fused`` its ``rp_constraint_mask_step``."""
        if constraint is None:
            return {}
        dec = self.decoder
        if constraint.vocab != dec.V or constraint.eos != self._eos:
            raise ValueError(f"a constraint over {constraint.vocab} ids with eos={constraint.eos} for a model of "
                             f"{dec.V} ids with eos={self._eos}")
        if fused:
            return dict(constraint=constraint, mask=lambda lp, active, pos, tokens, q: dec.constraint_mask_step(
                lp, active, pos, tokens, q, constraint))
        return dict(constraint=constraint, mask=lambda lp, q_rows: dec.constraint_mask(lp, q_rows, constraint))

    def greedy(self, ids: np.ndarray, max_length: int, prefix=None, constraint=None) -> BeamSearchOutput:
        """``generate(input_ids, num_beams=1, max_length)``: HF's greedy search (argmax, ties to the lowest id), not a
        one-beam beam search.  ``prefix`` / ``constraint``: as in ``generate``."""
        if self._check_prefixes([prefix], 1, max_length) is not None:
            return self.greedy_many([ids], max_length, prefixes=[prefix], constraint=constraint)[0]
        kw = self._constrained(constraint)
        enc = self.encode_hidden(ids)
        self.decoder.start(enc, 1, max_length)
        return greedy_search(self.decoder.step, max_length, eos_token_id=self._eos,
                             decoder_start_token_id=self._start, device=self.device, **kw)

    def generate(self, ids: np.ndarray, num_beams: int, max_length: int, length_penalty: float = 1.0,
                 trace: Optional[list] = None, sync_every: Optional[int] = None, prefix=None,
                 constraint=None) -> BeamSearchOutput:
        """``generate(input_ids, num_beams=n, num_return_sequences=n, length_penalty, max_length, early_stopping=False,
        do_sample=False)`` for one source.  Reads the selected candidates back once per step (generation.py);
        ``sync_every``: as in ``generate_many``, whose one-state call it then is.

        ``prefix`` (token ids; None or empty: none): HF's ``decoder_input_ids = [start] + prefix`` - every returned
        sequence begins with it, ``max_length`` counts it, the scores sum the generated tokens only.  Its cache rows are
        written in one pass (``rp_decoder_batch_prefill``, DESIGN.md section 9 "Tactic prefix"); host books only.

        ``constraint`` (a ``constraint.ByteAutomaton``; None: none): HF's ``prefix_allowed_tokens_fn`` walking that
        automaton - one ``rp_constraint_mask`` launch between every step and its selection writes ``-inf`` over the
        forbidden log-probs (DESIGN.md section 9 "Constrained decoding").  A prefix the automaton rejects is a
        ``ValueError``; host books only (``ValueError`` with ``sync_every``)."""
        if constraint is not None and sync_every is not None:
            raise ValueError("a constraint together with the device books (sync_every) is not built yet")
        if self._check_prefixes([prefix], 1, max_length) is not None:
            traces = None if trace is None else []
            out, = self.generate_many([ids], num_beams, max_length, length_penalty, traces=traces, sync_every=sync_every,
                                      prefixes=[prefix], constraint=constraint)
            if trace is not None:
                trace.extend(traces[0])
            return out
        if sync_every is not None:
            if trace is not None:
                raise ValueError("trace= needs the host books: it cannot be combined with sync_every")
            return self.generate_many([ids], num_beams, max_length, length_penalty, sync_every=sync_every)[0]
        kw = self._constrained(constraint)
        enc = self.encode_hidden(ids)
        self.decoder.start(enc, num_beams, max_length)
        return beam_search(self.decoder.step, num_beams, max_length, length_penalty,
                           eos_token_id=self._eos,
                           decoder_start_token_id=self._start,
                           select=self.decoder.select, device=self.device, trace=trace, **kw)

    def _start_many(self, sources, num_beams: int, max_length: int) -> int:
        srcs = [np.asarray(x, dtype=np.int32).reshape(-1) for x in sources]
        if not srcs:
            raise ValueError("generate_many needs at least one source")
        cu = np.concatenate([[0], np.cumsum([len(x) for x in srcs])]).astype(np.int32)
        enc = self.encode_hidden_packed(np.concatenate(srcs), cu)
        self.decoder.start_many(enc, cu, num_beams, max_length)
        return len(srcs)

    def greedy_many(self, sources, max_length: int, prefixes=None, constraint=None) -> List[BeamSearchOutput]:
        """``greedy`` for several sources through one decode loop: entry ``i`` is ``greedy(sources[i], max_length)`` bit
        for bit, whichever other sources share the call.  ``prefixes`` / ``constraint`` (one automaton, shared by every
        source): as in ``generate_many``."""
        sources = list(sources)
        prefixes = self._check_prefixes(prefixes, len(sources), max_length)
        ckw = self._constrained(constraint)
        if constraint is not None:
            for p in prefixes or []:
                constraint.state_after(p)  # a rejected prefix: ValueError before anything is launched
        n = self._start_many(sources, 1, max_length)
        kw = dict(ckw, **({} if prefixes is None else dict(prompts=prefixes, prefill_many=self.decoder.prefill_many)))
        return greedy_search_batch(self.decoder.step_many, n, max_length, eos_token_id=self._eos,
                                   decoder_start_token_id=self._start, device=self.device,
                                   **kw)

    def generate_many(self, sources, num_beams: int, max_length: int, length_penalty: float = 1.0,
                      traces: Optional[list] = None, sync_every: Optional[int] = None,
                      prefixes=None, constraint=None) -> List[BeamSearchOutput]:
        """``generate`` for several sources at once: one packed encoder pass, one cross-K/V GEMM and one decode loop that
        runs until the last state stops, with one readback per step.  Entry ``i`` equals ``generate(sources[i], ...)``
        bit for bit (sequences, scores and, in ``traces[i]``, every step's selected triples), whichever other sources
        share the call, in whatever order, and whenever they finish.

        ``sync_every`` (an integer >= 1; the default None is the loop above): the books live on the device
        (``rp_beam_advance``, DESIGN.md section 9 "device books"), nothing is uploaded or read back per position, and the
        states' stop flags are read every ``sync_every`` positions.  The outputs are the same sequences and scores.

        ``prefixes`` (None, or one token id sequence or None per source): source ``i``'s decoder prompt after the start
        token (``generate``'s ``prefix``).  All prompts' cache rows are written by one ``rp_decoder_batch_prefill``, then
        state ``i`` searches from position ``len(prefixes[i])`` (``rp_decoder_batch_step_pos``).  Entry ``i`` equals
        ``generate(sources[i], ..., prefix=prefixes[i])`` bit for bit.  Together with ``sync_every`` a ``ValueError``:
        the device books with a prompt are not built yet.

        ``constraint``: ``generate``'s, one automaton shared by every source; entry ``i`` equals
        ``generate(sources[i], ..., constraint=constraint)`` bit for bit.  With ``sync_every`` a ``ValueError``."""
        sources = list(sources)
        prefixes = self._check_prefixes(prefixes, len(sources), max_length)
        if prefixes is not None and sync_every is not None:
            raise ValueError("a decoder prompt together with the device books (sync_every) is not built yet")
        if constraint is not None and sync_every is not None:
            raise ValueError("a constraint together with the device books (sync_every) is not built yet")
        ckw = self._constrained(constraint)
        if constraint is not None:
            for p in prefixes or []:
                constraint.state_after(p)  # a rejected prefix: ValueError before anything is launched
        if sync_every is not None:
            if traces is not None:
                raise ValueError("traces= needs the host books: it cannot be combined with sync_every")
            sync_every = _check_count("sync_every", sync_every, " (or None)")
            _check_room(max_length)
        n = self._start_many(sources, num_beams, max_length)
        if sync_every is not None:
            dec = self.decoder
            return beam_search_batch_device(
                lambda active, tokens, ancestry, t: dec.step_many(active, tokens, ancestry, t=t), dec.select_many,
                dec.beam_advance, n, num_beams, max_length, length_penalty, eos_token_id=self._eos,
                decoder_start_token_id=self._start, sync_every=sync_every,
                device=self.device, init=dec.beam_books)
        kw = dict(ckw, **({} if prefixes is None else dict(prompts=prefixes, prefill_many=self.decoder.prefill_many)))
        return beam_search_batch(self.decoder.step_many, n, num_beams, max_length, length_penalty,
                                 eos_token_id=self._eos,
                                 decoder_start_token_id=self._start,
                                 select_many=self.decoder.select_many, device=self.device, traces=traces, **kw)

    def generate_stream(self, num_beams: int, max_length: int, length_penalty: float = 1.0,
                        n_slots: Optional[int] = None, src_cap: int = 2048,
                        sync_every: Optional[int] = None, constraint=None) -> "GenerateStream":
        """A running beam search that sources join while it runs (continuous batching): a
        ``GenerateStream`` of ``n_slots`` places (default ``HipT5Decoder.max_states(num_beams)``) for sources of at most
        ``src_cap`` tokens.  Every ticket's output is ``generate(source, num_beams, max_length, length_penalty)`` bit for
        bit.  The decoder carries one stream at a time: opening another retires this one.

        ``sync_every`` (an integer >= 1; the default None is the host-books pool): the slots' books live on the device
        (``generation.BeamBooksPool``, ``rp_beam_pool_advance``), nothing is uploaded or read back per step, and the
        stop flags are read every ``sync_every`` steps.  The same outputs; with ``sync_every = K > 1`` a result is
        delivered, and its slot taken again, up to ``K - 1`` steps after its state stopped.

        ``constraint``: ``generate``'s, one automaton for the whole stream; every ticket's output is
        ``generate(source, ..., constraint=constraint)`` bit for bit.  With ``sync_every`` a ``ValueError``."""
        if constraint is not None and sync_every is not None:
            raise ValueError("a constraint together with the device books (sync_every) is not built yet")
        ckw = self._constrained(constraint)
        if sync_every is not None:
            sync_every = _check_count("sync_every", sync_every, " (or None)")
            _check_room(max_length)
        return GenerateStream(self, num_beams, max_length, length_penalty,
                              self.decoder.max_states(num_beams) if n_slots is None else n_slots, src_cap, sync_every,
                              **ckw)

    def sample(self, ids: np.ndarray, num_samples: int, max_length: int, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, seed: int = 0, length_penalty: float = 0.0, sync_every: int = 16,
               params: Optional[SamplingParams] = None, constraint=None) -> BeamSearchOutput:
        """``num_samples`` sampled continuations of one source (``sample_many`` with one state; ``params``: this
        source's ``SamplingParams`` in place of the three scalars; ``constraint``: as there)."""
        return self.sample_many([ids], num_samples, max_length, temperature, top_k, top_p, [seed], length_penalty,
                                sync_every, None if params is None else [params], constraint=constraint)[0]

    def sample_many(self, sources, num_samples: int, max_length: int, temperature: float = 1.0, top_k: int = 0,
                    top_p: float = 1.0, seeds=None, length_penalty: float = 0.0,
                    sync_every: int = 16, params=None, constraint=None) -> List[BeamSearchOutput]:
        """Temperature / top-k / top-p sampling (``generate(do_sample=True, num_return_sequences=num_samples)``'s warper
        chain with a stated order and random number, DESIGN.md section 9 "Sampling") for several sources through one
        decode loop with no per-step readback.  ``seeds[i]`` (default ``0..n-1``) is source ``i``'s 32-bit seed.  Entry
        ``i`` equals ``sample(sources[i], ..., seed=seeds[i])`` bit for bit, tokens and scores, whichever states share
        the call, in whatever order, for any ``sync_every``.  Rows come in sample order; ``sequences_scores`` is the
        sum of the model's log-probs of the drawn tokens divided by ``n_generated ** length_penalty``.

        ``params`` (default None: the path above, ``rp_sample_step``): a sequence with one ``SamplingParams`` or None per
        source, None standing for the call's ``temperature`` / ``top_k`` / ``top_p``.  The sources' blocks form the
        parameter table, uploaded once, and every step is ``rp_sample_step_rows``: row ``b`` of entry ``i`` is the same
        bits as row ``b`` of ``sample(sources[i], ...)`` at that row's own three values (DESIGN.md section 9,
        "Sampling parameters per request").

        ``constraint`` (a ``constraint.ByteAutomaton``, shared by every source; None: none): the rows' automaton states
        live on the device and one ``rp_constraint_mask_step`` launch between every step and the sampler advances them
        and writes ``-inf`` over the forbidden log-probs, which the sampler then gives no mass (DESIGN.md section 9
        "Constrained decoding").  Nothing is read back; the scores stay sums of the model's own log-probs."""
        check_sampling(temperature, top_k, top_p)
        if num_samples < 1 or max_length <= 1:
            raise ValueError(f"num_samples={num_samples} (>= 1), max_length={max_length} (>= 2)")
        if sync_every < 1:
            raise ValueError(f"sync_every={sync_every} must be >= 1")
        ckw = self._constrained(constraint, fused=True)
        sources = list(sources)
        table = None
        if params is not None:
            params = list(params)
            if len(params) != len(sources) or not sources:
                raise ValueError(f"{len(params)} entries of params for {len(sources)} sources")
            own = SamplingParams(temperature, top_k, top_p)
            table = torch.stack([(own if q is None else q).rows(num_samples) for q in params])
        seeds = list(range(len(sources))) if seeds is None else [int(x) for x in seeds]
        if len(seeds) != len(sources):
            raise ValueError(f"{len(seeds)} seeds for {len(sources)} sources")
        if not sources or len(sources) > self.decoder.max_states(num_samples):
            raise ValueError(f"sample_many takes 1..{self.decoder.max_states(num_samples)} sources at "
                             f"{num_samples} samples, got {len(sources)}")
        n = self._start_many(sources, num_samples, max_length)
        eos = self._eos
        dec = self.decoder
        return sample_search_batch(
            lambda active, tokens, ancestry, t: dec.step_many(active, tokens, ancestry, t=t),
            lambda lp, active, t, state: dec.sample_step(lp, active, t, state, temperature, int(top_k), top_p, eos, 0),
            n, num_samples, max_length, seeds, length_penalty, eos_token_id=eos,
            decoder_start_token_id=self._start, pad_token_id=0, sync_every=sync_every,
            device=self.device, params=table, **ckw)

    def sample_stream(self, num_samples: int, max_length: int, temperature: float = 1.0, top_k: int = 0,
                      top_p: float = 1.0, length_penalty: float = 0.0, n_slots: Optional[int] = None, src_cap: int = 2048,
                      sync_every: int = 16, per_request: bool = False, constraint=None) -> "SampleStream":
        """A running sampled search that sources join while it runs (continuous batching): a
        ``SampleStream`` of ``n_slots`` places (default ``HipT5Decoder.max_states(num_samples)``) for sources of at most
        ``src_cap`` tokens, its books on the device (``generation.SamplePool``, ``rp_sample_pool_step``), nothing uploaded
        or read back per step, the finished flags read every ``sync_every`` steps.  Every ticket's output is
        ``sample(source, num_samples, max_length, temperature, top_k, top_p, seed, length_penalty)`` bit for bit, tokens
        and scores, whichever sources share the stream, in whatever order and slots.  The decoder carries one stream at a
        time, of either kind: opening another retires this one.

        The sampling parameters are the stream's unless ``per_request=True``: then ``submit(ids, seed, params,
        num_samples)`` takes a ``SamplingParams`` per ticket (None: the stream's three) and any ``1 <= num_samples <=``
        the stream's (None: the stream's), and the ticket's output is ``sample(source, that num_samples, ..., seed,
        params=those)``, bit for bit.  The stream then carries the parameter table on the device
        (``rp_sample_pool_step_rows``), written at admission only.

        ``constraint``: ``sample_many``'s, one automaton for the whole stream (``rp_constraint_mask_step`` with the
        slots' own positions; a slot's next tenant starts in the start state at its position 0)."""
        check_sampling(temperature, top_k, top_p)
        ckw = self._constrained(constraint, fused=True)
        if num_samples < 1 or max_length <= 1:
            raise ValueError(f"num_samples={num_samples} (>= 1), max_length={max_length} (>= 2)")
        sync_every = _check_count("sync_every", sync_every)
        if n_slots is not None:
            _check_count("n_slots", n_slots, " (or None)")
        return SampleStream(self, num_samples, max_length, temperature, int(top_k), top_p, length_penalty,
                            self.decoder.max_states(num_samples) if n_slots is None else n_slots, src_cap, sync_every,
                            bool(per_request), **ckw)


class GenerateStream:
    """``HipT5Generator.generate_stream``'s object: ``generation.BeamSearchPool`` over the decoder's slot pool.
    ``submit(ids)`` queues a source and returns its ticket; ``step()`` admits what fits (the newcomers encoded together,
    one packed encoder pass), takes one decode step and returns the ``(ticket, BeamSearchOutput)`` pairs that finished;
    ``drain()`` steps until the stream is idle.  ``in_flight`` / ``queued`` / ``steps`` are the pool's.  With
    ``sync_every`` the pool is ``generation.BeamBooksPool``: the books on the device, the pairs delivered at its sync
    points."""

    def __init__(self, generator: HipT5Generator, num_beams: int, max_length: int, length_penalty: float, n_slots: int,
                 src_cap: int, sync_every: Optional[int] = None, constraint=None, mask=None):
        dec = self._open(generator, n_slots, num_beams, max_length, src_cap)
        kw = dict(eos_token_id=generator._eos, decoder_start_token_id=generator._start, select_many=dec.select_many,
                  device=generator.device)
        if sync_every is not None:
            self.pool = BeamBooksPool(self._admit, self._step, n_slots, num_beams, max_length, length_penalty,
                                      sync_every=sync_every, books_admit=dec.beam_books_admit,
                                      advance=dec.beam_pool_advance, rows=dec.beam_books_rows, constraint=constraint,
                                      **kw)  # (with a constraint: BeamBooksPool's own refusal)
        else:
            self.pool = BeamSearchPool(self._admit, self._step, n_slots, num_beams, max_length, length_penalty,
                                       prefill=self._prefill, **kw,
                                       **({} if constraint is None else dict(constraint=constraint, mask=mask)))

    def _open(self, generator: HipT5Generator, n_slots: int, nb: int, max_length: int, src_cap: int) -> HipT5Decoder:
        """Take the decoder's slot pool (beam and sample streams alike: whoever held it is retired)."""
        self.generator, self.src_cap = generator, int(src_cap)
        dec = self.decoder = generator.decoder
        dec.pool_open(n_slots, nb, max_length, src_cap)
        dec._pool_owner = self
        self._src_len = [0] * int(n_slots)  # per slot: the source length of its tenant
        return dec

    def _mine(self) -> HipT5Decoder:
        if getattr(self.decoder, "_pool_owner", None) is not self:
            raise RuntimeError("this stream was retired: the decoder's slot pool was opened again")
        return self.decoder

    def _admit(self, slots, sources) -> None:
        cu = np.concatenate([[0], np.cumsum([len(x) for x in sources])]).astype(np.int32)
        enc = self.generator.encode_hidden_packed(np.concatenate(sources), cu)
        self._mine().pool_admit(slots, enc, cu)
        for s, x in zip(slots, sources):
            self._src_len[s] = len(x)

    def _prefill(self, slots, rows) -> None:
        self._mine().pool_prefill(slots, [self._src_len[s] for s in slots], rows)

    def _step(self, active, pos, tokens, ancestry) -> torch.Tensor:
        return self._mine().pool_step(active, pos, [self._src_len[s] for s in active], tokens, ancestry)

    def _source(self, ids) -> np.ndarray:
        ids = np.asarray(ids, dtype=np.int32).reshape(-1)
        if not 1 <= ids.size <= self.src_cap:
            raise ValueError(f"a source of {ids.size} tokens does not fit the stream's src_cap={self.src_cap} (1..src_cap)")
        return ids

    def submit(self, ids, prefix=None) -> int:
        """Queue a source.  ``prefix`` (token ids; None or empty: none): the ticket's decoder prompt, as in
        ``HipT5Generator.generate``; its cache rows are written in one pass at admission
        (``rp_decoder_pool_prefill``).  Host-books stream only: with ``sync_every`` a ``ValueError``."""
        prefix = HipT5Generator._prefix(prefix)
        if prefix is None:
            return self.pool.submit(self._source(ids))
        return self.pool.submit(self._source(ids), prompt=prefix)

    def step(self) -> List[Tuple[int, BeamSearchOutput]]:
        return self.pool.step()

    def drain(self) -> List[Tuple[int, BeamSearchOutput]]:
        return self.pool.drain()

    @property
    def in_flight(self) -> int:
        return self.pool.in_flight

    @property
    def queued(self) -> int:
        return self.pool.queued

    @property
    def steps(self) -> int:
        return self.pool.steps


class SampleStream(GenerateStream):
    """``HipT5Generator.sample_stream``'s object: ``generation.SamplePool`` over the decoder's slot pool, with
    ``GenerateStream``'s admission (the newcomers encoded together, one packed encoder pass) and its retirement rule.
    ``submit(ids, seed)`` queues a source with its 32-bit seed and returns its ticket; ``step()`` takes one decode step
    and returns the ``(ticket, BeamSearchOutput)`` pairs its sync points delivered; ``drain()`` steps until the stream
    is idle.  Opened with ``per_request``, ``submit`` also takes the ticket's ``SamplingParams`` and ``num_samples``
    (``SamplePool``'s ``per_request``); otherwise either is a ``ValueError``."""

    def __init__(self, generator: HipT5Generator, num_samples: int, max_length: int, temperature: float, top_k: int,
                 top_p: float, length_penalty: float, n_slots: int, src_cap: int, sync_every: int,
                 per_request: bool = False, constraint=None, mask=None):
        dec = self._open(generator, n_slots, num_samples, max_length, src_cap)
        eos = generator._eos
        self.pool = SamplePool(
            self._admit, self._step,
            lambda lp, active, pos, state: self._mine().sample_pool_step(lp, active, pos, state, temperature, top_k, top_p,
                                                                         eos, 0),
            n_slots, num_samples, max_length, length_penalty,
            decoder_start_token_id=generator._start, pad_token_id=0, sync_every=sync_every,
            device=generator.device, books_admit=dec.sample_books_admit, rows=dec.sample_books_rows,
            **(dict(per_request=True, params=SamplingParams(temperature, top_k, top_p)) if per_request else {}),
            **({} if constraint is None else dict(constraint=constraint, mask=mask)))
        self.num_samples, self.per_request = int(num_samples), bool(per_request)

    def submit(self, ids, seed: int, params: Optional[SamplingParams] = None, num_samples: Optional[int] = None,
               prefix=None) -> int:
        if HipT5Generator._prefix(prefix) is not None:
            raise ValueError("a decoder prompt together with sampling is not built yet")
        if params is None and num_samples is None:
            return self.pool.submit(self._source(ids), seed)
        return self.pool.submit(self._source(ids), seed, params, num_samples)


class HipSeq2SeqGradients:
    """d loss / d every parameter of a T5ForConditionalGeneration for the reference's ``training_step`` loss
    (``generation/model.py:117-121``), in one deterministic pass:
    ``HipT5Trainer.forward_hidden`` (the encoder with saved activations) -> ``HipT5Decoder.loss_grad`` (the loss, the
    decoder's gradients and d_enc) -> ``HipT5Trainer.backward_hidden`` (the encoder's gradients from d_enc).

    ``dropout_rate > 0``: T5's training mode.  Call number n draws one seed from
    (``dropout_seed``, n) - the trainer's stream - and that seed drives both halves; ``last_dropout_seed`` is the last
    call's (None without dropout).  Inference through the same weights (``HipT5Generator``) never drops.

    Holds the encoder's fp32 masters (``self.trainer``) and the decoder (``self.decoder``).  No optimizer, no weight
    reload and no ``fit`` here: those layers go on top of this gradient."""

    def __init__(self, cfg: Dict, sd: Dict[str, torch.Tensor], device, dropout_rate: float = 0.0,
                 dropout_seed: Optional[int] = None):
        from .train import HipT5Trainer

        self.cfg = dict(cfg)
        self.device = _require_gpu(device)
        enc_sd = {k: v for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
        self.trainer = HipT5Trainer(cfg, enc_sd, self.device, dropout_rate=dropout_rate, dropout_seed=dropout_seed)
        self.decoder = HipT5Decoder(cfg, sd, self.device)
        self.last_d_enc: Optional[torch.Tensor] = None

    @property
    def dropout_rate(self) -> float:
        return self.trainer.dropout_rate

    @property
    def last_dropout_seed(self) -> Optional[int]:
        return self.trainer.last_dropout_seed

    # the decoder's flat gradient buffer: None = a fresh zeroed one per call; HipSeq2SeqTrainer keeps one for its optimizer
    dec_grads: Optional[torch.Tensor] = None

    def loss_and_grads(self, state_ids, state_mask, tactic_ids):
        """(loss, grads) for padded int batches as the reference's collate makes them.  ``grads`` maps every parameter
        name of the HF model (``shared.weight``, every ``encoder.*`` and ``decoder.*`` weight, ``lm_head.weight`` when the
        head is untied) to an fp32 device tensor of HF's shape.  ``shared.weight`` is the encoder's embedding gradient +
        the decoder's ``shared`` entry (which holds the tied head's), added on the device in that order; the other
        ``encoder.*`` entries are views of the trainer's flat gradient buffer, which the next call overwrites.  ``loss``
        is ``rp_decoder_loss_grad``'s on the trainer's hidden rows; with no counted label it is NaN and every gradient 0.
        A pair with an empty source raises ``ValueError`` (the trainer takes at least one token per sequence).  d_enc of
        the call is kept in ``last_d_enc``."""
        packed, src_cu, tokens, labels, tgt_cu = packed_pairs(self.cfg, state_ids, state_mask, tactic_ids)
        if len(src_cu) < 2 or int(np.diff(src_cu).min()) <= 0:
            raise ValueError("every pair needs a source of at least one token")
        drop = self.trainer.dropout_rate > 0
        hidden = self.trainer.forward_hidden(packed, src_cu, dropout=drop)
        _, (s, c), flat, d_enc = self.decoder.loss_grad(
            hidden, src_cu, tokens, labels, tgt_cu, want_d_enc=True, grads=self.dec_grads,
            dropout=(self.trainer.dropout_rate, self.trainer.last_dropout_seed) if drop else None)
        self.trainer.backward_hidden(d_enc, dropout=drop)
        self.last_d_enc = d_enc
        names, off = self.decoder.grad_layout()
        shapes = self.decoder.grad_shapes()
        grads = {n: flat[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))].view(shapes[n]) for i, n in enumerate(names)}
        for name, g in self.trainer.named_gradients():
            grads[name] = torch.add(g, grads[name]) if name == "shared.weight" else g
        return (s / c if c else float("nan")), grads
