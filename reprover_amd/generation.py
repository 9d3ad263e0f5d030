"""Beam search with HuggingFace's exact semantics, model-agnostic.

A restatement of transformers 5.15's vectorised ``GenerationMixin._beam_search`` (generation/utils.py:3208-3540) for one
source, ``do_sample=False`` and ``early_stopping=False``: what ``T5ForConditionalGeneration.generate(num_beams=n,
num_return_sequences=n, length_penalty=lp, max_length=L, early_stopping=False, do_sample=False)`` computes on the
reference's proving path (prover/tactic_generator.py:203-214).

The model enters through two callables:

- ``step(tokens, ancestry) -> log_probs``: ``tokens`` int64 ``[nb]`` are the beams' last tokens (position ``t``);
  ``ancestry`` int64 ``[nb, t + 1]`` names, for every position ``p <= t`` of beam ``b``, the cache row its self-attention
  key/value lives in.  Row ``t * nb + b`` is where the step stores the new key/value of beam ``b``; ``ancestry[:, t]`` is
  exactly that.  Reordering beams reorders this table only - no cache row moves (HF's ``_reorder_cache`` gathers the whole
  cache).  Returns fp32 ``log_softmax`` ``[nb, vocab]``.
- ``select(log_probs, running_scores, k) -> (scores, tokens, parents)``: the top ``k`` of
  ``log_probs + running_scores[:, None]`` over the flattened ``[nb * vocab]``, ties to the lowest flat index
  (``torch.topk``'s order).  The default is ``torch.topk``; the HIP engine passes its device kernel
  (``rp_beam_select``).

Host synchronisation: the ``2 nb`` selected triples are read back once per step (``.cpu()``) because the finished-beam
bookkeeping below runs on the host.  At 64 beams that is one ~1.5 KB copy and one stream sync per step.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

NEG = -1.0e9  # HF's masking constant (utils.py: running_beam_scores[:, 1:] = -1e9, ... * -1.0e9)


@dataclass
class BeamSearchOutput:
    sequences: torch.Tensor         # int64 [num_return, out_len], starting with the decoder start token
    sequences_scores: torch.Tensor  # fp32 [num_return], length-penalised


def topk_select(log_probs: torch.Tensor, running_scores: torch.Tensor, k: int):
    """Reference selection: utils.py:3300-3302 then ``_get_top_k_continuations``' ``torch.topk`` (:3110)."""
    nb, V = log_probs.shape
    acc = (log_probs + running_scores[:, None]).reshape(nb * V)
    vals, idx = torch.topk(acc, k=k)
    return vals, idx % V, torch.div(idx, V, rounding_mode="floor")


def beam_search(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], num_beams: int, max_length: int,
                length_penalty: float = 1.0, eos_token_id: int = 1, decoder_start_token_id: int = 0,
                num_return_sequences: Optional[int] = None, select: Callable = topk_select,
                device=None, trace: Optional[list] = None) -> BeamSearchOutput:
    """Beam search over ``step`` (module docstring).  ``trace``, when a list, receives the per-step top-``2 nb``
    candidates ``(scores, tokens, parents)`` as host tensors."""
    nb = int(num_beams)
    nret = nb if num_return_sequences is None else int(num_return_sequences)
    assert 1 <= nret <= nb
    prompt_len = 1  # the decoder prompt is the start token alone (utils.py:3266 decoder_prompt_len = cur_len)
    cur_len = prompt_len
    keep = 2 * nb  # beams_to_keep = max(2, 1 + n_eos_tokens) * num_beams with one EOS id (:3271)
    fill = eos_token_id  # output_fill_value = pad_token_id (0, falsy) or eos_token_id[0] (:3294)
    if max_length <= cur_len:
        raise ValueError(f"max_length={max_length} leaves no room after the decoder start token")

    running_seq = torch.full((nb, max_length), fill, dtype=torch.int64)
    running_seq[:, 0] = decoder_start_token_id
    sequences = running_seq.clone()
    running_scores = torch.zeros(nb, dtype=torch.float32)
    running_scores[1:] = NEG  # :3301 - only beam 0 is live at the first step
    beam_scores = torch.full((nb,), NEG, dtype=torch.float32)
    is_sent_finished = torch.zeros(nb, dtype=torch.bool)
    heuristic_unsatisfied = True
    running_bi = torch.full((nb, max_length - cur_len), -1, dtype=torch.int32)
    beam_indices = running_bi.clone()
    top_num_beam_mask = torch.cat([torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool)])
    ancestry = torch.zeros((nb, 0), dtype=torch.int64)
    running_scores_dev = running_scores.to(device) if device is not None else running_scores

    while True:
        t = cur_len - 1  # position of the token fed this step
        tokens = running_seq[:, t]
        ancestry = torch.cat([ancestry, (t * nb + torch.arange(nb, dtype=torch.int64))[:, None]], dim=1)
        if device is not None:
            log_probs = step(tokens.to(device), ancestry.to(device))
        else:
            log_probs = step(tokens, ancestry)
        # _get_top_k_continuations (:3077-3129)
        vals, toks, parents = select(log_probs, running_scores_dev, keep)
        vals, toks, parents = vals.float().cpu(), toks.long().cpu(), parents.long().cpu()  # the per-step host sync
        if trace is not None:
            trace.append((vals.clone(), toks.clone(), parents.clone()))
        topk_seq = running_seq[parents].clone()
        topk_seq[:, cur_len] = toks
        topk_bi = running_bi[parents].clone()
        topk_bi[:, cur_len - prompt_len] = parents.to(torch.int32)
        # stopping criteria on topk_running_sequences[:, :cur_len + 1] (:3321-3327): MaxLength, then EOS
        hits = (toks == eos_token_id) | torch.tensor(cur_len + 1 >= max_length)
        # _get_running_beams_for_next_iteration (:3131-3151)
        run_lp = vals + hits.to(torch.float32) * NEG
        nxt = torch.topk(run_lp, k=nb)[1]
        new_running_seq = topk_seq[nxt]
        running_scores = run_lp[nxt]
        new_running_bi = topk_bi[nxt]
        # _update_finished_beams (:3153-3206)
        just_finished = hits & top_num_beam_mask
        fin_lp = vals / ((cur_len + 1 - prompt_len) ** length_penalty)
        fin_lp = fin_lp + (0.0 if heuristic_unsatisfied else NEG)
        fin_lp = fin_lp + (~just_finished).to(torch.float32) * NEG
        m_seq = torch.cat([sequences, topk_seq], 0)
        m_scores = torch.cat([beam_scores, fin_lp], 0)
        m_bi = torch.cat([beam_indices, topk_bi], 0)
        m_fin = torch.cat([is_sent_finished, just_finished], 0)
        sel = torch.topk(m_scores, k=nb)[1]
        sequences, beam_scores, beam_indices, is_sent_finished = m_seq[sel], m_scores[sel], m_bi[sel], m_fin[sel]
        # the cache reorder (:3478-3489) is a reorder of the ancestry table here
        src = parents[nxt]
        ancestry = ancestry[src]
        running_seq, running_bi = new_running_seq, new_running_bi
        running_scores_dev = running_scores.to(device) if device is not None else running_scores
        cur_len += 1
        # _check_early_stop_heuristic (:3008-3053), early_stopping=False: best length = cur_len - prompt_len
        best_running = running_scores[0] / ((cur_len - prompt_len) ** length_penalty)
        worst_finished = torch.where(is_sent_finished, beam_scores.min(), torch.tensor(NEG))
        heuristic_unsatisfied = heuristic_unsatisfied and bool((best_running > worst_finished).any())
        # _beam_search_has_unfinished_sequences (:3055-3075), early_stopping=False
        if not heuristic_unsatisfied or bool(hits.all()):
            break

    sequences = sequences[:nret]
    beam_scores = beam_scores[:nret]
    beam_indices = beam_indices[:nret]
    max_generated = int(((beam_indices + 1).bool()).sum(dim=1).max())  # :3514-3517
    return BeamSearchOutput(sequences[:, : prompt_len + max_generated], beam_scores)


def greedy_search(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], max_length: int, eos_token_id: int = 1,
                  decoder_start_token_id: int = 0, device=None) -> BeamSearchOutput:
    """``generate(num_beams=1, do_sample=False, max_length=L)``, which HF runs as greedy search (``_sample`` without
    sampling), not as a one-beam beam search: the argmax token (ties to the lowest id) until EOS or ``max_length``
    tokens including the start token.  After an EOS candidate a beam search keeps looking and may return a longer
    sequence; greedy stops.  ``sequences_scores`` holds the sum of the chosen tokens' log-probs (HF reports none)."""
    if max_length <= 1:
        raise ValueError(f"max_length={max_length} leaves no room after the decoder start token")
    seq = [int(decoder_start_token_id)]
    total = 0.0
    while len(seq) < max_length:
        t = len(seq) - 1
        tokens = torch.tensor([seq[-1]], dtype=torch.int64)
        anc = torch.arange(t + 1, dtype=torch.int64)[None]
        if device is not None:
            tokens, anc = tokens.to(device), anc.to(device)
        lp = step(tokens, anc)[0].float().cpu()
        best = int(torch.nonzero(lp == lp.max())[0, 0])
        total += float(lp[best])
        seq.append(best)
        if best == eos_token_id:
            break
    return BeamSearchOutput(torch.tensor([seq], dtype=torch.int64), torch.tensor([total], dtype=torch.float32))
