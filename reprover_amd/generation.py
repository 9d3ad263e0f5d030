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

The drivers, by where the beam books live and whether sources may join a running search:

- Lockstep, books on the host: ``beam_search_batch`` (one ``_BeamState`` per source) and ``greedy_search_batch``, over
  1..n sources; ``beam_search`` and ``greedy_search`` wrap their callables into the ``_many`` protocol and run them
  with one source.  A decoder prompt (HF's ``decoder_input_ids``: tokens after the start token that every returned
  sequence begins with) is ``prompt=`` / ``prompts=`` here and in ``BeamSearchPool.submit``: a state starts at
  ``cur_len = prompt_len = P + 1`` with an ancestry that names one cache row per prompt position (beam 0's, ``p * nb``),
  written before its first step by a ``prefill`` callable (the engine's one-pass ``rp_decoder_batch_prefill``) or, without
  one, through ordinary steps (``prefill_by_steps``); ``_prefill_prompts`` is that dispatch.  With any prompt the loops
  hand ``step_many`` a position per state (``pos=``).
- Lockstep, books on the device: ``beam_search_batch_device`` (a ``BeamBooks`` block that ``advance``,
  ``rp_beam_advance``, updates after every step) and ``sample_search_batch`` (a ``SampleState``; rows never reorder, so
  the ancestry table is the identity).  Nothing is read back per step: the stop flags are read every ``sync_every``
  positions.  ``sample_search`` is the one-source call.
- With admission (continuous batching): sources are submitted while the pool runs, each takes a free slot between two
  steps, is stepped at its own position and is returned when it has stopped.  ``BeamSearchPool`` keeps host books;
  ``BeamBooksPool`` (``rp_beam_pool_advance``) and ``SamplePool`` (``rp_sample_pool_step``) keep them on the device and
  look only at sync points.  The device books and sampling refuse a prompt (``ValueError``: not built yet).

What the drivers share exists once.  ``_SlotPool`` is the slot scheduler of the three pools: the queue, the tickets, a
position per slot, ``queued`` / ``in_flight`` / ``drain``, and for the two device-books pools the sync point (``_sync``:
read the flags, deliver the stopped, free their slots, admit into the lowest free slots, re-gather the by-row inputs if
the active list changed) and the ``step`` around it; a pool adds its done flags, its results, its ``books_admit`` call
and its per-step launch.  ``_beam_inputs`` / ``_beam_take`` are the host-books step body (the step's tokens, padded
ancestry, running scores and positions from the ``_BeamState``s; the one readback of the selected triples and every
state's ``advance``) of ``beam_search_batch`` and ``BeamSearchPool.step``.

The kernels' host restatements, which are their oracles and the callables of a CPU run: ``beam_advance_host`` /
``beam_pool_advance_host`` (one body, ``_advance_host``, with the kernel's stable order), ``beam_books_init_host``,
``beam_books_admit_host``, ``beam_books_rows_host``, ``sample_books_admit_host``, ``sample_books_rows_host`` and
``sample_row_params_host``.  ``SamplingParams`` and ``SamplePool``'s ``per_request`` make the sampling parameters and the
number of samples a property of the request: a parameter table by (state, sample) in ``SampleState.params``
(``rp_sample_step_rows`` / ``rp_sample_pool_step_rows``) and a live-row count per admitted state
(``rp_sample_pool_admit_rows``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
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


# ---- constrained decoding: an automaton state per row, the forbidden log-probs overwritten with -inf ------------------------
# Planted bugs of the constraint's bookkeeping, so that tests can show a comparison would notice them: "state_by_row" takes
# a candidate's automaton state from the launch row it sits in instead of its parent beam (``_BeamState.advance``) or the
# (state, sample) entry (``constraint_mask_step_host``); "admit_not_reset" leaves a slot's states as its last tenant left
# them (no reset at position 0); "mask_wrong_row" masks row r by the state of row r + 1; "eos_anywhere" lets EOS through in
# a state that does not accept.
CONSTRAINT_MUTANTS = ("state_by_row", "admit_not_reset", "mask_wrong_row", "eos_anywhere")


def _mask_rows(log_probs: torch.Tensor, q: torch.Tensor, constraint, mutant: Optional[str]) -> torch.Tensor:
    """``log_probs [rows, vocab]`` with ``-inf`` (in place) wherever ``constraint.next[q[r], v] < 0``; every other entry
    keeps its bits."""
    table = constraint.device_table(log_probs.device)
    if log_probs.shape[1] != table.shape[1]:
        raise ValueError(f"a constraint over {table.shape[1]} ids for log-probs over {log_probs.shape[1]}")
    q = q.to(device=log_probs.device, dtype=torch.int64).clamp(0, table.shape[0] - 1)
    if mutant == "mask_wrong_row":
        q = torch.roll(q, -1)
    forbidden = table[q] < 0
    if mutant == "eos_anywhere":
        forbidden[:, constraint.eos] = False
    log_probs.masked_fill_(forbidden, float("-inf"))
    return log_probs


def constraint_mask_host(log_probs: torch.Tensor, q_rows: torch.Tensor, constraint, mutant: Optional[str] = None
                         ) -> torch.Tensor:
    """``rp_constraint_mask`` on any device's tensors: row ``r`` of ``log_probs`` masked by state ``q_rows[r]`` (values
    clamped into the table, as the kernel does).  In place; returns ``log_probs``.  ``mutant``: ``CONSTRAINT_MUTANTS``."""
    assert mutant is None or mutant in CONSTRAINT_MUTANTS, mutant
    assert q_rows.numel() == log_probs.shape[0], (q_rows.shape, log_probs.shape)
    return _mask_rows(log_probs, q_rows.reshape(-1), constraint, mutant)


def constraint_mask_step_host(log_probs: torch.Tensor, active: Sequence[int], pos: Sequence[int], tokens_in: torch.Tensor,
                              q: torch.Tensor, constraint, mutant: Optional[str] = None) -> torch.Tensor:
    """``rp_constraint_mask_step`` on any device's tensors: ``q`` int32 ``[n, nb]`` by (state, sample).  Row ``a * nb + b``
    of slot ``active[a]``: at ``pos[a] == 0`` its state becomes 0, else it moves to ``next[q][tokens_in[row]]`` where that
    is ``>= 0`` and stays where it is not; the new state is stored and masks the row.  Values are clamped as the kernel
    clamps them.  In place; returns ``log_probs``.  ``mutant``: ``CONSTRAINT_MUTANTS``."""
    assert mutant is None or mutant in CONSTRAINT_MUTANTS, mutant
    n, nb = q.shape
    assert len(active) == len(pos) and len(set(active)) == len(active) and all(0 <= s < n for s in active)
    rows = len(active) * nb
    assert log_probs.shape[0] == rows and tokens_in.numel() >= rows and all(p >= 0 for p in pos)
    table = constraint.device_table(q.device)
    S, V = table.shape
    at = (torch.tensor(list(active), dtype=torch.int64, device=q.device)[:, None] * nb
          + torch.arange(nb, dtype=torch.int64, device=q.device)[None]).reshape(-1)
    if mutant == "state_by_row":
        at = torch.arange(rows, dtype=torch.int64, device=q.device)
    flat = q.view(-1)
    old = flat[at].long().clamp(0, S - 1)
    tok = tokens_in.reshape(-1)[:rows].to(device=q.device, dtype=torch.int64).clamp(0, V - 1)
    to = table[old, tok].long()
    new = torch.where(to >= 0, to.clamp(max=S - 1), old)
    if mutant != "admit_not_reset":
        first = torch.tensor([p == 0 for p in pos], device=q.device).repeat_interleave(nb)
        new = torch.where(first, torch.zeros_like(new), new)
    flat[at] = new.to(flat.dtype)
    return _mask_rows(log_probs, new, constraint, mutant)


def _constraint_mask(constraint, mask: Optional[Callable], fused: bool, mutant: Optional[str] = None) -> Optional[Callable]:
    """The loops' one ``mask`` callable: None without a constraint; else ``mask`` (the engine's launch) or the host
    emulation over ``constraint``.  ``fused`` False: ``mask(log_probs, q_rows)``, the by-row states uploaded with the
    step's tokens (the host-books loops).  ``fused`` True: ``mask(log_probs, active, pos, tokens_in, q)``, the states on
    the device by (state, sample) (the sampled loops)."""
    if constraint is None:
        if mask is not None:
            raise ValueError("mask= without constraint=")
        return None
    if mask is not None:
        return mask
    mutant = mutant if mutant in CONSTRAINT_MUTANTS else None
    if fused:
        return lambda lp, active, pos, tokens_in, q: constraint_mask_step_host(lp, active, pos, tokens_in, q, constraint,
                                                                               mutant)
    return lambda lp, q_rows: constraint_mask_host(lp, q_rows, constraint, mutant)


def _refuse_constraint(constraint, what: str) -> None:
    if constraint is not None:
        raise ValueError(f"a constraint together with {what} is not built yet")


def _with_states(tokens: torch.Tensor, q_rows: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The step's tokens and its by-row automaton states in one upload: (tokens, int32 q_rows) on ``device``."""
    rows = tokens.numel()
    both = torch.cat([tokens.to(torch.int64), q_rows.to(torch.int64)])
    if device is not None:
        both = both.to(device)
    return both[:rows], both[rows:].to(torch.int32)


def _prompt_tokens(prompt) -> List[int]:
    """A decoder prompt (the tokens after the start token; None: none) as a list of ints."""
    if prompt is None:
        return []
    return [int(x) for x in np.asarray(prompt).reshape(-1).tolist()]


def _no_room(max_length: int, P: int) -> str:
    if P == 0:
        return f"max_length={max_length} leaves no room after the decoder start token"
    return f"max_length={max_length} leaves no room after the decoder prompt of 1 + {P} tokens"


def _refuse_prompts(prompts, what: str) -> None:
    """The search kinds without a decoder prompt: a ``ValueError`` when any entry of ``prompts`` has tokens."""
    if prompts is not None and any(_prompt_tokens(p) for p in prompts):
        raise ValueError(f"a decoder prompt together with {what} is not built yet")


def _prompt_rows(prompt: Sequence[int], decoder_start_token_id: int) -> List[int]:
    """The tokens of the prompt's cache rows, positions ``0 .. P - 1``: the prompt ``[start, b_1 .. b_P]`` without its
    last token, which the search feeds itself at position ``P``."""
    return [int(decoder_start_token_id)] + list(prompt[:-1])


def prefill_by_steps(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], nb: int, rows: Sequence[int],
                     device=None) -> None:
    """Write a prompt's cache rows through ordinary decode steps, for models that have only ``step``: position ``p``
    is fed ``rows[p]`` repeated over the ``nb`` beams with identity ancestry, so beam 0's row ``p * nb`` - the one a
    prompted search reads - holds what a one-pass prefill writes there.  The log-probs are dropped."""
    nb = int(nb)
    beams = torch.arange(nb, dtype=torch.int64)
    for p, tok in enumerate(rows):
        tokens = torch.full((nb,), int(tok), dtype=torch.int64)
        anc = torch.arange(p + 1, dtype=torch.int64)[None] * nb + beams[:, None]
        if device is not None:
            tokens, anc = tokens.to(device), anc.to(device)
        step(tokens, anc)


def _check_prompts(prompts, n: int, max_length: int, what: str = "prompts", whose: str = "states"
                   ) -> Optional[List[List[int]]]:
    """``prompts`` (None, or one entry or None per state) as token lists; None when no state has a prompt.  (A state
    without one is the search's own to refuse when ``max_length`` leaves it no room.)"""
    if prompts is None:
        return None
    prompts = [_prompt_tokens(p) for p in prompts]
    if len(prompts) != n:
        raise ValueError(f"{len(prompts)} {what} for {n} {whose}")
    for p in prompts:
        if p and max_length <= 1 + len(p):
            raise ValueError(_no_room(max_length, len(p)))
    return prompts if any(prompts) else None


def _prefill_prompts(prefill: Optional[Callable], step_at: Callable, listed: Sequence[int], prompts: Sequence[Sequence[int]],
                     decoder_start_token_id: int, nb: int, device) -> None:
    """Write the prompt rows of the states (or slots) ``listed``, ``prompts[j]`` being ``listed[j]``'s: one
    ``prefill(listed, rows)`` where there is one, else one state and one position at a time through
    ``step_at(i, p, tokens, ancestry)``, an ordinary step of state ``i`` alone at position ``p`` (``prefill_by_steps``)."""
    rows = [_prompt_rows(p, decoder_start_token_id) for p in prompts]
    if prefill is not None:
        prefill(list(listed), rows)
        return
    for i, r in zip(listed, rows):
        prefill_by_steps(lambda tok, anc, i=i: step_at(i, anc.shape[1] - 1, tok, anc), nb, r, device)


def _check_room(max_length: int) -> None:
    if max_length <= 1:
        raise ValueError(_no_room(max_length, 0))


def _check_count(name: str, value, or_none: str = "") -> int:
    """``value`` as an int; a ``ValueError`` unless it is an integer >= 1 (``sync_every``, ``n_slots``)."""
    if int(value) != value or value < 1:
        raise ValueError(f"{name}={value} must be an integer >= 1{or_none}")
    return int(value)


# "divisors_count_prompt" plants a known bug: both length-penalty divisors count the prompt's tokens (prompt_len left at
# 1 there), so that tests can show the fixture tells HF's semantics from it
PROMPT_MUTANTS = ("divisors_count_prompt",)


class _BeamState:
    """The host bookkeeping of one source's beam search: ``inputs`` gives the step's tokens and ancestry table,
    ``advance`` takes the step's top-``2 nb`` candidates (host tensors) and says whether the search is over.
    ``beam_search_batch`` drives one per source in lockstep; ``beam_search`` is its one-source call."""

    def __init__(self, num_beams: int, max_length: int, length_penalty: float, eos_token_id: int,
                 decoder_start_token_id: int, num_return_sequences: Optional[int],
                 prompt: Optional[Sequence[int]] = None, mutant: Optional[str] = None, constraint=None):
        assert mutant is None or mutant in PROMPT_MUTANTS + CONSTRAINT_MUTANTS, mutant
        self.mutant, self.constraint = mutant, constraint
        nb = self.nb = int(num_beams)
        self.nret = nb if num_return_sequences is None else int(num_return_sequences)
        assert 1 <= self.nret <= nb
        # the decoder prompt is the start token and the ``prompt`` tokens (utils.py:3278 decoder_prompt_len = cur_len):
        # max_length counts it, the returned sequences hold it, the scores and both divisors count generated tokens only
        prompt = _prompt_tokens(prompt)
        P = len(prompt)
        self.prompt_len = 1 + P
        self.cur_len = self.prompt_len
        self.keep = 2 * nb  # beams_to_keep = max(2, 1 + n_eos_tokens) * num_beams with one EOS id (:3271)
        fill = eos_token_id  # output_fill_value = pad_token_id (0, falsy) or eos_token_id[0] (:3294)
        if max_length <= self.cur_len:
            raise ValueError(_no_room(max_length, P))
        self.max_length, self.length_penalty, self.eos_token_id = max_length, length_penalty, eos_token_id

        self.running_seq = torch.full((nb, max_length), fill, dtype=torch.int64)
        self.running_seq[:, 0] = decoder_start_token_id
        if P:
            self.running_seq[:, 1 : 1 + P] = torch.tensor(prompt, dtype=torch.int64)
        self.sequences = self.running_seq.clone()
        self.running_scores = torch.zeros(nb, dtype=torch.float32)
        self.running_scores[1:] = NEG  # :3301 - only beam 0 is live at the first step
        self.beam_scores = torch.full((nb,), NEG, dtype=torch.float32)
        self.is_sent_finished = torch.zeros(nb, dtype=torch.bool)
        self.heuristic_unsatisfied = True
        self.running_bi = torch.full((nb, max_length - self.cur_len), -1, dtype=torch.int32)
        self.beam_indices = self.running_bi.clone()
        self.top_num_beam_mask = torch.cat([torch.ones(nb, dtype=torch.bool),
                                            torch.zeros(self.keep - nb, dtype=torch.bool)])
        # the prompt's cache rows are shared by all beams: one row per prompt position, beam 0's (p * nb)
        self.ancestry = (torch.arange(P, dtype=torch.int64) * nb)[None].repeat(nb, 1)
        if constraint is not None:  # an automaton state per running beam; a prompt the automaton rejects raises here
            self.q = torch.full((nb,), constraint.state_after(prompt), dtype=torch.int64)

    def inputs(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(tokens [nb], ancestry [nb, t + 1]) of the step at position ``t = cur_len - 1``."""
        nb, t = self.nb, self.cur_len - 1
        self.ancestry = torch.cat([self.ancestry, (t * nb + torch.arange(nb, dtype=torch.int64))[:, None]], dim=1)
        return self.running_seq[:, t], self.ancestry

    def advance(self, vals: torch.Tensor, toks: torch.Tensor, parents: torch.Tensor) -> bool:
        """Take the selected candidates of this step; True when the search has stopped."""
        nb, cur_len, prompt_len, length_penalty = self.nb, self.cur_len, self.prompt_len, self.length_penalty
        running_seq, running_bi = self.running_seq, self.running_bi
        topk_seq = running_seq[parents].clone()
        topk_seq[:, cur_len] = toks
        topk_bi = running_bi[parents].clone()
        topk_bi[:, cur_len - prompt_len] = parents.to(torch.int32)
        # stopping criteria on topk_running_sequences[:, :cur_len + 1] (:3321-3327): MaxLength, then EOS
        hits = (toks == self.eos_token_id) | torch.tensor(cur_len + 1 >= self.max_length)
        # _get_running_beams_for_next_iteration (:3131-3151)
        run_lp = vals + hits.to(torch.float32) * NEG
        nxt = torch.topk(run_lp, k=nb)[1]
        new_running_seq = topk_seq[nxt]
        running_scores = run_lp[nxt]
        new_running_bi = topk_bi[nxt]
        # _update_finished_beams (:3153-3206)
        just_finished = hits & self.top_num_beam_mask
        div_prompt = 1 if self.mutant == "divisors_count_prompt" else prompt_len
        fin_lp = vals / ((cur_len + 1 - div_prompt) ** length_penalty)
        fin_lp = fin_lp + (0.0 if self.heuristic_unsatisfied else NEG)
        fin_lp = fin_lp + (~just_finished).to(torch.float32) * NEG
        m_seq = torch.cat([self.sequences, topk_seq], 0)
        m_scores = torch.cat([self.beam_scores, fin_lp], 0)
        m_bi = torch.cat([self.beam_indices, topk_bi], 0)
        m_fin = torch.cat([self.is_sent_finished, just_finished], 0)
        sel = torch.topk(m_scores, k=nb)[1]
        self.sequences, self.beam_scores, self.beam_indices, self.is_sent_finished = (
            m_seq[sel], m_scores[sel], m_bi[sel], m_fin[sel])
        # the cache reorder (:3478-3489) is a reorder of the ancestry table here
        src = parents[nxt]
        self.ancestry = self.ancestry[src]
        if self.constraint is not None:  # next[old[parent], token] of the nb kept beams (a dead candidate's stays)
            old = self.q[torch.arange(self.keep) % nb if self.mutant == "state_by_row" else parents]
            to = self.constraint.table()[old, toks].long()
            self.q = torch.where(to >= 0, to, old)[nxt]
        self.running_seq, self.running_bi, self.running_scores = new_running_seq, new_running_bi, running_scores
        self.cur_len = cur_len = cur_len + 1
        # _check_early_stop_heuristic (:3008-3053), early_stopping=False: best length = cur_len - prompt_len
        best_running = running_scores[0] / ((cur_len - div_prompt) ** length_penalty)
        worst_finished = torch.where(self.is_sent_finished, self.beam_scores.min(), torch.tensor(NEG))
        self.heuristic_unsatisfied = self.heuristic_unsatisfied and bool((best_running > worst_finished).any())
        # _beam_search_has_unfinished_sequences (:3055-3075), early_stopping=False
        return not self.heuristic_unsatisfied or bool(hits.all())

    def result(self) -> BeamSearchOutput:
        sequences = self.sequences[: self.nret]
        beam_scores = self.beam_scores[: self.nret]
        beam_indices = self.beam_indices[: self.nret]
        max_generated = int(((beam_indices + 1).bool()).sum(dim=1).max())  # :3514-3517
        return BeamSearchOutput(sequences[:, : self.prompt_len + max_generated], beam_scores)


def beam_search(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], num_beams: int, max_length: int,
                length_penalty: float = 1.0, eos_token_id: int = 1, decoder_start_token_id: int = 0,
                num_return_sequences: Optional[int] = None, select: Callable = topk_select,
                device=None, trace: Optional[list] = None, prompt: Optional[Sequence[int]] = None,
                prefill: Optional[Callable] = None, mutant: Optional[str] = None, constraint=None,
                mask: Optional[Callable] = None) -> BeamSearchOutput:
    """Beam search over ``step`` (module docstring): ``beam_search_batch`` with one state.  ``trace``, when a list,
    receives the per-step top-``2 nb`` candidates ``(scores, tokens, parents)`` as host tensors.

    ``prompt``: decoder tokens after the start token that every returned sequence begins with (HF's
    ``decoder_input_ids = [start] + prompt``); ``prefill(rows)`` writes the prompt's cache rows (``beam_search_batch``),
    by default through ``step`` (``prefill_by_steps``).  ``constraint`` / ``mask``: as in ``beam_search_batch``."""
    traces: Optional[list] = None if trace is None else []
    step_one = lambda active, tokens, ancestry, pos=None: step(tokens, ancestry)  # noqa: E731
    out, = beam_search_batch(step_one, 1, num_beams, max_length,
                             length_penalty, eos_token_id, decoder_start_token_id, num_return_sequences,
                             lambda lp, running, nb, k: tuple(x[None] for x in select(lp, running, k)), device, traces,
                             prompts=None if prompt is None else [prompt],
                             prefill_many=None if prefill is None else (lambda states, rows: prefill(rows[0])),
                             mutant=mutant, constraint=constraint, mask=mask)
    if trace is not None:
        trace.extend(traces[0])
    return out


def topk_select_many(log_probs: torch.Tensor, running_scores: torch.Tensor, nb: int, k: int):
    """``topk_select`` per state over ``[n_active * nb, vocab]`` rows: each output ``[n_active, k]``."""
    outs = [topk_select(log_probs[a * nb : (a + 1) * nb], running_scores[a * nb : (a + 1) * nb], k)
            for a in range(log_probs.shape[0] // nb)]
    return tuple(torch.stack(x) for x in zip(*outs))


def _beam_inputs(states: Sequence[_BeamState], nb: int, device=None):
    """The host-books step's ``(tokens [n * nb], ancestry [n * nb, W], running scores [n * nb], pos)`` over ``states``:
    ``pos[a]`` is the position of ``states[a]``, ``W`` the widest ``pos + 1``, a narrower state's ancestry rows
    right-padded with zeros (columns ``0..pos[a]`` are its own).  The tensors are moved to ``device`` when there is one.
    The fifth value is None, or with constrained states their automaton states by row (int32 ``[n * nb]``), which travel
    in the tokens' upload."""
    ins = [st.inputs() for st in states]
    pos = [st.cur_len - 1 for st in states]
    tokens = torch.cat([x[0] for x in ins])
    if states[0].constraint is not None:
        tokens, q_rows = _with_states(tokens, torch.cat([st.q for st in states]), device)
    else:
        q_rows = None
    running = torch.cat([st.running_scores for st in states])
    if min(pos) == max(pos):
        ancestry = torch.cat([x[1] for x in ins])
    else:
        ancestry = torch.zeros((len(states) * nb, max(pos) + 1), dtype=torch.int64)
        for a, (_, anc) in enumerate(ins):
            ancestry[a * nb : (a + 1) * nb, : anc.shape[1]] = anc
    if device is not None:
        tokens, ancestry, running = tokens.to(device), ancestry.to(device), running.to(device)
    return tokens, ancestry, running, pos, q_rows


def _beam_take(states: Sequence[_BeamState], selected, traces: Optional[Sequence[list]] = None) -> List[bool]:
    """Hand the step's selected triples (``select_many``'s three ``[n, 2 nb]`` outputs) to ``states``: one readback, then
    every state's ``advance``; entry ``a`` says whether ``states[a]`` has stopped.  ``traces[a]``, when given, receives
    that state's triples of this step."""
    vals, toks, parents = selected
    vals, toks, parents = vals.float().cpu(), toks.long().cpu(), parents.long().cpu()  # the per-step host sync
    stopped = []
    for a, st in enumerate(states):
        if traces is not None:
            traces[a].append((vals[a].clone(), toks[a].clone(), parents[a].clone()))
        stopped.append(st.advance(vals[a], toks[a], parents[a]))
    return stopped


def beam_search_batch(step_many: Callable, num_states: int, num_beams: int, max_length: int, length_penalty: float = 1.0,
                      eos_token_id: int = 1, decoder_start_token_id: int = 0,
                      num_return_sequences: Optional[int] = None, select_many: Callable = topk_select_many, device=None,
                      traces: Optional[list] = None, prompts: Optional[Sequence] = None,
                      prefill_many: Optional[Callable] = None, mutant: Optional[str] = None, constraint=None,
                      mask: Optional[Callable] = None) -> List[BeamSearchOutput]:
    """The search loop: ``num_states`` sources in lockstep, one ``step_many`` and one ``select_many`` per position, one
    readback of the ``n_active x 2 nb`` triples.  Every state keeps its own bookkeeping (``_BeamState``) and leaves the
    active list at the step where it would stop alone; the loop runs until the last one has.

    - ``step_many(active, tokens, ancestry) -> log_probs``: ``active`` is the list of state indices still searching
      (ascending); row ``a * nb + b`` of ``tokens [n_active * nb]`` / ``ancestry [n_active * nb, t + 1]`` is beam ``b``
      of state ``active[a]``, ancestry entries local to that state's own cache.  Returns ``[n_active * nb, vocab]``.
    - ``select_many(log_probs, running_scores, nb, k)``: per state the top ``k`` of its own ``[nb * vocab]`` block,
      each output ``[n_active, k]``, parents local to the state.

    ``traces``, when a list, receives one per-state list of ``(scores, tokens, parents)`` per step.

    ``prompts`` (None, or one token sequence or None per state): state ``i``'s decoder prompt after the start token, of
    ``P_i >= 0`` tokens.  Its search starts at position ``P_i`` with the prompt in every sequence; the prompt's cache rows
    ``p * nb``, ``p < P_i``, are written before the loop by ``prefill_many(states, rows)`` - ``states`` the indices with
    ``P_i >= 1``, ``rows[j]`` the tokens of positions ``0 .. P - 1`` (``_prompt_rows``) - by default through
    ``step_many``, one state and one position at a time (``prefill_by_steps``).  With any prompt the loop hands
    ``step_many`` a position per active state, ``step_many(active, tokens, ancestry, pos=pos)``, and pads the ancestry
    table as ``BeamSearchPool.step`` does: state ``i`` stands at ``P_i + k`` after ``k`` steps.  Without prompts the
    loop is the one above, call for call.  ``mutant``: one of ``PROMPT_MUTANTS`` or ``CONSTRAINT_MUTANTS``.

    ``constraint`` (a ``constraint.ByteAutomaton``; None: the loop above, call for call): every state keeps an automaton
    state per running beam (after its prompt: ``state_after(prompt)``, a rejected prompt a ``ValueError`` before anything
    is launched), the by-row states go up with the step's tokens, and ``mask(log_probs, q_rows)`` overwrites the
    forbidden entries with ``-inf`` between the step and the selection (default ``constraint_mask_host``; the engine
    passes ``rp_constraint_mask``)."""
    prompts = _check_prompts(prompts, num_states, max_length)
    mask = _constraint_mask(constraint, mask, False, mutant)
    states = [_BeamState(num_beams, max_length, length_penalty, eos_token_id, decoder_start_token_id,
                         num_return_sequences, None if prompts is None else prompts[i], mutant, constraint)
              for i in range(num_states)]
    per_state = [[] for _ in states]
    active = list(range(num_states))
    nb = int(num_beams)
    if prompts is not None:
        listed = [i for i in range(num_states) if prompts[i]]
        _prefill_prompts(prefill_many, lambda i, p, tok, anc: step_many([i], tok, anc, pos=[p]), listed,
                         [prompts[i] for i in listed], decoder_start_token_id, nb, device)
    while active:
        stepped = [states[i] for i in active]
        tokens, ancestry, running, pos, q_rows = _beam_inputs(stepped, nb, device)
        if prompts is None:
            log_probs = step_many(list(active), tokens, ancestry)
        else:
            log_probs = step_many(list(active), tokens, ancestry, pos=pos)
        if mask is not None:
            log_probs = mask(log_probs, q_rows)
        stopped = _beam_take(stepped, select_many(log_probs, running, nb, 2 * nb),
                             None if traces is None else [per_state[i] for i in active])
        active = [i for i, over in zip(active, stopped) if not over]
    if traces is not None:
        traces.extend(per_state)
    return [st.result() for st in states]


# ---- continuous batching: states join a running search between steps -------------------------------------------------------
POOL_MUTANTS = ("shared_position",)


class _SlotPool:
    """The slot scheduler of the three pools: ``n_slots`` places, a first-in-first-out queue of ``(ticket, source, ...)``
    entries, per slot its tenant's ticket (None: free) and, for the device-books pools, the position of its next step.
    ``BeamSearchPool`` takes the queue, the tickets and the slots from it and looks at its host books every step.  The
    device-books pools (``sync_every`` given) take ``_sync`` and ``step`` too and supply what differs: ``_stopped()``
    (read the done flags through ``to_host``; the slots in use that are over), ``_results(stopped)``, ``_admit_books(slots,
    entries)`` (their ``books_admit`` call), ``_launch(active, pos)`` (the step's engine calls), ``_book`` (what ``rows``
    is handed) and ``_last_pos`` (where a slot's position stays)."""

    def __init__(self, n_slots: int, width_name: str, width: int, max_length: int, sync_every: Optional[int] = None):
        if int(n_slots) < 1 or int(width) < 1:
            raise ValueError(f"n_slots={n_slots} and {width_name}={width} must be >= 1")
        _check_room(max_length)
        self.n_slots, self.nb, self.max_length = int(n_slots), int(width), int(max_length)
        self._queue: List[tuple] = []                                # (ticket, source, ...), first in first out
        self._ticket: List[Optional[int]] = [None] * self.n_slots    # per slot: its tenant's ticket
        self._next_ticket = 0
        self.steps = 0
        if sync_every is not None:
            self.sync_every = _check_count("sync_every", sync_every)
            self._pos = [0] * self.n_slots                           # per slot: the position of its next step
            self._active: List[int] = []                             # the slots in use, ascending: the by-row order
            self._since = 0                                          # steps since the last sync point
            self.sync_points = 0

    @property
    def queued(self) -> int:
        return len(self._queue)

    @property
    def in_flight(self) -> int:
        return sum(t is not None for t in self._ticket)

    def _issue(self, *entry) -> int:
        """Queue ``(ticket, *entry)`` under the next ticket."""
        ticket = self._next_ticket
        self._next_ticket += 1
        self._queue.append((ticket,) + entry)
        return ticket

    def _take(self) -> Tuple[List[int], List[tuple]]:
        """The lowest free slots (ascending) and the queue entries that take them, first in first out."""
        free = [s for s in range(self.n_slots) if self._ticket[s] is None]
        take = min(len(free), len(self._queue))
        new, self._queue = self._queue[:take], self._queue[take:]
        return free[:take], new

    def _sync(self) -> List[Tuple[int, BeamSearchOutput]]:
        """A sync point (``BeamBooksPool``): the pairs it delivered."""
        self.sync_points += 1
        self._since = 0
        out: List[Tuple[int, BeamSearchOutput]] = []
        changed = False
        if self._active:
            stopped = self._stopped()
            if stopped:
                out = self._results(stopped)
                for s in stopped:
                    self._ticket[s] = None
                changed = True
        slots, new = self._take()
        if slots:
            self._admit(slots, [entry[1] for entry in new])
            self._admit_books(slots, new)
            for s, entry in zip(slots, new):
                self._ticket[s], self._pos[s] = entry[0], 0
            changed = True
        self._active = [s for s in range(self.n_slots) if self._ticket[s] is not None]
        if changed and self._active:
            self._rows(self._book, list(self._active), [self._pos[s] for s in self._active])
        return out

    def step(self) -> List[Tuple[int, BeamSearchOutput]]:
        """One decode step, with a sync point before it when a queued source can take a free slot and one after it when
        ``sync_every`` steps have passed or a slot stands at ``max_length - 1``; the ``(ticket, output)`` pairs those
        sync points delivered."""
        out: List[Tuple[int, BeamSearchOutput]] = []
        if self._queue and self.in_flight < self.n_slots:
            out.extend(self._sync())
        if not self._active:
            return out
        active = list(self._active)
        pos = [self._pos[s] for s in active]
        self._launch(active, pos)
        self.steps += 1
        self._since += 1
        last = self._last_pos
        pos = [p + 1 if p < last else last for p in pos]
        for s, p in zip(active, pos):
            self._pos[s] = p
        if self._since >= self.sync_every or max(pos) + 1 >= self.max_length:
            out.extend(self._sync())
        return out

    def drain(self) -> List[Tuple[int, BeamSearchOutput]]:
        """Step until nothing is queued or in flight; every pair that was delivered on the way, in delivery order."""
        out = []
        while self._queue or self.in_flight:
            out.extend(self.step())
        return out


class BeamSearchPool(_SlotPool):
    """``beam_search_batch``'s loop opened up: ``n_slots`` places, each carrying one source's search (a ``_BeamState``)
    at its own position.  ``submit`` queues a source; every ``step`` first admits queued sources into the free slots,
    then runs one decode step and one selection over the slots in use, reads the selected triples back once, advances
    every state's books and frees the slots of the states that stopped.  A ticket's output is ``beam_search``'s for that
    source alone, whatever else is in flight and whenever it joined: a row's log-probs depend on its own state and
    position only, and selection reads no position.

    - ``admit(slots, sources)``: make the engine ready to step ``sources[j]`` in slot ``slots[j]`` (encode, cross K/V);
      one call for all newcomers of a step.
    - ``step(active, pos, tokens, ancestry) -> log_probs``: ``active`` the slots in use (ascending), ``pos[a]`` the
      position of slot ``active[a]``; row ``a * nb + b`` of ``tokens [n_active * nb]`` / ``ancestry [n_active * nb, W]``
      is beam ``b`` of that slot, ``W`` the widest ``pos + 1`` of the step, a narrower slot's rows right-padded with
      zeros (columns ``0..pos[a]`` are its own).  Returns ``[n_active * nb, vocab]``.
    - ``select_many(log_probs, running_scores, nb, k)``: as in ``beam_search_batch``.

    ``steps`` counts the decode steps taken.  ``mutant`` plants a known bug (``POOL_MUTANTS``: "shared_position" hands
    every slot the step's largest position, the uniform-``t`` engine's assumption) so that tests can show a comparison
    would notice it."""

    def __init__(self, admit: Callable, step: Callable, n_slots: int, num_beams: int, max_length: int,
                 length_penalty: float = 1.0, eos_token_id: int = 1, decoder_start_token_id: int = 0,
                 num_return_sequences: Optional[int] = None, select_many: Callable = topk_select_many, device=None,
                 mutant: Optional[str] = None, prefill: Optional[Callable] = None, constraint=None,
                 mask: Optional[Callable] = None):
        assert mutant is None or mutant in POOL_MUTANTS + CONSTRAINT_MUTANTS, mutant
        super().__init__(n_slots, "num_beams", num_beams, max_length)
        self.constraint, self._mask = constraint, _constraint_mask(constraint, mask, False, mutant)
        state_mutant = mutant if mutant in CONSTRAINT_MUTANTS else None
        self._admit, self._step, self._select_many, self._prefill = admit, step, select_many, prefill
        self.device, self.mutant, self._start_token = device, mutant, decoder_start_token_id
        self._new_state = lambda prompt=None: _BeamState(num_beams, max_length, length_penalty, eos_token_id,
                                                         decoder_start_token_id, num_return_sequences, prompt,
                                                         state_mutant, constraint)
        self._prompt: dict = {}                                       # ticket -> its decoder prompt, where it has one
        self._state: List[Optional[_BeamState]] = [None] * self.n_slots  # per slot in use: its tenant's books

    def submit(self, source, prompt: Optional[Sequence[int]] = None) -> int:
        """Queue a source; its ticket names it in ``step``'s return.  ``prompt``: the ticket's decoder prompt after
        the start token (``beam_search``'s): its slot starts at position ``len(prompt)``, its prompt rows written right
        after ``admit`` by ``prefill(slots, rows)`` - by default through ``step``, a position at a time."""
        prompt = _prompt_tokens(prompt)
        if self.max_length <= 1 + len(prompt):
            raise ValueError(_no_room(self.max_length, len(prompt)))
        if self.constraint is not None:
            self.constraint.state_after(prompt)  # a rejected prompt: ValueError before it is queued
        ticket = self._issue(source)
        if prompt:
            self._prompt[ticket] = prompt
        return ticket

    def step(self) -> List[Tuple[int, BeamSearchOutput]]:
        """Admit what fits, take one decode step, return the ``(ticket, output)`` pairs of the states that stopped."""
        slots, new = self._take()
        if slots:
            self._admit(slots, [src for _, src in new])
            prompted = []
            for s, (ticket, _) in zip(slots, new):
                prompt = self._prompt.pop(ticket, None)
                self._ticket[s], self._state[s] = ticket, self._new_state(prompt)
                if prompt:
                    prompted.append((s, prompt))
            if prompted:
                _prefill_prompts(self._prefill, lambda s, p, tok, anc: self._step([s], [p], tok, anc),
                                 [s for s, _ in prompted], [q for _, q in prompted], self._start_token, self.nb,
                                 self.device)
        active = [s for s in range(self.n_slots) if self._ticket[s] is not None]
        if not active:
            return []
        nb = self.nb
        states = [self._state[s] for s in active]
        tokens, ancestry, running, pos, q_rows = _beam_inputs(states, nb, self.device)
        if self.mutant == "shared_position":
            pos = [max(pos)] * len(pos)
        log_probs = self._step(list(active), pos, tokens, ancestry)
        if self._mask is not None:
            log_probs = self._mask(log_probs, q_rows)
        stopped = _beam_take(states, self._select_many(log_probs, running, nb, 2 * nb))
        self.steps += 1
        done = []
        for s, st, over in zip(active, states, stopped):
            if over:
                done.append((self._ticket[s], st.result()))
                self._ticket[s] = self._state[s] = None
        return done


# ---- beam search with its books on the device ------------------------------------------------------------------------------
# The parts of the books block (include/reprover_hip.h, rp_beam_books_bytes), in order: name, shape in terms of
# (n, nb, max_len), fp32 or int32.  Every part starts at a multiple of 16 bytes.
_BOOK_PARTS = (
    ("run_seq", lambda n, nb, L: (2, n, nb, L), False), ("anc", lambda n, nb, L: (2, n, nb, L), False),
    ("fin_seq", lambda n, nb, L: (2, n, nb, L), False), ("run_scores", lambda n, nb, L: (n, nb), True),
    ("beam_scores", lambda n, nb, L: (n, nb), True), ("fin_flag", lambda n, nb, L: (n, nb), False),
    ("fin_len", lambda n, nb, L: (n, nb), False), ("heur", lambda n, nb, L: (n,), False),
    ("done", lambda n, nb, L: (n,), False), ("steps", lambda n, nb, L: (n,), False),
    ("tokens", lambda n, nb, L: (n * nb,), False), ("running", lambda n, nb, L: (n * nb,), True),
    ("anc_rows", lambda n, nb, L: (n * nb, L), False),
)


def beam_books_bytes(n: int, nb: int, max_len: int) -> int:
    """The size of the books block (what ``rp_beam_books_bytes`` returns for arguments it accepts)."""
    total = 0
    for _, shape, _ in _BOOK_PARTS:
        words = 1
        for d in shape(n, nb, max_len):
            words *= d
        total += (4 * words + 15) // 16 * 16
    return total


class BeamBooks:
    """The books of a beam search over ``n`` states: one int32 ``block`` (on any device) and typed views of its parts.
    Row tables hold ``max_len`` columns; ``run_seq`` / ``anc`` / ``fin_seq`` are pairs of which the step at position ``t``
    reads member ``t & 1`` and writes the other, so ``steps[s] & 1`` is state ``s``'s current member.  ``tokens``,
    ``running`` and ``anc_rows`` are by row (slot * nb + beam): the next step's inputs.  ``rp_beam_advance`` (or
    ``beam_advance_host``) updates all of it in place."""

    def __init__(self, n: int, nb: int, max_len: int, device=None, block: Optional[torch.Tensor] = None):
        self.n, self.nb, self.max_len = int(n), int(nb), int(max_len)
        self.nbytes = beam_books_bytes(self.n, self.nb, self.max_len)
        if block is None:
            block = torch.zeros(self.nbytes // 4, dtype=torch.int32, device=device)
        assert block.dtype == torch.int32 and block.is_contiguous() and block.numel() == self.nbytes // 4
        self.block = block
        off = 0
        for name, shape, is_float in _BOOK_PARTS:
            shp = shape(self.n, self.nb, self.max_len)
            words = 1
            for d in shp:
                words *= d
            part = block[off : off + words]
            setattr(self, name, (part.view(torch.float32) if is_float else part).view(shp))
            off += (words + 3) // 4 * 4

    def cpu(self) -> "BeamBooks":
        """A host copy (one device-to-host transfer of the block)."""
        return BeamBooks(self.n, self.nb, self.max_len, block=self.block.cpu())

    def result(self, state: int, num_return_sequences: Optional[int] = None) -> BeamSearchOutput:
        """``_BeamState.result`` of one state from host books."""
        nret = self.nb if num_return_sequences is None else int(num_return_sequences)
        cur = int(self.steps[state]) & 1
        max_generated = int(self.fin_len[state, :nret].max())  # beam_indices' count of non-negative entries (:3514-3517)
        return BeamSearchOutput(self.fin_seq[cur, state, :nret, : 1 + max_generated].long().clone(),
                                self.beam_scores[state, :nret].clone())


def beam_books_init_host(n: int, nb: int, max_len: int, eos_token_id: int, decoder_start_token_id: int) -> BeamBooks:
    """``rp_beam_books_init`` on host tensors: ``_BeamState.__init__``'s values for ``n`` states."""
    bk = BeamBooks(n, nb, max_len)
    for tab in (bk.run_seq, bk.fin_seq):
        tab.fill_(eos_token_id)
        tab[..., 0] = decoder_start_token_id
    ident = (torch.arange(max_len, dtype=torch.int32)[None] * nb + torch.arange(nb, dtype=torch.int32)[:, None])
    bk.anc.copy_(ident.expand(2, n, nb, max_len))
    bk.anc_rows.copy_(ident.repeat(n, 1))
    bk.run_scores.fill_(NEG)
    bk.run_scores[:, 0] = 0.0
    bk.running.copy_(bk.run_scores.reshape(-1))
    bk.beam_scores.fill_(NEG)
    bk.heur.fill_(1)
    bk.tokens.fill_(decoder_start_token_id)
    return bk


def _stable_top(x: torch.Tensor, k: int) -> List[int]:
    """Indices of the top ``k`` of ``x`` in ``rp_beam_select``'s total order: descending, equal values (-0.0 == +0.0) to
    the lower index."""
    v = x.tolist()
    return sorted(range(len(v)), key=lambda j: (-v[j], j))[:k]


BEAM_ADVANCE_MUTANTS = ("late_candidates_finish", "heuristic_not_sticky", "ancestry_not_reordered", "done_not_frozen")


POOL_BOOKS_MUTANTS = ("shared_position", "admit_not_reset")


def _state_init_host(books: BeamBooks, s: int, eos_token_id: int, decoder_start_token_id: int, tables: bool = True) -> None:
    """``_BeamState.__init__``'s values in the by-state parts of state ``s`` (the device routine ``rp_beam_books_init``
    and ``rp_beam_books_admit`` share)."""
    nb, L = books.nb, books.max_len
    if tables:
        for tab in (books.run_seq, books.fin_seq):
            tab[:, s] = eos_token_id
            tab[:, s, :, 0] = decoder_start_token_id
        books.anc[:, s] = (torch.arange(L, dtype=torch.int32)[None] * nb + torch.arange(nb, dtype=torch.int32)[:, None])
    books.run_scores[s] = NEG
    books.run_scores[s, 0] = 0.0
    books.beam_scores[s] = NEG
    books.fin_flag[s] = 0
    books.fin_len[s] = 0
    books.heur[s] = 1
    books.done[s] = 0
    books.steps[s] = 0


def beam_books_admit_host(books: BeamBooks, states: Sequence[int], eos_token_id: int, decoder_start_token_id: int,
                          mutant: Optional[str] = None) -> None:
    """``rp_beam_books_admit`` on host books: ``beam_books_init_host``'s values for ``states`` only - every by-state part
    of those states over all ``max_len`` columns, both pair members (a previous tenant wrote them).  Nothing by row and
    nothing of another state is touched.  ``mutant`` "admit_not_reset" (``POOL_BOOKS_MUTANTS``): the row tables of a
    state that was used before stay as its last tenant left them."""
    assert mutant is None or mutant in POOL_BOOKS_MUTANTS, mutant
    assert len(set(states)) == len(states) and all(0 <= s < books.n for s in states)
    for s in states:
        used = int(books.steps[s]) > 0
        _state_init_host(books, s, eos_token_id, decoder_start_token_id,
                         tables=not (mutant == "admit_not_reset" and used))


def beam_books_rows_host(books: BeamBooks, active: Sequence[int], pos: Sequence[int]) -> None:
    """``rp_beam_books_rows`` on host books: the by-row inputs (``tokens``, ``running``, ``anc_rows``) of rows
    ``a * nb + b`` from the by-state parts of state ``active[a]``, read at its current pair member ``pos[a] & 1`` and
    column ``pos[a]`` of ``run_seq``."""
    nb, L = books.nb, books.max_len
    assert len(active) == len(pos) and len(set(active)) == len(active) and all(0 <= s < books.n for s in active)
    assert all(0 <= p <= L - 2 for p in pos)
    for a, (s, p) in enumerate(zip(active, pos)):
        books.anc_rows[a * nb : (a + 1) * nb] = books.anc[p & 1, s]
        books.tokens[a * nb : (a + 1) * nb] = books.run_seq[p & 1, s, :, p]
        books.running[a * nb : (a + 1) * nb] = books.run_scores[s]


def beam_pool_advance_host(books: BeamBooks, active: Sequence[int], pos: Sequence[int], scores: torch.Tensor,
                           tokens: torch.Tensor, parents: torch.Tensor, fin_div: Sequence[float],
                           run_div: Sequence[float], eos_token_id: int, mutant: Optional[str] = None) -> None:
    """``rp_beam_pool_advance`` on host books: ``beam_advance_host`` with slot ``a`` at its own position ``pos[a]`` and
    with its own divisors ``fin_div[a]`` / ``run_div[a]``.  ``mutant``: ``BEAM_ADVANCE_MUTANTS`` joined by "+", or
    "shared_position" (``POOL_BOOKS_MUTANTS``: every slot handed the step's largest position)."""
    assert len(pos) == len(active) == len(fin_div) == len(run_div)
    mutants = set(mutant.split("+")) if mutant else set()
    if "shared_position" in mutants:
        mutants.discard("shared_position")
        pos = [max(pos)] * len(pos)
    assert mutants <= set(BEAM_ADVANCE_MUTANTS), mutant
    _advance_host(books, active, pos, scores, tokens, parents, fin_div, run_div, eos_token_id, mutants)


def beam_advance_host(books: BeamBooks, active: Sequence[int], t: int, scores: torch.Tensor, tokens: torch.Tensor,
                      parents: torch.Tensor, fin_div: float, run_div: float, eos_token_id: int,
                      mutant: Optional[str] = None) -> None:
    """``rp_beam_advance`` restated on host books: ``_BeamState.advance`` for the states ``active`` at position ``t``
    from the step's ``[n_active, 2 nb]`` selected triples, with both selections in the stated stable order
    (``_stable_top``; ``torch.topk`` promises none among ties) and the same writes as the kernel, so that the whole block
    compares bit for bit.  ``fin_div`` / ``run_div``: the two divisors ``(t + 1) ** length_penalty`` of
    ``_BeamState.advance`` (finished scores; ``best_running`` after ``cur_len`` advanced), rounded to fp32 here as the C
    ABI's float arguments are.  A state whose ``done`` is set is left as it is.  ``mutant`` plants known bugs (one name
    of ``BEAM_ADVANCE_MUTANTS`` or several joined by "+") so that tests can show a comparison would notice them."""
    mutants = set(mutant.split("+")) if mutant else set()
    assert mutants <= set(BEAM_ADVANCE_MUTANTS), mutant
    k = len(active)
    _advance_host(books, active, [t] * k, scores, tokens, parents, [fin_div] * k, [run_div] * k, eos_token_id, mutants)


def _advance_host(books: BeamBooks, active: Sequence[int], pos: Sequence[int], scores: torch.Tensor, tokens: torch.Tensor,
                  parents: torch.Tensor, fin_divs: Sequence[float], run_divs: Sequence[float], eos_token_id: int,
                  mutants: set) -> None:
    """The one body of ``beam_advance_host`` and ``beam_pool_advance_host``, as the kernel is one: slot ``a`` at position
    ``pos[a]``."""
    n, nb, L = books.n, books.nb, books.max_len
    assert len(set(active)) == len(active) and all(0 <= s < n for s in active)
    assert all(0 <= t and t + 1 < L for t in pos)
    K = 2 * nb
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    width = 4 if L % 4 == 0 else 1  # the kernel moves rows in units of `width` columns
    for slot, s in enumerate(active):
        if int(books.done[s]) and "done_not_frozen" not in mutants:
            continue
        t, fin_div, run_div = pos[slot], fin_divs[slot], run_divs[slot]
        cur, new = t & 1, (t & 1) ^ 1
        ncol = (t + 2 + width - 1) // width * width
        val = scores[slot].to(torch.float32).cpu()
        tok = tokens[slot].to(torch.int32).cpu()
        par = parents[slot].to(torch.int64).cpu().clamp(0, nb - 1)
        heur = bool(books.heur[s])
        hits = (tok == eos_token_id) | torch.tensor(t + 2 >= L)
        run_lp = val + torch.where(hits, f32(NEG), f32(-0.0))
        nxt = _stable_top(run_lp, nb)
        just_finished = hits if "late_candidates_finish" in mutants else hits & (torch.arange(K) < nb)
        fin = val / f32(fin_div)
        fin = fin + f32(0.0 if heur else NEG)
        fin = fin + torch.where(just_finished, f32(-0.0), f32(NEG))
        merged = torch.cat([books.beam_scores[s], fin])
        sel = _stable_top(merged, nb)
        # the row gathers: columns 0 .. t of the source rows, column t + 1 the step's own
        topk_seq = books.run_seq[cur, s][par, :ncol].clone()
        topk_seq[:, t + 1] = tok
        src = torch.arange(nb) if "ancestry_not_reordered" in mutants else par[nxt]
        new_anc = books.anc[cur, s][src, :ncol].clone()
        new_anc[:, t + 1] = (t + 1) * nb + torch.arange(nb, dtype=torch.int32)
        books.run_seq[new, s][:, :ncol] = topk_seq[nxt]
        books.anc[new, s][:, :ncol] = new_anc
        books.anc_rows[slot * nb : (slot + 1) * nb, :ncol] = new_anc
        books.fin_seq[new, s][:, :ncol] = torch.cat([books.fin_seq[cur, s][:, :ncol], topk_seq])[sel]
        books.run_scores[s] = run_lp[nxt]
        books.tokens[slot * nb : (slot + 1) * nb] = tok[nxt]
        books.running[slot * nb : (slot + 1) * nb] = run_lp[nxt]
        books.beam_scores[s] = merged[sel]
        books.fin_flag[s] = torch.cat([books.fin_flag[s], just_finished.to(torch.int32)])[sel]
        books.fin_len[s] = torch.cat([books.fin_len[s], torch.full((K,), t + 1, dtype=torch.int32)])[sel]
        # the early-stop test and the stop flag
        best_running = books.run_scores[s, 0] / f32(run_div)
        worst = torch.where(books.fin_flag[s].bool(), books.beam_scores[s].min(), f32(NEG))
        unsatisfied = bool((best_running > worst).any())
        heur = unsatisfied if "heuristic_not_sticky" in mutants else (heur and unsatisfied)
        books.heur[s] = int(heur)
        books.done[s] = int(not heur or bool(hits.all()))
        books.steps[s] = t + 1


def beam_search_batch_device(step_many: Callable, select_many: Callable, advance: Callable, num_states: int,
                             num_beams: int, max_length: int, length_penalty: float = 1.0, eos_token_id: int = 1,
                             decoder_start_token_id: int = 0, num_return_sequences: Optional[int] = None,
                             sync_every: int = 16, device=None, init: Optional[Callable] = None,
                             to_host: Callable = lambda x: x.cpu(), prompts: Optional[Sequence] = None,
                             constraint=None) -> List[BeamSearchOutput]:
    """``beam_search_batch`` with the books on the device (``BeamBooks``): per position one ``step_many``, one
    ``select_many`` and one ``advance``, nothing uploaded but their arguments and nothing read back.  Every
    ``sync_every`` positions the ``num_states`` ``done`` flags are read once and the stopped states leave the active
    list; a stopped state that is still listed keeps being stepped, and ``advance`` leaves its books alone.  The loop
    ends when every state has stopped or at ``max_length``; then the block is read once.  Entry ``i`` is
    ``beam_search_batch``'s for any ``sync_every`` wherever ``torch.topk`` and the stable order pick the same
    candidates (always, unless live candidates tie exactly).

    - ``init(n, nb, max_length, eos, start) -> BeamBooks``: initialised books (default ``beam_books_init_host``, moved to
      ``device``).
    - ``step_many(active, tokens, ancestry, t) -> log_probs``: as in ``sample_search_batch``; ``tokens`` int32
      ``[n_active * nb]`` and ``ancestry`` int32 ``[n_active * nb, max_length]`` (columns ``0..t`` are read) are views
      of the books' by-row parts.
    - ``select_many(log_probs, running, nb, k)``: as in ``beam_search_batch``.
    - ``advance(books, active, t, scores, tokens, parents, fin_div, run_div, eos)``: ``rp_beam_advance``
      (``beam_advance_host`` on the host).
    - ``to_host``: the loop's every device-to-host copy goes through it (tests count them).

    ``constraint``: a ``ValueError`` (not built yet): after a device-side ``advance`` the automaton states would have to
    follow the parents that advance chose ("Constrained decoding")."""
    _refuse_prompts(prompts, "the device books (sync_every)")
    _refuse_constraint(constraint, "the device books (sync_every)")
    n, nb = int(num_states), int(num_beams)
    nret = nb if num_return_sequences is None else int(num_return_sequences)
    _check_room(max_length)
    if nb < 1 or n < 1 or sync_every < 1 or not 1 <= nret <= nb:
        raise ValueError(f"num_states={n}, num_beams={nb}, sync_every={sync_every} must all be >= 1 and "
                         f"num_return_sequences={nret} in 1..num_beams")
    if init is None:
        books = beam_books_init_host(n, nb, max_length, eos_token_id, decoder_start_token_id)
        if device is not None:
            books = BeamBooks(n, nb, max_length, block=books.block.to(device))
    else:
        books = init(n, nb, max_length, eos_token_id, decoder_start_token_id)
    prompt_len = 1
    active = list(range(n))
    t = 0
    while active and t + 1 < max_length:
        rows = len(active) * nb
        log_probs = step_many(list(active), books.tokens[:rows], books.anc_rows[:rows], t)
        vals, toks, parents = select_many(log_probs, books.running[:rows], nb, 2 * nb)
        cur_len = t + 1
        fin_div = float((cur_len + 1 - prompt_len) ** length_penalty)  # _BeamState.advance: the finished scores' divisor
        cur_len = cur_len + 1
        run_div = float((cur_len - prompt_len) ** length_penalty)      # ... and best_running's, after cur_len advanced
        advance(books, list(active), t, vals, toks, parents, fin_div, run_div, eos_token_id)
        t += 1
        if t % sync_every == 0 and t + 1 < max_length:
            done = to_host(books.done)  # the only host sync of the loop
            still = [i for i in active if not bool(done[i])]
            if still and len(still) != len(active):  # slots moved: the next step's inputs, by the new rows
                idx = torch.tensor(still, dtype=torch.int64, device=books.block.device)
                m = len(still) * nb
                books.tokens[:m] = books.run_seq[t & 1, idx, :, t].reshape(-1)
                books.running[:m] = books.run_scores[idx].reshape(-1)
                books.anc_rows[:m] = books.anc[t & 1, idx].reshape(m, max_length)
            active = still
    host = BeamBooks(n, nb, max_length, block=to_host(books.block))
    return [host.result(i, nret) for i in range(n)]


class BeamBooksPool(_SlotPool):
    """``BeamSearchPool`` with the books on the device: ``n_slots`` places, state index = slot place, one ``BeamBooks``
    block of ``n_slots`` states, a position per slot kept on the host.  Per ``step`` it runs one engine ``step``, one
    ``select_many`` and one ``advance``; nothing is uploaded but their arguments and the host ``active`` / ``pos`` lists,
    and nothing is read back.  A ticket's output is ``beam_search``'s for that source alone.

    At a *sync point* it (1) reads the ``done`` flags once, (2) reads the results of the states that stopped - their own
    ``fin_seq`` rows of the current member, ``beam_scores``, ``fin_len`` and ``steps``, gathered on the device into one
    buffer - (3) frees their slots, (4) admits queued sources into the lowest free slots (``admit``, then
    ``books_admit``) and (5), if the active list changed, runs ``rows``.  So at most two device-to-host copies per sync
    point, all through ``to_host``.  A sync point occurs after every ``sync_every`` steps since the last one, before a
    step whenever something is queued and a slot is known to be free, and at the step where the pool starts from idle
    (nothing is in flight then and nothing is read).  ``sync_points`` counts them.

    The trade-off: with ``sync_every = K > 1`` a result is delivered, and its slot taken again, up to ``K - 1`` steps
    after its state stopped.  Meanwhile the stopped slot is still stepped and ``advance`` leaves its books as they are.
    ``K = 1`` still removes the ancestry upload and the host ``advance`` and reads ``n_slots`` flags per step.  No launch
    carries ``pos + 1 >= max_length``: a slot that has advanced at ``max_length - 2`` is certainly done and is stepped
    at ``max_length - 2`` again until the next sync point.

    - ``admit(slots, sources)``: as in ``BeamSearchPool``.
    - ``step(active, pos, tokens, ancestry) -> log_probs``: ``tokens`` int32 ``[n_active * nb]`` and ``ancestry`` int32
      ``[n_active * nb, max_length]`` (columns ``0..pos[a]`` of slot ``active[a]``'s rows are read) are views of the
      books' by-row parts.
    - ``select_many(log_probs, running, nb, k)``: as in ``beam_search_batch``.
    - ``books_admit(books, states, eos, start)``: ``rp_beam_books_admit`` (default ``beam_books_admit_host``).
    - ``advance(books, active, pos, scores, tokens, parents, fin_div, run_div, eos)``: ``rp_beam_pool_advance``
      (``beam_pool_advance_host``); the divisors are per-slot lists.
    - ``rows(books, active, pos)``: ``rp_beam_books_rows`` (``beam_books_rows_host``).
    - ``to_host(x)``: every device-to-host copy.

    ``mutant`` (``POOL_BOOKS_MUTANTS``) plants a known bug in the host defaults."""

    def __init__(self, admit: Callable, step: Callable, n_slots: int, num_beams: int, max_length: int,
                 length_penalty: float = 1.0, eos_token_id: int = 1, decoder_start_token_id: int = 0,
                 num_return_sequences: Optional[int] = None, select_many: Callable = topk_select_many, device=None,
                 sync_every: int = 16, books_admit: Optional[Callable] = None, advance: Optional[Callable] = None,
                 rows: Optional[Callable] = None, to_host: Callable = lambda x: x.cpu(), mutant: Optional[str] = None,
                 constraint=None):
        assert mutant is None or mutant in POOL_BOOKS_MUTANTS, mutant
        _refuse_constraint(constraint, "the device books (sync_every)")
        super().__init__(n_slots, "num_beams", num_beams, max_length, sync_every)
        self.nret = self.nb if num_return_sequences is None else int(num_return_sequences)
        if not 1 <= self.nret <= self.nb:
            raise ValueError(f"num_return_sequences={self.nret} outside 1..num_beams={self.nb}")
        self.length_penalty, self.eos, self.start = length_penalty, eos_token_id, decoder_start_token_id
        self._admit, self._step, self._select_many, self._to_host = admit, step, select_many, to_host
        self._books_admit = books_admit or (lambda bk, states, eos, start: beam_books_admit_host(
            bk, states, eos, start, mutant="admit_not_reset" if mutant == "admit_not_reset" else None))
        self._advance = advance or (lambda bk, *a: beam_pool_advance_host(
            bk, *a, mutant="shared_position" if mutant == "shared_position" else None))
        self._rows = rows or beam_books_rows_host
        # every state is admitted before use
        self.books = self._book = BeamBooks(self.n_slots, self.nb, self.max_length, device=device)
        self._last_pos = self.max_length - 2  # (having advanced there the state is done: its books are frozen)

    def submit(self, source, prompt: Optional[Sequence[int]] = None) -> int:
        """Queue a source; its ticket names it in ``step``'s return.  (A decoder ``prompt`` is ``BeamSearchPool``'s: a
        ``ValueError`` here.)"""
        _refuse_prompts([prompt], "the device books (sync_every)")
        return self._issue(source)

    def _stopped(self) -> List[int]:
        done = self._to_host(self.books.done)
        return [s for s in self._active if bool(done[s])]

    def _results(self, stopped: List[int]) -> List[Tuple[int, BeamSearchOutput]]:
        """``BeamBooks.result`` of the stopped states from one buffer gathered on the device: per state its ``nret``
        ``fin_seq`` rows of the current member, ``beam_scores`` (as bits), ``fin_len``, ``steps``."""
        bk, nret, L = self.books, self.nret, self.max_length
        idx = torch.tensor(stopped, dtype=torch.int64, device=bk.block.device)
        steps = bk.steps[idx]
        buf = torch.cat([bk.fin_seq[(steps & 1).long(), idx, :nret].reshape(len(stopped), nret * L),
                         bk.beam_scores[idx, :nret].view(torch.int32), bk.fin_len[idx, :nret], steps[:, None]], dim=1)
        host = self._to_host(buf)
        out = []
        for j, s in enumerate(stopped):
            max_generated = int(host[j, nret * L + nret : nret * L + 2 * nret].max())
            seq = host[j, : nret * L].view(nret, L)[:, : 1 + max_generated].long().clone()
            scores = host[j, nret * L : nret * L + nret].clone().view(torch.float32)
            out.append((self._ticket[s], BeamSearchOutput(seq, scores)))
        return out

    def _admit_books(self, slots: List[int], new: List[tuple]) -> None:
        self._books_admit(self.books, slots, self.eos, self.start)

    def _launch(self, active: List[int], pos: List[int]) -> None:
        bk, nb, prompt_len = self.books, self.nb, 1
        rows = len(active) * nb
        log_probs = self._step(active, pos, bk.tokens[:rows], bk.anc_rows[:rows])
        vals, toks, parents = self._select_many(log_probs, bk.running[:rows], nb, 2 * nb)
        # _BeamState.advance's two divisors at cur_len = pos + 1, as beam_search_batch_device computes them
        fin_div = [float((p + 1 + 1 - prompt_len) ** self.length_penalty) for p in pos]
        run_div = [float((p + 2 - prompt_len) ** self.length_penalty) for p in pos]
        self._advance(bk, active, pos, vals, toks, parents, fin_div, run_div, self.eos)


def greedy_search(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], max_length: int, eos_token_id: int = 1,
                  decoder_start_token_id: int = 0, device=None, prompt: Optional[Sequence[int]] = None,
                  prefill: Optional[Callable] = None, constraint=None, mask: Optional[Callable] = None
                  ) -> BeamSearchOutput:
    """``generate(num_beams=1, do_sample=False, max_length=L)``, which HF runs as greedy search (``_sample`` without
    sampling), not as a one-beam beam search: the argmax token (ties to the lowest id) until EOS or ``max_length``
    tokens including the start token.  After an EOS candidate a beam search keeps looking and may return a longer
    sequence; greedy stops.  ``sequences_scores`` holds the sum of the chosen tokens' log-probs (HF reports none).
    ``greedy_search_batch`` with one state.  ``prompt`` / ``prefill``: as in ``beam_search``; the result starts with
    the start token and the prompt, as HF's does, and the score sums the generated tokens only."""
    return greedy_search_batch(lambda active, tokens, ancestry, pos=None: step(tokens, ancestry), 1, max_length,
                               eos_token_id, decoder_start_token_id, device,
                               prompts=None if prompt is None else [prompt],
                               prefill_many=None if prefill is None else (lambda states, rows: prefill(rows[0])),
                               constraint=constraint, mask=mask)[0]


def greedy_search_batch(step_many: Callable, num_states: int, max_length: int, eos_token_id: int = 1,
                        decoder_start_token_id: int = 0, device=None, prompts: Optional[Sequence] = None,
                        prefill_many: Optional[Callable] = None, constraint=None, mask: Optional[Callable] = None
                        ) -> List[BeamSearchOutput]:
    """The greedy loop (``greedy_search``'s semantics per source): ``num_states`` sources in lockstep, one beam each,
    one ``step_many`` (as in ``beam_search_batch``) and one readback of the active states' log-prob rows per position.
    A state leaves the active list at its EOS; the loop ends with the last one or at ``max_length``.

    ``prompts`` / ``prefill_many``: as in ``beam_search_batch`` with one beam.  State ``i`` starts at position ``P_i``
    with ``[start] + prompt`` as its sequence and ``step_many`` is handed ``pos=``; without prompts every state stands
    at the same position and ``pos=`` is not passed.  Either way a state leaves at its EOS or when its sequence holds
    ``max_length`` tokens.

    ``constraint`` / ``mask``: as in ``beam_search_batch`` with one beam - an automaton state per source, uploaded with the
    step's tokens, the row masked before it is read back."""
    _check_room(max_length)
    prompts = _check_prompts(prompts, num_states, max_length)
    mask = _constraint_mask(constraint, mask, False)
    if constraint is not None:  # (a rejected prompt: ValueError before anything is launched)
        q = [constraint.state_after(prompts[i] if prompts is not None else []) for i in range(num_states)]
    seqs = [[int(decoder_start_token_id)] for _ in range(num_states)]
    totals = [0.0] * num_states
    active = list(range(num_states))
    if prompts is not None:
        listed = [i for i in range(num_states) if prompts[i]]
        _prefill_prompts(prefill_many, lambda i, p, tok, anc: step_many([i], tok, anc, pos=[p]), listed,
                         [prompts[i] for i in listed], decoder_start_token_id, 1, device)
        for i in range(num_states):
            seqs[i].extend(prompts[i])
    while active:
        pos = [len(seqs[i]) - 1 for i in active]
        tokens = torch.tensor([seqs[i][-1] for i in active], dtype=torch.int64)
        cols = torch.arange(max(pos) + 1, dtype=torch.int64)[None]
        anc = cols * (cols <= torch.tensor(pos, dtype=torch.int64)[:, None])  # row a: 0..pos[a], then zeros
        if mask is not None:
            tokens, q_rows = _with_states(tokens, torch.tensor([q[i] for i in active], dtype=torch.int64), device)
            anc = anc if device is None else anc.to(device)
        elif device is not None:
            tokens, anc = tokens.to(device), anc.to(device)
        kw = {} if prompts is None else dict(pos=pos)
        lps = step_many(list(active), tokens, anc, **kw)
        if mask is not None:
            lps = mask(lps, q_rows)
        lps = lps.float().cpu()
        still = []
        for a, i in enumerate(active):
            lp = lps[a]
            best = int(torch.nonzero(lp == lp.max())[0, 0])
            if mask is not None:
                to = int(constraint.next[q[i], best])
                q[i] = to if to >= 0 else q[i]
            totals[i] += float(lp[best])
            seqs[i].append(best)
            if best != eos_token_id and len(seqs[i]) < max_length:
                still.append(i)
        active = still
    return [BeamSearchOutput(torch.tensor([s], dtype=torch.int64), torch.tensor([tot], dtype=torch.float32))
            for s, tot in zip(seqs, totals)]


@dataclass
class SampleState:
    """The per-row books of a sampled search, indexed by (state, sample); ``sample_step`` updates them in place."""
    seeds: torch.Tensor        # int32 [n]: the states' 32-bit seeds (the bits of a uint32)
    seq: torch.Tensor          # int32 [n, nb, max_length]: start token first, pad where nothing was written
    cum_logprob: torch.Tensor  # fp32 [n, nb]: sum of the model's log-probs of the drawn tokens
    n_generated: torch.Tensor  # int32 [n, nb]
    finished: torch.Tensor     # int32 [n, nb]
    tokens: torch.Tensor       # int32 [n * nb]: the next step's tokens by row (slot * nb + sample)
    # int32 [n, nb, 4] or None: the parameter table by (state, sample), rows of {temperature's fp32 bits, top_k, top_p's
    # fp32 bits, 0} (``SamplingParams.rows``).  None: the sampling parameters are ``sample_step``'s own, one set per call.
    params: Optional[torch.Tensor] = None


def check_sampling(temperature: float, top_k: int, top_p: float) -> None:
    """``ValueError`` for parameters outside the sampler's domain (``rp_sample_step``'s own rules)."""
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError(f"temperature={temperature} must be a positive finite number")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k={top_k} must be an integer >= 0 (0 = off)")
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p={top_p} must lie in (0, 1]")


def _f32_bits(x: float) -> int:
    """The bits of ``x`` as fp32, as the int32 that holds them."""
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


class SamplingParams:
    """One request's sampling parameters.  Each of ``temperature``, ``top_k`` and ``top_p`` is a scalar (every sample of
    the state) or a sequence with one value per sample (a ladder over the state's samples).  ``rows(nb)`` is the state's
    part of the sampler's parameter table."""

    def __init__(self, temperature=1.0, top_k=0, top_p=1.0):
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p

    def __repr__(self) -> str:
        return f"SamplingParams(temperature={self.temperature!r}, top_k={self.top_k!r}, top_p={self.top_p!r})"

    def values(self, nb: int) -> List[Tuple[float, int, float]]:
        """``(temperature, top_k, top_p)`` of each of ``nb`` samples, every one through ``check_sampling``;
        ``ValueError`` for a sequence that does not hold ``nb`` values."""
        nb = int(nb)
        if nb < 1:
            raise ValueError(f"num_samples={nb} must be >= 1")
        cols = []
        for name in ("temperature", "top_k", "top_p"):
            v = getattr(self, name)
            if isinstance(v, (str, bytes)):
                raise ValueError(f"{name}={v!r} is not a number or a sequence of numbers")
            if hasattr(v, "__len__"):
                if len(v) != nb:
                    raise ValueError(f"{name} holds {len(v)} values for {nb} samples")
                cols.append(list(v))
            else:
                cols.append([v] * nb)
        out = []
        for T, k, p in zip(*cols):
            check_sampling(T, k, p)
            if int(k) >= 2 ** 31:
                raise ValueError(f"top_k={k} does not fit 32 bits")
            out.append((float(T), int(k), float(p)))
        return out

    def rows(self, nb: int) -> torch.Tensor:
        """int32 ``[nb, 4]``: per sample the bits of fp32 ``temperature``, ``top_k``, the bits of fp32 ``top_p``, 0."""
        vals = self.values(nb)
        with np.errstate(over="ignore"):
            for T, _, p in vals:  # the domain holds for the fp32 values the kernel receives, too
                check_sampling(float(np.float32(T)), 0, float(np.float32(p)))
        return torch.tensor([[_f32_bits(T), k, _f32_bits(p), 0] for T, k, p in vals], dtype=torch.int32)


def sample_search_batch(step_many: Callable, sample_step: Callable, num_states: int, num_samples: int, max_length: int,
                        seeds: Sequence[int], length_penalty: float = 0.0, eos_token_id: int = 1,
                        decoder_start_token_id: int = 0, pad_token_id: int = 0, sync_every: int = 16,
                        device=None, params: Optional[torch.Tensor] = None,
                        prompts: Optional[Sequence] = None, constraint=None, mask: Optional[Callable] = None,
                        mutant: Optional[str] = None) -> List[BeamSearchOutput]:
    """The sampling loop: ``num_states`` sources in lockstep with ``num_samples`` independent rows each; per position one
    ``step_many`` and one ``sample_step``, nothing read back.  Every ``sync_every`` positions the finished flags are
    read once and the states whose samples have all finished leave the active list; the loop ends when it is empty or
    at ``max_length``.  A finished row of a state that is still active keeps being stepped (it is fed the pad token and
    its outputs are ignored): that is the price of not looking every step, and it changes no result, because a row's
    log-probs depend on no other row and its random numbers on (seed, sample, position) alone.  So entry ``i`` is the
    same bits whichever states share the call, in whatever order, for any ``sync_every``.

    - ``step_many(active, tokens, ancestry, t) -> log_probs``: as in ``beam_search_batch``, except that ``ancestry`` is
      the first ``n_active * nb`` rows of one identity table built here once, ``[num_states * nb, max_length]`` with
      entry ``[r, p] = p * nb + r % nb`` (row ``r`` keeps to its own cache rows), of which the step at position ``t``
      reads columns ``0..t``; ``tokens`` is int32 ``[n_active * nb]``.
    - ``sample_step(log_probs, active, t, state)``: draws one token per row and updates ``state`` (``SampleState``) as
      ``rp_sample_step`` does: token to ``seq[.., t + 1]`` and ``tokens``, the model's log-prob added to ``cum_logprob``,
      ``n_generated`` incremented, ``finished`` set at EOS; a finished row writes pad and nothing else.
    - ``params``: the parameter table int32 ``[num_states, num_samples, 4]`` (``SamplingParams.rows`` per state), or None.
      It becomes ``state.params``, from which ``sample_step`` takes row ``(state, sample)``'s parameters in place of
      its own; then row ``b`` of entry ``i`` is the same bits as row ``b`` of the search of source ``i`` alone in which
      every sample has the parameters of block ``(i, b)``.

    Returns per state ``sequences [num_samples, out_len]`` (start token first, pad after EOS, trimmed to the state's
    longest sample) in sample order and ``sequences_scores = cum_logprob / n_generated ** length_penalty`` (the
    finished-beam formula; the default 0.0 gives the sum).

    ``constraint`` (a ``constraint.ByteAutomaton``; None: the loop above, call for call): the rows' automaton states live
    on the device, int32 ``[num_states, num_samples]`` by (state, sample), and between ``step_many`` and ``sample_step``
    ``mask(log_probs, active, [t] * n_active, tokens, q)`` advances them by the tokens the step was fed and overwrites the
    forbidden entries with ``-inf`` (default ``constraint_mask_step_host``; the engine passes
    ``rp_constraint_mask_step``).  Nothing is read back.  The sampler gives a ``-inf`` entry no mass, and ``cum_logprob``
    stays the model's own log-prob of the drawn token.  ``mutant``: one of ``CONSTRAINT_MUTANTS`` (host default)."""
    _refuse_prompts(prompts, "sampling")
    mask = _constraint_mask(constraint, mask, True, mutant)
    n, nb = int(num_states), int(num_samples)
    _check_room(max_length)
    if len(seeds) != n:
        raise ValueError(f"{len(seeds)} seeds for {n} states")
    if nb < 1 or n < 1 or sync_every < 1:
        raise ValueError(f"num_states={n}, num_samples={nb}, sync_every={sync_every} must all be >= 1")
    seed_bits = torch.tensor([int(s) & 0xFFFFFFFF for s in seeds], dtype=torch.int64)
    st = SampleState(
        seeds=torch.where(seed_bits >= 2 ** 31, seed_bits - 2 ** 32, seed_bits).to(torch.int32),
        seq=torch.full((n, nb, max_length), pad_token_id, dtype=torch.int32),
        cum_logprob=torch.zeros((n, nb), dtype=torch.float32), n_generated=torch.zeros((n, nb), dtype=torch.int32),
        finished=torch.zeros((n, nb), dtype=torch.int32),
        tokens=torch.full((n * nb,), decoder_start_token_id, dtype=torch.int32))
    st.seq[:, :, 0] = decoder_start_token_id
    if params is not None:
        if tuple(params.shape) != (n, nb, 4) or params.dtype != torch.int32:
            raise ValueError(f"params of shape {tuple(params.shape)}, {params.dtype} for int32 {(n, nb, 4)}")
        st.params = params.contiguous()
    ancestry = (torch.arange(max_length, dtype=torch.int32)[None] * nb
                + (torch.arange(n * nb, dtype=torch.int32) % nb)[:, None]).contiguous()
    if device is not None:
        for f in ("seeds", "seq", "cum_logprob", "n_generated", "finished", "tokens"):
            setattr(st, f, getattr(st, f).to(device))
        if st.params is not None:
            st.params = st.params.to(device)  # the search's one upload of the table
        ancestry = ancestry.to(device)
    if mask is not None:
        q = torch.zeros((n, nb), dtype=torch.int32, device=device)
    active = list(range(n))
    t = 0
    while active and t + 1 < max_length:
        rows = len(active) * nb
        log_probs = step_many(list(active), st.tokens[:rows], ancestry[:rows], t)
        if mask is not None:
            log_probs = mask(log_probs, list(active), [t] * len(active), st.tokens[:rows], q)
        sample_step(log_probs, list(active), t, st)
        t += 1
        if t % sync_every == 0 and t + 1 < max_length:
            done = st.finished.bool().all(dim=1).cpu()  # the only host sync of the loop
            still = [i for i in active if not bool(done[i])]
            if still and len(still) != len(active):  # slots moved: the next step's tokens, by the new rows
                idx = torch.tensor(still, dtype=torch.int64, device=st.seq.device)
                st.tokens[: len(still) * nb] = st.seq[idx, :, t].reshape(-1)
            active = still
    seq, cum, ngen = st.seq.cpu().long(), st.cum_logprob.cpu(), st.n_generated.cpu()
    outs = []
    for i in range(n):
        out_len = 1 + int(ngen[i].max())
        scores = cum[i] / ngen[i].to(torch.float32) ** float(length_penalty)
        outs.append(BeamSearchOutput(seq[i, :, :out_len].clone(), scores))
    return outs


def sample_search(step: Callable, sample_step: Callable, num_samples: int, max_length: int, seed: int = 0,
                  length_penalty: float = 0.0, eos_token_id: int = 1, decoder_start_token_id: int = 0,
                  pad_token_id: int = 0, sync_every: int = 16, device=None,
                  params: Optional[torch.Tensor] = None, prompt: Optional[Sequence[int]] = None, constraint=None,
                  mask: Optional[Callable] = None, mutant: Optional[str] = None) -> BeamSearchOutput:
    """``sample_search_batch`` with one state: ``step(tokens, ancestry, t)``, ``sample_step`` as there; ``params`` is the
    state's int32 ``[num_samples, 4]`` block (``SamplingParams.rows``) or None.  (A decoder ``prompt`` is beam search's
    and greedy's: a ``ValueError`` here, as ``prompts`` is in ``sample_search_batch``.)  ``constraint`` / ``mask`` /
    ``mutant``: as there."""
    _refuse_prompts([prompt], "sampling")
    return sample_search_batch(lambda active, tokens, ancestry, t: step(tokens, ancestry, t), sample_step, 1,
                               num_samples, max_length, [seed], length_penalty, eos_token_id, decoder_start_token_id,
                               pad_token_id, sync_every, device, None if params is None else params[None],
                               constraint=constraint, mask=mask, mutant=mutant)[0]


# ---- continuous batching for the sampled search: a position per slot ---------------------------------------------------
SAMPLE_POOL_MUTANTS = ("shared_position", "admit_not_reset", "stale_tokens")
# ... and for the parameters and live rows per request: "stale_params" leaves the previous tenant's parameter blocks in
# place at admission, "params_by_row" reads the table at the launch row instead of (state, sample), "dead_rows_live"
# ignores the live-row count
SAMPLE_PARAMS_MUTANTS = ("stale_params", "params_by_row", "dead_rows_live")


def _seed_bits(seed: int) -> int:
    """A 32-bit seed as the int32 that holds its bits (``SampleState.seeds``)."""
    bits = int(seed) & 0xFFFFFFFF
    return bits - 2 ** 32 if bits >= 2 ** 31 else bits


def sample_books_admit_host(state: SampleState, states: Sequence[int], seeds: Sequence[int],
                            decoder_start_token_id: int = 0, pad_token_id: int = 0, mutant: Optional[str] = None,
                            n_live: Optional[Sequence[int]] = None, params: Optional[torch.Tensor] = None) -> None:
    """``rp_sample_pool_admit`` on host books: for ``states`` only, ``seeds[s]`` set, every ``seq`` row pad over all
    ``max_length`` columns with the start token in column 0 (a previous tenant wrote them), ``cum_logprob``,
    ``n_generated`` and ``finished`` zero.  Nothing of another state and nothing by row is touched.  ``mutant``
    "admit_not_reset" (``SAMPLE_POOL_MUTANTS``): ``seq`` and ``finished`` stay as the last tenant left them.

    ``n_live`` (one count in ``1..nb`` per admitted state; ``rp_sample_pool_admit_rows``): rows ``b >= n_live[i]`` of
    ``states[i]`` start with ``finished = 1``.  ``params`` (int32 ``[len(states), nb, 4]``): the admitted states' blocks
    of ``state.params``, and no other block.  ``mutant`` "stale_params" (``SAMPLE_PARAMS_MUTANTS``) leaves the blocks as
    they were, "dead_rows_live" ignores ``n_live``."""
    assert mutant is None or mutant in SAMPLE_POOL_MUTANTS + SAMPLE_PARAMS_MUTANTS, mutant
    n, nb, _ = state.seq.shape
    assert len(states) == len(seeds) and len(set(states)) == len(states) and all(0 <= s < n for s in states)
    assert n_live is None or (len(n_live) == len(states) and all(1 <= k <= nb for k in n_live)), n_live
    assert params is None or (state.params is not None and tuple(params.shape) == (len(states), nb, 4))
    for j, (s, seed) in enumerate(zip(states, seeds)):
        state.seeds[s] = _seed_bits(seed)
        if mutant != "admit_not_reset":
            state.seq[s] = pad_token_id
            state.seq[s, :, 0] = decoder_start_token_id
            state.finished[s] = 0
            if n_live is not None and mutant != "dead_rows_live":
                state.finished[s, int(n_live[j]):] = 1
        state.cum_logprob[s] = 0.0
        state.n_generated[s] = 0
        if params is not None and mutant != "stale_params":
            state.params[s] = params[j].to(state.params.device)


def sample_row_params_host(state: SampleState, active: Sequence[int], mutant: Optional[str] = None):
    """The table lookup of ``rp_sample_step_rows`` / ``rp_sample_pool_step_rows`` on host books: per launch row
    ``a * nb + b`` the ``(temperature, top_k, top_p)`` of block ``(active[a], b)`` of ``state.params``, the two floats
    as the fp32 values the kernel receives.  ``mutant`` "params_by_row" (``SAMPLE_PARAMS_MUTANTS``): block ``a * nb + b``
    of the flat table, the launch row's, instead."""
    assert mutant is None or mutant in SAMPLE_PARAMS_MUTANTS, mutant
    n, nb, _ = state.seq.shape
    assert state.params is not None and tuple(state.params.shape) == (n, nb, 4) and state.params.dtype == torch.int32
    table = state.params.cpu().contiguous().numpy().reshape(n * nb, 4)
    out = []
    for a, s in enumerate(active):
        for b in range(nb):
            w = table[a * nb + b if mutant == "params_by_row" else s * nb + b]
            out.append((float(w[0:1].view(np.float32)[0]), int(w[1]), float(w[2:3].view(np.float32)[0])))
    return out


def sample_books_rows_host(state: SampleState, active: Sequence[int], pos: Sequence[int]) -> None:
    """``rp_sample_pool_rows`` on host books: ``tokens[a * nb + b] = seq[active[a], b, pos[a]]``, the next step's tokens
    by row."""
    n, nb, L = state.seq.shape
    assert len(active) == len(pos) and len(set(active)) == len(active) and all(0 <= s < n for s in active)
    assert all(0 <= p <= L - 2 for p in pos)
    for a, (s, p) in enumerate(zip(active, pos)):
        state.tokens[a * nb : (a + 1) * nb] = state.seq[s, :, p]


class SamplePool(_SlotPool):
    """``sample_search_batch``'s loop with admission, the sampled counterpart of ``BeamBooksPool``: ``n_slots`` places,
    state index = slot place, the sampler's books (one ``SampleState`` of ``n_slots`` states) on the device, a position
    per slot kept on the host.  ``submit(source, seed)`` queues a source; per ``step`` it runs one engine ``step`` and one
    ``sample_step``, nothing is uploaded but their arguments and nothing is read back.  A ticket's output is
    ``sample_search``'s for that source alone at that seed, whichever sources share the pool, in whatever order and
    slots, for any ``n_slots`` and ``sync_every``: a row's log-probs depend on its own state and position only, and its
    random numbers on (seed, sample, position).

    At a *sync point* it (1) reads the ``finished`` flags once (reduced over a state's samples on the device: ``n_slots``
    ints), (2) reads the results of the states that stopped - their ``seq`` rows, ``cum_logprob`` (as bits) and
    ``n_generated``, gathered on the device into one buffer - (3) frees their slots, (4) admits queued sources into the
    lowest free slots (``admit``, then ``books_admit``) and (5), if the active list changed, runs ``rows``.  So at most
    two device-to-host copies per sync point, all through ``to_host``.  A sync point occurs after every ``sync_every``
    steps since the last one, before a step whenever something is queued and a slot is known to be free, at the step
    where the pool starts from idle, and after the step that took any slot to position ``max_length - 1``.  The last one
    is forced: that slot is done by length, which the host knows without reading anything, and it must not be stepped
    again - unlike a stopped beam state its books are not frozen, an unfinished row would draw again and add to
    ``cum_logprob`` (and no launch may carry ``pos + 1 >= max_length``).  ``sync_points`` counts them.

    Between sync points a state whose samples have all finished keeps being stepped; its rows write pad and change
    nothing else, as in ``sample_search_batch``.  The trade-off is ``BeamBooksPool``'s: with ``sync_every = K > 1`` a
    result is delivered, and its slot taken again, up to ``K - 1`` steps after its last sample finished.

    - ``admit(slots, sources)``: as in ``BeamSearchPool``.
    - ``step(active, pos, tokens, ancestry) -> log_probs``: ``tokens`` int32 ``[n_active * nb]`` is a view of the books'
      by-row part; ``ancestry`` int32 ``[n_active * nb, max_length]`` the first rows of the identity table
      ``[r, p] = p * nb + r % nb`` built here once (it depends on ``r % nb`` only, so it serves any active list), of
      which columns ``0..pos[a]`` of slot ``active[a]``'s rows are read.
    - ``sample_step(log_probs, active, pos, state)``: ``rp_sample_pool_step`` - ``sample_search_batch``'s ``sample_step``
      with slot ``active[a]`` at ``pos[a]``.  It has no host default.
    - ``books_admit(state, states, seeds, start, pad)``: ``rp_sample_pool_admit`` (default ``sample_books_admit_host``).
    - ``rows(state, active, pos)``: ``rp_sample_pool_rows`` (default ``sample_books_rows_host``).
    - ``to_host(x)``: every device-to-host copy.

    ``mutant`` (``SAMPLE_POOL_MUTANTS``) plants a known bug: "shared_position" samples every slot at the first slot's
    position, "admit_not_reset" leaves the previous tenant's ``seq`` / ``finished`` in place (host default), and
    "stale_tokens" skips ``rows`` after the active list changed.

    ``per_request=True`` (default off: everything above, call for call): the sampling parameters and the number of
    samples belong to the ticket.  The books carry the parameter table ``state.params`` (int32 ``[n_slots, nb, 4]``),
    from which ``sample_step`` takes row ``(state, sample)``'s parameters, and ``submit(source, seed, params,
    num_samples)`` takes a ``SamplingParams`` (None: ``params``, the pool's own, default ``SamplingParams()``) and any
    ``1 <= num_samples <= nb`` (None: ``nb``).  At admission ``books_admit`` is called with two keywords more,
    ``n_live`` (the tenants' ``num_samples``) and ``params`` (their blocks, int32 ``[m, nb, 4]``; the rows past
    ``num_samples`` hold the default parameters and are never read): ``rp_sample_pool_admit_rows`` and one upload of the
    blocks.  Nothing is uploaded per step.  Rows ``b >= num_samples`` start finished: they are stepped like any finished
    row (fed pad, their outputs ignored), keep ``n_generated = 0`` and do not delay the state's departure.  The ticket's
    output has ``num_samples`` rows, trimmed to its longest live sample, and equals ``sample_search`` of that source
    alone with ``num_samples`` rows at that seed and those parameters: row ``b`` of the engine's step depends on no
    other row, its random number on (seed, sample, position), its parameters on (state, sample).  ``mutant``
    (``SAMPLE_PARAMS_MUTANTS``, host default of ``books_admit``): "stale_params" and "dead_rows_live";
    "params_by_row" is ``sample_row_params_host``'s, for a host ``sample_step``."""

    def __init__(self, admit: Callable, step: Callable, sample_step: Callable, n_slots: int, num_samples: int,
                 max_length: int, length_penalty: float = 0.0, decoder_start_token_id: int = 0, pad_token_id: int = 0,
                 sync_every: int = 16, device=None, books_admit: Optional[Callable] = None,
                 rows: Optional[Callable] = None, to_host: Callable = lambda x: x.cpu(), mutant: Optional[str] = None,
                 per_request: bool = False, params: Optional[SamplingParams] = None, constraint=None,
                 mask: Optional[Callable] = None):
        assert mutant is None or mutant in SAMPLE_POOL_MUTANTS + SAMPLE_PARAMS_MUTANTS + CONSTRAINT_MUTANTS, mutant
        assert per_request or (params is None and mutant not in SAMPLE_PARAMS_MUTANTS), "these need per_request=True"
        super().__init__(n_slots, "num_samples", num_samples, max_length, sync_every)
        n, nb, L = self.n_slots, self.nb, self.max_length
        # the constraint (None: the pool above, call for call): the rows' automaton states by (state, sample) on the
        # device; a slot's next tenant starts clean because its first step stands at position 0
        self._mask = _constraint_mask(constraint, mask, True, mutant)
        if self._mask is not None:
            self.q = torch.zeros((n, nb), dtype=torch.int32, device=device)
        self.length_penalty, self.mutant = length_penalty, mutant
        self.start, self.pad = decoder_start_token_id, pad_token_id
        self._admit, self._step, self._sample_step, self._to_host = admit, step, sample_step, to_host
        host_mutant = mutant if mutant in ("admit_not_reset", "stale_params", "dead_rows_live") else None
        self._books_admit = books_admit or (lambda st, states, seeds, start, pad, **kw: sample_books_admit_host(
            st, states, seeds, start, pad, mutant=host_mutant, **kw))
        self._rows = (lambda *a: None) if mutant == "stale_tokens" else (rows or sample_books_rows_host)
        self.per_request = bool(per_request)
        self._own = None                                             # per_request: the pool's own block [nb, 4]
        self._request = {}                                           # per_request: ticket -> (num_samples, block)
        self._live = [nb] * n                                        # per slot: its tenant's num_samples
        self.state = self._book = SampleState(  # every state is admitted before use
            seeds=torch.zeros(n, dtype=torch.int32, device=device),
            seq=torch.zeros((n, nb, L), dtype=torch.int32, device=device),
            cum_logprob=torch.zeros((n, nb), dtype=torch.float32, device=device),
            n_generated=torch.zeros((n, nb), dtype=torch.int32, device=device),
            finished=torch.zeros((n, nb), dtype=torch.int32, device=device),
            tokens=torch.zeros(n * nb, dtype=torch.int32, device=device))
        if self.per_request:
            self._own = (params or SamplingParams()).rows(nb)
            self._pad_block = SamplingParams().rows(nb)  # what the rows past a tenant's num_samples hold
            table = self._own[None].repeat(n, 1, 1).contiguous()
            self.state.params = table if device is None else table.to(device)
        ancestry = (torch.arange(L, dtype=torch.int32)[None] * nb
                    + (torch.arange(n * nb, dtype=torch.int32) % nb)[:, None]).contiguous()
        self.ancestry = ancestry if device is None else ancestry.to(device)
        self._last_pos = L - 1  # (a slot that stands there is freed at the forced sync point, before any step)

    def submit(self, source, seed: int, params: Optional[SamplingParams] = None,
               num_samples: Optional[int] = None, prompt: Optional[Sequence[int]] = None) -> int:
        """Queue a source with its 32-bit seed; its ticket names it in ``step``'s return.  With ``per_request``:
        ``params`` are the ticket's sampling parameters (None: the pool's own) and ``num_samples`` its number of rows
        (None: the pool's); without it either is a ``ValueError``.  A decoder ``prompt`` is a ``ValueError``."""
        _refuse_prompts([prompt], "sampling")
        request = None
        if not self.per_request:
            if params is not None or num_samples is not None:
                raise ValueError("params / num_samples per ticket need a pool opened with per_request=True")
        else:
            k = self.nb if num_samples is None else num_samples
            if int(k) != k or not 1 <= k <= self.nb:
                raise ValueError(f"num_samples={num_samples} must be an integer in 1..{self.nb}, the pool's num_samples")
            k = int(k)
            # (every row of a ticket's own parameters goes through check_sampling here)
            block = torch.cat([self._own[:k] if params is None else params.rows(k), self._pad_block[k:]])
            request = (k, block)
        ticket = self._issue(source, int(seed))
        if request is not None:
            self._request[ticket] = request
        return ticket

    def _stopped(self) -> List[int]:
        done = self._to_host(self.state.finished.bool().all(dim=1).to(torch.int32))
        return [s for s in self._active if bool(done[s]) or self._pos[s] + 1 >= self.max_length]

    def _results(self, stopped: List[int]) -> List[Tuple[int, BeamSearchOutput]]:
        """``sample_search_batch``'s outputs of the stopped states from one buffer gathered on the device: per state its
        ``seq`` rows, ``cum_logprob`` (as bits), ``n_generated``."""
        st, nb, L = self.state, self.nb, self.max_length
        idx = torch.tensor(stopped, dtype=torch.int64, device=st.seq.device)
        buf = torch.cat([st.seq[idx].reshape(len(stopped), nb * L), st.cum_logprob[idx].view(torch.int32),
                         st.n_generated[idx]], dim=1)
        host = self._to_host(buf)
        out = []
        for j, s in enumerate(stopped):
            k = self._live[s]  # the tenant's rows: the rows past them never drew (n_generated 0), so the trim is the live rows'
            ngen = host[j, nb * L + nb :]
            cum = host[j, nb * L : nb * L + nb].clone().view(torch.float32)[:k]
            seq = host[j, : nb * L].view(nb, L)[:k, : 1 + int(ngen.max())].long().clone()
            out.append((self._ticket[s],
                        BeamSearchOutput(seq, cum / ngen[:k].to(torch.float32) ** float(self.length_penalty))))
        return out

    def _admit_books(self, slots: List[int], new: List[tuple]) -> None:
        seeds = [seed for _, _, seed in new]
        if not self.per_request:
            self._books_admit(self.state, slots, seeds, self.start, self.pad)
            return
        requests = [self._request.pop(ticket) for ticket, _, _ in new]
        self._books_admit(self.state, slots, seeds, self.start, self.pad, n_live=[k for k, _ in requests],
                          params=torch.stack([blk for _, blk in requests]))
        for s, (k, _) in zip(slots, requests):
            self._live[s] = k

    def _launch(self, active: List[int], pos: List[int]) -> None:
        rows = len(active) * self.nb
        log_probs = self._step(active, pos, self.state.tokens[:rows], self.ancestry[:rows])
        if self._mask is not None:
            log_probs = self._mask(log_probs, list(active), list(pos), self.state.tokens[:rows], self.q)
        self._sample_step(log_probs, active, [pos[0]] * len(pos) if self.mutant == "shared_position" else list(pos),
                          self.state)
