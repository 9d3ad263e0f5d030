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

There is one loop per search kind, over 1..n sources (``beam_search_batch``, ``greedy_search_batch``,
``sample_search_batch``); ``beam_search``, ``greedy_search`` and ``sample_search`` wrap their callables into its ``_many``
protocol and run it with one source.

Sampling (``sample_search_batch``) keeps its whole state on the device and reads nothing back per step: rows never
reorder, so the ancestry table is the identity, and the finished flags are read once every ``sync_every`` positions.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

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


class _BeamState:
    """The host bookkeeping of one source's beam search: ``inputs`` gives the step's tokens and ancestry table,
    ``advance`` takes the step's top-``2 nb`` candidates (host tensors) and says whether the search is over.
    ``beam_search_batch`` drives one per source in lockstep; ``beam_search`` is its one-source call."""

    def __init__(self, num_beams: int, max_length: int, length_penalty: float, eos_token_id: int,
                 decoder_start_token_id: int, num_return_sequences: Optional[int]):
        nb = self.nb = int(num_beams)
        self.nret = nb if num_return_sequences is None else int(num_return_sequences)
        assert 1 <= self.nret <= nb
        self.prompt_len = 1  # the decoder prompt is the start token alone (utils.py:3266 decoder_prompt_len = cur_len)
        self.cur_len = self.prompt_len
        self.keep = 2 * nb  # beams_to_keep = max(2, 1 + n_eos_tokens) * num_beams with one EOS id (:3271)
        fill = eos_token_id  # output_fill_value = pad_token_id (0, falsy) or eos_token_id[0] (:3294)
        if max_length <= self.cur_len:
            raise ValueError(f"max_length={max_length} leaves no room after the decoder start token")
        self.max_length, self.length_penalty, self.eos_token_id = max_length, length_penalty, eos_token_id

        self.running_seq = torch.full((nb, max_length), fill, dtype=torch.int64)
        self.running_seq[:, 0] = decoder_start_token_id
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
        self.ancestry = torch.zeros((nb, 0), dtype=torch.int64)

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
        fin_lp = vals / ((cur_len + 1 - prompt_len) ** length_penalty)
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
        self.running_seq, self.running_bi, self.running_scores = new_running_seq, new_running_bi, running_scores
        self.cur_len = cur_len = cur_len + 1
        # _check_early_stop_heuristic (:3008-3053), early_stopping=False: best length = cur_len - prompt_len
        best_running = running_scores[0] / ((cur_len - prompt_len) ** length_penalty)
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
                device=None, trace: Optional[list] = None) -> BeamSearchOutput:
    """Beam search over ``step`` (module docstring): ``beam_search_batch`` with one state.  ``trace``, when a list,
    receives the per-step top-``2 nb`` candidates ``(scores, tokens, parents)`` as host tensors."""
    traces: Optional[list] = None if trace is None else []
    out, = beam_search_batch(lambda active, tokens, ancestry: step(tokens, ancestry), 1, num_beams, max_length,
                             length_penalty, eos_token_id, decoder_start_token_id, num_return_sequences,
                             lambda lp, running, nb, k: tuple(x[None] for x in select(lp, running, k)), device, traces)
    if trace is not None:
        trace.extend(traces[0])
    return out


def topk_select_many(log_probs: torch.Tensor, running_scores: torch.Tensor, nb: int, k: int):
    """``topk_select`` per state over ``[n_active * nb, vocab]`` rows: each output ``[n_active, k]``."""
    outs = [topk_select(log_probs[a * nb : (a + 1) * nb], running_scores[a * nb : (a + 1) * nb], k)
            for a in range(log_probs.shape[0] // nb)]
    return tuple(torch.stack(x) for x in zip(*outs))


def beam_search_batch(step_many: Callable, num_states: int, num_beams: int, max_length: int, length_penalty: float = 1.0,
                      eos_token_id: int = 1, decoder_start_token_id: int = 0,
                      num_return_sequences: Optional[int] = None, select_many: Callable = topk_select_many, device=None,
                      traces: Optional[list] = None) -> List[BeamSearchOutput]:
    """The search loop: ``num_states`` sources in lockstep, one ``step_many`` and one ``select_many`` per position, one
    readback of the ``n_active x 2 nb`` triples.  Every state keeps its own bookkeeping (``_BeamState``) and leaves the
    active list at the step where it would stop alone; the loop runs until the last one has.

    - ``step_many(active, tokens, ancestry) -> log_probs``: ``active`` is the list of state indices still searching
      (ascending); row ``a * nb + b`` of ``tokens [n_active * nb]`` / ``ancestry [n_active * nb, t + 1]`` is beam ``b``
      of state ``active[a]``, ancestry entries local to that state's own cache.  Returns ``[n_active * nb, vocab]``.
    - ``select_many(log_probs, running_scores, nb, k)``: per state the top ``k`` of its own ``[nb * vocab]`` block,
      each output ``[n_active, k]``, parents local to the state.

    ``traces``, when a list, receives one per-state list of ``(scores, tokens, parents)`` per step."""
    states = [_BeamState(num_beams, max_length, length_penalty, eos_token_id, decoder_start_token_id,
                         num_return_sequences) for _ in range(num_states)]
    per_state = [[] for _ in states]
    active = list(range(num_states))
    nb = int(num_beams)
    while active:
        ins = [states[i].inputs() for i in active]
        tokens = torch.cat([x[0] for x in ins])
        ancestry = torch.cat([x[1] for x in ins])
        running = torch.cat([states[i].running_scores for i in active])
        if device is not None:
            tokens, ancestry, running = tokens.to(device), ancestry.to(device), running.to(device)
        log_probs = step_many(list(active), tokens, ancestry)
        vals, toks, parents = select_many(log_probs, running, nb, 2 * nb)
        vals, toks, parents = vals.float().cpu(), toks.long().cpu(), parents.long().cpu()  # the per-step host sync
        still = []
        for a, i in enumerate(active):
            if traces is not None:
                per_state[i].append((vals[a].clone(), toks[a].clone(), parents[a].clone()))
            if not states[i].advance(vals[a], toks[a], parents[a]):
                still.append(i)
        active = still
    if traces is not None:
        traces.extend(per_state)
    return [st.result() for st in states]


def greedy_search(step: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], max_length: int, eos_token_id: int = 1,
                  decoder_start_token_id: int = 0, device=None) -> BeamSearchOutput:
    """``generate(num_beams=1, do_sample=False, max_length=L)``, which HF runs as greedy search (``_sample`` without
    sampling), not as a one-beam beam search: the argmax token (ties to the lowest id) until EOS or ``max_length``
    tokens including the start token.  After an EOS candidate a beam search keeps looking and may return a longer
    sequence; greedy stops.  ``sequences_scores`` holds the sum of the chosen tokens' log-probs (HF reports none).
    ``greedy_search_batch`` with one state."""
    return greedy_search_batch(lambda active, tokens, ancestry: step(tokens, ancestry), 1, max_length, eos_token_id,
                               decoder_start_token_id, device)[0]


def greedy_search_batch(step_many: Callable, num_states: int, max_length: int, eos_token_id: int = 1,
                        decoder_start_token_id: int = 0, device=None) -> List[BeamSearchOutput]:
    """The greedy loop (``greedy_search``'s semantics per source): ``num_states`` sources in lockstep, one beam each,
    one ``step_many`` (as in ``beam_search_batch``) and one readback of the active states' log-prob rows per position.
    A state leaves the active list at its EOS; the loop ends with the last one or at ``max_length``."""
    if max_length <= 1:
        raise ValueError(f"max_length={max_length} leaves no room after the decoder start token")
    seqs = [[int(decoder_start_token_id)] for _ in range(num_states)]
    totals = [0.0] * num_states
    active = list(range(num_states))
    t = 0
    while active and t + 1 < max_length:
        tokens = torch.tensor([seqs[i][-1] for i in active], dtype=torch.int64)
        anc = torch.arange(t + 1, dtype=torch.int64)[None].repeat(len(active), 1)
        if device is not None:
            tokens, anc = tokens.to(device), anc.to(device)
        lps = step_many(list(active), tokens, anc).float().cpu()
        still = []
        for a, i in enumerate(active):
            lp = lps[a]
            best = int(torch.nonzero(lp == lp.max())[0, 0])
            totals[i] += float(lp[best])
            seqs[i].append(best)
            if best != eos_token_id:
                still.append(i)
        active = still
        t += 1
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


def check_sampling(temperature: float, top_k: int, top_p: float) -> None:
    """``ValueError`` for parameters outside the sampler's domain (``rp_sample_step``'s own rules)."""
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError(f"temperature={temperature} must be a positive finite number")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k={top_k} must be an integer >= 0 (0 = off)")
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p={top_p} must lie in (0, 1]")


def sample_search_batch(step_many: Callable, sample_step: Callable, num_states: int, num_samples: int, max_length: int,
                        seeds: Sequence[int], length_penalty: float = 0.0, eos_token_id: int = 1,
                        decoder_start_token_id: int = 0, pad_token_id: int = 0, sync_every: int = 16,
                        device=None) -> List[BeamSearchOutput]:
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

    Returns per state ``sequences [num_samples, out_len]`` (start token first, pad after EOS, trimmed to the state's
    longest sample) in sample order and ``sequences_scores = cum_logprob / n_generated ** length_penalty`` (the
    finished-beam formula; the default 0.0 gives the sum)."""
    n, nb = int(num_states), int(num_samples)
    if max_length <= 1:
        raise ValueError(f"max_length={max_length} leaves no room after the decoder start token")
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
    ancestry = (torch.arange(max_length, dtype=torch.int32)[None] * nb
                + (torch.arange(n * nb, dtype=torch.int32) % nb)[:, None]).contiguous()
    if device is not None:
        for f in ("seeds", "seq", "cum_logprob", "n_generated", "finished", "tokens"):
            setattr(st, f, getattr(st, f).to(device))
        ancestry = ancestry.to(device)
    active = list(range(n))
    t = 0
    while active and t + 1 < max_length:
        rows = len(active) * nb
        log_probs = step_many(list(active), st.tokens[:rows], ancestry[:rows], t)
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
                  pad_token_id: int = 0, sync_every: int = 16, device=None) -> BeamSearchOutput:
    """``sample_search_batch`` with one state: ``step(tokens, ancestry, t)``, ``sample_step`` as there."""
    return sample_search_batch(lambda active, tokens, ancestry, t: step(tokens, ancestry, t), sample_step, 1,
                               num_samples, max_length, [seed], length_penalty, eos_token_id, decoder_start_token_id,
                               pad_token_id, sync_every, device)[0]
