"""Tactic generators on libreprover_hip, mirroring prover/tactic_generator.py of the reference.

``HuggingFaceGenerator`` loads a T5ForConditionalGeneration checkpoint directory into ``HipT5Generator`` (HIP encoder +
decoder, beam search with HF's semantics, reprover_amd/generation.py); ``RetrievalAugmentedGenerator`` retrieves premises
with ``PremiseRetriever`` and generates from the augmented state.  No ``transformers`` import at run time.
"""
from __future__ import annotations

import asyncio
from typing import Dict, List, Optional, Sequence, Tuple

from ..common import Pos, format_augmented_state, remove_marks, zip_strict
from ..constraint import ByteAutomaton
from ..decoder import HipT5Generator
from ..generation import SamplingParams, check_sampling
from ..retrieval.model import PremiseRetriever
from ..tokenizer import ByT5Tokenizer, encode_one


class TacticGenerator:
    def initialize(self) -> None:
        raise NotImplementedError

    async def generate(self, state: str, file_path: str, theorem_full_name: str, theorem_pos: Pos,
                       num_samples: int) -> List[Tuple[str, float]]:
        raise NotImplementedError


class HuggingFaceGenerator(TacticGenerator):
    """Beam-search tactic generator (reference :169-243).  ``num_samples`` beams, ``num_samples`` returned sequences,
    ``max_length=max_oup_seq_len`` (the decoder start token included), ``early_stopping=False``.

    ``do_sample=True`` draws ``num_samples`` samples instead (temperature / top-k / top-p, ``HipT5Generator.sample_many``)
    and returns them sorted by score, best first (a stable sort), de-duplicated keeping the first occurrence.  The seed
    of a served state mixes ``seed`` with the number of states this object has served so far: repeated calls on one
    state differ, and ``batch_generate_sync([a, b])`` equals ``generate_sync(a)`` then ``generate_sync(b)``.

    ``beam_sync_every`` (an integer >= 1; default None): the beam search keeps its books on the device and looks at the
    states' stop flags every that many positions (``HipT5Generator.generate_many(sync_every=...)``); same outputs.

    ``continuous=True`` (beam search only): concurrent ``await generate(...)`` calls share one running decode loop
    (``HipT5Generator.generate_stream``, ``continuous_slots`` places, default the engine's cap).  A call joins the loop
    between two steps and returns as soon as its own state stops, with ``generate_sync``'s result.  One driver
    coroutine steps the loop while anything is queued or in flight and yields to the event loop between steps.  With
    ``beam_sync_every=K`` as well, the stream keeps its books on the device (``generate_stream(sync_every=K)``): the same
    results, each returned up to ``K - 1`` steps after its state stopped.

    ``sample_stream=True`` (with ``do_sample=True``, without ``continuous``) is the same for sampling: concurrent
    ``await generate(...)`` calls share one ``HipT5Generator.sample_stream`` (``sample_stream_slots`` places, default the
    engine's cap; its finished flags read every ``sample_sync_every`` steps) through the same driver.  A call takes its
    seed when it submits, in call order, so ``asyncio.gather(generate(a), generate(b))`` equals ``generate_sync(a)`` then
    ``generate_sync(b)`` on a fresh object with the same ``seed``.

    Sampling parameters per request: ``generate``, ``generate_sync`` (keyword ``sampling``, a ``SamplingParams``) and
    ``batch_generate_sync`` (keyword ``sampling``, a sequence with one ``SamplingParams`` or None per state) sample that
    state under its own temperature / top-k / top-p - scalars or a ladder over its ``num_samples`` samples - in place of
    the object's; None is the object's.  It needs ``do_sample=True``.  With ``sample_stream=True`` it also needs
    ``per_request_sampling=True``: the stream is then opened per request (``sample_stream(per_request=True)``) with
    ``sample_stream_samples`` rows (default: the first call's ``num_samples``), and a call with ``num_samples`` up to
    that joins the running stream with that many live rows instead of waiting for it to drain; a call that asks for
    more rows waits and re-opens.  Seeds are taken at submit time in call order, as above."""

    def __init__(self, model_path: str, device, max_inp_seq_len: int, max_oup_seq_len: int, length_penalty: float,
                 template: str = "%s", do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, seed: int = 0, beam_sync_every: Optional[int] = None, continuous: bool = False,
                 continuous_slots: Optional[int] = None, sample_stream: bool = False,
                 sample_stream_slots: Optional[int] = None, sample_sync_every: int = 16,
                 per_request_sampling: bool = False, sample_stream_samples: Optional[int] = None,
                 valid_utf8: bool = False, banned: Sequence[str] = ()):
        self.model_path = model_path
        self.device = device
        self.max_inp_seq_len = max_inp_seq_len
        self.max_oup_seq_len = max_oup_seq_len
        self.length_penalty = length_penalty
        self.template = template
        check_sampling(temperature, top_k, top_p)
        self.do_sample, self.temperature, self.top_k, self.top_p, self.seed = do_sample, temperature, top_k, top_p, seed
        self.states_served = 0
        if beam_sync_every is not None and (int(beam_sync_every) != beam_sync_every or beam_sync_every < 1):
            raise ValueError(f"beam_sync_every={beam_sync_every} must be an integer >= 1 (or None)")
        self.beam_sync_every = beam_sync_every
        # the default leaves the beam-search calls exactly as they were
        self._books = {} if beam_sync_every is None else {"sync_every": int(beam_sync_every)}
        if continuous and do_sample:
            raise ValueError("continuous=True serves beam search only: it cannot be combined with do_sample=True")
        if continuous_slots is not None and (int(continuous_slots) != continuous_slots or continuous_slots < 1):
            raise ValueError(f"continuous_slots={continuous_slots} must be an integer >= 1 (or None)")
        self.continuous, self.continuous_slots = bool(continuous), continuous_slots
        if sample_stream and (not do_sample or continuous):
            raise ValueError("sample_stream=True serves sampling only: it needs do_sample=True and continuous=False")
        if sample_stream_slots is not None and (int(sample_stream_slots) != sample_stream_slots or sample_stream_slots < 1):
            raise ValueError(f"sample_stream_slots={sample_stream_slots} must be an integer >= 1 (or None)")
        if int(sample_sync_every) != sample_sync_every or sample_sync_every < 1:
            raise ValueError(f"sample_sync_every={sample_sync_every} must be an integer >= 1")
        self.sample_stream, self.sample_stream_slots = bool(sample_stream), sample_stream_slots
        self.sample_sync_every = int(sample_sync_every)
        if per_request_sampling and not sample_stream:
            raise ValueError("per_request_sampling=True is a property of the sample stream: it needs sample_stream=True")
        if sample_stream_samples is not None and (not per_request_sampling or int(sample_stream_samples) != sample_stream_samples
                                                  or sample_stream_samples < 1):
            raise ValueError(f"sample_stream_samples={sample_stream_samples} must be an integer >= 1 (or None) and needs "
                             "per_request_sampling=True")
        self.per_request_sampling, self.sample_stream_samples = bool(per_request_sampling), sample_stream_samples
        # constrained decoding (defaults: none, every engine call as it was): the tactics are well-formed UTF-8 and / or
        # hold none of the ``banned`` strings - one automaton, ``utf8 & ban``, handed to every engine call
        if isinstance(banned, (str, bytes)):
            raise ValueError(f"banned={banned!r} is one string: a sequence of strings is expected")
        self.valid_utf8, self.banned = bool(valid_utf8), tuple(banned)
        if any(not isinstance(b, str) or not b for b in self.banned):
            raise ValueError(f"banned={banned!r} must hold non-empty strings")
        if (self.valid_utf8 or self.banned) and beam_sync_every is not None:
            raise ValueError("valid_utf8 / banned together with beam_sync_every (the device books) is not built yet")
        self._automaton = None
        self._stream = None       # the open GenerateStream (or SampleStream) and its num_samples
        self._stream_beams: Optional[int] = None
        self._waiters: Dict[int, "asyncio.Future"] = {}  # ticket -> the generate() call that awaits it
        self._driver: Optional["asyncio.Task"] = None

    def _next_seeds(self, n: int) -> List[int]:
        """The 32-bit seeds of the next ``n`` served states (murmur3's finaliser over seed + golden-ratio steps)."""
        out = []
        for _ in range(n):
            self.states_served += 1
            h = (int(self.seed) + self.states_served * 0x9E3779B1) & 0xFFFFFFFF
            h ^= h >> 16
            h = (h * 0x85EBCA6B) & 0xFFFFFFFF
            h ^= h >> 13
            h = (h * 0xC2B2AE35) & 0xFFFFFFFF
            out.append(h ^ (h >> 16))
        return out

    def _check_request(self, sampling, n: Optional[int] = None):
        """``sampling`` as given to a call: refused without ``do_sample``; for ``n`` states, a sequence of ``n``."""
        if sampling is None:
            return None
        if not self.do_sample:
            raise ValueError("sampling parameters per request need do_sample=True")
        if n is None:
            if not isinstance(sampling, SamplingParams):
                raise ValueError(f"sampling={sampling!r} is not a SamplingParams")
            return sampling
        sampling = list(sampling)
        if len(sampling) != n or not all(q is None or isinstance(q, SamplingParams) for q in sampling):
            raise ValueError(f"sampling holds {len(sampling)} entries for {n} states (one SamplingParams or None each)")
        return sampling

    def _constraint(self) -> Dict:
        """The engine calls' ``constraint=`` keyword: nothing without ``valid_utf8`` / ``banned``, else the one automaton
        (built at first use over the engine's vocabulary; ByT5's 384 ids where the engine names none)."""
        if not (self.valid_utf8 or self.banned):
            return {}
        if self._automaton is None:
            vocab = int(getattr(self.generator, "cfg", {}).get("vocab_size", 384))
            parts = ([ByteAutomaton.utf8(vocab)] if self.valid_utf8 else []) + (
                [ByteAutomaton.ban(self.banned, vocab)] if self.banned else [])
            self._automaton = parts[0] if len(parts) == 1 else parts[0] & parts[1]
        return {"constraint": self._automaton}

    def _prefix_ids(self, prefix: Optional[str]) -> Optional[List[int]]:
        """A tactic prefix as decoder prompt tokens: its UTF-8 bytes + 3, no EOS (None or "": no prompt, the call as it
        always was).  Refused with ``do_sample``, with ``beam_sync_every``, and when the start token and the prefix leave
        no room under ``max_oup_seq_len``."""
        if prefix is None or prefix == "":
            return None
        if not isinstance(prefix, str):
            raise ValueError(f"prefix={prefix!r} is not a string")
        if self.do_sample:
            raise ValueError("a tactic prefix together with do_sample=True is not built yet")
        if self.beam_sync_every is not None:
            raise ValueError("a tactic prefix together with beam_sync_every (the device books) is not built yet")
        ids = [b + 3 for b in prefix.encode("utf-8")]
        if self.max_oup_seq_len <= 1 + len(ids):
            raise ValueError(f"the prefix of {len(ids)} bytes leaves no room under max_oup_seq_len={self.max_oup_seq_len}")
        return ids

    def _sampled(self, ids, num_samples: int, sampling=None) -> List[List[Tuple[str, float]]]:
        results: List[List[Tuple[str, float]]] = []
        cap = self.generator.decoder.max_states(num_samples)
        if sampling is not None and all(q is None for q in sampling):
            sampling = None  # the object's parameters throughout: the call as it always was
        for i in range(0, len(ids), cap):
            chunk = ids[i : i + cap]
            kw = dict({} if sampling is None else {"params": sampling[i : i + cap]}, **self._constraint())
            outs = self.generator.sample_many(chunk, num_samples, self.max_oup_seq_len, self.temperature, self.top_k,
                                              self.top_p, self._next_seeds(len(chunk)), self.length_penalty, **kw)
            results.extend(self._sampled_suggestions(out) for out in outs)
        return results

    def _sampled_suggestions(self, out) -> List[Tuple[str, float]]:
        """A sampled search's output as (tactic, score) pairs: decoded, marks removed, sorted by score, best first (a
        stable sort), de-duplicated keeping the first occurrence."""
        text = self.tokenizer.batch_decode(out.sequences, skip_special_tokens=True)
        scores = out.sequences_scores.tolist()
        output_text, output_score = [], []
        for j in sorted(range(len(scores)), key=lambda j: -scores[j]):  # sorted() is stable
            t = remove_marks(text[j])
            if t not in output_text:
                output_text.append(t)
                output_score.append(scores[j])
        return list(zip_strict(output_text, output_score))

    def initialize(self) -> None:
        # A decoder-only checkpoint (the reference's AutoModelForCausalLM fallback) raises ValueError here.
        self.generator = HipT5Generator.from_pretrained(self.model_path, self.device)
        self.decoder_only = False
        self.tokenizer = ByT5Tokenizer()

    def generate_sync(self, state: str, file_path: str, theorem_full_name: str, theorem_pos: Pos,
                      num_samples: int, *, sampling: Optional[SamplingParams] = None,
                      prefix: Optional[str] = None) -> List[Tuple[str, float]]:
        """``prefix``: the tactics returned all begin with it (HF's ``decoder_input_ids``: the decoder prompt is the
        start token and the prefix's bytes), scored by HF's ``sequences_scores`` over the generated tokens."""
        sampling = self._check_request(sampling)
        prompt = self._prefix_ids(prefix)
        state = self.template % state
        ids = encode_one(state, self.max_inp_seq_len)  # tokenizer(state, max_length=..., truncation=True)
        if self.do_sample:
            return self._sampled([ids], num_samples, None if sampling is None else [sampling])[0]
        kw = dict({} if prompt is None else {"prefix": prompt}, **self._constraint())
        out = self.generator.generate(ids, num_samples, self.max_oup_seq_len, self.length_penalty, **self._books, **kw)
        return self._suggestions(out, num_samples)

    def _suggestions(self, out, num_samples: int) -> List[Tuple[str, float]]:
        """A beam search's output as (tactic, score) pairs: decoded, marks removed, de-duplicated in order (:227-243)."""
        raw_output_text = self.tokenizer.batch_decode(out.sequences, skip_special_tokens=True)
        raw_scores = out.sequences_scores.tolist()
        output_text, output_score = [], []
        for j in range(num_samples):
            t = remove_marks(raw_output_text[j])
            if t not in output_text:
                output_text.append(t)
                output_score.append(raw_scores[j])
        return list(zip_strict(output_text, output_score))

    async def generate(self, state: str, file_path: str, theorem_full_name: str, theorem_pos: Pos,
                       num_samples: int, *, sampling: Optional[SamplingParams] = None,
                       prefix: Optional[str] = None) -> List[Tuple[str, float]]:
        sampling = self._check_request(sampling)
        prompt = self._prefix_ids(prefix)
        if not (self.continuous or self.sample_stream):
            kw = {} if prompt is None else {"prefix": prefix}
            return self.generate_sync(state, file_path, theorem_full_name, theorem_pos, num_samples, sampling=sampling,
                                      **kw)
        if self.per_request_sampling:
            return await self._generate_per_request(state, num_samples, sampling)
        if sampling is not None:
            raise ValueError("sampling parameters per request on a sample stream need per_request_sampling=True")
        ids = encode_one(self.template % state, self.max_inp_seq_len)
        # a stream serves one num_samples: a call with another waits until it has drained (the driver runs meanwhile)
        while self._stream is not None and self._stream_beams != num_samples and (self._stream.queued
                                                                                  or self._stream.in_flight):
            await asyncio.sleep(0)
        if self._stream is None or self._stream_beams != num_samples:
            if self.sample_stream:
                self._stream = self.generator.sample_stream(num_samples, self.max_oup_seq_len, self.temperature,
                                                            self.top_k, self.top_p, self.length_penalty,
                                                            n_slots=self.sample_stream_slots,
                                                            src_cap=self.max_inp_seq_len,
                                                            sync_every=self.sample_sync_every, **self._constraint())
            else:
                self._stream = self.generator.generate_stream(num_samples, self.max_oup_seq_len, self.length_penalty,
                                                              n_slots=self.continuous_slots,
                                                              src_cap=self.max_inp_seq_len, **self._books,
                                                              **self._constraint())
            self._stream_beams = num_samples
        future = asyncio.get_running_loop().create_future()
        # (a sampled call's seed is taken here, at submit time: in call order)
        if self.sample_stream:
            ticket = self._stream.submit(ids, self._next_seeds(1)[0])
        elif prompt is None:
            ticket = self._stream.submit(ids)
        else:
            ticket = self._stream.submit(ids, prefix=prompt)  # the prefix travels with the ticket
        self._waiters[ticket] = future
        if self._driver is None:
            self._driver = asyncio.ensure_future(self._drive())
        out = await future
        return self._sampled_suggestions(out) if self.sample_stream else self._suggestions(out, num_samples)

    async def _generate_per_request(self, state: str, num_samples: int,
                                    sampling: Optional[SamplingParams]) -> List[Tuple[str, float]]:
        """``generate`` on a stream opened per request: a call whose ``num_samples`` fits the stream's rows joins it with
        that many live rows and its own parameters; only a call that asks for more rows waits for the drain."""
        if int(num_samples) != num_samples or num_samples < 1:
            raise ValueError(f"num_samples={num_samples} must be an integer >= 1")
        if sampling is not None:
            sampling.rows(num_samples)  # refused here, before a seed is taken
        ids = encode_one(self.template % state, self.max_inp_seq_len)
        while self._stream is not None and num_samples > self._stream_beams and (self._stream.queued
                                                                                 or self._stream.in_flight):
            await asyncio.sleep(0)
        if self._stream is None or num_samples > self._stream_beams:
            rows = max(int(num_samples), int(self.sample_stream_samples or 0))
            self._stream = self.generator.sample_stream(rows, self.max_oup_seq_len, self.temperature, self.top_k,
                                                        self.top_p, self.length_penalty,
                                                        n_slots=self.sample_stream_slots, src_cap=self.max_inp_seq_len,
                                                        sync_every=self.sample_sync_every, per_request=True,
                                                        **self._constraint())
            self._stream_beams = rows
        future = asyncio.get_running_loop().create_future()
        ticket = self._stream.submit(ids, self._next_seeds(1)[0], params=sampling, num_samples=num_samples)
        self._waiters[ticket] = future
        if self._driver is None:
            self._driver = asyncio.ensure_future(self._drive())
        return self._sampled_suggestions(await future)

    async def _drive(self) -> None:
        """Step the open stream while it has work, resolving the waiting calls as their states finish; an exception
        reaches every call that waits.  Between steps the event loop runs, so that other calls can submit (or, once the
        stream is idle, open the next one: the loop looks at ``self._stream`` afresh every time)."""
        try:
            while self._stream is not None and (self._stream.queued or self._stream.in_flight):
                for ticket, out in self._stream.step():
                    future = self._waiters.pop(ticket)
                    if not future.done():  # (a cancelled call)
                        future.set_result(out)
                if self._stream.queued or self._stream.in_flight:  # (idle: end now, before any waiter wakes)
                    await asyncio.sleep(0)
        except Exception as exc:  # the stream's state is unknown now: fail the waiters and open a fresh one next time
            waiters, self._waiters = self._waiters, {}
            self._stream = self._stream_beams = None
            for future in waiters.values():
                if not future.done():
                    future.set_exception(exc)
        finally:
            self._driver = None

    def batch_generate_sync(self, states: List[str], file_paths: List[str], theorem_full_names: List[str],
                            theorem_poses: List[Pos], num_samples: int, *, sampling=None,
                            prefixes=None) -> List[List[Tuple[str, float]]]:
        """``generate_sync`` for several states through one decode loop (``HipT5Generator.generate_many``): entry ``i``
        is ``generate_sync(states[i], ...)`` exactly (with ``sampling=sampling[i]`` and ``prefix=prefixes[i]``),
        de-duplication order included.  ``prefixes``: one string or None per state."""
        sampling = self._check_request(sampling, len(states))
        prompts = None
        if prefixes is not None:
            prefixes = list(prefixes)
            if len(prefixes) != len(states):
                raise ValueError(f"prefixes holds {len(prefixes)} entries for {len(states)} states")
            prompts = [self._prefix_ids(p) for p in prefixes]
            if all(p is None for p in prompts):
                prompts = None  # no prompt anywhere: the call as it always was
        ids = [encode_one(self.template % s, self.max_inp_seq_len) for s in states]
        if self.do_sample:
            return self._sampled(ids, num_samples, sampling)
        results: List[List[Tuple[str, float]]] = []
        cap = self.generator.decoder.max_states(num_samples)  # the engine's cap on states per call
        for i in range(0, len(ids), cap):
            kw = dict({} if prompts is None else {"prefixes": prompts[i : i + cap]}, **self._constraint())
            outs = self.generator.generate_many(ids[i : i + cap], num_samples, self.max_oup_seq_len,
                                                self.length_penalty, **self._books, **kw)
            results.extend(self._suggestions(out, num_samples) for out in outs)
        return results

    async def batch_generate(self, states: List[str], file_paths: List[str], theorem_full_names: List[str],
                             theorem_poses: List[Pos], num_samples: int) -> List[List[Tuple[str, float]]]:
        return self.batch_generate_sync(states, file_paths, theorem_full_names, theorem_poses, num_samples)


class RetrievalAugmentedGenerator(TacticGenerator):
    """Reference :246-298: retrieve, format the augmented state, generate."""

    def __init__(self, gen_path: str, ret_path: str, indexed_corpus_path: str, device, max_inp_seq_len: int,
                 max_oup_seq_len: int, length_penalty: float, max_num_retrieved: int, do_sample: bool = False,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                 beam_sync_every: Optional[int] = None, continuous: bool = False,
                 continuous_slots: Optional[int] = None, sample_stream: bool = False,
                 sample_stream_slots: Optional[int] = None, sample_sync_every: int = 16,
                 per_request_sampling: bool = False, sample_stream_samples: Optional[int] = None,
                 valid_utf8: bool = False, banned: Sequence[str] = ()) -> None:
        self.gen_path = gen_path
        self.ret_path = ret_path
        self.indexed_corpus_path = indexed_corpus_path
        self.device = device
        self.max_inp_seq_len = max_inp_seq_len
        self.max_oup_seq_len = max_oup_seq_len
        self.length_penalty = length_penalty
        self.max_num_retrieved = max_num_retrieved
        self.hf_gen = HuggingFaceGenerator(gen_path, device, max_inp_seq_len, max_oup_seq_len, length_penalty,
                                           do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                           seed=seed, beam_sync_every=beam_sync_every, continuous=continuous,
                                           continuous_slots=continuous_slots, sample_stream=sample_stream,
                                           sample_stream_slots=sample_stream_slots,
                                           sample_sync_every=sample_sync_every,
                                           per_request_sampling=per_request_sampling,
                                           sample_stream_samples=sample_stream_samples, valid_utf8=valid_utf8,
                                           banned=banned)

    def initialize(self) -> None:
        self.hf_gen.initialize()
        self.retriever = PremiseRetriever.load_hf(self.ret_path, self.max_inp_seq_len, self.device)
        self.retriever.load_corpus(self.indexed_corpus_path)

    def generate_sync(self, state: str, file_path: str, theorem_full_name: str, theorem_pos: Pos,
                      num_samples: int, *, sampling: Optional[SamplingParams] = None,
                      prefix: Optional[str] = None) -> List[Tuple[str, float]]:
        self.hf_gen._check_request(sampling)
        self.hf_gen._prefix_ids(prefix)
        retrieved_premises, _ = self.retriever.retrieve(state, file_path, theorem_full_name, theorem_pos,
                                                        self.max_num_retrieved)
        aug_state = format_augmented_state(state, retrieved_premises, self.max_inp_seq_len)
        kw = {} if sampling is None else {"sampling": sampling}
        if prefix:
            kw["prefix"] = prefix
        return self.hf_gen.generate_sync(aug_state, file_path, theorem_full_name, theorem_pos, num_samples, **kw)

    async def generate(self, state: str, file_path: str, theorem_full_name: str, theorem_pos: Pos,
                       num_samples: int, *, sampling: Optional[SamplingParams] = None,
                       prefix: Optional[str] = None) -> List[Tuple[str, float]]:
        kw = {} if sampling is None else {"sampling": sampling}
        if prefix:
            kw["prefix"] = prefix
        if not (self.hf_gen.continuous or self.hf_gen.sample_stream):
            return self.generate_sync(state, file_path, theorem_full_name, theorem_pos, num_samples, **kw)
        self.hf_gen._check_request(sampling)
        self.hf_gen._prefix_ids(prefix)
        retrieved_premises, _ = self.retriever.retrieve(state, file_path, theorem_full_name, theorem_pos,
                                                        self.max_num_retrieved)
        aug_state = format_augmented_state(state, retrieved_premises, self.max_inp_seq_len)
        return await self.hf_gen.generate(aug_state, file_path, theorem_full_name, theorem_pos, num_samples, **kw)

    def batch_generate_sync(self, states: List[str], file_paths: List[str], theorem_full_names: List[str],
                            theorem_poses: List[Pos], num_samples: int, *, sampling=None,
                            prefixes=None) -> List[List[Tuple[str, float]]]:
        """Retrieve per state (``retrieve``, as ``generate_sync``), format each augmented state, then one batched
        generate."""
        sampling = self.hf_gen._check_request(sampling, len(states))
        if prefixes is not None:
            prefixes = list(prefixes)
            for p in prefixes:
                self.hf_gen._prefix_ids(p)  # refused here, before any retrieval
        aug_states = []
        for state, path, name, pos in zip_strict(states, file_paths, theorem_full_names, theorem_poses):
            retrieved_premises, _ = self.retriever.retrieve(state, path, name, pos, self.max_num_retrieved)
            aug_states.append(format_augmented_state(state, retrieved_premises, self.max_inp_seq_len))
        kw = {} if sampling is None else {"sampling": sampling}
        if prefixes is not None:
            kw["prefixes"] = prefixes
        return self.hf_gen.batch_generate_sync(aug_states, file_paths, theorem_full_names, theorem_poses, num_samples, **kw)

    async def batch_generate(self, states: List[str], file_paths: List[str], theorem_full_names: List[str],
                             theorem_poses: List[Pos], num_samples: int) -> List[List[Tuple[str, float]]]:
        return self.batch_generate_sync(states, file_paths, theorem_full_names, theorem_poses, num_samples)


__all__ = ["TacticGenerator", "HuggingFaceGenerator", "RetrievalAugmentedGenerator", "SamplingParams"]
