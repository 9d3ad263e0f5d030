"""Constrained decoding: a deterministic automaton over token ids that says, after every prefix, which tokens may follow.

HuggingFace's ``generate(prefix_allowed_tokens_fn=fn)`` (``PrefixConstrainedLogitsProcessor``: ``scores + mask`` with
``-inf`` at every id ``fn`` does not list) with ``fn`` walking a ``ByteAutomaton``.  The generation loops
(``generation.py``) keep one automaton state per row and overwrite the forbidden entries of every step's log-probs with
``-inf`` before the selection or the sampler sees them; on the GPU that is one launch per step (``rp_constraint_mask`` /
``rp_constraint_mask_step``, DESIGN.md section 9 "Constrained decoding").

The table: ``next`` int16 ``[S, vocab]``, state 0 the start state, ``next[s, v]`` the state after token ``v`` in state
``s`` and ``-1`` where ``v`` is forbidden there.  A state *accepts* when it allows EOS; where EOS leads does not matter
(a row that drew it is finished) as long as it is a state.  ``S <= 4096``.  The constructor refuses a table in which a row
could get stuck: a reachable state that allows no token, or a reachable state from which no accepting state can be
reached.

Builders, over ByT5's ids (byte ``b`` is token ``b + offset``, ``offset = 3``; pad 0, EOS 1, unk 2; ids from
``offset + 256`` on are the sentinels): ``utf8`` (well-formed UTF-8, Unicode Table 3-7), ``ban`` (no banned string
occurs, Aho-Corasick), ``trie`` (only these strings), ``null`` (everything), and ``a & b`` (both).
"""
from __future__ import annotations

from collections import deque
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

MAX_STATES = 4096  # rp_constraint_mask's n_q cap


def _byte_strings(strings: Iterable) -> List[bytes]:
    out = []
    for s in strings:
        b = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        if not b:
            raise ValueError("an empty string cannot be banned or listed")
        out.append(b)
    if not out:
        raise ValueError("no strings given")
    return out


class ByteAutomaton:
    """A deterministic automaton over token ids (module docstring).  ``next``: int16 ``[S, vocab]``; ``eos``: the EOS id."""

    def __init__(self, next: np.ndarray, eos: int = 1):
        table = np.ascontiguousarray(next, dtype=np.int16)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError(f"next of shape {table.shape}: int16 [S, vocab] expected")
        S, V = table.shape
        if S > MAX_STATES:
            raise ValueError(f"{S} states > {MAX_STATES}")
        if not 0 <= int(eos) < V:
            raise ValueError(f"eos={eos} outside the vocabulary of {V}")
        if not np.array_equal(table, np.asarray(next)) or int(table.max()) >= S:
            raise ValueError(f"next holds entries outside [-1, {S})")
        table = np.where(table < 0, np.int16(-1), table)
        self.next, self.eos, self.vocab, self.n_states = table, int(eos), V, S
        self._device: Dict[str, object] = {}
        # every state reachable from 0 allows a token, and an accepting state can be reached from it
        reach = np.zeros(S, dtype=bool)
        reach[0] = True
        todo = deque([0])
        while todo:
            s = todo.popleft()
            for t in np.unique(table[s][table[s] >= 0]):
                if not reach[t]:
                    reach[t] = True
                    todo.append(int(t))
        stuck = [s for s in np.nonzero(reach)[0] if not (table[s] >= 0).any()]
        if stuck:
            raise ValueError(f"state {int(stuck[0])} is reachable and allows no token: a row would get stuck there")
        alive = table[:, self.eos] >= 0  # can reach an accepting state
        changed = True
        while changed:
            to = np.where(table >= 0, alive[np.maximum(table, 0)], False).any(axis=1)
            new = alive | to
            changed = bool((new != alive).any())
            alive = new
        dead = np.nonzero(reach & ~alive)[0]
        if len(dead):
            raise ValueError(f"EOS cannot be reached from state {int(dead[0])}, which is reachable: a row would never end")

    # -- queries ---------------------------------------------------------------------------------------------------------
    def allowed(self, state: int) -> np.ndarray:
        """bool ``[vocab]``: the tokens that may follow in ``state``."""
        return self.next[int(state)] >= 0

    def accepts(self, state: int) -> bool:
        return bool(self.next[int(state), self.eos] >= 0)

    def state_after(self, tokens: Sequence[int], state: int = 0) -> int:
        """The state after ``tokens`` from ``state``; ``ValueError`` where the automaton rejects them."""
        s = int(state)
        for i, t in enumerate(tokens):
            t = int(t)
            to = int(self.next[s, t]) if 0 <= t < self.vocab else -1
            if to < 0:
                raise ValueError(f"the constraint forbids token {t} at index {i} of {[int(x) for x in tokens]}")
            s = to
        return s

    def viable(self, tokens: Sequence[int]) -> bool:
        """Whether ``tokens`` is a prefix the automaton allows."""
        try:
            self.state_after(tokens)
        except ValueError:
            return False
        return True

    def accepts_row(self, tokens: Sequence[int]) -> bool:
        """Whether ``tokens`` (ending with EOS or not) is allowed and, without its EOS, ends in an accepting state."""
        toks = [int(t) for t in tokens]
        if toks and toks[-1] == self.eos:
            toks = toks[:-1]
        try:
            return self.accepts(self.state_after(toks))
        except ValueError:
            return False

    def prefix_allowed_tokens_fn(self, prompt_len: int = 1):
        """HF's ``prefix_allowed_tokens_fn(batch_id, input_ids)`` over this automaton; the first ``prompt_len`` ids (the
        decoder start token) are not part of the constrained text.  After EOS (a finished row that HF keeps padding)
        everything is allowed: HF overwrites those rows itself."""
        def fn(batch_id, input_ids):
            toks = [int(t) for t in input_ids.tolist()][prompt_len:]
            if self.eos in toks:
                return list(range(self.vocab))
            return np.nonzero(self.allowed(self.state_after(toks)))[0].tolist()
        return fn

    def table(self):
        """The table as a host ``torch`` int16 tensor (shared, not to be written)."""
        return self.device_table("cpu")

    def device_table(self, device):
        """The contiguous int16 table on ``device``: uploaded once, cached."""
        import torch

        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.next).to(device).contiguous()
        return self._device[key]

    # -- builders --------------------------------------------------------------------------------------------------------
    @classmethod
    def null(cls, vocab: int, eos: int = 1) -> "ByteAutomaton":
        """One state, everything allowed: the unconstrained search."""
        return cls(np.zeros((1, int(vocab)), dtype=np.int16), eos)

    @classmethod
    def utf8(cls, vocab: int, offset: int = 3, eos: int = 1) -> "ByteAutomaton":
        """Well-formed UTF-8 as Unicode Table 3-7 defines it (no overlong forms, no surrogates, nothing above U+10FFFF);
        EOS only between characters; every id that is neither a byte nor EOS forbidden.  8 states."""
        nxt = np.full((8, int(vocab)), -1, dtype=np.int16)
        # 0 between characters; 1 / 2 / 5: one / two / three continuation bytes to go; 3 after E0 (A0..BF); 4 after ED
        # (80..9F); 6 after F0 (90..BF); 7 after F4 (80..8F)
        arcs = [(0, 0x00, 0x7F, 0), (0, 0xC2, 0xDF, 1), (0, 0xE0, 0xE0, 3), (0, 0xE1, 0xEC, 2), (0, 0xED, 0xED, 4),
                (0, 0xEE, 0xEF, 2), (0, 0xF0, 0xF0, 6), (0, 0xF1, 0xF3, 5), (0, 0xF4, 0xF4, 7),
                (1, 0x80, 0xBF, 0), (2, 0x80, 0xBF, 1), (3, 0xA0, 0xBF, 1), (4, 0x80, 0x9F, 1),
                (5, 0x80, 0xBF, 2), (6, 0x90, 0xBF, 2), (7, 0x80, 0x8F, 2)]
        for s, lo, hi, to in arcs:
            for b in range(lo, hi + 1):
                if offset + b < vocab:
                    nxt[s, offset + b] = to
        nxt[0, eos] = 0
        return cls(nxt, eos)

    @classmethod
    def ban(cls, strings: Iterable, vocab: int, offset: int = 3, eos: int = 1) -> "ByteAutomaton":
        """No listed string (its UTF-8 bytes) occurs in the output: Aho-Corasick over the strings, the transition that
        would complete one forbidden.  Every state accepts; ids that are neither a byte nor EOS are forbidden."""
        pats = _byte_strings(strings)
        goto: List[Dict[int, int]] = [{}]
        out = [False]
        for p in pats:
            s = 0
            for b in p:
                if b not in goto[s]:
                    goto.append({})
                    out.append(False)
                    goto[s][b] = len(goto) - 1
                s = goto[s][b]
            out[s] = True
        fail = [0] * len(goto)
        delta = [[0] * 256 for _ in goto]
        order = deque()
        for b in range(256):
            t = goto[0].get(b, 0)
            delta[0][b] = t
            if t:
                order.append(t)
        while order:
            s = order.popleft()
            out[s] = out[s] or out[fail[s]]
            for b in range(256):
                t = goto[s].get(b)
                if t is None:
                    delta[s][b] = delta[fail[s]][b]
                else:
                    fail[t] = delta[fail[s]][b]
                    delta[s][b] = t
                    order.append(t)
        keep = [s for s in range(len(goto)) if not out[s]]  # the states a row can stand in
        index = {s: i for i, s in enumerate(keep)}
        nxt = np.full((len(keep), int(vocab)), -1, dtype=np.int64)
        for s in keep:
            for b in range(256):
                t = delta[s][b]
                if not out[t] and offset + b < vocab:
                    nxt[index[s], offset + b] = index[t]
            nxt[index[s], eos] = index[s]
        if len(keep) > MAX_STATES:
            raise ValueError(f"{len(keep)} states > {MAX_STATES}")
        return cls(nxt.astype(np.int16), eos)

    @classmethod
    def trie(cls, strings: Iterable, vocab: int, offset: int = 3, eos: int = 1) -> "ByteAutomaton":
        """Only the listed strings (their UTF-8 bytes), each followed by EOS."""
        pats = _byte_strings(strings)
        if any(offset + b >= vocab for p in pats for b in p):
            raise ValueError(f"a listed string holds a byte outside the vocabulary of {vocab}")
        rows: List[Dict[int, int]] = [{}]
        for p in pats:
            s = 0
            for b in p:
                if offset + b not in rows[s]:
                    rows.append({})
                    rows[s][offset + b] = len(rows) - 1
                s = rows[s][offset + b]
            rows[s][eos] = s
        if len(rows) > MAX_STATES:
            raise ValueError(f"{len(rows)} states > {MAX_STATES}")
        nxt = np.full((len(rows), int(vocab)), -1, dtype=np.int16)
        for s, arcs in enumerate(rows):
            for v, t in arcs.items():
                nxt[s, v] = t
        return cls(nxt, eos)

    def __and__(self, other: "ByteAutomaton") -> "ByteAutomaton":
        """The product: a token is allowed where both allow it.  Only the pairs reachable from (0, 0) become states."""
        if not isinstance(other, ByteAutomaton):
            return NotImplemented
        if (self.vocab, self.eos) != (other.vocab, other.eos):
            raise ValueError(f"automata over different vocabularies: {(self.vocab, self.eos)} and {(other.vocab, other.eos)}")
        index: Dict[Tuple[int, int], int] = {(0, 0): 0}
        todo = deque([(0, 0)])
        rows = []
        while todo:
            sa, sb = todo.popleft()
            na, nb = self.next[sa].astype(np.int64), other.next[sb].astype(np.int64)
            ok = (na >= 0) & (nb >= 0)
            row = np.full(self.vocab, -1, dtype=np.int64)
            code = na * other.n_states + nb
            for c in np.unique(code[ok]):
                pair = (int(c) // other.n_states, int(c) % other.n_states)
                if pair not in index:
                    index[pair] = len(index)
                    if len(index) > MAX_STATES:
                        raise ValueError(f"the product has more than {MAX_STATES} states")
                    todo.append(pair)
                row[ok & (code == c)] = index[pair]
            rows.append(row)
        return ByteAutomaton(np.stack(rows).astype(np.int16), self.eos)
