"""What the constrained-decoding tests share: the G30 fixture (tests/golden/make_golden_constraint.py), its two automata,
and the property every returned row must have.  It never launches anything."""
from __future__ import annotations

import json
import os

import numpy as np

from reprover_amd import synth
from reprover_amd.constraint import ByteAutomaton

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOS = 1


def load_g30():
    """(arrays, meta) of G30."""
    z = np.load(os.path.join(GOLDEN, "g30_generate_constrained.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def g30_model(meta):
    """(cfg, state dict) of the fixture: the G20 weights."""
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][EOS] *= meta["eos_boost"]
    return cfg, sd


def g30_automata(meta, vocab: int):
    """name -> automaton, as the fixture's generator built them."""
    u = ByteAutomaton.utf8(vocab)
    return {"utf8": u, "utf8_ban": u & ByteAutomaton.ban([bytes(b) for b in meta["banned"]], vocab)}


def generated(row, start: int = 1):
    """The tokens of a returned row from column ``start`` on, through its EOS (the padding after it dropped)."""
    toks = [int(t) for t in row[start:]]
    return toks[: toks.index(EOS) + 1] if EOS in toks else toks


def obeys(aut: ByteAutomaton, row) -> bool:
    """The guarantee: every prefix of the row (start token dropped) is viable, and a row that ends with EOS is accepted."""
    toks = generated(row)
    return aut.accepts_row(toks) if toks and toks[-1] == EOS else aut.viable(toks)


def tokens_of(data: bytes, offset: int = 3):
    return [b + offset for b in data]
