"""Beam search with its books on the MI355X (rp_beam_books_init / rp_beam_advance, generate_many(sync_every=...)): the
kernel alone against its host restatement on scripted triples, bit for bit over the whole block; its refusals; whole
searches against the host-books loop; the loop's device-to-host copies counted."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_helpers import source_ids  # noqa: E402
from hip_helpers import Arena  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.common import Pos  # noqa: E402
from reprover_amd.decoder import HipT5Generator  # noqa: E402
from reprover_amd.generation import (BeamBooks, beam_advance_host, beam_books_bytes, beam_books_init_host,  # noqa: E402
                                     beam_search_batch_device)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS, START = 1, 0
GUARD = 1 << 20
C = _lib.C


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _act(*v):
    return np.array(v, dtype=np.int32)


# ---- the kernel alone ------------------------------------------------------------------------------------------------------
def _script(nb, ml, seed):
    """Per position t < ml - 1: (active list, {state: (scores, tokens, parents) of 2 nb candidates}) for three states.
    State 0 stops by the heuristic after position min(2, ml - 2): its first nb candidates are EOS and the rest score far
    below them.  State 1 runs to max_len: EOS among its first nb candidates at position 1 (nb > 1: the others go on),
    only among the second nb at position 2, exact ties (the two best, the two worst, signed zeros) from position 3 on.
    State 2 stops at its first step.  The active lists are permuted, shrink, and keep feeding stopped states."""
    g = torch.Generator().manual_seed(seed)
    K = 2 * nb
    lists = [[0, 1, 2], [2, 0, 1], [1, 0], [2, 1], [1], [0, 1]]
    steps = []
    for t in range(ml - 1):
        active = lists[t] if t < len(lists) else ([1, 2] if t % 5 == 0 else [1])
        triples = {}
        for s in active:
            vals = torch.sort(-30.0 * torch.rand(K, generator=g), descending=True)[0]
            toks = torch.randint(2, 20, (K,), generator=g, dtype=torch.int32)
            pars = torch.randint(0, nb, (K,), generator=g, dtype=torch.int32)
            if (s == 0 and t == min(2, ml - 2)) or (s == 2 and t == 0):
                toks[:nb] = EOS
                vals[nb:] -= 50.0
            if s == 1 and t == 1 and nb > 1:
                toks[0] = EOS
            if s == 1 and t == 2:
                toks[nb] = EOS
            if s == 1 and t >= 3 and t % 2 == 1:
                vals[1 % K] = vals[0]
                vals[K - 1] = vals[K - 2]
            if s == 1 and t == 4:
                vals[0], vals[1 % K] = -0.0, 0.0
            triples[s] = (vals, toks, pars)
        steps.append((active, triples))
    return steps


def _divs(t, lp=1.0):
    return float((t + 1) ** lp), float((t + 1) ** lp)


def _run_kernel(lib, nb, ml, script, fill):
    """The script through rp_beam_books_init / rp_beam_advance on a block of exactly rp_beam_books_bytes between guards,
    the block poisoned with ``fill`` first; after init and after every advance the whole block equals the restatement's.
    Returns the final block (host)."""
    n = 3
    need = lib.rp_beam_books_bytes(n, nb, ml)
    assert need == beam_books_bytes(n, nb, ml) and need % 16 == 0
    arena = Arena("books", need, GUARD, DEV, init=fill)
    ref = beam_books_init_host(n, nb, ml, EOS, START)
    assert lib.rp_beam_books_init(arena.ptr, need - 1, n, nb, ml, EOS, START, None) == -1  # one byte less is refused
    assert b"books" in lib.rp_last_error() and arena.at_rest()
    _lib.check(lib.rp_beam_books_init(arena.ptr, need, n, nb, ml, EOS, START, None), "rp_beam_books_init")
    block = lambda: arena.view(dtype=torch.int32).cpu()  # noqa: E731
    assert torch.equal(block(), ref.block), "init"
    assert not arena.broken_guards()
    for t, (active, triples) in enumerate(script):
        sc = torch.stack([triples[s][0] for s in active])
        tk = torch.stack([triples[s][1] for s in active])
        pr = torch.stack([triples[s][2] for s in active])
        d_sc, d_tk, d_pr = sc.to(DEV).contiguous(), tk.to(DEV).contiguous(), pr.to(DEV).contiguous()
        args = (n, nb, ml, _p(_act(*active)), len(active), t, d_sc.data_ptr(), d_tk.data_ptr(), d_pr.data_ptr(),
                *_divs(t), EOS, None)
        if t == 1:
            before = block()
            assert lib.rp_beam_advance(arena.ptr, need - 1, *args) == -1 and b"books" in lib.rp_last_error()
            torch.cuda.synchronize()
            assert torch.equal(block(), before)
        _lib.check(lib.rp_beam_advance(arena.ptr, need, *args), "rp_beam_advance")
        beam_advance_host(ref, active, t, sc, tk, pr, *_divs(t), EOS)
        got = block()
        if not torch.equal(got, ref.block):
            view = BeamBooks(n, nb, ml, block=got)
            bad = [f for f in ("run_seq", "anc", "fin_seq", "run_scores", "beam_scores", "fin_flag", "fin_len", "heur",
                               "done", "steps", "tokens", "running", "anc_rows")
                   if not torch.equal(getattr(view, f).view(torch.int32) if getattr(view, f).dtype == torch.float32
                                      else getattr(view, f),
                                      getattr(ref, f).view(torch.int32) if getattr(ref, f).dtype == torch.float32
                                      else getattr(ref, f))]
            raise AssertionError(f"position {t}, active {active}: parts {bad} differ from the restatement")
    assert not arena.broken_guards()
    return block(), ref


@pytest.mark.parametrize("nb", [1, 2, 3, 64])
@pytest.mark.parametrize("ml", [2, 3, 40])
def test_kernel_alone_equals_the_restatement(nb, ml):
    lib = _lib.load()
    script = _script(nb, ml, seed=1000 * nb + ml)
    a, ref = _run_kernel(lib, nb, ml, script, 0x5A)
    b, _ = _run_kernel(lib, nb, ml, script, 0xFF)
    assert torch.equal(a, b)  # nothing depends on what the block held
    steps, heur, done = ref.steps.tolist(), ref.heur.tolist(), ref.done.tolist()
    print("steps", steps, "heur", heur, "done", done)
    assert done == [1, 1, 1]
    if ml == 40:  # the three kinds of stop: the heuristic at position 2, max_len, the first step
        assert steps == [3, 39, 1] and heur[0] == 0 and heur[2] == 0
    else:
        assert steps[1] == ml - 1 and steps[2] == 1


def test_refusals_leave_the_books_untouched():
    lib = _lib.load()
    n, nb, ml = 3, 4, 9
    need = lib.rp_beam_books_bytes(n, nb, ml)
    arena = Arena("books", need, GUARD, DEV, init=0x5A)
    _lib.check(lib.rp_beam_books_init(arena.ptr, need, n, nb, ml, EOS, START, None), "rp_beam_books_init")
    K = 2 * nb
    sc = torch.zeros((n, K), dtype=torch.float32, device=DEV)
    tk = torch.full((n, K), 5, dtype=torch.int32, device=DEV)
    pr = torch.zeros((n, K), dtype=torch.int32, device=DEV)
    d = (sc.data_ptr(), tk.data_ptr(), pr.data_ptr())
    torch.cuda.synchronize()
    before = arena.payload().clone()
    act = _act(0, 1, 2)
    err = lambda: lib.rp_last_error()  # noqa: E731
    adv = lambda books=arena.ptr, nbytes=need, n=n, nb=nb, ml=ml, a=act, na=3, t=0, ptrs=d: lib.rp_beam_advance(  # noqa: E731
        books, nbytes, n, nb, ml, None if a is None else _p(a), na, t, *ptrs, 1.0, 1.0, EOS, None)
    cases = [
        (adv(books=None), b"null"), (adv(a=None), b"null"), (adv(ptrs=(None, d[1], d[2])), b"null"),
        (adv(ptrs=(d[0], None, d[2])), b"null"), (adv(ptrs=(d[0], d[1], None)), b"null"),
        (adv(nb=0), b"nb=0"), (adv(nb=65), b"nb=65"), (adv(n=0), b"states=0"), (adv(n=33), b"states=33"),
        (adv(n=17, nb=64), b"rows"), (adv(a=_act(1, 1, 2)), b"twice"), (adv(a=_act(0, 3, 2)), b"active[1]=3"),
        (adv(a=_act(0, -1, 2)), b"active[1]=-1"), (adv(na=0), b"active states=0"), (adv(na=4), b"active states=4"),
        (adv(t=ml - 1), b"t=8"), (adv(t=-1), b"t=-1"), (adv(nbytes=need - 1), b"books"), (adv(ml=1), b"max_len=1"),
    ]
    for i, (st, _) in enumerate(cases):
        assert st == -1, i
    # (the messages are read one call at a time: rp_last_error keeps the latest)
    assert adv(a=_act(1, 1, 2)) == -1 and b"twice" in err()
    assert adv(t=ml - 1) == -1 and b"t=8" in err()
    assert adv(nbytes=need - 1) == -1 and b"books" in err()
    assert lib.rp_beam_books_bytes(0, nb, ml) == 0 and b"states=0" in err()
    assert lib.rp_beam_books_bytes(n, 65, ml) == 0 and b"nb=65" in err()
    assert lib.rp_beam_books_bytes(17, 64, ml) == 0 and b"rows" in err()
    assert lib.rp_beam_books_bytes(n, nb, 1) == 0 and b"max_len" in err()
    assert lib.rp_beam_books_bytes(16, 64, 512) > 0
    assert lib.rp_beam_books_init(None, need, n, nb, ml, EOS, START, None) == -1 and b"null" in err()
    assert lib.rp_beam_books_init(arena.ptr, need, n, 65, ml, EOS, START, None) == -1 and b"nb=65" in err()
    torch.cuda.synchronize()
    assert torch.equal(arena.payload(), before) and not arena.broken_guards()
    assert adv() == 0  # and the accepted call does change them
    torch.cuda.synchronize()
    assert not torch.equal(arena.payload(), before)


# ---- whole searches --------------------------------------------------------------------------------------------------------
def _g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_generate.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = synth.seq2seq_config("tiny")
    sd = synth.synth_seq2seq_state_dict(cfg)
    sd["lm_head.weight"] = sd["lm_head.weight"].clone()
    sd["lm_head.weight"][1] *= meta["eos_boost"]
    return z, cfg, sd


@pytest.fixture(scope="module")
def tiny_gen(golden_dir):
    z, cfg, sd = _g20(golden_dir)
    return z, cfg, sd, HipT5Generator(cfg, sd, DEV)


def _sources(src):
    """Eight distinct sources: the G20 source, truncations of it (EOS re-appended) and seeded ones of other lengths
    (tests/test_generate_batch_gpu.py's)."""
    cut = lambda n: np.concatenate([src[:n], [1]]).astype(np.int32)  # noqa: E731
    return [np.asarray(src, dtype=np.int32), cut(40), cut(7), source_ids(120, 11), source_ids(33, 12), source_ids(1, 0),
            source_ids(257, 13), cut(150)]


def _same_output(got, want):
    assert got.sequences.dtype == want.sequences.dtype and torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.sequences_scores.view(torch.int32), want.sequences_scores.view(torch.int32))  # bits


def _device_books_equal_host_books(gen, srcs, nb, lp, L, spread=False):
    traces = []
    want = gen.generate_many(srcs, nb, L, lp, traces=traces)
    stops = [len(t) for t in traces]
    print("stop steps:", stops)
    if spread:  # the states stop at different positions, one at least 3 before the last
        assert len(set(stops)) > 1 and min(stops) <= max(stops) - 3, stops
    for k in (1, 3, 16, L):
        outs = gen.generate_many(srcs, nb, L, lp, sync_every=k)
        assert len(outs) == len(srcs)
        for o, w in zip(outs, want):
            _same_output(o, w)
    # permuted (one state twice), one state alone, and generate's own argument
    perm = [5, 2, 7, 0, 2, 6, 1, 4, 3]
    for o, i in zip(gen.generate_many([srcs[i] for i in perm], nb, L, lp, sync_every=3), perm):
        _same_output(o, want[i])
    for i in (0, 2):
        _same_output(gen.generate_many([srcs[i]], nb, L, lp, sync_every=3)[0], want[i])
        _same_output(gen.generate(srcs[i], nb, L, lp, sync_every=16), gen.generate(srcs[i], nb, L, lp))
        _same_output(gen.generate(srcs[i], nb, L, lp, sync_every=1), want[i])


@pytest.mark.parametrize("nb", [1, 4, 64])
@pytest.mark.parametrize("lp", [0.0, 1.0])
@pytest.mark.parametrize("L", [2, 24])
def test_generate_many_with_device_books_equals_the_host_books(tiny_gen, nb, lp, L):
    z, cfg, sd, gen = tiny_gen
    _device_books_equal_host_books(gen, _sources(z["src"]), nb, lp, L)


def test_generate_many_with_device_books_when_states_stop_at_different_positions(tiny_gen):
    """max_length 64, 4 beams, length_penalty 0 (tests/test_generate_batch_gpu.py's early-exit shape): at 24 positions
    every state of these sources runs to max_length; here they stop by the heuristic at different positions, so states
    leave the active list at the syncs and the by-row inputs are regathered."""
    z, cfg, sd, gen = tiny_gen
    _device_books_equal_host_books(gen, _sources(z["src"]), 4, 0.0, 64, spread=True)


def test_sync_every_arguments(tiny_gen):
    z, cfg, sd, gen = tiny_gen
    src = np.asarray(z["src"], dtype=np.int32)
    with pytest.raises(ValueError, match="traces"):
        gen.generate_many([src], 4, 8, 1.0, traces=[], sync_every=2)
    with pytest.raises(ValueError, match="trace"):
        gen.generate(src, 4, 8, 1.0, trace=[], sync_every=2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sync_every"):
            gen.generate_many([src], 4, 8, 1.0, sync_every=bad)
    with pytest.raises(ValueError):
        gen.generate_many([src], 4, 1, 1.0, sync_every=2)


@pytest.mark.parametrize("k", [1, 4, 100])
def test_the_loop_makes_no_per_step_transfer(tiny_gen, k):
    """The test's own driver of ``beam_search_batch_device`` over the engine's three callables: every device-to-host copy
    of the loop goes through ``to_host`` and is counted; the three callables return device tensors and are handed device
    tensors (views of the books), and nothing else is uploaded."""
    z, cfg, sd, gen = tiny_gen
    dec = gen.decoder
    srcs = _sources(z["src"])
    nb, L, lp = 4, 24, 0.0
    want = gen.generate_many(srcs, nb, L, lp)
    n = gen._start_many(srcs, nb, L)
    calls = {"step": 0, "select": 0, "advance": 0}
    copies = []

    def on_device(*xs):
        assert all(x.is_cuda for x in xs)

    def step(active, tokens, ancestry, t):
        calls["step"] += 1
        on_device(tokens, ancestry)
        assert tokens.dtype == torch.int32 and ancestry.dtype == torch.int32 and ancestry.shape[1] == L
        out = dec.step_many(active, tokens, ancestry, t=t)
        on_device(out)
        return out

    def select(log_probs, running, nb_, k_):
        calls["select"] += 1
        on_device(log_probs, running)
        outs = dec.select_many(log_probs, running, nb_, k_)
        on_device(*outs)
        return outs

    def advance(books, active, t, *rest):
        calls["advance"] += 1
        on_device(books.block, *rest[:3])
        dec.beam_advance(books, active, t, *rest)

    def to_host(x):
        copies.append(x.numel())
        return x.cpu()

    outs = beam_search_batch_device(step, select, advance, n, nb, L, lp, EOS, START, sync_every=k, device=gen.device,
                                    init=dec.beam_books, to_host=to_host)
    for o, w in zip(outs, want):
        _same_output(o, w)
    steps = calls["step"]
    assert steps == calls["select"] == calls["advance"] and 1 <= steps <= L - 1
    print("positions", steps, "device-to-host copies", copies)
    assert len(copies) <= -(-steps // k) + 1
    assert copies[-1] == beam_books_bytes(n, nb, L) // 4 and all(c == n for c in copies[:-1])


# ---- product ---------------------------------------------------------------------------------------------------------------
def test_prover_generator_with_beam_sync_every(golden_dir):
    from reprover_amd.prover.tactic_generator import HuggingFaceGenerator

    z, cfg, sd = _g20(golden_dir)
    gdir = os.path.join(tempfile.mkdtemp(), "gen")
    os.makedirs(gdir)
    hf_cfg = dict(model_type="t5", architectures=["T5ForConditionalGeneration"], is_encoder_decoder=True,
                  decoder_start_token_id=0, eos_token_id=1, pad_token_id=0,
                  **{k: cfg[k] for k in ("vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                         "num_decoder_layers", "relative_attention_num_buckets",
                                         "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj",
                                         "tie_word_embeddings")})
    with open(os.path.join(gdir, "config.json"), "w") as fh:
        json.dump(hf_cfg, fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()
               if k not in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight")},
              os.path.join(gdir, "model.safetensors"))
    rng = np.random.default_rng(17)
    states = [synth.synth_state(rng, n) for n in (60, 400, 15, 900, 60)]
    n = len(states)
    paths, names, poses = ["f.lean"] * n, ["thm"] * n, [Pos(1, 0)] * n
    base = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0)
    base.initialize()
    dev = HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, beam_sync_every=4)
    dev.initialize()
    want = base.batch_generate_sync(states, paths, names, poses, 8)
    assert dev.batch_generate_sync(states, paths, names, poses, 8) == want  # strings and scores (exact floats)
    assert dev.generate_sync(states[1], "f.lean", "thm", Pos(1, 0), 8) == want[1]
    with pytest.raises(ValueError):
        HuggingFaceGenerator(gdir, DEV, 512, 32, 0.0, beam_sync_every=0)
