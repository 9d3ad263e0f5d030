"""Memory hygiene of the C ABI's hot entry points on the MI355X (tests/hip_helpers.py: Arena, hygiene_findings; the
harness itself is tested in tests/test_hygiene_harness_cpu.py).  Every call goes through ctypes with its workspace, its
outputs and its inputs each inside a guarded arena; the workspace is exactly ``*_workspace_bytes()`` long and is filled
with 0x00, 0xFF and 0x7F bytes before the call.  Asserted for every case: RP_OK, every output the same bits under all
fills and under both fills of the bytes behind the inputs, every guard intact, ``workspace_bytes - 1`` refused with
RP_E_WORKSPACE and nothing written.  No tolerance anywhere: bit equality and guard integrity only."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hip_helpers import Arena, guard_bytes, hygiene_findings, quantize_e4m3  # noqa: E402
from seq2seq_grad_helpers import padded_labels  # noqa: E402
from reprover_amd import _lib, synth  # noqa: E402
from reprover_amd.decoder import HipT5Decoder, shift_and_segment  # noqa: E402
from reprover_amd.encoder import HipT5Encoder  # noqa: E402
from reprover_amd.train import HipT5Trainer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0  # what a flat gradient buffer holds before the call: the padding gaps keep it


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pc(a):
    return a.ctypes.data_as(C.c_void_p)


def _out(name, shape, dtype, guard, **kw):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return Arena(name, n, guard, DEV, dtype=dtype, **kw)


def _clean(call, workspace, outputs, inputs=(), **kw):
    """hygiene_findings must come back empty; returns the outputs of the zero-filled run by name"""
    results = {}
    with torch.cuda.device(DEV):
        found = hygiene_findings(call, workspace, outputs, inputs, results=results, **kw)
    assert not found, "\n".join(found)
    return results


def _stream():
    return _lib.current_stream()


def _ids(rng, lens):
    """packed ByT5 ids (byte + 3, EOS last) and cu_seqlens of sequences of the given lengths"""
    ids = np.concatenate([np.concatenate([rng.integers(3, 259, n - 1), [1]]) for n in lens]).astype(np.int32)
    return ids, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ---- encoder ---------------------------------------------------------------------------------------------------------------
def _enc_cfg(name):
    return dict(synth.t5_config("byt5-small"), num_layers=1) if name == "byt5-width" else synth.t5_config(name)


@functools.lru_cache(maxsize=None)
def _encoder(name):
    cfg = _enc_cfg(name)
    return cfg, HipT5Encoder(cfg, synth.synth_state_dict(cfg), DEV, keep_master_weights=False)


@pytest.mark.parametrize("lens", [(1,), (127, 1, 2), (129, 64, 7)], ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("name", ["tiny", "byt5-width"])
def test_encode_varlen_and_hidden(name, lens):
    """rp_encode_varlen (f32 and bf16 out) and rp_encode_hidden; 127 + 1 + 2 = 130 tokens pad to 256 rows"""
    cfg, enc = _encoder(name)
    lib, g, D = enc._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"]
    ids, cu = _ids(np.random.default_rng(len(lens)), lens)
    batch, T, max_len = len(lens), int(cu[-1]), max(lens)
    a_ids, a_cu = Arena.of("ids", _t(ids), g), Arena.of("cu_seqlens", _t(cu), g)
    ws = Arena("workspace", lib.rp_encoder_workspace_bytes(enc._handle, T, batch), g, DEV)
    for dt, tdt in ((_lib.RP_DT_F32, torch.float32), (_lib.RP_DT_BF16, torch.bfloat16)):
        out = _out("out", (batch, D), tdt, g)
        res = _clean(lambda n: lib.rp_encode_varlen(enc._handle, a_ids.ptr, a_cu.ptr, batch, T, max_len, out.ptr, dt, ws.ptr,
                                                    n, _stream()), ws, [out], [a_ids, a_cu])
        rows = res["out"].float().view(batch, D)
        assert torch.isfinite(rows).all() and bool(rows.any(dim=1).all())  # the call wrote every row
    hid = _out("hidden", (T, D), torch.bfloat16, g)
    res = _clean(lambda n: lib.rp_encode_hidden(enc._handle, a_ids.ptr, a_cu.ptr, batch, T, max_len, hid.ptr, ws.ptr, n,
                                                _stream()), ws, [hid], [a_ids, a_cu])
    assert torch.isfinite(res["hidden"].float()).all()


@pytest.mark.parametrize("lens", [(1, 129, 70), (1,)], ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("name", ["tiny", "byt5-width"])
def test_encode_padded(name, lens):
    """batch x 140 upper-bound rows of which 200 (or 1) are real: the pass is launched for batch * 140 tokens; the result is
    rp_encode_varlen's bits on the packed form (the documented contract)"""
    cfg, enc = _encoder(name)
    lib, g, D, L = enc._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"], 140
    ids, cu = _ids(np.random.default_rng(7), lens)
    batch, T = len(lens), int(cu[-1])
    pid, mask = np.zeros((batch, L), np.int64), np.zeros((batch, L), np.int64)
    for b, n in enumerate(lens):
        pid[b, :n] = ids[cu[b] : cu[b + 1]]
        mask[b, :n] = 1
    a_pid, a_mask = Arena.of("input_ids", _t(pid), g), Arena.of("attention_mask", _t(mask), g)
    ws = Arena("workspace", lib.rp_encode_padded_workspace_bytes(enc._handle, batch, L), g, DEV)
    out, meta = _out("out", (batch, D), torch.float32, g), _out("meta", (4,), torch.int32, g)
    res = _clean(lambda n: lib.rp_encode_padded(enc._handle, a_pid.ptr, a_mask.ptr, batch, L, out.ptr, _lib.RP_DT_F32,
                                                meta.ptr, ws.ptr, n, _stream()), ws, [out, meta], [a_pid, a_mask])
    assert res["meta"].tolist() == [T, max(lens), 0, 0]
    want = torch.empty((batch, D), dtype=torch.float32, device=DEV)
    ws2 = torch.empty(lib.rp_encoder_workspace_bytes(enc._handle, T, batch), dtype=torch.uint8, device=DEV)
    d_ids, d_cu = _t(ids), _t(cu)
    with torch.cuda.device(DEV):
        _lib.check(lib.rp_encode_varlen(enc._handle, d_ids.data_ptr(), d_cu.data_ptr(), batch, T, max(lens), want.data_ptr(),
                                        _lib.RP_DT_F32, ws2.data_ptr(), ws2.numel(), _stream()), "rp_encode_varlen")
    torch.cuda.synchronize()
    assert torch.equal(res["out"].view(batch, D), want)


# ---- training step -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer(name):
    cfg = _enc_cfg(name)
    return cfg, HipT5Trainer(cfg, synth.synth_state_dict(cfg), DEV)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("name", ["tiny", "byt5-width"])
def test_train_forward_backward(name, dropout):
    """rp_train_forward + rp_train_backward as one sequence: the workspace is poisoned before the forward only (the
    backward needs the forward's activations); the gradient buffer starts as a sentinel, which its padding gaps keep"""
    cfg, tr = _trainer(name)
    lib, g, D = tr._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"]
    lens = (1, 129, 70)
    ids, cu = _ids(np.random.default_rng(11), lens)
    batch, T = len(lens), int(cu[-1])
    a_ids, a_cu = Arena.of("ids", _t(ids), g), Arena.of("cu_seqlens", _t(cu), g)
    d_emb = Arena.of("d_emb", _t(np.random.default_rng(12).standard_normal((batch, D)).astype(np.float32)), g)
    ws = Arena("workspace", lib.rp_train_workspace_bytes(tr._handle, T, batch), g, DEV)
    emb = _out("out_emb", (batch, D), torch.float32, g)
    total = int(tr.layout[-1][2])
    grads = Arena.of("grads", torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV), g)

    def call(n):
        _lib.check(lib.rp_trainer_set_dropout(tr._handle, dropout, 20241), "rp_trainer_set_dropout")
        st = lib.rp_train_forward(tr._handle, a_ids.ptr, a_cu.ptr, batch, T, emb.ptr, ws.ptr, n, _stream())
        if st:
            return st
        return lib.rp_train_backward(tr._handle, tr.params.data_ptr(), a_ids.ptr, a_cu.ptr, batch, T, d_emb.ptr, grads.ptr,
                                     ws.ptr, n, _stream())

    try:
        res = _clean(call, ws, [emb, grads], [a_ids, a_cu, d_emb])
    finally:
        lib.rp_trainer_set_dropout(tr._handle, 0.0, 0)
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for _, shape, off in tr.layout[:-1]:
        live[int(off) : int(off) + int(np.prod(shape))] = True
    assert (res["grads"][~live] == SENTINEL).all(), "a padding gap was written"
    assert torch.isfinite(res["grads"][live]).all() and bool((res["grads"][live] != SENTINEL).any())


# ---- similarity scan ---------------------------------------------------------------------------------------------------------
SIM_CASES = [(1, 1, 64, 1), (5, 50, 64, 100), (3, 300, 64, 10),  # dense: one row; k > N; a partial third 128-row tile
             (3, 20037, 64, 100),                                 # two-pass, first-generation filter (<= 128 queries)
             (130, 20037, 64, 100)]                               # two-pass, second-generation filter (bf16 operands)


def _sim_operands(B, N, D, masked, seed):
    gen = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(B, D, generator=gen), dim=1).to(torch.bfloat16)
    E = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1).to(torch.bfloat16)
    F = min(7, N)
    masks, acc = synth.synth_masks(np.random.default_rng(seed), N, B, F) if masked else (None, np.ones((B, N), bool))
    return Q.to(DEV), E.to(DEV), masks, F, acc


def _sim_call(lib, form, ops, B, N, D, k, F, after, outs, ws):
    """the ctypes call of one of the four entry points on arena pointers"""
    p = lambda a: a.ptr if a is not None else None  # noqa: E731
    m = [p(ops.get(x)) for x in ("file_of", "end_key", "file_bits_t")] + [F if "file_of" in ops else 0] + \
        [p(ops.get(x)) for x in ("own_file", "q_key")]
    head = [p(ops["Q8"]), p(ops["q_scale"]), p(ops["E8"]), p(ops["e_scale"])] if "fp8" in form else [p(ops["Q"]), p(ops["E"])]
    aft = [p(after[0]), p(after[1])] if after else []
    fn = getattr(lib, {"bf16": "rp_sim_topk", "bf16_after": "rp_sim_topk_after", "fp8": "rp_sim_topk_fp8",
                       "fp8_after": "rp_sim_topk_fp8_after"}[form])
    return lambda n: fn(*head, B, N, D, *m, 1000, *aft, k, 0, outs[0].ptr, outs[1].ptr, outs[2].ptr, ws.ptr, n, _stream())


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("case", SIM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sim_topk_all_forms(case, masked):
    """rp_sim_topk, rp_sim_topk_fp8 and both _after forms (the second page: after the middle entry of the first)"""
    B, N, D, k = case
    lib, g = _lib.load(), guard_bytes()
    Q, E, masks, F, acc = _sim_operands(B, N, D, masked, seed=B + N)
    Q8, qs = quantize_e4m3(Q)
    E8, es = quantize_e4m3(E)
    ops = {n: Arena.of(n, t, g) for n, t in (("Q", Q), ("E", E), ("Q8", Q8), ("q_scale", qs), ("E8", E8), ("e_scale", es))}
    if masked:
        f, ek, bt, own, qk = masks
        for n, a in (("file_of", f), ("end_key", ek), ("file_bits_t", bt.view(np.int32)), ("own_file", own), ("q_key", qk)):
            ops[n] = Arena.of(n, _t(a), g)
    nbytes = lib.rp_sim_topk_workspace_bytes(B, N, D, k, 0)
    if N > 16384:
        assert nbytes != lib.rp_sim_topk_workspace_bytes(B, N, D, k, _lib.RP_TOPK_DENSE), "the case must take the two-pass plan"
    ws = Arena("workspace", nbytes, g, DEV)
    outs = [_out("out_scores", (B, k), torch.float32, g), _out("out_ids", (B, k), torch.int32, g),
            _out("out_count", (B,), torch.int32, g)]
    n_acc = torch.from_numpy(acc.sum(1))
    mask_arenas = [ops[n] for n in ("file_of", "end_key", "file_bits_t", "own_file", "q_key") if n in ops]
    for kind in ("bf16", "fp8"):
        used = [ops[n] for n in (("Q", "E") if kind == "bf16" else ("Q8", "q_scale", "E8", "e_scale"))] + mask_arenas
        res = _clean(_sim_call(lib, kind, ops, B, N, D, k, F, None, outs, ws), ws, outs, used)
        cnt = res["out_count"].cpu()
        assert torch.equal(cnt.long(), torch.clamp(n_acc, max=k)), "count = min(k, accessible rows)"
        sc, ids = res["out_scores"].view(B, k), res["out_ids"].view(B, k)
        mid = torch.clamp(cnt.long() // 2, min=0).to(DEV)
        rows = torch.arange(B, device=DEV)
        a_sc = Arena.of("after_score", sc[rows, mid].contiguous(), g)
        a_id = Arena.of("after_id", ids[rows, mid].contiguous(), g)  # (-1 where the first page is empty: no bound)
        res2 = _clean(_sim_call(lib, kind + "_after", ops, B, N, D, k, F, (a_sc, a_id), outs, ws), ws, outs,
                      used + [a_sc, a_id])
        # the pages concatenate: the second page opens with the first page's entries behind the bound
        sc2, ids2, cnt2 = res2["out_scores"].view(B, k), res2["out_ids"].view(B, k), res2["out_count"].cpu()
        for j in range(min(B, 8)):
            c, m_ = int(cnt[j]), int(mid[j])
            if c == 0:
                continue
            tail = c - m_ - 1
            assert int(cnt2[j]) == min(k, int(n_acc[j]) - m_ - 1)
            assert torch.equal(ids2[j, :tail], ids[j, m_ + 1 : c]) and torch.equal(sc2[j, :tail], sc[j, m_ + 1 : c])


def test_sim_topk_candidate_overflow():
    """the two-pass plan with its candidate list forced to k + 1 entries (option scan_cap, as
    test_candidate_overflow_contract_through_the_product does): every query reports out_count = -1, under every fill;
    scores and ids of an overflowed query are outside the contract (guarded, not compared)"""
    B, N, D, k = 3, 20037, 64, 100
    lib, g = _lib.load(), guard_bytes()
    Q, E, _, F, _ = _sim_operands(B, N, D, False, seed=5)
    ops = {"Q": Arena.of("Q", Q, g), "E": Arena.of("E", E, g)}
    _lib.check(lib.rp_set_option(b"scan_cap", 1), "scan_cap")
    try:
        ws = Arena("workspace", lib.rp_sim_topk_workspace_bytes(B, N, D, k, 0), g, DEV)
        outs = [_out("out_scores", (B, k), torch.float32, g, compare=False), _out("out_ids", (B, k), torch.int32, g, compare=False),
                _out("out_count", (B,), torch.int32, g)]
        res = _clean(_sim_call(lib, "bf16", ops, B, N, D, k, F, None, outs, ws), ws, outs, list(ops.values()))
    finally:
        _lib.check(lib.rp_set_option(b"scan_cap", 0), "scan_cap")
    assert res["out_count"].tolist() == [-1] * B


def _merge_inputs(R, B, k, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, k, size=(R, B)).astype(np.int32)  # every count < k
    scores = -np.sort(-rng.standard_normal((R, B, k)).astype(np.float32), axis=2)
    ids = rng.permutation(R * B * k).astype(np.int32).reshape(R, B, k)
    return scores, ids, counts


def test_topk_merge_and_strided():
    R, B, k = 3, 5, 7
    lib, g = _lib.load(), guard_bytes()
    scores, ids, counts = _merge_inputs(R, B, k, 3)
    ws = Arena("workspace", lib.rp_topk_merge_workspace_bytes(R, B, k), g, DEV)
    outs = [_out("out_scores", (B, k), torch.float32, g), _out("out_ids", (B, k), torch.int32, g),
            _out("out_count", (B,), torch.int32, g)]
    a_s, a_i, a_c = Arena.of("scores", _t(scores), g), Arena.of("ids", _t(ids), g), Arena.of("counts", _t(counts), g)
    res = _clean(lambda n: lib.rp_topk_merge(a_s.ptr, a_i.ptr, a_c.ptr, R, B, k, outs[0].ptr, outs[1].ptr, outs[2].ptr, ws.ptr,
                                             n, _stream()), ws, outs, [a_s, a_i, a_c])
    assert torch.equal(res["out_count"].cpu().long(), torch.from_numpy(np.minimum(counts.sum(0), k)).long())
    # the same lists as an all-gather's receive buffer: per rank [scores | ids | counts], this rank's queries last
    Bt, q0 = B + 4, 4
    packed = np.zeros((R, Bt * (2 * k + 1)), np.int32)
    for r in range(R):
        blk = packed[r]
        blk[: Bt * k].reshape(Bt, k)[q0:] = scores[r].view(np.int32)
        blk[Bt * k : 2 * Bt * k].reshape(Bt, k)[q0:] = ids[r]
        blk[2 * Bt * k :][q0:] = counts[r]
    a_p = Arena.of("recv_blocks", _t(packed), g)
    res2 = _clean(lambda n: lib.rp_topk_merge_strided(a_p.ptr + 4 * q0 * k, a_p.ptr + 4 * (Bt * k + q0 * k),
                                                      a_p.ptr + 4 * (2 * Bt * k + q0), Bt * (2 * k + 1), R, B, k, outs[0].ptr,
                                                      outs[1].ptr, outs[2].ptr, ws.ptr, n, _stream()), ws, outs, [a_p])
    for n in ("out_scores", "out_ids", "out_count"):
        assert torch.equal(res2[n], res[n]), n


def test_build_file_bits_and_quantize_rows():
    lib = _lib.load()
    g = guard_bytes()
    F, B = 70, 33
    rng = np.random.default_rng(9)
    reach = rng.integers(0, 1 << 62, size=(F, 2)).astype(np.int64)
    own = rng.integers(0, F, size=B).astype(np.int32)
    a_r, a_o = Arena.of("reach", _t(reach), g), Arena.of("own_file", _t(own), g)
    bits = _out("file_bits_t", (F, 2), torch.int32, g)
    res = _clean(lambda n: lib.rp_build_file_bits(a_r.ptr, F, a_o.ptr, B, bits.ptr, _stream()), None, [bits], [a_r, a_o])
    want = np.zeros((F, 2), np.uint32)
    for q in range(B):
        for f in range(F):
            want[f, q >> 5] |= np.uint32(((int(reach[own[q], f >> 6]) >> (f & 63)) & 1) << (q & 31))
    assert np.array_equal(res["file_bits_t"].cpu().numpy().view(np.uint32).reshape(F, 2), want)
    g = guard_bytes(3584)
    X = torch.randn(3, 1472, generator=torch.Generator().manual_seed(1))
    for x, dt in ((X, _lib.RP_DT_F32), (X.to(torch.bfloat16), _lib.RP_DT_BF16)):
        a_x = Arena.of("X", x.to(DEV), g)
        codes, scale = _out("out_fp8", (3, 1472), torch.uint8, g), _out("out_scale", (3,), torch.float32, g)
        res = _clean(lambda n: lib.rp_quantize_rows_e4m3(a_x.ptr, dt, 3, 1472, codes.ptr, scale.ptr, _stream()), None,
                     [codes, scale], [a_x])
        assert torch.equal(res["out_scale"].cpu(), x.float().abs().amax(dim=1) / 448.0)


# ---- decoder -------------------------------------------------------------------------------------------------------------------
def _dec_cfg(name):
    if name == "byt5-width":
        return dict(synth.seq2seq_config("byt5-small"), num_decoder_layers=1)
    return synth.seq2seq_config(name)


@functools.lru_cache(maxsize=None)
def _decoder(name):
    cfg = _dec_cfg(name)
    return cfg, HipT5Decoder(cfg, synth.synth_seq2seq_state_dict(cfg, scale="sharp"), DEV)


def _enc_rows(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return _t(rng.standard_normal((n, cfg["d_model"])).astype(np.float32) * 0.5).to(torch.bfloat16)


@pytest.mark.parametrize("shape", [(2, 3, (1, 129)), (1, 64, (5,))], ids=["2-states-3-beams", "1-state-64-beams"])
@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_decode_steps_and_beam_select(name, shape):
    """rp_decoder_batch_cross_kv, three rp_decoder_batch_step (every state, every state, the last state alone) and
    rp_beam_select_batch on the last step's rows, as one sequence on one workspace poisoned before the cross K/V only:
    the KV cache rows that no step has written (positions 3 .. 7, and state 0's position 2) hold the fill and must not
    reach any log-prob"""
    n, nb, src = shape
    cfg, dec = _decoder(name)
    lib, g, V, max_len = dec._lib, guard_bytes(cfg["d_ff"]), cfg["vocab_size"], 8
    src_cu = np.concatenate([[0], np.cumsum(src)]).astype(np.int32)
    enc = Arena.of("enc_bf16", _enc_rows(cfg, int(src_cu[-1]), 3), g)
    ws = Arena("workspace", lib.rp_decoder_batch_workspace_bytes(dec._handle, _pc(src_cu), n, nb, max_len), g, DEV)
    actives = [np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.array([n - 1], dtype=np.int32)]
    rng = np.random.default_rng(4)
    steps, lps, ins = [], [], [enc]
    for t, act in enumerate(actives):
        rows = len(act) * nb
        anc = np.zeros((rows, t + 1), np.int32)
        for r in range(rows):
            b = r % nb
            anc[r, :t] = np.arange(t) * nb + (b + 1) % nb  # the history of the neighbouring beam, rows written at p < t
            anc[r, t] = t * nb + b
        a_tok = Arena.of(f"tokens{t}", _t(rng.integers(0, 259, rows).astype(np.int32)), g)
        a_anc = Arena.of(f"ancestry{t}", _t(anc), g)
        lps.append(_out(f"logprobs{t}", (rows, V), torch.float32, g))
        steps.append((act, a_tok, a_anc))
        ins += [a_tok, a_anc]
    k = min(2 * nb, 128)
    running = Arena.of("running", _t(rng.standard_normal(nb).astype(np.float32)), g)
    sel_ws = Arena("select workspace", nb * min(k, V) * 8, g, DEV)
    sel = [_out("scores", (1, k), torch.float32, g), _out("tokens", (1, k), torch.int32, g),
           _out("parents", (1, k), torch.int32, g)]

    def call(nbytes):
        st = lib.rp_decoder_batch_cross_kv(dec._handle, enc.ptr, _pc(src_cu), n, nb, max_len, ws.ptr, nbytes, _stream())
        for t, (act, a_tok, a_anc) in enumerate(steps):
            if st:
                return st
            st = lib.rp_decoder_batch_step(dec._handle, _pc(src_cu), n, _pc(act), len(act), a_tok.ptr, a_anc.ptr, t + 1, nb,
                                           t, max_len, lps[t].ptr, ws.ptr, nbytes, _stream())
        if st:
            return st
        return lib.rp_beam_select_batch(lps[-1].ptr, running.ptr, 1, nb, V, k, sel[0].ptr, sel[1].ptr, sel[2].ptr,
                                        sel_ws.ptr, sel_ws.nbytes, _stream())

    res = _clean(call, [ws, sel_ws], lps + sel, ins + [running])
    for t in range(3):
        lp = res[f"logprobs{t}"].view(-1, V)
        assert torch.isfinite(lp).all() and bool((lp <= 0).all())  # log-softmax rows, not the fill
    assert bool((res["parents"] >= 0).all()) and bool((res["parents"] < nb).all())
    # rp_beam_select_batch's own workspace: one byte short is refused, nothing written
    found = hygiene_findings(lambda nbytes: lib.rp_beam_select_batch(lps[-1].ptr, running.ptr, 1, nb, V, k, sel[0].ptr,
                                                                     sel[1].ptr, sel[2].ptr, sel_ws.ptr, nbytes, _stream()),
                             sel_ws, sel, [running])
    assert not found, "\n".join(found)


def test_sample_step():
    """n = 2 states of 3 samples, V = 384, row (1, 2) already finished: every book is guarded in front and behind"""
    lib, g = _lib.load(), guard_bytes()
    n, nb, V, max_len, t = 2, 3, 384, 8, 2
    gen = torch.Generator().manual_seed(2)
    lp = Arena.of("logprobs", torch.log_softmax(torch.randn(n * nb, V, generator=gen) * 3, dim=1).to(DEV), g)
    seeds = Arena.of("seeds", _t(np.array([17, 0x7FFFFFF1], np.int32)), g)
    seq0 = np.zeros((n, nb, max_len), np.int32)
    seq0[:, :, 1 : t + 1] = 65
    fin0 = np.zeros((n, nb), np.int32)
    fin0[1, 2] = 1
    seq, tok = Arena.of("seq", _t(seq0), g), _out("tokens_next", (n * nb,), torch.int32, g)
    cum = Arena.of("cum_logprob", _t(np.full((n, nb), -1.5, np.float32)), g)
    ngen = Arena.of("n_generated", _t(np.full((n, nb), t, np.int32)), g)
    fin = Arena.of("finished", _t(fin0), g)
    active = np.array([1, 0], np.int32)
    res = _clean(lambda _: lib.rp_sample_step(lp.ptr, V, _pc(active), 2, n, nb, seeds.ptr, t, max_len, 0.8, 50, 0.9, 1, 0,
                                              seq.ptr, tok.ptr, cum.ptr, ngen.ptr, fin.ptr, _stream()), None,
                 [seq, tok, cum, ngen, fin], [lp, seeds])
    ng, sq = res["n_generated"].view(n, nb).cpu(), res["seq"].view(n, nb, max_len).cpu()
    want_ng = np.full((n, nb), t + 1)
    want_ng[1, 2] = t
    assert np.array_equal(ng.numpy(), want_ng) and int(sq[1, 2, t + 1]) == 0 and float(res["cum_logprob"].view(n, nb)[1, 2]) == -1.5
    assert np.array_equal(sq[:, :, : t + 1].numpy(), seq0[:, :, : t + 1]) and not sq[:, :, t + 2 :].any()
    assert res["tokens_next"].cpu().tolist() == [int(sq[s, b, t + 1]) for s in active for b in range(nb)]


SRC, TGT = (1, 70, 129), (1, 129, 0)  # 200 source rows (Sp = 256), 130 target rows (Tp = 256); the last pair is empty


def _pairs(cfg):
    rng = np.random.default_rng(25)
    y = padded_labels([np.concatenate([rng.integers(3, 259, max(n - 1, 0)), [1]])[:n].astype(np.int64) for n in TGT])
    tokens, labels, tgt_cu = shift_and_segment(y)
    src_cu = np.concatenate([[0], np.cumsum(SRC)]).astype(np.int32)
    return (_enc_rows(cfg, sum(SRC), 26), src_cu, np.ascontiguousarray(tokens, dtype=np.int32),
            np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(tgt_cu, dtype=np.int32))


@pytest.mark.parametrize("rows", [False, True], ids=["loss", "rows"])
@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_decoder_forward(name, rows):
    cfg, dec = _decoder(name)
    lib, g, V = dec._lib, guard_bytes(cfg["d_ff"]), cfg["vocab_size"]
    enc, src_cu, tokens, labels, tgt_cu = _pairs(cfg)
    B, T = len(TGT), int(tgt_cu[-1])
    assert T == sum(TGT) == 130
    a_enc, a_tok, a_lab = Arena.of("enc_bf16", enc, g), Arena.of("tokens", _t(tokens), g), Arena.of("labels", _t(labels), g)
    ws = Arena("workspace", lib.rp_decoder_forward_workspace_bytes(dec._handle, _pc(src_cu), _pc(tgt_cu), B), g, DEV)
    lp, sc = _out("label_logprobs", (T,), torch.float32, g), _out("loss_sum_count", (2,), torch.float64, g)
    lr = _out("logprob_rows", (T, V), torch.float32, g) if rows else None
    res = _clean(lambda n: lib.rp_decoder_forward(dec._handle, a_enc.ptr, _pc(src_cu), a_tok.ptr, a_lab.ptr, _pc(tgt_cu), B,
                                                  lp.ptr, sc.ptr, lr.ptr if rows else None, ws.ptr, n, _stream()), ws,
                 [lp, sc] + ([lr] if rows else []), [a_enc, a_tok, a_lab])
    s, c = res["loss_sum_count"].tolist()
    assert c == T and np.isfinite(s) and s > 0
    if rows:
        r = res["logprob_rows"].view(T, V)
        assert torch.equal(r[torch.arange(T, device=DEV), _t(labels).long()], res["label_logprobs"])


@pytest.mark.parametrize("want_d_enc", [True, False], ids=["d_enc", "no-d_enc"])
@pytest.mark.parametrize("name", ["tiny", "tiny-tied", "byt5-width"])
def test_decoder_loss_grad(name, want_d_enc):
    cfg, dec = _decoder(name)
    lib, g, D = dec._lib, guard_bytes(cfg["d_ff"]), cfg["d_model"]
    enc, src_cu, tokens, labels, tgt_cu = _pairs(cfg)
    B, T, S = len(TGT), int(tgt_cu[-1]), int(src_cu[-1])
    a_enc, a_tok, a_lab = Arena.of("enc_bf16", enc, g), Arena.of("tokens", _t(tokens), g), Arena.of("labels", _t(labels), g)
    ws = Arena("workspace", lib.rp_decoder_loss_grad_workspace_bytes(dec._handle, _pc(src_cu), _pc(tgt_cu), B), g, DEV)
    lp, sc = _out("label_logprobs", (T,), torch.float32, g), _out("loss_sum_count", (2,), torch.float64, g)
    names, off = dec.grad_layout()
    shapes = dec.grad_shapes()
    grads = Arena.of("grads", torch.full((int(off[-1]),), SENTINEL, dtype=torch.float32, device=DEV), g)
    d_enc = _out("d_enc", (S, D), torch.float32, g) if want_d_enc else None
    res = _clean(lambda n: lib.rp_decoder_loss_grad(dec._handle, a_enc.ptr, _pc(src_cu), a_tok.ptr, a_lab.ptr, _pc(tgt_cu), B,
                                                    lp.ptr, sc.ptr, grads.ptr, d_enc.ptr if want_d_enc else None, ws.ptr, n,
                                                    _stream()), ws, [lp, sc, grads] + ([d_enc] if want_d_enc else []),
                 [a_enc, a_tok, a_lab])
    live = torch.zeros(int(off[-1]), dtype=torch.bool, device=DEV)
    for i, nm in enumerate(names):
        live[int(off[i]) : int(off[i]) + int(np.prod(shapes[nm]))] = True
    assert (res["grads"][~live] == SENTINEL).all(), "a padding gap was written"
    assert torch.isfinite(res["grads"][live]).all() and bool((res["grads"][live] != SENTINEL).any())
    assert res["loss_sum_count"].tolist()[1] == T
    if want_d_enc:
        de = res["d_enc"].view(S, D)
        assert torch.isfinite(de).all() and bool(de[: src_cu[2]].any()) and not de[src_cu[2] :].any()  # the empty pair's source: 0
