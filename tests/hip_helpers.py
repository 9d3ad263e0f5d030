"""Thin callers of the C ABI used by the GPU parity tests (raw pointers in, torch tensors as
containers) + comparison helpers."""
import ctypes

import numpy as np
import torch

from reprover_amd import _lib


def dev():
    return torch.device("cuda:0")


def split_planes(x):
    """fp32 [M, N] -> the residual stream's two bf16 planes [2, M, N]: hi = bf16(x), lo = bf16(x - hi)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def merge_planes(planes):
    return planes[0].float() + planes[1].float()


def split_x24(x):
    """fp32 [M, N] -> the inference pass's 24-bit form of the residual stream (rp_encoder_kernels.h, x24_update2): the
    fp32 word rounded to its top 24 bits (half away from zero), as (hi bf16 [M, N] = that word rounded to 16 bits, half
    away from zero; ext uint8 [M, N] = the signed remainder in units of 2^-8 ulp(hi) stored BIASED by 128 = bits 8..15 of
    (the rounded word + 0x8000): round 6).  Returned as ONE uint8 buffer [M * N * 3] laid out [hi plane | ext plane] (what
    RP_EPI_RESID8 takes) plus the two views."""
    bits = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    q = (bits + 0x8080) & 0xFFFFFFFF
    ext = ((q >> 8) & 0xFF).to(torch.uint8)
    hi16 = (q >> 16).to(torch.int32).to(torch.int16)  # (wraps like uint16)
    M, N = x.shape
    buf = torch.empty(M * N * 3, dtype=torch.uint8, device=x.device)
    buf[: M * N * 2].view(torch.int16).view(M, N).copy_(hi16)
    buf[M * N * 2 :].view(M, N).copy_(ext)
    return buf, buf[: M * N * 2].view(torch.bfloat16).view(M, N), buf[M * N * 2 :].view(M, N)


def merge_x24(hi, ext):
    """x = float(((hi << 16) | (ext << 8)) - 0x8000) as 32-bit words."""
    w = (hi.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF) << 16
    w = (w + (ext.to(torch.int64) << 8) - 0x8000) & 0xFFFFFFFF
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w.view(torch.float32)


def gemm(A, W, n_valid, epilogue, out):
    """``out``: the epilogue's output; for RP_EPI_RESID an fp32 [M, n_valid] matrix that is updated in place THROUGH
    the engine's two-plane form of the residual stream (split before the call, merged after it)."""
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    target = split_planes(out) if epilogue == _lib.RP_EPI_RESID else out
    _lib.check(lib.rp_dbg_gemm(_lib.ptr(A), _lib.ptr(W), _lib.ptr(target), M, N, K, n_valid, epilogue,
                               _lib.current_stream()), "rp_dbg_gemm")
    torch.cuda.synchronize()
    if epilogue == _lib.RP_EPI_RESID:
        out.copy_(merge_planes(target))
    return out


def rowscale(ssp, inv_d, eps=1e-6):
    """rs [rows] from slot-major partial sums of squares ssp [np, rows] (rowscale_kernel, as the encoder runs it)."""
    lib = _lib.load()
    np_, rows = ssp.shape
    rs = torch.empty(rows, dtype=torch.float32, device=ssp.device)
    _lib.check(lib.rp_dbg_rowscale(_lib.ptr(ssp), _lib.ptr(rs), rows, np_, inv_d, eps, _lib.current_stream()),
               "rp_dbg_rowscale")
    torch.cuda.synchronize()
    return rs


def attention(qkv, cu, tab, H):
    lib = _lib.load()
    T = qkv.shape[0]
    out = torch.zeros((T, H * 64), dtype=torch.bfloat16, device=qkv.device)
    lens = (cu[1:] - cu[:-1]).cpu()
    _lib.check(lib.rp_dbg_attention(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(tab), _lib.ptr(out), len(lens),
                                    int(lens.max()), H, T, _lib.current_stream()), "rp_dbg_attention")
    torch.cuda.synchronize()
    return out


def sim_topk(Q, E, k, masks=None, id_offset=0, flags=0, N=None, retry_dense=True):
    """masks = (file_of i32 [N], end_key i64 [N], bits_t u32-as-i32 [F, W], own i32 [B], qk i64 [B]) device tensors.
    With flags & RP_TOPK_E_BLOCKED, E is the flat blocked copy and N must be given."""
    lib = _lib.load()
    B, D = Q.shape
    N = E.shape[0] if N is None else N
    out_s = torch.empty((B, k), dtype=torch.float32, device=Q.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=Q.device)
    out_c = torch.empty((B,), dtype=torch.int32, device=Q.device)
    nbytes = lib.rp_sim_topk_workspace_bytes(B, N, D, k, flags)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q.device)
    if masks is None:
        f = ek = bt = own = qk = None
        F = 0
    else:
        f, ek, bt, own, qk = masks
        F = bt.shape[0]
    _lib.check(lib.rp_sim_topk(_lib.ptr(Q), _lib.ptr(E), B, N, D, _lib.ptr(f), _lib.ptr(ek), _lib.ptr(bt), F,
                               _lib.ptr(own), _lib.ptr(qk), id_offset, k, flags, _lib.ptr(out_s), _lib.ptr(out_i),
                               _lib.ptr(out_c), _lib.ptr(ws), nbytes, _lib.current_stream()), "rp_sim_topk")
    torch.cuda.synchronize()
    if retry_dense and bool((out_c < 0).any()):  # the ABI's overflow contract, as every product caller honours it
        return sim_topk(Q, E, k, masks, id_offset, flags | _lib.RP_TOPK_DENSE, N, retry_dense=False)
    return out_i, out_s, out_c


def sim_plan(B, N, D, k, flags=0, fp8=False, paged=False):
    """rp_dbg_sim_plan as a dict (no GPU call): the fields by name, tiles and stages by name (None: not launched)."""
    out = (ctypes.c_int64 * len(_lib.SIM_PLAN_FIELDS))()
    _lib.check(_lib.load().rp_dbg_sim_plan(B, N, D, k, flags, int(fp8), int(paged), out), "rp_dbg_sim_plan")
    p = dict(zip(_lib.SIM_PLAN_FIELDS, out))
    for f in ("tile0", "tile1"):
        p[f] = _lib.SIM_TILES[p[f]] if p[f] >= 0 else None
    for f in ("stage0", "stage1"):
        p[f] = _lib.SIM_STAGES[p[f]] if p[f] >= 0 else None
    return p


def sim_topk_after(Q, E, k, after_score, after_id, masks=None, id_offset=0, flags=0, scales=None):
    """rp_sim_topk_after, or rp_sim_topk_fp8_after with scales = (q_scale, e_scale): the page behind (after_score, after_id)."""
    lib = _lib.load()
    (B, D), N = Q.shape, E.shape[0]
    out_s = torch.empty((B, k), dtype=torch.float32, device=Q.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=Q.device)
    out_c = torch.empty((B,), dtype=torch.int32, device=Q.device)
    nbytes = lib.rp_sim_topk_workspace_bytes(B, N, D, k, flags)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q.device)
    f, ek, bt, own, qk = masks if masks is not None else (None,) * 5
    tail = [B, N, D, _lib.ptr(f), _lib.ptr(ek), _lib.ptr(bt), 0 if bt is None else bt.shape[0], _lib.ptr(own), _lib.ptr(qk),
            id_offset, _lib.ptr(after_score), _lib.ptr(after_id), k, flags, _lib.ptr(out_s), _lib.ptr(out_i), _lib.ptr(out_c),
            _lib.ptr(ws), nbytes, _lib.current_stream()]
    if scales is None:
        _lib.check(lib.rp_sim_topk_after(_lib.ptr(Q), _lib.ptr(E), *tail), "rp_sim_topk_after")
    else:
        _lib.check(lib.rp_sim_topk_fp8_after(_lib.ptr(Q), _lib.ptr(scales[0]), _lib.ptr(E), _lib.ptr(scales[1]), *tail),
                   "rp_sim_topk_fp8_after")
    torch.cuda.synchronize()
    return out_i, out_s, out_c


def quantize_e4m3(X):
    """(codes uint8 [R, D], scale f32 [R]) device tensors via rp_quantize_rows_e4m3."""
    lib = _lib.load()
    X = X.contiguous()
    R, D = X.shape
    codes = torch.empty((R, D), dtype=torch.uint8, device=X.device)
    scale = torch.empty((R,), dtype=torch.float32, device=X.device)
    dt = _lib.RP_DT_F32 if X.dtype == torch.float32 else _lib.RP_DT_BF16
    _lib.check(lib.rp_quantize_rows_e4m3(_lib.ptr(X), dt, R, D, _lib.ptr(codes), _lib.ptr(scale),
                                         _lib.current_stream()), "rp_quantize_rows_e4m3")
    torch.cuda.synchronize()
    return codes, scale


def sim_topk_fp8(Q8, qs, E8, es, k, masks=None, id_offset=0, flags=0, N=None, retry_dense=True):
    """rp_sim_topk_fp8 on e4m3 codes (uint8) + per-row scales; masks as in sim_topk."""
    lib = _lib.load()
    B, D = Q8.shape
    N = E8.shape[0] if N is None else N
    out_s = torch.empty((B, k), dtype=torch.float32, device=Q8.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=Q8.device)
    out_c = torch.empty((B,), dtype=torch.int32, device=Q8.device)
    nbytes = lib.rp_sim_topk_workspace_bytes(B, N, D, k, flags)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q8.device)
    if masks is None:
        f = ek = bt = own = qk = None
        F = 0
    else:
        f, ek, bt, own, qk = masks
        F = bt.shape[0]
    _lib.check(lib.rp_sim_topk_fp8(_lib.ptr(Q8), _lib.ptr(qs), _lib.ptr(E8), _lib.ptr(es), B, N, D, _lib.ptr(f),
                                   _lib.ptr(ek), _lib.ptr(bt), F, _lib.ptr(own), _lib.ptr(qk), id_offset, k, flags,
                                   _lib.ptr(out_s), _lib.ptr(out_i), _lib.ptr(out_c), _lib.ptr(ws), nbytes,
                                   _lib.current_stream()), "rp_sim_topk_fp8")
    torch.cuda.synchronize()
    if retry_dense and bool((out_c < 0).any()):
        return sim_topk_fp8(Q8, qs, E8, es, k, masks, id_offset, flags | _lib.RP_TOPK_DENSE, N, retry_dense=False)
    return out_i, out_s, out_c


def topk_merge(scores, ids, counts):
    lib = _lib.load()
    R, B, k = scores.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=scores.device)
    out_c = torch.empty((B,), dtype=torch.int32, device=scores.device)
    nbytes = lib.rp_topk_merge_workspace_bytes(R, B, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    _lib.check(lib.rp_topk_merge(_lib.ptr(scores), _lib.ptr(ids), _lib.ptr(counts), R, B, k, _lib.ptr(out_s),
                                 _lib.ptr(out_i), _lib.ptr(out_c), _lib.ptr(ws), nbytes, _lib.current_stream()),
               "rp_topk_merge")
    torch.cuda.synchronize()
    return out_i, out_s, out_c


def topk_merge_strided(packed, R, Bt, k, q0, B, rank_stride=None):
    """rp_topk_merge_strided over queries [q0, q0 + B) of ``packed``: a flat 4-byte-unit device buffer (int32) holding R
    blocks [scores f32 [Bt, k] | ids i32 [Bt, k] | counts i32 [Bt]], block r at r * rank_stride (default Bt * (2 k + 1))."""
    lib = _lib.load()
    rank_stride = Bt * (2 * k + 1) if rank_stride is None else rank_stride
    assert packed.dtype == torch.int32 and packed.numel() >= (R - 1) * rank_stride + Bt * (2 * k + 1)
    assert 0 <= q0 and q0 + B <= Bt
    out_s = torch.empty((B, k), dtype=torch.float32, device=packed.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=packed.device)
    out_c = torch.empty((B,), dtype=torch.int32, device=packed.device)
    nbytes = lib.rp_topk_merge_workspace_bytes(R, B, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    base = _lib.ptr(packed)
    _lib.check(lib.rp_topk_merge_strided(base + 4 * q0 * k, base + 4 * (Bt * k + q0 * k), base + 4 * (2 * Bt * k + q0),
                                         rank_stride, R, B, k, _lib.ptr(out_s), _lib.ptr(out_i), _lib.ptr(out_c),
                                         _lib.ptr(ws), nbytes, _lib.current_stream()), "rp_topk_merge_strided")
    torch.cuda.synchronize()
    return out_i, out_s, out_c


GUARD = 64  # floats behind every array handed to the optimizer-end kernels


def guarded(n, fill, guard_value, device="cuda", dtype=torch.float32):
    """(whole buffer [n + GUARD], view of its first n elements): the view is what a kernel is handed, the GUARD elements
    behind it hold ``guard_value`` and must come back untouched (guard_intact) / unread."""
    buf = torch.full((n + GUARD,), guard_value, dtype=dtype, device=device)
    buf[:n] = fill
    return buf, buf[:n]


def guard_intact(buf, n, guard_value):
    g = buf[n:]
    want = torch.full_like(g, guard_value)
    return bool(torch.equal(g.view(torch.int32), want.view(torch.int32)))  # bits: NaN guards compare too


def grad_norm(g, n=None, scratch=None, sync=True):
    """rp_grad_norm over the first n floats of g -> device f32 [1]."""
    lib = _lib.load()
    n = g.numel() if n is None else n
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=g.device)
    scratch = torch.empty(1024, dtype=torch.float32, device=g.device) if scratch is None else scratch
    _lib.check(lib.rp_grad_norm(_lib.ptr(g), n, _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream()), "rp_grad_norm")
    if sync:
        torch.cuda.synchronize()
    return out


def adamw_step(p, g, m, v, step, lr, betas, eps, wd, total_norm=None, max_norm=0.0, clipped=True, n=None):
    """rp_adamw_step_clipped (clipped=False: rp_adamw_step) in place; returns the status (no exception: the error tests
    read it).  Launch only, no synchronisation."""
    lib = _lib.load()
    n = p.numel() if n is None else n
    if clipped:
        return lib.rp_adamw_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, lr, betas[0],
                                         betas[1], eps, wd, _lib.ptr(total_norm), max_norm, _lib.current_stream())
    return lib.rp_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, lr, betas[0], betas[1], eps,
                             wd, _lib.current_stream())


def contrastive_mse_raw(C, P, label, want_sim=True, ws_bytes=None, D=None):
    """rp_contrastive_mse through the ABI -> (status, loss buffer, similarity buffer or None); both outputs are `guarded`
    with NaN (loss: [1 + GUARD], similarity: [B * Pn + GUARD])."""
    lib = _lib.load()
    B, Pn = C.shape[0], P.shape[0]
    D = C.shape[1] if D is None else D
    need = lib.rp_contrastive_mse_workspace_bytes(B, Pn)
    ws_bytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=C.device)
    loss, _ = guarded(1, float("nan"), float("nan"))
    sim = guarded(B * Pn, float("nan"), float("nan"))[0] if want_sim else None
    st = lib.rp_contrastive_mse(_lib.ptr(C), _lib.ptr(P), _lib.ptr(label), B, Pn, D, _lib.ptr(loss), _lib.ptr(sim),
                                _lib.ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return st, loss, sim


def contrastive_mse_backward_raw(C, P, S, label):
    """rp_contrastive_mse_backward -> (status, d_ctx buffer [B * D + GUARD], d_prem buffer [Pn * D + GUARD]), NaN-guarded."""
    lib = _lib.load()
    (B, D), Pn = C.shape, P.shape[0]
    dC = guarded(B * D, float("nan"), float("nan"))[0]
    dP = guarded(Pn * D, float("nan"), float("nan"))[0]
    st = lib.rp_contrastive_mse_backward(_lib.ptr(C), _lib.ptr(P), _lib.ptr(S), _lib.ptr(label), B, Pn, D, _lib.ptr(dC),
                                         _lib.ptr(dP), _lib.current_stream())
    torch.cuda.synchronize()
    return st, dC, dP


def last_error():
    return _lib.load().rp_last_error().decode(errors="replace")


from reprover_amd.synth import synth_masks  # noqa: E402,F401  (moved: bench.py --config c5 draws the same operands)


def masks_to_device(m, device):
    f, ek, bt, own, qk = m
    return (torch.from_numpy(f).to(device), torch.from_numpy(ek).to(device),
            torch.from_numpy(bt.view(np.int32)).to(device), torch.from_numpy(own).to(device),
            torch.from_numpy(qk).to(device))


def check_topk_against_scores(ids, scores, counts, S, acc, k, tol):
    """Size-independent properties of an exact masked top-k, given the full fp32 score matrix S
    [B, N] (numpy) and the accessibility predicate acc [B, N]:
    sortedness, accessibility, no duplicates, count = min(k, #accessible), reported score = S at the
    reported id (within tol), and r-th reported score within tol of the true r-th best."""
    B = S.shape[0]
    masked = np.where(acc, S, -np.inf)
    want_sorted = -np.sort(-masked, axis=1)[:, :k]
    n_acc = acc.sum(1)
    assert np.array_equal(counts, np.minimum(k, n_acc)), (counts[:8], n_acc[:8])
    for j in range(B):
        c = int(counts[j])
        row_i, row_s = ids[j, :c], scores[j, :c]
        assert np.all(np.diff(row_s) <= 0), f"row {j} not sorted"
        assert len(set(row_i.tolist())) == c, f"row {j} has duplicate ids"
        assert acc[j, row_i].all(), f"row {j} returned an inaccessible premise"
        assert np.abs(S[j, row_i] - row_s).max(initial=0) <= tol, f"row {j} score mismatch"
        assert np.abs(want_sorted[j, :c] - row_s).max(initial=0) <= tol, f"row {j} not the top-k"
        assert np.all(ids[j, c:] == -1) and np.all(np.isneginf(scores[j, c:]))
        ties = np.flatnonzero(np.diff(row_s) == 0)  # equal scores must come lower-id first
        assert np.all(row_i[ties] < row_i[ties + 1]), f"row {j} tie order"


from oracle.parity_margins import gap_rule_ids  # noqa: E402,F401  (one definition, shared with smoke())


# ---- workspace hygiene: guarded arenas, poisoned workspaces, bit-exact comparison across fills -----------------------------
# (device-agnostic: tests/test_hygiene_harness_cpu.py runs it on CPU tensors against a toy entry point)
RP_E_WORKSPACE = -3
GUARD_BYTE = 0xA5              # what an untouched guard holds
OUTPUT_BYTE = 0x5A             # what an output holds before a call (elements a call leaves alone keep it)
WS_FILLS = (0x00, 0xFF, 0x7F)  # zero pages; NaN / -1 / 255; large finite values whose squares overflow
MIN_GUARD = 1 << 20


def guard_bytes(d_ff=0):
    """Bytes of each guard: at least 1 MiB, and 256 rows of the widest row an entry point stores for the model (the fp32
    gate | up row, 2 * d_ff * 4 bytes), so that one whole 256-row tile stored past a buffer lands in the guard."""
    return max(MIN_GUARD, 256 * 2 * int(d_ff) * 4)


class Arena:
    """One uint8 allocation [lead guard | payload | tail guard]; the payload starts at a multiple of 256 bytes and the
    tail guard at the payload's last byte + 1.  ``init``: the payload's content before every call - a byte value or a
    tensor whose bytes open the payload (the rest is OUTPUT_BYTE).  ``compare=False``: an output whose content is outside
    the determinism contract (guarded, not compared)."""

    def __init__(self, name, nbytes, guard, device, init=OUTPUT_BYTE, dtype=torch.uint8, compare=True):
        self.name, self.nbytes, self.dtype, self.compare = name, int(nbytes), dtype, compare
        self.raw = torch.empty(2 * guard + 256 + self.nbytes, dtype=torch.uint8, device=device)
        self.off = guard + (-(self.raw.data_ptr() + guard)) % 256
        self.lead_byte = self.tail_byte = GUARD_BYTE
        self.raw.fill_(GUARD_BYTE)
        self._init = init if isinstance(init, int) else init.detach().contiguous().view(-1).view(torch.uint8).clone()
        assert isinstance(init, int) or self._init.numel() <= self.nbytes
        self.reset()

    @classmethod
    def of(cls, name, tensor, guard, device=None, compare=True):
        """An arena that holds ``tensor``'s bytes (an input, or an output with a meaningful content on entry)."""
        t = tensor.detach().contiguous()
        return cls(name, t.numel() * t.element_size(), guard, device if device is not None else t.device, init=t,
                   dtype=t.dtype, compare=compare)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off

    def payload(self):
        return self.raw[self.off : self.off + self.nbytes]

    def view(self, *shape, dtype=None):
        """The payload's first elements as a typed tensor of ``shape`` (default: all of it, flat)."""
        dtype = self.dtype if dtype is None else dtype
        size = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) if shape else self.nbytes // size
        return self.payload()[: n * size].view(dtype).view(*(shape or (n,)))

    def at(self, byte_offset, nbytes):
        """Pointer arithmetic: ``nbytes`` bytes at payload + byte_offset, inside the payload or not (the self-test's toy
        entry point plants its out-of-range accesses through this)."""
        return self.raw[self.off + byte_offset : self.off + byte_offset + nbytes]

    def fill(self, byte):
        self.payload().fill_(byte)

    def reset(self):
        if isinstance(self._init, int):
            self.fill(self._init)
        else:
            self.fill(OUTPUT_BYTE)
            self.payload()[: self._init.numel()].copy_(self._init)

    def at_rest(self):
        """True when the payload holds exactly what reset() leaves (nothing was written)."""
        keep = self.payload().clone()
        self.reset()
        same = torch.equal(keep, self.payload())
        self.payload().copy_(keep)
        return same

    def set_tail(self, byte):
        self.tail_byte = byte
        self.raw[self.off + self.nbytes :].fill_(byte)

    def broken_guards(self):
        """The guards that no longer hold their byte pattern, by name ("lead" / "tail"): a bitwise check."""
        bad = []
        if not bool((self.raw[: self.off] == self.lead_byte).all()):
            bad.append("lead")
        if not bool((self.raw[self.off + self.nbytes :] == self.tail_byte).all()):
            bad.append("tail")
        return bad


def _first_difference(arena, a, b):
    size = torch.empty((), dtype=arena.dtype).element_size()
    i = int(torch.nonzero(a != b)[0])
    return f"first differing element {i // size} (byte {i}) of {arena.nbytes // size}"


def hygiene_findings(call, workspace, outputs, inputs=(), fills=WS_FILLS, undersized=True, results=None):
    """Run ``call(workspace_bytes) -> status`` under every workspace fill and input-tail fill and return what went wrong,
    one line per finding (an empty list: the call is clean).  ``workspace`` (an Arena, None, or a list of Arenas for a
    sequence of calls with a workspace each: workspace_bytes then speaks of the first), ``outputs`` and ``inputs``
    (Arenas) are what the call's pointers refer to; outputs and inputs are put back to their initial content before every
    run.  ``results`` (a dict) receives the outputs of the zero-filled run by name, as flat tensors of the arena's dtype.
    Findings, by the words they start with:
      status             a run did not return RP_OK
      guard NAME lead    bytes in front of NAME's payload changed (a store before the buffer, an index of -1)
      guard NAME tail    bytes behind NAME's payload changed (a store past the buffer)
      not reproducible   two runs on a zero-filled workspace differ (nothing else can be concluded then)
      stale workspace    an output depends on what the workspace held on entry (a read before the call's own write)
      input tail         an output depends on the bytes behind an input (a read past its end)
      undersized         workspace_bytes - 1 is not refused with RP_E_WORKSPACE, or the refused call wrote something"""
    spaces = [] if workspace is None else list(workspace) if isinstance(workspace, (list, tuple)) else [workspace]
    workspace = spaces[0] if spaces else None
    everything = spaces + list(outputs) + list(inputs)
    on_gpu = any(a.raw.is_cuda for a in everything)
    findings = []

    def guards(when):
        for a in everything:
            for side in a.broken_guards():
                line = f"guard {a.name} {side}: changed during {when}"
                if line not in findings:
                    findings.append(line)
                (a.raw[: a.off] if side == "lead" else a.raw[a.off + a.nbytes :]).fill_(
                    a.lead_byte if side == "lead" else a.tail_byte)  # re-arm: later runs report their own

    def run(fill, tail, when, ws_bytes=None):
        for a in list(outputs) + list(inputs):
            a.reset()
        for a in inputs:
            a.set_tail(tail)
        for w in spaces:
            w.fill(fill)
        st = call((workspace.nbytes if workspace is not None else 0) if ws_bytes is None else ws_bytes)
        if on_gpu:
            torch.cuda.synchronize()
        guards(when)
        return st, [a.payload().clone() for a in outputs]

    def compare(kind, base, got, when):
        for a, x, y in zip(outputs, base, got):
            if a.compare and not torch.equal(x, y):  # bytes: NaNs compare too
                findings.append(f"{kind}: output {a.name} differs {when}: {_first_difference(a, x, y)}")

    st, base = run(0x00, GUARD_BYTE, "the zero-filled run")
    if st != 0:
        return findings + [f"status {st} from the zero-filled run: {last_error() if on_gpu else ''}"]
    if results is not None:
        results.update({a.name: x.view(a.dtype) for a, x in zip(outputs, base)})
    st, again = run(0x00, GUARD_BYTE, "the repeated zero-filled run")
    compare("not reproducible", base, again, "between two zero-filled runs")
    if st != 0 or any(f.startswith("not reproducible") for f in findings):
        return findings
    for fill in fills:
        if fill == 0x00 or workspace is None:
            continue
        st, got = run(fill, GUARD_BYTE, f"the run with the workspace filled with 0x{fill:02X}")
        if st != 0:
            findings.append(f"status {st} with the workspace filled with 0x{fill:02X}")
        compare("stale workspace", base, got, f"with the workspace filled with 0x{fill:02X}")
    if inputs:
        for tail in (0x00, 0xFF):
            st, got = run(0x00, tail, f"the run with the input tails filled with 0x{tail:02X}")
            if st != 0:
                findings.append(f"status {st} with the input tails filled with 0x{tail:02X}")
            compare("input tail", base, got, f"with the bytes behind the inputs set to 0x{tail:02X}")
        for a in inputs:
            a.set_tail(GUARD_BYTE)
    if undersized and workspace is not None and workspace.nbytes > 0:
        st, _ = run(GUARD_BYTE, GUARD_BYTE, "the undersized call", ws_bytes=workspace.nbytes - 1)
        if st != RP_E_WORKSPACE:
            findings.append(f"undersized: workspace_bytes - 1 returned {st}, not RP_E_WORKSPACE")
        for a in outputs:
            if not a.at_rest():
                findings.append(f"undersized: the refused call wrote to output {a.name}")
        if not all(bool((w.payload() == GUARD_BYTE).all()) for w in spaces):
            findings.append("undersized: the refused call wrote to a workspace")
    return findings
