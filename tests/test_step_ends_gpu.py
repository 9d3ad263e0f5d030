"""The ends of the training step around the encoder's backward, called through the C ABI (ctypes, reprover_amd._lib) and
checked against the float64 restatements in oracle/train_ref.py (pinned to torch in float64 by tests/test_step_ends_cpu.py):
rp_grad_norm, rp_adamw_step / rp_adamw_step_clipped, the trainer's own optimizer_step on copied inputs, rp_contrastive_mse
and rp_contrastive_mse_backward - at the lengths and shapes where their launch arithmetic has an edge.

Bars (none is a measured number):
  * rp_grad_norm: the longest chain of fp32 roundings that any addend passes through is ceil(n / 2^20) * 4 fused
    multiply-adds in a thread (1024 x 256 threads, one float4 per trip) + 1 tail element + 6 wave + 2 block + 3 + 8 in the
    finishing block = ceil(n / 2^20) * 4 + 20, so the sum of squares is within that count x 2^-24 relative (first order;
    the second-order term is below 1e-9) and the norm within half of it plus one rounding of sqrtf.
  * AdamW: torch's own fp32 clip_grad_norm_ + torch.optim.AdamW on the same inputs on the GPU, measured against the same
    float64 oracle in the same test, is the yardstick: the kernel's max |error| may be at most 2 x the yardstick's plus one
    fp32 ulp of the largest value, for the parameters and for each moment (2: a different, equally valid operation order).
    Hyper-parameters cross the ABI as C floats, so all three - kernel, torch, oracle - are given the fp32-representable
    values (beta2 = 0.999 is 0.99900001287...): the kernel is AdamW for exactly the numbers it receives.  A caller that
    keeps beta2 in double (torch does: it rounds 1 - beta2 = 1e-3 on its own) gets an exp_avg_sq that differs from this
    library's by 1.3e-5 relative; the bias correction uses the same float, so the parameters do not see it.
  * rp_contrastive_mse: similarity within (D / 4 / 64 + 8) x 2^-24 x sum_c |a_c b_c| per entry (per-lane run + wave tree),
    the loss within (B P / 256 + 10) x 2^-24 relative plus the similarity error propagated through mean((S - label)^2);
    gradients within (max(B, P) + 2) x 2^-24 x sum_o |dS| |other| per entry (one fused multiply-add per row of the other
    side, two roundings in dS).  All computed from the inputs in float64.

Measured on the MI355X (the worst case of each group; also in docs/HISTORY.md section 12):
  * rp_grad_norm: relative error at most 7.0e-8 at every length (bound 7.7e-7 .. 2.6e-5); 4.6e-8 at 217,657,472 floats.
  * AdamW, worst kernel / bar pair: n = 3, norm far above max_norm, steps 10,000..10,004, exp_avg_sq: kernel 4.03e-10,
    torch fp32 1.07e-10, bar 4.48e-10 (0.90 of the bar); parameters: never above torch's own error by more than one ulp.
  * the trainer's step on its own inputs: parameters 1.7e-7 (torch fp32 2.5e-7, bar 9.8e-7); worst ratio 0.38 of the bar.
  * rp_contrastive_mse: similarity at most 0.27 of its bound, loss 0.08, gradients 0.46."""
import math

import numpy as np
import pytest
import torch

import hip_helpers as hh
import train_helpers as th
from oracle import train_ref
from reprover_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of fp32
RP_E_INVALID, RP_E_WORKSPACE = -1, -3
POISON = 1e30   # squares to +inf in fp32: a norm that reads one guard element is inf
GUARD_VALUE = 12345.0


def f32(x):
    """The value a C float parameter of the ABI receives."""
    return float(np.float32(x))


def norm64(t):
    """||t||_2 in float64 on the device, in pieces (no 8-byte copy of a 217 M buffer)."""
    s = 0.0
    for lo in range(0, t.numel(), 1 << 24):
        c = t[lo : lo + (1 << 24)].double()
        s += float((c * c).sum())
    return math.sqrt(s)


def norm_bound(n):
    """Relative error bound of rp_grad_norm over n floats (module docstring)."""
    return 0.5 * (math.ceil(n / 1048576) * 4 + 20) * U + U


# ---------------------------------------------------------------------------------------------------------------------
# rp_grad_norm
# ---------------------------------------------------------------------------------------------------------------------
def _small_flat_length():
    from reprover_amd import synth
    from reprover_amd.train import param_layout

    return int(param_layout(synth.t5_config("byt5-small"))[-1][2])


FIRST_TRIP = 262144 * 4  # one float4 per thread of the 1024 x 256 launch
NORM_LENGTHS = [1, 2, 3, 4, 5, 1023, FIRST_TRIP - 1, FIRST_TRIP, FIRST_TRIP + 1, 4 * FIRST_TRIP + 3, 100_003, "byt5-small"]


@pytest.mark.parametrize("n", NORM_LENGTHS)
def test_grad_norm_against_float64(n):
    if n == "byt5-small":
        n = _small_flat_length()
        assert 200e6 < n < 240e6
    gen = torch.Generator(device="cuda").manual_seed(1000 + n % 9973)
    bound = norm_bound(n)
    scratch = torch.empty(1024, dtype=torch.float32, device="cuda")
    buf = torch.empty(n + hh.GUARD, dtype=torch.float32, device="cuda")
    g = buf[:n]
    worst = 0.0
    for kind in ("randn", "heavy", "zero"):
        buf[n:] = POISON
        if kind == "randn":
            g.normal_(generator=gen)
        elif kind == "heavy":  # randn * exp(3 randn): a few elements carry the norm
            g.normal_(generator=gen)
            for lo in range(0, n, 1 << 24):
                c = g[lo : lo + (1 << 24)]
                c.mul_(torch.exp(3.0 * torch.randn(c.numel(), generator=gen, device="cuda")))
        else:
            g.zero_()
        got = float(hh.grad_norm(g, n, scratch))
        again = hh.grad_norm(g, n, scratch)
        assert float(again) == got, "two runs give the same bits"
        want = norm64(g)
        rel = abs(got - want) / want if want > 0 else abs(got)
        worst = max(worst, rel)
        print(f"rp_grad_norm n={n} {kind}: {got:.9g} vs float64 {want:.9g}: rel {rel:.2e}, bound {bound:.2e}")
        assert math.isfinite(got), "the guard behind the n floats was read"
        if kind == "zero":
            assert got == 0.0
        else:
            assert rel <= bound, (n, kind, got, want)
    # one non-zero element: in the last position and in each of the (up to three) tail positions behind the last whole
    # float4, and in the first position - a dropped piece reads as 0, not as a small error.  3^2 = 9, sqrt(9) = 3: exact
    for pos in sorted({0, n - 1} | set(range(n - n % 4, n))):
        g.zero_()
        g[pos] = -3.0
        got = float(hh.grad_norm(g, n, scratch))
        assert got == 3.0, (n, pos, got)
    del buf, g
    torch.cuda.empty_cache()
    print(f"rp_grad_norm n={n}: worst rel {worst:.2e} of bound {bound:.2e}")


def test_grad_norm_rejects_bad_arguments():
    g = torch.ones(8, device="cuda")
    out = torch.full((1,), 7.0, device="cuda")
    scratch = torch.zeros(1024, device="cuda")
    lib = _lib.load()
    for args in ((_lib.ptr(g), 0, _lib.ptr(out), _lib.ptr(scratch)), (None, 8, _lib.ptr(out), _lib.ptr(scratch)),
                 (_lib.ptr(g), 8, None, _lib.ptr(scratch)), (_lib.ptr(g), 8, _lib.ptr(out), None)):
        assert lib.rp_grad_norm(*args, _lib.current_stream()) == RP_E_INVALID and hh.last_error()
    torch.cuda.synchronize()
    assert float(out) == 7.0 and not scratch.any(), "nothing was launched"


# ---------------------------------------------------------------------------------------------------------------------
# rp_adamw_step / rp_adamw_step_clipped
# ---------------------------------------------------------------------------------------------------------------------
MAX_NORM = 1.0
HYPER = {  # name: (lr, betas, eps, weight_decay)
    "torch-defaults": (1e-3, (0.9, 0.999), 1e-8, 1e-2),
    "b.8-.95-eps1e-6-wd0": (1e-3, (0.8, 0.95), 1e-6, 0.0),
    "lr0-warmup": (0.0, (0.9, 0.999), 1e-8, 1e-2),
}
# "small-max-norm": max_norm = 1e-5 with gradient norms around it, where the + 1e-6 of the factor's denominator is 1 - 20 % of it
CLIP_MODES = ("null", "far-above", "below", "zero-grad", "norm-on-stream", "small-max-norm")
# the host picks grid = min(ceil(n4 / 512), 8192) workgroups of 256 threads, two float4 pieces per thread and trip
N_BETWEEN = 4 * (512 * 100 - 37) + 2      # n4 = 51163: grid 100, 100 * 256 < n4 < 2 * 100 * 256 - the second piece partly out of range
N_CAPPED = 8192 * 512 * 4 * 2 + 4 * 12345 + 3  # capped grid, three trips, ragged end and a three-element tail
ADAMW_LENGTHS = [1, 3, 4, 7, 1024, 100_003, N_BETWEEN, N_CAPPED]
_worst = {}  # group -> (ratio, text): the worst kernel / bar pair seen, printed by each test


def _note(group, err, bar, text):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    if group not in _worst or ratio > _worst[group][0]:
        _worst[group] = (ratio, text)


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _torch_yardstick(p0, grads, step0, lr, betas, eps, wd, clip, max_norm=MAX_NORM):
    """torch's fp32 clip_grad_norm_ + torch.optim.AdamW on the GPU over the same inputs -> (param, exp_avg, exp_avg_sq)."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(step0 - 1)),
                    "exp_avg": torch.zeros_like(p0), "exp_avg_sq": torch.zeros_like(p0)}
    for g in grads:
        p.grad = g.clone()
        if clip:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
    st = opt.state[p]
    assert int(st["step"]) == step0 - 1 + len(grads)
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def _compare_with_yardstick(tag, group, got, yard, want):
    """got / yard: (p, m, v) device fp32 of the kernel / of torch; want: the oracle's float64 numpy arrays."""
    for name, a, b, w in zip(("param", "exp_avg", "exp_avg_sq"), got, yard, want):
        e_hip = float(np.abs(a.cpu().numpy().astype(np.float64) - w).max())
        e_torch = float(np.abs(b.cpu().numpy().astype(np.float64) - w).max())
        # the bar: 2 x torch's own fp32 error against the same oracle + one fp32 ulp of the largest value (module docstring)
        bar = 2.0 * e_torch + _ulp(np.abs(w).max())
        print(f"  {tag} {name}: kernel {e_hip:.3e}, torch fp32 {e_torch:.3e}, bar {bar:.3e}")
        _note(group, e_hip, bar, f"{tag} {name}: kernel {e_hip:.3e} / torch fp32 {e_torch:.3e} / bar {bar:.3e}")
        assert np.isfinite(a.cpu().numpy()).all(), (tag, name)
        assert e_hip <= bar, (tag, name, e_hip, e_torch, bar)


def _run_adamw_case(n, mode, hyper, step0, seed):
    lr, betas, eps, wd = HYPER[hyper]
    lr, betas, eps, wd = f32(lr), (f32(betas[0]), f32(betas[1])), f32(eps), f32(wd)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p0 = torch.randn(n, generator=gen, device="cuda")
    # per-step target norms of the gradient relative to max_norm
    targets = {"null": [0.3, 5.0, 1.0, 50.0, 0.7], "far-above": [50.0, 80.0, 35.0, 1e3, 60.0], "below": [0.3, 0.9, 0.05, 0.5, 0.99],
               "zero-grad": [0.0] * 5, "norm-on-stream": [0.5, 40.0, 1.0, 3.0, 0.2], "small-max-norm": [3.0, 1.0, 0.5, 2.0, 10.0]}[mode]
    max_norm = f32(1e-5) if mode == "small-max-norm" else MAX_NORM
    grads = []
    for t in targets:
        g = torch.randn(n, generator=gen, device="cuda")
        g = g * (t * max_norm / norm64(g)) if t > 0 else torch.zeros_like(g)
        grads.append(g)
    bufs = [hh.guarded(n, src, GUARD_VALUE) for src in (p0, 0.0, 0.0, 0.0)]  # param, grad, exp_avg, exp_avg_sq
    (pb, p), (gb, g), (mb, m), (vb, v) = bufs
    twin = [t.clone() for t in (p0, torch.zeros_like(p0), torch.zeros_like(p0))] if mode == "below" else None
    norm_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    scratch = torch.empty(1024, dtype=torch.float32, device="cuda")
    po, mo, vo = p0.cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    for i, gi in enumerate(grads):
        step = step0 + i
        g.copy_(gi)
        true_norm = norm64(gi)
        if mode == "null":
            st = hh.adamw_step(p, g, m, v, step, lr, betas, eps, wd, None, max_norm)
            clip = None
        elif mode == "norm-on-stream":
            # stream order is the only ordering the product has between the norm and the update: no synchronisation
            norm_dev.fill_(float("nan"))
            _lib.check(_lib.load().rp_grad_norm(_lib.ptr(g), n, _lib.ptr(norm_dev), _lib.ptr(scratch), _lib.current_stream()),
                       "rp_grad_norm")
            st = hh.adamw_step(p, g, m, v, step, lr, betas, eps, wd, norm_dev, max_norm)
            clip = (true_norm, max_norm)
        else:
            norm_dev.fill_(true_norm)  # rounded to fp32: the oracle clips by the same number
            st = hh.adamw_step(p, g, m, v, step, lr, betas, eps, wd, norm_dev, max_norm)
            clip = (float(norm_dev), max_norm)
        assert st == 0, hh.last_error()
        if twin is not None:  # the factor is exactly 1: the same bits as the unclipped entry point
            assert hh.adamw_step(twin[0], gi, twin[1], twin[2], step, lr, betas, eps, wd, clipped=False) == 0
            torch.cuda.synchronize()
            for a, b in zip((p, m, v), twin):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (n, hyper, step, "not bit-identical to rp_adamw_step")
        po, mo, vo = train_ref.adamw_step64(po, gi.cpu().numpy(), mo, vo, step, lr, betas, eps, wd, clip=clip)
        if lr == 0.0:
            assert torch.equal(p, p0), "learning rate 0 leaves the parameters bit for bit"
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert hh.guard_intact(buf, n, GUARD_VALUE), "a guard region behind an array was written"
    assert torch.equal(g, grads[-1]), "the gradient is read-only"
    if lr == 0.0 and mode != "zero-grad":
        assert m.abs().max().item() > 0 and v.abs().max().item() > 0, "the moments move during the warm-up step"
    yard = _torch_yardstick(p0, grads, step0, lr, betas, eps, wd, clip=(mode != "null"), max_norm=max_norm)
    tag = f"adamw n={n} {mode} {hyper} steps {step0}..{step0 + 4}"
    _compare_with_yardstick(tag, "adamw", (p, m, v), yard, (po, mo, vo))


@pytest.mark.parametrize("n", ADAMW_LENGTHS)
def test_adamw_clipped_five_steps_against_float64_and_torch(n):
    if n == N_CAPPED:  # 33.6 M floats: the float64 oracle runs on the host, three cases that together cover every mode's code path
        cases = [("norm-on-stream", "torch-defaults", 1), ("below", "b.8-.95-eps1e-6-wd0", 10_000), ("null", "lr0-warmup", 1)]
    else:
        cases = [(mode, hyper, step0) for mode in CLIP_MODES for hyper in HYPER for step0 in (1, 10_000)]
    for i, (mode, hyper, step0) in enumerate(cases):
        _run_adamw_case(n, mode, hyper, step0, seed=31 * n % 100_003 + i)
        torch.cuda.empty_cache()
    print("worst adamw kernel / bar so far:", _worst.get("adamw"))


def test_adamw_rejects_bad_arguments():
    n = 1024
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-2
    bufs = [torch.full((n + 4,), 0.5, device="cuda") for _ in range(4)]
    p, g, m, v = [b[:n] for b in bufs]
    norm = torch.full((1,), 10.0, device="cuda")
    bad = []
    bad.append(hh.adamw_step(p, g, m, v, 1, lr, betas, eps, wd, norm, 1.0, n=0))
    bad.append(hh.adamw_step(p, g, m, v, 0, lr, betas, eps, wd, norm, 1.0))
    bad.append(hh.adamw_step(p, g, m, v, 1, lr, (1.0, 0.999), eps, wd, norm, 1.0))
    for k in range(4):  # each array in turn 4 bytes off a 16-byte boundary
        args = [p, g, m, v]
        args[k] = bufs[k][1 : n + 1]
        bad.append(hh.adamw_step(*args, 1, lr, betas, eps, wd, norm, 1.0))
        assert "aligned" in hh.last_error()
    bad.append(hh.adamw_step(p, g, m, v, 0, lr, betas, eps, wd, clipped=False))
    assert all(st == RP_E_INVALID for st in bad), bad
    assert hh.last_error()
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs), "nothing was launched"


# ---------------------------------------------------------------------------------------------------------------------
# the trainer's own optimizer step, on copied inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gap_elements_stay_zero():
    """A padding gap of the flat buffers as the optimizer end sees it: parameter, gradient and both moments zero.  Three
    clipped steps with weight decay leave every one of them +0.0 bit for bit (the norm runs over the whole flat buffer, so
    anything else would leak into every later clip factor), whatever the rest of the buffer holds."""
    n = 64 + 37
    gen = torch.Generator(device="cuda").manual_seed(5)
    p, g, m, v = (torch.randn(n, generator=gen, device="cuda") for _ in range(4))
    m.mul_(0.1), v.abs_()
    gap = slice(40, 64)
    for t in (p, g, m, v):
        t[gap] = 0.0
    for step in range(1, 4):
        norm = hh.grad_norm(g, sync=False)
        assert hh.adamw_step(p, g, m, v, step, 1e-3, (0.9, 0.999), 1e-8, 1e-2, norm, 0.5) == 0
        g[:40].normal_(generator=gen)
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert not bool(t[gap].view(torch.int32).any()), "a gap element left +0.0"
        assert bool(t[:40].any())


@pytest.mark.parametrize("clip_engages", [True, False])
def test_trainer_optimizer_step_equals_the_oracle_on_its_own_inputs(golden_dir, clip_engages):
    """HipT5Trainer.optimizer_step (rp_grad_norm + rp_adamw_step_clipped over the flat buffers, as the product runs them)
    isolated from the bf16 noise of the gradients: the float64 clipped AdamW is applied to COPIES of the trainer's own
    gradients, parameters and moments, so the optimizer end can be held to the AdamW bar where the end-to-end fixture
    needs 4.2 x lr."""
    from reprover_amd.train import HipT5Trainer

    cfg, sd, groups, label, g = th.g11_batch(golden_dir)
    lr_base, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-2
    tr = HipT5Trainer(cfg, sd, "cuda:0", lr=lr_base, warmup_steps=1, betas=betas, eps=eps, weight_decay=wd)
    n = tr.params.numel()
    covered = torch.zeros(n, dtype=torch.bool, device="cuda")
    for key, shape, off in tr.layout[:-1]:
        covered[off : off + int(np.prod(shape))] = True
    gaps = ~covered
    # Every tensor starts at a multiple of 64 elements; a gap exists only behind a tensor whose size is not one, and with
    # d_model and d_ff multiples of 64 that is the [32, heads] bias table of an odd head count alone: G11's geometry (and
    # ByT5-small / base) has none, so the assertion below holds for whatever gaps a layout has, and what the optimizer end
    # does to a gap element - all four arrays zero there - is checked directly by _gap_elements_stay_zero.
    assert all(off % 64 == 0 for _, _, off in tr.layout)
    print(f"flat layout: {n} elements, {int(gaps.sum())} in padding gaps")
    _gap_elements_stay_zero()
    fb = (f32(betas[0]), f32(betas[1]))
    for step in range(1, 4):
        tr.contrastive_step(groups, label)
        grads, p_in, m_in, v_in = tr.grads.clone(), tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
        true_norm = norm64(grads)
        # step 1 runs at learning rate 0 (warm-up): the first EFFECTIVE step is the second; half the norm always clips
        tr.gradient_clip_val = 0.5 * true_norm if clip_engages else 1e9
        lr = f32(tr.current_lr())
        tr.optimizer_step()
        torch.cuda.synchronize()
        got_norm = float(tr.grad_norm)
        rel = abs(got_norm - true_norm) / true_norm
        print(f"trainer step {step}: grad_norm {got_norm:.6g} vs float64 {true_norm:.6g}: rel {rel:.2e}, bound {norm_bound(n):.2e}")
        assert rel <= norm_bound(n)
        clip = (true_norm, f32(tr.gradient_clip_val))
        want = train_ref.adamw_step64(p_in.cpu().numpy(), grads.cpu().numpy(), m_in.cpu().numpy(), v_in.cpu().numpy(), step,
                                      lr, fb, f32(eps), f32(wd), clip=clip)
        if step == 1:
            assert lr == 0.0 and torch.equal(tr.params, p_in)
        # the yardstick takes ONE step from the same copies
        p = torch.nn.Parameter(p_in.clone())
        opt = torch.optim.AdamW([p], lr=lr, betas=fb, eps=f32(eps), weight_decay=f32(wd))
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m_in.clone(), "exp_avg_sq": v_in.clone()}
        p.grad = grads.clone()
        torch.nn.utils.clip_grad_norm_([p], f32(tr.gradient_clip_val))
        opt.step()
        yard = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
        _compare_with_yardstick(f"trainer step {step} clip {'on' if clip_engages else 'off'}", "trainer",
                                (tr.params, tr.exp_avg, tr.exp_avg_sq), yard, want)
        if clip_engages:
            assert train_ref.clip_coef(*clip) < 0.51
        for name, flat in (("grads", tr.grads), ("params", tr.params), ("exp_avg", tr.exp_avg), ("exp_avg_sq", tr.exp_avg_sq)):
            assert not bool(flat[gaps].any()), f"padding gaps of {name} must stay exactly zero (the norm runs over the whole buffer)"
    print("worst trainer kernel / bar:", _worst.get("trainer"))


# ---------------------------------------------------------------------------------------------------------------------
# rp_contrastive_mse / rp_contrastive_mse_backward
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = [(1, 0), (1, 1), (2, 1), (3, 2), (8, 3), (13, 3), (32, 7)]  # (B, negatives): P = B (1 + negatives)
FORWARD_D = [4, 12, 64, 252, 1472, 1536, 2048]
BACKWARD_D = FORWARD_D + [7, 300]


def _mse_operands(B, nneg, D, seed, big=False):
    P = B * (1 + nneg)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    C = torch.randn(B, D, generator=gen, device="cuda")
    Pm = torch.randn(P, D, generator=gen, device="cuda")
    if big:  # rows of norm ~ 30, labels in [-2, 2]: nothing may assume |similarity| <= 1
        C = torch.nn.functional.normalize(C, dim=1) * 30.0
        Pm = torch.nn.functional.normalize(Pm, dim=1) * 30.0
        label = torch.rand(B, P, generator=gen, device="cuda") * 4.0 - 2.0
    else:  # unit-norm rows and 0 / 1 labels, as the product hands them over
        C, Pm = torch.nn.functional.normalize(C, dim=1), torch.nn.functional.normalize(Pm, dim=1)
        label = (torch.rand(B, P, generator=gen, device="cuda") < 0.25).float()
    return C.contiguous(), Pm.contiguous(), label.contiguous()


def _check_forward(B, nneg, D, seed, big=False):
    C, Pm, label = _mse_operands(B, nneg, D, seed, big)
    P = Pm.shape[0]
    st, loss_b, sim_b = hh.contrastive_mse_raw(C, Pm, label)
    assert st == 0, hh.last_error()
    assert hh.guard_intact(loss_b, 1, float("nan")) and hh.guard_intact(sim_b, B * P, float("nan"))
    c64, p64, l64 = (t.cpu().numpy().astype(np.float64) for t in (C, Pm, label))
    loss_ref, S_ref, _, _ = train_ref.contrastive_mse(c64, p64, l64)
    sim = sim_b[: B * P].view(B, P).cpu().numpy().astype(np.float64)
    # per entry: (D / 4 / 64 + 8) roundings in the longest chain (per-lane run + wave tree) x 2^-24 x sum_c |a_c b_c|
    sim_bar = (D / 4 / 64 + 8) * U * (np.abs(c64) @ np.abs(p64).T)
    sim_err = np.abs(sim - S_ref)
    assert np.all(sim_err <= sim_bar), (B, P, D, float((sim_err / sim_bar).max()))
    # loss: (B P / 256 + 10) roundings (per-thread chunk + tree + the squares) relative, plus the similarity error
    # bound propagated through mean((S - label)^2): mean(2 |S - label| dS + dS^2)
    diff = np.abs(S_ref - l64)
    loss_bar = (B * P / 256 + 10) * U * loss_ref + float(np.mean(2.0 * diff * sim_bar + sim_bar ** 2))
    loss = float(loss_b[0])
    loss_err = abs(loss - loss_ref)
    ratio = float((sim_err / sim_bar).max())
    print(f"contrastive_mse B={B} P={P} D={D}{' big' if big else ''}: similarity err / bar {ratio:.3f}, loss {loss:.8g} err "
          f"{loss_err:.2e} bar {loss_bar:.2e}")
    _note("mse-forward", ratio, 1.0, f"B={B} P={P} D={D}: similarity err / bar {ratio:.3f}")
    _note("mse-loss", loss_err, loss_bar, f"B={B} P={P} D={D}: loss err {loss_err:.2e} / bar {loss_bar:.2e}")
    assert loss_err <= loss_bar, (B, P, D, loss, loss_ref)
    # without the similarity output: the same loss bits; and two runs agree bit for bit
    st2, loss2, none = hh.contrastive_mse_raw(C, Pm, label, want_sim=False)
    st3, loss3, sim3 = hh.contrastive_mse_raw(C, Pm, label)
    assert st2 == 0 and st3 == 0 and none is None
    assert torch.equal(loss2.view(torch.int32), loss_b.view(torch.int32)), "out_similarity = NULL changes the loss"
    assert torch.equal(loss3.view(torch.int32), loss_b.view(torch.int32)) and torch.equal(sim3.view(torch.int32), sim_b.view(torch.int32))
    return C, Pm, label


def _check_backward(B, nneg, D, seed, big=False):
    C, Pm, label = _mse_operands(B, nneg, D, seed, big)
    P = Pm.shape[0]
    c64, p64, l64 = (t.cpu().numpy().astype(np.float64) for t in (C, Pm, label))
    S32 = torch.from_numpy((c64 @ p64.T).astype(np.float32)).cuda().contiguous()  # the stored fp32 similarity the backward is handed
    st, dC_b, dP_b = hh.contrastive_mse_backward_raw(C, Pm, S32, label)
    assert st == 0, hh.last_error()
    assert hh.guard_intact(dC_b, B * D, float("nan")) and hh.guard_intact(dP_b, P * D, float("nan"))
    s64 = S32.cpu().numpy().astype(np.float64)
    _, _, dC_ref, dP_ref = train_ref.contrastive_mse(c64, p64, l64, similarity=s64)
    dS = np.abs(2.0 * (s64 - l64) / (B * P))
    # per entry: max(B, P) fused multiply-adds over the rows of the other side + 2 roundings in dS
    bar_c = (max(B, P) + 2) * U * (dS @ np.abs(p64))
    bar_p = (max(B, P) + 2) * U * (dS.T @ np.abs(c64))
    dC = dC_b[: B * D].view(B, D).cpu().numpy().astype(np.float64)
    dP = dP_b[: P * D].view(P, D).cpu().numpy().astype(np.float64)
    ec, ep = np.abs(dC - dC_ref), np.abs(dP - dP_ref)
    assert np.isfinite(dC).all() and np.isfinite(dP).all()
    tiny = 1e-300
    ratio = max(float((ec / (bar_c + tiny)).max()), float((ep / (bar_p + tiny)).max()))
    print(f"contrastive_mse_backward B={B} P={P} D={D}{' big' if big else ''}: max err / bar {ratio:.3f} "
          f"(max |dC| {np.abs(dC_ref).max():.2e}, max |dP| {np.abs(dP_ref).max():.2e})")
    _note("mse-backward", ratio, 1.0, f"B={B} P={P} D={D}: err / bar {ratio:.3f}")
    assert np.all(ec <= bar_c) and np.all(ep <= bar_p), (B, P, D, ratio)
    st2, dC2, dP2 = hh.contrastive_mse_backward_raw(C, Pm, S32, label)
    assert st2 == 0 and torch.equal(dC2.view(torch.int32), dC_b.view(torch.int32)) and torch.equal(dP2.view(torch.int32), dP_b.view(torch.int32))


@pytest.mark.parametrize("B,nneg", BATCHES)
def test_contrastive_mse_forward_against_float64(B, nneg):
    for D in FORWARD_D:
        _check_forward(B, nneg, D, seed=17 * B + nneg + D)
    _check_forward(B, nneg, 1472, seed=5 * B + nneg, big=True)
    print("worst so far:", _worst.get("mse-forward"), _worst.get("mse-loss"))


@pytest.mark.parametrize("B,nneg", BATCHES)
def test_contrastive_mse_backward_against_float64(B, nneg):
    for D in BACKWARD_D:
        _check_backward(B, nneg, D, seed=19 * B + nneg + D)
    _check_backward(B, nneg, 1472, seed=7 * B + nneg, big=True)
    print("worst so far:", _worst.get("mse-backward"))


def test_contrastive_mse_rejects_bad_arguments():
    C, Pm, label = _mse_operands(3, 2, 64, seed=3)
    need = _lib.load().rp_contrastive_mse_workspace_bytes(3, 9)
    assert need >= 3 * 9 * 4
    st, loss, sim = hh.contrastive_mse_raw(C, Pm, label, ws_bytes=need - 1)
    assert st == RP_E_WORKSPACE and "workspace" in hh.last_error()
    assert hh.guard_intact(loss, 0, float("nan")) and hh.guard_intact(sim, 0, float("nan")), "nothing was launched"
    # D = 6: the forward reads 16-byte pieces (the first six columns of the same buffers; never launched)
    st, loss, sim = hh.contrastive_mse_raw(C, Pm, label, D=6)
    assert st == RP_E_INVALID and "multiple of 4" in hh.last_error()
    assert hh.guard_intact(loss, 0, float("nan")) and hh.guard_intact(sim, 0, float("nan"))
    lib = _lib.load()
    dC, dP = torch.zeros_like(C), torch.zeros_like(Pm)
    S = torch.zeros(3, 9, device="cuda")
    assert lib.rp_contrastive_mse_backward(_lib.ptr(C), _lib.ptr(Pm), _lib.ptr(S), _lib.ptr(label), 3, 9, 0, _lib.ptr(dC),
                                           _lib.ptr(dP), _lib.current_stream()) == RP_E_INVALID
    assert lib.rp_contrastive_mse_backward(_lib.ptr(C), _lib.ptr(Pm), None, _lib.ptr(label), 3, 9, 64, _lib.ptr(dC),
                                           _lib.ptr(dP), _lib.current_stream()) == RP_E_INVALID
    torch.cuda.synchronize()
    assert not dC.any() and not dP.any()
