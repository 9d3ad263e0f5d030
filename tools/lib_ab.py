"""A/B of TWO BUILDS of the library on one box: the bench's encode pass (256 states of the length mix) under each, alternating
processes, and the embeddings compared bit for bit.   python tools/lib_ab.py <libA.so> <libB.so> [rounds]
(step_ab.py compares option sets inside one build; this compares source states.)

--grad (before the libraries) runs the teacher-forced decoder instead: tools/seq2seq_bench.py --grad's inputs (ByT5-small
synthetic sharp, B = 64, 2300-byte sources, targets 64 and 512), rp_decoder_forward and rp_decoder_loss_grad alternating as
there; lp, sc, the gradient buffer's live elements and d_enc are compared bit for bit between the builds and the medians of
both calls reported; the exit status is 0 only with equal bits and every median of B within A's median + A's spread over
its rounds.   python tools/lib_ab.py --grad [--out FILE] [--ids ID_A ID_B] <libA.so> <libB.so> [rounds]"""
import os, subprocess, sys, json, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _children(libs, rounds, leg):
    """`rounds` alternating fresh processes per library: the JSON line of each, per library, and what the last process of
    each library saved (exchanged through a directory of this run's own)"""
    res = {l: [] for l in libs}
    tmp = tempfile.TemporaryDirectory(prefix="lib_ab_")
    for r in range(rounds):
        for l in libs:
            path, _, envs = l.partition("@")  # "lib.so@VAR=value,VAR2=value": the same build under another environment
            env = dict(os.environ, **dict(kv.split("=") for kv in envs.split(",") if kv))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), leg, path, os.path.join(tmp.name, f"{libs.index(l)}.pt")],
                                 capture_output=True, text=True, timeout=600, env=env)
            line = [x for x in out.stdout.splitlines() if x.startswith("{")]
            if not line:
                print(out.stdout[-2000:], out.stderr[-2000:]); sys.exit(1)
            res[l].append(json.loads(line[-1]))
    import torch
    return res, torch.load(os.path.join(tmp.name, "0.pt")), torch.load(os.path.join(tmp.name, "1.pt"))


def _grad_parent(argv):
    out_file = ids = None
    if argv[0] == "--out":
        out_file, argv = argv[1], argv[2:]
    if argv[0] == "--ids":
        ids, argv = argv[1:3], argv[3:]
    libs, rounds = argv[:2], int(argv[2]) if len(argv) > 2 else 5
    res, a, b = _children(libs, rounds, "--child-grad")
    import torch
    report = dict(metric="seq2seq_unify_ab", measured=True, builds=dict(zip("ab", ids or libs)), rounds=rounds,
                  same_bits={k: bool(a[k].shape == b[k].shape and torch.equal(a[k], b[k])) for k in sorted(a)}, ms={})
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    for key in res[libs[0]][0]:  # "64.forward_ms", ...
        xa, xb = [x[key] for x in res[libs[0]]], [x[key] for x in res[libs[1]]]
        report["ms"][key] = dict(a_rounds=xa, b_rounds=xb, a_median=med(xa), b_median=med(xb), a_spread=round(max(xa) - min(xa), 3),
                                 b_within_a_spread=bool(med(xb) <= med(xa) + (max(xa) - min(xa))))
    line = json.dumps(report)
    print(line)
    if out_file:
        with open(out_file, "w") as fh:
            fh.write(line + "\n")
    # both are requirements: the same bits, and no median above the first build's by more than that build's own spread
    ok = set(a) == set(b) and all(report["same_bits"].values()) and all(v["b_within_a_spread"] for v in report["ms"].values())
    sys.exit(0 if ok else 1)


if len(sys.argv) >= 4 and sys.argv[1] == "--grad":
    _grad_parent(sys.argv[2:])
if len(sys.argv) >= 3 and not sys.argv[1].startswith("--child"):
    libs, rounds = sys.argv[1:3], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    res, a, b = _children(libs, rounds, "--child")
    import torch
    print("same bits:", bool(torch.equal(a, b)), " max |d|:", float((a.float() - b.float()).abs().max()))
    for l in libs:
        ms = sorted(x["ms"] for x in res[l]); ks = res[l][0]["kernels"].keys()
        med = {k: sorted(x["kernels"][k] for x in res[l])[len(res[l]) // 2] for k in ks}
        print(f"{l}: median {ms[len(ms) // 2]:.3f} ms | " + " ".join(f"{k} {v:.3f}" for k, v in med.items() if v > 0.05))
    sys.exit(0)
lib_path, out_path = sys.argv[2], sys.argv[3]
sys.path.insert(0, ROOT)
import numpy as np, torch, time
import bench
from reprover_amd import _lib, synth, tokenizer
from reprover_amd.encoder import HipT5Encoder
_lib.LIB_PATH = os.path.abspath(lib_path)
import ctypes
_probe = ctypes.CDLL(_lib.LIB_PATH)  # an OLDER build may lack debug entry points added since: bind what it has
for _name in [n for n in _lib.SIGNATURES if not hasattr(_probe, n)]:
    assert _name.startswith("rp_dbg_"), _name
    del _lib.SIGNATURES[_name]
lib = _lib.load()
dev = torch.device("cuda", 0)
if sys.argv[1] == "--child-grad":
    from seq2seq_bench import _source
    from reprover_amd.decoder import HipT5Generator, shift_and_segment
    cfg = synth.seq2seq_config("byt5-small")
    gen = HipT5Generator(cfg, synth.synth_seq2seq_state_dict(cfg, scale="sharp"), dev)
    dec = gen.decoder
    B, S, N = 64, 2300, 5
    src_cu = np.arange(B + 1, dtype=np.int32) * S
    enc = gen.encode_hidden_packed(np.concatenate([_source(S, 100 + b) for b in range(B)]), src_cu)
    names, off = dec.grad_layout()
    shapes = dec.grad_shapes()
    grads = torch.zeros(int(off[-1]), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    saved, times = {}, {}
    for T in (64, 512):
        y = np.concatenate([rng.integers(3, 259, size=(B, T - 1)), np.ones((B, 1), np.int64)], 1)
        tokens, labels, tgt_cu = shift_and_segment(y)
        fwd = lambda: dec.forward(enc, src_cu, tokens, labels, tgt_cu)  # noqa: E731
        bwd = lambda: dec.loss_grad(enc, src_cu, tokens, labels, tgt_cu, True, grads)  # noqa: E731
        fwd(), bwd()
        torch.cuda.synchronize()
        ts = {"forward_ms": [], "loss_grad_ms": []}
        for _ in range(N):  # alternating: both see the same clocks and the same neighbours
            for k, fn in (("forward_ms", fwd), ("loss_grad_ms", bwd)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1))
        for k, v in ts.items():
            times[f"{T}.{k}"] = round(float(np.median(v)), 3)
        lp, sc, flat, d_enc = out  # the last loss_grad
        live = torch.cat([flat[int(off[i]) : int(off[i]) + int(np.prod(shapes[n]))] for i, n in enumerate(names)])
        saved.update({f"{T}.lp": lp.cpu(), f"{T}.sc": torch.tensor(sc, dtype=torch.float64), f"{T}.grads": live.cpu(),
                      f"{T}.d_enc": d_enc.cpu(), f"{T}.forward_lp": fwd()[0].cpu()})
    torch.save(saved, out_path)
    print(json.dumps(times))
    sys.exit(0)
cfg = synth.t5_config("byt5-small")
enc = HipT5Encoder(cfg, bench.random_init_state_dict(cfg, dev, seed=synth.SEED), dev, torch.bfloat16)
rng = np.random.default_rng(synth.SEED + 100)
lens = synth.synth_lengths(rng, 256, "mix", lo=16, hi=2048)
ids_np, cu_np = tokenizer.encode_packed([synth.synth_state(rng, int(n) - 1) for n in lens], 2048)
T, max_len = int(cu_np[-1]), int(np.diff(cu_np).max())
ids_d, cu_d = torch.from_numpy(ids_np).to(dev), torch.from_numpy(cu_np).to(dev)
out = torch.empty((256, cfg["d_model"]), dtype=torch.bfloat16, device=dev)
for _ in range(3):
    enc.encode_packed_device(ids_d, cu_d, 256, T, max_len, out)
torch.cuda.synchronize()
t0 = time.perf_counter()
N = 10
for _ in range(N):
    enc.encode_packed_device(ids_d, cu_d, 256, T, max_len, out)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / N * 1e3
_lib.profile_enable(True)
for _ in range(N):
    enc.encode_packed_device(ids_d, cu_d, 256, T, max_len, out)
torch.cuda.synchronize()
prof = _lib.profile_read(); _lib.profile_enable(False)
torch.save(out.view(torch.int16).cpu(), out_path)
print(json.dumps({"ms": ms, "kernels": {k: v[0] / N for k, v in prof.items()}}))
