"""What the similarity scan launches, call by call, for comparing two source states (docs/HISTORY.md section 20).

  rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/scan_launches.py run CALLS.json
  python tools/scan_launches.py join CALLS.json TRACE > LISTING.json     # per call: hash + (kernel, grid, workgroup, LDS) sequence
  python tools/scan_launches.py same LISTING_A.json LISTING_B.json       # exit status 0 when equal

`run` walks a fixed list of calls - all four entry points, the four options tests use, the edges of the query-count classes, the
row shapes, dense and two-pass plans - and writes, per call, a hash of ids, scores and counts.  A marker kernel (rp_dbg_mfma_probe,
which nothing else here launches) separates the calls in the trace.  Uses only entry points both source states have."""
import csv, glob, hashlib, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCAN_KERNELS = re.compile(r"sim_scan_kernel|sim_filter_kernel|gather_select_kernel|select_kernel")
MARKER = "mfma_probe"
BF16, E4M3 = ((False, 64), (False, 96), (False, 1472)), ((True, 64), (True, 128), (True, 192), (True, 1472), (True, 1536))


def calls():
    """(e4m3, D, B, N, k, flags, paged, options)"""
    out = [(f, D, B, 16700, 10, 0, 0, {}) for f, D in BF16 + E4M3 for B in (1, 33, 65, 129)]
    out += [(f, D, B, 16700, 100, 0, 0, {}) for f, D in ((False, 64), (False, 96), (True, 128)) for B in (1792, 2048)]
    out += [(f, D, B, 130000, 100, 0, 0, {}) for f, D in ((False, 1472), (True, 1472), (True, 1536)) for B in (1, 256)]
    out += [(False, 64, 129, 16384, 10, 0, 0, {}), (True, 128, 129, 16384, 10, 0, 0, {}), (False, 96, 65, 16700, 10, 1, 0, {}),
            (True, 192, 65, 16700, 10, 1, 0, {})]
    out += [(f, D, B, 16700, 10, 0, 1, {}) for f, D in ((False, 64), (True, 128), (True, 192)) for B in (1, 129)]
    out += [(False, 64, 1, 16700, 10, 0, 0, {"scan_small_tiles": 0}), (True, 192, 33, 16700, 10, 0, 0, {"scan_small_tiles": 0}),
            (False, 64, 129, 16384, 10, 0, 0, {"scan_cfg": 1}), (True, 128, 129, 16700, 10, 0, 0, {"scan_cfg": 1, "scan_impl": 1}),
            (False, 64, 129, 16700, 10, 0, 0, {"scan_impl": 1}), (True, 128, 129, 16700, 10, 0, 1, {"scan_impl": 1}),
            (False, 64, 1, 16700, 10, 0, 0, {"scan_force_new": 1}), (True, 192, 33, 16700, 10, 0, 1, {"scan_force_new": 1})]
    return out


def run(out_path):
    import numpy as np, torch
    from reprover_amd import _lib, synth
    lib = _lib.load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    sink = torch.zeros(64, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    res = []
    for i, (fp8, D, B, N, k, flags, paged, opts) in enumerate(calls()):
        gen.manual_seed(i)
        E = torch.nn.functional.normalize(torch.randn(N, D, generator=gen, device=dev), dim=1).to(torch.bfloat16)
        Q = torch.nn.functional.normalize(torch.randn(B, D, generator=gen, device=dev), dim=1).to(torch.bfloat16)
        m, _ = synth.synth_masks(np.random.default_rng(i), N, B, 500)
        f, ek, bt, own, qk = [torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev) for a in m]
        scales = []
        if fp8:
            ops = []
            for X in (Q, E):
                codes, sc = torch.empty(X.shape, dtype=torch.uint8, device=dev), torch.empty(X.shape[0], dtype=torch.float32, device=dev)
                _lib.check(lib.rp_quantize_rows_e4m3(p(X), _lib.RP_DT_BF16, X.shape[0], D, p(codes), p(sc), _lib.current_stream()), "quantize")
                ops.append(codes)
                scales.append(sc)
            Q, E = ops
        outs = [torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev),
                torch.empty((B,), dtype=torch.int32, device=dev)]

        def call(after):
            nb = lib.rp_sim_topk_workspace_bytes(B, N, D, k, flags)  # (under the call's options)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            head = [p(Q), p(scales[0]), p(E), p(scales[1])] if fp8 else [p(Q), p(E)]
            tail = [B, N, D, p(f), p(ek), p(bt), bt.shape[0], p(own), p(qk), 3] + ([p(after[0]), p(after[1])] if after else []) + \
                [k, flags, p(outs[0]), p(outs[1]), p(outs[2]), p(ws), nb, _lib.current_stream()]
            name = "rp_sim_topk" + ("_fp8" if fp8 else "") + ("_after" if after else "")
            _lib.check(getattr(lib, name)(*head, *tail), name)
            torch.cuda.synchronize()

        _lib.check(lib.rp_dbg_mfma_probe(4, 32, p(sink), _lib.current_stream()), "marker")
        for n, v in opts.items():
            _lib.check(lib.rp_set_option(n.encode(), v), n)
        try:
            after = None
            if paged:  # the page behind the first page's last entry (both pages belong to this call's launches)
                call(None)
                after = (outs[0][:, -1].contiguous(), outs[1][:, -1].contiguous())
            call(after)
        finally:
            for n in opts:
                _lib.check(lib.rp_set_option(n.encode(), 1 if n == "scan_small_tiles" else 0), n)
        h = hashlib.sha1(b"".join(t.cpu().numpy().tobytes() for t in outs)).hexdigest()[:16]
        desc = f"{'e4m3' if fp8 else 'bf16'} D={D} B={B} N={N} k={k} flags={flags} paged={paged} {opts}"
        print(i, desc, h, flush=True)
        res.append({"call": desc, "hash": h})
    json.dump(res, open(out_path, "w"), indent=1)


def join(calls_path, trace_dir):
    res = json.load(open(calls_path))
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seg = -1
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            seg += 1
            res[seg]["launches"] = []
        elif seg >= 0 and SCAN_KERNELS.search(name):
            name = re.sub(r"^void |\(.*$", "", name)
            res[seg]["launches"].append([name, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]),
                                         int(r["Workgroup_Size_X"]) if "Workgroup_Size_X" in r else int(r["Workgroup_Size"]),
                                         int(r.get("LDS_Block_Size") or r["Group_Segment_Size"])])
    assert seg == len(res) - 1, (seg, len(res))
    json.dump(res, sys.stdout, indent=1)


def same(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = [x["call"] for x, y in zip(A, B) if x != y]
    print(f"{len(A)} / {len(B)} calls, {sum(len(x['launches']) for x in A)} launches; differing: {bad}")
    sys.exit(0 if len(A) == len(B) and not bad else 1)


if __name__ == "__main__":
    {"run": run, "join": join, "same": same}[sys.argv[1]](*sys.argv[2:])
