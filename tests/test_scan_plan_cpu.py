"""The similarity scan's plan (rp_dbg_sim_plan: what rp_sim_topk[_fp8][_after] would launch, no GPU call) against the selection
written out here - not read from the C source: the tile of each pass by row shape and query-count class, the workgroup
counts from the block arithmetic, the per-query stage forms, the workspace size."""
import ctypes
import itertools

import pytest

import hip_helpers as hh
from reprover_amd import _lib

BS = (1, 32, 33, 64, 65, 128, 129, 256, 257, 1792, 2048)
SHAPES = [(False, 96), (False, 64), (False, 1472), (True, 64), (True, 128), (True, 192), (True, 1472), (True, 1536)]  # (e4m3, D)
NK = [(16384, 10), (16700, 10), (16700, 100), (130000, 100)]
OPTION_SETTINGS = [{}, {"scan_small_tiles": 0}, {"scan_cfg": 1}, {"scan_impl": 1}, {"scan_force_new": 1}]
DEFAULTS = {"scan_small_tiles": 1, "scan_cfg": 0, "scan_impl": 0, "scan_force_new": 0}
CHIP_CUS = 256
# queries x premises of every first-generation tile
TILE_BM_BN = {"Q256": (256, 128), "Q128W8": (128, 128), "Q128K32W8": (128, 128), "Q64": (64, 128), "Q32": (32, 128),
              "SAMPLE": (128, 64), "SAMPLE_K64W8": (128, 64), "SAMPLE_Q32": (32, 64), "SAMPLE_BIG": (256, 128),
              "8Q256": (256, 128), "8Q128W8": (128, 128), "8Q64": (64, 128), "8Q64_TAIL": (64, 128), "8Q32": (32, 128),
              "8Q32_TAIL": (32, 128), "8SAMPLE": (128, 64), "8SAMPLE_K64W8": (128, 64), "8SAMPLE_K64_TAILW8": (128, 64),
              "8SAMPLE_Q32": (32, 64), "8SAMPLE_Q32_TAIL": (32, 64)}


def cdiv(a, b):
    return (a + b - 1) // b


def align256(x):
    return cdiv(x, 256) * 256


def row_shape(fp8, D):
    if not fp8:
        return "K64" if D % 64 == 0 else "K32"
    D2 = D // 2
    return "WHOLE" if D2 % 64 == 0 else "TAIL" if D2 % 64 == 32 and D2 > 64 else "SHORT"


def dense_tile(fp8, shape, bm):
    if fp8:
        return "8Q256" if bm == 256 else "8Q128W8"
    return "Q256" if bm == 256 else {"K64": "Q128W8", "K32": "Q128K32W8"}[shape]


def sample_tile(fp8, shape, big, q32):
    if big:
        return "8Q256" if fp8 else {"K64": "SAMPLE_BIG", "K32": "Q256"}[shape]
    if fp8:
        if q32 and shape != "SHORT":
            return {"WHOLE": "8SAMPLE_Q32", "TAIL": "8SAMPLE_Q32_TAIL"}[shape]
        return {"WHOLE": "8SAMPLE_K64W8", "TAIL": "8SAMPLE_K64_TAILW8", "SHORT": "8SAMPLE"}[shape]
    if shape == "K64":
        return "SAMPLE_Q32" if q32 else "SAMPLE_K64W8"
    return "SAMPLE"


def filter_tile_gen1(fp8, shape, bm, q32, q64):
    if fp8:
        if q32 and shape != "SHORT":
            return {"WHOLE": "8Q32", "TAIL": "8Q32_TAIL"}[shape]
        if q64 and shape != "SHORT":
            return {"WHOLE": "8Q64", "TAIL": "8Q64_TAIL"}[shape]
        return "8Q256" if bm == 256 else "8Q128W8"
    if bm == 256:
        return "Q256"
    if shape == "K64":
        return "Q32" if q32 else "Q64" if q64 else "Q128W8"
    return "Q128K32W8"


FILTER_TILE_GEN2 = {"K64": "FILTER_NT8", "WHOLE": "8FILTER_W8", "TAIL": "8FILTER_TAILW8"}


def expected_plan(B, N, D, k, flags, fp8, paged, opt):
    shape = row_shape(fp8, D)
    small = opt["scan_small_tiles"]
    bm = 256 if B > 128 and opt["scan_cfg"] != 1 else 128
    q32, q64 = B <= 32 and small, B <= 64 and small
    blocks = cdiv(N, 256)
    stride = 2
    while stride * 2 <= 64 and (stride * 2) ** 2 * k * 4 <= N:
        stride *= 2
    dense = bool(flags & _lib.RP_TOPK_DENSE) or blocks < 2 * stride or (N <= 16384 and B * N <= 16 << 20)
    new = (not dense and opt["scan_impl"] == 0 and shape in FILTER_TILE_GEN2 and (B > 128 or opt["scan_force_new"]))
    sample_blocks = 0 if dense else cdiv(blocks, stride)
    filter_blocks = 0 if dense else blocks - sample_blocks
    dense_ld = cdiv(N, 128) * 128 if dense else sample_blocks * 256
    cap = min(N + k, max(8192, 8 * k * stride) + k)
    tq256 = cdiv(B, 256)

    def wgs(tile, n_blocks, per_block):
        tbm, tbn = TILE_BM_BN[tile]
        return cdiv(B, tbm) * n_blocks * (256 // tbn if per_block else 1)

    def select(bound):
        return "SELECT_SMALL" if B >= 512 and bound <= 4096 else "SELECT"

    e = dict(dense_only=int(dense), new_filter=int(new), stride=stride, sample_blocks=sample_blocks, filter_blocks=filter_blocks,
             cap=cap, paged_filter=int(new and paged), stage0=select(dense_ld))
    if dense:
        e["tile0"] = dense_tile(fp8, shape, bm)
        e["wgs0"] = wgs(e["tile0"], cdiv(N, 128), False)
        e.update(tile1=None, wgs1=0, stage1=None)
    else:
        big = tq256 * sample_blocks * 2 >= CHIP_CUS
        e["tile0"] = sample_tile(fp8, shape, big, q32)
        e["wgs0"] = wgs(e["tile0"], sample_blocks, True)
        assert e["wgs0"] == cdiv(B, TILE_BM_BN[e["tile0"]][0]) * sample_blocks * (2 if big else 4)
        if new:
            e["tile1"] = FILTER_TILE_GEN2[shape]
            e["wgs1"] = tq256 * filter_blocks
            many = B >= 512 and k <= 128
            e["stage1"] = ("GATHER_SMALL" if many and 4 * k * stride <= 1664 else "GATHER_MID" if many and 4 * k * stride <= 3968
                           else "GATHER")
        else:
            e["tile1"] = filter_tile_gen1(fp8, shape, bm, q32, q64)
            e["wgs1"] = wgs(e["tile1"], filter_blocks, True)
            assert e["wgs1"] == cdiv(B, TILE_BM_BN[e["tile1"]][0]) * filter_blocks * 2
            e["stage1"] = select(cap)
    # workspace: dense keys, candidate lists, counters (one per 128-byte line), bounds, their floats, the private runs + counts
    nbytes = align256(B * dense_ld * 8) + (0 if dense else align256(B * cap * 8)) + align256(B * 4 * 32) + align256(B * 8) + \
        align256(B * 4)
    if new:
        nbytes += align256(tq256 * filter_blocks * 256 * 4 * 64 * 8) + align256(tq256 * filter_blocks * 256 * 4 * 4)
    e["bytes"] = nbytes
    return e


def _get(lib, name):
    v = ctypes.c_int32()
    _lib.check(lib.rp_dbg_get_option(name.encode(), ctypes.byref(v)), "get")
    return v.value


@pytest.mark.parametrize("setting", OPTION_SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "defaults")
def test_plan_is_the_written_selection(hip_lib, setting):
    before = {n: _get(hip_lib, n) for n in DEFAULTS}
    assert before == DEFAULTS
    opt = dict(DEFAULTS, **setting)
    seen = set()
    try:
        for n, v in setting.items():
            _lib.check(hip_lib.rp_set_option(n.encode(), v), n)
        for B, (fp8, D), (N, k), paged, flags in itertools.product(BS, SHAPES, NK, (0, 1), (_lib.RP_TOPK_AUTO, _lib.RP_TOPK_DENSE)):
            got = hh.sim_plan(B, N, D, k, flags, fp8, paged)
            want = expected_plan(B, N, D, k, flags, fp8, paged, opt)
            assert got == want, (B, N, D, k, flags, fp8, paged, {f: (got[f], want[f]) for f in got if got[f] != want[f]})
            ws = hip_lib.rp_sim_topk_workspace_bytes(B, N, D, k, flags)
            assert ws >= got["bytes"] if fp8 else ws == got["bytes"], (B, N, D, k, flags, fp8)
            seen.update((got["tile0"], got["tile1"]))
    finally:
        for n, v in before.items():
            _lib.check(hip_lib.rp_set_option(n.encode(), v), n)
    assert {n: _get(hip_lib, n) for n in DEFAULTS} == DEFAULTS
    if not setting:  # the sweep reaches every tile under the defaults
        assert seen - {None} == set(_lib.SIM_TILES), set(_lib.SIM_TILES) - seen


def test_plan_at_the_dense_limit_and_the_chip_fill_edge(hip_lib):
    auto = lambda B, N, k, D=64, fp8=False: hh.sim_plan(B, N, D, k, 0, fp8)  # noqa: E731
    for B in BS:  # 16384 rows: dense by the row limit while B * N <= 16 M keys, i.e. B <= 1024
        p = auto(B, 16384, 10)
        assert p["dense_only"] == (B <= 1024) and (p["dense_only"] or p["stride"] == 16)
        p = auto(B, 16700, 10)
        assert not p["dense_only"] and p["stride"] == 16
        p = auto(B, 16700, 100)
        assert not p["dense_only"] and p["stride"] == 4 and p["sample_blocks"] == 17
    assert 7 * 17 * 2 == 238 < CHIP_CUS <= 8 * 17 * 2 == 272
    assert auto(1792, 16700, 100)["tile0"] == "SAMPLE_K64W8" and auto(2048, 16700, 100)["tile0"] == "SAMPLE_BIG"
    assert auto(1792, 16700, 100, 96)["tile0"] == "SAMPLE" and auto(2048, 16700, 100, 96)["tile0"] == "Q256"
    assert auto(1792, 16700, 100, 128, True)["tile0"] == "8SAMPLE_K64W8" and auto(2048, 16700, 100, 128, True)["tile0"] == "8Q256"
    p = auto(256, 130000, 100, 1472)  # the workload
    assert (p["stride"], p["tile0"], p["tile1"], p["stage1"]) == (16, "SAMPLE_K64W8", "FILTER_NT8", "GATHER")


@pytest.mark.parametrize("args,message", [
    ((4, 100, 48, 10, 0, 0, 0), b"B=4 N=100 D=48 (D must be a multiple of 32)"),
    ((4, 100, 96, 10, 0, 1, 0), b"B=4 N=100 D=96 (D must be a multiple of 64 for e4m3)"),
    ((0, 100, 64, 10, 0, 0, 0), b"B=0 N=100 D=64 (D must be a multiple of 32)"),
    ((4, -1, 64, 10, 0, 1, 1), b"B=4 N=-1 D=64 (D must be a multiple of 64 for e4m3)"),
    ((4, 100, 64, 0, 0, 0, 0), b"k=0 out of range (1..1024)"),
    ((4, 100, 64, 1025, 0, 1, 0), b"k=1025 out of range (1..1024)"),
])
def test_plan_refuses_what_the_scan_refuses(hip_lib, args, message):
    """The messages are sim_topk_impl's own: the two share one check."""
    out = (ctypes.c_int64 * len(_lib.SIM_PLAN_FIELDS))(*([-7] * len(_lib.SIM_PLAN_FIELDS)))
    assert hip_lib.rp_dbg_sim_plan(*args, out) == -1
    assert hip_lib.rp_last_error() == message
    assert list(out) == [-7] * len(_lib.SIM_PLAN_FIELDS)
    # the entry point itself, which checks the shape before it touches a pointer (no GPU call is reached)
    B, N, D, k, flags, fp8, paged = args
    one = ctypes.c_void_p(1)
    if fp8:
        st = hip_lib.rp_sim_topk_fp8(one, one, one, one, B, N, D, None, None, None, 0, None, None, 0, k, flags, one, one, one, None, 0, None)
    else:
        st = hip_lib.rp_sim_topk(one, one, B, N, D, None, None, None, 0, None, None, 0, k, flags, one, one, one, None, 0, None)
    assert st == -1 and hip_lib.rp_last_error() == message


def test_workspace_bytes_takes_any_width(hip_lib):
    """rp_sim_topk_workspace_bytes plans with unchecked arguments: no width may fail."""
    for D in (-64, -1, 0, 1, 33, 48, 100):
        assert hip_lib.rp_sim_topk_workspace_bytes(256, 130000, D, 100, 0) > 0
