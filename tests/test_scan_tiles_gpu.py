"""Every tile of the similarity scan (RpSimTile in include/reprover_hip.h), the paged twins of the filter tiles included, alone at
the smallest shape that reaches it: the plan report (rp_dbg_sim_plan) must name the tile the case is called after, and on
small-integer embeddings - every score exact, ties abound - ids, scores and counts must equal the oracle's (score descending,
id ascending) ranking bit for bit, under the plan that reaches the tile and under RP_TOPK_DENSE.

N = 16700 is just over the dense limit and ends inside its last 256-row block; B sits at the edges of the query-count classes
(32 | 64 | 128 | the chip-filling sample at 2048 x 17 sampled blocks)."""
import functools

import numpy as np
import pytest
import torch

import hip_helpers as hh
from oracle import common_ref, fp8_ref
from reprover_amd import _lib

pytestmark = pytest.mark.gpu

N = 16700
FILTER_TILES = ("FILTER_NT8", "8FILTER_W8", "8FILTER_TAILW8")
# tile -> (pass whose tile it is, e4m3, B, D, k, options)
CASES = {
    "Q256": ("tile1", False, 129, 64, 10, {"scan_impl": 1}),
    "Q128W8": ("tile1", False, 65, 64, 10, {}),
    "Q128K32W8": ("tile1", False, 1, 96, 10, {}),
    "Q64": ("tile1", False, 33, 64, 10, {}),
    "Q32": ("tile1", False, 32, 64, 10, {}),
    "SAMPLE": ("tile0", False, 1, 96, 10, {}),
    "SAMPLE_K64W8": ("tile0", False, 33, 64, 10, {}),
    "SAMPLE_Q32": ("tile0", False, 32, 64, 10, {}),
    "SAMPLE_BIG": ("tile0", False, 2048, 64, 100, {}),
    "8Q256": ("tile1", True, 129, 128, 10, {"scan_impl": 1}),
    "8Q128W8": ("tile1", True, 65, 128, 10, {}),
    "8Q64": ("tile1", True, 64, 128, 10, {}),
    "8Q64_TAIL": ("tile1", True, 33, 192, 10, {}),
    "8Q32": ("tile1", True, 1, 128, 10, {}),
    "8Q32_TAIL": ("tile1", True, 32, 192, 10, {}),
    "8SAMPLE": ("tile0", True, 1, 64, 10, {}),
    "8SAMPLE_K64W8": ("tile0", True, 64, 128, 10, {}),
    "8SAMPLE_K64_TAILW8": ("tile0", True, 33, 192, 10, {}),
    "8SAMPLE_Q32": ("tile0", True, 1, 128, 10, {}),
    "8SAMPLE_Q32_TAIL": ("tile0", True, 32, 192, 10, {}),
    "FILTER_NT8": ("tile1", False, 129, 64, 10, {}),
    "8FILTER_W8": ("tile1", True, 129, 128, 10, {}),
    "8FILTER_TAILW8": ("tile1", True, 257, 192, 10, {}),
}
PARAMS = [(t, 0) for t in CASES] + [(t, 1) for t in FILTER_TILES]


@functools.lru_cache(maxsize=None)
def _problem(fp8, B, D, depth):
    """Operands in {-2 .. 2} (exact in bf16 and e4m3; e4m3: power-of-two row scales), masks, and the oracle's ranking `depth`
    deep - computed once per shape, shared by the cases that use it."""
    rng = np.random.default_rng(1000 * D + B + fp8)
    Ei = rng.integers(-2, 3, size=(N, D)).astype(np.float32)
    Qi = rng.integers(-2, 3, size=(B, D)).astype(np.float32)
    m, acc = hh.synth_masks(rng, N, B, F=500)
    dev = hh.dev()
    if fp8:
        E8, Q8 = fp8_ref.encode_e4m3(Ei), fp8_ref.encode_e4m3(Qi)
        es = (2.0 ** rng.integers(-3, 1, size=N)).astype(np.float32)
        qs = (2.0 ** rng.integers(-2, 2, size=B)).astype(np.float32)
        S = fp8_ref.scores_fp8(Q8, qs, E8, es)
        ops = tuple(torch.from_numpy(a).to(dev) for a in (Q8, qs, E8, es))
    else:
        S = Qi @ Ei.T  # exact: integers below 2^24
        ops = (torch.from_numpy(Qi).to(dev).to(torch.bfloat16), torch.from_numpy(Ei).to(dev).to(torch.bfloat16))
    want_i, want_s = common_ref.masked_topk(S, acc, depth)
    return ops, hh.masks_to_device(m, dev), want_i.astype(np.int32), want_s


def _first_page(fp8, ops, k, dm, flags):
    if fp8:
        return hh.sim_topk_fp8(*ops, k, dm, flags=flags, retry_dense=False)
    return hh.sim_topk(*ops, k, dm, flags=flags, retry_dense=False)


def _next_page(fp8, ops, k, dm, flags, after_score, after_id):
    if fp8:
        Q8, qs, E8, es = ops
        return hh.sim_topk_after(Q8, E8, k, after_score, after_id, dm, flags=flags, scales=(qs, es))
    return hh.sim_topk_after(*ops, k, after_score, after_id, dm, flags=flags)


class _options:
    def __init__(self, opts):
        self.opts, self.lib = opts, _lib.load()

    def __enter__(self):
        for n, v in self.opts.items():
            _lib.check(self.lib.rp_set_option(n.encode(), v), n)

    def __exit__(self, *exc):
        for n in self.opts:
            _lib.check(self.lib.rp_set_option(n.encode(), 0), n)  # (scan_impl and scan_force_new default to 0)


@pytest.mark.parametrize("tile,paged", PARAMS, ids=[f"{t}{'-paged' if p else ''}" for t, p in PARAMS])
def test_tile_alone_gives_the_oracle_ranking(tile, paged):
    which, fp8, B, D, k, opts = CASES[tile]
    (ops, dm, want_i, want_s) = _problem(fp8, B, D, 2 * k if paged else k)
    with _options(opts):
        plan = hh.sim_plan(B, N, D, k, _lib.RP_TOPK_AUTO, fp8, paged)
        assert plan[which] == tile and plan["paged_filter"] == paged, plan
        assert hh.sim_plan(B, N, D, k, _lib.RP_TOPK_DENSE, fp8, paged)["dense_only"] == 1
        for flags in (_lib.RP_TOPK_AUTO, _lib.RP_TOPK_DENSE):
            ids, sc, cnt = _first_page(fp8, ops, k, dm, flags)
            if paged:  # page 2 behind page 1's last entry = entries k .. 2k of the 2k-deep ranking
                assert np.array_equal(ids.cpu().numpy(), want_i[:, :k]) and np.array_equal(sc.cpu().numpy(), want_s[:, :k])
                ids, sc, cnt = _next_page(fp8, ops, k, dm, flags, sc[:, -1].contiguous(), ids[:, -1].contiguous())
            lo = k if paged else 0
            assert np.array_equal(ids.cpu().numpy(), want_i[:, lo:lo + k]), (tile, flags)
            assert np.array_equal(sc.cpu().numpy(), want_s[:, lo:lo + k]), (tile, flags)
            assert (cnt == k).all(), (tile, flags)


def test_the_cases_reach_every_tile():
    """No tile may be left out: the tiles the plan reports for this file's cases are the whole enum, and each filter tile is
    reached with and without paging."""
    reached = set()
    for tile, paged in PARAMS:
        which, fp8, B, D, k, opts = CASES[tile]
        with _options(opts):
            plan = hh.sim_plan(B, N, D, k, _lib.RP_TOPK_AUTO, fp8, paged)
        reached.add((plan[which], plan["paged_filter"]))
    assert {t for t, _ in reached} == set(_lib.SIM_TILES) and len(_lib.SIM_TILES) == 23
    assert {(t, p) for t in FILTER_TILES for p in (0, 1)} <= reached
