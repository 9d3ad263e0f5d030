"""The workspace-hygiene harness (tests/hip_helpers.py: Arena, hygiene_findings) on CPU tensors: a toy entry point written
in torch, run clean and with one planted error at a time.  The harness must pass the clean form and name every planted
one - what tests/test_workspace_hygiene_gpu.py relies on when it reports no finding for a HIP entry point."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hip_helpers import (GUARD_BYTE, MIN_GUARD, OUTPUT_BYTE, RP_E_WORKSPACE, WS_FILLS, Arena, guard_bytes,  # noqa: E402
                         hygiene_findings)

N = 37  # elements of the toy's input and output


def _f32(arena, byte_offset, n):
    return arena.at(byte_offset, 4 * n).view(torch.float32)


def toy_workspace_bytes(n):
    return 4 * n


def toy(x, ws, out, n, ws_bytes, plant=None, counter=None):
    """out[i] = 2 x[i] + 1 through a workspace array tmp [n] (the ABI's conventions: pointers, a workspace size, a
    status).  ``plant``: the one error this run commits."""
    if plant != "ignores_workspace_bytes" and ws_bytes < toy_workspace_bytes(n):
        return RP_E_WORKSPACE
    tmp = _f32(ws, 0, n)
    written = n - 1 if plant == "reads_unwritten_workspace" else n
    tmp[:written] = 2.0 * _f32(x, 0, n)[:written]
    _f32(out, 0, n).copy_(tmp + 1.0)
    if plant == "stores_past_output":
        _f32(out, 4 * n, 1)[0] = 1.0
    if plant == "stores_before_workspace":
        _f32(ws, -4, 1)[0] = 1.0
    if plant == "reads_past_input":
        _f32(out, 4 * (n - 1), 1)[0] += _f32(x, 4 * n, 1)[0]
    if plant == "not_deterministic":
        _f32(out, 0, 1)[0] += float(next(counter))
    return 0


def _findings(plant=None):
    guard = guard_bytes()
    x = Arena.of("x", torch.linspace(-3.0, 3.0, N), guard)
    ws = Arena("workspace", toy_workspace_bytes(N), guard, "cpu")
    out = Arena("out", 4 * N, guard, "cpu", dtype=torch.float32)
    counter = itertools.count()
    results = {}
    found = hygiene_findings(lambda nbytes: toy(x, ws, out, N, nbytes, plant, counter), ws, [out], [x], results=results)
    return found, results


def test_arena_layout():
    assert guard_bytes() == MIN_GUARD == 1 << 20
    assert guard_bytes(3584) == 256 * 2 * 3584 * 4 > MIN_GUARD  # ByT5-small: one 256-row tile of fp32 gate | up rows
    a = Arena("a", 100, 4096, "cpu")
    assert a.ptr % 256 == 0 and a.off >= 4096 and a.raw.numel() - a.off - a.nbytes >= 4096
    assert a.broken_guards() == [] and bool((a.payload() == OUTPUT_BYTE).all()) and a.at_rest()
    a.at(100, 1).fill_(0)  # the first byte behind the payload
    assert a.broken_guards() == ["tail"]
    a.at(100, 1).fill_(GUARD_BYTE)
    a.at(-1, 1).fill_(0)
    assert a.broken_guards() == ["lead"]
    a.view(dtype=torch.int32)[3] = 9
    assert not a.at_rest()
    t = torch.arange(6, dtype=torch.int64)
    b = Arena.of("b", t, 4096)
    assert b.nbytes == 48 and torch.equal(b.view(2, 3), t.view(2, 3))
    b.view()[0] = -1
    b.reset()
    assert torch.equal(b.view(), t)
    b.set_tail(0xFF)  # an input's tail takes other fills and is checked against the fill it holds
    assert b.broken_guards() == []
    nan = Arena("nan", 8, 4096, "cpu", init=0xFF, dtype=torch.float32)
    assert torch.isnan(nan.view()).all() and nan.at_rest()  # bytes are compared: NaN payloads are equal to themselves


def test_clean_toy_passes():
    found, results = _findings()
    assert found == []
    assert torch.equal(results["out"], 2.0 * torch.linspace(-3.0, 3.0, N) + 1.0)
    assert WS_FILLS == (0x00, 0xFF, 0x7F)


@pytest.mark.parametrize("plant, names", [
    ("stores_past_output", ["guard out tail"]),
    ("stores_before_workspace", ["guard workspace lead"]),
    ("reads_unwritten_workspace", ["stale workspace: output out differs with the workspace filled with 0xFF",
                                   "stale workspace: output out differs with the workspace filled with 0x7F"]),
    ("reads_past_input", ["input tail: output out differs"]),
])
def test_planted_error_is_flagged_by_name(plant, names):
    found, _ = _findings(plant)
    for name in names:
        assert any(f.startswith(name) for f in found), (plant, found)
    kinds = {f.split(":")[0].split(" ")[0] for f in found}  # nothing else is reported beside the planted error
    assert kinds == {names[0].split(":")[0].split(" ")[0]}, found


def test_stale_read_names_the_first_differing_element():
    found, _ = _findings("reads_unwritten_workspace")
    assert all(f"first differing element {N - 1} " in f for f in found), found


def test_undersized_and_irreproducible_calls_are_flagged():
    found, _ = _findings("ignores_workspace_bytes")
    assert any(f.startswith("undersized: workspace_bytes - 1 returned 0") for f in found), found
    assert any(f.startswith("undersized: the refused call wrote to output out") for f in found), found
    found, _ = _findings("not_deterministic")
    assert len(found) == 1 and found[0].startswith("not reproducible: output out"), found


def test_outputs_outside_the_contract_are_guarded_not_compared():
    guard = guard_bytes()
    ws = Arena("workspace", 4, guard, "cpu")
    free = Arena("free", 4, guard, "cpu", dtype=torch.int32, compare=False)
    counter = itertools.count()

    def call(nbytes):
        if nbytes < 4:
            return RP_E_WORKSPACE
        free.view()[0] = next(counter)
        return 0

    assert hygiene_findings(call, ws, [free]) == []
