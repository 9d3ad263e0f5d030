"""The generation drivers call for call (no GPU): every search function and pool of ``reprover_amd.generation`` is run
again over the scripted model of tests/golden/make_golden_gen_calls.py and the calls it made of its callables - names,
order, ``active`` / ``pos`` / ``t`` and their presence, list arguments, tensor dtypes and shapes, ``to_host`` shapes, the
tickets every pool ``step`` returned - must equal fixture G28, which was recorded before the drivers were folded onto one
slot scheduler and one host step body.  The outputs and the copy counts are the other generation tests' business."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_gen_calls import G28_FILE, record  # noqa: E402


@pytest.fixture(scope="module")
def traces(hip_lib, golden_dir):
    with open(os.path.join(golden_dir, G28_FILE)) as fh:
        want = json.load(fh)
    return record(hip_lib), want


def test_every_driver_of_the_fixture_is_recorded(traces):
    got, want = traces
    assert sorted(got) == sorted(want) and len(want) == 32


def test_every_driver_makes_the_recorded_calls(traces):
    got, want = traces
    differing = [name for name in want if got[name] != want[name]]
    for name in differing:  # the first difference of each case, for the report
        for j, (g, w) in enumerate(zip(got[name] + [None], want[name] + [None])):
            if g != w:
                print(f"{name}: call {j}: got {g!r}, recorded {w!r}")
                break
    assert not differing
