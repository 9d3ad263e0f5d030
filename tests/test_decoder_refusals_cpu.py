"""Every refusal of the decoder file's entry points that take no decoder handle, call for call (no GPU): the calls of
tests/golden/make_golden_decoder_refusals.py's ``cpu`` section are made again and their statuses and ``rp_last_error``
texts - and the accepted sizes of ``rp_beam_books_bytes`` - must equal fixture G29, which was recorded before the entry
points were folded onto one list check.  Every call is a refusal, so nothing is launched."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_decoder_refusals import G29_FILE, record_cpu  # noqa: E402


@pytest.fixture(scope="module")
def tables(hip_lib, golden_dir):
    with open(os.path.join(golden_dir, G29_FILE)) as fh:
        want = json.load(fh)["cpu"]
    return record_cpu(hip_lib), want


def test_every_call_of_the_fixture_is_made(tables):
    got, want = tables
    assert sorted(got) == sorted(want) and len(want) == 479


def test_every_refusal_keeps_its_status_and_text(tables):
    got, want = tables
    differing = [key for key in want if got.get(key) != want[key]]
    for key in differing:
        print(f"{key}: got {got.get(key)!r}, recorded {want[key]!r}")
    assert not differing
