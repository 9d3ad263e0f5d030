"""Every refusal of the decoder entry points that need a handle, call for call, on the MI355X: the calls of
tests/golden/make_golden_decoder_refusals.py's ``gpu`` section (``tiny`` configuration, 3 slots, 4 beams, ``max_len`` 8,
``src_cap`` 16) are made again; statuses, ``rp_last_error`` texts and the accepted workspace sizes must equal fixture G29,
recorded before the entry points were folded, and after every refused call the workspace and every output buffer still
hold their fill pattern: nothing was launched.  One accepted call per entry closes the run."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_decoder_refusals import FILL_BYTE, FILL_F32, G29_FILE, NB, record_gpu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(hip_lib, golden_dir):
    with open(os.path.join(golden_dir, G29_FILE)) as fh:
        want = json.load(fh)["gpu"]
    touched, accepted = [], {}

    def after(key, bufs):
        for name, t in bufs.items():
            if not bool((t == (FILL_BYTE if t.dtype == torch.uint8 else FILL_F32)).all()):
                touched.append((key, name))

    def ok(name, bufs):  # a step's rows hold log-probs, the rows behind them the fill; then the fill again for the next entry
        lp, rows = bufs["lp"], NB if name == "rp_decoder_step" else 2 * NB
        accepted[name] = bool(torch.isfinite(lp[:rows]).all()) and bool((lp[:rows] <= 0).all()) and bool((lp[rows:] == FILL_F32).all())
        lp.fill_(FILL_F32)

    return record_gpu(hip_lib, after, ok), want, touched, accepted


def test_every_call_of_the_fixture_is_made(tables):
    got, want, _, _ = tables
    assert sorted(got) == sorted(want) and len(want) == 501


def test_every_refusal_keeps_its_status_and_text(tables):
    got, want, _, _ = tables
    differing = [key for key in want if got.get(key) != want[key]]
    for key in differing:
        print(f"{key}: got {got.get(key)!r}, recorded {want[key]!r}")
    assert not differing


def test_no_refused_call_launches_anything(tables):
    assert tables[2] == []


def test_every_entry_accepts_its_plain_call(tables):
    got, _, _, accepted = tables
    plain = {key: v for key, v in got.items() if key.endswith("()") and "workspace_bytes" not in key}
    assert len(plain) == 12 and all(v == [0, ""] for v in plain.values()), plain
    # the three steps wrote log-probs over the fill
    assert accepted["rp_decoder_batch_step"] and accepted["rp_decoder_batch_step_pos"] and accepted["rp_decoder_pool_step"]
    assert accepted["rp_decoder_step"]
