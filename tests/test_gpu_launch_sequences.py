"""GPU: the codec and the training step call the library's entry points in the recorded order
(tests/golden/launch_sequences.json, written by tests/golden/make_launch_sequences.py from the slice loops as they stood
before they shared their prologue, their per-slice coding step and the quantiser object): compress + decompress without
a step, with a step and with a quality map, cnn and stf, both forms of the slice loop; a training step of cnn, stf (both
forms) and stf6."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_launch_sequences", os.path.join(GOLDEN, "make_launch_sequences.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def recorded():
    with open(G.FIXTURE) as fh:
        f = json.load(fh)
    return {cid: [f["names"][i] for i in idx] for cid, idx in f["cases"].items()}


@pytest.fixture(scope="module")
def nets():
    return {}


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c["id"] for c in G.CASES) and all(recorded.values())


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_launch_sequence_is_the_recorded_one(case, recorded, nets, monkeypatch):
    want = recorded[case["id"]]
    got = G.sequence(case, nets, monkeypatch.setattr)
    same = got == want          # (a bare assert on the two lists would print thousands of names)
    if not same:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        lo = max(0, at - 4)
        print(f"{case['id']}: {len(got)} calls, recorded {len(want)}; first difference at call {at}")
        print("  recorded:", want[lo:at], ">>", want[at:at + 5])
        print("  got:     ", got[lo:at], ">>", got[at:at + 5])
    assert same, f"{case['id']}: the sequence of library calls differs from the recorded one"
