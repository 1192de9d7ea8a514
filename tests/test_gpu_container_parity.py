"""The container layer on the GPU against tests/golden/container_parity.json: for every case of
tests/container_parity_cases.gpu_cases() the SHA-256 and length of each blob, what damaged containers report, and -- per public
call -- the ordered names of the rcx.Context methods and module device calls it made, and of its uploads and downloads, are the
ones recorded at the commit the fixture names; each case also checks that unpack returns what was packed.  The same calls in the same order with the same
number of syncs is the speed check of this layer: bench.py does not reach it."""
import json
import os

import pytest

import container_parity_cases as cases
from gpu_support import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.gpu_cases()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "container_parity.json")) as f:
        return json.load(f)["gpu"]


def test_every_case_is_recorded(golden):
    assert len(golden["commit"]) >= 7 and sorted(golden["cases"]) == sorted(CASES)
    reported = {(v[-1][1]["kind"], name.split()[0]) for name, rec in golden["cases"].items() for key, v in rec.get("values", {}).items()
                if key.startswith("damaged") and isinstance(v[-1][1], dict) and v[-1][1]["error"] == "ChecksumError"}
    assert {("block", "RCXB"), ("item", "RCXI"), ("block", "RCXT"), ("item", "RCXJ"), ("item", "tensors"), ("block", "RCXD"), ("item", "RCXK"),
            ("item", "tensors-delta"), ("item", "open_items"), ("item", "open_typed_items")} <= reported
    wrong = [v["error"] for rec in golden["cases"].values() for key, v in rec.get("values", {}).items() if key == "wrong base" and isinstance(v, dict)]
    wrong += [v[1]["error"] for rec in golden["cases"].values() for key, v in rec.get("values", {}).items() if key == "wrong base" and isinstance(v, list) and isinstance(v[1], dict)]
    assert "BaseMismatchError" in wrong and "BaseItemMismatchError" in wrong


@pytest.mark.parametrize("name", list(CASES))
def test_blobs_and_call_traces_are_the_recorded_ones(ctx, golden, monkeypatch, name):
    got = json.loads(json.dumps(cases.run_gpu_case(CASES[name], ctx, monkeypatch.setattr)))
    want = golden["cases"][name]
    assert got["blobs"] == want["blobs"]
    assert got.get("values") == want.get("values")
    assert sorted(got["traces"]) == sorted(want["traces"])
    for label, trace in want["traces"].items():
        assert got["traces"][label] == trace, (name, label)
    assert sorted(got["copies"]) == sorted(want["copies"])
    for label, moved in want["copies"].items():
        assert got["copies"][label] == moved, (name, label)
