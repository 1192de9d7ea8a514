"""The container layer against tests/golden/container_parity.json, as far as it goes without a GPU: the fixture was written by
tests/golden/make_golden_containers.py at the commit it names, from tests/container_parity_cases.py, and the same functions
run here must give the same -- header bytes and refusals of the four writers, the verdict of the four parsers on every
damaged form of a valid blob (which pins the order of their checks), the tensor directory, and what pack and unpack return
where there is nothing to code.  Also what the split into layout.py and container.py promises by itself."""
import json
import os
import subprocess
import sys

import pytest

import container_parity_cases as cases
from cpprcoder_amd import container, layout, stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "container_parity.json")) as f:
        return json.load(f)["cpu"]


@pytest.fixture(scope="module")
def replay():
    return json.loads(json.dumps(cases.cpu_section()))  # (through JSON, as the fixture went)


def test_the_fixture_covers_what_it_should(golden):
    assert len(golden["commit"]) >= 7
    sections = golden["sections"]
    headers = sections["headers"]
    for layout_name in cases.FIXED:
        ok = [k for k, v in headers.items() if k.startswith(layout_name) and "ok" in v]
        refused = [k for k, v in headers.items() if k.startswith(layout_name) and "error" in v]
        assert len(ok) >= 5 and len(refused) >= 3, layout_name
        blobs = [v for k, v in sections["parsers"].items() if k.startswith(layout_name)]
        assert len(blobs) >= 2 and all("parsed" in b["verdicts"] for b in blobs)
    for name, rec in sections["parsers"].items():
        blob = bytes.fromhex(rec["blob"])
        whats = [w for w, _ in rec["damaged"]]
        fixed = cases.FIXED[name[:4]]
        assert all(f"byte {at} {how}" in whats for at in range(fixed) for how in ("=00", "=ff", "+1")), name
        cuts = [int(w.split()[-1]) for w in whats if w.startswith("cut at ")]
        assert cuts == list(range(len(cuts))) and len(cuts) > fixed + 8 and "one byte more" in whats and len(blob) >= len(cuts) - 1, name


@pytest.mark.parametrize("section", ("constants", "coded_size", "pick_predictor", "errors", "headers", "directory", "no_gpu", "decisions", "names"))
def test_section_is_the_recorded_one(golden, replay, section):
    want, got = golden["sections"][section], replay[section]
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key] == want[key], (section, key)
    assert got == want


@pytest.mark.parametrize("name", sorted(cases.valid_blobs()))
def test_parser_verdicts_are_the_recorded_ones(golden, replay, name):
    want, got = golden["sections"]["parsers"][name], replay["parsers"][name]
    assert got["blob"] == want["blob"] and got["parsed"] == want["parsed"] and got["as_array"] == want["as_array"] and got["foreign"] == want["foreign"]
    assert len(got["damaged"]) == len(want["damaged"])
    for (what, g), (what_, w) in zip(got["damaged"], want["damaged"]):
        assert what == what_ and got["verdicts"][g] == want["verdicts"][w], (name, what)


def test_container_re_exports_the_layouts():
    names = ("MAGIC", "VERSION", "VERSION_CRC", "VERSION_STORED", "FLAG_BLKSORT", "FLAG_CRC32", "FLAG_STORED", "ITEM_MAGIC", "ITEM_VERSION", "MAX_ITEM",
             "TYPED_MAGIC", "TYPED_VERSION", "TYPED_VERSION_PRED", "TYPED_VERSION_STORED", "PREDICTORS", "WIDTHS", "TYPED_ITEMS_MAGIC", "TYPED_ITEMS_VERSION",
             "ITEM_WIDTHS", "coded_size", "ContainerError", "ChecksumError", "header_bytes", "parse", "item_header_bytes", "parse_items", "typed_header_bytes",
             "parse_typed", "typed_items_header_bytes", "parse_typed_items", "tensor_directory_bytes", "parse_tensor_directory",
             "DELTA_MAGIC", "DELTA_VERSION", "DELTA_FLAG_BASE_CRC", "BASE_OPS", "BaseMismatchError", "delta_header_bytes", "parse_delta",
             "DELTA_ITEMS_MAGIC", "DELTA_ITEMS_VERSION", "DELTA_ITEMS_FLAG_BASE_CRC", "BASE_OP_NONE", "BaseItemMismatchError", "delta_items_header_bytes",
             "parse_delta_items", "TYPED_ITEMS_VERSION_STORED", "block_lengths")
    for name in names:
        assert getattr(container, name) is getattr(layout, name), name
    assert stored.block_lengths is layout.block_lengths and list(stored.block_lengths(40, 16)) == [16, 16, 8] and len(stored.block_lengths(0, 16)) == 0


def test_imports_stay_lazy():
    """layout is numpy only; container imports neither torch nor the binding, and loads no library, until a call needs them."""
    code = ("import sys\n"
            "import cpprcoder_amd.layout\n"
            "assert not [m for m in sys.modules if m == 'torch' or m.startswith('cpprcoder_amd.') and m != 'cpprcoder_amd.layout'], sorted(sys.modules)\n"
            "import cpprcoder_amd.container, cpprcoder_amd.stored\n"
            "assert 'torch' not in sys.modules\n"
            "from cpprcoder_amd import rcx\n"
            "assert rcx._lib is None\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
