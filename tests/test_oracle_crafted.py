"""The oracle against the reference build on the crafted inputs: the adversarial builders that aim the GPU tests at each
kernel's switch points (tests/crafted_cases.py), where a restatement is most likely to drift from its original -- the table
halving, count()'s 16-bit squeeze, the rANS normaliser's steal loop, the far carry, find()'s fall-through past the table,
the unstable sort's row for long equal runs.  Every family's results are held to the digests the real reference build gave
(tests/golden/reference_crafted.json, made by tests/golden/make_golden_agreement.py) and, where oracle/_ref is present, to
the build itself.  tests/test_gpu_reference_digests.py holds the kernels to the same digests.
"""
import hashlib
import json

import numpy as np
import pytest

import adaptive_cases
import agreement_cases
import crafted_cases
import damaged_cases

FAMILIES = ("carry", "static", "rans", "bwt", "adaptive", "damaged", "truncations", "halving")


@pytest.mark.parametrize("family", FAMILIES)
def test_family_against_reference_build(oracle, reference, family):
    live = reference is not None and reference.ans is not None and reference.bwt is not None
    run = agreement_cases.CRAFTED[family]
    agreement_cases.agree(agreement_cases.stored_crafted(family), run(oracle), run(reference) if live else None)


def test_the_fixture_holds_the_registry_of_today(oracle):
    """Every key a device call can rebuild is a case the registry yields today, and the other way round: a builder whose
    output drifts (a case that comes or goes, a seed that finds no run any more) is noticed here, and its bytes by the
    digests above.  The fixture has the registry's families and no others."""
    with open(agreement_cases.STORED_CRAFTED) as f:
        fixture = json.load(f)
    assert set(fixture) - {"generator", "source"} == set(crafted_cases.FAMILIES) == set(FAMILIES) == set(agreement_cases.CRAFTED)
    for family in FAMILIES:
        today = crafted_cases.keys(family)
        assert len(set(today)) == len(today), family
        assert {k for k in fixture[family] if agreement_cases.device_key(k)} == set(today), family
        assert all(k.startswith(family + "/") for k in fixture[family]), family


# the crafted builders the GPU tests use, by the registry's family: written out here, not read from the test files
USED_BY_THE_GPU_TESTS = {
    "carry": ("carry_runs.carry_run_block", "carry_runs.carry_run_block_static"),
    "static": ("static_cases.squeeze_ladder", "static_cases.natural_block", "static_cases.natural_stream",
               "static_cases.crafted_blocks", "static_cases.aimed_streams"),
    "rans": ("rans_cases.block_cases", "rans_cases.victim_cases", "rans_cases.tie_counts", "rans_cases.singletons",
             "rans_cases.dense_rare", "rans_cases.one_symbol", "rans_cases.all_256", "rans_cases.rare_item"),
    "bwt": ("bwt_cases.open_ladder", "bwt_cases.runny_ladder", "bwt_cases.run_key_cases", "bwt_cases.aligned_runs",
            "bwt_cases.tied_runs", "bwt_cases.planted", "bwt_cases.periodic", "bwt_inverse_cases.all_cases"),
    "adaptive": ("adaptive_cases.pass_burst_blocks", "adaptive_cases.long_burst_block", "adaptive_cases.one_value_block",
                 "adaptive_cases.level3_block"),
    "damaged": ("adaptive_walk.past_the_table", "damaged_cases.build"),
    "truncations": ("damaged_cases.build",),
    "halving": ("golden_cases.LONG_ADAPTIVE", "resumable_cases.loop_input", "resumable_cases.backlog_input", "resumable_cases.carry_input"),
}


def test_every_family_the_gpu_tests_use_is_in_the_registry():
    import importlib
    assert crafted_cases.BUILDERS == USED_BY_THE_GPU_TESTS
    for family, names in USED_BY_THE_GPU_TESTS.items():
        assert family in crafted_cases.FAMILIES
        for name in names:
            module, attr = name.split(".")
            assert hasattr(importlib.import_module(module), attr), name
    # and what the registry takes from them is there: some cases of every builder's key in the family
    for family, word in (("carry", "static run"), ("static", "/ladder/"), ("static", "/natural block"), ("static", "/natural stream"), ("static", "/crafted/"),
                         ("static", "/aimed/"), ("rans", "victims, lane"), ("rans", "victims, tie"), ("rans", "singletons"),
                         ("rans", "dense_rare"), ("rans", "one_symbol"), ("rans", "all_256"), ("rans", "rare_item"),
                         ("bwt", "open_ladder"), ("bwt", "runny_ladder"), ("bwt", "run keys/aligned runs"), ("bwt", "run keys/tied runs"),
                         ("bwt", "planted"), ("bwt", "periodic/"), ("bwt", "/inverse/"), ("adaptive", "pass burst"),
                         ("adaptive", "long burst"), ("adaptive", "one value"), ("adaptive", "level 3"),
                         ("damaged", "past the table/first_pass"), ("damaged", "past the table/late_pass"), ("damaged", "run of 0xFF"),
                         ("truncations", "cut by 16"), ("halving", "carry_input")):
        assert any(word in k for k in agreement_cases.stored_crafted(family)), (family, word)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


# sha256 of what each builder made while it still stood in its GPU test file (test_gpu_dec_pass64, test_gpu_parity,
# test_gpu_dec_borrow_words, test_gpu_enc_seven_waves), and of the streams of gpu_support.build() before it moved
MOVED = {
    "pass_burst_blocks(1)": "665688cd00b494ff7c495b31592bc5e1d41d57a242578fbcc26e469a467c550f",
    "pass_burst_blocks(2)": "74f88959da3288e814cdda1ce0853532958b72e9a41551db22c4bb74ae421ca9",
    "pass_burst_blocks(3)": "a5152d8f4f97745848f9d7593be9b1b26cd736284cf679d982ff4b9dd0d4d19e",
    "long_bursts()": "66112d78711829f1178b482f3df531769537871e61fddc5ee6b93534f4f1d6e6",
    "one_value_block(0)": "8a39d2abd3999ab73c34db2476849cddf303ce389b35826850f9a700589b4a90",
    "one_value_block(255)": "3b874d3ba46c638fc3094f8e92fb744ca974893873f8885f54e23760f9b6311b",
    "level3_block('all 0')": "de2f256064a0af797747c2b97505dc0b9f3df0de4f489eac731c23ae9ca9cc31",
    "level3_block('all 255')": "71189f7fb6aed638640078fba3a35fda6c39c8962e74dcc75935aac948da9063",
    "level3_block('0 then 255')": "03d58aa571ff86196650f01a03269a9a7e1a3751356f0b577b6e19bc0a9af11a",
    "build(coder 0)": "d7c3113b2d21df8876c5a1cd9b3a0d9223dd29e3711711f94ed4e1a959668ba7",
    "build(coder 1)": "cbb094c9bf31e6b02aec82b79c79a2edaae3d36faa5f9cc01c76b5e3b43a6d9e",
    "build(coder 2)": "8b040449708e5c89b81fc168d0372d4cc46cf672658795abafec86c3216b65d3",
    "build(coder 3)": "99c0e4718d60b0767b388d3ed666f18305411c7672bd366f0089304ade4a4227",
}


def test_the_moved_builders_make_the_bytes_they_made(oracle):
    got = {f"pass_burst_blocks({g})": sha(np.concatenate(adaptive_cases.pass_burst_blocks(g))) for g in adaptive_cases.PASS_BURST_GROUPS}
    got["long_bursts()"] = sha(adaptive_cases.long_bursts())
    got.update({f"one_value_block({b})": sha(adaptive_cases.one_value_block(b)) for b in adaptive_cases.ONE_VALUE_BYTES})
    got.update({f"level3_block({c!r})": sha(adaptive_cases.level3_block(c)) for c in adaptive_cases.LEVEL3_CASES})
    got.update({f"build(coder {c})": sha(damaged_cases.build(oracle, c, 4096, 100, 100 + c).streams()[0]) for c in range(4)})
    assert got == MOVED
    assert adaptive_cases.PASS_LENGTHS == (48, 64, 80, 112, 128, 129, 191, 192, 375) and adaptive_cases.ALL_THREE == 375
    assert (adaptive_cases.PASS_BLOCK, adaptive_cases.ONE_VALUE_N, adaptive_cases.LONG_BURST_BLOCK) == (4096, 1 << 18, 1 << 20)
