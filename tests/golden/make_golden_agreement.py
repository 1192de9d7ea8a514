#!/usr/bin/env python3
"""Generate tests/golden/reference_agreement.json from the REAL reference build: a digest of every result of the checks in
tests/agreement_cases.py (range coders, rANS, block sort, damaged streams), so that the tests that compare the oracle with the reference
build run where oracle/_ref/ is not present too; and tests/golden/reference_crafted.json, the same for the crafted families
of tests/crafted_cases.py (agreement_cases.CRAFTED), which tests/test_oracle_crafted.py holds the oracle to and
tests/test_gpu_reference_digests.py the kernels.  Runs only where oracle/_ref/ was built (`make -C oracle ref`, see
make_golden.py).  Outputs are data: digests of the reference's outputs.

    python tests/golden/make_golden_agreement.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agreement_cases  # noqa: E402
import bwt_cases  # noqa: E402
import oracle_lib  # noqa: E402


def main() -> None:
    oracle_lib.build_oracle()
    ref = oracle_lib.reference()
    if ref is None or ref.ans is None or ref.bwt is None:
        raise SystemExit("oracle/_ref/ (libcpprcoder_ref.so, libcppans_ref.so, libblksort_ref.so) missing: run `make -C oracle ref`")
    out = {"generator": "tests/golden/make_golden_agreement.py",
           "source": "oracle/_ref/ (the unmodified reference headers compiled by `make -C oracle ref`)",
           "adaptive": {k: agreement_cases.digest(r) for k, r in agreement_cases.adaptive(ref)},
           "rans": {k: agreement_cases.digest(r) for k, r in agreement_cases.rans(ref)},
           "bwt": {k: agreement_cases.digest(r) for k, r in agreement_cases.bwt(ref, bwt_cases.cases())},
           "damaged": {k: agreement_cases.digest(r) for k, r in agreement_cases.damaged(ref)}}
    for part in ("adaptive", "rans", "bwt", "damaged"):
        print(part, len(out[part]), "results", flush=True)
    with open(os.path.join(HERE, "reference_agreement.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    # the crafted families (tests/crafted_cases.py), in a fixture of their own so that the one above stays as it is
    crafted = {"generator": out["generator"], "source": out["source"]}
    for family, run in agreement_cases.CRAFTED.items():
        crafted[family] = {k: agreement_cases.digest(r) for k, r in run(ref)}
        print("crafted", family, len(crafted[family]), "results", flush=True)
    with open(os.path.join(HERE, "reference_crafted.json"), "w") as f:
        json.dump(crafted, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
