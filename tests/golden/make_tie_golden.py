#!/usr/bin/env python3
"""Generate tests/golden/tie_classes.json by running the REFERENCE implementation on the tie-class cases of
tests/tie_classes.py: every unscaled case of BASE, ZERO, INT8_LARGE and INT8_126, and two scaled BASE cases per
traceback word width (cost tables and gap open cost times k).

Like make_general_golden.py this script is the only place that executes the reference (iamgiddyaboutgit/globalign,
found as make_golden.py finds it); it writes plain JSON data only:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_tie_golden.py

Reference entry points exercised (paths relative to the reference's root):
  * make_dp_array / dp_array_forward / dp_array_backward   src/globalign/globaligner.py:756-821, 366-392, 395-593
Each record holds the case, the factor k, the seed given to random.seed (tie_classes.case_seed), the status, the
cost, a digest of the three strings (tests/conftest.py aln_digest) and a digest of random.getstate() afterwards.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import _import_reference, aln_digest  # noqa: E402
from make_general_golden import run_case  # noqa: E402
from tests import tie_classes as tc  # noqa: E402


def golden_cases():
    """[(case, k)]: the unscaled lists, then per width the first two BASE cases whose factor is not 1."""
    out = [(c, 1) for c in tc.BASE + tc.ZERO + tc.INT8_LARGE + tc.INT8_126]
    for width in tc.WIDTHS:
        out += [(c, k) for c, k in tc.width_cases(width) if k != 1 and k == tc.FACTORS[c[2]][width][-1]][:2]
    return out


def main():
    ga, start, _ = _import_reference()
    out = []
    for case, k in golden_cases():
        cmat, s1, s2, o = tc.scaled_problem(case, k)
        rec = run_case(ga, start, s1, s2, cmat, o, tc.case_seed(case))
        assert rec["status"] == "ok"
        out.append({"case": list(case), "k": k, "seed": rec["seed"], "status": rec["status"], "cost": rec["cost"],
                    "aln_sha16": aln_digest(*rec["strings"]), "state_after": rec["state_after"]})
        print(len(out), case, k, rec["cost"], flush=True)
    with open(os.path.join(HERE, "tie_classes.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
