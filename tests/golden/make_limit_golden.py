#!/usr/bin/env python3
"""Generate tests/golden/limit_costs.json by running the REFERENCE implementation under the cost tables of
tests/limit_costs.py: the families that sit on the host checks' limits (sub' at +-127 / +-128 / +-32767, alphabets of
33 and 64 keys, tables scaled to the largest factor the int32 range guard admits, gap open 32766).

Like make_general_golden.py this script is the only place that executes the reference (iamgiddyaboutgit/globalign,
found as make_golden.py finds it); it writes plain JSON data only:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_limit_golden.py

Reference entry points exercised (paths relative to the reference's root):
  * make_dp_array / dp_array_forward / dp_array_backward   src/globalign/globaligner.py:756-821, 366-392, 395-593
The reference computes with Python's unbounded ints; the oracle's int64 must agree with it at magnitudes of 2^26.
Each case records its inputs, the costing dict, the factor of a scaled family, the seed given to random.seed, the
status ("ok" or "IndexError", the reference's degenerate-length quirk), the cost, the three strings and a digest of
random.getstate() afterwards.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import _import_reference  # noqa: E402
from make_general_golden import run_case  # noqa: E402
from tests import limit_costs as lc  # noqa: E402

FAMILIES = [lc.P8, lc.P8A, lc.P8B, lc.P16, lc.K_(33), lc.K_(64), lc.V16, lc.VPHI, lc.VNEG]
GAP_OPENS = [6, 126, lc.O_MAX, 0, 127]
PER_FAMILY = 4


def main():
    ga, start, _ = _import_reference()
    rng = random.Random(20261021)  # private generator: never touches the global one
    cases = []
    for fi, fam in enumerate(FAMILIES):
        for k in range(PER_FAMILY):
            m, n = rng.randint(4, 140), rng.randint(4, 140)
            if k == 0:
                m, n = 140, 139 - fi
            cases.append(fam + (m, n, GAP_OPENS[(k + fi) % len(GAP_OPENS)]))
    # one letter against a few at the largest gap open: where the reference's walk raises IndexError
    cases += [lc.V16 + (1, 6, lc.O_MAX), lc.VPHI + (5, 1, lc.O_MAX), lc.P8 + (1, 4, lc.O_MAX), lc.VNEG + (1, 1, lc.O_MAX),
              lc.K_(33) + (7, 1, lc.O_MAX)]
    out = []
    for case in cases:
        cmat, s1, s2, o = lc.problem(case)
        rec = run_case(ga, start, s1, s2, cmat, o, rng.randint(0, 2 ** 31 - 1))
        rec.update(family=case[0], variant=case[1])
        if lc.is_v(case):
            rec["factor"] = lc.v_factor(case[0], case[2], case[3], o)
        out.append(rec)
    with open(os.path.join(HERE, "limit_costs.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", len(out), "cases;", sum(c["status"] != "ok" for c in out), "IndexError")


if __name__ == "__main__":
    main()
