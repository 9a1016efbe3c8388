#!/usr/bin/env python3
"""Generate tests/golden/path_geometry.json by running the REFERENCE implementation on the path-geometry cases of
tests/path_geometry.py (path_geometry.golden_cases()): every list entry under 4 * 10^5 cells at one-byte traceback
words, the first entry of every list whatever its size, the first two RUNS and ARRIVE entries at two- and four-byte
words, and the ARRIVE entries under the "gap8" table that the int8 lists run at four-byte words.

Left out (the reference is pure Python, about 1.4 * 10^6 cells a second): the list entries of 4 * 10^5 cells and more
other than each list's first -- the second RC_RUNS entry, the COUNT entries from D = 1023 up, and the SLABS entries
after the first.

Like make_tie_golden.py this script is the only place that executes the reference (iamgiddyaboutgit/globalign, found
as make_golden.py finds it); it writes plain JSON data only:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_path_golden.py

Reference entry points exercised (paths relative to the reference's root):
  * make_dp_array / dp_array_forward / dp_array_backward   src/globalign/globaligner.py:756-821, 366-392, 395-593
Each record holds the case, the seed given to random.seed (path_geometry.case_seed), the status, the cost, a digest of
the three strings (tests/conftest.py aln_digest) and a digest of random.getstate() afterwards.
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
from tests import path_geometry as pg  # noqa: E402


def main():
    ga, start, _ = _import_reference()
    out = []
    for case in pg.golden_cases():
        cmat, s1, s2, o = pg.problem(case)
        rec = run_case(ga, start, s1, s2, cmat, o, pg.case_seed(case))
        assert rec["status"] == "ok"
        out.append({"case": [list(case[0]), [list(seg) for seg in case[1]], case[2]], "seed": rec["seed"],
                    "status": rec["status"], "cost": rec["cost"], "aln_sha16": aln_digest(*rec["strings"]),
                    "state_after": rec["state_after"]})
        print(len(out), case, rec["cost"], flush=True)
    with open(os.path.join(HERE, "path_geometry.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
