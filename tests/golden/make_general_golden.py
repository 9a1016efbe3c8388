#!/usr/bin/env python3
"""Generate tests/golden/general_costs.json by running the REFERENCE implementation under letter-dependent,
asymmetric cost tables (the families of tests/general_costs.py: G general int8, W wide and signed, S a score
matrix file with a gap score per letter).

Like make_golden.py this script is the only place that executes the reference (iamgiddyaboutgit/globalign,
mounted read-only at /root/reference in the build container); it writes plain JSON data only:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_general_golden.py

Reference entry points exercised (paths relative to /root/reference):
  * make_dp_array / dp_array_forward / dp_array_backward   src/globalign/globaligner.py:756-821, 366-392, 395-593
  * validate_and_transform_args (family S: the .mtx reader and score -> cost transform)   src/globalign/start.py:150-353
Each case records its inputs, the costing dict, the seed given to random.seed, the status ("ok" or "IndexError",
the reference's degenerate-length quirk), the cost, the three strings and a digest of random.getstate() afterwards.
"""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import _import_reference, state_digest  # noqa: E402
from tests import general_costs as gc  # noqa: E402

GAP_OPENS = [0, 1, 6, 7, 20, 127, 300]
PER_FAMILY = 20


def run_case(ga, start, s1, s2, cmat, o, seed):
    max_cost = start.get_max_val(cmat)
    dp = ga.make_dp_array(seq_1=s1, seq_2=s2, costing_mat=cmat, max_cost=max_cost, gap_open_cost=o)
    ga.dp_array_forward(dp_array=dp, seq_1=s1, seq_2=s2, costing_mat=cmat, gap_open_cost=o)
    rec = {"seq_1": s1, "seq_2": s2, "costing_mat": cmat, "gap_open_cost": o, "seed": seed,
           "cost": min(dp[len(s1)][len(s2)])}
    random.seed(seed)
    try:
        a, mid, b, cost = ga.dp_array_backward(dp_array=dp, seq_1=s1, seq_2=s2, costing_mat=cmat, gap_open_cost=o)
        assert cost == rec["cost"]
        rec.update(status="ok", strings=[a, mid, b])
    except IndexError:
        rec.update(status="IndexError", strings=None)
    rec["state_after"] = state_digest()
    return rec


def main():
    ga, start, _ = _import_reference()
    rng = random.Random(20261020)  # private generator: never touches the global one
    tmp = tempfile.mkdtemp(prefix="ga_general_")
    cases = []
    for family in "GWS":
        for k in range(PER_FAMILY):
            tseed = 100 + k
            short = k % 5 == 4  # a few cases with a side of 1-3 letters
            m = rng.randint(1, 3) if short and k % 2 == 0 else rng.randint(4, 140)
            n = rng.randint(1, 3) if short and k % 2 == 1 else rng.randint(4, 140)
            if k == 4:  # one letter against a few, at large gap opens: where the reference's walk raises IndexError
                m, n = 1, rng.randint(4, 8)
            if k == 9:
                m, n = rng.randint(4, 8), 1
            if k == 0:
                m, n = 140, 139
            s1 = gc.splitmix_seq(m, rng.getrandbits(64))
            s2 = gc.splitmix_seq(n, rng.getrandbits(64))
            o = GAP_OPENS[(k + "GWS".index(family)) % len(GAP_OPENS)]
            if short:  # the degenerate sides at the larger gap opens, one word width each
                o = [127, 300, 20, 7][k // 5]
            seed = rng.randint(0, 2 ** 31 - 1)
            extra = {}
            if family == "S":
                letters, rows = gc.api_score_rows(tseed)
                path = gc.write_mtx(os.path.join(tmp, f"s{k}.mtx"), letters, rows)
                _, _, _, cmat, _, goc, _ = start.validate_and_transform_args(
                    None, None, s1, s2, scoring_mat_path=path, gap_open_score=-o)
                assert goc == o
                extra["mtx"] = {"letters": letters, "scores": rows}
            else:
                cmat = gc.table(family, tseed)
            rec = run_case(ga, start, s1, s2, cmat, o, seed)
            rec.update(family=family, table_seed=tseed, **extra)
            cases.append(rec)
    with open(os.path.join(HERE, "general_costs.json"), "w") as fh:
        json.dump(cases, fh, separators=(",", ":"))
    print("wrote", len(cases), "cases;", sum(c["status"] != "ok" for c in cases), "IndexError")


if __name__ == "__main__":
    main()
