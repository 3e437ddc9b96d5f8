"""Writes tests/golden/pose_prior_reference.json: what the GPU tests of the pose-from-the-prediction rule compare with -- the 50-digit
reference's masks round by round, rounds_run, converged and result for every case of tests/pose_prior_cases.py, keyed by a digest of the
case's inputs.  tests/test_pose_prior_reference.py holds every record to the live solve (and asserts the input condition on it); run this
after changing the case table.  About a minute.

    python tools/make_pose_prior_reference.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_prior_cases as pc      # noqa: E402
import pose_prior_mp as ppm        # noqa: E402


def main():
    out = {}
    for cid in pc.IDS:
        ref = pc.reference_live(cid)
        bad = ppm.band_violations(ref)
        if bad:
            raise SystemExit("%s: wrong fixture (replace the seed): %r" % (cid, bad[:5]))
        out[cid] = pc.record(cid, ref)
        print(cid, "rounds", ref["rounds_run"], "converged", ref["converged"], "result", ref["result"], [int(m.sum()) for m in ref["masks"]])
    with open(pc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", pc.GOLDEN)


if __name__ == "__main__":
    main()
