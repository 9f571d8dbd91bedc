"""Writes tests/golden/finch.npz by running the reference's FINCH (local_utils/finch.py, cosine distance) on the CPU on the cases of
tests/finch_cases.py.  The reference is imported at run time from $SCD_REFERENCE (oracle/gen_golden.py's convention); nothing of it is
copied.  A missing pyflann is only the reference's own warning: every case is below its 70,000-row flann threshold.

  c_<case>          int32 [N, P]   the reference's partitions
  num_<case>        int32 [P]      their cluster counts
  req_<case>_<r>    int32 [N]      req_c for req_clust = r
  margins_<case>    float64 [2]    smallest top-2 first-neighbour margin over all levels, smallest threshold margin (float64 restatement)

The generator ASSERTS, per case, that the float64 restatement (finch_cases.finch_f64) equals the reference at every level and for every
req_clust value, and that the margins are at least finch_cases.MIN_NEIGHBOUR_MARGIN / MIN_THRESHOLD_MARGIN: the reference computes in
float32, and those margins are what makes "equal to the reference" a fair demand.  A case that stops meeting them is replaced by
another seed, not loosened.

  SCD_REFERENCE=/path/to/reference python tools/gen_finch_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import finch_cases as fc                                        # noqa: E402

REF = os.environ.get("SCD_REFERENCE")


def main():
    if not REF or not os.path.exists(os.path.join(REF, "local_utils", "finch.py")):
        raise SystemExit("set SCD_REFERENCE to a checkout of the reference (it holds local_utils/finch.py)")
    sys.path.insert(0, os.path.join(REF, "local_utils"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import finch as ref                                     # the reference's module
    out = {}
    for name, (n, d, k, noise, seed, half, reqs) in fc.CASES.items():
        x = fc.case_input(name)
        c, num, _ = ref.FINCH(x, verbose=False)
        c64, num64, _ = fc.finch_f64(x)
        assert list(num) == num64 == fc.NUM_CLUST[name], (name, num, num64)
        assert np.array_equal(c, c64), name
        nb, th = fc.margins(x)
        assert nb >= fc.MIN_NEIGHBOUR_MARGIN and th >= fc.MIN_THRESHOLD_MARGIN, (name, nb, th)
        out["c_" + name] = np.asarray(c, dtype=np.int32)
        out["num_" + name] = np.asarray(num, dtype=np.int32)
        out["margins_" + name] = np.array([nb, th])
        for r in reqs:
            _, _, req = ref.FINCH(x, req_clust=r, verbose=False)
            _, _, req64 = fc.finch_f64(x, req_clust=r)
            assert np.array_equal(req, req64), (name, r)
            assert len(np.unique(req)) == r
            out["req_%s_%d" % (name, r)] = np.asarray(req, dtype=np.int32)
        print("%-6s N %5d D %4d: clusters %s, neighbour margin %.2e, threshold margin %.2e" % (name, n, d, list(num), nb, th))
    path = os.path.join(ROOT, "tests", "golden", "finch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
