"""Runs greedy seedings of tests/seeding_cases.py through ops.kpp_greedy_lockstep with the exact fp16 copy and stores picks and centres:
as a fresh child process (python seeding_child.py OUT.npz INDEX [INDEX ...], indices into seeding_cases.GREEDY_SPECS) under a
SCD_KM_FILTER_FROM other than the default, which the library reads once per process."""
import os
import sys

import numpy as np


def run_specs(ops, indices):
    import torch
    import seeding_cases as sc
    res = {}
    for i in indices:
        sp = sc.GREEDY_SPECS[i]
        x, first, u, _ = sc.greedy_inputs(sp)
        xt = torch.from_numpy(x).cuda()
        x16 = ops.f16_exact(xt)
        assert x16 is not None
        cent, picks = ops.kpp_greedy_lockstep(xt, x16, first, u, sp.k)
        res["picks_%d" % i] = picks.cpu().numpy().T
        res["cent_%d" % i] = cent.cpu().numpy()
    return res


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from scd_amd import ops
    np.savez(sys.argv[1], **run_specs(ops, [int(a) for a in sys.argv[2:]]))
    print("done")
