"""Runs the planted and degenerate similarity cases at d = 512 through ops.sim_topk and stores every index / value array.  In-process it
gives tests/test_gpu_sim.py the default library's results; as a fresh child process (python sim_child.py OUT.npz K [K ...]) the same
under SCD_SIM_RB / SCD_SIM_REFINE4 / SCD_SIM_SPLIT, which the library reads once per process."""
import os
import sys

import numpy as np

N, V, D = 300, 1031, 512


def cases(k):
    import sim_cases as sc
    out = {}
    for spacing in ("wide", "narrow"):
        out["%s_k%d" % (spacing, k)] = sc.planted(N, V, D, k, spacing, neg_rows=spacing == "narrow")[0]
    out["repeat_k%d" % k] = sc.repeated_vocab(N, V, D, k)
    return out


def run_cases(ops, ks):
    import torch
    res = {}
    for k in ks:
        for name, c in cases(k).items():
            wt = ops.transpose_f16(torch.from_numpy(c.w).cuda())
            for mode in ("raw", "softmax"):
                idx, val, fb = ops.sim_topk(torch.from_numpy(c.f).cuda(), wt, k, mode, scale=c.scale, return_fallback=True)
                res["%s_%s_idx" % (name, mode)] = idx.cpu().numpy()
                res["%s_%s_val" % (name, mode)] = val.cpu().numpy()
                res["%s_%s_fb" % (name, mode)] = np.array(int(fb.item()))
                res["%s_%s_path" % (name, mode)] = np.array(ops.sim_last_path())
    return res


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from scd_amd import ops
    np.savez(sys.argv[1], **run_cases(ops, [int(a) for a in sys.argv[2:]]))
    print("done")
