"""Unpacks the label-pair cases of tests/golden/cluster_scores.npz (tools/gen_cluster_scores_golden.py packs them back to back)."""
import numpy as np


def cases(gold):
    """One dict per case: pred, truth int64 [n], mask bool [n], table int64 [D, D], scores [4] (ACC, NMI, ARI, purity), ints [6],
    info [3]."""
    out = []
    r0 = t0 = 0
    for c, (n, d) in enumerate(zip(gold["rows"], gold["dims"])):
        n, d = int(n), int(d)
        out.append(dict(pred=gold["pred"][r0:r0 + n].astype(np.int64), truth=gold["truth"][r0:r0 + n].astype(np.int64),
                        mask=gold["mask"][r0:r0 + n], table=gold["tables"][t0:t0 + d * d].reshape(d, d).astype(np.int64),
                        scores=gold["scores"][c], ints=gold["ints"][c], info=gold["info"][c]))
        r0, t0 = r0 + n, t0 + d * d
    assert r0 == gold["pred"].size and t0 == gold["tables"].size
    return out
