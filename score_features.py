"""Which tower suits this data set?  Scores the feature caches main_unsup.py / main_ptsup.py write

  ROOT/extracted_features/{feat_model}_{dataset_name}_all.pt     dict all_feats, mask_lab, targets (main_unsup.py:141-146)

by the weighted k-NN protocol of DINO / DINOv2 (Caron et al., ICCV 2021, section 4.1): every labelled row is classified by its k nearest
OTHER labelled rows under cosine similarity (leave-one-out), each neighbour voting exp(cosine / temperature) for its class; the score
of a tower is the accuracy.  One exact k-NN pass per tower on the device (scd_amd.knn, csrc/knn.hip) instead of a pipeline run per
tower.  The cache names are the mains' (main_unsup.feat_cache_name: `clip` carries the tag of --clip_model).

  python score_features.py --root_dir ROOT --dataset_name D --feat_models clip dino_vit dinov2_vitb14 [--clip_model ViT-L/14]
                           [--k 20] [--temperature 0.07] [--weights softmax|uniform]

Prints one table and writes ROOT/cluster/knn_score_{dataset_name}.json.

--probe adds the protocol's other half, the linear probe (scd_amd.probe.LinearProbe, csrc/probe.hip): multinomial logistic regression
on the unit rows of a deterministic stratified split of the labelled rows (within each class, in cache order, the rows whose
within-class index is 4 mod 5 validate, the rest train), one fit per value of --probe_C.  It prints a second table (tower, C, training
and validation accuracy, iterations, evaluations) and writes ROOT/cluster/probe_score_{dataset_name}.json.
"""
import argparse
import json
import os

import numpy as np
import torch

import main_unsup as mu

NO_LABELS = ("the cache {path} has no labelled row: the k-NN score is an accuracy on the labelled rows.  "
             "Without labels, `estimate_k.py --criterion silhouette` scores a tower's clusterings instead")
MISSING = ("no feature cache at {path}: write it with `main_unsup.py --extract_feat true --feat_model {feat_model}` "
           "(or drop {feat_model} from --feat_models)")


def build_parser():
    p = argparse.ArgumentParser(description='score_features', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--root_dir', type=str, required=True)
    p.add_argument('--dataset_name', type=str, required=True)
    p.add_argument('--feat_models', type=str, nargs='+', required=True, help='{feat_model} of the caches to score, as the mains take it')
    p.add_argument('--clip_model', type=str, default='ViT-B/16', choices=mu.clip.available_models(), help='CLIP backbone of feat_model clip')
    p.add_argument('--k', type=int, default=20)
    p.add_argument('--temperature', type=float, default=0.07)
    p.add_argument('--weights', type=str, default='softmax', choices=['softmax', 'uniform'])
    p.add_argument('--probe', action='store_true', help='also fit the linear probe on a stratified split of the labelled rows')
    p.add_argument('--probe_C', type=float, nargs='+', default=[1.0], help="inverse L2 strengths, scikit-learn's C: one fit per value")
    return p


PROBE_ARGS = ('probe', 'probe_C')               # kept out of the k-NN file: it is the same with and without them


def stratified_split(targets, period=5, slot=4):
    """(train mask, validation mask) of the rows: within each class, in row order, the rows whose within-class index is `slot` mod `period`
    validate.  A class with fewer than `period` rows has no validation row."""
    targets = np.asarray(targets)
    order = np.argsort(targets, kind='stable')
    st = targets[order]
    first = np.r_[True, st[1:] != st[:-1]] if st.size else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(st.size), 0))
    val = np.zeros(targets.shape[0], bool)
    val[order] = (np.arange(st.size) - start) % period == slot
    return ~val, val


def probe_towers(args, loaded):
    """One LinearProbe fit per tower and C on the unit rows of the split -> {tower: {N_train, N_val, D, classes, fits: [...]}}."""
    from scd_amd.knn import unit_rows
    from scd_amd.probe import LinearProbe
    towers = {}
    for fm, path, feats, targets in loaded:
        train, val = stratified_split(targets)
        if not val.any():
            raise SystemExit(f"the cache {path} has no class with 5 labelled rows: the probe has no validation row")
        counts = np.unique(targets, return_counts=True)[1]
        u = unit_rows(torch.as_tensor(feats).cuda())
        tr, va = torch.as_tensor(np.flatnonzero(train)).cuda(), torch.as_tensor(np.flatnonzero(val)).cuda()
        fits = []
        for C in args.probe_C:
            lp = LinearProbe(C=C).fit(u[tr], targets[train])
            fits.append(dict(C=float(C), train_acc=lp.score(u[tr], targets[train]), val_acc=lp.score(u[va], targets[val]),
                             n_iter=lp.n_iter_, n_eval=lp.n_eval_, converged=bool(lp.converged_), objective=lp.objective_))
        towers[fm] = dict(N_train=int(train.sum()), N_val=int(val.sum()), D=int(feats.shape[1]), classes=int(counts.size),
                          classes_without_validation=int((counts < 5).sum()), cache=path, fits=fits)
    return towers


def report_probe(args, towers):
    print('linear probe on the unit rows (validation: within-class index 4 mod 5 of the labelled rows)')
    print('%-24s %10s %10s %9s %6s %6s' % ('feat_model', 'C', 'train_acc', 'val_acc', 'iter', 'eval'))
    rows = [(fm, f) for fm, t in towers.items() for f in t['fits']]
    for fm, f in sorted(rows, key=lambda r: -r[1]['val_acc']):
        print('%-24s %10g %10.4f %9.4f %6d %6d' % (fm, f['C'], f['train_acc'], f['val_acc'], f['n_iter'], f['n_eval']))
    for fm, t in towers.items():
        if t['classes_without_validation']:
            print(f"{fm}: {t['classes_without_validation']} classes have fewer than 5 labelled rows and no validation row")
    best = max(rows, key=lambda r: r[1]['val_acc'])
    out = dict(args=vars(args), towers=towers, best=best[0], best_C=best[1]['C'])
    jpath = os.path.join(args.root_dir, 'cluster', f'probe_score_{args.dataset_name}.json')
    with open(jpath, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(f'written to {jpath}')
    return out


def cache_path(args, feat_model):
    name = mu.feat_cache_name(argparse.Namespace(feat_model=feat_model, clip_model=args.clip_model))
    return os.path.join(args.root_dir, 'extracted_features', f'{name}_{args.dataset_name}_all.pt')


def load_labelled(args, feat_model):
    """(features float32 [L, D] numpy, targets int64 [L]) of the labelled rows of one tower's cache; SystemExit with a message otherwise."""
    path = cache_path(args, feat_model)
    if not os.path.exists(path):
        raise SystemExit(MISSING.format(path=path, feat_model=feat_model))
    data = torch.load(path, weights_only=False)
    mask_lab = np.asarray(data['mask_lab']).astype(bool)
    if not mask_lab.any():
        raise SystemExit(NO_LABELS.format(path=path))
    feats = np.asarray(data['all_feats'], dtype=np.float32)[mask_lab]
    return np.ascontiguousarray(feats), np.asarray(data['targets']).astype(np.int64)[mask_lab]


def main(argv=None):
    args = build_parser().parse_args(argv)
    loaded = [(fm, cache_path(args, fm)) + load_labelled(args, fm) for fm in args.feat_models]      # every cache is checked before any run
    assert torch.cuda.is_available(), "score_features.py needs a HIP device"
    from scd_amd import knn
    towers = {}
    for fm, path, feats, targets in loaded:
        if feats.shape[0] <= args.k:
            raise SystemExit(f"the cache {path} has {feats.shape[0]} labelled rows: leave-one-out k-NN with --k {args.k} needs more")
        acc, info = knn.knn_accuracy(torch.as_tensor(feats).cuda(), targets, k=args.k, temperature=args.temperature, weights=args.weights,
                                     return_info=True)
        towers[fm] = dict(acc=acc, N=int(feats.shape[0]), D=int(feats.shape[1]), cache=path, info=[int(v) for v in info.cpu().tolist()])
    print(f'leave-one-out k-NN accuracy on the labelled rows (k = {args.k}, {args.weights}, T = {args.temperature})')
    print('%-24s %8s %6s %9s' % ('feat_model', 'N', 'D', 'knn_acc'))
    for fm, t in sorted(towers.items(), key=lambda kv: -kv[1]['acc']):
        print('%-24s %8d %6d %9.4f' % (fm, t['N'], t['D'], t['acc']))
    out = dict(args={k: v for k, v in vars(args).items() if k not in PROBE_ARGS}, towers=towers, best=max(towers, key=lambda fm: towers[fm]['acc']))
    cdir = os.path.join(args.root_dir, 'cluster')
    os.makedirs(cdir, exist_ok=True)
    jpath = os.path.join(cdir, f'knn_score_{args.dataset_name}.json')
    with open(jpath, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(f'written to {jpath}')
    if args.probe:
        out['probe'] = report_probe(args, probe_towers(args, loaded))
    return out


if __name__ == "__main__":
    main()
