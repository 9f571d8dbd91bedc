"""How many categories are there?  GCD's estimator (the reference's gcd/methods/estimate_k/estimate_k.py, which the SCD paper points
to for an unknown class number) on the feature caches main_unsup.py / main_ptsup.py write:

  ROOT/extracted_features/{feat_model}_{dataset_name}_all.pt     dict all_feats, mask_lab, targets (main_unsup.py:141-146)

All features, labelled and unlabelled, are L2-normalised once (estimate_k.py:61) and clustered with
`KMeans(n_clusters=K, random_state=0)` for the Ks a search asks for.  Three criteria:

  --criterion acc (default)   GCD's: the K with the highest clustering accuracy on the LABELLED rows wins; bounded Brent search
                              (default, :221-242) or the reference's binary search (:172-218).  Needs labelled rows.
  --criterion silhouette      label-free: the K with the highest mean silhouette coefficient over all rows wins; integer grid search
                              by default.  For caches without labelled rows (main_unsup.py's setting).
  --criterion bic             label-free: a diagonal Gaussian mixture of K components (scd_amd.gmm, --covariance_type) is fitted
                              instead of k-means and the K with the LOWEST Bayesian information criterion wins; integer grid search
                              by default.  One n x K x d pass per EM step and no n x n pass; K <= 1024, d <= 1024.
                              --covariance_type full | tied fits scd_amd.gmm_full's mixture instead: d <= 64, so with --pca_dim.

--clusterer ward (with acc or silhouette) fits one Ward tree on all rows (scd_amd.ward, docs/design/ward.md) and scores its cut at
every K a search asks for: no fit per K.  The default, kmeans, is the reference's.

Fits and scores run on the GPU (scd_amd.cluster.KMeans, scd_amd.metrics).  Writes
ROOT/cluster/estimated_k_{feat_model}_{dataset_name}.json and prints the value to pass as --n_cluster.

  python estimate_k.py --root_dir ROOT --dataset_name cub --feat_model clip [--max_classes 1000] [--search_mode brent|binary|grid|finch]
  python estimate_k.py --root_dir ROOT --dataset_name D --feat_model clip --criterion silhouette --max_classes 1000
  python estimate_k.py --root_dir ROOT --dataset_name D --feat_model clip --criterion bic --max_classes 200 [--covariance_type spherical]

--pca_dim M [--pca_whiten] reduces the normalised features to M principal components first (scd_amd.pca, docs/design/pca.md) and
renormalises the rows; the mixture's responsibilities are informative there.
"""
import argparse
import json
import os

import numpy as np
import torch

from scd_amd import estimate_k as ek
from scd_amd import ops


def build_parser():
    p = argparse.ArgumentParser(description='estimate_k', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--root_dir', type=str, required=True)
    p.add_argument('--dataset_name', type=str, required=True)
    p.add_argument('--feat_model', type=str, default='clip', help='{feat_model} of the cache file name')
    p.add_argument('--max_classes', default=1000, type=int)
    p.add_argument('--min_classes', default=None, type=int,
                   help='default: acc - the number of distinct targets among the labelled rows (the reference\'s num_labeled_classes); '
                        'silhouette and bic - 2')
    p.add_argument('--criterion', type=str, default='acc', choices=['acc', 'silhouette', 'bic'],
                   help='acc: clustering accuracy on the labelled rows (GCD); silhouette: mean silhouette coefficient, needs no labels; '
                        'bic: lowest Bayesian information criterion of a diagonal Gaussian mixture, needs no labels')
    p.add_argument('--clusterer', type=str, default='kmeans', choices=['kmeans', 'ward'],
                   help='kmeans: one fit per K searched; ward: one Ward tree on all rows (scd_amd.ward), every K is a cut of it; '
                        'with --criterion acc or silhouette')
    p.add_argument('--covariance_type', type=str, default='diag', choices=['diag', 'spherical', 'full', 'tied'],
                   help="--criterion bic: the mixture's covariances; full and tied (scd_amd.gmm_full) take rows of at most 64 dimensions")
    p.add_argument('--search_mode', type=str, default=None, choices=['brent', 'binary', 'grid', 'finch'],
                   help='Mode for black box optimisation; default: brent for acc, grid for silhouette and bic.  finch: score only the '
                        'cluster counts of FINCH\'s partitions of all rows, clipped to [min_classes, max_classes]')
    p.add_argument('--pca_dim', type=int, default=0,
                   help='> 0: the normalised features are reduced to this many principal components (scd_amd.pca.PCA fitted on all rows) '
                        'and renormalised to unit rows before the search; 0: off')
    p.add_argument('--pca_whiten', action='store_true', help='--pca_dim: whiten the components before the renormalisation')
    return p


def parse_args(argv=None):
    """The parsed arguments with the criterion-dependent defaults resolved."""
    args = build_parser().parse_args(argv)
    if args.clusterer == 'ward' and args.criterion == 'bic':
        raise SystemExit("--clusterer ward scores cuts of one tree; --criterion bic fits a Gaussian mixture per K and has no use for "
                         "it: use --criterion acc or silhouette")
    if args.search_mode is None:
        args.search_mode = 'brent' if args.criterion == 'acc' else 'grid'
    if args.min_classes is None and args.criterion in ('silhouette', 'bic'):
        args.min_classes = 2
    return args


def main(argv=None):
    args = parse_args(argv)
    assert torch.cuda.is_available(), "estimate_k.py needs a HIP device"
    dev = torch.device("cuda")
    path = os.path.join(args.root_dir, 'extracted_features', f'{args.feat_model}_{args.dataset_name}_all.pt')
    data = torch.load(path, weights_only=False)
    mask_lab = np.asarray(data['mask_lab']).astype(bool)
    targets = np.asarray(data['targets']).astype(int)
    sil, bic = args.criterion == 'silhouette', args.criterion == 'bic'
    if not sil and not bic and not mask_lab.any():
        raise SystemExit("the cache has no labelled row: the estimator scores K on the labelled rows")
    feats = ops.l2norm_rows(torch.as_tensor(np.asarray(data['all_feats'])).to(dev).float())
    if args.pca_dim:
        from scd_amd.pca import PCA
        pca = PCA(n_components=args.pca_dim, whiten=args.pca_whiten)
        feats = pca.fit_transform(feats, unit=True)
        print(f'PCA: {pca.n_components_} of {pca.n_features_in_} dimensions keep {pca.explained_variance_ratio_.sum():.4f} of the variance')
    if sil:
        small_k = args.min_classes
        big_k = min(args.max_classes, feats.shape[0] - 1)       # the silhouette needs fewer clusters than rows
    elif bic:
        small_k = args.min_classes
        big_k = min(args.max_classes, feats.shape[0], 1024)     # the mixture kernel's limit on K
    else:
        small_k = args.min_classes if args.min_classes is not None else len(np.unique(targets[mask_lab]))
        big_k = min(args.max_classes, feats.shape[0])
    if big_k <= small_k:
        raise SystemExit(f"--max_classes {big_k} must be above the smallest K searched, {small_k}")
    print(f'{feats.shape[0]} rows, {int(mask_lab.sum())} labelled; searching K in [{small_k}, {big_k}] ({args.search_mode}, {args.criterion})')
    scores = {}
    tree = None
    if args.clusterer == 'ward':
        from scd_amd.ward import ward_tree
        tree, winfo = ward_tree(feats)
        print(f"Ward tree: {winfo['rounds']} rounds, {winfo['full_requeries']} full requeries")

    if tree is not None:
        targets_dev = None if sil else torch.as_tensor(targets, device=dev)
        mask_dev = None if sil else torch.as_tensor(mask_lab, device=dev)

        def evaluate(K):
            s, scores[int(K)] = ek.evaluate_cut(K, feats, tree, targets_dev, mask_dev, verbose=True)
            return s
        name = 'silhouette' if sil else 'labelled_acc'
    elif sil:
        def evaluate(K):
            s, scores[int(K)] = ek.evaluate_k_unlabelled(K, feats, verbose=True)
            return s
        name = 'silhouette'
    elif bic:
        def evaluate(K):                                        # the searches maximise: -BIC; scores[K] keeps the BIC and the lower bound
            s, scores[int(K)] = ek.evaluate_k_bic(K, feats, covariance_type=args.covariance_type, verbose=True)
            return s
        name = 'neg_bic'
    else:
        targets_dev = torch.as_tensor(targets, device=dev)
        mask_dev = torch.as_tensor(mask_lab, device=dev)

        def evaluate(K):
            acc, scores[int(K)] = ek.evaluate_k(K, feats, targets_dev, mask_dev, verbose=True)
            return acc
        name = 'labelled_acc'

    if args.search_mode == 'brent':
        print('Optimising with Brents algorithm')
        x, k, trace = ek.brent(evaluate, small_k, big_k)
        print(f'Optimal K is {x}')
        out = dict(x=x, trace=[{'K': kf, 'int_K': ki, name: a} for kf, ki, a in trace])
    elif args.search_mode == 'binary':
        k, trace = ek.binary_search(evaluate, small_k, big_k, log=print)
        out = dict(trace=[dict(small_k=s, middle_k=m, big_k=b, accs=list(a)) for s, m, b, a in trace])
    elif args.search_mode == 'finch':
        from scd_amd.finch import Finch
        finch_num_clust = [int(v) for v in Finch().fit(feats).num_clust_]
        print(f'FINCH partitions: {finch_num_clust} clusters')
        k, trace = ek.finch_search(evaluate, finch_num_clust, small_k, big_k, log=print)
        out = dict(trace=[dict(ks=list(ks), scores=list(sc), best=int(b)) for ks, sc, b in trace], finch_num_clust=finch_num_clust)
    else:
        k, trace = ek.grid_search(evaluate, small_k, big_k, log=print)
        out = dict(trace=[dict(ks=list(ks), scores=list(sc), best=int(b)) for ks, sc, b in trace])
    out.update(k=int(k), criterion=args.criterion, clusterer=args.clusterer, search_mode=args.search_mode, min_classes=int(small_k), max_classes=int(big_k),
               scores={str(kk): v for kk, v in sorted(scores.items())})
    if args.pca_dim:
        out.update(pca_dim=int(args.pca_dim), pca_whiten=bool(args.pca_whiten))
    cdir = os.path.join(args.root_dir, 'cluster')
    os.makedirs(cdir, exist_ok=True)
    jpath = os.path.join(cdir, f'estimated_k_{args.feat_model}_{args.dataset_name}.json')
    with open(jpath, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(f'Estimated number of categories: {int(k)}  (written to {jpath}); pass --n_cluster {int(k)}')
    return out


if __name__ == "__main__":
    main()
