"""Which tower suits this data set?  Scores the feature caches main_unsup.py / main_ptsup.py write

  ROOT/extracted_features/{feat_model}_{dataset_name}_all.pt     dict all_feats, mask_lab, targets (main_unsup.py:141-146)

by the weighted k-NN protocol of DINO / DINOv2 (Caron et al., ICCV 2021, section 4.1): every labelled row is classified by its k nearest
OTHER labelled rows under cosine similarity (leave-one-out), each neighbour voting exp(cosine / temperature) for its class; the score
of a tower is the accuracy.  One exact k-NN pass per tower on the device (scd_amd.knn, csrc/knn.hip) instead of a pipeline run per
tower.  The cache names are the mains' (main_unsup.feat_cache_name: `clip` carries the tag of --clip_model).

  python score_features.py --root_dir ROOT --dataset_name D --feat_models clip dino_vit dinov2_vitb14 [--clip_model ViT-L/14]
                           [--k 20] [--temperature 0.07] [--weights softmax|uniform]

Prints one table and writes ROOT/cluster/knn_score_{dataset_name}.json.
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
    return p


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
    out = dict(args=vars(args), towers=towers, best=max(towers, key=lambda fm: towers[fm]['acc']))
    cdir = os.path.join(args.root_dir, 'cluster')
    os.makedirs(cdir, exist_ok=True)
    jpath = os.path.join(cdir, f'knn_score_{args.dataset_name}.json')
    with open(jpath, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(f'written to {jpath}')
    return out


if __name__ == "__main__":
    main()
