"""A picture of a feature cache: the exact t-SNE embedding (scd_amd.tsne, csrc/tsne.hip; docs/design/tsne.md) of the rows of

  ROOT/extracted_features/{feat_model}_{dataset_name}_all.pt     dict all_feats, mask_lab, targets (main_unsup.py:141-146)

coloured by the targets or by a clustering, as the reference's save_tsne draws it (local_utils/util.py:178-194).

  python plot_features.py --root_dir ROOT --dataset_name D --feat_model clip [--clip_model ViT-L/14] [--perplexity 30]
                          [--colour targets|clusters --cluster_result FILE] [--class_names JSON] [--out PNG]

Writes the PNG (default ROOT/cluster/tsne_{feat_model}_{dataset_name}.png), the coordinates beside it as .npy (float32 [N, 2]) and a .json
with the arguments, kl_divergence_, n_iter_ and the affinity info.  --cluster_result: a .npy / .pt of one cluster id per row.
--class_names: a JSON list (or {id: name} object) that names the legend entries.
"""
import argparse
import json
import os

import numpy as np
import torch

import main_unsup as mu
import score_features as sf


def build_parser():
    p = argparse.ArgumentParser(description='plot_features', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--root_dir', type=str, required=True)
    p.add_argument('--dataset_name', type=str, required=True)
    p.add_argument('--feat_model', type=str, required=True)
    p.add_argument('--clip_model', type=str, default='ViT-B/16', choices=mu.clip.available_models(), help='CLIP backbone of feat_model clip')
    p.add_argument('--perplexity', type=float, default=30.0)
    p.add_argument('--colour', type=str, default='targets', choices=['targets', 'clusters'])
    p.add_argument('--cluster_result', type=str, default=None, help='one cluster id per row (.npy or .pt), for --colour clusters')
    p.add_argument('--class_names', type=str, default=None, help='JSON list or {id: name} object for the legend')
    p.add_argument('--out', type=str, default=None, help='the PNG; the .npy and .json go beside it')
    return p


def load_labels(args, n, targets):
    if args.colour == 'targets':
        return np.asarray(targets).astype(np.int64)
    if not args.cluster_result or not os.path.exists(args.cluster_result):
        raise SystemExit("--colour clusters needs --cluster_result FILE with one cluster id per row")
    raw = np.load(args.cluster_result) if args.cluster_result.endswith('.npy') else torch.load(args.cluster_result, weights_only=False)
    labels = np.asarray(raw).astype(np.int64).reshape(-1)
    if labels.shape[0] != n:
        raise SystemExit(f"{args.cluster_result} holds {labels.shape[0]} ids for {n} rows")
    return labels


def main(argv=None):
    args = build_parser().parse_args(argv)
    path = sf.cache_path(args, args.feat_model)
    if not os.path.exists(path):
        raise SystemExit(sf.MISSING.format(path=path, feat_model=args.feat_model))
    data = torch.load(path, weights_only=False)
    feats = np.ascontiguousarray(np.asarray(data['all_feats'], dtype=np.float32))
    labels = load_labels(args, feats.shape[0], data['targets'])
    assert torch.cuda.is_available(), "plot_features.py needs a HIP device"
    from scd_amd.local_utils.util import scatter_png
    from scd_amd.tsne import TSNE
    t = TSNE(n_components=2, perplexity=args.perplexity, random_state=0)
    Y = t.fit_transform(feats)
    cdir = os.path.join(args.root_dir, 'cluster')
    os.makedirs(cdir, exist_ok=True)
    png = args.out or os.path.join(cdir, f'tsne_{args.feat_model}_{args.dataset_name}.png')
    base = os.path.splitext(png)[0]
    names = None
    if args.class_names:
        with open(args.class_names) as fh:
            raw = json.load(fh)
        names = {int(c): str(v) for c, v in (raw.items() if isinstance(raw, dict) else enumerate(raw))}
    scatter_png(Y, labels, png, marker_sz=5, names=names)
    np.save(base + '.npy', Y)
    out = dict(args=vars(args), N=int(feats.shape[0]), D=int(feats.shape[1]), cache=path, kl_divergence_=t.kl_divergence_, n_iter_=int(t.n_iter_),
               info=t.info_)
    with open(base + '.json', 'w') as fh:
        json.dump(out, fh, indent=1)
    print(f'KL {t.kl_divergence_:.4f} after {t.n_iter_ + 1} iterations; written {png}, {base}.npy, {base}.json')
    return out


if __name__ == "__main__":
    main()
