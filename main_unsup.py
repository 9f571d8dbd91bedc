#!/usr/bin/env python
"""Unsupervised semantic category discovery on MI355X - the entry point of /root/reference/main_unsup.py with the
same flags (:207-224), stage order (:298-641) and cache files, running on libscd_hip.so.

Data.  The reference reads image folders through torchvision dataset classes (gcd/data: out of scope).
Here every stage starts from the reference's own cache files under --root_dir, byte-compatible with the ones it writes:
  extracted_features/{feat_model}_{dataset}_all.pt   dict all_feats, mask_lab, mask_cls, targets      (:141-146,294-301)
  extracted_features/clip_{dataset}_all.pt           same dict, CLIP features                          (:306-311)
  cluster/{cluster}_{feat_model}_{dataset}_{n_cluster}.pt   dict all_preds, u_preds, u_targets, mask  (:366-374)
                                                            ({cluster} = KM, SSKM, ConSSKM, FINCH, SC, GMM or WARD; WARD adds linkage)
  cluster/HDBSCAN_{feat_model}_{dataset}_mcs{min_cluster_size}[_ms{min_samples}].pt   the same dict plus noise, probabilities, n_cluster
                                                            (--cluster HDBSCAN: the number of clusters is a result, not a flag)
  zeroshot_weights/zeroshot_weights_all_{nouns|wikibird|wikidog}_vit_b_16.pt   tensor [512, V]        (:389-394)
--clip_model picks the CLIP backbone (clip.available_models(), default ViT-B/16: the names above).  With another one every
CLIP-derived cache carries its tag, so that no cache of one backbone is read as another's features:
  extracted_features/clip_vit_l_14_{dataset}_all.pt, zeroshot_weights/zeroshot_weights_all_{corpus}_vit_l_14.pt, and
  clip_vit_l_14 in place of {feat_model} when --feat_model clip.  A missing classifier of such a backbone is built from the corpus
  (clip_lang_util.zeroshot_classifier, the 80 templates, the backbone's text tower; needs the BPE merges file) and saved.
The two things the reference takes from its dataset objects are passed as files instead:
  --class_names  JSON {original class name: class index}  (`datasets['test'].class_to_idx` / the sorted breed / wnid tables)
  --images_pt    torch file dict(images [N,3,224,224] preprocessed, targets [N], mask_lab [N]) for --extract_feat true, or
  --image_list   CSV of `path,target,labelled` rows (paths relative to the CSV's directory; labelled rows first, MergedDataset order,
                 data_utils.py:12-37) for --extract_feat true straight from image files: one PIL decode per image, CLIP's
                 `preprocess` (:271) on the device bit for bit, both towers fed from it, and the two caches above written
                 (scd_amd/images.py; scd_amd.images.list_image_folder lists an ImageFolder tree and its class_to_idx)
  --decode       with --image_list: `pil` (default), or `device` = baseline JPEGs decoded on the device to the pixels PIL gives, every
                 other file and every stream the device decoder rejects through PIL (scd_amd/jpeg.py); the caches are the same
With --synthetic everything is generated from seeds (no dataset / checkpoint needed).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import scd_amd  # noqa: E402
scd_amd.install()

import clip  # noqa: E402
from gcd.project_utils.cluster_and_log_utils import split_cluster_acc_v2  # noqa: E402
from local_utils.util import str2bool  # noqa: E402
from local_utils.sskm_constrained import K_Means as ConSemiSupKMeans  # noqa: E402
from gcd.methods.clustering.faster_mix_k_means_pytorch import K_Means as SemiSupKMeans  # noqa: E402
from local_utils.clip_lang_util import get_nouns  # noqa: E402
from scd_amd import naming, ops, pipeline  # noqa: E402
from scd_amd.cluster import KMeans  # noqa: E402   (sklearn.cluster.KMeans surface on the HIP kernels)


def build_parser():
    p = argparse.ArgumentParser(description='cluster', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--num_workers', default=2, type=int)
    p.add_argument('--root_dir', type=str, default='/Your_data_dir')
    p.add_argument('--dataset_name', type=str, default='imagenet_1000')
    p.add_argument('--feat_model', type=str, default='dino_vit',
                   help='clustering features: clip, dino_vit, gcd, or a DINOv2 tower dinov2_vitb14 | dinov2_vitl14 | dinov2_vitb14_reg | '
                        'dinov2_vitl14_reg ($SCD_ROOT/dinov2/); the cache files carry the name as given')
    p.add_argument('--prop_train_labels', type=float, default=0.5)
    p.add_argument('--transform', type=str, default='imagenet')
    p.add_argument('--extract_feat', type=str2bool, default=False)
    p.add_argument('--run_cluster', type=str2bool, default=False)
    p.add_argument('--cluster', type=str, default='KM', help='options: KM, SSKM, ConSSKM, FINCH (first-neighbour clustering refined to --n_cluster clusters), '
                                                                     'SC (spectral clustering on the exact k-NN graph, see --n_neighbors), '
                                                                     'HDBSCAN (no --n_cluster: the number of clusters is a result, see --min_cluster_size), '
                                                                     'WARD (agglomerative clustering with Ward linkage cut at --n_cluster; the whole tree '
                                                                     'is stored as linkage, so another K needs no refit), '
                                                                     'GMM (a diagonal Gaussian mixture of --n_cluster components, see --covariance_type), '
                                                                     'GMM_FULL, GMM_TIED (a covariance matrix per component, or one for all; rows of at '
                                                                     'most 64 dimensions, see --pca_dim; --covariance_type is not read)')
    p.add_argument('--save_cluster', type=str2bool, default=False)
    p.add_argument('--n_cluster', type=int, default=1000)
    p.add_argument('--n_neighbors', type=int, default=10,
                   help="--cluster SC: neighbours per row of the graph, the row itself included (scikit-learn's n_neighbors), 2 to 65")
    p.add_argument('--min_cluster_size', type=int, default=5, help="--cluster HDBSCAN: scikit-learn's min_cluster_size")
    p.add_argument('--min_samples', type=int, default=None,
                   help="--cluster HDBSCAN: scikit-learn's min_samples, the row itself included, 1 to 65 (default: min_cluster_size)")
    p.add_argument('--covariance_type', type=str, default='diag', choices=['diag', 'spherical'],
                   help="--cluster GMM: scikit-learn's covariance_type, a variance per component and dimension or one per component")
    p.add_argument('--cluster_size_min', type=int, default=50)
    p.add_argument('--cluster_size_max', type=int, default=1200)
    p.add_argument('--corpus', type=str, default='wordnet', help='options: wordnet, wikibird, wikidog')
    p.add_argument('--topk', type=int, default=5)
    p.add_argument('--clip_model', type=str, default='ViT-B/16', choices=clip.available_models(), help='CLIP backbone')
    p.add_argument('--num_common_vote', type=int, default=20)
    p.add_argument('--num_common_linear', type=int, default=4)
    # additions (see the module docstring)
    p.add_argument('--synthetic', type=str2bool, default=False, help='seeded synthetic images / vocabulary')
    p.add_argument('--synthetic_images', type=int, default=8192)
    p.add_argument('--synthetic_vocab', type=int, default=21000)
    p.add_argument('--class_names', type=str, default='', help='JSON {original class name: class index} of the data set')
    p.add_argument('--images_pt', type=str, default='', help='preprocessed images for --extract_feat true')
    p.add_argument('--image_list', type=str, default='', help='CSV path,target,labelled of image files for --extract_feat true')
    p.add_argument('--decode', type=str, default='pil', choices=['pil', 'device'],
                   help="--image_list: decode with Pillow on the host, or baseline JPEGs on the device (same pixels; other files through Pillow)")
    p.add_argument('--pca_dim', type=int, default=0,
                   help='> 0: the clustering features are reduced to this many principal components (scd_amd.pca.PCA fitted on all rows, '
                        'labelled and unlabelled) and renormalised to unit rows before the clustering; 0: off')
    p.add_argument('--pca_whiten', action='store_true', help='--pca_dim: whiten the components (unit variance each) before the renormalisation')
    return p


def pca_tag(args):
    """'' without --pca_dim, else '_pca{M}' ('_pca{M}w' when whitened): the suffix of the names of results computed on reduced features.
    Read with getattr: callers build their own Namespace."""
    m = getattr(args, 'pca_dim', 0)
    return '' if not m else f'_pca{m}' + ('w' if getattr(args, 'pca_whiten', False) else '')


def pca_reduce(args, u_feats, l_feats):
    """--pca_dim M > 0 (docs/design/pca.md): PCA(M, whiten) fitted on ALL rows, labelled first, then each part projected and its rows
    renormalised to unit length, which every clusterer here expects.  Returns (u_feats, l_feats) as float32 numpy arrays [*, M]; without
    the flag both come back untouched.  The naming stage and the CLIP similarities keep the original features."""
    m = getattr(args, 'pca_dim', 0)
    if not m:
        return u_feats, l_feats
    from scd_amd.pca import PCA
    u, l = np.asarray(u_feats, dtype=np.float32), np.asarray(l_feats, dtype=np.float32).reshape(-1, np.shape(u_feats)[1])
    pca = PCA(n_components=m, whiten=getattr(args, 'pca_whiten', False)).fit(np.concatenate([l, u]))
    print(f"PCA: {pca.n_components_} of {u.shape[1]} dimensions keep {pca.explained_variance_ratio_.sum():.4f} of the variance"
          + (", whitened" if pca.whiten else ""))
    return tuple(pca.transform(x, unit=True).cpu().numpy() if len(x) else np.zeros((0, pca.n_components_), np.float32) for x in (u, l))


FULL_COVARIANCE = {'GMM_FULL': 'full', 'GMM_TIED': 'tied'}                     # --cluster value -> FullGaussianMixture's covariance_type


def run_gmm(args, u_feats, l_feats=None, l_targets=None):
    """--cluster GMM (docs/design/gmm.md): scd_amd.gmm.GaussianMixture(n_cluster, covariance_type, random_state=0); --cluster GMM_FULL |
    GMM_TIED (docs/design/gmm_full.md): scd_amd.gmm_full.FullGaussianMixture(n_cluster, 'full' | 'tied', random_state=0).  Without labelled
    rows it is fitted on the unlabelled rows, as KM is.  With them (main_ptsup.py) the labelled rows come first, each clamped to the
    component of its class (the classes numbered in ascending order), and every row gets a label, as SSKM gives."""
    u = np.asarray(u_feats, dtype=np.float32)
    if args.cluster in FULL_COVARIANCE:
        # docs/design/gmm_full.md: a covariance matrix per component (GMM_FULL) or one for all (GMM_TIED); --covariance_type is not read
        from scd_amd.gmm_full import MAX_FEATURES, FullGaussianMixture
        if u.shape[1] > MAX_FEATURES:
            raise SystemExit(f"--cluster {args.cluster}: rows of {u.shape[1]} dimensions; pass --pca_dim M with M <= {MAX_FEATURES}")
        gm = FullGaussianMixture(n_components=args.n_cluster, covariance_type=FULL_COVARIANCE[args.cluster], random_state=0)
    else:
        from scd_amd.gmm import GaussianMixture
        gm = GaussianMixture(n_components=args.n_cluster, covariance_type=args.covariance_type, random_state=0)
    if l_feats is None:
        gm.fit(u)
        print(f"{args.cluster}: {gm.n_iter_} iterations, converged {gm.converged_}, lower bound {gm.lower_bound_:.6f}, BIC {gm.bic(u):.1f}")
        return None, gm.labels_
    classes, y_l = np.unique(np.asarray(l_targets), return_inverse=True)
    if len(classes) > args.n_cluster:
        raise SystemExit(f"--cluster {args.cluster}: {len(classes)} labelled classes need --n_cluster >= {len(classes)} (got {args.n_cluster})")
    x = np.concatenate([np.asarray(l_feats, dtype=np.float32), u])
    y = np.concatenate([y_l.astype(np.int64), np.full(len(u), -1, dtype=np.int64)])
    gm.fit(x, y)
    print(f"{args.cluster}: {len(y_l)} rows clamped to {len(classes)} classes, {gm.n_iter_} iterations, converged {gm.converged_}, "
          f"lower bound {gm.lower_bound_:.6f}")
    return gm.labels_, gm.labels_[len(y_l):]


def run_clustering(args, u_feats, l_feats, l_targets, semi_supervised=False):
    """main_unsup.py:334-364.  Returns (all_preds or None, u_preds numpy).  semi_supervised: --cluster GMM clamps the labelled rows
    (main_ptsup.py); the other methods ignore it."""
    dev = torch.device("cuda")
    if args.cluster == 'ConSSKM':
        km = ConSemiSupKMeans(k=args.n_cluster, tolerance=1e-4, max_iterations=10, init='k-means++', size_min=args.cluster_size_min,
                              size_max=args.cluster_size_max, n_init=10, random_state=None, n_jobs=None, pairwise_batch_size=1024)
    elif args.cluster == 'SSKM':
        km = SemiSupKMeans(k=args.n_cluster, tolerance=1e-4, max_iterations=10, init='k-means++', n_init=10, random_state=None,
                           n_jobs=None, pairwise_batch_size=1024, mode=None)
    elif args.cluster == 'KM':
        # :362 `KMeans(n_clusters=args.n_cluster, random_state=0).fit(u_feats).labels_` - on the device, no host sklearn
        return None, KMeans(n_clusters=args.n_cluster, random_state=0).fit(np.asarray(u_feats, dtype=np.float32)).labels_
    elif args.cluster == 'FINCH':
        # no K-dependent fit: the first-neighbour hierarchy on the unlabelled rows, then req_clust = n_cluster (local_utils/finch.py:164-171)
        from scd_amd.local_utils.finch import FINCH
        _, _, req_c = FINCH(np.asarray(u_feats, dtype=np.float32), req_clust=args.n_cluster, verbose=True)
        return None, req_c.astype(np.int64)
    elif args.cluster == 'SC':
        # sklearn's SpectralClustering(n_clusters, affinity='nearest_neighbors', n_neighbors, random_state=0) on the unlabelled rows: the
        # k-NN graph, its normalised affinity and the eigensolver's sparse products on the device (docs/design/spectral.md)
        from scd_amd.spectral import SpectralClustering
        sc = SpectralClustering(n_clusters=args.n_cluster, n_neighbors=args.n_neighbors, random_state=0)
        return None, sc.fit_predict(np.asarray(u_feats, dtype=np.float32)).astype(np.int64)
    elif args.cluster == 'WARD':
        return None, run_ward(args, u_feats)['u_preds']
    elif args.cluster == 'GMM' or args.cluster in FULL_COVARIANCE:
        return run_gmm(args, u_feats, l_feats, l_targets) if semi_supervised else run_gmm(args, u_feats)
    else:
        raise NotImplementedError(args.cluster)
    u, l, lt = (torch.as_tensor(x).to(dev) for x in (u_feats, l_feats, l_targets))
    km.fit_mix(u.float(), l.float(), lt)
    all_preds = km.labels_.cpu().numpy()
    return all_preds, all_preds[len(l_targets):]


def run_ward(args, u_feats):
    """--cluster WARD on the unlabelled rows (docs/design/ward.md): scikit-learn's AgglomerativeClustering(n_clusters, linkage='ward').
    One fit gives the whole tree; the labels are its cut at n_cluster.  Returns the entries of the result file: u_preds and linkage
    (scipy's Z: scd_amd.ward.cut_tree(linkage, K) gives the labels at any other K without a refit)."""
    from scd_amd.ward import Ward
    w = Ward(n_clusters=args.n_cluster).fit(np.asarray(u_feats, dtype=np.float32))
    print(f"WARD: {w.info_['rounds']} rounds, {w.info_['full_requeries']} full requeries, {w.info_['inversions']} inversions")
    return dict(u_preds=w.labels_, linkage=w.linkage_)


def run_hdbscan(args, u_feats):
    """--cluster HDBSCAN on the unlabelled rows (docs/design/hdbscan.md).  The naming stage needs a full partition, so each noise row
    joins the cluster of its nearest clustered row.  Returns the extra entries of the result file: u_preds (the full partition), noise
    (bool per unlabelled row), probabilities, n_cluster (a RESULT of the fit)."""
    from scd_amd.hdbscan import HDBSCAN, attach_noise
    x = np.asarray(u_feats, dtype=np.float32)
    h = HDBSCAN(min_cluster_size=args.min_cluster_size, min_samples=args.min_samples).fit(x)
    print(f"HDBSCAN: {h.n_clusters_} clusters, {int((h.labels_ < 0).sum())} noise rows of {len(x)}, {h.info_['rounds']} rounds")
    return dict(u_preds=attach_noise(x, h.labels_), noise=h.labels_ < 0, probabilities=h.probabilities_, n_cluster=int(h.n_clusters_))


def cluster_result_name(args):
    """{cluster}_{feat_model}_{dataset}_{n_cluster}.pt; HDBSCAN's result is named by its parameters, the cluster count being a result;
    --pca_dim M appends _pca{M} (_pca{M}w when whitened)."""
    tag = str(args.n_cluster)
    if args.cluster == 'HDBSCAN':
        tag = f'mcs{args.min_cluster_size}' + ('' if args.min_samples is None else f'_ms{args.min_samples}')
    return f'{args.cluster}_{feat_cache_name(args)}_{args.dataset_name}_{tag}{pca_tag(args)}.pt'


def load_or_extract(args, model, feat_model_name, out_name):
    """:294-313: extract with the HIP towers and save, or load the cache."""
    fdir = os.path.join(args.root_dir, 'extracted_features')
    path = os.path.join(fdir, out_name)
    if not args.extract_feat:
        return torch.load(path, weights_only=False)
    if not args.images_pt:
        raise SystemExit("--extract_feat true needs --images_pt or --image_list (the reference's dataset classes are out of scope)")
    blob = torch.load(args.images_pt, weights_only=False)
    images, targets, mask_lab = blob['images'], np.asarray(blob['targets']), np.asarray(blob['mask_lab'])
    args_feat = argparse.Namespace(feat_model=feat_model_name,
                                   train_classes=blob.get('train_classes', sorted(set(targets[mask_lab.astype(bool)].tolist()))))

    def loader():
        for s in range(0, len(images), 256):          # (images, label, uq_idx, mask_lab) like MergedDataset (data_utils.py:12-37)
            yield images[s:s + 256], targets[s:s + 256], None, mask_lab[s:s + 256]
    data = naming.extract_feature(model, loader(), args_feat)
    os.makedirs(fdir, exist_ok=True)
    torch.save(data, path)
    return data


def clip_cache_name(args):
    """'clip' for the default backbone (the reference's cache names), 'clip_vit_l_14' for ViT-L/14."""
    return 'clip' if args.clip_model == 'ViT-B/16' else 'clip_' + clip.backbone_tag(args.clip_model)


def feat_cache_name(args):
    """{feat_model} of the cache names: tagged with the CLIP backbone when the clustering features are CLIP's."""
    return clip_cache_name(args) if args.feat_model == 'clip' else args.feat_model


def extract_or_load_all(args, feat_model, clip_model):
    """The two feature dicts of :294-313 ({feat_model} and clip).  With --extract_feat true and --image_list: both from ONE pass over
    the image files (scd_amd.images), written to the same cache files as load_or_extract writes; otherwise load_or_extract twice."""
    fname, cname = f'{feat_cache_name(args)}_{args.dataset_name}_all.pt', f'{clip_cache_name(args)}_{args.dataset_name}_all.pt'
    if not (args.extract_feat and args.image_list):
        return load_or_extract(args, feat_model, args.feat_model, fname), load_or_extract(args, clip_model, 'clip', cname)
    if args.images_pt:
        raise SystemExit("--images_pt and --image_list are alternatives: pass one")
    from scd_amd import images as img
    paths, targets, mask_lab = img.read_image_list(args.image_list)
    models = {args.feat_model: feat_model, 'clip': clip_model}
    out = img.extract_features_from_files(paths, targets, mask_lab, models, decode=args.decode)
    fdir = os.path.join(args.root_dir, 'extracted_features')
    os.makedirs(fdir, exist_ok=True)
    torch.save(out[args.feat_model], os.path.join(fdir, fname))
    torch.save(out['clip'], os.path.join(fdir, cname))
    return out[args.feat_model], out['clip']


def load_feat_model(args, clip_model):
    """:240-264.  dino_vit / gcd / dinov2_* weights come from $SCD_ROOT (no torch.hub offline)."""
    if args.feat_model == 'clip':
        return clip_model
    if args.feat_model.startswith('dinov2'):
        # $SCD_ROOT/dinov2/{name}_pretrain.pth; an unknown name is a ValueError, a missing file a FileNotFoundError naming the path
        return clip.load_dinov2(args.feat_model, root=os.environ.get("SCD_ROOT", args.root_dir)).cuda()
    from scd_amd.clip import DinoViT
    path = os.path.join(os.environ.get("SCD_ROOT", args.root_dir), 'dino' if args.feat_model == 'dino_vit' else 'gcd',
                        f'{args.feat_model}_{args.dataset_name}.pt' if args.feat_model == 'gcd' else 'dino_vitbase16_pretrain.pth')
    if not os.path.exists(path):
        raise FileNotFoundError(f"{args.feat_model} weights not found at {path}")
    return DinoViT(torch.load(path, map_location='cpu')).cuda()


def zeroshot_path(args):
    zname = {'wordnet': 'nouns', 'wikibird': 'wikibird', 'wikidog': 'wikidog'}[args.corpus]
    return os.path.join(args.root_dir, 'zeroshot_weights', f'zeroshot_weights_all_{zname}_{clip.backbone_tag(args.clip_model)}.pt')


def load_vocabulary(args, dev, model=None):
    """:381-394: nouns + the [embed_dim, V] text classifier (built with `model`'s text tower and saved when a non-default backbone
    has none yet)."""
    nouns = [n.lower().replace('-', '_') for n in get_nouns(corpus=args.corpus)]
    if args.corpus != 'wordnet':
        nouns = [n.lower().replace("'s", "").replace(' ', '_') for n in nouns]
    path = zeroshot_path(args)
    if args.clip_model != 'ViT-B/16' and not os.path.exists(path):
        from local_utils.clip_lang_util import zeroshot_classifier, imagenet_templates
        print(f"building the {args.clip_model} zero-shot classifier of {len(nouns)} names -> {path}")
        zw = zeroshot_classifier(nouns, imagenet_templates, model).cpu()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(zw, path)
    else:
        zw = torch.load(path, weights_only=False)
    return nouns, zw, ops.transpose_f16(torch.as_tensor(zw).to(dev).half())


def wordnet_tables(args):
    """get_wordnet_dict() (:386) when nltk + its corpus are installed; soft sACC is skipped otherwise."""
    if args.corpus != 'wordnet':
        return None
    try:
        from local_utils.clip_lang_util import get_wordnet_dict
        return get_wordnet_dict()
    except Exception as e:          # nltk is an optional host-side dependency
        print(f"(soft sACC disabled: {type(e).__name__}: {e})")
        return None


def main(argv=None):
    args = build_parser().parse_args(argv)
    assert torch.cuda.is_available(), "main_unsup.py needs a HIP device"
    dev = torch.device("cuda")
    if args.synthetic:
        clip.allow_synthetic()
    model, _ = clip.load(args.clip_model)
    model.cuda().eval()
    wn = None

    if args.synthetic:
        k = args.n_cluster
        images, y, base = pipeline.synthetic_images(args.synthetic_images, k, 0, dev)
        clip_all = pipeline.encode_images(model, images, 256)
        wt, nouns = pipeline.synthetic_vocab(model, base, args.synthetic_vocab, 0, dev)
        mask_lab = pipeline.labelled_split(y, k, args.prop_train_labels)
        targets = y.cpu().numpy().astype(np.float64)
        mask_cls = targets < k // 2
        all_feats = clip_all.float().cpu().numpy()
        cidx_to_cname = {c: nouns[c] for c in range(k)}
    else:
        feat_model = load_feat_model(args, model) if args.extract_feat else None
        data, cdata = extract_or_load_all(args, feat_model, model)
        all_feats, mask_lab, mask_cls, targets = data['all_feats'], data['mask_lab'], data['mask_cls'], data['targets']
        clip_all = torch.as_tensor(cdata['all_feats']).to(dev).half()
        nouns, zw, wt = load_vocabulary(args, dev, model)
        cidx_to_cname = None
        if args.class_names:
            with open(args.class_names) as fh:
                class_to_idx = {k: int(v) for k, v in json.load(fh).items()}
            # :398-502: class names that the vocabulary lacks are matched to their closest names by the text tower (row a7)
            cidx_to_cname = naming.resolve_class_names(args.dataset_name, args.corpus, class_to_idx, nouns, wt, model)
        else:
            print("(no --class_names: the semantic accuracies sACC / soft sACC and the name IoU of main_unsup.py:616-647 need the "
                  "data set's class names and are not reported; cluster accuracies and the vote loop run as usual)")
        wn = wordnet_tables(args) if args.dataset_name != 'cub' else None
    mask_lab = np.asarray(mask_lab, dtype=bool)
    l_feats, u_feats = all_feats[mask_lab], all_feats[~mask_lab]
    l_targets, u_targets = targets[mask_lab], targets[~mask_lab]
    mask = np.asarray(mask_cls, dtype=bool)[~mask_lab]

    cdir = os.path.join(args.root_dir, 'cluster')
    cpath = os.path.join(cdir, cluster_result_name(args))
    if args.run_cluster or args.synthetic:
        print(f'Fitting {args.cluster} ...')
        u_feats, l_feats = pca_reduce(args, u_feats, l_feats)
        if args.cluster == 'HDBSCAN':
            cluster_result = dict(all_preds=None, u_targets=u_targets, mask=mask, **run_hdbscan(args, u_feats))
        elif args.cluster == 'WARD':
            cluster_result = dict(all_preds=None, u_targets=u_targets, mask=mask, **run_ward(args, u_feats))
        else:
            all_preds, preds = run_clustering(args, u_feats, l_feats, l_targets)
            cluster_result = dict(all_preds=all_preds, u_preds=preds, u_targets=u_targets, mask=mask)
        if args.save_cluster:
            os.makedirs(cdir, exist_ok=True)
            torch.save(cluster_result, cpath)
    else:
        cluster_result = torch.load(cpath, weights_only=False)
    preds = cluster_result['u_preds']
    if args.cluster == 'HDBSCAN':                               # the number of clusters is a result: the naming stage takes it from here
        args.n_cluster = int(cluster_result['n_cluster'])
        print(f"HDBSCAN: n_cluster = {args.n_cluster}")
        if args.n_cluster == 0:
            raise SystemExit("HDBSCAN found no cluster (every row is noise): nothing to name; try a smaller --min_cluster_size")
    all_acc, old_acc, new_acc = split_cluster_acc_v2(y_true=u_targets, y_pred=preds, mask=mask)
    print(f"{args.cluster} Accuracies: All {all_acc} | Old {old_acc} | New {new_acc}")

    # CLIP voting (main_unsup.py:504-641)
    name_idx, _ = naming.full_vocab_topk(clip_all, None, args.topk, True, wt=wt)
    m = torch.as_tensor(~mask_lab, device=dev)
    soft_cache = {}

    def report(it, cand, u_preds):
        a, o, n = split_cluster_acc_v2(y_true=u_targets, y_pred=u_preds, mask=mask)
        print(f"iter {it}: Accuracies: All {a} | Old {o} | New {n}")
        if cidx_to_cname is None:
            return
        for tag, sel, acc in (("All", slice(None), a), ("old", mask, o), ("new", ~mask, n)):
            s_avg, s_all = naming.evaluate_semantic_acc(u_targets[sel], cidx_to_cname, u_preds[sel], cand)
            print(f"ACC/sACC_avg/sACC_all: {tag} {round(acc * 100, 2)}/{round(s_avg * 100, 2)}/{round(s_all * 100, 2)} ")
        if wn is not None:
            for tag, sel, acc in (("All", slice(None), a), ("old", mask, o), ("new", ~mask, n)):
                soft = naming.evaluate_soft_semantic_acc(u_targets[sel], cidx_to_cname, u_preds[sel], cand, wn[0], wn[2], cache=soft_cache)
                print(f"ACC/Soft sACC: {tag} {round(acc * 100, 2)}/{round(soft * 100, 2)}")

    cand, u_preds, trace = naming.vote_loop_unsup(name_idx[m], preds, clip_all[m], wt, nouns, args.n_cluster,
                                                  args.num_common_vote, args.num_common_linear, on_iter=report)
    print(f"voting converged after {len(trace)} iterations; {len(set(cand))} names")
    if cidx_to_cname is not None:       # :643-647 IoU of predicted names and GT names
        gt_names = list(cidx_to_cname.values())
        inter, union = set(cand) & set(gt_names), set(cand) | set(gt_names)
        print(f'IoU: {len(inter) * 1.0 / len(union)}')
    return cand, u_preds


if __name__ == "__main__":
    main()
