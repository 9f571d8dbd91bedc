"""What the mains and the figures use of the reference's local_utils/util.py: str2bool (:276) and the t-SNE scatter plots save_tsne /
save_tsne_wcolor (:178-216), restated on scd_amd.tsne.TSNE - the exact gradient on the device in place of scikit-learn's Barnes-Hut
(docs/design/tsne.md)."""
import argparse

import numpy as np


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def _embed(embeddings):
    from ..tsne import TSNE
    return TSNE(n_components=2, random_state=0).fit_transform(embeddings)


def scatter_png(X_2d, labels, path, colors=None, marker_sz=5, font_size=None, names=None):
    """One scatter series per distinct label, the legend to the right of the axes, equal axis scales, a tight PNG at `path`.  colors: one
    per label in order, or None for a shuffled gist_ncar map (the reference draws np.random.shuffle from the global generator there);
    names: {label: legend text}, the label itself where absent."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from matplotlib.colors import ListedColormap
    labels = np.asarray(labels)
    label_names = np.unique(labels).astype(int)
    with plt.rc_context({'font.size': font_size} if font_size else {}):
        fig = plt.figure(figsize=(8, 6))
        if colors is None:
            vals = np.linspace(0, 1, len(label_names))
            np.random.shuffle(vals)
            cmap = ListedColormap(plt.cm.gist_ncar(vals))
            colors = [cmap(i) for i in range(len(label_names))]
        elif len(label_names) > len(colors):
            raise ValueError("%d labels but %d colours" % (len(label_names), len(colors)))
        for i, name in enumerate(label_names):
            sel = labels == name
            plt.scatter(X_2d[sel, 0], X_2d[sel, 1], color=colors[i], label=(names or {}).get(int(name), name), s=marker_sz)
        plt.legend(loc='center left', bbox_to_anchor=(1, 0.5))
        plt.axis('equal')
        plt.savefig(path, bbox_inches='tight', format='png')
        plt.close(fig)


def save_tsne(embeddings, labels, path='tsne.png'):
    scatter_png(_embed(embeddings), labels, path, marker_sz=5)


WCOLORS = ('r', 'g', 'b', 'c', 'm', 'y', 'k', 'springgreen', 'orange', 'purple')


def save_tsne_wcolor(embeddings, labels, path='tsne.png'):
    """At most ten labels, in the reference's ten fixed colours, larger markers and font."""
    scatter_png(_embed(embeddings), labels, path, colors=WCOLORS, marker_sz=10, font_size=18)
