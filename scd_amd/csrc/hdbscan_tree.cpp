// scd_hdbscan_tree: from the sorted edges of a spanning tree to HDBSCAN's labels and membership strengths, on the host.  It restates
// scikit-learn 1.7.2's sklearn/cluster/_hdbscan/_linkage.pyx (make_single_linkage) and _tree.pyx (tree_to_labels: _condense_tree,
// _compute_stability, _get_clusters, _do_labelling, get_probabilities) at cluster_selection_epsilon = 0, max_cluster_size = None, decision
// for decision and sum for sum, so that labels, cluster numbering and probabilities are scikit-learn's (docs/design/hdbscan.md).
//
// Same decisions, different machinery: every traversal is a loop over an explicit queue (a path-shaped tree is as deep as it is long), the
// descendants of a chosen cluster are struck out in one top-down sweep instead of one search per chosen cluster, and a point finds its
// cluster through the condensed tree's parent links instead of a union-find over 2n nodes.  O(n alpha(n)) time, O(n) memory.
#include "common.h"
#include <cmath>
#include <limits>
#include <vector>

namespace {
struct Cond {                       // a row of the condensed tree: `child` leaves (a point) or splits off (a cluster) `parent` at lambda
    int64_t parent, child;
    double lambda;
    int64_t size;
};

int64_t uf_find(std::vector<int64_t>& par, int64_t x) {
    int64_t r = x;
    while (par[r] != r) r = par[r];
    while (par[x] != r) {
        const int64_t nx = par[x];
        par[x] = r;
        x = nx;
    }
    return r;
}
}  // namespace

extern "C" int scd_hdbscan_tree(const int32_t* lo, const int32_t* hi, const double* weight, int64_t n, int min_cluster_size, int method,
                                int allow_single_cluster, int32_t* labels_out, double* prob_out, int32_t* n_clusters_out) {
    SCD_REQUIRE(lo && hi && weight && labels_out && prob_out && n_clusters_out, "scd_hdbscan_tree: null argument");
    SCD_REQUIRE(n >= 2 && n < (1ll << 30), "scd_hdbscan_tree: n = %lld outside [2, 2^30)", (long long)n);
    SCD_REQUIRE(min_cluster_size >= 2, "scd_hdbscan_tree: min_cluster_size = %d must be at least 2", min_cluster_size);
    SCD_REQUIRE(method == 0 || method == 1, "scd_hdbscan_tree: method %d (0 eom, 1 leaf)", method);
    const int64_t mcs = min_cluster_size, ne = n - 1, root = 2 * ne;
    const double inf = std::numeric_limits<double>::infinity();

    // ---- make_single_linkage: the union of edge e's two sides is node n + e
    std::vector<int64_t> left(ne), right(ne), hsize(ne), par(2 * n - 1), usize(2 * n - 1, 1);
    for (int64_t v = 0; v < 2 * n - 1; ++v) par[v] = v;
    for (int64_t e = 0; e < ne; ++e) {
        SCD_REQUIRE(lo[e] >= 0 && lo[e] < n && hi[e] >= 0 && hi[e] < n, "scd_hdbscan_tree: edge %lld has an end outside [0, n)", (long long)e);
        SCD_REQUIRE(!(weight[e] != weight[e]), "scd_hdbscan_tree: edge %lld has a NaN weight", (long long)e);
        const int64_t a = uf_find(par, lo[e]), b = uf_find(par, hi[e]);
        SCD_REQUIRE(a != b, "scd_hdbscan_tree: edge %lld closes a cycle: the edges are no spanning tree", (long long)e);
        left[e] = a;
        right[e] = b;
        hsize[e] = usize[a] + usize[b];
        par[a] = par[b] = n + e;
        usize[n + e] = hsize[e];
    }
    // n - 1 edges without a cycle on n nodes: a spanning tree

    // ---- _condense_tree: breadth first from the root; a side smaller than min_cluster_size falls out point by point
    std::vector<int64_t> order;                                 // bfs_from_hierarchy(root)
    order.reserve(2 * n - 1);
    order.push_back(root);
    for (size_t q = 0; q < order.size(); ++q)
        if (order[q] >= n) {
            order.push_back(left[order[q] - n]);
            order.push_back(right[order[q] - n]);
        }
    std::vector<int64_t> relabel(root + 1, -1), sub;
    std::vector<char> ignore(root + 1, 0);
    std::vector<Cond> ct;
    ct.reserve(n + 16);
    relabel[root] = n;
    int64_t next_label = n + 1;
    auto fall_out = [&](int64_t from, int64_t parent, double lambda) {
        sub.clear();
        sub.push_back(from);
        for (size_t q = 0; q < sub.size(); ++q) {
            const int64_t s = sub[q];
            if (s < n) ct.push_back({parent, s, lambda, 1});
            else {
                sub.push_back(left[s - n]);
                sub.push_back(right[s - n]);
            }
            ignore[s] = 1;
        }
    };
    for (size_t q = 0; q < order.size(); ++q) {
        const int64_t node = order[q];
        if (ignore[node] || node < n) continue;
        const int64_t l = left[node - n], r = right[node - n];
        const double dist = weight[node - n];
        const double lambda = dist > 0.0 ? 1.0 / dist : inf;
        const int64_t lc = l >= n ? hsize[l - n] : 1, rcount = r >= n ? hsize[r - n] : 1;
        if (lc >= mcs && rcount >= mcs) {
            relabel[l] = next_label++;
            ct.push_back({relabel[node], relabel[l], lambda, lc});
            relabel[r] = next_label++;
            ct.push_back({relabel[node], relabel[r], lambda, rcount});
        } else if (lc < mcs && rcount < mcs) {
            fall_out(l, relabel[node], lambda);
            fall_out(r, relabel[node], lambda);
        } else if (lc < mcs) {
            relabel[r] = relabel[node];
            fall_out(l, relabel[node], lambda);
        } else {
            relabel[l] = relabel[node];
            fall_out(r, relabel[node], lambda);
        }
    }
    const int64_t rows = (int64_t)ct.size(), nclu = next_label - n;  // clusters n .. next_label - 1; the root is n; every one is a parent
    auto K = [&](int64_t c) { return c - n; };

    // ---- _compute_stability
    std::vector<double> birth(nclu, std::nan("")), stab(nclu, 0.0);
    std::vector<int64_t> cparent(nclu, -1);
    std::vector<char> is_parent(nclu, 0);
    for (const Cond& c : ct) {
        is_parent[K(c.parent)] = 1;
        if (c.child >= n) {
            birth[K(c.child)] = c.lambda;
            cparent[K(c.child)] = c.parent;
        }
    }
    birth[0] = 0.0;
    for (const Cond& c : ct) stab[K(c.parent)] += (c.lambda - birth[K(c.parent)]) * (double)c.size;

    // the two children of a cluster, in row order (np.sum over them is their sum in that order)
    std::vector<int64_t> kid0(nclu, -1), kid1(nclu, -1);
    for (const Cond& c : ct)
        if (c.child >= n) (kid0[K(c.parent)] < 0 ? kid0[K(c.parent)] : kid1[K(c.parent)]) = c.child;

    // ---- _get_clusters
    std::vector<char> chosen(nclu, 0);
    const int64_t first = allow_single_cluster ? 0 : 1;         // without allow_single_cluster the root is no candidate
    if (method == 0) {                                          // excess of mass: children before parents (larger ids first)
        std::vector<char> own(nclu, 0);
        for (int64_t k = nclu - 1; k >= first; --k) {
            double subtree = 0.0;
            if (kid0[k] >= 0) subtree += stab[K(kid0[k])];
            if (kid1[k] >= 0) subtree += stab[K(kid1[k])];
            if (subtree > stab[k]) stab[k] = subtree;
            else own[k] = 1;
        }
        std::vector<char> under(nclu, 0);                       // below a chosen cluster: ids grow downwards, so one ascending sweep
        for (int64_t k = first; k < nclu; ++k) {
            const int64_t p = cparent[k] >= 0 ? K(cparent[k]) : -1;
            if (p >= 0 && (under[p] || chosen[p])) under[k] = 1;
            chosen[k] = own[k] && !under[k];
        }
    } else {                                                    // the leaves of the cluster tree; none when no cluster ever split
        if (nclu > 1)
            for (int64_t k = 1; k < nclu; ++k) chosen[k] = kid0[k] < 0;
    }
    std::vector<int32_t> label_of(nclu, -1);
    int32_t n_clusters = 0;
    for (int64_t k = 0; k < nclu; ++k)
        if (chosen[k]) label_of[k] = n_clusters++;

    // ---- _do_labelling: a point belongs to the nearest chosen cluster above it; what reaches the root is noise, except ...
    std::vector<int64_t> top(nclu);
    for (int64_t k = 0; k < nclu; ++k) top[k] = (k == 0 || chosen[k]) ? k : top[K(cparent[k])];
    double root_max = -inf;                                     // ... with one cluster allowed: the root's points of the largest lambda
    for (const Cond& c : ct)
        if (c.parent == n && c.lambda > root_max) root_max = c.lambda;
    for (int64_t i = 0; i < n; ++i) {
        labels_out[i] = -1;
        prob_out[i] = 0.0;
    }
    std::vector<char> seen(n, 0);
    for (const Cond& c : ct) {
        if (c.child >= n) continue;
        seen[c.child] = 1;
        const int64_t t = top[K(c.parent)];
        if (t != 0) labels_out[c.child] = label_of[t];
        else if (n_clusters == 1 && allow_single_cluster && chosen[0] && c.lambda >= root_max) labels_out[c.child] = label_of[0];
    }
    for (int64_t i = 0; i < n; ++i) SCD_REQUIRE(seen[i], "scd_hdbscan_tree: point %lld is in no edge: the edges are no spanning tree", (long long)i);

    // ---- get_probabilities, with max_lambdas' rule: a cluster's death is the largest lambda of its LAST run of consecutive rows
    std::vector<double> death(nclu, 0.0);
    {
        int64_t cur = ct[0].parent;
        double mx = ct[0].lambda;
        for (int64_t q = 1; q < rows; ++q) {
            if (ct[q].parent == cur) mx = ct[q].lambda > mx ? ct[q].lambda : mx;     // Python's max(max_lambda, lambda_val)
            else {
                death[K(cur)] = mx;
                cur = ct[q].parent;
                mx = ct[q].lambda;
            }
        }
        death[K(cur)] = mx;
    }
    std::vector<int64_t> cluster_of(n_clusters > 0 ? n_clusters : 1, 0);
    for (int64_t k = 0; k < nclu; ++k)
        if (chosen[k]) cluster_of[label_of[k]] = k;
    for (const Cond& c : ct) {
        if (c.child >= n || labels_out[c.child] < 0) continue;
        const double mx = death[cluster_of[labels_out[c.child]]];
        if (mx == 0.0 || std::isinf(c.lambda)) prob_out[c.child] = 1.0;
        else prob_out[c.child] = (c.lambda < mx ? c.lambda : mx) / mx;               // Python's min(lambda, max_lambda)
    }
    *n_clusters_out = n_clusters;
    return SCD_OK;
}
