// Sanitizer driver for the host solver scd_hdbscan_tree (scd_amd/csrc/hdbscan_tree.cpp), built by
// tests/test_hdbscan_host.py::test_tree_under_sanitizers with clang's AddressSanitizer + UndefinedBehaviorSanitizer (host compilation
// only, run on the CPU).  Paths, stars and random spanning trees with random, tied and zero weights at every parameter combination,
// checked against the invariants of the output, and the inputs that must be refused; any sanitizer report aborts the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "scd_hip.h"

static thread_local char g_err[512];
extern "C" const char* scd_last_error(void) { return g_err; }
void scd_set_error(const char* fmt, ...) {      // api.cpp's definition lives beside the HIP entry points; the solver only reports through it
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
static uint64_t rs = 88172645463325252ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }

// every parameter combination on one tree; returns the number of broken invariants
static int drive(const std::vector<int32_t>& lo, const std::vector<int32_t>& hi, const std::vector<double>& w) {
    const int64_t n = (int64_t)lo.size() + 1;
    int fails = 0;
    for (int mcs : {2, 5, 15})
        for (int method = 0; method < 2; ++method)
            for (int single = 0; single < 2; ++single) {
                std::vector<int32_t> lab(n, -7);
                std::vector<double> prob(n, -1.0);
                int32_t k = -1;
                if (scd_hdbscan_tree(lo.data(), hi.data(), w.data(), n, mcs, method, single, lab.data(), prob.data(), &k) != 0) { ++fails; continue; }
                if (k < 0 || k > n / mcs + 1) ++fails;
                std::vector<int64_t> size(k > 0 ? k : 1, 0);
                for (int64_t i = 0; i < n; ++i) {
                    if (lab[i] < -1 || lab[i] >= k) { ++fails; break; }
                    if (lab[i] >= 0) ++size[lab[i]];
                    if (lab[i] < 0 && prob[i] != 0.0) ++fails;
                    if (prob[i] == prob[i] && (prob[i] < 0.0 || prob[i] > 1.0)) ++fails;      // NaN is scikit-learn's answer at inf / inf
                }
                for (int c = 0; c < k; ++c) if (size[c] == 0) ++fails;                         // every numbered cluster has a member
            }
    return fails;
}

int main() {
    int fails = 0;
    for (int trial = 0; trial < 120; ++trial) {
        const int64_t n = 2 + rnd() % (trial < 100 ? 60 : 3000);
        const int kind = trial % 3, shape = (trial / 3) % 3;           // weights: random, tied, with zeros; shape: random, path, star
        std::vector<int32_t> perm(n), lo(n - 1), hi(n - 1);
        std::iota(perm.begin(), perm.end(), 0);
        for (int64_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[rnd() % (i + 1)]);
        std::vector<double> w(n - 1);
        for (int64_t e = 0; e < n - 1; ++e) {
            const int32_t a = perm[e + 1], b = shape == 0 ? perm[rnd() % (e + 1)] : shape == 1 ? perm[e] : perm[0];
            lo[e] = std::min(a, b);
            hi[e] = std::max(a, b);
            w[e] = kind == 0 ? (1 + rnd() % 100000) / 100000.0 : kind == 1 ? (1 + rnd() % 5) / 4.0 : (rnd() % 3 == 0 ? 0.0 : (1 + rnd() % 3) / 2.0);
        }
        std::vector<int64_t> order(n - 1);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
            return w[x] != w[y] ? w[x] < w[y] : lo[x] != lo[y] ? lo[x] < lo[y] : hi[x] < hi[y];
        });
        std::vector<int32_t> slo(n - 1), shi(n - 1);
        std::vector<double> sw(n - 1);
        for (int64_t e = 0; e < n - 1; ++e) { slo[e] = lo[order[e]]; shi[e] = hi[order[e]]; sw[e] = w[order[e]]; }
        fails += drive(slo, shi, sw);
    }
    {   // a path as long as the largest fit: no recursion, no stack to overflow
        const int64_t n = 126976;
        std::vector<int32_t> lo(n - 1), hi(n - 1);
        std::vector<double> w(n - 1);
        for (int64_t e = 0; e < n - 1; ++e) { lo[e] = (int32_t)e; hi[e] = (int32_t)e + 1; w[e] = 0.1 + 1e-6 * (double)e; }
        fails += drive(lo, hi, w);
    }
    {   // what must be refused, outputs untouched or not: no write outside them either way
        std::vector<int32_t> lo = {0, 1, 2}, hi = {1, 2, 3}, lab(4);
        std::vector<double> w = {0.1, 0.2, 0.3}, prob(4);
        int32_t k = 0;
        if (scd_hdbscan_tree(lo.data(), hi.data(), w.data(), 4, 2, 0, 0, lab.data(), prob.data(), &k) != 0) ++fails;
        if (scd_hdbscan_tree(lo.data(), hi.data(), w.data(), 1, 2, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;      // n < 2
        if (scd_hdbscan_tree(lo.data(), hi.data(), w.data(), 4, 1, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;      // min_cluster_size < 2
        if (scd_hdbscan_tree(lo.data(), hi.data(), w.data(), 4, 2, 2, 0, lab.data(), prob.data(), &k) == 0) ++fails;      // no such method
        std::vector<int32_t> cyc = {1, 2, 0}, out = {1, 2, 4}, neg = {0, -1, 2};
        if (scd_hdbscan_tree(lo.data(), cyc.data(), w.data(), 4, 2, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;     // a cycle
        if (scd_hdbscan_tree(lo.data(), out.data(), w.data(), 4, 2, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;     // index n
        if (scd_hdbscan_tree(neg.data(), hi.data(), w.data(), 4, 2, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;     // index -1
        if (scd_hdbscan_tree(nullptr, hi.data(), w.data(), 4, 2, 0, 0, lab.data(), prob.data(), &k) == 0) ++fails;
    }
    printf("sanitize_hdbscan: %d failures\n", fails);
    return fails ? 1 : 0;
}
