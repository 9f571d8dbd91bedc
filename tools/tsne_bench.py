"""Times the exact t-SNE (scd_amd.tsne, csrc/tsne.hip) at the project's sizes and writes profiles/tsne_bench.json.  Nothing is asserted on time.

  python tools/tsne_bench.py [--sizes 50000 126976] [--dim 768] [--perplexity 30] [--out profiles/tsne_bench.json]
      per size: graph + calibration + joint matrix, one whole fit_transform, ms per iteration from device events over --iters
      iterations of gradient + update (profiler off), workspace bytes, the board's shader clock over that window (bench.PowerSampler),
      and the repulsion kernel's instruction-count floor at that clock.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tsne_bench.py --child --n 126976
      the traced run, in a process of its own: the same iterations, nothing timed by the host.
  python tools/tsne_bench.py --stats DIR/.../kernel_stats.csv --n 126976 [--out ...]
      folds the trace's per-kernel times into the JSON: ms per iteration split into repulse / attract / update / the rest.

The floor.  A pair costs the repulsion kernel 9 vector instructions (2 subtractions, 4 fused multiply-adds, v_rcp_f32, a product, an
addition); v_rcp_f32 takes two issue slots (MI355X: 8 cycles against 4 for one wave), so 10 slots, plus one LDS broadcast read per 4 pairs.
A wave-instruction occupies a SIMD for 2 cycles and serves 64 pairs: floor = pairs * 10 * 2 / 64 cycles / (CUs * 4 SIMDs).
"""
import argparse
import csv
import json
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS_PER_PAIR, FLOP_PER_PAIR = 10, 13                         # 13: 2 sub + 4 fma (2 each) + rcp + mul + add
PEAK_FP32_TFLOPS = 157.3


def rows(n, d, seed=0):
    """Unit blob rows generated on the device from a seed: 100 classes, noise 0.6 / sqrt(d) per coordinate."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(100, d, generator=g, device="cuda"), dim=1)
    y = torch.randint(0, 100, (n,), generator=g, device="cuda")
    return torch.nn.functional.normalize(centres[y] + 0.6 / d ** 0.5 * torch.randn(n, d, generator=g, device="cuda"), dim=1).contiguous()


def iteration_state(x, perplexity):
    import torch
    from scd_amd import knn, ops, tsne
    P = tsne.joint_affinities(x, perplexity)
    n = x.shape[0]
    y64 = tsne.pca_init(knn.unit_rows(x)).contiguous()
    y32 = y64.float().contiguous()
    nb = ops._L().scd_tsne_gradient_ws_bytes(n, P[1].numel())
    return P, (y32.double(), torch.zeros_like(y64), torch.ones_like(y64), y32), ops._ws(max(nb, 16), x.device), nb


def iterate(P, st, ws, iters, lr):
    from scd_amd import ops
    y64, vel, gains, y32 = st
    for i in range(iters):
        grad, _, _, _ = ops.tsne_gradient(y32, P[0], P[1], P[2], 12.0, want_kl=(i + 1) % 50 == 0, ws=ws)
        ops.tsne_update(grad, y64, vel, gains, y32, 0.5, lr)


def measure(n, d, perplexity, iters):
    import torch
    import bench
    from scd_amd import tsne
    x = rows(n, d)
    torch.cuda.synchronize()
    tsne.joint_affinities(x[:4096], perplexity)                 # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P, st, ws, nb = iteration_state(x, perplexity)
    torch.cuda.synchronize()
    t_graph = time.perf_counter() - t0
    lr = max(n / 12.0 / 4.0, 50.0)
    iterate(P, st, ws, 20, lr)
    torch.cuda.synchronize()
    sampler = bench.PowerSampler(0)
    sampler.start()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    iterate(P, st, ws, iters, lr)
    e1.record()
    torch.cuda.synchronize()
    power = sampler.stop()
    ms_iter = e0.elapsed_time(e1) / iters
    t0 = time.perf_counter()
    t = tsne.TSNE(perplexity=perplexity, random_state=0)
    t.fit_transform(x)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sclk = (power or {}).get("sclk_mhz_median")
    pairs = float(n) * (n - 1)
    floor_ms = pairs * SLOTS_PER_PAIR * 2 / 64 / (cus * 4) / (sclk * 1e3) if sclk else None
    return dict(n=n, d=d, perplexity=perplexity, k=P[3]["k"], nnz=int(P[1].numel()), info=P[3], graph_calibration_joint_s=round(t_graph, 4),
                ms_per_iteration=round(ms_iter, 4), iterations_timed=iters, fit_transform_s=round(t_fit, 3), fit_n_iter=int(t.n_iter_),
                fit_kl=t.kl_divergence_, workspace_bytes=int(nb), board_power=power, compute_units=cus,
                repulse_floor_ms_at_sclk=None if floor_ms is None else round(floor_ms, 4),
                note="floor: pairs * 10 issue slots * 2 cycles / 64 lanes / (CUs * 4 SIMDs) at the median shader clock of the timed window")


def fold_stats(path, n, iters, out):
    groups = {"repulse": 0.0, "attract": 0.0, "update": 0.0, "rest_of_gradient": 0.0}
    calls = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            if "tsne_repulse" in name:
                key = "repulse"
            elif "tsne_attract" in name:
                key = "attract"
            elif "tsne_update" in name:
                key = "update"
            elif "tsne_finish" in name or "tsne_reduce" in name or "tsne_combine" in name:
                key = "rest_of_gradient"
            else:
                continue
            groups[key] += ns
            calls[key] = calls.get(key, 0) + int(row["Calls"])
    js = json.load(open(out)) if os.path.exists(out) else {"sizes": []}
    per_iter = {k: round(v / 1e6 / max(calls.get(k, 1) / (3 if k == "rest_of_gradient" else 1), 1), 4) for k, v in groups.items()}
    for rec in js["sizes"]:
        if rec["n"] == n:
            rec["kernel_trace_ms_per_iteration"] = per_iter
            rec["kernel_trace_calls"] = calls
            fl, rep = rec.get("repulse_floor_ms_at_sclk"), per_iter["repulse"]
            if fl and rep:
                rec["repulse_share_of_floor"] = round(fl / rep, 3)
                rec["repulse_tflops"] = round(float(n) * (n - 1) * FLOP_PER_PAIR / (rep * 1e-3) / 1e12, 1)
                rec["repulse_share_of_fp32_vector_peak"] = round(rec["repulse_tflops"] / PEAK_FP32_TFLOPS, 3)
    with open(out, "w") as fh:
        json.dump(js, fh, indent=1)
    print(json.dumps(per_iter))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 126976])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int, default=126976)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        return fold_stats(a.stats, a.n, a.iters, a.out)
    import torch
    assert torch.cuda.is_available(), "tsne_bench.py needs a HIP device"
    if a.child:
        P, st, ws, _ = iteration_state(rows(a.n, a.dim), a.perplexity)
        iterate(P, st, ws, a.iters, max(a.n / 48.0, 50.0))
        torch.cuda.synchronize()
        return
    js = {"device": torch.cuda.get_device_name(0), "sizes": [measure(n, a.dim, a.perplexity, a.iters) for n in a.sizes]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(js, fh, indent=1)
    print(json.dumps(js))


if __name__ == "__main__":
    main()
