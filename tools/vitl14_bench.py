"""CLIP ViT-L/14 on one MI355X: image tower images/s (batch 256, synthetic weights, warm), text tower prompts/s, and the d = 768
similarity + top-k call at the bench's shape (n = 126,976, V = 21,000, k = 5, softmax).  Each with its algorithmic FLOP from shapes and
the fraction of the 2.5 PFLOP/s dense fp16 peak; the board's shader clock over the timed windows as bench.py records it.

  python tools/vitl14_bench.py [--only tower|text|sim] [--reps N]       -> one JSON line
  python tools/vitl14_bench.py --stats KERNEL_STATS_CSV                  -> kernel-time shares of a rocprofv3 --kernel-trace --stats run
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 2.5e15                      # MI355X dense fp16 MFMA FLOP/s (MI355X_MICROARCH.md)


def tower_flop_per_image(cfg):
    """2 x MACs of the ViT-L/14 image tower: patch GEMM (K = 3 P^2), per block QKV + proj + MLP (12 w^2 per token) and Q K^T + P V
    (2 T^2 w), the CLS row's projection."""
    w, p = cfg["v_width"], cfg["patch"]
    t = (cfg["image"] // p) ** 2 + 1
    mac = (t - 1) * 3 * p * p * w + cfg["v_layers"] * (t * 12 * w * w + 2 * t * t * w) + w * cfg["embed_dim"]
    return 2.0 * mac


def text_flop(cfg, n, ctx):
    w = cfg["t_width"]
    return 2.0 * n * (cfg["t_layers"] * (ctx * 12 * w * w + 2 * ctx * ctx * w) + w * cfg["embed_dim"])


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def stats(path):
    """Kernel-time shares from rocprofv3's kernel_stats.csv (Name, TotalDurationNs)."""
    tot, groups = 0.0, {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            ns = float(row["TotalDurationNs"])
            name = row["Name"]
            tot += ns
            key = next((g for g in ("attention", "sim_topk", "sim_refine", "sim_exact", "gemm", "im2col", "layernorm") if g in name), "other")
            groups[key] = groups.get(key, 0.0) + ns
    return {"total_ms": round(tot / 1e6, 3), "share": {k: round(v / tot, 4) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])},
            "ms": {k: round(v / 1e6, 3) for k, v in groups.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["tower", "text", "sim"], default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats)))
        return
    import bench
    from scd_amd import ops
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP
    assert torch.cuda.is_available(), "vitl14_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    cfg = W.CLIP_VITL14
    out = {"model": "ViT-L/14", "peak_flops": PEAK, "weights": "synthetic seed 0"}
    power = bench.PowerSampler(0)
    power.start()
    if a.only in (None, "tower", "text"):
        model = CLIP(W.synthetic_clip_state_dict(seed=0, cfg=cfg, visual=a.only != "text", text=a.only != "tower")).cuda()
    if a.only in (None, "tower"):
        batch = 256
        x = torch.randn((batch, 3, 224, 224), device=dev, generator=torch.Generator(device=dev).manual_seed(0)).half()
        enc = model.visual.enc
        enc.encode_image(x)
        s = timed(lambda: enc.encode_image(x), a.reps)
        f = tower_flop_per_image(cfg) * batch
        out["image_tower"] = {"batch": batch, "ms_per_batch": round(s * 1e3, 3), "images_per_s": round(batch / s, 1),
                              "gflop_per_image": round(tower_flop_per_image(cfg) / 1e9, 2), "peak_fraction": round(f / s / PEAK, 4),
                              "target_images_per_s": 6100}
    if a.only in (None, "text"):
        n = 20480                                     # 256 names x 80 templates; prompts of 8-19 tokens, SOT / EOT around them
        rs = np.random.RandomState(1)
        tok = torch.zeros(n, 77, dtype=torch.int32)
        lens = rs.randint(8, 20, size=n)
        for i, ln in enumerate(lens):
            tok[i, 0] = 49406
            tok[i, 1:1 + ln] = torch.from_numpy(rs.randint(1, 49405, size=ln).astype(np.int32))
            tok[i, 1 + ln] = 49407
        ctx = int(lens.max()) + 2
        td = tok.cuda()
        s = timed(lambda: model._text.encode_text(td, ctx_len=ctx), a.reps)
        f = text_flop(cfg, n, ctx)
        out["text_tower"] = {"prompts": n, "ctx_len": ctx, "ms": round(s * 1e3, 3), "prompts_per_s": round(n / s, 1),
                             "gflop": round(f / 1e9, 1), "peak_fraction": round(f / s / PEAK, 4)}
    if a.only in (None, "sim"):
        n, v, d, k = 126976, 21000, 768, 5
        g = torch.Generator(device=dev).manual_seed(2)
        f16 = torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=g), dim=-1).half()
        wt = ops.freeze_vocab(torch.nn.functional.normalize(torch.randn(v, d, device=dev, generator=g), dim=-1).half().contiguous())
        res = {}

        def call():
            res["r"] = ops.sim_topk(f16, wt, k, "softmax", return_fallback=True)
        s = timed(call, a.reps)
        fl = 2.0 * n * v * d
        out["sim_topk"] = {"n": n, "v": v, "d": d, "k": k, "mode": "softmax", "ms": round(s * 1e3, 3), "tflop": round(fl / 1e12, 3),
                           "peak_fraction": round(fl / s / PEAK, 4), "fallback_rows": int(res["r"][2].item()), "target_ms": 4.3}
    out["board_power"] = power.stop()
    out["sclk_mhz_median"] = (out["board_power"] or {}).get("sclk_mhz_median")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
