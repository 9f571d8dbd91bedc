"""Images/s of the CLIP ViT-B/16 image tower and of the DINO / GCD ViT-B/16 tower on the same box, same launch size (round 6: the
DINO tower is --feat_model dino_vit of both shipped scripts, main_unsup.py:240-255; its fc1 epilogue is exact GELU).

  python tools/tower_bench.py [launches] [batch] [both|clip|dino|dinov2]
        -> one JSON line; fc1 launches bracketed by HIP events (scd_encoder_timing)

`dinov2`: the four DINOv2 towers (ViT-B/14, ViT-L/14, with and without the four register tokens; docs/design/dinov2.md) beside DINO
ViT-B/16, each with its images/s and the fraction of the fp16 peak (2.5 PFLOP/s) its algorithmic FLOPs reach, and the token-assembly
launch (scd_vit_assemble_f16) with and without registers.
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scd_amd import ops                                    # noqa: E402
from scd_amd.clip import weights as W                      # noqa: E402
from scd_amd.clip.model import CLIP, DinoViT               # noqa: E402

PEAK_FP16 = 2.5e15


def tower_flop_per_image(desc):
    """Algorithmic FLOPs of one image through every block in full (2 per multiply-add): patch GEMM, per block the QKV / proj / fc1 / fc2
    GEMMs (24 T W^2 with mlp_dim = 4 W) and the attention's Q K^T and P V (4 T^2 W)."""
    T, w = desc["tokens"], desc["width"]
    n_p = (desc["image"] // desc["patch"]) ** 2
    block = 2.0 * T * w * (4 * w + 2 * desc["mlp_dim"]) + 4.0 * T * T * w
    return 2.0 * n_p * w * 3 * desc["patch"] ** 2 + desc["layers"] * block


def time_assembly(batch, width, registers, reps=5):
    """microseconds per scd_vit_assemble_f16 launch (statistics on), 256 patches + 1 + registers tokens"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    T = 257 + registers
    patch = torch.randn((batch * 256, width), device=dev, generator=g).half()
    vec = lambda *s: torch.randn(s, device=dev, generator=g)
    bias, cls, pos = vec(width), vec(width), vec(257, width)
    reg = vec(registers, width) if registers else None
    ops.vit_assemble_f16(patch, bias, cls, pos, reg, batch, T, stats=True)
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.vit_assemble_f16(patch, bias, cls, pos, reg, batch, T, stats=True)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3)
    return round(best, 1)


def main():
    launches = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 3990
    which = sys.argv[3] if len(sys.argv) > 3 else "both"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((batch, 3, 224, 224), device=dev, generator=g, dtype=torch.float32).half()
    towers = []
    if which in ("both", "clip"):
        clip = CLIP(W.synthetic_clip_state_dict(seed=0, text=False)).cuda()
        towers.append(("clip", clip.visual.enc))
    if which in ("both", "dino", "dinov2"):
        dino = DinoViT(W.synthetic_dino_state_dict(seed=1, layers=12)).cuda()
        towers.append(("dino", dino._enc))
    if which == "dinov2":
        for name, cfg in W.DINOV2.items():
            towers.append((name, DinoViT(W.synthetic_dinov2_state_dict(seed=2, **cfg)).cuda()._enc))
    out = {"batch": batch, "launches": launches, "lib": os.environ.get("SCD_HIP_LIB", "default")}
    for rep in range(2):
        for name, enc in towers:
            enc.encode_image(x)
            torch.cuda.synchronize()
            enc.timing(True)
            t0 = time.perf_counter()
            for _ in range(launches):
                enc.encode_image(x)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms, n, flop = enc.timing(False)
            tower = tower_flop_per_image(enc.desc)
            out["%s_rep%d" % (name, rep)] = {"images_per_s": round(batch * launches / dt, 1), "fc1_us_per_launch": round(ms * 1e3 / max(n, 1), 1),
                                            "fc1_frac_of_2.5PF": round(flop / max(ms, 1e-9) / 1e9 / 2500.0, 4), "fc1_launches": n,
                                            "tokens": enc.desc["tokens"], "gflop_per_image": round(tower / 1e9, 2),
                                            "tower_frac_of_2.5PF": round(tower * batch * launches / dt / PEAK_FP16, 4)}
    if which == "dinov2":
        out["assemble_us"] = {"w%d_r%d" % (w, r): time_assembly(batch, w, r) for w in (768, 1024) for r in (0, 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
