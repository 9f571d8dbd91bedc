"""Print 1 - cos and max|err| / max|ref| of every tower-vs-oracle assertion (the inputs of tests/tower_tolerances.py, which the tests
use), next to the tolerance it is held to.  Needs the GPU.  `python tests/tower_cos.py [--json out.json]`"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # repo root (this script lives in tests/: it uses the oracle)
sys.path.insert(0, HERE)
import tower_tolerances as tt
from oracle import clip_oracle as co
from oracle import naming_oracle as no
from scd_amd.clip.model import CLIP, DinoViT

res = {}


def rec(name, out, ref):
    res[name] = tt.metrics(out, ref)
    print("%-24s 1-cos %.3e  max|err|/max|ref| %.3e   (tolerance %.1e / %.1e)" % ((name,) + res[name] + tt.TOL[name]), flush=True)


norm = lambda t: torch.nn.functional.normalize(t.float(), dim=-1)
for layers in (2, 12):
    sd, sd16, img, tok = tt.clip_case(layers)
    model = CLIP(sd).cuda().eval()
    rec("clip%d_image" % layers, model.encode_image(img.cuda()).float().cpu(), co.clip_encode_image(sd16, img.half().float()))
    rec("clip%d_text" % layers, model.encode_text(tok.cuda()).float().cpu(), co.clip_encode_text(sd16, tok.long()))
sd, sd16, img = tt.dino_case()
rec("dino12", DinoViT(sd).cuda()(img.cuda()).float().cpu(), co.dino_forward(sd16, img.half().float()))
for tower in ("clip_image", "clip_text", "dino"):
    sd, sd16, x = tt.outlier_case(tower)
    if tower == "dino":
        out, ref = DinoViT(sd).cuda()(x.cuda()).float().cpu(), co.dino_forward(sd16, x)
    elif tower == "clip_image":
        out, ref = CLIP(sd).cuda().eval().encode_image(x.cuda()).float().cpu(), co.clip_encode_image(sd16, x)
    else:
        out, ref = CLIP(sd).cuda().eval().encode_text(x.cuda()).float().cpu(), co.clip_encode_text(sd16, x.long())
    rec("outlier_" + tower, out, ref)
import scd_amd.clip as clip
from scd_amd.local_utils import clip_lang_util as clu
clip.allow_synthetic()
sd, sd16, names, tmpl = tt.zeroshot_case()
zs = clu.zeroshot_classifier(names, tmpl, CLIP(sd).cuda(), names_per_batch=2)
ref = no.zeroshot_classifier(names, tmpl, lambda t: co.clip_encode_text(sd16, t.long()).numpy(), clip.tokenize)
rec("zeroshot_text", zs.float().cpu().t(), torch.from_numpy(ref).t())
import outlier_weights as ow
y, img, tok = tt.outlier_features_case()
sdd, _ = ow.dino_outlier_state_dict(seed=1, layers=12)
sdd16 = ow.round_like_the_device(sdd)
rec("outlier_feat_dino", norm(DinoViT(sdd).cuda()(img.cuda())).cpu(),
    norm(torch.cat([co.dino_forward(sdd16, img[i:i + 12]) for i in range(0, len(img), 12)])))
sd, _, _ = ow.clip_outlier_state_dict(seed=0, layers=12)
sd16 = ow.round_like_the_device(sd)
model = CLIP(sd).cuda().eval()
rec("outlier_feat_clip_image", norm(model.encode_image(img.cuda())).cpu(),
    norm(torch.cat([co.clip_encode_image(sd16, img[i:i + 12]) for i in range(0, len(img), 12)])))
rec("outlier_feat_text", norm(model.encode_text(tok.cuda())).cpu(), norm(co.clip_encode_text(sd16, tok.long())))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(res, f, indent=1)
