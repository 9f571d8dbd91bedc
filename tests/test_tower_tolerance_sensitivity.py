"""The tower tolerances (tests/tower_tolerances.py) are tight enough to see what goes wrong in attention and LayerNorm kernels.

Bugs are injected into the fp32 oracle (oracle/clip_oracle.py) on the exact weights and inputs of the tower tests; each moves the
12-block features away from the clean oracle by at least 3 x the tolerance in 1 - cos, which is what the HIP towers are held to
against that same clean oracle (their real error is ~10 x below the tolerance):
  * image towers (CLIP and DINO): the K / V padding to 224 keys leaking into the softmax (27 copies of the last key, as the
    persistent kernels pad, or 27 zero rows, as attention_kernel<7> pads), one head's output zeroed, LayerNorm eps x 100;
  * text tower: a causal mask that lets query i see key i + 1, one head's output zeroed.
The smallest of these deviations (CLIP image, zero-row padding leak: 1 - cos = 1.0e-4) is 15 x its tolerance; the test fails if a
1 - cos tolerance is raised above a third of the deviation it has to show.  The max|err| / max|ref| bound is a second guard only:
these bugs move it by 1.4 x (that same zero-row leak) to 46 x its bound.
What the tower bounds cannot see, because random synthetic weights make attention nearly uniform and dilute such bugs before
they reach the features: a softmax scale off by 1 % and the last key dropped on the image towers (an off-by-one loop bound).
tests/test_gpu_attention.py catches those at the kernel, with planted sharp attention.
"""
import pytest
import torch

import tower_tolerances as tt
from oracle import clip_oracle as co

MARGIN = 3.0


def _buggy_attention(kind):
    def att(x, qkv_w, qkv_b, out_w, out_b, heads, causal):
        b, t, c = x.shape
        qkv = x @ qkv_w.float().t() + qkv_b.float()
        q, k, v = qkv.view(b, t, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
        if kind == "pad_leak":                       # keys / values padded to 224 rows with copies of the last one, not masked
            n = 224 - t
            k = torch.cat([k, k[..., -1:, :].expand(-1, -1, n, -1)], 2)
            v = torch.cat([v, v[..., -1:, :].expand(-1, -1, n, -1)], 2)
        if kind == "pad_leak_zero":                  # ... with zero rows (attention_kernel<7>'s padding), not masked
            n = 224 - t
            k = torch.cat([k, torch.zeros_like(k[..., :1, :]).expand(-1, -1, n, -1)], 2)
            v = torch.cat([v, torch.zeros_like(v[..., :1, :]).expand(-1, -1, n, -1)], 2)
        s = (q @ k.transpose(-2, -1)) * (c // heads) ** -0.5
        if causal:
            s = s + torch.full((t, t), float("-inf")).triu_(2 if kind == "causal_next" else 1)
        o = s.softmax(dim=-1) @ v
        if kind == "head_zero":
            o[:, 0] = 0
        return o.transpose(1, 2).reshape(b, t, c) @ out_w.float().t() + out_b.float()
    return att


def _inject(monkeypatch, kind):
    if kind == "ln_eps":
        ln = co._ln
        monkeypatch.setattr(co, "_ln", lambda x, w, b, eps: ln(x, w, b, eps * 100))
    else:
        monkeypatch.setattr(co, "_attention", _buggy_attention(kind))


_CASES = {}


def _case(tower):
    """(tolerance name, oracle forward) on the tower test's data"""
    if tower not in _CASES:
        if tower == "dino":
            _, sd16, img = tt.dino_case()
            _CASES[tower] = ("dino12", lambda: co.dino_forward(sd16, img.half().float()))
        else:
            _, sd16, img, tok = tt.clip_case(12)
            if tower == "clip_image":
                _CASES[tower] = ("clip12_image", lambda: co.clip_encode_image(sd16, img.half().float()))
            else:
                _CASES[tower] = ("clip12_text", lambda: co.clip_encode_text(sd16, tok.long()))
    return _CASES[tower]


_CLEAN = {}


@pytest.mark.parametrize("tower,kind", [("clip_image", "pad_leak"), ("clip_image", "pad_leak_zero"), ("clip_image", "head_zero"),
                                        ("clip_image", "ln_eps"), ("dino", "pad_leak"), ("dino", "pad_leak_zero"), ("dino", "head_zero"),
                                        ("dino", "ln_eps"),
                                        ("clip_text", "causal_next"), ("clip_text", "head_zero")])
def test_tower_tolerance_sees_injected_bug(monkeypatch, tower, kind):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    name, fwd = _case(tower)
    if tower not in _CLEAN:
        _CLEAN[tower] = fwd()
    _inject(monkeypatch, kind)
    gap, _ = tt.metrics(fwd(), _CLEAN[tower])
    assert gap >= MARGIN * tt.TOL[name][0], "%s / %s: 1 - cos %.3e < %g x the tolerance %.1e" % (tower, kind, gap, MARGIN, tt.TOL[name][0])
