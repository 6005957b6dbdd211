"""HIP-event timing of the fused reconstruction scoring (ldc_recon_scores) and preprocessing (ldc_recon_preprocess) calls against the
reference's torch-op composition on the same device, at the real size (2, 89, 120, 240).  Call times: 200 back-to-back calls between two
events, so each figure holds the binding's host work and both launches, not a kernel alone.

    python tools/recon_bench.py [out.json]
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ladcast_amd.metric.utils import recon_scores
from ladcast_amd.evaluate.evaluate_encdec_model import preprocess_batch

B, C, S, H, W = 2, 84, 5, 120, 240
Cp = C + S
g = torch.Generator().manual_seed(0)
target = torch.randn(B, C, H, W, generator=g).cuda()
static = torch.randn(1, S, H, W, generator=g).cuda()
pred = (torch.cat([target, static.expand(B, -1, -1, -1)], 1) + 0.1 * torch.randn(B, Cp, H, W, generator=g).cuda()).contiguous()
mask = (torch.rand(B, H, W, generator=g) < 0.3).cuda()
w = torch.rand(H, generator=g).cuda() + 0.5
mean, std = torch.randn(Cp, generator=g).cuda(), torch.rand(Cp, generator=g).cuda() + 0.5
raw = torch.randn(B, C + 1, H + 1, W, generator=g).cuda()
raw[:, 82][:, torch.rand(H + 1, W, generator=g).cuda() < 0.3] = float("nan")

def fused():
    return recon_scores(pred, target, static, mask, 82, w, mean, std)

def composed():
    ch = torch.arange(Cp, device="cuda").view(1, -1, 1, 1) == 82
    p = torch.where(mask.unsqueeze(1) & ch, -2.0, pred)
    chT = torch.arange(C, device="cuda").view(1, -1, 1, 1) == 82
    t = torch.where(mask.unsqueeze(1) & chT, -2.0, target)
    t = torch.cat([t, static.expand(B, -1, -1, -1)], dim=1)
    w4 = w.view(1, 1, -1, 1)
    diff = torch.norm((w4 * (p - t)).flatten(start_dim=-2), p=2, dim=-1) / torch.norm((w4 * t).flatten(start_dim=-2), p=2, dim=-1)
    sd, mu = std.view(-1, 1, 1), mean.view(-1, 1, 1)
    mse = torch.nn.functional.mse_loss(p * sd + mu, t * sd + mu, reduction="none")
    return diff, None, (mse * w4).mean(dim=[0, 2, 3])

def fused_pre():
    return preprocess_batch(raw, mean[:C], std[:C], True, 82, False)

def composed_pre():
    b = raw[..., 1:, :][:, :-1]
    b = (b - mean[:C].view(-1, 1, 1)) / std[:C].view(-1, 1, 1)
    m = torch.isnan(b[:, 82])
    b[:, 82][m] = -2
    return b, m

def time(fn, n=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / n * 1e3)
    return best

a, c = fused(), composed()
print("max rel dev fused vs composed: rel", float(((a[0] - c[0]).abs() / c[0].abs()).max()), "lw", float(((a[2] - c[2]).abs() / c[2].abs()).max()))
res = {}
for rnd in range(2):  # alternate
    for name, fn in (("scores_fused", fused), ("scores_torch", composed), ("pre_fused", fused_pre), ("pre_torch", composed_pre)):
        res.setdefault(name, []).extend(time(fn))
bytes_scores = 4 * (B * Cp * H * W + B * C * H * W + S * H * W) + B * H * W
bytes_pre = 4 * 2 * B * C * H * W + B * H * W
out = {k: {"us_median": sorted(v)[len(v) // 2], "us_min": min(v), "us_max": max(v)} for k, v in res.items()}
out["scores_fused"]["GBps_at_median"] = bytes_scores / out["scores_fused"]["us_median"] / 1e3
out["pre_fused"]["GBps_at_median"] = bytes_pre / out["pre_fused"]["us_median"] / 1e3
out["bytes_scores"], out["bytes_pre"] = bytes_scores, bytes_pre
print(json.dumps(out, indent=1))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
