#!/usr/bin/env python
"""Time of the metric sweep with and without the multi-scale SSIM on the same images, in one process:

  sweep         dlib.metrics.sweep(E, H, border, thresholds, levels=L): the two launches of today's sweep,
  sweep_msssim  dlib.metrics.sweep(..., msssim=--scales): the same plus srhip_metrics_msssim_lv (one launch per scale, which also
                writes the next scale's image pair, and one for the product),

at the white levels 255 and 65535, --thresholds ROI thresholds, a batch of --batch images of --size pixels a side: one evaluation
batch, the set-up of tools/deep_metrics_rate.py.

An arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP events around --iters sweeps; the median
is reported with the spread, and the difference of the two medians as what the option costs.  The images are a few MB and stay in
the Infinity Cache between iterations: cache-resident figures, host launch cost included, which is how fast_eval meets the sweep.

    python tools/msssim_rate.py --out profiles/msssim_rate.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))


def event_ms(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_rate.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--border", type=int, default=8)
    ap.add_argument("--thresholds", type=int, default=7)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/msssim_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from dlib import metrics
    B, S, M = ns.batch, ns.size, ns.scales
    g = torch.Generator().manual_seed(1)
    v = torch.randint(0, 256, (B, 1, S, S), generator=g).float()
    H = (v / 255).cuda()                                                   # a target on the 8-bit grid
    E = (H + 0.02 * torch.randn(B, 1, S, S, generator=g).cuda()).contiguous()
    ths = tuple(int(t) for t in torch.linspace(10, 200, ns.thresholds))
    keep = {}
    arms = {}
    for L in (255, 65535):
        arms[f"sweep_L{L}"] = lambda L=L: keep.__setitem__(f"s{L}", metrics.sweep(E, H, ns.border, ths, levels=L))
        arms[f"sweep_msssim_L{L}"] = lambda L=L: keep.__setitem__(f"m{L}", metrics.sweep(E, H, ns.border, ths, levels=L, msssim=M))
    out = {"tool": "tools/msssim_rate.py", "device": torch.cuda.get_device_name(0), "images": [B, 1, S, S], "border": ns.border,
           "thresholds": list(ths), "scales": M, "repeats": ns.repeats, "iters_per_timing": ns.iters,
           "timer": "HIP events around the sweep (every launch; host launch cost included), arms alternating in one process, "
                    "median of the repeats after a warm-up; cache-resident images"}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ns.repeats):
        for k, fn in arms.items():
            times[k].append(event_ms(fn, ns.iters))
    for k, t in times.items():
        out[f"{k}_us"] = round(statistics.median(t) * 1e3, 2)
        out[f"{k}_spread_us"] = [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)]
        print(k, out[f"{k}_us"], out[f"{k}_spread_us"], flush=True)
    for L in (255, 65535):
        out[f"msssim_cost_L{L}_us"] = round(out[f"sweep_msssim_L{L}_us"] - out[f"sweep_L{L}_us"], 2)
        # no atomics in the multi-scale SSIM: a second sweep gives the same bits; the other five tensors are today's
        again = metrics.sweep(E, H, ns.border, ths, levels=L, msssim=M)
        out[f"same_msssim_bits_twice_L{L}"] = bool(torch.equal(again["msssim"], keep[f"m{L}"]["msssim"]))
        out[f"msssim_mean_L{L}"] = float(again["msssim"].mean())
    print({k: v for k, v in out.items() if k.startswith(("msssim_", "same_"))}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
