#!/usr/bin/env python
"""Time of the full-depth metric sweep beside the 8-bit sweep on the same images, in one process:

  sweep_8bit    dlib.metrics.sweep(E, H, border, thresholds): srhip_metrics_psnr_family + srhip_metrics_ssim (float32 window
                moments, atomics),
  sweep_levels  dlib.metrics.sweep(..., levels=--levels): srhip_metrics_psnr_family_lv + srhip_metrics_ssim_lv (float64 window
                moments, one partial per block and a fixed-order sum),

both launches of each, --thresholds ROI thresholds, a batch of --batch images of --size pixels a side: one evaluation batch.

An arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP events around --iters sweeps; the median
is reported with the spread.  The images are a few MB and stay in the Infinity Cache between iterations: cache-resident figures,
host launch cost included, which is how fast_eval meets the sweep (right behind the forward that wrote E).

    python tools/deep_metrics_rate.py --out profiles/deep_metrics_rate.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_metrics_rate.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--border", type=int, default=8)
    ap.add_argument("--thresholds", type=int, default=7)
    ap.add_argument("--levels", type=int, default=65535)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/deep_metrics_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from dlib import metrics
    B, S, L = ns.batch, ns.size, ns.levels
    g = torch.Generator().manual_seed(1)
    v = torch.randint(0, 256, (B, 1, S, S), generator=g).float()
    H = (v / 255).cuda()                                                   # a target on the 8-bit grid
    E = (H + 0.02 * torch.randn(B, 1, S, S, generator=g).cuda()).contiguous()
    ths = tuple(int(t) for t in torch.linspace(10, 200, ns.thresholds))
    keep = {}
    arms = {"sweep_8bit": lambda: keep.__setitem__("s8", metrics.sweep(E, H, ns.border, ths)),
            "sweep_levels": lambda: keep.__setitem__("sl", metrics.sweep(E, H, ns.border, ths, levels=L))}
    out = {"tool": "tools/deep_metrics_rate.py", "device": torch.cuda.get_device_name(0), "images": [B, 1, S, S], "border": ns.border,
           "thresholds": list(ths), "levels": L, "repeats": ns.repeats, "iters_per_timing": ns.iters,
           "timer": "HIP events around the sweep (both launches; host launch cost included), arms alternating in one process, "
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
    # no atomics in the full-depth sweep: a second one gives the same bits
    again = metrics.sweep(E, H, ns.border, ths, levels=L)
    out["same_bits_twice"] = all(bool(torch.equal(again[k], keep["sl"][k])) for k in again)
    out["ssim_8bit_minus_levels_max"] = float((keep["s8"]["ssim"].double() - keep["sl"]["ssim"]).abs().max())
    print({k: out[k] for k in ("same_bits_twice", "ssim_8bit_minus_levels_max")}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
