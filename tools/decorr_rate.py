#!/usr/bin/env python
"""Time of the image decorrelation analysis (srhip_metrics_decorr_lv, predict.py --resolution True), in one process:

  decorr              srhip.ops.metrics_decorr_lv(X): the three launches (rows, columns + ring partials, 21 curves + peaks) on a
                      batch of --batch images of --size pixels a side; two images share a transform,
  decorr_curves       the same with the 21 curves and their peak rings written out,
  frc                 srhip.ops.metrics_frc_lv(X, Y) on the same batch against a second one: B transforms where decorr takes B / 2,
                      three ring sums a frequency where decorr takes four and a square root, one curve where decorr takes 21,
  predict             Predictor(--exp_path).run(pages) on --batch 8-bit pages whose output is --size pixels a side (upload,
                      ingest, the net, emit, download),
  predict_resolution  the same with resolution=True: two analyses more a group (the LR pages, the output) and one download.

The set-up is that of tools/frc_rate.py: an arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP
events around --iters calls (the predict arms end in a download, so the host waits for every call); the median is reported with
the spread.  Every timing is printed when it is made, and an arm whose warmed-up call takes more than --call-limit-ms is reported
and not looped.  The images are a few MB and stay in the Infinity Cache between iterations: cache-resident figures, host launch
cost included, which is how predict.py meets the calls.

    python tools/decorr_rate.py --out profiles/decorr_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decorr_rate.json"))
    ap.add_argument("--exp_path", default=os.path.join(ROOT, "tests", "golden", "eval_exp", "exp"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--call-limit-ms", type=float, default=500.0,
                    help="an arm whose warmed-up call takes longer than this on the host clock is reported and not looped")
    ns = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/decorr_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from srhip import ops
    from srhip.predict import Predictor
    B, size = ns.batch, ns.size
    S = ops.frc_side(size, size)
    g = torch.Generator().manual_seed(1)
    v = torch.randint(0, 256, (B, 1, size, size), generator=g).float()
    Y = (v / 255).cuda()                                                   # an image on the 8-bit grid
    X = (torch.nn.functional.avg_pool2d(Y, 3, 1, 1) + 0.02 * torch.randn(B, 1, size, size, generator=g).cuda()).contiguous()
    pred = Predictor(ns.exp_path, batch=B)
    if size % pred.scale:
        raise SystemExit(f"--size {size} is no multiple of the experiment's scale {pred.scale}")
    lr = size // pred.scale
    pages = np.random.RandomState(1).randint(0, 256, size=(B, lr, lr)).astype(np.uint8)
    keep = {}
    arms = {"decorr": lambda: keep.__setitem__("decorr", ops.metrics_decorr_lv(X)),
            "decorr_curves": lambda: keep.__setitem__("decorr_curves", ops.metrics_decorr_lv(X, curves=True)),
            "frc": lambda: keep.__setitem__("frc", ops.metrics_frc_lv(X, Y)),
            "predict": lambda: keep.__setitem__("predict", pred.run(pages)),
            "predict_resolution": lambda: keep.__setitem__("predict_resolution", pred.run(pages, resolution=True))}
    out = {"tool": "tools/decorr_rate.py", "device": torch.cuda.get_device_name(0), "images": [B, 1, size, size], "side": S,
           "pages": [B, lr, lr], "net": pred.args.netG["net_type"], "scale": pred.scale, "repeats": ns.repeats,
           "iters_per_timing": ns.iters, "call_limit_ms": ns.call_limit_ms,
           "timer": "HIP events around the calls (every launch; host launch cost included), arms alternating in one process, "
                    "median of the repeats after a warm-up; cache-resident images"}
    t_start = time.perf_counter()
    for k in list(arms):
        fn = arms[k]
        host = []
        for _ in range(3):                                                  # the first call may load code; the third is warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        out[f"{k}_first_calls_host_ms"] = [round(t, 3) for t in host]
        print(f"warm-up {k}: {out[f'{k}_first_calls_host_ms']} ms on the host clock", flush=True)
        if host[-1] > ns.call_limit_ms:
            out[f"{k}_not_timed"] = f"a warmed-up call took {host[-1]:.1f} ms, above --call-limit-ms {ns.call_limit_ms}"
            print(f"{k}: NOT timed: {out[f'{k}_not_timed']}", flush=True)
            del arms[k]
    times = {k: [] for k in arms}
    for rep in range(ns.repeats):
        for k, fn in arms.items():
            times[k].append(event_ms(fn, ns.iters))
            print(f"repeat {rep} {k}: {times[k][-1] * 1e3:.2f} us a call   ({time.perf_counter() - t_start:.1f} s in)", flush=True)
    for k, t in times.items():
        out[f"{k}_us"] = round(statistics.median(t) * 1e3, 2)
        out[f"{k}_spread_us"] = [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)]
        print(k, out[f"{k}_us"], out[f"{k}_spread_us"], flush=True)
    if "decorr" in times and "frc" in times:
        out["decorr_over_frc"] = round(out["decorr_us"] / out["frc_us"], 3)
    if "predict" in times and "predict_resolution" in times:
        out["resolution_cost_in_predict_us"] = round(out["predict_resolution_us"] - out["predict_us"], 2)
        out["predict_resolution_over_predict"] = round(out["predict_resolution_us"] / out["predict_us"], 3)
    res = keep["decorr"]
    out["same_bits_twice"] = bool(torch.equal(ops.metrics_decorr_lv(X), res))
    out["same_bits_with_curves"] = bool(torch.equal(keep["decorr_curves"][0], res))
    out["same_pages_with_resolution"] = bool(np.array_equal(keep["predict"], keep["predict_resolution"]))
    out["cut_mean"] = float(res[:, 0].mean())
    pred.run(pages, resolution=True)
    out["first_page"] = pred.last_resolution[0]
    print({k: v for k, v in out.items() if k.startswith(("decorr_over", "resolution_cost", "predict_resolution_over", "same_", "cut_"))},
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
