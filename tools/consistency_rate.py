#!/usr/bin/env python
"""Time of the resolution-scaled error (srhip_consistency, predict.py --consistency True), in one process, at two shapes -- 8 pages
of 64 x 64 at x8 (the predict shape) and 8 pages of 256 x 256 at x2:

  consistency            srhip.ops.consistency(E, L, s): two banks of 16 candidate blurs and two decisions, four launches; no
                         candidate image is written to memory,
  consistency_maps       the same with the 32 scores and the residual map written out (a fifth launch),
  composition            what the call replaces: 32 srhip.ops.psf_bin calls (each writes its float32 row pass and its degraded
                         image) and, per candidate, the five sums and the score as torch float64 reductions, then the argmax.
                         It is given the fine bank's q list beforehand (the same 16 candidates for every page), which the real
                         search only knows after a download of the coarse decision: the arm is charged less than it would cost.
                         Its model images are rounded to float32 twice, so its figures are not the statement's,
  predict                Predictor(--exp_path).run(pages) on 8 8-bit pages of 64 x 64 (upload, ingest, the net, emit, download),
  predict_consistency    the same with consistency=True: one call more a group and one small download.

The set-up is that of tools/decorr_rate.py: an arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP
events around --iters calls; the median is reported with the spread.  Every timing is printed when it is made, and an arm whose
warmed-up call takes more than --call-limit-ms is reported and not looped.  The images stay in the Infinity Cache between
iterations: cache-resident figures, host launch cost included, which is how predict.py meets the call.  Not a gate.

    python tools/consistency_rate.py --out profiles/consistency_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))

SHAPES = (("8x64x64_s8", 8, 64, 64, 8), ("8x256x256_s2", 8, 256, 256, 2))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_rate.json"))
    ap.add_argument("--exp_path", default=os.path.join(ROOT, "tests", "golden", "eval_exp", "exp"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--call-limit-ms", type=float, default=500.0,
                    help="an arm whose warmed-up call takes longer than this on the host clock is reported and not looped")
    ns = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/consistency_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from srhip import ops
    from srhip.predict import Predictor
    keep, arms, data = {}, {}, {}
    g = torch.Generator().manual_seed(1)
    for tag, B, h, w, s in SHAPES:
        E = torch.nn.functional.avg_pool2d(torch.rand(B, 1, s * h + 2, s * w + 2, generator=g), 3, 1).cuda().contiguous()
        q0 = 72 if s == 8 else 40
        wts = {q: ops.psf_bin_weights(q * s / 64.0, s) for q in set(range(0, 128, 8)) | set(range(q0 - 8, q0 + 8))}
        L = (0.8 * ops.psf_bin(E[:, 0], wts[q0], s) + 0.05 + 0.02 * torch.randn(B, h, w, generator=g).cuda())[:, None].contiguous()
        data[tag] = (E, L, s)

        def composition(E=E, L=L, s=s, wts=wts, q0=q0, n=float(h * w)):
            l = L[:, 0].double()
            sl, sll = l.sum((1, 2)), (l * l).sum((1, 2))
            cll = sll - sl * sl / n
            best = None
            for bank in (range(0, 128, 8), range(q0 - 8, q0 + 8)):
                scores = []
                for q in bank:
                    b = ops.psf_bin(E[:, 0], wts[q], s).double()
                    sb, sbb, sbl = b.sum((1, 2)), (b * b).sum((1, 2)), (b * l).sum((1, 2))
                    cbb, cbl = sbb - sb * sb / n, sbl - sb * sl / n
                    scores.append(cbl * cbl.abs() / (cbb * cll))
                best = torch.stack(scores, 1).argmax(1)
            return best
        arms[f"consistency_{tag}"] = lambda E=E, L=L, s=s, tag=tag: keep.__setitem__(f"consistency_{tag}", ops.consistency(E, L, s))
        arms[f"consistency_maps_{tag}"] = lambda E=E, L=L, s=s, tag=tag: keep.__setitem__(
            f"consistency_maps_{tag}", ops.consistency(E, L, s, scores=True, residual=True))
        arms[f"composition_{tag}"] = lambda fn=composition, tag=tag: keep.__setitem__(f"composition_{tag}", fn())
    pred = Predictor(ns.exp_path, batch=8)
    pages = np.random.RandomState(1).randint(0, 256, size=(8, 64, 64)).astype(np.uint8)
    arms["predict"] = lambda: keep.__setitem__("predict", pred.run(pages))
    arms["predict_consistency"] = lambda: keep.__setitem__("predict_consistency", pred.run(pages, consistency=True))
    out = {"tool": "tools/consistency_rate.py", "device": torch.cuda.get_device_name(0),
           "shapes": {tag: {"pages": [B, h, w], "scale": s} for tag, B, h, w, s in SHAPES},
           "predict_pages": [8, 64, 64], "net": pred.args.netG["net_type"], "scale": pred.scale, "repeats": ns.repeats,
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
    for tag, *_ in SHAPES:
        if f"consistency_{tag}" in times and f"composition_{tag}" in times:
            out[f"composition_over_consistency_{tag}"] = round(out[f"composition_{tag}_us"] / out[f"consistency_{tag}_us"], 3)
        E, L, s = data[tag]
        res = keep[f"consistency_{tag}"]
        out[f"same_bits_twice_{tag}"] = bool(torch.equal(ops.consistency(E, L, s), res))
        out[f"same_bits_with_maps_{tag}"] = bool(torch.equal(keep[f"consistency_maps_{tag}"][0], res))
        out[f"q_{tag}"] = [int(v) for v in res[:, 5].tolist()]
        out[f"rsp_mean_{tag}"] = float(res[:, 3].mean())
    if "predict" in times and "predict_consistency" in times:
        out["consistency_cost_in_predict_us"] = round(out["predict_consistency_us"] - out["predict_us"], 2)
        out["predict_consistency_over_predict"] = round(out["predict_consistency_us"] / out["predict_us"], 3)
    out["same_pages_with_consistency"] = bool(np.array_equal(keep["predict"], keep["predict_consistency"]))
    pred.run(pages, consistency=True)
    out["first_page"] = pred.last_consistency[0]
    print({k: v for k, v in out.items() if k.startswith(("composition_over", "consistency_cost", "predict_consistency_over", "same_",
                                                          "q_", "rsp_"))}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
