#!/usr/bin/env python
"""Time of the Fourier ring correlation (srhip_metrics_frc_lv, --frc) on one evaluation batch, in one process:

  frc        srhip.ops.metrics_frc_lv(E, H): the three launches (rows, columns + ring partials, curve + cutoff),
  torch      the same statement composed from torch.fft.fft2 in float64 plus index ops: quantise, crop, window, two transforms,
             three ring sums by a prepared gather (ring r's points padded to the longest ring, then one sum), the curve (the
             cutoff search is left out of this arm),
  sweep      dlib.metrics.sweep(E, H, border, thresholds): what fast_eval calls per batch today,
  sweep_frc  the same followed by dlib.metrics.frc(E, H): what fast_eval calls per batch under --frc True,

on a batch of --batch images of --size pixels a side, the set-up of tools/msssim_rate.py.

The torch arm's ring sums are a gather and a sum, NOT index_add_ / bincount / scatter_add_.  On gfx950 torch adds float64 by a
compare-and-swap loop at system scope (global_atomic_cmpswap_x2 ... sc0 sc1 and a branch back, in indexFuncLargeIndex<double>:
there is no hardware float64 add in it), and a batch of 8 x 512^2 sends 2 M such adds onto 2056 doubles (129 cache lines, about
1000 adds a double, every resident thread of the device contending for them), 3 times a call.  A first form of this script used
index_add_ and did not finish its 250 such calls within 300 s; it printed nothing before the end, so where the time went was
not recorded.  The arm also pays, once, for rocFFT building its float64 kernels at first use.

So that no arm can run away silently: every timing is printed when it is made; an arm's first call is timed by the host, and an
arm whose call takes more than --call-limit-ms (default 100) is reported and NOT looped.  With the defaults that bounds the whole
run by 4 arms x (3 + 5 x 50) calls x 0.1 s = 101 s plus the one-off FFT build; run it under a limit of 300 s.

An arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP events around --iters calls; the median is
reported with the spread.  The images are a few MB and stay in the Infinity Cache between iterations: cache-resident figures,
host launch cost included, which is how fast_eval meets the calls.

    python tools/frc_rate.py --out profiles/frc_rate.json
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


def ring_gather(S, dev):
    """(S/2 + 1, longest ring) int64: for every kept ring the flat indices of its frequencies in FFT order, padded with S * S (the
    index of a zero appended behind the flattened image); built once, on the host"""
    import numpy as np
    import torch
    k = np.arange(S, dtype=np.int64)
    k = np.where(k < S // 2, k, k - S)
    q = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    r = (np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64) + 1) // 2
    r = np.where((2 * r - 1) ** 2 > q, r - 1, r)
    r = np.where((2 * r + 1) ** 2 <= q, r + 1, r)
    r = np.where(q == 0, 0, r).ravel()                                             # k = 0 is ring 0 (the rule alone gives -1)
    nr = S // 2 + 1
    assert r.min() == 0
    order = np.argsort(r, kind="stable")
    order = order[r[order] < nr]
    counts = np.bincount(r[order], minlength=nr)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    idx = np.full((nr, counts.max()), S * S, dtype=np.int64)
    col = np.arange(len(order)) - np.repeat(starts, counts)
    idx[r[order], col] = order
    assert idx.min() >= 0 and idx.max() == S * S
    return torch.from_numpy(idx).to(dev)


def torch_statement(S, N, dev):
    """the definition of include/srhip.h in torch float64 on ``dev``; returns fn(E, H) -> curve (B, S/2 + 1)"""
    import torch
    idx = ring_gather(S, dev)
    win = 0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(S, device=dev, dtype=torch.float64) / S)
    win2 = win[:, None] * win[None, :]

    def sums(v):
        flat = torch.nn.functional.pad(v.reshape(v.shape[0], -1), (0, 1))           # the zero the padding points at
        return flat[:, idx].sum(-1)

    def fn(E, H):
        h, w = E.shape[-2:]
        oy, ox = (h - S) // 2, (w - S) // 2
        a, b = ((t[:, 0, oy:oy + S, ox:ox + S].clamp(0, 1) * float(N)).round().double() / N * win2 for t in (E, H))
        F1, F2 = torch.fft.fft2(a), torch.fft.fft2(b)
        c, p1, p2 = sums((F1 * F2.conj()).real), sums(F1.real ** 2 + F1.imag ** 2), sums(F2.real ** 2 + F2.imag ** 2)
        den = p1 * p2
        return torch.where(den > 0, c / den.clamp(min=1e-300).sqrt(), torch.zeros_like(c))
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frc_rate.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--border", type=int, default=8)
    ap.add_argument("--thresholds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--call-limit-ms", type=float, default=100.0,
                    help="an arm whose warmed-up call takes longer than this on the host clock is reported and not looped")
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/frc_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from dlib import metrics
    from srhip import ops
    B, size = ns.batch, ns.size
    S = ops.frc_side(size, size)
    g = torch.Generator().manual_seed(1)
    v = torch.randint(0, 256, (B, 1, size, size), generator=g).float()
    H = (v / 255).cuda()                                                   # a target on the 8-bit grid
    E = (torch.nn.functional.avg_pool2d(H, 3, 1, 1) + 0.02 * torch.randn(B, 1, size, size, generator=g).cuda()).contiguous()
    ths = tuple(int(t) for t in torch.linspace(10, 200, ns.thresholds))
    stmt = torch_statement(S, 255, E.device)
    keep = {}
    arms = {"frc": lambda: keep.__setitem__("frc", ops.metrics_frc_lv(E, H)),
            "torch": lambda: keep.__setitem__("torch", stmt(E, H)),
            "sweep": lambda: keep.__setitem__("sweep", metrics.sweep(E, H, ns.border, ths)),
            "sweep_frc": lambda: keep.__setitem__("sweep_frc", (metrics.sweep(E, H, ns.border, ths), metrics.frc(E, H)))}
    out = {"tool": "tools/frc_rate.py", "device": torch.cuda.get_device_name(0), "images": [B, 1, size, size], "side": S,
           "border": ns.border, "thresholds": list(ths), "repeats": ns.repeats, "iters_per_timing": ns.iters,
           "call_limit_ms": ns.call_limit_ms,
           "timer": "HIP events around the calls (every launch; host launch cost included), arms alternating in one process, "
                    "median of the repeats after a warm-up; cache-resident images"}
    t_start = time.perf_counter()
    for k in list(arms):
        fn = arms[k]
        host = []
        for _ in range(3):                                                  # the first call may build kernels; the third is warm
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
    if "sweep_frc" in times and "sweep" in times:
        out["frc_cost_in_fast_eval_us"] = round(out["sweep_frc_us"] - out["sweep_us"], 2)
    if "torch" in times and "frc" in times:
        out["torch_over_frc"] = round(out["torch_us"] / out["frc_us"], 2)
    curve, cut = keep["frc"]
    again = ops.metrics_frc_lv(E, H)
    out["same_bits_twice"] = bool(torch.equal(again[0], curve) and torch.equal(again[1], cut))
    out["curve_max_diff_from_torch"] = float((curve - keep["torch"]).abs().max())
    out["cut_mean"] = float(cut.mean())
    print({k: v for k, v in out.items() if k.startswith(("frc_cost", "torch_over", "same_", "curve_", "cut_"))}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
