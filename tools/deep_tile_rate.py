#!/usr/bin/env python
"""Time of the three launches behind 16-bit tiles, each beside the launch(es) it stands next to, in one process:

  gather    srhip_patch_gather_u16 against srhip_patch_gather: a training batch of --batch patches of --patch pixels a side
            out of resident --tile x --tile tiles (the 16-bit arm reads twice the bytes and writes the same floats),
  resize    srhip_imresize_aa_u16 against srhip_imresize_aa on a uint8 tile, one tile at 1 / --scale (once per tile, when a
            set is built),
  levels    srhip_levels_u16_to_u8 against the composition it replaces -- srhip_ingest_pad (uint16 -> float32),
            srhip_tensor2uint82float and a cast to uint8 -- on one LR tile (once per tile, when a set is built).

An arm is warmed up, then timed --repeats times, the arms alternating, each timing HIP events around --iters runs; the median
is reported with the spread.  The buffers are a few MB and stay in the Infinity Cache between iterations: these are
cache-resident figures, which is also how the training step meets the gather.

    python tools/deep_tile_rate.py --out profiles/deep_tile_rate.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_tile_rate.json"))
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--patch", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ns = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/deep_tile_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from srhip import ops
    T, P, B, s = ns.tile, ns.patch, ns.batch, ns.scale
    rng = np.random.RandomState(1)
    t8 = [rng.randint(0, 256, size=(T, T)).astype(np.uint8) for _ in range(B)]
    d8 = [torch.from_numpy(t).cuda() for t in t8]
    d16 = [torch.from_numpy((257 * t.astype(np.int64)).astype(np.uint16)).cuda() for t in t8]
    ids, modes = list(range(B)), [b % 8 for b in range(B)]
    y0 = [int(v) for v in rng.randint(0, T - P + 1, size=B)]
    x0 = [int(v) for v in rng.randint(0, T - P + 1, size=B)]
    out8, out16 = torch.empty(B, 1, P, P, device="cuda"), torch.empty(B, 1, P, P, device="cuda")
    lo8, lo16 = torch.empty(1, T // s, T // s, device="cuda"), torch.empty(1, T // s, T // s, device="cuda")
    one8, one16 = d8[0][None].contiguous(), d16[0][None].contiguous()
    lv = torch.empty(T, T, dtype=torch.uint8, device="cuda")
    keep = {}

    def levels_composition():
        keep["lv"] = ops.tensor2uint82float(ops.ingest_pad(one16, 65535, T, T)).to(torch.uint8)

    groups = {
        "gather": {"patch_gather_u8": lambda: ops.patch_gather(d8, ids, y0, x0, modes, P, out=out8),
                   "patch_gather_u16": lambda: ops.patch_gather_u16(d16, ids, y0, x0, modes, P, out=out16)},
        "resize": {"imresize_aa_u8": lambda: ops.imresize_aa(one8, 1 / s, out=lo8),
                   "imresize_aa_u16": lambda: ops.imresize_aa(one16, 1 / s, out=lo16)},
        "levels": {"ingest_u8ify_cast": levels_composition,
                   "levels_u16_to_u8": lambda: ops.levels_u16_to_u8(d16[0], out=lv)},
    }
    out = {"tool": "tools/deep_tile_rate.py", "device": torch.cuda.get_device_name(0), "tile": [T, T], "patch": P, "batch": B,
           "scale": s, "repeats": ns.repeats, "iters_per_timing": ns.iters, "timer": "HIP events around the arm (host launch "
           "cost included), arms alternating in one process, median of the repeats after a warm-up; cache-resident buffers"}
    for name, arms in groups.items():
        for fn in arms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(ns.repeats):
            for k, fn in arms.items():
                times[k].append(event_ms(fn, ns.iters))
        rec = {}
        for k, v in times.items():
            rec[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
            rec[f"{k}_spread_us"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
        out[name] = rec
        print(name, rec, flush=True)
    # the 257 v tiles give the bits of the 8-bit arm: the two arms of a group did the same work
    out["same_bits"] = {"gather": bool(torch.equal(out8, out16)), "resize": bool(torch.equal(lo8, lo16)),
                        "levels": bool(torch.equal(keep["lv"].view(T, T), lv) and torch.equal(lv, d8[0]))}
    print(out["same_bits"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
