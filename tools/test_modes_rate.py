#!/usr/bin/env python
"""Time per image of the test modes (dlib/utils/utils_model.py: x8 self-ensemble, split, split and x8) on the README's SwinIR,
x8, one 256 x 256 low-resolution image -- arm A, this package (one gather launch per tile shape, forwards in batches of 8,
one merge launch), against arm B, the same plan run the reference's way in the same process: one forward per view or tile,
torch slicing, rot90 / flip, stack().mean() (tests/test_modes_ref.ref_test_mode).  Both arms call the same net.

Modes: 3 (eight 256 x 256 views), 2 with refield 32 and min_size 128 (four 160 x 160 tiles), 4 with the same (32 tiles).  Each
arm is warmed up on every shape it uses, then timed --repeats times, alternating, each timing a host clock around one call
that ends in a device synchronise; the median is reported with the spread, and the distance between the arms' outputs.

The two kernels alone (mode 4's launches: 16 tiles per shape, eight views merged into 2048 x 2048): device events around
--kernel_iters launches through the C-ABI with the tables uploaded once, the bytes the algorithm reads and writes over that
time, beside a device-to-device copy (Tensor.copy_) moving the same number of bytes.

    python tools/test_modes_rate.py --out profiles/test_modes_rate.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def event_ms(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_rates(L, sf, refield, min_size, iters):
    """mode 4's gather launches and its merge, through the C-ABI, against a copy of the same bytes"""
    import torch
    from dlib.utils import utils_model as um
    from srhip import ops
    from srhip._lib import call
    B, C, H, W = L.shape
    N, st = B * C, torch.cuda.current_stream().cuda_stream
    res, views = {}, []
    src = L.view(N, H, W)

    def copy_gbs(nbytes):
        n = nbytes // 8                                         # a copy of n floats reads 4 n bytes and writes 4 n
        a, b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        return 8 * n / (event_ms(lambda: b.copy_(a), iters) * 1e-3) / 1e9

    for turning in (0, 1):
        fh, fw = (W, H) if turning else (H, W)
        levels, (th, tw) = um.split_levels(fh, fw, refield, min_size, 1)
        jobs = [um._view_rect(m, leaf["src"], H, W) + (m,) for m in range(8) if m & 1 == turning
                for leaf in um.split_plan(fh, fw, refield, min_size, 1)]
        host = (ops._ViewJob * len(jobs))(*[ops._ViewJob(*j) for j in jobs])
        dev = ops._to_device_table(host, L.device)
        out = torch.empty(len(jobs), N, th, tw, device="cuda")
        ms = event_ms(lambda: call("srhip_view_gather", src.data_ptr(), N, H, W, dev.data_ptr(), ctypes.addressof(host), len(jobs),
                                   out.data_ptr(), th, tw, st), iters)
        nbytes = 2 * out.numel() * 4
        res["gather_turning" if turning else "gather_straight"] = {
            "jobs": len(jobs), "tile": [th, tw], "us": round(ms * 1e3, 2), "bytes": nbytes,
            "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "copy_same_bytes_GBps": round(copy_gbs(nbytes), 1)}
        tiles = torch.rand(len(jobs), N, th * sf, tw * sf, device="cuda")
        n_leaves = 4 ** (len(levels) - 1)
        for i, m in enumerate(m for m in range(8) if m & 1 == turning):
            views.append((m, (tiles[i * n_leaves:(i + 1) * n_leaves], m, th, tw, levels)))
    views = [v for _, v in sorted(views, key=lambda t: t[0])]
    dst = torch.empty(N, H * sf, W * sf, device="cuda")
    host = (ops._ViewDesc * 8)()
    for d, (tl, m, th, tw, levels) in zip(host, views):
        d.tiles, d.mode, d.depth, d.th, d.tw = tl.data_ptr(), m, len(levels) - 1, th, tw
        for l, (h, w) in enumerate(levels):
            d.h[l], d.w[l] = h, w
    dev = ops._to_device_table(host, L.device)
    ms = event_ms(lambda: call("srhip_view_merge", dev.data_ptr(), ctypes.addressof(host), 8, dst.data_ptr(), N, H, W, sf, st), iters)
    nbytes = 9 * dst.numel() * 4                                 # eight owned pixels read, one written, per destination pixel
    res["merge"] = {"views": 8, "dst": [H * sf, W * sf], "us": round(ms * 1e3, 2), "bytes": nbytes,
                    "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "copy_same_bytes_GBps": round(copy_gbs(nbytes), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "test_modes_rate.json"))
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel_iters", type=int, default=50)
    ap.add_argument("--refield", type=int, default=32)
    ap.add_argument("--min_size", type=int, default=128)
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/test_modes_rate.py measures on the GPU; there is none here")
    import test_modes_ref as R
    from dlib.models.network_swinir import SwinIR
    from dlib.utils import utils_model as um
    sf = 8
    torch.manual_seed(0)
    net = SwinIR(upscale=sf, in_chans=1, img_size=64, window_size=8, depths=[6, 6, 6, 6], embed_dim=180,
                 num_heads=[6, 6, 6, 6], mlp_ratio=2, upsampler="pixelshuffledirect").cuda().eval()
    L = torch.rand(1, 1, ns.size, ns.size, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(refield=ns.refield, min_size=ns.min_size, sf=sf, modulo=1)

    def single(x):                                               # arm B hands the net views made by rot90 / flip
        return net(x.contiguous()).clone()

    out = {"tool": "tools/test_modes_rate.py", "device": torch.cuda.get_device_name(0),
           "net": "SwinIR README configuration (window 8, depths 6x4, embed 180, heads 6x4, mlp_ratio 2, pixelshuffledirect)",
           "scale": sf, "lr": [ns.size, ns.size], "refield": ns.refield, "min_size": ns.min_size, "max_batch": 8,
           "repeats": ns.repeats, "modes": {}}
    with torch.no_grad():
        for mode in (3, 2, 4):
            arms = {"batched": lambda: um.test_mode(net, L, mode, **kw),
                    "sequential": lambda: R.ref_test_mode(single, L, mode, **kw)}
            ya, yb = arms["batched"](), arms["sequential"]()     # warm-up of every shape of both arms
            d = (ya - yb).abs()
            times = {k: [] for k in arms}
            for _ in range(ns.repeats):
                for k, fn in arms.items():
                    times[k].append(timed(fn)[0])
            levels, pad = um.split_levels(ns.size, ns.size, ns.refield, ns.min_size, 1) if mode != 3 else ([(ns.size, ns.size)], (ns.size,) * 2)
            rec = {"forwards_sequential": (8 if mode != 2 else 1) * 4 ** (len(levels) - 1), "tile": list(pad),
                   "mean_abs_diff": d.mean().item(), "max_abs_diff": d.max().item()}
            for k, v in times.items():
                rec[f"{k}_ms"] = round(statistics.median(v) * 1e3, 2)
                rec[f"{k}_spread_ms"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
            rec["sequential_over_batched"] = round(rec["sequential_ms"] / rec["batched_ms"], 3)
            out["modes"][str(mode)] = rec
            print(mode, rec, flush=True)
            del ya, yb, d
            torch.cuda.empty_cache()
        out["kernels"] = kernel_rates(L, sf, ns.refield, ns.min_size, ns.kernel_iters)
        print(out["kernels"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
