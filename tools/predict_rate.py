#!/usr/bin/env python
"""Time per page of prediction on images without an HR partner (srhip/predict.py) on the README's SwinIR, x8, a 3-page 16-bit
256 x 256 stack.

Ingest + emit: arm A, the two launches of this package (srhip_ingest_pad: uint16 -> [0, 1] float32 padded to 264 x 264;
srhip_emit_uint: the net's 2112 x 2112 output -> uint16 2048 x 2048 pages and the non-finite flag), against arm B, the torch
composition they replace in the same process: cast, divide, two cat + flip; slice, clamp, multiply, round, cast.  Both arms
read and write the same device tensors.  An arm is warmed up, then timed --repeats times, alternating, each timing HIP events
around --iters runs of the arm; the median is reported with the spread, per page, and whether the torch arm gave the bits of
the HIP arm (which the tests pin to the reference's rounding).

Beside it the whole ``Predictor.run`` per page (upload, ingest, forward, emit, download): a host clock around the call, which
ends in the download; median of --repeats after a warm-up.

    python tools/predict_rate.py --out profiles/predict_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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


def make_experiment(folder):
    """a reference-format experiment folder holding the README SwinIR x8 with seeded random weights"""
    import torch
    import main as M
    from dlib.models.select_model import define_model
    from dlib.utils.utils_config import save_config
    args = M.parse_input("--method SWINIR --net_type swinir --scale 8 --n_channels 1 --h_size 512 --swinir_window_size 8 "
                         "--swinir_depths 6+6+6+6 --swinir_embed_dim 180 --swinir_num_heads 6+6+6+6 --swinir_mlp_ratio 2 "
                         "--swinir_upsampler pixelshuffledirect --amp False".split())
    os.makedirs(os.path.join(folder, "best-models"), exist_ok=True)
    save_config(args, folder, "config_model.yml")
    torch.manual_seed(0)
    model = define_model(args)
    torch.save(model.netG.state_dict(), os.path.join(folder, "best-models", "G-model.pth"))
    return args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_rate.json"))
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pages", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ns = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/predict_rate.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from srhip import ops
    from srhip.predict import Predictor, padded_size
    N, H, W, m = ns.pages, ns.size, ns.size, 65535
    pages = np.random.RandomState(1).randint(0, m + 1, size=(N, H, W)).astype(np.uint16)
    with tempfile.TemporaryDirectory() as folder:
        args = make_experiment(folder)
        sf = int(args.scale)
        pred = Predictor(folder, batch=N, out_dtype="float32")
        Hp, Wp = padded_size(pred.args, H, W)
        sH, sW = H * sf, W * sf
        pred.run(pages)                                              # warm-up of the net at this shape
        E = pred.model.E.detach().float().contiguous()               # the net's own (padded) output: what emit reads
        assert tuple(E.shape) == (N, 1, Hp * sf, Wp * sf), E.shape
        src = torch.from_numpy(pages).cuda()
        h_pad, w_pad = Hp - H, Wp - W
        x_a = torch.empty(N, Hp, Wp, device="cuda")
        u_a = torch.empty(N, sH, sW, dtype=torch.uint16, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        E3 = E.view(N, Hp * sf, Wp * sf)
        keep = {}

        def arm_hip():
            ops.ingest_pad(src, m, Hp, Wp, out=x_a)
            ops.emit_uint(E3, 16, sH, sW, flag=flag, out=u_a)

        def arm_torch():
            im = (src.to(torch.float32) / float(m))[:, None]
            im = torch.cat([im, torch.flip(im[:, :, H - h_pad:, :], [2])], 2)
            im = torch.cat([im, torch.flip(im[:, :, :, W - w_pad:], [3])], 3)
            keep["x"] = im
            keep["u"] = (E[..., :sH, :sW].clamp(0, 1) * float(m)).round().to(cast)

        cast = torch.uint16
        try:
            arm_torch()
            torch.cuda.synchronize()
        except RuntimeError:                                        # this torch has no float -> uint16 cast on the device:
            cast = torch.int32                                      # the arm writes twice the bytes in its last step; recorded
        arms = {"hip_two_launches": arm_hip, "torch_composition": arm_torch}
        for fn in arms.values():                                    # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # (torch divides by a scalar as a product with its reciprocal: its ingest is not the reference's rounding everywhere)
        same = {"ingest": bool(torch.equal(keep["x"][:, 0], x_a)),
                "ingest_max_abs_diff": (keep["x"][:, 0] - x_a).abs().max().item(),
                "emit": bool(torch.equal(keep["u"][:, 0].to(torch.int32), u_a.to(torch.int32)))}
        times = {k: [] for k in arms}
        for _ in range(ns.repeats):
            for k, fn in arms.items():
                times[k].append(event_ms(fn, ns.iters) / N)
        out = {"tool": "tools/predict_rate.py", "device": torch.cuda.get_device_name(0),
               "net": "SwinIR README configuration (window 8, depths 6x4, embed 180, heads 6x4, mlp_ratio 2, pixelshuffledirect), "
                      "seeded random weights",
               "scale": sf, "stack": {"pages": N, "lr": [H, W], "dtype": "uint16", "padded": [Hp, Wp], "out": [sH, sW]},
               "repeats": ns.repeats, "iters_per_timing": ns.iters, "timer": "HIP events around the arm",
               "ingest_plus_emit_per_page": {"torch_arm_equals_hip": same, "torch_arm_last_cast": str(cast)}}
        rec = out["ingest_plus_emit_per_page"]
        for k, v in times.items():
            rec[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
            rec[f"{k}_spread_us"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
        rec["torch_over_hip"] = round(rec["torch_composition_us"] / rec["hip_two_launches_us"], 2)
        # bytes the two passes must move per page: the page in, the padded float image out; the crop in, the page out
        nbytes = H * W * 2 + Hp * Wp * 4 + sH * sW * 4 + sH * sW * 2
        rec["bytes_per_page"] = nbytes
        rec["hip_GBps"] = round(nbytes / (rec["hip_two_launches_us"] * 1e-6) / 1e9, 1)
        print(rec, flush=True)
        for dt_name in ("uint16", "float32"):
            pred.out_dtype = "same" if dt_name == "uint16" else dt_name
            pred.run(pages)
            runs = []
            for _ in range(ns.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pred.run(pages)
                runs.append((time.perf_counter() - t0) / N)
            out[f"predictor_run_per_page_{dt_name}"] = {
                "timer": "host clock around Predictor.run (ends in the download)", "ms": round(statistics.median(runs) * 1e3, 3),
                "spread_ms": [round(min(runs) * 1e3, 3), round(max(runs) * 1e3, 3)]}
            print(dt_name, out[f"predictor_run_per_page_{dt_name}"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    with open(ns.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {ns.out}")


if __name__ == "__main__":
    main()
