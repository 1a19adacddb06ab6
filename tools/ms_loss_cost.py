#!/usr/bin/env python3
"""Cost of the multi-image loss on the MSLapSRN x8 training step: B = 8 synthetic 512 x 512 HR patches (64 x 64 LR), one
MI355X, one process, the arms alternated round by round.

    python tools/ms_loss_cost.py [--batch 8] [--steps 20] [--rounds 5] [--graph] [--out profiles/ms_loss_cost.json]

Arms (ModelPlain.optimize_parameters: the eager step, this engine's default; --graph: the step replayed from its hipGraph):
  l1_aten     --l1 True, the level targets by stock torch (clamp(F.interpolate(bicubic, align_corners=True)) per level, the
              step before the pyramid kernel)
  l1          --l1 True, the level targets by srhip_resize_bicubic_ac_pyramid (one launch)
  readme      --l1 False --l2 True --ssim True --ssim_lambda 5.0 --ssim_window_s 19

Per arm: ms per step of every round (device-synchronised host clock around `steps` steps), the median and the spread over the
rounds -> one JSON line.  The spread of l1_aten is the yardstick for "l1 is not slower"."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["SRHIP_TRAIN_GRAPH"] = "1" if a.graph else "0"
    import torch
    import torch.nn.functional as F
    import main as M
    from dlib.models.select_model import define_model
    from srhip import ops
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about the step"

    def aten_pyramid(src, shapes, out=None, clamp=True):
        return [src if tuple(s) == tuple(src.shape[-2:]) else
                torch.clamp(F.interpolate(src, size=tuple(s), mode="bicubic", align_corners=True), 0.0, 1.0).contiguous()
                for s in shapes]
    kernel_pyramid = ops.resize_bicubic_ac_pyramid
    base = ["--net_type", "MSLapSRN", "--method", "MSLAPSR", "--task", "super-resolution", "--scale", "8", "--n_channels", "1",
            "--h_size", "512", "--batch_size", str(a.batch)]
    readme = ["--l1", "False", "--l2", "True", "--ssim", "True", "--ssim_lambda", "5.0", "--ssim_window_s", "19"]
    arms = {}
    for name, extra, pyr in (("l1_aten", [], aten_pyramid), ("l1", [], kernel_pyramid), ("readme", readme, kernel_pyramid)):
        model = define_model(M.parse_input(base + extra))
        model.init_train()
        arms[name] = (model, pyr)
    batch = M.synth_batch(a.batch, 8, 512, arms["l1"][0].device, 7)

    def run(name, n):
        model, pyr = arms[name]
        ops.resize_bicubic_ac_pyramid = pyr       # train.py looks it up at call time; a captured graph keeps what it captured
        for i in range(n):
            model.feed_data(batch)
            model.optimize_parameters(epoch=0, current_step=i + 1)
        torch.cuda.synchronize()
    for name in arms:
        run(name, 4)            # eager step, capture, replays
    times = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps)
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    ops.resize_bicubic_ac_pyramid = kernel_pyramid
    row = {"what": "MSLapSRN x8 ModelPlain.optimize_parameters, ms per step", "batch": a.batch, "steps": a.steps,
           "graph": {n: bool(getattr(m.step_fn, "_graph", None) and m.step_fn._graph["g"] is not None) for n, (m, _) in arms.items()},
           "loss": {n: [float(v) for v in m.step_fn.loss_values()] for n, (m, _) in arms.items()}}
    for name, t in times.items():
        row[name] = {"ms": [round(v, 4) for v in t], "median": round(statistics.median(t), 4),
                     "spread": round(max(t) - min(t), 4)}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
