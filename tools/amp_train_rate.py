"""Training rate of EDSR-baseline (16 ResBlocks x 64 features, the bench.py workloads edsr_x8 / x4 / x2: B = 8, LR (512/s)^2,
L1, Adam) for the f32-grade step and the --amp step (fp16 storage + the GradScaler's rules, TrainStep(amp=True)), both
replayed from their captured graphs (TrainStep.step_graph, ModelPlain's default for EDSR), in ONE process and alternated
round by round, timed with device events.  Prints one JSON line: patches/s per scale and step kind, and their ratio.

    python tools/amp_train_rate.py [--scales 8,4,2] [--batch 8] [--steps 10] [--warmup 3] [--rounds 3] [--kinds f32,amp]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sr-caco-2_amd"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def make_step(scale, amp):
    import sr_oracle as O
    from dlib.models.network_edsr_liif import EDSR_LIIF
    from srhip.train import Optimizer, TrainStep
    cfg = O.edsr_config(upscale=scale)
    net = EDSR_LIIF(scale=scale)
    net.load_state_dict(O.edsr_init_state_dict(cfg, seed=0), strict=True)
    net = net.cuda()
    net.amp = amp
    st = TrainStep(net, [("l1", 1.0)], amp=amp)
    st.opt = Optimizer(st.fp, "adam", lr=2e-4)
    return st


def timed(st, x, y, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        st.step_graph(x, y)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="8,4,2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kinds", default="f32,amp", help="amp alone: the step a kernel trace looks at")
    a = ap.parse_args()
    out = {"tool": "amp_train_rate", "batch": a.batch, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for s in [int(v) for v in a.scales.split(",")]:
        lr = 512 // s
        g = torch.Generator(device="cuda").manual_seed(s)
        x = torch.rand(a.batch, 1, lr, lr, device="cuda", generator=g)
        y = torch.rand(a.batch, 1, lr * s, lr * s, device="cuda", generator=g)
        steps = {k: make_step(s, k == "amp") for k in a.kinds.split(",")}
        for st in steps.values():
            for _ in range(max(a.warmup, 2)):      # eager (buffers), capture, replays
                st.step_graph(x, y)
        torch.cuda.synchronize()
        best = {k: float("inf") for k in steps}
        for _ in range(a.rounds):                   # alternated: both see the same clocks / thermals
            for k, st in steps.items():
                best[k] = min(best[k], timed(st, x, y, a.steps))
        rate = {k: a.batch * a.steps / t for k, t in best.items()}
        out[f"x{s}"] = {f"{k}_patches_per_s": round(v, 1) for k, v in rate.items()}
        if len(rate) == 2:
            out[f"x{s}"]["amp_speedup"] = round(rate["amp"] / rate["f32"], 3)
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
