"""Training rate of EDSR-baseline (--net edsr: 16 ResBlocks x 64 features, the bench.py workloads edsr_x8 / x4 / x2) or of
DRRN (--net drrn: the registry's 25 residual units x 128 features) at B = 8, LR (512/s)^2, L1, Adam, for the f32-grade step
and the --amp step (fp16 storage + the GradScaler's rules, TrainStep(amp=True)), both replayed from their captured graphs
(TrainStep.step_graph), in ONE process and alternated round by round, timed with device events.  Prints one JSON line:
patches/s per scale and step kind, their ratio, and each step's peak memory (what its buffers, workspaces and the
transients of its warm-up steps added to the allocator's peak; the f32-grade step is made and warmed up first).

    python tools/amp_train_rate.py [--net edsr|drrn] [--scales 8,4,2] [--batch 8] [--steps 10] [--warmup 3] [--rounds 3]
                                   [--kinds f32,amp]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sr-caco-2_amd"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def make_step(net_name, scale, amp):
    import sr_oracle as O
    from srhip.train import Optimizer, TrainStep
    if net_name == "drrn":
        from dlib.models.network_drrn import DRRN
        net = DRRN(in_chans=1, upscale=scale, num_residual_units=25)
        net.load_state_dict(O.drrn_init_state_dict(1, seed=0), strict=True)
    else:
        from dlib.models.network_edsr_liif import EDSR_LIIF
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
    ap.add_argument("--net", choices=("edsr", "drrn"), default="edsr")
    ap.add_argument("--scales", default="8,4,2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kinds", default="f32,amp", help="amp alone: the step a kernel trace looks at")
    a = ap.parse_args()
    out = {"tool": "amp_train_rate", "net": a.net, "batch": a.batch, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for s in [int(v) for v in a.scales.split(",")]:
        lr = 512 // s
        g = torch.Generator(device="cuda").manual_seed(s)
        x = torch.rand(a.batch, 1, lr, lr, device="cuda", generator=g)
        y = torch.rand(a.batch, 1, lr * s, lr * s, device="cuda", generator=g)
        steps, peak = {}, {}
        for k in a.kinds.split(","):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            st = steps[k] = make_step(a.net, s, k == "amp")
            for _ in range(max(a.warmup, 2)):      # eager (buffers), capture, replays
                st.step_graph(x, y)
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        best = {k: float("inf") for k in steps}
        for _ in range(a.rounds):                   # alternated: both see the same clocks / thermals
            for k, st in steps.items():
                best[k] = min(best[k], timed(st, x, y, a.steps))
        rate = {k: a.batch * a.steps / t for k, t in best.items()}
        out[f"x{s}"] = {f"{k}_patches_per_s": round(v, 1) for k, v in rate.items()}
        out[f"x{s}"].update({f"{k}_ms_per_step": round(1e3 * best[k] / a.steps, 2) for k in steps})
        out[f"x{s}"].update({f"{k}_peak_memory_gib": round(v, 2) for k, v in peak.items()})
        if len(rate) == 2:
            out[f"x{s}"]["amp_speedup"] = round(rate["amp"] / rate["f32"], 3)
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
