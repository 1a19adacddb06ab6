#!/usr/bin/env python3
"""Headline benchmark: training patches/sec of the patch-level hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload swinir_x8|edsr_x8|edsr_x4|edsr_x2] [--full]
                    [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the result line; everything else it can measure (the
eager rates, the live roofline, the forward-only figures, config.secondary, torch_rocm_baseline, cpu_baseline) runs
behind the timed steps only with --full.  --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy.

One process per GPU.  With --gpus N > 1 and no WORLD_SIZE in the environment the
script launches itself under ``python -m torch.distributed.run`` (before any GPU
call is made in this process) and relays rank 0's JSON line, so the documented
command is one line; under torchrun (RANK / LOCAL_RANK / WORLD_SIZE set) it is the
worker.  A step is forward + loss + backward + (RCCL gradient all-reduce) +
optimizer on one synthetic batch of 8 patches per GPU:

  swinir_x8 (default, BASELINE.json's metric): SwinIR README.md:120-197 configuration
            (embed 180, depths 6x4, heads 6, window 8, mlp 2, pixelshuffledirect), LR 64^2 -> HR 512^2,
            L1, SGD-Nesterov
  edsr_x{8,4,2}: EDSR-baseline (16 ResBlocks x 64 features), LR (512/s)^2 -> HR 512^2, L1, Adam

Rank 0 prints ONE JSON line.  ``value`` = patches of all ranks / wall time of exactly K steps between
barrier + synchronize pairs (max over ranks); ``step_ms`` = median / p10 / p90 of the per-step durations
from HIP events recorded on the compute stream; with --full: ``roofline`` = the dominant KERNEL (largest summed launch time) timed
live with HIP events around every launch of three eager steps run right BEHIND the timed region (events cannot be recorded
inside a hipGraph replay and an event pair slows a step: the timed K steps carry none); ``cpu_baseline`` = the oracle (PyTorch-fp32
CPU restatement, validated against the reference) timed on the host cores on a bounded sample, B=1 and B=8.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))

# algorithmic work per patch, FORWARD (SURVEY.md 8d / BASELINE.md; fwd + bwd = 3x): GFLOP, GB
WORK = {"swinir_x8": (68.30, 2.853), "edsr_x8": (35.64, 0.518), "edsr_x4": (64.34, 0.976),
        "edsr_x2": (179.16, 2.809)}
F32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
BX3_PEAK_TFLOPS = 2500.0 / 6.0   # bf16 dense / 6 products per f32-accurate product
HBM_PEAK_GBS = 8000.0


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="swinir_x8", choices=sorted(WORK))
    ap.add_argument("--batch", type=int, default=8, help="patches per GPU (README --batch_size 8)")
    ap.add_argument("--loss", default="l1", choices=["l1", "l2ssim"])
    ap.add_argument("--optimizer", default=None, choices=["sgd", "adam"])
    ap.add_argument("--graph", action="store_true", help="replay the step from a hipGraph (TrainStep.step_graph) also under data "
                    "parallelism; on ONE GPU that is the default since round 5 (what ModelPlain.optimize_parameters does)")
    ap.add_argument("--no-graph", action="store_true", help="eager steps only")
    ap.add_argument("--droppath-per-rank", action="store_true", help="every rank draws its own DropPath masks; default: all "
                    "ranks draw the same ones, as the reference's trainer seeds every rank with myseed + current_step "
                    "(utils_trainer.py:359-361)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the EDSR x8 / x4 / x2 lines under config.secondary")
    ap.add_argument("--train-only", action="store_true",
                    help="profiling runs: nothing but the warm-up and the timed training steps (no evaluation figure, no "
                         "secondary workloads, no CPU baseline), so that per-kernel statistics and PMC byte counts divide "
                         "by the step count")
    ap.add_argument("--full", action="store_true",
                    help="behind the timed steps, also measure everything beside the headline (eager rates, roofline, "
                         "forward-only figures, secondary workloads, torch and CPU baselines); the --no-* options and "
                         "--train-only leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (the loss buffer, the updated "
                         "parameters and their gradients) as DIR/<name>.npy, float32")
    args = ap.parse_args(argv)
    if not args.full:           # a plain run: set-up, warm-up, the K timed steps and the result line
        args.train_only = args.no_roofline = True
    return args


# ------------------------------------------------------------------ parent: self-launch
def launch_workers(args):
    """--gpus N > 1 outside torchrun: start the N workers as CHILD processes (this process has not
    touched the GPU and never execs), relay rank 0's JSON line, propagate failure."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, text=True, env=env)
    line = None
    for out in p.stdout:
        if out.startswith('{"metric"'):
            line = out.strip()
        else:
            sys.stderr.write(out)
    rc = p.wait()
    if rc != 0 or line is None:
        sys.stderr.write(f"bench.py: worker launch failed (exit {rc}, json line {'seen' if line else 'missing'})\n")
        return rc or 1
    print(line, flush=True)
    return 0


# ------------------------------------------------------------------ worker
def synth_batch(batch, scale, device, seed):
    """H = round(rand*255)/255; L = clamp(bicubic_down(H), 0, 1)."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    hr = (torch.rand(batch, 1, 512, 512, generator=g) * 255).round() / 255
    lr = F.interpolate(hr, scale_factor=1.0 / scale, mode="bicubic").clamp(0, 1)
    return lr.to(device), hr.to(device)


DUMP_MAX_ELEMS = 6_000_000      # per array: the parameters and gradients of SwinIR x8 stay under 64 MB together


def write_outputs(outdir, arrays):
    """{name: tensor} -> outdir/<name>.npy, flattened to float32.  A tensor of more than DUMP_MAX_ELEMS elements is
    written as a sample of that many, at sorted indices drawn from a fixed seed (the same ones for the same size), so
    that two builds of the project compare output for output."""
    import numpy as np
    import torch
    os.makedirs(outdir, exist_ok=True)
    for name, t in arrays.items():
        v = t.detach().float().reshape(-1).cpu()
        if v.numel() > DUMP_MAX_ELEMS:
            idx = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_MAX_ELEMS]
            v = v[idx.sort().values]
        np.save(os.path.join(outdir, f"{name}.npy"), v.numpy())


def measured_bytes_per_step(workload):
    """HBM bytes one training step moved in the COMMITTED rocprofv3 PMC passes of this workload (newest
    profiles/r0N_hbm_traffic_per_kernel_<workload>_b8.json: FETCH_SIZE x 2 + WRITE_SIZE per launch x launches,
    tools/collect_traffic.sh), divided by the optimizer launches of that run (= its steps).  Not counters of the run being
    reported: the keys that use it say 'from_committed_pmc' and name the file.  None if not collected, or if the profile
    was collected from other kernel sources than the ones this library was built from (its `_meta.csrc_sha16`)."""
    tag = workload.replace("swinir_x8", "swinir")
    for r in (9, 8, 7, 6, 5, 4, 3, 2):
        path = os.path.join(ROOT, "profiles", f"r0{r}_hbm_traffic_per_kernel_{tag}_b8.json")
        if os.path.isfile(path):
            table = json.load(open(path))
            from srhip.probe import csrc_hash
            if table.pop("_meta", {}).get("csrc_sha16") != csrc_hash():
                return None, None       # the newest profile belongs to another build of the kernels: no figure
            steps = sum(v["launches"] for k, v in table.items() if "k_sgd_dc" in k or "k_adam_dc" in k)
            if steps:
                tot = sum(v["hbm_bytes_per_launch"] * v["launches"] for v in table.values())
                return tot / steps, os.path.basename(path)
    return None, None


def secondary_edsr(scale, batch, dev, steps=10, warmup=3):
    """One EDSR-baseline workload (BASELINE.json configs[1]: x4; north_star's HBM target: x8) for `steps` training
    steps after the headline's timed region, so that its figures are driver-observed too: patches/s, whole-step
    hbm_frac (algorithmic bytes) and the dominant kernel class's live roofline fraction."""
    import torch
    from srhip import probe
    from srhip.train import TrainStep, Optimizer
    from dlib.models.network_edsr_liif import EDSR_LIIF
    torch.manual_seed(0)
    net = EDSR_LIIF(scale=scale).to(dev).train()
    ts = TrainStep(net, [("l1", 1.0)])
    ts.opt = Optimizer(ts.fp, "adam", lr=2e-4, wd=1e-4)
    lr_img, hr_img = synth_batch(batch, scale, dev, seed=2000 + scale)
    for _ in range(warmup):
        ts.step(lr_img, hr_img)
    torch.cuda.synchronize()
    kinds = ("conv_nt", "conv_tn")
    t0 = time.perf_counter()
    for i in range(steps):
        ts.step(lr_img, hr_img)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the dominant kernel's live roofline from ONE more step with HIP events around every launch, outside the timed steps
    # (inside, the ~100 event pairs of that step cost the 10-step average 5 %: 1,616 against 1,704 patches/s at x8)
    probe.enable(kinds)
    ts.step(lr_img, hr_img)
    roof = probe.collect()
    probe.disable()
    pps = batch * steps / dt
    gflop, gbyte = WORK[f"edsr_x{scale}"]
    out = {"patches_per_s": pps, "ms_per_step": 1000.0 * dt / steps, "steps": steps,
           "hbm_frac": gbyte * 3.0 * pps / HBM_PEAK_GBS, "final_loss": ts.loss_values()[0]}
    mb, src = measured_bytes_per_step(f"edsr_x{scale}")
    if mb:
        out["hbm_frac_from_committed_pmc"] = mb * (pps / batch) / 1e9 / HBM_PEAK_GBS
        out["committed_pmc_gbyte_per_step"] = mb / 1e9
        out["committed_pmc_source"] = src
    if roof:
        out["dominant_kernel"] = {"kernel": roof["kernel"].split(":")[0], "frac": roof["frac"], "peak": roof["peak"],
                                  "achieved": roof["achieved"], "unit": roof["unit"], "avg_launch_us": roof["avg_launch_us"]}
    del ts, net
    torch.cuda.empty_cache()
    return out



EVAL_NETS = [("swinir", "SWINIR"), ("EDSR_LIIF", "EDSR_LIIF"), ("VDSR", "VDSR"), ("DRRN", "DRRN"), ("SRCNN", "SRCNN"),
             ("MSLapSRN", "MSLAPSR"), ("MemNet", "MemNet"), ("DBPN", "DBPN"), ("SRFBN", "SRFBN"), ("ProSR", "PROSR"),
             ("ENLCN", "ENLCN"), ("NLSN", "NLSN"), ("DFCAN", "DFCAN"), ("ACT", "ACT"), ("OmniSR", "OmniSR"), ("GRL", "GRL")]


def secondary_exact_f32(batch, dev, steps=5, warmup=2):
    """The headline workload on the EXACT-f32 matrix path (SRHIP_MM=f32: v_mfma_f32_32x32x2_f32, no operand split) for a
    few steps: what the fp16x2 split (22 significant bits per operand, three products) buys over IEEE f32 products."""
    import torch
    from srhip.train import TrainStep, Optimizer
    from dlib.models.network_swinir import SwinIR
    old = os.environ.get("SRHIP_MM")
    os.environ["SRHIP_MM"] = "f32"
    try:
        torch.manual_seed(0)
        net = SwinIR(upscale=8, in_chans=1, img_size=64, window_size=8, depths=[6, 6, 6, 6], embed_dim=180,
                     num_heads=[6, 6, 6, 6], mlp_ratio=2, upsampler="pixelshuffledirect").to(dev).train()
        ts = TrainStep(net, [("l1", 1.0)])
        ts.opt = Optimizer(ts.fp, "sgd", lr=0.01, momentum=0.9, nesterov=True, wd=0.0)
        lr_img, hr_img = synth_batch(batch, 8, dev, seed=1000)
        torch.manual_seed(1234)
        for _ in range(warmup):
            ts.step(lr_img, hr_img)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ts.step(lr_img, hr_img)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = {"patches_per_s": batch * steps / dt, "ms_per_step": 1000.0 * dt / steps, "steps": steps,
               "final_loss": ts.loss_values()[0], "matmul": "exact f32 MFMA (v_mfma_f32_32x32x2_f32), f32 operands"}
        del ts, net
        torch.cuda.empty_cache()
        return out
    finally:
        if old is None:
            os.environ.pop("SRHIP_MM", None)
        else:
            os.environ["SRHIP_MM"] = old


def secondary_model_plain(batch, steps=20, warmup=3):
    """The headline workload through the PRODUCT entry point: main.parse_input (the README's flags) -> define_model ->
    ModelPlain.feed_data / optimize_parameters, what `main.py` runs per iteration -- against `value`, which times
    TrainStep.step directly.  (profiles/r04_train_sweep.json's 379 patches/s was the REGISTRY-DEFAULT SwinIR -- 36 blocks and
    the conv 'pixelshuffle' upsampler, Adam -- not this README net of 24 blocks / 'pixelshuffledirect': VERDICT r4 item 3.)"""
    import torch
    import main as M
    from dlib.models.select_model import define_model
    argv = ["--task", "super-resolution", "--scale", "8", "--method", "SWINIR", "--net_type", "swinir", "--n_channels", "1",
            "--h_size", "512", "--batch_size", str(batch), "--G_optimizer_type", "sgd", "--G_optimizer_lr", "0.01",
            "--G_optimizer_wd", "0.0", "--G_scheduler_type", "MyStepLR", "--G_scheduler_step_size", "30",
            "--G_scheduler_gamma", "0.5", "--swinir_window_size", "8", "--swinir_depths", "6+6+6+6",
            "--swinir_embed_dim", "180", "--swinir_num_heads", "6+6+6+6", "--swinir_mlp_ratio", "2",
            "--swinir_upsampler", "pixelshuffledirect", "--l1", "True", "--amp", "False",
            "--outd", os.path.join(ROOT, "gpurun_out", "bench_model_plain")]
    args = M.parse_input(argv)
    torch.manual_seed(0)
    model = define_model(args)
    model.init_train()
    model.feed_data(M.synth_batch(batch, 8, 512, model.device, 1000))
    for k in range(warmup):
        model.optimize_parameters(0, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        model.optimize_parameters(0, warmup + k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"patches_per_s": batch * steps / dt, "ms_per_step": 1000.0 * dt / steps, "steps": steps,
           "entry": "main.parse_input -> define_model -> ModelPlain.optimize_parameters (README flags, L1, SGD-Nesterov)",
           "final_loss": float(model.current_log()["G_loss"]), "finite": bool(model.check_finite())}
    del model
    torch.cuda.empty_cache()
    return out


def torch_rocm_baseline(batch, dev, steps=5, warmup=2):
    """The same step through the vendor-library path on the SAME GPU: the oracle's module (plain PyTorch ops: aten /
    rocBLAS / MIOpen kernels, fp32, autograd) on cuda, same batch, same L1 loss, SGD-Nesterov by torch.optim.  The
    checker is timed here as a baseline, never shipped (oracle/ header)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import sr_oracle as O
    cfg = O.swinir_config(drop_path_rate=0.0)
    sd = {k: v.to(dev) for k, v in O.swinir_init_state_dict(cfg, seed=0).items()}
    params = []
    for k, v in sd.items():
        if v.dtype == torch.float32 and not k.endswith("attn_mask"):
            v.requires_grad_(True)
            params.append(v)
    opt = torch.optim.SGD(params, lr=0.01, momentum=0.9, nesterov=True)
    lr_img, hr_img = synth_batch(batch, 8, dev, seed=1000)

    def step():
        opt.zero_grad(set_to_none=True)
        O.loss_l1(O.swinir_forward(sd, lr_img, cfg), hr_img).backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"value": batch * steps / dt, "unit": "patches/s", "ms_per_step": 1000.0 * dt / steps, "steps": steps,
           "what": "oracle SwinIR x8 README module on cuda: stock PyTorch-ROCm kernels (aten elementwise, rocBLAS/hipBLASLt "
                   "GEMMs, MIOpen convs), fp32, autograd + torch.optim.SGD(nesterov); DropPath off; same B, same GPU",
           "torch": torch.__version__}
    del sd, params, opt
    torch.cuda.empty_cache()
    return out


def secondary_eval_x8(batch, iters=3):
    """BASELINE.json config 5 at x8: model.test() patches/s of every registry network, fp32-accurate kernels and with
    --amp True (reduced-precision kernels where the network takes them), a few iterations each."""
    import torch
    import main as M
    from dlib.models.select_model import define_model
    rows = {}
    for net_type, method in EVAL_NETS:
        row = {}
        for amp in (False, True):
            argv = ["--net_type", net_type, "--method", method, "--task", "super-resolution", "--scale", "8",
                    "--n_channels", "1", "--h_size", "512", "--batch_size", str(batch), "--amp", str(amp),
                    "--outd", os.path.join(ROOT, "gpurun_out", "bench_eval")]
            args = M.parse_input(argv)
            torch.manual_seed(0)
            model = define_model(args)
            model.netG.eval()
            data = M.synth_batch(batch, 8, 512, model.device, 7)
            model.feed_data(data)
            if net_type == "MemNet":
                # BatchNorm running statistics from a few training-mode forwards on a crop: with the initial (0, 1) the
                # feature maps grow by orders of magnitude per memory block (and leave fp16's range under --amp)
                model.netG.train()
                with torch.no_grad():
                    crop = model.L[:2, :, :32, :32].contiguous()
                    for _ in range(30):
                        model.netG(crop)
                model.netG.eval()
            model.test()                                   # weight preparation, buffers
            model.test()
            torch.cuda.synchronize()
            # median of `iters` spans of two forwards each: one stray host stall (allocator, page faults behind empty_cache)
            # inside a single short span once read 30x low for a 1-ms forward
            spans = []
            for _ in range(iters):
                t0 = time.perf_counter()
                model.test()
                model.test()
                torch.cuda.synchronize()
                spans.append((time.perf_counter() - t0) / 2)
            dt = sorted(spans)[len(spans) // 2]
            assert tuple(model.E.shape[-2:]) == (512, 512) and bool(torch.isfinite(model.E).all())
            row["amp_patches_per_s" if amp else "patches_per_s"] = batch / dt
            if amp:
                row["reduced_precision_kernels"] = bool(getattr(model.netG, "amp", False)
                                                        and getattr(model.netG, "amp_takes_effect", True))
                eng = getattr(model.netG, "_engine", None)
                row["amp_storage"] = getattr(eng, "last_eval_path", "f32 storage")
            del model
            torch.cuda.empty_cache()
        rows[net_type] = row
    return {"batch": batch, "iters": iters, "nets": rows}


def physical_cores():
    """sockets x cores per socket from lscpu (hardware threads are reported separately)."""
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {l.split(":")[0].strip(): l.split(":")[1].strip() for l in out.splitlines() if ":" in l}
        return int(kv["Socket(s)"]) * int(kv["Core(s) per socket"])
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline(workload, optimizer):
    """Oracle fwd + L1 + bwd + optimizer on the host, the same workload at B=1 and B=8, bounded to
    ~25 s: B=1 steps for ~8 s, then one warm-up + up to two timed B=8 steps."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import sr_oracle as O
    cores = physical_cores()
    threads = min(32, os.cpu_count() or 1)   # a few dozen threads is where torch's CPU kernels peak here
    torch.set_num_threads(threads)
    scale = int(workload.split("_x")[1])
    if workload.startswith("swinir"):
        cfg = O.swinir_config(drop_path_rate=0.0)
        sd = O.swinir_init_state_dict(cfg, seed=0)
        fwd = lambda x: O.swinir_forward(sd, x, cfg)
    else:
        cfg = O.edsr_config(upscale=scale)
        sd = O.edsr_init_state_dict(cfg, seed=0)
        fwd = lambda x: O.edsr_forward(sd, x, cfg)
    for k, v in sd.items():
        if v.dtype == torch.float32 and not k.endswith("attn_mask"):
            v.requires_grad_(True)
    params = [v for v in sd.values() if v.requires_grad]
    m = [torch.zeros_like(p) for p in params]
    v2 = [torch.zeros_like(p) for p in params]
    count = [0]

    def step(lr, hr):
        for p in params:
            p.grad = None
        O.loss_l1(fwd(lr), hr).backward()
        count[0] += 1
        with torch.no_grad():
            for i, p in enumerate(params):
                if optimizer == "sgd":
                    O.sgd_nesterov_step(p, p.grad, m[i], count[0] == 1, 0.01)
                else:
                    O.adam_step(p, p.grad, m[i], v2[i], count[0], 2e-4, wd=1e-4)

    res = {}
    for B, budget, max_steps in ((1, 8.0, 12), (8, 12.0, 2)):
        lr, hr = synth_batch(B, scale, "cpu", 0)
        step(lr, hr)                                   # untimed warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            step(lr, hr)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= budget or n >= max_steps:
                break
        res[B] = {"patches_per_s": B * n / dt, "steps": n, "seconds": dt}
    best = max(res, key=lambda b: res[b]["patches_per_s"])
    return {"value": res[best]["patches_per_s"], "unit": "patches/s", "cores": cores, "threads": threads,
            "kind": "port", "b1": res[1], "b8": res[8],
            "sample": f"{workload}: oracle fwd+L1+bwd+{optimizer}, fp32, {threads} threads on {cores} physical cores; "
                      f"B=1: {res[1]['steps']} steps in {res[1]['seconds']:.1f} s, B=8: {res[8]['steps']} steps in "
                      f"{res[8]['seconds']:.1f} s (each after one warm-up step); value = the better of the two"}


def worker(args):
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE\n")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    n_ranks_seen = 1
    if world > 1 or os.environ.get("SRHIP_FORCE_DDP", "0") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # nccl == RCCL
        pg = dist.group.WORLD
        n_ranks_seen = dist.get_world_size()

    from srhip import probe
    from srhip.ops import use_bx3 as ops_use_bx3
    from srhip import ops as ops_mod
    from srhip.train import TrainStep, Optimizer

    torch.manual_seed(0)                      # same weights on every rank
    scale = int(args.workload.split("_x")[1])
    if args.workload == "swinir_x8":
        from dlib.models.network_swinir import SwinIR
        net = SwinIR(upscale=8, in_chans=1, img_size=64, window_size=8, depths=[6, 6, 6, 6], embed_dim=180,
                     num_heads=[6, 6, 6, 6], mlp_ratio=2, upsampler="pixelshuffledirect").to(dev).train()
        desc = ("SwinIR x8 README config (embed 180, depths 6+6+6+6, heads 6, window 8, mlp 2, "
                "pixelshuffledirect), LR 1x64x64 -> HR 1x512x512")
        opt_kind = args.optimizer or "sgd"    # README.md:152-159
        kinds = ("gemm_nt", "linear_tn", "wattn", "conv_nt", "mlp_fused", "wmsa_fused")
    else:
        from dlib.models.network_edsr_liif import EDSR_LIIF
        net = EDSR_LIIF(scale=scale).to(dev).train()
        desc = (f"EDSR-baseline x{scale} (16 ResBlocks x 64 features, pixel-shuffle tail), "
                f"LR 1x{512 // scale}x{512 // scale} -> HR 1x512x512")
        opt_kind = args.optimizer or "adam"   # utils_instance.py:216-247 default
        kinds = ("conv_nt", "conv_tn")
    terms = [("l1", 1.0)] if args.loss == "l1" else [("l2", 1.0), ("ssim", 5.0, 19)]
    ts = TrainStep(net, terms, process_group=pg, world_size=world)
    if opt_kind == "sgd":
        ts.opt = Optimizer(ts.fp, "sgd", lr=0.01, momentum=0.9, nesterov=True, wd=0.0,
                           scheduler={"type": "MyStepLR", "step_size": 30, "gamma": 0.5, "min_lr": 1e-4})
    else:
        ts.opt = Optimizer(ts.fp, "adam", lr=2e-4, wd=1e-4)
    lr_img, hr_img = synth_batch(args.batch, scale, dev, seed=1000 + rank)
    # DropPath masks: the reference re-seeds EVERY rank with myseed + current_step (utils_trainer.py:359-361), i.e. the same
    # masks on all ranks; --droppath-per-rank gives each rank its own stream
    torch.manual_seed(1234 + (rank if args.droppath_per_rank else 0))

    def barrier():
        if pg is not None:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    # The step replayed from a hipGraph (bit for bit the eager step; one host call instead of ~330 launches): the default on
    # one GPU since round 5 -- the product entry point (ModelPlain.optimize_parameters) does the same; --graph asks for it
    # under data parallelism too (the RCCL bucket all-reduces are captured with the step), --no-graph for eager steps.  A
    # capture that fails falls back to eager steps for the whole run.  The steps that carry the roofline's per-launch HIP
    # events run eagerly BEHIND the timed region (round 6; VERDICT r5 item 5: one of them used to sit inside it).
    use_graph = (args.graph or world == 1) and not args.no_graph
    gpu_legs = {}                     # wall seconds of every leg that keeps the GPU busy (synchronize-bracketed)
    t_leg = time.perf_counter()
    if use_graph:
        try:
            for _ in range(max(args.warmup, 3)):             # eager step, capture, then replays
                ts.step_graph(lr_img, hr_img)
        except Exception as e:        # noqa: BLE001  (capture not possible here: say so and time eager steps)
            print(f"[bench] hipGraph capture failed ({str(e).splitlines()[0][:160]}): eager steps", file=sys.stderr, flush=True)
            ts._graph = None
            use_graph = False
    if not use_graph:
        for _ in range(args.warmup):
            ts.step(lr_img, hr_img)
    step_fn = ts.step_graph if use_graph else ts.step
    barrier()
    gpu_legs["warmup"] = time.perf_counter() - t_leg
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    for i in range(args.steps):               # the timed region: exactly K steps of the step function, nothing else
        marks[i].record()
        step_fn(lr_img, hr_img)
    marks[args.steps].record()
    barrier()
    dt = time.perf_counter() - t0
    gpu_legs["timed_steps"] = dt
    if args.dump_outputs and rank == 0:
        # what step_fn leaves its caller after the last timed step, before anything below trains on: the loss buffer it
        # returns, the updated parameters and their gradients (named_parameters order, without the flat buffers' padding)
        fp = ts.fp
        write_outputs(args.dump_outputs, {
            "loss": ts.loss_buf,
            "params": torch.cat([fp.flat[fp.offsets[k]:fp.offsets[k] + fp.gviews[k].numel()] for k in fp.names]),
            "grads": torch.cat([fp.gviews[k].reshape(-1) for k in fp.names])})
    # behind the timed region: the same step eagerly (what the earlier rounds' headline timed; ADVICE r5: both methodologies
    # in the line), then three eager steps with HIP events around every launch of the probed op classes (an event pair is two
    # barrier packets: a probed step runs ~18 % slower)
    eager_pps = None
    if use_graph and not args.no_roofline:
        t_leg = time.perf_counter()
        n_eager = min(10, args.steps)
        ts.step(lr_img, hr_img)
        barrier()
        t1 = time.perf_counter()
        for _ in range(n_eager):
            ts.step(lr_img, hr_img)
        barrier()
        eager_pps = args.batch * world * n_eager / (time.perf_counter() - t1)
        gpu_legs["eager_steps"] = time.perf_counter() - t_leg
    # From here on the launches are IN ORDER on one stream (SwinIR: SRHIP_SWIN_SIDE_WGRAD=0 -- the timed steps ran a layer's
    # weight gradients on a side stream beside the next layer's chain, round 6): a kernel that shares the chip with another
    # stream's launch has no duration of its own, and the roofline below is a statement about ONE kernel.  The profiles under
    # profiles/ are taken the same way (tools/refresh_profiles.sh exports the switch).
    side_env = os.environ.get("SRHIP_SWIN_SIDE_WGRAD")
    side_default = (side_env or "1") == "1" and args.workload == "swinir_x8"
    eager_in_order_pps = None
    if not args.no_roofline:
        os.environ["SRHIP_SWIN_SIDE_WGRAD"] = "0"
        if use_graph and side_default:
            ts.step(lr_img, hr_img)
            barrier()
            t1 = time.perf_counter()
            for _ in range(n_eager):
                ts.step(lr_img, hr_img)
            barrier()
            eager_in_order_pps = args.batch * world * n_eager / (time.perf_counter() - t1)
        t_leg = time.perf_counter()
        probe.enable(kinds)
        for _ in range(3):
            ts.step(lr_img, hr_img)
        barrier()
        gpu_legs["probed_steps"] = time.perf_counter() - t_leg
    # PMC traffic of THIS workload's kernels (profiles/, collected with tools/refresh_profiles.sh)
    for r in (9, 8, 7, 6, 5, 4, 3, 2):
        tj = os.path.join(ROOT, "profiles", f"r0{r}_hbm_traffic_per_kernel_{args.workload.replace('swinir_x8', 'swinir')}_b8.json")
        if os.path.isfile(tj):
            os.environ.setdefault("SRHIP_TRAFFIC_JSON", tj)
            break
    roof = probe.collect() if not args.no_roofline else None
    probe.disable()
    if not args.no_roofline:                 # what follows (config.secondary) runs the product's default again
        if side_env is None:
            os.environ.pop("SRHIP_SWIN_SIDE_WGRAD", None)
        else:
            os.environ["SRHIP_SWIN_SIDE_WGRAD"] = side_env
    steps_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))

    def pct(q):
        return steps_ms[min(len(steps_ms) - 1, int(round(q * (len(steps_ms) - 1))))]

    if pg is not None:
        import torch.distributed as dist
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    loss = ts.loss_values()[0]
    # secondary figure, outside the timed region: forward-only patches/s of the same net and batch
    eval_pps = eval_amp_pps = None
    if args.train_only:
        args.no_secondary = args.no_cpu_baseline = True
    if rank == 0 and world == 1 and not args.train_only:
        t_leg = time.perf_counter()
        net.eval()
        with torch.no_grad():
            for _ in range(2):
                net(lr_img)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                net(lr_img)
            torch.cuda.synchronize()
            eval_pps = args.batch * 10 / (time.perf_counter() - t1)
            # config 5: reduced-precision inference (one bf16 product; PSNR-gated in tests/test_gpu_amp.py)
            net.amp = True
            for _ in range(2):
                net(lr_img)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                net(lr_img)
            torch.cuda.synchronize()
            eval_amp_pps = args.batch * 10 / (time.perf_counter() - t1)
            net.amp = False
        net.train()
        gpu_legs["eval_forward"] = time.perf_counter() - t_leg
    secondary = None
    torch_base = None
    if rank == 0 and world == 1 and args.workload == "swinir_x8" and not args.no_secondary:
        t_leg = time.perf_counter()
        secondary = {f"edsr_x{sc}": secondary_edsr(sc, args.batch, dev) for sc in (8, 4, 2)}
        gpu_legs["secondary_edsr"] = time.perf_counter() - t_leg
        # the training state of the headline run is not needed any more: its buffers make room for the legs below
        del ts
        net.engine.bufs.d.clear()
        torch.cuda.empty_cache()
        t_leg = time.perf_counter()
        secondary["swinir_x8_exact_f32"] = secondary_exact_f32(args.batch, dev)
        gpu_legs["secondary_exact_f32"] = time.perf_counter() - t_leg
        t_leg = time.perf_counter()
        secondary["model_plain"] = secondary_model_plain(args.batch)
        secondary["model_plain_patches_per_s"] = secondary["model_plain"]["patches_per_s"]
        gpu_legs["secondary_model_plain"] = time.perf_counter() - t_leg
        t_leg = time.perf_counter()
        secondary["eval_x8"] = secondary_eval_x8(args.batch)
        gpu_legs["secondary_eval_x8"] = time.perf_counter() - t_leg
        t_leg = time.perf_counter()
        torch_base = torch_rocm_baseline(args.batch, dev)
        gpu_legs["torch_rocm_baseline"] = time.perf_counter() - t_leg
    if rank == 0:
        patches = args.batch * world * args.steps
        pps = patches / dt
        gflop, gbyte = WORK[args.workload]
        bx = ops_use_bx3()
        out = {
            "metric": "train patches/sec, SwinIR x8 64->512 1ch" if args.workload == "swinir_x8"
                      else f"train patches/sec, EDSR-baseline x{scale} {512 // scale}->512 1ch",
            "value": pps, "unit": "patches/s", "n_gpus": world, "n_ranks_seen": n_ranks_seen,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps,
            "step_ms": {"median": pct(0.5), "p10": pct(0.1), "p90": pct(0.9), "timer": "HIP events, rank 0"},
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            # what the matrix core computes in: f32 operands as two fp16 planes under power-of-two block exponents, three
            # products, f32 accumulate (f32-grade results: parity gates of tests/); nothing is STORED below f32
            "dtype": "f32 (fp16x2 split-MFMA, f32 accumulate)" if bx and getattr(ops_mod, "F16X2", False) else "f32",
            "data": "synthetic",
            "config": {"workload": f"{desc}, fwd + {args.loss} + bwd + {opt_kind}",
                       "global_batch": args.batch * world, "batch_per_gpu": args.batch,
                       "parallelism": f"dp{world}", "final_loss": loss, "hip_graph": bool(use_graph),
                       # `value` is measured on step_fn: graph replay when hip_graph is true; the same K-step protocol on eager
                       # steps (the methodology of rounds 1-4) beside it
                       "eager_patches_per_s": eager_pps,
                       # SwinIR: the timed steps run each RSTB layer's weight gradients on a side stream; the same eager steps
                       # with every launch in order on one stream -- the mode the roofline's per-launch durations (and the
                       # profiles under profiles/) are taken in
                       "side_stream_weight_gradients": bool(side_default),
                       "eager_in_order_patches_per_s": eager_in_order_pps,
                       "droppath_masks": "per rank" if args.droppath_per_rank else "same on every rank (reference seeding)",
                       "eval_patches_per_s_one_gpu": eval_pps, "eval_amp_patches_per_s_one_gpu": eval_amp_pps,
                       "matmul": (("Linear GEMMs: fp16x2 split MFMA (2 fp16 planes per operand under per-row power-of-two "
                                   "scales, 3 products, f32 accumulate: f32-grade per row), the 180-channel convs (scales per "
                                   "weight channel / halo tile) and the Linear weight gradients (running scale per operand "
                                   "column) likewise; 180-channel conv weight gradients: "
                                   if getattr(ops_mod, "F16X2", False) and args.workload.startswith("swinir") else
                                   ("3x3 convs (64 .. 256 channels, fused PixelShuffle included) and their weight gradients: "
                                    "fp16x2 split MFMA (2 fp16 planes, power-of-two scales per weight channel / halo tile / "
                                    "operand column, 3 products: f32-grade per pixel and per dW row); anything else on the matrix core: "
                                    if getattr(ops_mod, "F16X2_CONV", False) and args.workload.startswith("edsr") else "")) +
                                  "bf16x3 split MFMA: f32 operands split into 3 bf16 parts, 6 products, "
                                  "f32 accumulate (f32-accurate)") if bx else "f32 MFMA"},
            # whole step against both rooflines: algorithmic bytes / flops x 3 (fwd + bwd) x patches/s
            "whole_step": {"hbm_frac": gbyte * 3.0 * pps / world / HBM_PEAK_GBS,
                           "flop_frac": gflop * 3.0 * pps / world / 1000.0 / (BX3_PEAK_TFLOPS if bx else F32_MFMA_PEAK_TFLOPS),
                           "flop_frac_of_f32_mfma_peak": gflop * 3.0 * pps / world / 1000.0 / F32_MFMA_PEAK_TFLOPS,
                           # most matrix work of the step now runs three fp16 products per f32-grade product (fp16 dense / 3)
                           "flop_frac_of_fp16x2_peak": gflop * 3.0 * pps / world / 1000.0 / (2.0 * BX3_PEAK_TFLOPS),
                           "algorithmic_gflop_per_patch_fwd": gflop, "algorithmic_gbyte_per_patch_fwd": gbyte,
                           "per_gpu": True},
        }
        # hbm_frac above prices the UNFUSED-convention bytes of SURVEY 8d; this one the bytes a step moved in the committed PMC passes
        # (profiles/, named in committed_pmc_source: stale after a kernel change until tools/refresh_profiles.sh is run again)
        mb, mb_src = measured_bytes_per_step(args.workload)
        if mb:
            out["whole_step"]["hbm_frac_from_committed_pmc"] = mb * (pps / world / args.batch) / 1e9 / HBM_PEAK_GBS
            out["whole_step"]["committed_pmc_gbyte_per_step"] = mb / 1e9
            out["whole_step"]["committed_pmc_source"] = mb_src
        if secondary:
            out["config"]["secondary"] = secondary
        if roof:
            out["roofline"] = roof
        if torch_base:
            out["torch_rocm_baseline"] = torch_base
        # how much of this run was GPU work (the timed region is a fraction of a second; the CPU baseline is most of the rest)
        out["gpu_seconds_total"] = sum(gpu_legs.values())
        out["gpu_seconds"] = gpu_legs
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args.workload, opt_kind)
        print(json.dumps(out), flush=True)
    if pg is not None:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_workers(args)
    return worker(args)


if __name__ == "__main__":
    sys.exit(main())
