"""tests/golden/g52_act_dropout.npz: a training step of the REFERENCE's ACT with dropout_rate = 0.25 under prescribed masks --
the yardstick of Tape.dropout's wiring into srhip/act_engine.py (tests/test_cpu_act_dropout.py, tests/test_gpu_act_dropout.py,
which read nothing but the .npz and tests/philox_ref.py).

Run on the build machine from the repository root (it imports the real reference through oracle/ref_shim.py; the GPU box
has none):  python tools/make_golden_act_dropout.py

The configuration of g45_act_grad.npz (n_feats 16, 4 residual groups of 2 blocks, reduction 4, 4 heads, 8 layers, 4 fusion
blocks; x2; input 2 x 1 x 12 x 15; weights oracle.seeded_state_dict(layout, 502)) in training mode, L1 loss against a random
target.  Every nn.Dropout of the reference gets a forward hook that replaces its output by
    input * mask(DROP_SEED, site, 0, numel, 0.25) * scale,   scale = 1 / 0.75 (rounded to the input's dtype),
tests/philox_ref.py's restatement of the library's generator; `site` counts the modules' calls in the order the forward makes
them (28 per forward).  The layout is g45's (x, tgt, y, loss, seed, grad/<name>, or gslice/<name> = two rows in full + gsum/<name>
= sum / sum of magnitudes / largest magnitude, n_grads) plus drop_seed, p, and the same run in float64 (y64, loss64,
grad64/<name>, gslice64/<name>): the float32 run's distance from it is the tests' measure of float32 noise.  Two economies keep
the archive below 1 MiB with twice g45's content: tensors above FULL (1024) entries are stored as slices (g45: 8192), and the
float64 run's gradients are stored rounded to float32 (2^-24 relative, a fiftieth of the distance they measure)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DROP_SEED = 20260101
P = 0.25
SCALE, HW, WEIGHT_SEED = 2, (12, 15), 502
FULL = 1024
CFG = dict(n_feats=16, n_resgroups=4, n_resblocks=2, reduction=4, n_heads=4, n_layers=8, n_fusionblocks=4)


def run(RefACT, sd, x, tgt, dtype, rate):
    """one training-mode forward + backward of the reference in `dtype`; rate > 0: the masks forced.  -> (y, loss, grads, calls)"""
    import philox_ref
    net = RefACT(upscale=SCALE, in_chans=1, dropout_rate=rate, **CFG)
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).train()
    calls = [0]

    def hook(mod, inp, out):
        site = calls[0]
        calls[0] += 1
        v = inp[0]
        m = torch.from_numpy(philox_ref.mask(DROP_SEED, site, 0, v.numel(), P)).view(v.shape)
        return torch.where(m, v * torch.tensor(1.0 / (1.0 - P), dtype=v.dtype), torch.zeros_like(v))
    if rate > 0:
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                assert m.p == rate
                m.register_forward_hook(hook)
    y = net(x.to(dtype))
    loss = (y - tgt.to(dtype)).abs().mean()
    loss.backward()
    return y.detach(), loss.detach(), {k: p.grad for k, p in net.named_parameters() if p.grad is not None}, calls[0]


def main():
    import ref_shim
    ref_shim.install()
    import sr_oracle as O
    from dlib.models.network_act import ACT as RefACT       # the reference's module

    layout = [(k, tuple(v.shape)) for k, v in RefACT(upscale=SCALE, in_chans=1, **CFG).state_dict().items()]
    sd = O.seeded_state_dict(layout, WEIGHT_SEED)
    torch.manual_seed(505 + SCALE)
    x = torch.rand(2, 1, *HW)
    tgt = torch.rand(2, 1, HW[0] * SCALE, HW[1] * SCALE)

    y, loss, grads, calls = run(RefACT, sd, x, tgt, torch.float32, P)
    y64, loss64, grads64, calls64 = run(RefACT, sd, x, tgt, torch.float64, P)
    y0, _, _, _ = run(RefACT, sd, x, tgt, torch.float32, 0.0)
    assert calls == calls64 == 7 * CFG["n_fusionblocks"], calls
    # a hook that did not fire cannot produce a golden: the forced forward is not the forward without dropout
    diff = (y - y0).abs().max().item()
    assert diff > 1e-3 * y0.abs().max().item(), diff
    assert sorted(grads) == sorted(grads64)

    pre = f"x{SCALE}/"
    out = {pre + "x": x, pre + "tgt": tgt, pre + "y": y, pre + "loss": loss, pre + "seed": np.array(WEIGHT_SEED),
           pre + "drop_seed": np.array(DROP_SEED, dtype=np.int64), pre + "p": np.array(P), pre + "y64": y64, pre + "loss64": loss64}
    worst = 0.0
    for k, g in grads.items():
        g64 = grads64[k]
        worst = max(worst, ((g.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-30)).item())
        if g.numel() <= FULL:
            out[pre + "grad/" + k], out[pre + "grad64/" + k] = g, g64.float()
        else:
            out[pre + "gslice/" + k], out[pre + "gslice64/" + k] = g[:2].clone(), g64[:2].float()
            out[pre + "gsum/" + k] = torch.stack([g.double().sum(), g.double().abs().sum(), g.double().abs().max()])
    out[pre + "n_grads"] = np.array(len(grads))
    path = os.path.join(ROOT, "tests", "golden", "g52_act_dropout.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote {path}: {len(grads)} gradients, {os.path.getsize(path) / 1024:.0f} KiB; max |y - y(no dropout)| = {diff:.3g}; "
          f"largest relative float32 - float64 gradient distance {worst:.3g}")


if __name__ == "__main__":
    main()
