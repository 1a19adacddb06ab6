"""tests/golden/g53_dsr_splines.npz: a forward and an L1 training gradient of the REFERENCE's DsrSplines at four
configurations -- the yardstick of csrc/dsr_splines.hip, srhip/dsr_splines_engine.py and tests/dsr_splines_ref.py
(tests/test_cpu_dsr_splines.py, tests/test_gpu_dsr_splines.py, which read nothing but the .npz and the restatement).

Run on the build machine from the repository root (it imports the real reference through oracle/ref_shim.py; the GPU box
has none):  python tools/make_golden_dsr_splines.py

Cases (key prefix A/ ... D/):
  A  registry default (in_ksz 3, snet_type1, 16 splines, no residuals), x2, input 2 x 1 x 9 x 11
  B  in_ksz 5, snet_type3, 7 splines (uneven bins), both residuals, x4, input 2 x 1 x 5 x 7
  C  in_ksz 15, snet_type8, 3 splines, both residuals, x2, input 1 x 1 x 4 x 5 (the 8 x 10 image: a side = the pad + 1)
  D  in_ksz 3, snet_type1, 256 splines, local residual only, x2, input 2 x 1 x 9 x 11
Weights are not stored: oracle.seeded_state_dict(tests/dsr_splines_ref.layout(...), seed), the seed is.  Stored per case: cfg
(in_ksz, hidden layers, n_splines, local, global, scale), x, x_interp, tgt, y, loss, ids (the expert of every pixel, read
from the reference's masks), seed, in_seed, keys / shapes / ndim (the reference's state_dict layout), grad (float32 run: the
gradients of the whole layout end to end), and the same run in float64 fed with the float32 x_interp: y64, loss64, grad64
(float64: the restatement is compared with it to 1e-12).

Conditions asserted, the seeds advanced until they hold:
  * A - C: every x_interp * 255 that is not clamped lies >= 1e-3 grey levels from the lower edge of every bin of the case
    (another F.interpolate cannot move a pixel to another expert); D is exempt (every integer is an edge there: its GPU
    test feeds the stored x_interp)
  * A - C: some pixels are clamped to exactly 0.0 and some to exactly 1.0.  Not D: a spline that owns one or two pixels has
    a dead output ReLU about every second time, so D's input is confined to a band of half a dozen grey levels -- a 0 -> 1
    transition would hand single pixels to dozens of its 256 splines and the condition on the gradients below could not
    hold for any seed
  * A and D: at least one expert owns no pixel
  * every expert that owns pixels has a non-zero gradient in each of its tensors; the others' are exactly zero
  * the float32 and float64 runs pick the same experts, and their distance is at most a tenth of the tests' gates (forward
    1e-6 absolute; gradients 2e-6 of the tensor's largest entry + 1e-12); printed
  * tests/dsr_splines_ref.py reproduces the float64 run to 1e-12"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {
    "A": dict(in_ksz=3, nh=1, n=16, local=False, glob=False, scale=2, shape=(2, 1, 9, 11)),
    "B": dict(in_ksz=5, nh=3, n=7, local=True, glob=True, scale=4, shape=(2, 1, 5, 7)),
    "C": dict(in_ksz=15, nh=8, n=3, local=True, glob=True, scale=2, shape=(1, 1, 4, 5)),
    "D": dict(in_ksz=3, nh=1, n=256, local=True, glob=False, scale=2, shape=(2, 1, 9, 11)),
}
MARGIN = 1e-3
FWD_GATE, GRAD_GATE = 1e-5, 2e-5
MAX_TRIES = 20000
FIRST = {"A": 425, "B": 19, "C": 217, "D": 12}       # where the search from 0 arrives (minutes); 0 everywhere repeats it


def make_input(name, c, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(c["shape"], generator=g)
    if name == "D":
        return 0.45 + 0.013 * r                      # a band of about half a dozen grey levels
    if name == "A":                                  # a dark field with a bright band: some of the 16 bins between them stay empty
        hi = torch.zeros(c["shape"], dtype=torch.bool)
        hi[..., -3:] = True
        return torch.where(hi, 0.85 + 0.2 * r, -0.05 + 0.3 * r).clamp(0, 1)
    return (r * 1.3 - 0.15).clamp(0, 1)              # overshoots of the bicubic kernel are clamped to 0 and 1


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12)).item()


def run_reference(Ref, c, sd, x, xi32, tgt, dtype):
    net = Ref(upscale=c["scale"], in_planes=1, in_ksz=c["in_ksz"], splinenet_type=f"snet_type{c['nh']}",
              n_splines_per_color=c["n"], use_global_residual=c["glob"], use_local_residual=c["local"])
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).train()
    if dtype == torch.float64:                       # the same run: the float32 interpolated image, not another one
        net._interpolate = lambda _x: xi32.to(dtype)
    y = net(x.to(dtype))
    masks = torch.stack([s.mask for s in net.splines])[:, :, 0]           # [n, B, H, W]
    assert bool((masks.sum(0) == 1).all()), "the masks do not partition the image"
    ids = masks.argmax(0)
    xi = net.x_interp.detach()
    loss = (y - tgt.to(dtype)).abs().mean()
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in net.named_parameters()}
    return y.detach(), loss.detach(), grads, ids, xi


def quick_checks(name, c, xi, R):
    """the conditions on the image alone"""
    ids = R.expert_ids(xi.numpy(), c["n"])
    if name != "D":
        if not (bool((xi == 0).any()) and bool((xi == 1).any())):
            return None
        v = xi.double().numpy() * 255.0
        edges = np.array([s[0] for s in np.array_split(np.arange(256), c["n"])][1:], dtype=np.float64)
        free = (xi.numpy() > 0) & (xi.numpy() < 1)
        if edges.size and np.abs(v[free][:, None] - edges[None]).min() < MARGIN:
            return None
    if name in ("A", "D") and np.unique(ids).size == c["n"]:
        return None
    return ids


def main():
    import ref_shim
    ref_shim.install()
    import sr_oracle as O
    import dsr_splines_ref as R
    from dlib.models.network_dsr_splines import DsrSplines as Ref       # the reference's module

    out = {}
    for ci, (name, c) in enumerate(CASES.items()):
        hidden = R.HIDDEN[f"snet_type{c['nh']}"]
        lay = R.layout(c["in_ksz"], hidden, c["n"], c["local"])
        ref_lay = [(k, tuple(v.shape)) for k, v in Ref(upscale=c["scale"], in_planes=1, in_ksz=c["in_ksz"],
                                                        splinenet_type=f"snet_type{c['nh']}", n_splines_per_color=c["n"],
                                                        use_global_residual=c["glob"],
                                                        use_local_residual=c["local"]).state_dict().items()]
        assert lay == ref_lay, f"{name}: the restatement's layout is not the reference's state_dict"
        T = len(lay) // c["n"]
        for t in range(FIRST[name], MAX_TRIES):
            in_seed, seed = 5300 + 100000 * ci + t, 530 + 100000 * ci + t
            x = make_input(name, c, in_seed)
            xi = R.interpolate(x, c["scale"])
            ids = quick_checks(name, c, xi, R)
            if ids is None:
                continue
            sd = O.seeded_state_dict(lay, seed)
            tgt = torch.rand(xi.shape, generator=torch.Generator().manual_seed(in_seed + 7))
            y32, _, g32 = R.loss_and_grads(sd, xi, ids[:, 0], tgt, hidden, c["in_ksz"], c["local"], c["glob"], torch.float32)
            y64, _, g64 = R.loss_and_grads(sd, xi, ids[:, 0], tgt, hidden, c["in_ksz"], c["local"], c["glob"], torch.float64)
            owners = set(np.unique(ids).tolist())
            if any(float(g64[k].abs().max()) == 0 for k, _ in lay if int(k.split(".")[1]) in owners):
                continue
            if (y32.double() - y64).abs().max().item() > FWD_GATE / 10 or max(rel(g32[k], g64[k]) for k in g64) > GRAD_GATE / 10:
                continue
            # the candidate passes on the restatement: now the reference itself
            y, loss, grads, rid, rxi = run_reference(Ref, c, sd, x, xi[:, :1], tgt, torch.float32)
            ry64, loss64, grads64, rid64, _ = run_reference(Ref, c, sd, x, xi, tgt, torch.float64)
            assert torch.equal(rxi, xi), "the reference's interpolated image is not the restatement's"
            if not (np.array_equal(rid.numpy(), ids[:, 0]) and torch.equal(rid, rid64)):
                continue                              # a pixel on a bin edge: the float64 product picks another expert
            dy = (y.double() - ry64).abs().max().item()
            dg = max(rel(grads[k], grads64[k]) for k in grads)
            if dy > FWD_GATE / 10 or dg > GRAD_GATE / 10:
                continue
            for k, _ in lay:
                own = int(k.split(".")[1]) in owners
                assert (float(grads[k].abs().max()) > 0) == own and (float(grads64[k].abs().max()) > 0) == own, k
            r64 = max(rel(g64[k], grads64[k]) for k in g64)
            assert r64 < 1e-12 and rel(y64, ry64) < 1e-12, (r64, rel(y64, ry64))
            break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_TRIES} tries satisfies the conditions")
        pre = name + "/"
        out.update({pre + "cfg": np.array([c["in_ksz"], c["nh"], c["n"], int(c["local"]), int(c["glob"]), c["scale"]]),
                    pre + "x": x, pre + "x_interp": xi, pre + "tgt": tgt, pre + "y": y, pre + "loss": loss,
                    pre + "ids": rid.to(torch.uint8), pre + "seed": np.array(seed), pre + "in_seed": np.array(in_seed),
                    pre + "y64": ry64, pre + "loss64": loss64})
        # one entry per tensor would cost D's 2048 tensors more in zip headers than in data: the names and shapes once, the
        # gradients of the whole layout end to end
        out[pre + "keys"] = np.array([k for k, _ in lay])
        out[pre + "shapes"] = np.array([list(s) + [1] * (4 - len(s)) for _, s in lay], dtype=np.int32)
        out[pre + "ndim"] = np.array([len(s) for _, s in lay], dtype=np.int8)
        out[pre + "grad"] = torch.cat([grads[k].reshape(-1) for k, _ in lay])
        out[pre + "grad64"] = torch.cat([grads64[k].reshape(-1) for k, _ in lay])
        nclamp = int((xi == 0).sum()), int((xi == 1).sum())
        print(f"{name}: try {t}, seed {seed}; {len(owners)} of {c['n']} experts own pixels ({T} tensors each); clamped to 0 / 1: "
              f"{nclamp}; reference float32 - float64: forward {dy:.3g} (gate {FWD_GATE:g}), gradients {dg:.3g} of the "
              f"tensor's largest entry (gate {GRAD_GATE:g}); restatement - reference in float64 {r64:.3g}", flush=True)
    path = os.path.join(ROOT, "tests", "golden", "g53_dsr_splines.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
