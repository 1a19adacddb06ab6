"""Host logic of the multi-image training losses (srhip/train.py), no GPU: loss_and_grad and multiscale_loss_and_grad go
through ONE term table -- the calls they make into srhip.ops are recorded by a stand-in module -- and the C-ABI entry point
of the target pyramid refuses what it must before any launch."""
import ctypes
import os
import subprocess
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """stands in for srhip.ops inside srhip.train: records (name, args, kwargs) of every call"""
    STENCIL_OPS = ("grad", "laplace", "lv")

    def __init__(self, real_ops):
        self.calls = []
        self.lib = real_ops.lib         # srhip_ssim_loss_ws is a host function

    def resize_bicubic_ac_pyramid(self, src, shapes, out=None, clamp=True):
        self.calls.append(("resize_bicubic_ac_pyramid", (src, [tuple(s) for s in shapes]), {"out": out, "clamp": clamp}))
        res = []
        for s, o in zip(shapes, out):
            if tuple(s) == tuple(src.shape[-2:]):
                assert o is None
                res.append(src)
            else:
                assert tuple(o.shape) == tuple(src.shape[:-2]) + tuple(s)
                res.append(o.copy_(F.interpolate(src, size=tuple(s), mode="bicubic", align_corners=True).clamp(0, 1)))
        return res

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a, k))
        return f


def bare_step(monkeypatch, terms):
    from srhip import ops, train
    rec = Recorder(ops)
    monkeypatch.setattr(train, "ops", rec)
    ts = object.__new__(train.TrainStep)            # the loss layer alone: no network, no device
    ts.loss_terms = list(terms)
    ts.loss_buf = torch.zeros(1 + len(terms))
    ts.fp = types.SimpleNamespace(flat=torch.ones(10))
    ts.dy = None
    return ts, rec


def same(a, b):
    """recorded argument == expected one: tensors by storage address and shape, the rest by value"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr() and a.shape == b.shape
    return type(a) is type(b) and a == b


def assert_calls(got, want):
    assert [c[0] for c in got] == [c[0] for c in want]
    for (n, a, k), (_, wa, wk) in zip(got, want):
        assert len(a) == len(wa) and all(same(x, y) for x, y in zip(a, wa)), (n, a, wa)
        assert sorted(k) == sorted(wk) and all(same(k[key], wk[key]) for key in k), (n, k, wk)


def test_single_image_path_makes_the_calls_it_always_made(monkeypatch):
    """l1 + ssim through loss_and_grad: the two kernel calls of the step before the term table was factored out, argument
    for argument (positional / keyword form included: the stand-in would see a difference)."""
    ts, rec = bare_step(monkeypatch, [("l1", 1.0), ("ssim", 2.0, 11)])
    y, tgt, w = torch.rand(2, 1, 8, 8), torch.rand(2, 1, 8, 8), torch.rand(2, 1, 8, 8)
    dy = ts.loss_and_grad(y, tgt, w)
    lb = ts.loss_buf
    assert dy is ts.dy and dy.shape == y.shape
    assert_calls(rec.calls, [("loss_l1l2", (y, tgt, 0, 1.0, w, dy, lb[1:2]), {"grad_accum": False}),
                             ("ssim_loss", (y, tgt, 11, 2.0, dy, lb[2:3]), {"grad_accum": True})])
    # every other term of the table, single image: the lambda is the term's own, the first term writes
    terms = [("charbonnier", 0.5, 1e-3), ("l2", 3.0), ("l2sum", 0.25), ("norm_lv", 1.5, 2, 5), ("local_moments", 0.7),
             ("w_sparsity", 1e-4)]
    ts, rec = bare_step(monkeypatch, terms)
    dy = ts.loss_and_grad(y, tgt)
    lb = ts.loss_buf
    assert_calls(rec.calls, [
        ("loss_pointwise", (y, tgt, 2, 0.5, 1e-3, None, dy, lb[1:2]), {"grad_accum": False}),
        ("loss_l1l2", (y, tgt, 1, 3.0, None, dy, lb[2:3]), {"grad_accum": True}),
        ("loss_pointwise", (y, tgt, 3, 0.25), {"grad": dy, "loss_out": lb[3:4], "grad_accum": True}),
        ("loss_stencil", (y, tgt, "lv", 1.5, 2, 5, True, dy, lb[4:5]), {"grad_accum": True}),
        ("loss_local_moments", (y, tgt, 0.7, dy, lb[5:6]), {"grad_accum": True}),
        ("l1_sparsity", (ts.fp.flat, 1e-4, None, lb[6:7]), {})])


def test_multiscale_path_calls_the_same_table_per_image_with_lam_over_n(monkeypatch):
    ts, rec = bare_step(monkeypatch, [("l1", 1.0), ("ssim", 5.0, 19)])
    tgt = torch.rand(2, 1, 32, 32)
    outs = [torch.rand(2, 1, 32, 32), torch.rand(2, 1, 8, 8), torch.rand(2, 1, 16, 16)]
    dy, d_inter = ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt)
    ms = ts._ms
    dys, parts, tg, ws = ms["dy"], ms["parts"], ms["tgt"], ms["ssim_ws"]
    assert dy is dys[0] and list(d_inter) == dys[1:] and [d.shape for d in dys] == [o.shape for o in outs]
    assert tg[0] is None and [tuple(t.shape) for t in tg[1:]] == [(2, 1, 8, 8), (2, 1, 16, 16)]
    assert [w.numel() for w in ws] == [rec.lib.srhip_ssim_loss_ws(2, h, h) for h in (32, 8, 16)]
    want = [("resize_bicubic_ac_pyramid", (tgt, [(32, 32), (8, 8), (16, 16)]), {"out": tg, "clamp": True})]
    for j, o in enumerate(outs):
        t = tgt if j == 0 else tg[j]
        want += [("loss_l1l2", (o, t, 0, 1.0 / 3.0, None, dys[j], parts[j, 0:1]), {"grad_accum": False}),
                 ("ssim_loss", (o, t, 19, 5.0 / 3.0, dys[j], parts[j, 1:2]), {"grad_accum": True, "workspace": ws[j]})]
    got = [c if c[0] != "resize_bicubic_ac_pyramid" else (c[0], c[1], c[2]) for c in rec.calls]
    assert got[0][0] == "resize_bicubic_ac_pyramid" and got[0][1][0] is tgt and got[0][1][1] == want[0][1][1]
    assert got[0][2]["out"] is tg and got[0][2]["clamp"] is True
    assert_calls(got[1:], want[1:])
    # steady state: the second call reuses every buffer
    rec.calls.clear()
    ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt)
    assert ts._ms is ms and len(rec.calls) == 7
    # another shape set replaces them
    ts.multiscale_loss_and_grad(outs[0], outs[2:], tgt)
    assert ts._ms is not ms and len(ts._ms["dy"]) == 2


def test_multiscale_sums_the_images_into_the_term_slots(monkeypatch):
    from srhip import ops, train
    rec = Recorder(ops)

    def l1(pred, target, mode, lam, weight, grad, part, grad_accum=False):       # a CPU stand-in with the kernel's contract
        part.copy_((lam * (pred - target).abs().mean()).reshape(1))
        grad.copy_(lam * torch.sign(pred - target) / pred.numel())
    rec.loss_l1l2 = l1
    monkeypatch.setattr(train, "ops", rec)
    ts = object.__new__(train.TrainStep)
    ts.loss_terms, ts.loss_buf, ts.dy = [("l1", 2.0)], torch.zeros(2), None
    tgt = torch.rand(2, 1, 16, 16)
    outs = [torch.rand(2, 1, 16, 16), torch.rand(2, 1, 8, 8)]
    ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt)
    small = F.interpolate(tgt, size=(8, 8), mode="bicubic", align_corners=True).clamp(0, 1)
    want = 2.0 * ((outs[0] - tgt).abs().mean() + (outs[1] - small).abs().mean()) / 2.0
    assert abs(ts.loss_buf[1].item() - want.item()) <= 1e-6


def test_w_sparsity_enters_once_with_its_full_lambda(monkeypatch):
    """The reference adds lam * sum|w| at every image's loss_fn call and divides the sum by n: once, undivided.  As the first
    term it still has to leave every image's gradient buffer zeroed for the terms that accumulate behind it."""
    ts, rec = bare_step(monkeypatch, [("w_sparsity", 1e-4), ("l2", 1.0)])
    tgt = torch.rand(2, 1, 16, 16)
    outs = [torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16)]
    ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt)
    sp = [c for c in rec.calls if c[0] == "l1_sparsity"]
    assert len(sp) == 1
    assert_calls(sp, [("l1_sparsity", (ts.fp.flat, 1e-4, None, ts._ms["parts"][0, 0:1]), {})])
    l2 = [c for c in rec.calls if c[0] == "loss_l1l2"]
    assert len(l2) == 3 and all(c[1][3] == 1.0 / 3.0 and c[2] == {"grad_accum": True} for c in l2)
    assert all(float(d.abs().max()) == 0.0 for d in ts._ms["dy"])      # zeroed (the stand-in kernels wrote nothing)
    # same-size images (SRFBN): no resized target at all
    assert ts._ms["tgt"] == [None, None, None]
    # behind another term it zeroes nothing and still enters once
    ts, rec = bare_step(monkeypatch, [("l1", 1.0), ("w_sparsity", 0.5)])
    ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt)
    assert [c[0] for c in rec.calls].count("l1_sparsity") == 1
    assert [c for c in rec.calls if c[0] == "l1_sparsity"][0][1][1] == 0.5


def test_per_pixel_weights_same_size_images_only(monkeypatch):
    ts, rec = bare_step(monkeypatch, [("l1", 1.0), ("l2", 1.0)])
    tgt, w = torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16)
    outs = [torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16)]
    ts.multiscale_loss_and_grad(outs[0], outs[1:], tgt, w)
    l = [c for c in rec.calls if c[0] == "loss_l1l2"]
    assert [c[1][4] is w for c in l] == [True, False, True, False]      # L1 consumes them, L2 does not
    with pytest.raises(NotImplementedError, match="reference itself fails there on the shape mismatch"):
        ts.multiscale_loss_and_grad(outs[0], [torch.rand(2, 1, 8, 8)], tgt, w)


def test_unknown_term_is_refused_on_both_paths(monkeypatch):
    ts, _ = bare_step(monkeypatch, [("nonsense", 1.0)])
    y = torch.rand(1, 1, 8, 8)
    with pytest.raises(NotImplementedError):
        ts.loss_and_grad(y, y.clone())
    with pytest.raises(NotImplementedError):
        ts.multiscale_loss_and_grad(y, [y.clone()], y.clone())


def test_pyramid_struct_mirrors_the_header_and_refusals_need_no_device(tmp_path):
    from srhip import _lib, ops
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(srhip_pyr_level), offsetof(srhip_pyr_level, Ho), '
                   'offsetof(srhip_pyr_level, Wo));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_ho, o_wo = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert (ctypes.sizeof(ops._PyrLevel), ops._PyrLevel.Ho.offset, ops._PyrLevel.Wo.offset) == (size, o_ho, o_wo)
    assert _lib.parse_header()["srhip_resize_bicubic_ac_pyramid"] == ("i", "piiipiip")
    # argument checks run on the host, in front of the launch
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    lv = (ops._PyrLevel * 2)()

    def refused(n, what):
        rc = _lib.lib.srhip_resize_bicubic_ac_pyramid(base, 1, 8, 8, ctypes.addressof(lv), n, 1, None)
        assert rc != 0 and what in _lib.lib.srhip_last_error().decode(), _lib.lib.srhip_last_error()
    lv[0].dst, lv[0].Ho, lv[0].Wo = base + 4 * 32, 4, 4             # inside the 8 x 8 source
    refused(1, "overlaps the source")
    lv[0].dst = base + 4 * 64
    lv[1].dst, lv[1].Ho, lv[1].Wo = base + 4 * 72, 2, 2             # inside level 0
    refused(2, "levels 0 and 1 overlap")
    lv[1].dst, lv[1].Ho = base + 4 * 80, 0
    refused(2, "level 1 is empty")
    refused(0, "0 levels")
    with pytest.raises(ops.SrhipError, match="CUDA/HIP tensors"):
        ops.resize_bicubic_ac_pyramid(torch.rand(1, 1, 8, 8), [(4, 4)])
