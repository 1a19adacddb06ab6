"""srhip_bn_stats / _apply / _bwd against nn.functional.batch_norm in float64: the one flow that tests/test_gpu_memnet.py
(small shapes, 16 rows per block) and tests/test_gpu_launch_plans.py (shapes past bn_plan's 16 rows per block) both run."""
import torch
import torch.nn.functional as F

# largest error relative to the reference's largest entry
GATE_Y, GATE_RUNNING, GATE_DX, GATE_PARAM = 2e-6, 1e-6, 5e-6, 2e-6
KINK = 1e-4           # about 8e-5 of the elements lose their gradient: 322 of 4 160 000


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def check_batchnorm_vs_float64(shape, C, seed=None):
    """x of shape (*shape, C), channels last (shape = (B, H, W)): training mode with batch statistics, running-statistics
    update, ReLU, gradients of x, gamma, beta with a skip gradient added, the accumulate form, the eval form.  Prints every
    figure before it asserts; returns them."""
    from srhip import ops
    gen = torch.Generator().manual_seed(C + shape[1] if seed is None else seed)
    B, H, W = shape
    x = torch.randn(B, H, W, C, generator=gen) * 1.7 + 0.4
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    rm0, rv0 = 0.1 * torch.randn(C, generator=gen), 1 + 0.3 * torch.rand(C, generator=gen)
    dy, res = torch.randn(B, H, W, C, generator=gen), torch.randn(B, H, W, C, generator=gen)
    # No gradient arrives where the float64 pre-activation lies within KINK of the ReLU's kink: there ANY float32 evaluation
    # may take the other branch (its error is a few 2^-24 of |x - mean| k, below 1e-6 here) and then differs by a whole dy --
    # at 4 M elements torch's own float32 batch_norm does so once ((65000, 64): z = -3.3e-9), which is no property of a kernel.
    with torch.no_grad():
        z = F.batch_norm(x.permute(0, 3, 1, 2).double(), None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
    dy[(z.abs() < KINK).permute(0, 2, 3, 1)] = 0.0
    # float64 reference (NCHW)
    xd = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    yd = F.relu(F.batch_norm(xd, rm, rv, gd, bd, training=True, momentum=0.1, eps=1e-5))
    yd.backward(dy.permute(0, 3, 1, 2).double())
    # device
    xc, dyc, resc = x.cuda(), dy.cuda(), res.cuda()
    rmc, rvc = rm0.cuda(), rv0.cuda()
    coef = torch.empty(4, C, device="cuda")
    ops.bn_stats(xc, gamma.cuda(), beta.cuda(), coef, rmc, rvc, 0.1, 1e-5)
    y = ops.bn_apply(xc, coef, relu=True)
    e = {"y": rel(y.permute(0, 3, 1, 2), yd), "running_mean": rel(rmc, rm), "running_var": rel(rvc, rv)}
    print(f"batchnorm {tuple(shape)} C={C}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] < GATE_Y
    assert e["running_mean"] < GATE_RUNNING and e["running_var"] < GATE_RUNNING
    dx = torch.full_like(xc, float("nan"))
    dg, db = torch.full((C,), 7.0, device="cuda"), torch.full((C,), -3.0, device="cuda")
    ops.bn_bwd(dyc, xc, coef, a=y, dx=dx, res=resc, dgamma=dg, dbeta=db)
    e.update(dx=rel(dx - resc, xd.grad.permute(0, 2, 3, 1)), dgamma=rel(dg, gd.grad), dbeta=rel(db, bd.grad))
    print(f"batchnorm {tuple(shape)} C={C} backward:", {k: f"{e[k]:.2e}" for k in ("dx", "dgamma", "dbeta")})
    assert e["dx"] < GATE_DX
    assert e["dgamma"] < GATE_PARAM and e["dbeta"] < GATE_PARAM
    ops.bn_bwd(dyc, xc, coef, a=y, dgamma=dg, dbeta=db, accumulate=True)      # parameter gradients only, added
    e.update(dgamma_acc=rel(dg, 2 * gd.grad), dbeta_acc=rel(db, 2 * bd.grad))
    assert e["dgamma_acc"] < GATE_PARAM and e["dbeta_acc"] < GATE_PARAM
    # eval form: coefficients from the running statistics, no ReLU
    rstd = torch.rsqrt(rv0 + 1e-5)
    ce = torch.stack([rm0, rstd, gamma * rstd, beta]).cuda()
    ye = ops.bn_apply(xc, ce, relu=False)
    yed = F.batch_norm(x.permute(0, 3, 1, 2).double(), rm0.double(), rv0.double(), gamma.double(), beta.double(),
                       training=False, eps=1e-5)
    e["y_eval"] = rel(ye.permute(0, 3, 1, 2), yed)
    print(f"batchnorm {tuple(shape)} C={C} accumulate / eval:", {k: f"{e[k]:.2e}" for k in ("dgamma_acc", "dbeta_acc", "y_eval")})
    assert e["y_eval"] < GATE_Y
    return e
