"""What an engine allocates, by name: the runs and the description behind tests/test_gpu_engine_buffers.py and the table in
tests/golden/engine_buffers.json.  Per net of net_protocol_cases.py, at test_gpu_net_protocol.py's input (B = 2, 16 x 16):
a training forward + backward, an evaluation forward and an --amp evaluation forward on ONE engine; for the two nets that
train under --amp (EDSR at 64 features, DRRN) the fp16-storage training forward + backward on a fresh one, at the smallest
patches of tests/test_gpu_amp_train.py (32 x 32) and tests/test_gpu_amp_train_drrn.py (16 x 16 at x2: the smallest maps).
The generator is seeded in front of every forward (NLSN draws hash rotations); the caller turns torch's deterministic
algorithms on (OmniSR / GRL: index_add_)."""
import torch

import net_protocol_cases as C

AMP_TRAIN = {
    "EDSR_LIIF.amp_train": ("network_edsr_liif", "EDSR_LIIF", dict(scale=2, n_resblocks=2, n_feats=64), (2, 32, 32)),
    "DRRN.amp_train": ("network_drrn", "DRRN", dict(in_chans=1, upscale=2, num_residual_units=3), (2, 16, 16)),
}
CASES = list(C.NETS) + list(AMP_TRAIN)


def _seeded(fn, *a, **k):
    torch.manual_seed(11)
    return fn(*a, **k)


def _tensor(t):
    return [list(t.shape), str(t.dtype).replace("torch.", "")]


def _entry(v):
    """a tensor: [shape, dtype]; planes: + (rows, K, fmt); a tape bank's conv: its kind and sizes"""
    from srhip import ops
    from srhip.tape import ConvW
    if isinstance(v, torch.Tensor):
        return _tensor(v)
    if isinstance(v, ops.Bx3):
        return _tensor(v.planes) + [v.rows, v.K, v.fmt]
    assert isinstance(v, ConvW), type(v)
    return [v.kind, v.s, v.k, v.p, v.Co, v.Ci, bool(v.use_planes)]


def _table(holder):
    return [] if holder is None else sorted([str(k)] + _entry(v) for k, v in holder.d.items())


def describe(eng):
    bank = getattr(eng, "bank", None)
    pool = getattr(eng.bufs, "pool", None)
    out = {"bufs": _table(eng.bufs), "derived": _table(getattr(eng, "derived", None)), "ws": _table(getattr(eng, "ws", None)),
           "bank": _table(bank), "bank.bufs": _table(getattr(bank, "bufs", None)), "bank.ws": _table(getattr(bank, "ws", None)),
           "pool": {} if pool is None else {"x".join(map(str, k)): len(v) for k, v in sorted(pool.all.items())}}
    return out


def run(case, keep=None):
    """Run the case's forwards and backwards; returns describe(engine).  keep(tag, tensor): every output and gradient."""
    from srhip import ops
    keep = keep or (lambda tag, t: None)
    gen = torch.Generator().manual_seed(7)
    if case in AMP_TRAIN:
        import importlib
        mod, cls, kw, (B, P, Q) = AMP_TRAIN[case]
        torch.manual_seed(0)
        net = getattr(importlib.import_module(f"dlib.models.{mod}"), cls)(**kw).cuda().train()
        x = torch.rand(B, 1, P, Q, generator=gen).cuda()
        xi = net.prepare_input(x)[0]
        eng = net.engine
        y = _seeded(eng.forward_h16, xi, save=True)
        keep("amp_train.y", y)
        dy = (torch.rand(y.shape, generator=gen) * 64.0).cuda()
        grads = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
        eng.backward_h16(dy, grads, grads_zeroed=True)
        for k, g in grads.items():
            keep("amp_train.grad." + k, g)
        return describe(eng)
    net = C.build(case).cuda().train()
    x = torch.rand(2, 1, 16, 16, generator=gen).cuda()
    xi = net.prepare_input(x)[0]
    eng = net.engine
    y = _seeded(eng.forward, xi, None, save=True)
    keep("train.y", y)
    dy = torch.rand(y.shape, generator=gen).cuda()
    grads = {k: torch.empty_like(p) for k, p in net.named_parameters()}
    dx = eng.backward(dy, grads, need_dx=True) if case in C.INPUT_GRAD else eng.backward(dy, grads)
    for k, p in net.named_parameters():
        if p.requires_grad:
            keep("train.grad." + k, grads[k])
    if dx is not None:
        keep("train.dx", dx)
    net.eval()
    with torch.no_grad():
        keep("eval.y", _seeded(eng.forward, xi, None, save=False))
        with ops.amp_inference(True):
            keep("amp_eval.y", _seeded(eng.forward, xi, None, save=False))
    return describe(eng)
