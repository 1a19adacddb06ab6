"""ACT's dropout without a GPU: the numpy restatement of the library's mask generator (tests/philox_ref.py) against the
known-answer vectors of Philox4x32-10 and its statistical / indexing properties, the constructor, and the wiring of
Tape.dropout into srhip/act_engine.py::_forward_tape with torch stand-ins for the kernels (tests/emul_ops.py + the stand-in
of ops.dropout in philox_ref) against the REFERENCE's autograd under the same masks (tests/golden/g52_act_dropout.npz, written
by tools/make_golden_act_dropout.py).  The same comparison with the real kernels: tests/test_gpu_act_dropout.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import philox_ref as PR  # noqa: E402

CFG = dict(n_feats=16, n_resgroups=4, n_resblocks=2, reduction=4, n_heads=4, n_layers=8, n_fusionblocks=4)


def test_philox_restatement_reproduces_the_known_answer_vectors():
    assert len(PR.KAT) == 3
    for ctr, key, want in PR.KAT:
        got = tuple(int(v) for v in PR.philox4x32_10(*ctr, *key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # the array form is the scalar form element by element
    ctrs = np.array([k[0] for k in PR.KAT[:1] * 3], dtype=np.uint64)
    ctrs[:, 0] = (0, 1, 2)
    arr = PR.philox4x32_10(ctrs[:, 0], ctrs[:, 1], ctrs[:, 2], ctrs[:, 3], 5, 9)
    for i in range(3):
        assert tuple(int(w[i]) for w in arr) == tuple(int(v) for v in PR.philox4x32_10(i, 0, 0, 0, 5, 9))


def test_mask_properties():
    n, p = 1 << 20, 0.25
    sigma = (p * (1 - p) / n) ** 0.5
    for seed in (20260101, 7):
        for site in (0, 1, 27):
            frac = PR.mask(seed, site, 0, n, p).mean()
            assert abs(frac - (1 - p)) <= 4 * sigma, (seed, site, frac, (frac - (1 - p)) / sigma)
    # two sites are independent: both keep with probability 0.75, so they agree on 0.75^2 + 0.25^2 = 0.625
    a, b = PR.mask(20260101, 0, 0, 1 << 16, p), PR.mask(20260101, 1, 0, 1 << 16, p)
    assert abs((a == b).mean() - 0.625) <= 0.01
    # a slice sees the whole tensor's mask
    assert np.array_equal(PR.mask(7, 3, 4096, 1000, p), PR.mask(7, 3, 0, 5096, p)[4096:])
    # the high counter word is in use
    assert not np.array_equal(PR.mask(7, 3, (1 << 34) + 8, 4096, p), PR.mask(7, 3, 8, 4096, p))
    # the ends of the range: p = 0 keeps everything
    assert PR.mask(7, 0, 0, 4096, 0.0).all()
    assert PR.threshold(0.25) == (1 << 30, 1 / 0.75)


def test_act_constructor_accepts_a_dropout_rate():
    from dlib.models.network_act import ACT
    g = np.load(os.path.join(ROOT, "tests", "golden", "g36_act.npz"))
    net = ACT(upscale=2, in_chans=1, dropout_rate=0.25)
    assert net.dropout_rate == 0.25
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys_default"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(k) for k in g["state_dict_shapes_default"]]
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            ACT(upscale=2, in_chans=1, dropout_rate=bad, **CFG)
    small = ACT(upscale=2, in_chans=1, dropout_rate=0.25, **CFG)
    assert sum(isinstance(m, torch.nn.Dropout) and m.p == 0.25 for m in small.modules()) == 7 * 4
    # no seed where dropout is the identity
    assert small.eval().sample_drop_path(2, "cpu") is None
    assert ACT(upscale=2, in_chans=1, **CFG).train().sample_drop_path(2, "cpu") is None
    s = small.train().sample_drop_path(2, "cpu")
    assert s.dtype == torch.int64 and s.shape == (1,) and 0 <= int(s) < 2 ** 62


def test_act_dropout_tape_wiring_against_reference_gradients(monkeypatch):
    """forward and every parameter gradient against g52_act_dropout.npz at the gates of
    tests/test_cpu_tape_logic.py::test_act_tape_wiring_against_reference_gradients (2e-5 forward, 2e-4 gradients)"""
    import emul_ops
    import sr_oracle as O
    from srhip import ops
    from dlib.models.network_act import ACT
    emul_ops.install(monkeypatch)
    sites = []

    def dropout(x, out, seed, site, p, offset=0):
        sites.append(site)
        return PR.dropout_standin(x, out, seed, site, p, offset)
    monkeypatch.setattr(ops, "dropout", dropout, raising=False)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g52_act_dropout.npz"))
    g = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("x2/")}
    net = ACT(upscale=2, in_chans=1, dropout_rate=float(g["p"]), **CFG)
    layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(O.seeded_state_dict(layout, int(g["seed"])), strict=True)
    net.train()
    x, tgt = g["x"], g["tgt"]
    eng = net.engine
    seed = torch.tensor([int(g["drop_seed"])], dtype=torch.int64)
    y = eng.forward(x[:, 0].contiguous(), seed, save=True).clone()     # (a view of a pooled buffer)
    assert sites == list(range(28))                   # forward order: sites 0 .. 27
    assert (y - g["y"]).abs().max().item() <= 2e-5 * g["y"].abs().max().item()
    dy = torch.sign(y - tgt) / y.numel()
    grads = {k: torch.full_like(p, float("nan")) for k, p in net.named_parameters()}
    eng.backward(dy, grads)
    assert sorted(sites[28:]) == list(range(28))      # every site's mask regenerated once by the backward
    n = 0
    for k, got in grads.items():
        if "grad/" + k in g:
            ref = g["grad/" + k]
            e = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
        elif "gslice/" + k in g:
            ref, sums = g["gslice/" + k], g["gsum/" + k]
            e = ((got[:2] - ref).abs().max() / sums[2].float().clamp_min(1e-30)).item()
            assert abs(got.double().sum().item() - sums[0].item()) <= 1e-4 * sums[1].item(), k
            assert abs(got.double().abs().sum().item() - sums[1].item()) <= 1e-4 * sums[1].item(), k
        else:                                   # a parameter the forward does not reach
            assert float(got.abs().max()) == 0.0, k
            continue
        assert e <= 2e-4, (k, e)
        n += 1
    assert n == int(g["n_grads"])
    # evaluation mode (nn.Dropout follows module.training): the same tape graph without a dropout launch, seed or no seed
    del sites[:]
    net.eval()
    y_eval = eng.forward(x[:, 0].contiguous(), seed, save=True).clone()
    assert sites == [] and (y_eval - g["y"]).abs().max().item() > 1e-3 * g["y"].abs().max().item()
    # training mode under no_grad: dropout stays on (the graph without the recording); one seed, one output
    net.train()
    y_ng = eng.forward(x[:, 0].contiguous(), seed, save=False)
    assert sites == list(range(28)) and torch.equal(y_ng, y)
