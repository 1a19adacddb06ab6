"""The resolution-scaled error on the device: srhip_consistency against the float64 statement of tests/consistency_ref.py on the
cases of tests/consistency_cases.py, dlib.metrics.consistency, Predictor.run(consistency=True) and predict.py --consistency True
on the experiment fixture.

Gates.  All 32 q of the two banks and the winner are EQUAL: test_cpu_consistency.py asserts that every bank of every page is
decided by at least 1e-9 against every candidate with other weights, far above the gate of a score.  Scores, alpha, beta and rse:
64 e_ref of the quantity (tests/consistency_cases.py::bound and its reasoning; e_ref is the statement's own rounding against an
np.longdouble chain: score 7.7e-14, alpha 1.6e-14, beta 2.3e-15, rse 4.1e-10).  rsp = sqrt(|score|): |sqrt(x) - sqrt(y)| =
|x - y| / (sqrt(x) + sqrt(y)) <= |x - y| / sqrt(y), so the score's gate over the statement's |rsp|, plus two roundings of the root.
The residual map float32(l - (alpha b + beta)): one float32 spacing of the statement's value (the final rounding may fall either
way) plus 64 e_ref of alpha times max |b| plus 64 e_ref of beta."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import consistency_cases as K  # noqa: E402
import consistency_ref as C  # noqa: E402
import decorr_cases as DK  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "tests", "golden", "eval_exp", "exp")
NAN = float("nan")
EPS = float(np.finfo(np.float64).eps)
GUARD = 16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srhip import ops as _ops
    return _ops


def dev(a):
    """a numpy array on the device with its strides: a view of a padded array stays a view of a padded tensor"""
    base = a
    while base.base is not None:
        base = base.base
    t = torch.from_numpy(np.array(base, order="C")).cuda()
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return t.as_strided(a.shape, tuple(s // a.itemsize for s in a.strides), off)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _ws_doubles(ops, B, h, w, s):
    import ctypes
    n = ctypes.c_long(-1)
    ops.call("srhip_consistency_ws", B, h, w, s, ctypes.addressof(n))
    return n.value


def _call(ops, E, L, s, ws=None, optional=True):
    """the raw call: a NaN workspace of the declared size with a NaN guard behind it, NaN outputs with guards of their own"""
    E, L = (t[:, 0] if t.dim() == 4 else t for t in (E, L))
    B, h, w = L.shape
    need = _ws_doubles(ops, B, h, w, s)
    ws = need if ws is None else ws
    buf = torch.full((max(ws, 1) + GUARD,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((B * 8 + GUARD,), NAN, dtype=torch.float64, device="cuda")
    sc = torch.full((B * 32 + GUARD,), NAN, dtype=torch.float64, device="cuda")
    qs = torch.full((B * 32 + GUARD,), -7, dtype=torch.int32, device="cuda")
    res = torch.full((B * h * w + GUARD,), NAN, dtype=torch.float32, device="cuda")
    table = ops.consistency_weights(s)
    ops.call("srhip_consistency", E.data_ptr(), E.stride(0), E.stride(1), L.data_ptr(), L.stride(0), L.stride(1), B, h, w, s,
             table.data_ptr(), buf.data_ptr(), ws, out.data_ptr(), sc.data_ptr() if optional else None,
             qs.data_ptr() if optional else None, res.data_ptr() if optional else None, ops._st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[max(ws, 1):]).all()), "the guard behind the workspace was written"
    assert bool(torch.isnan(out[B * 8:]).all()) and bool(torch.isnan(sc[B * 32:]).all()) and bool((qs[B * 32:] == -7).all())
    assert bool(torch.isnan(res[B * h * w:]).all())
    if not optional:
        assert bool(torch.isnan(sc).all()) and bool((qs == -7).all()) and bool(torch.isnan(res).all())
    return out[:B * 8].view(B, 8).cpu(), sc[:B * 32].view(B, 32).cpu(), qs[:B * 32].view(B, 32).cpu(), res[:B * h * w].view(B, h, w).cpu()


def _against_statement(tag, got, each, s):
    out, sc, qs, res = got
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(sc).all()) and bool(torch.isfinite(res).all())
    worst = dict.fromkeys(("score", "alpha", "beta", "rsp", "rse", "residual"), 0.0)
    for i, o in enumerate(each):
        sigma, alpha, beta, rsp, rse, q, n, zero = out[i].tolist()
        d = {"score": float(np.abs(sc[i].numpy() - o["scores"]).max()), "alpha": abs(alpha - float(o["alpha"])),
             "beta": abs(beta - float(o["beta"])), "rsp": abs(rsp - float(o["rsp"])), "rse": abs(rse - float(o["rse"]))}
        g_rsp = K.bound("score") / abs(float(o["rsp"])) + 2 * EPS
        want = o["residual"]
        g_res = np.spacing(np.abs(want)).astype(np.float64) + K.bound("alpha") * float(np.abs(o["b"]).max()) + K.bound("beta")
        e_res = np.abs(res[i].numpy().astype(np.float64) - want.astype(np.float64))
        d["residual"] = float(e_res.max())
        print(f"[consistency] {tag}[{i}]: " + " ".join(f"{k} {v:.3e}" for k, v in d.items())
              + f"   (gates: score {K.bound('score'):.1e} alpha {K.bound('alpha'):.1e} beta {K.bound('beta'):.1e} rsp {g_rsp:.1e} rse "
              f"{K.bound('rse'):.1e})   q {int(q)} sigma {sigma:.4f} rsp {rsp:.6f} rse {rse:.3e}; residual off by a float32 spacing at "
              f"{int((e_res > K.bound('alpha') + K.bound('beta')).sum())} of {e_res.size} pixels")
        for k in worst:
            worst[k] = max(worst[k], d[k])
        assert qs[i].tolist() == o["qs"].tolist(), "the q of the 32 slots"
        assert q == float(o["q"]) and sigma == o["sigma"] and n == float(o["n"]) and zero == 0.0
        for k in ("score", "alpha", "beta", "rse"):
            assert d[k] <= K.bound(k), f"{k}: {d[k]:.3e} above {K.bound(k):.3e}"
        assert d["rsp"] <= g_rsp, f"rsp: {d['rsp']:.3e} above {g_rsp:.3e}"
        assert bool((e_res <= g_res).all()), f"residual: {float((e_res - g_res).max()):.3e} above its gate"
    return worst


@pytest.mark.parametrize("name", list(K.CASES))
def test_consistency_against_statement(ops, name):
    """kernel against statement; two calls give the same bits; without the optional pointers the same result; the wrapper is the
    raw call"""
    B, h, w, s = K.CASES[name][:4]
    E, L = (dev(a) for a in K.tensors(name))
    assert E.is_contiguous() == (K.CASES[name][7] is None)
    got = _call(ops, E, L, s)
    worst = _against_statement(name, got, K.expect(name), s)
    print(f"[consistency] {name}: largest differences " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    again = _call(ops, E, L, s)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), "two calls"
    assert torch.equal(bits(_call(ops, E, L, s, optional=False)[0]), bits(got[0])), "without scores, qs and residual: other bits"
    wo, wsc, wqs, wres = ops.consistency(E, L, s, scores=True, residual=True)
    assert wo.shape == (B, 8) and wsc.shape == (B, 32) and wqs.shape == (B, 32) and wres.shape == (B, h, w)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((wo, wsc, wqs, wres), got)), "the wrapper: other bits"
    assert torch.equal(bits(ops.consistency(E, L, s)), bits(got[0]))
    o2, r2 = ops.consistency(E, L, s, residual=True)
    assert torch.equal(bits(o2), bits(got[0])) and torch.equal(bits(r2), bits(got[3]))


def test_a_page_alone_and_in_any_place_of_a_batch(ops):
    """the same bits for a page alone and as page 0, 1 or 2 of a batch of 3"""
    name = "3x21x37_s4"
    E, L = (dev(a) for a in K.tensors(name))
    alone = [_call(ops, E[i:i + 1], L[i:i + 1], 4) for i in range(3)]
    for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        idx = torch.tensor(order, device="cuda")
        batch = _call(ops, E[idx], L[idx], 4)
        for place, i in enumerate(order):
            assert all(torch.equal(bits(b[place:place + 1]), bits(a)) for a, b in zip(alone[i], batch)), (order, place)


def test_views_and_their_copies_give_the_same_bits(ops):
    name = "8x64x64_s8_strided"
    E, L = (dev(a) for a in K.tensors(name))
    assert E.stride() == (576 * 576, 576 * 576, 576, 1) and L.stride() == (72 * 72, 72 * 72, 72, 1)
    a, b = _call(ops, E, L, 8), _call(ops, E.contiguous(), L.contiguous(), 8)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_duplicate_slots_give_identical_bits(ops):
    """the fine bank of a page whose coarse winner is q = 0 holds q = 0 nine times"""
    name = "2x64x64_s8"
    out, sc, qs, _ = _call(ops, *(dev(a) for a in K.tensors(name)), 8)
    assert qs[1, 16:25].tolist() == [0] * 9 and qs[1, 0].item() == 0
    assert len({int(v) for v in bits(sc[1, 16:25])} | {int(bits(sc[1, :1])[0])}) == 1


def test_scaling_the_page_scales_the_fit(ops):
    """L -> float32(2 L + 0.1): the kernel follows the statement of the new page within the gates, q stays, and alpha -> 2 alpha,
    beta -> 2 beta + 0.1 within what one more float32 rounding of L allows (tests/test_cpu_consistency.py derives it: d sqrt(n /
    C_bb) and d + that times |mean(b)|, d a float32 spacing at max |L|)"""
    name = "3x21x37_s4"
    E, L = K.tensors(name)
    L2 = (2.0 * L.astype(np.float64) + 0.1).astype(np.float32)
    each2 = C.consistency(E[:, 0], L2[:, 0], 4)
    assert min(C.margin(each2)) >= K.MIN_MARGIN
    got, got2 = _call(ops, dev(E), dev(L), 4), _call(ops, dev(E), dev(L2), 4)
    _against_statement("2 L + 0.1", got2, each2, 4)
    assert torch.equal(got2[2], got[2]) and torch.equal(got2[0][:, 5], got[0][:, 5]), "q"
    n = 21 * 37
    for i, o in enumerate(K.expect(name)):
        sb, sbb = float(o["sums"][0]), float(o["sums"][1])
        d = float(np.spacing(np.float32(np.abs(L2[i]).max())))
        g_alpha = d * np.sqrt(n / (sbb - sb * sb / n))
        assert abs(got2[0][i, 1].item() - 2 * got[0][i, 1].item()) <= g_alpha + 3 * K.bound("alpha")
        assert abs(got2[0][i, 2].item() - (2 * got[0][i, 2].item() + 0.1)) <= d + g_alpha * abs(sb / n) + 3 * K.bound("beta")
        # rsp is the cosine between the centred b and the centred page; a linear map of L leaves it alone, and the rounding delta
        # turns the centred page by at most asin(eps) <= 2 eps, eps = |delta| / |centred page| <= d sqrt(n / C_ll); the cosine
        # moves by no more than the angle.  Both runs are within the gate of rsp.
        cll2 = float(each2[i]["sums"][4]) - float(each2[i]["sums"][3]) ** 2 / n
        g_rsp = K.bound("score") / abs(float(o["rsp"])) + 2 * EPS
        assert abs(got2[0][i, 3].item() - got[0][i, 3].item()) <= 2 * g_rsp + 2 * d * np.sqrt(n / cll2)


def test_an_invented_structure_shows_in_rsp_and_in_the_map(ops):
    """a blob the acquisition does not hold, added to both outputs of 2x64x64_s8: RSP drops on both pages, and the map changes
    most within two LR pixels of it on both.  On page 1 (best blur half a pixel) the blob is also the largest |residual| of the
    whole map, and negative: the output is brighter there than the acquisition explains.  On page 0 the best blur, 8.75 HR pixels,
    spreads the blob (sigma 3) to 0.035, below the 4-sigma peaks of the planted noise (0.08): there the statement's own map has
    its largest value elsewhere too, and the kernel's largest value is where the statement's is."""
    name = "2x64x64_s8"
    E, L = K.tensors(name)
    Eb = np.stack([K.with_blob(e) for e in E[:, 0]])[:, None]
    plain, blob = _call(ops, dev(E), dev(L), 8), _call(ops, dev(Eb), dev(L), 8)
    cy, cx = K.BLOB[0] / 8.0, K.BLOB[1] / 8.0
    for i in range(2):
        rsp0, rsp1 = plain[0][i, 3].item(), blob[0][i, 3].item()
        delta = (blob[3][i] - plain[3][i]).abs().numpy()
        ky, kx = np.unravel_index(int(delta.argmax()), delta.shape)
        my, mx = np.unravel_index(int(blob[3][i].abs().numpy().argmax()), delta.shape)
        print(f"[consistency] blob page {i}: rsp {rsp0:.6f} -> {rsp1:.6f}; the map changes most at ({ky}, {kx}), its largest |value| "
              f"{blob[3][i, my, mx].item():.4f} is at ({my}, {mx}); the blob is at ({cy:.2f}, {cx:.2f})")
        assert rsp1 < rsp0
        assert abs(ky - cy) <= 2 and abs(kx - cx) <= 2
        want = C.consistency_one(Eb[i, 0], L[i, 0], 8)["residual"]
        assert (my, mx) == np.unravel_index(int(np.abs(want).argmax()), want.shape)
        if i == 1:
            assert abs(my - cy) <= 2 and abs(mx - cx) <= 2 and blob[3][i, my, mx].item() < 0


def test_degenerate_pages(ops):
    """a constant page and an empty output: sigma = alpha = rsp = 0, beta the mean of L, no NaN"""
    E, L = (dev(a) for a in K.tensors("16x16_s2"))
    out, sc, qs, res = _call(ops, E, torch.full_like(L, 0.5), 2)
    assert out.tolist() == [[0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 256.0, 0.0]] and sc.abs().max().item() == 0.0 and res.abs().max().item() == 0.0
    assert qs[0, :16].tolist() == list(range(0, 128, 8)) and qs[0, 16:].tolist() == [0] * 9 + list(range(1, 8))
    out, sc, qs, res = _call(ops, torch.zeros_like(E), L, 2)
    l = K.tensors("16x16_s2")[1][0, 0].astype(np.float64)
    assert out[0, :2].tolist() == [0.0, 0.0] and out[0, 3].item() == 0.0 and out[0, 5:].tolist() == [0.0, 256.0, 0.0]
    assert abs(out[0, 2].item() - l.mean()) <= 256 * EPS and abs(out[0, 4].item() - l.std()) <= 256 * EPS * 16
    assert np.abs(res[0].numpy() - (l - out[0, 2].item()).astype(np.float32)).max() == 0.0


def test_the_entry_point_refuses(ops):
    """what the header says it refuses, with real buffers: nothing is launched and nothing is written"""
    E, L = (dev(a) for a in K.tensors("16x16_s2"))
    need = _ws_doubles(ops, 1, 16, 16, 2)
    assert need == 16 * 5 + 8
    with pytest.raises(ops.SrhipError, match=f"holds {need - 1} doubles, the call needs {need}"):
        _call(ops, E, L, 2, ws=need - 1)
    with pytest.raises(ops.SrhipError, match="2 .. 8"):
        _call(ops, E, L, 9)
    with pytest.raises(ops.SrhipError, match="at least 4"):
        _call(ops, E[:, :, :6], L[:, :, :3], 2)
    table, ws, out = ops.consistency_weights(2), torch.empty(need, dtype=torch.float64, device="cuda"), torch.empty(8, dtype=torch.float64, device="cuda")
    e, l = E[:, 0], L[:, 0]

    def raw(**kw):
        a = dict(E=e.data_ptr(), E_ld=32, L=l.data_ptr(), L_ld=16, table=table.data_ptr(), ws=ws.data_ptr(), out=out.data_ptr(), residual=None)
        a.update(kw)
        ops.call("srhip_consistency", a["E"], 32 * 32, a["E_ld"], a["L"], 16 * 16, a["L_ld"], 1, 16, 16, 2, a["table"], a["ws"], need,
                 a["out"], None, None, a["residual"], ops._st())
    for kw, text in ((dict(E=None), "null pointer"), (dict(out=None), "null pointer"), (dict(table=None), "null pointer"),
                     (dict(E_ld=31), "row stride below the row"), (dict(L_ld=15), "row stride below the row"),
                     (dict(residual=l.data_ptr()), "overlap"), (dict(out=ws.data_ptr()), "overlap"), (dict(ws=table.data_ptr()), "overlap")):
        with pytest.raises(ops.SrhipError, match=text):
            raw(**kw)
    with pytest.raises(ops.SrhipError, match=r"E is \[1, 32, 32\]"):
        ops.consistency(E[:, :, :30], L, 2)
    with pytest.raises(ops.SrhipError, match="contiguous rows"):
        ops.consistency(E[:, :, :, ::2], L[:, :, :8, :8], 2)
    with pytest.raises(ops.SrhipError, match="contiguous rows"):
        ops.consistency(E.double(), L, 2)


def test_metrics_surface(ops):
    from dlib import metrics
    name = "3x21x37_s4"
    E, L = (dev(a) for a in K.tensors(name))
    out, sc, qs, res = _call(ops, E, L, 4)
    d = metrics.consistency(E, L, 4)
    assert list(d) == ["sigma", "alpha", "beta", "rsp", "rse", "q"]
    assert all(d[k].shape == (3,) and d[k].is_cuda for k in d) and d["q"].dtype == torch.int64
    for col, k in enumerate(("sigma", "alpha", "beta", "rsp", "rse")):
        assert d[k].dtype == torch.float64 and torch.equal(bits(d[k]), bits(out[:, col]))
    assert d["q"].tolist() == [o["q"] for o in K.expect(name)]
    full = metrics.consistency(E, L, 4, scores=True, residual=True)
    assert list(full) == ["sigma", "alpha", "beta", "rsp", "rse", "q", "scores", "qs", "residual"]
    assert full["scores"].shape == (3, 32) and full["qs"].shape == (3, 32) and full["qs"].dtype == torch.int32
    assert full["residual"].shape == (3, 21, 37) and full["residual"].dtype == torch.float32
    assert torch.equal(bits(full["scores"]), bits(sc)) and torch.equal(full["qs"].cpu(), qs) and torch.equal(bits(full["residual"]), bits(res))
    assert list(metrics.consistency(E, L, 4, residual=True)) == ["sigma", "alpha", "beta", "rsp", "rse", "q", "residual"]
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.consistency(E.cpu(), L, 4)
    assert "consistency" in metrics.__all__


# ------------------------------------------------------------------ predict.py --consistency True
def _pages():
    """three 8-bit LR pages of 40 x 45, the pages of the decorrelation tests: emitters under a PSF"""
    return np.stack([np.rint(255.0 * DK.dots(40, 45, 40 + i, sigma=1.2)).astype(np.uint8) for i in range(3)])


def _by_hand(ops, pred, pages, in_max):
    """ops.consistency on the tensors the run saw, group by group: the ingested pages without their padding, and the float
    output of the same groups (out_dtype float32) cropped to the page"""
    from srhip.predict import Predictor, consistency_record, padded_size
    H, W = pages.shape[-2:]
    Hp, Wp = padded_size(pred.args, H, W)
    flt = Predictor(EXP, batch=pred.batch, in_max=pred.in_max, out_dtype="float32").run(pages)
    want, maps = [], []
    for g0 in range(0, len(pages), pred.batch):
        grp = pages[g0:g0 + pred.batch]
        lr = ops.ingest_pad(torch.from_numpy(np.ascontiguousarray(grp)).cuda(), in_max, Hp, Wp).view(len(grp), 1, Hp, Wp)[:, :, :H, :W]
        out, res = ops.consistency(torch.from_numpy(flt[g0:g0 + pred.batch]).cuda()[:, None], lr, pred.scale, residual=True)
        want.extend(consistency_record(pred.scale, in_max, r) for r in out.cpu().tolist())
        maps.append(res.cpu().numpy())
    return want, np.concatenate(maps)


@pytest.mark.parametrize("dtype,in_max", (("uint8", 255), ("uint16", 4095)))
def test_predictor_with_consistency(ops, dtype, in_max):
    """run(pages, consistency=True, consistency_maps=True): the pages of a run without the option, bit for bit; the records and
    the maps are ops.consistency by hand; the same with resolution=True switched on as well"""
    from srhip.predict import Predictor
    pages = _pages().astype(dtype) * (1 if dtype == "uint8" else 16)
    pred = Predictor(EXP, batch=2, in_max=None if dtype == "uint8" else in_max)
    plain = pred.run(pages)
    assert pred.last_consistency is None and pred.last_residuals is None
    got = pred.run(pages, consistency=True, consistency_maps=True)
    assert got.dtype == plain.dtype and np.array_equal(got, plain)
    recs, maps = pred.last_consistency, pred.last_residuals
    assert len(recs) == 3 and all(list(r) == ["sigma_px", "sigma_lr", "alpha", "beta", "rsp", "rse", "rse_levels"] for r in recs)
    assert maps.shape == (3, 40, 45) and maps.dtype == np.float32 and np.isfinite(maps).all()
    want, want_maps = _by_hand(ops, pred, pages, in_max)
    assert recs == want and np.array_equal(maps, want_maps)
    for r in recs:
        assert r["sigma_lr"] == r["sigma_px"] / 8 and r["rse_levels"] == r["rse"] * in_max and -1.0 <= r["rsp"] <= 1.0 and r["rse"] >= 0.0
    print(f"[consistency] predictor {dtype}: {recs}")
    assert np.array_equal(pred.run(pages, consistency=True), plain) and pred.last_consistency == recs and pred.last_residuals is None
    both = pred.run(pages, resolution=True, consistency=True, consistency_maps=True)
    res_both = pred.last_resolution
    assert np.array_equal(both, plain) and pred.last_consistency == recs and np.array_equal(pred.last_residuals, maps)
    assert np.array_equal(pred.run(pages, resolution=True), plain) and pred.last_resolution == res_both and pred.last_consistency is None
    assert np.array_equal(pred.run(pages), plain) and pred.last_consistency is None and pred.last_resolution is None


def test_command_line_with_consistency(tmp_path):
    """predict.py --consistency True --consistency_maps True: the output files of a run without the flags, byte for byte, plus
    consistency.yml with what the Predictor reports, one float32 residual TIFF per file and one more log line per file"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from srhip.predict import Predictor
    spec = importlib.util.spec_from_file_location("srhip_predict_cli_con", os.path.join(ROOT, "sr-caco-2_amd", "predict.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    src = tmp_path / "in"
    src.mkdir()
    pages = _pages()
    ims = [Image.fromarray(p) for p in pages[:2]]
    ims[0].save(str(src / "a_stack.tif"), save_all=True, append_images=ims[1:])
    Image.fromarray(pages[2]).save(str(src / "b_single.png"))
    outs = {}
    for name, flags in (("plain", []), ("con", ["--consistency", "True"]), ("maps", ["--consistency", "True", "--consistency_maps", "True"])):
        outs[name] = tmp_path / name
        assert cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(outs[name]), "--batch", "2"] + flags) == 0
    files = ["a_stack_x8.tif", "b_single_x8.png", "log.json", "log.txt"]
    assert sorted(os.listdir(outs["plain"])) == files                  # without the options: exactly what it holds today
    assert sorted(os.listdir(outs["con"])) == sorted(files + ["consistency.yml"])
    assert sorted(os.listdir(outs["maps"])) == sorted(files + ["consistency.yml", "a_stack_x8_residual.tif", "b_single_x8_residual.tif"])
    for f in files[:2]:
        assert open(outs["plain"] / f, "rb").read() == open(outs["con"] / f, "rb").read() == open(outs["maps"] / f, "rb").read(), f
    pred = Predictor(EXP, batch=2)
    pred.run(pages[:2], consistency=True, consistency_maps=True)
    want = {"a_stack.tif": [{"page": k, **r} for k, r in enumerate(pred.last_consistency)]}
    want_maps = {"a_stack_x8_residual.tif": pred.last_residuals}
    pred.run(pages[2:], consistency=True, consistency_maps=True)
    want["b_single.png"] = [{"page": 0, **pred.last_consistency[0]}]
    want_maps["b_single_x8_residual.tif"] = pred.last_residuals
    for name in ("con", "maps"):
        rep = yaml.safe_load(open(outs[name] / "consistency.yml"))
        assert rep == want and list(rep) == ["a_stack.tif", "b_single.png"] and [r["page"] for r in rep["a_stack.tif"]] == [0, 1]
    for f, maps in want_maps.items():
        im = Image.open(outs["maps"] / f)
        assert im.mode == "F" and im.size == (45, 40) and getattr(im, "n_frames", 1) == len(maps)
        for k in range(len(maps)):
            im.seek(k)
            assert np.array_equal(np.asarray(im), maps[k])
    log, log0 = (outs["maps"] / "log.txt").read_text(), (outs["plain"] / "log.txt").read_text()
    assert log.count(": consistency RSP ") == 2 and ": consistency RSP " not in log0
