#!/usr/bin/env python3
"""Super-resolve low-resolution images that have no HR partner with a trained experiment folder:

    python predict.py --exp_path <folder> --input <file | directory> [--output <directory>]
                      [--cudaid 0] [--batch 8] [--in_max N] [--out_dtype same|uint8|uint16|float32]
                      [--test_mode {0..4} [--test_refield 32] [--test_min_size 256]] [--resolution True]
                      [--consistency True [--consistency_maps True]]

<folder> is the experiment directory ``eval.py`` reads (``config_model.yml``, ``best-models/G-model.pth``).  Inputs are
single-channel ``.tif`` / ``.tiff`` / ``.png`` files of PIL mode ``L`` or ``I;16`` (a grey palette counts as ``L``); every
page of a multi-page TIFF is an image.  16-bit pages are divided by 65535, or by ``--in_max`` (4095 for 12-bit data in a
16-bit container; values above it saturate): the net was trained on 8-bit data and sees finer grey levels, nothing in the
reference pins the quality of that.  Files are taken in the order of their names; consecutive pages of equal (dtype, H, W)
go through the net together, at most ``--batch`` at a time (srhip/predict.py: Predictor).  Each input file gives one output
file ``<stem>_x<scale><ext>`` under ``--output`` (default ``<folder>/predict/<basename of the input>/``): same container,
page count and page order; ``--out_dtype float32`` is written as TIFF mode ``F``.  One log line per file (``log.txt`` /
``log.json`` in the output directory).  A file whose pages gave a non-finite output is not written and is named in the
log; the run goes on with the next file and exits with status 1.

``--resolution True`` (default off) also measures what the net bought: image decorrelation analysis (Descloux et al. 2019;
include/srhip.h: srhip_metrics_decorr_lv), a resolution figure from one image with no target, of every LR page and of its
output.  ``<output>/resolution.yml`` then holds ``{file: [{page, in: {side, cut, res_px, amp}, out: {...}, gain}]}``: ``cut`` a
fraction of Nyquist, ``res_px = 2 / cut`` in that image's own pixels (null: none found), ``gain = res_px_in * scale /
res_px_out``; one more log line per file carries the means.  The output files are those of a run without the option.  Every
page needs both sides to be at least 32.

``--consistency True`` (default off) checks every output against the LR page it was made from: the resolution-scaled error of
NanoJ-SQUIRREL (Culley et al. 2018; include/srhip.h: srhip_consistency).  The float output is blurred, binned by the scale and
rescaled linearly so that it explains the LR page best; ``<output>/consistency.yml`` then holds ``{file: [{page, sigma_px,
sigma_lr, alpha, beta, rsp, rse, rse_levels}]}``: the blur in output and in LR pixels, the intensity rescaling, the Pearson
coefficient RSP, the RMS residual RSE in units of the white level and in the file's grey levels; one more log line per file
carries the mean RSP and RSE.  ``--consistency_maps True`` (only with ``--consistency True``) also writes
``<stem>_x<scale>_residual.tif``: float32 (TIFF mode ``F``), one page per input page at the LR size, LR page minus rescaled
degraded output, positive where the acquisition is brighter than the output explains.  Scales 2 .. 8, both sides of a page at
least 4.  A file that was not written gets no record and no map."""
import argparse
import os
import sys
import time
from os.path import join, dirname, abspath, basename, splitext, isdir, isfile, normpath

HERE = dirname(abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import dlib.dllogger as DLLogger  # noqa: E402
from dlib.utils.own_options import str2bool  # noqa: E402
from srhip.predict import Predictor, PredictError, NonFiniteError, OUT_DTYPES, check_request  # noqa: E402

EXTS = (".tif", ".tiff", ".png")


def _grey_palette(im):
    """the grey level of every palette index, or None when an entry is not grey"""
    pal = im.getpalette()
    if pal is None or im.palette.mode != "RGB":
        return None
    pal = np.asarray(pal, dtype=np.uint8).reshape(-1, 3)
    if not (np.array_equal(pal[:, 0], pal[:, 1]) and np.array_equal(pal[:, 0], pal[:, 2])):
        return None
    lut = np.zeros(256, dtype=np.uint8)
    lut[:len(pal)] = pal[:, 0]
    return lut


def _page_dtype(im, path, k):
    if im.mode == "L" or (im.mode == "P" and _grey_palette(im) is not None):
        return "uint8"
    if im.mode == "I;16":
        return "uint16"
    raise PredictError(f"{path}: page {k} has mode {im.mode!r}; single-channel 8-bit ('L') or 16-bit ('I;16') images only")


def _page(im, path, k):
    name = _page_dtype(im, path, k)
    if im.mode == "P":
        return _grey_palette(im)[np.array(im, dtype=np.uint8)]
    return np.array(im).astype(name, copy=False)


def _pages_of(path, fn):
    from PIL import Image
    with Image.open(path) as im:
        out = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            out.append(fn(im, path, k))
    return out


def read_pages(path):
    """every page of a TIFF / PNG file as a uint8 or uint16 array [H, W] (PIL); a mode that is neither raises PredictError
    naming the file and the mode"""
    return _pages_of(path, _page)


def read_meta(path):
    """[(dtype name, H, W)] of a file's pages, from the headers; raises as read_pages does"""
    return _pages_of(path, lambda im, p, k: (_page_dtype(im, p, k), im.size[1], im.size[0]))


def list_inputs(inp):
    if isfile(inp):
        return [inp]
    if not isdir(inp):
        raise PredictError(f"{inp}: no such file or directory")
    return [join(inp, f) for f in os.listdir(inp) if f.lower().endswith(EXTS) and isfile(join(inp, f))]


def plan(files, batch, scale, out_dir, out_dtype="same"):
    """files: [(path, [(dtype name, H, W) per page])] in any order.  A pure function; returns

        order    the paths sorted by file name,
        groups   [[(file index in ``order``, page index)]]: the pages in that order, consecutive pages of equal
                 (dtype, H, W) together, at most ``batch`` in a group,
        outputs  per file of ``order``: its output path ``<out_dir>/<stem>_x<scale><ext>`` -- the input's container, TIFF for
                 float32 pages, which PNG cannot hold."""
    files = sorted(files, key=lambda f: (basename(f[0]), f[0]))
    groups, key = [], None
    for fi, (_, metas) in enumerate(files):
        for pi, meta in enumerate(metas):
            if tuple(meta) != key or len(groups[-1]) >= batch:
                groups.append([])
                key = tuple(meta)
            groups[-1].append((fi, pi))
    outputs = []
    for path, _ in files:
        stem, ext = splitext(basename(path))
        if out_dtype == "float32" and ext.lower() == ".png":
            ext = ".tif"
        outputs.append(join(out_dir, f"{stem}_x{scale}{ext}"))
    if len(set(outputs)) != len(outputs):
        raise PredictError("two input files would be written to the same output file")
    return {"order": [f[0] for f in files], "groups": groups, "outputs": outputs}


def write_pages(path, pages):
    """uint8 -> mode L, uint16 -> I;16, float32 -> F (TIFF); several pages: a multi-page TIFF in the given order"""
    from PIL import Image
    ims = [Image.fromarray(np.ascontiguousarray(p)) for p in pages]
    if len(ims) > 1:
        ims[0].save(path, save_all=True, append_images=ims[1:])
    else:
        ims[0].save(path)


def resolution_rows(records):
    """{page index: resolution_record} of one file -> its list in resolution.yml, [{page, in, out, gain}] in page order"""
    return [{"page": k, **records[k]} for k in sorted(records)]


def resolution_means(rows):
    """(mean res_px of the inputs, of the outputs, mean gain) over the pages that have one; None where no page has"""
    def mean(vals):
        vals = [v for v in vals if v is not None]
        return sum(vals) / len(vals) if vals else None
    return mean(r["in"]["res_px"] for r in rows), mean(r["out"]["res_px"] for r in rows), mean(r["gain"] for r in rows)


def resolution_line(name, rows):
    """the log line of one file under --resolution True"""
    def px(v):
        return "none found" if v is None else f"{v:.2f} px"
    m_in, m_out, gain = resolution_means(rows)
    return (f"{name}: resolution {px(m_in)} in -> {px(m_out)} out [MEAN of 2 / cut over {len(rows)} page(s), own pixels]"
            + ("" if gain is None else f", gain x{gain:.2f}"))


def write_resolution(out_dir, report):
    import yaml
    with open(join(out_dir, "resolution.yml"), "w") as f:
        yaml.safe_dump(report, f, sort_keys=False)


def consistency_rows(records):
    """{page index: consistency_record} of one file -> its list in consistency.yml, [{page, sigma_px, ...}] in page order"""
    return [{"page": k, **records[k]} for k in sorted(records)]


def consistency_means(rows):
    """(mean RSP, mean RSE, mean RSE in grey levels) over the pages of a file"""
    return tuple(sum(r[k] for r in rows) / len(rows) for k in ("rsp", "rse", "rse_levels"))


def consistency_line(name, rows):
    """the log line of one file under --consistency True"""
    rsp, rse, lv = consistency_means(rows)
    return (f"{name}: consistency RSP {rsp:.4f}, RSE {rse:.5f} of the white level = {lv:.2f} grey level(s) "
            f"[MEAN over {len(rows)} page(s), against the LR page]")


def write_consistency(out_dir, report):
    import yaml
    with open(join(out_dir, "consistency.yml"), "w") as f:
        yaml.safe_dump(report, f, sort_keys=False)


def residual_path(output):
    """<stem>_x<scale><ext> -> <stem>_x<scale>_residual.tif beside it"""
    return splitext(output)[0] + "_residual.tif"


def predict(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--exp_path", type=str, required=True)
    ap.add_argument("--input", type=str, required=True, help="a .tif / .tiff / .png file, or a directory of them")
    ap.add_argument("--output", type=str, default=None, help="default: <exp_path>/predict/<basename of the input>/")
    ap.add_argument("--cudaid", type=str, default="0")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--in_max", type=int, default=None, help="the input's white level (default 255 / 65535)")
    ap.add_argument("--out_dtype", type=str, default="same", choices=OUT_DTYPES)
    ap.add_argument("--test_mode", type=int, default=0, choices=range(5),
                    help="0 plain (default), 1 pad, 2 split, 3 x8 self-ensemble, 4 split and x8")
    ap.add_argument("--test_refield", type=int, default=32)
    ap.add_argument("--test_min_size", type=int, default=256)
    ap.add_argument("--resolution", type=str2bool, default=False,
                    help="also write resolution.yml: the decorrelation-analysis resolution of every LR page and of its output")
    ap.add_argument("--consistency", type=str2bool, default=False,
                    help="also write consistency.yml: the resolution-scaled error (RSP, RSE) of every output against its LR page")
    ap.add_argument("--consistency_maps", type=str2bool, default=False,
                    help="with --consistency True: also write <stem>_x<scale>_residual.tif, the signed float32 error maps")
    ns = ap.parse_args(argv)
    if ns.consistency_maps and not ns.consistency:
        raise PredictError("--consistency_maps True needs --consistency True: the maps belong to the resolution-scaled error")
    pred = Predictor(ns.exp_path, cudaid=ns.cudaid, test_mode=ns.test_mode, test_refield=ns.test_refield,
                     test_min_size=ns.test_min_size, batch=ns.batch, in_max=ns.in_max, out_dtype=ns.out_dtype)
    out_dir = ns.output or join(ns.exp_path, "predict", basename(normpath(ns.input)))
    files = [(f, read_meta(f)) for f in list_inputs(ns.input)]
    if not files:
        raise PredictError(f"{ns.input}: no .tif / .tiff / .png file")
    p = plan(files, pred.batch, pred.scale, out_dir, ns.out_dtype)
    metas = dict(files)
    for grp in p["groups"]:                                # every refusal before anything runs on the device
        fi, pi = grp[0]
        try:
            check_request(pred.args, *metas[p["order"][fi]][pi], in_max=ns.in_max, out_dtype=ns.out_dtype, resolution=ns.resolution,
                          consistency=ns.consistency)
        except PredictError as e:
            raise PredictError(f"{basename(p['order'][fi])}, page {pi}: {e}") if ns.resolution or ns.consistency else e
    os.makedirs(out_dir, exist_ok=True)
    DLLogger.init_arb(log_dir=out_dir, is_master=True, reset=True)
    DLLogger.log(f"predict: {len(files)} file(s), {sum(len(g) for g in p['groups'])} page(s) in {len(p['groups'])} group(s) "
                 f"-> {out_dir} (x{pred.scale}, test mode {pred.test_mode})")

    n_pages = [len(metas[f]) for f in p["order"]]
    last_group = {fi: gi for gi, grp in enumerate(p["groups"]) for fi, _ in grp}
    cache, results, ms, failed = {}, {}, {}, set()
    res_pages, report = {}, {}
    con_pages, con_maps, con_report = {}, {}, {}
    extra = {k: True for k in ("resolution", "consistency", "consistency_maps") if getattr(ns, k)}
    for gi, grp in enumerate(p["groups"]):
        for fi in {fi for fi, _ in grp}:
            if fi not in cache:
                cache[fi] = read_pages(p["order"][fi])
        stack = np.stack([cache[fi][pi] for fi, pi in grp])
        t0 = time.perf_counter()
        try:
            res = pred.run(stack, **extra)
        except NonFiniteError:
            res = None
            failed.update(fi for fi, _ in grp)
        dt_ms = (time.perf_counter() - t0) * 1e3
        for k, (fi, pi) in enumerate(grp):
            ms[fi] = ms.get(fi, 0.0) + dt_ms / len(grp)
            if res is not None:
                results.setdefault(fi, {})[pi] = res[k]
                if ns.resolution:
                    res_pages.setdefault(fi, {})[pi] = pred.last_resolution[k]
                if ns.consistency:
                    con_pages.setdefault(fi, {})[pi] = pred.last_consistency[k]
                if ns.consistency_maps:
                    con_maps.setdefault(fi, {})[pi] = pred.last_residuals[k]
        for fi in sorted({fi for fi, _ in grp}):
            if last_group[fi] != gi:
                continue
            name, (dt_name, H, W) = basename(p["order"][fi]), metas[p["order"][fi]][0]
            what = f"{name}: {H} x {W} {dt_name}, {n_pages[fi]} page(s), {ms[fi]:.1f} ms"
            if fi in failed:
                DLLogger.log(f"{what}: NOT WRITTEN, the output of its pages is not finite (NaN or inf)")
            else:
                write_pages(p["outputs"][fi], [results[fi][k] for k in range(n_pages[fi])])
                DLLogger.log(f"{what} -> {basename(p['outputs'][fi])}")
                if ns.resolution:
                    report[name] = resolution_rows(res_pages.pop(fi))
                    DLLogger.log(resolution_line(name, report[name]))
                if ns.consistency:
                    con_report[name] = consistency_rows(con_pages[fi])
                    DLLogger.log(consistency_line(name, con_report[name]))
                if ns.consistency_maps:
                    write_pages(residual_path(p["outputs"][fi]), [con_maps[fi][k] for k in range(n_pages[fi])])
            cache.pop(fi, None)
            results.pop(fi, None)
            con_pages.pop(fi, None)
            con_maps.pop(fi, None)
    if ns.resolution:
        write_resolution(out_dir, report)
    if ns.consistency:
        write_consistency(out_dir, con_report)
    if failed:
        DLLogger.log(f"predict: {len(failed)} of {len(files)} file(s) not written")
    return 1 if failed else 0


if __name__ == "__main__":
    try:
        sys.exit(predict())
    except PredictError as e:
        sys.exit(f"predict.py: {e}")
