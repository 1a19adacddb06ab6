"""Super-resolve images that have no HR partner with a trained experiment folder.

``Predictor(exp_path).run(pages)`` takes integer pages [N, H, W] (uint8, or uint16 as a 16-bit microscope file holds them)
and returns the super-resolved pages [N, scale * H, scale * W].  The folder is the one ``eval.py`` reads: ``config_model.yml``
and ``best-models/G-model.pth``.  Per group of at most ``batch`` pages the device sees one upload, one ``srhip_ingest_pad``
(integer -> [0, 1] float32 and, for SwinIR, the flipped-strip padding of ``_forward_with_padding``), the forward --
``ModelPlain.test`` or one of the test modes --, one ``srhip_emit_uint`` (crop, clamp, scale, round, cast, non-finite flag)
and one download.

16-bit pages are read as v / 65535, or v / in_max for e.g. 12-bit data in a 16-bit container: the rule by which main.py reads
16-bit tiles, so a net trained on such a fold sees here what it saw in training; without ``in_max`` the white level that
run recorded in ``config_model.yml`` (--in_max) applies.  A net trained on 8-bit data gets finer grey levels than it has seen:
the reference has no such path, so nothing pins the quality of that combination.

What cannot be done is refused by name before anything runs on the device (``PredictError``): 16-bit pages with SRCNN (its
input is cv2's fixed-point cubic interpolation of a uint8 image) or DSR-Splines (one spline net per grey level 0 .. 255),
pages too small for the padding rule, an ``in_max`` above the pages' range.

``run(pages, resolution=True)`` (predict.py --resolution True) also says what the run produced, with no target to compare with:
image decorrelation analysis (what ``dlib.metrics.decorr`` returns; include/srhip.h: srhip_metrics_decorr_lv) of every ingested LR page, at
the levels ``in_max``, and of the net's output for it, at 255 levels for uint8 pages and 65535 otherwise.  That is two more calls
a group and two small downloads; ``Predictor.last_resolution`` then holds one ``resolution_record`` per page.  The returned pages
are those of a run without the option, bit for bit.  Refused with the option: a page with a side below 32, an ``in_max`` below
255.

``run(pages, consistency=True)`` (predict.py --consistency True) asks the other question of an output without ground truth: is
it still an image of what was acquired?  The resolution-scaled error of NanoJ-SQUIRREL (Culley et al. 2018; what
``dlib.metrics.consistency`` returns; include/srhip.h: srhip_consistency): the float output, blurred, binned by the scale and
rescaled linearly, against the ingested LR page -- one call a group on strided views of the two tensors the run holds anyway,
and one small download.  ``Predictor.last_consistency`` then holds one ``consistency_record`` per page; with
``consistency_maps=True`` ``Predictor.last_residuals`` holds the signed float32 error maps [N, H, W].  The returned pages are
those of a run without the option, bit for bit, and it combines with ``resolution=True``.  Refused with the option: a scale
outside 2 .. 8, a page with a side below 4."""
import os
from os.path import join

import numpy as np

from dlib.utils import constants
from dlib.utils.own_options import in_levels

OUT_DTYPES = ("same", "uint8", "uint16", "float32")
_RANGE = {"uint8": 255, "uint16": 65535}
RESOLUTION_MIN_SIDE = 32        # srhip.ops.FRC_MIN_SIDE, without the library
RESOLUTION_MIN_LEVELS = 255
CONSISTENCY_SCALES = (2, 8)     # srhip.ops.CONSISTENCY_MIN_SCALE / _MAX_SCALE / _MIN_SIDE, without the library
CONSISTENCY_MIN_SIDE = 4


class PredictError(ValueError):
    """a request this path refuses"""


class NonFiniteError(RuntimeError):
    """the net's output for a group of pages holds NaN or +-inf; ``pages`` are the indices of that group's pages"""

    def __init__(self, pages):
        self.pages = list(pages)
        super().__init__(f"non-finite output for pages {self.pages[0]} .. {self.pages[-1]}: nothing is returned for them")


def load_config(exp_path):
    """``config_model.yml`` of an experiment folder as the args object ``define_model`` takes (eval.py)."""
    import yaml
    from dlib.utils.tools import Dict2Obj
    if not (exp_path and os.path.isdir(exp_path)):
        raise PredictError(f"{exp_path}: not an experiment folder")
    with open(join(exp_path, "config_model.yml"), "r") as fy:
        args = Dict2Obj(yaml.safe_load(fy))
    args.distributed = False
    args.outd = args.outd_backup = exp_path
    args.is_train = False
    args.netG["checkpoint_path_netG"] = join(exp_path, "best-models/G-model.pth")
    return args


def padded_size(args, H, W):
    """(Hp, Wp) the net sees for an H x W page: for SwinIR the next multiple of the window, a whole extra window when the size
    already is one (64 -> 72), as ``_forward_with_padding``; the page's own size for every other net."""
    net = args.netG["net_type"]
    if net != constants.SWINIR:
        return H, W
    wsz = int(args.netG[f"{net}_window_size"])
    return (H // wsz + 1) * wsz, (W // wsz + 1) * wsz


def resolution_record(scale, r_in, r_out):
    """one page of ``Predictor.last_resolution`` from {'side', 'cut', 'amp'} of the LR page and of the output:
    {'in': {side, cut, res_px, amp}, 'out': {...}, 'gain'}.  res_px = 2 / cut in that image's own pixels (None: cut is 0, no
    resolution was found); gain = (res_px_in * scale) / res_px_out, both in output pixels (None when either is)."""
    def one(r):
        cut = float(r["cut"])
        return {"side": int(r["side"]), "cut": cut, "res_px": 2.0 / cut if cut > 0 else None, "amp": float(r["amp"])}
    a, b = one(r_in), one(r_out)
    both = a["res_px"] is not None and b["res_px"] is not None
    return {"in": a, "out": b, "gain": (a["res_px"] * scale) / b["res_px"] if both else None}


def consistency_record(scale, in_max, row):
    """one page of ``Predictor.last_consistency`` from its row of srhip_consistency's result (sigma, alpha, beta, rsp, rse, ...):
    {sigma_px, sigma_lr, alpha, beta, rsp, rse, rse_levels}.  sigma_px is the blur in output pixels, sigma_lr = sigma_px / scale
    the same in LR pixels; rse is in units of the white level, rse_levels = rse * in_max in the grey levels of the input file."""
    sigma, alpha, beta, rsp, rse = (float(v) for v in row[:5])
    return {"sigma_px": sigma, "sigma_lr": sigma / scale, "alpha": alpha, "beta": beta, "rsp": rsp, "rse": rse,
            "rse_levels": rse * in_max}


def check_request(args, dtype, H, W, in_max=None, out_dtype="same", resolution=False, consistency=False):
    """Raises PredictError for what this path refuses; returns (in_max, output dtype name).  No device use."""
    name = np.dtype(dtype).name
    if name not in _RANGE:
        raise PredictError(f"pages must be uint8 or uint16 (got {name})")
    if out_dtype not in OUT_DTYPES:
        raise PredictError(f"out_dtype must be one of {OUT_DTYPES} (got {out_dtype!r})")
    net = args.netG["net_type"]
    if name == "uint16" and net == constants.SRCNN:
        raise PredictError("SRCNN takes 8-bit pages only: its input 'l_to_h_img' is cv2's fixed-point cubic interpolation of a "
                           "uint8 image")
    if name == "uint16" and net == constants.DSRSPLINES:
        raise PredictError("DSR-Splines takes 8-bit pages only: it holds one spline net per grey level 0 .. 255")
    if in_max is None and name == "uint16":         # the white level the folder's run trained with (main.py --in_max), if any
        in_max = getattr(args, "in_max", None)
    if in_max is None:
        in_max = _RANGE[name]
    if not in_levels(in_max, 1, _RANGE[name]):
        raise PredictError(f"in_max {in_max} is outside 1 .. {_RANGE[name]}, the range of {name} pages")
    if net == constants.SRCNN and in_max != 255:
        raise PredictError("SRCNN reads the interpolated uint8 image / 255: in_max does not apply to it")
    if H < 1 or W < 1:
        raise PredictError(f"empty page {H} x {W}")
    Hp, Wp = padded_size(args, H, W)
    if Hp - H > H or Wp - W > W:
        raise PredictError(f"a {H} x {W} page is too small: the padding to {Hp} x {Wp} flips a strip of {Hp - H} rows / "
                           f"{Wp - W} columns of the page, more than it has")
    if resolution and min(H, W) < RESOLUTION_MIN_SIDE:
        raise PredictError(f"--resolution True: a {H} x {W} page is too small, the decorrelation analysis needs both sides to be "
                           f"at least {RESOLUTION_MIN_SIDE}")
    if resolution and in_max < RESOLUTION_MIN_LEVELS:
        raise PredictError(f"--resolution True: in_max {in_max} is below {RESOLUTION_MIN_LEVELS}, the smallest white level of "
                           f"the decorrelation analysis")
    if consistency and not CONSISTENCY_SCALES[0] <= int(args.scale) <= CONSISTENCY_SCALES[1]:
        raise PredictError(f"--consistency True: scale {int(args.scale)} is outside {CONSISTENCY_SCALES[0]} .. "
                           f"{CONSISTENCY_SCALES[1]}, the scales of the resolution-scaled error (its largest blur has the "
                           f"radius 64 at scale 8)")
    if consistency and min(H, W) < CONSISTENCY_MIN_SIDE:
        raise PredictError(f"--consistency True: a {H} x {W} page is too small, the resolution-scaled error needs both sides to "
                           f"be at least {CONSISTENCY_MIN_SIDE}")
    return int(in_max), (name if out_dtype == "same" else out_dtype)


class Predictor:
    def __init__(self, exp_path, cudaid=0, test_mode=0, test_refield=32, test_min_size=256, batch=8, in_max=None,
                 out_dtype="same"):
        if out_dtype not in OUT_DTYPES:
            raise PredictError(f"out_dtype must be one of {OUT_DTYPES} (got {out_dtype!r})")
        if in_max is not None and not in_levels(in_max, 1, _RANGE["uint16"]):
            raise PredictError(f"in_max {in_max} is outside 1 .. 65535, the range of uint16 pages")
        if int(test_mode) not in range(5):
            raise PredictError(f"test_mode 0 .. 4 (got {test_mode})")
        if int(batch) < 1:
            raise PredictError(f"batch >= 1 (got {batch})")
        self.args = load_config(exp_path)
        self.scale = int(self.args.scale)
        self.cudaid = int(str(cudaid).split(",")[0])
        self.test_mode, self.test_refield, self.test_min_size = int(test_mode), int(test_refield), int(test_min_size)
        self.batch, self.in_max, self.out_dtype = int(batch), in_max, out_dtype
        self._model = None
        self.last_resolution = None      # run(pages, resolution=True): one resolution_record per page
        self.last_consistency = None     # run(pages, consistency=True): one consistency_record per page
        self.last_residuals = None       # ... consistency_maps=True: float32 [N, H, W], the signed error maps

    @property
    def model(self):
        """the experiment's net, built and loaded on first use exactly as eval.py does"""
        if self._model is None:
            import torch
            from dlib.models.select_model import define_model
            torch.manual_seed(int(self.args.myseed or 0))
            torch.cuda.set_device(self.cudaid)
            model = define_model(self.args)
            model.load()
            model.netG.eval()
            self._model = model
        return self._model

    def out_shape(self, H, W):
        return H * self.scale, W * self.scale

    def run(self, pages, resolution=False, consistency=False, consistency_maps=False):
        """pages: np.ndarray [N, H, W], uint8 or uint16 -> np.ndarray [N, scale H, scale W] of the output dtype, the pages in
        order in groups of at most ``batch``.  A group whose output is not finite raises NonFiniteError.  ``resolution``: the
        same pages, and ``last_resolution`` holds a ``resolution_record`` for every one of them; ``consistency``: the same
        pages, and ``last_consistency`` holds a ``consistency_record`` for every one of them, ``last_residuals`` their error
        maps under ``consistency_maps`` (module docstring)."""
        pages = np.asarray(pages)
        if pages.ndim != 3:
            raise PredictError(f"pages [N, H, W] (got shape {pages.shape})")
        N, H, W = pages.shape
        if consistency_maps and not consistency:
            raise PredictError("consistency_maps=True needs consistency=True: the maps belong to the resolution-scaled error")
        in_max, out_name = check_request(self.args, pages.dtype, H, W, self.in_max, self.out_dtype, resolution, consistency)
        sH, sW = self.out_shape(H, W)
        out = np.empty((N, sH, sW), dtype=out_name)
        self.last_resolution = self.last_consistency = self.last_residuals = None
        records = [] if resolution else None
        cons = {"records": [], "maps": [] if consistency_maps else None} if consistency else None
        for g0 in range(0, N, self.batch):
            out[g0:g0 + self.batch] = self._run_group(pages[g0:g0 + self.batch], g0, in_max, out_name, records, cons)
        self.last_resolution = records
        if consistency:
            self.last_consistency = cons["records"]
            if consistency_maps:
                self.last_residuals = np.concatenate(cons["maps"]) if cons["maps"] else np.empty((0, H, W), np.float32)
        return out

    def _run_group(self, grp, first, in_max, out_name, records=None, cons=None):
        import torch
        from srhip import ops
        model = self.model
        B, H, W = grp.shape
        sH, sW = self.out_shape(H, W)
        Hp, Wp = padded_size(self.args, H, W)
        src = torch.from_numpy(np.ascontiguousarray(grp)).to(model.device)                        # one upload
        data = {"l_im": ops.ingest_pad(src, in_max, Hp, Wp).view(B, 1, Hp, Wp)}
        if self.args.netG["net_type"] == constants.SRCNN:
            from dlib.datasets import lowres
            data["l_to_h_img"] = ops.u8_to_unit(lowres.l_to_h(src, (sH, sW))).view(B, 1, sH, sW)
        if records is not None:                                     # the LR pages as ingested, without the padding
            r_in = ops.metrics_decorr_lv(data["l_im"][:, :, :H, :W].contiguous(), in_max)
        model.feed_data(data, need_H=False)
        if self.test_mode == 0:
            model.test()
        else:
            model.test_tta(self.test_mode, refield=self.test_refield, min_size=self.test_min_size)
        E = model.E.detach().float().contiguous()
        if tuple(E.shape) != (B, 1, Hp * self.scale, Wp * self.scale):
            raise RuntimeError(f"the net returned {tuple(E.shape)} for an input of {(B, 1, Hp, Wp)} at scale {self.scale}")
        if records is not None:                                     # the output before it is rounded to the file's levels
            r_out = ops.metrics_decorr_lv(E[:, :, :sH, :sW].contiguous(), 255 if out_name == "uint8" else 65535)
        if cons is not None:        # the float output as returned against the ingested pages: two strided views, no copy
            c_out = ops.consistency(E[:, :, :sH, :sW], data["l_im"][:, :, :H, :W], self.scale, residual=cons["maps"] is not None)
        if out_name == "float32":
            res = E[:, 0, :sH, :sW].cpu().numpy()
            bad = not np.isfinite(res).all()
        else:
            # the flag and the pages share one buffer, [flag, 12 bytes unused, pages], so that they come back in one download
            bits = 8 if out_name == "uint8" else 16
            buf = torch.empty(16 + B * sH * sW * (bits // 8), dtype=torch.uint8, device=E.device)
            buf[:4].zero_()
            dst = buf[16:].view(torch.uint8 if bits == 8 else torch.uint16).view(B, sH, sW)
            ops.emit_uint(E.view(B, E.shape[-2], E.shape[-1]), bits, sH, sW, flag=buf[:4].view(torch.int32), out=dst)
            host = buf.cpu().numpy()                                                              # one download
            res, bad = host[16:].view(out_name).reshape(B, sH, sW), bool(host[:4].view(np.int32)[0])
        if bad:
            raise NonFiniteError(range(first, first + B))
        if records is not None:
            rows = zip(r_in.cpu().tolist(), r_out.cpu().tolist())       # [B][5] = cut, ring, amp, sigma, side: two downloads
            records.extend(resolution_record(self.scale, *({"cut": r[0], "amp": r[2], "side": r[4]} for r in pair)) for pair in rows)
        if cons is not None:
            rows = (c_out[0] if cons["maps"] is not None else c_out).cpu().tolist()         # [B][8]: one small download
            cons["records"].extend(consistency_record(self.scale, in_max, r) for r in rows)
            if cons["maps"] is not None:
                cons["maps"].append(c_out[1].cpu().numpy())
        return res
