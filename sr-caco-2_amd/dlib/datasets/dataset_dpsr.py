"""Training-crop sampling of the reference's dataset (dlib/datasets/dataset_dpsr.py:293-507):
where in a high-resolution tile the next training patch is cut.

``PatchSampler`` keeps the reference's constructor and call protocol -- ``sampler(img_u8_hxw,
return_roi) -> (row0, col0, roi_uint8 | None)`` -- for the sampling styles that need nothing but
numpy: 'uniform' (Python's ``random.randint``, :319-328) and 'roi' with a fixed threshold (:330-369:
one ``np.random.multinomial`` draw from probabilities proportional to ``exp(5 * roi) + 1`` over the
(H-P) x (W-P) candidate origins), 'edt' / 'edt*roi' (:371-457: scipy's Euclidean distance transform of the ROI, as
the reference) and both threshold styles ('fix_threshold'; 'automatic_threshold' = Otsu, restated from skimage's
published algorithm in dlib/datasets/lowres.py since skimage is not in this image).  With the same ``random`` /
``np.random`` seeds it returns the reference's origins (golden g21, g32).

``DeviceRoiSampler`` is the MI355X form of the 'roi' style: the tiles stay resident in HBM as
uint8, one launch draws the origins of a whole batch from device-side uniforms by the inverse CDF of
the SAME probabilities (srhip_roi_sample), and they go straight into srhip_patch_gather -- no
host round trip per sample, so 8 GPUs x 8 patches per step are not host-bound.

``DeviceWeightedSampler`` is the same for 'edt', 'edt*roi' and every style under 'automatic_threshold' (a threshold per
tile): what depends only on the tile -- Otsu's threshold from a device histogram, the exact squared distance transform
(srhip_edt_sq), the fp64 row prefix of the weights ``origin_weights`` states -- is computed once at construction, and a batch
is one srhip_origin_sample launch."""
import math
import os
import random

import numpy as np

SAMPLE_UNIF, SAMPLE_ROI, SAMPLE_EDT, SAMPLE_EDTXROI = 'uniform', 'roi', 'edt', 'edt*roi'
SAMPLE_PATCHES = [SAMPLE_UNIF, SAMPLE_ROI, SAMPLE_EDT, SAMPLE_EDTXROI]
TH_AUTO, TH_FIX = 'automatic_threshold', 'fix_threshold'
ROI_STYLE_TH = [TH_AUTO, TH_FIX]


def roi_probabilities(img: np.ndarray, threshold: float, psize: int) -> np.ndarray:
    """Probability of every candidate origin, (H-P) x (W-P), as the reference builds it (:343-347)."""
    h, w = img.shape
    lo, hi = int(psize / 2), math.ceil(psize / 2)
    roi = (img >= threshold).astype(np.float64)[lo:h - hi, lo:w - hi]
    wgt = np.exp(roi * 5.)
    return ((wgt.flatten() + 1.) / (wgt + 1.).sum()).reshape(roi.shape)


def origin_weights(d2: np.ndarray, roi: np.ndarray, style: str) -> np.ndarray:
    """Unnormalised fp64 weight of candidate origins, proportional to the reference's probabilities (:343-347,389-392,
    431-439; its normalisers cancel): ``d2`` the SQUARED Euclidean distance to the nearest pixel outside the ROI and ``roi``
    the ROI bit, both at the pixel the candidate looks at (row0 + P // 2, col0 + P // 2).  The formula srhip_origin_rowcum /
    srhip_origin_sample evaluate on the device."""
    assert style in (SAMPLE_ROI, SAMPLE_EDT, SAMPLE_EDTXROI), style
    w_roi = np.exp(5. * np.asarray(roi, dtype=np.float64)) + 1.
    if style == SAMPLE_ROI:
        return w_roi
    d = np.sqrt(np.asarray(d2, dtype=np.float64))
    if style == SAMPLE_EDT:
        return d + 1.
    with np.errstate(over='ignore'):
        return w_roi * (np.exp(d) + 1.)


def check_origin_total(total: float, tile, style: str) -> float:
    """The total weight of a tile must be finite: where exp(distance) overflows (distance above ~709) the reference's
    probabilities are NaN and its np.random.multinomial raises; so does the construction of the device sampler."""
    total = float(total)
    if not math.isfinite(total) or total <= 0.:
        raise ValueError(f"sample_tr_patch={style}: tile {tile}: the total origin weight is {total} (exp of the distance "
                         f"transform overflows: the reference's probabilities are NaN for this tile)")
    return total


def int_threshold(th) -> int:
    """for a uint8 image, img >= th with a float th is img >= ceil(th)"""
    return int(math.ceil(float(th)))


class PatchSampler(object):
    def __init__(self, sample_type: str, psize: int, nbr_colors: int, threshold_style: str, threshold: float):
        assert sample_type in SAMPLE_PATCHES, sample_type
        assert isinstance(psize, int) and psize > 0, psize
        assert isinstance(nbr_colors, int) and nbr_colors > 0, nbr_colors
        assert threshold_style in ROI_STYLE_TH, f"{threshold_style} not in {ROI_STYLE_TH}"
        self.sample_type, self.psize, self.nbr_colors = sample_type, psize, nbr_colors
        self.threshold_style, self.threshold = threshold_style, threshold

    def _threshold(self, img=None):
        if self.threshold_style == TH_FIX:
            return self.threshold
        from dlib.datasets.lowres import otsu_threshold          # threshold_otsu(image=img, nbins=self.nbr_colors) (:479-480)
        return otsu_threshold(img, self.nbr_colors)

    def _uniform(self, img: np.ndarray):
        h, w = img.shape
        return random.randint(0, max(0, h - self.psize)), random.randint(0, max(0, w - self.psize))

    def _draw(self, p: np.ndarray, img: np.ndarray):
        hit = np.random.multinomial(1, p.flatten(), size=1).reshape(p.shape).nonzero()
        r0, c0 = int(hit[0][0]), int(hit[1][0])
        assert 0 <= r0 <= img.shape[0] - self.psize and 0 <= c0 <= img.shape[1] - self.psize
        return r0, c0

    def _roi(self, img: np.ndarray, th):
        return self._draw(roi_probabilities(img, th, self.psize), img)

    def origin_probabilities(self, img: np.ndarray, th) -> np.ndarray:
        """probability of every candidate origin for the 'roi' / 'edt' / 'edt*roi' styles (:343-347,:389-392,:431-439)"""
        if self.sample_type == SAMPLE_ROI:
            return roi_probabilities(img, th, self.psize)
        from scipy.ndimage import distance_transform_edt as edt_fn
        h, w = img.shape
        lo, hi = int(self.psize / 2), math.ceil(self.psize / 2)
        roi = (img >= th).astype(np.float64)
        edt = edt_fn(input=roi, return_distances=True, return_indices=False)[lo:h - hi, lo:w - hi]
        if self.sample_type == SAMPLE_EDT:
            return ((edt.flatten() + 1.) / (edt + 1.).sum()).reshape(edt.shape)
        croi = roi[lo:h - hi, lo:w - hi]
        t1 = np.exp(croi * 5.)
        p_roi = (t1.flatten() + 1.) / (t1 + 1.).sum()
        t2 = np.exp(edt)
        p_edt = (t2.flatten() + 1.) / (t2 + 1.).sum()
        prob = p_roi * p_edt
        return (prob / prob.sum()).reshape(edt.shape)

    def __call__(self, img: np.ndarray, return_roi: bool):
        assert img.ndim == 2, img.ndim
        roi_u8 = None
        th = None
        if return_roi or self.sample_type != SAMPLE_UNIF:
            th = self._threshold(img)
            if return_roi:
                roi_u8 = (img >= th).astype(np.uint8)
        if self.sample_type == SAMPLE_UNIF:
            r0, c0 = self._uniform(img)
        else:
            r0, c0 = self._draw(self.origin_probabilities(img, th), img)
        return r0, c0, roi_u8


class DeviceRoiSampler:
    """'roi' sampling for a batch on the GPU.  ``tiles``: resident uint8 CUDA tensors [H, W] (the
    images the reference thresholds: the low-resolution tile interpolated to high resolution,
    dataset_dpsr.py:852-857); ``sample(ids)`` -> int32 [B, 2] origins (row, col) on the device."""

    def __init__(self, tiles, psize: int, threshold: int, seed: int = 0):
        import torch
        self.tiles, self.psize, self.threshold = tiles, int(psize), int(threshold)
        self.gen = torch.Generator(device=tiles[0].device)
        self.gen.manual_seed(int(seed))

    def sample(self, ids):
        import torch
        from srhip import ops
        u = torch.rand(len(ids), dtype=torch.float64, device=self.tiles[0].device, generator=self.gen)
        return ops.roi_sample(self.tiles, ids, self.psize, self.threshold, u), u


class DeviceWeightedSampler:
    """'edt', 'edt*roi' and 'roi' sampling with one threshold PER TILE for a batch on the GPU (the styles and the
    'automatic_threshold' of PatchSampler).  ``tiles``: resident uint8 CUDA tensors [H, W] as for DeviceRoiSampler;
    ``thresholds``: one number for all tiles, a list with one per tile, or None = Otsu's threshold of each tile
    (lowres.otsu_from_counts on srhip_hist_u8's counts).  Per tile and once: d2 = srhip_edt_sq (4 B per pixel, kept), the
    fp64 row prefix of ``origin_weights`` and the total, which must be finite (check_origin_total names the tile
    otherwise).  ``sample(ids)`` -> (int32 [B, 2] origins (row, col) on the device, the uniforms): one launch, the
    inverse CDF in row-major order.

    The probabilities are the reference's; the random stream is not: the host PatchSampler consumes numpy's global stream
    through np.random.multinomial, this one a torch device generator seeded like DeviceRoiSampler's (myseed + rank), as
    'roi' + 'fix_threshold' has done since round 2."""

    def __init__(self, tiles, psize: int, style: str, thresholds=None, seed: int = 0, names=None):
        import torch
        from srhip import ops
        from dlib.datasets.lowres import otsu_from_counts
        assert style in (SAMPLE_ROI, SAMPLE_EDT, SAMPLE_EDTXROI), style
        self.tiles, self.psize, self.style = tiles, int(psize), style
        dev = tiles[0].device
        if thresholds is None:
            thresholds = [otsu_from_counts(ops.hist_u8(t).cpu().numpy()) for t in tiles]
        elif not isinstance(thresholds, (list, tuple)):
            thresholds = [thresholds] * len(tiles)
        assert len(thresholds) == len(tiles), (len(thresholds), len(tiles))
        self.thresholds = [int_threshold(t) for t in thresholds]
        self.d2, self.rowcum, self.totals, desc = [], [], [], []
        for k, (t, th) in enumerate(zip(tiles, self.thresholds)):
            d2 = ops.edt_sq(t, th) if style != SAMPLE_ROI else None
            d, rowcum = ops.origin_rowsums(t, d2, self.psize, th, style)
            self.totals.append(check_origin_total(rowcum[-1].item(), names[k] if names else k, style))
            self.d2.append(d2)
            self.rowcum.append(rowcum)
            desc.append(d)
        self.table = ops.origin_table(desc, dev)          # built once: a launch takes tile ids and uniforms only
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(int(seed))

    def sample(self, ids):
        import torch
        from srhip import ops
        dev = self.tiles[0].device
        if not isinstance(ids, torch.Tensor):
            assert all(0 <= i < len(self.tiles) for i in ids), ids
            ids = torch.tensor(ids, dtype=torch.int32).to(dev)
        u = torch.rand(ids.numel(), dtype=torch.float64, device=dev, generator=self.gen)
        return ops.origin_sample(self.table, ids, u), u


DA_SEED_SALT = 0x6C725F6175676D74          # keeps the augmentation stream (da_gen) apart from the crop stream (gen)
LR_SYNTH_SEED_SALT = 0x70686F746F6E7321    # keeps the noise stream of --lr_synth psf (synth_gen) apart from both


def check_da_device(args):
    """The parameters of --da_device as ops.lr_augment takes them, ((on, prob, area, sigma), (on, prob, area, p), (on, prob,
    area, std)); a value the kernels cannot run, of a stage that is on, is refused by the name of its option."""
    from srhip import ops

    def unit(stage):
        for k in (f'{stage}_prob', f'{stage}_area'):
            v = float(getattr(args, k))
            if not 0. <= v <= 1.:
                raise ValueError(f"--da_device: {k} = {v} lies outside [0, 1]")
        return float(getattr(args, f'{stage}_prob')), float(getattr(args, f'{stage}_area'))
    blur = dot = gaus = (False, 0., 0., 0.)
    if getattr(args, 'da_blur', False):
        sigma = float(args.da_blur_sigma)
        if not sigma > 0.:
            raise ValueError(f"--da_device: da_blur_sigma = {sigma} must be above 0")
        if ops.lr_blur_radius(sigma) > ops.LR_BLUR_MAX_RADIUS:
            raise ValueError(f"--da_device: da_blur_sigma = {sigma} gives a blur radius of {ops.lr_blur_radius(sigma)}, above "
                             f"{ops.LR_BLUR_MAX_RADIUS}")
        blur = (True,) + unit('da_blur') + (sigma,)
    if getattr(args, 'da_dot_bin_noise', False):
        p = float(args.da_dot_bin_noise_p)
        if not 0. <= p < 1.:
            raise ValueError(f"--da_device: da_dot_bin_noise_p = {p} lies outside [0, 1)")
        dot = (True,) + unit('da_dot_bin_noise') + (p,)
    if getattr(args, 'da_add_gaus_noise', False):
        std = float(args.da_add_gaus_noise_std)
        if not 0. <= std < math.inf:
            raise ValueError(f"--da_device: da_add_gaus_noise_std = {std} must be a finite number >= 0")
        gaus = (True,) + unit('da_add_gaus_noise') + (std,)
    return blur, dot, gaus


def EvalPairsLike(args, pairs_h, pairs_l):
    """the LR resolution logic (true tile or synthesis) is EvalPairs' (utils_dataloaders.py)"""
    from dlib.utils.utils_dataloaders import EvalPairs
    return EvalPairs(args, pairs_h, pairs_l)


class ResidentTrainSet:
    """Training batches assembled ON the GPU from tiles that stay resident in HBM (uint8, or uint16 at full depth; float32 LR tiles of HR-only pairs) (a CACO-2
    split is a few hundred 8-bit tiles: tens of MB against 288 GB) -- the MI355X form of the TRAIN phase of
    DatasetDPSR.__getitem__ + DataLoader (dataset_dpsr.py:746-757,826-947, utils_dataloaders.py:138-158) for
    sets that ship true low-resolution tiles:

      per epoch   ShardedSampler(shuffle, seed + epoch, drop_last) -> this rank's minibatch index lists
      per batch   crop origins on the device ('uniform': torch.randint; 'roi': srhip_roi_sample on the
                  low-resolution tile interpolated to the high-resolution size and thresholded, as
                  :852-857), LR origin = HR origin // scale (:866-867), one augmentation mode 0..7 per
                  sample (:890), srhip_patch_gather for h_im and l_im (bit-exact crop / flip / rotate /
                  uint8 -> float32, g12)

    and returns the batch dict the trainer feeds ModelPlain: l_im, h_im, l_to_h_img (+ _aug), h_id, l_id and, with
    --ppiw, h_per_pixel_weight.  Also from the reference's item (round 3):
      * pairs without a true LR tile (or --use_interpolated_low): the LR tile is synthesised once at construction as the
        reference does per item (:776-804; dlib/datasets/lowres.py, seeded by the item index);
      * HR-only pairs -- no true LR tile and not a CACO-2 tile, e.g. the BioSR folds (:798-824,862-867): the LR tile is
        util.imresize_np of the mod-cropped HR tile / 255, computed once at construction by srhip_imresize_aa and kept
        resident in FLOAT32 (neither quantised nor clipped); its patches come from srhip_patch_gather_f32.  The reference
        crops such pairs uniformly and asserts it (:863-864); so does the constructor.  One set may mix uint8 and float
        LR tiles (CACO-2 and HR-only folds in one --train_dsets list);
      * the ROI image of the samplers is the LR tile brought to the HR size by srhip_resize_cubic (cv2.resize, :813-821);
        every style draws on the device: 'roi' + fixed threshold through srhip_roi_sample (DeviceRoiSampler), 'edt' /
        'edt*roi' and every style under 'automatic_threshold' (Otsu, per tile) through DeviceWeightedSampler -- the exact
        distance transform, the thresholds and the fp64 row prefixes are computed once at construction, a batch is one
        srhip_origin_sample launch.  SRHIP_HOST_SAMPLER=1 in the environment keeps these on the host PatchSampler (scipy
        per sample), the baseline of tools/sampler_rate.py;
      * the LR-only augmentations (--da_blur / --da_dot_bin_noise / --da_add_gaus_noise, :899-905) run on the host on
        the B low-resolution patches (a few hundred pixels each) with the reference's numpy stream, then l_to_h_img is
        resized from the augmented patch on the device and clipped (:905-906);
      * --da_device (not a reference option): the same three augmentations in place on the gathered l_im by one
        ops.lr_augment call (srhip_lr_augment) -- no host read, no upload, no scipy per sample.  The reference's order and
        rules (block, probabilities, scipy's Gaussian filter), the library's draws: Philox4x32-10 under a per-batch seed, a
        one-element int64 device tensor (the batch's 'da_seed') drawn by torch.randint from ``da_gen``, a generator of the
        set's own seeded from (myseed, rank) and a constant of its own -- the crop stream (``gen``) does not move, so origins
        and modes equal the un-augmented epoch's batch for batch.  The blur weights are built once at construction.  The random block is
        clamped to the patch where the reference would raise (an area near 0 or 1).  Refused by name at construction: a
        blur radius above 64, prob or area outside [0, 1], p outside [0, 1), a negative std or sigma, sigma 0 with the blur on;
      * --lr_synth psf (not a reference option): the resident float tile of an HR-only pair is the camera model's clean image
        bin_s(G_sigma * HR) (srhip_psf_bin, once per tile at construction) instead of util.imresize_np, and every batch gets fresh
        photon and read noise, LR = (Poisson(photons * clean) + read_std * N(0, 1)) / photons, by one ops.photon_noise call
        (srhip_photon_noise) in place on the gathered l_im of its HR-only samples -- before the da_* stages and before
        l_to_h_img is made -- under the batch's 'lr_synth_seed', a one-element int64 device tensor drawn from ``synth_gen``, a
        third generator seeded from (myseed, rank) and a constant of its own: ``gen`` and ``da_gen`` do not move.  photons 0: no
        noise and no launch.  Every other pair keeps its true tile or the reference's synthesis.  Refused by name at
        construction: a set without an HR-only pair, negative values, a blur radius above 64, read noise without photons;
      * 16-bit tiles (PIL mode I;16; the reference's cv2.imread(path, 0) would reduce them to 8 bits) stay resident as uint16
        and reach the batch at full depth, np.float32(min(v, in_max) / in_max) with --in_max (65535; 4095 for 12-bit data):
        srhip_patch_gather_u16, and srhip_imresize_aa_u16 for the float LR tile of an HR-only pair.  Where grey levels 0 .. 255
        are needed -- the ROI image, Otsu's histogram, --sample_tr_patch_th -- a 16-bit LR tile is reduced once by
        srhip_levels_u16_to_u8 to the levels of the metrics' ROI.  A set and a pair may mix depths.  Refused by name with a
        16-bit tile: --ppiw, SRCNN, DSR-Splines, and a CACO-2 tile without a true LR tile;
      * --ppiw: per-colour weights from the split's HR histogram (:592-645), per-pixel lookup on the device (:1037-1056)."""

    def __init__(self, args, pairs_h: dict, pairs_l: dict, device, rank: int = 0, world: int = 1):
        import torch
        import torch.nn.functional as F
        from dlib.utils.utils_dataloaders import imread_gray, refuse_16bit, ShardedSampler
        from dlib.utils.own_options import check_in_max
        from dlib.datasets import lowres
        if getattr(args, 'augment', False):
            raise NotImplementedError("ResidentTrainSet: --augment (the reference drops it too: dataset_dpsr.py:860-862 'passed')")
        da_params = check_da_device(args) if getattr(args, 'da_device', False) else None      # before any tile is read
        self.args, self.device, self.sf = args, torch.device(device), int(args.scale)
        self.psize, self.batch = int(args.h_size), int(args.batch_size)
        self.ids_h = list(pairs_h.keys())
        self.ids_l = [pairs_h[k]['low_path_key'] for k in self.ids_h]
        self.hr, self.lr, self.roi_src = [], [], []
        style = getattr(args, 'sample_tr_patch', SAMPLE_UNIF)
        assert style in SAMPLE_PATCHES, style
        self.style = style
        th_style = getattr(args, 'sample_tr_patch_th_style', TH_FIX)
        self.device_roi = style == SAMPLE_ROI and th_style == TH_FIX
        self.host_sampler = None
        self.device_weighted = (style != SAMPLE_UNIF and not self.device_roi
                                and os.environ.get('SRHIP_HOST_SAMPLER', '') != '1')
        if style != SAMPLE_UNIF and not self.device_roi and not self.device_weighted:
            self.host_sampler = PatchSampler(style, self.psize, int(getattr(args, 'color_max', 255)) + 1, th_style,
                                             float(getattr(args, 'sample_tr_patch_th', 0) or 0))
        ev = EvalPairsLike(args, pairs_h, pairs_l)
        self.hr_only = [ev.is_hr_only(idx) for idx in range(len(self.ids_h))]
        if any(self.hr_only) and style != SAMPLE_UNIF:
            # dataset_dpsr.py:863-864: `spatch = self.args.sample_tr_patch; assert spatch == constants.SAMPLE_UNIF, spatch`
            raise AssertionError(f"{style} (sample_tr_patch: a pair whose low-resolution image is synthesised from a tile "
                                 f"that is not a CACO-2 tile is cropped uniformly only; first: "
                                 f"{self.ids_h[self.hr_only.index(True)]})")
        self.in_max = check_in_max(getattr(args, 'in_max', None))           # the white level of 16-bit tiles (--in_max)
        self.lr_synth = ev.lr_synth     # None, or (sigma, photons, read_std) of --lr_synth psf: checked by EvalPairs
        if self.lr_synth is not None and not any(self.hr_only):
            raise ValueError("--lr_synth psf: the set has no HR-only pair (every pair has a true low-resolution tile or is a "
                             "CACO-2 tile, whose low-resolution image the option does not touch)")
        hr_host = []
        for idx, (hk, lk) in enumerate(zip(self.ids_h, self.ids_l)):
            h_path = pairs_h[hk]['abs_path']
            h_full = imread_gray(h_path)                                    # uint8, or uint16 at full depth
            if h_full.dtype == np.uint16:
                refuse_16bit(args, hk)
            h = torch.from_numpy(h_full[:, :, 0].copy())
            hh, ww = h.shape[0] - h.shape[0] % self.sf, h.shape[1] - h.shape[1] % self.sf      # modcrop
            h = h[:hh, :ww].contiguous()
            if self.hr_only[idx]:                                         # float32, resident: imresize_np of the cropped tile
                l = ev.low_res_f32(h_full[:hh, :ww], self.device).contiguous()
            else:
                l_np, _ = ev.low_res_u8(idx, h_full, h_path)              # true tile, or the reference's synthesis
                if l_np.dtype == np.uint16:
                    refuse_16bit(args, lk)
                l = torch.from_numpy(np.array(l_np[:, :, 0], copy=True))
                l = l[:hh // self.sf, :ww // self.sf].contiguous()
            assert l.shape == (hh // self.sf, ww // self.sf), (hk, tuple(h.shape), tuple(l.shape))
            assert hh >= self.psize and ww >= self.psize, f"{hk}: tile {hh}x{ww} < patch {self.psize}"
            self.hr.append(h.to(self.device))
            self.lr.append(l.to(self.device))
            hr_host.append(h.numpy())
            if style != SAMPLE_UNIF:      # the image the reference thresholds: cv2.resize(LR, HR size, INTER_CUBIC) (:813-821,852-857)
                roi_l = self.lr[-1]
                if roi_l.dtype == torch.uint16:       # at the 8-bit levels of the metrics' ROI, reduced once
                    from srhip import ops
                    roi_l = ops.levels_u16_to_u8(roi_l, self.in_max)
                self.roi_src.append(lowres.l_to_h(roi_l[None], (hh, ww))[0].contiguous())
        self.roi_host = [t.cpu().numpy() for t in self.roi_src] if self.host_sampler is not None else None
        if self.device_roi:
            self.roi = DeviceRoiSampler(self.roi_src, self.psize, int(args.sample_tr_patch_th), seed=int(args.myseed or 0) + rank)
        if self.device_weighted:
            self.weighted = DeviceWeightedSampler(
                self.roi_src, self.psize, style,
                thresholds=float(getattr(args, 'sample_tr_patch_th', 0) or 0) if th_style == TH_FIX else None,
                seed=int(args.myseed or 0) + rank, names=self.ids_h)
        self.da = any(getattr(args, f, False) for f in ('da_blur', 'da_dot_bin_noise', 'da_add_gaus_noise'))
        self.da_device = bool(getattr(args, 'da_device', False)) and self.da
        if self.da_device:      # the draws of ops.lr_augment: a stream of the set's own, so that the crop stream does not move
            from srhip import ops
            self.da_params = da_params
            self.da_weights = ops.lr_blur_weights(da_params[0][3], self.device) if da_params[0][0] else None
            self.da_gen = torch.Generator(device=self.device)
            self.da_gen.manual_seed((int(args.myseed or 0) * 1000003 + rank) ^ DA_SEED_SALT)
        if self.lr_synth is not None:     # the noise seeds of --lr_synth psf: a third stream, so that gen and da_gen do not move
            self.synth_gen = torch.Generator(device=self.device)
            self.synth_gen.manual_seed((int(args.myseed or 0) * 1000003 + rank) ^ LR_SYNTH_SEED_SALT)
        self.ppiw_table = None
        if getattr(args, 'ppiw', False):
            self.ppiw_table = torch.from_numpy(lowres.per_color_weights(
                hr_host, int(getattr(args, 'color_min', 0)), int(getattr(args, 'color_max', 255)),
                float(getattr(args, 'ppiw_min_per_col_w', 1e-3)))).float().to(self.device)
        self.sampler = ShardedSampler(len(self.ids_h), world, rank, shuffle=True, seed=int(args.myseed or 0), drop_last=True)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(args.myseed or 0) * 1000003 + rank)

    def __len__(self):
        return len(self.sampler) // self.batch

    def epoch(self, epoch: int):
        """Iterator over this rank's batch dicts of one epoch (set_epoch semantics of utils_trainer.py:325-326)."""
        import torch
        from srhip import ops
        self.sampler.set_epoch(epoch)
        P, sf = self.psize, self.sf
        for ids in self.sampler.batches(self.batch, drop_last=True):
            B = len(ids)
            if self.device_roi or self.device_weighted:
                org, _ = (self.roi if self.device_roi else self.weighted).sample(ids)
                org = org.cpu().tolist()                      # B x 2 ints: the only host round trip of the batch
            elif self.host_sampler is not None:               # SRHIP_HOST_SAMPLER=1: the reference's sampler on the host
                org = [list(self.host_sampler(self.roi_host[i], False)[:2]) for i in ids]
            else:
                u = torch.rand(B, 2, device=self.device, generator=self.gen).cpu()
                org = [[int(u[b, 0] * (self.hr[i].shape[0] - P + 1)), int(u[b, 1] * (self.hr[i].shape[1] - P + 1))]
                       for b, i in enumerate(ids)]
            modes = torch.randint(0, 8, (B,), device=self.device, generator=self.gen).cpu().tolist()
            y0, x0 = [o[0] for o in org], [o[1] for o in org]
            batch = ops.train_batch(self.hr, self.lr, ids, y0, x0, modes, P, sf, in_max=self.in_max)
            if self.lr_synth is not None:     # --lr_synth psf: fresh photon and read noise on the HR-only samples' clean patches
                batch['lr_synth_seed'] = torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, device=self.device,
                                                       generator=self.synth_gen)   # stays on the device: the kernel reads it there
                on = [self.hr_only[i] for i in ids]
                if self.lr_synth[1] > 0. and any(on):
                    ops.photon_noise(batch['l_im'], batch['lr_synth_seed'], self.lr_synth[1], self.lr_synth[2], on)
            if self.da_device:      # LR-only augmentations (:899-905) in place on the device, one seed per batch
                batch['da_seed'] = torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, device=self.device,
                                                 generator=self.da_gen)       # stays on the device: the kernels read it there
                ops.lr_augment(batch['l_im'], batch['da_seed'], self.da_params, self.da_weights)
            elif self.da:     # LR-only augmentations (:899-905): B patches of (P / s)^2 pixels through the reference's numpy code
                from dlib.datasets import lowres
                host = batch['l_im'].permute(0, 2, 3, 1).cpu().numpy()
                host = np.stack([lowres.apply_lr_augmentations(np.ascontiguousarray(host[b]), self.args) for b in range(B)])
                batch['l_im'] = torch.from_numpy(host).permute(0, 3, 1, 2).contiguous().to(self.device)
            # the LR patch at the HR size: cv2.resize(img_l, (P, P), INTER_CUBIC) clipped to [0, 1] (:905-907)
            up = ops.clip01_(ops.resize_cubic(batch['l_im'][:, 0].contiguous(), (P, P)))
            batch['l_to_h_img'] = up[:, None]
            batch['l_to_h_img_aug'] = batch['l_to_h_img']
            if self.ppiw_table is not None:
                from dlib.datasets import lowres
                batch['h_per_pixel_weight'] = lowres.per_pixel_weight(batch['h_im'], self.ppiw_table)
            batch['h_id'] = [self.ids_h[i] for i in ids]
            batch['l_id'] = [self.ids_l[i] for i in ids]
            batch['origin'], batch['mode'] = org, modes
            yield batch
