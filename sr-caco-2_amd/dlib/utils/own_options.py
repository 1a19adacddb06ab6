"""The run options the reference's parser does not have, stated once: OPTIONS declares each flag (type, the command lines that
take it, help text, group), GROUPS gives each group its resolver -- the only place where its ranges and "needs --X" rules are
written -- and, where a resumed run must match the folder, the compared value.

The contract they share: a flag is a key of the configuration and of config_model.yml only when it is given, so a run without it
is bit for bit the earlier run; eval.py reads the recorded value back and overrides it with a flag of its own (apply_recorded); a
bad value is refused by option name with exit code 2 before the device is used (validate); the evaluation path takes its answers
from one resolved record (eval_plan).  No torch and no device use at import."""
import argparse
import math
from collections import namedtuple
from typing import NamedTuple

from dlib.utils import constants


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('true', '1', 'yes'):
        return True
    if v.lower() in ('false', '0', 'no'):
        return False
    raise argparse.ArgumentTypeError(f'boolean expected, got {v!r}')


Option = namedtuple('Option', 'name type clis help group')          # clis: the command lines that take it, of 'main', 'eval'
BOTH = ('main', 'eval')
OPTIONS = (
    # the white level of 16-bit tiles, which are read as min(v, in_max) / in_max: 65535 when not given, 4095 for 12-bit data in a
    # 16-bit container; no effect on 8-bit tiles.  predict.py finds it in config_model.yml as eval.py does.
    Option('in_max', int, BOTH, "white level of 16-bit tiles, 1 .. 65535 (default: the one the run recorded in config_model.yml, "
           "else 65535); no effect on 8-bit tiles", 'in_max'),
    # the white level the evaluation metrics quantise prediction and target to, 255 .. 65535 -- normally the set's in_max.  Not
    # given: 255, the reference's 8-bit-level metrics.  Given: MSE in levels^2, PSNR against that white level, SSIM in float64
    # (dlib.metrics.sweep); the ROIs stay defined at the 8-bit levels.
    Option('metric_levels', int, BOTH, "white level the metrics quantise prediction and target to, 255 .. 65535 (default: the one "
           "the run recorded in config_model.yml, else 255: the reference's 8-bit-level metrics); the bicubic baseline row is "
           "measured at the same level", 'metric_levels'),
    # --msssim True: every evaluation also computes the multi-scale SSIM of Wang, Simoncelli and Bovik (2003) over --msssim_scales
    # scales (1 .. 5, default 5), in float64 at the white level of the metrics (include/srhip.h states it): 'msssim' in the tracker,
    # details_*.yml, the best-model yaml files and the log, never in the ROI files; and --model_select_mtr msssim becomes possible.
    Option('msssim', str2bool, BOTH, "also compute the multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of the net and of the bicubic "
           "baseline row (default: what the run recorded in config_model.yml, else off)", 'msssim'),
    Option('msssim_scales', int, BOTH, "--msssim True: the number of scales, 1 .. 5 (default: the run's, else 5); both sides of an "
           "evaluation image, the border excluded, must be at least 10 * 2^(scales - 1) + 1", 'msssim'),
    # --frc True: every evaluation also computes the Fourier ring correlation of prediction against target (include/srhip.h states
    # it) and reports its cutoff at --frc_threshold (in (0, 1), default 1 / 7) as a fraction of Nyquist: 'frc_cut' per image in
    # details_*.yml, the set mean in the log, best-models/frc_<ds>.yml with the mean curve.  A report metric: no tracker holds it and
    # --model_select_mtr frc_cut is refused; nothing a resumed run records depends on it.
    Option('frc', str2bool, BOTH, "also compute the Fourier ring correlation of prediction against target, for the net and for the "
           "bicubic baseline row: 'frc_cut' per image in details_*.yml, best-models/frc_<ds>.yml, the mean in the log "
           "(default: what the run recorded in config_model.yml, else off)", 'frc'),
    Option('frc_threshold', float, BOTH, "--frc True: the threshold of the cutoff, in (0, 1) (default: the run's, else 1 / 7)", 'frc'),
    # how the LR image of an HR-only pair is made: 'bicubic' (default: util.imresize_np, the reference's) or 'psf', a camera model --
    # clean = bin_s(G_sigma * HR) with sigma in HR pixels, then per training batch LR = (Poisson(photons * clean) + read_std *
    # N(0, 1)) / photons with photons the expected count at white level and read_std in counts; photons 0: no noise.  float32, no
    # offset, no clipping, no quantisation.  Keys of the configuration and of config_model.yml -- where eval.py finds them -- only
    # when --lr_synth is given.
    Option('lr_synth', str, ('main',), "how the LR image of an HR-only pair is made: bicubic (default) or psf, a camera model", 'lr_synth'),
    Option('lr_synth_psf_sigma', float, ('main',), "--lr_synth psf: sigma of the Gaussian PSF, in HR pixels", 'lr_synth'),
    Option('lr_synth_photons', float, ('main',), "--lr_synth psf: expected photon count at white level; 0: no noise", 'lr_synth'),
    Option('lr_synth_read_std', float, ('main',), "--lr_synth psf: read noise, in photon counts", 'lr_synth'),
)


def in_levels(v, lo, hi):
    """v is a whole number in lo .. hi: the range rule of a white level"""
    return int(v) == v and lo <= v <= hi


def check_in_max(in_max):
    """--in_max: the white level of 16-bit tiles, 1 .. 65535 (None: 65535); no effect on 8-bit tiles"""
    if in_max is None:
        return 65535
    if isinstance(in_max, bool) or not in_levels(in_max, 1, 65535):
        raise ValueError(f'--in_max {in_max}: the white level of 16-bit tiles is an integer in 1 .. 65535')
    return int(in_max)


def check_metric_levels(levels):
    """--metric_levels: the white level the metrics quantise both images to, 255 .. 65535 (None: 255, the reference's metrics)"""
    if levels is None:
        return 255
    if isinstance(levels, bool) or not in_levels(levels, 255, 65535):
        raise ValueError(f'--metric_levels {levels}: the white level of the metrics is an integer in 255 .. 65535')
    return int(levels)


def check_msssim(args):
    """--msssim / --msssim_scales: the number of scales of the multi-scale SSIM this run computes, 1 .. 5 (default 5), or 0
    without --msssim True; also what --model_select_mtr msssim needs"""
    on, scales = getattr(args, 'msssim', None), getattr(args, 'msssim_scales', None)
    if not on:
        if scales is not None:
            raise ValueError(f'--msssim_scales {scales} needs --msssim True')
        if getattr(args, 'model_select_mtr', None) == constants.MSSSIM_MTR:
            raise ValueError(f'--model_select_mtr {constants.MSSSIM_MTR} needs --msssim True')
        return 0
    scales = 5 if scales is None else scales
    if isinstance(scales, bool) or not in_levels(scales, 1, 5):
        raise ValueError(f'--msssim_scales {scales}: the number of scales is an integer in 1 .. 5')
    if getattr(args, 'model_select_mtr', None) == constants.MSSSIM_MTR and getattr(args, 'eval_over_roi_also_model_select', False):
        raise ValueError(f'--model_select_mtr {constants.MSSSIM_MTR} is a whole-image metric: it cannot select the model over the '
                         f'ROI (--eval_over_roi_also_model_select True)')
    return int(scales)


def check_frc(args):
    """--frc / --frc_threshold: the threshold of the Fourier ring correlation cutoff this run reports, a number in (0, 1) (default
    1 / 7), or 0 without --frc True.  The cutoff is a report metric, a threshold crossing that is discontinuous in the weights:
    --model_select_mtr frc_cut is refused by name, with or without the option"""
    on, thr = getattr(args, 'frc', None), getattr(args, 'frc_threshold', None)
    if getattr(args, 'model_select_mtr', None) == constants.FRC_CUT:
        raise ValueError(f'--model_select_mtr {constants.FRC_CUT}: the cutoff of the Fourier ring correlation is a report metric '
                         f'(--frc True), not a selection criterion')
    if not on:
        if thr is not None:
            raise ValueError(f'--frc_threshold {thr} needs --frc True')
        return 0
    thr = 1.0 / 7.0 if thr is None else thr
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not 0.0 < thr < 1.0:
        raise ValueError(f'--frc_threshold {thr}: the threshold is a number in (0, 1)')
    return float(thr)


LR_SYNTHS = ('bicubic', 'psf')
_LR_SYNTH_FLOATS = ('lr_synth_psf_sigma', 'lr_synth_photons', 'lr_synth_read_std')


def check_lr_synth(args):
    """--lr_synth (not a reference option): None for 'bicubic' (or no key: util.imresize_np, the reference's LR image of an
    HR-only pair), else (sigma, photons, read_std) of the camera model 'psf' -- clean = bin_s(G_sigma * HR), LR = (Poisson(photons
    * clean) + read_std * N(0, 1)) / photons; photons 0: no noise.  A value the kernels cannot run is refused by option name."""
    from dlib.datasets import lowres
    kind = getattr(args, 'lr_synth', None)
    if kind is None:
        kind = 'bicubic'
    if kind not in LR_SYNTHS:
        raise ValueError(f"--lr_synth {kind}: one of {', '.join(LR_SYNTHS)}")
    vals = {}
    for k in _LR_SYNTH_FLOATS:
        v = getattr(args, k, None)
        v = 0. if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0. <= v < math.inf:
            raise ValueError(f"--{k} {v}: a finite number >= 0")
        vals[k] = float(v)
    sigma, photons, read_std = vals['lr_synth_psf_sigma'], vals['lr_synth_photons'], vals['lr_synth_read_std']
    if kind != 'psf':
        if sigma or photons or read_std:
            raise ValueError("--lr_synth_psf_sigma / --lr_synth_photons / --lr_synth_read_std need --lr_synth psf")
        return None
    if int(4.0 * sigma + 0.5) > lowres.LR_BLUR_MAX_RADIUS:
        raise ValueError(f"--lr_synth_psf_sigma {sigma} gives a blur radius of {int(4.0 * sigma + 0.5)}, above "
                         f"{lowres.LR_BLUR_MAX_RADIUS}")
    if photons > lowres.LR_SYNTH_MAX_PHOTONS:
        raise ValueError(f"--lr_synth_photons {photons}: at most {lowres.LR_SYNTH_MAX_PHOTONS:g}")
    if read_std > 0. and photons == 0.:
        raise ValueError(f"--lr_synth_read_std {read_std} needs --lr_synth_photons above 0: the read noise is in photon counts")
    return sigma, photons, read_std


def _lr_synth_given(args):
    """the group on a command line: a float without --lr_synth is refused, and with it all three are keys, 0. where not given"""
    given = [k for k in _LR_SYNTH_FLOATS if getattr(args, k, None) is not None]
    if getattr(args, 'lr_synth', None) is None:
        if given:
            raise ValueError(f"--{given[0]} needs --lr_synth psf")
    else:
        for k in _LR_SYNTH_FLOATS:
            if k not in given:
                setattr(args, k, 0.)
    return check_lr_synth(args)


# what a resumed run must find unchanged in the folder's config_model.yml: the key the refusal shows, the value a recorded
# configuration stands for (an absent key meaning the default) and the value this run's args ask for
Resume = namedtuple('Resume', 'key recorded asked')
# resolve: args -> the group's resolved value, or ValueError by option name
Group = namedtuple('Group', 'name resolve resume', defaults=(None,))
GROUPS = (                               # in the order a command line is checked
    Group('in_max', lambda a: check_in_max(getattr(a, 'in_max', None))),
    # metric_levels, absent meaning 255: a tracker that mixed 8-bit and full-depth PSNRs would select a wrong best model
    Group('metric_levels', lambda a: check_metric_levels(getattr(a, 'metric_levels', None)),
          Resume('metric_levels', lambda old: old.get('metric_levels', 255), lambda a: getattr(a, 'metric_levels', None) or 255)),
    Group('lr_synth', _lr_synth_given),
    # msssim_scales, 0 meaning a run without --msssim True: its tracker would gain or lose the key
    Group('msssim', check_msssim,
          Resume('msssim_scales', lambda old: int(old.get('msssim_scales') or 5) if str(old.get('msssim')).lower() == 'true' else 0,
                 check_msssim)),
    Group('frc', check_frc),
)
RESUME = tuple(g.resume for g in GROUPS if g.resume)
# the keys RESUME reads, for a config_model.yml that has to be searched as text
RESUME_KEYS = tuple(o.name for o in OPTIONS if any(g.name == o.group and g.resume for g in GROUPS))


def add_arguments(ap, cli):
    """the flags ``cli`` ('main' or 'eval') takes; none has a default, so a flag not given stays out of the configuration"""
    for o in OPTIONS:
        if cli in o.clis:
            ap.add_argument(f'--{o.name}', type=o.type, default=None, help=o.help)


def validate(args, error):
    """every group's resolver on a configuration or a parsed command line; a refusal goes to ``error`` (ap.error: exit code 2)"""
    try:
        for g in GROUPS:
            g.resolve(args)
    except ValueError as e:
        error(str(e))


def apply_recorded(args, ns, error):
    """eval.py: the configuration config_model.yml recorded, overridden by the flags given; then validate"""
    for o in OPTIONS:
        if getattr(ns, o.name, None) is not None:
            args[o.name] = getattr(ns, o.name)
    if ns.frc is False and ns.frc_threshold is None:
        args.pop('frc_threshold', None)               # --frc False alone turns off a run recorded with a threshold of its own
    validate(args, error)


class EvalPlan(NamedTuple):
    """what the evaluation path asks the options: the white level of the metrics (255: the reference's), the scales of the
    multi-scale SSIM (0: none) and the threshold of the Fourier ring correlation (0: none)"""
    levels: int
    msssim_scales: int
    frc_threshold: float

    def frc_kwargs(self):
        return {} if self.levels == 255 else {'levels': self.levels}

    def sweep_kwargs(self):
        """what dlib.metrics.sweep gets beyond the reference's arguments; {} is the reference's call"""
        return {**self.frc_kwargs(), **({'msssim': self.msssim_scales} if self.msssim_scales else {})}


def eval_plan(args):
    return EvalPlan(check_metric_levels(getattr(args, 'metric_levels', None)), check_msssim(args), check_frc(args))
