"""The options the reference's parser does not have (dlib/utils/own_options.py), case by case: an entry point plus a command line
or a configuration.  tests/golden/own_options.json holds each case's outcome as the commit before the table gave it;
tests/test_cpu_own_options.py replays the list and compares for equality.

Entry points: 'main' (main.parse_input), 'eval' (eval.load_args on tests/golden/eval_exp, or on a temporary copy whose
config_model.yml also records ``recorded``), 'resume' (main._resume_point on a temporary folder that holds ``yml`` as its
config_model.yml), 'resolvers' (the five check_* on a configuration that no command line can produce).

An outcome is {'keys': the keys among these options with their values, 'resolved': what the five check_* return, 'plan': the three
fields of eval_plan}, or {'exit': code, 'error': the stderr line after 'error: '}, or {'raises': type, 'text': message}, or
{'returns': the iteration _resume_point found}.  Every value is its repr, so 5 is not 5.0 is not True."""
import contextlib
import functools
import importlib.util
import io
import os

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")
NAMES = ("in_max", "metric_levels", "msssim", "msssim_scales", "frc", "frc_threshold", "lr_synth", "lr_synth_psf_sigma",
         "lr_synth_photons", "lr_synth_read_std")
SWIN = ["--net_type", "swinir", "--method", "SWINIR"]
RECORDED = dict(in_max=4095, metric_levels=4095, msssim=True, msssim_scales=3, frc=True, frc_threshold=0.25, lr_synth="psf",
                lr_synth_psf_sigma=1.2, lr_synth_photons=150.0, lr_synth_read_std=1.5)
TAGGED = "net_type: swinir\nscale: 2\nmetric_levels: 4095\nmsssim: true\nmsssim_scales: 3\nodd: !!python/tuple [1, 2]\n"


def _main(name, *flags):
    return {"id": f"main-{name}", "entry": "main", "argv": list(flags)}


def _eval(name, *flags, recorded=None):
    return {"id": f"eval-{name}", "entry": "eval", "argv": list(flags), "recorded": recorded}


def _resume(name, yml, *flags):
    return {"id": f"resume-{name}", "entry": "resume", "argv": list(flags), "yml": yml}


def _cfg(name, **cfg):
    return {"id": f"resolvers-{name}", "entry": "resolvers", "cfg": cfg}


CASES = [
    # ---- main.py: nothing given, nothing recorded; then option by option, each a key only when given
    _main("plain"),
    _main("in_max", "--in_max", "4095"),
    _main("in_max-0", "--in_max", "0"),
    _main("in_max-65536", "--in_max", "65536"),
    _main("metric_levels", "--metric_levels", "4095"),
    _main("metric_levels-254", "--metric_levels", "254"),
    _main("metric_levels-65536", "--metric_levels", "65536"),
    _main("msssim", "--msssim", "True"),
    _main("msssim-false", "--msssim", "False"),
    _main("msssim-3", "--msssim", "True", "--msssim_scales", "3"),
    _main("msssim-selects", "--msssim", "True", "--model_select_mtr", "msssim"),
    _main("msssim_scales-alone", "--msssim_scales", "3"),
    _main("msssim_scales-off", "--msssim", "False", "--msssim_scales", "3"),
    _main("msssim-select-alone", "--model_select_mtr", "msssim"),
    _main("msssim_scales-6", "--msssim", "True", "--msssim_scales", "6"),
    _main("msssim_scales-0", "--msssim", "True", "--msssim_scales", "0"),
    _main("msssim-select-roi", "--msssim", "True", "--model_select_mtr", "msssim", "--eval_over_roi_also_model_select", "True"),
    _main("frc", "--frc", "True"),
    _main("frc-false", "--frc", "False"),
    _main("frc-0.5", "--frc", "True", "--frc_threshold", "0.5"),
    _main("frc-select", "--model_select_mtr", "frc_cut"),
    _main("frc-select-on", "--frc", "True", "--model_select_mtr", "frc_cut"),
    _main("frc_threshold-alone", "--frc_threshold", "0.5"),
    _main("frc_threshold-off", "--frc", "False", "--frc_threshold", "0.5"),
    _main("frc_threshold-0", "--frc", "True", "--frc_threshold", "0"),
    _main("frc_threshold-1", "--frc", "True", "--frc_threshold", "1.0"),
    _main("frc_threshold-nan", "--frc", "True", "--frc_threshold", "nan"),
    _main("lr_synth-psf", "--lr_synth", "psf"),
    _main("lr_synth-bicubic", "--lr_synth", "bicubic"),
    _main("lr_synth-full", "--lr_synth", "psf", "--lr_synth_psf_sigma", "1.2", "--lr_synth_photons", "150", "--lr_synth_read_std",
          "1.5"),
    _main("lr_synth-sigma", "--lr_synth", "psf", "--lr_synth_psf_sigma", "2"),
    _main("lr_synth-other", "--lr_synth", "lanczos"),
    _main("lr_synth_psf_sigma-alone", "--lr_synth_psf_sigma", "1.2"),
    _main("lr_synth_photons-alone", "--lr_synth_photons", "150"),
    _main("lr_synth_read_std-alone", "--lr_synth_read_std", "1.5"),
    _main("lr_synth-two-alone", "--lr_synth_read_std", "1.5", "--lr_synth_photons", "150"),
    _main("lr_synth_photons-negative", "--lr_synth", "psf", "--lr_synth_photons", "-1"),
    _main("lr_synth_photons-inf", "--lr_synth", "psf", "--lr_synth_photons", "inf"),
    _main("lr_synth_read_std-nan", "--lr_synth", "psf", "--lr_synth_photons", "10", "--lr_synth_read_std", "nan"),
    _main("lr_synth-bicubic-sigma", "--lr_synth", "bicubic", "--lr_synth_psf_sigma", "1.2"),
    _main("lr_synth_psf_sigma-radius", "--lr_synth", "psf", "--lr_synth_psf_sigma", "20"),
    _main("lr_synth_photons-above", "--lr_synth", "psf", "--lr_synth_photons", "2e6"),
    _main("lr_synth_read_std-no-photons", "--lr_synth", "psf", "--lr_synth_read_std", "1.5"),
    _main("all", "--in_max", "4095", "--metric_levels", "4095", "--msssim", "True", "--msssim_scales", "2", "--frc", "True",
          "--frc_threshold", "0.25", "--lr_synth", "psf", "--lr_synth_psf_sigma", "1.2", "--lr_synth_photons", "150"),
    _main("unknown-flag", "--frc_treshold", "0.5"),
    _main("msssim-not-a-bool", "--msssim", "maybe"),
    # ---- eval.py on the fixture, whose config_model.yml records none of them
    _eval("plain"),
    _eval("in_max", "--in_max", "4095"),
    _eval("in_max-0", "--in_max", "0"),
    _eval("metric_levels", "--metric_levels", "65535"),
    _eval("metric_levels-100", "--metric_levels", "100"),
    _eval("msssim", "--msssim", "True"),
    _eval("msssim-2", "--msssim", "True", "--msssim_scales", "2"),
    _eval("msssim_scales-alone", "--msssim_scales", "2"),
    _eval("msssim_scales-9", "--msssim", "True", "--msssim_scales", "9"),
    _eval("frc", "--frc", "True"),
    _eval("frc-0.25", "--frc", "True", "--frc_threshold", "0.25"),
    _eval("frc_threshold-alone", "--frc_threshold", "0.25"),
    _eval("frc_threshold-1.5", "--frc", "True", "--frc_threshold", "1.5"),
    _eval("frc-not-a-bool", "--frc", "perhaps"),
    _eval("no-lr_synth-flag", "--lr_synth", "psf"),
    # ---- eval.py on a copy that records all of them: read back, overridden flag by flag
    _eval("recorded", recorded=RECORDED),
    _eval("recorded-in_max", "--in_max", "1023", recorded=RECORDED),
    _eval("recorded-metric_levels", "--metric_levels", "255", recorded=RECORDED),
    _eval("recorded-msssim_scales", "--msssim_scales", "5", recorded=RECORDED),
    _eval("recorded-msssim-false", "--msssim", "False", recorded=RECORDED),
    _eval("recorded-frc_threshold", "--frc_threshold", "0.5", recorded=RECORDED),
    _eval("recorded-frc-false", "--frc", "False", recorded=RECORDED),
    _eval("recorded-frc-false-threshold", "--frc", "False", "--frc_threshold", "0.5", recorded=RECORDED),
    _eval("recorded-frc-only", "--frc", "True", recorded=dict(frc=False)),
    _eval("recorded-msssim-select", recorded=dict(msssim=True, model_select_mtr="msssim")),
    _eval("recorded-msssim-select-off", "--msssim", "False", recorded=dict(msssim=True, model_select_mtr="msssim")),
    # ---- a resumed run against the folder's config_model.yml
    _resume("no-file", None),
    _resume("same", "net_type: swinir\nscale: 2\n"),
    _resume("nested-net_type", "netG:\n  net_type: swinir\nscale: 2\n"),
    _resume("other-net", "net_type: vdsr\nscale: 2\n"),
    _resume("other-scale", "net_type: swinir\nscale: 4\n"),
    _resume("metric_levels-recorded", "net_type: swinir\nscale: 2\nmetric_levels: 4095\n"),
    _resume("metric_levels-asked", "net_type: swinir\nscale: 2\n", "--metric_levels", "4095"),
    _resume("metric_levels-same", "net_type: swinir\nscale: 2\nmetric_levels: 4095\n", "--metric_levels", "4095"),
    _resume("metric_levels-255", "net_type: swinir\nscale: 2\n", "--metric_levels", "255"),
    _resume("msssim-recorded", "net_type: swinir\nscale: 2\nmsssim: true\nmsssim_scales: 3\n"),
    _resume("msssim-asked", "net_type: swinir\nscale: 2\nmsssim: false\n", "--msssim", "True"),
    _resume("msssim-other-scales", "net_type: swinir\nscale: 2\nmsssim: true\nmsssim_scales: 3\n", "--msssim", "True"),
    _resume("msssim-same", "net_type: swinir\nscale: 2\nmsssim: true\nmsssim_scales: 3\n", "--msssim", "True", "--msssim_scales", "3"),
    _resume("msssim-default-scales", "net_type: swinir\nscale: 2\nmsssim: true\n", "--msssim", "True", "--msssim_scales", "5"),
    _resume("msssim-false-both", "net_type: swinir\nscale: 2\nmsssim: false\n", "--msssim", "False"),
    _resume("frc-and-lr_synth-are-free", "net_type: swinir\nscale: 2\nfrc: true\nfrc_threshold: 0.25\nlr_synth: psf\nin_max: 4095\n"),
    _resume("empty-file", ""),
    _resume("tagged-plain", TAGGED),
    _resume("tagged-levels-only", TAGGED, "--metric_levels", "4095"),
    _resume("tagged-same", TAGGED, "--metric_levels", "4095", "--msssim", "True", "--msssim_scales", "3"),
    _resume("tagged-other-net", TAGGED.replace("swinir", "vdsr")),
    # ---- the resolvers on values only a hand-written configuration holds
    _cfg("nothing"),
    _cfg("in_max-70000", in_max=70000),
    _cfg("in_max-bool", in_max=True),
    _cfg("in_max-float", in_max=4095.0),
    _cfg("in_max-fraction", in_max=1.5),
    _cfg("metric_levels-100", metric_levels=100),
    _cfg("metric_levels-float", metric_levels=4095.0),
    _cfg("metric_levels-bool", metric_levels=True),
    _cfg("msssim_scales-float", msssim=True, msssim_scales=2.0),
    _cfg("msssim_scales-bool", msssim=True, msssim_scales=True),
    _cfg("msssim_scales-fraction", msssim=True, msssim_scales=2.5),
    _cfg("frc_threshold-text", frc=True, frc_threshold="0.5"),
    _cfg("frc_threshold-bool", frc=True, frc_threshold=True),
    _cfg("frc_threshold-int", frc=True, frc_threshold=1),
    _cfg("lr_synth_photons-text", lr_synth="psf", lr_synth_photons="3"),
    _cfg("lr_synth_psf_sigma-no-kind", lr_synth_psf_sigma=1.0),
    _cfg("lr_synth-int-values", lr_synth="psf", lr_synth_psf_sigma=1, lr_synth_photons=10, lr_synth_read_std=2),
]


@functools.lru_cache(maxsize=None)
def _eval_module():
    spec = importlib.util.spec_from_file_location("srhip_eval_own_options", os.path.join(ROOT, "sr-caco-2_amd", "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def _resolved(a):
    O = importlib.import_module("dlib.utils.own_options")
    out = {"keys": {k: repr(a[k]) for k in NAMES if k in a},
           "resolved": {"in_max": repr(O.check_in_max(getattr(a, "in_max", None))),
                        "metric_levels": repr(O.check_metric_levels(getattr(a, "metric_levels", None))),
                        "msssim_scales": repr(O.check_msssim(a)), "frc_threshold": repr(O.check_frc(a)),
                        "lr_synth": repr(O.check_lr_synth(a))}}
    plan = O.eval_plan(a)
    out["plan"] = [repr(plan.levels), repr(plan.msssim_scales), repr(plan.frc_threshold)]
    return out


def _run(case, tmp):
    import main
    if case["entry"] == "main":
        return _resolved(main.parse_input(SWIN + case["argv"]))
    if case["entry"] == "eval":
        exp = os.path.join(FX, "exp")
        if case["recorded"] is not None:
            cfg = yaml.safe_load(open(os.path.join(exp, "config_model.yml")))
            cfg.update(case["recorded"])
            exp = str(tmp / "exp")
            os.makedirs(exp)
            yaml.dump(cfg, open(os.path.join(exp, "config_model.yml"), "w"))
        ns, a = _eval_module().load_args(["--exp_path", exp, "--data_root", os.path.join(FX, "data")] + case["argv"])
        assert {k for k in NAMES if hasattr(ns, k)} == set(NAMES[:6])            # eval.py takes six of them, no --lr_synth*
        return _resolved(a)
    if case["entry"] == "resume":
        a = main.parse_input(SWIN + ["--outd", str(tmp)] + case["argv"])
        a.outd_backup = a.outd
        if case["yml"] is not None:
            open(tmp / "config_model.yml", "w").write(case["yml"])
        return {"returns": repr(main._resume_point(a))}
    from dlib.utils.tools import Dict2Obj
    return _resolved(Dict2Obj(case["cfg"]))


def outcome(case, tmp):
    """what the case gives, in the module docstring's form; ``tmp``: an empty folder (a pathlib.Path) of the case's own"""
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return _run(case, tmp)
    except SystemExit as e:
        if isinstance(e.code, int):                  # argparse: usage, then '<prog>: error: <text>'
            return {"exit": e.code, "error": err.getvalue().split("error: ", 1)[1].rstrip("\n")}
        return {"raises": "SystemExit", "text": str(e).replace(str(tmp), "<outd>")}
    except ValueError as e:
        return {"raises": "ValueError", "text": str(e)}

