"""The options the reference's parser does not have (dlib/utils/own_options.py): every case of tests/own_option_cases.py gives what
tests/golden/own_options.json recorded from the commit before the table -- the same keys, resolver results, error lines and
refusals, strings compared exactly and floats through their repr -- and the structure that keeps them stated once."""
import json
import os
import re
import subprocess
import sys

import pytest

import own_option_cases as K

PKG = os.path.join(K.ROOT, "sr-caco-2_amd")
HOST_FILES = ("main.py", "eval.py", "predict.py") + tuple(os.path.join("dlib", *p) for p in (
    ("utils", "utils_dataloaders.py"), ("utils", "utils_trainer.py"), ("utils", "utils_tracker.py"), ("datasets", "dataset_dpsr.py")))
GOLDEN = json.load(open(os.path.join(K.ROOT, "tests", "golden", "own_options.json")))


def test_the_golden_file_holds_the_case_list():
    ids = [c["id"] for c in K.CASES]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(GOLDEN)


@pytest.mark.parametrize("case", K.CASES, ids=[c["id"] for c in K.CASES])
def test_case_gives_the_recorded_outcome(case, tmp_path):
    got = K.outcome(case, tmp_path)
    assert got == GOLDEN[case["id"]]
    if "plan" in got:           # the plan is the three resolvers' answers
        assert got["plan"] == [got["resolved"][k] for k in ("metric_levels", "msssim_scales", "frc_threshold")]


def test_each_option_is_a_key_only_when_given():
    """over the cases that main.py and eval.py accept with nothing recorded: the configuration holds exactly the flags given, plus
    the three --lr_synth_* floats once --lr_synth is"""
    seen = set()
    for c in K.CASES:
        out = GOLDEN[c["id"]]
        if c["entry"] in ("main", "eval") and not c.get("recorded") and "keys" in out:
            given = {f[2:] for f in c["argv"] if f.startswith("--") and f[2:] in K.NAMES}
            if "lr_synth" in given:
                given |= set(K.NAMES[6:])
            assert set(out["keys"]) == given, c["id"]
            seen |= given
    assert seen == set(K.NAMES)


def test_the_table():
    from dlib.utils import own_options as O
    assert tuple(o.name for o in O.OPTIONS) == K.NAMES
    assert [o.name for o in O.OPTIONS if "eval" in o.clis] == list(K.NAMES[:6]) and all("main" in o.clis for o in O.OPTIONS)
    assert {o.group for o in O.OPTIONS} == {g.name for g in O.GROUPS} == {"in_max", "metric_levels", "msssim", "frc", "lr_synth"}
    assert [r.key for r in O.RESUME] == ["metric_levels", "msssim_scales"]
    assert O.RESUME_KEYS == ("metric_levels", "msssim", "msssim_scales")


def test_the_plan_gives_the_calls_of_fast_eval():
    from dlib.utils.own_options import EvalPlan, eval_plan
    from dlib.utils.tools import Dict2Obj
    assert EvalPlan(255, 0, 0).sweep_kwargs() == {} and EvalPlan(255, 0, 0).frc_kwargs() == {}
    assert EvalPlan(255, 3, 0.25).sweep_kwargs() == {"msssim": 3} and EvalPlan(255, 3, 0.25).frc_kwargs() == {}
    assert EvalPlan(4095, 0, 0).sweep_kwargs() == {"levels": 4095} == EvalPlan(4095, 0, 0).frc_kwargs()
    assert EvalPlan(4095, 5, 0.5).sweep_kwargs() == {"levels": 4095, "msssim": 5}
    plan = eval_plan(Dict2Obj(metric_levels=4095, msssim=True, frc=True))
    assert plan == EvalPlan(4095, 5, 1.0 / 7.0)
    with pytest.raises(Exception):
        plan.levels = 255           # frozen


def test_the_module_needs_no_torch():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import dlib.utils.own_options; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code, PKG], check=True)


def _sources():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                yield os.path.relpath(os.path.join(d, f), PKG), open(os.path.join(d, f)).read()


def test_stated_once():
    """outside own_options.py no file of the package adds one of these flags, restates a range or defines a resolver (srhip/predict.py
    keeps its PredictError texts); _resume_point names none of the options; one str2bool"""
    names = "|".join(K.NAMES)
    n_str2bool = 0
    for path, txt in _sources():
        n_str2bool += len(re.findall(r"^def str2bool\(", txt, re.M))
        if path == os.path.join("dlib", "utils", "own_options.py"):
            continue
        if path != "predict.py":                 # (its --in_max is a flag of its own: the default follows the pages' dtype)
            assert not re.search(rf"add_argument\(\s*f?[\"']--({names})[\"']", txt), path
        assert not re.search(r"def check_(in_max|metric_levels|msssim|frc|lr_synth)\(", txt), path
        if path in HOST_FILES:                   # (srhip/ops.py and dlib/metrics keep the kernels' own argument rule)
            assert "1 .. 65535" not in txt and "255 .. 65535" not in txt, path
    assert n_str2bool == 1
    main = open(os.path.join(PKG, "main.py")).read()
    body = main.split("def _resume_point(args):", 1)[1].split("\ndef ", 1)[0]
    assert not re.search(names, body)
    import dlib.utils.utils_dataloaders as D
    assert not any(hasattr(D, f"check_{g}") for g in ("in_max", "metric_levels", "msssim", "frc", "lr_synth"))
