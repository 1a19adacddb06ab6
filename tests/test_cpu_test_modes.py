"""CPU side of the test modes (dlib/utils/utils_model.py of this package; the reference's utils_model.py:51-214): the split
plan against what the reference's recursion handed to a recording model, the plain-torch restatement of the five modes
against the reference's outputs (tests/golden/g54_test_modes.npz, written by tools/make_golden_test_modes.py), the public
surface, and the loud failure without a GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import test_modes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = R.load_golden(os.path.join(ROOT, "tests", "golden", R.GOLDEN))


@pytest.mark.parametrize("name", list(R.CASES))
def test_split_plan_is_the_reference_recursion(name):
    from dlib.utils import utils_model as um
    (_, _, H, W), refield, min_size, sf, modulo = R.CASES[name]
    assert GOLD[name]["cfg"].tolist() == [refield, min_size, sf, modulo] and GOLD[name]["L"].shape == R.CASES[name][0]
    plan = um.split_plan(H, W, refield, min_size, modulo)
    # (origin, shape) of every call of the reference's recursion, in its order
    got = [leaf["src"][:2] + leaf["pad"] for leaf in plan]
    assert got == [tuple(t) for t in GOLD[name]["tiles"].tolist()]
    levels, pad = um.split_levels(H, W, refield, min_size, modulo)
    assert len(plan) == 4 ** (len(levels) - 1) and all(leaf["src"][2:] == levels[-1] and leaf["pad"] == pad for leaf in plan)
    # the owned rectangles tile the image exactly once, each inside its leaf
    cover = np.zeros((H, W), dtype=np.int32)
    for leaf in plan:
        (sy, sx, sh, sw), (y0, x0, h, w) = leaf["src"], leaf["dst"]
        assert 0 <= sy and sy + sh <= H and 0 <= sx and sx + sw <= W
        if h and w:
            assert sy <= y0 and y0 + h <= sy + sh and sx <= x0 and x0 + w <= sx + sw
        cover[y0:y0 + h, x0:x0 + w] += 1
    assert (cover == 1).all()


def test_split_plan_shapes_named_in_the_cases():
    from dlib.utils import utils_model as um
    assert um.split_levels(21, 27, 4, 8, 1) == ([(21, 27), (12, 16), (8, 12)], (8, 12))
    assert um.split_levels(45, 53, 4, 8, 1) == ([(45, 53), (24, 28), (16, 16), (12, 12)], (12, 12))
    assert um.split_levels(5, 9, 4, 8, 4) == ([(5, 9)], (8, 12))              # the base case pads to modulo ...
    assert um.split_levels(16, 16, 4, 8, 8) == ([(16, 16), (12, 12)], (12, 12))   # ... a level that splits does not
    assert um.split_levels(53, 45, 4, 8, 1)[0] == [(w, h) for h, w in um.split_levels(45, 53, 4, 8, 1)[0]]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_reference_outputs(name):
    _, refield, min_size, sf, modulo = R.CASES[name]
    L = torch.from_numpy(GOLD[name]["L"])
    assert torch.equal(L, R.make_input(name))
    for mode in range(5):
        E = R.ref_test_mode(R.toy_model(sf), L, mode, refield, min_size, sf, modulo)
        assert np.array_equal(E.numpy(), GOLD[name][f"E{mode}"]), (name, mode)
    # the goldens tell the modes apart, and pin which of views 3 and 5 undoes which
    for a in (3, 4):
        assert not np.array_equal(GOLD[name][f"E{a}"], GOLD[name]["E0"]) and not np.array_equal(GOLD[name][f"E{a}"], GOLD[name]["E2"])
        swapped = R.ref_test_mode(R.toy_model(sf), L, a, refield, min_size, sf, modulo, inverse={m: m for m in range(8)})
        assert not np.array_equal(swapped.numpy(), GOLD[name][f"E{a}"])


def test_a_side_shorter_than_its_quadrant_raises():
    from dlib.utils import utils_model as um
    # 6 x 40, refield 4, min_size 4: the level splits (240 > 16) and the height's quadrant is (6 // 2 // 4 + 1) * 4 = 4 <= 6,
    # fine; with refield 8 it is 8 > 6: the reference's slice(6 - 8, 6) would wrap around
    um.split_plan(6, 40, 4, 4, 1)
    with pytest.raises(ValueError, match="height"):
        um.split_plan(6, 40, 8, 4, 1)
    with pytest.raises(ValueError, match="width"):
        um.split_plan(40, 6, 8, 4, 1)
    with pytest.raises(ValueError, match="height"):
        um.split_levels(6, 40, 8, 4, 1)


def test_public_surface_has_the_reference_signatures():
    from dlib.utils import utils_model as um
    from dlib.models.model_plain import ModelPlain

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    extra = [("max_batch", 8)]
    assert params(um.test_mode) == [("model", E), ("L", E), ("mode", 0), ("refield", 32), ("min_size", 256), ("sf", 1),
                                    ("modulo", 1)] + extra
    assert params(um.test) == [("model", E), ("L", E)]
    assert params(um.test_pad) == [("model", E), ("L", E), ("modulo", 16), ("sf", 1)] + extra
    assert params(um.test_split) == [("model", E), ("L", E), ("refield", 32), ("min_size", 256), ("sf", 1), ("modulo", 1)] + extra
    assert params(um.test_x8) == [("model", E), ("L", E), ("modulo", 1), ("sf", 1)] + extra
    assert params(um.test_split_x8) == [("model", E), ("L", E), ("refield", 32), ("min_size", 256), ("sf", 1), ("modulo", 1)] + extra
    assert params(um.split_plan) == [("h", E), ("w", E), ("refield", 32), ("min_size", 256), ("modulo", 1)]
    assert params(ModelPlain.testx8) == [("self", E)]
    assert params(ModelPlain.test_tta) == [("self", E), ("mode", E), ("refield", 32), ("min_size", 256), ("modulo", 1)]


def test_library_exports_the_two_entry_points(tmp_path):
    from srhip import _lib, ops
    protos = _lib.parse_header()
    assert protos["srhip_view_gather"] == ("i", "piiippipiip") and protos["srhip_view_merge"] == ("i", "ppipiiiip")
    assert hasattr(_lib.lib, "srhip_view_gather") and hasattr(_lib.lib, "srhip_view_merge")
    # the tables ops.py builds are laid out as the header declares them
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(srhip_view_job), offsetof(srhip_view_job, mode), '
                   'sizeof(srhip_view_desc), offsetof(srhip_view_desc, w));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ops._ViewJob), ops._ViewJob.mode.offset, ctypes.sizeof(ops._ViewDesc), ops._ViewDesc.w.offset]


@pytest.mark.parametrize("mode", range(5))
def test_a_cpu_tensor_raises_gpu_only(mode):
    from dlib.utils import utils_model as um
    with pytest.raises(RuntimeError, match="GPU only"):
        um.test_mode(R.toy_model(2), torch.zeros(1, 1, 16, 16), mode, refield=4, min_size=8, sf=2, modulo=1)


def test_the_kernel_wrappers_raise_on_cpu_tensors():
    from srhip import ops
    with pytest.raises(ops.SrhipError, match="GPU only"):
        ops.view_gather(torch.zeros(2, 5, 9), [(0, 0, 5, 9, 0)], 8, 12)
    with pytest.raises(ops.SrhipError, match="GPU only"):
        ops.view_merge([(torch.zeros(1, 2, 8, 12), 0, 8, 12, [(5, 9)])], 2, 5, 9, 1)
