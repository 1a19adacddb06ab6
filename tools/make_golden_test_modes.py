"""tests/golden/g54_test_modes.npz: the REFERENCE's test modes (dlib/utils/utils_model.py:51-214: test_mode 0 .. 4) run on
the toy model of tests/test_modes_ref.py -- the yardstick of csrc/tta.hip, dlib/utils/utils_model.py and the restatement in
tests/test_modes_ref.py (tests/test_cpu_test_modes.py, tests/test_gpu_test_modes.py, which read nothing but the .npz and the
restatement).

Run on the build machine from the repository root (it imports the real reference through oracle/ref_shim.py; the GPU box
has none):  python tools/make_golden_test_modes.py

Cases (key prefix A/ ... E/; tests/test_modes_ref.CASES): shape of L, refield, min_size, sf, modulo.  Stored per case: cfg
(refield, min_size, sf, modulo), L, E0 .. E4 (the outputs of modes 0 .. 4), and tiles [n, 4] = (y0, x0, h, w) of every call
the reference's split recursion (test_split) made to a recording model, in call order: the origin is read from the image
itself (pixel value = its row-major index; replicate padding leaves the first pixel alone), the shape is what the model got.

Conditions asserted:
  * the toy model is exact whatever the order of its additions (float64 run, rounded, gives the same bits) and is not
    equivariant under any of the seven non-identity views
  * modes 3 and 4 differ from modes 0 and 2, and mode 2 from mode 0 wherever the image is split
  * exchanging the inverses of views 3 and 5 changes the result of modes 3 and 4 (the reference's `8 - i`)
  * tests/test_modes_ref.py reproduces every output of the reference bit for bit"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_utils_model():
    import ref_shim
    ref_shim.install()
    import dlib.utils.utils_image as ref_image
    # the reference's utils_model says `from utils import utils_image` (it is run from inside dlib/)
    pkg = types.ModuleType("utils")
    pkg.__path__ = []
    pkg.utils_image = ref_image
    sys.modules["utils"], sys.modules["utils.utils_image"] = pkg, ref_image
    import dlib.utils.utils_model as ref
    return ref


def main():
    import test_modes_ref as R
    ref = reference_utils_model()
    out = {}
    for name, (shape, refield, min_size, sf, modulo) in R.CASES.items():
        L = R.make_input(name)
        model = R.toy_model(sf)
        with torch.no_grad():
            y64 = R.toy_model(sf)(L.double())
            assert torch.equal(y64.float().double(), y64) and torch.equal(model(L), y64.float()), f"{name}: the toy model is not exact"
            for m in range(1, 8):
                assert not torch.equal(model(R.view(L, m)), R.view(model(L), m)), f"{name}: the toy model commutes with view {m}"
            E = [ref.test_mode(model, L, mode, refield=refield, min_size=min_size, sf=sf, modulo=modulo) for mode in range(5)]
            for mode in range(5):
                mine = R.ref_test_mode(model, L, mode, refield, min_size, sf, modulo)
                assert mine.dtype == E[mode].dtype and torch.equal(mine, E[mode]), f"{name}: the restatement of mode {mode} differs"
            for a in (3, 4):
                for b in (0, 2):
                    assert not torch.equal(E[a], E[b]), f"{name}: mode {a} equals mode {b}"
                swapped = R.ref_test_mode(model, L, a, refield, min_size, sf, modulo, inverse={m: m for m in range(8)})
                assert not torch.equal(swapped, E[a]), f"{name}: mode {a} does not see the inverses of views 3 and 5"
            # what the split hands to the model
            H, W = shape[-2:]
            calls = []

            def recorder(x):
                y0, x0 = divmod(int(x[0, 0, 0, 0]), W)
                calls.append((y0, x0) + tuple(x.shape[-2:]))
                return x.repeat_interleave(sf, dim=-2).repeat_interleave(sf, dim=-1)
            idx = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
            ref.test_mode(recorder, idx, 2, refield=refield, min_size=min_size, sf=sf, modulo=modulo)
            if len(calls) > 1:
                assert not torch.equal(E[2], E[0]), f"{name}: the split does not show"
        pre = name + "/"
        out[pre + "cfg"] = np.array([refield, min_size, sf, modulo], dtype=np.int32)
        out[pre + "L"] = L.numpy()
        for mode in range(5):
            out[pre + f"E{mode}"] = E[mode].numpy()
        out[pre + "tiles"] = np.array(calls, dtype=np.int32)
        print(f"{name}: L {tuple(shape)}, refield {refield}, min_size {min_size}, sf {sf}, modulo {modulo}: {len(calls)} tile(s) of "
              f"{calls[0][2]} x {calls[0][3]} per view; restatement == reference for modes 0 .. 4", flush=True)
    path = os.path.join(ROOT, "tests", "golden", R.GOLDEN)
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
