"""tests/golden/g51_imresize.npz: inputs and the REFERENCE's own ``util.imresize_np(img, scale, True)`` outputs -- the
yardstick of dlib.utils.utils_image.imresize_np and of srhip_imresize_aa (tests/test_cpu_imresize.py,
tests/test_gpu_imresize.py, which read nothing but the .npz).

Run on the build machine from the repository root (it imports the real reference through oracle/ref_shim.py; the GPU box
has none):  python tools/make_golden_imresize.py

Cases: uniform random uint8 tiles (read as np.float32(v / 255.), util.uint2single) and uniform random float32 images of
40x56, 64x64, 72x88, 36x50, 37x50, 33x47, 16x24 and 24x40 pixels at scales 1/2, 1/4 and 1/8, plus one HWC image.  Random
tiles keep the reference's output inside [0, 1] (asserted below): the dataset truncates l_im * 255 to uint8 without a
clamp, which is only defined there.  The archive is written with fixed member dates, so a second run reproduces it byte
for byte.

--hr-only-fixture additionally (re)writes tests/golden/hr_only_exp/: three synthetic 8-bit 1-channel TIFFs of 96 x 128
pixels (smooth numpy blobs plus mild noise; not taken from anywhere) under data/biosr/t/ and the folds
biosrv1-ccps-{train,val,test}-X-2 whose low-resolution keys are 'None_<i>': a set that has high-resolution images only."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SIZES = [(40, 56), (64, 64), (72, 88), (36, 50), (37, 50), (33, 47), (16, 24), (24, 40)]
SCALES = [2, 4, 8]


def main():
    import ref_shim
    ref_shim.install()
    from dlib.utils import utils_image as ref       # the reference's module

    out = {}
    rng = np.random.RandomState(51)
    for h, w in SIZES:
        u8 = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
        f32 = rng.rand(h, w).astype(np.float32)
        out[f"u8_{h}x{w}"] = u8
        out[f"f32_{h}x{w}"] = f32
        for kind, img in (("u8", np.float32(u8 / 255.)), ("f32", f32)):
            for s in SCALES:
                y = ref.imresize_np(np.copy(img), 1 / s, True)
                assert y.dtype == np.float32 and y.shape == (-(-h // s), -(-w // s)), (y.dtype, y.shape)
                assert 0.0 <= y.min() and y.max() <= 1.0, (kind, h, w, s, y.min(), y.max())
                out[f"{kind}_{h}x{w}_s{s}"] = y
    hwc = rng.rand(40, 56, 3).astype(np.float32)
    out["f32_40x56x3"] = hwc
    y = ref.imresize_np(np.copy(hwc), 1 / 2, True)
    assert y.shape == (20, 28, 3) and 0.0 <= y.min() and y.max() <= 1.0
    out["f32_40x56x3_s2"] = y

    path = os.path.join(ROOT, "tests", "golden", "g51_imresize.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    lo = min(float(v.min()) for k, v in out.items() if "_s" in k)
    hi = max(float(v.max()) for k, v in out.items() if "_s" in k)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB, reference outputs in [{lo:.3f}, {hi:.3f}]")


def hr_only_fixture():
    from PIL import Image
    fx = os.path.join(ROOT, "tests", "golden", "hr_only_exp")
    d = os.path.join(fx, "data", "biosr", "t")
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(512)
    yy, xx = np.mgrid[0:96, 0:128].astype(np.float64)
    for i in range(3):
        img = np.full((96, 128), 20.0)
        for _ in range(9):                  # smooth blobs
            cy, cx, r, a = rng.uniform(0, 96), rng.uniform(0, 128), rng.uniform(5, 16), rng.uniform(40, 150)
            img += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        img += rng.normal(0.0, 3.0, img.shape)      # mild noise
        Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8), mode="L").save(os.path.join(d, f"h_{i}.tif"))
    for split, ids in (("train", (0, 1, 2)), ("val", (0, 2)), ("test", (0, 1, 2))):
        fold = os.path.join(fx, "folds", f"biosrv1-ccps-{split}-X-2")
        os.makedirs(fold, exist_ok=True)
        with open(os.path.join(fold, "h_l.txt"), "w") as f:
            f.write("".join(f"t/h_{i}.tif,None_{i}\n" for i in ids))
        with open(os.path.join(fold, "l_h.txt"), "w") as f:
            f.write("".join(f"None_{i},t/h_{i}.tif\n" for i in ids))
    print(f"wrote {fx}")


if __name__ == "__main__":
    main()
    if "--hr-only-fixture" in sys.argv:
        hr_only_fixture()
