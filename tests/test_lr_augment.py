"""--da_device, the host side: the numpy statement of srhip_lr_augment (lr_augment_ref.py) against the reference's functions
(lowres.da_*, pinned to the reference by g31) and against scipy, the frequencies of its decisions, the case selection the GPU
file relies on, the option and the set's refusals."""
import numpy as np
import pytest

import lr_augment_ref as R
import philox_ref as PR


class Scripted:
    """np.random's five functions as the reference's augmentations call them, answering with the statement's own draws in the
    reference's order (u_apply; z, ch, cw; then u_side, the mask or the noise) and checking what they are asked for."""

    def __init__(self, answers):
        self.answers = list(answers)

    def take(self, kind):
        k, v = self.answers.pop(0)
        assert k == kind, (k, kind)
        return v

    def rand(self, n):
        assert n == 1
        return np.array([self.take("rand")])

    def randn(self):
        return self.take("randn")

    def randint(self, lo, hi):
        v, want_hi = self.take("randint")
        assert (lo, int(hi)) == (0, want_hi), (lo, hi, want_hi)         # the statement's block side is the reference's
        return v

    def binomial(self, n, p, size):
        mask, p_keep = self.take("binomial")
        assert n == 1 and p == p_keep and tuple(int(s) for s in size) == mask.shape + (1,)
        return mask.astype(np.int64)[:, :, None]

    def normal(self, loc, scale, size):
        noise, std = self.take("normal")
        assert loc == 0.0 and scale == std and tuple(int(s) for s in size) == noise.shape + (1,)
        return noise[:, :, None]


def script_of(seed, b, h, w, params):
    """the draws the reference's functions consume for sample b, taken from the statement; None when a ratio leaves [0, 1]
    (the reference raises there: the clamp is the statement's documented difference)"""
    out = []
    for s, (on, prob, area, value) in enumerate(params):
        if not on or area == 0:
            continue
        (applied, ch, cw, bh, bw, inside), raw = R.decide(seed, b, s, h, w, prob, area)
        out.append(("rand", raw["u_apply"]))
        if not applied:
            continue
        if not 0.0 <= raw["ratio"] <= 1.0:
            return None
        out += [("randn", raw["z"]), ("randint", (ch, h - bh + 1)), ("randint", (cw, w - bw + 1))]
        if s == 0:
            out.append(("rand", raw["u_side"]))
        elif s == 1:
            out.append(("binomial", (R.pixel_draws(seed, b, h, w, 1, ch, cw, bh, bw, value), 1. - value)))
        else:
            out.append(("normal", (R.pixel_draws(seed, b, h, w, 2, ch, cw, bh, bw, value), value)))
    return out


def test_case_selection_every_decision_is_cut_away_from_its_threshold():
    """every case of the shared list keeps h ratio, w ratio, u_ch (h - bh + 1), u_cw (w - bw + 1) at least 1e-9 away from an
    integer and u_apply, u_side at least 1e-9 away from their thresholds: a last-bit difference of the device's log / cos
    cannot move a decision, so the GPU file compares decisions exactly and skips nothing"""
    cases = R.cases()
    assert len(cases) == len(R.SHAPES) * len(R.MODES) * len(R.VALUES)
    assert len({c[5] for c in cases}) == len(cases) and all(c[5] >> 32 and c[5] & PR.MASK32 for c in cases)
    applied = 0
    for k, (name, B, h, w, params, seed) in enumerate(cases):
        x, want, decs, m = R.case_reference(k)
        assert m >= 1e-9, (name, m)
        applied += sum(d[0] for per in decs for d in per)
    assert applied > len(cases)           # the list is not a list of skipped stages


def test_blur_restated_pass_by_pass_is_scipy_bit_for_bit():
    """the order the kernel sums in -- rows axis, columns axis, the channel axis of length 1; the centre tap, then the pairs
    from the farthest inwards; 'reflect' for a radius beyond the patch -- gives scipy.ndimage.gaussian_filter's bits"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(4)
    for (h, w, sigma) in ((8, 8, 1.0), (8, 8, 2.0), (5, 7, 3.0), (3, 4, 6.0), (32, 32, 1.3), (64, 64, 1.0), (16, 12, 1.0)):
        img = rng.random((h, w), dtype=np.float32)
        assert np.array_equal(R.blur_passes(img, sigma), gaussian_filter(input=img[:, :, None], sigma=sigma)[:, :, 0]), (h, w, sigma)
        wt = R.blur_weights(sigma)
        assert len(wt) == 2 * int(4 * sigma + 0.5) + 1 and np.array_equal(wt, wt[::-1])


def test_statement_follows_the_reference_functions(monkeypatch):
    """with np.random scripted to return the statement's draws, lowres.apply_lr_augmentations (the reference's functions, g31)
    gives the statement's bits on every case whose ratios lie in [0, 1]"""
    from types import SimpleNamespace
    from dlib.datasets import lowres as L
    checked = 0
    for k, (name, B, h, w, params, seed) in enumerate(R.cases()):
        x, want, decs, _ = R.case_reference(k)
        (b_on, b_prob, b_area, sigma), (d_on, d_prob, d_area, p), (g_on, g_prob, g_area, std) = params
        args = SimpleNamespace(da_blur=b_on, da_blur_prob=b_prob, da_blur_area=b_area, da_blur_sigma=sigma,
                               da_dot_bin_noise=d_on, da_dot_bin_noise_prob=d_prob, da_dot_bin_noise_area=d_area,
                               da_dot_bin_noise_p=p, da_add_gaus_noise=g_on, da_add_gaus_noise_prob=g_prob,
                               da_add_gaus_noise_area=g_area, da_add_gaus_noise_std=std)
        for b in range(B):
            script = script_of(seed, b, h, w, params)
            if script is None:
                continue
            s = Scripted(script)
            for fn in ("rand", "randn", "randint", "binomial", "normal"):
                monkeypatch.setattr(np.random, fn, getattr(s, fn))
            got = L.apply_lr_augmentations(np.ascontiguousarray(x[b].transpose(1, 2, 0)).copy(), args)
            monkeypatch.undo()
            assert not s.answers, (name, b)
            assert got.dtype == np.float32 and np.array_equal(got[:, :, 0], want[b, 0]), (name, b)
            checked += 1
    assert checked > 200


def test_decision_and_mask_frequencies():
    """over 4096 (seed, sample) pairs: applied against prob, inside against 0.02, a mask's kept share against 1 - p, each
    within 4 standard deviations of a 4096-draw frequency"""
    n = 4096
    pairs = [(((i // 4 + 1) * 0xD1B54A32D192ED03) & 0x7FFFFFFFFFFFFFFF, i % 4) for i in range(n)]

    def within(count, q):
        return abs(count / n - q) <= 4 * np.sqrt(q * (1 - q) / n)
    for prob in (0.5, 0.3):
        assert within(sum(R.decide(sd, b, 1, 16, 12, prob, 0.3)[0][0] for sd, b in pairs), prob)
    assert within(sum(R.decide(sd, b, 0, 16, 12, 1.0, 0.3)[0][5] for sd, b in pairs), 0.02)
    for p in (0.5, 0.3, 0.999):
        kept = PR.words(pairs[7][0], 1, 4 * 5 * 7, n) >= np.uint64(PR.threshold(p)[0])      # 4096 pixels of one mask
        assert within(int(kept.sum()), 1 - p)
        first = [bool(PR.words(sd, 1, b * 35, 1)[0] >= np.uint64(PR.threshold(p)[0])) for sd, b in pairs]
        assert within(sum(first), 1 - p)                                                  # and one pixel over the pairs


def test_main_parses_da_device():
    import main as M
    base = ["--net_type", "swinir", "--da_blur", "True"]
    assert M.get_config("swinir")["da_device"] is False
    assert M.parse_input(base)["da_device"] is False
    cfg = M.parse_input(base + ["--da_device", "True"])
    assert cfg["da_device"] is True and cfg["da_blur"] is True


def _args(**kw):
    from types import SimpleNamespace
    a = dict(scale=8, h_size=64, batch_size=2, myseed=3, da_device=True,
             da_blur=True, da_blur_prob=0.5, da_blur_area=0.3, da_blur_sigma=1.,
             da_dot_bin_noise=True, da_dot_bin_noise_prob=0.5, da_dot_bin_noise_area=0.3, da_dot_bin_noise_p=0.5,
             da_add_gaus_noise=True, da_add_gaus_noise_prob=0.5, da_add_gaus_noise_area=0.3, da_add_gaus_noise_std=0.03)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("name,value", [
    ("da_blur_sigma", 16.2), ("da_blur_sigma", 0.0), ("da_blur_sigma", -1.0), ("da_blur_prob", 1.5), ("da_blur_area", -0.1),
    ("da_dot_bin_noise_prob", -0.5), ("da_dot_bin_noise_area", 1.01), ("da_dot_bin_noise_p", 1.0), ("da_dot_bin_noise_p", -0.1),
    ("da_add_gaus_noise_prob", 2.0), ("da_add_gaus_noise_area", -1.0), ("da_add_gaus_noise_std", -0.03)])
def test_resident_train_set_refuses_bad_device_augmentation_parameters_by_name(name, value):
    """when the set is built, before a tile is read or a kernel launched: a blur radius above 64 (sigma 16.2: int(65.3)),
    prob / area outside [0, 1], p outside [0, 1), a negative std or sigma, sigma 0"""
    from dlib.datasets.dataset_dpsr import ResidentTrainSet, check_da_device
    with pytest.raises(ValueError, match=name):
        ResidentTrainSet(_args(**{name: value}), {}, {}, "cpu")
    # the same value on the host path, or with its stage off, is not this check's business
    stage = name.rsplit("_", 1)[0]
    assert check_da_device(_args(**{name: value, stage: False}))[("da_blur", "da_dot_bin_noise", "da_add_gaus_noise").index(stage)] \
        == (False, 0., 0., 0.)


def test_device_augmentation_parameters_as_the_op_takes_them():
    from dlib.datasets.dataset_dpsr import check_da_device
    assert check_da_device(_args()) == ((True, 0.5, 0.3, 1.), (True, 0.5, 0.3, 0.5), (True, 0.5, 0.3, 0.03))
    assert check_da_device(_args(da_blur_sigma=16.0))[0] == (True, 0.5, 0.3, 16.0)       # radius int(64.5) = 64: the last accepted
    assert check_da_device(_args(da_blur=False, da_add_gaus_noise=False)) == ((False, 0., 0., 0.), (True, 0.5, 0.3, 0.5),
                                                                              (False, 0., 0., 0.))
