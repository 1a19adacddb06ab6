"""The shapes of tests/launch_plan_cases.py lie on the intended side of the boundaries they were chosen against (no GPU).

Every constant is read back out of the source that defines it, so a later change of a chunk size, a grid cap or bn_plan
fails here instead of leaving tests/test_gpu_launch_plans.py to cover first chunks only."""
import os
import re

import numpy as np
import pytest

import launch_plan_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sr-caco-2_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name) if name.endswith((".hip", ".h")) else os.path.join(ROOT, "sr-caco-2_amd", name)) as f:
        return f.read()


def constant(name, const):
    m = re.findall(r"constexpr\s+(?:int|long)\s+%s\s*=\s*(\d+)\s*;" % re.escape(const), source(name))
    assert len(m) == 1, (name, const, m)
    return int(m[0])


def cdiv(a, b):
    return (a + b - 1) // b


def test_the_constants_are_the_sources():
    assert constant("edt.hip", "EDT_CHUNK") == L.EDT_CHUNK
    assert constant("bn.hip", "BN_MAXBLK") == L.BN_MAXBLK
    assert constant("lr_synth.hip", "NOISE_CHUNK") == L.NOISE_CHUNK
    assert constant("data.hip", "MAXJOBS") == L.MAXJOBS
    assert constant("gemm_tnb.hip", "TNB_BATCH_MAX") == L.TNB_BATCH_MAX
    assert constant("gemm_tnb.hip", "TNB_GROUP_MAX") == L.TNB_GROUP_MAX
    # the dropout grid: blocks of 256 four-element groups, capped
    d = source("dropout.hip")
    cap, = re.findall(r"gb < (\d+) \? gb : (\d+)", d)
    assert int(cap[0]) == int(cap[1]) == L.DROPOUT_GRID_CAP
    assert re.search(r"gb = \(ngroups \+ 255\) / 256;", d) and re.search(r"ngroups = \(n \+ 3\) >> 2;", d)
    assert re.search(r"dim3\(grid\), dim3\(%d\)" % L.DROPOUT_BLOCK, d)
    # the sweep of the BatchNorm kernels: both walk their rows 16 at a time, bn_plan never goes below it
    b = source("bn.hip")
    assert len(re.findall(r"r < r1; r \+= (\d+)\)", b)) == 2 and set(re.findall(r"r < r1; r \+= (\d+)\)", b)) == {str(L.BN_SWEEP)}
    assert re.search(r"if \(p\.rpb < %d\) p\.rpb = %d;" % (L.BN_SWEEP, L.BN_SWEEP), b)
    # the wrapper that splits walks in steps of the library's bound
    o = source(os.path.join("srhip", "ops.py"))
    body = o[o.index("def conv3x3_wgrad_batched("):o.index("# ------------------------------------------------------------------ weight prep")]
    assert re.findall(r"range\(0, len\(items\), (\d+)\)", body) == [str(L.TNB_BATCH_MAX)]
    assert re.findall(r"items\[j0:j0 \+ (\d+)\]", body) == [str(L.TNB_BATCH_MAX)]
    # the survey's caps
    e = source("edt.hip")
    assert re.search(r"g = \(n \+ 256 \* 16 - 1\) / \(256 \* 16\);\s*if \(g > (\d+)\) g = \1;", e).group(1) == str(L.HIST_GRID_CAP)
    assert L.HIST_PER_BLOCK == 256 * 16
    r = source("resize.hip")
    assert re.search(r"g = \(n \+ 255\) / 256;\s*return \(int\)\(g > (\d+) \? \1 :", r).group(1) == str(L.RS_GRID_CAP)
    g = re.findall(r"gx = sr_cdiv\(\(long\)P \* P, 256\) < (\d+) \? sr_cdiv\(\(long\)P \* P, 256\) : (\d+);", source("data.hip"))
    assert len(g) == 3 and set(g) == {(str(L.GATHER_GX_CAP),) * 2}


def test_bn_plan_restated_is_the_source_formula():
    """bn_plan of launch_plan_cases against the lines of bn.hip it restates, and on hand-computed plans"""
    b = source("bn.hip")
    for line in ("p.Wd = C == 1 ? 64 : C;", "p.rows = (n + p.Wd - 1) / p.Wd;", "p.ncg = p.Wd / 64;",
                 "const long maxblk = BN_MAXBLK / p.ncg > 0 ? BN_MAXBLK / p.ncg : 1;", "p.rpb = (p.rows + maxblk - 1) / maxblk;",
                 "p.nblk = (int)((p.rows + p.rpb - 1) / p.rpb);"):
        assert line in b, line
    assert L.bn_plan(2 * 24 * 20, 64) == (64, 960, 1, 60, 16)
    assert L.bn_plan(2046, 448) == (448, 2046, 7, 128, 16)                # the largest the older test reaches: 16 rows a block
    assert L.bn_plan(16 * 2048, 64)[4] == 16 and L.bn_plan(16 * 2048 + 1, 64)[4] == 17
    assert L.bn_plan(16 * 292, 448)[4] == 16 and L.bn_plan(16 * 292 + 1, 448)[4] == 17
    assert L.bn_plan(5 * 13, 1) == (64, 2, 1, 1, 16)


def test_edt_cases_cross_the_chunk():
    for H, W, chunks in L.EDT_CASES:
        assert cdiv(W, L.EDT_CHUNK) == chunks and W <= 16384, (H, W)
    widths = [W for _, W, _ in L.EDT_CASES]
    assert L.EDT_CHUNK in widths and L.EDT_CHUNK + 1 in widths          # both sides of the boundary, next to it
    assert sum(W > L.EDT_CHUNK for W in widths) >= 4 and max(cdiv(W, L.EDT_CHUNK) for W in widths) >= 3
    assert any((W - L.EDT_CHUNK) % 4 for W in widths if W > L.EDT_CHUNK)          # a last chunk the sentinel pads
    assert any((W - L.EDT_CHUNK) % 4 == 0 for W in widths if W > L.EDT_CHUNK)     # and one it does not
    for H, W, chunks in L.EDT_CASES:
        if chunks > 1:
            x = L.edt_extra_foregrounds(H, W)
            last, first, none = (x[k] for k in x)
            assert (~last).sum() == 1 and not last[0, W - 1] and (~first).sum() == 1 and not first[H // 2, 0] and none.all()


def test_bn_cases_walk_more_than_one_sweep():
    rpbs = []
    for T, C in L.BN_CASES:
        Wd, rows, ncg, nblk, rpb = L.bn_plan(T, C)
        assert rpb > L.BN_SWEEP and nblk > 1 and nblk * ncg <= L.BN_MAXBLK, (T, C, rpb, nblk)
        assert (nblk - 1) * rpb < rows <= nblk * rpb
        rpbs.append(rpb)
    assert any(r % L.BN_SWEEP for r in rpbs) and any(r % L.BN_SWEEP == 0 for r in rpbs), rpbs
    assert any(r % 4 for r in rpbs), rpbs                                 # a wave's last four-row pass is ragged too
    ragged = [(T, C) for T, C in L.BN_CASES if C == 1 and T % 64]
    assert ragged, "a C = 1 case whose last pseudo-row is ragged"
    assert {C for _, C in L.BN_CASES} >= {1, 64, 448}                     # one and seven column groups, the pixel rows


def test_noise_cases_cross_the_chunk():
    assert L.NOISE_CHUNK in L.NOISE_B and L.NOISE_CHUNK + 1 in L.NOISE_B and max(L.NOISE_B) > 2 * L.NOISE_CHUNK
    assert L.NOISE_CHUNK % 32 == 0                                        # 1023 is the last bit of a mask word
    for B in L.NOISE_B:
        masks = L.noise_masks(B)
        assert masks["all"] is None
        if B > L.NOISE_CHUNK:
            only = masks["only 1024"]
            assert len(only) == B and sum(only) == 1 and only[L.NOISE_CHUNK] and not any(only[:L.NOISE_CHUNK])
        if B > L.NOISE_CHUNK + 1:
            m = masks["1023 and 1025"]
            assert len(m) == B and sum(m) == 2 and m[L.NOISE_CHUNK - 1] and m[L.NOISE_CHUNK + 1] and not m[L.NOISE_CHUNK]
        for h, w in L.NOISE_HW:
            x = L.noise_input(B, h, w)
            assert x.dtype == np.float32 and x.shape == (B, 1, h, w) and x.min() == 0.0 and x.max() == 1.0
            if B > L.NOISE_CHUNK:       # no sample of a later launch repeats the sample a restarted counter would pair it with
                assert all(not np.array_equal(x[b], x[b - L.NOISE_CHUNK]) for b in range(L.NOISE_CHUNK, B))
            lam = 200.0 * x.astype(np.float64)
            assert ((lam > 0) & (lam < 30)).any() and (lam >= 30).any()
    assert {p for p, _ in L.NOISE_SETTINGS} == {0.5, 200.0} and {r for _, r in L.NOISE_SETTINGS} == {0.0, 2.5}
    assert len(L.NOISE_SETTINGS) == 4


def test_gather_cases_cross_the_chunk():
    assert L.MAXJOBS in L.GATHER_JOBS and L.MAXJOBS + 1 in L.GATHER_JOBS and max(L.GATHER_JOBS) > 2 * L.MAXJOBS
    assert len(set(L.GATHER_TILES)) == 2
    for P in L.GATHER_P:
        for n in L.GATHER_JOBS:
            ids, y0, x0, modes = L.gather_jobs(L.GATHER_TILES, P, n)
            jobs = list(zip(ids, y0, x0, modes))
            assert len(jobs) == n and set(modes) == set(range(8)) and set(ids) == {0, 1}
            for i, y, x, m in jobs:
                H, W = L.GATHER_TILES[i]
                assert 0 <= y <= H - P and 0 <= x <= W - P
            corners = {(i, cy * (H - P), cx * (W - P), m) for i, (H, W) in enumerate(L.GATHER_TILES) for m in range(8)
                       for cy in (0, 1) for cx in (0, 1)}
            assert corners <= set(jobs)
            for b in range(L.MAXJOBS, n):                                 # what `jobs[b]` in place of `jobs[b0 + b]` would read
                assert jobs[b] != jobs[b % L.MAXJOBS], (P, n, b)
    assert L.GATHER_BIG_P ** 2 > L.GATHER_GX_CAP * 256 and (L.GATHER_BIG_P - 8) ** 2 <= L.GATHER_GX_CAP * 256


def test_dropout_case_is_past_the_cap_and_its_parts_are_not():
    assert L.DROPOUT_PASS == 8388608 and L.DROPOUT_N == 8388608 + 4 * 256 * 3 + 5
    blocks = lambda n: cdiv(cdiv(n, 4), L.DROPOUT_BLOCK)
    assert blocks(L.DROPOUT_N) > L.DROPOUT_GRID_CAP and L.DROPOUT_N % 4
    s = L.DROPOUT_SPLITS
    assert s[0] == 0 and s[-1] == L.DROPOUT_N and len(s) == 4
    for a, b in zip(s, s[1:]):
        assert a % 4 == 0 and 0 < b - a and blocks(b - a) <= L.DROPOUT_GRID_CAP
    assert (1 << 20) + 5 < L.DROPOUT_PASS                                 # the older test's largest n: one pass


def test_wrapper_cases_need_more_than_one_launch():
    assert [cdiv(n, L.TNB_BATCH_MAX) for n in L.CONV_BATCHED_N] == [2, 3] and all(n % L.TNB_BATCH_MAX == 1 for n in L.CONV_BATCHED_N)
    assert [cdiv(n, L.TNB_GROUP_MAX) for n in L.LINEAR_GROUPED_N] == [2, 3] and all(n % L.TNB_GROUP_MAX == 1 for n in L.LINEAR_GROUPED_N)
    assert L.CONV_BATCHED_SHAPE[3] >= 64                                  # the bf16x3 kernels' channel floor


def test_survey_cases_are_past_their_caps():
    assert cdiv(L.HIST_N, L.HIST_PER_BLOCK) > L.HIST_GRID_CAP and L.HIST_N < 1 << 31
    assert cdiv(L.RS_N, 256) > L.RS_GRID_CAP
    for name in ("omni_ops.hip", "act_ops.hip", "grl_ops.hip"):
        cap, = re.findall(r"inline int ew_blocks\(long n\) \{ const long g = \(n \+ 255\) / 256; return \(int\)\(g < (\d+) \? g : (\d+)\); \}",
                          source(name))
        assert cap == (str(L.EW_GRID_CAP),) * 2, name
    assert L.EW_N > L.EW_PASS and L.EW_PERIODIC[0] * L.EW_PERIODIC[1] > L.EW_PASS
    B, H, W, C = L.POOL_SHAPE
    assert B * ((H - 3) // 2 + 1) * ((W - 3) // 2 + 1) * C > L.EW_PASS and B * (H // 2) * (W // 2) * C > L.EW_PASS
    B, H, W, C, Ho, Wo = L.BILINEAR_CASE
    assert B * Ho * Wo * C > L.EW_PASS
    B, H, W, C = L.DWCONV_SCALAR_SHAPE
    assert C % 4 and B * H * W * C > L.EW_PASS
    B, H, W, C, k, s = L.UNFOLD_CASE
    assert B * H * W * C > L.EW_PASS and (H - k) % s == 0 and (W - k) % s == 0         # fold's items; unfold has k k / s s as many
    assert constant("dsr_splines.hip", "DS_GMAX") == L.DS_GMAX and constant("dsr_splines.hip", "DS_NB") == L.DS_NB
    d = source("dsr_splines.hip")
    assert "long G = 1024 / n_splines;" in d and "if (G > DS_GMAX) G = DS_GMAX;" in d and "b0 < hi; b0 += DS_NB)" in d
    for n, shape in L.DS_CASES:          # whatever the deal: the shares of all workgroups together are too small at one batch each
        assert int(np.prod(shape)) > L.DS_NB * n * min(1024 // n, L.DS_GMAX), (n, shape)
    d = source("data.hip")
    assert len(re.findall(r"if \(g > 16384\) g = 16384;", d)) == 2 and "long g = ((n + 3) / 4 + 255) / 256;" in d
    assert L.LEVELS_N > L.LEVELS_PASS >= max(L.LEVELS_SPLIT, L.LEVELS_N - L.LEVELS_SPLIT) and L.LEVELS_SPLIT % 8 == 0
    B, H, W, ks, ldo = L.IM2COL_CASE
    assert B * H * W * ldo > 16384 * 256 and ks * ks <= ldo and ldo % 4 == 0
    heads, N1, N2, entries = L.CPB_CASE
    assert heads * N1 * N2 > L.EW_PASS >= heads * cdiv(N1, 2) * N2


@pytest.mark.parametrize("name", ["augment.hip", "tta.hip", "io.hip"])
def test_files_the_survey_found_uncapped_still_are(name):
    """the survey of test_gpu_launch_plans.py lists these as launching one thread (or one tile) per item, with no capped grid
    and no host loop: a grid-stride loop or a chunk constant appearing there asks for a case"""
    s = source(name)
    assert not re.search(r"\+=\s*(\(long\)\s*)?gridDim", s) and not re.search(r"for \(int \w*0 = 0; \w*0 < \w+; \w*0 \+= [A-Z_]+\)\s*\{\s*const int nb", s)
