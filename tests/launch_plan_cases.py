"""Shapes at which an entry point of libsrhip leaves its first chunk: a host loop that launches in chunks, a grid capped so
that the kernel walks with a stride, rows-per-block above the minimum, a row staged through LDS in pieces.

tests/test_gpu_launch_plans.py runs the kernels at these shapes; tests/test_cpu_launch_plans.py reads the constants back
out of the sources and checks that every shape lies on the side of its boundary that its comment names -- so raising a
chunk size fails there instead of quietly turning the GPU tests into first-chunk tests.  Both import the shapes from here.

The constants below are what the shapes were chosen against; nothing but test_cpu_launch_plans.py may rely on them."""
import numpy as np

# ---------------------------------------------------------------- srhip_edt_sq: k_edt_rows stages EDT_CHUNK ints of a row
EDT_CHUNK = 4096
# (H, W, chunks of the row walk): 4096 is the last one-chunk width; 4097 a chunk of one int (padded to four by the sentinel);
# 4100 a chunk of exactly four; 8193 three chunks; 4099 a ragged chunk on five rows
EDT_CASES = ((3, 4096, 1), (2, 4097, 2), (3, 4100, 2), (2, 8193, 3), (5, 4099, 2))


def edt_extra_foregrounds(H, W):
    """three images on top of the foregrounds() family of tests/test_gpu_edt_sampler.py: the only background pixel in the
    last column / in column 0 (the nearest background pixel of most output pixels lies in another chunk, in either direction),
    and none at all"""
    last = np.ones((H, W), bool)
    last[0, W - 1] = False
    first = np.ones((H, W), bool)
    first[H // 2, 0] = False
    return {"only background pixel in the last column": last, "only background pixel in column 0": first,
            "no background pixel": np.ones((H, W), bool)}


# ---------------------------------------------------------------- srhip_bn_*: bn_plan's rows per block
BN_MAXBLK = 2048
BN_SWEEP = 16          # rows one sweep of a block's four waves covers (r += 16, four rows a wave)
# (T, C): rpb 20, 18, 17 (C = 1: rows of 64 pixels, the last one ragged) and 32 (a whole number of sweeps above one)
BN_CASES = ((40000, 64), (5000, 448), (64 * 33000 + 17, 1), (65000, 64))


def bn_plan(T, C, maxblk=BN_MAXBLK):
    """bn_plan of csrc/bn.hip: (row width, rows, column groups, blocks, rows per block)"""
    Wd = 64 if C == 1 else C
    rows = (T * C + Wd - 1) // Wd
    ncg = Wd // 64
    mb = max(maxblk // ncg, 1)
    rpb = max((rows + mb - 1) // mb, BN_SWEEP)
    return Wd, rows, ncg, (rows + rpb - 1) // rpb, rpb


# ---------------------------------------------------------------- srhip_photon_noise: NOISE_CHUNK samples a launch
NOISE_CHUNK = 1024
NOISE_B = (1024, 1025, 2050)               # the last one-launch batch, a launch of one sample, three launches
NOISE_HW = ((1, 3), (2, 2))
NOISE_SETTINGS = ((0.5, 0.0), (0.5, 2.5), (200.0, 0.0), (200.0, 2.5))       # (photons, read_std): both Poisson samplers


def noise_masks(B):
    """the `on` arguments of a batch of B: absent; only sample 1024 (the first launch has nothing to do, the second one bit);
    1023 and 1025 with 1024 clear (the last bit of one mask word, bits 1 and 0 of the next launch's first)"""
    masks = {"all": None}
    if B > 1024:
        masks["only 1024"] = [b == 1024 for b in range(B)]
    if B > 1025:
        masks["1023 and 1025"] = [b in (1023, 1025) for b in range(B)]
    return masks


def noise_input(B, h, w):
    """float32 [B, 1, h, w] in [0, 1], every sample its own values (a counter that restarts per launch would pair sample
    1024 + j with the noise of sample j), exact 0 and 1 present, both sides of lambda = 30 at 200 photons"""
    rng = np.random.default_rng(1000 * B + 10 * h + w)
    x = rng.random((B, 1, h, w), dtype=np.float32)
    x[::7, 0, 0, 0] = 0.0
    x[3::7, 0, h - 1, w - 1] = 1.0
    x[5::7, 0, 0, w - 1] *= np.float32(0.1)
    return x


# ---------------------------------------------------------------- srhip_patch_gather / _f32: MAXJOBS jobs a launch
MAXJOBS = 64
GATHER_JOBS = (64, 65, 130)                # the last one-launch batch, a launch of one job, three launches
GATHER_TILES = ((19, 23), (16, 16))
GATHER_P = (8, 5)


def gather_jobs(shapes, P, n):
    """n jobs over tiles of `shapes`: every mode at every corner of both tiles (64 jobs), then random origins and modes; past
    64 the list is rotated by three so that launches begin and end inside both kinds.  Job 64 + b never equals job b."""
    rng = np.random.RandomState(100 * P + n)
    jobs = []
    for i, (H, W) in enumerate(shapes):
        for m in range(8):
            for (cy, cx) in ((0, 0), (0, 1), (1, 0), (1, 1)):
                jobs.append((i, cy * (H - P), cx * (W - P), m))
    jobs = jobs[:n]
    while len(jobs) < n:
        i = int(rng.randint(len(shapes)))
        jobs.append((i, int(rng.randint(0, shapes[i][0] - P + 1)), int(rng.randint(0, shapes[i][1] - P + 1)), int(rng.randint(8))))
    if n > MAXJOBS:
        jobs = jobs[3:] + jobs[:3]
    ids, y0, x0, modes = (list(v) for v in zip(*jobs))
    return ids, y0, x0, modes


# ---------------------------------------------------------------- srhip_dropout: 8192 blocks of 256 four-element groups
DROPOUT_GRID_CAP, DROPOUT_BLOCK = 8192, 256
DROPOUT_PASS = DROPOUT_GRID_CAP * DROPOUT_BLOCK * 4        # elements one pass of the capped grid covers
DROPOUT_N = DROPOUT_PASS + 4 * 256 * 3 + 5                 # three more blocks' worth of groups and a ragged last group
DROPOUT_P = 0.25
DROPOUT_SPLITS = (0, 2796204, 5592408, DROPOUT_N)          # three consecutive sub-ranges, each one pass, offsets multiples of 4

# ---------------------------------------------------------------- the Python wrappers over a bounded launch
TNB_BATCH_MAX = 40                         # ops.conv3x3_wgrad_batched splits a longer list
CONV_BATCHED_N = (41, 81)                  # two launches (40 + 1), three (40 + 40 + 1)
CONV_BATCHED_SHAPE = (1, 9, 7, 128)        # B, H, W, C: the smallest of test_conv_wgrad_batched_matches_float64
TNB_GROUP_MAX = 24                         # ops.linear_wgrad_grouped hands a longer list to the library, which refuses it
LINEAR_GROUPED_N = (25, 49)

# ---------------------------------------------------------------- the survey's own cases (see test_gpu_launch_plans.py)
HIST_GRID_CAP, HIST_PER_BLOCK = 1024, 256 * 16
HIST_N = HIST_GRID_CAP * HIST_PER_BLOCK + 77               # one block more than the cap would hold
RS_GRID_CAP = 8192                                         # resize.hip: rs_grid, blocks of 256 one-element threads
RS_N = RS_GRID_CAP * 256 + 77
GATHER_GX_CAP = 64                                         # data.hip: blocks of 256 pixels per patch
GATHER_BIG_P = 136                                         # 136^2 = 18496 pixels > 64 * 256: a thread takes a second pixel
EW_GRID_CAP = 16384                                        # omni_ops.hip / act_ops.hip / grl_ops.hip: ew_blocks, blocks of 256
EW_PASS = EW_GRID_CAP * 256                                # items one pass of that grid covers
EW_N = EW_PASS + 77
EW_PERIODIC = (4093, 1025)                                 # add_periodic: rows x period
POOL_SHAPE = (1, 523, 515, 64)                             # maxpool2d 3 / 2 and avgpool2d 2: 261 x 257 x 64 outputs
BILINEAR_CASE = (1, 131, 128, 64, 262, 256)                # B, H, W, C -> Ho, Wo
DWCONV_SCALAR_SHAPE = (1, 840, 840, 6)                     # C = 6: the scalar kernel, one item per element
UNFOLD_CASE = (1, 264, 264, 64, 6, 3)                      # B, H, W, C, k, s: 87 x 87 tokens of 2304; fold writes H W C items
CPB_CASE = (4, 1025, 1025, 225)                            # heads, N1, N2, table entries
# dsr_splines.hip: the backward deals n * G workgroups (G = min(1024 / n, the 32 MiB bound, DS_GMAX)) to the experts; each walks
# its share of an expert's pixels in batches of DS_NB.  More pixels than DS_NB * n * G: some workgroup walks a second batch.
DS_GMAX, DS_NB = 64, 64
DS_CASES = ((1, (1, 65, 64)), (2, (1, 96, 96)))            # (splines, image): 4160 > 4096 and 9216 > 8192 pixels
# data.hip: srhip_levels_u16_to_u8 (16384 blocks of 256 four-pixel groups) and srhip_im2col_c1 (16384 blocks of 256 floats)
LEVELS_PASS = 16384 * 256 * 4
LEVELS_N = LEVELS_PASS + 8 * 9 + 5                         # nine more aligned groups of four pairs and a ragged tail
LEVELS_SPLIT = 8388640                                     # a multiple of 8: both parts keep the vector path, each one pass
IM2COL_CASE = (1, 400, 400, 5, 28)                         # B, H, W, ksize, ldo: 4.48 M floats > 16384 * 256
