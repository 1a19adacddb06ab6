"""Entry points of libsrhip past their first chunk: host loops that launch in chunks, grids capped so that the kernel walks with
a stride, BatchNorm's rows-per-block above the minimum, the EDT row staged through LDS in pieces.  The shapes come from
tests/launch_plan_cases.py; tests/test_cpu_launch_plans.py ties them to the constants in the sources.  References and gates
are those of the older test of the same kernel (named at each test); no new tolerance is introduced.

The two wrappers over a bounded launch differ: ops.conv3x3_wgrad_batched splits a list longer than TNB_BATCH_MAX = 40 into
several launches (tested as such); ops.linear_wgrad_grouped does not split -- more than TNB_GROUP_MAX = 24 problems are
refused by the library's host check before any launch, and its callers (swinir_engine's cuts, srcnn_engine) keep their
groups within the bound.  The refusal is what is tested, together with the caller-side split.

Survey of the remaining entry points (host code read at this commit; `covered by` names the test that crosses the boundary):

    entry point (file)                      boundary                                   smallest shape across it         covered by
    srhip_hist_u8 (edt.hip)                 grid capped at 1024 blocks of 256 x 16     n = 4 194 305 pixels             test_hist_u8_past_the_grid_cap (new); the stride
                                            pixels; the kernel strides at every size                                    loop itself runs from n > 256 on (older test)
    srhip_origin_rowcum / _sample (edt.hip) one wave per row / per patch, 64-wide       --                               no cap, no chunk
                                            tiles of a row walked inside the wave
    srhip_dsr_splines_bwd (dsr_splines.hip) n G workgroups, G = min(1024 / n, 8 Mi     more than 64 n G pixels:         test_dsr_splines_backward_walks_more_than_one_
                                            floats / (n P), DS_GMAX = 64), dealt to    4097 at one spline               batch (new); G > 1 itself at every size
                                            the experts; each walks its share in                                        (test_gpu_dsr_splines.py)
                                            batches of 64 pixels
    srhip_dsr_splines_order / _fwd / _pack  one block per DS_CH pixels / per tile /    --                               no cap, no chunk
                                            per tensor
    srhip_lr_augment (augment.hip)          one thread per pixel (blur) / per group    --                               no cap, no chunk
                                            of four (compose), B h w < 2^31
    srhip_resize_cubic, srhip_u8_to_unit,   rs_grid: 8192 blocks of 256, one element   n = 2 097 153                    test_resize_entries_past_the_grid_cap (new)
    srhip_clip01 (resize.hip)               a thread, then a stride
    srhip_resize_bicubic_ac_pyramid         PYR_MAXL = 8 levels a launch; the wrapper  9 levels                         test_pyramid_wrapper_splits_past_eight_levels (new)
                                            splits a longer list
    srhip_imresize_aa{,_u16} (resize.hip)   one thread per run of 4 / 8 pixels         --                               no cap, no chunk
    srhip_psf_bin (lr_synth.hip)            one thread per run of 4 pixels             --                               no cap, no chunk
    srhip_view_gather / _merge (tta.hip)    3-d grid: tiles x planes x jobs            --                               no cap (65535 planes / jobs are refused)
    srhip_ingest_pad / _emit_uint (io.hip)  one thread per group of four               --                               no cap, no chunk
    srhip_patch_gather{,_f32,_u16}          64 blocks of 256 pixels per patch          P^2 > 16384: P = 129             uint8: test_patch_assembly_bit_exact_vs_
    (data.hip)                                                                                                          reference_golden (P = 512); f32, u16:
                                                                                                                        test_patch_gather_past_the_pixel_grid_cap (new)
    srhip_patch_gather_u16, srhip_roi_      MAXJOBS = 64 jobs a launch                 65 jobs                          test_gpu_deep_tiles.py (72 jobs),
    sample (data.hip)                                                                                                   test_patch_sampler.py (4096)
    srhip_levels_u16_to_u8, srhip_im2col_   16384 blocks of 256 (groups of four        16 777 217 pixels /              test_levels_u16_to_u8_and_im2col_past_the_grid_
    c1 (data.hip)                           pixels / floats)                           4 194 305 floats                 cap (new)
    srhip_nlsa_order / _attention           one thread per key, one block per (sample, --                               no capped grid; the in-block walk over a long
    (nlsa.hip)                              round) / per chunk / per four tokens                                        sequence: test_gpu_tape_op_kernels.py (L = 1025,
                                                                                                                        4096, 5000)
    srhip_nlsa_hash_buckets (nlsa.hip)      the reference's min(.., 128), on the host  L = 127 chunks                   test_nlsa_hash_buckets_cap (new)
    srhip_channel_gate (dfca.hip)           P < 4096: one pooling block a sample,      P = 4096                         test_gpu_tape_op_kernels.py (P = 63, 4095, 4096,
                                            else 64 partial blocks                                                      16384)
    srhip_unary{,_bwd}, the gate's apply    ew_blocks: 8192 blocks of 256              n = 2 097 153                    test_gpu_tape_op_kernels.py (2 100 003 elements;
    pass (dfca.hip)                                                                                                     channel_gate at 2 x 16384 x 256)
    srhip_dwconv3x3 (v4), srhip_gelu_gate,  ew_blocks: 16384 blocks of 256             4 194 305 items                  test_gpu_tape_op_kernels.py: `v4 past the grid
    srhip_mul_sigmoid (omni_ops.hip)                                                                                    cap`, 16400 x 257 elements
    srhip_dwconv3x3 (scalar), srhip_mul,    the same cap                               4 194 305 items                  the five `..._past_the_grid_cap` tests at the end
    _add_periodic, _maxpool2d{,_bwd},                                                                                   of this file (new)
    _bilinear_resize (omni_ops.hip);
    srhip_unfold, _fold (act_ops.hip);
    srhip_avgpool2d, _cpb_bias (grl_ops.hip)
    srhip_sum_periodic (omni_ops.hip)       one thread per column of the period        --                               no cap
    srhip_group_attention, _channel_        one block per group / per (sample, head,   --                               no cap, no chunk: the tiles of a long row are
    attention, _cosine_window_attention,    tile)                                                                       walked inside a block (test_gpu_tape_op_kernels.py)
    row softmaxes, rowdot, layernorm_rows
    srhip_layernorm_rows_bwd (act_ops.hip)  512 blocks of four rows, then a stride     M = 2049 rows                    test_layernorm_rows_backward_kernel (M = 4100)

Measured on an MI355X (every gate here is the older test's; the whole file runs in under six seconds): BatchNorm at 17 to 32
rows a block 1.6e-7 at most where the gates are 1e-6 to 5e-6; the split conv weight gradients 3.2e-7 (gate 2e-6); EDT, photon
counts, gathers, dropout and the other bit-for-bit comparisons exact, no photon-noise pixel marked as near a decision."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deep_tile_cases as D
import launch_plan_cases as L
import philox_ref as PR
import sr_oracle as O
from bn_float64 import check_batchnorm_vs_float64
from test_gpu_edt_sampler import foregrounds, scipy_d2
from test_gpu_lr_synth import check_noise

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED = 20260101


def recorded(monkeypatch, ops):
    """the names of the library calls the wrappers make from here on"""
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a, _f=ops.call: (calls.append(name), _f(name, *a))[1])
    return calls


# ---------------------------------------------------------------- EDT: more than one LDS chunk per row
@pytest.mark.parametrize("H,W,chunks", L.EDT_CASES, ids=lambda v: str(v))
def test_edt_sq_rows_wider_than_the_lds_chunk(H, W, chunks):
    """test_edt_sq_equals_scipy's gate (equality with scipy's squared EDT, the tail of a larger buffer untouched) on rows of
    one, two and three chunks: c0 offsets, the sentinel padding of a ragged last chunk, the barrier between chunks."""
    from srhip import ops
    rng = np.random.RandomState(H * 100000 + W)
    th = 100
    images = foregrounds(H, W, rng)
    images.update(L.edt_extra_foregrounds(H, W))
    for name, fg in images.items():
        img = np.where(fg, rng.randint(th, 256, (H, W)), rng.randint(0, th, (H, W))).astype(np.uint8)
        assert np.array_equal(img >= th, fg)
        buf = torch.full((H * W + 131,), -1, dtype=torch.int32, device="cuda")
        out = ops.edt_sq(torch.from_numpy(img).cuda(), th, out=buf)
        assert out is buf
        got = buf.cpu().numpy()
        want = scipy_d2(fg)
        bad = np.argwhere(got[:H * W].reshape(H, W) != want)
        assert bad.size == 0, ((H, W), name, len(bad), bad[:4].tolist())
        assert (got[H * W:] == -1).all(), ((H, W), name)


# ---------------------------------------------------------------- BatchNorm: more than 16 rows per block
@pytest.mark.parametrize("T,C", L.BN_CASES)
def test_batchnorm_blocks_of_more_than_one_sweep(T, C):
    """The flow and the gates of test_batchnorm_kernels_vs_float64 (2e-6 / 1e-6 / 5e-6 of the float64 result's largest entry)
    where bn_plan hands a block 20, 18, 17 (C = 1, ragged last pseudo-row) and 32 rows: a block's waves come round a second
    time, and the last sweep is cut by r1 inside a wave's four rows."""
    assert L.bn_plan(T, C)[4] > L.BN_SWEEP
    check_batchnorm_vs_float64((1, 1, T), C, seed=T % 1000 + C)


# ---------------------------------------------------------------- photon noise: more than NOISE_CHUNK samples
@pytest.mark.parametrize("hw", L.NOISE_HW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("B", L.NOISE_B)
def test_photon_noise_batches_of_more_than_one_launch(B, hw):
    """check_noise of tests/test_gpu_lr_synth.py (the numpy statement, its bounds) on batches the host walks in launches of
    1024 samples: x + b0 * hw, the counter word b = b0 + j, bit j of the launch's mask.  Samples with `on` clear keep their
    bits (check_noise asserts it)."""
    from srhip import ops
    h, w = hw
    x = L.noise_input(B, h, w)
    for photons, read_std in L.NOISE_SETTINGS:
        seed = 0x5EED0000 + int(photons) * 7 + B
        sd = torch.tensor([seed], dtype=torch.int64).cuda()
        for name, on in L.noise_masks(B).items():
            got = ops.photon_noise(torch.from_numpy(x.copy()).cuda(), sd, photons, read_std, on).cpu().numpy()
            marked, worst, info = check_noise(got, x, seed, photons, read_std, on=on)
            print(f"photon_noise B={B} {h}x{w} photons {photons:g} read_std {read_std:g} on={name}: marked {marked}, "
                  f"max |got - statement| = {worst:.3e}")
            if on is not None:
                touched = np.asarray(on, bool)
                assert np.array_equal(got[~touched].view(np.uint32), x[~touched].view(np.uint32))
                assert not np.array_equal(got[touched], x[touched])
        if B > L.NOISE_CHUNK:       # the samples of the later launches alone, under their own counters
            check_noise(got[L.NOISE_CHUNK:], x[L.NOISE_CHUNK:], seed, photons, read_std,
                        on=None if on is None else on[L.NOISE_CHUNK:], first_sample=L.NOISE_CHUNK)


# ---------------------------------------------------------------- patch gather: more than MAXJOBS jobs
def _gather_tiles(kind):
    rng = np.random.RandomState(11)
    if kind == "u8":
        return [rng.randint(0, 256, s).astype(np.uint8) for s in L.GATHER_TILES]
    return [rng.randn(*s).astype(np.float32) for s in L.GATHER_TILES]             # values outside [0, 1] too


@pytest.mark.parametrize("n", L.GATHER_JOBS)
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_patch_gather_batches_of_more_than_one_launch(kind, n):
    """srhip_patch_gather against O.patch_batch and srhip_patch_gather_f32 against the numpy crop + augment_img, bit for bit
    (the gates of test_patch_assembly_bit_exact_vs_reference_golden and test_patch_gather_f32_is_the_numpy_crop_and_
    augmentation), with 64, 65 and 130 jobs: jobs[b0 + b] and out + b0 * P * P of the later launches."""
    from srhip import ops
    tiles = _gather_tiles(kind)
    dev = [torch.from_numpy(t).cuda() for t in tiles]
    for P in L.GATHER_P:
        ids, y0, x0, modes = L.gather_jobs(L.GATHER_TILES, P, n)
        buf = torch.full((n * P * P + 64,), NAN, device="cuda")
        out = buf[:n * P * P].view(n, 1, P, P)
        got = (ops.patch_gather if kind == "u8" else ops.patch_gather_f32)(dev, ids, y0, x0, modes, P, out=out)
        assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (n, 1, P, P)
        if kind == "u8":
            want = O.patch_batch(tiles, ids, y0, x0, modes, P)
        else:
            want = torch.from_numpy(np.stack([np.ascontiguousarray(D.augment_img(
                tiles[ids[b]][y0[b]:y0[b] + P, x0[b]:x0[b] + P], modes[b])) for b in range(n)])[:, None])
        bad = [b for b in range(n) if not torch.equal(got[b].cpu().view(torch.int32), want[b].view(torch.int32))]
        assert not bad, (kind, P, n, bad[:8])
        assert bool(torch.isnan(buf[n * P * P:]).all())


# ---------------------------------------------------------------- dropout: past the grid cap
def _dropout_words(seed, site, n):
    """PR.words(seed, site, 0, n) with one Philox call per group of four elements (PR.words makes one per element)"""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    w = PR.philox4x32_10(g & np.uint64(PR.MASK32), g >> np.uint64(32), np.full(g.shape, site, dtype=np.uint64),
                         np.zeros(g.shape, dtype=np.uint64), seed & PR.MASK32, (seed >> 32) & PR.MASK32)
    return np.stack(w, axis=1).reshape(-1)[:n]


@functools.lru_cache(maxsize=None)
def _dropout_statement():
    n, site = L.DROPOUT_N, 5
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    words = _dropout_words(SEED, site, n)
    edge = 1 << 16
    assert np.array_equal(words[:edge], PR.words(SEED, site, 0, edge))                    # tied to the restatement at both ends
    assert np.array_equal(words[n - edge:], PR.words(SEED, site, n - edge, edge))
    thr, scale = PR.threshold(L.DROPOUT_P)
    keep = torch.from_numpy(words >= np.uint64(thr))
    ref = torch.where(keep, x * torch.tensor(scale, dtype=torch.float32), torch.zeros(n))
    return x, keep, ref, site


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned (vector)", "4 bytes off (scalar)"])
def test_dropout_past_the_grid_cap(shift):
    """n = 8 388 608 + 3 x 1024 + 5: the grid is capped at 8192 blocks, the first 770 threads take a second group at
    gridDim.x * blockDim.x.  (a) the output is the concatenation of three launches over consecutive sub-ranges, each below the
    cap and given its offset; (b) the kept / zeroed pattern is philox_ref's mask over the WHOLE range (one Philox call per
    group, about a second on the host; tied to PR.words on the first and last 2^16 elements), kept values x * scale bit for
    bit -- the gate of test_kernel_equals_the_restatement_bit_for_bit.  Cells outside [0, n) keep their NaN."""
    from srhip import ops
    x, keep, ref, site = _dropout_statement()
    n = L.DROPOUT_N
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    xb = torch.full((n + 8,), NAN, device="cuda")
    ob, pb = torch.full((n + 8,), NAN, device="cuda"), torch.full((n + 8,), NAN, device="cuda")
    xs, os_, ps = (b[4 + shift:4 + shift + n] for b in (xb, ob, pb))
    assert xs.data_ptr() % 16 == 4 * shift and os_.data_ptr() % 16 == 4 * shift
    xs.copy_(x)
    ops.dropout(xs, os_, seed, site, L.DROPOUT_P)
    for a, b in zip(L.DROPOUT_SPLITS, L.DROPOUT_SPLITS[1:]):
        ops.dropout(xs[a:b], ps[a:b], seed, site, L.DROPOUT_P, offset=a)
    got, parts = os_.cpu(), ps.cpu()
    bits = lambda t: t.view(torch.int32)
    diff = torch.nonzero(bits(got) != bits(parts)).flatten()
    assert diff.numel() == 0, ("one launch against three", diff.numel(), diff[:4].tolist())
    kept = got != 0
    wrong = torch.nonzero(kept != (keep & (x != 0))).flatten()
    assert wrong.numel() == 0, ("mask", wrong.numel(), wrong[:4].tolist())
    diff = torch.nonzero(bits(got) != bits(ref)).flatten()
    assert diff.numel() == 0, ("values", diff.numel(), diff[:4].tolist())
    assert torch.equal(bits(xs.cpu()), bits(x)), "the input is left alone"
    ops.dropout(xs, xs, seed, site, L.DROPOUT_P)                                          # in place
    assert torch.equal(bits(xs.cpu()), bits(ref))
    for buf in (xb, ob, pb):
        assert bool(torch.isnan(buf[:4 + shift]).all()) and bool(torch.isnan(buf[4 + shift + n:]).all())


# ---------------------------------------------------------------- the wrappers over a bounded launch
def _relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _conv_problems():
    """max(CONV_BATCHED_N) problems of CONV_BATCHED_SHAPE, every one with its own data and float64 weight / bias gradient"""
    B, H, W, C = L.CONV_BATCHED_SHAPE
    gen = torch.Generator().manual_seed(4100)
    out = []
    for _ in range(max(L.CONV_BATCHED_N)):
        x, dy = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
        wr = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
        br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wr, br, padding=1).backward(dy.double())
        out.append((dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous(), wr.grad, br.grad))
    return out


@pytest.mark.parametrize("n", L.CONV_BATCHED_N)
def test_conv_wgrad_batched_splits_a_list_longer_than_one_launch(monkeypatch, n):
    """ops.conv3x3_wgrad_batched with 41 and 81 same-shape problems: two and three launches of at most 40, every problem
    against float64 autograd at test_conv_wgrad_batched_matches_float64's gate (2e-6 of the largest entry); outputs start
    as 7.0, so a problem a launch skips, or one whose operands come from another chunk, fails."""
    from srhip import ops
    C = L.CONV_BATCHED_SHAPE[3]
    probs = _conv_problems()[:n]
    items = [(dy.cuda(), x.cuda(), torch.full((C, C, 3, 3), 7.0).cuda(), torch.full((C,), 7.0).cuda()) for dy, x, _, _ in probs]
    calls = recorded(monkeypatch, ops)
    ops.conv3x3_wgrad_batched(items)
    launches = calls.count("srhip_conv3x3_wgrad_batched_bx3")
    assert launches == -(-n // L.TNB_BATCH_MAX) > 1, calls
    worst = (0.0, 0.0)
    for k, ((_, _, dw, db), (_, _, rw, rb)) in enumerate(zip(items, probs)):
        ew, eb = _relerr(dw, rw), _relerr(db, rb)
        worst = max(worst, (ew, eb))
        assert ew < 2e-6 and eb < 2e-6, (k, ew, eb)
    print(f"conv3x3_wgrad_batched n={n}: {launches} launches, worst (dW, db) error {worst[0]:.2e}, {worst[1]:.2e}")


@pytest.mark.parametrize("n", L.LINEAR_GROUPED_N)
def test_linear_wgrad_grouped_refuses_a_longer_list_and_the_callers_split_works(monkeypatch, n):
    """ops.linear_wgrad_grouped does NOT split: 25 and 49 problems (the 64-column shapes of narrow_group in
    tests/test_gpu_linear_wgrad_grouped.py, each with its own data) reach the library's host check and are refused before
    any launch -- the reducer is never called and the NaN-filled outputs stay NaN.  The same problems in the callers' groups
    of at most 24 pass that file's bf16x3 gates (relerr < 2e-6; LayerNorm-folded: max(3 e32, 3e-5))."""
    import test_gpu_linear_wgrad_grouped as G
    from srhip import ops
    M = 100
    kinds = (dict(N=64, K=32, b_mode=1, ln=True), dict(N=32, K=64, b_mode=2, rs_rows=7), dict(N=64, K=64, rs_rows=7), dict(N=48, K=20))
    qs = [G.Prob(500 + i, M, **kinds[i % 4]) for i in range(n)]
    assert G.launch_class(ops, qs) == 1

    def problems(group):
        outs = [q.fresh_outputs() for q in group]
        ps = []
        for q, o in zip(group, outs):
            d = dict(dY=q.dev("dY"), X=q.dev("X"), dW=o["dW"], db=o["db"], b_mode=q.b_mode)
            if q.rs is not None:
                d.update(a_rowscale=q.dev("rs"), a_rowscale_rows=q.rs_rows)
            if q.stats is not None:
                d.update(ln_stats=q.dev("stats"))
            if q.ln:
                d.update(ln=(q.dev("W"), q.dev("gamma"), q.dev("beta"), o["dgamma"], o["dbeta"]))
            ps.append(d)
        return ps, outs
    ps, outs = problems(qs)
    calls = recorded(monkeypatch, ops)
    with pytest.raises(ops.SrhipError, match="problems"):
        ops.linear_wgrad_grouped(ps)
    assert calls[-1] == "srhip_gemm_tn_grouped_bx3" and "srhip_reduce_wgrad_grouped" not in calls, calls
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for o in outs for t in o.values())
    del calls[:]
    for j0 in range(0, n, L.TNB_GROUP_MAX):
        group = qs[j0:j0 + L.TNB_GROUP_MAX]
        G.check_group(ops, group, G.run_wrapper(ops, group), "bx3", 1)
    assert calls.count("srhip_gemm_tn_grouped_bx3") == calls.count("srhip_reduce_wgrad_grouped") == -(-n // L.TNB_GROUP_MAX)


# ---------------------------------------------------------------- the survey's cases
def test_hist_u8_past_the_grid_cap():
    """4 194 381 pixels: one block more than the 1024 the grid is capped at would hold at 16 pixels a thread; equality with
    np.bincount (test_hist_u8_and_otsu_roi_on_a_mixed_batch's gate)"""
    from srhip import ops
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, L.HIST_N).astype(np.uint8)
    img[-77:] = 255                                       # the pixels past the cap's last whole block: a bin of their own
    img[:-77][img[:-77] == 255] = 254
    got = ops.hist_u8(torch.from_numpy(img).cuda()).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, np.bincount(img, minlength=256)) and got[255] == 77


def test_resize_entries_past_the_grid_cap():
    """rs_grid caps srhip_u8_to_unit, srhip_clip01 and srhip_resize_cubic at 8192 blocks of 256 one-element threads.
    u8_to_unit: np.float32(v / 255.) and clip01_: clamp, bit for bit at 2 097 229 elements (tests/test_lowres.py's gates).
    resize_cubic: three 600 x 600 images to 840 x 840 in one launch (2 116 800 outputs, past the cap) give the bits of three
    one-image launches (705 600 each, below it; that path is gated against cv2's rule in tests/test_lowres.py)."""
    from srhip import ops
    rng = np.random.RandomState(6)
    u = rng.randint(0, 256, L.RS_N).astype(np.uint8)
    got = ops.u8_to_unit(torch.from_numpy(u).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.float32(u / 255.).view(np.uint32))
    x = torch.from_numpy((rng.rand(L.RS_N) * 3 - 1).astype(np.float32))
    x[-1], x[-2], x[0] = 2.0, -1.0, -0.0
    got = ops.clip01_(x.clone().cuda()).cpu()
    assert torch.equal(got, x.clamp(0.0, 1.0)) and got[-1] == 1.0 and got[-2] == 0.0 and float(got.min()) == 0.0
    for src in (torch.from_numpy(rng.randint(0, 256, (3, 600, 600)).astype(np.uint8)),
                torch.from_numpy(rng.rand(3, 600, 600).astype(np.float32))):
        assert 3 * 840 * 840 > L.RS_GRID_CAP * 256 >= 840 * 840
        dev = src.cuda()
        whole = ops.resize_cubic(dev, (840, 840))
        for b in range(3):
            alone = ops.resize_cubic(dev[b:b + 1].contiguous(), (840, 840))
            assert torch.equal(whole[b:b + 1].view(torch.uint8), alone.view(torch.uint8)), (src.dtype, b)


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_patch_gather_past_the_pixel_grid_cap(kind):
    """P = 136: 18496 pixels a patch, more than the 64 blocks of 256 a patch gets, so a thread takes a second pixel at
    gridDim.x * 256 (the uint8 form runs there at P = 512 in tests/test_gpu_edsr_api.py).  Bit for bit against the numpy crop
    + augment_img (+ the value rule of deep_tile_cases for 16-bit tiles), every mode."""
    from srhip import ops
    P = L.GATHER_BIG_P
    rng = np.random.RandomState(P)
    shapes = ((P + 3, P + 9), (P, P))
    if kind == "f32":
        tiles = [rng.randn(*s).astype(np.float32) for s in shapes]
        value = lambda v: v
    else:
        tiles = [D.tile_u16(s[0], s[1], 4095, seed=7 + i) for i, s in enumerate(shapes)]
        value = lambda v: D.unit(v, 4095)
    dev = [torch.from_numpy(t).cuda() for t in tiles]
    ids = [m % 2 for m in range(8)]
    y0 = [int(rng.randint(0, shapes[i][0] - P + 1)) for i in ids]
    x0 = [int(rng.randint(0, shapes[i][1] - P + 1)) for i in ids]
    modes = list(range(8))
    if kind == "f32":
        got = ops.patch_gather_f32(dev, ids, y0, x0, modes, P)
    else:
        got = ops.patch_gather_u16(dev, ids, y0, x0, modes, P, in_max=4095)
    for b in range(8):
        want = np.ascontiguousarray(D.augment_img(value(tiles[ids[b]][y0[b]:y0[b] + P, x0[b]:x0[b] + P]), modes[b]))
        assert np.array_equal(got[b, 0].cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, b)


@pytest.mark.parametrize("n", [9, 17])
def test_pyramid_wrapper_splits_past_eight_levels(monkeypatch, n):
    """ops.resize_bicubic_ac_pyramid walks its levels PYR_MAXL = 8 at a time: 9 and 17 levels of different sizes in two and
    three launches give, level by level, the bits of a launch of that level alone (which test_pyramid_kernel_vs_torch_float64
    gates against float64)."""
    from srhip import ops
    x = (torch.rand(2, 1, 24, 32, generator=torch.Generator().manual_seed(n)) * 1.2 - 0.1).cuda()
    shapes = [(3 + k, 40 - 2 * k) for k in range(n)]
    assert len(set(shapes)) == n and (24, 32) not in shapes
    calls = recorded(monkeypatch, ops)
    outs = ops.resize_bicubic_ac_pyramid(x, shapes)
    assert calls == ["srhip_resize_bicubic_ac_pyramid"] * -(-n // ops.PYR_MAX_LEVELS) and len(calls) > 1
    for s, o in zip(shapes, outs):
        alone = ops.resize_bicubic_ac_pyramid(x, [s])[0]
        assert tuple(o.shape) == (2, 1) + s and torch.equal(o.view(torch.int32), alone.view(torch.int32)), s


# ---------------------------------------------------------------- the tape nets' element-wise entries past ew_blocks' cap
def test_mul_and_add_periodic_past_the_grid_cap():
    """srhip_mul and srhip_add_periodic past the 16384 blocks of 256 of one grid pass, bit for bit against torch
    (test_omnisr_backward_pieces's gate)"""
    from srhip import ops
    g = torch.Generator().manual_seed(21)
    a, b = torch.randn(L.EW_N, generator=g).cuda(), torch.randn(L.EW_N, generator=g).cuda()
    assert torch.equal(ops.mul(a, b), a * b)
    x, v = torch.randn(*L.EW_PERIODIC, generator=g).cuda(), torch.randn(L.EW_PERIODIC[1], generator=g).cuda()
    assert torch.equal(ops.add_periodic(x.clone(), v), x + v)


def test_pooling_entries_past_the_grid_cap():
    """srhip_maxpool2d (k 3, s 2: equality), srhip_maxpool2d_bwd (1e-6 absolute) -- test_omnisr_backward_pieces's gates -- and
    srhip_avgpool2d (k 2: 1e-6 of the largest entry, the gate at the end of tests/test_gpu_tape_nets.py's GRL attention test)
    on 523 x 515 x 64: 4.29 M outputs each, 17.2 M items in the max pool's backward"""
    from srhip import ops
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*L.POOL_SHAPE, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    # gradients of a quarter of a normal: a dx, the sum of up to four of them, stays below 8, where three float32 roundings are
    # at most 7.2e-7 -- under the older test's absolute 1e-6 whatever the order of the sum (at 17 M normal draws it would not be)
    gr = torch.randn(yr.shape, generator=g) * 0.25
    (dref,) = torch.autograd.grad(yr, xr, gr)
    assert float(dref.abs().max()) < 8.0
    xd = x.cuda()
    assert torch.equal(ops.maxpool2d(xd, 3, 2).cpu(), yr.detach().contiguous())
    e = (ops.maxpool2d_bwd(xd, gr.contiguous().cuda(), 3, 2).cpu() - dref).abs().max().item()
    print(f"maxpool2d_bwd past the cap: max |dx - torch| = {e:.3e}")
    assert e <= 1e-6
    ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    e = _relerr(ops.avgpool2d(xd, 2), ref)
    print(f"avgpool2d past the cap: {e:.3e} of the largest entry")
    assert e < 1e-6


def test_bilinear_resize_and_scalar_dwconv_past_the_grid_cap():
    """srhip_bilinear_resize (131 x 128 -> 262 x 256, 64 channels: 4.29 M outputs) and the scalar arm of srhip_dwconv3x3
    (C = 6 on 840 x 840: 4.23 M; the v4 arm has its own past-the-cap case) under the Gates of tests/test_gpu_tape_op_kernels.py:
    min(ceiling, 3 e32) with the ceilings of test_bilinear_resize and test_dwconv3x3"""
    import tape_op_refs as R
    from srhip import ops
    from test_gpu_tape_op_kernels import CONTRACTION, ELEMENTWISE, Gates
    g = torch.Generator().manual_seed(23)
    B, H, W, C, Ho, Wo = L.BILINEAR_CASE
    x = torch.randn(B, H, W, C, generator=g)
    with Gates("bilinear_resize past the grid cap") as G:
        G(ops.bilinear_resize(x.cuda(), Ho, Wo), R.bilinear_resize(x.double(), Ho, Wo), R.bilinear_resize(x, Ho, Wo), ELEMENTWISE, "out")
    B, H, W, C = L.DWCONV_SCALAR_SHAPE
    x, w, bias = torch.randn(B, H, W, C, generator=g), torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, generator=g)
    out = torch.full((B, H, W, C), NAN, device="cuda")
    ops.dwconv3x3(x.cuda(), w.cuda(), bias.cuda(), out)
    with Gates("dwconv3x3 scalar past the grid cap") as G:
        G(out, R.dwconv3x3(x.double(), w.double(), bias.double()), R.dwconv3x3(x, w, bias), CONTRACTION, "out")


def test_unfold_and_fold_past_the_grid_cap():
    """srhip_unfold (17.4 M items: equality with F.unfold) and srhip_fold (264 x 264 x 64 = 4.46 M items: 1e-6 of the largest
    entry against F.fold) -- the gates of test_unfold_fold_vs_torch"""
    from srhip import ops
    B, H, W, C, k, s = L.UNFOLD_CASE
    g = torch.Generator().manual_seed(24)
    x = torch.randn(B, C, H, W, generator=g)
    ref = F.unfold(x, k, stride=s).permute(0, 2, 1)
    T = ref.shape[1]
    tok = torch.full((B * T, C * k * k), NAN, device="cuda")
    ops.unfold(x.permute(0, 2, 3, 1).contiguous().cuda(), C, k, s, 0, tok)
    assert torch.equal(tok.cpu().view(B, T, -1), ref)
    fref = F.fold(ref.permute(0, 2, 1), (H, W), k, stride=s).permute(0, 2, 3, 1)
    img = torch.full((B, H, W, C), NAN, device="cuda")
    ops.fold(tok, C, k, s, img)
    e = _relerr(img, fref)
    print(f"fold past the cap: {e:.3e} of the largest entry")
    assert e < 1e-6


def test_cpb_bias_past_the_grid_cap():
    """srhip_cpb_bias with heads N1 N2 = 4.2 M outputs: the bits of two launches over the two halves of the query rows, each
    below the cap (the values themselves are gated through the attention tests of tests/test_gpu_tape_nets.py)"""
    from srhip import ops
    heads, N1, N2, entries = L.CPB_CASE
    g = torch.Generator().manual_seed(25)
    table = torch.randn(entries, heads, generator=g).cuda()
    index = torch.randint(0, entries, (N1, N2), generator=g).cuda()
    whole = ops.cpb_bias(table, index, heads)
    assert tuple(whole.shape) == (heads, N2, N1)
    half = (N1 + 1) // 2
    for a, b in ((0, half), (half, N1)):
        part = ops.cpb_bias(table, index[a:b].contiguous(), heads)
        assert torch.equal(whole[:, :, a:b].contiguous().view(torch.int32), part.view(torch.int32)), (a, b)
    ref = 16 * torch.sigmoid(table.double()[index.view(-1)].view(N1, N2, heads).permute(2, 1, 0))
    assert _relerr(whole, ref) < 5e-6


# ---------------------------------------------------------------- DSR-Splines: a backward workgroup's second batch of pixels
@pytest.mark.parametrize("n,shape", L.DS_CASES, ids=lambda v: str(v))
def test_dsr_splines_backward_walks_more_than_one_batch(n, shape):
    """k_ds_bwd with more pixels than the n * 64 workgroups hold at 64 a batch: the b0 loop of a workgroup's share runs again.
    The flow and gates of test_shapes_against_the_float64_restatement (forward and every gradient against the float64
    restatement), which this calls on a 3 x 3 / two-hidden-layer net."""
    import test_gpu_dsr_splines as DS
    DS.test_shapes_against_the_float64_restatement(f"{n} splines {shape}", DS.config(3, 2, n, n == 1, True), shape)


# ---------------------------------------------------------------- data.hip's other capped grids
def test_levels_u16_to_u8_and_im2col_past_the_grid_cap():
    """srhip_levels_u16_to_u8 at 16 777 293 pixels (past 16384 blocks of 256 four-pixel groups): the bits of two launches over
    its two parts, each one pass, and deep_tile_cases.level8 on the first and last 2^16 pixels (test_gpu_deep_tiles.py's
    statement).  srhip_im2col_c1 at 400 x 400 x 28 floats: equality with F.unfold's columns, zero in the padding columns."""
    from srhip import ops
    rng = np.random.RandomState(31)
    v = rng.randint(0, 65536, L.LEVELS_N).astype(np.uint16)
    dev = torch.from_numpy(v).cuda()
    whole = ops.levels_u16_to_u8(dev, 4095)
    a = L.LEVELS_SPLIT
    assert torch.equal(whole[:a], ops.levels_u16_to_u8(dev[:a], 4095)) and torch.equal(whole[a:], ops.levels_u16_to_u8(dev[a:], 4095))
    got = whole.cpu().numpy()
    edge = 1 << 16
    assert np.array_equal(got[:edge], D.level8(v[:edge], 4095)) and np.array_equal(got[-edge:], D.level8(v[-edge:], 4095))
    B, H, W, ks, ldo = L.IM2COL_CASE
    x = torch.randn(B, H, W, generator=torch.Generator().manual_seed(32))
    got = ops.im2col_c1(x.cuda(), ks, ldo).cpu()
    want = F.unfold(x[:, None], ks, padding=ks // 2).permute(0, 2, 1).reshape(B * H * W, ks * ks)
    assert tuple(got.shape) == (B * H * W, ldo) and torch.equal(got[:, :ks * ks], want) and bool((got[:, ks * ks:] == 0).all())


def test_nlsa_hash_buckets_cap():
    """srhip_nlsa_hash_buckets (a host function): q + q % 2 for q = L // chunk_size chunks, at most 128 (network_nlsn.py:193-194)"""
    from srhip import ops
    assert [ops.nlsa_hash_buckets(144 * q + 5, 144) for q in (1, 2, 125, 126, 127, 128, 129, 500)] == [2, 2, 126, 126, 128, 128, 128, 128]
