"""The grouped Linear weight gradient (srhip_gemm_tn_grouped{,_bx3}) and its reducers (srhip_reduce_wgrad_grouped), arm by
arm, against a float64 statement of one problem evaluated on the CPU:

    dW = (rowscale . dY)^T pro(X),  db = colsum(rowscale . dY),   pro = identity | (X - mean) rstd | gelu (erf form)
    LayerNorm-folded finish:  dW' = gamma G + beta (x) d,  db' = d,  dgamma[k] = sum_n W[n,k] G[n,k],  dbeta[k] = sum_n W[n,k] d[n]

The same statement in float32 (plain torch matmuls on the same inputs) gives the e32 of the gates.  Outputs start as NaN,
the C-ABI cases hand NaN-filled part / colsum / ln_ws (the wrapper's scratch buffers are filled with NaN before every call
too), pitched operands are column slices of wider NaN-filled buffers, and every case runs twice and must give the same bits.

Arms and the rule that routes a case there (pick_tile's classes are restated below and tied to srhip_tn_tiles; the launch
takes the largest class of all widths of the group):
    class 3 -> k_tnb_grouped_h<3>, per problem (even = NI, NJ and both tiles multiples of 3):
        arm 1  even, b_mode 1, no row scale     tnb_body_h<3, 1, false, true>   LayerNorm-folded Linears (qkv, fc1)
        arm 2  even, b_mode 0, row scale        tnb_body_h<3, 0, true, true>    DropPath-scaled gradients (proj; fc2 with gh)
        arm 3  even, b_mode 2, row scale        tnb_body_h<3, 2, true, true>    fc2, gelu(h) recomputed
        arm 0  everything else                  tnb_body_h<3>                   64- / 128-column tiles, ragged 3-tuples, eval
    class 2 / 1 -> k_tnb_grouped<2> / <1> (bf16x3 body);  SRHIP_MM=f32 -> k_tn_grouped<w, w>, up to 4 problems
    reducers: k_reduce_group (plain: gamma == NULL; LayerNorm: + k_ln_affine_finish_group), slice loop tails 8 / 4 / 1

Gates (the suite's own):
    fp16x2 forms (class 3)   per row of dW, relative to the row's largest reference entry: e <= max(3 e32, 2e-6); db 2e-6
    bf16x3 bodies            relerr < 2e-6 (test_linear_wgrad_bx3_ragged_rows)
    exact-f32 arm            relerr <= 2e-5 (test_linear_wgrad)
    LayerNorm-folded dW' (per row), dgamma, dbeta:  e <= max(3 e32, 3e-5) (the ceiling of test_linear_wgrad_modes)
    synthetic reducer cases  float64 sums of the same float32 partials: e <= max(3 e32, 2e-6), e32 from float32 sums in
                             slice order
No headroom over 3 e32 was needed anywhere.

Out of contract, not run: nothing of case 6 -- a trailing slice with no rows at all IS inside the contract (the header
leaves S to the caller; both bodies give chunks past the slice end the zero row, count their barriers from the same chunk
count in both roles and store zero sums), so its partial sums are asserted to be zeros.  Problems that disagree in M or S
are not expressible through the C-ABI: both are arguments of the launch, not fields of srhip_tn_problem (asserted).

Measured on an MI355X, the worst e / gate over every case of an arm:

    arm                                   worst e / gate
    k_tnb_grouped_h<3> arm 0                       0.302
    k_tnb_grouped_h<3> arm 0 + ln finish           0.104
    k_tnb_grouped_h<3> arm 1 + ln finish           0.183
    k_tnb_grouped_h<3> arm 2                       0.349
    k_tnb_grouped_h<3> arm 3                       0.395
    k_tnb_grouped<2>                               0.156
    k_tnb_grouped<2> + ln finish                   0.086
    k_tnb_grouped<1>                               0.157
    k_tnb_grouped<1> + ln finish                   0.056
    k_tn_grouped (f32)                             0.017
    k_tn_grouped (f32) + ln finish                 0.019
    k_reduce_group plain                           0.163
    k_reduce_group ln                              0.182
    single-problem reducer plain                   0.163
    single-problem reducer ln                      0.181

(arm 3, the worst: e = 8.1e-7 of a row's largest entry where the float32 statement has 6.8e-7.)  64 cases, 3.4 s in all.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
TKB = 32            # tokens per staged chunk (gemm_tnb.hip / gemm_tn.hip)
RG_ROWS = 16        # rows per block of k_reduce_group (misc.hip)
CANARY = 256        # floats behind every ln_ws slice


@pytest.fixture(scope="module")
def ops():
    from srhip import ops as o
    return o


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n    arm                                   worst e / gate")
    for k in sorted(WORST):
        print(f"    {k:<38s}{WORST[k]:>14.3f}")


def note(arm, e, gate):
    WORST[arm] = max(WORST.get(arm, 0.0), e / gate)


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the routing rules, restated
def pick_tile(n):
    """(tile, class) of one operand width: pick_tile() of gemm_tnb.hip / gemm_tn.hip"""
    if n % 180 == 0:
        return 180, 3
    if n <= 64:
        return 64, 1
    if n <= 128 or n % 128 == 0:
        return 128, 2
    return 192, 3


def tiles_of(N, K):
    return cdiv(N, pick_tile(N)[0]) * cdiv(K, pick_tile(K)[0])


def launch_class(ops, qs):
    """largest tile class of the group's widths; the restated classes give the library's tile counts"""
    for q in qs:
        assert ops.lib.srhip_tn_tiles(q.N, q.K) == tiles_of(q.N, q.K), (q.N, q.K)
    return max(max(pick_tile(q.N)[1], pick_tile(q.K)[1]) for q in qs)


def h_arm(q):
    """the per-problem instantiation inside k_tnb_grouped_h<3>"""
    even = all(v % 3 == 0 for v in (q.N, q.K, pick_tile(q.N)[0], pick_tile(q.K)[0]))
    if even and q.b_mode == 1 and q.rs is None:
        return 1
    if even and q.b_mode == 0 and q.rs is not None:
        return 2
    if even and q.b_mode == 2 and q.rs is not None:
        return 3
    return 0


def plan_S(ops, qs, sfx="_bx3"):
    S = ctypes.c_int(0)
    ops.call("srhip_tn_group_plan" + sfx, qs[0].M, sum(tiles_of(q.N, q.K) for q in qs), ctypes.addressof(S))
    return S.value


def rows_per_slice(M, S):
    return cdiv(cdiv(M, S), TKB) * TKB


# ------------------------------------------------------------------ one problem and its statement
def finish(G, d, W, gamma, beta):
    """the LayerNorm-folded finish on G = sum of partials, d = sum of column sums (any dtype)"""
    return dict(dW=gamma[None] * G + beta[None] * d[:, None], db=d, dgamma=(W * G).sum(0), dbeta=(W * d[:, None]).sum(0))


class Prob:
    """dY [M][N], X [M][K] and the options of one srhip_tn_problem, with its own data (seed)."""

    def __init__(self, seed, M, N, K, b_mode=0, rs_rows=0, ln=False, regime=None, drop=None, pitch=None):
        g = torch.Generator().manual_seed(7000 + seed)
        self.M, self.N, self.K, self.b_mode, self.ln, self.pitch = M, N, K, b_mode, ln, pitch
        dY = torch.randn(M, N, generator=g) * (0.25 + 0.5 * (seed % 5))      # every problem at its own magnitude
        X = torch.randn(M, K, generator=g) * 1.5 + 0.3
        if regime == "grad":      # tiny, every token at its own scale, channels decades apart
            dY = dY * 1e-7 * torch.exp(torch.randn(M, 1, generator=g) * 2.5) * torch.exp(torch.randn(1, N, generator=g) * 3.0)
        if regime == "rise":      # magnitudes that grow by 2^40 along the tokens: the running scales must follow
            ramp = torch.exp2(torch.linspace(-30, 10, M)).reshape(M, 1)
            dY, X = dY * ramp, X * ramp
        if regime == "zero":      # columns that are zero everywhere / until late
            dY[:, :5] = 0
            X[:, 7] = 0
            dY[: M // 2, 9] = 0
        self.dY, self.X = dY.contiguous(), X.contiguous()
        self.rs, self.rs_rows = None, rs_rows
        if rs_rows:
            ns = cdiv(M, rs_rows)
            rs = torch.rand(ns, generator=g) + 0.5
            if drop == "first":
                rs[0] = 0
            if drop == "last":
                rs[-1] = 0
            if drop == "allbut1":
                keep = rs[ns // 2].item()
                rs.zero_()
                rs[ns // 2] = keep
            self.rs = rs
        self.stats = None
        if b_mode == 1:
            self.stats = torch.stack([X.mean(1), 1 / torch.sqrt(X.var(1, unbiased=False) + 1e-5)], 1).contiguous()
        if ln:
            self.W = torch.randn(N, K, generator=g) * 0.1
            self.gamma = 1 + 0.1 * torch.randn(K, generator=g)
            self.beta = 0.1 * torch.randn(K, generator=g)
        self._st, self._dev = {}, {}

    def variant(self, **kw):
        q = copy.copy(self)
        q._st, q._dev = {}, {}
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def statement(self, dtype):
        if dtype not in self._st:
            dY, X = self.dY.to(dtype), self.X.to(dtype)
            if self.rs is not None:
                dY = dY * self.rs.to(dtype).repeat_interleave(self.rs_rows)[: self.M, None]
            if self.b_mode == 1:
                X = (X - self.stats[:, :1].to(dtype)) * self.stats[:, 1:].to(dtype)
            elif self.b_mode == 2:
                X = F.gelu(X)
            G, d = dY.t() @ X, dY.sum(0)
            r = finish(G, d, self.W.to(dtype), self.gamma.to(dtype), self.beta.to(dtype)) if self.ln else dict(dW=G, db=d)
            self._st[dtype] = {k: v.double() for k, v in r.items()}
        return self._st[dtype]

    def dev(self, name):
        """device copy of an operand; dY / X of a pitched problem: a column slice of a wider NaN-filled buffer"""
        if name not in self._dev:
            t = getattr(self, name)
            if self.pitch and name in self.pitch:
                ld, off = self.pitch[name]
                buf = torch.full((self.M, ld), NAN, device="cuda")
                buf[:, off:off + t.shape[1]] = t.cuda()
                self._dev[name] = buf[:, off:off + t.shape[1]]
                assert self._dev[name].stride(0) == ld and off % 4 == 0 and ld % 4 == 0
            else:
                self._dev[name] = t.cuda()
        return self._dev[name]

    def opt(self, name):
        return None if getattr(self, name, None) is None else self.dev(name)

    def fresh_outputs(self):
        o = dict(dW=torch.full((self.N, self.K), NAN, device="cuda"), db=torch.full((self.N,), NAN, device="cuda"))
        if self.ln:
            o.update(dgamma=torch.full((self.K,), NAN, device="cuda"), dbeta=torch.full((self.K,), NAN, device="cuda"))
        return o


# ------------------------------------------------------------------ gates
def rowerr(x, ref):
    """largest error of a row, relative to the row's largest reference entry (a zero row must be exactly zero)"""
    den = ref.abs().max(1, keepdim=True).values.clamp_min(1e-300)
    return ((x.double().cpu() - ref).abs() / den).max().item()


def relerr(x, ref):
    return ((x.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def gate_check(arm, what, e, e32, ceiling, strict=False):
    gate = ceiling if e32 is None else max(3.0 * e32, ceiling)
    print(f"{arm} {what}: e {e:.3e} e32 {-1.0 if e32 is None else e32:.3e} gate {gate:.3e}")
    note(arm, e, gate)
    assert (e < gate) if strict else (e <= gate), (arm, what, e, e32, gate)


def check(q, out, kind, arm, r64=None, r32=None):
    """kind: 'h' (fp16x2 forms) | 'bx3' | 'f32' | 'red' (synthetic reducer input)"""
    r64 = q.statement(torch.float64) if r64 is None else r64
    r32 = q.statement(torch.float32) if r32 is None else r32
    dbtol = {"h": 2e-6, "bx3": 2e-6, "f32": 2e-5, "red": 2e-6}[kind]
    if q.ln:
        ceil = 2e-6 if kind == "red" else 3e-5
        gate_check(arm, "dW'", rowerr(out["dW"], r64["dW"]), rowerr(r32["dW"], r64["dW"]), ceil)
        for k in ("dgamma", "dbeta"):
            gate_check(arm, k, relerr(out[k], r64[k]), relerr(r32[k], r64[k]), ceil)
    elif kind in ("h", "red"):
        gate_check(arm, "dW", rowerr(out["dW"], r64["dW"]), rowerr(r32["dW"], r64["dW"]), 2e-6)
    elif kind == "bx3":
        gate_check(arm, "dW", relerr(out["dW"], r64["dW"]), None, 2e-6, strict=True)
    else:
        gate_check(arm, "dW", relerr(out["dW"], r64["dW"]), None, 2e-5)
    if kind == "red":
        gate_check(arm, "db", relerr(out["db"], r64["db"]), relerr(r32["db"], r64["db"]), dbtol)
    else:
        gate_check(arm, "db", relerr(out["db"], r64["db"]), None, dbtol, strict=kind != "f32")


def arm_name(kind, q, w):
    if kind == "h":
        return f"k_tnb_grouped_h<3> arm {h_arm(q)}" + (" + ln finish" if q.ln else "")
    if kind == "bx3":
        return f"k_tnb_grouped<{w}>" + (" + ln finish" if q.ln else "")
    return "k_tn_grouped (f32)" + (" + ln finish" if q.ln else "")


# ------------------------------------------------------------------ launchers
def st():
    return torch.cuda.current_stream().cuda_stream


def gemm_cabi(ops, qs, S, sfx="_bx3"):
    """srhip_gemm_tn_grouped{,_bx3} with an explicit S; NaN-filled part [S][N][K] / colsum [S][N] per problem"""
    n = len(qs)
    arr = (ops._TnProblem * n)()
    bufs = []
    for a, q in zip(arr, qs):
        part = torch.full((S, q.N, q.K), NAN, device="cuda")
        cs = torch.full((S, q.N), NAN, device="cuda")
        dY, X = q.dev("dY"), q.dev("X")
        a.A, a.lda, a.B, a.ldb, a.NI, a.NJ = dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), q.N, q.K
        rs, stats = q.opt("rs"), q.opt("stats")
        a.a_rowscale = None if rs is None else rs.data_ptr()
        a.a_rowscale_rows = q.rs_rows or 1
        a.b_mode = q.b_mode
        a.ln_stats = None if stats is None else stats.data_ptr()
        a.part, a.part_colsum = part.data_ptr(), cs.data_ptr()
        bufs.append((part, cs))
    ops.call("srhip_gemm_tn_grouped" + sfx, ctypes.addressof(arr), n, qs[0].M, S, st())
    return bufs


def reduce_cabi(ops, qs, bufs, S):
    """srhip_reduce_wgrad_grouped on (part, colsum) per problem; NaN outputs, every ln_ws slice sized by srhip_ln_affine_ws
    and followed by a NaN canary that must survive"""
    n = len(qs)
    red = (ops._ReduceProblem * n)()
    sizes = [ops.lib.srhip_ln_affine_ws(q.N, q.K) if q.ln else 0 for q in qs]
    for q, sz in zip(qs, sizes):
        assert sz == (cdiv(q.N, 4) * 2 * q.K if q.ln else 0) and sz >= cdiv(q.N, RG_ROWS) * 2 * q.K * bool(q.ln)
    arena = torch.full((sum(sz + CANARY for sz in sizes) + 1,), NAN, device="cuda")
    outs, lo, tails = [], 0, []
    for r, q, (part, cs), sz in zip(red, qs, bufs, sizes):
        o = q.fresh_outputs()
        r.part, r.colsum, r.dW, r.db, r.N, r.K = part.data_ptr(), cs.data_ptr(), o["dW"].data_ptr(), o["db"].data_ptr(), q.N, q.K
        if q.ln:
            r.W, r.gamma, r.beta = q.dev("W").data_ptr(), q.dev("gamma").data_ptr(), q.dev("beta").data_ptr()
            r.dgamma, r.dbeta = o["dgamma"].data_ptr(), o["dbeta"].data_ptr()
            r.ln_ws = arena[lo:].data_ptr()
            tails.append((lo + cdiv(q.N, RG_ROWS) * 2 * q.K, lo + sz + CANARY))     # behind what the row blocks write
            lo += sz + CANARY
        outs.append(o)
    ops.call("srhip_reduce_wgrad_grouped", ctypes.addressof(red), n, S, st())
    for a, b in tails:
        assert torch.isnan(arena[a:b]).all(), "k_reduce_group wrote past its ln_ws slice"
    return outs


def run_cabi(ops, qs, S, sfx="_bx3"):
    bufs = gemm_cabi(ops, qs, S, sfx)
    for part, cs in bufs:
        assert not torch.isnan(part).any() and not torch.isnan(cs).any()      # every slice of every tile written
    return reduce_cabi(ops, qs, bufs, S), bufs


def poison_scratch(ops, qs):
    """the wrapper's grow-only scratch (partial sums, column sums, LayerNorm workspace; sized as the wrapper sizes them)
    starts as NaN as well: a tile that a launch skips must not find the sums an earlier case left at the same place"""
    S = plan_S(ops, qs, ops._tn_sfx())
    lnws = sum(ops.lib.srhip_ln_affine_ws(q.N, q.K) for q in qs if q.ln)
    for name, n in (("tng_part", S * sum(q.N * q.K for q in qs)), ("tng_colsum", S * sum(q.N for q in qs)),
                    ("ln_affine_ws_g", max(1, lnws))):
        ops.SCRATCH.get(name, n, device="cuda").fill_(NAN)


def run_wrapper(ops, qs):
    """ops.linear_wgrad_grouped (the planner's S, the product's scratch buffers)"""
    poison_scratch(ops, qs)
    outs = [q.fresh_outputs() for q in qs]
    probs = []
    for q, o in zip(qs, outs):
        d = dict(dY=q.dev("dY"), X=q.dev("X"), dW=o["dW"], db=o["db"], b_mode=q.b_mode)
        if q.rs is not None:
            d.update(a_rowscale=q.dev("rs"), a_rowscale_rows=q.rs_rows)
        if q.stats is not None:
            d.update(ln_stats=q.dev("stats"))
        if q.ln:
            d.update(ln=(q.dev("W"), q.dev("gamma"), q.dev("beta"), o["dgamma"], o["dbeta"]))
        probs.append(d)
    ops.linear_wgrad_grouped(probs)
    return outs


def same_bits(a, b):
    """two results of one case: no NaN anywhere and the same bits"""
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), "two runs of one case differ (or left NaN)"
    elif isinstance(a, dict):
        for k in a:
            same_bits(a[k], b[k])
    else:
        for x, y in zip(a, b):
            same_bits(x, y)


def twice(fn):
    r1, r2 = fn(), fn()
    same_bits(r1, r2)
    return r1


def check_group(ops, qs, outs, kind, w=3):
    for q, o in zip(qs, outs):
        check(q, o, kind, arm_name(kind, q, w))


# ------------------------------------------------------------------ the groups of the cases
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def block_group(C, M, rs_rows, seed0=0, hidden=2):
    """the four Linears of one Swin block of width C: qkv (ln), fc2 (gelu + row scale), fc1 (ln), proj (row scale)"""
    H = hidden * C
    return [Prob(seed0 + 0, M, 3 * C, C, b_mode=1, ln=True), Prob(seed0 + 1, M, C, H, b_mode=2, rs_rows=rs_rows),
            Prob(seed0 + 2, M, H, C, b_mode=1, ln=True), Prob(seed0 + 3, M, C, C, rs_rows=rs_rows)]


def readme_group():
    """one RSTB layer of the README net: six blocks of qkv 540x180, fc2 180x360, fc1 360x180, proj 180x180 over M = 2077
    rows, DropPath groups of 260 rows (no multiple of the 32-token chunk)"""
    return cached("readme", lambda: [q for b in range(6) for q in block_group(180, 2077, 260, seed0=4 * b)])


def narrow_group(M):
    return [Prob(40, M, 64, 32, b_mode=1, ln=True), Prob(41, M, 32, 64, b_mode=2, rs_rows=7), Prob(42, M, 64, 64, rs_rows=7),
            Prob(43, M, 48, 20)]


# ------------------------------------------------------------------ 1. the README layer group
@pytest.mark.parametrize("variant,n", [("train", 24), ("train", 23), ("train", 4), ("train", 1), ("gh", 24), ("eval", 24)])
def test_readme_layer_group(ops, variant, n):
    """24 problems of four shapes (3 + 2 + 2 + 1 tiles, 48 tiles, S = 5) in k_tnb_grouped_h<3>: arm 1 (qkv, fc1:
    tnb_body_h<3, 1, false, true>), arm 3 (fc2 from h under the DropPath scale: tnb_body_h<3, 2, true, true>), arm 2 (proj;
    variant gh: fc2 from a stored gelu(h): tnb_body_h<3, 0, true, true>); variant eval (no row scale anywhere) puts b_mode 2
    and the plain proj into the general arm 0.  Every problem has its own data and its own reference (an off-by-one
    problem select fails); the first 1 / 4 / 23 problems walk shorter tile_start[] chains at S = 17 / 17 / 5.  Row-scale
    groups of 260 rows straddle the 32-token chunks."""
    base = readme_group()

    def make():
        if variant == "gh":
            return [q.variant(X=F.gelu(q.X), b_mode=0) if q.b_mode == 2 else q for q in base]
        if variant == "eval":
            return [q.variant(rs=None, rs_rows=0) if q.rs is not None else q for q in base]
        return base
    qs = cached(("readme", variant), make)[:n]
    assert launch_class(ops, qs) == 3
    want = {"train": [1, 3, 1, 2], "gh": [1, 2, 1, 2], "eval": [1, 0, 1, 0]}[variant]
    assert [h_arm(q) for q in qs] == (want * 6)[:n]
    if n == 24:
        assert sum(ops.lib.srhip_tn_tiles(q.N, q.K) for q in qs) == 48 and plan_S(ops, qs) == 5
        assert [ops.lib.srhip_tn_tiles(q.N, q.K) for q in qs[:4]] == [3, 2, 2, 1]
    else:
        assert plan_S(ops, qs) == {23: 5, 4: 17, 1: 17}[n]
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")


# ------------------------------------------------------------------ 2. place in the group does not change the bits
def test_place_in_group_keeps_the_bits_gemm(ops):
    """k_tnb_grouped_h<3>, the 24-way tile_start[] select: problem k = 0, 1, 12, 23 of the README group at S = 5 leaves the
    part / colsum bits of the same problem launched alone at that S."""
    qs = readme_group()
    S = 5
    bufs = twice(lambda: gemm_cabi(ops, qs, S))
    for k in (0, 1, 12, 23):
        (part, cs), = gemm_cabi(ops, [qs[k]], S)
        assert torch.equal(part, bufs[k][0]) and torch.equal(cs, bufs[k][1]), k


def test_place_in_group_keeps_the_bits_reducer(ops):
    """k_reduce_group (blk0 select) and k_ln_affine_finish_group (fblk0 select): a plain and a LayerNorm problem reduced
    alone give the bits they give at positions 0, middle and last of a mixed plain / LayerNorm group."""
    S = 7
    fill = [RProb(300 + i, S, N, K, ln=bool(i & 1)) for i, (N, K) in enumerate(RSHAPES)]
    for ln in (False, True):
        q = RProb(320 + ln, S, 180, 360, ln=ln)
        alone, = twice(lambda: reduce_cabi(ops, [q], [q.bufs()], S))
        for pos in (0, 3, 6):
            qs = fill[:pos] + [q] + fill[pos:]
            outs = reduce_cabi(ops, qs, [x.bufs() for x in qs], S)
            same_bits(alone, outs[pos])


# ------------------------------------------------------------------ 3. mixed tile classes under W = 3
@pytest.mark.parametrize("M", [31, 100, 515, 1500])
def test_mixed_tile_classes_c60_block(ops, M):
    """A C = 60 Swin block (qkv 180x60 ln, fc2 60x120 gelu + scale, fc1 120x60 ln, proj 60x60 scale): the 180 puts the launch
    in class 3, the 64- and 128-column tiles run inside k_tnb_grouped_h<3> with even = false -- the general arm
    tnb_body_h<3>, whose colq / dsh clamp the 3-column tuples at 60 and 120 valid columns."""
    qs = cached(("c60", M), lambda: block_group(60, M, 16, seed0=50))
    assert launch_class(ops, qs) == 3 and [h_arm(q) for q in qs] == [0, 0, 0, 0]
    assert {pick_tile(q.N)[0] for q in qs} | {pick_tile(q.K)[0] for q in qs} == {180, 64, 128}
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")


def test_ragged_w_tuples(ops):
    """k_tnb_grouped_h<3>, general arm with ragged = true: widths 184, 200, 68, 64 and 20 (multiples of 4, not of 3: a
    lane's 3-column tuple straddles the valid width and is shifted back by dsh) combined with 180 and 360."""
    M = 515

    def make():
        return [Prob(60, M, 184, 180, b_mode=1, ln=True), Prob(61, M, 180, 200, b_mode=2, rs_rows=16),
                Prob(62, M, 68, 360, rs_rows=16), Prob(63, M, 200, 68), Prob(64, M, 360, 184, b_mode=2),
                Prob(65, M, 64, 180, rs_rows=16), Prob(66, M, 180, 20, b_mode=1, ln=True)]
    qs = cached("ragged", make)
    assert launch_class(ops, qs) == 3 and all(h_arm(q) == 0 for q in qs)
    assert all((w % pick_tile(w)[0] or pick_tile(w)[0]) % 3 for w in (184, 200, 68, 64, 20))      # the last tile's valid width
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")


def test_ragged_64_column_tile_reads_only_its_columns(ops):
    """k_tnb_grouped_h<3>, general arm, 64-column tiles of 64 and 20 valid columns under W = 3 (colq clamped to opvalid - W):
    the narrow operands are columns 4.. of [M][256] buffers whose other columns are NaN, so a lane that reads past the valid
    width and uses what it read poisons the result."""
    M = 100
    pa, pb = dict(dY=(256, 4)), dict(X=(256, 4))

    def make():
        return [Prob(70, M, 64, 180, rs_rows=16, pitch=pa), Prob(71, M, 180, 64, b_mode=2, rs_rows=16, pitch=pb),
                Prob(72, M, 20, 360, pitch=pa), Prob(73, M, 180, 20, b_mode=1, ln=True, pitch=pb)]
    qs = cached("ragged64", make)
    assert launch_class(ops, qs) == 3 and all(h_arm(q) == 0 for q in qs)
    assert pick_tile(64) == (64, 1) and pick_tile(20) == (64, 1)
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")


# ------------------------------------------------------------------ 4. the bf16x3 bodies
@pytest.mark.parametrize("M", [100, 1500])
@pytest.mark.parametrize("group", ["c128", "narrow"])
def test_bf16x3_grouped_bodies(ops, group, M):
    """k_tnb_grouped<2>: a C = 128 block (384x128 ln, 128x256 gelu + scale, 256x128 ln, 128x128 scale), every width in the
    128-column class; k_tnb_grouped<1>: 64x32 ln, 32x64 gelu + scale, 64x64 scale, 48x20 plain, every width in the
    64-column class (tnb_body<W>, three bf16 planes / six products)."""
    qs = cached((group, M), lambda: block_group(128, M, 16, seed0=30) if group == "c128" else narrow_group(M))
    w = launch_class(ops, qs)
    assert w == (2 if group == "c128" else 1)
    assert all(pick_tile(q.N)[1] == w and pick_tile(q.K)[1] == w for q in qs)
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "bx3", w)


# ------------------------------------------------------------------ 5. the exact-f32 arm
def f32_classes(qs):
    return max(pick_tile(q.N)[1] for q in qs), max(pick_tile(q.K)[1] for q in qs)


@pytest.mark.parametrize("group", ["readme4", "readme1", "c60", "c128", "narrow", "narrow1"])
def test_exact_f32_arm(ops, monkeypatch, group):
    """SRHIP_MM=f32 -> srhip_gemm_tn_grouped -> k_tn_grouped<w, w>: one block of the README group (<3, 3>) and its qkv
    alone, the C = 60 block (wi = 3, wj = 2: widened to <3, 3>), the C = 128 block (<2, 2>), the narrow group (<1, 1>)
    and its 48x20 alone."""
    monkeypatch.setenv("SRHIP_MM", "f32")
    assert ops._tn_sfx() == ""
    qs = {"readme4": lambda: readme_group()[:4], "readme1": lambda: readme_group()[:1],
          "c60": lambda: cached(("c60", 515), lambda: block_group(60, 515, 16, seed0=50)),
          "c128": lambda: cached(("c128", 100), lambda: block_group(128, 100, 16, seed0=30)),
          "narrow": lambda: cached(("narrow", 1500), lambda: narrow_group(1500)),
          "narrow1": lambda: cached(("narrow", 1500), lambda: narrow_group(1500))[3:]}[group]()
    launch_class(ops, qs)
    assert f32_classes(qs) == {"readme4": (3, 3), "readme1": (3, 3), "c60": (3, 2), "c128": (2, 2), "narrow": (1, 1),
                               "narrow1": (1, 1)}[group]
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "f32")


# ------------------------------------------------------------------ 6. slices
@pytest.mark.parametrize("M,S,what", [(515, 1, "S = 1"), (257, 5, "last slice: one row"), (224, 4, "last slice: one chunk"),
                                      (100, 4, "every slice within one chunk"), (100, 5, "trailing slice without rows")])
def test_caller_chosen_slices(ops, M, S, what):
    """A caller-chosen S through the C-ABI on 180x360 gelu + scale (k_tnb_grouped_h<3> arm 3) and 540x180 ln (arm 1): one
    slice; a last slice of one row; of one whole chunk; M = 100 in four slices (25 rows each before the rounding to
    chunks); a trailing slice with no rows at all, whose partial sums must be zeros (in contract: see the module
    docstring; the planner never produces it)."""
    qs = cached(("slices", M), lambda: [Prob(80, M, 180, 360, b_mode=2, rs_rows=7), Prob(81, M, 540, 180, b_mode=1, ln=True)])
    assert launch_class(ops, qs) == 3 and [h_arm(q) for q in qs] == [3, 1]
    rps = rows_per_slice(M, S)
    last = M - (S - 1) * rps
    assert {"S = 1": last == M, "last slice: one row": last == 1, "last slice: one chunk": last == TKB,
            "every slice within one chunk": rps == TKB and cdiv(M, S) < TKB and last > 0,
            "trailing slice without rows": last <= 0 and M - (S - 2) * rps > 0}[what]
    outs, bufs = twice(lambda: run_cabi(ops, qs, S))
    if last <= 0:
        for part, cs in bufs:
            assert (part[S - 1] == 0).all() and (cs[S - 1] == 0).all()
    check_group(ops, qs, outs, "h")


# ------------------------------------------------------------------ 7. DropPath zeros and scale dynamics
@pytest.mark.parametrize("drop", ["first", "last", "allbut1"])
def test_droppath_dropped_samples(ops, drop):
    """k_tnb_grouped_h<3> arms 2 and 3 with samples dropped by DropPath: the row scale is exactly 0.0 over the whole leading
    (first sample, all but one) or trailing chunks of a slice, so the running column scale of tnb_body_h starts from, or
    ends on, an all-zero maximum.  Planner's S = 17: whole slices of zeros too."""
    M = 2077
    qs = cached(("drop", drop), lambda: [Prob(90, M, 180, 180, rs_rows=260, drop=drop),
                                         Prob(91, M, 180, 360, b_mode=2, rs_rows=260, drop=drop)])
    assert launch_class(ops, qs) == 3 and [h_arm(q) for q in qs] == [2, 3] and plan_S(ops, qs) == 17
    assert all((q.rs == 0).sum().item() == (7 if drop == "allbut1" else 1) for q in qs)
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")


@pytest.mark.parametrize("regime", ["grad", "rise", "zero"])
def test_scale_dynamics_regimes(ops, regime):
    """The 'grad' (tiny, tokens and channels decades apart), 'rise' (2^40 along the tokens) and 'zero' (zero columns)
    regimes of the fp16x2 weight-gradient test on 540x180 ln (k_tnb_grouped_h<3> arm 1) and 180x360 gelu + scale (arm 3);
    rows of dW that must be exactly zero are."""
    M = 2077
    qs = cached(("regime", regime), lambda: [Prob(100, M, 540, 180, b_mode=1, ln=True, regime=regime),
                                             Prob(101, M, 180, 360, b_mode=2, rs_rows=260, regime=regime)])
    assert launch_class(ops, qs) == 3 and [h_arm(q) for q in qs] == [1, 3]
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h")
    if regime == "zero":
        for o in outs:
            assert (o["dW"][:5] == 0).all() and (o["db"][:5] == 0).all()
        assert (outs[1]["dW"][:, 7] == 0).all()       # gelu(0) = 0 (the LayerNorm prologue moves a zero column)


# ------------------------------------------------------------------ 8. pitched operands
@pytest.mark.parametrize("mm", ["bx3", "f32"])
def test_pitched_operands(ops, monkeypatch, mm):
    """dY = columns 180..360 of an [M][540] buffer, X = columns 4..184 of an [M][192] buffer (the rest NaN), one problem
    of each arm of k_tnb_grouped_h<3> (1: ln, 3: gelu + scale, 2: scale, 0: gelu without scale) in one launch; the same
    four on k_tn_grouped<3, 3>."""
    if mm == "f32":
        monkeypatch.setenv("SRHIP_MM", "f32")
    M = 515
    pitch = dict(dY=(540, 180), X=(192, 4))

    def make():
        return [Prob(110, M, 180, 180, b_mode=1, ln=True, pitch=pitch), Prob(111, M, 180, 180, b_mode=2, rs_rows=260, pitch=pitch),
                Prob(112, M, 180, 180, rs_rows=260, pitch=pitch), Prob(113, M, 180, 180, b_mode=2, pitch=pitch)]
    qs = cached("pitched", make)
    assert launch_class(ops, qs) == 3 and [h_arm(q) for q in qs] == [1, 3, 2, 0]
    assert all(q.dev("dY").stride(0) == 540 and q.dev("X").stride(0) == 192 for q in qs)
    outs = twice(lambda: run_wrapper(ops, qs))
    check_group(ops, qs, outs, "h" if mm == "bx3" else "f32")


# ------------------------------------------------------------------ 9. the reducers alone
RSHAPES = [(180, 180), (540, 180), (180, 360), (60, 120), (20, 48), (4, 4)]     # N no multiple of RG_ROWS, K none of 64


class RProb:
    """synthetic partial sums part [S][N][K] and column sums colsum [S][N] of one reduce problem (on the device)"""

    def __init__(self, seed, S, N, K, ln=False):
        g = torch.Generator().manual_seed(9000 + seed)
        self.S, self.N, self.K, self.ln = S, N, K, ln
        self.part = (torch.randn(S, N, K, generator=g) * torch.exp(torch.randn(S, 1, 1, generator=g))).cuda()
        self.colsum = (torch.randn(S, N, generator=g) * torch.exp(torch.randn(S, 1, generator=g))).cuda()
        self.W, self.gamma = (torch.randn(N, K, generator=g) * 0.1).cuda(), (1 + 0.1 * torch.randn(K, generator=g)).cuda()
        self.beta = (0.1 * torch.randn(K, generator=g)).cuda()
        self._st = {}

    def as_ln(self, ln):
        q = copy.copy(self)
        q.ln, q._st = ln, {}
        return q

    def dev(self, name):
        return getattr(self, name)

    def bufs(self):
        return self.part, self.colsum

    fresh_outputs = Prob.fresh_outputs

    def statement(self, dtype):
        if dtype not in self._st:
            if dtype == torch.float64:
                G, d = self.part.double().sum(0), self.colsum.double().sum(0)
            else:           # float32, in slice order
                G, d = torch.zeros_like(self.part[0]), torch.zeros_like(self.colsum[0])
                for s in range(self.S):
                    G, d = G + self.part[s], d + self.colsum[s]
            r = finish(G, d, self.W.to(dtype), self.gamma.to(dtype), self.beta.to(dtype)) if self.ln else dict(dW=G, db=d)
            self._st[dtype] = {k: v.double().cpu() for k, v in r.items()}
        return self._st[dtype]


def check_reduced(qs, outs, arm):
    for q, o in zip(qs, outs):
        check(q, o, "red", arm + (" ln" if q.ln else " plain"))


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 17])
def test_reducers_slice_tails(ops, S):
    """k_reduce_group's slice loop (blocks of 8, a block of 4, single slices) at every tail, on the six shapes, LayerNorm
    (gamma != NULL: dW = gamma G + beta (x) d, the dgamma / dbeta shares, k_ln_affine_finish_group) and plain problems
    alternating with the parity of S; the single-problem reducers k_reduce_slices / k_fin_ln_linear + k_ln_affine_finish
    on the same inputs against the same statement."""
    qs = [RProb(200 + 10 * S + i, S, N, K, ln=bool((i + S) & 1)) for i, (N, K) in enumerate(RSHAPES)]
    outs = twice(lambda: reduce_cabi(ops, qs, [q.bufs() for q in qs], S))
    check_reduced(qs, outs, "k_reduce_group")
    for q in qs:
        def single():
            o = q.fresh_outputs()
            if q.ln:
                sz = ops.lib.srhip_ln_affine_ws(q.N, q.K)
                ws = torch.full((sz + CANARY,), NAN, device="cuda")
                ops.call("srhip_reduce_ln_linear_wgrad", q.part.data_ptr(), q.colsum.data_ptr(), S, q.W.data_ptr(),
                         q.gamma.data_ptr(), q.beta.data_ptr(), o["dW"].data_ptr(), o["db"].data_ptr(), o["dgamma"].data_ptr(),
                         o["dbeta"].data_ptr(), q.N, q.K, ws.data_ptr(), st())
                assert torch.isnan(ws[sz:]).all()
            else:
                ops.call("srhip_reduce_linear_wgrad", q.part.data_ptr(), q.colsum.data_ptr(), S, o["dW"].data_ptr(),
                         o["db"].data_ptr(), q.N, q.K, st())
            return o
        check(q, twice(single), "red", "single-problem reducer" + (" ln" if q.ln else " plain"))


@pytest.mark.parametrize("pattern", ["first", "last", "alternating", "all", "none"])
@pytest.mark.parametrize("n", [1, 5, 24])
def test_reducer_groups(ops, n, pattern):
    """k_reduce_group / k_ln_affine_finish_group with 1, 5 and 24 problems of the six shapes at S = 13 (8 + 4 + 1), the
    LayerNorm problems first, last, alternating, all and none: the blk0 chain, and fblk0 with plain problems in front of,
    behind and between the LayerNorm ones."""
    S = 13
    base = cached("rgroup", lambda: [RProb(400 + i, S, *RSHAPES[i % 6]) for i in range(24)])[:n]
    is_ln = {"first": lambda i: i < (n + 1) // 2, "last": lambda i: i >= n // 2, "alternating": lambda i: i % 2 == 0,
             "all": lambda i: True, "none": lambda i: False}[pattern]
    qs = [q.as_ln(is_ln(i)) for i, q in enumerate(base)]
    outs = twice(lambda: reduce_cabi(ops, qs, [q.bufs() for q in qs], S))
    check_reduced(qs, outs, "k_reduce_group")


# ------------------------------------------------------------------ 10. refusals
def test_refusals_come_from_the_host_checks(ops, monkeypatch):
    """Each of these is refused by a host check and reaches no launch (the NaN-filled outputs stay NaN): 25 problems (bf16x3
    launch and reducer), 5 problems on the exact-f32 launch, a width that is no multiple of 4, b_mode 1 without
    statistics, b_mode 3, S = 0, M = 0, a row scale over groups of 0 rows, an incomplete plain and an incomplete LayerNorm
    reduce problem.  Problems that disagree in M or S cannot be written down: both are arguments of the launch."""
    M, S = 64, 2
    assert not {"M", "S"} & {f[0] for f in ops._TnProblem._fields_}
    q = Prob(120, M, 180, 180, rs_rows=16)
    part = torch.full((S, 180, 180), NAN, device="cuda")
    cs = torch.full((S, 180), NAN, device="cuda")
    stats = torch.zeros(M, 2, device="cuda")

    def tn(n=1, sfx="_bx3", M=M, S=S, **kw):
        arr = (ops._TnProblem * n)()
        for a in arr:
            a.A, a.lda, a.B, a.ldb, a.NI, a.NJ = q.dev("dY").data_ptr(), 180, q.dev("X").data_ptr(), 180, 180, 180
            a.a_rowscale_rows, a.part, a.part_colsum = 1, part.data_ptr(), cs.data_ptr()
            for k, v in kw.items():
                setattr(a, k, v)
        with pytest.raises(ops.SrhipError):
            ops.call("srhip_gemm_tn_grouped" + sfx, ctypes.addressof(arr), n, M, S, st())
    tn(n=25)
    tn(n=5, sfx="")
    for sfx in ("_bx3", ""):
        tn(sfx=sfx, NI=178)
        tn(sfx=sfx, NJ=182)
        tn(sfx=sfx, lda=182)
        tn(sfx=sfx, b_mode=1)
        tn(sfx=sfx, b_mode=3, ln_stats=stats.data_ptr())
        tn(sfx=sfx, S=0)
        tn(sfx=sfx, M=0)
        tn(sfx=sfx, a_rowscale=q.dev("rs").data_ptr(), a_rowscale_rows=0)
    r = RProb(130, S, 180, 180, ln=True)
    o = r.fresh_outputs()
    ws = torch.full((ops.lib.srhip_ln_affine_ws(180, 180),), NAN, device="cuda")

    def red(n=1, S=S, **kw):
        arr = (ops._ReduceProblem * n)()
        for a in arr:
            a.part, a.colsum, a.dW, a.db, a.N, a.K = r.part.data_ptr(), r.colsum.data_ptr(), o["dW"].data_ptr(), o["db"].data_ptr(), 180, 180
            a.W, a.gamma, a.beta = r.W.data_ptr(), r.gamma.data_ptr(), r.beta.data_ptr()
            a.dgamma, a.dbeta, a.ln_ws = o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), ws.data_ptr()
            for k, v in kw.items():
                setattr(a, k, v)
        with pytest.raises(ops.SrhipError):
            ops.call("srhip_reduce_wgrad_grouped", ctypes.addressof(arr), n, S, st())
    red(n=25)
    red(S=0)
    red(dW=None)
    red(N=0)
    for missing in ("W", "beta", "dgamma", "dbeta", "ln_ws"):
        red(**{missing: None})
    torch.cuda.synchronize()
    for t in (part, cs, ws, *o.values()):
        assert torch.isnan(t).all()
    monkeypatch.setenv("SRHIP_MM", "f32")        # the wrapper on the exact-f32 arm: five problems
    with pytest.raises(ops.SrhipError):
        run_wrapper(ops, narrow_group(64) + narrow_group(64)[:1])
