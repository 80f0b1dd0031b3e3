"""The fp32 ends of a DiT pass (csrc/embed_head.hip: wanq_linear_f32, wanq_patch_embed, wanq_head_fwd, wanq_time_sinusoid; csrc/stepops.hip:
wanq_lincomb) on operands whose answer is known exactly.  Every call goes through the C ABI and the test owns every buffer: outputs
AND inputs are windows in flat allocations with guard zones of GUARD elements in front and behind, every allocation holds a quiet-NaN
bit pattern before EVERY launch (an over-read that reaches a sum shows as a NaN), and after it both guards of the output must still
hold that pattern.

  A  Linear, exact: integer operands over a shape table (gemv at M = 1..4, tile kernel above), one-hot rows (which k is read), padded
     input rows = act_out(bias), activations on exact pre-activations against torch's own fp32 SiLU / GELU as the yardstick.
  B  patch embedding, exact: the latent holds its own flat index, weight rows are one-hot: the output is the index Conv3d's definition
     gathers; all four patch-resident forms (K = 16, 32, 48, 64) and the tile kernel's gather (K = 80, 144); zero rows up to out_rows.
  C  head: constant rows exactly, +-a_r rows under the bound derived in profiles/PARITY_NOTES.md, the eps probe, unpatchify against
     model.py's definition and bit for bit against the plain form.
  D  isolation on the three matrix entries: a huge row, NaN / Inf in a row, a weight row, a latent patch stay where they belong.
  E  time sinusoid: pos = 0 exactly, the dtype reads, everything else within one fp32 rounding + the float64 library terms.
  F  wanq_lincomb exactly: all 32 (n_out, n_in), the grid-stride loop's second turn, an output that aliases an input.
  G  empty and refused calls leave every window untouched.
  H  CPU self-tests (not marked gpu): a numpy model of the kernels' index maps and dispatch passes the same probes, thirteen mutants of
     it fail named ones, the tables' coverage and the exactness of every expectation are proved.

Every probe is a function of a `run` object, so that the GPU (GpuRun) and the model (ModelRun) go through the same checkers.
Kernel rules restated here:
  tiling            BM = BN = 64, BK = 16, nk = K / 16, two LDS buffers chosen by kt & 1
  Linear dispatch   1 <= M <= 4: the gemv, one wave per output channel (four per workgroup; a wave with n >= N returns), lanes read
                    k = 4 lane + 256 j; rows >= x_rows enter as zeros; otherwise the tile kernel
  patch embedding   K = C pt ph pw <= 64: the patch-resident kernel, NK4 = K / 4 in {4, 8, 12, 16}, walking ceil(N / 64) chunks of 64
                    channels; larger K: the tile kernel with the A_PATCH loader (the same (c, dt, dh, dw) decomposition of k)
  head              A_LNMOD with C_PLAIN, or C_UNPATCH when asked (N <= 64); statistics prologue reads c = 4 lane + 256 j, two passes,
                    rstd = rsqrtf(var + eps); operand = (x - mean) rstd (1 + scale + e) + (shift + e), modulation = [shift row, scale row]
  stores            rows < out_rows, columns < N; rows [M, out_rows) are 0; rows [x_rows, M) are act_out(bias)
  lincomb           min(ceil(numel / 4 / 256), 2048) workgroups of 256 threads, one float4 each, grid-stride."""
import collections
import ctypes
import math

import numpy as np
import pytest
import torch

# The GPU part (sections A - G) is marked test by test, so that section H below runs without a GPU; test_gpu_part_is_marked keeps a
# test added above section H from being left unmarked.
gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
ACTS = {None: 0, "gelu": 1, "silu": 2}
GUARD = 4096  # fp32 elements; a multiple of 4, so every window stays 16-byte aligned
SENT = 0x7FC5A5A5  # a quiet NaN with a payload; compared as an integer
BM, BN, BK = 64, 64, 16
# rsqrtf: 1 ulp, the figure of the single-precision table in the published HIP documentation ("HIP math API"); no copy of that table
# ships with the toolkit, so the figure is taken from the published page and was not verified on a machine (profiles/PARITY_NOTES.md)
RSQ_ULP = 1.0

Result = collections.namedtuple("Result", "win fails")


# ================================================================================================ buffers and checkers
class Window:
    """fp32 elements of `shape` inside a flat allocation with GUARD elements in front and behind, all preset to the sentinel."""

    def __init__(self, shape, dev, values=None):
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape)) if len(self.shape) else 1
        self.flat = torch.full((2 * GUARD + self.n,), SENT, dtype=torch.int32, device=dev)
        if values is not None:
            self.window().copy_(values.to(dev).reshape(self.shape).float())

    def bits(self):
        return self.flat[GUARD:GUARD + self.n].view(self.shape)

    def window(self):
        return self.bits().view(torch.float32)

    def ptr(self):
        p = self.flat.data_ptr() + GUARD * 4
        assert p % 16 == 0
        return p


def guard_failures(win, what="output"):
    n = GUARD + win.n
    fails = []
    if bool((win.flat[:GUARD] != SENT).any()):
        fails.append(f"the guard in front of the {what} was written at element {int((win.flat[:GUARD] != SENT).nonzero()[0]) - GUARD}")
    if bool((win.flat[n:] != SENT).any()):
        fails.append(f"the guard behind the {what} was written at element {win.n + int((win.flat[n:] != SENT).nonzero()[0])}")
    return fails


def check_exact(res, expect, describe=None):
    """Bit equality of every element of the window with the fp32 value of `expect` (asserted to be exact in fp32; -0.0 where +0.0 is
    due fails, as does an element that still holds the sentinel), guards intact.  describe(index tuple, got) adds what the probe knows
    about the first bad element."""
    win = res.win
    fails = list(res.fails) + guard_failures(win)
    got = win.window()
    want = expect.to(got.device).reshape(win.shape).double()
    assert torch.equal(want.float().double(), want)
    bad = win.bits() != want.float().view(torch.int32)
    if bool(bad.any()):
        idx = bad.nonzero()
        at = tuple(int(v) for v in idx[0])
        unwritten = int((win.bits()[bad] == SENT).sum())
        more = "" if describe is None else "; " + describe(at, float(got[at]))
        fails.append(f"{len(idx)} elements differ ({unwritten} of them never written); first at {at}: got {got[at].item()} "
                     f"expected {expect.reshape(win.shape)[at].item()}{more}")
    return fails


def check_bound(res, ref, bound):
    """|out - ref| <= bound elementwise (NaN fails), guards intact.  Returns (failures, largest err / bound)."""
    win = res.win
    fails = list(res.fails) + guard_failures(win)
    ref, bound = ref.to(win.flat.device).reshape(win.shape), bound.to(win.flat.device).reshape(win.shape)
    err = (win.window().double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        at = tuple(int(v) for v in bad.nonzero()[0])
        fails.append(f"{int(bad.sum())} elements beyond the bound; first at {at}: got {win.window()[at].item()} ref {ref[at].item()} "
                     f"bound {bound[at].item():.3e}")
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return fails, float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0


def hash32(r, c, salt):
    """A fixed integer hash of (r, c): int64 tensor of values below 2^32 (the products wrap mod 2^64; the low 32 bits are kept)."""
    m = 0xFFFFFFFF
    h = (r * 0x9E3779B1 + c * 0x85EBCA77 + (salt * 0x27D4EB2F + 1)) & m
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & m
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & m
    return h ^ (h >> 15)


def ints(R, C, salt, lo, hi, dev="cpu"):
    """int64 [R, C] (or [R] when C is None) of hashed integers in [lo, hi]."""
    r = torch.arange(R, dtype=torch.int64, device=dev)
    if C is None:
        return hash32(r, torch.zeros((), dtype=torch.int64, device=dev), salt) % (hi - lo + 1) + lo
    return hash32(r[:, None], torch.arange(C, dtype=torch.int64, device=dev)[None, :], salt) % (hi - lo + 1) + lo


def exact_f32(x):
    return torch.equal(x.double().float().double(), x.double())


def act64(v, kind):
    """The float64 definitions: SiLU v / (1 + e^-v); GELU in torch's tanh form."""
    if kind == "silu":
        return v * torch.special.expit(v)
    if kind == "gelu":
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    return v


def act_unit(v, kind):
    """The scale an activation's fp32 error is measured in: SiLU is a quotient (relative to |silu(v)|); GELU's 1 + tanh carries
    tanhf's ABSOLUTE error at magnitude 1 into 0.5 v (.), so its unit is u |v| (profiles/PARITY_NOTES.md)."""
    return U * (act64(v, kind).abs() if kind == "silu" else v.abs())


def act_extra(v, kind):
    """Roundings in which the kernel's formula differs from torch's, in units of act_unit: none for SiLU (the same expression); GELU:
    the kernel's cube ((c v) v) v against torch's c ((v v) v), three roundings of the cubic term carried through
    0.5 |v| (1 - tanh^2) sqrt(2 / pi)."""
    if kind == "silu":
        return torch.zeros_like(v)
    t = torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3))
    return 0.5 * (1 - t * t) * math.sqrt(2.0 / math.pi) * 3 * 0.044715 * v.abs() ** 3


def act_yardstick(run, kind):
    """torch's own fp32 activation on this device on every v the probes use (integers and half-integers in [-8, 8]): its worst
    elementwise error against float64, in units of act_unit."""
    v = torch.arange(-16, 17, dtype=torch.float64) / 2
    got = run.torch_act(v, kind)
    unit = act_unit(v, kind)
    e = (got - act64(v, kind)).abs()
    return float(torch.where(e == 0, torch.zeros_like(e), e / unit).max())


def act_bound(v, kind, yard):
    return (yard + act_extra(v, kind)) * act_unit(v, kind) * (1 + 2.0 ** -10)


class Geom:
    """Latent [C, F, H, W], patch (pt, ph, pw), token grid (gf, gh, gw)."""

    def __init__(self, C, patch, grid=(3, 5, 7)):
        self.C, self.patch, self.grid = C, tuple(patch), tuple(grid)
        (self.pt, self.ph, self.pw), (self.gf, self.gh, self.gw) = patch, grid
        self.F, self.H, self.W = self.gf * self.pt, self.gh * self.ph, self.gw * self.pw
        self.L, self.K = self.gf * self.gh * self.gw, C * self.pt * self.ph * self.pw
        self.numel = C * self.F * self.H * self.W

    def conv_index(self):
        """int64 [L, K]: the flat latent index of element k = ((c pt + dt) ph + dh) pw + dw of token (f, h, w): Conv3d with kernel ==
        stride, weight.flatten(1), tokens as .flatten(2) orders them.  Built from meshgrids, no division."""
        f, h, w, c, dt, dh, dw = torch.meshgrid(*[torch.arange(n) for n in (self.gf, self.gh, self.gw, self.C, self.pt, self.ph, self.pw)], indexing="ij")
        idx = ((c * self.F + f * self.pt + dt) * self.H + h * self.ph + dh) * self.W + w * self.pw + dw
        return idx.reshape(self.L, self.K)

    def unpatchify(self, rows):
        """model.py's unpatchify of [L, C pt ph pw] -> [C, F, H, W]."""
        u = rows[:self.L].reshape(*self.grid, *self.patch, self.C)
        return torch.einsum("fhwpqrc->cfphqwr", u).reshape(self.C, self.F, self.H, self.W)

    def args(self):
        return (self.C, self.F, self.H, self.W, self.pt, self.ph, self.pw)


# ================================================================================================ the GPU runner
class GpuRun:
    """One launch per call through the C ABI.  Operands are float64 tensors of values exact in fp32; each is copied into its own
    sentinel-guarded window; the output is a fresh sentinel-filled window."""
    dev = DEV

    def _go(self, rc):
        from viditq_extension import _C

        torch.cuda.synchronize()
        assert rc == WANQ_OK, (rc, _C.lib.wanq_last_error().decode())

    def _in(self, t, shape=None):
        return None if t is None else Window(t.shape if shape is None else shape, DEV, t)

    @staticmethod
    def _p(w):
        return None if w is None else w.ptr()

    def linear(self, x, w, bias, M, in_act=None, out_act=None):
        from viditq_extension import _C

        (N, K), x_rows = w.shape, x.shape[0]
        xs, ws, bs, win = self._in(x), self._in(w), self._in(bias), Window((M, N), DEV)
        self._go(_C.lib.wanq_linear_f32(xs.ptr(), x_rows, ws.ptr(), self._p(bs), win.ptr(), M, N, K, ACTS[in_act], ACTS[out_act], _C.stream()))
        return Result(win, [])

    def patch(self, g, latent, w, bias, out_rows):
        from viditq_extension import _C

        N = w.shape[0]
        ls, ws, bs, win = self._in(latent), self._in(w), self._in(bias), Window((out_rows, N), DEV)
        self._go(_C.lib.wanq_patch_embed(ls.ptr(), ws.ptr(), self._p(bs), win.ptr(), *g.args(), N, out_rows, _C.stream()))
        return Result(win, [])

    def head(self, x, mod, e, w, bias, eps, g=None):
        from viditq_extension import _C

        (rows, K), N = x.shape, w.shape[0]
        xs, ms, es, ws, bs = self._in(x), self._in(mod), self._in(e), self._in(w), self._in(bias)
        win = Window((rows, N) if g is None else (g.C, g.F, g.H, g.W), DEV)
        geo = (0,) * 8 if g is None else (1,) + g.args()
        self._go(_C.lib.wanq_head_fwd(xs.ptr(), ms.ptr(), es.ptr(), ws.ptr(), self._p(bs), win.ptr(), rows, K, N, eps, *geo, _C.stream()))
        return Result(win, [])

    def sinusoid(self, t, kind, dim):
        """t: a numpy array of the dtype the kind names (0 float32, 1 int64, 2 float64, 3 int32)."""
        from viditq_extension import _C

        n = len(t)
        raw = torch.full((GUARD * 4 * 2 + t.nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        raw[GUARD * 4:GUARD * 4 + t.nbytes] = torch.from_numpy(t.view(np.uint8).copy()).to(DEV)
        win = Window((n, dim), DEV)
        self._go(_C.lib.wanq_time_sinusoid(raw.data_ptr() + GUARD * 4, kind, win.ptr(), n, dim, _C.stream()))
        return Result(win, [])

    def lincomb(self, coef, ins, numel, alias=None):
        """coef [n_out, n_in]; ins: list of float64 [numel]; alias {o: i}: output o IS input i.  -> list of Results."""
        from viditq_extension import _C

        n_out, n_in = coef.shape
        alias = alias or {}
        iw = [Window((numel,), DEV, t) for t in ins]
        ow = [iw[alias[o]] if o in alias else Window((numel,), DEV) for o in range(n_out)]
        c = (ctypes.c_float * (n_out * n_in))(*[float(v) for v in coef.flatten().tolist()])
        pin, pout = (ctypes.c_void_p * n_in)(*[w.ptr() for w in iw]), (ctypes.c_void_p * n_out)(*[w.ptr() for w in ow])
        self._go(_C.lib.wanq_lincomb(n_out, n_in, ctypes.cast(c, ctypes.c_void_p), ctypes.cast(pin, ctypes.c_void_p),
                                     ctypes.cast(pout, ctypes.c_void_p), numel, _C.stream()))
        fails = []
        for i, w in enumerate(iw):
            if i not in alias.values():
                fails += guard_failures(w, f"input {i}")
                if not torch.equal(w.window().double(), ins[i].to(DEV)):
                    fails.append(f"input {i} was written")
        return [Result(w, fails) for w in ow]

    def torch_act(self, v, kind):
        x = v.float().to(DEV)
        y = torch.nn.functional.silu(x) if kind == "silu" else torch.nn.functional.gelu(x, approximate="tanh")
        return y.double().cpu()


# ================================================================================================ A. Linear, exact
LIN_MS, LIN_NS, LIN_KS = (1, 2, 3, 4, 5, 63, 64, 65, 129), (1, 3, 5, 63, 64, 65, 130), (16, 32, 48, 240, 256, 272)
GEMV_MS, TILE_MS = LIN_MS[:4], LIN_MS[4:]


def x_rows_of(M, kind):
    return (0, 1, M - 1, M)[kind]


def linear_table():
    """(M, N, K, x_rows): per kernel every (K, N) pair, M and the x_rows kind by rotations; M = 4 with x_rows = 2 on the gemv.
    test_tables_reach_every_case proves what this reaches."""
    cases = []
    for ms in (GEMV_MS, TILE_MS):
        for i, K in enumerate(LIN_KS):
            for j, N in enumerate(LIN_NS):
                M = ms[(i + j) % len(ms)]
                cases.append((M, N, K, x_rows_of(M, (i + 2 * j + len(ms)) % 4)))
    cases += [(4, 5, 272, 2), (4, 130, 16, 2)]
    for M in LIN_MS:  # every M with every x_rows kind
        cases += [(M, 65, 48, x_rows_of(M, kind)) for kind in range(4)]
    return list(dict.fromkeys(cases))


LIN_CASES = linear_table()


class LinCase:
    """x in [-4, 4], w in [-255, 255], bias in [-999, 999], hashed integers; rows >= x_rows do not exist.  K <= 272: |y| < 2^24."""

    def __init__(self, M, N, K, x_rows):
        self.M = M
        self.x, self.w = ints(x_rows, K, 11, -4, 4).double(), ints(N, K, 12, -255, 255).double()
        self.bias = ints(N, None, 13, -999, 999).double()
        xp = torch.cat([self.x, torch.zeros(M - x_rows, K, dtype=torch.float64)])
        self.y64 = xp @ self.w.T + self.bias[None, :]
        assert float((xp.abs() @ self.w.abs().T).max()) + 999 < 2 ** 24 and K <= 272


def probe_linear_exact(run, M, N, K, x_rows):
    case = LinCase(M, N, K, x_rows)
    fails = check_exact(run.linear(case.x, case.w, case.bias, M), case.y64)
    if x_rows < M and not torch.equal(case.y64[x_rows:], case.bias[None, :].expand(M - x_rows, N)):
        fails.append("builder: padded rows are not the bias row")
    return fails


@gpu
@pytest.mark.parametrize("K", LIN_KS)
def test_linear_exact_over_the_shape_table(K):
    """Every case of the table at this K: the exact integer x w^T + b, rows [x_rows, M) the bias row, guards intact."""
    run, fails, n = GpuRun(), [], 0
    for M, N, k, xr in LIN_CASES:
        if k == K:
            fails += [f"({M}, {N}, {K}) x_rows {xr}: {f}" for f in probe_linear_exact(run, M, N, K, xr)]
            n += 1
    assert n >= 14
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


def probe_linear_one_hot(run, M, N, K, k0=0):
    """Row m of x is e_k, k = (k0 + m) mod K: the output row is weight column k.  A failure names the k that went missing."""
    w = ints(N, K, 14, -255, 255)
    if N >= 3:
        assert len({tuple(c.tolist()) for c in w.T}) == K  # pairwise different columns
    ks = (k0 + torch.arange(M)) % K
    x = torch.zeros(M, K, dtype=torch.float64)
    x[torch.arange(M), ks] = 1.0

    def describe(at, got):
        k = int(ks[at[0]])
        others = (w[at[1]].double() == got).nonzero().flatten().tolist()
        return f"k = {k} (K-step {k // BK}, lane {k % 256 // 4}, turn {k // 256}); the value is that of k in {others[:4]}"

    return check_exact(run.linear(x, w.double(), None, M), w.T[ks].double(), describe)


ONE_HOT = [(273, 65, 272, 0), (65, 130, 48, 0), (64, 5, 16, 0), (257, 3, 256, 0)] + \
          [(4, 5, 272, k0) for k0 in (0, 252, 254, 268)] + [(3, 130, 16, 0), (4, 65, 16, 12), (2, 3, 256, 255), (1, 63, 240, 239)]


@gpu
def test_linear_one_hot_rows_return_the_weight_column():
    run, fails = GpuRun(), []
    for M, N, K, k0 in ONE_HOT:
        fails += [f"({M}, {N}, {K}) k0 {k0}: {f}" for f in probe_linear_one_hot(run, M, N, K, k0)]
    assert not fails, "\n".join(fails[:20])


ACT_SHAPES = [(4, 65, 48, 2), (4, 5, 272, 3), (66, 65, 48, 60), (129, 130, 32, 129)]  # (M, N, K, x_rows): gemv twice, tile twice


def probe_out_act(run, kind, yard, M, N, K, x_rows, salt=0):
    """x[m, k_m] = c_m, w = 1/2 everywhere, bias b_n in {-1, 0, 1}: the pre-activation is v = c_m / 2 + b_n exactly, an integer or
    half-integer in [-8, 8]; rows [x_rows, M) get v = b_n.  out = act(v) under the bound; act(0) == 0 exactly."""
    c = ints(x_rows, None, 15 + salt, -14, 14).double()
    ks = (torch.arange(x_rows) * 7 + salt) % K
    x = torch.zeros(x_rows, K, dtype=torch.float64)
    x[torch.arange(x_rows), ks] = c
    w = torch.full((N, K), 0.5, dtype=torch.float64)
    b = ints(N, None, 16 + salt, -1, 1).double()
    v = torch.cat([c, torch.zeros(M - x_rows, dtype=torch.float64)])[:, None] / 2 + b[None, :]
    assert float(v.abs().max()) <= 8 and torch.equal(v * 2, torch.round(v * 2))
    res = run.linear(x, w, b, M, out_act=kind)
    fails, ratio = check_bound(res, act64(v, kind), act_bound(v, kind, yard))
    zero = (v == 0).to(res.win.flat.device)
    if bool((res.win.bits()[zero] != 0).any()):  # as bits: +0.0
        fails.append(f"act_out(0) != +0.0 for {kind}")
    return fails, ratio, set((v * 2).long().flatten().tolist())


def probe_in_act(run, kind, yard, M, N, K, x_rows, salt=0):
    """x[m, k_m] = v_m = c_m / 2 in [-8, 8], zeros elsewhere; w[n, k] = 2^e, e = (n + k) % 5 - 2; no bias: out = act(v_m) 2^e, where the
    scaling is exact and every other term is act(0) w = 0.  Rows [x_rows, M) are exactly 0."""
    c = ints(x_rows, None, 17 + salt, -16, 16).double()
    ks = (torch.arange(x_rows) * 5 + salt) % K
    x = torch.zeros(x_rows, K, dtype=torch.float64)
    x[torch.arange(x_rows), ks] = c / 2
    e = (torch.arange(N)[:, None] + torch.arange(K)[None, :]) % 5 - 2
    w = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[e + 2]
    v = torch.cat([c / 2, torch.zeros(M - x_rows, dtype=torch.float64)])
    scale = torch.cat([w[:, ks].T, torch.zeros(M - x_rows, N, dtype=torch.float64)])
    ref, bound = act64(v, kind)[:, None] * scale, act_bound(v, kind, yard)[:, None] * scale
    res = run.linear(x, w, None, M, in_act=kind)
    fails, ratio = check_bound(res, ref, bound)
    zero = (v == 0).to(res.win.flat.device)
    if bool((res.win.bits()[zero] != 0).any()):  # as bits: +0.0
        fails.append(f"act_in(0) != +0.0 for {kind}: the zero padding relies on it")
    return fails, ratio, set(c.long().tolist())


@gpu
@pytest.mark.parametrize("kind", ["silu", "gelu"])
def test_linear_activations_on_exact_preactivations(kind):
    """Both sides, both kernels; the bound is torch's own worst fp32 error on the same values plus the roundings in which the kernel's
    formula differs (act_extra)."""
    run = GpuRun()
    yard = act_yardstick(run, kind)
    fails, worst, seen_out, seen_in = [], {"out": 0.0, "in": 0.0}, set(), set()
    for M, N, K, xr in ACT_SHAPES:
        for salt in range(3):
            f, r, s = probe_out_act(run, kind, yard, M, N, K, xr, salt)
            fails += [f"out_act ({M}, {N}, {K}): {x}" for x in f]
            worst["out"], seen_out = max(worst["out"], r), seen_out | s
            f, r, s = probe_in_act(run, kind, yard, M, N, K, xr, salt)
            fails += [f"in_act ({M}, {N}, {K}): {x}" for x in f]
            worst["in"], seen_in = max(worst["in"], r), seen_in | s
    print(f"RATIO act {kind}: torch's worst error {yard:.3f} units; kernel err / bound out_act {worst['out']:.3f} in_act {worst['in']:.3f}")
    assert seen_out >= set(range(-16, 17)) and seen_in >= set(range(-16, 17))  # every integer and half-integer of [-8, 8] was used
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ B. patch embedding, exact
GEOMS = [(2, (1, 2, 4)), (4, (1, 2, 4)), (6, (1, 2, 4)), (8, (1, 2, 4)), (2, (2, 1, 4)), (4, (4, 2, 1)), (36, (1, 2, 2)), (5, (2, 2, 4))]
PATCH_NS = (4, 60, 64, 68, 132)


def out_rows_of(L, kind):
    return (L, L + 1, L + 64 + 3)[kind]


def probe_patch_index(run, g, N, out_rows, with_bias, shift=0):
    """The latent holds its own flat index, weight row n is one-hot at k = (n + shift) mod K: out[tok, n] is the index Conv3d gathers
    (+ an integer bias).  Rows [L, out_rows) are exactly 0 and the element behind the last row keeps the sentinel (the guard)."""
    assert g.numel < 2 ** 24
    latent = torch.arange(g.numel, dtype=torch.float64).reshape(g.C, g.F, g.H, g.W)
    ks = (torch.arange(N) + shift) % g.K
    w = torch.zeros(N, g.K, dtype=torch.float64)
    w[torch.arange(N), ks] = 1.0
    bias = ints(N, None, 21, -999, 999).double() if with_bias else None
    idx = g.conv_index()
    expect = torch.zeros(out_rows, N, dtype=torch.float64)
    expect[:g.L] = idx[:, ks].double() + (bias[None, :] if with_bias else 0.0)
    assert float(expect.abs().max()) < 2 ** 24

    def describe(at, got):
        tok, k = at[0], int(ks[at[1]])
        if tok >= g.L:
            return f"row {tok} lies behind the {g.L} tokens and must be 0"
        dw, dh, dt, c = k % g.pw, k // g.pw % g.ph, k // (g.pw * g.ph) % g.pt, k // (g.pw * g.ph * g.pt)
        return f"token {tok} = (f, h, w) {(tok // (g.gh * g.gw), tok // g.gw % g.gh, tok % g.gw)}, k = {k} = (c, dt, dh, dw) {(c, dt, dh, dw)}"

    return check_exact(run.patch(g, latent, w, bias, out_rows), expect, describe)


def probe_patch_dense(run, g, N, out_rows):
    """latent in [-4, 4], w in [-255, 255], integer bias: the exact integer Conv3d gives."""
    latent = ints(g.numel, None, 22, -4, 4).double().reshape(g.C, g.F, g.H, g.W)
    w, bias = ints(N, g.K, 23, -255, 255).double(), ints(N, None, 24, -999, 999).double()
    ref = torch.nn.functional.conv3d(latent[None], w.reshape(N, g.C, *g.patch), bias, stride=g.patch).flatten(2).transpose(1, 2)[0]
    assert torch.equal(ref, latent.flatten()[g.conv_index()] @ w.T + bias[None, :]) and float(ref.abs().max()) < 2 ** 24
    expect = torch.cat([ref, torch.zeros(out_rows - g.L, N, dtype=torch.float64)])
    return check_exact(run.patch(g, latent, w, bias, out_rows), expect)


def patch_table():
    """(geometry, N, out_rows kind, bias, shift): every geometry with every N; out_rows kinds and NULL bias by rotation; the K = 144
    geometry (the only K above the largest N, 132) a second time with shifted one-hot rows so that every k is asked for."""
    cases = []
    for gi, (C, patch) in enumerate(GEOMS):
        K = C * patch[0] * patch[1] * patch[2]
        for ni, N in enumerate(PATCH_NS):
            cases.append((gi, N, (gi + ni) % 3, (gi + ni) % 4 != 0, 0))
        if K > 132:
            cases.append((gi, 132, 2, True, K - 132))
    return cases


PATCH_CASES = patch_table()


@gpu
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_patch_embed_returns_the_index_conv3d_gathers(gi):
    run, g, fails = GpuRun(), Geom(*GEOMS[gi]), []
    for _, N, ok, with_bias, shift in [c for c in PATCH_CASES if c[0] == gi]:
        fails += [f"C {g.C} patch {g.patch} N {N} out_rows {out_rows_of(g.L, ok)} bias {with_bias}: {f}"
                  for f in probe_patch_index(run, g, N, out_rows_of(g.L, ok), with_bias, shift)]
    fails += [f"dense C {g.C} patch {g.patch}: {f}" for f in probe_patch_dense(run, g, 132, g.L + 67)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ C. head
HEAD_KS, HEAD_ROWS, HEAD_NS = (16, 48, 256, 272), (1, 63, 64, 65, 105), (1, 16, 64, 65, 130)
UNPATCH = [(16, (1, 2, 2)), (2, (2, 2, 4)), (3, (2, 1, 2)), (1, (1, 1, 1))]


class HeadCase:
    """Rows x = m_r + a_r s, s = +-1 with exactly K / 2 of each (placed by a hash), m_r an integer, a_r a power of two (or 0: constant
    rows).  modulation and e are integers such that G = 1 + scale + e in [1, 4] and S = shift + e in [-3, 3] are hashed per column;
    w in [-3, 3] (or one-hot rows with bias 1000 n), integer bias."""

    def __init__(self, rows, K, N, m=None, a=None, one_hot=False):
        r = torch.arange(rows)
        order = torch.argsort(hash32(r[:, None], torch.arange(K)[None, :], 31), dim=1)
        self.s = torch.ones(rows, K, dtype=torch.float64)
        self.s.scatter_(1, order[:, :K // 2], -1.0)
        assert bool((self.s.sum(1) == 0).all())
        self.m = (ints(rows, None, 32, -200, 200).double() if m is None else torch.full((rows,), float(m), dtype=torch.float64))
        self.a = (torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)[r % 3] if a is None else torch.full((rows,), float(a), dtype=torch.float64))
        self.x = self.m[:, None] + self.a[:, None] * self.s
        self.e = ints(K, None, 33, -2, 2).double()
        self.G, self.S = ints(K, None, 34, 1, 4).double(), ints(K, None, 35, -3, 3).double()
        self.mod = torch.stack([self.S - self.e, self.G - 1 - self.e])  # [shift row, scale row]
        if one_hot:
            self.w = torch.zeros(N, K, dtype=torch.float64)
            self.w[torch.arange(N), torch.arange(N) % K] = 1.0
            self.bias = 1000.0 * torch.arange(N, dtype=torch.float64)
        else:
            self.w, self.bias = ints(N, K, 36, -3, 3).double(), ints(N, None, 37, -8, 8).double()
        self.rows, self.K, self.N = rows, K, N
        assert exact_f32(self.x) and float(self.x.abs().max()) * K < 2 ** 24

    def reference(self, eps):
        """(float64 reference, bound) of the plain output [rows, N]: profiles/PARITY_NOTES.md, "Derivation of the head bound".  eps is
        the fp32 value the ABI carries."""
        K, eps = self.K, float(np.float32(eps))
        x = self.x
        mean = x.mean(1, keepdim=True)
        d = x - mean
        var = (d * d).mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        z = d * rstd
        xm = z * self.G[None, :] + self.S[None, :]
        ref = xm @ self.w.T + self.bias[None, :]
        k = 2 + -(-K // 256) + 6  # additions between an element and the row total: in the float4, per lane turn, six exchange steps
        A = x.abs().amax(1, keepdim=True)
        # integer rows with K A < 2^24 are summed exactly in any order, and K mean is that sum: the quotient is the representable mean
        exact_mean = torch.equal(x, torch.round(x)) and float(A.max()) * K < 2 ** 24 and exact_f32(mean)
        c = torch.zeros_like(A) if exact_mean else (k + 1) * U * A * rstd
        theta = (k + 4) * U + c * c
        rho = (theta + U) / 2 + 2 * U * RSQ_ULP
        dz = z.abs() * (rho + 2 * U) + c
        dxm = (self.G[None, :] * dz + U * (z * self.G[None, :]).abs() + U * xm.abs()) * (1 + 2.0 ** -10)
        bound = dxm @ self.w.abs().T + (K + 1) * U * (xm.abs() @ self.w.abs().T + self.bias.abs()[None, :]) * (1 + 2.0 ** -10)
        return ref, bound + 2.0 ** -126


def head_table():
    return [(HEAD_ROWS[(i + j) % 5], K, N) for i, K in enumerate(HEAD_KS) for j, N in enumerate(HEAD_NS)] + \
           [(rows, 48, 65) for rows in HEAD_ROWS]


HEAD_CASES = list(dict.fromkeys(head_table()))


def probe_head_constant(run, rows, K, N, g=None):
    """Constant rows at eps = 1e-6: every deviation is exactly 0, the operand is S, the output the exact integer S w^T + b."""
    case = HeadCase(rows, K, N, a=0.0, one_hot=g is not None)
    expect = case.S[None, :].expand(rows, K) @ case.w.T + case.bias[None, :]
    assert exact_f32(expect)
    return check_exact(run.head(case.x, case.mod, case.e, case.w, case.bias, 1e-6, g), expect if g is None else g.unpatchify(expect))


def probe_head_bound(run, rows, K, N, eps=1e-6, m=None, a=None):
    case = HeadCase(rows, K, N, m=m, a=a)
    ref, bound = case.reference(eps)
    assert float(bound.max()) < 0.25  # far below the 1 by which a dropped, swapped or misplaced term moves a result
    return check_bound(run.head(case.x, case.mod, case.e, case.w, case.bias, eps), ref, bound)


@gpu
@pytest.mark.parametrize("K", HEAD_KS)
def test_head_plain_constant_rows_exactly_and_signed_rows_under_the_bound(K):
    run, fails, worst = GpuRun(), [], 0.0
    for rows, k, N in HEAD_CASES:
        if k == K:
            fails += [f"constant ({rows}, {K}, {N}): {f}" for f in probe_head_constant(run, rows, K, N)]
            f, ratio = probe_head_bound(run, rows, K, N)
            fails += [f"bound ({rows}, {K}, {N}): {x}" for x in f]
            worst = max(worst, ratio)
    print(f"RATIO head plain K {K}: {worst:.3f}")
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


def probe_head_eps(run, K=48, rows=65, N=16):
    """Rows +-2^-10 (variance 2^-20) at eps 0, 1e-6 and 3 2^-20, each under the bound; the last halves the normalised row: with
    P = S w^T + b (the constant-row result), out(3 2^-20) - P = (out(0) - P) / 2 within the two bounds.  Then m_r = 4096, a_r = 1."""
    fails, ratios, outs = [], [], {}
    case = HeadCase(rows, K, N, m=0.0, a=2.0 ** -10)
    P = (case.S[None, :].expand(rows, K) @ case.w.T + case.bias[None, :])
    for eps in (0.0, 1e-6, 3 * 2.0 ** -20):
        ref, bound = case.reference(eps)
        res = run.head(case.x, case.mod, case.e, case.w, case.bias, eps)
        f, r = check_bound(res, ref, bound)
        fails += [f"eps {eps}: {x}" for x in f]
        ratios.append(r)
        outs[eps] = (res.win.window().double().cpu(), bound, ref)
    (o0, b0, r0), (o3, b3, r3) = outs[0.0], outs[3 * 2.0 ** -20]
    assert torch.equal((r3 - P) * 2, r0 - P) or float(((r3 - P) * 2 - (r0 - P)).abs().max()) < 1e-12
    assert float((r0 - P).abs().max()) >= 1  # the normalised part is visible
    if not bool((((o3 - P) * 2 - (o0 - P)).abs() <= 2 * b3 + b0).all()):
        fails.append("eps = 3 var does not halve the normalised row")
    f, r = probe_head_bound(run, rows, K, N, m=4096.0, a=1.0)
    fails += [f"m_r = 4096: {x}" for x in f]
    ratios.append(r)
    return fails, ratios


@gpu
def test_head_eps_enters_under_the_square_root():
    fails, ratios = probe_head_eps(GpuRun())
    print("RATIO head eps 0 / 1e-6 / 3 var / offset 4096: " + " ".join(f"{r:.3f}" for r in ratios))
    assert not fails, "\n".join(fails[:20])


def probe_unpatchify(run, C, patch, K):
    """One-hot weight rows with bias 1000 n, so that each latent element names (token, n): the float64 reference through model.py's
    unpatchify under the bound; every element written; bit-equal to the plain output through the host unpatchify; constant rows exactly."""
    g = Geom(C, patch)
    N = g.K
    case = HeadCase(g.L, K, N, one_hot=True)
    ref, bound = case.reference(1e-6)
    res = run.head(case.x, case.mod, case.e, case.w, case.bias, 1e-6, g)
    fails, ratio = check_bound(res, g.unpatchify(ref), g.unpatchify(bound))
    if bool((res.win.bits() == SENT).any()):
        fails.append(f"{int((res.win.bits() == SENT).sum())} latent elements were never written")
    plain = run.head(case.x, case.mod, case.e, case.w, case.bias, 1e-6)
    fails += [f"plain: {f}" for f in check_bound(plain, ref, bound)[0]]
    if not torch.equal(g.unpatchify(plain.win.bits()), res.win.bits()):
        fails.append("the scattered output is not bit-equal to the plain output through the host unpatchify")
    fails += [f"constant rows: {f}" for f in probe_head_constant(run, g.L, K, N, g)]
    return fails, ratio


@gpu
@pytest.mark.parametrize("ui", range(len(UNPATCH)))
def test_head_unpatchify_puts_every_element_where_the_model_does(ui):
    C, patch = UNPATCH[ui]
    fails, ratio = probe_unpatchify(GpuRun(), C, patch, HEAD_KS[ui])
    print(f"RATIO head unpatchify C {C} patch {patch} K {HEAD_KS[ui]}: {ratio:.3f}")
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ D. isolation
def _compare(name, clean, res, mask, nonfinite=True):
    """Everything outside `mask` is bit-equal to the clean run; inside it every element is non-finite (when asked)."""
    out = [f"{name}: {f}" for f in list(res.fails) + guard_failures(res.win)]
    mask = mask.to(res.win.flat.device)
    moved = (res.win.bits() != clean.win.bits()) & ~mask
    if bool(moved.any()):
        at = tuple(int(v) for v in moved.nonzero()[0])
        out.append(f"{name}: {int(moved.sum())} elements outside the poisoned part changed; first at {at}: {res.win.window()[at].item()} "
                   f"was {clean.win.window()[at].item()}")
    if nonfinite and bool(torch.isfinite(res.win.window())[mask].any()):
        out.append(f"{name}: finite elements inside the poisoned part")
    if not nonfinite and not bool((res.win.bits() != clean.win.bits())[mask].any()):
        out.append(f"{name}: the poisoned part did not change")
    return out


def _masks(M, N):
    return (lambda r: (torch.arange(M) == r)[:, None].expand(M, N)), (lambda c: (torch.arange(N) == c)[None, :].expand(M, N))


def probe_isolation_linear(run, M, N, K):
    case = LinCase(M, N, K, M)
    clean = run.linear(case.x, case.w, case.bias, M)
    fails = [f"clean: {f}" for f in check_exact(clean, case.y64)]
    row, col = _masks(M, N)
    x2 = case.x.clone()
    x2[M // 2] *= 2.0 ** 50
    fails += _compare(f"row {M // 2} of magnitude 2^50", clean, run.linear(x2, case.w, case.bias, M), row(M // 2), False)
    x2 = case.x.clone()
    x2[M - 1, 1], x2[M - 1, K - 2] = float("nan"), float("inf")
    fails += _compare(f"NaN and Inf in x row {M - 1}", clean, run.linear(x2, case.w, case.bias, M), row(M - 1))
    w2 = case.w.clone()
    w2[N - 1, 2], w2[N - 1, K - 1] = float("nan"), float("inf")
    fails += _compare(f"NaN and Inf in w row {N - 1}", clean, run.linear(case.x, w2, case.bias, M), col(N - 1))
    return fails


def probe_isolation_patch(run, gi, N=68):
    g = Geom(*GEOMS[gi])
    latent = ints(g.numel, None, 22, -4, 4).double().reshape(g.C, g.F, g.H, g.W)
    w, bias = ints(N, g.K, 23, -255, 255).double(), ints(N, None, 24, -999, 999).double()
    rows = g.L + 3
    clean = run.patch(g, latent, w, bias, rows)
    expect = torch.cat([latent.flatten()[g.conv_index()] @ w.T + bias[None, :], torch.zeros(3, N, dtype=torch.float64)])
    fails = [f"clean: {f}" for f in check_exact(clean, expect)]
    row, col = _masks(rows, N)
    idx = g.conv_index()
    l2 = latent.clone().flatten()
    l2[idx[g.L // 2]] *= 2.0 ** 50
    fails += _compare("a patch of magnitude 2^50", clean, run.patch(g, l2.reshape(latent.shape), w, bias, rows), row(g.L // 2), False)
    l2 = latent.clone().flatten()
    l2[idx[g.L - 1, 0]], l2[idx[g.L - 1, g.K - 1]] = float("nan"), float("inf")
    fails += _compare("NaN and Inf in the last token's patch", clean, run.patch(g, l2.reshape(latent.shape), w, bias, rows), row(g.L - 1))
    w2 = w.clone()
    w2[N - 1, 0], w2[N - 1, g.K - 1] = float("nan"), float("inf")
    # 0 x NaN is a NaN: the zero rows behind the tokens are stored as 0, not computed
    fails += _compare(f"NaN and Inf in w row {N - 1}", clean, run.patch(g, latent, w2, bias, rows), col(N - 1) & (torch.arange(rows) < g.L)[:, None])
    return fails


def probe_isolation_head(run, rows, K, N, g=None):
    case = HeadCase(rows, K, N, one_hot=g is not None)
    args = (case.mod, case.e, case.w, case.bias, 1e-6, g)
    clean = run.head(case.x, *args)
    row, col = _masks(rows, N)
    lat = (lambda m: m) if g is None else (lambda m: g.unpatchify(m.double()).bool())
    x2 = case.x.clone()
    x2[rows // 2] *= 2.0 ** 50
    res = run.head(x2, *args)
    # LayerNorm removes the scale: the row itself may come out unchanged
    fails = [f for f in _compare("a row of magnitude 2^50", clean, res, lat(row(rows // 2)), False) if "did not change" not in f]
    if not bool(torch.isfinite(res.win.window()).all()):
        fails.append("a row of magnitude 2^50 is not finite after the LayerNorm")
    x2 = case.x.clone()
    x2[rows - 1, 1], x2[rows - 1, K - 2] = float("nan"), float("inf")
    fails += _compare(f"NaN and Inf in x row {rows - 1}", clean, run.head(x2, *args), lat(row(rows - 1)))
    w2 = case.w.clone()
    w2[N - 1, 2], w2[N - 1, K - 1] = float("nan"), float("inf")
    fails += _compare(f"NaN and Inf in w row {N - 1}", clean, run.head(case.x, case.mod, case.e, w2, case.bias, 1e-6, g), lat(col(N - 1)))
    return fails


ISO_LINEAR = [(129, 130, 48), (128, 65, 32), (4, 5, 272)]  # row M - 1 alone in the last tile; the last tile's last row; the gemv
ISO_HEAD = [(129, 48, 65, None), (128, 16, 130, None), (105, 48, 64, 0), (105, 16, 12, 2)]  # (rows, K, N, index into UNPATCH)


@gpu
def test_disturbances_stay_where_the_definition_puts_them():
    run, fails = GpuRun(), []
    for M, N, K in ISO_LINEAR:
        fails += [f"linear ({M}, {N}, {K}): {f}" for f in probe_isolation_linear(run, M, N, K)]
    for gi in (1, 4, 6):  # NK4 = 8, pt = 2, the tile kernel's gather
        fails += [f"patch {GEOMS[gi]}: {f}" for f in probe_isolation_patch(run, gi)]
    for rows, K, N, ui in ISO_HEAD:
        fails += [f"head ({rows}, {K}, {N}) {ui}: {f}" for f in probe_isolation_head(run, rows, K, N, None if ui is None else Geom(*UNPATCH[ui]))]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ E. time sinusoid
def sinusoid_reference(pos, dim):
    """sinusoidal_embedding_1d in numpy float64: (reference [n, dim], |angle| [n, dim])."""
    half = dim // 2
    ang = np.asarray(pos, np.float64)[:, None] * np.power(10000.0, -np.arange(half, dtype=np.float64) / half)[None, :]
    return np.concatenate([np.cos(ang), np.sin(ang)], 1), np.concatenate([np.abs(ang), np.abs(ang)], 1)


def sinusoid_bound(ref, ang):
    """One fp32 rounding of the result, plus twice (the device and numpy) the float64 terms: the angle carries the product's rounding, the
    rounding of the exponent's quotient through |y ln 10000| <= 9.3 and pow at 2 ulp, (1 + 9.3 + 4) 2^-53 |angle| in all, which cos / sin
    pass on at slope <= 1; cos / sin themselves 2 ulp of a value <= 1 (profiles/PARITY_NOTES.md)."""
    return U * np.abs(ref) + 2.0 ** -149 + 2 * (14.3 * 2.0 ** -53 * ang + 4 * 2.0 ** -53)


# pos = 0 comes first, so that the single-row call (n = 1) is the equality case and row 0 holds it in the five-row call
SIN_T = {0: np.array([0.0, 999.0, 500.25, 37.5, 0.1], np.float32), 1: np.array([0, 999, 2 ** 33 + 1, 37, 500], np.int64),
         2: np.array([0.0, 999.0, 500.1, 37.5, 1e-3], np.float64), 3: np.array([0, 999, -37, 500, 1], np.int32)}


def probe_sinusoid(run, kind, dim, n):
    t = SIN_T[kind][:n]
    if kind == 2 and n >= 3:
        assert np.float64(np.float32(t[2])) != t[2]  # a float64 timestep that a 32-bit read would change
    ref, ang = sinusoid_reference(t.astype(np.float64), dim)
    res = run.sinusoid(t, kind, dim)
    fails, ratio = check_bound(res, torch.from_numpy(ref), torch.from_numpy(sinusoid_bound(ref, ang)))
    half, got = dim // 2, res.win.bits().cpu()
    zero_rows = np.nonzero(t == 0)[0].tolist()
    assert zero_rows and zero_rows[0] == 0  # every call holds the equality case, in row 0
    one = int(np.float32(1.0).view(np.int32))
    for r in zero_rows:  # pos = 0: cos 1 first, then sin 0, as bits
        if not (bool((got[r, :half] == one).all()) and bool((got[r, half:] == 0).all())):
            fails.append(f"row {r} (pos = 0) is not [1 ... 1, 0 ... 0]")
    return fails, ratio


@gpu
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_time_sinusoid_reads_every_dtype_and_rounds_once(kind):
    run, fails, worst = GpuRun(), [], 0.0
    for dim in (2, 6, 64):
        for n in (1, 5):
            f, r = probe_sinusoid(run, kind, dim, n)
            fails += [f"kind {kind} dim {dim} n {n}: {x}" for x in f]
            worst = max(worst, r)
    print(f"RATIO sinusoid kind {kind}: {worst:.3f}")
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ F. lincomb, exact
BIG_NUMEL = 4 * (2048 * 256 + 5)


def lincomb_operands(n_out, n_in, numel):
    """in[i][e] = (7 e + 13 i) % 61 - 30 names (i, e mod 61); coef[o][i] = +-(1 + 8 o + i) names (o, i).  |out| <= 8 32 30 < 2^24."""
    e = torch.arange(numel, dtype=torch.int64)
    ins = [((7 * e + 13 * i) % 61 - 30).double() for i in range(n_in)]
    coef = torch.tensor([[(1 + 8 * o + i) * (-1) ** (o + i) for i in range(n_in)] for o in range(n_out)], dtype=torch.float64)
    return coef, ins, [sum(coef[o, i] * ins[i] for i in range(n_in)) for o in range(n_out)]


def probe_lincomb(run, n_out, n_in, numel, alias=None):
    coef, ins, expect = lincomb_operands(n_out, n_in, numel)
    fails = []
    for o, res in enumerate(run.lincomb(coef, ins, numel, alias)):
        fails += [f"output {o}: {f}" for f in check_exact(res, expect[o], lambda at, got: f"float4 {at[0] // 4}, grid-stride turn {at[0] // 4 // (2048 * 256)}")]
    return fails


@gpu
def test_lincomb_all_pairs_exactly():
    run, fails = GpuRun(), []
    for n_out in range(1, 5):
        for n_in in range(1, 9):
            for numel in (4, 1028):
                fails += [f"({n_out}, {n_in}) numel {numel}: {f}" for f in probe_lincomb(run, n_out, n_in, numel)]
    fails += [f"aliased: {f}" for f in probe_lincomb(run, 3, 4, 1028, {1: 2})]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
def test_lincomb_second_grid_stride_turn():
    fails = probe_lincomb(GpuRun(), 1, 2, BIG_NUMEL)
    assert not fails, "\n".join(fails)


# ================================================================================================ G. empty and refused calls
def _untouched(*wins):
    torch.cuda.synchronize()
    return all(bool((w.flat == SENT).all()) for w in wins)


def _edge_buffers():
    return {k: Window((4096,), DEV) for k in ("x", "w", "b", "m", "e", "out", "out2")}


@gpu
def test_empty_calls_are_ok_and_write_nothing():
    from viditq_extension import _C

    lib, st, b = _C.lib, _C.stream(), _edge_buffers()
    p = {k: v.ptr() for k, v in b.items()}
    assert lib.wanq_linear_f32(p["x"], 0, p["w"], p["b"], p["out"], 0, 8, 16, 0, 0, st) == WANQ_OK
    assert lib.wanq_head_fwd(p["x"], p["m"], p["e"], p["w"], p["b"], p["out"], 0, 16, 8, 1e-6, 0, 0, 0, 0, 0, 0, 0, 0, st) == WANQ_OK
    assert lib.wanq_time_sinusoid(p["x"], 0, p["out"], 0, 8, st) == WANQ_OK
    coef = (ctypes.c_float * 1)(1.0)
    pin, pout = (ctypes.c_void_p * 1)(p["x"]), (ctypes.c_void_p * 1)(p["out"])
    assert lib.wanq_lincomb(1, 1, ctypes.cast(coef, ctypes.c_void_p), ctypes.cast(pin, ctypes.c_void_p), ctypes.cast(pout, ctypes.c_void_p), 0, st) == WANQ_OK
    assert _untouched(*b.values())


def refusals(p, st, lib):
    """(name, thunk, expected code, a piece of the message): one per WANQ_REQUIRE that looks at more than a NULL pointer."""
    coef = (ctypes.c_float * 36)(*([1.0] * 36))
    pin, pout = (ctypes.c_void_p * 9)(*([p["x"]] * 9)), (ctypes.c_void_p * 4)(*([p["out"]] * 4))
    c, i, o = (ctypes.cast(v, ctypes.c_void_p) for v in (coef, pin, pout))
    lin = lambda x=p["x"], xr=4, M=8, N=8, K=16, ia=0, oa=0: lib.wanq_linear_f32(x, xr, p["w"], p["b"], p["out"], M, N, K, ia, oa, st)  # noqa: E731
    pe = lambda C=4, F=1, H=4, W=4, pt=1, ph=2, pw=2, N=8, rows=4, w=p["w"]: lib.wanq_patch_embed(p["x"], w, p["b"], p["out"], C, F, H, W, pt, ph, pw, N, rows, st)  # noqa: E731
    hd = lambda rows=4, K=16, N=16, un=1, C=4, F=1, H=4, W=4, x=p["x"]: lib.wanq_head_fwd(x, p["m"], p["e"], p["w"], p["b"], p["out"], rows, K, N, 1e-6, un, C, F, H, W, 1, 2, 2, st)  # noqa: E731
    return [
        ("linear K % 16", lambda: lin(K=24), WANQ_E_SHAPE, "multiple of 16"),
        ("linear x_rows > M", lambda: lin(xr=9), WANQ_E_SHAPE, "x_rows"),
        ("linear misaligned x", lambda: lin(x=p["x"] + 4), WANQ_E_ARG, "aligned"),
        ("linear in_act 3", lambda: lin(ia=3), WANQ_E_ARG, "activations"),
        ("linear out_act 3", lambda: lin(oa=3), WANQ_E_ARG, "activations"),
        ("linear N = 0", lambda: lin(N=0), WANQ_E_SHAPE, "N=0"),
        ("patch partial patches", lambda: pe(H=5), WANQ_E_SHAPE, "whole number"),
        ("patch K % 16", lambda: pe(C=3), WANQ_E_SHAPE, "multiple of 16"),
        ("patch N % 4", lambda: pe(N=6), WANQ_E_SHAPE, "multiple of 4"),
        ("patch out_rows < L", lambda: pe(rows=3), WANQ_E_SHAPE, "out_rows"),
        ("patch misaligned w", lambda: pe(w=p["w"] + 4), WANQ_E_ARG, "aligned"),
        ("patch empty dimension", lambda: pe(F=0), WANQ_E_SHAPE, "empty"),
        ("head K % 16", lambda: hd(K=24), WANQ_E_SHAPE, "multiple of 16"),
        ("head misaligned x", lambda: hd(x=p["x"] + 8), WANQ_E_ARG, "aligned"),
        ("head unpatchify N > 64", lambda: hd(N=80, C=20), WANQ_E_SHAPE, "at most 64"),
        ("head unpatchify N != C pt ph pw", lambda: hd(N=12), WANQ_E_SHAPE, "must be C"),
        ("head rows != tokens", lambda: hd(rows=5), WANQ_E_SHAPE, "token count"),
        ("head partial patches", lambda: hd(H=5), WANQ_E_SHAPE, "latent"),
        ("sinusoid t_kind 4", lambda: lib.wanq_time_sinusoid(p["x"], 4, p["out"], 2, 8, st), WANQ_E_ARG, "t_kind"),
        ("sinusoid odd dim", lambda: lib.wanq_time_sinusoid(p["x"], 0, p["out"], 2, 7, st), WANQ_E_SHAPE, "even"),
        ("lincomb numel % 4", lambda: lib.wanq_lincomb(1, 1, c, i, o, 6, st), WANQ_E_SHAPE, "multiple of 4"),
        ("lincomb n_in 9", lambda: lib.wanq_lincomb(1, 9, c, i, o, 8, st), WANQ_E_ARG, "n_in"),
        ("lincomb n_out 5", lambda: lib.wanq_lincomb(5, 1, c, i, o, 8, st), WANQ_E_ARG, "n_out"),
        ("lincomb misaligned output", lambda: lib.wanq_lincomb(1, 1, c, i, ctypes.cast((ctypes.c_void_p * 1)(p["out"] + 4), ctypes.c_void_p), 8, st),
         WANQ_E_ARG, "aligned"),
    ]


@gpu
def test_refused_calls_write_nothing():
    from viditq_extension import _C

    b = _edge_buffers()
    fails = []
    for name, call, code, piece in refusals({k: v.ptr() for k, v in b.items()}, _C.stream(), _C.lib):
        rc = call()
        msg = _C.lib.wanq_last_error().decode()
        if rc != code or piece not in msg:
            fails.append(f"{name}: returned {rc} ({msg!r}), expected {code} with {piece!r}")
        if not _untouched(*b.values()):
            fails.append(f"{name}: a window was written")
            break
    assert not fails, "\n".join(fails)


# ================================================================================================ H. CPU self-tests of the probes
def test_tables_reach_every_case():
    """Linear: every M, N, K and x_rows kind with every kernel it can reach, M = 4 with x_rows = 2, nk of 1, 2, 3, 15, 16, 17 (both LDS
    buffers last) and, on the gemv, 4 lanes, all lanes, a second turn.  Patch embedding: all four NK4, the tile gather, pt > 1 on
    both, every N and out_rows kind per kernel, NULL bias per kernel.  Head: every K, rows, N; both store forms.  All geometries have
    pairwise distinct patch extents (1 may repeat only where the issue's list does) and grid extents."""
    for name, ms in (("gemv", GEMV_MS), ("tile", TILE_MS)):
        mine = [c for c in LIN_CASES if c[0] in ms]
        assert {c[0] for c in mine} == set(ms) and {c[1] for c in mine} == set(LIN_NS) and {c[2] for c in mine} == set(LIN_KS), name
        for M in ms:
            assert {xr for m, n, k, xr in mine if m == M} >= {0, min(1, M), M - 1, M}, (name, M)
        assert {(c[1], c[2]) for c in mine} >= {(N, K) for N in LIN_NS for K in LIN_KS}
    assert (4, 5, 272, 2) in LIN_CASES
    assert [K // BK for K in LIN_KS] == [1, 2, 3, 15, 16, 17] and {K // BK % 2 for K in LIN_KS} == {0, 1}
    assert [min(64, K // 4) for K in LIN_KS[:1] + LIN_KS[4:]] == [4, 64, 64] and LIN_KS[-1] > 256
    assert all(max(c[:3]) <= 273 for c in LIN_CASES) and len(LIN_CASES) <= 130
    assert {k for m, n, K, k0 in ONE_HOT if m >= K for k in range(K)} >= set(range(272))
    assert any(m <= 4 and K > 256 and (k0 + m - 1) >= 256 for m, n, K, k0 in ONE_HOT)  # the gemv's second lane turn, one-hot
    geoms = [Geom(*x) for x in GEOMS]
    assert {g.K // 4 for g in geoms if g.K <= 64} == {4, 8, 12, 16} and {g.K for g in geoms if g.K > 64} == {80, 144}
    assert any(g.K <= 64 and g.pt > 1 for g in geoms) and any(g.K > 64 and g.pt > 1 for g in geoms)
    for g in geoms + [Geom(*x) for x in UNPATCH]:
        assert len({g.gf, g.gh, g.gw}) == 3 and g.L == 105 and g.numel < 2 ** 24
        assert g.patch == (1, 1, 1) or g.ph != g.pw or g.pt != g.ph  # the extents the issue lists: never all three equal
    for C, patch in GEOMS:
        assert patch[1] != patch[2] or (C, patch) == (36, (1, 2, 2))  # ph != pw but at the i2v width, which is Wan's own patch
    for gi, g in enumerate(geoms):
        mine = [c for c in PATCH_CASES if c[0] == gi]
        assert {c[1] for c in mine} == set(PATCH_NS) and {c[2] for c in mine} == {0, 1, 2} and any(not c[3] for c in mine), gi
        assert {int(k) for c in mine for k in (torch.arange(c[1]) + c[4]) % g.K} == set(range(g.K)), gi  # every k is asked for
    assert {c[1] for c in HEAD_CASES} == set(HEAD_KS) and {c[0] for c in HEAD_CASES} == set(HEAD_ROWS) and {c[2] for c in HEAD_CASES} == set(HEAD_NS)
    assert {(c[1], c[2]) for c in HEAD_CASES} >= {(K, N) for K in HEAD_KS for N in HEAD_NS}
    assert [Geom(*x).K for x in UNPATCH] == [64, 32, 12, 1]
    assert BIG_NUMEL // 4 > 2048 * 256 and BIG_NUMEL * 4 < 8.5e6


def test_gpu_part_is_marked():
    import inspect
    import sys

    first_cpu = inspect.getsourcelines(test_tables_reach_every_case)[1]
    for name, fn in list(vars(sys.modules[__name__]).items()):
        if name.startswith("test_") and inspect.isfunction(fn) and inspect.getsourcelines(fn)[1] < first_cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name


def test_expected_values_are_exact_in_fp32():
    """Linear: every partial sum in any order is an integer below 2^24 (LinCase asserts the absolute sums).  Patch embedding: indices
    below 2^24 plus a bias below 1000, one non-zero term per sum.  Head: constant rows give integer sums below 272 3 3 + 8.  lincomb:
    |out| <= 8 32 30.  Activations: v and the scalings 2^e are exact."""
    for M, N, K, xr in LIN_CASES:
        case = LinCase(M, N, K, xr)
        assert exact_f32(case.y64) and exact_f32(case.x) and exact_f32(case.w)
    for C, patch in GEOMS:
        g = Geom(C, patch)
        idx = g.conv_index()
        assert int(idx.max()) == g.numel - 1 and len(torch.unique(idx)) == g.numel  # every latent element belongs to exactly one (token, k)
    for rows, K, N in HEAD_CASES:
        case = HeadCase(rows, K, N, a=0.0)
        assert exact_f32(case.mod) and exact_f32(case.e) and float((case.S.abs()[None, :] @ case.w.abs().T).max()) + 8 < 2 ** 24
        assert torch.equal(1 + case.mod[1] + case.e, case.G) and torch.equal(case.mod[0] + case.e, case.S)
    coef, ins, expect = lincomb_operands(4, 8, 1028)
    assert all(exact_f32(t) for t in expect) and float(sum(c.abs().sum() for c in coef)) * 30 < 2 ** 24
    assert len({float(v) for v in coef.flatten()}) == 32
    g = Geom(3, (2, 1, 2))  # the unpatchify definition against its index form
    rows = torch.arange(g.L * g.K, dtype=torch.float64).reshape(g.L, g.K)
    lat = g.unpatchify(rows)
    tok, n = (lat // g.K).long(), (lat % g.K).long()
    c, f, h, w = torch.meshgrid(*[torch.arange(s) for s in lat.shape], indexing="ij")
    assert torch.equal(tok, (f // g.pt * g.gh + h // g.ph) * g.gw + w // g.pw)
    assert torch.equal(n, (((f % g.pt) * g.ph + h % g.ph) * g.pw + w % g.pw) * g.C + c)


# ------------------------------------------------------------------------------------------------ the numpy model and its mutants
MUTANTS = ["gather_ph_pw_swapped", "scatter_ph_pw_swapped", "pt_dropped", "gh_gw_swapped", "eps_ignored", "padded_rows_zero",
           "out_rows_ignored", "gemv_padded_rows_read", "last_chunk_skipped", "second_lane_turn_skipped", "shift_scale_swapped",
           "second_grid_turn_skipped", "lds_parity_dropped"]
PAD = 1024  # poison behind every operand of the model: what a read past the end returns (NaN), and is counted


class ModelRun:
    """The kernels' index maps and dispatch as written, in numpy float64 (exact on the integer probes; the float64 formulas elsewhere):
      Linear        1 <= M <= 4: gemv: channel n, lanes k = 4 lane + 256 j + (0..3) while < K, rows m < M with zeros for m >= x_rows;
                    else the tile kernel
      tile kernel   grid ceil(max(out_rows, M) / 64) x ceil(N / 64); operand rows >= x_rows and weight rows >= N staged as zeros;
                    K-step kt staged into LDS buffer kt & 1 and read from it; a lane reads k = 4 fk + kk of the step for both
                    operands (a permutation of the 16 k both share); store: column < N, row < out_rows, act(acc + b) for row < M, else 0
      A_PATCH       token row -> tw = row % gw, th = (row / gw) % gh, tf = row / (gw gh); k -> dw = k % pw, dh = (k / pw) % ph,
                    dt = (k / (pw ph)) % pt, c = k / (pw ph pt); latent[((c F + tf pt + dt) H + th ph + dh) W + tw pw + dw]
      patch kernel  K <= 64: grid ceil(out_rows / 64); rows >= M and k >= K zero-filled; ceil(N / 64) chunks, weight rows >= N zero;
                    store in groups of four columns < N: row < out_rows, acc + b for row < M, else 0
      A_LNMOD       per row: mean, centred squares, rstd = 1 / sqrt(var + eps) over c = 4 lane + 256 j; (x - mean) rstd (1 + sc + e) + (sh + e)
      C_UNPATCH     tile + bias into sC[64][65] (bias 0 for columns >= N); idx -> rr = idx % pw, tok = (idx / pw) % 64, q, pp, c;
                    n = ((pp ph + q) pw + rr) C + c; out[((c F + f pt + pp) H + h ph + q) W + w pw + rr] = sC[tok][n] for row < M
      lincomb       float4 i = block 256 + thread + turn gridDim 256, gridDim = min(ceil(n4 / 256), 2048).
    Reads outside an operand are counted and return NaN; they are reported as a failure, as a bounds checker would."""
    dev = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.oob = mutant, 0

    # ---- plumbing
    def _flat(self, t):
        return np.concatenate([t.double().numpy().ravel(), np.full(PAD, np.nan)])

    def _read(self, flat, idx):
        size = len(flat) - PAD
        bad = (idx < 0) | (idx >= size)
        self.oob += int(bad.sum())
        return flat[np.where(bad, size, idx)]

    def _result(self, win):
        fails = [f"model: {self.oob} elements read outside an operand"] if self.oob else []
        self.oob = 0
        return Result(win, fails)

    @staticmethod
    def _store(win, idx, val):
        flat = win.flat.numpy()
        idx = idx + GUARD
        keep = (idx >= 0) & (idx < len(flat))
        flat[idx[keep]] = np.asarray(val, np.float64).astype(np.float32)[keep].view(np.int32)

    @staticmethod
    def _act(v, kind):
        with np.errstate(all="ignore"):
            return act64(torch.from_numpy(np.asarray(v, np.float64)), kind).numpy()

    # ---- the tile kernel
    def _tile(self, win, a_rows, w, bias, M, x_rows, out_rows, N, K, out_act=None, unpatch=None):
        mut = self.mutant
        wf = self._flat(w)
        b = np.zeros(N) if bias is None else bias.double().numpy()
        rows_all = max(out_rows, M)
        perm = (4 * np.arange(4)[None, :] + np.arange(4)[:, None]).ravel()  # MFMA step kk takes k = 4 fk + kk on k-group fk
        for bm in range(-(-rows_all // BM)):
            rr = bm * BM + np.arange(BM)
            ok = rr < x_rows
            A = np.zeros((BM, K))
            if ok.any():
                A[ok] = a_rows(rr[ok])
            for bn in range(-(-N // BN)):
                cc = bn * BN + np.arange(BN)
                wok = cc < N
                Wt = np.zeros((BN, K))
                Wt[wok] = self._read(wf, cc[wok][:, None] * K + np.arange(K)[None, :])
                sA, sW = np.full((2, BM, BK), np.nan), np.full((2, BN, BK), np.nan)
                acc = np.zeros((BM, BN))
                for kt in range(K // BK):
                    sA[kt & 1], sW[kt & 1] = A[:, kt * BK:(kt + 1) * BK], Wt[:, kt * BK:(kt + 1) * BK]
                    buf = 0 if mut == "lds_parity_dropped" else kt & 1
                    with np.errstate(invalid="ignore", over="ignore"):
                        acc = acc + sA[buf][:, perm] @ sW[buf][:, perm].T
                if unpatch is None:
                    live_r = rr < (BM * (bm + 1) if mut == "out_rows_ignored" else out_rows)
                    val = self._act(acc + np.where(wok, b[np.minimum(cc, N - 1)], 0.0)[None, :], out_act)
                    inside = rr < (x_rows if mut == "padded_rows_zero" else M)
                    val = np.where(inside[:, None], val, 0.0)
                    sel = np.ix_(live_r, wok)
                    self._store(win, (rr[:, None] * N + cc[None, :])[sel].ravel(), val[sel].ravel())
                else:
                    self._scatter(win, unpatch, acc + np.where(wok, b[np.minimum(cc, N - 1)], 0.0)[None, :], bm, M, N)

    def _scatter(self, win, g, tile, bm, M, N):
        mut = self.mutant
        sC = np.full((BM, BN + 1), np.nan)
        sC[:, :BN] = tile
        ph, pw = (g.pw, g.ph) if mut == "scatter_ph_pw_swapped" else (g.ph, g.pw)
        gh, gw = (g.gw, g.gh) if mut == "gh_gw_swapped" else (g.gh, g.gw)
        i = np.arange(g.C * g.pt * g.ph * BM * g.pw)
        rr = i % pw; i = i // pw
        tok = i % BM; i = i // BM
        q = i % ph; i = i // ph
        pp = (i % g.pt) if mut != "pt_dropped" else 0 * i
        c = i // g.pt
        row = bm * BM + tok
        live = row < M
        w_, h_, f_ = row % gw, (row // gw) % gh, row // (gw * gh)
        n = ((pp * ph + q) * pw + rr) * g.C + c
        dst = ((c * g.F + f_ * g.pt + pp) * g.H + h_ * g.ph + q) * g.W + w_ * g.pw + rr
        inside = live & (dst >= 0) & (dst < g.numel) & (n <= BN)
        self.oob += int((live & ~inside).sum())  # a store outside the latent, or an LDS read outside sC
        self._store(win, dst[inside], sC[tok[inside], n[inside]])

    def _gather(self, g, lat, rows, ks):
        """[len(rows), len(ks)] latent elements by the kernels' decomposition (both kernels spell the same one)."""
        mut = self.mutant
        ph, pw = (g.pw, g.ph) if mut == "gather_ph_pw_swapped" else (g.ph, g.pw)
        gh, gw = (g.gw, g.gh) if mut == "gh_gw_swapped" else (g.gh, g.gw)
        tw, th, tf = rows % gw, (rows // gw) % gh, rows // (gw * gh)
        kk = ks.copy()
        dw = kk % pw; kk = kk // pw
        dh = kk % ph; kk = kk // ph
        dt = (kk % g.pt) if mut != "pt_dropped" else 0 * kk
        c = kk // g.pt
        idx = ((c[None, :] * g.F + tf[:, None] * g.pt + dt[None, :]) * g.H + th[:, None] * g.ph + dh[None, :]) * g.W + tw[:, None] * g.pw + dw[None, :]
        return self._read(lat, idx)

    # ---- entries
    def linear(self, x, w, bias, M, in_act=None, out_act=None):
        mut = self.mutant
        (N, K), x_rows = w.shape, x.shape[0]
        win = Window((M, N), "cpu")
        xf = self._flat(x)
        if 1 <= M <= 4:
            wf = self._flat(w)
            turns = 1 if mut == "second_lane_turn_skipped" else -(-K // 256)
            ks = np.array([4 * lane + 256 * j + q for j in range(turns) for lane in range(64) for q in range(4) if 4 * lane + 256 * j < K])
            b = np.zeros(N) if bias is None else bias.double().numpy()
            Wn = self._read(wf, np.arange(N)[:, None] * K + ks[None, :])
            for m in range(M):
                if m < x_rows or mut == "gemv_padded_rows_read":
                    xr = self._read(xf, m * K + ks)
                else:
                    xr = np.zeros(len(ks))
                with np.errstate(invalid="ignore", over="ignore"):
                    self._store(win, m * N + np.arange(N), self._act(Wn @ self._act(xr, in_act) + b, out_act))
            return self._result(win)
        a_rows = lambda rr: self._act(self._read(xf, rr[:, None] * K + np.arange(K)[None, :]), in_act)  # noqa: E731
        self._tile(win, a_rows, w, bias, M, x_rows, M, N, K, out_act)
        return self._result(win)

    def patch(self, g, latent, w, bias, out_rows):
        mut = self.mutant
        N, K, L = w.shape[0], g.K, g.L
        win = Window((out_rows, N), "cpu")
        lat = self._flat(latent)
        if K > 64:
            self._tile(win, lambda rr: self._gather(g, lat, rr, np.arange(K)), w, bias, L, L, out_rows, N, K)
            return self._result(win)
        wf = self._flat(w)
        b = np.zeros(N) if bias is None else bias.double().numpy()
        for bm in range(-(-out_rows // BM)):
            rr = bm * BM + np.arange(BM)
            ok = rr < L
            A = np.zeros((BM, 64))
            if ok.any():
                A[np.ix_(ok, np.arange(64) < K)] = self._gather(g, lat, rr[ok], np.arange(K))
            chunks = N // BN if mut == "last_chunk_skipped" else -(-N // BN)
            for ch in range(chunks):
                cc = ch * BN + np.arange(BN)
                wok = cc < N
                Wt = np.zeros((BN, 64))
                Wt[np.ix_(wok, np.arange(64) < K)] = self._read(wf, cc[wok][:, None] * K + np.arange(K)[None, :])
                with np.errstate(invalid="ignore", over="ignore"):
                    acc = A[:, :K] @ Wt[:, :K].T  # NK4 / 4 blocks of 16 k, each k = 16 j + 4 fk + kk: all of [0, K)
                val = np.where(ok[:, None], acc + np.where(wok, b[np.minimum(cc, N - 1)], 0.0)[None, :], 0.0)
                live_r = rr < (BM * (bm + 1) if mut == "out_rows_ignored" else out_rows)
                sel = np.ix_(live_r, wok)
                self._store(win, (rr[:, None] * N + cc[None, :])[sel].ravel(), val[sel].ravel())
        return self._result(win)

    def head(self, x, mod, e, w, bias, eps, g=None):
        mut = self.mutant
        (rows, K), N = x.shape, w.shape[0]
        win = Window((rows, N) if g is None else (g.C, g.F, g.H, g.W), "cpu")
        xf, mf, ef = self._flat(x), self._flat(mod), self._flat(e)
        eps = 0.0 if mut == "eps_ignored" else float(np.float32(eps))
        cs = np.array([4 * lane + 256 * j + q for j in range(-(-K // 256)) for lane in range(64) for q in range(4) if 4 * lane + 256 * j < K])
        sh, sc = (self._read(mf, np.arange(K)), self._read(mf, K + np.arange(K)))
        if mut == "shift_scale_swapped":
            sh, sc = sc, sh
        ee = self._read(ef, np.arange(K))

        def a_rows(rr):
            with np.errstate(all="ignore"):
                v = self._read(xf, rr[:, None] * K + cs[None, :])
                mean = v.sum(1, keepdims=True) / K
                var = ((v - mean) ** 2).sum(1, keepdims=True) / K
                rstd = 1.0 / np.sqrt(var + eps)
                xv = self._read(xf, rr[:, None] * K + np.arange(K)[None, :])
                return (xv - mean) * rstd * (1.0 + (sc + ee))[None, :] + (sh + ee)[None, :]

        self._tile(win, a_rows, w, bias, rows, rows, rows, N, K, None, g)
        return self._result(win)

    def sinusoid(self, t, kind, dim):
        raw = t.view(np.uint8)
        pos = raw.view([np.float32, np.int64, np.float64, np.int32][kind]).astype(np.float64)
        win = Window((len(t), dim), "cpu")
        ref, _ = sinusoid_reference(pos, dim)
        self._store(win, np.arange(len(t) * dim), ref.ravel())
        return self._result(win)

    def lincomb(self, coef, ins, numel, alias=None):
        n_out, n_in = coef.shape
        alias = alias or {}
        iw = [Window((numel,), "cpu", t) for t in ins]
        ow = [iw[alias[o]] if o in alias else Window((numel,), "cpu") for o in range(n_out)]
        n4 = numel // 4
        grid = min(-(-n4 // 256), 2048)
        turns = 1 if self.mutant == "second_grid_turn_skipped" else -(-n4 // (grid * 256))
        i4 = np.concatenate([np.arange(grid * 256) + t * grid * 256 for t in range(turns)])
        i4 = i4[i4 < n4]
        el = (i4[:, None] * 4 + np.arange(4)[None, :]).ravel()
        vals = [w.window().numpy().astype(np.float64)[el] for w in iw]  # all loads of a float4 come before its stores
        for o in range(n_out):
            self._store(ow[o], el, sum(float(coef[o, i]) * vals[i] for i in range(n_in)))
        return [Result(w, []) for w in ow]

    def torch_act(self, v, kind):
        x = v.float()
        return (torch.nn.functional.silu(x) if kind == "silu" else torch.nn.functional.gelu(x, approximate="tanh")).double()


def model_battery(run):
    """The probes of A - F at the smallest shapes that tell the mutants apart; -> {probe name: failures}."""
    got = {}
    got["A exact gemv (4, 5, 272) x_rows 2"] = probe_linear_exact(run, 4, 5, 272, 2)
    got["A exact gemv (3, 65, 48) x_rows 0"] = probe_linear_exact(run, 3, 65, 48, 0)
    got["A exact tile (65, 130, 48) x_rows 64"] = probe_linear_exact(run, 65, 130, 48, 64)
    got["A exact tile (129, 3, 32) x_rows 1"] = probe_linear_exact(run, 129, 3, 32, 1)
    got["A one-hot gemv (4, 5, 272) k0 254"] = probe_linear_one_hot(run, 4, 5, 272, 254)
    got["A one-hot tile (65, 130, 48)"] = probe_linear_one_hot(run, 65, 130, 48)
    for kind in ("silu", "gelu"):
        yard = act_yardstick(run, kind)
        got[f"A out_act {kind} tile (66, 65, 48) x_rows 60"] = probe_out_act(run, kind, yard, 66, 65, 48, 60)[0]
        got[f"A out_act {kind} gemv (4, 65, 48) x_rows 2"] = probe_out_act(run, kind, yard, 4, 65, 48, 2)[0]
        got[f"A in_act {kind} gemv (4, 5, 272) x_rows 3"] = probe_in_act(run, kind, yard, 4, 5, 272, 3)[0]
    for gi in (0, 2, 4, 5, 7):
        g = Geom(*GEOMS[gi])
        got[f"B index {GEOMS[gi]} N 68 out_rows L + 67"] = probe_patch_index(run, g, 68, g.L + 67, True)
        got[f"B index {GEOMS[gi]} N 60 out_rows L + 1"] = probe_patch_index(run, g, 60, g.L + 1, False)
    got["B dense (4, (4, 2, 1))"] = probe_patch_dense(run, Geom(*GEOMS[5]), 132, 105 + 67)
    got["C constant (65, 48, 65)"] = probe_head_constant(run, 65, 48, 65)
    got["C bound (105, 272, 16)"] = probe_head_bound(run, 105, 272, 16)[0]
    got["C eps"] = probe_head_eps(run)[0]
    for ui in (1, 2):
        got[f"C unpatchify {UNPATCH[ui]}"] = probe_unpatchify(run, *UNPATCH[ui], HEAD_KS[ui])[0]
    got["D isolation linear (129, 130, 48)"] = probe_isolation_linear(run, 129, 130, 48)
    got["D isolation head (105, 16, 12) unpatchify"] = probe_isolation_head(run, 105, 16, 12, Geom(*UNPATCH[2]))
    got["E sinusoid int64"] = probe_sinusoid(run, 1, 6, 5)[0]
    for kind in (0, 2, 3):
        for n in (1, 5):
            got[f"E sinusoid kind {kind} n {n}"] = probe_sinusoid(run, kind, 2, n)[0]
    got["F lincomb (3, 4) aliased"] = probe_lincomb(run, 3, 4, 1028, {1: 2})
    got["F lincomb second turn"] = probe_lincomb(run, 1, 2, BIG_NUMEL)
    return got


def test_model_passes_every_probe():
    run = ModelRun()
    got = model_battery(run)
    assert {k: v for k, v in got.items() if v} == {}
    for M, N, K, k0 in ONE_HOT[4:]:
        assert probe_linear_one_hot(run, M, N, K, k0) == []
    for gi in range(len(GEOMS)):
        g = Geom(*GEOMS[gi])
        for _, N, ok, with_bias, shift in [c for c in PATCH_CASES if c[0] == gi][:2]:
            assert probe_patch_index(run, g, N, out_rows_of(g.L, ok), with_bias, shift) == [], (gi, N)
    for ui in range(len(UNPATCH)):
        assert probe_unpatchify(run, *UNPATCH[ui], HEAD_KS[ui])[0] == [], ui
    assert probe_isolation_patch(run, 6) == [] and probe_isolation_linear(run, 4, 5, 272) == []


# what each mutant must fail at the least (a substring of the probe's name)
MUTANT_FAILS = {
    "gather_ph_pw_swapped": ("B index (2, (1, 2, 4))", "B index (5, (2, 2, 4))", "B dense"),
    "scatter_ph_pw_swapped": ("C unpatchify (2, (2, 2, 4))", "C unpatchify (3, (2, 1, 2))"),
    "pt_dropped": ("B index (2, (2, 1, 4))", "B index (4, (4, 2, 1))", "C unpatchify (2, (2, 2, 4))"),
    "gh_gw_swapped": ("B index (2, (1, 2, 4))", "B index (5, (2, 2, 4))", "C unpatchify"),
    "eps_ignored": ("C eps",),
    "padded_rows_zero": ("A exact tile (65, 130, 48)", "A exact tile (129, 3, 32)", "A out_act silu tile", "A out_act gelu tile"),
    "out_rows_ignored": ("B index (2, (1, 2, 4)) N 60 out_rows L + 1", "B index (5, (2, 2, 4)) N 60"),
    "gemv_padded_rows_read": ("A exact gemv (4, 5, 272) x_rows 2", "A exact gemv (3, 65, 48) x_rows 0", "A out_act silu gemv"),
    "last_chunk_skipped": ("B index (2, (1, 2, 4)) N 68", "B index (2, (1, 2, 4)) N 60", "B dense"),
    "second_lane_turn_skipped": ("A exact gemv (4, 5, 272)", "A one-hot gemv (4, 5, 272) k0 254"),
    "shift_scale_swapped": ("C constant", "C bound", "C unpatchify"),
    "second_grid_turn_skipped": ("F lincomb second turn",),
    "lds_parity_dropped": ("A exact tile (65, 130, 48)", "A one-hot tile", "C bound (105, 272, 16)", "B index (5, (2, 2, 4))"),
}
# probes a mutant must NOT fail: it is seen where its path runs and nowhere else
MUTANT_PASSES = {
    "second_grid_turn_skipped": ("F lincomb (3, 4) aliased", "A exact"), "eps_ignored": ("C bound", "A exact"),
    "second_lane_turn_skipped": ("A exact gemv (3, 65, 48)", "A exact tile"), "lds_parity_dropped": ("A exact gemv", "B index (2, (1, 2, 4))"),
    "pt_dropped": ("B index (2, (1, 2, 4))",), "last_chunk_skipped": ("B index (5, (2, 2, 4))",),
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_named_probes(mutant):
    got = model_battery(ModelRun(mutant))
    failed = {k: v for k, v in got.items() if v}
    print(f"MUTANT {mutant}: fails {sorted(failed)}")
    assert failed, mutant
    for want in MUTANT_FAILS[mutant]:
        assert any(want in k for k in failed), (mutant, want, sorted(failed))
    for keep in MUTANT_PASSES.get(mutant, ()):
        assert not any(keep in k for k in failed), (mutant, keep, sorted(failed))
    if mutant == "out_rows_ignored":  # a store behind the last row: seen by the guard, not by a value
        assert any("guard behind the output" in f for v in failed.values() for f in v)
    if mutant == "gemv_padded_rows_read":  # rows that do not exist: the NaN guard behind x reaches the sum
        assert any("read outside an operand" in f for v in failed.values() for f in v)


def test_bounds_are_far_below_one_and_the_yardstick_is_sane():
    """Every head bound of the table is below 0.25 while a wrong term moves a result by at least 1; torch's fp32 activations on the
    CPU lie within a few units of the float64 definitions (the unit of act_unit), and a GELU in the erf form does not."""
    worst = 0.0
    for rows, K, N in HEAD_CASES:
        worst = max(worst, float(HeadCase(rows, K, N).reference(1e-6)[1].max()))
    print(f"BOUND head, largest over the table: {worst:.3e}")
    assert worst < 0.25
    v = torch.arange(-16, 17, dtype=torch.float64) / 2
    for kind in ("silu", "gelu"):
        assert act_yardstick(ModelRun(), kind) < 16
    erf = 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    assert float(((erf - act64(v, "gelu")).abs() / (act_bound(v, "gelu", 16.0) + 1e-300)).max()) > 100
