"""The three int8 GEMM kernels -- the 128 x 128 kernel gemm_w8a8_kernel (v1), the persistent 256 x 256 kernel gemm_w8a8_big_kernel (v2;
csrc/gemm_w8a8.hip) and the ping-pong kernel gemm_w8a8_pp_kernel (pp; csrc/gemm_w8a8_pp.hip) -- on operands whose answer is known
exactly, and on GELU / random data under derived bounds.  Every call goes through the C ABI (wanq_gemm_w8a8 / wanq_gemm_w4a8) and the
test owns every buffer: the output is a window in a flat allocation with guard zones of GUARD elements in front and behind, the whole
allocation holds a quiet-NaN bit pattern before EVERY launch, and after it both guards must still hold that pattern, bit for bit.

  A  exact probes   every fp32 intermediate of the epilogue is exact, so term order, fma contraction and the kernel do not matter:
                    the output equals the one rounding of an exactly known number.  Assertion: equality, guards intact.
  B  GELU on the exact pre-activations of A, and full-range random operands, under the bounds derived in profiles/PARITY_NOTES.md.
  C  refusals and M = 0 through the ABI: code, a word of the message, the sentinel-filled output untouched.
  E  CPU self-tests (not marked gpu): the dispatch rules restated and the shape table checked against them, exactness proved in
     float64 and float32 with both term orders, a plain fp32 numpy model that passes the checkers and mutants of it that fail.

Dispatch (gemm_entry / launch_gemm in csrc/gemm_w8a8.hip, gemm_pp_eligible in csrc/gemm_w8a8_pp.hip, both on persistent_shape_ok of
csrc/gemm_i8_common.h), `dispatch()` below; `tile_origin()` below restates the walk of that header:
  pp   select 0, W8, M >= 512, K % 128 == 0, K >= 256, no gate + residual unless fp32 output, no GELU with fp32 output
  v2   select 0 / 2, M >= 512, K % 128 == 0              v1   everything else, or select 1
Store loops: 16 (16-bit, no residual), f32res (fp32 + gate + residual, residual ring), f32 and i32 (the 32-bit loop), 16res (16-bit +
gate + residual: v2's generic loop with OutIo<OUT>::load4, pp is not eligible).  pp prefetches its scales by LDS-DMA (`fast`) when
every vector is fp32 and K >= 512.
"""
import collections
import functools
import math

import numpy as np
import pytest
import torch

# The GPU part (sections A - C) is marked test by test, so that section E below runs without a GPU; test_gpu_part_is_marked keeps a
# test added above section E from being left unmarked.
gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "i32": torch.int32}
DTC = {"f16": 0, "bf16": 1, "f32": 2, "i32": 3, "i16": 4}  # WANQ_F16 / BF16 / F32 / I32 / I16 (include/wanq_hip.h)
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}
TINY = {"f16": 2.0 ** -25, "bf16": 2.0 ** -126, "f32": 2.0 ** -126}  # half a subnormal step of fp16; flush-to-zero below the normal range
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
EPI_GELU, EPI_GATE_RES = 1, 2
GUARD = 4096  # elements; a multiple of 16, so the window stays 16-byte aligned in every type
# quiet NaNs with a payload (int32 output: a value above every accumulator, |acc| <= 512 * 128 * 128); compared as integers
SENT_BITS = {"f16": 0x7E5A, "bf16": 0x7FC5, "f32": 0x7FC5A5A5, "i32": 0x7FC5A5A5}
SELECT = {"v1": 1, "v2": 2, "pp": 0}
GROUP_M = 4

Form = collections.namedtuple("Form", "out vec zp bias epi gelu w4")  # vec: f32 | f16 (fp16 vectors, int16 zp); epi: none | res | inplace


# ================================================================================================ dispatch rules, restated
def dispatch(M, N, K, form, select):
    """(kernel, store loop) that gemm_entry launches for this problem under wanq_gemm_select_kernel(select)."""
    res, out16 = form.epi != "none", form.out in ("f16", "bf16")
    small = M * K < 2 ** 32 and N * K < 2 ** 32
    pp_ok = (not form.w4 and M >= 512 and K % 128 == 0 and K >= 256 and small and not (res and form.out != "f32")
             and not (form.gelu and form.out == "f32"))
    if select == 0 and pp_ok:
        kernel = "pp"
    elif M >= 512 and K % 128 == 0 and select != 1 and small:
        kernel = "v2"
    else:
        kernel = "v1"
    loop = "i32" if form.out == "i32" else ("16res" if res else "16") if out16 else ("f32res" if res else "f32")
    return kernel, (loop if kernel != "v1" else "epilogue")  # (v1 has one epilogue path, templated on the output type)


def fast_scales(K, form):
    """pp: the tile's scales are prefetched by LDS-DMA into the turn buffer (all vectors fp32 and at least four K-tiles)."""
    return form.out != "i32" and form.vec == "f32" and K >= 4 * 128


def tile_origin(t, mt, nt, group_m=GROUP_M):
    """tile id -> (m-tile, n-tile) of the persistent kernels: the XCD remap, then groups of group_m m-tiles, a short last group."""
    ntiles = mt * nt
    xq, xr, xcd = ntiles >> 3, ntiles & 7, t & 7
    wg = (xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq) + (t >> 3)
    per_group = group_m * nt
    group = wg // per_group
    first_m = group * group_m
    gsz = min(mt - first_m, group_m)
    in_g = wg - group * per_group
    return first_m + in_g % gsz, in_g // gsz


def persistent_walk(M, N):
    """(grid, [tiles of workgroup b as (mi, ni, full)]) of the persistent kernels for an M x N output."""
    mt, nt = -(-M // 256), -(-N // 256)
    ntiles = mt * nt
    grid = (ntiles + 7) & ~7 if ntiles < 256 else 256
    walks = []
    for b in range(grid):
        tiles = []
        for t in range(b, ntiles, grid):
            mi, ni = tile_origin(t, mt, nt)
            tiles.append((mi, ni, (mi + 1) * 256 <= M and (ni + 1) * 256 <= N))
        walks.append(tiles)
    return grid, walks


# ================================================================================================ A. the exact probe
def hash32(r, c, salt):
    """A fixed integer hash of (r, c): int64 tensor of values below 2^32 (the products wrap mod 2^64; the low 32 bits are kept)."""
    m = 0xFFFFFFFF
    h = (r * 0x9E3779B1 + c * 0x85EBCA77 + (salt * 0x27D4EB2F + 1)) & m
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & m
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & m
    return h ^ (h >> 15)


class Probe:
    """a[m, k] = am[m] at k = km[m] only (am in +-{1, 2, 3}; K-tile of km = m mod #K-tiles, the place inside it by a hash: every K-tile
    of every output tile with as many rows as K-tiles is hit), w in [-8, 7] (also the 4-bit codes w + 8 with zp - 8), so
    acc[m, n] = am[m] w[n, km[m]] is a gather.  sa = 2^-{0..3}, sw = 2^{-2..1}, zp in [-2, 2], asum = sa am (the true row sum),
    bias = j / 32 with |bias| <= 4, gate = +-{0.5, 1, 2}, residual = j / 32 with |j| <= 127 (exact in bf16).  Every choice is a hash
    of m or n.  All tensors float64 / int64 on `dev`."""

    def __init__(self, M, N, K, dev="cpu"):
        self.M, self.N, self.K, self.dev = M, N, K, dev
        m, n = torch.arange(M, dtype=torch.int64, device=dev), torch.arange(N, dtype=torch.int64, device=dev)
        z = torch.zeros((), dtype=torch.int64, device=dev)
        nkt = -(-K // 128)
        kt = m % nkt
        width = torch.minimum(torch.full_like(kt, 128), K - kt * 128)  # the last K-tile may be a tail of 16 .. 112
        self.km = kt * 128 + hash32(m, z, 1) % width
        self.am = (hash32(m, z, 2) % 3 + 1) * (1 - 2 * (hash32(m, z, 3) & 1))
        self.w = hash32(n[:, None], torch.arange(K, dtype=torch.int64, device=dev)[None, :], 4) % 16 - 8
        # (the two exponents step by 1 .. 3 mod 4 from one index to the next: neighbouring rows and neighbouring columns always differ)
        self.sa = 2.0 ** -(torch.cumsum(hash32(m, z, 5) % 3 + 1, 0) % 4).double()
        self.sw = 2.0 ** ((torch.cumsum(hash32(n, z, 6) % 3 + 1, 0) % 4).double() - 2)
        self.zp = (hash32(n, z, 7) % 5 - 2).double()
        self.asum = self.sa * self.am
        self.bias = (hash32(n, z, 8) % 257 - 128).double() / 32
        self.gate = (1 - 2 * (hash32(n, z, 9) & 1)).double() * 2.0 ** ((hash32(n, z, 10) % 3).double() - 1)
        self.res = (hash32(m[:, None], n[None, :], 11) % 255 - 127).double() / 32
        self.acc = self.am[:, None] * self.w[:, self.km].T            # W8: codes w
        self.acc4 = self.am[:, None] * (self.w[:, self.km].T + 8)     # W4: unsigned codes w + 8

    def a_matrix(self):
        a = torch.zeros(self.M, self.K, dtype=torch.int8, device=self.dev)
        a[torch.arange(self.M, device=self.dev), self.km] = self.am.to(torch.int8)
        return a

    def terms(self, form):
        """(acc, zp used, bias used) of a form, float64."""
        acc = (self.acc4 if form.w4 else self.acc).double()
        zp = (self.zp - 8 if form.w4 else self.zp) if form.zp else None
        return acc, zp, (self.bias if form.bias else None)

    def pre(self, form):
        """The exact pre-activation acc sa sw + asum zp sw + bias, float64 [M, N]."""
        acc, zp, bias = self.terms(form)
        y = acc * self.sa[:, None] * self.sw[None, :]
        if zp is not None:
            y = y + self.asum[:, None] * (zp * self.sw)[None, :]
        if bias is not None:
            y = y + bias[None, :]
        return y

    def expect(self, form):
        """The expected output: int accumulators, or the one rounding of the exact value into the output type (as float64)."""
        if form.out == "i32":
            return self.acc4 if form.w4 else self.acc
        y = self.pre(form)
        if form.epi != "none":
            y = self.res + y * self.gate[None, :]
        return y.to(TDT[form.out]).double()


def pack_w4(u):
    """The packed layout of include/wanq_hip.h restated: per 32 codes 16 bytes (P0a, P1a, P0b, P1b); for a 16-code half u:
    P0 byte i = u[i] | u[4 + i] << 4, P1 byte i = u[8 + i] | u[12 + i] << 4.  u: int64 [N, K] of 0 .. 15."""
    N, K = u.shape
    u = u.reshape(N, K // 16, 16)
    p0 = u[:, :, 0:4] | (u[:, :, 4:8] << 4)
    p1 = u[:, :, 8:12] | (u[:, :, 12:16] << 4)
    return torch.cat([p0, p1], dim=2).reshape(N, K // 2).to(torch.uint8)


def exact_forms(w4):
    """The product of Section A: output type x vector types x (zp, bias) x epilogue; int32 once."""
    forms = [Form("i32", "f32", False, False, "none", False, w4)]
    for out in ("f16", "bf16", "f32"):
        for vec in ("f32", "f16"):
            for zp, bias in ((False, False), (False, True), (True, True), (True, False)):
                for epi in ("none", "res", "inplace"):
                    forms.append(Form(out, vec, zp, bias, epi, False, w4))
    return forms


# (kernel, M, N, K, w4): the full product of exact_forms runs on each (forms that dispatch elsewhere are left to the kernel they go to)
SMALL_CASES = [
    ("v1", 1, 8, 16, False), ("v1", 130, 136, 144, False), ("v1", 777, 264, 256, False),
    ("v1", 1, 8, 32, True), ("v1", 130, 136, 160, True), ("v1", 777, 264, 256, True),
    ("v2", 520, 264, 128, False), ("v2", 777, 264, 256, False), ("v2", 777, 264, 384, False), ("v2", 777, 264, 512, False),
    ("v2", 520, 264, 128, True), ("v2", 777, 264, 256, True), ("v2", 777, 264, 384, True), ("v2", 777, 264, 512, True),
    ("pp", 777, 264, 256, False), ("pp", 777, 264, 384, False), ("pp", 777, 264, 512, False),
]
# 38 x 7 = 266 tiles on 256 workgroups: one case per store loop, five launches each.  K = 256 with the fp16 / int16 vectors (pp: the
# scales are loaded), K = 512 with fp32 vectors (pp: the scales are prefetched).  (At 9221 rows = 37 x 7 tiles every workgroup with
# two tiles runs two full ones: test_shape_table_reaches_every_form walks the tiles.)
BIG_M, BIG_N = 9477, 1544
RAND_M = 9221
BIG_LOOPS = {
    "16": Form("bf16", "f32", True, True, "none", False, False),
    "f32res": Form("f32", "f32", True, True, "inplace", False, False),
    "f32": Form("f32", "f32", True, True, "none", False, False),
    "i32": Form("i32", "f32", False, False, "none", False, False),
    "16res": Form("f16", "f32", True, True, "inplace", False, False),
}
BIG_CASES = [(k, K, loop) for k in ("v2", "pp") for K in (256, 512) for loop in BIG_LOOPS if not (k == "pp" and loop == "16res")]
BIG_CASES += [("v2", 512, "16", True), ("v2", 512, "f32res", True)]  # packed 4-bit weights: v2's other main loop under both residual paths


def big_form(K, loop, w4=False):
    return BIG_LOOPS[loop]._replace(vec="f32" if K >= 512 or loop == "i32" else "f16", w4=w4)


def forms_of_case(kernel, M, N, K, w4):
    return [f for f in exact_forms(w4) if dispatch(M, N, K, f, SELECT[kernel])[0] == kernel]


# ------------------------------------------------------------------------------------------------ buffers and checkers
class Window:
    """The output as a window of M * N elements inside a flat allocation with GUARD elements in front and behind."""

    def __init__(self, M, N, out, dev):
        self.M, self.N, self.out = M, N, out
        self.idt = torch.int32 if out in ("f32", "i32") else torch.int16
        self.flat = torch.empty(2 * GUARD + M * N, dtype=self.idt, device=dev)
        self.fill()

    def fill(self):
        self.flat.fill_(SENT_BITS[self.out])

    def window(self):
        return self.flat[GUARD:GUARD + self.M * self.N].view(self.M, self.N).view(TDT[self.out])

    def ptr(self):
        assert (self.flat.data_ptr() + GUARD * self.flat.element_size()) % 16 == 0
        return self.flat.data_ptr() + GUARD * self.flat.element_size()


def guard_failures(win):
    s, n = SENT_BITS[win.out], GUARD + win.M * win.N
    fails = []
    if bool((win.flat[:GUARD] != s).any()):
        fails.append(f"the guard in front of the output was written at element {int((win.flat[:GUARD] != s).nonzero()[0]) - GUARD}")
    if bool((win.flat[n:] != s).any()):
        fails.append(f"the guard behind the output was written at element {win.M * win.N + int((win.flat[n:] != s).nonzero()[0])}")
    return fails


def check_exact(win, expect, tile=256):
    """Equality of every element of the window with `expect` (an element that still holds the sentinel is a NaN: unequal), guards intact."""
    fails = guard_failures(win)
    got = win.window()
    bad = ~(got.double() == expect.double()) if win.out != "i32" else got.long() != expect
    if bool(bad.any()):
        idx = bad.nonzero()
        r, c = int(idx[0, 0]), int(idx[0, 1])
        unwritten = int((win.flat[GUARD:GUARD + win.M * win.N].view(win.M, win.N)[bad] == SENT_BITS[win.out]).sum())
        tiles = sorted({(int(i) // tile, int(j) // tile) for i, j in idx[:: max(1, len(idx) // 64)].tolist()})[:6]
        fails.append(f"{len(idx)} elements differ ({unwritten} of them never written), tiles {tiles}; first at row {r} col {c}: "
                     f"got {got[r, c].item()} expected {expect[r, c].item()}")
    return fails


def check_bound(win, ref, bound):
    """|out - ref| <= bound elementwise (NaN fails), guards intact.  Returns (failures, largest err / bound)."""
    fails = guard_failures(win)
    err = (win.window().double() - ref).abs()
    ratio = err / bound
    bad = ~(err <= bound)
    if bool(bad.any()):
        r, c = [int(v) for v in bad.nonzero()[0]]
        fails.append(f"{int(bad.sum())} elements beyond the bound; first at row {r} col {c}: got {win.window()[r, c].item()} ref {ref[r, c].item()} "
                     f"bound {bound[r, c].item():.3e}")
    return fails, float(torch.nan_to_num(ratio, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------ the ABI call
def _vec(x, vec, integer=False):
    if x is None:
        return None
    if integer and vec == "f16":
        return x.to(torch.int16)
    return x.to(torch.float16 if vec == "f16" else torch.float32)


class Operands:
    """Device buffers of one problem in both vector types, from a (int8), w (codes) and float64 sa, asum, sw, zp, bias, gate, res."""

    def __init__(self, M, N, K, a, w, sa, asum, sw, zp, bias, gate, res, dev):
        self.M, self.N, self.K = M, N, K
        self.a, self.w8 = a.contiguous().to(dev), w.to(torch.int8).contiguous().to(dev)
        self.w4 = pack_w4(w.long() + 8).to(dev) if K % 32 == 0 and int(w.min()) >= -8 and int(w.max()) <= 7 else None
        # (rounded into the storage type where they were made, then moved: the reference rounds the same tensors the same way)
        self.vecs = {v: {k: x.to(dev) for k, x in dict(sa=_vec(sa, v), asum=_vec(asum, v), sw=_vec(sw, v), bias=_vec(bias, v), zp=_vec(zp, v, True),
                                                       zp4=_vec(zp - 8, v, True)).items()} for v in ("f32", "f16")}
        self.gate, self.res = gate.float().contiguous().to(dev), res.to(dev)

    def launch(self, form, win, residual=None):
        """One call of wanq_gemm_w8a8 / wanq_gemm_w4a8 into `win`; returns the return code.  Nothing is synchronised here."""
        from viditq_extension import _C

        v, fl = self.vecs[form.vec], form.out != "i32"
        zp = (v["zp4"] if form.w4 else v["zp"]) if form.zp else None
        epi = (EPI_GELU if form.gelu else 0) | (EPI_GATE_RES if form.epi != "none" else 0)
        resp = None if form.epi == "none" else win.ptr() if form.epi == "inplace" else _C.ptr(residual)
        fn = _C.lib.wanq_gemm_w4a8 if form.w4 else _C.lib.wanq_gemm_w8a8
        return fn(_C.ptr(self.a), _C.ptr(self.w4 if form.w4 else self.w8), win.ptr(), DTC[form.out], _C.ptr(v["sa"]) if fl else None,
                  _C.ptr(v["asum"]) if fl and form.zp else None, DTC[form.vec], _C.ptr(v["sw"]) if fl else None,
                  _C.ptr(v["bias"]) if fl and form.bias else None, DTC[form.vec], _C.ptr(zp) if fl else None,
                  DTC["i16" if form.vec == "f16" else "f32"], _C.ptr(self.gate) if epi & EPI_GATE_RES else None, resp, epi,
                  self.M, self.N, self.K, _C.stream())

    def run(self, form, win):
        """Fresh sentinel, the residual placed (in the window when in place), one launch, synchronised."""
        win.fill()
        residual = None
        if form.epi == "inplace":
            win.window().copy_(self.res.to(TDT[form.out]))
        elif form.epi == "res":
            residual = self.res.to(TDT[form.out]).contiguous()
        rc = self.launch(form, win, residual)
        torch.cuda.synchronize()
        assert rc == WANQ_OK, rc
        return win


@functools.lru_cache(maxsize=3)
def probe_on_gpu(M, N, K):
    p = Probe(M, N, K, DEV)
    return p, Operands(M, N, K, p.a_matrix(), p.w, p.sa, p.asum, p.sw, p.zp, p.bias, p.gate, p.res, DEV)


@pytest.fixture
def kernel_select():
    from viditq_extension import _C

    before = []

    def select(which):
        before.append(_C.lib.wanq_gemm_select_kernel(which))
        return before[-1]

    yield select
    if before and before[0] >= 0:  # back to what was set before the test's first call
        _C.lib.wanq_gemm_select_kernel(before[0])


@gpu
@pytest.mark.parametrize("kernel,M,N,K,w4", SMALL_CASES)
def test_exact_probe_every_form(kernel_select, kernel, M, N, K, w4):
    """Output type x vector types x (zp, bias) x (no flag, gate + residual, the same in place): equality with the one rounding of the
    exact value, both guards intact, a fresh sentinel in front of every launch."""
    kernel_select(SELECT[kernel])
    p, ops = probe_on_gpu(M, N, K)
    forms = forms_of_case(kernel, M, N, K, w4)
    assert len(forms) == (41 if kernel == "pp" else 73)  # pp takes no 16-bit output with gate + residual
    wins, fails = {}, []
    for form in forms:
        win = wins.setdefault(form.out, Window(M, N, form.out, DEV))
        fails += [f"{form}: {f}" for f in check_exact(ops.run(form, win), p.expect(form), 128 if kernel == "v1" else 256)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("case", BIG_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_exact_probe_several_tiles_per_workgroup(kernel_select, case):
    """266 tiles on 256 workgroups (a full tile then a ragged one and the reverse, ntiles % 8 = 2, mt % group_m = 2, a last n-tile of 8
    columns), one case per store loop, five launches each from a fresh sentinel: the race screen of the counted waits, with exact
    expectations."""
    kernel, K, loop = case[:3]
    form = big_form(K, loop, len(case) > 3)
    assert dispatch(BIG_M, BIG_N, K, form, SELECT[kernel]) == (kernel, loop)
    kernel_select(SELECT[kernel])
    p, ops = probe_on_gpu(BIG_M, BIG_N, K)
    expect, win, fails = p.expect(form), Window(BIG_M, BIG_N, form.out, DEV), []
    for launch in range(5):
        fails += [f"launch {launch}: {f}" for f in check_exact(ops.run(form, win), expect)]
    assert not fails, f"{form}\n" + "\n".join(fails[:20])


# ================================================================================================ B. GELU and random data
C1 = -2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e)  # -2 u log2(e) = x (C1 + C3 x^2)
C3 = C1 * 0.044715
C1F, C3F = float(np.float32(-2.3022082)), float(np.float32(-0.10294324))  # the constants of gelu_tanh_fast_f32 (csrc/wanq_common.h)


def gelu_ref(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), float64, written as x / (1 + e^{-2u}): the same function without the
    cancellation of 1 + tanh(u) in the negative tail."""
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x * torch.special.expit(2.0 * u)


def gelu_bound(x):
    """Absolute error bound of gelu_tanh_fast_f32(x) = x rcp(1 + exp2(t)), t = fl(x fl(fma(fl(x^2), c3, c1))), against gelu_ref(x)
    (derivation: profiles/PARITY_NOTES.md).  x float64, exactly representable in fp32."""
    T = x * (C1 + C3 * x * x)
    dT = 3 * U * T.abs() * (1 + 2.0 ** -10) + x.abs() * abs(C1F - C1) + x.abs() ** 3 * abs(C3F - C3)  # roundings of t, the constants
    eps_e = torch.expm1(math.log(2.0) * dT) + 2 * U                       # exp2 carries dT, v_exp_f32 one ulp
    s = torch.special.expit(T * math.log(2.0))                            # E / (1 + E): the share of E in the denominator
    rel = (s * eps_e + U + 2 * U + U) * (1 + 2.0 ** -10)                  # fl(1 + E), v_rcp_f32 one ulp, the final multiply
    return gelu_ref(x).abs() * rel + 2.0 ** -125 * torch.clamp(x.abs(), min=1.0)  # + flush-to-zero of 1 / (1 + E) and of the product


def output_bound(y, err, out):
    """err on the fp32 value y, then one rounding into the output type (fp32: the register is stored)."""
    return (err * (1 + U_OUT[out]) + U_OUT[out] * y.abs()) * (1 + 2.0 ** -10) + TINY[out]


def gelu_case_bound(p, form):
    """(reference, bound) of a GELU form on the probe operands: the pre-activation is exact in fp32, so the error is GELU's alone."""
    x = p.pre(form)
    g, eg = gelu_ref(x), gelu_bound(x)
    if form.epi == "none":
        return g, output_bound(g, eg, form.out)
    y = p.res + g * p.gate[None, :]
    return y, output_bound(y, p.gate.abs()[None, :] * (eg + U * g.abs()) + U * y.abs(), form.out)


def gelu_forms(kernel, M, N, K):
    forms = [Form(out, vec, True, True, epi, True, w4) for out in ("f16", "bf16", "f32") for vec in ("f32", "f16")
             for epi in ("none", "res", "inplace") for w4 in ((False, True) if kernel != "pp" and K % 32 == 0 else (False,))]
    return [f for f in forms if dispatch(M, N, K, f, SELECT[kernel])[0] == kernel]


GELU_CASES = [("v1", 130, 136, 144), ("v1", 130, 136, 160), ("v2", 520, 264, 128), ("v2", 777, 264, 512), ("pp", 777, 264, 256), ("pp", 777, 264, 512)]


@gpu
@pytest.mark.parametrize("kernel,M,N,K", GELU_CASES)
def test_gelu_epilogue_under_the_derived_bound(kernel_select, kernel, M, N, K):
    """GELU on pre-activations known exactly (multiples of 2^-5 over [-64, 64]: both tails saturate), alone and with gate + residual
    (out of place and in place), fp32 output and packed weights included; against float64 under the bound of gelu_tanh_fast_f32."""
    kernel_select(SELECT[kernel])
    p, ops = probe_on_gpu(M, N, K)
    forms = gelu_forms(kernel, M, N, K)
    if kernel != "pp":  # the three forms that nothing else runs: GELU + gate + residual, fp32 output with GELU, W4 with GELU on v2
        assert any(f.epi != "none" for f in forms) and any(f.out == "f32" for f in forms) and (K % 32 != 0 or any(f.w4 for f in forms))
    wins, fails, worst = {}, [], {}
    for form in forms:
        win = wins.setdefault(form.out, Window(M, N, form.out, DEV))
        ref, bound = gelu_case_bound(p, form)
        f, ratio = check_bound(ops.run(form, win), ref, bound)
        fails += [f"{form}: {x}" for x in f]
        key = (form.out, form.epi != "none")
        worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"RATIO gelu {kernel} {M}x{N}x{K} " + " ".join(f"{o}{'+res' if r else ''}={v:.3f}" for (o, r), v in sorted(worst.items())))
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


class RandomCase:
    """Full-range operands: a, w uniform over int8, positive scales, zp in [-20, 20], Gaussian bias, gate and residual.  The accumulators
    are a float64 BLAS product on the CPU (exact: |acc| <= 512 * 2^14 < 2^53).  The vectors are rounded into their storage type
    first; the reference takes the rounded values."""

    def __init__(self, M, N, K, dev):
        g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
        self.M, self.N, self.K = M, N, K
        a = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
        w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
        self.acc = (a.double() @ w.double().T).to(dev)
        sa = torch.rand(M, generator=g, dtype=torch.float64) * 0.015 + 0.005
        sw = torch.rand(N, generator=g, dtype=torch.float64) * 0.002 + 0.001
        zp = torch.randint(-20, 21, (N,), generator=g).double()
        bias, gate = torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64).float().double()
        asum = a.double().sum(1) * sa
        self.res = torch.randn(M, N, generator=g, dtype=torch.float32).to(dev)
        self.gate = gate.to(dev)
        self.host = dict(sa=sa, asum=asum, sw=sw, zp=zp, bias=bias)
        self.ops = Operands(M, N, K, a, w, sa, asum, sw, zp, bias, gate, self.res, dev)

    def reference(self, form):
        """(float64 reference, bound).  S = |acc sa sw| + |asum zp sw| + |bias|.  v1 rounds acc sa, (acc sa) sw, asum zp, (asum zp) sw and
        two additions: <= 4 u S; v2 / pp round acc sa, zp sw and two fmas: <= 3 u S.  Bound 4 u S (1 + 2^-10), carried through the gate
        (one product, one addition: |gate| (4 u S + u |y|) + u |out|), then half a unit of the output type."""
        rt = torch.float16 if form.vec == "f16" else torch.float32
        v = {k: x.to(rt).double().to(self.acc.device) for k, x in self.host.items()}
        t1 = self.acc * v["sa"][:, None] * v["sw"][None, :]
        t2 = v["asum"][:, None] * (v["zp"] * v["sw"])[None, :] if form.zp else torch.zeros_like(t1)
        t3 = v["bias"][None, :] if form.bias else torch.zeros_like(t1[:1])
        y = t1 + t2 + t3
        err = 4 * U * (t1.abs() + t2.abs() + t3.abs()) * (1 + 2.0 ** -10)
        if form.epi != "none":
            out = self.res.to(TDT[form.out]).double() + y * self.gate[None, :]
            err = self.gate.abs()[None, :] * (err + U * y.abs()) + U * out.abs()
            y = out
        return y, output_bound(y, err, form.out)


@functools.lru_cache(maxsize=1)
def random_case(M, N, K):
    return RandomCase(M, N, K, DEV)


RANDOM_CASES = [("v1", 130, 136, 144), ("v1", 777, 264, 512), ("v2", 777, 264, 512), ("pp", 777, 264, 512),
                ("v1", RAND_M, BIG_N, 256), ("v2", RAND_M, BIG_N, 256), ("pp", RAND_M, BIG_N, 256)]


def random_forms(kernel, M, N, K):
    forms = [Form(out, vec, zp, bias, epi, False, False) for out in ("f16", "bf16", "f32") for vec in ("f32", "f16")
             for zp, bias, epi in ((True, True, "none"), (True, True, "inplace"), (False, False, "none"))]
    return [f for f in forms if dispatch(M, N, K, f, SELECT[kernel])[0] == kernel]


@gpu
@pytest.mark.parametrize("kernel,M,N,K", RANDOM_CASES)
def test_random_operands_under_the_derived_bound(kernel_select, kernel, M, N, K):
    """int32 output equals the float64 BLAS product; every floating output type within the bound derived from the two summation
    orders, with no absolute floor beyond flush-to-zero (fp16: half a subnormal step)."""
    kernel_select(SELECT[kernel])
    case = random_case(M, N, K)
    win = Window(M, N, "i32", DEV)
    fails = [f"int32: {f}" for f in check_exact(case.ops.run(Form("i32", "f32", False, False, "none", False, False), win), case.acc.long())]
    del win
    worst = {}
    for out in ("f16", "bf16", "f32"):
        win = Window(M, N, out, DEV)
        for form in (f for f in random_forms(kernel, M, N, K) if f.out == out):
            ref, bound = case.reference(form)
            f, ratio = check_bound(case.ops.run(form, win), ref, bound)
            fails += [f"{form}: {x}" for x in f]
            worst[out] = max(worst.get(out, 0.0), ratio)
        del win
    print(f"RATIO random {kernel} {M}x{N}x{K} " + " ".join(f"{o}={v:.3f}" for o, v in sorted(worst.items())))
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ C. refusals and M = 0
def _abi_args(M=5, N=16, K=32, out="f32", tok="f32", ch="f32", zpd="f32", epi=0, w4=False, drop=()):
    """Argument list of one call on small valid buffers (a refused call reads none of them) and the sentinel-filled output."""
    from viditq_extension import _C

    n, k = max(min(N, 64), 8) + 8, max(min(K, 64), 16) + 16
    a = torch.zeros(max(min(M, 8), 1), k, dtype=torch.int8, device=DEV)
    w = torch.zeros(n, k, dtype=torch.int8, device=DEV)
    vec = torch.ones(4, max(n, 8), dtype=torch.float32, device=DEV)
    res = torch.zeros(8, n, dtype=torch.float32, device=DEV)
    win = Window(8, n, out if out in TDT else "f32", DEV)
    ptrs = dict(a=_C.ptr(a), w=_C.ptr(w), out=win.ptr(), sa=_C.ptr(vec[0]), asum=_C.ptr(vec[1]), sw=_C.ptr(vec[2]), bias=_C.ptr(vec[3]),
                zp=_C.ptr(vec[1]), gate=_C.ptr(vec[0]), res=_C.ptr(res))
    for name in drop:
        ptrs[name] = None
    dtc = lambda d: DTC[d] if isinstance(d, str) else d
    args = [ptrs["a"], ptrs["w"], ptrs["out"], dtc(out), ptrs["sa"], ptrs["asum"], dtc(tok), ptrs["sw"], ptrs["bias"], dtc(ch), ptrs["zp"], dtc(zpd),
            ptrs["gate"], ptrs["res"], epi, M, N, K, _C.stream()]
    return ("wanq_gemm_w4a8" if w4 else "wanq_gemm_w8a8"), args, win, (a, w, vec, res)


def _untouched(win):
    torch.cuda.synchronize()
    return bool((win.flat == SENT_BITS[win.out]).all())


REFUSALS = [
    (dict(drop=("a",)), WANQ_E_ARG, "must be non-NULL"), (dict(drop=("w",)), WANQ_E_ARG, "must be non-NULL"),
    (dict(out=4), WANQ_E_ARG, "bad out dtype"), (dict(out=7), WANQ_E_ARG, "bad out dtype"), (dict(out=-1), WANQ_E_ARG, "bad out dtype"),
    (dict(M=-1), WANQ_E_SHAPE, "out of range"), (dict(M=2 ** 30), WANQ_E_SHAPE, "out of range"),
    (dict(N=12), WANQ_E_SHAPE, "multiple of 8"), (dict(N=0), WANQ_E_SHAPE, "multiple of 8"),
    (dict(K=24), WANQ_E_SHAPE, "multiple of 16"), (dict(K=0), WANQ_E_SHAPE, "multiple of 16"),
    (dict(K=48, w4=True), WANQ_E_SHAPE, "multiple of 32"), (dict(K=16, w4=True), WANQ_E_SHAPE, "multiple of 32"),
    (dict(drop=("sa",)), WANQ_E_ARG, "sa and sw are required"), (dict(drop=("sw",)), WANQ_E_ARG, "sa and sw are required"),
    (dict(tok="bf16"), WANQ_E_ARG, "tok/ch dtype"), (dict(ch="i16"), WANQ_E_ARG, "tok/ch dtype"),
    (dict(drop=("asum",)), WANQ_E_ARG, "zp needs asum"), (dict(zpd="f16"), WANQ_E_ARG, "zp needs asum"), (dict(zpd="bf16"), WANQ_E_ARG, "zp needs asum"),
    (dict(epi=EPI_GATE_RES, drop=("gate",)), WANQ_E_ARG, "needs gate and residual"),
    (dict(epi=EPI_GATE_RES, drop=("res",)), WANQ_E_ARG, "needs gate and residual"),
    (dict(out="i32", epi=EPI_GELU), WANQ_E_ARG, "takes no epilogue flags"), (dict(out="i32", epi=EPI_GATE_RES), WANQ_E_ARG, "takes no epilogue flags"),
    (dict(epi=4), WANQ_E_ARG, "unknown epilogue flag"), (dict(epi=8 | EPI_GELU), WANQ_E_ARG, "unknown epilogue flag"),
    (dict(M=2 ** 29, N=2 ** 24), WANQ_E_SHAPE, "too many tiles"),
]


# every requirement on both entry points (the K rules are each entry point's own)
REFUSAL_CASES = [(w4, kw, code, message) for w4 in (False, True) for kw, code, message in REFUSALS
                 if kw.get("w4", w4) == w4 and not (w4 and kw.get("K") in (24, 0))]


def _refusal_id(case):
    w4, kw, code, message = case
    what = "-".join(f"{k}={'+'.join(v) if isinstance(v, tuple) else v}" for k, v in kw.items() if k != "w4")
    return f"{'w4a8' if w4 else 'w8a8'}-{what}-{message.replace(' ', '_').replace('/', '_')}"


@gpu
@pytest.mark.parametrize("case", REFUSAL_CASES, ids=_refusal_id)
def test_refusals_through_the_abi(case):
    """One requirement of gemm_entry: its code, a word of its message, nothing written."""
    from viditq_extension import _C

    w4, kw, code, message = case
    entry, args, win, keep = _abi_args(**dict(kw, w4=w4))
    assert getattr(_C.lib, entry)(*args) == code, (entry, kw, _C.lib.wanq_last_error().decode())
    assert message in _C.lib.wanq_last_error().decode(), (kw, _C.lib.wanq_last_error().decode())
    assert _untouched(win), kw


@gpu
@pytest.mark.parametrize("w4", [False, True])
@pytest.mark.parametrize("out", ["i32", "f16", "bf16", "f32"])
def test_no_rows_is_ok_and_writes_nothing(out, w4):
    from viditq_extension import _C

    entry, args, win, keep = _abi_args(M=0, out=out, w4=w4, epi=0 if out == "i32" else EPI_GATE_RES)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK
    assert _untouched(win)


@gpu
def test_select_kernel_refuses_an_unknown_value(kernel_select):
    from viditq_extension import _C

    kernel_select(2)
    for bad in (3, -1, 17):
        assert _C.lib.wanq_gemm_select_kernel(bad) == -1
    assert _C.lib.wanq_gemm_select_kernel(1) == 2  # the setting survived the refused calls
    assert _C.lib.wanq_gemm_select_kernel(0) == 1


# ================================================================================================ E. CPU self-tests of the probes
def test_shape_table_reaches_every_form():
    """Every (kernel, store loop, full / ragged tile, one / several tiles per workgroup) combination and, for pp, both scale paths;
    v2 at one K-tile; idle workgroups; a workgroup that runs a full tile then a ragged one and one that does the reverse;
    ntiles % 8 != 0 and mt % group_m != 0; the W4 forms of v1 and v2; v1 with a K tail and a short last group."""
    reached = set()
    for kernel, M, N, K, w4 in SMALL_CASES:
        forms = forms_of_case(kernel, M, N, K, w4)
        for f in forms:
            assert dispatch(M, N, K, f, SELECT[kernel])[0] == kernel
        tile = 128 if kernel == "v1" else 256
        kinds = {((mi + 1) * tile <= M and (ni + 1) * tile <= N) for mi in range(-(-M // tile)) for ni in range(-(-N // tile))}
        for f in forms:
            loop = dispatch(M, N, K, f, SELECT[kernel])[1]
            scales = ("fast" if fast_scales(K, f) else "slow") if kernel == "pp" and f.out != "i32" else "-"
            for full in kinds:
                reached.add((kernel, loop, "full" if full else "ragged", "one", scales, w4))
    for case in BIG_CASES:
        kernel, K, loop = case[:3]
        f = big_form(K, loop, len(case) > 3)
        assert dispatch(BIG_M, BIG_N, K, f, SELECT[kernel]) == (kernel, loop)
        scales = ("fast" if fast_scales(K, f) else "slow") if kernel == "pp" and f.out != "i32" else "-"
        # full / ragged: the kinds of tile that the workgroups WITH SEVERAL TILES hold, from the walk
        for full in {full for w in persistent_walk(BIG_M, BIG_N)[1] if len(w) > 1 for mi, ni, full in w}:
            reached.add((kernel, loop, "full" if full else "ragged", "several", scales, f.w4))
    loops = {"v1": ("epilogue",), "v2": ("16", "16res", "f32", "f32res", "i32"), "pp": ("16", "f32", "f32res", "i32")}
    for w4 in (False, True):  # v1's one epilogue in every output type, with and without the residual, W8 and W4
        v1 = {(f.out, f.epi) for k, M, N, K, w in SMALL_CASES if k == "v1" and w == w4 for f in forms_of_case(k, M, N, K, w)}
        assert v1 == {("i32", "none")} | {(o, e) for o in ("f16", "bf16", "f32") for e in ("none", "res", "inplace")}
    missing = []
    for kernel, ls in loops.items():
        for loop in ls:
            for full in ("full", "ragged"):
                for tiles in ("one",) if kernel == "v1" else ("one", "several"):
                    for scales in ("fast", "slow") if kernel == "pp" and loop != "i32" else ("-",):
                        if (kernel, loop, full, tiles, scales, False) not in reached:
                            missing.append((kernel, loop, full, tiles, scales))
            if kernel != "pp" and not {(kernel, loop, full, "one", "-", True) for full in ("full", "ragged")} <= reached:
                missing.append((kernel, loop, "w4"))
    assert not missing, missing
    # the walk of the persistent kernels at the table's shapes
    for M, N in {(M, N) for k, M, N, K, w4 in SMALL_CASES if k != "v1"} | {(BIG_M, BIG_N)}:
        grid, walks = persistent_walk(M, N)
        mt, nt = -(-M // 256), -(-N // 256)
        seen = sorted((mi, ni) for w in walks for mi, ni, full in w)
        assert seen == [(mi, ni) for mi in range(mt) for ni in range(nt)], "the walk visits every tile once"
    grid, walks = persistent_walk(520, 264)
    assert grid == 8 and sum(1 for w in walks if not w) == 2  # six tiles: two workgroups return at once
    grid, walks = persistent_walk(BIG_M, BIG_N)
    mt, nt = -(-BIG_M // 256), -(-BIG_N // 256)
    assert (mt, nt, grid) == (38, 7, 256) and (mt * nt) % 8 == 2 and mt % GROUP_M == 2 and BIG_N - (nt - 1) * 256 == 8 and BIG_M % 256 == 5
    orders = {(w[0][2], w[1][2]) for w in walks if len(w) == 2}
    assert (True, False) in orders and (False, True) in orders, orders
    # v2 at one K-tile, v1 with a K tail of 16 and of 32, v1's short last group of m-tiles, one-row problems
    assert ("v2", 520, 264, 128, False) in SMALL_CASES and ("v2", 520, 264, 128, True) in SMALL_CASES
    assert {K % 128 for k, M, N, K, w4 in SMALL_CASES if k == "v1"} >= {16, 32}
    assert any(k == "v1" and -(-M // 128) % GROUP_M != 0 and -(-M // 128) > GROUP_M for k, M, N, K, w4 in SMALL_CASES)
    assert {K for k, M, N, K, w4 in SMALL_CASES if k == "pp"} == {256, 384, 512}  # below, below and at the fast_scales boundary


def test_gpu_part_is_marked():
    import inspect
    import sys

    first_cpu = inspect.getsourcelines(test_shape_table_reaches_every_form)[1]
    for name, fn in list(vars(sys.modules[__name__]).items()):
        if name.startswith("test_") and inspect.isfunction(fn) and inspect.getsourcelines(fn)[1] < first_cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name


CPU_SHAPES = [(1, 8, 16), (130, 136, 144), (130, 136, 160), (520, 264, 128), (777, 264, 512)]


@pytest.mark.parametrize("M,N,K", CPU_SHAPES + [(BIG_M, BIG_N, 256)])
def test_probe_hits_every_k_tile_and_encodes_rows_columns_and_tile_edges(M, N, K):
    p = Probe(M, N, K)
    nkt = -(-K // 128)
    assert int(p.km.max()) < K and int(p.am.abs().min()) >= 1 and int(p.am.abs().max()) <= 3 and int(p.w.min()) == -8 and int(p.w.max()) == 7
    for tile in (128, 256):  # every K-tile of every block of rows that has at least as many rows as there are K-tiles
        for r0 in range(0, M, tile):
            kts = set((p.km[r0:r0 + tile] // 128).tolist())
            assert len(kts) == min(nkt, len(p.km[r0:r0 + tile])), (tile, r0)
    if M >= 128:
        assert len(set((p.km % 128 // 16).tolist())) == min(8, K // 16) and len(set((p.km % 16).tolist())) == 16  # every 16-B chunk, every byte
    # a value taken from d rows / columns further on changes the output: the per-row and per-column tuples differ between every two
    # neighbouring aligned groups of d, on both sides of every tile edge included
    rows = torch.stack([p.sa, p.am.double(), p.km.double()], 1)
    cols = torch.stack([p.sw, p.zp, p.bias, p.gate], 1)
    for t, n in ((rows, M), (cols, N)):
        for d in (1, 4, 8, 16, 32, 64, 128, 256):
            if n < 2 * d:
                continue
            k = (n - d) // d * d
            same = (t[:k].reshape(-1, d, t.shape[1]) == t[d:d + k].reshape(-1, d, t.shape[1])).all(2).all(1)
            assert not bool(same.any()), (n, d)
            # ... and most single values differ from the one d places further on
            assert float((t[:n - d] == t[d:]).all(1).double().mean()) < 0.05, (n, d)
    # moved by one row, one 4-column group or one tile, the exact output changes in every tile
    if M >= 130:
        e = p.expect(Form("f32", "f32", True, True, "res", False, False))
        for dr, dc in ((1, 0), (0, 4), (0, 8), (0, 16), (0, 32), (0, 64), (16, 0), (128, 0), (0, 128)):
            moved = e[dr:, dc:] != e[:M - dr, :N - dc]
            assert float(moved.double().mean()) > 0.5, (dr, dc)


def test_probe_intermediates_are_exact_in_float32_in_both_term_orders():
    """float64 and float32, the v1 order (acc sa) sw + (asum zp) sw + bias and the v2 / pp order fma(acc sa, sw, fma(asum, zp sw,
    bias)), then gate y + residual: the same bits at every step, for W8 and W4 codes; the vectors are exact in fp16, zp in int16, the
    residual in bf16 and fp16."""
    f, d = np.float32, np.float64
    for M, N, K in CPU_SHAPES:
        p = Probe(M, N, K)
        for name in ("sa", "asum", "sw", "bias", "gate", "res"):
            v = getattr(p, name)
            assert torch.equal(v.to(torch.float16).double(), v), name
        assert torch.equal(p.res.to(torch.bfloat16).double(), p.res) and torch.equal(p.zp.to(torch.int16).double(), p.zp)
        assert torch.equal(p.asum, p.a_matrix().double().sum(1) * p.sa)  # the true row sum
        assert torch.equal(p.acc, p.a_matrix().long() @ p.w.T)           # the gather is the matrix product
        for w4 in (False, True):
            form = Form("f32", "f32", True, True, "res", False, w4)
            acc, zp, bias = [t.numpy() for t in p.terms(form)]
            sa, asum, sw, gate, res = [t.numpy() for t in (p.sa, p.asum, p.sw, p.gate, p.res)]
            steps = {}
            for t in (d, f):
                A, SA, AS, SW, Z, B, G, R = [x.astype(t) for x in (acc, sa[:, None], asum[:, None], sw[None, :], zp[None, :], bias[None, :], gate[None, :], res)]
                t1 = (A * SA).astype(t)
                t1s = (t1 * SW).astype(t)
                t2 = ((AS * Z).astype(t) * SW).astype(t)
                zs = (Z * SW).astype(t)
                t2b = (AS * zs).astype(t)
                v1 = ((t1s + t2).astype(t) + B).astype(t)
                v2 = (t1s + (t2b + B).astype(t)).astype(t)
                steps[t] = [t1, t1s, t2, zs, t2b, (t2b + B).astype(t), (t1s + t2).astype(t), v1, v2, (v1 * G).astype(t), (R + (v1 * G).astype(t)).astype(t)]
            for x64, x32 in zip(steps[d], steps[f]):
                assert np.array_equal(x64, x32.astype(d))
            pre, out = steps[d][7], steps[d][10]
            assert np.array_equal(steps[d][7], steps[d][8]) and np.array_equal(pre, p.pre(form).numpy())
            assert np.abs(pre).max() <= (64 if not w4 else 160) and np.array_equal(pre * 32, np.round(pre * 32)) and np.array_equal(out * 64, np.round(out * 64))
            # one rounding into the 16-bit types: not the identity (ties and inexact values occur), so the rounding mode is tested
            if M >= 130:
                o = torch.from_numpy(out)
                assert not torch.equal(o.to(torch.bfloat16).double(), o)
                frac = out * 2.0 ** (7 - np.floor(np.log2(np.maximum(np.abs(out), 2.0 ** -6))))  # in units of the bf16 step
                assert (np.abs(frac - np.floor(frac) - 0.5) == 0).any(), "a bf16 tie occurs"


# ------------------------------------------------------------------------------------------------ the numpy model and its mutants
def to_bits(y, out, truncate=False):
    """float64 [M, N] -> the bit pattern of its one rounding into the output type (int64)."""
    if out == "i32":
        return y.astype(np.int64)
    if out == "f32":
        return y.astype(np.float32).view(np.int32).astype(np.int64)
    t = torch.from_numpy(np.ascontiguousarray(y.astype(np.float32)))
    if out == "bf16" and truncate:
        return (t.view(torch.int32) >> 16).to(torch.int16).numpy().astype(np.int64)
    return t.to(TDT[out]).view(torch.int16).numpy().astype(np.int64)


def fma32(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu_fast_model(y):
    """gelu_tanh_fast_f32 in numpy fp32 (exp2 and the reciprocal as numpy rounds them)."""
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        t = (y * fma32(y * y, np.full_like(y, f(-0.10294324)), np.full_like(y, f(-2.3022082)))).astype(f)
        return (y * (f(1) / (f(1) + np.exp2(t, dtype=f))).astype(f)).astype(f)


def model(v, M, N, K, form, order, tile, mutant=None, res=None):
    """A plain fp32 model of the three kernels' epilogue on the operands v (numpy: acc int64, sa, asum, sw, zp, bias, gate), written
    tile by tile into a sentinel-filled flat buffer; returns the Window it filled (CPU).  order: v1 | v2."""
    f = np.float32
    win = Window(M, N, form.out, "cpu")
    flat = win.flat.numpy()
    W = flat[GUARD:GUARD + M * N].reshape(M, N)
    acc = v["acc"].copy()
    if mutant == "k_tile_dropped":  # K-tile 0 of the last m-tile never reaches the accumulators
        rows = np.arange(M) >= (M - 1) // tile * tile
        acc[rows & (v["km"] < 128)] = 0
    if form.out == "i32":
        bits = acc
    else:
        r32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float16 if form.vec == "f16" else torch.float32).float().numpy()
        sa, asum, sw, bias, gate = r32(v["sa"])[:, None], r32(v["asum"])[:, None], r32(v["sw"])[None, :], r32(v["bias"])[None, :], v["gate"].astype(f)[None, :]
        zp = v["zp"].astype(f)[None, :]
        n, m = np.arange(N), np.arange(M)
        last_n0, last_m0 = (N - 1) // tile * tile, (M - 1) // tile * tile
        if mutant == "sw_shifted":  # sW of the next 4-channel group
            sw = sw[:, np.minimum(n + 4, N - 1)]
        zs_sw, zs_zp = sw, zp
        if mutant == "zp_sw_clamped":  # zp * sW of a ragged n-tile from the clamped column N - 1
            cl = np.where((n >= last_n0) & (last_n0 + tile > N), N - 1, n)
            zs_sw, zs_zp = sw[:, cl], zp[:, cl]
        if mutant == "sa_clamped":  # the last (partial) 16-row block of a ragged m-tile takes sA of row M - 1
            sa = sa[np.where((m >= (M - 1) // 16 * 16) & (M % tile != 0), M - 1, m)]
        a = acc.astype(f)
        if not form.zp:
            asum, zs_zp = np.zeros_like(asum), np.zeros_like(zp)
        if not form.bias:
            bias = np.zeros_like(bias)
        if order == "v1":
            y = ((a * sa).astype(f) * sw).astype(f)
            y = (y + ((asum * zs_zp).astype(f) * zs_sw).astype(f)).astype(f)
            y = (y + bias).astype(f)
        else:
            y = fma32((a * sa).astype(f), np.broadcast_to(sw, a.shape), fma32(np.broadcast_to(asum, a.shape), (zs_zp * zs_sw).astype(f), bias))
        if form.gelu:
            y = gelu_fast_model(y)
        if form.epi != "none":
            r = (v["res"] if res is None else res).astype(f)
            r = torch.from_numpy(r).to(TDT[form.out]).float().numpy()
            if mutant == "bias_after_gate":
                y = (fma32((y - bias).astype(f), gate, r) + bias).astype(f)
            else:
                y = fma32(y, gate, r) if order == "v2" else (r + (y * gate).astype(f)).astype(f)
            if mutant == "residual_twice":
                y = (y + r).astype(f)
        bits = to_bits(y.astype(np.float64), form.out, truncate=(mutant == "bf16_truncated"))
    mt, nt = -(-M // tile), -(-N // tile)
    for mi in range(mt):
        for ni in range(nt):
            r0, c0 = mi * tile, ni * tile
            blk = bits[r0:r0 + tile, c0:c0 + tile]
            if mutant == "tile_unwritten" and (mi, ni) == (mt - 1, 0):
                continue
            if mutant == "tile_at_neighbour" and (mi, ni) == (0, nt - 1):  # stored at the origin of the n-tile in front
                c0 -= tile
                W[r0:r0 + blk.shape[0], c0:c0 + blk.shape[1]] = blk
                continue
            W[r0:r0 + blk.shape[0], c0:c0 + blk.shape[1]] = blk
    if mutant == "guard_front":
        flat[GUARD - 1] = bits[0, 0]
    if mutant == "guard_behind":
        flat[GUARD + M * N] = bits[-1, -1]
    return win


def probe_values(p, form):
    acc, zp, bias = p.terms(form)
    return dict(acc=acc.long().numpy(), km=p.km.numpy(), sa=p.sa.numpy(), asum=p.asum.numpy(), sw=p.sw.numpy(),
                zp=(zp if zp is not None else p.zp).numpy(), bias=p.bias.numpy(), gate=p.gate.numpy(), res=p.res.numpy())


MODEL_FORMS = [Form("i32", "f32", False, False, "none", False, False), Form("bf16", "f32", True, True, "res", False, False),
               Form("f16", "f16", True, False, "none", False, True), Form("f32", "f16", False, True, "inplace", False, False),
               Form("bf16", "f16", True, True, "inplace", False, True), Form("f16", "f32", False, False, "res", False, False)]


@functools.lru_cache(maxsize=4)
def cpu_probe(M, N, K):
    return Probe(M, N, K)


@pytest.mark.parametrize("M,N,K,tile", [(130, 136, 160, 128), (777, 264, 256, 256)])
@pytest.mark.parametrize("order", ["v1", "v2"])
def test_model_passes_the_exact_probe_in_both_term_orders(M, N, K, tile, order):
    p = cpu_probe(M, N, K)
    for form in MODEL_FORMS:
        win = model(probe_values(p, form), M, N, K, form, order, tile)
        assert check_exact(win, p.expect(form), tile) == [], form


MUTANTS = ["tile_unwritten", "tile_at_neighbour", "zp_sw_clamped", "sw_shifted", "sa_clamped", "bias_after_gate", "residual_twice",
           "k_tile_dropped", "bf16_truncated", "guard_front", "guard_behind"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_the_exact_probe(mutant):
    """Each mutant fails the Section A checker at the small v1 shape and at the pp / v2 shape, in both term orders."""
    form = Form("bf16", "f32", True, True, "res", False, False)
    for M, N, K, tile in ((130, 136, 160, 128), (777, 264, 256, 256)):
        p = cpu_probe(M, N, K)
        for order in ("v1", "v2"):
            fails = check_exact(model(probe_values(p, form), M, N, K, form, order, tile, mutant), p.expect(form), tile)
            assert fails, (mutant, M, order)
            if mutant.startswith("guard"):
                assert len(fails) == 1 and "guard" in fails[0]


def test_gelu_reference_and_model_within_the_bound():
    """The stable form of the reference equals 0.5 x (1 + tanh u) where that form is well conditioned; the fp32 model of the fast
    GELU stays within the derived bound on every multiple of 2^-5 in [-64, 64], and a GELU without its cubic term does not."""
    x = torch.arange(-2048, 2049, dtype=torch.float64) / 32
    u = math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)
    plain = 0.5 * x * (1 + torch.tanh(u))
    assert float((gelu_ref(x) - plain).abs().max()) <= 2.0 ** -48 and bool((gelu_ref(x[:1600]) <= 0).all()) and float(gelu_ref(x)[-1]) == 64.0
    assert abs(C1F - C1) < 2.0 ** -24 * 2.4 and abs(C3F - C3) < 2.0 ** -24 * 0.11
    got = torch.from_numpy(gelu_fast_model(x.numpy().astype(np.float32)).astype(np.float64))
    ratio = (got - gelu_ref(x)).abs() / gelu_bound(x)
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    rel = ((got - gelu_ref(x)).abs() / gelu_ref(x).abs().clamp(min=2.0 ** -120))[(x.abs() <= 4) & (x != 0)]
    assert float(rel.max()) < 3e-6  # the claim of the kernel's comment, over the range where GELU is not saturated
    wrong = x * torch.special.expit(2 * math.sqrt(2 / math.pi) * x)
    assert float(((wrong - gelu_ref(x)).abs() / gelu_bound(x)).max()) > 100


def test_model_within_the_random_data_bound_and_a_wrong_order_is_not():
    """The fp32 model in both term orders stays within the bound of RandomCase.reference on every output type; a model that rounds
    acc sa sw into fp16 first does not."""
    M, N, K = 130, 136, 144
    case = RandomCase(M, N, K, "cpu")
    h = case.host
    for out in ("f16", "bf16", "f32"):
        for vec in ("f32", "f16"):
            for epi in ("none", "inplace"):
                form = Form(out, vec, True, True, epi, False, False)
                ref, bound = case.reference(form)
                for order in ("v1", "v2"):
                    v = dict(acc=case.acc.long().numpy(), km=None, gate=case.gate.numpy(), res=case.res.numpy(), **{k: x.numpy() for k, x in h.items()})
                    win = model(v, M, N, K, form, order, 128)
                    fails, ratio = check_bound(win, ref, bound)
                    assert not fails and ratio <= 1.0, (form, order, ratio)
    form = Form("f32", "f32", True, True, "none", False, False)
    ref, bound = case.reference(form)
    win = Window(M, N, "f32", "cpu")
    t1 = (case.acc * h["sa"].float().double()[:, None] * h["sw"].float().double()[None, :]).to(torch.float16).double()
    y = t1 + h["asum"].float().double()[:, None] * (h["zp"] * h["sw"].float().double())[None, :] + h["bias"].float().double()[None, :]
    win.window().copy_(y.float())
    assert check_bound(win, ref, bound)[0]
