"""The bf16 / fp16 GEMM (csrc/gemm_bf16.hip, wanq_gemm_bf16) and the epilogue it shares with the weight-only GEMMs (epilogue16 of
csrc/gemm16_common.h; wanq_gemm_wq16, wanq_gemm_wq16_grouped) on operands whose answer is known exactly.  Every call goes through the
C ABI and the test owns every buffer: the output is a window in a flat allocation with guard zones of GUARD elements in front and
behind, the whole allocation holds a quiet-NaN bit pattern before EVERY launch, and after it both guards must still hold that pattern.

  A  exact probes of the FP kernel: integer operands, every fp32 intermediate exact, so summation order, the matrix cores' internals
     and fma contraction cannot matter: the output equals the one rounding of a known integer.  Dense operands over a shape table,
     one-hot rows (which k reaches which fragment slot), encoded operands (a failure names row, column and K-tile).
  B  the shared epilogue on all three entries: bias none / fp16 / bf16 / fp32 x gate + residual none / out of place / in place x
     output type, exactly; GELU on exact pre-activations under the bound derived in profiles/PARITY_NOTES.md.
  C  isolation: a huge row M - 1, a huge weight row N - 1, a huge column N - 1, one NaN and one Inf stay where the definition puts them.
  D  M = 0 and one refused call leave the sentinel-filled window untouched.
  E  CPU self-tests (not marked gpu): a numpy model of the kernel as written (tile origin, clamps, the DMA lane map with its swizzle,
     koff and the half-tile rule, frag_addr, two 32-deep steps, the epilogue's lane map, one rounding) passes the checkers of A - C;
     mutants of it fail named probes; the shape table's coverage, the tie counts and the exactness of every expectation are proved.

Every probe is a function of a `run` callable, so that the GPU (GpuRun) and the model (ModelRun) go through the same checkers.
Kernel rules restated here: TM = TN = 128, TK = 64, nk = ceil(K / 64), the last tile is `half` when K % 64 == 32."""
import collections
import math

import numpy as np
import pytest
import torch

# The GPU part (sections A - D) is marked test by test, so that section E below runs without a GPU; test_gpu_part_is_marked keeps a
# test added above section E from being left unmarked.
gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DTC = {"f16": 0, "bf16": 1, "f32": 2}  # WANQ_F16 / BF16 / F32 (include/wanq_hip.h)
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}
TINY = {"f16": 2.0 ** -25, "bf16": 2.0 ** -126, "f32": 2.0 ** -126}
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
EPI_GELU, EPI_GATE_RES = 1, 2
GUARD = 4096  # elements; a multiple of 16, so the window stays 16-byte aligned in every type
SENT_BITS = {"f16": 0x7E5A, "bf16": 0x7FC5, "f32": 0x7FC5A5A5}  # quiet NaNs with a payload; compared as integers
TM, TN, TK = 128, 128, 64
OPS, OUTS = ("bf16", "f16"), ("f16", "bf16", "f32")
ENTRIES = ("fp", "wq", "wqg")  # wanq_gemm_bf16, wanq_gemm_wq16 (W8, zp NULL), wanq_gemm_wq16_grouped (W8, zp NULL, groups of 64)
GROUP = 64

Result = collections.namedtuple("Result", "win fails")


# ================================================================================================ buffers and checkers
class Window:
    """The output as a window of M * N elements inside a flat allocation with GUARD elements in front and behind."""

    def __init__(self, M, N, out, dev):
        self.M, self.N, self.out = M, N, out
        self.idt = torch.int32 if out == "f32" else torch.int16
        self.flat = torch.full((2 * GUARD + M * N,), SENT_BITS[out], dtype=self.idt, device=dev)

    def bits(self):
        return self.flat[GUARD:GUARD + self.M * self.N].view(self.M, self.N)

    def window(self):
        return self.bits().view(TDT[self.out])

    def ptr(self):
        p = self.flat.data_ptr() + GUARD * self.flat.element_size()
        assert p % 16 == 0
        return p


def guard_failures(win):
    s, n = SENT_BITS[win.out], GUARD + win.M * win.N
    fails = []
    if bool((win.flat[:GUARD] != s).any()):
        fails.append(f"the guard in front of the output was written at element {int((win.flat[:GUARD] != s).nonzero()[0]) - GUARD}")
    if bool((win.flat[n:] != s).any()):
        fails.append(f"the guard behind the output was written at element {win.M * win.N + int((win.flat[n:] != s).nonzero()[0])}")
    return fails


def check_exact(res, expect, describe=None):
    """Equality of every element of the window with `expect` (an element that still holds the sentinel is a NaN: unequal), guards
    intact.  describe(m, n, got) adds what the probe knows about the first bad element."""
    win = res.win
    fails = list(res.fails) + guard_failures(win)
    got = win.window()
    bad = ~(got.double() == expect.double())
    if bool(bad.any()):
        idx = bad.nonzero()
        r, c = int(idx[0, 0]), int(idx[0, 1])
        unwritten = int((win.bits()[bad] == SENT_BITS[win.out]).sum())
        tiles = sorted({(int(i) // TM, int(j) // TN) for i, j in idx[:: max(1, len(idx) // 64)].tolist()})[:6]
        more = "" if describe is None else "; " + describe(r, c, float(got[r, c]))
        fails.append(f"{len(idx)} elements differ ({unwritten} of them never written), tiles {tiles}; first at row {r} col {c}: "
                     f"got {got[r, c].item()} expected {expect[r, c].item()}{more}")
    return fails


def check_bound(res, ref, bound):
    """|out - ref| <= bound elementwise (NaN fails), guards intact.  Returns (failures, largest err / bound)."""
    win = res.win
    fails = list(res.fails) + guard_failures(win)
    err = (win.window().double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        r, c = [int(v) for v in bad.nonzero()[0]]
        fails.append(f"{int(bad.sum())} elements beyond the bound; first at row {r} col {c}: got {win.window()[r, c].item()} ref {ref[r, c].item()} "
                     f"bound {bound[r, c].item():.3e}")
    return fails, float(torch.nan_to_num(err / bound, nan=float("inf")).max())


def hash32(r, c, salt):
    """A fixed integer hash of (r, c): int64 tensor of values below 2^32 (the products wrap mod 2^64; the low 32 bits are kept)."""
    m = 0xFFFFFFFF
    h = (r * 0x9E3779B1 + c * 0x85EBCA77 + (salt * 0x27D4EB2F + 1)) & m
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & m
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & m
    return h ^ (h >> 15)


def ints(R, C, salt, lo, hi, dev):
    """int64 [R, C] (or [R] when C is None) of hashed integers in [lo, hi]."""
    r = torch.arange(R, dtype=torch.int64, device=dev)
    if C is None:
        return hash32(r, torch.zeros((), dtype=torch.int64, device=dev), salt) % (hi - lo + 1) + lo
    return hash32(r[:, None], torch.arange(C, dtype=torch.int64, device=dev)[None, :], salt) % (hi - lo + 1) + lo


def pow2(e):
    """2^e for an int64 tensor e in [-8, 8], from a table (a device's pow need not be exact)."""
    return torch.tensor([2.0 ** i for i in range(-8, 9)], dtype=torch.float64, device=e.device)[e + 8]


def exact_in(x, *dts):
    return all(torch.equal(x.double().to(TDT[d]).double(), x.double()) for d in dts)


# ================================================================================================ the GPU runner
class GpuRun:
    """run(entry, op, out, a, w, ...): one launch through the C ABI into a fresh sentinel-filled window.  a [M, K] and w [N, K] hold
    values exact in the operand type (w: the int8 codes for the weight-only entries); sw [N] or [K / 64, N]; bias, gate [N] and
    res [M, N] float64 of values exact in their storage type.  The residual is placed in the window when `inplace`."""
    dev = DEV

    def __call__(self, entry, op, out, a, w, sw=None, bias=None, bias_dt="f32", gate=None, res=None, inplace=False, gelu=False):
        from viditq_extension import _C

        (M, K), N = a.shape, w.shape[0]
        a16 = a.to(TDT[op]).contiguous()
        wk = w.to(TDT[op] if entry == "fp" else torch.int8).contiguous()
        b = None if bias is None else bias.to(TDT[bias_dt]).contiguous()
        g = None if gate is None else gate.float().contiguous()
        s = None if sw is None else sw.float().contiguous()
        win = Window(M, N, out, DEV)
        r = r0 = None
        if gate is not None:
            if inplace:
                win.window().copy_(res.to(TDT[out]))
            else:
                r = res.to(TDT[out]).contiguous()
                r0 = r.clone()
        epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
        rp = None if gate is None else win.ptr() if inplace else _C.ptr(r)
        tail = (win.ptr(), DTC[out], _C.ptr(b), DTC[bias_dt], _C.ptr(g), rp, epi, M, N, K, _C.stream())
        if entry == "fp":
            rc = _C.lib.wanq_gemm_bf16(_C.ptr(a16), _C.ptr(wk), DTC[op], *tail)
        elif entry == "wq":
            rc = _C.lib.wanq_gemm_wq16(_C.ptr(a16), _C.ptr(wk), DTC[op], 8, _C.ptr(s), None, *tail)
        else:
            rc = _C.lib.wanq_gemm_wq16_grouped(_C.ptr(a16), _C.ptr(wk), DTC[op], 8, _C.ptr(s), None, GROUP, *tail)
        torch.cuda.synchronize()
        assert rc == WANQ_OK, (rc, _C.lib.wanq_last_error().decode())
        fails = []
        if r is not None and not torch.equal(r.view(win.idt), r0.view(win.idt)):
            fails.append("the out-of-place residual was written")
        return Result(win, fails)


# ================================================================================================ A. exact probes of the FP kernel
MS, NS, KS = (1, 127, 128, 129, 257), (8, 72, 136, 264), (32, 64, 96, 128, 160, 192)
TIE_ELEMS = 129 * 136  # the tie condition is asserted on every 16-bit case with at least this many elements


def weight_range(K, out):
    """|w| <= 255 (exact in bf16 and fp16); for an fp16 output narrowed so that 4 K |w| < 65504 whatever the signs."""
    return 255 if out != "f16" else min(255, 65503 // (4 * K))


def tie_counts(y64, out):
    """(#ties whose even neighbour lies below in magnitude, #ties whose even neighbour lies above) of integers |y| < 2^24 in a 16-bit
    type: the fp32 pattern of y ends in exactly 1000...0 below the type's last kept bit; that bit says which neighbour is even."""
    low = 16 if out == "bf16" else 13
    b = y64.float().view(torch.int32)
    tie = (b & ((1 << low) - 1)) == (1 << (low - 1))
    odd = ((b >> low) & 1) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum())


class FpCase:
    """Dense integer operands: a in [-4, 4], w in [-wmax, wmax]; y64 = a w^T exactly, |y64| < 2^24."""

    def __init__(self, M, N, K, out, dev):
        assert K <= 16448
        wmax = weight_range(K, out)
        self.a, self.w = ints(M, K, 21, -4, 4, dev), ints(N, K, 22, -wmax, wmax, dev)
        assert exact_in(self.a, "bf16", "f16") and exact_in(self.w, "bf16", "f16")
        self.y64 = self.a.double() @ self.w.double().T
        assert float(self.y64.abs().max()) < 2 ** 24
        if out == "f16":
            assert float(self.y64.abs().max()) < 65504
        self.expect = self.y64.to(TDT[out])
        self.ties = tie_counts(self.y64, out) if out != "f32" else None
        if out != "f32" and M * N >= TIE_ELEMS:  # a condition on the inputs: the rounding mode is tested in both directions
            assert min(self.ties) >= 200, (M, N, K, out, self.ties)


def shape_table():
    """(M, N, K, op, out): per (K, operand type, output type) the four N against four M by a rotation, M = 257 against another N, and
    (129, 136), the shape of the tie counts.  test_shape_table_reaches_every_case proves what this reaches."""
    cases = []
    for ki, K in enumerate(KS):
        for oi, op in enumerate(OPS):
            for ti, out in enumerate(OUTS):
                rot = ki + 2 * oi + ti
                pairs = [(MS[i], NS[(i + rot) % 4]) for i in range(4)] + [(257, NS[(rot + 2) % 4]), (129, 136)]
                cases += [(M, N, K, op, out) for M, N in dict.fromkeys(pairs)]
    return cases


SHAPE_CASES = shape_table()


def edge_kinds(M, N):
    """The structural cases of the issue that (M, N) reaches under TM = TN = 128: which rows the clamp at M - 1 pads, which 4-channel
    groups and wave columns of the last n-tile are live, how many tiles the block id is split over."""
    mt, nt, lastn = -(-M // TM), -(-N // TN), N - (-(-N // TN) - 1) * TN
    kinds = {f"M={M}", f"N={N}"}
    if M == 1:
        kinds.add("one row: 127 padded rows read row 0")
    if M % TM == 0:
        kinds.add("full m-tile")
    if M % TM == 1 and mt > 1:
        kinds.add("one row into the last m-tile")
    if mt == 3:
        kinds.add("three m-tiles")
    if N == 8:
        kinds.add("two 4-channel groups in all")
    if 64 < lastn < 128:
        kinds.add("wave column 1 partly live")
    if lastn <= 64 and nt > 1:
        kinds.add("wave column 1 wholly past N in the last n-tile")
    if nt == 3:
        kinds.add("nt = 3")
    return kinds


def probe_exact(run, M, N, K, op, out):
    case = FpCase(M, N, K, out, run.dev)
    return check_exact(run("fp", op, out, case.a, case.w), case.expect)


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("K", KS)
def test_exact_probe_over_the_shape_table(K, op):
    """Every case of the table at this (K, operand type): equality with the one rounding of the exact integer, guards intact."""
    fails, n = [], 0
    for M, N, k, o, out in SHAPE_CASES:
        if (k, o) == (K, op):
            fails += [f"({M}, {N}, {K}) {op} -> {out}: {f}" for f in probe_exact(GpuRun(), M, N, K, op, out)]
            n += 1
    assert n >= 15
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


def probe_one_hot(run, K, op, N=136):
    """Row m of a is e_m for every m < K: the output row is weight column m exactly.  A k that reaches the wrong fragment slot, a skipped
    first half in place of the second or a doubled first half returns another column, or a sum of two."""
    w = ints(N, K, 23, -255, 255, run.dev)
    assert len({tuple(c.tolist()) for c in w.T}) == K  # pairwise different columns: the probe can tell them apart
    a = torch.eye(K, dtype=torch.int64, device=run.dev)

    def describe(m, n, got):
        ks = (w[n].double() == got).nonzero().flatten().tolist()
        return f"k = {m} (K-tile {m // TK}, step {m % TK // 32}); the value is that of k in {ks[:4]}"

    return check_exact(run("fp", op, "f32", a, w), w.T.double().contiguous(), describe)


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("K", [96, 160])
def test_one_hot_rows_return_the_weight_column(K, op):
    fails = probe_one_hot(GpuRun(), K, op)
    assert not fails, "\n".join(fails)


ENC_M, ENC_N = 257, 264


def probe_encoded(run, K, op, out="f32"):
    """a[m, :] is one-hot at k = m % K scaled by 1 + (m // K) % 4, w[n, k] = (17 n + 5 k) % 251 - 125: y[m, n] names m, n and k."""
    dev = run.dev
    m, n, k = [torch.arange(x, dtype=torch.int64, device=dev) for x in (ENC_M, ENC_N, K)]
    scale = 1 + (m // K) % 4
    a = torch.zeros(ENC_M, K, dtype=torch.int64, device=dev)
    a[m, m % K] = scale
    w = (17 * n[:, None] + 5 * k[None, :]) % 251 - 125
    y = (scale[:, None] * w[:, m % K].T).double()
    assert torch.equal(y, a.double() @ w.double().T)

    def describe(r, c, got):
        kk, s = r % K, int(scale[r])
        ks = (w[c].double() * s == got).nonzero().flatten().tolist()
        return (f"row {r} = {s} e_{kk}: K-tile {kk // TK} of {-(-K // TK)}, step {kk % TK // 32}, chunk {kk % 32 // 8}; m-tile {r // TM}, n-tile {c // TN}; "
                f"the value is {s} w[{c}, k] for k in {ks[:4]}")

    return check_exact(run("fp", op, out, a, w), y.to(TDT[out]), describe)


@gpu
@pytest.mark.parametrize("K", KS)
def test_encoded_operands_name_row_column_and_k_tile(K):
    """One case per (nk, half): nk = 1, 2, 3 is buffer 0 only, both buffers, buffer 0 reused after the barrier."""
    fails = probe_encoded(GpuRun(), K, OPS[(K // 32) % 2])
    assert not fails, "\n".join(fails)


# ================================================================================================ B. the shared epilogue
EPI_M, EPI_N = 129, 136
EPI_K = {"fp": 96, "wq": 128, "wqg": 128}
BIAS_KINDS, EPI_KINDS = (None, "f16", "bf16", "f32"), ("none", "res", "inplace")
RES_MAX = {"bf16": 256, "f16": 2048, "f32": 2 ** 15 - 1}


class EpiCase:
    """Exact operands of the epilogue.  a in [-4, 4]; w (codes) in [-127, 127], for an fp16 output [-31, 31] so that the result stays
    finite; sw = 2^-{0..6}; integer bias, |b| <= 256; gate one of +-{1/4, 1/2, 1, 2}; integer residual exact in the output type.

    Exactness.  acc is an integer below 2^16 and acc sw a scaling of it; y = acc sw + bias is a multiple of sw below 2^16 sw + 2^8.
    y gate is again a scaling.  residual + y gate is a multiple of q = sw |gate| >= 2^-8 whose size in units of q is below
    2^16 + 2^8 / sw + |r| / q <= 2^16 + 2^14 + 2^23 < 2^24 for |r| < 2^15: exact in fp32.  (The residual of an fp32 output therefore
    stays below 2^15, inside the 2^20 the type would hold.)  Products are exact, so fma(y, gate, r) and r + fl(y gate) are the same
    number, as are fma(acc, sw, bias) and fl(acc sw) + bias.  check() asserts all of it in float64 and in float32."""

    def __init__(self, entry, out, dev, M=EPI_M, N=EPI_N):
        K = EPI_K[entry]
        self.entry, self.out, self.M, self.N, self.K = entry, out, M, N, K
        wmax = 31 if out == "f16" else 127
        self.a, self.w = ints(M, K, 31, -4, 4, dev), ints(N, K, 32, -wmax, wmax, dev)
        self.sw = None
        if entry == "wq":
            self.sw = pow2(-ints(N, None, 33, 0, 6, dev))
        elif entry == "wqg":
            self.sw = pow2(-ints(K // GROUP, N, 33, 0, 6, dev))
        self.bias = ints(N, None, 34, -256, 256, dev).double()
        self.gate = (1 - 2 * ints(N, None, 35, 0, 1, dev)).double() * pow2(ints(N, None, 36, 0, 3, dev) - 2)
        self.res = ints(M, N, 37, -RES_MAX[out], RES_MAX[out], dev).double()
        self.check()

    def acc(self, t=torch.float64):
        """acc sw (the FP kernel: acc) in type t, every step rounded to t."""
        a, w = self.a.double(), self.w.double()
        if self.entry == "fp":
            return (a @ w.T).to(t)
        if self.entry == "wq":
            return (a @ w.T).to(t) * self.sw.to(t)[None, :]
        y = torch.zeros(self.M, self.N, dtype=t, device=a.device)
        for g in range(self.K // GROUP):
            k = slice(g * GROUP, (g + 1) * GROUP)
            y = (a[:, k] @ w[:, k].T).to(t) * self.sw[g].to(t)[None, :] + y
        return y

    def pre(self, bias, t=torch.float64):
        y = self.acc(t)
        return y if not bias else y + self.bias.to(t)[None, :]

    def value(self, bias, epi, t=torch.float64):
        y = self.pre(bias, t)
        return y if epi == "none" else self.res.to(t) + y * self.gate.to(t)[None, :]

    def expect(self, bias, epi):
        return self.value(bias, epi).to(TDT[self.out])

    def check(self):
        assert exact_in(self.a, "bf16", "f16") and exact_in(self.w, "bf16", "f16") and exact_in(self.bias, "bf16", "f16", "f32")
        assert exact_in(self.res, self.out) and exact_in(self.gate, "f32") and (self.sw is None or exact_in(self.sw, "f32"))
        assert float((self.a.double().abs() @ self.w.double().abs().T).max()) < 2 ** 16
        for bias in (False, True):
            assert float(self.pre(bias).abs().max()) < 2 ** 20
            for epi in ("none", "res"):
                v64, v32 = self.value(bias, epi), self.value(bias, epi, torch.float32)
                assert torch.equal(v32.double(), v64), (self.entry, self.out, bias, epi)
            y64, g = self.pre(bias), self.gate[None, :]
            assert torch.equal((self.pre(bias, torch.float32) * g.float()).double(), y64 * g)  # the product alone is exact: fma = mul + add
            assert torch.equal(y64 * g * 256, torch.round(y64 * g * 256))
            assert float(self.value(bias, "res").abs().max()) < (65504 if self.out == "f16" else 2 ** 22)
        v = self.value(True, "res")
        if self.out != "f32":  # the rounding is no identity here
            assert not torch.equal(v.to(TDT[self.out]).double(), v)


def probe_epilogue(run, entry, op, out, bias_dt, epi, case=None):
    case = case or EpiCase(entry, out, run.dev)
    kw = dict(sw=case.sw)
    if bias_dt:
        kw.update(bias=case.bias, bias_dt=bias_dt)
    if epi != "none":
        kw.update(gate=case.gate, res=case.res, inplace=epi == "inplace")
    return check_exact(run(entry, op, out, case.a, case.w, **kw), case.expect(bool(bias_dt), epi))


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_epilogue_exactly_on_every_entry(entry, op):
    """bias none / fp16 / bf16 / fp32 x gate + residual none / out of place / in place x output type: the float64 expression rounded
    once, guards intact, the out-of-place residual bit-unchanged."""
    run, fails, n = GpuRun(), [], 0
    for out in OUTS:
        case = EpiCase(entry, out, DEV)
        for bias_dt in BIAS_KINDS:
            for epi in EPI_KINDS:
                fails += [f"{entry} {op} -> {out} bias {bias_dt} {epi}: {f}" for f in probe_epilogue(run, entry, op, out, bias_dt, epi, case)]
                n += 1
    assert n == 36
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ------------------------------------------------------------------------------------------------ GELU on exact pre-activations
C1 = -2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e)  # -2 u log2(e) = x (C1 + C3 x^2)
C3 = C1 * 0.044715
C1F, C3F = float(np.float32(-2.3022082)), float(np.float32(-0.10294324))  # the constants of gelu_tanh_fast_f32 (csrc/wanq_common.h)


def gelu_ref(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), float64, written as x / (1 + e^{-2u})."""
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x * torch.special.expit(2.0 * u)


def gelu_bound(x):
    """Absolute error bound of gelu_tanh_fast_f32(x) against gelu_ref(x): profiles/PARITY_NOTES.md, "Derivation of the GELU bound
    (B)", steps 1 - 5.  x float64, exactly representable in fp32."""
    T = x * (C1 + C3 * x * x)
    dT = 3 * U * T.abs() * (1 + 2.0 ** -10) + x.abs() * abs(C1F - C1) + x.abs() ** 3 * abs(C3F - C3)
    eps_e = torch.expm1(math.log(2.0) * dT) + 2 * U
    s = torch.special.expit(T * math.log(2.0))
    rel = (s * eps_e + U + 2 * U + U) * (1 + 2.0 ** -10)
    return gelu_ref(x).abs() * rel + 2.0 ** -125 * torch.clamp(x.abs(), min=1.0)


def output_bound(y, err, out):
    """err on the fp32 value y, then one rounding into the output type (fp32: the register is stored)."""
    return (err * (1 + U_OUT[out]) + U_OUT[out] * y.abs()) * (1 + 2.0 ** -10) + TINY[out]


class GeluCase:
    """Pre-activations known exactly in [-6, 6]: a = i / 8 with i in [-4, 4]; w = j / 64 with j in [-31, 31] for the FP kernel, the codes
    j with sw in {2^-6, 2^-7} for the weight-only ones; bias = j / 64 in [-1, 1], fp32.  Every product is a multiple of 2^-10 and the
    sums stay below 8: exact in fp32 (13 bits).  Gate and residual: +-{1/4 .. 2} and integers in [-16, 16]."""

    def __init__(self, entry, dev, M=EPI_M, N=EPI_N):
        K = EPI_K[entry]
        self.entry, self.M, self.N = entry, M, N
        ai, wi = ints(M, K, 41, -4, 4, dev), ints(N, K, 42, -31, 31, dev)
        self.a = ai.double() / 8
        self.w = wi.double() / 64 if entry == "fp" else wi
        self.sw = None
        acc = (ai.double() @ wi.double().T) * 2.0 ** -9
        if entry == "wq":
            self.sw = pow2(-ints(N, None, 43, 6, 7, dev))
            acc = (self.a @ wi.double().T) * self.sw[None, :]
        elif entry == "wqg":
            self.sw = pow2(-ints(K // GROUP, N, 43, 6, 7, dev))
            acc = sum((self.a[:, g * GROUP:(g + 1) * GROUP] @ wi.double()[:, g * GROUP:(g + 1) * GROUP].T) * self.sw[g][None, :] for g in range(K // GROUP))
        self.bias = ints(N, None, 44, -64, 64, dev).double() / 64
        self.pre = acc + self.bias[None, :]
        self.gate = (1 - 2 * ints(N, None, 45, 0, 1, dev)).double() * pow2(ints(N, None, 46, 0, 3, dev) - 2)
        self.res = ints(M, N, 47, -16, 16, dev).double()
        assert exact_in(self.a, "bf16", "f16") and exact_in(self.w, "bf16", "f16")
        assert torch.equal(self.pre * 1024, torch.round(self.pre * 1024)) and 3 <= float(self.pre.abs().max()) <= 6
        assert float(self.pre.min()) < -3 and float(self.pre.max()) > 3  # both sides of the curved part

    def reference(self, out, epi):
        """(float64 reference, bound): GELU's error alone (steps 1 - 5), through the gate and the residual (step 6), one rounding."""
        g, eg = gelu_ref(self.pre), gelu_bound(self.pre)
        if epi == "none":
            return g, output_bound(g, eg, out)
        y = self.res + g * self.gate[None, :]
        return y, output_bound(y, self.gate.abs()[None, :] * (eg + U * g.abs()) + U * y.abs(), out)


def probe_gelu(run, entry, op, out, epi, case=None):
    case = case or GeluCase(entry, run.dev)
    kw = dict(sw=case.sw, bias=case.bias, bias_dt="f32", gelu=True)
    if epi != "none":
        kw.update(gate=case.gate, res=case.res, inplace=epi == "inplace")
    ref, bound = case.reference(out, epi)
    return check_bound(run(entry, op, out, case.a, case.w, **kw), ref, bound)


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_gelu_on_exact_preactivations_under_the_derived_bound(entry, op):
    run, case, fails, worst = GpuRun(), GeluCase(entry, DEV), [], {}
    for out in OUTS:
        for epi in EPI_KINDS:
            f, ratio = probe_gelu(run, entry, op, out, epi, case)
            fails += [f"{entry} {op} -> {out} {epi}: {x}" for x in f]
            key = (out, epi != "none")
            worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"RATIO gelu16 {entry} {op} {EPI_M}x{EPI_N}x{EPI_K[entry]} " + " ".join(f"{o}{'+res' if r else ''}={v:.3f}" for (o, r), v in sorted(worst.items())))
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ C. isolation
ISO_M, ISO_N, ISO_K = 129, 136, 96
BIG = {"bf16": 2.0 ** 100, "f16": 32768.0}


def probe_isolation(run, op):
    """A clean run, then one poisoned operand at a time; everything outside the poisoned row / column is bit-equal to the clean run."""
    dev, M, N, K = run.dev, ISO_M, ISO_N, ISO_K
    a, w = ints(M, K, 51, -4, 4, dev).double(), ints(N, K, 52, -255, 255, dev).double()
    bias = ints(N, None, 53, -256, 256, dev).double()
    clean = run("fp", op, "f32", a, w, bias=bias)
    fails = [f"clean: {f}" for f in check_exact(clean, (a @ w.T + bias[None, :]).float())]
    ms, ns, ks = 70, 67, 41  # interior: wave row 1, wave column 1 of the first tiles, chunk 5 of K-tile 0
    rows, cols = torch.arange(M, device=dev), torch.arange(N, device=dev)

    def poisoned(name, a2, w2, row, col, nonfinite):
        res = run("fp", op, "f32", a2, w2, bias=bias)
        out = [f"{name}: {f}" for f in list(res.fails) + guard_failures(res.win)]
        keep = (rows != row)[:, None] & (cols != col)[None, :]
        moved = (res.win.bits() != clean.win.bits()) & keep
        if bool(moved.any()):
            r, c = [int(v) for v in moved.nonzero()[0]]
            out.append(f"{name}: {int(moved.sum())} elements outside row {row} / column {col} changed; first at row {r} col {c}: "
                       f"{res.win.window()[r, c].item()} was {clean.win.window()[r, c].item()}")
        if nonfinite and bool(torch.isfinite(res.win.window())[~keep].any()):
            out.append(f"{name}: finite elements in row {row} / column {col}")
        return out

    a2 = a.clone()
    a2[M - 1] = BIG[op]
    fails += poisoned("row M - 1 of a huge", a2, w, M - 1, -1, False)
    w2 = w.clone()
    w2[N - 1] = BIG[op]
    fails += poisoned("weight row N - 1 huge", a, w2, -1, N - 1, False)
    a2, w2 = a.clone(), w.clone()
    a2[M - 1], w2[N - 1] = BIG[op], BIG[op]
    fails += poisoned("row M - 1 and weight row N - 1 huge", a2, w2, M - 1, N - 1, False)
    a2, w2 = a.clone(), w.clone()
    a2[ms, ks], w2[ns, ks] = float("nan"), float("inf")
    fails += poisoned(f"NaN at a[{ms}, {ks}], Inf at w[{ns}, {ks}]", a2, w2, ms, ns, True)
    return fails


@gpu
@pytest.mark.parametrize("op", OPS)
def test_rows_and_channels_stay_in_their_own_row_and_column(op):
    fails = probe_isolation(GpuRun(), op)
    assert not fails, "\n".join(fails)


# ================================================================================================ D. M = 0 and one refusal
def _abi_call(M, N, K, out):
    from viditq_extension import _C

    a = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, 64, dtype=torch.bfloat16, device=DEV)
    win = Window(8, N, out, DEV)
    rc = _C.lib.wanq_gemm_bf16(_C.ptr(a), _C.ptr(w), DTC["bf16"], win.ptr(), DTC[out], None, DTC["f32"], None, None, 0, M, N, K, _C.stream())
    torch.cuda.synchronize()
    return rc, bool((win.flat == SENT_BITS[out]).all())


@gpu
@pytest.mark.parametrize("out", OUTS)
def test_no_rows_is_ok_and_writes_nothing(out):
    assert _abi_call(0, 16, 64, out) == (WANQ_OK, True)


@gpu
def test_a_refused_call_writes_nothing():
    from viditq_extension import _C

    assert _abi_call(5, 16, 48, "bf16") == (WANQ_E_SHAPE, True)
    assert "multiple of 32" in _C.lib.wanq_last_error().decode()


# ================================================================================================ E. CPU self-tests of the probes
def test_shape_table_reaches_every_case():
    """Every (edge kind, nk, half last tile, operand type, output type) is hit by a case of the table; the one-hot and encoded probes
    reach every (nk, half); all shapes stay within the size the file is allowed."""
    reached = set()
    for M, N, K, op, out in SHAPE_CASES:
        assert M in MS and N in NS and K in KS and N % 8 == 0 and K % 32 == 0
        nk, half = -(-K // TK), K % TK == 32
        for kind in edge_kinds(M, N):
            reached.add((kind, nk, half, op, out))
    kinds = {f"M={M}" for M in MS} | {f"N={N}" for N in NS} | {
        "one row: 127 padded rows read row 0", "full m-tile", "one row into the last m-tile", "three m-tiles", "two 4-channel groups in all",
        "wave column 1 partly live", "wave column 1 wholly past N in the last n-tile", "nt = 3"}
    missing = [(kind, nk, half, op, out) for kind in sorted(kinds) for nk in (1, 2, 3) for half in (False, True) for op in OPS for out in OUTS
               if (kind, nk, half, op, out) not in reached]
    assert not missing, missing[:10]
    assert {(-(-K // TK), K % TK == 32) for K in KS} == {(nk, half) for nk in (1, 2, 3) for half in (False, True)}
    # the kinds say what the issue lists: restated from the kernel's rules
    assert edge_kinds(129, 136) >= {"one row into the last m-tile", "wave column 1 wholly past N in the last n-tile"}
    assert "wave column 1 partly live" in edge_kinds(1, 72) and "nt = 3" in edge_kinds(1, 264) and "three m-tiles" in edge_kinds(257, 8)
    assert all(M <= 257 and N <= 264 and K <= 192 for M, N, K, op, out in SHAPE_CASES) and len(SHAPE_CASES) <= 216
    # every 16-bit (K, operand type, output type) holds a case that carries the tie condition
    for K in KS:
        for op in OPS:
            for out in ("f16", "bf16"):
                assert any(c[2:] == (K, op, out) and c[0] * c[1] >= TIE_ELEMS for c in SHAPE_CASES)


def test_gpu_part_is_marked():
    import inspect
    import sys

    first_cpu = inspect.getsourcelines(test_shape_table_reaches_every_case)[1]
    for name, fn in list(vars(sys.modules[__name__]).items()):
        if name.startswith("test_") and inspect.isfunction(fn) and inspect.getsourcelines(fn)[1] < first_cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name


def test_tie_counts():
    """The integer outputs hold exact ties of both 16-bit types, evenly split between an even neighbour below and above: truncation,
    round-half-up and round-half-away each fail one side."""
    for K in (32, 96, 192):
        for out in ("bf16", "f16"):
            case = FpCase(129, 136, K, out, "cpu")
            dn, up = case.ties
            print(f"TIES (129, 136, {K}) {out}: {dn} + {up} of {129 * 136}")
            assert dn >= 200 and up >= 200 and 0.8 < dn / up < 1.25, (K, out, dn, up)
            # a tie is what it says: the two neighbours in the type are equally far
            y = case.y64
            low = 16 if out == "bf16" else 13
            b = y.float().view(torch.int32)
            tie = (b & ((1 << low) - 1)) == (1 << (low - 1))
            below = ((b >> low) << low).view(torch.float32).double()
            above = (((b >> low) + 1) << low).view(torch.float32).double()
            assert torch.equal((y - below)[tie], (above - y)[tie]) and exact_in(below[tie], out) and exact_in(above[tie], out)
            even = torch.where(((b >> low) & 1) == 0, below, above)
            assert torch.equal(case.expect.double()[tie], even[tie])


def test_expected_values_are_exact_in_every_dtype():
    """Section A: operands exact in both operand types, |y64| < 2^24 (fp32 holds every partial sum in any order), below 65504 for fp16;
    section B: EpiCase.check in float64 and float32; GELU pre-activations: multiples of 2^-10 below 8."""
    for M, N, K, op, out in dict.fromkeys((M, N, K, "", out) for M, N, K, op, out in SHAPE_CASES):
        case = FpCase(M, N, K, out, "cpu")
        assert float((case.a.double().abs() @ case.w.double().abs().T).max()) <= 4 * 255 * K < 2 ** 24  # every partial sum, any order
        assert torch.equal(case.y64.float().double(), case.y64)
        if out != "f32" and M * N >= TIE_ELEMS:
            assert not torch.equal(case.expect.double(), case.y64)
    for entry in ENTRIES:
        for out in OUTS:
            EpiCase(entry, out, "cpu")  # asserts in __init__
        g = GeluCase(entry, "cpu")
        assert torch.equal(g.pre.float().double(), g.pre)
    for K in (96, 160):
        assert probe_one_hot(ModelRun(), K, "bf16") == []


# ------------------------------------------------------------------------------------------------ the numpy model and its mutants
def to_bits(y, out, truncate=False):
    """float32 array -> the bit pattern of its one rounding into the output type (int64); truncate: toward zero."""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    if out == "f32":
        return t.view(torch.int32).numpy().astype(np.int64)
    if out == "bf16" and truncate:
        return (t.view(torch.int32) >> 16).to(torch.int16).numpy().astype(np.int64)
    h = t.to(TDT[out])
    bits = h.view(torch.int16)
    if truncate:  # sign-magnitude: one pattern back where nearest-even went away from zero
        bits = bits - (h.float().abs() > t.abs()).to(torch.int16)
    return bits.numpy().astype(np.int64)


def from_bits(bits, dt):
    t = torch.from_numpy(np.ascontiguousarray(bits)).to(torch.int32 if dt == "f32" else torch.int16)
    return t.view(TDT[dt]).float().numpy()


def fma32(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu_fast_model(y):
    """gelu_tanh_fast_f32 in numpy fp32 (exp2 and the reciprocal as numpy rounds them)."""
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        t = (y * fma32(y * y, np.full_like(y, f(-0.10294324)), np.full_like(y, f(-2.3022082)))).astype(f)
        return (y * (f(1) / (f(1) + np.exp2(t, dtype=f))).astype(f)).astype(f)


MUTANTS = ["half_ignored", "koff_never_shifted", "read_parity_dropped", "source_swizzle_dropped", "row_clamp_to_M", "channel_guard_removed",
           "bias_lane_shifted", "bf16_bias_as_f16", "truncation", "rounded_before_gate"]
PAD = 4 * TK  # poison behind a and w: what a read past the last row returns (NaN)


class ModelRun:
    """The kernel as written, in numpy, block by block:
      tile origin   tm = bid / nt, tn = bid - tm nt
      DMA           instruction q of wave v, lane l -> LDS row r = 8 (4 q + v) + (l >> 3) (weights: 128 rows further down), physical
                    chunk l & 7, from logical chunk c = (l & 7) ^ ((r >> 1) & 7) of token row min(m0 + r, M - 1) / weight row
                    min(n0 + r, N - 1) at k = koff + 8 c, koff = 64 t, or 64 t - 32 where 64 t + 8 c >= K; into buffer t & 1
      fragments     row R, step kk, quarter fq: physical chunk (4 kk + fq) ^ ((R >> 1) & 7) of buffer t & 1; the step's 32 k of token row
                    R against those of weight row R'; the second step is skipped when 64 t + 32 >= K
      epilogue      channel group n = n0 + 64 wn + 16 j + 4 fq (skipped when n >= N), row m = m0 + 64 wm + 16 i + fr (skipped when
                    m >= M); acc + bias (fma(acc, sw, bias); per group fma(part, sw_g, acc)), GELU, r + y gate, one rounding; stored
                    at m N + n.
    Values are float64 in LDS (NaN where nothing was copied) and fp32 in the epilogue.  Reads outside a or w are counted and return
    NaN; they are reported as a failure, as a bounds checker would."""
    dev = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def __call__(self, entry, op, out, a, w, sw=None, bias=None, bias_dt="f32", gate=None, res=None, inplace=False, gelu=False):
        mut, f = self.mutant, np.float32
        (M, K), N = a.shape, w.shape[0]
        a_flat = np.concatenate([a.double().numpy().ravel(), np.full(PAD, np.nan)])
        w_flat = np.concatenate([w.double().numpy().ravel(), np.full(PAD, np.nan)])
        win = Window(M, N, out, "cpu")
        flat = win.flat.numpy()
        mt, nt, nk = -(-M // TM), -(-N // TN), -(-K // TK)
        ncol = nt * TN + 8

        def vec(x, dt="f32", as_f16=False):  # a per-channel vector as the kernel reads it, NaN past N
            v = np.full(ncol, np.nan, dtype=f)
            if x is not None:
                t = x.to(TDT[dt])
                if as_f16:
                    t = t.view(torch.int16).view(torch.float16)
                v[:N] = t.float().numpy()
            return v

        b = vec(bias, bias_dt, mut == "bf16_bias_as_f16" and bias_dt == "bf16") if bias is not None else np.zeros(ncol, dtype=f)
        g = vec(gate)
        sws = None if sw is None else [vec(s) for s in (sw if sw.dim() == 2 else sw[None])]
        tpg = nk if sw is None or sw.dim() == 1 else GROUP // TK
        r_bits = None if gate is None else to_bits(res.float().numpy(), out)
        if gate is not None and inplace:
            flat[GUARD:GUARD + M * N] = r_bits.ravel()
        wave, q, lane = np.meshgrid(np.arange(4), np.arange(4), np.arange(64), indexing="ij")
        r = 8 * (4 * q + wave) + (lane >> 3)
        c = (lane & 7) if mut == "source_swizzle_dropped" else (lane & 7) ^ ((r >> 1) & 7)
        R = np.arange(128)
        swz = (R >> 1) & 7
        oob = 0
        for bid in range(mt * nt):
            tm = bid // nt
            tn = bid - tm * nt
            m0, n0 = tm * TM, tn * TN
            mrow = np.where(m0 + r < M, m0 + r, M if mut == "row_clamp_to_M" else M - 1)
            nrow = np.where(n0 + r < N, n0 + r, N - 1)
            lds = np.full((2, 256, 8, 8), np.nan)
            acc = np.zeros((128, 128), dtype=f)
            part = np.zeros((128, 128))
            for t in range(nk):
                koff = t * TK if mut == "koff_never_shifted" else np.where(t * TK + c * 8 < K, t * TK, t * TK - 32)
                for base, src, row, size in ((0, a_flat, mrow, M * K), (128, w_flat, nrow, N * K)):
                    idx = (row * K + c * 8 + koff)[..., None] + np.arange(8)
                    oob += int((idx >= size).sum())
                    lds[t & 1, base + r, lane & 7] = src[idx]
                buf = lds[0 if mut == "read_parity_dropped" else t & 1]
                half = t * TK + 32 >= K and mut != "half_ignored"
                with np.errstate(invalid="ignore", over="ignore"):
                    for kk in range(1 if half else 2):
                        p = (4 * kk + np.arange(4))[None, :] ^ swz[:, None]
                        x = buf[R[:, None], p].reshape(128, 32)
                        y = buf[128 + R[:, None], p].reshape(128, 32)
                        part = part + x @ y.T
                    if (t + 1) % tpg == 0:  # the end of a group (per-channel scales and the FP kernel: of K)
                        if sws is not None and len(sws) > 1:
                            acc = fma32(part.astype(f), np.broadcast_to(sws[t // tpg][n0:n0 + 128], part.shape), acc)
                            part = np.zeros((128, 128))
            with np.errstate(invalid="ignore", over="ignore"):
                if sws is None:
                    y = (part.astype(f) + b[n0:n0 + 128]).astype(f)
                elif len(sws) == 1:
                    y = fma32(part.astype(f), np.broadcast_to(sws[0][n0:n0 + 128], part.shape), np.broadcast_to(b[n0:n0 + 128], part.shape))
                else:
                    y = (acc + b[n0:n0 + 128]).astype(f)
                if mut == "bias_lane_shifted" and bias is not None:  # the bias of the next 4-channel group, clamped inside N
                    nb = np.minimum(n0 + R // 4 * 4 + 4, N - 4) + R % 4
                    y = (y - b[n0:n0 + 128] + b[nb]).astype(f)
                if gelu:
                    y = gelu_fast_model(y)
                live_m = R[m0 + R < M]
                live_n = R if mut == "channel_guard_removed" else R[n0 + R < N]
                o = GUARD + (m0 + live_m)[:, None] * N + (n0 + live_n)[None, :]
                y = y[np.ix_(live_m, live_n)]
                if gate is not None:
                    ro = np.minimum(o - GUARD, M * N - 1)
                    rr = from_bits(flat[np.minimum(o, len(flat) - 1)] if inplace else r_bits.ravel()[ro], out)
                    if mut == "rounded_before_gate" and out != "f32":
                        y = from_bits(to_bits(y, out), out)
                    y = (rr + (y * g[n0 + live_n][None, :]).astype(f)).astype(f)
                flat[o] = to_bits(y, out, truncate=mut == "truncation")
        fails = [f"model: {oob} elements read outside a or w"] if oob else []
        return Result(win, fails)


def model_battery(run):
    """The probes of A - C at the smallest shapes that tell the mutants apart; -> {probe name: failures}."""
    got = {}
    for K in (32, 96, 128):
        got[f"A exact (129, 136, {K}) bf16 -> bf16"] = probe_exact(run, 129, 136, K, "bf16", "bf16")
    got["A exact (1, 8, 96) f16 -> f16"] = probe_exact(run, 1, 8, 96, "f16", "f16")
    got["A exact (257, 264, 160) f16 -> f32"] = probe_exact(run, 257, 264, 160, "f16", "f32")
    got["A one-hot 96"] = probe_one_hot(run, 96, "bf16")
    got["A one-hot 160"] = probe_one_hot(run, 160, "f16")
    got["A encoded 32"] = probe_encoded(run, 32, "bf16")
    got["A encoded 192"] = probe_encoded(run, 192, "f16")
    got["B fp bias bf16, f16 operands -> f32"] = probe_epilogue(run, "fp", "f16", "f32", "bf16", "none")
    got["B fp bias f16, bf16 operands -> bf16 res"] = probe_epilogue(run, "fp", "bf16", "bf16", "f16", "res")
    got["B wq bias f32 -> f16 inplace"] = probe_epilogue(run, "wq", "f16", "f16", "f32", "inplace")
    got["B wqg no bias -> bf16 res"] = probe_epilogue(run, "wqg", "bf16", "bf16", None, "res")
    got["B gelu fp -> f32"] = probe_gelu(run, "fp", "bf16", "f32", "none")[0]
    got["B gelu wqg -> bf16 res"] = probe_gelu(run, "wqg", "f16", "bf16", "res")[0]
    got["C isolation bf16"] = probe_isolation(run, "bf16")
    return got


def test_model_passes_every_probe():
    got = model_battery(ModelRun())
    assert {k: v for k, v in got.items() if v} == {}
    run = ModelRun()
    for entry in ENTRIES:  # the full product of B on the model, one operand type
        for out in OUTS:
            case = EpiCase(entry, out, "cpu")
            for bias_dt in BIAS_KINDS:
                for epi in EPI_KINDS:
                    assert probe_epilogue(run, entry, "bf16", out, bias_dt, epi, case) == [], (entry, out, bias_dt, epi)


# what each mutant must fail at the least (a substring of the probe's name), and how: "guard" = a guard word was written,
# "bounds" = no output differs (the values read are computed, never stored, or never multiplied) and only the bounds check sees it
MUTANT_FAILS = {
    "half_ignored": ("A exact (129, 136, 32)", "A exact (129, 136, 96)", "A one-hot 96", "A one-hot 160", "A encoded 32", "B fp bias"),
    "koff_never_shifted": ("bounds",),
    "read_parity_dropped": ("A exact (129, 136, 96)", "A exact (129, 136, 128)", "A one-hot 96", "A encoded 192"),
    "source_swizzle_dropped": ("A exact (129, 136, 32)", "A one-hot 96", "A encoded 32", "C isolation"),
    "row_clamp_to_M": ("bounds",),
    "channel_guard_removed": ("guard",),
    "bias_lane_shifted": ("B fp bias bf16", "B fp bias f16", "B wq bias f32", "C isolation"),
    "bf16_bias_as_f16": ("B fp bias bf16, f16 operands",),
    "truncation": ("A exact (129, 136, 32)", "A exact (129, 136, 96)", "A exact (129, 136, 128)", "B fp bias f16, bf16 operands -> bf16 res",
                   "B wq bias f32 -> f16 inplace"),
    "rounded_before_gate": ("B fp bias f16, bf16 operands -> bf16 res", "B wq bias f32 -> f16 inplace", "B wqg no bias -> bf16 res"),
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_named_probes(mutant):
    got = {k: v for k, v in model_battery(ModelRun(mutant)).items() if v}
    print(f"MUTANT {mutant}: fails {sorted(got)}")
    assert got, mutant
    for want in MUTANT_FAILS[mutant]:
        if want == "guard":
            assert any("guard behind the output" in f for v in got.values() for f in v)
        elif want == "bounds":  # every failure is the bounds check's: no probe of the outputs can see this mutant
            assert all(len(v) >= 1 and all("read outside a or w" in f for f in v) for v in got.values()), got
        else:
            assert any(want in k for k in got), (mutant, want, sorted(got))
    if mutant == "bf16_bias_as_f16":  # only a bf16 bias is misread
        assert all("bias bf16" in k for k in got), sorted(got)
    if mutant == "rounded_before_gate":  # only 16-bit outputs with gate + residual
        assert all(("res" in k or "inplace" in k) for k in got), sorted(got)


def test_gelu_model_within_the_bound_and_a_wrong_gelu_is_not():
    """The fp32 model of the fast GELU stays within the derived bound on the pre-activations of every entry; the erf GELU, which
    differs from the tanh form by up to 4.7e-4 in the curved part, does not."""
    for entry in ENTRIES:
        case = GeluCase(entry, "cpu")
        x = case.pre
        got = torch.from_numpy(gelu_fast_model(x.numpy().astype(np.float32)).astype(np.float64))
        assert float(((got - gelu_ref(x)).abs() / gelu_bound(x)).max()) <= 1.0
        erf = 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
        ref, bound = case.reference("f32", "none")
        assert float(((erf - ref).abs() / bound).max()) > 100
