"""The weight-only GEMMs (csrc/gemm_wq16.hip: wanq_gemm_wq16 and wanq_gemm_wq16_grouped) on operands whose answer is known exactly:
what is theirs alone -- the weight codes read straight from global memory into MFMA fragments, the in-register decode, and the
double-buffered sw / zp group rows that travel by 4-byte LDS-DMA one group ahead.  (The epilogue they share with the FP kernel is
tests/test_gpu_gemm16_probes.py's.)  Every call goes through the C ABI and the test owns every buffer; the output is that file's
Window between guard zones, refilled with a quiet-NaN bit pattern before EVERY launch.

  A  slot map and code table: a = identity, so row k of the output is weight column k: fp32(c + zp) * sw, one rounding.  The code
     table puts every code value at every in-tile k position; zp cycles through the ends of its range (c + zp reaches +-255); sw is a
     distinct non-power-of-two per (group, channel).  A failure names (K-tile, kk, fq, byte / nibble) and (channel tile, wn, j, fr).
  B  the group schedule of the grouped entry: dense integer data over (K, g) with 1, 3 and 5 groups of 1, 2, 3 and 6 K-tiles; a
     one-hot group signature whose checker names the group whose row was wrong; no leakage between groups.
  C  twin relations: grouped with g = K is bit-equal to the per-channel entry; sw = 1 is bit-equal to wanq_gemm_bf16 on (c + zp).
  D  isolation: a NaN or 2^100 in one sw, one zp, one code channel or one token row stays in its column or row.
  E  M = 0 and one refused call per entry leave the window untouched.
  F  CPU self-tests (not marked gpu): a numpy model of both kernels as written passes every checker of A - E; single-error mutants
     of it fail named probes (profiles/wq16_probe_mutants.txt); the census of the code table and the exactness of every expectation.

Every probe is a function of a `run` callable: run(entry, op, bits, a, codes, sw, zp, g, out) -> Result, and run.fp(op, out, a, w)
for wanq_gemm_bf16.  `codes` are the bytes as the kernel reads them: int8 [N, K] (W8) or the packed nibbles [N, K / 2] (W4) of
pack_w4_np, a packer written here from the documented layout (include/wanq_hip.h), not the library's.
Conventions (include/wanq_hip.h): W8 c in [-128, 127], zp in [-127, 128]; W4 nibbles u in 0..15, zp = zero_point - 8 in [-8, 7]."""
import os

import numpy as np
import pytest
import torch

from test_gpu_gemm16_probes import DEV, DTC, GUARD, OPS, SENT_BITS, TDT, TK, TM, TN, WANQ_E_SHAPE, WANQ_OK  # noqa: F401
from test_gpu_gemm16_probes import GpuRun as FpGpuRun
from test_gpu_gemm16_probes import ModelRun as FpModelRun
from test_gpu_gemm16_probes import Result, Window, check_exact, exact_in, fma32, guard_failures, ints, pow2, to_bits

gpu = pytest.mark.gpu
BITS = (8, 4)
CODE_RANGE = {8: (-128, 127), 4: (0, 15)}
ZP_RANGE = {8: (-127, 128), 4: (-8, 7)}
NAN = float("nan")


# ================================================================================================ operands
def pack_w4_np(u):
    """uint8 [N, K] nibbles 0..15 -> [N, K / 2] bytes: 16-byte groups of 32 codes; dword fq (bytes 4 fq .. 4 fq + 3) holds codes
    8 fq + i in the low nibble of its byte i and codes 8 fq + 4 + i in the high nibble (i = 0..3)."""
    N, K = u.shape
    assert K % 32 == 0 and u.dtype == np.uint8 and int(u.max(initial=0)) <= 15
    v = u.reshape(N, K // 32, 4, 2, 4)  # group, fq, low / high, i
    return (v[:, :, :, 0, :] | (v[:, :, :, 1, :] << 4)).reshape(N, K // 2)


def raw_codes(cval, bits):
    """int64 code values [N, K] -> the bytes the kernel reads."""
    lo, hi = CODE_RANGE[bits]
    assert int(cval.min()) >= lo and int(cval.max()) <= hi
    if bits == 8:
        return cval.to(torch.int8).contiguous()
    return torch.from_numpy(pack_w4_np(cval.cpu().numpy().astype(np.uint8))).to(cval.device)


def wint_of(cval, zp, K):
    """c + zp float64 [N, K]; zp None, [N] or [G, N]."""
    w = cval.double()
    if zp is None:
        return w
    if zp.dim() == 1:
        return w + zp.double()[:, None]
    return w + zp.double().T.repeat_interleave(K // zp.shape[0], dim=1)


def contract(a, wint, sw, t=torch.float64):
    """The header's contract in type t, each step rounded to t: acc = fma(part_g, sw[g], acc), g ascending from 0 (one group: the
    per-channel entry's acc * sw)."""
    sw2 = sw[None] if sw.dim() == 1 else sw
    G, K = sw2.shape[0], a.shape[1]
    gs = K // G
    y = torch.zeros(a.shape[0], wint.shape[0], dtype=t, device=a.device)
    for g in range(G):
        k = slice(g * gs, (g + 1) * gs)
        y = (a.double()[:, k] @ wint[:, k].T).to(t) * sw2[g].to(t)[None, :] + y
    return y


def same(x, y):
    return bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())


def assert_exact(a, wint, sw, unit):
    """From the inputs: every term is a multiple of `unit` and the sum of absolute terms stays below 2^24 units, so every fp32
    intermediate is exact in any order; the fp32 evaluation equals the float64 one."""
    sw2 = sw[None] if sw.dim() == 1 else sw
    S = contract(a.abs(), wint.abs(), sw2.abs())
    y = contract(a, wint, sw2)
    assert float(S.max()) / unit < 2.0 ** 24, float(S.max()) / unit
    assert torch.equal(y / unit, torch.round(y / unit)) and torch.equal(contract(a, wint, sw2, torch.float32).double(), y)
    assert exact_in(a, "bf16", "f16") and exact_in(sw2, "f32") and float(wint.abs().max()) <= 255
    return y


def hash_codes(N, K, bits, salt, dev):
    return ints(N, K, salt, *CODE_RANGE[bits], dev)


# ================================================================================================ the GPU runner
class GpuRun:
    """One launch through the C ABI into a fresh sentinel-filled window.  a [M, K] float64 of values exact in the operand type;
    codes as raw_codes gives them; sw, zp [N] or [G, N] (any float type, passed as fp32); g the group size of the grouped entry."""
    dev = DEV

    def __call__(self, entry, op, bits, a, codes, sw, zp=None, g=None, out="f32"):
        from viditq_extension import _C

        (M, K), N = a.shape, codes.shape[0]
        assert codes.shape[1] == (K if bits == 8 else K // 2) and codes.dtype == (torch.int8 if bits == 8 else torch.uint8)
        a16, ck, s = a.to(TDT[op]).contiguous(), codes.contiguous(), sw.float().contiguous()
        z = None if zp is None else zp.float().contiguous()
        win = Window(M, N, out, DEV)
        tail = (win.ptr(), DTC[out], None, DTC["f32"], None, None, 0, M, N, K, _C.stream())
        if entry == "wq":
            assert s.shape == (N,) and g is None
            rc = _C.lib.wanq_gemm_wq16(_C.ptr(a16), _C.ptr(ck), DTC[op], bits, _C.ptr(s), _C.ptr(z), *tail)
        else:
            assert entry == "wqg" and s.shape == (K // g, N)
            rc = _C.lib.wanq_gemm_wq16_grouped(_C.ptr(a16), _C.ptr(ck), DTC[op], bits, _C.ptr(s), _C.ptr(z), g, *tail)
        torch.cuda.synchronize()
        assert rc == WANQ_OK, (rc, _C.lib.wanq_last_error().decode())
        return Result(win, [])

    def fp(self, op, out, a, w):
        return FpGpuRun()("fp", op, out, a, w)


# ================================================================================================ A. slot map and code table
A_K, A_N = 192, 264
A_FORMS = (("wq", None), ("wqg", 64), ("wqg", A_K))
ZP_CYCLE = {8: (-127, -1, 0, 1, 128), 4: (-8, 0, 7)}


def odd_scales(G, N, dev):
    """A distinct non-power-of-two fp32 per (group, channel), about 0.37 .. 0.56."""
    i = torch.arange(G * N, dtype=torch.float64, device=dev).view(G, N)
    return ((1.0 + (2 * i + 1) / 4096.0) * 0.37).float().double()


def table_case(bits, g, zp_null, dev, N=A_N, K=A_K, skew=False):
    """-> (code values, sw, zp): c[n, k] = (n + 37 k) % 256 - 128 (W8) or (n + 5 k) % 16 (W4); zp cycles per channel and group;
    g None: the per-channel entry's vectors.  The W4 table has period 16 in k: columns k and k + 16 are the same, so it cannot tell a
    kk, an fq + 2 or a K-tile mix-up.  `skew` adds (n / 16) (k / 16), another multiple of k / 16 in every 16-channel block, which
    keeps every code at every in-tile k and makes the columns pairwise distinct (block 1 tells k / 16 apart, block 0 k % 16)."""
    n, k = torch.arange(N, dtype=torch.int64, device=dev), torch.arange(K, dtype=torch.int64, device=dev)
    cval = (n[:, None] + 37 * k[None, :]) % 256 - 128 if bits == 8 else (n[:, None] + 5 * k[None, :]) % 16
    if skew:
        assert bits == 4
        cval = (cval + (n[:, None] // 16) * (k[None, :] // 16)) % 16
    G = 1 if g is None else K // g
    cyc = torch.tensor(ZP_CYCLE[bits], dtype=torch.float64, device=dev)
    gi = torch.arange(G, dtype=torch.int64, device=dev)
    zp = cyc[(n[None, :] + (2 if bits == 8 else 1) * gi[:, None]) % len(cyc)]
    sw = odd_scales(G, N, dev)
    if g is None:
        sw, zp = sw[0], zp[0]
    return cval, sw, None if zp_null else zp


def slot_name(k, n, bits):
    e = k % 8
    where = f"byte {e} of the 8-byte load" if bits == 8 else f"{'low' if e < 4 else 'high'} nibble of byte {e % 4} of the 4-byte load"
    return (f"k = {k}: K-tile {k // TK}, kk {k % TK // 32}, fq {k % 32 // 8}, {where}; channel {n}: tile {n // TN}, wn {n % TN // 64}, "
            f"j {n % 64 // 16}, fr {n % 16}")


def probe_table(run, entry, g, bits, op, zp_null, skew=False):
    """a = I: out[k, n] = fp32(c[n, k] + zp) * sw, the one rounding of an exact product of two fp32."""
    dev = run.dev
    cval, sw, zp = table_case(bits, g, zp_null, dev, skew=skew)
    wint = wint_of(cval, zp, A_K)
    assert float(wint.abs().max()) <= 255 and exact_in(sw, "f32")
    a = torch.eye(A_K, dtype=torch.float64, device=dev)
    sw2 = sw[None] if sw.dim() == 1 else sw
    gs = A_K // sw2.shape[0]
    expect = (wint.T * sw2.repeat_interleave(gs, dim=0)).float()  # both factors fp32: the product is exact in float64, rounded once

    def describe(m, n, got):
        ks = ((wint[n] * sw2.repeat_interleave(gs, dim=0)[:, n]).float() == got).nonzero().flatten().tolist()
        return slot_name(m, n, bits) + f"; the value is that of k in {ks[:4]}"

    return check_exact(run(entry, op, bits, a, raw_codes(cval, bits), sw, zp, g), expect, describe)


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("entry,g", A_FORMS)
def test_identity_rows_return_every_slot_of_the_code_table(entry, g, bits, op):
    fails = []
    for zp_null in (False, True):
        for skew in (False, True)[:2 if bits == 4 else 1]:
            fails += [f"zp {'NULL' if zp_null else 'present'}{' skewed table' if skew else ''}: {f}"
                      for f in probe_table(GpuRun(), entry, g, bits, op, zp_null, skew)]
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("bias", [0, 8])
def test_numpy_packer_equals_wanq_pack_w4(bias):
    from viditq_extension import _C

    N, K = 24, 192
    u = ints(N, K, 5, 0, 15, DEV)
    q = (u - bias).to(torch.int8).contiguous()
    packed = torch.full((N, K // 2), 0xA5, dtype=torch.uint8, device=DEV)
    assert _C.lib.wanq_pack_w4(_C.ptr(q), _C.ptr(packed), bias, N, K, _C.stream()) == WANQ_OK
    torch.cuda.synchronize()
    assert torch.equal(packed.cpu(), torch.from_numpy(pack_w4_np(u.cpu().numpy().astype(np.uint8))))


# ================================================================================================ B. the group schedule
B_SHAPES = ((64, 64), (192, 64), (320, 64), (384, 128), (640, 128), (576, 192), (384, 384))
B_MS, B_NS = (1, 129, 257), (8, 136, 264)


def dense_case(M, N, K, g, bits, zp_null, dev):
    """|a| <= 2, hashed codes and zero points over their whole ranges, sw in 2^-3 .. 2^3: multiples of 2^-3."""
    G = K // g
    a, cval = ints(M, K, 61, -2, 2, dev).double(), hash_codes(N, K, bits, 62, dev)
    zp = None if zp_null else ints(G, N, 63, *ZP_RANGE[bits], dev).double()
    sw = pow2(ints(G, N, 64, -3, 3, dev))
    return a, cval, sw, zp


def probe_dense(run, M, N, K, g, bits, op, zp_null):
    a, cval, sw, zp = dense_case(M, N, K, g, bits, zp_null, run.dev)
    y = assert_exact(a, wint_of(cval, zp, K), sw, 2.0 ** -3)
    return check_exact(run("wqg", op, bits, a, raw_codes(cval, bits), sw, zp, g), y.float())


def signature_case(M, N, K, g, bits, zp_null, dev):
    """Row m is one-hot in every group, at k = g gi + (29 m + 13 gi + 7 (m / g)) % g.  sw[gi, n] = 2 ((n % 128) + 128 gi) + 1, an odd
    integer that differs between any two groups and any two channels of a workgroup's 128; zp differs between any two groups (up
    to 5) and any two channels of a 16-channel block; c + zp is never 0 (a code that would give 0 is moved by one)."""
    G = K // g
    m, n, gi = [torch.arange(x, dtype=torch.int64, device=dev) for x in (M, N, G)]
    kabs = gi[None, :] * g + (29 * m[:, None] + 13 * gi[None, :] + 7 * (m[:, None] // g)) % g  # [M, G]
    a = torch.zeros(M, K, dtype=torch.float64, device=dev)
    a[m[:, None].expand(M, G), kabs] = 1.0
    sw = (2 * ((n[None, :] % 128) + 128 * gi[:, None]) + 1).double()
    zp = ((11 * n[None, :] + 53 * gi[:, None]) % 256 - 127 if bits == 8 else (n[None, :] + 3 * gi[:, None]) % 16 - 8).double()
    zp = None if zp_null else zp
    cval = hash_codes(N, K, bits, 65, dev)
    step = torch.where(cval < CODE_RANGE[bits][1], 1, -1)
    cval = torch.where(wint_of(cval, zp, K) == 0, cval + step, cval)
    return a, kabs, cval, sw, zp


def probe_signature(run, M, N, K, g, bits, op, zp_null):
    dev = run.dev
    a, kabs, cval, sw, zp = signature_case(M, N, K, g, bits, zp_null, dev)
    G, wint = K // g, wint_of(cval, zp, K)
    assert bool((wint != 0).all())
    y = assert_exact(a, wint, sw, 1.0)

    def describe(m, n, got):
        """Which wrong row explains the value: first one group's term made with another group's row (or missing), then one rule
        applied to every group (the row of a neighbouring group, no refresh after group 1, the other lane map's channel)."""
        c = [float(cval[n, kabs[m, i]]) for i in range(G)]
        z = [[0.0 if zp is None else float(zp[h, x]) for x in range(N)] for h in range(G)]
        s = [[float(sw[h, x]) for x in range(N)] for h in range(G)]
        term = [(c[i] + z[i][n]) * s[i][n] for i in range(G)]
        blk = n // 16 * 16
        for i in range(G):
            r = got - (float(y[m, n]) - term[i])
            if r == 0.0:
                return f"group {i}: its term is missing (k = {int(kabs[m, i])})"
            if r == c[i] * s[i][n] and zp is not None:
                return f"group {i}: its zero point was not applied"
            for h in range(G):
                if h != i and r == (c[i] + z[i][n]) * s[h][n]:
                    return f"group {i}: folded with the scale row of group {h}"
                if h != i and r == (c[i] + z[h][n]) * s[i][n]:
                    return f"group {i}: decoded with the zero-point row of group {h}"
                if h != i and r == (c[i] + z[h][n]) * s[h][n]:
                    return f"group {i}: both rows are those of group {h}"
        rules = {"the next group's (the last group: the one before)": lambda i: i + 1 if i + 1 < G else max(i - 1, 0),
                 "the one of the group before": lambda i: max(i - 1, 0), "the one of group min(g, 1): no refresh after group 1": lambda i: min(i, 1),
                 "group 0's": lambda i: 0}
        for text, h in rules.items():
            wrong = [i for i in range(G) if h(i) != i]
            if wrong and got == sum((c[i] + z[i][n]) * s[h(i)][n] for i in range(G)):
                return f"group {wrong[0]} (and {wrong[1:]}): folded with another scale row: {text}"
            if wrong and got == sum((c[i] + z[h(i)][n]) * s[i][n] for i in range(G)):
                return f"group {wrong[0]} (and {wrong[1:]}): decoded with another zero-point row: {text}"
            if wrong and got == sum((c[i] + z[h(i)][n]) * s[h(i)][n] for i in range(G)):
                return f"group {wrong[0]} (and {wrong[1:]}): both rows are another group's: {text}"
        zch = [blk + 4 * (int(kabs[m, i]) % 32 // 8) for i in range(G)]
        if max(zch) < N and got == sum((c[i] + z[i][zch[i]]) * s[i][n] for i in range(G)):
            return f"every group: decoded with the zero point of channel 16 j + 4 fq (sw's lane map), here {zch}, not {n}"
        sch = blk + m % 16 + n % 4
        if sch < N and got == sum((c[i] + z[i][n]) * s[i][sch] for i in range(G)):
            return f"every group: folded with the scale of channel 16 j + fr + e (zp's lane map), here {sch}, not {n}"
        return f"no single wrong row explains it; the groups' terms are {term}"

    return check_exact(run("wqg", op, bits, a, raw_codes(cval, bits), sw, zp, g), y.float(), describe)


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("K,g", B_SHAPES)
def test_group_schedule_dense_and_signature(K, g, bits, op):
    """ng = 1, 3, 5, 3, 5, 3, 1 groups of tpg = 1, 1, 1, 2, 2, 3, 6 K-tiles: the first reuse of a row buffer (ng >= 3), the tightest
    schedule (tpg = 1), zp present and NULL, M in {1, 129, 257}, N in {8, 136, 264}."""
    run, fails = GpuRun(), []
    for zp_null in (False, True):
        for M in B_MS:
            for N in B_NS:
                tag = f"({M}, {N}, {K}) g={g} zp {'NULL' if zp_null else 'present'}"
                fails += [f"dense {tag}: {f}" for f in probe_dense(run, M, N, K, g, bits, op, zp_null)]
                fails += [f"signature {tag}: {f}" for f in probe_signature(run, M, N, K, g, bits, op, zp_null)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


LEAK_K, LEAK_G, LEAK_M, LEAK_N = 320, 64, 129, 136


def probe_no_leak(run, gstar, bits, op):
    """ng = 5, tpg = 1: activations nonzero in group gstar only; every other group's sw is 2^10, so a product that reaches another
    group's fold, or another group's scale that reaches this one's, is off by a factor of at least 2^7."""
    dev, K, g = run.dev, LEAK_K, LEAK_G
    a, cval, sw, zp = dense_case(LEAK_M, LEAK_N, K, g, bits, False, dev)
    live = (torch.arange(K, device=dev) // g) == gstar
    a = a * live.double()[None, :]
    sw = torch.where((torch.arange(K // g, device=dev) == gstar)[:, None], sw, torch.full_like(sw, 1024.0))
    y = assert_exact(a, wint_of(cval, zp, K), sw, 2.0 ** -3)
    assert float(y.abs().max()) <= 2 * 255 * 64 * 8
    return check_exact(run("wqg", op, bits, a, raw_codes(cval, bits), sw, zp, g), y.float())


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits", BITS)
def test_no_group_leaks_into_another(bits, op):
    fails = [f"group {gs}: {f}" for gs in range(LEAK_K // LEAK_G) for f in probe_no_leak(GpuRun(), gs, bits, op)]
    assert not fails, "\n".join(fails)


# ================================================================================================ C. twin relations
TWIN_M = 129


def bits_differ(r1, r2, what):
    fails = [f"{what}: {f}" for r in (r1, r2) for f in list(r.fails) + guard_failures(r.win)]
    d = r1.win.bits() != r2.win.bits()
    if bool(d.any()):
        r, c = [int(v) for v in d.nonzero()[0]]
        fails.append(f"{what}: {int(d.sum())} elements differ; first at row {r} col {c}: {r1.win.window()[r, c].item()} against "
                     f"{r2.win.window()[r, c].item()}")
    if bool((r1.win.bits() == SENT_BITS[r1.win.out]).any()):
        fails.append(f"{what}: elements never written")
    return fails


def probe_twins(run, bits, op, N):
    """At the code table of A (c + zp reaches +-255), K = 192, activations i 2^-e (|i| <= 7, e in 0..8: exact in both operand types,
    inexact sums in fp32, so the summation order shows): the grouped entry with g = K against the per-channel entry, and the
    per-channel entry with sw = 1 against wanq_gemm_bf16 on (c + zp) cast to the operand type."""
    dev, K = run.dev, A_K
    cval, sw, zp = table_case(bits, None, False, dev, N=N)
    a = ints(TWIN_M, K, 71, -7, 7, dev).double() * pow2(-ints(TWIN_M, K, 72, 0, 8, dev))
    wint = wint_of(cval, zp, K)
    assert exact_in(a, "bf16", "f16") and exact_in(wint, "bf16", "f16")
    codes, one, fails = raw_codes(cval, bits), torch.ones_like(sw), []
    for out in ("f32", op):
        fails += bits_differ(run("wq", op, bits, a, codes, sw, zp, None, out), run("wqg", op, bits, a, codes, sw[None], zp[None], K, out),
                             f"g = K against per channel -> {out}")
        fails += bits_differ(run("wq", op, bits, a, codes, one, zp, None, out), run.fp(op, out, a, wint), f"sw = 1 against wanq_gemm_bf16 -> {out}")
    return fails


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N", [A_N, 8])
def test_twin_relations_at_the_code_table(N, bits, op):
    fails = probe_twins(GpuRun(), bits, op, N)
    assert not fails, "\n".join(fails)


# ================================================================================================ D. isolation
ISO_M, ISO_N, ISO_K, ISO_G = 130, 136, 192, 64
BIG_A = {"bf16": 2.0 ** 100, "f16": 32768.0}


def isolation_cases(entry, bits, op, sw, zp, cval, a, quick=False):
    """(name, a, cval, sw, zp, poisoned row or -1, poisoned column or -1), one poison each."""
    G = ISO_K // ISO_G if entry == "wqg" else 1
    cases = []
    for ns in (0, ISO_N - 1):
        for gs in range(G):
            if quick and gs != (1 if ns == 0 else G - 1) % G:
                continue
            at = (gs, ns) if entry == "wqg" else ns
            for val, name in ((NAN, "NaN"), (2.0 ** 100, "2^100")):
                s2 = sw.clone()
                s2[at] = val
                cases.append((f"sw[{at}] = {name}", a, cval, s2, zp, -1, ns))
                if name == "NaN" or op == "bf16":  # 2^100 is no fp16 operand
                    z2 = zp.clone()
                    z2[at] = val
                    cases.append((f"zp[{at}] = {name}", a, cval, sw, z2, -1, ns))
        c2 = cval.clone()
        c2[ns, :] = CODE_RANGE[bits][0] if bits == 8 else CODE_RANGE[bits][1]
        cases.append((f"every code of channel {ns} = {int(c2[ns, 0])}", a, c2, sw, zp, -1, ns))
    for ms in (0, 127, ISO_M - 1):
        for val, name in ((NAN, "NaN"), (BIG_A[op], f"{BIG_A[op]:g}")):
            if quick and (ms == 127) == (name == "NaN"):
                continue
            a2 = a.clone()
            a2[ms, :] = val
            cases.append((f"token row {ms} = {name}", a2, cval, sw, zp, ms, -1))
    return cases


def probe_isolation(run, entry, bits, op, quick=False):
    """A clean exact run, then one poison at a time: outside the poisoned column / row every element is bit-equal to the clean run;
    inside, the float64 contract decides (NaN where it says NaN).  The poisoned values keep the contract's evaluation exact: a huge
    term is a multiple of 2^97 with a small integer coefficient, and next to it every finite term is below half a unit in fp32 and
    in float64 alike (asserted: the fp32 evaluation equals the float64 one)."""
    dev, M, N, K = run.dev, ISO_M, ISO_N, ISO_K
    grouped = entry == "wqg"
    a, cval, sw, zp = dense_case(M, N, K, ISO_G if grouped else K, bits, False, dev)
    if not grouped:
        sw, zp = sw[0].clone(), zp[0].clone()
    g = ISO_G if grouped else None

    def launch(a, cval, sw, zp):
        return run(entry, op, bits, a, raw_codes(cval, bits), sw, zp, g)

    clean = launch(a, cval, sw, zp)
    fails = [f"clean: {f}" for f in check_exact(clean, assert_exact(a, wint_of(cval, zp, K), sw, 2.0 ** -3).float())]
    rows, cols = torch.arange(M, device=dev), torch.arange(N, device=dev)
    for name, a2, c2, s2, z2, row, col in isolation_cases(entry, bits, op, sw, zp, cval, a, quick):
        res = launch(a2, c2, s2, z2)
        fails += [f"{name}: {f}" for f in list(res.fails) + guard_failures(res.win)]
        keep = (rows != row)[:, None] & (cols != col)[None, :]
        moved = (res.win.bits() != clean.win.bits()) & keep
        if bool(moved.any()):
            r, c = [int(v) for v in moved.nonzero()[0]]
            fails.append(f"{name}: {int(moved.sum())} elements outside row {row} / column {col} changed; first at row {r} col {c}: "
                         f"{res.win.window()[r, c].item()} was {clean.win.window()[r, c].item()}")
        w2 = wint_of(c2, z2, K)
        y64, y32 = contract(a2, w2, s2), contract(a2, w2, s2, torch.float32)
        assert same(y32.double(), y64), name
        got = res.win.window().double()
        bad = ~((got == y64) | (torch.isnan(got) & torch.isnan(y64))) & ~keep
        if bool(bad.any()):
            r, c = [int(v) for v in bad.nonzero()[0]]
            fails.append(f"{name}: {int(bad.sum())} elements inside row {row} / column {col} differ from the contract; first at row {r} "
                         f"col {c}: got {got[r, c].item()} expected {y64[r, c].item()}")
    return fails


@gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("entry", ["wq", "wqg"])
def test_a_poisoned_scale_zero_point_channel_or_row_stays_in_place(entry, bits, op):
    fails = probe_isolation(GpuRun(), entry, bits, op)
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ E. M = 0 and one refusal each
def _edge_call(entry, M, K, g):
    from viditq_extension import _C

    N = 16
    a = torch.zeros(8, 192, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, 192, dtype=torch.int8, device=DEV)
    sw = torch.ones(3, N, dtype=torch.float32, device=DEV)
    win = Window(8, N, "bf16", DEV)
    tail = (win.ptr(), DTC["bf16"], None, DTC["f32"], None, None, 0, M, N, K, _C.stream())
    if entry == "wq":
        rc = _C.lib.wanq_gemm_wq16(_C.ptr(a), _C.ptr(w), DTC["bf16"], 8, _C.ptr(sw), None, *tail)
    else:
        rc = _C.lib.wanq_gemm_wq16_grouped(_C.ptr(a), _C.ptr(w), DTC["bf16"], 8, _C.ptr(sw), None, g, *tail)
    torch.cuda.synchronize()
    return rc, bool((win.flat == SENT_BITS["bf16"]).all()), _C.lib.wanq_last_error().decode()


@gpu
@pytest.mark.parametrize("entry", ["wq", "wqg"])
def test_no_rows_is_ok_and_writes_nothing(entry):
    assert _edge_call(entry, 0, 192, 64)[:2] == (WANQ_OK, True)


@gpu
def test_a_refused_call_writes_nothing():
    rc, clean, msg = _edge_call("wq", 5, 96, None)
    assert (rc, clean) == (WANQ_E_SHAPE, True) and "multiple of 64" in msg
    rc, clean, msg = _edge_call("wqg", 5, 192, 128)
    assert (rc, clean) == (WANQ_E_SHAPE, True) and "group_size=128" in msg


# ================================================================================================ F. CPU self-tests of the probes
def test_code_table_census():
    """The inputs of A: every code value at every in-tile k position; c + zp reaches both ends of the exactness claim on every entry
    form (and at N = 8, family C's width); the columns of wint pairwise distinct; every scale a distinct non-power-of-two."""
    for bits in BITS:
        lo, hi = CODE_RANGE[bits]
        for entry, g in A_FORMS:
            cval, sw, zp = table_case(bits, g, False, "cpu")
            seen = {(int(k) % TK, int(c)) for k in range(A_K) for c in cval[:, k].unique()}
            assert seen == {(k, c) for k in range(TK) for c in range(lo, hi + 1)}
            wint = wint_of(cval, zp, A_K)
            assert float(wint.max()) == hi + ZP_RANGE[bits][1] and float(wint.min()) == lo + ZP_RANGE[bits][0]
            assert (float(wint.max()), float(wint.min())) == ((255.0, -255.0) if bits == 8 else (22.0, -8.0))
            for z in (zp, None):
                w = wint_of(table_case(bits, g, False, "cpu", skew=bits == 4)[0], z, A_K)
                assert len({tuple(c.tolist()) for c in w.T}) == A_K
            if bits == 4:  # the plain W4 table repeats every 16 k; the skewed one holds every code at every in-tile k as well
                assert torch.equal(cval[:, :-16], cval[:, 16:])
                skewed = table_case(bits, g, False, "cpu", skew=True)[0]
                assert {(int(k) % TK, int(c)) for k in range(A_K) for c in skewed[:, k].unique()} == seen
                ws = wint_of(skewed, zp, A_K)
                assert (float(ws.max()), float(ws.min())) == (22.0, -8.0)
            s = sw.flatten().float()
            assert len(s.unique()) == s.numel() and bool(((s.view(torch.int32) & 0x7FFFFF) != 0).all())
            assert set(zp.unique().tolist()) == {float(v) for v in ZP_CYCLE[bits]}
        cval, sw, zp = table_case(bits, None, False, "cpu", N=8)
        wint = wint_of(cval, zp, A_K)
        assert (float(wint.max()), float(wint.min())) == ((255.0, -255.0) if bits == 8 else (22.0, -8.0))
    # each end of the code range in every byte / nibble position of a load, in both 32-deep steps of a tile
    for bits in BITS:
        cval = table_case(bits, None, False, "cpu")[0]
        for c in CODE_RANGE[bits]:
            assert {int(k) % TK for k in (cval == c).nonzero()[:, 1]} == set(range(TK))


def test_packer_layout_is_the_documented_one():
    """include/wanq_hip.h: per 16-code half e, P0 byte i = u[i] | u[4 + i] << 4, P1 byte i = u[8 + i] | u[12 + i] << 4; a 16-byte group is
    (P0a, P1a, P0b, P1b).  The kernel comment: dword fq's low nibbles are codes 8 fq .. + 3, its high nibbles 8 fq + 4 .. + 7."""
    u = (np.arange(2 * 64, dtype=np.int64).reshape(2, 64) * 7 % 16).astype(np.uint8)
    p = pack_w4_np(u)
    for row in range(2):
        for grp in range(2):
            for half in range(2):
                e = u[row, 32 * grp + 16 * half:][:16].astype(int)
                for i in range(4):
                    assert p[row, 16 * grp + 8 * half + i] == e[i] | e[4 + i] << 4
                    assert p[row, 16 * grp + 8 * half + 4 + i] == e[8 + i] | e[12 + i] << 4
    with pytest.raises(AssertionError):
        pack_w4_np(np.full((1, 32), 16, dtype=np.uint8))


def test_gpu_part_is_marked():
    import inspect
    import sys

    first_cpu = inspect.getsourcelines(test_code_table_census)[1]
    for name, fn in list(vars(sys.modules[__name__]).items()):
        if name.startswith("test_") and inspect.isfunction(fn) and inspect.getsourcelines(fn)[1] < first_cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name


def test_signature_tells_every_row_and_lane_map_apart():
    """The group signature's inputs: with another group's scale or zero point, or the channel the other lane map would give, a
    term changes -- so the value changes, the other terms being the same."""
    for bits in BITS:
        for K, g in ((320, 64), (640, 128), (576, 192)):
            a, kabs, cval, sw, zp = signature_case(33, 136, K, g, bits, False, "cpu")
            G = K // g
            assert torch.equal(a.sum(1), torch.full((33,), float(G), dtype=torch.float64)) and int(kabs.min()) >= 0
            assert all(bool((a[:, i * g:(i + 1) * g].sum(1) == 1).all()) for i in range(G))
            assert bool((wint_of(cval, zp, K) != 0).all()) and bool((sw % 2 == 1).all())
            for t in (sw, zp):
                for i in range(G):
                    for h in range(i):
                        assert bool((t[i] != t[h]).all())
                blocks = t[:, :128].reshape(G, 8, 16)
                assert all(len(b.unique()) == 16 for row in blocks for b in row)
        assert len({int(k) % TK for k in signature_case(257, 8, 64, 64, bits, False, "cpu")[1].flatten()}) == TK


def test_expected_values_are_exact():
    """Every dense, signature and no-leak case of B at its largest size, and D's clean case: asserted from the inputs by the probes'
    own assert_exact (run here on the CPU for every (K, g), both widths, zp present and NULL)."""
    for bits in BITS:
        for K, g in B_SHAPES:
            for zp_null in (False, True):
                a, cval, sw, zp = dense_case(257, 264, K, g, bits, zp_null, "cpu")
                assert_exact(a, wint_of(cval, zp, K), sw, 2.0 ** -3)
                a, _, cval, sw, zp = signature_case(257, 264, K, g, bits, zp_null, "cpu")
                assert_exact(a, wint_of(cval, zp, K), sw, 1.0)
        a, cval, sw, zp = dense_case(ISO_M, ISO_N, ISO_K, ISO_G, bits, False, "cpu")
        assert_exact(a, wint_of(cval, zp, ISO_K), sw, 2.0 ** -3)
    assert {(K // g, g // TK) for K, g in B_SHAPES} == {(1, 1), (3, 1), (5, 1), (3, 2), (5, 2), (3, 3), (1, 6)}
    assert all(M <= 300 and N <= 264 and K <= 640 for M in B_MS for N in B_NS for K, _ in B_SHAPES)


# ------------------------------------------------------------------------------------------------ the numpy model and its mutants
MUTANTS = ["nibbles_swapped", "fq_stride_wrong", "kk_offset_wrong", "w4_decoded_with_128", "w8_decoded_without_128", "xor_dropped",
           "zp_through_sw_lane_map", "sw_through_zp_lane_map", "sw_row_from_other_buffer", "zp_refresh_skipped_from_group_2",
           "group_row_over_live_buffer", "group_row_stride_dropped", "fold_one_tile_early", "fold_one_tile_late", "last_group_not_folded",
           "part_not_zeroed", "token_parity_swapped", "clamp_n_to_N", "clamp_m_to_0"]
PAD = 4 * TK


def cut16(f, op):
    """pack2: fp32 -> the 16-bit operand.  bf16: the high half (v_perm_b32); fp16: round toward zero (v_cvt_pkrtz_f16_f32)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if op == "bf16":
        return (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        h = f.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(f)
    return (h.view(np.uint16) - over.astype(np.uint16)).view(np.float16).astype(np.float64)


class ModelRun:
    """Both kernels of csrc/gemm_wq16.hip as written, in numpy, block by block:
      tile origin   tm = bid / nt, tn = bid - tm nt
      tokens        token_dma_sources: instruction q of wave v, lane l -> LDS row r = 8 (4 q + v) + (l >> 3), physical chunk l & 7, from
                    logical chunk (l & 7) ^ ((r >> 1) & 7) of token row min(m0 + r, M - 1) at k = 64 t, into buffer t & 1; frag_addr:
                    row R, step kk, quarter fq reads physical chunk (4 kk + fq) ^ ((R >> 1) & 7) of buffer t & 1
      codes         lane (fr, fq), channel block j of wave column wn: channel min(n0 + 64 wn + 16 j + fr, N - 1); the 8 bytes (W8) or
                    4 bytes (W4) at  n rowbytes + fq CT / 8 + t CT + kk CT / 2,  CT = 64 (W8) or 32 (W4) bytes per row and K-tile
      decode        W8: u = byte ^ 0x80, W4: low nibbles are codes 0..3 of the 8, high nibbles 4..7; fp32(u) + zadj with
                    zadj = zp - 128 (W8) or zp (W4), cut to the operand type (pack2)
      steps         two 32-deep steps per tile: token row R's 32 k of step kk against those of channel R'
      grouped       group rows in LDS: sw rows 0, 1 | zp rows 0, 1 of 128 floats; row g goes to buffer g & 1 (waves 0, 1: sw, waves
                    2, 3: zp when present; lane l -> local channel 64 (wave & 1) + l, clamped to N - 1); group 0 before the loop, group
                    g + 1 under the first tile of group g.  At tin == 0 zadj = zp row (g & 1) at local channel 64 wn + 16 j + fr; at the
                    group's last tile acc = fma(part, sw row (g & 1) at local channel 64 wn + 16 j + 4 fq + e, acc) and part = 0
      epilogue      channel n0 + 64 wn + 16 j + 4 fq + e (skipped when >= N), row m0 + 64 wm + 16 i + fr (skipped when >= M):
                    fma(acc, sw[n], 0) per channel, acc + 0 grouped; one rounding; stored at m N + n.
    Reads outside a, the codes, sw or zp are counted and reported as a failure, as a bounds checker would; so is a read of a group
    row whose DMA was issued under the same tile (not yet retired by the next vmcnt(0) + barrier).  pad_rows records which token
    rows the lanes past M read."""
    dev = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.pad_rows = set()

    def fp(self, op, out, a, w):
        return FpModelRun()("fp", op, out, a, w)

    def __call__(self, entry, op, bits, a, codes, sw, zp=None, g=None, out="f32"):
        mut, f = self.mutant, np.float32
        (M, K), N = a.shape, codes.shape[0]
        w4, grouped = bits == 4, entry == "wqg"
        rowb = K // 2 if w4 else K
        assert codes.shape[1] == rowb and K % TK == 0 and N % 8 == 0 and (not grouped or (g % TK == 0 and K % g == 0))
        a_flat = np.concatenate([a.to(TDT[op]).double().numpy().ravel(), np.full(PAD, np.nan)])
        c_flat = np.concatenate([codes.contiguous().numpy().view(np.uint8).ravel(), np.full(rowb + PAD, 0x5A, dtype=np.uint8)])
        sizes = {"a": M * K, "codes": N * rowb, "sw": sw.numel(), "zp": 0 if zp is None else zp.numel()}
        s_flat = np.concatenate([sw.float().numpy().ravel(), np.full(2 * TN, np.nan, dtype=f)])
        z_flat = None if zp is None else np.concatenate([zp.float().numpy().ravel(), np.full(2 * TN, np.nan, dtype=f)])
        oob = {k: 0 for k in sizes}
        races = 0
        win = Window(M, N, out, "cpu")
        flat = win.flat.numpy()
        mt, nt, nk = -(-M // TM), -(-N // TN), K // TK
        tpg = g // TK if grouped else nk
        ng = nk // tpg
        CT, nb = (TK // 2, 4) if w4 else (TK, 8)
        fq_stride = CT // 16 if mut == "fq_stride_wrong" else CT // 8
        kk_stride = CT // 4 if mut == "kk_offset_wrong" else CT // 2
        zoff = f(0.0 if w4 else 128.0)
        if mut == "w4_decoded_with_128" and w4:
            zoff = f(128.0)
        if mut == "w8_decoded_without_128" and not w4:
            zoff = f(0.0)
        wave, q, lane = np.meshgrid(np.arange(4), np.arange(4), np.arange(64), indexing="ij")
        r = 8 * (4 * q + wave) + (lane >> 3)
        c = (lane & 7) ^ ((r >> 1) & 7)
        R = np.arange(128)
        swz = (R >> 1) & 7
        kk_i, fq_i, b_i = np.arange(2)[None, :, None, None], np.arange(4)[None, None, :, None], np.arange(nb)[None, None, None, :]
        for bid in range(mt * nt):
            tm = bid // nt
            tn = bid - tm * nt
            m0, n0 = tm * TM, tn * TN
            mrow = np.where(m0 + r < M, m0 + r, 0 if mut == "clamp_m_to_0" else M - 1)
            self.pad_rows |= set(mrow[m0 + r >= M].tolist())
            ncl = np.where(n0 + R < N, n0 + R, N if mut == "clamp_n_to_N" else N - 1)  # local channel 64 wn + 16 j + fr
            ngr = np.where(n0 + R < N, n0 + R, N - 1)                                  # the group rows' own clamp
            lds = np.full((2, 128, 8, 8), np.nan)
            glds = np.full(4 * TN, np.nan, dtype=f)  # sw row 0 | sw row 1 | zp row 0 | zp row 1
            issued = {}

            def issue_group(x, t):
                dst = (x + 1) & 1 if mut == "group_row_over_live_buffer" else x & 1
                base = 0 if mut == "group_row_stride_dropped" else x * N
                for kind, src, off in (("sw", s_flat, 0), ("zp", z_flat, 2 * TN)):
                    if src is not None:
                        oob[kind] += int((base + ngr >= sizes[kind]).sum())
                        glds[off + dst * TN + R] = src[base + ngr]
                        issued[(kind, dst)] = t

            zadj = np.full((128, 4), -zoff, dtype=f)  # [local channel, fq]
            if not grouped and z_flat is not None:
                oob["zp"] += int((ncl >= sizes["zp"]).sum())
                zadj = np.repeat((z_flat[ncl] - zoff).astype(f)[:, None], 4, axis=1)
            acc = np.zeros((128, 128), dtype=f)
            part = np.zeros((128, 128))
            late = None
            if grouped:
                issue_group(0, -1)
            gi = tin = 0
            with np.errstate(invalid="ignore", over="ignore"):
                for t in range(nk):
                    idx = (mrow * K + c * 8 + t * TK)[..., None] + np.arange(8)
                    oob["a"] += int((idx >= sizes["a"]).sum())
                    lds[t & 1, r, lane & 7] = a_flat[idx]
                    if grouped and tin == 0:
                        if gi + 1 < ng:
                            issue_group(gi + 1, t)
                        if z_flat is not None and not (mut == "zp_refresh_skipped_from_group_2" and gi >= 2):
                            races += issued.get(("zp", gi & 1)) == t
                            zrow = glds[2 * TN + (gi & 1) * TN:][:TN]
                            if mut == "zp_through_sw_lane_map":  # fq * 16 bytes in place of fr * 4
                                zadj = (zrow[(R // 16 * 16)[:, None] + 4 * np.arange(4)[None, :]] - zoff).astype(f)
                            else:
                                zadj = np.repeat((zrow - zoff).astype(f)[:, None], 4, axis=1)
                    last = grouped and tin + 1 == tpg

                    def fold(group):
                        nonlocal acc, part, races
                        sel = (group + 1) & 1 if mut == "sw_row_from_other_buffer" else group & 1
                        races += issued.get(("sw", sel)) == t
                        srow = np.concatenate([glds[sel * TN:], np.full(8, np.nan, dtype=f)])
                        if mut == "sw_through_zp_lane_map":  # fr * 4 bytes in place of fq * 16: token lane fr, element e
                            s2 = srow[(R // 16 * 16 + R % 4)[None, :] + (R % 16)[:, None]]
                        else:
                            s2 = np.broadcast_to(srow[:TN][None, :], (128, 128))
                        acc = fma32(part.astype(f), s2, acc)
                        if mut != "part_not_zeroed":
                            part = np.zeros((128, 128))

                    if last and mut == "fold_one_tile_early":
                        fold(gi)
                    addr = (ncl * rowb)[:, None, None, None] + fq_i * fq_stride + t * CT + kk_i * kk_stride + b_i
                    oob["codes"] += int((addr >= sizes["codes"]).sum())
                    byte = c_flat[addr]
                    if w4:
                        lo, hi = byte & 15, byte >> 4
                        u = np.concatenate([hi, lo] if mut == "nibbles_swapped" else [lo, hi], axis=-1)
                    else:
                        u = byte if mut == "xor_dropped" else byte ^ 0x80
                    wop = cut16((u.astype(f) + zadj[:, None, :, None]).astype(f), op)  # [channel, kk, fq, 8]
                    buf = lds[(t + 1) & 1 if mut == "token_parity_swapped" else t & 1]
                    for kk in range(2):
                        p = (4 * kk + np.arange(4))[None, :] ^ swz[:, None]
                        part = part + buf[R[:, None], p].reshape(128, 32) @ wop[:, kk].reshape(128, 32).T
                    if late is not None:
                        fold(late)
                        late = None
                    if last:
                        if mut == "fold_one_tile_late" and gi + 1 < ng:
                            late = gi
                        elif mut == "last_group_not_folded" and gi + 1 == ng:
                            pass
                        elif mut != "fold_one_tile_early":
                            fold(gi)
                        gi, tin = gi + 1, 0
                    else:
                        tin += 1
                if grouped:
                    y = (acc + f(0.0)).astype(f)
                else:
                    oob["sw"] += 0  # the epilogue reads sw only for channels below N
                    y = fma32(part.astype(f), np.broadcast_to(s_flat[np.minimum(n0 + R, N - 1)][None, :], (128, 128)), np.zeros((128, 128), dtype=f))
            live_m, live_n = R[m0 + R < M], R[n0 + R < N]
            o = GUARD + (m0 + live_m)[:, None] * N + (n0 + live_n)[None, :]
            flat[o] = to_bits(y[np.ix_(live_m, live_n)], out)
        fails = [f"model: {v} elements read outside {k}" for k, v in oob.items() if v]
        if races:
            fails.append(f"model: {races} reads of a group row whose DMA was still in flight")
        return Result(win, fails)


def probe_pad_rows(run):
    """Model only: the lanes past M read row M - 1 (the header's rule; such a lane's result is never stored, so no output can tell)."""
    if not isinstance(run, ModelRun):
        return []
    a, cval, sw, zp = dense_case(5, 8, 64, 64, 8, False, "cpu")
    run.pad_rows.clear()
    run("wq", "bf16", 8, a, raw_codes(cval, 8), sw[0], zp[0])
    return [] if run.pad_rows == {4} else [f"model: the lanes past M read token rows {sorted(run.pad_rows)}, not row M - 1"]


def model_battery(run):
    """The probes of A - D at the smallest set of cases that tells the mutants apart; -> {probe name: failures}."""
    got = {}
    for entry, g, bits, op, zp_null, skew in (("wq", None, 8, "bf16", False, False), ("wq", None, 4, "f16", False, False), ("wq", None, 4, "f16", False, True),
                                              ("wq", None, 8, "f16", True, False), ("wq", None, 4, "bf16", True, True), ("wqg", 64, 8, "f16", False, False),
                                              ("wqg", 64, 4, "bf16", False, True), ("wqg", A_K, 8, "bf16", False, False)):
        tag = "" if bits == 8 else " skewed" if skew else " plain"
        got[f"A table {entry} g={g} w{bits} {op} zp {'NULL' if zp_null else 'present'}{tag}"] = probe_table(run, entry, g, bits, op, zp_null, skew)
    for M, N, K, g, bits, op, zp_null in ((1, 8, 64, 64, 8, "bf16", False), (129, 136, 192, 64, 4, "f16", False), (129, 136, 320, 64, 8, "bf16", False),
                                          (129, 136, 384, 128, 4, "bf16", False), (257, 264, 640, 128, 8, "f16", True), (1, 136, 576, 192, 8, "bf16", False),
                                          (129, 8, 384, 384, 4, "f16", False)):
        tag = f"({M}, {N}, {K}) g={g} w{bits} {op} zp {'NULL' if zp_null else 'present'}"
        got[f"B dense {tag}"] = probe_dense(run, M, N, K, g, bits, op, zp_null)
        got[f"B signature {tag}"] = probe_signature(run, M, N, K, g, bits, op, zp_null)
    for gs in (0, 2, 4):
        got[f"B no leak group {gs} w8 bf16"] = probe_no_leak(run, gs, 8, "bf16")
    got["C twins w8 bf16 N=264"] = probe_twins(run, 8, "bf16", A_N)
    got["C twins w4 f16 N=8"] = probe_twins(run, 4, "f16", 8)
    got["D isolation wq w8 bf16"] = probe_isolation(run, "wq", 8, "bf16", quick=True)
    got["D isolation wqg w4 f16"] = probe_isolation(run, "wqg", 4, "f16", quick=True)
    got["D isolation wqg w8 bf16"] = probe_isolation(run, "wqg", 8, "bf16", quick=True)
    got["F padded lanes read row M - 1"] = probe_pad_rows(run)
    return got


def test_model_passes_every_probe():
    got = model_battery(ModelRun())
    assert {k: v for k, v in got.items() if v} == {}
    run = ModelRun()
    assert probe_isolation(run, "wq", 4, "f16") == [] and probe_isolation(run, "wqg", 8, "bf16") == []
    assert [f for gs in (1, 3) for f in probe_no_leak(run, gs, 4, "f16")] == []
    assert probe_dense(run, 257, 264, 576, 192, 4, "bf16", True) == [] and probe_signature(run, 257, 8, 320, 64, 4, "f16", True) == []


# what each mutant must fail at the least and what it must pass (substrings of the names in model_battery); "bounds": no output
# differs and only the model's bounds check sees it
MUTANT_FAILS = {
    "nibbles_swapped": ("A table wq g=None w4", "A table wqg g=64 w4", "B dense (129, 136, 192) g=64 w4", "C twins w4"),
    "fq_stride_wrong": ("A table wq g=None w8", "A table wq g=None w4", "B dense (1, 8, 64) g=64 w8", "B signature (129, 136, 384) g=128 w4"),
    "kk_offset_wrong": ("A table wq g=None w8", "A table wqg g=64 w4", "B dense (1, 8, 64) g=64 w8", "D isolation wq w8"),
    "w4_decoded_with_128": ("A table wq g=None w4 f16 zp present", "A table wq g=None w4 bf16 zp NULL", "B dense (129, 8, 384) g=384 w4", "C twins w4"),
    "w8_decoded_without_128": ("A table wq g=None w8 bf16 zp present", "A table wq g=None w8 f16 zp NULL", "B dense (257, 264, 640) g=128 w8", "C twins w8"),
    "xor_dropped": ("A table wq g=None w8 bf16 zp present", "A table wqg g=64 w8", "B signature (129, 136, 320) g=64 w8", "C twins w8"),
    "zp_through_sw_lane_map": ("A table wqg g=64 w8", "A table wqg g=64 w4", "B signature (129, 136, 320) g=64 w8", "D isolation wqg w4"),
    "sw_through_zp_lane_map": ("A table wqg g=64 w8", "A table wqg g=192 w8", "B signature (129, 136, 384) g=128 w4", "D isolation wqg w8"),
    "sw_row_from_other_buffer": ("A table wqg g=64 w8", "B dense (129, 136, 320) g=64 w8", "B signature (129, 136, 192) g=64 w4", "B no leak group 2"),
    "zp_refresh_skipped_from_group_2": ("A table wqg g=64 w4", "B dense (129, 136, 320) g=64 w8", "B signature (129, 136, 384) g=128 w4"),
    "group_row_over_live_buffer": ("A table wqg g=64 w8", "B dense (129, 136, 192) g=64 w4", "B signature (129, 136, 320) g=64 w8", "B no leak group 0"),
    "group_row_stride_dropped": ("A table wqg g=64 w8", "B dense (129, 136, 384) g=128 w4", "B signature (1, 136, 576) g=192 w8", "B no leak group 4"),
    "fold_one_tile_early": ("A table wqg g=64 w8", "B dense (1, 8, 64) g=64 w8", "B dense (129, 8, 384) g=384 w4", "B no leak group 2"),
    "fold_one_tile_late": ("A table wqg g=64 w4", "B dense (129, 136, 320) g=64 w8", "B signature (129, 136, 384) g=128 w4", "B no leak group 0"),
    "last_group_not_folded": ("A table wqg g=192 w8", "B dense (1, 8, 64) g=64 w8", "B signature (129, 136, 320) g=64 w8", "B no leak group 4"),
    "part_not_zeroed": ("A table wqg g=64 w8", "B dense (129, 136, 192) g=64 w4", "B signature (129, 136, 320) g=64 w8", "B no leak group 0"),
    "token_parity_swapped": ("A table wq g=None w8", "B dense (1, 8, 64) g=64 w8", "C twins w4", "D isolation wq w8"),
    "clamp_n_to_N": ("bounds",),
    "clamp_m_to_0": ("F padded lanes read row M - 1",),
}
MUTANT_PASSES = {
    "nibbles_swapped": ("w8",),
    "kk_offset_wrong": ("plain",),
    "w4_decoded_with_128": ("w8",),
    "w8_decoded_without_128": ("w4",),
    "xor_dropped": ("w4",),
    "zp_through_sw_lane_map": ("A table wq ", "zp NULL", "D isolation wq "),
    "sw_through_zp_lane_map": ("A table wq ", "D isolation wq "),
    "sw_row_from_other_buffer": ("A table wq ", "D isolation wq "),
    "zp_refresh_skipped_from_group_2": ("A table wq ", "zp NULL", "B dense (1, 8, 64)", "B dense (129, 8, 384) g=384", "B no leak group 0"),
    "group_row_over_live_buffer": ("A table wq ", "D isolation wq "),
    "group_row_stride_dropped": ("A table wq ", "B dense (1, 8, 64)", "B dense (129, 8, 384) g=384"),
    "fold_one_tile_early": ("A table wq ", "D isolation wq "),
    "fold_one_tile_late": ("A table wq ", "B dense (1, 8, 64)", "B dense (129, 8, 384) g=384", "A table wqg g=192"),
    "last_group_not_folded": ("A table wq ", "D isolation wq "),
    "part_not_zeroed": ("A table wq ", "B dense (1, 8, 64)", "B dense (129, 8, 384) g=384", "A table wqg g=192"),
    "clamp_m_to_0": ("A", "B", "C", "D"),
}
MUTANT_NOTES = {
    "kk_offset_wrong": "W4: the half-tile offset moves a load by 16 codes, and the plain W4 table (n + 5 k) % 16 repeats every 16 k: only the skewed table sees it",
    "clamp_n_to_N": "no output differs: a lane past N computes and never stores; the model's bounds check alone sees the read past the codes and zp",
    "clamp_m_to_0": "no output can differ: a lane past M computes and never stores, and row 0 is a valid address; seen only by the model's record of the rows those lanes read",
    "zp_refresh_skipped_from_group_2": "needs three groups and a zero point: the shapes with ng = 1 and the zp = NULL passes cannot see it",
    "fold_one_tile_late": "the last group folds in place, so one group is unaffected",
}


@pytest.fixture(scope="module")
def mutant_results():
    cache = {}

    def get(mutant):
        if mutant not in cache:
            cache[mutant] = {k: v for k, v in model_battery(ModelRun(mutant)).items() if v}
        return cache[mutant]

    return get


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_named_probes(mutant, mutant_results):
    failed = mutant_results(mutant)
    print(f"MUTANT {mutant}: fails {sorted(failed)}")
    assert failed, mutant
    for want in MUTANT_FAILS[mutant]:
        if want == "bounds":  # every failure is the bounds check's
            assert all(all("read outside" in f for f in v) for v in failed.values()), failed
        else:
            assert any(want in k for k in failed), (mutant, want, sorted(failed))
    for keep in MUTANT_PASSES.get(mutant, ()):
        assert not any(k.startswith(keep) or f" {keep}" in k for k in failed), (mutant, keep, sorted(failed))


def test_signature_checker_names_the_group():
    """What the signature's failure message says for the three mutants that misplace one group's row."""
    for mutant, K, want in (("zp_refresh_skipped_from_group_2", 192, "group 2: decoded with the zero-point row of group 1"),
                            ("zp_refresh_skipped_from_group_2", 320, "group 2 (and [3, 4]): decoded with another zero-point row"),
                            ("sw_row_from_other_buffer", 320, "group 0 (and [1, 2, 3, 4]): folded with another scale row"),
                            ("zp_through_sw_lane_map", 320, "sw's lane map"), ("sw_through_zp_lane_map", 320, "zp's lane map")):
        fails = probe_signature(ModelRun(mutant), 129, 136, K, 64, 8, "bf16", False)
        assert fails and any(want in f for f in fails), (mutant, fails)
    fails = probe_table(ModelRun("kk_offset_wrong"), "wq", None, 4, "bf16", False, skew=True)
    assert any("kk 1" in f and "nibble" in f and "fr " in f for f in fails), fails


def mutant_table_text():
    lines = ["Mutants of the numpy model in tests/test_gpu_wq16_probes.py (ModelRun) and the probes that catch them",
             "=" * 102, "",
             "The model restates both kernels of csrc/gemm_wq16.hip as written (tile origin and clamps, the code address and load per",
             "(j, kk, fq), the W8 / W4 decode, the token DMA and fragment reads, the two 32-deep steps, the two group-row buffers with",
             "their one-group-ahead issue, the zp refresh, the fold, the epilogue's lane map); each mutant is one deliberate error in it.",
             "test_mutants_of_the_model_fail_named_probes runs the probes of the GPU tests on every mutant, on a machine without a GPU, and",
             "asserts for each the probes named below (substrings of the names in model_battery; `bounds`: only the model's bounds check);",
             "test_mutant_table_is_the_committed_one keeps this file equal to the table asserted there.", ""]
    for m in MUTANTS:
        lines.append(m)
        lines += [f"    fails   {p}" for p in MUTANT_FAILS[m]]
        lines += [f"    passes  {p}" for p in MUTANT_PASSES.get(m, ())]
        if m in MUTANT_NOTES:
            lines.append(f"    note    {MUTANT_NOTES[m]}")
    return "\n".join(lines) + "\n"


def test_mutant_table_is_the_committed_one():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wq16_probe_mutants.txt")
    with open(path) as fh:
        assert fh.read() == mutant_table_text()
    assert set(MUTANT_FAILS) == set(MUTANTS) and all(MUTANT_FAILS[m] for m in MUTANTS)
    single = [MUTANT_FAILS[m] for m in MUTANTS if len(MUTANT_FAILS[m]) == 1]
    assert len(single) == len(set(single)) == 2  # the two clamps, each seen by its own check alone (MUTANT_NOTES)


if __name__ == "__main__":  # PYTHONPATH=tests:wan2.1-quantization_amd python tests/test_gpu_wq16_probes.py > profiles/wq16_probe_mutants.txt
    print(mutant_table_text(), end="")
