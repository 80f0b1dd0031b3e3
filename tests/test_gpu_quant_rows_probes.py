"""The per-row quantisers in front of every quantised Linear (csrc/rowwise.hip) -- wanq_quant_rows (plain, GELU, static absmax),
wanq_quant_rows_levels, wanq_quant_rows_fp8, wanq_quant_rows_mx -- on rows whose answer is known bit for bit.  Every call goes through
the C ABI; every output carries one guard row (codes) / one guard slot (scale, sum) behind the last row, checked after every call.

  A  int8 probes     rows x[r, c] = k[r, c] 2^e_r with k from a hash of (r, c) and one element +-levels 2^e_r: amax / levels is
                     2^e_r exactly, the codes are k, the sum is (sum k) 2^e_r.  Placement, the absmax walk, ties, the static form,
                     the levels entry, a GELU that is exact by saturation, the library's own GELU on random data, the wave kernel
                     against the general kernel, random rows against kr.quant_sum.
  B  fp8 and MX      e4m3 / e2m1 codes from a hash times a power of two: codes, scales and scale bytes by equality.
  C  rows = 0 and the width rules through the ABI (what tests/test_abi.py, test_fp8_abi.py and test_mx_abi.py do not hold).
  E  CPU self-tests (not marked gpu): a numpy model of the row frame and of the wave kernel passes every checker, thirteen mutants
     of it fail named probes (profiles/quant_rows_probe_mutants.txt), the generators refuse rows without an exact expectation.

Every comparison is an equality.  An fp16 scale or sum is the exact (float64) value rounded once to nearest even; every exact
value here is an fp32 number, so the kernel's __float2half_rn of its fp32 result is that one rounding.

Exact GELU: gelu_tanh_fast_f32(x) = x rcp(1 + exp2(t)), t = x fma(x^2, -0.10294324, -2.3022082).  For x >= 11, t <= -162 and
exp2(t) = 0 in fp32 (below 2^-149), rcp(1) = 1: the result is x.  For x <= -11, t >= 162 > 128, exp2(t) = inf, rcp(inf) = 0: the
result is -0.  The probe keeps |x| >= 16 (GELU_EXACT_FROM); gelu_np restates the expression and the generator checks it on every row.

Width -> compiled form (chunks = cols / 8; row_ladder in csrc/row_frame.h; (WPR, NCH) = waves per row, chunk slots per lane):

  chunks <=   64   128   192   256   512   768   1024  1280  1536  1792  2048
  form       (1,1) (1,2) (1,3) (1,4) (4,2) (4,3) (4,4) (4,5) (4,6) (4,7) (4,8)
  smallest / largest width tested: 8 | 264 / 512, 520 / 1024, 1032 / 1536, 1544 / 2048, 2056 / 4096, 4104 / 6144, 6152 / 8192,
  8200 / 10240, 10248 / 12288, 12296 / 14336, 14344 / 16384 (MX: 32 | 288 / 512, 544 / 1024, ..., 14368 / 16384)

  entry                    input          widths                              kernel
  wanq_quant_rows          f32            the ladder                          rowwise_kernel<WPR, NCH, false>
  wanq_quant_rows          bf16, f16      the ladder but 8712 .. 9216         rowwise_kernel<WPR, NCH, false>
  wanq_quant_rows          bf16, f16      8712, 8720, 8960, 9208, 9216        quant_rows_wave_kernel<T, 18, GELU>: 8712 (1089 chunks) and
                                                                              9208 (1151) end in the 8-byte store, the others in the 16-byte one
  wanq_quant_rows          bf16, f16      8704 | 9224 (outside the window)    rowwise_kernel<4, 5, false>
  wanq_quant_rows static   every dtype    the ladder and the window           rowwise_kernel<WPR, NCH, false> (never the wave kernel)
  wanq_quant_rows_levels   every dtype    the ladder                          rowwise_kernel<WPR, NCH, false>
  wanq_quant_rows_fp8      every dtype    the ladder                          quant_rows_fp8_kernel<WPR, NCH>
  wanq_quant_rows_mx       every dtype    32 and the ladder in steps of 32    quant_rows_mx_kernel<WPR, NCH, FP4>, both formats
"""
import collections
import os

import numpy as np
import pytest
import torch

from oracle import kernel_ref as kr
from test_gpu_rowwise_probes import DTC, FORMS, LN_WIDTHS, SENT, SENT8, TDT, WANQ_E_SHAPE, WANQ_OK, first_bad, form_of, hash32, rnd

gpu = pytest.mark.gpu
DEV = "cuda"
F = np.float32
DTS = ["f16", "bf16", "f32"]
VECS = [("f32", True), ("f16", True), ("f32", False), ("f16", False)]  # (vector dtype, sum present)
LADDER = [w for w in LN_WIDTHS if w not in (5120, 8960, 13824)]  # the smallest and the largest width of every form, and 264
WAVE_WIDTHS = [8704, 8712, 8720, 8960, 9208, 9216, 9224]
MX_WIDTHS = [32, 288, 512] + [w for (lo, _, _), (hi, _, _) in zip(FORMS, FORMS[1:]) for w in (lo * 8 + 32, hi * 8)]
U8_SENT, SCALE_SENT = 0x7F, 0xFF  # never produced: the e4m3 NaN pattern; an E8M0 byte above 254
GELU_EXACT_FROM = 16.0
E_IN = {"f16": (-6, 2), "bf16": (-18, 18), "f32": (-18, 18)}  # 127.5 2^e and (sub-floor rows aside) 2^e >= 1e-6 are exact in the dtype
E_VEC = {"f32": (-18, 18), "f16": (-14, 8)}                    # 2^e and 127 2^e are exact in the vector dtype
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.int64)  # the 254 finite e4m3 codes
E4M3_VAL = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
E2M1_VAL = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0] + [-0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
Rows = collections.namedtuple("Rows", "x q scale sum amax", defaults=(None,))


def in_window(dt, cols):
    return dt in ("bf16", "f16") and 8704 < cols <= 9216


def kernel_of(dt, cols, static=False, levels=False):
    """What wanq_quant_rows / _levels launches: ("wave", store branch of the last chunk) or ("general", WPR, NCH)."""
    if in_window(dt, cols) and not static and not levels:
        return ("wave", 8 if (cols // 8) % 2 else 16)
    return ("general",) + form_of(cols)


# ================================================================================================ generators
def exps(rows, dt, vec, salt):
    lo, hi = max(E_IN[dt][0], E_VEC[vec][0]), min(E_IN[dt][1], E_VEC[vec][1])
    return lo + (hash32(np.arange(rows), 7, salt) % np.uint64(hi - lo + 1)).astype(np.int64)


def hashed(rows, cols, salt, mod):
    return (hash32(np.arange(rows)[:, None], np.arange(cols)[None, :], salt) % np.uint64(mod)).astype(np.int64)


def pin(k, value, salt, at=None):
    """One element per row set to +-value (sign and column by a hash of the row, or the columns `at`)."""
    r = np.arange(k.shape[0])
    col = (hash32(r, 3, salt) % np.uint64(k.shape[1])).astype(np.int64) if at is None else np.asarray(at)
    k[r, col] = np.where(hash32(r, 5, salt) & np.uint64(1), value, -value)
    return col


def f32_expr(x, levels, floor, amax=None):
    """The contract in plain fp32 numpy: scale = max(amax / levels, floor), q = rint(x / scale) (0 where scale is 0; clamped in the
    static form), sum = (float)(sum q) scale."""
    x32 = np.asarray(x, F)
    am = np.abs(x32).max(axis=1) if amax is None else np.asarray(amax, F)
    scale = np.maximum(am / F(levels), F(floor))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale[:, None] > 0, np.rint(x32 / scale[:, None]), 0).astype(np.int64)
    if amax is not None:
        q = np.clip(q, -128, 127)
    return q, scale.astype(np.float64), (q.sum(axis=1).astype(F) * scale).astype(np.float64)


def finish(x, q, scale, ssum, dt, what, levels=127, floor=1e-6, amax=None):
    """Refuses (ValueError) a row that is not exact in its dtype, or whose stated expectation is not the fp32 expression's."""
    if not np.array_equal(rnd(x, dt), x):
        raise ValueError(f"{what}: an input is not exact in {dt}")
    eq, es, esum = f32_expr(x, levels, floor, amax)
    if not (np.array_equal(eq, q) and np.array_equal(es, scale) and np.array_equal(esum, ssum)):
        raise ValueError(f"{what}: the stated expectation is not exact")
    return Rows(x, q.astype(np.int64), scale, ssum, amax)


def place_rows(rows, cols, dt, vec, n=127, floor=1e-6, salt=1, kmax=None, at=None, e=None):
    """k in [-(n - 1), n - 1] by a hash of (r, c), one +-n: codes k, scale 2^e_r, sum (sum k) 2^e_r."""
    kmax = (n - 1 if n > 1 else 1) if kmax is None else kmax
    k = hashed(rows, cols, salt, 2 * kmax + 1) - kmax
    pin(k, n, salt, at)
    e = exps(rows, dt, vec, salt) if e is None else e
    s = np.ldexp(1.0, e)
    return finish(k * s[:, None], k, s, k.sum(axis=1) * s, dt, "placement", n, floor)


def walk_positions(kernel, cols):
    """Columns of the single maximum, one row each: first and last column, the first and last lane of every wave's share, every
    chunk slot (its first live chunk, a hashed one, its last live chunk), both chunks of a pair in every pair slot of the wave kernel;
    padded with hashed columns to 4 n + 1 rows."""
    chunks = cols // 8
    ch = {0, chunks - 1}
    if kernel[0] == "wave":
        for h in range(9):
            for lane in {int(hash32(h, 1, 41) % np.uint64(64))} | ({0, 63} if h in (0, 8) else set()):
                ch |= {c for c in (2 * (lane + 64 * h), 2 * (lane + 64 * h) + 1) if c < chunks}
    else:
        wpr, nch = kernel[1:]
        for sub in range(wpr):
            ch |= {c for c in (sub * 64, sub * 64 + 63) if c < chunks}
        for i in range(nch):
            base = i * 64 * wpr
            ch |= {c for c in (base, base + int(hash32(i, 2, 41) % np.uint64(64 * wpr)), base + 64 * wpr - 1) if c < chunks} | {min(base + 64 * wpr, chunks) - 1}
    cols_at = [0, cols - 1] + [c * 8 + int(hash32(c, 3, 41) % np.uint64(8)) for c in sorted(ch)]
    j = 0
    while len(cols_at) % 4 != 1:
        cols_at.append(int(hash32(j, 4, 41) % np.uint64(cols)))
        j += 1
    assert len(cols_at) <= 41
    return cols_at


def walk_rows(kernel, cols, dt, vec):
    at = walk_positions(kernel, cols)
    return place_rows(len(at), cols, dt, vec, salt=2, kmax=63, at=at)


def tie_rows(rows, cols, dt, vec, n=127, floor=1e-6, neighbours=False, salt=3):
    """x = (k + 1/2) 2^e, |k + 1/2| <= n - 1/2, one +-n: codes round to nearest even.  neighbours (fp32): each tie, its fp32
    predecessor or its successor by a hash; the codes are the fp32 expression's."""
    k = hashed(rows, cols, salt, 2 * n) - n + 0.5
    col = pin(k, float(n), salt)
    e = exps(rows, dt, vec, salt)
    s = np.ldexp(1.0, e)
    x = k * s[:, None]
    q = np.rint(k)  # ties to even
    if neighbours:
        assert dt == "f32"
        step = hashed(rows, cols, salt + 100, 3) - 1
        step[np.arange(rows), col] = 0
        x32 = x.astype(F)
        x = np.where(step == 0, x32, np.nextafter(x32, np.where(step > 0, F(np.inf), F(-np.inf)).astype(F))).astype(np.float64)
        q = np.where(step == 0, q, np.where(step > 0, np.ceil(k), np.floor(k)))
    q = q.astype(np.int64)
    return finish(x, q, s, q.sum(axis=1) * s, dt, "ties", n, floor)


def static_rows(rows, cols, dt, vec, salt=4):
    """k in [-300, 300] (above 256 even, so that bf16 holds it), the given absmax 127 2^e: codes clip(k, -128, 127)."""
    k = hashed(rows, cols, salt, 601) - 300
    k = np.where(np.abs(k) > 256, 2 * (k // 2), k)
    e = exps(rows, dt, vec, salt)
    s = np.ldexp(1.0, e)
    q = np.clip(k, -128, 127)
    return finish(k * s[:, None], q, s, q.sum(axis=1) * s, dt, "static", amax=127.0 * s)


def zero_rows(rows, cols, dt, n, floor):
    z = np.zeros((rows, cols))
    return finish(z, z.astype(np.int64), np.full(rows, float(F(floor))), np.zeros(rows), dt, "zero rows", n, floor)


def subfloor_rows(rows, cols, dt, n, floor, salt=5):
    """x = k 2^-20 with one +-n 2^-20: amax / n = 2^-20 < 1e-6.  The expectation is the fp32 expression (with floor 0: k and 2^-20)."""
    k = hashed(rows, cols, salt, 2 * n + 1) - n
    pin(k, n, salt)
    x = k * 2.0 ** -20
    q, s, ssum = f32_expr(x, n, floor)
    if floor == 0 and not np.array_equal(q, k):
        raise ValueError("sub-floor rows: not exact")
    return finish(x, q, s, ssum, dt, "sub-floor rows", n, floor)


def gelu_np(x):
    """gelu_tanh_fast_f32 (csrc/wanq_common.h), operation by operation in fp32 (the fma through float64)."""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        xx = (x * x).astype(F)
        inner = (xx.astype(np.float64) * float(F(-0.10294324)) + float(F(-2.3022082))).astype(F)
        t = (x * inner).astype(F)
        return (x * (F(1) / (F(1) + np.exp2(t).astype(F)))).astype(F)


def gelu_rows(rows, cols, dt, vec, salt=6, scale_from_all=False):
    """By a hash of (r, c): zero, 16 k 2^e (k in 1 .. 127) or -(2048 + 16 m) 2^e, e in 0 .. 3, one +127 16 2^e: after the GELU the
    positives are unchanged and everything else is 0, so the codes are k / 0 and the scale 16 2^e comes from the positives alone."""
    kind = hashed(rows, cols, salt, 3)
    k = np.where(kind == 1, 1 + hashed(rows, cols, salt + 1, 127), 0)
    neg = np.where(kind == 2, 128 + hashed(rows, cols, salt + 2, 128), 0)
    r = np.arange(rows)
    col = (hash32(r, 3, salt) % np.uint64(cols)).astype(np.int64)
    k[r, col], neg[r, col] = 127, 0
    s = 16.0 * np.ldexp(1.0, (hash32(r, 7, salt) % np.uint64(4)).astype(np.int64))
    x = (k - neg) * s[:, None]
    if not np.array_equal(rnd(x, dt), x):
        raise ValueError(f"gelu rows: an input is not exact in {dt}")
    g = gelu_np(x).astype(np.float64)
    if not (np.abs(x[x != 0]).min() >= GELU_EXACT_FROM and np.array_equal(g, np.where(x > 0, x, 0.0)) and np.signbit(g[x < 0]).all()):
        raise ValueError("gelu rows: the GELU is not exact on this row")
    if scale_from_all:
        s = np.abs(x).max(axis=1) / 127.0
    return finish(g, k, s, k.sum(axis=1) * s, "f32", "gelu rows")._replace(x=x)


def random_rows(rows, cols, dt, seed):
    """The rows of tests/test_gpu_rowwise.py: Gaussian times per-column log-normal scales, a zero row, a row with outliers."""
    g = torch.Generator().manual_seed(seed * 100003 + cols)
    x = torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(cols, generator=g))
    x[1] = 0
    x[2, ::7] *= 30
    return x.to(TDT[dt]).double().numpy()


def fp8_rows(rows, cols, dt, salt=8):
    """e4m3 values by a hash of (r, c) over the 254 finite codes, times 2^e_r, one +-448 2^e_r: codes as hashed, scale 2^e_r."""
    code = FINITE[hashed(rows, cols, salt, 254)]
    r = np.arange(rows)
    col = (hash32(r, 3, salt) % np.uint64(cols)).astype(np.int64)
    code[r, col] = np.where(hash32(r, 5, salt) & np.uint64(1), 0x7E, 0xFE)
    s = np.ldexp(1.0, exps(rows, dt, "f32", salt))
    x = E4M3_VAL[code] * s[:, None]
    if not np.array_equal(rnd(x, dt), x):
        raise ValueError(f"fp8 rows: an input is not exact in {dt}")
    return Rows(x, code, s, None)


def mx_rows(rows, cols, dt, fp4, salt=9):
    """Per block of 32: codes by a hash of (r, c), the block's scale byte s by a hash of (r, block) (20 .. 240; fp16: 112 .. 134, where
    every value is exact), at a hashed place in the block a code with the format's largest exponent (e4m3: 256 .. 448, e2m1: 4 or 6),
    so that E(amax) - emax = s whatever the other codes are.  x = value 2^(s - 127).  -> codes [rows, cols], scale bytes [rows, cols / 32]."""
    nb = cols // 32
    lo, hi = (112, 134) if dt == "f16" else (20, 240)
    s = lo + hashed(rows, nb, salt, hi - lo + 1)
    code = hashed(rows, cols, salt + 1, 16) if fp4 else FINITE[hashed(rows, cols, salt + 1, 254)]
    h = hash32(np.arange(rows)[:, None], np.arange(nb)[None, :], salt + 2)
    at = (np.arange(nb)[None, :] * 32 + (h % np.uint64(32)).astype(np.int64))
    top = ((6 + ((h >> np.uint64(5)) & np.uint64(1))) if fp4 else (0x78 + (h >> np.uint64(5)) % np.uint64(7))).astype(np.int64)
    top |= np.where((h >> np.uint64(9)) & np.uint64(1), 8 if fp4 else 0x80, 0)
    np.put_along_axis(code, at, top, axis=1)
    x = np.ldexp((E2M1_VAL if fp4 else E4M3_VAL)[code], np.repeat(s, 32, axis=1) - 127)
    if not (np.array_equal(rnd(x, dt), x) and np.isfinite(x).all()):
        raise ValueError(f"mx rows: an input is not exact in {dt}")
    return Rows(x, code, s, None)


def pack_e2m1(code):
    return code[:, 0::2] | (code[:, 1::2] << 4)  # even column in the low nibble


# ================================================================================================ checkers
def vec_round(a, vec):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16 if vec == "f16" else F).astype(np.float64)


def check_int8(o, want, vec, with_sum, name):
    """o: q [rows + 1, cols], scale, sum [rows + 1] as the runner returns them.  Static form: the scale buffer must hold the given absmax."""
    rows, fails = want.q.shape[0], []
    bad = ~(o["q"][:rows] == want.q)
    if bad.any():
        fails.append(first_bad(bad, o["q"], want.q, "q", f", slot stride {64 * 8}"))
    if not (o["q"][rows] == SENT8).all():
        c = int(np.argwhere(o["q"][rows] != SENT8)[0][0])
        fails.append(f"q: the guard row behind the last row was written, first at col {c} (chunk {c // 8}): {o['q'][rows, c]}")
    wscale = vec_round(want.scale if want.amax is None else want.amax, vec)
    if not np.array_equal(o["scale"][:rows], wscale):
        r = int(np.argwhere(~(o["scale"][:rows] == wscale))[0][0])
        fails.append(f"scale: first difference at row {r}: got {o['scale'][r]!r} expected {wscale[r]!r}" + (" (the given absmax was overwritten)" if want.amax is not None else ""))
    wsum = vec_round(want.sum, vec) if with_sum else np.full(rows, SENT)
    if not np.array_equal(o["sum"][:rows], wsum):
        r = int(np.argwhere(~(o["sum"][:rows] == wsum))[0][0])
        fails.append(f"sum: first difference at row {r}: got {o['sum'][r]!r} expected {wsum[r]!r}" + ("" if with_sum else " (sum is NULL: nothing may be written)"))
    if o["scale"][rows] != SENT or o["sum"][rows] != SENT:
        fails.append("scale / sum: the guard slot behind the last row was written")
    return [f"{name}: {f}" for f in fails]


def check_bytes(o, want_q, want_scale, name):
    """fp8 / MX: o["q"] [rows + 1, bytes per row], o["scale"] [rows + 1] (fp32) or [rows + 1, blocks] (bytes)."""
    rows, fails = want_q.shape[0], []
    bad = ~(o["q"][:rows] == want_q)
    if bad.any():
        per = 8 * want_q.shape[1] // (want_scale.shape[1] * 32) if want_scale.ndim == 2 else 8  # bytes per chunk
        r, c = [int(v) for v in np.argwhere(bad)[0]]
        fails.append(f"q: {int(bad.sum())} bytes differ; first at row {r} byte {c} (chunk {c // per}, lane {(c // per) % 64}): got {int(o['q'][r, c]):#x} expected {int(want_q[r, c]):#x}")
    if not (o["q"][rows] == U8_SENT).all():
        fails.append("q: the guard row behind the last row was written")
    if not np.array_equal(o["scale"][:rows], want_scale):
        at = np.argwhere(~(o["scale"][:rows] == want_scale))[0].tolist()
        fails.append(f"scale: first difference at (row, block) {at}: got {o['scale'][tuple(at)]!r} expected {want_scale[tuple(at)]!r}")
    if not (o["scale"][rows] == (SCALE_SENT if want_scale.ndim == 2 else SENT)).all():
        fails.append("scale: the guard behind the last row was written")
    return [f"{name}: {f}" for f in fails]


# ================================================================================================ the GPU runner
def dev_t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TDT[dt]).to(DEV)


class Gpu:
    """The four entries through the C ABI on buffers with a guard row.  x: float64 values exact in dt."""

    def int8(self, x, dt, vec, with_sum, act=0, amax=None, levels=None, floor=None):
        from viditq_extension import _C

        rows, cols = x.shape
        xt = dev_t(x, dt)
        q = torch.full((rows + 1, cols), SENT8, dtype=torch.int8, device=DEV)
        scale = torch.full((rows + 1,), SENT, dtype=TDT[vec], device=DEV)
        ssum = torch.full((rows + 1,), SENT, dtype=TDT[vec], device=DEV)
        if amax is not None:
            scale[:rows] = dev_t(amax, vec)
        head = (_C.ptr(xt), DTC[dt], _C.ptr(q), _C.ptr(scale), _C.ptr(ssum) if with_sum else None, DTC[vec], rows, cols)
        if levels is None:
            _C.call("wanq_quant_rows", *head, act, 0 if amax is None else 1, _C.stream())
        else:
            _C.call("wanq_quant_rows_levels", *head, int(levels), float(floor), _C.stream())
        torch.cuda.synchronize()
        return {"q": q.cpu().to(torch.int64).numpy(), "scale": scale.cpu().double().numpy(), "sum": ssum.cpu().double().numpy()}

    def fp8(self, x, dt):
        from viditq_extension import _C

        rows, cols = x.shape
        xt = dev_t(x, dt)
        q = torch.full((rows + 1, cols), U8_SENT, dtype=torch.uint8, device=DEV)
        scale = torch.full((rows + 1,), SENT, dtype=torch.float32, device=DEV)
        _C.call("wanq_quant_rows_fp8", _C.ptr(xt), DTC[dt], _C.ptr(q), _C.ptr(scale), rows, cols, 0, _C.stream())
        torch.cuda.synchronize()
        return {"q": q.cpu().to(torch.int64).numpy(), "scale": scale.cpu().double().numpy()}

    def mx(self, x, dt, fp4):
        from viditq_extension import _C

        rows, cols = x.shape
        xt = dev_t(x, dt)
        q = torch.full((rows + 1, cols // 2 if fp4 else cols), U8_SENT, dtype=torch.uint8, device=DEV)
        scale = torch.full((rows + 1, cols // 32), SCALE_SENT, dtype=torch.uint8, device=DEV)
        _C.call("wanq_quant_rows_mx", _C.ptr(xt), DTC[dt], _C.ptr(q), _C.ptr(scale), rows, cols, 1 if fp4 else 0, 0, _C.stream())
        torch.cuda.synchronize()
        return {"q": q.cpu().to(torch.int64).numpy(), "scale": scale.cpu().to(torch.int64).numpy()}


# ================================================================================================ the probes (run: Gpu() or Model())
def dts_at(cols):
    return DTS if cols in LADDER else ["f16", "bf16"]


def probe_placement(run, cols, dt, vec, with_sum, rows=13):
    want = place_rows(rows, cols, dt, vec)
    return check_int8(run.int8(want.x, dt, vec, with_sum), want, vec, with_sum, f"A1 placement {dt} {cols} vec={vec} sum={with_sum} {kernel_of(dt, cols)}")


def probe_walk(run, cols, dt, vec):
    kernel = kernel_of(dt, cols)
    want = walk_rows(kernel, cols, dt, vec)
    return check_int8(run.int8(want.x, dt, vec, True), want, vec, True, f"A2 walk {dt} {cols} vec={vec} {kernel}")


def probe_ties(run, cols, dt, vec, with_sum, neighbours=False, rows=13):
    want = tie_rows(rows, cols, dt, vec, neighbours=neighbours)
    return check_int8(run.int8(want.x, dt, vec, with_sum), want, vec, with_sum, f"A3 ties{' and neighbours' if neighbours else ''} {dt} {cols} vec={vec} {kernel_of(dt, cols)}")


def probe_static(run, cols, dt, vec, with_sum, rows=13):
    want = static_rows(rows, cols, dt, vec)
    return check_int8(run.int8(want.x, dt, vec, with_sum, amax=want.amax), want, vec, with_sum, f"A4 static {dt} {cols} vec={vec} sum={with_sum}")


def stack(*parts):
    return Rows(np.concatenate([p.x for p in parts]), np.concatenate([p.q for p in parts]), np.concatenate([p.scale for p in parts]),
                np.concatenate([p.sum for p in parts]))


def probe_levels(run, cols, dt, vec, with_sum, n, floor):
    """13 rows: 5 of placement, 4 of ties (the fp32 neighbours too for fp32 input), 2 of zeros, 2 below the floor."""
    want = stack(place_rows(5, cols, dt, vec, n, floor, salt=11), tie_rows(4, cols, dt, vec, n, floor, neighbours=(dt == "f32"), salt=12),
                 zero_rows(2, cols, dt, n, floor), subfloor_rows(2, cols, dt, n, floor))
    return check_int8(run.int8(want.x, dt, vec, with_sum, levels=n, floor=floor), want, vec, with_sum, f"A5 levels n={n} floor={floor} {dt} {cols} vec={vec} sum={with_sum}")


def probe_gelu_exact(run, cols, dt, vec, with_sum, rows=13):
    want = gelu_rows(rows, cols, dt, vec)
    return check_int8(run.int8(want.x, dt, vec, with_sum, act=1), want, vec, with_sum, f"A6 gelu exact {dt} {cols} vec={vec} {kernel_of(dt, cols)}")


def probe_wave_against_general(run, cols, dt, act, rows=13):
    """The same 16-bit rows as they are (the wave kernel) and converted exactly to fp32 (rowwise_kernel<4, 5, false>)."""
    assert kernel_of(dt, cols)[0] == "wave" and kernel_of("f32", cols) == ("general", 4, 5)
    x = random_rows(rows, cols, dt, 17) * (0.25 if act else 1.0)
    x = rnd(x, dt)
    a, b = run.int8(x, dt, "f32", True, act=act), run.int8(x, "f32", "f32", True, act=act)
    fails = []
    bad = ~(a["q"][:rows] == b["q"][:rows])
    if bad.any():
        fails.append(first_bad(bad, a["q"], b["q"], "q (wave kernel: got, general kernel: expected)"))
    if not ((a["q"][rows] == SENT8).all() and (b["q"][rows] == SENT8).all()):
        fails.append("q: the guard row behind the last row was written")
    for key in ("scale", "sum"):
        if not np.array_equal(a[key], b[key]):
            fails.append(f"{key}: wave kernel {a[key]} general kernel {b[key]}")
    return [f"A8 wave against general {dt} {cols} act={act}: {f}" for f in fails]


def probe_random(run, cols, dt, vec="f32", rows=13):
    x = random_rows(rows, cols, dt, 23)
    q, scale, ssum = kr.quant_sum(x.astype(F))
    want = Rows(x, q.astype(np.int64), scale.astype(np.float64), ssum.astype(np.float64))
    return check_int8(run.int8(x, dt, vec, True), want, vec, True, f"A9 random {dt} {cols} {kernel_of(dt, cols)}")


def probe_fp8(run, cols, dt, rows=13):
    want = fp8_rows(rows, cols, dt)
    return check_bytes(run.fp8(want.x, dt), want.q, want.scale, f"B fp8 {dt} {cols} {form_of(cols)}")


def probe_mx(run, cols, dt, fp4, rows=13):
    want = mx_rows(rows, cols, dt, fp4)
    return check_bytes(run.mx(want.x, dt, fp4), pack_e2m1(want.q) if fp4 else want.q, want.scale, f"B mx {'e2m1' if fp4 else 'e4m3'} {dt} {cols} {form_of(cols)}")


def report(fails):
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ A. int8 probes (GPU)
@gpu
@pytest.mark.parametrize("cols", LADDER + WAVE_WIDTHS)
def test_placement_and_sum(cols):
    """Codes in [-126, 126] and one +-127: codes, scale and sum by equality, every input dtype against both vector dtypes, sum
    present and NULL; 13 rows (one surplus wave in the one-wave-per-row forms and in the wave kernel)."""
    report([f for dt in dts_at(cols) for vec, with_sum in VECS for f in probe_placement(Gpu(), cols, dt, vec, with_sum)])


@gpu
@pytest.mark.parametrize("cols", LADDER + WAVE_WIDTHS)
def test_absmax_walk(cols):
    """One row per position class of the single maximum, all other |k| <= 63: a reduction that misses a wave, a slot, a lane or the
    second chunk of a pair halves the scale."""
    report([f for i, dt in enumerate(dts_at(cols)) for f in probe_walk(Gpu(), cols, dt, ("f32", "f16")[(i + cols // 8) % 2])])


@gpu
@pytest.mark.parametrize("cols", LADDER + WAVE_WIDTHS)
def test_ties_round_to_even(cols):
    fails = []
    for i, dt in enumerate(dts_at(cols)):
        vec, with_sum = VECS[(i + cols // 8) % 4]
        fails += probe_ties(Gpu(), cols, dt, vec, with_sum)
    if cols in LADDER:
        fails += probe_ties(Gpu(), cols, "f32", "f32", True, neighbours=True)
    report(fails)


@gpu
@pytest.mark.parametrize("cols", LADDER + WAVE_WIDTHS)
def test_static_absmax_clamps_and_keeps_its_buffer(cols):
    """k in [-300, 300] against a given absmax of 127 2^e in fp32 and fp16 buffers: codes clip(k, -128, 127), the sum over the clipped
    codes, the absmax buffer bit-unchanged.  Inside the window the 16-bit rows must take the general kernel: the wave kernel would
    ignore the given absmax and overwrite it."""
    report([f for dt in DTS for vec, with_sum in VECS for f in probe_static(Gpu(), cols, dt, vec, with_sum)])


@gpu
@pytest.mark.parametrize("cols", LADDER)
def test_levels_entry(cols):
    fails = []
    for ni, n in enumerate((1, 7, 31, 127)):
        for fi, floor in enumerate((1e-6, 0.0)):
            for di, dt in enumerate(DTS):
                vec, with_sum = VECS[(ni + fi + di + cols // 8) % 4]
                fails += probe_levels(Gpu(), cols, dt, vec, with_sum, n, floor)
    report(fails)


GELU_GENERAL_WIDTHS = [264, 520, 1032, 1544, 2056, 4104, 6152, 8200, 10248, 12296, 16384]  # one width per form


@gpu
@pytest.mark.parametrize("cols", GELU_GENERAL_WIDTHS + [8712, 8960, 9216])
def test_gelu_exact_by_saturation(cols):
    dts = DTS if cols in GELU_GENERAL_WIDTHS else ["f16", "bf16"]
    report([f for i, dt in enumerate(dts) for vec, with_sum in (VECS[i % 4], VECS[(i + 1) % 4]) for f in probe_gelu_exact(Gpu(), cols, dt, vec, with_sum)])


@gpu
@pytest.mark.parametrize("cols,dt", [(8712, "bf16"), (8712, "f16"), (8960, "bf16"), (8960, "f16"), (9216, "bf16"), (9216, "f16"), (2056, "f32"), (8960, "f32")])
def test_gelu_on_random_rows_bit_for_bit(cols, dt):
    """The pin is the library's own GELU: the fp32 output of the 16-bit GEMM's GELU epilogue on x times a 64 x 64 identity (exact
    pre-activation), then kr.quant_sum.  fp32 rows hold bf16 values."""
    from viditq_extension import qgemm

    rows = 8
    x16 = torch.from_numpy(random_rows(rows, cols, "bf16" if dt == "f32" else dt, 31) * 0.25).to(TDT["bf16" if dt == "f32" else dt]).to(DEV)
    eye = torch.eye(64, dtype=x16.dtype, device=DEV)
    gel = qgemm.fp_linear(x16.view(-1, 64).contiguous(), eye, None, torch.float32, gelu=True).view(rows, cols)
    q, scale, ssum = kr.quant_sum(gel.cpu().numpy())
    want = Rows(x16.cpu().double().numpy(), q.astype(np.int64), scale.astype(np.float64), ssum.astype(np.float64))
    report(check_int8(Gpu().int8(want.x, dt, "f32", True, act=1), want, "f32", True, f"A7 gelu random {dt} {cols} {kernel_of(dt, cols)}"))


@gpu
@pytest.mark.parametrize("cols", [8712, 8720, 8960, 9216])
def test_wave_kernel_equals_general_kernel(cols):
    report([f for dt in ("bf16", "f16") for act in (0, 1) for f in probe_wave_against_general(Gpu(), cols, dt, act)])


@gpu
@pytest.mark.parametrize("cols", LADDER)
def test_random_rows_equal_the_oracle(cols):
    report([f for dt in DTS for f in probe_random(Gpu(), cols, dt)])


# ================================================================================================ B. fp8 and MX placement (GPU)
@gpu
@pytest.mark.parametrize("cols", LADDER)
def test_fp8_placement(cols):
    report([f for dt in DTS for f in probe_fp8(Gpu(), cols, dt)])


@gpu
@pytest.mark.parametrize("cols", MX_WIDTHS)
def test_mx_placement(cols):
    report([f for dt in DTS for fp4 in (False, True) for f in probe_mx(Gpu(), cols, dt, fp4)])


# ================================================================================================ C. entry rules through the ABI
def _entry_args(entry, rows, cols):
    from viditq_extension import _C

    n, w = max(rows, 1), min(max(cols, 32), 16384) + 32
    x = torch.zeros(n, w, dtype=torch.float32, device=DEV)
    q = torch.full((n, w), U8_SENT, dtype=torch.uint8, device=DEV)
    sc = torch.full((n * (w // 32 + 1),), SENT, dtype=torch.float32, device=DEV)
    sm = torch.full((n,), SENT, dtype=torch.float32, device=DEV)
    p, st, f32 = _C.ptr, _C.stream(), DTC["f32"]
    args = {"wanq_quant_rows": [p(x), f32, p(q), p(sc), p(sm), f32, rows, cols, 0, 0, st],
            "wanq_quant_rows_levels": [p(x), f32, p(q), p(sc), p(sm), f32, rows, cols, 31, 0.0, st],
            "wanq_quant_rows_fp8": [p(x), f32, p(q), p(sc), rows, cols, 0, st],
            "wanq_quant_rows_mx": [p(x), f32, p(q), p(sc), rows, cols, 0, 0, st]}[entry]
    return args, (q, sc, sm), x


def _untouched(outs):
    torch.cuda.synchronize()
    q, sc, sm = outs
    return bool((q == U8_SENT).all()) and bool((sc == SENT).all()) and bool((sm == SENT).all())


QUANT_ENTRIES = ["wanq_quant_rows", "wanq_quant_rows_levels", "wanq_quant_rows_fp8", "wanq_quant_rows_mx"]


@gpu
@pytest.mark.parametrize("entry", QUANT_ENTRIES)
def test_no_rows_is_ok_and_writes_nothing(entry):
    from viditq_extension import _C

    args, outs, keep = _entry_args(entry, 0, 256)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK
    assert _untouched(outs)


@gpu
@pytest.mark.parametrize("entry", QUANT_ENTRIES)
def test_width_rules_are_refused_and_nothing_is_written(entry):
    """cols = 0, 4, 16392 and 16416 (the ladder ends at 16384) return WANQ_E_SHAPE with the rule in the message, and so does a width
    that holds no whole block of 32 for the MX entry; nothing is enqueued."""
    from viditq_extension import _C

    rules = [(c, "must be a multiple of 8 in [8, 16384]") for c in (0, 4, 16392, 16416)]
    if entry == "wanq_quant_rows_mx":
        rules += [(c, "must be a multiple of 32") for c in (8, 2056)]
    for cols, message in rules:
        args, outs, keep = _entry_args(entry, 5, cols)
        assert getattr(_C.lib, entry)(*args) == WANQ_E_SHAPE, (entry, cols)
        text = _C.lib.wanq_last_error().decode()
        assert entry + ":" in text and f"cols={cols}" in text and message in text, text
        assert _untouched(outs), cols


# ================================================================================================ E. the numpy model and its mutants
MUTANTS = ["max_omits_last_wave", "max_omits_last_slot", "max_before_gelu", "store16_at_odd_last_chunk", "pair_chunks_swapped",
           "sum_omits_last_pair", "ties_away_from_zero", "static_wraps", "floor_ignored", "levels_fixed_at_127", "f16_vector_truncated",
           "mx_scale_of_neighbour_block", "e2m1_nibbles_swapped"]


def frame(cols, wpr, nch):
    """RowFrame: chunk [nch, wpr, 64] of (slot i, sub-wave, lane) = sub 64 + lane + i 64 WPR, and whether it lies in the row."""
    i, sub, lane = np.meshgrid(np.arange(nch), np.arange(wpr), np.arange(64), indexing="ij")
    ch = sub * 64 + lane + i * 64 * wpr
    return ch, ch < cols // 8


def gather(x32, ch):
    """RowFrame::load: [rows, nch, wpr, 64, 8]; slots past the row end are zero."""
    rows, cols = x32.shape
    pad = np.zeros((rows, ch.size * 8), F)
    pad[:, :cols] = x32
    return pad.reshape(rows, ch.size, 8)[:, ch]


def scatter(buf, cols, codes, ch, ok, per=8):
    """One `per`-byte store per live chunk at row r cols + chunk 8 (both counted in codes) into the flat buffer."""
    rows = codes.shape[0]
    idx = (np.arange(rows)[:, None, None, None, None] * cols + ch[None, ..., None] * 8) * per // 8 + np.arange(per)[None, None, None, None, :]
    sel = np.broadcast_to(ok[None, ..., None], idx.shape)
    buf[idx[sel]] = codes[sel]


class Model:
    """numpy model of the kernels as written: the row frame (chunk -> slot, sub-wave, lane; per-wave results, then the cross-wave
    max / sum), the wave kernel (pairs of chunks, the clamped re-read, 16-byte and 8-byte stores), stores into FLAT buffers with the
    guard row behind them, the fp32 arithmetic as the contract states it.  `mutant`: one deliberate error."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.kernels = mutant, set()

    # ---- shared pieces
    def _vec(self, a32, vec):
        a32 = np.asarray(a32, F)
        if vec == "f32":
            return a32.astype(np.float64)
        with np.errstate(over="ignore"):
            h = a32.astype(np.float16)
            if self.mutant == "f16_vector_truncated":
                h = np.where(np.abs(h.astype(F)) > np.abs(a32), np.nextafter(h, np.float16(0)), h)
        return h.astype(np.float64)

    def _scale(self, am, levels, floor):
        scale = (am / F(127 if self.mutant == "levels_fixed_at_127" else levels)).astype(F)
        return scale if self.mutant == "floor_ignored" else np.where(scale < F(floor), F(floor), scale).astype(F)

    def _codes(self, v, scale, static):
        s = scale.reshape((-1,) + (1,) * (v.ndim - 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(s > 0, v / s, F(0)).astype(F)
        r = np.where(t < 0, -np.floor(-t + F(0.5)), np.floor(t + F(0.5))) if self.mutant == "ties_away_from_zero" else np.rint(t)
        r = r.astype(np.int64)
        if static and self.mutant != "static_wraps":
            return np.clip(r, -128, 127)
        return ((r + 128) % 256) - 128  # the low byte

    def _vectors(self, rows, scale, tot, vec, with_sum, amax):
        sc, sm = np.full(rows + 1, SENT), np.full(rows + 1, SENT)
        sc[:rows] = self._vec(scale, vec) if amax is None else self._vec(amax, vec)  # (static: the buffer is read, never written)
        if with_sum:
            sm[:rows] = self._vec((tot.astype(F) * scale).astype(F), vec)
        return sc, sm

    # ---- wanq_quant_rows / wanq_quant_rows_levels
    def int8(self, x, dt, vec, with_sum, act=0, amax=None, levels=None, floor=None):
        x32 = rnd(x, dt).astype(F)
        if in_window(dt, x.shape[1]) and amax is None and levels is None:
            return self._wave(x32, vec, with_sum, act)
        if amax is not None:
            amax = self._vec(np.asarray(amax, F), vec).astype(F)  # as the buffer holds it
        return self._general(x32, vec, with_sum, act, amax, 127.0 if levels is None else float(levels), 1e-6 if floor is None else floor)

    def _general(self, x32, vec, with_sum, act, amax, levels, floor):
        rows, cols = x32.shape
        wpr, nch = form_of(cols)
        self.kernels.add(("general", wpr, nch))
        ch, ok = frame(cols, wpr, nch)
        v = gather(x32, ch)
        before = np.abs(v)
        if act:
            v = gelu_np(v)
        if amax is None:
            a = before if self.mutant == "max_before_gelu" else np.abs(v)
            if self.mutant == "max_omits_last_slot" and nch > 1:
                a = a[:, : nch - 1]
            per_wave = a.max(axis=(1, 3, 4))  # [rows, wpr]: the wave butterfly
            if self.mutant == "max_omits_last_wave" and wpr == 4:
                per_wave = per_wave[:, :3]
            am = per_wave.max(axis=1)         # the LDS slots
        else:
            am = amax
        scale = self._scale(am.astype(F), levels, floor)
        codes = self._codes(v, scale, amax is not None)
        tot = codes.sum(axis=(1, 3, 4)).sum(axis=1)  # (slots past the row end hold code 0)
        buf = np.full((rows + 1) * cols, SENT8, np.int64)
        scatter(buf, cols, codes, ch, ok)
        sc, sm = self._vectors(rows, scale, tot, vec, with_sum, amax)
        return {"q": buf.reshape(rows + 1, cols), "scale": sc, "sum": sm}

    def _wave(self, x32, vec, with_sum, act, nch=18):
        rows, cols = x32.shape
        last = cols // 8 - 1
        self.kernels.add(("wave", 8 if last % 2 == 0 else 16))
        i, lane = np.arange(nch)[:, None], np.arange(64)[None, :]
        ch = 2 * (lane + 64 * (i >> 1)) + (i & 1)  # [nch, 64]
        ok = ch <= last
        v = x32.reshape(rows, cols // 8, 8)[:, np.minimum(ch, last)]  # a lane past the row end re-reads the last chunk
        before = np.abs(v) * ok[None, :, :, None]
        if act:
            v = gelu_np(v)
        v = np.where(ok[None, :, :, None], v, F(0))
        a = before if self.mutant == "max_before_gelu" else np.abs(v)
        if self.mutant == "max_omits_last_slot":
            a = a[:, : nch - 1]
        scale = self._scale(a.max(axis=(1, 2, 3)).astype(F), 127.0, 1e-6)
        codes = self._codes(v, scale, False)
        tot = (codes[:, : nch - 2] if self.mutant == "sum_omits_last_pair" else codes).sum(axis=(1, 2, 3))
        buf = np.full((rows + 1) * cols, SENT8, np.int64)
        for r in range(rows):  # rows in order: what a store past the row end leaves in the next row is overwritten there
            for h in range(nch // 2):
                pa, pb = codes[r, 2 * h], codes[r, 2 * h + 1]  # [64, 8]
                if self.mutant == "pair_chunks_swapped":
                    pa, pb = pb, pa
                c0 = 2 * (np.arange(64) + 64 * h)
                wide = (c0 <= last) if self.mutant == "store16_at_odd_last_chunk" else (c0 + 1 <= last)
                narrow = ~wide & (c0 <= last)
                dst = r * cols + c0[:, None] * 8 + np.arange(8)[None, :]
                buf[dst[wide | narrow]] = pa[wide | narrow]
                buf[dst[wide] + 8] = pb[wide]
        sc, sm = self._vectors(rows, scale, tot, vec, with_sum, None)
        return {"q": buf.reshape(rows + 1, cols), "scale": sc, "sum": sm}

    # ---- wanq_quant_rows_fp8
    def fp8(self, x, dt):
        x32 = rnd(x, dt).astype(F)
        rows, cols = x32.shape
        wpr, nch = form_of(cols)
        ch, ok = frame(cols, wpr, nch)
        v = gather(x32, ch)
        scale = np.maximum(np.abs(v).max(axis=(1, 3, 4)).max(axis=1) / F(448), F(1e-6)).astype(F)
        t = np.clip(v / scale[:, None, None, None, None], F(-448), F(448)).astype(F)
        codes = torch.from_numpy(t).to(torch.float8_e4m3fn).view(torch.uint8).numpy().astype(np.int64)
        buf = np.full((rows + 1) * cols, U8_SENT, np.int64)
        scatter(buf, cols, codes, ch, ok)
        return {"q": buf.reshape(rows + 1, cols), "scale": np.concatenate([scale.astype(np.float64), [SENT]])}

    # ---- wanq_quant_rows_mx
    def mx(self, x, dt, fp4):
        x32 = rnd(x, dt).astype(F)
        rows, cols = x32.shape
        wpr, nch = form_of(cols)
        ch, ok = frame(cols, wpr, nch)
        v = gather(x32, ch)
        m = np.abs(v).max(axis=4)                                                  # the lane's chunk
        m = np.repeat(m.reshape(rows, nch, wpr, 16, 4).max(axis=4), 4, axis=3)     # the aligned quad: one block of 32
        s = np.clip(((m.astype(F).view(np.uint32) >> 23) & 0xFF).astype(np.int64) - (2 if fp4 else 8), 0, 254)
        t = np.ldexp(v, (127 - s)[..., None]).astype(F)
        sbuf = np.full((rows + 1) * (cols // 32), SCALE_SENT, np.int64)
        first = np.broadcast_to((ok & (np.arange(64) % 4 == 0))[None], s.shape)
        block = np.broadcast_to(np.arange(rows)[:, None, None, None] * (cols // 32) + ch[None] // 4, s.shape)
        if self.mutant == "mx_scale_of_neighbour_block":
            sbuf[block[first]] = np.roll(s, -4, axis=3)[first]  # (the quad past the row end has s = 0)
        else:
            sbuf[block[first]] = s[first]
        if fp4:
            a = np.minimum(np.abs(t), F(6))
            mag = ((a > 0.25).astype(np.int64) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
            code = mag | (np.signbit(t).astype(np.int64) << 3)
            order = np.arange(8) ^ 1 if self.mutant == "e2m1_nibbles_swapped" else np.arange(8)
            code = code[..., order]
            packed = code[..., 0::2] | (code[..., 1::2] << 4)  # the dword's four bytes, low first
            buf = np.full((rows + 1) * (cols // 2), U8_SENT, np.int64)
            scatter(buf, cols, packed, ch, ok, per=4)
            return {"q": buf.reshape(rows + 1, cols // 2), "scale": sbuf.reshape(rows + 1, cols // 32)}
        codes = torch.from_numpy(np.clip(t, F(-448), F(448))).to(torch.float8_e4m3fn).view(torch.uint8).numpy().astype(np.int64)
        buf = np.full((rows + 1) * cols, U8_SENT, np.int64)
        scatter(buf, cols, codes, ch, ok)
        return {"q": buf.reshape(rows + 1, cols), "scale": sbuf.reshape(rows + 1, cols // 32)}


def model_battery(run):
    """The probes of the GPU tests at the widths that tell the mutants apart -> {probe name: failures}."""
    out = {}

    def add(name, fails):
        out[name] = out.get(name, []) + fails

    for cols, dt in ((8, "f32"), (520, "bf16"), (1544, "f16"), (2056, "f32"), (8200, "f32"), (8704, "bf16"), (8712, "bf16"), (8960, "f16"), (9216, "bf16"), (16384, "f16")):
        for vec, with_sum in (("f32", True), ("f16", True), ("f32", False)):
            add(f"A1 placement {dt} {cols} vec={vec} sum={with_sum}", probe_placement(run, cols, dt, vec, with_sum))
        add(f"A2 walk {dt} {cols}", probe_walk(run, cols, dt, "f32"))
        add(f"A3 ties {dt} {cols}", probe_ties(run, cols, dt, "f32", True))
        add(f"A4 static {dt} {cols}", probe_static(run, cols, dt, "f16" if cols == 8960 else "f32", True))
    add("A3 ties and neighbours f32 2056", probe_ties(run, 2056, "f32", "f32", True, neighbours=True))
    for n in (1, 7, 127):
        for floor in (1e-6, 0.0):
            add(f"A5 levels n={n} floor={floor}", probe_levels(run, 1032, "f32", "f32", True, n, floor) + probe_levels(run, 4104, "bf16", "f16", True, n, floor))
    for cols, dt in ((264, "f32"), (6152, "bf16"), (8712, "f16"), (8960, "bf16")):
        add(f"A6 gelu exact {dt} {cols}", probe_gelu_exact(run, cols, dt, "f32", True))
    for cols in (8712, 8960):
        add(f"A8 wave against general {cols}", probe_wave_against_general(run, cols, "bf16", 0) + probe_wave_against_general(run, cols, "f16", 1))
    for cols, dt in ((264, "f16"), (2056, "f32"), (8712, "bf16")):
        add(f"A9 random {dt} {cols}", probe_random(run, cols, dt))
    for cols, dt in ((8, "f32"), (2056, "bf16"), (14344, "f16")):
        add(f"B fp8 {dt} {cols}", probe_fp8(run, cols, dt))
    for cols, dt in ((32, "f32"), (544, "f16"), (2080, "bf16"), (14368, "f32")):
        for fp4 in (False, True):
            add(f"B mx {'e2m1' if fp4 else 'e4m3'} {dt} {cols}", probe_mx(run, cols, dt, fp4))
    return out


# what each mutant must fail at the least (a substring of the probe's name), and probes it must NOT fail
MUTANT_FAILS = {
    "max_omits_last_wave": ("A2 walk f32 2056", "A2 walk f16 16384", "A2 walk bf16 8704"),
    "max_omits_last_slot": ("A2 walk bf16 520", "A2 walk f32 2056", "A2 walk bf16 8712", "A2 walk f16 8960"),
    "max_before_gelu": ("A6 gelu exact f32 264", "A6 gelu exact bf16 6152", "A6 gelu exact f16 8712", "A6 gelu exact bf16 8960"),
    "store16_at_odd_last_chunk": ("A1 placement bf16 8712", "A2 walk bf16 8712", "A6 gelu exact f16 8712", "A9 random bf16 8712"),
    "pair_chunks_swapped": ("A1 placement bf16 8712", "A1 placement f16 8960", "A8 wave against general 8960"),
    "sum_omits_last_pair": ("A1 placement bf16 8712 vec=f32 sum=True", "A1 placement f16 8960 vec=f32 sum=True", "A9 random bf16 8712"),
    "ties_away_from_zero": ("A3 ties f32 8", "A3 ties bf16 8712", "A3 ties and neighbours f32 2056", "A5 levels n=1 floor=0.0"),
    "static_wraps": ("A4 static f32 8", "A4 static f16 8960", "A4 static f16 16384"),
    "floor_ignored": ("A5 levels n=1 floor=1e-06", "A5 levels n=7 floor=1e-06", "A5 levels n=127 floor=1e-06"),
    "levels_fixed_at_127": ("A5 levels n=1 floor=1e-06", "A5 levels n=7 floor=0.0"),
    "f16_vector_truncated": ("A1 placement bf16 520 vec=f16", "A1 placement f16 16384 vec=f16", "A5 levels n=7 floor=1e-06"),
    "mx_scale_of_neighbour_block": ("B mx e4m3 f32 32", "B mx e2m1 f16 544", "B mx e4m3 f32 14368"),
    "e2m1_nibbles_swapped": ("B mx e2m1 f32 32", "B mx e2m1 bf16 2080"),
}
MUTANT_PASSES = {
    "max_omits_last_wave": ("A2 walk bf16 520", "A2 walk bf16 8712", "B"),
    "max_before_gelu": ("A1", "A2", "A9"),
    "store16_at_odd_last_chunk": ("8960", "9216", "8704", "A4", "B"),
    "pair_chunks_swapped": ("A1 placement bf16 8704", "A4", "A5"),
    "sum_omits_last_pair": ("sum=False", "A2 walk bf16 8704", "A4"),
    "static_wraps": ("A1", "A3", "A5"),
    "floor_ignored": ("floor=0.0", "A1", "A4"),
    "levels_fixed_at_127": ("A5 levels n=127", "A1", "A4"),
    "f16_vector_truncated": ("vec=f32", "A2", "A3"),
    "mx_scale_of_neighbour_block": ("A", "B fp8"),
    "e2m1_nibbles_swapped": ("B mx e4m3", "B fp8", "A"),
}
MUTANT_NOTES = {
    "store16_at_odd_last_chunk": "seen by the guard row alone: the 16 bytes of an earlier row's last pair land in the next row's first chunk, which that row stores itself",
    "max_omits_last_wave": "the four-wave forms only; the one-wave forms and the wave kernel have no cross-wave step",
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_named_probes(mutant):
    failed = {k: v for k, v in model_battery(Model(mutant)).items() if v}
    print(f"MUTANT {mutant}: fails {sorted(failed)}")
    for want in MUTANT_FAILS[mutant]:
        assert any(want in k for k in failed), (mutant, want, sorted(failed))
    for keep in MUTANT_PASSES.get(mutant, ()):
        assert not any(k.startswith(keep) or f" {keep}" in k for k in failed), (mutant, keep, sorted(failed))
    if mutant == "store16_at_odd_last_chunk":
        assert all("guard row" in f for v in failed.values() for f in v)


def test_model_passes_every_probe_and_reaches_both_kernels():
    run = Model()
    failed = {k: v for k, v in model_battery(run).items() if v}
    assert not failed, failed
    assert {("wave", 8), ("wave", 16), ("general", 1, 1), ("general", 4, 5), ("general", 4, 8)} <= run.kernels


def test_width_tables_reach_every_form():
    """Every (WPR, NCH) form at its smallest and largest width for all four entries, both store branches of the wave kernel, both
    sides of both edges of its window, and the static form outside the wave kernel."""
    for widths, step in ((LADDER, 8), (MX_WIDTHS, 32)):
        lo = 0
        for limit, wpr, nch in FORMS:
            mine = [w for w in widths if lo < w // 8 <= limit]
            assert limit * 8 in mine and min(mine) <= (lo * 8 // step + 1) * step, (wpr, nch, mine)
            assert all(form_of(w) == (wpr, nch) and kernel_of("f32", w) == ("general", wpr, nch) for w in mine)
            lo = limit
    assert all(w % 32 == 0 for w in MX_WIDTHS) and 8 in LADDER and 32 in MX_WIDTHS
    assert sorted(form_of(w) for w in GELU_GENERAL_WIDTHS) == sorted((wpr, nch) for _, wpr, nch in FORMS)
    for dt in ("bf16", "f16"):
        assert [kernel_of(dt, w) for w in WAVE_WIDTHS] == [("general", 4, 5), ("wave", 8), ("wave", 16), ("wave", 16), ("wave", 8), ("wave", 16), ("general", 4, 5)]
        assert all(kernel_of(dt, w, static=True)[0] == "general" and kernel_of(dt, w, levels=True)[0] == "general" for w in WAVE_WIDTHS)
    assert all(kernel_of("f32", w) == ("general", 4, 5) for w in WAVE_WIDTHS)
    assert 8704 + 8 == 8712 and 9216 + 8 == 9224  # the window's edges are neighbours in steps of one chunk
    for kernel, cols in ((("wave", 8), 8712), (("wave", 16), 9216), (("general", 4, 8), 14344), (("general", 1, 1), 8)):
        at = walk_positions(kernel, cols)
        assert {0, cols - 1} <= set(at) and len(at) % 4 == 1
    at = {c // 8 for c in walk_positions(("wave", 8), 8712)}
    assert any(c % 2 for c in at) and 1088 in at and all(any(2 * 64 * h <= c < 2 * 64 * (h + 1) for c in at) for h in range(9))
    at = {c // 8 for c in walk_positions(("general", 4, 8), 14344)}
    assert all(any(i * 256 <= c < (i + 1) * 256 for c in at) for i in range(8)) and {0, 63, 64, 127, 128, 191, 192, 255} <= at


def test_generators_refuse_rows_without_an_exact_expectation():
    place_rows(5, 264, "bf16", "f16")
    with pytest.raises(ValueError):  # 2^12 127 overflows fp16
        place_rows(5, 264, "f16", "f32", e=np.full(5, 12))
    with pytest.raises(ValueError):  # amax / 127 = 2^-22 lies below the floor: the codes are not k
        place_rows(5, 264, "f32", "f32", e=np.full(5, -22))
    with pytest.raises(ValueError):  # 129 2^e is no multiple of 7: the scale is not a power of two
        finish(np.full((1, 8), 129.0), np.full((1, 8), 7), np.array([129.0 / 7]), np.array([56 * 129.0 / 7]), "f32", "probe", 7, 0.0)
    with pytest.raises(ValueError):  # 8 bits and a half: a tie at 300.5 is not a bf16 number
        finish(np.full((1, 8), 300.5), np.full((1, 8), 127), np.array([300.5 / 127]), np.array([0.0]), "bf16", "probe")
    for dt in DTS:
        for vec in ("f32", "f16"):
            for rows in (static_rows(5, 520, dt, vec), tie_rows(5, 520, dt, vec), gelu_rows(5, 520, dt, vec)):
                assert np.array_equal(rnd(rows.x, dt), rows.x)
                assert np.array_equal(vec_round(rows.scale, vec), rows.scale)
        for fp4 in (False, True):
            assert np.array_equal(rnd(mx_rows(5, 544, dt, fp4).x, dt), mx_rows(5, 544, dt, fp4).x)
        assert np.array_equal(rnd(fp8_rows(5, 520, dt).x, dt), fp8_rows(5, 520, dt).x)


def test_gelu_is_exact_from_the_stated_threshold():
    """The numpy restatement of gelu_tanh_fast_f32: x for x >= 16, -0 for x <= -16, over every bf16 and fp16 value in the probe's range
    and at the threshold itself; below 8 it is not exact (the probe would not be one there)."""
    x = np.concatenate([np.arange(16.0, 32768.0, 8.0), [16.0, 16.125, 65504.0, 3.0e38]])
    assert np.array_equal(gelu_np(x), x.astype(F))
    g = gelu_np(-x)
    assert (g == 0).all() and np.signbit(g).all()
    assert gelu_np(np.array([4.0]))[0] != 4.0 and gelu_np(np.array([-4.0]))[0] != 0.0
    with pytest.raises(ValueError):
        gelu_rows(5, 264, "f32", "f32", scale_from_all=True)  # an absmax taken before the activation is another scale


def mutant_table_text():
    lines = ["Mutants of the numpy model in tests/test_gpu_quant_rows_probes.py (Model) and the probes that catch them",
             "=" * 105, "",
             "The model restates the row quantisers of csrc/rowwise.hip as written (the row frame, the wave kernel's pairs and stores, flat",
             "buffers with their guard row, the fp32 arithmetic); each mutant is one deliberate error in it.",
             "test_mutants_of_the_model_fail_named_probes runs the probes of the GPU tests on every mutant, on a machine without a GPU, and",
             "asserts for each the probes named below (substrings of the names in model_battery); test_mutant_table_is_the_committed_one",
             "keeps this file equal to the table asserted there.", ""]
    for m in MUTANTS:
        lines.append(m)
        lines += [f"    fails   {p}" for p in MUTANT_FAILS[m]]
        lines += [f"    passes  {p}" for p in MUTANT_PASSES.get(m, ())]
        if m in MUTANT_NOTES:
            lines.append(f"    note    {MUTANT_NOTES[m]}")
    return "\n".join(lines) + "\n"


def test_mutant_table_is_the_committed_one():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quant_rows_probe_mutants.txt")
    with open(path) as f:
        assert f.read() == mutant_table_text()
    assert set(MUTANT_FAILS) == set(MUTANTS) and all(MUTANT_FAILS[m] for m in MUTANTS)


def test_gpu_part_is_marked():
    """Every test above section E asks for a GPU; nothing below does."""
    import sys

    mod = sys.modules[__name__]
    cpu = {"test_mutants_of_the_model_fail_named_probes", "test_model_passes_every_probe_and_reaches_both_kernels", "test_width_tables_reach_every_form",
           "test_generators_refuse_rows_without_an_exact_expectation", "test_gelu_is_exact_from_the_stated_threshold", "test_mutant_table_is_the_committed_one",
           "test_gpu_part_is_marked"}
    for name, fn in vars(mod).items():
        if name.startswith("test_") and callable(fn):
            marked = any(m.name == "gpu" for m in getattr(fn, "pytestmark", []))
            assert marked != (name in cpu), name


if __name__ == "__main__":  # PYTHONPATH=. python tests/test_gpu_quant_rows_probes.py > profiles/quant_rows_probe_mutants.txt
    print(mutant_table_text(), end="")
