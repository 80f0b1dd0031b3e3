"""The PTQ tool kernels (csrc/quant_tools.hip: wanq_col_absmax, wanq_row_minmax, wanq_weight_quant, wanq_weight_export_f16,
wanq_fake_quant_cols, wanq_fake_quant_with_delta, wanq_pack_w4, wanq_unpack_w4) on operands whose answer is known bit for bit.  Every call
goes through the C ABI and the test owns every buffer: each output AND each input is a window inside a flat byte allocation with
GUARD bytes in front and behind.  An output allocation holds the byte 0xA5 everywhere before every launch and its guards must still
hold it afterwards; an input allocation holds 0x7B around the data (a huge finite value in all three types, so that a read past a
row or a matrix shows in a maximum) and must come back unchanged.

  A  exact probes: planted extrema for the two statistics kernels; for the quantisers operands that are exact by construction
     (delta a power of two, w = (k + f) delta, f in quarters) next to random data against the numpy restatement; the nibble
     layout; the second turn of every grid-stride loop.
  C  empty and refused calls through the ABI leave every window untouched and name the rule.
  E  CPU self-tests (not marked gpu): a numpy model of the kernels as written passes A and C, nineteen mutants of it (one of them provably equivalent) are run against the
     probes (profiles/quant_tools_probe_mutants.txt), the tables' coverage and the exactness of every constructed operand are proved.

Why equality everywhere: max and min are order independent, and every other kernel here is a chain of single IEEE fp32 operations
with no add after a multiply (nothing contracts into an fma); the library is built with -O3 and no fast-math flag, so its fp32
division is the correctly rounded one.  The numpy float32 / float16 restatement, operation by operation (np.rint ties to even, true
division), must therefore give the same bits, and a 16-bit output is the fp32 result rounded once, to nearest even.

Kernel rules restated here (csrc/quant_tools.hip, csrc/row_frame.h):
  row frame     chunks = cols / 8 <= 256: row_minmax_kernel<1, 4>, one wave per row, ceil(rows / 4) workgroups, a surplus wave of the
                last one returns; else <4, 8>, one workgroup per row.  Slot i of lane l of wave `sub` is chunk sub 64 + l + i 64 WPR
  col_absmax    panels = ceil(cols / 512); slabs = max(2048 / panels, 1); rpb = max(ceil(rows / slabs), 64); grid (panels,
                ceil(rows / rpb)); wave w reads rows r0 + w + 4 t, four at a time while r + 12 < r1; one atomic max per column
  grid-stride   chunk ch = block 256 + thread + turn gridDim 256, gridDim = min(ceil(total / 256), cap); cap 8192 (weight_quant,
                weight_export_f16, fake_quant_cols, fake_quant_with_delta), 4096 (pack_w4, unpack_w4); row = ch / (cols / 8)
  nibbles       per 32 codes 16 bytes (P0a, P1a, P0b, P1b); P0 byte i = u[i] | u[4 + i] << 4, P1 byte i = u[8 + i] | u[12 + i] << 4."""
import collections
import functools
import os

import numpy as np
import pytest
import torch

# The GPU part (sections A and C) is marked test by test, so that section E below runs without a GPU; test_gpu_part_is_marked keeps
# a test added above section E from being left unmarked.
gpu = pytest.mark.gpu
DEV = "cuda"
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
DTC = {"f16": 0, "bf16": 1, "f32": 2}  # WANQ_F16 / BF16 / F32 (include/wanq_hip.h)
DTS = ("f16", "bf16", "f32")
NPT = {"f16": np.float16, "bf16": np.uint16, "f32": np.float32}  # storage types; bf16 is kept as its 16 bits
GUARD = 65536  # bytes; a multiple of 16, so every window stays 16-byte aligned; one row of the widest shape (16384 fp32 columns), so
# that a read of the row behind a matrix, or of the rows of three surplus waves (cols <= 2048), stays inside the test's own allocation
OUT_FILL, IN_FILL = 0xA5, 0x7B  # 0x7B7B.. is 61280 (f16), 1.3e36 (bf16, f32): finite and above every probe value
F32 = np.float32
FRACS = (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75)
CAP8, CAP32 = 8192, 4096

Res = collections.namedtuple("Res", "rc msg wins fails reads")


# ================================================================================================ number formats
def bf16_bits(a32):
    """fp32 -> the 16 bits of the nearest bf16, ties to even (finite values)."""
    u = np.ascontiguousarray(a32, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def enc(a, dt):
    """Values -> the storage array of type dt: one rounding from fp32, to nearest even."""
    a32 = np.ascontiguousarray(a, F32)
    return a32.astype(np.float16) if dt == "f16" else bf16_bits(a32) if dt == "bf16" else a32


def dec(s, dt):
    """Storage array -> fp32 (exact)."""
    if dt == "bf16":
        return (np.ascontiguousarray(s, np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)
    return np.ascontiguousarray(s).astype(F32)


def exact_in(a64, dt):
    a64 = np.asarray(a64, np.float64)
    with np.errstate(over="ignore"):  # beyond fp16's range: inf, which is not the value
        return dec(enc(a64.astype(F32), dt), dt).astype(np.float64) == a64


def hash32(r, c, salt):
    """A fixed integer hash of (r, c): uint64 array of values below 2^32."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(r, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(c, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(salt * 0x27D4EB2F + 1)) & m
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h = h ^ (h >> np.uint64(12))
    h = (h * np.uint64(0x297A2D39)) & m
    return h ^ (h >> np.uint64(15))


def hidx(rows, cols, salt, n):
    return (hash32(np.arange(rows)[:, None], np.arange(cols)[None, :], salt) % np.uint64(n)).astype(np.int64)


def rint_away(x):
    """Round half away from zero: what a mutant does in place of rint."""
    t = np.trunc(x)
    return np.where(np.abs(x - t) == 0.5, t + np.sign(x), np.rint(x)).astype(x.dtype)


# ================================================================================================ the arithmetic, restated in numpy
# One function per kernel body, fp32 operation by operation.  `mut` names a deliberate error: only the model's mutants pass one.
def wq_math(v, d, z, qmin, qmax, mut=None):
    """weight_quant: t = rint(w / d) - z; the loose clamp; int8 saturation on top; deq = (t + z) d.  -> (int8 codes, fp32 deq)"""
    with np.errstate(all="ignore"):
        r = (rint_away if mut == "ties_away" else np.rint)(v / d)
        t = r + z if mut == "plus_zp" else r - z
        if mut != "loose_clamp_dropped":
            t = np.minimum(np.maximum(t, F32(qmin)), F32(qmax))
        qi = np.minimum(np.maximum(t, F32(-128)), F32(127))
        deq = ((qi if mut == "deq_from_saturated_code" else t) + z) * d
    return np.nan_to_num(qi).astype(np.int8), deq.astype(F32)


def f16r(a):
    return np.asarray(a).astype(np.float16).astype(F32)


def export_math(v, d, z, mut=None):
    """weight_export_f16: fl16(w), fl16(fl32(w16 / d)), fl16(rint(q) - z), clamp.  d, z: fp32 values of the fp16 parameters."""
    with np.errstate(all="ignore"):
        w16 = v if mut == "export_weight_not_rounded_first" else f16r(v)
        if mut == "export_quotient_rounded_once":
            quo = f16r(w16.astype(np.float64) / d.astype(np.float64))
        else:
            quo = f16r(w16 / d)
        r = (rint_away if mut == "ties_away" else np.rint)(quo)
        t = f16r(r + z if mut == "plus_zp" else r - z)
        return np.nan_to_num(np.minimum(np.maximum(t, F32(-128)), F32(127))).astype(np.int8)


def fqc_math(v, m, nlev, mut=None):
    """fake_quant_cols: d = m / nlev floored at 1e-6; clamp(rint(v / d), -nlev - 1, nlev) d."""
    nlev = F32(nlev)
    with np.errstate(all="ignore"):
        d = m / nlev
        if mut != "colmax_floor_missing":
            d = np.where(d < F32(1e-6), F32(1e-6), d)
        xi = (rint_away if mut == "ties_away" else np.rint)(v / d)
        return (np.minimum(np.maximum(xi, -nlev - F32(1)), nlev) * d).astype(F32)


def fqd_math(v, d, bits, n_bits, mut=None):
    """fake_quant_with_delta.  Plain: d' = max(d, 1e-6) / (2^b - 1); clamp(rint(v / d'), 0, 2^b - 1) d', where everything at or below
    zero gives +0.0 (include/wanq_hip.h).  With a bits map: levels 2^bits - 1 per element, clipped from above only, 0 bits -> +0.0."""
    rint = rint_away if mut == "ties_away" else np.rint
    with np.errstate(all="ignore"):
        dj = np.where(d < F32(1e-6), F32(1e-6), d).astype(F32)
        if bits is None:
            lev = F32(2 ** n_bits - 1)
            dj = dj / lev
            xi = rint(v / dj)
            return (np.where(xi > 0, np.minimum(xi, lev), F32(0)) * dj).astype(F32)
        zero = bits == 0
        nl = np.where(zero, 255, 2.0 ** bits - 1).astype(F32)
        dj = dj / nl
        xi = rint(v / dj)
        y = (np.where(xi > nl, nl, xi) * dj).astype(F32)
        return y if mut == "bits0_not_masked" else np.where(zero, F32(0), y)


def pack_ref(q, bias):
    """The documented layout (include/wanq_hip.h) restated, as _pack_w4_ref of tests/test_gpu_gemm.py: u = (e + bias) mod 16."""
    N, K = q.shape
    u = ((q.astype(np.int32) + bias) & 15).reshape(N, K // 16, 16)
    p0 = u[:, :, 0:4] | (u[:, :, 4:8] << 4)
    p1 = u[:, :, 8:12] | (u[:, :, 12:16] << 4)
    return np.concatenate([p0, p1], axis=2).reshape(N, K // 2).astype(np.uint8)


def unpack_ref(p, bias):
    N, K2 = p.shape
    b = p.reshape(N, K2 // 8, 2, 4).astype(np.int32)  # [half of 16 codes][P0 | P1][byte i]
    u = np.stack([b[:, :, 0] & 15, b[:, :, 0] >> 4, b[:, :, 1] & 15, b[:, :, 1] >> 4], axis=2)  # codes i, 4 + i, 8 + i, 12 + i
    return (u.reshape(N, K2 * 2) - bias).astype(np.int8)


# ================================================================================================ buffers and checkers
class Win:
    """`nbytes` inside a flat byte allocation with GUARD bytes in front and behind (and up to the next multiple of 16), all preset
    to `fill`; `data` (any numpy array) is copied into the window."""

    def __init__(self, nbytes, dev, fill, data=None):
        self.n, self.fill, self.dev = int(nbytes), fill, dev
        self.t = torch.full((2 * GUARD + (self.n + 15) // 16 * 16,), fill, dtype=torch.uint8, device=dev)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).ravel()
            assert raw.size == self.n
            self.t[GUARD:GUARD + self.n] = torch.from_numpy(raw.copy()).to(dev)
        self.before = None if data is None else np.ascontiguousarray(data).view(np.uint8).ravel().copy()
        self._host = None

    def ptr(self):
        p = self.t.data_ptr() + GUARD
        assert p % 16 == 0
        return p

    def host(self):
        if self.dev == "cpu":
            return self.t.numpy()
        if self._host is None:
            self._host = self.t.cpu().numpy()
        return self._host

    def get(self, npt, count=None):
        w = self.host()[GUARD:GUARD + self.n].view(npt)
        return w if count is None else w[:count]


def guard_failures(win, what):
    h = win.host()
    fails = []
    front, back = h[:GUARD] != win.fill, h[GUARD + win.n:] != win.fill
    if front.any():
        fails.append(f"the guard in front of {what} was written at byte {int(np.nonzero(front)[0][-1]) - GUARD}")
    if back.any():
        fails.append(f"the guard behind {what} was written at byte {win.n + int(np.nonzero(back)[0][0])}")
    return fails


def untouched(res):
    """Every output window still holds the sentinel, every input its data, every guard its fill."""
    fails = list(res.fails)
    for name, w in res.wins.items():
        fails += guard_failures(w, name)
        if w.before is None and (w.get(np.uint8) != w.fill).any():
            fails.append(f"{name} was written")
    return fails


def check(res, name, want, describe=None):
    """Bit equality of window `name` with `want` (a numpy array of the stored type), guards intact, nothing written behind `want`.
    describe(flat index) adds what the probe knows about the first bad element."""
    win = res.wins[name]
    fails = list(res.fails) + guard_failures(win, name)
    want = np.ascontiguousarray(want)
    ut = {1: np.uint8, 2: np.uint16, 4: np.uint32}[want.dtype.itemsize]
    got, wb = win.get(ut, want.size), want.view(ut).ravel()
    bad = got != wb
    if (win.get(np.uint8)[want.nbytes:] != win.fill).any():
        fails.append(f"{name} was written behind its {want.size} elements")
    if bad.any():
        sent = ut(int.from_bytes(bytes([win.fill]) * want.dtype.itemsize, "little"))
        i = int(np.nonzero(bad)[0][0])
        more = "" if describe is None else "; " + describe(i)
        fails.append(f"{name}: {int(bad.sum())} of {want.size} elements differ ({int((bad & (got == sent)).sum())} of them never written); first at "
                     f"{i}: got {win.get(want.dtype, want.size)[i]!r} expected {want.ravel()[i]!r}{more}")
    return fails


# argument order of include/wanq_hip.h: P pointers by name (None = NULL), S scalars
ABI = {
    "wanq_row_minmax": lambda P, S, st: (P["w"], S["dt"], P["rmin"], P["rmax"], P["rabs"], S["rows"], S["cols"], st),
    "wanq_col_absmax": lambda P, S, st: (P["x"], S["dt"], P["colmax"], S["rows"], S["cols"], st),
    "wanq_weight_quant": lambda P, S, st: (P["w"], S["dt"], P["delta"], P["zp"], S["qmin"], S["qmax"], P["q8"], P["deq"], S["rows"], S["cols"], st),
    "wanq_weight_export_f16": lambda P, S, st: (P["w"], S["dt"], P["delta"], P["zp"], P["q8"], S["rows"], S["cols"], st),
    "wanq_fake_quant_cols": lambda P, S, st: (P["x"], S["dt"], P["colmax"], P["out"], S["odt"], S["n_bits"], S["rows"], S["cols"], st),
    "wanq_fake_quant_with_delta": lambda P, S, st: (P["x"], S["dt"], P["delta"], P["bits"], P["out"], S["odt"], S["n_bits"], S["n"], st),
    "wanq_pack_w4": lambda P, S, st: (P["q"], P["packed"], S["bias"], S["rows"], S["cols"], st),
    "wanq_unpack_w4": lambda P, S, st: (P["packed"], P["q"], S["bias"], S["rows"], S["cols"], st),
}


def make_windows(dev, ins, outs):
    """ins: name -> array | None (a NULL pointer).  outs: name -> byte count | None (NULL) | (byte count, initial array) | the name of
    an input (in place)."""
    wins = {k: Win(v.nbytes, dev, IN_FILL, v) for k, v in ins.items() if v is not None}
    for k, v in outs.items():
        if isinstance(v, str):
            wins[k] = wins[v]
        elif isinstance(v, tuple):
            wins[k] = Win(v[0], dev, OUT_FILL, v[1])
        elif v is not None:
            wins[k] = Win(v, dev, OUT_FILL)
    return wins


def input_failures(wins, ins, outs):
    alias = {v for v in outs.values() if isinstance(v, str)}
    fails = []
    for k in ins:
        if k in wins and k not in alias:
            fails += guard_failures(wins[k], f"input {k}")
            if not np.array_equal(wins[k].get(np.uint8), wins[k].before):
                fails.append(f"input {k} was written")
    return fails


class GpuRun:
    """One launch per call through the C ABI on fresh windows."""
    dev, mutant = DEV, None

    def call(self, entry, ins, outs, **S):
        from viditq_extension import _C

        wins = make_windows(DEV, ins, outs)
        P = {k: (wins[k].ptr() if k in wins else None) for k in list(ins) + list(outs)}
        rc = getattr(_C.lib, entry)(*ABI[entry](P, S, _C.stream()))
        torch.cuda.synchronize()
        msg = _C.lib.wanq_last_error().decode() if rc != WANQ_OK else ""
        return Res(rc, msg, wins, input_failures(wins, ins, outs), None)


def ok(res):
    return [] if res.rc == WANQ_OK else [f"returned {res.rc}: {res.msg}"]


# ================================================================================================ A1. wanq_row_minmax
RM_WIDTHS = (8, 64, 128, 520, 2048, 2056, 5120, 8960, 13824, 16384)
RM_ROWS = (1, 3, 5, 6, 9)  # 3, 1, 3, 2, 3 surplus waves in the last workgroup of the one-wave form
RM_KINDS = ("mixed", "positive", "negative", "equal", "absmax from the minimum", "zeros")
RM_OUTS = ("rmin", "rmax", "rabs")


def rm_form(cols):
    return (1, 4) if cols // 8 <= 256 else (4, 8)


def rm_launches(rows, cols):
    """Launches per (rows, cols): enough for every 512-column stripe (one chunk slot of one wave) to hold a planted extremum although
    two of the six row kinds plant none (twice round the stripes; test_tables_reach_every_case proves what is reached), and two at
    the least."""
    return max(-(-2 * (-(-cols // 512)) // rows), 2)


def rm_plan(rows, cols, j):
    """(kind, column of the minimum, column of the maximum) of every row of launch j: row r takes stripe t = r J + j (mod the stripe
    count) for its minimum and the stripe half way round for its maximum, at hashed places inside the stripe."""
    nst, J = -(-cols // 512), rm_launches(rows, cols)
    plan = []
    for r in range(rows):
        t = r * J + j
        smin, smax = t % nst, (t + max(1, nst // 2)) % nst
        cmin = smin * 512 + int(hash32(r, j, 41)) % min(512, cols - smin * 512)
        cmax = smax * 512 + int(hash32(r, j, 42)) % min(512, cols - smax * 512)
        if cmax == cmin:
            cmax = smax * 512 + (cmax - smax * 512 + 1) % min(512, cols - smax * 512)
        plan.append((RM_KINDS[(r + j) % 6], cmin, cmax))
    return plan


def rm_case(rows, cols, j):
    """float64 [rows, cols], every value n 2^e with |n| < 256 (exact in f16, bf16 and f32); no -0.0.  The planted values differ per row."""
    m = hidx(rows, cols, 43 + j, 129).astype(np.float64)  # 0 .. 128
    x = np.zeros((rows, cols))
    for r, (kind, cmin, cmax) in enumerate(rm_plan(rows, cols, j)):
        if kind == "mixed":
            x[r] = (m[r] - 64) / 64
            x[r, cmin], x[r, cmax] = -(130 + r) / 64, (140 + r) / 64
        elif kind == "positive":
            x[r] = (128 + m[r] % 32) / 32
            x[r, cmin], x[r, cmax] = (96 + r) / 32, (192 + r) / 32
        elif kind == "negative":
            x[r] = -(128 + m[r] % 32) / 32
            x[r, cmin], x[r, cmax] = -(192 + r) / 32, -(96 + r) / 32
        elif kind == "equal":
            x[r] = (100 + r) / 32 * (1 if r % 2 else -1)
        elif kind == "absmax from the minimum":
            x[r] = (m[r] - 64) / 64
            x[r, cmin], x[r, cmax] = -(128 + r) / 16, (140 + r) / 64
    return x + 0.0


def probe_row_minmax(run, rows, cols, dt, j, outs=RM_OUTS):
    x = rm_case(rows, cols, j)
    w = enc(x, dt)
    v = dec(w, dt).reshape(rows, cols)
    want = {"rmin": v.min(1), "rmax": v.max(1), "rabs": np.abs(v).max(1)}
    res = run.call("wanq_row_minmax", {"w": w}, {k: (rows * 4 if k in outs else None) for k in RM_OUTS}, dt=DTC[dt], rows=rows, cols=cols)
    fails = ok(res)
    plan = rm_plan(rows, cols, j)

    def describe(i):
        kind, cmin, cmax = plan[i]
        wpr = rm_form(cols)[0]
        place = lambda c: f"col {c} (wave {(c // 8 % (64 * wpr)) // 64 if wpr == 4 else i % 4}, slot {c // 8 // (64 * wpr)}, lane {c // 8 % 64})"  # noqa: E731
        return f"row {i} ({kind}): minimum at {place(cmin)}, maximum at {place(cmax)}"

    for k in outs:
        if not fails:
            fails += check(res, k, want[k].astype(F32), describe)
    return fails


def rm_table(dt):
    """(rows, cols, j, outputs): every launch asks for all three outputs; a second launch of the same data asks for one alone."""
    cases = []
    for cols in RM_WIDTHS:
        for rows in RM_ROWS:
            for j in range(rm_launches(rows, cols)):
                cases += [(rows, cols, j, RM_OUTS), (rows, cols, j, (RM_OUTS[(j + rows + DTS.index(dt)) % 3],))]
    return cases


@gpu
@pytest.mark.parametrize("dt", DTS)
def test_row_minmax_finds_planted_extrema_in_every_slot(dt):
    run, fails = GpuRun(), []
    for rows, cols, j, outs in rm_table(dt):
        fails += [f"({rows}, {cols}) launch {j} outputs {outs}: {f}" for f in probe_row_minmax(run, rows, cols, dt, j, outs)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ A2. wanq_col_absmax
# rows: fewer than waves and one more; the four-deep loop's bound (12, 13, 15 and 28 are the lengths at which `r + 12 < r1` and
# `r + 12 <= r1` part: the latter reads the row behind the slab); a second slab of one row; one slab longer than 64 rows
CA_ROWS = (1, 3, 4, 5, 12, 13, 15, 16, 17, 20, 28, 64, 65, 129)
CA_WIDTHS = (8, 512, 520, 1536)
CA_LONG = (140000, 8)


def ca_slabs(rows, cols):
    """The host rule: (row slabs, rows per slab)."""
    panels = -(-cols // 512)
    slabs = max(2048 // panels, 1)
    rpb = max(-(-rows // slabs), 64)
    return -(-rows // rpb), rpb


def ca_stride(rows, cols):
    return -(-rows // min(cols, rows))


def ca_masked(cols, j):
    """The columns whose prefill lies above the column maximum in launch j: c % 3 == 0 in even launches, c % 3 == 2 in odd ones.
    Launches 2 i and 2 i + 1 plant the same rows, so every planted maximum stands once on a column whose prefill lies below it."""
    return (np.arange(cols) + j % 2) % 3 == 0


def ca_launches(rows, cols):
    """Two launches (the two sets of masked columns) per row offset; the long shape takes three in all."""
    return 2 * ca_stride(rows, cols) if rows <= 129 else 3


def ca_rows_of_max(rows, cols, j):
    """The row that holds column c's maximum in launch j: (a c + j) % rows with a = ceil(rows / min(cols, rows)), so that over the
    row offsets j // 2 every row holds one.  The long shape: the first and last rows of slabs instead (first, second, last but one,
    last slab)."""
    c = np.arange(cols)
    if rows <= 129:
        return (ca_stride(rows, cols) * c + j // 2) % rows
    slabs, rpb = ca_slabs(rows, cols)
    slab = np.array([0, 1, slabs - 2, slabs - 1, 0, 1, slabs - 2, slabs - 1])[c % 8] if j < 2 else (c * 251 + 7) % slabs
    r0 = slab * rpb
    r1 = np.minimum(r0 + rpb, rows)
    return np.where(c % 8 < 4, r0, r1 - 1) if j == 0 else np.where(c % 8 < 4, r1 - 1, r0) if j == 1 else np.minimum(r0 + 64 + c % 5, r1 - 1)


def ca_case(rows, cols, j):
    """x in [-1, 1] (multiples of 1/64), column c's maximum +-(128 + c % 64) / 32 in [4, 6), negative on odd columns, in one row;
    prefill: 7 + c % 5 (above the maximum) on the columns of ca_masked (every third, moving with the launch), (c % 5) / 4 (below
    it) elsewhere."""
    x = (hidx(rows, cols, 51 + j, 129).astype(np.float64) - 64) / 64
    c = np.arange(cols)
    rmax = ca_rows_of_max(rows, cols, j)
    x[rmax, c] = (128 + c % 64) / 32 * np.where(c % 2, -1.0, 1.0)
    prefill = np.where(ca_masked(cols, j), 7.0 + c % 5, (c % 5) / 4)
    return x + 0.0, prefill.astype(F32), rmax


def probe_col_absmax(run, rows, cols, dt, j):
    x, prefill, rmax = ca_case(rows, cols, j)
    w = enc(x, dt)
    want = np.maximum(prefill, np.abs(dec(w, dt).reshape(rows, cols)).max(0))
    res = run.call("wanq_col_absmax", {"x": w}, {"colmax": (cols * 4, prefill)}, dt=DTC[dt], rows=rows, cols=cols)
    _, rpb = ca_slabs(rows, cols)
    fails = ok(res) or check(res, "colmax", want.astype(F32), lambda c: f"column {c}: its maximum is in row {rmax[c]} (slab {rmax[c] // rpb}, row "
                                                                         f"{rmax[c] % rpb} of it, wave {rmax[c] % rpb % 4}); prefill {prefill[c]}")
    if res.reads is not None and res.reads != rows:  # the model counts the rows its waves read: each row once
        fails.append(f"model: the waves read {res.reads} rows of {rows}")
    return fails


def ca_table():
    return [(rows, cols) for rows in CA_ROWS for cols in CA_WIDTHS] + [CA_LONG]


@gpu
@pytest.mark.parametrize("dt", DTS)
def test_col_absmax_reads_every_row_and_keeps_a_larger_prefill(dt):
    run, fails = GpuRun(), []
    for rows, cols in ca_table():
        for j in range(ca_launches(rows, cols)):
            fails += [f"({rows}, {cols}) launch {j}: {f}" for f in probe_col_absmax(run, rows, cols, dt, j)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ A3. wanq_weight_quant / wanq_weight_export_f16
# (rows, cols): every width of the issue with a partial last workgroup (rows cols / 8 is no multiple of 256); (3075, 64) and
# (1027, 128) are the group-wise shape [N K / g, g]
WQ_SHAPES = ((37, 8), (3075, 64), (1027, 128), (5, 1536), (3, 8960))
WQ_CLAMPS = ((-257, 256), (-17, 16), (-128, 127))  # 8-bit and 4-bit asymmetric (the reference's loose clamp), 8-bit symmetric


def row_params(rows):
    """Per-row delta = 2^-(2 + r % 7) and zp = (37 r) % 41 - 20: neighbouring rows differ in both."""
    r = np.arange(rows)
    return (2.0 ** -(2 + r % 7)).astype(F32), ((37 * r) % 41 - 20).astype(F32)


def wq_exact_case(rows, cols, dt, qmin, qmax, salt=0):
    """w = (k + f) delta with k - zp within 3 of qmin, -128, 0, 127 and qmax, f in quarters; an element that the input type cannot
    hold takes the nearest even integer k instead.  -> (stored w, delta, zp, k + f as float64)"""
    delta, zp = row_params(rows)
    E = np.array(sorted({a + i + f for a in (qmin, -128, 0, 127, qmax) for i in range(-3, 4) for f in FRACS}))
    kf = zp[:, None].astype(np.float64) + E[hidx(rows, cols, 61 + salt, len(E))]
    kf = np.where(exact_in(kf, dt), kf, 2 * np.rint(kf / 2)) + 0.0
    w64 = kf * delta[:, None].astype(np.float64)
    assert exact_in(kf, dt).all() and exact_in(w64, dt).all()
    return enc(w64, dt), delta, zp, kf


def wq_closed_form(kf, delta, zp, qmin, qmax):
    """The definition on exact operands, in float64: every step is exact."""
    t = np.clip(np.rint(kf) - zp[:, None], qmin, qmax)
    return np.clip(t, -128, 127).astype(np.int8), ((t + zp[:, None]) * delta[:, None]).astype(F32)


def wq_random_case(rows, cols, dt, salt=0):
    """Random weights with the delta a real 8-bit asymmetric quantiser gives them: (max - min) / 255, zp = rint(-min / delta) - 128...
    shifted per row so that some rows clip."""
    rng = np.random.default_rng(600 + salt + rows + cols)
    w = enc(rng.standard_normal((rows, cols)).astype(F32) * F32(0.04) * (1 + np.arange(rows)[:, None] % 3).astype(F32), dt)
    v = dec(w, dt).reshape(rows, cols)
    delta = ((v.max(1) - v.min(1)) / F32(255) * (F32(0.7) + F32(0.1) * (np.arange(rows) % 4).astype(F32))).astype(F32)
    zp = np.rint(v.min(1) / delta).astype(F32) + F32(128)
    return w, delta, zp


def describe_rc(cols, extra=None):
    return lambda i: f"row {i // cols} col {i % cols} (chunk {i // 8}, workgroup {i // 8 // 256})" + ("" if extra is None else extra(i))


def call_wq(run, w, dt, delta, zp, qmin, qmax, rows, cols, q8=True, deq=True):
    return run.call("wanq_weight_quant", {"w": w, "delta": delta, "zp": zp}, {"q8": rows * cols if q8 else None, "deq": rows * cols * 4 if deq else None},
                    dt=DTC[dt], qmin=qmin, qmax=qmax, rows=rows, cols=cols)


def probe_weight_quant_exact(run, rows, cols, dt, qmin, qmax, q8=True, deq=True):
    w, delta, zp, kf = wq_exact_case(rows, cols, dt, qmin, qmax)
    q_want, d_want = wq_closed_form(kf, delta, zp, qmin, qmax)
    q_re, d_re = wq_math(dec(w, dt).reshape(rows, cols), delta[:, None], zp[:, None], qmin, qmax)
    assert np.array_equal(q_re, q_want) and np.array_equal(d_re.view(np.uint32), d_want.view(np.uint32))  # the restatement IS the definition
    res = call_wq(run, w, dt, delta, zp, qmin, qmax, rows, cols, q8, deq)
    fails = ok(res)
    more = lambda i: f": k + f = {kf.ravel()[i]}, zp {zp[i // cols]}, delta {delta[i // cols]}"  # noqa: E731
    if q8 and not fails:
        fails += check(res, "q8", q_want, describe_rc(cols, more))
    if deq and not fails:
        fails += check(res, "deq", d_want, describe_rc(cols, more))
    return fails


def probe_weight_quant_random(run, rows, cols, dt):
    w, delta, zp = wq_random_case(rows, cols, dt)
    q_want, d_want = wq_math(dec(w, dt).reshape(rows, cols), delta[:, None], zp[:, None], -257, 256)
    res = call_wq(run, w, dt, delta, zp, -257, 256, rows, cols)
    return ok(res) or check(res, "q8", q_want, describe_rc(cols)) + check(res, "deq", d_want, describe_rc(cols))


@gpu
@pytest.mark.parametrize("dt", DTS)
def test_weight_quant_codes_and_dequantised_values_bit_for_bit(dt):
    run, fails = GpuRun(), []
    for si, (rows, cols) in enumerate(WQ_SHAPES):
        for ci, (qmin, qmax) in enumerate(WQ_CLAMPS):
            for q8, deq in ((True, True), (True, False), (False, True)) if (si + ci) % 3 == 0 else ((True, True),):
                fails += [f"exact ({rows}, {cols}) clamp ({qmin}, {qmax}) q8 {q8} deq {deq}: {f}"
                          for f in probe_weight_quant_exact(run, rows, cols, dt, qmin, qmax, q8, deq)]
        fails += [f"random ({rows}, {cols}): {f}" for f in probe_weight_quant_random(run, rows, cols, dt)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@functools.lru_cache(maxsize=None)
def near_midpoint_pairs():
    """fp16 pairs (a, b) with a / b in [1024, 2047) (fp16 spacing 1) whose exact quotient lies as close to k + 1/2 as two 11-bit
    operands allow: with a = A 2^i, b = B 2^j the distance is a multiple of 1 / (2 B) >= 2^-12.  That is four fp32 roundings at this
    magnitude, so fl32(a / b) is never the midpoint itself unless the quotient is, and fl16(fl32(a / b)) == fl16(a / b) for EVERY fp16
    pair (24 >= 2 11 + 2 bits: double rounding is innocuous for a quotient): the mutant that rounds the exact quotient once is
    equivalent, which test_constructed_operands_are_exact_and_hit_every_edge checks on all 1536 x 512 pairs searched here.  The pairs
    stay in the probe: they are where a division that is not correctly rounded has the least room.
    float64 division stands for the exact quotient.  -> (a, b, the number of pairs on which one rounding and two differ)"""
    b = ((1024 + np.arange(1, 1024, 2)) / 1024 * 2.0 ** -7).astype(np.float16)
    a = np.arange(8, 32, 2.0 ** -6)[:, None].astype(np.float16)
    q64 = a.astype(np.float64) / b.astype(np.float64)[None, :]
    q32 = a.astype(F32) / b.astype(F32)[None, :]
    differ = int((q64.astype(np.float16) != q32.astype(np.float16)).sum())
    near = (np.abs(q64 - np.floor(q64) - 0.5) < 2.0 ** -11.5) & (q64 >= 1024) & (q64 < 2047)
    ia, ib = np.nonzero(near)
    return a[ia, 0].astype(np.float64), b[ib].astype(np.float64), differ


def export_case(rows, cols, dt):
    """Random weights (fp32 ones carry 24 significant bits, so fl16(w) moves them), a sixth of them tripled so that codes saturate at
    both ends; per row an fp16 delta that is no power of two and an fp16 integer zp.  For f16 and f32 weights the first elements of a
    row are near-midpoint pairs, that row's delta their b and its zp near their quotient."""
    rng = np.random.default_rng(700 + rows + cols)
    r = np.arange(rows)
    w = rng.standard_normal((rows, cols)).astype(F32) * F32(0.05)
    w = np.where(hidx(rows, cols, 71, 6) == 0, w * 3, w)
    delta = (F32(0.3) / 255 * (1 + (r % 5) / 7)).astype(np.float16)
    zp = ((37 * r) % 41 - 20).astype(np.float16)
    planted = 0
    if dt != "bf16":
        a, b, _ = near_midpoint_pairs()
        for i in range(min(max(rows // 3, 1), len(a))):  # every third row, so that the random rows stay
            row = min(3 * i + 1, rows - 1)
            delta[row], zp[row] = b[i], np.rint(a[i] / b[i]) - (i % 7 - 3)
            sel = np.nonzero(b == b[i])[0]
            w[row, :min(cols, len(sel))] = a[sel][:cols]
            planted += 1
    return enc(w, dt), delta, zp, planted


def probe_weight_export(run, rows, cols, dt):
    w, delta, zp, _ = export_case(rows, cols, dt)
    want = export_math(dec(w, dt).reshape(rows, cols), delta.astype(F32)[:, None], zp.astype(F32)[:, None])
    res = run.call("wanq_weight_export_f16", {"w": w, "delta": delta, "zp": zp}, {"q8": rows * cols}, dt=DTC[dt], rows=rows, cols=cols)
    return ok(res) or check(res, "q8", want, describe_rc(cols, lambda i: f": w {dec(w, dt).ravel()[i]!r} delta {delta[i // cols]!r} zp {zp[i // cols]!r}"))


@gpu
@pytest.mark.parametrize("dt", DTS)
def test_weight_export_f16_rounds_where_half_precision_torch_does(dt):
    run, fails = GpuRun(), []
    for rows, cols in WQ_SHAPES:
        fails += [f"({rows}, {cols}): {f}" for f in probe_weight_export(run, rows, cols, dt)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ A4. the two fake-quantisers
FQC_SHAPES = ((37, 8), (9, 520), (3, 1536))  # 37, 585 and 576 chunks: a partial last workgroup each
FQC_BITS = (2, 4, 6, 8)
FQD_NS = (8, 8 * (256 + 3), 8 * (512 + 3))
FQD_BITS = (2, 8, 16)
BITMAP = np.array([0, 2, 4, 8, 16], np.int32)


def edge_grid(anchors, dt, lo=-1e30, hi=1e30):
    """k + f for k within 3 of every anchor, f in quarters: those the type dt holds exactly."""
    E = np.array(sorted({a + i + f for a in anchors for i in range(-3, 4) for f in FRACS}))
    E = E[(E >= lo) & (E <= hi)]
    return E[exact_in(E, dt)] + 0.0


def fqc_case(rows, cols, xdt, n_bits, salt=0):
    """Columns by c % 4: 0, 1: colmax = nlev 2^e (d = 2^e exactly), x = (k + f) d with k around -nlev - 1, 0 and nlev; 2: random x
    with an arbitrary colmax; 3: colmax = 0 or 1e-7 nlev (the floor), x a few 1e-6."""
    nlev = 2 ** (n_bits - 1) - 1
    c = np.arange(cols)
    e = -(c % 5).astype(np.float64) - 1
    E = edge_grid((-nlev - 1, 0, nlev), xdt)
    rng = np.random.default_rng(800 + rows + cols + n_bits + salt)
    x = E[hidx(rows, cols, 81 + salt, len(E))] * 2.0 ** e[None, :]
    colmax = (nlev * 2.0 ** e).astype(F32)
    rnd = rng.standard_normal((rows, cols))
    x = np.where(c % 4 == 2, rnd, x)
    colmax = np.where(c % 4 == 2, np.abs(rnd).max(0) * 0.9, colmax).astype(F32)
    x = np.where(c % 4 == 3, rnd * 3e-6, x)
    colmax = np.where(c % 4 == 3, np.where(c % 8 == 3, 0.0, 1e-7 * nlev), colmax).astype(F32)
    return enc(x, xdt), colmax, nlev, E


def probe_fq_cols(run, rows, cols, xdt, odt, n_bits, inplace=False):
    x, colmax, nlev, _ = fqc_case(rows, cols, xdt, n_bits)
    y = fqc_math(dec(x, xdt).reshape(rows, cols), colmax[None, :], nlev)
    res = run.call("wanq_fake_quant_cols", {"x": x, "colmax": colmax}, {"out": "x" if inplace else rows * cols * NPT[odt]().itemsize},
                   dt=DTC[xdt], odt=DTC[odt], n_bits=n_bits, rows=rows, cols=cols)
    return ok(res) or check(res, "out", enc(y, odt), describe_rc(cols, lambda i: f": x {dec(x, xdt).ravel()[i]!r} colmax {colmax[i % cols]!r}"))


@gpu
@pytest.mark.parametrize("n_bits", FQC_BITS)
def test_fake_quant_cols_all_type_pairs_and_in_place(n_bits):
    run, fails = GpuRun(), []
    for rows, cols in FQC_SHAPES:
        for xdt in DTS:
            for odt in DTS:
                fails += [f"({rows}, {cols}) {xdt} -> {odt}: {f}" for f in probe_fq_cols(run, rows, cols, xdt, odt, n_bits)]
            fails += [f"({rows}, {cols}) {xdt} in place: {f}" for f in probe_fq_cols(run, rows, cols, xdt, xdt, n_bits, True)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


def fqd_case(n, xdt, n_bits, with_bits, salt=0):
    """Elements by i % 4: 0, 1: delta = levels 2^e (d' = 2^e exactly), x = (k + f) d' with k around 0 and levels; 2: random x and
    delta; 3: delta below the 1e-6 floor (0 or 1e-7).  With a bits map the levels are those of the element's own bit-width."""
    i = np.arange(n)
    bits = BITMAP[hidx(1, n, 91 + salt, 5)[0]] if with_bits else None
    b = np.where(bits == 0, 8, bits) if with_bits else np.full(n, n_bits)
    lev = 2.0 ** b - 1
    e = -(i % 5).astype(np.float64) - 1
    grids = {bb: edge_grid((0, 2 ** bb - 1), xdt) for bb in set(b.tolist())}
    kf = np.array([grids[bb][h % len(grids[bb])] for bb, h in zip(b.tolist(), hidx(1, n, 92 + salt, 1 << 20)[0].tolist())])
    rng = np.random.default_rng(900 + n + n_bits + salt)
    rnd, rd = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    x = np.where(i % 4 == 2, rnd, np.where(i % 4 == 3, rnd * 3e-6, kf * 2.0 ** e))
    delta = np.where(i % 4 == 2, rd, np.where(i % 4 == 3, np.where(i % 8 == 3, 0.0, 1e-7), lev * 2.0 ** e)).astype(F32)
    return enc(x, xdt), delta, bits


def probe_fq_delta(run, n, xdt, odt, n_bits, with_bits, inplace=False):
    x, delta, bits = fqd_case(n, xdt, n_bits, with_bits)
    y = fqd_math(dec(x, xdt), delta, bits, n_bits)
    res = run.call("wanq_fake_quant_with_delta", {"x": x, "delta": delta, "bits": bits}, {"out": "x" if inplace else n * NPT[odt]().itemsize},
                   dt=DTC[xdt], odt=DTC[odt], n_bits=n_bits, n=n)
    more = lambda i: f": x {dec(x, xdt)[i]!r} delta {delta[i]!r}" + ("" if bits is None else f" bits {bits[i]}")  # noqa: E731
    return ok(res) or check(res, "out", enc(y, odt), lambda i: f"chunk {i // 8}" + more(i))


@gpu
@pytest.mark.parametrize("mode", ["2", "8", "16", "map"])
def test_fake_quant_with_delta_all_type_pairs(mode):
    run, fails = GpuRun(), []
    n_bits, with_bits = (8, True) if mode == "map" else (int(mode), False)
    for n in FQD_NS:
        for xdt in DTS:
            for odt in DTS:
                fails += [f"n {n} {xdt} -> {odt}: {f}" for f in probe_fq_delta(run, n, xdt, odt, n_bits, with_bits)]
            fails += [f"n {n} {xdt} in place: {f}" for f in probe_fq_delta(run, n, xdt, xdt, n_bits, with_bits, True)]
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ A5. the nibble layout
W4_SHAPES = ((17, 32), (17, 64), (3, 8960))  # 17, 34 and 840 groups of 32: a partial last workgroup each


def w4_codes(rows, cols, bias):
    """u = (r + 5 position + 3 group) % 16: every nibble value in every one of the 32 positions (over rows or over groups), and group g
    differs from group 0 by 3 g."""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return ((r + 5 * (c % 32) + 3 * (c // 32)) % 16 - bias).astype(np.int8)


def probe_w4(run, rows, cols, bias):
    q = w4_codes(rows, cols, bias)
    p_want = pack_ref(q, bias)
    assert np.array_equal(unpack_ref(p_want, bias), q)
    where = lambda per: lambda i: f"row {i // per} group {i % per // (per // (cols // 32))} (group {i // (per // (cols // 32))} of the matrix)"  # noqa: E731
    res = run.call("wanq_pack_w4", {"q": q}, {"packed": rows * cols // 2}, bias=bias, rows=rows, cols=cols)
    fails = ok(res) or check(res, "packed", p_want, where(cols // 2))
    res = run.call("wanq_unpack_w4", {"packed": p_want}, {"q": rows * cols}, bias=bias, rows=rows, cols=cols)
    fails += ok(res) or check(res, "q", q, where(cols))
    # arbitrary bytes: unpack, then pack what came out: the same bytes
    p = (hidx(rows, cols // 2, 95 + bias, 256)).astype(np.uint8)
    res = run.call("wanq_unpack_w4", {"packed": p}, {"q": rows * cols}, bias=bias, rows=rows, cols=cols)
    fails += ok(res) or check(res, "q", unpack_ref(p, bias), where(cols))
    if not fails:
        res2 = run.call("wanq_pack_w4", {"q": res.wins["q"].get(np.int8).reshape(rows, cols).copy()}, {"packed": rows * cols // 2}, bias=bias, rows=rows, cols=cols)
        fails += ok(res2) or check(res2, "packed", p, where(cols // 2))
    return fails


@gpu
@pytest.mark.parametrize("bias", [0, 8])
def test_w4_pack_and_unpack_follow_the_documented_layout(bias):
    run, fails = GpuRun(), []
    for rows, cols in W4_SHAPES:
        fails += [f"({rows}, {cols}): {f}" for f in probe_w4(run, rows, cols, bias)]
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ A6. the second turn of every grid-stride loop
BIG8 = (2049, 8192)    # rows cols / 8 = 8192 * 256 + 1024 chunks
BIG32 = (2049, 16384)  # rows cols / 32 = 4096 * 256 + 512 groups
BIG_N = 8 * (CAP8 * 256 + 3)


def second_turn(fails, res, name, want, first):
    """The failures of check(), and separately how many elements of the second turn (flat index >= first) still hold the sentinel."""
    fails = fails + check(res, name, want)
    ut = {1: np.uint8, 2: np.uint16, 4: np.uint32}[want.dtype.itemsize]
    sent = ut(int.from_bytes(bytes([OUT_FILL]) * want.dtype.itemsize, "little"))
    got, wb = res.wins[name].get(ut, want.size)[first:], want.view(ut).ravel()[first:]
    never = int(((got == sent) & (wb != sent)).sum())
    if never:
        fails.append(f"{name}: {never} of the {want.size - first} elements of the second turn were never written")
    return fails


def probe_big(run, kernel):
    rows, cols = BIG32 if "w4" in kernel else BIG8
    first = (CAP32 * 256 * 32) if "w4" in kernel else CAP8 * 256 * 8
    if kernel == "weight_quant":
        w, delta, zp = wq_random_case(rows, cols, "f16")
        q_want, d_want = wq_math(dec(w, "f16").reshape(rows, cols), delta[:, None], zp[:, None], -257, 256)
        res = call_wq(run, w, "f16", delta, zp, -257, 256, rows, cols)
        return second_turn(second_turn(ok(res), res, "q8", q_want, first), res, "deq", d_want, first)
    if kernel == "weight_export_f16":
        w, delta, zp, _ = export_case(rows, cols, "bf16")
        want = export_math(dec(w, "bf16").reshape(rows, cols), delta.astype(F32)[:, None], zp.astype(F32)[:, None])
        res = run.call("wanq_weight_export_f16", {"w": w, "delta": delta, "zp": zp}, {"q8": rows * cols}, dt=DTC["bf16"], rows=rows, cols=cols)
        return second_turn(ok(res), res, "q8", want, first)
    if kernel == "fake_quant_cols":
        x, colmax, nlev, _ = fqc_case(rows, cols, "f16", 8)
        y = fqc_math(dec(x, "f16").reshape(rows, cols), colmax[None, :], nlev)
        res = run.call("wanq_fake_quant_cols", {"x": x, "colmax": colmax}, {"out": rows * cols * 2}, dt=0, odt=0, n_bits=8, rows=rows, cols=cols)
        return second_turn(ok(res), res, "out", enc(y, "f16"), first)
    if kernel == "fake_quant_with_delta":
        rng = np.random.default_rng(99)
        x, delta = enc(rng.standard_normal(BIG_N).astype(F32), "f16"), rng.uniform(0.5, 2.0, BIG_N).astype(F32)
        y = fqd_math(dec(x, "f16"), delta, None, 8)
        res = run.call("wanq_fake_quant_with_delta", {"x": x, "delta": delta, "bits": None}, {"out": BIG_N * 2}, dt=0, odt=0, n_bits=8, n=BIG_N)
        return second_turn(ok(res), res, "out", enc(y, "f16"), first)
    q = w4_codes(rows, cols, 8)
    if kernel == "pack_w4":
        res = run.call("wanq_pack_w4", {"q": q}, {"packed": rows * cols // 2}, bias=8, rows=rows, cols=cols)
        return second_turn(ok(res), res, "packed", pack_ref(q, 8), first // 2)
    res = run.call("wanq_unpack_w4", {"packed": pack_ref(q, 8)}, {"q": rows * cols}, bias=8, rows=rows, cols=cols)
    return second_turn(ok(res), res, "q", q, first)


BIG_KERNELS = ("weight_quant", "weight_export_f16", "fake_quant_cols", "fake_quant_with_delta", "pack_w4", "unpack_w4")


@gpu
@pytest.mark.parametrize("kernel", BIG_KERNELS)
def test_grid_stride_loop_takes_its_second_turn(kernel):
    fails = probe_big(GpuRun(), kernel)
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ C. empty and refused calls
def edge_calls(empty):
    """(name, entry, ins, outs, scalars, expected code, a piece of the message).  empty: rows = 0 / n = 0 on otherwise valid calls."""
    R, C = 4, 64
    w, v4 = np.ones((R, C), F32), np.ones(R, F32)
    h4, q, p, cm = np.ones(R, np.float16), np.ones((R, C), np.int8), np.ones((R, C // 2), np.uint8), np.ones(C, F32)
    base = {
        "wanq_row_minmax": ({"w": w}, {"rmin": 16, "rmax": 16, "rabs": 16}, dict(dt=2, rows=R, cols=C)),
        "wanq_col_absmax": ({"x": w}, {"colmax": C * 4}, dict(dt=2, rows=R, cols=C)),
        "wanq_weight_quant": ({"w": w, "delta": v4, "zp": v4}, {"q8": R * C, "deq": R * C * 4}, dict(dt=2, qmin=-128, qmax=127, rows=R, cols=C)),
        "wanq_weight_export_f16": ({"w": w, "delta": h4, "zp": h4}, {"q8": R * C}, dict(dt=2, rows=R, cols=C)),
        "wanq_fake_quant_cols": ({"x": w, "colmax": cm}, {"out": R * C * 4}, dict(dt=2, odt=2, n_bits=8, rows=R, cols=C)),
        "wanq_fake_quant_with_delta": ({"x": w, "delta": w, "bits": None}, {"out": R * C * 4}, dict(dt=2, odt=2, n_bits=8, n=R * C)),
        "wanq_pack_w4": ({"q": q}, {"packed": R * C // 2}, dict(bias=8, rows=R, cols=C)),
        "wanq_unpack_w4": ({"packed": p}, {"q": R * C}, dict(bias=8, rows=R, cols=C)),
    }
    if empty:
        return [(f"{e} empty", e, i, o, {**s, **({"n": 0} if "n" in s else {"rows": 0})}, WANQ_OK, "") for e, (i, o, s) in base.items()]

    def var(entry, name, code, piece, ins=None, outs=None, **s):
        i, o, sc = base[entry]
        return (f"{entry}: {name}", entry, {**i, **(ins or {})}, {**o, **(outs or {})}, {**sc, **s}, code, piece)

    out = []
    for e in ("wanq_row_minmax", "wanq_weight_quant", "wanq_weight_export_f16"):  # the row-frame entries
        out += [var(e, "cols % 8", WANQ_E_SHAPE, "multiple of 8", cols=60), var(e, "cols > 16384", WANQ_E_SHAPE, "16384", cols=16392),
                var(e, "dtype 3", WANQ_E_ARG, "bad dtype", dt=3), var(e, "NULL w", WANQ_E_ARG, "NULL pointer", ins={"w": None})]
    out += [var("wanq_row_minmax", "all three outputs NULL", WANQ_E_ARG, "NULL pointer", outs={"rmin": None, "rmax": None, "rabs": None}),
            var("wanq_weight_quant", "qmin >= qmax", WANQ_E_ARG, "bad clamp range", qmin=5, qmax=5),
            var("wanq_weight_quant", "both outputs NULL", WANQ_E_ARG, "NULL pointer", outs={"q8": None, "deq": None}),
            var("wanq_weight_quant", "NULL zp", WANQ_E_ARG, "NULL pointer", ins={"zp": None}),
            var("wanq_weight_export_f16", "NULL delta", WANQ_E_ARG, "NULL pointer", ins={"delta": None}),
            var("wanq_weight_export_f16", "NULL q8", WANQ_E_ARG, "NULL pointer", outs={"q8": None}),
            var("wanq_col_absmax", "cols % 8", WANQ_E_SHAPE, "multiple of 8", cols=60),
            var("wanq_col_absmax", "dtype -1", WANQ_E_ARG, "bad dtype", dt=-1),
            var("wanq_col_absmax", "NULL colmax", WANQ_E_ARG, "NULL pointer", outs={"colmax": None}),
            var("wanq_fake_quant_cols", "cols % 8", WANQ_E_SHAPE, "multiple of 8", cols=60),
            var("wanq_fake_quant_cols", "n_bits 1", WANQ_E_ARG, "n_bits=1", n_bits=1),
            var("wanq_fake_quant_cols", "n_bits 9", WANQ_E_ARG, "n_bits=9", n_bits=9),
            var("wanq_fake_quant_cols", "out dtype 3", WANQ_E_ARG, "bad dtype", odt=3),
            var("wanq_fake_quant_cols", "NULL colmax", WANQ_E_ARG, "NULL pointer", ins={"colmax": None}),
            var("wanq_fake_quant_with_delta", "n % 8", WANQ_E_SHAPE, "multiple of 8", n=60),
            var("wanq_fake_quant_with_delta", "n_bits 1", WANQ_E_ARG, "n_bits=1", n_bits=1),
            var("wanq_fake_quant_with_delta", "n_bits 17", WANQ_E_ARG, "n_bits=17", n_bits=17),
            var("wanq_fake_quant_with_delta", "x dtype 4", WANQ_E_ARG, "bad dtype", dt=4),
            var("wanq_fake_quant_with_delta", "NULL delta", WANQ_E_ARG, "NULL pointer", ins={"delta": None})]
    for e, o in (("wanq_pack_w4", "packed"), ("wanq_unpack_w4", "q")):
        out += [var(e, "cols % 32", WANQ_E_SHAPE, "multiple of 32", cols=48), var(e, "bias 4", WANQ_E_ARG, "bias must be", bias=4),
                var(e, "NULL output", WANQ_E_ARG, "NULL pointer", outs={o: None})]
    return out


def probe_edge_calls(run, empty):
    fails = []
    for name, entry, ins, outs, S, code, piece in edge_calls(empty):
        res = run.call(entry, ins, outs, **S)
        if res.rc != code or piece not in res.msg:
            fails.append(f"{name}: returned {res.rc} ({res.msg!r}), expected {code} with {piece!r}")
        fails += [f"{name}: {f}" for f in untouched(res)]
    return fails


@gpu
def test_empty_calls_are_ok_and_write_nothing():
    fails = probe_edge_calls(GpuRun(), True)
    assert not fails, "\n".join(fails)


@gpu
def test_refused_calls_name_the_rule_and_write_nothing():
    fails = probe_edge_calls(GpuRun(), False)
    assert not fails, "\n".join(fails)


# ================================================================================================ E. CPU self-tests of the probes
def test_tables_reach_every_case():
    """row_minmax: both forms, <4, 8> at 2056, 5120, 8960, 13824 and 16384; 1 to 3 surplus waves; per width every stripe of 512 columns
    (one chunk slot of one wave) holds a planted minimum and a planted maximum, in a launch that asks for that output; every row
    kind at every width, the all-positive and all-negative rows at ragged widths.  col_absmax: over the launches every row holds a
    column's maximum; both signs; prefill above and below; a slab longer than 64 rows whose ends are probed.  The grid-stride shapes
    end in a partial workgroup, the big ones pass the cap."""
    assert [rm_form(c) for c in RM_WIDTHS] == [(1, 4)] * 5 + [(4, 8)] * 5
    assert {(-r) % 4 for r in RM_ROWS} == {1, 2, 3}  # surplus waves in the last workgroup of the one-wave form
    for dt in DTS:
        table = rm_table(dt)
        for cols in RM_WIDTHS:
            nst = -(-cols // 512)
            seen = {k: set() for k in ("rmin", "rmax")}
            kinds = set()
            for rows, c, j, outs in table:
                if c != cols:
                    continue
                for kind, cmin, cmax in rm_plan(rows, cols, j):
                    kinds.add(kind)
                    assert 0 <= cmin < cols and 0 <= cmax < cols and cmin != cmax
                    if kind in ("mixed", "positive", "negative", "absmax from the minimum"):
                        if "rmin" in outs:
                            seen["rmin"].add(cmin // 512)
                        if "rmax" in outs:
                            seen["rmax"].add(cmax // 512)
            assert seen["rmin"] == set(range(nst)) and seen["rmax"] == set(range(nst)), (dt, cols)
            assert kinds == set(RM_KINDS), (dt, cols, kinds)
        assert {len(o) for _, _, _, o in table} == {1, 3} and {o for _, _, _, o in table if len(o) == 1} == {("rmin",), ("rmax",), ("rabs",)}
    # the last stripe of a ragged width holds fewer than 64 live lanes: 520 -> 1 lane, 2056 -> 1 lane (slot 1 of wave 0), 8960 -> 32
    assert [(c - (-(-c // 512) - 1) * 512) // 8 for c in (520, 2056, 8960)] == [1, 1, 32] and 64 // 8 == 8  # g = 64: 8 live lanes
    x = rm_case(9, 520, 0)
    assert (x[1] > 0).all() and (x[2] < 0).all() and not np.signbit(x[x == 0]).any()
    for rows, cols in ca_table():
        hit = set()
        for j in range(ca_launches(rows, cols)):
            x, prefill, rmax = ca_case(rows, cols, j)
            mx = np.abs(x).max(0)
            hit |= set(rmax[prefill < mx].tolist())  # only a column whose prefill lies below its maximum can tell
            assert (np.abs(x)[rmax, np.arange(cols)] == mx).all() and (np.sort(np.abs(x), 0)[-2] < mx).all() if rows > 1 else True
            assert (prefill > mx).any() and (prefill < mx).any() and (x[rmax, np.arange(cols)] < 0).sum() == cols // 2
        if rows <= 129:
            assert hit == set(range(rows)), (rows, cols)
    slabs, rpb = ca_slabs(*CA_LONG)
    assert rpb == 69 and slabs == 2029 and ca_slabs(129, 8) == (3, 64) and ca_slabs(65, 1536) == (2, 64)
    r0 = set(ca_rows_of_max(*CA_LONG, 0)[~ca_masked(8, 0)].tolist()) | set(ca_rows_of_max(*CA_LONG, 1)[~ca_masked(8, 1)].tolist())
    assert r0 >= {0, rpb - 1, rpb, 2 * rpb - 1, (slabs - 1) * rpb, CA_LONG[0] - 1}
    assert {r % 16 for r in CA_ROWS} >= {12, 13, 15}  # where `r + 12 < r1` and `<=` part
    for rows, cols in WQ_SHAPES + FQC_SHAPES:
        assert (rows * cols // 8) % 256 != 0
    assert {c for _, c in WQ_SHAPES} == {8, 64, 128, 1536, 8960} and {c for _, c in FQC_SHAPES} == {8, 520, 1536}
    assert all((r * c // 32) % 256 for r, c in W4_SHAPES) and {c for _, c in W4_SHAPES} == {32, 64, 8960}
    assert BIG8[0] * BIG8[1] // 8 > CAP8 * 256 and BIG_N // 8 > CAP8 * 256 and BIG32[0] * BIG32[1] // 32 > CAP32 * 256
    assert FQD_NS == (8, 8 * (256 + 3), 8 * (256 * 2 + 3))
    for bias in (0, 8):
        for rows, cols in ((17, 32), (3, 8960)):
            u = w4_codes(rows, cols, bias).astype(int) + bias
            assert u.min() == 0 and u.max() == 15
            for pos in range(32):
                assert set(u[:, pos::32].ravel().tolist()) == set(range(16))
        assert not np.array_equal(w4_codes(17, 64, bias)[:, :32], w4_codes(17, 64, bias)[:, 32:])


def test_gpu_part_is_marked():
    import inspect
    import sys

    first_cpu = inspect.getsourcelines(test_tables_reach_every_case)[1]
    for name, fn in list(vars(sys.modules[__name__]).items()):
        if name.startswith("test_") and inspect.isfunction(fn) and inspect.getsourcelines(fn)[1] < first_cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name


def test_constructed_operands_are_exact_and_hit_every_edge():
    """Every "exact by construction" input is exactly representable in its type (the builders assert it element by element); here:
    what the hashed choice reaches.  weight_quant, per type and clamp over all shapes: both ends of the loose clamp, the int8
    saturation alone (the 8-bit asymmetric clamp only: the other two lie inside int8), halves on even and on odd k.  The statistics
    probes hold only values n 2^e with |n| < 256.  Double-rounding pairs exist and move the exported code."""
    for dt in DTS:
        for qmin, qmax in WQ_CLAMPS:
            got = collections.Counter()
            for rows, cols in WQ_SHAPES:
                w, delta, zp, kf = wq_exact_case(rows, cols, dt, qmin, qmax)
                assert np.array_equal(dec(w, dt).reshape(rows, cols).astype(np.float64), kf * delta[:, None])
                t = np.rint(kf) - zp[:, None]
                half = np.abs(kf - np.trunc(kf)) == 0.5
                got.update(above=int((t > qmax).sum()), below=int((t < qmin).sum()), sat_hi=int(((t > 127) & (t <= qmax)).sum()),
                           sat_lo=int(((t < -128) & (t >= qmin)).sum()), half_even=int((half & (np.floor(kf) % 2 == 0)).sum()),
                           half_odd=int((half & (np.floor(kf) % 2 == 1)).sum()))
            need = ["above", "below", "half_even", "half_odd"] + (["sat_hi", "sat_lo"] if qmax > 127 else [])
            assert all(got[k] >= 8 for k in need), (dt, qmin, got)
        for rows, cols in ((9, 2056), (5, 8)):
            for j in range(2):
                assert exact_in(rm_case(rows, cols, j), dt).all()
        assert exact_in(ca_case(20, 520, 0)[0], dt).all() and exact_in(ca_case(*CA_LONG, 1)[0], dt).all()
        for n_bits in FQC_BITS:  # around both clamp ends and zero, past them by 3
            nlev = 2 ** (n_bits - 1) - 1
            E = fqc_case(9, 520, dt, n_bits)[3]
            assert E.min() <= -nlev - 3 and E.max() >= nlev + 2 and (np.abs(E - np.trunc(E)) == 0.5).any()
        for n_bits in FQD_BITS:
            E = edge_grid((0, 2 ** n_bits - 1), dt)
            assert E.min() <= -3 and (E.max() >= 2 ** n_bits or (dt == "f16" and n_bits == 16))  # past the upper end; fp16 itself ends at 65504 < 2^16 - 1
    a, b, differ = near_midpoint_pairs()
    assert len(a) >= 64 and differ == 0  # one rounding of the exact quotient and fl16(fl32(.)) agree on every pair: an equivalent mutant
    assert (np.abs(a / b - np.floor(a / b) - 0.5) < 2.0 ** -11.5).all()  # the exact quotient lies next to k + 1/2
    for dt in ("f16", "f32"):
        assert export_case(5, 1536, dt)[3] >= 1 and export_case(3075, 64, dt)[3] >= 64
    w = dec(export_case(5, 1536, "f32")[0], "f32")
    assert (f16r(w) != w).mean() > 0.9  # more than 11 significant bits
    for dt in DTS:  # codes saturate at both ends
        w, delta, zp, _ = export_case(1027, 128, dt)
        q = export_math(dec(w, dt).reshape(1027, 128), delta.astype(F32)[:, None], zp.astype(F32)[:, None])
        assert (q == 127).sum() > 50 and (q == -128).sum() > 50 and np.isfinite(dec(w, dt)).all()


# ------------------------------------------------------------------------------------------------ the numpy model and its mutants
MUTANTS = ["absmax_last_slab_r1_off_by_one", "absmax_deep_loop_bound_le", "absmax_wave_stride_3", "second_grid_turn_skipped",
           "row_from_cpr_plus_1", "surplus_wave_writes", "dead_slots_read_as_zero", "wave0_only_reduction", "ties_away",
           "plus_zp", "loose_clamp_dropped", "deq_from_saturated_code", "export_quotient_rounded_once", "export_weight_not_rounded_first",
           "colmax_floor_missing",
           "bits0_not_masked", "nibbles_swapped", "bias_flip_high_nibble_only", "groups_at_stride_32"]
PAD = 1 << 16  # poison behind every operand of the model: what a read past the end returns (NaN), and is counted


class ModelRun:
    """The kernels as written, in numpy: host checks, launch geometry, index arithmetic, and the arithmetic of the restatement above.
    Reads outside an operand are counted, return NaN and are reported as a failure, as a bounds checker would; stores go to the flat
    allocation, so that one outside the window lands in a guard."""
    dev = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.oob, self.reads = mutant, 0, None

    def call(self, entry, ins, outs, **S):
        wins = make_windows("cpu", ins, outs)
        self.oob, self.reads = 0, None
        arr = {k: (None if k not in wins else wins[k]) for k in list(ins) + list(outs)}
        err = self._host_checks(entry, arr, S)
        if err is None and S.get("rows", S.get("n")) != 0:
            getattr(self, "_k_" + entry[5:])(arr, ins, **S)
        rc, msg = err or (WANQ_OK, "")
        fails = input_failures(wins, ins, outs) + ([f"model: {self.oob} elements read outside an operand"] if self.oob else [])
        return Res(rc, msg, wins, fails, self.reads)

    # ---- host side
    def _host_checks(self, entry, A, S):
        name = entry
        need = {"wanq_row_minmax": ["w"], "wanq_col_absmax": ["x", "colmax"], "wanq_weight_quant": ["w", "delta", "zp"],
                "wanq_weight_export_f16": ["w", "delta", "zp", "q8"], "wanq_fake_quant_cols": ["x", "colmax", "out"],
                "wanq_fake_quant_with_delta": ["x", "delta", "out"], "wanq_pack_w4": ["q", "packed"], "wanq_unpack_w4": ["q", "packed"]}[entry]
        if any(A[k] is None for k in need) or (entry == "wanq_row_minmax" and all(A[k] is None for k in RM_OUTS)) or \
                (entry == "wanq_weight_quant" and A["q8"] is None and A["deq"] is None):
            return WANQ_E_ARG, f"{name}: NULL pointer"
        if "w4" in entry:
            if not (S["cols"] >= 32 and S["cols"] % 32 == 0):
                return WANQ_E_SHAPE, f"{name}: cols={S['cols']} must be a multiple of 32"
            if not (S["rows"] >= 0 and S["bias"] in (0, 8)):
                return WANQ_E_ARG, f"{name}: bias must be 0 (unsigned codes) or 8 (signed codes)"
            return None
        if S["dt"] not in (0, 1, 2) or S.get("odt", 0) not in (0, 1, 2):
            return WANQ_E_ARG, f"{name}: bad dtype code"
        if entry == "wanq_weight_quant" and not S["qmin"] < S["qmax"]:
            return WANQ_E_ARG, f"{name}: bad clamp range [{S['qmin']},{S['qmax']}]"
        if "fake_quant" in entry and not 2 <= S["n_bits"] <= (8 if "cols" in entry else 16):
            return WANQ_E_ARG, f"{name}: n_bits={S['n_bits']} must be in [2, {8 if 'cols' in entry else 16}]"
        if "n" in S:
            return None if S["n"] >= 0 and S["n"] % 8 == 0 else (WANQ_E_SHAPE, f"{name}: n={S['n']} must be a multiple of 8")
        row_frame = entry in ("wanq_row_minmax", "wanq_weight_quant", "wanq_weight_export_f16")
        if not (S["cols"] >= 8 and S["cols"] % 8 == 0 and (S["cols"] <= 16384 or not row_frame)):
            return WANQ_E_SHAPE, f"{name}: cols={S['cols']} must be a multiple of 8" + (" in [8, 16384]" if row_frame else "")
        return None

    # ---- plumbing
    def _flat(self, a, dt=None):
        v = (dec(a, DTS[dt]) if dt is not None else np.asarray(a).astype(F32)).ravel()
        return np.concatenate([v, np.full(PAD, np.nan, F32)])

    def _read(self, flat, idx):
        size = len(flat) - PAD
        bad = (idx < 0) | (idx >= size)
        if bad.any():
            self.oob += int(bad.sum())
            idx = np.where(bad, size, idx)
        return flat[idx]

    @staticmethod
    def _store(win, idx, val):
        """val (an array of the stored type) to elements idx of the window; an index outside it lands in the allocation around it."""
        flat = win.t.numpy().view(val.dtype)
        idx = np.asarray(idx) + GUARD // val.dtype.itemsize
        keep = (idx >= 0) & (idx < len(flat))
        flat[idx[keep]] = val[keep]

    def _chunks(self, total, cap):
        """Chunk ids in launch order: block 256 + thread + turn gridDim 256 over the turns = 0 .. total - 1 in order."""
        grid = min(-(-total // 256), cap)
        turns = 1 if self.mutant == "second_grid_turn_skipped" else -(-total // (grid * 256))
        return np.arange(min(turns * grid * 256, total), dtype=np.int64)

    def _row_col(self, ch, cols):
        cpr = cols // 8
        row = ch // (cpr + 1 if self.mutant == "row_from_cpr_plus_1" else cpr)
        return row, row * cols + (ch - row * cpr) * 8

    def _m(self, *names):
        return self.mutant if self.mutant in names else None

    # ---- kernels
    def _k_row_minmax(self, A, ins, dt, rows, cols):
        mut = self.mutant
        wf = self._flat(ins["w"], dt)
        wpr, nch = rm_form(cols)
        ids = np.arange(-(-rows // 4) * 4 if wpr == 1 else rows)
        if wpr == 1 and mut != "surplus_wave_writes":
            ids = ids[ids < rows]  # surplus(): the wave returns
        lo = np.full((len(ids), wpr), np.inf, F32)
        hi = np.full((len(ids), wpr), -np.inf, F32)
        lane = np.arange(64)
        for sub in range(wpr):
            for i in range(nch):
                col = (sub * 64 + lane + i * 64 * wpr) * 8
                live = col < cols
                if live.any():
                    v = self._read(wf, ids[:, None, None] * cols + col[live][None, :, None] + np.arange(8)[None, None, :])
                    lo[:, sub], hi[:, sub] = np.minimum(lo[:, sub], v.min((1, 2))), np.maximum(hi[:, sub], v.max((1, 2)))
                if mut == "dead_slots_read_as_zero" and not live.all():
                    lo[:, sub], hi[:, sub] = np.minimum(lo[:, sub], 0), np.maximum(hi[:, sub], 0)
        lo, hi = (lo[:, 0], hi[:, 0]) if mut == "wave0_only_reduction" else (lo.min(1), hi.max(1))
        for k, v in (("rmin", lo), ("rmax", hi), ("rabs", np.maximum(np.abs(lo), np.abs(hi)))):
            if A[k] is not None:
                self._store(A[k], ids, v.astype(F32))

    def _k_col_absmax(self, A, ins, dt, rows, cols):
        mut = self.mutant
        xf = self._flat(ins["x"], dt)
        slabs, rpb = ca_slabs(rows, cols)
        out = A["colmax"].get(F32)
        c = np.arange(cols)  # lanes with c0 >= cols of the last panel read nothing; cols % 8 == 0, so a live lane's 8 columns exist
        self.reads = 0
        for slab in range(slabs):
            r0 = slab * rpb
            r1 = min(r0 + rpb, rows)
            if mut == "absmax_last_slab_r1_off_by_one" and r0 + rpb >= rows:
                r1 -= 1
            rr = []
            for wave in range(4):
                r = r0 + wave
                while (r + 12 <= r1) if mut == "absmax_deep_loop_bound_le" else (r + 12 < r1):
                    rr += [r, r + 4, r + 8, r + 12]
                    r += 16
                while r < r1:
                    rr.append(r)
                    r += 3 if mut == "absmax_wave_stride_3" else 4
            self.reads += len(rr)
            if rr:
                m = np.abs(self._read(xf, np.array(rr, np.int64)[:, None] * cols + c[None, :])).max(0)
                out[:] = np.maximum(out, m)  # atomicMax on the bits of non-negative floats

    def _k_weight_quant(self, A, ins, dt, qmin, qmax, rows, cols):
        ch = self._chunks(rows * (cols // 8), CAP8)
        row, el = self._row_col(ch, cols)
        v = self._read(self._flat(ins["w"], dt), el[:, None] + np.arange(8)[None, :])
        d, z = self._read(self._flat(ins["delta"]), row)[:, None], self._read(self._flat(ins["zp"]), row)[:, None]
        qi, deq = wq_math(v, d, z, qmin, qmax, self._m("ties_away", "plus_zp", "loose_clamp_dropped", "deq_from_saturated_code"))
        idx = (el[:, None] + np.arange(8)[None, :]).ravel()
        if A["q8"] is not None:
            self._store(A["q8"], idx, qi.ravel())
        if A["deq"] is not None:
            self._store(A["deq"], idx, deq.ravel())

    def _k_weight_export_f16(self, A, ins, dt, rows, cols):
        ch = self._chunks(rows * (cols // 8), CAP8)
        row, el = self._row_col(ch, cols)
        v = self._read(self._flat(ins["w"], dt), el[:, None] + np.arange(8)[None, :])
        d, z = self._read(self._flat(ins["delta"]), row)[:, None], self._read(self._flat(ins["zp"]), row)[:, None]
        q = export_math(v, d, z, self._m("ties_away", "plus_zp", "export_quotient_rounded_once", "export_weight_not_rounded_first"))
        self._store(A["q8"], (el[:, None] + np.arange(8)[None, :]).ravel(), q.ravel())

    def _k_fake_quant_cols(self, A, ins, dt, odt, n_bits, rows, cols):
        ch = self._chunks(rows * (cols // 8), CAP8)
        row, el = self._row_col(ch, cols)
        c0 = el - row * cols
        v = self._read(self._flat(ins["x"], dt), el[:, None] + np.arange(8)[None, :])
        m = self._read(self._flat(ins["colmax"]), c0[:, None] + np.arange(8)[None, :])
        y = fqc_math(v, m, (1 << (n_bits - 1)) - 1, self._m("ties_away", "colmax_floor_missing"))
        self._store(A["out"], (el[:, None] + np.arange(8)[None, :]).ravel(), enc(y, DTS[odt]).ravel())

    def _k_fake_quant_with_delta(self, A, ins, dt, odt, n_bits, n):
        ch = self._chunks(n // 8, CAP8)
        idx = (ch[:, None] * 8 + np.arange(8)[None, :]).ravel()
        v, d = self._read(self._flat(ins["x"], dt), idx), self._read(self._flat(ins["delta"]), idx)
        bits = None if ins["bits"] is None else ins["bits"][np.minimum(idx, n - 1)]
        y = fqd_math(v, d, bits, n_bits, self._m("ties_away", "bits0_not_masked"))
        self._store(A["out"], idx, enc(y, DTS[odt]).ravel())

    def _k_pack_w4(self, A, ins, bias, rows, cols):
        mut = self.mutant
        i = self._chunks(rows * (cols // 32), CAP32)
        q = ins["q"].view(np.uint8).reshape(-1, 32)[i].astype(np.uint32)  # group i is read at q + i 32
        flip = 8 if bias else 0
        lo_flip = 0 if mut == "bias_flip_high_nibble_only" else flip
        out = np.zeros((len(i), 16), np.uint32)
        for half in range(2):  # a, b: 16 codes = dwords x y z w of 4 codes each
            e = q[:, half * 16:half * 16 + 16]
            for p in range(2):  # (x | y << 4), (z | w << 4)
                lo, hi = (e[:, p * 8:p * 8 + 4] ^ lo_flip) & 15, (e[:, p * 8 + 4:p * 8 + 8] ^ flip) & 15
                if mut == "nibbles_swapped":
                    lo, hi = hi, lo
                out[:, half * 8 + p * 4:half * 8 + p * 4 + 4] = lo | (hi << 4)
        stride = 32 if mut == "groups_at_stride_32" else 16
        self._store(A["packed"], (i[:, None] * stride + np.arange(16)[None, :]).ravel(), out.astype(np.uint8).ravel())

    def _k_unpack_w4(self, A, ins, bias, rows, cols):
        mut = self.mutant
        i = self._chunks(rows * (cols // 32), CAP32)
        stride = 32 if mut == "groups_at_stride_32" else 16
        pf = np.concatenate([ins["packed"].ravel().astype(F32), np.full(PAD, np.nan, F32)])
        p = np.nan_to_num(self._read(pf, (i[:, None] * stride + np.arange(16)[None, :]))).astype(np.int32)
        out = np.zeros((len(i), 32), np.int32)
        for d in range(4):  # dword d of the 16 bytes -> codes 8 d .. 8 d + 7: the low nibbles, then the high ones
            lo, hi = p[:, d * 4:d * 4 + 4] & 15, p[:, d * 4:d * 4 + 4] >> 4
            if mut == "nibbles_swapped":
                lo, hi = hi, lo
            out[:, d * 8:d * 8 + 4] = lo - (0 if mut == "bias_flip_high_nibble_only" else bias)
            out[:, d * 8 + 4:d * 8 + 8] = hi - bias
        self._store(A["q"], (i[:, None] * 32 + np.arange(32)[None, :]).ravel(), out.astype(np.int8).ravel())


def model_battery(run, big=()):
    """The probes of A and C at the smallest shapes that tell the mutants apart; -> {probe name: failures}.  big: the second-turn
    probes to run as well (16 million elements each: the unmutated model runs all six, a mutant those its kernel is in)."""
    got = {}
    for rows, cols, dt in ((5, 2056, "f16"), (9, 520, "bf16"), (3, 16384, "f32"), (9, 8, "f16"), (5, 8960, "bf16"), (1, 2048, "f32")):
        for j in range(rm_launches(rows, cols)):
            key = f"A1 row_minmax ({rows}, {cols}) {dt}"
            got[key] = got.get(key, []) + probe_row_minmax(run, rows, cols, dt, j) + probe_row_minmax(run, rows, cols, dt, j, (RM_OUTS[j % 3],))
    for rows, cols, dt in ((13, 8, "f16"), (28, 520, "bf16"), (17, 512, "f32"), (129, 8, "f32"), (3, 1536, "f16"), (65, 8, "bf16")):
        key = f"A2 col_absmax ({rows}, {cols}) {dt}"
        got[key] = sum((probe_col_absmax(run, rows, cols, dt, j) for j in range(ca_launches(rows, cols))), [])
    got[f"A2 col_absmax {CA_LONG} f16 slab ends"] = probe_col_absmax(run, *CA_LONG, "f16", 0) + probe_col_absmax(run, *CA_LONG, "f16", 1)
    for (rows, cols), dt, (qmin, qmax) in zip(WQ_SHAPES, ("f32", "f16", "bf16", "f32", "f16"), WQ_CLAMPS + WQ_CLAMPS[:2]):
        got[f"A3 weight_quant exact ({rows}, {cols}) {dt} clamp ({qmin}, {qmax})"] = probe_weight_quant_exact(run, rows, cols, dt, qmin, qmax)
    got["A3 weight_quant exact (37, 8) f32 q8 only"] = probe_weight_quant_exact(run, 37, 8, "f32", -257, 256, True, False)
    got["A3 weight_quant exact (37, 8) f32 deq only"] = probe_weight_quant_exact(run, 37, 8, "f32", -257, 256, False, True)
    got["A3 weight_quant random (5, 1536) f32"] = probe_weight_quant_random(run, 5, 1536, "f32")
    for (rows, cols), dt in zip(WQ_SHAPES[1:4], ("f16", "bf16", "f32")):
        got[f"A3 weight_export_f16 ({rows}, {cols}) {dt}"] = probe_weight_export(run, rows, cols, dt)
    for n_bits, (rows, cols), xdt, odt in ((2, FQC_SHAPES[0], "f32", "f16"), (4, FQC_SHAPES[1], "f16", "bf16"), (8, FQC_SHAPES[2], "bf16", "f32")):
        got[f"A4 fake_quant_cols {n_bits} bits ({rows}, {cols}) {xdt} -> {odt}"] = probe_fq_cols(run, rows, cols, xdt, odt, n_bits)
    got["A4 fake_quant_cols 6 bits (9, 520) f16 in place"] = probe_fq_cols(run, 9, 520, "f16", "f16", 6, True)
    for n_bits, n, xdt, odt in ((2, FQD_NS[1], "f32", "f32"), (8, FQD_NS[2], "f16", "bf16"), (16, FQD_NS[1], "bf16", "f16"), (8, 8, "f32", "f32")):
        got[f"A4 fake_quant_with_delta {n_bits} bits n {n} {xdt} -> {odt}"] = probe_fq_delta(run, n, xdt, odt, n_bits, False)
    got["A4 fake_quant_with_delta bits map n 2072 f32 -> f32"] = probe_fq_delta(run, FQD_NS[1], "f32", "f32", 8, True)
    got["A4 fake_quant_with_delta bits map n 4120 f16 in place"] = probe_fq_delta(run, FQD_NS[2], "f16", "f16", 8, True, True)
    for bias in (0, 8):
        got[f"A5 w4 (17, 64) bias {bias}"] = probe_w4(run, 17, 64, bias)
    got["A5 w4 (3, 8960) bias 8"] = probe_w4(run, 3, 8960, 8)
    for kernel in big:
        got[f"A6 second turn {kernel}"] = probe_big(run, kernel)
    got["C empty calls"] = probe_edge_calls(run, True)
    got["C refused calls"] = probe_edge_calls(run, False)
    return got


def test_model_passes_every_probe():
    got = model_battery(ModelRun(), BIG_KERNELS)
    assert {k: v[:3] for k, v in got.items() if v} == {}


def test_model_passes_the_tables_of_the_gpu_tests():
    """The GPU tests' own loops on the model, thinned where they are long: every launch of one type for the statistics kernels."""
    run = ModelRun()
    for rows, cols, j, outs in rm_table("bf16"):
        if rows in (3, 9):
            assert probe_row_minmax(run, rows, cols, "bf16", j, outs) == [], (rows, cols, j, outs)
    for rows, cols in ca_table()[:-1]:
        for j in range(min(ca_launches(rows, cols), 3)):
            assert probe_col_absmax(run, rows, cols, "f16", j) == [], (rows, cols, j)
    assert probe_col_absmax(run, *CA_LONG, "f32", 2) == []
    for dt in DTS:
        for qmin, qmax in WQ_CLAMPS:
            assert probe_weight_quant_exact(run, 5, 1536, dt, qmin, qmax) == []
        assert probe_weight_export(run, 3, 8960, dt) == [] and probe_weight_quant_random(run, 37, 8, dt) == []


# what each mutant must fail at the least (a substring of the probe's name)
MUTANT_FAILS = {
    "absmax_last_slab_r1_off_by_one": ("A2 col_absmax (13, 8)", "A2 col_absmax (129, 8)", "A2 col_absmax (140000, 8)"),
    "absmax_deep_loop_bound_le": ("A2 col_absmax (13, 8)", "A2 col_absmax (28, 520)"),
    "absmax_wave_stride_3": ("A2 col_absmax (13, 8)", "A2 col_absmax (28, 520)"),
    "second_grid_turn_skipped": tuple(f"A6 second turn {k}" for k in BIG_KERNELS),
    "row_from_cpr_plus_1": ("A3 weight_quant exact (37, 8)", "A3 weight_quant exact (3, 8960)", "A3 weight_export_f16 (3075, 64)", "A4 fake_quant_cols 4 bits"),
    "surplus_wave_writes": ("A1 row_minmax (9, 520)", "A1 row_minmax (9, 8)", "A1 row_minmax (1, 2048)"),
    "dead_slots_read_as_zero": ("A1 row_minmax (5, 2056)", "A1 row_minmax (9, 520)", "A1 row_minmax (5, 8960)"),
    "wave0_only_reduction": ("A1 row_minmax (5, 2056)", "A1 row_minmax (3, 16384)", "A1 row_minmax (5, 8960)"),
    "ties_away": ("A3 weight_quant exact (3075, 64)", "A4 fake_quant_cols 2 bits", "A4 fake_quant_with_delta 2 bits"),
    "plus_zp": ("A3 weight_quant exact (37, 8)", "A3 weight_quant random", "A3 weight_export_f16 (3075, 64)"),
    "loose_clamp_dropped": ("A3 weight_quant exact (3075, 64)", "A3 weight_quant exact (37, 8) f32 deq only"),
    "deq_from_saturated_code": ("A3 weight_quant exact (37, 8) f32 deq only", "A3 weight_quant exact (5, 1536)"),
    "export_quotient_rounded_once": (),  # equivalent: see MUTANT_NOTES
    "export_weight_not_rounded_first": ("A3 weight_export_f16 (5, 1536) f32",),
    "colmax_floor_missing": ("A4 fake_quant_cols 2 bits", "A4 fake_quant_cols 8 bits"),
    "bits0_not_masked": ("A4 fake_quant_with_delta bits map n 2072", "A4 fake_quant_with_delta bits map n 4120"),
    "nibbles_swapped": ("A5 w4 (17, 64) bias 0", "A5 w4 (17, 64) bias 8", "A5 w4 (3, 8960)"),
    "bias_flip_high_nibble_only": ("A5 w4 (17, 64) bias 8", "A5 w4 (3, 8960) bias 8"),
    "groups_at_stride_32": ("A5 w4 (17, 64) bias 0", "A5 w4 (3, 8960)"),
}
# probes a mutant must NOT fail: it is seen where its path runs and nowhere else
MUTANT_PASSES = {
    "surplus_wave_writes": ("A1 row_minmax (5, 2056)", "A1 row_minmax (3, 16384)", "A2", "A3"), "wave0_only_reduction": ("A1 row_minmax (9, 520)", "A1 row_minmax (9, 8)"),
    "bias_flip_high_nibble_only": ("A5 w4 (17, 64) bias 0",), "loose_clamp_dropped": ("q8 only", "A3 weight_export"),
    "deq_from_saturated_code": ("q8 only", "clamp (-17, 16)"), "bits0_not_masked": ("A4 fake_quant_with_delta 8 bits",),
    "absmax_deep_loop_bound_le": ("A2 col_absmax (17, 512)", "A2 col_absmax (129, 8)", "A1"), "second_grid_turn_skipped": ("A3", "A4", "A5"),
    "export_weight_not_rounded_first": ("A3 weight_export_f16 (3075, 64) f16", "A3 weight_export_f16 (1027, 128) bf16", "A3 weight_quant"),
}
MUTANT_BIG = {"second_grid_turn_skipped": BIG_KERNELS}
EQUIVALENT = ("export_quotient_rounded_once",)
MUTANT_NOTES = {
    "export_quotient_rounded_once": "EQUIVALENT, fails nothing: fl16(fl32(a / b)) == fl16(a / b) for every fp16 pair (fp32 holds 24 >= 2 11 + 2 bits, so the double "
                                    "rounding of a quotient is innocuous; near_midpoint_pairs checks 786 432 pairs).  The probes keep quotients next to k + 1/2, "
                                    "where a division that is not correctly rounded would have the least room",
    "absmax_wave_stride_3": "computes the same maxima (every row is still read by some wave): seen only by the model's count of rows read, which has no GPU counterpart",
    "surplus_wave_writes": "seen by the guards: the wave reads behind the matrix and stores behind the vector",
    "absmax_deep_loop_bound_le": "reads the row behind the last slab: the input's guard holds a huge value there",
    "groups_at_stride_32": "the guard behind the packed bytes is written, and the odd 16-byte groups keep the sentinel",
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_model_fail_named_probes(mutant):
    got = model_battery(ModelRun(mutant), MUTANT_BIG.get(mutant, ()))
    failed = {k: v for k, v in got.items() if v}
    print(f"MUTANT {mutant}: fails {sorted(failed)}")
    assert bool(failed) != (mutant in EQUIVALENT), (mutant, sorted(failed))
    for want in MUTANT_FAILS[mutant]:
        assert any(want in k for k in failed), (mutant, want, sorted(failed))
    for keep in MUTANT_PASSES.get(mutant, ()):
        assert not any(keep in k for k in failed), (mutant, keep, sorted(failed))
    flat = [f for v in failed.values() for f in v]
    if mutant == "surplus_wave_writes":
        assert any("guard behind rm" in f for f in flat) and any("read outside an operand" in f for f in flat)
    if mutant == "absmax_deep_loop_bound_le":
        assert any("read outside an operand" in f for f in flat)
    if mutant == "absmax_wave_stride_3":
        assert all("rows of" in f for f in flat)
    if mutant == "groups_at_stride_32":
        assert any("guard behind packed" in f for f in flat) and any("never written" in f for f in flat)
    if mutant == "second_grid_turn_skipped":
        assert all(any("of the second turn were never written" in f for f in got[f"A6 second turn {k}"]) for k in BIG_KERNELS)


def mutant_table_text():
    lines = ["Mutants of the numpy model in tests/test_gpu_quant_tools_probes.py (ModelRun) and the probes that catch them",
             "=" * 109, "",
             "The model restates the kernels of csrc/quant_tools.hip as written (host checks, launch geometry, index arithmetic, the fp32",
             "arithmetic); each mutant is one deliberate error in it.  test_mutants_of_the_model_fail_named_probes runs the probes of the GPU",
             "tests on every mutant, on a machine without a GPU, and asserts for each the probes named below (substrings of the names in",
             "model_battery); test_mutant_table_is_the_committed_one keeps this file equal to the table asserted there.", ""]
    for m in MUTANTS:
        lines.append(m)
        lines += [f"    fails   {p}" for p in MUTANT_FAILS[m]]
        lines += [f"    passes  {p}" for p in MUTANT_PASSES.get(m, ())]
        if m in MUTANT_NOTES:
            lines.append(f"    note    {MUTANT_NOTES[m]}")
    return "\n".join(lines) + "\n"


def test_mutant_table_is_the_committed_one():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quant_tools_probe_mutants.txt")
    with open(path) as f:
        assert f.read() == mutant_table_text()
    assert set(MUTANT_FAILS) == set(MUTANTS) and all(MUTANT_FAILS[m] for m in MUTANTS if m not in EQUIVALENT)


if __name__ == "__main__":  # python tests/test_gpu_quant_tools_probes.py > profiles/quant_tools_probe_mutants.txt
    print(mutant_table_text(), end="")
