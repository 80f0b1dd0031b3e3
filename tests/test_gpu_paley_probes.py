"""The Paley transforms in front of ffn.2 -- rotate140_kernel (8960 = 140 x 64 columns) and rotate108_kernel (13824 = 108 x 128) of
csrc/rotate_paley.hip -- on inputs whose answer is known bit for bit.  Every call goes through the C ABI (wanq_rotate_quant_rows
with had_k = 140 / 108), so every pointer is NULL or set freely and every dtype code is chosen; every output has a sentinel row
behind it.  The arguments are in profiles/PARITY_NOTES.md ("Paley transforms").

  A  exact probes   1  one entry of P_K per row (one-hot rows)         2  one dense block of integers per row
                    3  more rows than workgroups (2 x 512 + 3)          4  every output form
  C  refusals and rows = 0 through the ABI.
  E  CPU self-tests (not marked gpu): the checkers take (outputs, case); a plain numpy model of the kernel (butterfly, scale,
     three-way split into LDS planes, P mix per k-step, Y back over the planes, quantiser tail) passes them and mutants fail them.

The pin (float64 / numpy, written here):
  P_K        oracle.qdiff_ref.paley1(K - 1); H_M[j, j0] = (-1)^popcount(j & j0).
  c          float32(1) / sqrt(float32(n)): the kernel MULTIPLIES by this value (the oracle divides by the sqrt; not the pin here).
  split      x = fl32(v c); hi = bf16(x); r = x - hi (order 108) or fl32(v c - hi) from the exact product (order 140; float64 holds
             it exactly); mid = bf16(r); lo = bf16(r - mid); all RNE.
  one term   a row with ONE non-zero block k0 gives every output one non-zero product per plane, so
             out[m M + j] = P[m, k0] * fl32(fl32(lo_j + mid_j) + hi_j)  whatever order the matrix core walks k in; lo + mid is
             always representable (asserted), and at order 108 so is the total: it is x.  At order 140 the total can need 25 bits:
             where it is an fp32 number equality is demanded, elsewhere one fp32 unit is allowed -- the only allowance in this file.
  tail       codes, scale and sum are oracle.kernel_ref.quant_sum of the fp32 values (the model the row-wise probes use).

Geometry, from K and M as PaleyOrder in the kernel derives it:

  order  M    lanes/block  SLOTS  passes  k-steps  KP   row tiles  halves  first remainder  padding rows
  140    64   8            32     5       9        144  5 (3 : 2)  1       fma(v, c, -hi)   zeroed per row (140..143)
  108    128  16           16     7       7        112  4          2       x - hi           written as zeros by the slots 108..111
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_ref as kr
from oracle import qdiff_ref as qr

gpu = pytest.mark.gpu
DEV = "cuda"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DTC = {"f16": 0, "bf16": 1, "f32": 2}  # WANQ_F16 / BF16 / F32 (include/wanq_hip.h)
DTS = ["f16", "bf16", "f32"]
SENT = -7776.0  # exact in fp16, bf16 and fp32
SENT8 = -77
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
GRID = 512  # workgroups of a launch with at least that many rows; below it row r runs in workgroup r
F32, F64 = np.float32, np.float64


def popcount(a):
    a, c = np.array(a, dtype=np.int64), 0
    while a.any():
        c = c + (a & 1)
        a = a >> 1
    return c + np.zeros_like(a)


class Order:
    """The constants of PaleyOrder<K, M, ...> in csrc/rotate_paley.hip, computed the same way."""

    def __init__(self, K, M, fma_r):
        self.K, self.M, self.N, self.fma_r = K, M, K * M, fma_r
        self.LPB = M // 8
        self.SLOTS = 256 // self.LPB
        self.PASSES = -(-K // self.SLOTS)
        self.KSTEPS = -(-K // 16)
        self.KP = 16 * self.KSTEPS
        self.PLANE = self.KP * 128  # bytes
        self.HALVES = M // 64
        self.TILES = -(-K // 32)
        self.LIGHT = K % 32 != 0 and self.HALVES == 1  # order 140: 3 : 2 row tiles, the last with K - 32 (TILES - 1) live rows
        self.PAD_SLOTS = self.SLOTS * self.PASSES == self.KP
        self.c = F32(1) / np.sqrt(F32(self.N))
        self.P = qr.paley1(K - 1)
        j = np.arange(M)
        self.H = (1 - 2 * (popcount(j[:, None] & j[None, :]) & 1)).astype(F64)

    def __repr__(self):
        return f"order {self.K}"


ORDERS = {140: Order(140, 64, True), 108: Order(108, 128, False)}
# k0 of the dense block: both sides of every block-slot pass boundary (SLOTS ps) and the two ends
K0_TABLE = {140: [0, 31, 32, 127, 128, 139], 108: [0, 15, 16, 95, 96, 107]}


def hash32(r, c, salt):
    """A fixed integer hash of (r, c): uint64 array of values below 2^32 (the one of test_gpu_rowwise_probes.py)."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(r, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(c, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(salt * 0x27D4EB2F + 1)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return h


def rnd32(a, dt):
    """a rounded once into dtype dt, as float32 (every value of the three types is an fp32 number)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(TDT[dt]).float().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def bf16_rne(a):
    """The bf16 nearest to each (finite) fp32 value, ties to even, as fp32."""
    u = bits(a).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(F32)


def split3(w, c, fma_r):
    """numpy model of split3_store: (x, hi, mid, lo) of the fp32 values w scaled by c.  w c is exact in float64 (24 x 24 bits), and so
    is w c - hi (it spans no more bits than w c)."""
    prod = np.asarray(w, F64) * float(c)
    x = prod.astype(F32)
    hi = bf16_rne(x)
    r = (prod - hi).astype(F32) if fma_r else x - hi
    mid = bf16_rne(r)
    lo = bf16_rne(r - mid)
    return x, hi, mid, lo


def one_term_sum(w, od):
    """(value, exact): fl32(fl32(lo + mid) + hi), the accumulator after the three planes of the only non-zero k, and whether
    hi + mid + lo is itself an fp32 number (then no rounding is left anywhere)."""
    x, hi, mid, lo = split3(w, od.c, od.fma_r)
    lm = lo + mid
    assert np.array_equal(lm.astype(F64), lo.astype(F64) + mid), "lo + mid must be representable"
    y = lm + hi
    exact = y.astype(F64) == hi.astype(F64) + mid + lo
    if not od.fma_r:
        assert exact.all() and np.array_equal(y, x), "order 108: hi + mid + lo == fl32(v c)"
    return y, exact


# ================================================================================================ cases
class PaleyCase:
    """x [rows, n] (values exact in x_dt), premul [n] or None, and for every pinned row -- its non-zero blocks, one in
    every probe here, lie in one group of 8 -- the exact expected fp32 row and the mask of elements whose last addition is not exact (order 140 only).
    Rows that are not pinned (dense data) are compared between launches, never with a model."""

    def __init__(self, od, x, premul=None, pinned=None, x_dt="f32", out_dt="f32", vec_dt="f32", want_out=True, want_q=True, want_sum=True,
                 what=""):
        self.od, self.x_dt, self.out_dt, self.vec_dt, self.what = od, x_dt, out_dt, vec_dt, what
        self.want_out, self.want_q, self.want_sum = want_out, want_q, want_sum
        self.x = np.ascontiguousarray(x, dtype=F32)
        self.rows = R = self.x.shape[0]
        assert self.x.shape == (R, od.N) and np.array_equal(rnd32(self.x, x_dt), self.x), "inputs must be exact in their dtype"
        self.premul = None if premul is None else np.ascontiguousarray(premul, dtype=F32)
        self.pinned = np.ones(R, bool) if pinned is None else np.asarray(pinned, bool)
        K, M = od.K, od.M
        xb = self.x.reshape(R, K, M)
        nz = (xb != 0).any(axis=2)
        pm = np.ones((K, M)) if premul is None else self.premul.astype(F64).reshape(K, M)
        p = np.flatnonzero(self.pinned)
        # the non-zero blocks of a pinned row lie in ONE group of 8 consecutive blocks -- the 8 elements of k that one lane holds in one
        # matrix-core step -- so the accumulator takes three additions in all: the lo terms, the mid terms, the hi terms
        blocks = (nz[p].argmax(axis=1) // 8)[:, None] * 8 + np.arange(8)[None, :]
        live = blocks < K
        blocks = np.minimum(blocks, K - 1)
        assert (nz[p].sum(axis=1) == (nz[p[:, None], blocks] & live).sum(axis=1)).all(), "a pinned row's non-zero blocks share a group of 8"
        self.single = np.zeros(R, bool)
        self.single[p] = nz[p].sum(axis=1) <= 1
        w = (xb[p[:, None], blocks].astype(F64) * live[:, :, None] * pm[blocks]) @ od.H  # H_M (x premul): exact
        assert np.array_equal(w.astype(F32), w) and np.abs(w).max(initial=0) < 2 ** 24, "the butterfly must stay exact"
        _, hi, mid, lo = split3(w, od.c, od.fma_r)
        Pg = od.P[:, blocks].transpose(1, 0, 2) * live[:, None, :]  # [row, m, k]
        a = np.zeros((len(p), K, M))
        for plane in (lo, mid, hi):
            assert np.array_equal(a.astype(F32), a), "the sums of the lo and of the lo + mid terms must be representable"
            a = a + np.einsum("rmk,rkj->rmj", Pg, plane.astype(F64))
        y = a.astype(F32)
        one, _ = one_term_sum(w[self.single[p]], od)  # (a single block: the three-term sum of the module docstring, checked there)
        assert np.array_equal(np.abs(y[self.single[p]]), np.abs(one).max(axis=1)[:, None, :] * np.ones((1, K, 1), F32))
        self.expect = np.full((R, od.N), np.nan, dtype=F32)
        self.inexact = np.zeros((R, od.N), bool)
        self.expect[p] = y.reshape(len(p), od.N)
        self.inexact[p] = (y != a).reshape(len(p), od.N)
        assert od.fma_r or not self.inexact.any()

    def variant(self, **kw):
        """The same rows and expectation with other dtypes / outputs."""
        import copy

        c = copy.copy(self)
        for k, v in kw.items():
            assert hasattr(c, k)
            setattr(c, k, v)
        assert np.array_equal(rnd32(c.x, c.x_dt), c.x)
        return c

    def name(self):
        outs = "+".join(n for n, on in (("out:" + self.out_dt, self.want_out), ("q", self.want_q), ("sum", self.want_q and self.want_sum)) if on)
        return f"{self.od} {self.what} rows={self.rows} x={self.x_dt} premul={'NULL' if self.premul is None else 'set'} {outs} vec={self.vec_dt}"

    def out_bounds(self):
        """Lowest and highest admissible stored value of every element of the pinned rows: both are the expectation rounded into
        out_dt, except where the three-term sum is not an fp32 number -- there its two fp32 neighbours bound it."""
        e, ix = self.expect[self.pinned], self.inexact[self.pinned]
        lo = np.where(ix, np.nextafter(e, F32(-np.inf)), e)
        hi = np.where(ix, np.nextafter(e, F32(np.inf)), e)
        return rnd32(lo, self.out_dt), rnd32(hi, self.out_dt)


def premul_of(od, kind, salt=0):
    """None | 'sign': +-1 | 'pow2': +-2^f, f in [-2, 2] | 'small': +-1, +-2 -- by a hash of the column."""
    if kind is None:
        return None
    h = hash32(salt, np.arange(od.N), 51)
    s = np.where(h & np.uint64(1), 1.0, -1.0)
    if kind == "sign":
        return s
    if kind == "pow2":
        return s * 2.0 ** ((h >> np.uint64(1)) % np.uint64(5)).astype(np.int64).astype(F64) / 4.0
    assert kind == "small"
    return s * np.where(h & np.uint64(2), 2.0, 1.0)


def onehot_params(od, r):
    """(j0, sign, e) of probe row r: j0 = 0 on every 16th row (r = 0 is the one column of P whose sum is not zero)."""
    r = np.asarray(r)
    j0 = np.where(r % 16 == 0, 0, (hash32(r, 0, 41) % np.uint64(od.M)).astype(np.int64))
    sign = np.where(hash32(r, 0, 42) & np.uint64(1), 1.0, -1.0)
    e = (hash32(r, 0, 43) % np.uint64(7)).astype(np.int64) - 3
    return j0, sign, e


def onehot_rows(od, rs):
    """Row i is zero except x[i, r M + j0(r)] = +-2^e(r), r = rs[i]: one entry of column r of P_K per output block."""
    rs = np.asarray(rs)
    x = np.zeros((len(rs), od.N), dtype=F32)
    j0, sign, e = onehot_params(od, rs)
    x[np.arange(len(rs)), rs * od.M + j0] = sign * 2.0 ** e.astype(F64)
    return x


def onehot_closed_form(od, rs, premul):
    """out[i, m M + j] = P[m, r] Hsign(j, j0) sign premul[r M + j0] fl32(2^e c): the statement of probe 1, written out."""
    rs = np.asarray(rs)
    j0, sign, e = onehot_params(od, rs)
    pm = np.ones(len(rs)) if premul is None else np.asarray(premul, F64)[rs * od.M + j0]
    v = (sign * pm * 2.0 ** e.astype(F64) * float(od.c)).astype(F32)  # a power of two times c: exact
    hs = od.H[:, j0].T  # [i, j]
    return (od.P[:, rs].T[:, :, None] * hs[:, None, :] * v[:, None, None].astype(F64)).astype(F32).reshape(len(rs), od.N)


def block_rows(od, k0s, x_dt, salt=0):
    """Row i: block k0s[i] holds integers (|.| <= 8 for the 16-bit types, <= 2^15 for fp32: with |premul| <= 2 the butterfly stays
    below 2^24 while the scaled values carry full significands into mid and lo), every other block is zero."""
    x = np.zeros((len(k0s), od.N), dtype=F32)
    span = 8 if x_dt != "f32" else 2 ** 15
    for i, k0 in enumerate(k0s):
        h = hash32(i + 100 * salt, np.arange(od.M), 61)
        v = (h % np.uint64(2 * span + 1)).astype(np.int64) - span
        v[int(hash32(i, 0, 62) % np.uint64(od.M))] = span  # never an all-zero block, and the bound is reached
        x[i, k0 * od.M:(k0 + 1) * od.M] = v
    return x


def onehot_case(od, x_dt, premul_kind, lead, **kw):
    """The K one-hot rows behind `lead` zero rows: lead = 1 puts every column of P on the other parity of the 3 : 2 split."""
    x = np.concatenate([np.zeros((lead, od.N), F32), onehot_rows(od, np.arange(od.K))])
    return PaleyCase(od, x, premul_of(od, premul_kind), x_dt=x_dt, what=f"one-hot lead={lead} premul={premul_kind}", **kw)


def block_case(od, x_dt, premul_kind, salt=0, zero_row=False, **kw):
    x = block_rows(od, K0_TABLE[od.K], x_dt, salt)
    if zero_row:  # an all-zero row between two probe rows
        x = np.concatenate([x[:1], np.zeros((1, od.N), F32), x[1:]])
    return PaleyCase(od, x, premul_of(od, premul_kind, salt), x_dt=x_dt, what=f"dense block premul={premul_kind}", **kw)


def poison_value(od):
    """An fp32 v whose scaled value fl32(v c) has all ones in bits 14..7: read as two bf16, its low half is an Inf / NaN pattern.
    A row holding only v leaves that pattern in every element of Y, hence in whatever Y overwrites."""
    v = F32(1.0) + np.arange(1, 1 << 16, dtype=F32) * F32(2.0 ** -23)
    y, _ = one_term_sum(v.astype(F64), od)
    return v[np.flatnonzero((bits(y) & 0x7FE0) == 0x7FC0)[0]]  # bits 6..5 = 10: a unit either way keeps bits 14..7


@functools.lru_cache(maxsize=None)
def many_rows_case(od):
    """2 x 512 + 3 rows, fp32.  Rows below 512: dense full-significand data of magnitudes 2^-20 .. 2^20, every eighth a 'poison' row
    whose Y is Inf / NaN patterns when read as bf16; rows 2, 5, 510 and 511 hold the same data (even and odd workgroups).  Rows from
    512 up, which the same workgroups run on their second and third trip: one-hot and dense-block probes with zero rows between."""
    R, K = 2 * GRID + 3, od.K
    g = np.random.default_rng(140108 + K)
    x = np.zeros((R, od.N), dtype=F32)
    x[:GRID] = (g.standard_normal((GRID, od.N)) * 2.0 ** g.integers(-20, 21, size=(GRID, od.N))).astype(F32)
    pv = poison_value(od)
    for r in range(3, GRID, 8):
        x[r] = 0
        x[r, int(hash32(r, 0, 71) % np.uint64(od.N))] = pv
    x[5] = x[510] = x[511] = x[2]
    i = np.arange(R - GRID)
    blocks = block_rows(od, [K0_TABLE[K][t % 6] for t in range(24)], "f32", salt=3)
    hot = onehot_rows(od, np.arange(K))
    for t in i:
        if t % 3 == 0:
            x[GRID + t] = hot[(t // 3) % K]
        elif t % 3 == 1:
            x[GRID + t] = blocks[(t // 3) % 24]
    x[GRID + 7] = x[GRID + 4]  # the same probe on an odd and an even workgroup
    pinned = np.arange(R) >= GRID
    return PaleyCase(od, x, premul_of(od, "small", 5), pinned=pinned, what="more rows than workgroups")


# ================================================================================================ checker
def first_bad(bad, got, lo, hi, od, what):
    r, c = [int(v) for v in np.argwhere(bad)[0]]
    return (f"{what}: {int(bad.sum())} elements differ in rows {sorted(set(np.argwhere(bad)[:, 0].tolist()))[:8]}; first at row {r} col {c} "
            f"(block m={c // od.M}, j={c % od.M}): got {got[r, c]!r} expected {lo[r, c]!r}" + ("" if lo[r, c] == hi[r, c] else f" .. {hi[r, c]!r}"))


def check_paley(o, case, y32=None):
    """o: out float32 [rows + 1, n] | None, q int8 [rows + 1, n] | None, scale, sum float64 [rows + 1] (always allocated: they keep
    their sentinel where the call does not ask for them).  y32: the fp32 rows that feed the quantiser tail where the model cannot say
    them bit for bit (rows with an inexact element, rows that are not pinned); default: this launch's own fp32 out_fp."""
    od, R, pin, fails = case.od, case.rows, case.pinned, []
    if case.want_out:
        lo, hi = case.out_bounds()
        got = o["out"][:R][pin]
        bad = ~((got >= lo) & (got <= hi))
        if bad.any():
            fails.append(first_bad(bad, got, lo, hi, od, "out_fp (pinned rows, numbered among themselves)"))
        if not (o["out"][R] == SENT).all():
            fails.append("out_fp: the row after the last was written")
    vdt = np.float16 if case.vec_dt == "f16" else F32
    if case.want_q:
        src = case.expect.copy()
        own = case.inexact.any(axis=1) | ~pin
        if own.any():
            y = y32 if y32 is not None else (o["out"][:R] if case.want_out and case.out_dt == "f32" else None)
            if y is None:
                return fails + [f"{case.name()}: no fp32 values to pin the quantiser tail of rows {np.flatnonzero(own)[:6]}"]
            src[own] = y[own]
        if not np.isfinite(src).all():
            fails.append(f"non-finite values in rows {np.flatnonzero(~np.isfinite(src).all(axis=1))[:8]}")
            src = np.nan_to_num(src, nan=0.0, posinf=0.0, neginf=0.0)
        with np.errstate(over="ignore"):
            q, sc, sm = kr.quant_sum(src)
            sc, sm = sc.astype(vdt).astype(F64), sm.astype(vdt).astype(F64)
        bad = o["q"][:R] != q
        if bad.any():
            fails.append(first_bad(bad, o["q"], q, q, od, "q"))
        if not (o["q"][R] == SENT8).all():
            fails.append("q: the row after the last was written")
        if not np.array_equal(o["scale"][:R], sc):
            b = np.flatnonzero(o["scale"][:R] != sc)
            fails.append(f"scale: rows {b[:8]} differ; first got {o['scale'][b[0]]!r} expected {sc[b[0]]!r}")
        want_sum = sm if case.want_sum else np.full(R, SENT)
        if not np.array_equal(o["sum"][:R], want_sum):
            b = np.flatnonzero(o["sum"][:R] != want_sum)
            fails.append(f"sum: rows {b[:8]} differ; first got {o['sum'][b[0]]!r} expected {want_sum[b[0]]!r}")
    elif not ((o["scale"][:R] == SENT).all() and (o["sum"][:R] == SENT).all()):
        fails.append("scale / sum written without q")
    if o["scale"][R] != SENT or o["sum"][R] != SENT:
        fails.append("scale / sum: the slot after the last was written")
    return [f"{case.name()}: {f}" for f in fails]


def check_onehot_codes(o, case, lead):
    """Probe 1's own statement on the codes: exactly +-127 in the sign pattern of P[m, r] Hsign(j, j0) sign premul."""
    want = (127 * np.sign(case.expect[lead:])).astype(np.int64)
    assert (np.abs(want) == 127).all()
    return [] if np.array_equal(o["q"][lead:case.rows], want) else [f"{case.name()}: codes are not +-127 in the sign pattern of the column of P"]


def same_bits(a, b):
    return a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype == F32 else np.array_equal(a, b))


def check_same_rows(o1, rows1, o2, rows2, what):
    """Rows rows1 of launch o1 and rows2 of launch o2 agree bit for bit in every output both have."""
    fails = []
    for key in ("out", "q", "scale", "sum"):
        if o1.get(key) is not None and o2.get(key) is not None and not same_bits(o1[key][rows1], o2[key][rows2]):
            a, b = o1[key][rows1], o2[key][rows2]
            d = (bits(a) != bits(b)) if a.dtype == F32 else (a != b)
            fails.append(f"{what}: {key} differs in {int(d.sum())} places, first in position {np.argwhere(d)[0].tolist()} of the compared rows")
    return fails


# ================================================================================================ the numpy model of the kernel (E)
MUTANTS = ["lo_dropped", "p_transposed", "p_rules_swapped", "chi_shifted", "hm_bit_reversed", "blocks_exchanged", "tail_11",
           "stale_pad_nonzero_a", "no_pad_zeroing", "scale_one_half", "sum_missing_wave", "fma_r_flipped"]


def a_matrix(od, mutant=None):
    """The A operand: P_K in the top-left of [32 TILES, KP] zeros."""
    P = od.P.copy()
    if mutant == "p_transposed":
        P = P.T.copy()
    elif mutant == "p_rules_swapped":  # first row +1, first column -1
        P[0, 1:], P[1:, 0] = 1, -1
    elif mutant == "chi_shifted":  # chi(m - k + 1) off the diagonal
        core = np.roll(P[1:, 1:], 1, axis=1)
        np.fill_diagonal(core, 1)
        P[1:, 1:] = core
    A = np.zeros((32 * od.TILES, od.KP))
    A[:od.K, :od.K] = P
    if mutant == "stale_pad_nonzero_a":
        A[:od.K, od.K:] = 1
    return A


class ModelWorkgroup:
    """One workgroup's LDS (the three bf16 planes, Y in fp32 over them) and its rows, one after the other.  The planes start as
    zeros (on the GPU: whatever the LDS held; the kernel may not depend on it)."""

    def __init__(self, od, mutant=None):
        self.od, self.mutant, self.A = od, mutant, a_matrix(od, mutant)
        self.lds16 = np.zeros(3 * od.PLANE // 2, dtype=np.uint16)
        self.lds32 = self.lds16.view(F32)
        b, j = np.arange(od.KP)[:, None], np.arange(64)[None, :]
        self.idx = b * 64 + (j ^ (((b >> 1) & 1) << 5))  # plane_off / 2: the two 64-B halves of rows 2, 3 (mod 4) swap
        rev = np.arange(od.M)
        nb = od.M.bit_length() - 1
        self.bitrev = sum(((rev >> t) & 1) << (nb - 1 - t) for t in range(nb))

    def row(self, x, premul):
        """x [n] fp32 -> (y [n] fp32, amax)."""
        od, mutant, f = self.od, self.mutant, F32
        K, M, KP, half16 = od.K, od.M, od.KP, od.PLANE // 2
        v = x.reshape(K, M).astype(f)
        if premul is not None:
            v = v * premul.reshape(K, M)
        if mutant == "blocks_exchanged":  # pass 1 loads the blocks of pass 0 and the other way round
            perm = np.arange(K)
            perm[:od.SLOTS], perm[od.SLOTS:2 * od.SLOTS] = np.arange(od.SLOTS, 2 * od.SLOTS), np.arange(od.SLOTS)
            v = v[perm]
        h = 1
        while h < M:  # fp32 butterfly, natural order
            v = v.reshape(K, M // (2 * h), 2, h)
            a, b = v[:, :, 0, :], v[:, :, 1, :]
            v = np.stack([a + b, a - b], axis=2).reshape(K, M)
            h *= 2
        if mutant == "hm_bit_reversed":  # the stages pair the bits in reversed order: the block comes out bit-reversed
            v = v[:, self.bitrev]
        if not od.PAD_SLOTS and mutant not in ("no_pad_zeroing", "stale_pad_nonzero_a"):
            for pl in range(3):
                self.lds16[pl * half16 + K * 64: pl * half16 + KP * 64] = 0
        y, am = np.zeros((K, M), dtype=f), f(0)
        for half in range(od.HALVES):
            cols = slice(64 * half, 64 * half + 64)
            _, hi, mid, lo = split3(v[:, cols], od.c, od.fma_r != (mutant == "fma_r_flipped"))
            for pl, t in enumerate((hi, mid, lo)):
                self.lds16[pl * half16 + self.idx[:K]] = (bits(t) >> 16).astype(np.uint16)
                if od.PAD_SLOTS and mutant != "stale_pad_nonzero_a":
                    self.lds16[pl * half16 + self.idx[K:]] = 0
            acc = np.zeros((32 * od.TILES, 64), dtype=f)
            with np.errstate(invalid="ignore", over="ignore"):  # (a mutant's stale planes may read as anything)
                B = [(self.lds16[pl * half16 + self.idx].astype(np.uint32) << 16).view(f).astype(F64) for pl in range(3)]
                for s in range(od.KSTEPS):
                    for pl in (2, 1, 0):  # smallest terms first
                        if pl == 2 and mutant == "lo_dropped":
                            continue
                        acc = (acc.astype(F64) + self.A[:, 16 * s:16 * s + 16] @ B[pl][16 * s:16 * s + 16]).astype(f)
            m = np.fmax.reduce(np.abs(acc), axis=None)
            am = m if mutant == "scale_one_half" else np.fmax(am, m)
            nrows = 32 * od.TILES if not od.LIGHT else (K - 1 if mutant == "tail_11" else K + 1 if mutant == "tail_13" else K)
            self.lds32[:nrows * 64] = acc[:nrows].ravel()  # Y over the planes, after every read of them
            y[:, cols] = self.lds32[:K * 64].reshape(K, 64)
        return y.reshape(-1), am


def paley_model(case, mutant=None, rows=None):
    """The launch as the kernel runs it: min(rows, 512) workgroups, rows round-robin, one LDS per workgroup; then the shared tail."""
    od, f = case.od, F32
    R = case.rows if rows is None else rows
    grid = min(R, GRID)
    wgs = [ModelWorkgroup(od, mutant) for _ in range(grid)]
    y, amax = np.zeros((R, od.N), dtype=f), np.zeros(R, dtype=f)
    for r in range(R):
        y[r], amax[r] = wgs[r % grid].row(case.x[r], case.premul)
    o = {"out": None, "q": None, "scale": np.full(R + 1, SENT), "sum": np.full(R + 1, SENT)}
    if case.want_out:
        o["out"] = np.concatenate([rnd32(y, case.out_dt), np.full((1, od.N), SENT, dtype=f)])
    if case.want_q:
        scale = np.maximum(amax / f(127), f(1e-6)).astype(f)
        with np.errstate(invalid="ignore"):
            q = np.clip(np.rint(np.nan_to_num(y / scale[:, None])), -128, 127).astype(np.int64)
        qs = q
        if mutant == "sum_missing_wave":  # the thread of block b, chunk li is (b % SLOTS) LPB + li; wave 3 is left out
            wave = ((np.arange(od.K) % od.SLOTS)[:, None] * od.LPB + (np.arange(od.M) // 8)[None, :]) // 64
            qs = q * (wave.reshape(-1) != 3)
        vdt = np.float16 if case.vec_dt == "f16" else f
        with np.errstate(over="ignore", invalid="ignore"):
            o["scale"][:R] = scale.astype(vdt).astype(F64)
            if case.want_sum:
                o["sum"][:R] = (qs.sum(axis=1).astype(f) * scale).astype(vdt).astype(F64)
        o["q"] = np.concatenate([q, np.full((1, od.N), SENT8)]).astype(np.int8)
    return o


# ================================================================================================ the launch
def paley_gpu(case, rows=None):
    """wanq_rotate_quant_rows on the first `rows` rows of the case; every output has one row / slot more, prefilled with a sentinel."""
    from viditq_extension import _C

    od = case.od
    R = case.rows if rows is None else rows
    xt = torch.from_numpy(case.x[:R]).to(TDT[case.x_dt]).to(DEV)
    pm = None if case.premul is None else torch.from_numpy(case.premul).to(DEV)
    out = torch.full((R + 1, od.N), SENT, dtype=TDT[case.out_dt], device=DEV) if case.want_out else None
    q = torch.full((R + 1, od.N), SENT8, dtype=torch.int8, device=DEV) if case.want_q else None
    scale = torch.full((R + 1,), SENT, dtype=TDT[case.vec_dt], device=DEV)
    ssum = torch.full((R + 1,), SENT, dtype=TDT[case.vec_dt], device=DEV)
    rc = _C.lib.wanq_rotate_quant_rows(_C.ptr(xt), DTC[case.x_dt], _C.ptr(pm), od.K, _C.ptr(out), DTC[case.out_dt], _C.ptr(q), _C.ptr(scale),
                                       _C.ptr(ssum if case.want_q and case.want_sum else None), DTC[case.vec_dt], R, od.N, _C.stream())
    assert rc == WANQ_OK, _C.lib.wanq_last_error().decode()
    torch.cuda.synchronize()
    return {"out": None if out is None else out.float().cpu().numpy(), "q": None if q is None else q.cpu().numpy(),
            "scale": scale.double().cpu().numpy(), "sum": ssum.double().cpu().numpy()}


def head(o, n):
    """The first n rows of a launch's outputs (without its sentinel row)."""
    return {k: (None if v is None else v[:n]) for k, v in o.items()}


def unit_report(o, case):
    """(elements whose three-term sum is not an fp32 number, those of them where out_fp is not the nearest fp32)."""
    ix = case.inexact[case.pinned]
    got = o["out"][:case.rows][case.pinned]
    return int(ix.sum()), int((ix & (got != case.expect[case.pinned])).sum())


# ================================================================================================ A. exact probes on the GPU
PREMULS = [None, "sign", "pow2"]


def run_probe_kinds(launch, od, x_dt, kinds):
    """The sequence of launches and checks of probes 1, 2 and 4, written once for the GPU (launch = paley_gpu) and the model."""
    fails = []
    if "onehot" in kinds:
        for pk in PREMULS:
            for lead in (0, 1):
                case = onehot_case(od, x_dt, pk, lead)
                assert np.array_equal(case.expect[lead:], onehot_closed_form(od, np.arange(od.K), case.premul)) and not case.inexact.any()
                o = launch(case)
                fails += check_paley(o, case) + check_onehot_codes(o, case, lead)
    if "block" in kinds:
        for i, pk in enumerate((None, "small")):
            case = block_case(od, x_dt, pk, salt=i)
            full = launch(case)
            fails += check_paley(full, case)
            n_inexact, n_off = unit_report(full, case)
            print(f"PROBE paley {case.name()}: {n_inexact} of {case.inexact.size} elements have a three-term sum that is no fp32 number; "
                  f"{n_off} of them are not the nearest fp32")
            assert od.fma_r or n_inexact == 0
            for out_dt in ("bf16", "f16"):  # the 16-bit output types: one rounding of the fp32 expectation; the tail from the fp32 launch
                c16 = case.variant(out_dt=out_dt, vec_dt=("f16" if out_dt == "f16" else "f32"))
                fails += check_paley(launch(c16), c16, y32=full["out"][:case.rows])
    if "forms" in kinds:
        case = block_case(od, x_dt, "small", salt=7, zero_row=True)
        full = launch(case)
        fails += check_paley(full, case)
        y32 = full["out"][:case.rows]
        if not ((full["q"][1] == 0).all() and full["scale"][1] == float(F32(1e-6)) and full["sum"][1] == 0 and (full["out"][1] == 0).all()):
            fails.append(f"{case.name()}: the all-zero row is not codes 0 under scale 1e-6")
        for kw in (dict(want_q=False), dict(want_out=False), dict(want_sum=False), dict(want_out=False, want_sum=False),
                   dict(vec_dt="f16"), dict(want_out=False, vec_dt="f16"), dict(out_dt="bf16"), dict(out_dt="f16", vec_dt="f16"),
                   dict(want_q=False, out_dt="bf16"), dict(want_q=False, out_dt="f16")):
            c = case.variant(**kw)
            o = launch(c)
            fails += check_paley(o, c, y32=y32)
            same = {k: v for k, v in o.items() if not (k in ("scale", "sum") and (c.vec_dt != "f32" or not c.want_q or (k == "sum" and not c.want_sum)))
                    and not (k == "out" and c.out_dt != "f32")}
            fails += check_same_rows(same, slice(0, case.rows), full, slice(0, case.rows), f"{c.name()} against the launch with every output")
    return fails


@gpu
@pytest.mark.parametrize("x_dt", DTS)
@pytest.mark.parametrize("K", [140, 108])
def test_one_entry_of_P_per_row(K, x_dt):
    """Probe 1: K one-hot rows, premul NULL / +-1 / +-2^f, once with a zero row in front (the other parity of the 3 : 2 split):
    out_fp == P[m, r] Hsign(j, j0) sign premul fl32(2^e c), codes exactly +-127, scale and sum the quantiser tail's own values."""
    fails = run_probe_kinds(paley_gpu, ORDERS[K], x_dt, ["onehot"])
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("x_dt", DTS)
@pytest.mark.parametrize("K", [140, 108])
def test_one_dense_block(K, x_dt):
    """Probe 2: block k0 of integers on both sides of every pass boundary and at the ends: P[m, k0] * model(H_M(x premul)_j).  Order
    108: equality.  Order 140: equality wherever hi + mid + lo is an fp32 number, one unit elsewhere (the count is printed)."""
    fails = run_probe_kinds(paley_gpu, ORDERS[K], x_dt, ["block"])
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("K", [140, 108])
def test_every_output_form(K):
    """Probe 4: out_fp only, q only, both, sum NULL, scale / sum in fp16 and fp32, out_fp in each type, an all-zero row between two
    probe rows; every form agrees bit for bit with the launch that asks for everything, and no sentinel moves."""
    fails = []
    for x_dt in ("f32", "bf16"):
        fails += run_probe_kinds(paley_gpu, ORDERS[K], x_dt, ["forms"])
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


def run_many_rows(launch, od):
    case = many_rows_case(od)
    o = launch(case)
    fails = check_paley(o, case)  # the probes of the second and third trip exactly; the tail of the dense rows from their own out_fp
    alone = launch(case, rows=GRID)
    fails += check_same_rows(o, slice(0, GRID), alone, slice(0, GRID), f"{od}: the dense rows against a launch of their own")
    for a, b in ((2, 5), (2, 510), (2, 511), (GRID + 4, GRID + 7)):
        fails += check_same_rows(o, slice(a, a + 1), o, slice(b, b + 1), f"{od}: rows {a} and {b} hold the same data")
    one = launch(case, rows=1)
    fails += check_same_rows(o, slice(0, 1), one, slice(0, 1), f"{od}: row 0 against rows = 1")
    probe = PaleyCase(od, case.x[GRID:GRID + 1], case.premul, what="rows = 1")
    fails += check_paley(launch(probe), probe)
    return fails


@gpu
@pytest.mark.parametrize("K", [140, 108])
def test_more_rows_than_workgroups(K):
    """Probe 3: 2 x 512 + 3 rows: every workgroup's second (and three workgroups' third) trip through the row loop meets its
    probe exactly although dense rows -- and rows whose Y reads as Inf / NaN bf16 patterns -- went over the planes and the padding
    rows before; dense rows equal a launch of their own; equal rows on even and odd workgroups give equal bits; rows = 1."""
    fails = run_many_rows(paley_gpu, ORDERS[K])
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ C. refusals through the ABI
def _abi_args(had_k, cols, rows=3, scale=True, vec="f32"):
    from viditq_extension import _C

    n = max(rows, 1)
    w = max(cols, 13824) + 8
    x = torch.zeros(n, w, dtype=torch.float32, device=DEV)
    pm = torch.ones(w, dtype=torch.float32, device=DEV)
    out = torch.full((n, w), SENT, dtype=torch.float32, device=DEV)
    q = torch.full((n, w), SENT8, dtype=torch.int8, device=DEV)
    sc = torch.full((n,), SENT, dtype=TDT[vec], device=DEV)
    sm = torch.full((n,), SENT, dtype=TDT[vec], device=DEV)
    p = _C.ptr
    args = [p(x), DTC["f32"], p(pm), had_k, p(out), DTC["f32"], p(q), p(sc) if scale else None, p(sm), DTC[vec], rows, cols, _C.stream()]
    return args, (out, q, sc, sm), (x, pm)


def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((t == (SENT8 if t.dtype == torch.int8 else SENT)).all()) for t in outs)


@gpu
def test_refusals_through_the_abi():
    """A width that is not the order's is refused with WANQ_E_SHAPE and a message that names the width the order transforms; q
    without scale, and a bf16 scale / sum (the ABI's vectors are fp16 or fp32), with WANQ_E_ARG; nothing is written."""
    from viditq_extension import _C

    rules = [(dict(had_k=140, cols=13824), WANQ_E_SHAPE, "had_k=140 is the transform of cols=8960 (got 13824)"),
             (dict(had_k=108, cols=8960), WANQ_E_SHAPE, "had_k=108 is the transform of cols=13824 (got 8960)"),
             (dict(had_k=140, cols=8968), WANQ_E_SHAPE, "had_k=140 is the transform of cols=8960 (got 8968)"),
             (dict(had_k=108, cols=8968), WANQ_E_SHAPE, "had_k=108 is the transform of cols=13824 (got 8968)"),
             (dict(had_k=140, cols=8960, scale=False), WANQ_E_ARG, "q needs scale"),
             (dict(had_k=108, cols=13824, scale=False), WANQ_E_ARG, "q needs scale"),
             (dict(had_k=140, cols=8960, vec="bf16"), WANQ_E_ARG, "valid vec dtype"),
             (dict(had_k=108, cols=13824, vec="bf16"), WANQ_E_ARG, "valid vec dtype")]
    for kw, code, message in rules:
        args, outs, keep = _abi_args(**kw)
        assert _C.lib.wanq_rotate_quant_rows(*args) == code, kw
        assert message in _C.lib.wanq_last_error().decode(), (kw, _C.lib.wanq_last_error().decode())
        assert _untouched(outs), kw


@gpu
@pytest.mark.parametrize("K", [140, 108])
def test_no_rows_is_ok_and_writes_nothing(K):
    from viditq_extension import _C

    args, outs, keep = _abi_args(K, ORDERS[K].N, rows=0)
    assert _C.lib.wanq_rotate_quant_rows(*args) == WANQ_OK
    assert _untouched(outs)


# ================================================================================================ E. CPU self-tests of the probes
def test_constants_of_the_pin():
    """c has a non-zero lo term at both widths; P is not symmetric and its columns are pairwise different (a one-hot names its
    column, and P is told from its transpose); the k0 table straddles every pass boundary; the geometry is the kernel's."""
    for K, cbits in ((140, 0x3C2D166C), (108, 0x3C0B5948)):
        od = ORDERS[K]
        assert int(bits(od.c)[0]) == cbits
        _, hi, mid, lo = split3(np.array([1.0]), od.c, False)
        assert lo[0] != 0 and float(hi[0]) + float(mid[0]) + float(lo[0]) == float(od.c)
        P = od.P
        assert not np.array_equal(P, P.T) and len({c.tobytes() for c in P.T}) == K and np.array_equal(P @ P.T, K * np.eye(K, dtype=np.int64))
        assert (P.sum(axis=0)[1:] == 0).all() and P.sum(axis=0)[0] == K  # only column 0 has a non-zero code sum: row 0 has j0 = 0
        assert onehot_params(od, 0)[0] == 0
        bounds = [od.SLOTS * ps for ps in range(1, od.PASSES) if od.SLOTS * ps < K]
        assert bounds, K
        want = {0, K - 1} | {b - 1 for b in (bounds[0], bounds[-1])} | {bounds[0], bounds[-1]}  # both sides of the first and the last boundary
        assert set(K0_TABLE[K]) == want, (K, sorted(want))
    a, b = ORDERS[140], ORDERS[108]
    assert (a.SLOTS, a.PASSES, a.KSTEPS, a.KP, a.TILES, a.HALVES, a.LIGHT, a.PAD_SLOTS) == (32, 5, 9, 144, 5, 1, True, False)
    assert (b.SLOTS, b.PASSES, b.KSTEPS, b.KP, b.TILES, b.HALVES, b.LIGHT, b.PAD_SLOTS) == (16, 7, 7, 112, 4, 2, False, True)
    assert a.K - 32 * (a.TILES - 1) == 12  # the live rows of a light wave's last tile


@pytest.mark.parametrize("K", [140, 108])
def test_three_way_split_loses_no_bit(K):
    """hi + mid + lo == fl32(v c) on 10^6 random fp32 values under the order-108 rule; under the order-140 rule the three terms
    equal the exact product's leading bits: |v c - (hi + mid + lo)| <= |v c - fl32(v c)|."""
    od = ORDERS[K]
    g = np.random.default_rng(K)
    v = (g.standard_normal(10 ** 6) * 2.0 ** g.integers(-30, 31, size=10 ** 6)).astype(F32)
    x, hi, mid, lo = split3(v, od.c, False)
    assert np.array_equal(hi.astype(F64) + mid + lo, x.astype(F64))
    x, hi, mid, lo = split3(v, od.c, True)
    prod = v.astype(F64) * float(od.c)
    assert (np.abs(prod - (hi.astype(F64) + mid + lo)) <= np.abs(prod - x)).all()


def test_poison_value_reads_as_inf_or_nan_in_bf16():
    for od in ORDERS.values():
        y, _ = one_term_sum(np.array([poison_value(od)], F64), od)
        for u in (int(bits(y)[0]) - 1, int(bits(y)[0]), int(bits(y)[0]) + 1):
            assert (u >> 7) & 0xFF == 0xFF  # the low half of the fp32 word, as bf16: exponent all ones


CPU_KINDS = [(140, "bf16", "onehot"), (140, "f32", "block"), (140, "f16", "block"), (140, "f32", "forms"), (108, "f16", "onehot"),
             (108, "f32", "block"), (108, "bf16", "block"), (108, "bf16", "forms")]


@pytest.mark.parametrize("K,x_dt,kind", CPU_KINDS)
def test_model_passes_the_probes(K, x_dt, kind):
    fails = run_probe_kinds(paley_model, ORDERS[K], x_dt, [kind])
    assert not fails, "\n".join(fails[:10])


@pytest.mark.parametrize("K", [140, 108])
def test_model_passes_more_rows_than_workgroups(K):
    fails = run_many_rows(paley_model, ORDERS[K])
    assert not fails, "\n".join(fails[:10])


def _small_probes(od):
    """The cases a mutant is run against: one-hot rows (both leads), dense blocks in fp32 and in a 16-bit type."""
    return [onehot_case(od, "f32", "pow2", 0), onehot_case(od, "bf16", None, 1), block_case(od, "f32", "small", salt=1), block_case(od, "f16", None),
            block_case(od, "f32", None)]


def _caught_by(od, mutant, cases):
    hits = []
    for case in cases:
        o = paley_model(case, mutant)
        f = check_paley(o, case)
        if case.what.startswith("one-hot"):
            f += check_onehot_codes(o, case, case.rows - od.K)
        if f:
            hits.append(case.what)
    return hits


# (order, mutant): the 12-row tail exists at order 140 only, the second half at order 108 only
MUTANT_RUNS = [(K, m) for K in (140, 108) for m in MUTANTS if m not in ("no_pad_zeroing", "stale_pad_nonzero_a")
               and (K, m) not in ((108, "tail_11"), (140, "scale_one_half"), (140, "fma_r_flipped"))]
# (140, fma_r_flipped): x - hi in place of fma(v, c, -hi) moves an output by one fp32 unit at the most, and only where hi + mid + lo is
# no fp32 number -- inside the one allowance of probe 2.  profiles/PARITY_NOTES.md, "Paley transforms", has what was tried.


@pytest.mark.parametrize("K,mutant", MUTANT_RUNS)
def test_mutated_models_fail_a_probe(K, mutant):
    od = ORDERS[K]
    hits = _caught_by(od, mutant, _small_probes(od))
    assert hits, (K, mutant)
    if mutant in ("p_transposed", "p_rules_swapped", "chi_shifted", "hm_bit_reversed", "sum_missing_wave"):
        assert any(h.startswith("one-hot") for h in hits), (K, mutant, hits)


@pytest.mark.parametrize("mutant", ["no_pad_zeroing", "stale_pad_nonzero_a"])
def test_stale_padding_rows_fail_the_second_trip(mutant):
    """Order 140 re-zeroes the planes' rows 140..143 for every row, because Y overwrote those of the hi plane.  Left stale they
    meet zeros of A -- harmless unless they read as Inf / NaN, which the poison rows of probe 3 see to -- or, with A's padding
    columns not zero either, any value."""
    od = ORDERS[140]
    case = many_rows_case(od)
    o = paley_model(case, mutant)
    assert check_paley(o, case)


def test_a_tail_of_13_rows_cannot_be_observed():
    """The light wave's last tile cut at 13 instead of 12 rows writes Y's row 140 -- a zero, 256 bytes inside the mid plane (rows
    136, 137), after every wave has read the planes; the next row's split writes those rows again before anything reads them, and
    the read-back stops at row 139.  So that mutant computes the same outputs: the model with it passes every probe."""
    od = ORDERS[140]
    assert 141 * 256 <= 3 * od.PLANE
    for case in _small_probes(od):
        assert not check_paley(paley_model(case, "tail_13"), case)
