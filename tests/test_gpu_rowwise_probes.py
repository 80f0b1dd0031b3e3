"""The row-wise kernels in front of and behind attention -- LayerNorm + modulate (+ quantise) (csrc/rowwise.hip), RMSNorm + RoPE
with its int8 and scatter forms (csrc/attn_prep.hip), LayerNorm + ViDiT transform (csrc/rotate.hip), gate + residual -- on
inputs whose answer is known exactly, and on random data under a derived elementwise bound.  The pin is a float64 definition
written here, or oracle/ where it has the function (kr.quant_sum, qr.matmul_hadU, qr.dynamic_quantize_sym).  Every kernel is
called through the C ABI, so mod_stride, gate_stride, rows_per_batch, positions, eps and the dtype codes are set freely.

  A  exact probes   every intermediate is exactly representable, so any correct evaluation order gives the same bits: equality.
  B  random data    |y - y64| under the bound derived in profiles/PARITY_NOTES.md; a code may differ from the float64 pipeline's
                    only where y64 / scale64 lies within delta of a half-integer, by one, and the excused share is <= 1 %.
  C  refusals and rows = 0 through the ABI.
  E  CPU self-tests (not marked gpu): the checkers take (outputs, case); a plain fp32 two-pass numpy model of each kernel
     passes them and eight mutants fail them.

Width -> compiled form, by chunks = cols / 8 (row_ladder in csrc/row_frame.h: one ladder for launch_rowwise in csrc/rowwise.hip and
rmsnorm_rope_impl in csrc/attn_prep.hip):

  chunks <=   64   128   192   256   512   768   1024  1280  1536  1792  2048
  form       (1,1) (1,2) (1,3) (1,4) (4,2) (4,3) (4,4) (4,5) (4,6) (4,7) (4,8)     (WPR, NCH)
  cols  <=    512  1024  1536  2048  4096  6144  8192 10240 12288 14336 16384

  smallest / largest width of a form: 8 | 264 / 512, 520 / 1024, 1032 / 1536, 1544 / 2048, 2056 / 4096, 4104 / 6144, 6152 / 8192,
  8200 / 10240, 10248 / 12288, 12296 / 14336, 14344 / 16384.
  At the smallest width of a form the last chunk slot of a lane is live on few lanes only (the ok[i] masking).

had_k -> rotate_kernel<KIN, Q, EPL> (launch_rotate in csrc/rotate.hip), rows per wave = 64 / (128 / EPL * Q):

  had_k   1        2        4        8        16       32       12        40
  cols    128      256      512      1024     2048     4096     1536      5120
  form    (1,1,8)  (2,1,8)  (4,1,8)  (2,4,8)  (8,2,8)  (8,4,8)  (12,1,4)  (20,2,4)
  rows/w  4        4        4        1        2        1        2         1
  had_k 140 (cols 8960) and 108 (cols 13824): rotate140_kernel / rotate108_kernel of csrc/rotate_paley.hip -> tests/test_gpu_paley_probes.py
"""
import collections
import math

import numpy as np
import pytest
import torch

from oracle import kernel_ref as kr
from oracle import qdiff_ref as qr

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DTC = {"f16": 0, "bf16": 1, "f32": 2}  # WANQ_F16 / BF16 / F32 (include/wanq_hip.h)
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}  # unit roundoff of the output type (fp32 values are stored as they are)
SENT = -7776.0  # exact in fp16, bf16 and fp32
SENT8 = -77
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
QMAGIC = np.float32(-12582912.0)

FORMS = [(64, 1, 1), (128, 1, 2), (192, 1, 3), (256, 1, 4), (512, 4, 2), (768, 4, 3), (1024, 4, 4), (1280, 4, 5), (1536, 4, 6),
         (1792, 4, 7), (2048, 4, 8)]
LN_WIDTHS = [8, 264, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200, 10240, 10248, 12288, 12296,
             14336, 14344, 16384, 5120, 8960, 13824]
RMS_WIDTHS = [8, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200, 10240, 10248, 12288, 12296, 14336, 14344,
              16384]
Q8_WIDTHS = [128, 512, 640, 1024, 1152, 1536, 1664, 2048, 2176, 4096, 4224, 6144, 6272, 8192, 8320, 10240, 10368, 12288, 12416, 14336, 14464,
             16384]
ROT_HADK = [1, 2, 4, 8, 16, 32, 12, 40]


def form_of(cols):
    """(WPR, NCH) of the instantiation that the dispatch picks for this width."""
    for limit, wpr, nch in FORMS:
        if cols // 8 <= limit:
            return wpr, nch
    raise ValueError(cols)


def rnd(a, dt):
    """a rounded once into dtype dt, as float64."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TDT[dt]).double().numpy()


def hash32(r, c, salt):
    """A fixed integer hash of (r, c): uint64 array of values below 2^32."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(r, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(c, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(salt * 0x27D4EB2F + 1)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return h


def first_bad(bad, got, want, what, cols_info=""):
    r, c = [int(v) for v in np.argwhere(bad)[0]]
    return (f"{what}: {int(bad.sum())} elements differ in rows {sorted(set(np.argwhere(bad)[:, 0].tolist()))[:6]}; first at row {r} col {c} "
            f"(chunk {c // 8}, lane {(c // 8) % 64}{cols_info}): got {got[r, c]} expected {want[r, c]}")


def with_sentinel_row(a, fill):
    return np.concatenate([np.asarray(a), np.full((1,) + np.asarray(a).shape[1:], fill, dtype=np.asarray(a).dtype)], axis=0)


# ================================================================================================ LayerNorm probe rows (A)
def ln_probe_rows(rows, cols, const_row=None, unbalance=0, salt=1):
    """x[r, c] = m_r + a_r s[r, c]: s in {+1, -1} with exactly cols / 2 of each per row, placed by a hash of (r, c); m_r an integer
    in [-200, 200]; a_r in {16, 32} (0 for the constant row).  Returns (x, z): z = s is the normalised row (0 on the constant row).
    Refuses (ValueError) a row whose mean is not m_r or whose deviations are not +-a_r: its expectation is not an integer."""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    order = np.argsort(hash32(r, c, salt), axis=1, kind="stable")
    s = -np.ones((rows, cols))
    np.put_along_axis(s, order[:, : cols // 2 + unbalance], 1.0, axis=1)
    m = (hash32(np.arange(rows), 0, salt + 1) % np.uint64(401)).astype(np.int64) - 200
    a = np.where(hash32(np.arange(rows), 0, salt + 2) & np.uint64(1), 32.0, 16.0)
    if const_row is not None:
        a[const_row] = 0.0
    x = m[:, None] + a[:, None] * s
    mean = x.sum(axis=1) / cols
    if not ((mean == m).all() and (np.abs(x - mean[:, None]) == a[:, None]).all() and (np.abs(x) <= 256).all()):
        raise ValueError("probe row without an exact expectation: the signs do not balance")
    return x, s * (a[:, None] != 0)


def modulation(n_batch, cols):
    """gamma[c], 1 + mscale[b, c], mshift[b, c]: small integers that encode c and b, so that a value from another column, chunk or
    batch moves the output by at least 1; |z gamma (1 + mscale) + mshift| <= 7 * 4 + 40 = 68."""
    c, b = np.arange(cols)[None, :], np.arange(n_batch)[:, None]
    gamma = 1.0 + c[0] % 7
    mscale = ((c // 7 + b) % 4).astype(np.float64)  # 1 + mscale in 1 .. 4
    mshift = ((c // 28) % 16 + 16 * (b % 4) - 40).astype(np.float64)
    return gamma, mshift, mscale


LnCfg = collections.namedtuple("LnCfg", "x mod out q sum vec gamma shift scale wide")
LN_CONFIGS = [
    # x dtype, mod dtype, out_fp dtype | None, q, sum, vec dtype, gamma, shift, scale, mod_stride = 6 * cols
    LnCfg("bf16", "f32", None, True, True, "f32", False, True, True, True),    # the model's norm1 / norm2 call
    LnCfg("bf16", "f32", "bf16", False, False, "f32", True, False, False, True),  # the model's affine norm3
    LnCfg("f16", "f16", "f16", True, False, "f16", True, True, True, False),
    LnCfg("f32", "f32", "f32", True, True, "f32", True, True, True, True),
    LnCfg("bf16", "bf16", "f32", False, False, "f32", False, True, False, True),
    LnCfg("f32", "f32", "bf16", False, False, "f32", True, False, True, True),
    LnCfg("f16", "f32", None, True, False, "f32", False, False, False, False),
    LnCfg("f32", "f16", "f16", True, True, "f16", True, True, True, False),
    LnCfg("bf16", "bf16", "bf16", True, True, "f32", True, True, True, True),
    LnCfg("f16", "f32", "f32", False, False, "f32", False, False, True, True),
    LnCfg("f32", "bf16", None, True, True, "f16", True, True, False, False),
    LnCfg("bf16", "f32", "f16", True, True, "f32", False, False, False, True),
]


class LnCase:
    """One LayerNorm probe: x [rows, cols] of integers, modulation per batch, eps, the configuration, the exact expected row."""

    def __init__(self, cols, cfg, eps, rows=11, rpb=3, const_row=None):
        self.rows, self.cols, self.rpb, self.eps, self.cfg = rows, cols, rpb, eps, cfg
        self.nb = -(-rows // rpb)
        self.x, z = ln_probe_rows(rows, cols, const_row)
        g, sh, sc = modulation(self.nb, cols)
        self.gamma, self.mshift, self.mscale = (g if cfg.gamma else None), (sh if cfg.shift else None), (sc if cfg.scale else None)
        self.expect = ln_modulate(z, self.gamma, self.mshift, self.mscale, rpb)
        assert np.abs(self.expect).max() <= 127

    def name(self):
        return f"cols={self.cols} eps={self.eps} {self.cfg}"


def ln_modulate(z, gamma, mshift, mscale, rpb, batch_of=None):
    b = np.arange(z.shape[0]) // rpb if batch_of is None else batch_of
    y = z.copy()
    if gamma is not None:
        y = y * gamma
    if mscale is not None:
        y = y * (1.0 + mscale[b])
    if mshift is not None:
        y = y + mshift[b]
    return y


def ln_cases(cols, with_const_row=True):
    """Every configuration at eps = 0 and at eps = 1e-6, and the constant row at eps = 1e-6 (at eps = 0 its rstd is 1 / 0).
    eps = 1e-6 must give the same bits: var = a^2 >= 256, and half an fp32 ulp of 256 is 2^-16 = 1.5e-5 > eps, so var + eps == var."""
    out = []
    for i, cfg in enumerate(LN_CONFIGS):
        out.append(LnCase(cols, cfg, 0.0))
        out.append(LnCase(cols, cfg, 1e-6, const_row=(i % 11 if with_const_row else None)))
    return out


def check_ln_exact(o, case):
    """o: dict of float64 / int arrays with one row more than the case (out, q, scale, sum: None where not requested)."""
    cfg, rows, fails = case.cfg, case.rows, []
    if cfg.out:
        bad = ~(o["out"][:rows] == case.expect)
        if bad.any():
            fails.append(first_bad(bad, o["out"], case.expect, "out_fp", f", batch {int(np.argwhere(bad)[0][0]) // case.rpb}"))
        if not (o["out"][rows] == SENT).all():
            fails.append("out_fp: the row after the last was written")
    if cfg.q:
        oq, oscale, osum = kr.quant_sum(case.expect.astype(np.float32))
        with np.errstate(over="ignore"):
            vdt = np.float16 if cfg.vec == "f16" else np.float32
            oscale, osum = oscale.astype(vdt).astype(np.float64), osum.astype(vdt).astype(np.float64)
        bad = ~(o["q"][:rows] == oq)
        if bad.any():
            fails.append(first_bad(bad, o["q"], oq, "q"))
        if not (o["q"][rows] == SENT8).all():
            fails.append("q: the row after the last was written")
        if not np.array_equal(o["scale"][:rows], oscale):
            fails.append(f"scale: got {o['scale'][:rows]} expected {oscale}")
        if o["scale"][rows] != SENT:
            fails.append("scale: the slot after the last was written")
        want_sum = osum if cfg.sum else np.full(rows, SENT)
        if not np.array_equal(o["sum"][:rows], want_sum):
            fails.append(f"sum: got {o['sum'][:rows]} expected {want_sum}")
        if o["sum"][rows] != SENT:
            fails.append("sum: the slot after the last was written")
    return [f"{case.name()}: {f}" for f in fails]


def ln_model(case, mutant=None):
    """Plain numpy model of rowwise_kernel<*, *, true>: fp32, two passes; inputs rounded into their dtypes first."""
    cfg, rows, cols, rpb = case.cfg, case.rows, case.cols, case.rpb
    f = np.float32
    x = rnd(case.x, cfg.x).astype(f)
    mod = lambda a: None if a is None else rnd(a, cfg.mod).astype(f)
    gamma, mshift, mscale = mod(case.gamma), mod(case.mshift), mod(case.mscale)
    xs = x
    if mutant == "drop_last_partial_chunk":  # the chunk slot NCH - 1 is left out of the mean where it is partial
        wpr, nch = form_of(cols)
        start = (nch - 1) * 64 * wpr * 8
        if start < cols < nch * 64 * wpr * 8:
            xs = x[:, :start]
    mean = (xs.sum(axis=1, dtype=f) / f(cols)).astype(f)
    d = x - mean[:, None]
    if mutant == "one_pass_variance":
        var = ((x * x).sum(axis=1, dtype=f) / f(cols) - mean * mean).astype(f)
    else:
        var = ((d * d).sum(axis=1, dtype=f) / f(cols)).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (f(1) / np.sqrt(var + f(case.eps), dtype=f)).astype(f)
        y = (d * rstd[:, None]).astype(f)
    b = np.arange(rows) // rpb
    if mutant == "neighbour_batch":  # the first row of a batch takes the batch in front
        b = np.where((np.arange(rows) % rpb == 0) & (b > 0), b - 1, b)
    if gamma is not None:
        g = gamma
        if mutant == "gamma_lane":  # lane 5 reads gamma one chunk further on
            c = np.arange(cols)
            g = np.where((c // 8) % 64 == 5, gamma[np.minimum(c + 8, cols - 1)], gamma)
        y = y * g
    if mscale is not None:
        y = y * (f(1) + mscale[b])
    if mshift is not None:
        y = y + mshift[b]
    y = y.astype(f)
    o = {"out": None, "q": None, "scale": None, "sum": None}
    if cfg.out:
        o["out"] = with_sentinel_row(rnd(y, cfg.out), SENT)
    if cfg.q:
        q, sc, sm = kr.quant_sum(np.nan_to_num(y))
        vdt = np.float16 if cfg.vec == "f16" else np.float32
        with np.errstate(over="ignore"):
            o["q"] = with_sentinel_row(q.astype(np.int64), SENT8)
            o["scale"] = with_sentinel_row(sc.astype(vdt).astype(np.float64), SENT)
            o["sum"] = with_sentinel_row(sm.astype(vdt).astype(np.float64), SENT) if cfg.sum else np.full(rows + 1, SENT)
    return o


def dev_t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TDT[dt]).to(DEV)


def mod_tensors(case_gamma, mshift, mscale, nb, cols, dt, wide):
    """gamma [cols]; shift and scale as chunks 1 and 4 of a [B, 6, cols] tensor whose other chunks hold 99 (mod_stride = 6 cols),
    or as [B, cols] tensors of their own (mod_stride = cols).  Returns (gamma, shift, scale, mod_stride, keep-alive)."""
    g = None if case_gamma is None else dev_t(case_gamma, dt)
    if wide:
        m = torch.full((nb, 6, cols), 99.0, dtype=TDT[dt], device=DEV)
        if mshift is not None:
            m[:, 1] = dev_t(mshift, dt)
        if mscale is not None:
            m[:, 4] = dev_t(mscale, dt)
        return g, (m[:, 1] if mshift is not None else None), (m[:, 4] if mscale is not None else None), 6 * cols, m
    sh = None if mshift is None else dev_t(mshift, dt)
    sc = None if mscale is None else dev_t(mscale, dt)
    return g, sh, sc, cols, None


def ln_gpu(case, x=None):
    """wanq_layernorm_rows on the case; every output has one row / slot more than the case, prefilled with a sentinel."""
    from viditq_extension import _C

    cfg, rows, cols = case.cfg, case.rows, case.cols
    xt = dev_t(case.x if x is None else x, cfg.x)
    g, sh, sc, stride, keep = mod_tensors(case.gamma, case.mshift, case.mscale, case.nb, cols, cfg.mod, cfg.wide)
    out = torch.full((rows + 1, cols), SENT, dtype=TDT[cfg.out], device=DEV) if cfg.out else None
    q = torch.full((rows + 1, cols), SENT8, dtype=torch.int8, device=DEV) if cfg.q else None
    scale = torch.full((rows + 1,), SENT, dtype=TDT[cfg.vec], device=DEV) if cfg.q else None
    ssum = torch.full((rows + 1,), SENT, dtype=TDT[cfg.vec], device=DEV) if cfg.q else None
    _C.call("wanq_layernorm_rows", _C.ptr(xt), DTC[cfg.x], _C.ptr(g), _C.ptr(sh), _C.ptr(sc), DTC[cfg.mod], stride, case.rpb, float(case.eps),
            _C.ptr(out), DTC[cfg.out or "f32"], _C.ptr(q), _C.ptr(scale), _C.ptr(ssum if cfg.sum else None), DTC[cfg.vec], rows, cols, _C.stream())
    torch.cuda.synchronize()
    host = lambda t, kind=np.float64: None if t is None else t.cpu().to(torch.float64 if kind is np.float64 else torch.int64).numpy()
    return {"out": host(out), "q": host(q, np.int64), "scale": host(scale), "sum": host(ssum)}


@gpu
@pytest.mark.parametrize("cols", LN_WIDTHS)
def test_layernorm_exact_probe(cols):
    """11 rows, rows_per_batch = 3 (a batch boundary inside a 4-row workgroup, a ragged last batch, one surplus wave); every
    configuration of LN_CONFIGS at eps = 0 and 1e-6: out_fp equals the integers, q / scale / sum equal kr.quant_sum of them."""
    fails = []
    for case in ln_cases(cols):
        fails += check_ln_exact(ln_gpu(case), case)
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ RMSNorm + RoPE probes (A)
class RmsCase:
    """x[r, c] = +-a_r (a_r a power of two: ss = cols a_r^2 and, with eps = 0 or 1e-6 << ulp(a_r^2) / 2, x rinv = +-1), weight[c] in
    1 .. 4 by a hash of c, a RoPE table of integers in [-3, 3] that encode (pos, pair).  17 rows = 2 batches of 7 + 3, positions = 5:
    pos wraps, and rows with pos >= 5 come out normalised and unrotated in every batch.  |y| <= 24: exact in every dtype and through
    the kernel's fmaf / __fmul_rn pair.  Without the norm a_r is in {1, 2, 4}, so the same bound holds."""

    def __init__(self, cols, hd, norm=True, rope=True, eps=0.0, rows=17, rpb=7, positions=5):
        assert cols % hd == 0 and (norm or rope)
        self.cols, self.hd, self.norm, self.rope, self.eps, self.rows, self.rpb, self.positions = cols, hd, norm, rope, eps, rows, rpb, positions
        r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
        sign = np.where(hash32(r, c, 11) & np.uint64(1), 1.0, -1.0)
        pick = (hash32(np.arange(rows), 0, 12) % np.uint64(3)).astype(np.int64)
        a = np.array([16.0, 32.0, 64.0] if norm else [1.0, 2.0, 4.0])[pick]
        self.x = sign * a[:, None]
        self.weight = 1.0 + (hash32(0, np.arange(cols), 13) % np.uint64(4)).astype(np.float64)
        pos, pair = np.arange(positions)[:, None], np.arange(hd // 2)[None, :]
        self.table = np.stack([(pos * 3 + pair * 5 + 1) % 7 - 3, (pos * 2 + pair * 3 + pair // 7 + 4) % 7 - 3], axis=-1).astype(np.float64)
        self.expect = self.definition(sign * self.weight if norm else self.x, self.table)
        assert np.abs(self.expect).max() <= 24

    def definition(self, n, table, pos=None, rotate_padding=False):
        """float64: the normalised row n rotated per head with (cos, sin)[pos, pair], pos = row % rows_per_batch, rows with
        pos >= positions left as they are."""
        if not self.rope:
            return n.copy()
        pos = np.arange(self.rows) % self.rpb if pos is None else pos
        rot = pos < self.positions
        pidx = pos % self.positions if rotate_padding else np.minimum(pos, self.positions - 1)
        pair = (np.arange(self.cols) % self.hd) // 2
        cs = table[pidx][:, pair[0::2]]  # [rows, cols / 2, 2]
        a, b = n[:, 0::2], n[:, 1::2]
        y = n.copy()
        ya, yb = a * cs[..., 0] - b * cs[..., 1], a * cs[..., 1] + b * cs[..., 0]
        if rotate_padding:
            rot = np.ones_like(rot)
        y[:, 0::2] = np.where(rot[:, None], ya, a)
        y[:, 1::2] = np.where(rot[:, None], yb, b)
        return y

    def name(self):
        return f"cols={self.cols} head_dim={self.hd} norm={self.norm} rope={self.rope} eps={self.eps}"

    # ---- the scatter form: head h of row r lands at head_map[2h] + r head_map[2h + 1]; heads permuted, row stride cols + 16
    def head_map(self):
        H = self.cols // self.hd
        perm = np.argsort(hash32(0, np.arange(H), 14), kind="stable")
        return perm, self.cols + 16

    def scattered(self, y, swap=False):
        perm, rs = self.head_map()
        if swap and len(perm) > 1:
            perm = perm.copy()
            perm[[0, 1]] = perm[[1, 0]]
        d = np.full((self.rows + 1, rs), SENT)
        for h, p in enumerate(perm):
            d[: self.rows, p * self.hd:(p + 1) * self.hd] = y[:, h * self.hd:(h + 1) * self.hd]
        return d

    # ---- the int8 form: per-(token, head) codes and the two scale planes [heads][scale_stride]
    def q8_expected(self, y, stride):
        H = self.cols // 128
        q, delta = qr.dynamic_quantize_sym(y.reshape(self.rows * H, 128).astype(np.float32), 8)
        planes = np.full((2, H, stride), SENT, dtype=np.float64)
        planes[0, :, : self.rows] = delta.reshape(self.rows, H).T
        planes[1, :, : self.rows] = (QMAGIC * delta).astype(np.float32).reshape(self.rows, H).T
        return q.reshape(self.rows, self.cols).astype(np.int64), planes


def check_rms_exact(o, case, mode, out_dt="f32"):
    """mode: plain | scatter | q8 | q8_noout.  o: out [rows + 1, cols] (scatter: [rows + 1, cols + 16]), q8 [rows + 1, cols], planes."""
    rows, fails = case.rows, []
    if mode == "scatter":
        want = case.scattered(case.expect)
        bad = ~(o["out"] == want)
        if bad.any():
            r, c = [int(v) for v in np.argwhere(bad)[0]]
            fails.append(f"scatter: {int(bad.sum())} elements differ; first at row {r} buffer col {c} (slot {c // case.hd}): got {o['out'][r, c]} expected {want[r, c]}")
    elif mode != "q8_noout":
        bad = ~(o["out"][:rows] == case.expect)
        if bad.any():
            fails.append(first_bad(bad, o["out"], case.expect, "out", f", pos {int(np.argwhere(bad)[0][0]) % case.rpb}, pair {(int(np.argwhere(bad)[0][1]) % case.hd) // 2}"))
        if not (o["out"][rows] == SENT).all():
            fails.append("out: the row after the last was written")
    if mode in ("q8", "q8_noout"):
        stride = o["planes"].shape[2]
        q, planes = case.q8_expected(case.expect, stride)
        bad = ~(o["q8"][:rows] == q)
        if bad.any():
            fails.append(first_bad(bad, o["q8"], q, "q8"))
        if not (o["q8"][rows] == SENT8).all():
            fails.append("q8: the row after the last was written")
        if not np.array_equal(o["planes"], planes):
            bad = np.argwhere(~(o["planes"] == planes))[0]
            fails.append(f"scale planes: first difference at (plane, head, row) {bad.tolist()}: got {o['planes'][tuple(bad)]} expected {planes[tuple(bad)]}")
    return [f"{case.name()} {mode} out={out_dt}: {f}" for f in fails]


def rms_model(case, mode="plain", x_dt="f32", out_dt="f32", mutant=None, stride=64):
    """Plain numpy model of rmsnorm_rope_kernel (fp32)."""
    f = np.float32
    x = rnd(case.x, x_dt).astype(f)
    if case.norm:
        rinv = (f(1) / np.sqrt((x * x).sum(axis=1, dtype=f) / f(case.cols) + f(case.eps), dtype=f)).astype(f)
        n = (x * rinv[:, None]).astype(f) * case.weight.astype(f)
    else:
        n = x
    pos = np.arange(case.rows) if mutant == "pos_is_row" else None
    y = case.definition(n.astype(f), case.table.astype(f), pos=pos, rotate_padding=(mutant == "rope_on_padding")).astype(f)
    o = {}
    if mode == "scatter":
        o["out"] = rnd(case.scattered(y.astype(np.float64), swap=(mutant == "swap_heads")), out_dt)
    elif mode != "q8_noout":
        o["out"] = with_sentinel_row(rnd(y, out_dt), SENT)
    if mode in ("q8", "q8_noout"):
        q, planes = case.q8_expected(y.astype(np.float64), stride)
        o["q8"], o["planes"] = with_sentinel_row(q, SENT8), planes
    return o


def rms_gpu(case, mode="plain", x_dt="f32", out_dt="f32", inplace=False, x=None, table=None, weight=None):
    from viditq_extension import _C

    rows, cols = case.rows, case.cols
    xt = torch.full((rows + 1, cols), SENT, dtype=TDT[x_dt], device=DEV)
    xt[:rows] = dev_t(case.x if x is None else x, x_dt)
    w = dev_t(case.weight if weight is None else weight, "f32") if case.norm else None
    tab = dev_t(case.table if table is None else table, "f32") if case.rope else None
    o = {}
    if mode == "scatter":
        perm, rs = case.head_map()
        hm = torch.tensor([[int(p) * case.hd, rs] for p in perm], dtype=torch.int64, device=DEV)
        out = torch.full((rows + 1, rs), SENT, dtype=TDT[out_dt], device=DEV)
        _C.call("wanq_rmsnorm_rope_scatter", _C.ptr(xt), DTC[x_dt], _C.ptr(w), _C.ptr(tab), _C.ptr(out), DTC[out_dt], _C.ptr(hm), rows, cols, case.hd,
                case.rpb, case.positions, float(case.eps), _C.stream())
    elif mode == "plain":
        assert not inplace or x_dt == out_dt
        out = xt if inplace else torch.full((rows + 1, cols), SENT, dtype=TDT[out_dt], device=DEV)
        _C.call("wanq_rmsnorm_rope", _C.ptr(xt), DTC[x_dt], _C.ptr(w), _C.ptr(tab), _C.ptr(out), DTC[out_dt], rows, cols, case.hd, case.rpb,
                case.positions, float(case.eps), _C.stream())
    else:
        stride = -(-rows // 64) * 64  # rows rounded up to 64, as for keys: greater than rows, the gap keeps its sentinel
        out = torch.full((rows + 1, cols), SENT, dtype=TDT[out_dt], device=DEV) if mode == "q8" else None
        q8 = torch.full((rows + 1, cols), SENT8, dtype=torch.int8, device=DEV)
        planes = torch.full((2, cols // 128, stride), SENT, dtype=torch.float32, device=DEV)
        _C.call("wanq_rmsnorm_rope_q8", _C.ptr(xt), DTC[x_dt], _C.ptr(w), _C.ptr(tab), _C.ptr(out), DTC[out_dt], _C.ptr(q8), _C.ptr(planes), stride, rows,
                cols, case.hd, case.rpb, case.positions, float(case.eps), _C.stream())
        torch.cuda.synchronize()
        o["q8"], o["planes"] = q8.cpu().to(torch.int64).numpy(), planes.cpu().double().numpy()
    torch.cuda.synchronize()
    if out is not None:
        o["out"] = out.cpu().double().numpy()
    return o


FLAGS = [(True, True), (True, False), (False, True)]  # (norm, rope)
DTS = ["f16", "bf16", "f32"]


def head_dims(cols):
    return [hd for hd in (8, 64, 128) if cols % hd == 0]


@gpu
@pytest.mark.parametrize("cols", RMS_WIDTHS)
def test_rmsnorm_rope_exact_probe(cols):
    """Plain and scatter forms: every head_dim of {8, 64, 128} that divides the width; norm only, RoPE only and both, each with the
    three input dtypes against rotating output dtypes, once in place, once scattered; eps 0 and 1e-6 alternate."""
    wi, fails = RMS_WIDTHS.index(cols), []
    for hd in head_dims(cols):
        for fi, (norm, rope) in enumerate(FLAGS):
            for xi, x_dt in enumerate(DTS):
                case = RmsCase(cols, hd, norm, rope, eps=(0.0, 1e-6)[(xi + fi) % 2])
                out_dt = DTS[(xi + fi + wi) % 3]
                fails += check_rms_exact(rms_gpu(case, "plain", x_dt, out_dt), case, "plain", out_dt)
            dt = DTS[(fi + wi) % 3]
            fails += check_rms_exact(rms_gpu(case, "plain", dt, dt, inplace=True), case, "plain", dt)
            fails += check_rms_exact(rms_gpu(case, "scatter", dt, DTS[(fi + wi + 1) % 3]), case, "scatter", DTS[(fi + wi + 1) % 3])
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("cols", [512, 8960])
def test_rmsnorm_rope_every_dtype_pair(cols):
    """Input and output dtype fully crossed (fp16 included) with every flag, at one width per WPR."""
    fails = []
    for norm, rope in FLAGS:
        case = RmsCase(cols, 64 if cols == 512 else 128, norm, rope)
        for x_dt in DTS:
            for out_dt in DTS:
                fails += check_rms_exact(rms_gpu(case, "plain", x_dt, out_dt), case, "plain", out_dt)
    assert not fails, "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("cols", Q8_WIDTHS)
def test_rmsnorm_rope_q8_exact_probe(cols):
    """The int8 form: codes equal the oracle quantiser on every exact 128-column slice, both scale planes bit-equal (delta and
    -12582912 delta), scale_stride = 64 > rows with the gap untouched, out NULL and out present."""
    wi, fails = Q8_WIDTHS.index(cols), []
    for fi, (norm, rope) in enumerate(FLAGS):
        case = RmsCase(cols, 128, norm, rope, eps=(0.0, 1e-6)[fi % 2])
        for mi, mode in enumerate(("q8", "q8_noout")):
            x_dt, out_dt = DTS[(wi + fi + mi) % 3], DTS[(wi + 2 * fi + mi + 1) % 3]
            fails += check_rms_exact(rms_gpu(case, mode, x_dt, out_dt), case, mode, out_dt)
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


# ================================================================================================ LayerNorm + ViDiT transform (A)
def premul_of(cols, salt):
    h = hash32(salt, np.arange(cols), 21)
    return np.where(h & np.uint64(1), 1.0, -1.0) * np.where(h & np.uint64(2), 2.0, 1.0)


class RotCase:
    """37 rows of the LayerNorm probe (surplus lane groups recompute the last row), rows_per_batch = 3 (a batch boundary inside a
    wave for every form with several rows per wave), mod_stride = 6 cols, fp32 modulation; premul = +-1 times {1, 2}.  The
    normalised, modulated and pre-multiplied row is exact integers, the Hadamard sums t are exact integers below 2^24, and the value
    is t / sqrt(cols).  ln = False: the same integer rows go to wanq_rotate_quant_rows directly."""

    def __init__(self, had_k, ln=True, x_dt="bf16", mods=(True, True, True), nsets=1, rows=37, rpb=3, eps=0.0):
        self.had_k, self.cols, self.ln, self.x_dt, self.rows, self.rpb, self.eps, self.nsets = had_k, had_k * 128, ln, x_dt, rows, rpb, eps, nsets
        cols = self.cols
        self.nb = -(-rows // rpb)
        self.x, z = ln_probe_rows(rows, cols, salt=31)
        g, sh, sc = modulation(self.nb, cols)
        self.gamma, self.mshift, self.mscale = (g if mods[0] else None), (sh if mods[1] else None), (sc if mods[2] else None)
        self.premul = [premul_of(cols, s) for s in range(nsets)]
        y = ln_modulate(z, self.gamma, self.mshift, self.mscale, rpb) if ln else self.x
        self.y = [y * p for p in self.premul]
        self.v64 = [qr.matmul_hadU(v.astype(np.float64)) for v in self.y]  # t / float64(fp32 sqrt(cols))
        t = [v * float(np.sqrt(np.float32(cols))) for v in self.v64]
        assert all(np.abs(a - np.rint(a)).max() < 1e-6 and np.abs(a).max() < 2 ** 24 for a in t)

    def name(self):
        return f"had_k={self.had_k} ln={self.ln} x={self.x_dt} gamma/shift/scale={self.gamma is not None}/{self.mshift is not None}/{self.mscale is not None}"


# Codes of the transform.  With t the integer Hadamard sum and T = max |t| of the row, the exact quotient is R = 127 t / T; the 1 / sqrt
# cancels.  The kernel forms amax = fl(T cdiv), scale = fl(amax / 127), inv = fl(1 / scale), cinv = fl(cdiv inv) and rounds the exact
# product t cinv once (or, in a flagged chunk, fl(fl(t cdiv) / scale)): four roundings between R and the rounded value on either
# path, |value - R| <= ((1 + u)^4 - 1) |R|, and cdiv's own rounding (1 / sqrt(cols), then the reciprocal) cancels between cinv and
# scale.  The float64 pipeline (qr.matmul_hadU in float64, then qr.dynamic_quantize_sym, which quantises in fp32) has four as well:
# fl32(v64), the division by 127, the quotient, and the fp32 sqrt it shares with the kernel cancels likewise.  Both therefore give
# rne(R) unless R lies within ROT_DELTA of a half-integer.  With out_fp the kernel scales first (one product) and then has
# scale, inv and the product t' inv: four again.  The scale itself: cdiv = fl(1 / fl32 sqrt), the product with T, the division by
# 127 -- three roundings against T / float64(fp32 sqrt(cols)) / 127.
ROT_DELTA = ((1 + U) ** 4 - 1) * 127.5
ROT_SCALE_REL = (1 + U) ** 3 - 1


def near_tie_check(q, q_ref, ratio64, delta, what):
    """A code may differ from the reference's only where ratio64 lies within delta of a half-integer, and then by one.  Returns
    (failures, excused share): the share is computed from the reference alone."""
    dist = np.abs(ratio64 - np.floor(ratio64) - 0.5)
    excused = dist <= delta
    diff = np.abs(np.asarray(q, np.int64) - np.asarray(q_ref, np.int64))
    bad = (diff > 1) | ((diff != 0) & ~excused)
    fails = []
    if bad.any():
        r, c = [int(v) for v in np.argwhere(bad)[0]]
        fails.append(f"{what}: {int(bad.sum())} codes differ away from a tie; first at row {r} col {c}: got {q[r, c]} reference {q_ref[r, c]} "
                     f"quotient {ratio64[r, c]:.6f}")
    return fails, float(excused.mean())


def check_rot(o, case):
    """o: q [nsets][rows + 1, cols], scale, sum [nsets][rows + 1] (fp32 vectors), out (ln = False only) [rows + 1, cols] fp32."""
    rows, fails, shares = case.rows, [], []
    for s in range(case.nsets):
        v64 = case.v64[s]
        q_ref, _ = qr.dynamic_quantize_sym(v64, 8)
        s64 = np.abs(v64).max(axis=1) / 127.0
        f, share = near_tie_check(o["q"][s][:rows], q_ref, v64 / s64[:, None], ROT_DELTA, f"set {s} q")
        fails += f
        shares.append(share)
        if share > 0.01:
            fails.append(f"set {s}: {share:.4f} of the reference's own quotients lie within delta of a tie (cap 0.01)")
        sc = o["scale"][s][:rows]
        if not (np.abs(sc - s64) <= ROT_SCALE_REL * s64).all():
            fails.append(f"set {s} scale: largest relative deviation {np.abs(sc / s64 - 1).max():.3e} (bound {ROT_SCALE_REL:.3e})")
        own = (o["q"][s][:rows].sum(axis=1).astype(np.float32) * sc.astype(np.float32)).astype(np.float64)  # (float)tot * scale in fp32
        if not np.array_equal(o["sum"][s][:rows], own):
            fails.append(f"set {s} sum: not the kernel's own codes times its scale")
        if not ((o["q"][s][rows] == SENT8).all() and o["scale"][s][rows] == SENT and o["sum"][s][rows] == SENT):
            fails.append(f"set {s}: the row / slot after the last was written")
    if o.get("out") is not None:
        v64 = case.v64[0]
        pow2 = math.sqrt(case.cols) == int(math.sqrt(case.cols))  # inv_div is a power of two: t / sqrt(cols) is exact
        tol = 0.0 if pow2 else ((1 + U) ** 2 - 1)  # the reciprocal of the fp32 sqrt and one product
        if not (np.abs(o["out"][:rows] - v64) <= tol * np.abs(v64)).all():
            fails.append(f"out_fp: largest relative deviation {np.nanmax(np.abs(o['out'][:rows] - v64) / np.maximum(np.abs(v64), 1e-300)):.3e} (bound {tol:.3e})")
        if not (o["out"][rows] == SENT).all():
            fails.append("out_fp: the row after the last was written")
    return [f"{case.name()}: {f}" for f in fails]


def rot_model(case, bump=False):
    """Plain numpy model: LayerNorm model in fp32, the transform summed in float64 (exact on these integers) and scaled and
    quantised in fp32 the way the kernel does it.  bump: one code moved by one, away from any tie."""
    f = np.float32
    o = {"q": [], "scale": [], "sum": [], "out": None}
    inv_div = f(1) / np.sqrt(f(case.cols))
    for s in range(case.nsets):
        t = np.rint(case.v64[s] * float(np.sqrt(f(case.cols)))).astype(f)
        v = (t * inv_div).astype(f)
        q, sc, _ = kr.quant_sum(v)
        q = q.astype(np.int64)
        if bump:
            ratio = case.v64[s] / (np.abs(case.v64[s]).max(axis=1) / 127.0)[:, None]
            far = np.argwhere((np.abs(ratio - np.floor(ratio) - 0.5) > 0.25) & (np.abs(q) < 100))[0]
            q[tuple(far)] += 1
        sm = (q.sum(axis=1).astype(f) * sc).astype(np.float64)
        o["q"].append(with_sentinel_row(q, SENT8))
        o["scale"].append(with_sentinel_row(sc.astype(np.float64), SENT))
        o["sum"].append(with_sentinel_row(sm, SENT))
        if not case.ln and s == 0:
            o["out"] = with_sentinel_row(v.astype(np.float64), SENT)
    return o


def rot_gpu(case, multi=False):
    from viditq_extension import _C

    rows, cols, n = case.rows, case.cols, case.nsets
    xt = dev_t(case.x, case.x_dt)
    pm = [dev_t(p, "f32") for p in case.premul]
    q = [torch.full((rows + 1, cols), SENT8, dtype=torch.int8, device=DEV) for _ in range(n)]
    scale = [torch.full((rows + 1,), SENT, dtype=torch.float32, device=DEV) for _ in range(n)]
    ssum = [torch.full((rows + 1,), SENT, dtype=torch.float32, device=DEV) for _ in range(n)]
    out = None
    if case.ln:
        g, sh, sc, stride, keep = mod_tensors(case.gamma, case.mshift, case.mscale, case.nb, cols, "f32", True)
        if multi:
            _C.call("wanq_layernorm_rotate_quant_rows_multi", _C.ptr(xt), DTC[case.x_dt], _C.ptr(g), _C.ptr(sh), _C.ptr(sc), DTC["f32"], stride, case.rpb,
                    float(case.eps), n, _C.ptr_array(pm), case.had_k, _C.ptr_array(q), _C.ptr_array(scale), _C.ptr_array(ssum), DTC["f32"], rows, cols,
                    _C.stream())
        else:
            for s in range(n):
                _C.call("wanq_layernorm_rotate_quant_rows", _C.ptr(xt), DTC[case.x_dt], _C.ptr(g), _C.ptr(sh), _C.ptr(sc), DTC["f32"], stride, case.rpb,
                        float(case.eps), _C.ptr(pm[s]), case.had_k, _C.ptr(q[s]), _C.ptr(scale[s]), _C.ptr(ssum[s]), DTC["f32"], rows, cols, _C.stream())
    else:
        out = torch.full((rows + 1, cols), SENT, dtype=torch.float32, device=DEV)
        _C.call("wanq_rotate_quant_rows", _C.ptr(xt), DTC[case.x_dt], _C.ptr(pm[0]), case.had_k, _C.ptr(out), DTC["f32"], _C.ptr(q[0]), _C.ptr(scale[0]),
                _C.ptr(ssum[0]), DTC["f32"], rows, cols, _C.stream())
    torch.cuda.synchronize()
    return {"q": [t.cpu().to(torch.int64).numpy() for t in q], "scale": [t.cpu().double().numpy() for t in scale],
            "sum": [t.cpu().double().numpy() for t in ssum], "out": None if out is None else out.cpu().double().numpy()}


ROT_MODS = [(True, True, True), (False, True, True), (True, False, False), (False, False, False)]


@gpu
@pytest.mark.parametrize("had_k", ROT_HADK)
def test_layernorm_rotate_exact_probe(had_k):
    """wanq_layernorm_rotate_quant_rows on all eight forms: bf16 and fp32 rows, gamma / shift / scale present or NULL, eps 0 and
    1e-6; the codes against qr.dynamic_quantize_sym(qr.matmul_hadU(float64)) under the near-tie rule, the scale within three
    roundings, the sum exactly the kernel's own codes times its scale.  _multi with 2 and 3 sets equals the single calls bit for bit."""
    fails = []
    for i, mods in enumerate(ROT_MODS):
        case = RotCase(had_k, True, ("bf16", "f32")[i % 2], mods, eps=(0.0, 1e-6)[(i // 2) % 2])
        fails += check_rot(rot_gpu(case), case)
    for nsets in (2, 3):
        case = RotCase(had_k, True, "bf16", ROT_MODS[nsets - 2], nsets=nsets)
        single, multi = rot_gpu(case), rot_gpu(case, multi=True)
        fails += check_rot(single, case)
        for key in ("q", "scale", "sum"):
            for s in range(nsets):
                if not np.array_equal(single[key][s], multi[key][s]):
                    fails.append(f"{case.name()}: _multi with {nsets} sets: {key}[{s}] differs from the single call")
    assert not fails, f"{len(fails)} failures\n" + "\n".join(fails[:20])


@gpu
@pytest.mark.parametrize("had_k", [2, 4, 8, 16])
def test_rotate_exact_probe_without_layernorm(had_k):
    """wanq_rotate_quant_rows on the forms the tiny-model block tests rest on: out_fp == t / sqrt(cols) exactly at cols 256 and
    1024 (inv_div a power of two), within two roundings at 512 and 2048; codes, scale and sum as above."""
    fails = []
    for x_dt in ("bf16", "f32"):
        case = RotCase(had_k, False, x_dt)
        fails += check_rot(rot_gpu(case), case)
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ gate + residual (A)
GATE_DTYPES = [("bf16", "f32", "f32", "f32"), ("bf16", "bf16", "bf16", "bf16"), ("f16", "f16", "f16", "f16"), ("f16", "f32", "f32", "f32"),
               ("f32", "bf16", "f16", "bf16"), ("bf16", "f32", "bf16", "f16"), ("f32", "f32", "f32", "f32")]  # y, gate, residual, out


class GateCase:
    """y, gate and residual are small integers that encode (row, col) and (batch, col): out = y gate[b] + residual, |out| <= 21,
    exact in every dtype.  gate is chunk 2 of a [B, 6, cols] tensor (gate_stride = 6 cols) or a [B, cols] tensor.  Held as torch
    tensors on `device`, so that the one large case is generated and compared on the GPU."""

    def __init__(self, rows, cols, dts, rpb=3, wide=True, inplace=False, device="cpu"):
        self.rows, self.cols, self.dts, self.rpb, self.wide, self.inplace = rows, cols, dts, rpb, wide, inplace
        assert not inplace or dts[2] == dts[3]
        r = torch.arange(rows, device=device).view(-1, 1)
        c = torch.arange(cols, device=device).view(1, -1)
        self.nb = -(-rows // rpb)
        b = torch.arange(self.nb, device=device).view(-1, 1)
        self.y = ((r * 3 + c) % 11 - 5).to(TDT[dts[0]])
        self.gate = ((b * 5 + c * 2) % 7 - 3).to(TDT[dts[1]])
        self.res = ((r + 7 * c) % 13 - 6).to(TDT[dts[2]])
        self.expect = (self.y.float() * self.gate.float()[torch.div(r[:, 0], rpb, rounding_mode="floor")] + self.res.float())
        assert float(self.expect.abs().max()) <= 21

    def name(self):
        return f"rows={self.rows} cols={self.cols} dtypes={self.dts} wide={self.wide} inplace={self.inplace}"


def check_gate(out, case):
    """out: [rows + 1, cols] tensor of the output dtype, the last row a sentinel."""
    fails = []
    if not torch.equal(out[: case.rows].float(), case.expect):
        bad = torch.nonzero(out[: case.rows].float() != case.expect)
        r, c = [int(v) for v in bad[0]]
        fails.append(f"{bad.shape[0]} elements differ; first at row {r} col {c}: got {float(out[r, c])} expected {float(case.expect[r, c])}")
    if not bool((out[case.rows].float() == SENT).all()):
        fails.append("the row after the last was written")
    return [f"{case.name()}: {f}" for f in fails]


def gate_model(case):
    out = torch.full((case.rows + 1, case.cols), SENT, dtype=TDT[case.dts[3]], device=case.y.device)
    b = torch.div(torch.arange(case.rows, device=case.y.device), case.rpb, rounding_mode="floor")
    out[: case.rows] = (case.y.float() * case.gate.float()[b] + case.res.float()).to(TDT[case.dts[3]])
    return out


def gate_gpu(case):
    from viditq_extension import _C

    rows, cols = case.rows, case.cols
    if case.wide:
        g = torch.full((case.nb, 6, cols), 99.0, dtype=TDT[case.dts[1]], device=DEV)
        g[:, 2] = case.gate.to(DEV)
        gate, stride = g[:, 2], 6 * cols
    else:
        gate, stride = case.gate.to(DEV).contiguous(), cols
    y = case.y.to(DEV).contiguous()
    res = torch.full((rows + 1, cols), SENT, dtype=TDT[case.dts[2]], device=DEV)
    res[:rows] = case.res.to(DEV)
    out = res if case.inplace else torch.full((rows + 1, cols), SENT, dtype=TDT[case.dts[3]], device=DEV)
    _C.call("wanq_gate_residual", _C.ptr(y), DTC[case.dts[0]], _C.ptr(gate), DTC[case.dts[1]], stride, _C.ptr(res), DTC[case.dts[2]], _C.ptr(out),
            DTC[case.dts[3]], rows, cols, case.rpb, _C.stream())
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("cols", [8, 520, 1536, 16384])
def test_gate_residual_exact_probe(cols):
    """11 rows, rows_per_batch = 3, gate_stride = 6 cols and cols, every dtype quadruple, and in place (out == residual)."""
    fails = []
    for i, dts in enumerate(GATE_DTYPES):
        case = GateCase(11, cols, dts, wide=(i % 3 != 2))
        fails += check_gate(gate_gpu(case).cpu(), case)
        if dts[2] == dts[3]:
            case = GateCase(11, cols, dts, wide=(i % 2 == 0), inplace=True)
            fails += check_gate(gate_gpu(case).cpu(), case)
    assert not fails, "\n".join(fails[:20])


@gpu
def test_gate_residual_grid_stride_second_turn():
    """2200 x 8192 bf16: 2 252 800 chunks > 8192 * 256 = 2 097 152 threads, so the grid-stride loop takes a second turn."""
    assert 2200 * (8192 // 8) > 8192 * 256
    case = GateCase(2200, 8192, ("bf16", "f32", "bf16", "bf16"), rpb=3, wide=True, device=DEV)
    fails = check_gate(gate_gpu(case), case)
    assert not fails, "\n".join(fails)


# ================================================================================================ B. random data, derived bounds
# The derivations are in profiles/PARITY_NOTES.md ("Row-wise norm kernels"); u = 2^-24.
def sum_depth(wpr, nch):
    """Additions between one element and the row total: 8 NCH - 1 in the lane, 6 wave exchange steps, 3 over the LDS slots."""
    return 8 * nch - 1 + 6 + (3 if wpr == 4 else 0)


SECOND_ORDER = 1 + 2.0 ** -10  # products of two first-order terms (each below 2^-10 relative on these inputs)


class LnRandomCase:
    """13 rows, rows_per_batch = 5, mod_stride = 6 cols, fp32 modulation (Gaussian), eps = 1e-6; out_fp, q, scale and sum."""

    def __init__(self, cols, kind, dt, seed, gamma=True):
        self.cols, self.kind, self.dt, self.rows, self.rpb, self.eps = cols, kind, dt, 13, 5, 1e-6
        self.nb = 3
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(self.rows, cols, generator=g, dtype=torch.float64)
        if kind == "gauss":  # per-column log-normal scales
            x = x * torch.exp(torch.randn(cols, generator=g, dtype=torch.float64))
        elif kind == "shifted":  # exercises the cancellation term
            x = x + 64.0
        else:  # one outlier column of 30 sigma
            x[:, 17 % cols] = 30.0 * torch.sign(x[:, 17 % cols])
        self.x = rnd(x.numpy(), dt)
        f32 = lambda t: t.float().double().numpy()
        self.gamma = f32(1.0 + 0.5 * torch.randn(cols, generator=g)) if gamma else None
        self.mshift = f32(0.5 * torch.randn(self.nb, cols, generator=g))
        self.mscale = f32(0.3 * torch.randn(self.nb, cols, generator=g))
        self.cfg = LnCfg(dt, "f32", dt, True, True, "f32", gamma, True, True, True)
        self._bound()

    def name(self):
        return f"cols={self.cols} {self.kind} {self.dt} gamma={self.gamma is not None}"

    def _bound(self):
        x, n = self.x, self.cols
        k = sum_depth(*form_of(n))
        mean = x.mean(axis=1)
        d = x - mean[:, None]
        rstd = 1.0 / np.sqrt((d * d).mean(axis=1) + float(np.float32(self.eps)))
        z = d * rstd[:, None]
        b = np.arange(self.rows) // self.rpb
        G = np.abs((1.0 if self.gamma is None else self.gamma) * (1.0 + self.mscale[b]))
        self.y64 = ln_modulate(z, self.gamma, self.mshift, self.mscale, self.rpb)
        cancel = (k + 1) * U * np.abs(x).max(axis=1) * rstd  # the error of the mean, (k + 1) u max|x|, in units of the normalised row
        rho = ((k + 4) * U + cancel ** 2) / 2 + 2.5 * U  # relative error of rstd
        n_mod = (1 if self.gamma is not None else 0) + 2
        e = G * (np.abs(z) * (rho + 2 * U)[:, None] + cancel[:, None]) + np.abs(z) * G * n_mod * U + U * np.abs(self.y64)
        self.bound32 = e * SECOND_ORDER  # on the fp32 value that is stored or quantised
        self.bound_out = self.bound32 + U_OUT[self.dt] * (np.abs(self.y64) + self.bound32) + (2.0 ** -25 if self.dt == "f16" else 0.0)
        # codes: quotient y / scale with scale = fl(amax / 127): the element's own error, the error of the row maximum scaled by
        # the quotient, two roundings of the kernel's quantiser and four of the reference's fp32 quantiser (kr.quant_sum)
        amax = np.abs(self.y64).max(axis=1)
        self.s64 = amax / 127.0
        self.ratio = self.y64 / self.s64[:, None]
        self.delta = self.bound32 / self.s64[:, None] + np.abs(self.ratio) * (self.bound32.max(axis=1) / amax + 6 * U)[:, None]
        self.q_ref, _, _ = kr.quant_sum(self.y64.astype(np.float32))


def check_ln_random(o, case):
    """Returns (failures, largest err / bound of out_fp, excused share)."""
    rows, fails = case.rows, []
    err = np.abs(o["out"][:rows] - case.y64)
    ratio = float(np.nan_to_num(err / case.bound_out, nan=np.inf).max())
    if not (err <= case.bound_out).all():
        bad = ~(err <= case.bound_out)
        r, c = [int(v) for v in np.argwhere(bad)[0]]
        fails.append(f"out_fp: {int(bad.sum())} elements out of bound, err / bound {ratio:.3f}; first at row {r} col {c}: got {o['out'][r, c]} y64 {case.y64[r, c]}")
    f, share = near_tie_check(o["q"][:rows], case.q_ref, case.ratio, case.delta, "q")
    fails += f
    if share > 0.01:
        fails.append(f"{share:.4f} of the reference's own quotients lie within delta of a tie (cap 0.01)")
    rel = case.bound32.max(axis=1) / (case.s64 * 127.0) + 2 * U
    if not (np.abs(o["scale"][:rows] - case.s64) <= rel * case.s64).all():
        fails.append(f"scale: largest relative deviation {np.abs(o['scale'][:rows] / case.s64 - 1).max():.3e}")
    own = (o["q"][:rows].sum(axis=1).astype(np.float32) * o["scale"][:rows].astype(np.float32)).astype(np.float64)
    if not np.array_equal(o["sum"][:rows], own):
        fails.append("sum: not the kernel's own codes times its scale")
    return [f"{case.name()}: {f}" for f in fails], ratio, share


B_WIDTHS = [264, 1536, 5120, 13824]
LN_RANDOM = [("gauss", "f32", True), ("gauss", "bf16", False), ("gauss", "f16", True), ("shifted", "f32", True), ("outlier", "f32", False),
             ("outlier", "bf16", True)]


def ln_random_cases(cols):
    return [LnRandomCase(cols, kind, dt, seed=cols * 10 + i, gamma=gm) for i, (kind, dt, gm) in enumerate(LN_RANDOM)]


@gpu
@pytest.mark.parametrize("cols", B_WIDTHS)
def test_layernorm_random_under_the_derived_bound(cols):
    fails = []
    for case in ln_random_cases(cols):
        f, ratio, share = check_ln_random(ln_gpu(case), case)
        print(f"PROBE layernorm {case.name()}: largest err/bound {ratio:.3f}, excused share {share:.5f}")
        fails += f
    assert not fails, "\n".join(fails[:20])


class RmsRandomCase:
    """13 rows, rows_per_batch = 5, positions = 4, eps = 1e-6, a unit-modulus table of random angles rounded to fp32, Gaussian
    weight; head_dim 128 where it divides the width, else 8."""

    def __init__(self, cols, kind, x_dt, out_dt, seed):
        self.cols, self.kind, self.x_dt, self.out_dt = cols, kind, x_dt, out_dt
        self.rows, self.rpb, self.positions, self.eps, self.norm, self.rope = 13, 5, 4, 1e-6, True, True
        self.hd = 128 if cols % 128 == 0 else 8
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(self.rows, cols, generator=g, dtype=torch.float64)
        if kind == "gauss":
            x = x * torch.exp(torch.randn(cols, generator=g, dtype=torch.float64))
        elif kind == "shifted":
            x = x + 64.0
        else:
            x[:, 17 % cols] = 30.0 * torch.sign(x[:, 17 % cols])
        self.x = rnd(x.numpy(), x_dt)
        self.weight = (1.0 + 0.5 * torch.randn(cols, generator=g)).float().double().numpy()
        ang = torch.rand(self.positions, self.hd // 2, generator=g, dtype=torch.float64) * 2 * math.pi
        self.table = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float().double().numpy()
        self._bound()

    definition = RmsCase.definition

    def name(self):
        return f"cols={self.cols} {self.kind} {self.x_dt}->{self.out_dt}"

    def _bound(self):
        x, n = self.x, self.cols
        k = sum_depth(*form_of(n)) + 1  # + the square
        rinv = 1.0 / np.sqrt((x * x).mean(axis=1) + float(np.float32(self.eps)))
        rho = (k + 2) * U / 2 + 2 * U  # sum, division, + eps under the square root; the square root; the reciprocal
        nrm = x * rinv[:, None] * self.weight
        en = np.abs(nrm) * (rho + 2 * U)  # x rinv and the product with weight
        pos = np.arange(self.rows) % self.rpb
        rot = (pos < self.positions)[:, None]
        pair = (np.arange(n) % self.hd) // 2
        cs = self.table[np.minimum(pos, self.positions - 1)][:, pair[0::2]]
        c, s = np.abs(cs[..., 0]), np.abs(cs[..., 1])
        a, b, ea, eb = nrm[:, 0::2], nrm[:, 1::2], en[:, 0::2], en[:, 1::2]
        y = nrm.copy()
        ya, yb = a * cs[..., 0] - b * cs[..., 1], a * cs[..., 1] + b * cs[..., 0]
        y[:, 0::2], y[:, 1::2] = np.where(rot, ya, a), np.where(rot, yb, b)
        e = en.copy()  # fma(a, cos, -fl(b sin)): the errors of a and b, the product b sin, the result
        e[:, 0::2] = np.where(rot, ea * c + eb * s + U * np.abs(b) * s + U * np.abs(ya), ea)
        e[:, 1::2] = np.where(rot, ea * s + eb * c + U * np.abs(b) * c + U * np.abs(yb), eb)
        self.y64, self.bound32 = y, e * SECOND_ORDER
        self.bound_out = self.bound32 + U_OUT[self.out_dt] * (np.abs(y) + self.bound32) + (2.0 ** -25 if self.out_dt == "f16" else 0.0)


def check_rms_random(o, case):
    err = np.abs(o["out"][: case.rows] - case.y64)
    ratio = float(np.nan_to_num(err / case.bound_out, nan=np.inf).max())
    fails = []
    if not (err <= case.bound_out).all():
        bad = ~(err <= case.bound_out)
        r, c = [int(v) for v in np.argwhere(bad)[0]]
        fails.append(f"{case.name()}: {int(bad.sum())} elements out of bound, err / bound {ratio:.3f}; first at row {r} col {c}: got {o['out'][r, c]} y64 {case.y64[r, c]}")
    return fails, ratio


RMS_RANDOM = [("gauss", "f32", "f32"), ("gauss", "bf16", "bf16"), ("gauss", "f16", "f16"), ("gauss", "f32", "bf16"), ("shifted", "f32", "f32"),
              ("outlier", "f32", "f32"), ("outlier", "bf16", "f32")]


def rms_random_cases(cols):
    return [RmsRandomCase(cols, kind, x_dt, out_dt, seed=cols * 10 + 5 + i) for i, (kind, x_dt, out_dt) in enumerate(RMS_RANDOM)]


@gpu
@pytest.mark.parametrize("cols", B_WIDTHS)
def test_rmsnorm_rope_random_under_the_derived_bound(cols):
    fails = []
    for case in rms_random_cases(cols):
        f, ratio = check_rms_random(rms_gpu(case, "plain", case.x_dt, case.out_dt), case)
        print(f"PROBE rmsnorm_rope {case.name()}: largest err/bound {ratio:.3f}")
        fails += f
    assert not fails, "\n".join(fails[:20])


# ================================================================================================ C. refusals and no-ops
def _abi_call(entry, rows=5, cols=256, rpb=3, hd=128, had_k=None, mod="f32", stride=None, q8_hd=None):
    """Argument list of one entry point on small valid buffers (sized for max(rows, 1) rows of min(cols, 16384) + 8 columns; a refused
    call reads none of them).  Returns (args, outputs that must keep their sentinel)."""
    from viditq_extension import _C

    n = max(rows, 1)
    w = min(max(cols, 8), 16384) + 8
    x = torch.zeros(n, w, dtype=torch.float32, device=DEV)
    vecs = torch.zeros(3, 6 * w, dtype=TDT[mod], device=DEV)
    f32v = torch.ones(w * 2, dtype=torch.float32, device=DEV)
    out = torch.full((n, w), SENT, dtype=torch.float32, device=DEV)
    q = torch.full((n, w), SENT8, dtype=torch.int8, device=DEV)
    sc = torch.full((2 * n * 64 * (w // 128 + 1),), SENT, dtype=torch.float32, device=DEV)
    sm = torch.full((n,), SENT, dtype=torch.float32, device=DEV)
    p, st, F = _C.ptr, _C.stream(), DTC["f32"]
    had_k = cols // 128 if had_k is None else had_k
    if entry == "wanq_layernorm_rows":
        args = [p(x), F, p(vecs[0]), p(vecs[1]), p(vecs[2]), DTC[mod], w, rpb, 1e-6, p(out), F, p(q), p(sc), p(sm), F, rows, cols, st]
    elif entry == "wanq_gate_residual":
        args = [p(x), F, p(vecs[0]), DTC[mod], w, p(x), F, p(out), F, rows, cols, rpb, st]
    elif entry == "wanq_rmsnorm_rope":
        args = [p(x), F, p(f32v), p(f32v), p(out), F, rows, cols, hd, rpb, 1, 1e-6, st]
    elif entry == "wanq_rmsnorm_rope_q8":
        args = [p(x), F, p(f32v), p(f32v), p(out), F, p(q), p(sc), (64 if stride is None else stride), rows, cols, hd, rpb, 1, 1e-6, st]
    elif entry == "wanq_rmsnorm_rope_scatter":
        hm = torch.zeros(2 * (w // 8), dtype=torch.int64, device=DEV)
        args = [p(x), F, p(f32v), p(f32v), p(out), F, p(hm), rows, cols, hd, rpb, 1, 1e-6, st]
    elif entry == "wanq_rotate_quant_rows":
        args = [p(x), F, p(f32v), had_k, p(out), F, p(q), p(sc), p(sm), F, rows, cols, st]
    elif entry == "wanq_layernorm_rotate_quant_rows":
        args = [p(x), F, p(vecs[0]), p(vecs[1]), p(vecs[2]), DTC[mod], w, rpb, 1e-6, p(f32v), had_k, p(q), p(sc), p(sm), F, rows, cols, st]
    else:
        assert entry == "wanq_layernorm_rotate_quant_rows_multi"
        args = [p(x), F, p(vecs[0]), p(vecs[1]), p(vecs[2]), DTC[mod], w, rpb, 1e-6, 1, _C.ptr_array([f32v]), had_k, _C.ptr_array([q]),
                _C.ptr_array([sc]), _C.ptr_array([sm]), F, rows, cols, st]
    return args, (out, q, sc, sm), (x, vecs, f32v)


ENTRIES = ["wanq_layernorm_rows", "wanq_gate_residual", "wanq_rmsnorm_rope", "wanq_rmsnorm_rope_q8", "wanq_rmsnorm_rope_scatter",
           "wanq_rotate_quant_rows", "wanq_layernorm_rotate_quant_rows", "wanq_layernorm_rotate_quant_rows_multi"]
ROT_ENTRIES = ENTRIES[5:]


def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((t == (SENT8 if t.dtype == torch.int8 else SENT)).all()) for t in outs)


@gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_no_rows_is_ok_and_writes_nothing(entry):
    from viditq_extension import _C

    args, outs, keep = _abi_call(entry, rows=0)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK
    assert _untouched(outs)


@gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_shape_rules_are_refused_through_the_abi(entry):
    """Each rule returns its documented code with a message that names it, before anything is enqueued (the outputs keep their
    sentinel).  The transform entry points state their width rule as cols == had_k * 128 (had_k = 0: the multiple-of-8 rule)."""
    from viditq_extension import _C

    rot = entry in ROT_ENTRIES
    rules = []
    if rot:
        rules += [(dict(cols=260, had_k=0), WANQ_E_SHAPE, "must be a multiple of 8"), (dict(cols=16392, had_k=0), WANQ_E_SHAPE, "must be a multiple of 8"),
                  (dict(cols=260, had_k=2), WANQ_E_SHAPE, "must be had_k * 128"), (dict(cols=512, had_k=2), WANQ_E_SHAPE, "must be had_k * 128"),
                  (dict(cols=16512, had_k=129), WANQ_E_SHAPE, "no fused Hadamard transform")]
    elif entry == "wanq_rmsnorm_rope_q8":  # (its own width rule comes first: whole heads of 128 columns)
        rules += [(dict(cols=260), WANQ_E_ARG, "cols % 128 == 0"), (dict(cols=16512), WANQ_E_SHAPE, "must be a multiple of 8")]
    else:
        rules += [(dict(cols=260), WANQ_E_SHAPE, "must be a multiple of 8"), (dict(cols=16392), WANQ_E_SHAPE, "must be a multiple of 8")]
    if entry in ("wanq_layernorm_rows", "wanq_gate_residual", "wanq_layernorm_rotate_quant_rows", "wanq_layernorm_rotate_quant_rows_multi"):
        rules.append((dict(rpb=0), WANQ_E_ARG, "rows_per_batch must be >= 1"))
    if entry.startswith("wanq_rmsnorm_rope"):
        rules.append((dict(rpb=0), WANQ_E_SHAPE, "bad rows"))
        if entry != "wanq_rmsnorm_rope_q8":
            rules.append((dict(cols=256, hd=96), WANQ_E_SHAPE, "must be a multiple of 8 dividing cols"))
        else:
            rules += [(dict(cols=256, hd=64), WANQ_E_ARG, "head_dim == 128"), (dict(rows=5, stride=4), WANQ_E_ARG, "scale_stride >= rows")]
    if entry.startswith("wanq_layernorm_rotate"):
        rules += [(dict(mod="bf16"), WANQ_E_ARG, "must be fp32 here"), (dict(mod="f16"), WANQ_E_ARG, "must be fp32 here")]
    for kw, code, message in rules:
        args, outs, keep = _abi_call(entry, **kw)
        assert getattr(_C.lib, entry)(*args) == code, (entry, kw)
        assert message in _C.lib.wanq_last_error().decode(), (kw, _C.lib.wanq_last_error().decode())
        assert _untouched(outs), kw


# ================================================================================================ E. CPU self-tests of the probes
CPU_LN_WIDTHS = [8, 264, 512, 1032, 2056, 5120, 8200, 13824, 14344, 16384]


def test_width_tables_reach_every_form():
    """The smallest and the largest width of each (WPR, NCH) form of the dispatch ladder, for every width table, and all eight had_k."""
    for widths in (LN_WIDTHS, RMS_WIDTHS, Q8_WIDTHS):
        lo = 0
        for limit, wpr, nch in FORMS:
            mine = [w for w in widths if lo < w // 8 <= limit]
            step = 128 if widths is Q8_WIDTHS else 8
            assert limit * 8 in mine and min(mine) <= (lo * 8 // step + 1) * step, (wpr, nch, mine)
            assert all(form_of(w) == (wpr, nch) for w in mine)
            lo = limit
    assert {5120, 8960, 13824} <= set(LN_WIDTHS) and 8 in LN_WIDTHS and 8 in RMS_WIDTHS
    assert sorted(k * 128 for k in ROT_HADK) == [128, 256, 512, 1024, 1536, 2048, 4096, 5120]
    assert all(w % 128 == 0 for w in Q8_WIDTHS)


def test_generator_refuses_unbalanced_signs():
    ln_probe_rows(11, 264)
    for unbalance in (1, -1):
        with pytest.raises(ValueError):
            ln_probe_rows(11, 264, unbalance=unbalance)


def test_expected_values_are_exact_in_every_dtype():
    """Every expected value of section A, and every input, survives a rounding into each dtype it is stored or compared in."""
    for cols in (8, 264, 5120, 16384):
        for case in ln_cases(cols):
            for dt in DTS:
                assert np.array_equal(rnd(case.expect, dt), case.expect) and np.array_equal(rnd(case.x, dt), case.x)
                for m in (case.gamma, case.mshift, case.mscale):
                    assert m is None or np.array_equal(rnd(m, dt), m)
    for cols in (8, 520, 16384):
        for hd in head_dims(cols):
            for norm, rope in FLAGS:
                case = RmsCase(cols, hd, norm, rope)
                for dt in DTS:
                    assert np.array_equal(rnd(case.expect, dt), case.expect) and np.array_equal(rnd(case.x, dt), case.x)
    for dts in GATE_DTYPES:
        case = GateCase(11, 520, dts)
        for dt in DTS:
            assert torch.equal(case.expect.to(TDT[dt]).float(), case.expect)
        assert torch.equal(case.y.float(), (case.y.float()).round()) and float(case.gate.float().abs().max()) <= 3
    for had_k in (1, 12):
        case = RotCase(had_k, True, "bf16")
        assert np.array_equal(rnd(case.x, "bf16"), case.x) and np.array_equal(case.y[0], np.rint(case.y[0]))


@pytest.mark.parametrize("cols", CPU_LN_WIDTHS)
def test_model_passes_the_layernorm_probe(cols):
    fails = []
    for case in ln_cases(cols):
        fails += check_ln_exact(ln_model(case), case)
    assert not fails, "\n".join(fails[:10])


def _ln_mutant_caught(mutant, widths):
    return [cols for cols in widths if any(check_ln_exact(ln_model(case, mutant), case) for case in ln_cases(cols, with_const_row=False))]


@pytest.mark.parametrize("mutant", ["gamma_lane", "neighbour_batch", "drop_last_partial_chunk"])
def test_layernorm_mutants_fail_the_exact_probe(mutant):
    """(The one-pass variance is the business of section B: on integer rows its fp32 sums of squares can come out exact.  It
    fails the shifted set there, test_random_cases_model_within_bound_and_tie_cap_on_the_reference.)"""
    caught = _ln_mutant_caught(mutant, [264, 1032, 2056, 13824])
    assert 264 in caught and 13824 in caught, (mutant, caught)


def test_model_passes_and_mutants_fail_the_rmsnorm_probe():
    for cols, hd in ((8, 8), (520, 8), (1536, 128), (4224, 128), (12296, 8)):
        for norm, rope in FLAGS:
            case = RmsCase(cols, hd, norm, rope, eps=1e-6)
            for mode in ("plain", "scatter") + (("q8", "q8_noout") if hd == 128 else ()):
                assert not check_rms_exact(rms_model(case, mode, "bf16", "f16"), case, mode)
    case = RmsCase(1536, 128)
    assert check_rms_exact(rms_model(case, "plain", mutant="rope_on_padding"), case, "plain")
    assert check_rms_exact(rms_model(case, "plain", mutant="pos_is_row"), case, "plain")
    assert check_rms_exact(rms_model(case, "q8", mutant="pos_is_row"), case, "q8")
    assert check_rms_exact(rms_model(case, "scatter", mutant="swap_heads"), case, "scatter")
    assert not check_rms_exact(rms_model(case, "scatter"), case, "scatter")


@pytest.mark.parametrize("had_k", ROT_HADK)
def test_model_passes_the_transform_probe_and_a_moved_code_fails(had_k):
    """Also the near-tie cap on the reference alone, for every case the GPU tests run."""
    for i, mods in enumerate(ROT_MODS):
        case = RotCase(had_k, True, ("bf16", "f32")[i % 2], mods)
        assert not check_rot(rot_model(case), case), case.name()
    for nsets in (2, 3):
        case = RotCase(had_k, True, "bf16", ROT_MODS[nsets - 2], nsets=nsets)
        assert not check_rot(rot_model(case), case), case.name()
    if had_k in (2, 4, 8, 16):
        for x_dt in ("bf16", "f32"):
            case = RotCase(had_k, False, x_dt)
            assert not check_rot(rot_model(case), case), case.name()
    case = RotCase(had_k, True, "bf16")
    fails = check_rot(rot_model(case, bump=True), case)
    assert fails and "away from a tie" in fails[0]


def test_model_passes_the_gate_probe():
    for cols in (8, 520):
        for i, dts in enumerate(GATE_DTYPES):
            case = GateCase(11, cols, dts, wide=(i % 2 == 0))
            assert not check_gate(gate_model(case), case)
            bad = gate_model(case)
            bad[3] = bad[2]
            assert check_gate(bad, case)


@pytest.mark.parametrize("cols", B_WIDTHS)
def test_random_cases_model_within_bound_and_tie_cap_on_the_reference(cols):
    """The fp32 two-pass model lies inside the derived bounds, the excused share of the float64 reference alone is <= 1 % in every
    case, the one-pass variance leaves the bound on the shifted set, and a code moved by one away from a tie is caught."""
    for case in ln_random_cases(cols):
        fails, ratio, share = check_ln_random(ln_model(case), case)
        assert not fails and ratio < 1 and share <= 0.01, (fails, ratio, share)
        if case.kind == "shifted":
            fails, ratio, _ = check_ln_random(ln_model(case, "one_pass_variance"), case)
            assert fails and ratio > 1, (case.name(), ratio)
    o = ln_model(case)
    far = np.argwhere((np.abs(case.ratio - np.floor(case.ratio) - 0.5) > 0.25) & (np.abs(case.q_ref) < 100))[0]
    o["q"][tuple(far)] += 1
    assert any("away from a tie" in f for f in check_ln_random(o, case)[0])
    for case in rms_random_cases(cols):
        fails, ratio = check_rms_random(rms_model(case, "plain", case.x_dt, case.out_dt), case)
        assert not fails and ratio < 1, (fails, ratio)
