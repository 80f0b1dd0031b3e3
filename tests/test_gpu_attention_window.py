"""Sliding-window local attention (csrc/attention.hip, WIN; wanq_attention_window_fwd; wan.ops.attention(window=...)) against
the float64 definition computed here:

    query i sees key j  iff  i + off - left <= j <= i + off + right  and  0 <= j < Lk,   off = Lk - Lq,
    a negative side is unbounded, a query that sees no key gets a row of zeros.

As in tests/test_gpu_attention_probes.py the operands are small integers times powers of two, exact in bf16 and in fp16, so every
score is exact and the expected value of the exact families is a count over the window:
  A  census        every score 0, V a binary code of the key index: o[i] = mean of V over i's window at one rounding of the output
                   type.  A key wrongly added or dropped at a band edge moves a count by 1.
  B  poison        in-window scores 0, every out-of-window key 2^7 log2 units higher (a leaked key takes the whole row).  The score
                   matrix 128 * [j outside the band of i] has full rank and q.k has rank 128, so a launch carries the pattern for
                   128 queries (q = one-hot of the query, k = the pattern's columns) and five launches cover the 600; every key
                   that NO checked query of a launch sees holds V = SENTINEL, the others the census code.
  C  first visible tile   every visible score -200, and again +150 log2 units: a row whose masked leading tiles had fixed its
                   reference at 0 or at -inf comes out as zeros or NaN.
  D  random data   |o - o64| <= (2^-8 + 2^-14) (P64 |V|) + 2^-9 |o64| with P64 the masked float64 map (family C of the probe file;
                   fp16: 2^-10 + 2^-14, 2^-11 and that file's range term over the visible keys).
  E  Lq != Lk, k_len in front of decoy keys, rows that see nothing.
  F  windows (-1, -1) and (5000, 5000) are bit-equal to wanq_attention_fwd.
  G  stores stay inside their rows' columns; rows of query blocks with an empty band are written as zeros.
  H  wan.ops.attention: window with splits > 1 is refused; without a window the output is today's, bit for bit, split path included.
  I  the FP WanModel and the kernel-mode block with window_size=(40, 40) against the same module with wan.ops.attention replaced
     by the float64 masked definition, and against their dense selves.
Every family of A-G runs on bf16 and fp16 with 8 and with 4 waves, forced by wanq_attention_select_form and restored."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
SENTINEL = -7776.0  # exact in bf16, fp16 and fp32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMS = {  # name -> (dtype, wanq_attention_select_form value, relative rounding of the output type)
    "bf16-8w": (torch.bfloat16, 0, 2.0 ** -8),
    "bf16-4w": (torch.bfloat16, 1 << 40, 2.0 ** -8),
    "fp16-8w": (torch.float16, 0, 2.0 ** -11),
    "fp16-4w": (torch.float16, 1 << 40, 2.0 ** -11),
}
H0, L0 = 2, 600  # three 256-query (five 128-query) blocks, ten key tiles, the last one ragged with 24 keys
WINDOWS = [(0, 0), (1, 0), (0, 1), (63, 64), (64, 63), (100, 37), (255, 0), (0, 255), (-1, 17), (17, -1), (599, 599), (5000, 5000)]
# scale * log2(e) = 2^-3 and 2^-4 exactly in fp32 (asserted below): the kernel's rounding of q * c is then exact
POW2_SCALES = [float(np.float32(2.0 ** -3 / math.log2(math.e))), float(np.float32(2.0 ** -4 / math.log2(math.e)))]


def test_scale_times_log2e_is_a_power_of_two_in_fp32():
    log2e = np.float32(1.4426950408889634)
    assert np.float32(POW2_SCALES[0]) * log2e == np.float32(0.125) and np.float32(POW2_SCALES[1]) * log2e == np.float32(0.0625)


# ---------------------------------------------------------------------------------------------------------------- the definition
def band(Lq, Lk, window):
    """(lo, hi) int64 [Lq]: query i sees keys lo[i] ... hi[i]; hi < lo where it sees none."""
    left, right = window
    i = torch.arange(Lq, dtype=torch.int64)
    off = Lk - Lq
    lo = torch.zeros(Lq, dtype=torch.int64) if left < 0 else (i + off - left).clamp(min=0)
    hi = torch.full((Lq,), Lk - 1, dtype=torch.int64) if right < 0 else (i + off + right).clamp(max=Lk - 1)
    return lo, hi


def band_mask(Lq, Lk, window):
    lo, hi = band(Lq, Lk, window)
    j = torch.arange(Lk, dtype=torch.int64).unsqueeze(0)
    return (j >= lo.unsqueeze(1)) & (j <= hi.unsqueeze(1))  # [Lq, Lk]


def window_mean(v, Lq, Lk, window):
    """float64 mean of v[:Lk] ([Lk, C]) over every query's window, zeros where the window is empty: [Lq, C]."""
    lo, hi = band(Lq, Lk, window)
    cs = torch.cat([torch.zeros(1, v.shape[1], dtype=torch.float64), v[:Lk].double().cumsum(0)])
    n = (hi - lo + 1).clamp(min=0)
    s = cs[(hi + 1).clamp(min=0)] - cs[lo.clamp(max=Lk)]
    return torch.where(n.unsqueeze(1) > 0, s / n.clamp(min=1).unsqueeze(1), torch.zeros_like(s))


def definition64(q, k, v, H, Lk, window, scale):
    """o64 = softmax over the visible keys (q k^T scale) v, P64 |v| and the scores in log2 units [H, Lq, Lk] (-inf where masked),
    float64 on the GPU; rows without a visible key are zero."""
    Lq = q.shape[0]
    q64, k64, v64 = (t.to(DEV).double().reshape(t.shape[0], H, D) for t in (q, k[:Lk], v[:Lk]))
    t = torch.einsum("qhd,khd->hqk", q64, k64) * (float(np.float32(scale)) * math.log2(math.e))
    t = t.masked_fill(~band_mask(Lq, Lk, window).to(DEV).unsqueeze(0), float("-inf"))
    m = t.max(dim=-1, keepdim=True).values
    w = torch.exp2(t - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = w.sum(dim=-1, keepdim=True)
    p = w / torch.where(l > 0, l, torch.ones_like(l))
    o = torch.einsum("hqk,khd->qhd", p, v64).reshape(Lq, -1)
    a = torch.einsum("hqk,khd->qhd", p, v64.abs()).reshape(Lq, -1)
    return o, a, t, p


def run(form, q, k, v, H, Lk, window, scale=POW2_SCALES[0], out=None, entry="wanq_attention_window_fwd"):
    """One launch through the C ABI on the form's type and workgroup size; q / k / v fp32 tensors whose values both types hold."""
    from viditq_extension import _C

    dtype, sel, _ = FORMS[form]
    qd, kd, vd = (t.to(DEV).to(dtype).contiguous() for t in (q, k, v))
    for a, b in ((qd, q), (kd, k), (vd, v)):
        assert torch.equal(a.float().cpu(), b.float().cpu()), "operands must be exact in the form's type"
    Lq = q.shape[0]
    if out is None:
        out = torch.full((Lq, H * D), float("nan"), dtype=dtype, device=DEV)
    prev = _C.lib.wanq_attention_select_form(sel)
    try:
        args = [_C.ptr(qd), _C.ptr(kd), _C.ptr(vd), _C.ptr(out), _C.dt(dtype), Lq, Lk, H, D, qd.stride(0), kd.stride(0), vd.stride(0),
                out.stride(0), float(scale)]
        if entry == "wanq_attention_window_fwd":
            args += [int(window[0]), int(window[1])]
        _C.call(entry, *args, _C.stream())
    finally:
        _C.lib.wanq_attention_select_form(prev)
    return out


def census_code(n_keys, H, seed=5):
    """v[k, h, :] in {0, 1}: the bits of the key index and their complements, the one-hot of k mod 64 and of (k >> 6) & 3, random
    bits; rotated by 17 channels per head so that a head mix-up shows too."""
    k = torch.arange(n_keys)
    v = torch.zeros(n_keys, H, D)
    for b in range(12):
        v[:, :, b] = ((k >> b) & 1).float().unsqueeze(-1)
        v[:, :, 12 + b] = 1.0 - v[:, :, b]
    v[k, :, 24 + (k % 64)] = 1.0
    v[k, :, 88 + ((k >> 6) & 3)] = 1.0
    v[:, :, 92:] = (torch.rand(n_keys, H, D - 92, generator=torch.Generator().manual_seed(seed)) < 0.25).float()
    for h in range(H):
        v[:, h] = torch.roll(v[:, h], 17 * h, dims=-1)
    return v.reshape(n_keys, H * D)


def check_counts(out, expect, rel, what, rows=None):
    """|o - mean| <= rel * mean (one rounding of the output type) + 2^-60, over `rows` (all by default)."""
    o = out.double().cpu()
    if rows is not None:
        o, expect = o[rows], expect[rows]
    err = (o - expect).abs()
    tol = rel * expect.abs() + 2.0 ** -60
    bad = ~(err <= tol)  # (a NaN is out of bound)
    if bad.any():
        r, c = [int(x) for x in torch.nonzero(bad)[0]]
        return (f"{what}: {int(bad.sum())} elements out of bound; worst excess {torch.nan_to_num(err - tol, nan=float('inf')).max().item():.3e}; "
                f"first at row {r} head {c // D} channel {c % D}: got {o[r, c].item()} expected {expect[r, c].item():.6f}")
    return None


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def zero_score_qk(Lq, Lkb, H, n_valid=None):
    """Even query rows 0, odd rows 1 on channels 64-127; valid keys +-1/8 on channels 0-63: every valid score is exactly 0.  Keys
    from n_valid on are decoys: 8 on channels 64-127 (512 log2 units at c = 2^-3 for the odd rows)."""
    g = torch.Generator().manual_seed(Lq * 1000 + Lkb * 7 + H)
    q = torch.zeros(Lq, H, D)
    q[1::2, :, 64:] = 1.0
    k = torch.zeros(Lkb, H, D)
    k[:, :, :64] = (torch.randint(0, 2, (Lkb, H, 64), generator=g) * 2 - 1).float() * 0.125
    if n_valid is not None:
        k[n_valid:] = 0
        k[n_valid:, :, 64:] = 8.0
    return q.view(Lq, H * D), k.view(Lkb, H * D)


def base_census():
    def make():
        q, k = zero_score_qk(L0, L0, H0)
        v = census_code(L0, H0)
        return q, k, v, {w: window_mean(v, L0, L0, w) for w in WINDOWS}

    return cached("census", make)


# ---------------------------------------------------------------------------------------------------------------- A. census
@pytest.mark.parametrize("form", list(FORMS))
def test_census(form):
    q, k, v, expect = base_census()
    fails = [m for w in WINDOWS for m in [check_counts(run(form, q, k, v, H0, L0, w), expect[w], FORMS[form][2], f"window {w}")] if m]
    assert not fails, f"{form}: {len(fails)} of {len(WINDOWS)} windows\n" + "\n".join(fails)


def test_census_windows_put_every_kind_of_edge_inside_a_band():
    """(host arithmetic) over the windows of the base shape a band edge falls on a key-tile boundary, inside the ragged tile, and
    strictly inside a tile for queries in the middle of a wave; some wave skips a tile that its workgroup walks; some window leaves
    all tiles interior."""
    seen = set()
    for w in WINDOWS:
        lo, hi = band(L0, L0, w)
        seen.update(["lo on a tile boundary"] if ((lo % 64 == 0) & (lo > 0)).any() else [])
        seen.update(["hi on a tile boundary"] if ((hi % 64 == 63) & (hi < L0 - 1)).any() else [])
        seen.update(["edge inside the ragged tile"] if ((lo > 576) | ((hi >= 576) & (hi < L0 - 1))).any() else [])
        seen.update(["edge inside a tile, mid-wave"] if ((lo % 64 != 0) & (torch.arange(L0) % 32 == 13)).any() else [])
        for b0 in range(0, L0, 256):
            b1 = min(b0 + 256, L0)
            for w0 in range(b0, b1, 32):
                if int(hi[w0:w0 + 32].max()) // 64 < int(hi[b0:b1].max()) // 64 or int(lo[w0:w0 + 32].min()) // 64 > int(lo[b0:b1].min()) // 64:
                    seen.add("a wave skips a tile of its workgroup")
        if int(lo.max()) == 0 and int(hi.min()) == L0 - 1:
            seen.add("all interior")
    assert len(seen) == 6, seen


# ---------------------------------------------------------------------------------------------------------------- B. poison
@pytest.mark.parametrize("form", list(FORMS))
def test_poison(form):
    """See the file header: per launch 128 checked queries; score(i, j) = 128 log2 units exactly where j is outside i's band."""
    v_code = census_code(L0, H0)
    fails, n = [], 0
    for w in WINDOWS:
        mask = band_mask(L0, L0, w)
        expect = base_census()[3][w]
        for r0 in range(0, L0, D):
            rows = torch.arange(r0, min(r0 + D, L0))
            q = torch.zeros(L0, H0, D)
            q[rows, :, rows - r0] = 32.0
            k = torch.zeros(L0, H0, D)
            k[:, :, :len(rows)] = ((~mask[rows]).float().t() * 32.0).unsqueeze(1)  # 32 * 32 * 2^-3 = 2^7
            v = v_code.clone()
            v[~mask[rows].any(dim=0)] = SENTINEL
            msg = check_counts(run(form, q.view(L0, -1), k.view(L0, -1), v, H0, L0, w), expect, FORMS[form][2], f"window {w} queries {r0}-{int(rows[-1])}", rows)
            n += 1
            if msg:
                fails.append(msg)
    assert not fails, f"{form}: {len(fails)} of {n} launches\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- C. first visible tile
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("level", [-200, 150])
def test_first_visible_tile_fixes_the_reference(form, level):
    """Every score is `level` log2 units (q = 10 on 16 or 12 channels, k = -+10, c = 2^-3): the softmax over a window is uniform
    whatever the level, unless the row's reference was taken from a tile in which the row sees nothing."""
    n_ch = 16 if level == -200 else 12
    q = torch.zeros(L0, H0, D)
    k = torch.zeros(L0, H0, D)
    q[:, :, 40:40 + n_ch] = 10.0
    k[:, :, 40:40 + n_ch] = -10.0 if level < 0 else 10.0
    assert n_ch * 100 * (-1 if level < 0 else 1) * 0.125 == level
    v, expect = base_census()[2], base_census()[3]
    fails = []
    for w in WINDOWS:
        out = run(form, q.view(L0, -1), k.view(L0, -1), v, H0, L0, w)
        if not torch.isfinite(out.float()).all():
            fails.append(f"window {w}: {int((~torch.isfinite(out.float())).sum())} non-finite outputs")
            continue
        msg = check_counts(out, expect[w], FORMS[form][2], f"window {w}")
        if msg:
            fails.append(msg)
    assert not fails, f"{form} level {level}: {len(fails)} of {len(WINDOWS)} windows\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- D. random data
def random_qkv(Lq, Lk, H, seed):
    """Gaussian int8 codes (sigma 40) times 2^(-5 + {-1, 0, 1}) per (token, head) (sigma about 1.25), one dominant key (x 4); V
    Gaussian, rounded to bf16 and flushed below 2^-14, so that bf16 and fp16 hold all three."""
    g = torch.Generator().manual_seed(seed)

    def operand(L):
        codes = (torch.randn(L, H, D, generator=g) * 40).round().clamp(-127, 127)
        return codes * 2.0 ** (-5 + torch.randint(-1, 2, (L, H, 1), generator=g).float())

    q, k = operand(Lq), operand(Lk)
    if Lk > 70:
        k[69] *= 4.0
    v = torch.randn(Lk, H * D, generator=g).to(torch.bfloat16).float()
    v[v.abs() < 2.0 ** -14] = 0
    return q.view(Lq, H * D), k.view(Lk, H * D), v


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("window", [(100, 37), (0, 0)])
def test_random_data_under_the_derived_bound(form, window):
    q, k, v = cached("random", lambda: random_qkv(L0, L0, H0, 11))
    f16 = FORMS[form][0] == torch.float16
    fails = []
    for scale in POW2_SCALES:
        o64, pva, t, p = cached(("random64", window, scale), lambda: definition64(q, k, v, H0, L0, window, scale))
        tol = ((2.0 ** -10 + 2.0 ** -14) if f16 else (2.0 ** -8 + 2.0 ** -14)) * pva + (2.0 ** -11 if f16 else 2.0 ** -9) * o64.abs()
        if f16:  # the range term of tests/test_gpu_attention_fp16_probes.py (definition64_deep), over the visible keys
            m = t.max(dim=-1, keepdim=True).values
            deep = (torch.isfinite(t) & (t < m - (22.0 - 2.0 ** -6))).double()
            l = torch.exp2(t - m).sum(dim=-1)
            v64 = v.to(DEV).double().view(L0, H0, D)
            dv = torch.einsum("hqk,khd->qhd", deep, v64.abs())
            nd = deep.sum(dim=-1).transpose(0, 1).unsqueeze(-1)
            tol = tol + (2.0 ** -22 * (dv + nd * o64.view(L0, H0, D).abs()) / l.transpose(0, 1).unsqueeze(-1)).reshape(L0, -1)
        out = run(form, q, k, v, H0, L0, window, scale)
        err = torch.nan_to_num((out.double() - o64).abs(), nan=float("inf"))
        ok = tol > 0
        ratio = (err[ok] / tol[ok]).max().item() if ok.any() else 0.0
        print(f"PROBE window random {form} window {window} scale {scale:.4f}: largest err/bound {ratio:.3f}")
        n_bad = int((~(err <= tol)).sum())
        if n_bad:
            fails.append(f"scale {scale}: {n_bad} elements out of bound; worst excess {(err - tol).max().item():.3e}; err/bound {ratio:.3f}")
    assert not fails, f"{form} window {window}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- E. Lq != Lk
@pytest.mark.parametrize("form", list(FORMS))
def test_more_queries_than_valid_keys_with_k_len_and_decoys(form):
    """Lq = 300, key buffer 320, k_len = 200, window (10, 10): off = -100, so rows below 90 see nothing and are exact zeros; the
    keys from 200 on are decoys (512 log2 units for the odd rows, V = 2^10) and must not appear."""
    Lq, Lkb, n = 300, 320, 200
    q, k = zero_score_qk(Lq, Lkb, H0, n)
    v = census_code(Lkb, H0)
    v[n:] = 1024.0
    out = run(form, q, k, v, H0, n, (10, 10))
    lo, hi = band(Lq, n, (10, 10))
    assert int((hi < lo).sum()) == 90 and bool((hi[:90] < lo[:90]).all())
    assert bool((out[:90] == 0).all()), f"{int((out[:90] != 0).sum())} non-zero (or NaN) elements in the rows that see no key"
    msg = check_counts(out, window_mean(v, Lq, n, (10, 10)), FORMS[form][2], "rows 90-299", torch.arange(90, Lq))
    assert not msg, msg


@pytest.mark.parametrize("form", list(FORMS))
def test_more_keys_than_queries(form):
    Lq, Lk = 200, 300
    q, k = zero_score_qk(Lq, Lk, H0)
    v = census_code(Lk, H0)
    lo, hi = band(Lq, Lk, (10, 10))
    assert int(lo[0]) == 90 and int(hi[0]) == 110 and int(hi[-1]) == 299
    msg = check_counts(run(form, q, k, v, H0, Lk, (10, 10)), window_mean(v, Lq, Lk, (10, 10)), FORMS[form][2], "Lq 200 Lk 300")
    assert not msg, msg


# ---------------------------------------------------------------------------------------------------------------- F. equalities
@pytest.mark.parametrize("form", list(FORMS))
def test_unbounded_and_all_interior_windows_are_bit_equal_to_the_dense_call(form):
    """(-1, -1) launches what wanq_attention_fwd launches; (5000, 5000) runs the banded instantiation with every tile interior,
    which pins its summation order and its epilogue to the dense kernel's."""
    q, k, v = cached("random", lambda: random_qkv(L0, L0, H0, 11))
    dense = run(form, q, k, v, H0, L0, None, POW2_SCALES[0], entry="wanq_attention_fwd")
    assert torch.isfinite(dense.float()).all()
    for w in ((-1, -1), (5000, 5000)):
        out = run(form, q, k, v, H0, L0, w, POW2_SCALES[0])
        assert torch.equal(out, dense), f"window {w}: {int((out != dense).sum())} elements differ from wanq_attention_fwd"


# ---------------------------------------------------------------------------------------------------------------- G. stores
@pytest.mark.parametrize("form", list(FORMS))
def test_stores_stay_inside_their_rows_and_empty_band_blocks_are_written(form):
    """o is the column slice [128, 128 + H*128) of a sentinel-filled [Lq + 2, H*128 + 384] buffer, rows 1 ... Lq.  With 100 valid
    keys and window (10, 10), off = -500: rows below 490 see nothing -- whole query blocks (0-255 of 256, 0-383 of 128) have an
    empty band and must still write their rows, as zeros."""
    Lq, n = L0, 100
    q, k = zero_score_qk(Lq, L0, H0, n)
    v = census_code(L0, H0)
    v[n:] = 1024.0
    C = H0 * D
    big = torch.full((Lq + 2, C + 384), SENTINEL, dtype=FORMS[form][0], device=DEV)
    view = big[1:Lq + 1, 128:128 + C]
    run(form, q, k, v, H0, n, (10, 10), out=view)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:Lq + 1, 128:128 + C] = False
    assert bool((big[keep] == SENTINEL).all()), f"{int((big[keep] != SENTINEL).sum())} elements outside the output columns were written"
    out = view.clone()
    assert bool((out[:490] == 0).all()), f"{int((out[:490] != 0).sum())} elements of the rows that see no key are not zero"
    msg = check_counts(out, window_mean(v, Lq, n, (10, 10)), FORMS[form][2], "rows 490-599", torch.arange(490, Lq))
    assert not msg, msg


# ---------------------------------------------------------------------------------------------------------------- H. Python surface
def test_ops_attention_window_refuses_splits_and_leaves_the_dense_paths_alone():
    from viditq_extension import _C
    from wan import ops

    q, k, v = (t.to(DEV).to(torch.bfloat16) for t in cached("random", lambda: random_qkv(L0, L0, H0, 11)))
    with pytest.raises(RuntimeError, match="splits"):
        ops.attention(q, k, v, H0, window=(10, 10), splits=2)
    ref1 = torch.empty_like(q)
    _C.call("wanq_attention_fwd", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(ref1), _C.BF16, L0, L0, H0, D, q.stride(0), k.stride(0), v.stride(0),
            ref1.stride(0), 1.0 / math.sqrt(D), _C.stream())
    nbytes = _C.lib.wanq_attention_split_workspace(L0, H0, D, 2)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    ref2 = torch.empty_like(q)
    _C.call("wanq_attention_fwd_split", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(ref2), _C.BF16, L0, L0, H0, D, q.stride(0), k.stride(0),
            v.stride(0), ref2.stride(0), 1.0 / math.sqrt(D), 2, _C.ptr(ws), nbytes, _C.stream())
    assert torch.equal(ops.attention(q, k, v, H0, splits=1), ref1) and torch.equal(ops.attention(q, k, v, H0, splits=1, window=(-1, -1)), ref1)
    assert torch.equal(ops.attention(q, k, v, H0, splits=2), ref2) and torch.equal(ops.attention(q, k, v, H0, splits=2, window=(-1, -1)), ref2)
    assert not torch.equal(ref1, ref2)  # (the split path is another summation order: the two references are two paths)
    # a bounded window through the wrapper is the C entry's output, and the work figure counts the visible pairs
    o = ops.attention(q, k, v, H0, window=(100, 37))
    ref3 = torch.empty_like(q)
    _C.call("wanq_attention_window_fwd", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(ref3), _C.BF16, L0, L0, H0, D, q.stride(0), k.stride(0),
            v.stride(0), ref3.stride(0), 1.0 / math.sqrt(D), 100, 37, _C.stream())
    assert torch.equal(o, ref3) and not torch.equal(o, ref1)
    assert ops.window_pairs(L0, L0, (100, 37)) == int(band_mask(L0, L0, (100, 37)).sum()) < L0 * L0
    assert ops.window_pairs(300, 200, (10, 10)) == int(band_mask(300, 200, (10, 10)).sum()) and ops.window_pairs(L0, L0, (-1, -1)) == L0 * L0


# ---------------------------------------------------------------------------------------------------------------- I. model
WINDOW_I = (40, 40)
BLOCK_TOL = 1e-2  # relative Frobenius error a kernel-mode block is allowed against its oracle: tests/test_gpu_block.py:122


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def attention64(q, k, v, num_heads, k_len=None, out=None, splits=None, window=(-1, -1)):
    """wan.ops.attention by the float64 masked definition, rounded to the attention's type."""
    if q.dtype == torch.float32:
        q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
    Lk = k.shape[0] if k_len is None else min(int(k_len), k.shape[0])
    o = definition64(q, k, v, num_heads, Lk, window, 1.0 / math.sqrt(q.shape[1] // num_heads))[0].to(q.dtype)
    if out is not None:
        out.copy_(o)
        return out
    return o


def _sharpen(blocks):
    """Self-attention that matters: its gate at 1 and q scaled up, so that a row's weight sits on few keys -- losing the ones
    outside the window then moves the output by far more than the tolerance."""
    for blk in blocks:
        blk.modulation.data[:, 2] = 1.0
        blk.self_attn.norm_q.weight.data.fill_(3.0)


def test_fp_model_honours_window_size(monkeypatch):
    from wan import ops
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel

    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, freq_dim=64, window_size=WINDOW_I).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    _sharpen(fp.blocks)
    assert all(b.self_attn.window_size == WINDOW_I for b in fp.blocks)
    shape = (16, 2, 24, 24)  # grid (2, 12, 12): 288 tokens, two query blocks
    latent, ctx, t = torch.randn(shape, generator=g, device=DEV), torch.randn(16, 64, generator=g, device=DEV) * 0.1, torch.tensor([500], device=DEV)

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return fp([latent], t, [ctx], seq_len_for(shape))[0].float()

    calls = []
    real = ops.attention
    monkeypatch.setattr(ops, "attention", lambda *a, **kw: (calls.append(tuple(kw.get("window", (-1, -1)))), real(*a, **kw))[1])
    got = forward()
    assert calls.count(WINDOW_I) == 2 and calls.count((-1, -1)) == 2, calls  # self-attention with the window, cross-attention without
    monkeypatch.setattr(ops, "attention", attention64)
    ref = forward()
    for b in fp.blocks:
        b.self_attn.window_size = (-1, -1)
    monkeypatch.setattr(ops, "attention", real)
    dense = forward()
    err, moved = rel_err(got, ref), rel_err(dense, ref)
    print(f"FP model, window {WINDOW_I}: rel err vs float64 masked attention {err:.2e}; dense vs windowed {moved:.2e}")
    assert torch.isfinite(got).all() and err < BLOCK_TOL
    assert moved > 10 * BLOCK_TOL  # the window is live


def test_kernel_mode_block_honours_window_size(monkeypatch):
    from wan import ops
    from wan.modules.model import WanAttentionBlock, rope_params
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    dim, ffn, heads, grid, pad, lc = 256, 512, 2, (2, 12, 12), 4, 40
    torch.manual_seed(0)
    blk = WanAttentionBlock("t2v_cross_attn", dim, ffn, heads, window_size=WINDOW_I, cross_attn_norm=True)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.normal_(m.bias, std=0.05)
    _sharpen([blk])
    n_tok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_tok + pad, dim, generator=g)
    x[n_tok:] = 0
    e0 = torch.randn(1, 6, dim, generator=g) * 0.3
    ctx = torch.randn(lc, dim, generator=g)
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    hb = WanAttentionBlockWithHipKernel.from_float(blk.to(DEV))
    assert hb.window_size == WINDOW_I
    rope = ops.rope_table(freqs, grid, DEV)

    def forward():
        return hb(x.to(DEV).clone(), e0.to(DEV), rope, n_tok, _FpSrc(ctx.to(DEV), torch.bfloat16)).float()[:n_tok]

    real = ops.attention
    got = forward()
    monkeypatch.setattr(ops, "attention", attention64)
    ref = forward()
    monkeypatch.setattr(ops, "attention", real)
    hb.window_size = (-1, -1)
    dense = forward()
    err, moved = rel_err(got, ref), rel_err(dense, ref)
    print(f"kernel-mode block, window {WINDOW_I}: rel err vs float64 masked attention {err:.2e}; dense vs windowed {moved:.2e}")
    assert torch.isfinite(got).all() and err < BLOCK_TOL
    assert moved > 10 * BLOCK_TOL


def test_kernel_mode_refuses_a_window_with_quantised_attention():
    """window_size with attn.qk / attn.attn_map configured: NotImplementedError naming the keys and the layer, from the block
    builder and from the model built with quant_configs/w8a8_all_linears_qk8.yaml -- never a dense run that ignores the window."""
    from qdiff import config as qcfg
    from wan.modules.model import WanAttentionBlock, WanModel
    from wan.quant_wanx import QuantWanModel
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel

    blk = WanAttentionBlock("t2v_cross_attn", 256, 512, 2, window_size=WINDOW_I, cross_attn_norm=True).to(DEV)
    with pytest.raises(NotImplementedError, match=r"blocks\.3\.self_attn.*attn\.qk"):
        WanAttentionBlockWithHipKernel.from_float(blk, attn_qk8=True, name="blocks.3")
    with pytest.raises(NotImplementedError, match=r"attn\.attn_map \+ attn\.v"):
        WanAttentionBlockWithHipKernel.from_float(blk, attn_map=(8, False), attn_v_bits=8)
    assert WanAttentionBlockWithHipKernel.from_float(blk, attn_v_bits=8).window_size == WINDOW_I  # v's fake-quant alone is no obstacle
    assert WanAttentionBlockWithHipKernel.from_float(blk, cross_attn_qk8=True).window_size == WINDOW_I  # nor the cross-attention's recipe
    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, freq_dim=64, window_size=WINDOW_I).eval()
    model = QuantWanModel.from_float(fp, qcfg.load(os.path.join(ROOT, "wan2.1-quantization_amd", "quant_configs", "w8a8_all_linears_qk8.yaml")))
    model.quant_layer_refactor()
    model.set_init_done()
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn.*window_size=\(40, 40\).*attn\.qk"):
        model.hardware_forward_refactor()
