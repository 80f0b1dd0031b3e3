"""Flash attention (csrc/attention.hip) and the streamed attention-map quantiser (csrc/attn_map.hip) on inputs whose answer is
known exactly, and on random data under a derived elementwise bound -- the pin is the float64 definition computed here.

The existing attention tests use Gaussian inputs under max-abs < 3e-2 / rel-Frobenius < 1e-2: one key dropped or counted
twice out of a few hundred moves the output by ~1/Lk and passes.  Here:
  A  key census    q.k = 0 for every valid key, V = a binary code of the key index: o = count / n, integers that fp32 holds
                   exactly, asserted at one bf16 rounding.  A one-key error moves a count by 1.
  B  windows       eight query classes per wave, each with its own window of keys at score ~130 (log2 units) above the rest:
                   o = mean of V over the window; the lazy-rescale vote fires at a different tile for every class.  Plus a
                   staircase of per-tile scores j * step under the bound of C.
  C  random data   |o - o64| <= (2^-8 + 2^-14) (P64 |V|) + 2^-9 |o64| elementwise, with scale * log2(e) a power of two so that
                   the kernel's second rounding of Q is exact (derivation: profiles/PARITY_NOTES.md).
  D  stores stay inside their rows, Lq = 0, the stride refusals of the ABI.
Every family runs on every form, chosen explicitly: bf16 with 8 and with 4 waves, bf16 split-KV (2, 3, 5 shares), int8 Q.K^T
unsplit and split, and (A, B) the two attention-map forms.  One data generator and one expected value for all forms: q and k
are int8 codes times power-of-two per-(token, head) scales, which bf16 holds exactly, so the int8 and bf16 forms see the same
numbers and every score is exact."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
SENTINEL = -7776.0  # exact in bf16 and fp32
WANQ_OK, WANQ_E_SHAPE = 0, 2

ATTN_FORMS = {  # name -> (kind, splits, wanq_attention_select_form value)
    "bf16-8w": ("bf16", 1, 0),
    "bf16-4w": ("bf16", 1, 1 << 40),
    "bf16-split2": ("bf16", 2, None),
    "bf16-split3": ("bf16", 3, None),
    "bf16-split5": ("bf16", 5, None),
    "qk8": ("qk8", 1, None),
    "qk8-split3": ("qk8", 3, None),
}
MAP_FORMS = {"map": ("map", 1, None), "map-qk8": ("map-qk8", 1, None)}
ALL_FORMS = {**ATTN_FORMS, **MAP_FORMS}


class Case:
    """q / k as int8 codes [L, H*128] with fp32 power-of-two scales [L, H]; v bf16 [Lk_buffer, H*128]; k_len valid keys."""

    def __init__(self, qc, qs, kc, ks, v, H, k_len=None):
        self.qc, self.qs, self.kc, self.ks, self.v, self.H = qc.to(torch.int8), qs.float(), kc.to(torch.int8), ks.float(), v.to(torch.bfloat16), H
        self.Lq, self.Lkb = qc.shape[0], kc.shape[0]
        self.k_len = k_len
        self.n = self.Lkb if k_len is None else k_len
        assert v.shape[0] == self.Lkb and torch.isfinite(self.v.float()).all()

    def _deq(self, codes, scales):
        L = codes.shape[0]
        x = codes.float().view(L, self.H, D) * scales.view(L, self.H, 1)
        b = x.to(torch.bfloat16)
        assert torch.equal(b.float(), x), "codes * scale must be exact in bf16"
        return b.reshape(L, self.H * D)

    def bf16(self):
        return self._deq(self.qc, self.qs).to(DEV), self._deq(self.kc, self.ks).to(DEV), self.v.to(DEV)

    def q8(self):
        from wan import ops

        def rows(codes, scales, for_keys):
            L = codes.shape[0]
            planes = torch.stack([scales, -12582912.0 * scales], dim=-1).reshape(L, self.H * 2)
            return ops.Q8Rows.from_exchange(codes.to(DEV).contiguous(), planes.to(DEV), D, for_keys)

        return rows(self.qc, self.qs, False), rows(self.kc, self.ks, True), self.v.to(DEV)

    def f64(self):
        """q [Lq, H, 128], k, v [n, H, 128] of the valid keys, float64 on the GPU."""
        q = self.qc.to(DEV).double().view(self.Lq, self.H, D) * self.qs.to(DEV).double().unsqueeze(-1)
        k = self.kc.to(DEV).double().view(self.Lkb, self.H, D) * self.ks.to(DEV).double().unsqueeze(-1)
        return q, k[: self.n], self.v.to(DEV).double().view(self.Lkb, self.H, D)[: self.n]


def run_form(form, case, scale=None, out=None, ws=None):
    """One call of `form` on `case`.  scale None and no out: through wan.ops (scale = 1 / sqrt(128)); otherwise through the C ABI
    directly.  out: a [Lq, H*128] view whose row stride is passed on; ws: caller's split workspace (fp32), sized by the caller."""
    from viditq_extension import _C
    from wan import ops

    kind, splits, sel = ALL_FORMS[form]
    H, Lq, Lk = case.H, case.Lq, case.n
    prev = _C.lib.wanq_attention_select_form(sel) if sel is not None else None
    try:
        if kind in ("map", "map-qk8"):
            assert scale is None and out is None
            q, k, v = case.bf16() if kind == "map" else case.q8()
            return ops.attention_map_quant(q, k, v, H, 8, False, case.k_len)
        q, k, v = case.bf16() if kind == "bf16" else case.q8()
        if scale is None and out is None:
            return (ops.attention if kind == "bf16" else ops.attention_qk8)(q, k, v, H, case.k_len, splits=splits)
        scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
        if out is None:
            out = torch.empty(Lq, H * D, dtype=torch.bfloat16, device=DEV)
        nbytes = _C.lib.wanq_attention_split_workspace(Lq, H, D, splits)
        if ws is None and splits > 1:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        if kind == "qk8":
            _C.call("wanq_attention_qk8_fwd", _C.ptr(q.codes), _C.ptr(q.scales), q.stride, _C.ptr(k.codes), _C.ptr(k.scales), k.stride,
                    _C.ptr(v), _C.ptr(out), _C.BF16, Lq, Lk, H, D, q.codes.stride(0), k.codes.stride(0), v.stride(0), out.stride(0),
                    scale, splits, _C.ptr(ws), nbytes, _C.stream())
        elif splits > 1:
            _C.call("wanq_attention_fwd_split", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(out), _C.BF16, Lq, Lk, H, D, q.stride(0),
                    k.stride(0), v.stride(0), out.stride(0), scale, splits, _C.ptr(ws), nbytes, _C.stream())
        else:
            _C.call("wanq_attention_fwd", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(out), _C.BF16, Lq, Lk, H, D, q.stride(0), k.stride(0),
                    v.stride(0), out.stride(0), scale, _C.stream())
        return out
    finally:
        if prev is not None:
            _C.lib.wanq_attention_select_form(prev)


# ---------------------------------------------------------------------------------------------------------------- expected values
def census_code(n_keys, H, seed=5):
    """v[k, h, :] in {0, 1}: a code word of the key index whose column sums over any key set change when one key is dropped or
    counted twice (the one-hot of k mod 64: those columns count <= ceil(n / 64)) or replaced by the key 64, 128 or 192 away (bits 6
    and 7 of k and the one-hot of (k >> 6) & 3); rotated by 17 channels per head so that a head mix-up shows too."""
    k = torch.arange(n_keys)
    v = torch.zeros(n_keys, H, D)
    for b in range(8):
        v[:, :, b] = ((k >> b) & 1).float().unsqueeze(-1)
        v[:, :, 8 + b] = 1.0 - v[:, :, b]
        v[:, :, 84 + b] = ((k >> (8 + b)) & 1).float().unsqueeze(-1)
    v[k, :, 16 + (k % 64)] = 1.0
    v[k, :, 80 + ((k >> 6) & 3)] = 1.0
    v[:, :, 92:] = (torch.rand(n_keys, H, D - 92, generator=torch.Generator().manual_seed(seed)) < 0.25).float()
    for h in range(H):
        v[:, h] = torch.roll(v[:, h], 17 * h, dims=-1)
    return v


def check_counts(out, expect, what):
    """|o - count/n| <= 2^-8 count/n (one bf16 rounding of the result) + 2^-60; expect [Lq, H*128] float64."""
    err = (out.double().cpu() - expect).abs()
    tol = 2.0 ** -8 * expect.abs() + 2.0 ** -60
    bad = ~(err <= tol)  # (a NaN is out of bound)
    if bad.any():
        r, c = [int(x) for x in torch.nonzero(bad)[0]]
        return (f"{what}: {int(bad.sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}; first at query {r} head {c // D} "
                f"channel {c % D}: got {out[r, c].item()} expected {expect[r, c].item():.6f}")
    return None


def definition64(case, scale):
    """o64 = softmax(q k^T scale) v and P64 |v| by the float64 definition, [Lq, H*128] each."""
    q, k, v = case.f64()
    s = torch.einsum("qhd,khd->hqk", q, k) * float(np.float32(scale))
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("hqk,khd->qhd", p, v).reshape(case.Lq, -1)
    a = torch.einsum("hqk,khd->qhd", p, v.abs()).reshape(case.Lq, -1)
    return o, a


def bound_excess(out, o64, pv_abs):
    """Family C's bound.  Returns (number of elements out of bound, worst excess, largest err / bound)."""
    err = (out.double() - o64).abs()
    tol = (2.0 ** -8 + 2.0 ** -14) * pv_abs + 2.0 ** -9 * o64.abs()
    bad = ~(err <= tol)  # (a NaN is out of bound)
    err = torch.nan_to_num(err, nan=float("inf"))
    ok = tol > 0
    ratio = (err[ok] / tol[ok]).max().item() if ok.any() else 0.0
    return int(bad.sum()), (err - tol).max().item(), ratio


# ---------------------------------------------------------------------------------------------------------------- A. key census
CENSUS_LK = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
CENSUS_LQ = [1, 33, 130, 257, 300]


def census_case(Lq, Lk, H, tail):
    """Even query rows are 0.  Odd rows carry 8 on channels 64-127, where every valid key is 0 (valid keys hold +-1/8 on channels
    0-63 only): every valid score is exactly 0, weight 1/n.  The `tail` keys beyond k_len are decoys: k = 8 on channels 64-127
    (score ~520 log2 units for the odd rows: it would take all the mass) and v = 2^10."""
    g = torch.Generator().manual_seed(Lq * 1000 + Lk * 7 + H)
    qc = torch.zeros(Lq, H, D, dtype=torch.int8)
    qc[1::2, :, 64:] = 64
    kc = torch.zeros(Lk + tail, H, D, dtype=torch.int8)
    kc[:Lk, :, :64] = (torch.randint(0, 2, (Lk, H, 64), generator=g) * 2 - 1).to(torch.int8)
    kc[Lk:, :, 64:] = 64
    v = census_code(Lk + tail, H)
    v[Lk:] = 1024.0
    expect = (v[:Lk].double().sum(0) / Lk).reshape(1, H * D).expand(Lq, H * D)
    c = Case(qc.view(Lq, H * D), torch.full((Lq, H), 0.125), kc.view(Lk + tail, H * D), torch.full((Lk + tail, H), 0.125),
             v.view(Lk + tail, H * D), H, Lk if tail else None)
    return c, expect


@pytest.mark.parametrize("form", list(ALL_FORMS))
def test_key_census(form):
    """Every Lk around the tile and 16-key block edges up to 256, once as the whole buffer and once as k_len in front of 70
    decoy keys; Lq and H rotate so that partial waves and partial workgroups of both workgroup sizes meet every Lk.

    On the map forms this holds because csrc/attn_map.hip hands the normalised map to the P.V MFMAs as a bf16 pair hi + lo: with a
    single bf16 value bf16(1/n) was a rounding of its own in front of the output's (7/15 came out as 0.46875, 1.14 of this
    tolerance; 8 of the 32 cases failed on both map forms)."""
    fails, i = [], 0
    for Lk in CENSUS_LK:
        for tail in (0, 70):
            Lq, H = CENSUS_LQ[(i * 2 + (1 if tail else 0)) % 5], (1, 3)[(i + (1 if tail else 0)) % 2]
            case, expect = census_case(Lq, Lk, H, tail)
            msg = check_counts(run_form(form, case), expect, f"Lk={Lk} tail={tail} Lq={Lq} H={H}")
            if msg:
                fails.append(msg)
        i += 1
    assert not fails, f"{form}: {len(fails)} of {2 * len(CENSUS_LK)} cases\n" + "\n".join(fails)


def test_key_census_covers_every_query_count_and_head_count():
    seen, i = set(), 0
    for _ in CENSUS_LK:
        for tail in (0, 70):
            seen.add((CENSUS_LQ[(i * 2 + (1 if tail else 0)) % 5], (1, 3)[(i + (1 if tail else 0)) % 2]))
        i += 1
    assert {q for q, _ in seen} == set(CENSUS_LQ) and {h for _, h in seen} == {1, 3}


# ---------------------------------------------------------------------------------------------------------------- B. windows
WINDOW_CASES = [  # k_len, Lq, H, window size, layout
    (700, 257, 2, 3, 0), (700, 515, 3, 64, 1), (1100, 515, 2, 100, 0), (1100, 257, 3, 1, 1), (2050, 257, 2, 64, 1),
    (2050, 515, 3, 3, 0), (4129, 257, 3, 100, 1), (4129, 515, 2, 1, 0), (16001, 515, 2, 64, 1)]
CLASS_OF_WINDOW = [3, 0, 5, 1, 7, 2, 6, 4]  # the i-th window by position belongs to this query class


def window_starts(k_len, w, layout):
    """Eight disjoint windows of w keys: the first at key 0, the last ending at k_len - 1, six between that straddle (w = 1: touch)
    the boundaries in `targets`, five keys in front of the boundary.  Layout 0: the ring wraps of both ring depths (tiles 1|2, 2|3,
    3|4), a tile boundary in the middle, the share boundary of 2 splits and the last one of 3.  Layout 1: tile 0|1, the first share
    boundary of 3 splits and all four of 5 splits (with the first and the last window: a window in every share)."""
    nt = -(-k_len // 64)

    def shares(s):
        tps = -(-nt // s)
        return [z * tps * 64 for z in range(1, s) if z * tps * 64 < k_len]

    targets = [128, 192, 256, 64 * (nt // 2 + 1)] + shares(2) + shares(3)[-1:] if layout == 0 else [64] + shares(3)[:1] + shares(5)
    last = k_len - w
    wins, end = [0], w
    for i, b in enumerate(sorted(set(targets))):
        s = max(b - (i % 2 if w == 1 else min(5, w - 1)), end)
        if len(wins) < 7 and s + w * (7 - len(wins)) <= last:
            wins.append(s)
            end = s + w
    while len(wins) < 7:  # the rest inside tiles, spread over what is left
        left = 7 - len(wins)
        gap = min(37, (last - end - left * w) // left)
        assert gap >= 0, "windows do not fit"
        wins.append(end + gap)
        end = wins[-1] + w
    wins = sorted(wins) + [last]
    assert all(b - a >= w for a, b in zip(wins, wins[1:])) and len(wins) == 8
    return wins


def window_case(k_len, Lq, H, w, layout, tail=80):
    """Class g = channels [16 g, 16 g + 16).  A key of window g holds +-8 there (signs fixed per channel), a query of class g
    (row mod 8) likewise: score 16 * 8 * 8 * scale for the own window, exactly 0 for every other key.  Decoys beyond k_len: key
    k_len + i looks like class i mod 8 at twice the amplitude, with v = 2^10."""
    g = torch.Generator().manual_seed(k_len + 13 * w + layout)
    sign = (torch.randint(0, 2, (H, D), generator=g) * 2 - 1).to(torch.int8)
    wins = window_starts(k_len, w, layout)
    Lkb = k_len + tail
    kc = torch.zeros(Lkb, H, D, dtype=torch.int8)
    v = census_code(Lkb, H)
    v[k_len:] = 1024.0
    expect_cls = torch.zeros(8, H, D, dtype=torch.float64)
    for i, s in enumerate(wins):
        c = CLASS_OF_WINDOW[i]
        kc[s:s + w, :, 16 * c:16 * c + 16] = 8 * sign[:, 16 * c:16 * c + 16]
        expect_cls[c] = v[s:s + w].double().sum(0) / w
    for i in range(tail):
        c = i % 8
        kc[k_len + i, :, 16 * c:16 * c + 16] = 16 * sign[:, 16 * c:16 * c + 16]
    qc = torch.zeros(Lq, H, D, dtype=torch.int8)
    for c in range(8):
        qc[c::8, :, 16 * c:16 * c + 16] = 8 * sign[:, 16 * c:16 * c + 16]
    expect = expect_cls[torch.arange(Lq) % 8].reshape(Lq, H * D)
    case = Case(qc.view(Lq, H * D), torch.ones(Lq, H), kc.view(Lkb, H * D), torch.ones(Lkb, H), v.view(Lkb, H * D), H, k_len)
    return case, expect, wins


def test_window_layouts_reach_the_boundaries_they_name():
    """(host arithmetic only) the ring wraps and every share boundary of 2, 3 and 5 splits are straddled in some case, every share
    of every split count holds a window in some case, and own-window scores are >= 64 log2 units above the rest."""
    assert 16 * 8 * 8 / math.sqrt(128) * math.log2(math.e) >= 64
    ring, per_split = set(), {2: False, 3: False, 5: False}
    for k_len, _, _, w, layout in WINDOW_CASES:
        wins = window_starts(k_len, w, layout)
        nt = -(-k_len // 64)
        assert wins[0] == 0 and wins[-1] + w == k_len
        for b in (128, 192, 256):
            if any(s < b < s + w for s in wins):
                ring.add(b)
        for s_ in per_split:
            tps = -(-nt // s_)
            n_sh = -(-nt // tps)
            in_share = {min(k // (tps * 64), n_sh - 1) for s in wins for k in (s, s + w - 1)}
            bounds = [z * tps * 64 for z in range(1, n_sh)]
            if len(in_share) == n_sh and w > 1 and all(any(s < b < s + w for s in wins) for b in bounds):
                per_split[s_] = True
    assert ring == {128, 192, 256} and all(per_split.values()), (ring, per_split)


@pytest.mark.parametrize("form", list(ALL_FORMS))
def test_windows(form):
    """o[r] = mean of V over the window of class r mod 8 = count / w at one bf16 rounding.  Inside every wave the eight classes meet
    their maximum in eight different tiles: the vote that one class causes must rescale the others by exactly 1 (window still to
    come) or leave them on their reference (window passed), and the decoys beyond k_len must not appear."""
    fails = []
    for k_len, Lq, H, w, layout in WINDOW_CASES:
        case, expect, wins = window_case(k_len, Lq, H, w, layout)
        msg = check_counts(run_form(form, case), expect, f"k_len={k_len} Lq={Lq} H={H} w={w} windows at {wins} classes {CLASS_OF_WINDOW}")
        if msg:
            fails.append(msg)
    assert not fails, f"{form}: {len(fails)} of {len(WINDOW_CASES)} cases\n" + "\n".join(fails)


POW2_SCALES = [float(np.float32(2.0 ** -3 / math.log2(math.e))), float(np.float32(2.0 ** -4 / math.log2(math.e)))]


def test_scale_times_log2e_is_a_power_of_two_in_fp32():
    """The library forms c = scale * 1.4426950408889634f in fp32: for these two scales the product is exactly 2^-3 and 2^-4, so
    the second bf16 rounding of Q (q * c) is exact."""
    log2e = np.float32(1.4426950408889634)
    assert np.float32(POW2_SCALES[0]) * log2e == np.float32(0.125) and np.float32(POW2_SCALES[1]) * log2e == np.float32(0.0625)


STAIR = {3.0: (3, 2.0 ** -4), 5.5: (11, 2.0 ** -5), 6.5: (13, 2.0 ** -5), 20.0: (5, 2.0 ** -2)}  # step -> (code per tile, key scale)


def staircase_case(step, descending, Lk=1100, Lq=130, H=2):
    """Every key of tile j scores exactly j * step log2 units for the even query rows (q * c = 1 on channels 0-63) and half that
    for the odd rows (q * c = 1/2), at scale = 2^-3 / log2(e): the key holds T * key_scale on 16 channels per 127 of its code T."""
    mult, kscale = STAIR[step]
    nt = -(-Lk // 64)
    j = torch.arange(Lk) // 64
    T = (nt - 1 - j if descending else j) * mult
    kc = torch.zeros(Lk, H, D, dtype=torch.int8)
    for grp in range(4):
        kc[:, :, 16 * grp:16 * grp + 16] = (T - 127 * grp).clamp(0, 127).to(torch.int8).view(Lk, 1, 1)
    assert int(T.max()) <= 4 * 127
    qc = torch.zeros(Lq, H, D, dtype=torch.int8)
    qc[0::2, :, :64] = 8
    qc[1::2, :, :64] = 4
    v = torch.randn(Lk, H * D, generator=torch.Generator().manual_seed(int(step * 2) + descending))
    return Case(qc.view(Lq, H * D), torch.ones(Lq, H), kc.view(Lk, H * D), torch.full((Lk, H), kscale), v, H)


# the two map forms are left out: their output carries the map quantiser's own step (1/255 of a column's maximum per key), which
# the bound of family C does not contain
@pytest.mark.parametrize("form", list(ATTN_FORMS))
def test_staircase(form):
    """Per-tile scores j * step, ascending and descending, steps 3 and 5.5 (cross the 6-unit vote threshold only cumulatively), 6.5
    and 20, against the float64 softmax under the bound of family C."""
    fails, worst = [], 0.0
    for step in STAIR:
        for desc in (False, True):
            case = staircase_case(step, desc)
            q64, k64, _ = case.f64()
            s = torch.einsum("qhd,khd->hqk", q64[:2], k64) * 0.125  # the staircase is what it says: rows 0 and 1, tile 3 and the zero tile
            j3, zero = (case.Lkb // 64 - 3 if desc else 3), (-1 if desc else 0)
            assert s[0, 0, 64 * 3].item() == j3 * step and s[0, 1, 64 * 3].item() == j3 * step / 2 and s[0, 0, zero].item() == 0.0
            o64, pva = definition64(case, POW2_SCALES[0])
            n_bad, excess, ratio = bound_excess(run_form(form, case, scale=POW2_SCALES[0]), o64, pva)
            worst = max(worst, ratio)
            if n_bad:
                fails.append(f"step {step} {'descending' if desc else 'ascending'}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}")
    print(f"PROBE staircase {form}: largest err/bound {worst:.3f}")
    assert not fails, f"{form}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- C. random data
RANDOM_SHAPES = [  # Lq, Lk, H, k_len: the shapes of test_flash_attention_vs_fp32_softmax and of the split test (test_gpu_block.py)
    (32, 64, 1, None), (300, 300, 2, None), (256, 64, 3, None), (100, 512, 2, None), (1000, 777, 2, None), (515, 640, 12, 601),
    (2050, 2050, 4, None), (1, 17, 1, None), (5, 63, 2, None), (17, 65, 1, 33), (300, 2100, 2, None), (257, 2500, 1, 2437),
    (64, 4096, 3, None), (500, 130, 2, None)]


def random_case(Lq, Lk, H, k_len, sigma_exp):
    """Gaussian codes (sigma 40, clipped to +-127) times 2^(sigma_exp + {-1, 0, 1}) per (token, head): sigma about 0.3, 1.25 and
    2.5 for sigma_exp -7, -5, -4; one dominant key (x 4) where the sequence is long enough."""
    g = torch.Generator().manual_seed(Lq * 31 + Lk)

    def codes(L):
        return (torch.randn(L, H * D, generator=g) * 40).round().clamp(-127, 127).to(torch.int8)

    def scales(L):
        return 2.0 ** (sigma_exp + torch.randint(-1, 2, (L, H), generator=g).float())

    qc, qs, kc, ks = codes(Lq), scales(Lq), codes(Lk), scales(Lk)
    if Lk > 70:
        ks[69] *= 4.0
    v = torch.randn(Lk, H * D, generator=g)
    return Case(qc, qs, kc, ks, v, H, k_len)


# bf16 forms: the two scales whose c is a power of two (any other scale rounds q * c a second time, by 2^-9 of every score, which
# the bound does not contain).  int8 forms: scores are exact at any scale -- the model's 1 / sqrt(128) and 2^-3 / log2(e).
# The map forms are left out: see test_staircase.
RANDOM_FORMS = [(f, i) for f in ATTN_FORMS for i in (0, 1)]


@pytest.mark.parametrize("form,which", RANDOM_FORMS)
def test_random_data_under_the_derived_bound(form, which):
    """|o - o64| <= (2^-8 + 2^-14) (P64 |V|) + 2^-9 |o64| for every element (derivation in profiles/PARITY_NOTES.md)."""
    kind = ATTN_FORMS[form][0]
    scale = POW2_SCALES[which] if kind == "bf16" else (1.0 / math.sqrt(D), POW2_SCALES[0])[which]
    fails, worst = [], 0.0
    for i, (Lq, Lk, H, k_len) in enumerate(RANDOM_SHAPES):
        case = random_case(Lq, Lk, H, k_len, (-7, -5, -4)[i % 3])
        o64, pva = definition64(case, scale)
        n_bad, excess, ratio = bound_excess(run_form(form, case, scale=scale), o64, pva)
        worst = max(worst, ratio)
        if n_bad:
            fails.append(f"Lq={Lq} Lk={Lk} H={H} k_len={k_len}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}")
    print(f"PROBE random {form} scale {scale:.6f}: largest err/bound {worst:.3f}")
    assert not fails, f"{form} scale={scale}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- D. small items
@pytest.mark.parametrize("form", list(ATTN_FORMS))
def test_stores_stay_inside_their_rows(form):
    """o with a row stride wider than heads * 128 and more rows than Lq, the split workspace with room behind the size the library
    asks for, all prefilled with a sentinel: the sentinel survives and the rows hold what the plain call returns."""
    from viditq_extension import _C

    H, Lk = 2, 300
    splits = ATTN_FORMS[form][1]
    for Lq in (1, 130, 257):
        case = random_case(Lq, Lk, H, None, -5)
        plain = run_form(form, case)
        big = torch.full((Lq + 3, H * D + 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
        need = _C.lib.wanq_attention_split_workspace(Lq, H, D, splits) // 4
        ws = torch.full((need + 4096,), SENTINEL, dtype=torch.float32, device=DEV)
        run_form(form, case, out=big[:Lq, : H * D], ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(big[:Lq, : H * D], plain), Lq
        assert bool((big[Lq:] == SENTINEL).all()) and bool((big[:, H * D:] == SENTINEL).all()), Lq
        assert bool((ws[need:] == SENTINEL).all()), Lq


def _abi_args(entry, Lq=4, Lk=70, H=2, strides=None, splits=2):
    """Argument list of one attention entry point on small valid buffers; strides = (q, k, v, o) token strides in elements."""
    from viditq_extension import _C

    C = H * D
    qs, ks, vs, os_ = strides or (C, C, C, C)
    t = {n: torch.zeros(max(Lq, 1) if n in "qo" else Lk, C, dtype=torch.bfloat16, device=DEV) for n in "qkvo"}
    t["o"].fill_(SENTINEL)
    ws = torch.zeros(_C.lib.wanq_attention_split_workspace(max(Lq, 1), H, D, splits) // 4, dtype=torch.float32, device=DEV)
    keep = [t, ws]
    if entry == "wanq_attention_fwd":
        args = [_C.ptr(t["q"]), _C.ptr(t["k"]), _C.ptr(t["v"]), _C.ptr(t["o"]), _C.BF16, Lq, Lk, H, D, qs, ks, vs, os_, 1.0 / math.sqrt(D), _C.stream()]
    elif entry == "wanq_attention_fwd_split":
        args = [_C.ptr(t["q"]), _C.ptr(t["k"]), _C.ptr(t["v"]), _C.ptr(t["o"]), _C.BF16, Lq, Lk, H, D, qs, ks, vs, os_, 1.0 / math.sqrt(D), splits,
                _C.ptr(ws), ws.numel() * 4, _C.stream()]
    else:
        q8 = torch.zeros(max(Lq, 1), C, dtype=torch.int8, device=DEV)
        k8 = torch.zeros(Lk, C, dtype=torch.int8, device=DEV)
        qsc = torch.ones(2, H, max(Lq, 1), dtype=torch.float32, device=DEV)
        ksc = torch.ones(2, H, -(-Lk // 64) * 64, dtype=torch.float32, device=DEV)
        keep += [q8, k8, qsc, ksc]
        args = [_C.ptr(q8), _C.ptr(qsc), qsc.shape[2], _C.ptr(k8), _C.ptr(ksc), ksc.shape[2], _C.ptr(t["v"]), _C.ptr(t["o"]), _C.BF16, Lq, Lk, H, D,
                C, C, vs, os_, 1.0 / math.sqrt(D), splits, _C.ptr(ws), ws.numel() * 4, _C.stream()]
    return args, t["o"], keep


ENTRIES = ["wanq_attention_fwd", "wanq_attention_fwd_split", "wanq_attention_qk8_fwd"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_queries_is_ok_and_writes_nothing(entry):
    from viditq_extension import _C

    args, o, keep = _abi_args(entry, Lq=0)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())


@pytest.mark.parametrize("entry", ENTRIES)
def test_stride_rules_are_refused_through_the_abi(entry):
    """attention_impl's stride rules: each returns WANQ_E_SHAPE with its message, and nothing is launched (o keeps its sentinel)."""
    from viditq_extension import _C

    C = 2 * D
    rules = [((C, C, C, C - 8), "token stride smaller than heads*head_dim"), ((C, C, C - 8, C), "token stride smaller than heads*head_dim"),
             ((C, C, C, C + 4), "strides must be multiples of 8 elements"), ((C, C, C + 12, C), "strides must be multiples of 8 elements"),
             ((C, C, 1 << 24, C), "k / v token stride must be below 2^24 elements")]
    if entry != "wanq_attention_qk8_fwd":  # (the int8 entry point takes no bf16 q / k strides)
        rules += [((C - 8, C, C, C), "token stride smaller than heads*head_dim"), ((C, C - 8, C, C), "token stride smaller than heads*head_dim"),
                  ((C + 4, C, C, C), "strides must be multiples of 8 elements"), ((C, C + 12, C, C), "strides must be multiples of 8 elements"),
                  ((C, 1 << 24, C, C), "k / v token stride must be below 2^24 elements")]
    for strides, message in rules:
        args, o, keep = _abi_args(entry, strides=strides)
        assert getattr(_C.lib, entry)(*args) == WANQ_E_SHAPE, strides
        assert message in _C.lib.wanq_last_error().decode(), (strides, _C.lib.wanq_last_error().decode())
        torch.cuda.synchronize()
        assert bool((o == SENTINEL).all())
