"""The streamed attention-map quantiser (csrc/attn_map.hip: six attn_map_kernel<PASS, QK8> forms and attn_map_delta_kernel) on
inputs whose answer is known exactly, and at every bit width under a derived elementwise bound.  Both entry points are called
through the C ABI, so scale, n_bits, sym, the strides and the workspace are the test's to choose.  The pin is the float64
definition written here (definition64 / quantise64): base-2 softmax with the kernel's own fp32 constant c = scale * log2(e) (a
power of two for the scale used), per-key maximum over the valid queries, delta = max(cmax / levels, eps), rne(P / delta) * delta,
then @ v.  It is cross-checked once against oracle/wan_ref.py::attention_map_quant on the CPU.

The census and window probes of test_gpu_attention_probes.py cannot see the quantiser (a flat map: every code is `levels`; 255
levels: a step wrong by 4 moves P~ by 2^-8).  Here:
  A  exact probes   overlapping windows of power-of-two sizes s, 4 s and 8 s: P = 1 / |W| is dyadic, and the largest P of a key
                    column comes from exactly one query, one 16-query block, one 32-query wave or one 256-query workgroup; every
                    other query that sees the key holds cmax / 4 or cmax / 8 (never cmax / 2: `levels` is odd, a tie at every
                    width).  At n_bits = 2, sym (levels = 1) delta = cmax, P~ is cmax or 0, V is the census code: every partial sum
                    is dyadic and exact in fp32 in any order, so the output EQUALS the float64 definition rounded once to bf16.  A
                    lost maximum turns entries that quantise to 0 into cmax / 4: whole output channels move by integer counts.
  B  every width    the same cases and one Gaussian case per shape at n_bits 2, 3, 4, 6, 8, sym and asym, under
                        |o - o64| <= E + 2^-8 (|o64| + E) + 2^-100,
                        E = eps_rel (P~64 |V|) + sum over excused entries of delta_k |v_k|,
                        eps_P = (n + 16) 2^-24, eps_rel = eps_P + 2^-23 + 2^-16 + (2 n + 16) 2^-24      (n = valid keys),
                    an entry being excused (its code may differ by one) only where P64 / delta64 lies within
                    delta_tie = (2 eps_P + 3 2^-24) P64 / delta64 + 2^-30 of a half-integer; the excused share is <= 1 % per case, on
                    the float64 reference alone (section D).  Derivation: profiles/PARITY_NOTES.md.
  C  refusals       Lq = 0 and every argument rule of the two entry points; nothing is launched.
  D  CPU self-tests a numpy fp32 model of the three passes passes A and B; ten mutants of it fail; the generator refuses ties.

The window generator of test_gpu_attention_probes.py builds DISJOINT windows (each key has one holder and nobody else sees it), so
the windows here come from a generator of their own; Case, census_code and the Gaussian generator are that file's.

One mutant the issue lists under A cannot fail there: with levels = 1 every quotient is 1, 1/4 or 1/8, where truncation and rint
agree.  It is asserted under B (n_bits = 2 asym: 3/4 -> 1 by rint, 0 by truncation), like the dropped lo term (8 bits)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_attention_probes import DEV, POW2_SCALES, SENTINEL, Case, census_code, random_case

gpu = pytest.mark.gpu
D = 128
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
KINDS = ["map", "map-qk8"]
SCALE = POW2_SCALES[0]  # fp32(2^-3 / log2 e): the kernel's scale * 1.4426950408889634f is exactly 2^-3
C2 = 0.125
EPS = {True: float(np.float32(1e-6)), False: float(np.float32(1e-8))}  # the kernel's fp32 constants, sym / asym


def levels_of(n_bits, sym):
    return (1 << (n_bits - 1)) - 1 if sym else (1 << n_bits) - 1


def test_scale_gives_a_power_of_two():
    assert np.float32(SCALE) * np.float32(1.4426950408889634) == np.float32(C2)


# ================================================================================================ the probe generator
GROUPS, GCH, KAMP = 32, 4, 8  # 32 classes of 4 channels; a key of a class holds +-8 there
PAD_GROUP = 28                # groups 28..31: the four sub-window classes that only padded queries use
SOLE = [0, 15, 16, 31, 40, 77, 114, 151, 188, 193, 230, 271, 511, 512]  # lanes n16 0 / 15, nq 0 / 1, waves 1-7, workgroups 1 and 2
BLOCK, WAVE, GROUP = range(80, 96), range(128, 160), range(256, 512)    # wave 2's nq = 1 block, wave 4, the second workgroup
QSCALES = (1.0, 2.0, 4.0)


class Probe:
    """case: the Case (rows >= Lq of q are sequence padding, keys >= n are decoys); narrow: the query lists that own a window of s
    keys each; holder [H, n]: index into narrow of the class that holds the key's maximum, -1 where none does."""


def _pow2(x):
    return x >= 1 and (x & (x - 1)) == 0


def probe_case(Lq, n, H, tail=0, start=0, qamp=64, npad=0, narrow_size=None, broad_mult=(8, 4), check_levels=(1, 3, 7, 15, 63, 127, 255)):
    """Queries fall into classes; class c gives the score 4 * qamp (log2 units at c = 2^-3: 256 or 144) to the keys of its window
    W_c and 0 to every other key.  Narrow classes (one query of SOLE or the last query, or the rest of BLOCK, WAVE, GROUP) own s keys
    each, dealt round-robin over a run of keys that starts at `start` and wraps; the remaining queries are dealt over broad classes
    of 8 s or 4 s keys that tile the same run.  Head h shifts the run by 7 h and the deal by 3 h.  Keys outside the run are favoured
    by no query: their column maximum is 2^-144 / |W| (a denormal) or 0, and the eps floor applies.  Decoys beyond n hold 16 on every
    channel (twice any valid score) and v = 2^10.  Padded query (i, u) takes narrow class i and sub-window class u: the keys in both
    score twice, so it would hold 4 / s on them -- four times the column's maximum.
    Raises ValueError for a window size that is no power of two, for two classes on one key whose sizes are not 1 : 4 or 1 : 8, and
    for a quotient levels * ratio within 1/8 of a half-integer for any of check_levels."""
    g = torch.Generator().manual_seed(Lq * 1009 + n * 17 + H + start)
    sign = (torch.randint(0, 2, (H, D), generator=g) * 2 - 1).to(torch.int32)
    lists = [[q] for q in dict.fromkeys([Lq - 1] + SOLE) if q < Lq]
    taken = {q[0] for q in lists}
    lists += [x for x in ([q for q in r if q < Lq and q not in taken] for r in (BLOCK, WAVE, GROUP)) if x]
    free = 1 if n >= 5 else 0
    if n < 4:  # no room for a second window size: one class for everybody
        lists, m, s = [list(range(Lq))], 1, 1 << (n.bit_length() - 1)
    else:
        m = min(len(lists), n - free, PAD_GROUP - 5)
        s = 1 << (((n - free) // m).bit_length() - 1)
        while 4 * s > n:
            s //= 2
        lists = lists[:m]
    if narrow_size is not None:
        s = narrow_size
    cov = m * s
    if cov > n:
        raise ValueError(f"{m} windows of {s} keys do not fit into {n} keys")
    in_narrow = {q for x in lists for q in x}
    rest = [q for q in range(Lq) if q not in in_narrow]
    broad, j = [], 0  # intervals of the run
    if rest:
        big, small = broad_mult[0] * s, broad_mult[1] * s
        while cov - j >= big:
            broad.append((j, j + big))
            j += big
        if cov - j >= small:
            broad.append((j, j + small))
            j += small
        if j < cov or all(b - a != small for a, b in broad):  # the rest of the run, and always one window of the smaller size
            broad.append((cov - small, cov) if cov >= small else (0, small))
        if max(b for _, b in broad) > n or m + len(broad) > PAD_GROUP:
            raise ValueError("the broad windows do not fit")
    sizes = [s] * m + [b - a for a, b in broad]
    for w in sizes:
        if not _pow2(w):
            raise ValueError(f"window of {w} keys: 1 / {w} is not dyadic, the partial sums would round")
    Lkb, rows = n + tail, Lq + npad
    kc = torch.zeros(Lkb, H, D, dtype=torch.int32)
    qc = torch.zeros(rows, H, D, dtype=torch.int32)
    qs = torch.tensor(QSCALES)[(torch.arange(rows).view(-1, 1) + torch.arange(H).view(1, -1)) % 3]
    ks = torch.tensor([1.0, 0.5])[(torch.arange(Lkb).view(-1, 1) // 3 + torch.arange(H).view(1, -1)) % 2]
    member = torch.zeros(H, len(sizes), n, dtype=torch.bool)  # class x key
    holder = torch.full((H, n), -1, dtype=torch.int64)
    for h in range(H):
        pos = [(start + 7 * h + jj) % n for jj in range(max(cov, max([b for _, b in broad], default=0)))]
        for jj in range(cov):
            c = (jj + 3 * h) % m
            member[h, c, pos[jj]] = True
            holder[h, pos[jj]] = c
            u = PAD_GROUP + (jj // m) % 4
            kc[pos[jj], h, GCH * u:GCH * u + GCH] = KAMP * sign[h, GCH * u:GCH * u + GCH]
        for b, (j0, j1) in enumerate(broad):
            member[h, m + b, pos[j0:j1]] = True
        for c in range(len(sizes)):
            kc[:n][member[h, c], h, GCH * c:GCH * c + GCH] = KAMP * sign[h, GCH * c:GCH * c + GCH]
    kc = (kc.float() / ks.unsqueeze(-1)).to(torch.int32)  # the code that, times its scale, is +-8
    if tail:
        kc[n:] = 16 * sign.unsqueeze(0)
        ks[n:] = 1.0
    cls = torch.zeros(Lq, H, dtype=torch.int64)
    for c, x in enumerate(lists):
        cls[x] = c
    for i, q in enumerate(rest):
        for h in range(H):
            cls[q, h] = m + (i + h) % len(broad)
    for q in range(Lq):
        for h in range(H):
            c = int(cls[q, h])
            qc[q, h, GCH * c:GCH * c + GCH] = qamp * sign[h, GCH * c:GCH * c + GCH]
    for r in range(npad):
        for c in (r % m, PAD_GROUP + (r // m) % 4):
            qc[Lq + r, :, GCH * c:GCH * c + GCH] = qamp * sign[:, GCH * c:GCH * c + GCH]
    qc = (qc.float() / qs.unsqueeze(-1))
    if not torch.equal(qc, qc.round()):
        raise ValueError(f"qamp {qamp} is not a multiple of every query scale")
    # every key: the smallest window on it holds the maximum; every other window there is 4 or 8 times as large
    used = torch.zeros(H, len(sizes), dtype=torch.bool)
    for h in range(H):
        used[h, cls[:, h].unique()] = True
    sz = torch.tensor(sizes).view(1, -1, 1).expand(H, -1, n)
    seen = member & used.unsqueeze(-1)
    smin = torch.where(seen, sz, torch.full_like(sz, 1 << 30)).min(dim=1)[0]  # [H, n]
    for h in range(H):
        for c in range(len(sizes)):
            ratio = sizes[c] // smin[h][seen[h, c]]
            for r in ratio.unique().tolist():
                if r == 2:
                    raise ValueError(f"two windows of {sizes[c] // 2} and {sizes[c]} keys on one key: P / cmax = 1/2 is a tie at every odd number of levels")
                for L in check_levels:
                    t = L / r
                    if r > 1 and abs(t - math.floor(t) - 0.5) < 0.125:
                        raise ValueError(f"quotient {L}/{r} lies within 1/8 of a half-integer")
                if r not in (1, 4, 8):
                    raise ValueError(f"two windows of {sizes[c] // r} and {sizes[c]} keys on one key: P / cmax = 1/{r} is not 1/4 or 1/8")
    v = census_code(Lkb, H)
    if tail:
        v[n:] = 1024.0
    pr = Probe()
    pr.case = Case(qc.view(rows, H * D), qs, kc.view(Lkb, H * D), ks, v.view(Lkb, H * D), H, n if tail else None)
    pr.Lq, pr.n, pr.H, pr.s, pr.narrow, pr.holder, pr.broad, pr.tail, pr.npad = Lq, n, H, s, lists, holder, len(broad), tail, npad
    pr.favoured = seen.any(dim=1)  # [H, n]: some valid query's window holds the key
    pr.name = f"probe Lq={Lq} Lk={n} H={H} tail={tail} start={start} qamp={qamp} (s={s}, {m} narrow, {len(broad)} broad)"
    return pr


def loud_case(Lq, n, H, tail):
    """Query i puts all its mass on key i mod n (9 index bits x 14 channels of +-8: a full match scores 1008 log2 units, the next
    best 784): every column maximum is 1 when Lq >= n."""
    assert Lq >= n and n <= 512
    bits = ((torch.arange(512).view(-1, 1) >> torch.arange(9).view(1, -1)) & 1) * 2 - 1  # [512, 9]
    pat = torch.zeros(512, D)
    pat[:, :126] = bits.float().repeat_interleave(14, dim=1) * 8
    kc = torch.zeros(n + tail, H, D)
    kc[:n] = pat[:n].unsqueeze(1)
    qc = pat[torch.arange(Lq) % n].unsqueeze(1).expand(Lq, H, D)
    pr = Probe()
    pr.case = Case(qc.reshape(Lq, H * D), torch.ones(Lq, H), kc.view(n + tail, H * D), torch.ones(n + tail, H), census_code(n + tail, H).view(n + tail, H * D),
                   H, n if tail else None)
    pr.Lq, pr.n, pr.H, pr.tail, pr.npad, pr.name = Lq, n, H, tail, 0, f"loud Lq={Lq} Lk={n} H={H}"
    return pr


def gauss_case(Lq, n, H, tail, i):
    """The Gaussian case of a shape: test_gpu_attention_probes.random_case (one dominant key where Lk > 70), sigma rotating."""
    pr = Probe()
    pr.case = random_case(Lq, n + tail, H, n if tail else None, (-7, -5, -4)[i % 3])
    pr.Lq, pr.n, pr.H, pr.tail, pr.npad, pr.name = Lq, n, H, tail, 0, f"gauss Lq={Lq} Lk={n} H={H} tail={tail}"
    return pr


# Lq, Lk, H, tail, start, qamp: every Lq of {1, 31, 33, 255, 257, 300, 513}, every Lk of {1, 5, 63, 64, 65, 128, 129, 192, 193, 257}, both
# head counts; `start` moves the run of held keys (and with it the keys no query favours) and lets it wrap over the last key
SHAPES = [(1, 257, 1, 0, 0, 64), (31, 5, 3, 70, 2, 36), (33, 63, 1, 0, 40, 64), (255, 64, 3, 0, 0, 36), (257, 65, 1, 70, 33, 64),
          (300, 128, 3, 0, 100, 64), (513, 129, 1, 70, 0, 36), (300, 192, 1, 0, 0, 64), (257, 193, 3, 70, 150, 36), (513, 257, 3, 70, 0, 64),
          (255, 1, 1, 0, 0, 64), (513, 257, 1, 0, 192, 36), (300, 129, 3, 70, 101, 64), (33, 257, 3, 0, 230, 64)]
_cache = {}


def cases():
    """[(probe, its Gaussian twin)] of SHAPES, built once."""
    if "cases" not in _cache:
        _cache["cases"] = [(probe_case(*sh), gauss_case(*sh[:4], i)) for i, sh in enumerate(SHAPES)]
    return _cache["cases"]


# ================================================================================================ the float64 definition
def definition64(pr, c, dev):
    """P [H, Lq, n] = base-2 softmax of c * q k^T over the valid keys, for the valid queries; its column maxima [H, n]; v [n, H, 128]."""
    case, Lq, n, H = pr.case, pr.Lq, pr.n, pr.H
    q = case.qc.to(dev).double().view(-1, H, D)[:Lq] * case.qs.to(dev).double()[:Lq].unsqueeze(-1)
    k = case.kc.to(dev).double().view(-1, H, D)[:n] * case.ks.to(dev).double()[:n].unsqueeze(-1)
    s = torch.einsum("qhd,khd->hqk", q, k) * c
    e = torch.exp2(s - s.max(dim=-1, keepdim=True)[0])
    P = e / e.sum(dim=-1, keepdim=True)
    return {"P": P, "cmax": P.max(dim=1)[0], "v": case.v.to(dev).double().view(-1, H, D)[:n], "Lq": Lq, "n": n}


def quantise64(dfn, n_bits, sym):
    """delta [H, n], the quotients t = P / delta and the quantised map rne(t) * delta (torch.round rounds halves to even)."""
    delta = torch.clamp(dfn["cmax"] / levels_of(n_bits, sym), min=EPS[bool(sym)])
    t = dfn["P"] / delta.unsqueeze(1)
    return delta, t, torch.round(t) * delta.unsqueeze(1)


def expectation(dfn, n_bits, sym):
    """o64 [Lq, H*128], the bound of family B and the share of excused entries."""
    n = dfn["n"]
    delta, t, pq = quantise64(dfn, n_bits, sym)
    eps_p = (n + 16) * 2.0 ** -24
    tie = ((t - torch.floor(t) - 0.5).abs() <= (2 * eps_p + 3 * 2.0 ** -24) * t + 2.0 ** -30).double()
    eps_rel = eps_p + 2.0 ** -23 + 2.0 ** -16 + (2 * n + 16) * 2.0 ** -24
    va = dfn["v"].abs()
    o64 = torch.einsum("hqk,khd->qhd", pq, dfn["v"]).reshape(dfn["Lq"], -1)
    E = (eps_rel * torch.einsum("hqk,khd->qhd", pq, va) + torch.einsum("hqk,khd->qhd", tie * delta.unsqueeze(1), va)).reshape(dfn["Lq"], -1)
    return o64, E + 2.0 ** -8 * (o64.abs() + E) + 2.0 ** -100, float(tie.mean())


def check_exact(out, dfn, what):
    """Family A: out equals the float64 definition at n_bits = 2, sym, rounded once to bf16.  Returns a message or None."""
    _, _, pq = quantise64(dfn, 2, True)
    o64 = torch.einsum("hqk,khd->qhd", pq, dfn["v"]).reshape(dfn["Lq"], -1)
    assert torch.equal(o64.float().double(), o64), "the expected value must be exact in fp32"
    expect = o64.float().to(torch.bfloat16)
    got = out.to(expect.device)
    bad = ~(got == expect)  # (a NaN is unequal)
    if bad.any():
        r, ch = [int(x) for x in torch.nonzero(bad)[0]]
        return (f"{what}: {int(bad.sum())} elements differ ({int(bad.any(dim=1).sum())} query rows); first at query {r} head {ch // D} channel {ch % D}: "
                f"got {got[r, ch].item()} expected {expect[r, ch].item()}")
    return None


def check_bound(out, dfn, n_bits, sym, what):
    """Family B.  Returns (message or None, largest err / bound, excused share)."""
    o64, bound, share = expectation(dfn, n_bits, sym)
    err = torch.nan_to_num((out.to(o64.device).double() - o64).abs(), nan=float("inf"))
    bad = ~(err <= bound)
    ratio = float((err / bound).max())
    msg = None
    if bad.any():
        r, ch = [int(x) for x in torch.nonzero(bad)[0]]
        msg = (f"{what}: {int(bad.sum())} elements out of bound, err/bound {ratio:.3f}; first at query {r} head {ch // D} channel {ch % D}: "
               f"got {out[r, ch].item()} expected {o64[r, ch].item():.6g} bound {bound[r, ch].item():.3g}")
    return msg, ratio, share


# ================================================================================================ the two entry points
TIGHT = dict(q=0, k=0, v=0, o=0, q8=0, k8=0, qs=0, ks=0)
WIDE = dict(q=8, k=24, v=16, o=12, q8=16, k8=48, qs=3, ks=8)  # every stride larger than the tight one, within its multiple rule
JUNK = 1024.0  # in every element between a row's end and the next row, and in the scale planes behind the valid tokens


def run_abi(kind, pr, n_bits, sym, layout=TIGHT, ws=None, scale=SCALE):
    """One call on the valid queries and keys of pr.  The output is a view with `o` sentinel columns and a sentinel row behind it, the
    workspace is exactly wanq_attention_map_workspace bytes with 64 sentinel floats behind it (ws: reuse the caller's); both are
    checked.  The key-scale planes hold JUNK for the masked keys of a ragged last tile: with the clamped key row those carry the
    largest raw scores in the buffer.  Returns (out [Lq, H*128], ws)."""
    from viditq_extension import _C

    case, Lq, n, H = pr.case, pr.Lq, pr.n, pr.H
    C = H * D
    need = _C.lib.wanq_attention_map_workspace(Lq, n, H)
    assert need == (2 * Lq + 3 * n) * H * 4
    if ws is None:
        ws = torch.full((need // 4 + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    big = torch.full((Lq + 1, C + layout["o"]), SENTINEL, dtype=torch.bfloat16, device=DEV)

    def rows(x, pad, dtype):
        b = torch.full((x.shape[0], C + pad), 77, dtype=dtype, device=DEV)
        b[:, :C] = x.to(DEV)
        return b

    v = rows(case.v, layout["v"], torch.bfloat16)
    if kind == "map":
        qb, kb, _ = case.bf16()
        q, k = rows(qb, layout["q"], torch.bfloat16), rows(kb, layout["k"], torch.bfloat16)
        _C.call("wanq_attention_map_quant_fwd", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(big), _C.BF16, Lq, n, H, D, q.stride(0), k.stride(0), v.stride(0),
                big.stride(0), float(scale), n_bits, int(sym), _C.ptr(ws), need, _C.stream())
    else:
        q8, k8 = rows(case.qc, layout["q8"], torch.int8), rows(case.kc, layout["k8"], torch.int8)
        qsc = torch.full((H, Lq + layout["qs"]), JUNK, dtype=torch.float32, device=DEV)
        qsc[:, :Lq] = case.qs[:Lq].t().to(DEV)
        ksc = torch.full((H, -(-n // 64) * 64 + layout["ks"]), JUNK, dtype=torch.float32, device=DEV)
        ksc[:, :n] = case.ks[:n].t().to(DEV)
        _C.call("wanq_attention_map_quant_qk8_fwd", _C.ptr(q8), _C.ptr(qsc), qsc.stride(0), _C.ptr(k8), _C.ptr(ksc), ksc.stride(0), _C.ptr(v), _C.ptr(big),
                _C.BF16, Lq, n, H, D, q8.stride(0), k8.stride(0), v.stride(0), big.stride(0), float(scale), n_bits, int(sym), _C.ptr(ws), need, _C.stream())
    torch.cuda.synchronize()
    assert bool((big[Lq:] == SENTINEL).all()) and bool((big[:, C:] == SENTINEL).all()), f"{pr.name}: a store left the output's rows"
    assert bool((ws[need // 4:] == SENTINEL).all()), f"{pr.name}: a store left the workspace"
    return big[:Lq, :C], ws


def dfn_of(pr):
    """The float64 definition of a case on the GPU, computed once."""
    if pr.name not in _cache:
        _cache[pr.name] = definition64(pr, C2, DEV)
    return _cache[pr.name]


# ================================================================================================ A. exact probes
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_exact_probe(kind):
    """n_bits = 2, sym: the output equals the float64 definition rounded once to bf16, for every shape of SHAPES, tight and wide
    strides alternating (which shape gets which swaps between the two forms).  Reached: a key's maximum held by one query alone on
    lanes n16 0 and 15, in query blocks nq 0 and 1, in each of the 8 waves, in the second and third workgroup and by the last query
    of a ragged block; by one block, one wave, one workgroup; every slot of a tile, tiles 0 - 4; masked keys with the largest raw
    scores; keys under the eps floor (test_probe_cases_reach_what_they_name counts all of these on the CPU)."""
    fails = []
    for i, (pr, _) in enumerate(cases()):
        layout = WIDE if (i + KINDS.index(kind)) % 2 else TIGHT
        out, _ = run_abi(kind, pr, 2, True, layout)
        msg = check_exact(out, dfn_of(pr), pr.name + (" wide" if layout is WIDE else " tight"))
        if msg:
            fails.append(msg)
    assert not fails, f"{kind}: {len(fails)} of {len(SHAPES)} cases\n" + "\n".join(fails)


REUSE_SHAPES = [(300, 129, 3, 70, 101, 64), (513, 257, 1, 0, 192, 36)]


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_workspace_reuse_leaves_no_stale_maximum(kind):
    """A run whose column maxima are all 1 (at least 4 / s: four times the probe's), then the probe in the same workspace: bit-equal
    to the probe in a fresh workspace, and to the definition."""
    for sh in REUSE_SHAPES:
        pr = cases()[SHAPES.index(sh)][0]
        assert pr.s >= 4
        fresh, _ = run_abi(kind, pr, 2, True)
        _, ws = run_abi(kind, loud_case(*sh[:4]), 2, True)
        cmax = ws[2 * pr.Lq * pr.H:(2 * pr.Lq + pr.n) * pr.H]
        assert bool((cmax == 1.0).all()), "the loud run's column maxima"
        again, _ = run_abi(kind, pr, 2, True, ws=ws)
        assert torch.equal(again, fresh), pr.name
        assert check_exact(again, dfn_of(pr), pr.name) is None


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_padded_queries_and_keys_change_no_code(kind):
    """wan.ops.attention_map_quant with q_len and k_len: 4 m padded query rows that would hold four times the maximum of every held
    column, 70 decoy keys.  The rows in front equal the definition, the padded rows are zero.  (ops passes scale = 1 / sqrt(128):
    c is no power of two, but every key of a window still gets the same score, so P = 1 / |W| stays; the int8 form's fused
    multiply-add leaves P an ulp of fp32 off, which the bf16 rounding of the output removes since the expected counts / s are bf16
    numbers.)"""
    from wan import ops

    Lq, n, H = 300, 129, 3
    base = probe_case(Lq, n, H, 70, 101, 64)
    pr = probe_case(Lq, n, H, 70, 101, 64, npad=4 * len(base.narrow))
    assert pr.s >= 4 and pr.case.Lq == Lq + 4 * len(base.narrow)
    q, k, v = pr.case.bf16() if kind == "map" else pr.case.q8()
    out = ops.attention_map_quant(q, k, v, H, 2, True, k_len=n, q_len=Lq)
    torch.cuda.synchronize()
    assert out.shape[0] == pr.case.Lq and bool((out[Lq:] == 0).all())
    dfn = definition64(pr, 1.0 / math.sqrt(D) * math.log2(math.e), DEV)
    msg = check_exact(out[:Lq], dfn, pr.name)
    assert msg is None, msg
    # and the padded rows, had they counted, would have changed codes: with the column maxima over all rows the answer differs
    pr.Lq = pr.case.Lq
    full = definition64(pr, 1.0 / math.sqrt(D) * math.log2(math.e), DEV)
    assert check_exact(out[:Lq], {**full, "P": full["P"][:, :Lq], "Lq": Lq}, "all rows") is not None


# ================================================================================================ B. every bit width
BITS = [2, 3, 4, 6, 8]


@gpu
@pytest.mark.parametrize("sym", [1, 0])
@pytest.mark.parametrize("n_bits", BITS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_bit_width_under_the_derived_bound(kind, n_bits, sym):
    """|o - o64| <= E + 2^-8 (|o64| + E) + 2^-100 with E = eps_rel (P~64 |V|) + sum_excused delta_k |v_k| (module docstring;
    derivation in profiles/PARITY_NOTES.md), on every probe case and the Gaussian case of its shape."""
    fails, worst, worst_share = [], 0.0, 0.0
    for i, pair in enumerate(cases()):
        for pr in pair:
            out, _ = run_abi(kind, pr, n_bits, sym, WIDE if (i + n_bits) % 2 else TIGHT)
            msg, ratio, share = check_bound(out, dfn_of(pr), n_bits, sym, pr.name)
            worst, worst_share = max(worst, ratio), max(worst_share, share)
            if msg:
                fails.append(msg)
    print(f"PROBE attn-map {kind} n_bits={n_bits} sym={sym}: largest err/bound {worst:.3f}, largest excused share {worst_share:.5f}")
    assert not fails, f"{kind} n_bits={n_bits} sym={sym}: {len(fails)} of {2 * len(SHAPES)} cases\n" + "\n".join(fails)


# ================================================================================================ C. refusals and empty calls
def _abi_args(kind, Lq=4, Lk=70, H=2, n_bits=8, sym=0, dtype=None, head_dim=D, strides=None, ws_short=0, ws_shift=0, code_strides=None, ks_stride=None,
              ks_shift=0):
    """Argument list of one entry point on small valid buffers (strides = v, o token strides); returns (args, buffers to watch)."""
    from viditq_extension import _C

    C = H * D
    vs, os_ = strides or (C, C)
    rows_q, rows_k = max(Lq, 1), max(Lk, 1)
    t = {n: torch.zeros(rows_q if n in "qo" else rows_k, C + 64, dtype=torch.bfloat16, device=DEV) for n in "qkvo"}
    t["o"].fill_(SENTINEL)
    need = _C.lib.wanq_attention_map_workspace(rows_q, rows_k, H)
    ws = torch.full((need // 4 + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    wsp = _C.ptr(ws) + ws_shift
    tail = [float(SCALE), n_bits, sym, wsp, need - ws_short, _C.stream()]
    dt = _C.BF16 if dtype is None else dtype
    if kind == "map":
        args = [_C.ptr(t["q"]), _C.ptr(t["k"]), _C.ptr(t["v"]), _C.ptr(t["o"]), dt, Lq, Lk, H, head_dim, C, C, vs, os_] + tail
        keep = [t]
    else:
        q8 = torch.zeros(rows_q, C + 64, dtype=torch.int8, device=DEV)
        k8 = torch.zeros(rows_k, C + 64, dtype=torch.int8, device=DEV)
        qsc = torch.ones(H, rows_q, dtype=torch.float32, device=DEV)
        ksc = torch.ones(H * (-(-rows_k // 64) * 64 + 8) + 4, dtype=torch.float32, device=DEV)
        q8s, k8s = code_strides or (C, C)
        kss = -(-rows_k // 64) * 64 if ks_stride is None else ks_stride
        args = [_C.ptr(q8), _C.ptr(qsc), rows_q, _C.ptr(k8), _C.ptr(ksc) + ks_shift, kss, _C.ptr(t["v"]), _C.ptr(t["o"]), dt, Lq, Lk, H, head_dim, q8s, k8s,
                vs, os_] + tail
        keep = [t, q8, k8, qsc, ksc]
    return args, (t["o"], ws), keep


ENTRY = {"map": "wanq_attention_map_quant_fwd", "map-qk8": "wanq_attention_map_quant_qk8_fwd"}


def _untouched(watch):
    torch.cuda.synchronize()
    return all(bool((b == SENTINEL).all()) for b in watch)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_no_queries_is_ok_and_writes_nothing(kind):
    from viditq_extension import _C

    args, watch, keep = _abi_args(kind, Lq=0)
    assert getattr(_C.lib, ENTRY[kind])(*args) == WANQ_OK
    assert _untouched(watch)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_argument_rules_are_refused_through_the_abi(kind):
    """Each rule returns its code with its message; the output and the workspace keep their sentinel.  Only argument checks run:
    every buffer is as large as the valid call's."""
    from viditq_extension import _C

    C = 2 * D
    rules = [(dict(n_bits=1), WANQ_E_ARG, "must be 2..8"), (dict(n_bits=9), WANQ_E_ARG, "must be 2..8"),
             (dict(dtype=_C.F16), WANQ_E_ARG, "only bf16 is implemented"), (dict(head_dim=64), WANQ_E_SHAPE, "only 128 is implemented"),
             (dict(Lk=0), WANQ_E_SHAPE, "bad lengths"), (dict(ws_short=1), WANQ_E_ARG, "bytes needed"),
             (dict(ws_shift=4), WANQ_E_ARG, "workspace must be 16-byte aligned"),
             (dict(strides=(C - 8, C)), WANQ_E_SHAPE, "token stride smaller than heads*head_dim"),
             (dict(strides=(C, C - 4)), WANQ_E_SHAPE, "token stride smaller than heads*head_dim"),
             (dict(strides=(C + 12, C)), WANQ_E_SHAPE, "v stride must be a multiple of 8, o of 4"),
             (dict(strides=(C, C + 2)), WANQ_E_SHAPE, "v stride must be a multiple of 8, o of 4")]
    if kind == "map-qk8":
        planes = "the key scale planes must be 16-byte aligned"
        rules += [(dict(code_strides=(C + 8, C)), WANQ_E_SHAPE, "multiples of 16 bytes"), (dict(code_strides=(C, C + 8)), WANQ_E_SHAPE, "multiples of 16 bytes"),
                  (dict(ks_stride=64), WANQ_E_SHAPE, planes), (dict(ks_stride=128 + 2), WANQ_E_SHAPE, planes), (dict(ks_shift=4), WANQ_E_SHAPE, planes)]
    for kw, code, message in rules:
        args, watch, keep = _abi_args(kind, **kw)
        assert getattr(_C.lib, ENTRY[kind])(*args) == code, kw
        assert message in _C.lib.wanq_last_error().decode(), (kw, _C.lib.wanq_last_error().decode())
        assert _untouched(watch), kw
    args, watch, keep = _abi_args(kind)  # and the unmodified call is a valid one
    assert getattr(_C.lib, ENTRY[kind])(*args) == WANQ_OK
    torch.cuda.synchronize()


# ================================================================================================ D. CPU self-tests
def _bf16r(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, numpy."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


MUTANTS = ["no_wave7", "no_nq1", "no_second_workgroup", "other_head", "flush_as_previous_tile", "masked_key", "stale_cmax", "other_levels"]


def model(pr, n_bits, sym, mutant=None, c=C2):
    """The three passes in numpy fp32, without the MFMA order: row statistics, column maxima per 16-query block reduced over the
    blocks (where the mutants drop a wave, a query block or a workgroup), the delta kernel, P~ as a bf16 pair, fp32 P.V, one bf16
    rounding.  Returns bf16 [Lq, H*128]."""
    f32 = np.float32
    case, Lq, n, H = pr.case, pr.Lq, pr.n, pr.H
    q = (case.qc.float().view(-1, H, D) * case.qs.unsqueeze(-1)).numpy()[:Lq]
    k = (case.kc.float().view(-1, H, D) * case.ks.unsqueeze(-1)).numpy()
    v = case.v.float().view(-1, H, D).numpy()
    nk = n + 1 if mutant == "masked_key" and case.Lkb > n else n  # the first masked key passes the mask
    s = np.matmul(q.transpose(1, 0, 2), k[:nk].transpose(1, 2, 0)) * f32(c)
    e = np.exp2(s - s.max(-1, keepdims=True)).astype(f32)
    P = (e * (f32(1) / e.sum(-1, keepdims=True, dtype=f32)))[:, :, :n]
    nb = -(-Lq // 16)
    Pp = np.zeros((H, nb * 16, n), f32)
    Pp[:, :Lq] = P
    pm = Pp.reshape(H, nb, 16, n).max(2)
    b = np.arange(nb)
    keep = np.ones(nb, bool)
    if mutant == "no_wave7":
        keep &= (b // 2) % 8 != 7
    if mutant == "no_nq1":
        keep &= b % 2 == 0
    if mutant == "no_second_workgroup":
        keep &= b // 16 != 1
    cmax = pm[:, keep].max(1) if keep.any() else np.zeros((H, n), f32)
    if mutant == "flush_as_previous_tile":
        cmax = np.concatenate([cmax[:, 64:], np.zeros((H, min(64, n)), f32)], axis=1)[:, :n]
    if mutant == "stale_cmax":
        cmax = np.maximum(cmax, f32(1))  # what loud_case leaves behind
    if mutant == "other_head":
        cmax = cmax[[h ^ 1 if h ^ 1 < H else h for h in range(H)]]
    L = f32(levels_of(n_bits, (not sym) if mutant == "other_levels" else sym))
    delta = np.maximum(cmax / L, f32(EPS[bool(sym)]))
    dinv = f32(1) / delta
    t = P * dinv[:, None, :]
    pq = (np.trunc(t) if mutant == "trunc" else np.rint(t)).astype(f32) * delta[:, None, :]
    hi = _bf16r(pq)
    lo = np.zeros_like(hi) if mutant == "no_lo" else _bf16r(pq - hi)
    vt = v[:n].transpose(1, 0, 2)
    o = (np.matmul(hi, vt) + np.matmul(lo, vt)).transpose(1, 0, 2)
    return torch.from_numpy(_bf16r(np.ascontiguousarray(o).reshape(Lq, H * D))).to(torch.bfloat16)


def applies(mutant, pr):
    """Whether the shape holds what the mutant breaks: a held key all of whose holders the mutant drops (and somebody else who sees
    the key), a second head, a second tile, a masked key."""
    def held_only_by(pred):
        return pr.broad > 0 and any(all(pred(q) for q in x) for x in pr.narrow)

    if mutant == "no_wave7":
        return held_only_by(lambda q: (q // 32) % 8 == 7)
    if mutant == "no_nq1":
        return held_only_by(lambda q: (q // 16) % 2 == 1)
    if mutant == "no_second_workgroup":
        return held_only_by(lambda q: q // 256 == 1)
    if mutant == "other_head":
        return pr.H > 1 and pr.broad > 0
    if mutant == "flush_as_previous_tile":
        return pr.n > 64 and pr.broad > 0  # (a lone window under a zero maximum meets the eps floor: 1e6 codes of 1e-6, the same bf16)
    if mutant == "masked_key":
        return pr.tail > 0
    if mutant == "stale_cmax":
        return pr.s >= 2
    return pr.broad > 0  # other_levels, trunc: somebody holds cmax / 4


def dfn_cpu(pr):
    if ("cpu", pr.name) not in _cache:
        _cache["cpu", pr.name] = definition64(pr, C2, "cpu")
    return _cache["cpu", pr.name]


def test_definition_matches_the_oracle_on_a_random_case():
    """definition64 / quantise64 against oracle/wan_ref.py::attention_map_quant in float64, at the oracle's scale 1 / sqrt(128)."""
    from oracle import wan_ref as wr

    pr = gauss_case(70, 100, 2, 30, 1)
    dfn = definition64(pr, math.log2(math.e) / math.sqrt(D), "cpu")
    H = pr.H
    q = pr.case.qc.double().view(-1, H, D) * pr.case.qs.double().unsqueeze(-1)
    k = pr.case.kc.double().view(-1, H, D) * pr.case.ks.double().unsqueeze(-1)
    v = pr.case.v.double().view(-1, H, D)
    for n_bits, sym in ((8, False), (4, True), (2, True), (3, False)):
        _, _, pq = quantise64(dfn, n_bits, sym)
        mine = torch.einsum("hqk,khd->qhd", pq, dfn["v"])
        ref = wr.attention_map_quant(q, k, v, pr.n, n_bits, sym)
        assert ref.dtype == torch.float64
        assert float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (n_bits, sym)


def test_probe_cases_reach_what_they_name():
    """(host arithmetic only) over SHAPES: every Lq, Lk and H the issue lists; sole holders on lanes 0 and 15, both query blocks,
    all 8 waves, workgroups 1 and 2 and the clamped last query of a ragged block; a block, a wave and a workgroup as holders; a sole
    holder's key on every slot of a tile and in tiles 0 - 4; two heads that give one key to different queries; keys under the eps
    floor in the sym and the asym form; masked keys behind a ragged tile."""
    assert {s[0] for s in SHAPES} == {1, 31, 33, 255, 257, 300, 513} and {s[1] for s in SHAPES} == {1, 5, 63, 64, 65, 128, 129, 192, 193, 257}
    assert {s[2] for s in SHAPES} == {1, 3}
    soles, slots, tiles, kinds, ragged_last, heads_differ, floored, masked = set(), set(), set(), set(), False, False, 0, False
    for pr, _ in cases():
        for c, x in enumerate(pr.narrow):
            if pr.broad and len(x) == 1:
                soles.add(x[0])
                ragged_last |= x[0] == pr.Lq - 1 and pr.Lq % 32 != 0
                keys = torch.nonzero(pr.holder == c)[:, 1]
                slots |= set((keys % 64).tolist())
                tiles |= set((keys // 64).tolist())
            elif pr.broad:
                kinds.add("block" if x[0] in BLOCK else "wave" if x[0] in WAVE else "workgroup")
        if pr.H > 1 and pr.broad:
            heads_differ |= bool(((pr.holder[0] != pr.holder[1]) & (pr.holder[0] >= 0) & (pr.holder[1] >= 0)).any())
        dfn = dfn_cpu(pr)
        for sym in (True, False):
            low = dfn["cmax"] / levels_of(2, sym) < EPS[sym]
            assert bool((low == ~pr.favoured).all()), pr.name
            floored += int(low.sum())
        masked |= pr.tail > 0 and pr.n % 64 != 0
    assert {q % 16 for q in soles} >= {0, 15} and {(q // 16) % 2 for q in soles} == {0, 1} and {(q // 32) % 8 for q in soles} == set(range(8))
    assert {q // 256 for q in soles} == {0, 1, 2} and ragged_last and kinds == {"block", "wave", "workgroup"}
    assert slots == set(range(64)) and tiles == {0, 1, 2, 3, 4}, (sorted(set(range(64)) - slots), tiles)
    assert heads_differ and floored > 0 and masked


def test_generator_refuses_ties_and_sums_that_round():
    probe_case(300, 129, 3)
    for kw, word in ((dict(narrow_size=3), "not dyadic"), (dict(broad_mult=(2, 4)), "tie"), (dict(broad_mult=(8, 2)), "tie"),
                     (dict(broad_mult=(16, 4)), "within 1/8 of a half-integer"), (dict(qamp=33), "multiple of every query scale")):
        with pytest.raises(ValueError, match=word):
            probe_case(300, 129, 3, **kw)
    # a quotient inside delta_tie of family B on the float64 definition itself: cmax / 2 at 255 levels is 127.5
    pr = probe_case(300, 129, 3, check_levels=())
    dfn = dict(dfn_cpu(pr))
    dfn["P"] = dfn["P"].clone()
    h, k_ = [int(x) for x in torch.nonzero(pr.holder >= 0)[0]]
    other = int(torch.nonzero(dfn["P"][h, :, k_] < dfn["cmax"][h, k_])[0])
    dfn["P"][h, other, k_] = dfn["cmax"][h, k_] / 2
    assert expectation(dfn, 8, False)[2] > 0 and expectation(dfn_cpu(pr), 8, False)[2] == 0


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_model_passes_and_mutants_fail(shape):
    """The fp32 model passes A, and B on the probe and the Gaussian case at every width with the float64 reference's excused share
    <= 1 % (the probe cases excuse nothing); every mutant fails A on every shape that holds what it breaks -- each one somewhere;
    truncation fails B at n_bits = 2 asym and the dropped lo term B at 8 bits (A cannot see either: see the module docstring)."""
    pr, gs = cases()[shape]
    dfn = dfn_cpu(pr)
    msg = check_exact(model(pr, 2, True), dfn, pr.name)
    assert msg is None, msg
    # the expected value is dyadic: the quantised map and the output are exact in fp32
    _, _, pq = quantise64(dfn, 2, True)
    assert torch.equal(pq.float().double(), pq)
    for mutant in MUTANTS:
        if applies(mutant, pr):
            assert check_exact(model(pr, 2, True, mutant), dfn, pr.name) is not None, (mutant, pr.name)
    for case_ in (pr, gs):
        d = dfn_cpu(case_)
        for n_bits in BITS:
            for sym in (1, 0):
                msg, ratio, share = check_bound(model(case_, n_bits, sym), d, n_bits, sym, case_.name)
                assert msg is None and ratio < 1 and share <= 0.01, (msg, ratio, share, n_bits, sym)
                assert case_ is gs or share == 0
    if applies("trunc", pr):
        assert check_bound(model(pr, 2, 0, "trunc"), dfn, 2, 0, pr.name)[0] is not None, pr.name
    if pr.n >= 63 and pr.Lq > 1:
        assert check_bound(model(gs, 8, 0, "no_lo"), dfn_cpu(gs), 8, 0, gs.name)[0] is not None, gs.name


def test_every_mutant_applies_somewhere():
    for mutant in MUTANTS + ["trunc"]:
        n = sum(applies(mutant, pr) for pr, _ in cases())
        assert n >= (2 if mutant in ("no_wave7", "no_second_workgroup") else 4), (mutant, n)
