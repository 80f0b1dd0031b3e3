"""The fp16 forms of the flash-attention kernel (csrc/attention.hip, dtype WANQ_F16) on the probes of
tests/test_gpu_attention_probes.py: the same data generator (int8 codes times power-of-two scales, exact in bf16 AND fp16, so
that both types and the float64 definition see the same numbers), the same families, through the same two routes (wan.ops and
the C ABI), at fp16's unit roundoff:
  A  key census    o = count / n at one fp16 rounding: the exact-integer check of the fp16 A/B lane map and of every tile-edge
                   and k_len mask.
  B  windows       o = count / w at one fp16 rounding.
  C  bound         |o - o64| <= (2^-10 + 2^-14) (P64 |V|) + 2^-11 |o64| + 2^-22 (sum_deep |v_k| + n_deep |o64|) / L elementwise
                   (derivation: profiles/PARITY_NOTES.md).  The last term is the range statement of DESIGN 3.2: a key more than 22
                   log2 units below its row's maximum may leave fp16's normal range in P' = 2^(s - reference + 8) and, at worst, lose
                   all of its weight, which is below 2^-22 of the largest key's; L = sum_k 2^(s_k - max) >= 1.
  C' deep tail     one key at score 0 and 16000 keys at -t, t in {11.5, 15.5, 19.5}, spike first and spike last, under C's bound:
                   a form without the exponent headroom (P' subnormal or flushed at these depths) is off by percents.
  D  stores stay inside their rows, Lq = 0, the stride refusals and the dtype refusals of the ABI.
  E  every fp16 form is closer to the float64 definition than its bf16 twin on the same case.
  F  the 8- and 4-wave forms are bit-identical, the split forms within one fp16 unit of the unsplit one.
  G  |v| up to 60000 stays finite and under C's bound."""
import math

import pytest
import torch

import test_gpu_attention_probes as P
from test_gpu_attention_probes import D, DEV, POW2_SCALES, SENTINEL, WANQ_E_SHAPE, WANQ_OK

pytestmark = pytest.mark.gpu
WANQ_E_ARG = 1

F16_FORMS = {  # name -> (kind, splits, wanq_attention_select_form value)
    "fp16-8w": ("fp16", 1, 0),
    "fp16-4w": ("fp16", 1, 1 << 40),
    "fp16-split2": ("fp16", 2, None),
    "fp16-split3": ("fp16", 3, None),
    "fp16-split5": ("fp16", 5, None),
    "qk8-fp16": ("qk8", 1, None),
    "qk8-fp16-split3": ("qk8", 3, None),
}
TWINS = {"fp16-8w": "bf16-8w", "fp16-split3": "bf16-split3", "qk8-fp16": "qk8"}
DEEP = 22.0  # log2 units below the row maximum down to which P' is a normal fp16 number


def as_f16(case):
    """The case with q, k and V exact in fp16 AND bf16 (asserted): the few V entries below fp16's normal range become 0 in both
    (bf16 holds them, fp16 would need a subnormal).  Returns the same Case object, so the bf16 twins run on the same numbers."""
    tiny = case.v.float().abs() < 2.0 ** -14
    case.v[tiny] = 0
    v16 = case.v.to(torch.float16)
    assert torch.equal(v16.float(), case.v.float()) and torch.isfinite(v16.float()).all(), "V must be exact in fp16 and bf16"
    for codes, scales in ((case.qc, case.qs), (case.kc, case.ks)):
        x = codes.float().view(codes.shape[0], case.H, D) * scales.view(-1, case.H, 1)
        assert torch.equal(x.to(torch.float16).float(), x) and torch.equal(x.to(torch.bfloat16).float(), x), "codes * scale must be exact in fp16 and bf16"
        assert not ((x != 0) & (x.abs() < 2.0 ** -8)).any(), "q * c and k stay normal fp16 numbers"
    return case


def f16_operands(case):
    q, k, v = case.bf16()
    return q.to(torch.float16), k.to(torch.float16), v.to(torch.float16)


def run_form16(form, case, scale=None, out=None, ws=None, dtype_code=None):
    """tests/test_gpu_attention_probes.run_form for the fp16 forms: scale None and no out -> wan.ops, otherwise the C ABI."""
    from viditq_extension import _C
    from wan import ops

    kind, splits, sel = F16_FORMS[form]
    H, Lq, Lk = case.H, case.Lq, case.n
    code = _C.F16 if dtype_code is None else dtype_code
    prev = _C.lib.wanq_attention_select_form(sel) if sel is not None else None
    try:
        if kind == "fp16":
            q, k, v = f16_operands(case)
        else:
            q, k, v = case.q8()
            v = v.to(torch.float16)
        if scale is None and out is None:
            o = (ops.attention if kind == "fp16" else ops.attention_qk8)(q, k, v, H, case.k_len, splits=splits)
            assert o.dtype == torch.float16
            return o
        scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
        if out is None:
            out = torch.empty(Lq, H * D, dtype=torch.float16, device=DEV)
        nbytes = _C.lib.wanq_attention_split_workspace(Lq, H, D, splits)
        if ws is None and splits > 1:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        if kind == "qk8":
            _C.call("wanq_attention_qk8_fwd", _C.ptr(q.codes), _C.ptr(q.scales), q.stride, _C.ptr(k.codes), _C.ptr(k.scales), k.stride,
                    _C.ptr(v), _C.ptr(out), code, Lq, Lk, H, D, q.codes.stride(0), k.codes.stride(0), v.stride(0), out.stride(0),
                    scale, splits, _C.ptr(ws), nbytes, _C.stream())
        elif splits > 1:
            _C.call("wanq_attention_fwd_split", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(out), code, Lq, Lk, H, D, q.stride(0),
                    k.stride(0), v.stride(0), out.stride(0), scale, splits, _C.ptr(ws), nbytes, _C.stream())
        else:
            _C.call("wanq_attention_fwd", _C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(out), code, Lq, Lk, H, D, q.stride(0), k.stride(0),
                    v.stride(0), out.stride(0), scale, _C.stream())
        return out
    finally:
        if prev is not None:
            _C.lib.wanq_attention_select_form(prev)


def check_counts16(out, expect, what):
    """|o - count/n| <= 2^-11 count/n (one fp16 rounding of the result) + 2^-60; expect [Lq, H*128] float64."""
    assert out.dtype == torch.float16
    err = (out.double().cpu() - expect).abs()
    tol = 2.0 ** -11 * expect.abs() + 2.0 ** -60
    bad = ~(err <= tol)
    if bad.any():
        r, c = [int(x) for x in torch.nonzero(bad)[0]]
        return (f"{what}: {int(bad.sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}; first at query {r} head {c // D} "
                f"channel {c % D}: got {out[r, c].item()} expected {expect[r, c].item():.6f}")
    return None


def definition64_deep(case, scale):
    """o64, P64 |v| (as tests/test_gpu_attention_probes.definition64) and the range term 2^-22 (sum_deep |v_k| + n_deep |o64|) / L,
    deep = more than DEEP - 2^-6 log2 units below the row maximum (2^-6: far above the fp32 rounding of a score)."""
    q, k, v = case.f64()
    t = torch.einsum("qhd,khd->hqk", q, k) * (float(torch.tensor(scale, dtype=torch.float32)) * math.log2(math.e))
    m = t.max(dim=-1, keepdim=True).values
    w = torch.exp2(t - m)
    L = w.sum(dim=-1, keepdim=True)
    p = w / L
    o = torch.einsum("hqk,khd->qhd", p, v)
    a = torch.einsum("hqk,khd->qhd", p, v.abs())
    deep = (t < m - (DEEP - 2.0 ** -6)).double()
    dv = torch.einsum("hqk,khd->qhd", deep, v.abs())
    nd = deep.sum(dim=-1).transpose(0, 1).unsqueeze(-1)  # [Lq, H, 1]
    extra = 2.0 ** -22 * (dv + nd * o.abs()) / L.squeeze(-1).transpose(0, 1).unsqueeze(-1)
    Lq = case.Lq
    return o.reshape(Lq, -1), a.reshape(Lq, -1), extra.reshape(Lq, -1)


def bound_excess16(out, o64, pv_abs, extra):
    """Family C's fp16 bound.  Returns (number of elements out of bound, worst excess, largest err / bound)."""
    err = (out.double() - o64).abs()
    tol = (2.0 ** -10 + 2.0 ** -14) * pv_abs + 2.0 ** -11 * o64.abs() + extra
    bad = ~(err <= tol)
    err = torch.nan_to_num(err, nan=float("inf"))
    ok = tol > 0
    ratio = (err[ok] / tol[ok]).max().item() if ok.any() else 0.0
    return int(bad.sum()), (err - tol).max().item(), ratio


_REF = {}


def reference(key, case, scale):
    """The float64 definition of a case, computed once and shared by the tests that need it."""
    if key not in _REF:
        _REF[key] = definition64_deep(case, scale)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- A. key census
@pytest.mark.parametrize("form", list(F16_FORMS))
def test_key_census(form):
    fails, i = [], 0
    for Lk in P.CENSUS_LK:
        for tail in (0, 70):
            Lq, H = P.CENSUS_LQ[(i * 2 + (1 if tail else 0)) % 5], (1, 3)[(i + (1 if tail else 0)) % 2]
            case, expect = P.census_case(Lq, Lk, H, tail)
            msg = check_counts16(run_form16(form, as_f16(case)), expect, f"Lk={Lk} tail={tail} Lq={Lq} H={H}")
            if msg:
                fails.append(msg)
        i += 1
    assert not fails, f"{form}: {len(fails)} of {2 * len(P.CENSUS_LK)} cases\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- B. windows
@pytest.mark.parametrize("form", list(F16_FORMS))
def test_windows(form):
    fails = []
    for k_len, Lq, H, w, layout in P.WINDOW_CASES:
        case, expect, wins = P.window_case(k_len, Lq, H, w, layout)
        msg = check_counts16(run_form16(form, as_f16(case)), expect, f"k_len={k_len} Lq={Lq} H={H} w={w} windows at {wins}")
        if msg:
            fails.append(msg)
    assert not fails, f"{form}: {len(fails)} of {len(P.WINDOW_CASES)} cases\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- C. bound
@pytest.mark.parametrize("form", list(F16_FORMS))
def test_staircase(form):
    fails, worst = [], 0.0
    for step in P.STAIR:
        for desc in (False, True):
            case = as_f16(P.staircase_case(step, desc))
            o64, pva, extra = reference(("stair", step, desc), case, POW2_SCALES[0])
            n_bad, excess, ratio = bound_excess16(run_form16(form, case, scale=POW2_SCALES[0]), o64, pva, extra)
            worst = max(worst, ratio)
            if n_bad:
                fails.append(f"step {step} {'descending' if desc else 'ascending'}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}")
    print(f"PROBE staircase {form}: largest err/bound {worst:.3f}")
    assert not fails, f"{form}:\n" + "\n".join(fails)


def form_scale(kind, which):
    """The scales of the bf16 file: the two whose c is a power of two for the 16-bit forms, 1 / sqrt(128) and the first of them
    for the int8 forms."""
    return POW2_SCALES[which] if kind in ("fp16", "bf16") else (1.0 / math.sqrt(D), POW2_SCALES[0])[which]


def random_case16(i):
    Lq, Lk, H, k_len = P.RANDOM_SHAPES[i]
    return as_f16(P.random_case(Lq, Lk, H, k_len, (-7, -5, -4)[i % 3]))


@pytest.mark.parametrize("form,which", [(f, i) for f in F16_FORMS for i in (0, 1)])
def test_random_data_under_the_derived_bound(form, which):
    scale = form_scale(F16_FORMS[form][0], which)
    fails, worst = [], 0.0
    for i, (Lq, Lk, H, k_len) in enumerate(P.RANDOM_SHAPES):
        case = random_case16(i)
        o64, pva, extra = reference(("random", i, scale), case, scale)
        n_bad, excess, ratio = bound_excess16(run_form16(form, case, scale=scale), o64, pva, extra)
        worst = max(worst, ratio)
        if n_bad:
            fails.append(f"Lq={Lq} Lk={Lk} H={H} k_len={k_len}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}")
    print(f"PROBE random {form} scale {scale:.6f}: largest err/bound {worst:.3f}")
    assert not fails, f"{form} scale={scale}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- C'. deep tail
TAIL_N, TAIL_LQ, TAIL_H = 16000, 33, 2
TAIL_DEPTHS = [11.5, 15.5, 19.5]


def deep_tail_case(t, spike_last):
    """Per head one key (the spike) scores exactly 0 and TAIL_N keys score exactly -t log2 units for every query, at scale =
    2^-3 / log2(e): q * c = 1 on channels 0-15, the tail keys hold code 2 t x key scale 2^-5 = t / 16 with a minus sign on those 16
    channels, the spike key is 0.  V = 1 on channels 0-63 for the tail keys and on channels 64-127 for the spike.  Closed form:
    o = N 2^-t / (1 + N 2^-t) on the tail's channels and 1 / (1 + N 2^-t) on the spike's."""
    n = TAIL_N + 1
    spike = n - 1 if spike_last else 0
    code = int(round(2 * t))
    assert code == 2 * t and code <= 127
    kc = torch.zeros(n, TAIL_H, D, dtype=torch.int8)
    kc[:, :, :16] = -code
    kc[spike] = 0
    qc = torch.zeros(TAIL_LQ, TAIL_H, D, dtype=torch.int8)
    qc[:, :, :16] = 8
    v = torch.zeros(n, TAIL_H, D)
    v[:, :, :64] = 1.0
    v[spike] = 0.0
    v[spike, :, 64:] = 1.0
    case = P.Case(qc.view(TAIL_LQ, -1), torch.ones(TAIL_LQ, TAIL_H), kc.view(n, -1), torch.full((n, TAIL_H), 2.0 ** -5), v.view(n, -1), TAIL_H)
    mass = TAIL_N * 2.0 ** -t
    expect = torch.zeros(TAIL_LQ, TAIL_H, D, dtype=torch.float64)
    expect[:, :, :64] = mass / (1.0 + mass)
    expect[:, :, 64:] = 1.0 / (1.0 + mass)
    return as_f16(case), expect.view(TAIL_LQ, -1)


@pytest.mark.parametrize("form", list(F16_FORMS))
def test_deep_tail(form):
    fails, worst = [], 0.0
    for t in TAIL_DEPTHS:
        for spike_last in (False, True):
            case, expect = deep_tail_case(t, spike_last)
            o64, pva, extra = reference(("tail", t, spike_last), case, POW2_SCALES[0])
            assert (o64.cpu() - expect).abs().max().item() < 1e-6  # the case is what it says: the definition gives the closed form (its log2(e) is float64's, c is fp32's 2^-3)
            assert float(extra.max()) == 0.0  # every key is less than 22 units deep: the range term is not in play
            n_bad, excess, ratio = bound_excess16(run_form16(form, case, scale=POW2_SCALES[0]), expect.to(DEV), pva, extra)
            worst = max(worst, ratio)
            if n_bad:
                fails.append(f"t={t} spike {'last' if spike_last else 'first'}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}")
    print(f"PROBE deep tail {form}: largest err/bound {worst:.3f}")
    assert not fails, f"{form}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- D. small items
@pytest.mark.parametrize("form", list(F16_FORMS))
def test_stores_stay_inside_their_rows(form):
    from viditq_extension import _C

    H, Lk = 2, 300
    splits = F16_FORMS[form][1]
    for Lq in (1, 130, 257):
        case = as_f16(P.random_case(Lq, Lk, H, None, -5))
        plain = run_form16(form, case)
        big = torch.full((Lq + 3, H * D + 64), SENTINEL, dtype=torch.float16, device=DEV)
        assert float(big[0, 0]) == SENTINEL  # exact in fp16
        need = _C.lib.wanq_attention_split_workspace(Lq, H, D, splits) // 4
        ws = torch.full((need + 4096,), SENTINEL, dtype=torch.float32, device=DEV)
        run_form16(form, case, out=big[:Lq, : H * D], ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(big[:Lq, : H * D], plain), Lq
        assert bool((big[Lq:] == SENTINEL).all()) and bool((big[:, H * D:] == SENTINEL).all()), Lq
        assert bool((ws[need:] == SENTINEL).all()), Lq


def _abi_args16(entry, code, **kw):
    """tests/test_gpu_attention_probes._abi_args with 16-bit buffers and the dtype code replaced (the buffers are 2 bytes per
    element under either 16-bit type; o keeps the sentinel's bf16 bit pattern, compared bit for bit)."""
    from viditq_extension import _C

    args, o, keep = P._abi_args(entry, **kw)
    at = 8 if entry == "wanq_attention_qk8_fwd" else 4
    assert args[at] == _C.BF16
    args[at] = code
    return args, o, keep


@pytest.mark.parametrize("entry", P.ENTRIES)
def test_no_queries_is_ok_and_writes_nothing(entry):
    from viditq_extension import _C

    args, o, keep = _abi_args16(entry, _C.F16, Lq=0)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())


@pytest.mark.parametrize("entry", P.ENTRIES)
def test_stride_rules_are_refused_through_the_abi(entry):
    from viditq_extension import _C

    C = 2 * D
    rules = [((C, C, C, C - 8), "token stride smaller than heads*head_dim"), ((C, C, C - 8, C), "token stride smaller than heads*head_dim"),
             ((C, C, C, C + 4), "strides must be multiples of 8 elements"), ((C, C, C + 12, C), "strides must be multiples of 8 elements"),
             ((C, C, 1 << 24, C), "k / v token stride must be below 2^24 elements")]
    if entry != "wanq_attention_qk8_fwd":
        rules += [((C - 8, C, C, C), "token stride smaller than heads*head_dim"), ((C, C - 8, C, C), "token stride smaller than heads*head_dim"),
                  ((C + 4, C, C, C), "strides must be multiples of 8 elements"), ((C, C + 12, C, C), "strides must be multiples of 8 elements"),
                  ((C, 1 << 24, C, C), "k / v token stride must be below 2^24 elements")]
    for strides, message in rules:
        args, o, keep = _abi_args16(entry, _C.F16, strides=strides)
        assert getattr(_C.lib, entry)(*args) == WANQ_E_SHAPE, strides
        assert message in _C.lib.wanq_last_error().decode(), (strides, _C.lib.wanq_last_error().decode())
        torch.cuda.synchronize()
        assert bool((o == SENTINEL).all())


@pytest.mark.parametrize("entry", P.ENTRIES)
def test_other_dtype_codes_are_refused(entry):
    """WANQ_F32 and an unknown code: WANQ_E_ARG, a message that names the two accepted types, nothing written; WANQ_F16 on the same
    arguments is accepted (on the parent commit it was refused like the others)."""
    from viditq_extension import _C

    for code in (_C.F32, 77):
        args, o, keep = _abi_args16(entry, code)
        assert getattr(_C.lib, entry)(*args) == WANQ_E_ARG, code
        msg = _C.lib.wanq_last_error().decode()
        assert "WANQ_BF16" in msg and "WANQ_F16" in msg, msg
        torch.cuda.synchronize()
        assert bool((o == SENTINEL).all())
    args, o, keep = _abi_args16(entry, _C.F16)
    assert getattr(_C.lib, entry)(*args) == WANQ_OK, _C.lib.wanq_last_error().decode()
    torch.cuda.synchronize()
    assert not bool((o == SENTINEL).any())


# ---------------------------------------------------------------------------------------------------------------- E. fp16 is what it claims
def rel_fro(out, o64):
    return ((out.double() - o64).norm() / o64.norm()).item()


@pytest.mark.parametrize("form", list(TWINS))
def test_fp16_is_closer_to_the_definition_than_its_bf16_twin(form):
    """rel-Frobenius error against the float64 definition, per random shape of family C: fp16 form < bf16 twin (a relation, not a
    tuned number: 2^-11 against 2^-8 in P and in the output leaves about 1/8)."""
    scale = form_scale(F16_FORMS[form][0], 0)
    fails = []
    for i, (Lq, Lk, H, k_len) in enumerate(P.RANDOM_SHAPES):
        case = random_case16(i)
        o64 = reference(("random", i, scale), case, scale)[0]
        e16 = rel_fro(run_form16(form, case, scale=scale), o64)
        e_b = rel_fro(P.run_form(TWINS[form], case, scale=scale), o64)
        print(f"PROBE twin {form} Lq={Lq} Lk={Lk} H={H} k_len={k_len}: fp16 {e16:.3e} bf16 {e_b:.3e} ratio {e16 / e_b:.3f}")
        if not e16 < e_b:
            fails.append(f"Lq={Lq} Lk={Lk} H={H} k_len={k_len}: fp16 {e16:.3e} >= bf16 {e_b:.3e}")
    assert not fails, f"{form} against {TWINS[form]}:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- F. forms agree
def _gauss16(Lq, Lk, H):
    g = torch.Generator().manual_seed(Lq * 31 + Lk)  # the data of tests/test_gpu_block.py's attention tests, rounded to fp16
    q = (torch.randn(Lq, H * D, generator=g) * 1.5).to(torch.float16)
    k = (torch.randn(Lk, H * D, generator=g) * 1.5).to(torch.float16)
    v = torch.randn(Lk, H * D, generator=g).to(torch.float16)
    if Lk > 70:
        k[69] *= 4.0
    return q.to(DEV), k.to(DEV), v.to(DEV)


@pytest.mark.parametrize("Lq,Lk,H,klen", [(300, 300, 2, None), (515, 640, 12, 601), (1, 17, 1, None), (17, 65, 1, 33), (100, 512, 2, None),
                                           (130, 1100, 2, 1061), (257, 1500, 3, None), (2050, 2050, 4, None)])
def test_both_workgroup_forms_bit_identical(Lq, Lk, H, klen):
    from viditq_extension import _C
    from wan import ops

    q, k, v = _gauss16(Lq, Lk, H)
    prev = _C.lib.wanq_attention_select_form(0)
    try:
        o8 = ops.attention(q, k, v, H, klen, splits=1)
        _C.lib.wanq_attention_select_form(1 << 40)
        o4 = ops.attention(q, k, v, H, klen, splits=1)
    finally:
        _C.lib.wanq_attention_select_form(prev)
    assert o8.dtype == torch.float16 and torch.equal(o8, o4)


@pytest.mark.parametrize("Lq,Lk,H,klen,splits", [(300, 2100, 2, None, 2), (257, 2500, 1, 2437, 3), (64, 4096, 3, None, 4), (500, 130, 2, None, 5)])
def test_split_forms_within_one_fp16_unit_of_the_unsplit_one(Lq, Lk, H, klen, splits):
    """The shapes of test_flash_attention_split_kv_matches_unsplit_and_fp32 with its criterion at fp16's unit: the fp32 merge
    order moves a result by at most one fp16 rounding at the output's magnitude."""
    from wan import ops

    q, k, v = _gauss16(Lq, Lk, H)
    k[Lk // 2 + 5] *= 4.0
    one = ops.attention(q, k, v, H, klen, splits=1)
    many = ops.attention(q, k, v, H, klen, splits=splits)
    assert many.dtype == torch.float16
    assert float((many.float() - one.float()).abs().max()) <= 2.0 ** -10 * float(one.float().abs().max())


# ---------------------------------------------------------------------------------------------------------------- G. the edge of the format
@pytest.mark.parametrize("form", list(F16_FORMS))
def test_large_values_stay_finite_and_under_the_bound(form):
    """|v| up to 60000 (fp16's largest is 65504) under moderate scores: P' up to 2^14 times such a V lives in the fp32
    accumulators only, the output is a convex combination of V and finite, and the bound of C scales with |V|."""
    Lq, Lk, H = 130, 1100, 2
    case = P.random_case(Lq, Lk, H, None, -5)
    g = torch.Generator().manual_seed(9)
    v = (torch.randn(Lk, H * D, generator=g) * 25000).clamp(-60000, 60000)
    v[::7] = 60000.0 * (torch.randint(0, 2, v[::7].shape, generator=g) * 2 - 1)
    case.v = v.to(torch.bfloat16)
    assert float(case.v.float().abs().max()) <= 60160  # bf16's neighbour of 60000, below 65504
    case = as_f16(case)
    scale = form_scale(F16_FORMS[form][0], 0)
    o64, pva, extra = reference(("large", scale), case, scale)
    out = run_form16(form, case, scale=scale)
    assert bool(torch.isfinite(out.float()).all())
    n_bad, excess, ratio = bound_excess16(out, o64, pva, extra)
    print(f"PROBE large values {form}: largest err/bound {ratio:.3f}")
    assert n_bad == 0, f"{form}: {n_bad} elements out of bound; worst excess {excess:.3e}; err/bound {ratio:.3f}"
