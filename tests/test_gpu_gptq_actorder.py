"""gptq.act_order and the one-pass Gram kernel on the GPU (wanq_gptq_block_gidx in csrc/gptq.hip, csrc/gram.hip, qdiff/base/gptq.py).

a. wanq_gptq_block_gidx against the host model gptq_block_host on the same column map, bit for bit (codes, errors, updated weight), on
   the exact operands of tests/test_gpu_gptq.py section b (every fp32 operation exact), over row counts, block places (odd c0
   included), block widths, group counts and maps (identity, a permutation's, alternating); the identity map against wanq_gptq_block;
   a map with indices outside 0..G-1 equals the host model on the clamped map (the clamp is the contract).
b. End to end: gptq_solve(act_order=True) on the GPU is bit-equal to gptq_solve_host on a real factor; a QuantizedLinear of the
   shipped act_order config, requantised and taken over by kernel mode's HipLinearWq16, gives simulation mode's output.
c. wanq_gram_accumulate: exact on integer operands (one tile, ragged tiles, 2 x 2 and 3 x 3 tile grids), symmetric to the bit,
   guard words intact, accumulating; on random operands within the bound of an fp32 sum, and bit-identical across calls and base
   pointers.
d. The layer objective with act_order is not above plain GPTQ's on inputs whose channel energies spread over decades (the inputs
   were chosen with the host model on the CPU: act_order / plain 0.56 at this shape and seed, profiles/gptq.txt)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
DEV = "cuda:0"
GUARD = 64


def _guarded(t, fill, strided=False):
    """a copy of `t` on the GPU inside a buffer with GUARD sentinel elements in front and behind (`strided`: beside every row too,
    the view has a row stride of K + GUARD): -> (view, buffer)"""
    n = t.numel()
    if strided:
        N, K = t.shape
        buf = torch.full((GUARD + N * (K + GUARD),), fill, dtype=t.dtype, device=DEV)
        view = buf[GUARD:].view(N, K + GUARD)[:, :K]
    else:
        buf = torch.full((n + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
        view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    return view, buf


def _guards_intact(view, buf, fill):
    mask = torch.ones_like(buf, dtype=torch.bool)
    if view.dim() == 2 and view.stride(0) == view.shape[1] + GUARD:
        N, K = view.shape
        mask[GUARD:].view(N, K + GUARD)[:, :K] = False
    else:
        mask[GUARD:GUARD + view.numel()] = False
    return bool((buf[mask] == fill).all())


# ---- a. the block kernel with a column map ----------------------------------------------------------------------------------------
K_A = 192


def _exact_u(K, g):
    """upper triangular: diagonal in {1, 1/2, 1/4}; u[j, k] in {+-1/4, +-1/2} for about a tenth of the k > j with j % 3 < k % 3, so that
    an error travels through at most two updates and every value stays on a 2^-10 lattice"""
    j, k = torch.arange(K)[:, None], torch.arange(K)[None, :]
    allowed = (k > j) & ((j % 3) < (k % 3)) & (torch.rand(K, K, generator=g) < 0.1)
    vals = torch.tensor([0.25, 0.5, -0.25, -0.5])[torch.randint(0, 4, (K, K), generator=g)]
    u = torch.where(allowed, vals, torch.zeros(()))
    return (u + torch.diag(2.0 ** -torch.randint(0, 3, (K,), generator=g).float())).contiguous()


def _exact_case(N, G, g_idx, seed):
    """W4 with zero points on G groups: delta a power of two, integer zp, w on the 2^-6 lattice within a few delta of ITS column's
    group (through the map), the last row clamping on both sides"""
    g = torch.Generator().manual_seed(seed)
    delta = 2.0 ** -torch.randint(1, 4, (N, G), generator=g).float()
    zp = torch.randint(-3, 4, (N, G), generator=g).float()
    dcol = delta[:, g_idx]
    w = torch.round(torch.randint(-64 * 3, 64 * 3 + 1, (N, K_A), generator=g).float() / 64 * dcol * 64) / 64
    w[N - 1, 0::2] = 12.0 * dcol[N - 1, 0::2]
    w[N - 1, 1::4] = -12.0 * dcol[N - 1, 1::4]
    return w, _exact_u(K_A, g), delta, zp


def _maps(G, seed):
    j = torch.arange(K_A)
    if G == 1:
        return {"one group": torch.zeros(K_A, dtype=torch.long)}
    perm = torch.randperm(K_A, generator=torch.Generator().manual_seed(seed))
    a = (j // 2) % G  # neighbouring columns alternate between group a and group G - 1 - a
    return {"identity": j // (K_A // G), "permutation": perm // (K_A // G), "alternating": torch.where(j % 2 == 0, a, G - 1 - a)}


def _gidx_gpu(w, u, delta, zp, g_idx, c0, cols, plain_group_size=None):
    """one launch on guarded buffers: -> (codes, w, err) on the CPU; every sentinel is checked.  `plain_group_size`: wanq_gptq_block"""
    from viditq_extension import fused

    N, K = w.shape
    wv, wbuf = _guarded(w, 7.5, strided=True)
    cv, cbuf = _guarded(torch.full((N, K), 99, dtype=torch.int8), 99)
    ev, ebuf = _guarded(torch.zeros(N, cols), -3.25)
    if plain_group_size is not None:
        fused.gptq_block_(wv, u.to(DEV), delta.to(DEV), zp.to(DEV), plain_group_size, -8, 7, cv, ev, c0, cols)
    else:
        fused.gptq_block_gidx_(wv, u.to(DEV), delta.to(DEV), zp.to(DEV), g_idx.to(device=DEV, dtype=torch.int32), -8, 7, cv, ev, c0, cols)
    torch.cuda.synchronize()
    assert _guards_intact(wv, wbuf, 7.5) and _guards_intact(cv, cbuf, 99) and _guards_intact(ev, ebuf, -3.25), "a sentinel was overwritten"
    return cv.cpu(), wv.cpu(), ev.cpu()


def _host(w, u, delta, zp, g_idx, c0, cols):
    from qdiff.base import gptq

    hw, hc = w.clone(), torch.full(w.shape, 99, dtype=torch.int8)
    he = gptq.gptq_block_host(hw, u, delta, zp, None, -8, 7, hc, c0, cols, g_idx)
    return hc, hw, he


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("G", [1, 12])
@pytest.mark.parametrize("N", [1, 5, 130])
def test_gidx_kernel_equals_the_host_model_bit_for_bit(N, G):
    """(N = 130: 17 workgroups, the last with two rows; cols 1, 7: lanes without columns; c0 = 3: odd, which wanq_gptq_block refuses)"""
    moved = 0
    for name, g_idx in _maps(G, seed=N).items():
        assert g_idx.min() == 0 and g_idx.max() == G - 1
        w, u, delta, zp = _exact_case(N, G, g_idx, seed=100 * N + G)
        for c0 in (0, 3, 64):
            for cols in (1, 7, 128):
                hc, hw, he = _host(w, u, delta, zp, g_idx, c0, cols)
                gc, gw, ge = _gidx_gpu(w, u, delta, zp, g_idx, c0, cols)
                where = f"{name} c0={c0} cols={cols}"
                assert torch.equal(gc, hc), where
                assert torch.equal(_bits(ge), _bits(he)), where
                assert torch.equal(_bits(gw), _bits(hw)), where
                assert (gc[:, :c0] == 99).all() and (gc[:, c0 + cols:] == 99).all() and torch.equal(gw[:, :c0], w[:, :c0]), where
                moved += int((he != 0).any()) + int(cols > 1 and not torch.equal(hw[:, c0:c0 + cols], w[:, c0:c0 + cols]))
        hc, _, _ = _host(w, u, delta, zp, g_idx, 0, 128)
        assert (hc[N - 1, :128] == 7).any() and (hc[N - 1, :128] == -8).any()  # the built row clamps on both sides
    assert moved > 9  # the probes are not trivial: errors are made and pushed on


@pytest.mark.parametrize("c0,cols", [(0, 128), (64, 128), (0, 7), (64, 1)])
def test_identity_map_equals_the_plain_block_kernel(c0, cols):
    N, G = 21, 12
    g_idx = torch.arange(K_A) // 16
    w, u, delta, zp = _exact_case(N, G, g_idx, seed=c0 + cols)
    pc, pw, pe = _gidx_gpu(w, u, delta, zp, None, c0, cols, plain_group_size=16)
    gc, gw, ge = _gidx_gpu(w, u, delta, zp, g_idx, c0, cols)
    assert torch.equal(gc, pc) and torch.equal(_bits(ge), _bits(pe)) and torch.equal(_bits(gw), _bits(pw))
    assert (pe != 0).any()


def test_indices_outside_the_groups_are_clamped():
    """-1 and G (and far beyond) in the map: the launch completes and computes what the host model computes on the clamped map"""
    N, G = 5, 12
    good = torch.arange(K_A) // 16
    bad = good.clone()
    bad[0::5], bad[1::7], bad[2::11], bad[3::13] = -1, G, -(2 ** 31), 2 ** 31 - 1
    clamped = bad.clamp(0, G - 1)
    assert (bad < 0).any() and (bad >= G).any() and not torch.equal(clamped, good)
    w, u, delta, zp = _exact_case(N, G, clamped, seed=7)
    for c0, cols in ((0, 128), (3, 128), (64, 7)):
        hc, hw, he = _host(w, u, delta, zp, clamped, c0, cols)
        gc, gw, ge = _gidx_gpu(w, u, delta, zp, bad, c0, cols)
        assert torch.equal(gc, hc) and torch.equal(_bits(ge), _bits(he)) and torch.equal(_bits(gw), _bits(hw))


# ---- b. end to end ----------------------------------------------------------------------------------------------------------------
def _xavier(N, K, g):
    return (torch.rand(N, K, generator=g) * 2 - 1) * (6.0 / (N + K)) ** 0.5


def _spread_hessian(K, rows, g, sigma=1.0):
    """H = X^T X (float64): x = z (I + M / sqrt(K)) diag(s), z and M standard normal, s lognormal: the channels' energies s^2 spread
    over 2 sigma * (range of a normal sample) / ln 10 decades"""
    z = torch.randn(rows, K, generator=g, dtype=torch.float64)
    x = z @ (torch.eye(K, dtype=torch.float64) + torch.randn(K, K, generator=g, dtype=torch.float64) / K ** 0.5)
    x = x * torch.exp(sigma * torch.randn(K, generator=g, dtype=torch.float64))
    return x.T @ x


def _quantizer(group_size, w):
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer

    q = StaticQuantizer(qcfg.create({"n_bits": 4, "sym": False, "group_size": group_size}))
    q.init_quant_params(w.detach().float())
    q.init_done = True
    return q


@pytest.mark.parametrize("block", [128, 33])
def test_act_order_solve_on_the_gpu_is_the_host_models(block):
    from qdiff.base import gptq

    N, K, gs = 96, 256, 64
    g = torch.Generator().manual_seed(block)
    w, H = _xavier(N, K, g).to(DEV), _spread_hessian(K, 4 * K, g)
    U, wp, perm = gptq.gptq_prepare(H.float().to(DEV), w, 0.01, act_order=True)
    assert U.is_cuda and perm.is_cuda and perm.dtype == torch.int64 and not torch.equal(perm.cpu(), torch.arange(K))
    assert torch.equal(perm.cpu(), torch.sort(torch.diagonal(H.float().double()), descending=True, stable=True).indices)
    q = _quantizer(gs, w)
    codes, deq = gptq.gptq_solve(wp, U, q, block, act_order=True, perm=perm)
    h_codes, h_deq = gptq.gptq_solve_host(wp, U, q, block, act_order=True, perm=perm)
    assert codes.is_cuda and codes.dtype == torch.int8 and deq.dtype == torch.float32
    assert torch.equal(codes, h_codes) and torch.equal(_bits(deq), _bits(h_deq))
    G = K // gs
    assert torch.equal(deq, ((codes.float().view(N, G, -1) + q.zero_point.view(N, G, 1)) * q.delta.view(N, G, 1)).view(N, K))
    rtn = q(w)
    assert gptq.objective(w.cpu(), deq.cpu(), H).sum() < gptq.objective(w.cpu(), rtn.cpu(), H).sum()


def test_a_layer_of_the_shipped_config_runs_in_kernel_mode_as_in_simulation_mode():
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from wan.quant_wanx_hip import HipLinearWq16, _to_hip_linear

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "gptq", "w4a16_g128_gptq_actorder_all_linears.yaml"))
    assert cfg.gptq.act_order is True
    N, K, T = 136, 256, 130
    g = torch.Generator().manual_seed(11)
    fp = torch.nn.Linear(K, N, bias=True)
    fp.weight.data.copy_(_xavier(N, K, g))
    fp.bias.data.copy_(torch.randn(N, generator=g) * 0.1)
    fp = fp.to(DEV)
    ql = QuantizedLinear(K, N, True, DEV, cfg, fp, "blocks.0.ffn.0")
    rtn_codes, delta, zp = ql.int_weight.clone(), ql.w_quantizer.delta.clone(), ql.w_quantizer.zero_point.clone()
    ql.requantize_gptq_(_spread_hessian(K, 4 * K, g).float().to(DEV))
    assert not torch.equal(ql.int_weight, rtn_codes)
    assert torch.equal(_bits(ql.w_quantizer.delta), _bits(delta)) and torch.equal(_bits(ql.w_quantizer.zero_point), _bits(zp))
    x = torch.randn(1, T, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.bfloat16)
    hl = _to_hip_linear(ql, None, False, torch.bfloat16, "hip", "blocks.0.ffn.0")
    assert isinstance(hl, HipLinearWq16) and hl.group_size == 128
    sim, hw = ql(x)[0], hl(x[0])
    rel = ((hw.float() - sim.float()).norm() / sim.float().norm()).item()
    print(f"w4a16 g128 gptq act_order layer: kernel vs simulation {rel:.3e}")
    assert torch.isfinite(hw).all() and torch.isfinite(sim).all() and rel < 0.03  # the bar of tests/test_gpu_gptq.py for this comparison


# ---- c. the one-pass Gram kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 72, 136, 264])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gram_onepass_is_exact_symmetric_and_in_bounds(rows, C, dtype):
    """(C = 8: one ragged tile; 72: one tile; 136: 2 x 2 tiles, the second ragged; 264: 3 x 3 with an 8-column edge.  rows = 257: five
    steps of 64 rows, the last holding one.  Every partial sum is an integer below 2^24.)"""
    from viditq_extension import fused

    g = torch.Generator().manual_seed(1000 * rows + C)
    x1, x2 = (torch.randint(-8, 9, (rows, C), generator=g).to(dtype) for _ in range(2))
    h0 = torch.randint(-50, 51, (C, C), generator=g).float()
    h0 = torch.triu(h0) + torch.triu(h0, 1).T
    H, buf = _guarded(h0, -3.25)
    assert fused.gram_accumulate_onepass_(H, x1.to(DEV)) is H
    want1 = h0.double() + x1.double().T @ x1.double()
    assert torch.equal(H.cpu().double(), want1)
    assert torch.equal(_bits(H), _bits(H.T.contiguous()))
    fused.gram_accumulate_onepass_(H, x2.to(DEV).view(1, rows, C))  # a second call accumulates; [..., C] inputs are flattened
    assert torch.equal(H.cpu().double(), want1 + x2.double().T @ x2.double())
    assert torch.equal(_bits(H), _bits(H.T.contiguous()))
    torch.cuda.synchronize()
    assert _guards_intact(H, buf, -3.25), "H: a guard word was overwritten"
    # an H that is not symmetric gets x^T x added on both sides all the same
    skew = torch.arange(C * C, dtype=torch.float32).view(C, C) % 7
    Hs = skew.to(DEV)
    fused.gram_accumulate_onepass_(Hs, x1.to(DEV))
    assert torch.equal(Hs.cpu().double(), skew.double() + x1.double().T @ x1.double())


def test_gram_onepass_on_random_operands_is_within_the_fp32_bound_and_deterministic():
    """Bound.  The products of two bf16 (fp16) numbers are exact in fp32; an element is a sum of `rows` of them in some order of
    fp32 additions (inside the matrix core and across its calls), each with a relative error of at most 2^-23 (rounding to
    nearest gives 2^-24; the factor 2 covers an adder that chops).  To first order |sum - exact| <= (rows - 1) 2^-23 sum |product|;
    rows * 2^-23 * (|x|^T |x|) is asserted.  (tests/test_gpu_gptq.py has no bound for this: its Gram tests are exact, as the
    integer test above is; this one is derived.)"""
    from viditq_extension import fused

    rows, C = 300, 264
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.bfloat16, torch.float16):
        big = torch.randn(rows + 5, C, generator=g).to(dtype).to(DEV)
        x = big[:rows].clone()
        H = torch.zeros(C, C, device=DEV)
        fused.gram_accumulate_onepass_(H, x)
        xd = x.cpu().double()
        err = (H.cpu().double() - xd.T @ xd).abs()
        bound = rows * 2.0 ** -23 * (xd.abs().T @ xd.abs())
        print(f"{dtype}: worst error / bound {(err / bound).max().item():.4f}")
        assert (err <= bound).all()
        assert torch.equal(_bits(H), _bits(H.T.contiguous()))
        again = torch.zeros(C, C, device=DEV)
        fused.gram_accumulate_onepass_(again, x)
        assert torch.equal(_bits(again), _bits(H))                    # across calls
        shifted = big.clone()
        shifted[3:3 + rows] = x                                       # the same rows from another base pointer (3 rows = 1584 bytes on)
        view = shifted[3:3 + rows]
        assert view.data_ptr() != x.data_ptr() and (view.data_ptr() - shifted.data_ptr()) % 128 != 0
        moved = torch.zeros(C, C, device=DEV)
        fused.gram_accumulate_onepass_(moved, view)
        assert torch.equal(_bits(moved), _bits(H))
        # the two-sided form sums in another order: the two agree within twice the bound
        old = torch.zeros(C, C, device=DEV)
        fused.gram_accumulate_(old, x)
        assert ((old.cpu().double() - H.cpu().double()).abs() <= 2 * bound).all()


def test_gram_onepass_rounds_fp32_to_bf16_and_checks_its_operands():
    from viditq_extension import fused

    x = torch.full((4, 32), 1.0 + 2.0 ** -10)  # not a bf16 number: rounds to 1
    H = torch.zeros(32, 32, device=DEV)
    fused.gram_accumulate_onepass_(H, x.to(DEV))
    assert torch.equal(H.cpu(), torch.full((32, 32), 4.0))
    fused.gram_accumulate_onepass_(H, torch.zeros(0, 32, device=DEV, dtype=torch.bfloat16))  # no rows: untouched
    assert torch.equal(H.cpu(), torch.full((32, 32), 4.0))
    with pytest.raises(RuntimeError, match="must have shape"):
        fused.gram_accumulate_onepass_(torch.zeros(32, 64, device=DEV), x.to(DEV))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        fused.gram_accumulate_onepass_(torch.zeros(12, 12, device=DEV), torch.zeros(4, 12, device=DEV))


# ---- d. the objective -------------------------------------------------------------------------------------------------------------
def test_act_order_does_not_raise_the_layer_objective_on_spread_channel_energies():
    """W4 g128 on a reduced ffn shape, N = 64, K = 512; inputs with a lognormal channel scale (sigma = 1, seed 0: diag H spreads
    over 4.6 decades).  Chosen on the CPU with the host model: act_order / plain GPTQ = 0.5595 there."""
    from qdiff.base import gptq

    N, K = 64, 512
    g = torch.Generator().manual_seed(0)
    w = _xavier(N, K, g)
    H = _spread_hessian(K, 4 * K, g)
    d = torch.diagonal(H)
    assert torch.log10(d.max() / d.min()) >= 2.0
    wd, Hd = w.to(DEV), H.float().to(DEV)
    q = _quantizer(128, wd)
    U, w0 = gptq.gptq_prepare(Hd, wd, 0.01)
    _, plain = gptq.gptq_solve(w0, U, q, 128)
    U, wp, perm = gptq.gptq_prepare(Hd, wd, 0.01, act_order=True)
    _, ao = gptq.gptq_solve(wp, U, q, 128, act_order=True, perm=perm)
    o_a, o_p, o_r = (gptq.objective(w, t.cpu(), H).sum().item() for t in (ao, plain, q(wd)))
    print(f"N={N} K={K} g=128: objective act_order / plain GPTQ {o_a / o_p:.4f}, plain / RTN {o_p / o_r:.4f}, act_order / RTN {o_a / o_r:.4f}")
    assert o_a <= o_p * (1 + 1e-6)
