"""The clip search on the GPU (csrc/clip_search.hip, StaticQuantizer.search_clip, `weight.clip`) against a float64 restatement.
The reference's inputs are the fp32 candidate grid (base_quantizer.clip_params / clip_ratios) and the integer codes on it, which are
wanq_weight_quant's fp32 expression (a float64 quotient would pick the other code at a near-tie and flip the error's sign); error,
products and sums are float64.  Bound (profiles/PARITY_NOTES.md, "Clip search"): |objective - float64| <= gamma B with B = sum_ij
|e_i| |H_ij| |e_j|, gamma = (n_lane + 16) 2^-24 elementwise (n_lane = 8 ceil(cols / 8 / lanes), lanes 64 up to 2048 columns, else
256) and (1.5 g + 8) 2^-24 for the block kernel; the chosen s then has f64(s) <= min f64 + gamma (B(s) + B(argmin)).
Weights: Gaussian, 6 sigma outliers at two columns of every other quantiser row.  Rows with s > 0 AND rows with s = 0 in the float64
optimum of every case cannot be had: at 8 bits clipping the largest weight A by 5 % costs (0.05 A)^2 and saves a tenth of the noise
n (A / 255)^2 / 12, which pays from n > 20000 columns only, and at 4 bits a row of 384 Gaussians always gains.  So a case asserts the
kind its width can have (4 bits: some s > 0; 8 bits: some s = 0; the rows of 8960 gain at either width and assert none)."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, S = 20, 10
U = 2.0 ** -24


def _weight(N, K, n, seed):
    """fp32 [N, K], quantiser rows of n columns: standard normal, +6 / -6 at columns 3 / n - 5 of every other quantiser row"""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(seed))
    rows = w.view(-1, n)
    rows[0::2, 3], rows[0::2, n - 5] = 6.0, -6.0
    return w


def _hessian(K, seed):
    """H = X^T X of 256 correlated Gaussian tokens whose channel scales fall from 1 to 1/8 along every 128 channels: float64 -> fp32"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(256, K, generator=g, dtype=torch.float64)
    x = x @ (torch.eye(K, dtype=torch.float64) + torch.randn(K, K, generator=g, dtype=torch.float64) / K ** 0.5)
    x = x * (2.0 ** (-3 * (torch.arange(K) % 128) / 127.0)).double()
    return (x.T @ x).float()


def _reference(w, n, n_bits, sym, h=None, Hb=None):
    """-> (delta, zp fp32 [R, S]; objective, B float64 [R, S]).  h [K] float64: sum_j h_j e_j^2; Hb [K / n, n, n]: e H_gg e^T"""
    from qdiff.base import base_quantizer as bq

    rows = w.view(-1, n)
    lo, hi = rows.amin(1, keepdim=True), rows.amax(1, keepdim=True)
    delta, zp = bq.clip_params(lo, hi, bq.clip_ratios(STEPS, S)[None, :], n_bits, sym)
    d3, z3 = delta[:, :, None], zp[:, :, None]
    q = torch.clamp(torch.round(rows[:, None, :] / d3) - z3, -(2 ** (n_bits - 1)), 2 ** (n_bits - 1) - 1)
    e = rows.double()[:, None, :] - (q.double() + z3.double()) * d3.double()
    if Hb is not None:
        Hr = Hb.double()[torch.arange(rows.shape[0]) % Hb.shape[0]]  # row r of w.view(-1, n) lies in group r % (K / n)
        return delta, zp, torch.einsum("rsi,rij,rsj->rs", e, Hr, e), torch.einsum("rsi,rij,rsj->rs", e.abs(), Hr.abs(), e.abs())
    hr = torch.ones(n, dtype=torch.float64) if h is None else h.double().view(-1, n)[torch.arange(rows.shape[0]) % (h.numel() // n)][:, None, :]
    obj = (e * e * hr).sum(-1)
    return delta, zp, obj, obj


def _check(out, ref, gamma, n_bits, kinds=True):
    (d, z, sel, table), (delta, zp, obj, B) = (tuple(t.cpu() for t in out), ref)
    best = obj.argmin(1)
    assert not kinds or ((best > 0).any() if n_bits == 4 else (best == 0).any())
    pick = sel.long()[:, None]
    assert torch.equal(d.view(torch.int32), delta.gather(1, pick)[:, 0].view(torch.int32))          # 1. the grid, to the bit
    assert torch.equal(z.view(torch.int32), zp.gather(1, pick)[:, 0].view(torch.int32))
    err = (table.double() - obj).abs()
    print(f"table: worst |err| / (gamma B) {(err / (gamma * B).clamp_min(1e-300)).max().item():.3f}; rows with s > 0: {(sel > 0).sum().item()} of {sel.numel()}"
          f" (float64: {(best > 0).sum().item()}); choices differing from the float64 argmin: {(sel.long() != best).sum().item()}")
    assert (err <= gamma * B).all()                                                                   # 2. the table
    assert (obj.gather(1, pick)[:, 0] <= obj.min(1).values + gamma * (B.gather(1, pick)[:, 0] + B.gather(1, best[:, None])[:, 0])).all()  # 3.


CASES = [(m, N, K, g) for N in (8, 72) for K in (128, 384) for m, gs in (("mse", (128, None)), ("diag", (128, None)), ("hessian", (32, 64, 128)))
         for g in gs] + [("mse", 3, 8960, None), ("diag", 3, 8960, None)]  # (8960: the four-wave rung of the row frame)


@pytest.mark.parametrize("n_bits,sym", [(4, False), (4, True), (8, False), (8, True)], ids=["W4", "W4 sym", "W8", "W8 sym"])
@pytest.mark.parametrize("mode,N,K,g", CASES, ids=[f"{m} N{n} K{k} g{g}" for m, n, k, g in CASES])
def test_search_against_float64(mode, N, K, g, n_bits, sym):
    from viditq_extension import fused

    n, rng = g or K, (n_bits, sym, -(2 ** (n_bits - 1)), 2 ** (n_bits - 1) - 1, STEPS, S)
    w, H = _weight(N, K, n, seed=N + K + n), _hessian(K, 7)
    if mode == "hessian":
        Hb = torch.stack([H[k:k + g, k:k + g] for k in range(0, K, g)]).contiguous()
        out = fused.clip_search_blocks(w.to(DEV), Hb.to(DEV), *rng, want_table=True)
        return _check(out, _reference(w, g, n_bits, sym, Hb=Hb), (1.5 * g + 8) * U, n_bits)
    h = None if mode == "mse" else torch.diagonal(H).contiguous()
    out = fused.clip_search(w.view(-1, n).to(DEV), *rng, chan_w=None if h is None else h.to(DEV), want_table=True)
    gamma = (8 * -(-(n // 8) // (64 if n <= 2048 else 256)) + 16) * U
    _check(out, _reference(w, n, n_bits, sym, h), gamma, n_bits, kinds=K < 8960)


# ---- the layer ------------------------------------------------------------------------------------------------------------------
def _layer(weight_cfg, N, K, extra=None):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(_weight(N, K, 128, seed=3) * K ** -0.5)
    return QuantizedLinear(K, N, True, DEV, qcfg.create({"weight": weight_cfg, **(extra or {})}), fp, module_name="lin"), fp


def _deq(ql):
    """(codes + zp) delta of the layer's STORED codes, fp32 [N, K]"""
    wq, N = ql.w_quantizer, ql.out_features
    return ((ql.int_weight.float().view(N, wq.delta.numel() // N, -1) + wq.zero_point.view(N, -1, 1)) * wq.delta.view(N, -1, 1)).view(N, -1)


def _metric(fp, ql, mode, H):
    """the searched metric of the stored codes per weight row, float64 [N], and its B (the plain layer's weight.data keeps the
    reference's 17th level where lo = -hi, which no 4-bit checkpoint holds)"""
    e = (fp.weight.data.double() - _deq(ql).double()).cpu()
    if mode != "hessian":
        m = (e * e * (1.0 if mode == "mse" else torch.diagonal(H).double())).sum(1)
        return m, m
    eb = e.view(e.shape[0], -1, ql.group_size)
    Hb = torch.stack([H[k:k + ql.group_size, k:k + ql.group_size] for k in range(0, e.shape[1], ql.group_size)]).double()
    return torch.einsum("ngi,gij,ngj->n", eb, Hb, eb), torch.einsum("ngi,gij,ngj->n", eb.abs(), Hb.abs(), eb.abs())


@pytest.mark.parametrize("mode,g", [("mse", 128), ("mse", None), ("diag", None), ("hessian", 128), ("hessian", 32)])
def test_a_clip_layer_lies_on_its_grid_and_lowers_the_searched_metric(mode, g):
    N, K = 72, 384
    wc = {"n_bits": 4, "sym": False, **({"group_size": g} if g else {})}
    H = _hessian(K, 5)
    plain, fp = _layer(wc, N, K)
    ql, _ = _layer(dict(wc, clip={"search": mode}), N, K, {"gptq": {"layer_name_regex": ""}} if mode != "mse" else None)
    if mode != "mse":  # s = 0 until PTQ: the un-clipped grid and codes
        assert torch.equal(ql.w_quantizer.delta, plain.w_quantizer.delta) and torch.equal(ql.int_weight, plain.int_weight)
        assert ql.requantize_clip_(H) is ql
    assert torch.equal(ql.weight.data, _deq(ql)) and not torch.equal(ql.w_quantizer.delta, plain.w_quantizer.delta)
    (m_c, B_c), (m_p, B_p) = _metric(fp, ql, mode, H), _metric(fp, plain, mode, H)
    print(f"{mode} g={g}: metric clipped / un-clipped {(m_c.sum() / m_p.sum()).item():.4f}")
    # per quantiser row the kernel's objective of its choice is <= its objective of s = 0, each within gamma B of float64
    assert (m_c <= m_p + (1.5 * 128 + 8) * U * (B_c + B_p)).all() and m_c.sum() < m_p.sum()
    if mode != "mse":  # GPTQ solves on the clipped grid and leaves it alone
        delta = ql.w_quantizer.delta.clone()
        ql.requantize_gptq_(H)
        assert torch.equal(ql.w_quantizer.delta, delta) and torch.equal(ql.weight.data, _deq(ql))


def test_quant_param_file_round_trip_into_a_kernel_mode_layer(tmp_path):
    """the fitted delta / zero_point through the quant-parameter file into a fresh layer and kernel mode's weight-only g128 GEMM: the
    output equals float64 x W_hat^T + bias at the tolerance of tests/test_gpu_wq16_grouped.py for that GEMM and a bf16 output"""
    from qdiff.base.quant_model import load_quant_param_dict_, save_quant_param_dict_
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import HipLinearWq16

    N, K, g = 72, 384, 128
    wc = {"n_bits": 4, "sym": False, "group_size": g, "clip": {"search": "hessian"}}
    ql, _ = _layer(wc, N, K)
    ql.requantize_clip_(_hessian(K, 5))
    model = types.SimpleNamespace(quant_param_dict={})
    save_quant_param_dict_(ql.w_quantizer, "lin.w_quantizer", ql, model)
    path = os.path.join(tmp_path, "quant_params.pth")
    torch.save({k: {kk: (vv.cpu() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in model.quant_param_dict.items()}, path)
    fresh, _ = _layer(wc, N, K)
    assert not torch.equal(fresh.w_quantizer.delta, ql.w_quantizer.delta)
    load_quant_param_dict_(fresh.w_quantizer, "lin.w_quantizer", fresh, torch.load(path, weights_only=True), model)
    assert torch.equal(fresh.w_quantizer.delta, ql.w_quantizer.delta) and torch.equal(fresh.weight.data, ql.weight.data)
    x = torch.randn(33, K, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    out = HipLinearWq16.from_quantized(fresh)(x)
    codes, sw, zp, _ = fresh.weight_only_operands()
    wint = qgemm.unpack_w4(codes, bias=0).double() + zp.double().T.repeat_interleave(g, dim=1)
    Sabs = sum((x.double()[:, k:k + g].abs() @ wint[:, k:k + g].abs().T) * sw[k // g].double().abs() for k in range(0, K, g))
    y = x.double() @ fresh.weight.data.double().T + fresh.bias.double()
    tol = Sabs * (2.0 ** -14 + (K // g + 1) * 2.0 ** -24) + 2.0 ** -23 * y.abs() + y.abs() * 2.0 ** -7
    assert out.dtype == torch.bfloat16 and not ((out.double() - y).abs() > tol).any()
