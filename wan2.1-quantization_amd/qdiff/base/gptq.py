"""GPTQ (Frantar et al., 2022) for the integer weight quantisers: the grid stays, the choice of the codes changes.

Round-to-nearest minimises ||W - W_hat||; GPTQ minimises the layer's output error on the calibration inputs,
sum_n (w_n - w_hat_n) H (w_n - w_hat_n)^T with H = X^T X, by quantising the input channels in order and pushing every column's error,
through the upper Cholesky factor U of H^-1, onto the columns that are still free.  Scales and zero points are fixed beforehand from
the ORIGINAL weight by StaticQuantizer.init_quant_params (GPTQ's "static groups"): they are bit-equal to the round-to-nearest
checkpoint's, and so are the checkpoint layout and every GEMM that reads it.

  gptq_prepare(H, w, damp)            float64: dead channels, damping, U = cholesky(H^-1, upper) -> (U fp32, w with dead columns zeroed)
  gptq_solve(w, U, quantizer, block)  (codes int8, dequantised weight fp32): wanq_gptq_block / wanq_gptq_propagate on the GPU, and
                                      gptq_solve_host for a weight in host memory
  gptq_solve_host(...)                the same loop in torch on the CPU: the model the kernels are bit-equal to

act_order (`gptq.act_order: True`) is defined here, once: gptq_prepare sorts the input channels by descending diag H (after the
dead-channel rule, before damping; a stable sort, so a tie goes to the lower channel) and returns the permuted problem together with
`perm`; the solve visits the columns in that order with the per-column group map g_idx[j] = perm[j] // group_size on the SAME delta /
zero_point (derived from the unpermuted original weight, so a group stays a contiguous run of original channels), on
wanq_gptq_block_gidx; codes and dequantised weight go back as codes[:, perm] = codes_p.  Nothing downstream sees the order.

The arithmetic of the loop is defined once, for both: fp32, every operation rounded on its own (no fma), true divisions, and the
propagation summed over the block's columns in ascending order.  The host model therefore spells every step as one torch
operation.  Not implemented: activation-aware scaling, the transformed (SmoothQuant / QuaRot / ViDiT) layer classes and
the fp8 / MX formats."""
import re

import torch

from viditq_extension import fused

BLOCK_MAX = 128  # columns of one wanq_gptq_block launch


def gptq_section(quant_config, full_name):
    """The config's `gptq:` section when its layer_name_regex matches `full_name`, else None."""
    sec = quant_config.get("gptq", None) if quant_config is not None else None
    if sec is None or not re.search(re.compile(sec.get("layer_name_regex", "")), full_name or ""):
        return None
    return sec


def stored_range(quantizer):
    """(qmin, qmax) of the codes a checkpoint keeps: the quantiser's clamp [-n-1, n] intersected with the bit-width's range (the
    reference's clamp is one level looser than the storage)."""
    n, b = quantizer.n_levels, quantizer.n_bits
    return max(-n - 1, -(2 ** (b - 1))), min(n, 2 ** (b - 1) - 1)


def gptq_prepare(H, w, damp=0.01, act_order=False):
    """-> (U fp32 [K, K], w fp32 [N, K]), and with `act_order` -> (U, w, perm): the problem with its input channels in the order
    perm = stable descending sort of diag H (int64 [K]; taken in float64 after the dead-channel rule -- damping adds a constant and
    does not change it), H <- H[perm][:, perm] and w <- w[:, perm] before damping and factorisation.  In float64, on the weight's device where this build has the factorisation there and
    otherwise on the host (the rule of low_rank.fit_low_rank: only NotImplementedError falls back, every other error is raised):
      dead input channels, H[i,i] == 0: H[i,i] = 1 and w[:, i] = 0 (the channel never fires: its weight is free, zero costs nothing);
      damping: H += damp * mean(diag H) * I;
      U = cholesky(H^-1, upper), so that H^-1 = U^T U."""
    if H.dim() != 2 or H.shape[0] != H.shape[1] or H.shape[0] != w.shape[1]:
        raise ValueError(f"gptq_prepare: H is {tuple(H.shape)}, the weight {tuple(w.shape)}: H must be [K, K]")
    w = w.detach().float().clone()
    H = H.detach().to(device=w.device, dtype=torch.float64).clone()
    diag = torch.diagonal(H)
    dead = diag == 0
    diag[dead] = 1.0
    w[:, dead] = 0.0
    perm = None
    if act_order:
        perm = torch.sort(diag, descending=True, stable=True).indices
        H, w = H[perm][:, perm].contiguous(), w[:, perm].contiguous()
        diag = torch.diagonal(H)
    diag += damp * diag.mean()

    def factor(h):
        return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(h)), upper=True)

    try:
        U = factor(H)
    except NotImplementedError:  # no float64 factorisation for this device in this build
        U = factor(H.cpu()).to(w.device)
    return (U.float().contiguous(), w, perm) if act_order else (U.float().contiguous(), w)


def _group_index(K, group_size, device):
    return torch.arange(K, device=device) // group_size if group_size else torch.zeros(K, dtype=torch.long, device=device)


def gptq_block_host(w, u, delta, zp, group_size, qmin, qmax, codes, c0, cols, g_idx=None):
    """wanq_gptq_block in torch, in place on w / codes: -> err fp32 [N, cols].  delta / zp: fp32 [N, K / group_size] (or [N, 1]).
    With `g_idx` (integer [K], values in 0 .. G-1) it is wanq_gptq_block_gidx: the map names every column's group and `group_size`
    is not looked at."""
    N, K = w.shape
    gi = _group_index(K, group_size, w.device) if g_idx is None else g_idx.to(device=w.device, dtype=torch.long)
    err = torch.empty(N, cols, dtype=torch.float32, device=w.device)
    for j in range(c0, c0 + cols):
        d, z, x = delta[:, gi[j]], zp[:, gi[j]], w[:, j].clone()
        q = torch.clamp(torch.round(x / d) - z, qmin, qmax)
        w_hat = (q + z) * d
        e = (x - w_hat) / u[j, j]
        codes[:, j] = q.to(torch.int8)
        err[:, j - c0] = e
        if j + 1 < c0 + cols:
            prod = e[:, None] * u[j, j + 1:c0 + cols][None, :]  # the product rounded, then the difference: two operations
            w[:, j + 1:c0 + cols] = w[:, j + 1:c0 + cols] - prod
        w[:, j] = w_hat
    return err


def gptq_propagate_host(w, u, err, c0, cols):
    """wanq_gptq_propagate in torch, in place on w: the sum over the block's columns ascending, product and sum rounded apart."""
    k0 = c0 + cols
    if k0 >= w.shape[1]:
        return
    acc = torch.zeros(w.shape[0], w.shape[1] - k0, dtype=torch.float32, device=w.device)
    for i in range(cols):
        prod = err[:, i:i + 1] * u[c0 + i, k0:][None, :]
        acc = acc + prod
    w[:, k0:] = w[:, k0:] - acc


def _check_block(block):
    if isinstance(block, bool) or not isinstance(block, int) or not 1 <= block <= BLOCK_MAX:
        raise ValueError(f"gptq: block={block!r} must be an integer in 1..{BLOCK_MAX}")


def _check_perm(act_order, perm, K):
    if bool(act_order) != (perm is not None):
        raise ValueError("gptq: act_order=True needs perm, the channel order gptq_prepare(..., act_order=True) returned with w and U "
                         "(and perm is given with act_order=True only)")
    if perm is not None and (perm.dim() != 1 or perm.numel() != K or perm.dtype != torch.int64):
        raise ValueError(f"gptq: perm must be int64 [{K}], got {tuple(perm.shape)} {perm.dtype}")


def solve_with_params(w, U, delta, zp, group_size, qmin, qmax, block=BLOCK_MAX, host=False, keep_err=False, act_order=False, perm=None):
    """The block / propagate loop over all columns on a given grid: -> (codes int8 [N, K], w_hat fp32 [N, K], errs).  `w` is not
    modified.  On the GPU the two kernels; `host=True` or a weight in host memory: the torch model, on the CPU.  `errs`: the
    blocks' scaled errors (a list of [N, cols]) when `keep_err`, else None.
    `act_order`: w and U are the permuted problem of gptq_prepare(..., act_order=True) and `perm` its channel order; delta / zp stay
    those of the unpermuted weight.  The loop runs on the column map g_idx[j] = perm[j] // group_size (wanq_gptq_block_gidx; any
    `block`, any group size) and codes / w_hat are returned in the ORIGINAL channel order; `errs` stay in solve order."""
    _check_block(block)
    _check_perm(act_order, perm, w.shape[1])
    N, K = w.shape
    dev = w.device
    on_host = host or not w.is_cuda
    work = torch.device("cpu") if on_host else dev
    w = w.detach().to(device=work, dtype=torch.float32).clone()
    U = U.to(device=work, dtype=torch.float32).contiguous()
    G = K // group_size if group_size else 1
    delta = delta.to(device=work, dtype=torch.float32).reshape(N, G).contiguous()
    zp = zp.to(device=work, dtype=torch.float32).reshape(N, G).contiguous()
    codes = torch.empty(N, K, dtype=torch.int8, device=work)
    g_idx = None
    if act_order:
        perm = perm.to(work)
        g_idx = (perm // group_size if group_size else torch.zeros_like(perm)).to(torch.int32)
    errs = []
    for c0 in range(0, K, block):
        cols = min(block, K - c0)
        if on_host:
            err = gptq_block_host(w, U, delta, zp, group_size, qmin, qmax, codes, c0, cols, g_idx)
            gptq_propagate_host(w, U, err, c0, cols)
        else:
            err = torch.empty(N, cols, dtype=torch.float32, device=work)
            if act_order:
                fused.gptq_block_gidx_(w, U, delta, zp, g_idx, qmin, qmax, codes, err, c0, cols)
            else:
                fused.gptq_block_(w, U, delta, zp, group_size, qmin, qmax, codes, err, c0, cols)
            fused.gptq_propagate_(w, U, err, c0, cols)
        if keep_err:
            errs.append(err)
    if act_order:  # back to the original channel order
        codes_p, w_p = codes, w
        codes, w = torch.empty_like(codes_p), torch.empty_like(w_p)
        codes[:, perm], w[:, perm] = codes_p, w_p
    return codes.to(dev), w.to(dev), (errs if keep_err else None)


def _solve(w, U, quantizer, block, host, act_order, perm):
    _check_perm(act_order, perm, w.shape[1])
    if getattr(quantizer, "delta", None) is None or quantizer.init_done is not True:
        w_orig = w.detach().float()
        if act_order:  # the grid belongs to the weight in its original channel order
            w_orig = torch.empty_like(w_orig)
            w_orig[:, perm.to(w.device)] = w.detach().float()
        quantizer.init_quant_params(w_orig)
    qmin, qmax = stored_range(quantizer)
    codes, w_hat, _ = solve_with_params(w, U, quantizer.delta, quantizer.zero_point, getattr(quantizer, "group_size", None), qmin, qmax,
                                        block, host=host, act_order=act_order, perm=perm)
    return codes, w_hat


def gptq_solve(w, U, quantizer, block=BLOCK_MAX, act_order=False, perm=None):
    """(codes int8 [N, K], dequantised weight fp32 [N, K]) of GPTQ on the grid of `quantizer` (a StaticQuantizer).  Its delta /
    zero_point are used as they are when the quantiser is initialised (the layer derived them from the original weight), and
    derived from `w` by init_quant_params otherwise.  The dequantised weight is exactly (codes + zero_point) * delta.
    `act_order=True, perm=...`: (U, w, perm) come from gptq_prepare(..., act_order=True); the results are in the original channel
    order, so the sentence above holds on the unpermuted layout."""
    return _solve(w, U, quantizer, block, False, act_order, perm)


def gptq_solve_host(w, U, quantizer, block=BLOCK_MAX, act_order=False, perm=None):
    """gptq_solve by the torch model on the CPU, whatever device `w` is on (results are returned on that device)."""
    return _solve(w, U, quantizer, block, True, act_order, perm)


def objective(w, w_hat, H):
    """Per-row layer objective (w_n - w_hat_n) H (w_n - w_hat_n)^T in float64: fp64 [N]."""
    d = w.double() - w_hat.double()
    return ((d @ H.to(d.device).double()) * d).sum(dim=1)


def load_hessians(path):
    """The file get_calib_data_wanx.py --hessian wrote, {layer name: fp32 [C, C]}, memory mapped (it runs to gigabytes)."""
    return torch.load(path, map_location="cpu", weights_only=True, mmap=True)


def requantize_model_(model, quant_config, hessians, path):
    """ptq_wanx.py: GPTQ on every QuantizedLinear the `gptq:` section names, with its Hessian from `hessians` (the file at `path`).
    -> the number of layers solved.  A layer without a Hessian in the file is a KeyError that names both."""
    from .quant_layer import QuantizedLinear

    done = 0
    for name, mod in model.named_modules():
        if isinstance(mod, QuantizedLinear) and mod.gptq is not None and mod.w_quantizer is not None and mod.quant_mode:
            if name not in hessians:
                raise KeyError(f"{name}: no Hessian for this layer in {path} (collect it with get_calib_data_wanx.py --hessian and the "
                               "same gptq.layer_name_regex)")
            mod.requantize_gptq_(hessians[name])
            done += 1
    return done


def load_codes_(model, state_dict, path):
    """Simulation mode of a GPTQ checkpoint: a QuantizedLinear re-derives its codes from the FP weight by round-to-nearest, so the
    layers the `gptq:` section names take theirs from the integer checkpoint instead (`<name>.weight` of int_weight.pt)."""
    from .quant_layer import QuantizedLinear

    done = 0
    for name, mod in model.named_modules():
        if isinstance(mod, QuantizedLinear) and mod.gptq is not None and mod.w_quantizer is not None and mod.quant_mode:
            if name + ".weight" not in state_dict:
                raise KeyError(f"{name}: no integer codes for this layer in {path}")
            mod.set_codes_(state_dict[name + ".weight"])
            done += 1
    return done
