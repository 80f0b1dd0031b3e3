"""The 16-bit low-rank side branch of a weight-only quantised Linear, y = x W_hat^T + (x A^T) B^T, shared by the simulation-mode layer
(QuantizedLinear) and the kernel-mode one (HipLinearWq16).  Two uses, one operator (wanq_gemm_wq16_lowrank):

  * LoRC, the low-rank compensation of the quantisation error (ZeroQuant-V2, L2QER): with E = W - W_hat, B A is the best rank-r
    approximation of E (Eckart-Young), kept in 16 bits beside the integer codes.  The config key `weight.low_rank: r`.
  * a LoRA adapter on a quantised Linear: `set_low_rank(a, b, scale)`, concatenated behind the LoRC factors along r.

The GEMM takes ranks that are multiples of 64 up to 256, so factors are zero padded along r; a zero column contributes exactly 0.
On this repository's synthetic xavier weights E has a flat spectrum -- rank 32 of a 1536 x 1536 W4-g128 layer removes about 4 % of
||E||_F -- and the gain is unmeasured on a trained checkpoint."""
import torch

RANK_TILE, RANK_MAX = 64, 256


def padded_rank(r):
    return (r + RANK_TILE - 1) // RANK_TILE * RANK_TILE


def fit_low_rank(err, r):
    """The best rank-r approximation B A of `err` [N, K] split evenly, B = U_r sqrt(S_r) [N, r] and A = sqrt(S_r) V_r^T [r, K], from a
    full float64 SVD; -> (A [Rp, K], B [N, Rp]) fp32 on err's device, zero padded to Rp = padded_rank(r).  Deterministic: the same
    `err` on the same device gives the same bits.  The SVD runs on err's device; only if torch.linalg.svd raises NotImplementedError
    there (a build without a float64 SVD for that device) it runs on the host and the factors are moved back -- every other error,
    a device fault included, is raised.  This project's torch-ROCm build has the device form: on an MI355X a fit takes 0.6 s at
    1536 x 1536, 8960 x 1536 and 1536 x 8960 alike (the host takes 0.5 / 0.7 / 2.4 s), about three minutes for the 300 Linears of the
    1.3B model."""
    e64 = err.detach().double()
    try:
        U, S, Vh = torch.linalg.svd(e64, full_matrices=False)
    except NotImplementedError:  # no float64 SVD for this device in this build; any other error, a device fault included, is raised
        U, S, Vh = (t.to(e64.device) for t in torch.linalg.svd(e64.cpu(), full_matrices=False))
    s = S[:r].sqrt()
    N, K = err.shape
    a = torch.zeros(padded_rank(r), K, dtype=torch.float32, device=err.device)
    b = torch.zeros(N, padded_rank(r), dtype=torch.float32, device=err.device)
    a[:r] = (s[:, None] * Vh[:r]).float()
    b[:, :r] = (U[:, :r] * s).float()
    return a, b


class LowRankBranch:
    """Mixin of a Linear with `in_features`, `out_features`, the optional buffers `lr_a` [Rp, K] / `lr_b` [N, Rp] (the LoRC factors,
    zero padded behind rank `low_rank`; None without the config key) and a user adapter.  `low_rank_operands(dtype)` hands the GEMM
    the factors it multiplies: LoRC's first `low_rank` ranks, the adapter behind them, zero padded to a multiple of 64 and cast once
    to the activation dtype; None when the layer has neither."""
    low_rank = None
    _adapter = None
    _lr16 = None

    def _lr_name(self):
        return getattr(self, "module_name", None) or getattr(self, "name", None) or type(self).__name__

    def _refuse_adapter(self):
        """(a subclass names what cannot carry an adapter)"""

    def set_low_rank(self, a, b=None, scale=1.0):
        """Attach a user adapter, y += scale * (x a^T) b^T with a [r, K] and b [N, r] (`scale` is folded into b), behind the layer's
        LoRC factors along r; `set_low_rank(None)` removes it.  A total padded rank above 256 is refused by layer name."""
        if a is None:
            self._adapter = self._lr16 = None
            return self
        self._refuse_adapter()
        name = self._lr_name()
        if b is None or a.dim() != 2 or b.dim() != 2 or a.shape[1] != self.in_features or b.shape[0] != self.out_features \
                or a.shape[0] != b.shape[1] or a.shape[0] < 1:
            raise ValueError(f"{name}: set_low_rank takes a [r, {self.in_features}] and b [{self.out_features}, r], got "
                             f"{None if a is None else tuple(a.shape)} and {None if b is None else tuple(b.shape)}")
        total = (self.low_rank or 0) + a.shape[0]
        if padded_rank(total) > RANK_MAX:
            raise ValueError(f"{name}: set_low_rank: the adapter's rank {a.shape[0]}"
                             + (f" behind weight.low_rank={self.low_rank}" if self.low_rank else "")
                             + f" makes a padded rank of {padded_rank(total)}, above the GEMM's {RANK_MAX}")
        self._adapter = (a.detach().float().contiguous(), (b.detach().float() * float(scale)).contiguous())
        self._lr16 = None
        return self

    def low_rank_operands(self, dtype, device=None):
        if self.low_rank is None and self._adapter is None:
            return None
        device = device if device is not None else (self.lr_a.device if self.low_rank is not None else self._adapter[0].device)
        if self._adapter is None and self.lr_a.dtype == dtype and self.lr_a.device == device:
            return self.lr_a, self.lr_b  # the buffers as they are (kernel mode without an adapter): no second copy, nothing to go stale
        # the cache is made for one state of the buffers: an in-place write or a load into lr_a / lr_b makes it again
        state = None if self.low_rank is None else (self.lr_a._version, self.lr_b._version, self.lr_a.data_ptr(), self.lr_b.data_ptr())
        if self._lr16 is None or self._lr16[0].dtype != dtype or self._lr16[0].device != device or self._lr16[2] != state:
            r0 = self.low_rank or 0
            parts_a, parts_b = [], []
            if r0:
                parts_a.append(self.lr_a[:r0].to(device=device, dtype=dtype))
                parts_b.append(self.lr_b[:, :r0].to(device=device, dtype=dtype))
            if self._adapter is not None:
                parts_a.append(self._adapter[0].to(device=device, dtype=dtype))
                parts_b.append(self._adapter[1].to(device=device, dtype=dtype))
            r = sum(p.shape[0] for p in parts_a)
            a16 = torch.zeros(padded_rank(r), self.in_features, dtype=dtype, device=device)
            b16 = torch.zeros(self.out_features, padded_rank(r), dtype=dtype, device=device)
            a16[:r] = torch.cat(parts_a, 0)
            b16[:, :r] = torch.cat(parts_b, 1)
            self._lr16 = (a16, b16, state)
        return self._lr16[:2]
