"""Quant-config loading without omegaconf (absent from the image): attribute-style dicts + a list type that is not a
`list`, i.e. exactly what the reference's code relies on (`cfg.weight.n_bits`, `cfg.get('viditq')`,
`isinstance(n_bits, ListConfig)`).  Schema: ViDiT-Q/examples/Wan2.1/quant_configs/config.yaml, plus one key of
this repository: `weight.group_size: <int>` -- one (delta, zero_point) per output channel and per group of that many input
channels, with or without an `act:` section (no bit-width list, no transform section; it must divide in_features; with an `act:`
section the layer's weight must be on the GPU; QuantizedLinear refuses everything else by layer name when it is built), and
`format: fp8_e4m3` in BOTH the `weight:` and the `act:` section -- OCP e4m3fn codes with one fp32 scale per output channel and per
token (absmax / 448) instead of int8 codes, on wanq_gemm_fp8; `n_bits: 8, sym: True` stay as written.  Refused by layer name when
the layer is built: the key in only one section, with `group_size`, with `sym: False`, with `n_bits` other than 8 or a bit-width
list, and on a SmoothQuant / QuaRot / ViDiT layer.
The OCP Microscaling formats use the same key: `format: mxfp8_e4m3` (`n_bits: 8`) and `format: mxfp4_e2m1` (`n_bits: 4`) in `act:` and
in `weight:` -- one E8M0 power-of-two scale per block of 32 input channels on both sides, applied by the matrix cores
(wanq_quant_rows_mx, wanq_gemm_mx, wanq_gemm_mx4).  The accepted pairs are weight mxfp8_e4m3 or mxfp4_e2m1 against act mxfp8_e4m3, and
the W4A4 pair weight mxfp4_e2m1 against act mxfp4_e2m1, `sym: True`, `weight.group_size` absent or 32; `act.format: mxfp4_e2m1` with
`n_bits: 8` or against an e4m3 weight, an MX format against `fp8_e4m3` or against no format, a bit-width list, another group size and
the SmoothQuant / QuaRot / ViDiT layer classes are refused by layer name.
`format: mxfp6_e2m3fn` (`n_bits: 6`; the spelling torch and ml_dtypes use for finite-only formats; `mxfp6_e2m3` is not a key) in `act:`,
against `weight:` mxfp6_e2m3fn (W6A6) or mxfp4_e2m1 (W4A6): OCP MXFP6 e2m3 codes, 32 to 24 bytes, under the block scales of e2m1
(wanq_quant_rows_mx6, wanq_gemm_mx6).  An e2m3 weight against an e4m3 or e2m1 activation, an e4m3 weight against an e2m3 activation
and `mx.block_hadamard` with either are refused by layer name.
`mx: {block_hadamard: True}`, a top-level section: both sides of every MX Linear are quantised behind the unnormalised 32-point
Hadamard transform of each block of 32 input channels (wanq_quant_rows_mx_had32; the weight as w / 32, so the product is unchanged and
nothing is rotated back).  Accepted only with the W4A4 pair; with any other pair, or without a format, refused by layer name.
`weight.low_rank: r` (a positive int, r <= min(N, K), at most 256 after padding to a multiple of 64): the best rank-r approximation
of the quantisation error W - W_hat is kept in 16 bits beside the integer codes and added inside the weight-only GEMM
(qdiff/base/low_rank.py, wanq_gemm_wq16_lowrank).  For a weight-only integer config only, per channel or with `group_size`: with an
`act:` section, a `format:`, a bit-width list or a SmoothQuant / QuaRot / ViDiT layer class it is refused by layer name.
`gptq: {layer_name_regex: ..., damp: 0.01, block: 128}`, a top-level section in the style of `viditq:` / `smooth_quant:`: the layers
the regex names get their integer codes from the GPTQ solver (qdiff/base/gptq.py) on the Hessians under `calib_data.hessian_path`
instead of round-to-nearest; scales, zero points and everything downstream stay.  `damp` (relative to the mean of the Hessian's
diagonal) and `block` (columns per solver launch, at most 128; even with a `weight.group_size`) default to GPTQ's published values.
`act_order: True` (default False) solves the input channels in order of descending diag H on the same static groups; nothing
downstream changes, and `block` / `weight.group_size` need not be even then.
Refused by layer name: a SmoothQuant / QuaRot / ViDiT layer class, a `weight.format`, a bit-width list."""
import yaml


class ListConfig:
    def __init__(self, items=()):
        self._items = list(items)

    def __getitem__(self, i):
        return self._items[i]

    def __len__(self):
        return len(self._items)

    def __iter__(self):
        return iter(self._items)

    def __repr__(self):
        return f"ListConfig({self._items})"


class DictConfig(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def create(obj):
    if isinstance(obj, dict):
        return DictConfig({k: create(v) for k, v in obj.items()})
    if isinstance(obj, (list, tuple)):
        return ListConfig([create(v) for v in obj])
    return obj


def load(path):
    with open(path) as f:
        return create(yaml.safe_load(f))


class OmegaConf:  # the two calls the reference's scripts make
    create = staticmethod(create)
    load = staticmethod(load)
