"""CPU-only checks of the MX Linears with outlier channels (`mx: {outlier_channels: n8}`): the host expression of the mixed MX row
format, the config key and its refusals, the choice of the channel order, and what the feature is for."""
import pytest
import torch

MX4 = {"n_bits": 4, "sym": True, "format": "mxfp4_e2m1"}
MX8 = {"n_bits": 8, "sym": True, "format": "mxfp8_e4m3"}


def layer(K=256, N=16, name="blocks.0.ffn.0", seed=0, **cfg):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    fp = torch.nn.Linear(K, N)
    fp.weight.data.copy_(torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * K ** -0.5)
    cfg = {"weight": dict(MX4), "act": dict(MX4), **cfg}
    return QuantizedLinear(K, N, True, "cpu", qcfg.create(cfg), fp, module_name=name)


@pytest.mark.parametrize("cols,n8", [(256, 128), (640, 384)])
def test_host_expression_is_the_two_plain_quantisers_on_the_gathers_and_requantising_its_decode_changes_nothing(cols, n8):
    from qdiff.base.base_quantizer import mx_decode_mixed, mx_quant_rows_host, mx_quant_rows_mixed_host

    g = torch.Generator().manual_seed(cols)
    x = torch.randn(7, cols, generator=g) * torch.exp2(torch.randint(-8, 8, (7, cols), generator=g).float())
    perm = torch.randperm(cols, generator=g).to(torch.int32)
    codes, s = mx_quant_rows_mixed_host(x, perm, n8)
    c8, s8 = mx_quant_rows_host(x[:, perm[:n8].long()], "mxfp8_e4m3")
    c4, s4 = mx_quant_rows_host(x[:, perm[n8:].long()], "mxfp4_e2m1")
    assert torch.equal(codes, torch.cat((c8, c4), 1)) and torch.equal(s, torch.cat((s8, s4), 1))
    deq = mx_decode_mixed(codes, s, n8)                      # permuted order: quantise it again in the identity order
    again, s2 = mx_quant_rows_mixed_host(deq, torch.arange(cols, dtype=torch.int32), n8)
    assert torch.equal(mx_decode_mixed(again, s2, n8), deq)


X5 = torch.zeros(5, 256)
REFUSALS = [  # (config, what is done with the layer once it is built, the refusal)
    (dict(mx={"outlier_channels": 128, "block_hadamard": True}), None, NotImplementedError, r"blocks.0.ffn.0: mx.outlier_channels with mx.block_hadamard"),
    (dict(mx={"outlier_channels": 128}, weight={**MX4, "low_rank": 8}), None, NotImplementedError, r"blocks.0.ffn.0: mx.outlier_channels with weight.low_rank"),
    (dict(mx={"outlier_channels": 128}, act=dict(MX8)), None, NotImplementedError, r"blocks.0.ffn.0: mx.outlier_channels is not supported with weight.format"),
    (dict(mx={"outlier_channels": 256}), None, ValueError, r"blocks.0.ffn.0: mx.outlier_channels=256 must be .* in_features - 128"),
    (dict(mx={"outliers": 128}), None, ValueError, r"mx.outliers is not a known key .*it has two: block_hadamard, outlier_channels"),
    (dict(mx={"outlier_channels": 128}), lambda ql: ql(X5), RuntimeError, r"blocks.0.ffn.0: mx.outlier_channels needs calibration activation statistics"),
    (dict(mx={"outlier_channels": 128}), lambda ql: ql.set_low_rank(X5[:, :8].T, X5[:, :16].T), NotImplementedError, r"set_low_rank with mx.outlier_channels"),
]


@pytest.mark.parametrize("cfg,then,exc,msg", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_name_the_layer_and_the_key(cfg, then, exc, msg):
    with pytest.raises(exc, match=msg):
        ql = layer(**cfg)
        then(ql)


def test_order_is_top_n8_by_absmax_ties_to_the_lower_index_segments_ascending_and_shared_by_consumers():
    q, k = layer(name="q", seed=1, mx={"outlier_channels": 128}), layer(name="k", seed=2, mx={"outlier_channels": 128})
    stat = torch.ones(256)
    stat[200:] = 3.0          # 56 clear outliers
    stat[10:100] = 2.0        # 90 tied candidates for the remaining 72 places: the lower indices 10 .. 81 win
    for ql in (q, k):
        ql.select_outlier_perm(stat)
    perm = q.mx_perm.tolist()
    assert perm[:128] == list(range(10, 82)) + list(range(200, 256))
    assert perm[128:] == list(range(0, 10)) + list(range(82, 200)) and q.mx_perm.dtype == torch.int32
    assert torch.equal(q.mx_perm, k.mx_perm) and not torch.equal(q._codes, k._codes)     # the weights differ, the order does not


def test_outlier_channels_lower_the_layer_error_on_activations_with_outlier_channels():
    """Seeded Gaussian activations [64, 512] with 128 channels scaled by 64 (seed 0), weights N(0, 1 / K) [96, 512]; layer output
    against float64 x w^T, both layers by their host expressions alone.  rel-L2 on this CPU: plain W4A4 1.715e-01, mixed (n8 = 128)
    4.222e-02.  The test states the direction only."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 512, generator=g)
    hot = torch.randperm(512, generator=g)[:128]
    x[:, hot] *= 64
    plain, mixed = layer(512, 96, seed=3), layer(512, 96, seed=3, mx={"outlier_channels": 128})
    mixed.get_channel_mask(x.abs().amax(0))
    assert sorted(mixed.mx_perm[:128].tolist()) == sorted(hot.tolist())
    ref = x.double() @ plain.fp_module.weight.data.double().T + plain.bias.detach().double()
    err = [float((m(x).detach().double() - ref).norm() / ref.norm()) for m in (plain, mixed)]
    print(f"rel-L2 against float64: plain W4A4 {err[0]:.3e}, mixed n8 = 128 {err[1]:.3e}")
    assert err[1] < err[0]
