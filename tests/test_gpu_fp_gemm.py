"""The bf16 / fp16 GEMM with fused epilogues (csrc/gemm_bf16.hip, qgemm.fp_linear) and kernel mode's fp_gemm="hip" built on it.

Bound against the float64 definition (stated): |y - y64| <= 2^-14 * (|a| |w|^T)[m,n] elementwise for an fp32 output -- far above fp32
accumulation error over K <= 13824, far below one dropped 32-deep K slice.  Through GELU the bound grows by GELU's Lipschitz constant
(1.13) plus the epilogue's fast-GELU relative error (3e-6); through gate + residual it is scaled by |gate|.  A 16-bit output may
differ by one more unit in the last place of its type.  These are bounds on random data at full-size shapes; what the kernel and its
epilogue compute exactly (the rounding mode, the k -> fragment-slot map, stores outside the output) is pinned in
tests/test_gpu_gemm16_probes.py."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
_ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}


def gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))


def reference(a, w, bias, gelu, gate, res, hidden_ulp=0.0):
    """float64 definition and the elementwise bound of the module docstring.  hidden_ulp: the unit in the last place of a 16-bit
    GEMM output that GELU / gate + residual then read as separate passes (fp_gemm="torch"); 0 for the fused epilogue."""
    y = a.double() @ w.double().T
    s = a.double().abs() @ w.double().abs().T * 2.0 ** -14
    if bias is not None:
        y = y + bias.double()
    s = s + y.abs() * hidden_ulp
    if gelu:
        s = s * 1.13 + 3e-6 * gelu64(y).abs()
        y = gelu64(y)
    if gate is not None:
        y = res.double() + y * gate.double()
        s = s * gate.double().abs()
    return y, s


def check(out, a, w, bias=None, gelu=False, gate=None, res=None, rows=None, hidden_ulp=0.0):
    if rows is not None:
        a, out = a[rows], out[rows]
        res = None if res is None else res[rows]
    y, s = reference(a, w, bias, gelu, gate, res, hidden_ulp)
    tol = s + y.abs() * _ULP[out.dtype] + (2.0 ** -24 if out.dtype == torch.float16 else 0.0)
    err = (out.double() - y).abs()
    bad = err > tol
    assert not bad.any(), f"{int(bad.sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}"


def rand(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("gres", [None, "inplace", "outofplace"])
def test_epilogue_combinations_vs_float64(dtype, out_dtype, with_bias, gelu, gres):
    """every epilogue combination on a ragged shape with K % 64 == 32 (the half last K-tile)"""
    from viditq_extension import qgemm

    g = torch.Generator(device=DEV).manual_seed(1)
    M, N, K = 257, 136, 96
    a, w = rand((M, K), dtype, g), rand((N, K), dtype, g, 0.2)
    bias = rand((N,), dtype, g, 0.5) if with_bias else None
    gate = res = None
    if gres:
        gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
        res = rand((M, N), out_dtype, g)
    res0 = None if res is None else res.clone()
    out = qgemm.fp_linear(a, w, bias, out_dtype, gelu=gelu, gate=gate, residual=res, out=res if gres == "inplace" else None)
    assert out.dtype == out_dtype and out.shape == (M, N)
    if gres == "inplace":
        assert out.data_ptr() == res.data_ptr()
    elif gres:
        assert torch.equal(res, res0)
    check(out, a, w, bias, gelu, gate, res0)


@pytest.mark.parametrize("M", [1, 7, 130, 257, 1000, 4680])
@pytest.mark.parametrize("NK", [(8, 32), (24, 96), (136, 160), (8960, 1536), (1536, 8960), (5120, 5120)])
def test_shapes_vs_float64(M, NK):
    from viditq_extension import qgemm

    N, K = NK
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N)
    i = (M + N + K) % 4  # rotate the operand dtype and the epilogue over the sweep
    dtype = (torch.bfloat16, torch.float16)[i % 2]
    out_dtype = (torch.bfloat16, torch.float32, torch.float16, torch.float32)[i]
    a, w = rand((M, K), dtype, g), rand((N, K), dtype, g, K ** -0.5)
    bias = rand((N,), torch.float32, g, 0.1)
    gelu = i == 1
    gate = torch.rand(N, device=DEV, generator=g) if i == 3 else None
    res = rand((M, N), out_dtype, g) if i == 3 else None
    res0 = None if res is None else res.clone()
    out = qgemm.fp_linear(a, w, bias, out_dtype, gelu=gelu, gate=gate, residual=res, out=res)
    check(out, a, w, bias, gelu, gate, res0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_identity_operand_catches_transposed_store(dtype):
    """a = I with an asymmetric weight: out[m, n] = w[n, m] exactly (a swapped operand or a transposed store gives w[m, n])"""
    from viditq_extension import qgemm

    K, N = 64, 40
    g = torch.Generator(device=DEV).manual_seed(3)
    w = rand((N, K), dtype, g)
    a = torch.eye(K, device=DEV, dtype=dtype)
    out = qgemm.fp_linear(a, w, None, torch.float32)
    assert torch.equal(out, w.float().T.contiguous())


def test_rows_are_bit_equal_in_any_launch():
    from viditq_extension import qgemm

    g = torch.Generator(device=DEV).manual_seed(4)
    L, C = 32760, 1536
    x, w = rand((L, C), torch.bfloat16, g), rand((C, C), torch.bfloat16, g, C ** -0.5)
    bias = rand((C,), torch.bfloat16, g, 0.1)
    full = qgemm.fp_linear(x, w, bias, gelu=True)
    assert torch.equal(full, qgemm.fp_linear(x, w, bias, gelu=True))
    for M in (1, 77, 4680):
        for off in (0, 12345, L - M):
            part = qgemm.fp_linear(x[off:off + M].contiguous(), w, bias, gelu=True)
            assert torch.equal(part, full[off:off + M]), (M, off)
    # the fp32 gate + residual form, in place
    gate = torch.rand(C, device=DEV, generator=g)
    r = torch.randn(L, C, device=DEV, generator=g)
    rf = r.clone()
    qgemm.fp_linear(x, w, None, torch.float32, gate=gate, residual=rf, out=rf)
    rp = r[100:177].clone()
    qgemm.fp_linear(x[100:177].contiguous(), w, None, torch.float32, gate=gate, residual=rp, out=rp)
    assert torch.equal(rp, rf[100:177])


def _sample_rows(M, g):
    mid = torch.randint(4, M - 4, (24,), generator=g).tolist()
    return sorted(set([0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1] + mid))


def test_headline_ffn0_gelu_and_ffn2_gate_residual():
    from viditq_extension import qgemm

    g = torch.Generator(device=DEV).manual_seed(5)
    gc = torch.Generator().manual_seed(5)
    L, C, F = 32760, 1536, 8960
    x, w0 = rand((L, C), torch.bfloat16, g), rand((F, C), torch.bfloat16, g, C ** -0.5)
    b0 = rand((F,), torch.bfloat16, g, 0.1)
    hid = qgemm.fp_linear(x, w0, b0, gelu=True)
    rows = _sample_rows(L, gc)
    check(hid, x, w0, b0, True, rows=rows)
    w2, b2 = rand((C, F), torch.bfloat16, g, F ** -0.5), rand((C,), torch.bfloat16, g, 0.1)
    gate = torch.rand(C, device=DEV, generator=g)
    res = torch.randn(L, C, device=DEV, generator=g)
    res0 = res[rows].clone()
    qgemm.fp_linear(hid, w2, b2, torch.float32, gate=gate, residual=res, out=res)
    y, s = reference(hid[rows], w2, b2, False, gate, res0)
    assert ((res[rows].double() - y).abs() <= s + y.abs() * 2.0 ** -23).all()


def test_14b_product_and_offsets_past_2_31():
    """The 14B [75600, 5120] x [13824, 5120]^T product with an fp32 output (4.18e9 bytes; in bf16 it is 2.09e9, just short of 2^31),
    and a product with more than 2^31 output ELEMENTS; rows near both ends checked"""
    from viditq_extension import qgemm

    g = torch.Generator(device=DEV).manual_seed(6)
    M, N, K = 75600, 13824, 5120
    a, w = rand((M, K), torch.bfloat16, g), rand((N, K), torch.bfloat16, g, K ** -0.5)
    out = qgemm.fp_linear(a, w, None, torch.float32)
    assert out.numel() * out.element_size() > 2 ** 31
    rows = [0, 1, 63, 40000, M - 130, M - 2, M - 1]
    check(out, a, w, rows=rows)
    bf = qgemm.fp_linear(a, w)
    assert torch.equal(bf[rows], out[rows].to(torch.bfloat16))
    del out, bf, a, w
    M, K = 160000, 64
    a, w = rand((M, K), torch.bfloat16, g), rand((N, K), torch.bfloat16, g, K ** -0.5)
    out = qgemm.fp_linear(a, w)
    assert out.numel() > 2 ** 31
    check(out, a, w, rows=[0, 1, 77777, 155343, M - 2, M - 1])


# ---- kernel mode ----------------------------------------------------------------------------------------------------
def _make_block(dim, ffn, heads, seed):
    from wan.modules.model import WanAttentionBlock

    torch.manual_seed(seed)
    blk = WanAttentionBlock("t2v_cross_attn", dim, ffn, heads, cross_attn_norm=True)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.normal_(m.bias, std=0.05)
    blk.norm3.weight.data.uniform_(0.5, 1.5)
    blk.norm3.bias.data.normal_(std=0.1)
    for nm in (blk.self_attn.norm_q, blk.self_attn.norm_k, blk.cross_attn.norm_q, blk.cross_attn.norm_k):
        nm.weight.data.uniform_(0.5, 1.5)
    return blk


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("fp_gemm", ["hip", "torch"])
def test_block_linear_on_a_floating_point_linear_vs_float64(fp_gemm):
    """WanAttentionBlockWithHipKernel._linear on a HipLinearFp of either fp_gemm: plain, with GELU, and gate + fp32 residual with the
    update landing in the passed tensor.  M, N, K = 130, 136, 96: a ragged M tile, a ragged N tile and the K % 64 == 32 half tile.
    "hip" is held to the bound of test_epilogue_combinations_vs_float64 as it stands.  "torch" rounds the GEMM's output to bf16 before
    GELU / gate + residual run as separate passes, so that one rounding (|y| 2^-7) joins the GEMM's bound before the later stages
    scale it; its plain call has no later stage and is held to the bound unchanged."""
    from wan.quant_wanx_hip import HipLinearFp, WanAttentionBlockWithHipKernel, _FpSrc

    g = torch.Generator(device=DEV).manual_seed(7)
    M, N, K, dtype = 130, 136, 96, torch.bfloat16
    x, w, bias = rand((M, K), dtype, g), rand((N, K), dtype, g, 0.2), rand((N,), dtype, g, 0.5)
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    res = torch.randn(M, N, device=DEV, generator=g)
    res0, ptr = res.clone(), res.data_ptr()
    blk = WanAttentionBlockWithHipKernel(128, 256, 2, act_dtype=dtype, fp_gemm=fp_gemm).to(DEV)
    lin = HipLinearFp(w, bias, dtype, fp_gemm)
    hidden = _ULP[dtype] if fp_gemm == "torch" else 0.0
    y = blk._linear(lin, _FpSrc(x))
    assert y.dtype == dtype and y.shape == (M, N)
    check(y, x, w, bias)
    y = blk._linear(lin, _FpSrc(x), gelu=True)
    assert y.dtype == dtype
    check(y, x, w, bias, gelu=True, hidden_ulp=hidden)
    y = blk._linear(lin, _FpSrc(x), gate=gate, residual=res)
    assert y is res and res.data_ptr() == ptr and res.dtype == torch.float32
    check(res, x, w, bias, gate=gate, res=res0, hidden_ulp=hidden)


def test_shipped_config_block_with_hip_fp_gemm(monkeypatch):
    """The shipped configuration (ViDiT W8A8 on self_attn q / k / v, the other seven Linears FP) on one real-size block with
    fp_gemm="hip": within 1e-2 of the simulation oracle (the bar of tests/test_gpu_block.py), within 5e-3 of the same block with
    fp_gemm="torch" (the two differ by where GELU and gate + residual round: bf16 hidden state vs fp32), and neither torch's linear nor
    the separate gate + residual pass is called.  bf16 only: the block's attention kernel takes bf16 q / k / v in either mode (fp16
    operands of the GEMM itself are covered above)."""
    from oracle import qdiff_ref as qr
    from oracle import wan_ref as wr
    from qdiff import config as qcfg
    from qdiff.base.quant_model import quant_layer_refactor_
    from qdiff.utils import apply_func_to_submodules
    from viditq_extension import fused
    from wan import calib, ops
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    dim, ffn, heads, grid, lc = 1536, 8960, 12, (2, 6, 8), 64
    blk = _make_block(dim, ffn, heads, 3)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n_tok, dim, generator=g)
    x[:, 9] *= 15.0
    e0 = torch.randn(1, 6, dim, generator=g) * 0.3
    ctx = torch.randn(lc, dim, generator=g)
    freqs = wr.rope_freqs(dim // heads)
    act_mask = (torch.rand(dim, generator=g) * 3 + 0.2)
    cfg = qcfg.create({"weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": 8, "sym": True},
                       "viditq": {"alpha": 0.5665, "layer_name_regex": ""},
                       "remain_fp_regex": r"self_attn\.(?!q$)(?!k$)(?!v$)[^.]+|ffn.*|cross_attn"})
    blk = blk.to(DEV)
    apply_func_to_submodules(blk, torch.nn.Linear, quant_layer_refactor_, name=None, parent_module=None, quant_config=cfg,
                             full_name=None, remain_fp_regex=cfg.remain_fp_regex)
    gen = torch.Generator().manual_seed(11)
    vidit = {}
    for name in ("q", "k", "v"):
        lin = getattr(blk.self_attn, name)
        calib.init_rotation_and_channel_mask_(lin, "x", {"x": act_mask[None]}, gen)
        R = torch.from_numpy(qr.hadamard_from_signs(lin.rotation_signs.numpy()))
        vidit["self_attn." + name] = (lin.channel_mask.cpu(), R)
    lin = {}
    for nm in wr.LINEARS:
        w, b = sd[nm + ".weight"], sd[nm + ".bias"]
        lin[nm] = wr.FakeQuantLinear(w, b, 8, 8, False, *vidit[nm]) if nm in vidit else wr.FpLinear(w, b)
    norm_w = {k: sd[k + ".weight"].float() for k in ("self_attn.norm_q", "self_attn.norm_k", "cross_attn.norm_q", "cross_attn.norm_k")}
    ref = wr.BlockRef(lin, norm_w, sd["modulation"], heads, 1e-6, (sd["norm3.weight"].float(), sd["norm3.bias"].float()))(x, e0, grid, n_tok, ctx, freqs)

    rope = ops.rope_table(freqs, grid, DEV)
    act_dtype = torch.bfloat16
    outs = {}
    for mode in ("torch", "hip"):
        hb = WanAttentionBlockWithHipKernel.from_float(blk, None, act_dtype=act_dtype, fp_gemm=mode)
        assert hb.self_attn.q.quantized and not hb.self_attn.o.quantized and hb.ffn0.fp_gemm == mode
        outs[mode] = hb(x.to(DEV).clone(), e0.to(DEV), rope, n_tok, _FpSrc(ctx.to(DEV), act_dtype))
    err, dist = _rel(outs["hip"].float().cpu(), ref), _rel(outs["hip"], outs["torch"])
    print(f"shipped-config block, fp_gemm=hip: rel err vs oracle {err:.2e} (torch: {_rel(outs['torch'].float().cpu(), ref):.2e}), "
          f"hip vs torch {dist:.2e}")
    assert err < 1e-2 and dist < 5e-3

    def refuse(*a, **k):
        raise AssertionError("called on the fp_gemm='hip' path")

    monkeypatch.setattr(torch.nn.functional, "linear", refuse)
    monkeypatch.setattr(fused, "gate_residual_into_", refuse)
    again = hb(x.to(DEV).clone(), e0.to(DEV), rope, n_tok, _FpSrc(ctx.to(DEV), act_dtype))
    assert torch.equal(again, outs["hip"])


def _tiny_shipped_model(fp_gemm):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from wan import calib
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    quant_config = qcfg.load(os.path.join(PKG, "quant_configs", "config.yaml"))
    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=512, ffn_dim=1024, num_heads=4, num_layers=2, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 3, 20, 18)
    seq_len = seq_len_for(shape)
    ctx = [torch.randn(24, 64, device=DEV, generator=g) * 0.1 for _ in range(2)]
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, quant_config)
    model.quant_layer_refactor()
    hooks = calib.add_hooks(fp)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fp([lat0], torch.tensor([900], device=DEV), [ctx[0]], seq_len)
    data = calib.gather_and_save_activation(hooks)
    gen = torch.Generator().manual_seed(0)
    for name, mod in model.named_modules():
        if isinstance(mod, QuantizedLinear) and (mod.uses_mask or mod.uses_rotation):
            calib.init_rotation_and_channel_mask_(mod, name, data, gen)
    model.set_init_done()
    model.hardware_forward_refactor(fp_gemm=fp_gemm)
    n_fp = sum(1 for m in model.hip_blocks.modules() if getattr(m, "fp_gemm", None) == fp_gemm and not getattr(m, "quantized", True))
    assert n_fp == 14  # 7 FP Linears in each of the 2 blocks
    return model, shape, seq_len, ctx, lat0, g


def test_graph_replay_with_hip_fp_gemm_is_bit_equal_to_eager():
    from wan.graph import GraphedPasses

    model, shape, seq_len, ctx, lat0, g = _tiny_shipped_model("hip")
    gp = GraphedPasses(model, lat0, ctx, seq_len)
    for step in range(3):
        lat = torch.randn(shape, device=DEV, generator=g)
        t = torch.tensor([900 - 300 * step], device=DEV)
        eager = [model([lat], t, [c], seq_len)[0].clone() for c in ctx]
        outs = gp(lat, t)
        torch.cuda.synchronize()
        for e, o in zip(eager, outs):
            assert torch.isfinite(e).all() and torch.equal(e, o)


def test_two_pass_streams_with_hip_fp_gemm_are_bit_equal_to_one_stream():
    from wan.utils.fm_solvers_unipc import FlowUniPCMultistepScheduler
    from wan.utils.fused_step import FusedStep
    from wan.utils.two_pass import TwoPassStreams

    model, shape, seq_len, ctx, lat0, g = _tiny_shipped_model("hip")

    def loop(two):
        sched = FlowUniPCMultistepScheduler(1000, shift=1.0)
        sched.set_timesteps(4, device=DEV, shift=5.0)
        fused = FusedStep(sched, 5.0, lat0)
        lat, lats = lat0, []
        for t in sched.timesteps:
            cond, uncond = two(lambda c: model([lat], t.reshape(1), [c], seq_len)[0], lat, ctx)
            lat = fused.step(cond, uncond, lat, t)
            lats.append(lat.clone())
        torch.cuda.synchronize()
        return lats

    one = loop(TwoPassStreams(DEV, enabled=False))
    two = TwoPassStreams(DEV, mode="2")
    both = loop(two)
    assert two.enabled
    for a, b in zip(one, both):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def _run(script, *args, cwd):
    cmd = [sys.executable, os.path.join(PKG, script), "--task", "t2v-1.3B", "--size", "832*480", "--frame_num", "5", "--num_layers", "2",
           "--sample_steps", "2", "--base_seed", "42", "--output_dir", str(cwd), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd, timeout=600)
    assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def test_quant_generate_fp_gemm_hip_and_two_ranks_bit_equal(tmp_path):
    """The shipped config.yaml through the entry scripts: --fp_gemm hip is finite and within 1e-2 of --fp_gemm torch, and
    `--ulysses_size 2 --dit_fsdp --fp_gemm hip` (one-GPU rehearsal, as tests/test_gpu_entrypoints.py launches it) reproduces the
    one-rank --fp_gemm hip latent bit for bit: the GEMM's rows do not depend on how many tokens a rank holds."""
    import socket

    qc = os.path.join(PKG, "quant_configs", "config.yaml")
    calib = str(tmp_path / "calib.pth")
    _run("fp_generate.py", cwd=tmp_path)
    _run("get_calib_data_wanx.py", "--quant_config", qc, "--calib_data", calib, cwd=tmp_path)
    _run("ptq_wanx.py", "--quant_config", qc, "--calib_data", calib, cwd=tmp_path)
    _run("quant_generate.py", "--quant_config", qc, "--save_file", str(tmp_path / "torch.pt"), cwd=tmp_path)
    _run("quant_generate.py", "--quant_config", qc, "--fp_gemm", "hip", "--save_file", str(tmp_path / "one.pt"), cwd=tmp_path)
    ref, one = torch.load(tmp_path / "torch.pt", weights_only=True), torch.load(tmp_path / "one.pt", weights_only=True)
    print(f"config.yaml: --fp_gemm hip vs torch rel {_rel(one, ref):.3e}")
    assert torch.isfinite(one).all() and _rel(one, ref) < 1e-2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(PKG, "quant_generate.py"), "--task", "t2v-1.3B", "--size", "832*480", "--frame_num", "5",
           "--num_layers", "2", "--sample_steps", "2", "--base_seed", "42", "--output_dir", str(tmp_path), "--quant_config", qc,
           "--ulysses_size", "2", "--dit_fsdp", "--fp_gemm", "hip", "--save_file", str(tmp_path / "two.pt")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_ON_ONE_GPU="1"))
    assert r.returncode == 0, f"two-rank quant_generate failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "dit_fsdp:" in r.stdout + r.stderr
    two = torch.load(tmp_path / "two.pt", weights_only=True)
    assert torch.equal(one, two)
