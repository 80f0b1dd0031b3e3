"""K smoothing for the int8 Q.K^T attention (attn.qk.smooth_k / cross_attn.qk.smooth_k): the column sums of the normalised and rotated
k (wanq_rmsnorm_rope_colsum), the quantiser of k - centre (wanq_rmsnorm_rope_q8_centered), the kernel-mode block with the key set, and
the two-rank Ulysses form.  Subtracting one vector from every key of a head moves all scores of a query row alike and softmax drops
it (tests/test_smooth_k_abi.py states that in fp64), so no attention kernel changes and no bar is loosened here.

Shapes: cols 256 (one wave per row) and 1536 (the 1.3B width); rows 1, 63, 64, 65, 256, 1000 -- one ragged slab, one full slab, two
slabs, several, several with a ragged last one (a slab is 64 rows at these sizes); x in fp32, bf16 and fp16."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import qdiff_ref as qr
from oracle import wan_ref as wr

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, COLS, DTYPES = (1, 63, 64, 65, 256, 1000), (256, 1536), (torch.float32, torch.bfloat16, torch.float16)
GUARD = 64  # fp32 words of sentinel on either side of colsum and of the workspace
U = 2.0 ** -24  # unit roundoff of fp32


def _ident(L, d=128):
    t = torch.zeros(L, d // 2, 2, device=DEV)
    t[..., 0] = 1.0  # cos = 1, sin = 0: fma(a, 1, -(b * 0)) == a, the rotation is the identity bit for bit
    return t


def _colsum_guarded(x, rows, weight=None, rope=None, head_dim=128, eps=1e-6):
    """wanq_rmsnorm_rope_colsum on the first `rows` rows of x, colsum and workspace each inside sentinel words that must survive."""
    from viditq_extension import _C

    cols = x.shape[1]
    nbytes = _C.lib.wanq_rmsnorm_rope_colsum_workspace(rows, cols)
    out = torch.full((GUARD + cols + GUARD,), -77.0, dtype=torch.float32, device=DEV)
    ws = torch.full((GUARD + nbytes // 4 + GUARD,), -99.0, dtype=torch.float32, device=DEV)
    _C.call("wanq_rmsnorm_rope_colsum", _C.ptr(x), _C.dt(x), _C.ptr(weight), _C.ptr(rope), rows, cols, head_dim, max(rows, 1),
            0 if rope is None else rope.shape[0], float(eps), out[GUARD:].data_ptr(), ws[GUARD:].data_ptr(), nbytes, _C.stream())
    assert bool((out[:GUARD] == -77.0).all()) and bool((out[GUARD + cols:] == -77.0).all()), "colsum written out of bounds"
    assert bool((ws[:GUARD] == -99.0).all()) and bool((ws[GUARD + nbytes // 4:] == -99.0).all()), "workspace written out of bounds"
    return out[GUARD:GUARD + cols].clone()


# ---- G1: exact column sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_column_sums_of_integers_are_exact(rows, cols, dtype):
    """weight = rope = None, so y = x; x integer-valued in [-8, 8]: every partial sum is an integer below 2^24, so the fp32 sums
    are the integer sums whatever the order, and a slab or a row counted twice or not at all shows.  The launch sums a prefix of a
    larger buffer whose further rows are large; repeated launches agree bit for bit; the centre is sum / rows in one rounding."""
    from wan import ops

    g = torch.Generator().manual_seed(rows * 7 + cols)
    buf = torch.randint(-8, 9, (rows + 37, cols), generator=g).float()
    buf[rows:] = 1000.0  # rows past the prefix: must not be read into the sums
    xd = buf.to(dtype).to(DEV)
    want = buf[:rows].sum(0, dtype=torch.int64).float()
    got = _colsum_guarded(xd, rows)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_colsum_guarded(xd, rows), got)
    # the Python entry on the prefix as a tensor of its own, and the centre
    again = ops.rmsnorm_rope_colsum(xd[:rows].contiguous(), None, None, 128)
    assert torch.equal(again, got)
    assert torch.equal(ops.center_of(again, rows).cpu(), want / float(rows))


def test_column_sums_of_no_rows_are_zeros():
    x = torch.ones(4, 256, device=DEV)
    assert torch.equal(_colsum_guarded(x, 0), torch.zeros(256, device=DEV))


# ---- G2: general column sums ----------------------------------------------------------------------------------------------------
def _operands(rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * torch.exp(0.5 * torch.randn(cols, generator=g)) + 2.0 * torch.randn(cols, generator=g)).to(dtype)
    w = torch.rand(cols, generator=g) + 0.5
    return x.to(DEV), w.to(DEV)


def _rope(rows):
    from wan import ops

    return ops.rope_table(wr.rope_freqs(128), (1, 1, rows), DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_column_sums_with_norm_and_rope_within_the_summation_bound(rows, cols, dtype):
    """With weight and rope, against the fp64 sum of the fp32 y the plain kernel writes (ops.rmsnorm_rope_ with an fp32 `out`: the
    same row arithmetic, the same bits).  Bound: a recursive fp32 sum of n terms in ANY fixed order errs by at most
    gamma_(n-1) * sum|y_i|, gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4;
    the slab partials and their sum are such a sum, every term passing through at most n - 1 additions).  n u >= gamma_(n-1) for
    n (n - 1) u <= 1, i.e. all n <= 4096, so the bound used is rows * 2^-24 * sum|y| per column.  One row is y itself, exactly."""
    from wan import ops

    x, w = _operands(rows, cols, dtype, rows + cols)
    rope = _rope(rows)
    y = ops.rmsnorm_rope_(x, w, rope, 128, out=torch.empty(rows, cols, dtype=torch.float32, device=DEV))
    got = _colsum_guarded(x, rows, w, rope).double().cpu()
    want, mag = y.double().sum(0).cpu(), y.double().abs().sum(0).cpu()
    err, bound = (got - want).abs(), rows * U * mag
    print(f"colsum {rows}x{cols} {dtype}: max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    if rows == 1:
        assert torch.equal(got.float(), y[0].cpu())
    assert torch.equal(_colsum_guarded(x, rows, w, rope).double().cpu(), got)  # bit-reproducible


# ---- G3: centred codes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", (1, 65, 1000))
def test_centred_codes_and_scale_planes(rows, cols, dtype):
    """center = 0 is wanq_rmsnorm_rope_q8 bit for bit; a random centre gives the codes and both planes of the quantiser expression
    the q8 tests use (oracle DynamicQuantizer on [tokens * heads, 128] rows; the constant plane -12582912 * delta) applied to
    y - c computed in fp32, y being the plain kernel's fp32 row; `out` is still the uncentred row; key planes are padded to 64."""
    from wan import ops

    H = cols // 128
    x, w = _operands(rows, cols, dtype, rows * 3 + cols)
    rope = _rope(rows)
    plain, plain_fp = ops.rmsnorm_rope_q8(x, w, rope, 128, True, want_fp=True)
    zero, zero_fp = ops.rmsnorm_rope_q8(x, w, rope, 128, True, want_fp=True, center=torch.zeros(cols, device=DEV))
    assert torch.equal(zero.codes, plain.codes) and torch.equal(zero.scales, plain.scales) and torch.equal(zero_fp, plain_fp)

    c = torch.randn(cols, generator=torch.Generator().manual_seed(5)).to(DEV) * 2.0
    got, got_fp = ops.rmsnorm_rope_q8(x, w, rope, 128, True, want_fp=True, center=c)
    y = ops.rmsnorm_rope_(x, w, rope, 128, out=torch.empty(rows, cols, dtype=torch.float32, device=DEV))
    oq, odelta = qr.dynamic_quantize_sym((y - c).cpu().reshape(rows * H, 128).numpy())
    assert got.stride % 64 == 0 and got.stride >= rows and tuple(got.scales.shape) == (2, H, got.stride)
    delta = got.scales[0, :, :rows].t().contiguous().cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(delta, odelta.reshape(-1))
    np.testing.assert_array_equal(got.scales[1, :, :rows].cpu().numpy(), (np.float32(-12582912.0) * odelta).reshape(rows, H).T)
    np.testing.assert_array_equal(got.codes.cpu().numpy().astype(np.int32).reshape(rows * H, 128), oq)
    assert not bool(got.scales[:, :, rows:].any())  # the padding of the key planes stays zero
    assert torch.equal(got_fp, plain_fp)  # the 16-bit row beside the codes is the uncentred y
    q_side = ops.rmsnorm_rope_q8(x, w, rope, 128, False, center=c)  # (the query layout: unpadded planes)
    assert q_side.stride == rows and torch.equal(q_side.codes, got.codes)


# ---- G4: offset invariance, exact -----------------------------------------------------------------------------------------------
def _offset_inputs():
    """q random; k0 fp32 on a 2^-6 grid with |k0| <= 4; b = +-64 per channel; 256 rows (a power of two).  k0 + b, its column sums
    (below 2^15 on the 2^-6 grid: 21 bits) and sum / 256 are all exact in fp32, so (k0 + b) - mean(k0 + b) == k0 - mean(k0) bit for bit.
    Seed and offset were fixed after the torch-only emulation recorded in profiles/attn_smooth_k.txt."""
    L, H, d = 256, 2, 128
    g = torch.Generator().manual_seed(0)
    q = torch.randn(L, H * d, generator=g)
    k0 = (torch.randn(L, H * d, generator=g) * 64).round().clamp_(-256, 256) / 64
    b = (torch.randint(0, 2, (H * d,), generator=g) * 2 - 1).float() * 64.0
    v = torch.randn(L, H * d, generator=g).to(torch.bfloat16)
    return q, k0, b, v, H


def _ref64(q, k, v, H, d=128):
    L = q.shape[0]
    q, k, v = (t.double().view(-1, H, d).transpose(0, 1) for t in (q, k, v))
    return (torch.softmax(q @ k.transpose(1, 2) / d ** 0.5, -1) @ v).transpose(0, 1).reshape(L, H * d)


def test_a_per_channel_offset_of_k_is_invisible_with_smoothing_and_costly_without():
    """Smoothed codes, scales and attention output of k0 + b are bit-equal to those of k0.  Against fp64 attention on the same
    operands the plain int8 path's relative Frobenius error on k0 + b is at least 4 times the smoothed path's -- a condition with a
    twofold margin over the torch-only emulation (per-(token, head) fake-quant with the header's formula, fp32 attention), which
    gives 1.454e-01 against 8.946e-03, a factor 16.3 (required of it: at least 8).  This test fails without the feature."""
    from wan import ops

    q, k0, b, v, H = _offset_inputs()
    ident = _ident(q.shape[0])
    q8 = ops.rmsnorm_rope_q8(q.to(DEV), None, ident, 128, False)
    vd = v.to(DEV)

    def smooth(k):
        kd = k.to(DEV)
        c = ops.center_of(ops.rmsnorm_rope_colsum(kd, None, ident, 128), kd.shape[0])
        return c, ops.rmsnorm_rope_q8(kd, None, ident, 128, True, center=c)

    c0, s0 = smooth(k0)
    c1, s1 = smooth(k0 + b)
    assert torch.equal(c0.cpu(), k0.sum(0) / 256.0) and torch.equal(c1.cpu(), c0.cpu() + b)
    assert torch.equal(s1.codes, s0.codes) and torch.equal(s1.scales, s0.scales)
    o0, o1 = ops.attention_qk8(q8, s0, vd, H), ops.attention_qk8(q8, s1, vd, H)
    assert torch.equal(o1, o0)
    plain = ops.attention_qk8(q8, ops.rmsnorm_rope_q8((k0 + b).to(DEV), None, ident, 128, True), vd, H)
    ref = _ref64(q, k0 + b, v.float(), H)
    e_plain = ((plain.double().cpu() - ref).norm() / ref.norm()).item()
    e_smooth = ((o1.double().cpu() - ref).norm() / ref.norm()).item()
    print(f"k0 + b against fp64 attention: plain int8 {e_plain:.3e}, smoothed int8 {e_smooth:.3e}, factor {e_plain / e_smooth:.1f}")
    assert e_plain >= 4.0 * e_smooth, (e_plain, e_smooth)


# ---- G5: block --------------------------------------------------------------------------------------------------------------------
def _block_case(dim, ffn, heads, seed, outlier=False, **oracle_kw):
    from test_gpu_block import make_block
    from wan import ops

    grid, lc = (2, 6, 8), 64
    blk = make_block(dim, ffn, heads, 0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_tok, dim, generator=g)
    if outlier:
        x[:, 5] *= 12.0
    e0 = torch.randn(1, 6, dim, generator=g) * 0.3
    ctx = torch.randn(lc, dim, generator=g)
    freqs = wr.rope_freqs(dim // heads)
    ref = wr.block_from_state(sd, heads, quant=True, **oracle_kw)(x, e0, grid, n_tok, ctx, freqs)
    blk = blk.to(DEV)

    def run(**kw):
        from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

        hb = WanAttentionBlockWithHipKernel.from_float(blk, **kw)
        return hb(x.to(DEV).clone(), e0.to(DEV), ops.rope_table(freqs, grid, DEV), n_tok, _FpSrc(ctx.to(DEV), torch.bfloat16)).float().cpu()

    return ref, run


@pytest.fixture(scope="module")
def qk8_block():
    """tests/test_gpu_attn_qk8.py's block case (its shape, inputs and simulation-oracle call), computed once"""
    return _block_case(1536, 8960, 12, 1, outlier=True, qk_bits=8, cross_qk_bits=8)


@pytest.mark.parametrize("where", ["attn", "cross_attn"])
def test_kernel_mode_block_with_smooth_k_meets_the_unsmoothed_bar(qk8_block, where):
    """attn.qk + smooth_k, and cross_attn.qk + smooth_k, against the one simulation-oracle call of the unsmoothed recipe
    (BlockRef(qk_bits=8, cross_qk_bits=8)): smoothing is invisible in exact arithmetic, so the bar is that file's, 1e-2."""
    from test_gpu_block import rel_err

    ref, run = qk8_block
    out = run(attn_qk8=True, cross_attn_qk8=True, **{f"{where}_smooth_k": True})
    err = rel_err(out, ref)
    print(f"block with {where}.qk.smooth_k: rel err vs recipe oracle {err:.2e}")
    assert err < 1e-2


def test_kernel_mode_block_full_recipe_with_smooth_k_and_the_key_false():
    """The full recipe (attn_map + qk + v in both attentions) with the key set meets its existing bar, 1.5e-2; with the key false the
    block output is bit-equal to a block built without the argument."""
    from test_gpu_block import rel_err

    kw = dict(qk_bits=8, cross_qk_bits=8, v_bits=8, cross_v_bits=8, attn_map=(8, False), cross_attn_map=(8, True))
    ref, run = _block_case(512, 1024, 4, 3, **kw)
    full = dict(attn_qk8=True, cross_attn_qk8=True, attn_v_bits=8, cross_attn_v_bits=8, attn_map=(8, False), cross_attn_map=(8, True))
    err = rel_err(run(attn_smooth_k=True, cross_attn_smooth_k=True, **full), ref)
    print(f"block with the full recipe + smooth_k: rel err vs recipe oracle {err:.2e}")
    assert err < 1.5e-2
    without = run(attn_qk8=True, cross_attn_qk8=True)
    assert torch.equal(run(attn_qk8=True, cross_attn_qk8=True, attn_smooth_k=False, cross_attn_smooth_k=False), without)
    assert not torch.equal(run(attn_qk8=True, cross_attn_qk8=True, attn_smooth_k=True), without)  # (the key does something)


def test_cross_attention_memo_caches_the_centred_keys():
    """The cached cross-attention k (a context source with a `derived` dict) holds the centred Q8Rows: the second pass reuses it,
    launches no column sums, and gives the first pass's bits."""
    from test_gpu_block import make_block
    from viditq_extension import _C
    from wan import ops
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    dim, heads, grid = 512, 4, (2, 6, 8)
    hb = WanAttentionBlockWithHipKernel.from_float(make_block(dim, 1024, heads, 0).to(DEV), attn_qk8=True, cross_attn_qk8=True,
                                                   cross_attn_smooth_k=True)
    g = torch.Generator().manual_seed(2)
    x, e0, ctx = torch.randn(96, dim, generator=g).to(DEV), (torch.randn(1, 6, dim, generator=g) * 0.3).to(DEV), torch.randn(64, dim, generator=g).to(DEV)
    rope = ops.rope_table(wr.rope_freqs(dim // heads), grid, DEV)
    src = _FpSrc(ctx, torch.bfloat16)
    src.derived = {}
    names, call = [], _C.call
    try:
        _C.call = lambda name, *a, **kw: (names.append(name), call(name, *a, **kw))[1]
        first = hb(x.clone(), e0, rope, 96, src)
        n1 = names.count("wanq_rmsnorm_rope_colsum")
        second = hb(x.clone(), e0, rope, 96, src)
    finally:
        _C.call = call
    k8, _ = src.derived[id(hb)]
    assert isinstance(k8, ops.Q8Rows) and n1 == 1 and names.count("wanq_rmsnorm_rope_colsum") == 1
    assert names.count("wanq_rmsnorm_rope_q8_centered") == 1 and torch.equal(first, second)


# ---- G6: Ulysses ------------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_gpu_smooth_k_under_ulysses():
    """attn.qk + smooth_k on two ranks (tests/smooth_k_sp_worker.py: tests/sp_rehearsal_worker.py reads its config from a shipped file
    and asserts bit equality, neither of which fits a key that ships in no file and whose all-reduced sum is ordered differently):
    block output against the single-rank block under G5's bar, the all-reduced centre against the single-rank centre under G2's bound."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "smooth_k_sp_worker.py")]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("smooth_k_sp_rel=") == 2 and r.stdout.count("centre_ok=True") == 2, r.stdout[-2000:]
