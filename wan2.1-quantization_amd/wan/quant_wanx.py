"""QuantWanModel: WanModel + the quantization API the four entry points call.

Counterpart of ViDiT-Q/examples/Wan2.1/wan/quant_wanx.py:28-228 (same method names):
    quant_layer_refactor / convert_quant, save_quant_param_dict, load_quant_param_dict, set_init_done,
    bitwidth_refactor, quantize_and_save_weight(save_path), hardware_forward_refactor(load_path, seq_len).
Simulation mode = the qdiff drop-in layers inside the unmodified WanAttentionBlock (they already compute in int8);
kernel mode = every block replaced by WanAttentionBlockWithHipKernel (fused producers / epilogues around the GEMMs)."""
import logging
import math

import torch
import torch.nn as nn

from qdiff.base.quant_layer import QuantizedLinear
from qdiff.base.quant_model import QuantModel
from viditq_extension import _C

from .modules.model import WanModel
from .quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc
from . import ops

logger = logging.getLogger(__name__)


class QuantWanModel(WanModel, QuantModel):
    def __init__(self, quant_config=None, **model_kwargs):
        WanModel.__init__(self, **model_kwargs)
        self.q_cfg = quant_config
        self.quant_param_dict = {}
        self.hip_blocks = None
        self._fsdp = None
        self._rope_cache = {}

    @classmethod
    def from_pretrained(cls, checkpoint_dir, quant_config=None, **overrides):
        fp = WanModel.from_pretrained(checkpoint_dir, **overrides)
        return cls.from_float(fp, quant_config)

    @classmethod
    def from_float(cls, fp_model, quant_config):
        """A quantisable copy of `fp_model` on its device: the module tree is built without drawing initial values (every parameter is
        overwritten by the strict load that follows) and straight on that device (no host round trip of the weights)."""
        dev = next(fp_model.parameters()).device
        m = cls(quant_config, _skip_init=True, _device=dev, **fp_model.config)
        m.load_state_dict(fp_model.state_dict(), strict=True)
        return m

    def convert_quant(self, quant_config=None):
        if quant_config is not None:
            self.q_cfg = quant_config
        self.quant_layer_refactor()

    # ---- kernel mode -----------------------------------------------------------------------------------
    def quantize_and_save_weight(self, save_path=None, reference_format=False):
        """Integer state dict of every quantized Linear (reference quant_wanx.py:137-185): `<name>.weight` int8,
        `<name>.scale_weight`, `<name>.zp_weight`, `<name>.bias`; fp_module / fp_weight entries are dropped; ViDiT /
        SmoothQuant / QuaRot layers also carry `<name>.act_premul` (= channel_mask * rotation signs).
        A weight-only layer with `weight.low_rank` also carries `<name>.lr_a` [Rp, K] and `<name>.lr_b` [N, Rp], its LoRC factors
        in fp32 (qdiff/base/low_rank.py); the loader takes them when the kernel-mode layer has the buffers and raises KeyError when
        they are missing, or present without a buffer.  reference_format=True refuses such a layer by name.

        reference_format=False (default): parameters fp32 -- the precision the simulation path computes with.
        reference_format=True: byte-for-byte what the reference's `int_weight.pt` holds, so that its loader
        (W8A8OF16LinearDynamicInputScale buffers, K/viditq_extension/nn/qlinear.py:23-58) can read it: fp16 `scale_weight`,
        fp16 `zp_weight` (integer-valued: the loader copies it into an int16 buffer), fp16 bias, every other floating tensor
        fp16 (the kernel-mode blocks are `.half()`), `blocks.N.norm{1,2}.weight` = ones, and int8 codes by the reference's
        own half-precision equation (quantize_and_save_weight_, quant_wanx_cuda.py:39-53) on the HIP export kernel.  For a
        plain QuantizedLinear that equation is applied to the FP weight, exactly as the reference does; for a transformed
        layer it is applied to the layer's transformed weight (the reference applies it to the RAW weight with parameters
        fitted on the transformed one -- SURVEY D3 -- and its kernel path has no activation transform to go with it)."""
        from viditq_extension import fused

        sd = {}
        skip = set()
        f16 = torch.float16
        for name, mod in self.named_modules():
            if isinstance(mod, QuantizedLinear) and mod.w_quantizer is not None and mod.quant_mode:
                wq = mod.w_quantizer
                premul, _ = mod._act_transform()
                if reference_format:
                    if mod.fp8 or mod.mx:
                        raise NotImplementedError(f"{name}: the reference's int_weight.pt format holds int8 codes (the layer is "
                                                  f"format: {mod.mx or 'fp8_e4m3'}; save with reference_format=False)")
                    if mod.low_rank is not None or mod._adapter is not None:
                        raise NotImplementedError(f"{name}: the reference's int_weight.pt format has no low-rank branch "
                                                  "(weight.low_rank / set_low_rank; save with reference_format=False)")
                    if mod.gptq is not None:
                        raise NotImplementedError(f"{name}: the reference's int_weight.pt format derives its codes from the FP weight "
                                                  "by the reference's own half-precision equation; a `gptq:` layer's codes come "
                                                  "from the solver (save with reference_format=False)")
                    if mod.group_size is not None:
                        raise NotImplementedError(f"{name}: the reference's int_weight.pt format has one scale per output channel "
                                                  "(weight.group_size is set; save with reference_format=False)")
                    if wq.n_bits != 8:
                        raise NotImplementedError(f"{name}: the reference's int_weight.pt format is W8 only (n_bits={wq.n_bits})")
                    s16 = wq.delta.reshape(-1).to(f16).contiguous()
                    z16 = (torch.zeros_like(s16) if wq.sym else wq.zero_point.reshape(-1).to(f16)).contiguous()
                    src = mod.fp_module.weight.data if premul is None else mod.weight.data
                    sd[name + ".weight"] = fused.weight_export_f16(src.detach().contiguous(), s16, z16)
                    sd[name + ".scale_weight"] = s16
                    sd[name + ".zp_weight"] = z16
                    if mod.bias is not None:
                        sd[name + ".bias"] = mod.bias.detach().to(f16).clone()
                else:
                    # 8-bit: int8 [N, K]; 4-bit: uint8 [N, K/2], the packed nibbles exactly as the GEMM reads them; format: fp8_e4m3:
                    # uint8 [N, K], the e4m3 bytes, with their per-channel scales
                    # (weight.group_size: the parameters as the group-wise GEMM reads them, [K / g, N]); format: mxfp8_e4m3 /
                    # mxfp4_e2m1: uint8 [N, K] e4m3 bytes / uint8 [N, K/2] packed e2m1 nibbles, scale_weight uint8 [N, K/32] E8M0 bytes;
                    # mxfp6_e2m3fn: uint8 [N, 3K/4] packed e2m3 codes, and `mx_fmt` with either weight of an e2m3-activation layer
                    grouped = mod.group_size is not None
                    sd[name + ".weight"] = mod._codes.clone()
                    sd[name + ".scale_weight"] = (wq.scale_u8.clone() if mod.mx else
                                                  wq.delta.float().t().contiguous() if grouped else wq.delta.reshape(-1).float().clone())
                    if not wq.sym:
                        sd[name + ".zp_weight"] = (wq.zero_point.float().t().contiguous() if grouped
                                                   else wq.zero_point.reshape(-1).float().clone())
                    if mod.bias is not None:
                        sd[name + ".bias"] = mod.bias.detach().float().clone()
                    if mod.mx_act == "mxfp6_e2m3fn":  # W6A6 / W4A6: the (weight, act) format codes of wanq_gemm_mx6, recorded with the layer
                        sd[name + ".mx_fmt"] = torch.tensor([_C.MX6_FMT[mod.mx], _C.MX6_FMT[mod.mx_act]], dtype=torch.uint8)
                    if mod.mx_had32:  # codes made behind the block Hadamard rotation (mx.block_hadamard): recorded with the layer
                        sd[name + ".mx_had32"] = torch.ones(1, dtype=torch.uint8)
                    if mod.low_rank is not None:  # the LoRC factors, fp32 [Rp, K] / [N, Rp] (an adapter is not part of the weights)
                        sd[name + ".lr_a"] = mod.lr_a.detach().float().clone()
                        sd[name + ".lr_b"] = mod.lr_b.detach().float().clone()
                if premul is not None:
                    sd[name + ".act_premul"] = premul.clone()
                skip.add(name)
        for k, v in self.state_dict().items():
            owner = k.rsplit(".", 1)[0]
            if any(owner == s or owner.startswith(s + ".") for s in skip):
                continue
            v = v.detach().clone()
            sd[k] = v.to(f16) if reference_format and v.is_floating_point() and k.startswith("blocks.") else v
        if reference_format:
            for i in range(len(self.blocks)):  # the fused LayerNorm kernel takes a weight: vanilla LN = ones (quant_wanx.py:173-177)
                sd[f"blocks.{i}.norm1.weight"] = torch.ones(self.dim, dtype=f16)
                sd[f"blocks.{i}.norm2.weight"] = torch.ones(self.dim, dtype=f16)
        if save_path:
            torch.save(sd, save_path)
        return sd

    def hardware_forward_refactor(self, load_path=None, seq_len=None, act_dtype=torch.bfloat16, fp_gemm="torch"):
        """Switch forward() to kernel mode: every block becomes a WanAttentionBlockWithHipKernel (reference
        quant_wanx.py:188-228).  The blocks are built from the model's current layers (which fixes which Linears are
        quantized and which carry a rotation); with `load_path` the integer checkpoint is then LOADED into them, as the
        reference does with `int_weight.pt`: codes, scales, zero points, biases and activation pre-multipliers of every
        quantized Linear come from the file (either format of quantize_and_save_weight), a quantized Linear without its keys
        or with a shape mismatch is an error, and the number of tensors taken is logged.  fp_gemm: the GEMM of the Linears kept
        floating point, "torch" (hipBLASLt + separate GELU / gate + residual passes) or "hip" (csrc/gemm_bf16.hip, both fused)."""
        qk8, vb, amap, smooth = {}, {}, {}, {}
        for key in ("attn", "cross_attn"):  # quant_config.attn.qk / cross_attn.qk (Q/base/quant_attn.py:19-29,130-143)
            sub = self.q_cfg.get(key, None) if self.q_cfg is not None else None
            qk = sub.get("qk", None) if sub is not None else None
            if qk is not None:
                if qk.get("n_bits", 8) != 8 or not qk.get("sym", True):
                    raise NotImplementedError(f"{key}.qk: the int8 Q.K^T kernel implements symmetric 8-bit q / k")
                qk8[key] = True
                # qk.smooth_k: k is quantised as k - its mean over the tokens (exact under softmax; one more read of k per attention)
                smooth[key] = bool(qk.get("smooth_k", False))
            if sub is not None and sub.get("smooth_k", None) is not None:
                raise ValueError(f"{key}.smooth_k: K smoothing is a property of the int8 q / k codes and is spelled {key}.qk.smooth_k"
                                 + ("" if qk is not None else f"; this section has no {key}.qk for it to act on"))
            vq = sub.get("v", None) if sub is not None else None
            if vq is not None:  # v fake-quant per (head, channel) over all tokens (W/models/quant_opensora.py:438-440)
                if not vq.get("sym", True):
                    raise NotImplementedError(f"{key}.v: symmetric v quantisation is implemented (the reference's DynamicQuantizer default)")
                vb[key] = int(vq.get("n_bits", 8))
            am = sub.get("attn_map", None) if sub is not None else None
            if am is not None:  # post-softmax map, one dynamic group per KEY column (Q/base/quant_attn.py:166-173, group 'row')
                if am.get("group", "row") not in ("row", "column"):  # the OpenSORA class calls it 'row', the CogVideoX class 'column': same code
                    raise NotImplementedError(
                        f"{key}.attn_map.group = {am.get('group')!r}: the 'block' mode of the reference is tied to CogVideoX's 13x30x45 grid "
                        "and to per-head reorder tables (Q/base/quant_attn.py:176-236); 'row' is implemented (streamed, csrc/attn_map.hip)")
                if act_dtype == torch.float16:
                    raise NotImplementedError(
                        f"{key}.attn_map with act_dtype=torch.float16: the attention-map kernels (csrc/attn_map.hip) hand P to the matrix "
                        "cores as a bf16 hi + lo pair and take bf16 q / k / v only; build kernel mode with act_dtype=torch.bfloat16")
                amap[key] = (int(am.get("n_bits", 8)), bool(am.get("sym", False)))
        # the fp32 ends of a pass (csrc/embed_head.hip: patch / time / text embeddings, head) read these parameters as fp32, as the
        # reference computes them (amp.autocast(dtype=torch.float32) around the time MLPs and the head, model.py:592-597,396-399):
        # say so here, once, instead of a dtype refusal from inside the first forward
        ends = [("patch_embedding", self.patch_embedding), ("time_embedding.0", self.time_embedding[0]), ("time_embedding.2", self.time_embedding[2]),
                ("time_projection.1", self.time_projection[1]), ("text_embedding.0", self.text_embedding[0]), ("text_embedding.2", self.text_embedding[2]),
                ("head.head", self.head.head)]
        bad = [f"{n}.weight is {m.weight.dtype}" for n, m in ends if m.weight.dtype != torch.float32]
        if bad or self.head.modulation.dtype != torch.float32:
            raise TypeError("kernel mode keeps the embeddings and the head in fp32 (load the checkpoint in fp32, or call .float() on them "
                            "before hardware_forward_refactor): " + ", ".join(bad + ([f"head.modulation is {self.head.modulation.dtype}"]
                                                                                   if self.head.modulation.dtype != torch.float32 else [])))
        self.__dict__.pop("_ctx_cache", None)
        self.hip_blocks = nn.ModuleList([WanAttentionBlockWithHipKernel.from_float(
            b, None, False, act_dtype, attn_qk8=qk8.get("attn", False), cross_attn_qk8=qk8.get("cross_attn", False),
            attn_v_bits=vb.get("attn"), cross_attn_v_bits=vb.get("cross_attn"), attn_map=amap.get("attn"),
            cross_attn_map=amap.get("cross_attn"), fp_gemm=fp_gemm, name=f"blocks.{i}", attn_smooth_k=smooth.get("attn", False),
            cross_attn_smooth_k=smooth.get("cross_attn", False)) for i, b in enumerate(self.blocks)])
        if load_path:
            sd = torch.load(load_path, map_location="cpu", weights_only=True)
            taken = taken_wo = 0
            for i, hb in enumerate(self.hip_blocks):
                for owner, attr, key in [(hb.self_attn, l, f"self_attn.{l}") for l in "qkvo"] + \
                                        [(hb.cross_attn, l, f"cross_attn.{l}") for l in "qkvo"] + \
                                        [(hb, "ffn0", "ffn.0"), (hb, "ffn2", "ffn.2")]:
                    lin = getattr(owner, attr)
                    if not lin.checkpointed:
                        continue
                    weight_only = lin.weight_only  # HipLinearWq16: the same keys, no act_premul
                    base = f"blocks.{i}.{key}"
                    # The two formats carry no marker.  What tells them apart is that reference_format=True writes fp16 scales and the
                    # default format fp32 ones (quantize_and_save_weight): the test below relies on that.  A file with fp32 scales
                    # around codes of the reference's half-precision equation would be taken as the default format.
                    if weight_only and f"{base}.scale_weight" in sd and sd[f"{base}.scale_weight"].dtype == torch.float16:
                        raise NotImplementedError(f"{load_path}: {base} is a weight-only layer and the file is in the reference's "
                                                  "int_weight.pt format, which is W8A8 only (save with reference_format=False)")
                    # an MX layer's codes are those of one rotation setting: `<name>.mx_had32` says the file's (absent: unrotated)
                    rec = sd.get(f"{base}.mx_had32", None)
                    had_file, had_layer = rec is not None and bool(rec.reshape(-1)[0] != 0), bool(getattr(lin, "had32", False))
                    if had_file != had_layer:
                        raise ValueError(f"{load_path}: {base} holds codes quantised {'behind' if had_file else 'without'} the block "
                                         f"Hadamard rotation (mx.block_hadamard) and the model's layer was built "
                                         f"{'with' if had_layer else 'without'} it: the two are not interchangeable")
                    # an e2m3-activation layer records its (weight, act) formats in `<name>.mx_fmt`; no other layer has the key
                    rec, own = sd.get(f"{base}.mx_fmt", None), getattr(lin, "mx_fmt", None)
                    if (rec is None) != (own is None) or (rec is not None and rec.reshape(-1).tolist() != own.reshape(-1).tolist()):
                        said = lambda v: "no mx_fmt (not an MXFP6 layer)" if v is None else f"mx_fmt {v.reshape(-1).tolist()}"  # noqa: E731
                        raise ValueError(f"{load_path}: {base} was saved with {said(rec)} and the model's layer was built with "
                                         f"{said(own)} ((weight, act) codes of wanq_gemm_mx6: 2 = mxfp6_e2m3fn, 1 = mxfp4_e2m1)")
                    for buf, k, required in (("weight", "weight", True), ("scale_weight", "scale_weight", True),
                                             ("mx_fmt", "mx_fmt", own is not None),
                                             ("zp_weight", "zp_weight", lin.zp_weight is not None),
                                             ("bias", "bias", lin.bias is not None),
                                             ("act_premul", "act_premul", lin.act_premul is not None),
                                             ("mx_had32", "mx_had32", had_layer),
                                             ("lr_a", "lr_a", getattr(lin, "lr_a", None) is not None),
                                             ("lr_b", "lr_b", getattr(lin, "lr_b", None) is not None)):
                        dst = getattr(lin, buf, None)
                        if f"{base}.{k}" not in sd:
                            if required:
                                raise KeyError(f"{load_path}: missing {base}.{k}")
                            continue
                        src = sd[f"{base}.{k}"]
                        if dst is None:
                            # the reference's format always carries `zp_weight` (quant_wanx_cuda.py:39-53 writes one per layer):
                            # for a symmetric layer it is all zeros and there is nothing to load
                            if buf == "zp_weight" and not bool(src.float().abs().max() > 0):
                                continue
                            raise KeyError(f"{load_path}: {base}.{k} present but the model's layer has no {buf}")
                        if tuple(src.shape) != tuple(dst.shape) or ((buf == "weight" or dst.dtype == torch.uint8) and src.dtype != dst.dtype):
                            raise ValueError(f"{load_path}: {base}.{k} is {tuple(src.shape)} {src.dtype}, expected {tuple(dst.shape)} {dst.dtype}")
                        dst.copy_(src.to(dst.dtype))
                        taken += 1
                        taken_wo += weight_only
                    lin.refresh_zp_gemm()
            logger.info("loaded %d tensors of the integer checkpoint %s into the kernel-mode blocks (%d of them into weight-only layers)",
                        taken, load_path, taken_wo)
        for i, hb in enumerate(self.hip_blocks):
            hb.block_index = i
        self.__dict__.pop("_mod_all", None)
        return self

    def shard_blocks(self, group=None):
        """`--dit_fsdp` (reference wan/distributed/fsdp.py:10-32, text2video.py:106-107): shard the kernel-mode blocks' integer
        weights over the ranks of `group`; forward() then all-gathers one block ahead of the one it is computing."""
        from .distributed.fsdp import ShardedBlocks

        assert self.hip_blocks is not None, "shard_blocks applies to kernel mode (call hardware_forward_refactor first)"
        self.__dict__.pop("_ctx_cache", None)
        self._fsdp = ShardedBlocks(self.hip_blocks, group)
        return self._fsdp

    def software_forward(self):
        self.hip_blocks = None
        return self

    def _rope(self, grid, device):
        if grid not in self._rope_cache:
            self._rope_cache[grid] = ops.rope_table(self.freqs, grid, device)
        return self._rope_cache[grid]

    def _context_source(self, raw, embed):
        """The blocks' view of one text context, with what they derive from it kept across the sampling loop.  Everything a pass
        computes from the context alone -- text_embedding, its plain int8 copy, cross_attn.k (+ RMSNorm) and cross_attn.v -- is
        independent of the timestep and the latent, and text2video.py hands every step the SAME context tensors (cond, uncond), so
        it is kept per live tensor: the entry holds the tensor itself (its storage cannot be recycled under the cache) and its
        in-place version counter; a different tensor, or the same one after an in-place write, recomputes.  `embed` is the callable
        that runs text_embedding (only on a miss).  At most four entries; `context_cache = False` (bench.py --no-context-cache)
        turns it off, anything that rebuilds the kernel-mode blocks (hardware_forward_refactor, shard_blocks) empties it.  Never
        used under graph capture (wan/graph.py turns it off for its warm-up and capture as well): a captured graph must hold the
        text_embedding / cross_attn.k / .v launches itself -- it would otherwise bake in pointers to tensors that only this cache
        owns (freed by the fifth other context or a rebuild of the blocks) and ignore later in-place updates of its static
        context buffers."""
        src = lambda: _FpSrc(embed().float().contiguous(), self.hip_blocks[0].act_dtype)  # noqa: E731
        if not getattr(self, "context_cache", True) or (raw.is_cuda and torch.cuda.is_current_stream_capturing()):
            return src()
        cache = self.__dict__.setdefault("_ctx_cache", [])
        for ent in cache:
            if ent[0] is raw and ent[1] == raw._version:
                return ent[2]
        cq = src()
        cq.derived = {}
        cache.append((raw, raw._version, cq))
        del cache[:-4]
        return cq

    def _modulations(self, device):
        """All kernel-mode blocks' modulation tables as one [blocks, 6, C] tensor (so that `modulation + e0` of reference
        model.py:322-324 is one launch per pass, not one per block); rebuilt when a block's table was written or moved."""
        if torch.cuda.is_current_stream_capturing():
            # under graph capture the table must live in the graph's own memory pool: a tensor this cache owns would be freed by the
            # next rebuild (a modulation write, .to(), hardware_forward_refactor) while the captured graph still points at it
            return torch.cat([hb.modulation.to(device) for hb in self.hip_blocks]).contiguous()
        key = (device, tuple(hb.modulation._version for hb in self.hip_blocks), tuple(hb.modulation.data_ptr() for hb in self.hip_blocks))
        ent = self.__dict__.get("_mod_all")
        if ent is None or ent[0] != key:
            ent = (key, torch.cat([hb.modulation.to(device) for hb in self.hip_blocks]).contiguous())
            self.__dict__["_mod_all"] = ent
        return ent[1]

    def _embed_hip(self, xi, ti, seq_len):
        """The embeddings in front of the blocks (reference model.py:580-597) on csrc/embed_head.hip, all fp32: patch embedding
        gathered straight from the latent (padded to seq_len rows with zeros), sinusoid -> time_embedding -> time_projection.
        -> (h [seq_len, dim], e [dim], e0 [1, 6, dim], token grid)."""
        pe, te, tp = self.patch_embedding, self.time_embedding, self.time_projection
        dev = pe.weight.device
        h, grid = ops.patch_embed(xi.to(dev, torch.float32).contiguous(), pe.weight, pe.bias, out_rows=seq_len)
        assert math.prod(grid) <= seq_len
        e = ops.linear_f32(ops.time_sinusoid(ti.to(dev), self.freq_dim), te[0].weight, te[0].bias, out_act="silu")
        e = ops.linear_f32(e, te[2].weight, te[2].bias)
        e0 = ops.linear_f32(e, tp[1].weight, tp[1].bias, in_act="silu")
        return h, e[0], e0.view(1, 6, self.dim), grid

    def _text_embed_hip(self, ci):
        """text_embedding (reference model.py:600-605): the context padded to text_len rows with zeros BEFORE the MLP."""
        tx = self.text_embedding
        c = ci.to(tx[0].weight.device, torch.float32).contiguous()
        assert c.shape[0] <= self.text_len
        return ops.linear_f32(ops.linear_f32(c, tx[0].weight, tx[0].bias, out_act="gelu_tanh", rows=self.text_len), tx[2].weight, tx[2].bias)

    @torch.no_grad()
    def forward(self, x, t, context, seq_len, sp=None):
        if self.hip_blocks is None:  # simulation mode: the fake-quant Linears are token-local, the FP model's Ulysses path applies
            return WanModel.forward(self, x, t, context, seq_len, sp)
        outs = []
        hd = self.head
        for xi, ci, ti in zip(x, context, t.reshape(-1, 1)):
            with torch.autocast("cuda", enabled=False):
                h, e, e0, grid = self._embed_hip(xi, ti, seq_len)
                L0 = math.prod(grid)
                rope = self._rope(grid, h.device)
                if sp is not None and sp.size > 1:
                    lp = seq_len // sp.size
                    h = sp.shard_rows(h).contiguous()
                    rope = rope[sp.rank * lp:(sp.rank + 1) * lp]
                cq = self._context_source(ci, lambda: self._text_embed_hip(ci))
                e_all = self._modulations(e0.device) + e0  # every block's modulation + e0 (reference model.py:322-324), one launch per pass
                if getattr(self, "_fsdp", None) is not None:
                    self._fsdp.run(lambda blk: blk(h, e0, rope, L0, cq, sp, e=e_all[blk.block_index:blk.block_index + 1]))
                else:
                    for i, blk in enumerate(self.hip_blocks):
                        blk(h, e0, rope, L0, cq, sp, e=e_all[i:i + 1])
                hw, hb, mod = hd.head.weight, hd.head.bias, hd.modulation.view(2, self.dim)
                if sp is not None and sp.size > 1:  # the head is token-local: on the shard, then gathered (xdit_context_parallel.py:138-142)
                    out = sp.all_gather_rows(ops.head(h, mod, e, hw, hb, hd.eps)).unsqueeze(0)
                    outs.append(self.unpatchify(out, [grid])[0].float())
                else:  # LayerNorm + modulation + Linear + unpatchify in one launch
                    latent = (self.out_dim, *[g * p for g, p in zip(grid, self.patch_size)])
                    outs.append(ops.head(h[:L0], mod, e, hw, hb, hd.eps, latent_shape=latent, patch=self.patch_size))
        return outs
