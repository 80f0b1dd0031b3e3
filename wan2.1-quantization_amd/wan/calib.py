"""PTQ calibration: per-input-channel absmax of every nn.Linear input, reduced on the device.

The reference registers a forward hook on every Linear that does `x.reshape(-1,C).abs().max(dim=0)` per call and
appends the result to a Python list (get_calib_data_wanx.py:240-275), stacks the list at the end (:443-449) and
gathers pickled dicts across ranks (:455-470); ptq then takes `.max(dim=0)` over the stack (ptq_wanx.py:336).
Here each hook folds its call into ONE running fp32 [C] vector with the HIP column-absmax kernel, ranks are
joined with all_reduce(MAX), and the saved file keeps the reference's format {layer_name: Tensor[N, C]} with
N = 1 (so `calib_data[name].max(dim=0)[0]` gives the same mask)."""
import torch
import torch.distributed as dist
import torch.nn as nn

from viditq_extension import fused


class SaveActivationHook:
    def __init__(self):
        self.running = None
        self.calls = 0
        self.hook_handle = None

    def __call__(self, module, module_in, module_out):
        x = module_in[0]
        c = x.shape[-1]
        if self.running is None:
            self.running = torch.zeros(c, dtype=torch.float32, device=x.device)
        x2 = x.reshape(-1, c)
        if x2.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            x2 = x2.float()
        fused.col_absmax_(self.running, x2.contiguous())
        self.calls += 1

    @property
    def outputs(self):
        return [self.running]


class GramAccumulator:
    """H = sum of x^T x over every call (fp32 [C, C] on the device) and the number of rows summed: the GPTQ Hessian of every Linear
    that reads this input."""

    def __init__(self):
        self.H = None
        self.tokens = 0

    def add(self, x):
        c = x.shape[-1]
        x2 = x.reshape(-1, c)
        if x2.dtype not in (torch.float16, torch.bfloat16):
            x2 = x2.to(torch.bfloat16)  # (the kernel's wrapper rounds an fp32 input to bf16 itself; stated here for every other type)
        if self.H is None:
            self.H = torch.zeros(c, c, dtype=torch.float32, device=x.device)
        # The one-pass kernel (x as it lies, upper tile pairs only) launches T (T + 1) / 2 workgroups, T = ceil(C / 128).  Measured
        # against the two-sided GEMM on a transposed copy (profiles/gptq.txt): 0.70x / 0.97x of its time at C = 8960 (2485
        # workgroups; 32760 / 3120 rows), 1.5-1.6x at C = 1536 (78 workgroups leave most of the 256 CUs idle).  Nothing in between
        # is measured; the switch is put where every CU gets a workgroup.
        t = (c + 127) // 128
        if t * (t + 1) // 2 >= torch.cuda.get_device_properties(x.device).multi_processor_count:
            fused.gram_accumulate_onepass_(self.H, x2.contiguous())
        else:
            fused.gram_accumulate_(self.H, x2.contiguous())
        self.tokens += x2.shape[0]


class GramCollector:
    """What the GramHooks of one model share: the input tensor the last hook saw and its accumulator.  Layers that are called one
    after the other with the SAME tensor (self-attention q / k / v, cross-attention k / v) share one accumulator: the first of them
    adds the input, the others only point at it."""

    def __init__(self):
        self.last_x = self.last_acc = None


class GramHook:
    """Forward hook of one Linear: accumulates H = X^T X of its input (`acc.H`, `acc.tokens`), beside SaveActivationHook."""

    def __init__(self, collector):
        self.collector = collector
        self.acc = None
        self.follows = False  # this layer reads the tensor the layer before it read: that layer's accumulator is this one's
        self.hook_handle = None

    def __call__(self, module, module_in, module_out):
        x, col = module_in[0], self.collector
        if self.acc is None:  # first call: the group is fixed by who reads the same tensor
            self.follows = col.last_x is x
            self.acc = col.last_acc if self.follows else GramAccumulator()
        if not self.follows:
            self.acc.add(x)
        elif col.last_x is not x:
            raise RuntimeError("GramHook: a layer that shared its input with the layer before it was called with another tensor")
        col.last_x, col.last_acc = x, self.acc


def add_gram_hooks(model, layer_name_regex="", class_type=nn.Linear):
    """A GramHook on every `class_type` module whose name matches `layer_name_regex` (the `gptq:` section's): {name: hook}."""
    import re

    rgx, col, hooks = re.compile(layer_name_regex or ""), GramCollector(), {}
    for name, mod in model.named_modules():
        if isinstance(mod, class_type) and rgx.search(name):
            h = GramHook(col)
            h.hook_handle = mod.register_forward_hook(h)
            hooks[name] = h
    return hooks


def gather_and_save_hessians(hooks, save_path=None, group=None):
    """{clean layer name: fp32 [C, C] on the CPU}, all ranks joined with all_reduce(SUM) first; layers that shared an accumulator
    share one tensor in the file too (torch.save writes a storage once).  The file is large: C^2 x 4 bytes per accumulator, 321 MB
    for ffn.2 of the 1.3B model (C = 8960), per block."""
    out, moved = {}, {}
    for name, h in hooks.items():
        if h.hook_handle is not None:
            h.hook_handle.remove()
        if h.acc is None or (h.acc.H is None and id(h.acc) not in moved):
            continue
        if id(h.acc) not in moved:
            H = h.acc.H
            if dist.is_initialized() and dist.get_world_size(group) > 1:
                dist.all_reduce(H, op=dist.ReduceOp.SUM, group=group)
            moved[id(h.acc)] = H.cpu()
            h.acc.H = None  # one accumulator at a time leaves the device
        out[name.replace("_fsdp_wrapped_module.", "")] = moved[id(h.acc)]
    if save_path and (not dist.is_initialized() or dist.get_rank() == 0):
        torch.save(out, save_path)
    return out


def add_hooks(model, class_type=nn.Linear):
    hooks = {}
    for name, mod in model.named_modules():
        if isinstance(mod, class_type):
            h = SaveActivationHook()
            h.hook_handle = mod.register_forward_hook(h)
            hooks[name] = h
    return hooks


def gather_and_save_activation(hooks, save_path=None, group=None):
    """{clean layer name: [1, C] fp32 on CPU}; all ranks reduce with MAX first."""
    out = {}
    for name, h in hooks.items():
        if h.hook_handle is not None:
            h.hook_handle.remove()
        if h.running is None:
            continue
        r = h.running
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(r, op=dist.ReduceOp.MAX, group=group)
        out[name.replace("_fsdp_wrapped_module.", "")] = r.unsqueeze(0).cpu()
    if save_path and (not dist.is_initialized() or dist.get_rank() == 0):
        torch.save(out, save_path)
    return out


def init_rotation_and_channel_mask_(module, full_name, calib_data, generator=None):
    """ptq_wanx.py:334-344: act_mask = max over calls, floor 1e-3, then mask -> rotation -> re-quantised weight."""
    act_mask = calib_data[full_name].max(dim=0)[0].to(module.fp_module.weight.device)
    act_mask = torch.where(act_mask < 1e-3, torch.full_like(act_mask, 1e-3), act_mask)
    if getattr(module, "uses_mask", False):
        module.get_channel_mask(act_mask)
    if getattr(module, "uses_rotation", False):
        module.get_rotation_matrix(generator)
    if module.uses_mask and module.uses_rotation:
        module.update_quantized_weight_rotated_and_scaled()
    elif module.uses_mask:
        module.update_quantized_weight_scaled()
    elif module.uses_rotation:
        module.update_quantized_weight_rotated()
