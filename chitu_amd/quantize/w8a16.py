"""W8A16 weight-only int8 linears (bf16 activations x int8 weights, one fp32 scale per output row) on HIP.

Mirrors chitu/quantize/w8a16.py::WeightOnlyLinear and chitu/quantize/quantizer.py:88-114,243-250 (replace_with_w8a16,
quantize_w8a16).  The reference forwards to the third-party EETQ.w8_a16_gemm, whose arithmetic and weight permutation are
closed; the contract here is the reference's own Triton use_int8_w8a16 branch (chitu/fused_moe.py:226-227,293-294):

    acc[m][n] = sum_k float(x[m][k]) * float(q[n][k])      fp32
    out[m][n] = bf16(acc[m][n] * s[n])                     one fp32 multiply, one rounding

The quantiser is quantize/w8a8.py::quant_weight's: per output row, symmetric, s = clamp(max|w_row|, 1e-5) / 127 in fp32,
q = round(w / s) clamped to [-127, 127].  It runs at load time in plain torch on the rank's own shard.  Loading EETQ's
pre-quantised, pre-permuted checkpoints is out of scope: a bf16 / fp16 checkpoint is quantised here.
"""

import torch
from torch import nn

from .. import ops


@torch.no_grad()
def quant_weight_w8a16(w: torch.Tensor):
    """(q int8 [N, K], s fp32 [N]) of w [N, K]: s = clamp(max|w_row|, 1e-5) / 127, q = clamp(round(w / s), -127, 127)."""
    wf = w.to(torch.float32)
    s = wf.abs().max(dim=-1, keepdim=True)[0].clamp_(min=1e-5).div_(127.0)
    q = wf.div(s).round_().clamp_(-127, 127)
    return q.to(torch.int8).contiguous(), s.view(-1).contiguous()


@torch.no_grad()
def dequant_weight_w8a16(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 q * s per row: the matrix a W8A16 linear multiplies with, before any rounding."""
    return q.to(torch.float32) * s.to(torch.float32).view(-1, 1)


class WeightOnlyLinear(nn.Module):
    """The reference's name and constructor.  Buffers: `q_weight` int8 -- here [out_features, in_features], row-major like
    W8A8Linear.weight (the reference stores EETQ's [in, out] permuted layout) -- and `q_scale_col` fp32 [out_features].
    A bias is a plain torch add behind the kernel; the model path (LlamaDecoder) has none."""

    def __init__(self, in_features, out_features, bias=None, name=None):
        super().__init__()
        self.in_features, self.out_features, self.name = in_features, out_features, name
        self.register_buffer("q_weight", torch.zeros(out_features, in_features, dtype=torch.int8))
        self.register_buffer("q_scale_col", torch.ones(out_features, dtype=torch.float32))
        self.register_buffer("bias", bias)

    @torch.no_grad()
    def forward(self, x):
        y = ops.w8a16_linear(x.contiguous(), self.q_weight, self.q_scale_col)
        return y if self.bias is None else y + self.bias.to(y.dtype)

    @staticmethod
    def from_float(module, name=None):
        bias = None if getattr(module, "bias", None) is None else module.bias.data.clone()
        new = WeightOnlyLinear(module.in_features, module.out_features, bias, name)
        new.q_weight, new.q_scale_col = quant_weight_w8a16(module.weight.data)
        return new.to(module.weight.device)

    def __repr__(self):
        return f"WeightOnlyLinear({self.in_features}, {self.out_features}, bias={self.bias is not None})"


def replace_with_w8a16(model: nn.Module, skip=("lm_head", "head")):
    """Swap every nn.Linear but the output head for a WeightOnlyLinear (quantizer.py:88-114).  in_features must be a multiple
    of 64 (the kernels' K step); other linears stay as they are."""
    for name, child in list(model.named_children()):
        if isinstance(child, nn.Linear) and name not in skip and child.in_features % 64 == 0:
            setattr(model, name, WeightOnlyLinear.from_float(child, name=name))
        else:
            replace_with_w8a16(child, skip)
    return model


W8A16_WEIGHTS = (("attn", "wqkv"), ("attn", "wo"), ("ffn", "w13"), ("ffn", "w2"))


@torch.no_grad()
def quantize_w8a16_(decoder):
    """Convert an initialised bf16 LlamaDecoder (Llama, Qwen2, Qwen3) in place: wqkv, wo, w13 and w2 of every layer become
    int8 parameters with an fp32 `<name>_scale` beside them; the head, the embedding, the norms and bqkv stay bf16.  Call it
    before the first decode: a captured graph holds the bf16 addresses."""
    from ..llama import LlamaDecoder, check_quant_supported

    if not isinstance(decoder, LlamaDecoder) or not hasattr(decoder.layers[0], "ffn") or not hasattr(decoder.layers[0].ffn, "w13"):
        raise TypeError("quantize_w8a16_ converts dense LlamaDecoder models (Llama, Qwen2, Qwen3)")
    check_quant_supported("w8a16", type(decoder).__name__, dense=decoder.layers[0].ffn.w13.dim() == 2)
    if decoder.graphs:
        raise RuntimeError("quantize_w8a16_ after a decode graph was captured: the graph holds the bf16 weights")
    for layer in decoder.layers:
        for part, name in W8A16_WEIGHTS:
            mod = getattr(layer, part)
            w = getattr(mod, name)
            if w.dtype == torch.int8:
                continue
            q, s = quant_weight_w8a16(w.data)
            setattr(mod, name, nn.Parameter(q, requires_grad=False))
            setattr(mod, name + "_scale", nn.Parameter(s, requires_grad=False))
    decoder.args.quant = "w8a16"
    return decoder
