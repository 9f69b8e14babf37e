"""W4A16 group-128 weight-only int4 linears (bf16 activations x 4-bit codes, one fp32 scale per row and 128 input channels).

The format of GPTQ sym=true checkpoints (bits 4, group 128), which the reference serves through AutoGPTQ / awq_inference_engine
CUDA kernels only (serve_config_gptq.yaml, serve_config_awq.yaml).  For a linear [N, K], K % 128 == 0:

    u[n][k] in 0..15, value u - 8 (zero point 8)          s[n][k // 128] fp32
    streaming form:  out[m][n] = round( sum_g s[n][g] * sum_{k in g} float(x[m][k]) * float(u[n][k] - 8) )
                     fp32 sums of exact products, one fp32 multiply(-add) per group, one rounding
    tiled form:      out = bf16_linear(x, W'),  W'[n][k] = bf16(float(u - 8) * s)     (prefill-sized token counts)

The device layout is this module's own (pack_w4a16 / unpack_w4a16; csrc/w4a16_gemm.hip reads it, nothing else may assume it):

    packed uint8 [N, K / 2]: channel k in byte (k // 8) * 4 + k % 4, low nibble for k % 8 < 4, high nibble otherwise, stored
                             as u ^ 8 -- the two's-complement nibble of u - 8, so that a sign-extending byte convert widens it
    scales fp32 [ceil(N / 2), ceil(K / 256), 4]: {s[2p][2t], s[2p][2t+1], s[2p+1][2t], s[2p+1][2t+1]}, zero where the row or
                             the group does not exist: the four scales a lane folds a K step with are one 16-byte load
    w13 = [w1; w3] is packed per half (halves=2): the scale pairs of w1, then those of w3.

The quantiser is round-to-nearest at load time, per (row, group): s = clamp(max|w|, 1e-5) / 7, u = clamp(rint(w / s), -8, 7) + 8.
from_gptq repacks AutoGPTQ's tensors.  Out of scope: asymmetric zero points / AWQ, act-order, other group sizes.
"""

import torch
from torch import nn

from .. import ops

GROUP = 128


@torch.no_grad()
def quant_weight_w4a16(w: torch.Tensor):
    """(u uint8 [N, K] in 0..15, s fp32 [N, K / 128]) of w [N, K]: s = clamp(max|w_group|, 1e-5) / 7 in fp32,
    u = clamp(rint(w / s), -8, 7) + 8."""
    N, K = w.shape
    if K % GROUP:
        raise ValueError(f"w4a16g128: K = {K} is not a multiple of {GROUP}")
    wf = w.to(torch.float32).view(N, K // GROUP, GROUP)
    s = wf.abs().amax(dim=-1, keepdim=True).clamp_(min=1e-5).div_(7.0)
    u = wf.div(s).round_().clamp_(-8, 7).add_(8)
    return u.to(torch.uint8).view(N, K).contiguous(), s.view(N, K // GROUP).contiguous()


@torch.no_grad()
def dequant_weight_w4a16(u: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 (u - 8) * s per (row, group): the matrix a W4A16 linear multiplies with, before any rounding."""
    N, K = u.shape
    return ((u.to(torch.float32) - 8.0).view(N, K // GROUP, GROUP) * s.to(torch.float32).view(N, K // GROUP, 1)).view(N, K)


@torch.no_grad()
def pack_w4a16(u: torch.Tensor, s: torch.Tensor, halves: int = 1):
    """(packed uint8 [N, K / 2], scales fp32 [halves * ceil(N / halves / 2), ceil(K / 256), 4]) in the device layout above."""
    N, K = u.shape
    G = K // GROUP
    assert K % GROUP == 0 and N % halves == 0 and tuple(s.shape) == (N, G) and u.dtype == torch.uint8 and int(u.max()) <= 15
    t = (u ^ 8).view(N, K // 8, 2, 4)
    packed = (t[:, :, 0] | (t[:, :, 1] << 4)).reshape(N, K // 2).contiguous()
    n, P, T = N // halves, (N // halves + 1) // 2, (G + 1) // 2
    pad = torch.zeros(halves, 2 * P, 2 * T, dtype=torch.float32, device=s.device)
    pad[:, :n, :G] = s.to(torch.float32).view(halves, n, G)
    scales = pad.view(halves, P, 2, T, 2).permute(0, 1, 3, 2, 4).reshape(halves * P, T, 4).contiguous()
    return packed, scales


@torch.no_grad()
def unpack_w4a16(packed, scales=None, halves: int = 1):
    """(u, s) of pack_w4a16's result, given as two tensors or as its tuple."""
    if scales is None:
        packed, scales = packed
    N, K = packed.shape[0], packed.shape[1] * 2
    G, n = K // GROUP, N // halves
    t = packed.view(N, K // 8, 1, 4)
    u = (torch.cat([t & 15, t >> 4], dim=2) ^ 8).reshape(N, K).contiguous()
    P, T = scales.shape[0] // halves, scales.shape[1]
    s = scales.view(halves, P, T, 2, 2).permute(0, 1, 3, 2, 4).reshape(halves, 2 * P, 2 * T)[:, :n, :G].reshape(N, G).contiguous()
    return u, s


@torch.no_grad()
def from_gptq(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor, g_idx: torch.Tensor = None):
    """AutoGPTQ tensors of one linear (bits 4, group 128) -> (packed, scales) of pack_w4a16.

    qweight int32 [K / 8, N]: code of input channel k in bits 4 (k % 8) .. of qweight[k // 8][n].  scales fp16 [K / 128, N].
    qzeros int32 [K / 128, N / 8]: the zero point of output n in bits 4 (n % 8) .. of qzeros[g][n // 8], stored in one of two
    conventions: AutoGPTQ up to 0.7 (and the checkpoints made with it) stores zero - 1, i.e. 7 for sym=true; the "v2" format
    (GPTQModel, AutoGPTQ's gptq_v2 checkpoints) stores the zero itself, 8.  Both mean value = u - 8 and both are accepted; any
    other zero point is an asymmetric checkpoint and raises ValueError, as does a g_idx that is not k // 128 (act-order)."""
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    if K % GROUP or tuple(scales.shape) != (K // GROUP, N) or tuple(qzeros.shape) != (K // GROUP, (N + 7) // 8):
        raise ValueError(f"from_gptq: bits 4, group {GROUP} tensors expected; qweight {tuple(qweight.shape)}, qzeros "
                         f"{tuple(qzeros.shape)}, scales {tuple(scales.shape)}")
    if g_idx is not None and not torch.equal(g_idx.to(torch.int64).cpu(), torch.arange(K) // GROUP):
        raise ValueError("from_gptq: act-order checkpoints (g_idx != k // 128) are not supported")
    shifts = torch.arange(0, 32, 4, device=qweight.device)
    zeros = ((qzeros.unsqueeze(-1) >> shifts) & 15).reshape(K // GROUP, -1)[:, :N]
    if not (bool((zeros == 7).all()) or bool((zeros == 8).all())):
        raise ValueError("from_gptq: zero points other than 8 (stored as 7 or 8) are not supported (sym=true checkpoints only)")
    u = ((qweight.unsqueeze(1) >> shifts.view(1, 8, 1)) & 15).reshape(K, N).t().contiguous().to(torch.uint8)
    return pack_w4a16(u, scales.t().to(torch.float32).contiguous())


class W4A16Linear(nn.Module):
    """nn.Linear's forward over `packed` uint8 [out, in / 2] and `scales` (pack_w4a16).  A bias is a plain torch add behind the
    kernel; the model path (LlamaDecoder) has none."""

    def __init__(self, in_features, out_features, bias=None, name=None):
        super().__init__()
        self.in_features, self.out_features, self.name = in_features, out_features, name
        self.register_buffer("packed", torch.zeros(out_features, in_features // 2, dtype=torch.uint8))
        self.register_buffer("scales", torch.zeros(ops.w4a16_scale_shape(out_features, in_features), dtype=torch.float32))
        self.register_buffer("bias", bias)

    @torch.no_grad()
    def forward(self, x):
        y = ops.w4a16_linear(x.contiguous(), self.packed, self.scales)
        return y if self.bias is None else y + self.bias.to(y.dtype)

    @staticmethod
    def from_float(module, name=None):
        bias = None if getattr(module, "bias", None) is None else module.bias.data.clone()
        new = W4A16Linear(module.in_features, module.out_features, bias, name)
        new.packed, new.scales = pack_w4a16(*quant_weight_w4a16(module.weight.data))
        return new.to(module.weight.device)

    def __repr__(self):
        return f"W4A16Linear({self.in_features}, {self.out_features}, bias={self.bias is not None})"


def replace_with_w4a16(model: nn.Module, skip=("lm_head", "head")):
    """Swap every nn.Linear but the output head for a W4A16Linear.  in_features must be a multiple of 128 (the scale group);
    other linears stay as they are."""
    for name, child in list(model.named_children()):
        if isinstance(child, nn.Linear) and name not in skip and child.in_features % GROUP == 0:
            setattr(model, name, W4A16Linear.from_float(child, name=name))
        else:
            replace_with_w4a16(child, skip)
    return model


W4A16_WEIGHTS = (("attn", "wqkv", 1), ("attn", "wo", 1), ("ffn", "w13", 2), ("ffn", "w2", 1))


@torch.no_grad()
def quantize_w4a16_(decoder):
    """Convert an initialised bf16 LlamaDecoder (Llama, Qwen2, Qwen3, GLM-4) in place: wqkv, wo, w13 and w2 of every layer
    become packed uint8 parameters with the fp32 `<name>_scale` beside them; the head, the embedding, the norms and bqkv stay
    bf16.  Call it before the first decode: a captured graph holds the bf16 addresses."""
    from ..llama import LlamaDecoder, check_quant_supported

    if not isinstance(decoder, LlamaDecoder) or not hasattr(decoder.layers[0], "ffn") or not hasattr(decoder.layers[0].ffn, "w13"):
        raise TypeError("quantize_w4a16_ converts dense LlamaDecoder models (Llama, Qwen2, Qwen3, GLM-4)")
    check_quant_supported("w4a16g128", type(decoder).__name__, dense=decoder.layers[0].ffn.w13.dim() == 2)
    if decoder.graphs:
        raise RuntimeError("quantize_w4a16_ after a decode graph was captured: the graph holds the bf16 weights")
    for layer in decoder.layers:
        for part, name, halves in W4A16_WEIGHTS:
            mod = getattr(layer, part)
            w = getattr(mod, name)
            if w.dtype == torch.uint8:
                continue
            if w.dtype != torch.bfloat16:
                raise ValueError(f"quantize_w4a16_: {part}.{name} is {w.dtype}, not bf16")
            packed, scales = pack_w4a16(*quant_weight_w4a16(w.data), halves=halves)
            setattr(mod, name, nn.Parameter(packed, requires_grad=False))
            setattr(mod, name + "_scale", nn.Parameter(scales, requires_grad=False))
    decoder.args.quant = "w4a16g128"
    return decoder
