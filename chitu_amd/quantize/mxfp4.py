"""OCP MXFP4 (MX v1.0) weight tensors for the W4A8 expert path (`fused_experts(use_mxfp4_w4a8=True)`).

Format: e2m1 elements (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), two per byte with the even k in the low nibble, and one E8M0
scale byte per 32 consecutive k of a row (value 2^(byte - 127), 0xFF = NaN) -- the layout public MXFP4 checkpoints use.
`[..., K]` values become `uint8 [..., K/2]` + `uint8 [..., K/32]`.

Every function takes device tensors and runs a HIP kernel of csrc/moe_mxfp4.hip; there is no CPU path (the tests keep their
own pure-torch statement of the format).  New: no reference counterpart.
"""

from typing import Tuple

import torch

from .. import _lib
from .._lib import check, i32, i64, ptr, require_cuda, stream_ptr

__all__ = ["quant_mxfp4", "quant_mxfp4_from_fp8_block", "dequant_mxfp4"]

_SRC_KIND = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def _alloc(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    K = w.shape[-1]
    packed = torch.empty(*w.shape[:-1], K // 2, dtype=torch.uint8, device=w.device)
    scales = torch.empty(*w.shape[:-1], K // 32, dtype=torch.uint8, device=w.device)
    return packed, scales


def quant_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 / f16 / f32 `[..., K]` (K % 32 == 0) -> (packed uint8 `[..., K/2]`, scales uint8 `[..., K/32]`).

    The OCP rule per 32-block: shared exponent X = floor(log2(max|v|)) - 2, scale byte = clamp(X + 127, 0, 254); elements =
    round-to-nearest-even of v / 2^X on the e2m1 grid, saturated to +-6.  An all-zero block gets scale byte 0."""
    require_cuda(w)
    assert w.dtype in _SRC_KIND, "bf16, f16 or f32 values"
    assert w.dim() >= 1 and w.shape[-1] % 32 == 0, "the last dimension must hold whole 32-blocks"
    w = w.contiguous()
    packed, scales = _alloc(w)
    K = w.shape[-1]
    check(_lib.lib().chitu_hip_quant_mxfp4(ptr(w), i32(_SRC_KIND[w.dtype]), ptr(None), i64(w.numel() // K), i64(K), i64(1),
                                           ptr(packed), ptr(scales), stream_ptr()), "quant_mxfp4")
    return packed, scales


def quant_mxfp4_from_fp8_block(w: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """e4m3 weights `[..., R, K]` with DeepSeek's [128, 128] fp32 block scales `[..., ceil(R/128), K/128]` -> MXFP4 of the
    dequantised values float(w) * scale (one fp32 product per element, then `quant_mxfp4`'s rule), without materialising
    them.  K % 128 == 0."""
    require_cuda(w, scale)
    assert w.element_size() == 1 and w.dim() >= 2 and scale.dtype == torch.float32
    R, K = w.shape[-2], w.shape[-1]
    assert K % 128 == 0, "K must hold whole 128-blocks"
    assert tuple(scale.shape) == tuple(w.shape[:-2]) + ((R + 127) // 128, K // 128), "block scales must be [..., ceil(R/128), K/128]"
    w, scale = w.contiguous(), scale.contiguous()
    packed, scales = _alloc(w)
    check(_lib.lib().chitu_hip_quant_mxfp4(ptr(w), i32(3), ptr(scale), i64(w.numel() // K), i64(K), i64(R), ptr(packed),
                                           ptr(scales), stream_ptr()), "quant_mxfp4_from_fp8_block")
    return packed, scales


def dequant_mxfp4(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(packed uint8 `[..., K/2]`, scales uint8 `[..., K/32]`) -> bf16 `[..., K]`: e2m1 x 2^(byte - 127).  Exact for scale
    bytes 2..252 (two significant bits, every product a normal number); byte 0xFF gives NaN."""
    require_cuda(packed, scales)
    assert packed.dtype == torch.uint8 and scales.dtype == torch.uint8
    K = packed.shape[-1] * 2
    assert K % 32 == 0 and tuple(scales.shape) == tuple(packed.shape[:-1]) + (K // 32,), "scales must be [..., K/32]"
    packed, scales = packed.contiguous(), scales.contiguous()
    out = torch.empty(*packed.shape[:-1], K, dtype=torch.bfloat16, device=packed.device)
    check(_lib.lib().chitu_hip_dequant_mxfp4(ptr(packed), ptr(scales), i64(packed.numel() * 2 // K), i64(K), ptr(out),
                                             stream_ptr()), "dequant_mxfp4")
    return out
