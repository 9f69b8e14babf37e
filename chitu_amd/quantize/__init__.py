"""Quantised linears on the decode path (reference: chitu/quantize/).  The W8A8 int8 path (`simple_w8a8`,
quantizer.py:117-145) and the W8A16 weight-only int8 path (`w8a16`, quantizer.py:88-114,243-250) are on the MI355X hot
path; AWQ / GPTQ / muxi variants are other formats backed by closed or third-party kernels and are out of scope
(SURVEY.md 2.2)."""

from .w8a8 import W8A8Linear, quant_act, quant_weight, replace_with_simple_w8a8  # noqa: F401
from .w8a16 import (WeightOnlyLinear, dequant_weight_w8a16, quant_weight_w8a16, quantize_w8a16_,  # noqa: F401
                    replace_with_w8a16)


def quant(model, method="simple_w8a8", **kwargs):
    """Dispatcher with the reference's name (chitu/quantize/quantizer.py:277-291)."""
    if method in ("simple_w8a8", "w8a8"):
        return replace_with_simple_w8a8(model, **kwargs)
    if method == "w8a16":
        return replace_with_w8a16(model, **kwargs)
    raise NotImplementedError(f"quant method {method!r} is not part of the MI355X decode path")
