"""Generate tests/golden/attn_multi.npz: the REFERENCE's RefAttnBackend._attention (chitu/attn_backend.py:294-392, pure torch, CPU)
with causal=True on seqlen_q = T query tokens per sequence -- the bottom-right aligned causal mask and the window formula for
seqlen_q > 1 of the attn_with_kvcache contract (:92-164) -- on the inputs of tests/attn_multi_ref.py.

Run in the build container only:   python tests/golden/gen_attn_multi.py
The cache is contiguous [B, S, Hkv, 128] with a key padding mask that keeps each sequence's attended length (the reference has
no paged pure-torch path); T of FIXM_T, every (W, softcap) of FIXM_WINDOWS x FIXM_CAPS.  Only outputs are stored (bf16 bit
patterns); the tests recompute the inputs."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shims  # noqa: E402

ref_shims.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import attn_multi_ref as mr  # noqa: E402
from tests.util import bits16, max_rel_to_peak  # noqa: E402


def main():
    from chitu.attn_backend import RefAttnBackend

    be = RefAttnBackend()
    out = {}
    for T in mr.FIXM_T:
        inp = mr.fixture_multi_inputs(T)
        S = inp["K"].shape[1]
        keep = torch.arange(S).view(1, S) < inp["lens"].view(-1, 1)
        for W in mr.FIXM_WINDOWS:
            res = {}
            for c in mr.FIXM_CAPS:
                o, _ = be._attention(inp["q"], inp["K"], inp["V"], key_padding_mask=keep, causal=True, window_size=(W, -1), softcap=c,
                                     softmax_scale=128 ** -0.5)
                assert tuple(o.shape) == tuple(inp["q"].shape) and o.dtype == torch.bfloat16
                res[c] = o
                out[mr.fixture_multi_key(T, W, c)] = bits16(o)
            if W != 0:  # the cap must matter (W = 0: one key, its weight is 1 whatever the score)
                gap = max_rel_to_peak(res[0.0], res[5.0])
                print(f"T={T} W={W}: capped vs uncapped differ by {gap:.3f} of the peak")
                assert gap > 10 * 1e-2, (T, W, gap)
    path = os.path.join(HERE, "attn_multi.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
