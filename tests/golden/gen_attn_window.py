"""Generate tests/golden/attn_window.npz: the REFERENCE's RefAttnBackend (chitu/attn_backend.py:246-501, pure torch, CPU) under
window_size = (W, 0) / causal windows and softcap, on the inputs of tests/attn_window_ref.py.

Run in the build container only:   python tests/golden/gen_attn_window.py
  decode:  attn_with_kvcache on a contiguous cache [B, S, Hkv, 128] with the in-place append (the reference has no paged
           pure-torch path), attended lengths FIX_LENGTHS, every (W, softcap) of FIX_WINDOWS x FIX_CAPS;
  prefill: attn_varlen_func with causal=True on the sequences FIX_SEQS in one batch, the same (W, softcap); kept rows only.
Only outputs are stored (bf16 bit patterns); the tests recompute the inputs."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shims  # noqa: E402

ref_shims.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import attn_window_ref as wr  # noqa: E402
from tests.util import bits16, max_rel_to_peak  # noqa: E402


def main():
    from chitu.attn_backend import RefAttnBackend

    be = RefAttnBackend()
    out = {}
    dec, pre = wr.fixture_decode_inputs(), wr.fixture_prefill_inputs()
    cu = torch.tensor(pre["cu"], dtype=torch.int32)
    rows = wr.fixture_prefill_rows()
    m = max(wr.FIX_SEQS)
    for W in wr.FIX_WINDOWS:
        res = {}
        for c in wr.FIX_CAPS:
            kc, vc = dec["k_cache"].clone(), dec["v_cache"].clone()
            d = be.attn_with_kvcache(dec["q"], kc, vc, dec["k_new"], dec["v_new"], cache_seqlens=dec["cache_seqlens"],
                                     window_size=(W, 0) if W >= 0 else (-1, -1), softcap=c, softmax_scale=128 ** -0.5)
            K, V = wr.fixture_decode_rows(dec)
            assert torch.equal(kc, K) and torch.equal(vc, V)  # the reference appended in place
            p = be.attn_varlen_func(pre["q"], pre["k"], pre["v"], cu, cu, m, m, causal=True, window_size=(W, -1), softcap=c,
                                    softmax_scale=128 ** -0.5)
            res[c] = (d[:, 0], p)
            out[wr.fixture_key("decode", W, c)] = bits16(d[:, 0])
            out[wr.fixture_key("prefill", W, c)] = bits16(p[rows])
        # the cap must matter: a kernel that ignores softcap has to miss the comparison bar by a wide margin (W = 0: one key, its
        # weight is 1 whatever the score)
        if W == 0:
            continue
        for kind, (a, b) in zip(("decode", "prefill"), zip(res[0.0], res[5.0])):
            gap = max_rel_to_peak(a, b)
            print(f"W={W} {kind}: capped vs uncapped differ by {gap:.3f} of the peak")
            assert gap > 10 * wr.FIX_BAR, (W, kind, gap)
    path = os.path.join(HERE, "attn_window.npz")
    np.savez_compressed(path, prefill_rows=rows, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
