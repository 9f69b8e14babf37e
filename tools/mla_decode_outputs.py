#!/usr/bin/env python3
"""MLA paged decode outputs of the loaded build over a fixed set of small cases, one sha256 per case and entry: run it once per
build (CHITU_HIP_LIB=<other build>) and diff the two listings -- a kernel rewrite that claims unchanged arithmetic must produce
the same listing.
    python tools/mla_decode_outputs.py > a.txt; CHITU_HIP_LIB=build_probe/lib_x.so python tools/mla_decode_outputs.py > b.txt; diff a.txt b.txt
All five entries: chitu_hip_mla_decode and _kv_fp8 (the fp8 cache holds the quantised rows of the bf16 one), _merge_uv_quant_fp8
(the quantised rows, their scales and the workspace partials), _multi and _multi_kv_fp8 (forced: kernel="multi") at q_len 1, 2,
3.  A split launch is hashed twice, its merged output and its workspace partials.  Cases: ragged lengths, an empty sequence, lengths around a tile
boundary (a pair's tokens on both sides of it; L < T, so that L_t <= 0), 5 and 16 heads, 64- and 128-token pages, 1 and 3 splits,
more splits than tiles, the default split count, batch 16 at whole tiles and one key past them, ragged thousands, and one sequence of 33,000 keys at 64-token pages -- at 2 splits the second
split starts at page 258, past the 256 table entries the bf16 kernel requests beside seqlens, with 258 tiles per split (below
kMaxTilesLds); at 1 split its 516 tiles take the per-tile table path."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chitu_amd import ops, workspace  # noqa: E402
from chitu_amd.attn_backend import HipAttnBackend  # noqa: E402

C, R, SCALE = 512, 64, 0.1352


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def run_case(tag, heads, page_size, lens_l, splits_l, q_lens=(1, 2, 3), seed=0):
    torch.manual_seed(seed)
    bs = len(lens_l)
    per = max(lens_l) // page_size + 2
    c16 = (torch.randn(bs * per, page_size, C + R, device="cuda") * 0.5).to(torch.bfloat16)
    c8 = ops.mla_kv_quant_fp8(c16.view(-1, C + R)).view(bs * per, page_size, -1)
    table = torch.randperm(bs * per, device="cuda").to(torch.int32).view(bs, per)
    lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
    w_uv = (torch.randn(heads, 128, C, device="cuda") * 0.5).to(torch.float8_e4m3fn)
    sc = torch.rand(heads * 2, C // 128, device="cuda") * 0.02 + 0.01
    be = HipAttnBackend(local_n_heads=heads, max_seq_len=max(lens_l) + 64)

    def both(name, call, rows, splits):
        """the merged output, and for a split launch the workspace partials as well"""
        line = f"{tag} {name} splits {splits}: out {sha(call(False))}"
        res = call(True)
        if isinstance(res, tuple):
            ws, S = res
            line += f" partials[{S}] {sha(ws[:rows * heads * S * (C * 2 + 4)])}"
        print(line, flush=True)

    for T in q_lens:
        qn = torch.randn(bs, T, heads, C, device="cuda").to(torch.bfloat16)
        qp = torch.randn(bs, T, heads, R, device="cuda").to(torch.bfloat16)
        for splits in splits_l:
            for fmt, cache in (("bf16", c16), ("fp8", c8)):
                if T == 1:
                    both(f"decode {fmt}", lambda p: be.mla_decode(qn[:, 0], qp[:, 0], cache, lens, table, SCALE, num_splits=splits,
                                                                  return_partials=p), bs, splits)
                both(f"multi T={T} {fmt}", lambda p: be.mla_decode_multi(qn, qp, cache, lens, table, SCALE, num_splits=splits,
                                                                        return_partials=p, kernel="multi"), bs * T, splits)
            if T == 1 and splits is not None and splits > 1:
                res = be.mla_decode_merge_uv_quant(qn[:, 0], qp[:, 0], c16, lens, table, SCALE, w_uv, sc, 4, 8, 1, num_splits=splits)
                ws = workspace.get(1, qn.device, "mla")  # the buffer the launch carved its partials from
                print(f"{tag} fused splits {splits}: q {sha(res[0])} scales {sha(res[1])} "
                      f"partials[{splits}] {sha(ws[:bs * heads * splits * (C * 2 + 4)])}", flush=True)
    torch.cuda.synchronize()


@torch.inference_mode()
def main():
    n = 0
    for heads in (16, 5):
        for page_size in (64, 128):
            for lens_l in ([63, 64, 65], [1000, 17, 0, 300], [64, 65, 66, 1, 2]):
                n += 1
                # 9 splits: more than the 1 .. 2 tiles of the short sequences (and than most of the others')
                run_case(f"heads {heads} page {page_size} lens {lens_l}", heads, page_size, lens_l, (None, 1, 3, 9), seed=n)
    # longer and wider: one key, whole tiles at batch 16, one key past a tile at batch 16, ragged thousands, 313 tiles beside 1
    for heads in (16, 5):
        for page_size in (64, 128):
            for lens_l in ([1], [1024] * 16, [1041] * 16, [5000, 4097, 64, 1], [20000, 3]):
                n += 1
                run_case(f"heads {heads} page {page_size} lens {lens_l[:4]}{'...' if len(lens_l) > 4 else ''}", heads, page_size, lens_l,
                         (None, 1, 3), q_lens=(1, 2), seed=n)
    # 33,000 keys: 516 tiles
    run_case("heads 16 page 64 lens [33000]", 16, 64, [33000], (1, 2), q_lens=(1, 2), seed=100)


if __name__ == "__main__":
    main()
