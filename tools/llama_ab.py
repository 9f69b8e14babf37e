#!/usr/bin/env python3
"""Step-time A/B of Llama-3-8B decode variants in ONE process on ONE box (model built once, a fresh hipGraph per variant):
    python tools/llama_ab.py [--steps 40] [--reps 2] [--bs 1,2,4]
Variants: the two add + RMSNorm launches of a layer as their own kernels (fuse 0) vs as the prologue of the GEMM behind
them (ops.bf16_linear_add_norm / bf16_linear_silu_add_norm), and any launch-variant overrides given as
--opt name=value (chitu_amd._lib.DEBUG_OPTIONS), each measured with and without the fusion.

    python tools/llama_ab.py --w8a16 [--bs 1,16] [--out FILE]
instead: the whole step of the bf16 decoder against the W8A16 one (quantize.quantize_w8a16_: int8 wqkv / wo / w13 / w2), each
(format, batch size) in a fresh child process under its own time limit, one after the other (this process never opens the
GPU); a child that fails ends the run.  Prints one JSON line per child and the step-time ratios."""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from chitu_amd import _lib, llama  # noqa: E402


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--bs", default="1")
    ap.add_argument("--opt", action="append", default=[], help="name=value launch-variant override, measured as its own variant")
    ap.add_argument("--w8a16", action="store_true", help="whole-step A/B of the bf16 and the W8A16 decoder, fresh child processes")
    ap.add_argument("--child-format", default="", help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.w8a16:
        rows = {}
        for bs in [int(b) for b in a.bs.split(",")]:
            for fmt in ("bf16", "w8a16"):
                cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child-format", fmt,
                       "--bs", str(bs), "--steps", str(a.steps), "--warmup", str(a.warmup), "--ctx", str(a.ctx)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                if res.returncode != 0 or not line:
                    print(res.stdout[-2000:], res.stderr[-2000:])
                    sys.exit(f"the {fmt} bs {bs} child ended with status {res.returncode}: nothing more is started")
                rows[f"{fmt} bs{bs}"] = json.loads(line[-1])
                print(line[-1], flush=True)
            rows[f"ratio_w8a16_over_bf16 bs{bs}"] = round(rows[f"w8a16 bs{bs}"]["ms_per_step"] / rows[f"bf16 bs{bs}"]["ms_per_step"], 4)
            print(f"bs {bs}: bf16 {rows[f'bf16 bs{bs}']['ms_per_step']} ms -> w8a16 {rows[f'w8a16 bs{bs}']['ms_per_step']} ms, ratio "
                  f"{rows[f'ratio_w8a16_over_bf16 bs{bs}']}", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager

    args = llama.LlamaArgs()
    max_seq = a.ctx + (a.steps + a.warmup) * 64 + 512
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=16, block_size=256, max_seq_len=max_seq, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = llama.LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq),
                               max_position_embeddings=max_seq, device="cuda")
    llama.init_synthetic_(model, seed=3)
    cache.paged_k_cache.normal_(0, 0.5)
    cache.paged_v_cache.normal_(0, 0.5)
    if a.child_format:
        if a.child_format == "w8a16":
            from chitu_amd.quantize import quantize_w8a16_

            quantize_w8a16_(model)
            torch.cuda.empty_cache()
        bs = int(a.bs)
        dt = bench.measure(model, cache, bs, a.ctx, a.steps, a.warmup, 1, True, "c_")
        weights = sum(p.numel() * p.element_size() for n, p in model.named_parameters() if ".attn.w" in n or ".ffn.w" in n)
        print(json.dumps({"format": a.child_format, "bs": bs, "ctx": a.ctx, "ms_per_step": round(dt / a.steps * 1e3, 4),
                          "layer_weight_GB": round(weights / 1e9, 3)}), flush=True)
        return
    variants = [("norm launches", 0, None), ("norm in GEMM prologue", 4, None)]
    for o in a.opt:
        name, val = o.split("=")
        variants += [(f"{o}, norm launches", 0, (name, int(val))), (f"{o}, norm in GEMM prologue", 4, (name, int(val)))]
    n = 0
    for bs in [int(b) for b in a.bs.split(",")]:
        for rep in range(a.reps):
            for label, fuse, opt in variants:
                llama.FUSE_NORM_MAX_BS = fuse
                model.graphs.clear()
                ctxm = _lib.debug_option(*opt) if opt else contextlib.nullcontext()
                with ctxm:
                    n += 1
                    dt = bench.measure(model, cache, bs, a.ctx, a.steps, a.warmup, 1, True, f"v{n}_")
                print(json.dumps({"bs": bs, "rep": rep, "variant": label, "ms_per_step": round(dt / a.steps * 1e3, 4)}), flush=True)


if __name__ == "__main__":
    main()
