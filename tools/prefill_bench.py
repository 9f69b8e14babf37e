#!/usr/bin/env python3
"""Prefill timing of one TP=8 rank shard of DeepSeek-R1 FP8: python tools/prefill_bench.py [layers=8] [T ...]
One prompt of T tokens through `DeepSeekV3Decoder.prefill` (eager launches: absorb-mode MLA prefill kernel, fp8 GEMMs
that stream the weights once per 64 rows, fused MoE over T * 8 slots), T in {128, 512, 2048}; ms per layer and the
rank's tokens/s extrapolated to 61 layers.  Decode is the metric; this records where the step before it stands.

python tools/prefill_bench.py --paged-gqa [--heads HQ,HKV] [--layers 4] [--kernel-only] [--out FILE]: what the block table costs the GQA flash prefill, and what
continued prefill buys.  (1) Llama-3-8B heads (32 q / 8 kv), prefix 0, n = 2048 and 8192 new tokens, pages of 16 and
512 tokens in a shuffled pool: chitu_hip_gqa_prefill on the contiguous rows against chitu_hip_gqa_prefill_paged over the pages, in
ONE process, launches alternated after warm-up, 5 back-to-back launches per timed interval; the outputs are checked bit-identical
first.  (2) A Llama-3-8B-shaped stack of --layers layers with a 2048-token prefix cached: prefill_continue of 512 tokens against the
same 512 tokens as 64 decode_multi steps of 8 (graph replay), alternated, the cache rolled back in between.  Median [min .. max].
--heads HQ,HKV (default 32,8): the same at another head count, the stack's hidden size being 128 HQ (40,8 is Qwen3-14B,
24,8 Llama-3.2-3B, 28,4 Qwen2.5-7B).  At a group size that is no power of two the launches are chitu_ext4_gqa_prefill[_paged], and
part (1) has a third arm, the composition from the decode kernel (CHITU_GQA_PREFILL=compose: what ran for such a shape before
those entries existed; its output is checked against the flash kernel's at 1e-2 of the peak first).  ns_per_q_row: the flash
launch's median over the n * HQ live Q rows, the figure to compare across group sizes.

python tools/prefill_bench.py --paged-mla [--layers 4] [--kv bf16|fp8] [--kernel-only] [--flash-only] [--out FILE]: the same two
questions for DeepSeek-V3's continued prefill over the latent cache.  (1) 16 heads, (P, n) = (2048, 512), pages of 64
rows in a shuffled pool: the bare gather (chitu_ext2_mla_kv_gather), the bare flash launch with separate extents
(chitu_ext2_mla_prefill_flash_continue) and the two together (HipAttnBackend.mla_attn_varlen_with_kvcache) against
chitu_hip_mla_prefill_flash on one whole 2560-token sequence and on 2048 tokens, alternated in one process.  --flash-only: the two
whole-sequence launches alone, which any build of the library has -- run once per build (CHITU_HIP_LIB) to compare the kCont = false
instantiation with the kernel before the template.  (2) An R1-rank-shard-shaped stack of --layers layers with a 2048-token prefix
cached: prefill_continue of 512 tokens against 64 decode_multi steps of 8 (graph replay), alternated, the cache rolled back in between."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@torch.inference_mode()
def main():
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder, init_synthetic_

    layers = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    args = DeepSeekV3Args(shard_degree=8, n_layers=layers)
    cache = PagedKVCacheManager(0, layers, num_hot_req=2, block_size=64, max_seq_len=4096, device="cuda",
                                kv_shape_per_sample=(576,), dtype=torch.bfloat16)
    model = DeepSeekV3Decoder(args, cache, HipAttnBackend(local_n_heads=16, max_seq_len=4096), max_position_embeddings=4097,
                              device="cuda")
    init_synthetic_(model, seed=1)
    g = torch.Generator().manual_seed(0)
    for T in [int(a) for a in sys.argv[2:]] or (128, 512, 2048):
        prompt = torch.randint(100, 1000, (T,), generator=g).tolist()
        times = []
        for rep in range(3):
            rid = f"p{T}_{rep}"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.prefill([prompt], [rid])
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            cache.finalize_cache_all_decode(rid)
        best = min(times[1:])
        print(json.dumps({"prompt_tokens": T, "layers": layers, "ms": round(best * 1e3, 2), "ms_per_layer": round(best * 1e3 / layers, 3),
                          "rank_tok_s_at_61_layers": round(T / (best / layers * 61), 1)}), flush=True)


def _alternate(arms, warmup, repeats, per):
    """{name: callable} run in turn -> {name: [us per call]}; `per` back-to-back calls per timed interval"""
    out = {k: [] for k in arms}
    for it in range(warmup + repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per)
    return out


def _stats(v):
    import statistics

    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "repeats": len(v)}


def _box():
    import subprocess

    try:
        res = subprocess.run(["rocm-smi", "-d", "0", "--showuniqueid"], capture_output=True, text=True, timeout=10)
        ids = [ln.split(":")[-1].strip() for ln in res.stdout.splitlines() if ln.strip().startswith("GPU[")]
        return ids[0] if ids else f"no answer (rc {res.returncode})"
    except Exception as exc:  # noqa: BLE001
        return f"unavailable: {type(exc).__name__}"


@torch.inference_mode()
def paged_gqa_main():
    import argparse

    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.llama import LlamaArgs, LlamaDecoder, init_synthetic_

    ap = argparse.ArgumentParser()
    ap.add_argument("--paged-gqa", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--heads", default="32,8", help="HQ,HKV")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="part (1) only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [{"box": _box(), "device": torch.cuda.get_device_name(0)}]
    print(json.dumps(rows[0]), flush=True)
    Hq, Hkv = (int(x) for x in a.heads.split(","))
    G = Hq // Hkv
    with_compose = (G & (G - 1)) != 0 and G <= 16  # (the decode kernel, which the composition runs, stops at G = 16)
    be = HipAttnBackend(local_n_heads=Hq, max_seq_len=8192)
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (2048, 8192):
        q = (torch.randn(n, Hq, 128, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        k = torch.randn(n, Hkv, 128, device="cuda", generator=g).to(torch.bfloat16)
        v = torch.randn(n, Hkv, 128, device="cuda", generator=g).to(torch.bfloat16)
        cu = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        lens = torch.tensor([n], dtype=torch.int32, device="cuda")
        for page in (16, 512):
            pages = n // page
            perm = torch.randperm(pages + 3, device="cuda", generator=g)[:pages]
            kc = torch.zeros(pages + 3, page, Hkv, 128, dtype=torch.bfloat16, device="cuda")
            vc = torch.zeros_like(kc)
            kc[perm], vc[perm] = k.view(pages, page, Hkv, 128), v.view(pages, page, Hkv, 128)
            table = perm.to(torch.int32).view(1, pages).contiguous()
            arms = {"contiguous": lambda: be.attn_varlen_func(q, k, v, cu, cu, n, n, causal=True),
                    "paged": lambda: be.attn_varlen_with_kvcache(q, kc, vc, cu, lens, table, n)}
            if not torch.equal(arms["contiguous"](), arms["paged"]()):
                rows.append({"n": n, "page": page, "error": "outputs differ: no times"})
                print(json.dumps(rows[-1]), flush=True)
                continue
            if with_compose and page == 16:  # (the composition stages its own pages: one page size is enough)
                def compose():
                    os.environ["CHITU_GQA_PREFILL"] = "compose"
                    try:
                        return be.attn_varlen_func(q, k, v, cu, cu, n, n, causal=True)
                    finally:
                        del os.environ["CHITU_GQA_PREFILL"]

                want = arms["contiguous"]().float()
                err = float((compose().float() - want).abs().max() / want.abs().max())
                if not err < 1e-2:
                    rows.append({"n": n, "page": page, "error": f"composition and flash kernel differ by {err:.3e} of the peak: no times"})
                    print(json.dumps(rows[-1]), flush=True)
                    continue
                arms["compose"] = compose
            t = {k_: _stats(v_) for k_, v_ in _alternate(arms, a.warmup, a.repeats, 5).items()}
            rows.append({"what": "kernel", "Hq": Hq, "Hkv": Hkv, "prefix": 0, "n": n, "page": page, **t,
                         "paged_over_contiguous": round(t["paged"]["median_us"] / t["contiguous"]["median_us"], 4),
                         "ns_per_q_row": round(t["contiguous"]["median_us"] * 1e3 / (n * Hq), 4)})
            if "compose" in t:
                rows[-1]["compose_over_flash"] = round(t["compose"]["median_us"] / t["contiguous"]["median_us"], 3)
            print(json.dumps(rows[-1]), flush=True)
            del kc, vc
    if a.kernel_only:
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    # (2) the model path: 512 tokens onto a cached 2048-token prefix
    args = LlamaArgs(n_layers=a.layers, n_heads=Hq, n_kv_heads=Hkv, dim=128 * Hq)
    cache = PagedKVCacheManager(0, a.layers, num_hot_req=1, block_size=256, max_seq_len=4096, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=128, dtype=torch.bfloat16)
    model = LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=4096), max_position_embeddings=4096, device="cuda")
    init_synthetic_(model, seed=1)
    gc = torch.Generator().manual_seed(0)
    prompt = torch.randint(100, 1000, (2048,), generator=gc).tolist()
    tail = torch.randint(100, 1000, (512,), generator=gc)
    model.prefill([prompt], ["r"])
    steps = tail.view(64, 1, 8).cuda()

    def continued():
        model.prefill_continue([tail.tolist()], ["r"])
        cache.rollback(["r"], [512])

    def multi_steps():
        for i in range(64):
            cache.prepare_block_table_for_decode_multi(["r"], 8)
            model.decode_multi(steps[i], use_graph=True)
            cache.finalize_cache_multi_decode(["r"], [8])
        cache.rollback(["r"], [512])

    t = {k_: _stats(v_) for k_, v_ in _alternate({"prefill_continue_512": continued, "decode_multi_64x8": multi_steps}, 2, 7, 1).items()}
    rows.append({"what": "model", "Hq": Hq, "Hkv": Hkv, "layers": a.layers, "prefix": 2048, "new_tokens": 512, **t,
                 "continue_over_multi": round(t["prefill_continue_512"]["median_us"] / t["decode_multi_64x8"]["median_us"], 4)})
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


@torch.inference_mode()
def paged_mla_main():
    import argparse
    import dataclasses

    from chitu_amd import ops
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, mla_kv_layout
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder, init_synthetic_

    ap = argparse.ArgumentParser()
    ap.add_argument("--paged-mla", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="part (1) only")
    ap.add_argument("--flash-only", action="store_true", help="the whole-sequence launches of part (1) only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [{"box": _box(), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("CHITU_HIP_LIB") or "in-tree"}]
    print(json.dumps(rows[0]), flush=True)
    H, P, n, page, scale = 16, 2048, 512, 64, 0.1352
    L = P + n
    be = HipAttnBackend(local_n_heads=H, max_seq_len=4096)
    g = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(L, H, 576, device="cuda", generator=g) * 0.3).to(torch.bfloat16)
    kv = torch.randn(L, 1, 576, device="cuda", generator=g).to(torch.bfloat16)

    def whole(T):
        cu = torch.tensor([0, T], dtype=torch.int32, device="cuda")
        return lambda: be.attn_varlen_func(q[:T], kv[:T], kv[:T, :, :512], cu, cu, T, T, causal=True, softmax_scale=scale)

    arms = {"whole_2560": whole(L), "whole_2048": whole(2048)}
    if not a.flash_only:
        pages = L // page
        perm = torch.randperm(pages + 3, device="cuda", generator=g)[:pages]
        pool = torch.zeros(pages + 3, page, 576, dtype=torch.bfloat16, device="cuda")
        pool[perm] = kv.view(pages, page, 576)
        if a.kv == "fp8":
            pool = ops.mla_kv_quant_fp8(pool.view(-1, 576)).view(pages + 3, page, -1)
        table = perm.to(torch.int32).view(1, pages).contiguous()
        lens = torch.tensor([L], dtype=torch.int32, device="cuda")
        cu_q = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        cu_k = torch.tensor([0, L], dtype=torch.int32, device="cuda")
        qn = q[P:].contiguous()
        buf = torch.empty(L, 576, dtype=torch.bfloat16, device="cuda")
        both = lambda: be.mla_attn_varlen_with_kvcache(qn, pool, cu_q, lens, table, n, L, scale, gathered=buf)  # noqa: E731
        got, want = both(), arms["whole_2560"]()[P:]
        if a.kv == "bf16" and not torch.equal(got, want):  # P = 2048 is a multiple of 8: every row sits in a whole block
            rows.append({"error": "continued rows differ from the whole-sequence call: no times"})
            print(json.dumps(rows[-1]), flush=True)
            return
        from chitu_amd import _lib
        from chitu_amd._lib import f32, i32, i64, ptr, stream_ptr

        out = torch.empty(n, H, 512, dtype=torch.bfloat16, device="cuda")
        arms.update({
            "gather": lambda: ops.mla_kv_gather(pool, table, cu_k, L, out=buf),
            "flash_continue": lambda: _lib.check(_lib.lib().chitu_ext2_mla_prefill_flash_continue(
                ptr(qn), i64(qn.stride(0)), i64(qn.stride(1)), ptr(buf), i64(576), ptr(cu_q), ptr(cu_k), i32(1), i32(n), f32(scale),
                ptr(out), i32(H), i32(512), i32(64), stream_ptr()), "flash_continue"),
            "gather+flash_continue": both})
    t = {k_: _stats(v_) for k_, v_ in _alternate(arms, a.warmup, a.repeats, 5).items()}
    rows.append({"what": "kernel", "heads": H, "prefix": P, "n": n, "page": page, "kv": a.kv, **t})
    if not a.flash_only:
        rows[-1]["continued_over_whole_2560"] = round(t["gather+flash_continue"]["median_us"] / t["whole_2560"]["median_us"], 4)
    print(json.dumps(rows[-1]), flush=True)
    if not (a.kernel_only or a.flash_only):
        # (2) the model path: 512 tokens onto a cached 2048-token prefix
        args = dataclasses.replace(DeepSeekV3Args(shard_degree=8, n_layers=a.layers), kv_cache_dtype=a.kv)
        shape, dtype = mla_kv_layout(a.kv)
        cache = PagedKVCacheManager(0, a.layers, num_hot_req=1, block_size=64, max_seq_len=4096, device="cuda",
                                    kv_shape_per_sample=shape, dtype=dtype)
        model = DeepSeekV3Decoder(args, cache, HipAttnBackend(local_n_heads=16, max_seq_len=4096), max_position_embeddings=4097,
                                  device="cuda")
        init_synthetic_(model, seed=1)
        gc = torch.Generator().manual_seed(0)
        prompt = torch.randint(100, 1000, (P,), generator=gc).tolist()
        tail = torch.randint(100, 1000, (n,), generator=gc)
        model.prefill([prompt], ["r"])
        steps = tail.view(64, 1, 8).cuda()

        def continued():
            model.prefill_continue([tail.tolist()], ["r"])
            cache.rollback(["r"], [n])

        def multi_steps():
            for i in range(64):
                cache.prepare_block_table_for_decode_multi(["r"], 8)
                model.decode_multi(steps[i], use_graph=True)
                cache.finalize_cache_multi_decode(["r"], [8])
            cache.rollback(["r"], [n])

        t = {k_: _stats(v_) for k_, v_ in _alternate({"prefill_continue_512": continued, "decode_multi_64x8": multi_steps}, 2, 7, 1).items()}
        rows.append({"what": "model", "layers": a.layers, "kv": a.kv, "prefix": P, "new_tokens": n, **t,
                     "continue_over_multi": round(t["prefill_continue_512"]["median_us"] / t["decode_multi_64x8"]["median_us"], 4)})
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    if "--paged-mla" in sys.argv:
        paged_mla_main()
    elif "--paged-gqa" in sys.argv:
        paged_gqa_main()
    else:
        main()
