#!/usr/bin/env python3
"""A/B of the dense linears of one decode step in three weight formats: ops.bf16_linear, ops.w8a16_linear and ops.w4a16_linear
(w13: the *_linear_silu launches), tools/w8a16_ab.py's method.

One process.  The four dense shapes of Llama-3-8B and of Qwen2-7B at bs 1 and bs 16.  Each arm is one hipGraph holding the launch
for as many different weight sets back to back as make the int4 sets alone exceed 640 MB, beyond L2 + MALL, so every launch of
every arm streams cold; after warm-up the three graphs are replayed ALTERNATELY `--repeats` times, each replay timed with events.
Reported per arm: median us per launch, min / max, algorithmic weight bytes, achieved TB/s; then the time ratios against bf16 and
-- the bar of the int4 launch -- against W8A16.  Every shape is recorded, faster or not.
Then the whole Llama-3-8B decode step (synthetic weights, ctx 1024, graph replay, bench.py's measure) per format at the same
batch sizes, the three decoders built one after the other.

--sweep T [T ...]: instead, the streaming form against the widen + tiled bf16 GEMM form at T tokens (both forced) on the
Llama-3-8B shapes, beside what ops.w4a16_tiled picks.
Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, nargs="+", default=[1, 16])
ap.add_argument("--layers", type=int, default=4, help="weight sets rotated through (each launch of a replay uses another one)")
ap.add_argument("--repeats", type=int, default=21)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--step-steps", type=int, default=40, help="decode steps of the whole-step measurement (0: skip it)")
ap.add_argument("--sweep", type=int, nargs="+", default=[], help="token counts: streaming against tiled, both forced")
ap.add_argument("--out", type=str, default="")
a = ap.parse_args()

import torch  # noqa: E402

from chitu_amd import ops  # noqa: E402
from chitu_amd.quantize import pack_w4a16  # noqa: E402

MODELS = {
    "llama3-8b": {"wqkv": (6144, 4096), "wo": (4096, 4096), "w13": (2 * 14336, 4096), "w2": (4096, 14336)},
    "qwen2-7b": {"wqkv": (4608, 3584), "wo": (3584, 3584), "w13": (2 * 18944, 3584), "w2": (3584, 18944)},
}
torch.cuda.set_device(0)
dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)


def weights(N, K, L):
    bf = [(torch.randn(N, K, device=dev, dtype=torch.bfloat16, generator=gen) * K ** -0.5) for _ in range(L)]
    q = [torch.randint(-127, 128, (N, K), device=dev, generator=gen, dtype=torch.int8) for _ in range(L)]
    s = [torch.rand(N, device=dev, generator=gen) * 1e-3 + 1e-4 for _ in range(L)]
    return bf, q, s


def weights4(N, K, L, halves):
    out = []
    for _ in range(L):
        u = torch.randint(0, 16, (N, K), device=dev, generator=gen, dtype=torch.uint8)
        out.append(pack_w4a16(u, torch.rand(N, K // 128, device=dev, generator=gen) * 1e-2 + 1e-3, halves=halves))
    return out


def graph_of(fns):
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def alternate(graphs, per_replay):
    out = {k: [] for k in graphs}
    for it in range(a.warmup + a.repeats):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return out


def stats(us, nbytes):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "bytes": nbytes,
            "tb_per_s": round(nbytes / med / 1e6, 3), "repeats": len(us)}


def arms(name, x, bf, q, s, p4, l):
    if name == "w13":
        return {"bf16": lambda: ops.bf16_linear_silu(x, bf[l]), "w8a16": lambda: ops.w8a16_linear_silu(x, q[l], s[l]),
                "w4a16": lambda: ops.w4a16_linear_silu(x, *p4[l])}
    return {"bf16": lambda: ops.bf16_linear(x, bf[l]), "w8a16": lambda: ops.w8a16_linear(x, q[l], s[l]),
            "w4a16": lambda: ops.w4a16_linear(x, *p4[l])}


def whole_step(fmt, bs):
    """ms per decode step of Llama-3-8B in one format: a fresh decoder, bench.py's measure under graph replay."""
    import bench
    from chitu_amd import llama
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.quantize import quantize_w4a16_, quantize_w8a16_

    args, ctx, warm = llama.LlamaArgs(), 1024, 5
    max_seq = ctx + (a.step_steps + warm) * 64 + 512
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=16, block_size=256, max_seq_len=max_seq, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = llama.LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq),
                               max_position_embeddings=max_seq, device="cuda")
    llama.init_synthetic_(model, seed=3)
    cache.paged_k_cache.normal_(0, 0.5)
    cache.paged_v_cache.normal_(0, 0.5)
    if fmt != "bf16":
        {"w8a16": quantize_w8a16_, "w4a16": quantize_w4a16_}[fmt](model)
        torch.cuda.empty_cache()
    out = {}
    for b in bs:
        model.graphs.clear()
        out[b] = round(bench.measure(model, cache, b, ctx, a.step_steps, warm, 1, True, f"{fmt}{b}_") / a.step_steps * 1e3, 4)
    return out


result = {"layers": a.layers, "shapes": {}, "sweep": {}, "whole_step_ms": {}}
slower = []
if not a.sweep:
    for model, shapes in MODELS.items():
        for name, (N, K) in shapes.items():
            L = max(a.layers, -(-(640 << 20) // (N * K // 2)))  # the int4 sets of one replay alone exceed L2 + the 256 MB MALL
            bf, q, s = weights(N, K, L)
            p4 = weights4(N, K, L, 2 if name == "w13" else 1)
            nbytes = {"bf16": N * K * 2, "w8a16": N * K + N * 4, "w4a16": N * K // 2 + p4[0][1].numel() * 4}
            for bs in a.bs:
                x = torch.randn(bs, K, device=dev, dtype=torch.bfloat16, generator=gen)
                graphs = {arm: graph_of([arms(name, x, bf, q, s, p4, l)[arm] for l in range(L)]) for arm in nbytes}
                us = alternate(graphs, L)
                row = {arm: stats(us[arm], nbytes[arm]) for arm in nbytes}
                row["weight_sets"] = L
                row["plan"] = ops.w4a16_plan(bs, N // 2 if name == "w13" else N, K, silu=name == "w13")["launches"]
                for arm, base in (("w8a16", "bf16"), ("w4a16", "bf16"), ("w4a16", "w8a16")):
                    row[f"time_ratio_{arm}_over_{base}"] = round(row[arm]["median_us"] / row[base]["median_us"], 4)
                if row["time_ratio_w4a16_over_w8a16"] >= 1.0:
                    slower.append(f"{model} {name} bs {bs}")
                result["shapes"][f"{model} {name} bs{bs}"] = row
                print(f"{model:10s} {name:4s} [{N:6d} x {K:5d}] bs {bs:2d}: " + " | ".join(
                    f"{arm} {row[arm]['median_us']:7.1f} us [{row[arm]['min_us']:.1f} .. {row[arm]['max_us']:.1f}] {row[arm]['tb_per_s']:.2f} TB/s"
                    for arm in nbytes) + f" | w4/bf16 {row['time_ratio_w4a16_over_bf16']:.3f} w8/bf16 {row['time_ratio_w8a16_over_bf16']:.3f} "
                    f"w4/w8 {row['time_ratio_w4a16_over_w8a16']:.3f}", flush=True)
            del bf, q, s, p4, graphs
            torch.cuda.empty_cache()
    result["int4_not_faster_than_int8_at"] = slower
    print("int4 launch faster than the W8A16 launch at every shape:", "YES" if not slower else f"NO: {slower}")
    if a.step_steps:
        for fmt in ("bf16", "w8a16", "w4a16"):
            result["whole_step_ms"][fmt] = whole_step(fmt, a.bs)
            torch.cuda.empty_cache()
            print(f"Llama-3-8B whole step, {fmt}: " + ", ".join(f"bs {b} {ms} ms" for b, ms in result["whole_step_ms"][fmt].items()), flush=True)
else:
    rule = ops.w4a16_tiled
    for name, (N, K) in MODELS["llama3-8b"].items():
        L = 3
        p4 = weights4(N, K, L, 2 if name == "w13" else 1)
        for T in a.sweep:
            x = torch.randn(T, K, device=dev, dtype=torch.bfloat16, generator=gen)
            picks = rule(T, N, K)
            graphs = {}
            for form in ("stream", "tiled"):
                ops.w4a16_tiled = (lambda M, n, k, _f=form: _f == "tiled")
                fn = ops.w4a16_linear_silu if name == "w13" else ops.w4a16_linear
                graphs[form] = graph_of([(lambda l=l: fn(x, *p4[l])) for l in range(L)])
            ops.w4a16_tiled = rule
            us = alternate(graphs, L)
            row = {f: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for f, v in us.items()}
            row["tiled_over_stream"] = round(row["tiled"]["median_us"] / row["stream"]["median_us"], 4)
            row["rule_picks"] = "tiled" if picks else "stream"
            result["sweep"][f"{name} T{T}"] = row
            print(f"{name:4s} T {T:4d}: stream {row['stream']['median_us']:8.1f} us | tiled {row['tiled']['median_us']:8.1f} us | "
                  f"tiled / stream {row['tiled_over_stream']:.3f} | rule picks {row['rule_picks']}", flush=True)
        del p4, graphs
        torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
