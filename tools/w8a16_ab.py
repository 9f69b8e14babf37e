#!/usr/bin/env python3
"""A/B of the dense linears of one decode step: ops.bf16_linear against ops.w8a16_linear, and ops.bf16_linear_silu against
ops.w8a16_linear_silu (tools/moe_mxfp4_ab.py's method).

One process.  The four dense shapes of Llama-3-8B (wqkv 6144 x 4096, wo 4096 x 4096, w13 2 x 14336 x 4096, w2 4096 x 14336) and
of Qwen2-7B (wqkv 4608 x 3584, wo 3584 x 3584, w13 2 x 18944 x 3584, w2 3584 x 18944) at bs 1 and bs 16.  Each arm is one
hipGraph holding the launch for at least `--layers` different weight sets back to back -- as many as make the int8 sets alone
exceed 640 MB, beyond L2 + MALL, so every launch of either arm streams cold; after warm-up the two graphs are replayed
ALTERNATELY `--repeats` times, each replay timed with events.
Reported per arm: median us per launch, min / max, algorithmic weight bytes, achieved TB/s; then the time ratio int8 / bf16.
The yardstick is the bf16 launch in the same run: the int8 launch moves half the bytes and has to be faster at every shape.

--sweep T [T ...]: instead, the streaming form against the widen + tiled GEMM + scale_round form at T tokens (both forced)
on the Llama-3-8B shapes, beside what ops.w8a16_tiled picks (below chitu_hip_bf16_gemm's own tiled rule -- 128 tokens -- the GEMM
over the widened weights is itself the streaming one: that column then shows why the rule never goes there).  Also timed, each
in a graph of its own: the widen launch alone and the bf16 GEMM alone over widened weights with a bf16 output; tiled minus those
two is what the fp32 round trip and the scale_round launch cost -- the most a scale epilogue inside the tiled kernel could save
(for w13 the bf16 GEMM alone has no SiluAndMul, so the rest there includes it).
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
ap.add_argument("--sweep", type=int, nargs="+", default=[], help="token counts: streaming against tiled, both forced")
ap.add_argument("--out", type=str, default="")
a = ap.parse_args()

import torch  # noqa: E402

from chitu_amd import ops  # noqa: E402

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


def arms(name, x, bf, q, s, l):
    if name == "w13":
        return {"bf16": lambda: ops.bf16_linear_silu(x, bf[l]), "w8a16": lambda: ops.w8a16_linear_silu(x, q[l], s[l])}
    return {"bf16": lambda: ops.bf16_linear(x, bf[l]), "w8a16": lambda: ops.w8a16_linear(x, q[l], s[l])}


result = {"layers": a.layers, "shapes": {}, "sweep": {}}
slower = []
if not a.sweep:
    for model, shapes in MODELS.items():
        for name, (N, K) in shapes.items():
            L = max(a.layers, -(-(640 << 20) // (N * K)))  # the int8 sets of one replay alone exceed L2 + the 256 MB MALL
            bf, q, s = weights(N, K, L)
            for bs in a.bs:
                x = torch.randn(bs, K, device=dev, dtype=torch.bfloat16, generator=gen)
                graphs = {arm: graph_of([arms(name, x, bf, q, s, l)[arm] for l in range(L)]) for arm in ("bf16", "w8a16")}
                us = alternate(graphs, L)
                row = {"bf16": stats(us["bf16"], N * K * 2), "w8a16": stats(us["w8a16"], N * K + N * 4), "weight_sets": L,
                       "plan": ops.w8a16_plan(bs, N // 2 if name == "w13" else N, K, silu=name == "w13")["launches"]}
                row["time_ratio_w8a16_over_bf16"] = round(row["w8a16"]["median_us"] / row["bf16"]["median_us"], 4)
                row["faster"] = bool(row["w8a16"]["max_us"] < row["bf16"]["min_us"]) or row["time_ratio_w8a16_over_bf16"] < 1.0
                if row["time_ratio_w8a16_over_bf16"] >= 1.0:
                    slower.append(f"{model} {name} bs {bs}")
                result["shapes"][f"{model} {name} bs{bs}"] = row
                print(f"{model:10s} {name:4s} [{N:6d} x {K:5d}] bs {bs:2d}: bf16 {row['bf16']['median_us']:7.1f} us {row['bf16']['tb_per_s']:.2f} TB/s | "
                      f"w8a16 {row['w8a16']['median_us']:7.1f} us [{row['w8a16']['min_us']:.1f} .. {row['w8a16']['max_us']:.1f}] "
                      f"{row['w8a16']['tb_per_s']:.2f} TB/s | ratio {row['time_ratio_w8a16_over_bf16']:.3f}", flush=True)
            del bf, q, s, graphs
            torch.cuda.empty_cache()
    result["int8_not_faster_at"] = slower
    print("int8 launch faster than the bf16 launch at every shape:", "YES" if not slower else f"NO: {slower}")
else:
    rule = ops.w8a16_tiled
    for name, (N, K) in MODELS["llama3-8b"].items():
        L = 3
        bf, q, s = weights(N, K, L)
        del bf
        for T in a.sweep:
            x = torch.randn(T, K, device=dev, dtype=torch.bfloat16, generator=gen)
            picks = rule(T, N, K)
            graphs = {}
            for form in ("stream", "tiled"):
                ops.w8a16_tiled = (lambda M, n, k, _f=form: _f == "tiled")
                fn = ops.w8a16_linear_silu if name == "w13" else ops.w8a16_linear
                graphs[form] = graph_of([(lambda l=l: fn(x, q[l], s[l])) for l in range(L)])
            ops.w8a16_tiled = rule
            # what the tiled form is made of: the widen launch alone, and the bf16 GEMM alone over already-widened weights with a
            # bf16 output -- the floor of a scale epilogue inside the tiled kernel (no fp32 round trip, no scale_round launch)
            wide = [ops.w8a16_widen(q[l]) for l in range(L)]
            scratch = torch.empty_like(wide[0])
            graphs["widen"] = graph_of([(lambda l=l: ops.w8a16_widen(q[l], scratch)) for l in range(L)])
            graphs["bf16_gemm"] = graph_of([(lambda l=l: ops.bf16_linear(x, wide[l])) for l in range(L)])
            us = alternate(graphs, L)
            row = {f: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for f, v in us.items()}
            row["tiled_over_stream"] = round(row["tiled"]["median_us"] / row["stream"]["median_us"], 4)
            row["rule_picks"] = "tiled" if picks else "stream"
            row["fp32_round_trip_and_scale_round_us"] = round(row["tiled"]["median_us"] - row["widen"]["median_us"] - row["bf16_gemm"]["median_us"], 1)
            result["sweep"][f"{name} T{T}"] = row
            print(f"{name:4s} T {T:4d}: stream {row['stream']['median_us']:8.1f} us | tiled {row['tiled']['median_us']:8.1f} us | "
                  f"tiled / stream {row['tiled_over_stream']:.3f} | rule picks {row['rule_picks']} | widen {row['widen']['median_us']:.1f} us, "
                  f"bf16 GEMM alone {row['bf16_gemm']['median_us']:.1f} us, rest {row['fp32_round_trip_and_scale_round_us']:.1f} us", flush=True)
            del wide, scratch
        del q, s, graphs
        torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
