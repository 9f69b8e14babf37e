#!/usr/bin/env python3
"""A/B of the routed-expert launch pair of one decode step: fp8 block-scaled experts (chitu_hip_moe_gemm1_silu_fp8 +
chitu_hip_moe_gemm2_quant_fp8) against MXFP4 experts (chitu_hip_moe_gemm1_silu_mxfp4 + chitu_hip_moe_gemm2_quant_mxfp4).

One process, DeepSeek-R1 TP=8 rank shapes (E = 257: 256 routed + the shared expert, I = 256, K = 7168, 8 routed + 1 shared
slot per token, balanced routing: every token picks 8 experts nobody else picks), bs 1 and bs 16.  Each arm is one hipGraph
holding the pair for `--layers` different weight sets back to back (one layer's experts are > 1 GB fp8 / > 0.7 GB MXFP4, far
beyond L2 + MALL, so every launch streams cold); after warm-up the two graphs are replayed ALTERNATELY `--repeats` times and
each replay is timed with events.  Reported per arm: median us per launch pair, min / max and the spread (max - min) over the
repeats, algorithmic weight bytes (weights + their scales of the distinct experts touched), achieved TB/s; then the time ratio
MXFP4 / fp8 beside the derived byte ratio, per-kernel medians from graphs of their own, and whether the requirement holds:
at bs 16 the MXFP4 pair is faster than the fp8 pair by more than the fp8 arm's measured spread.
Writes one JSON document (--out).  One GPU process; nothing else is started.

--step: instead, time a whole DeepSeek-R1 TP=8 rank-shard decode step (61 layers, bs 16, ctx 1024, greedy, hipGraph; bench.py's
workload) with fp8 and then with MXFP4 experts, each in a fresh child process under its own time limit, one after the other
(this process never opens the GPU); a child that fails ends the run.  The result is merged into --out under "whole_step".

--prefill T [T ...]: instead, the routed-expert launch sequence of one PREFILL call of T prompt tokens (fused_experts: align, quant,
GEMM1 + SiLU-and-mul, [quant of h,] GEMM2, top-k sum), same shapes (every token picks 8 random routed experts and the shared one), timed
three ways in one process: fp8 experts tiled (csrc/moe_tiled.hip), MXFP4 experts streaming (csrc/moe_mxfp4.hip, the 16-slot decode
kernels: CHITU_MOE_TILED_MIN_TOKENS=0) and MXFP4 experts tiled (csrc/moe_mxfp4_tiled.hip).  The form is FORCED per arm (the
per-expert slot floor of fused_moe._takes_tiled is lifted), and what the dispatch rule itself would pick at T is recorded beside
the times.  Each arm is one hipGraph of `--layers` calls on different weight sets (cold weights); the graphs are replayed alternately."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--step", action="store_true", help="time the whole rank-shard decode step for both expert formats (child processes)")
ap.add_argument("--child-step", type=str, default="", help=argparse.SUPPRESS)
ap.add_argument("--step-bs", type=int, default=16)
ap.add_argument("--step-ctx", type=int, default=1024)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--step-timeout", type=int, default=400, help="seconds per child")
ap.add_argument("--bs", type=int, nargs="+", default=[1, 16])
ap.add_argument("--layers", type=int, default=6, help="weight sets rotated through (each launch of a replay uses another one)")
ap.add_argument("--repeats", type=int, default=21)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--prefill", type=int, nargs="+", default=[], help="prompt token counts: time the prefill-sized expert sequence three ways")
ap.add_argument("--out", type=str, default="")
ap.add_argument("--opt", type=str, default="", help="launch-variant overrides for a sweep, e.g. moe_gemm1_wk=2,moe_gemm1_d=2 (both arms)")
a = ap.parse_args()

if a.step:
    import subprocess

    whole = {}
    for mode in ("fp8", "mxfp4"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child-step", mode,
               "--step-bs", str(a.step_bs), "--step-ctx", str(a.step_ctx), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not line:
            print(res.stdout[-2000:], res.stderr[-2000:])
            sys.exit(f"the {mode} step child ended with status {res.returncode}: nothing more is started")
        whole[mode] = json.loads(line[-1])
        print(mode, whole[mode], flush=True)
    whole["ms_ratio_mxfp4_over_fp8"] = round(whole["mxfp4"]["ms_per_step"] / whole["fp8"]["ms_per_step"], 4)
    print("whole step:", whole["fp8"]["ms_per_step"], "->", whole["mxfp4"]["ms_per_step"], "ms, ratio", whole["ms_ratio_mxfp4_over_fp8"])
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["whole_step"] = whole
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    sys.exit(0)

import torch  # noqa: E402

from chitu_amd import _lib, fused_moe  # noqa: E402
from chitu_amd._lib import f32, i32, i64, ptr, stream_ptr  # noqa: E402

def alternate_graphs(graphs, per_replay, warmup, repeats):
    """graphs: {arm: graph}; replays them in turn; returns {arm: [us per (replay / per_replay)]}."""
    out = {k: [] for k in graphs}
    for it in range(warmup + repeats):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return out


if a.child_step:
    import time

    from chitu_amd import sampling
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder, init_synthetic_

    torch.cuda.set_device(0)
    margs = DeepSeekV3Args(shard_degree=8, expert_dtype=a.child_step)
    max_seq = a.step_ctx + a.steps + a.warmup + 256
    cache = PagedKVCacheManager(0, margs.n_layers, num_hot_req=a.step_bs, block_size=64, max_seq_len=max_seq, device="cuda",
                                kv_shape_per_sample=(margs.kv_lora_rank + margs.qk_rope_head_dim,), dtype=torch.bfloat16)
    model = DeepSeekV3Decoder(margs, cache, HipAttnBackend(local_n_heads=margs.n_heads // 8, max_seq_len=max_seq),
                              max_position_embeddings=max(max_seq, 4097), device="cuda")
    init_synthetic_(model, seed=1000)
    g = torch.Generator(device="cuda").manual_seed(77)
    flat = cache.paged_kv_cache.view(-1)
    for i in range(0, flat.numel(), 1 << 26):
        n = min(1 << 26, flat.numel() - i)
        flat[i:i + n].copy_(torch.randn(n, device="cuda", dtype=torch.bfloat16, generator=g) * 0.5)
    reqs = [f"r{i}" for i in range(a.step_bs)]
    for r in reqs:
        cache.register_sequence(r, a.step_ctx)
    tokens = torch.randint(100, 1000, (a.step_bs,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))

    def run(n):
        global tokens
        for _ in range(n):
            cache.prepare_cache_decode(reqs)
            cache.prepare_block_table_for_decode(reqs)
            logits = model.decode(tokens, use_graph=True)
            tokens = sampling.argmax(logits)
            cache.finalize_cache_single_decode(reqs)
        return logits

    run(max(a.warmup, 4))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logits = run(a.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    experts = sum(p.numel() * p.element_size() for n, p in model.named_parameters() if ".ffn.w1w3_" in n or ".ffn.w2_" in n)
    print(json.dumps({"expert_dtype": a.child_step, "ms_per_step": round(dt / a.steps * 1e3, 4), "steps": a.steps, "bs": a.step_bs,
                      "ctx": a.step_ctx, "expert_bytes_GB": round(experts / 1e9, 2), "logits_finite": bool(torch.isfinite(logits).all())}))
    sys.exit(0)

if a.prefill:
    torch.cuda.set_device(0)
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    FP8 = torch.float8_e4m3fn
    E, K, I, TOPK, L = 257, 7168, 256, 9, a.layers

    def chunked(t, fill):
        flat = t.view(-1)
        for i in range(0, flat.numel(), 1 << 26):
            n = min(1 << 26, flat.numel() - i)
            flat[i:i + n].copy_(fill(n))
        return t

    rfp8 = lambda *sh: chunked(torch.empty(*sh, dtype=FP8, device=dev), lambda n: (torch.randn(n, device=dev, dtype=torch.bfloat16, generator=gen) * 0.5).to(FP8))
    ru8 = lambda lo, hi, *sh: torch.randint(lo, hi, sh, device=dev, generator=gen, dtype=torch.uint8)
    W8 = [(rfp8(E, 2 * I, K), torch.rand(E, 4, K // 128, device=dev, generator=gen) * 0.02 + 0.01,
           rfp8(E, K, I), torch.rand(E, K // 128, 2, device=dev, generator=gen) * 0.02 + 0.01) for _ in range(L)]
    W4 = [(ru8(0, 256, E, 2 * I, K // 2), ru8(118, 121, E, 2 * I, K // 32), ru8(0, 256, E, K, I // 2), ru8(118, 121, E, K, I // 32))
          for _ in range(L)]
    layer_bytes = {"fp8": sum(t.numel() * t.element_size() for t in W8[0]), "mxfp4": sum(t.numel() for t in W4[0])}
    result = {"shapes": {"E": E, "K": K, "I": I, "topk": TOPK, "layers": L, "block_m": fused_moe._MOE_TILED_BLOCK_M},
              "layer_weight_bytes": layer_bytes, "tokens": {}}
    defaults = (fused_moe._MOE_TILED_MIN_PER_EXPERT, fused_moe._MOE_TILED_MIN_TOKENS, fused_moe._MOE_MXFP4_TILED_MIN_TOKENS)

    def force(tiled):
        fused_moe._MOE_TILED_MIN_PER_EXPERT = 0
        fused_moe._MOE_TILED_MIN_TOKENS = fused_moe._MOE_MXFP4_TILED_MIN_TOKENS = 1 if tiled else 0

    for T in a.prefill:
        x = torch.randn(T, K, device=dev, dtype=torch.bfloat16, generator=gen) * 0.5
        ids = torch.stack([torch.randperm(E - 1, device=dev, generator=gen)[:TOPK - 1] for _ in range(T)])
        ids = torch.cat([ids, torch.full((T, 1), E - 1, device=dev)], 1).contiguous()
        wts = torch.rand(T, TOPK, device=dev, generator=gen).to(torch.bfloat16)

        def call(arm, l):
            if arm == "fp8_tiled":
                w1, s1, w2, s2 = W8[l]
                return lambda: fused_moe.fused_experts(x, w1, w2, wts, ids, use_fp8_w8a8=True, w1_scale=s1, w2_scale=s2, block_shape=[128, 128])
            w1, s1, w2, s2 = W4[l]
            return lambda: fused_moe.fused_experts(x, w1, w2, wts, ids, use_mxfp4_w4a8=True, w1_scale=s1, w2_scale=s2)

        graphs, outs = {}, {}
        for arm in ("fp8_tiled", "mxfp4_streaming", "mxfp4_tiled"):
            force(arm != "mxfp4_streaming")
            fns = [call(arm, l) for l in range(L)]
            outs[arm] = fns[0]().clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for f in fns:
                    f()
            g.replay()
            torch.cuda.synchronize()
            graphs[arm] = g
        fused_moe._MOE_TILED_MIN_PER_EXPERT, fused_moe._MOE_TILED_MIN_TOKENS, fused_moe._MOE_MXFP4_TILED_MIN_TOKENS = defaults
        us = alternate_graphs(graphs, L, a.warmup, a.repeats)
        row = {arm: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "repeats": len(v)}
               for arm, v in us.items()}
        same = (outs["mxfp4_tiled"].float() - outs["mxfp4_streaming"].float()).abs().max().item() / outs["mxfp4_streaming"].float().abs().max().item()
        row["tiled_vs_streaming_peak_rel_diff"] = same
        row["tiled_over_streaming"] = round(row["mxfp4_tiled"]["median_us"] / row["mxfp4_streaming"]["median_us"], 4)
        row["mxfp4_tiled_over_fp8_tiled"] = round(row["mxfp4_tiled"]["median_us"] / row["fp8_tiled"]["median_us"], 4)
        row["slots_per_expert"] = round(T * TOPK / E, 1)
        row["dispatch_rule_takes_tiled"] = bool(fused_moe._takes_tiled(T, T * TOPK, E, I, K, None, min_tokens=fused_moe._MOE_MXFP4_TILED_MIN_TOKENS))
        result["tokens"][str(T)] = row
        print(f"{T:5d} tokens: fp8 tiled {row['fp8_tiled']['median_us']:.1f} us | mxfp4 streaming {row['mxfp4_streaming']['median_us']:.1f} us | "
              f"mxfp4 tiled {row['mxfp4_tiled']['median_us']:.1f} us [{row['mxfp4_tiled']['min_us']:.1f} .. {row['mxfp4_tiled']['max_us']:.1f}] | "
              f"tiled / streaming {row['tiled_over_streaming']:.3f} | mxfp4 tiled / fp8 tiled {row['mxfp4_tiled_over_fp8_tiled']:.3f} | "
              f"rule picks {'tiled' if row['dispatch_rule_takes_tiled'] else 'streaming'} | outputs differ by {same:.1e} of the peak", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    sys.exit(0)

for kv in filter(None, a.opt.split(",")):
    k, v = kv.split("=")
    _lib.check(_lib.lib().chitu_hip_debug_option(i32(_lib.DEBUG_OPTIONS[k]), i32(int(v))), "debug_option")
    print(f"# override {k} = {v}")

torch.cuda.set_device(0)
dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
FP8 = torch.float8_e4m3fn
E, K, I, TOPK = 257, 7168, 256, 9
L = a.layers
lib = _lib.lib()


def rfp8(*shape):
    t = torch.empty(*shape, dtype=FP8, device=dev)
    flat = t.view(-1)
    for i in range(0, flat.numel(), 1 << 26):
        n = min(1 << 26, flat.numel() - i)
        flat[i:i + n].copy_((torch.randn(n, device=dev, dtype=torch.bfloat16, generator=gen) * 0.5).to(FP8))
    return t


def ru8(lo, hi, *shape):
    return torch.randint(lo, hi, shape, device=dev, generator=gen, dtype=torch.uint8)


w1_8 = [rfp8(E, 2 * I, K) for _ in range(L)]
w1_8s = [torch.rand(E, 4, K // 128, device=dev, generator=gen) * 0.02 + 0.01 for _ in range(L)]
w2_8 = [rfp8(E, K, I) for _ in range(L)]
w2_8s = [torch.rand(E, K // 128, 2, device=dev, generator=gen) * 0.02 + 0.01 for _ in range(L)]
w1_4 = [ru8(0, 256, E, 2 * I, K // 2) for _ in range(L)]
w1_4s = [ru8(118, 121, E, 2 * I, K // 32) for _ in range(L)]
w2_4 = [ru8(0, 256, E, K, I // 2) for _ in range(L)]
w2_4s = [ru8(118, 121, E, K, I // 32) for _ in range(L)]
BYTES = {
    "fp8": {"gemm1": 2 * I * K + 4 * (K // 128) * 4, "gemm2": K * I + (K // 128) * 2 * 4},
    "mxfp4": {"gemm1": 2 * I * K // 2 + 2 * I * K // 32, "gemm2": K * I // 2 + K * I // 32},
}


def graph_of(fns):
    for f in fns:
        rc = f()
        assert rc == 0, rc
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def alternate(graphs, per_replay):
    return alternate_graphs(graphs, per_replay, a.warmup, a.repeats)


def stats(us, nbytes):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread_us": round(max(us) - min(us), 2), "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e6, 3), "repeats": len(us)}


result = {"shapes": {"E": E, "K": K, "I": I, "topk": TOPK, "layers": L}, "derived_byte_ratio": round(
    (BYTES["mxfp4"]["gemm1"] + BYTES["mxfp4"]["gemm2"]) / (BYTES["fp8"]["gemm1"] + BYTES["fp8"]["gemm2"]), 4), "bs": {}}
for bs in a.bs:
    ids = (torch.arange(bs * 8, device=dev).view(bs, 8) % 256)
    ids = torch.cat([ids, torch.full((bs, 1), E - 1, device=dev)], 1).contiguous()
    distinct = int(ids.unique().numel())
    x = torch.randn(bs, K, device=dev, dtype=torch.bfloat16, generator=gen)
    xq, xs = fused_moe.per_token_group_quant_fp8(x, 128)
    sid, eid, npost = fused_moe.moe_align_block_size(ids, 16, E)
    numel = bs * TOPK
    mmb = min(eid.numel(), numel)
    wts = torch.rand(bs, TOPK, device=dev, generator=gen).to(torch.bfloat16)
    h = torch.empty(numel, I, dtype=torch.bfloat16, device=dev)
    c3 = torch.empty(numel, K, dtype=torch.bfloat16, device=dev)
    st = stream_ptr

    def g1(arm, l):
        if arm == "fp8":
            return lambda: lib.chitu_hip_moe_gemm1_silu_fp8(ptr(xq), ptr(xs), ptr(w1_8[l]), ptr(w1_8s[l]), ptr(sid), ptr(eid), ptr(npost),
                                                            ptr(h), i64(numel), i32(TOPK), i64(I), i64(K), i64(mmb), st())
        return lambda: lib.chitu_hip_moe_gemm1_silu_mxfp4(ptr(xq), ptr(xs), ptr(w1_4[l]), ptr(w1_4s[l]), ptr(sid), ptr(eid), ptr(npost),
                                                          ptr(h), i64(numel), i32(TOPK), i64(I), i64(K), i64(mmb), st())

    def g2(arm, l):
        if arm == "fp8":
            return lambda: lib.chitu_hip_moe_gemm2_quant_fp8(ptr(h), ptr(w2_8[l]), ptr(w2_8s[l]), ptr(sid), ptr(eid), ptr(npost), ptr(wts),
                                                             i32(0), i32(1), ptr(c3), i64(numel), i64(K), i64(I), i64(mmb), f32(1e-10), st())
        return lambda: lib.chitu_hip_moe_gemm2_quant_mxfp4(ptr(h), ptr(w2_4[l]), ptr(w2_4s[l]), ptr(sid), ptr(eid), ptr(npost), ptr(wts),
                                                           i32(0), i32(1), ptr(c3), i64(numel), i64(K), i64(I), i64(mmb), f32(1e-10), st())

    row = {"distinct_experts": distinct}
    pair = alternate({arm: graph_of([f for l in range(L) for f in (g1(arm, l), g2(arm, l))]) for arm in ("fp8", "mxfp4")}, L)
    for arm in ("fp8", "mxfp4"):
        row[arm] = {"pair": stats(pair[arm], distinct * (BYTES[arm]["gemm1"] + BYTES[arm]["gemm2"]))}
    for name, mk in (("gemm1", g1), ("gemm2", g2)):
        one = alternate({arm: graph_of([mk(arm, l) for l in range(L)]) for arm in ("fp8", "mxfp4")}, L)
        for arm in ("fp8", "mxfp4"):
            row[arm][name] = stats(one[arm], distinct * BYTES[arm][name])
    f8, m4 = row["fp8"]["pair"], row["mxfp4"]["pair"]
    row["time_ratio_mxfp4_over_fp8"] = round(m4["median_us"] / f8["median_us"], 4)
    row["gain_us"] = round(f8["median_us"] - m4["median_us"], 2)
    row["faster_by_more_than_fp8_spread"] = bool(f8["median_us"] - m4["median_us"] > f8["spread_us"])
    result["bs"][str(bs)] = row
    print(f"bs {bs:3d} ({distinct} experts): fp8 pair {f8['median_us']:.1f} us [{f8['min_us']:.1f} .. {f8['max_us']:.1f}] {f8['tb_per_s']:.2f} TB/s | "
          f"mxfp4 pair {m4['median_us']:.1f} us [{m4['min_us']:.1f} .. {m4['max_us']:.1f}] {m4['tb_per_s']:.2f} TB/s | time ratio "
          f"{row['time_ratio_mxfp4_over_fp8']:.3f} (bytes {result['derived_byte_ratio']:.3f}) | gemm1 {row['fp8']['gemm1']['median_us']:.1f} -> "
          f"{row['mxfp4']['gemm1']['median_us']:.1f}, gemm2 {row['fp8']['gemm2']['median_us']:.1f} -> {row['mxfp4']['gemm2']['median_us']:.1f}", flush=True)
if "16" in result["bs"]:
    result["requirement_met_at_bs16"] = result["bs"]["16"]["faster_by_more_than_fp8_spread"]
    print("requirement (bs 16: MXFP4 pair faster than the fp8 pair by more than the fp8 arm's spread):",
          "MET" if result["requirement_met_at_bs16"] else "NOT MET")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
