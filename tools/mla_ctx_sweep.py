#!/usr/bin/env python3
"""MLA paged decode (chitu_hip_mla_decode + the fused merge / W_UV / quant launch) over the context length:
python tools/mla_ctx_sweep.py [bs=16] -> JSON lines {ctx, splits, decode_us, merge_us, kv_MB, decode_TBs, total_TBs}.
16 local heads (TP=8 rank of R1), 64-token pages, random latent cache; each launch pair is captured 50x in a
hipGraph and timed with events on the replay stream; kv bytes = bs * ctx * 576 * 2.

--fused: also the one-launch form chitu_hip_mla_decode_merge_uv_quant_fp8 (bf16 cache only), 50 launches captured in a hipGraph,
median of --repeats timed replays behind --warmup untimed ones, as fused_us (min ... max beside it).
--kv-format fp8: the same sweep over the fp8 latent cache (chitu_hip_mla_decode_kv_fp8; kv bytes = bs * ctx * 656).
--kv-format ab [--bs 1 16 32] [--out profiles/mla_kv_fp8_ctx_sweep.json]: both formats in ONE process -- the decode (+ merge)
launches of the bf16 and the fp8 cache, each captured 20x in a hipGraph, the two graphs replayed alternately; medians with
min ... max per arm, and the quantising append launch (ops.append_mla_kv_fp8, the launch the fp8 mode adds per layer) timed
the same way.  The fp8 cache holds the quantised rows of the bf16 arm's cache, so both arms attend over the same tokens.
--step CTX [CTX ...] [--step-bs 16] [--layers 61]: the whole decode step of the R1 rank shard (tools/moe_mxfp4_ab.py --step's
loop) with a bf16 and an fp8 cache, each format in a fresh child process; appended to --out under "whole_step".
--multi T [T ...] [--bs 1 16] [--ctx 1024 8192] [--out profiles/mla_multi_sweep.json]: the multi-token launch
(chitu_hip_mla_decode_multi / _kv_fp8, T query tokens per sequence, forced: kernel="multi") against the composition it replaces, chitu_hip_mla_decode on
bs * T expanded rows -- same process, both cache formats, each arm (launch + the merge / W_UV / quant launch on bs * T rows)
captured 20x in a hipGraph, the graphs replayed alternately; the outputs are checked equal at one split first.
--multi-step T [T ...] [--layers 61] [--step-ctx 1024]: the whole decode step of the R1 rank shard at bs 1, decode() against
decode_multi() at each T (its attention routed by the backend's rule), one process, the graph-replayed steps timed in alternating
rounds; under "multi_whole_step"."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("bs_pos", nargs="?", type=int, default=None, help="batch size (the original positional form)")
ap.add_argument("--kv-format", choices=("bf16", "fp8", "ab"), default="bf16")
ap.add_argument("--fused", action="store_true", help="default mode, bf16 cache: also time the fused decode + merge + W_UV + quant launch")
ap.add_argument("--bs", type=int, nargs="*", default=None)
ap.add_argument("--ctx", type=int, nargs="*", default=None, help="contexts (default 1024 4096 8192 32768; with --multi 1024 8192)")
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--step", type=int, nargs="*", default=None, help="contexts of the whole-step A/B (fresh child per format)")
ap.add_argument("--step-bs", type=int, default=16)
ap.add_argument("--layers", type=int, default=61)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--child-step", default=None, help=argparse.SUPPRESS)
ap.add_argument("--multi", type=int, nargs="*", default=None, help="query tokens per sequence of the multi-token launch A/B")
ap.add_argument("--multi-step", type=int, nargs="*", default=None, help="T values of the whole-step decode_multi vs decode timing (bs 1)")
ap.add_argument("--step-ctx", type=int, default=1024)
a = ap.parse_args()
if a.ctx is None:
    a.ctx = [1024, 8192] if a.multi else [1024, 4096, 8192, 32768]


def merge_into_out(key, value):
    if not a.out:
        return
    path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


if a.step is not None and a.child_step is None:
    whole = []
    for ctx in a.step:
        row = {"bs": a.step_bs, "ctx": ctx, "layers": a.layers}
        for fmt in ("bf16", "fp8"):  # a fresh process per format: no allocator state, graph pool or warmed cache shared
            cmd = [sys.executable, os.path.abspath(__file__), "--child-step", fmt, "--step", str(ctx), "--step-bs", str(a.step_bs),
                   "--layers", str(a.layers), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            print(f"whole step: bs {a.step_bs} ctx {ctx} {fmt} ...", flush=True)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"child {fmt} ctx {ctx} failed with {res.returncode}")
            row[fmt] = json.loads(res.stdout.strip().splitlines()[-1])
        row["ms_ratio_fp8_over_bf16"] = round(row["fp8"]["ms_per_step"] / row["bf16"]["ms_per_step"], 4)
        print(json.dumps(row), flush=True)
        whole.append(row)
    merge_into_out("whole_step", whole)
    sys.exit(0)

import torch  # noqa: E402

from chitu_amd import ops  # noqa: E402
from chitu_amd.attn_backend import HipAttnBackend  # noqa: E402

H, C, R = 16, 512, 64


def child_step(fmt, ctx):
    """ms per decode step of the R1 TP=8 rank shard (synthetic weights, random cache) with the cache in format `fmt`"""
    import time

    from chitu_amd import sampling
    from chitu_amd.cache_manager import PagedKVCacheManager, mla_kv_layout
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder, init_synthetic_

    torch.cuda.set_device(0)
    margs = DeepSeekV3Args(shard_degree=8, n_layers=a.layers, kv_cache_dtype=fmt)
    max_seq = ctx + 2 * (a.steps + a.warmup) + 256
    shape, dtype = mla_kv_layout(fmt, margs.kv_lora_rank, margs.qk_rope_head_dim)
    cache = PagedKVCacheManager(0, margs.n_layers, num_hot_req=a.step_bs, block_size=64, max_seq_len=max_seq, device="cuda",
                                kv_shape_per_sample=shape, dtype=dtype)
    model = DeepSeekV3Decoder(margs, cache, HipAttnBackend(local_n_heads=margs.n_heads // 8, max_seq_len=max_seq),
                              max_position_embeddings=max(max_seq, 4097), device="cuda")
    init_synthetic_(model, seed=1000)
    g = torch.Generator(device="cuda").manual_seed(77)
    for li in range(margs.n_layers):  # the same random rows in both formats
        layer = cache.paged_kv_cache[li]
        for p0 in range(0, layer.shape[0], 256):
            n = min(256, layer.shape[0] - p0)
            rows = torch.randn(n * 64, C + R, device="cuda", dtype=torch.bfloat16, generator=g) * 0.5
            if fmt == "fp8":
                ops.mla_kv_quant_fp8(rows, out=layer[p0:p0 + n].view(n * 64, -1))
            else:
                layer[p0:p0 + n].view(n * 64, -1).copy_(rows)
    reqs = [f"r{i}" for i in range(a.step_bs)]
    for r in reqs:
        cache.register_sequence(r, ctx)
    state = {"tokens": torch.randint(100, 1000, (a.step_bs,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))}

    def run(n):
        logits = None
        for _ in range(n):
            cache.prepare_cache_decode(reqs)
            cache.prepare_block_table_for_decode(reqs)
            logits = model.decode(state["tokens"], use_graph=True)
            state["tokens"] = sampling.argmax(logits)
            cache.finalize_cache_single_decode(reqs)
        return logits

    run(max(a.warmup, 4))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logits = run(a.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"kv_cache_dtype": fmt, "ms_per_step": round(dt / a.steps * 1e3, 4), "steps": a.steps,
                      "kv_cache_GB": round(cache.paged_kv_cache.numel() * cache.paged_kv_cache.element_size() / 1e9, 3),
                      "logits_finite": bool(torch.isfinite(logits).all())}))


def make_inputs(bs, ctx, g):
    pages_per = ctx // 64 + 1
    cache = (torch.randn(bs * pages_per, 64, C + R, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    table = torch.randperm(bs * pages_per, device="cuda", generator=g).to(torch.int32).view(bs, pages_per)
    lens = torch.full((bs,), ctx, dtype=torch.int32, device="cuda")
    q_nope = torch.randn(bs, H, C, device="cuda", generator=g).to(torch.bfloat16)
    q_pe = torch.randn(bs, H, R, device="cuda", generator=g).to(torch.bfloat16)
    return cache, table, lens, q_nope, q_pe


def capture(fn, n):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(n):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def alternate(graphs, per_replay):
    """{arm: graph} replayed in turn -> {arm: [us per launch sequence]}"""
    out = {k: [] for k in graphs}
    for it in range(a.warmup + a.repeats):
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return out


def stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "repeats": len(v)}


@torch.inference_mode()
def sweep_ab():
    g = torch.Generator(device="cuda").manual_seed(0)
    w_uv = (torch.randn(H, 128, C, device="cuda", generator=g) * 0.5).to(torch.float8_e4m3fn)
    sc = torch.rand(H * 2, C // 128, device="cuda", generator=g) * 0.02 + 0.01
    rows, per = [], 20
    for bs in (a.bs or [1, 16, 32]):
        for ctx in a.ctx:
            c16, table, lens, q_nope, q_pe = make_inputs(bs, ctx, g)
            c8 = ops.mla_kv_quant_fp8(c16.view(-1, C + R)).view(c16.shape[0], 64, -1)
            be = HipAttnBackend(local_n_heads=H, max_seq_len=ctx + 64)
            new_kv = torch.randn(bs, C + R, device="cuda", generator=g).to(torch.bfloat16)
            old = lens - 1

            def both(cache):
                o = be.mla_decode(q_nope, q_pe, cache, lens, table, 0.1, return_partials=True)
                if isinstance(o, tuple):
                    return ops.mla_merge_absorb_uv_quant_fp8(o[0], o[1], bs, w_uv, sc, 4, 8, 1)
                return ops.absorb_uv_quant_fp8(o, w_uv, sc, 4, 8, 1)

            same = all(torch.equal(x.view(torch.uint8) if x.element_size() == 1 else x, y.view(torch.uint8) if y.element_size() == 1 else y)
                       for x, y in zip(both(c8), both(ops.mla_kv_dequant_fp8(c8))))
            o = be.mla_decode(q_nope, q_pe, c16, lens, table, 0.1, return_partials=True)
            graphs = {"bf16_decode": capture(lambda: be.mla_decode(q_nope, q_pe, c16, lens, table, 0.1, return_partials=True), per),
                      "fp8_decode": capture(lambda: be.mla_decode(q_nope, q_pe, c8, lens, table, 0.1, return_partials=True), per),
                      "bf16_decode_merge": capture(lambda: both(c16), per), "fp8_decode_merge": capture(lambda: both(c8), per),
                      "fp8_append": capture(lambda: ops.append_mla_kv_fp8(c8, table, new_kv, old), per)}
            us = alternate(graphs, per)
            row = {"bs": bs, "ctx": ctx, "splits": o[1] if isinstance(o, tuple) else 1,
                   "kv_MB": {"bf16": round(bs * ctx * (C + R) * 2 / 1e6, 2), "fp8": round(bs * ctx * 656 / 1e6, 2)},
                   "fp8_equals_bf16_on_dequantised_cache": bool(same)}
            row.update({k: stats(v) for k, v in us.items()})
            for fmt, nbytes in (("bf16", bs * ctx * (C + R) * 2), ("fp8", bs * ctx * 656)):
                row[fmt + "_decode_TBs"] = round(nbytes / row[fmt + "_decode"]["median_us"] / 1e6, 3)
            row["fp8_over_bf16_decode"] = round(row["fp8_decode"]["median_us"] / row["bf16_decode"]["median_us"], 4)
            row["fp8_plus_append_over_bf16_decode_merge"] = round(
                (row["fp8_decode_merge"]["median_us"] + row["fp8_append"]["median_us"]) / row["bf16_decode_merge"]["median_us"], 4)
            # the criterion the MXFP4 work was held to: faster by more than the bf16 arm's own min ... max spread
            row["fp8_gain_exceeds_bf16_spread"] = bool(
                row["bf16_decode"]["median_us"] - row["fp8_decode"]["median_us"] > row["bf16_decode"]["max_us"] - row["bf16_decode"]["min_us"])
            print(json.dumps(row), flush=True)
            rows.append(row)
            del graphs, c16, c8
            torch.cuda.empty_cache()
    merge_into_out("sweep", rows)


@torch.inference_mode()
def sweep_one(bs, fmt):
    g = torch.Generator(device="cuda").manual_seed(0)
    w_uv = (torch.randn(H, 128, C, device="cuda", generator=g) * 0.5).to(torch.float8_e4m3fn)
    sc = torch.rand(H * 2, C // 128, device="cuda", generator=g) * 0.02 + 0.01
    for ctx in a.ctx:
        cache, table, lens, q_nope, q_pe = make_inputs(bs, ctx, g)
        if fmt == "fp8":
            cache = ops.mla_kv_quant_fp8(cache.view(-1, C + R)).view(cache.shape[0], 64, -1)
        be = HipAttnBackend(local_n_heads=H, max_seq_len=ctx + 64)

        def attn():
            return be.mla_decode(q_nope, q_pe, cache, lens, table, 0.1, return_partials=True)

        def both():
            o = attn()
            if isinstance(o, tuple):
                return ops.mla_merge_absorb_uv_quant_fp8(o[0], o[1], bs, w_uv, sc, 4, 8, 1)
            return ops.absorb_uv_quant_fp8(o, w_uv, sc, 4, 8, 1)

        res = {}
        o = attn()
        splits = o[1] if isinstance(o, tuple) else 1
        for name, fn in (("decode", attn), ("both", both)):
            gr = capture(fn, 50)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name] = e0.elapsed_time(e1) * 1e3 / 50
            del gr
        kv = bs * ctx * (656 if fmt == "fp8" else (C + R) * 2)
        row = {"bs": bs, "ctx": ctx, "splits": splits, "decode_us": round(res["decode"], 2),
               "merge_uv_quant_us": round(res["both"] - res["decode"], 2), "kv_MB": round(kv / 1e6, 1),
               "decode_TBs": round(kv / res["decode"] / 1e6, 3), "decode_plus_merge_TBs": round(kv / res["both"] / 1e6, 3),
               "frac_of_8TBs": round(kv / res["decode"] / 1e6 / 8, 3)}
        if fmt == "fp8":
            row["kv_format"] = "fp8"
        elif a.fused:
            def fused():
                return be.mla_decode_merge_uv_quant(q_nope, q_pe, cache, lens, table, 0.1, w_uv, sc, 4, 8, 1)

            if fused() is None:
                row["fused_us"] = None  # the shape takes the two-launch form (one split)
            else:
                us = alternate({"fused": capture(fused, 50)}, 50)["fused"]
                row.update({"fused_us": round(statistics.median(us), 2), "fused_min_us": round(min(us), 2), "fused_max_us": round(max(us), 2)})
        print(json.dumps(row), flush=True)
        del cache
        torch.cuda.empty_cache()


@torch.inference_mode()
def sweep_multi():
    g = torch.Generator(device="cuda").manual_seed(0)
    w_uv = (torch.randn(H, 128, C, device="cuda", generator=g) * 0.5).to(torch.float8_e4m3fn)
    sc = torch.rand(H * 2, C // 128, device="cuda", generator=g) * 0.02 + 0.01
    rows, per = [], 20
    for bs in (a.bs or [1, 16]):
        for ctx in a.ctx:
            c16, table, lens, _, _ = make_inputs(bs, ctx, g)
            c8 = ops.mla_kv_quant_fp8(c16.view(-1, C + R)).view(c16.shape[0], 64, -1)
            be = HipAttnBackend(local_n_heads=H, max_seq_len=ctx + 64)
            for T in a.multi:
                q_nope = torch.randn(bs, T, H, C, device="cuda", generator=g).to(torch.bfloat16)
                q_pe = torch.randn(bs, T, H, R, device="cuda", generator=g).to(torch.bfloat16)
                # the expanded problem: bs * T rows, each table row T times, lengths L - T + t + 1
                qn_x, qp_x = q_nope.view(bs * T, H, C), q_pe.view(bs * T, H, R)
                table_x = table.repeat_interleave(T, dim=0).contiguous()
                lens_x = (lens.view(bs, 1) - T + 1 + torch.arange(T, device="cuda", dtype=torch.int32).view(1, T)).reshape(-1).contiguous()

                def tail(o):
                    if isinstance(o, tuple):
                        return ops.mla_merge_absorb_uv_quant_fp8(o[0], o[1], bs * T, w_uv, sc, 4, 8, 1)
                    return ops.absorb_uv_quant_fp8(o.view(bs * T, H, C), w_uv, sc, 4, 8, 1)

                def multi(cache, partials=True):
                    return be.mla_decode_multi(q_nope, q_pe, cache, lens, table, 0.1, return_partials=partials, kernel="multi")

                def composed(cache, partials=True):
                    return be.mla_decode(qn_x, qp_x, cache, lens_x, table_x, 0.1, return_partials=partials,
                                         num_splits=None if partials else 1)

                row = {"bs": bs, "ctx": ctx, "T": T}
                for fmt, cache, nbytes in (("bf16", c16, (C + R) * 2), ("fp8", c8, 656)):
                    same = torch.equal(be.mla_decode_multi(q_nope, q_pe, cache, lens, table, 0.1, num_splits=1, kernel="multi").view(bs * T, H, C),
                                       composed(cache, partials=False))
                    om, oc = multi(cache), composed(cache)
                    graphs = {"multi": capture(lambda: multi(cache), per), "composed": capture(lambda: composed(cache), per),
                              "multi_tail": capture(lambda: tail(multi(cache)), per), "composed_tail": capture(lambda: tail(composed(cache)), per)}
                    us = alternate(graphs, per)
                    r = {k: stats(v) for k, v in us.items()}
                    r["equal_at_one_split"] = bool(same)
                    r["splits"] = {"multi": om[1] if isinstance(om, tuple) else 1, "composed": oc[1] if isinstance(oc, tuple) else 1}
                    r["kv_MB_read"] = {"multi": round(bs * ctx * nbytes * ((T + 1) // 2) / 1e6, 2), "composed": round(bs * ctx * nbytes * T / 1e6, 2)}
                    r["multi_over_composed"] = round(r["multi"]["median_us"] / r["composed"]["median_us"], 4)
                    r["multi_over_composed_with_tail"] = round(r["multi_tail"]["median_us"] / r["composed_tail"]["median_us"], 4)
                    row[fmt] = r
                    del graphs
                print(json.dumps(row), flush=True)
                rows.append(row)
            del c16, c8
            torch.cuda.empty_cache()
    merge_into_out("multi_sweep", rows)


@torch.inference_mode()
def multi_whole_step():
    """ms per step of the R1 TP=8 rank shard at bs 1: decode() and decode_multi() at each T of --multi-step, graph replays,
    alternating rounds in one process (synthetic weights, random bf16 cache)"""
    import time

    from chitu_amd.cache_manager import PagedKVCacheManager, mla_kv_layout
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder, init_synthetic_

    torch.cuda.set_device(0)
    margs = DeepSeekV3Args(shard_degree=8, n_layers=a.layers)
    rounds, per_round = 4, max(2, a.steps // 4)
    max_seq = a.step_ctx + (rounds + 2) * per_round * (1 + sum(a.multi_step)) + 256
    shape, dtype = mla_kv_layout("bf16", margs.kv_lora_rank, margs.qk_rope_head_dim)
    cache = PagedKVCacheManager(0, margs.n_layers, num_hot_req=1, block_size=64, max_seq_len=max_seq, device="cuda",
                                kv_shape_per_sample=shape, dtype=dtype)
    model = DeepSeekV3Decoder(margs, cache, HipAttnBackend(local_n_heads=margs.n_heads // 8, max_seq_len=max_seq),
                              max_position_embeddings=max(max_seq, 4097), device="cuda")
    init_synthetic_(model, seed=1000)
    cache.paged_kv_cache.copy_(torch.randn(cache.paged_kv_cache.shape, device="cuda", dtype=torch.bfloat16) * 0.5)
    reqs = ["r0"]
    cache.register_sequence(reqs[0], a.step_ctx)
    gt = torch.Generator(device="cuda").manual_seed(5)

    def run(T, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tok = torch.randint(100, 1000, (1, T), device="cuda", generator=gt)
            if T == 1:
                cache.prepare_cache_decode(reqs)
                cache.prepare_block_table_for_decode(reqs)
                model.decode(tok.view(1), use_graph=True)
                cache.finalize_cache_single_decode(reqs)
            else:
                cache.prepare_block_table_for_decode_multi(reqs, T)
                model.decode_multi(tok, use_graph=True)
                cache.finalize_cache_multi_decode(reqs, [T])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    Ts = [1] + list(a.multi_step)
    for T in Ts:
        run(T, 3)
    ms = {T: [] for T in Ts}
    for _ in range(rounds):
        for T in Ts:
            ms[T].append(run(T, per_round))
    res = {"bs": 1, "ctx": a.step_ctx, "layers": a.layers, "steps_per_round": per_round, "rounds": rounds,
           "note": "random tokens per step: T tokens route to up to T x 8 distinct experts per layer"}
    base = statistics.median(ms[1])
    for T in Ts:
        m = statistics.median(ms[T])
        res[f"T={T}"] = {"ms_per_step": round(m, 4), "min": round(min(ms[T]), 4), "max": round(max(ms[T]), 4),
                         "ms_per_token": round(m / T, 4), "step_over_T1": round(m / base, 4)}
    print(json.dumps(res), flush=True)
    merge_into_out("multi_whole_step", res)


if __name__ == "__main__":
    if a.multi_step:
        multi_whole_step()
    elif a.multi:
        sweep_multi()
    elif a.child_step:
        child_step(a.child_step, a.step[0])
    elif a.kv_format == "ab":
        sweep_ab()
    else:
        sweep_one(a.bs_pos if a.bs_pos is not None else (a.bs[0] if a.bs else 16), a.kv_format)
