"""Multi-token GQA paged decode (chitu_hip_gqa_decode_multi: T query tokens per sequence in one launch) against the only other way
to verify T draft tokens: the single-token kernel on bs * T expanded batch rows, each walking the same pages again.

  python tools/gqa_multi_sweep.py [--bs 1 16] [--ctx 1024 4096 8192 32768] [--T 2 4] [--parent-lib PATH] [--step] [--out FILE]

Llama-3-8B heads (32 q / 8 kv, head_dim 128: 4 query tokens per tile), 256-token pages, every sequence at the full context, both
cache formats, in the manner of tools/gqa_ctx_sweep.py: ONE process, the launch (+ merge) of each arm captured in a hipGraph of 20
back-to-back launches, the graphs replayed alternately after warm-up replays, so drift of the box hits all arms alike.  Before any
time is taken the multi launch's output is checked against the expanded launch's (attention bar, 1e-2 of the peak: the two are not
bit-identical, the rescale vote of a wave sees other tokens' columns); a shape that fails reports no times.  Per arm: median with
min .. max over the replays; then multi / expanded.  Each arm takes the split count attn_with_kvcache gives it by default.

  --parent-lib PATH: a build of the parent commit's library.  T = 1 through the existing single-token entry of THIS build and of that
  one, loaded side by side and alternated the same way: the existing kernels are the same code, so the ratio should be 1.
  --step: the whole Llama-3-8B step (synthetic weights, hipGraph): decode_multi at T = 4 against four decode steps, bs 1 and 16 at
  context 4096 -- the ratio that speculation has to beat with accepted tokens.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chitu_amd import _lib, ops  # noqa: E402
from chitu_amd._lib import f32, i32, i64, ptr, stream_ptr  # noqa: E402
from chitu_amd.attn_backend import HipAttnBackend, gqa_num_splits  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, nargs="*", default=[1, 16])
ap.add_argument("--ctx", type=int, nargs="*", default=[1024, 4096, 8192, 32768])
ap.add_argument("--T", type=int, nargs="*", default=[2, 4])
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--per-graph", type=int, default=20, help="launch sequences per captured graph")
ap.add_argument("--parent-lib", default=None, help="the parent commit's libchitu_hip.so: T = 1 through both builds")
ap.add_argument("--step", action="store_true", help="also the whole Llama-3-8B step: decode_multi(T = 4) against four decode steps")
ap.add_argument("--out", default=None)
a = ap.parse_args()

HQ, HKV, D, PAGE = 32, 8, 128, 256


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


def alternate(runs, per_replay):
    """{arm: graph or callable} run in turn -> {arm: [us per launch sequence]}"""
    out = {k: [] for k in runs}
    for it in range(a.warmup + a.repeats):
        for k, r in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.replay() if hasattr(r, "replay") else r()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return out


def stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "repeats": len(v)}


def ratio(row, num, den):
    """num / den of two arms' medians, and whether the difference exceeds the denominator arm's own min .. max spread"""
    return {"ratio": round(row[num]["median_us"] / row[den]["median_us"], 4),
            "difference_exceeds_spread": bool(abs(row[num]["median_us"] - row[den]["median_us"]) > row[den]["max_us"] - row[den]["min_us"])}


def randn_bf16(shape, g, chunk=64):
    out = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    for i in range(0, shape[0], chunk):
        out[i : i + chunk] = (torch.randn((min(chunk, shape[0] - i),) + tuple(shape[1:]), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    return out


def raw_single(lib, fp8, q3, kc, vc, table, lens, out, splits, ws):
    name = "chitu_hip_gqa_decode_kv_fp8" if fp8 else "chitu_hip_gqa_decode"
    rc = getattr(lib, name)(ptr(q3), i64(q3.stride(0)), i64(q3.stride(1)), ptr(kc), ptr(vc), i64(kc.shape[0]), i32(kc.shape[1]), i32(HKV),
                            ptr(table), i32(table.stride(0)), ptr(lens), f32(D ** -0.5), ptr(out), i32(q3.shape[0]), i32(HQ), i32(D),
                            i32(splits), ptr(ws), i64(ws.numel()), stream_ptr())
    assert rc == 0, (name, rc)


@torch.inference_mode()
def kernel_sweep():
    g = torch.Generator(device="cuda").manual_seed(0)
    be = HipAttnBackend(local_n_heads=HQ)
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    rows = []
    for bs in a.bs:
        for ctx in a.ctx:
            pages_per = ctx // PAGE + 1
            n_pages = bs * pages_per
            k16, v16 = randn_bf16((n_pages, PAGE, HKV, D), g), randn_bf16((n_pages, PAGE, HKV, D), g)
            k8 = ops.gqa_kv_quant_fp8(k16.view(-1, HKV, D)).view(n_pages, PAGE, HKV, -1)
            v8 = ops.gqa_kv_quant_fp8(v16.view(-1, HKV, D)).view(n_pages, PAGE, HKV, -1)
            table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(bs, pages_per)
            lens = torch.full((bs,), ctx, dtype=torch.int32, device="cuda")
            caches = {"bf16": (k16, v16), "fp8": (k8, v8)}
            if parent is not None:
                q1 = (torch.randn(bs, HQ, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
                splits = gqa_num_splits(bs, HKV, pages_per, PAGE)
                ws = torch.empty(max(bs * HQ * splits * (D + 1) * 4, 16), dtype=torch.uint8, device="cuda")
                for fmt, (kc, vc) in caches.items():
                    outs = {n: torch.empty(bs, HQ, D, dtype=torch.bfloat16, device="cuda") for n in ("this", "parent")}
                    libs = {"this": _lib.lib(), "parent": parent}
                    for n in libs:
                        raw_single(libs[n], fmt == "fp8", q1, kc, vc, table, lens, outs[n], splits, ws)
                    row = {"bs": bs, "ctx": ctx, "T": 1, "cache": fmt, "splits": splits,
                           "outputs_equal": bool(torch.equal(outs["this"].view(torch.int16), outs["parent"].view(torch.int16)))}
                    if row["outputs_equal"]:
                        gr = {n: capture(lambda n=n: raw_single(libs[n], fmt == "fp8", q1, kc, vc, table, lens, outs[n], splits, ws), a.per_graph)
                              for n in libs}
                        row.update({"single_" + k: stats(v) for k, v in alternate(gr, a.per_graph).items()})
                        row["this_over_parent"] = ratio(row, "single_this", "single_parent")
                        del gr
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            for T in a.T:
                q = (torch.randn(bs, T, HQ, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
                q_rows = q.view(bs * T, 1, HQ, D)
                lens_rows = (lens.view(bs, 1) - T + 1 + torch.arange(T, dtype=torch.int32, device="cuda")).view(bs * T).contiguous()
                table_rows = table.repeat_interleave(T, dim=0).contiguous()
                tiles = -(-T // (16 // (HQ // HKV)))
                for fmt, (kc, vc) in caches.items():
                    def multi():
                        return be.attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=table, causal=True)

                    def expanded():
                        return be.attn_with_kvcache(q_rows, kc, vc, cache_seqlens=lens_rows, block_table=table_rows)

                    m, e = multi().float().view(bs * T, HQ, D), expanded().float().view(bs * T, HQ, D)
                    err = float((m - e).abs().max() / e.abs().max())
                    row = {"bs": bs, "ctx": ctx, "T": T, "cache": fmt, "splits_multi": gqa_num_splits(bs * tiles, HKV, pages_per, PAGE),
                           "splits_expanded": gqa_num_splits(bs * T, HKV, pages_per, PAGE), "multi_vs_expanded_err_of_peak": round(err, 6)}
                    if err < 1e-2:  # no time is reported for a kernel that computes something else
                        gr = {"multi": capture(multi, a.per_graph), "expanded": capture(expanded, a.per_graph)}
                        row.update({k: stats(v) for k, v in alternate(gr, a.per_graph).items()})
                        row["multi_over_expanded"] = ratio(row, "multi", "expanded")
                        del gr
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del k16, v16, k8, v8, caches
            torch.cuda.empty_cache()
    return rows


@torch.inference_mode()
def step_sweep(ctx=4096, T=4, per=5):
    """Llama-3-8B, synthetic weights (bench.py's llama3_8b_extra): one decode_multi(T) replay against T decode replays"""
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.llama import LlamaArgs, LlamaDecoder, init_synthetic_

    args = LlamaArgs()
    max_seq = ctx + 512
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=16, block_size=256, max_seq_len=max_seq, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq), max_position_embeddings=max_seq, device="cuda")
    init_synthetic_(model, seed=3)
    cache.paged_k_cache.normal_(0, 0.5)
    cache.paged_v_cache.normal_(0, 0.5)
    rows = []
    for bs in (1, 16):
        reqs = [f"s{bs}_{i}" for i in range(bs)]
        for r in reqs:
            cache.register_sequence(r, ctx)
        tokens = torch.randint(100, 1000, (bs, T), device="cuda")
        # the lengths never advance: every replay rewrites the same rows and reads the same bytes
        cache.prepare_block_table_for_decode_multi(reqs, T)
        cache.prepare_cache_decode(reqs)
        cache.prepare_block_table_for_decode(reqs)
        model.decode_multi(tokens)
        model.decode(tokens[:, 0].contiguous())
        cols = [tokens[:, t].contiguous() for t in range(T)]

        def multi():
            for _ in range(per):
                model.decode_multi(tokens)

        def single():
            for _ in range(per):
                for c in cols:
                    model.decode(c)

        us = alternate({"decode_multi": multi, f"{T}_decode_steps": single}, per)
        row = {"model": "Llama-3-8B bf16, synthetic weights, hipGraph", "bs": bs, "ctx": ctx, "T": T}
        row.update({k: stats(v) for k, v in us.items()})
        row["multi_over_T_steps"] = ratio(row, "decode_multi", f"{T}_decode_steps")
        row["multi_over_one_step"] = round(row["decode_multi"]["median_us"] / (row[f"{T}_decode_steps"]["median_us"] / T), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        cache.finalize_cache_multi_decode(reqs, [1] * bs)  # returns the pages the multi step took
        for r in reqs:
            cache.finalize_cache_all_decode(r)
    return rows


def main():
    out = {"tool": "tools/gqa_multi_sweep.py", "device": torch.cuda.get_device_name(0), "heads": [HQ, HKV], "page": PAGE,
           "launch_sequences_per_graph": a.per_graph, "warmup_replays": a.warmup, "sweep": kernel_sweep()}
    if a.step:
        out["llama3_8b_step"] = step_sweep()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


main()
