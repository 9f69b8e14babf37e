"""GQA paged decode, bf16 K / V cache vs the fp8 cache (144-byte rows), over batch size and context.

  python tools/gqa_ctx_sweep.py [--bs 1 16 32] [--ctx 1024 4096 8192 32768] [--out profiles/gqa_kv_fp8_ctx_sweep.json]

Llama-3-8B heads (32 q / 8 kv, head_dim 128), 256-token pages, every sequence at the full context.  Both formats run in ONE
process: the fp8 caches hold the quantised rows of the bf16 arm's caches, the decode (+ merge) launch of each arm is captured in a
hipGraph of 20 back-to-back launches, and the graphs are replayed alternately (warm-up replays first), so drift of the box hits
both arms alike.  Before any time is taken, the fp8 arm's output is checked bit for bit against the bf16 kernel on the
DEQUANTISED fp8 cache at the same split count; a shape that fails the check reports no times.  Per arm: median with min .. max
over the replays, K + V bytes read, TB/s; then fp8 / bf16.  One launch sequence re-reads the same caches 20 times: at the
smallest shapes (bs 1, ctx 1024: 4 MB of bf16 rows) they stay in the last-level cache, and the figure is not an HBM rate.

  --window W: the same launches with window_size = (W, 0) (chitu_hip_gqa_decode_window / _kv_fp8_window) join the alternation as
two more arms per shape, after the windowed fp8 output is checked bit for bit against the windowed bf16 kernel on the dequantised
cache and the windowed bf16 output against the unwindowed kernel on the last W + 1 keys alone (attention bar, 1e-2 of the peak).
A windowed launch at context L reads the bytes the unwindowed launch reads at context W + 1: when the sweep also holds
ctx = W + 1, every windowed row reports its time over that row's unwindowed time of the same batch size and process.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chitu_amd import ops  # noqa: E402
from chitu_amd.attn_backend import HipAttnBackend, gqa_num_splits  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, nargs="*", default=[1, 16, 32])
ap.add_argument("--ctx", type=int, nargs="*", default=[1024, 4096, 8192, 32768])
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--per-graph", type=int, default=20, help="launch sequences per captured graph")
ap.add_argument("--window", type=int, default=None, help="also time the launches with window_size=(W, 0)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

HQ, HKV, D, PAGE = 32, 8, 128, 256
ROW16, ROW8 = HKV * D * 2, HKV * ops.GQA_KV_FP8_ROW  # bytes per token and cache


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


def randn_bf16(shape, g, chunk=64):
    """randn * 0.5 as bf16 without an fp32 temporary of the whole cache"""
    out = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    for i in range(0, shape[0], chunk):
        out[i : i + chunk] = (torch.randn((min(chunk, shape[0] - i),) + tuple(shape[1:]), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    return out


@torch.inference_mode()
def main():
    g = torch.Generator(device="cuda").manual_seed(0)
    be = HipAttnBackend(local_n_heads=HQ)
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
            q = (torch.randn(bs, 1, HQ, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
            new_k = torch.randn(bs, HKV, D, device="cuda", generator=g).to(torch.bfloat16)
            new_v = torch.randn(bs, HKV, D, device="cuda", generator=g).to(torch.bfloat16)
            old = lens - 1

            def decode(kc, vc, window=-1):
                return be.attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=table, window_size=(window, 0))

            dk, dv = ops.gqa_kv_dequant_fp8(k8), ops.gqa_kv_dequant_fp8(v8)
            same = torch.equal(decode(k8, v8).view(torch.int16), decode(dk, dv).view(torch.int16))
            W = a.window
            if W is not None:
                # the window's keys alone, as a sequence of its own: the last pages of every table row, the length cut to match
                w0 = max(0, ctx - 1 - W)
                cut = w0 // PAGE
                alone = be.attn_with_kvcache(q, dk, dv, cache_seqlens=lens - w0, block_table=table[:, cut:].contiguous()) if w0 % PAGE == 0 else None
                win = decode(dk, dv, W)
                same_w = torch.equal(decode(k8, v8, W).view(torch.int16), win.view(torch.int16))
                if alone is not None:
                    same_w = same_w and float((win.float() - alone.float()).abs().max() / alone.float().abs().max()) < 1e-2
                same = same and same_w
            del dk, dv
            row = {"bs": bs, "ctx": ctx, "splits": gqa_num_splits(bs, HKV, pages_per, PAGE),  # what decode() above was given
                   "kv_MB": {"bf16": round(2 * bs * ctx * ROW16 / 1e6, 2), "fp8": round(2 * bs * ctx * ROW8 / 1e6, 2)},
                   "fp8_equals_bf16_on_dequantised_cache": bool(same)}
            if W is not None:
                row.update(window=W, window_splits=gqa_num_splits(bs, HKV, pages_per, PAGE, W), window_keys=min(ctx, W + 1))
            if not same:  # no time is reported for a kernel that computes something else
                print(json.dumps(row), flush=True)
                rows.append(row)
                continue
            per = a.per_graph
            # the append graphs overwrite position ctx - 1 of the caches the decode graphs read: after the equality check above,
            # and a timed decode reads the same bytes whatever they hold
            graphs = {"bf16_decode": capture(lambda: decode(k16, v16), per), "fp8_decode": capture(lambda: decode(k8, v8), per),
                      "bf16_append": capture(lambda: (ops.append_to_paged_kv_cache(k16, table, new_k, old),
                                                      ops.append_to_paged_kv_cache(v16, table, new_v, old)), per),
                      "fp8_append": capture(lambda: ops.append_gqa_kv_fp8(k8, v8, table, new_k, new_v, old), per)}
            if W is not None:
                graphs["bf16_decode_window"] = capture(lambda: decode(k16, v16, W), per)
                graphs["fp8_decode_window"] = capture(lambda: decode(k8, v8, W), per)
            us = alternate(graphs, per)
            row.update({k: stats(v) for k, v in us.items()})
            for fmt, nbytes in (("bf16", 2 * bs * ctx * ROW16), ("fp8", 2 * bs * ctx * ROW8)):
                row[fmt + "_decode_TBs"] = round(nbytes / row[fmt + "_decode"]["median_us"] / 1e6, 3)
            row["fp8_over_bf16_decode"] = round(row["fp8_decode"]["median_us"] / row["bf16_decode"]["median_us"], 4)
            # a difference counts when it exceeds the bf16 arm's own min .. max spread
            row["difference_exceeds_bf16_spread"] = bool(
                abs(row["bf16_decode"]["median_us"] - row["fp8_decode"]["median_us"]) > row["bf16_decode"]["max_us"] - row["bf16_decode"]["min_us"])
            if W is not None:
                for fmt in ("bf16", "fp8"):
                    row[f"{fmt}_window_over_unwindowed_same_ctx"] = round(row[fmt + "_decode_window"]["median_us"] / row[fmt + "_decode"]["median_us"], 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del graphs, k16, v16, k8, v8
            torch.cuda.empty_cache()
    if a.window is not None:
        # windowed at ctx against unwindowed at ctx = W + 1 (the same bytes), same batch size, same process
        for row in rows:
            base = [r for r in rows if r["bs"] == row["bs"] and r["ctx"] == a.window + 1 and "bf16_decode" in r]
            if not base or "bf16_decode_window" not in row:
                continue
            for fmt in ("bf16", "fp8"):
                b, w = base[0][fmt + "_decode"], row[fmt + "_decode_window"]
                row[f"{fmt}_window_over_unwindowed_at_window_ctx"] = round(w["median_us"] / b["median_us"], 4)
                row[f"{fmt}_window_difference_exceeds_spread"] = bool(abs(w["median_us"] - b["median_us"]) > b["max_us"] - b["min_us"])
            print(json.dumps({k: v for k, v in row.items() if k in ("bs", "ctx", "splits", "window_splits") or "window_" in k}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/gqa_ctx_sweep.py", "device": torch.cuda.get_device_name(0), "heads": [HQ, HKV], "page": PAGE,
                       "launch_sequences_per_graph": a.per_graph, "warmup_replays": a.warmup, "window": a.window, "sweep": rows}, f, indent=1)
            f.write("\n")


main()
