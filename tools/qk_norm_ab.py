#!/usr/bin/env python3
"""Qwen3's per-head QK-norm on the decode path, timed in ONE process on ONE box:
    python tools/qk_norm_ab.py [--bs 1,16,64] [--inner 100] [--rounds 30] [--no-model] [--out FILE]
(a) the fused launch (ops.gqa_qkv_norm_post: head norm + RoPE + K / V page append) against the composition it replaces --
    ops.rms_norm on the q heads, ops.rms_norm on the k heads (each on a reshaped copy of its strided slice, the result copied
    back into the merged row), then ops.gqa_qkv_post -- at 32 / 8 heads of 128.  Each side is captured as one hipGraph of
    `inner` back-to-back repetitions; the two graphs are replayed alternately `rounds` times and timed with device events.
    Reported: the median and the minimum per repetition, in microseconds.
(b) one decode step of a synthetic Qwen3-8B-shaped model (bench.measure: hipGraph replay, 1024 tokens of context) at bs 1 and
    16: recorded, not judged -- there is no earlier Qwen3 step to compare with.
One JSON line per measurement; --out also appends them to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chitu_amd import llama, ops  # noqa: E402

HQ, HKV, D, PAGE, EPS = 32, 8, 128, 256, 1e-6


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def capture(fn, inner):
    fn()  # warm: code objects loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


@torch.inference_mode()
def launch_ab(bs, inner, rounds, out):
    gen = torch.Generator(device="cuda").manual_seed(bs)
    qkv = torch.randn(bs, HQ + 2 * HKV, D, device="cuda", generator=gen).to(torch.bfloat16)
    q_w, k_w = ((1 + 0.1 * torch.randn(D, device="cuda", generator=gen)).to(torch.bfloat16) for _ in range(2))
    pages = 4 * bs
    k_cache, v_cache = (torch.zeros(pages, PAGE, HKV, D, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    table = torch.arange(pages, dtype=torch.int32, device="cuda").view(bs, 4).contiguous()
    lens = (torch.arange(bs, dtype=torch.int32, device="cuda") * 37 + 300) % (4 * PAGE)
    cos_t, sin_t = llama.precompute_freqs_cis(D, 4 * PAGE, 1e6)
    cos, sin = cos_t.cuda()[lens.long()].contiguous(), sin_t.cuda()[lens.long()].contiguous()
    a_buf, b_buf = qkv.clone(), qkv.clone()

    def fused():
        ops.gqa_qkv_norm_post(a_buf, HQ, HKV, cos, sin, k_cache, v_cache, table, lens, q_w, k_w, EPS, rotary_type="hf-llama")

    def composed():
        nq = ops.rms_norm(b_buf[:, :HQ].reshape(-1, D), q_w, EPS)
        nk = ops.rms_norm(b_buf[:, HQ:HQ + HKV].reshape(-1, D), k_w, EPS)
        b_buf[:, :HQ] = nq.view(bs, HQ, D)
        b_buf[:, HQ:HQ + HKV] = nk.view(bs, HKV, D)
        ops.gqa_qkv_post(b_buf, HQ, HKV, cos, sin, k_cache, v_cache, table, lens, rotary_type="hf-llama")

    # one repetition of each from the same row: the two compute the same thing (the sums of squares run in different orders,
    # so rr may differ in its last bit and a few bf16 values with it) before either is timed
    fused()
    ka = k_cache.clone()
    composed()
    torch.cuda.synchronize()
    for got, want in ((a_buf[:, :HQ], b_buf[:, :HQ]), (ka, k_cache)):
        err = ((got.float() - want.float()).abs().max() / want.float().abs().max()).item()
        assert err < 1e-2, ("fused launch != composition", err)
    graphs = {"fused": capture(fused, inner), "composed": capture(composed, inner)}
    times = {k: [] for k in graphs}
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    rec = {"what": "qk_norm launch A/B", "bs": bs, "heads": [HQ, HKV], "inner": inner, "rounds": rounds}
    for name, ts in times.items():
        rec[f"{name}_us_median"], rec[f"{name}_us_min"] = round(statistics.median(ts), 3), round(min(ts), 3)
    emit(rec, out)


@torch.inference_mode()
def model_steps(steps, warmup, out):
    import bench
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.qwen3 import Qwen3Args, Qwen3Decoder

    args, ctx = Qwen3Args(), 1024
    max_seq = ctx + steps + warmup + 512
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=16, block_size=256, max_seq_len=max_seq, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = Qwen3Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq), max_position_embeddings=max_seq,
                         device="cuda")
    llama.init_synthetic_(model, seed=3)
    cache.paged_k_cache.normal_(0, 0.5)
    cache.paged_v_cache.normal_(0, 0.5)
    for bs in (1, 16):
        dt = bench.measure(model, cache, bs, ctx, steps, warmup, 1, True, f"q{bs}_")
        emit({"what": "synthetic Qwen3-8B decode step", "bs": bs, "ctx": ctx, "steps": steps, "ms_per_step": round(dt / steps * 1e3, 4)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,16,64")
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    for bs in [int(b) for b in a.bs.split(",")]:
        launch_ab(bs, a.inner, a.rounds, a.out)
    if not a.no_model:
        model_steps(a.steps, a.warmup, a.out)


if __name__ == "__main__":
    main()
