"""bf16 experts at prefill sizes: the 16-slot streaming grouped GEMMs (csrc/moe_bf16.hip) against the tiled ones
(csrc/moe_bf16_tiled.hip), same process, alternating, cold weights -- the measurement behind chitu_amd.qwen3_moe.TILED_MIN_TOKENS.

    python tools/moe_bf16_ab.py --prefill 128 256 384 512 1024 2048 8192 [--out profiles/moe_bf16_tiled_ab.json]

Shapes default to one Qwen3-30B-A3B layer: E = 128, top 8, K = 2048, I = 768 (1.2 GB of expert weights).  Each arm is one
hipGraph of `--layers` fused_experts calls on different weight sets (together beyond L2 + MALL, so every call streams its
weights cold); after warm-up the two graphs are replayed ALTERNATELY `--repeats` times and the per-call medians compared
(tools/moe_mxfp4_ab.py --prefill's method).  Then, per arm, the recorded GEMM1 and GEMM2 launches of those calls are replayed on
their own (one graph per entry, same weight rotation) for the split of the time.  Reported beside the times: the fraction of
the 2.5 PFLOP/s dense bf16 peak the two GEMMs reach, and the HBM bytes each form has to move AS COMPUTED FROM THE SHAPES AND
THE ROUTING (not from counters): weights of every expert that holds a token once per m-block of the form (16 slots streaming,
`block_m` tiled) plus activations in and out.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--prefill", type=int, nargs="+", default=[128, 256, 384, 512, 1024, 2048, 8192], help="prompt token counts")
ap.add_argument("--experts", type=int, default=128)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--hidden", type=int, default=2048)
ap.add_argument("--inter", type=int, default=768)
ap.add_argument("--layers", type=int, default=3, help="weight sets rotated through (each call of a replay uses another one)")
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", type=str, default="")
a = ap.parse_args()

import torch  # noqa: E402

from chitu_amd import _lib, fused_moe  # noqa: E402
from chitu_amd._lib import stream_ptr  # noqa: E402

PEAK_BF16 = 2.5e15
G1 = {"tiled": "chitu_ext3_moe_gemm1_silu_bf16_tiled", "streaming": "chitu_hip_moe_gemm_bf16"}
G2 = {"tiled": "chitu_ext3_moe_gemm2_bf16_tiled", "streaming": "chitu_hip_moe_gemm_bf16"}


def timed_replays(graphs, per_replay, warmup, repeats):
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


def graph_of(fns):
    for f in fns:  # one eager pass: workspaces exist before the capture
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def summary(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "repeats": len(v)}


torch.cuda.set_device(0)
dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
E, K, I, TOPK, L = a.experts, a.hidden, a.inter, a.topk, a.layers
BLOCK_M = fused_moe._MOE_TILED_BLOCK_M


def rbf16(scale, *shape):
    t = torch.empty(*shape, dtype=torch.bfloat16, device=dev)
    flat = t.view(-1)
    for i in range(0, flat.numel(), 1 << 26):
        n = min(1 << 26, flat.numel() - i)
        flat[i:i + n].copy_(torch.randn(n, device=dev, dtype=torch.bfloat16, generator=gen) * scale)
    return t


W = [(rbf16(K ** -0.5, E, 2 * I, K), rbf16(I ** -0.5, E, K, I)) for _ in range(L)]
layer_bytes = sum(t.numel() * t.element_size() for t in W[0])
result = {"shapes": {"E": E, "K": K, "I": I, "topk": TOPK, "layers": L, "block_m": BLOCK_M}, "layer_weight_bytes": layer_bytes,
          "peak_bf16_flops": PEAK_BF16, "hbm_bytes_are": "computed from the shapes and the routing, not from counters", "tokens": {}}
keep_floor = fused_moe._MOE_TILED_MIN_PER_EXPERT
fused_moe._MOE_TILED_MIN_PER_EXPERT = 0  # forced forms: the per-expert floor is part of what is being measured

for T in a.prefill:
    x = torch.randn(T, K, device=dev, dtype=torch.bfloat16, generator=gen) * 0.5
    ids = torch.stack([torch.randperm(E, device=dev, generator=gen)[:TOPK] for _ in range(T)]).contiguous()
    wts = torch.rand(T, TOPK, device=dev, generator=gen).to(torch.bfloat16)
    numel = T * TOPK
    counts = torch.bincount(ids.reshape(-1), minlength=E).tolist()
    flops1, flops2 = 2.0 * numel * 2 * I * K, 2.0 * numel * K * I
    act_bytes = T * K * 2 + 2 * numel * I * 2 + numel * K * 2  # x in, h out and in again, per-slot outputs
    per_expert = 3 * I * K * 2
    hbm = {"algorithmic": sum(per_expert for c in counts if c) + act_bytes,
           "streaming": sum(per_expert * -(-c // 16) for c in counts) + act_bytes,
           "tiled": sum(per_expert * -(-c // BLOCK_M) for c in counts) + act_bytes}

    def call(arm, l):
        w1, w2 = W[l]
        floor = 1 if arm == "tiled" else 0
        return lambda: fused_moe.fused_experts(x, w1, w2, wts, ids, bf16_tiled_min_tokens=floor)

    graphs, outs, entries = {}, {}, {}
    for arm in ("streaming", "tiled"):
        fns = [call(arm, l) for l in range(L)]
        outs[arm] = fns[0]().clone()
        _lib.call_log_ctypes = []
        try:
            for f in fns:
                f()
            entries[arm] = list(_lib.call_log_ctypes)
        finally:
            _lib.call_log_ctypes = None
        graphs[arm] = graph_of(fns)
    us = timed_replays(graphs, L, a.warmup, a.repeats)
    row = {arm: summary(v) for arm, v in us.items()}

    # the split: each arm's recorded GEMM launches on their own, behind one whole replay of that arm (its h, its sorted ids)
    lib = _lib._lib  # the plain CDLL: these replays are not recorded again
    for arm in ("streaming", "tiled"):
        gemms = [(n, args) for n, args in entries[arm] if n in (G1[arm], G2[arm])]
        assert len(gemms) == 2 * L, (arm, [n for n, _ in entries[arm]])
        first, second = gemms[0::2], gemms[1::2]  # per call: GEMM1, then GEMM2
        graphs[arm].replay()
        torch.cuda.synchronize()
        replay = lambda n, args: (lambda: _lib.check(getattr(lib, n)(*args[:-1], stream_ptr()), n))
        parts = {"gemm1": graph_of([replay(n, args) for n, args in first]), "gemm2": graph_of([replay(n, args) for n, args in second])}
        for part, v in timed_replays(parts, L, a.warmup, a.repeats).items():
            row[arm][part] = summary(v)
        t1, t2 = row[arm]["gemm1"]["median_us"] * 1e-6, row[arm]["gemm2"]["median_us"] * 1e-6
        row[arm]["gemm1_fraction_of_peak"] = round(flops1 / t1 / PEAK_BF16, 4)
        row[arm]["gemm2_fraction_of_peak"] = round(flops2 / t2 / PEAK_BF16, 4)
        row[arm]["hbm_bytes"] = hbm[arm]
        row[arm]["hbm_GBps_over_both_gemms"] = round(hbm[arm] / (t1 + t2) / 1e9, 1)
    diff = (outs["tiled"].float() - outs["streaming"].float()).abs().max().item() / outs["streaming"].float().abs().max().item()
    row["tiled_vs_streaming_peak_rel_diff"] = diff
    row["tiled_over_streaming"] = round(row["tiled"]["median_us"] / row["streaming"]["median_us"], 4)
    row["slots_per_expert"] = round(numel / E, 1)
    row["hbm_bytes_algorithmic"] = hbm["algorithmic"]
    result["tokens"][str(T)] = row
    s, t = row["streaming"], row["tiled"]
    print(f"{T:5d} tokens ({row['slots_per_expert']:6.1f} slots/expert): streaming {s['median_us']:8.1f} us [{s['min_us']:.1f} .. {s['max_us']:.1f}] "
          f"(g1 {s['gemm1']['median_us']:.1f} + g2 {s['gemm2']['median_us']:.1f}, {hbm['streaming'] / 1e9:.2f} GB) | tiled {t['median_us']:8.1f} us "
          f"[{t['min_us']:.1f} .. {t['max_us']:.1f}] (g1 {t['gemm1']['median_us']:.1f} = {t['gemm1_fraction_of_peak']:.3f} of peak + g2 "
          f"{t['gemm2']['median_us']:.1f} = {t['gemm2_fraction_of_peak']:.3f}, {hbm['tiled'] / 1e9:.2f} GB) | tiled / streaming "
          f"{row['tiled_over_streaming']:.3f} | outputs differ by {diff:.1e} of the peak", flush=True)

fused_moe._MOE_TILED_MIN_PER_EXPERT = keep_floor
# the smallest measured T from which the tiled form wins at every larger measured T (0: it never does)
floor = 0
for T in sorted(a.prefill, reverse=True):
    if result["tokens"][str(T)]["tiled_over_streaming"] < 1.0:
        floor = T
    else:
        break
result["floor"] = floor
print("smallest measured token count from which the tiled form wins at every larger one:", floor or "none (0)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
