"""Device time of chitu_hip_speculative_verify_sampled next to chitu_hip_speculative_verify: bs 16 x T 8 = 128 rows of
129280 fp32 logits, peaked target rows and peaked draft rows, temperature 0.8 / top-k 50 / top-p 0.9.  Method of
tools/spec_verify_timing.py: each launch pair is captured `--launches` times back to back in a hipGraph, the graphs are replayed
alternately in one process, and the per-launch median, minimum and maximum over `--replays` rounds are printed and written as JSON.

  sampled_accepted / point_accepted   every draft is the target row's arg-max with u_acc = 0: the 112 draft rows accept, the 16
                                      bonus rows draw
  sampled_rejected / point_rejected   every draft is a token outside both kept sets: every row draws its replacement

Bytes read per pass over a row pair: 2 x 129280 x 4 = 1.03 MB by the new entry's pair passes (count, residual, rescan: one
segment of both rows per wave), 517 KB per pass of one row (the maxima, the radix levels, every pass of the point-mass entry).

usage: python tools/spec_verify_sampled_timing.py [--out profiles/spec_verify_sampled.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chitu_amd import sampling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    bs, T, vocab = 16, 8, 129280
    rows = bs * T
    x = torch.randn(rows, vocab, generator=torch.Generator().manual_seed(2)).cuda() * 3.0
    q = x + torch.randn(rows, vocab, generator=torch.Generator().manual_seed(3)).cuda() * 0.5
    temps = torch.full((rows,), 0.8, device="cuda")
    ks = torch.full((rows,), 50, dtype=torch.int32, device="cuda")
    ps = torch.full((rows,), 0.9, device="cuda")
    u2 = torch.stack([torch.zeros(rows, device="cuda"), torch.rand(rows, device="cuda")], dim=1).contiguous()
    best = x.argmax(dim=-1).to(torch.int32)
    worst = (x + q).argmin(dim=-1).to(torch.int32)
    best[T - 1 :: T] = -1
    worst[T - 1 :: T] = -1
    results = {}

    def sampled(name, d):
        return lambda: results.__setitem__(name, sampling.speculative_verify_sampled(x, q, d, T, temps, ks, ps, uniforms=u2, return_rows=True))

    def point(name, d):
        return lambda: results.__setitem__(name, sampling.speculative_verify(x, d, T, temps, ks, ps, uniforms=u2, return_rows=True))

    launches = {"sampled_accepted": sampled("sa", best), "point_accepted": point("pa", best),
                "sampled_rejected": sampled("sr", worst), "point_rejected": point("pr", worst)}
    graphs = {}
    for name, fn in launches.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.launches):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[name] = g
    for k in ("sa", "pa"):
        assert int(results[k][0][:, 0].min()) == T, k
    for k in ("sr", "pr"):
        assert int(results[k][1].max()) == 0, k

    times = {name: [] for name in graphs}
    for _ in range(a.replays):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches * 1e3)
    doc = {"rows": rows, "bs": bs, "T": T, "vocab": vocab, "dtype": "fp32", "temperature": 0.8, "top_k": 50, "top_p": 0.9,
           "launches_per_graph": a.launches, "replays": a.replays, "device": torch.cuda.get_device_name(0),
           "bytes_per_pass": {"pair_pass": 2 * vocab * 4, "single_row_pass": vocab * 4}, "us_per_launch": {}}
    for name, ts in times.items():
        doc["us_per_launch"][name] = {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}
        print(f"{name:18s} median {statistics.median(ts):8.2f} us  (min {min(ts):.2f}, max {max(ts):.2f})")
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
