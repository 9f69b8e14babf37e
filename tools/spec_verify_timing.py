"""Device time of chitu_hip_speculative_verify next to chitu_hip_sample: bs 16 x T 4 = 64 rows of 129280 fp32
logits, peaked rows, temperature 0.8 / top-k 50 / top-p 0.9.  Each launch is captured `--launches` times back to back in a
hipGraph (device time, not the Python call overhead); the graphs are replayed alternately in one process and the per-launch
median, minimum and maximum over `--replays` rounds are printed and written as JSON.

  verify_accepted   every draft is its row's arg-max with u_acc = 0: the 48 draft rows return before the draw passes, the 16
                    bonus rows (draft -1) draw
  verify_rejected   every draft is a token outside the kept set: all 64 rows draw
  verify_rows_accepted  as verify_accepted with the arg-max as the draft of the bonus rows too (the entry allows a draft there, it
                    just does not count): no row draws -- the cost of an accepted row
  sample            chitu_hip_sample over the same 64 rows
  sample_parent     the same launch from another build of the library (--parent-lib), e.g. the parent commit's
  verify_accepted_parent / verify_rejected_parent   the two verify calls from that build

usage: python tools/spec_verify_timing.py [--parent-lib PATH] [--radix] [--out profiles/spec_verify_timing.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chitu_amd import _lib, sampling  # noqa: E402
from chitu_amd._lib import i32, i64, ptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--radix", action="store_true", help="force the radix descent (debug option sample_radix)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    bs, T, vocab = 16, 4, 129280
    rows = bs * T
    x = torch.randn(rows, vocab, generator=torch.Generator().manual_seed(2)).cuda() * 3.0
    temps = torch.full((rows,), 0.8, device="cuda")
    ks = torch.full((rows,), 50, dtype=torch.int32, device="cuda")
    ps = torch.full((rows,), 0.9, device="cuda")
    u1 = torch.rand(rows, device="cuda")
    u2 = torch.stack([torch.zeros(rows, device="cuda"), u1], dim=1).contiguous()
    best = x.argmax(dim=-1).to(torch.int32)
    worst = x.argmin(dim=-1).to(torch.int32)
    best_all = best.clone()
    best[T - 1 :: T] = -1
    worst[T - 1 :: T] = -1
    out_tok = torch.zeros(rows, dtype=torch.int64, device="cuda")
    out_par = torch.zeros(rows, dtype=torch.int64, device="cuda")
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None

    def sample_with(lib, out):
        _lib.check(lib.chitu_hip_sample(ptr(x), 2, i64(vocab), i64(rows), i32(vocab), ptr(temps), ptr(ks), ptr(ps), ptr(u1), i32(0),
                                        ptr(out), None, None, stream_ptr()), "sample")

    results = {}
    launches = {
        "verify_accepted": lambda: results.__setitem__("acc", sampling.speculative_verify(x, best, T, temps, ks, ps, uniforms=u2, return_rows=True)),
        "verify_rejected": lambda: results.__setitem__("rej", sampling.speculative_verify(x, worst, T, temps, ks, ps, uniforms=u2, return_rows=True)),
        "verify_rows_accepted": lambda: results.__setitem__("all", sampling.speculative_verify(x, best_all, T, temps, ks, ps, uniforms=u2, return_rows=True)),
        "sample": lambda: sample_with(_lib.lib(), out_tok),
    }
    if parent is not None:
        launches["sample_parent"] = lambda: sample_with(parent, out_par)
        par_out = {k: (torch.zeros(bs, T + 1, dtype=torch.int64, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda"),
                       torch.zeros(rows, dtype=torch.int64, device="cuda")) for k in ("acc", "rej")}

        def verify_parent(key, drafts):
            o, acc_o, tok_o = par_out[key]
            _lib.check(parent.chitu_hip_speculative_verify(ptr(x), 2, i64(vocab), i64(rows), i32(vocab), ptr(temps), ptr(ks), ptr(ps), ptr(drafts),
                                                           ptr(u2), i32(T), i32(0), ptr(o), ptr(acc_o), ptr(tok_o), stream_ptr()), "verify (parent)")

        launches["verify_accepted_parent"] = lambda: verify_parent("acc", best)
        launches["verify_rejected_parent"] = lambda: verify_parent("rej", worst)

    if a.radix:
        _lib.check(_lib.lib().chitu_hip_debug_option(i32(_lib.DEBUG_OPTIONS["sample_radix"]), i32(1)), "debug_option")
        if parent is not None:
            _lib.check(parent.chitu_hip_debug_option(i32(_lib.DEBUG_OPTIONS["sample_radix"]), i32(1)), "debug_option")
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
    acc, rej = results["acc"], results["rej"]
    assert int(acc[1].view(bs, T)[:, : T - 1].min()) == 1 and int(rej[1].max()) == 0
    assert int(acc[0][:, 0].min()) == T and int(rej[0][:, 0].max()) == 1 and int(results["all"][1].min()) == 1
    if parent is not None:
        assert torch.equal(out_tok, out_par), "chitu_hip_sample differs from the parent build's"
        for key in ("acc", "rej"):
            for mine, theirs in zip(results[key], par_out[key]):
                assert torch.equal(mine, theirs), "chitu_hip_speculative_verify differs from the parent build's"
    assert torch.equal(rej[2], out_tok), "a rejected draft outside the kept set leaves chitu_hip_sample's draw for u_alt"

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
           "path": "radix" if a.radix else "candidates", "launches_per_graph": a.launches, "replays": a.replays,
           "device": torch.cuda.get_device_name(0), "us_per_launch": {}}
    for name, ts in times.items():
        doc["us_per_launch"][name] = {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}
        print(f"{name:24s} median {statistics.median(ts):8.2f} us  (min {min(ts):.2f}, max {max(ts):.2f})")
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
