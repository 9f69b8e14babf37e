"""Same-process A/B of the partial-rotary decode launch (include/chitu_hip_ext7.h) against the full-width one it stands beside,
GLM-4-9B's 32 / 2 heads, bf16 K / V pages, bs 1 and 16, by tools/qkv_bias_ab.py's method:

  ext7_R64      chitu_ext7_gqa_qkv_bias_post, rotary_dim 64, layout 0 (GLM-4's launch)
  ext5          chitu_ext5_gqa_qkv_bias_post, layout 0 (the same kernel at the full width; every other model's launch)
  ext5@NAME     --other-lib NAME=PATH (repeatable): the same entry of another build of the library, loaded beside this one -- the
                parent commit's build shows what this tree costs the models that do not use the width; a byte-for-byte COPY of
                this tree's own build is the control: what it reads against `ext5` is the method's own bias between two loaded
                libraries, and only a difference beyond it means anything

Each arm is a hipGraph of `--per` back-to-back launches on one stream; after warm-up the arms' graphs are replayed in turn
`--repeats` times, the order rotated by one arm every round, every replay between two events.  Reported per arm: median
[min .. max] microseconds per launch.  One JSON line per batch size; --out writes them all, with the GPU's unique id, into one file.

    python tools/glm4_rope_ab.py --out profiles/glm4_rope_ab.json [--other-lib parent=path/to/libchitu_hip.so ...]
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.qkv_bias_ab import _box, _graph_of  # noqa: E402

HQ, HKV, D, PAGE, R = 32, 2, 128, 16, 64
BF16 = torch.bfloat16


def _rotating(arms, warmup, repeats, per):
    """tools/qkv_bias_ab.py::_alternate with the order of the arms rotated by one every round, so that no arm always runs
    behind the same neighbour."""
    graphs = [(k, _graph_of(fn, per)) for k, fn in arms.items()]
    out = {k: [] for k in arms}
    for it in range(warmup + repeats):
        shift = it % len(graphs)
        for k, g in graphs[shift:] + graphs[:shift]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per)
    return {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3), "repeats": len(v)}
            for k, v in out.items()}


def case(bs, others, warmup, repeats, per):
    from chitu_amd import _lib
    from chitu_amd._lib import i32, i64, ptr, stream_ptr
    from chitu_amd.llama import precompute_freqs_cis

    g = torch.Generator().manual_seed(bs)
    nh = HQ + 2 * HKV
    x = torch.randn(bs, nh, D, generator=g).to(BF16).cuda()
    bias = (0.5 * torch.randn(nh * D, generator=g)).to(BF16).cuda()
    pos = torch.randint(0, 4096, (bs,), generator=g)
    rows = {w: tuple(t[pos].contiguous().cuda() for t in precompute_freqs_cis(w, 4096, 5e6)) for w in (R, D)}
    per_seq = 8
    num_pages = bs * per_seq
    table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(bs, per_seq).cuda()
    lens = torch.tensor([(37 * b + 5) % (per_seq * PAGE) for b in range(bs)], dtype=torch.int32).cuda()
    keep = []

    def arm(lib, entry, width):
        work = x.clone()  # rotated in place again and again: the values wander, the work does not
        kc, vc = (torch.zeros(num_pages, PAGE, HKV, D, dtype=BF16, device="cuda") for _ in range(2))
        cos, sin = rows[width or D]
        keep.extend((work, kc, vc))
        fn = getattr(lib, entry)

        def launch():
            rc = fn(ptr(work), i64(nh * D), i32(HQ), i32(HKV), i32(D), ptr(cos), ptr(sin), i32(0), *((i32(width),) if width else ()),
                    ptr(kc), ptr(vc), i64(num_pages), i32(PAGE), ptr(table), i32(per_seq), ptr(lens), i32(bs), ptr(bias), stream_ptr())
            assert rc == 0, (entry, rc)

        return launch

    lib = _lib.lib()
    arms = {"ext7_R64": arm(lib, "chitu_ext7_gqa_qkv_bias_post", R), "ext5": arm(lib, "chitu_ext5_gqa_qkv_bias_post", None)}
    for name, other in others.items():
        arms["ext5@" + name] = arm(other, "chitu_ext5_gqa_qkv_bias_post", None)
    t = _rotating(arms, warmup, repeats, per)
    out = {"case": "decode", "bs": bs, "kv": "bf16", "q_heads": HQ, "kv_heads": HKV, "rotary_dim": R, "per_graph": per, **t,
           "ext7_over_ext5": round(t["ext7_R64"]["median_us"] / t["ext5"]["median_us"], 4)}
    for name in others:
        out[f"ext5_over_{name}"] = round(t["ext5"]["median_us"] / t["ext5@" + name]["median_us"], 4)
    return out


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per", type=int, default=200, help="launches per graph")
    ap.add_argument("--other-lib", action="append", default=[], metavar="NAME=PATH",
                    help="another build of libchitu_hip.so: its chitu_ext5_ entry is timed as one more arm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    others = {}
    for spec in a.other_lib:
        name, _, path = spec.partition("=")
        others[name] = ctypes.CDLL(os.path.abspath(path))
    rows = [{"box": _box(), "device": torch.cuda.get_device_name(0), "other_libs": sorted(others)}]
    print(json.dumps(rows[0]), flush=True)
    for bs in (1, 16):
        rows.append(case(bs, others, a.warmup, a.repeats, a.per))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
