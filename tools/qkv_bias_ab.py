"""Same-process A/B of the q / k / v bias launches (csrc/qkv_post_row16.hip) against what they stand beside, Qwen2.5-7B's 28 / 4 heads.

  decode   chitu_ext5_gqa_qkv_bias_post[_kv_fp8] against chitu_hip_gqa_qkv_post[_kv_fp8] -- the launch the same model without a
           bias takes -- at bs 1 and 16, bf16 and fp8 K / V pages.  The bias entry reads one more 16-byte chunk per lane and head.
  prefill  chitu_ext5_qkv_bias_rope against the composition it replaces -- a bf16 add of the bias, chitu_hip_rope on the q and k
           heads, the copy of v -- at 2048 rows.

Outputs are compared first (bit for bit: the new entry against the old one on qkv + bias).  Each arm is a hipGraph of `--per`
back-to-back launches on one stream (a chain, no branches); after warm-up the arms' graphs are replayed ALTERNATELY `--repeats`
times, every replay between two events.  Reported per arm: median [min .. max] microseconds per launch (prefill: per
composition).  One JSON line per case; --out writes them all, with the GPU's unique id, into one file.

    python tools/qkv_bias_ab.py --out profiles/qwen2_bias_ab.json
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D, PAGE = 28, 4, 128, 16
BF16 = torch.bfloat16


def _box():
    try:
        res = subprocess.run(["rocm-smi", "-d", "0", "--showuniqueid"], capture_output=True, text=True, timeout=10)
        ids = [ln.split(":")[-1].strip() for ln in res.stdout.splitlines() if ln.strip().startswith("GPU[")]
        return ids[0] if ids else f"no answer (rc {res.returncode})"
    except Exception as exc:  # noqa: BLE001
        return f"unavailable: {type(exc).__name__}"


def _graph_of(fn, per):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    return g


def _alternate(arms, warmup, repeats, per):
    """{name: callable} -> {name: {median_us, min_us, max_us, repeats}} per call, the arms' graphs replayed in turn."""
    graphs = {k: _graph_of(fn, per) for k, fn in arms.items()}
    out = {k: [] for k in arms}
    for it in range(warmup + repeats):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(e0.elapsed_time(e1) * 1e3 / per)
    return {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3), "repeats": len(v)}
            for k, v in out.items()}


def _inputs(rows, seed=0):
    from chitu_amd.llama import precompute_freqs_cis

    g = torch.Generator().manual_seed(seed)
    nh = HQ + 2 * HKV
    x = torch.randn(rows, nh, D, generator=g).to(BF16).cuda()
    bias = (0.5 * torch.randn(nh * D, generator=g)).to(BF16).cuda()
    cos_t, sin_t = precompute_freqs_cis(D, 4096, 1e6)
    pos = torch.randint(0, 4096, (rows,), generator=g)
    return x, bias, cos_t[pos].contiguous().cuda(), sin_t[pos].contiguous().cuda()


def decode_case(bs, fmt, warmup, repeats, per):
    from chitu_amd import ops

    x, bias, cos, sin = _inputs(bs)
    per_seq = 8
    num_pages = bs * per_seq
    table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(bs, per_seq).cuda()
    lens = torch.tensor([(37 * b + 5) % (per_seq * PAGE) for b in range(bs)], dtype=torch.int32).cuda()

    def caches():
        if fmt == "fp8":
            return [torch.zeros(num_pages, PAGE, HKV, 144, dtype=torch.uint8, device="cuda") for _ in range(2)]
        return [torch.zeros(num_pages, PAGE, HKV, D, dtype=BF16, device="cuda") for _ in range(2)]

    new = ops.gqa_qkv_bias_post_kv_fp8 if fmt == "fp8" else ops.gqa_qkv_bias_post
    old = ops.gqa_qkv_post_kv_fp8 if fmt == "fp8" else ops.gqa_qkv_post
    (kn, vn), (ko, vo) = caches(), caches()
    qn = new(x.clone(), HQ, HKV, cos, sin, kn, vn, table, lens, bias, rotary_type="hf-llama")
    qo = old((x + bias.view(-1, D)).contiguous(), HQ, HKV, cos, sin, ko, vo, table, lens, rotary_type="hf-llama")
    torch.cuda.synchronize()
    same = bool(torch.equal(qn, qo) and torch.equal(kn, ko) and torch.equal(vn, vo))
    assert same, f"decode bs={bs} {fmt}: the bias entry differs from the biasless entry on qkv + bias"
    wn, wo = x.clone(), x.clone()  # rotated in place again and again: the values wander, the work does not
    arms = {"bias_post": lambda: new(wn, HQ, HKV, cos, sin, kn, vn, table, lens, bias, rotary_type="hf-llama"),
            "post": lambda: old(wo, HQ, HKV, cos, sin, ko, vo, table, lens, rotary_type="hf-llama")}
    t = _alternate(arms, warmup, repeats, per)
    return {"case": "decode", "bs": bs, "kv": fmt, "q_heads": HQ, "kv_heads": HKV, "outputs_identical": same, "per_graph": per, **t,
            "bias_over_plain": round(t["bias_post"]["median_us"] / t["post"]["median_us"], 4)}


def prefill_case(rows, warmup, repeats, per):
    from chitu_amd import ops

    x, bias, cos, sin = _inputs(rows)

    def composed():
        y = x + bias.view(-1, D)
        q, k = ops.apply_rotary_pos_emb(y[:, :HQ], y[:, HQ:HQ + HKV], cos, sin, rotary_type="hf-llama")
        return q, k, y[:, HQ + HKV:].contiguous()

    fused = lambda: ops.qkv_bias_rope(x, HQ, HKV, bias, cos, sin, rotary_type="hf-llama")
    a, b = fused(), composed()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(u, v)) for u, v in zip(a, b))
    assert same, f"prefill rows={rows}: qkv_bias_rope differs from add + rope + copy"
    t = _alternate({"qkv_bias_rope": fused, "add+rope+copy": composed}, warmup, repeats, per)
    return {"case": "prefill", "rows": rows, "q_heads": HQ, "kv_heads": HKV, "outputs_identical": same, "per_graph": per, **t,
            "fused_over_composed": round(t["qkv_bias_rope"]["median_us"] / t["add+rope+copy"]["median_us"], 4)}


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per", type=int, default=200, help="launches per graph (decode); prefill uses a tenth")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    rows = [{"box": _box(), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("CHITU_HIP_LIB") or "in-tree"}]
    print(json.dumps(rows[0]), flush=True)
    for fmt in ("bf16", "fp8"):
        for bs in (1, 16):
            rows.append(decode_case(bs, fmt, a.warmup, a.repeats, a.per))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(prefill_case(a.rows, a.warmup, a.repeats, max(1, a.per // 10)))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
