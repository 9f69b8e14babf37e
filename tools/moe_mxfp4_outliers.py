#!/usr/bin/env python3
"""Census of the elements of fused_experts(use_mxfp4_w4a8=True) that miss the element-wise bar against the CPU reference, and
of their cause, for the shapes of tests/test_gpu_moe_mxfp4.py (both weight families).

The experts' intermediate h is re-quantised to fp8 between the two GEMMs.  Where the HIP kernels' and the reference's fp32
sums over K (different summation order) round an h value to neighbouring e4m3 codes (one step = 6 %), the outputs fed by it
move.  The census separates that cause from everything else:
  flipped   e4m3 codes of h (and group scales) that differ between HIP's GEMM1 + SiLU + quant and the reference's;
  outside   elements of the HIP output outside the bar against the reference;
  hybrid    the same count against the reference's GEMM2 evaluated ON HIP's h codes -- what is left when the flips are
            taken out.  0 here means the flips are the sole cause;
  ref32/64  elements by which two evaluations of the reference (block dots in fp32 and in fp64) differ between themselves.
One GPU process.  Usage: python tools/moe_mxfp4_outliers.py [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from chitu_amd import _lib, fused_moe  # noqa: E402
from chitu_amd._lib import check, i32, i64, ptr, stream_ptr  # noqa: E402
from oracle import fp8 as ofp8  # noqa: E402
from tests import mxfp4_ref as mx  # noqa: E402
from tests.test_gpu_moe_mxfp4 import SHAPES, free_case, run_mx, twin_case  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--only", default="", help="e.g. 16,64,8,2048,1408")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def outside(x, ref, peak_tol=1e-2, rtol=1e-2):
    x, ref = x.float(), ref.float()
    bound = rtol * ref.abs() + 0.5 * peak_tol * ref.abs().max()
    return int(((x - ref).abs() > bound).sum())


def hip_h(c):
    """HIP's e4m3 codes and group scales of h [numel, I]: plain GEMM1, then SiLU-and-mul + quant (the three-launch form; the
    two-launch form computes the same values)."""
    M, K = c["x"].shape
    topk, N = c["ids"].shape[1], c["w1"].shape[1]
    E = c["w1"].shape[0]
    numel = M * topk
    aq, as_ = fused_moe.per_token_group_quant_fp8(c["x"].cuda(), 128)
    sid, eid, npost = fused_moe.moe_align_block_size(c["ids"].cuda(), 16, E)
    c1 = torch.empty(numel, N, dtype=torch.bfloat16, device="cuda")
    w1, w1s = c["w1"].cuda(), c["w1s"].cuda()
    check(_lib.lib().chitu_hip_moe_gemm_mxfp4(ptr(aq), ptr(as_), i32(topk), ptr(w1), ptr(w1s), ptr(sid), ptr(eid), ptr(npost), ptr(None),
                                              i32(0), i32(0), ptr(c1), i64(numel), i64(N), i64(K), i64(min(eid.numel(), numel)), stream_ptr()),
          "gemm1")
    hq, hs = fused_moe.silu_and_mul_quant(c1, mode="group")
    torch.cuda.synchronize()
    return hq.cpu(), hs.cpu()


def ref_h(c):
    x, ids = c["x"], c["ids"]
    M, topk = ids.shape
    a1_q, a1_s = ofp8.per_token_group_quant_fp8(x)
    c1 = torch.empty(M, topk, c["w1"].shape[1], dtype=x.dtype)
    for t in range(M):
        for j in range(topk):
            e = int(ids[t, j])
            c1[t, j] = mx.gemm(a1_q[t:t + 1], a1_s[t:t + 1], c["w1"][e], c["w1s"][e], x.dtype)[0]
    d = c1.shape[-1] // 2
    c1 = c1.view(-1, 2 * d)
    return ofp8.per_token_group_quant_fp8(F.silu(c1[..., :d]) * c1[..., d:])


def gemm2_on(c, hq, hs):
    ids, wts = c["ids"], c["wts"]
    M, topk = ids.shape
    c3 = torch.empty(M, topk, c["w2"].shape[1], dtype=c["x"].dtype)
    for t in range(M):
        for j in range(topk):
            e, r = int(ids[t, j]), t * topk + j
            acc = mx.gemm(hq[r:r + 1], hs[r:r + 1], c["w2"][e], c["w2s"][e], torch.float32)[0]
            c3[t, j] = ofp8.to_out(acc * wts[t, j].float(), c["x"].dtype)
    return c3.sum(dim=1)


say("family shape                      | flipped h codes (of) | scales differing | outside vs reference (of) | vs reference on HIP's h | ref fp32 vs fp64")
for shape in SHAPES:
    if a.only and tuple(int(v) for v in a.only.split(",")) != shape:
        continue
    for fam, mk in (("twin", twin_case), ("free", free_case)):
        c = mk(*shape)
        out = run_mx(c)
        ref = c["ref"]
        hq, hs = hip_h(c)
        rq, rs = ref_h(c)
        flips = int((hq.view(torch.uint8) != rq.view(torch.uint8)).sum())
        sdiff = int((hs.view(-1) != rs.view(-1)).sum())
        hybrid = gemm2_on(c, hq, hs.view(rs.shape))
        r64 = mx.fused_experts_mxfp4(c["x"], c["w1"], c["w1s"], c["w2"], c["w2s"], c["wts"], c["ids"], dot_dtype=torch.float64)
        say(f"{fam:5s}  {str(shape):26s} | {flips:6d} ({hq.numel()}) | {sdiff:6d} | {outside(out, ref):4d} ({out.numel()}) | "
            f"{outside(out, hybrid):4d} | {outside(ref, r64):4d}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
