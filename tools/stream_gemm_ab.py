#!/usr/bin/env python3
"""Writes profiles/stream_gemm_ab.json from the outputs of runs made on one GPU in one session:

    CHITU_HIP_LIB=<parent build> python tools/w8a16_ab.py --out parent1.json
    python tools/w8a16_ab.py --out new.json
    CHITU_HIP_LIB=<parent build> python tools/w8a16_ab.py --out parent2.json
    python tools/stream_gemm_ab.py --parent1 parent1.json --new new.json --parent2 parent2.json \
        [--steps steps.log ...] --parent-commit 76c16b0 --out profiles/stream_gemm_ab.json

A case is within the bar when this tree's median is at most the slower parent median plus the distance between the two
parent medians.  --steps: a log of alternating whole-step readings -- a line `parent` or `new`, then the JSON line that
`tools/llama_ab.py --child-format F --bs B` printed with that library; one file per (format, batch size).  No GPU is needed
to merge; the GPU's unique id is read (tools/qkv_bias_ab.py's way) only when --gpu-id is not given."""
import argparse
import json
import subprocess


def box():
    try:
        res = subprocess.run(["rocm-smi", "-d", "0", "--showuniqueid"], capture_output=True, text=True, timeout=10)
        ids = [ln.split(":")[-1].strip() for ln in res.stdout.splitlines() if ln.strip().startswith("GPU[")]
        return ids[0] if ids else f"no answer (rc {res.returncode})"
    except Exception as exc:  # noqa: BLE001
        return f"unavailable: {type(exc).__name__}"


def step_readings(path):
    out, cur, key = {"parent": [], "this_tree": []}, None, None
    for ln in open(path):
        ln = ln.strip()
        if ln in ("parent", "new"):
            cur = "parent" if ln == "parent" else "this_tree"
        elif ln.startswith("{") and cur:
            row = json.loads(ln)
            key = f"{row['format']} bs{row['bs']}"
            out[cur].append(row["ms_per_step"])
    return key, out


ap = argparse.ArgumentParser()
ap.add_argument("--parent1", required=True)
ap.add_argument("--new", required=True)
ap.add_argument("--parent2", required=True)
ap.add_argument("--steps", nargs="*", default=[])
ap.add_argument("--gpu-id", default="")
ap.add_argument("--parent-commit", default="")
ap.add_argument("--out", required=True)
a = ap.parse_args()
p1, new, p2 = (json.load(open(f))["shapes"] for f in (a.parent1, a.new, a.parent2))
cases = {}
for case in p1:
    for arm in ("bf16", "w8a16"):
        x, y, z = (d[case][arm]["median_us"] for d in (p1, new, p2))
        floor = round(abs(x - z), 2)
        bar = round(max(x, z) + floor, 2)
        cases[f"{case} {arm}"] = {"parent_1_us": x, "this_tree_us": y, "parent_2_us": z, "noise_floor_us": floor, "bar_us": bar,
                                  "within_bar": y <= bar + 1e-9}
doc = {"what": "tools/w8a16_ab.py as three processes (parent build, this tree, parent build) on one GPU in one session: median "
               "us per cold launch; written by tools/stream_gemm_ab.py",
       "gpu_unique_id": a.gpu_id or box(), "parent_commit": a.parent_commit, "cases": cases,
       "misses": [k for k, v in cases.items() if not v["within_bar"]],
       "llama3_8b_step_ms": dict(step_readings(f) for f in a.steps)}
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
print(f"{len(doc['misses'])} of {len(cases)} readings outside their bar: {doc['misses']}")
