#!/usr/bin/env python3
"""Record the launch plans of fused_experts into tests/golden/fused_moe_plan.json (no GPU needed).

The plans are a record of what one commit issues, so run this with that commit's checkout in front on PYTHONPATH:

    git worktree add /tmp/parent <commit>
    PYTHONPATH=/tmp/parent python tools/record_fused_moe_plan.py

chitu_amd is then imported from that checkout; the cases and the recorder are this tree's tests/moe_plan_exact.py.
tests/test_fused_moe_plan_host.py asserts that the tree issues exactly the recorded plans."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fused_moe_plan.json"))
    args = ap.parse_args()
    sys.path.append(ROOT)  # behind PYTHONPATH: another checkout's chitu_amd wins
    spec = importlib.util.spec_from_file_location("moe_plan_exact", os.path.join(ROOT, "tests", "moe_plan_exact.py"))
    mp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mp)
    from chitu_amd import fused_moe

    plans = {mp.case_id(c): mp.record(fused_moe, c) for c in mp.CASES}
    assert len(plans) == len(mp.CASES), "case ids must be unique"
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in plans.items()) + "\n}\n")
    print(f"{len(plans)} plans from {os.path.dirname(os.path.dirname(fused_moe.__file__))} -> {args.out} "
          f"({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
