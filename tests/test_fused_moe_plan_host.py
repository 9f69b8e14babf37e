"""Host tests (no GPU) of what fused_experts issues: for every expert format the sequence of C-ABI entries, every argument
value and every workspace offset equal the plans recorded before the four host routines were merged into one plan
(tests/golden/fused_moe_plan.json, tools/record_fused_moe_plan.py; cases and recorder: tests/moe_plan_exact.py), and every
refusal fires before the first library call."""
import ast
import json
import os
import re

import pytest
import torch

from chitu_amd import fused_moe
from tests import moe_plan_exact as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "fused_moe_plan.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    ids = [mp.case_id(c) for c in mp.CASES]
    assert len(set(ids)) == len(ids) and sorted(golden) == sorted(ids)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fused_moe_plan.json")) < 100 << 10
    # every mode reaches its last launch in the plain case, and every axis is on both sides somewhere
    for m in mp.MODES:
        assert golden[m]["calls"][-1][0] == "chitu_hip_moe_sum"
    for axis in ("aligned", "a1_quant", "reduce_topk", "gne", "inplace", "bf16_floor", "strided"):
        assert len({repr(c[axis]) for c in mp.CASES}) >= 2, axis
    assert {c["tokens"] for c in mp.CASES} == {0, mp.DECODE, mp.PREFILL} and {c["block_m"] for c in mp.CASES} == {64, 128}


@pytest.mark.parametrize("c", mp.CASES, ids=mp.case_id)
def test_plan_is_the_recorded_one(c, golden):
    got = json.loads(json.dumps(mp.record(fused_moe, c)))
    want = golden[mp.case_id(c)]
    assert [e for e, _ in got["calls"]] == [e for e, _ in want["calls"]]
    for (entry, a), (_, b) in zip(got["calls"], want["calls"]):
        assert a == b, entry
    assert got == want


@pytest.mark.parametrize("c", [c for c in mp.CASES if c["tokens"] and not c["reduce_topk"]], ids=mp.case_id)
def test_unreduced_result_is_a_view_of_c3(c):
    """reduce_topk=False: [tokens, topk, Nout] bf16, contiguous, at the address GEMM2 wrote (its output argument)."""
    plan = mp.record(fused_moe, c)
    ret = plan["ret"]
    assert ret["shape"] == [c["tokens"], mp.TOPK, c["nout"]] and ret["dtype"] == "torch.bfloat16" and ret["contiguous"]
    assert ret["at"][0] == "ws" and ret["at"][1] % 256 == 0
    assert ret["at"] in plan["calls"][-1][1]  # the last launch is GEMM2, and no moe_sum follows
    assert ret["at"][1] + c["tokens"] * mp.TOPK * c["nout"] * 2 <= plan["ws"][0][0]
    assert plan["ws"] == [[plan["ws"][0][0], "moe"]]


@pytest.mark.parametrize("mode", mp.MODES)
def test_empty_batch_returns_before_anything_is_touched(mode):
    for inplace in (False, True):
        plan = mp.record(fused_moe, mp.case(mode, tokens=0, inplace=inplace))
        assert plan["calls"] == [] and plan["ws"] == []
        assert plan["ret"]["shape"] == [0, mp.K] and plan["ret"]["at"][0] == ("hidden_states" if inplace else "out")


# ---------------------------------------------------------------- refusals: the exception, and no library call before it
def _refused(exc, c, **override):
    """fused_experts for case c with keyword / input overrides raises `exc` with an empty call log."""
    t = mp.inputs(c)
    kw = mp.call_kwargs(c, t)
    for k in list(override):
        if k in ("hidden_states", "w1", "w2", "topk_weights", "topk_ids"):
            t[k] = override.pop(k)
    kw.update(override)
    lib, ws = mp.FakeLib(), []
    with mp.substituted(fused_moe, lib, ws, 128):
        with pytest.raises(exc):
            fused_moe.fused_experts(t["hidden_states"], t["w1"], t["w2"], t["topk_weights"], t["topk_ids"], **kw)
    assert lib.calls == []


@pytest.mark.parametrize("mode", mp.MODES)
def test_refusals_fire_before_the_first_library_call(mode):
    c = mp.case(mode)
    t = mp.inputs(c)
    _refused(ValueError, c, activation="gelu")
    _refused(AssertionError, c, topk_weights=torch.zeros(mp.DECODE, mp.TOPK + 1))                 # topk shape mismatch
    _refused(AssertionError, c, hidden_states=torch.zeros(mp.DECODE, mp.K // 2, dtype=torch.bfloat16))  # hidden size
    _refused(AssertionError, c, hidden_states=torch.zeros(mp.DECODE, 2 * mp.K, dtype=torch.bfloat16)[:, :mp.K])
    _refused(AssertionError, c, hidden_states=torch.zeros(mp.DECODE, mp.K, dtype=torch.float16))
    _refused(AssertionError, c, w2=t["w2"][:, :, : t["w2"].shape[2] // 2].contiguous())            # w2 is not [E, Nout, I]
    if mode != "bf16":
        _refused(AssertionError, c, w1_scale=None)
    if mode != "mxfp4":
        _refused(AssertionError, c, w1=t["w1"].transpose(1, 2))                                     # not contiguous
    # the summed output must have the hidden size: moe_sum writes Nout columns into `out`
    _refused(AssertionError, mp.case(mode, nout=384))
    # a caller's `aligned`: int32, and the sizes of block 16 over global_num_experts
    ca = mp.case(mode, aligned=True)
    ta = mp.inputs(ca)
    s, e, n = ta["a_sorted"], ta["a_experts"], ta["a_npost"]
    _refused(AssertionError, ca, aligned=(s.long(), e, n))
    _refused(AssertionError, ca, aligned=(s, e.long(), n))
    _refused(AssertionError, ca, aligned=(s, e, n.long()))
    _refused(AssertionError, ca, aligned=(s[:-1], e, n))
    _refused(AssertionError, ca, aligned=(s, e[:-1], n))


def test_weight_only_modes_are_refused_before_the_first_library_call():
    c = mp.case("bf16")
    _refused(NotImplementedError, c, use_int8_w8a16=True)
    _refused(NotImplementedError, c, use_int4_w4a16=True)
    _refused(AssertionError, mp.case("fp8"), block_shape=[64, 64])
    _refused(AssertionError, mp.case("fp8"), a1_scale=torch.ones(1))


@pytest.mark.parametrize("mode", ["fp8", "mxfp4", "int8"])
def test_a_producers_a1_quant_is_checked(mode):
    """Size and dtype of a1_quant=(q, s); the fp8 and MXFP4 experts share one form (one byte per element, fp32 group scales)."""
    c = mp.case(mode, a1_quant=True, aligned=True)  # with `aligned` the quantiser would be the first launch
    t = mp.inputs(c)
    q, s = t["a1_q"], t["a1_s"]
    _refused(AssertionError, c, a1_quant=(q[:-1], s))
    _refused(AssertionError, c, a1_quant=(q, s[:-1]))
    _refused(AssertionError, c, a1_quant=(q, s.double()))
    _refused(AssertionError, c, a1_quant=(q.to(torch.bfloat16), s))
    _refused(AssertionError, c, a1_quant=(q.t(), s))


# ---------------------------------------------------------------- one copy of what the formats share
def test_shared_steps_are_written_once():
    src = open(fused_moe.__file__).read()
    body = src[src.index("class _MoePlan"):]  # behind the public moe_align_block_size / cuda_moe_align_block_size
    assert len(re.findall(r"\.chitu_hip_moe_align_block_size_mapped\(", body)) == 1
    assert len(re.findall(r"\.chitu_hip_moe_sum\(", src)) == 1
    assert len(re.findall(r"\.view\(torch\.bfloat16\)", src)) == 1           # the reduce_topk=False view of "c3"
    assert len(re.findall(r"workspace\.get\(", src)) == 1 and '"moe"' in src
    tree = ast.parse(src)
    imports = [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert all(n in tree.body for n in imports)                                # no function-local import
    assert len(re.findall(r"^import ctypes$", src, flags=re.M)) == 1
