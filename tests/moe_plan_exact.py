"""The launch plan of chitu_amd.fused_moe.fused_experts, recorded without a GPU (tests/test_fused_moe_plan_host.py).

fused_experts is host logic in front of C-ABI launches: which entries it calls, in which order, with which sizes and which
offsets into the persistent "moe" workspace.  All of that can be observed on the CPU once four things are substituted:

  _lib.lib            an object whose every attribute records (entry, arguments) and returns 0
  require_cuda        a no-op (the inputs are host tensors)
  stream_ptr          NULL
  workspace.get       one host uint8 buffer; each request is recorded as (bytes, tag)

record(fused_moe, case) runs one case and returns its plan as JSON-able data.  Every argument is written as [kind, value]:
["i32", 5], ["i64", 400], ["f32", 1e-10], ["int", 0] (a bare Python int, which ctypes passes as a C int) and for pointers
["ws", offset], [<name of the input tensor>, offset], ["out", offset] (the tensor the call returned), ["copy"] (a tensor the
call made itself, e.g. the contiguous copy of strided top-k ids) or "null".  CASES is the list the fixture
tests/golden/fused_moe_plan.json holds, recorded at the commit before the host routines were merged into one plan
(tools/record_fused_moe_plan.py); K = 256, E = 4, topk = 2 are the smallest shapes at which every branch is taken.
"""

import contextlib
import ctypes
import os

import torch

K, E, TOPK = 256, 4, 2
DECODE, PREFILL = 5, 200  # 200 tokens = 400 slots >= 24 * E: tiled-sized once the format's token floor allows it
WS_BYTES = 4 << 20
MODES = ("fp8", "soft_fp8", "bf16", "int8", "mxfp4")


def case(mode, tokens=DECODE, I=128, **kw):
    """tiled_floor: value of the three module floors (fp8 / MXFP4 / bf16) for the call; None = 128 / 512 / 0, the defaults.
    block_m: _MOE_TILED_BLOCK_M.  gne: global_num_experts with an int32 expert_map over it.  fuse_silu: CHITU_MOE_FUSE_SILU.
    bf16_floor: fused_experts(bf16_tiled_min_tokens=).  nout: rows of w2 (default K).  strided / ids64: the top-k tensors."""
    c = dict(mode=mode, tokens=tokens, I=I, tiled_floor=None, block_m=128, aligned=False, a1_quant=False, reduce_topk=True,
             gne=None, inplace=False, fuse_silu=None, bf16_floor=None, nout=K, strided=False, ids64=False)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def case_id(c):
    d = case(c["mode"])
    return "-".join([c["mode"]] + [f"{k}={c[k]}" for k in c if k != "mode" and c[k] != d[k]])


def _cases():
    out = []
    for m in MODES:
        out += [case(m), case(m, tokens=0), case(m, gne=8, inplace=True), case(m, aligned=True), case(m, strided=True, ids64=True),
                case(m, reduce_topk=False, nout=384), case(m, aligned=True, reduce_topk=False, inplace=True, gne=8)]
        if m in ("fp8", "bf16", "mxfp4"):  # prefill-sized: the defaults (fp8 tiles, MXFP4 and bf16 do not), then every floor at 128
            out += [case(m, tokens=PREFILL), case(m, tokens=PREFILL, tiled_floor=128, block_m=64),
                    case(m, tokens=PREFILL, tiled_floor=128, reduce_topk=False, gne=8, inplace=True),
                    case(m, tokens=PREFILL, tiled_floor=128, aligned=True),  # the caller's triple is block 16: streaming
                    case(m, tokens=PREFILL, tiled_floor=0)]
        else:  # no tiled form
            out += [case(m, tokens=PREFILL, tiled_floor=128, block_m=64)]
        if m in ("fp8", "int8", "mxfp4"):
            out += [case(m, a1_quant=True, aligned=True, inplace=True),
                    case(m, tokens=PREFILL if m != "int8" else DECODE, tiled_floor=128, a1_quant=True)]
        if m in ("fp8", "mxfp4"):  # wider than 512: three launches
            out += [case(m, I=640), case(m, I=640, a1_quant=True, aligned=True, reduce_topk=False),
                    case(m, tokens=PREFILL, I=640, tiled_floor=128, block_m=64)]
    out += [case("fp8", tokens=0, inplace=True), case("fp8", fuse_silu="0"), case("fp8", tokens=PREFILL, fuse_silu="0"),
            case("mxfp4", fuse_silu="0")]  # the switch is the fp8 path's alone
    # the per-call floor: bf16 experts only
    out += [case("bf16", tokens=PREFILL, bf16_floor=128), case("bf16", tokens=PREFILL, bf16_floor=256),
            case("bf16", tokens=PREFILL, tiled_floor=128, bf16_floor=0), case("soft_fp8", tokens=PREFILL, bf16_floor=128)]
    return out


CASES = _cases()


def inputs(c):
    """name -> host tensor; the values are never read."""
    T, I, nout, mode = c["tokens"], c["I"], c["nout"], c["mode"]
    gne = c["gne"] or E
    t = dict(hidden_states=torch.zeros(T, K, dtype=torch.bfloat16))
    if mode == "mxfp4":
        t.update(w1=torch.zeros(E, 2 * I, K // 2, dtype=torch.uint8), w1_scale=torch.zeros(E, 2 * I, K // 32, dtype=torch.uint8),
                 w2=torch.zeros(E, nout, I // 2, dtype=torch.uint8), w2_scale=torch.zeros(E, nout, I // 32, dtype=torch.uint8))
    elif mode == "int8":
        t.update(w1=torch.zeros(E, 2 * I, K, dtype=torch.int8), w1_scale=torch.zeros(E, 2 * I),
                 w2=torch.zeros(E, nout, I, dtype=torch.int8), w2_scale=torch.zeros(E, nout))
    elif mode == "bf16":
        t.update(w1=torch.zeros(E, 2 * I, K, dtype=torch.bfloat16), w2=torch.zeros(E, nout, I, dtype=torch.bfloat16))
    else:
        t.update(w1=torch.zeros(E, 2 * I, K, dtype=torch.float8_e4m3fn), w1_scale=torch.zeros(E, 2 * I // 128, K // 128),
                 w2=torch.zeros(E, nout, I, dtype=torch.float8_e4m3fn), w2_scale=torch.zeros(E, -(-nout // 128), I // 128))
    idt = torch.int64 if c["ids64"] else torch.int32
    if c["strided"]:
        t.update(topk_ids=torch.zeros(T, TOPK + 1, dtype=idt)[:, :TOPK], topk_weights=torch.zeros(T, TOPK + 1)[:, :TOPK])
    else:
        t.update(topk_ids=torch.zeros(T, TOPK, dtype=idt), topk_weights=torch.zeros(T, TOPK))
    if c["gne"]:
        t["expert_map"] = torch.tensor([0, -1, 1, -1, 2, -1, 3, -1], dtype=torch.int32)
    if c["aligned"]:
        cap = T * TOPK + gne * 15
        t.update(a_sorted=torch.zeros(cap, dtype=torch.int32), a_experts=torch.zeros(-(-cap // 16), dtype=torch.int32),
                 a_npost=torch.zeros(1, dtype=torch.int32))
    if c["a1_quant"]:
        if mode == "int8":
            t.update(a1_q=torch.zeros(T, K, dtype=torch.int8), a1_s=torch.zeros(T))
        else:
            t.update(a1_q=torch.zeros(T, K, dtype=torch.float8_e4m3fn), a1_s=torch.zeros(T, K // 128))
    return t


def call_kwargs(c, t):
    mode = c["mode"]
    kw = dict(inplace=c["inplace"], reduce_topk=c["reduce_topk"], w1_scale=t.get("w1_scale"), w2_scale=t.get("w2_scale"))
    if mode in ("fp8", "soft_fp8"):
        kw.update(use_fp8_w8a8=True, block_shape=[128, 128], soft_fp8=mode == "soft_fp8")
    elif mode == "int8":
        kw.update(use_int8_w8a8=True)
    elif mode == "mxfp4":
        kw.update(use_mxfp4_w4a8=True)
    if c["gne"]:
        kw.update(global_num_experts=c["gne"], expert_map=t["expert_map"])
    if c["aligned"]:
        kw.update(aligned=(t["a_sorted"], t["a_experts"], t["a_npost"]))
    if c["a1_quant"]:
        kw.update(a1_quant=(t["a1_q"], t["a1_s"]))
    if c["bf16_floor"] is not None:
        kw.update(bf16_tiled_min_tokens=c["bf16_floor"])
    return kw


class FakeLib:
    """Stands in for the loaded library: every attribute is an entry that records its call and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


@contextlib.contextmanager
def substituted(fm, lib, ws_requests, floors=None, block_m=128, fuse_silu=None):
    """fused_moe `fm` with the library, the device check, the stream and the workspace replaced, and every module constant
    that decides a plan pinned (they are read from the environment at import)."""
    ws = torch.zeros(WS_BYTES, dtype=torch.uint8)

    def get(nbytes, device, tag="default"):
        assert nbytes <= WS_BYTES
        ws_requests.append([int(nbytes), tag])
        return ws

    f8, mx, bf = (128, 512, 0) if floors is None else (floors,) * 3
    new = {(fm._lib, "lib"): lambda: lib, (fm, "require_cuda"): lambda *t: None, (fm, "stream_ptr"): lambda: ctypes.c_void_p(0),
           (fm.workspace, "get"): get, (fm, "_MOE_BLOCK_M"): 16, (fm, "_MOE_TILED_BLOCK_M"): block_m,
           (fm, "_MOE_TILED_MIN_TOKENS"): f8, (fm, "_MOE_TILED_MIN_PER_EXPERT"): 24, (fm, "_MOE_MXFP4_TILED_MIN_TOKENS"): mx,
           (fm, "_MOE_BF16_TILED_MIN_TOKENS"): bf}
    old = {k: getattr(*k) for k in new}
    env = os.environ.pop("CHITU_MOE_FUSE_SILU", None)
    if fuse_silu is not None:
        os.environ["CHITU_MOE_FUSE_SILU"] = fuse_silu
    try:
        for (obj, name), v in new.items():
            setattr(obj, name, v)
        yield ws
    finally:
        for (obj, name), v in old.items():
            setattr(obj, name, v)
        os.environ.pop("CHITU_MOE_FUSE_SILU", None)
        if env is not None:
            os.environ["CHITU_MOE_FUSE_SILU"] = env


def _arg(a, regions):
    if isinstance(a, ctypes.c_void_p):
        if not a.value:
            return "null"
        for name, (lo, nbytes) in regions.items():
            if lo <= a.value < lo + max(nbytes, 1):
                return [name, a.value - lo]
        return ["copy"]
    if a is None:
        return "null"
    for ct, kind in ((ctypes.c_int64, "i64"), (ctypes.c_int32, "i32"), (ctypes.c_float, "f32")):
        if isinstance(a, ct):
            return [kind, a.value]
    assert type(a) is int, (type(a), a)
    return ["int", a]


def record(fm, c):
    """One fused_experts call of module `fm` for case `c`: {"ws": [[bytes, tag] ...], "calls": [[entry, [args ...]] ...],
    "ret": what came back}."""
    t = inputs(c)
    lib, ws_requests = FakeLib(), []
    with substituted(fm, lib, ws_requests, c["tiled_floor"], c["block_m"], c["fuse_silu"]) as ws:
        ret = fm.fused_experts(t["hidden_states"], t["w1"], t["w2"], t["topk_weights"], t["topk_ids"], **call_kwargs(c, t))
    regions = {"ws": (ws.data_ptr(), WS_BYTES)}
    regions.update({name: (x.data_ptr(), x.numel() * x.element_size()) for name, x in t.items()})
    in_ws = ws.data_ptr() <= ret.data_ptr() < ws.data_ptr() + WS_BYTES and ret.numel() > 0
    if ret is t["hidden_states"]:
        where = ["hidden_states", 0]
    elif in_ws:
        assert ret.untyped_storage().data_ptr() == ws.untyped_storage().data_ptr()
        where = ["ws", ret.data_ptr() - ws.data_ptr()]
    else:
        regions["out"] = (ret.data_ptr(), ret.numel() * ret.element_size())
        where = ["out", 0]
    return {"ws": ws_requests,
            "calls": [[name, [_arg(a, regions) for a in args]] for name, args in lib.calls],
            "ret": {"at": where, "shape": list(ret.shape), "dtype": str(ret.dtype), "contiguous": ret.is_contiguous()}}
