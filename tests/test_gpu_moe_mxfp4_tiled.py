"""The prefill form of the MXFP4 experts (W4A8, csrc/moe_mxfp4_tiled.hip) on the MI355X: fused_experts(use_mxfp4_w4a8=True) at
>= 128 tokens against the streaming form (bit for bit with its K split off), the pinned fp8 oracle and the fp8 HIP tiled path on
weights that are both formats, tests/mxfp4_ref.py on freely quantised weights, its options, and a tiny DeepSeek-V3 prefill.
Helpers that live inside tests/test_gpu_moe_mxfp4.py are restated here."""

import functools

import pytest
import torch

from oracle import moe as omoe
from tests import mxfp4_ref as mx
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

# (M, E, topk, K, I): the smallest shapes at which each mechanism can go wrong; all have M >= 128 and M * topk >= 24 * E
SHAPES = [
    (300, 8, 2, 128, 128),    # one K block in both GEMMs: the ring never turns
    (128, 8, 2, 256, 128),    # exactly 128 tokens; two K blocks, then one
    (129, 8, 2, 384, 640),    # odd block counts (3 and 5), wide experts, one token past a tile
    (300, 16, 4, 512, 256),   # R1's expert width
    (600, 4, 2, 256, 128),    # ~300 slots per expert: several blocks per expert, the last one partly padding
    (128, 32, 8, 7168, 256),  # R1's hidden size: 56 K blocks
]
# the three smallest by M * topk * K * I, and the wide-expert shape beside them
FREE_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[2]]


@pytest.fixture(autouse=True)
def _mxfp4_switch_over_at_128_tokens(monkeypatch):
    """By default the MXFP4 path switches over at 512 tokens (measured).  The shapes here are the smallest at
    which the kernels can go wrong, from 128 tokens on, so the tests lower that threshold to the shared rule's 128."""
    from chitu_amd import fused_moe

    monkeypatch.setattr(fused_moe, "_MOE_MXFP4_TILED_MIN_TOKENS", 128)


def _rel_mean(a, b):
    return ((a.float() - b.float()).abs().mean() / b.float().abs().mean()).item()


@functools.lru_cache(maxsize=None)
def twin_case(M, E, topk, K, I, seed=None, nout=None):
    """Inputs whose MXFP4 weights are at the same time fp8 block-scaled weights (tests/test_mxfp4_host.py proves the equality).
    Computed once per shape and left unchanged."""
    g = torch.Generator().manual_seed(M * 1000 + E if seed is None else seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w1p, w1s, w1_8, w1_bs = mx.fp8_twin_weights(E, 2 * I, K, g)
    w2p, w2s, w2_8, w2_bs = mx.fp8_twin_weights(E, K if nout is None else nout, I, g)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(M)])
    wts = torch.rand(M, topk, generator=g).to(torch.bfloat16)
    return dict(x=x, w1=w1p, w1s=w1s, w2=w2p, w2s=w2s, w1_8=w1_8, w2_8=w2_8, w1_bs=w1_bs, w2_bs=w2_bs, ids=ids, wts=wts)


@functools.lru_cache(maxsize=None)
def twin_oracle(M, E, topk, K, I):
    c = twin_case(M, E, topk, K, I)
    return omoe.fused_experts_fp8(c["x"], c["w1_8"], c["w2_8"], c["wts"], c["ids"], c["w1_bs"], c["w2_bs"])


@functools.lru_cache(maxsize=None)
def free_case(M, E, topk, K, I):
    """Weights quantised freely from randn (any scale byte per block, no fp8 twin) and the local reference's result."""
    g = torch.Generator().manual_seed(M * 1000 + E + 3)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w1, w1s = mx.quant(torch.randn(E, 2 * I, K, generator=g) * 0.01)
    w2, w2s = mx.quant(torch.randn(E, K, I, generator=g) * 0.01)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(M)])
    wts = torch.rand(M, topk, generator=g).to(torch.bfloat16)
    ref = mx.fused_experts_mxfp4(x, w1, w1s, w2, w2s, wts, ids)
    return dict(x=x, w1=w1, w1s=w1s, w2=w2, w2s=w2s, ids=ids, wts=wts, ref=ref)


TILED_ENTRIES = {"chitu_hip_moe_gemm1_silu_mxfp4_tiled", "chitu_hip_moe_gemm2_mxfp4_tiled"}
STREAMING_ENTRIES = {"chitu_hip_moe_gemm1_silu_mxfp4", "chitu_hip_moe_gemm2_quant_mxfp4", "chitu_hip_moe_gemm_mxfp4"}


def run_mx(c, x=None, form="tiled", **kw):
    """fused_experts(use_mxfp4_w4a8=True) on the case; `form`: which expert GEMM entries the call must have gone through
    (read off the C-ABI call log), "tiled" or "streaming"."""
    from chitu_amd import _lib, fused_moe

    xd = (c["x"] if x is None else x).cuda().clone()
    wts, ids = kw.pop("wts", c["wts"]), kw.pop("ids", c["ids"])
    w1, w1s, w2, w2s = (kw.pop(k, c[k]) for k in ("w1", "w1s", "w2", "w2s"))
    args = (xd, w1.cuda(), w2.cuda(), wts.cuda(), ids.cuda())
    _lib.call_log = []
    try:
        out = fused_moe.fused_experts(*args, use_mxfp4_w4a8=True, w1_scale=w1s.cuda(), w2_scale=w2s.cuda(), **kw)
        called = {name for name, _ in _lib.call_log}
    finally:
        _lib.call_log = None
    want, other = (TILED_ENTRIES, STREAMING_ENTRIES) if form == "tiled" else (STREAMING_ENTRIES, TILED_ENTRIES)
    assert called & want and not called & other, (form, sorted(called))
    if form == "tiled":
        assert want <= called
    if kw.get("inplace"):
        assert out.data_ptr() == xd.data_ptr()
    return out.cpu()


def _is_tiled(c, aligned=None):
    from chitu_amd import fused_moe

    M, topk = c["ids"].shape
    return fused_moe._takes_tiled(M, M * topk, c["w1"].shape[0], c["w1"].shape[1] // 2, c["w2"].shape[1], aligned,
                                  min_tokens=fused_moe._MOE_MXFP4_TILED_MIN_TOKENS)


def _streamed(c, monkeypatch, wk=None, **kw):
    """The streaming form on the same inputs (tiling switched off); wk = 1: without its K split."""
    from chitu_amd import fused_moe
    from chitu_amd._lib import debug_option

    with monkeypatch.context() as m:
        m.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 0)
        assert not _is_tiled(c)
        if wk is None:
            return run_mx(c, form="streaming", **kw)
        with debug_option("moe_gemm1_wk", wk):
            return run_mx(c, form="streaming", **kw)


# ---------------------------------------------------------------- the tiled form against the streaming form and the oracles
@pytest.mark.parametrize("M,E,topk,K,I", SHAPES)
def test_tiled_vs_streaming_and_the_fp8_oracle_on_fp8_representable_weights(M, E, topk, K, I, monkeypatch):
    """(1) Bit identity with the streaming form without its K split: both are then the same ascending fma chain per output over
    the same hardware block dots, the same bf16 / SiLU rounding points and the same per_token_group_quant_fp8 rule for h.
    (2) Against the default streaming form (heuristic K split): peak 1e-2, mean < 5e-3.  (3) Against the pinned fp8 oracle and
    the fp8 HIP tiled path on the twin weights, at the bars the fp8 tiled test uses for hundreds of rows.  (5) Run to run."""
    from chitu_amd import fused_moe

    c = twin_case(M, E, topk, K, I)
    assert M >= 128 and M * topk >= 24 * E and _is_tiled(c)
    tiled = run_mx(c)
    assert torch.isfinite(tiled.float()).all()
    assert torch.equal(tiled, run_mx(c)), "no atomics: run to run identical"
    s1 = _streamed(c, monkeypatch, wk=1)
    diff = (tiled.float() - s1.float()).abs()
    print(f"{M, E, topk, K, I}: tiled vs streaming (WK = 1): {int((diff != 0).sum())} of {diff.numel()} differ, "
          f"peak {max_rel_to_peak(tiled, s1):.3e}")
    assert torch.equal(tiled, s1), "tiled form != streaming form without its K split"
    s = _streamed(c, monkeypatch)
    print(f"{M, E, topk, K, I}: tiled vs streaming (default): peak {max_rel_to_peak(tiled, s):.3e}, mean {_rel_mean(tiled, s):.3e}")
    assert_close(tiled, s, 1e-2, what="tiled vs default streaming")
    assert _rel_mean(tiled, s) < 5e-3
    f8 = fused_moe.fused_experts(c["x"].cuda().clone(), c["w1_8"].cuda(), c["w2_8"].cuda(), c["wts"].cuda(), c["ids"].cuda(),
                                 use_fp8_w8a8=True, w1_scale=c["w1_bs"].cuda(), w2_scale=c["w2_bs"].cuda(), block_shape=[128, 128]).cpu()
    print(f"{M, E, topk, K, I}: tiled mxfp4 vs tiled fp8 HIP: peak {max_rel_to_peak(tiled, f8):.3e}, mean {_rel_mean(tiled, f8):.3e}")
    assert_close(tiled, f8, 2e-2, what="mxfp4 tiled vs fp8 HIP tiled on the twin")
    assert _rel_mean(tiled, f8) < 5e-3
    if M * topk * K * I <= 3e9:
        ref = twin_oracle(M, E, topk, K, I)
        print(f"{M, E, topk, K, I}: tiled vs the fp8 oracle: peak {max_rel_to_peak(tiled, ref):.3e}, mean {_rel_mean(tiled, ref):.3e}")
        # hundreds of rows: the largest single deviation (one h value on an fp8 rounding boundary, SiLU by expf vs torch.exp)
        # grows with the element count and is shared with the streaming kernels; the mean stays put
        assert_close(tiled, ref, 2e-2, what="mxfp4 tiled vs the fp8 oracle")
        assert _rel_mean(tiled, ref) < 5e-3


@pytest.mark.parametrize("M,E,topk,K,I", FREE_SHAPES)
def test_tiled_vs_the_local_reference_on_freely_quantised_weights(M, E, topk, K, I):
    """Scale bytes outside the narrow band of the twin weights.  Bars: those of the oracle comparison above (hundreds of rows:
    one h value on an e4m3 rounding boundary moves the outputs it feeds; the mean does not move)."""
    c = free_case(M, E, topk, K, I)
    assert _is_tiled(c)
    out = run_mx(c)
    print(f"{M, E, topk, K, I}: tiled vs mxfp4_ref, randn weights: peak {max_rel_to_peak(out, c['ref']):.3e}, mean {_rel_mean(out, c['ref']):.3e}")
    assert_close(out, c["ref"], 2e-2, what="mxfp4 tiled vs mxfp4_ref")
    assert _rel_mean(out, c["ref"]) < 5e-3


# ---------------------------------------------------------------- options
def test_block_heights_64_and_128_return_the_same_bits(monkeypatch):
    from chitu_amd import fused_moe

    c = twin_case(600, 4, 2, 256, 128)
    outs = {}
    for bm in (64, 128):
        monkeypatch.setattr(fused_moe, "_MOE_TILED_BLOCK_M", bm)
        outs[bm] = run_mx(c)
    assert torch.equal(outs[64], outs[128])
    cw = twin_case(129, 8, 2, 384, 640)
    for bm in (64, 128):
        monkeypatch.setattr(fused_moe, "_MOE_TILED_BLOCK_M", bm)
        outs[bm] = run_mx(cw)
    assert torch.equal(outs[64], outs[128])


def test_expert_map_with_absent_experts_and_an_idle_local_expert():
    """Half the experts live on another rank (-1) and local expert 2 gets no token at all: an absent expert = a zero routed
    weight, bit for bit."""
    M, E, topk, K, I = 300, 8, 2, 256, 128
    c = twin_case(M, E, topk, K, I, seed=23)
    g = torch.Generator().manual_seed(5)
    pool = torch.tensor([0, 1, 3, 4, 5, 6, 7])
    ids = torch.stack([pool[torch.randperm(len(pool), generator=g)[:topk]] for _ in range(M)])
    assert not (ids == 2).any() and (ids >= 4).any()
    h = E // 2
    emap = torch.full((E,), -1, dtype=torch.int32)
    emap[:h] = torch.arange(h, dtype=torch.int32)
    assert _is_tiled(c)
    mapped = run_mx(c, ids=ids, w1=c["w1"][:h].contiguous(), w1s=c["w1s"][:h].contiguous(), w2=c["w2"][:h].contiguous(),
                    w2s=c["w2s"][:h].contiguous(), expert_map=emap.cuda(), global_num_experts=E)
    masked = torch.where(ids < h, c["wts"].float(), torch.zeros(())).to(c["wts"].dtype)
    assert torch.equal(mapped, run_mx(c, ids=ids, wts=masked))
    ref = omoe.fused_experts_fp8(c["x"], c["w1_8"], c["w2_8"], masked, ids, c["w1_bs"], c["w2_bs"])
    assert max_rel_to_peak(mapped, ref) < 2e-2


def test_unreduced_output_with_a_row_tail_equals_the_streaming_form(monkeypatch):
    """reduce_topk=False, w2 with Nout = 200 rows (no multiple of 128 nor of 16): the tail tile re-reads clamped rows and
    does not store them."""
    M, E, topk, K, I = 300, 8, 2, 256, 128
    c = twin_case(M, E, topk, K, I, seed=29, nout=200)
    assert _is_tiled(c)
    un = run_mx(c, reduce_topk=False)
    assert tuple(un.shape) == (M, topk, 200) and torch.isfinite(un.float()).all()
    assert torch.equal(un, _streamed(c, monkeypatch, wk=1, reduce_topk=False))


def test_inplace_and_a1_quant_equal_the_plain_call():
    from chitu_amd import fused_moe

    c = twin_case(300, 8, 2, 128, 128)
    plain = run_mx(c)
    assert torch.equal(run_mx(c, inplace=True), plain)
    aq, as_ = fused_moe.per_token_group_quant_fp8(c["x"].cuda(), 128)
    assert torch.equal(run_mx(c, a1_quant=(aq, as_)), plain)
    un = run_mx(c, reduce_topk=False)
    assert torch.equal(un.float().sum(1).to(torch.bfloat16), plain)


def test_default_switch_over_is_512_tokens(monkeypatch):
    """With the default threshold a 300-token call streams and a 512-token call is tiled (run_mx reads the form off the call
    log); both agree with the other form of the same call bit for bit (K split off)."""
    from chitu_amd import fused_moe

    monkeypatch.setattr(fused_moe, "_MOE_MXFP4_TILED_MIN_TOKENS", 512)
    c300, c512 = twin_case(300, 8, 2, 128, 128), twin_case(512, 8, 2, 128, 128)
    assert not _is_tiled(c300) and _is_tiled(c512)
    s300 = run_mx(c300, form="streaming")
    t512 = run_mx(c512, form="tiled")
    assert torch.equal(t512, _streamed(c512, monkeypatch, wk=1))
    monkeypatch.setattr(fused_moe, "_MOE_MXFP4_TILED_MIN_TOKENS", 128)
    assert max_rel_to_peak(run_mx(c300, form="tiled"), s300) < 1e-2


# ---------------------------------------------------------------- model
def _tiny_args(**kw):
    """tests/test_gpu_moe_mxfp4.py::tiny_args, restated: 16 routed + 1 shared expert, top 4 + 1."""
    from chitu_amd.deepseek_v3 import DeepSeekV3Args

    return DeepSeekV3Args(
        vocab_size=1024, dim=512, inter_dim=1024, moe_inter_dim=256, n_layers=3, n_dense_layers=1, n_heads=16,
        n_routed_experts=16, n_shared_experts=1, n_activated_experts=4, n_expert_groups=4, n_limited_groups=2,
        q_lora_rank=256, gate_bias=True, **kw)


def _build(args, seed=0):
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.deepseek_v3 import DeepSeekV3Decoder, init_synthetic_

    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=2, block_size=64, max_seq_len=256, device="cuda",
                                kv_shape_per_sample=(576,), dtype=torch.bfloat16)
    model = DeepSeekV3Decoder(args, cache, HipAttnBackend(local_n_heads=16, max_seq_len=256), max_position_embeddings=256,
                              device="cuda")
    init_synthetic_(model, seed=seed)
    return model, cache


def test_tiny_model_prefill_with_mxfp4_experts_takes_the_tiled_form(monkeypatch):
    """model.prefill of a 200-token and a 7-token prompt: the routed experts see 207 tokens x (4 + 1) slots over 17 experts and
    take the tiled form; a second, identically seeded model with tiling switched off takes the streaming form (its own K
    split: another order of the fp32 sum).  Layer 0 is dense: its KV rows are the same bits; the last layer's carry the
    re-quantisation noise of the two summation orders through two MoE layers (the bar of the prefill-vs-decode test)."""
    from chitu_amd import _lib, fused_moe

    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (200, 7)]
    calls = []
    real = fused_moe._takes_tiled

    def recorded(num_tokens, *rest, **kw):
        calls.append((num_tokens, real(num_tokens, *rest, **kw)))
        return calls[-1][1]

    monkeypatch.setattr(fused_moe, "_takes_tiled", recorded)
    res = {}
    for mode in ("tiled", "streamed"):
        monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 128 if mode == "tiled" else 0)
        del calls[:]
        model, cache = _build(_tiny_args(expert_dtype="mxfp4"), seed=1)
        reqs = ["p0", "p1"]
        _lib.call_log = []
        try:
            logits = model.prefill(prompts, reqs).clone()
            entries = [name for name, _ in _lib.call_log if name in TILED_ENTRIES | STREAMING_ENTRIES]
        finally:
            _lib.call_log = None
        rows = [torch.cat([cache.paged_kv_cache[:, b] for b in cache.block_table[r]], dim=1)[:, :len(p)].cpu()
                for r, p in zip(reqs, prompts)]
        res[mode] = (logits.cpu(), rows, list(calls), entries)
        del model, cache
    (lt, rt, ct, et), (ls, rs, cs, es) = res["tiled"], res["streamed"]
    assert et == ["chitu_hip_moe_gemm1_silu_mxfp4_tiled", "chitu_hip_moe_gemm2_mxfp4_tiled"] * 2, et
    assert es == ["chitu_hip_moe_gemm1_silu_mxfp4", "chitu_hip_moe_gemm2_quant_mxfp4"] * 2, es
    assert len(ct) == 2 and all(n == 207 and took for n, took in ct), ct   # the two MoE layers, 207 tokens each, tiled
    assert len(cs) == 2 and not any(took for _, took in cs), cs
    assert tuple(lt.shape) == (2, 1024) and torch.isfinite(lt).all() and torch.isfinite(ls).all()
    print(f"tiny model prefill, tiled vs streamed MXFP4 experts: logits {max_rel_to_peak(lt, ls):.3e} of the peak")
    assert max_rel_to_peak(lt, ls) < 1e-2
    for a, b in zip(rt, rs):
        assert torch.equal(a[0], b[0]), "layer 0 (dense) sees identical arithmetic"
        assert_close(a[-1], b[-1], 6e-2, what="KV rows of the last layer")
