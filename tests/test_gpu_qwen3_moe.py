"""Qwen3MoeDecoder on the GPU, at the fixture's size (tests/golden/qwen3_moe_hf.npz: hidden 256, 16 experts of width 128, top 4
renormalised, 2 layers, 4 / 2 heads of 128, vocab 512; weights regenerated from the seed, loaded through the checkpoint path).

A bf16 run cannot be held against Hugging Face's fp32 logits directly: near-tied experts flip (HF's own bf16 run lands 0.16 of
the peak away under free routing, 9.3e-3 with its routing forced to the fp32 run's ids -- the fixture's generator).  So the
router is checked on its own, exactly, from what it saw (record_routing), and the logits are checked against the fp32
restatement (tests/qwen3_moe_ref.py, itself within 1e-4 of HF's fp32 run) forced to the ids the engine chose, at the 2e-2 bar
of the dense Qwen3 test."""

import gc

import numpy as np
import pytest
import torch

from tests import qwen3_moe_ref as mr
from tests import route_exact as rx
from tests.test_gpu_prefill_paged import HEAD_LENS, compare_with_whole, prompts_of, release, rows_of
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

PAGE = 16


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


def build(kv="bf16", max_reqs=8, max_seq_len=256, tmp_path=None, tiled_floor=None):
    """A Qwen3MoeDecoder of the fixture's shape with the fixture's weights, page 16, and a cache of its own.  tmp_path: the
    weights travel through an HF directory and load_checkpoint_hf_qwen3_moe instead of a direct copy."""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.checkpoint import load_checkpoint_hf_qwen3_moe
    from chitu_amd.qwen3_moe import Qwen3MoeDecoder

    g, cfg = mr.fixture()
    args = mr.moe_args(cfg, kv_cache_dtype=kv)
    shape, dtype = gqa_kv_layout(kv, args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=PAGE, max_seq_len=max_seq_len, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = Qwen3MoeDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq_len),
                            max_position_embeddings=max_seq_len, device="cuda")
    hf = mr.hf_params(g)
    if tmp_path is not None:
        load_checkpoint_hf_qwen3_moe(model, mr.write_hf_dir(hf, str(tmp_path / "qwen3_moe")))
    else:
        p = mr.module_params(hf, args)
        params = dict(model.named_parameters())
        assert set(params) == set(p)
        for k, t in params.items():
            t.data.copy_(p[k])
    if tiled_floor is not None:
        for layer in model.layers:
            layer.ffn.tiled_min_tokens = tiled_floor
    return model, cache, g, cfg, hf


def record(model):
    logs = []
    for layer in model.layers:
        layer.ffn.record_routing = []
        logs.append(layer.ffn.record_routing)
    return logs


def stop_recording(model):
    for layer in model.layers:
        layer.ffn.record_routing = None


def check_router(logs, model, cfg, what):
    """Every recorded call of every layer: the bf16 logits are within one bf16 ulp of the fp64 product of the recorded input
    with the gate; ids and weights are route_exact's oracle on the recorded bf16 logits (ids exactly, in rank order, ties to
    the lower expert; weights by its softmax rule).  Returns the ids [layers, tokens, top_k] in call order."""
    top_k, E = cfg["num_experts_per_tok"], cfg["num_experts"]
    case = rx.Case("qwen3_moe", "recorded", E, topk=top_k, score=rx.RENORM if cfg["norm_topk_prob"] else rx.SOFTMAX, scale=1.0)
    all_ids, worst_ulp, ties, strict = [], 0.0, 0, []
    for layer, calls in zip(model.layers, logs):
        gate64 = layer.ffn.gate.detach().double().cpu()
        x = torch.cat([c[0] for c in calls]).cpu()
        logits = torch.cat([c[1] for c in calls]).cpu()
        ids = torch.cat([c[2] for c in calls]).cpu()
        w = torch.cat([c[3] for c in calls]).cpu()
        assert logits.dtype == torch.bfloat16 and tuple(ids.shape) == tuple(w.shape) == (x.shape[0], top_k)
        exact = (x.double() @ gate64.T).numpy()
        ulps = np.abs(logits.double().numpy() - exact) / rx.bf16_ulp64(np.where(exact == 0, 1e-30, exact))
        worst_ulp = max(worst_ulp, float(ulps.max()))
        assert float(ulps.max()) <= 1.0, (what, float(ulps.max()))
        want = rx.spec(case, logits.float().numpy(), None)
        ties += int(want["cut_tie"].sum())
        assert np.array_equal(ids.numpy(), want["ids"]), (what, "router ids differ from the oracle on the recorded logits")
        ok, share = rx.softmax_weight_ok(want["w64"], rx.bf16_bits(w.float().numpy()))
        strict.append(share)
        assert bool(ok.all()), (what, int((~ok).sum()), "router weights are no bf16 neighbour of the float64 value")
        all_ids.append(ids)
    print(f"QWEN3-MOE router {what}: {all_ids[0].shape[0]} tokens x {len(logs)} layers, logits within {worst_ulp:.3f} bf16 ulp of fp64, "
          f"ids == oracle ({ties} exact ties at the cut), weights ok (strict share {min(strict):.3f})")
    return torch.stack(all_ids)


def teacher_forced(model, cache, prompt, toks, req, use_graph):
    rows = [model.prefill([prompt], [req]).float().cpu()]
    for step in range(len(toks) - 1):
        cache.prepare_cache_decode([req])
        cache.prepare_block_table_for_decode([req])
        tok = torch.tensor([toks[step]], dtype=torch.int64, device="cuda")
        rows.append(model.decode(tok, use_graph=use_graph).float().cpu())
        cache.finalize_cache_single_decode([req])
    cache.finalize_cache_all_decode(req)
    return torch.cat(rows)


def test_router_is_exact_and_logits_meet_the_forced_routing_bar_and_graph_decode_is_eager_decode(tmp_path):
    """Eager prefill of the prompt and 32 teacher-forced eager decode steps with record_routing on, through the checkpoint
    loader; then the same steps as hipGraph replays (the hook off: it is eager only)."""
    model, cache, g, cfg, hf = build(max_reqs=2, max_seq_len=64, tmp_path=tmp_path)
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    fed = prompt + toks[:-1]
    logs = record(model)
    eager = teacher_forced(model, cache, prompt, toks, "e", use_graph=False)
    stop_recording(model)
    ids = check_router(logs, model, cfg, "prefill + 32 decode steps")
    assert tuple(ids.shape) == (cfg["num_hidden_layers"], len(fed), cfg["num_experts_per_tok"])
    same_as_fp32 = (ids.sort(-1).values == torch.from_numpy(g["router_ids"]).long().sort(-1).values).all(-1)
    ref = mr.forward(hf, fed, cfg, route_ids=ids)[0][len(prompt) - 1:]
    print(f"QWEN3-MOE (layer, token) pairs routed as in HF's fp32 run: {int(same_as_fp32.sum())} of {same_as_fp32.numel()}")
    mr.check_logits(eager, ref, "HIP eager vs the fp32 restatement forced to the engine's ids")
    # the run without the hook is the run with it (the hook feeds the router the same bf16 logits as one fp32 plane) ...
    plain = teacher_forced(model, cache, prompt, toks, "p", use_graph=False)
    same = int((plain == eager).all(-1).sum())
    print(f"QWEN3-MOE eager rows identical with and without record_routing: {same} / 33")
    mr.check_logits(plain, ref, "HIP eager (no hook) vs the same restatement")
    # ... and graph decode equals eager decode bit for bit
    graph = teacher_forced(model, cache, prompt, toks, "g", use_graph=True)
    print(f"QWEN3-MOE graph replay rows identical to eager launches: {int((graph == plain).all(-1).sum())} / 33")
    assert torch.equal(graph, plain)


def test_tiled_prefill_routes_like_the_streaming_prefill_and_meets_the_forced_routing_bar():
    """A 130-token prompt: 520 slots >= 24 x 16, so with the floor at 1 both expert GEMMs of both layers take the tiled form
    (checked in the C-ABI call log); floor 0 is the streaming form.  Layer 0 sees the same input either way; further down,
    ids are compared wherever the recorded logits are equal."""
    from chitu_amd import _lib

    prompt = prompts_of(512, lens=(130,), seed=11)[0]
    out, logs_of, ids_of = {}, {}, {}
    for floor in (0, 1):
        model, cache, g, cfg, hf = build(max_reqs=2, tiled_floor=floor)
        logs = record(model)
        _lib.call_log = []
        try:
            out[floor] = model.prefill([prompt], ["t"]).float().cpu()
            called = {n for n, _ in _lib.call_log if "moe_gemm" in n}
        finally:
            _lib.call_log = None
        assert called == ({"chitu_ext3_moe_gemm1_silu_bf16_tiled", "chitu_ext3_moe_gemm2_bf16_tiled"} if floor else {"chitu_hip_moe_gemm_bf16"}), called
        stop_recording(model)
        ids_of[floor] = check_router(logs, model, cfg, f"130-token prefill, tiled floor {floor}")
        logs_of[floor] = [torch.cat([c[1] for c in calls]).cpu() for calls in logs]
        release(cache)
        ref = mr.forward(hf, prompt, cfg, route_ids=ids_of[floor])[0][-1:]
        mr.check_logits(out[floor], ref, f"130-token prefill, tiled floor {floor}, vs the fp32 restatement forced to its ids")
        del model, cache
    assert torch.equal(logs_of[0][0], logs_of[1][0]), "layer 0's router saw different logits"
    for layer in range(len(logs_of[0])):
        same = (logs_of[0][layer] == logs_of[1][layer]).all(-1)
        assert torch.equal(ids_of[0][layer][same], ids_of[1][layer][same]), layer
        print(f"QWEN3-MOE tiled vs streaming prefill, layer {layer}: {int(same.sum())} of {same.numel()} tokens with equal router logits, "
              f"equal ids on all of them")
    print(f"QWEN3-MOE tiled vs streaming prefill logits: {assert_close(out[1], out[0], 3e-2, what='tiled vs streaming'):.3e}")


A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]


def test_prefill_continue_of_a_tail_is_the_whole_prefill():
    model, cache, *_ = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "qwen3-moe split", elementwise=False)
    release(cache)


def test_chunked_prefill_is_the_whole_prefill():
    model, cache, *_ = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    got = model.prefill(prompts, B, chunk_size=16)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "qwen3-moe chunk_size=16", elementwise=False)
    release(cache)


def test_one_multi_token_step_is_three_single_token_steps():
    """tests/test_gpu_llama_multi.py's comparison and bars: logits per position at 3e-2, the appended rows at 1e-2."""
    model, cache, *_ = build()
    vocab, T = model.args.vocab_size, 3
    prompts = prompts_of(vocab)
    model.prefill(prompts, A)
    model.prefill(prompts, B)
    tokens = torch.randint(0, vocab, (3, T), generator=torch.Generator().manual_seed(T)).cuda()
    cache.prepare_block_table_for_decode_multi(A, T)
    multi = model.decode_multi(tokens, use_graph=False).clone()
    cache.finalize_cache_multi_decode(A, [T] * 3)
    for t in range(T):
        cache.prepare_cache_decode(B)
        cache.prepare_block_table_for_decode(B)
        single = model.decode(tokens[:, t].contiguous(), use_graph=False)
        cache.finalize_cache_single_decode(B)
        print(f"QWEN3-MOE decode_multi position {t}: {assert_close(multi[:, t], single, 3e-2, what=('multi', t)):.3e}")
    for a, b, p in zip(A, B, prompts):
        n = len(p) + T
        assert cache.seq_lens[a] == cache.seq_lens[b] == n
        assert_close(rows_of(cache, a, n)[:, :, len(p):], rows_of(cache, b, n)[:, :, len(p):], 1e-2, what=("rows", a))
    release(cache)


def test_fp8_kv_cache_decodes_and_generates():
    """kv_cache_dtype="fp8": layer 0's page rows are the quantised rows of the bf16 model bit for bit (they depend on no
    attention and no expert), the decode logits are finite, generate returns its pages."""
    from chitu_amd import ops

    m16, c16, *_ = build()
    m8, c8, *_ = build(kv="fp8")
    prompts = prompts_of(m16.args.vocab_size)
    logits = {}
    for key, model, cache in (("bf16", m16, c16), ("fp8", m8, c8)):
        model.prefill(prompts, A)
        for step in range(4):
            cache.prepare_cache_decode(A)
            cache.prepare_block_table_for_decode(A)
            logits[key] = model.decode(torch.full((3,), 7 + step, dtype=torch.int64, device="cuda"), use_graph=False).float().cpu()
            cache.finalize_cache_single_decode(A)
    for r, p in zip(A, prompts):
        r16, r8 = rows_of(c16, r, len(p) + 4), rows_of(c8, r, len(p) + 4)
        for i, name in enumerate("KV"):
            assert torch.equal(r8[i, 0], ops.gqa_kv_quant_fp8(r16[i, 0].contiguous())), (r, name)
    assert bool(torch.isfinite(logits["fp8"]).all())
    # (recorded only: one flipped expert behind an fp8 K / V row moves a logit by more than any fp8 bar)
    print(f"QWEN3-MOE fp8 KV cache, 4th decode step vs the bf16 cache, of the peak: {max_rel_to_peak(logits['fp8'], logits['bf16']):.3e}")
    release(c16), release(c8)
    free = len(c8.free_blocks)
    out = m8.generate(prompts, 4)
    assert tuple(out.shape) == (3, 4) and len(c8.free_blocks) == free and not c8.seq_lens
