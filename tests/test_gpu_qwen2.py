"""Qwen2Decoder on the GPU: against Hugging Face's Qwen2ForCausalLM (tests/golden/qwen2_hf.npz, made on the CPU by
tests/golden/gen_qwen2_hf.py: 7 query heads over 1 kv head, a bias on q / k / v) through the checkpoint loader, and against
itself -- continued and chunked prefill, decode_multi, the fp8 K / V cache, greedy generation.  The bars of the self-comparisons
are tests/test_gpu_qwen3.py's."""

import gc

import pytest
import torch

from tests import qwen2_ref as q2
from tests.test_gpu_prefill_paged import HEAD_LENS, compare_with_whole, prompts_of, release, rows_of
from tests.util import assert_close

pytestmark = pytest.mark.gpu

PAGE = 16


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


def build(n_layers=2, kv="bf16", max_reqs=8):
    """A Qwen2Decoder of the fixture's shape (hidden 896, 7 / 1 heads of 128) with the fixture's weights (the first n_layers
    layers), page 16, and a cache of its own."""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.qwen2 import Qwen2Decoder

    g, cfg = q2.fixture()
    args = q2.qwen2_args(cfg, n_layers=n_layers, kv_cache_dtype=kv)
    shape, dtype = gqa_kv_layout(kv, args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=PAGE, max_seq_len=256, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = Qwen2Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=256), max_position_embeddings=256, device="cuda")
    p = q2.module_params(q2.qwen2_hf_params(g), args)
    params = dict(model.named_parameters())
    assert set(params) <= set(p) and any("bqkv" in k for k in params)
    for k, t in params.items():
        assert t.shape == p[k].shape, k
        t.data.copy_(p[k])
    return model, cache


def test_hf_checkpoint_reproduces_the_hf_fp32_run(tmp_path):
    """Parameters regenerated from the seed, written as an HF-named safetensors directory, loaded by load_checkpoint_hf_llama;
    prefill of the prompt, then 32 decode steps fed the fixture's tokens, as one hipGraph replay per step and as eager launches."""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.qwen2 import Qwen2Decoder

    g, cfg = q2.fixture()
    args = q2.qwen2_args(cfg)
    path = q2.write_hf_dir(q2.qwen2_hf_params(g), str(tmp_path / "qwen2"))
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=2, block_size=PAGE, max_seq_len=64, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = Qwen2Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=64), max_position_embeddings=64, device="cuda")
    load_checkpoint_hf_llama(model, path)
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    k0, v0 = torch.from_numpy(g["k0_fp32"]), torch.from_numpy(g["v0_fp32"])

    def run(req, use_graph):
        rows = [model.prefill([prompt], [req]).float().cpu()]
        for step in range(32):
            cache.prepare_cache_decode([req])
            cache.prepare_block_table_for_decode([req])
            tok = torch.tensor([toks[step]], dtype=torch.int64, device="cuda")
            rows.append(model.decode(tok, use_graph=use_graph).float().cpu())
            cache.finalize_cache_single_decode([req])
        assert cache.seq_lens[req] == len(prompt) + 32 == k0.shape[0]
        kv_rows = rows_of(cache, req, k0.shape[0])[:, 0].float().cpu()  # K and V, layer 0
        cache.finalize_cache_all_decode(req)
        return torch.cat(rows), kv_rows

    (graph, kv_graph), (eager, kv_eager) = run("g", True), run("e", False)
    same = int((graph == eager).all(-1).sum())
    print("QWEN2 graph replay rows identical to eager launches:", same, "/ 33")
    q2.check_logits(eager, g, "Qwen2 HIP eager vs HF fp32")
    q2.check_logits(graph, g, "Qwen2 HIP graph vs HF fp32")
    assert same == 33 and torch.equal(kv_graph, kv_eager)
    print("QWEN2 layer-0 K page rows vs HF fp32:", assert_close(kv_eager[0], k0, 1e-2, what="layer 0 K page rows"))
    print("QWEN2 layer-0 V page rows vs HF fp32:", assert_close(kv_eager[1], v0, 1e-2, what="layer 0 V page rows"))


# ---------------------------------------------------------------- the engine against itself
A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]


def test_prefill_continue_of_a_tail_is_the_whole_prefill():
    model, cache = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "qwen2 split")
    release(cache)


def test_chunked_prefill_is_the_whole_prefill():
    model, cache = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    got = model.prefill(prompts, B, chunk_size=7)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "qwen2 chunk_size=7")
    release(cache)


def test_one_multi_token_step_is_three_single_token_steps():
    """tests/test_gpu_llama_multi.py's comparison and bars: logits per position at 3e-2, the appended rows at 1e-2."""
    model, cache = build()
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
        print(f"QWEN2 decode_multi position {t}: {assert_close(multi[:, t], single, 3e-2, what=('multi', t)):.3e}")
    for a, b, p in zip(A, B, prompts):
        n = len(p) + T
        assert cache.seq_lens[a] == cache.seq_lens[b] == n
        assert_close(rows_of(cache, a, n)[:, :, len(p):], rows_of(cache, b, n)[:, :, len(p):], 1e-2, what=("rows", a))
    release(cache)


def test_fp8_cache_rows_are_the_quantised_rows_of_the_bf16_model():
    """Prefill attends over the unquantised rows in both modes, so every layer's prompt rows are the same bf16 rows: the fp8
    model's page rows are their quantised image bit for bit, and four decode steps behind them leave them alone."""
    from chitu_amd import ops

    m16, c16 = build()
    m8, c8 = build(kv="fp8")
    prompts = prompts_of(m16.args.vocab_size)
    for model, cache in ((m16, c16), (m8, c8)):
        model.prefill(prompts, A)
        for step in range(4):
            cache.prepare_cache_decode(A)
            cache.prepare_block_table_for_decode(A)
            model.decode(torch.full((3,), 7 + step, dtype=torch.int64, device="cuda"), use_graph=False)
            cache.finalize_cache_single_decode(A)
    for r, p in zip(A, prompts):
        r16, r8 = rows_of(c16, r, len(p) + 4), rows_of(c8, r, len(p) + 4)  # [2, layers, rows, hkv, 128 | 144]
        for i, name in enumerate("KV"):
            for layer in range(r16.shape[1]):
                want = ops.gqa_kv_quant_fp8(r16[i, layer, :len(p)].contiguous())
                assert torch.equal(r8[i, layer, :len(p)], want), (r, name, layer)
            # the decode rows of layer 0 depend on no attention either
            assert torch.equal(r8[i, 0, len(p):], ops.gqa_kv_quant_fp8(r16[i, 0, len(p):].contiguous())), (r, name, "decode rows")
    release(c16), release(c8)


def test_greedy_generate_gives_the_fixtures_tokens_where_the_margin_is_clear():
    """Free-running greedy generation of 33 tokens.  A row is comparable while every earlier token is the fixture's (the same
    history), and binding when the fixture's top-2 margin exceeds twice the logits bar: both sides may move a logit by the bar."""
    model, cache = build()
    g, _ = q2.fixture()
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    free = len(cache.free_blocks)
    out = model.generate([prompt], len(toks))[0].tolist()
    ref = torch.from_numpy(g["logits_fp32"])
    top2 = ref.topk(2, -1).values
    clear = ((top2[:, 0] - top2[:, 1]) / ref.abs().amax(-1) > 2 * q2.LOGITS_BAR).tolist()
    compared = bound = 0
    for i, (mine, want) in enumerate(zip(out, toks)):
        compared += 1
        if clear[i]:
            bound += 1
            assert mine == want, (i, out, toks)
        if mine != want:
            break
    print(f"QWEN2 greedy generate: {compared} of {len(toks)} rows on the fixture's history, {bound} of them with a clear margin, all equal")
    assert bound >= 2 and len(cache.free_blocks) == free and not cache.seq_lens
