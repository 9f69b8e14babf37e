"""Glm4Decoder on the GPU: against Hugging Face's GlmForCausalLM (tests/golden/glm4_hf.npz, made on the CPU by
tests/golden/gen_glm4_hf.py: 4 query heads over 2 kv heads, a bias on q / k / v, the first 64 channels of a head rotated) through
the checkpoint loader under both key namings, and against itself -- continued and chunked prefill, decode_multi, the fp8 K / V
cache, graph capture, W8A16.  The bars of the self-comparisons are tests/test_gpu_qwen2.py's and tests/test_gpu_w8a16_model.py's."""

import gc

import pytest
import torch

from tests import glm4_exact as gx
from tests import glm4_ref as g4
from tests.test_gpu_prefill_paged import HEAD_LENS, compare_with_whole, prompts_of, release, rows_of
from tests.util import assert_close

pytestmark = pytest.mark.gpu

PAGE = 16
A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


def build(kv="bf16", max_reqs=8, path=None, **over):
    """A Glm4Decoder of the fixture's shape (hidden 512, 4 / 2 heads of 128, rotary_dim 64), page 16, a cache of its own, and the
    fixture's weights: copied in through the loader's steps, or -- path given -- loaded from that safetensors directory."""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.glm4 import Glm4Decoder

    g, cfg = g4.fixture()
    args = g4.glm4_args(cfg, kv_cache_dtype=kv, **over)
    shape, dtype = gqa_kv_layout(kv, args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=PAGE, max_seq_len=256, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = Glm4Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=256), max_position_embeddings=256, device="cuda")
    assert model.cos_table.shape == (256, 32) and model.layers[0].attn.rotary_type == "glm4"
    if path is not None:
        load_checkpoint_hf_llama(model, path)
        return model, cache
    p = g4.module_params(g4.glm4_hf_params(g), args)
    params = dict(model.named_parameters())
    assert set(params) == set(p) and any("bqkv" in k for k in params)
    for k, t in params.items():
        assert t.shape == p[k].shape, k
        t.data.copy_(p[k])
    return model, cache


def decode_step(model, cache, reqs, tokens, use_graph):
    cache.prepare_cache_decode(reqs)
    cache.prepare_block_table_for_decode(reqs)
    out = model.decode(tokens, use_graph=use_graph).clone()
    cache.finalize_cache_single_decode(reqs)
    return out


def test_hf_checkpoint_reproduces_the_hf_fp32_run_under_both_key_namings(tmp_path):
    """Parameters regenerated from the seed, written as a safetensors directory under Hugging Face's native names and loaded by
    load_checkpoint_hf_llama; prefill of the prompt, then 32 decode steps fed the fixture's tokens, as one hipGraph replay per step
    and as eager launches.  The same parameters under the ChatGLM remote-code names load to the same logits bit for bit."""
    g, _ = g4.fixture()
    hf = g4.glm4_hf_params(g)
    model, cache = build(max_reqs=2, path=g4.write_hf_dir(hf, str(tmp_path / "glm4-hf")))
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    k0, v0 = torch.from_numpy(g["k0_fp32"]), torch.from_numpy(g["v0_fp32"])

    def run(req, use_graph):
        rows = [model.prefill([prompt], [req]).float().cpu()]
        for step in range(32):
            tok = torch.tensor([toks[step]], dtype=torch.int64, device="cuda")
            rows.append(decode_step(model, cache, [req], tok, use_graph).float().cpu())
        assert cache.seq_lens[req] == len(prompt) + 32 == k0.shape[0]
        kv_rows = rows_of(cache, req, k0.shape[0])[:, 0].float().cpu()  # K and V, layer 0
        cache.finalize_cache_all_decode(req)
        return torch.cat(rows), kv_rows

    (graph, kv_graph), (eager, kv_eager) = run("g", True), run("e", False)
    same = int((graph == eager).all(-1).sum())
    print("GLM4 graph replay rows identical to eager launches:", same, "/ 33")
    g4.check_logits(eager, g, "GLM4 HIP eager vs HF fp32")
    g4.check_logits(graph, g, "GLM4 HIP graph vs HF fp32")
    assert same == 33 and torch.equal(kv_graph, kv_eager)
    print("GLM4 layer-0 K page rows vs HF fp32:", assert_close(kv_eager[0], k0, 1e-2, what="layer 0 K page rows"))
    print("GLM4 layer-0 V page rows vs HF fp32:", assert_close(kv_eager[1], v0, 1e-2, what="layer 0 V page rows"))
    # the ChatGLM naming into the same module: the same parameters bit for bit, so the same logits bit for bit
    native = {k: p.detach().clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.data.zero_()
    from chitu_amd.checkpoint import load_checkpoint_hf_llama

    load_checkpoint_hf_llama(model, g4.write_hf_dir(g4.chatglm_names(hf), str(tmp_path / "glm4-chat")))
    for k, p in model.named_parameters():
        assert torch.equal(p, native[k]), k
    again = model.prefill([prompt], ["c"]).float().cpu()
    cache.finalize_cache_all_decode("c")
    assert torch.equal(again, eager[:1])
    release(cache)


def test_greedy_decode_gives_the_fixtures_tokens_where_the_margin_is_clear_and_graph_is_eager():
    """Free-running greedy generation of 33 tokens under graph capture and as eager launches: the same tokens.  A row is comparable
    with the fixture while every earlier token is the fixture's, and binding when the fixture's top-2 margin exceeds twice the
    logits bar (tests/test_gpu_qwen2.py's rule)."""
    model, cache = build()
    g, _ = g4.fixture()
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    free = len(cache.free_blocks)
    out = model.generate([prompt], len(toks), use_graph=True)
    assert torch.equal(out, model.generate([prompt], len(toks), use_graph=False))
    out = out[0].tolist()
    ref = torch.from_numpy(g["logits_fp32"])
    top2 = ref.topk(2, -1).values
    clear = ((top2[:, 0] - top2[:, 1]) / ref.abs().amax(-1) > 2 * g4.LOGITS_BAR).tolist()
    compared = bound = 0
    for i, (mine, want) in enumerate(zip(out, toks)):
        compared += 1
        if clear[i]:
            bound += 1
            assert mine == want, (i, out, toks)
        if mine != want:
            break
    print(f"GLM4 greedy generate: {compared} of {len(toks)} rows on the fixture's history, {bound} of them with a clear margin, all equal")
    assert bound >= 2 and len(cache.free_blocks) == free and not cache.seq_lens


def test_layer0_page_rows_are_the_oracles_rows_bit_for_bit():
    """Layer 0's projection depends on no attention: its qkv rows recomputed with the decoder's own norm and GEMM launches, then
    tests/glm4_exact.py's oracle on the CPU -- bias, the first 64 channels rotated by the decoder's table, the rest and v passed
    through -- against the K / V page rows that prefill (the one-launch form) and two decode steps (the decode form) left."""
    from chitu_amd import ops
    from chitu_amd import tensor_parallel as tp

    model, cache = build()
    prompt = prompts_of(model.args.vocab_size)[0]
    model.prefill([prompt], ["r"])
    extra = [11, 12]
    for t in extra:
        decode_step(model, cache, ["r"], torch.tensor([t], dtype=torch.int64, device="cuda"), False)
    n = len(prompt) + len(extra)
    rows = rows_of(cache, "r", n)[:, 0].cpu()  # [2, n, hkv, 128]
    layer, hq, hkv = model.layers[0], model.args.n_heads, model.args.n_kv_heads
    pos = torch.arange(n)
    cos, sin = model.cos_table.cpu()[pos].contiguous(), model.sin_table.cpu()[pos].contiguous()
    for lo, hi, tokens in ((0, len(prompt), prompt), (len(prompt), len(prompt) + 1, extra[:1]), (len(prompt) + 1, n, extra[1:])):
        x = model.embed(torch.tensor(tokens, dtype=torch.int64, device="cuda"))
        hn = tp.add_norm(x, None, layer.attn_norm, layer.eps)[1]
        qkv = ops.bf16_linear(hn, layer.attn.wqkv).cpu().view(hi - lo, hq + 2 * hkv, 128)
        y = gx.add_bias(qkv, layer.attn.bqkv.cpu())
        want_k = gx.rotate_partial(y[:, hq:hq + hkv].contiguous(), cos[lo:hi], sin[lo:hi])
        assert torch.equal(gx.bits(rows[0, lo:hi]), gx.bits(want_k)), ("K", lo, hi)
        assert torch.equal(gx.bits(rows[1, lo:hi]), gx.bits(y[:, hq + hkv:].contiguous())), ("V", lo, hi)
        assert torch.equal(gx.bits(rows[0, lo:hi, :, 64:]), gx.bits(y[:, hq:hq + hkv, 64:].contiguous()))
    print(f"GLM4 layer-0 K / V page rows == the oracle's, bit for bit: {len(prompt)} prefill rows, {len(extra)} decode rows")
    release(cache)


def test_prefill_continue_of_a_tail_is_the_whole_prefill():
    model, cache = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "glm4 split")
    release(cache)


def test_chunked_prefill_is_the_whole_prefill():
    model, cache = build()
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    got = model.prefill(prompts, B, chunk_size=16)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "glm4 chunk_size=16")
    release(cache)


def test_one_multi_token_step_is_three_single_token_steps():
    """tests/test_gpu_qwen2.py's comparison and bars: logits per position at 3e-2, the appended rows at 1e-2."""
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
        single = decode_step(model, cache, B, tokens[:, t].contiguous(), False)
        print(f"GLM4 decode_multi position {t}: {assert_close(multi[:, t], single, 3e-2, what=('multi', t)):.3e}")
    for a, b, p in zip(A, B, prompts):
        n = len(p) + T
        assert cache.seq_lens[a] == cache.seq_lens[b] == n
        assert_close(rows_of(cache, a, n)[:, :, len(p):], rows_of(cache, b, n)[:, :, len(p):], 1e-2, what=("rows", a))
    release(cache)


def test_fp8_cache_rows_are_the_quantised_rows_of_the_bf16_model_and_its_logits_agree():
    """tests/test_gpu_qwen2.py's comparison: prefill attends over the unquantised rows in both modes, so the fp8 model's prompt
    rows are the quantised image of the bf16 model's bit for bit (and so are layer 0's decode rows), and the prefill logits are
    the bf16 model's; the decode logits over the quantised cache stay within the self-comparison bar of 3e-2."""
    from chitu_amd import ops

    m16, c16 = build()
    m8, c8 = build(kv="fp8")
    prompts = prompts_of(m16.args.vocab_size)
    logits = {}
    for name, model, cache in (("bf16", m16, c16), ("fp8", m8, c8)):
        logits[name] = [model.prefill(prompts, A).clone()]
        for step in range(4):
            logits[name].append(decode_step(model, cache, A, torch.full((3,), 7 + step, dtype=torch.int64, device="cuda"), False))
    assert torch.equal(logits["bf16"][0], logits["fp8"][0])
    for step in range(1, 5):
        print(f"GLM4 fp8-cache decode step {step - 1} vs the bf16 cache: {assert_close(logits['fp8'][step], logits['bf16'][step], 3e-2, what=('fp8', step)):.3e}")
    for r, p in zip(A, prompts):
        r16, r8 = rows_of(c16, r, len(p) + 4), rows_of(c8, r, len(p) + 4)  # [2, layers, rows, hkv, 128 | 144]
        for i, name in enumerate("KV"):
            for layer in range(r16.shape[1]):
                want = ops.gqa_kv_quant_fp8(r16[i, layer, :len(p)].contiguous())
                assert torch.equal(r8[i, layer, :len(p)], want), (r, name, layer)
            # the decode rows of layer 0 depend on no attention either
            assert torch.equal(r8[i, 0, len(p):], ops.gqa_kv_quant_fp8(r16[i, 0, len(p):].contiguous())), (r, name, "decode rows")
    release(c16), release(c8)


def test_w8a16_builds_and_matches_its_bf16_twin(tmp_path):
    """tests/test_gpu_w8a16_model.py's comparison and logits bar (3e-2 of the peak): the fixture's model quantised in place against
    a twin whose four linears per layer hold bf16(dequant(q, s)); prefill and four decode steps, the last under graph capture."""
    from chitu_amd.quantize import dequant_weight_w8a16, quantize_w8a16_
    from chitu_amd.quantize.w8a16 import W8A16_WEIGHTS
    from tests.test_gpu_w8a16_model import LOGITS_BAR

    mq, cq = build()
    mt, ct = build()
    quantize_w8a16_(mq)
    assert mq.args.quant == "w8a16" and mq.layers[0].attn.wqkv.dtype == torch.int8 and mq.layers[0].attn.bqkv.dtype == torch.bfloat16
    for lq, lt in zip(mq.layers, mt.layers):
        for part, name in W8A16_WEIGHTS:
            q, s = getattr(getattr(lq, part), name), getattr(getattr(lq, part), name + "_scale")
            getattr(getattr(lt, part), name).data.copy_(dequant_weight_w8a16(q, s).to(torch.bfloat16))
    prompts = prompts_of(mq.args.vocab_size)
    lq, lt = mq.prefill(prompts, A).clone(), mt.prefill(prompts, A).clone()
    print(f"GLM4 w8a16 prefill logits vs the bf16 twin: {assert_close(lq, lt, LOGITS_BAR, what='w8a16 prefill'):.3e}")
    g = torch.Generator().manual_seed(11)
    for step in range(4):
        tok = torch.randint(0, mq.args.vocab_size, (3,), generator=g).cuda()
        dq, dt = decode_step(mq, cq, A, tok, step == 3), decode_step(mt, ct, A, tok, False)
        print(f"GLM4 w8a16 decode step {step} vs the bf16 twin: {assert_close(dq, dt, LOGITS_BAR, what=('w8a16 decode', step)):.3e}")
    release(cq), release(ct)
    # built with quant="w8a16" and filled by the loader from the bf16 files (llama_to_w8a16 quantises on the host): the same
    # parameters by name, shape and type, and the twin's prefill logits under the same bar
    g_, _ = g4.fixture()
    ml, cl = build(path=g4.write_hf_dir(g4.glm4_hf_params(g_), str(tmp_path / "glm4-hf")), quant="w8a16")
    loaded = dict(ml.named_parameters())
    assert {k: (p.dtype, p.shape) for k, p in mq.named_parameters()} == {k: (p.dtype, p.shape) for k, p in loaded.items()}
    print(f"GLM4 w8a16 through the loader, prefill logits vs the bf16 twin: {assert_close(ml.prefill(prompts, A), lt, LOGITS_BAR, what='w8a16 loaded'):.3e}")
    release(cl)


def test_full_size_shapes_pass_the_decoders_asserts_without_allocation():
    """Glm4Args() -- glm-4-9b-chat -- on the meta device, unsharded: 32 / 2 heads (G = 16), 36 heads of 128 in the merged projection."""
    from chitu_amd.glm4 import Glm4Args, Glm4Decoder

    args = Glm4Args(n_layers=2)  # every layer has the same shapes
    m = Glm4Decoder(args, None, None, max_position_embeddings=8, device="meta")
    a = m.layers[0].attn
    assert (a.hq, a.hkv, a.hd) == (32, 2, 128) and tuple(a.wqkv.shape) == (36 * 128, 4096) and tuple(a.bqkv.shape) == (36 * 128,)
    assert tuple(m.layers[0].ffn.w13.shape) == (2 * 13696, 4096) and tuple(m.embed_weight.shape) == (151552, 4096)
    assert tuple(m.cos_table.shape) == (8, 32) and Glm4Args().n_layers == 40 and all(p.is_meta for p in m.parameters())
