"""W8A16 decoders on the GPU: tiny Llama / Qwen2 / Qwen3 models (2 layers, dim 256, 2 / 1 heads of 128, ffn 512, vocab 512,
page 16) after quantize_w8a16_, against a bf16 twin whose four linears per layer hold bf16(dequant(q, s)).  The bars are the
ones tests/test_gpu_prefill_paged.py::compare_with_whole uses between two runs of one model: logits within 3e-2 of the peak,
K / V page rows within 1e-2 per element.  With the quantiser's scales the twin differs from the W8A16 model by the rounding of
q * s to bf16 (the int8 model multiplies the fp32 accumulator by the fp32 scale): the logits bar is asserted.  With the scales
rounded down to powers of two the twin is the same real arithmetic: the row bars are asserted too."""
import gc

import pytest
import torch

from tests.test_gpu_prefill_paged import HEAD_LENS, prompts_of, release, rows_of
from tests.util import assert_close

pytestmark = pytest.mark.gpu

PAGE = 16
A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]
SHAPE = dict(dim=256, n_layers=2, n_heads=2, n_kv_heads=1, vocab_size=512, ffn_dim=512)
LOGITS_BAR, ROWS_BAR = 3e-2, 1e-2  # compare_with_whole's


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


def _decoder(kind, kv="bf16", seed=0, **extra):
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.llama import LlamaArgs, LlamaDecoder, init_synthetic_
    from chitu_amd.qwen2 import Qwen2Args, Qwen2Decoder
    from chitu_amd.qwen3 import Qwen3Args, Qwen3Decoder

    args_t, dec_t = {"llama": (LlamaArgs, LlamaDecoder), "qwen2": (Qwen2Args, Qwen2Decoder), "qwen3": (Qwen3Args, Qwen3Decoder)}[kind]
    args = args_t(kv_cache_dtype=kv, **SHAPE, **extra)
    shape, dtype = gqa_kv_layout(kv, args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=8, block_size=PAGE, max_seq_len=512, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = dec_t(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=512), max_position_embeddings=512, device="cuda")
    init_synthetic_(model, seed=seed)
    return model, cache


def pair(kind, kv="bf16", pow2=False):
    """(W8A16 model, its cache, bf16 twin, its cache): the same synthetic weights, the first quantised in place, the twin's
    four linears per layer overwritten with bf16(dequant) of the first's codes.  pow2: every scale is first rounded down to a
    power of two -- then bf16(q * s) IS q * s and the twin computes the same real numbers as the int8 model (the scale commutes
    with every rounding), the two differing only in the order of fp32 summation, like two runs of one bf16 model."""
    from chitu_amd.quantize import dequant_weight_w8a16, quantize_w8a16_
    from chitu_amd.quantize.w8a16 import W8A16_WEIGHTS

    mq, cq = _decoder(kind, kv)
    mt, ct = _decoder(kind, kv)
    quantize_w8a16_(mq)
    assert mq.args.quant == "w8a16" and mt.args.quant is None
    for lq, lt in zip(mq.layers, mt.layers):
        for part, name in W8A16_WEIGHTS:
            q, s = getattr(getattr(lq, part), name), getattr(getattr(lq, part), name + "_scale")
            assert q.dtype == torch.int8 and s.dtype == torch.float32
            if pow2:
                s.data.copy_(torch.exp2(torch.floor(torch.log2(s.data))))
                assert torch.equal(dequant_weight_w8a16(q, s).to(torch.bfloat16).float(), dequant_weight_w8a16(q, s))
            getattr(getattr(lt, part), name).data.copy_(dequant_weight_w8a16(q, s).to(torch.bfloat16))
    for (kq, pq), (kt, pt) in zip(sorted((k, p) for k, p in mq.named_parameters() if p.dtype == torch.bfloat16),
                                  sorted((k, p) for k, p in mt.named_parameters() if not any(k.endswith(n) for _, n in W8A16_WEIGHTS))):
        assert kq == kt and torch.equal(pq, pt)  # the head, the embedding, the norms, the bias: bf16 and untouched
    return mq, cq, mt, ct


def decode_step(model, cache, reqs, tokens, use_graph):
    cache.prepare_cache_decode(reqs)
    cache.prepare_block_table_for_decode(reqs)
    out = model.decode(tokens, use_graph=use_graph).clone()
    cache.finalize_cache_single_decode(reqs)
    return out


def compare_rows(cq, ct, reqs, lens, tag, first=0):
    for r, n in zip(reqs, lens):
        assert cq.seq_lens[r] == ct.seq_lens[r] == n
        rq, rt = rows_of(cq, r, n)[:, :, first:], rows_of(ct, r, n)[:, :, first:]
        for layer in range(rq.shape[1]):
            for i, name in enumerate("KV"):
                assert_close(rq[i, layer], rt[i, layer], ROWS_BAR, what=(tag, r, name, layer))


def prefill_and_four_steps_against_the_twin(kind, tag, prompt_lens=None, pow2=False):
    """logits at compare_with_whole's 3e-2 of the peak.  pow2 (the twin is the same real arithmetic): also every layer's K / V
    page rows at its 1e-2, per element.  With the quantiser's scales the twin's weights carry a rounding of their own (2^-9
    relative per weight), which compare_with_whole's row bars -- made for two runs over the same weights -- do not cover."""
    mq, cq, mt, ct = pair(kind, pow2=pow2)
    tag = tag + (" pow2" if pow2 else "")
    vocab = mq.args.vocab_size
    prompts = prompts_of(vocab) if prompt_lens is None else prompts_of(vocab, lens=prompt_lens)
    lq, lt = mq.prefill(prompts, A), mt.prefill(prompts, A)
    assert lq.dtype == torch.float32 and tuple(lq.shape) == (3, vocab) and bool(torch.isfinite(lq).all())
    print(f"W8A16MODEL {tag} prefill logits vs the bf16 twin, of the peak: {assert_close(lq, lt, LOGITS_BAR, what=(tag, 'prefill')):.3e}")
    g = torch.Generator().manual_seed(11)
    for step in range(4):
        tok = torch.randint(0, vocab, (3,), generator=g).cuda()
        dq, dt = decode_step(mq, cq, A, tok, False), decode_step(mt, ct, A, tok, False)
        print(f"W8A16MODEL {tag} decode step {step} logits vs the bf16 twin: {assert_close(dq, dt, LOGITS_BAR, what=(tag, 'decode', step)):.3e}")
    if pow2:
        compare_rows(cq, ct, A, [len(p) + 4 for p in prompts], tag)
    release(cq), release(ct)
    return mq, cq


def test_llama_prefill_and_decode_match_the_bf16_twin_and_run_the_int8_kernels():
    from chitu_amd import _lib

    prefill_and_four_steps_against_the_twin("llama", "llama", pow2=True)
    mq, cq = prefill_and_four_steps_against_the_twin("llama", "llama")
    # the launches of one bs-1 decode step: the int8 stream for all four linears of every layer, no bf16 norm-prologue GEMM
    mq.prefill([[1, 2, 3]], ["r"])
    cq.prepare_cache_decode(["r"])
    cq.prepare_block_table_for_decode(["r"])
    _lib.call_log = []
    try:
        mq.decode(torch.tensor([5], dtype=torch.int64, device="cuda"), use_graph=False)
        names = [n for n, _ in _lib.call_log]
    finally:
        _lib.call_log = None
    cq.finalize_cache_single_decode(["r"])
    L = mq.args.n_layers
    assert names.count("chitu_ext6_w8a16_gemm") == 3 * L and names.count("chitu_ext6_w8a16_gemm_silu") == L, names
    assert not [n for n in names if "add_norm" in n and "gemm" in n], names
    assert names.count("chitu_hip_bf16_gemm") == 1  # the head stays bf16
    release(cq)


def test_a_prefill_long_enough_for_the_tiled_form_matches_the_twin():
    """265 prompt rows: every linear of the prefill takes the widen + tiled GEMM + scale_round form"""
    from chitu_amd import ops

    assert ops.w8a16_tiled(150 + 70 + 45, 256, 256)
    prefill_and_four_steps_against_the_twin("llama", "llama-tiled-prefill", prompt_lens=(150, 70, 45))
    prefill_and_four_steps_against_the_twin("llama", "llama-tiled-prefill", prompt_lens=(150, 70, 45), pow2=True)


def test_qwen2_with_its_bias_matches_the_twin():
    prefill_and_four_steps_against_the_twin("qwen2", "qwen2", pow2=True)
    mq, _ = prefill_and_four_steps_against_the_twin("qwen2", "qwen2")
    assert mq.layers[0].attn.qkv_bias and mq.layers[0].attn.bqkv.dtype == torch.bfloat16


def test_qwen3_with_its_head_norm_matches_the_twin():
    prefill_and_four_steps_against_the_twin("qwen3", "qwen3", pow2=True)
    mq, _ = prefill_and_four_steps_against_the_twin("qwen3", "qwen3")
    assert mq.layers[0].attn.qk_norm and mq.layers[0].attn.q_norm.dtype == torch.bfloat16


def test_decode_graph_is_the_eager_step_bit_for_bit_and_generate_agrees():
    mq, cq = _decoder("llama", quant=None)
    from chitu_amd.quantize import quantize_w8a16_

    quantize_w8a16_(mq)
    vocab = mq.args.vocab_size
    prompts = prompts_of(vocab)
    mq.prefill(prompts, A), mq.prefill(prompts, B)
    g = torch.Generator().manual_seed(12)
    for step in range(4):
        tok = torch.randint(0, vocab, (3,), generator=g).cuda()
        eager, graph = decode_step(mq, cq, A, tok, False), decode_step(mq, cq, B, tok, True)
        assert torch.equal(eager, graph), step
    for a, b, p in zip(A, B, prompts):
        assert torch.equal(rows_of(cq, a, len(p) + 4), rows_of(cq, b, len(p) + 4))
    release(cq)
    with_graph = mq.generate(prompts, 6, use_graph=True)
    without = mq.generate(prompts, 6, use_graph=False)
    assert torch.equal(with_graph, without) and tuple(with_graph.shape) == (3, 6)
    assert len(cq.free_blocks) == cq.num_blocks


def test_prefill_continue_and_decode_multi_match_the_twin():
    mq, cq, mt, ct = pair("llama", pow2=True)  # (the row bars need the exact twin; the logits bar holds either way)
    vocab, T = mq.args.vocab_size, 3
    prompts = prompts_of(vocab)
    heads, tails = [p[:h] for p, h in zip(prompts, HEAD_LENS)], [p[h:] for p, h in zip(prompts, HEAD_LENS)]
    outs = []
    for model in (mq, mt):
        model.prefill(heads, A)
        outs.append(model.prefill_continue(tails, A))
    print(f"W8A16MODEL prefill_continue logits vs the bf16 twin: {assert_close(outs[0], outs[1], LOGITS_BAR, what='continue'):.3e}")
    compare_rows(cq, ct, A, [len(p) for p in prompts], "continue")
    tokens = torch.randint(0, vocab, (3, T), generator=torch.Generator().manual_seed(T)).cuda()
    multi = []
    for model, cache in ((mq, cq), (mt, ct)):
        cache.prepare_block_table_for_decode_multi(A, T)
        multi.append(model.decode_multi(tokens, use_graph=False).clone())
        cache.finalize_cache_multi_decode(A, [T] * 3)
    for t in range(T):
        print(f"W8A16MODEL decode_multi position {t} vs the bf16 twin: {assert_close(multi[0][:, t], multi[1][:, t], LOGITS_BAR, what=('multi', t)):.3e}")
    compare_rows(cq, ct, A, [len(p) + T for p in prompts], "multi")
    release(cq), release(ct)


def test_fp8_kv_cache_together_with_w8a16_runs():
    mq, cq, mt, ct = pair("llama", kv="fp8")
    vocab = mq.args.vocab_size
    prompts = prompts_of(vocab)
    lq, lt = mq.prefill(prompts, A), mt.prefill(prompts, A)
    print(f"W8A16MODEL fp8-kv prefill logits vs the bf16 twin: {assert_close(lq, lt, LOGITS_BAR, what='fp8 prefill'):.3e}")
    for step in range(2):
        tok = torch.full((3,), 7 + step, dtype=torch.int64, device="cuda")
        eager = decode_step(mq, cq, A, tok, False)
        assert bool(torch.isfinite(eager).all()) and tuple(eager.shape) == (3, vocab)
    tok = torch.full((3,), 9, dtype=torch.int64, device="cuda")
    assert bool(torch.isfinite(decode_step(mq, cq, A, tok, True)).all())
    assert cq.paged_k_cache.element_size() == 1 and mq.layers[0].attn.fp8_kv
    release(cq), release(ct)


def test_models_with_formats_of_their_own_refuse_w8a16():
    from chitu_amd.deepseek_v3 import DeepSeekV3Args
    from chitu_amd.mixtral import MixtralArgs
    from chitu_amd.quantize import quantize_w8a16_
    from chitu_amd.qwen3_moe import Qwen3MoeArgs

    for cls in (MixtralArgs, Qwen3MoeArgs, DeepSeekV3Args):
        with pytest.raises(ValueError):
            cls(quant="w8a16")
    with pytest.raises(TypeError):
        quantize_w8a16_(torch.nn.Linear(64, 64))
