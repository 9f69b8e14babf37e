"""Multi-process (gloo, world_size 2 and 4, CPU) tests of the tensor-parallel path.

1. chitu_amd.tensor_parallel layers vs an unsharded reference (same checks the reference would need
   for chitu/tensor_parallel.py:42-208).
2. The DeepSeek-V3 decode step wiring under TP=2: shard a tiny model with the reference's rules
   (chitu/models/model.py:332-370 + model_deepseek_v3.py:1167-1288: heads / FFN width split, wqkv_a,
   gate and KV cache replicated, gate|up halves chunked separately), run chitu_amd.deepseek_v3 on
   each rank with the HIP ops swapped for the oracle (tests/cpu_ops_shim.py), and compare the
   all-reduced result with the single-rank run.
"""

import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(fn, world, *args):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_entry, args=(fn, r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for r in results:
        assert r[1] == "ok", r
    return results


def _entry(fn, rank, world, port, q, *args):
    try:
        # CPU ranks on any host: the device stays hidden from them (before HIP initialises), so a host with a GPU runs what a
        # host without one does -- including the no-device verdict of the transport decision in _tp_layers
        os.environ["HIP_VISIBLE_DEVICES"] = "-1"
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from chitu_amd import tensor_parallel as tp

        tp.init_tp(world, 1)
        fn(rank, world, *args)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, "fail: " + repr(e) + traceback.format_exc()))


def _tp_layers(rank, world):
    from chitu_amd import tensor_parallel as tp

    assert tp.get_tp_size() == world and tp.get_tp_rank() == rank
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 64, generator=g)
    w_col = torch.randn(48, 64, generator=g)
    b_col = torch.randn(48, generator=g)
    w_row = torch.randn(32, 64, generator=g)
    b_row = torch.randn(32, generator=g)
    emb = torch.randn(40, 16, generator=g)

    col = tp.ColumnParallelLinear(64, 48, has_bias=True, gather_output=True, dtype=torch.float32)
    n = 48 // world
    col.weight.data.copy_(w_col[rank * n : (rank + 1) * n])
    col.bias.data.copy_(b_col[rank * n : (rank + 1) * n])
    assert torch.allclose(col(x), torch.nn.functional.linear(x, w_col, b_col), atol=1e-5)

    row = tp.RowParallelLinear(64, 32, has_bias=True, input_is_parallel=False, dtype=torch.float32)
    k = 64 // world
    row.weight.data.copy_(w_row[:, rank * k : (rank + 1) * k])
    row.bias.data.copy_(b_row)
    assert torch.allclose(row(x), torch.nn.functional.linear(x, w_row, b_row), atol=1e-4)

    e = tp.VocabParallelEmbedding(40, 16, dtype=torch.float32)
    v = 40 // world
    e.weight.data.copy_(emb[rank * v : (rank + 1) * v])
    ids = torch.tensor([[0, 39, 20], [19, 21, 5]])
    ids_copy = ids.clone()
    assert torch.allclose(e(ids), torch.nn.functional.embedding(ids, emb))
    assert torch.equal(ids, ids_copy)  # caller's ids untouched (the reference mutates them in place)

    y = torch.arange(6.0).view(2, 3) + 100 * rank
    gth = tp.all_gather_last_dim(y)
    assert gth.shape == (2, 3 * world) and torch.equal(gth[:, 3 * rank : 3 * rank + 3], y)
    # with the logits' cast the result is DENSE (the sampler reads rows with a unit stride; bench.py --gpus N on the
    # library path failed on the permuted view a plain .to() keeps)
    g64 = tp.all_gather_last_dim(y, out_dtype=torch.float64)
    assert g64.dtype == torch.float64 and g64.is_contiguous() and torch.equal(g64, gth.double())
    # the transport decision is an object a bench line can carry: on a host without a GPU the in-graph collectives are not
    # enabled, every rank says so with the stage and the reason, and the library path stays in place
    assert tp.xgmi_report["enabled"] is False
    assert tp.enable_xgmi() is False and tp.xgmi_comm() is None
    assert tp.xgmi_report["enabled"] is False and tp.xgmi_report["stage"] == "none" and tp.xgmi_report["reason"]


def test_tp_layers_world2():
    _run(_tp_layers, 2)


def _tiny_args(wide=False):
    """wide: FFN widths that still leave whole 128-blocks per rank at 4 ranks."""
    from chitu_amd.deepseek_v3 import DeepSeekV3Args

    return DeepSeekV3Args(vocab_size=256, dim=256, inter_dim=1024 if wide else 512, moe_inter_dim=512 if wide else 256, n_layers=2,
                          n_dense_layers=1, n_heads=16, n_routed_experts=8, n_shared_experts=1, n_activated_experts=2,
                          n_expert_groups=2, n_limited_groups=1, q_lora_rank=128, gate_bias=True)


def _build_cpu_model(args, seed=0):
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.deepseek_v3 import DeepSeekV3Decoder
    from tests import cpu_ops_shim

    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=2, block_size=64, max_seq_len=128, device="cpu",
                                kv_shape_per_sample=(576,), dtype=torch.bfloat16)
    model = DeepSeekV3Decoder(args, cache, cpu_ops_shim.CpuAttnBackend(args.n_heads), max_position_embeddings=256,
                              device="cpu")
    return model, cache


def _full_state(args):
    """Deterministic TP=1 parameters (fp8 weights via bf16 randn, scales U(0.01,0.03))."""
    import copy

    a1 = copy.copy(args)
    a1.shard_degree = 1
    model, _ = _build_cpu_model(a1)
    g = torch.Generator().manual_seed(123)
    sd = {}
    for k, p in model.named_parameters():
        if p.dtype == torch.float8_e4m3fn:
            sd[k] = (torch.randn(p.shape, generator=g) * 0.5).to(torch.float8_e4m3fn)
        elif p.dtype == torch.float32:
            sd[k] = torch.rand(p.shape, generator=g) * 0.02 + 0.01
        elif k.endswith("norm.weight"):
            sd[k] = torch.ones(p.shape, dtype=p.dtype)
        else:
            sd[k] = (torch.randn(p.shape, generator=g) * 0.05).to(p.dtype)
    return sd


def _shard(sd, args, rank, world):
    """Megatron-style chunking as in chitu/models/model.py:332-370."""
    H = args.n_heads
    out = {}
    for k, v in sd.items():
        def rows(t, n_units):  # split dim -2 (or 0) into `world` contiguous chunks
            c = t.shape[-2] // world
            return t[..., rank * c : (rank + 1) * c, :].contiguous()

        def cols(t):
            c = t.shape[-1] // world
            return t[..., rank * c : (rank + 1) * c].contiguous()

        def halves_rows(t):  # [.., 2I, K] = [gate | up]: chunk each half separately
            i = t.shape[-2] // 2
            return torch.cat([rows(t[..., :i, :], 0), rows(t[..., i:, :], 0)], dim=-2).contiguous()

        if any(s in k for s in ("wq_b.", "wkv_b.")):
            out[k] = rows(v, H)
        elif "wo." in k or ".w2.weight" in k or ".w2.scale" in k or "w2_weight" in k or "w2_scale" in k:
            out[k] = cols(v)
        elif "w1w3" in k:
            out[k] = halves_rows(v)
        elif k in ("embed_weight", "head_weight"):
            c = v.shape[0] // world
            out[k] = v[rank * c : (rank + 1) * c].contiguous()
        else:
            out[k] = v.clone()
    return out


def _shard_ep(sd, args, rank, world):
    """Expert-parallel layout of the MoE layers (chitu_amd.deepseek_v3.MoEDeepSeekV3, moe_world_size = world):
    routed experts [rank*E/ep, (rank+1)*E/ep) whole, the shared experts as ONE MLP of width n_shared*I chunked
    like a column/row-parallel MLP; everything else as _shard."""
    nr, ns = args.n_routed_experts, args.n_shared_experts
    n_local = nr // world
    lo, hi = rank * n_local, (rank + 1) * n_local
    out = {k: v for k, v in _shard(sd, args, rank, world).items() if ".ffn.w1w3_" not in k and ".ffn.w2_" not in k}

    def chunk(t, dim):
        c = t.shape[dim] // world
        return t.narrow(dim, rank * c, c)

    for k, v in sd.items():
        pre = k[: k.rfind(".") + 1]
        if k.endswith(".ffn.w1w3_weight") or k.endswith(".ffn.w1w3_scale"):
            out[k] = v[lo:hi].contiguous()
            name = "shared.w1w3.weight" if k.endswith("weight") else "shared.w1w3.scale"
            sh = v[nr:]  # [ns, 2I(/128), K(/128)] = per expert [gate | up]
            i = sh.shape[1] // 2
            gate = sh[:, :i].reshape(ns * i, -1)
            up = sh[:, i:].reshape(ns * i, -1)
            out[pre + name] = torch.cat([chunk(gate, 0), chunk(up, 0)], 0).contiguous()
        elif k.endswith(".ffn.w2_weight") or k.endswith(".ffn.w2_scale"):
            out[k] = v[lo:hi].contiguous()
            name = "shared.w2.weight" if k.endswith("weight") else "shared.w2.scale"
            sh = torch.cat(list(v[nr:]), dim=-1)  # [K(/128), ns*I(/128)]
            out[pre + name] = chunk(sh, 1).contiguous()
    return out


def _decode_tp(rank, world, expert_parallel=False, wide=False):
    import copy

    from tests import cpu_ops_shim

    cpu_ops_shim.install(setattr)
    args = _tiny_args(wide)
    full = _full_state(args)
    a = copy.copy(args)
    a.shard_degree = None  # live TP group size
    if expert_parallel:
        a.moe_world_size = world
    model, cache = _build_cpu_model(a)
    sharded = (_shard_ep if expert_parallel else _shard)(full, args, rank, world)
    assert set(sharded) == {k for k, _ in model.named_parameters()}
    for k, p in model.named_parameters():
        assert p.shape == sharded[k].shape, (k, p.shape, sharded[k].shape)
        p.data.copy_(sharded[k])
    reqs = ["a", "b"]
    g = torch.Generator().manual_seed(9)
    for r, n in zip(reqs, (5, 64)):
        cache.register_sequence(r, n)
        for blk in cache.block_table[r]:
            cache.paged_kv_cache[:, blk] = (torch.randn(args.n_layers, 64, 576, generator=g) * 0.5).to(torch.bfloat16)
    tokens = torch.tensor([3, 200])
    outs = []
    for _ in range(2):
        cache.prepare_cache_decode(reqs)
        cache.prepare_block_table_for_decode(reqs)
        with torch.inference_mode():
            logits = model.decode(tokens, use_graph=False)
        assert logits.shape == (2, args.vocab_size) and logits.dtype == torch.float32
        outs.append(logits.clone())
        tokens = logits.argmax(-1)
        cache.finalize_cache_single_decode(reqs)
    # every rank must hold identical logits (all-gathered) and an identical replicated KV cache
    for t in outs + [cache.paged_kv_cache.float()]:
        ref = t.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(ref, t)
    if rank == 0:
        torch.save({"logits": outs}, os.environ["TP_OUT"] + (f".ep{world}" if expert_parallel else f".w{world}"))


def test_decode_step_tp4_and_ep4_match_tp1(tmp_path):
    """Four ranks: 4 of 16 heads, a quarter of every FFN width and of the vocabulary per rank (TP); 2 of 8 routed experts
    at full width + a quarter of the shared expert per rank (EP).  Both against the same single-rank step."""
    base = str(tmp_path / "tp")
    os.environ["TP_OUT"] = base
    _run(_decode_tp, 1, False, True)
    _run(_decode_tp, 4, False, True)
    _run(_decode_tp, 4, True, True)
    l1 = torch.load(base + ".w1")["logits"]
    for other in (".w4", ".ep4"):
        for a, b in zip(l1, torch.load(base + other)["logits"]):
            err = ((a - b).abs().max() / a.abs().max()).item()
            assert err < 5e-2, (other, err)


def test_decode_step_tp2_matches_tp1(tmp_path):
    base = str(tmp_path / "tp")
    os.environ["TP_OUT"] = base
    _run(_decode_tp, 1)
    _run(_decode_tp, 2)
    l1 = torch.load(base + ".w1")["logits"]
    l2 = torch.load(base + ".w2")["logits"]
    for a, b in zip(l1, l2):
        err = ((a - b).abs().max() / a.abs().max()).item()
        assert err < 5e-2, err  # bf16 partial sums are rounded per rank before the all-reduce


def test_decode_step_ep2_matches_tp1(tmp_path):
    """Expert parallelism: 2 ranks, each holding half of the routed experts at full width and
    half of the shared expert's width; attention stays tensor parallel; the layer's all-reduce is the combine."""
    base = str(tmp_path / "ep")
    os.environ["TP_OUT"] = base
    _run(_decode_tp, 1)
    _run(_decode_tp, 2, True)
    l1 = torch.load(base + ".w1")["logits"]
    l2 = torch.load(base + ".ep2")["logits"]
    for a, b in zip(l1, l2):
        err = ((a - b).abs().max() / a.abs().max()).item()
        assert err < 5e-2, err


def _graph_break_protocol(rank, world):
    """tensor_parallel's cut points (chitu_amd/graphs.py): while a piecewise capture is active every collective
    hands its launch to the capture instead of running it; issued later, in order, the closures do the step's
    communication.  (The hipGraph side of the protocol is tested on the GPU.)"""
    from chitu_amd import tensor_parallel as tp

    deferred = []
    tp._graph_break = deferred.append
    try:
        a = torch.full((4,), float(rank + 1))
        out = tp.all_reduce(a)
        assert out is a and torch.equal(a, torch.full((4,), float(rank + 1)))  # nothing has run yet
        y = torch.arange(6, dtype=torch.float32).view(2, 3) + 10 * rank
        g = tp.all_gather_last_dim(y)
    finally:
        tp._graph_break = None
    assert len(deferred) == 2 and all(callable(r) for r in deferred)
    for run in deferred:
        run()
    assert torch.equal(a, torch.full((4,), float(sum(range(1, world + 1)))))
    want = torch.cat([torch.arange(6, dtype=torch.float32).view(2, 3) + 10 * r for r in range(world)], dim=-1)
    assert torch.equal(g, want)
    # outside a capture the collectives run immediately
    b = torch.ones(2)
    tp.all_reduce(b)
    assert torch.equal(b, torch.full((2,), float(world)))


def test_graph_break_protocol_world2():
    _run(_graph_break_protocol, 2)


def _llama_tp(rank, world):
    """chitu_amd/llama.py's wiring under tensor parallelism (heads, SwiGLU width and vocabulary split, two
    all-reduces per layer, logits all-gather) on the REFERENCE'S Llama CPU run (BASELINE config 1,
    tests/golden/ref_llama.npz): prefill of the prompt + 64 decode steps fed the reference's greedy tokens."""
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.llama import LlamaArgs, LlamaDecoder
    from tests import cpu_ops_shim
    from tests.util import ref_llama_fixture

    cpu_ops_shim.install_llama(setattr)
    g, cfg, full = ref_llama_fixture()
    hq, hkv, hd = cfg["n_heads"], cfg["n_kv_heads"], cfg["dim"] // cfg["n_heads"]
    ffn = full["layers.0.ffn.w2"].shape[1]
    args = LlamaArgs(dim=cfg["dim"], n_layers=cfg["n_layers"], n_heads=hq, n_kv_heads=hkv, vocab_size=cfg["vocab_size"],
                     ffn_dim=ffn, norm_eps=cfg["norm_eps"], rope_theta=cfg["rope_theta"])
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=1, block_size=64, max_seq_len=128, device="cpu",
                                n_local_kv_heads=hkv // world, head_dim=hd, dtype=torch.bfloat16)
    model = LlamaDecoder(args, cache, cpu_ops_shim.CpuGqaBackend(), max_position_embeddings=128, device="cpu")

    def chunk(t, dim):
        c = t.shape[dim] // world
        return t.narrow(dim, rank * c, c)

    for k, p in model.named_parameters():
        t = full[k]
        if k.endswith("attn.wqkv"):  # [wq | wk | wv] rows: every part is split by heads (models/model.py:332-370)
            q, kk, v = t[: hq * hd], t[hq * hd : (hq + hkv) * hd], t[(hq + hkv) * hd :]
            t = torch.cat([chunk(q, 0), chunk(kk, 0), chunk(v, 0)], 0)
        elif k.endswith("ffn.w13"):
            i = t.shape[0] // 2
            t = torch.cat([chunk(t[:i], 0), chunk(t[i:], 0)], 0)
        elif k.endswith("attn.wo") or k.endswith("ffn.w2"):
            t = chunk(t, 1)
        elif k in ("embed_weight", "head_weight"):
            t = chunk(t, 0)
        assert p.shape == t.shape, (k, p.shape, t.shape)
        p.data.copy_(t)
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    rows = [model.prefill([prompt], ["r"]).float()]
    for step in range(64):
        cache.prepare_cache_decode(["r"])
        cache.prepare_block_table_for_decode(["r"])
        rows.append(model.decode(torch.tensor([toks[step]]), use_graph=False).float())
        cache.finalize_cache_single_decode(["r"])
    logits = torch.cat(rows)
    ref = torch.from_numpy(g["logits"])
    assert logits.shape == ref.shape
    err = ((logits - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()
    assert err < 3e-2, err  # bf16 partial sums are rounded per rank before each all-reduce
    top2 = ref.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.08 * ref.abs().amax(-1)
    assert clear.sum() >= 20 and bool((logits.argmax(-1) == torch.from_numpy(g["tokens"]))[clear].all())
    same = logits.clone()
    dist.broadcast(same, 0)
    assert torch.equal(same, logits)  # every rank holds the gathered logits


@pytest.mark.parametrize("world", [1, 2])
def test_llama_wiring_reproduces_the_reference_cpu_run(world):
    _run(_llama_tp, world)


def _mixtral_tp(rank, world, heads=4, kv_heads=2, ffn_dim=256, tag="mx"):
    """BASELINE config 4's parallelism at test size: chitu_amd/mixtral.py under tensor parallelism -- attention heads
    and every expert's width split over the ranks (w13 rows per gate / up half, w2 columns; per-channel scales follow
    their channels, w2's stay whole), router replicated, two all-reduces per layer -- two decode steps."""
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.mixtral import MixtralArgs, MixtralDecoder
    from oracle import w8a8 as ow
    from tests import cpu_ops_shim

    cpu_ops_shim.install_llama(setattr)
    args = MixtralArgs(dim=128 * heads, n_layers=2, n_heads=heads, n_kv_heads=kv_heads, vocab_size=512, ffn_dim=ffn_dim,
                       num_local_experts=4, num_experts_per_tok=2)
    hq, hkv, hd = args.n_heads, args.n_kv_heads, args.head_dim
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=2, block_size=64, max_seq_len=128, device="cpu",
                                n_local_kv_heads=hkv // world, head_dim=hd, dtype=torch.bfloat16)
    model = MixtralDecoder(args, cache, cpu_ops_shim.CpuGqaBackend(), max_position_embeddings=128, device="cpu")
    g = torch.Generator().manual_seed(21)
    full = {}
    D = args.dim
    shapes = {"embed_weight": (512, D), "head_weight": (512, D), "norm": (D,)}
    for i in range(args.n_layers):
        pre = f"layers.{i}."
        shapes.update({pre + "attn.wqkv": ((hq + 2 * hkv) * hd, D), pre + "attn.wo": (D, hq * hd), pre + "attn_norm": (D,),
                       pre + "ffn_norm": (D,), pre + "ffn.gate": (4, D)})
    for k, shp in shapes.items():
        full[k] = torch.ones(shp, dtype=torch.bfloat16) if k.endswith("norm") else \
            (torch.randn(shp, generator=g) * (1.0 if k == "embed_weight" else shp[-1] ** -0.5)).to(torch.bfloat16)
    for i in range(args.n_layers):
        pre = f"layers.{i}.ffn."
        q13, s13, q2, s2 = [], [], [], []
        for e in range(4):
            a, b = ow.quant_weight(torch.randn(2 * args.ffn_dim, D, generator=g) * D ** -0.5)
            c, d = ow.quant_weight(torch.randn(D, args.ffn_dim, generator=g) * args.ffn_dim ** -0.5)
            q13.append(a), s13.append(b.view(-1)), q2.append(c), s2.append(d.view(-1))
        full[pre + "w13"], full[pre + "w13_scale"] = torch.stack(q13), torch.stack(s13)
        full[pre + "w2"], full[pre + "w2_scale"] = torch.stack(q2), torch.stack(s2)

    def chunk(t, dim):
        c = t.shape[dim] // world
        return t.narrow(dim, rank * c, c)

    for k, p in model.named_parameters():
        t = full[k]
        if k.endswith("attn.wqkv"):
            q, kk, v = t[: hq * hd], t[hq * hd : (hq + hkv) * hd], t[(hq + hkv) * hd :]
            t = torch.cat([chunk(q, 0), chunk(kk, 0), chunk(v, 0)], 0)
        elif k.endswith("ffn.w13") or k.endswith("ffn.w13_scale"):
            i = t.shape[1] // 2
            t = torch.cat([chunk(t[:, :i], 1), chunk(t[:, i:], 1)], 1)
        elif k.endswith("ffn.w2"):
            t = chunk(t, 2)
        elif k.endswith("attn.wo"):
            t = chunk(t, 1)
        elif k in ("embed_weight", "head_weight"):
            t = chunk(t, 0)
        assert p.shape == t.shape, (k, p.shape, t.shape)
        p.data.copy_(t)
    reqs = ["a", "b"]
    for r, n in zip(reqs, (5, 64)):
        cache.register_sequence(r, n)
        for blk in cache.block_table[r]:
            kv = (torch.randn(2, args.n_layers, 64, hkv, hd, generator=g) * 0.5).to(torch.bfloat16)
            cache.paged_k_cache[:, blk] = chunk(kv[0], 2)
            cache.paged_v_cache[:, blk] = chunk(kv[1], 2)
    tokens, outs = torch.tensor([3, 200]), []
    for _ in range(2):
        cache.prepare_cache_decode(reqs)
        cache.prepare_block_table_for_decode(reqs)
        with torch.inference_mode():
            logits = model.decode(tokens, use_graph=False)
        assert logits.shape == (2, args.vocab_size)
        outs.append(logits.float().clone())
        tokens = logits.argmax(-1)
        cache.finalize_cache_single_decode(reqs)
    for t in outs:
        ref = t.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(ref, t)
    if rank == 0:
        torch.save({"logits": outs}, os.environ["TP_OUT"] + f".{tag}{world}")


def test_mixtral_int8_decode_step_tp4_matches_tp1(tmp_path):
    """BASELINE config 4 at its stated degree: "Mixtral-8x7B W8A8 ... TP=4".  World-size-4 gloo run of the Mixtral INT8
    step (8 query / 4 kv heads, expert width 512: every rank keeps whole 128-column int8 blocks) against TP = 1."""
    base = str(tmp_path / "mx4")
    os.environ["TP_OUT"] = base
    _run(_mixtral_tp, 1, 8, 4, 512, "q")
    _run(_mixtral_tp, 4, 8, 4, 512, "q")
    l1, l4 = torch.load(base + ".q1")["logits"], torch.load(base + ".q4")["logits"]
    err = ((l1[0] - l4[0]).abs().max() / l1[0].abs().max()).item()
    assert err < 5e-2, err  # per-rank int8 quantisation of the experts' hidden activations (see the TP = 2 test)


def test_mixtral_int8_decode_step_tp2_matches_tp1(tmp_path):
    base = str(tmp_path / "mx")
    os.environ["TP_OUT"] = base
    _run(_mixtral_tp, 1)
    _run(_mixtral_tp, 2)
    l1, l2 = torch.load(base + ".mx1")["logits"], torch.load(base + ".mx2")["logits"]
    # first step: same tokens on both sides; a rank quantises ITS slice of the experts' hidden activations per token
    # (W8A8Linear under row parallelism), so TP = 2 differs from TP = 1 by int8 rounding, not bit for bit
    err = ((l1[0] - l2[0]).abs().max() / l1[0].abs().max()).item()
    assert err < 5e-2, err


def _decode_bs1_fused_vs_unfused(rank, world):
    """Host wiring of the batch-1 norm-prologue launch (deepseek_v3._fuses_attn_norm_into_first_projection ->
    ops.fp8_linear_add_norm -> decode_forward_paged(first=...)) on the CPU shim, where the fused op IS the composition it
    replaces: the step with the fusion must equal the step without it, behind a dense FFN and behind a MoE layer, and the KV
    rows it appends must be the same.  (The un-summed top-k form of the pending tensor is a device-side optimisation the shim
    does not model; tests/test_gpu_deepseek.py covers it.)"""
    from chitu_amd import deepseek_v3 as ds
    from chitu_amd import ops
    from tests import cpu_ops_shim

    cpu_ops_shim.install(setattr)
    args = _tiny_args()
    args.n_layers = 3  # dense, MoE, MoE: a plain pending and a 3-D (terms) pending both reach an attn_norm
    args.dim = 1024    # (the fused launch needs >= 4 waves of K split: 8 K blocks of 128)
    full = _full_state(args)
    taken = []
    real = ops.fp8_linear_add_norm
    ops.fp8_linear_add_norm = lambda x, add, *a, **k: (taken.append(add.dim()), real(x, add, *a, **k))[1]
    res = {}
    for limit in (0, 1):
        ds.FUSE_ATTN_NORM_MAX_BS = limit
        model, cache = _build_cpu_model(args)
        for k, p in model.named_parameters():
            p.data.copy_(full[k])
        cache.register_sequence("a", 70)
        g = torch.Generator().manual_seed(3)
        for blk in cache.block_table["a"]:
            cache.paged_kv_cache[:, blk] = (torch.randn(args.n_layers, 64, 576, generator=g) * 0.5).to(torch.bfloat16)
        tokens, outs = torch.tensor([7]), []
        for _ in range(2):
            cache.prepare_cache_decode(["a"])
            cache.prepare_block_table_for_decode(["a"])
            with torch.inference_mode():
                logits = model.decode(tokens, use_graph=False)
            outs.append(logits.clone())
            tokens = logits.argmax(-1)
            cache.finalize_cache_single_decode(["a"])
        res[limit] = (outs, cache.paged_kv_cache.clone())
        if limit == 0:
            assert not taken
    # two steps x layers 1 and 2 (layer 0 has no pending); the shim's fused_experts sums its top-k itself, so both are plain
    assert len(taken) == 2 * 2 and set(taken) <= {2, 3}
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[0][1], res[1][1])


def test_decode_bs1_with_attn_norm_in_the_first_projection_equals_the_step_without():
    _run(_decode_bs1_fused_vs_unfused, 1)
