"""Times of the chitu_ext8_logprobs launch beside the arg-max and top-k / top-p sampling launches at vocab 129280, one process: each
launch captured 50 times in a hipGraph, the graph replayed 20 times between device events, the variants alternating over 5 rounds
(profiles/logprobs_times.json).  Usage: python tools/logprobs_time.py [out.json]"""
import json, os, socket, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chitu_amd import sampling

V, REP, REPLAYS, ROUNDS = 129280, 50, 20, 5
g = torch.Generator().manual_seed(0)
x16 = (torch.randn(16, V, generator=g) * 3).cuda()
x1 = x16[:1].contiguous()
tok16 = sampling.argmax(x16)
tok1 = tok16[:1].contiguous()
temps, ks, ps = torch.full((16,), 0.8).cuda(), torch.full((16,), 50, dtype=torch.int32).cuda(), torch.full((16,), 0.9).cuda()
u = torch.rand(16, generator=g).cuda()
out_tok = torch.empty(16, dtype=torch.int64, device="cuda")

def lp_fn(x, tok, n):
    outs = sampling.logprobs(x, tok, n)
    return lambda: sampling.logprobs(x, tok, n, out=outs)

variants = {
    "logprobs rows=1 N=0": lp_fn(x1, tok1, 0), "logprobs rows=1 N=20": lp_fn(x1, tok1, 20),
    "logprobs rows=16 N=0": lp_fn(x16, tok16, 0), "logprobs rows=16 N=20": lp_fn(x16, tok16, 20),
    "argmax rows=16": lambda: sampling.argmax(x16, out=out_tok),
    "sample top-k/top-p rows=16": lambda: sampling.top_k_top_p_sampling_from_logits(x16, temps, ks, ps, uniforms=u, out=out_tok),
}
graphs = {}
for name, fn in variants.items():
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(REP):
            fn()
    gr.replay(); torch.cuda.synchronize()
    graphs[name] = gr
times = {n: [] for n in variants}
for _ in range(ROUNDS):
    for name, gr in graphs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gr.replay(); a.record()
        for _ in range(REPLAYS):
            gr.replay()
        b.record(); torch.cuda.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / (REP * REPLAYS))
res = {"device": torch.cuda.get_device_name(0), "host": socket.gethostname(), "torch": torch.__version__, "hip": torch.version.hip,
       "us_per_launch": {n: {"median": round(statistics.median(t), 2), "all": [round(v, 2) for v in t]} for n, t in times.items()}}
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
