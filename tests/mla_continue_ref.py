"""Builders and restatements of the continued MLA prefill tests (tests/test_mla_continue_host.py on the CPU,
tests/test_gpu_mla_continue.py on the GPU): the position map of mla_prefill_flash_pipe_kernel<kCont = true> in Python, the fp64
attention with separate query and key extents, the exact constructions of tests/attn_exact.py with a prefix in front of the
queries, and thin ctypes callers of the two chitu_ext2_ entries.  Expected values come from closed forms and from fp64, never from
a kernel."""
import ctypes

import torch

from tests import attn_exact as ax

KEY_BLOCK = 32  # pfp::kKeys: the causal mask is applied in a workgroup's last 32-key block only
WAVES, ROWS_PER_WAVE = 4, 2  # a workgroup's 8 query tokens: wave w owns tokens 2 w and 2 w + 1


def kbq():
    return int(ax.source_constant("mla_prefill_flash.hip", "kBQ"))


def grid_x(max_seqlen_q, bq):
    """the host's grid: one workgroup column more than ceil(max_seqlen_q / kBQ)"""
    return -(-max_seqlen_q // bq) + 1


def position_map(cu_q0, n, L, grid, bq, aligned=True):
    """The kernel's index arithmetic for one sequence with query rows cu_q0 .. cu_q0 + n - 1 and L keys.  Returns a list with one
    entry per workgroup that does not exit: dict(p0, nq, nb, t_lo, q_rows = the Q row every (wave, r) LOADS (8 entries, the clamp
    included), stores = [(wave, t, position, out row)]).  aligned = False: the REJECTED layout (blocks start at the first new
    token), for the test that shows what the alignment is for."""
    if n <= 0:
        return []
    P = max(L - n, 0)
    q_off = cu_q0 - (L - n)
    out = []
    for x in range(grid):
        p0 = (bq * (P // bq) if aligned else P) + bq * (grid - 1 - x)
        if p0 >= L:
            continue
        nq = min(bq, L - p0)
        t_lo = max(P - p0, 0)
        nb = -(-(p0 + nq) // KEY_BLOCK)
        q_rows, stores = [], []
        for w in range(WAVES):
            for r in range(ROWS_PER_WAVE):
                t = ROWS_PER_WAVE * w + r
                q_rows.append(q_off + p0 + max(min(t, nq - 1), t_lo))
                if t_lo <= t < nq:
                    stores.append((w, t, p0 + t, q_off + p0 + t))
        out.append(dict(x=x, p0=p0, nq=nq, nb=nb, t_lo=t_lo, q_rows=q_rows, stores=stores))
    return out


def prefill64_offset(q, kv, cu_q, cu_k, scale):
    """q [Tq, H, 576], kv [Tk, 576]; query i of sequence s sits at position L_s - n_s + i and sees keys 0 .. that position
    (bottom-right aligned causal mask) -> [Tq, H, 512] fp64.  L_s < n_s: the first n_s - L_s rows are left zero."""
    out = torch.zeros(q.shape[0], q.shape[1], 512, dtype=torch.float64)
    for s in range(len(cu_q) - 1):
        q0, n = cu_q[s], cu_q[s + 1] - cu_q[s]
        k0, L = cu_k[s], cu_k[s + 1] - cu_k[s]
        if n == 0 or L == 0:
            continue
        k = kv[k0:k0 + L].double()
        sc = torch.einsum("thd,sd->hts", q[q0:q0 + n].double() * scale, k)
        pos = torch.arange(n).view(n, 1) + (L - n)
        sc.masked_fill_(torch.arange(L).view(1, L) > pos, float("-inf"))
        p = torch.nan_to_num(torch.softmax(sc, dim=-1), nan=0.0)
        out[q0:q0 + n] = torch.einsum("hts,sc->thc", p, k[:, :512])
    return out


def tails(q, cu, ns):
    """the last ns[s] query rows of every sequence of a whole-sequence batch -> (q rows, cu_q, index of those rows in the batch)"""
    idx = torch.cat([torch.arange(cu[s + 1] - n, cu[s + 1]) for s, n in enumerate(ns)])
    return q[idx].contiguous(), ax.cu_of(ns), idx


# ---------------------------------------------------------------- exact constructions with a prefix
def count_case(pairs, H, seed=0):
    """pairs [(P, n)]: sequence s has P + n latent rows, the last n are queries; q = 0, so query i must return the mean of exactly
    the first P + i + 1 latent rows (attn_exact.prefill_count_case's rows, one whole sequence each)."""
    whole = ax.prefill_count_case([P + n for P, n in pairs], H, 1, 512, ax.P_MLA, seed=seed)
    ns = [n for _, n in pairs]
    _, cu_q, idx = tails(whole["q"], whole["cu"], ns)
    return dict(q=torch.zeros(len(idx), H, 576), kv=whole["k"][:, 0], cu_q=cu_q, cu_k=whole["cu"], want=whole["want"][idx], max_q=max(ns))


def probe_keys(P, i):
    """keys a query at position P + i is probed with: 0, P - 1, P, P + i, both sides of every 32-key block edge up to it"""
    a = P + i
    toks = {0, P - 1, P, a}
    for e in range(KEY_BLOCK, a + 1, KEY_BLOCK):
        toks |= {e - 1, e}
    return sorted(t for t in toks if 0 <= t <= a)


def dominant_case(P, n, H, beyond=False):
    """One sequence per (query i, probed key): every head of query i steers to rope channel 0, and only the probed key has K_AMP
    there, so the output is that key's latent row (identity rows).  beyond: the key one PAST the causal edge (P + i + 1, present in
    the key rows when i < n - 1) carries the amplitude instead: it must not appear -- the permitted keys all score 0 and tie, so
    the output is the mean of rows 0 .. P + i, far from row P + i + 1.  Each sequence holds all n queries (the others are 0: they return
    their own means).  probed: the batch rows that carry a steering query."""
    L = P + n
    latent = ax.identity_rows(L, 1, 512)[:, 0]
    qs, kvs, want, cu_q, cu_k, probed = [], [], [], [0], [0], []
    for i in range(n):
        probes = [P + i + 1] if beyond else probe_keys(P, i)
        for t in probes:
            if t >= L:
                continue
            rope = torch.zeros(L, 64)
            rope[t, 0] = ax.K_AMP
            q = torch.zeros(n, H, 576)
            q[i, :, 512] = ax.Q_AMP
            qs.append(q)
            kvs.append(ax.mla_rows(latent, rope))
            w = ax.count_expected(latent.view(L, 1, 512))[P + 1:P + n + 1].expand(n, H, 512).clone()  # q = 0 rows: the mean
            if not beyond:
                w[i] = latent[t].double()
            want.append(w)
            probed.append(cu_q[-1] + i)
            cu_q.append(cu_q[-1] + n)
            cu_k.append(cu_k[-1] + L)
    return dict(q=torch.cat(qs), kv=torch.cat(kvs), cu_q=cu_q, cu_k=cu_k, want=torch.cat(want), max_q=n,
                probed=torch.tensor(probed))


# ---------------------------------------------------------------- callers
def _i32(v):
    return ctypes.c_int32(int(v))


def _i64(v):
    return ctypes.c_int64(int(v))


def flash_continue(q, kv, cu_q, cu_k, max_q, scale, out=None, kv_stride=None):
    """chitu_ext2_mla_prefill_flash_continue on device tensors; returns out [Tq, H, 512] bf16 (device)"""
    from chitu_amd import _lib

    q = q.to(torch.bfloat16).cuda().contiguous()
    kv = kv.to(torch.bfloat16).cuda().contiguous()
    cq = torch.tensor(cu_q, dtype=torch.int32, device="cuda")
    ck = torch.tensor(cu_k, dtype=torch.int32, device="cuda")
    if out is None:
        out = torch.empty(q.shape[0], q.shape[1], 512, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().chitu_ext2_mla_prefill_flash_continue(
        _lib.ptr(q), _i64(q.stride(0)), _i64(q.stride(1)), _lib.ptr(kv), _i64(kv_stride or kv.stride(0)), _lib.ptr(cq), _lib.ptr(ck),
        _i32(len(cu_q) - 1), _i32(max_q), _lib.f32(scale), _lib.ptr(out), _i32(q.shape[1]), _i32(512), _i32(64), _lib.stream_ptr()),
        "mla_prefill_flash_continue")
    return out


def flash_whole(q, kv, cu, scale):
    """chitu_hip_mla_prefill_flash: the whole-sequence call the continued form is compared with"""
    from chitu_amd import _lib

    q = q.to(torch.bfloat16).cuda().contiguous()
    kv = kv.to(torch.bfloat16).cuda().contiguous()
    c = torch.tensor(cu, dtype=torch.int32, device="cuda")
    out = torch.empty(q.shape[0], q.shape[1], 512, dtype=torch.bfloat16, device="cuda")
    seqs = [b - a for a, b in zip(cu[:-1], cu[1:])]
    _lib.check(_lib.lib().chitu_hip_mla_prefill_flash(
        _lib.ptr(q), _i64(q.stride(0)), _i64(q.stride(1)), _lib.ptr(kv), _i64(kv.stride(0)), _lib.ptr(c), _i32(len(cu) - 1),
        _i32(max(seqs)), _lib.f32(scale), _lib.ptr(out), _i32(q.shape[1]), _i32(512), _i32(64), _lib.stream_ptr()), "mla_prefill_flash")
    return out
