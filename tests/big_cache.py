"""Paged KV caches beyond 4 GiB: the page layout, the case builders and the CPU oracles shared by tests/test_big_cache_host.py
(CPU) and tests/test_gpu_big_cache.py (GPU), and the three helpers of the two older beyond-4-GiB tests of
tests/test_gpu_attn_exact.py.  No GPU is needed to import this module.

The layout (high_layout).  Every NAMED page lies at a byte offset in (2^32, 2^32 + 2^31) of its allocation, so an offset cut
to 32 bits lands inside the allocation, in a known low ALIAS page: page (offset mod 2^32) // page_bytes, and the page after it
where the cut offset is no multiple of the page size.  The GUARD set is page 0 plus every alias page.  Guard pages hold decoy
rows (K: attn_exact.K_AMP everywhere, V: 1.0 everywhere; the quantised rows of those in the fp8 formats): a reader that
wraps sees a row that no construction of tests/attn_exact.py tolerates, a writer that wraps changes a guard page.  The same
rows are also placed at LOW page ids (past the guard set) of the same allocation: page ids enter addresses only, so the two
calls must agree bit for bit.

What this layout does not catch: an ELEMENT index held in 32 bits.  In a bf16 cache an unsigned 32-bit element index does
not wrap below 8 GiB and passes; a signed one goes negative past 4 GiB and reads before the allocation -- a fault, not a
failed assertion.  Only the uint8 (fp8) caches turn products such as `trow * 576` or `row * hkv * d` held in an `int` into
an alias inside the allocation.  The byte-offset cut is what every cache format here is guarded against.

A reader case is a dict: fam ("gqa" / "mla"), entry, seqs (the logical rows of each sequence, token order), rows (the
sequence of every table row), the query tensors, totals, kind ("count" / "dominant" / "exact") and want.  Expected values are
the closed forms of tests/attn_exact.py and its multi-token, window and paged-prefill analogues, never a kernel's output."""
import random

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_multi_ref as mr
from tests import attn_paged_prefill_ref as pp
from tests import attn_window_ref as wr
from tests import mla_multi_ref as mm
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8

WRAP = 2 ** 32
FILLS_GQA = [ax.K_AMP, 1.0]  # place_and_append's decoys: K, V
FILLS_MLA = [ax.K_AMP]
GQA_HQ, GQA_HKV, GQA_PAGE = 32, 8, 256
ANY_HQ, ANY_HKV = 6, 2  # the non-power-of-two group: the same allocation seen as pages of 2 KV heads
MLA_H, MLA_PAGE = 16, 64
SPLITS = [1, 3]


# ---------------------------------------------------------------- the helpers of the two older tests
def first_page_beyond_4gib(page_bytes):
    return 2 ** 32 // page_bytes + 1


def need_free(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * nbytes:
        pytest.skip(f"{nbytes / 2**30:.1f} GiB cache: needs {3 * nbytes / 2**30:.0f} GiB free, {free / 2**30:.0f} GiB are")


def place_and_append(caches, rows, fills, tables, lens, quant, append):
    """Write every sequence's rows but its last into its pages (the pages' other rows and page 0 hold fills[c] everywhere: what a
    wrongly admitted key would show), append the last row through the project's append op, and assert that exactly the addressed
    rows of the named pages changed, page 0 not at all.  caches / rows / fills: one entry per cache (K and V, or the one MLA
    cache); rows[c][s]: [n_s, ...] bf16 logical rows of sequence s."""
    page = caches[0].shape[1]
    ids = sorted({int(p) for t in tables for p in t})
    want = []
    for cache, seq_rows, fill in zip(caches, rows, fills):
        sentinel = quant(torch.full((page,) + tuple(seq_rows[0].shape[1:]), fill, dtype=torch.bfloat16))
        cache[0] = sentinel.cuda()
        for i in ids:
            cache[i] = sentinel.cuda()
        for r, t, n in zip(seq_rows, tables, lens):
            for p in range((n + page - 1) // page):
                stop = min(n - 1, (p + 1) * page)
                if stop > p * page:
                    cache[int(t[p]), : stop - p * page] = quant(r[p * page : stop]).cuda()
        w = cache[ids].cpu()
        for r, t, n in zip(seq_rows, tables, lens):
            w[ids.index(int(t[(n - 1) // page])), (n - 1) % page] = quant(r[n - 1 : n])[0]
        want.append((w, sentinel))
    width = max(len(t) for t in tables)
    table = torch.tensor([list(t) + [t[-1]] * (width - len(t)) for t in tables], dtype=torch.int32).cuda()
    old = torch.tensor([n - 1 for n in lens], dtype=torch.int32).cuda()
    append(table, [torch.stack([r[n - 1] for r, n in zip(seq_rows, lens)]).cuda() for seq_rows in rows], old)
    for cache, (w, sentinel) in zip(caches, want):
        assert torch.equal(cache[ids].cpu(), w), "the append changed another row of the named pages, or not the addressed one"
        assert torch.equal(cache[0].cpu(), sentinel), "the append wrote into page 0"
    return table


# ---------------------------------------------------------------- the page layout
def alias_pages(page_id, page_bytes):
    """the pages a 32-bit cut of page_id's byte offset touches: (offset mod 2^32) // page_bytes, and the next one where the cut
    offset is not page aligned"""
    off = (page_id * page_bytes) % WRAP
    first = off // page_bytes
    return [first] if off % page_bytes == 0 else [first, first + 1]


def high_layout(page_bytes, n):
    """(named, alias, guard) for n slots: named[k] = the k-th page past 2^32 bytes; alias[k] = (offset of named[k] mod 2^32) //
    page_bytes; guard = page 0 plus every page a cut offset of a named page touches, sorted."""
    first = first_page_beyond_4gib(page_bytes)
    named = [first + k for k in range(n)]
    assert all(WRAP < p * page_bytes and (p + 1) * page_bytes < WRAP + 2 ** 31 for p in named), "a named page outside (2^32, 2^32 + 2^31)"
    alias = [((p * page_bytes) % WRAP) // page_bytes for p in named]
    assert alias == [alias_pages(p, page_bytes)[0] for p in named]
    guard = sorted({0} | {a for p in named for a in alias_pages(p, page_bytes)})
    assert not set(guard) & set(named)
    return named, alias, guard


def low_pages(page_bytes, n):
    """n low page ids past the guard set of high_layout(page_bytes, n): where the same rows are placed for the bit identity"""
    _, _, guard = high_layout(page_bytes, n)
    return [guard[-1] + 2 + k for k in range(n)]


def page_bytes_of(cache):
    return cache[0].numel() * cache.element_size()


def row_offsets(page_ids, page, page_bytes):
    """byte offset of every row of the given pages"""
    return [p * page_bytes + r * (page_bytes // page) for p in page_ids for r in range(page)]


# ---------------------------------------------------------------- row formats
def quant_of(fam, fp8):
    if not fp8:
        return lambda r: r.to(torch.bfloat16)
    q = g8.quant_ref if fam == "gqa" else m8.quant_ref
    return lambda r: q(r.to(torch.bfloat16))


def widen(fam, rows):
    """cache rows of either format -> fp32 logical rows"""
    if rows.dtype == torch.uint8:
        return (g8.dequant_ref if fam == "gqa" else m8.dequant_ref)(rows).float()
    return rows.float()


def sentinel_page(fam, fp8, page, fill, hkv=GQA_HKV):
    shape = (page, hkv, 128) if fam == "gqa" else (page, 576)
    return quant_of(fam, fp8)(torch.full(shape, fill, dtype=torch.bfloat16))


# ---------------------------------------------------------------- reader cases
def assign_slots(cases, page, seed=0):
    """give every sequence of every case its page slots, shuffled ("in no order"): case["slots"][s] = the slots of sequence s"""
    need = [(c, s, max(1, -(-seq[0].shape[0] // page))) for c in cases for s, seq in enumerate(c["seqs"])]
    order = list(range(sum(n for _, _, n in need)))
    random.Random(seed).shuffle(order)
    at = 0
    for c in cases:
        c["slots"] = []
    for c, s, n in need:
        c["slots"].append(order[at : at + n])
        at += n
    return at


def table_of(case, ids):
    """[table rows, width] int32: every table row names its sequence's pages (ids[slot]); unused entries repeat the last one"""
    width = max(len(s) for s in case["slots"])
    rows = [[ids[k] for k in case["slots"][s]] for s in case["rows"]]
    return torch.tensor([r + [r[-1]] * (width - len(r)) for r in rows], dtype=torch.int32)


def gqa_reader_cases(Hq=GQA_HQ, Hkv=GQA_HKV, page=GQA_PAGE, prefill_only=False):
    """17 and 130 keys, and 258 / 260 keys over a page edge.  Multi-token counting (each query counts exactly its own keys) and
    dominant keys at T in {2, 8}; the window forms with the window's first key in the second page and the key before it in
    the first; paged prefill (counting, windowed counting, dominant keys) behind prefixes in those pages."""
    cases = []
    if not prefill_only:
        for n, T in ((17, 2), (130, 8), (258, 2), (258, 8)):
            c = ax.gqa_count_case(n, Hq, Hkv, seed=n + T, lengths=mr.expanded_lengths([n], T), salt=T)
            cases.append(dict(name=f"multi counting n={n} T={T}", fam="gqa", entry="decode", seqs=[(c["K"], c["V"])], rows=[0],
                              q=c["q"].view(1, T, Hq, 128), totals=[n], W=-1, kind="count", want=c["want"]))
        for n, T in ((130, 8), (258, 2)):
            c = mr.multi_dominant_case(n, T, Hq, Hkv, page, SPLITS)
            cases.append(dict(name=f"multi dominant n={n} T={T}", fam="gqa", entry="decode", seqs=[(c["K"], c["V"])], rows=[0] * c["q"].shape[0],
                              q=c["q"], totals=c["lens"].tolist(), W=-1, kind="dominant", want=c["want"]))
        for n, T, W in ((258, 1, 1), (260, 2, 3)):  # the first visible key is key 256 (of the last query: T = 2 starts one earlier)
            c = ax.gqa_count_case(n, Hq, Hkv, seed=n, lengths=mr.expanded_lengths([n], T), salt=3 + T)
            assert wr.first_key(n, W) == page
            cases.append(dict(name=f"window counting n={n} T={T} W={W}", fam="gqa", entry="decode", seqs=[(c["K"], c["V"])], rows=[0],
                              q=c["q"].view(1, T, Hq, 128), totals=[n], W=W, kind="count", want=wr.gqa_count_want(c, Hq, W)))
        c = mr.multi_dominant_case(260, 1, Hq, Hkv, page, SPLITS, 3)  # probes key 256, and key 255 from outside the window
        cases.append(dict(name="window dominant n=260 W=3", fam="gqa", entry="decode", seqs=[(c["K"], c["V"])], rows=[0] * c["q"].shape[0],
                          q=c["q"], totals=c["lens"].tolist(), W=3, kind="dominant", want=c["want"]))
    pairs = [(12, 5), (120, 10), (250, 9)]  # 17, 130 and 259 keys: the last chunk lies across the page edge
    c = pp.count_case(pairs, Hq, Hkv)
    assert pp.max_keys_per_position_channel(c) <= 16
    seqs = list(zip(c["K"], c["V"]))
    base = dict(fam="gqa", entry="prefill", rows=[0, 1, 2], news=c["news"], totals=[P + n for P, n in pairs])
    cases.append(dict(base, name="prefill counting", seqs=seqs, q=c["q"], W=-1, kind="count", want=c["want"]))
    cw = pp.count_case([(253, 9)], Hq, Hkv, seed=5)  # query 0 sits at key 253: under W = 2 the later queries' windows start past the page edge
    cases.append(dict(fam="gqa", entry="prefill", rows=[0], news=cw["news"], totals=[262], name="prefill windowed counting W=2",
                      seqs=list(zip(cw["K"], cw["V"])), q=cw["q"], W=2, kind="count", want=pp.count_want_window(cw, Hq, 2)))
    d = pp.dominant_case(pairs, Hq, Hkv, page)
    cases.append(dict(base, name="prefill dominant", seqs=list(zip(d["K"], d["V"])), q=d["q"], W=-1, kind="dominant", want=d["want"]))
    return cases


def mla_reader_cases(H=MLA_H, page=MLA_PAGE):
    """17 keys, 66 keys over one page edge and 130 keys over two: multi-token counting at T in {2, 8}; dominant keys that every
    one of the T queries sees (both sides of every tile, page and split edge up to key n - T)."""
    cases = []
    for n, T in ((17, 2), (66, 8), (130, 2), (130, 8)):
        c = mm.count_case(H, T, [n], salt=T + n % 7)
        cases.append(dict(name=f"multi counting n={n} T={T}", fam="mla", entry="mla_multi", seqs=[(c["rows"][0],)], rows=[0],
                          q_nope=c["q_nope"], q_pe=c["q_pe"], totals=[n], kind="count", want=c["want"].reshape(T, H, 512)))
    for n, T in ((66, 2), (130, 8)):
        probes = sorted({p for p in ax.probe_tokens(n, ax.TILE, page, [3]) if p <= n - T} | {n - T})
        c = ax.mla_dominant_case(n, H, probes, seq=T)
        r = c["q_pe"].shape[0]
        bs = -(-r // T)
        idx = [i % r for i in range(bs * T)]
        cases.append(dict(name=f"multi dominant n={n} T={T}", fam="mla", entry="mla_multi", seqs=[(c["rows"],)], rows=[0] * bs,
                          q_nope=c["q_nope"][idx].view(bs, T, H, 512), q_pe=c["q_pe"][idx].view(bs, T, H, 64).contiguous(),
                          totals=[n] * bs, kind="dominant", want=c["want"][idx]))
    g = torch.Generator().manual_seed(3)
    seqs = [(torch.cat([ax.small_ints((n, 512), n) * 2.0 ** (n % 3), torch.randn(n, 64, generator=g).to(torch.bfloat16).float()], -1),)
            for n in (17, 130, 66)]
    cases.append(dict(name="gather", fam="mla", entry="gather", seqs=seqs, rows=[0, 1, 2, 1], totals=[17, 130, 66, 70], kind="exact",
                      dead=(3, 1)))  # table row 3 = sequence 1's pages with entry 1 (rows 64 .. 69) out of range: zeros
    return cases


# ---------------------------------------------------------------- placing rows into pages (CPU or GPU caches alike)
def place_case(caches, case, ids, quant):
    page = caches[0].shape[1]
    for s, seq in enumerate(case["seqs"]):
        for cache, rows in zip(caches, seq):
            n = rows.shape[0]
            for j, k in enumerate(case["slots"][s]):
                r0, r1 = j * page, min((j + 1) * page, n)
                if r1 > r0:
                    cache[ids[k], : r1 - r0] = quant(rows[r0:r1]).to(cache.device)


def fill_pages(caches, sentinels, page_ids):
    for cache, s in zip(caches, sentinels):
        s = s.to(cache.device)
        for p in page_ids:
            cache[p] = s


# ---------------------------------------------------------------- the CPU oracles, through the table
def logical_rows(fam, cache, table_row, n):
    """[n, ...] fp32: the first n rows of a sequence as a correct kernel reads them through its table row"""
    page = cache.shape[1]
    t = torch.arange(n)
    return widen(fam, cache[table_row.long()[t // page], t % page])


def oracle_run(case, caches, table, splits=None):
    """the case through fp64 attention on the rows the TABLE names (rounded to bf16, what a kernel returns); gather: the
    indexed rows"""
    fam, outs = case["fam"], []
    if case["entry"] == "decode":
        q = case["q"].float()
        T = q.shape[1]
        for b, L in enumerate(case["totals"]):
            K, V = (logical_rows(fam, c, table[b], L) for c in caches)
            outs.append(wr.decode64_window(q[b], K, V, mr.expanded_lengths([L], T), ax.GQA_SCALE, case["W"]))
    elif case["entry"] == "prefill":
        cu = ax.cu_of(case["news"])
        for s, (L, n) in enumerate(zip(case["totals"], case["news"])):
            K, V = (logical_rows(fam, c, table[s], L) for c in caches)
            outs.append(wr.decode64_window(case["q"][cu[s] : cu[s + 1]].float(), K, V, pp.query_lengths(L - n, n), ax.GQA_SCALE, case["W"]))
    elif case["entry"] == "mla_multi":
        T = case["q_nope"].shape[1]
        rows = [logical_rows(fam, caches[0], table[b], L) for b, L in enumerate(case["totals"])]
        outs.append(mm.multi64(case["q_nope"].float(), case["q_pe"].float(), rows, case["totals"]).flatten(0, 1))
    else:
        assert case["entry"] == "gather"
        for b, L in enumerate(case["totals"]):
            r = logical_rows(fam, caches[0], table[b].clamp(0, caches[0].shape[0] - 1), L)
            page = caches[0].shape[1]
            bad = (table[b] < 0) | (table[b] >= caches[0].shape[0])
            r[bad[torch.arange(L) // page]] = 0.0
            outs.append(r)
    return torch.cat(outs).to(torch.bfloat16)


def gather_table(case, ids, num_pages):
    table = table_of(case, ids)
    b, j = case["dead"]
    table[b, j] = num_pages
    return table


def gather_want(case):
    """the rows mla_kv_gather must return, bit for bit (fp8 pages: the widened quantised rows, by the caller)"""
    out = []
    for b, L in enumerate(case["totals"]):
        rows = case["seqs"][case["rows"][b]][0]
        r = torch.zeros(L, 576)
        r[: min(L, rows.shape[0])] = rows[:L]
        if b == case["dead"][0]:
            j = case["dead"][1]
            r[j * MLA_PAGE : (j + 1) * MLA_PAGE] = 0.0
        out.append(r)
    return torch.cat(out)


def check(case, got, fp8=False):
    """assertion (a): the closed form at the existing bars; returns the worst error"""
    if case["kind"] == "count":
        return ax.check_count(got, case["want"])
    if case["kind"] == "dominant":
        return ax.check_dominant(got, case["want"])
    want = gather_want(case).to(torch.bfloat16)
    if fp8:
        want = m8.dequant_ref(m8.quant_ref(want))
        b, j = case["dead"]
        at = sum(case["totals"][:b]) + j * MLA_PAGE
        want[at : at + min(MLA_PAGE, case["totals"][b] - j * MLA_PAGE)] = 0.0
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), "mla_kv_gather: not the indexed rows"
    return 0.0


# ---------------------------------------------------------------- writers
WRITER_SLOTS = [[3, 0], [1, 4], [5, 2]]  # batch 3, two pages each, six different pages in no order


def writer_positions(page, T=1):
    """(old lengths, [(sequence, position)] of the rows written): a page's interior, its last row(s) and, with T > 1, new rows
    across the page edge (T = 1: the first row of the second page)"""
    old = [16, page - T, page - 1 if T > 1 else page]
    return old, [(b, L + t) for b, L in enumerate(old) for t in range(T)]


def writer_table(ids):
    return torch.tensor([[ids[k] for k in row] for row in WRITER_SLOTS], dtype=torch.int32)


def write_oracle(cache, table, positions, rows):
    """what a correct append does to a cache: row i of `rows` at (sequence, position) positions[i] through the table"""
    page = cache.shape[1]
    for (b, pos), r in zip(positions, rows):
        cache[int(table[b, pos // page]), pos % page] = r
    return cache


def _first(want):
    """one expected tensor of a writer case: the tensor itself, or the central candidate of [C, ...] candidates"""
    return want[1][0] if isinstance(want, tuple) else want


def cand(t):
    """marks [C, ...] candidates (one per rsqrtf neighbour): every head of the result equals one of them as a whole"""
    return ("one of", t)


def gqa_writer_cases(fp8):
    """The single-token GQA writers at batch 3 on the caches' geometry (32 q heads, 8 KV heads): dicts of entry (the ops
    name, without the _kv_fp8 suffix), x / cos / sin, the entry's further operands, and the expected [k rows, v rows] and
    [outputs] -- from tests/row_exact.py, qk_norm_exact.py, qkv_bias_exact.py, glm4_exact.py and, for the GEMM-fused
    launch, the signed-selection projection of tests/test_gpu_row_exact.py (one exact product per element)."""
    from tests import glm4_exact as gx
    from tests import qk_norm_exact as qx
    from tests import qkv_bias_exact as bx
    from tests import row_exact as rx

    hq, hkv = GQA_HQ, GQA_HKV
    rows = qx.fp8_rows if fp8 else (lambda t: t)
    sfx = "_kv_fp8" if fp8 else ""
    cases = []
    for rt, layout in (("llama", 0), ("hf-llama", 1)):
        x, cos, sin = rx.rope_inputs(3, hq + 2 * hkv, 128, torch.bfloat16, seed=31 + layout)
        rot = rx.rope_oracle(x[:, :hq + hkv], cos, sin, layout)
        cases.append(dict(name=f"gqa_qkv_post{sfx} {rt}", entry="gqa_qkv_post", x=x, cos=cos, sin=sin, extra=[], kw=dict(rotary_type=rt),
                          want_rows=[rows(rot[:, hq:]), rows(x[:, hq + hkv:])], want_aux=[rot[:, :hq]]))
    c = qx.qk_case(3, hq, hkv)
    (_, _, yq), (_, _, yk) = qx.qk_oracle(c, 1)
    cases.append(dict(name=f"gqa_qkv_norm_post{sfx}", entry="gqa_qkv_norm_post", x=c["x"], cos=c["cos"], sin=c["sin"],
                      extra=[c["q_w"], c["k_w"], qx.EPS], kw=dict(rotary_type="hf-llama"),
                      want_rows=[cand(rows(yk)), rows(c["x"][:, hq + hkv:])], want_aux=[cand(yq)]))
    c = bx.bias_case(3, hq, hkv)
    _, q, k, v = bx.bias_oracle(c, 1)
    cases.append(dict(name=f"gqa_qkv_bias_post{sfx}", entry="gqa_qkv_bias_post", x=c["x"], cos=c["cos"], sin=c["sin"], extra=[c["bias"]],
                      kw=dict(rotary_type="hf-llama"), want_rows=[rows(k), rows(v)], want_aux=[q]))
    c = gx.glm4_case(3, hq, hkv, 64)
    _, q, k, v = gx.glm4_oracle(c)
    cases.append(dict(name=f"gqa_qkv_bias_post{sfx} glm4", entry="gqa_qkv_bias_post", x=c["x"], cos=c["cos"], sin=c["sin"], extra=[c["bias"]],
                      kw=dict(rotary_type="glm4"), want_rows=[rows(k), rows(v)], want_aux=[q]))
    if not fp8:  # bf16_linear_add_norm_qkv_post: every weight row holds one signed power of two
        M, K, N = 3, 512, (hq + 2 * hkv) * 128
        c = rx.rms_case(M, K, 1, seed=9)
        g = torch.Generator().manual_seed(8)
        W = torch.zeros(N, K)
        W[torch.arange(N), (torch.arange(N) * 37 + 5) % K] = (torch.ldexp(torch.ones(N), torch.randint(-1, 2, (N,), generator=g).int())
                                                             * (torch.randint(0, 2, (N,), generator=g) * 2 - 1))
        ang = torch.rand(M, 64, generator=g) * 6.2831853
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
        _, _, y = rx.rms_oracle(c["v"], c["w"])
        cq, ck, cv = [], [], []
        for yc in y:
            proj = (yc.float() @ W.T).to(torch.bfloat16)
            assert torch.equal(proj.double(), yc.double() @ W.double().T)
            heads = proj.view(M, hq + 2 * hkv, 128)
            rot = rx.rope_oracle(heads[:, : hq + hkv], cos, sin, 0)
            cq.append(rot[:, :hq]), ck.append(rot[:, hq:]), cv.append(heads[:, hq + hkv:])
        cases.append(dict(name="bf16_linear_add_norm_qkv_post", entry="bf16_linear_add_norm_qkv_post", x=c["x"], add=c["add"].reshape(M, K),
                          w=c["w"], wqkv=W.to(torch.bfloat16), cos=cos, sin=sin, eps=rx.EPS,
                          want_rows=[cand(torch.stack(ck)), cand(torch.stack(cv))], want_aux=[c["v"], cand(torch.stack(cq))]))
    return cases


def mla_writer_cases():
    """The single-token writers of the bf16 latent cache at batch 3: mla_kv_prep, mla_qkv_post, mla_q_proj (bs 3 fits) and
    absorb_bmm_rope_kv_fp8, on the inputs of tests/test_gpu_row_exact.py and tests/test_gpu_fused_exact.py.  The page row is
    [one kv_norm candidate, whole | RoPE(k_pe)]."""
    from oracle import fp8 as ofp8
    from tests import dense_exact as dx
    from tests import fused_exact as fx
    from tests import row_exact as rx
    from tests.test_gpu_row_exact import _mla_inputs

    def page_rows(c_kv, k_pe, cos, sin):
        _, _, y = rx.rms_oracle(c_kv["v"], c_kv["w"])
        pe = rx.rope_oracle(k_pe[:, None, :], cos, sin, 0)[:, 0]
        return cand(torch.cat([y, pe[None].expand(y.shape[0], *pe.shape)], -1).contiguous())

    B, H = 3, 5
    cases = []
    row, _, c_kv, k_pe, cos, sin = _mla_inputs(B, 0, seed=21)
    q_pe = (dx.ints(torch.Generator().manual_seed(5), 40, B, H, 64).float() * 0.25).to(torch.bfloat16)
    cases.append(dict(name="mla_kv_prep", kind="kv_prep", row=row, q_pe=q_pe, cos=cos, sin=sin, kv_w=c_kv["w"],
                      want_rows=[page_rows(c_kv, k_pe, cos, sin)], want_aux=[rx.rope_oracle(q_pe, cos, sin, 0)]))
    q_lora = 256
    row, c_q, c_kv, k_pe, cos, sin = _mla_inputs(B, q_lora, seed=41)
    _, _, yq = rx.rms_oracle(c_q["v"], c_q["w"])
    quant = [ofp8.act_quant_deepseek_v3(w_) for w_ in yq]
    both = torch.stack([torch.cat([cq.view(torch.uint8), cs.contiguous().view(torch.uint8).view(B, -1)], 1) for cq, cs in quant])
    cases.append(dict(name="mla_qkv_post", kind="qkv_post", row=row, q_lora=q_lora, q_w=c_q["w"], cos=cos, sin=sin, kv_w=c_kv["w"],
                      want_rows=[page_rows(c_kv, k_pe, cos, sin)], want_aux=[cand(both)]))  # codes | scales of ONE candidate row
    rank, N = 256, 200
    c, w = fx.norm_case(B, rank, 0, seed=1), fx.fp8_weight(N, rank)
    kv_row, _, c_kv, k_pe, cos, sin = _mla_inputs(B, 0, seed=67)
    cases.append(dict(name="mla_q_proj", kind="q_proj", row=torch.cat([c["x"], kv_row], 1), rank=rank, q_w=c["w"], q_eps=c["eps"], wq=w["w_q"],
                      ws=w["w_s"], cos=cos, sin=sin, kv_w=c_kv["w"], want_rows=[page_rows(c_kv, k_pe, cos, sin)],
                      want_aux=[dx.expect(fx.fp8_exact(c, w), torch.float32)]))
    Hn, N, K = 5, 128, 192
    c = dx.absorb_case(B, Hn, N, K, "w_uk")
    q, cos, sin, q_want = dx.rope_case(B, Hn, seed=B + Hn + N + K)
    kv_row, _, c_kv, k_pe, _, _ = _mla_inputs(B, 0, seed=80 + B + Hn)
    cases.append(dict(name="absorb_bmm_rope_kv_fp8", kind="absorb", c=c, q=q, cos=cos, sin=sin, row=kv_row, kv_w=c_kv["w"], K=K, N=N, H=Hn,
                      want_rows=[page_rows(c_kv, k_pe, cos, sin)], want_aux=[dx.expect(c["exact"], torch.bfloat16), q_want]))
    return cases
