"""Multi-token MLA paged decode (chitu_hip_mla_decode_multi / _kv_fp8: T <= 8 query tokens per sequence): the fp64 reference
written from the entry's contract, and the input builders of tests/test_gpu_mla_multi.py and tests/test_mla_multi_host.py.

Contract: seqlens[b] = L counts all keys of sequence b, the T rows of this step included; query token t sits at position
L - T + t and sees keys k <= L - T + t, i.e. the first L_t = L - T + t + 1 rows; L_t <= 0 gives zeros.  The single-token call on
the EXPANDED problem -- batch * T rows in (b, t) order, sequence b's table row repeated T times, lengths L_t -- is the same
attention.

The counting and dominant-key constructions are those of tests/attn_exact.py; wherever no key lives (rows >= L of a sequence's
last page, pages no table names) the caches hold NaN: bf16 NaN, and in the fp8 format NaN codes, NaN scales and NaN rope values."""
import torch

from tests import attn_exact as ax
from tests.test_mla_kv_fp8_host import ROW, quant_ref

PAGE = 64
SCALE = ax.MLA_SCALE


def expanded_lengths(lens, T):
    """[bs] -> [bs * T] in (b, t) order: max(0, L - T + t + 1)"""
    return [max(0, int(L) - T + t + 1) for L in lens for t in range(T)]


def multi64(q_nope, q_pe, rows, lens, scale=SCALE):
    """q_nope [bs, T, H, 512], q_pe [bs, T, H, 64]; rows[b] [>= L_b, 576] the logical rows of sequence b in token order (one
    tensor: every sequence reads the same rows) -> [bs, T, H, 512] fp64, straight from the contract."""
    bs, T, H, C = q_nope.shape
    q = torch.cat([q_nope, q_pe], -1).double()
    out = torch.zeros(bs, T, H, C, dtype=torch.float64)
    for b in range(bs):
        kv = (rows if torch.is_tensor(rows) else rows[b]).double()
        L = int(lens[b])
        for t in range(T):
            last = L - T + t  # the query's own position: the last key it sees
            if last < 0:
                continue
            k = kv[: last + 1]
            p = torch.softmax(q[b, t] @ k.T * scale, dim=-1)
            out[b, t] = p @ k[:, :C]
    return out


# ---------------------------------------------------------------- pages
def nan_fp8_row():
    row = torch.empty(ROW, dtype=torch.uint8)
    row[:512] = 0x7F                                                                  # e4m3fn NaN
    row[512:528] = torch.full((4,), float("nan")).view(torch.uint8)
    row[528:] = torch.full((64,), float("nan")).to(torch.bfloat16).view(torch.uint8)
    return row


def paged(rows_per_seq, lens, seed, spare=2, fp8=False):
    """Per-sequence logical rows (bf16 values, [n_b, 576], n_b >= L_b) -> (cache, table [bs, per + 1] int32): each sequence's
    first L_b rows in shuffled pages of 64, NaN everywhere else; the table's unused entries name whole NaN pages.  fp8: the
    656-byte rows of the quantiser's CPU statement (tests/test_mla_kv_fp8_host.py)."""
    bs = len(lens)
    per = max(1, max((int(L) + PAGE - 1) // PAGE for L in lens)) + 1
    num_pages = bs * per + spare
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))
    table = perm[: bs * per].view(bs, per).to(torch.int32)
    if fp8:
        cache = nan_fp8_row().repeat(num_pages, PAGE, 1)
    else:
        cache = torch.full((num_pages, PAGE, 576), float("nan"), dtype=torch.bfloat16)
    for b, L in enumerate(int(x) for x in lens):
        if L == 0:
            continue
        r = rows_per_seq[b][:L].to(torch.bfloat16)
        r = quant_ref(r) if fp8 else r
        for p in range((L + PAGE - 1) // PAGE):
            k = min(PAGE, L - p * PAGE)
            cache[int(table[b, p]), :k] = r[p * PAGE : p * PAGE + k]
    return cache, table.contiguous()


# ---------------------------------------------------------------- builders
def random_case(H, T, lens, seed):
    """Random q and rows; q_nope / q_pe contiguous [bs, T, H, .].  rows: list of [max(L, 1), 576] bf16-exact fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    bs = len(lens)
    rows = [torch.cat([torch.randn(max(L, 1), 512, generator=g) * (0.5 + b), torch.randn(max(L, 1), 64, generator=g)], -1)
            .to(torch.bfloat16).float() for b, L in enumerate(lens)]
    q = (torch.randn(bs, T, H, 576, generator=g) * 0.3).to(torch.bfloat16)
    return dict(q_nope=q[..., :512].contiguous(), q_pe=q[..., 512:].contiguous(), rows=rows, lens=torch.tensor(lens, dtype=torch.int32),
                T=T, seed=seed)


def count_case(H, T, lens, salt=0):
    """attn_exact's counting construction (q = 0: the output is the mean of exactly the permitted keys' indicator rows) for
    T tokens per sequence: every sequence holds the same rows; want [bs, T, H, 512] is the closed form at the expanded lengths"""
    exp = expanded_lengths(lens, T)
    c = ax.mla_count_case(max(max(lens), 1), H, seed=salt, lengths=exp, salt=salt)
    bs = len(lens)
    assert ax.max_keys_per_position_channel(c["rows"][:, :512].unsqueeze(1), ax.P_MLA) <= 16
    return dict(q_nope=c["q_nope"].view(bs, T, H, 512), q_pe=c["q_pe"].view(bs, T, H, 64), rows=[c["rows"]] * bs,
                lens=torch.tensor(lens, dtype=torch.int32), T=T, want=c["want"].reshape(bs, T, H, 512), seed=salt)


CAUSAL = [(2, 65), (5, 67), (8, 200), (4, 4)]  # (T, L) of the causality probes


def causal_probe_case(H, T, L, probes=None):
    """attn_exact's dominant-key construction as a causality probe.  Sequence i (i in `probes`, default 0 .. T - 2) has its dominant key at
    position L - T + i + 1, one past token i's horizon, in rope channel i, and all its T query tokens steer to that channel.
    Tokens t > i see the key: their output is its latent row (`seen`, within ABS_DOMINANT).  Tokens t <= i do not: every key
    they see scores 0, their output is the mean of their visible latent rows (multi64), far from the key's row.  A kernel that
    masks by L instead of L_t hands tokens t <= i the key's row."""
    assert T >= 2 and L >= T
    probes = list(range(T - 1)) if probes is None else list(probes)
    bs = len(probes)
    rows, pos = [], []
    q_pe = torch.zeros(bs, T, H, 64)
    for n, i in enumerate(probes):
        p = L - T + i + 1
        latent = ax.identity_rows(L, 1, 512, seq=i)[:, 0]
        rope = torch.zeros(L, 64)
        rope[p, i] = ax.K_AMP
        rows.append(ax.mla_rows(latent, rope))
        q_pe[n, :, :, i] = ax.Q_AMP
        pos.append(p)
    assert ax.margin_nats(ax.Q_AMP, ax.K_AMP, SCALE) >= ax.MIN_MARGIN_NATS
    return dict(q_nope=torch.zeros(bs, T, H, 512, dtype=torch.bfloat16), q_pe=q_pe.to(torch.bfloat16), rows=rows,
                lens=torch.full((bs,), L, dtype=torch.int32), T=T, pos=pos, probes=probes, seed=L)


def expand(case, table):
    """The expanded single-token problem of a case: q [bs * T, H, .], the table rows repeated T times, the lengths L_t"""
    bs, T, H, _ = case["q_nope"].shape
    return (case["q_nope"].reshape(bs * T, H, 512), case["q_pe"].reshape(bs * T, H, 64), table.repeat_interleave(T, dim=0).contiguous(),
            torch.tensor(expanded_lengths(case["lens"].tolist(), T), dtype=torch.int32))


def same_tile(lens, T):
    """do all T tokens of every sequence end in the same 64-key tile (ceil(L_t / 64) equal for all t)?"""
    return all(len({-(-x // 64) for x in expanded_lengths([L], T)}) == 1 for L in lens)
