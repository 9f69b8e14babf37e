"""Token sampling on the GPU: the step right after the decode hot path.

Reference (read-only): `NormalExecutor.update_response` chitu/executor.py:82-112 (frequency penalty,
argmax for all-greedy batches, else softmax(logits / temperature) + top-k / top-p sampling) and
`top_k_top_p_min_p_sampling_from_probs_torch` chitu/utils.py:62-81 (full sort + cumsum + multinomial).
Here: `chitu_hip_frequency_penalty` + ONE `chitu_hip_sample` launch (csrc/sample.hip, no sort), tokens
stay on the device, everything is hipGraph-capturable.

Semantics kept: penalty only for rows with frequency_penalty > 0 and a non-empty response; a batch is
greedy iff every top_k <= 1; a top_k of 1 inside a sampling batch keeps only the arg-max; an entry at
sorted position `pos` survives iff pos < top_k and its exclusive cumulative probability <= top_p.
Conscious differences: a top_k <= 0 inside a sampling batch means "no top-k limit" (serve.py:52
documents -1 that way; the reference's mask zeroes the whole row and multinomial fails); ties in the
sorted order go to the lower token id (torch.sort leaves them unspecified); the draw is an inverse CDF
driven by one uniform per row from a torch.Generator (multinomial's exponential-race draw has the same
distribution but another stream).

No reference counterpart: speculative decoding.  `generate_speculative_greedy` / `generate_speculative_sampled` are the
draft-and-verify loops of the decoders' generate_speculative / generate_speculative_sampled; the sampled one judges the drafts on the
device with ONE `chitu_hip_speculative_verify` call per round (`speculative_verify`; rule and proof in DESIGN 3.9).  `ModelDrafter`
drafts with a second, smaller decoder of this package on the device; where it samples its drafts the round is judged by
`chitu_hip_speculative_verify_sampled` (`speculative_verify_sampled`: accept with min(1, p / q), replace from max(p - q, 0)).
"""

from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, float_dtype_code, i32, i64, ptr, require_cuda, stream_ptr

__all__ = [
    "apply_frequency_penalty",
    "argmax",
    "top_k_top_p_sampling_from_logits",
    "top_k_top_p_min_p_sampling_from_probs_torch",
    "sample_tokens",
    "DeviceSampler",
    "NgramDrafter",
    "ModelDrafter",
    "speculative_verify",
    "speculative_verify_sampled",
    "generate_speculative_greedy",
    "generate_speculative_sampled",
]


def _rows(t: torch.Tensor, writable: bool = False) -> Tuple[torch.Tensor, int, int]:
    """[rows, vocab] with a unit stride along the vocabulary.  Read-only consumers take a dense copy of a strided input
    (e.g. the permuted view a library all-gather hands back); in-place ones refuse it."""
    assert t.dim() >= 1
    if t.stride(-1) != 1 and not writable:
        t = t.contiguous()
    t2 = t.reshape(-1, t.shape[-1]) if not writable else t.view(-1, t.shape[-1])
    assert t2.stride(-1) == 1, "the vocabulary axis must be contiguous"
    return t2, t2.shape[0], t2.shape[1]


def apply_frequency_penalty(logits: torch.Tensor, responses: Sequence[Sequence[int]],
                            frequency_penalties: Sequence[float]) -> torch.Tensor:
    """logits[row, t] -= penalty[row] for every occurrence of t in responses[row], in place
    (executor.py:89-102).  Rows with penalty <= 0 or an empty response are untouched."""
    require_cuda(logits)
    assert logits.dtype == torch.float32, "fp32 logits (model.py:475 casts them)"
    lg, rows, vocab = _rows(logits, writable=True)
    assert len(responses) == rows and len(frequency_penalties) == rows
    if not any(p > 0 and len(r) > 0 for p, r in zip(frequency_penalties, responses)):
        return logits
    flat: List[int] = []
    offs = [0]
    for r in responses:
        flat.extend(int(t) for t in r)
        offs.append(len(flat))
    dev = logits.device
    tok = torch.tensor(flat if flat else [0], dtype=torch.int32, device=dev)
    off = torch.tensor(offs, dtype=torch.int32, device=dev)
    pen = torch.tensor([float(p) for p in frequency_penalties], dtype=torch.float32, device=dev)
    return apply_frequency_penalty_device(logits, tok, off, pen)


def apply_frequency_penalty_device(logits, tokens_i32, offsets_i32, penalties_f32):
    """Same with the ragged response lists already on the device (graph-capturable): tokens_i32 flat,
    offsets_i32 [rows + 1], penalties_f32 [rows]."""
    require_cuda(logits, tokens_i32, offsets_i32, penalties_f32)
    lg, rows, vocab = _rows(logits, writable=True)
    assert logits.dtype == torch.float32
    assert tokens_i32.dtype == torch.int32 and offsets_i32.dtype == torch.int32 and penalties_f32.dtype == torch.float32
    assert offsets_i32.numel() == rows + 1 and penalties_f32.numel() == rows
    check(_lib.lib().chitu_hip_frequency_penalty(ptr(lg), i64(lg.stride(0)), i64(rows), i32(vocab), ptr(tokens_i32),
                                                 ptr(offsets_i32), ptr(penalties_f32), stream_ptr()),
          "frequency_penalty")
    return logits


def _launch(x, temperatures, top_ks, top_ps, uniforms, probs_mode, out, stats):
    x2, rows, vocab = _rows(x)
    n_kept = mass = None
    if stats:
        n_kept = torch.empty(rows, dtype=torch.int32, device=x.device)
        mass = torch.empty(rows, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=x.device)
    assert out.dtype == torch.int64 and out.numel() == rows and out.is_contiguous()
    check(_lib.lib().chitu_hip_sample(ptr(x2), float_dtype_code(x.dtype), i64(x2.stride(0)), i64(rows), i32(vocab),
                                      ptr(temperatures), ptr(top_ks), ptr(top_ps), ptr(uniforms), i32(probs_mode),
                                      ptr(out), ptr(n_kept), ptr(mass), stream_ptr()), "sample")
    return (out, n_kept, mass) if stats else out


def argmax(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Greedy tokens [rows] int64 (executor.py:103-104): first index of the row maximum."""
    require_cuda(logits)
    return _launch(logits, None, None, None, None, 0, out, False)


def _per_row(v, rows, dtype, device):
    if isinstance(v, torch.Tensor):
        t = v.to(device=device, dtype=dtype).contiguous().view(-1)
    else:
        t = torch.tensor(list(v), dtype=dtype, device=device)
    assert t.numel() == rows
    return t


def _uniforms(rows, device, uniforms, generator):
    if uniforms is not None:
        return _per_row(uniforms, rows, torch.float32, device)
    return torch.rand(rows, dtype=torch.float32, device=device, generator=generator)


def top_k_top_p_sampling_from_logits(logits, temperatures, top_ks, top_ps, uniforms=None, generator=None,
                                     out=None, return_stats=False):
    """softmax(logits / temperature) -> top-k / top-p mask -> one draw per row, in one launch
    (executor.py:106-109).  `uniforms` [rows] in [0, 1) makes the draw reproducible; otherwise they
    come from `generator` (a CUDA torch.Generator) or the default one.  return_stats: also the
    number of kept tokens and their probability mass per row."""
    require_cuda(logits)
    _, rows, _ = _rows(logits)
    dev = logits.device
    return _launch(logits, _per_row(temperatures, rows, torch.float32, dev), _per_row(top_ks, rows, torch.int32, dev),
                   _per_row(top_ps, rows, torch.float32, dev), _uniforms(rows, dev, uniforms, generator), 0, out,
                   return_stats)


def top_k_top_p_min_p_sampling_from_probs_torch(probs, top_ks, top_ps, min_ps=None, uniforms=None, generator=None,
                                                return_stats=False):
    """Same name and arguments as chitu/utils.py:62-81 (min_ps is unused there too), on probabilities."""
    assert min_ps is None, "min_p is a TODO in the reference (utils.py:66) and is not implemented"
    require_cuda(probs)
    _, rows, _ = _rows(probs)
    dev = probs.device
    return _launch(probs, None, _per_row(top_ks, rows, torch.int32, dev), _per_row(top_ps, rows, torch.float32, dev),
                   _uniforms(rows, dev, uniforms, generator), 1, None, return_stats)


def sample_tokens(logits, temperatures, top_ks, top_ps, frequency_penalties=None, responses=None, uniforms=None,
                  generator=None):
    """update_response's device work (executor.py:82-109) for a decode batch: optional frequency
    penalty, then argmax if every top_k <= 1 (`is_all_greedy`, task.py:457) else the sampling launch.
    logits [rows, vocab] fp32 (penalised in place, like the reference); returns int64 tokens on the
    device (the reference's one `.cpu()` per step is the caller's choice)."""
    logits2, rows, _ = _rows(logits)
    if frequency_penalties is not None and responses is not None:
        apply_frequency_penalty(logits2, responses, frequency_penalties)
    ks = [int(k) for k in (top_ks.tolist() if isinstance(top_ks, torch.Tensor) else top_ks)]
    if all(k <= 1 for k in ks):
        return argmax(logits2)
    return top_k_top_p_sampling_from_logits(logits2, temperatures, ks, top_ps, uniforms=uniforms, generator=generator)


class DeviceSampler:
    """Sampling state of one generate() call kept on the device: the per-request parameters
    (task.py:433-457 gathers them from the requests every step), the tokens generated so far (the
    frequency penalty's input, executor.py:89-102) and the uniform stream.  Calling it with the step's
    fp32 logits [n_req, vocab] returns the int64 tokens [n_req] without a host round trip: at most one
    penalty launch, one sampling launch, and the bookkeeping copies.

    Greedy iff every top_k <= 1 (`is_all_greedy`, task.py:457) -- also the default when no sampling
    parameter is given.  `generator`: a CUDA torch.Generator for the uniforms (reproducible runs)."""

    def __init__(self, n_req: int, max_new_tokens: int, device, temperatures=None, top_ks=None, top_ps=None,
                 frequency_penalties=None, generator=None):
        self.n_req, self.device, self.generator = n_req, torch.device(device), generator
        ks = [1] * n_req if top_ks is None else [int(k) for k in (top_ks.tolist() if isinstance(top_ks, torch.Tensor) else top_ks)]
        assert len(ks) == n_req
        self.greedy = all(k <= 1 for k in ks)
        if not self.greedy:
            self.top_ks = _per_row(ks, n_req, torch.int32, self.device)
            self.temperatures = _per_row([1.0] * n_req if temperatures is None else temperatures, n_req, torch.float32, self.device)
            self.top_ps = _per_row([1.0] * n_req if top_ps is None else top_ps, n_req, torch.float32, self.device)
        pens = None if frequency_penalties is None else [float(p) for p in frequency_penalties]
        self.penalise = pens is not None and any(p > 0 for p in pens)
        if self.penalise:
            assert len(pens) == n_req
            self.penalties = torch.tensor(pens, dtype=torch.float32, device=self.device)
            self.history = torch.zeros(n_req, max(max_new_tokens, 1), dtype=torch.int32, device=self.device)
            self.row_ids = torch.arange(n_req + 1, dtype=torch.int32, device=self.device)
        self.n_generated = 0

    def __call__(self, logits: torch.Tensor) -> torch.Tensor:
        lg, rows, _ = _rows(logits)
        assert rows == self.n_req
        t = self.n_generated
        if self.penalise:
            assert t <= self.history.shape[1], "DeviceSampler: more calls than max_new_tokens (the penalty history is full)"
        if self.penalise and t > 0:
            # every request has generated exactly t tokens: row r's list is history[r, :t]
            flat = self.history[:, :t].contiguous().view(-1)  # (a [n, 1] slice would otherwise reshape to a strided view)
            apply_frequency_penalty_device(lg, flat, self.row_ids * t, self.penalties)
        if self.greedy:
            tok = argmax(lg)
        else:
            tok = top_k_top_p_sampling_from_logits(lg, self.temperatures, self.top_ks, self.top_ps, generator=self.generator)
        if self.penalise and t < self.history.shape[1]:
            self.history[:, t] = tok.to(torch.int32)
        self.n_generated = t + 1
        return tok


class NgramDrafter:
    """Prompt-lookup drafts for LlamaDecoder.generate_speculative: propose(history, k) returns the k tokens that followed the
    latest EARLIER occurrence of the history's last n tokens (an occurrence that ends before the history's end, so it has at
    least one token behind it); where that continuation runs into the end of the history it goes on repeating the last token it
    gave.  No earlier occurrence (or fewer than n tokens of history): the last token k times.  Runs on the host over Python ints
    -- the verify step's accepted counts go to the host every round anyway."""

    def __init__(self, n: int = 2):
        if n < 1:
            raise ValueError(f"NgramDrafter(n={n}): the lookup key has at least one token")
        self.n = n

    def propose(self, history: Sequence[int], k: int) -> List[int]:
        h = [int(t) for t in history]
        assert h and k >= 0
        n = self.n
        out: List[int] = []
        if len(h) > n:
            key = h[-n:]
            for start in range(len(h) - n - 1, -1, -1):  # latest first; start + n <= len(h) - 1: one token follows at least
                if h[start : start + n] == key:
                    out = h[start + n : start + n + k]
                    break
        fill = out[-1] if out else h[-1]
        return out + [fill] * (k - len(out))


def speculative_verify(logits, drafts, T, temperatures, top_ks, top_ps, uniforms=None, generator=None, probs_mode=False,
                       return_rows=False):
    """Draft verification of speculative decoding with sampling, one call (chitu_hip_speculative_verify: a launch over the rows and a
    tiny one over the sequences; new: the reference has no speculative path).  logits [bs * T, vocab] (or [bs, T, vocab]): row (b, t) is the target model's distribution for the token
    after position t of sequence b, under the row's temperature / top_k / top_p exactly as top_k_top_p_sampling_from_logits
    draws from it (probs_mode: the rows are probabilities, temperatures may be None).  drafts [bs * T] int32: the deterministic
    proposal for that token, -1 at each sequence's last row.  A draft d is accepted with probability p(d); the first rejected
    row emits a draw from p without d, renormalised, and the row after the last draft a plain draw -- so every emitted token is
    distributed as p.  uniforms [bs * T, 2] in [0, 1) (acceptance, replacement) make the result reproducible; otherwise they come
    from `generator` (a CUDA torch.Generator) or the default one.

    Returns out [bs, T + 1] int64 on the device: column 0 the number of emitted tokens (leading accepted drafts + 1), then the
    tokens, then -1.  return_rows: also (accepted [bs * T] int32, row_tokens [bs * T] int64), the per-row results."""
    require_cuda(logits)
    x2, rows, vocab = _rows(logits)
    T = int(T)
    if T < 2 or rows % T:
        raise ValueError(f"speculative_verify: {rows} rows are not sequences of T={T} >= 2 rows")
    dev = logits.device
    d = _per_row(drafts, rows, torch.int32, dev)
    if uniforms is None:
        u = torch.rand(rows, 2, dtype=torch.float32, device=dev, generator=generator)
    else:
        u = _per_row(uniforms, rows * 2, torch.float32, dev)
    temps = None if probs_mode and temperatures is None else _per_row(temperatures, rows, torch.float32, dev)
    ks, ps = _per_row(top_ks, rows, torch.int32, dev), _per_row(top_ps, rows, torch.float32, dev)
    out = torch.empty(rows // T, T + 1, dtype=torch.int64, device=dev)
    accepted = row_tokens = None
    if return_rows:
        accepted = torch.empty(rows, dtype=torch.int32, device=dev)
        row_tokens = torch.empty(rows, dtype=torch.int64, device=dev)
    check(_lib.lib().chitu_hip_speculative_verify(ptr(x2), float_dtype_code(x2.dtype), i64(x2.stride(0)), i64(rows), i32(vocab),
                                                  ptr(temps), ptr(ks), ptr(ps), ptr(d), ptr(u), i32(T), i32(1 if probs_mode else 0),
                                                  ptr(out), ptr(accepted), ptr(row_tokens), stream_ptr()), "speculative_verify")
    return (out, accepted, row_tokens) if return_rows else out


def speculative_verify_sampled(logits, draft_logits, drafts, T, temperatures, top_ks, top_ps, uniforms=None, generator=None,
                               probs_mode=False, return_rows=False):
    """speculative_verify for drafts that were SAMPLED (chitu_hip_speculative_verify_sampled; new: the reference has no speculative
    path): draft_logits [bs * T, vocab] (or [bs, T, vocab]; any float dtype, its own row stride) holds, in row (b, t), the draft
    model's logits that drafts[b * T + t] was drawn from under the row's own temperature / top_k / top_p -- the parameters apply to
    both rows of a pair.  With p the target row's distribution and q the draft row's, a draft d is accepted with probability
    min(1, p(d) / q(d)) and the first rejected row emits a draw from max(p - q, 0), renormalised: every emitted token is distributed
    as p, whatever q is, provided q is what d was drawn from.  The draft row of each sequence's last row (drafts -1) is never read.
    Everything else -- uniforms [bs * T, 2], the result [bs, T + 1], return_rows -- as speculative_verify."""
    require_cuda(logits, draft_logits)
    x2, rows, vocab = _rows(logits)
    q2, q_rows, q_vocab = _rows(draft_logits)
    T = int(T)
    if T < 2 or rows % T:
        raise ValueError(f"speculative_verify_sampled: {rows} rows are not sequences of T={T} >= 2 rows")
    if (q_rows, q_vocab) != (rows, vocab):
        raise ValueError(f"speculative_verify_sampled: draft_logits [{q_rows}, {q_vocab}] against logits [{rows}, {vocab}]")
    dev = logits.device
    d = _per_row(drafts, rows, torch.int32, dev)
    if uniforms is None:
        u = torch.rand(rows, 2, dtype=torch.float32, device=dev, generator=generator)
    else:
        u = _per_row(uniforms, rows * 2, torch.float32, dev)
    temps = None if probs_mode and temperatures is None else _per_row(temperatures, rows, torch.float32, dev)
    ks, ps = _per_row(top_ks, rows, torch.int32, dev), _per_row(top_ps, rows, torch.float32, dev)
    out = torch.empty(rows // T, T + 1, dtype=torch.int64, device=dev)
    accepted = row_tokens = None
    if return_rows:
        accepted = torch.empty(rows, dtype=torch.int32, device=dev)
        row_tokens = torch.empty(rows, dtype=torch.int64, device=dev)
    check(_lib.lib().chitu_hip_speculative_verify_sampled(
        ptr(x2), float_dtype_code(x2.dtype), i64(x2.stride(0)), ptr(q2), float_dtype_code(q2.dtype), i64(q2.stride(0)), i64(rows),
        i32(vocab), ptr(temps), ptr(ks), ptr(ps), ptr(d), ptr(u), i32(T), i32(1 if probs_mode else 0), ptr(out), ptr(accepted),
        ptr(row_tokens), stream_ptr()), "speculative_verify_sampled")
    return (out, accepted, row_tokens) if return_rows else out


class ModelDrafter:
    """Drafts from a draft MODEL: any decoder of this package (prefill, decode, cache, device, args.vocab_size) with the target's
    vocabulary, built by the caller with a paged cache of its own -- Llama-3.2-3B for Llama-3-8B, a shallow stack for a deep one.
    Both speculative loops take it (they look for `draft`; a drafter with only propose(history, k) takes the host path):

      start(prompts, req_ids)   prefills the draft model (the logits are dropped).
      draft(last_tokens, req_ids, draft_len, temperatures, top_ks, top_ps, generator) -> (drafts, draft_logits)
                                draft_len + 1 graph-replayed decode steps from last_tokens [n] int64 on the device.  Step s's token
                                is picked on the device -- arg-max, or with sample=True and top_ks given
                                top_k_top_p_sampling_from_logits under the requests' parameters ([n] each) with uniforms from
                                `generator` -- and feeds step s + 1 without visiting the host, as generate() does.  drafts
                                [n, draft_len] int64; draft_logits [n, draft_len + 1, vocab] f32 where the drafts were sampled
                                (each draft's logits, copied out of the graph's static output before the next replay; the last
                                row is unused and left unwritten), else None -- arg-max drafts keep no logits.
      settle(req_ids, kept)     after the verify step emitted kept[b] tokens: the draft cache goes back to the target's length.
                                Pairs with draft(): it gives back the rows that the request's LAST draft() appended, less
                                kept[b], and raises for a request that has no draft() since its last settle().
      retire(req_id)            frees the request's pages.

    The step after the last draft is ALWAYS run: it appends the last draft's row, which a request that accepts every draft needs
    and would otherwise lack, so after a round every request's draft cache holds last token + all drafts and settle() is one
    rollback of draft_len + 1 - kept[b] rows -- no second, ragged catch-up step with a batch (and a captured graph) of its own, and
    nothing in the round waits for the verify result."""

    def __init__(self, model, sample=True):
        for name in ("prefill", "decode", "cache", "device", "args"):
            if not hasattr(model, name):
                raise TypeError(f"ModelDrafter: the draft model has no {name!r}")
        self.model, self.sample = model, bool(sample)
        self._appended = {}  # req_id -> rows its last draft() appended and no settle() has accounted for yet

    def check_target(self, target):
        """ValueError unless the draft model can draft for `target` (the loops call this before anything is prefilled)"""
        if int(self.model.args.vocab_size) != int(target.args.vocab_size):
            raise ValueError(f"ModelDrafter: the draft model's vocabulary ({self.model.args.vocab_size}) differs from the "
                             f"target's ({target.args.vocab_size})")
        if self.model.cache is target.cache:
            raise ValueError("ModelDrafter: the draft model shares the target's cache object; it needs a paged cache of its own")

    def start(self, prompts, req_ids):
        self.model.prefill(prompts, list(req_ids))

    def draft(self, last_tokens, req_ids, draft_len, temperatures=None, top_ks=None, top_ps=None, generator=None, use_graph=True):
        m, ids = self.model, list(req_ids)
        n = len(ids)
        assert last_tokens.dtype == torch.int64 and tuple(last_tokens.shape) == (n,)
        sampled = self.sample and top_ks is not None
        drafts = torch.empty(n, draft_len, dtype=torch.int64, device=m.device)
        kept_logits = torch.empty(n, draft_len + 1, int(m.args.vocab_size), dtype=torch.float32, device=m.device) if sampled else None
        tok = last_tokens
        for r in ids:
            if r in self._appended:
                raise RuntimeError(f"ModelDrafter.draft: request {r!r} has a draft() that no settle() followed")
            self._appended[r] = draft_len + 1  # settle() gives back all but the kept ones
        for s in range(draft_len + 1):
            m.cache.prepare_cache_decode(ids)
            m.cache.prepare_block_table_for_decode(ids)
            logits = m.decode(tok, use_graph=use_graph)
            m.cache.finalize_cache_single_decode(ids)
            if kept_logits is not None and s < draft_len:  # the row after the last draft judges nothing
                kept_logits[:, s].copy_(logits)
            if s < draft_len:
                if sampled:
                    tok = top_k_top_p_sampling_from_logits(logits, temperatures, top_ks, top_ps, generator=generator)
                else:
                    tok = argmax(logits)
                drafts[:, s] = tok
        return drafts, kept_logits

    def settle(self, req_ids, kept):
        """the requests' last draft() appended draft_len + 1 rows each, the target kept kept[b] (1 .. draft_len + 1) of them"""
        ids = list(req_ids)
        missing = [r for r in ids if r not in self._appended]
        if missing:
            raise RuntimeError(f"ModelDrafter.settle: no draft() to settle for {missing!r}")
        self.model.cache.rollback(ids, [self._appended.pop(r) - int(k) for r, k in zip(ids, kept)])

    def retire(self, req_id):
        self._appended.pop(req_id, None)
        self.model.cache.finalize_cache_all_decode(req_id)


def _check_draft_len(draft_len, max_q):
    if not 1 <= draft_len <= max_q - 1:
        raise ValueError(f"draft_len={draft_len}: a verify step holds the last token and 1 .. {max_q - 1} drafts")


def _propose_drafts(drafter, prompts, out, live, draft_len):
    """draft_len tokens per live request from the drafter, history = prompt + tokens so far"""
    drafts = []
    for i in live:
        d = [int(t) for t in drafter.propose(list(prompts[i]) + out[i], draft_len)]
        assert len(d) == draft_len, f"drafter proposed {len(d)} tokens, not draft_len={draft_len}"
        drafts.append(d)
    return drafts


def _retire_finished(model, req_ids, out, live, max_new_tokens):
    """requests that have max_new_tokens leave the batch and return their pages"""
    for i in [i for i in live if len(out[i]) >= max_new_tokens]:
        model.cache.finalize_cache_all_decode(req_ids[i])
        live.remove(i)


def _finish_speculative(model, out, stats, max_new_tokens):
    from . import tensor_parallel as tp

    model.speculative_stats = stats
    if tp.xgmi_comm() is not None:
        torch.cuda.current_stream().synchronize()
        tp.check_comm()
    return torch.tensor([o[:max_new_tokens] for o in out], dtype=torch.int64, device=model.device)


def _start_model_drafter(model, drafter, prompts, req_ids):
    if hasattr(drafter, "check_target"):
        drafter.check_target(model)
    drafter.start(prompts, req_ids)


def _retire_finished_drafted(model, drafter, req_ids, out, live, last, max_new_tokens):
    """_retire_finished for both models; returns `last` (the live requests' last tokens, on the device) without the rows that left"""
    gone = [i for i in live if len(out[i]) >= max_new_tokens]
    if not gone:
        return last
    keep = [j for j, i in enumerate(live) if i not in gone]
    for i in gone:
        model.cache.finalize_cache_all_decode(req_ids[i])
        drafter.retire(req_ids[i])
        live.remove(i)
    return last[torch.tensor(keep, dtype=torch.int64, device=last.device)] if keep else last[:0]


def _generate_speculative_greedy_drafted(model, prompts, max_new_tokens, drafter, draft_len, req_ids, use_graph):
    """generate_speculative_greedy with a drafter that drafts on the device (ModelDrafter's protocol): arg-max drafts, today's
    comparison.  The step tensor is assembled on the device and the next round's last tokens are gathered there; one device ->
    host copy per round carries the drafts and the arg-maxes."""
    n_req, T = len(prompts), draft_len + 1
    _start_model_drafter(model, drafter, prompts, req_ids)
    last = argmax(model.prefill(prompts, req_ids))
    out = [[t] for t in last.tolist()]
    stats = {"steps": 0, "accepted": 0, "drafted": 0}
    live = list(range(n_req))
    if max_new_tokens <= 1:
        live = []
        for r in req_ids:
            model.cache.finalize_cache_all_decode(r)
            drafter.retire(r)
    while live:
        ids = [req_ids[i] for i in live]
        drafts, _ = drafter.draft(last, ids, draft_len, use_graph=use_graph)
        model.cache.prepare_block_table_for_decode_multi(ids, T)
        logits = model.decode_multi(torch.cat([last.view(-1, 1), drafts], dim=1), use_graph=use_graph)
        best = argmax(logits.view(len(live) * T, -1)).view(len(live), T)
        n_ok = (drafts == best[:, :draft_len]).to(torch.int64).cumprod(dim=1).sum(dim=1, keepdim=True)
        last = best.gather(1, n_ok).view(-1)  # the bonus token: the next round's last token, never off the device
        both = torch.cat([drafts, best], dim=1).tolist()
        kept = []
        for i, row in zip(live, both):
            d, a = row[:draft_len], row[draft_len:]
            k = 0
            while k < draft_len and d[k] == a[k]:
                k += 1
            out[i].extend(d[:k] + [a[k]])
            kept.append(k + 1)
            stats["accepted"] += k
            stats["drafted"] += draft_len
        stats["steps"] += 1
        model.cache.finalize_cache_multi_decode(ids, kept)
        drafter.settle(ids, kept)
        last = _retire_finished_drafted(model, drafter, req_ids, out, live, last, max_new_tokens)
    return _finish_speculative(model, out, stats, max_new_tokens)


def _generate_speculative_sampled_drafted(model, prompts, max_new_tokens, drafter, draft_len, temps, ks, ps, pens, generator, req_ids,
                                          use_graph):
    """generate_speculative_sampled with a drafter that drafts on the device (ModelDrafter's protocol).  The drafter draws each
    draft from ITS distribution q under the request's temperature / top_k / top_p (without the frequency penalty: the rule is
    lossless for any q, provided q is what d was drawn from) and hands over the logits; speculative_verify_sampled judges the
    round.  A drafter that does not sample (sample=False, or every top_k <= 1) proposes arg-maxes: a point mass, judged by
    speculative_verify.  Without a penalty the round's only device -> host copy is the [bs, T + 1] result; with one, the drafts
    travel too (the penalty of row t counts them, as with a host drafter)."""
    n_req, T = len(prompts), draft_len + 1
    dev = model.device
    greedy = all(k <= 1 for k in ks)
    penalise = any(p > 0 for p in pens)
    _start_model_drafter(model, drafter, prompts, req_ids)
    last = sample_tokens(model.prefill(prompts, req_ids), temps, ks, ps, generator=generator)
    out = [[t] for t in last.tolist()]
    stats = {"steps": 0, "accepted": 0, "drafted": 0}
    live = list(range(n_req))
    if max_new_tokens <= 1:
        live = []
        for r in req_ids:
            model.cache.finalize_cache_all_decode(r)
            drafter.retire(r)
    params_of = None
    no_draft = None
    while live:
        ids = [req_ids[i] for i in live]
        n = len(live)
        if params_of != live:  # the parameters on the device, per request (the drafter's) and per row (the verify launch's)
            params_of = list(live)
            req_params = [_per_row([v[i] for i in live], n, dt, dev) for v, dt in ((temps, torch.float32), (ks, torch.int32), (ps, torch.float32))]
            dev_params = [v.repeat_interleave(T) for v in req_params]
            no_draft = torch.full((n, 1), -1, dtype=torch.int64, device=dev)
        if greedy:
            drafts, draft_logits = drafter.draft(last, ids, draft_len, use_graph=use_graph)
        else:
            drafts, draft_logits = drafter.draft(last, ids, draft_len, *req_params, generator=generator, use_graph=use_graph)
        model.cache.prepare_block_table_for_decode_multi(ids, T)
        logits = model.decode_multi(torch.cat([last.view(-1, 1), drafts], dim=1), use_graph=use_graph).view(n * T, -1)
        if penalise:
            host_drafts = drafts.tolist()
            apply_frequency_penalty(logits, [out[i] + d[:t] for i, d in zip(live, host_drafts) for t in range(T)],
                                    [pens[i] for i in live for _ in range(T)])
        row_drafts = torch.cat([drafts, no_draft], dim=1).to(torch.int32).view(-1)
        if draft_logits is not None and not greedy:
            res = speculative_verify_sampled(logits, draft_logits.view(n * T, -1), row_drafts, T, *dev_params, generator=generator)
        else:
            res = speculative_verify(logits, row_drafts, T, *dev_params, generator=generator)
        last = res.gather(1, res[:, :1]).view(-1)  # column n_emitted holds the last emitted token
        kept = []
        for i, row in zip(live, res.tolist()):
            out[i].extend(row[1 : 1 + row[0]])
            kept.append(row[0])
            stats["accepted"] += row[0] - 1
            stats["drafted"] += draft_len
        stats["steps"] += 1
        model.cache.finalize_cache_multi_decode(ids, kept)
        drafter.settle(ids, kept)
        last = _retire_finished_drafted(model, drafter, req_ids, out, live, last, max_new_tokens)
    return _finish_speculative(model, out, stats, max_new_tokens)


def generate_speculative_greedy(model, prompts, max_new_tokens, drafter, draft_len, max_q, req_ids=None, use_graph=True,
                                sampling_args=()):
    """The draft-and-verify loop of LlamaDecoder / DeepSeekV3Decoder.generate_speculative (their docstrings state the contract):
    model-independent, it needs model.prefill, model.decode_multi, model.cache and model.device, and leaves
    model.speculative_stats.  max_q: the most tokens a verify step of the model holds (the last token + max_q - 1 drafts).
    A drafter with `draft` (ModelDrafter) drafts arg-maxes on the device; one with only propose(history, k) takes the host path."""
    if any(a is not None for a in sampling_args):
        raise NotImplementedError("generate_speculative is greedy (it accepts a draft iff draft == argmax): "
                                  "generate_speculative_sampled takes temperatures, top_ks, top_ps and frequency_penalties")
    _check_draft_len(draft_len, max_q)
    n_req = len(prompts)
    req_ids = [f"gen{i}" for i in range(n_req)] if req_ids is None else list(req_ids)
    if hasattr(drafter, "draft"):  # a drafter that drafts on the device (ModelDrafter)
        return _generate_speculative_greedy_drafted(model, prompts, max_new_tokens, drafter, draft_len, req_ids, use_graph)
    T = draft_len + 1
    first = argmax(model.prefill(prompts, req_ids)).tolist()
    out = [[t] for t in first]
    stats = {"steps": 0, "accepted": 0, "drafted": 0}
    live = list(range(n_req))
    if max_new_tokens <= 1:
        live = []
        for r in req_ids:
            model.cache.finalize_cache_all_decode(r)
    while live:
        drafts = _propose_drafts(drafter, prompts, out, live, draft_len)
        ids = [req_ids[i] for i in live]
        model.cache.prepare_block_table_for_decode_multi(ids, T)
        step = torch.tensor([[out[i][-1]] + d for i, d in zip(live, drafts)], dtype=torch.int64, device=model.device)
        logits = model.decode_multi(step, use_graph=use_graph)
        best = argmax(logits.view(len(live) * T, -1)).view(len(live), T).tolist()
        kept = []
        for i, d, a in zip(live, drafts, best):
            n_ok = 0
            while n_ok < draft_len and d[n_ok] == a[n_ok]:
                n_ok += 1
            out[i].extend(d[:n_ok] + [a[n_ok]])
            kept.append(n_ok + 1)
            stats["accepted"] += n_ok
            stats["drafted"] += draft_len
        stats["steps"] += 1
        model.cache.finalize_cache_multi_decode(ids, kept)
        _retire_finished(model, req_ids, out, live, max_new_tokens)
    return _finish_speculative(model, out, stats, max_new_tokens)


def generate_speculative_sampled(model, prompts, max_new_tokens, drafter, draft_len, max_q, temperatures, top_ks, top_ps,
                                 frequency_penalties=None, generator=None, req_ids=None, use_graph=True):
    """generate_speculative_greedy's loop with the acceptance rule in sampling form (the decoders' generate_speculative_sampled
    docstrings state the contract).  The first token is sampled from the prefill logits as DeviceSampler does.  Each round: with
    any penalty > 0, row (b, t) of the verify logits is penalised with response[b] + drafts[b][:t] (what the response would be if
    the drafts before t are accepted -- and row t only counts if they are) in one launch over the bs * T rows; then ONE
    speculative_verify call and ONE copy of its [bs, T + 1] result to the host.  If every top_k <= 1 the rows are greedy rows
    of the same kernel (accepted iff draft == argmax): generate_speculative_greedy's tokens.  A drafter with `draft` (ModelDrafter)
    takes _generate_speculative_sampled_drafted's rounds instead: sampled drafts, judged with their probabilities."""
    _check_draft_len(draft_len, max_q)
    n_req = len(prompts)
    req_ids = [f"gen{i}" for i in range(n_req)] if req_ids is None else list(req_ids)
    T = draft_len + 1
    ks = [1] * n_req if top_ks is None else [int(k) for k in (top_ks.tolist() if isinstance(top_ks, torch.Tensor) else top_ks)]
    if all(k <= 1 for k in ks):  # `is_all_greedy` (task.py:457), as in sample_tokens / DeviceSampler
        ks = [1] * n_req

    def as_list(v, default):
        return [default] * n_req if v is None else [float(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]

    temps, ps, pens = as_list(temperatures, 1.0), as_list(top_ps, 1.0), as_list(frequency_penalties, 0.0)
    assert len(ks) == len(temps) == len(ps) == len(pens) == n_req
    if hasattr(drafter, "draft"):  # a drafter that drafts on the device (ModelDrafter)
        return _generate_speculative_sampled_drafted(model, prompts, max_new_tokens, drafter, draft_len, temps, ks, ps, pens, generator,
                                                     req_ids, use_graph)
    penalise = any(p > 0 for p in pens)
    first = sample_tokens(model.prefill(prompts, req_ids), temps, ks, ps, generator=generator).tolist()
    out = [[t] for t in first]
    stats = {"steps": 0, "accepted": 0, "drafted": 0}
    live = list(range(n_req))
    if max_new_tokens <= 1:
        live = []
        for r in req_ids:
            model.cache.finalize_cache_all_decode(r)
    params_of = None  # the per-row parameters on the device, rebuilt when a request leaves the batch
    while live:
        drafts = _propose_drafts(drafter, prompts, out, live, draft_len)
        ids = [req_ids[i] for i in live]
        model.cache.prepare_block_table_for_decode_multi(ids, T)
        step = torch.tensor([[out[i][-1]] + d for i, d in zip(live, drafts)], dtype=torch.int64, device=model.device)
        logits = model.decode_multi(step, use_graph=use_graph).view(len(live) * T, -1)
        if penalise:
            apply_frequency_penalty(logits, [out[i] + d[:t] for i, d in zip(live, drafts) for t in range(T)],
                                    [pens[i] for i in live for _ in range(T)])
        if params_of != live:
            params_of = list(live)
            dev_params = [_per_row([v[i] for i in live for _ in range(T)], len(live) * T, dt, model.device)
                          for v, dt in ((temps, torch.float32), (ks, torch.int32), (ps, torch.float32))]
        res = speculative_verify(logits, [t for d in drafts for t in d + [-1]], T, *dev_params, generator=generator).tolist()
        kept = []
        for i, row in zip(live, res):
            out[i].extend(row[1 : 1 + row[0]])
            kept.append(row[0])
            stats["accepted"] += row[0] - 1
            stats["drafted"] += draft_len
        stats["steps"] += 1
        model.cache.finalize_cache_multi_decode(ids, kept)
        _retire_finished(model, req_ids, out, live, max_new_tokens)
    return _finish_speculative(model, out, stats, max_new_tokens)
