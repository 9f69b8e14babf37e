"""What every decoder here means by a step: ragged, chunked and continued prefill, the single- and the multi-token decode step
with their hipGraph cache, generate and the speculative loops -- written once, for LlamaDecoder (and the families built on it) and
DeepSeekV3Decoder (reference: chitu/models/model.py -- prefill_single_device:451-465, decode_single_device:468-475,
Transformer.decode:538-622).

A family supplies its constructor (embed_weight, layers, norm, head_weight, cos_table / sin_table, vocab_local / vocab_start) and
what DecoderBase names as its differences: final_norm(), multi_max_q, prepare_decoding_attn(), prepare_continue_attn() and
check_step().
"""

import torch
import torch.nn.functional as F

from . import graphs, ops, sampling
from . import tensor_parallel as tp


class VarLens:
    """Ragged-batch bookkeeping of a prefill call (chitu/utils.py:84-101): same fields."""

    def __init__(self, tokens, device) -> None:
        self.cpu_lens = [len(t) for t in tokens]
        self.cpu_prefix_lens = [0]
        for n in self.cpu_lens:
            self.cpu_prefix_lens.append(self.cpu_prefix_lens[-1] + n)
        self.lens = torch.tensor(self.cpu_lens, device=device, dtype=torch.int32)
        self.prefix_lens = torch.tensor(self.cpu_prefix_lens, device=device, dtype=torch.int32)
        self.max_len = max(self.cpu_lens)
        self.total_len = self.cpu_prefix_lens[-1]
        self.position_ids = torch.cat([torch.arange(n) for n in self.cpu_lens]).to(device)


class DecoderBase(torch.nn.Module):
    """embed -> blocks -> norm -> head -> fp32 logits, with the decode step captured as a hipGraph per batch size."""

    multi_max_q = None  # tokens per sequence of the family's multi-token attention (attn_backend.*_MULTI_MAX_Q)

    def __init__(self, args, cache, attn_backend, device):
        super().__init__()
        self.args, self.cache, self.attn_backend, self.device = args, cache, attn_backend, torch.device(device)
        # the captured steps: graphs[(bs, mode)] / [(bs, T, mode)], their static buffers under bs / (bs, T)
        self.graphs, self.static_tokens, self.static_out = {}, {}, {}
        self.graph_pool = None

    # ------------------------------------------------------------------ what a family states
    def final_norm(self):
        """(weight, eps) of the norm in front of the head."""
        raise NotImplementedError

    def prepare_decoding_attn(self):
        """What the attention backend needs before a single-token step, outside the graph: nothing, unless a family says so."""

    def prepare_continue_attn(self, varlens, req_ids):
        """What the family's continued-prefill attention reads from varlens beyond VarLens's own fields
        (cache.prepare_cache_prefill_continue has run): nothing, unless a family says so."""

    def check_step(self, kind, rows=0):
        """Raise for a step this family does not run, before a launch and before cache state changes.  kind: "chunked prefill" |
        "continued prefill" | "multi-token decode" (rows = batch * tokens per sequence)."""

    # ------------------------------------------------------------------ the stack
    def embed(self, tokens):
        """tensor_parallel.py:199-208: mask ids outside this rank's vocab slice, lookup, all-reduce."""
        if self.vocab_local == self.args.vocab_size:
            return F.embedding(tokens, self.embed_weight)
        local = tokens - self.vocab_start
        mask = (local < 0) | (local >= self.vocab_local)
        y = F.embedding(torch.where(mask, torch.zeros_like(local), local), self.embed_weight)
        return tp.all_reduce(torch.where(mask.unsqueeze(-1), torch.zeros_like(y), y))

    def _head(self, h, pending):
        """The final norm (+ the last residual add) and the head; bf16 logits -> fp32 (model.py:475), the cast riding in the gather."""
        h = tp.add_norm(h, pending, *self.final_norm())[1]
        return tp.all_gather_last_dim(ops.bf16_linear(h, self.head_weight), out_dtype=torch.float32)

    def decode_eager(self, tokens, q_len=1):
        """tokens [rows] int64 -> logits [rows, vocab] fp32 (decode_single_device, model.py:468-475).  q_len > 1: rows = q_len
        consecutive tokens of each sequence, positions and page rows from the cache manager's multi-token buffers."""
        # embedding rows of this rank's vocabulary slice + every row's rotary row (prepare_freqs_cis_decode,
        # model.py:429-448): one launch
        positions = self.cache.get_gpu_multi_row_lens() if q_len > 1 else self.cache.get_gpu_seq_lens_excl_this_decode()
        h, cos, sin = ops.embed_rope_gather(tokens, self.embed_weight, self.vocab_start if self.vocab_local != self.args.vocab_size else 0,
                                            positions, self.cos_table, self.sin_table)
        if self.vocab_local != self.args.vocab_size:
            h = tp.all_reduce(h)  # tensor_parallel.py:199-208
        pending = None
        for layer in self.layers:
            h, pending = layer(h, pending, cos, sin, q_len=q_len)
        return self._head(h, pending)

    def _prefill_stack(self, tokens, varlens, position_ids):
        """Ragged rows through every layer -> fp32 logits [n_req, vocab] of each sequence's last row.  Eager launches."""
        flat = torch.tensor([t for seq in tokens for t in seq], dtype=torch.int64, device=self.device)
        cos, sin = self.cos_table[position_ids], self.sin_table[position_ids]
        h, pending = self.embed(flat), None
        for layer in self.layers:
            h, pending = layer(h, pending, cos, sin, varlens)
        last = torch.tensor([p - 1 for p in varlens.cpu_prefix_lens[1:]], dtype=torch.int64, device=self.device)
        h, pending = h[last], tp.resolve(pending)
        if pending is not None:
            pending = pending[last].contiguous()
        return self._head(h, pending)

    # ------------------------------------------------------------------ prefill
    @torch.inference_mode()
    def prefill(self, tokens, req_ids, chunk_size=None):
        """tokens: list of per-request token-id lists; req_ids: their cache keys.  Runs the prompts through every layer, fills
        the KV pages, returns fp32 logits [n_req, vocab] of each prompt's LAST token (prefill_single_device, model.py:451-465).
        chunk_size = c: the first c tokens of every prompt run here, the rest in rounds of prefill_continue with at most c tokens
        per request (a request whose prompt is exhausted leaves the later rounds), so no round holds more than n_req * c rows."""
        if chunk_size is not None:
            c = int(chunk_size)
            if c < 1:
                raise ValueError(f"chunk_size={chunk_size}: at least one token per round")
            self.check_step("chunked prefill")
            req_ids = list(req_ids)
            logits = self.prefill([list(t[:c]) for t in tokens], req_ids)
            done = c
            while True:
                live = [i for i, t in enumerate(tokens) if len(t) > done]
                if not live:
                    return logits
                out = self.prefill_continue([list(tokens[i][done : done + c]) for i in live], [req_ids[i] for i in live])
                logits[torch.tensor(live, device=logits.device)] = out  # a later round overwrites it until the prompt ends
                done += c

        graphs.sweep_if_memory_was_recycled()  # the eager path's canary: once after an xGMI communicator came or went
        varlens = VarLens(tokens, self.device)
        self.cache.curr_varlens, self.cache.curr_req_ids = varlens, list(req_ids)
        logits = self._prefill_stack(tokens, varlens, varlens.position_ids)
        self.cache.finalize_cache_all_prefill(req_ids, varlens)
        return logits

    @torch.inference_mode()
    def prefill_continue(self, tokens, req_ids):
        """Ragged chunks of new tokens for requests that are already cached (a conversation's next turn, the next chunk of a
        long prompt, a draft model's catch-up) -> fp32 logits [n_req, vocab] of each chunk's last token; appends their KV
        rows.  Positions, and so cos / sin, continue from each request's cached length.  The attention reads the pages (the
        family's prefill_forward_paged); everything else is prefill's stack on the new rows, tensor- and expert-parallel paths
        included.  An unknown request, a chunk that overruns the rotary table or the block table, too few free pages, or a
        cache format the family's paged prefill does not read (check_step) raises before any cache state changes."""
        self.check_step("continued prefill")
        req_ids = list(req_ids)
        assert len(tokens) == len(req_ids) and all(len(t) >= 1 for t in tokens)
        for r, t in zip(req_ids, tokens):
            if r not in self.cache.seq_lens:
                raise KeyError(f"request {r!r} is not cached: a continued prefill extends a sequence that prefill registered")
            assert self.cache.seq_lens[r] + len(t) <= self.cos_table.shape[0], \
                f"request {r!r}: {self.cache.seq_lens[r]} + {len(t)} tokens exceed max_position_embeddings={self.cos_table.shape[0]}"
        graphs.sweep_if_memory_was_recycled()
        varlens = VarLens(tokens, self.device)
        varlens.continued = True
        self.cache.prepare_cache_prefill_continue(req_ids, varlens)
        self.prepare_continue_attn(varlens, req_ids)
        logits = self._prefill_stack(tokens, varlens, self.cache.get_continue_position_ids())
        self.cache.finalize_cache_all_prefill_continue(req_ids)
        return logits

    # ------------------------------------------------------------------ decode
    def _step(self, tokens, q_len, use_graph):
        """decode_eager(tokens, q_len), or the replay of that step captured per (batch size[, q_len], mode) on static buffers
        of its own."""
        if not use_graph or tp.xgmi_split_phase():  # (split-phase collectives hold a host barrier: not capturable)
            return self.decode_eager(tokens, q_len)
        bs = tokens.shape[0] // q_len
        mode = graphs.graph_mode(use_graph)
        if q_len == 1:
            key, skey, what = (bs, mode), bs, f"decode step bs={bs}"
        else:
            key, skey, what = (bs, q_len, mode), (bs, q_len), f"multi-token decode step bs={bs} T={q_len}"
        if skey not in self.static_tokens:
            self.static_tokens[skey] = tokens.clone()
        else:
            self.static_tokens[skey].copy_(tokens)
        if key not in self.graphs:
            # Eager step on the static inputs (it replicates the graph's side effect, the append at position L, which the
            # replays then overwrite with the same values), capture, ONE replay checked bit for bit against that eager
            # step (graphs.capture_verified): a graph that does not reproduce the eager launches is never used.
            g, self.graph_pool, self.static_out[skey] = graphs.capture_verified(
                lambda: self.decode_eager(self.static_tokens[skey], q_len), self.static_out.get(skey), mode, self.graph_pool,
                what=f"{type(self).__name__} {what}")
            self.graphs[key] = g
        self.graphs[key].replay()
        return self.static_out[skey]

    @torch.inference_mode()
    def decode(self, tokens, use_graph=True):
        """One decode step -> fp32 logits [bs, vocab].  use_graph: False = eager launches; True = replay of
        the step captured per batch size -- as ONE hipGraph when this rank has no collectives (or when
        CHITU_TP_GRAPH=full asks for the collectives to be captured too), else PIECEWISE: the step is cut at
        every all-reduce / all-gather, the pieces are hipGraphs and the collectives are issued between them
        (RCCL never has to be capturable; 2 x layers + 2 host calls per step, far below the pieces' GPU
        time); "piecewise" / "full" force a mode."""
        tp.check_comm()  # a collective of an earlier step that timed out: raise instead of decoding garbage
        self.prepare_decoding_attn()
        return self._step(tokens, 1, use_graph)

    @torch.inference_mode()
    def decode_multi(self, tokens, use_graph=True):
        """One step over T = tokens.shape[1] tokens per sequence (1 < T <= multi_max_q): tokens [bs, T] int64 are appended at
        each sequence's length .. + T - 1 and token t attends to everything up to itself -- the verify step of speculative
        decoding.  Returns fp32 logits [bs, T, vocab]: row (b, t) predicts the token after tokens[b, t].  The caller has run
        cache.prepare_block_table_for_decode_multi(req_ids, T) and settles the lengths with finalize_cache_multi_decode.

        The stack runs on bs * T rows (embedding, norms, GEMMs and the RoPE + append launch take per-row positions; the fused
        small-batch launches apply by their row limits on bs * T); only the attention call knows T.  Graph replay as in decode(),
        keyed (bs, T, mode), on static buffers of its own."""
        tp.check_comm()
        assert tokens.dim() == 2 and tokens.dtype == torch.int64
        bs, T = tokens.shape
        if T == 1:
            raise ValueError("decode_multi is the multi-token step (T > 1); decode() is the single-token one")
        if T > self.multi_max_q:
            raise ValueError(f"decode_multi: {T} tokens per sequence; 2 .. {self.multi_max_q} are implemented")
        self.check_step("multi-token decode", bs * T)
        return self._step(tokens.reshape(bs * T), T, use_graph).view(bs, T, -1)

    # ------------------------------------------------------------------ generation
    @torch.inference_mode()
    def generate(self, prompts, max_new_tokens, req_ids=None, use_graph=True, temperatures=None, top_ks=None,
                 top_ps=None, frequency_penalties=None, generator=None, prefill_chunk_size=None):
        """Prefill (prefill_chunk_size: in chunks, prefill's chunk_size), then max_new_tokens - 1 decode steps; returns
        [n_req, max_new_tokens] int64 and frees the requests' pages.  Token selection is executor.py:82-112 on the device
        (chitu_amd.sampling): greedy unless some top_k > 1 (then per-request temperature / top-k / top-p sampling, uniforms from
        `generator`), with an optional per-request frequency penalty; tokens never visit the host."""
        req_ids = [f"gen{i}" for i in range(len(prompts))] if req_ids is None else list(req_ids)
        pick = sampling.DeviceSampler(len(prompts), max_new_tokens, self.device, temperatures, top_ks, top_ps,
                                      frequency_penalties, generator)
        tok = pick(self.prefill(prompts, req_ids) if prefill_chunk_size is None else
                   self.prefill(prompts, req_ids, chunk_size=prefill_chunk_size))
        out = [tok]
        for _ in range(max_new_tokens - 1):
            self.cache.prepare_cache_decode(req_ids)
            self.cache.prepare_block_table_for_decode(req_ids)
            tok = pick(self.decode(tok, use_graph=use_graph))
            self.cache.finalize_cache_single_decode(req_ids)
            out.append(tok)
        for r in req_ids:
            self.cache.finalize_cache_all_decode(r)
        tokens_out = torch.stack(out, dim=1)
        if tp.xgmi_comm() is not None:
            # the tokens are about to leave the engine: make sure no collective behind them gave up on a peer
            torch.cuda.current_stream().synchronize()
            tp.check_comm()
        return tokens_out

    @torch.inference_mode()
    def generate_speculative(self, prompts, max_new_tokens, drafter, draft_len, req_ids=None, use_graph=True, temperatures=None,
                             top_ks=None, top_ps=None, frequency_penalties=None, generator=None):
        """Greedy generation with draft-and-verify: the tokens plain greedy generate() picks, in fewer steps when the drafter is
        right.  Each round, drafter.propose(history, draft_len) names draft_len tokens per request (history = prompt + tokens
        so far; chitu_amd.sampling.NgramDrafter is such a drafter, a DeepSeek-V3 checkpoint's multi-token-prediction head
        another), ONE decode_multi step runs over [last token | drafts], the longest prefix with draft[i] == argmax(logits[i]) is
        accepted, the argmax at the first mismatch (or after the last draft) is emitted as the bonus token, and the cache
        keeps accepted + 1 rows.  A request leaves the batch when it has max_new_tokens.  Returns [n_req, max_new_tokens] int64
        and frees the requests' pages; self.speculative_stats = {"steps": verify steps run, "accepted": drafts accepted,
        "drafted": drafts proposed}.  Greedy only: any sampling argument raises (generate_speculative_sampled takes them).  The
        drafter runs on the host: the accepted counts have to reach the host for the page accounting anyway (one small copy
        per round).  Every request needs room for draft_len tokens beyond prompt + max_new_tokens in its block table.
        draft_len outside 1 .. multi_max_q - 1 raises."""
        return sampling.generate_speculative_greedy(self, prompts, max_new_tokens, drafter, draft_len, self.multi_max_q, req_ids,
                                                    use_graph, (temperatures, top_ks, top_ps, frequency_penalties, generator))

    @torch.inference_mode()
    def generate_speculative_sampled(self, prompts, max_new_tokens, drafter, draft_len, temperatures=None, top_ks=None, top_ps=None,
                                     frequency_penalties=None, generator=None, req_ids=None, use_graph=True):
        """generate_speculative's draft-and-verify loop with generate()'s sampling parameters (per request: temperature, top_k,
        top_p, frequency penalty; `generator`: a CUDA torch.Generator for the uniforms).  The first token is sampled from the
        prefill logits.  Each round ONE decode_multi step runs over [last token | drafts] and ONE chitu_hip_speculative_verify
        call judges the drafts on the device: under the distribution p that generate()'s sampler draws from for the row, a
        draft d is accepted with probability p(d); the first rejected draft is replaced by a draw from p without d,
        renormalised; after draft_len accepted drafts a bonus token is drawn from p.  The frequency penalty of row t counts the
        response so far and the round's drafts before t.

        A drafter with propose(history, draft_len) names tokens: a deterministic proposal, and the rule above is rejection
        sampling against a point mass.  A sampling.ModelDrafter drafts on the device with a draft model (e.g. a shallow stack of
        this decoder) and, with sample=True, draws each draft from the draft model's distribution q under the request's own
        temperature / top_k / top_p (without the frequency penalty) and hands over its logits: ONE
        chitu_hip_speculative_verify_sampled call accepts d with min(1, p(d) / q(d)) and replaces a rejected draft by a draw from
        max(p - q, 0), renormalised -- lossless for any q, provided q is what d was drawn from.  The output tokens are
        distributed as generate()'s with the same parameters, but they come from another uniform stream: the same generator seed
        does not give generate()'s tokens.  With every top_k <= 1 the result is generate_speculative's.

        Returns [n_req, max_new_tokens] int64, frees the requests' pages, leaves self.speculative_stats as generate_speculative
        does.  draft_len outside 1 .. multi_max_q - 1 raises."""
        return sampling.generate_speculative_sampled(self, prompts, max_new_tokens, drafter, draft_len, self.multi_max_q, temperatures,
                                                     top_ks, top_ps, frequency_penalties, generator, req_ids, use_graph)
