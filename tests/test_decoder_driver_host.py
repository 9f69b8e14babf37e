"""Host logic of chitu_amd.decoder.DecoderBase (no GPU): the per-key cache of captured steps behind decode and decode_multi, and the
round schedule of a chunked prefill.  A minimal subclass stands in for a family -- its decode_eager, prefill and prefill_continue
record their arguments -- and graphs.capture_verified is replaced by a stand-in; the control flow is the product's."""

import pytest
import torch

from chitu_amd import graphs
from chitu_amd.decoder import DecoderBase

VOCAB = 5


class _FakeGraph:
    def __init__(self, run_eager, static_out):
        self.run_eager, self.static_out, self.replays = run_eager, static_out, 0

    def replay(self):
        self.replays += 1
        self.static_out.copy_(self.run_eager())


class _Decoder(DecoderBase):
    multi_max_q = 4

    def __init__(self):
        super().__init__(None, None, None, "cpu")
        self.eager, self.prepared, self.checked, self.rounds = [], 0, [], []

    def decode_eager(self, tokens, q_len=1):
        self.eager.append((tokens.clone(), q_len))
        return tokens.float().unsqueeze(1) * torch.arange(1, VOCAB + 1, dtype=torch.float32)

    def prepare_decoding_attn(self):
        self.prepared += 1

    def check_step(self, kind, rows=0):
        self.checked.append((kind, rows))

    def _round(self, kind, tokens, req_ids):
        """Row b of the logits: (index of the round, the request, the last token it was given)."""
        self.rounds.append((kind, [list(t) for t in tokens], list(req_ids)))
        return torch.tensor([[len(self.rounds) - 1, r, t[-1]] for r, t in zip(req_ids, tokens)], dtype=torch.float32)

    def prefill(self, tokens, req_ids, chunk_size=None):
        if chunk_size is not None:
            return DecoderBase.prefill(self, tokens, req_ids, chunk_size)
        return self._round("prefill", tokens, req_ids)

    def prefill_continue(self, tokens, req_ids):
        return self._round("continue", tokens, req_ids)


@pytest.fixture
def captures(monkeypatch):
    """graphs.capture_verified -> a graph whose replay re-runs the eager step into the static output; one record per call."""
    made = []

    def fake_capture_verified(run_eager, static_out, mode, pool, what="decode step"):
        out = run_eager().clone() if static_out is None else static_out
        made.append({"what": what, "mode": mode, "pool": pool, "graph": _FakeGraph(run_eager, out)})
        return made[-1]["graph"], ("pool", 1) if pool is None else pool, out

    monkeypatch.setattr(graphs, "capture_verified", fake_capture_verified)
    return made


def _logits(tokens):
    return tokens.float().reshape(-1, 1) * torch.arange(1, VOCAB + 1, dtype=torch.float32)


def test_single_step_is_captured_once_per_batch_size_and_mode(captures):
    m = _Decoder()
    a, b = torch.tensor([3, 4]), torch.tensor([7, 9])
    out = m.decode(a)
    assert torch.equal(out, _logits(a)) and len(captures) == 1
    assert captures[0]["what"] == "_Decoder decode step bs=2" and captures[0]["mode"] == "full" and captures[0]["pool"] is None
    assert list(m.graphs) == [(2, "full")] and list(m.static_tokens) == [2] and list(m.static_out) == [2]
    assert m.graph_pool == ("pool", 1) and out is m.static_out[2]
    buf, g = m.static_tokens[2], m.graphs[(2, "full")]
    assert buf is not a and g.replays == 1
    # the second call at the key: a copy into the same static buffer and a replay, no capture
    out = m.decode(b)
    assert len(captures) == 1 and m.static_tokens[2] is buf and torch.equal(buf, b) and g.replays == 2
    assert out is m.static_out[2] and torch.equal(out, _logits(b))
    # another batch size and another mode are captures of their own; the mode shares the batch size's static buffers
    m.decode(torch.tensor([1, 2, 3]))
    m.decode(a, use_graph="piecewise")
    assert [c["what"] for c in captures[1:]] == ["_Decoder decode step bs=3", "_Decoder decode step bs=2"]
    assert [c["mode"] for c in captures[1:]] == ["full", "piecewise"] and all(c["pool"] == ("pool", 1) for c in captures[1:])
    assert set(m.graphs) == {(2, "full"), (3, "full"), (2, "piecewise")} and set(m.static_tokens) == {2, 3} == set(m.static_out)
    assert m.static_tokens[2] is buf and torch.equal(buf, a)
    assert m.prepared == 4 and not m.checked


def test_multi_step_is_captured_once_per_batch_size_T_and_mode(captures):
    m = _Decoder()
    a, b = torch.tensor([[3, 4, 5], [6, 7, 8]]), torch.tensor([[1, 2, 3], [9, 9, 9]])
    out = m.decode_multi(a)
    assert len(captures) == 1 and captures[0]["what"] == "_Decoder multi-token decode step bs=2 T=3" and captures[0]["mode"] == "full"
    assert list(m.graphs) == [(2, 3, "full")] and list(m.static_tokens) == [(2, 3)] and list(m.static_out) == [(2, 3)]
    # a [bs, T, vocab] view of the static output; the stack saw bs * T rows and T
    assert out.shape == (2, 3, VOCAB) and out.data_ptr() == m.static_out[(2, 3)].data_ptr() and m.static_out[(2, 3)].shape == (6, VOCAB)
    assert torch.equal(out, _logits(a).view(2, 3, VOCAB))
    assert all(q == 3 and t.shape == (6,) for t, q in m.eager)
    buf = m.static_tokens[(2, 3)]
    out = m.decode_multi(b)
    assert len(captures) == 1 and m.static_tokens[(2, 3)] is buf and torch.equal(buf, b.reshape(6))
    assert m.graphs[(2, 3, "full")].replays == 2 and torch.equal(out, _logits(b).view(2, 3, VOCAB))
    m.decode_multi(a[:, :2])
    m.decode(a[:, 0])  # the single step at the same batch size: keys of its own
    assert set(m.graphs) == {(2, 3, "full"), (2, 2, "full"), (2, "full")} and set(m.static_tokens) == {(2, 3), (2, 2), 2}
    # the rows reach check_step; only the single-token step prepares the attention metadata
    assert m.checked == [("multi-token decode", 6), ("multi-token decode", 6), ("multi-token decode", 4)] and m.prepared == 1


def test_without_a_graph_nothing_is_captured(captures):
    m = _Decoder()
    a = torch.tensor([[3, 4], [6, 7]])
    assert torch.equal(m.decode(a[:, 0], use_graph=False), _logits(a[:, 0]))
    out = m.decode_multi(a, use_graph=False)
    assert out.shape == (2, 2, VOCAB) and torch.equal(out, _logits(a).view(2, 2, VOCAB))
    assert not captures and not m.graphs and not m.static_tokens and not m.static_out and m.graph_pool is None
    assert [q for _, q in m.eager] == [1, 2]


@pytest.mark.parametrize("T", [1, _Decoder.multi_max_q + 1])
@pytest.mark.parametrize("use_graph", [True, False])
def test_multi_step_refuses_T_outside_its_range_before_anything_runs(captures, T, use_graph):
    m = _Decoder()
    with pytest.raises(ValueError):
        m.decode_multi(torch.zeros(2, T, dtype=torch.int64), use_graph=use_graph)
    assert not m.eager and not captures and not m.graphs and not m.static_tokens
    m.decode_multi(torch.zeros(2, _Decoder.multi_max_q, dtype=torch.int64), use_graph=use_graph)  # the largest T runs
    assert len(m.eager) >= 1


def test_chunked_prefill_runs_every_prompt_in_rounds_of_chunk_size():
    m = _Decoder()
    prompts = [[10], [20, 21, 22, 23, 24], [30, 31, 32, 33, 34, 35, 36, 37, 38]]
    logits = m.prefill(prompts, [0, 1, 2], chunk_size=4)
    assert m.rounds == [
        ("prefill", [[10], [20, 21, 22, 23], [30, 31, 32, 33]], [0, 1, 2]),
        ("continue", [[24], [34, 35, 36, 37]], [1, 2]),
        ("continue", [[38]], [2]),
    ]
    # each request's row is the one of the last round it took part in
    assert logits.tolist() == [[0.0, 0.0, 10.0], [1.0, 1.0, 24.0], [2.0, 2.0, 38.0]]
    assert m.checked == [("chunked prefill", 0)]


def test_chunk_size_below_one_is_refused_before_anything_is_called():
    m = _Decoder()
    for c in (0, -3):
        with pytest.raises(ValueError):
            m.prefill([[1, 2, 3]], [0], chunk_size=c)
    assert not m.rounds and not m.checked
