"""CPU checks of tests/route_exact.py: the safe sigmoid table, every builder through the torch oracles, the reference
mutations, and the proof that the GPU case list reaches every routing kernel and every way into the sort.

Which case catches which reference mutation (asserted in test_reference_mutations_change_the_named_expectations; "every
shape" = the R1 router, 3 groups of 64, 5 and 3 groups of 32, 4 groups of 4):
  higher index wins             <shape>-group_tie_at_cut-bias / -nobias (the other tied group), <E>-topk_ties
  group max, not top-2 sum      <shape>-group_max_twice (0.8 + 0.55 overtakes 0.7 + 0.7)
  mask to -inf, not x 0         <shape>-negative_vs_masked_zero, <shape>-unmasked_zero_vs_masked_zero
  one plane dropped             every case with planes (74)
  the last plane doubled        every plane-sweep case planes-<form>-S<n> (and 71 of the 74 in all)
  sum rounded per plane         planes-<form>-S<n> for every form at S = 15 or 16
  plane sum not rounded to bf16 planes-<form>-S<n> for every form at two S or more
  no renormalisation            soft-mixtral-rand, soft-e160-rand and every other softmax_renorm case (12)
"""

import numpy as np
import pytest
import torch

from oracle import deepseek as ods
from oracle import mixtral as omx
from tests import route_exact as rx

CASES = rx.gpu_cases()
BY_NAME = {c.name: c for c in CASES}
GROUPED = ("r1", "e192_g64", "e160_g32", "e96_g32", "e16_g4")


def _bf16(values32):
    return torch.from_numpy(rx.bf16_bits(values32).view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------- the table
def test_safe_sigmoid_table():
    x, s, normal, safe = rx.sigmoid_table()
    assert int(normal.sum()) == 49711 and int(safe.sum()) == 49678
    near = safe & (np.abs(x) <= 16)
    assert len(np.unique(rx.r64(s[near]))) == 751
    # torch's bf16 sigmoid on the safe set = the float64 value rounded once
    pat = np.nonzero(safe)[0].astype(np.uint16)
    got = _bits(torch.from_numpy(pat.view(np.int16).copy()).view(torch.bfloat16).sigmoid())
    assert np.array_equal(got, rx.bf16_bits(rx.r64(s[safe]).astype(np.float32)))
    sc, xs = rx.levels()
    assert len(sc) > 500 and (np.diff(sc) > 0).all() and sc[-1] == 1.0
    assert np.array_equal(rx.bf16_bits(sc), _bits(_bf16(xs).sigmoid()))


def test_rounding_helpers_agree_with_torch():
    rng = np.random.default_rng(1)
    v = (rng.standard_normal(20000) * np.exp(rng.uniform(-20, 20, 20000))).astype(np.float32)
    assert np.array_equal(rx.bf16_bits(v), _bits(torch.from_numpy(v).to(torch.bfloat16)))
    v64 = v.astype(np.float64)
    assert np.array_equal(rx.r64(v64), rx.r32(v).astype(np.float64))
    mid = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.75 + 2.0 ** -9])  # ties go to even
    assert rx.r64(mid).tolist() == [1.0, 1.0 + 2.0 ** -6, 0.75] and (rx.midpoint_distance(mid) == 0).all()


# ---------------------------------------------------------------- every case through the torch oracles
def _torch_route(c, d):
    """(weights bits [M, topk], ids, torch's kept groups or None, torch's bf16/fp32 group scores or None)."""
    logits = _bf16(d["logit"])
    bias = _bf16(d["bias"]) if d["bias"] is not None else None
    if c.score == rx.RENORM:
        assert c.G == 1 and bias is None and c.scale == 1.0
        w, ids = omx.route(logits, torch.eye(c.E, dtype=torch.bfloat16), c.topk)  # F.linear with the identity: the logits
        return _bits(w), ids.numpy(), None, None
    w, ids, mid = ods.gate_from_logits(logits, bias, c.G, c.Kg, c.topk, c.score, c.scale, return_masked=True)
    kept = mid["group_scores"].topk(c.Kg, dim=-1)[1].numpy() if c.G > 1 else None
    return _bits(w), ids.numpy(), kept, (mid["group_scores"].double().numpy() if c.G > 1 else None)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_against_the_torch_oracle(case):
    c, d = case, rx.build(case)
    sp = d["spec"]
    if c.S:
        assert np.array_equal(rx.sum_planes(d["planes"], c.S), d["logit"]) and np.isnan(d["planes"][c.S:]).all()
    w_t, ids_t, kept_t, gs_t = _torch_route(c, d)
    if c.G > 1:
        if c.score == rx.SIGMOID:
            assert np.array_equal(gs_t, sp["gscore"].astype(np.float64))  # bf16 group scores, bit for bit
        else:
            assert np.allclose(gs_t, sp["gscore"], rtol=1e-5, atol=0)
        if sp["group_tie"].any():
            # torch.topk's choice among tied groups is unspecified: it must be A valid top-Kg, and the rest is followed with it
            g = sp["gscore"]
            for t in range(c.M):
                out = np.setdiff1d(np.arange(c.G), kept_t[t])
                assert g[t, kept_t[t]].min() >= g[t, out].max()
            sp = rx.spec(c, d["logit"], d["bias"], keep_groups=kept_t)
        else:
            assert np.array_equal(np.sort(kept_t, axis=1), np.sort(sp["kept"], axis=1))
    masked = sp["masked"]
    for t in range(c.M):
        mine, theirs = sp["ids"][t], ids_t[t]
        assert len(set(theirs.tolist())) == c.topk
        if sp["cut_tie"][t]:
            out = np.setdiff1d(np.arange(c.E), theirs)
            assert masked[t, theirs].min() >= masked[t, out].max(), (c.name, t)  # still a valid top-k
        else:
            assert set(mine.tolist()) == set(theirs.tolist()), (c.name, t)
            if len(np.unique(masked[t, mine])) == c.topk:
                assert mine.tolist() == theirs.tolist(), (c.name, t)
        if set(mine.tolist()) != set(theirs.tolist()):
            continue
        col = [theirs.tolist().index(e) for e in mine.tolist()]  # weights are compared expert by expert
        if c.score == rx.SIGMOID:
            assert np.array_equal(w_t[t, col], sp["w_bits"][t]), (c.name, t)
        else:
            ok, _ = rx.softmax_weight_ok(sp["w64"][t], w_t[t, col])
            assert ok.all(), (c.name, t)
    if c.score != rx.SIGMOID:
        assert d["spec"]["strict_share"] >= 0.95


def test_named_edges_are_what_their_names_say():
    for shape in GROUPED:
        for b in ("bias", "nobias"):
            c = BY_NAME[f"{shape}-group_tie_at_cut-{b}"]
            sp = rx.build(c)["spec"]
            a, bgrp, _, _ = rx._group_roles(c)
            assert sp["group_tie"].all() and (sp["kept"] == a).any(axis=1).all() and not (sp["kept"] == bgrp).any()
            assert ((sp["ids"] // c.gs) == a).sum(axis=1).min() == 2  # both of a's top experts are routed to
        c = BY_NAME[f"{shape}-group_max_twice"]
        sp = rx.build(c)["spec"]
        a, bgrp, _, _ = rx._group_roles(c)
        top2 = np.sort(sp["sel"].reshape(c.M, c.G, -1), axis=-1)[:, bgrp, -2:]
        assert (top2[:, 0] == top2[:, 1]).all() and (sp["kept"] == bgrp).any(axis=1).all() and not (sp["kept"] == a).any()
        for kind in ("negative_vs_masked_zero", "unmasked_zero_vs_masked_zero"):
            c = BY_NAME[f"{shape}-{kind}"]
            sp = rx.build(c)["spec"]
            assert (sp["ids"][:, c.Kg:] == np.arange(c.Kg)).all()  # the masked zeros of group 0, lowest index first
            unmasked_rest = sp["masked"][:, (c.G - c.Kg) * c.gs:]
            if kind.startswith("negative"):
                assert ((unmasked_rest < 0).sum(axis=1) == c.Kg * (c.gs - 1)).all()
            else:
                z = unmasked_rest == 0
                assert (z.sum(axis=1) == c.Kg * (c.gs - 1)).all() and not np.signbit(unmasked_rest[z]).any()
    for name in ("e256", "e128", "e72", "e64", "e10", "e8", "e1024"):
        c = BY_NAME[f"{name}-topk_ties"]
        d = rx.build(c)
        sp = d["spec"]
        assert (sp["orig"][-2] == sp["orig"][-2, 0]).all() and sp["ids"][-2].tolist() == list(range(c.topk))  # all equal
        assert (sp["orig"][-1] == 1.0).sum() >= c.E // 2  # saturated
        if c.M == 5:
            assert sp["cut_tie"][:2].all() and not sp["cut_tie"][2]
            m = sp["masked"][2, sp["ids"][2]]
            assert len(np.unique(m)) == c.topk - 2  # two equal pairs among the selected, positions far apart
            if c.E > 64:  # 63 | 64: the tie spans two waves of the fast kernel's pre-selection, and the cut falls inside it
                tied = np.nonzero(sp["masked"][1] == sp["masked"][1, 63])[0]
                assert {63, 64} <= set(tied.tolist()) and len(tied) == 4 and sp["ids"][1, -2:].tolist() == [1, 63]


# ---------------------------------------------------------------- reference mutations
def _expectation_changes(c, mut):
    d = rx.build(c)
    sp = d["spec"]
    logit = rx.sum_planes(d["planes"], c.S, (mut,)) if c.S else d["logit"]
    m = rx.spec(c, logit, d["bias"], (mut,))
    if not np.array_equal(m["ids"], sp["ids"]):
        return True
    if c.score == rx.SIGMOID:
        return not np.array_equal(m["w_bits"], sp["w_bits"])
    return not rx.softmax_weight_ok(sp["w64"], rx.bf16_bits(m["w64"].astype(np.float32)))[0].all()


def _plane_cases(S_values):
    return [f"planes-{form}-S{S}" for form in rx.FORMS for S in S_values]


MUTATION_CATCHERS = {
    "higher_index": [f"{s}-group_tie_at_cut-{b}" for s in GROUPED for b in ("bias", "nobias")]
                    + [f"{e}-topk_ties" for e in ("e256", "e128", "e72", "e64", "e10", "e1024")],
    "group_max": [f"{s}-group_max_twice" for s in GROUPED],
    "mask_neginf": [f"{s}-{k}" for s in GROUPED for k in ("negative_vs_masked_zero", "unmasked_zero_vs_masked_zero")],
    "drop_plane": [c.name for c in CASES if c.S],
    "double_last": _plane_cases([S for S in rx.PLANES if S]),
    "round_per_plane": None,   # per form, below
    "no_sum_round": None,      # per form, below
    "no_renorm": [c.name for c in CASES if c.score == rx.RENORM],
}


@pytest.mark.parametrize("mut", list(MUTATION_CATCHERS))
def test_reference_mutations_change_the_named_expectations(mut):
    names = MUTATION_CATCHERS[mut]
    if names is not None:
        assert names
        missed = [n for n in names if not _expectation_changes(BY_NAME[n], mut)]
        assert not missed, (mut, missed)
        return
    for form in rx.FORMS:
        caught = [S for S in rx.PLANES if S and _expectation_changes(BY_NAME[f"planes-{form}-S{S}"], mut)]
        if mut == "round_per_plane":
            assert 15 in caught or 16 in caught, (mut, form, caught)
        else:
            assert len(caught) >= 2, (mut, form, caught)


# ---------------------------------------------------------------- coverage, from the dispatch mirror
def test_the_gpu_cases_reach_every_kernel_and_every_sort():
    reached = {}
    for c in CASES:
        for v in rx.variants(c):
            reached.setdefault(rx.dispatch(c, **rx.VARIANTS[v]), []).append((c, v))
    kernels = {k for k, _ in reached}
    assert kernels == {"gate_route_kernel<0>", "gate_route_kernel<1>", "gate_route_fast_kernel<0>", "gate_route_fast_kernel<32>",
                       "gate_route_fast_kernel<64>", "gate_route_align_wg_kernel<0>", "gate_route_align_wg_kernel<32>",
                       "gate_route_align_wg_softmax_kernel"}
    sorts = {s for _, s in reached}
    assert sorts == {"none", "bs1_tail", "ticket", "wg_general", "wg_small"}
    for k in kernels:  # every kernel with and without the sort; the per-token kernels through both tails
        assert any(kk == k and s != "none" for kk, s in reached), k
        if "align_wg" in k:
            assert (k, "wg_small") in reached and (k, "wg_general") in reached, k
        else:
            assert (k, "none") in reached and (k, "ticket") in reached and (k, "bs1_tail") in reached, k
    declined = [c.name for c in CASES if rx.small_declined(c)]
    assert any("extra_inside_routed" in n for n in declined) and any("extra_past_table" in n for n in declined)
    assert any("v2lite" in n for n in declined)  # the softmax one-workgroup kernel's fall-back too
    # every instantiation sums planes at every count of the sweep, the one-workgroup forms at 1, 2, 15 and 16 tokens
    for S in rx.PLANES:
        assert {rx.dispatch(c)[0] for c in CASES if c.S == S and c.name.startswith("planes-")} == kernels, S
    assert {c.S for c in CASES if rx.dispatch(c)[0].startswith("gate_route_kernel")} >= {17, 24}
    for k in kernels:
        if "align_wg" in k:
            assert {c.M for c in CASES if rx.dispatch(c)[0] == k} >= {1, 2, 15, 16}, k
    assert {c.M for c in CASES if rx.dispatch(c)[1] == "ticket"} >= {17, 40, 300}
    assert {c.block for c in CASES if c.alE} == {16, 64} and any(c.ep for c in CASES) and any(c.alE and not c.ep for c in CASES)


def test_dispatch_mirror_on_the_documented_shapes():
    C = rx.Case
    assert rx.dispatch(C("a", "rand", **rx.R1, bias=True))[0] == "gate_route_fast_kernel<32>"
    assert rx.dispatch(C("a", "rand", **rx.R1, bias=True), generic=1)[0] == "gate_route_kernel<1>"
    assert rx.dispatch(C("a", "rand", E=64, topk=6))[0] == "gate_route_kernel<1>"  # 6 % 4 != 0
    assert rx.dispatch(C("a", "rand", E=128, topk=6))[0] == "gate_route_fast_kernel<0>"
    assert rx.dispatch(C("a", "rand", E=1024, topk=64))[0] == "gate_route_kernel<1>"
    assert rx.dispatch(C("a", "rand", **rx.R1, S=17))[0] == "gate_route_kernel<1>"
    r1 = C("a", "rand", **rx.R1, alE=257, extra_n=1, extra_id=256, M=16)
    assert rx.dispatch(r1) == ("gate_route_align_wg_kernel<32>", "wg_small")
    assert rx.dispatch(r1, small_sort=0) == ("gate_route_align_wg_kernel<32>", "wg_general")
    assert rx.dispatch(r1, ticket=1) == ("gate_route_fast_kernel<32>", "ticket")
    assert rx.dispatch(r1, generic=1) == ("gate_route_kernel<1>", "ticket")
    assert rx.variants(r1) == ["default", "gate_generic", "gate_ticket", "gate_small_sort0"]
