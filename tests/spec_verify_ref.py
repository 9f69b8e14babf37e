"""Draft verification of speculative decoding with sampling (chitu_hip_speculative_verify, csrc/sample.hip): the integer
specification, stated on top of oracle/sampling.py's restatement of chitu_hip_sample (the same 2^40 fixed-point weights, the same
kept set, the same inverse CDF in index order).  New: the reference project has no speculative path.

The drafters are deterministic, so the draft distribution is a point mass at the draft d and rejection sampling against the target
distribution p (the one chitu_hip_sample draws from for the row) is: accept d with probability p(d); otherwise emit a draw from p
with d removed and the rest renormalised.  The emitted token is distributed as p:
    P(emit d) = p(d);   P(emit x != d) = (1 - p(d)) * p(x) / (1 - p(d)) = p(x).

In integers, with K the kept set, w_i = floor(e_i * 2^40) for i in K, S = sum_K w_i and target(u, s) the sampler's formula:
    greedy row (top_k == 1) or S == 0:  accepted iff d == argmax, token = argmax
    otherwise, w_d = d's kept weight (0 if d is not kept or out of range):
        accepted iff target(u_acc, S) < w_d, token = d
        else token = inverse CDF in index order over K \\ {d} at target(u_alt, S - w_d)
    d < 0 (the bonus row after the last draft): not accepted, token = chitu_hip_sample's for u_alt.
Per sequence of T rows: n_ok = leading accepted rows among the first T - 1; out = [n_ok + 1, tok[0 .. n_ok], -1 ...].
"""

import numpy as np

from oracle import sampling as osmp


def target(u, s):
    """integer position in [0, s) that a uniform u selects (sample_fixed_point's formula), s > 0"""
    uu = np.float32(min(max(np.float32(u), np.float32(0)), np.float32(1)))
    t = np.float64(uu) * np.float64(s)
    return s - 1 if t >= np.float64(s) else min(int(t), s - 1)


def kept_weights(row, temperature, top_k, top_p, probs_mode=False):
    """What verification needs of one row: w (uint64 [vocab], the kept integer weights, 0 outside K), S, the arg-max, and whether
    the row is greedy or degenerate (accepted iff draft == arg-max)."""
    x, e, fix = osmp._weights_fixed(row, temperature, probs_mode)
    arg_max = osmp._argmax(x)
    if top_k == 1:
        return dict(w=None, S=0, arg_max=arg_max, mask=None)
    mask, n, fix, z = osmp.kept_set_fixed_point(row, temperature, top_k, top_p, probs_mode)
    w = np.where(mask, fix, np.uint64(0)).astype(np.uint64)
    return dict(w=w, S=int(w.sum(dtype=np.uint64)), arg_max=arg_max, mask=mask)


def _inverse_cdf(w, t):
    return int(np.searchsorted(np.cumsum(w, dtype=np.uint64), np.uint64(t), side="right"))


def verify_row_from(kw, draft, u_acc, u_alt):
    """(accepted, token) of one row from kept_weights(...)"""
    draft = int(draft)
    w, S, arg_max = kw["w"], kw["S"], kw["arg_max"]
    if w is None or S == 0:
        return (draft >= 0 and draft == arg_max), arg_max
    if draft < 0:
        return False, _inverse_cdf(w, target(u_alt, S))
    w_d = int(w[draft]) if draft < w.size else 0
    if target(u_acc, S) < w_d:
        return True, draft
    if w_d:
        w = w.copy()
        w[draft] = 0
    return False, _inverse_cdf(w, target(u_alt, S - w_d))


def verify_row(row, temperature, top_k, top_p, draft, u_acc, u_alt, probs_mode=False):
    return verify_row_from(kept_weights(row, temperature, top_k, top_p, probs_mode), draft, u_acc, u_alt)


def sequences(accepted, tokens, T):
    """out [bs, T + 1] int64 from the per-row results: the emitted count, the emitted tokens, -1 padding"""
    accepted, tokens = list(accepted), list(tokens)
    assert len(accepted) == len(tokens) and len(tokens) % T == 0
    out = np.full((len(tokens) // T, T + 1), -1, dtype=np.int64)
    for b in range(out.shape[0]):
        n_ok = 0
        while n_ok < T - 1 and accepted[b * T + n_ok]:
            n_ok += 1
        out[b, 0] = n_ok + 1
        out[b, 1 : n_ok + 2] = tokens[b * T : b * T + n_ok + 1]
    return out


def verify(rows, T, temperatures, top_ks, top_ps, drafts, uniforms, probs_mode=False):
    """(accepted [rows] bool list, tokens [rows] int list, out [bs, T + 1]) for rows [bs * T, vocab], uniforms [bs * T, 2]"""
    acc, tok = [], []
    for r in range(len(rows)):
        a, t = verify_row(rows[r], temperatures[r], int(top_ks[r]), float(top_ps[r]), drafts[r], uniforms[r][0], uniforms[r][1], probs_mode)
        acc.append(bool(a))
        tok.append(int(t))
    return acc, tok, sequences(acc, tok, T)


def u_around(w_d, S):
    """float32 uniforms on both sides of the acceptance threshold w_d / S: (the largest u with target(u, S) < w_d or None if there is
    none, the smallest u with target(u, S) >= w_d or None)"""
    one_below = np.nextafter(np.float32(1), np.float32(0))
    u = np.float32(min(w_d / S, float(one_below)))
    while u > 0 and target(u, S) >= w_d:
        u = np.nextafter(u, np.float32(0))
    while u < one_below and target(np.nextafter(u, np.float32(1)), S) < w_d:
        u = np.nextafter(u, np.float32(1))
    below = float(u) if target(u, S) < w_d else None
    above = np.nextafter(u, np.float32(1)) if below is not None else np.float32(0)
    above = float(above) if above <= one_below and target(above, S) >= w_d else None
    return below, above
