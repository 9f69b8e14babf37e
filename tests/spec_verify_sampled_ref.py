"""Verification of a SAMPLED draft (chitu_hip_speculative_verify_sampled, csrc/sample.hip): the integer specification, stated in Python
integers on top of oracle/sampling.py and tests/spec_verify_ref.py.  New: the reference project has no speculative path.

The draft d of a row was drawn from the draft model's distribution q (cut under the row's own temperature / top_k / top_p, as the
target's p is).  Rejection sampling: accept d with probability min(1, p(d) / q(d)); otherwise emit a draw from max(p - q, 0),
renormalised.  The emitted token is distributed as p for any q:
    P(emit x) = q(x) min(1, p(x) / q(x)) + P(reject) * max(p(x) - q(x), 0) / sum_y max(p(y) - q(y), 0)
              = min(p(x), q(x)) + max(p(x) - q(x), 0) = p(x),    since P(reject) = 1 - sum_y min(p(y), q(y)) = sum_y max(p(y) - q(y), 0).

In integers, with K_p, w_i, S_p = kept_weights of the target row, K_q, v_i, S_q = the same of the draft row (so p_i = w_i / S_p,
q_i = v_i / S_q) and U(u) = min(floor(u * 2^24), 2^24 - 1) for a float32 u clamped to [0, 1]:
    greedy row (top_k == 1), S_p == 0 or S_q == 0:  accepted iff d == argmax(target row), token = that arg-max
    d < 0 (the bonus row):                          not accepted, token = chitu_hip_sample's for u_alt on the target row
    otherwise, w_d / v_d = d's kept weights (0 when not kept or d >= vocab):
        accepted iff U(u_acc) * v_d * S_p < 2^24 * w_d * S_q, token = d
        else r_i = max(0, w_i * S_q - v_i * S_p), R = sum r_i, t = (R >> 24) * U + (((R & (2^24 - 1)) * U) >> 24) with U = U(u_alt)
             (exactly floor(U * R / 2^24)), token = inverse CDF over r in index order at t; R == 0: the arg-max.
Per sequence of T rows: spec_verify_ref.sequences.
"""

import numpy as np

from tests import spec_verify_ref as sv

GRID_BITS = 24
GRID = 1 << GRID_BITS


def grid(u):
    """U(u): the uniform on the 2^-24 grid (u * 2^24 is exact in float32; NaN counts as 0)"""
    uu = np.float32(u)
    if np.isnan(uu):
        return 0
    uu = min(max(uu, np.float32(0)), np.float32(1))
    return min(int(np.float32(uu) * np.float32(GRID)), GRID - 1)


kept_weights = sv.kept_weights


def _ints(w):
    return [int(x) for x in w]


def residual(kw_p, kw_q):
    """(r as Python ints, R); kept with kw_q for the next row of the same pair"""
    memo = kw_q.get("_residual")
    if memo is None or memo[0] is not kw_p:
        S_p, S_q = kw_p["S"], kw_q["S"]
        r = [max(0, a * S_q - b * S_p) for a, b in zip(_ints(kw_p["w"]), _ints(kw_q["w"]))]
        memo = kw_q["_residual"] = (kw_p, r, sum(r))
    return memo[1], memo[2]


def position(R, U):
    t = (R >> GRID_BITS) * U + (((R & (GRID - 1)) * U) >> GRID_BITS)
    assert t == (U * R) >> GRID_BITS
    return t


def accepts(w_d, v_d, S_p, S_q, U):
    return U * v_d * S_p < GRID * w_d * S_q


def verify_row_from(kw_p, kw_q, draft, u_acc, u_alt):
    """(accepted, token) of one row pair from the two kept_weights(...)"""
    draft = int(draft)
    arg_max = kw_p["arg_max"]
    if kw_p["w"] is None or kw_p["S"] == 0:
        return (draft >= 0 and draft == arg_max), arg_max
    if draft < 0:
        return sv.verify_row_from(kw_p, draft, u_acc, u_alt)
    if kw_q["w"] is None or kw_q["S"] == 0:
        return draft == arg_max, arg_max
    n = kw_p["w"].size
    w_d = int(kw_p["w"][draft]) if draft < n else 0
    v_d = int(kw_q["w"][draft]) if draft < n else 0
    if accepts(w_d, v_d, kw_p["S"], kw_q["S"], grid(u_acc)):
        return True, draft
    r, R = residual(kw_p, kw_q)
    if R == 0:
        return False, arg_max
    t = position(R, grid(u_alt))
    acc = 0
    for i, ri in enumerate(r):
        acc += ri
        if acc > t:
            return False, i
    raise AssertionError("unreachable")


def verify_row(row, draft_row, temperature, top_k, top_p, draft, u_acc, u_alt, probs_mode=False):
    kw_p = kept_weights(row, temperature, top_k, top_p, probs_mode)
    kw_q = None if (int(draft) < 0 or draft_row is None) else kept_weights(draft_row, temperature, top_k, top_p, probs_mode)
    return verify_row_from(kw_p, kw_q, draft, u_acc, u_alt)


def verify(rows, draft_rows, T, temperatures, top_ks, top_ps, drafts, uniforms, probs_mode=False):
    """(accepted [rows] bool list, tokens [rows] int list, out [bs, T + 1]) for rows / draft_rows [bs * T, vocab], uniforms [bs * T, 2]"""
    acc, tok = [], []
    for r in range(len(rows)):
        a, t = verify_row(rows[r], draft_rows[r], temperatures[r], int(top_ks[r]), float(top_ps[r]), drafts[r], uniforms[r][0],
                          uniforms[r][1], probs_mode)
        acc.append(bool(a))
        tok.append(int(t))
    return acc, tok, sv.sequences(acc, tok, T)


def u_acc_around(w_d, v_d, S_p, S_q):
    """The two grid neighbours of the acceptance threshold as float32 uniforms: (the largest grid u that accepts or None, the
    smallest that rejects or None).  accepts() is monotone in U: true up to some U, false from there on."""
    lo, hi = -1, GRID  # lo accepts (or -1), hi rejects (or GRID)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepts(w_d, v_d, S_p, S_q, mid):
            lo = mid
        else:
            hi = mid
    below = float(np.float32(lo) / np.float32(GRID)) if lo >= 0 else None
    above = float(np.float32(hi) / np.float32(GRID)) if hi < GRID else None
    return below, above
