"""The definitions of ``dvg_packed_bonds`` ("DVG bonds v1") and ``dvg_packed_overlap_link`` ("DVG link overlap v1",
include/dvg.h) in numpy -- a helper of the bond tests, not a test.  Rows are unpacked with ``trace_oracle.unpack`` (bits of
spins >= n dropped); the bonds are ``t = s[:, edge_i] * s[:, edge_j]`` followed by the sign rule of satisfied mode, packed with
``trace_oracle.pack`` (pad bits 0).  Pair statistics come from the int64 Gram matrices of the spins and of the bonds: d = (n -
G) / 2, l = (E - G_t) / 2, ``np.bincount`` for the two histograms and ``np.add.at`` for the sums of l and l^2 per d.  The
estimators of ``sampler.LinkOverlap`` are restated next to them, each sum written out as the definition has it."""
import numpy as np

import trace_oracle


def _u32(bits):
    bits = np.asarray(bits)
    return bits.view(np.uint32) if bits.dtype == np.int32 else bits


def bond_spins(s, edge_i, edge_j, quadratic=None):
    """(..., n) +-1 -> (..., E) int8 +-1: s_i s_j, or with ``quadratic`` +1 iff the bond is satisfied."""
    s = np.asarray(s, dtype=np.int8)
    t = s[..., np.asarray(edge_i)] * s[..., np.asarray(edge_j)]
    if quadratic is not None:
        J = np.asarray(quadratic, dtype=np.float32)
        t = np.where(J > 0, -t, np.where(J < 0, t, np.int8(1)))  # (+0, -0 and NaN are neither: always satisfied)
    return t.astype(np.int8)


def bonds(bits, n, edge_i, edge_j, quadratic=None):
    """Packed rows (..., W) -> packed bond rows (..., WE) uint32, bits >= E cleared."""
    return trace_oracle.pack(bond_spins(trace_oracle.unpack(_u32(bits), n), edge_i, edge_j, quadratic))


def _groups(bits, n):
    """(rows, W) or (C, M, W) packed -> (groups, rows, n) int64 +-1: a 3-D set is M groups of C rows."""
    s = trace_oracle.unpack(_u32(bits), n).astype(np.int64)
    return s[None] if s.ndim == 2 else s.transpose(1, 0, 2)


def link_overlap(a, a_bonds, b, b_bonds, n, n_edges):
    """``(hist (n + 1,), link_hist (E + 1,), link_sum (n + 1,), link_sq (n + 1,))`` int64 of packed ``a`` with bond rows
    ``a_bonds`` against ``b`` / ``b_bonds`` (None: self mode; 2-D with a 3-D ``a``: shared by every group)."""
    E = n_edges
    A, TA = _groups(a, n), _groups(a_bonds, E)
    B, TB = (None, None) if b is None else (_groups(b, n), _groups(b_bonds, E))
    assert A.shape[:2] == TA.shape[:2] and (B is None or B.shape[:2] == TB.shape[:2])
    if B is not None and B.shape[0] == 1 and A.shape[0] > 1:
        B, TB = np.broadcast_to(B, (A.shape[0],) + B.shape[1:]), np.broadcast_to(TB, (A.shape[0],) + TB.shape[1:])
    hist, link_hist = np.zeros(n + 1, dtype=np.int64), np.zeros(E + 1, dtype=np.int64)
    link_sum, link_sq = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for g in range(A.shape[0]):
        gs, gt = A[g] @ (A[g] if B is None else B[g]).T, TA[g] @ (TA[g] if B is None else TB[g]).T
        assert ((n - gs) % 2 == 0).all() and ((E - gt) % 2 == 0).all()
        d, l = (n - gs) // 2, (E - gt) // 2
        if B is None:
            pick = np.triu_indices(d.shape[0], 1)
            d, l = d[pick], l[pick]
        d, l = d.reshape(-1), l.reshape(-1)
        hist += np.bincount(d, minlength=n + 1)
        link_hist += np.bincount(l, minlength=E + 1)
        np.add.at(link_sum, d, l)
        np.add.at(link_sq, d, l * l)
    return hist, link_hist, link_sum, link_sq


# ---------------------------------------------------------------------------------------------------- sampler.LinkOverlap
def pair_values(hist, link_hist, link_sum, link_sq, n, n_edges):
    """What the sums say about the pairs: per bin d the count, the grid q_d, and the sums of q_l and q_l^2 over its pairs."""
    h, E = np.asarray(hist, np.float64), float(n_edges)
    s, sq = np.asarray(link_sum, np.float64), np.asarray(link_sq, np.float64)
    q = 1.0 - 2.0 * np.arange(n + 1, dtype=np.float64) / n
    return h, q, h - 2.0 * s / E, h - 4.0 * s / E + 4.0 * sq / (E * E)


def estimates(hist, link_hist, link_sum, link_sq, n, n_edges):
    """Every property of ``sampler.LinkOverlap`` (and ``fit()`` as ``fit_a``, ``fit_b``) by name, float64 numpy."""
    h, q, s1, s2 = pair_values(hist, link_hist, link_sum, link_sq, n, n_edges)
    lh = np.asarray(link_hist, np.float64)
    ql = 1.0 - 2.0 * np.arange(n_edges + 1, dtype=np.float64) / n_edges
    with np.errstate(invalid="ignore", divide="ignore"):
        P = h.sum()
        x = q ** 2
        mx, my = (h * x).sum() / P, 1.0 - 2.0 * np.asarray(link_sum, np.float64).sum() / (n_edges * P)
        var_x = (h * (x - mx) ** 2).sum() / P
        var_y = (lh * (ql - my) ** 2).sum() / P
        cov = ((x - mx) * (s1 - my * h)).sum() / P
        b = cov / var_x
        return dict(pairs=P, q=q, link_given_q=1.0 - 2.0 * np.asarray(link_sum, np.float64) / (n_edges * h), link_var_given_q=s2 / h - (s1 / h) ** 2, mean_link=my,
                    corr_q2_link=cov / np.sqrt(var_x * var_y), fit_a=my - b * mx, fit_b=b)
