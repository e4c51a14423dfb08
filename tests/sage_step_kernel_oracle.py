"""fp64 restatements of the four operations that the SAGE "gcn" training step fuses into its aggregation launches (csrc/spmm.hip,
csrc/source_tail_dev.h), each with a CONDITION SUM: the same expression with every term replaced by its absolute value and every
subtraction by an addition.  A correct fp32 kernel, whatever its summation order, stays within

    |got - value| <= (T + SLACK) * 2^-24 * condition          (bound())

of the fp64 value: T = the number of terms that enter the element (the forward error bound of a length-T sum in any order), SLACK = 16
roundings for the elementwise arithmetic around the sum (the affine map, the reciprocal-and-correct division, 1 / (1 - p)).

  tail_bn / tail_ln    h = drop(relu(norm(z))) of a stored pre-activation (tail_apply)
  sage_mean            (sum_{u -> v} h[u] + h[v]) / (deg + 1)                       (finish_row_s, mean4)
  transposed_sum       da[u] = sum_{v in T(u)} dagg[v] * inv_deg[v]                 (the gather of the two backward kernels)
  bn_dy                dy, S1 = sum dy, S2 = sum dy xhat                            (finish_dy_row)
  ln_dz                dy, dxh, m1, m2, dz, dgamma, dbeta, sum dz                   (finish_ln_row)

Every function returns (value, condition) pairs.  The ReLU gate of the backward is discontinuous: undecided() names the elements whose
fp64 pre-activation is too close to zero for fp32 to decide."""
import numpy as np
import scipy.sparse as sp

F64 = np.float64
U = 2.0 ** -24
SLACK = 16
GATE_ULPS = 8


def bound(terms, cond):
    """The tolerance of an element that `terms` terms enter (scalar or an array that broadcasts against cond)."""
    return (np.asarray(terms, F64) + SLACK) * U * cond


def _adj(indptr, indices, n_cols, weights=None):
    n_rows = len(indptr) - 1
    w = np.ones(len(indices), F64) if weights is None else np.asarray(weights, F64)
    return sp.csr_matrix((w, np.asarray(indices, np.int64), np.asarray(indptr, np.int64)), shape=(n_rows, n_cols))


def _keep(mask, p, like):
    return np.ones_like(like) if mask is None else np.asarray(mask, F64) / (1.0 - p)


# ------------------------------------------------------------------------------------------------ forward
def pre_bn(z, scale=None, shift=None):
    """(y, condition) of the BatchNorm-affine / no-norm pre-activation y = z * scale + shift."""
    z = np.asarray(z, F64)
    if scale is None:
        return z, np.abs(z)
    s, b = np.asarray(scale, F64), np.asarray(shift, F64)
    return z * s + b, np.abs(z * s) + np.abs(b)


def pre_ln(z, mean, rstd, gamma, beta):
    """(y, condition, xhat, |xhat| condition) of y = ((z - mean_r) * rstd_r) * gamma + beta with per-row statistics."""
    z, mu, rs = np.asarray(z, F64), np.asarray(mean, F64)[:, None], np.asarray(rstd, F64)[:, None]
    g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
    xh, xc = (z - mu) * rs, (np.abs(z) + np.abs(mu)) * np.abs(rs)
    return xh * g + b, xc * np.abs(g) + np.abs(b), xh, xc


def tail_bn(z, scale=None, shift=None, mask=None, p=0.0):
    """drop(relu(z * scale + shift)); mask [rows, cols] is the 0/1 keep mask keyed by (source row, column).  The condition is NOT gated
    by the ReLU: relu is continuous, a pre-activation that rounds across zero moves the result by its own rounding error only."""
    y, c = pre_bn(z, scale, shift)
    k = _keep(mask, p, y)
    return np.maximum(y, 0) * k, c * k


def tail_ln(z, mean, rstd, gamma, beta, mask=None, p=0.0):
    y, c, _, _ = pre_ln(z, mean, rstd, gamma, beta)
    k = _keep(mask, p, y)
    return np.maximum(y, 0) * k, c * k


def sage_mean(indptr, indices, h, h_cond, self_rows=None):
    """The SAGE-"gcn" mean over a block whose destinations are its first sources (or the rows self_rows of h); T = deg + 1."""
    n_dst = len(indptr) - 1
    a = _adj(indptr, indices, h.shape[0])
    own = slice(0, n_dst) if self_rows is None else np.asarray(self_rows, np.int64)
    d1 = (np.diff(indptr).astype(F64) + 1)[:, None]
    return (a @ h + h[own]) / d1, (a @ h_cond + h_cond[own]) / d1, d1


# ------------------------------------------------------------------------------------------------ backward
def transposed_sum(t_indptr, t_indices, dagg, inv_deg):
    """da = (A^T + I_dst)(dagg * inv_deg) over the transposed block with its self entries; (value, condition, entries per row)."""
    w = np.asarray(inv_deg, F64)[np.asarray(t_indices, np.int64)]
    a = _adj(t_indptr, t_indices, dagg.shape[0], w)
    dagg = np.asarray(dagg, F64)
    return a @ dagg, a @ np.abs(dagg), np.diff(t_indptr).astype(F64)[:, None]


def undecided(y, y_cond):
    """Elements whose ReLU gate fp32 cannot be trusted to decide as fp64 does."""
    return np.abs(y) <= GATE_ULPS * U * y_cond


def bn_dy(da, da_cond, z, mean, rstd, a_scale, a_shift, mask=None, p=0.0):
    """finish_dy_row over all rows: dict(dy, S1, S2) of (value, condition) pairs + the undecided elements.  The column sums' conditions
    carry, per undecided element, the |dy| term it would add if the gate fell the other way."""
    z = np.asarray(z, F64)
    y, yc = pre_bn(z, a_scale, a_shift)
    k = _keep(mask, p, y)
    und = undecided(y, yc)
    gate = (y > 0).astype(F64)
    dy, dyc = da * k * gate, da_cond * k * gate
    mu, rs = np.asarray(mean, F64), np.asarray(rstd, F64)
    xh, xc = (z - mu) * rs, (np.abs(z) + np.abs(mu)) * np.abs(rs)
    flip = da_cond * k * und                                        # what an undecided gate may add to or take from its column
    return dict(dy=(dy, dyc), S1=(dy.sum(0), dyc.sum(0)), S2=((dy * xh).sum(0), (dyc * xc).sum(0)),
                flip=(flip.sum(0), (flip * xc).sum(0)), undecided=und)


def ln_dz(da, da_cond, z, mean, rstd, gamma, beta, mask=None, p=0.0):
    """finish_ln_row over all rows (d = z.shape[1] real columns: m1, m2 are means over d)."""
    y, yc, xh, xc = pre_ln(z, mean, rstd, gamma, beta)
    g, rs = np.asarray(gamma, F64), np.asarray(rstd, F64)[:, None]
    k = _keep(mask, p, y)
    und = undecided(y, yc)
    gate = (y > 0).astype(F64)
    dy, dyc = da * k * gate, da_cond * k * gate
    dxh, dxc = dy * g, dyc * np.abs(g)
    m1, m1c = dxh.mean(1, keepdims=True), dxc.mean(1, keepdims=True)
    m2, m2c = (dxh * xh).mean(1, keepdims=True), (dxc * xc).mean(1, keepdims=True)
    dz, dzc = rs * (dxh - m1 - xh * m2), np.abs(rs) * (dxc + m1c + xc * m2c)
    flip = da_cond * k * und
    # ... and to its whole ROW of dz: the condition of dz with the flipped |dy| terms alone in the place of dy
    fx = flip * np.abs(g)
    flip_dz = np.abs(rs) * (fx + fx.mean(1, keepdims=True) + xc * (fx * xc).mean(1, keepdims=True))
    return dict(dy=(dy, dyc), dxh=(dxh, dxc), m1=(m1, m1c), m2=(m2, m2c), dz=(dz, dzc),
                dgamma=((dy * xh).sum(0), (dyc * xc).sum(0)), dbeta=(dy.sum(0), dyc.sum(0)), sum_dz=(dz.sum(0), dzc.sum(0)),
                flip=(flip.sum(0), (flip * xc).sum(0), flip_dz.sum(0)), undecided=und)
