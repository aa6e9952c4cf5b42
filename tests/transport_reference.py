"""Float64 numpy definition of the optimal-transport (W2) trace objective (misfit.transport, csrc/mifwi_transport.hip): test
infrastructure only.

Traces are [nt, ntrace], time on axis 0 and counted in samples; every trace is treated on its own; ``b`` > 0 is one
absolute scalar.  With s the modelled and o the observed trace:

    u = softplus(b s),  p = u / sum u,  P = cumsum p          v, q, Q likewise from o           (Q_{-1} = 0)
    Pm_k = P_k - p_k / 2,  tau_k = k + 1/2
    j(k) = the first j with Q_j >= Pm_k (clamped to nt - 1),  T_k = j + (Pm_k - Q_{j-1}) / q_j
    W = sum_k p_k (tau_k - T_k)**2,  loss = 1/2 sum over traces of W
    a_k = 2 p_k (T_k - tau_k) / q_j(k),  g_m = (tau_m - T_m)**2 + a_m / 2 + sum_{k > m} a_k
    dloss/ds_m = 1/2 (g_m - sum_k g_k p_k) / U * b * sigmoid(b s_m)

A term whose divisor q_j is zero contributes 0 (T_k = tau_k there); a trace with U == 0 or V == 0 contributes 0 and gets a
zero adjoint source."""
import numpy as np


def softplus(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(under="ignore"):
        return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def trace_terms(s, o, b):
    """One trace: (W, dW/ds) as float and [nt]"""
    nt = s.shape[0]
    u, v = softplus(b * s), softplus(b * o)
    U, V = float(u.sum()), float(v.sum())
    if U == 0.0 or V == 0.0:
        return 0.0, np.zeros(nt)
    p, q = u / U, v / V
    P, Q = np.cumsum(p), np.cumsum(q)
    Pm = P - 0.5 * p
    k = np.arange(nt)
    tau = k + 0.5
    j = np.minimum(np.searchsorted(Q, Pm, side="left"), nt - 1)
    Qprev = np.where(j > 0, Q[np.maximum(j - 1, 0)], 0.0)
    qj = q[j]
    live = qj > 0
    safe = np.where(live, qj, 1.0)
    d = np.where(live, j + (Pm - Qprev) / safe - tau, 0.0)                   # T - tau
    a = np.where(live, 2.0 * p * d / safe, 0.0)
    suffix = np.concatenate([np.cumsum(a[::-1])[::-1][1:], [0.0]])          # sum_{k > m} a_k
    g = d * d + 0.5 * a + suffix
    return float((p * d * d).sum()), (g - float((g * p).sum())) / U * b * sigmoid(b * s)


def loss_adj(s, o, b):
    """loss = 1/2 sum over traces of W and adj = dloss/ds for traces [nt, ntrace] (or one trace [nt])"""
    s, o = np.asarray(s, dtype=np.float64), np.asarray(o, dtype=np.float64)
    if s.ndim == 1:
        w, adj = trace_terms(s, o, float(b))
        return 0.5 * w, 0.5 * adj
    loss, adj = 0.0, np.zeros_like(s)
    for tr in range(s.shape[1]):
        w, adj[:, tr] = trace_terms(s[:, tr], o[:, tr], float(b))
        loss += w
    return 0.5 * loss, 0.5 * adj


def composed(s, o, sos, sel_dense, b=None, b_rel=4.0):
    """Loss and dloss/ds of transport(W F s, W F o) (envelope_reference.stage_and_window); b None: b_rel / max|W F o|.
    Returns (loss, grad, b)."""
    from scipy import signal
    from envelope_reference import stage_and_window
    shape = np.shape(s)
    ws, wo = stage_and_window(s, sos, sel_dense), stage_and_window(o, sos, sel_dense)
    if b is None:
        b = b_rel / float(np.abs(wo).max())
    loss, adj = loss_adj(ws.reshape(shape[0], -1), wo.reshape(shape[0], -1), b)
    adj = adj.reshape(shape)
    if sel_dense is not None:
        adj = adj * sel_dense
    if sos is not None:
        adj = signal.sosfilt(sos, adj[::-1], axis=0)[::-1]
    return loss, adj, b
