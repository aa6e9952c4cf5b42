"""TEST INFRASTRUCTURE ONLY: the yardstick of the viscoacoustic fluid propagator.

A float64 torch (CPU) restatement of the four-field recursion of the viscoacoustic section of include/mifwi.h: the fluid
scheme (vx, vz, p, four C-PML memory variables, odd mirroring of p under a free surface) with one memory variable r on the
p node, ``relax`` = (a, b):

    mat4 = K_u, dt/(h rho_x), dt/(h rho_z), R          (the moduli times dt/h)
    V:  vx += bx d1',  vz += bz d4'                     (d1, d4 = Dp_x p, Dp_z p);  fx / fz: vx / vz += w f
    P:  q = R (e1' + e2');  p += K_u e1' + K_u e2' + ((1 + a)/2 r - b/2 q);  r = a r - b q      (e1, e2 = Dm_x vx, Dm_z vz)
        explosive: p += w f;  free surface: p(0,.) = 0
    rec_vx, rec_vz = sum w v,  rec_p = sum w (p + p)

Stencils, padding, taps and the C-PML recursion are those of tests/psv_reference.py (imported, one copy); tests/
test_viscofluid_host.py pins this file to ``psv_reference.forward(medium="visco")`` on ``visco.materials(vp, 0, rho, qp,
inf, ...)``, which inherits the physics pin of tests/test_visco_host.py.  Autograd through :func:`forward` gives the
gradients with respect to the planes and ``f``; a central difference of it gives J.  Shots are vectorised, time is a
Python loop.
"""
import numpy as np
import torch

from psv_reference import PA, PAH, PB, PBH, PK, PKH, _Taps, _pad, _pad_odd, _shift, _t


def forward(mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, relax, free_surface=0, fd_order=4, source_type=0):
    """mat [4,nz,nx], pz [6,nz], px [6,nx], f [nt,ns,nsrc]; cells [ns,n,ntap] (negative: inactive); relax = (a, b).  Returns
    (rec_vx, rec_vz, rec_p), float64 tensors [nt,ns,nrec]; ``mat`` and ``f`` may require gradients."""
    mat, pz, px, f = _t(mat), _t(pz), _t(px), _t(f)
    assert mat.shape[0] == 4
    _, nz, nx = mat.shape
    nt, ns, _ = f.shape
    c1, c2 = (1.0, 0.0) if fd_order == 2 else (9.0 / 8.0, -1.0 / 24.0)
    K, bx, bz, Rm = (mat[k][None] for k in range(4))
    ra, rb = float(relax[0]), float(relax[1])
    X = [px[k][None, None, :] for k in range(6)]
    Z = [pz[k][None, :, None] for k in range(6)]
    src, rec = _Taps(src_cell, src_w, nz * nx), _Taps(rec_cell, rec_w, nz * nx)
    zero = torch.zeros(ns, nz, nx, dtype=torch.float64)
    vx = vz = p = r = zero
    psi = [zero] * 4
    keep = torch.ones(1, nz, 1, dtype=torch.float64)
    keep[0, 0, 0] = 0.0

    def dp(P, ax):          # forward difference, lands on +1/2
        s = (lambda k: _shift(P, k, 0, nz, nx)) if ax == 0 else (lambda k: _shift(P, 0, k, nz, nx))
        return c1 * (s(1) - s(0)) + c2 * (s(2) - s(-1))

    def dm(P, ax):          # backward difference
        s = (lambda k: _shift(P, k, 0, nz, nx)) if ax == 0 else (lambda k: _shift(P, 0, k, nz, nx))
        return c1 * (s(0) - s(-1)) + c2 * (s(1) - s(-2))

    def pml(k, T, half, d):
        a, b, ik = (T[PAH], T[PBH], T[PKH]) if half else (T[PA], T[PB], T[PK])
        psi[k] = b * psi[k] + a * d
        return d * ik + psi[k]

    out = [], [], []
    for n in range(nt):
        Pp = _pad_odd(p, 1) if free_surface else _pad(p)
        d1 = pml(0, X, True, dp(Pp, 1))
        d4 = pml(1, Z, True, dp(Pp, 0))
        vx = vx + bx * d1
        vz = vz + bz * d4
        if source_type == 1:
            vx = vx + src.scatter(f[n]).reshape(ns, nz, nx)
        elif source_type == 2:
            vz = vz + src.scatter(f[n]).reshape(ns, nz, nx)
        e1 = pml(2, X, False, dm(_pad(vx), 1))
        e2 = pml(3, Z, False, dm(_pad(vz), 0))
        q = Rm * (e1 + e2)
        p = p + K * e1 + K * e2 + (0.5 * (1.0 + ra) * r - 0.5 * rb * q)
        r = ra * r - rb * q
        if source_type == 0:
            p = p + src.scatter(f[n]).reshape(ns, nz, nx)
        if free_surface:
            p = p * keep
        out[0].append(rec.gather(vx))
        out[1].append(rec.gather(vz))
        out[2].append(rec.gather(p + p))
    return tuple(torch.stack(o) for o in out)


def gradients(mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, g, relax, **kw):
    """(traces [3], grad_mat, grad_f, g) as float64 numpy arrays: the three traces and the gradient of sum(g_k rec_k) by
    autograd.  ``g`` may be a callable (rec_vx, rec_vz, rec_p) -> three adjoint sources of the traces as numpy arrays."""
    m = _t(mat).clone().requires_grad_(True)
    ff = _t(f).clone().requires_grad_(True)
    rec = forward(m, pz, px, ff, src_cell, src_w, rec_cell, rec_w, relax, **kw)
    if callable(g):
        g = g(*(a.detach().numpy() for a in rec))
    sum((a * _t(b)).sum() for a, b in zip(rec, g)).backward()
    return [a.detach().numpy() for a in rec], m.grad.numpy(), ff.grad.numpy(), list(g)


def jvp(mat, dmat, pz, px, f, df, src_cell, src_w, rec_cell, rec_w, relax, eps=1e-5, **kw):
    """J (dmat, df) [3,nt,ns,nrec] by a central difference of :func:`forward` (``df`` None: no source perturbation)."""
    m, dm_, ff = _t(mat), _t(dmat), _t(f)
    dff = torch.zeros_like(ff) if df is None else _t(df)
    with torch.no_grad():
        p = forward(m + eps * dm_, pz, px, ff + eps * dff, src_cell, src_w, rec_cell, rec_w, relax, **kw)
        q = forward(m - eps * dm_, pz, px, ff - eps * dff, src_cell, src_w, rec_cell, rec_w, relax, **kw)
    return np.stack([((a - b) / (2 * eps)).numpy() for a, b in zip(p, q)])
