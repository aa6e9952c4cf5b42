"""TEST INFRASTRUCTURE ONLY: the TTI medium for the yardstick of tests/psv_reference.py and the checks of tests/psv_media.py.

Importing this module registers ``psv_reference._MEDIA["tti"]``, the masked stress update of the TTI section of
include/mifwi.h (float64 torch, CPU), and builds ``TTI``, the entry ``psv_media.MEDIA`` would hold for the medium:

    mat8 = c13, c11, c55_xz, dt/(h rho_x), dt/(h rho_z), c33, c15, c35
    w = (c55_xz != 0);  A: sxz nodes -> sxx node, A^T: sxx nodes -> sxz node (four-point averages, 0 outside the grid)
    S:  sxx += c11 e1' + c13 e2' + c15 A(w e5');  szz += c13 e1' + c33 e2' + c35 A(w e5')
        sxz += c55_xz e5' + w A^T(c15 e1' + c35 e2'),  e5' = e3' + e4'

With c15 = c35 = 0 every operation of the VTI update comes first and a zero is added: the "vti" reference's numbers.
``stress_tti(masked=False)`` is the same update without w, which tests/test_tti_host.py shows to be unstable.  The 45 degree
physics pin (``pin_case`` / ``pin_check``) and the long run of the stability test serve the host test on this reference and
the GPU test on the kernels alike.
"""
from types import SimpleNamespace

import numpy as np
import torch

import psv_media as P
import psv_reference as R
from oracle import helpers as H


def avg_to_sxx(q):
    """(A q)(j,i) = 1/4 [q(j,i) + q(j-1,i) + q(j,i-1) + q(j-1,i-1)] of q [ns,nz,nx]"""
    p = torch.nn.functional.pad(q, (1, 0, 1, 0))
    return 0.25 * (p[:, 1:, 1:] + p[:, :-1, 1:] + p[:, 1:, :-1] + p[:, :-1, :-1])


def avg_to_sxz(q):
    """(A^T p)(j,i) = 1/4 [p(j,i) + p(j+1,i) + p(j,i+1) + p(j+1,i+1)] of p [ns,nz,nx]"""
    p = torch.nn.functional.pad(q, (0, 1, 0, 1))
    return 0.25 * (p[:, :-1, :-1] + p[:, 1:, :-1] + p[:, :-1, 1:] + p[:, 1:, 1:])


def stress_tti(masked=True):
    """S of a TTI medium as psv_reference takes it; ``masked`` False: without w (the unstable scheme)."""
    def stress(mat, relax):
        c13, c11, c55, c33, c15, c35 = (mat[k][None] for k in (0, 1, 2, 5, 6, 7))
        w = (c55.detach() != 0).to(torch.float64) if masked else torch.ones_like(c55.detach())

        def update(sxx, szz, sxz, r, e1, e2, e3, e4):
            e5 = e3 + e4
            a = avg_to_sxx(w * e5)
            return (sxx + c11 * e1 + c13 * e2 + c15 * a, szz + c13 * e1 + c33 * e2 + c35 * a,
                    sxz + c55 * e5 + w * avg_to_sxz(c15 * e1 + c35 * e2), r)
        return update
    return stress


R._MEDIA["tti"] = (8, stress_tti())


def mat8_of(vp0, vs0, rho, epsilon, delta, theta, dt, h, free_surface=False):
    """float64 numpy planes of ``tti.materials`` (the product's torch expression on CPU float64 is the definition)."""
    from physicsbasedfwi2_amd import tti
    t = [torch.tensor(np.asarray(a, dtype=np.float64)) for a in (vp0, vs0, rho, epsilon, delta, theta)]
    return tti.materials(*t, dt, h, free_surface=free_surface).numpy()


def tilt_field(s):
    """The seeded tilt of the cases: 0.6 s radians for a smooth field s in [-1, 1] (+-34 degrees), 0 in the water rows"""
    theta = 0.6 * s
    theta[:P.WATER] = 0.0
    assert np.abs(theta).max() <= 0.6 and theta[P.WATER:].std() > 0.1
    return theta


def _tti_planes(c, s1, s2):
    """The Thomsen fields of the VTI cases (psv_media._thomsen_planes) and the tilt field of s2: the eight planes of
    tti.materials (CPU float64, then rounded)."""
    eps, dl = 0.125 + 0.125 * s1, 0.025 + 0.125 * s2
    eps[:P.WATER] = 0.0
    dl[:P.WATER] = 0.0
    mat8 = P.f32(mat8_of(*P._model3(c), P.f32(eps), P.f32(dl), P.f32(tilt_field(s2.copy())), c["dt"], c["h"],
                         free_surface=bool(c["fs"])))
    assert np.abs(mat8[6]).max() > 0 and np.abs(mat8[7]).max() > 0      # tilted for real
    assert not mat8[6, :P.WATER].any() and not mat8[7, :P.WATER].any() and not mat8[2, :P.WATER].any()
    return mat8


TTI = SimpleNamespace(
    name="tti", planes=("c13", "c11", "c55", "bx", "bz", "c33", "c15", "c35"),
    ISO_OF={"c13": "L", "c11": "M", "c33": "M", "c55": "mu", "bx": "bx", "bz": "bz", "c15": "L", "c35": "L", "f": "f"},
    model=_tti_planes, limit=lambda mat5: np.concatenate([mat5, mat5[1:2], np.zeros((2,) + mat5.shape[1:])]),
    limit_label="tti(iso)", iso=P.MEDIA["vti"].iso, takes_relax=False, plan="TtiPlan", state_fields=None,
    segments_same_bits=True)


def no_coupling(mat8):
    """``mat8`` with c15 = c35 = 0: a medium of VTI form, its six planes the rotated stiffnesses"""
    return np.concatenate([mat8[:6], np.zeros((2,) + mat8.shape[1:])])


# ---- the 45 degree physics pin ------------------------------------------------------------------------------------------
PIN_EPS, PIN_DELTA = 0.2, 0.1


def pin_case(epsilon, delta, theta_deg, vp0=2000.0):
    """psv_reference.pin_case (homogeneous 121 x 121, no layer, explosive source at (60, 60)) with the axis tilted by
    ``theta_deg`` and two vx receivers at (z, x) = (88, 88) and (32, 88): 28 cells along and across the axis of +45 degrees.
    Returns (mat8, pz, px, f, sc, sw, rc, rw)."""
    n, h, dt = 121, 10.0, 1e-3
    _, pz, px, f, sc, sw, _, _ = R.pin_case(epsilon, delta, vp0=vp0)
    full = lambda v: np.full((n, n), float(v))
    mat8 = mat8_of(full(vp0), full(1100.0), full(2000.0), full(epsilon), full(delta), full(np.deg2rad(theta_deg)), dt, h)
    rc, rw = H.cell_taps(np.array([[88, 32]]), np.array([[88, 88]]), n)
    return mat8, pz, px, f, sc, sw, rc, rw


def pin_check(run, theta_deg, report=print):
    """The pin on ``run(mat8, pz, px, f, sc, sw, rc, rw) -> rec_vx`` [nt,1,2]: with epsilon 0.2, delta 0.1 and the axis at
    +45 degrees - along (sin, cos) in (x, z), z down: the slow direction - the qP peak at (88, 88) arrives with the
    isotropic vp0 run's at that receiver and the peak at (32, 88) with the isotropic vp0 sqrt(1 + 2 epsilon) run's, each
    within 2 samples, and the two are more than 25 samples apart.  At -45 degrees the receivers swap roles."""
    along, across = (0, 1) if theta_deg > 0 else (1, 0)
    tilted = run(*pin_case(PIN_EPS, PIN_DELTA, theta_deg))
    slow = run(*pin_case(0.0, 0.0, 0.0))
    fast = run(*pin_case(0.0, 0.0, 0.0, vp0=2000.0 * np.sqrt(1 + 2 * PIN_EPS)))
    t = lambda tr, k: R.peak_time(np.asarray(tr)[:, 0, k])
    d_along, d_across = abs(t(tilted, along) - t(slow, along)), abs(t(tilted, across) - t(fast, across))
    apart = abs(t(tilted, along) - t(tilted, across))
    report("TTI pin at %+d degrees: |t_along - t(vp0)| = %.2f, |t_across - t(vp0 sqrt(1 + 2 eps))| = %.2f, apart %.1f samples"
           % (theta_deg, d_along, d_across, apart))
    assert d_along <= 2.0 and d_across <= 2.0 and apart > 25.0
    return d_along, d_across, apart


# ---- the long run of the stability test ---------------------------------------------------------------------------------
def long_run(medium, nt, window=500):
    """Case A_fw0 (44 x 60, no absorbing layer, water rows above the solid, the seeded tilt field of +-0.6 rad), shot 0,
    its forcing zero-padded to ``nt`` steps, under the reference's ``medium``: max |vx| over the whole grid in every
    ``window`` of steps."""
    c = P.case(TTI, "A_fw0")
    nz, nx = c["vp"].shape
    f = np.zeros((nt, 1, c["f"].shape[2]))
    f[:c["f"].shape[0]] = c["f"][:, :1]
    every = np.arange(nz * nx, dtype=np.int32).reshape(1, -1, 1)
    with torch.no_grad():
        vx, _ = R.forward(c["matm"], c["pz"], c["px"], f, c["sc"][:1], c["sw"][:1], every, np.ones(every.shape), medium,
                          free_surface=c["fs"], fd_order=4)
    return [float(vx[b:b + window].abs().max()) for b in range(0, nt, window)]
