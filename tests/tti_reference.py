"""TEST INFRASTRUCTURE ONLY: the TTI medium for the yardstick of tests/psv_reference.py and the checks of tests/psv_media.py.

Importing this module registers ``psv_reference._MEDIA["tti"]``, the masked stress update of the TTI section of
include/mifwi.h (float64 torch, CPU), and builds ``TTI``, the entry ``psv_media.MEDIA`` would hold for the medium:

    mat8 = c13, c11, c55_xz, dt/(h rho_x), dt/(h rho_z), c33, c15, c35
    w = (c55_xz != 0);  A: sxz nodes -> sxx node, A^T: sxx nodes -> sxz node (four-point averages, 0 outside the grid)
    S:  sxx += c11 e1' + c13 e2' + c15 A(w e5');  szz += c13 e1' + c33 e2' + c35 A(w e5')
        sxz += c55_xz e5' + w A^T(c15 e1' + c35 e2'),  e5' = e3' + e4'

With c15 = c35 = 0 every operation of the VTI update comes first and a zero is added: the "vti" reference's numbers.
``stress_tti(masked=False)`` is the same update without w, which tests/test_tti_host.py shows to be unstable; "tti_wx" and
"tti_wz" are the update with w rolled by one column / one row, the yardstick of what the cases can see of the mask's
indexing.  ``inclusion_case`` builds the grids with fluid blocks in the solid on which they differ from "tti"
(tests/test_tti_edges_gpu.py); ``MEDIA3`` is psv_media.MEDIA with TTI, the table of the shared tests.  The 45 degree
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


def stress_tti(masked=True, shift=None):
    """S of a TTI medium as psv_reference takes it; ``masked`` False: without w (the unstable scheme); ``shift`` (rows,
    columns): with w rolled by that much - a wrong scheme, the one a kernel with a one-node error in its mask's indexing
    would compute (tests/test_tti_host.py shows on which cases the references tell the two apart)."""
    def stress(mat, relax):
        c13, c11, c55, c33, c15, c35 = (mat[k][None] for k in (0, 1, 2, 5, 6, 7))
        w = (c55.detach() != 0).to(torch.float64) if masked else torch.ones_like(c55.detach())
        if shift is not None:
            w = torch.roll(w, shift, dims=(1, 2))

        def update(sxx, szz, sxz, r, e1, e2, e3, e4):
            e5 = e3 + e4
            a = avg_to_sxx(w * e5)
            return (sxx + c11 * e1 + c13 * e2 + c15 * a, szz + c13 * e1 + c33 * e2 + c35 * a,
                    sxz + c55 * e5 + w * avg_to_sxz(c15 * e1 + c35 * e2), r)
        return update
    return stress


R._MEDIA["tti"] = (8, stress_tti())
R._MEDIA["tti_wx"] = (8, stress_tti(shift=(0, 1)))            # w one column to the right
R._MEDIA["tti_wz"] = (8, stress_tti(shift=(1, 0)))            # w one row down


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
    for r0, r1, c0, c1 in c.get("blocks", ()):               # true fluid: with vs0 = 0 alone c55' stays non-zero at a tilted node
        eps[r0:r1 + 1, c0:c1 + 1] = 0.0
        dl[r0:r1 + 1, c0:c1 + 1] = 0.0
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


# the media of the shared tests (test_psv_media_gpu.py, test_psv_fuzz_gpu.py, test_psv_host.py) with TTI among them
MEDIA3 = dict(P.MEDIA, tti=TTI)


def variant(medium):
    """TTI under another stress update of the reference ("tti_wx", "tti_wz", "tti_unmasked"): the same case, cached under
    the variant's name."""
    return SimpleNamespace(**dict(vars(TTI), name=medium))


# ---- fluid inclusions: the cases on which the mask's indexing shows -----------------------------------------------------------
# On every case of psv_media.CASES the only fluid is the water layer, w is constant along every row and a mask read from
# the wrong column changes no number (tests/test_tti_host.py pins that).  Here fluid blocks (row0, row1, col0, col1) are
# cut into the solid, one grid per forward tile width.  A block masks the sxz nodes of its rows and columns and of the row
# above and the column left of it (c55_xz is a four-point harmonic average).  Per grid: a block across the adjoint tiles'
# column seam (63|64 or 127|128; I-16's second block lies across 127|128, the forward seam once it is forced to 32 lanes)
# and across the row seam 15|16, a block of one node, a block under the water's last row, whose mask joins the water's, and
# on I-32 and I-64 a block that takes in the last column, whose group is partial; the vertical edges of w fall on all four
# column phases.  Sources sit in the water above the blocks, the receiver line (row 20) runs through two blocks.
INCLUSIONS = {
    "I-16": dict(nz=44, nx=150, ns=2, nt=120, nrec=13, src=((4, 52), (3, 112)),
                 blocks=((13, 22, 61, 70), (26, 30, 126, 130), (24, 24, 34, 34), (6, 9, 97, 105))),
    "I-32": dict(nz=41, nx=117, ns=2, nt=120, fw=0, nrec=13, src=((4, 48), (3, 100)),
                 blocks=((12, 21, 58, 66), (17, 24, 112, 116), (27, 27, 29, 29), (6, 8, 87, 93))),
    "I-64": dict(nz=35, nx=230, ns=2, nt=120, nrec=13, src=((4, 128), (3, 200)),
                 blocks=((13, 21, 122, 131), (17, 23, 224, 229), (25, 25, 63, 63), (6, 9, 186, 194))),
}
INCLUSION_WIDTH = {"I-16": 16, "I-32": 32, "I-64": 64}
# the free-surface form of a grid: shot 0 recorded on the buried line, not on row 0, where the direct wave of a source four
# rows below is 40 times all the other shot records and a mask rolled by a column moves shot 0's traces by 2e-6
FREE_SURFACE = dict(free_surface=True, surface_receivers=False)


def inclusion(name, **more):
    """The configuration (psv_media._config) of an inclusion grid; ``more``: free_surface, source_type, ntap, ..."""
    return dict(INCLUSIONS[name], **more)


def inclusion_case(name, m=TTI, **more):
    """The TTI case of the inclusion grid ``name`` (psv_media.case of ``inclusion(name, **more)``), with what the tests of
    the mask rely on asserted: inside a block vs0 = epsilon = delta = 0 (vp, rho and the tilt stay), so c55_xz, c15 and c35
    are exact zeros there; c55_xz == 0 on the blocks and their rim and nowhere else below the water; c15 and c35 non-zero
    at every sxx node whose A footprint holds masked and unmasked nodes and on the A^T footprint of every unmasked node
    next to a masked one; dmat zero where c55_xz is; the geometry of the comment above."""
    spec = inclusion(name, **more)
    c = P.case(m, spec)
    nz, nx = c["vp"].shape
    blocks = spec["blocks"]
    assert P.width(spec) == INCLUSION_WIDTH[name] and (name == "I-16" or nx % 4 != 0)
    fluid = np.zeros((nz, nx), dtype=bool)
    fluid[:P.WATER] = True
    for r0, r1, c0, c1 in blocks:
        fluid[r0:r1 + 1, c0:c1 + 1] = True
    assert np.array_equal(c["vs"] == 0, fluid) and (c["vp"] > 0).all() and (c["rho"] > 0).all()
    # a node of c55_xz is masked where any of (j, i), (j, i+1), (j+1, i), (j+1, i+1) is fluid (edges replicated)
    pad = np.pad(fluid, ((0, 1), (0, 1)), "edge")
    masked = pad[:-1, :-1] | pad[:-1, 1:] | pad[1:, :-1] | pad[1:, 1:]
    c55, c15, c35 = c["matm"][2], c["matm"][6], c["matm"][7]
    assert np.array_equal(c55 == 0, masked) and np.array_equal(c["mat"][2] == 0, masked) and np.array_equal(c["matlim"][2] == 0, masked)
    assert not c15[fluid].any() and not c35[fluid].any()
    assert not c["dmat"][2][masked].any() and c["dmat"][2][~masked].all()
    w = np.pad(~masked, 1)                                                      # w with zeros outside the grid
    near_a = w[1:-1, 1:-1].astype(int) + w[:-2, 1:-1] + w[1:-1, :-2] + w[:-2, :-2]       # the A footprint of sxx node (j, i)
    mixed = (near_a > 0) & (near_a < 4)
    mixed[0] = mixed[:, 0] = False                                              # there the zeros outside make it "mixed"
    assert mixed[P.WATER:].sum() >= 2 * sum(r1 - r0 + c1 - c0 for r0, r1, c0, c1 in blocks)
    assert c15[mixed].all() and c35[mixed].all()
    beside = ~masked & (np.pad(masked, 1)[:-2, 1:-1] | np.pad(masked, 1)[2:, 1:-1] | np.pad(masked, 1)[1:-1, :-2] | np.pad(masked, 1)[1:-1, 2:])
    for k in (c15, c35):
        q = np.pad(k != 0, ((0, 1), (0, 1)), constant_values=True)              # the A^T footprint, inside the grid
        assert (q[:-1, :-1] & q[1:, :-1] & q[:-1, 1:] & q[1:, 1:])[beside].all()
    # geometry
    edges = (masked[P.WATER:, 1:] != masked[P.WATER:, :-1]).any(axis=0)
    assert {int(i + 1) % 4 for i in np.flatnonzero(edges)} == {0, 1, 2, 3}
    spans = lambda lo, hi: any(r0 <= lo and hi <= r1 for r0, r1, _, _ in blocks)
    assert any(c0 <= s - 1 and s <= c1 for _, _, c0, c1 in blocks for s in (64, 128)) and spans(15, 16)
    assert any(r0 == r1 and c0 == c1 for r0, r1, c0, c1 in blocks) and any(r0 == P.WATER for r0, _, _, _ in blocks)
    if name == "I-16":
        assert any(c0 <= 127 and 128 <= c1 for _, _, c0, c1 in blocks)           # the forward seam at 32 lanes
    else:
        assert any(c1 == nx - 1 for _, _, _, c1 in blocks)                       # the partial last group's padded columns
    rec = np.asarray(c["rc"])[..., 0]
    assert all(fluid.ravel()[rec[s]].any() and not fluid.ravel()[rec[s]].all() for s in range(rec.shape[0]) if (rec[s] // nx >= P.WATER).all())
    return c


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
