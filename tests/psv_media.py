"""TEST INFRASTRUCTURE ONLY: what the tests of the P-SV media beyond the isotropic one share (tests/test_psv_media_gpu.py,
test_vti_gpu.py, test_visco_gpu.py and the two host modules): the seeded cases, the cached float64 references
(tests/psv_reference.py), the device helpers, ``MEDIA``, which names what differs between the media, and the checks that
the media's own files run under the names their cases have always had (and, on random configurations,
tests/test_psv_fuzz_gpu.py).

A new medium is one more entry of ``MEDIA`` and one more branch of psv_reference's stress update; a test that needs more
of a medium than an entry holds belongs in the medium's own file.

Shapes: A = the default 44 x 60 x 120 steps case (15 groups: less than one column block, a partial tile in z), B = 37 x 150,
3 shots, 50 steps (three column blocks with the last partial, nx no multiple of 4): both run at 16 lanes per row
(``pick_lx``).  C = 41 x 117, 2 shots, 70 steps (30 groups: 32 lanes with two idle, nx % 4 = 1), D = 35 x 230, 2 shots, 60
steps (58 groups: 64 lanes, nx % 4 = 2).  All with an 8-cell C-PML, A and C also without a layer, A and D also with a free
surface (not C: both its sources would sit on the surface row in the water and never see the medium; the reference's
rec_vz and four of its gradient planes are all zero there).  A case is a name of ``CASES`` or a configuration (``case``): the draws of tests/test_psv_fuzz_gpu.py are built,
referenced and checked by the same functions.  Inputs are rounded to f32 first (what the device computes with).  Every
reference result is computed once per case and left unchanged."""
import ctypes
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import torch

import psv_reference as R
from cases import elastic_case, rel_l2
from oracle import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C, _D = dict(nz=41, nx=117, ns=2, nt=70), dict(nz=35, nx=230, ns=2, nt=60)
CASES = {"A": dict(), "A_fw0": dict(fw=0), "A_fs": dict(free_surface=True), "B": dict(nz=37, nx=150, ns=3, nt=50),
         "C": _C, "C_fw0": dict(_C, fw=0), "D": _D, "D_fs": dict(_D, free_surface=True)}
PER_STEP = {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_FUSED": "0"}
TOL_TRACE, TOL_SUM = 2e-6, 2e-5
WATER = 6
# f_relax at the wavelet's centre frequency; the velocities are given at 30 Hz, above the wavelet's band, as a model from
# sonic logs or from another survey would be: the medium then differs from the elastic one by the dispersion of the standard
# linear solid as well as by its loss.  (With f_ref = 10 Hz and any Q field inside the ranges the one live shot of the
# free-surface case at order 2, whose receivers record mostly water-borne energy, moves by 0.6 ... 0.9 %, short of the percent
# that test_attenuating_traces_and_gradients_match_the_reference asks first; with 30 Hz it moves by 6.5 %.)
F_RELAX, F_REF = 8.0, 30.0
_cache = {}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _model3(c):
    return f32(c["vp"]), f32(c["vs"]), f32(c["rho"])


def _thomsen_planes(c, s1, s2):
    """Seeded smooth epsilon in [0, 0.25] and delta in [-0.1, 0.15] over the solid (0 in the water rows): the six planes of
    vti.materials (CPU float64, then rounded)."""
    eps, dl = 0.125 + 0.125 * s1, 0.025 + 0.125 * s2
    eps[:WATER] = 0.0
    dl[:WATER] = 0.0
    assert 0 <= eps.min() and eps.max() <= 0.25 and -0.1 <= dl.min() and dl.max() <= 0.15
    assert eps[WATER:].std() > 0.03 and dl[WATER:].std() > 0.03
    mat6 = f32(R.thomsen_mat6(*_model3(c), f32(eps), f32(dl), c["dt"], c["h"], free_surface=bool(c["fs"])))
    assert rel_l2(mat6[1], mat6[5]) > 0.05                    # anisotropic for real
    return mat6


def _sls_planes(c, s1, s2):
    """Seeded smooth qp in [20, 200] and qs in [10, 100] over the solid (qp = 1000 in the water rows), f_relax = 8 Hz, the
    wavelet's centre frequency, f_ref = 30 Hz: the eight planes of visco.materials (CPU float64, then rounded)."""
    from physicsbasedfwi2_amd import visco
    # u, v smooth in [0, 1]; cubed, the fields spend most of the grid in the lower, attenuating part of their ranges
    # (means about 57 and 33): the 120 steps of case A are two periods of the wavelet, little time for a Q of 100 to act
    u, v = 0.5 + 0.5 * s1, 0.5 + 0.5 * s2
    qp, qs = 20 + 180 * u ** 3, 10 + 90 * v ** 3
    qp[:WATER] = 1000.0
    assert 20 <= qp[WATER:].min() and qp[WATER:].max() <= 200 and 10 <= qs.min() and qs.max() <= 100
    assert qp[WATER:].std() > 10 and qs[WATER:].std() > 5
    c["relax"] = visco.relaxation(F_RELAX, c["dt"])
    mat8 = f32(R.visco_mat8(*_model3(c), f32(qp), f32(qs), F_REF, F_RELAX, c["dt"], c["h"], free_surface=bool(c["fs"])))
    assert all(np.abs(mat8[k]).max() > 0 for k in range(8))
    return mat8


# What differs between the media.  name: the propagator module and the reference's ``medium``; planes, and ISO_OF, the
# isotropic gradient whose error on the same geometry sets a plane's bound; model: the case's planes from two smooth seeded
# fields in [-1, 1]; limit: the planes that must run as the elastic propagator, from mat5, and iso: the limit's (or the
# reference's) plane gradients as the elastic ones, in the order the limit test prints them; takes_relax: propagate / born /
# gauss_newton_product take ``F_RELAX, dt`` and the plan (a, b); state_fields: fields per shot the plan's state must hold
# (eight: the memory variables are state); segments_same_bits: time checkpoints give the resident run's gradient bits.
MEDIA = {
    "vti": SimpleNamespace(
        name="vti", planes=("c13", "c11", "c44", "bx", "bz", "c33"),
        ISO_OF={"c13": "L", "c11": "M", "c33": "M", "c44": "mu", "bx": "bx", "bz": "bz", "f": "f"},
        model=_thomsen_planes, limit=lambda mat5: np.concatenate([mat5, mat5[1:2]]), limit_label="vti(iso)",
        iso=lambda g: {"L": g[0], "mu": g[2], "bx": g[3], "bz": g[4], "M": g[1] + g[5]},
        takes_relax=False, plan="VtiPlan", state_fields=None, segments_same_bits=True),
    "visco": SimpleNamespace(
        name="visco", planes=("lam", "lam2mu", "mu", "bx", "bz", "R2", "R1", "rmu"),
        ISO_OF={"lam": "L", "lam2mu": "M", "mu": "mu", "bx": "bx", "bz": "bz", "R2": "L", "R1": "M", "rmu": "mu", "f": "f"},
        model=_sls_planes, limit=lambda mat5: np.concatenate([mat5, np.zeros((3,) + mat5.shape[1:])]),
        limit_label="visco(elastic limit)",
        iso=lambda g: {"L": g[0], "M": g[1], "mu": g[2], "bx": g[3], "bz": g[4]},
        takes_relax=True, plan="ViscoPlan", state_fields=8, segments_same_bits=False),
}


def module(m):
    return importlib.import_module("physicsbasedfwi2_amd." + m.name)


def pick_lx(ng):
    """The plan's rule for the forward tile width (mifwi::pick_lx in csrc/mifwi_host.h), restated: 64 lanes per row, then
    32, where padding a row of ng four-cell groups to a multiple of that costs at most 20 %; otherwise 16."""
    for cand in (64, 32):
        if -(-ng // cand) * cand * 10 <= ng * 12:
            return cand
    return 16


def _config(spec):
    """(configuration, cache key) of ``spec``: a name of ``CASES``, or a configuration itself - the keywords of
    cases.elastic_case and, optionally, "seed" (83), "source_type" (0; 1 / 2: a point force fx / fz), "ntap" (1) and
    "surface_receivers" (True; False: under a free surface shot 0 is recorded on the buried line of the other shots, not on
    row 0, where its own source's injection is 1e5 times everything the other shots record), "blocks" (none; fluid blocks
    (row0, row1, col0, col1), bounds inclusive, cut into the solid: vs = 0 there, the elastic planes rebuilt from that vs)
    and "src" (elastic_case's; the (row, column) of each shot's one source)."""
    cfg = dict(CASES[spec] if isinstance(spec, str) else spec)
    return cfg, (spec if isinstance(spec, str) else tuple(sorted(cfg.items())))


def width(spec):
    """Lanes per row the plan picks for the case's grid."""
    return pick_lx(-(-_config(spec)[0].get("nx", 60) // 4))


def _four_taps(c, seed):
    """The case's one-tap points as bilinear four-tap points (oracle.helpers.bilinear_taps) at seeded fractional positions
    inside the cells elastic_case chose: every tap active, no weight 0 or 1."""
    nz, nx = c["vp"].shape
    rng = np.random.default_rng([seed, 4])
    for cell, w in (("sc", "sw"), ("rc", "rw")):
        q = np.asarray(c[cell])[..., 0]
        pos = np.stack([q // nx, q % nx], axis=-1) + rng.uniform(0.05, 0.95, q.shape + (2,))
        c[cell], c[w] = H.bilinear_taps(pos * c["h"], (c["h"], c["h"]), 0, (nz, nx))
        assert c[cell].shape == q.shape + (4,) and (c[cell] >= 0).all() and ((c[w] > 0) & (c[w] < 1)).all()
        assert np.array_equal(c[cell][..., 0], q)


def case(m, spec):
    """The elastic case of ``spec`` (a name of ``CASES`` or a configuration, see ``_config``) with its inputs rounded to f32,
    the medium's planes "matm" of smooth seeded fields, its limit "matlim" that must run as the elastic propagator, "relax"
    (None without memory variables), "st", the source type (a force's amplitudes are scaled by 1e-3, as the elastic sweep
    scales them) and seeded 1 % perturbations "dmat" of the planes and "df" of the source amplitudes."""
    cfg, key = _config(spec)
    key = (m.name, key)
    if key not in _cache:
        seed, st, ntap = cfg.pop("seed", 83), cfg.pop("source_type", 0), cfg.pop("ntap", 1)
        on_surface = cfg.pop("surface_receivers", True)
        blocks, src = cfg.pop("blocks", ()), cfg.pop("src", None)
        c = elastic_case(seed=seed, **cfg)
        c["st"], c["blocks"] = st, blocks
        if blocks:
            for r0, r1, c0, c1 in blocks:
                assert WATER <= r0 <= r1 < c["vs"].shape[0] and 0 <= c0 <= c1 < c["vs"].shape[1]
                c["vs"][r0:r1 + 1, c0:c1 + 1] = 0.0
            c["mat"] = H.elastic_materials(c["vp"], c["vs"], c["rho"], c["dt"], c["h"], free_surface=bool(c["fs"]))
        if src is not None:
            assert len(src) == c["sc"].shape[0] and c["sc"].shape[1] == 1
            c["sc"], c["sw"] = H.cell_taps(np.array([[z] for z, _ in src]), np.array([[x] for _, x in src]), c["vp"].shape[1])
        if c["fs"] and not on_surface:
            c["rc"][0], c["rw"][0] = c["rc"][1], c["rw"][1]           # shot 0 recorded on the buried line of the others
        if st:
            c["f"] = c["f"] * 1e-3
        if ntap == 4:
            _four_taps(c, seed)
        nz, nx = c["vp"].shape
        rng = np.random.default_rng(31)
        z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
        ph = 2 * np.pi * rng.random(4)
        s1 = np.sin(2 * np.pi * (1.3 * z + 0.7 * x) + ph[0]) * np.cos(2 * np.pi * 0.9 * x + ph[1])
        s2 = np.sin(2 * np.pi * (0.8 * z - 1.1 * x) + ph[2]) * np.cos(2 * np.pi * 0.6 * z + ph[3])
        assert not c["vs"][:WATER].any()
        c["relax"] = None
        c["matm"] = m.model(c, s1, s2)
        for k in ("mat", "pz", "px", "f", "sw", "rw"):
            c[k] = f32(c[k])
        c["matlim"] = m.limit(c["mat"])
        prng = np.random.default_rng(100)
        c["dmat"] = f32(0.01 * prng.standard_normal(c["matm"].shape) * c["matm"])
        c["df"] = f32(0.01 * prng.standard_normal(c["f"].shape) * np.abs(c["f"]).max())
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def g_of(rvx, rvz):
    """The adjoint source of the gradient tests: seeded noise at the size of each trace set."""
    rng = np.random.default_rng(12)
    return [f32(rng.standard_normal(a.shape) * np.abs(a).max()) for a in (rvx, rvz)]


def geo(c):
    return c["sc"], c["sw"], c["rc"], c["rw"]


def ref(m, spec, order, which):
    """The reference on ``which`` = "matm" / "matlim": traces, the adjoint source built from them, gradients."""
    key = ("ref", m.name, _config(spec)[1], order, which)
    if key not in _cache:
        c = case(m, spec)
        rvx, rvz, gm, gf = R.gradients(c[which], c["pz"], c["px"], c["f"], *geo(c), g_of, None, m.name, c["relax"],
                                       free_surface=c["fs"], fd_order=order, source_type=c["st"])
        out = dict(rvx=rvx, rvz=rvz, g=g_of(rvx, rvz), f=gf, planes=gm)
        out.update({p: gm[k] for k, p in enumerate(m.planes)})
        for v in out.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def ref_jvp(m, spec, order):
    key = ("jvp", m.name, _config(spec)[1], order)
    if key not in _cache:
        c = case(m, spec)
        assert c["st"] == 0                                   # Born modelling serves explosive sources only
        d = R.jvp(c["matm"], c["dmat"], c["pz"], c["px"], c["f"], None, *geo(c), m.name, c["relax"], eps=1e-5,
                  free_surface=c["fs"], fd_order=order)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def dev(a):
    a = np.asarray(a)
    return torch.tensor(a, device="cuda:0", dtype=torch.int32 if a.dtype.kind == "i" else torch.float32)


def args(c, mat, f=None):
    """(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width)"""
    return [mat, dev(c["f"]) if f is None else f] + [dev(c[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")] + [c["fw"]]


def extra(m, c):
    """What the medium's propagate / born / gauss_newton_product take after the pml width."""
    return [F_RELAX, c["dt"]] if m.takes_relax else []


def run(m, c, mat_np, order, g=None, need_f=True, **kw):
    """propagate (+ backward with the adjoint source ``g``) of the medium ``m``, or of the elastic propagator (``m``
    None): traces, grad_mat, grad_f as float64."""
    from physicsbasedfwi2_amd import elastic
    mat = dev(mat_np).requires_grad_(g is not None)
    f = dev(c["f"]).requires_grad_(g is not None and need_f)
    mod, more = (elastic, []) if m is None else (module(m), extra(m, c))
    rvx, rvz = mod.propagate(*args(c, mat, f), *more, free_surface=bool(c["fs"]), fd_order=order, source_type=c["st"], **kw)
    if g is None:
        return rvx, rvz
    torch.autograd.backward([rvx, rvz], [dev(a) for a in g])
    return rvx.detach(), rvz.detach(), mat.grad.double().cpu().numpy(), (f.grad.double().cpu().numpy() if need_f else None)


def born(m, c, order, dmat=None, df=None, **kw):
    a = args(c, dev(c["matm"]))
    return module(m).born(a[0], dev(c["dmat"]) if dmat is None else dmat, *a[1:], *extra(m, c), df=df,
                          free_surface=bool(c["fs"]), fd_order=order, **kw)


def plan(m, c, ns=None, order=4, gs=0):
    """The plan a propagate call on the case creates, for ``ns`` shots (default: the case's); ``m`` None: the elastic
    propagator's.  The caller closes it."""
    from physicsbasedfwi2_amd import elastic
    nz, nx = c["vp"].shape
    nt, n, nsrc = c["f"].shape
    make, relax = (elastic.ElasticPlan, ()) if m is None else (getattr(module(m), m.plan), c["relax"] or ())
    return make(nz, nx, nt, ns or n, nsrc, c["rc"].shape[1], c["rc"].shape[2], c["fw"], 0, *relax, shots_per_group=gs,
                free_surface=c["fs"], source_type=c["st"], fd_order=order)


def step_bytes(m, c, ns=None, order=4, gs=0):
    """Bytes of one time step's snapshots for ``ns`` shots (default: the case's), from the medium's own plan (``m`` None:
    the elastic propagator's, which may run a single-launch loop)."""
    nz, n = c["vp"].shape[0], c["f"].shape[1]
    pl = plan(m, c, ns, order, gs)
    lay = pl.layout
    if m is not None:
        assert pl.cluster_slabs(False) == 0 and pl.cluster_slabs(True) == 0
        if m.state_fields:
            assert lay.state_elems >= m.state_fields * (nz + 4) * lay.pitch * (ns or n)
    b = 4 * lay.snap_step_elems
    pl.close()
    return b


def segment_budget(m, c, segments, order=4, gs=0):
    """The snapshot budget that cuts the case's time range into ``segments`` time-checkpoint segments on the plan of ``m``
    (None: the elastic propagator's): one segment's snapshots and as much again for the checkpoints."""
    from physicsbasedfwi2_amd._driver import checkpoint_schedule, segment_length
    nt = c["f"].shape[0]
    sb = step_bytes(m, c, order=order, gs=gs)
    seg = -(-nt // segments)
    budget = 2 * seg * sb
    assert segment_length(budget, torch.device("cuda:0"), sb, nt) == seg
    assert len(checkpoint_schedule(nt, seg, "elastic")[0]) >= 2
    return budget


def pair(a, b):
    return torch.stack([a, b]).double().cpu().numpy()


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def dot(a, b):
    return float((a.double() * b.double()).sum())


def close(a, b, tol, what):
    print("%s: %.9e vs %.9e, |diff| / max = %.2e" % (what, a, b, abs(a - b) / max(abs(a), abs(b))))
    assert abs(a - b) <= tol * max(abs(a), abs(b)), what


def no_fallback():
    """The body of an autouse fixture: no call of the module may count a fall-back (the counter is the process's: other
    modules move it on purpose)."""
    from physicsbasedfwi2_amd import _lib
    before = _lib.load().mifwi_fallback_count()
    yield
    assert _lib.load().mifwi_fallback_count() == before


# ---- the two tests whose cases keep their names in the media's own files ------------------------------------------------
ISO_KEYS = ("L", "M", "mu", "bx", "bz", "f")


def check_limit_is_the_elastic_propagator(m, monkeypatch, name, form, order):
    """The medium's limit planes run as elastic.propagate: the same trace bits, gradients within TOL_SUM"""
    setenv(monkeypatch, PER_STEP if form == "per_step" else {})
    c = case(m, name)
    g = ref(m, name, order, "matlim")["g"]
    evx, evz, eg, egf = run(None, c, c["mat"], order, g)
    vvx, vvz, vg, vgf = run(m, c, c["matlim"], order, g)
    assert evx.abs().max() > 0 and evz.abs().max() > 0
    assert torch.equal(vvx, evx) and torch.equal(vvz, evz)
    got = dict(m.iso(vg), f=vgf)
    elastic = dict(L=eg[0], M=eg[1], mu=eg[2], bx=eg[3], bz=eg[4], f=egf)
    want = {k: elastic[k] for k in got}
    errs = {k: rel_l2(got[k], want[k]) for k in want}
    print("%s vs elastic gradients rel-L2" % m.limit_label, {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert np.abs(want[k]).max() > 0, k
        assert v <= TOL_SUM, (k, v)


def live_shots(tr, floor):
    """Shots whose traces [2, nt, ns, nrec] hold at least ``floor`` of the largest shot's norm (the wave has not reached the
    receivers of the others: their samples are stencil leakage of size 1e-30, whose ratios mean nothing)."""
    norms = [np.linalg.norm(tr[:, :, s]) for s in range(tr.shape[2])]
    return [s for s, v in enumerate(norms) if v >= floor * max(norms)]


def moved_from_the_limit(m, spec, order, floor=0.0):
    """rel-L2, shot by shot, between the reference's traces in the medium and in its limit, over the live shots"""
    iso, ref_m = ref(m, spec, order, "matlim"), ref(m, spec, order, "matm")
    ref_mtr, iso_tr = np.stack([ref_m["rvx"], ref_m["rvz"]]), np.stack([iso["rvx"], iso["rvz"]])
    return [rel_l2(ref_mtr[:, :, s], iso_tr[:, :, s]) for s in live_shots(ref_mtr, floor)]


def check_traces_and_gradients_match_the_reference(m, name, order, floor=0.0, segments=0, **kw):
    """The medium's traces within TOL_TRACE and every gradient within max(TOL_SUM, 4 E_iso) of the float64 reference.
    ``name``: a name of CASES or a configuration; ``floor``: see live_shots; ``segments`` > 0: that many time-checkpoint
    segments, each propagator's budget from its own plan; ``kw``: further options of both propagate calls.  Returns the
    measured errors {"traces", the planes, "f", "E_iso"} and what the medium's run returned."""
    c = case(m, name)
    iso, ref_m = ref(m, name, order, "matlim"), ref(m, name, order, "matm")
    budget = lambda mm: dict(snapshot_budget=segment_budget(mm, c, segments, order, kw.get("shots_per_group", 0))) if segments else {}
    # today's isotropic kernels against the same reference in the isotropic limit: the case's own error level
    evx, evz, eg, egf = run(None, c, c["mat"], order, iso["g"], **budget(None), **kw)
    e_tr = rel_l2(pair(evx, evz), np.stack([iso["rvx"], iso["rvz"]]))
    iso_g = dict(m.iso(iso["planes"]), f=iso["f"])
    e_iso = {k: rel_l2(e, iso_g[k]) for k, e in zip(ISO_KEYS, list(eg) + [egf])}
    print("E_iso %s order %d: traces %.2e, gradients %s" % (name, order, e_tr, {k: "%.2e" % v for k, v in e_iso.items()}))
    assert e_tr <= TOL_TRACE, "the isotropic kernels miss the trace bound on this case: not a case for this test"
    vvx, vvz, vg, vgf = run(m, c, c["matm"], order, ref_m["g"], **budget(m), **kw)
    assert np.abs(ref_m["rvx"]).max() > 0 and np.abs(ref_m["rvz"]).max() > 0
    ref_mtr, iso_tr, got_tr = np.stack([ref_m["rvx"], ref_m["rvz"]]), np.stack([iso["rvx"], iso["rvz"]]), pair(vvx, vvz)
    shots = range(ref_mtr.shape[2])
    # another medium for real: some shot's traces move by more than a percent.  (Under the free surface shot 0 is shot and
    # recorded on row 0 in the water, whose effective moduli are all zero: its traces never see the medium, are the same
    # bits in both references and carry nearly all the energy of the case, so all shots pooled move by 7e-7 there whatever
    # Q is.)
    moved = moved_from_the_limit(m, name, order, floor)
    print("%s vs elastic reference traces: rel-L2 of the live shots %s, pooled %.2e"
          % (m.name, ["%.2e" % v for v in moved], rel_l2(ref_mtr, iso_tr)))
    assert max(moved) > 0.01
    err = rel_l2(got_tr, ref_mtr)
    print("%s traces vs reference: rel-L2 %.2e, shot by shot %s"
          % (m.name, err, ["%.2e" % rel_l2(got_tr[:, :, s], ref_mtr[:, :, s]) for s in shots]))
    assert err <= TOL_TRACE
    got = dict(zip(m.planes, vg), f=vgf)
    width = max(len(p) for p in m.planes)
    errs = dict(traces=err, E_iso=max(e_iso.values()))
    for k in got:
        want = ref_m[k]
        if k == "c33" and c["fs"]:
            # c33 of the surface row never acts (szz = 0 there): both gradients are 0
            assert not got[k][0].any() and not want[0].any()
            e = rel_l2(got[k][1:], want[1:])
        else:
            e = rel_l2(got[k], want)
        tol = max(TOL_SUM, 4 * e_iso[m.ISO_OF[k]])
        print("gradient %-*s rel-L2 %.2e (bound %.2e)" % (width, k, e, tol))
        assert np.abs(want).max() > 0, k
        assert e <= tol, (k, e, tol)
        errs[k] = e
    return errs, (got_tr, vg, vgf)


def check_forced_width(m, monkeypatch, name, lx, order):
    """MIFWI_EL_LX = ``lx`` on a case whose plan would pick 16 lanes per row: traces, every gradient and Born against the
    same cached references within the same bounds; the largest difference from the 16-lane run is printed, not bounded."""
    c = case(m, name)
    assert width(name) == 16 and lx in (32, 64)
    g = ref(m, name, order, "matm")["g"]
    base = run(m, c, c["matm"], order, g)
    base_born = pair(*born(m, c, order)[2:])
    monkeypatch.setenv("MIFWI_EL_LX", str(lx))
    errs, (tr, vg, vgf) = check_traces_and_gradients_match_the_reference(m, name, order)
    got = pair(*born(m, c, order)[2:])
    want = ref_jvp(m, name, order)
    e_born = rel_l2(got, want)
    print("%s.born at %d lanes vs central difference of the reference, %s order %d: rel-L2 %.3e" % (m.name, lx, name, order, e_born))
    assert np.abs(want).max() > 0
    assert e_born <= TOL_TRACE
    diffs = dict(traces=rel_l2(tr, pair(base[0], base[1])), f=rel_l2(vgf, base[3]), born=rel_l2(got, base_born))
    diffs.update({p: rel_l2(vg[k], base[2][k]) for k, p in enumerate(m.planes)})
    print("%s %s order %d: %d lanes vs 16 lanes, rel-L2 %s, largest %.2e"
          % (m.name, name, order, lx, {k: "%.1e" % v for k, v in diffs.items()}, max(diffs.values())))
    return errs, e_born


# ---- the host modules (no GPU) ----------------------------------------------------------------------------------------
def seeded_model(fourth, fifth, nz=5, nx=6, seed=0, water=1):
    """vp, vs, rho and the medium's two fields, ``fourth`` and ``fifth`` (lo, width) of a uniform draw, as float64 tensors;
    Vs = 0 in the first ``water`` rows."""
    rng = np.random.default_rng(seed)
    vp = 2000 + 1000 * rng.random((nz, nx))
    vs = vp * (0.4 + 0.2 * rng.random((nz, nx)))
    rho = 1800 + 600 * rng.random((nz, nx))
    a = fourth[0] + fourth[1] * rng.random((nz, nx))
    b = fifth[0] + fifth[1] * rng.random((nz, nx))
    vs[:water] = 0.0
    return [torch.tensor(t, dtype=torch.float64) for t in (vp, vs, rho, a, b)]


def check_struct_layouts(structs, tmp_path):
    """ctypes ``structs`` {C name: class} against include/mifwi.h as gcc lays it out: sizes and every field's offset."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mifwi.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
