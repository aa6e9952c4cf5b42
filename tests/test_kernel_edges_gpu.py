"""The small device kernels around the propagators at the inputs where a reduction or a guard goes wrong: the three
misfits (csrc/mifwi_misfit.hip), the gradient conditioning (csrc/mifwi_gradient.hip) and every library entry point on a
caller's stream.  Each kernel against a plain float64 definition of the same operation, computed on the CPU."""
import numpy as np
import pytest
import torch

from oracle import misfit as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24                                    # fp32 unit round-off
SLICES = 16                                       # interleaved time slices of a misfit workgroup (kSl)


# ---- L1 trace-normalised misfit ---------------------------------------------------------------------------------------

def _l1_traces(nt, ntrace, rng, with_direct):
    """d = pred - direct [nt, ntrace] with planted maxima of |d| = 4: ties inside one slice (t, t + 16), across slices,
    with the earlier time in the later slice (17 / 32), at t = nt - 1, and all-zero traces.  With a direct wave every
    value is a small multiple of a power of two, so pred - direct is exact in fp32 and the ties are real there."""
    top = 4.0
    if with_direct:
        d = rng.integers(-63, 64, size=(nt, ntrace)) / 16.0
        direct = (rng.integers(-16, 17, size=(nt, ntrace)) / 8.0).astype(np.float32)
    else:
        d = rng.uniform(-0.98 * top, 0.98 * top, size=(nt, ntrace))
        direct = None
    d = d.astype(np.float32)
    for j in range(ntrace):
        kind = (j + ntrace) % 7
        s1, s2 = rng.choice([-top, top], size=2)
        if kind == 1 and nt > SLICES:                                    # same slice: t, t + 16
            t = int(rng.integers(0, nt - SLICES))
            d[t, j], d[t + SLICES, j] = s1, s2
        elif kind == 2 and nt > 1:                                       # two slices, the earlier time in the earlier slice
            t1 = int(rng.integers(0, nt - 1))
            t2 = int(rng.integers(t1 + 1, nt))
            if t2 % SLICES == t1 % SLICES:
                t2 = t1 + 1
            d[t1, j], d[t2, j] = s1, s2
        elif kind == 3 and nt > SLICES:                                  # the earlier time in a LATER slice
            if nt > 32 and j % 2:
                t1, t2 = 17, 32                                          # slice 0 reports 32, slice 1 reports 17
            else:
                t2 = SLICES * int(rng.integers(1, (nt - 1) // SLICES + 1))
                t1 = int(rng.integers(t2 - SLICES + 1, t2))
            d[t1, j], d[t2, j] = s1, s2
        elif kind == 4:                                                  # the maximum at the last sample
            d[nt - 1, j] = s1
        elif kind == 5:                                                  # an all-zero trace: inv = 1e10
            d[:, j] = 0.0
        elif kind == 6 and nt > 1:                                       # a tie with the last sample
            d[int(rng.integers(0, nt - 1)), j], d[nt - 1, j] = s1, s2
    pred = d if direct is None else (direct + d).astype(np.float32)
    return pred, direct


@pytest.mark.parametrize("with_direct", [False, True])
@pytest.mark.parametrize("nt", [1, 15, 16, 17, 300])
def test_l1_trace_norm_ties_zero_traces_and_ragged_shapes(nt, with_direct):
    """misfit_l1_trace_norm: per-trace max |d| in 16 slices merged with a tie-break on the smallest time; the max's own
    gradient lands on that one sample.  Sample by sample against oracle/misfit.py in float64."""
    from physicsbasedfwi2_amd import misfit
    rng = np.random.default_rng(100 + nt + 7 * with_direct)
    for ntrace in (1, 63, 64, 65, 64 * 3 + 1, 64 * 10 + 1):
        pred, direct = _l1_traces(nt, ntrace, rng, with_direct)
        dd = pred if direct is None else pred - direct                   # fp32, what the kernel sees
        a = np.abs(dd.astype(np.float64))
        arg = a.argmax(axis=0)                                           # the first maximum
        cols = np.arange(ntrace)
        inv = 1.0 / (a[arg, cols] + M.EPS)
        s = rng.choice([-1.0, 1.0], size=(nt, ntrace))
        obs = (dd * inv + s * (0.01 + rng.random((nt, ntrace)))).astype(np.float32)      # |residual| >= 0.01
        lo, ref = M.l1_trace_normalized(dd, obs)
        p = torch.tensor(pred, device=DEV, requires_grad=True)
        loss = misfit.l1_trace_normalized(p, torch.tensor(obs, device=DEV),
                                          None if direct is None else torch.tensor(direct, device=DEV))
        loss.backward()
        got = p.grad.cpu().numpy().astype(np.float64)
        where = "nt=%d ntrace=%d direct=%s" % (nt, ntrace, with_direct)
        assert np.isfinite(got).all(), where
        assert abs(float(loss.detach()) - lo) <= 2e-6 * abs(lo), where
        zero = ref == 0
        assert (got[zero] == 0).all(), where
        at_arg = np.zeros((nt, ntrace), dtype=bool)
        at_arg[arg, cols] = True
        rest = ~at_arg & ~zero
        err = np.abs(got - ref)
        assert (err[rest] <= 1e-6 * np.abs(ref[rest])).all(), (where, float((err[rest] / np.abs(ref[rest])).max()))
        # the argmax sample: the correction there is an fp32 sum over nt samples.  The scale is the trace's largest
        # adjoint magnitude, the argmax's own uncorrected term inv / n included (at nt = 1 the two cancel to ~1e-10)
        base = inv / dd.size
        scale = np.maximum(np.abs(ref).max(axis=0), base)
        tol = max(2e-5, 4 * nt * U) * scale
        assert (err[arg, cols] <= tol).all(), (where, float((err[arg, cols] / scale).max()))
        # ... and it lands on the sample the reference puts it on (the first of tied maxima)
        r = dd.astype(np.float64) * inv - obs
        plain = np.sign(r) / dd.size * inv                               # the adjoint without the max's gradient
        moved = np.abs(got - plain).argmax(axis=0)
        seen = np.abs(ref[arg, cols] - plain[arg, cols]) > 100 * tol     # corrections well above round-off
        assert np.array_equal(moved[seen], arg[seen]), where
        if nt > 1:
            assert seen.sum() >= ntrace // 2, where                      # the check above is not vacuous


# ---- L2 misfit --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 4 * 257 + 3, 2_100_003])
def test_l2_misfit_sizes_and_misaligned_views(n):
    """misfit_l2 reads float4 where pred, obs and adj are 16-byte aligned and one float at a time otherwise (decided in
    mifwi_misfit): views with storage offsets of 1, 2, 3 floats, tails shorter than 4, and n > 2048 x 256 x 4 (the
    grid-stride loop wraps).  The adjoint is one fp32 subtraction: torch's pred - obs bit for bit."""
    from physicsbasedfwi2_amd import _lib, misfit
    rng = np.random.default_rng(n % 1000)
    bp = torch.tensor(rng.standard_normal(n + 4).astype(np.float32), device=DEV)
    bo = torch.tensor(rng.standard_normal(n + 4).astype(np.float32), device=DEV)
    for op, oo in ((0, 0), (1, 0), (0, 2), (3, 3), (2, 1)):
        pred, obs = bp[op:op + n].view(n, 1), bo[oo:oo + n].view(n, 1)
        assert pred.is_contiguous() and pred.storage_offset() == op and obs.storage_offset() == oo
        p = pred.detach().requires_grad_(True)
        loss = misfit.l2_half(p, obs)
        loss.backward()
        lo, _ = M.l2_half(pred.cpu().numpy(), obs.cpu().numpy())
        assert abs(float(loss.detach()) - lo) <= 1e-6 * lo, (n, op, oo)
        assert torch.equal(p.grad, pred - obs), (n, op, oo)
    # an adjoint buffer that is itself only 4-byte aligned, through the C entry point; nothing written outside it
    lib = _lib.load()
    pred, obs = bp[1:1 + n].view(n, 1), bo[:n].view(n, 1)
    out = torch.full((n + 2,), float("nan"), device=DEV)
    adj = out[1:n + 1]
    loss = torch.empty((), device=DEV)
    work = torch.empty(lib.mifwi_misfit_work_elems(_lib.MISFIT_L2, n, 1), device=DEV)
    _lib.check(lib.mifwi_misfit(0, _lib.MISFIT_L2, _lib.ptr(pred), _lib.ptr(obs), None, n, 1, _lib.ptr(loss),
                                _lib.ptr(adj), _lib.ptr(work), torch.cuda.current_stream().cuda_stream))
    assert torch.equal(adj, (pred - obs).view(-1))
    assert bool(out[0].isnan()) and bool(out[-1].isnan())


# ---- global correlation -----------------------------------------------------------------------------------------------

def _gc_check(pred, obs, where):
    from physicsbasedfwi2_amd import misfit
    p = torch.tensor(pred, device=DEV, requires_grad=True)
    loss = misfit.global_correlation(p, torch.tensor(obs, device=DEV))
    loss.backward()
    lo, ref = M.global_correlation(pred, obs)
    got = p.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), where
    assert abs(float(loss.detach()) - lo) <= 1e-5 * abs(lo), where
    nt = pred.shape[0]
    g2, r2 = got.reshape(nt, -1), ref.reshape(nt, -1)
    dead = (np.abs(pred.reshape(nt, -1)).max(0) == 0) | (np.abs(obs.reshape(nt, -1)).max(0) == 0)
    assert (g2[:, dead] == 0).all(), where
    if nt == 1:
        # a one-sample trace is always perfectly (anti-)correlated: the two terms of the adjoint cancel; both sides agree
        # to the existing tolerance of the terms' size 1 / |s|
        s = np.abs(pred.reshape(1, -1).astype(np.float64))
        live = ~dead
        assert (np.abs(g2 - r2)[:, live] <= 1e-5 / s[:, live]).all(), where
    else:
        # per trace, so that a weak trace (adjoint ~1e30) does not hide the others
        live = np.flatnonzero(~dead)
        e = np.linalg.norm(g2[:, live] - r2[:, live], axis=0) / np.linalg.norm(r2[:, live], axis=0)
        assert (e <= 1e-5).all(), (where, float(e.max()))


def test_global_correlation_edges():
    """misfit_gc: nt = 1, a trace with |pred| ~ 1e-30 (its two coefficients overflow a float: the double
    path), and dead traces on either side for every trace count remainder modulo the 64-trace workgroup."""
    rng = np.random.default_rng(41)
    for nt in (1, 37):
        ntrace = 70
        pred = (rng.standard_normal((nt, ntrace)) * (0.5 + rng.random(ntrace))).astype(np.float32)
        obs = (0.7 * pred + 0.5 * rng.standard_normal((nt, ntrace))).astype(np.float32)
        pred[:, 3] *= np.float32(1e-30)                               # weak predicted trace
        obs[:, 9] *= np.float32(1e-30)                                # weak observed trace
        pred[:, 66] = 0.0
        obs[:, 67] = 0.0
        _gc_check(pred, obs, "nt=%d weak traces" % nt)
    for rem in range(64):
        ntrace = 64 + rem
        nt = 37
        pred = rng.standard_normal((nt, ntrace)).astype(np.float32)
        obs = (0.6 * pred + 0.6 * rng.standard_normal((nt, ntrace))).astype(np.float32)
        pred[:, ntrace - 1] = 0.0                                      # the last trace, in the partial workgroup
        obs[:, (ntrace - 2) if ntrace > 64 else 0] = 0.0
        pred[:, 63] = 0.0                                              # the last lane of the first workgroup
        _gc_check(pred, obs, "ntrace=%d" % ntrace)


# ---- gradient conditioning --------------------------------------------------------------------------------------------

def _condition_ref(g, m, w, sigma, flip, mute, fac):
    """networks.py:7808-7862 / 10522-10540 in numpy / scipy, float64 after the fp32 depth weight."""
    from scipy.ndimage import gaussian_filter
    out = []
    for k in range(g.shape[0]):
        t = g[k] if w is None else (g[k] * w[:, None]).astype(np.float32)
        t = (np.flipud(t) if flip else t).astype(np.float64)
        if sigma > 0:
            t = gaussian_filter(t, sigma=sigma)
        t = t.copy()
        t[0:mute] = 0.0
        scale = fac[k] * (np.max(m[k]) / np.max(t)) if m is not None else fac[k]
        out.append(t * scale)
    return out


@pytest.mark.parametrize("sigma", [0.0, 0.1, 1.3, 7.9])
def test_gradient_conditioning_small_grids_and_large_radii(sigma):
    """grad_condition on grids smaller than a 32 x 64 tile and than the Gaussian radius (scipy's 'reflect' folds more
    than once), R = 0 with sigma > 0, R = 32 (sigma 7.9, the largest served), 1 and 4 planes, flip with and without a
    depth weight, with and without models, a non-contiguous gradient.  <= 2e-5 of each plane's largest magnitude."""
    from physicsbasedfwi2_amd import conditioning as C
    rng = np.random.default_rng(int(sigma * 10) + 3)
    i = 0
    for nz in (1, 2, 3, 31, 32, 33):
        for nx in (1, 63, 64, 65, 129):
            k = 1 if i % 2 == 0 else 4
            flip = i % 3 != 0
            w = (0.5 + rng.random(nz)).astype(np.float32) if (i // 2) % 2 == 0 else None
            mute = min(2, nz - 1) if i % 4 == 1 else 0
            fac = (0.5,) if k == 1 else (1.0, 0.5, 0.1, 2.0)
            g = (1.0 + 0.5 * rng.standard_normal((k, nz, nx))).astype(np.float32)
            m = None if i % 5 == 0 else (500.0 + 1000.0 * rng.random((k, nz, nx))).astype(np.float32)
            if i % 3 == 1:                                             # columns 1 .. nx of a wider array
                wide = torch.zeros((k, nz, nx + 3), device=DEV)
                wide[:, :, 1:nx + 1] = torch.tensor(g, device=DEV)
                gt = wide[:, :, 1:nx + 1]
                assert gt.is_contiguous() == (k * nz == 1)
            else:
                gt = torch.tensor(g, device=DEV)
            out = C.condition_gradients(gt, None if m is None else torch.tensor(m, device=DEV),
                                        None if w is None else torch.tensor(w), sigma, flip, mute, fac)
            o = out.cpu().numpy()
            ref = _condition_ref(g, m, w, sigma, flip, mute, fac)
            where = (nz, nx, k, flip, w is not None, mute, m is not None)
            for q in range(k):
                assert np.abs(o[q] - ref[q]).max() <= 2e-5 * np.abs(ref[q]).max(), (where, q)
                assert (o[q][:mute] == 0).all(), (where, q)
            i += 1


def test_gradient_conditioning_negative_plane_and_the_radius_limit():
    """The max ratio uses the plain maximum (np.max), through an order-preserving key: a plane that is negative
    everywhere scales by its negative maximum, the value closest to 0 - not by its largest magnitude.  No mute band
    (it would make the maximum 0).  R = 33 (sigma 8.125) is refused."""
    from physicsbasedfwi2_amd import conditioning as C
    from physicsbasedfwi2_amd._lib import MifwiError
    rng = np.random.default_rng(77)
    nz, nx = 33, 65
    for sigma in (0.0, 1.3):
        for flip in (False, True):
            g = rng.standard_normal((2, nz, nx)).astype(np.float32)
            g[0] = -(1.0 + np.abs(g[0]))                               # negative everywhere, bounded away from 0
            m = (500.0 + 1000.0 * rng.random((2, nz, nx))).astype(np.float32)
            fac = (1.0, 0.1)
            out = C.condition_gradients(torch.tensor(g, device=DEV), torch.tensor(m, device=DEV), None, sigma, flip, 0,
                                        fac).cpu().numpy()
            ref = _condition_ref(g, m, None, sigma, flip, 0, fac)
            for q in range(2):
                assert np.abs(out[q] - ref[q]).max() <= 2e-5 * np.abs(ref[q]).max(), (sigma, flip, q)
            assert (out[0] > 0).all()                                  # negative plane / negative maximum
    g = torch.zeros((1, 8, 8), device=DEV)
    C.condition_gradients(g, sigma=7.9)                                # R = 32: served
    with pytest.raises(MifwiError):
        C.condition_gradients(g, sigma=8.125)                          # R = 33: refused


# ---- every entry point on the caller's stream ------------------------------------------------------------------------

def _stream_calls():
    """(name, environment, function of the device inputs, device inputs): each function returns the tensors to compare."""
    from cases import acoustic_case, elastic_case
    from oracle import helpers as H
    from physicsbasedfwi2_amd import acoustic, conditioning, elastic, misfit
    from physicsbasedfwi2_amd.compat.deepwave import scalar
    rng = np.random.default_rng(9)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)
    calls = []

    def l1(p, o, d):
        p = p.requires_grad_(True)
        loss = misfit.l1_trace_normalized(p, o, d)
        loss.backward()
        return loss.detach(), p.grad

    def l2(p, o):
        p = p.requires_grad_(True)
        loss = misfit.l2_half(p, o)
        loss.backward()
        return loss.detach(), p.grad

    def gc(p, o):
        p = p.requires_grad_(True)
        loss = misfit.global_correlation(p, o)
        loss.backward()
        return loss.detach(), p.grad

    shape = (130, 3, 45)
    calls.append(("misfit L1", {}, l1, [t(rng.standard_normal(shape)), t(rng.standard_normal(shape)),
                                        t(0.3 * rng.standard_normal(shape))]))
    calls.append(("misfit L2", {}, l2, [t(rng.standard_normal(shape)), t(rng.standard_normal(shape))]))
    calls.append(("misfit GC", {}, gc, [t(rng.standard_normal(shape)), t(rng.standard_normal(shape))]))
    calls.append(("conditioning", {},
                  lambda g, m, w: (conditioning.condition_gradients(g, m, w, 1.3, True, 2, (1.0, 1.0, 0.1)),),
                  [t(rng.standard_normal((3, 40, 70))), t(500 + 1000 * rng.random((3, 40, 70))), t(0.5 + rng.random(40))]))
    nz, nx = 37, 53
    vp = 1500.0 + 2500.0 * rng.random((nz, nx))
    vs = vp / 1.8
    vs[:3] = 0.0
    rho = 1000.0 + 1500.0 * rng.random((nz, nx))

    def materials(a, b, c, g):
        a, b, c = (x.requires_grad_(True) for x in (a, b, c))
        out = elastic.staggered_materials(a, b, c, 2e-3, 20.0, free_surface=True)
        out.backward(g)
        return out.detach(), a.grad, b.grad, c.grad

    calls.append(("materials", {}, materials, [t(vp), t(vs), t(rho), t(rng.standard_normal((5, nz, nx)))]))
    for mode in (elastic.PARAM_IMPEDANCE, elastic.PARAM_LAME):
        calls.append(("INVMAT1=%d" % mode, {},
                      lambda a, b, c, ga, gb, gc_, mode=mode: elastic.gradient_parametrization((a, b, c), (ga, gb, gc_), mode),
                      [t(vp), t(vs), t(rho)] + [t(rng.standard_normal((nz, nx))) for _ in range(3)]))

    def coefficients(v, g):
        v = v.requires_grad_(True)
        r = scalar._Coefficients.apply(v, 6, 1e-4)
        r.backward(g)
        return r.detach(), v.grad

    calls.append(("acoustic coefficients", {}, coefficients, [t(vp), t(rng.standard_normal((nz + 12, nx + 12)))]))

    ac = acoustic_case(seed=19, n0=48, n1=70, nb=8, nt=60, ns=2, nrec=11)
    cp = acoustic_case(seed=5, n0=40, n1=56, nb=8, nt=60, ns=2, nrec=9)
    N0, N1 = cp["shape"]
    vmax = float(cp["vp"].max())
    ab0 = torch.tensor(H.cpml_profiles(N0, 8, 10.0, cp["s"], vmax, 0.02)[:2])
    ab1 = torch.tensor(H.cpml_profiles(N1, 8, 10.0, cp["s"], vmax, 0.02)[:2])

    def acoustic_run(c, q0, q1, **kw):
        def run(r, f, sc, sw, rc, rw, g):
            r, f = r.requires_grad_(True), f.requires_grad_(True)
            rec = acoustic.propagate(r, f, q0, q1, sc, sw, rc, rw, c["c0"], c["c1"], **kw)
            rec.backward(g)
            return rec.detach(), r.grad, f.grad
        return run

    def geom(c, nt, ns, nrec):
        return [t(c["r"]), t(c["f"]), torch.tensor(c["sc"], device=DEV), t(c["sw"]), torch.tensor(c["rc"], device=DEV),
                t(c["rw"]), t(rng.standard_normal((nt, ns, nrec)))]

    for fam in ("1", "0"):
        calls.append(("acoustic sponge MIFWI_AC_CLUSTER=" + fam, {"MIFWI_AC_CLUSTER": fam},
                      acoustic_run(ac, torch.tensor(ac["q0"]), torch.tensor(ac["q1"])), geom(ac, 60, 2, 11)))
    calls.append(("acoustic C-PML", {}, acoustic_run(cp, ab0, ab1, cpml_width=8), geom(cp, 60, 2, 9)))

    ec = elastic_case(seed=4, nz=44, nx=60, fw=8, nt=70, ns=2, nrec=9)

    def elastic_run(mat, f, sc, sw, rc, rw, gx, gz):
        mat, f = mat.requires_grad_(True), f.requires_grad_(True)
        rvx, rvz = elastic.propagate(mat, f, torch.tensor(ec["pz"]), torch.tensor(ec["px"]), sc, sw, rc, rw, ec["fw"])
        torch.autograd.backward([rvx, rvz], [gx, gz])
        return rvx.detach(), rvz.detach(), mat.grad, f.grad

    for env in ({}, {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0"},
                {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_FUSED": "1"}):
        calls.append(("elastic %s" % env, env, elastic_run,
                      [t(ec["mat"]), t(ec["f"]), torch.tensor(ec["sc"], device=DEV), t(ec["sw"]),
                       torch.tensor(ec["rc"], device=DEV), t(ec["rw"])] + [t(rng.standard_normal((70, 2, 9))) for _ in range(2)]))

    # the fluid family: the source's bounding box, the per-tile receiver lists, the pressure receivers and their adjoint, the
    # point-force sampling and the finalize are launches of their own beside the four of a step
    from cases import fluid_planes
    from physicsbasedfwi2_amd import fluid
    fc = fluid_planes(elastic_case(seed=6, nz=37, nx=53, fw=6, nt=60, ns=2, nrec=9, water=0), 0)

    def fluid_run(kind):
        def run(mat, f, sc, sw, rc, rw, gx, gz, gp):
            mat, f = mat.requires_grad_(True), f.requires_grad_(True)
            out = fluid.propagate(mat, f, torch.tensor(fc["pz"]), torch.tensor(fc["px"]), sc, sw, rc, rw, fc["fw"],
                                  source_type=kind, record_pressure=True)
            torch.autograd.backward(list(out), [gx, gz, gp])
            return tuple(a.detach() for a in out) + (mat.grad, f.grad)
        return run

    for kind in ("explosive", "fx"):
        calls.append(("fluid " + kind, {}, fluid_run(kind),
                      [t(fc["mat3"]), t(fc["f"]), torch.tensor(fc["sc"], device=DEV), t(fc["sw"]),
                       torch.tensor(fc["rc"], device=DEV), t(fc["rw"])] + [t(rng.standard_normal((60, 2, 9))) for _ in range(3)]))
    return calls


def test_every_entry_point_runs_on_the_callers_stream(monkeypatch):
    """Each entry point on a fresh torch.cuda.Stream(), its inputs produced on that stream right before the call: first
    poisoned (NaN, or -1 = inactive tap), then a spin, then the copy.  A launch or a memset on another stream would read
    the poison.  Every output the same bits as on the default stream."""
    for name, env, fn, inputs in _stream_calls():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ref = [x.clone() for x in fn(*[x.clone() for x in inputs])]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            xs = [torch.full_like(x, float("nan") if x.is_floating_point() else -1) for x in inputs]
            torch.cuda._sleep(2_000_000)
            for x, y in zip(xs, inputs):
                x.copy_(y)
            got = [x.clone() for x in fn(*xs)]
        torch.cuda.synchronize()
        for k in env:
            monkeypatch.delenv(k)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert torch.equal(a, b), name
