"""Stage-filtered misfit kernels (csrc/mifwi_misfit_filter.h) against scipy in float64, computed here from the same float32
inputs:  F = sosfilt(sos, ., axis=0),  F^T z = sosfilt(sos, z[::-1], axis=0)[::-1],  the misfit formulas of oracle/misfit.py
re-evaluated on the filtered arrays.

Shapes cross every seam of the kernel: ntrace 1 / 63 / 65 / 130 (a partial wave, a wave boundary, more than two waves) and
nt 1 / 15 / 17 / 301 around the kernel's chunk of 16 rows requested ahead (shorter than one chunk, one past, not a multiple).
Every trace has its own amplitude between 1e-6 and 1e2, and every bound is per trace.

Tolerances (eps = 2^-24, one float rounding):
  filter            |y - ref| <= 2 eps max_t |ref|                      the output rounding, doubled
  dot product       |<Fx, y> - <x, F^T y>| <= 4 eps sum |Fx||y|         both sides from the kernel's float outputs, all traces;
                    per trace <= 2 eps (sum |Fx||y| + sum |x||F^T y|)    each side's own output rounding, doubled
  L2 adjoint source |adj - ref| <= 2 (1 + |h|_1) eps max_t |r|          one rounding of the stored r carried through F^T
                                                                        (|h|_1: absolute sum of the impulse response over nt
                                                                        samples, 1.5 ... 2.6 here) plus the output rounding
  global correlation the same with max|r| -> |ka| max|F obs| + |kb| max|F pred|, ka, kb from the float64 comparator
  losses            L2 relative 1e-6; global correlation absolute 1e-6 per trace
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import signal

from physicsbasedfwi2_amd import _lib, misfit
from physicsbasedfwi2_amd._lib import MifwiError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
STAGES = [(0.002, 0.0, 10.0, 6), (0.0025, 2.0, 12.0, 6), (0.002, 3.0, 10.0, 6)]      # networks.py:7761, 9863, 10503
NTS = (1, 15, 17, 301)
NTRACES = (1, 63, 65, 130)
SHAPES = [(nt, ntr) for nt in NTS for ntr in NTRACES]


def _dev():
    return torch.device("cuda:0")


def F(sos, a):
    return signal.sosfilt(sos, a, axis=0)


def FT(sos, a):
    return signal.sosfilt(sos, a[::-1], axis=0)[::-1]


def _traces(seed, nt, ntrace):
    """float32 [nt, ntrace], per-trace amplitudes spread over 1e-6 ... 1e2"""
    rng = np.random.default_rng(seed)
    amp = 10.0 ** rng.uniform(-6.0, 2.0, ntrace)
    return (rng.standard_normal((nt, ntrace)) * amp).astype(np.float32), amp


@pytest.fixture(scope="module")
def cases():
    """inputs and float64 references, computed once: cases[(stage index, nt, ntrace)]"""
    out = {}
    for si, (dt, lo, hi, order) in enumerate(STAGES):
        sos = misfit.butterworth_sos(dt, lo, hi, order)
        for nt, ntr in SHAPES:
            x, amp = _traces(1000 * si + 10 * nt + ntr, nt, ntr)
            y, _ = _traces(7 + 1000 * si + 10 * nt + ntr, nt, ntr)
            rng = np.random.default_rng(nt + ntr)
            obs = (0.7 * x + 0.5 * amp * rng.standard_normal((nt, ntr))).astype(np.float32)     # partly correlated
            spike = np.zeros(nt)
            spike[0] = 1.0
            out[si, nt, ntr] = dict(sos=sos, x=x, y=y, obs=obs, h1=float(np.abs(F(sos, spike)).sum()),
                                    Fx=F(sos, x.astype(np.float64)), FTy=FT(sos, y.astype(np.float64)))
    return out


def _gpu(a):
    return torch.tensor(a, device=_dev())


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _filter_inplace(x, sos, transpose):
    lib = _lib.load()
    buf = x.clone()
    nt = buf.shape[0]
    _lib.check(lib.mifwi_trace_filter(0, _lib.ptr(buf), _lib.ptr(buf), nt, buf.numel() // nt,
                                      sos.ctypes.data_as(ctypes.c_void_p), sos.shape[0], int(transpose),
                                      torch.cuda.current_stream().cuda_stream))
    return buf


@pytest.mark.parametrize("si", range(len(STAGES)))
def test_trace_filter_and_transpose_match_sosfilt(cases, si):
    for nt, ntr in SHAPES:
        c = cases[si, nt, ntr]
        for transpose, src, ref in ((False, c["x"], c["Fx"]), (True, c["y"], c["FTy"])):
            xg = _gpu(src)
            out = misfit.trace_filter(xg, c["sos"], transpose=transpose)
            assert out.shape == xg.shape and out.dtype == torch.float32
            err = np.abs(_np(out) - ref).max(axis=0)
            bound = 2.0 * EPS * np.abs(ref).max(axis=0)
            print("stage %d nt %d ntrace %d transpose %d: worst err/bound %.3f" % (si, nt, ntr, transpose,
                                                                                  (err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (si, nt, ntr, transpose)
            assert torch.equal(_filter_inplace(xg, c["sos"], transpose), out)          # y == x: the same bits


@pytest.mark.parametrize("si", range(len(STAGES)))
def test_dot_product(cases, si):
    for nt, ntr in SHAPES:
        c = cases[si, nt, ntr]
        Fx = _np(misfit.trace_filter(_gpu(c["x"]), c["sos"]))
        FTy = _np(misfit.trace_filter(_gpu(c["y"]), c["sos"], transpose=True))
        x, y = c["x"].astype(np.float64), c["y"].astype(np.float64)
        lhs, rhs = (Fx * y).sum(axis=0), (x * FTy).sum(axis=0)                          # per trace
        left, right = (np.abs(Fx) * np.abs(y)).sum(axis=0), (np.abs(x) * np.abs(FTy)).sum(axis=0)
        # all traces together, the bound as stated: 4 eps sum |Fx||y|
        print("stage %d nt %d ntrace %d: |lhs - rhs| / (4 eps sum |Fx||y|) = %.3f; per trace, worst |lhs - rhs| / "
              "(2 eps (sum |Fx||y| + sum |x||F^T y|)) = %.3f"
              % (si, nt, ntr, abs(lhs.sum() - rhs.sum()) / (4.0 * EPS * left.sum()),
                 (np.abs(lhs - rhs) / np.maximum(2.0 * EPS * (left + right), 1e-300)).max()))
        assert abs(lhs.sum() - rhs.sum()) <= 4.0 * EPS * left.sum(), (si, nt, ntr)
        # per trace, each side within its own output rounding (eps per sample of Fx on the left, of F^T y on the right),
        # doubled.  The right-hand sum is not bounded by the left-hand one: a low-pass over a trace shorter than its rise
        # puts all of sum |Fx||y| into the last samples
        assert np.all(np.abs(lhs - rhs) <= 2.0 * EPS * (left + right)), (si, nt, ntr)


def _l2(pred, obs, sos, grad=True):
    p = pred.clone().requires_grad_(grad)
    loss = misfit.l2_half(p, obs, sos=sos)
    if grad:
        loss.backward()
    return loss.detach(), p.grad


def _l2_check(c, pred_g, obs_g, tag):
    pred, obs = _np(pred_g), _np(obs_g)
    nt = pred.shape[0]
    r = F(c["sos"], pred - obs)
    loss_ref, adj_ref = 0.5 * (r * r).sum(), FT(c["sos"], r)
    loss, adj = _l2(pred_g, obs_g, c["sos"])
    assert adj.shape == pred_g.shape
    err = np.abs(_np(adj) - adj_ref).reshape(nt, -1).max(axis=0)
    bound = 2.0 * (1.0 + c["h1"]) * EPS * np.abs(r).reshape(nt, -1).max(axis=0)
    print("%s: loss rel err %.2e, adjoint worst err/bound %.3f" % (tag, abs(float(loss) - loss_ref) / loss_ref,
                                                                    (err / np.maximum(bound, 1e-300)).max()))
    assert abs(float(loss) - loss_ref) <= 1e-6 * loss_ref, tag
    assert np.all(err <= bound), tag
    return loss, adj


@pytest.mark.parametrize("si", range(len(STAGES)))
def test_filtered_l2(cases, si):
    for nt, ntr in SHAPES:
        c = cases[si, nt, ntr]
        pg, og = _gpu(c["x"]), _gpu(c["obs"])
        loss, adj = _l2_check(c, pg, og, "stage %d nt %d ntrace %d" % (si, nt, ntr))
        # no adjoint source asked for: the same loss, bit for bit; a second call: the same bits all over
        assert torch.equal(_l2(pg, og, c["sos"], grad=False)[0], loss)
        loss2, adj2 = _l2(pg, og, c["sos"])
        assert torch.equal(loss2, loss) and torch.equal(adj2, adj)


def test_filtered_l2_3d_and_unaligned_views(cases):
    c = cases[1, 301, 130]
    # [nt, ns, nrec]
    pg, og = _gpu(c["x"]).view(301, 5, 26), _gpu(c["obs"]).view(301, 5, 26)
    loss3, adj3 = _l2_check(c, pg, og, "3-D")
    loss2, adj2 = _l2(pg.view(301, 130), og.view(301, 130), c["sos"])
    assert torch.equal(loss3, loss2) and torch.equal(adj3.view(301, 130), adj2)
    # a contiguous view that is only 4-byte aligned
    buf = torch.empty(301 * 130 + 1, device=_dev())
    pv = buf[1:].view(301, 130)
    pv.copy_(_gpu(c["x"]))
    assert pv.data_ptr() % 8 == 4
    lossv, adjv = _l2(pv, og.view(301, 130), c["sos"])
    assert torch.equal(lossv, loss2) and torch.equal(adjv, adj2)
    assert torch.equal(misfit.trace_filter(pv, c["sos"]), misfit.trace_filter(_gpu(c["x"]), c["sos"]))
    f3 = misfit.trace_filter(pg, c["sos"], transpose=True)
    assert f3.shape == pg.shape and torch.equal(f3.view(301, 130), misfit.trace_filter(_gpu(c["x"]), c["sos"], transpose=True))


@pytest.mark.parametrize("si", range(len(STAGES)))
def test_filtered_global_correlation(cases, si):
    for nt, ntr in SHAPES:
        c = cases[si, nt, ntr]
        pred, obs = c["x"].copy(), c["obs"].copy()
        if ntr >= 3:
            pred[:, 1] = 0.0                    # a dead modelled trace and a dead observed one among the others
            obs[:, ntr - 1] = 0.0
        sos = c["sos"]
        s, o = F(sos, pred.astype(np.float64)), F(sos, obs.astype(np.float64))
        ss, oo, so = (s * s).sum(0), (o * o).sum(0), (s * o).sum(0)
        ok = (ss > 0) & (oo > 0)
        den = np.where(ok, np.sqrt(ss) * np.sqrt(oo), 1.0)
        cc = np.where(ok, so / den, 0.0)
        ka, kb = np.where(ok, -1.0 / den, 0.0), np.where(ok, cc / np.where(ok, ss, 1.0), 0.0)
        loss_ref, adj_ref = -cc.sum(), FT(sos, ka * o + kb * s)
        pg, og = _gpu(pred).requires_grad_(True), _gpu(obs)
        loss = misfit.global_correlation(pg, og, sos=sos)
        loss.backward()
        err = np.abs(_np(pg.grad) - adj_ref).max(axis=0)
        bound = 2.0 * (1.0 + c["h1"]) * EPS * (np.abs(ka) * np.abs(o).max(axis=0) + np.abs(kb) * np.abs(s).max(axis=0))
        print("stage %d nt %d ntrace %d: loss abs err per trace %.2e, adjoint worst err/bound %.3f"
              % (si, nt, ntr, abs(float(loss.detach()) - loss_ref) / ntr, (err[ok] / bound[ok]).max() if ok.any() else 0.0))
        assert abs(float(loss.detach()) - loss_ref) <= 1e-6 * ntr, (si, nt, ntr)
        assert np.all(err <= bound), (si, nt, ntr)
        if ntr >= 3:
            assert not ok[1] and not ok[ntr - 1]
            assert bool((pg.grad[:, 1] == 0).all()) and bool((pg.grad[:, ntr - 1] == 0).all())      # exactly zero
        # loss only: the same bits; twice: the same bits
        assert torch.equal(misfit.global_correlation(pg.detach(), og, sos=sos), loss.detach())
        p2 = _gpu(pred).requires_grad_(True)
        l2 = misfit.global_correlation(p2, og, sos=sos)
        l2.backward()
        assert torch.equal(l2.detach(), loss.detach()) and torch.equal(p2.grad, pg.grad)


def test_autograd(cases):
    c = cases[1, 301, 65]
    sos = c["sos"]
    pg, og = _gpu(c["x"]), _gpu(c["obs"])
    loss, adj = _l2(pg, og, sos)
    p3 = pg.clone().requires_grad_(True)
    og3 = og.clone().requires_grad_(True)
    l3 = 3.0 * misfit.l2_half(p3, og3, sos=sos)
    l3.backward()
    assert torch.equal(p3.grad, 3.0 * adj) and og3.grad is None                     # obs gets no gradient
    assert torch.equal(misfit.l2_half(pg, og, sos=sos), loss)                        # requires_grad = False: the same bits
    assert not misfit.l2_half(pg, og, sos=sos).requires_grad
    # sos = None is the unfiltered path
    assert torch.equal(misfit.l2_half(pg, og, sos=None), misfit.l2_half(pg, og))
    # trace_filter back-propagates F^T (and its transpose back-propagates F)
    w = _gpu(c["y"])
    x = pg.clone().requires_grad_(True)
    (misfit.trace_filter(x, sos) * w).sum().backward()
    assert torch.equal(x.grad, misfit.trace_filter(w, sos, transpose=True))
    x = pg.clone().requires_grad_(True)
    (misfit.trace_filter(x, sos, transpose=True) * w).sum().backward()
    assert torch.equal(x.grad, misfit.trace_filter(w, sos))


def test_invalid_arguments_raise_with_a_message(cases):
    lib = _lib.load()
    c = cases[1, 17, 65]
    nt, ntr = 17, 65
    good = c["sos"]
    x, o = _gpu(c["x"]), _gpu(c["obs"])
    y, loss = torch.empty_like(x), torch.empty((), device=_dev())
    work = torch.empty(lib.mifwi_misfit_filtered_work_elems(_lib.MISFIT_GLOBAL_CORRELATION, nt, ntr) + 2, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    sp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def bad(a, j, v):
        b = a.copy()
        b[0, j] = v
        return b

    def filt(xp=P(x), yp=P(y), nt_=nt, ntr_=ntr, sos=good, nsec=None, sosp=True):
        return lib.mifwi_trace_filter(0, xp, yp, nt_, ntr_, sp(sos) if sosp else None, sos.shape[0] if nsec is None else nsec,
                                      0, st)

    def fused(kind=_lib.MISFIT_L2, pp=P(x), op=P(o), nt_=nt, ntr_=ntr, sos=good, nsec=None, sosp=True, lp=P(loss), wp=P(work)):
        return lib.mifwi_misfit_filtered(0, kind, pp, op, nt_, ntr_, sp(sos) if sosp else None,
                                         sos.shape[0] if nsec is None else nsec, lp, P(y), wp, st)

    assert filt() == 0 and fused() == 0 and fused(kind=_lib.MISFIT_GLOBAL_CORRELATION) == 0
    nine = np.concatenate([good, good])[:9].copy()
    calls = {
        "filter: null x": lambda: filt(xp=None), "filter: null y": lambda: filt(yp=None),
        "filter: null sos": lambda: filt(sosp=False),
        "filter: nsec 0": lambda: filt(nsec=0), "filter: nsec 9": lambda: filt(sos=nine),
        "filter: a0": lambda: filt(sos=bad(good, 3, 2.0)), "filter: nan": lambda: filt(sos=bad(good, 1, np.nan)),
        "filter: inf": lambda: filt(sos=bad(good, 5, np.inf)),
        "filter: nt 0": lambda: filt(nt_=0), "filter: ntrace 0": lambda: filt(ntr_=0), "filter: nt 2^31": lambda: filt(nt_=2 ** 31),
        "fused: null pred": lambda: fused(pp=None), "fused: null obs": lambda: fused(op=None),
        "fused: null sos": lambda: fused(sosp=False), "fused: null loss": lambda: fused(lp=None),
        "fused: null work": lambda: fused(wp=None),
        "fused: nsec 0": lambda: fused(nsec=0), "fused: nsec 9": lambda: fused(sos=nine),
        "fused: a0": lambda: fused(sos=bad(good, 3, 0.5)), "fused: nan": lambda: fused(sos=bad(good, 0, np.nan)),
        "fused: L1": lambda: fused(kind=_lib.MISFIT_L1_TRACE_NORM), "fused: kind 7": lambda: fused(kind=7),
        "fused: work alignment": lambda: fused(wp=ctypes.c_void_p(work.data_ptr() + 4)),
        "fused: nt 0": lambda: fused(nt_=0), "fused: ntrace 0": lambda: fused(ntr_=0),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == -1, name
        with pytest.raises(MifwiError, match="EINVAL: .+"):
            _lib.check(rc)
    torch.cuda.synchronize()
    # CPU tensors: no fallback
    xc, oc = torch.tensor(c["x"]), torch.tensor(c["obs"])
    for call in (lambda: misfit.trace_filter(xc, good), lambda: misfit.l2_half(xc, oc, sos=good),
                 lambda: misfit.global_correlation(xc, oc, sos=good)):
        with pytest.raises(MifwiError):
            call()
    with pytest.raises(ValueError):
        misfit.trace_filter(x, good[:, :5])


# ---- the pyapi_denise shim ------------------------------------------------------------------------------------------

def _denise(api, time):
    d = api.Denise(None, 0)
    d.PHYSICS, d.ITERMAX = 1, 1
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = time, 0.002, 0, 10, 5.0, 1500.0
    return d


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """The small set-up of the Denise tests (60 x 90 cells, three shots, 31 receivers), with TIME = 1.8 s = 900 steps: the
    frequency-domain form wraps the impulse response of the 2 Hz high-pass around its padded window, and at the 250 steps
    of that set-up it is 5e-4 away from sosfilt, which is not the recursive kernels' error; at 900 steps it is within 1e-8
    (tests/test_golden_helpers.py pins it at that length).  One forward for the observed data, one for the modelled traces,
    grad() once with the frequency-domain stage and twice with the recursive one."""
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 60, 90, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3)).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    vs[:8] = 0; vp[:8] = 1500; rho[:8] = 1000
    xsrc = np.array([400.0, 1000.0, 1400.0])
    src = api.Sources(xsrc, 40.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1500.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    true = api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx)
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)
    cwd, env = os.getcwd(), os.environ.get("MIFWI_STAGE_FILTER")
    os.chdir(tmp_path_factory.mktemp("shim"))
    try:
        d0 = _denise(api, 1.8)
        ox, oy = d0.forward(true, src, rec)
        obs = (np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))          # [nshot, nt, nrec]
        vx, vy = d0.forward(model, src, rec)
        runs = {}
        for key, mode in (("fft", "fft"), ("recursive", "recursive"), ("again", "recursive")):
            os.environ["MIFWI_STAGE_FILTER"] = mode
            d = _denise(api, 1.8)
            d.set_observed(*obs)
            d.add_fwi_stage(fc_low=2.0, fc_high=12.0)
            loss = d.grad(model, src, rec)
            runs[key] = (loss, [np.array(g) for g in d.get_fwi_gradients(["seis"])])
    finally:
        os.chdir(cwd)
        if env is None:
            os.environ.pop("MIFWI_STAGE_FILTER", None)
        else:
            os.environ["MIFWI_STAGE_FILTER"] = env
    to_t = lambda a: torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=_dev())     # -> [nt, nshot, nrec]
    return dict(runs=runs, v=(to_t(vx), to_t(vy)), o=(to_t(ox), to_t(oy)))


def test_shim_recursive_stage_agrees_with_frequency_domain_stage(shim):
    (lf, gf), (lr, gr) = shim["runs"]["fft"], shim["runs"]["recursive"]
    assert lf > 0 and lr > 0
    rel = [float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64))) for a, b in zip(gr, gf)]
    print("loss fft %.9e recursive %.9e (rel %.2e); gradient rel-L2 rho, vp, vs: %s" % (lf, lr, abs(lf - lr) / lf, rel))
    assert abs(lf - lr) <= 1e-5 * lf
    assert len(rel) == 3 and max(rel) <= 2e-5


def test_shim_recursive_stage_is_repeatable(shim):
    (l1, g1), (l2, g2) = shim["runs"]["recursive"], shim["runs"]["again"]
    assert l1 == l2
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


def test_shim_loss_is_the_l2_of_the_filtered_traces(shim):
    sos = misfit.butterworth_sos(0.002, 2.0, 12.0, 6)
    tot = sum(float(misfit.l2_half(misfit.trace_filter(v, sos), misfit.trace_filter(o, sos)))
              for v, o in zip(shim["v"], shim["o"]))
    loss = shim["runs"]["recursive"][0]
    print("grad() loss %.9e, l2_half of the filtered traces %.9e" % (loss, tot))
    assert abs(loss - tot) <= 1e-6 * tot
