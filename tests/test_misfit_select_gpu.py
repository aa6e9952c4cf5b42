"""Trace kill, trace weights and time windows inside the misfit kernels (csrc/mifwi_misfit_select.h) against scipy in
float64, computed here from the same float32 inputs:  F = sosfilt(sos, ., axis=0) (the identity without a stage),
F^T z = sosfilt(sos, z[::-1], axis=0)[::-1],  W = TraceSelection.dense(nt),

    L2                  r = W F(pred - obs);  loss = 1/2 sum r^2;  adj = F^T W r
    GLOBAL_CORRELATION  s = W F pred, o = W F obs;  loss = -sum <s,o>/(|s||o|);  adj = F^T W (ka o + kb s)

Shapes: nt 1 / 15 / 17 / 301 (the kernel's chunk of 16 rows) x ntrace 1 / 63 / 65 / 130 (the wave seams), the three reference
stages and no stage, gamma 0 / 0.02 / inf.  Per-trace amplitudes 1e-6 ... 1e2, trace weights a in [0.25, 4], t_on uniform in
(-5, nt), t_off = t_on + U(-3, nt) (reversed and out-of-range windows among them), ntrace // 8 traces killed.

Bounds, per trace, eps = 2^-24:
  adjoint source  L2: 2 (1 + |h|_1) eps max(1, a) max_t |r|;  global correlation: max_t |r| -> |ka| max|o| + |kb| max|s|;
                  without a stage |h|_1 = 1
  losses          L2 relative 1e-6; global correlation absolute 1e-6 per trace
  killed traces and traces whose window holds no sample: adj == 0 exactly
  trace_window    per sample eps |ref| (+ 2^-149, the spacing of float32 where the taper takes a sample below 2^-126)

Coverage, asserted on the comparator so that another seed cannot hide it: at most a quarter of the traces killed, the
single trace of ntrace = 1 alive, and at least half of the traces with a non-zero reference adjoint source.  Two families of
cases cannot meet the last one under the draws above, whatever the seed, and are exempt from it (they are still run and
bounded): nt = 1 with gamma = inf (a boxcar holds the one sample for fewer than 3 % of the draws of t_on, t_off), and the
global correlation at nt = 1 (the derivative of s o / (|s||o|) for one sample is identically zero).
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
TINY = 2.0 ** -149        # the spacing of float32 below 2^-126: a tapered sample down there is not rounded to eps |ref|
STAGES = [(0.002, 0.0, 10.0, 6), (0.0025, 2.0, 12.0, 6), (0.002, 3.0, 10.0, 6), None]   # networks.py:7761, 9863, 10503; no stage
NTS = (1, 15, 17, 301)
NTRACES = (1, 63, 65, 130)
SHAPES = [(nt, ntr) for nt in NTS for ntr in NTRACES]
GAMMAS = (0.0, 0.02, float("inf"))
SEED = 0


def _dev():
    return torch.device("cuda:0")


def F(sos, a):
    return a if sos is None else signal.sosfilt(sos, a, axis=0)


def FT(sos, a):
    return a if sos is None else signal.sosfilt(sos, a[::-1], axis=0)[::-1]


def _sos(si):
    return None if STAGES[si] is None else misfit.butterworth_sos(*STAGES[si])


def _h1(sos, nt):
    spike = np.zeros(nt)
    spike[0] = 1.0
    return float(np.abs(F(sos, spike)).sum())


def make_case(si, gi, nt, ntr, whole_wave=False):
    """inputs (float32), the selection and the float64 comparator of one case"""
    key = 100000 * gi + 10000 * si + 10 * nt + ntr
    rng = np.random.default_rng(SEED + key)
    amp = 10.0 ** rng.uniform(-6.0, 2.0, ntr)
    pred = (rng.standard_normal((nt, ntr)) * amp).astype(np.float32)
    obs = (0.7 * pred + 0.5 * amp * rng.standard_normal((nt, ntr))).astype(np.float32)          # partly correlated
    a = rng.uniform(0.25, 4.0, ntr)
    if whole_wave:
        a[64:128] = 0.0
    else:
        a[rng.permutation(ntr)[:ntr // 8]] = 0.0
    t_on = rng.uniform(-5.0, nt, ntr)
    t_off = t_on + rng.uniform(-3.0, nt, ntr)
    sel = misfit.TraceSelection(a, t_on, t_off, GAMMAS[gi])
    sos = _sos(si)
    w = sel.dense(nt)
    # the comparator selects as the kernels do: a killed trace is not read
    live = sel.weight > 0
    p64, o64 = pred.astype(np.float64) * live, obs.astype(np.float64) * live
    r = w * F(sos, p64 - o64)
    s, o = w * F(sos, p64), w * F(sos, o64)
    ss, oo, so = (s * s).sum(0), (o * o).sum(0), (s * o).sum(0)
    ok = (ss > 0) & (oo > 0)
    den = np.where(ok, np.sqrt(ss) * np.sqrt(oo), 1.0)
    cc = np.where(ok, so / den, 0.0)
    ka, kb = np.where(ok, -1.0 / den, 0.0), np.where(ok, cc / np.where(ok, ss, 1.0), 0.0)
    scale = 2.0 * (1.0 + _h1(sos, nt)) * EPS * np.maximum(1.0, sel.weight.astype(np.float64))
    return dict(si=si, gi=gi, nt=nt, ntr=ntr, sos=sos, pred=pred, obs=obs, sel=sel, w=w, live=live,
                dead=~live | ~(w != 0).any(axis=0),
                l2=dict(loss=0.5 * (r * r).sum(), adj=FT(sos, w * r), bound=scale * np.abs(r).max(axis=0)),
                gc=dict(loss=-cc.sum(), adj=FT(sos, w * (ka * o + kb * s)), ok=ok,
                        bound=scale * (np.abs(ka) * np.abs(o).max(axis=0) + np.abs(kb) * np.abs(s).max(axis=0))))


def coverage_expected(kind, gi, nt):
    """the two families the module docstring exempts"""
    return not (nt == 1 and (kind == "gc" or GAMMAS[gi] == float("inf")))


def check_coverage(c, kind):
    ntr = c["ntr"]
    killed = int((~c["live"]).sum())
    nonzero = int((np.abs(c[kind]["adj"]).max(axis=0) > 0).sum())
    if ntr == 1:
        assert killed == 0
    else:
        assert 4 * killed <= ntr, (kind, c["si"], c["gi"], c["nt"], ntr, killed)
        if coverage_expected(kind, c["gi"], c["nt"]):
            assert 2 * nonzero >= ntr, (kind, c["si"], c["gi"], c["nt"], ntr, nonzero)
    return killed, nonzero


@pytest.fixture(scope="module")
def cases():
    """computed once, never written to: cases[(stage index, gamma index, nt, ntrace)]"""
    return {(si, gi, nt, ntr): make_case(si, gi, nt, ntr)
            for si in range(len(STAGES)) for gi in range(len(GAMMAS)) for nt, ntr in SHAPES}


def _gpu(a):
    return torch.tensor(a, device=_dev())


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


KERNEL = {"l2": misfit.l2_half, "gc": misfit.global_correlation}


def _run(kind, pred, obs, sos, sel, grad=True):
    p = pred.clone().requires_grad_(grad)
    loss = KERNEL[kind](p, obs, sos=sos, select=sel)
    if grad:
        loss.backward()
    return loss.detach(), p.grad


def _check(c, kind, pg=None, og=None, coverage=True):
    """one case against the comparator; returns loss, adjoint source and the worst err / bound"""
    pg = _gpu(c["pred"]) if pg is None else pg
    og = _gpu(c["obs"]) if og is None else og
    ref = c[kind]
    tag = "%s stage %d gamma %g nt %d ntrace %d" % (kind, c["si"], GAMMAS[c["gi"]], c["nt"], c["ntr"])
    killed, nonzero = check_coverage(c, kind) if coverage else (int((~c["live"]).sum()), -1)
    loss, adj = _run(kind, pg, og, c["sos"], c["sel"])
    assert adj.shape == pg.shape and adj.dtype == torch.float32
    got = _np(adj).reshape(c["nt"], -1)
    err = np.abs(got - ref["adj"]).max(axis=0)
    frac = float((err / np.maximum(ref["bound"], 1e-300)).max())
    lerr = abs(float(loss) - ref["loss"])
    print("%s: killed %d, non-zero adjoint %d; loss err %.2e (%s); adjoint worst err/bound %.3f"
          % (tag, killed, nonzero, lerr / abs(ref["loss"]) if kind == "l2" and ref["loss"] else lerr / c["ntr"],
             "relative" if kind == "l2" else "absolute per trace", frac))
    assert np.all(np.isfinite(got)), tag
    if kind == "l2":
        assert lerr <= 1e-6 * ref["loss"], tag
    else:
        assert lerr <= 1e-6 * c["ntr"], tag
    assert np.all(err <= ref["bound"]), tag
    assert np.all(got[:, c["dead"]] == 0), tag                     # killed or nothing inside the window: exactly zero
    assert np.all(ref["adj"][:, c["dead"]] == 0), tag
    return loss, adj, frac


@pytest.mark.parametrize("gi", range(len(GAMMAS)))
@pytest.mark.parametrize("si", range(len(STAGES)))
@pytest.mark.parametrize("kind", ["l2", "gc"])
def test_selected_misfit_matches_the_comparator(cases, kind, si, gi):
    worst = 0.0
    for nt, ntr in SHAPES:
        c = cases[si, gi, nt, ntr]
        pg, og = _gpu(c["pred"]), _gpu(c["obs"])
        loss, adj, frac = _check(c, kind, pg, og)
        worst = max(worst, frac)
        # no adjoint source asked for: the same loss, bit for bit; a second call: the same bits all over
        assert torch.equal(_run(kind, pg, og, c["sos"], c["sel"], grad=False)[0], loss)
        loss2, adj2 = _run(kind, pg, og, c["sos"], c["sel"])
        assert torch.equal(loss2, loss) and torch.equal(adj2, adj)
    print("%s stage %d gamma %g: worst err/bound over all shapes %.3f" % (kind, si, GAMMAS[gi], worst))


@pytest.mark.parametrize("si", [1, 3])
@pytest.mark.parametrize("kind", ["l2", "gc"])
def test_a_whole_wave_killed(kind, si):
    c = make_case(si, 1, 301, 130, whole_wave=True)
    assert not c["live"][64:128].any() and c["live"][:64].all() and c["live"][128:].all()
    nan_p, nan_o = c["pred"].copy(), c["obs"].copy()
    nan_p[:, 64:128] = np.nan
    nan_o[:, 64:128] = np.nan
    loss, adj, _ = _check(c, kind, coverage=False)              # the extra case: 64 of 130 traces killed
    assert bool((adj[:, 64:128] == 0).all()) and bool((adj[:, :64] != 0).any()) and bool((adj[:, 128:] != 0).any())
    loss_n, adj_n = _run(kind, _gpu(nan_p), _gpu(nan_o), c["sos"], c["sel"])
    assert torch.equal(loss_n, loss) and torch.equal(adj_n, adj)


@pytest.mark.parametrize("si", [1, 3])
@pytest.mark.parametrize("kind", ["l2", "gc"])
def test_nan_and_inf_in_killed_traces_change_nothing(cases, kind, si):
    for nt, ntr in ((17, 65), (301, 130)):
        c = cases[si, 1, nt, ntr]
        dead = ~c["live"]
        assert dead.any()
        zero_p, zero_o = c["pred"].copy(), c["obs"].copy()
        zero_p[:, dead] = 0.0
        zero_o[:, dead] = 0.0
        bad_p, bad_o = zero_p.copy(), zero_o.copy()
        bad_p[:, dead] = np.nan
        bad_o[:, dead] = np.inf
        bad_p[0, dead] = -np.inf
        bad_o[nt - 1, dead] = np.nan
        loss0, adj0 = _run(kind, _gpu(zero_p), _gpu(zero_o), c["sos"], c["sel"])
        loss1, adj1 = _run(kind, _gpu(bad_p), _gpu(bad_o), c["sos"], c["sel"])
        assert bool(torch.isfinite(loss1)) and bool(torch.isfinite(adj1).all())
        assert torch.equal(loss1, loss0) and torch.equal(adj1, adj0)
        assert torch.equal(_run(kind, _gpu(bad_p), _gpu(bad_o), c["sos"], c["sel"], grad=False)[0], loss0)
        # and the comparator's case itself, with what it had in those traces
        loss2, adj2 = _run(kind, _gpu(c["pred"]), _gpu(c["obs"]), c["sos"], c["sel"])
        assert torch.equal(loss2, loss0) and torch.equal(adj2, adj0)


@pytest.mark.parametrize("kind", ["l2", "gc"])
def test_no_selection_is_the_existing_call_bit_for_bit(cases, kind):
    for si in (1, 3):
        for nt, ntr in ((17, 65), (301, 130)):
            c = cases[si, 1, nt, ntr]
            pg, og = _gpu(c["pred"]), _gpu(c["obs"])
            p0 = pg.clone().requires_grad_(True)
            l0 = KERNEL[kind](p0, og, sos=c["sos"]) if c["sos"] is not None else KERNEL[kind](p0, og)
            l0.backward()
            # select=None: today's path;  a selection without arrays: the C call with three NULLs, the same kernels
            for sel in (None, misfit.TraceSelection()):
                l1, a1 = _run(kind, pg, og, c["sos"], sel)
                assert torch.equal(l1, l0.detach()) and torch.equal(a1, p0.grad), (si, nt, ntr, sel)
            # weights of one and windows that cover every trace: the selected kernels, and the bits of the filtered ones
            ones = misfit.TraceSelection(np.ones(ntr), np.full(ntr, -3.0), np.full(ntr, nt + 2.0), 0.02)
            if c["sos"] is None:
                # without a stage the global correlation has one body for both (the same 64 x 16 layout, the same sums;
                # w = 1 leaves a sample as it is); L2 without a selection is misfit_l2: another grid, squares in float
                if kind == "gc":
                    l2, a2 = _run(kind, pg, og, None, ones)
                    assert torch.equal(l2, l0.detach()) and torch.equal(a2, p0.grad), (si, nt, ntr)
                continue
            l2, a2 = _run(kind, pg, og, c["sos"], ones)
            assert torch.equal(l2, l0.detach()) and torch.equal(a2, p0.grad), (si, nt, ntr)
            assert torch.equal(_run(kind, pg, og, c["sos"], ones, grad=False)[0], l0.detach())


def test_3d_and_unaligned_views(cases):
    for si in (1, 3):
        c = cases[si, 1, 301, 130]
        sel3 = misfit.TraceSelection(*(a.reshape(5, 26) for a in (c["sel"].weight, c["sel"].t_on, c["sel"].t_off)), c["sel"].gamma)
        for kind in ("l2", "gc"):
            pg, og = _gpu(c["pred"]), _gpu(c["obs"])
            loss2, adj2, _ = _check(c, kind, pg, og)
            loss3, adj3 = _run(kind, pg.view(301, 5, 26), og.view(301, 5, 26), c["sos"], sel3)
            assert adj3.shape == (301, 5, 26) and torch.equal(loss3, loss2) and torch.equal(adj3.view(301, 130), adj2)
            # a contiguous view that is only 4-byte aligned
            buf = torch.empty(301 * 130 + 1, device=_dev())
            pv = buf[1:].view(301, 130)
            pv.copy_(pg)
            assert pv.data_ptr() % 8 == 4
            lossv, adjv = _run(kind, pv, og, c["sos"], c["sel"])
            assert torch.equal(lossv, loss2) and torch.equal(adjv, adj2)
        with pytest.raises(ValueError):
            misfit.l2_half(pg.view(301, 5, 26), og.view(301, 5, 26), sos=c["sos"], select=c["sel"])     # [130] is not [5, 26]
        # the selection of a shot range
        part = sel3.shots(slice(1, 4))
        lp, ap = _run("l2", pg.view(301, 5, 26)[:, 1:4], og.view(301, 5, 26)[:, 1:4], c["sos"], part)
        full = _run("l2", pg.view(301, 5, 26), og.view(301, 5, 26), c["sos"], sel3)[1]
        assert torch.equal(ap, full[:, 1:4])


def _window_inplace(x, sel):
    lib = _lib.load()
    buf = x.clone()
    nt = buf.shape[0]
    a, on, off = sel._on(buf.device, buf.shape[1:])
    _lib.check(lib.mifwi_trace_window(0, _lib.ptr(buf), _lib.ptr(buf), nt, buf.numel() // nt, _lib.ptr(a), _lib.ptr(on),
                                      _lib.ptr(off), sel.gamma, torch.cuda.current_stream().cuda_stream))
    return buf


@pytest.mark.parametrize("gi", range(len(GAMMAS)))
def test_trace_window_is_dense_times_x(cases, gi):
    for nt, ntr in SHAPES:
        c = cases[0, gi, nt, ntr]
        xg = _gpu(c["pred"])
        y = misfit.trace_window(xg, c["sel"])
        assert y.shape == xg.shape and y.dtype == torch.float32
        ref = c["w"] * (c["pred"].astype(np.float64) * c["live"])
        err = np.abs(_np(y) - ref)
        print("gamma %g nt %d ntrace %d: worst err / (eps |ref| + 2^-149) %.3f"
              % (GAMMAS[gi], nt, ntr, (err / (EPS * np.abs(ref) + TINY)).max()))
        assert np.all(err <= EPS * np.abs(ref) + TINY), (gi, nt, ntr)
        assert torch.equal(_window_inplace(xg, c["sel"]), y)                    # y == x: the same bits
    # NaN in a killed trace is selected away; weight or window alone
    c = cases[0, gi, 17, 65]
    bad = c["pred"].copy()
    bad[:, ~c["live"]] = np.nan
    assert torch.equal(misfit.trace_window(_gpu(bad), c["sel"]), misfit.trace_window(_gpu(c["pred"]), c["sel"]))
    only_w = misfit.TraceSelection(weight=c["sel"].weight)
    assert np.array_equal(_np(misfit.trace_window(_gpu(c["pred"]), only_w)),
                          (c["pred"] * c["sel"].weight).astype(np.float32).astype(np.float64))
    only_t = misfit.TraceSelection(t_on=c["sel"].t_on, t_off=c["sel"].t_off, gamma=GAMMAS[gi])
    ref = only_t.dense(17) * c["pred"].astype(np.float64)
    assert np.all(np.abs(_np(misfit.trace_window(_gpu(c["pred"]), only_t)) - ref) <= EPS * np.abs(ref) + TINY)


def test_autograd(cases):
    for si in (1, 3):
        c = cases[si, 1, 301, 65]
        pg, og = _gpu(c["pred"]), _gpu(c["obs"])
        for kind in ("l2", "gc"):
            loss, adj = _run(kind, pg, og, c["sos"], c["sel"])
            p3 = pg.clone().requires_grad_(True)
            o3 = og.clone().requires_grad_(True)
            (3.0 * KERNEL[kind](p3, o3, sos=c["sos"], select=c["sel"])).backward()
            assert torch.equal(p3.grad, 3.0 * adj) and o3.grad is None              # obs gets no gradient
            assert not KERNEL[kind](pg, og, sos=c["sos"], select=c["sel"]).requires_grad
    # W is its own transpose
    c = cases[0, 1, 301, 65]
    x = _gpu(c["pred"]).requires_grad_(True)
    g = _gpu(c["obs"])
    (misfit.trace_window(x, c["sel"]) * g).sum().backward()
    assert torch.equal(x.grad, misfit.trace_window(g, c["sel"]))
    # the composed form is the same objective: W F pred against W F obs, then the plain kernel
    c = cases[1, 1, 301, 65]
    pg, og = _gpu(c["pred"]), _gpu(c["obs"])
    p = pg.clone().requires_grad_(True)
    composed = misfit.l2_half(misfit.trace_window(misfit.trace_filter(p, c["sos"]), c["sel"]),
                              misfit.trace_window(misfit.trace_filter(og, c["sos"]), c["sel"]))
    composed.backward()
    assert abs(float(composed.detach()) - c["l2"]["loss"]) <= 1e-6 * c["l2"]["loss"]
    # it stores F pred, W F pred, F obs, W F obs and W g as float on the way: the project's gradient tolerance, per trace
    live = ~c["dead"]
    rel = np.linalg.norm(_np(p.grad) - c["l2"]["adj"], axis=0)[live] / np.linalg.norm(c["l2"]["adj"], axis=0)[live]
    print("composed form against the comparator: worst rel-L2 of a trace %.2e" % rel.max())
    assert rel.max() <= 2e-5 and bool((p.grad[:, torch.tensor(c["dead"], device=_dev())] == 0).all())


def test_invalid_arguments_raise_with_a_message(cases):
    lib = _lib.load()
    c = cases[1, 1, 17, 65]
    nt, ntr = 17, 65
    good = c["sos"]
    x, o = _gpu(c["pred"]), _gpu(c["obs"])
    a, on, off = c["sel"]._on(_dev(), (ntr,))
    y, loss = torch.empty_like(x), torch.empty((), device=_dev())
    work = torch.empty(lib.mifwi_misfit_selected_work_elems(_lib.MISFIT_GLOBAL_CORRELATION, nt, ntr, 6) + 2, device=_dev())
    assert lib.mifwi_misfit_selected_work_elems(_lib.MISFIT_L2, nt, ntr, 0) >= lib.mifwi_misfit_work_elems(_lib.MISFIT_L2, nt, ntr)
    assert lib.mifwi_misfit_selected_work_elems(_lib.MISFIT_L2, 0, ntr, 0) == 0
    st = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    sp = lambda s: None if s is None else s.ctypes.data_as(ctypes.c_void_p)

    def bad(s, j, v):
        b = s.copy()
        b[0, j] = v
        return b

    def fused(kind=_lib.MISFIT_L2, pp=P(x), op=P(o), nt_=nt, ntr_=ntr, sos=good, nsec=None, ap=P(a), onp=P(on), offp=P(off),
              gamma=0.02, lp=P(loss), wp=P(work)):
        return lib.mifwi_misfit_selected(0, kind, pp, op, nt_, ntr_, sp(sos), (0 if sos is None else sos.shape[0]) if nsec is None
                                         else nsec, ap, onp, offp, gamma, lp, P(y), wp, st)

    def window(xp=P(x), yp=P(y), nt_=nt, ntr_=ntr, onp=P(on), offp=P(off), gamma=0.02):
        return lib.mifwi_trace_window(0, xp, yp, nt_, ntr_, P(a), onp, offp, gamma, st)

    assert fused() == 0 and fused(kind=_lib.MISFIT_GLOBAL_CORRELATION) == 0 and fused(sos=None) == 0 and window() == 0
    assert fused(onp=None, offp=None) == 0 and fused(ap=None) == 0 and fused(gamma=float("inf")) == 0
    nine = np.concatenate([good, good])[:9].copy()
    calls = {
        "t_on alone": lambda: fused(offp=None), "t_off alone": lambda: fused(onp=None),
        "t_on alone, no weights": lambda: fused(ap=None, offp=None),
        "gamma < 0": lambda: fused(gamma=-1.0), "gamma nan": lambda: fused(gamma=float("nan")),
        "gamma nan, nothing selected": lambda: fused(ap=None, onp=None, offp=None, gamma=float("nan")),
        "sos without nsec": lambda: fused(nsec=0), "nsec without sos": lambda: fused(sos=None, nsec=3),
        "L1": lambda: fused(kind=_lib.MISFIT_L1_TRACE_NORM), "L1, no stage": lambda: fused(kind=_lib.MISFIT_L1_TRACE_NORM, sos=None),
        "L1, nothing selected": lambda: fused(kind=_lib.MISFIT_L1_TRACE_NORM, sos=None, ap=None, onp=None, offp=None),
        "kind 7": lambda: fused(kind=7), "kind 7, no stage": lambda: fused(kind=7, sos=None),
        "null pred": lambda: fused(pp=None), "null obs": lambda: fused(op=None), "null loss": lambda: fused(lp=None),
        "null work": lambda: fused(wp=None), "null pred, no stage": lambda: fused(pp=None, sos=None),
        "null pred, nothing selected": lambda: fused(pp=None, ap=None, onp=None, offp=None),
        "nsec 9": lambda: fused(sos=nine), "nsec -1": lambda: fused(nsec=-1),
        "a0": lambda: fused(sos=bad(good, 3, 0.5)), "nan coefficient": lambda: fused(sos=bad(good, 0, np.nan)),
        "work alignment": lambda: fused(wp=ctypes.c_void_p(work.data_ptr() + 4)),
        "work alignment, no stage": lambda: fused(sos=None, wp=ctypes.c_void_p(work.data_ptr() + 4)),
        "nt 0": lambda: fused(nt_=0), "ntrace 0": lambda: fused(ntr_=0), "nt 2^31": lambda: fused(nt_=2 ** 31),
        "nt 0, no stage": lambda: fused(nt_=0, sos=None), "ntrace 0, no stage": lambda: fused(ntr_=0, sos=None),
        "window: null x": lambda: window(xp=None), "window: null y": lambda: window(yp=None),
        "window: t_on alone": lambda: window(offp=None), "window: t_off alone": lambda: window(onp=None),
        "window: gamma < 0": lambda: window(gamma=-0.5), "window: gamma nan": lambda: window(gamma=float("nan")),
        "window: nt 0": lambda: window(nt_=0), "window: ntrace 0": lambda: window(ntr_=0), "window: nt 2^31": lambda: window(nt_=2 ** 31),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == -1, name
        with pytest.raises(MifwiError, match="EINVAL: .+"):
            _lib.check(rc)
    torch.cuda.synchronize()
    # CPU tensors: no fallback; a selection of another shape: ValueError
    xc, oc = torch.tensor(c["pred"]), torch.tensor(c["obs"])
    for call in (lambda: misfit.trace_window(xc, c["sel"]), lambda: misfit.l2_half(xc, oc, sos=good, select=c["sel"]),
                 lambda: misfit.global_correlation(xc, oc, select=c["sel"])):
        with pytest.raises(MifwiError):
            call()
    other = cases[1, 1, 17, 63]["sel"]
    for call in (lambda: misfit.trace_window(x, other), lambda: misfit.l2_half(x, o, sos=good, select=other),
                 lambda: misfit.global_correlation(x, o, select=other)):
        with pytest.raises(ValueError):
            call()


# ---- the pyapi_denise shim ------------------------------------------------------------------------------------------

def _denise(api):
    d = api.Denise(None, 0)
    d.PHYSICS, d.ITERMAX = 1, 1
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.5, 0.002, 0, 10, 5.0, 1500.0        # 250 steps
    d.add_fwi_stage(fc_low=2.0, fc_high=12.0)
    return d


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """The small set-up of the Denise tests (60 x 90 cells, three shots, 31 receivers, 250 steps): one forward for the
    observed data, one for the modelled traces, and grad() with and without a selection."""
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 60, 90, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3)).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    vs[:8] = 0; vp[:8] = 1500; rho[:8] = 1000
    xsrc = np.array([400.0, 1000.0, 1400.0])
    xrec = np.arange(300.0, 1500.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    sources = lambda n: api.Sources(xsrc[:n], 40.0 * xsrc[:n] / xsrc[:n], 8.0)
    true = api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx)
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)
    kill = np.zeros((len(xrec), 3))                     # TRKILL_FILE layout [nrec, nshot]
    kill[:, 2] = 1
    # picks along a linear move-out from each source, the window a third of the trace
    picks = 0.08 + np.abs(xrec[None, :] - xsrc[:, None]) / 3000.0
    cwd, env = os.getcwd(), os.environ.pop("MIFWI_STAGE_FILTER", None)
    os.chdir(tmp_path_factory.mktemp("shim_select"))
    try:
        d0 = _denise(api)
        ox, oy = d0.forward(true, sources(3), rec)
        obs = [np.transpose(a, (0, 2, 1)).copy() for a in (ox, oy)]                   # [nshot, nt, nrec]
        vx, vy = d0.forward(model, sources(3), rec)
        nan = [a.copy() for a in obs]
        nan[0][2], nan[1][2, ::2] = np.nan, np.inf
        runs = {}

        def run(key, nshot=3, observed=obs, trkill=0, table=None, windows=None, mode=None):
            d = _denise(api)
            d.set_observed(*(a[:nshot] for a in observed))
            d.TRKILL = trkill
            if table is not None:
                d.set_trace_kill(table)
            if windows is not None:
                d.set_time_windows(*windows)
            if mode:
                os.environ["MIFWI_STAGE_FILTER"] = mode
            try:
                loss = d.grad(model, sources(nshot), rec)
            finally:
                os.environ.pop("MIFWI_STAGE_FILTER", None)
            runs[key] = (loss, [np.array(g) for g in d.get_fwi_gradients(["seis"])])

        run("plain")
        run("two shots", nshot=2)
        run("killed", trkill=1, table=kill)
        run("killed again", trkill=1, table=kill)
        run("killed, nan", trkill=1, table=kill, observed=nan)
        run("table without TRKILL", trkill=0, table=kill)
        run("windows", windows=(picks, 0.03, 0.14, 400.0))
        run("killed, windows", trkill=1, table=kill, windows=(picks, 0.03, 0.14, 400.0))
        run("killed, windows, fft", trkill=1, table=kill, windows=(picks, 0.03, 0.14, 400.0), mode="fft")
        d = _denise(api)
        d.set_observed(*obs)
        d.TRKILL = 1
        with pytest.raises(api.MifwiError, match="set_trace_kill"):
            d.grad(model, sources(3), rec)
    finally:
        os.chdir(cwd)
        if env is not None:
            os.environ["MIFWI_STAGE_FILTER"] = env
    to_t = lambda a: torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=_dev())     # -> [nt, nshot, nrec]
    sel = misfit.TraceSelection.from_picks(picks, 0.03, 0.14, 0.002, gamma_per_s2=400.0, weight=np.where(kill.T != 0, 0.0, 1.0))
    return dict(runs=runs, v=(to_t(vx), to_t(vy)), o=(to_t(ox), to_t(oy)), sel=sel, api=api)


def _rel(a, b):
    return [float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64))) for x, y in zip(a, b)]


def test_shim_killing_a_shot_is_the_run_without_it(shim):
    (lk, gk), (l2, g2) = shim["runs"]["killed"], shim["runs"]["two shots"]
    rel = _rel(gk, g2)
    print("loss killed %.9e two shots %.9e (rel %.2e); gradient rel-L2 rho, vp, vs: %s" % (lk, l2, abs(lk - l2) / l2, rel))
    assert l2 > 0 and abs(lk - l2) <= 1e-6 * l2
    assert len(rel) == 3 and max(rel) <= 2e-5
    # and it is not the three-shot run; a table without TRKILL = 1 is not acted on
    lp, gp = shim["runs"]["plain"]
    assert lp > lk and min(_rel(gk, gp)) > 1e-2
    lt, gt = shim["runs"]["table without TRKILL"]
    assert lt == lp and all(np.array_equal(a, b) for a, b in zip(gt, gp))


def test_shim_nan_in_killed_observed_traces_changes_nothing(shim):
    (lk, gk), (ln, gn) = shim["runs"]["killed"], shim["runs"]["killed, nan"]
    assert np.isfinite(ln) and ln == lk
    for a, b in zip(gk, gn):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


def test_shim_selection_is_repeatable(shim):
    (l1, g1), (l2, g2) = shim["runs"]["killed"], shim["runs"]["killed again"]
    assert l1 == l2
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


def test_shim_loss_is_the_l2_of_the_windowed_filtered_traces(shim):
    sos = misfit.butterworth_sos(0.002, 2.0, 12.0, 6)
    sel = shim["sel"]
    tot = sum(float(misfit.l2_half(misfit.trace_window(misfit.trace_filter(v, sos), sel),
                                   misfit.trace_window(misfit.trace_filter(o, sos), sel)))
              for v, o in zip(shim["v"], shim["o"]))
    loss = shim["runs"]["killed, windows"][0]
    print("grad() loss %.9e, l2_half of the windowed filtered traces %.9e" % (loss, tot))
    assert tot > 0 and abs(loss - tot) <= 1e-6 * tot
    # the frequency-domain stage composes the same selection through trace_window
    api = shim["api"]
    fl = lambda a: api.butterworth(a, 0.002, 2.0, 12.0, 6)
    tot_fft = sum(float(misfit.l2_half(misfit.trace_window(fl(v), sel), misfit.trace_window(fl(o), sel)))
                  for v, o in zip(shim["v"], shim["o"]))
    loss_fft = shim["runs"]["killed, windows, fft"][0]
    print("fft stage: grad() loss %.9e, composed %.9e" % (loss_fft, tot_fft))
    assert abs(loss_fft - tot_fft) <= 1e-6 * tot_fft


def test_shim_time_windows_change_the_gradient(shim):
    (lp, gp), (lw, gw) = shim["runs"]["plain"], shim["runs"]["windows"]
    rel = _rel(gw, gp)
    print("loss %.9e with windows %.9e; gradient change rel-L2 rho, vp, vs: %s" % (lp, lw, rel))
    assert 0 < lw < lp
    assert min(rel) > 0.1
