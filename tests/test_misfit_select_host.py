"""misfit.TraceSelection on the host: constructors and .dense() against the definition

    w[t, tr] = a[tr] g,   d = max(t_on - t, t - t_off, 0),   g = 1 where d == 0, else exp(-gamma d^2)

written out sample by sample in float64 from the float32 values the selection keeps; reversed and out-of-range windows,
gamma = 0 and inf, .shots(), validation, and how the pyapi_denise shim classifies TRKILL and TIMEWIN."""
import math

import numpy as np
import pytest

from physicsbasedfwi2_amd import misfit


def _dense_by_hand(nt, a, on, off, gamma):
    """the definition, one sample at a time"""
    ntr = len(a)
    w = np.empty((nt, ntr))
    for tr in range(ntr):
        for t in range(nt):
            d = max(float(on[tr]) - t, t - float(off[tr]), 0.0)
            w[t, tr] = float(a[tr]) * (1.0 if d == 0 else math.exp(-gamma * d * d))
    return w


@pytest.mark.parametrize("gamma", [0.0, 0.02, math.inf])
def test_dense_is_the_definition(gamma):
    rng = np.random.default_rng(5)
    nt, ntr = 17, 11
    a = rng.uniform(0.25, 4.0, ntr).astype(np.float32)
    a[3] = 0.0
    on = rng.uniform(-5.0, nt, ntr).astype(np.float32)
    off = (on + rng.uniform(-3.0, nt, ntr)).astype(np.float32)
    on[0], off[0] = -7.5, -2.0                   # wholly before the trace
    on[1], off[1] = nt + 3.0, nt + 9.0           # wholly after it
    on[2], off[2] = 9.0, 4.0                     # reversed: no sample inside
    on[4], off[4] = -100.0, 1000.0               # covers everything
    sel = misfit.TraceSelection(a, on, off, gamma)
    assert sel.shape == (ntr,) and sel.weight.dtype == np.float32 and sel.t_on.dtype == np.float32
    w = sel.dense(nt)
    assert w.dtype == np.float64 and w.shape == (nt, ntr)
    ref = _dense_by_hand(nt, a, on, off, gamma)
    assert np.allclose(w, ref, rtol=1e-15, atol=0.0)
    assert np.all(w[:, 3] == 0) and np.all(w[:, 4] == np.float64(a[4]))
    if gamma == 0.0:
        assert np.array_equal(w, np.broadcast_to(a.astype(np.float64), (nt, ntr)))
    if gamma == math.inf:
        assert np.all(w[:, :3] == 0)             # empty windows
        inside = (np.arange(nt)[:, None] >= on) & (np.arange(nt)[:, None] <= off)
        assert np.array_equal(w != 0, inside & (a > 0))
    if gamma == 0.02:
        assert np.all(w[:, :3] < a[:3]) and np.all(w[:, [0, 2]] > 0)      # tapered, never cut


def test_absent_parts_are_neutral():
    a = np.array([[1.0, 0.0, 2.5], [0.5, 1.0, 1.0]], dtype=np.float32)
    assert np.array_equal(misfit.TraceSelection(weight=a).dense(4), np.broadcast_to(a.astype(np.float64), (4, 2, 3)))
    on, off = np.full((2, 3), 1.0), np.full((2, 3), 2.0)
    w = misfit.TraceSelection(t_on=on, t_off=off, gamma=math.inf).dense(4)
    assert np.array_equal(w, np.broadcast_to(np.array([0.0, 1.0, 1.0, 0.0]).reshape(4, 1, 1), (4, 2, 3)))
    none = misfit.TraceSelection()
    assert none.shape is None and none.gamma == 0.0
    with pytest.raises(ValueError):
        none.dense(4)


def test_from_kill_and_from_picks():
    kill = np.array([[0, 1, 0], [2, 0, 0]])
    sel = misfit.TraceSelection.from_kill(kill)
    assert np.array_equal(sel.weight, np.array([[1, 0, 1], [0, 1, 1]], dtype=np.float32)) and sel.t_on is None
    dt = 0.002
    picks = np.array([[0.1, 0.2, 0.3], [0.15, 0.25, 0.35]])
    sel = misfit.TraceSelection.from_picks(picks, 0.02, 0.05, dt, gamma_per_s2=5000.0)
    assert np.array_equal(sel.t_on, ((picks - 0.02) / dt).astype(np.float32))
    assert np.array_equal(sel.t_off, ((picks + 0.05) / dt).astype(np.float32))
    assert sel.gamma == 5000.0 * dt * dt and sel.weight is None
    # seconds to samples: 10 samples ahead of the window the taper is exp(-gamma_s (10 dt)^2)
    w = sel.dense(200)
    t0 = int(round((0.1 - 0.02) / dt))
    assert w[t0, 0, 0] == 1.0 and abs(w[t0 - 10, 0, 0] - math.exp(-5000.0 * (10 * dt) ** 2)) < 1e-6
    # per-trace window lengths and a weight on top
    before = np.full((2, 3), 0.02)
    both = misfit.TraceSelection.from_picks(picks, before, 0.05, dt, gamma_per_s2=5000.0, weight=sel_weight(kill))
    assert np.array_equal(both.dense(200), w * sel_weight(kill))


def sel_weight(kill):
    return np.where(kill != 0, 0.0, 1.0)


def test_shots_selects_a_shot_range():
    rng = np.random.default_rng(1)
    a, on = rng.uniform(0.5, 2.0, (5, 7)), rng.uniform(0.0, 10.0, (5, 7))
    sel = misfit.TraceSelection(a, on, on + 4.0, 0.1)
    part = sel.shots(slice(1, 4))
    assert part.shape == (3, 7) and part.gamma == sel.gamma
    assert np.array_equal(part.dense(12), sel.dense(12)[:, 1:4])
    assert misfit.TraceSelection().shots(slice(0, 2)).shape is None
    with pytest.raises(ValueError):
        misfit.TraceSelection(a[0]).shots(slice(0, 1))           # no shot axis
    with pytest.raises(ValueError):
        sel.shots(2)


def test_validation():
    ok = np.ones((2, 3))
    bad = {
        "negative weight": lambda: misfit.TraceSelection(weight=-ok),
        "nan weight": lambda: misfit.TraceSelection(weight=ok * np.nan),
        "inf weight": lambda: misfit.TraceSelection(weight=ok * np.inf),
        "nan t_on": lambda: misfit.TraceSelection(t_on=ok * np.nan, t_off=ok),
        "inf t_off": lambda: misfit.TraceSelection(t_on=ok, t_off=ok * np.inf),
        "t_on alone": lambda: misfit.TraceSelection(t_on=ok),
        "t_off alone": lambda: misfit.TraceSelection(t_off=ok),
        "negative gamma": lambda: misfit.TraceSelection(weight=ok, gamma=-1.0),
        "nan gamma": lambda: misfit.TraceSelection(weight=ok, gamma=float("nan")),
        "shapes": lambda: misfit.TraceSelection(weight=ok, t_on=np.ones(6), t_off=np.ones(6)),
    }
    for name, call in bad.items():
        with pytest.raises(ValueError):
            call()
        print("rejected:", name)


def test_select_refuses_cpu_tensors_and_wrong_shapes():
    import torch
    from physicsbasedfwi2_amd._lib import MifwiError
    sel = misfit.TraceSelection(weight=np.ones((2, 3)))
    x = torch.zeros(5, 2, 3)
    for call in (lambda: misfit.l2_half(x, x, select=sel), lambda: misfit.global_correlation(x, x, select=sel),
                 lambda: misfit.trace_window(x, sel)):
        with pytest.raises(MifwiError):
            call()
    with pytest.raises(ValueError):
        sel._on(torch.device("cpu"), (3, 2))


def test_shim_serves_trkill_and_still_refuses_timewin():
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    d = api.Denise(None, 0)
    assert d.TRKILL == 0
    d.TRKILL = 1                                                  # served
    assert d.TRKILL == 1
    d.TIMEWIN = 0
    with pytest.raises(api.MifwiError, match="set_time_windows"):
        d.TIMEWIN = 1
    # TRKILL = 1 without a table is an error of grad(), raised where the selection is put together
    with pytest.raises(api.MifwiError, match="set_trace_kill"):
        d._selection((3, 31), 0.002)
    table = np.zeros((31, 3))                                     # TRKILL_FILE layout [nrec, nshot]
    table[4, 2] = 1
    d.set_trace_kill(table)
    sel = d._selection((3, 31), 0.002)
    assert sel.shape == (3, 31) and sel.weight[2, 4] == 0 and sel.weight.sum() == 3 * 31 - 1 and sel.t_on is None
    with pytest.raises(api.MifwiError):
        d._selection((2, 31), 0.002)                              # a table for another survey
    d.set_time_windows(np.full((3, 31), 0.2), 0.05, 0.1, gamma=1000.0)
    sel = d._selection((3, 31), 0.002)
    assert sel.weight[2, 4] == 0 and sel.t_on[0, 0] == np.float32(0.15 / 0.002) and sel.gamma == 1000.0 * 0.002 ** 2
    d.TRKILL = 0                                                  # the table stays, and is not acted on
    assert d._selection((3, 31), 0.002).weight is None
    d.set_time_windows(None)
    assert d._selection((3, 31), 0.002) is None
    with pytest.raises(api.MifwiError):
        d.set_trace_kill(np.zeros(31))
