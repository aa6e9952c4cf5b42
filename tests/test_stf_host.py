"""Source-wavelet estimation without a GPU: the float64 reference states what it claims to state, the host solve of
misfit.solve_matching_filter agrees with it and with scipy's Levinson solver, and the pyapi_denise shim accepts INV_STF."""
import numpy as np
import pytest
import torch
from scipy.linalg import solve_toeplitz

import stf_reference as R
from physicsbasedfwi2_amd import misfit
from physicsbasedfwi2_amd._lib import MifwiError

CASES = [(301, 13, 12), (64, 5, 8), (17, 3, 5)]           # nt, nrec, lag_after
NSHOT = 2


def _decaying_filter(rng, nshot, nlag):
    return rng.standard_normal((nshot, nlag)) * np.exp(-np.arange(nlag) / 3.0)[None, :]


def _matched_pair(nt, nrec, lag_after, seed=0):
    """pred: coloured noise that has died out lag_after samples before the record ends; obs = h * pred exactly."""
    rng = np.random.default_rng(seed + nt)
    e = rng.standard_normal((nt + 1, NSHOT, nrec))
    pred = e[1:] + 0.5 * e[:-1]
    pred[nt - lag_after:] = 0.0
    h = _decaying_filter(rng, NSHOT, lag_after + 1)
    return pred, R.convolve(pred, h, 0), h


@pytest.mark.parametrize("lag_before,lag_after", [(0, 0), (0, 7), (4, 12), (3, 6)])
@pytest.mark.parametrize("nt", [1, 5, 40])
def test_reference_transpose_is_the_adjoint(nt, lag_before, lag_after):
    rng = np.random.default_rng(nt + lag_after)
    u, v = rng.standard_normal((2, nt, 3, 4))
    h = rng.standard_normal((3, lag_before + lag_after + 1))
    lhs = np.sum(R.convolve(u, h, lag_before) * v)
    rhs = np.sum(u * R.convolve(v, h, lag_before, transpose=True))
    scale = np.sum(R.convolve(u, h, lag_before, absolute=True) * np.abs(v))
    assert abs(lhs - rhs) <= 1e-13 * max(scale, 1.0)


def test_reference_convolution_is_numpy_convolve():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((30, 1, 1))
    h = rng.standard_normal((1, 9))
    full = np.convolve(x[:, 0, 0], h[0])                   # index n = t + i
    assert np.allclose(R.convolve(x, h, 0)[:, 0, 0], full[:30], rtol=0, atol=1e-13)
    assert np.allclose(R.convolve(x, h, 3)[:, 0, 0], full[3:33], rtol=0, atol=1e-13)


@pytest.mark.parametrize("nt,nrec,lag_after", CASES)
def test_reference_recovers_a_causal_filter(nt, nrec, lag_after):
    pred, obs, h = _matched_pair(nt, nrec, lag_after)
    a, _ = R.correlations(pred, obs, 0, lag_after)
    assert max(np.linalg.cond(R.toeplitz(a[s], 1e-8)) for s in range(NSHOT)) <= 1e4
    got = R.estimate(pred, obs, 0, lag_after, 1e-8)
    assert np.linalg.norm(got - h) <= 1e-5 * np.linalg.norm(h)


@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-8])
@pytest.mark.parametrize("nt,nrec,lag_after", CASES)
def test_solve_matching_filter_against_levinson_and_reference(nt, nrec, lag_after, eps):
    pred, obs, _ = _matched_pair(nt, nrec, lag_after, seed=1)
    obs = obs + 0.1 * np.random.default_rng(9).standard_normal(obs.shape)
    a, c = R.correlations(pred, obs, 0, lag_after)
    h = misfit.solve_matching_filter(torch.tensor(a), torch.tensor(c), eps)
    assert h.dtype == torch.float64 and h.device.type == "cpu" and tuple(h.shape) == (NSHOT, lag_after + 1)
    nlag = lag_after + 1
    for s in range(NSHOT):
        t = R.toeplitz(a[s], eps)
        cond = np.linalg.cond(t)
        assert cond <= 1e4
        col = a[s].copy()
        col[0] += eps * a[s, 0]
        lev = solve_toeplitz(col, c[s])
        tol = nlag * cond * R.U64
        assert np.linalg.norm(h[s].numpy() - lev) <= tol * np.linalg.norm(lev)
        ref = R.solve(a, c, eps)[s]
        assert np.linalg.norm(h[s].numpy() - ref) <= tol * np.linalg.norm(ref)


def test_solve_matching_filter_one_filter_for_all_shots():
    pred, obs, _ = _matched_pair(64, 5, 8, seed=2)
    a, c = R.correlations(pred, obs, 2, 6)
    h = misfit.solve_matching_filter(torch.tensor(a), torch.tensor(c), 1e-3, per_shot=False, lag_before=2)
    one = misfit.solve_matching_filter(torch.tensor(a.sum(0, keepdims=True)), torch.tensor(c.sum(0, keepdims=True)), 1e-3,
                                       lag_before=2)
    assert tuple(h.shape) == (NSHOT, 9)
    for s in range(NSHOT):
        assert torch.equal(h[s], one[0])
    assert np.allclose(h.numpy(), R.solve(a, c, 1e-3, 2, per_shot=False), rtol=1e-12, atol=0)


def test_solve_matching_filter_zero_energy_shot_and_bad_water_level():
    pred, obs, _ = _matched_pair(64, 5, 8, seed=3)
    pred[:, 1] = 0.0
    a, c = R.correlations(pred, obs, 3, 5)
    h = misfit.solve_matching_filter(a, c, lag_before=3).numpy()
    spike = np.zeros(9)
    spike[3] = 1.0
    assert np.array_equal(h[1], spike) and np.abs(h[0]).max() > 0 and np.isfinite(h).all()
    for eps in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError):
            misfit.solve_matching_filter(a, c, eps)


def test_no_cpu_fallback_for_the_device_ops():
    x = torch.zeros(8, 2, 3)
    with pytest.raises(MifwiError):
        misfit.stf_correlations(x, x, 0, 2)
    with pytest.raises(MifwiError):
        misfit.trace_convolve(x, torch.ones(2, 3), 0)
    with pytest.raises(MifwiError):
        misfit.estimate_matching_filter(x, x, 0, 2)


def _shim():
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    return api, api.Denise(None, 0)


def test_shim_serves_inv_stf_0_and_1_only():
    api, d = _shim()
    assert d.INV_STF == 0
    d.INV_STF = 1
    d.INV_STF = 0
    for bad in (2, -1, "on"):
        with pytest.raises(MifwiError):
            d.INV_STF = bad
    with pytest.raises(MifwiError):
        d.set_stf(after=0.1, water_level=0.0)
    with pytest.raises(MifwiError):
        d.set_stf(before=-0.1)


def test_shim_inv_stf_needs_set_stf(tmp_path, monkeypatch):
    api, d = _shim()
    monkeypatch.chdir(tmp_path)
    vp = np.full((20, 30), 2000.0, dtype=np.float32)
    model = api.Model(vp, vp / 2, vp, 10.0)
    x = np.array([100.0, 200.0])
    src, rec = api.Sources(x, 0 * x + 20.0, 8.0), api.Receivers(x, 0 * x + 40.0)
    d.set_observed(np.zeros((2, 10, 2)), np.zeros((2, 10, 2)))
    d.INV_STF = 1
    with pytest.raises(MifwiError, match="set_stf"):
        d.grad(model, src, rec)
