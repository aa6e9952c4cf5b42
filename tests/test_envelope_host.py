"""The envelope objective without a GPU: the float64 definition (tests/envelope_reference.py) against scipy, against its
own transpose and central differences, the cycle-skipping pin that is the reason for the objective, and the C ABI of
``mifwi_trace_hilbert`` / ``mifwi_misfit_envelope``."""
import ctypes

import numpy as np
import pytest
import torch

import envelope_reference as R


# ---- 1-3: the Hilbert transform ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 2, 3, 5, 64, 65, 301, 1024, 1025])
def test_reference_hilbert_is_scipys_padded_hilbert(nt):
    from scipy import signal
    x = np.random.default_rng(nt).standard_normal((nt, 4))
    n = R.padded_length(nt)
    assert n >= nt and n & (n - 1) == 0 and (n == 1 or n // 2 < nt)
    want = signal.hilbert(x, N=n, axis=0).imag[:nt]
    err = np.abs(R.hilbert(x) - want).max()
    print("nt %d N %d: max |reference - scipy| %.2e" % (nt, n, err))
    assert err <= 1e-13
    if n <= 2:
        assert not R.hilbert(x).any()


@pytest.mark.parametrize("nt", [1, 2, 3, 5, 64, 65, 301, 1024, 1025])
def test_reference_transpose_is_the_negated_transform(nt):
    rng = np.random.default_rng(100 + nt)
    x, y = rng.standard_normal((nt, 3)), rng.standard_normal((nt, 3))
    lhs, rhs = float((R.hilbert(x) * y).sum()), float((x * R.hilbert(y, transpose=True)).sum())
    size = np.linalg.norm(x) * np.linalg.norm(y)
    print("nt %d: <Hx, y> = %.15e, <x, H^T y> = %.15e, difference / (|x| |y|) %.1e" % (nt, lhs, rhs, abs(lhs - rhs) / size))
    assert abs(lhs - rhs) <= 1e-13 * size
    assert np.array_equal(R.hilbert(y, transpose=True), -R.hilbert(y))


def test_reference_turns_a_cosine_into_a_sine():
    t = np.arange(256)
    err = np.abs(R.hilbert(np.cos(2 * np.pi * 5 * t / 256)) - np.sin(2 * np.pi * 5 * t / 256)).max()
    print("cos -> sin, nt = N = 256, k = 5: max error %.1e" % err)
    assert err <= 1e-12


# ---- 4: the adjoint source is the gradient -------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 2, 3, 64, 65, 1000, 1025, 4097])
def test_reference_adjoint_source_is_the_central_difference_of_the_loss(nt):
    """Step 1e-6 of the data's size in a random direction: truncation ~ 1e-12 of the first derivative, cancellation
    ~ 1e-16 / 1e-6 of the loss; the bound is 1e-5 relative."""
    s, o = R.ricker_traces(nt, 7, 2 * nt), R.ricker_traces(nt, 7, 2 * nt + 1)
    eps = 1e-3 * np.abs(o).max()
    loss, adj = R.loss_adj(s, o, eps)
    d = np.random.default_rng(nt).standard_normal(s.shape) * np.abs(s).max()
    h = 1e-6
    fd = (R.loss_adj(s + h * d, o, eps)[0] - R.loss_adj(s - h * d, o, eps)[0]) / (2 * h)
    lin = float((adj * d).sum())
    print("nt %d: loss %.6e, <adj, d> = %.9e, central difference %.9e, relative %.1e" % (nt, loss, lin, fd, abs(fd - lin) / abs(fd)))
    assert loss > 0 and abs(fd - lin) <= 1e-5 * abs(fd)


def test_a_zero_divisor_contributes_nothing():
    s, o = R.ricker_traces(65, 3, 1), R.ricker_traces(65, 3, 2)
    s[:, 1] = 0.0
    loss, adj = R.loss_adj(s, o, 0.0)
    assert np.isfinite(loss) and np.isfinite(adj).all() and not adj[:, 1].any() and adj[:, 0].any()


# ---- 5: the reason for the objective -----------------------------------------------------------------------------------
def test_envelope_loss_grows_with_the_shift_where_l2_cycle_skips():
    SHIFTS = R.SHIFTS
    env, l2 = [], []
    for k in SHIFTS:
        s, o = R.shifted_pair(k)
        env.append(R.loss_adj(s, o, 1e-3 * np.abs(o).max())[0])
        l2.append(0.5 * float(((s - o) ** 2).sum()))
    print("envelope:", ["%.4f" % v for v in env])
    print("l2      :", ["%.4f" % v for v in l2])
    assert env[0] == 0.0 and all(b > a for a, b in zip(env, env[1:]))
    assert SHIFTS[int(np.argmax(l2))] == 15 and l2[-1] < l2[5] and any(b < a for a, b in zip(l2, l2[1:]))


# ---- 6: ABI --------------------------------------------------------------------------------------------------------------
def test_envelope_symbols_are_exported_and_bound():
    from physicsbasedfwi2_amd import _lib
    lib = _lib.load()
    for name in ("mifwi_trace_hilbert", "mifwi_misfit_envelope_work_elems", "mifwi_misfit_envelope"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mifwi_version() == 7 and _lib.ENVELOPE_MAX_NT == 8192
    assert lib.mifwi_misfit_envelope_work_elems(3000, 8832) >= 2 * 8832
    assert lib.mifwi_misfit_envelope_work_elems(8193, 4) == 0 and lib.mifwi_misfit_envelope_work_elems(0, 4) == 0


def test_envelope_entry_points_refuse_bad_arguments():
    """The argument checks come before the device check: every case is -1 (MIFWI_EINVAL) with a message, GPU or not.
    The pointers are never followed."""
    from physicsbasedfwi2_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def refused(rc, word):
        msg = lib.mifwi_last_error()
        assert rc == -1 and msg and word.encode() in msg, (rc, msg)

    for x, y in ((None, q), (p, None)):
        refused(lib.mifwi_trace_hilbert(0, x, y, 8, 2, 0, None), "null")
    for nt, ntrace, word in ((0, 2, "sizes"), (8, 0, "sizes"), (-1, 2, "sizes"), (8193, 2, "longer records")):
        refused(lib.mifwi_trace_hilbert(0, p, q, nt, ntrace, 0, None), word)
        refused(lib.mifwi_misfit_envelope(0, p, p, nt, ntrace, 0.0, q, q, q, None), word)
    ok = dict(pred=p, obs=p, loss=q, adj=q, work=q)
    for missing in ("pred", "obs", "loss", "work"):
        a = dict(ok, **{missing: None})
        refused(lib.mifwi_misfit_envelope(0, a["pred"], a["obs"], 8, 2, 0.0, a["loss"], a["adj"], a["work"], None), "null")
    for eps in (-1e-30, float("nan"), float("inf"), -float("inf")):
        refused(lib.mifwi_misfit_envelope(0, p, p, 8, 2, eps, q, q, q, None), "eps")
    refused(lib.mifwi_misfit_envelope(0, p, p, 8, 2, 0.0, q, q, ctypes.c_void_p(8196), None), "aligned")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_envelope_fails_loudly_without_a_device():
    from physicsbasedfwi2_amd import _lib, misfit
    from physicsbasedfwi2_amd._lib import MifwiError
    lib = _lib.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert lib.mifwi_trace_hilbert(0, p, q, 8, 2, 0, None) == -2 and b"no CPU fallback" in lib.mifwi_last_error()
    assert lib.mifwi_misfit_envelope(0, p, p, 8, 2, 0.0, q, None, q, None) == -2
    x = torch.ones(8, 2)
    for call in (lambda: misfit.envelope(x, x), lambda: misfit.envelope(x, x, eps=0.1), lambda: misfit.trace_hilbert(x),
                 lambda: misfit.trace_envelope(x, 0.1), lambda: misfit.envelope(x, x, sos=misfit.butterworth_sos(0.002, 0.0, 10.0))):
        with pytest.raises(MifwiError):
            call()
