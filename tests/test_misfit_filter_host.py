"""misfit.butterworth_sos: the second-order sections of a frequency stage (add_fwi_stage(fc_low, fc_high, order)) are
scipy.signal.butter's, low-pass first, with the rules of compat.pyapi_denise.butterworth for absent corners."""
import numpy as np
import pytest
from scipy import signal

from physicsbasedfwi2_amd import _lib, misfit


def _expected(dt, lo, hi, order):
    fnyq = 0.5 / dt
    parts = []
    if hi > 0:
        parts.append(signal.butter(order, hi / fnyq, "lowpass", output="sos"))
    if lo > 0:
        parts.append(signal.butter(order, lo / fnyq, "highpass", output="sos"))
    return np.concatenate(parts, axis=0)


# the three stages the reference uses (networks.py:7761, 9863, 10503) and an odd order (one section has a single pole: a2 = 0)
@pytest.mark.parametrize("dt,lo,hi,order", [(0.002, 0.0, 10.0, 6), (0.0025, 2.0, 12.0, 6), (0.002, 3.0, 10.0, 6),
                                            (0.002, 3.0, 10.0, 5), (0.002, 0.0, 10.0, 5)])
def test_sections_are_scipys(dt, lo, hi, order):
    sos = misfit.butterworth_sos(dt, fc_low=lo, fc_high=hi, order=order)
    ref = _expected(dt, lo, hi, order)
    assert sos.dtype == np.float64 and sos.flags.c_contiguous and sos.shape == ref.shape
    assert sos.shape == (((order + 1) // 2) * ((lo > 0) + (hi > 0)), 6)
    assert np.array_equal(sos, ref)
    assert np.all(sos[:, 3] == 1.0)                      # a0 = 1: what mifwi_trace_filter requires
    if order % 2:
        assert np.any(sos[:, 5] == 0.0)                   # the real pole of an odd order: a section with a2 = 0


def test_nothing_to_filter_is_none():
    assert misfit.butterworth_sos(0.002) is None
    assert misfit.butterworth_sos(0.002, fc_low=0.0, fc_high=0.0) is None
    assert misfit.butterworth_sos(0.002, fc_low=-1.0, fc_high=None) is None
    assert misfit.butterworth_sos(0.002, fc_high=250.0) is None          # low-pass at Nyquist
    assert misfit.butterworth_sos(0.002, fc_high=400.0) is None          # ... and above
    # the high-pass survives a dropped low-pass
    assert np.array_equal(misfit.butterworth_sos(0.002, fc_low=3.0, fc_high=250.0), _expected(0.002, 3.0, 0.0, 6))


def test_too_many_sections_raise():
    assert _lib.FILTER_MAX_SECTIONS == 8
    assert misfit.butterworth_sos(0.002, 3.0, 10.0, order=8).shape == (8, 6)
    with pytest.raises(ValueError):
        misfit.butterworth_sos(0.002, 3.0, 10.0, order=10)
    with pytest.raises(ValueError):
        misfit.butterworth_sos(0.002, 0.0, 10.0, order=17)
