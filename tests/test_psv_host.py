"""What the tests of the VTI, viscoelastic and TTI kernels rely on, checked without a GPU: the yardstick (tests/psv_reference.py)
on the axes tests/test_vti_host.py and tests/test_visco_host.py do not reach - point forces and four-tap points - against
the fp64 C oracle in each medium's limit, the tile widths the cases of tests/psv_media.py are meant to run at, and what
the draws of tests/test_psv_fuzz_gpu.py cover.  Bounds as in test_vti_host.py: 1e-10 rel-L2 on the traces, 1e-9 on every
gradient (two float64 statements of one recursion that sum in different orders).
Measured: traces <= 1.1e-15, gradients <= 3.7e-15."""
import numpy as np
import pytest

import psv_media as M
import psv_reference as R
from cases import elastic_case, elastic_case_taps4, rel_l2
from tti_reference import MEDIA3

RELAX = (0.9, 0.1)             # any pair inside (0, 1): with planes 5-7 zero it must not matter
_cache = {}


def _oracle(key, c, st, order):
    """The fp64 oracle on the case: traces, a seeded adjoint source, gradients; once per case."""
    if key not in _cache:
        import oracle
        o64 = oracle.load("f64")
        geo = (c["sc"], c["sw"], c["rc"], c["rw"])
        ovx, ovz, S = o64.elastic_forward(c["mat"], c["pz"], c["px"], c["f"], *geo, save=True, free_surface=c["fs"],
                                          source_type=st, fd_order=order)
        rng = np.random.default_rng(7)
        g = [rng.standard_normal(a.shape) * np.abs(a).max() for a in (ovx, ovz)]
        gm, gf = o64.elastic_backward(c["mat"], c["pz"], c["px"], *geo, g[0], g[1], S, free_surface=c["fs"], source_type=st,
                                      fd_order=order)
        _cache[key] = ovx, ovz, g, gm, gf
    return _cache[key]


def _check_limit(medium, key, c, st, order):
    m = MEDIA3[medium]
    ovx, ovz, g, gm, gf = _oracle(key, c, st, order)
    rvx, rvz, gp, rgf = R.gradients(m.limit(c["mat"]), c["pz"], c["px"], c["f"], c["sc"], c["sw"], c["rc"], c["rw"], g[0], g[1],
                                    medium, RELAX if m.takes_relax else None, free_surface=c["fs"], fd_order=order,
                                    source_type=st)
    err = rel_l2(np.stack([rvx, rvz]), np.stack([ovx, ovz]))
    print("%s seismograms rel-L2 %.2e" % (m.limit_label, err))
    assert np.abs(ovx).max() > 0 and np.abs(ovz).max() > 0
    assert err <= 1e-10
    want = {"L": gm[0], "M": gm[1], "mu": gm[2], "bx": gm[3], "bz": gm[4], "f": gf}
    got = dict(m.iso(gp), f=rgf)
    assert set(got) == set(want)
    for k in want:
        e = rel_l2(got[k], want[k])
        print("gradient %s rel-L2 %.2e" % (k, e))
        assert np.abs(want[k]).max() > 0, k
        assert e <= 1e-9, k


# ---- 1: the reference against oracle64 in each medium's limit, force sources and four-tap points ---------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("st", [1, 2], ids=["fx", "fz"])
@pytest.mark.parametrize("medium", list(MEDIA3))
def test_reference_with_a_force_source_is_the_oracle_in_the_limit(medium, st, fs, order):
    c = elastic_case(seed=4, free_surface=fs)
    c["f"] = c["f"] * 1e-3                               # as the elastic sweep scales a force's amplitudes
    _check_limit(medium, ("force", st, fs, order), c, st, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("medium", list(MEDIA3))
def test_reference_with_four_tap_points_is_the_oracle_in_the_limit(medium, fs, order):
    _check_limit(medium, ("taps4", fs, order), elastic_case_taps4("T", 21, free_surface=fs), 0, order)


# ---- 2: the cases sit on the tile widths they were made for ----------------------------------------------------------------
def test_cases_run_at_the_three_tile_widths():
    """A later change of the plan's rule (or of a case) cannot move the cases off their widths unnoticed."""
    want = {"A": 16, "A_fw0": 16, "A_fs": 16, "B": 16, "C": 32, "C_fw0": 32, "D": 64, "D_fs": 64}
    assert {name: M.width(name) for name in M.CASES} == want
    groups = {name: -(-M.CASES[name].get("nx", 60) // 4) for name in ("A", "B", "C", "D")}
    assert groups == {"A": 15, "B": 38, "C": 30, "D": 58}
    assert [M.CASES[n]["nx"] % 4 for n in ("C", "D")] == [1, 2]
    # the rule itself at its edges: 32 for 27 ... 32 groups, 64 from 54 on
    assert [M.pick_lx(ng) for ng in (26, 27, 32, 33, 53, 54, 64, 65)] == [16, 32, 32, 16, 16, 64, 64, 16]


# ---- 3: the draws of the sweep ---------------------------------------------------------------------------------------------
def test_fuzz_draws_of_the_psv_media_cover_what_they_are_meant_to():
    """The committed draws of test_psv_fuzz_gpu.test_random_configuration (that module carries the gpu mark)."""
    import test_psv_fuzz_gpu
    test_psv_fuzz_gpu.test_draws_cover_widths_sources_taps_and_driver_forms()
    assert list(test_psv_fuzz_gpu.MEDIA) == ["vti", "visco", "tti"]


@pytest.mark.parametrize("k", range(12))
def test_fuzz_draws_meet_the_preconditions_of_the_tilted_medium(k):
    """The sweep's ``preconditions`` for TTI with the reference alone, draw by draw: nothing compared is all zero, the medium
    moves some live shot by more than 1 % from its isotropic limit and the tilt by more than 1 % from theta = 0.  (Those of
    VTI and the viscoelastic medium chose PSV_SEED; TTI meets its own on the same seed.)"""
    import test_psv_fuzz_gpu as F
    _, cfg, opt = F._configs()[k]
    moved = F.preconditions(MEDIA3["tti"], cfg, opt["order"])
    print("draw %d: moved from the limit %.3f, from theta = 0 %.3f" % (k, moved, F.tilt_moved(cfg, opt["order"])))
