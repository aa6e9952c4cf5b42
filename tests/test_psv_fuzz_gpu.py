"""Seeded sweep over small random configurations of the VTI, viscoelastic and TTI propagators: grids on all three forward tile
widths and every nx % 4, C-PML widths 0 / 3 / 5 / 8, free surface, explosive and point-force sources, one-tap and bilinear
four-tap points, both stencil orders, shots per accumulator group, forced shot and group passes over the time range, time
checkpoints, row-major snapshot planes and every tile -> XCD order.  Twelve draws, the same for all three media; the planes
of a medium are the smooth seeded fields of tests/psv_media.py (TTI: of tests/tti_reference.py) on the draw's grid.

Per draw and medium: the checks of tests/test_psv_media_gpu.py on the draw (psv_media.check_traces_and_gradients_match_
the_reference: traces within 2e-6 rel-L2 of the float64 reference tests/psv_reference.py, every plane's gradient and grad_f
within max(2e-5, 4 E_iso), E_iso the error of elastic.propagate in the medium's limit on the same draw and options), and for
explosive sources Born against the central difference of the reference within 2e-6.

PSV_SEED and the CPU preconditions it was chosen by stand below.  The reference's traces in the medium against those in
its limit, rel-L2 of the live shot that moved most, draw by draw (``preconditions``; printed once on the CPU):
  vti   0.574 0.450 0.035 0.233 2.749 0.751 0.130 0.108 0.212 0.076 0.102 6.374
  visco 0.072 0.083 0.063 0.067 0.042 0.079 0.084 0.055 0.073 0.108 0.087 0.106
  tti   1.901 1.312 0.050 0.191 18.57 1.032 0.201 0.234 0.776 0.133 0.837 9.191
(more than 1 where a draw's steps end in the precursor of the wave, whose shape the anisotropy changes altogether).  TTI
passes on the same seed, so the three media share their draws; its tilted reference against its reference at theta = 0:
  tilt  0.847 0.597 0.080 0.227 4.243 0.295 0.235 0.222 0.859 0.135 0.983 1.457
Measured on the MI355X over the twelve draws, VTI: traces 4.0e-8 ... 3.0e-7, gradients 6.7e-8 ... 1.7e-6, Born (five
draws) 7.3e-8 ... 2.1e-7; viscoelastic: traces 5.8e-8 ... 3.0e-7, gradients 4.2e-8 ... 2.5e-6, Born 2.1e-7 ... 9.5e-7;
E_iso <= 2.1e-6, so the bound in force was 2e-5 everywhere.  By path, VTI / viscoelastic - 32 lanes: traces <= 1.1e-7 /
1.7e-7, gradients <= 1.7e-6 / 2.5e-6; 64 lanes: traces <= 1.2e-7 / 7.6e-8, gradients <= 4.8e-7 / 1.1e-6; force sources (eight
draws): traces <= 3.0e-7 / 3.0e-7, gradients <= 1.7e-6 / 2.5e-6; four-tap points (seven draws): traces <= 1.1e-7 / 1.7e-7,
gradients <= 1.7e-6 / 2.5e-6.  The largest gradient errors are those of bx on draw 10 (four-tap fz sources under a free
surface, order 2, three checkpoint segments), where the isotropic kernels' own bx gradient is 2.1e-6 from the reference.
TTI over the same twelve draws: traces 3.8e-8 ... 2.9e-7 (the largest on draw 0), gradients 7.5e-8 ... 2.5e-6 (bx on draw 10
again, c11 1.1e-6 there; every other draw <= 7.1e-7), Born (the four draws with explosive sources) 7.0e-8 ... 2.8e-7, E_iso <= 2.1e-6."""
import numpy as np
import pytest

import psv_media as M
from cases import rel_l2
from psv_media import TOL_TRACE
from tti_reference import MEDIA3 as MEDIA

pytestmark = pytest.mark.gpu

# Chosen on the CPU: the first seed from 2051 on whose twelve draws pass test_draws_cover_widths_sources_taps_and_driver_forms
# and on which the reference alone meets ``preconditions`` on every draw, for all three media.
PSV_SEED = 2051
LIVE = 1e-3                     # a shot counts where its reference traces hold this share of the draw's largest shot norm
BANDS = ((40, 105), (105, 129), (213, 257))       # nx: 10 ... 26 groups (16 lanes), 27 ... 32 (32 lanes), 54 ... 64 (64 lanes)


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


def _configs(seed=PSV_SEED):
    rng = np.random.default_rng(seed)
    pairs = rng.permutation(12) % 6                # every (source type, free surface) pair twice
    out = []
    for k in range(12):
        fw, fs = int(rng.choice([0, 3, 5, 8])), bool(pairs[k] // 3)
        # under a free surface elastic_case shoots shot 0 from row 0 in the water, where nothing propagates, and records it
        # there: its source's own injection, 1e5 times what any other shot records, which never sees the medium (psv_media.
        # check_traces_and_gradients_match_the_reference).  Here such a draw has a second shot and records shot 0 on the
        # buried line of the others (all zero unless it has a second, deeper source), so that the pooled trace error is the
        # live shots'.  90 steps and more: the wavelet's peak leaves the source at step 75
        cfg = dict(seed=500 + k, surface_receivers=False, nx=int(rng.integers(*BANDS[k % 3])), fw=fw, nz=int(rng.integers(max(30, 2 * fw + 22), 70)),
                   ns=int(rng.integers(2 if fs else 1, 5)), nsrc=int(rng.integers(1, 3)), nrec=int(rng.integers(1, 13)),
                   nt=int(rng.integers(90, 120)), free_surface=fs, source_type=int(pairs[k] % 3),
                   ntap=int(rng.choice([1, 1, 4])))
        # segments 0: the default snapshot budget (resident snapshots); 3: a budget that holds a third of the steps
        opt = dict(order=int(rng.choice([2, 4])), gs=int(rng.integers(0, 4)), pass_shots=int(rng.integers(1, 4)),
                   pass_groups=int(rng.integers(1, 3)), segments=int(rng.choice([0, 0, 3])), blocked=int(rng.integers(0, 2)),
                   xcd=int(rng.integers(0, 4)))
        out.append((k, cfg, opt))
    return out


def test_draws_cover_widths_sources_taps_and_driver_forms(draws=None):
    """Needs no GPU (tests/test_psv_host.py runs it there)."""
    draws = _configs() if draws is None else draws
    assert len(draws) == 12
    widths = [M.width(cfg) for _, cfg, _ in draws]
    assert all(widths.count(lx) >= 3 for lx in (16, 32, 64)), widths
    assert {cfg["nx"] % 4 for _, cfg, _ in draws} == {0, 1, 2, 3}
    assert {(cfg["source_type"], cfg["free_surface"]) for _, cfg, _ in draws} == {(st, fs) for st in range(3) for fs in (False, True)}
    assert {opt["order"] for _, _, opt in draws} == {2, 4}
    taps = [cfg["ntap"] for _, cfg, _ in draws]
    assert set(taps) == {1, 4} and taps.count(1) >= 3 and taps.count(4) >= 3, taps
    assert sum(opt["segments"] > 0 for _, _, opt in draws) >= 2
    assert sum(opt["pass_shots"] < cfg["ns"] and cfg["ns"] % opt["pass_shots"] != 0 for _, cfg, opt in draws) >= 2
    assert any(cfg["ntap"] == 4 and cfg["source_type"] != 0 for _, cfg, _ in draws)
    assert any(lx == 64 and cfg["source_type"] == 0 for lx, (_, cfg, _) in zip(widths, draws))       # Born at 64 lanes
    assert all(cfg["nz"] <= 69 and cfg["nx"] <= 256 and cfg["ns"] <= 4 and cfg["nt"] < 120 for _, cfg, _ in draws)


def preconditions(m, cfg, order):
    """What the reference alone must hold on a draw before the kernels are compared with it: no compared trace set,
    gradient plane or grad_f all zero (Born's traces where the source is explosive), and the medium's traces more than 1 %
    from its limit's in some live shot; for TTI also the tilted reference more than 1 % from the reference at theta = 0
    (the VTI reference of the same Thomsen fields) in some live shot, as test_tti_gpu.test_the_tilt_moves_the_traces asks.
    Returns the rel-L2 from the limit of the shot that moved most."""
    ref = M.ref(m, cfg, order, "matm")
    for k in ("rvx", "rvz", "f") + m.planes:
        assert np.abs(ref[k]).max() > 0, k
    if cfg["source_type"] == 0:
        assert np.abs(M.ref_jvp(m, cfg, order)).max() > 0
    moved = max(M.moved_from_the_limit(m, cfg, order, LIVE))
    assert moved > 0.01, moved
    if m.name == "tti":
        assert tilt_moved(cfg, order) > 0.01
    return moved


def tilt_moved(cfg, order):
    """rel-L2 between the TTI reference's traces and the VTI reference's (theta = 0) on the draw, the live shot that moves most"""
    tilted, flat = M.ref(MEDIA["tti"], cfg, order, "matm"), M.ref(MEDIA["vti"], cfg, order, "matm")
    a, b = np.stack([tilted["rvx"], tilted["rvz"]]), np.stack([flat["rvx"], flat["rvz"]])
    return max(rel_l2(a[:, :, s], b[:, :, s]) for s in M.live_shots(a, LIVE))


@pytest.mark.parametrize("medium", list(MEDIA))
@pytest.mark.parametrize("k,cfg,opt", _configs(), ids=["draw%d" % k for k in range(12)])
def test_random_configuration(monkeypatch, k, cfg, opt, medium):
    m = MEDIA[medium]
    order, gs = opt["order"], opt["gs"]
    print("draw %d at %d lanes: %s %s" % (k, M.width(cfg), cfg, opt))
    M.setenv(monkeypatch, {"MIFWI_EL_PASS_SHOTS": str(opt["pass_shots"]), "MIFWI_EL_PASS_GROUPS": str(opt["pass_groups"]),
                           "MIFWI_EL_SNAP_BLOCKED": str(opt["blocked"]), "MIFWI_EL_XCD": str(opt["xcd"])})
    c = M.case(m, cfg)
    preconditions(m, cfg, order)
    pl = M.plan(m, c, order=order, gs=gs)
    assert pl.pass_sizes() == (min(opt["pass_shots"], cfg["ns"]), min(opt["pass_groups"], pl.layout.ngroups))
    assert pl.cluster_slabs(False) == 0 and pl.cluster_slabs(True) == 0
    pl.close()
    M.check_traces_and_gradients_match_the_reference(m, cfg, order, floor=LIVE, segments=opt["segments"], shots_per_group=gs)
    if cfg["source_type"] == 0:
        want = M.ref_jvp(m, cfg, order)
        _, _, dvx, dvz = M.born(m, c, order)
        err = rel_l2(M.pair(dvx, dvz), want)
        print("%s.born vs central difference of the reference, draw %d order %d: rel-L2 %.3e" % (m.name, k, order, err))
        assert err <= TOL_TRACE
