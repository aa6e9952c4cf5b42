"""The TTI kernels (tti_strain, tti_stress, tti_adj_e, tti_adj_s of csrc/mifwi_tti.h) where their footprints can go wrong:
on the inclusion grids of tests/tti_reference.py, whose fluid blocks put edges of the mask w = (c55_xz != 0) on every
column phase of a four-cell group, across the column and row seams of the forward and adjoint tiles, into the partial last
group and under the water layer.  tests/test_tti_host.py shows with the reference alone that a mask read one column or one
row off moves the traces of these grids by at least 1.3e-3 rel-L2 and every gradient plane by at least 4.2e-4 - and on the
layered cases of tests/test_tti_gpu.py, for the column, by exactly nothing.

I-16 = 44 x 150 (16 lanes per row, forward tiles 16 rows x 64 columns), I-32 = 41 x 117 (32 lanes, 8 x 128, nx % 4 = 1, no
absorbing layer), I-64 = 35 x 230 (64 lanes, 4 x 256, nx % 4 = 2); two shots, 120 steps, orders 2 and 4.  I-16 also forced
to 32 and 64 lanes, with row-major and blocked snapshot planes, in three time-checkpoint segments (the strains then go
through the work planes) and with one shot per accumulator group; I-64 also under a free surface with fz sources, with
four-tap fx sources and with four-tap explosive sources, shot 0 recorded on the buried line.

Bounds, the project's for a medium on these kernels: traces and Born within TOL_TRACE = 2e-6 of the float64 reference,
every gradient and grad_f within max(TOL_SUM, 4 E_iso), E_iso measured in the same test on the isotropic kernels
(psv_media.check_traces_and_gradients_match_the_reference), <J dm, g> = <dm, J^T g> within TOL_SUM = 2e-5 of the sum of
the absolute terms.

Measured on the MI355X (records, not bounds).  The three grids, both orders: traces 9.3e-8 ... 1.7e-7, gradients 8.6e-8 ...
1.1e-6 (the largest: c11 on I-64 at order 2; bx on I-16 at order 4 1.0e-6), E_iso <= 9.6e-7, so the bound in force was 2e-5
everywhere; Born 1.9e-7 ... 5.2e-7 (the largest on I-64 at order 2); <J dm, g> - <dm, J^T g> over the sum of the absolute
terms 1.7e-9 ... 7.4e-8 (the largest: the tilt's two planes alone on I-16 at order 2).  I-16 at 32 and 64 lanes: traces, all
gradients and Born the same bits as at 16 lanes; row-major against blocked snapshot planes: the same figures against the
reference, the traces the same bits; three checkpoint segments: the resident run's bits; one shot per accumulator group:
gradients <= 2.2e-12 from the default's.  I-64 under a free surface: traces 6.9e-8 ... 1.9e-7, gradients <= 1.2e-6 (the
largest: c55 with fz sources at order 4; fx with four-tap points <= 9.5e-7, c11), E_iso <= 7.4e-7, Born with four-tap points
1.6e-7 and 2.3e-7."""
import numpy as np
import pytest
import torch

import psv_media as M
import tti_reference as T
from cases import rel_l2
from psv_media import TOL_SUM, TOL_TRACE

pytestmark = pytest.mark.gpu
TTI = T.TTI
GRIDS = list(T.INCLUSIONS)


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


def _born_matches(spec, order, what):
    c = M.case(TTI, spec)
    want = M.ref_jvp(TTI, spec, order)
    _, _, dvx, dvz = M.born(TTI, c, order)
    err = rel_l2(M.pair(dvx, dvz), want)
    print("tti.born vs central difference of the reference, %s order %d: rel-L2 %.3e" % (what, order, err))
    assert np.abs(want).max() > 0
    assert err <= TOL_TRACE
    return err


# ---- the three grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_traces_and_gradients_match_the_reference_around_fluid_blocks(name, order):
    T.inclusion_case(name)
    M.check_traces_and_gradients_match_the_reference(TTI, T.inclusion(name), order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_born_is_the_directional_derivative_of_the_reference(name, order):
    """Born's second footprint (dmat8 on the background's strains) uses the background's w."""
    T.inclusion_case(name)
    _born_matches(T.inclusion(name), order, name)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_born_and_the_adjoint_are_transposes(name, order):
    """<J dm, g> = <dm, J^T g>, for all eight planes and for the two planes of the tilt alone: sums of terms of both signs,
    held to TOL_SUM of their absolute sum (as test_tti_gpu.test_born_dot_products_gauss_newton_and_the_force_refusal)."""
    c = T.inclusion_case(name)
    dev, dot = M.dev, M.dot
    rvx, rvz, mvx, mvz = M.born(TTI, c, order)
    g = M.g_of(rvx.cpu().numpy(), rvz.cpu().numpy())
    _, _, gm, _ = M.run(TTI, c, c["matm"], order, g)
    only = np.array(c["dmat"])
    only[:6] = 0.0
    _, _, qvx, qvz = M.born(TTI, c, order, dmat=dev(only))
    assert float(mvx.abs().max()) > 0 and float(qvx.abs().max()) > 0 and np.abs(gm[6:]).max() > 0
    for what, (dvx, dvz), dm in (("dm", (mvx, mvz), np.asarray(c["dmat"])), ("dc15, dc35", (qvx, qvz), only)):
        lhs, rhs = dot(dvx, dev(g[0])) + dot(dvz, dev(g[1])), float((gm * dm).sum())
        size = float(np.abs(gm * dm).sum())
        print("%s order %d, %s: <J dm, g> = %.9e, <dm, J^T g> = %.9e, sum |terms| = %.3e, |diff| / sum = %.2e"
              % (name, order, what, lhs, rhs, size, abs(lhs - rhs) / size))
        assert size > 0 and abs(lhs - rhs) <= TOL_SUM * size


# ---- I-16: the other tile widths, both snapshot layouts, the work planes, shot groups -----------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("lx", [32, 64])
def test_forced_tile_width_matches_the_reference(monkeypatch, lx, order):
    """At 32 lanes the block of columns 126 ... 130 lies across the forward tiles' seam 127|128; at 64 lanes the 38 groups
    are one partial tile column of 4-row tiles"""
    T.inclusion_case("I-16")
    M.check_forced_width(TTI, monkeypatch, T.inclusion("I-16"), lx, order)


@pytest.mark.parametrize("order", [2, 4])
def test_row_major_and_blocked_snapshot_planes_give_the_same_traces(monkeypatch, order):
    """The strain planes have the snapshot planes' layout: tti_row5<kLaySnap> takes its fifth value from
    snap_cell(p, j, g +- 1) in either.  Both layouts against the reference, and the traces of the two the same bits."""
    T.inclusion_case("I-16")
    tr = {}
    for blocked in (0, 1):
        monkeypatch.setenv("MIFWI_EL_SNAP_BLOCKED", str(blocked))
        print("MIFWI_EL_SNAP_BLOCKED=%d" % blocked)
        _, (tr[blocked], _, _) = M.check_traces_and_gradients_match_the_reference(TTI, T.inclusion("I-16"), order)
        _born_matches(T.inclusion("I-16"), order, "I-16 blocked %d" % blocked)
    assert np.abs(tr[0]).max() > 0 and np.array_equal(tr[0], tr[1])


def test_time_checkpoints_and_shot_groups(monkeypatch):
    """Three time-checkpoint segments: the forward pass writes its strains to the work planes, a segment's re-run to its
    snapshot planes; the same values either way and the adjoint reads the same planes in the same order: held to the
    reference and to the resident run's bits, traces and gradients (test_tti_gpu.test_time_checkpoints_and_repeats_give_
    the_same_bits).  One shot per accumulator group: held to the reference, the traces to the same bits."""
    c = T.inclusion_case("I-16")
    spec = T.inclusion("I-16")
    g = M.ref(TTI, spec, 4, "matm")["g"]
    bvx, bvz, bg, bgf = M.run(TTI, c, c["matm"], 4, g)
    base_tr = M.pair(bvx, bvz)
    assert np.abs(base_tr).max() > 0 and np.abs(bg).max() > 0
    _, (tr, vg, vgf) = M.check_traces_and_gradients_match_the_reference(TTI, spec, 4, segments=3)
    assert np.array_equal(tr, base_tr) and np.array_equal(vg, bg) and np.array_equal(vgf, bgf)
    _, (tr, vg, vgf) = M.check_traces_and_gradients_match_the_reference(TTI, spec, 4, shots_per_group=1)
    assert np.array_equal(tr, base_tr)
    errs = [rel_l2(vg[k], bg[k]) for k in range(8)] + [rel_l2(vgf, bgf)]
    print("shots_per_group 1 vs 0: gradients rel-L2 %s" % ["%.1e" % e for e in errs])
    assert max(errs) <= TOL_SUM


# ---- I-64 under a free surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("more", [dict(source_type=2), dict(source_type=1, ntap=4), dict(ntap=4)], ids=["fz", "fx_taps4", "taps4"])
def test_free_surface_force_sources_and_four_tap_points(more, order):
    """drop_row0 of tti_At (the adjoint szz of row 0 counts as 0) with sources that load the surface row, bilinear four-tap
    sources and receivers, shot 0 recorded on the buried line; Born where the source is explosive."""
    more = dict(T.FREE_SURFACE, **more)
    c = T.inclusion_case("I-64", **more)
    assert c["fs"] == 1
    M.check_traces_and_gradients_match_the_reference(TTI, T.inclusion("I-64", **more), order)
    if c["st"] == 0:
        _born_matches(T.inclusion("I-64", **more), order, "I-64 under a free surface, four-tap points")
