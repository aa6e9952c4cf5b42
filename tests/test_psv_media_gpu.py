"""The P-SV media beyond the isotropic one on the GPU - VTI (physicsbasedfwi2_amd.vti, mifwi_vti_*), viscoelastic
(physicsbasedfwi2_amd.visco, mifwi_visco_*) and TTI (physicsbasedfwi2_amd.tti, mifwi_tti_*; its entry and its stress
update come from tests/tti_reference.py) - against their yardstick tests/psv_reference.py (float64; pinned to the fp64
C oracle in the isotropic limit, to Thomsen's kinematics and to the attenuation law of a standard linear solid by
tests/test_vti_host.py and tests/test_visco_host.py): Born, its identities and the driver forms, once for both media.  The
limit and the parity with the reference are check_limit_is_the_elastic_propagator and
check_traces_and_gradients_match_the_reference of tests/psv_media.py, run under their earlier names by
tests/test_vti_gpu.py and tests/test_visco_gpu.py, which also hold what each medium has of its own; the cases and what
differs between the media are in tests/psv_media.py.

Stencil orders 2 and 4.  Bounds: 2e-6 rel-L2 for an f32 recursion against its fp64 reference (the project's bound; measured
6.1e-7 on the isotropic kernels), 2e-5 for gradients summed in another order, and for the gradients of the new medium
max(2e-5, 4 E_iso) with E_iso the error of today's isotropic kernels against the same reference in the isotropic limit on
the same geometry, measured in the same test and printed.
Measured on the MI355X, VTI: traces 7.2e-8 ... 5.0e-7, gradients <= 1.1e-6, E_iso 5.4e-8 ... 8.5e-7, Born 1.9e-7 ... 1.8e-6
(the largest on B at order 2, whose 50 steps record only the precursor of the wave), identities <= 7.9e-6.
Viscoelastic: the elastic limit's traces and gradients the same bits as elastic.propagate's; attenuating traces
8.2e-8 ... 3.3e-7 from the reference (and 2 ... 7 % from the elastic reference, the live shots), gradients of the eight planes
and of f 4.6e-8 ... 1.14e-6, E_iso 5.4e-8 ... 8.5e-7 (so the bound in force was 2e-5 everywhere); Born 1.8e-7 ... 6.8e-7;
identities 2.5e-8 ... 9.8e-6; time checkpoints and shot groups: gradients <= 3.3e-7 from the resident run, traces the same
bits.
Shapes: A and B run at 16 lanes per row, C (41 x 117) at 32, D (35 x 230) at 64 (tests/psv_media.py;
tests/test_psv_host.py pins the widths).  On C, C_fw0, D and D_fs, VTI: traces 3.5e-8 ... 4.0e-7, gradients 8.7e-8 ... 1.1e-6,
Born 3.0e-8 ... 4.1e-7; viscoelastic: traces 4.3e-8 ... 1.6e-7, gradients 4.2e-8 ... 5.7e-7, Born 2.1e-8 ... 1.9e-7; E_iso
<= 5.4e-7.  A and B forced to 32 and 64 lanes (MIFWI_EL_LX; test_forced_tile_width_matches_the_reference of the media's own
files): traces, gradients and Born the same bits as at 16 lanes.  Random configurations: tests/test_psv_fuzz_gpu.py.
TTI, the same three tests: Born on the eight cases 7.1e-8 ... 7.6e-7 (the largest on B at order 4); identities 6.7e-9 ...
1.0e-5 (the largest <H a, b> = <a, H b> on B, whose terms are of size 1e-24); time checkpoints the resident run's bits,
shot groups <= 3.4e-7 from it, Born in shot chunks the same bits."""
import numpy as np
import pytest
import torch

import psv_media as M
from cases import rel_l2
from psv_media import CASES, TOL_SUM, TOL_TRACE
from tti_reference import MEDIA3 as MEDIA

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


# ---- Born ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("medium", list(MEDIA))
def test_born_is_the_directional_derivative_of_the_reference(medium, name, order):
    m = MEDIA[medium]
    c = M.case(m, name)
    want = M.ref_jvp(m, name, order)
    _, _, dvx, dvz = M.born(m, c, order)
    got = M.pair(dvx, dvz)
    err = rel_l2(got, want)
    print("%s.born vs central difference of the reference, %s order %d: rel-L2 %.3e" % (m.name, name, order, err))
    assert np.abs(want).max() > 0
    assert err <= TOL_TRACE


@pytest.mark.parametrize("name", ["A", "A_fs", "B", "D"])
@pytest.mark.parametrize("medium", list(MEDIA))
def test_born_background_dot_products_and_gauss_newton(medium, name):
    m = MEDIA[medium]
    c = M.case(m, name)
    order = 4
    dev, dot, close = M.dev, M.dot, M.close
    mat = dev(c["matm"])
    rvx, rvz, dvx, dvz = M.born(m, c, order, df=dev(c["df"]))
    pvx, pvz = M.run(m, c, c["matm"], order)
    assert torch.equal(rvx, pvx) and torch.equal(rvz, pvz)                         # the background traces
    # <J (dm, df), g> = <dm, J^T g> + <df, J^T g>
    g = [dev(a) for a in M.g_of(rvx.cpu().numpy(), rvz.cpu().numpy())]
    _, _, gm, gf = M.run(m, c, c["matm"], order, [a.cpu().numpy() for a in g])
    _, _, mvx, mvz = M.born(m, c, order)                                           # dm alone
    close(dot(mvx, g[0]) + dot(mvz, g[1]), float((gm * c["dmat"]).sum()), TOL_SUM, "<J dm, g> vs <dm, J^T g>")
    # the planes the medium adds to the elastic five, alone: their Born terms against their gradients
    only = np.array(c["dmat"])
    only[:5] = 0.0
    _, _, qvx, qvz = M.born(m, c, order, dmat=dev(only))
    assert float(qvx.abs().max()) > 0
    # (a sum of terms of both signs that partly cancel: the f32 gradients' error, bounded by TOL_SUM per plane, is relative
    # to the terms, so this identity is held to TOL_SUM of their absolute sum)
    lhs, rhs, size = dot(qvx, g[0]) + dot(qvz, g[1]), float((gm[5:] * only[5:]).sum()), float(np.abs(gm[5:] * only[5:]).sum())
    print("<J dR, g> = %.9e, <dR, J^T g> = %.9e, sum |terms| = %.3e, |diff| / sum = %.2e" % (lhs, rhs, size, abs(lhs - rhs) / size))
    assert abs(lhs - rhs) <= TOL_SUM * size
    zero = torch.zeros_like(mat)
    _, _, fvx, fvz = M.born(m, c, order, dmat=zero, df=dev(c["df"]))               # df alone
    close(dot(fvx, g[0]) + dot(fvz, g[1]), float((gf * c["df"]).sum()), TOL_SUM, "<J df, g> vs <df, J^T g>")
    assert rel_l2(M.pair(mvx + fvx, mvz + fvz), M.pair(dvx, dvz)) <= TOL_TRACE     # J is linear
    # Gauss-Newton: <H a, b> = <a, H b>
    a = M.args(c, mat) + M.extra(m, c)
    kw = dict(free_surface=bool(c["fs"]), fd_order=order)
    other = dev(M.f32(0.01 * np.random.default_rng(5).standard_normal(c["matm"].shape) * c["matm"]))
    gauss_newton_product = M.module(m).gauss_newton_product
    ha, hvx, hvz = gauss_newton_product(a[0], dev(c["dmat"]), *a[1:], **kw)
    hb, _, _ = gauss_newton_product(a[0], other, *a[1:], **kw)
    assert ha.shape == mat.shape and torch.equal(hvx, mvx) and torch.equal(hvz, mvz)
    close(dot(ha, other), dot(hb, dev(c["dmat"])), TOL_SUM, "<H a, b> vs <a, H b>")
    close(dot(ha, dev(c["dmat"])), dot(mvx, mvx) + dot(mvz, mvz), TOL_SUM, "<H a, a> vs |J a|^2")


# ---- driver forms: time checkpoints, shot groups, shot chunks, repeats -------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "D"])
@pytest.mark.parametrize("medium", list(MEDIA))
def test_checkpoints_groups_chunks_and_repeats(medium, name):
    """Time checkpoints save and restore the state of a shot: a checkpoint without the memory variables would restart every
    segment but the first from r = 0 and move traces (recorded once, by the first pass) not at all but gradients by far
    more than rounding."""
    m = MEDIA[medium]
    c = M.case(m, name)
    order = 4
    nt = c["f"].shape[0]
    n = len(m.planes)
    g = M.ref(m, name, order, "matm")["g"]
    base = M.run(m, c, c["matm"], order, g)
    again = M.run(m, c, c["matm"], order, g)
    host = lambda t: np.asarray(t.cpu() if torch.is_tensor(t) else t)
    for a, b in zip(base, again):                                                  # a repeated call: the same bits
        assert np.array_equal(host(a), host(b))
    # time checkpoints: segments of 7 steps, at least three of them
    seg = M.run(m, c, c["matm"], order, g, snapshot_budget=14 * M.step_bytes(m, c) + 1)
    assert nt > 3 * 7
    assert torch.equal(seg[0], base[0]) and torch.equal(seg[1], base[1])
    errs = [rel_l2(seg[2][k], base[2][k]) for k in range(n)] + [rel_l2(seg[3], base[3])]
    print("time checkpoints vs resident snapshots: gradients rel-L2 %s" % ["%.1e" % e for e in errs])
    assert max(errs) <= TOL_SUM
    if m.segments_same_bits:
        for a, b in zip(base, seg):
            assert np.array_equal(host(a), host(b))
    # shots per gradient accumulator
    for gs in (1, 2):
        r = M.run(m, c, c["matm"], order, g, shots_per_group=gs)
        assert torch.equal(r[0], base[0]) and torch.equal(r[1], base[1])
        errs = [rel_l2(r[2][k], base[2][k]) for k in range(n)] + [rel_l2(r[3], base[3])]
        print("shots_per_group %d vs 0: gradients rel-L2 %s" % (gs, ["%.1e" % e for e in errs]))
        assert max(errs) <= TOL_SUM
    # Born in shot chunks of one
    whole = M.born(m, c, order, df=M.dev(c["df"]))
    chunked = M.born(m, c, order, df=M.dev(c["df"]), snapshot_budget=int(1.5 * nt * M.step_bytes(m, c, 1)))
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)

