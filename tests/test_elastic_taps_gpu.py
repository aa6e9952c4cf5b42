"""The elastic HIP kernels with bilinear four-tap sources and receivers (ntap = 4: per-step kernels only) against the fp32
oracle on the points of cases.elastic_case_taps4; tests/test_elastic_taps_oracle.py shows that the oracle is a sound
reference for them and that these points tell a wrong tap loop from a right one.

Bounds: test_elastic_gpu's TOL_TRACE = 1e-6 (seismograms) and TOL_GRAD = 2e-5 (the five material planes and grad_f), the
same operation chain on both sides.  Seismograms are bit-equal to the oracle as well: no cell holds two source taps of a
shot, and sampling is the oracle's fmaf chain in tap order.
"""
import numpy as np
import pytest
import torch

import test_elastic_born_gpu as EB
import test_elastic_gpu as EG
from cases import elastic_case_taps4, flatten_taps, rel_l2, sum_taps
from test_elastic_gpu import TOL_GRAD, TOL_TRACE

pytestmark = pytest.mark.gpu
FS = pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
PER_STEP = {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0"}
PLANES = ["lambda", "lambda+2mu", "mu_xz", "1/rho_x", "1/rho_z"]
_cache = {}


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _case(geometry, fs, **kw):
    key = ("case", geometry, fs) + tuple(sorted(kw.items()))
    if key not in _cache:
        _cache[key] = _frozen(elastic_case_taps4(geometry, seed=41, free_surface=fs, **kw))
    return _cache[key]


def _reference(o, case, tag, source_type=0, fd_order=4, pressure=False, f_scale=None):
    """The fp32 oracle's traces, white-noise adjoint sources of their size and the gradients for them: computed once per
    case and left unchanged."""
    key = ("ref", tag, source_type, fd_order, pressure, f_scale)
    if key not in _cache:
        f = case["f"] if f_scale is None else (case["f"] * f_scale).astype(np.float32)
        geo = (case["sc"], case["sw"], case["rc"], case["rw"])
        out = o.elastic_forward(case["mat"], case["pz"], case["px"], f, *geo, save=True, free_surface=case["fs"],
                                source_type=source_type, fd_order=fd_order, pressure=pressure)
        rec, S = [out[0], out[1]] + list(out[3:]), out[2]
        rng = np.random.default_rng(12)
        g = [(rng.standard_normal(r.shape) * np.abs(r).max()).astype(np.float32) for r in rec]
        gm, gf = o.elastic_backward(case["mat"], case["pz"], case["px"], *geo, g[0], g[1], S, free_surface=case["fs"],
                                    source_type=source_type, fd_order=fd_order, g_p=g[2] if pressure else None)
        ref = dict(f=f, rec=rec, S=S, g=g, gm=gm, gf=gf)
        for v in [f, S, gm, gf] + rec + g:
            v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def _propagate(case, f=None, source_type=0, fd_order=4, pressure=False, gs=0, need_grad=True, **kw):
    from physicsbasedfwi2_amd import elastic
    dev = torch.device("cuda:0")
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=need_grad)
    ft = torch.tensor(case["f"] if f is None else f, dtype=torch.float32, device=dev, requires_grad=need_grad)
    rec = elastic.propagate(mat, ft, torch.tensor(case["pz"]), torch.tensor(case["px"]), torch.tensor(case["sc"]),
                            torch.tensor(case["sw"]), torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"],
                            shots_per_group=gs, free_surface=bool(case["fs"]), source_type=source_type, fd_order=fd_order,
                            record_pressure=pressure, **kw)
    return mat, ft, list(rec)


def _backward(rec, g):
    torch.autograd.backward(rec, [torch.tensor(np.asarray(q), device=rec[0].device) for q in g])


def _np(t):
    return t.detach().cpu().numpy()


def _check(what, ref, rec, mat, f, bitwise=True):
    """Traces <= TOL_TRACE (and bit-equal), the five material planes and grad_f <= TOL_GRAD against the oracle."""
    et = [rel_l2(_np(a), b) for a, b in zip(rec, ref["rec"])]
    bits = [bool(np.array_equal(_np(a), b)) for a, b in zip(rec, ref["rec"])]
    eg = [rel_l2(_np(mat.grad[k]), ref["gm"][k]) for k in range(5)]
    ef = rel_l2(_np(f.grad), ref["gf"])
    print("%s: traces rel-L2 %s bit-equal %s; planes %s (max %.2e of %.0e); grad_f %.2e"
          % (what, ["%.2e" % e for e in et], bits, ["%.2e" % e for e in eg], max(eg), TOL_GRAD, ef))
    assert all(np.isfinite(_np(a)).all() and np.abs(b).max() > 0 for a, b in zip(rec, ref["rec"]))
    assert np.abs(ref["gf"]).max() > 0 and all(np.abs(ref["gm"][k]).max() > 0 for k in range(5))
    assert max(et) <= TOL_TRACE
    if bitwise:
        assert all(bits[:2])                      # vx, vz
    for k in range(5):
        assert eg[k] <= TOL_GRAD, PLANES[k]
    assert ef <= TOL_GRAD


def _parity(o, case, tag, what, bitwise=True, gs=0, **kw):
    ref = _reference(o, case, tag, **kw)
    kw = dict(kw)
    kw.pop("f_scale", None)
    mat, f, rec = _propagate(case, f=ref["f"], gs=gs, **kw)
    _backward(rec, ref["g"])
    _check(what, ref, rec, mat, f, bitwise)
    return ref, mat, f, rec


# ---- 1: the plan ----------------------------------------------------------------------------------------------------
def test_four_taps_take_the_per_step_kernels():
    """100x300 with 6 shots runs the single-launch loops with one tap; with four it must not (their receiver and source
    code is written for one), and a bf16 request - ignored by a single-launch plan - is then honoured.  2 or 3 taps are
    refused."""
    from physicsbasedfwi2_amd import _lib, elastic
    one = elastic.ElasticPlan(100, 300, 200, 6, 1, 200, 1, 10, 0, snapshot_format="bf16")
    four = elastic.ElasticPlan(100, 300, 200, 6, 1, 200, 4, 10, 0, snapshot_format="bf16")
    try:
        assert one.cluster_slabs(False) >= 1 and one.cluster_slabs(True) >= 1
        assert one.layout.snapshot_format == _lib.SNAPSHOT_F32
        assert four.cluster_slabs(False) == 0 and four.cluster_slabs(True) == 0
        fam = elastic.kernel_family(four.layout.kernel_flags)
        assert not any("single-launch" in name for name in fam), fam
        assert any("single-launch" in name for name in elastic.kernel_family(one.layout.kernel_flags))
        assert four.layout.snapshot_format == _lib.SNAPSHOT_BF16
    finally:
        one.close()
        four.close()
    c = _case("U", False)
    for ntap in (2, 3):
        cut = dict(c, **{k: np.ascontiguousarray(c[k][:, :, :ntap]) for k in ("sc", "sw", "rc", "rw")})
        with pytest.raises(elastic.MifwiError, match="ntap must be 1 or 4"):
            _propagate(cut, need_grad=False)


# ---- 2: parity on "T" through the formulations of the per-step family -----------------------------------------------
ENVS = {
    "default": ({}, {}),
    "fused": ({"MIFWI_EL_FUSED": "1"}, {}),
    "blocked": ({"MIFWI_EL_SNAP_BLOCKED": "1"}, {}),
    "row_major": ({"MIFWI_EL_SNAP_BLOCKED": "0"}, {}),
    "one_shot_passes": ({"MIFWI_EL_PASS_SHOTS": "1", "MIFWI_EL_PASS_GROUPS": "1"}, dict(ns=3)),
}


@FS
@pytest.mark.parametrize("env", list(ENVS))
def test_parity_on_tiles_with_many_taps_per_cell(oracle32, monkeypatch, env, fs):
    """Geometry "T": 280 receiver taps per shot (more than the 256 threads that sort them into tiles), four per interior
    cell, across the 15|16 row and 63|64 column boundaries of the adjoint tiles; a source with its taps in four tiles; a
    receiver with three inactive taps; under the free surface taps on rows 0 and 1 of both kinds."""
    for k, v in ENVS[env][0].items():
        monkeypatch.setenv(k, v)
    kw = ENVS[env][1]
    case = _case("T", fs, **kw)
    _parity(oracle32, case, ("T", fs, kw.get("ns", 2)), "T %s fs=%d" % (env, fs), gs=1 if env == "one_shot_passes" else 0)


# ---- 3: other tile shapes -------------------------------------------------------------------------------------------
SHAPES = {
    "one_tile_column_ragged": dict(nz=40, nx=53, rx0=10.25, src0=(15.4, 30.3), min_tiles=2),
    "column_255_256": dict(nz=34, nx=300, fw=10, rx0=238.25, src0=(15.4, 255.5)),
}


@FS
@pytest.mark.parametrize("env", ["default", "fused"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_on_other_tile_shapes(oracle32, monkeypatch, shape, env, fs):
    """40x53: a single, ragged adjoint tile column.  34x300: the receiver line across column 255|256 and a source at
    x = 255.5, the boundary of the forward injection tile at 64 groups per row."""
    for k, v in ENVS[env][0].items():
        monkeypatch.setenv(k, v)
    case = _case("T", fs, **SHAPES[shape])
    _parity(oracle32, case, ("T", fs, shape), "T %s %s fs=%d" % (shape, env, fs))


# ---- 4: point forces ------------------------------------------------------------------------------------------------
@FS
@pytest.mark.parametrize("source_type", [1, 2], ids=["fx", "fz"])
def test_point_forces(oracle32, source_type, fs):
    """el_inject_force / el_sample_force: one thread adds a shot's taps in the oracle's order."""
    _parity(oracle32, _case("T", fs), ("T", fs, 2), "T force %d fs=%d" % (source_type, fs), source_type=source_type,
            f_scale=1e-3)


# ---- 5: pressure receivers ------------------------------------------------------------------------------------------
@FS
def test_pressure_receivers(oracle32, monkeypatch, fs):
    """el_sample_pressure / el_inject_pressure with one shot per pass of three (s0 > 0): rec_p and all gradients of an
    objective on (vx, vz, p); the velocity seismograms are those of a plain plan bit for bit."""
    monkeypatch.setenv("MIFWI_EL_PASS_SHOTS", "1")
    case = _case("T", fs, ns=3)
    _, _, _, rec = _parity(oracle32, case, ("T", fs, 3), "T pressure fs=%d" % fs, pressure=True)
    _, _, plain = _propagate(case, need_grad=False)
    assert torch.equal(rec[0].detach(), plain[0]) and torch.equal(rec[1].detach(), plain[1])


# ---- 6: second-order stencils ---------------------------------------------------------------------------------------
def test_second_order_stencils(oracle32):
    _parity(oracle32, _case("T", True), ("T", True, 2), "T fd_order=2 fs=1", fd_order=2)


# ---- 7: bf16 snapshot planes ----------------------------------------------------------------------------------------
@FS
def test_bf16_snapshot_planes(oracle32, monkeypatch, fs):
    """The assertions of test_elastic_gpu.test_bf16_snapshot_planes with four taps: unchanged seismograms, the oracle's
    gradient from bf16-rounded planes within TOL_GRAD, within 4e-3 of the exact gradient (and not equal to it), grad_f
    untouched, 17-step checkpoint segments bit-equal to the resident run where the adjoint's bits are defined ("U")."""
    from physicsbasedfwi2_amd import _lib, elastic
    for k, v in PER_STEP.items():
        monkeypatch.setenv(k, v)
    case = _case("T", fs)
    ref = _reference(oracle32, case, ("T", fs, 2))
    nt, ns, nsrc = case["f"].shape
    nz, nx = case["mat"].shape[1:]
    lay = {}
    for fmt in ("f32", "bf16"):
        pl = elastic.ElasticPlan(nz, nx, nt, ns, nsrc, case["rc"].shape[1], 4, case["fw"], 0, 0, case["fs"],
                                 snapshot_format=fmt)
        lay[fmt] = (pl.layout.snapshot_format, pl.layout.snap_step_elems)
        pl.close()
    assert lay["f32"][0] == _lib.SNAPSHOT_F32 and lay["bf16"][0] == _lib.SNAPSHOT_BF16
    assert lay["bf16"][1] <= 0.5 * lay["f32"][1] + 4 * ns

    def run(fmt, **kw):
        mat, f, rec = _propagate(case, snapshot_format=fmt, **kw)
        _backward(rec, ref["g"])
        return rec[0].detach(), rec[1].detach(), mat.grad.clone(), f.grad.clone()
    ex, bf = run("f32"), run("bf16")
    assert torch.equal(ex[0], bf[0]) and torch.equal(ex[1], bf[1])
    assert np.array_equal(_np(bf[0]), ref["rec"][0]) and np.array_equal(_np(bf[1]), ref["rec"][1])
    gm_round, _ = oracle32.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"], case["rc"],
                                            case["rw"], ref["g"][0], ref["g"][1], EG._bf16_round(ref["S"]),
                                            free_surface=case["fs"])
    gh = _np(bf[2])
    er = [rel_l2(gh[k], gm_round[k]) for k in range(5)]
    ee = [rel_l2(gh[k], ref["gm"][k]) for k in range(5)]
    ef = rel_l2(_np(bf[3]), ref["gf"])
    print("T bf16 fs=%d: vs rounded-plane oracle %s; vs exact %s; grad_f %.2e"
          % (fs, ["%.2e" % e for e in er], ["%.2e" % e for e in ee], ef))
    for k in range(5):
        assert er[k] <= TOL_GRAD, PLANES[k]
        assert 1e-6 < ee[k] <= 4e-3, (PLANES[k], ee[k])
    assert ef <= TOL_GRAD
    # 17-step checkpoint segments: the same seismograms; the gradient bits are defined only while no cell gets more than
    # two receiver taps of a shot (see propagate), so on "T" the segmented gradient is held to the bounds above and the
    # bit comparison of test_bf16_snapshot_planes is made on "U"
    seg = run("bf16", snapshot_budget=4 * lay["bf16"][1] * 2 * 17)
    assert torch.equal(bf[0], seg[0]) and torch.equal(bf[1], seg[1])
    es = [rel_l2(_np(seg[2])[k], gm_round[k]) for k in range(5)]
    print("T bf16 fs=%d in 17-step segments: vs rounded-plane oracle %s" % (fs, ["%.2e" % e for e in es]))
    assert max(es) <= TOL_GRAD and rel_l2(_np(seg[3]), ref["gf"]) <= TOL_GRAD
    case = _case("U", fs)
    g = None
    outs = []
    for kw in ({}, {"snapshot_budget": 4 * lay["bf16"][1] * 2 * 17}):
        mat, f, rec = _propagate(case, snapshot_format="bf16", **kw)
        g = g or [torch.sign(r.detach()) + 0.5 for r in rec]
        torch.autograd.backward(rec, g)
        outs.append((rec[0].detach(), rec[1].detach(), mat.grad.clone(), f.grad.clone()))
    assert all(float(t.abs().max()) > 0 for t in outs[0])
    for a, b, what in zip(outs[0], outs[1], ("vx", "vz", "mat.grad", "f.grad")):
        assert torch.equal(a, b), what


# ---- 8: bit comparisons where no cell gets more than two receiver taps of a shot ------------------------------------
@FS
def test_repeatable_and_checkpointed_bits_with_two_taps_per_cell(fs):
    """Geometry "U": two float adds into a cell commute, so two identical calls give the same bits for traces, mat.grad
    and f.grad, and so does a run in 11-step checkpoint segments (the tile lists are rebuilt by every backward call,
    once per segment)."""
    case = _case("U", fs)
    outs = []
    nz, nx = case["mat"].shape[1:]
    step_bytes = 4 * 5 * 2 * nz * ((nx + 3) // 4 * 4)
    g = None
    for kw in ({}, {}, {"snapshot_budget": step_bytes * 2 * 11}):
        mat, f, rec = _propagate(case, **kw)
        g = g or [torch.sign(r.detach()) + 0.5 for r in rec]
        torch.autograd.backward(rec, g)
        outs.append((rec[0].detach().clone(), rec[1].detach().clone(), mat.grad.clone(), f.grad.clone()))
    assert all(float(t.abs().max()) > 0 for t in outs[0])
    for other, name in ((outs[1], "second call"), (outs[2], "checkpointed")):
        for a, b, what in zip(outs[0], other, ("vx", "vz", "mat.grad", "f.grad")):
            assert torch.equal(a, b), (name, what)


def test_gradient_in_shot_chunks_of_one():
    """elastic.gradient_in_shot_chunks with chunk 1 on "U" with three shots against the all-shots call: 2e-6, the bound
    of test_gradient_in_shot_chunks_equals_the_all_shots_gradient."""
    from physicsbasedfwi2_amd import elastic, misfit
    case = _case("U", False, ns=3)
    dev = "cuda:0"
    nt, ns, _ = case["f"].shape
    nrec = case["rc"].shape[1]
    gen = torch.Generator().manual_seed(3)
    obs = [(torch.randn(nt, ns, nrec, generator=gen) * 1e-3).to(dev) for _ in range(2)]
    t = lambda n: torch.tensor(case[n])

    def loss_fn(rvx, rvz, sl):
        return misfit.l2_half(rvx, obs[0][:, sl].contiguous()) + misfit.l2_half(rvz, obs[1][:, sl].contiguous())

    def run(chunk):
        mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
        f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
        args = (t("pz"), t("px"), t("sc"), t("sw"), t("rc"), t("rw"), case["fw"])
        if chunk:
            loss = elastic.gradient_in_shot_chunks(mat, f, *args, loss_fn, chunk)
        else:
            rvx, rvz = elastic.propagate(mat, f, *args)
            loss = loss_fn(rvx, rvz, slice(0, ns))
            loss.backward()
            loss = loss.detach()
        return float(loss), _np(mat.grad), _np(f.grad)
    l0, gm0, gf0 = run(0)
    l1, gm1, gf1 = run(1)
    em, ef = rel_l2(gm1, gm0), rel_l2(gf1, gf0)
    print("U shot chunks of one: loss %.9e vs %.9e, mat.grad %.2e, f.grad %.2e" % (l1, l0, em, ef))
    assert l0 > 0 and np.abs(gm0).max() > 0 and np.abs(gf0).max() > 0
    assert abs(l1 - l0) <= 1e-6 * l0
    assert em <= 2e-6 and ef <= 2e-6


# ---- 9: Born modelling and Gauss-Newton products --------------------------------------------------------------------
def _born_case(fs):
    """"T" with its real inputs rounded to f32 (what the device computes with) and seeded 1 % perturbations."""
    key = ("born", fs)
    if key not in _cache:
        c = dict(_case("T", fs))
        for k in ("mat", "pz", "px", "f", "sw", "rw"):
            c[k] = EB._f32(c[k])
        rng = np.random.default_rng(100)
        c["dmat"] = EB._f32(0.01 * rng.standard_normal(c["mat"].shape) * c["mat"])
        if fs:
            c["dmat"][0, 0] = 0.0
        c["df"] = EB._f32(0.01 * rng.standard_normal(c["f"].shape) * np.abs(c["f"]).max())
        _cache[key] = _frozen(c)
    return _cache[key]


@FS
def test_born_is_the_directional_derivative_of_the_oracle(oracle64, fs):
    """elastic.born against the central difference of the fp64 oracle's forward (eps = 1e-5, inputs rounded to f32
    first), as test_elastic_born_gpu builds it: 2e-6 rel-L2 over vx and vz together."""
    c = _born_case(fs)
    run = lambda m: oracle64.elastic_forward(m, c["pz"], c["px"], c["f"], c["sc"], c["sw"], c["rc"], c["rw"],
                                             free_surface=c["fs"])
    p, m = run(c["mat"] + EB.EPS * c["dmat"]), run(c["mat"] - EB.EPS * c["dmat"])
    want = np.stack([(p[0] - m[0]) / (2 * EB.EPS), (p[1] - m[1]) / (2 * EB.EPS)])
    _, _, dvx, dvz = EB._born(c)
    got = EB._pair(dvx, dvz)
    err = rel_l2(got, want)
    print("T born vs fp64 central difference fs=%d: rel-L2 %.3e" % (fs, err))
    assert np.abs(got).max() > 0
    assert err <= 2e-6


@FS
def test_born_and_gauss_newton_transpose_identities(fs):
    """<J dm, g> = <dm, J^T g>, <J df, g> = <df, J^T g> and <dm, H dm> = |J dm|^2 with H = J^T J from
    gauss_newton_product: 2e-5, the project's bound for gradients summed in another order."""
    from physicsbasedfwi2_amd import elastic
    c = _born_case(fs)
    a = EB._args(c)
    dm, df = EB._dev(c, "dmat", "df")
    _, _, dvx, dvz = EB._born(c)
    g = EB._adjoint_source(dvx, dvz)
    mat, _ = EB._gradient(c, lambda *_: g)
    EB._close(EB._dot(dvx, g[0]) + EB._dot(dvz, g[1]), EB._dot(dm, mat.grad), 2e-5, "T fs=%d <J dm, g> vs <dm, J^T g>" % fs)
    _, _, svx, svz = EB._born(c, dmat=torch.zeros_like(dm), df=df)
    assert svx.abs().max() > 0
    g = EB._adjoint_source(svx, svz)
    _, f = EB._gradient(c, lambda *_: g, need_f=True)
    EB._close(EB._dot(svx, g[0]) + EB._dot(svz, g[1]), EB._dot(df, f.grad), 2e-5, "T fs=%d <J df, g> vs <df, J^T g>" % fs)
    hv, gx, gz = elastic.gauss_newton_product(a[0], dm, *a[1:], free_surface=fs)
    assert torch.equal(gx, dvx) and torch.equal(gz, dvz)
    EB._close(EB._dot(dm, hv), EB._dot(dvx, dvx) + EB._dot(dvz, dvz), 2e-5, "T fs=%d <d, H d> vs |J d|^2" % fs)


# ---- 10: the same points as one-tap points, on the device -----------------------------------------------------------
@FS
def test_four_taps_equal_the_same_points_as_one_tap_points(oracle32, monkeypatch, fs):
    """Independent of every `ntap` loop and index on the device: 8 one-tap sources and 280 one-tap receivers per shot
    through the same per-step kernels.  Traces summed over a point's taps within TOL_TRACE, material planes and the
    tap-summed grad_f within TOL_GRAD."""
    for k, v in PER_STEP.items():
        monkeypatch.setenv(k, v)
    case = _case("T", fs)
    ref = _reference(oracle32, case, ("T", fs, 2))
    mat, f, rec = _propagate(case)
    _backward(rec, ref["g"])
    flat = flatten_taps(case)
    fmat, ff, frec = _propagate(flat)
    _backward(frec, [np.repeat(q, 4, axis=2) for q in ref["g"]])
    et = [rel_l2(sum_taps(_np(a)), _np(b)) for a, b in zip(frec, rec)]
    eg = [rel_l2(_np(fmat.grad[k]), _np(mat.grad[k])) for k in range(5)]
    ef = rel_l2(sum_taps(_np(ff.grad)), _np(f.grad))
    print("T flattened vs four taps on the device fs=%d: traces %s; planes %s; grad_f %.2e"
          % (fs, ["%.2e" % e for e in et], ["%.2e" % e for e in eg], ef))
    assert float(rec[0].abs().max()) > 0 and float(f.grad.abs().max()) > 0
    assert max(et) <= TOL_TRACE
    assert max(eg) <= TOL_GRAD and ef <= TOL_GRAD


# ---- 11: repeatability where cells get three or more taps -----------------------------------------------------------
def test_gradients_with_four_taps_per_cell_stay_within_the_bound(oracle32):
    """el_adj_s adds the receiver taps of a cell with LDS float atomics in hardware order, so with three or more taps
    per cell ("T": four) the adjoint is not bit-repeatable by contract - every run is within TOL_GRAD of the oracle.
    Two runs, both asserted; whether they were bit-equal is printed, not asserted."""
    case = _case("T", False)
    ref = _reference(oracle32, case, ("T", False, 2))
    grads = []
    for i in range(2):
        mat, f, rec = _propagate(case)
        _backward(rec, ref["g"])
        _check("T run %d" % i, ref, rec, mat, f)
        grads.append((mat.grad.clone(), f.grad.clone()))
    print("T two runs: mat.grad bit-equal %s, f.grad bit-equal %s"
          % (torch.equal(grads[0][0], grads[1][0]), torch.equal(grads[0][1], grads[1][1])))
