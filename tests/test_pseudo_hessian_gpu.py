"""Elastic pseudo-Hessian: the snapshot second moments (mifwi_elastic_snapshot_moments), the map to a Hessian per
parametrisation (mifwi_elastic_pseudo_hessian), the preconditioning kernel (mifwi_gradient_precondition) and the
EPRECOND / EPSILON_WE parameters of the pyapi_denise shim.

Reference for the moments: the oracle's snapshot planes S [nt, ns, 5, nz, nx] reduced in numpy float64.  Bound 2e-5 rel-L2
per plane: the project's bound for time-and-shot sums taken in another order (<= 360 f32 terms here).
Shapes: A = the default 44 x 60 case (15 groups: less than one column block of 16), B = 37 x 150 (38 groups: three column
blocks, the last partial; nx no multiple of 4, gp = 152)."""
import ctypes

import numpy as np
import pytest
import torch

from cases import elastic_case, rel_l2

pytestmark = pytest.mark.gpu
TOL = 2e-5
SHAPES = {"A": dict(), "B": dict(nz=37, nx=150, ns=3, nt=50)}
# plan forms: environment, snapshot_format
FORMS = {
    "default": ({}, None),
    "per_step_blocked": ({"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0"}, None),
    "per_step_row_major": ({"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_SNAP_BLOCKED": "0"}, None),
    "per_step_blocked_bf16": ({"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0"}, "bf16"),
    "per_step_row_major_bf16": ({"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_SNAP_BLOCKED": "0"}, "bf16"),
}
_cache = {}


def _case(shape, fs=False, **kw):
    return elastic_case(seed=71, free_surface=fs, **dict(SHAPES[shape], **kw))


def _oracle_S(o, shape, fs=False, **kw):
    """The oracle's snapshot planes of a case, float64, computed once per case and left unchanged."""
    key = (shape, fs, tuple(sorted(kw.items())))
    if key not in _cache:
        c = _case(shape, fs, **kw)
        _, _, S = o.elastic_forward(c["mat"], c["pz"], c["px"], c["f"], c["sc"], c["sw"], c["rc"], c["rw"], save=True,
                                    free_surface=c["fs"])
        S = np.asarray(S, dtype=np.float64)
        S.setflags(write=False)
        _cache[key] = S
    return _cache[key]


def _reduce(S, stride=1):
    """[6, nz, nx] float64: stride * sum over the steps n % stride == 0 and the shots."""
    S = S[0::stride]
    m = [(S[:, :, k] ** 2).sum(axis=(0, 1)) for k in range(5)] + [(S[:, :, 0] * S[:, :, 1]).sum(axis=(0, 1))]
    return stride * np.stack(m)


def _run(case, holder, fmt=None, budget=None):
    """One forward + backward through elastic.propagate with the holder; returns the material gradient."""
    from physicsbasedfwi2_amd import elastic
    dev = torch.device("cuda:0")
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=dev)
    kw = {} if budget is None else {"snapshot_budget": budget}
    rvx, rvz = elastic.propagate(mat, f, torch.tensor(case["pz"]), torch.tensor(case["px"]), torch.tensor(case["sc"]),
                                 torch.tensor(case["sw"]), torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"],
                                 free_surface=bool(case["fs"]), snapshot_format=fmt, pseudo_hessian=holder, **kw)
    torch.autograd.backward([rvx, rvz], [torch.sign(rvx.detach()), torch.sign(rvz.detach())])
    return mat.grad


def _layout(case, fmt=None):
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    _, nz, nx = case["mat"].shape
    nt, ns, nsrc = case["f"].shape
    pl = ElasticPlan(nz, nx, nt, ns, nsrc, case["rc"].shape[1], 1, case["fw"], 0, free_surface=case["fs"], snapshot_format=fmt)
    lay = (pl.layout.kernel_flags, pl.layout.snapshot_format, pl.layout.snap_step_elems, pl.layout.gp)
    pl.close()
    return lay


def _assert_planes(got, want, tol=TOL):
    errs = [rel_l2(got[k], want[k]) for k in range(len(want))]
    print("rel-L2 per plane:", " ".join("%.2e" % e for e in errs))
    assert np.abs(want).max() > 0
    for k, e in enumerate(errs):
        assert e <= tol, (k, e)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_moments_against_the_oracle_in_every_snapshot_layout(oracle32, monkeypatch, shape, fs, form):
    from physicsbasedfwi2_amd import _lib, elastic
    env, fmt = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = _case(shape, fs)
    flags, sfmt, step_elems, gp = _layout(case, fmt)
    single = _lib.EL_KERNEL_FWD_SINGLE_LAUNCH | _lib.EL_KERNEL_ADJ_SINGLE_LAUNCH
    _, nz, nx = case["mat"].shape
    ns = case["f"].shape[1]
    if form == "default":                         # these grids fit the LDS of a few CUs: row-major f32 planes
        assert (flags & single) != 0 and sfmt == _lib.SNAPSHOT_F32 and step_elems == ns * 5 * nz * gp
    else:
        assert flags & single == 0
        assert sfmt == (_lib.SNAPSHOT_BF16 if fmt else _lib.SNAPSHOT_F32)
        blocked = "MIFWI_EL_SNAP_BLOCKED" not in env
        plane = nz * 64 * ((gp // 4 + 15) // 16) if blocked else nz * gp
        assert step_elems == ns * ((5 * plane // 2 + 3) // 4 * 4 if fmt else 5 * plane)
    holder = elastic.PseudoHessian()
    _run(case, holder, fmt)
    S = _oracle_S(oracle32, shape, fs)
    if fmt:                                       # what the planes hold after their trip through memory
        S = torch.tensor(S, dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    assert tuple(holder.moments.shape) == (6, nz, nx) and holder.moments.is_cuda
    _assert_planes(holder.moments.cpu().numpy(), _reduce(S))


def test_stride_and_checkpoint_segments(oracle32):
    """stride = 3 selects the steps n % 3 == 0 in ABSOLUTE n and weights them by 3; a checkpointed backward (segments of 11
    steps, no multiple of 3) hands the kernel one regenerated segment at a time and selects the same steps."""
    from physicsbasedfwi2_amd import elastic
    case = _case("B")
    h1 = elastic.PseudoHessian(stride=3)
    g1 = _run(case, h1)
    _assert_planes(h1.moments.cpu().numpy(), _reduce(_oracle_S(oracle32, "B"), 3))
    _, nz, nx = case["mat"].shape
    step_bytes = 4 * 5 * case["f"].shape[1] * nz * ((nx + 3) // 4 * 4)
    h2 = elastic.PseudoHessian(stride=3)
    g2 = _run(case, h2, budget=step_bytes * 2 * 11)
    assert torch.equal(g1, g2)                    # the gradient itself is what it was
    _assert_planes(h2.moments.cpu().numpy(), h1.moments.cpu().numpy().astype(np.float64))
    with pytest.raises(elastic.MifwiError):
        elastic.PseudoHessian(stride=0)


def test_c_abi_ranges_overwrite_padding_and_bad_arguments(monkeypatch):
    """The entry point itself on a row-major f32 buffer of random planes whose pad columns hold NaN."""
    from physicsbasedfwi2_amd import _lib
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    monkeypatch.setenv("MIFWI_EL_CLUSTER", "0")
    monkeypatch.setenv("MIFWI_EL_CLUSTER_ADJ", "0")
    monkeypatch.setenv("MIFWI_EL_SNAP_BLOCKED", "0")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nz, nx, ns, nt = 37, 150, 3, 50
    pl = ElasticPlan(nz, nx, nt, ns, 1, 4, 1, 8, 0)
    gp = pl.layout.gp
    assert gp == 152 and pl.layout.snap_step_elems == ns * 5 * nz * gp
    g = torch.Generator().manual_seed(5)
    snap = torch.randn((nt, ns, 5, nz, gp), generator=g, dtype=torch.float32)
    want = _reduce(snap[..., :nx].double().numpy())
    snap[..., nx:] = float("nan")
    snap = snap.to(dev)
    work = torch.empty(lib.mifwi_elastic_snapshot_moments_work_elems(pl.handle), device=dev)
    assert work.numel() >= 6 * nz * gp

    def call(out, b, e, stride=1, flags=0, first=0):
        return lib.mifwi_elastic_snapshot_moments(pl.handle, _lib.ptr(snap[first:]), first, b, e, stride, _lib.ptr(out),
                                                  _lib.ptr(work), flags, None)
    whole = torch.full((6, nz, gp), float("nan"), device=dev)
    assert call(whole, 0, nt, flags=_lib.ZERO_STATE) == 0
    assert torch.isfinite(whole).all()                              # ZERO_STATE overwrites
    assert float(whole[:, :, nx:].abs().max()) == 0.0               # whatever the pad of the snapshot buffer holds
    _assert_planes(whole[:, :, :nx].cpu().numpy(), want)
    parts = torch.full((6, nz, gp), float("nan"), device=dev)
    assert call(parts, 0, 20, flags=_lib.ZERO_STATE) == 0 and call(parts, 20, nt, first=20) == 0
    assert float(parts[:, :, nx:].abs().max()) == 0.0
    _assert_planes(parts[:, :, :nx].cpu().numpy(), whole[:, :, :nx].cpu().numpy().astype(np.float64))
    # bad arguments: MIFWI_EINVAL, nothing launched (the output keeps its bits)
    before = parts.clone()
    for args in (dict(b=0, e=nt, stride=0), dict(b=10, e=10), dict(b=30, e=20)):
        assert call(parts, flags=_lib.ZERO_STATE, **args) == -1
    grad = torch.ones((2, 8), device=dev)
    pwork = torch.empty(lib.mifwi_gradient_precondition_work_elems(2), device=dev)

    def pre(nplane, eps):
        e = (ctypes.c_float * len(eps))(*eps)
        return lib.mifwi_gradient_precondition(0, _lib.ptr(grad), _lib.ptr(grad), _lib.ptr(grad), nplane, 8,
                                               ctypes.cast(e, ctypes.c_void_p), _lib.ptr(pwork), None)
    assert pre(2, [0.1, 0.0]) == -1 and pre(0, [0.1]) == -1 and pre(5, [0.1] * 5) == -1
    torch.cuda.synchronize()
    assert torch.equal(parts, before) and float(grad.min()) == 1.0 and float(grad.max()) == 1.0
    pl.close()


def test_shot_chunks_sum_into_the_holder_and_reset(oracle32):
    from physicsbasedfwi2_amd import elastic
    case = _case("A", ns=5)
    whole = elastic.PseudoHessian()
    _run(case, whole)
    dev = torch.device("cuda:0")
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
    chunks = elastic.PseudoHessian()
    elastic.gradient_in_shot_chunks(
        mat, torch.tensor(case["f"], dtype=torch.float32, device=dev), torch.tensor(case["pz"]), torch.tensor(case["px"]),
        torch.tensor(case["sc"]), torch.tensor(case["sw"]), torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"],
        lambda vx, vz, sl: 0.5 * (vx ** 2).sum() + 0.5 * (vz ** 2).sum(), 2, pseudo_hessian=chunks)
    _assert_planes(chunks.moments.cpu().numpy(), whole.moments.cpu().numpy().astype(np.float64))
    _assert_planes(whole.moments.cpu().numpy(), _reduce(_oracle_S(oracle32, "A", ns=5)))
    chunks.reset()
    assert tuple(chunks.moments.shape) == tuple(whole.moments.shape) and float(chunks.moments.abs().max()) == 0.0


def test_forward_only_run_with_a_holder_raises():
    from physicsbasedfwi2_amd import elastic
    case = _case("A")
    dev = torch.device("cuda:0")
    with pytest.raises(elastic.MifwiError):
        elastic.propagate(torch.tensor(case["mat"], dtype=torch.float32, device=dev),
                          torch.tensor(case["f"], dtype=torch.float32, device=dev), torch.tensor(case["pz"]),
                          torch.tensor(case["px"]), torch.tensor(case["sc"]), torch.tensor(case["sw"]),
                          torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"],
                          pseudo_hessian=elastic.PseudoHessian())


@pytest.mark.parametrize("form", ["default", "per_step_blocked"])
def test_two_identical_runs_give_the_same_bits(monkeypatch, form):
    from physicsbasedfwi2_amd import elastic
    for k, v in FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    case = _case("B")
    out = []
    for _ in range(2):
        h = elastic.PseudoHessian()
        _run(case, h)
        out.append(h.moments)
    assert float(out[0].abs().max()) > 0 and torch.equal(out[0], out[1])


def _partials(mode, vp, vs, rho, s):
    """(L_p, M_p, mu_p, b_p) of the three parameters of a parametrisation: the table of include/mifwi.h in float64."""
    z = torch.zeros_like(vp)
    b = torch.where(rho == 0, z, -s / torch.where(rho == 0, torch.ones_like(rho), rho) ** 2)
    if mode == 1:
        return [(2 * rho * vp * s, 2 * rho * vp * s, z, z), (-4 * rho * vs * s, z, 2 * rho * vs * s, z),
                ((vp ** 2 - 2 * vs ** 2) * s, vp ** 2 * s, vs ** 2 * s, b)]
    if mode == 2:
        return [(2 * vp * s, 2 * vp * s, z, z), (-4 * vs * s, z, 2 * vs * s, z),
                (-(vp ** 2 - 2 * vs ** 2) * s, -vp ** 2 * s, -vs ** 2 * s, b)]
    return [(s + z, s + z, z, z), (z, 2 * s + z, s + z, z), (z, z, z, b)]


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_hessian_map_against_the_table(mode):
    from physicsbasedfwi2_amd import elastic
    g = torch.Generator().manual_seed(9)
    nz, nx = 9, 13
    vp = 1500 + 2000 * torch.rand((nz, nx), generator=g, dtype=torch.float64)
    vs = vp / 1.8
    rho = 1000 + 1500 * torch.rand((nz, nx), generator=g, dtype=torch.float64)
    vs[:3] = 0.0                                                   # water rows
    rho[5, 7] = 0.0                                                # a cell whose b partial has a zero divisor
    vp, vs, rho = (t.float().double() for t in (vp, vs, rho))
    M = torch.rand((6, nz, nx), generator=g, dtype=torch.float64) * 1e3
    M[5] = (2 * torch.rand((nz, nx), generator=g, dtype=torch.float64) - 1) * torch.sqrt(M[0] * M[1])
    M[5, 0] = -torch.sqrt(M[0, 0] * M[1, 0])                        # the bound itself: full cancellation for Vp
    M = M.float()
    M[5] = torch.minimum(M[5].abs(), torch.sqrt(M[0] * M[1]) * (1 - 1e-6)) * torch.sign(M[5])
    dt, h = 0.002, 20.0
    holder = elastic.PseudoHessian()
    holder.moments = M.to("cuda:0")
    H = holder.hessian(vp, vs, rho, dt, h, parametrization=mode)
    assert tuple(H.shape) == (3, nz, nx) and torch.isfinite(H).all() and float(H.min()) >= 0.0
    Md = M.double()
    want = [(L * L + Mp * Mp) * (Md[0] + Md[1]) + 4 * L * Mp * Md[5] + mu * mu * Md[2] + b * b * (Md[3] + Md[4])
            for L, Mp, mu, b in _partials(mode, vp, vs, rho, dt / h)]
    _assert_planes(H.cpu().numpy(), torch.stack(want).numpy(), tol=1e-5)
    with pytest.raises(elastic.MifwiError):
        holder.hessian(vp, vs, rho, dt, h, parametrization=4)


def test_hessian_of_vp_against_the_virtual_sources_and_its_peak_at_the_source(oracle32):
    """H_vp of the VELOCITY set = sum over steps and shots of | d(virtual source) / dVp |^2, formed from the oracle's planes
    directly (no moments): (S1 L_p + S0 M_p)^2 + (S0 L_p + S1 M_p)^2 with L_p = M_p = 2 rho Vp s."""
    from physicsbasedfwi2_amd import elastic
    case = _case("A")
    holder = elastic.PseudoHessian()
    _run(case, holder)
    H = holder.hessian(torch.tensor(case["vp"]), torch.tensor(case["vs"]), torch.tensor(case["rho"]), case["dt"], case["h"])
    S = _oracle_S(oracle32, "A")
    vp32, rho32 = case["vp"].astype(np.float32).astype(np.float64), case["rho"].astype(np.float32).astype(np.float64)
    Lp = 2 * rho32 * vp32 * (case["dt"] / case["h"])
    want = ((S[:, :, 1] * Lp + S[:, :, 0] * Lp) ** 2 + (S[:, :, 0] * Lp + S[:, :, 1] * Lp) ** 2).sum(axis=(0, 1))
    _assert_planes(H[:1].cpu().numpy(), want[None])
    # one shot: the raw energy peaks at the source (what the preconditioner is there to flatten)
    one = _case("A", ns=1)
    h1 = elastic.PseudoHessian()
    _run(one, h1)
    Hv = h1.hessian(torch.tensor(one["vp"]), torch.tensor(one["vs"]), torch.tensor(one["rho"]), one["dt"], one["h"])[0]
    nx = Hv.shape[1]
    k = int(Hv.argmax())
    sz, sx = divmod(int(one["sc"].reshape(-1)[0]), nx)
    print("source (%d, %d), maximum of H_vp at (%d, %d)" % (sz, sx, k // nx, k % nx))
    assert abs(k // nx - sz) <= 1 and abs(k % nx - sx) <= 1


def test_precondition_kernel_against_numpy():
    """Three roundings in f32 (h / max, + eps, g / .), all operands of the sum positive: 1e-6 relative per element."""
    from physicsbasedfwi2_amd import _lib, conditioning
    rng = np.random.default_rng(21)
    nz, nx = 37, 53
    g = rng.standard_normal((3, nz, nx)).astype(np.float32)
    h = (rng.random((3, nz, nx)) ** 4 * 7e5).astype(np.float32)
    h[1] = 0.0                                                     # Vs in a fluid: the plane passes through
    eps = [0.005, 0.01, 0.2]
    want = g.astype(np.float64).copy()
    for k in (0, 2):
        want[k] = g[k] / (h[k].astype(np.float64) / float(h[k].max()) + float(np.float32(eps[k])))
    gd, hd = torch.tensor(g, device="cuda:0"), torch.tensor(h, device="cuda:0")
    out = conditioning.precondition_gradients(gd, hd, eps)
    assert torch.equal(out[1], gd[1])
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-6, atol=0)
    one = conditioning.precondition_gradients(gd, hd, 0.005)       # one water level for all planes
    np.testing.assert_allclose(one[2].cpu().numpy(), g[2] / (h[2].astype(np.float64) / float(h[2].max()) + float(np.float32(0.005))),
                               rtol=1e-6, atol=0)
    with pytest.raises(_lib.MifwiError):
        conditioning.precondition_gradients(gd, hd, 0.0)
    # out aliasing grad
    lib = _lib.load()
    work = torch.empty(lib.mifwi_gradient_precondition_work_elems(3), device="cuda:0")
    e = (ctypes.c_float * 3)(*eps)
    inplace = gd.clone()
    assert lib.mifwi_gradient_precondition(0, _lib.ptr(inplace), _lib.ptr(hd), _lib.ptr(inplace), 3, nz * nx,
                                           ctypes.cast(e, ctypes.c_void_p), _lib.ptr(work), None) == 0
    assert torch.equal(inplace, out)


def _denise(tmp_path):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 60, 90, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3)).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    vs[:8] = 0; vp[:8] = 1500; rho[:8] = 1000

    def make():
        d = api.Denise(None, 0)
        d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.5, 0.002, 0, 10, 5.0, 1500.0
        return d
    xsrc = np.array([400.0, 1000.0, 1400.0])
    src = api.Sources(xsrc, 40.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1500.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    return api, make, (vp, vs, rho), dx, src, rec


def test_shim_eprecond_and_epsilon_we(tmp_path, monkeypatch):
    """EPRECOND = 1 in d.grad = the EPRECOND = 0 gradients put through PseudoHessian.hessian (same INVMAT1) and
    precondition_gradients with EPSILON_WE; both the arrays of get_fwi_gradients and the planes left on the device."""
    from physicsbasedfwi2_amd import conditioning
    api, make, (vp, vs, rho), dx, src, rec = _denise(tmp_path)
    monkeypatch.chdir(tmp_path)
    d = make()
    assert d.EPRECOND == 0 and d.EPSILON_WE == 0.005               # DENISE.inp's values
    ox, oy = d.forward(api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx), src, rec)
    obs = (np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)

    def run(mode, precond, eps=None):
        dd = make()
        dd.INVMAT1, dd.EPRECOND = mode, precond
        if eps is not None:
            dd.EPSILON_WE = eps
        dd.set_observed(*obs)
        dd.add_fwi_stage(fc_high=10)
        dd.grad(model, src, rec)
        return dd

    for mode, eps in ((1, None), (3, 0.01)):
        raw, pre = run(mode, 0), run(mode, 1, eps)
        assert raw._pseudo_hessian is None and pre.loss == raw.loss
        hess = pre._pseudo_hessian.hessian(vp, vs, rho, pre.DT_used, dx, mode)
        want = conditioning.precondition_gradients(raw._gradients_dev, hess, pre.EPSILON_WE).cpu().numpy()
        assert pre.EPSILON_WE == (0.005 if eps is None else eps)
        _assert_planes(pre._gradients_dev.cpu().numpy(), want, tol=1e-5)
        assert rel_l2(pre._gradients_dev.cpu().numpy(), raw._gradients_dev.cpu().numpy()) > 0.1      # it did something
        g_rho, g_a, g_b = (np.flipud(a) for a in pre.get_fwi_gradients(["seis"]))
        _assert_planes(np.stack([g_a, g_b, g_rho]), want, tol=1e-5)
    d3 = make()
    d3.EPRECOND = 3                                                # accepted as a name, refused where it would act
    d3.set_observed(*obs)
    with pytest.raises(api.MifwiError):
        d3.grad(model, src, rec)
    with pytest.raises(api.MifwiError):
        d3.TIMEWIN = 1
    with pytest.raises(api.MifwiError):
        d3.SWS_TAPER_GRAD_SOURCES = 1
