"""The refusals of the host code the three propagators share (physicsbasedfwi2_amd/_driver.py: the autograd function, the
linearised driver, the pseudo-Hessian holder's base), word for word as each physics phrases them.  Every one is a Python
exception raised before the launch it refuses; the grids are the smallest off the tile sizes (37 x 50, 36 x 50 with an
8-cell C-PML), 3 shots, 24 steps."""
import pytest
import torch

from cases import acoustic_case, elastic_case, fluid_planes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PHYSICS = ["acoustic", "elastic", "fluid"]
MODEL = {"acoustic": "r", "elastic": "mat", "fluid": "mat"}
_cases = {}


def _module(physics):
    import importlib
    return importlib.import_module("physicsbasedfwi2_amd." + physics)


def _case(physics):
    """(model, f, the positional arguments after them) on the device, built once per physics and never modified."""
    if physics not in _cases:
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
        if physics == "acoustic":
            c = acoustic_case(seed=3, n0=21, n1=34, nb=8, nt=24, ns=3, nrec=5)
            model, rest = t(c["r"]), [torch.tensor(c[k]) for k in ("q0", "q1", "sc", "sw", "rc", "rw")] + [c["c0"], c["c1"]]
        else:
            c = fluid_planes(elastic_case(seed=3, nz=36, nx=50, fw=8, nt=24, ns=3, nrec=5), 0)
            model = t(c["mat" if physics == "elastic" else "mat3"])
            rest = [torch.tensor(c[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")] + [c["fw"]]
        _cases[physics] = (model, t(c["f"]), rest)
    return _cases[physics]


def _propagate(physics, grad=True, **kw):
    model, f, rest = _case(physics)
    model = model.clone().requires_grad_(grad)
    out = _module(physics).propagate(model, f, *rest, **kw)
    return model, (out if isinstance(out, tuple) else (out,))


def _linearised(physics, fn, **kw):
    """born / gauss_newton_product with a perturbation of the model's shape; acoustic.born takes (r, f, dr, ...)."""
    model, f, rest = _case(physics)
    mod = _module(physics)
    if physics == "acoustic" and fn == "born":
        return mod.born(model, f, 0.01 * model, *rest, **kw)
    return getattr(mod, fn)(model, 0.01 * model, f, *rest, **kw)


@pytest.mark.parametrize("physics", PHYSICS)
def test_a_second_backward_is_refused(physics):
    mod = _module(physics)
    model, out = _propagate(physics)
    loss = sum((t ** 2).sum() for t in out)
    loss.backward(retain_graph=True)
    assert float(model.grad.abs().max()) > 0
    with pytest.raises(mod.MifwiError, match="backward through the %s propagator was called twice" % physics):
        loss.backward()


@pytest.mark.parametrize("physics", PHYSICS)
def test_a_holder_needs_a_run_that_requires_a_gradient(physics):
    mod = _module(physics)
    with pytest.raises(mod.MifwiError, match="neither %s nor f requires a gradient" % MODEL[physics]):
        _propagate(physics, grad=False, pseudo_hessian=mod.PseudoHessian())


@pytest.mark.parametrize("physics", PHYSICS)
def test_a_holder_of_another_physics_is_refused(physics):
    mod = _module(physics)
    other = _module(PHYSICS[(PHYSICS.index(physics) + 1) % 3]).PseudoHessian()
    article = "a" if physics == "fluid" else "an"
    with pytest.raises(mod.MifwiError, match=r"must be %s %s\.PseudoHessian holder" % (article, physics)):
        _propagate(physics, pseudo_hessian=other)


@pytest.mark.parametrize("physics", PHYSICS)
def test_a_holder_without_moments_has_no_hessian(physics):
    mod = _module(physics)
    holder = mod.PseudoHessian()
    plane = torch.ones(4, 4)
    calls = {"acoustic": [lambda: holder.hessian_velocity(plane, 0.3, 0), lambda: holder.hessian_slowness2(plane, 0.3)],
             "elastic": [lambda: holder.hessian(plane, plane, plane, 1e-3, 10.0)],
             "fluid": [lambda: holder.hessian(plane, plane, 1e-3, 10.0)]}[physics]
    for call in calls:
        with pytest.raises(mod.MifwiError, match="no moments yet"):
            call()


@pytest.mark.parametrize("fn", ["born", "gauss_newton_product"])
@pytest.mark.parametrize("physics", PHYSICS)
def test_a_budget_below_one_shot_is_refused(physics, fn):
    with pytest.raises(_module(physics).MifwiError, match="not even one shot's fit"):
        _linearised(physics, fn, snapshot_budget=1)


@pytest.mark.parametrize("fn", ["born", "gauss_newton_product"])
def test_what_the_elastic_linearised_passes_do_not_serve(monkeypatch, fn):
    from physicsbasedfwi2_amd import elastic
    only = "%s serves explosive sources and velocity receivers only" % fn
    with pytest.raises(elastic.MifwiError, match=only):
        _linearised("elastic", fn, source_type="fx")
    with pytest.raises(elastic.MifwiError, match=only):
        _linearised("elastic", fn, record_pressure=True)
    monkeypatch.setenv("MIFWI_EL_CLUSTER", "0")           # the per-step kernels: the plan keeps bf16 planes when asked to
    monkeypatch.setenv("MIFWI_EL_CLUSTER_ADJ", "0")
    with pytest.raises(elastic.MifwiError, match="%s reads f32 snapshot planes: this plan keeps them as bf16" % fn):
        _linearised("elastic", fn, snapshot_format="bf16")


WEIGHT_TEXT = {"acoustic": "weight must return a tensor of the shape of its argument",
               "elastic": r"weight must return \(g_vx, g_vz\) of the shape of its arguments",
               "fluid": "weight must return 2 tensors of the shape of its arguments"}


@pytest.mark.parametrize("physics", PHYSICS)
def test_a_weight_of_the_wrong_shape_or_count_is_refused(physics):
    mod = _module(physics)
    one = physics == "acoustic"
    short = (lambda d: d[:-1]) if one else (lambda *d: tuple(t[:-1] for t in d))
    with pytest.raises(mod.MifwiError, match=WEIGHT_TEXT[physics]):
        _linearised(physics, "gauss_newton_product", weight=short)
    if not one:
        with pytest.raises(mod.MifwiError, match=WEIGHT_TEXT[physics]):
            _linearised(physics, "gauss_newton_product", weight=lambda *d: d[:1])
    if physics == "fluid":
        with pytest.raises(mod.MifwiError, match="weight must return 3 tensors of the shape of its arguments"):
            _linearised(physics, "gauss_newton_product", record_pressure=True, weight=lambda *d: d[:2])
