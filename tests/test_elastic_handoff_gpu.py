"""The halo hand-off of the elastic single-launch time loops on the smallest slabs at which a receive can go wrong.

A slab takes six row-fields per hand-off from its neighbours (EcHandoff in csrc/mifwi_elastic_cluster.h); the adjoint
asks for them a pass ahead of where it needs them.  Every case forces the slab count (MIFWI_EL_NW), checks that the plan
took it, and compares with the oracle: seismograms bit for bit, gradients to 2e-5 (summation order).  conftest fails a
test whose time loop gave up and left the numbers to the per-step kernels.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cases import elastic_case, rel_l2

pytestmark = pytest.mark.gpu
TOL_GRAD = 2e-5
DEV = "cuda:0"

# id -> (nz, nx, nw, elastic_case keywords, fd_order)
CASES = {
    # four-row slabs: rows 0, 1 take from above and rows 2, 3 from below, no interior row; 75 groups: a row crosses a wave
    "16x300/4": (16, 300, 4, dict(nt=60), 4),
    # five-row slabs of 8 groups: all four boundary rows, and rows 0 and 1 of a column, sit in one wave
    "20x30/4": (20, 30, 4, dict(nt=60), 4),
    # two slabs: one neighbour each, and the top slab mirrors at the free surface
    "26x100/2-free-surface": (26, 100, 2, dict(nt=60, free_surface=True), 4),
    # uneven slabs (10, 10, 9 rows): rows R-2, R-1 differ between neighbours; nx is no multiple of 4
    "29x83/3": (29, 83, 3, dict(nt=60), 4),
    # 15 rows x 68 groups: no room for the pad, a wave's slot holds two classes, lane-halo form off
    "45x272/3": (45, 272, 3, dict(nt=60), 4),
    # the headline deal (13 x 75, two slots, lane halo on); 70 steps: the 32-step collective check runs twice and both
    # parities are reused many times
    "52x300/4": (52, 300, 4, dict(nt=70), 4),
    "29x83/3-no-cpml": (29, 83, 3, dict(nt=60, fw=0, water=0), 4),
    "29x83/3-second-order": (29, 83, 3, dict(nt=60), 2),
}


def _case(cid):
    nz, nx, nw, kw, fd = CASES[cid]
    kw = dict(dict(fw=6, ns=2, nrec=12), **kw)
    return elastic_case(seed=131 + nz + nx, nz=nz, nx=nx, **kw), kw


def _grad_seeds(shape, scale_x, scale_z):
    rng = np.random.default_rng(12)
    return ((rng.standard_normal(shape) * scale_x).astype(np.float32),
            (rng.standard_normal(shape) * scale_z).astype(np.float32))


_HIP = {}


def _hip(cid, monkeypatch):
    """Traces and gradients of one case through the library, computed once per session and left unchanged."""
    if cid in _HIP:
        return _HIP[cid]
    from physicsbasedfwi2_amd import elastic
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    nz, nx, nw, _, fd = CASES[cid]
    case, kw = _case(cid)
    monkeypatch.setenv("MIFWI_EL_NW", str(nw))
    pl = ElasticPlan(nz, nx, kw["nt"], 2, 1, 12, 1, kw["fw"], 0, free_surface=case["fs"], fd_order=fd)
    slabs = (pl.cluster_slabs(False), pl.cluster_slabs(True))
    pl.close()
    assert slabs == (nw, nw), slabs
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=DEV, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=DEV, requires_grad=True)
    rvx, rvz = elastic.propagate(mat, f, *[torch.tensor(case[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")],
                                 case["fw"], free_surface=bool(case["fs"]), fd_order=fd)
    hx, hz = rvx.detach().cpu().numpy(), rvz.detach().cpu().numpy()
    gx, gz = _grad_seeds(hx.shape, np.abs(hx).max(), np.abs(hz).max())
    torch.autograd.backward([rvx, rvz], [torch.tensor(gx, device=DEV), torch.tensor(gz, device=DEV)])
    _HIP[cid] = dict(vx=hx, vz=hz, gx=gx, gz=gz, gm=mat.grad.cpu().numpy(), gf=f.grad.cpu().numpy())
    return _HIP[cid]


@pytest.mark.parametrize("cid", list(CASES))
def test_handoff_on_small_slabs(oracle32, monkeypatch, cid):
    nz, nx, nw, _, fd = CASES[cid]
    case, _ = _case(cid)
    h = _hip(cid, monkeypatch)
    ovx, ovz, S = oracle32.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], case["sc"], case["sw"],
                                           case["rc"], case["rw"], save=True, free_surface=case["fs"], fd_order=fd)
    assert np.isfinite(h["vx"]).all() and np.abs(ovx).max() > 0 and np.abs(ovz).max() > 0
    print("max |hip-oracle| vx %.3e vz %.3e" % (np.abs(h["vx"] - ovx).max(), np.abs(h["vz"] - ovz).max()))
    assert np.array_equal(h["vx"], ovx) and np.array_equal(h["vz"], ovz)
    gm_o, gf_o = oracle32.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"], case["rc"],
                                           case["rw"], h["gx"], h["gz"], S, free_surface=case["fs"], fd_order=fd)
    errs = [rel_l2(h["gm"][k], gm_o[k]) for k in range(5)] + [rel_l2(h["gf"], gf_o)]
    print("gradient rel-L2", " ".join("%.2e" % e for e in errs))
    assert max(errs) <= TOL_GRAD, errs


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(root)r)
from test_elastic_handoff_gpu import CASES, _case
from physicsbasedfwi2_amd import _lib, elastic
cid = %(cid)r
case, kw = _case(cid)
dev = "cuda:0"
mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
vx, vz = elastic.propagate(mat, f, *[torch.tensor(case[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")], case["fw"])
seeds = np.load(sys.argv[1])
torch.autograd.backward([vx, vz], [torch.tensor(seeds["gx"], device=dev), torch.tensor(seeds["gz"], device=dev)])
lib = _lib.load()
np.savez(sys.argv[2], vx=vx.detach().cpu().numpy(), vz=vz.detach().cpu().numpy(), gm=mat.grad.cpu().numpy(),
         gf=f.grad.cpu().numpy(), counts=np.array([lib.mifwi_fallback_count(), lib.mifwi_agent_handoff_count()]))
"""


def test_handoff_through_the_fabric_gives_the_same_bits(monkeypatch, tmp_path):
    """The agent-scope tier: in the ablation build debug bit 128 makes every workgroup report another XCD, the placement
    check fails and the host repeats the launch with granules published through the fabric (the AG kernel variants).
    Four-row slabs in a fresh process: the bits of the plain run, no fall-back to the per-step kernels."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "physicsbasedfwi2_amd", "libmifwi_ablations.so")
    if not os.path.exists(lib):
        pytest.skip("ablation build not present (python __graft_entry__.py builds it)")
    cid = "16x300/4"
    ref = _hip(cid, monkeypatch)
    seeds, out, script = tmp_path / "seeds.npz", tmp_path / "abl.npz", tmp_path / "child.py"
    np.savez(seeds, gx=ref["gx"], gz=ref["gz"])
    script.write_text(_CHILD % {"tests": os.path.join(root, "tests"), "root": root, "cid": cid})
    env = dict(os.environ, MIFWI_LIB=lib, MIFWI_EL_CL_DBG="128", MIFWI_EL_NW=str(CASES[cid][2]))
    res = subprocess.run([sys.executable, str(script), str(seeds), str(out)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    abl = dict(np.load(out))
    fb, ag = (int(v) for v in abl["counts"])
    assert fb == 0 and ag > 0, (fb, ag)
    assert np.abs(ref["vx"]).max() > 0
    for k in ("vx", "vz", "gm", "gf"):
        assert np.array_equal(ref[k], abl[k]), k
