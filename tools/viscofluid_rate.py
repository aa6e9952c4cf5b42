#!/usr/bin/env python3
"""One gradient pass - materials, forward, misfit.l2_half on both velocity components, backward - of the viscoacoustic
route (physicsbasedfwi2_amd.viscofluid: four fields per shot, four material planes) next to the two routes a marine user
had before it, on the same tree: ``visco.propagate`` with Vs = 0 (eight fields, eight planes - the route it replaces) and
the lossless ``fluid.propagate`` (three fields, three planes - the floor).  What the viscoacoustic kernels add to the
fluid's per cell and step: r read and written and the R plane read in the P launch (12 B on 36 B); r_bar and the R plane
read in the adjoint-P launch (own cells; the halo cells on top), r_bar read and written in the adjoint-V launch, one more
accumulator per shot group (about 28 B on 48 B).  One process, device events around the whole pass, one warm-up pass of each
route, then five alternating windows of PASSES back-to-back passes (plan creation and allocations are part of a pass, as
they are for a caller).  The timed model has qp = 80; the viscoacoustic and the viscoelastic pass compute the same
objective, and their losses and Vp / rho gradients are reported side by side.  Needs a GPU:

    python tools/viscofluid_rate.py [out.json]          ->  profiles/r23_viscofluid_rate.json
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import fluid, misfit, profiles, visco, viscofluid  # noqa: E402

# (nz, nx, shots, steps)
CASES = [(350, 1700, 8, 90), (100, 300, 32, 90)]
ROUTES = ("visco_vs0", "fluid", "viscofluid")
REPS, PASSES = 5, 40
FW, H, NREC = 10, 10.0, 64
F0, QP = 30.0, 80.0


def run_case(nz, nx, ns, nt, dev):
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, nz)[:, None]
    vp0 = torch.tensor(1500.0 + 2500.0 * z + 100.0 * rng.random((nz, nx)), dtype=torch.float32, device=dev)
    rho0 = 1000.0 + 0.3 * vp0
    qp, inf = torch.full_like(vp0, QP), torch.full_like(vp0, float("inf"))
    dt = 0.8 * profiles.elastic_cfl_limit(H, viscofluid.max_velocity(vp0, qp, F0, F0))
    pz = torch.tensor(profiles.cpml_tables(nz, FW, H, dt, 3000.0, 5.0, low=False), dtype=torch.float32)
    px = torch.tensor(profiles.cpml_tables(nx, FW, H, dt, 3000.0, 5.0), dtype=torch.float32)
    wav = (profiles.ricker(F0, nt, dt, 0.04)[:, None, None] * torch.ones(1, ns, 1)).to(dev).contiguous()
    f = wav * (dt / (H * H))
    sx = torch.linspace(20, nx - 21, ns).long()
    sc = (12 * nx + sx).to(torch.int32).reshape(ns, 1, 1).to(dev)
    rx = torch.linspace(12, nx - 13, NREC).long()
    rc = (14 * nx + rx).to(torch.int32).reshape(1, NREC, 1).repeat(ns, 1, 1).contiguous().to(dev)
    sw, rw = torch.ones(ns, 1, 1, device=dev), torch.ones(ns, NREC, 1, device=dev)
    obs = {}

    def gradient_pass(route):
        vp, rho = (t.clone().requires_grad_(True) for t in (vp0, rho0))
        if route == "visco_vs0":
            mat = visco.materials(vp, torch.zeros_like(vp), rho, qp, inf, F0, F0, dt, H, free_surface=True)
            rvx, rvz = visco.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, F0, dt, free_surface=True)
        elif route == "viscofluid":
            mat = viscofluid.materials(vp, rho, qp, F0, F0, dt, H, free_surface=True)
            rvx, rvz = viscofluid.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, F0, dt, free_surface=True)
        else:
            mat = fluid.materials(vp, rho, dt, H, free_surface=True)
            rvx, rvz = fluid.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, free_surface=True)
        if not obs:
            obs["x"], obs["z"] = 0.9 * rvx.detach(), 0.9 * rvz.detach()
        loss = misfit.l2_half(rvx, obs["x"]) + misfit.l2_half(rvz, obs["z"])
        loss.backward()
        return loss.detach(), vp.grad, rho.grad

    def timed(route):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PASSES):
            gradient_pass(route)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / PASSES

    ref = {r: gradient_pass(r) for r in ROUTES}     # warm-up of every route (the first one's traces make the observed data)
    torch.cuda.synchronize()
    t = {r: [] for r in ROUTES}
    for _ in range(REPS):
        for r in ROUTES:
            t[r].append(timed(r))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    le, gve, gre = ref["visco_vs0"]
    lv, gvv, grv = ref["viscofluid"]
    assert float(le) > 0 and float(gve.abs().max()) > 0 and float(gvv.abs().max()) > 0, "the gradient pass is empty"
    a, b = visco.relaxation(F0, dt)
    plan = viscofluid.ViscofluidPlan(nz, nx, nt, ns, 1, NREC, 1, FW, dev.index or 0, a, b, free_surface=1)
    passes = plan.pass_sizes()
    plan.close()
    spread = lambda v: (max(v) - min(v)) / min(v)
    med = {r: statistics.median(t[r]) for r in ROUTES}
    ratio = lambda num, den: [round(x / y, 4) for x, y in zip(t[num], t[den])]
    cellsteps = float(nz) * nx * ns * nt
    return {"grid": [nz, nx], "shots": ns, "steps": nt, "viscofluid_pass_sizes": list(passes),
            "ms": {r: [round(v, 3) for v in t[r]] for r in ROUTES},
            "median_ms": {r: round(med[r], 3) for r in ROUTES}, "spread": {r: round(spread(t[r]), 4) for r in ROUTES},
            "gcellsteps_per_s": {r: round(cellsteps / med[r] / 1e6, 2) for r in ROUTES},
            "viscofluid_over_visco_vs0": round(med["viscofluid"] / med["visco_vs0"], 4),
            "viscofluid_over_visco_vs0_by_window": ratio("viscofluid", "visco_vs0"),
            "viscofluid_over_fluid": round(med["viscofluid"] / med["fluid"], 4),
            "viscofluid_over_fluid_by_window": ratio("viscofluid", "fluid"),
            "loss": {"visco_vs0": float(le), "viscofluid": float(lv), "fluid": float(ref["fluid"][0])},
            "two_routes_loss_rel_diff": abs(float(lv) - float(le)) / float(le),
            "two_routes_vp_grad_rel_l2": rel(gvv, gve), "two_routes_rho_grad_rel_l2": rel(grv, gre)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/viscofluid_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    doc = {"how": "device events around one gradient pass (materials, forward, misfit.l2_half of vx and vz, backward) of each "
                  "route, free surface, %d-cell C-PML, %d receivers per shot, explosive sources, Vs = 0, qp = %g, f_relax = "
                  "f_ref = %g Hz; one warm-up pass of each, then %d alternating windows of %d passes; ms per pass, end to end, "
                  "of a 90-step sample.  visco_vs0: visco.propagate on visco.materials(vp, 0, rho, qp, inf); fluid: the "
                  "lossless fluid.propagate on the same vp, rho; two_routes_*: the viscoacoustic pass against the "
                  "viscoelastic one, the same objective" % (FW, NREC, QP, F0, REPS, PASSES),
           "bytes_per_cell_step_model": {"forward": {"fluid": 36, "viscofluid": 48, "visco_vs0": 96},
                                         "adjoint": {"fluid": 48, "viscofluid": 76}},
           "device": torch.cuda.get_device_name(dev),
           "cases": [run_case(*c, dev) for c in CASES]}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_viscofluid_rate.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
