#!/usr/bin/env python3
"""One gradient pass of a PHYSICS = 2 medium - materials, forward, misfit.l2_half on both velocity components, backward -
through the fluid kernels (physicsbasedfwi2_amd.fluid) next to the elastic kernels on staggered_materials(vp, 0, rho),
the route the pyapi_denise shim takes by default.  One process, device events around the whole pass, one warm-up pass of
each route, then five alternating windows of PASSES back-to-back passes each (a quarter of a second per window on the
large grid; plan creation and allocations are part of a pass, as they are for a caller); the two routes' losses and
Vp / rho gradients are compared in the same run.  The figures are end-to-end times of a pass over a 90-step sample.  Cases: 350x1700 x 8 shots (a 90-step sample; both routes stream from the Infinity Cache / HBM, one launch per
(half) step) with an explosive and with an fx source, 100x300 x 32 shots with fx (both routes per-step) and with an
explosive source (the elastic route runs its single-launch time loops there; no bar is set for that one).  Needs a GPU:

    python tools/fluid_rate.py [out.json]          ->  profiles/r13_fluid_rate.json
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import elastic, fluid, misfit, profiles  # noqa: E402

# (nz, nx, shots, steps, source)
CASES = [(350, 1700, 8, 90, "explosive"), (350, 1700, 8, 90, "fx"), (100, 300, 32, 90, "fx"), (100, 300, 32, 90, "explosive")]
REPS, PASSES = 5, 20
FW, H, NREC = 10, 10.0, 64


def run_case(nz, nx, ns, nt, kind, dev):
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, nz)[:, None]
    vp0 = torch.tensor(1500.0 + 2500.0 * z + 100.0 * rng.random((nz, nx)), dtype=torch.float32, device=dev)
    rho0 = 1000.0 + 0.3 * vp0
    dt = 0.8 * profiles.elastic_cfl_limit(H, float(vp0.max()))
    pz = torch.tensor(profiles.cpml_tables(nz, FW, H, dt, 3000.0, 5.0, low=False), dtype=torch.float32)
    px = torch.tensor(profiles.cpml_tables(nx, FW, H, dt, 3000.0, 5.0), dtype=torch.float32)
    # (a wavelet that has passed its peak within the sample: losses and gradients of full size, not a start-up ramp)
    wav = (profiles.ricker(30.0, nt, dt, 0.04)[:, None, None] * torch.ones(1, ns, 1)).to(dev).contiguous()
    sx = torch.linspace(20, nx - 21, ns).long()
    sc = (12 * nx + sx).to(torch.int32).reshape(ns, 1, 1).to(dev)
    rx = torch.linspace(12, nx - 13, NREC).long()
    rc = (14 * nx + rx).to(torch.int32).reshape(1, NREC, 1).repeat(ns, 1, 1).contiguous().to(dev)
    sw, rw = torch.ones(ns, 1, 1, device=dev), torch.ones(ns, NREC, 1, device=dev)
    obs = {}

    def gradient_pass(route):
        vp, rho = vp0.clone().requires_grad_(True), rho0.clone().requires_grad_(True)
        if route == "fluid":
            mod, mat = fluid, fluid.materials(vp, rho, dt, H, free_surface=True)
        else:
            mod, mat = elastic, elastic.staggered_materials(vp, torch.zeros_like(vp), rho, dt, H, free_surface=True)
        f = wav * (dt / (H * H)) if kind == "explosive" else mod.force_amplitude(wav, mat, sc, sw, H, kind)
        rvx, rvz = mod.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, free_surface=True, source_type=kind)
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

    ref = {r: gradient_pass(r) for r in ("elastic", "fluid")}               # warm-up of both routes (and the observed data)
    torch.cuda.synchronize()
    t = {"elastic": [], "fluid": []}
    for _ in range(REPS):
        for r in ("elastic", "fluid"):
            t[r].append(timed(r))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    (le, gve, gre), (lf, gvf, grf) = ref["elastic"], ref["fluid"]
    assert float(le) > 0 and float(gve.abs().max()) > 0, "the gradient pass is empty"
    plan = elastic.ElasticPlan(nz, nx, nt, ns, 1, NREC, 1, FW, dev.index or 0, free_surface=1,
                               source_type=elastic.SOURCE_TYPES[kind])
    family = elastic.kernel_family(plan.layout.kernel_flags)
    plan.close()
    me, mf = statistics.median(t["elastic"]), statistics.median(t["fluid"])
    spread = lambda v: (max(v) - min(v)) / min(v)
    cellsteps = float(nz) * nx * ns * nt
    return {"grid": [nz, nx], "shots": ns, "steps": nt, "source": kind, "elastic_kernels": list(family),
            "elastic_ms": [round(v, 3) for v in t["elastic"]], "fluid_ms": [round(v, 3) for v in t["fluid"]],
            "elastic_median_ms": round(me, 3), "fluid_median_ms": round(mf, 3),
            "elastic_spread": round(spread(t["elastic"]), 4), "fluid_spread": round(spread(t["fluid"]), 4),
            "fluid_over_elastic": round(mf / me, 4),
            "elastic_gcellsteps_per_s": round(cellsteps / me / 1e6, 2), "fluid_gcellsteps_per_s": round(cellsteps / mf / 1e6, 2),
            "loss_rel_diff": abs(float(lf) - float(le)) / float(le),
            "vp_grad_rel_l2": rel(gvf, gve), "rho_grad_rel_l2": rel(grf, gre)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/fluid_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    doc = {"how": "device events around one gradient pass (materials, forward, misfit.l2_half of vx and vz, backward) of each "
                  "route, free surface, %d-cell C-PML, %d receivers per shot; one warm-up pass of each, then %d alternating "
                  "windows of %d passes; ms per pass, end to end, of a 90-step sample" % (FW, NREC, REPS, PASSES),
           "device": torch.cuda.get_device_name(dev),
           "cases": [run_case(*c, dev) for c in CASES]}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_fluid_rate.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
