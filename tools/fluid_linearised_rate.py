#!/usr/bin/env python3
"""The linearised passes of the fluid propagator next to the elastic route, and what the pseudo-Hessian's moments cost.

1. fluid.gauss_newton_product (background forward with resident snapshots, Born pass, adjoint pass) against
   elastic.gauss_newton_product on mat5 = [K, K, 0, bx, bz] and dmat5 = [dK, dK, 0, dbx, dbz]: the same medium, explosive
   sources, velocity receivers, free surface.  One process, device events around the whole call, one warm-up call of each
   route, then five alternating windows of PASSES back-to-back calls each; plan creation and allocations are part of a
   call, as they are for a caller.  The two routes' hv (planes K = L + M, bx, bz) and drec are compared in the same run.
2. mifwi_fluid_snapshot_moments at stride 1 and 4 over the resident snapshots of that case against mifwi_fluid_backward
   over the same steps (the adjoint pass the moments ride on), each alone between device events, same windows.
Case: 350x1700, 90 steps, 32 shots.  Needs a GPU:

    python tools/fluid_linearised_rate.py [out.json]          ->  profiles/r14_fluid_linearised.json
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import _lib, elastic, fluid, profiles  # noqa: E402
from physicsbasedfwi2_amd._driver import ptrs, run_forward  # noqa: E402

NZ, NX, NS, NT = 350, 1700, 32, 90
REPS, PASSES = 5, 4
FW, H, NREC = 10, 10.0, 64


def windows(calls):
    """{name: [ms per call of each window]}: one warm-up call of each, then REPS alternating windows of PASSES calls."""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(REPS):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PASSES):
                fn()
            b.record()
            b.synchronize()
            t[k].append(a.elapsed_time(b) / PASSES)
    return t


def summary(v):
    return {"ms": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3),
            "spread": round((max(v) - min(v)) / min(v), 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/fluid_linearised_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, NZ)[:, None]
    vp = torch.tensor(1500.0 + 2500.0 * z + 100.0 * rng.random((NZ, NX)), dtype=torch.float32, device=dev)
    rho = 1000.0 + 0.3 * vp
    dt = 0.8 * profiles.elastic_cfl_limit(H, float(vp.max()))
    pz = torch.tensor(profiles.cpml_tables(NZ, FW, H, dt, 3000.0, 5.0, low=False), dtype=torch.float32)
    px = torch.tensor(profiles.cpml_tables(NX, FW, H, dt, 3000.0, 5.0), dtype=torch.float32)
    wav = (profiles.ricker(30.0, NT, dt, 0.04)[:, None, None] * torch.ones(1, NS, 1)).to(dev).contiguous()
    f = wav * (dt / (H * H))
    sx = torch.linspace(20, NX - 21, NS).long()
    sc = (12 * NX + sx).to(torch.int32).reshape(NS, 1, 1).to(dev)
    rx = torch.linspace(12, NX - 13, NREC).long()
    rc = (14 * NX + rx).to(torch.int32).reshape(1, NREC, 1).repeat(NS, 1, 1).contiguous().to(dev)
    sw, rw = torch.ones(NS, 1, 1, device=dev), torch.ones(NS, NREC, 1, device=dev)
    with torch.no_grad():
        mat3 = fluid.materials(vp, rho, dt, H, free_surface=True)
        dmat3 = mat3 * torch.tensor(0.01 * rng.standard_normal((3, NZ, NX)), dtype=torch.float32, device=dev)
        zero = torch.zeros_like(mat3[0])
        mat5 = torch.stack([mat3[0], mat3[0], zero, mat3[1], mat3[2]])
        dmat5 = torch.stack([dmat3[0], dmat3[0], zero, dmat3[1], dmat3[2]])
    geo = (sc, sw, rc, rw)
    out = {}

    def gn_fluid():
        out["fluid"] = fluid.gauss_newton_product(mat3, dmat3, f, pz, px, *geo, FW, free_surface=True)

    def gn_elastic():
        out["elastic"] = elastic.gauss_newton_product(mat5, dmat5, f, pz, px, *geo, FW, free_surface=True)
    t = windows({"elastic": gn_elastic, "fluid": gn_fluid})
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    (hf, fx_, fz_), (he, ex_, ez_) = out["fluid"], out["elastic"]
    assert float(he.abs().max()) > 0 and float(ex_.abs().max()) > 0, "the product is empty"
    plan = elastic.ElasticPlan(NZ, NX, NT, NS, 1, NREC, 1, FW, 0, free_surface=1)
    family = elastic.kernel_family(plan.layout.kernel_flags)
    plan.close()
    me, mf = statistics.median(t["elastic"]), statistics.median(t["fluid"])
    product = {"elastic_kernels": list(family) + ["Born: one launch per half step"],
               "elastic": summary(t["elastic"]), "fluid": summary(t["fluid"]), "fluid_over_elastic": round(mf / me, 4),
               "hv_K_rel_l2": rel(hf[0][1:], (he[0] + he[1])[1:]), "hv_bx_rel_l2": rel(hf[1], he[3]),
               "hv_bz_rel_l2": rel(hf[2], he[4]), "drec_vx_rel_l2": rel(fx_, ex_), "drec_vz_rel_l2": rel(fz_, ez_)}
    del out, hf, he
    torch.cuda.empty_cache()

    # ---- the moments pass next to the adjoint pass it rides on ------------------------------------------------------
    lib = _lib.load()
    plan = fluid.FluidPlan(NZ, NX, NT, NS, 1, NREC, 1, FW, 0, 0, 1, 0, 4)
    lay = plan.layout
    mat_p, pz_d, px_p = elastic._padded_inputs(mat3, pz, px, lay.gp)
    coef, g = ptrs(mat_p, pz_d, px_p), ptrs(*geo)
    rvx, rvz = (torch.empty((NT, NS, NREC), device=dev) for _ in range(2))
    work = torch.empty(max(lay.work_forward_elems, lay.work_backward_elems), device=dev)
    snap = torch.empty((NT, lay.snap_step_elems), device=dev)
    run_forward(fluid._forward_call(plan, coef, f.contiguous(), g, [rvx, rvz]), NT, NT, work, lay.state_elems, snap)
    grad = torch.empty((3, NZ, lay.gp), device=dev)
    mom = torch.empty((3, NZ, lay.gp), device=dev)
    mwork = torch.empty(lib.mifwi_fluid_snapshot_moments_work_elems(plan.handle), device=dev)
    adjoint = fluid._adjoint_call(plan, coef, g, [rvx, rvz], grad, None, work)

    def moments(stride):
        _lib.check(lib.mifwi_fluid_snapshot_moments(plan.handle, _lib.ptr(snap), 0, 0, NT, stride, _lib.ptr(mom),
                                                    _lib.ptr(mwork), _lib.ZERO_STATE, None))
    t2 = windows({"adjoint": lambda: adjoint(_lib.ptr(snap), 0, NT - 1, 0, _lib.ZERO_STATE | _lib.FINALIZE),
                  "moments_stride_1": lambda: moments(1), "moments_stride_4": lambda: moments(4)})
    assert float(mom.abs().max()) > 0 and float(grad.abs().max()) > 0
    plan.close()
    ma = statistics.median(t2["adjoint"])
    mom_doc = {k: summary(v) for k, v in t2.items()}
    for k in ("moments_stride_1", "moments_stride_4"):
        mom_doc[k]["share_of_adjoint"] = round(statistics.median(t2[k]) / ma, 4)
    mom_doc["snapshot_gb"] = round(4.0 * NT * lay.snap_step_elems / 1e9, 2)

    doc = {"how": "device events; one warm-up call of each, then %d alternating windows of %d calls; ms per call.  product: "
                  "gauss_newton_product end to end (plan, allocations, background forward, Born pass, adjoint pass), free "
                  "surface, %d-cell C-PML, explosive sources, %d velocity receivers per shot.  moments: the C entry alone over "
                  "the resident snapshots of the run, next to mifwi_fluid_backward over the same %d steps"
                  % (REPS, PASSES, FW, NREC, NT),
           "device": torch.cuda.get_device_name(dev), "grid": [NZ, NX], "shots": NS, "steps": NT,
           "gauss_newton_product": product, "moments": mom_doc}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_fluid_linearised.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
