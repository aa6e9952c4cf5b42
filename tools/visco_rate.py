#!/usr/bin/env python3
"""One gradient pass - materials, forward, misfit.l2_half on both velocity components, backward - of the viscoelastic
route (physicsbasedfwi2_amd.visco, eight material planes, three memory variables per shot) next to the isotropic elastic
route forced onto the same kernels: one launch per half step, no fused V+S step (MIFWI_EL_CLUSTER=0 MIFWI_EL_CLUSTER_ADJ=0
MIFWI_EL_FUSED=0).  What the viscoelastic kernels add per cell and step: three fields read and written and three planes
read in the S launch (36 B); three fields and three planes read (own cells; the halo cells on top) in the adjoint-S launch
and three fields read and written in the adjoint-V launch (48 B); three more accumulators per shot group.  The adjoint-S
launch runs at two waves per SIMD instead of three.  On 100x300 the default elastic plan is timed too: its single-launch
time loops are what a viscoelastic run gives up there.  One process, device events around the whole pass, one warm-up pass
of each route, then five alternating windows of PASSES back-to-back passes (plan creation and allocations are part of a
pass, as they are for a caller).  The timed viscoelastic model has qp = 80, qs = 50; a pass with qp = qs = inf, the same
medium as the elastic route's, is compared with it in the same run (loss, Vp and rho gradients).  Needs a GPU:

    python tools/visco_rate.py [out.json]          ->  profiles/r17_visco_rate.json
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import elastic, misfit, profiles, visco  # noqa: E402

# (nz, nx, shots, steps, routes)
CASES = [(350, 1700, 8, 90, ("elastic_per_step", "visco")), (100, 300, 32, 90, ("elastic_per_step", "visco", "elastic_default"))]
PER_STEP = {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_FUSED": "0"}
REPS, PASSES = 5, 40
FW, H, NREC = 10, 10.0, 64
F0, QP, QS = 30.0, 80.0, 50.0


def run_case(nz, nx, ns, nt, routes, dev):
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, nz)[:, None]
    vp0 = torch.tensor(1500.0 + 2500.0 * z + 100.0 * rng.random((nz, nx)), dtype=torch.float32, device=dev)
    vs0 = vp0 / 3.0 ** 0.5
    vs0[:12] = 0.0
    rho0 = 1000.0 + 0.3 * vp0
    q = {"visco": (torch.full_like(vp0, QP), torch.full_like(vp0, QS)),
         "visco_lossless": (torch.full_like(vp0, float("inf")), torch.full_like(vp0, float("inf")))}
    dt = 0.8 * profiles.elastic_cfl_limit(H, visco.max_velocity(vp0, q["visco"][0], F0, F0))
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
        for k in PER_STEP:
            os.environ.pop(k, None)
        if route == "elastic_per_step":
            os.environ.update(PER_STEP)
        vp, vs, rho = (t.clone().requires_grad_(True) for t in (vp0, vs0, rho0))
        if route in q:
            mat = visco.materials(vp, vs, rho, *q[route], F0, F0, dt, H, free_surface=True)
            rvx, rvz = visco.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, F0, dt, free_surface=True)
        else:
            mat = elastic.staggered_materials(vp, vs, rho, dt, H, free_surface=True)
            rvx, rvz = elastic.propagate(mat, f, pz, px, sc, sw, rc, rw, FW, free_surface=True)
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

    ref = {r: gradient_pass(r) for r in routes + ("visco_lossless",)}     # warm-up of every route (and the observed data)
    torch.cuda.synchronize()
    t = {r: [] for r in routes}
    for _ in range(REPS):
        for r in routes:
            t[r].append(timed(r))
    for k in PER_STEP:
        os.environ.pop(k, None)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    le, gve, gre = ref["elastic_per_step"]
    lv, gvv, grv = ref["visco_lossless"]
    la = ref["visco"][0]
    assert float(le) > 0 and float(gve.abs().max()) > 0, "the gradient pass is empty"
    plan = elastic.ElasticPlan(nz, nx, nt, ns, 1, NREC, 1, FW, dev.index or 0, free_surface=1)
    family = elastic.kernel_family(plan.layout.kernel_flags)
    plan.close()
    spread = lambda v: (max(v) - min(v)) / min(v)
    med = {r: statistics.median(t[r]) for r in routes}
    cellsteps = float(nz) * nx * ns * nt
    out = {"grid": [nz, nx], "shots": ns, "steps": nt, "default_elastic_kernels": list(family),
           "ms": {r: [round(v, 3) for v in t[r]] for r in routes},
           "median_ms": {r: round(med[r], 3) for r in routes}, "spread": {r: round(spread(t[r]), 4) for r in routes},
           "gcellsteps_per_s": {r: round(cellsteps / med[r] / 1e6, 2) for r in routes},
           "visco_over_elastic_per_step": round(med["visco"] / med["elastic_per_step"], 4),
           "lossless_loss_rel_diff": abs(float(lv) - float(le)) / float(le), "lossless_vp_grad_rel_l2": rel(gvv, gve),
           "lossless_rho_grad_rel_l2": rel(grv, gre), "attenuating_loss_over_elastic_loss": float(la) / float(le)}
    if "elastic_default" in routes:
        out["visco_over_elastic_default"] = round(med["visco"] / med["elastic_default"], 4)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/visco_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    doc = {"how": "device events around one gradient pass (materials, forward, misfit.l2_half of vx and vz, backward) of each "
                  "route, free surface, %d-cell C-PML, %d receivers per shot, explosive sources, qp = %g, qs = %g, f_relax = "
                  "f_ref = %g Hz; one warm-up pass of each, then %d alternating windows of %d passes; ms per pass, end to end, "
                  "of a 90-step sample.  elastic_per_step: the isotropic kernels with %s.  lossless_*: a viscoelastic pass "
                  "with qp = qs = inf against the elastic pass" % (FW, NREC, QP, QS, F0, REPS, PASSES, " ".join(
                      "%s=%s" % kv for kv in sorted(PER_STEP.items()))),
           "extra_bytes_per_cell_step": {"forward_S": 36, "adjoint_S_own_cells": 24, "adjoint_V": 24,
                                         "accumulators_per_shot_group": 24},
           "device": torch.cuda.get_device_name(dev),
           "cases": [run_case(*c, dev) for c in CASES]}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_visco_rate.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
