#!/usr/bin/env python3
"""Cost of the acoustic pseudo-Hessian and Gauss-Newton product on the C2 grid (174 x 500 model, 29 shots, 300 steps):
with the reference's 20-cell sponge and with a 10-cell C-PML,

  * the moments pass (mifwi_acoustic_snapshot_moments, stride 1 and stride 4) next to the adjoint sweep of the same
    backward (mifwi_acoustic_backward over the same resident snapshots): device events, one warm-up, median / min / max
    of five calls; and the pass's byte rate - 4 B per cell-step read - against the 6.3 TB/s HBM streams reach;
  * acoustic.gauss_newton_product against the composition born + propagate + backward, which runs the background
    forward twice and is code the product does not touch: the gain expected is about one forward sweep;
  * the VGPR and scratch use of the new kernels, as the compiler reports them (no GPU needed for this part):

    python tools/acoustic_hessian_rate.py --resources   ->  "kernel_resources" of profiles/r09_acoustic_hessian.json
    python tools/acoustic_hessian_rate.py [out.json]    ->  everything else (needs a GPU; keeps "kernel_resources")
"""
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import _lib, acoustic, build, profiles  # noqa: E402

NZ, NX, NS, NT, H, DT = 174, 500, 29, 300, 10.0, 0.001
LAYERS = [("sponge", 20), ("cpml", 10)]
REPS = 5
HBM_ACHIEVABLE = 6.3e12
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r09_acoustic_hessian.json")
KERNELS = ("ac_snapshot_moments", "moments_sum", "ac_hess_velocity", "ac_hess_slowness2")


def kernel_resources():
    """VGPRs, scratch and occupancy of the new kernels from hipcc -Rpass-analysis=kernel-resource-usage."""
    out = {}
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    for src in ("mifwi_acoustic.hip", "mifwi_materials.hip"):
        text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, src)], check=True, text=True,
                              stderr=subprocess.PIPE).stderr
        for block in text.split("Function Name: ")[1:]:
            name = next((k for k in KERNELS if k in block.split()[0]), None)
            if name is None or (name == "moments_sum" and src != "mifwi_acoustic.hip"):
                continue
            grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
            out[name] = {"vgprs": grab("VGPRs"), "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                         "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]")}
    missing = [k for k in KERNELS if k not in out]
    if missing:
        raise SystemExit("no resource report for %s" % missing)
    return out


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_case(layer, width, dev):
    lib = _lib.load()
    n0, n1 = NZ + 2 * width, NX + 2 * width
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, NZ)[:, None]
    vp = np.pad(1500.0 + 2500.0 * z + 100.0 * rng.random((NZ, NX)), width, mode="edge")
    r = torch.tensor((vp * DT / H) ** 2, dtype=torch.float32, device=dev)
    dr = 0.02 * r * torch.randn(r.shape, device=dev)
    cpml = width if layer == "cpml" else 0
    if cpml:
        q0 = torch.tensor(profiles.cpml_tables(n0, width, H, DT, 4100.0, 10.0)[:2].copy(), dtype=torch.float32)
        q1 = torch.tensor(profiles.cpml_tables(n1, width, H, DT, 4100.0, 10.0)[:2].copy(), dtype=torch.float32)
    else:
        q0 = torch.tensor(profiles.sponge_q(n0, width, H, H, DT), dtype=torch.float32)
        q1 = torch.tensor(profiles.sponge_q(n1, width, H, H, DT), dtype=torch.float32)
    f = (profiles.ricker(8.0, NT, DT, 0.125)[:, None, None] * torch.ones(1, NS, 1) * (H * H)).to(dev).contiguous()
    sx = torch.linspace(0, NX - 1, NS).long() + width
    src_cell = (width * n1 + sx).to(torch.int32).reshape(NS, 1, 1).to(dev)
    rec_cell = (width * n1 + width + torch.arange(NX)).to(torch.int32).reshape(1, NX, 1).repeat(NS, 1, 1).contiguous().to(dev)
    src_w, rec_w = torch.ones(NS, 1, 1, device=dev), torch.ones(NS, NX, 1, device=dev)
    geo_t = (src_cell, src_w, rec_cell, rec_w)

    # ---- the moments pass next to the adjoint sweep, on the buffers a backward pass holds
    plan = acoustic.AcousticPlan(n0, n1, NT, NS, 1, NX, 1, 1.0, 1.0, dev.index or 0, 0, 0, cpml)
    lay = plan.layout
    gp = lay.gp
    r_p = torch.zeros((n0, gp), device=dev)
    r_p[:, :n1] = r
    q0_d = q0.to(dev).contiguous()
    q1_p = torch.zeros((2, gp) if cpml else (gp,), device=dev)
    q1_p[..., :n1] = q1.to(dev)
    P, st = _lib.ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    geo = [P(t) for t in geo_t]
    rec = torch.empty((NT, NS, NX), device=dev)
    snap = torch.empty((NT, NS, n0, gp), device=dev)
    work = torch.empty(max(lay.work_forward_elems, lay.work_backward_elems), device=dev)
    _lib.check(lib.mifwi_acoustic_forward(plan.handle, P(r_p), P(q0_d), P(q1_p), P(f), *geo, P(rec), P(snap), P(work), 0, NT,
                                          _lib.ZERO_STATE, st))
    g = rec.clone()
    grad = torch.empty((n0, gp), device=dev)
    mom = torch.empty((n0, gp), device=dev)
    mwork = torch.empty(lib.mifwi_acoustic_snapshot_moments_work_elems(plan.handle), device=dev)

    def adjoint():
        _lib.check(lib.mifwi_acoustic_backward(plan.handle, P(r_p), P(q0_d), P(q1_p), *geo, P(g), P(snap), 0, P(grad), None,
                                               P(work), NT - 1, 1, _lib.ZERO_STATE | _lib.FINALIZE, st))

    def moments(stride):
        _lib.check(lib.mifwi_acoustic_snapshot_moments(plan.handle, P(snap), 0, 0, NT - 1, stride, P(mom), P(mwork),
                                                       _lib.ZERO_STATE, st))
    passes = {"adjoint_sweep": adjoint, "moments_stride1": lambda: moments(1), "moments_stride4": lambda: moments(4)}
    for fn in passes.values():
        fn()                                                        # one warm-up of each
    torch.cuda.synchronize()
    ts = {k: [] for k in passes}
    for _ in range(REPS):
        for k, fn in passes.items():
            ts[k].append(timed(fn))
    assert bool(torch.isfinite(mom).all()) and float(mom.max()) > 0 and float(grad.abs().max()) > 0
    out = {"layer": "%s, %d cells" % (layer, width), "padded_grid": [n0, n1], "gp": gp, "shots": NS, "steps": NT,
           "single_launch_slabs": plan.cluster_slabs(), "moments_work_planes": int(mwork.numel() // lay.coef_elems)}
    for k in passes:
        out[k] = stats(ts[k])
    for stride in (1, 4):
        nsel = len(range(0, NT - 1, stride))
        nbytes = 4.0 * lay.coef_elems * NS * nsel
        rate = nbytes / (statistics.median(ts["moments_stride%d" % stride]) * 1e-3)
        out["moments_stride%d" % stride].update({"bytes_read": int(nbytes), "tb_per_s": round(rate / 1e12, 3),
                                                 "share_of_6.3_tb_per_s": round(rate / HBM_ACHIEVABLE, 3)})
    out["moments_stride1_over_adjoint_sweep"] = round(out["moments_stride1"]["median_ms"] / out["adjoint_sweep"]["median_ms"], 4)
    plan.close()
    del snap, work, mwork

    # ---- Gauss-Newton product against the composition born + propagate + backward
    host = (q0, q1) + geo_t

    def product():
        return acoustic.gauss_newton_product(r, dr, f, *host, 1.0, 1.0, cpml_width=cpml)[0]

    def composition():
        _, drec = acoustic.born(r, f, dr, *host, 1.0, 1.0, cpml_width=cpml)
        rr = r.clone().requires_grad_(True)
        acoustic.propagate(rr, f, *host, 1.0, 1.0, cpml_width=cpml).backward(drec)
        return rr.grad
    ways = {"gauss_newton_product": product, "born_propagate_backward": composition}
    res = {k: fn() for k, fn in ways.items()}                       # one warm-up of each
    torch.cuda.synchronize()
    a, b = res["gauss_newton_product"].double(), res["born_propagate_backward"].double()
    out["hv_rel_l2_product_vs_composition"] = float((a - b).norm() / b.norm())
    tw = {k: [] for k in ways}
    for _ in range(REPS):
        for k, fn in ways.items():
            tw[k].append(timed(fn))
    for k in ways:
        out[k] = stats(tw[k])
    out["composition_over_product"] = round(out["born_propagate_backward"]["median_ms"] / out["gauss_newton_product"]["median_ms"], 4)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else DEFAULT_OUT
    held = [p for p in (path, DEFAULT_OUT) if os.path.exists(p)]     # "kernel_resources" of an earlier --resources run
    doc = json.load(open(held[0])) if held else {}
    if "--resources" in sys.argv:
        doc["kernel_resources"] = kernel_resources()
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tools/acoustic_hessian_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around each call, one warm-up, median / min / max of %d alternating calls; "
                           "bytes = 4 B x padded cells x shots x selected steps" % REPS,
                    "device": torch.cuda.get_device_name(dev),
                    "cases": [run_case(layer, width, dev) for layer, width in LAYERS]})
        if "kernel_resources" not in doc:
            doc["kernel_resources"] = kernel_resources()
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
