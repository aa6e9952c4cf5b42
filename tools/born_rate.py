#!/usr/bin/env python3
"""Per-step time of the elastic Born pass (mifwi_elastic_born) next to the two-launch forward step that WRITES the f32
snapshot planes the Born pass reads - same plan (MIFWI_EL_CLUSTER=0 MIFWI_EL_FUSED=0), same buffers, one process, device
events, five alternating repetitions of 200 steps after a warm-up of both.  Expectation: the two move the same bytes
(40 B/cell of state each way, 20 B/cell of planes written / read), so the ratio should be 1.  Needs a GPU:

    python tools/born_rate.py [out.json]          ->  profiles/r08_elastic_born.json
"""
import ctypes
import json
import os
import statistics
import sys

os.environ["MIFWI_EL_CLUSTER"] = "0"          # the two-launch per-step form of the forward, whatever the grid
os.environ["MIFWI_EL_CLUSTER_ADJ"] = "0"
os.environ["MIFWI_EL_FUSED"] = "0"

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import _lib, elastic, profiles  # noqa: E402
from physicsbasedfwi2_amd._driver import pad_columns  # noqa: E402

CASES = [(350, 1700, 6), (100, 300, 32)]
STEPS, WARMUP, REPS = 200, 20, 5


def run_case(nz, nx, ns, dev):
    lib = _lib.load()
    h, fw, nrec = 10.0, 10, 64
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, nz)[:, None]
    vp = torch.tensor(1500.0 + 2500.0 * z + 100.0 * rng.random((nz, nx)), dtype=torch.float32, device=dev)
    vs, rho = vp / 1.8, 1000.0 + 0.3 * vp
    dt = 0.8 * profiles.elastic_cfl_limit(h, float(vp.max()))
    mat = elastic.staggered_materials(vp, vs, rho, dt, h)
    dmat = 0.01 * mat * torch.randn(mat.shape, device=dev)
    pz = torch.tensor(profiles.cpml_tables(nz, fw, h, dt, 3000.0, 5.0), dtype=torch.float32)
    px = torch.tensor(profiles.cpml_tables(nx, fw, h, dt, 3000.0, 5.0), dtype=torch.float32)
    plan = elastic.ElasticPlan(nz, nx, STEPS, ns, 1, nrec, 1, fw, dev.index or 0, snapshot_format="f32")
    lay = plan.layout
    assert lay.kernel_flags == 0 and lay.snapshot_format == _lib.SNAPSHOT_F32, "not the two-launch f32 plan"
    mat_p, pz_d, px_p = elastic._padded_inputs(mat, pz, px, lay.gp)
    dmat_p = pad_columns(dmat, lay.gp)
    f = (profiles.ricker(12.0, STEPS, dt, 0.1)[:, None, None] * torch.ones(1, ns, 1)).to(dev).contiguous()
    sx = torch.linspace(20, nx - 21, ns).long()
    src_cell = (12 * nx + sx).to(torch.int32).reshape(ns, 1, 1).to(dev)
    rx = torch.linspace(12, nx - 13, nrec).long()
    rec_cell = (14 * nx + rx).to(torch.int32).reshape(1, nrec, 1).repeat(ns, 1, 1).contiguous().to(dev)
    src_w, rec_w = torch.ones(ns, 1, 1, device=dev), torch.ones(ns, nrec, 1, device=dev)
    rec = [torch.empty((STEPS, ns, nrec), device=dev) for _ in range(4)]
    work = torch.empty(lay.work_forward_elems, device=dev)
    snap = torch.empty((STEPS, lay.snap_step_elems), device=dev)
    P, st = _lib.ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    geo = (P(src_cell), P(src_w), P(rec_cell), P(rec_w))

    def forward(n):
        _lib.check(lib.mifwi_elastic_forward(plan.handle, P(mat_p), P(pz_d), P(px_p), P(f), *geo, P(rec[0]), P(rec[1]),
                                             P(snap), P(work), 0, n, _lib.ZERO_STATE, st))

    def born(n):
        _lib.check(lib.mifwi_elastic_born(plan.handle, P(mat_p), P(dmat_p), P(pz_d), P(px_p), None, *geo, P(snap), 0,
                                          P(rec[2]), P(rec[3]), P(work), 0, n, _lib.ZERO_STATE, st))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(STEPS)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / STEPS            # us per step

    forward(WARMUP)
    born(WARMUP)
    torch.cuda.synchronize()
    tf, tb = [], []
    for _ in range(REPS):
        tf.append(timed(forward))
        tb.append(timed(born))
    assert bool(torch.isfinite(rec[2]).all()) and float(rec[2].abs().max()) > 0, "the Born traces are empty"
    plan.close()
    mf, mb = statistics.median(tf), statistics.median(tb)
    spread = lambda t: (max(t) - min(t)) / min(t)
    return {"grid": [nz, nx], "shots": ns, "steps": STEPS,
            "forward_save_us_per_step": [round(t, 3) for t in tf], "born_us_per_step": [round(t, 3) for t in tb],
            "forward_median_us": round(mf, 3), "born_median_us": round(mb, 3),
            "forward_spread": round(spread(tf), 4), "born_spread": round(spread(tb), 4),
            "ratio_born_to_forward": round(mb / mf, 4),
            "ratio_exceeds_one_by_more_than_3_forward_spreads": bool(mb / mf - 1.0 > 3.0 * spread(tf))}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/born_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
    dev = torch.device("cuda:0")
    doc = {"how": "device events around %d steps of mifwi_elastic_forward (snapshots written) and mifwi_elastic_born (read), "
                  "two-launch per-step plan, %d alternating repetitions after %d warm-up steps of both" % (STEPS, REPS, WARMUP),
           "device": torch.cuda.get_device_name(dev),
           "cases": [run_case(nz, nx, ns, dev) for nz, nx, ns in CASES]}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_elastic_born.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
