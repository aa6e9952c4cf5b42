#!/usr/bin/env python3
"""Cost of the frequency stage of Denise.grad(): the fused recursive kernels (csrc/mifwi_misfit_filter.h: one launch per
component reads pred and obs and delivers the loss of the filtered traces and the adjoint source through the transposed
filter) against the frequency-domain form they replace (compat.pyapi_denise.butterworth on spectra padded to four times the
trace length, once for pred, once for obs, once more through autograd, followed by the unfiltered misfit kernel).

Workloads - loss and adjoint source of BOTH components, L2:
  c3     3000 x (32 x 276), dt 2 ms, low-pass 10 Hz        the elastic bench workload (networks.py:7761 stage)
  batch  2500 x (5 x 276),  dt 2 ms, low-pass 10 Hz        what networks.py:7650 runs per step
  seam   3600 x (4 x 301),  dt 2.5 ms, band-pass 2-12 Hz   SEAM, networks.py:9863
Device events around each path, one warm-up, median / min / max of five alternating calls; torch.cuda.max_memory_allocated
of each path above what the inputs hold.  Then one whole Denise.grad() call on the C3 grid (100 x 300, 32 shots, 3000 steps)
with MIFWI_STAGE_FILTER=fft and =recursive: what share of the call the stage is.

    python tools/stage_filter_rate.py --resources   ->  "kernel_resources" of profiles/r11_stage_filter.json (no GPU needed)
    python tools/stage_filter_rate.py [out.json]    ->  everything else (needs a GPU; keeps "kernel_resources")
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import build, misfit  # noqa: E402

WORKLOADS = [("c3", 3000, 32, 276, 0.002, 0.0, 10.0), ("batch", 2500, 5, 276, 0.002, 0.0, 10.0),
             ("seam", 3600, 4, 301, 0.0025, 2.0, 12.0)]
ORDER = 6
REPS = 5
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r11_stage_filter.json")


def kernel_resources():
    """VGPRs, SGPRs, scratch and occupancy of every instance of the stage-filter kernels, from
    hipcc -Rpass-analysis=kernel-resource-usage.  Scratch must be 0: the section state lives in registers."""
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, "mifwi_misfit.hip")], check=True, text=True,
                          stderr=subprocess.PIPE).stderr
    out = {}
    for block in text.split("Function Name: ")[1:]:
        # misfit_filtered_l2 / _gc: the instances of misfit_staged_l2 / _gc<NSEC, W...> without a selection (W... empty)
        m = re.match(r"_ZN12mifwi_filter\d+(trace_filter)ILi(\d)ELb([01])E|_ZN12_GLOBAL__N_1\d+misfit_staged_(l2|gc)ILi(\d)EJEEE", block)
        if not m:
            continue
        name = ("trace_filter<nsec=%s, transpose=%s>" % m.group(2, 3) if m.group(1) else
                "misfit_filtered_%s<nsec=%s>" % m.group(4, 5))
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        out[name] = {"vgprs": grab("VGPRs"), "sgprs": grab("TotalSGPRs"), "sgprs_spilled_to_vgpr_lanes": grab("SGPRs Spill"),
                     "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                     "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]")}
    if len(out) != 32:
        raise SystemExit("expected the resource report of 32 kernel instances, found %d" % len(out))
    bad = [k for k, v in out.items() if v["scratch_bytes_per_lane"] != 0]
    if bad:
        raise SystemExit("scratch in %s" % bad)
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


def run_workload(name, nt, ns, nrec, dt, lo, hi, dev):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    gen = torch.Generator(device=dev).manual_seed(nt + ns)
    # band-limited traces with a per-trace amplitude, two components
    base = [torch.randn((nt, ns, nrec), device=dev, generator=gen) for _ in range(4)]
    sm = misfit.butterworth_sos(dt, 0.0, 30.0, 4)
    amp = 10.0 ** (2.0 * torch.rand((1, ns, nrec), device=dev, generator=gen) - 1.0)
    preds = [(misfit.trace_filter(b, sm) * amp).contiguous() for b in base[:2]]
    obss = [(0.8 * p + 0.3 * misfit.trace_filter(b, sm) * amp).contiguous() for p, b in zip(preds, base[2:])]
    del base
    sos = misfit.butterworth_sos(dt, lo, hi, ORDER)
    res = {}

    def fused():
        for p, o in zip(preds, obss):
            q = p.detach().requires_grad_(True)
            loss = misfit.l2_half(q, o, sos=sos)
            loss.backward()
            res["fused"] = (loss.detach(), q.grad)

    def fft():
        for p, o in zip(preds, obss):
            q = p.detach().requires_grad_(True)
            loss = misfit.l2_half(api.butterworth(q, dt, lo, hi, ORDER), api.butterworth(o, dt, lo, hi, ORDER))
            loss.backward()
            res["fft"] = (loss.detach(), q.grad)

    paths = {"fused": fused, "fft": fft}
    out = {"nt": nt, "shots": ns, "receivers": nrec, "traces": ns * nrec, "waves": (ns * nrec + 63) // 64, "dt": dt,
           "fc_low": lo, "fc_high": hi, "sections": int(sos.shape[0])}
    for k, fn in paths.items():                                         # the warm-up doubles as the memory measurement
        res.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        out[k] = {"peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - held)}
    fused(); fft()
    lf, gf = res["fused"]
    lq, gq = res["fft"]
    out["last_component_loss_rel_diff"] = float(abs(lf.double() - lq.double()) / lq.double())
    out["last_component_adjoint_rel_l2_diff"] = float((gf.double() - gq.double()).norm() / gq.double().norm())
    res.clear()
    ts = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ts[k].append(timed(fn))
            res.clear()
    for k in paths:
        out[k].update(stats(ts[k]))
    out["fft_over_fused"] = round(out["fft"]["median_ms"] / out["fused"]["median_ms"], 3)
    out["fused_not_slower"] = out["fused"]["median_ms"] <= out["fft"]["median_ms"]
    return out


def denise_grad_c3(dev):
    """One whole Denise.grad() on the C3 grid with the stage of networks.py:7761, both settings of MIFWI_STAGE_FILTER and
    without a stage: host clock around the call (it ends with the gradients on the host)."""
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    nz, nx, h, ns, nrec = 100, 300, 20.0, 32, 276
    rng = np.random.default_rng(0)
    z = np.linspace(0.0, 1.0, nz)[:, None]
    vp = (1500.0 + 2500.0 * z + 50.0 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3.0)).astype(np.float32)
    rho = (1800.0 + 600.0 * z + 0.0 * vp).astype(np.float32)
    src = api.Sources(np.linspace(400.0, 5600.0, ns), np.full(ns, 40.0), 5.0)
    rec = api.Receivers(240.0 + h * np.arange(nrec), np.full(nrec, 460.0))
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), h)
    true = api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), h)

    def make(stage):
        d = api.Denise(None, 0)
        d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 6.0, 0.002, 1, 10, 5.0, 1500.0
        if stage:
            d.add_fwi_stage(fc_high=10, inv_rho_iter=10000)
        return d
    d0 = make(False)
    ox, oy = d0.forward(true, src, rec)
    obs = (np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    ways = {"no_stage": (False, None), "fft": (True, "fft"), "recursive": (True, "recursive")}
    ds = {}
    for k, (stage, mode) in ways.items():
        ds[k] = make(stage)
        ds[k].set_observed(*obs)
    old = os.environ.get("MIFWI_STAGE_FILTER")
    ts = {k: [] for k in ways}
    out = {}
    cwd = os.getcwd()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                                             # grad() writes loss_curve_grad.out where it stands
        try:
            for rep in range(4):                                  # the first round is the warm-up
                for k, (stage, mode) in ways.items():
                    os.environ.pop("MIFWI_STAGE_FILTER", None)
                    if mode:
                        os.environ["MIFWI_STAGE_FILTER"] = mode
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loss = ds[k].grad(model, src, rec)
                    torch.cuda.synchronize()
                    if rep:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
                    out.setdefault(k, {})["loss"] = loss
        finally:
            os.chdir(cwd)
            os.environ.pop("MIFWI_STAGE_FILTER", None)
            if old is not None:
                os.environ["MIFWI_STAGE_FILTER"] = old
    for k in ways:
        out[k].update(stats(ts[k]))
    base = out["no_stage"]["median_ms"]
    for k in ("fft", "recursive"):
        out[k]["stage_ms"] = round(out[k]["median_ms"] - base, 4)
        out[k]["stage_share_of_call"] = round((out[k]["median_ms"] - base) / out[k]["median_ms"], 4)
    out["how"] = ("host clock around Denise.grad() (forward, stage + L2, adjoint, chain rule, gradients to the host), one "
                  "warm-up, median / min / max of three alternating calls; stage = call with the stage minus call without")
    out["grid"] = [nz, nx]
    out["shots"], out["receivers"], out["steps"] = ns, nrec, 3000
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
            raise SystemExit("tools/stage_filter_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around loss + adjoint source of both components, one warm-up, median / min / max "
                           "of %d alternating calls; peak memory: torch.cuda.max_memory_allocated above the inputs" % REPS,
                    "device": torch.cuda.get_device_name(dev),
                    "workloads": {w[0]: run_workload(*w, dev) for w in WORKLOADS}})
        doc["fused_not_slower_on_all"] = all(w["fused_not_slower"] for w in doc["workloads"].values())
        doc["denise_grad_c3"] = denise_grad_c3(dev)
        if "kernel_resources" not in doc:
            doc["kernel_resources"] = kernel_resources()
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "kernel_resources"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
