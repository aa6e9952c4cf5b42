#!/usr/bin/env python3
"""Cost of source-wavelet estimation (csrc/mifwi_stf.hip): the correlations of the matching filter and the convolution of
the traces with it, next to the composed torch form a caller would otherwise write.

Workloads (traces [nt, nshot, nrec], lags before + after):
  c3     3000 x (32 x 276), lags 0 + 300
  field  2001 x (20 x 300), lags 0 + 86     the field-data record of models/networks.py:10419-10452 (TIME 7.0035 s at DT 3.5 ms;
                                            its shot and receiver counts come from files at run time, 20 x 300 stands in), 0.3 s
Paths, in one process, alternating:
  correlate   misfit.stf_correlations(pred, obs)                                       (a)
  convolve    misfit.trace_convolve(x, h)                                              (b)
  transpose   misfit.trace_convolve(x, h, transpose=True)                              (b), the backward of the former
  composed_correlate   torch.fft: irfft(conj(rfft(pred)) rfft(.)) summed over the receivers, float32
  composed_convolve    torch.nn.functional.conv1d along time on a permuted copy, one group per shot, permuted back
Device events around each path, one warm-up, median / min / max of five alternating calls; torch.cuda.max_memory_allocated
of each path above what the inputs hold.

    python tools/stf_rate.py --resources  ->  "kernel_resources" of profiles/r15_stf.json (no GPU needed)
    python tools/stf_rate.py [out.json]   ->  everything else (needs a GPU; keeps "kernel_resources")
"""
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import build, misfit  # noqa: E402

WORKLOADS = [("c3", 3000, 32, 276, 0, 300), ("field", 2001, 20, 300, 0, 86)]
REPS = 5
PROPAGATOR_MS_C3 = 45.0                    # the propagator time of Denise.grad() on C3
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r15_stf.json")


def kernel_resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the kernels of csrc/mifwi_stf.hip, from
    hipcc -Rpass-analysis=kernel-resource-usage.  Scratch must be 0."""
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, "mifwi_stf.hip")], check=True, text=True,
                          stderr=subprocess.PIPE).stderr
    out = {}
    for block in text.split("Function Name: ")[1:]:
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+(stf_correlate|stf_finish|trace_convolve)(?:ILb(\d)E)?", block)
        if not m:
            continue
        name = m.group(1) if m.group(2) is None else "%s<transpose=%s>" % (m.group(1), m.group(2))
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        out[name] = {"vgprs": grab("VGPRs"), "agprs": grab("AGPRs"), "sgprs": grab("TotalSGPRs"),
                     "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                     "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]"), "lds_bytes_per_block": grab("LDS Size [bytes/block]")}
    if len(out) != 4:
        raise SystemExit("expected the resource report of 4 kernel instances, found %d" % len(out))
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


def composed_correlations(pred, obs, lb, la):
    """a, c [nshot, nlag] through padded spectra, float32."""
    nt = pred.shape[0]
    n = 1 << (nt + lb + la).bit_length()
    xf, df = torch.fft.rfft(pred, n=n, dim=0), torch.fft.rfft(obs, n=n, dim=0)
    a = torch.fft.irfft((xf.conj() * xf).sum(2), n=n, dim=0)[:lb + la + 1]                    # sum_t x[t] x[t + j]
    cc = torch.fft.irfft((xf.conj() * df).sum(2), n=n, dim=0)                                 # sum_t x[t] d[t + k]
    c = torch.cat([cc[n - lb:], cc[:la + 1]]) if lb else cc[:la + 1]
    return a.T.contiguous(), c.T.contiguous()


def composed_convolve(x, h, lb):
    """y = h * x with conv1d on a [nrec, nshot, nt] copy, one group per shot."""
    ns, nlag = h.shape
    xp = torch.nn.functional.pad(x.permute(2, 1, 0), (nlag - 1 - lb, lb))
    return torch.nn.functional.conv1d(xp, h.flip(1)[:, None, :], groups=ns).permute(2, 1, 0).contiguous()


def run_workload(name, nt, ns, nrec, lb, la, dev):
    gen = torch.Generator(device=dev).manual_seed(nt + ns)
    sm = misfit.butterworth_sos(0.002, 0.0, 30.0, 4)
    pred = misfit.trace_filter(torch.randn((nt, ns, nrec), device=dev, generator=gen), sm).contiguous()
    obs = (0.8 * pred + 0.3 * misfit.trace_filter(torch.randn((nt, ns, nrec), device=dev, generator=gen), sm)).contiguous()
    h = (torch.randn((ns, lb + la + 1), device=dev, generator=gen) * torch.exp(-torch.arange(lb + la + 1, device=dev) / 20.0)).contiguous()
    res = {}
    paths = {
        "correlate": lambda: res.__setitem__("corr", misfit.stf_correlations(pred, obs, lb, la)),
        "convolve": lambda: res.__setitem__("conv", misfit.trace_convolve(pred, h, lb)),
        "transpose": lambda: res.__setitem__("convT", misfit.trace_convolve(pred, h, lb, True)),
        "composed_correlate": lambda: res.__setitem__("ccorr", composed_correlations(pred, obs, lb, la)),
        "composed_convolve": lambda: res.__setitem__("cconv", composed_convolve(pred, h, lb)),
    }
    out = {"nt": nt, "shots": ns, "receivers": nrec, "lag_before": lb, "lag_after": la,
           "multiply_adds_correlate": 2 * nt * ns * nrec * (lb + la + 1), "multiply_adds_convolve": nt * ns * nrec * (lb + la + 1),
           "trace_bytes": 4 * nt * ns * nrec}
    for k, fn in paths.items():                                         # the warm-up doubles as the memory measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        out[k] = {"peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - held)}
        held = None
    (a, c), (ca, cc) = res["corr"], res["ccorr"]
    out["composed_vs_kernel_auto_rel_diff"] = float((ca.double() - a).norm() / a.norm())
    out["composed_vs_kernel_cross_rel_diff"] = float((cc.double() - c).norm() / c.norm())
    out["composed_vs_kernel_convolve_rel_diff"] = float((res["cconv"] - res["conv"]).norm() / res["conv"].norm())
    res.clear()
    ts = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ts[k].append(timed(fn))
            res.clear()
    for k in paths:
        out[k].update(stats(ts[k]))
    med = lambda k: out[k]["median_ms"]
    out["gflops_correlate_fp64"] = round(2e-6 * out["multiply_adds_correlate"] / med("correlate"), 1)
    out["gflops_convolve_fp32"] = round(2e-6 * out["multiply_adds_convolve"] / med("convolve"), 1)
    out["estimate_and_apply_ms"] = round(med("correlate") + med("convolve") + med("transpose"), 4)       # (a) + 2 (b)
    out["composed_ms"] = round(med("composed_correlate") + 2 * med("composed_convolve"), 4)
    out["composed_over_kernels"] = round(out["composed_ms"] / out["estimate_and_apply_ms"], 3)
    out["kernels_not_slower_than_composed"] = {"correlate": med("correlate") <= med("composed_correlate"),
                                               "convolve": med("convolve") <= med("composed_convolve")}
    if name == "c3":
        out["share_of_propagator_time"] = round(out["estimate_and_apply_ms"] / PROPAGATOR_MS_C3, 4)
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
            raise SystemExit("tools/stf_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around each path, one warm-up, median / min / max of %d alternating calls; peak "
                           "memory: torch.cuda.max_memory_allocated above the inputs" % REPS,
                    "device": torch.cuda.get_device_name(dev),
                    "propagator_ms_c3": PROPAGATOR_MS_C3,
                    "workloads": {w[0]: run_workload(*w, dev) for w in WORKLOADS}})
        if "kernel_resources" not in doc:
            doc["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "kernel_resources"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
