#!/usr/bin/env python3
"""Cost of the envelope objective (csrc/mifwi_envelope.hip) next to the L2 objective on the same traces.

Workloads (traces [nt, nshot, nrec]):
  c3     3000 x (32 x 276)    N = 4096
  c5     5000 x (16 x 301)    N = 8192, the largest LDS image
Paths, in one process, alternating; each is the objective and its backward into ``pred`` (loss.backward()):
  envelope        misfit.envelope(pred, obs, eps=e)               one launch (+ the partial sum)
  envelope_sos    misfit.envelope(pred, obs, sos=sos, eps=e)      composed: trace_filter on both sides, the launch, F^T back
  l2              misfit.l2_half(pred, obs)
  l2_sos          misfit.l2_half(pred, obs, sos=sos)              fused with the stage filter in one launch
  hilbert         misfit.trace_hilbert(pred)                      H alone, no backward
sos: the 6th-order 10 Hz low-pass of a frequency stage at dt = 2 ms.  The composition reads and writes the traces two
more times each way than a fused form would (F pred and F obs out and in again forward, the adjoint source out and in
again backward): "composition_extra_ms" = envelope_sos - envelope is what that costs.
Device events around each path, one warm-up, median / min / max of five alternating calls.

    python tools/envelope_rate.py --resources                 ->  "kernel_resources" of profiles/r21_envelope.json (no GPU needed)
    python tools/envelope_rate.py [out.json] [--bench-ms=X]   ->  everything else (needs a GPU; keeps "kernel_resources" and
                                                                  "measured_errors"); X: bench.py's ms_per_step of the same
                                                                  visit, for the share of one gradient pass
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

WORKLOADS = [("c3", 3000, 32, 276), ("c5", 5000, 16, 301)]
REPS = 5
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r21_envelope.json")


def kernel_resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the kernels of csrc/mifwi_envelope.hip, from
    hipcc -Rpass-analysis=kernel-resource-usage.  Scratch must be 0.  The LDS figure is the static part: the traces and
    twiddles are dynamic, 16 N bytes (N = the padded length)."""
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, "mifwi_envelope.hip")], check=True, text=True,
                          stderr=subprocess.PIPE).stderr
    out = {}
    for block in text.split("Function Name: ")[1:]:
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+(env_trace_hilbert|env_misfit|env_finish)", block)
        if not m:
            continue
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        out[m.group(1)] = {"vgprs": grab("VGPRs"), "agprs": grab("AGPRs"), "sgprs": grab("TotalSGPRs"),
                           "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                           "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]"),
                           "static_lds_bytes_per_block": grab("LDS Size [bytes/block]")}
    if len(out) != 3:
        raise SystemExit("expected the resource report of 3 kernels, found %d" % len(out))
    bad = [k for k, v in out.items() if v["scratch_bytes_per_lane"] != 0]
    if bad:
        raise SystemExit("scratch in %s" % bad)
    out["dynamic_lds_bytes"] = {"formula": "16 N", "c3 (N = 4096)": 16 * 4096, "c5 (N = 8192)": 16 * 8192}
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


def run_workload(name, nt, ns, nrec, dev, bench_ms):
    gen = torch.Generator(device=dev).manual_seed(nt + ns)
    shape = torch.randn((nt, ns, nrec), device=dev, generator=gen)
    sm = misfit.butterworth_sos(0.002, 0.0, 30.0, 4)
    pred = misfit.trace_filter(shape, sm).contiguous()
    obs = (0.8 * pred + 0.3 * misfit.trace_filter(torch.randn((nt, ns, nrec), device=dev, generator=gen), sm)).contiguous()
    del shape
    sos = misfit.butterworth_sos(0.002, 0.0, 10.0, 6)
    eps = 1e-3 * float(obs.abs().max())
    pred.requires_grad_(True)

    def grad_of(objective):
        def fn():
            pred.grad = None
            objective().backward()
        return fn

    paths = {
        "envelope": grad_of(lambda: misfit.envelope(pred, obs, eps=eps)),
        "envelope_sos": grad_of(lambda: misfit.envelope(pred, obs, sos=sos, eps=eps)),
        "l2": grad_of(lambda: misfit.l2_half(pred, obs)),
        "l2_sos": grad_of(lambda: misfit.l2_half(pred, obs, sos=sos)),
        "hilbert": lambda: misfit.trace_hilbert(pred.detach()),
    }
    n = 1 << (nt - 1).bit_length()
    out = {"nt": nt, "shots": ns, "receivers": nrec, "padded_length": n, "trace_bytes": 4 * nt * ns * nrec,
           "dynamic_lds_bytes_per_workgroup": 16 * n}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ts[k].append(timed(fn))
    for k in paths:
        out[k] = stats(ts[k])
    med = lambda k: out[k]["median_ms"]
    out["envelope_over_l2"] = round(med("envelope") / med("l2"), 3)
    out["envelope_sos_over_l2_sos"] = round(med("envelope_sos") / med("l2_sos"), 3)
    out["composition_extra_ms"] = round(med("envelope_sos") - med("envelope"), 4)
    if bench_ms:
        out["share_of_bench_gradient_pass"] = {"envelope": round(med("envelope") / bench_ms, 4),
                                               "envelope_sos": round(med("envelope_sos") / bench_ms, 4)}
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bench = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--bench-ms=")]
    bench_ms = float(bench[0]) if bench else None
    path = args[0] if args else DEFAULT_OUT
    held = [p for p in (path, DEFAULT_OUT) if os.path.exists(p)]     # what an earlier run left: resources, measured errors
    doc = json.load(open(held[0])) if held else {}
    if "--resources" in sys.argv:
        doc["kernel_resources"] = kernel_resources()
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tools/envelope_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around each path (objective + backward into pred), one warm-up, median / min / max of "
                           "%d alternating calls" % REPS,
                    "device": torch.cuda.get_device_name(dev),
                    "bench_ms_per_gradient_pass": bench_ms,
                    "workloads": {w[0]: run_workload(*w, dev, bench_ms) for w in WORKLOADS}})
        if "kernel_resources" not in doc:
            doc["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "kernel_resources"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
