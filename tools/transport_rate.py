#!/usr/bin/env python3
"""Cost of the optimal-transport objective (csrc/mifwi_transport.hip) next to the envelope objective on the same traces.

Both launches put one workgroup on a trace and keep the trace in LDS, so mifwi_misfit_envelope is the yardstick.
Workloads (traces [nt, nshot x nrec]):
  c3     3000 x (32 x 300)    chunks of 8 samples, 384 threads, 54 KB of LDS per workgroup
  long   8192 x (8 x 1700)    chunks of 16 samples, 512 threads, 136 KB: the largest image
Paths, the C entry points themselves, in one process, alternating:
  transport        mifwi_misfit_transport with adj_out
  transport_loss   mifwi_misfit_transport with adj_out = NULL (ends after the search: no suffix sums, no second reduction)
  envelope         mifwi_misfit_envelope with adj_out
  envelope_loss    mifwi_misfit_envelope with adj_out = NULL
Device events around each call, one warm-up, median / min / max of five alternating calls.

    python tools/transport_rate.py --resources      ->  "kernel_resources" of profiles/r22_transport.json (no GPU needed)
    python tools/transport_rate.py [out.json]       ->  everything else (needs a GPU; keeps "kernel_resources" and
                                                        "measured_errors")
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
from physicsbasedfwi2_amd import _lib, build, misfit  # noqa: E402

WORKLOADS = [("c3", 3000, 32, 300), ("long", 8192, 8, 1700)]
REPS = 5
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r22_transport.json")


def kernel_resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the kernels of csrc/mifwi_transport.hip, from
    hipcc -Rpass-analysis=kernel-resource-usage.  Scratch must be 0.  The LDS figure is the static part: Q and q are
    dynamic, 16 T (C + 1) bytes (T threads, chunks of C samples; C = 1: 16 T)."""
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, "mifwi_transport.hip")], check=True, text=True,
                          stderr=subprocess.PIPE).stderr
    out = {}
    for block in text.split("Function Name: ")[1:]:
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+(tr_misfit|tr_finish)(?:ILi(\d+)E)?", block)
        if not m:
            continue
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        name = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
        out[name] = {"vgprs": grab("VGPRs"), "agprs": grab("AGPRs"), "sgprs": grab("TotalSGPRs"),
                     "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                     "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]"),
                     "static_lds_bytes_per_block": grab("LDS Size [bytes/block]")}
    if len(out) != 6:
        raise SystemExit("expected the resource report of 6 kernels, found %d" % len(out))
    bad = [k for k, v in out.items() if v["scratch_bytes_per_lane"] != 0]
    if bad:
        raise SystemExit("scratch in %s" % bad)
    out["dynamic_lds_bytes"] = {"formula": "16 T (C + 1)", "c3 (T = 384, C = 8)": 16 * 384 * 9, "long (T = 512, C = 16)": 16 * 512 * 17}
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


def run_workload(name, nt, ns, nrec, dev):
    lib = _lib.load()
    ntrace = ns * nrec
    gen = torch.Generator(device=dev).manual_seed(nt + ns)
    sm = misfit.butterworth_sos(0.002, 0.0, 30.0, 4)
    pred = misfit.trace_filter(torch.randn((nt, ntrace), device=dev, generator=gen), sm).contiguous()
    obs = (0.8 * pred + 0.3 * misfit.trace_filter(torch.randn((nt, ntrace), device=dev, generator=gen), sm)).contiguous()
    peak = float(obs.abs().max())
    b, eps = 4.0 / peak, 1e-3 * peak
    adj = torch.empty_like(pred)
    loss = torch.empty((), device=dev)
    work = torch.empty(max(int(lib.mifwi_misfit_transport_work_elems(nt, ntrace)), int(lib.mifwi_misfit_envelope_work_elems(nt, ntrace))),
                       device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(fn, scalar, out):
        return lambda: _lib.check(fn(0, _lib.ptr(pred), _lib.ptr(obs), nt, ntrace, scalar, _lib.ptr(loss), _lib.ptr(out),
                                     _lib.ptr(work), stream))

    paths = {"transport": call(lib.mifwi_misfit_transport, b, adj), "transport_loss": call(lib.mifwi_misfit_transport, b, None),
             "envelope": call(lib.mifwi_misfit_envelope, eps, adj), "envelope_loss": call(lib.mifwi_misfit_envelope, eps, None)}
    out = {"nt": nt, "shots": ns, "receivers": nrec, "trace_bytes": 4 * nt * ntrace}
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
    out["transport_over_envelope"] = round(med("transport") / med("envelope"), 3)
    out["transport_loss_over_envelope_loss"] = round(med("transport_loss") / med("envelope_loss"), 3)
    out["transport_loss_share_of_transport"] = round(med("transport_loss") / med("transport"), 3)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else DEFAULT_OUT
    held = [p for p in (path, DEFAULT_OUT) if os.path.exists(p)]     # what an earlier run left: resources, measured errors
    doc = json.load(open(held[0])) if held else {}
    if "--resources" in sys.argv:
        doc["kernel_resources"] = kernel_resources()
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tools/transport_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around each C entry point, one warm-up, median / min / max of %d alternating calls" % REPS,
                    "device": torch.cuda.get_device_name(dev),
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
