#!/usr/bin/env python3
"""Cost of trace kill and time windows inside the stage-filtered misfit kernels (csrc/mifwi_misfit_select.h).

Workloads: those of tools/stage_filter_rate.py - loss and adjoint source of BOTH components, L2 and global correlation:
  c3     3000 x (32 x 276), dt 2 ms, low-pass 10 Hz
  batch  2500 x (5 x 276),  dt 2 ms, low-pass 10 Hz
  seam   3600 x (4 x 301),  dt 2.5 ms, band-pass 2-12 Hz
Selection: 10 % of the traces killed, a window of a third of the trace around a pick that moves out across the receivers,
Gaussian taper outside (gamma finite).  Three paths, in one process, alternating:
  filtered   misfit.l2_half / global_correlation(pred, obs, sos)                   no selection: what the selected kernel adds to
  selected   the same with select=                                                  one launch per component
  composed   dense [nt, nshot, nrec] weights multiplied around misfit.trace_filter, then the unfiltered kernel, through
             autograd: what a caller writes without select=
Device events around each path, one warm-up, median / min / max of five alternating calls; torch.cuda.max_memory_allocated
of each path above what the inputs hold (the dense weights of the composed form are an input of it and are counted
separately).  "filtered_again" is the first path timed a second time in the same rotation: its ratio to "filtered" is the
spread a ratio between two different paths has to leave to mean anything.

    python tools/trace_selection_rate.py --resources  ->  "kernel_resources" of profiles/r12_trace_selection.json (no GPU needed)
    python tools/trace_selection_rate.py [out.json]   ->  everything else (needs a GPU; keeps "kernel_resources")
"""
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
from physicsbasedfwi2_amd import build, misfit  # noqa: E402

WORKLOADS = [("c3", 3000, 32, 276, 0.002, 0.0, 10.0), ("batch", 2500, 5, 276, 0.002, 0.0, 10.0),
             ("seam", 3600, 4, 301, 0.0025, 2.0, 12.0)]
ORDER = 6
REPS = 5
KILLED = 0.10
GAMMA_PER_S2 = 200.0
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r12_trace_selection.json")
KINDS = {"l2": misfit.l2_half, "gc": misfit.global_correlation}


def kernel_resources():
    """VGPRs, SGPRs, scratch and occupancy of every kernel that applies a trace selection (csrc/mifwi_misfit_select.h), from
    hipcc -Rpass-analysis=kernel-resource-usage.  Scratch must be 0: the section state lives in registers."""
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run([build.HIPCC] + flags + [os.path.join(build.CSRC, "mifwi_misfit.hip")], check=True, text=True,
                          stderr=subprocess.PIPE).stderr
    out = {}
    for block in text.split("Function Name: ")[1:]:
        # misfit_selected_l2 / _gc and misfit_selected_gc_plain: the instances of misfit_staged_l2 / _gc<NSEC, W...> and of
        # misfit_gc<W...> with a selection (W... = mifwi_select::Sel)
        m = re.match(r"_ZN12mifwi_select\d+(trace_window)|_ZN12_GLOBAL__N_1\d+(?:(misfit_selected_l2_plain)|"
                     r"misfit_(gc)IJN12mifwi_select3SelEEEE|misfit_staged_(l2|gc)ILi(\d)EJN12mifwi_select3SelEEEE)", block)
        if not m:
            continue
        name = (m.group(1) or m.group(2) or ("misfit_selected_gc_plain" if m.group(3) else
                                             "misfit_selected_%s<nsec=%s>" % m.group(4, 5)))
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        out[name] = {"vgprs": grab("VGPRs"), "agprs": grab("AGPRs"), "sgprs": grab("TotalSGPRs"),
                     "sgprs_spilled_to_vgpr_lanes": grab("SGPRs Spill"),
                     "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                     "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]"), "lds_bytes_per_block": grab("LDS Size [bytes/block]")}
    if len(out) != 19:
        raise SystemExit("expected the resource report of 19 kernel instances, found %d" % len(out))
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


def selection(nt, ns, nrec, dt):
    rng = np.random.default_rng(nt + ns)
    kill = rng.random((ns, nrec)) < KILLED
    third = nt * dt / 3.0
    picks = 0.1 * nt * dt + 0.5 * nt * dt * np.abs(np.arange(nrec)[None, :] - nrec * (np.arange(ns)[:, None] + 0.5) / ns) / nrec
    return misfit.TraceSelection.from_picks(picks, 0.25 * third, 0.75 * third, dt, gamma_per_s2=GAMMA_PER_S2,
                                            weight=np.where(kill, 0.0, 1.0))


def run_workload(name, nt, ns, nrec, dt, lo, hi, dev):
    gen = torch.Generator(device=dev).manual_seed(nt + ns)
    base = [torch.randn((nt, ns, nrec), device=dev, generator=gen) for _ in range(4)]
    sm = misfit.butterworth_sos(dt, 0.0, 30.0, 4)
    amp = 10.0 ** (2.0 * torch.rand((1, ns, nrec), device=dev, generator=gen) - 1.0)
    preds = [(misfit.trace_filter(b, sm) * amp).contiguous() for b in base[:2]]
    obss = [(0.8 * p + 0.3 * misfit.trace_filter(b, sm) * amp).contiguous() for p, b in zip(preds, base[2:])]
    del base
    sos = misfit.butterworth_sos(dt, lo, hi, ORDER)
    sel = selection(nt, ns, nrec, dt)
    dense = torch.tensor(sel.dense(nt), device=dev, dtype=torch.float32)
    sel._on(dev, (ns, nrec))                                            # the copy to the device is not part of a call
    out = {"nt": nt, "shots": ns, "receivers": nrec, "traces": ns * nrec, "waves": (ns * nrec + 63) // 64, "dt": dt,
           "fc_low": lo, "fc_high": hi, "sections": int(sos.shape[0]), "killed_traces": int((sel.weight == 0).sum()),
           "share_of_samples_with_w_above_1e-3": round(float((dense > 1e-3).float().mean()), 4),
           "dense_weight_bytes": dense.numel() * 4}
    for kind, kernel in KINDS.items():
        res = {}

        def over(loss_of):
            for p, o in zip(preds, obss):
                q = p.detach().requires_grad_(True)
                loss = loss_of(q, o)
                loss.backward()
                res["last"] = (loss.detach(), q.grad)

        paths = {
            "filtered": lambda: over(lambda q, o: kernel(q, o, sos=sos)),
            "selected": lambda: over(lambda q, o: kernel(q, o, sos=sos, select=sel)),
            "composed": lambda: over(lambda q, o: kernel(dense * misfit.trace_filter(q, sos), dense * misfit.trace_filter(o, sos))),
        }
        paths["filtered_again"] = paths["filtered"]
        k_out = {}
        for k, fn in paths.items():                                     # the warm-up doubles as the memory measurement
            res.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
            fn()
            torch.cuda.synchronize()
            k_out[k] = {"peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - held)}
            if k in ("selected", "composed"):
                k_out[k]["_last"] = tuple(t.double() for t in res["last"])
        (ls, gs), (lc, gc) = k_out["selected"].pop("_last"), k_out["composed"].pop("_last")
        k_out["selected_vs_composed_loss_rel_diff"] = float(abs(ls - lc) / abs(lc))
        k_out["selected_vs_composed_adjoint_rel_l2_diff"] = float((gs - gc).norm() / gc.norm())
        res.clear()
        ts = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                ts[k].append(timed(fn))
                res.clear()
        for k in paths:
            k_out[k].update(stats(ts[k]))
        med = lambda k: k_out[k]["median_ms"]
        k_out["selected_over_filtered"] = round(med("selected") / med("filtered"), 3)
        k_out["filtered_again_over_filtered"] = round(med("filtered_again") / med("filtered"), 3)
        k_out["composed_over_selected"] = round(med("composed") / med("selected"), 3)
        k_out["selected_not_slower_than_composed"] = med("selected") <= med("composed")
        out[kind] = k_out
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
            raise SystemExit("tools/trace_selection_rate.py measures on a GPU and none is visible: there is nothing to fall back to")
        dev = torch.device("cuda:0")
        doc.update({"how": "device events around loss + adjoint source of both components, one warm-up, median / min / max of "
                           "%d alternating calls (filtered, selected, composed, filtered again); peak memory: "
                           "torch.cuda.max_memory_allocated above the inputs" % REPS,
                    "selection": "%.0f %% of the traces killed, windows of a third of the trace, gamma %.0f / s^2"
                                 % (100 * KILLED, GAMMA_PER_S2),
                    "device": torch.cuda.get_device_name(dev),
                    "workloads": {w[0]: run_workload(*w, dev) for w in WORKLOADS}})
        doc["selected_not_slower_than_composed_on_all"] = all(w[k]["selected_not_slower_than_composed"]
                                                              for w in doc["workloads"].values() for k in KINDS)
        if "kernel_resources" not in doc:
            doc["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "kernel_resources"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
