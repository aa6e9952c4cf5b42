#!/usr/bin/env python3
"""Instruction mix of the time loop of the elastic single-launch kernels, from the compiler's assembly (no GPU needed):

    python tools/loop_mix.py                      the two headline instances (forward SAVE NG=2 XH, adjoint NG=2 XH)
    python tools/loop_mix.py 'el_cluster_adj<1'   instances whose demangled name contains the string
    python tools/loop_mix.py --blocks ...         one row per basic block as well
    python tools/loop_mix.py --asm FILE ...       read an assembly file instead of compiling

mifwi_elastic.hip is compiled device-only with build.FLAGS.  The time loop of a kernel is the depth-1 loop with the
most instructions (the compiler's own "in Loop: Header=" annotations).  Per block and in total: vector instructions by
class, scalar instructions, LDS and global operations, s_nop; per kernel NumVgprs, SGPR spills and ScratchSize; for all
el_cluster instances a one-line resource summary (the budget check: NumVgprs <= 256, no scratch, spills not grown).

tools/loop_mix_blocks.json says which blocks of the loop a wave of the headline shape (100x300, 8 slabs, 32 shots)
executes and how often per step: `weights` maps a block label, or a range "first..last" in layout order, to the
fraction of the workgroup's 8 waves that run it (0: not executed - slow source and receiver paths, the other publish
scope, free-surface branches, time-out handling); unlisted blocks count once.  The tables are keyed by the fingerprint
of the kernel sources, so one for the parent and one for the current kernels can sit side by side; without a table
for the sources at hand only the static counts are printed.  The weighted sum is the `executed vector instructions per
wave-step` figure, to be set against SQ_INSTS_VALU per wave-step of tools/issue_counters.py.
"""
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicsbasedfwi2_amd import build  # noqa: E402

CSRC = os.path.join(ROOT, "physicsbasedfwi2_amd", "csrc")
SRC = os.path.join(CSRC, "mifwi_elastic.hip")
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_mix_blocks.json")
HEADLINE = ["el_cluster_fwd<true, 2, false, true>", "el_cluster_adj<2, false, true>"]
VCLASSES = ["farith", "v_mov", "dpp", "cndmask", "cmp", "int/addr", "lane"]
COLS = VCLASSES + ["valu", "salu", "s_nop", "lds", "global"]


def fingerprint():
    """sha1 over the sources the time loops are compiled from"""
    h = hashlib.sha1()
    for f in ("mifwi_elastic.hip", "mifwi_elastic_cluster.h", "mifwi_stagger.h", "mifwi_common.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:12]


def classify(line):
    """column of one instruction line (None for directives)"""
    m = re.match(r"^\s+([a-z][a-z0-9_]+)", line)
    if not m:
        return None
    op = m.group(1)
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if not op.startswith("v_"):
        return None
    if re.match(r"v_(readlane|writelane|readfirstlane)", op):
        return "lane"
    if "_dpp" in op or re.search(r"\b(row_|wave_sh|wave_ro|quad_perm|row_bcast)", line):
        return "dpp"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith("v_cmp"):
        return "cmp"
    if re.match(r"v_(pk_)?mov_|v_accvgpr_", op):
        return "v_mov"
    if re.search(r"_f(16|32|64)$", op) and not op.startswith("v_cvt"):
        return "farith"
    return "int/addr"


def kernels(asm):
    """{mangled name: {"lines": [...], "meta": {NumVgprs, ScratchSize, ...}}} for the functions of an assembly file"""
    out, name = collections.OrderedDict(), None
    for line in asm:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = {"lines": [], "meta": {}}
            continue
        if name is None:
            continue
        m = re.match(r"^; (NumVgprs|NumSgprs|ScratchSize|Occupancy): (\d+)", line)
        if m:
            out[name]["meta"][m.group(1)] = int(m.group(2))
        if line.startswith(".Lfunc_end"):
            out[name]["done"] = True                 # the resource comments of the function follow its end label
        if not out[name].get("done"):
            out[name]["lines"].append(line)
    return out


def metadata_spills(asm):
    """{mangled name: (sgpr_spill_count, vgpr_spill_count)} from the code-object metadata at the end of the file"""
    res, name, cur = {}, None, {}
    for line in asm:
        m = re.match(r"^\s+\.name:\s+(_Z\w+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"^\s+\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", line)
        if m:
            cur[m.group(1)] = int(m.group(2))
        if name and len(cur) == 2:
            res[name] = (cur["sgpr_spill_count"], cur["vgpr_spill_count"])
            name, cur = None, {}
    return res


def blocks(lines):
    """[[label, loop header or None, parent header or None, Counter, branch target]] in layout order.  A label opens a
    block and so does the instruction behind a branch: the fall-through part of `.LBB0_7` is `.LBB0_7+1`."""
    res = [["entry", None, None, collections.Counter(), ""]]
    sub = 0
    for line in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", line)
        if m:
            rest = m.group(2)
            hdr = re.search(r"in Loop: Header=(BB\d+_\d+)", rest)
            par = re.search(r"Parent Loop (BB\d+_\d+)", rest)
            own = "Loop Header" in rest or "Parent Loop" in rest
            res.append([m.group(1), "." + "L" + hdr.group(1) if hdr else (m.group(1) if own else None),
                        ".L" + par.group(1) if par else None, collections.Counter(), ""])
            sub = 0
            continue
        # continuation lines of a nested header's annotation ("Parent Loop ...") follow the label
        par = re.match(r"^\s+;\s+Parent Loop (BB\d+_\d+)", line)
        if par and res[-1][2] is None:
            res[-1][2] = ".L" + par.group(1)
            continue
        c = classify(line)
        if c and res[-1][4]:                               # first instruction behind a branch
            sub += 1
            last = res[-1]
            res.append([last[0].split("+")[0] + "+%d" % sub, last[1] if last[1] != last[0] else last[0].split("+")[0],
                        last[2], collections.Counter(), ""])
        br = re.match(r"^\s+(s_cbranch_\w+|s_branch)\s+(\S+)", line)
        if br:
            res[-1][4] = br.group(1).replace("s_cbranch_", "").replace("s_branch", "always") + " " + br.group(2)
        if c:
            res[-1][3][c] += 1
            if c in VCLASSES:
                res[-1][3]["valu"] += 1
    return res


def time_loop(bl):
    """blocks of the depth-1 loop with the most instructions (inner loops included)"""
    parent = {}
    for label, hdr, par, _, _ in bl:
        if hdr == label and par:
            parent[label] = par

    def top(h):
        while h in parent:
            h = parent[h]
        return h
    size = collections.Counter()
    for label, hdr, par, cnt, _ in bl:
        if hdr:
            size[top(hdr)] += sum(cnt[c] for c in ("valu", "salu", "lds", "global"))
    if not size:
        return None, []
    head = size.most_common(1)[0][0]
    return head, [b for b in bl if b[1] and top(b[1]) == head]


def weight_map(loop, spec):
    """label -> weight from {"label" | "first..last": weight}; later entries override earlier ones"""
    order = [b[0] for b in loop]
    w = {lab: 1.0 for lab in order}
    for key, val in spec.items():
        if ".." in key:
            a, b = key.split("..")
            b = b if b.startswith(".") else "." + b
            ia, ib = order.index(a), order.index(b)
            for lab in order[ia:ib + 1]:
                w[lab] = float(val)
        else:
            if key not in w:
                raise SystemExit("block table names %s, which is not in the loop" % key)
            w[key] = float(val)
    return w


def row(name, cnt, extra=""):
    return "%-16s" % name + "".join("%9s" % (("%.0f" % cnt[c]) if cnt[c] == int(cnt[c]) else "%.1f" % cnt[c])
                                    for c in COLS) + extra


def main(argv):
    show_blocks = "--blocks" in argv
    asm_file = None
    if "--asm" in argv:
        asm_file = argv[argv.index("--asm") + 1]
        argv = [a for a in argv if a != asm_file]
    filt = [a for a in argv if not a.startswith("--")] or HEADLINE
    if asm_file is None:
        flags = [f for f in build.FLAGS if f != "-shared"]
        tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
        tmp.close()
        asm_file = tmp.name
        subprocess.run([build.HIPCC] + flags + ["--cuda-device-only", "-S", "-o", asm_file, SRC], check=True,
                       capture_output=True)
    asm = open(asm_file).read().splitlines()
    if "--asm" not in argv:
        os.unlink(asm_file)
    ks = kernels(asm)
    spills = metadata_spills(asm)
    names = list(ks)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    short = {n: re.sub(r"\(anonymous namespace\)::|void |\(.*", "", d) for n, d in zip(names, dem)}
    fp = fingerprint()
    table = json.load(open(TABLE)).get(fp, {}) if os.path.exists(TABLE) else {}
    print("kernel sources %s%s" % (fp, "" if table else "  (no block table for these sources: static counts only)"))
    print()
    print("resources of the single-launch instances")
    print("%-44s %8s %8s %11s %11s" % ("instance", "NumVgprs", "Scratch", "sgpr_spill", "vgpr_spill"))
    for n in names:
        if "el_cluster" not in short[n]:
            continue
        m = ks[n]["meta"]
        sp = spills.get(n, (-1, -1))
        print("%-44s %8d %8d %11d %11d" % (short[n], m.get("NumVgprs", -1), m.get("ScratchSize", -1), sp[0], sp[1]))
    for n in names:
        if not any(f in short[n] for f in filt):
            continue
        bl = blocks(ks[n]["lines"])
        head, loop = time_loop(bl)
        print()
        print("%s: time loop %s, %d blocks" % (short[n], head, len(loop)))
        print(" " * 16 + "".join("%9s" % c for c in COLS))
        spec = table.get(short[n])
        w = weight_map(loop, spec["weights"]) if spec else None
        tot, exe = collections.Counter(), collections.Counter()
        for label, _, _, cnt, br in loop:
            for c in COLS:
                tot[c] += cnt[c]
                if w:
                    exe[c] += w[label] * cnt[c]
            if show_blocks:
                print(row(label, cnt, ("   x%-6.3g" % w[label] if w else "   ") + br))
        print(row("loop body", tot))
        if w:
            print(row("executed", exe))
            print("executed vector instructions per wave-step: %.0f   (v_readlane/v_writelane %.0f + s_nop %.0f)"
                  % (exe["valu"], exe["lane"], exe["s_nop"]))


if __name__ == "__main__":
    main(sys.argv[1:])
