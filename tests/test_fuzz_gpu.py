"""Seeded sweep over small random configurations of the elastic path (grid sizes off the tile sizes, C-PML width,
free surface, source type, pressure receivers, shots per accumulator group, forced shot passes, both kernel
families): seismograms and every gradient against oracle/elastic.c."""
import os

import numpy as np
import pytest
import torch

from cases import acoustic_case, elastic_case, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _configs():
    rng = np.random.default_rng(2026)
    out = []
    for k in range(14):
        fs = bool(rng.integers(0, 2))
        cfg = dict(nz=int(rng.integers(34, 75)), nx=int(rng.integers(40, 140)), fw=int(rng.choice([0, 5, 8])),
                   ns=int(rng.integers(1, 6)), nsrc=int(rng.integers(1, 3)), nrec=int(rng.integers(1, 20)),
                   nt=int(rng.integers(20, 70)), free_surface=fs, water=int(rng.choice([0, 6])))
        opt = dict(source_type=int(rng.integers(0, 3)), pressure=bool(rng.integers(0, 2)),
                   gs=int(rng.integers(0, 4)), cluster=str(int(rng.integers(0, 2))),
                   pass_shots=str(int(rng.integers(1, 4))), pass_groups=str(int(rng.integers(1, 3))))
        # round 4 (drawn from a generator of their own: the configurations above stay the ones of rounds 1-3): plane
        # layout, tile -> XCD order, fused forward, snapshot format
        r4 = np.random.default_rng(4000 + k)
        r4.choice([0, 1, 2, 2]), r4.choice([14, 28, 42, 70])   # options of removed adjoint forms: drawn, keep the sequence
        opt.update(blocked=str(int(r4.integers(0, 2))), xcd=str(int(r4.choice([0, 1, 2, 3]))), fused=str(int(r4.integers(0, 2))),
                   fmt=str(r4.choice(["f32", "f32", "bf16"])))
        out.append((k, cfg, opt))
    return out


@pytest.mark.parametrize("k,cfg,opt", _configs())
def test_random_elastic_configuration(oracle32, monkeypatch, k, cfg, opt):
    from physicsbasedfwi2_amd import elastic
    monkeypatch.setenv("MIFWI_EL_CLUSTER", opt["cluster"])
    monkeypatch.setenv("MIFWI_EL_CLUSTER_ADJ", opt["cluster"])
    monkeypatch.setenv("MIFWI_EL_PASS_SHOTS", opt["pass_shots"])
    monkeypatch.setenv("MIFWI_EL_PASS_GROUPS", opt["pass_groups"])
    monkeypatch.setenv("MIFWI_EL_SNAP_BLOCKED", opt["blocked"])
    monkeypatch.setenv("MIFWI_EL_XCD", opt["xcd"])
    monkeypatch.setenv("MIFWI_EL_FUSED", opt["fused"])
    bf16 = opt["fmt"] == "bf16"
    case = elastic_case(seed=100 + k, **cfg)
    if opt["source_type"]:
        case["f"] = (case["f"] * 1e-3).astype(np.float32)
    o, fs, st = oracle32, case["fs"], opt["source_type"]
    geo = (case["sc"], case["sw"], case["rc"], case["rw"])
    res = o.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], *geo, save=True, free_surface=fs,
                            source_type=st, pressure=opt["pressure"])
    ovx, ovz, S = res[:3]
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=DEV, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=DEV, requires_grad=True)
    tg = [torch.tensor(case[n]) for n in ("pz", "px", "sc", "sw", "rc", "rw")]
    out = elastic.propagate(mat, f, *tg, case["fw"], shots_per_group=opt["gs"], free_surface=bool(fs),
                            source_type=st, record_pressure=opt["pressure"], snapshot_format=opt["fmt"])
    scale = max(np.abs(ovx).max(), np.abs(ovz).max())
    assert scale > 0
    for h, r in zip(out, res[:2] + ((res[3],) if opt["pressure"] else ())):
        assert np.abs(h.detach().cpu().numpy() - r).max() <= 2e-5 * max(scale, np.abs(r).max())
    rng = np.random.default_rng(k)
    gs_ = [(rng.standard_normal(r.shape) * scale).astype(np.float32) for r in (ovx, ovz)]
    gp = (rng.standard_normal(ovx.shape) * scale).astype(np.float32) if opt["pressure"] else None
    torch.autograd.backward(list(out), [torch.tensor(g, device=DEV) for g in gs_ + ([gp] if gp is not None else [])])
    gm_o, gf_o = o.elastic_backward(case["mat"], case["pz"], case["px"], *geo, gs_[0], gs_[1], S, free_surface=fs,
                                    source_type=st, g_p=gp)
    # bf16 snapshot planes (per-step kernels only; a single-launch plan keeps f32): the stated 4e-3 on the material gradients
    tol = 4e-3 if bf16 and opt["cluster"] == "0" else 5e-5
    for j in range(5):
        assert rel_l2(mat.grad[j].cpu().numpy(), gm_o[j]) <= tol, (j, cfg, opt)
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= 5e-5, (cfg, opt)


def _acoustic_configs():
    rng = np.random.default_rng(2027)
    out = []
    for k in range(12):
        cfg = dict(n0=int(rng.integers(30, 90)), n1=int(rng.integers(36, 150)), nb=int(rng.choice([4, 8, 12])),
                   ns=int(rng.integers(1, 7)), nsrc=int(rng.integers(1, 3)), nrec=int(rng.integers(1, 25)),
                   nt=int(rng.integers(20, 80)), ntap=int(rng.choice([1, 1, 4])),
                   h=(10.0, float(rng.choice([10.0, 12.5]))))
        opt = dict(gs=int(rng.integers(0, 4)), cluster=str(int(rng.integers(0, 2))),
                   groups=str(int(rng.integers(1, 3))), nw=str(int(rng.choice([0, 0, 2, 3]))))
        out.append((k, cfg, opt))
    return out


@pytest.mark.parametrize("k,cfg,opt", _acoustic_configs())
def test_random_acoustic_configuration(oracle32, monkeypatch, k, cfg, opt):
    from physicsbasedfwi2_amd import acoustic
    monkeypatch.setenv("MIFWI_AC_CLUSTER", opt["cluster"])
    monkeypatch.setenv("MIFWI_AC_PASS_GROUPS", opt["groups"])
    if opt["nw"] != "0":
        monkeypatch.setenv("MIFWI_AC_NW", opt["nw"])
    case = acoustic_case(seed=200 + k, **cfg)
    o = oracle32
    geo = (case["sc"], case["sw"], case["rc"], case["rw"])
    rec_o, G = o.acoustic_forward(case["r"], case["q0"], case["q1"], case["f"], *geo, case["c0"], case["c1"], save=True)
    r = torch.tensor(case["r"], dtype=torch.float32, device=DEV, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=DEV, requires_grad=True)
    rec = acoustic.propagate(r, f, torch.tensor(case["q0"]), torch.tensor(case["q1"]),
                             *[torch.tensor(a) for a in geo], case["c0"], case["c1"], shots_per_group=opt["gs"])
    scale = np.abs(rec_o).max()
    assert scale > 0 and np.abs(rec.detach().cpu().numpy() - rec_o).max() <= 2e-5 * scale
    g = (np.random.default_rng(k).standard_normal(rec_o.shape) * scale).astype(np.float32)
    rec.backward(torch.tensor(g, device=DEV))
    gr_o, gf_o = o.acoustic_backward(case["r"], case["q0"], case["q1"], *geo, g, G, case["c0"], case["c1"])
    assert rel_l2(r.grad.cpu().numpy(), gr_o) <= 5e-5, (cfg, opt)
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= 5e-5, (cfg, opt)


# A generator of its own for the fluid draws.  The seed was chosen on the CPU: the first from 2031 on whose 16 draws cover
# what test_fluid_draws_cover_the_tile_widths_and_column_remainders asks for and all keep the f32 oracle's gL + gM within
# 5e-6 of the f64 oracle's (the largest is 3.3e-6) with no compared quantity all zero.
FLUID_SEED = 2037


def _pick_lx(ng):
    """The plan's rule for the forward tile width (mifwi::pick_lx in csrc/mifwi_host.h), restated: 64 lanes per row, then
    32, where padding a row of ng four-cell groups to a multiple of that costs at most 20 %; otherwise 16."""
    for cand in (64, 32):
        if -(-ng // cand) * cand * 10 <= ng * 12:
            return cand
    return 16


def _fluid_configs(seed=FLUID_SEED):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(16):
        fw = int(rng.choice([0, 3, 6, 9]))
        cfg = dict(nz=int(rng.integers(max(24, 2 * fw + 4), 75)), nx=int(rng.integers(40, 260)), fw=fw,
                   ns=int(rng.integers(1, 6)), nsrc=int(rng.integers(1, 3)), nrec=int(rng.integers(1, 20)),
                   nt=int(rng.integers(60, 120)), free_surface=bool(rng.integers(0, 2)))
        # segments 0: the default snapshot budget (resident snapshots); 3 or 4: a budget that holds that share of the steps
        opt = dict(source_type=int(rng.integers(0, 3)), order=int(rng.choice([2, 4])), pressure=bool(rng.integers(0, 2)),
                   gs=int(rng.integers(0, 4)), pass_shots=str(int(rng.integers(1, 4))),
                   pass_groups=str(int(rng.integers(1, 3))), segments=int(rng.choice([0, 0, 3, 4])))
        out.append((k, cfg, opt))
    return out


def _fluid_case(k, cfg):
    from cases import fluid_planes, fluid_sources_off_the_surface
    c = elastic_case(seed=400 + k, water=0, **cfg)
    if cfg["free_surface"]:
        fluid_sources_off_the_surface(c)
    return fluid_planes(c, c["fs"])


def test_fluid_draws_cover_the_tile_widths_and_column_remainders():
    """Needs no GPU.  Over the 16 draws: every forward tile width at least twice, every nx % 4, every source type with and
    without a free surface."""
    draws = _fluid_configs()
    widths = [_pick_lx(-(-cfg["nx"] // 4)) for _, cfg, _ in draws]
    assert all(widths.count(lx) >= 2 for lx in (16, 32, 64)), widths
    assert {cfg["nx"] % 4 for _, cfg, _ in draws} == {0, 1, 2, 3}
    assert {(opt["source_type"], cfg["free_surface"]) for _, cfg, opt in draws} == {(st, fs) for st in range(3)
                                                                                    for fs in (False, True)}


@pytest.mark.parametrize("k,cfg,opt", _fluid_configs())
def test_random_fluid_configuration(monkeypatch, k, cfg, opt):
    """Random grids, layer widths, shot and point counts, surface, source type, FD order, pressure receivers, group size,
    pass sizes and checkpoint segments of the fluid propagator against the f32 oracle of the elastic scheme on
    mat5 = [K, K, 0, bx, bz]: the reference and the bounds of tests/test_fluid_gpu.py (cases.fluid_check)."""
    from cases import fluid_check, fluid_oracle, fluid_precondition
    from physicsbasedfwi2_amd import fluid
    from physicsbasedfwi2_amd._driver import checkpoint_schedule, segment_length
    c = _fluid_case(k, cfg)
    st, order = opt["source_type"], opt["order"]
    ref = fluid_oracle(c, st, order, pressure=opt["pressure"])
    fluid_precondition(c, ref)
    monkeypatch.setenv("MIFWI_FL_PASS_SHOTS", opt["pass_shots"])
    monkeypatch.setenv("MIFWI_FL_PASS_GROUPS", opt["pass_groups"])
    pl = fluid.FluidPlan(cfg["nz"], cfg["nx"], cfg["nt"], cfg["ns"], cfg["nsrc"], cfg["nrec"], 1, cfg["fw"], 0, opt["gs"],
                         c["fs"], st, order)
    step_bytes = 4 * pl.layout.snap_step_elems
    assert pl.pass_sizes()[0] == min(int(opt["pass_shots"]), cfg["ns"])
    pl.close()
    budget = None
    if opt["segments"]:
        seg = -(-cfg["nt"] // opt["segments"])
        budget = 2 * seg * step_bytes
        assert segment_length(budget, torch.device(DEV), step_bytes, cfg["nt"]) == seg
        assert len(checkpoint_schedule(cfg["nt"], seg, "elastic")[0]) >= 2
    fluid_check(c, ref, st, order, gs=opt["gs"], budget=budget, pressure=opt["pressure"])


def _cpml_configs():
    rng = np.random.default_rng(2029)
    out = []
    for k in range(int(os.environ.get("MIFWI_FUZZ_CPML", "14"))):      # more draws: a one-off soak of the layer's kernel forms
        w = int(rng.choice([4, 6, 7, 10, 12]))
        cfg = dict(n0=int(rng.integers(40, 110)), n1=int(rng.integers(48, 170)), w=w, ns=int(rng.integers(1, 6)),
                   nrec=int(rng.integers(1, 30)), nt=int(rng.integers(30, 90)), h=(10.0, float(rng.choice([10.0, 12.5]))))
        cfg["nt"] += cfg["n1"]            # long enough for the wave to reach a receiver (the traces must not be all zero)
        # the forms the single-launch kernels carry the layer in: edge slabs own-group / generic, the last
        # phase with / without its own barrier, layer arrays in LDS as far as they fit / less LDS / all through L2; slab
        # counts; the per-step family; time checkpointing
        opt = dict(cluster=str(int(rng.integers(0, 4) > 0)), own=str(int(rng.integers(0, 3) > 0)),
                   late=str(int(rng.integers(0, 3) > 0)), nw=str(int(rng.choice([0, 0, 3, 4, 5]))),
                   shrink=str(int(rng.choice([0, 0, 8, 24, 60]))), lds=str(int(rng.integers(0, 4) > 0)),
                   budget=(None if rng.integers(0, 3) else 1 << 20), gs=int(rng.integers(0, 3)))
        out.append((k, cfg, opt))
    return out


@pytest.mark.parametrize("k,cfg,opt", _cpml_configs())
def test_random_acoustic_cpml_configuration(oracle32, monkeypatch, k, cfg, opt):
    """The second-order C-PML (the deepwave-shaped API's default layer) on random grids, widths and shot counts through
    randomly drawn forms of the kernels, against oracle/acoustic_cpml.c: traces bit for bit, gradients <= 5e-5."""
    from physicsbasedfwi2_amd import acoustic
    from test_acoustic_gpu import _cpml_case
    monkeypatch.setenv("MIFWI_AC_CLUSTER", opt["cluster"])
    monkeypatch.setenv("MIFWI_AC_PML_OWN", opt["own"])
    monkeypatch.setenv("MIFWI_AC_PML_LATE_E", opt["late"])
    monkeypatch.setenv("MIFWI_AC_PML_LDS", opt["lds"])
    monkeypatch.setenv("MIFWI_AC_PML_LDS_SHRINK_KB", opt["shrink"])
    if opt["nw"] != "0":
        monkeypatch.setenv("MIFWI_AC_NW", opt["nw"])
    c = _cpml_case(seed=300 + k, **cfg)
    o = oracle32
    geo = (c["sc"], c["sw"], c["rc"], c["rw"])
    rec_o, G_o = o.acoustic_cpml_forward(c["r"], c["ab0"], c["ab1"], c["f"], *geo, c["c0"], c["c1"], save=True)
    r = torch.tensor(c["r"], dtype=torch.float32, device=DEV, requires_grad=True)
    f = torch.tensor(c["f"], dtype=torch.float32, device=DEV, requires_grad=True)
    kw = {} if opt["budget"] is None else {"snapshot_budget": opt["budget"]}
    rec = acoustic.propagate(r, f, torch.tensor(c["ab0"]), torch.tensor(c["ab1"]), *[torch.tensor(a) for a in geo],
                             c["c0"], c["c1"], cpml_width=c["w"], shots_per_group=opt["gs"], **kw)
    scale = np.abs(rec_o).max()
    assert scale > 0 and np.abs(rec.detach().cpu().numpy() - rec_o).max() == 0.0, (cfg, opt)
    g = (np.random.default_rng(k).standard_normal(rec_o.shape) * scale).astype(np.float32)
    rec.backward(torch.tensor(g, device=DEV))
    gr_o, gf_o = o.acoustic_cpml_backward(c["r"], c["ab0"], c["ab1"], *geo, g, G_o, c["c0"], c["c1"])
    assert rel_l2(r.grad.cpu().numpy(), gr_o) <= 5e-5, (cfg, opt)
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= 5e-5, (cfg, opt)
