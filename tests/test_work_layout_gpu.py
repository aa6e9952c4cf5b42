"""The numbers a plan reports - padded sizes, the work buffer's sizes, the head of it that is the state, slab counts of the
single-launch kernels, shots per pass - are a contract between calls (a checkpoint written by one call is read by another) and
with the Python side, which allocates by them.  They are pinned here against the values the library reported before the
work-buffer maps and the slab-count search were gathered into one place each (recorded_parent.json, recorded on an
MI355X from the library of commit 70b3316).  Plan creation asks the device for its CU count, hence the gpu mark; no time loop runs."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

AC_FIELDS = ("gp", "pitch", "ngroups", "shots_per_group", "field_elems", "coef_elems", "state_elems",
             "work_forward_elems", "work_backward_elems")
EL_FIELDS = AC_FIELDS[:4] + AC_FIELDS[5:] + ("snap_step_elems", "snapshot_format", "kernel_flags")

# name -> (physics, plan arguments (positional, keyword), environment)
# acoustic: n0, n1, nt, nshot, nsrc, nrec, ntap, c0, c1, device;  elastic: nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device
PLANS = {
    "ac_120x200_sponge_6": ("ac", (120, 200, 120, 6, 1, 40, 1, 1.0, 1.0, 0), {}, {}),                  # single launch
    "ac_120x200_edge10_6": ("ac", (120, 200, 120, 6, 1, 40, 1, 1.0, 1.0, 0), {"edge_rows": 10}, {}),   # uneven slabs priced
    "ac_100x150_cpml10_3": ("ac", (100, 150, 130, 3, 1, 30, 1, 1.0, 1.0, 0), {"cpml_width": 10}, {}),  # edge slabs W + 2
    "ac_101x150_cpml9_3": ("ac", (101, 150, 130, 3, 1, 30, 1, 1.0, 1.0, 0), {"cpml_width": 9}, {}),    # odd W * n0: rounded regions
    "ac_120x200_ntap4_6": ("ac", (120, 200, 120, 6, 1, 40, 4, 1.0, 1.0, 0), {}, {}),                   # no single launch
    "ac_120x200_gs3_6": ("ac", (120, 200, 120, 6, 1, 40, 4, 1.0, 1.0, 0), {"shots_per_group": 3}, {}),
    "ac_1000x3000_16": ("ac", (1000, 3000, 100, 16, 1, 300, 1, 1.0, 1.0, 0), {}, {}),                  # passes, no single launch
    "ac_40x64_2": ("ac", (40, 64, 20, 2, 1, 7, 1, 1.0, 1.0, 0), {}, {}),
    "ac_120x200_nw5_6": ("ac", (120, 200, 120, 6, 1, 40, 1, 1.0, 1.0, 0), {}, {"MIFWI_AC_NW": "5"}),
    "el_100x300_fw10_6": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {}, {}),          # both single-launch kernels, lane halo
    "el_100x300_gs2_6": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {"shots_per_group": 2}, {}),      # forward single launch only
    "el_100x300_ntap4_6": ("el", (100, 300, 120, 6, 1, 100, 4, 10, 0), {}, {}),                        # per-step only, tile lists
    "el_100x300_pressure_6": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {"record_pressure": 1}, {}),
    "el_100x300_fs_nopml_3": ("el", (100, 300, 120, 3, 1, 50, 1, 0, 0), {"free_surface": 1}, {}),
    "el_350x1700_6": ("el", (350, 1700, 100, 6, 1, 400, 1, 20, 0), {}, {}),                            # fused forward, blocked snapshots
    "el_350x1700_bf16_6": ("el", (350, 1700, 100, 6, 1, 400, 1, 20, 0), {"snapshot_format": "bf16"}, {}),
    "el_100x300_bf16_6": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {"snapshot_format": "bf16"}, {}),  # single launch keeps f32
    "el_1000x3000_16": ("el", (1000, 3000, 100, 16, 1, 300, 1, 20, 0), {}, {}),                        # passes of both families
    "el_200x500_40": ("el", (200, 500, 100, 40, 1, 100, 1, 10, 0), {}, {}),                            # several launches per attempt
    "el_40x64_fw6_2": ("el", (40, 64, 20, 2, 1, 9, 1, 6, 0), {}, {}),
    "el_100x300_nw4_adj5": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {}, {"MIFWI_EL_NW": "4", "MIFWI_EL_ADJ_NW": "5"}),
    "el_100x300_nw10_adj2": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {}, {"MIFWI_EL_NW": "10", "MIFWI_EL_ADJ_NW": "2"}),
    "el_100x300_skew3": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {}, {"MIFWI_EL_PL_SKEW": "3"}),    # pitch falls back per loop
    "el_100x300_no_fwd": ("el", (100, 300, 120, 6, 1, 100, 1, 10, 0), {}, {"MIFWI_EL_CLUSTER": "0"}),   # adjoint single launch only
}


def describe(name):
    """What the library reports for one plan of the table, as plain ints (the recording used this very function)."""
    from physicsbasedfwi2_amd.acoustic import AcousticPlan
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    kind, args, kw, _ = PLANS[name]
    plan = (AcousticPlan if kind == "ac" else ElasticPlan)(*args, **kw)
    out = {k: int(getattr(plan.layout, k)) for k in (AC_FIELDS if kind == "ac" else EL_FIELDS)}
    out["cluster_slabs"] = [plan.cluster_slabs(False), plan.cluster_slabs(True)]
    out["pass_sizes"] = list(plan.pass_sizes())
    plan.close()
    return out


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "recorded_parent.json")) as _f:
    RECORDED = json.load(_f)


def test_the_table_is_the_recorded_one():
    assert RECORDED["parent_commit"].startswith("70b3316")
    assert sorted(RECORDED["plans"]) == sorted(PLANS)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_reports_what_the_parent_reported(monkeypatch, name):
    for k, v in PLANS[name][3].items():
        monkeypatch.setenv(k, v)
    assert describe(name) == RECORDED["plans"][name]


def test_the_table_reaches_every_kind_of_plan():
    """Guards the table itself: the recorded values must show each branch of the maps and of the slab search taken."""
    p = RECORDED["plans"]
    assert p["ac_120x200_sponge_6"]["cluster_slabs"][0] >= 1 and p["ac_100x150_cpml10_3"]["cluster_slabs"][0] >= 3
    assert p["ac_120x200_ntap4_6"]["cluster_slabs"] == [0, 0] and p["ac_1000x3000_16"]["cluster_slabs"] == [0, 0]
    assert p["ac_1000x3000_16"]["pass_sizes"][0] < p["ac_1000x3000_16"]["ngroups"]
    assert p["el_100x300_fw10_6"]["kernel_flags"] & 51 == 51                # both single-launch kernels, both with the lane halo
    assert p["el_100x300_gs2_6"]["kernel_flags"] & 3 == 1 and p["el_100x300_no_fwd"]["kernel_flags"] & 3 == 2
    assert p["el_100x300_ntap4_6"]["kernel_flags"] & 3 == 0 and p["el_100x300_pressure_6"]["kernel_flags"] & 3 == 0
    assert p["el_350x1700_6"]["kernel_flags"] & 7 == 4 and p["el_350x1700_bf16_6"]["snapshot_format"] == 1
    # forced slab counts: taken where the slabs fit (13 rows of 100x300 at most), no single launch where they do not
    assert p["el_100x300_nw10_adj2"]["cluster_slabs"] == [10, 0] and p["el_100x300_nw4_adj5"]["cluster_slabs"] == [0, 0]
