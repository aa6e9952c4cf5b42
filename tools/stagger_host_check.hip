// Host check of the plan-time arithmetic in csrc/mifwi_stagger.h: stagger_grid, default_group_size, blocked_plane_elems
// and tile_taps_elems over a sweep of small grids, each result against the formulas the two create functions carried
// before the header existed (written out a second time below).  Needs no device.  Build with the host sanitizers and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -o /tmp/stagger_host_check tools/stagger_host_check.hip && /tmp/stagger_host_check
#include "../physicsbasedfwi2_amd/csrc/mifwi_stagger.h"

#include <cstdio>

namespace {

int cdiv(int a, int b) { return (a + b - 1) / b; }
long long rup(long long a, long long b) { return (a + b - 1) / b * b; }

// the geometry as mifwi_elastic.hip and mifwi_fluid.hip computed it (psi: 4 | 2); false: the C-PML refusal
bool old_grid(int nz, int nx, int pml_width, int psi, StaggerGrid *o)
{
    o->ng = cdiv(nx, 4);
    o->gp = 4 * o->ng;
    o->pitch = (int)rup(4 * (o->ng + 3), 32);
    o->field_stride = (long long)(nz + 4) * o->pitch;
    o->coef_elems = (long long)nz * o->gp;
    o->W = pml_width > 0 ? pml_width + 1 : 0;
    if (o->W > 0) {
        o->wl = (int)rup(o->W, 4);
        o->xr0 = ((nx - o->W) / 4) * 4;
        if (o->xr0 < o->wl || 2 * o->W > nz) return false;
        o->wx = o->wl + (o->gp - o->xr0);
    } else {
        o->wl = o->xr0 = o->wx = 0;
    }
    o->psix_shot = (long long)psi * nz * o->wx;
    o->psiz_shot = (long long)psi * 2 * o->W * o->gp;
    return true;
}

// elastic's rule with MIFWI_EL_GS unset (fluid's is the same with no environment variable at all)
int old_group_size(int spg, int nshot)
{
    int gs = spg > 0 ? spg : 4;
    if (gs > nshot) gs = nshot;
    if (spg <= 0 && gs == 4 && nshot % 4 != 0 && nshot % 3 == 0) gs = 3;
    return gs;
}
// ... and with MIFWI_EL_GS = env (> 0: no 3-rule; <= 0: one shot per group)
int old_group_size_env(int spg, int nshot, int env)
{
    int gs = spg;
    if (gs <= 0) gs = env;
    if (gs <= 0) gs = 1;
    if (gs > nshot) gs = nshot;
    if (spg <= 0 && env <= 0 && gs == 4 && nshot % 4 != 0 && nshot % 3 == 0) gs = 3;
    return gs;
}

}  // namespace

int main()
{
    const int sizes[] = {3, 4, 5, 16, 17, 63, 64, 65, 100}, widths[] = {0, 1, 2, 10, 31};
    const int shots[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 12}, recs[] = {0, 1, 5};
    long long checked = 0, refused = 0, bad = 0;
    auto expect = [&](bool ok, const char *what, int a, int b, int c, int d) {
        ++checked;
        if (!ok && ++bad <= 20) fprintf(stderr, "MISMATCH %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
    };
    for (int nz : sizes) for (int nx : sizes) for (int w : widths) for (int psi : {4, 2}) {
        StaggerGrid g, o;
        const int rc = stagger_grid(nz, nx, w, psi, &g);
        const bool fits = old_grid(nz, nx, w, psi, &o);
        expect((rc == MIFWI_OK) == fits, "refusal", nz, nx, w, psi);
        if (rc != MIFWI_OK) {
            char want[128];
            snprintf(want, sizeof want, "grid %dx%d too small for a %d-node C-PML", nz, nx, w);
            expect(rc == MIFWI_EINVAL && strcmp(mifwi::err_buf(), want) == 0, "refusal text", nz, nx, w, psi);
            ++refused;
            continue;
        }
        expect(g.ng == o.ng && g.gp == o.gp && g.pitch == o.pitch && g.field_stride == o.field_stride &&
               g.coef_elems == o.coef_elems, "grid", nz, nx, w, psi);
        expect(g.W == o.W && g.wl == o.wl && g.xr0 == o.xr0 && g.wx == o.wx, "strips", nz, nx, w, psi);
        expect(g.psix_shot == o.psix_shot && g.psiz_shot == o.psiz_shot, "psi", nz, nx, w, psi);
        expect(blocked_plane_elems(nz, g.ng) == 64LL * nz * cdiv(g.ng, 16), "blocked plane", nz, nx, w, psi);
        for (int ns : shots) for (int nr : recs) for (int ntap : {1, 4}) {
            const long long ntiles = (long long)cdiv(g.ng, 16) * cdiv(nz, 16);
            const long long want = std::max<long long>(1024, rup(ns * (2 * ntiles + 1 + (long long)nr * ntap), 64));
            expect(tile_taps_elems(ns, nz, g.ng, nr, ntap) == want, "tile taps", nz, nx, ns, nr * ntap);
        }
    }
    for (int ns : shots) for (int spg = -1; spg <= 13; ++spg) {
        expect(default_group_size(spg, ns, 4) == old_group_size(spg, ns), "group size", spg, ns, 4, 0);
        for (int env = -1; env <= 9; ++env)      // elastic's call with MIFWI_EL_GS = env
            expect(default_group_size(spg > 0 ? spg : env, ns, env) == old_group_size_env(spg, ns, env), "group size (env)",
                   spg, ns, env, 0);
    }
    printf("stagger_host_check: %lld comparisons, %lld grids refused by both sides, %lld mismatches\n", checked, refused, bad);
    return bad ? 1 : 0;
}
