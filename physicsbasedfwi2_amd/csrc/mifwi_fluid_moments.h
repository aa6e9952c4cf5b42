// Second moments of the fluid forward snapshot planes: the ingredient of the diagonal pseudo-Hessian of the
// variable-density acoustic gradient (mifwi_fluid_pseudo_hessian, csrc/mifwi_materials.hip).  Included at the end of
// mifwi_fluid.hip: it reads the snapshot buffer exactly as the adjoint does (the plan, snap_cell).
//
// The three planes a forward step saves are the virtual sources of the three material planes (S0 = e1' + e2' of K,
// S1 = d1' of bx, S2 = d4' of bz).  Per cell, summed over the shots of the plan and the selected steps:
//   M0 = sum S0^2,  M1 = sum S1^2,  M2 = sum S2^2
// (no cross moment: the fluid's S0 is already the sum exx' + ezz' the elastic route squares through M0 + M1 + 2 M5).
// The same COLLOCATED approximation as the elastic moments.
//
// One thread owns one 4-cell group and keeps three float4 accumulators; it walks the shots, then its share of the selected
// steps, in a fixed order, with 16-byte loads.  Threads are numbered in the order the groups lie in the column-blocked
// plane (consecutive threads, consecutive 16 bytes); the pad groups of the last column block are never read (the forward
// never writes them).  The step range is split over blockIdx.y into partial planes; a second launch (mifwi_moments_sum.h)
// adds the partials in index order.  The split depends on the plan and the range only, there is no atomic anywhere: two
// identical calls give the same bits.
#pragma once
#include "mifwi_moments_sum.h"

namespace {

struct FlMomParams {
    const float *snap;      // shot 0 of the first selected step
    long long step;         // floats from one selected step to the next (stride * snap_step_elems)
    int nsel, per;          // selected steps; selected steps per blockIdx.y
    float *part;            // [gridDim.y][3][nz][gp], row-major
};

// threads of one partial plane: the 4-cell groups of a snapshot plane, pad groups of the last column block included
inline long long fl_mom_threads(const mifwi_fluid_plan *pl) { return pl->splane / 4; }
inline MomShape fl_mom_shape(const mifwi_fluid_plan *pl) { return {3, fl_mom_threads(pl), 3 * pl->splane, pl->d.nx}; }

__global__ __launch_bounds__(kThreads) void fl_snapshot_moments(const FlParams p, const FlMomParams m)
{
    const long long idx = (long long)blockIdx.x * kThreads + (long long)threadIdx.x;
    // [g / 16][j][16 groups]
    const long long per_block = 16LL * p.nz;
    const int b = (int)(idx / per_block), r = (int)(idx - (long long)b * per_block);
    const int j = r >> 4, g = 16 * b + (r & 15);
    if (j >= p.nz || g >= p.ng) return;
    const unsigned off = snap_cell(p, j, g);
    const long long sp = p.splane;
    const int k0 = (int)blockIdx.y * m.per, k1 = min(m.nsel, k0 + m.per);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 M0 = zero4, M1 = zero4, M2 = zero4;
    for (int s = 0; s < p.nshot; ++s) {
        const float *base = m.snap + 3LL * s * sp + (long long)k0 * m.step + off;
#pragma unroll 2
        for (int k = k0; k < k1; ++k, base += m.step) {
            const float4 S0 = mifwi::ldnt4(base), S1 = mifwi::ldnt4(base + sp), S2 = mifwi::ldnt4(base + 2 * sp);
#define FL_MOM4(dst, a) dst.x = fmaf(a.x, a.x, dst.x); dst.y = fmaf(a.y, a.y, dst.y); \
                        dst.z = fmaf(a.z, a.z, dst.z); dst.w = fmaf(a.w, a.w, dst.w)
            FL_MOM4(M0, S0); FL_MOM4(M1, S1); FL_MOM4(M2, S2);
#undef FL_MOM4
        }
    }
    const long long plane = (long long)p.nz * p.gp;
    float *o = m.part + 3LL * blockIdx.y * plane + (long long)j * p.gp + 4 * g;
    st4(o, M0); st4(o + plane, M1); st4(o + 2 * plane, M2);
}

}  // namespace

extern "C" {

int64_t mifwi_fluid_snapshot_moments_work_elems(const mifwi_fluid_plan *pl)
{
    return moments_work_elems(pl, fl_mom_shape);
}

int mifwi_fluid_snapshot_moments(mifwi_fluid_plan *pl, const float *snap, int32_t snap_first, int32_t n_begin,
                                 int32_t n_end, int32_t stride, float *moments, float *work, int32_t flags, void *stream)
{
    if (const int rc = check_medium(pl, kLossless)) return rc;       // the pseudo-Hessian of a viscoacoustic medium is not built
    return snapshot_moments<FlMomParams>(pl, fl_mom_shape, snap, snap_first, n_begin, n_end, stride, moments, work, flags,
                                         stream, [pl](const FlMomParams &m, int nsplit, hipStream_t st) {
        const FlParams p = fl_base(pl, nullptr, nullptr, nullptr);
        const dim3 grid((unsigned)((fl_mom_threads(pl) + kThreads - 1) / kThreads), nsplit), block(kThreads);
        hipLaunchKernelGGL(fl_snapshot_moments, grid, block, 0, st, p, m);
    });
}

}  // extern "C"
