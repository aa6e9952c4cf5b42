// Second moments of the elastic forward snapshot planes: the ingredient of the diagonal pseudo-Hessian (Shin et al.;
// DENISE's EPRECOND / EPSILON_WE preconditioner).  Included at the end of mifwi_elastic.hip: it reads the snapshot
// buffer exactly as the adjoint does (the plan, snap_cell, the bf16 helpers).
//
// The five planes a forward step saves are the virtual sources of the five material planes (oracle/elastic.c: S0 = exx',
// S1 = ezz', S2 = exz', S3, S4 = the two force sums).  Per cell, summed over the shots of the plan and the selected steps:
//   M0..M4 = sum Sk^2,   M5 = sum S0 S1
// (the cross moment because Vp, rho and lambda each move L = lambda s and M = (lambda + 2 mu) s together; the map from
// the moments to a pseudo-Hessian is mifwi_elastic_pseudo_hessian, csrc/mifwi_materials.hip).  This is a COLLOCATED
// approximation: the staggered averages of the material planes, the harmonic mu_xz and the effective row 0 under a
// free surface are ignored - every plane is taken as if it lived at the cell's own node.
//
// One thread owns one 4-cell group and keeps six float4 accumulators; it walks the shots, then its share of the selected
// steps, in a fixed order, with 16-byte loads (every layout a plan writes: row-major f32, column-blocked f32,
// column-blocked bf16).  The step range is split over blockIdx.y into partial planes (a 100x300 grid has 7.5 k groups,
// far too few threads for the stream); a second launch (mifwi_moments_sum.h) adds the partials in index order.  The split depends on the plan
// and the range only, there is no atomic anywhere: two identical calls give the same bits.
#pragma once
#include "mifwi_moments_sum.h"

namespace {

struct MomParams {
    const float *snap;      // shot 0 of the first selected step
    long long step;         // floats from one selected step to the next (stride * snap_step_elems)
    int nsel, per;          // selected steps; selected steps per blockIdx.y
    float *part;            // [gridDim.y][6][nz][gp], row-major whatever the snapshot layout
};

// threads of one partial plane: the 4-cell groups in the order they lie in a snapshot plane (blocked planes carry the
// pad groups of their last column block)
inline long long mom_threads(const mifwi_elastic_plan *pl)
{
    return pl->sblk ? 16LL * mifwi::ceil_div(pl->ng, 16) * pl->d.nz : (long long)pl->d.nz * pl->ng;
}
inline MomShape mom_shape(const mifwi_elastic_plan *pl) { return {6, mom_threads(pl), pl->snap_shot, pl->d.nx}; }

template <bool BF16>
__global__ __launch_bounds__(kThreads) void el_snapshot_moments(const ElParams p, const MomParams m)
{
    const int idx = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    int j, g;
    if (p.sblk) {                           // [g / 16][j][16 groups]: consecutive threads, consecutive 16 bytes
        const int b = idx / (16 * p.nz), r = idx - b * 16 * p.nz;
        j = r >> 4; g = 16 * b + (r & 15);
    } else {
        j = idx / p.ng; g = idx - j * p.ng;
    }
    if (j >= p.nz || g >= p.ng) return;     // pad groups of the last column block are never written by the forward
    const unsigned off = snap_cell(p, j, g);
    const long long sp = p.splane;
    const int k0 = (int)blockIdx.y * m.per, k1 = min(m.nsel, k0 + m.per);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 M0 = zero4, M1 = zero4, M2 = zero4, M3 = zero4, M4 = zero4, M5 = zero4;
    for (int s = 0; s < p.nshot; ++s) {
        const float *base = m.snap + (long long)s * p.snap_shot + (long long)k0 * m.step;
#pragma unroll 2
        for (int k = k0; k < k1; ++k, base += m.step) {
            float4 S0, S1, S2, S3, S4;
            if (BF16) {
                BfPlanes q;
                bf_request(base, p.splane, off >> 2, q);
                bf_widen(q, S0, S1, S2, S3, S4);
            } else {
                S0 = mifwi::ldnt4(el_at(base, off)); S1 = mifwi::ldnt4(el_at(base + sp, off));
                S2 = mifwi::ldnt4(el_at(base + 2 * sp, off)); S3 = mifwi::ldnt4(el_at(base + 3 * sp, off));
                S4 = mifwi::ldnt4(el_at(base + 4 * sp, off));
            }
#define MOM4(dst, a, b) dst.x = fmaf(a.x, b.x, dst.x); dst.y = fmaf(a.y, b.y, dst.y); \
                        dst.z = fmaf(a.z, b.z, dst.z); dst.w = fmaf(a.w, b.w, dst.w)
            MOM4(M0, S0, S0); MOM4(M1, S1, S1); MOM4(M2, S2, S2); MOM4(M3, S3, S3); MOM4(M4, S4, S4); MOM4(M5, S0, S1);
#undef MOM4
        }
    }
    const long long plane = (long long)p.nz * p.gp;
    float *o = m.part + 6LL * blockIdx.y * plane + (long long)j * p.gp + 4 * g;
    st4(o, M0); st4(o + plane, M1); st4(o + 2 * plane, M2); st4(o + 3 * plane, M3); st4(o + 4 * plane, M4);
    st4(o + 5 * plane, M5);
}

}  // namespace

extern "C" {

int64_t mifwi_elastic_snapshot_moments_work_elems(const mifwi_elastic_plan *pl)
{
    return moments_work_elems(pl, mom_shape);
}

int mifwi_elastic_snapshot_moments(mifwi_elastic_plan *pl, const float *snap, int32_t snap_first, int32_t n_begin,
                                   int32_t n_end, int32_t stride, float *moments, float *work, int32_t flags, void *stream)
{
    return snapshot_moments<MomParams>(pl, mom_shape, snap, snap_first, n_begin, n_end, stride, moments, work, flags, stream,
                                       [pl](const MomParams &m, int nsplit, hipStream_t st) {
        const ElParams p = el_base(pl, nullptr, nullptr, nullptr);
        const dim3 grid((unsigned)((mom_threads(pl) + kThreads - 1) / kThreads), nsplit), block(kThreads);
        if (pl->snap_bf16) hipLaunchKernelGGL(el_snapshot_moments<true>, grid, block, 0, st, p, m);
        else hipLaunchKernelGGL(el_snapshot_moments<false>, grid, block, 0, st, p, m);
    });
}

}  // extern "C"
