// Second moment of the scalar scheme's forward snapshot plane: the ingredient of the acoustic diagonal pseudo-Hessian
// (Shin et al.).  Included at the end of mifwi_acoustic.hip: it reads the snapshot buffer exactly as the adjoint does.
//
// The plane G^n a forward step saves is the virtual source of the coefficient r (the Born pass injects G^n dr), so per
// cell, summed over the shots of the plan and the selected steps,
//   M = sum (G^n)^2
// is the diagonal of J^T J with respect to r with the propagation between the cells left out; the map to a model
// parameter is mifwi_acoustic_pseudo_hessian (csrc/mifwi_materials.hip).
//
// Every plan writes the same layout, step n of shot s at snap + ((n - snap_first) nshot + s) n0 gp, row-major f32, so one
// thread owns one 4-cell group of the plane and keeps one float4 accumulator; it walks the shots, then its share of the
// selected steps, in a fixed order, kAcMomUnroll independent 16-byte non-temporal loads in flight.  The reference's grids
// are small and long (191 x 240 cells: 11.5 k groups, 4001 steps), far too few threads for the stream: the step range is
// split over blockIdx.y into partial planes, and a second launch (mifwi_moments_sum.h) adds them in index order.  The
// split depends on the plan and the range only, there is no atomic anywhere: two identical calls give the same bits.
#pragma once
#include "mifwi_moments_sum.h"

namespace {

struct AcMomParams {
    const float *snap;      // shot 0 of the first selected step
    long long step, shot;   // floats from one selected step to the next (stride * nshot * n0 * gp); from shot to shot
    int nshot, ngr;         // shots; 4-cell groups of a plane
    int nsel, per;          // selected steps; selected steps per blockIdx.y
    float *part;            // [gridDim.y][n0][gp]
};

constexpr int kAcMomUnroll = 4;

inline MomShape ac_mom_shape(const mifwi_acoustic_plan *pl)
{
    return {1, pl->coef_elems / 4, pl->coef_elems, pl->d.n1};
}

__device__ __forceinline__ void ac_mom_add(float4 &m, const float4 &v)
{
    m.x = fmaf(v.x, v.x, m.x); m.y = fmaf(v.y, v.y, m.y); m.z = fmaf(v.z, v.z, m.z); m.w = fmaf(v.w, v.w, m.w);
}

__global__ __launch_bounds__(kThreads) void ac_snapshot_moments(const AcMomParams m)
{
    const int idx = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (idx >= m.ngr) return;
    const int k0 = (int)blockIdx.y * m.per, k1 = min(m.nsel, k0 + m.per);
    float4 M = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < m.nshot; ++s) {
        const float *p = m.snap + (long long)s * m.shot + (long long)k0 * m.step + 4LL * idx;
        int k = k0;
        for (; k + kAcMomUnroll <= k1; k += kAcMomUnroll, p += kAcMomUnroll * m.step) {
            float4 v[kAcMomUnroll];
#pragma unroll
            for (int u = 0; u < kAcMomUnroll; ++u) v[u] = mifwi::ldnt4(p + u * m.step);
#pragma unroll
            for (int u = 0; u < kAcMomUnroll; ++u) ac_mom_add(M, v[u]);      // the order of the plain loop
        }
        for (; k < k1; ++k, p += m.step) ac_mom_add(M, mifwi::ldnt4(p));
    }
    *reinterpret_cast<float4 *>(m.part + (long long)blockIdx.y * 4 * m.ngr + 4LL * idx) = M;
}

}  // namespace

extern "C" {

int64_t mifwi_acoustic_snapshot_moments_work_elems(const mifwi_acoustic_plan *pl)
{
    return moments_work_elems(pl, ac_mom_shape);
}

int mifwi_acoustic_snapshot_moments(mifwi_acoustic_plan *pl, const float *snap, int32_t snap_first, int32_t n_begin,
                                    int32_t n_end, int32_t stride, float *moments, float *work, int32_t flags, void *stream)
{
    return snapshot_moments<AcMomParams>(pl, ac_mom_shape, snap, snap_first, n_begin, n_end, stride, moments, work, flags,
                                         stream, [pl](AcMomParams &m, int nsplit, hipStream_t st) {
        m.shot = pl->coef_elems;
        m.nshot = pl->d.nshot;
        m.ngr = (int)(pl->coef_elems / 4);
        const dim3 grid((unsigned)mifwi::ceil_div(m.ngr, kThreads), nsplit), block(kThreads);
        hipLaunchKernelGGL(ac_snapshot_moments, grid, block, 0, st, m);
    });
}

}  // extern "C"
