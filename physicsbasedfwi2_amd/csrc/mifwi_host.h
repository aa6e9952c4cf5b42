// What every propagator (scalar acoustic, elastic, fluid) shares besides the single-launch driver (mifwi_cluster_host.h, which holds host code only):
// the selector -> kernel dispatch behind every variant table, the opening of a C-ABI call, the plan-time rules for the
// tile width and the Infinity Cache passes - and the shared device code: the bounding box of a shot's point set (per-step
// kernels), the row-slab split and the per-slab receiver lists (single-launch kernels and their plans).  What only the two
// staggered-grid families share is in mifwi_stagger.h.
#pragma once
#include "mifwi_common.h"

#include <cmath>

namespace mifwi {

// ---- variant tables -----------------------------------------------------------------------------------
// A kernel family has ONE function that maps its runtime selectors to the address of an instantiation (ac_cluster_variant,
// el_step_variant, ...): the launch calls it and launches through the pointer, the LDS-attribute pass walks its whole
// domain (mifwi::lds_cap_once).  The instantiations named inside that function are the ones the library carries.
// with_bool / with_int (mifwi_common.h) hand a runtime selector to it as a std::integral_constant.

// ---- the opening of a call ----------------------------------------------------------------------------
// Range checks shared by the entry points (forward / Born: steps [n_begin, n_end); a pass that reads snapshots: the
// first step it needs must be in the buffer).
inline int check_steps(int n_begin, int n_end, int nt)
{
    if (n_begin < 0 || n_end > nt || n_begin > n_end)
        return fail(MIFWI_EINVAL, "bad step range [%d,%d) for nt=%d", n_begin, n_end, nt);
    return MIFWI_OK;
}
// adjoint: steps hi down to lo (`name`: what the physics calls its step index, `lowest`: its first adjoint step)
inline int check_adjoint_steps(char name, int lowest, int hi, int lo, int nt)
{
    if (lo < lowest || hi > nt - 1 || lo > hi + 1)
        return fail(MIFWI_EINVAL, "bad adjoint range %c=%d..%d for nt=%d", name, hi, lo, nt);
    return MIFWI_OK;
}
inline int check_snapshots(int snap_first, int needed)
{
    if (snap_first > needed)
        return fail(MIFWI_EINVAL, "snapshots start at step %d but step %d is needed", snap_first, needed);
    return MIFWI_OK;
}
// A propagation call once its arguments are checked (`m`: the physics' work_map of the call's work buffer): device and
// stream, and the state zeroed when the call starts from rest (MIFWI_ZERO_STATE).  Nothing is enqueued before this.
template <class Map>
int open_call(int device, void *stream, float *work, const Map &m, int32_t flags, hipStream_t *st)
{
    int rc = select_device(device, stream, st);
    if (rc) return rc;
    if (flags & MIFWI_ZERO_STATE) MIFWI_HIP_TRY(hipMemsetAsync(work, 0, sizeof(float) * m.state, *st));
    return MIFWI_OK;
}

// ---- plan-time rules ----------------------------------------------------------------------------------
// lanes per row of the per-step kernels' tiles: the widest tile whose padding waste stays small (ng: 4-cell groups per row)
inline int pick_lx(int ng)
{
    for (int cand : {64, 32}) {
        const int padded = ceil_div(ng, cand) * cand;
        if (padded * 10 <= ng * 12) return cand;
    }
    return 16;
}

// Infinity Cache residency of the per-step families: the units (shots, shot groups) a pass over the time range takes.
// All `n` while n units of `unit` bytes beside `fixed` bytes (model, materials) stay within `trigger` bytes; otherwise as
// many as fit `target` bytes - and `none_fit` when not even one does.  The bounds are measurements: they and the figures
// behind them stand at the call sites.
inline int units_per_pass(int n, double unit, double fixed, double trigger, double target, int none_fit)
{
    if (n * unit + fixed <= trigger) return n;
    const double k = std::floor((target - fixed) / unit);
    return k < 1.0 ? none_fit : (int)k;
}

}  // namespace mifwi

namespace {

// ---- a shot's point set -------------------------------------------------------------------------------
constexpr int kPointThreads = 256;

// per-shot bounding box of a point set (sources or receivers; dead taps, cell < 0, left out), one block per shot
__global__ void points_bbox(const int *cell, int npts_per_shot, int n1, int *bbox)
{
    __shared__ int red[4][kPointThreads];
    const int s = blockIdx.x;
    int a0 = 0x7fffffff, a1 = -1, b0 = 0x7fffffff, b1 = -1;
    for (int e = threadIdx.x; e < npts_per_shot; e += kPointThreads) {
        const int c = cell[(long long)s * npts_per_shot + e];
        if (c < 0) continue;
        const int i0 = c / n1, i1 = c - i0 * n1;
        a0 = min(a0, i0); a1 = max(a1, i0); b0 = min(b0, i1); b1 = max(b1, i1);
    }
    red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1;
    red[2][threadIdx.x] = b0; red[3][threadIdx.x] = b1;
    __syncthreads();
    for (int st = kPointThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + st]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + st]);
            red[2][threadIdx.x] = min(red[2][threadIdx.x], red[2][threadIdx.x + st]);
            red[3][threadIdx.x] = max(red[3][threadIdx.x], red[3][threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bbox[4 * s + 0] = red[0][0]; bbox[4 * s + 1] = red[1][0];
        bbox[4 * s + 2] = red[2][0]; bbox[4 * s + 3] = red[3][0];
    }
}
inline void launch_points_bbox(const int *cell, int nshot, int npts_per_shot, int n1, int *bbox, hipStream_t st)
{
    hipLaunchKernelGGL(points_bbox, dim3(nshot), dim3(kPointThreads), 0, st, cell, npts_per_shot, n1, bbox);
}

// Row slabs of a shot (single-launch kernels).  rt == 0: n0 rows split evenly over NW slabs.  rt > 0 (NW >= 3): the first
// and the last slab hold rt rows each - the acoustic absorbing layer, whose cells cost an IEEE division per step - and
// the other NW-2 slabs share the rest evenly, so that the all-sponge slabs do not set the pace.  (Elastic: rt = 0.)
__host__ __device__ __forceinline__ void slab_rows(int n0, int NW, int rt, int w, int &r0, int &rows)
{
    if (rt > 0) {
        if (w == 0) { r0 = 0; rows = rt; return; }
        if (w == NW - 1) { r0 = n0 - rt; rows = rt; return; }
        const int m = n0 - 2 * rt, k = NW - 2, v = w - 1;
        const int base = m / k, rem = m - base * k;
        rows = base + (v < rem ? 1 : 0);
        r0 = rt + v * base + (v < rem ? v : rem);
        return;
    }
    const int base = n0 / NW, rem = n0 - base * NW;
    rows = base + (w < rem ? 1 : 0);
    r0 = w * base + (w < rem ? w : rem);
}

__host__ __device__ __forceinline__ int slab_of_row(int n0, int NW, int rt, int i0)
{
    int m = n0, k = NW, off = 0, first = 0;
    if (rt > 0) {
        if (i0 < rt) return 0;
        if (i0 >= n0 - rt) return NW - 1;
        m = n0 - 2 * rt; k = NW - 2; off = rt; first = 1;
    }
    const int base = m / k, rem = m - base * k, i = i0 - off;
    return first + ((i < rem * (base + 1)) ? i / (base + 1) : rem + (i - rem * (base + 1)) / base);
}

// lists of the receiver taps that fall into each slab (adjoint sources of the single-launch loops), one block per shot:
// slab_cnt [nshot][NW], slab_list [nshot][NW][ntaps]
__global__ void build_slab_lists(const int *rec_cell, int ntaps, int n0, int n1, int NW, int rt,
                                 int *slab_cnt, int *slab_list)
{
    const int s = blockIdx.x;
    __shared__ int cnt[64];
    if ((int)threadIdx.x < NW) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < ntaps; e += blockDim.x) {
        const int cell = rec_cell[(long long)s * ntaps + e];
        if (cell < 0) continue;
        const int w = slab_of_row(n0, NW, rt, cell / n1);
        const int pos = atomicAdd(&cnt[w], 1);
        slab_list[((long long)s * NW + w) * ntaps + pos] = e;
    }
    __syncthreads();
    if ((int)threadIdx.x < NW) slab_cnt[s * NW + threadIdx.x] = cnt[threadIdx.x];
}
// `lists`: the region of the work buffer that holds both, [counts | lists]
inline void launch_build_slab_lists(const int *rec_cell, int nshot, int ntaps, int n0, int n1, int NW, int rt, int *lists,
                                    hipStream_t st)
{
    hipLaunchKernelGGL(build_slab_lists, dim3(nshot), dim3(256), 0, st, rec_cell, ntaps, n0, n1, NW, rt, lists,
                       lists + (long long)nshot * NW);
}

}  // namespace
