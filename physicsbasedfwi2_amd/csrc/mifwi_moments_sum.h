// What the three snapshot-moments passes share (mifwi_acoustic_moments.h, mifwi_elastic_moments.h, mifwi_fluid_moments.h):
// the host body of their entry points - argument checks, selection of the steps, split into partial planes - and their
// second launch: the partial planes the first launch left in `work` are added in index order, a fixed order, no atomics.
#pragma once

namespace {

constexpr int kMomSumThreads = 256;

// out [n] = (add ? out : 0) + w * (part[0] + part[1] + ...); n floats = whole rows of gp columns, columns >= nx are
// written as 0 whatever the partial planes hold there
__global__ __launch_bounds__(kMomSumThreads) void moments_sum(const float *part, int nsplit, long long n, int gp, int nx, float w,
                                                              int add, float *out)
{
    const long long e = 4 * ((long long)blockIdx.x * kMomSumThreads + threadIdx.x);
    if (e >= n) return;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nsplit; ++c) {
        const float4 v = *reinterpret_cast<const float4 *>(part + (long long)c * n + e);
        a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
    }
    const float4 old = add ? *reinterpret_cast<const float4 *>(out + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float o[4] = {old.x, old.y, old.z, old.w};
    const int col = (int)(e % gp);
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = col + c < nx ? fmaf(w, a[c], o[c]) : 0.f;
    *reinterpret_cast<float4 *>(out + e) = make_float4(r[0], r[1], r[2], r[3]);
}

inline void launch_moments_sum(const float *part, int nsplit, long long n, int gp, int nx, float w, int add, float *out,
                               hipStream_t st)
{
    hipLaunchKernelGGL(moments_sum, dim3((unsigned)((n / 4 + kMomSumThreads - 1) / kMomSumThreads)), dim3(kMomSumThreads), 0, st,
                       part, nsplit, n, gp, nx, w, add, out);
}

// enough threads to keep the snapshot stream busy (256 CUs x 16 waves), at most 64 partial planes
constexpr long long kMomThreads = 256LL * 16 * 64;
constexpr int kMomMaxSplit = 64;

// what a pass tells the shared host code about its plan: moment planes, threads of one partial plane (its 4-cell groups
// in the order they lie in a snapshot plane), floats of one shot in a snapshot step, visible columns of a row
struct MomShape {
    int planes;
    long long threads, snap_shot;
    int ncol;
};

inline int moments_max_split(const MomShape &s)
{
    return (int)std::min<long long>(kMomMaxSplit, std::max<long long>(1, (kMomThreads + s.threads - 1) / s.threads));
}

template <class Plan, class Shape>
int64_t moments_work_elems(const Plan *pl, Shape shape)
{
    return pl ? shape(pl).planes * pl->coef_elems * moments_max_split(shape(pl)) : 0;
}

// The body of mifwi_<physics>_snapshot_moments.  `shape(pl)` -> MomShape; `launch(m, nsplit, st)` launches the pass's own
// kernel over `nsplit` partial planes with Params m, whose snap, step, nsel, per and part are filled in here.
template <class Params, class Plan, class Shape, class Launch>
int snapshot_moments(const Plan *pl, Shape shape, const float *snap, int snap_first, int n_begin, int n_end, int stride,
                     float *moments, float *work, int flags, void *stream, Launch launch)
{
    if (!pl || !snap || !moments || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    const int nt = pl->d.nt;
    if (stride < 1) return mifwi::fail(MIFWI_EINVAL, "stride %d: must be >= 1", stride);
    if (n_begin < 0 || n_end > nt || n_begin >= n_end)
        return mifwi::fail(MIFWI_EINVAL, "bad step range [%d,%d) for nt=%d", n_begin, n_end, nt);
    if (snap_first < 0 || snap_first > n_begin)
        return mifwi::fail(MIFWI_EINVAL, "snap_first %d lies behind the range [%d,%d)", snap_first, n_begin, n_end);
    if (((uintptr_t)snap | (uintptr_t)moments | (uintptr_t)work) & 15)
        return mifwi::fail(MIFWI_EINVAL, "snap, moments and work must be 16-byte aligned");
    hipStream_t st;
    if (int rc = mifwi::select_device(pl->device, stream, &st)) return rc;
    const MomShape s = shape(pl);
    // selected steps: the multiples of stride inside the range (absolute n, so a run cut into ranges anywhere selects
    // the same steps as the whole run)
    const long long first = ((long long)n_begin + stride - 1) / stride * stride;
    const int nsel = first < n_end ? (int)((n_end - 1 - first) / stride) + 1 : 0;
    const long long snap_step = s.snap_shot * pl->d.nshot;
    int nsplit = 0;
    if (nsel > 0) {
        Params m;
        m.per = mifwi::ceil_div(nsel, std::min(nsel, moments_max_split(s)));
        nsplit = mifwi::ceil_div(nsel, m.per);
        m.snap = snap + (first - snap_first) * snap_step;
        m.step = (long long)stride * snap_step;
        m.nsel = nsel;
        m.part = work;
        launch(m, nsplit, st);
    }
    launch_moments_sum(work, nsplit, s.planes * pl->coef_elems, pl->gp, s.ncol, (float)stride,
                       (flags & MIFWI_ZERO_STATE) ? 0 : 1, moments, st);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // namespace
