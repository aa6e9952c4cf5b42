// What the two snapshot-moments passes share (mifwi_elastic_moments.h, mifwi_acoustic_moments.h): the argument checks of
// their entry points, and their second launch - the partial planes the first launch left in `work` are added in index
// order, a fixed order, no atomics.
#pragma once

namespace {

// the argument checks both snapshot-moments entry points open with (behind their null checks)
inline int moments_check(int nt, const void *snap, const void *moments, const void *work, int snap_first, int n_begin,
                         int n_end, int stride)
{
    if (stride < 1) return mifwi::fail(MIFWI_EINVAL, "stride %d: must be >= 1", stride);
    if (n_begin < 0 || n_end > nt || n_begin >= n_end)
        return mifwi::fail(MIFWI_EINVAL, "bad step range [%d,%d) for nt=%d", n_begin, n_end, nt);
    if (snap_first < 0 || snap_first > n_begin)
        return mifwi::fail(MIFWI_EINVAL, "snap_first %d lies behind the range [%d,%d)", snap_first, n_begin, n_end);
    if (((uintptr_t)snap | (uintptr_t)moments | (uintptr_t)work) & 15)
        return mifwi::fail(MIFWI_EINVAL, "snap, moments and work must be 16-byte aligned");
    return MIFWI_OK;
}

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

}  // namespace
