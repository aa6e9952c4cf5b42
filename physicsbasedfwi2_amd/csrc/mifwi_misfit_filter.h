// The stage filter F of the misfit kernels (included by mifwi_misfit.hip): the causal recursive Butterworth filter that
// DENISE's frequency stages apply along time (add_fwi_stage(fc_low, fc_high), models/networks.py:6374 ... 11676) and its
// transpose, as the sweep that the staged objectives of mifwi_misfit.hip (misfit_staged_l2, misfit_staged_gc) run inside
// their one launch, and as a kernel of its own (trace_filter).
// F is a cascade of nsec second-order sections in transposed direct form II with zero initial state,
//     y = b0 x + s1;   s1 = b1 x - a1 y + s2;   s2 = b2 x - a2 y;     (x of the next section = y)
// which is what scipy.signal.sosfilt runs; F^T is the same recurrence from the last sample to the first (exact for a finite
// trace with zero initial state: the sections are lower-triangular Toeplitz matrices, they commute and transpose to the
// time-reversed recurrence).  Coefficients and state are double - the 2 Hz high-pass at a 2.5 ms step has poles within 3 %
// of the unit circle - traces are read and written as float, so the only float roundings are the stored intermediate and
// the output.
//
// One lane owns one trace for the whole kernel, a workgroup is one wave = 64 neighbouring traces: every sample step is one
// coalesced 256-byte row, nothing is shared, nothing is atomic.  The recurrence is a serial chain of double operations per
// trace, so the kernel is latency-bound (the reference's batches are 22 ... 138 waves): the rows of the NEXT chunk of kCh
// samples are requested before the recurrence runs over the current one, which keeps the memory round trip off the chain.
// The section state lives in registers (templates on nsec, every array index is a compile-time constant after unrolling;
// the compiler's resource report must say 0 bytes of scratch - tools/stage_filter_rate.py --resources).  The coefficients
// travel by value in the kernel arguments and stay wave-uniform.
#pragma once
#include <cmath>

namespace mifwi_filter {

constexpr int kLanes = 64;       // traces per workgroup = one wave
constexpr int kCh = 16;          // rows requested ahead of the recurrence

struct Sos {                     // a0 == 1 (checked on the host); unused sections are never read
    double b0[MIFWI_FILTER_MAX_SECTIONS], b1[MIFWI_FILTER_MAX_SECTIONS], b2[MIFWI_FILTER_MAX_SECTIONS];
    double a1[MIFWI_FILTER_MAX_SECTIONS], a2[MIFWI_FILTER_MAX_SECTIONS];
};

#ifdef __HIPCC__
// One sweep of NCHAN traces of this lane through the cascade, first sample to last (REV: last to first).
// in(t, x[NCHAN]) delivers sample t, out(t, y[NCHAN]) takes the filtered one; out(t) may store where in(t) read (in-place),
// because sample t is requested before out(t') of any earlier-swept t' != t is stored and never again.
template <int NSEC, int NCHAN, bool REV, class In, class Out>
__device__ __forceinline__ void sweep(const Sos &c, int nt, In in, Out out)
{
    double s1[NCHAN][NSEC], s2[NCHAN][NSEC];
#pragma unroll
    for (int q = 0; q < NCHAN; ++q)
#pragma unroll
        for (int k = 0; k < NSEC; ++k) s1[q][k] = s2[q][k] = 0.0;
    // rows past the end are requested as the last row again and never used: every load of a chunk is unconditional, so
    // the compiler issues the chunk back to back and waits once (a branch around each load would wait for each)
    double cur[kCh][NCHAN], nxt[kCh][NCHAN];
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
        const int i = min(j, nt - 1);
        in(REV ? nt - 1 - i : i, nxt[j]);
    }
    for (int i0 = 0; i0 < nt; i0 += kCh) {
#pragma unroll
        for (int j = 0; j < kCh; ++j) {
#pragma unroll
            for (int q = 0; q < NCHAN; ++q) cur[j][q] = nxt[j][q];
        }
#pragma unroll
        for (int j = 0; j < kCh; ++j) {
            const int i = min(i0 + kCh + j, nt - 1);
            in(REV ? nt - 1 - i : i, nxt[j]);
        }
#pragma unroll
        for (int j = 0; j < kCh; ++j) {
            const int i = i0 + j;
            if (i < nt) {
                double y[NCHAN];
#pragma unroll
                for (int q = 0; q < NCHAN; ++q) {
                    double x = cur[j][q];
#pragma unroll
                    for (int k = 0; k < NSEC; ++k) {
                        const double v = c.b0[k] * x + s1[q][k];
                        s1[q][k] = c.b1[k] * x - c.a1[k] * v + s2[q][k];
                        s2[q][k] = c.b2[k] * x - c.a2[k] * v;
                        x = v;
                    }
                    y[q] = x;
                }
                out(REV ? nt - 1 - i : i, y);
            }
        }
    }
}

// y = F x (REV: F^T x); y == x allowed
template <int NSEC, bool REV>
__global__ __launch_bounds__(kLanes) void trace_filter(const Sos c, const float *x, float *y, int nt, long long ntrace)
{
    const long long tr = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (tr >= ntrace) return;
    sweep<NSEC, 1, REV>(c, nt, [&](int t, double *v) { v[0] = (double)x[(long long)t * ntrace + tr]; },
                        [&](int t, const double *v) { y[(long long)t * ntrace + tr] = (float)v[0]; });
}

#endif  // __HIPCC__

inline long long blocks(long long ntrace) { return (ntrace + kLanes - 1) / kLanes; }

// sizes as every misfit entry point rejects them; by_trace: the grid has one workgroup per kLanes traces
inline int check_sizes(int64_t nt, int64_t ntrace, bool by_trace = true)
{
    if (nt < 1 || ntrace < 1 || nt > 0x7fffffff)
        return mifwi::fail(MIFWI_EINVAL, "bad sizes nt=%lld ntrace=%lld", (long long)nt, (long long)ntrace);
    if (by_trace && blocks(ntrace) > 0x7fffffff) return mifwi::fail(MIFWI_EINVAL, "too many traces");
    return MIFWI_OK;
}

// sos: HOST [nsec][6] rows b0 b1 b2 a0 a1 a2 (scipy's order), a0 == 1
inline int check(int64_t nt, int64_t ntrace, const double *sos, int32_t nsec, Sos *c)
{
    if (int rc = check_sizes(nt, ntrace)) return rc;
    if (nsec < 1 || nsec > MIFWI_FILTER_MAX_SECTIONS)
        return mifwi::fail(MIFWI_EINVAL, "nsec=%d: a stage filter has 1 ... %d second-order sections", nsec,
                           (int)MIFWI_FILTER_MAX_SECTIONS);
    memset(c, 0, sizeof(*c));
    for (int k = 0; k < nsec; ++k) {
        const double *r = sos + 6 * k;
        for (int j = 0; j < 6; ++j)
            if (!std::isfinite(r[j])) return mifwi::fail(MIFWI_EINVAL, "section %d: coefficient %d is not finite", k, j);
        if (r[3] != 1.0) return mifwi::fail(MIFWI_EINVAL, "section %d: a0 = %g, must be 1 (normalise the section)", k, r[3]);
        c->b0[k] = r[0]; c->b1[k] = r[1]; c->b2[k] = r[2]; c->a1[k] = r[4]; c->a2[k] = r[5];
    }
    return MIFWI_OK;
}

}  // namespace mifwi_filter
