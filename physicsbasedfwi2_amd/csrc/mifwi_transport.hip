// Optimal-transport objective: the quadratic Wasserstein distance between normalised traces (Engquist and Froese 2014;
// Yang et al. 2018) along time, trace by trace, and its exact adjoint source in one launch.  C-ABI: include/mifwi.h,
// "TRANSPORT MISFIT".
//
// Traces are [nt][ntrace] float, time slowest.  One workgroup per trace; thread t owns the C consecutive samples
// k = t C .. t C + C - 1 (C = 1, 2, 4, 8 or 16, the smallest power of two with 512 C >= nt; ceil(nt / C) threads rounded up
// to whole waves), so every running sum is a serial sum inside a chunk and one exclusive scan over the chunk totals.
// Everything past the float samples is double.
//
// Kept where (s modelled, o observed; u, p, P from s and v, q, Q from o as in the header):
//   LDS        Q_j and q_j of the observed trace, the only arrays that are read at positions other threads own (the
//              search), as two double arrays in a chunk-padded order: 16 T (C + 1) bytes, 136 KB at nt = 8192
//   registers  per own sample u_k (then p_k), the local sum (then P_k), sigmoid(b s_k), T_k - tau_k and a_k
// P is never stored: Pm_k is used by the thread that owns k alone.  Nothing is recomputed from global memory.
//
// Phases: (1) softplus of both chunks and their running sums; (2) exclusive scan of the chunk totals of v and of u (wave
// shuffles, then the wave totals in index order), which also gives V and U; (3) Q and q normalised into LDS, P and p in
// registers; (4) per own sample a branch-free lower-bound search of Pm_k in Q (the same number of steps for every sample,
// the C searches of a thread interleaved so that C LDS reads are in flight; a merge walk along Q measured no faster and
// its balance would be the data's), T_k - tau_k, the loss term and a_k; (5) the
// loss partial of the trace into partial[trace] - adj == NULL ends here, the same loss bits; (6) the suffix sums of a by the
// same scan run backwards; (7) g, its p-weighted mean, the adjoint source.
//
// T_k - tau_k is evaluated as (j - k) + (Pm_k - Qm_j) / q_j with Qm_j = Q_j - q_j / 2, the same expression that makes Pm_k
// from P_k and p_k: it equals j + (Pm_k - Q_{j-1}) / q_j - (k + 1/2) because Q_j - Q_{j-1} = q_j, and when pred holds the
// bits of obs, P, p and Q, q are the same bits (the same operations in the same order; the build has no contraction), the
// search finds j = k and the difference is an exact 0: loss and adjoint source are exact zeros, not rounding noise.
//
// Banks: a double at position c (C + 1) + i (chunk c, offset i; C = 1: position c).  A thread walks its own chunk in phases
// 1 and 3, so the 32 lanes of a half wave are (C + 1) doubles = 2 (C + 1) dwords apart; C + 1 is odd, so the 32 starts fall
// on 32 different even banks of the 64 (ds_read_b64 / ds_write_b64) and no access of these phases has a conflict, where
// unpadded chunks of 16 doubles would put all 32 lanes on one bank.  The search reads where the data send it and keeps
// its conflicts.
#include "mifwi_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kTrMaxThreads = 512;
constexpr int kTrMaxChunk = 16;
constexpr int kTrMaxWaves = kTrMaxThreads / 64;
constexpr int kTrLdsLimit = 16 * kTrMaxThreads * (kTrMaxChunk + 1);        // bytes, the largest image
static_assert(kTrMaxThreads * kTrMaxChunk == MIFWI_TRANSPORT_MAX_NT, "512 chunks of 16 samples are the longest record");

// Exclusive scan of one double per thread over the workgroup (REV: from the last thread down), and the sum of all.  Wave
// scan by shuffles, then the wave totals added in a fixed order: the same bits on every call.  blockDim.x is a multiple of
// 64; collective (two barriers), `wt` holds kTrMaxWaves doubles and is free again on return.
template <bool REV>
__device__ __forceinline__ double tr_scan(double x, double *total, double *wt, int tid, int T)
{
    const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    double incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = REV ? __shfl_down(incl, o) : __shfl_up(incl, o);
        if (REV ? lane + o < 64 : lane >= o) incl += y;
    }
    double excl = REV ? __shfl_down(incl, 1) : __shfl_up(incl, 1);
    if (lane == (REV ? 63 : 0)) excl = 0.0;
    if (lane == (REV ? 0 : 63)) wt[wave] = incl;
    __syncthreads();
    double base = 0.0, sum = 0.0;
    for (int i = 0; i < nw; ++i) {
        const int w = REV ? nw - 1 - i : i;
        const double v = wt[w];
        if (REV ? w > wave : w < wave) base += v;
        sum += v;
    }
    __syncthreads();
    *total = sum;
    return base + excl;
}

template <int C>
__device__ __forceinline__ int tr_pos(int k)
{
    return C == 1 ? k : (k / C) * (C + 1) + (k & (C - 1));
}

// exp(-|z|) serves both: softplus(z) = max(z, 0) + log1p(e), sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e)
__device__ __forceinline__ double tr_softplus(double z, double *sig)
{
    const double e = exp(-fabs(z));
    if (sig) *sig = (z >= 0.0 ? 1.0 : e) / (1.0 + e);
    return fmax(z, 0.0) + log1p(e);
}

template <int C>
__global__ __launch_bounds__(kTrMaxThreads) void tr_misfit(const float *pred, const float *obs, float *adj, double *partial, int nt,
                                                           long long ntrace, double b)
{
    extern __shared__ __attribute__((aligned(16))) double tr_lds[];
    __shared__ double wt[kTrMaxWaves];
    const int tid = threadIdx.x, T = blockDim.x;
    double *Qc = tr_lds, *qd = tr_lds + T * (C == 1 ? 1 : C + 1);
    const long long tr = blockIdx.x;
    const int k0 = tid * C, base = tr_pos<C>(k0);
    const int n = min(max(nt - k0, 0), C);                       // samples of this chunk inside the record

    // (1) the observed chunk into LDS (v and its running sum), the modelled one into registers
    float sf[C], of[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        sf[i] = i < n ? pred[(long long)(k0 + i) * ntrace + tr] : 0.0f;
        of[i] = i < n ? obs[(long long)(k0 + i) * ntrace + tr] : 0.0f;
    }
    double u[C], cu[C], sg[C];
    double runv = 0.0, runu = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const double v = i < n ? tr_softplus(b * (double)of[i], nullptr) : 0.0;
        runv += v;
        qd[base + i] = v;
        Qc[base + i] = runv;
        u[i] = i < n ? tr_softplus(b * (double)sf[i], &sg[i]) : 0.0;
        if (i >= n) sg[i] = 0.0;
        runu += u[i];
        cu[i] = runu;
    }
    // (2) the chunk totals across the workgroup
    double V, U;
    const double offv = tr_scan<false>(runv, &V, wt, tid, T);
    const double offu = tr_scan<false>(runu, &U, wt, tid, T);
    if (!(U != 0.0 && V != 0.0)) {                               // a trace without mass on either side contributes nothing
        if (tid == 0) partial[tr] = 0.0;
        if (adj)
            for (int i = 0; i < n; ++i) adj[(long long)(k0 + i) * ntrace + tr] = 0.0f;
        return;                                                  // the same for every thread of the workgroup
    }
    // (3) normalised: Q and q in LDS, P (in cu) and p (in u) in registers
    // (divisions, not products with 1 / V: v / V is exactly 1 for a one-sample trace, as in the definition)
#pragma unroll
    for (int i = 0; i < C; ++i) {
        Qc[base + i] = (offv + Qc[base + i]) / V;
        qd[base + i] = qd[base + i] / V;
        cu[i] = (offu + cu[i]) / U;
        u[i] = u[i] / U;
    }
    __syncthreads();
    // (4) j(k) = the first j with Q_j >= Pm_k, clamped to nt - 1: lower bound without a branch, nt > 1 steps alike for all
    double pm[C];
    int j[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        pm[i] = cu[i] - 0.5 * u[i];
        j[i] = 0;
    }
    for (int len = nt; len > 1; len -= len >> 1) {
        const int half = len >> 1;
#pragma unroll
        for (int i = 0; i < C; ++i) j[i] += Qc[tr_pos<C>(j[i] + half - 1)] < pm[i] ? half : 0;
    }
    double w = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        int jj = j[i];                                           // <= nt - 1
        jj = min(jj + (Qc[tr_pos<C>(jj)] < pm[i] ? 1 : 0), nt - 1);
        const double qj = qd[tr_pos<C>(jj)], qm = Qc[tr_pos<C>(jj)] - 0.5 * qj;
        double d = 0.0, a = 0.0;
        if (i < n && qj > 0.0) {                                 // a term whose divisor is 0 contributes 0
            d = (double)(jj - (k0 + i)) + (pm[i] - qm) / qj;     // T_k - tau_k
            a = 2.0 * u[i] * d / qj;
        }
        w += u[i] * d * d;
        pm[i] = d;
        cu[i] = a;
    }
    // (5) the trace's W
    double wsum;
    tr_scan<false>(w, &wsum, wt, tid, T);
    if (tid == 0) partial[tr] = wsum;
    if (!adj) return;
    // (6) sum_{k > m} a_k: inside the chunk from its end, then the chunks behind this one
    double runa = 0.0, suf[C];
#pragma unroll
    for (int i = C - 1; i >= 0; --i) {
        suf[i] = runa;
        runa += cu[i];
    }
    double unused;
    const double offa = tr_scan<true>(runa, &unused, wt, tid, T);
    // (7) g_m = (tau_m - T_m)^2 + a_m / 2 + sum_{k > m} a_k, its mean under p, the chain rule through softplus
    double gp = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        suf[i] = pm[i] * pm[i] + 0.5 * cu[i] + (offa + suf[i]);
        gp += suf[i] * u[i];
    }
    double G;
    tr_scan<false>(gp, &G, wt, tid, T);
#pragma unroll
    for (int i = 0; i < C; ++i)
        if (i < n) adj[(long long)(k0 + i) * ntrace + tr] = (float)(0.5 * (suf[i] - G) / U * b * sg[i]);
}

// loss = 1/2 sum of the trace partials: thread i adds partials i, i + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void tr_finish(const double *partial, long long ntrace, float *loss)
{
    __shared__ double red[256];
    double sum = 0.0;
    for (long long i = threadIdx.x; i < ntrace; i += 256) sum += partial[i];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(0.5 * red[0]);
}

int tr_sizes(int64_t nt, int64_t ntrace)
{
    if (nt < 1 || ntrace < 1) return mifwi::fail(MIFWI_EINVAL, "bad sizes nt=%lld ntrace=%lld", (long long)nt, (long long)ntrace);
    if (nt > MIFWI_TRANSPORT_MAX_NT)
        return mifwi::fail(MIFWI_EINVAL, "nt=%lld: the distribution functions of a trace live in one workgroup's LDS and take records "
                                         "of up to %d samples; longer records are not supported", (long long)nt,
                           (int)MIFWI_TRANSPORT_MAX_NT);
    if (ntrace > 0x7fffffff) return mifwi::fail(MIFWI_EINVAL, "ntrace=%lld is beyond the launch grid (2^31 - 1)", (long long)ntrace);
    return MIFWI_OK;
}

}  // namespace

extern "C" {

int64_t mifwi_misfit_transport_work_elems(int64_t nt, int64_t ntrace)
{
    if (nt < 1 || ntrace < 1 || nt > MIFWI_TRANSPORT_MAX_NT) return 0;
    return mifwi::round_up64(2 * ntrace, 64);                    // one double per trace, counted in floats
}

int mifwi_misfit_transport(int device, const float *pred, const float *obs, int64_t nt, int64_t ntrace, double b, float *loss_out,
                           float *adj_out, float *work, void *stream)
{
    if (!pred || !obs || !loss_out || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    int rc = tr_sizes(nt, ntrace);
    if (rc) return rc;
    if (!(b > 0.0) || std::isinf(b)) return mifwi::fail(MIFWI_EINVAL, "b=%g: the softplus scale must be finite and > 0", b);
    if ((reinterpret_cast<uintptr_t>(work) & 7) != 0) return mifwi::fail(MIFWI_EINVAL, "work must be 8-byte aligned");
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;
    int chunk = 1;
    while ((int64_t)kTrMaxThreads * chunk < nt) chunk <<= 1;     // <= kTrMaxChunk, see the static_assert
    const int threads = mifwi::ceil_div(mifwi::ceil_div((int)nt, chunk), 64) * 64;
    const size_t lds = sizeof(double) * 2 * (size_t)threads * (chunk == 1 ? 1 : chunk + 1);
    double *partial = reinterpret_cast<double *>(work);
    rc = mifwi::with_int<1, 2, 4, 8, 16>(chunk, [&](auto c) -> int {
        auto kernel = tr_misfit<decltype(c)::value>;
        if (lds > 48 * 1024)
            MIFWI_HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kTrLdsLimit));
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntrace), dim3(threads), lds, st, pred, obs, adj_out, partial, (int)nt,
                           (long long)ntrace, b);
        return MIFWI_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(tr_finish, dim3(1), dim3(256), 0, st, partial, (long long)ntrace, loss_out);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // extern "C"
