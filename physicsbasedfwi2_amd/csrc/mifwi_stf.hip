// Source-wavelet estimation (DENISE's INV_STF) in the time domain: the correlations of a finite-lag Wiener matching
// filter, and the convolution of traces with per-shot taps together with its exact transpose.  C-ABI: include/mifwi.h,
// "MATCHING FILTER"; the Toeplitz solve in between is host code (misfit.solve_matching_filter).
//
// Traces are [nt][nshot][nrec] float, time slowest: the fast axis is the trace.  Both kernels therefore put lanes along
// the receivers of ONE shot (a workgroup never mixes shots: per-shot taps, per-shot sums), stage (time chunk + lags) rows
// x 64 receivers in LDS with coalesced row loads, and walk time inside a thread with a register window, so that a staged
// value is read from LDS once per 4 multiply-adds instead of once per multiply-add.  With lanes along the receivers
// a wave reads 64 consecutive floats of a staged row: the 256-byte row pitch is conflict-free as it is; the one strided
// access - the sum over the 64 receivers of a tile, lane = lag - goes through a table padded to 65 doubles a row.
// Rows outside [0, nt) are staged as zeros: a term whose time index falls outside the record is absent, never wrapped.
#include "mifwi_common.h"

namespace {

constexpr int kStfLanes = 64;                       // receivers of a tile = one wave
constexpr int kStfGroups = 4;                       // waves of a workgroup
constexpr int kStfThreads = kStfLanes * kStfGroups;

// rows [row0, row0 + nrows) of column `col` -> tile[.][lane]; a dead lane (beyond nrec, or a killed trace) and a row
// outside the record give 0 without a read.  Wave g takes rows g, g + 4, ...
__device__ __forceinline__ void stf_stage(float *tile, const float *src, long long row0, int nrows, int nt, long long ntrace,
                                          long long col, bool live, int lane, int g)
{
    for (int q = g; q < nrows; q += kStfGroups) {
        const long long row = row0 + q;
        float v = 0.0f;
        if (live && row >= 0 && row < nt) v = src[row * ntrace + col];
        tile[q * kStfLanes + lane] = v;
    }
}

// ---- correlations ------------------------------------------------------------------------------------------------
// One sum covers both tables:  S[m] = sum_r w_r^2 sum_t b[t] x[t + off + m],  m = 0 .. nlag-1, x = pred,
//   auto   b = pred, off = 0,                     a[m] = S[m]
//   cross  b = obs,  off = lag_before - (nlag-1), c[nlag-1-m] = S[m]     (c[i] = sum d[t] x[t - (i - lag_before)])
// A workgroup owns (table, 64 lags, receiver tile, shot) and walks the whole record in chunks of kCorT samples; thread
// (lane, g) owns the 16 lags 16 g .. 16 g + 15 of its receiver in double registers (a product of two floats is exact in
// double).  Per 8 samples it reads 8 base values and a window of 23 moving values for 128 multiply-adds.  The sum over
// the receivers of the tile is taken once at the end, in lane order; the tiles are added in index order by stf_finish.
constexpr int kCorT = 64, kCorU = 16, kCorE = 8;
constexpr int kCorL = kStfGroups * kCorU;           // lags per workgroup
constexpr int kCorRows = kCorT + kCorL - 1;         // moving rows per chunk
constexpr int kRedPitch = kStfLanes + 1;            // doubles

__global__ __launch_bounds__(kStfThreads) void stf_correlate(const float *pred, const float *obs, const float *trace_w, int nt,
                                                             int nshot, int nrec, int lag_before, int nlag, double *partial)
{
    __shared__ __attribute__((aligned(16))) float sm[(kCorT + kCorRows) * kStfLanes];
    static_assert(sizeof(double) * kCorL * kRedPitch <= sizeof(float) * (kCorT + kCorRows) * kStfLanes, "the reduce table reuses the tiles");
    float *bt = sm, *mt = sm + kCorT * kStfLanes;
    const int lane = threadIdx.x & (kStfLanes - 1), g = threadIdx.x / kStfLanes;
    const int nchunk = (nlag + kCorL - 1) / kCorL;
    const bool cross = (int)blockIdx.x >= nchunk;
    const int m0 = ((int)blockIdx.x - (cross ? nchunk : 0)) * kCorL;
    const int tile = blockIdx.y, ntile = gridDim.y, s = blockIdx.z;
    const int rec = tile * kStfLanes + lane;
    const long long ntrace = (long long)nshot * nrec, col = (long long)s * nrec + rec;
    bool live = rec < nrec;
    float wv = 1.0f;
    if (live && trace_w) {
        wv = trace_w[col];
        live = wv != 0.0f;                          // a killed trace is not read
    }
    const float *base = cross ? obs : pred;
    const long long off = (cross ? (long long)lag_before - (nlag - 1) : 0) + m0;

    // the rows of the next chunk travel in registers while this one is summed (wave g owns rows g, g + 4, ...)
    constexpr int kNb = kCorT / kStfGroups, kNm = (kCorRows + kStfGroups - 1) / kStfGroups;
    float nb[kNb], nm[kNm];
    auto fetch = [&](long long t0) {
#pragma unroll
        for (int k = 0; k < kNb; ++k) {
            const long long row = t0 + g + kStfGroups * k;
            nb[k] = live && row < nt ? base[row * ntrace + col] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kNm; ++k) {
            const int q = g + kStfGroups * k;
            const long long row = t0 + off + q;
            nm[k] = live && q < kCorRows && row >= 0 && row < nt ? pred[row * ntrace + col] : 0.0f;
        }
    };
    double acc[kCorU];
#pragma unroll
    for (int u = 0; u < kCorU; ++u) acc[u] = 0.0;
    fetch(0);
    for (long long t0 = 0; t0 < nt; t0 += kCorT) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kNb; ++k) bt[(g + kStfGroups * k) * kStfLanes + lane] = nb[k];
#pragma unroll
        for (int k = 0; k < kNm; ++k)
            if (g + kStfGroups * k < kCorRows) mt[(g + kStfGroups * k) * kStfLanes + lane] = nm[k];
        __syncthreads();
        if (t0 + kCorT < nt) fetch(t0 + kCorT);
        for (int tt = 0; tt < kCorT; tt += kCorE) {
            double b[kCorE], w[kCorE + kCorU - 1];
#pragma unroll
            for (int e = 0; e < kCorE; ++e) b[e] = (double)bt[(tt + e) * kStfLanes + lane];
#pragma unroll
            for (int q = 0; q < kCorE + kCorU - 1; ++q) w[q] = (double)mt[(tt + g * kCorU + q) * kStfLanes + lane];
#pragma unroll
            for (int e = 0; e < kCorE; ++e)         // time ascending within every sum
#pragma unroll
                for (int u = 0; u < kCorU; ++u) acc[u] = fma(b[e], w[e + u], acc[u]);
        }
    }
    __syncthreads();
    double *red = reinterpret_cast<double *>(sm);   // [kCorL][kRedPitch]
    const double w2 = (double)wv * (double)wv;
#pragma unroll
    for (int u = 0; u < kCorU; ++u) red[(g * kCorU + u) * kRedPitch + lane] = trace_w ? acc[u] * w2 : acc[u];
    __syncthreads();
    const int m = m0 + (int)threadIdx.x;
    if ((int)threadIdx.x < kCorL && m < nlag) {
        double sum = 0.0;
        for (int l = 0; l < kStfLanes; ++l) sum += red[threadIdx.x * kRedPitch + l];
        const int idx = cross ? nlag - 1 - m : m;
        partial[(((long long)(cross ? nshot : 0) + s) * ntile + tile) * nlag + idx] = sum;
    }
}

// partial [2][nshot][ntile][nlag] -> auto_out, cross_out [nshot][nlag]: the receiver tiles added in index order
__global__ __launch_bounds__(256) void stf_finish(const double *partial, int nshot, int ntile, int nlag, double *auto_out,
                                                  double *cross_out)
{
    const long long n = (long long)nshot * nlag, e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * n) return;
    const long long which = e / n, r = e - which * n, s = r / nlag, i = r - s * nlag;
    const double *p = partial + ((which * nshot + s) * ntile) * nlag + i;
    double sum = 0.0;
    for (int k = 0; k < ntile; ++k) sum += p[(long long)k * nlag];
    (which ? cross_out : auto_out)[r] = sum;
}

// ---- convolution and its transpose -------------------------------------------------------------------------------
//   y[t] = sum_i h[i] x[t - k],  k = i - lag_before        TRANSPOSE: z[t] = sum_i h[i] x[t + k]
// the same sum with k -> -k, so one body serves both: only the staged row a (t, i) pair reads differs.  A workgroup owns
// (64 samples, receiver tile, shot); thread (lane, g) owns the 16 consecutive samples 16 g .. 16 g + 15 of its receiver
// and adds the lags in ascending i, 64 at a time: the taps of the chunk and the rows they reach are staged, and per 8
// lags a window of 23 rows serves 128 multiply-adds.  The order of the lags in a sum depends on nothing else, so a
// shot computed alone gives the bits of the whole call.
constexpr int kCvT = 64, kCvJ = 16, kCvU = 8, kCvL = 64;
constexpr int kCvW = kCvJ + kCvU - 1;

template <bool TRANSPOSE>
__global__ __launch_bounds__(kStfThreads) void trace_convolve(const float *x, float *y, const float *filt, int nt, int nshot,
                                                              int nrec, int lag_before, int nlag)
{
    __shared__ float xs[(kCvT + kCvL - 1) * kStfLanes];
    __shared__ float hs[kCvL];
    const int lane = threadIdx.x & (kStfLanes - 1), g = threadIdx.x / kStfLanes;
    const long long t0 = (long long)blockIdx.x * kCvT;
    const int tile = blockIdx.y, s = blockIdx.z;
    const int rec = tile * kStfLanes + lane;
    const bool live = rec < nrec;
    const long long ntrace = (long long)nshot * nrec, col = (long long)s * nrec + rec;

    float acc[kCvJ];
#pragma unroll
    for (int j = 0; j < kCvJ; ++j) acc[j] = 0.0f;
    for (int i0 = 0; i0 < nlag; i0 += kCvL) {
        const int nl = min(kCvL, nlag - i0);
        const int nl8 = (nl + kCvU - 1) / kCvU * kCvU;         // lags of this chunk, in whole groups of 8
        // staged row q of the chunk holds x[first + q]; sample t0 + a with lag i0 + b reads row
        //   TRANSPOSE: a + b        plain: a + (nl8 - 1) - b
        const long long first = TRANSPOSE ? t0 + i0 - lag_before : t0 + lag_before - i0 - (nl8 - 1);
        __syncthreads();
        if ((int)threadIdx.x < kCvL) hs[threadIdx.x] = (int)threadIdx.x < nl ? filt[(long long)s * nlag + i0 + threadIdx.x] : 0.0f;
        stf_stage(xs, x, first, kCvT + nl8 - 1, nt, ntrace, col, live, lane, g);
        __syncthreads();
        for (int ii = 0; ii < nl8; ii += kCvU) {
            const int w0 = g * kCvJ + (TRANSPOSE ? ii : nl8 - kCvU - ii);
            float w[kCvW];
#pragma unroll
            for (int q = 0; q < kCvW; ++q) w[q] = xs[(w0 + q) * kStfLanes + lane];
            const int nu = nl - ii;
#pragma unroll
            for (int u = 0; u < kCvU; ++u) {
                if (u < nu) {                       // uniform: the last group of a chunk may be short
                    const float hv = hs[ii + u];
#pragma unroll
                    for (int j = 0; j < kCvJ; ++j) acc[j] = fmaf(hv, w[TRANSPOSE ? j + u : j + kCvU - 1 - u], acc[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kCvJ; ++j) {
        const long long t = t0 + g * kCvJ + j;
        if (live && t < nt) y[t * ntrace + col] = acc[j];
    }
}

int stf_check(int64_t nt, int64_t nshot, int64_t nrec, int32_t lag_before, int32_t lag_after)
{
    if (nt < 1 || nshot < 1 || nrec < 1 || nt > 0x7fffffff || nrec > 0x7fffffff)
        return mifwi::fail(MIFWI_EINVAL, "bad sizes nt=%lld nshot=%lld nrec=%lld", (long long)nt, (long long)nshot, (long long)nrec);
    if (lag_before < 0 || lag_after < 0 || (int64_t)lag_before + lag_after + 1 > MIFWI_STF_MAX_LAGS)
        return mifwi::fail(MIFWI_EINVAL, "bad lags before=%d after=%d (both >= 0, before + after + 1 <= %d)", lag_before,
                           lag_after, (int)MIFWI_STF_MAX_LAGS);
    // shots and receiver tiles are the y and z axes of the launch grids
    if (nshot > 65535 || (nrec + kStfLanes - 1) / kStfLanes > 65535)
        return mifwi::fail(MIFWI_EINVAL, "too many shots (%lld > 65535) or receivers per shot (%lld > 65535 * 64)",
                           (long long)nshot, (long long)nrec);
    return MIFWI_OK;
}

}  // namespace

extern "C" {

int64_t mifwi_stf_correlate_work_elems(int64_t nt, int64_t nshot, int64_t nrec, int32_t lag_before, int32_t lag_after)
{
    if (nt < 1 || nshot < 1 || nrec < 1 || lag_before < 0 || lag_after < 0 ||
        (int64_t)lag_before + lag_after + 1 > MIFWI_STF_MAX_LAGS)
        return 0;
    const int64_t nlag = (int64_t)lag_before + lag_after + 1, ntile = (nrec + kStfLanes - 1) / kStfLanes;
    return mifwi::round_up64(2 * (2 * nshot * ntile * nlag), 64);          // doubles, counted in floats
}

int mifwi_stf_correlate(int device, const float *pred, const float *obs, const float *trace_w, int64_t nt, int64_t nshot,
                        int64_t nrec, int32_t lag_before, int32_t lag_after, double *auto_out, double *cross_out, float *work,
                        void *stream)
{
    if (!pred || !obs || !auto_out || !cross_out || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    int rc = stf_check(nt, nshot, nrec, lag_before, lag_after);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(work) & 7) != 0) return mifwi::fail(MIFWI_EINVAL, "work must be 8-byte aligned");
    rc = mifwi::check_device(device);
    if (rc) return rc;
    MIFWI_HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int nlag = lag_before + lag_after + 1, ntile = (int)((nrec + kStfLanes - 1) / kStfLanes);
    double *partial = reinterpret_cast<double *>(work);
    hipLaunchKernelGGL(stf_correlate, dim3(2 * ((nlag + kCorL - 1) / kCorL), ntile, (unsigned)nshot), dim3(kStfThreads), 0, st,
                       pred, obs, trace_w, (int)nt, (int)nshot, (int)nrec, lag_before, nlag, partial);
    hipLaunchKernelGGL(stf_finish, dim3((unsigned)((2 * nshot * nlag + 255) / 256)), dim3(256), 0, st, partial, (int)nshot,
                       ntile, nlag, auto_out, cross_out);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

int mifwi_trace_convolve(int device, const float *x, float *y, const float *filt, int64_t nt, int64_t nshot, int64_t nrec,
                         int32_t lag_before, int32_t lag_after, int32_t transpose, void *stream)
{
    if (!x || !y || !filt) return mifwi::fail(MIFWI_EINVAL, "null argument");
    if (x == y) return mifwi::fail(MIFWI_EINVAL, "y == x: the convolution does not run in place");
    int rc = stf_check(nt, nshot, nrec, lag_before, lag_after);
    if (rc) return rc;
    rc = mifwi::check_device(device);
    if (rc) return rc;
    MIFWI_HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int nlag = lag_before + lag_after + 1;
    const dim3 grid((unsigned)((nt + kCvT - 1) / kCvT), (unsigned)((nrec + kStfLanes - 1) / kStfLanes), (unsigned)nshot);
    if (transpose)
        hipLaunchKernelGGL(trace_convolve<true>, grid, dim3(kStfThreads), 0, st, x, y, filt, (int)nt, (int)nshot, (int)nrec,
                           lag_before, nlag);
    else
        hipLaunchKernelGGL(trace_convolve<false>, grid, dim3(kStfThreads), 0, st, x, y, filt, (int)nt, (int)nshot, (int)nrec,
                           lag_before, nlag);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // extern "C"
