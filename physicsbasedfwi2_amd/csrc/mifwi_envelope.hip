// Envelope objective (DENISE's lnorm = 6, Chi, Dong and Liu 2014): the Hilbert transform along time as a power-of-two
// padded DFT held in LDS, the envelope residual and its exact adjoint source in one launch.  C-ABI: include/mifwi.h,
// "ENVELOPE MISFIT".
//
// Traces are [nt][ntrace] float, time slowest.  N = the smallest power of two >= nt, M = N / 2.
//
// The transform of a REAL trace of N samples is an M-point complex FFT of z[n] = x[2n] + i x[2n+1]: a radix-2
// decimation-in-frequency forward transform (natural order in, bit-reversed out), one pointwise pass over the pairs of
// bins (k, M - k) that untangles the spectrum of x from that of z, applies the Hilbert multiplier and tangles the
// product back, and a radix-2 decimation-in-time inverse (bit-reversed in, natural out), so nothing is ever permuted.
// With X[k] the spectrum of x, A = Z[k], B = Z[M-k], w = exp(-2 pi i k / N):
//     E = A + conj(B),  O = -i (A - conj(B))            X[k] = (E + w O) / 2,  X[M-k] = conj(E - w O) / 2
//     P = w O,  Q = conj(w) E                           Z'[k] = sigma (Q - i P),  Z'[M-k] = -sigma conj(Q + i P)
// is the tangled form of Y[k] = -i sigma X[k] (0 < k < M), Y[0] = Y[M] = 0; sigma = -1 gives H^T = -H, the same
// operations with every sign turned, so the transposed transform is the negated one bit for bit.  The factors 1/2 and
// the 1/M of the inverse are one multiplication by 1/N (exact) when a sample leaves LDS.
// A trace is never packed with another signal into one complex transform: that would halve the work again, but the
// complex twiddle products round the two parts into each other, so an all-zero trace next to a live one would no longer
// transform to exact zeros and with eps = 0 its adjoint source would be rounding noise times 1 / E.  Here an all-zero
// trace gives exact zeros and the error of H x scales with |x| alone.
//
// LDS (dynamic, 16 N bytes: 128 KB at N = 8192): two traces [re M][im M] each, then the twiddles [re N][im N]:
//   index h + j, j < h, h = 1, 2, .. M/2:   exp(-2 pi i j / (2 h)), the table of the pass with half-size h, contiguous
//   index M + k, k < M:                     exp(-2 pi i k / N), for the untangling pass
// The base table comes from double sincospi, rounded once to float; the pass tables are copies of its entries.
// Banks: re and im are separate float arrays (ds_read_b32 / ds_write_b32: 32 banks, conflicts within a 32-lane half).  A
// butterfly pass with half-size h >= 32 reads 32 consecutive floats per half wave; with h < 32 the 32 lanes read the
// 32 elements of a 64-element span whose bit log2(h) is clear (or set), 16 from each 32-element block, on the same 16
// banks twice.  The index is therefore swizzled: every odd 32-element block is stored in reverse, sw(i) = i ^ 31 there,
// which maps the second block's 16 elements onto the other 16 banks for every h < 32 and leaves a 32-consecutive access
// a permutation of one block: no pass has a bank conflict.  The pass tables are read at h + j: consecutive (or broadcast).
// The untangling pass reads bit-reversed positions, one pass in 2 log2 M, conflicts accepted.
#include "mifwi_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kEnvMaxThreads = 512;
constexpr int kEnvLdsLimit = 16 * MIFWI_ENVELOPE_MAX_NT;      // bytes, the largest image

__device__ __forceinline__ int env_sw(int i) { return i ^ (-((i >> 5) & 1) & 31); }

// tw = [re N][im N]; collective over the workgroup.  N >= 2.
__device__ __forceinline__ void env_twiddles(float *twr, float *twi, int N, int tid, int T)
{
    const int M = N >> 1;
    for (int k = tid; k < M; k += T) {
        double s, c;
        sincospi(-2.0 * (double)k / (double)N, &s, &c);
        twr[M + k] = (float)c;
        twi[M + k] = (float)s;
    }
    __syncthreads();
    for (int idx = tid + 1; idx < M; idx += T) {
        const int h = 1 << (31 - __clz(idx)), j = idx - h;
        const int src = M + j * (M / h);
        twr[idx] = twr[src];
        twi[idx] = twi[src];
    }
    __syncthreads();
}

// In place on NB traces at data + b * 2 M ([re M][im M], swizzled, z[n] = x[2n] + i x[2n+1]): x -> N sigma H x.
// Collective over the workgroup; the caller has synchronised after filling the traces, and the result is visible to
// every thread on return.
template <int NB>
__device__ __forceinline__ void env_hilbert(float *data, const float *twr, const float *twi, int M, int logM, float sigma, int tid,
                                            int T)
{
    if (M < 2) {                                                 // N <= 2: bins 0 and N/2 are all there is, H = 0
        if (tid < 2 * M * NB) data[tid] = 0.0f;
        __syncthreads();
        return;
    }
    const int nb = M >> 1;
    for (int h = nb; h >= 1; h >>= 1) {
        for (int b = tid; b < nb; b += T) {
            const int j = b & (h - 1), lo = ((b - j) << 1) + j;
            const int i0 = env_sw(lo), i1 = env_sw(lo + h);
            const float wr = twr[h + j], wi = twi[h + j];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                float *re = data + q * 2 * M, *im = re + M;
                const float ur = re[i0], ui = im[i0], vr = re[i1], vi = im[i1];
                const float dr = ur - vr, di = ui - vi;
                re[i0] = ur + vr;
                im[i0] = ui + vi;
                re[i1] = dr * wr - di * wi;
                im[i1] = dr * wi + di * wr;
            }
        }
        __syncthreads();
    }
    for (int k = tid; k <= nb; k += T) {
        if (k == 0) {
#pragma unroll
            for (int q = 0; q < NB; ++q) data[q * 2 * M] = data[q * 2 * M + M] = 0.0f;          // env_sw(0) == 0
            continue;
        }
        const int p = env_sw((int)(__brev((unsigned)k) >> (32 - logM)));
        const int m = env_sw((int)(__brev((unsigned)(M - k)) >> (32 - logM)));
        const float c = twr[M + k], s = twi[M + k];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            float *re = data + q * 2 * M, *im = re + M;
            const float ar = re[p], ai = im[p], br = re[m], bi = im[m];
            const float er = ar + br, ei = ai - bi, orr = ai + bi, oi = br - ar;
            const float pr = c * orr - s * oi, pi = c * oi + s * orr;
            const float qr = c * er + s * ei, qi = c * ei - s * er;
            re[p] = sigma * (qr + pi);
            im[p] = sigma * (qi - pr);
            if (m != p) {                                        // k == M/2 pairs with itself: both forms agree
                re[m] = sigma * (pi - qr);
                im[m] = sigma * (qi + pr);
            }
        }
    }
    __syncthreads();
    for (int h = 1; h <= nb; h <<= 1) {
        for (int b = tid; b < nb; b += T) {
            const int j = b & (h - 1), lo = ((b - j) << 1) + j;
            const int i0 = env_sw(lo), i1 = env_sw(lo + h);
            const float wr = twr[h + j], wi = twi[h + j];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                float *re = data + q * 2 * M, *im = re + M;
                const float ur = re[i0], ui = im[i0], xr = re[i1], xi = im[i1];
                const float vr = xr * wr + xi * wi, vi = xi * wr - xr * wi;
                re[i0] = ur + vr;
                im[i0] = ui + vi;
                re[i1] = ur - vr;
                im[i1] = ui - vi;
            }
        }
        __syncthreads();
    }
}

// One workgroup per pair of neighbouring traces (the last one of an odd count transforms a zero trace next to it).
__global__ __launch_bounds__(kEnvMaxThreads) void env_trace_hilbert(const float *x, float *y, int nt, long long ntrace, int N,
                                                                    int logM, float sigma)
{
    extern __shared__ __attribute__((aligned(16))) float env_lds[];
    const int M = N > 1 ? N >> 1 : 1, tid = threadIdx.x, T = blockDim.x;
    float *data = env_lds, *twr = env_lds + 4 * M, *twi = twr + N;
    const long long tr0 = 2ll * blockIdx.x;
    const int ntr = tr0 + 1 < ntrace ? 2 : 1;
    if (N >= 4) env_twiddles(twr, twi, N, tid, T);
    for (int n = tid; n < M; n += T) {
        const int t = 2 * n, i = env_sw(n);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float *re = data + q * 2 * M, *im = re + M;
            re[i] = q < ntr && t < nt ? x[(long long)t * ntrace + tr0 + q] : 0.0f;
            im[i] = q < ntr && t + 1 < nt ? x[(long long)(t + 1) * ntrace + tr0 + q] : 0.0f;
        }
    }
    __syncthreads();                                             // y == x: the traces are in LDS before one is written
    env_hilbert<2>(data, twr, twi, M, logM, sigma, tid, T);
    const float inv = 1.0f / (float)N;
    for (int n = tid; n < M; n += T) {
        const int t = 2 * n, i = env_sw(n);
        for (int q = 0; q < ntr; ++q) {
            const float *re = data + q * 2 * M, *im = re + M;
            if (t < nt) y[(long long)t * ntrace + tr0 + q] = re[i] * inv;
            if (t + 1 < nt) y[(long long)(t + 1) * ntrace + tr0 + q] = im[i] * inv;
        }
    }
}

// One workgroup per trace.  Phases: twiddles; s = pred and o = obs into the two LDS traces; both Hilbert transforms in
// the same passes; per sample, in double, E(s), E(o), r, the loss term, a = r s / E(s) into the second trace and
// q = r H s / E(s) into the first; the loss partial of the trace (threads in index order through a fixed tree) into
// partial[trace]; the Hilbert transform of q; adj = a - H q.  adj == NULL ends after the partial: the same loss bits.
__global__ __launch_bounds__(kEnvMaxThreads) void env_misfit(const float *pred, const float *obs, float *adj, double *partial,
                                                             int nt, long long ntrace, int N, int logM, double eps2)
{
    extern __shared__ __attribute__((aligned(16))) float env_lds[];
    __shared__ double red[kEnvMaxThreads];
    const int M = N > 1 ? N >> 1 : 1, tid = threadIdx.x, T = blockDim.x;
    float *data = env_lds, *twr = env_lds + 4 * M, *twi = twr + N;
    float *re0 = data, *im0 = data + M, *re1 = data + 2 * M, *im1 = data + 3 * M;
    const long long tr = blockIdx.x;
    if (N >= 4) env_twiddles(twr, twi, N, tid, T);
    for (int n = tid; n < M; n += T) {
        const int t = 2 * n, i = env_sw(n);
        re0[i] = t < nt ? pred[(long long)t * ntrace + tr] : 0.0f;
        im0[i] = t + 1 < nt ? pred[(long long)(t + 1) * ntrace + tr] : 0.0f;
        re1[i] = t < nt ? obs[(long long)t * ntrace + tr] : 0.0f;
        im1[i] = t + 1 < nt ? obs[(long long)(t + 1) * ntrace + tr] : 0.0f;
    }
    __syncthreads();
    env_hilbert<2>(data, twr, twi, M, logM, 1.0f, tid, T);
    const float inv = 1.0f / (float)N;
    double sum = 0.0;
    for (int n = tid; n < M; n += T) {
        const int i = env_sw(n);
        float a[2] = {0.0f, 0.0f}, q[2] = {0.0f, 0.0f};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int t = 2 * n + e;
            if (t >= nt) continue;                               // the padding stays zero
            const double s = (double)pred[(long long)t * ntrace + tr], o = (double)obs[(long long)t * ntrace + tr];
            const double hs = (double)((e ? im0 : re0)[i] * inv), ho = (double)((e ? im1 : re1)[i] * inv);
            const double es = sqrt(s * s + hs * hs + eps2), eo = sqrt(o * o + ho * ho + eps2);
            const double r = es - eo;
            sum += r * r;
            if (es > 0.0) {                                      // a term whose divisor is 0 contributes 0
                a[e] = (float)(r * s / es);
                q[e] = (float)(r * hs / es);
            }
        }
        re0[i] = q[0];
        im0[i] = q[1];
        re1[i] = a[0];
        im1[i] = a[1];
    }
    red[tid] = sum;
    __syncthreads();
    for (int w = kEnvMaxThreads / 2; w >= 1; w >>= 1) {
        if (tid < w && tid + w < T) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[tr] = red[0];
    if (!adj) return;
    env_hilbert<1>(data, twr, twi, M, logM, 1.0f, tid, T);
    for (int n = tid; n < M; n += T) {
        const int t = 2 * n, i = env_sw(n);
        if (t < nt) adj[(long long)t * ntrace + tr] = re1[i] - re0[i] * inv;
        if (t + 1 < nt) adj[(long long)(t + 1) * ntrace + tr] = im1[i] - im0[i] * inv;
    }
}

// loss = 1/2 sum of the trace partials: thread i adds partials i, i + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void env_finish(const double *partial, long long ntrace, float *loss)
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

struct EnvShape {
    int N, logM, threads;
    size_t lds;
};

int env_shape(int64_t nt, int64_t ntrace, EnvShape *sh)
{
    if (nt < 1 || ntrace < 1) return mifwi::fail(MIFWI_EINVAL, "bad sizes nt=%lld ntrace=%lld", (long long)nt, (long long)ntrace);
    if (nt > MIFWI_ENVELOPE_MAX_NT)
        return mifwi::fail(MIFWI_EINVAL, "nt=%lld: the Hilbert transform of a trace runs inside one workgroup's LDS and takes records "
                                         "of up to %d samples; longer records are not supported", (long long)nt,
                           (int)MIFWI_ENVELOPE_MAX_NT);
    if (ntrace > 0x7fffffff) return mifwi::fail(MIFWI_EINVAL, "ntrace=%lld is beyond the launch grid (2^31 - 1)", (long long)ntrace);
    int N = 1, logN = 0;
    while (N < nt) { N <<= 1; ++logN; }
    sh->N = N;
    sh->logM = logN > 0 ? logN - 1 : 0;
    sh->threads = std::min(kEnvMaxThreads, std::max(64, N / 4));  // a pass has N / 4 butterflies
    sh->lds = sizeof(float) * 4 * (size_t)std::max(N, 2);
    return MIFWI_OK;
}

template <class K>
int env_raise_lds(K kernel, size_t lds)
{
    if (lds > 48 * 1024) MIFWI_HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kEnvLdsLimit));
    return MIFWI_OK;
}

}  // namespace

extern "C" {

int mifwi_trace_hilbert(int device, const float *x, float *y, int64_t nt, int64_t ntrace, int32_t transpose, void *stream)
{
    if (!x || !y) return mifwi::fail(MIFWI_EINVAL, "null argument");
    EnvShape sh;
    int rc = env_shape(nt, ntrace, &sh);
    if (rc) return rc;
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;
    rc = env_raise_lds(env_trace_hilbert, sh.lds);
    if (rc) return rc;
    hipLaunchKernelGGL(env_trace_hilbert, dim3((unsigned)((ntrace + 1) / 2)), dim3(sh.threads), sh.lds, st, x, y, (int)nt,
                       (long long)ntrace, sh.N, sh.logM, transpose ? -1.0f : 1.0f);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

int64_t mifwi_misfit_envelope_work_elems(int64_t nt, int64_t ntrace)
{
    if (nt < 1 || ntrace < 1 || nt > MIFWI_ENVELOPE_MAX_NT) return 0;
    return mifwi::round_up64(2 * ntrace, 64);                    // one double per trace, counted in floats
}

int mifwi_misfit_envelope(int device, const float *pred, const float *obs, int64_t nt, int64_t ntrace, double eps,
                          float *loss_out, float *adj_out, float *work, void *stream)
{
    if (!pred || !obs || !loss_out || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    EnvShape sh;
    int rc = env_shape(nt, ntrace, &sh);
    if (rc) return rc;
    if (!(eps >= 0.0) || std::isinf(eps)) return mifwi::fail(MIFWI_EINVAL, "eps=%g: the regularisation must be finite and >= 0", eps);
    if ((reinterpret_cast<uintptr_t>(work) & 7) != 0) return mifwi::fail(MIFWI_EINVAL, "work must be 8-byte aligned");
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;
    rc = env_raise_lds(env_misfit, sh.lds);
    if (rc) return rc;
    double *partial = reinterpret_cast<double *>(work);
    hipLaunchKernelGGL(env_misfit, dim3((unsigned)ntrace), dim3(sh.threads), sh.lds, st, pred, obs, adj_out, partial, (int)nt,
                       (long long)ntrace, sh.N, sh.logM, eps * eps);
    hipLaunchKernelGGL(env_finish, dim3(1), dim3(256), 0, st, partial, (long long)ntrace, loss_out);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // extern "C"
