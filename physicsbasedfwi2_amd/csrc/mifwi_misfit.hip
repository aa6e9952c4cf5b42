// Fused data misfit + adjoint source (libmifwi, gfx950).
//
// Replaces the O(data) torch expressions between the propagator call and .backward() in the
// reference's prop() methods:
//   kind L1_TRACE_NORM  models/networks.py:5418-5419 (observed side), 5467-5476 (predicted side):
//       d = pred - direct;  m = max_t |d|;  dn = d / (m + 1e-10);  loss = mean |dn - obs|
//       adj = dloss/dpred (what autograd's backward of those lines delivers to the propagator)
//   kind L2             seisgan/fwi/layers.py:176-178 and DENISE lnorm=2 (networks.py:7758):
//       loss = 1/2 sum (pred - obs)^2;  adj = pred - obs
//   kind GLOBAL_CORRELATION  (DENISE's global-correlation norm, the `lnorm` argument of add_fwi_stage at
//       models/networks.py:9863, 10503; Choi & Alkhalifah 2012): per trace s = pred, o = obs
//       loss = - sum_traces <s, o> / (|s| |o|);  adj = -(o/|o| - <s,o>/(|s||o|) s/|s|) / |s|
//       (a trace with |s| = 0 or |o| = 0 contributes nothing)
// Layout [nt][ntrace] (trace = shot*nrec + receiver fastest), i.e. the propagators' own output.
//
// L2 and GLOBAL_CORRELATION also run on the traces of a frequency stage and of a trace selection, in ONE launch: F the
// stage filter (mifwi_misfit_filter.h), W the selection (mifwi_misfit_select.h), either absent or both,
//     L2                  r = float(W F(pred - obs));  loss = 1/2 sum r^2;  adj = float(F^T W r)
//     GLOBAL_CORRELATION  s = float(W F pred), o = float(W F obs);  loss = -sum_traces <s,o>/(|s||o|);
//                         adj = float(F^T W (ka o + kb s))
// Each objective has one kernel body per grid, W in it as the SELECT instances (the others hold no trace of W):
//     with a stage   misfit_staged_l2<NSEC, W...>, misfit_staged_gc<NSEC, W...>      one lane per trace, one wave
//     without        misfit_gc<W...>, misfit_selected_l2_plain, misfit_l1_trace_norm  64 traces x 16 time slices
//                    misfit_l2<VEC> (no F, no W: every sample on its own)             flat
//
// One workgroup = 64 neighbouring traces x 16 interleaved time slices: every wave reads whole
// 256-byte rows, traces never leave their lane, the 16 slices of a trace meet twice in LDS
// (max/argmax, then the sum the max's gradient needs).  HBM-bound: pred/direct are read twice,
// obs once, adj written once = 28 B per sample (20 without a direct wave).
#include "mifwi_common.h"

#include "mifwi_misfit_filter.h"
#include "mifwi_misfit_select.h"

namespace {

using mifwi_filter::kLanes;                // traces per workgroup
using mifwi_filter::Sos;
using mifwi_filter::sweep;
using mifwi_select::kSl;                   // time slices per workgroup of the kernels without a stage (1024 threads)
using mifwi_select::pick;
using mifwi_select::Sel;
using mifwi_select::Trace;
using mifwi_select::TraceOf;
constexpr float kEps = 1e-10f;

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// workgroup sum of the 64 x 16 kernels in a fixed order: the lanes of a wave, then the 16 waves
__device__ __forceinline__ void block_sum(double v, double *s_loss, int lane, int sl, double *partial)
{
    v = wave_sum(v);
    if (lane == 0) s_loss[sl] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < kSl; ++k) tot += s_loss[k];
        partial[blockIdx.x] = tot;
    }
}

template <bool DIRECT>
__global__ __launch_bounds__(kLanes *kSl) void misfit_l1_trace_norm(const float *pred, const float *obs,
                                                                    const float *direct, int nt, long long ntrace,
                                                                    float inv_n, float *adj, double *partial)
{
    __shared__ float s_max[kSl][kLanes];
    __shared__ int s_arg[kSl][kLanes];
    __shared__ float s_c[kSl][kLanes];
    __shared__ double s_loss[kSl];
    const int lane = (int)threadIdx.x % kLanes, sl = (int)threadIdx.x / kLanes;
    const long long tr = (long long)blockIdx.x * kLanes + lane;
    const bool live = tr < ntrace;
    // ---- pass 1: max |d| and the first time it is reached --------------------------------------
    float m = -1.f;
    int arg = 0;
    if (live)
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            const float d = DIRECT ? pred[o] - direct[o] : pred[o];
            const float a = fabsf(d);
            if (a > m) { m = a; arg = t; }
        }
    s_max[sl][lane] = m; s_arg[sl][lane] = arg;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSl; ++k) {
        const float mk = s_max[k][lane];
        const int ak = s_arg[k][lane];
        if (mk > m || (mk == m && ak < arg)) { m = mk; arg = ak; }
    }
    const float inv = 1.0f / (m + kEps);
    // ---- pass 2: residual sign, loss, adj without the max's own gradient ----------------------
    float c = 0.f;
    double loss = 0.0;
    if (live)
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            const float d = DIRECT ? pred[o] - direct[o] : pred[o];
            const float r = d * inv - obs[o];
            const float a = sgn(r) * inv_n;
            loss += (double)fabsf(r);
            c = fmaf(a, d, c);
            if (adj) adj[o] = a * inv;
        }
    s_c[sl][lane] = c;
    block_sum(loss, s_loss, lane, sl, partial);          // its barrier publishes s_c as well
    // ---- the max feeds every sample of its trace: d(dn_t)/d(d_t*) = -d_t sign(d_t*) / (m+eps)^2 --
    if (live && adj && sl == arg % kSl) {
        float ctot = 0.f;
#pragma unroll
        for (int k = 0; k < kSl; ++k) ctot += s_c[k][lane];
        const long long o = (long long)arg * ntrace + tr;
        const float d = DIRECT ? pred[o] - direct[o] : pred[o];
        adj[o] = adj[o] - sgn(d) * ctot * inv * inv;
    }
}

// global correlation without a stage: pass 1 the three inner products of a trace (fp64, fixed order), pass 2 the adjoint
// source.  W... = Sel (SELECT): of W pred, W obs; a killed trace is never read.  Where the body asks for SELECT by name
// (here and in misfit_staged_gc) the two instances differ in which loads and sums they issue and in what order, not in
// what they compute from finite data: each keeps the device code it was measured with.
template <class... W>
__global__ __launch_bounds__(kLanes *kSl) void misfit_gc(const W... sel, const float *pred, const float *obs, int nt,
                                                         long long ntrace, float *adj, double *partial)
{
    constexpr bool SELECT = sizeof...(W) != 0;
    __shared__ double s_ss[kSl][kLanes], s_oo[kSl][kLanes], s_so[kSl][kLanes];
    __shared__ double s_loss[kSl];
    const int lane = (int)threadIdx.x % kLanes, sl = (int)threadIdx.x / kLanes;
    const long long tr = (long long)blockIdx.x * kLanes + lane;
    const bool inside = tr < ntrace;
    const TraceOf<W...> s(sel..., tr, inside);
    const bool live = SELECT ? s.live() : inside;
    // s, o of sample t as the sums see them: rounded to float after W
    auto sample = [&](int t, long long o, double &a, double &b) {
        const auto w = s.w(t);
        a = (double)(float)pick(w, (double)pred[o]); b = (double)(float)pick(w, (double)obs[o]);
        return w;
    };
    double ss = 0.0, oo = 0.0, so = 0.0;
    if (live)
        for (int t = sl; t < nt; t += kSl) {
            double a, b;
            sample(t, (long long)t * ntrace + tr, a, b);
            ss += a * a; oo += b * b; so += a * b;
        }
    s_ss[sl][lane] = ss; s_oo[sl][lane] = oo; s_so[sl][lane] = so;
    __syncthreads();
    ss = oo = so = 0.0;
#pragma unroll
    for (int k = 0; k < kSl; ++k) { ss += s_ss[k][lane]; oo += s_oo[k][lane]; so += s_so[k][lane]; }
    const bool ok = live && ss > 0.0 && oo > 0.0;
    const double ns = sqrt(ss), no = sqrt(oo);
    const double cc = ok ? so / (ns * no) : 0.0;
    if (adj && inside) {
        // in double: on a weak trace the two coefficients overflow a float long before their combination does
        const double ka = ok ? -1.0 / (ns * no) : 0.0;               // coefficient of o
        const double kb = ok ? cc / ss : 0.0;                        // coefficient of s
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            float g = 0.f;
            if constexpr (SELECT) {
                if (ok) {
                    double a, b;
                    const auto w = sample(t, o, a, b);
                    g = (float)pick(w, ka * b + kb * a);
                }
            } else {                                                 // a trace without energy gets 0 * its samples
                g = (float)(ka * (double)obs[o] + kb * (double)pred[o]);
            }
            adj[o] = g;
        }
    }
    double loss = sl == 0 ? -cc : 0.0;                                  // one slice speaks for the trace
    if constexpr (SELECT) {
        block_sum(loss, s_loss, lane, sl, partial);
    } else {                                                            // the other fifteen slots hold zeros
        for (int off = 32; off > 0; off >>= 1) loss += __shfl_down(loss, off, 64);
        if (lane == 0) s_loss[sl] = loss;
        __syncthreads();
        if (threadIdx.x == 0) partial[blockIdx.x] = s_loss[0];
    }
}

// L2 of W (pred - obs) without a stage (without W as well: misfit_l2); a killed trace is never read
__global__ __launch_bounds__(kLanes *kSl) void misfit_selected_l2_plain(const Sel sel, const float *pred, const float *obs,
                                                                        int nt, long long ntrace, float *adj, double *partial)
{
    __shared__ double s_loss[kSl];
    const int lane = (int)threadIdx.x % kLanes, sl = (int)threadIdx.x / kLanes;
    const long long tr = (long long)blockIdx.x * kLanes + lane;
    const bool inside = tr < ntrace;
    const Trace s(sel, tr, inside);
    double loss = 0.0;
    if (inside)
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            float g = 0.f;
            if (s.live()) {
                const double w = s.w(t);
                const float r = (float)pick(w, (double)pred[o] - (double)obs[o]);
                loss += (double)r * (double)r;
                g = (float)pick(w, (double)r);
            }
            if (adj) adj[o] = g;
        }
    block_sum(loss, s_loss, lane, sl, partial);
}

// ---- with a stage: mifwi_filter::sweep, one lane per trace, one wave per workgroup --------------------------------
// W... = Sel (SELECT): W after the forward sweep, W again before the reverse one.  A killed lane among live ones runs the
// recurrence on zeros - its rows are requested like the others' (every load of a chunk stays unconditional) and dropped -
// and a wave without a live trace runs no sweep and writes zeros.
template <int NSEC, class... W>
__global__ __launch_bounds__(kLanes) void misfit_staged_l2(const Sos c, const W... sel, const float *pred, const float *obs,
                                                           int nt, long long ntrace, float *adj, double *partial)
{
    constexpr bool SELECT = sizeof...(W) != 0;
    const long long tr = (long long)blockIdx.x * kLanes + threadIdx.x;
    const bool inside = tr < ntrace;
    const TraceOf<W...> s(sel..., tr, inside);
    const bool live = s.live();
    double loss = 0.0;
    if (!SELECT || __any(live)) {
        if (inside) {
            // forward: r = W F(pred - obs), rounded to float where it is stored AND where it is summed
            sweep<NSEC, 1, false>(c, nt,
                                  [&](int t, double *v) {
                                      const long long o = (long long)t * ntrace + tr;
                                      const double x = (double)pred[o] - (double)obs[o];
                                      v[0] = live ? x : 0.0;
                                  },
                                  [&](int t, const double *v) {
                                      const float r = (float)pick(s.w(t), v[0]);
                                      loss += (double)r * (double)r;
                                      if (adj) adj[(long long)t * ntrace + tr] = r;
                                  });
            // backward: adj <- F^T W r in place (a lane only ever touches its own column)
            if (adj)
                sweep<NSEC, 1, true>(c, nt,
                                     [&](int t, double *v) { v[0] = pick(s.w(t), (double)adj[(long long)t * ntrace + tr]); },
                                     [&](int t, const double *v) { adj[(long long)t * ntrace + tr] = live ? (float)v[0] : 0.f; });
        }
    } else if (adj && inside) {
        for (int t = 0; t < nt; ++t) adj[(long long)t * ntrace + tr] = 0.f;
    }
    loss = wave_sum(loss);
    if (threadIdx.x == 0) partial[blockIdx.x] = loss;
}

// fobs [nt][ntrace]: W F obs, kept between the two sweeps
template <int NSEC, class... W>
__global__ __launch_bounds__(kLanes) void misfit_staged_gc(const Sos c, const W... sel, const float *pred, const float *obs,
                                                           int nt, long long ntrace, float *adj, float *fobs, double *partial)
{
    constexpr bool SELECT = sizeof...(W) != 0;
    const long long tr = (long long)blockIdx.x * kLanes + threadIdx.x;
    const bool inside = tr < ntrace;
    const TraceOf<W...> s(sel..., tr, inside);
    const bool live = s.live();
    double loss = 0.0;
    if (!SELECT || __any(live)) {
        if (inside) {
            double ss = 0.0, oo = 0.0, so = 0.0;
            sweep<NSEC, 2, false>(c, nt,
                                  [&](int t, double *v) {
                                      const long long o = (long long)t * ntrace + tr;
                                      const double x = (double)pred[o], y = (double)obs[o];
                                      v[0] = live ? x : 0.0;
                                      v[1] = live ? y : 0.0;
                                  },
                                  [&](int t, const double *v) {
                                      const auto w = s.w(t);
                                      const float a = (float)pick(w, v[0]), b = (float)pick(w, v[1]);
                                      ss += (double)a * (double)a; oo += (double)b * (double)b; so += (double)a * (double)b;
                                      if (adj) {
                                          const long long o = (long long)t * ntrace + tr;
                                          adj[o] = a; fobs[o] = b;
                                      }
                                  });
            const bool ok = ss > 0.0 && oo > 0.0;
            const double ns = sqrt(ss), no = sqrt(oo);
            const double cc = ok ? so / (ns * no) : 0.0;
            loss = -cc;
            if (adj) {
                // coefficients as in misfit_gc; a trace without energy on either side gets zeros (SELECT: +0 as stored
                // here; otherwise what the recurrence makes of zeros, of either sign)
                const double ka = ok ? -1.0 / (ns * no) : 0.0, kb = ok ? cc / ss : 0.0;
                sweep<NSEC, 1, true>(c, nt,
                                     [&](int t, double *v) {
                                         const long long o = (long long)t * ntrace + tr;
                                         // SELECT: both rows requested whatever `ok` says, like every other row of a chunk
                                         if constexpr (SELECT) {
                                             const double x = ka * (double)fobs[o] + kb * (double)adj[o];
                                             v[0] = ok ? pick(s.w(t), x) : 0.0;
                                         } else {
                                             v[0] = ok ? ka * (double)fobs[o] + kb * (double)adj[o] : 0.0;
                                         }
                                     },
                                     [&](int t, const double *v) {
                                         adj[(long long)t * ntrace + tr] = !SELECT || ok ? (float)v[0] : 0.f;
                                     });
            }
        }
    } else if (adj && inside) {
        for (int t = 0; t < nt; ++t) adj[(long long)t * ntrace + tr] = 0.f;
    }
    loss = wave_sum(loss);
    if (threadIdx.x == 0) partial[blockIdx.x] = loss;
}

// VEC: pred, obs and adj are 16-byte aligned (decided on the host, misfit_run); otherwise every group of four is
// read one float at a time
template <bool VEC>
__global__ __launch_bounds__(256) void misfit_l2(const float *pred, const float *obs, long long n, float *adj,
                                                 double *partial)
{
    __shared__ double s_loss[4];
    const long long stride = (long long)gridDim.x * blockDim.x * 4;
    double loss = 0.0;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (VEC && i + 3 < n) {
            const float4 p = *reinterpret_cast<const float4 *>(pred + i);
            const float4 q = *reinterpret_cast<const float4 *>(obs + i);
            const float4 r = make_float4(p.x - q.x, p.y - q.y, p.z - q.z, p.w - q.w);
            loss += (double)(r.x * r.x) + (double)(r.y * r.y) + (double)(r.z * r.z) + (double)(r.w * r.w);
            if (adj) *reinterpret_cast<float4 *>(adj + i) = r;
        } else {
            const long long e = VEC || i + 4 > n ? n : i + 4;      // VEC: only the tail of fewer than 4 lands here
            for (long long k = i; k < e; ++k) {
                const float r = pred[k] - obs[k];
                loss += (double)(r * r);
                if (adj) adj[k] = r;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) loss += __shfl_down(loss, off, 64);
    if ((threadIdx.x & 63) == 0) s_loss[threadIdx.x >> 6] = loss;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = s_loss[0] + s_loss[1] + s_loss[2] + s_loss[3];
}

// fixed-order sum of the workgroup partials (run-to-run deterministic loss)
__global__ __launch_bounds__(256) void misfit_finish(const double *partial, int n, double scale, float *loss_out)
{
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_out = (float)(s[0] * scale);
}

// ---- host: one size function and one path behind the three entry points ------------------------------------------
int l2_blocks(long long n) { return (int)std::min<long long>(2048, (n / 4 + 255) / 256 + 1); }

// the head of every work buffer: one double per workgroup, counted in floats
int64_t partial_elems(long long blocks) { return mifwi::round_up64(2 * blocks + 2, 64); }

// staged: the call has a stage filter; may_select: it may carry a selection.  Without a stage, L2 without a selection is
// misfit_l2, which sums over another grid than every other kernel: a call that may go either way gets the larger buffer.
int64_t work_elems(int32_t kind, int64_t nt, int64_t ntrace, bool staged, bool may_select)
{
    if (nt < 1 || ntrace < 1) return 0;
    const long long by_trace = mifwi_filter::blocks(ntrace);
    if (staged) return partial_elems(by_trace) + (kind == MIFWI_MISFIT_GLOBAL_CORRELATION ? nt * ntrace : 0);   // + W F obs
    const long long flat = kind == MIFWI_MISFIT_L2 ? l2_blocks(nt * ntrace) : by_trace;
    return partial_elems(may_select ? std::max(flat, by_trace) : flat);
}

// Loss and adjoint source of `kind`.  staged: F = sos[nsec] (HOST) applies; sel: W applies (NULL: nothing selected);
// direct: L1_TRACE_NORM alone.  Nothing is enqueued before every argument is checked.
int misfit_run(int device, int32_t kind, const float *pred, const float *obs, const float *direct, int64_t nt, int64_t ntrace,
               bool staged, const double *sos, int32_t nsec, const Sel *sel, float *loss_out, float *adj_out, float *work,
               void *stream)
{
    if (!pred || !obs || (staged && !sos) || !loss_out || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    if (staged && kind == MIFWI_MISFIT_L1_TRACE_NORM)
        return mifwi::fail(MIFWI_EINVAL, "the trace-normalised L1 misfit has no stage filter (the acoustic protocol has no stage)");
    if (kind != MIFWI_MISFIT_L1_TRACE_NORM && kind != MIFWI_MISFIT_L2 && kind != MIFWI_MISFIT_GLOBAL_CORRELATION)
        return mifwi::fail(MIFWI_EINVAL, "unknown misfit kind %d", kind);
    if (kind != MIFWI_MISFIT_L1_TRACE_NORM && direct)
        return mifwi::fail(MIFWI_EINVAL, "only the trace-normalised L1 misfit takes a direct wave");
    if ((reinterpret_cast<uintptr_t>(work) & 7) != 0) return mifwi::fail(MIFWI_EINVAL, "work must be 8-byte aligned");
    const bool flat = kind == MIFWI_MISFIT_L2 && !staged && !sel;          // misfit_l2; every other kernel: 64 traces a group
    Sos c;
    int rc = staged ? mifwi_filter::check(nt, ntrace, sos, nsec, &c) : mifwi_filter::check_sizes(nt, ntrace, !flat);
    if (rc) return rc;
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;

    const int T = (int)nt;
    const long long N = ntrace, n = nt * ntrace;
    const int nblk = flat ? l2_blocks(n) : (int)mifwi_filter::blocks(ntrace);
    const dim3 grid(nblk), wave(kLanes), slices(kLanes * kSl);
    double *partial = reinterpret_cast<double *>(work);
    double scale = kind == MIFWI_MISFIT_L2 ? 0.5 : 1.0;
    if (kind == MIFWI_MISFIT_L1_TRACE_NORM) {
        scale = 1.0 / (double)n;
        mifwi::with_bool(direct != nullptr, [&](auto D) {
            hipLaunchKernelGGL(misfit_l1_trace_norm<decltype(D)::value>, grid, slices, 0, st, pred, obs, direct, T, N,
                               (float)scale, adj_out, partial);
        });
    } else if (flat) {
        // float4 loads and stores only where all three pointers allow them: a view such as buf[1:] is contiguous but
        // only 4-byte aligned, and the callers pass such views through unchanged
        const bool vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(obs) |
                           reinterpret_cast<uintptr_t>(adj_out)) & 15) == 0;
        mifwi::with_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL(misfit_l2<decltype(VEC)::value>, grid, dim3(256), 0, st, pred, obs, n, adj_out, partial);
        });
    } else if (!staged) {
        if (kind == MIFWI_MISFIT_L2)
            hipLaunchKernelGGL(misfit_selected_l2_plain, grid, slices, 0, st, *sel, pred, obs, T, N, adj_out, partial);
        else if (sel)
            hipLaunchKernelGGL(misfit_gc<Sel>, grid, slices, 0, st, *sel, pred, obs, T, N, adj_out, partial);
        else
            hipLaunchKernelGGL(misfit_gc<>, grid, slices, 0, st, pred, obs, T, N, adj_out, partial);
    } else {
        float *fobs = work + partial_elems(nblk);
        mifwi::with_int<1, 2, 3, 4, 5, 6, 7, 8>(nsec, [&](auto NSEC) {
            constexpr int S = decltype(NSEC)::value;
            if (kind == MIFWI_MISFIT_L2 && sel)
                hipLaunchKernelGGL((misfit_staged_l2<S, Sel>), grid, wave, 0, st, c, *sel, pred, obs, T, N, adj_out, partial);
            else if (kind == MIFWI_MISFIT_L2)
                hipLaunchKernelGGL(misfit_staged_l2<S>, grid, wave, 0, st, c, pred, obs, T, N, adj_out, partial);
            else if (sel)
                hipLaunchKernelGGL((misfit_staged_gc<S, Sel>), grid, wave, 0, st, c, *sel, pred, obs, T, N, adj_out, fobs, partial);
            else
                hipLaunchKernelGGL(misfit_staged_gc<S>, grid, wave, 0, st, c, pred, obs, T, N, adj_out, fobs, partial);
        });
    }
    hipLaunchKernelGGL(misfit_finish, dim3(1), dim3(256), 0, st, partial, nblk, scale, loss_out);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // namespace

extern "C" {

int64_t mifwi_misfit_work_elems(int32_t kind, int64_t nt, int64_t ntrace) { return work_elems(kind, nt, ntrace, false, false); }

int mifwi_misfit(int device, int32_t kind, const float *pred, const float *obs, const float *direct,
                 int64_t nt, int64_t ntrace, float *loss_out, float *adj_out, float *work, void *stream)
{
    return misfit_run(device, kind, pred, obs, direct, nt, ntrace, false, nullptr, 0, nullptr, loss_out, adj_out, work, stream);
}

int64_t mifwi_misfit_filtered_work_elems(int32_t kind, int64_t nt, int64_t ntrace) { return work_elems(kind, nt, ntrace, true, false); }

int mifwi_misfit_filtered(int device, int32_t kind, const float *pred, const float *obs, int64_t nt, int64_t ntrace,
                          const double *sos, int32_t nsec, float *loss_out, float *adj_out, float *work, void *stream)
{
    return misfit_run(device, kind, pred, obs, nullptr, nt, ntrace, true, sos, nsec, nullptr, loss_out, adj_out, work, stream);
}

int64_t mifwi_misfit_selected_work_elems(int32_t kind, int64_t nt, int64_t ntrace, int32_t nsec)
{
    return work_elems(kind, nt, ntrace, nsec > 0, true);
}

int mifwi_misfit_selected(int device, int32_t kind, const float *pred, const float *obs, int64_t nt, int64_t ntrace,
                          const double *sos, int32_t nsec, const float *trace_w, const float *t_on, const float *t_off,
                          double gamma, float *loss_out, float *adj_out, float *work, void *stream)
{
    if (kind == MIFWI_MISFIT_L1_TRACE_NORM)
        return mifwi::fail(MIFWI_EINVAL, "the trace-normalised L1 misfit has no trace selection (the acoustic protocol has none)");
    if ((sos != nullptr) != (nsec != 0))
        return mifwi::fail(MIFWI_EINVAL, "sos and nsec=%d disagree: sos is NULL exactly when nsec is 0 (no stage)", nsec);
    int rc = mifwi_select::check(t_on, t_off, gamma);
    if (rc) return rc;
    // nothing selected: the very instances of the calls without a selection
    const Sel sel = {trace_w, t_on, t_off, gamma};
    return misfit_run(device, kind, pred, obs, nullptr, nt, ntrace, sos != nullptr, sos, nsec, trace_w || t_on ? &sel : nullptr,
                      loss_out, adj_out, work, stream);
}

int mifwi_trace_filter(int device, const float *x, float *y, int64_t nt, int64_t ntrace, const double *sos,
                       int32_t nsec, int32_t transpose, void *stream)
{
    if (!x || !y || !sos) return mifwi::fail(MIFWI_EINVAL, "null argument");
    Sos c;
    int rc = mifwi_filter::check(nt, ntrace, sos, nsec, &c);
    if (rc) return rc;
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;
    mifwi::with_int<1, 2, 3, 4, 5, 6, 7, 8>(nsec, [&](auto NSEC) {
        mifwi::with_bool(transpose != 0, [&](auto REV) {
            hipLaunchKernelGGL((mifwi_filter::trace_filter<decltype(NSEC)::value, decltype(REV)::value>),
                               dim3((unsigned)mifwi_filter::blocks(ntrace)), dim3(kLanes), 0, st, c, x, y, (int)nt,
                               (long long)ntrace);
        });
    });
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

int mifwi_trace_window(int device, const float *x, float *y, int64_t nt, int64_t ntrace, const float *trace_w,
                       const float *t_on, const float *t_off, double gamma, void *stream)
{
    if (!x || !y) return mifwi::fail(MIFWI_EINVAL, "null argument");
    int rc = mifwi_filter::check_sizes(nt, ntrace);
    if (rc) return rc;
    rc = mifwi_select::check(t_on, t_off, gamma);
    if (rc) return rc;
    hipStream_t st;
    rc = mifwi::select_device(device, stream, &st);
    if (rc) return rc;
    const Sel sel = {trace_w, t_on, t_off, gamma};
    hipLaunchKernelGGL(mifwi_select::trace_window, dim3((unsigned)mifwi_filter::blocks(ntrace)), dim3(kLanes * kSl), 0, st,
                       sel, x, y, (int)nt, (long long)ntrace);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

}  // extern "C"
