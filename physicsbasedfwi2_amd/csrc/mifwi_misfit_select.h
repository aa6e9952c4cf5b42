// Trace selection inside the misfit kernels (included by mifwi_misfit.hip after mifwi_misfit_filter.h): what DENISE's
// TRKILL and TIMEWIN do to the data of a field survey - dead channels, noisy near offsets and everything after the picked
// event leave the OBJECTIVE, not the arrays.  The selection is the diagonal operator W,
//     w[t, tr] = a[tr] g(t; t_on[tr], t_off[tr], gamma),   d = max(t_on - t, t - t_off, 0),   g = d == 0 ? 1 : exp(-gamma d^2)
// (a >= 0 the trace weight, 0 = killed; t the sample index; t_on, t_off float, in samples, anywhere and in any order;
// gamma >= 0 per sample^2, +inf = boxcar), evaluated in double from the float inputs, applied after the stage filter F
// (the identity without a stage) and before the norm:
//     L2                  r = float(W F(pred - obs));  loss = 1/2 sum r^2;  adj = float(F^T W r)
//     GLOBAL_CORRELATION  s = float(W F pred), o = float(W F obs);  loss, ka, kb as misfit_filtered_gc;
//                         adj = float(F^T W (ka o + kb s))
// W SELECTS, it does not multiply: where w == 0 exactly the sample's value is not used (w ? w x : 0).  A killed trace
// (a == 0) may therefore hold anything in pred and obs, NaN and Inf included: it is never fed to the recurrence, its loss
// contribution is exactly 0 and its adj column is exactly 0.  Inside a LIVE trace the guarantee does not hold: a NaN that
// went through the recursive filter stays in its state for the rest of the trace, and no zero weight further down can
// take it out again.
//
// With a stage: mifwi_filter::sweep as the filtered kernels run it (one lane per trace, one wave per workgroup, rows
// requested ahead of the recurrence); W sits in the forward sweep's out and in the reverse sweep's in, exp runs only where
// d > 0, and a wave whose 64 traces are all killed runs no sweep and writes zeros.  Without a stage: the 64 traces x 16
// time slices of misfit_global_correlation.  No atomics, fixed summation order.
#pragma once
#include <cmath>

namespace mifwi_select {

using mifwi_filter::kLanes;
using mifwi_filter::Sos;

constexpr int kSl = 16;          // time slices per workgroup of the kernels without a stage

struct Sel {                     // device [ntrace] arrays; a == NULL: weight 1, on == off == NULL: no window
    const float *a, *on, *off;
    double gamma;
};

#ifdef __HIPCC__
using mifwi_filter::sweep;

struct Trace {                   // one trace's selection, in registers
    double a, on, off, gamma;
    bool win;
    __device__ __forceinline__ Trace(const Sel &s, long long tr, bool inside)
        : a(inside ? (s.a ? (double)s.a[tr] : 1.0) : 0.0), on(inside && s.on ? (double)s.on[tr] : 0.0),
          off(inside && s.on ? (double)s.off[tr] : 0.0), gamma(s.gamma), win(s.on != nullptr) {}
    __device__ __forceinline__ bool live() const { return a > 0.0; }
    __device__ __forceinline__ double w(int t) const
    {
        if (!win) return a;
        const double d = fmax(fmax(on - (double)t, (double)t - off), 0.0);
        return d > 0.0 ? a * exp(-gamma * d * d) : a;
    }
};

// w ? w x : 0
__device__ __forceinline__ double pick(double w, double x) { return w != 0.0 ? w * x : 0.0; }

template <int NSEC>
__global__ __launch_bounds__(kLanes) void misfit_selected_l2(const Sos c, const Sel sel, const float *pred, const float *obs,
                                                             int nt, long long ntrace, float *adj, double *partial)
{
    const long long tr = (long long)blockIdx.x * kLanes + threadIdx.x;
    const bool inside = tr < ntrace;
    const Trace s(sel, tr, inside);
    const bool live = s.live();
    double loss = 0.0;
    if (__any(live)) {
        if (inside) {
            // a killed lane among live ones runs the recurrence on zeros: its rows are requested like the others' (every
            // load of a chunk stays unconditional) and dropped
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
            if (adj)
                sweep<NSEC, 1, true>(c, nt,
                                     [&](int t, double *v) { v[0] = pick(s.w(t), (double)adj[(long long)t * ntrace + tr]); },
                                     [&](int t, const double *v) { adj[(long long)t * ntrace + tr] = live ? (float)v[0] : 0.f; });
        }
    } else if (adj && inside) {
        for (int t = 0; t < nt; ++t) adj[(long long)t * ntrace + tr] = 0.f;
    }
    loss = mifwi_filter::wave_sum(loss);
    if (threadIdx.x == 0) partial[blockIdx.x] = loss;
}

template <int NSEC>
__global__ __launch_bounds__(kLanes) void misfit_selected_gc(const Sos c, const Sel sel, const float *pred, const float *obs,
                                                             int nt, long long ntrace, float *adj, float *fobs, double *partial)
{
    const long long tr = (long long)blockIdx.x * kLanes + threadIdx.x;
    const bool inside = tr < ntrace;
    const Trace s(sel, tr, inside);
    const bool live = s.live();
    double loss = 0.0;
    if (__any(live)) {
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
                                      const double w = s.w(t);
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
                const double ka = ok ? -1.0 / (ns * no) : 0.0, kb = ok ? cc / ss : 0.0;
                sweep<NSEC, 1, true>(c, nt,
                                     [&](int t, double *v) {
                                         const long long o = (long long)t * ntrace + tr;
                                         const double x = ka * (double)fobs[o] + kb * (double)adj[o];
                                         v[0] = ok ? pick(s.w(t), x) : 0.0;
                                     },
                                     [&](int t, const double *v) { adj[(long long)t * ntrace + tr] = ok ? (float)v[0] : 0.f; });
            }
        }
    } else if (adj && inside) {
        for (int t = 0; t < nt; ++t) adj[(long long)t * ntrace + tr] = 0.f;
    }
    loss = mifwi_filter::wave_sum(loss);
    if (threadIdx.x == 0) partial[blockIdx.x] = loss;
}

// ---- without a stage: 64 traces x 16 interleaved time slices per workgroup; a killed trace is never read -------------
// workgroup sum in a fixed order: the lanes of a wave, then the 16 waves
__device__ __forceinline__ void block_sum(double v, double *s_loss, int lane, int sl, double *partial)
{
    v = mifwi_filter::wave_sum(v);
    if (lane == 0) s_loss[sl] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < kSl; ++k) tot += s_loss[k];
        partial[blockIdx.x] = tot;
    }
}

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

__global__ __launch_bounds__(kLanes *kSl) void misfit_selected_gc_plain(const Sel sel, const float *pred, const float *obs,
                                                                        int nt, long long ntrace, float *adj, double *partial)
{
    __shared__ double s_ss[kSl][kLanes], s_oo[kSl][kLanes], s_so[kSl][kLanes];
    __shared__ double s_loss[kSl];
    const int lane = (int)threadIdx.x % kLanes, sl = (int)threadIdx.x / kLanes;
    const long long tr = (long long)blockIdx.x * kLanes + lane;
    const bool inside = tr < ntrace;
    const Trace s(sel, tr, inside);
    const bool live = s.live();
    double ss = 0.0, oo = 0.0, so = 0.0;
    if (live)
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            const double w = s.w(t);
            const double a = (double)(float)pick(w, (double)pred[o]), b = (double)(float)pick(w, (double)obs[o]);
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
        const double ka = ok ? -1.0 / (ns * no) : 0.0, kb = ok ? cc / ss : 0.0;
        for (int t = sl; t < nt; t += kSl) {
            const long long o = (long long)t * ntrace + tr;
            float g = 0.f;
            if (ok) {
                const double w = s.w(t);
                const double a = (double)(float)pick(w, (double)pred[o]), b = (double)(float)pick(w, (double)obs[o]);
                g = (float)pick(w, ka * b + kb * a);
            }
            adj[o] = g;
        }
    }
    block_sum(sl == 0 ? -cc : 0.0, s_loss, lane, sl, partial);          // one slice speaks for the trace
}

// y = W x; y == x allowed (every sample is read and written by one thread)
__global__ __launch_bounds__(kLanes *kSl) void trace_window(const Sel sel, const float *x, float *y, int nt, long long ntrace)
{
    const int lane = (int)threadIdx.x % kLanes, sl = (int)threadIdx.x / kLanes;
    const long long tr = (long long)blockIdx.x * kLanes + lane;
    if (tr >= ntrace) return;
    const Trace s(sel, tr, true);
    for (int t = sl; t < nt; t += kSl) {
        const long long o = (long long)t * ntrace + tr;
        y[o] = s.live() ? (float)pick(s.w(t), (double)x[o]) : 0.f;
    }
}
#endif  // __HIPCC__

// trace_w, t_on, t_off: device [ntrace] or NULL
inline int check(const float *t_on, const float *t_off, double gamma)
{
    if ((t_on == nullptr) != (t_off == nullptr))
        return mifwi::fail(MIFWI_EINVAL, "a time window needs both t_on and t_off (one of them is NULL)");
    if (!(gamma >= 0.0)) return mifwi::fail(MIFWI_EINVAL, "gamma=%g: the taper needs gamma >= 0 (+inf: boxcar)", gamma);
    return MIFWI_OK;
}

#ifdef __HIPCC__
#define MIFWI_SELECT_BY_NSEC(CALL)                                                                                   \
    switch (nsec) {                                                                                                  \
    case 1: CALL(1); break;                                                                                          \
    case 2: CALL(2); break;                                                                                          \
    case 3: CALL(3); break;                                                                                          \
    case 4: CALL(4); break;                                                                                          \
    case 5: CALL(5); break;                                                                                          \
    case 6: CALL(6); break;                                                                                          \
    case 7: CALL(7); break;                                                                                          \
    default: CALL(8); break;                                                                                         \
    }

inline void launch_l2(int nsec, unsigned nblk, hipStream_t st, const Sos &c, const Sel &s, const float *pred, const float *obs,
                      int nt, long long ntrace, float *adj, double *partial)
{
    if (nsec == 0) {
        hipLaunchKernelGGL(misfit_selected_l2_plain, dim3(nblk), dim3(kLanes * kSl), 0, st, s, pred, obs, nt, ntrace, adj, partial);
        return;
    }
#define MIFWI_CALL(N) \
    hipLaunchKernelGGL(misfit_selected_l2<N>, dim3(nblk), dim3(kLanes), 0, st, c, s, pred, obs, nt, ntrace, adj, partial)
    MIFWI_SELECT_BY_NSEC(MIFWI_CALL)
#undef MIFWI_CALL
}

inline void launch_gc(int nsec, unsigned nblk, hipStream_t st, const Sos &c, const Sel &s, const float *pred, const float *obs,
                      int nt, long long ntrace, float *adj, float *fobs, double *partial)
{
    if (nsec == 0) {
        hipLaunchKernelGGL(misfit_selected_gc_plain, dim3(nblk), dim3(kLanes * kSl), 0, st, s, pred, obs, nt, ntrace, adj, partial);
        return;
    }
#define MIFWI_CALL(N) \
    hipLaunchKernelGGL(misfit_selected_gc<N>, dim3(nblk), dim3(kLanes), 0, st, c, s, pred, obs, nt, ntrace, adj, fobs, partial)
    MIFWI_SELECT_BY_NSEC(MIFWI_CALL)
#undef MIFWI_CALL
}
#undef MIFWI_SELECT_BY_NSEC
#endif  // __HIPCC__

}  // namespace mifwi_select
