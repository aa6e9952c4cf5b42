// Trace selection inside the misfit kernels (included by mifwi_misfit.hip after mifwi_misfit_filter.h): what DENISE's
// TRKILL and TIMEWIN do to the data of a field survey - dead channels, noisy near offsets and everything after the picked
// event leave the OBJECTIVE, not the arrays.  The selection is the diagonal operator W,
//     w[t, tr] = a[tr] g(t; t_on[tr], t_off[tr], gamma),   d = max(t_on - t, t - t_off, 0),   g = d == 0 ? 1 : exp(-gamma d^2)
// (a >= 0 the trace weight, 0 = killed; t the sample index; t_on, t_off float, in samples, anywhere and in any order;
// gamma >= 0 per sample^2, +inf = boxcar), evaluated in double from the float inputs, applied after the stage filter F
// (the identity without a stage) and before the norm:
//     L2                  r = float(W F(pred - obs));  loss = 1/2 sum r^2;  adj = float(F^T W r)
//     GLOBAL_CORRELATION  s = float(W F pred), o = float(W F obs);  loss, ka, kb as without a selection;
//                         adj = float(F^T W (ka o + kb s))
// W SELECTS, it does not multiply: where w == 0 exactly the sample's value is not used (w ? w x : 0).  A killed trace
// (a == 0) may therefore hold anything in pred and obs, NaN and Inf included: it is never fed to the recurrence, its loss
// contribution is exactly 0 and its adj column is exactly 0.  Inside a LIVE trace the guarantee does not hold: a NaN that
// went through the recursive filter stays in its state for the rest of the trace, and no zero weight further down can
// take it out again.
//
// This header holds W itself: its arguments (Sel), one trace's share of it in registers (Trace, pick), the kernel that
// applies it alone (trace_window).  The objectives of mifwi_misfit.hip take it as their SELECT instances.  With a stage
// (misfit_staged_l2, misfit_staged_gc: mifwi_filter::sweep, one lane per trace) W sits in the forward sweep's out and in
// the reverse sweep's in, exp runs only where d > 0, and a wave whose 64 traces are all killed runs no sweep and writes
// zeros.  Without a stage: 64 traces x 16 time slices (misfit_gc, misfit_selected_l2_plain).  No atomics, fixed
// summation order.
#pragma once
#include <cmath>
#include <type_traits>

namespace mifwi_select {

using mifwi_filter::kLanes;

constexpr int kSl = 16;          // time slices per workgroup of the kernels without a stage

struct Sel {                     // device [ntrace] arrays; a == NULL: weight 1, on == off == NULL: no window
    const float *a, *on, *off;
    double gamma;
};

#ifdef __HIPCC__
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

// Nothing selected, in Trace's shape: what the objectives' instances without SELECT are written against.  Every sample
// passes as it is, so such an instance holds no trace of W.
struct One {};
struct Every {
    __device__ __forceinline__ Every(long long, bool) {}
    __device__ constexpr bool live() const { return true; }
    __device__ constexpr One w(int) const { return {}; }
};
__device__ __forceinline__ double pick(One, double x) { return x; }
// W... = Sel: that selection's Trace; empty: Every
template <class... W>
using TraceOf = std::conditional_t<sizeof...(W) != 0, Trace, Every>;

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

}  // namespace mifwi_select
