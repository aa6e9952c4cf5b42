// Host-side driver of the single-launch ("cluster") time loops of both physics: LDS attribute of a kernel family, hand-off
// buffer view, copy of a resumed call's state, phase trace, and the ladder single launch -> agent-scope publishes -> one
// launch per step.  No device code.
#pragma once
#include "mifwi_common.h"
#include <vector>

namespace mifwi {

inline int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// nap between two poll passes of a halo hand-off (mifwi::poll_nap): fat slabs nap long, thin ones short; `fat_rows` is
// the physics' threshold (acoustic 16, elastic 8)
inline int poll_nap_default(int rows_per_slab, int fat_rows)
{
    return env_int("MIFWI_POLL_NAP", rows_per_slab >= fat_rows ? 48 : 1);
}

// Dynamic-LDS cap of a single-launch kernel family: entry(0 .. entries-1) walks the whole domain of the family's variant
// table (the selectors packed into the index; null: no such variant).  The attribute is per function, so it is set once
// per device and process (`done`: the family's guard, one bit per device), not once per plan - a plan is created on every
// propagate call.  False: a call failed (not sticky) - this plan does without the family, and the guard stays unset, so
// the next plan tries again.
template <class Entry>
bool lds_cap_once(std::atomic<unsigned> &done, int device, int bytes, int entries, Entry &&entry)
{
    if (device < 32 && (done.load() >> device & 1u)) return true;
    for (int v = 0; v < entries; ++v) {
        const void *fn = (const void *)entry(v);
        if (fn && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    }
    if (device < 32) done.fetch_or(1u << device);
    return true;
}

// A single-launch attempt may give up (some workgroup was not resident in time, or the slabs of a shot were not dealt to
// one XCD) after it has advanced the state by an unknown number of steps.  A call that starts from the zero state is
// simply zeroed again; a resumed call (time checkpointing) keeps a copy of its input state behind the work buffer's
// other regions and gets it back.
inline int cluster_backup(float *work, long long state_elems, float *backup, int32_t flags, hipStream_t st)
{
    if (flags & MIFWI_ZERO_STATE) return MIFWI_OK;
    MIFWI_HIP_TRY(hipMemcpyAsync(backup, work, sizeof(float) * state_elems, hipMemcpyDeviceToDevice, st));
    return MIFWI_OK;
}
inline int cluster_restore(float *work, long long state_elems, const float *backup, int32_t flags, hipStream_t st)
{
    if (flags & MIFWI_ZERO_STATE) MIFWI_HIP_TRY(hipMemsetAsync(work, 0, sizeof(float) * state_elems, st));
    else MIFWI_HIP_TRY(hipMemcpyAsync(work, backup, sizeof(float) * state_elems, hipMemcpyDeviceToDevice, st));
    return MIFWI_OK;
}

// The hand-off buffer of a single-launch kernel, `elems` floats: [granules | xcc_tab | error block].  xcc_tab is the
// XCC_ID table of mifwi::same_xcd ([nshot][slabs] ints, rounded up to 64), the error block the last 64 ints (kErr*).
inline long long handoff_xcc_elems(long long nshot, long long slabs) { return round_up64(nshot * slabs, 64); }
inline long long handoff_elems(long long granule_floats, long long xcc_elems) { return round_up64(granule_floats, 64) + xcc_elems + 64; }
struct Handoff { float *base; long long elems; unsigned long long *granules; int *xcc_tab, *err; };
inline Handoff handoff_view(float *xbuf, long long xbuf_elems, long long xcc_elems)
{
    return {xbuf, xbuf_elems, reinterpret_cast<unsigned long long *>(xbuf),
            reinterpret_cast<int *>(xbuf + xbuf_elems - 64 - xcc_elems), reinterpret_cast<int *>(xbuf + xbuf_elems - 64)};
}

// Phase trace (ablation builds only): MIFWI_AC_CL_TRACE / MIFWI_EL_CL_TRACE=<file> make one workgroup write time stamps
// at its phase boundaries (CL_STAMP / EC_STAMP), steps 64..127; every attempt appends them to the file as text: the
// header line (a format taking the two ints), then 16 stamps per line (tools/cluster_trace.py reads them).
struct TraceSpec { const char *env; size_t n; const char *header; int a, b; };      // n stamps: 64 steps x waves x 16 phases
// the parameter structs carry their `trace` pointer in ablation builds only
template <class Params>
inline void set_trace(Params &c, long long *trace)
{
#ifdef MIFWI_ABLATIONS
    c.trace = trace;
#endif
}
#ifdef MIFWI_ABLATIONS
struct PhaseTrace {
    long long *dev = nullptr;
    size_t n = 0;
    long long *begin(hipStream_t st, size_t count)          // zeroed device stamps (null: no memory, no trace)
    {
        n = count;
        if (hipMalloc(&dev, n * sizeof(long long)) != hipSuccess) dev = nullptr;
        else (void)hipMemsetAsync(dev, 0, n * sizeof(long long), st);
        return dev;
    }
    void end(const char *path, const TraceSpec &ts)          // after the stream has been synchronised
    {
        if (!dev) return;
        std::vector<long long> h(n);
        (void)hipMemcpy(h.data(), dev, n * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(dev);
        if (FILE *fp = fopen(path, "a")) {
            fprintf(fp, ts.header, ts.a, ts.b);
            fprintf(fp, "\n");
            for (size_t i = 0; i < n; i += 16) {
                for (int k = 0; k < 16; ++k) fprintf(fp, "%lld ", h[i + k]);
                fprintf(fp, "\n");
            }
            fclose(fp);
        }
    }
};
#endif

// What cluster_ladder returns when the single-launch kernels gave up: the state is back where the call found it, the
// notes are said, and the caller runs the range with one launch per (half) step.  (Errors are negative, MIFWI_OK is 0.)
constexpr int kClusterFellBack = 3;

// The ladder every single-launch time loop runs through.  `launch(agent, trace)` only enqueues the kernels of one attempt
// over the shot batches (agent: the variants that publish granules at agent scope; trace: for set_trace).  After a failed
// placement check the state is restored and the launch repeated once at agent scope; after a time-out (or a second
// placement failure) the state is restored and kClusterFellBack returned.  MIFWI_OK: the range is done.
// MIFWI_TEST_FAKE_TIMEOUT (mifwi::fake_timeout): 1 gives up before anything is enqueued, 2 after the attempt has run.
template <class Launch>
int cluster_ladder(const char *what, float *work, long long state_elems, float *backup, int32_t flags, hipStream_t st,
                   const Handoff &h, const TraceSpec &ts, Launch &&launch)
{
    int rc = cluster_backup(work, state_elems, backup, flags, st);
    if (rc) return rc;
    const int fake = fake_timeout();
    auto attempt = [&](bool agent) -> int {
        MIFWI_HIP_TRY(hipMemsetAsync(h.base, 0, sizeof(float) * h.elems, st));
        long long *stamps = nullptr;
#ifdef MIFWI_ABLATIONS
        PhaseTrace trace;
        const char *trace_path = getenv(ts.env);
        if (trace_path && *trace_path) stamps = trace.begin(st, ts.n);
#endif
        launch(agent, stamps);
        MIFWI_HIP_TRY(hipGetLastError());
        int err[4] = {0, 0, 0, 0};
        MIFWI_HIP_TRY(hipMemcpyAsync(err, h.err, sizeof(err), hipMemcpyDeviceToHost, st));
        MIFWI_HIP_TRY(hipStreamSynchronize(st));
#ifdef MIFWI_ABLATIONS
        trace.end(trace_path, ts);
#endif
        const int verdict = cluster_verdict(err, what);
        return fake == 2 ? kClusterTimedOut : verdict;
    };
    int verdict = fake == 1 ? kClusterTimedOut : attempt(false);
    if (verdict == kClusterMisplaced) {          // not on one XCD: once more with hand-offs through the fabric
        note_agent_tier(what);
        rc = cluster_restore(work, state_elems, backup, flags, st);
        if (rc) return rc;
        verdict = attempt(true);
    }
    if (verdict != kClusterTimedOut && verdict != kClusterMisplaced) return verdict;      // done, or an error
    note_fallback(what);
    rc = cluster_restore(work, state_elems, backup, flags, st);
    return rc ? rc : kClusterFellBack;
}

// the hand-off buffer of a plan inside a call's work buffer (`m`: the physics' map of that buffer)
template <class Plan, class Map>
Handoff cluster_handoff(const Plan *pl, float *work, const Map &m) { return handoff_view(work + m.xbuf, pl->xbuf_elems, pl->xcc_elems); }

}  // namespace mifwi
