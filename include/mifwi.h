/*
 * mifwi.h -- C-ABI of the MI355X-native 2-D finite-difference wave propagator
 * (libmifwi.so, hand-written HIP for gfx950).
 *
 * The reference (ADharaUTEXAS123007/PhysicsBasedFWI2) has no C interface of its own: its
 * hot path is reached through three third-party Python call protocols.  Every entry point
 * below names the reference call site(s) it replaces (paths relative to the reference
 * tree); INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MIFWI_E* code otherwise; no C++
 *     exception crosses the boundary; mifwi_last_error() gives the message (thread-local).
 *   - all array arguments are DEVICE pointers owned by the caller (the Python host passes
 *     torch tensors' data_ptr()); the library allocates no device memory and keeps no
 *     global state; `stream` is a hipStream_t (0 = default stream).
 *   - arithmetic is fp32; indices are int32; cells are linear indices i0*n1+i1 into the
 *     computational grid (axis 1 fastest), -1 = inactive tap.
 *   - there is NO CPU fallback: without a visible gfx950 device every compute call fails
 *     with MIFWI_ENODEVICE.
 */
#ifndef MIFWI_H
#define MIFWI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIFWI_VERSION_MAJOR 0
#define MIFWI_VERSION_MINOR 7   /* 3: elastic desc gained snapshot_format, fd_order; layout snap_step_elems, snapshot_format; 4: mifwi_fallback_count; 5: mifwi_agent_handoff_count, mifwi_slow_handoff_count; acoustic desc gained cpml_width, layout state_elems; 6: mifwi_elastic_materials(_vjp), mifwi_acoustic_coefficients(_vjp); 7: mifwi_elastic_gradient_parametrization; elastic snapshot planes column-blocked in plans without a single-launch kernel; later additions that leave every existing call as it was keep 7: mifwi_elastic_snapshot_moments, mifwi_elastic_pseudo_hessian, mifwi_gradient_precondition, mifwi_elastic_born, mifwi_acoustic_snapshot_moments, mifwi_acoustic_pseudo_hessian, mifwi_fluid_born, mifwi_fluid_snapshot_moments, mifwi_fluid_pseudo_hessian */

enum {
    MIFWI_OK = 0,
    MIFWI_EINVAL = -1,     /* bad argument / shape mismatch                     */
    MIFWI_ENODEVICE = -2,  /* no HIP device / wrong architecture                */
    MIFWI_EHIP = -3,       /* a HIP runtime call failed                          */
    MIFWI_ECFL = -4,       /* stability limit violated                           */
    MIFWI_ENOMEM = -5      /* caller-provided workspace too small                */
};

const char *mifwi_last_error(void);
int mifwi_version(void);                 /* major*1000 + minor                  */
/* Calls of this process whose single-launch time loop gave up (hand-off time-out, slabs of a shot not on one XCD) and
 * were re-run with one launch per step: results are the same, the time is not.  Monitoring and tests read it; the
 * first such call is also noted on stderr (MIFWI_QUIET=1 silences that). */
int64_t mifwi_fallback_count(void);
/* Single-launch time loops that were repeated with hand-offs through the fabric (agent-scope publishes) because the
 * slabs of a shot had not been placed on one XCD: still one launch per time loop, 10-15 % slower per step. */
int64_t mifwi_agent_handoff_count(void);
/* Single-launch time loops in which some workgroup needed more than 32 poll passes for a neighbour's rows - what a
 * GPU shared with another process looks like (the loop then runs many times slower, results unchanged, no fall-back):
 * one rank must own the GPU while a propagator call runs.  The first such launch is noted on stderr. */
int64_t mifwi_slow_handoff_count(void);
int mifwi_device_count(void);            /* number of visible HIP devices, >=0  */
/* engine / memory clock (kHz) and compute units of a device, for measurement reports; 0 where unknown */
int mifwi_device_info(int device, int32_t *sclk_khz, int32_t *mclk_khz, int32_t *compute_units);

/* ======================================================================================
 * 2-D constant-density ACOUSTIC propagator (forward + exact discrete adjoint)
 *
 * Replaces:
 *   deepwave.scalar.Propagator({'vp': m}, dx)(src, x_s, x_r, dt) and its autograd
 *   backward                                   models/networks.py:5408-5411, 5449, 5464, 5491
 *   Devito Forward/Gradient operators          seisgan/fwi/pde/seismic/acoustic/operators.py:54-89,
 *                                              127-165 ; wavesolver.py:72-107, 143-172
 *
 * Scheme:  r = vp^2 dt^2/h^2 = s^2/(m h^2);  q = q0[i0]+q1[i1]
 *   u+ = (2u - (1-q r) u- + r L4(u)) / (1+q r) + sum_taps w f[n] r[cell]
 *   rec[n] = sum_taps w u^n[cell]            (time loop n = 0..nt-1)
 * ==================================================================================== */
typedef struct {
    int32_t n0, n1;        /* computational grid (caller has already padded the model)      */
    int32_t nt;            /* time steps                                                    */
    int32_t nshot;         /* shots propagated together (independent wavefields)            */
    int32_t nsrc, nrec;    /* sources / receivers per shot                                  */
    int32_t ntap;          /* taps per point: 1 = nearest cell, 4 = bilinear                */
    float c0, c1;          /* (h/h0)^2, (h/h1)^2 with h = min(h0,h1)                        */
    int32_t shots_per_group; /* shots marched by one thread (gradient RMW amortisation); 0 = auto */
    int32_t edge_rows;     /* optional hint: rows of absorbing layer at the top and at the bottom
                              (0 = unknown); lets the single-launch kernels give the layer slabs
                              of its own.  Results do not depend on it.                       */
    int32_t cpml_width;    /* 0: absorbing layer = the sponge q0, q1.  W > 0: second-order convolutional
                              PML, W cells wide on all four sides (what deepwave.scalar.Propagator's
                              pml_width is, models/networks.py:5408-5411):
                                psi_d <- b psi_d + a d_d u;  zeta_d <- b zeta_d + a (d_d^2 u + d_d psi_d)
                                u_tt = vp^2 sum_d [d_d^2 u + d_d psi_d + zeta_d]
                              with its exact transposed adjoint (DESIGN.md section 3,
                              oracle/acoustic_cpml.c).  The q0 / q1 arguments of the calls then carry the
                              layer's profiles instead of the sponge: q0 = [2][n0] (a, b along axis 0),
                              q1 = [2][gp] (a, b along axis 1), zero outside the layer.  One launch per
                              step family; the wavefield state grows by the memory variables
                              (layout.state_elems).                                              */
} mifwi_acoustic_desc;

typedef struct mifwi_acoustic_plan mifwi_acoustic_plan;

int mifwi_acoustic_plan_create(mifwi_acoustic_plan **plan, int device,
                               const mifwi_acoustic_desc *desc);
int mifwi_acoustic_plan_destroy(mifwi_acoustic_plan *plan);

/* Buffer layout the caller needs for allocation (all counts in floats):
 *   wavefields      [nshot][n0+4][pitch]   (2 halo rows top/bottom, interior column 0 at +4)
 *   coefficient r, every snapshot slice, gradients, accumulators   [n0][gp]
 *   gp = n1 rounded up to a multiple of 4; cells i1 >= n1 of r must be 0.                   */
typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t field_elems;          /* one wavefield set                                       */
    int64_t coef_elems;           /* n0*gp                                                   */
    int64_t work_forward_elems;   /* size of `work` for mifwi_acoustic_forward               */
    int64_t work_backward_elems;  /* size of `work` for mifwi_acoustic_backward              */
    int64_t state_elems;          /* head of `work` that is the forward state a checkpoint must keep:
                                     2*field_elems (+ the C-PML memory variables)             */
} mifwi_acoustic_layout;

int mifwi_acoustic_plan_layout(const mifwi_acoustic_plan *plan, mifwi_acoustic_layout *out);
/* Shot groups per pass of the per-step kernels (forward, adjoint); introspection only. */
int mifwi_acoustic_plan_pass_sizes(const mifwi_acoustic_plan *plan, int32_t *forward_groups, int32_t *adjoint_groups);

/* flags for the time-range calls */
#define MIFWI_ZERO_STATE 1   /* zero the wavefield state (and accumulators) in `work` first   */
#define MIFWI_FINALIZE   2   /* backward: reduce accumulators into grad_r, emit grad_f[k_lo-1] */

/* Forward modelling of steps n = n_begin .. n_end-1 (a full run is [0, nt) with
 * MIFWI_ZERO_STATE).  The wavefield state (u^n, u^{n-1}) lives in the first
 * 2*field_elems floats of `work`; buffer parity is absolute in n, so a run can be split
 * into ranges and the state copied out/in by the caller (time checkpointing).
 *   r [n0][gp], q0 [n0], q1 [gp]
 *   f [nt][nshot][nsrc]; src_cell/src_w [nshot][nsrc][ntap]; rec_cell/rec_w [nshot][nrec][ntap]
 *   rec_out [nt][nshot][nrec] or NULL (no sampling)
 *   snap : NULL, or [n_end-n_begin][nshot][n0][gp] receiving G^n = d u^{n+1}/d r
 *   work : layout.work_forward_elems floats                                                 */
int mifwi_acoustic_forward(mifwi_acoustic_plan *plan, const float *r, const float *q0,
                           const float *q1, const float *f, const int32_t *src_cell,
                           const float *src_w, const int32_t *rec_cell, const float *rec_w,
                           float *rec_out, float *snap, float *work, int32_t n_begin,
                           int32_t n_end, int32_t flags, void *stream);

/* Born / linearised modelling (seisgan/fwi/pde/seismic/acoustic/operators.py:168-207,
 * wavesolver.py:174-209): first-order change of the seismograms, drec = J dr, around the forward
 * run whose snapshots are passed in.  The perturbation field obeys the forward recursion with the
 * distributed source G^n dr and no point source; J is the exact transpose partner of the gradient
 * mifwi_acoustic_backward returns (<J dr, g> = <dr, grad_r(g)>).
 *   dr [n0][gp] perturbation of r;  snap as written by mifwi_acoustic_forward (step n at
 *   snap + (n-snap_first)*nshot*n0*gp);  drec_out [nt][nshot][nrec];  work = work_forward_elems   */
int mifwi_acoustic_born(mifwi_acoustic_plan *plan, const float *r, const float *q0, const float *q1,
                        const float *dr, const int32_t *rec_cell, const float *rec_w, const float *snap,
                        int32_t snap_first, float *drec_out, float *work, int32_t n_begin, int32_t n_end,
                        int32_t flags, void *stream);

/* Exact discrete adjoint + imaging for k = k_hi down to k_lo (a full run is k_hi = nt-1,
 * k_lo = 1 with MIFWI_ZERO_STATE | MIFWI_FINALIZE).  Step k needs snapshot G^{k-1}, found at
 * snap + (k-1-snap_first)*nshot*n0*gp.
 *   grad_rec [nt][nshot][nrec] = dJ/d rec
 *   grad_r [n0][gp]  (written when MIFWI_FINALIZE; sum over the plan's shots)
 *   grad_f NULL or [nt][nshot][nsrc]
 *   work : layout.work_backward_elems floats (adjoint state + accumulators)                 */
int mifwi_acoustic_backward(mifwi_acoustic_plan *plan, const float *r, const float *q0,
                            const float *q1, const int32_t *src_cell, const float *src_w,
                            const int32_t *rec_cell, const float *rec_w, const float *grad_rec,
                            const float *snap, int32_t snap_first, float *grad_r, float *grad_f,
                            float *work, int32_t k_hi, int32_t k_lo, int32_t flags,
                            void *stream);

/* ======================================================================================
 * 2-D P-SV ELASTIC velocity-stress propagator (forward + exact discrete adjoint)
 *
 * Replaces the DENISE-Black-Edition runs behind pyapi_denise:
 *   d.forward(model, src, rec) / d.grad(model, src, rec)   models/networks.py:7787, 9853-9877
 *   (parameter block 7698-7731 / 9790-9833; gradient read-back 7799-7802)
 *
 * Scheme: standard staggered grid, 4th-order space, leapfrog time,
 * C-PML memory variables on every derivative (layer inside the grid, pml_width nodes),
 * explosive source into sxx/szz, receivers sample vx/vz after the velocity update.
 *   mat [5][nz][gp] = lambda dt/h, (lambda+2mu) dt/h, mu_xz dt/h, dt/(h rho_x), dt/(h rho_z)
 *                     (staggered averages are formed by the host; columns >= nx must be 0)
 *   pz [6][nz], px [6][gp] : C-PML a, b, 1/kappa at integer then at half nodes
 *                     (a = b = 0, 1/kappa = 1 outside the layer and in columns >= nx)
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none); profiles may still be zero
                                on a side (e.g. free surface)                                 */
    int32_t free_surface;    /* 1: stress-imaging free surface on row 0 (DENISE FREE_SURF): szz = 0
                                there, stresses mirrored oddly above it; the caller passes row 0 of
                                mat[0..1] in the effective form (0, M - L^2/M)                    */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive, f added to sxx and szz after S (DENISE QUELLTYPB 1);
                                1 / 2: point force, f added to vx / vz between V and S (QUELLTYPB 2 / 3,
                                pyapi_denise attribute at networks.py:10419-10453).  f arrives scaled by the
                                host in every case; grad_f is the matching adjoint sample.  Force sources
                                run on the one-launch-per-half-step kernels.                          */
    int32_t record_pressure; /* 1: the plan also serves pressure receivers (DENISE SEISMO 2 / 4, adjoint source
                                type QUELLTYPB 4) through mifwi_elastic_plan_bind_pressure; such plans run on
                                the one-launch-per-half-step kernels.                                     */
    int32_t snapshot_format; /* MIFWI_SNAPSHOT_F32 (exact discrete adjoint) or MIFWI_SNAPSHOT_BF16: the five
                                forward snapshot planes are rounded to bf16 on their way to memory (10 instead of
                                20 B per cell-step each way, twice the steps per checkpoint segment; material
                                gradients within 4e-3 rel-L2 of the f32 form in the worst case, seismograms unchanged) - the
                                counterpart of the wavefield compression / decimation DENISE and deepwave apply to
                                their stored fields.  Honoured by plans that run the per-step
                                kernels; single-launch plans keep f32 (layout.snapshot_format says which).     */
    int32_t fd_order;        /* spatial order of the staggered-grid first derivatives (DENISE FD_ORDER, left commented at
                                models/networks.py:10447): 4 (Taylor weights 9/8, -1/24; 0 means 4) or 2 (1, 0).
                                Higher orders need a wider halo than the state layout carries: EINVAL.             */
} mifwi_elastic_desc;

enum { MIFWI_SNAPSHOT_F32 = 0, MIFWI_SNAPSHOT_BF16 = 1 };

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / snapshot / gradient plane           */
    int64_t state_elems;          /* forward state (5 fields + memory variables) at the start
                                     of `work`: what a time checkpoint copies                  */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots)  */
    int32_t snapshot_format;      /* the format this plan writes and reads                          */
    int32_t kernel_flags;         /* MIFWI_EL_KERNEL_*: which formulation of the time loops the plan picked   */
} mifwi_elastic_layout;

/* kernel_flags: forward / adjoint as ONE launch for the whole time loop (LDS-resident slabs), or - on grids that do not
   fit - the forward's V+S fused into one launch per step; neither bit = one launch per half step */
enum { MIFWI_EL_KERNEL_FWD_SINGLE_LAUNCH = 1, MIFWI_EL_KERNEL_ADJ_SINGLE_LAUNCH = 2, MIFWI_EL_KERNEL_FWD_FUSED_STEP = 4,
       MIFWI_EL_KERNEL_ADJ_FUSED_STEP = 8,       /* reserved: no longer set by this library (the adjoint per-step form
                                                    is always two launches per step) */
       /* the single-launch loop takes the outer cells of its x-stencils from the neighbouring lanes (DPP wave shifts)
          instead of misaligned LDS reads: chosen when the plan's deal of groups to lanes allows it */
       MIFWI_EL_KERNEL_FWD_LANE_HALO = 16, MIFWI_EL_KERNEL_ADJ_LANE_HALO = 32 };

typedef struct mifwi_elastic_plan mifwi_elastic_plan;

int mifwi_elastic_plan_create(mifwi_elastic_plan **plan, int device,
                              const mifwi_elastic_desc *desc);
int mifwi_elastic_plan_destroy(mifwi_elastic_plan *plan);
int mifwi_elastic_plan_layout(const mifwi_elastic_plan *plan, mifwi_elastic_layout *out);
/* How the per-step kernels of this plan sweep the time range: shots per forward pass, shot groups per adjoint
 * pass (Infinity Cache residency; nshot / ngroups when everything fits or nothing does).  Introspection only. */
int mifwi_elastic_plan_pass_sizes(const mifwi_elastic_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);

/* Pressure receivers of a plan created with record_pressure = 1 (same cells and weights as the velocity
 * receivers).  The buffers stay bound to the plan until the next call of this function:
 *   rec_p [nt][nshot][nrec] or NULL: mifwi_elastic_forward writes sum w (sxx + szz)[cell], sampled after the
 *         stress update and the source term of each step (DENISE's pressure is its negative);
 *   g_p   [nt][nshot][nrec] or NULL: mifwi_elastic_backward adds w g_p[n] to the adjoint sxx and szz before the
 *         adjoint stress update of step n (the exact transpose of the sampling).                          */
int mifwi_elastic_plan_bind_pressure(mifwi_elastic_plan *plan, float *rec_p, const float *g_p);

/* mifwi_elastic_forward, _backward and _born refuse a plan of mifwi_vti_plan_create, mifwi_tti_plan_create or
 * mifwi_visco_plan_create with MIFWI_EINVAL ("the plan was not created by mifwi_elastic_plan_create"): its kernels read six
 * or eight planes.
 *
 * Steps n = n_begin .. n_end-1.
 *   f [nt][nshot][nsrc] (added to sxx and szz - or to vx / vz, desc.source_type - pre-scaled by the host)
 *   rec_vx, rec_vz [nt][nshot][nrec] or both NULL
 *   snap NULL or [n_end-n_begin][layout.snap_step_elems]: per step and shot the five PML-filtered derivative
 *        sums the material gradient needs (exx', ezz', exz', and the two force terms); f32 format:
 *        [nshot][5][nz][gp]                                                                   */
int mifwi_elastic_forward(mifwi_elastic_plan *plan, const float *mat, const float *pz,
                          const float *px, const float *f, const int32_t *src_cell,
                          const float *src_w, const int32_t *rec_cell, const float *rec_w,
                          float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin,
                          int32_t n_end, int32_t flags, void *stream);

/* Adjoint steps n = n_hi down to n_lo (full run: nt-1 .. 0, ZERO_STATE|FINALIZE).
 *   g_vx, g_vz [nt][nshot][nrec] = dJ/d rec;  snapshot of step n at snap+(n-snap_first)*layout.snap_step_elems
 *   grad_mat [5][nz][gp] (on FINALIZE): dJ/d mat summed over the plan's shots
 *   grad_f NULL or [nt][nshot][nsrc]                                                        */
int mifwi_elastic_backward(mifwi_elastic_plan *plan, const float *mat, const float *pz,
                           const float *px, const int32_t *src_cell, const float *src_w,
                           const int32_t *rec_cell, const float *rec_w, const float *g_vx,
                           const float *g_vz, const float *snap, int32_t snap_first,
                           float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo,
                           int32_t flags, void *stream);

/* Born (linearised) modelling: drec = J (dmat, df), the first-order change of the velocity seismograms, steps
 * n = n_begin .. n_end-1 - the JVP partner of mifwi_elastic_backward's (grad_mat, grad_f).  The perturbed state obeys
 * the forward recursion (same materials, profiles, free surface, stencil order) without the point source; at step n the
 * five snapshot planes S0..S4 of the background run's step n are its virtual sources:
 *   after V:  dvx += dmat[3] S3,  dvz += dmat[4] S4
 *   after S:  dsxx += dmat[1] S0 + dmat[0] S1,  dszz += dmat[0] S0 + dmat[1] S1,  dsxz += dmat[2] S2
 *             (before row 0 of dszz is zeroed under a free surface)
 *   dmat [5][nz][gp]: perturbation of `mat`, same layout (columns >= nx must be 0)
 *   df   NULL or [nt][nshot][nsrc]: perturbation of f, injected as f is
 *   snap: f32 planes as mifwi_elastic_forward of the same plan wrote them (either layout); step n at
 *         snap + (n - snap_first) * layout.snap_step_elems
 *   drec_vx, drec_vz [nt][nshot][nrec] or both NULL, sampled after V as the forward samples
 *   work: layout.work_forward_elems floats; the perturbed state lives at its head (MIFWI_ZERO_STATE as in the forward)
 * Runs on the one-launch-per-half-step kernels whatever family the plan's forward runs.  MIFWI_EINVAL: null dmat / snap /
 * work, a bad step range, plans with bf16 snapshot planes, source_type != 0 (a force source needs df from the density
 * at the source node) and record_pressure plans (pressure receivers are not sampled). */
int mifwi_elastic_born(mifwi_elastic_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                       const float *df, const int32_t *src_cell, const float *src_w,
                       const int32_t *rec_cell, const float *rec_w,
                       const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                       float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream);

/* Which kernel family a plan selected: the number of row slabs a shot is cut
 * into by the single-launch "cluster" time loop, or 0 when the plan runs one launch per (half)
 * step.  `adjoint` = 0 asks about the forward loop, 1 about the adjoint loop.                  */
int mifwi_acoustic_plan_cluster_slabs(const mifwi_acoustic_plan *plan, int32_t adjoint);
int mifwi_elastic_plan_cluster_slabs(const mifwi_elastic_plan *plan, int32_t adjoint);

/* ======================================================================================
 * 2-D P-SV ELASTIC propagator in a medium with VERTICAL TRANSVERSE ISOTROPY (VTI; forward + exact discrete adjoint)
 *
 * Serves pyapi_denise runs with PHYSICS = 3 (this library's number for the P-SV VTI medium; no DENISE table of PHYSICS
 * values is at hand to pin against): Thomsen media, where far-offset kinematics need epsilon and delta.  The elastic
 * scheme above - same grid, staggering, Dp / Dm, C-PML recursion, pz / px tables, free surface, sources, receivers and
 * five snapshot planes - with four stiffnesses instead of lambda, lambda + 2 mu and mu: c11, c13 and c33 on the sxx / szz
 * node, c44 on the sxz node.
 *   mat [6][nz][gp] = c13, c11, c44_xz, dt/(h rho_x), dt/(h rho_z), c33, the stiffnesses times dt/h.  Planes 0..4 stand
 *                     where the elastic lambda, lambda + 2 mu, mu_xz, bx, bz stand; c33 is appended.  Columns >= nx must
 *                     be 0; under a free surface row 0 must hold c13 = 0 and c11 - c13^2 / c33 (szz = 0 there).
 * Forward step n ( ' : through the C-PML; S0..S4 the snapshot planes, as in the elastic scheme):
 *   V:  unchanged (the elastic V launch):  vx = fmaf(bx, d1' + d2', vx), vz = fmaf(bz, d3' + d4', vz);  S3, S4
 *   source_type 1 / 2: vx / vz [cell] += w f[n]
 *   S:  e1 = Dm_x vx, e2 = Dm_z vz, e3 = Dp_z vx, e4 = Dp_x vz;  S0 = e1', S1 = e2', S2 = e3' + e4'
 *       sxx = fmaf(c11, e1', fmaf(c13, e2', sxx));  szz = fmaf(c13, e1', fmaf(c33, e2', szz));  sxz = fmaf(c44, S2, sxz)
 *   source_type 0: sxx, szz [cell] += w f[n];  free surface: szz(0,.) = 0
 * With c33 == c11 every operation is the elastic one: the seismograms of mifwi_elastic_forward bit for bit.
 * Adjoint step n = nt-1 .. 0, the exact transpose (V^T is the elastic launch):
 *   S^T: E1 = pmlT(fmaf(c11, sxx_bar, c13 szz_bar)), E2 = pmlT(fmaf(c13, sxx_bar, c33 szz_bar)), E3 = E4 = pmlT(c44 sxz_bar)
 *        g_c11 += S0 sxx_bar;  g_c33 += S1 szz_bar;  g_c13 = fmaf(S1, sxx_bar, fmaf(S0, szz_bar, g_c13));  g_c44 += S2 sxz_bar
 *        g_bx += S3 vx_bar, g_bz += S4 vz_bar (the new v_bar)
 * Born step: after S  dsxx += dmat[1] S0 + dmat[0] S1,  dszz += dmat[0] S0 + dmat[5] S1,  dsxz += dmat[2] S2; V as elastic.
 * One launch per half step in both directions: there is no single-launch and no fused V+S form, no bf16 snapshot
 * planes and no pressure receivers.  Snapshots are f32 [nshot][5][nz][gp] planes, blocked by columns of 16 four-cell
 * groups; grad_mat and dmat are [6][nz][gp] like mat.
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none)                               */
    int32_t free_surface;    /* 1: stress-free surface on row 0 (needs nz >= 4)               */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive (sxx, szz), 1 / 2: point force on vx / vz        */
    int32_t fd_order;        /* 4 (0 means 4) or 2                                            */
} mifwi_vti_desc;

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / gradient plane                     */
    int64_t state_elems;          /* forward state (5 fields + memory variables) at the start
                                     of `work`: what a time checkpoint copies                 */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots) */
} mifwi_vti_layout;

typedef struct mifwi_vti_plan mifwi_vti_plan;

/* MIFWI_EINVAL as mifwi_elastic_plan_create: nulls, bad sizes, ntap other than 1 or 4, a grid too small for the layer */
int mifwi_vti_plan_create(mifwi_vti_plan **plan, int device, const mifwi_vti_desc *desc);
int mifwi_vti_plan_destroy(mifwi_vti_plan *plan);
int mifwi_vti_plan_layout(const mifwi_vti_plan *plan, mifwi_vti_layout *out);
/* shots per forward pass, shot groups per adjoint pass over the time range (Infinity Cache residency, six planes) */
int mifwi_vti_plan_pass_sizes(const mifwi_vti_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);
/* always 0: the VTI plan runs one launch per half step */
int mifwi_vti_plan_cluster_slabs(const mifwi_vti_plan *plan, int32_t adjoint);

/* Arguments, step ranges, flags and refusals as mifwi_elastic_forward / _backward / _born; mat, grad_mat, dmat
 * [6][nz][gp].  Born is served for source_type 0 only. */
int mifwi_vti_forward(mifwi_vti_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                      const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                      float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                      int32_t flags, void *stream);
int mifwi_vti_backward(mifwi_vti_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                       const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                       const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                       int32_t n_lo, int32_t flags, void *stream);
int mifwi_vti_born(mifwi_vti_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                   const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                   const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                   int32_t n_end, int32_t flags, void *stream);

/* ======================================================================================
 * 2-D P-SV ELASTIC propagator in a medium with a TILTED symmetry axis (TTI; forward + exact discrete adjoint)
 *
 * Serves pyapi_denise runs with PHYSICS = 4 (this library's number for the P-SV TTI medium): Thomsen media whose symmetry
 * axis follows dipping beds.  The VTI scheme above - same grid, staggering, Dp / Dm, C-PML recursion, pz / px tables, free
 * surface, sources, receivers and five snapshot planes - with the stiffnesses rotated by the tilt, which adds c15 and
 * c35: the normal stresses feel the shear strain and the shear stress the normal strains.
 *   mat [8][nz][gp] = c13, c11, c55_xz, dt/(h rho_x), dt/(h rho_z), c33, c15, c35, the stiffnesses times dt/h.  Planes 0..5
 *                     stand where the VTI planes stand; c15 and c35 sit on the sxx node.  Columns >= nx must be 0; under a
 *                     free surface row 0 is kept VTI-like: c13 = c15 = c35 = 0 and c11 - c13^2 / c33 there (no tilted
 *                     surface row; in marine data that row is water, where all three vanish anyway).
 * sxx, szz and S0 = e1', S1 = e2' sit at (j, i); sxz and S2 = e3' + e4' at (j + 1/2, i + 1/2); all strains after their C-PML
 * recursion.  Two four-point averages, entries outside the grid taken as 0:
 *   A,   sxz nodes -> sxx node:  (A q)(j,i)   = 1/4 [q(j,i) + q(j-1,i) + q(j,i-1) + q(j-1,i-1)]
 *   A^T, sxx nodes -> sxz node:  (A^T p)(j,i) = 1/4 [p(j,i) + p(j+1,i) + p(j,i+1) + p(j+1,i+1)]
 * and w = (c55_xz != 0), a 0/1 mask on the sxz node.
 * Forward step n:
 *   V:   unchanged (the elastic V launch); S3, S4.   source_type 1 / 2: vx / vz [cell] += w f[n]
 *   S:   sxx = fmaf(c11, S0, fmaf(c13, S1, sxx)) + c15 A(w S2);  szz = fmaf(c13, S0, fmaf(c33, S1, szz)) + c35 A(w S2)
 *        sxz = fmaf(c55_xz, S2, sxz) + w A^T(c15 S0 + c35 S1)
 *   source_type 0: sxx, szz [cell] += w f[n];  free surface: szz(0,.) = 0
 * The coupling terms are added after the VTI fmaf chain: with c15 = c35 = 0 the seismograms of mifwi_vti_forward on
 * planes 0..5 bit for bit.  The mask is part of the scheme: where the harmonic c55_xz is 0 (a fluid-solid interface)
 * A^T(c15 e1') would drive a shear stress that nothing restores, the stiffness operator becomes indefinite and the run
 * grows without bound; with w the 3 x 3 operator stays symmetric and the runs stay bounded.
 * Adjoint step n = nt-1 .. 0, the exact transpose (the operator is symmetric: the same form on the adjoint stresses):
 *   S^T: e1_bar = c11 sxx_bar + c13 szz_bar + c15 A(w sxz_bar);  e2_bar = c13 sxx_bar + c33 szz_bar + c35 A(w sxz_bar)
 *        e5_bar = c55_xz sxz_bar + w A^T(c15 sxx_bar + c35 szz_bar);  then the transposed C-PML and the stencils as elastic
 *        g_c15 += sxx_bar A(w S2) + S0 A(w sxz_bar);  g_c35 += szz_bar A(w S2) + S1 A(w sxz_bar);  planes 0..5 as VTI
 *        (w is a constant for every derivative)
 * Born step: dmat[0..7] on S0..S2 of the background run in the same pattern, w from the background c55_xz.
 * A node needs its neighbours' C-PML-corrected strains, so the stress half step is two launches (strains, then stresses)
 * and so is its transpose; V and V^T are one each.  No single-launch and no fused V+S form, no bf16 snapshot planes, no
 * pressure receivers.  Snapshots are f32 [nshot][5][nz][gp] planes, blocked by columns of 16 four-cell groups;
 * work_forward_elems and work_backward_elems hold three more planes per shot than a VTI plan's (the strains between the two
 * launches); grad_mat and dmat are [8][nz][gp] like mat.
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none)                               */
    int32_t free_surface;    /* 1: stress-free surface on row 0 (needs nz >= 4)               */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive (sxx, szz), 1 / 2: point force on vx / vz        */
    int32_t fd_order;        /* 4 (0 means 4) or 2                                            */
} mifwi_tti_desc;

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / gradient plane                     */
    int64_t state_elems;          /* forward state (5 fields + memory variables) at the start
                                     of `work`: what a time checkpoint copies                 */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots) */
} mifwi_tti_layout;

typedef struct mifwi_tti_plan mifwi_tti_plan;

/* MIFWI_EINVAL as mifwi_elastic_plan_create: nulls, bad sizes, ntap other than 1 or 4, a grid too small for the layer */
int mifwi_tti_plan_create(mifwi_tti_plan **plan, int device, const mifwi_tti_desc *desc);
int mifwi_tti_plan_destroy(mifwi_tti_plan *plan);
int mifwi_tti_plan_layout(const mifwi_tti_plan *plan, mifwi_tti_layout *out);
/* shots per forward pass, shot groups per adjoint pass over the time range (Infinity Cache residency, eight planes) */
int mifwi_tti_plan_pass_sizes(const mifwi_tti_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);
/* always 0: the TTI plan runs one launch per half-step phase */
int mifwi_tti_plan_cluster_slabs(const mifwi_tti_plan *plan, int32_t adjoint);

/* Arguments, step ranges, flags and refusals as mifwi_elastic_forward / _backward / _born; mat, grad_mat, dmat
 * [8][nz][gp].  Born is served for source_type 0 only. */
int mifwi_tti_forward(mifwi_tti_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                      const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                      float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                      int32_t flags, void *stream);
int mifwi_tti_backward(mifwi_tti_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                       const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                       const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                       int32_t n_lo, int32_t flags, void *stream);
int mifwi_tti_born(mifwi_tti_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                   const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                   const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                   int32_t n_end, int32_t flags, void *stream);

/* ======================================================================================
 * 2-D P-SV VISCOELASTIC propagator: one relaxation mechanism of a generalised standard linear solid (forward + exact
 * discrete adjoint)
 *
 * Serves pyapi_denise runs with PHYSICS = 1 and L = 1 (FL1, Qp / Qs models).  The elastic scheme above - same grid,
 * staggering, Dp / Dm, C-PML recursion, pz / px tables, free surface, sources, receivers and five snapshot planes - with
 * three memory variables per shot, rxx and rzz on the sxx node and rxz on the sxz node, which hold dt times DENISE's r.
 *   mat [8][nz][gp] = lam_u, lam2mu_u, mu_u_xz, dt/(h rho_x), dt/(h rho_z), R2, R1, rmu_xz: the UNRELAXED moduli where the
 *                     elastic ones stand, then R2 = pi_r tau_p - 2 mu_r tau_s, R1 = pi_r tau_p on the sxx node and
 *                     mu_r tau_s on the sxz node, all moduli times dt/h.  Columns >= nx must be 0; under a free surface
 *                     row 0 holds the effective form (lam_u = 0, R2 = 0; physicsbasedfwi2_amd.visco.materials).
 *   relax_a = (2 - eta) / (2 + eta), relax_b = 2 eta / (2 + eta) with eta = dt / tau_sigma = 2 pi FL dt, computed in double.
 * Forward step n ( ' : through the C-PML; S0..S4 the snapshot planes, as in the elastic scheme):
 *   V:  unchanged (the elastic V launch); S3, S4.   source_type 1 / 2: vx / vz [cell] += w f[n]
 *   S:  S0 = e1', S1 = e2', S2 = e3' + e4' as elastic;  qxx = R1 S0 + R2 S1, qzz = R2 S0 + R1 S1, qxz = rmu_xz S2
 *       sxx = fmaf(lam2mu_u, S0, fmaf(lam_u, S1, sxx)) + ((1 + a)/2 rxx - b/2 qxx)     (szz, sxz alike)
 *       r*  = a r* - b q*
 *   source_type 0: sxx, szz [cell] += w f[n];  free surface: szz(0,.) = 0
 * With planes 5..7 zero the memory variables stay 0 and every stress is the elastic fmaf chain's: the seismograms of
 * mifwi_elastic_forward (per-step kernels) bit for bit.
 * Adjoint step n = nt-1 .. 0, the exact transpose (r_bar: the adjoint memory variables, in the three extra fields):
 *   S^T: w* = -b (r*_bar + s*_bar / 2);  E1 = pmlT(lam2mu_u sxx_bar + lam_u szz_bar + R1 wxx + R2 wzz), E2 alike,
 *        E3 = E4 = pmlT(mu_u_xz sxz_bar + rmu_xz wxz);  v_bar -= stencils(E)
 *        gradients of planes 0..4 as elastic;  g_R1 += S0 wxx + S1 wzz;  g_R2 += S1 wxx + S0 wzz;  g_rmu += S2 wxz
 *   V^T: r*_bar = a r*_bar + (1 + a)/2 s*_bar with the s_bar that S^T saw, then s_bar -= stencils(D) as elastic
 *        (S^T reads r_bar of neighbouring cells for its halo, so the launch that advances it is V^T)
 * Born step: q* += dmat[5..7] times S0..S2 in the same pattern, the stresses += dmat[0..2] terms as elastic.
 * One launch per half step in both directions: no single-launch and no fused V+S form, no bf16 snapshot planes, no
 * pressure receivers.  The state of a shot is eight fields: time checkpoints (state_elems) carry the memory variables.
 * grad_mat and dmat are [8][nz][gp] like mat.
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none)                               */
    int32_t free_surface;    /* 1: stress-free surface on row 0 (needs nz >= 4)               */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive (sxx, szz), 1 / 2: point force on vx / vz        */
    int32_t fd_order;        /* 4 (0 means 4) or 2                                            */
    float relax_a, relax_b;  /* the two relaxation scalars, each inside (0, 1)                */
} mifwi_visco_desc;

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / gradient plane                     */
    int64_t state_elems;          /* forward state (8 fields + C-PML memory variables) at the start
                                     of `work`: what a time checkpoint copies                 */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots) */
} mifwi_visco_layout;

typedef struct mifwi_visco_plan mifwi_visco_plan;

/* MIFWI_EINVAL as mifwi_elastic_plan_create, and for relax_a or relax_b outside (0, 1) */
int mifwi_visco_plan_create(mifwi_visco_plan **plan, int device, const mifwi_visco_desc *desc);
int mifwi_visco_plan_destroy(mifwi_visco_plan *plan);
int mifwi_visco_plan_layout(const mifwi_visco_plan *plan, mifwi_visco_layout *out);
/* shots per forward pass, shot groups per adjoint pass over the time range (Infinity Cache residency, eight planes) */
int mifwi_visco_plan_pass_sizes(const mifwi_visco_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);
/* always 0: the viscoelastic plan runs one launch per half step */
int mifwi_visco_plan_cluster_slabs(const mifwi_visco_plan *plan, int32_t adjoint);

/* Arguments, step ranges, flags and refusals as mifwi_elastic_forward / _backward / _born; mat, grad_mat, dmat
 * [8][nz][gp].  Born is served for source_type 0 only. */
int mifwi_visco_forward(mifwi_visco_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                        const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                        float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                        int32_t flags, void *stream);
int mifwi_visco_backward(mifwi_visco_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                         const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                         const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                         int32_t n_lo, int32_t flags, void *stream);
int mifwi_visco_born(mifwi_visco_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                     const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                     const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                     int32_t n_end, int32_t flags, void *stream);

/* ======================================================================================
 * 2-D variable-density ACOUSTIC (fluid) velocity-pressure propagator (forward + exact discrete adjoint)
 *
 * Serves the DENISE runs with PHYSICS = 2 behind pyapi_denise (models/networks.py:10445-10453: an acoustic medium
 * driven by a point force) with the fields the physics has: the elastic scheme above with Vs = 0, where
 * sxx = szz = p and sxz = 0.  Same grid, staggering, Dp / Dm, C-PML recursion and pz / px tables as the elastic
 * propagator; its seismograms are the elastic ones on mat = [K, K, 0, bx, bz] bit for bit.
 *   state per shot: vx, vz, p and four memory variables (x strips: d1 @half, e1 @int; z strips: d4 @half, e2 @int)
 *   mat [3][nz][gp] = K dt/h, dt/(h rho_x), dt/(h rho_z), K = rho Vp^2 (columns >= nx must be 0; under a free
 *                     surface row 0 of K must be 0)
 * Forward step n ( ' : through the C-PML; S0..S2: the snapshot planes):
 *   free surface: p(-1,.) = -p(1,.)
 *   V:  d1 = Dp_x p, d4 = Dp_z p;  vx = fmaf(bx, d1', vx), vz = fmaf(bz, d4', vz);  S1 = d1', S2 = d4'
 *   source_type 1 / 2: vx / vz [cell] += w f[n]
 *   P:  e1 = Dm_x vx, e2 = Dm_z vz;  p = fmaf(K, e1', fmaf(K, e2', p));  S0 = e1' + e2'
 *   source_type 0: p[cell] += w f[n];  free surface: p(0,.) = 0
 *   receivers: rec_vx, rec_vz = sum fmaf(w, v, .), rec_p = sum fmaf(w, p + p, .)  (the elastic sxx + szz; DENISE's
 *   pressure is -rec_p)
 * Adjoint step n = nt-1 .. 0, the exact transpose:
 *   vx_bar += w g_vx, vz_bar += w g_vz, p_bar += 2 w g_p;  free surface: p_bar(0,.) = 0
 *   source_type 0: grad_f[n] = sum w p_bar
 *   P^T: acc_K += S0 p_bar;  E1, E2 = pmlT(K p_bar) with the x / z tables at integer nodes;
 *        vx_bar -= Dp_x E1, vz_bar -= Dp_z E2
 *   source_type 1 / 2: grad_f[n] = sum w vx_bar / vz_bar
 *   V^T: acc_bx += S1 vx_bar, acc_bz += S2 vz_bar;  D1, D4 = pmlT(bx vx_bar), pmlT(bz vz_bar) with the x / z tables at
 *        half nodes;  p_bar -= Dm_x D1 + Dm_z D4;  free surface: p_bar(1,.) += C2 D4(0,.)
 * One launch per half step in both directions; there is no single-launch form.
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none)                               */
    int32_t free_surface;    /* 1: pressure-free surface on row 0 (needs nz >= 3)             */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive (p), 1 / 2: point force on vx / vz               */
    int32_t fd_order;        /* 4 (0 means 4) or 2                                            */
} mifwi_fluid_desc;

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / gradient plane                     */
    int64_t state_elems;          /* forward state (3 fields + memory variables) at the start
                                     of `work`: what a time checkpoint copies                 */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots): three f32 planes
                                     per shot, blocked by columns of 16 four-cell groups      */
} mifwi_fluid_layout;

typedef struct mifwi_fluid_plan mifwi_fluid_plan;

int mifwi_fluid_plan_create(mifwi_fluid_plan **plan, int device, const mifwi_fluid_desc *desc);
int mifwi_fluid_plan_destroy(mifwi_fluid_plan *plan);
int mifwi_fluid_plan_layout(const mifwi_fluid_plan *plan, mifwi_fluid_layout *out);
/* shots per forward pass, shot groups per adjoint pass over the time range (Infinity Cache residency) */
int mifwi_fluid_plan_pass_sizes(const mifwi_fluid_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);
/* always 0: the fluid plan runs one launch per half step */
int mifwi_fluid_plan_cluster_slabs(const mifwi_fluid_plan *plan, int32_t adjoint);

/* Steps n = n_begin .. n_end-1; arguments as mifwi_elastic_forward.
 *   rec_vx, rec_vz [nt][nshot][nrec] or both NULL;  rec_p [nt][nshot][nrec] or NULL
 *   snap NULL or [n_end-n_begin][layout.snap_step_elems]
 *   work: layout.work_forward_elems floats, the state (layout.state_elems) at its head.  The calls take no buffer sizes:
 *         that `work` (here and in mifwi_fluid_backward: layout.work_backward_elems floats), `snap` and the outputs are
 *         large enough is the caller's to ensure and is NOT checked.                            */
int mifwi_fluid_forward(mifwi_fluid_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                        const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                        float *rec_vx, float *rec_vz, float *rec_p, float *snap, float *work, int32_t n_begin,
                        int32_t n_end, int32_t flags, void *stream);

/* Adjoint steps n = n_hi down to n_lo (full run: nt-1 .. 0, ZERO_STATE|FINALIZE); ranges, snap_first and flags as in
 * mifwi_elastic_backward.
 *   g_vx, g_vz, g_p [nt][nshot][nrec] = dJ/d rec, each NULL = zero
 *   grad_mat [3][nz][gp] (on FINALIZE): dJ/d mat summed over the plan's shots, shot groups added in order
 *   grad_f NULL or [nt][nshot][nsrc]                                                            */
int mifwi_fluid_backward(mifwi_fluid_plan *plan, const float *mat, const float *pz, const float *px,
                         const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                         const float *g_vx, const float *g_vz, const float *g_p, const float *snap, int32_t snap_first,
                         float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo, int32_t flags,
                         void *stream);

/* Born (linearised) modelling with the fluid kernels: drec = J (dmat, df), the first-order change of the three
 * seismograms, steps n = n_begin .. n_end-1 - the JVP partner of mifwi_fluid_backward's (grad_mat, grad_f).  The perturbed
 * state (dvx, dvz, dp) and its four memory variables obey the forward recursion above (same mat, pz / px, free surface
 * with dp(-1,.) = -dp(1,.) and dp(0,.) = 0, fd_order); the three snapshot planes S0..S2 the background run saved at
 * step n are its virtual sources.  Perturbed step n, the chain of each update:
 *   V:  dvx = fmaf(dmat[1], S1, fmaf(bx, d1', dvx)),  dvz = fmaf(dmat[2], S2, fmaf(bz, d4', dvz))   (d1, d4 of dp)
 *   source_type 1 / 2: dvx / dvz [cell] += w df[n]
 *   P:  dp = fmaf(dmat[0], S0, fmaf(K, e1', fmaf(K, e2', dp)))                                        (e1, e2 of dvx, dvz)
 *   source_type 0: dp[cell] += w df[n];  free surface: dp(0,.) = 0
 *   dmat [3][nz][gp]: perturbation of `mat`, same layout (columns >= nx must be 0)
 *   df   NULL or [nt][nshot][nsrc]: perturbation of f, injected exactly where f is for all three source types (for a
 *        force source the caller differentiates its own amplitude scaling)
 *   snap: the planes as mifwi_fluid_forward of the same plan wrote them; step n at
 *         snap + (n - snap_first) * layout.snap_step_elems.  They are read with 16-byte loads, none is written.
 *   drec_vx, drec_vz [nt][nshot][nrec] or both NULL; drec_p NULL or [nt][nshot][nrec] = sum w (dp + dp): sampled as the
 *         forward samples rec_vx, rec_vz and rec_p
 *   work: layout.work_forward_elems floats; the perturbed state lives at its head (MIFWI_ZERO_STATE as in the forward)
 * The same tiles, launch order and Infinity Cache passes as the forward (a compile-time variant of its two kernels).
 * MIFWI_EINVAL: null dmat / snap / work, a bad step range, snap_first < 0 or > n_begin. */
int mifwi_fluid_born(mifwi_fluid_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                     const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell,
                     const float *rec_w, const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                     float *drec_p, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream);

/* Second moments of the fluid snapshot planes, the ingredient of mifwi_fluid_pseudo_hessian:
 *   moments [3][nz][gp]:  M0 = sum S0^2,  M1 = sum S1^2,  M2 = sum S2^2   (each term fmaf(S, S, M))
 * per cell over the plan's shots and the steps n in [n_begin, n_end) with n % stride == 0, each weighted by stride.
 * Arguments, ranges, flags, alignment and refusals as mifwi_elastic_snapshot_moments; work:
 * mifwi_fluid_snapshot_moments_work_elems(plan) floats.  One thread owns one 4-cell group, the pad groups of the last
 * column block are never read; partial planes of the step range are added in a fixed order: no atomics, two identical
 * calls give the same bits. */
int64_t mifwi_fluid_snapshot_moments_work_elems(const mifwi_fluid_plan *plan);
int mifwi_fluid_snapshot_moments(mifwi_fluid_plan *plan, const float *snap, int32_t snap_first, int32_t n_begin,
                                 int32_t n_end, int32_t stride, float *moments, float *work, int32_t flags, void *stream);

/* ======================================================================================
 * 2-D VISCOACOUSTIC fluid propagator: one relaxation mechanism of a standard linear solid on the fluid kernels (forward +
 * exact discrete adjoint + Born)
 *
 * Serves pyapi_denise runs with PHYSICS = 2, acoustic_kernels = "fluid" and L = 1 (FL1, a Qp model): marine field data whose
 * amplitudes a lossless medium cannot match.  The fluid scheme above - same grid, staggering, Dp / Dm, C-PML recursion,
 * pz / px tables, free surface, sources, receivers (rec_p included) and three snapshot planes - with one memory variable per
 * shot, r on the p node, which holds dt times DENISE's r; equally the viscoelastic scheme with Vs = 0, where rxx = rzz = r,
 * sxx = szz = p and sxz = rxz = 0.
 *   state per shot: vx, vz, p, r and the four C-PML memory variables of the fluid plan
 *   mat [4][nz][gp] = K_u dt/h, dt/(h rho_x), dt/(h rho_z), R dt/h with the UNRELAXED K_u = pi_r (1 + tau_p) where K
 *                     stands, and R = pi_r tau_p (pi_r = rho vp^2 / (1 + s tau_p), tau_p = 2 / qp;
 *                     physicsbasedfwi2_amd.viscofluid.materials).  Columns >= nx must be 0; under a free surface row 0
 *                     of planes 0 and 3 must be 0.
 *   relax_a = (2 - eta) / (2 + eta), relax_b = 2 eta / (2 + eta) with eta = dt / tau_sigma = 2 pi FL dt, computed in double.
 * Forward step n: the fluid step, except
 *   P:  e1, e2, S0 = e1' + e2' as fluid;  q = fmaf(R, e1', R * e2')
 *       p = fmaf(K_u, e1', fmaf(K_u, e2', p)) + fmaf((1 + a)/2, r, -(b/2 * q))
 *       r = fmaf(a, r, -(b * q))
 *   source_type 0: p[cell] += w f[n] after the memory term;  free surface: p(0,.) = 0
 * With plane 3 zero r stays 0 and p is the fluid fmaf chain's: the three seismograms of mifwi_fluid_forward bit for bit.
 * On the planes of a model with Vs = 0 the operand order is that of mifwi_visco_forward: rec_vx, rec_vz are its bits.
 * Adjoint step n = nt-1 .. 0, the exact transpose (r_bar: the adjoint memory variable, in the fourth field):
 *   P^T: free surface: p_bar(0,.) = 0 first;  w = -b (r_bar + p_bar / 2);  acc_K += S0 p_bar,  acc_R += S0 w;
 *        E1, E2 = pmlT(K_u p_bar + R w);  vx_bar -= Dp_x E1, vz_bar -= Dp_z E2
 *   V^T: r_bar = a r_bar + (1 + a)/2 p_bar with the p_bar that P^T saw, then p_bar -= stencils(D) as fluid
 *        (P^T reads r_bar of neighbouring cells for its halo, so the launch that advances it is V^T)
 * Born step: q += dmat[3] S0, so that both p and r carry it; p += dmat[0] S0 and the V launch as fluid.
 * One launch per half step in both directions.  The state of a shot is four fields: time checkpoints (state_elems) carry
 * the memory variable.  grad_mat and dmat are [4][nz][gp] like mat.  The handle types are kept apart: mifwi_fluid_forward /
 * _backward / _born / _snapshot_moments refuse a viscoacoustic plan and the calls below a lossless one (MIFWI_EINVAL,
 * before any other argument is read).
 * ==================================================================================== */
typedef struct {
    int32_t nz, nx;          /* grid, z = depth is the slow axis                              */
    int32_t nt, nshot, nsrc, nrec, ntap;
    int32_t pml_width;       /* C-PML nodes per side (0 = none)                               */
    int32_t free_surface;    /* 1: pressure-free surface on row 0 (needs nz >= 3)             */
    int32_t shots_per_group; /* adjoint: shots sharing one gradient accumulator; 0 = auto     */
    int32_t source_type;     /* 0: explosive (p), 1 / 2: point force on vx / vz               */
    int32_t fd_order;        /* 4 (0 means 4) or 2                                            */
    float relax_a, relax_b;  /* the two relaxation scalars, each inside (0, 1)                */
} mifwi_viscofluid_desc;

typedef struct {
    int32_t gp, pitch, ngroups, shots_per_group;
    int64_t coef_elems;           /* nz*gp: one material / gradient plane                     */
    int64_t state_elems;          /* forward state (4 fields + C-PML memory variables) at the start
                                     of `work`: what a time checkpoint copies                 */
    int64_t work_forward_elems;
    int64_t work_backward_elems;
    int64_t snap_step_elems;      /* floats one time step of the snapshot buffer takes (all shots): three f32 planes
                                     per shot, as in the fluid plan                           */
} mifwi_viscofluid_layout;

typedef struct mifwi_viscofluid_plan mifwi_viscofluid_plan;

/* MIFWI_EINVAL as mifwi_fluid_plan_create, and for relax_a or relax_b outside (0, 1) */
int mifwi_viscofluid_plan_create(mifwi_viscofluid_plan **plan, int device, const mifwi_viscofluid_desc *desc);
int mifwi_viscofluid_plan_destroy(mifwi_viscofluid_plan *plan);
int mifwi_viscofluid_plan_layout(const mifwi_viscofluid_plan *plan, mifwi_viscofluid_layout *out);
/* shots per forward pass, shot groups per adjoint pass over the time range (Infinity Cache residency, four fields and planes) */
int mifwi_viscofluid_plan_pass_sizes(const mifwi_viscofluid_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups);
/* always 0: the viscoacoustic plan runs one launch per half step */
int mifwi_viscofluid_plan_cluster_slabs(const mifwi_viscofluid_plan *plan, int32_t adjoint);

/* Arguments, step ranges, flags and refusals as mifwi_fluid_forward / _backward / _born; mat, grad_mat, dmat [4][nz][gp].
 * Born is served for all three source types. */
int mifwi_viscofluid_forward(mifwi_viscofluid_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                             const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                             float *rec_vx, float *rec_vz, float *rec_p, float *snap, float *work, int32_t n_begin,
                             int32_t n_end, int32_t flags, void *stream);
int mifwi_viscofluid_backward(mifwi_viscofluid_plan *plan, const float *mat, const float *pz, const float *px,
                              const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                              const float *g_vx, const float *g_vz, const float *g_p, const float *snap,
                              int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo,
                              int32_t flags, void *stream);
int mifwi_viscofluid_born(mifwi_viscofluid_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                          const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell,
                          const float *rec_w, const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                          float *drec_p, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream);

/* ======================================================================================
 * Diagonal PSEUDO-HESSIAN of the elastic gradient (Shin's preconditioner)
 *
 * Serves: DENISE's EPRECOND = 1 / EPSILON_WE, reachable through pyapi_denise as every DENISE parameter is.  The
 * reference's parameter blocks (models/networks.py:7698-7731, 9790-9833) never set the switch; what stands in its
 * place there is the host heuristic of models/networks.py:7808-7862 (mute rows 0:25, rescale every plane to
 * max(model)/max(gradient)), needed because the raw gradient is dominated by the cells around the sources.  The
 * DENISE binary is not available to pin against: the definitions below are this library's documented choice.
 *
 * The five planes S0..S4 a forward step saves for the adjoint (exx', ezz', exz', the two force sums) are the virtual
 * sources of the five material planes; the pseudo-Hessian is their energy summed over time and shots, so it needs no
 * extra propagation, only one more read of the snapshot buffer.
 *
 * MOMENTS  [6][nz][gp], per cell summed over the plan's shots and the selected steps:
 *   M0..M4 = sum Sk^2,   M5 = sum S0 S1
 * A perturbation (dL, dM, dmu, db) of the collocated materials L = lambda s, M = (lambda + 2 mu) s, mu s, b = s / rho
 * (s = dt/h) excites the virtual source (S1 dL + S0 dM, S0 dL + S1 dM, S2 dmu, S3 db, S4 db) in the sxx / szz / sxz /
 * vx / vz equations; for a parameter p with pointwise partials (L_p, M_p, mu_p, b_p) the pseudo-Hessian is the summed
 * squared norm of that vector:
 *   H_p = (L_p^2 + M_p^2)(M0 + M1) + 4 L_p M_p M5 + mu_p^2 M2 + b_p^2 (M3 + M4)
 * (the cross moment M5 because Vp, rho and lambda each move L and M together).  Partials:
 *   VELOCITY   Vp:     (2 rho Vp s, 2 rho Vp s, 0, 0)    Vs: (-4 rho Vs s, 0, 2 rho Vs s, 0)
 *              rho:    ((Vp^2 - 2 Vs^2) s, Vp^2 s, Vs^2 s, -s / rho^2)
 *   IMPEDANCE  Zp:     (2 Vp s, 2 Vp s, 0, 0)            Zs: (-4 Vs s, 0, 2 Vs s, 0)
 *              rho:    (-(Vp^2 - 2 Vs^2) s, -Vp^2 s, -Vs^2 s, -s / rho^2)
 *   LAME       lambda: (s, s, 0, 0)                      mu: (0, 2 s, s, 0)
 *              rho:    (0, 0, 0, -s / rho^2)
 * A term whose divisor is zero contributes 0 (the convention of mifwi_elastic_gradient_parametrization).
 * This is a COLLOCATED approximation: the staggered averages of the material planes, the harmonic mu_xz and the
 * effective row 0 under a free surface are ignored.
 * ==================================================================================== */
int64_t mifwi_elastic_snapshot_moments_work_elems(const mifwi_elastic_plan *plan);
/* steps n in [n_begin, n_end) with n % stride == 0 (absolute n: a range may be cut anywhere), each weighted by
   stride; step n at snap + (n - snap_first) * layout.snap_step_elems; MIFWI_ZERO_STATE: overwrite, else add.
   snap: as written by mifwi_elastic_forward of the same plan (any of its layouts).  moments [6][nz][gp] row-major,
   columns >= nx written as 0.  work: mifwi_elastic_snapshot_moments_work_elems(plan) floats (partial planes of the
   step range, added in a fixed order: no atomics, two identical calls give the same bits).  stride < 1, an empty or
   reversed range: MIFWI_EINVAL. */
int mifwi_elastic_snapshot_moments(mifwi_elastic_plan *plan, const float *snap, int32_t snap_first,
                                   int32_t n_begin, int32_t n_end, int32_t stride, float *moments,
                                   float *work, int32_t flags, void *stream);

/* ======================================================================================
 * Fused data MISFIT + adjoint source (what sits between the propagator call and .backward())
 *
 * Replaces:
 *   L1_TRACE_NORM  models/networks.py:5418-5419 (observed side), 5467-5476, 5491 (predicted side):
 *                  d = pred - direct;  dn = d / (max_t |d| + 1e-10);  loss = mean |dn - obs|
 *   L2             seisgan/fwi/layers.py:176-178; DENISE lnorm = 2 (models/networks.py:7758):
 *                  loss = 1/2 sum (pred - obs)^2
 *   GLOBAL_CORRELATION  DENISE's global-correlation norm, selectable through add_fwi_stage(lnorm=...)
 *                  (models/networks.py:9863, 10503 pass lnorm): loss = - sum_traces <pred, obs> / (|pred| |obs|)
 * pred, obs, direct (NULL = none; L1 only), adj_out (NULL = loss only): [nt][ntrace] with
 * trace = shot*nrec + receiver, the propagators' own output layout.  adj_out = dloss/dpred
 * (including the path through each trace's maximum).  loss_out: one device float.
 * work: mifwi_misfit_work_elems(kind, nt, ntrace) floats, 8-byte aligned.
 * ==================================================================================== */
enum { MIFWI_MISFIT_L1_TRACE_NORM = 0, MIFWI_MISFIT_L2 = 1, MIFWI_MISFIT_GLOBAL_CORRELATION = 2 };

int64_t mifwi_misfit_work_elems(int32_t kind, int64_t nt, int64_t ntrace);
int mifwi_misfit(int device, int32_t kind, const float *pred, const float *obs, const float *direct,
                 int64_t nt, int64_t ntrace, float *loss_out, float *adj_out, float *work, void *stream);

/* ======================================================================================
 * STAGE FILTER of the elastic protocol, alone and fused with the objective that follows it
 *
 * Replaces what DENISE does with the corners of the last frequency stage: every prop() that calls d.grad() first calls
 * add_fwi_stage(fc_high=...) or add_fwi_stage(fc_low=..., fc_high=...) (models/networks.py:6374, 6738, 7116, 7761, 8432,
 * 9147, 9863, 10503, 11070, 11676); the modelled and the observed traces are filtered along time with a causal recursive
 * Butterworth filter F before the misfit, and the adjoint sources with its transpose.
 * F: a cascade of nsec second-order sections run with zero initial state in transposed direct form II,
 *     y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y;   (x of the next section = y)
 * i.e. scipy.signal.sosfilt; F^T is the same recurrence from the last sample to the first.  Coefficients and state are
 * double, traces float.  sos: HOST array [nsec][6], rows b0 b1 b2 a0 a1 a2 as scipy.signal.butter(..., output="sos") emits
 * them; a0 must be 1; a first-order section is a row with b2 = a2 = 0 (an odd order's rows with a2 = 0 or b2 = 0
 * need no special case).  Every other pointer is a device pointer.
 *   mifwi_trace_filter     y = F x (transpose != 0: y = F^T x); x, y [nt][ntrace]; y == x allowed
 *   mifwi_misfit_filtered  one launch for loss and adjoint source of the filtered traces:
 *     L2                  r = F(pred - obs) rounded to float;  loss = 1/2 sum r^2;  adj_out = F^T r
 *     GLOBAL_CORRELATION  s = F pred, o = F obs rounded to float;  loss = - sum_traces <s, o> / (|s| |o|);
 *                         adj_out = F^T(dloss/ds)  (a trace with |s| = 0 or |o| = 0 contributes nothing, adj_out 0)
 *     pred, obs, adj_out (NULL = loss only, the same bits), loss_out as for mifwi_misfit; no atomics, fixed summation
 *     order: two identical calls give the same bits.  work: mifwi_misfit_filtered_work_elems(kind, nt, ntrace) floats,
 *     8-byte aligned (GLOBAL_CORRELATION keeps F obs there between its two sweeps).
 * MIFWI_EINVAL: a null argument, nsec < 1 or > MIFWI_FILTER_MAX_SECTIONS, a0 != 1, a coefficient that is not finite,
 * kind L1_TRACE_NORM (the acoustic protocol has no stage), work not 8-byte aligned, sizes as mifwi_misfit rejects them.
 * ==================================================================================== */
enum { MIFWI_FILTER_MAX_SECTIONS = 8 };

int mifwi_trace_filter(int device, const float *x, float *y, int64_t nt, int64_t ntrace, const double *sos,
                       int32_t nsec, int32_t transpose, void *stream);
int64_t mifwi_misfit_filtered_work_elems(int32_t kind, int64_t nt, int64_t ntrace);
int mifwi_misfit_filtered(int device, int32_t kind, const float *pred, const float *obs, int64_t nt,
                          int64_t ntrace, const double *sos, int32_t nsec, float *loss_out, float *adj_out,
                          float *work, void *stream);

/* ======================================================================================
 * TRACE SELECTION inside the misfit kernels: trace kill, trace weights and time windows
 *
 * Replaces what DENISE does with TRKILL (a table of dead channels) and TIMEWIN (a window around picked times with a Gaussian
 * taper, GAMMA) when the data are a field survey (AutoRealData, models/networks.py:10321-10540): samples leave the objective,
 * not the arrays.  This library's documented choice (DENISE's binary is not available to pin against): the diagonal operator
 *     w[t, tr] = a[tr] g(t; t_on[tr], t_off[tr], gamma),   d = max(t_on - t, t - t_off, 0),   g = d == 0 ? 1 : exp(-gamma d^2)
 * with t the sample index, evaluated in double from the float inputs.
 *   trace_w  device [ntrace] or NULL (= 1): a >= 0 and finite; 0 kills the trace
 *   t_on, t_off  device [ntrace], both or neither (NULL = no window, g = 1): in samples, may lie outside [0, nt - 1] and
 *            may be reversed (t_on > t_off: no sample is inside)
 *   gamma    >= 0 per sample^2; +inf is a boxcar
 * W is applied after the stage filter F (the identity when nsec == 0) and before the norm:
 *   L2                  r = float(W F(pred - obs));  loss = 1/2 sum r^2;  adj_out = float(F^T W r)
 *   GLOBAL_CORRELATION  s = float(W F pred), o = float(W F obs);  loss = - sum_traces <s, o> / (|s| |o|);
 *                       adj_out = float(F^T W dloss/ds)  (a trace with |s| = 0 or |o| = 0 contributes nothing, adj_out 0)
 * W selects, it does not multiply: where w == 0 exactly the sample's value is not used.  A KILLED trace (a == 0) may hold
 * anything in pred and obs, NaN and Inf included: its loss contribution and its adj_out column are exactly 0.  Inside a
 * live trace there is no such guarantee (a NaN stays in the state of the recursive filter).
 *   mifwi_misfit_selected  sos (HOST) and nsec as for mifwi_misfit_filtered, or sos == NULL and nsec == 0: no stage.
 *     pred, obs, loss_out, adj_out (NULL = loss only, the same bits) as for mifwi_misfit; no atomics, fixed summation order.
 *     work: mifwi_misfit_selected_work_elems(kind, nt, ntrace, nsec) floats, 8-byte aligned.
 *     trace_w, t_on and t_off all NULL: the call IS mifwi_misfit_filtered / mifwi_misfit (the same kernels, the same bits).
 *   mifwi_trace_window     y = W x; x, y [nt][ntrace]; y == x allowed
 * MIFWI_EINVAL: exactly one of t_on / t_off NULL, gamma negative or NaN, sos NULL with nsec != 0 or the reverse, kind
 * L1_TRACE_NORM, and everything mifwi_misfit_filtered rejects.  The values of trace_w are the caller's to check (they are
 * on the device; misfit.TraceSelection validates them once on the host).
 * ==================================================================================== */
int64_t mifwi_misfit_selected_work_elems(int32_t kind, int64_t nt, int64_t ntrace, int32_t nsec);
int mifwi_misfit_selected(int device, int32_t kind, const float *pred, const float *obs, int64_t nt, int64_t ntrace,
                          const double *sos /* host, NULL iff nsec == 0 */, int32_t nsec,
                          const float *trace_w, const float *t_on, const float *t_off, double gamma,
                          float *loss_out, float *adj_out, float *work, void *stream);
int mifwi_trace_window(int device, const float *x, float *y, int64_t nt, int64_t ntrace,
                       const float *trace_w, const float *t_on, const float *t_off, double gamma, void *stream);

/* ======================================================================================
 * MATCHING FILTER: source-wavelet estimation in front of the objective (DENISE's INV_STF)
 *
 * Replaces what DENISE does with INV_STF = 1 (libstfinv): per shot, the filter that best maps the modelled seismograms onto
 * the recorded ones, carried through the objective.  This library's documented choice (neither binary is available to pin
 * against; libstfinv works in the frequency domain): the time-domain equivalent, a finite-lag Wiener filter with a water
 * level.  The library delivers the two device-side pieces; the Toeplitz solve in between is host code in float64
 * (misfit.solve_matching_filter).
 * Traces are [nt][nshot][nrec], time slowest.  lag_before >= 0 acausal and lag_after >= 0 causal lags,
 * nlag = lag_before + lag_after + 1 <= MIFWI_STF_MAX_LAGS; a filter is [nshot][nlag], index i holds lag k = i - lag_before.
 * Lags may exceed nt: a term whose time index falls outside [0, nt) is absent, never wrapped.
 *   mifwi_stf_correlate    per shot, in double (a product of two floats is exact there), x = pred, d = obs:
 *       auto_out[s][j]  = sum_r w^2 sum_t x[t] x[t+j],   j = 0 .. nlag-1
 *       cross_out[s][i] = sum_r w^2 sum_t d[t] x[t-k],   k = i - lag_before
 *     trace_w device [nshot][nrec] or NULL (= 1): weights >= 0 that multiply the traces, so the sums carry w^2; a trace with
 *     w == 0 is not read (it may hold NaN or Inf and changes no bit).  auto_out, cross_out device [nshot][nlag] double.
 *     No atomics: time ascending inside a receiver's sum, the receivers of a 64-wide tile in index order, the tiles in index
 *     order; a workgroup never mixes shots, so two identical calls give identical bits and a shot computed alone gives
 *     the bits it has in the whole call.  work: mifwi_stf_correlate_work_elems(...) floats, 8-byte aligned.
 *   mifwi_trace_convolve   y[t,s,r] = sum_i filt[s][i] x[t-k, s, r]   (transpose != 0: sum_i filt[s][i] x[t+k, s, r], its
 *     exact transpose), t in [0, nt); filt device [nshot][nlag] float; float accumulation with one fma per lag in ascending
 *     i, so |y - exact| <= (nlag + 1) 2^-24 sum_i |filt_i| |x_{t-k}|.  y == x is NOT allowed (every output reads nlag rows).
 * MIFWI_EINVAL: a null required argument, nt, nshot or nrec < 1, a negative lag, nlag > MIFWI_STF_MAX_LAGS, work not 8-byte
 * aligned, y == x, nt or nrec beyond 2^31 - 1, more than 65535 shots or 65535 * 64 receivers per shot (launch-grid axes).
 * ==================================================================================== */
enum { MIFWI_STF_MAX_LAGS = 1024 };

int64_t mifwi_stf_correlate_work_elems(int64_t nt, int64_t nshot, int64_t nrec, int32_t lag_before, int32_t lag_after);
int mifwi_stf_correlate(int device, const float *pred, const float *obs, const float *trace_w /* NULL or [nshot][nrec] */,
                        int64_t nt, int64_t nshot, int64_t nrec, int32_t lag_before, int32_t lag_after,
                        double *auto_out /* [nshot][nlag] */, double *cross_out /* [nshot][nlag] */, float *work, void *stream);
int mifwi_trace_convolve(int device, const float *x, float *y, const float *filt /* device, [nshot][nlag] */,
                         int64_t nt, int64_t nshot, int64_t nrec, int32_t lag_before, int32_t lag_after,
                         int32_t transpose, void *stream);

/* ======================================================================================
 * ENVELOPE MISFIT: the Hilbert transform along time, the envelope residual and its exact adjoint source (DENISE's lnorm = 6)
 *
 * The envelope objective of Chi, Dong and Liu (2014), used for the first low-frequency stages because it does not cycle-skip
 * where the sample-by-sample objectives do.  This library's documented choice (DENISE's binary is not available to pin against):
 * H on R^nt: with N the smallest power of two >= nt, zero-pad the trace to N, take the DFT, multiply bin k by -i for
 * 0 < k < N/2, by +i for N/2 < k < N and by 0 for k = 0 and k = N/2, take the inverse DFT (with its 1/N) and keep the real part
 * of the first nt samples: scipy.signal.hilbert(x, N=N, axis=0).imag[:nt]; H = 0 for N <= 2.  The multiplier is antisymmetric,
 * so H^T = -H exactly, and the transposed call returns the negated bits.
 *     E(x) = sqrt(x^2 + H(x)^2 + eps^2)            eps >= 0, one absolute scalar per call
 *     s = pred, o = obs, h = H s, r = E(s) - E(o):   loss = 1/2 sum r^2;   adj_out = dloss/ds = r s / E(s) - H(r h / E(s))
 * A term whose divisor E(s) is zero (possible with eps == 0 only) contributes 0.  |s| / E <= 1 and |h| / E <= 1: the adjoint
 * source is bounded by 2 |r| even where the envelope is small.
 * Traces are [nt][ntrace], time slowest; nt <= MIFWI_ENVELOPE_MAX_NT (a padded trace and its transform live in one workgroup's
 * LDS: an N/2-point complex FFT of the trace's even and odd samples, float arithmetic, twiddle factors rounded once from
 * double; envelope, residual and loss terms in double).  A trace is transformed on its own: an all-zero trace gives exact zeros.
 *   mifwi_trace_hilbert    y = H x (transpose != 0: y = H^T x = -H x); y == x allowed
 *   mifwi_misfit_envelope  one launch for both transforms, envelope, residual and the second Hilbert transform; pred, obs,
 *     adj_out (NULL = loss only, the same bits), loss_out as for mifwi_misfit.  No atomics: every trace's loss partial goes to
 *     work and a second kernel adds them in index order, so two identical calls give the same bits.
 *     work: mifwi_misfit_envelope_work_elems(nt, ntrace) floats, 8-byte aligned.
 * MIFWI_EINVAL: a null required argument, nt < 1, ntrace < 1, nt > MIFWI_ENVELOPE_MAX_NT (longer records are not supported),
 * ntrace > 2^31 - 1, eps negative, NaN or infinite, work not 8-byte aligned.
 * ==================================================================================== */
enum { MIFWI_ENVELOPE_MAX_NT = 8192 };

int mifwi_trace_hilbert(int device, const float *x, float *y, int64_t nt, int64_t ntrace, int32_t transpose, void *stream);
int64_t mifwi_misfit_envelope_work_elems(int64_t nt, int64_t ntrace);
int mifwi_misfit_envelope(int device, const float *pred, const float *obs, int64_t nt, int64_t ntrace, double eps,
                          float *loss_out, float *adj_out /* NULL: loss only, same bits */, float *work, void *stream);

/* ======================================================================================
 * TRANSPORT MISFIT: the quadratic Wasserstein distance between normalised traces along time and its exact adjoint source
 *
 * The optimal-transport objective of Engquist and Froese (2014) and Yang et al. (2018), trace by trace: it compares where the
 * energy of a trace sits in time and keeps growing with a time shift where the sample-by-sample objectives and, further out, the
 * envelope stop.  This library's documented choice; time is counted in samples; b > 0 is one absolute scalar per call.
 * With s = pred, o = obs of one trace, k = 0 .. nt - 1:
 *     u_k = softplus(b s_k) = max(z, 0) + log1p(exp(-|z|)), z = b s_k           v_k likewise from o_k
 *     p = u / U, U = sum u      q = v / V, V = sum v      P_k = sum_{j <= k} p_j      Q_k = sum_{j <= k} q_j      (Q_{-1} = 0)
 *     Pm_k = P_k - p_k / 2      tau_k = k + 1/2
 *     j(k) = the first j with Q_j >= Pm_k (clamped to nt - 1)
 *     T_k  = j + (Pm_k - Q_{j-1}) / q_j              the inverse of the piecewise-linear distribution function of q at Pm_k
 *     W = sum_k p_k (tau_k - T_k)^2                  loss = 1/2 sum over traces of W
 *     a_k = 2 p_k (T_k - tau_k) / q_{j(k)}           g_m = (tau_m - T_m)^2 + a_m / 2 + sum_{k > m} a_k
 *     adj_out_m = dloss/ds_m = 1/2 (g_m - sum_k g_k p_k) / U * b * sigmoid(b s_m)
 * A term whose divisor q_j is zero (softplus underflowed) contributes 0; a trace with U == 0 or V == 0 contributes 0 and gets a
 * zero adjoint source.  pred with the bits of obs gives loss == 0 and adj_out == 0 exactly (T_k - tau_k is evaluated as
 * (j - k) + (Pm_k - Qm_j) / q_j, Qm_j = Q_j - q_j / 2).
 * Traces are [nt][ntrace], time slowest; nt <= MIFWI_TRANSPORT_MAX_NT (Q and q of a trace live in one workgroup's LDS).  Softplus,
 * sums, distribution functions, T, the suffix sums and the loss are double.
 *   mifwi_misfit_transport  one launch, one workgroup per trace; pred, obs, adj_out (NULL = loss only, the same bits), loss_out
 *     as for mifwi_misfit.  No atomics: every trace's W goes to work and a second kernel adds them in index order, so two
 *     identical calls give the same bits.  work: mifwi_misfit_transport_work_elems(nt, ntrace) floats, 8-byte aligned.
 * MIFWI_EINVAL, before any device work: a null required argument, nt < 1, ntrace < 1, nt > MIFWI_TRANSPORT_MAX_NT (longer
 * records are not supported), ntrace > 2^31 - 1, b <= 0, NaN or infinite, work not 8-byte aligned.
 * ==================================================================================== */
enum { MIFWI_TRANSPORT_MAX_NT = 8192 };

int64_t mifwi_misfit_transport_work_elems(int64_t nt, int64_t ntrace);
int mifwi_misfit_transport(int device, const float *pred, const float *obs, int64_t nt, int64_t ntrace, double b,
                           float *loss_out, float *adj_out /* NULL: loss only, same bits */, float *work, void *stream);

/* ======================================================================================
 * GRADIENT CONDITIONING on the device (what sits between d.get_fwi_gradients(...) and fake_Vp.backward(grad))
 *
 * Replaces the numpy / scipy post-processing of the model gradients in the elastic prop() methods:
 *   models/networks.py:7808-7862, 9884-9919  flipud, zero rows 0:25, scale by max(model)/max(gradient), rho x 0.1
 *   models/networks.py:10522-10540           flipud, scipy.ndimage.gaussian_filter(sigma=3), zero rows 0:5, same scaling
 *   models/networks.py:7731, 9832-9833       SWS_TAPER_GRAD_HOR / EXP_TAPER_GRAD_HOR (a weight per depth row)
 * grad, out [nplane][nz][nx] device (nplane <= 4, out != grad); models NULL or [nplane][nz][nx] device;
 * row_weight NULL or [nz] device (indexed by the row of `grad` as stored);  flip: output row j reads stored row
 * nz-1-j;  sigma: 0 = no smoothing, else scipy's Gaussian (radius int(4 sigma + 0.5) <= 32, 'reflect' boundary);
 * mute_rows: output rows [0, mute_rows) are zeroed after the smoothing;  factors NULL or HOST array [nplane].
 *   out_k = factor_k * (models ? max(models_k) / max(t_k) : 1) * t_k,   t_k = mute(smooth(w * flip(grad_k)))
 * work: mifwi_gradient_condition_work_elems(nplane) floats.
 * ==================================================================================== */
int64_t mifwi_gradient_condition_work_elems(int32_t nplane);
int mifwi_gradient_condition(int device, const float *grad, const float *models, float *out, int32_t nplane,
                             int32_t nz, int32_t nx, const float *row_weight, float sigma, int32_t flip,
                             int32_t mute_rows, const float *factors, float *work, void *stream);

/* Pseudo-Hessian preconditioning (DENISE EPRECOND = 1 with the water level EPSILON_WE; see the pseudo-Hessian block above):
 *   out_k = grad_k / (hess_k / max(hess_k) + eps_k)      per plane; a plane whose maximum is not positive is copied.
 * grad, hess, out [nplane][n] device (nplane 1..4; out may alias grad); eps HOST array [nplane], every entry > 0
 * (else MIFWI_EINVAL); work: mifwi_gradient_precondition_work_elems(nplane) floats. */
int64_t mifwi_gradient_precondition_work_elems(int32_t nplane);
int mifwi_gradient_precondition(int device, const float *grad, const float *hess, float *out, int32_t nplane,
                                int64_t n, const float *eps /* host [nplane], > 0 */, float *work, void *stream);

/* ======================================================================================
 * MATERIAL PARAMETERISATION of the elastic kernels and its chain rule
 *
 * (Vp, Vs, rho) -> mat[5][nz][nx] = lambda dt/h, (lambda + 2 mu) dt/h, mu_xz dt/h (harmonic mean of the four mu
 * around the sxz node, 0 in water), dt/(h rho_x), dt/(h rho_z) (arithmetic means at the vx / vz nodes), edge values
 * replicated; free_surface: row 0 in the effective form of the stress-imaging condition.  What DENISE does inside
 * set_model before a forward run and undoes when get_fwi_gradients returns Vp / Vs / rho gradients
 * (models/networks.py:7698-7712, 7802-7806, 9790-9800); physicsbasedfwi2_amd/elastic.py:staggered_materials is the
 * definition (same operations and roundings).  All arrays device, [nz][nx] row-major, no padding.
 * mifwi_elastic_materials_vjp: grad_out [5][nz][nx] -> grad_vp, grad_vs, grad_rho (gather, bitwise repeatable).
 * ==================================================================================== */
int mifwi_elastic_materials(int device, const float *vp, const float *vs, const float *rho, float *mat, int32_t nz,
                            int32_t nx, float dt_over_h, int32_t free_surface, void *stream);
int mifwi_elastic_materials_vjp(int device, const float *vp, const float *vs, const float *rho, const float *grad_out,
                                float *grad_vp, float *grad_vs, float *grad_rho, int32_t nz, int32_t nx,
                                float dt_over_h, int32_t free_surface, void *stream);

/* DENISE's INVMAT1 (models/networks.py:11025 sets 2): the parameter set the gradients of `d.grad` / get_fwi_gradients
 * refer to.  Input: the gradients with respect to (Vp, Vs, rho) - what mifwi_elastic_materials_vjp returns - and the
 * model; output: the gradients with respect to
 *   MIFWI_PARAM_VELOCITY  (1)  Vp, Vs, rho                   (copy)
 *   MIFWI_PARAM_IMPEDANCE (2)  Zp = rho Vp, Zs = rho Vs, rho:  g_Zp = g_vp / rho,  g_Zs = g_vs / rho,
 *                              g_rho' = g_rho - (Vp g_vp + Vs g_vs) / rho
 *   MIFWI_PARAM_LAME      (3)  lambda, mu, rho:               g_lambda = g_vp / (2 rho Vp),
 *                              g_mu = g_vp / (rho Vp) + g_vs / (2 rho Vs)   (second term 0 where Vs = 0: a fluid has no mu to move),
 *                              g_rho' = g_rho - (Vp g_vp + Vs g_vs) / (2 rho)
 * i.e. the exact chain rule of the change of variables, cell by cell (a 3 x 3 Jacobian).  out_* may alias the inputs.
 * A term whose divisor is zero contributes 0, so every output is finite:
 *   IMPEDANCE, rho = 0:           g_Zp = g_Zs = 0, g_rho' = g_rho
 *   LAME, rho = 0 or Vp = 0:      g_lambda = 0 and no g_vp term in g_mu
 *   LAME, rho = 0 or Vs = 0:      no g_vs term in g_mu;   rho = 0: g_rho' = g_rho
 * n = number of cells; all arrays device. */
#define MIFWI_PARAM_VELOCITY 1
#define MIFWI_PARAM_IMPEDANCE 2
#define MIFWI_PARAM_LAME 3
int mifwi_elastic_gradient_parametrization(int device, int32_t parametrization, const float *vp, const float *vs,
                                           const float *rho, const float *grad_vp, const float *grad_vs,
                                           const float *grad_rho, float *out_a, float *out_b, float *out_rho,
                                           int64_t n, void *stream);

/* The pseudo-Hessian planes of one parameter set (MIFWI_PARAM_*) from the moments of mifwi_elastic_snapshot_moments:
 * H_p of the formulas in the pseudo-Hessian block above, cell by cell, in the order of
 * mifwi_elastic_gradient_parametrization (h_a, h_b: Vp, Vs / Zp, Zs / lambda, mu).  vp, vs, rho, h_* [nz][nx] device,
 * no padding; moments [6][nz][gp].  Every output is finite and >= 0. */
int mifwi_elastic_pseudo_hessian(int device, int32_t parametrization, const float *vp, const float *vs,
                                 const float *rho, const float *moments, int32_t nz, int32_t nx, int32_t gp,
                                 float dt_over_h, float *h_a, float *h_b, float *h_rho, void *stream);

/* The pseudo-Hessian planes of the fluid propagator's parameter sets from the moments of mifwi_fluid_snapshot_moments
 * [3][nz][gp]: mifwi_elastic_pseudo_hessian with Vs = 0, so that a preconditioned update does not depend on which kernels
 * ran.  There L_p = M_p = K_p and the fluid's S0 is the elastic S0 + S1, so the stress terms collapse:
 *   H_p = fmaf(2 K_p^2, M0, b_p^2 (M1 + M2)), clamped at 0       (2: the two identical stress equations the fluid merges)
 *   VELOCITY   Vp: K_p = 2 rho Vp s, b_p = 0      rho: K_p = Vp^2 s,  b_p = -s / rho^2
 *   IMPEDANCE  Zp: K_p = 2 Vp s,     b_p = 0      rho: K_p = -Vp^2 s, b_p = -s / rho^2
 *   LAME       K:  K_p = s,          b_p = 0      rho: K_p = 0,       b_p = -s / rho^2
 * with s = dt/h; a term whose divisor is zero contributes 0; the same collocated approximation.  vp, rho, h_a (Vp / Zp / K),
 * h_rho [nz][nx] device, no padding.  Every output is finite and >= 0. */
int mifwi_fluid_pseudo_hessian(int device, int32_t parametrization, const float *vp, const float *rho,
                               const float *moments, int32_t nz, int32_t nx, int32_t gp, float dt_over_h, float *h_a,
                               float *h_rho, void *stream);

/* vp [nz][nx] (m/s) -> r [nz + 2 pad][nx + 2 pad] = (vp dt/h)^2 with the model edge-replicated into the absorbing
 * layer: the coefficient of the scalar scheme as the deepwave-shaped call protocol needs it per call
 * (deepwave.scalar.Propagator({'vp': model}, dx), models/networks.py:5408-5411, 5449), and its chain rule
 * (grad_r [nz + 2 pad][nx + 2 pad] -> grad_vp [nz][nx]; the layer's cells folded into the edge cells in a fixed order). */
int mifwi_acoustic_coefficients(int device, const float *vp, float *r, int32_t nz, int32_t nx, int32_t pad,
                                float dt_over_h, void *stream);
int mifwi_acoustic_coefficients_vjp(int device, const float *vp, const float *grad_r, float *grad_vp, int32_t nz,
                                    int32_t nx, int32_t pad, float dt_over_h, void *stream);

/* ======================================================================================
 * Diagonal PSEUDO-HESSIAN of the acoustic gradient (the scalar counterpart of the elastic block above)
 *
 * Serves the deepwave-shaped protocol (models/networks.py:5408-5491 and its prop() variants) and the square-slowness
 * protocol of seisgan/fwi (layers.py:158-197), whose raw gradients are dominated by the cells around the sources.
 *
 * The plane G^n a forward step saves for the adjoint is the virtual source of the coefficient r (mifwi_acoustic_born
 * injects G^n dr), so
 *   MOMENT  M [n0][gp] = sum over the plan's shots and the selected steps of (G^n)^2
 * is the pseudo-Hessian with respect to r: one more read of the snapshot buffer, no extra propagation.
 * steps n in [n_begin, n_end) with n % stride == 0 (absolute n: a range may be cut anywhere), each weighted by stride;
 * step n at snap + (n - snap_first) * nshot * n0 * gp as mifwi_acoustic_forward of the same plan wrote it (both kernel
 * families, sponge and C-PML plans); MIFWI_ZERO_STATE: overwrite, else add.  Columns >= n1 are written as 0 whatever
 * the snapshot pad holds.  work: mifwi_acoustic_snapshot_moments_work_elems(plan) floats (partial planes of the step
 * range, added in a fixed order: no atomics, two identical calls give the same bits).  MIFWI_EINVAL: a null pointer,
 * stride < 1, an empty or reversed range or one outside [0, nt), snap_first > n_begin, a pointer that is not 16-byte
 * aligned.  (G^{nt-1} never reaches a recorded sample: a gradient's own Hessian takes [0, nt - 1).)
 * ==================================================================================== */
int64_t mifwi_acoustic_snapshot_moments_work_elems(const mifwi_acoustic_plan *plan);
int mifwi_acoustic_snapshot_moments(mifwi_acoustic_plan *plan, const float *snap, int32_t snap_first,
                                    int32_t n_begin, int32_t n_end, int32_t stride, float *moments,
                                    float *work, int32_t flags, void *stream);

/* The pseudo-Hessian plane of a model parameter from that moment:
 *   MIFWI_AC_PARAM_VELOCITY  (1)  the deepwave protocol: model = vp [nz][nx], moments [nz + 2 pad][gp], scale = dt/h,
 *                                 r = (edge-replicated vp * scale)^2 as mifwi_acoustic_coefficients forms it;
 *                                 hess[i][j] = (2 vp scale^2)^2 * sum of M over the padded cells that replicate (i, j)
 *                                 (the fold of mifwi_acoustic_coefficients_vjp; exact when J^T J is diagonal)
 *   MIFWI_AC_PARAM_SLOWNESS2 (2)  the seisgan protocol: model = m = 1/vp^2 [nz][nx] on the padded grid itself, every
 *                                 cell its own variable (pad must be 0), r = scale^2 / m with scale = s/h;
 *                                 hess = (r / m)^2 * M
 * hess [nz][nx] device, no padding.  Every output is finite and >= 0; a cell with vp = 0 or m <= 0 gives 0. */
#define MIFWI_AC_PARAM_VELOCITY 1
#define MIFWI_AC_PARAM_SLOWNESS2 2
int mifwi_acoustic_pseudo_hessian(int device, int32_t parametrization, const float *model, const float *moments,
                                  int32_t nz, int32_t nx, int32_t pad, int32_t gp, float scale, float *hess,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIFWI_H */
