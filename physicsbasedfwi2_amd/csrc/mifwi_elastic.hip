// 2-D P-SV elastic velocity-stress propagator for gfx950 (MI355X): forward, snapshot save and
// the exact discrete adjoint with material-gradient accumulation.  Memory-bound staggered-grid
// stencil (4th order space, leapfrog time, C-PML memory variables); MFMA unused.
//
// Replaces (reference tree): the DENISE-Black-Edition runs behind pyapi_denise's
// `d.forward(...)` / `d.grad(...)` as called at models/networks.py:7787, 9853-9877 (mpirun of 30
// MPI ranks + files on disk in the reference).
//
// Forward: two launches per time step (V: velocities from stresses, S: stresses from the new
// velocities).  A thread owns 4 consecutive cells (16-B lane accesses) and marches RZ rows with
// the z windows in registers; x neighbours come from 8-B halo loads that hit the lines the
// neighbouring lanes fetch.  C-PML memory variables live in compact strips (group-aligned in x,
// row-aligned in z) so that interior tiles never touch them.  Source injection (LDS image of
// the tile, only where the shot's bounding box intersects it) and receiver sampling (extra
// workgroups) ride in the S launch.
// Born (mifwi_elastic_born): the same two launches on the perturbed state; instead of writing the step's five snapshot
// planes they read the background run's and add dmat times them (SAVE = kBorn), the JVP partner of the adjoint's gradients.
// Adjoint: two launches per step (S^T then V^T).  The transposed C-PML acts on the
// material-scaled adjoint fields BEFORE the spatial derivative, so each workgroup first
// evaluates those four per-cell quantities on its tile + 2-cell halo into LDS, then applies the
// stencils from LDS.  All five material-gradient accumulators are updated in the S^T launch and
// stay in registers across the shots of a group (one read-modify-write per group, not per shot).
// Tiles are taken in an XCD-contiguous order (xcd_tile) so that neighbouring tiles share an L2, and the
// drivers sweep the time range a few shots at a time when all shots together would not stay inside the
// 256 MiB Infinity Cache (plan->pass_shots / pass_groups).  Grids whose shot fits the LDS of a few CUs run
// the whole time loop in one launch instead (mifwi_elastic_cluster.h); point forces (source_type 1 / 2) and
// the opt-in fused V+S launch (el_step_fused) live on the per-step path only.
// VTI (mifwi_vti_*): the same scheme with c11, c13, c33, c44 for lambda + 2 mu, lambda, mu - one more material plane (M_C33), a
// compile-time variant of el_step_s, el_adj_s / stage_E and finalize_groups on the per-step path; with c33 == c11 the same bits.
// Viscoelastic (mifwi_visco_*): one relaxation mechanism - three memory variables behind the five fields of a shot, three more
// material planes; a compile-time VISCO variant of el_step_s, el_adj_s / stage_E, el_adj_v (which advances the adjoint memory
// variables) and finalize_groups on the per-step path; with the three planes zero the same bits.
// TTI (mifwi_tti_*): the VTI stiffnesses rotated by a tilt field - two more planes (c15, c35) that couple the normal stresses to
// the shear strain through four-point averages; the stress half step and its transpose are two launches each, kernels of
// their own in mifwi_tti.h (tti_strain + tti_stress, tti_adj_e + tti_adj_s) around the V launches of every medium.
// What this scheme shares with the fluid one below the cell arithmetic (stencil and C-PML primitives, strip and tile
// helpers, build_tile_taps / sample_force / finalize_groups, the plan's grid geometry) is in mifwi_stagger.h.
// Arithmetic = the explicit fmaf chain of oracle/elastic.c (build with -ffp-contract=off).
#include "mifwi_cluster_host.h"
#include "mifwi_stagger.h"

#include <cmath>
#include <cstdlib>

namespace {

#ifndef MIFWI_EL_MINWAVES
#define MIFWI_EL_MINWAVES 1
#endif
enum { F_VX = 0, F_VZ = 1, F_SXX = 2, F_SZZ = 3, F_SXZ = 4 };
enum { M_L = 0, M_M = 1, M_MU = 2, M_BX = 3, M_BZ = 4 };
// VTI variant (mifwi_vti_*): the same planes with c13 at M_L, c11 at M_M, c44_xz at M_MU, and c33 appended as a sixth plane
enum { M_C33 = 5 };
// viscoelastic variant (mifwi_visco_*, one relaxation mechanism): three memory variables behind the five fields, and three planes
// behind the five unrelaxed ones: R2 = pi_r tau_p - 2 mu_r tau_s, R1 = pi_r tau_p, mu_r tau_s at the sxz node (all times dt/h)
enum { F_RXX = 5, F_RZZ = 6, F_RXZ = 7 };
enum { M_RL = 5, M_RM = 6, M_RMU = 7 };
// psi index: x strips hold (0: d1 sxx_x @half, 1: d3 sxz_x @int, 2: e1 vx_x @int, 3: e4 vz_x @half)
//            z strips hold (0: d2 sxz_z @int, 1: d4 szz_z @half, 2: e2 vz_z @int, 3: e3 vx_z @half)

struct ElParams {
    int nz, nx, ng, gp, pitch;
    unsigned field_stride;       // (nz+4)*pitch
    long long shot_stride;       // 5*field_stride; 8*field_stride on a viscoelastic plan (F_RXX..F_RXZ)
    int nshot, gs;
    int s0;                      // first shot of this pass over the time range (blockIdx.z counts from it)
    int W, wl, xr0, wx;          // C-PML strip geometry; W = 0 disables the layer
    int fsurf;                   // 1: stress-imaging free surface on row 0
    long long psix_shot, psiz_shot;   // floats per shot: 4*nz*wx, 4*2W*gp
    const float *mat, *pz, *px;
    float *fields;
    float *fields_out;           // fused forward step: the copy of the state this launch writes
    float *psix, *psiz;          // forward: updated in place; adjoint: read side
    float *psix_out, *psiz_out;  // adjoint: write side (ping-pong)
    float *S;                    // snapshot slice of this step: f32 [nshot][5][nz][gp]; bf16: snap_shot floats per shot
    long long snap_shot;         // floats per shot of one snapshot step (5 * splane for f32)
    unsigned splane;             // floats per snapshot plane: nz*gp, or nz * 64 * ceil(ng / 16) in the column-blocked layout
    int sblk;                    // 1: snapshot planes stored as [column block of 16 groups][row][64 floats] (snap_cell)
    float *acc;                  // [ngroups][5][nz][gp] (6 planes per group on a VTI plan, 8 on a viscoelastic one)
    // injection (S launch: sxx,szz += a ; S^T launch: vx += ax, vz += az)
    int ninj, ntap_inj;
    const int *inj_cell;
    const float *inj_w;
    const float *inj_amp0, *inj_amp1;     // [nshot][ninj] of this step (amp1 only in S^T)
    const int *inj_bbox;
    const int *tile_start, *tile_list;   // el_adj_s: receiver taps of each (shot, tile): [nshot][ntiles + 1], [nshot][ninj * ntap_inj]
    // sampling (S launch: vx, vz ; S^T launch: sxx+szz)
    int nsmp, ntap_smp;
    const int *smp_cell;
    const float *smp_w;
    float *smp_out0, *smp_out1;
    int tiles_z;
    int xcd;                     // XCD-aware tile order (xcd_tile): 1 contiguous runs per shot, 2 whole shots, 3 tile-major over the shots
    FdK K;                       // stencil weights
    const float *dmat;           // Born step (SAVE 3): perturbation of the five material planes, [5][nz][gp] like mat
    float rel_a, rel_b;          // viscoelastic plans: r <- a r - b q per step, a = (2 - eta) / (2 + eta), b = 2 eta / (2 + eta)
};

// uniform base + 32-bit lane offset (in floats): selects the `global_* v_off, s[base]` addressing form - no 64-bit
// vector address per plane and lane
__device__ __forceinline__ const float *el_at(const float *base, unsigned off)
{
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + 4u * off);
}
__device__ __forceinline__ float *el_at(float *base, unsigned off)
{
    return reinterpret_cast<float *>(reinterpret_cast<char *>(base) + 4u * off);
}
// a per-lane value the compiler must treat as unknown here: what is derived from it is recomputed at the use instead of
// being hoisted out of a loop and kept (or spilled) across it
__device__ __forceinline__ int f_opaque(int x)
{
    asm volatile("" : "+v"(x));
    return x;
}
// ---- bf16 snapshot planes (plan snapshot_format = 1): the five per-step planes the material gradient needs are
// rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32) on their way to memory and widened again by the
// adjoint: 10 instead of 20 B per cell-step each way.  Arithmetic stays f32.  Layout of one shot-step, in
// 4-cell groups g = (j*gp + 4*i)/4:  [g][S1 x4, S2 x4] 16 B | [g][S4 x4, S5 x4] 16 B | [g][S3 x4] 8 B.
typedef __bf16 mifwi_bf2 __attribute__((ext_vector_type(2)));
typedef float mifwi_f2 __attribute__((ext_vector_type(2)));
typedef unsigned mifwi_u4 __attribute__((ext_vector_type(4)));
typedef unsigned mifwi_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf_pack(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(mifwi_f2{a, b}, mifwi_bf2));
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ void bf_store2(float *base, unsigned grp, const float *a, const float *b)
{
    const mifwi_u4 v{bf_pack(a[0], a[1]), bf_pack(a[2], a[3]), bf_pack(b[0], b[1]), bf_pack(b[2], b[3])};
    __builtin_nontemporal_store(v, reinterpret_cast<mifwi_u4 *>(base) + grp);
}
__device__ __forceinline__ void bf_store1(float *base, unsigned grp, const float *a)
{
    const mifwi_u2 v{bf_pack(a[0], a[1]), bf_pack(a[2], a[3])};
    __builtin_nontemporal_store(v, reinterpret_cast<mifwi_u2 *>(base) + grp);
}
// offsets (in floats) of the three regions of a bf16 shot-step
__device__ __forceinline__ long long bf_reg_de(unsigned ncell) { return (long long)ncell; }
__device__ __forceinline__ long long bf_reg_c(unsigned ncell) { return 2LL * ncell; }
// The packed planes of one group.  Loading and widening are two steps: the loads are requested before a barrier
// and consumed after it, and the widening must stay behind the barrier too (`bf_pin`) - scheduled in front of it,
// the wave would sit out the latency of the snapshot stream, the one stream that always comes from HBM, before
// every barrier (measured: el_adj_s 80 instead of 72 us per launch on 350x1700 although it reads 10 B less).
struct BfPlanes { mifwi_u4 ab, de; mifwi_u2 c; };
__device__ __forceinline__ void bf_request(const float *shot_base, unsigned ncell, unsigned grp, BfPlanes &q)
{
    q.ab = __builtin_nontemporal_load(reinterpret_cast<const mifwi_u4 *>(shot_base) + grp);
    q.de = __builtin_nontemporal_load(reinterpret_cast<const mifwi_u4 *>(shot_base + bf_reg_de(ncell)) + grp);
    q.c = __builtin_nontemporal_load(reinterpret_cast<const mifwi_u2 *>(shot_base + bf_reg_c(ncell)) + grp);
}
__device__ __forceinline__ void bf_pin(BfPlanes &q)
{
    asm volatile("" : "+v"(q.ab), "+v"(q.de), "+v"(q.c));
}
__device__ __forceinline__ void bf_widen(const BfPlanes &q, float4 &S1, float4 &S2, float4 &S3, float4 &S4, float4 &S5)
{
    S1 = make_float4(bf_lo(q.ab.x), bf_hi(q.ab.x), bf_lo(q.ab.y), bf_hi(q.ab.y));
    S2 = make_float4(bf_lo(q.ab.z), bf_hi(q.ab.z), bf_lo(q.ab.w), bf_hi(q.ab.w));
    S4 = make_float4(bf_lo(q.de.x), bf_hi(q.de.x), bf_lo(q.de.y), bf_hi(q.de.y));
    S5 = make_float4(bf_lo(q.de.z), bf_hi(q.de.z), bf_lo(q.de.w), bf_hi(q.de.w));
    S3 = make_float4(bf_lo(q.c.x), bf_hi(q.c.x), bf_lo(q.c.y), bf_hi(q.c.y));
}

// Offset (floats) of group g of row j inside a snapshot plane.  Row-major [nz][gp] (the layout the single-launch
// kernels share), or - per-step family, plans without a single-launch kernel - blocked by columns of 16 groups
// (snap_cell_blocked).
__device__ __forceinline__ unsigned snap_cell(const ElParams &p, int j, int g)
{
    return p.sblk ? snap_cell_blocked(p.nz, j, g) : (unsigned)j * p.gp + 4u * (unsigned)g;
}

// XCD-aware tile order (p.xcd; a bijection on the launch grid in every mode).  3: tile-major over the shots of the launch
// (xcd_tile_major_index).  Otherwise:
//  * 2, z slices (shots / shot groups) in full sets of eight: XCD c takes the slices c, c+8, ... WHOLE, walking
//    each in row-major tile order - every halo a tile reads was fetched by the same L2 one tile row earlier
//    (measured on 350x1700, 8 shots per launch: the halo rows of a 2.7-tile-row run per XCD came from the
//    other XCDs' runs, i.e. from beyond L2);
//  * 1 and the remaining slices of 2: each XCD walks one contiguous, row-major run of the (x, y) tiles of the slice.
__device__ __forceinline__ void xcd_tile(const ElParams &p, int &bx, int &by, int &bz)
{
    bx = (int)blockIdx.x; by = (int)blockIdx.y; bz = (int)blockIdx.z;
    if (!p.xcd) return;
    const unsigned gx = gridDim.x, n2 = gx * gridDim.y;
    const unsigned z8 = gridDim.z & ~7u;          // p.xcd == 2: whole slices per XCD
    unsigned T;
    if (p.xcd == 3) {
        T = xcd_tile_major_index(bz);
    } else if (p.xcd == 2 && blockIdx.z < z8) {
        const unsigned L = blockIdx.x + gx * blockIdx.y + n2 * blockIdx.z;
        const unsigned c = L & 7u, idx = L >> 3, zl = idx / n2;
        T = idx - zl * n2;
        bz = (int)(c + 8u * zl);
    } else {
        const unsigned L = blockIdx.x + gx * blockIdx.y;
        const unsigned c = L & 7u, idx = L >> 3, q = n2 >> 3, r = n2 & 7u;
        T = c * q + (c < r ? c : r) + idx;
    }
    by = (int)(T / gx); bx = (int)(T - (unsigned)by * gx);
}

// ------------------------------------------------------------------------------------------------
// sampling workgroups.  mode 0: out0 = sum w vx, out1 = sum w vz ; mode 1: out0 = sum w (sxx+szz)
template <int MODE>
__device__ void sample_points(const ElParams &p, int bx, int by, int bz)
{
    if (p.smp_out0 == nullptr) return;
    const int nrb = (int)(gridDim.y - p.tiles_z) * (int)gridDim.x;
    const int rb = (by - p.tiles_z) * (int)gridDim.x + bx;
    const int total = p.gs * p.nsmp;
    for (int e = rb * (int)blockDim.x + (int)threadIdx.x; e < total; e += nrb * (int)blockDim.x) {
        const int si = e / p.nsmp, ip = e - si * p.nsmp;
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) continue;
        const float *fl = p.fields + (long long)s * p.shot_stride;
        float a0 = 0.f, a1 = 0.f;
        for (int t = 0; t < p.ntap_smp; ++t) {
            const long long ee = ((long long)s * p.nsmp + ip) * p.ntap_smp + t;
            const int cell = p.smp_cell[ee];
            if (cell < 0) continue;
            const int j = cell / p.nx, i = cell - j * p.nx;
            const unsigned off = (unsigned)(j + 2) * p.pitch + 4 + i;
            const float w = p.smp_w[ee];
            if (MODE == 0) {
                a0 = fmaf(w, fl[F_VX * p.field_stride + off], a0);
                a1 = fmaf(w, fl[F_VZ * p.field_stride + off], a1);
            } else {
                const float zz = (p.fsurf && j == 0) ? 0.f : fl[F_SZZ * p.field_stride + off];
                a0 = fmaf(w, fl[F_SXX * p.field_stride + off] + zz, a0);
            }
        }
        p.smp_out0[(long long)s * p.nsmp + ip] = a0;
        if (MODE == 0) p.smp_out1[(long long)s * p.nsmp + ip] = a1;
    }
}

// stage the shot's injection amplitudes that fall into this tile (block-uniform decision)
template <int TZ, int TX, int NCOMP>
__device__ bool stage_injection(const ElParams &p, int s, int tile_j, int tile_i, float *inj)
{
    if (p.ninj <= 0) return false;
    const int b0 = p.inj_bbox[4 * s + 0], b1 = p.inj_bbox[4 * s + 1];
    const int b2 = p.inj_bbox[4 * s + 2], b3 = p.inj_bbox[4 * s + 3];
    const bool has = (b0 < tile_j + TZ) && (b1 >= tile_j) && (b2 < tile_i + TX) && (b3 >= tile_i);
    if (!has) return false;
    for (int e = (int)threadIdx.x; e < NCOMP * TZ * TX; e += kThreads) inj[e] = 0.f;
    __syncthreads();
    const int total = p.ninj * p.ntap_inj;
    for (int e = (int)threadIdx.x; e < total; e += kThreads) {
        const long long ee = (long long)s * total + e;
        const int cell = p.inj_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        const int tj = j - tile_j, ti = i - tile_i;
        if (tj >= 0 && tj < TZ && ti >= 0 && ti < TX) {
            const long long ai = (long long)s * p.ninj + e / p.ntap_inj;
            const float w = p.inj_w[ee];
            atomicAdd(&inj[tj * TX + ti], w * p.inj_amp0[ai]);
            if (NCOMP == 2) atomicAdd(&inj[TZ * TX + tj * TX + ti], w * p.inj_amp1[ai]);
        }
    }
    __syncthreads();
    return true;
}

// ================================================================================================
// forward V launch:  vx += bxs (Dp_x sxx' + Dm_z sxz'),  vz += bzs (Dm_x sxz' + Dp_z szz')
// ================================================================================================
// SAVE 0: no snapshots, 1: write f32 planes, 2: write bf16 planes, 3 (kBorn): the Born step - the state is the perturbed
// field, and the f32 planes of the background run's step are READ: times dmat they are the step's virtual sources
constexpr int kBorn = 3;
template <int LX, int RZ, int SAVE>
__global__ __launch_bounds__(kThreads, MIFWI_EL_MINWAVES) void el_step_v(const ElParams p)
{
    const FdK K = p.K;
    constexpr int LZ = kThreads / LX;
    const int lx = (int)threadIdx.x % LX, lz = (int)threadIdx.x / LX;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    const int g = bx * LX + lx;
    const int j0 = (by * LZ + lz) * RZ;
    if (g >= p.ng || j0 >= p.nz) return;
    const int s = p.s0 + bz;
    const unsigned fs = p.field_stride;
    float *fl = p.fields + (long long)s * p.shot_stride;
    const float *sxx = fl + F_SXX * fs, *szz = fl + F_SZZ * fs, *sxz = fl + F_SXZ * fs;
    float *vx = fl + F_VX * fs, *vz = fl + F_VZ * fs;
    const unsigned col = 4 + 4 * g;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const int xs_off = xstrip(p, g);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pxa = zero4, pxb = zero4, pxk = zero4, pxah = zero4, pxbh = zero4, pxkh = zero4;
    if (xs_off >= 0) {
        pxa = ld4(p.px + PA * p.gp + 4 * g); pxb = ld4(p.px + PB * p.gp + 4 * g);
        pxk = ld4(p.px + PK * p.gp + 4 * g); pxah = ld4(p.px + PAH * p.gp + 4 * g);
        pxbh = ld4(p.px + PBH * p.gp + 4 * g); pxkh = ld4(p.px + PKH * p.gp + 4 * g);
    }
    // windows: sxz rows j-2..j+1 (a0..a3), szz rows j-1..j+2 (b0..b3)
    float4 a0, a1, a2, a3, b0, b1, b2, b3;
    {
        const unsigned o = (unsigned)(j0 + 2) * p.pitch + col;     // row j0
        a0 = ld4(sxz + o - 2 * p.pitch); a1 = ld4(sxz + o - p.pitch); a2 = ld4(sxz + o);
        b0 = ld4(szz + o - p.pitch); b1 = ld4(szz + o); b2 = ld4(szz + o + p.pitch);
    }
#pragma unroll
    for (int rz = 0; rz < RZ; ++rz) {
        const int j = j0 + rz;
        if (j < p.nz) {
            const unsigned o = (unsigned)(j + 2) * p.pitch + col;
            const unsigned cc = (unsigned)j * p.gp + 4 * g;
            // every global request of this row up front (one memory round trip per row): the
            // memory variables of the C-PML strips are fetched together with the fields
            const int zs = zstrip(p, j);
            float *q1 = nullptr, *q3 = nullptr, *q2 = nullptr, *q4 = nullptr;
            float4 s1 = zero4, s3 = zero4, s2 = zero4, s4 = zero4;
            float za = 0.f, zb = 0.f, zk = 1.f, zah = 0.f, zbh = 0.f, zkh = 1.f;
            if (xs_off >= 0) {
                q1 = p.psix + (long long)s * p.psix_shot + ((long long)0 * p.nz + j) * p.wx + xs_off;
                q3 = p.psix + (long long)s * p.psix_shot + ((long long)1 * p.nz + j) * p.wx + xs_off;
                s1 = ld4(q1); s3 = ld4(q3);
            }
            if (zs >= 0) {
                q2 = p.psiz + (long long)s * p.psiz_shot + ((long long)0 * 2 * p.W + zs) * p.gp + 4 * g;
                q4 = p.psiz + (long long)s * p.psiz_shot + ((long long)1 * 2 * p.W + zs) * p.gp + 4 * g;
                s2 = ld4(q2); s4 = ld4(q4);
                za = p.pz[PA * p.nz + j]; zb = p.pz[PB * p.nz + j]; zk = p.pz[PK * p.nz + j];
                zah = p.pz[PAH * p.nz + j]; zbh = p.pz[PBH * p.nz + j]; zkh = p.pz[PKH * p.nz + j];
            }
            a3 = ld4(sxz + o + p.pitch);
            b3 = ld4(szz + o + 2 * p.pitch);
            if (p.fsurf && j < 2) {
                // odd mirroring about row 0: sxz(-m) = -sxz(m-1), szz(-m) = -szz(m)
                if (j == 0) {
                    a1 = make_float4(-a2.x, -a2.y, -a2.z, -a2.w);
                    a0 = make_float4(-a3.x, -a3.y, -a3.z, -a3.w);
                    b0 = make_float4(-b2.x, -b2.y, -b2.z, -b2.w);
                } else {
                    a0 = make_float4(-a1.x, -a1.y, -a1.z, -a1.w);
                }
            }
            const float4 cxx = ld4(sxx + o);
            const float2 Lxx = ld2(sxx + o - 2), Rxx = ld2(sxx + o + 4);
            const float2 Lxz = ld2(sxz + o - 2), Rxz = ld2(sxz + o + 4);
            float4 vxv = ld4(vx + o), vzv = ld4(vz + o);
            const float4 bxs = ld4(p.mat + M_BX * ncell + cc), bzs = ld4(p.mat + M_BZ * ncell + cc);
            float4 B3 = zero4, B4 = zero4, dbx = zero4, dbz = zero4;
            if (SAVE == kBorn) {
                const float *Sp = p.S + (long long)s * p.snap_shot + snap_cell(p, j, g);
                B3 = mifwi::ldnt4(Sp + 3 * (long long)p.splane); B4 = mifwi::ldnt4(Sp + 4 * (long long)p.splane);
                dbx = ld4(p.dmat + M_BX * ncell + cc); dbz = ld4(p.dmat + M_BZ * ncell + cc);
            }
            const float xx[8] = {Lxx.x, Lxx.y, cxx.x, cxx.y, cxx.z, cxx.w, Rxx.x, Rxx.y};
            const float xz[8] = {Lxz.x, Lxz.y, a2.x, a2.y, a2.z, a2.w, Rxz.x, Rxz.y};
            float d1[4], d2[4], d3[4], d4[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d1[c] = dfw(K, xx[c + 1], xx[c + 2], xx[c + 3], xx[c + 4]);
                d2[c] = dbw(K, comp(a0, c), comp(a1, c), comp(a2, c), comp(a3, c));
                d3[c] = dbw(K, xz[c], xz[c + 1], xz[c + 2], xz[c + 3]);
                d4[c] = dfw(K, comp(b0, c), comp(b1, c), comp(b2, c), comp(b3, c));
            }
            if (xs_off >= 0) {
                float t1[4] = {s1.x, s1.y, s1.z, s1.w}, t3[4] = {s3.x, s3.y, s3.z, s3.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    d1[c] = pml(t1[c], comp(pxah, c), comp(pxbh, c), comp(pxkh, c), d1[c]);
                    d3[c] = pml(t3[c], comp(pxa, c), comp(pxb, c), comp(pxk, c), d3[c]);
                }
                st4(q1, make_float4(t1[0], t1[1], t1[2], t1[3]));
                st4(q3, make_float4(t3[0], t3[1], t3[2], t3[3]));
            }
            if (zs >= 0) {
                float t2[4] = {s2.x, s2.y, s2.z, s2.w}, t4[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    d2[c] = pml(t2[c], za, zb, zk, d2[c]);
                    d4[c] = pml(t4[c], zah, zbh, zkh, d4[c]);
                }
                st4(q2, make_float4(t2[0], t2[1], t2[2], t2[3]));
                st4(q4, make_float4(t4[0], t4[1], t4[2], t4[3]));
            }
            float s4v[4], s5v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { s4v[c] = d1[c] + d2[c]; s5v[c] = d3[c] + d4[c]; }
            vxv.x = fmaf(bxs.x, s4v[0], vxv.x); vxv.y = fmaf(bxs.y, s4v[1], vxv.y);
            vxv.z = fmaf(bxs.z, s4v[2], vxv.z); vxv.w = fmaf(bxs.w, s4v[3], vxv.w);
            vzv.x = fmaf(bzs.x, s5v[0], vzv.x); vzv.y = fmaf(bzs.y, s5v[1], vzv.y);
            vzv.z = fmaf(bzs.z, s5v[2], vzv.z); vzv.w = fmaf(bzs.w, s5v[3], vzv.w);
            if (SAVE == kBorn) {
                vxv.x = fmaf(dbx.x, B3.x, vxv.x); vxv.y = fmaf(dbx.y, B3.y, vxv.y);
                vxv.z = fmaf(dbx.z, B3.z, vxv.z); vxv.w = fmaf(dbx.w, B3.w, vxv.w);
                vzv.x = fmaf(dbz.x, B4.x, vzv.x); vzv.y = fmaf(dbz.y, B4.y, vzv.y);
                vzv.z = fmaf(dbz.z, B4.z, vzv.z); vzv.w = fmaf(dbz.w, B4.w, vzv.w);
            }
            st4(vx + o, vxv);
            st4(vz + o, vzv);
            if (SAVE == 1) {
                float *Sp = p.S + (long long)s * p.snap_shot + snap_cell(p, j, g);
                mifwi::stnt4(Sp + 3 * (long long)p.splane, make_float4(s4v[0], s4v[1], s4v[2], s4v[3]));
                mifwi::stnt4(Sp + 4 * (long long)p.splane, make_float4(s5v[0], s5v[1], s5v[2], s5v[3]));
            } else if (SAVE == 2) {
                bf_store2(p.S + (long long)s * p.snap_shot + bf_reg_de(p.splane), snap_cell(p, j, g) >> 2, s4v, s5v);
            }
            a0 = a1; a1 = a2; a2 = a3;
            b0 = b1; b1 = b2; b2 = b3;
        }
    }
}

// ================================================================================================
// forward S launch: stresses from the new velocities + source injection + receiver sampling
// ================================================================================================
// VTI: sxx = fmaf(c11, e1, fmaf(c13, e2, sxx)), szz = fmaf(c13, e1, fmaf(c33, e2, szz)) with c33 read from plane M_C33 (of
// mat and, Born step, of dmat); c33 == c11 gives the isotropic bits.
// VISCO: q = R e (+ dR S, Born step) from planes M_RL, M_RM, M_RMU; the stress gets (1 + a)/2 r - b/2 q AFTER the fmaf chain and
// r <- a r - b q.  With the three planes zero r stays 0 and the chain's result is stored: the isotropic bits.
template <int LX, int RZ, int SAVE, bool VTI = false, bool VISCO = false>
__global__ __launch_bounds__(kThreads, MIFWI_EL_MINWAVES) void el_step_s(const ElParams p)
{
    const FdK K = p.K;
    constexpr int LZ = kThreads / LX;
    constexpr int TZ = LZ * RZ, TX = LX * 4;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    if (by >= p.tiles_z) {
        sample_points<0>(p, bx, by, bz);
        return;
    }
    __shared__ float inj[TZ * TX];
    const int lx = (int)threadIdx.x % LX, lz = (int)threadIdx.x / LX;
    const int g = bx * LX + lx;
    const int tile_j = by * TZ, tile_i = bx * TX;
    const int j0 = tile_j + lz * RZ;
    const bool active = (g < p.ng) && (j0 < p.nz);
    const unsigned fs = p.field_stride;
    const unsigned col = 4 + 4 * g;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const int xs_off = active ? xstrip(p, g) : -1;
    float4 pxa, pxb, pxk, pxah, pxbh, pxkh;
    if (xs_off >= 0) {
        pxa = ld4(p.px + PA * p.gp + 4 * g); pxb = ld4(p.px + PB * p.gp + 4 * g);
        pxk = ld4(p.px + PK * p.gp + 4 * g); pxah = ld4(p.px + PAH * p.gp + 4 * g);
        pxbh = ld4(p.px + PBH * p.gp + 4 * g); pxkh = ld4(p.px + PKH * p.gp + 4 * g);
    }
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        const bool has_inj = stage_injection<TZ, TX, 1>(p, s, tile_j, tile_i, inj);
        if (active) {
            float *fl = p.fields + (long long)s * p.shot_stride;
            const float *vx = fl + F_VX * fs, *vz = fl + F_VZ * fs;
            float *sxx = fl + F_SXX * fs, *szz = fl + F_SZZ * fs, *sxz = fl + F_SXZ * fs;
            // windows: vz rows j-2..j+1 (a0..a3), vx rows j-1..j+2 (b0..b3)
            float4 a0, a1, a2, a3, b0, b1, b2, b3;
            {
                const unsigned o = (unsigned)(j0 + 2) * p.pitch + col;
                a0 = ld4(vz + o - 2 * p.pitch); a1 = ld4(vz + o - p.pitch); a2 = ld4(vz + o);
                b0 = ld4(vx + o - p.pitch); b1 = ld4(vx + o); b2 = ld4(vx + o + p.pitch);
            }
#pragma unroll
            for (int rz = 0; rz < RZ; ++rz) {
                const int j = j0 + rz;
                if (j < p.nz) {
                    const unsigned o = (unsigned)(j + 2) * p.pitch + col;
                    const unsigned cc = (unsigned)j * p.gp + 4 * g;
                    a3 = ld4(vz + o + p.pitch);
                    b3 = ld4(vx + o + 2 * p.pitch);
                    const float2 Lvx = ld2(vx + o - 2), Rvx = ld2(vx + o + 4);
                    const float2 Lvz = ld2(vz + o - 2), Rvz = ld2(vz + o + 4);
                    float4 vxx = ld4(sxx + o), vzz = ld4(szz + o), vxz = ld4(sxz + o);
                    const float4 Ls = ld4(p.mat + M_L * ncell + cc), Ms = ld4(p.mat + M_M * ncell + cc);
                    const float4 mus = ld4(p.mat + M_MU * ncell + cc);
                    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    float4 Cs = Ms, dC = zero4;                  // the szz-on-ezz modulus and its perturbation: c33 under VTI
                    if (VTI) Cs = ld4(p.mat + M_C33 * ncell + cc);
                    float4 B0 = zero4, B1 = zero4, B2 = zero4, dL = zero4, dM = zero4, dmu = zero4;
                    if (SAVE == kBorn) {
                        const float *Sp = p.S + (long long)s * p.snap_shot + snap_cell(p, j, g);
                        B0 = mifwi::ldnt4(Sp); B1 = mifwi::ldnt4(Sp + (long long)p.splane);
                        B2 = mifwi::ldnt4(Sp + 2 * (long long)p.splane);
                        dL = ld4(p.dmat + M_L * ncell + cc); dM = ld4(p.dmat + M_M * ncell + cc);
                        dmu = ld4(p.dmat + M_MU * ncell + cc);
                        dC = VTI ? ld4(p.dmat + M_C33 * ncell + cc) : dM;
                    }
                    float4 R2s = zero4, R1s = zero4, Rmu = zero4, rxx = zero4, rzz = zero4, rxz = zero4;
                    float4 dR2 = zero4, dR1 = zero4, dRmu = zero4;
                    if (VISCO) {
                        R2s = ld4(p.mat + M_RL * ncell + cc); R1s = ld4(p.mat + M_RM * ncell + cc);
                        Rmu = ld4(p.mat + M_RMU * ncell + cc);
                        rxx = ld4(fl + F_RXX * fs + o); rzz = ld4(fl + F_RZZ * fs + o); rxz = ld4(fl + F_RXZ * fs + o);
                        if (SAVE == kBorn) {
                            dR2 = ld4(p.dmat + M_RL * ncell + cc); dR1 = ld4(p.dmat + M_RM * ncell + cc);
                            dRmu = ld4(p.dmat + M_RMU * ncell + cc);
                        }
                    }
                    const float xv[8] = {Lvx.x, Lvx.y, b1.x, b1.y, b1.z, b1.w, Rvx.x, Rvx.y};
                    const float zv[8] = {Lvz.x, Lvz.y, a2.x, a2.y, a2.z, a2.w, Rvz.x, Rvz.y};
                    float e1[4], e2[4], e3[4], e4[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        e1[c] = dbw(K, xv[c], xv[c + 1], xv[c + 2], xv[c + 3]);
                        e2[c] = dbw(K, comp(a0, c), comp(a1, c), comp(a2, c), comp(a3, c));
                        e3[c] = dfw(K, comp(b0, c), comp(b1, c), comp(b2, c), comp(b3, c));
                        e4[c] = dfw(K, zv[c + 1], zv[c + 2], zv[c + 3], zv[c + 4]);
                    }
                    if (xs_off >= 0) {
                        float *q5 = p.psix + (long long)s * p.psix_shot + ((long long)2 * p.nz + j) * p.wx + xs_off;
                        float *q8 = p.psix + (long long)s * p.psix_shot + ((long long)3 * p.nz + j) * p.wx + xs_off;
                        float4 s5 = ld4(q5), s8 = ld4(q8);
                        float t5[4] = {s5.x, s5.y, s5.z, s5.w}, t8[4] = {s8.x, s8.y, s8.z, s8.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            e1[c] = pml(t5[c], comp(pxa, c), comp(pxb, c), comp(pxk, c), e1[c]);
                            e4[c] = pml(t8[c], comp(pxah, c), comp(pxbh, c), comp(pxkh, c), e4[c]);
                        }
                        st4(q5, make_float4(t5[0], t5[1], t5[2], t5[3]));
                        st4(q8, make_float4(t8[0], t8[1], t8[2], t8[3]));
                    }
                    const int zs = zstrip(p, j);
                    if (zs >= 0) {
                        const float za = p.pz[PA * p.nz + j], zb = p.pz[PB * p.nz + j], zk = p.pz[PK * p.nz + j];
                        const float zah = p.pz[PAH * p.nz + j], zbh = p.pz[PBH * p.nz + j], zkh = p.pz[PKH * p.nz + j];
                        float *q6 = p.psiz + (long long)s * p.psiz_shot + ((long long)2 * 2 * p.W + zs) * p.gp + 4 * g;
                        float *q7 = p.psiz + (long long)s * p.psiz_shot + ((long long)3 * 2 * p.W + zs) * p.gp + 4 * g;
                        float4 s6 = ld4(q6), s7 = ld4(q7);
                        float t6[4] = {s6.x, s6.y, s6.z, s6.w}, t7[4] = {s7.x, s7.y, s7.z, s7.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            e2[c] = pml(t6[c], za, zb, zk, e2[c]);
                            e3[c] = pml(t7[c], zah, zbh, zkh, e3[c]);
                        }
                        st4(q6, make_float4(t6[0], t6[1], t6[2], t6[3]));
                        st4(q7, make_float4(t7[0], t7[1], t7[2], t7[3]));
                    }
                    float nxx[4], nzz[4], nxz[4], s3v[4], mxx[4], mzz[4], mxz[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        s3v[c] = e3[c] + e4[c];
                        nxx[c] = fmaf(comp(Ms, c), e1[c], fmaf(comp(Ls, c), e2[c], comp(vxx, c)));
                        nzz[c] = fmaf(comp(Ls, c), e1[c], fmaf(comp(Cs, c), e2[c], comp(vzz, c)));
                        nxz[c] = fmaf(comp(mus, c), s3v[c], comp(vxz, c));
                        if (SAVE == kBorn) {
                            nxx[c] = fmaf(comp(dM, c), comp(B0, c), fmaf(comp(dL, c), comp(B1, c), nxx[c]));
                            nzz[c] = fmaf(comp(dL, c), comp(B0, c), fmaf(comp(dC, c), comp(B1, c), nzz[c]));
                            nxz[c] = fmaf(comp(dmu, c), comp(B2, c), nxz[c]);
                        }
                        if (VISCO) {
                            const float ha = 0.5f * (1.f + p.rel_a), hb = 0.5f * p.rel_b;
                            float qxx = fmaf(comp(R1s, c), e1[c], comp(R2s, c) * e2[c]);
                            float qzz = fmaf(comp(R2s, c), e1[c], comp(R1s, c) * e2[c]);
                            float qxz = comp(Rmu, c) * s3v[c];
                            if (SAVE == kBorn) {
                                qxx = fmaf(comp(dR1, c), comp(B0, c), fmaf(comp(dR2, c), comp(B1, c), qxx));
                                qzz = fmaf(comp(dR2, c), comp(B0, c), fmaf(comp(dR1, c), comp(B1, c), qzz));
                                qxz = fmaf(comp(dRmu, c), comp(B2, c), qxz);
                            }
                            nxx[c] += fmaf(ha, comp(rxx, c), -(hb * qxx));
                            nzz[c] += fmaf(ha, comp(rzz, c), -(hb * qzz));
                            nxz[c] += fmaf(ha, comp(rxz, c), -(hb * qxz));
                            mxx[c] = fmaf(p.rel_a, comp(rxx, c), -(p.rel_b * qxx));
                            mzz[c] = fmaf(p.rel_a, comp(rzz, c), -(p.rel_b * qzz));
                            mxz[c] = fmaf(p.rel_a, comp(rxz, c), -(p.rel_b * qxz));
                        }
                        if (has_inj) {
                            const float a = inj[(j - tile_j) * TX + 4 * lx + c];
                            nxx[c] += a;
                            nzz[c] += a;
                        }
                        if (p.fsurf && j == 0) nzz[c] = 0.f;
                    }
                    st4(sxx + o, make_float4(nxx[0], nxx[1], nxx[2], nxx[3]));
                    st4(szz + o, make_float4(nzz[0], nzz[1], nzz[2], nzz[3]));
                    st4(sxz + o, make_float4(nxz[0], nxz[1], nxz[2], nxz[3]));
                    if (VISCO) {
                        st4(fl + F_RXX * fs + o, make_float4(mxx[0], mxx[1], mxx[2], mxx[3]));
                        st4(fl + F_RZZ * fs + o, make_float4(mzz[0], mzz[1], mzz[2], mzz[3]));
                        st4(fl + F_RXZ * fs + o, make_float4(mxz[0], mxz[1], mxz[2], mxz[3]));
                    }
                    if (SAVE == 1) {
                        float *Sp = p.S + (long long)s * p.snap_shot + snap_cell(p, j, g);
                        mifwi::stnt4(Sp, make_float4(e1[0], e1[1], e1[2], e1[3]));
                        mifwi::stnt4(Sp + (long long)p.splane, make_float4(e2[0], e2[1], e2[2], e2[3]));
                        mifwi::stnt4(Sp + 2 * (long long)p.splane, make_float4(s3v[0], s3v[1], s3v[2], s3v[3]));
                    } else if (SAVE == 2) {
                        float *Sp = p.S + (long long)s * p.snap_shot;
                        bf_store2(Sp, snap_cell(p, j, g) >> 2, e1, e2);
                        bf_store1(Sp + bf_reg_c(p.splane), snap_cell(p, j, g) >> 2, s3v);
                    }
                    a0 = a1; a1 = a2; a2 = a3;
                    b0 = b1; b1 = b2; b2 = b3;
                }
            }
        }
        if (has_inj) __syncthreads();
    }
}

// ================================================================================================
// adjoint launches, on the tile of mifwi_stagger.h (ATZ x 4*AGO owned cells, staged on ASZ x ASX in LDS)
// ================================================================================================

// staged coordinates of the halo group a thread stages besides its own group (threads 0..kHalo-1):
// the two rows above and below the tile, then the left/right halo group of every owned row
constexpr int kHalo = 4 * AGX + 2 * ATZ;
__device__ __forceinline__ void halo_item(int h, int &sr, int &sg)
{
    if (h < 4 * AGX) {
        const int q = h / AGX;
        sr = q < 2 ? q : ATZ + q;
        sg = h - q * AGX;
    } else {
        const int k = h - 4 * AGX;
        sr = 2 + (k >> 1);
        sg = (k & 1) * (AGX - 1);
    }
}

struct AdjIn { float4 a, b, c, m0, m1, m2; };
struct AdjInVti : AdjIn { float4 m3; };     // + c33 (m0 = c13, m1 = c11, m2 = c44_xz)

// E1..E4 of one group: C^T sigma_bar through the transposed C-PML (memory variables written by the owner)
__device__ __forceinline__ const float4 &adj_c33(const AdjIn &in) { return in.m1; }
__device__ __forceinline__ const float4 &adj_c33(const AdjInVti &in) { return in.m3; }
// viscoelastic: + R2, R1, mu_r tau_s (m3, m4, m5) and w = -b (r_bar + sigma_bar / 2), the adjoint of q (adj_w)
struct AdjInVisco : AdjIn { float4 m3, m4, m5, wa, wb, wc; };
__device__ __forceinline__ const float4 &adj_c33(const AdjInVisco &in) { return in.m1; }
__device__ __forceinline__ float4 adj_w(float b, const float4 &rb, const float4 &sb)
{
    return make_float4(-b * fmaf(0.5f, sb.x, rb.x), -b * fmaf(0.5f, sb.y, rb.y), -b * fmaf(0.5f, sb.z, rb.z),
                       -b * fmaf(0.5f, sb.w, rb.w));
}
// E += R^T w before the transposed C-PML (nothing for the lossless media)
__device__ __forceinline__ void adj_relax(const AdjIn &, int, float &, float &, float &) {}
__device__ __forceinline__ void adj_relax(const AdjInVisco &in, int c, float &e1, float &e2, float &e3)
{
    e1 += fmaf(comp(in.m4, c), comp(in.wa, c), comp(in.m3, c) * comp(in.wb, c));
    e2 += fmaf(comp(in.m3, c), comp(in.wa, c), comp(in.m4, c) * comp(in.wb, c));
    e3 += comp(in.m5, c) * comp(in.wc, c);
}
template <class In>
__device__ __forceinline__ void stage_E(const ElParams &p, int s, int j, int g, const In &in, bool mine,
                                        float4 &E1, float4 &E2, float4 &E3, float4 &E4)
{
    float e1[4], e2[4], e3[4], e4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        e1[c] = fmaf(comp(in.m1, c), comp(in.a, c), comp(in.m0, c) * comp(in.b, c));
        e2[c] = fmaf(comp(in.m0, c), comp(in.a, c), comp(adj_c33(in), c) * comp(in.b, c));
        e3[c] = comp(in.m2, c) * comp(in.c, c);
        adj_relax(in, c, e1[c], e2[c], e3[c]);
        e4[c] = e3[c];
    }
    const int xs_off = xstrip(p, g);
    if (xs_off >= 0) {
        const float4 pxa = ld4(p.px + PA * p.gp + 4 * g), pxb = ld4(p.px + PB * p.gp + 4 * g);
        const float4 pxk = ld4(p.px + PK * p.gp + 4 * g), pxah = ld4(p.px + PAH * p.gp + 4 * g);
        const float4 pxbh = ld4(p.px + PBH * p.gp + 4 * g), pxkh = ld4(p.px + PKH * p.gp + 4 * g);
        const long long q5 = (long long)s * p.psix_shot + ((long long)2 * p.nz + j) * p.wx + xs_off;
        const long long q8 = (long long)s * p.psix_shot + ((long long)3 * p.nz + j) * p.wx + xs_off;
        const float4 s5 = ld4(p.psix + q5), s8 = ld4(p.psix + q8);
        float n5[4], n8[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e1[c] = pmlT(comp(s5, c), comp(pxa, c), comp(pxb, c), comp(pxk, c), e1[c], n5[c]);
            e4[c] = pmlT(comp(s8, c), comp(pxah, c), comp(pxbh, c), comp(pxkh, c), e4[c], n8[c]);
        }
        if (mine) {
            st4(p.psix_out + q5, make_float4(n5[0], n5[1], n5[2], n5[3]));
            st4(p.psix_out + q8, make_float4(n8[0], n8[1], n8[2], n8[3]));
        }
    }
    const int zs = zstrip(p, j);
    if (zs >= 0) {
        const float za = p.pz[PA * p.nz + j], zb = p.pz[PB * p.nz + j], zk = p.pz[PK * p.nz + j];
        const float zah = p.pz[PAH * p.nz + j], zbh = p.pz[PBH * p.nz + j], zkh = p.pz[PKH * p.nz + j];
        const long long q6 = (long long)s * p.psiz_shot + ((long long)2 * 2 * p.W + zs) * p.gp + 4 * g;
        const long long q7 = (long long)s * p.psiz_shot + ((long long)3 * 2 * p.W + zs) * p.gp + 4 * g;
        const float4 s6 = ld4(p.psiz + q6), s7 = ld4(p.psiz + q7);
        float n6[4], n7[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e2[c] = pmlT(comp(s6, c), za, zb, zk, e2[c], n6[c]);
            e3[c] = pmlT(comp(s7, c), zah, zbh, zkh, e3[c], n7[c]);
        }
        if (mine) {
            st4(p.psiz_out + q6, make_float4(n6[0], n6[1], n6[2], n6[3]));
            st4(p.psiz_out + q7, make_float4(n7[0], n7[1], n7[2], n7[3]));
        }
    }
    E1 = make_float4(e1[0], e1[1], e1[2], e1[3]); E2 = make_float4(e2[0], e2[1], e2[2], e2[3]);
    E3 = make_float4(e3[0], e3[1], e3[2], e3[3]); E4 = make_float4(e4[0], e4[1], e4[2], e4[3]);
}

// S^T:  E = C^T sigma_bar through the transposed C-PML;  v_bar -= stencils(E);  all five material-gradient
//       accumulators.  The adjoint sources of the tile's cells (v_bar += R^T g, which the oracle applies at the head
//       of an adjoint step) are added to the loaded v_bar first, through the E planes while they are still empty
//       (p.tile_start set; null when the call has no receivers).
// Every global load of a shot (own group, halo group, adjoint velocities, the five snapshot planes) is
// requested before the first use: one memory round trip per shot instead of three.
// Register budget pinned at three waves per SIMD (<= 168 VGPRs; 146 in use since the plane loads address as uniform
// base + 32-bit lane offset and the C-PML branches derive their addresses from opaque indices - 207 before): three
// workgroups per CU, 768 workgroup slots.  1000x3000 adjoint pair 885 -> 853-864 us per step.
// VTI: six accumulators per group - acc[M_M] (c11) takes S1 sxx_bar alone, acc[M_C33] takes S2 szz_bar, acc[M_L] (c13) is
// the isotropic lambda sum; E2 uses c33 (stage_E).  158 VGPRs, no scratch: the bound of three waves per SIMD holds.
// VISCO: eight accumulators; w = -b (r_bar + sigma_bar / 2) on own and halo cells from the OLD r_bar (read only here: the
// neighbouring tiles stage it too - el_adj_v_visco advances it), E += R^T w in stage_E, acc[M_RM] += S1 wxx + S2 wzz,
// acc[M_RL] += S2 wxx + S1 wzz, acc[M_RMU] += S3 wxz.  A register bound of its own, two waves per SIMD: r_bar and three
// more planes on own and halo cells, w across the barrier and three more accumulators do not fit 168 VGPRs (bound at
// three waves the compiler reports 168 VGPRs and 132 B of scratch per lane).
constexpr int kAdjWavesVisco = 2;
template <bool BF16, bool VTI = false, bool VISCO = false>
__global__ __launch_bounds__(kThreads, VISCO ? kAdjWavesVisco : 3) void el_adj_s(const ElParams p)
{
    constexpr int NACC = VISCO ? 8 : VTI ? 6 : 5;
    const FdK K = p.K;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    if (by >= p.tiles_z) {
        sample_points<1>(p, bx, by, bz);
        return;
    }
    __shared__ float E[4][ASZ][ASX];
    const int tile_j = by * ATZ;
    const int tile_g = bx * AGO;           // first owned group
    const unsigned fs = p.field_stride;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const int t = (int)threadIdx.x;
    const int orow = t / AGO, ogrp = t % AGO;
    const int oj = tile_j + orow, og = tile_g + ogrp;
    const bool own_ok = oj < p.nz && og < p.ng;
    const unsigned occ = (unsigned)oj * p.gp + 4 * og;
    const unsigned oo = (unsigned)(oj + 2) * p.pitch + 4 + 4 * og;
    const unsigned osc = snap_cell(p, oj, og);          // snapshot and accumulator planes
    int hr = 0, hg = 0;
    if (t < kHalo) halo_item(t, hr, hg);
    const int hj = tile_j - 2 + hr, hgg = tile_g - 1 + hg;
    const bool halo_ok = t < kHalo && hj >= 0 && hj < p.nz && hgg >= 0 && hgg < p.ng;
    const unsigned hcc = (unsigned)hj * p.gp + 4 * hgg;
    const unsigned ho = (unsigned)(hj + 2) * p.pitch + 4 + 4 * hgg;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[NACC];
    typename std::conditional<VISCO, AdjInVisco, typename std::conditional<VTI, AdjInVti, AdjIn>::type>::type own, halo;
    own.m0 = own.m1 = own.m2 = halo.m0 = halo.m1 = halo.m2 = zero4;
    if constexpr (VTI) own.m3 = halo.m3 = zero4;
    if constexpr (VISCO) own.m3 = own.m4 = own.m5 = halo.m3 = halo.m4 = halo.m5 = zero4;
    if (own_ok) {
#pragma unroll
        for (int k = 0; k < NACC; ++k)       // accumulator planes share the snapshot planes' layout (snap_cell)
            acc[k] = ld4(el_at(p.acc + ((long long)(p.s0 / p.gs + bz) * NACC + k) * p.splane, osc));
        own.m0 = ld4(el_at(p.mat + M_L * ncell, occ)); own.m1 = ld4(el_at(p.mat + M_M * ncell, occ));
        own.m2 = ld4(el_at(p.mat + M_MU * ncell, occ));
        if constexpr (VTI) own.m3 = ld4(el_at(p.mat + M_C33 * ncell, occ));
        if constexpr (VISCO) {
            own.m3 = ld4(el_at(p.mat + M_RL * ncell, occ)); own.m4 = ld4(el_at(p.mat + M_RM * ncell, occ));
            own.m5 = ld4(el_at(p.mat + M_RMU * ncell, occ));
        }
    }
    if (halo_ok) {
        halo.m0 = ld4(el_at(p.mat + M_L * ncell, hcc)); halo.m1 = ld4(el_at(p.mat + M_M * ncell, hcc));
        halo.m2 = ld4(el_at(p.mat + M_MU * ncell, hcc));
        if constexpr (VTI) halo.m3 = ld4(el_at(p.mat + M_C33 * ncell, hcc));
        if constexpr (VISCO) {
            halo.m3 = ld4(el_at(p.mat + M_RL * ncell, hcc)); halo.m4 = ld4(el_at(p.mat + M_RM * ncell, hcc));
            halo.m5 = ld4(el_at(p.mat + M_RMU * ncell, hcc));
        }
    }
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        float *fl = p.fields + (long long)s * p.shot_stride;
        float4 vxb = zero4, vzb = zero4, S1 = zero4, S2 = zero4, S3 = zero4, S4 = zero4, S5 = zero4;
        BfPlanes packed;
        packed.ab = packed.de = mifwi_u4{0u, 0u, 0u, 0u};
        packed.c = mifwi_u2{0u, 0u};
        own.a = own.b = own.c = halo.a = halo.b = halo.c = zero4;
        if (own_ok) {
            own.a = ld4(el_at(fl + F_SXX * fs, oo)); own.b = ld4(el_at(fl + F_SZZ * fs, oo)); own.c = ld4(el_at(fl + F_SXZ * fs, oo));
        }
        if (halo_ok) {
            halo.a = ld4(el_at(fl + F_SXX * fs, ho)); halo.b = ld4(el_at(fl + F_SZZ * fs, ho)); halo.c = ld4(el_at(fl + F_SXZ * fs, ho));
        }
        if (own_ok) { vxb = ld4(el_at(fl + F_VX * fs, oo)); vzb = ld4(el_at(fl + F_VZ * fs, oo)); }
        if constexpr (VISCO) {            // r_bar for now; w once sigma_bar zz of a free surface is cleared
            own.wa = own.wb = own.wc = halo.wa = halo.wb = halo.wc = zero4;
            if (own_ok) {
                own.wa = ld4(el_at(fl + F_RXX * fs, oo)); own.wb = ld4(el_at(fl + F_RZZ * fs, oo)); own.wc = ld4(el_at(fl + F_RXZ * fs, oo));
            }
            if (halo_ok) {
                halo.wa = ld4(el_at(fl + F_RXX * fs, ho)); halo.wb = ld4(el_at(fl + F_RZZ * fs, ho)); halo.wc = ld4(el_at(fl + F_RXZ * fs, ho));
            }
        }
        // ---- adjoint sources of this tile (workgroup-uniform branch; E[0], E[1] are free until the staging) -----
        if (p.tile_start != nullptr) {
            const int ntiles = (int)gridDim.x * p.tiles_z, per = p.ninj * p.ntap_inj;
            const int *ts = p.tile_start + (long long)s * (ntiles + 1) + by * (int)gridDim.x + bx;
            const int e0 = ts[0], e1 = ts[1];
            if (e1 > e0) {
                const int x = 4 * (ogrp + 1);
                st4(&E[0][orow + 2][x], zero4); st4(&E[1][orow + 2][x], zero4);
                __syncthreads();
                for (int e = e0 + t; e < e1; e += kThreads) {
                    const int tap = p.tile_list[(long long)s * per + e];
                    const int cell = p.inj_cell[(long long)s * per + tap];
                    const int j = cell / p.nx, i = cell - j * p.nx;
                    const float w = p.inj_w[(long long)s * per + tap];
                    const long long ai = (long long)s * p.ninj + tap / p.ntap_inj;
                    atomicAdd(&E[0][j - tile_j + 2][i - 4 * tile_g + 4], w * p.inj_amp0[ai]);
                    atomicAdd(&E[1][j - tile_j + 2][i - 4 * tile_g + 4], w * p.inj_amp1[ai]);
                }
                __syncthreads();
                const float4 ix = ld4(&E[0][orow + 2][x]), iz = ld4(&E[1][orow + 2][x]);
                vxb = make_float4(vxb.x + ix.x, vxb.y + ix.y, vxb.z + ix.z, vxb.w + ix.w);
                vzb = make_float4(vzb.x + iz.x, vzb.y + iz.y, vzb.z + iz.z, vzb.w + iz.w);
                __syncthreads();
            }
        }
        // ---- stage E1..E4 on the tile + halo -------------------------------------------------
        if (p.fsurf && oj == 0) own.b = zero4;            // adjoint of szz(0,.) is discarded
        if (p.fsurf && hj == 0) halo.b = zero4;
        if constexpr (VISCO) {
            own.wa = adj_w(p.rel_b, own.wa, own.a); own.wb = adj_w(p.rel_b, own.wb, own.b); own.wc = adj_w(p.rel_b, own.wc, own.c);
            halo.wa = adj_w(p.rel_b, halo.wa, halo.a); halo.wb = adj_w(p.rel_b, halo.wb, halo.b); halo.wc = adj_w(p.rel_b, halo.wc, halo.c);
        }
        {
            float4 E1 = zero4, E2 = zero4, E3 = zero4, E4 = zero4;
            if (own_ok) stage_E(p, s, f_opaque(oj), f_opaque(og), own, true, E1, E2, E3, E4);
            const int x = 4 * (ogrp + 1);
            st4(&E[0][orow + 2][x], E1); st4(&E[1][orow + 2][x], E2);
            st4(&E[2][orow + 2][x], E3); st4(&E[3][orow + 2][x], E4);
        }
        if (t < kHalo) {
            float4 E1 = zero4, E2 = zero4, E3 = zero4, E4 = zero4;
            if (halo_ok) stage_E(p, s, f_opaque(hj), f_opaque(hgg), halo, false, E1, E2, E3, E4);
            st4(&E[0][hr][4 * hg], E1); st4(&E[1][hr][4 * hg], E2);
            st4(&E[2][hr][4 * hg], E3); st4(&E[3][hr][4 * hg], E4);
        }
        // the snapshot planes are only needed after the barrier: requested last, they do not delay the staging
        if (own_ok && !BF16) {
            const float *Sp = p.S + (long long)s * p.snap_shot;
            const long long sp = p.splane;
            S1 = mifwi::ldnt4(el_at(Sp, osc)); S2 = mifwi::ldnt4(el_at(Sp + sp, osc)); S3 = mifwi::ldnt4(el_at(Sp + 2 * sp, osc));
            S4 = mifwi::ldnt4(el_at(Sp + 3 * sp, osc)); S5 = mifwi::ldnt4(el_at(Sp + 4 * sp, osc));
        } else if (own_ok) {
            bf_request(p.S + (long long)s * p.snap_shot, p.splane, osc >> 2, packed);
        }
        __syncthreads();
        // ---- stencils from LDS + injection + gradient accumulation ---------------------------
        if (own_ok) {
            const int r = orow + 2, cb = 4 * (ogrp + 1);
            const float4 bxx = own.a, bzz = own.b, bxz = own.c;
            float nvx[4], nvz[4];
            const Row8 x1 = row8(&E[0][r][0], cb), x4 = row8(&E[3][r][0], cb);
            const float4 z3a = ld4(&E[2][r - 2][cb]), z3b = ld4(&E[2][r - 1][cb]);
            const float4 z3c = ld4(&E[2][r][cb]), z3d = ld4(&E[2][r + 1][cb]);
            const float4 z2a = ld4(&E[1][r - 1][cb]), z2b = ld4(&E[1][r][cb]);
            const float4 z2c = ld4(&E[1][r + 1][cb]), z2d = ld4(&E[1][r + 2][cb]);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float dx1 = dfw(K, x1.v[c + 1], x1.v[c + 2], x1.v[c + 3], x1.v[c + 4]);
                const float dz3 = dbw(K, comp(z3a, c), comp(z3b, c), comp(z3c, c), comp(z3d, c));
                const float dz2 = dfw(K, comp(z2a, c), comp(z2b, c), comp(z2c, c), comp(z2d, c));
                const float dx4 = dbw(K, x4.v[c], x4.v[c + 1], x4.v[c + 2], x4.v[c + 3]);
                float ax = comp(vxb, c) - (dx1 + dz3);
                float az = comp(vzb, c) - (dz2 + dx4);
                if (4 * og + c >= p.nx) { ax = 0.f; az = 0.f; }
                nvx[c] = ax; nvz[c] = az;
            }
            st4(el_at(fl + F_VX * fs, oo), make_float4(nvx[0], nvx[1], nvx[2], nvx[3]));
            st4(el_at(fl + F_VZ * fs, oo), make_float4(nvz[0], nvz[1], nvz[2], nvz[3]));
            // gradients (oracle order): Ms, Ls, mus from sigma_bar; bxs, bzs from the new v_bar
            if (BF16) {
                bf_pin(packed);
                bf_widen(packed, S1, S2, S3, S4, S5);
            }
#define ACC3(dst, a, b, c_, d) dst = fmaf(a, b, fmaf(c_, d, dst))
            if constexpr (VTI) {
                acc[M_M].x = fmaf(S1.x, bxx.x, acc[M_M].x); acc[M_M].y = fmaf(S1.y, bxx.y, acc[M_M].y);
                acc[M_M].z = fmaf(S1.z, bxx.z, acc[M_M].z); acc[M_M].w = fmaf(S1.w, bxx.w, acc[M_M].w);
                acc[NACC - 1].x = fmaf(S2.x, bzz.x, acc[NACC - 1].x); acc[NACC - 1].y = fmaf(S2.y, bzz.y, acc[NACC - 1].y);
                acc[NACC - 1].z = fmaf(S2.z, bzz.z, acc[NACC - 1].z); acc[NACC - 1].w = fmaf(S2.w, bzz.w, acc[NACC - 1].w);
            } else {
            ACC3(acc[M_M].x, S1.x, bxx.x, S2.x, bzz.x); ACC3(acc[M_M].y, S1.y, bxx.y, S2.y, bzz.y);
            ACC3(acc[M_M].z, S1.z, bxx.z, S2.z, bzz.z); ACC3(acc[M_M].w, S1.w, bxx.w, S2.w, bzz.w);
            }
            ACC3(acc[M_L].x, S2.x, bxx.x, S1.x, bzz.x); ACC3(acc[M_L].y, S2.y, bxx.y, S1.y, bzz.y);
            ACC3(acc[M_L].z, S2.z, bxx.z, S1.z, bzz.z); ACC3(acc[M_L].w, S2.w, bxx.w, S1.w, bzz.w);
#undef ACC3
            acc[M_MU].x = fmaf(S3.x, bxz.x, acc[M_MU].x); acc[M_MU].y = fmaf(S3.y, bxz.y, acc[M_MU].y);
            acc[M_MU].z = fmaf(S3.z, bxz.z, acc[M_MU].z); acc[M_MU].w = fmaf(S3.w, bxz.w, acc[M_MU].w);
            if constexpr (VISCO) {
#define ACC3(dst, a, b, c_, d) dst = fmaf(a, b, fmaf(c_, d, dst))
                const float4 wxx = own.wa, wzz = own.wb, wxz = own.wc;
                ACC3(acc[M_RM].x, S1.x, wxx.x, S2.x, wzz.x); ACC3(acc[M_RM].y, S1.y, wxx.y, S2.y, wzz.y);
                ACC3(acc[M_RM].z, S1.z, wxx.z, S2.z, wzz.z); ACC3(acc[M_RM].w, S1.w, wxx.w, S2.w, wzz.w);
                ACC3(acc[M_RL].x, S2.x, wxx.x, S1.x, wzz.x); ACC3(acc[M_RL].y, S2.y, wxx.y, S1.y, wzz.y);
                ACC3(acc[M_RL].z, S2.z, wxx.z, S1.z, wzz.z); ACC3(acc[M_RL].w, S2.w, wxx.w, S1.w, wzz.w);
#undef ACC3
                acc[M_RMU].x = fmaf(S3.x, wxz.x, acc[M_RMU].x); acc[M_RMU].y = fmaf(S3.y, wxz.y, acc[M_RMU].y);
                acc[M_RMU].z = fmaf(S3.z, wxz.z, acc[M_RMU].z); acc[M_RMU].w = fmaf(S3.w, wxz.w, acc[M_RMU].w);
            }
            acc[M_BX].x = fmaf(S4.x, nvx[0], acc[M_BX].x); acc[M_BX].y = fmaf(S4.y, nvx[1], acc[M_BX].y);
            acc[M_BX].z = fmaf(S4.z, nvx[2], acc[M_BX].z); acc[M_BX].w = fmaf(S4.w, nvx[3], acc[M_BX].w);
            acc[M_BZ].x = fmaf(S5.x, nvz[0], acc[M_BZ].x); acc[M_BZ].y = fmaf(S5.y, nvz[1], acc[M_BZ].y);
            acc[M_BZ].z = fmaf(S5.z, nvz[2], acc[M_BZ].z); acc[M_BZ].w = fmaf(S5.w, nvz[3], acc[M_BZ].w);
        }
        __syncthreads();          // E is reused by the next shot
    }
    if (own_ok) {
#pragma unroll
        for (int k = 0; k < NACC; ++k)
            st4(el_at(p.acc + ((long long)(p.s0 / p.gs + bz) * NACC + k) * p.splane, osc), acc[k]);
    }
}

// D1..D4 of one group: B^T v_bar through the transposed C-PML
__device__ __forceinline__ void stage_D(const ElParams &p, int s, int j, int g, const float4 &vxb, const float4 &vzb,
                                        const float4 &bxs, const float4 &bzs, bool mine,
                                        float4 &D1, float4 &D2, float4 &D3, float4 &D4)
{
    float d1[4], d2[4], d3[4], d4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        d1[c] = comp(bxs, c) * comp(vxb, c); d2[c] = d1[c];
        d3[c] = comp(bzs, c) * comp(vzb, c); d4[c] = d3[c];
    }
    const int xs_off = xstrip(p, g);
    if (xs_off >= 0) {
        const float4 pxa = ld4(p.px + PA * p.gp + 4 * g), pxb = ld4(p.px + PB * p.gp + 4 * g);
        const float4 pxk = ld4(p.px + PK * p.gp + 4 * g), pxah = ld4(p.px + PAH * p.gp + 4 * g);
        const float4 pxbh = ld4(p.px + PBH * p.gp + 4 * g), pxkh = ld4(p.px + PKH * p.gp + 4 * g);
        const long long q1 = (long long)s * p.psix_shot + ((long long)0 * p.nz + j) * p.wx + xs_off;
        const long long q3 = (long long)s * p.psix_shot + ((long long)1 * p.nz + j) * p.wx + xs_off;
        const float4 s1 = ld4(p.psix + q1), s3 = ld4(p.psix + q3);
        float n1[4], n3[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            d1[c] = pmlT(comp(s1, c), comp(pxah, c), comp(pxbh, c), comp(pxkh, c), d1[c], n1[c]);
            d3[c] = pmlT(comp(s3, c), comp(pxa, c), comp(pxb, c), comp(pxk, c), d3[c], n3[c]);
        }
        if (mine) {
            st4(p.psix_out + q1, make_float4(n1[0], n1[1], n1[2], n1[3]));
            st4(p.psix_out + q3, make_float4(n3[0], n3[1], n3[2], n3[3]));
        }
    }
    const int zs = zstrip(p, j);
    if (zs >= 0) {
        const float za = p.pz[PA * p.nz + j], zb = p.pz[PB * p.nz + j], zk = p.pz[PK * p.nz + j];
        const float zah = p.pz[PAH * p.nz + j], zbh = p.pz[PBH * p.nz + j], zkh = p.pz[PKH * p.nz + j];
        const long long q2 = (long long)s * p.psiz_shot + ((long long)0 * 2 * p.W + zs) * p.gp + 4 * g;
        const long long q4 = (long long)s * p.psiz_shot + ((long long)1 * 2 * p.W + zs) * p.gp + 4 * g;
        const float4 s2 = ld4(p.psiz + q2), s4 = ld4(p.psiz + q4);
        float n2[4], n4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            d2[c] = pmlT(comp(s2, c), za, zb, zk, d2[c], n2[c]);
            d4[c] = pmlT(comp(s4, c), zah, zbh, zkh, d4[c], n4[c]);
        }
        if (mine) {
            st4(p.psiz_out + q2, make_float4(n2[0], n2[1], n2[2], n2[3]));
            st4(p.psiz_out + q4, make_float4(n4[0], n4[1], n4[2], n4[3]));
        }
    }
    D1 = make_float4(d1[0], d1[1], d1[2], d1[3]); D2 = make_float4(d2[0], d2[1], d2[2], d2[3]);
    D3 = make_float4(d3[0], d3[1], d3[2], d3[3]); D4 = make_float4(d4[0], d4[1], d4[2], d4[3]);
}

// V^T:  D = B^T v_bar through the transposed C-PML;  sigma_bar -= stencils(D)
// VISCO: the owner also advances r_bar <- a r_bar + (1 + a)/2 sigma_bar with the sigma_bar this launch loaded, i.e. the one
// S^T saw (zz of a free-surface row counts as 0, as there).  Cell-local, and nothing else reads r_bar in this launch.
template <bool VISCO>
__device__ __forceinline__ void el_adj_v_body(const ElParams &p)
{
    const FdK K = p.K;
    __shared__ float D[4][ASZ][ASX];
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    const int tile_j = by * ATZ;
    const int tile_g = bx * AGO;
    const int s = p.s0 + bz;
    const unsigned fs = p.field_stride;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const int t = (int)threadIdx.x;
    float *fl = p.fields + (long long)s * p.shot_stride;
    const int orow = t / AGO, ogrp = t % AGO;
    const int oj = tile_j + orow, og = tile_g + ogrp;
    const bool own_ok = oj < p.nz && og < p.ng;
    const unsigned occ = (unsigned)oj * p.gp + 4 * og;
    const unsigned oo = (unsigned)(oj + 2) * p.pitch + 4 + 4 * og;
    int hr = 0, hg = 0;
    if (t < kHalo) halo_item(t, hr, hg);
    const int hj = tile_j - 2 + hr, hgg = tile_g - 1 + hg;
    const bool halo_ok = t < kHalo && hj >= 0 && hj < p.nz && hgg >= 0 && hgg < p.ng;
    const unsigned hcc = (unsigned)hj * p.gp + 4 * hgg;
    const unsigned ho = (unsigned)(hj + 2) * p.pitch + 4 + 4 * hgg;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ovx = zero4, ovz = zero4, obx = zero4, obz = zero4, hvx = zero4, hvz = zero4, hbx = zero4, hbz = zero4;
    float4 bxx = zero4, bzz = zero4, bxz = zero4;
    if (own_ok) {
        ovx = ld4(fl + F_VX * fs + oo); ovz = ld4(fl + F_VZ * fs + oo);
        obx = ld4(p.mat + M_BX * ncell + occ); obz = ld4(p.mat + M_BZ * ncell + occ);
    }
    if (halo_ok) {
        hvx = ld4(fl + F_VX * fs + ho); hvz = ld4(fl + F_VZ * fs + ho);
        hbx = ld4(p.mat + M_BX * ncell + hcc); hbz = ld4(p.mat + M_BZ * ncell + hcc);
    }
    if (own_ok) {
        bxx = ld4(fl + F_SXX * fs + oo); bzz = ld4(fl + F_SZZ * fs + oo); bxz = ld4(fl + F_SXZ * fs + oo);
    }
    {
        float4 D1 = zero4, D2 = zero4, D3 = zero4, D4 = zero4;
        if (own_ok) stage_D(p, s, oj, og, ovx, ovz, obx, obz, true, D1, D2, D3, D4);
        const int x = 4 * (ogrp + 1);
        st4(&D[0][orow + 2][x], D1); st4(&D[1][orow + 2][x], D2);
        st4(&D[2][orow + 2][x], D3); st4(&D[3][orow + 2][x], D4);
    }
    if (t < kHalo) {
        float4 D1 = zero4, D2 = zero4, D3 = zero4, D4 = zero4;
        if (halo_ok) stage_D(p, s, hj, hgg, hvx, hvz, hbx, hbz, false, D1, D2, D3, D4);
        st4(&D[0][hr][4 * hg], D1); st4(&D[1][hr][4 * hg], D2);
        st4(&D[2][hr][4 * hg], D3); st4(&D[3][hr][4 * hg], D4);
    }
    __syncthreads();
    if (own_ok) {
        const int r = orow + 2, cb = 4 * (ogrp + 1);
        float nxx[4], nzz[4], nxz[4];
        const Row8 x1 = row8(&D[0][r][0], cb), x3 = row8(&D[2][r][0], cb);
        const float4 z2a = ld4(&D[1][r - 1][cb]), z2b = ld4(&D[1][r][cb]);
        const float4 z2c = ld4(&D[1][r + 1][cb]), z2d = ld4(&D[1][r + 2][cb]);
        const float4 z4a = ld4(&D[3][r - 2][cb]), z4b = ld4(&D[3][r - 1][cb]);
        const float4 z4c = ld4(&D[3][r][cb]), z4d = ld4(&D[3][r + 1][cb]);
        float4 m12 = zero4, m13 = zero4, m32 = zero4;
        if (p.fsurf && oj < 2) { m12 = ld4(&D[1][2][cb]); m13 = ld4(&D[1][3][cb]); m32 = ld4(&D[3][2][cb]); }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dx1 = dbw(K, x1.v[c], x1.v[c + 1], x1.v[c + 2], x1.v[c + 3]);
            const float dz2 = dfw(K, comp(z2a, c), comp(z2b, c), comp(z2c, c), comp(z2d, c));
            const float dx3 = dfw(K, x3.v[c + 1], x3.v[c + 2], x3.v[c + 3], x3.v[c + 4]);
            const float dz4 = dbw(K, comp(z4a, c), comp(z4b, c), comp(z4c, c), comp(z4d, c));
            nxx[c] = comp(bxx, c) - dx1;
            nxz[c] = comp(bxz, c) - (dz2 + dx3);
            nzz[c] = comp(bzz, c) - dz4;
            if (p.fsurf && oj < 2) {
                // transposed odd mirroring (tile_j == 0 here: staged row 2 is grid row 0)
                if (oj == 0) nxz[c] = nxz[c] + fmaf(K.c1, comp(m12, c), K.c2 * comp(m13, c));
                else { nxz[c] = nxz[c] + K.c2 * comp(m12, c); nzz[c] = nzz[c] + K.c2 * comp(m32, c); }
            }
            if (4 * og + c >= p.nx) { nxx[c] = 0.f; nxz[c] = 0.f; nzz[c] = 0.f; }
        }
        st4(fl + F_SXX * fs + oo, make_float4(nxx[0], nxx[1], nxx[2], nxx[3]));
        st4(fl + F_SZZ * fs + oo, make_float4(nzz[0], nzz[1], nzz[2], nzz[3]));
        st4(fl + F_SXZ * fs + oo, make_float4(nxz[0], nxz[1], nxz[2], nxz[3]));
        if (VISCO) {
            const float ha = 0.5f * (1.f + p.rel_a);
            if (p.fsurf && oj == 0) bzz = zero4;
            const float4 rxx = ld4(fl + F_RXX * fs + oo), rzz = ld4(fl + F_RZZ * fs + oo), rxz = ld4(fl + F_RXZ * fs + oo);
            st4(fl + F_RXX * fs + oo, make_float4(fmaf(p.rel_a, rxx.x, ha * bxx.x), fmaf(p.rel_a, rxx.y, ha * bxx.y),
                                                  fmaf(p.rel_a, rxx.z, ha * bxx.z), fmaf(p.rel_a, rxx.w, ha * bxx.w)));
            st4(fl + F_RZZ * fs + oo, make_float4(fmaf(p.rel_a, rzz.x, ha * bzz.x), fmaf(p.rel_a, rzz.y, ha * bzz.y),
                                                  fmaf(p.rel_a, rzz.z, ha * bzz.z), fmaf(p.rel_a, rzz.w, ha * bzz.w)));
            st4(fl + F_RXZ * fs + oo, make_float4(fmaf(p.rel_a, rxz.x, ha * bxz.x), fmaf(p.rel_a, rxz.y, ha * bxz.y),
                                                  fmaf(p.rel_a, rxz.z, ha * bxz.z), fmaf(p.rel_a, rxz.w, ha * bxz.w)));
        }
    }
}
__global__ __launch_bounds__(kThreads) void el_adj_v(const ElParams p) { el_adj_v_body<false>(p); }
__global__ __launch_bounds__(kThreads) void el_adj_v_visco(const ElParams p) { el_adj_v_body<true>(p); }

#include "mifwi_elastic_fused.h"
#include "mifwi_tti.h"

// receivers of the state in p.fields (the last step of a fused range)
__global__ __launch_bounds__(kThreads) void el_sample_v(const ElParams p)
{
    sample_points<0>(p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// ---- point forces (source_type 1 / 2): a handful of cells per shot, launches of their own ---------------------
// forward: v[cell] += w * f[n] between V and S.  One thread per shot walks its sources in order (several
// sources may share a cell: no atomics, the sum order is fixed).
__global__ void el_inject_force(const ElParams p, int comp)
{
    const int s = p.s0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= p.nshot || s >= p.s0 + p.gs) return;
    float *v = p.fields + (long long)s * p.shot_stride + (comp == 1 ? F_VX : F_VZ) * (long long)p.field_stride;
    for (int e = 0; e < p.ninj * p.ntap_inj; ++e) {
        const long long ee = (long long)s * p.ninj * p.ntap_inj + e;
        const int cell = p.inj_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        v[(unsigned)(j + 2) * p.pitch + 4 + i] += p.inj_w[ee] * p.inj_amp0[(long long)s * p.ninj + e / p.ntap_inj];
    }
}

// ---- pressure receivers (desc.record_pressure): launches of their own on the per-step path -----------------
// forward: rec_p[n] = sum w (sxx + szz)[cell] after S and the source term, for the p.gs shots of this pass
__global__ void el_sample_pressure(const ElParams p)
{
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= p.gs * p.nsmp) return;
    const int s = p.s0 + idx / p.nsmp;
    if (s >= p.nshot) return;
    const int e = s * p.nsmp + idx % p.nsmp;
    const float *fl = p.fields + (long long)s * p.shot_stride;
    float a = 0.f;
    for (int t = 0; t < p.ntap_smp; ++t) {
        const long long ee = (long long)e * p.ntap_smp + t;
        const int cell = p.smp_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        const unsigned off = (unsigned)(j + 2) * p.pitch + 4 + i;
        a = fmaf(p.smp_w[ee], fl[F_SXX * (long long)p.field_stride + off] + fl[F_SZZ * (long long)p.field_stride + off], a);
    }
    p.smp_out0[e] = a;
}

// adjoint: sxx_bar, szz_bar [cell] += w g_p[n] before S^T (receivers normally sit on distinct cells; taps that
// share a cell add in hardware order, as in the LDS staging of the velocity receivers)
__global__ void el_inject_pressure(const ElParams p)
{
    const int per = p.ninj * p.ntap_inj;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= p.gs * per) return;
    const int s = p.s0 + idx / per, r = idx % per;
    if (s >= p.nshot) return;
    const long long ee = (long long)s * per + r;
    const int cell = p.inj_cell[ee];
    if (cell < 0) return;
    const int j = cell / p.nx, i = cell - j * p.nx;
    const unsigned off = (unsigned)(j + 2) * p.pitch + 4 + i;
    float *fl = p.fields + (long long)s * p.shot_stride;
    const float a = p.inj_w[ee] * p.inj_amp0[(long long)s * p.ninj + r / p.ntap_inj];
    atomicAdd(fl + F_SXX * (long long)p.field_stride + off, a);
    atomicAdd(fl + F_SZZ * (long long)p.field_stride + off, a);
}

#include "mifwi_elastic_cluster.h"

using mifwi::env_int;

// ---- the medium of a plan ---------------------------------------------------------------------------
// Every plan of this file is a mifwi_elastic_plan; its medium says which kernels serve it and how many planes they take.
// Isotropic plans have all kernel families; the other media run one launch per half step: el_step_s / el_adj_s with VTI
// or VISCO = true, el_adj_v_visco, finalize_groups<6> / <8> (el_step_variant, el_adj_variant).  A further medium is a row
// here, a case in those two selectors and its three entry points.  TTI plans run the kernels of mifwi_tti.h in place of
// el_step_s / el_adj_s (tti_step_variant; el_two_launch_steps and el_backward launch them).
enum ElMedium { kIsotropic = 0, kVti = 1, kVisco = 2, kTti = 3 };
struct ElMediumInfo {
    int nmat;                // material / gradient / accumulator planes
    int nfield;              // fields per shot: the five of the scheme (+ the three memory variables F_RXX..F_RXZ)
    const char *created_by;  // the family's plan_create, as messages name it
};
constexpr ElMediumInfo kMedia[] = {{5, 5, "mifwi_elastic_plan_create"}, {6, 5, "mifwi_vti_plan_create"},
                                   {8, 8, "mifwi_visco_plan_create"}, {8, 5, "mifwi_tti_plan_create"}};

}  // namespace

// ================================================================================================
struct mifwi_elastic_plan : StaggerGrid {    // grid, pitch and strips: stagger_grid with four memory variables per strip cell
    mifwi_elastic_desc d;
    int device;
    int lx, rz, gs, ngroups;
    int xcd;
    float *rec_p;          // pressure receivers bound by mifwi_elastic_plan_bind_pressure (or null)
    const float *g_p;
    int snap_bf16;         // snapshot planes as bf16 (per-step kernels on both sides only)
    long long snap_shot;   // floats per shot of one snapshot step
    long long splane;      // floats per snapshot plane
    int sblk;              // snapshot planes blocked by columns of 16 groups (snap_cell)
    int pass_shots;        // forward per-step family: shots per pass over the time range
    int pass_groups;       // adjoint per-step family: shot groups per pass
    int fused;             // forward V+S in one launch (second copy of the state in the work buffer)
    int fused_pass_shots;  // shots per pass of the fused forward (both copies of the state in the Infinity Cache)
    long long shot_stride, fields_elems, psix_elems, psiz_elems;
    long long psi_elems;  // psix+psiz rounded up to 64
    // cluster path (LDS-resident time loop); 0 when a shot does not fit
    int cluster, NW, PL, fwd_PL, adj_PL, cl_shots, cl_lds, cl_ng;
    int cl_xh, adj_xh;           // single-launch kernels fetch the x-stencils' outer cells from the neighbouring lanes (ec_xhalo)
    // adjoint cluster kernel (its own slab count: different LDS footprint)
    int cl_adj, adj_NW, adj_shots, adj_lds, adj_ng, adj_zrows;
    long long xbuf_elems, list_elems, xcc_elems;
    long long tile_elems;                  // per-tile receiver lists of el_adj_s (ints, in floats)
    ElMedium medium;       // kMedia[medium]: its planes, fields and entry points
    float rel_a, rel_b;    // the relaxation scalars of a viscoelastic plan (ElParams)
};
// a VTI or viscoelastic plan is an elastic plan of that medium (el_plan_create); the C ABI keeps the handle types apart
struct mifwi_vti_plan;
struct mifwi_visco_plan;
struct mifwi_tti_plan;

namespace {

ElParams el_base(const mifwi_elastic_plan *pl, const float *mat, const float *pz, const float *px)
{
    ElParams p;
    memset(&p, 0, sizeof(p));
    p.nz = pl->d.nz; p.nx = pl->d.nx; p.ng = pl->ng; p.gp = pl->gp; p.pitch = pl->pitch;
    p.field_stride = (unsigned)pl->field_stride; p.shot_stride = pl->shot_stride;
    p.nshot = pl->d.nshot; p.gs = 1;
    p.W = pl->W; p.wl = pl->wl; p.xr0 = pl->xr0; p.wx = pl->wx;
    p.fsurf = pl->d.free_surface;
    p.psix_shot = pl->psix_shot; p.psiz_shot = pl->psiz_shot;
    p.mat = mat; p.pz = pz; p.px = px;
    p.xcd = pl->xcd;
    p.snap_shot = pl->snap_shot;
    p.splane = (unsigned)pl->splane; p.sblk = pl->sblk;
    p.K = fd_weights(pl->d.fd_order);
    p.rel_a = pl->rel_a; p.rel_b = pl->rel_b;
    return p;
}

using mifwi::with_bool;
using mifwi::with_int;

// ---- variant tables (mifwi_host.h) ----------------------------------------------------------------
// the two launches of a per-step forward step, el_step_v<LX, 1, SAVE> (every medium's) / el_step_s<LX, 1, SAVE, VTI, VISCO>:
// lanes per row 64 | 32 | 16; save kBorn | 2 (bf16 planes; isotropic only) | 1 (f32 planes) | 0
using ElKernel = void (*)(ElParams);
struct ElStepKernels { ElKernel v, s; };
ElStepKernels el_step_variant(ElMedium medium, int lx, int save)
{
    return with_int<64, 32, 16>(lx, [&](auto LX) {
    return with_int<kVisco, kVti, kIsotropic>(medium, [&](auto M) {
        auto pair = [](auto SAVE) {
            constexpr int L = decltype(LX)::value, S = decltype(SAVE)::value, Md = decltype(M)::value;
            return ElStepKernels{el_step_v<L, 1, S>, el_step_s<L, 1, S, Md == kVti, Md == kVisco>};
        };
        if constexpr (decltype(M)::value == kIsotropic) return with_int<kBorn, 2, 1, 0>(save, pair);
        else return with_int<kBorn, 1, 0>(save, pair);
    }); });
}
// the V launch alone (every medium's) and the two launches of a TTI stress half step: lanes per row 64 | 32 | 16; Born or not
ElKernel el_step_v_variant(int lx, int save) { return el_step_variant(kVti, lx, save).v; }
using TtiKernel = void (*)(TtiParams);
struct TtiStepKernels { TtiKernel strain, stress; };
TtiStepKernels tti_step_variant(int lx, bool born)
{
    return with_int<64, 32, 16>(lx, [&](auto LX) {
    return with_bool(born, [&](auto B) {
        constexpr int L = decltype(LX)::value;
        return TtiStepKernels{tti_strain<L>, tti_stress<L, decltype(B)::value>};
    }); });
}
// el_fwd_fused<SAVE>: save 2 | 1 | 0 (no Born form: that pass runs the two launches)
ElKernel el_fwd_fused_variant(int save)
{
    return with_int<2, 1, 0>(save, [](auto SAVE) -> ElKernel { return el_fwd_fused<decltype(SAVE)::value>; });
}
// the three kernels of the per-step adjoint: S^T (bf16 planes: isotropic plans only), V^T and the sum over the shot groups
using ElFinalizeKernel = void (*)(const float *, int, int, int, long long, int, float *);
struct ElAdjKernels { ElKernel s, v; ElFinalizeKernel finalize; };
ElAdjKernels el_adj_variant(ElMedium medium, bool bf16)
{
    switch (medium) {
    case kVti: return {el_adj_s<false, true>, el_adj_v, finalize_groups<6>};
    case kVisco: return {el_adj_s<false, false, true>, el_adj_v_visco, finalize_groups<8>};
    case kTti: return {nullptr, el_adj_v, finalize_groups<8>};       // S^T: tti_adj_e + tti_adj_s (el_backward)
    default: return {bf16 ? el_adj_s<true> : el_adj_s<false>, el_adj_v, finalize_groups<5>};
    }
}
// el_cluster_fwd<SAVE, NG, AG, XH>: snapshots; one | two groups per thread; granules published at agent scope; x-halo from
// the neighbouring lanes.  The agent-scope tier keeps the plain reads (one variant less to build): AG takes XH off.
using EcKernel = void (*)(EcParams);
EcKernel el_cluster_fwd_variant(bool save, int ng, bool agent, bool xh)
{
    return with_bool(save, [&](auto SAVE) {
    return with_int<1, 2>(ng, [&](auto NG) {
    return with_bool(agent, [&](auto AG) {
    return with_bool(xh, [&](auto XH) -> EcKernel {
        constexpr bool A = decltype(AG)::value;
        return el_cluster_fwd<decltype(SAVE)::value, decltype(NG)::value, A, decltype(XH)::value && !A>;
    }); }); }); });
}
// el_cluster_adj<NG, AG, XH>: as above
using EaKernel = void (*)(EaParams);
EaKernel el_cluster_adj_variant(int ng, bool agent, bool xh)
{
    return with_int<1, 2>(ng, [&](auto NG) {
    return with_bool(agent, [&](auto AG) {
    return with_bool(xh, [&](auto XH) -> EaKernel {
        constexpr bool A = decltype(AG)::value;
        return el_cluster_adj<decltype(NG)::value, A, decltype(XH)::value && !A>;
    }); }); });
}

template <class P>
void launch_v(const mifwi_elastic_plan *pl, void (*kernel)(P), const P &p, int nshot, hipStream_t st)
{
    const int lz = kThreads / pl->lx;
    dim3 grid(mifwi::ceil_div(pl->ng, pl->lx), mifwi::ceil_div(pl->d.nz, lz), nshot);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, p);
}

template <class P>
void launch_s(const mifwi_elastic_plan *pl, void (*kernel)(P), const P &p0, int nshot, hipStream_t st)
{
    const int lz = kThreads / pl->lx;
    const int tiles_x = mifwi::ceil_div(pl->ng, pl->lx);
    P p = p0;
    p.tiles_z = mifwi::ceil_div(pl->d.nz, lz);
    int extra = 0;
    if (p.smp_out0 != nullptr && p.nsmp > 0)
        extra = mifwi::ceil_div(mifwi::ceil_div(p.gs * p.nsmp, kThreads), tiles_x);
    dim3 grid(tiles_x, p.tiles_z + extra, mifwi::ceil_div(nshot, p.gs));
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, p);
}

// Slab count (both loops): cost of a step ~ fixed part (barriers, two hand-off flights) + groups per
// thread, times the launches the shot batch needs (measured on 100x300: 6 shots 8.7 us at 8 slabs,
// 7.2 us at 20).  Few shots -> many thin slabs; a full batch -> the fewest slabs that fit.
// lds_of(slabs, rows of the tallest, LDS row pitch): the loop's dynamic LDS in bytes, which must stay within `limit`;
// where the wide (skewed) pitch does not fit a slab height, the plain one is tried.  NW == 0: nothing fits.
struct SlabChoice { int NW, shots, lds, PL, ng; };
template <class LdsOf>
SlabChoice slab_search(const mifwi_elastic_plan *pl, int ncu, int forced, int PL_wide, int PL_plain, long long limit, LdsOf lds_of)
{
    SlabChoice best{0, 0, 0, 0, 0};
    double best_cost = 1e30;
    for (int nw = 1; nw <= 32; ++nw) {
        if (forced > 0 && nw != forced) continue;
        if (pl->d.nz / nw < 4) break;
        const int rows = mifwi::ceil_div(pl->d.nz, nw);
        int PLq = PL_wide;
        long long lds = lds_of(nw, rows, PLq);
        if (lds > limit && PLq != PL_plain) {          // the wider rows do not fit this slab height: plain pitch
            PLq = PL_plain;
            lds = lds_of(nw, rows, PLq);
        }
        if (lds > limit) continue;
        if ((long long)rows * pl->ng > 2 * kEcThreads || kEcRowFields * pl->gp > kEcGr * kEcThreads) continue;
        const int per_launch = 8 * (ncu / (8 * nw));
        if (per_launch < 8) break;
        const double cost = mifwi::ceil_div(pl->d.nshot, per_launch) * (4.8 + (double)rows * pl->ng / kEcThreads);
        if (cost < best_cost - 1e-9) {
            best_cost = cost;
            best = {nw, per_launch, (int)lds, PLq, mifwi::ceil_div(rows * pl->ng, kEcThreads)};
        }
    }
    return best;
}
// LDS rows the adjoint loop reserves for the z-strip memory variables: the most C-PML rows any slab holds
int ea_zrows_max(const mifwi_elastic_plan *pl, int nw)
{
    int zmax = 0;
    for (int w = 0; w < nw && pl->W > 0; ++w) {
        int r0, R;
        slab_rows(pl->d.nz, nw, 0, w, r0, R);
        const int ntop = std::max(0, std::min(r0 + R, pl->W) - r0);
        const int nbot = std::max(0, r0 + R - std::max(r0, pl->d.nz - pl->W));
        zmax = std::max(zmax, ntop + nbot);
    }
    return zmax;
}

void el_cluster_setup(mifwi_elastic_plan *pl)
{
    pl->cluster = 0; pl->NW = 0; pl->PL = 4 * (pl->ng + 2); pl->cl_shots = 0;
    pl->cl_xh = 0; pl->adj_xh = 0;
    pl->adj_PL = pl->PL; pl->fwd_PL = pl->PL;
    // LDS row pitch: with the dense group -> thread deal (lane v <-> group v of the slab, row-major) a wave's 64 lanes
    // cross a row break almost always; the 16-byte slot of lane v stays congruent to v (mod 16) across the break - and
    // every ds_read_b128 lane group conflict-free - iff the pitch in slots is congruent to the groups per row
    // (measured on 100x300: SQ_LDS_BANK_CONFLICT of the forward loop -22 %, step 6.20 -> 6.07 us; the adjoint's LDS
    // has no room for the wider rows at 8 slabs).  MIFWI_EL_PL_SKEW: bit 0 forward (default on), bit 1 adjoint.
    const int skew = env_int("MIFWI_EL_PL_SKEW", 1);
    int Pskew = pl->ng + 2;
    while ((Pskew - pl->ng) % 16) ++Pskew;
    const int PL_plain = pl->PL;
    if (skew & 1) pl->PL = 4 * Pskew;
    if (skew & 2) pl->adj_PL = 4 * Pskew;
    pl->cl_lds = 0; pl->xbuf_elems = 0; pl->xcc_elems = 0;
    pl->cl_adj = 0; pl->adj_NW = 0; pl->adj_shots = 0; pl->adj_lds = 0; pl->adj_ng = 0; pl->adj_zrows = 0; pl->list_elems = 0;
    pl->tile_elems = tile_taps_elems(pl->d.nshot, pl->d.nz, pl->ng, pl->d.nrec, pl->d.ntap);
    if (pl->medium != kIsotropic || pl->d.ntap != 1 || pl->d.source_type != 0 || pl->d.record_pressure) return;   // per-step kernels only
    const bool want_fwd = env_int("MIFWI_EL_CLUSTER", 1) != 0;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device) != hipSuccess) return;
    const int forced = env_int("MIFWI_EL_NW", 0);
    if (want_fwd) {
        const SlabChoice f = slab_search(pl, ncu, forced, pl->PL, PL_plain, mifwi::kClusterLdsLimit, [&](int, int rows, int PLq) {
            return (5LL * (rows + 4) * PLq + 6LL * pl->gp + 8LL * rows + 8) * (long long)sizeof(float);
        });
        if (f.NW > 0) {
            pl->cluster = 1; pl->NW = f.NW; pl->cl_shots = f.shots; pl->cl_lds = f.lds; pl->cl_ng = f.ng; pl->fwd_PL = f.PL;
        }
    }
    // every slab's deal must suit the lane-shift form of the x-halo (ec_xhalo_deal_ok); MIFWI_EL_XHALO=0: plain LDS reads
    auto xhalo_ok = [&](int nw, int ngq) {
        if (env_int("MIFWI_EL_XHALO", 1) == 0) return 0;
        for (int w = 0; w < nw; ++w) {
            int r0, R;
            slab_rows(pl->d.nz, nw, 0, w, r0, R);
            if (!ec_xhalo_deal_ok(R, pl->ng, ngq * kEcThreads)) return 0;
        }
        return 1;
    };
    pl->cl_xh = pl->cluster ? xhalo_ok(pl->NW, pl->cl_ng) : 0;
    // (a failed attribute call: one launch per half step)
    static std::atomic<unsigned> fwd_attr_done{0}, adj_attr_done{0};
    if (pl->cluster && !mifwi::lds_cap_once(fwd_attr_done, pl->device, mifwi::kClusterLdsLimit, 16, [](int v) {
            return el_cluster_fwd_variant(v & 8, 1 + (v >> 2 & 1), v & 2, v & 1); }))
        pl->cluster = 0;
    // adjoint: four E/D planes + the adjoint memory variables of the slab's C-PML cells in LDS; the
    // gradient accumulators are per shot, so it needs shot groups of one (not used when the caller
    // asked for a group size)
    const int forced_adj = env_int("MIFWI_EL_ADJ_NW", forced);
    if (env_int("MIFWI_EL_CLUSTER_ADJ", 1) != 0 && pl->d.shots_per_group <= 0) {
        // (pl->adj_PL: the candidate pitch, MIFWI_EL_PL_SKEW bit 1, until the search says what the chosen slabs use)
        const SlabChoice a = slab_search(pl, ncu, forced_adj, pl->adj_PL, PL_plain, kEaLdsLimit, [&](int nw, int rows, int PLq) {
            return (4LL * (rows + 4) * PLq + 6LL * pl->gp + 8LL * rows + 4LL * rows * pl->wx + 4LL * ea_zrows_max(pl, nw) * pl->gp +
                    (rows + 4) + 2LL * kEaRcvRows * PLq) * (long long)sizeof(float);   // + row map, receiver rows
        });
        if (a.NW > 0) {
            pl->cl_adj = 1; pl->adj_NW = a.NW; pl->adj_shots = a.shots; pl->adj_lds = a.lds; pl->adj_PL = a.PL;
            pl->adj_ng = a.ng; pl->adj_zrows = ea_zrows_max(pl, a.NW);
        }
        pl->adj_xh = pl->cl_adj ? xhalo_ok(pl->adj_NW, pl->adj_ng) : 0;
        if (pl->cl_adj && !mifwi::lds_cap_once(adj_attr_done, pl->device, kEaLdsLimit, 8, [](int v) {
                return el_cluster_adj_variant(1 + (v >> 2 & 1), v & 2, v & 1); }))
            pl->cl_adj = 0;
    }
    const int nwmax = std::max(pl->cluster ? pl->NW : 0, pl->cl_adj ? pl->adj_NW : 0);
    // granules, the XCC_ID table of mifwi::same_xcd ([nshot][nwmax] ints) and the block of the error word
    pl->xcc_elems = nwmax > 0 ? mifwi::handoff_xcc_elems(pl->d.nshot, nwmax) : 0;
    if (nwmax > 0)
        pl->xbuf_elems = mifwi::handoff_elems(2LL * pl->d.nshot * nwmax * 4 * kEcRowFields * pl->gp, pl->xcc_elems);
    if (pl->cl_adj)
        pl->list_elems = mifwi::round_up64((long long)pl->d.nshot * pl->adj_NW * (1 + pl->d.nrec), 64);
}

// ---- the work buffer ---------------------------------------------------------------------------------
// Offsets (in floats) of its regions.  Forward call:  [fields | psi | bbox | xbuf | backup]   or, fused plans,
// [fields | psi | bbox | second];  backward call:  [fields | psi | psiB | acc | bbox | xbuf | lists | backup | tile].
// fields, the C-PML memory variables (backward: two copies that ping-pong, absolute in n) and the gradient accumulators
// (backward) are the `state`: what a call hands to the call that resumes it, what MIFWI_ZERO_STATE zeroes and what a
// rolled-back single-launch attempt gets back from `backup`.  xbuf (hand-off buffer), lists (receivers per slab) and
// backup exist only where the call's single-launch kernel does; tile: the per-tile receiver lists of el_adj_s.
// second: the fused forward's other copy of the state.  It starts where xbuf does: a plan has one or the other (`fused`
// needs `!cluster`), and the fused loop first touches it after a single-launch attempt has been given up and rolled
// back, when nobody reads xbuf or backup any more; `total` counts room for both all the same.
// strain (TTI plans): three planes per shot of the snapshot planes' layout behind everything else - the strains between
// tti_strain and tti_stress (forward and Born; unused while the step's snapshot planes take them), e_bar between tti_adj_e
// and tti_adj_s (backward).  Scratch inside a step: not part of the state.
struct ElWork { long long fields, psi, psiB, acc, bbox, xbuf, lists, backup, second, tile, strain, state, total; };
ElWork work_map(const mifwi_elastic_plan *pl, bool backward)
{
    const bool single = backward ? pl->cl_adj : pl->cluster;
    ElWork m;
    m.fields = 0; m.psi = pl->fields_elems; m.psiB = m.psi + pl->psi_elems;
    m.acc = backward ? m.psiB + pl->psi_elems : m.psiB;
    m.state = m.acc + (backward ? (long long)kMedia[pl->medium].nmat * pl->ngroups * pl->splane : 0);      // accumulator planes: the snapshot planes' layout and size
    m.bbox = m.state; m.xbuf = m.bbox + mifwi::round_up64(4LL * pl->d.nshot, 64);
    m.lists = m.xbuf + (single ? pl->xbuf_elems : 0);
    m.backup = m.lists + (single && backward ? pl->list_elems : 0);
    m.second = m.xbuf; m.tile = m.backup + (single ? m.state : 0);
    m.strain = backward ? m.tile + pl->tile_elems : m.tile + (pl->fused ? m.state : 0);
    m.total = m.strain + (pl->medium == kTti ? 3LL * pl->d.nshot * pl->splane : 0);
    return m;
}

// what EcParams and EaParams share: geometry, strides, layer, materials, stencil weights, hand-off buffer, knobs
template <class Params>
Params cluster_base(const mifwi_elastic_plan *pl, int NW, int PL, const float *mat, const float *pz, const float *px,
                    const mifwi::Handoff &h)
{
    Params c;
    memset(&c, 0, sizeof(c));
    const mifwi_elastic_desc &d = pl->d;
    c.nz = d.nz; c.nx = d.nx; c.ng = pl->ng; c.gp = pl->gp; c.pitch = pl->pitch;
    c.field_stride = (unsigned)pl->field_stride; c.shot_stride = pl->shot_stride;
    c.nshot = d.nshot; c.NW = NW; c.PL = PL;
    c.W = pl->W; c.wl = pl->wl; c.xr0 = pl->xr0; c.wx = pl->wx; c.fsurf = d.free_surface;
    c.psix_shot = pl->psix_shot; c.psiz_shot = pl->psiz_shot;
    c.mat = mat; c.pz = pz; c.px = px;
    c.nsrc = d.nsrc; c.nrec = d.nrec;
    c.xbuf = h.granules; c.err = h.err; c.xcc_tab = h.xcc_tab;
    c.dbg = env_int("MIFWI_EL_CL_DBG", 0);
    c.nap = mifwi::poll_nap_default(mifwi::ceil_div(d.nz, NW), 8);
    c.K = fd_weights(d.fd_order);
    return c;
}

// the kernels of one single-launch attempt over the shot batches (AG / agent: granules published at agent scope)
// (EcParams and an el_cluster_fwd, or EaParams and an el_cluster_adj; NW, shots, lds: that loop's slab count, batch, LDS)
template <class Params>
void el_cluster_launch(const mifwi_elastic_plan *pl, void (*kernel)(Params), int NW, int shots, int lds, Params c, hipStream_t st)
{
    for (int s0 = 0; s0 < pl->d.nshot; s0 += shots) {
        c.shot0 = s0;
        c.shot1 = std::min(pl->d.nshot, s0 + shots);
        const int nsl8 = mifwi::ceil_div(c.shot1 - s0, 8);
        hipLaunchKernelGGL(kernel, dim3(8 * NW * nsl8), dim3(kEcThreads), lds, st, c);
    }
}

// The two-launch per-step time loop over the steps [n_begin, n_end): mifwi_elastic_forward's plain form (save 0, 1, 2:
// `snap` is written) and the Born pass (save 3: `snap` is the background run's, read; p.dmat set; p.fields / psix / psiz
// hold the perturbed state; f is the source perturbation or null).  The planes of step n are at
// snap + (n - snap_first) * snap_step.  rec_vx null: no sampling.
void el_two_launch_steps(const mifwi_elastic_plan *pl, ElParams p, int save, const float *f, const int32_t *src_cell,
                         const float *src_w, const int *bbox, const int32_t *rec_cell, const float *rec_w, float *rec_vx,
                         float *rec_vz, float *snap, int snap_first, int n_begin, int n_end, float *strain, hipStream_t st)
{
    const mifwi_elastic_desc &d = pl->d;
    const long long snap_step = pl->snap_shot * d.nshot;
    const bool want_rec = rec_vx != nullptr;
    const bool tti = pl->medium == kTti;       // `strain`: the TTI plan's three work planes per shot (ElWork), else unused
    const ElStepKernels step = tti ? ElStepKernels{el_step_v_variant(pl->lx, save), nullptr} : el_step_variant(pl->medium, pl->lx, save);
    const TtiStepKernels tstep = tti_step_variant(pl->lx, save == kBorn);
    ElParams ps = p;
    const bool force = d.source_type != 0;      // point force: injected into vx / vz by a launch of its own
    ps.ninj = (force || !f) ? 0 : d.nsrc; ps.ntap_inj = d.ntap; ps.inj_cell = src_cell; ps.inj_w = src_w;
    ps.inj_bbox = bbox;
    ElParams pf = p;
    pf.ninj = d.nsrc; pf.ntap_inj = d.ntap; pf.inj_cell = src_cell; pf.inj_w = src_w;
    ps.nsmp = want_rec ? d.nrec : 0; ps.ntap_smp = d.ntap; ps.smp_cell = rec_cell; ps.smp_w = rec_w;
    // shots are independent: taken a few at a time, their state and the materials stay inside the
    // 256 MiB Infinity Cache from one launch to the next (pl->pass_shots; all shots when they fit anyway)
    for (int s0 = 0; s0 < d.nshot; s0 += pl->pass_shots) {
        const int cs = std::min(pl->pass_shots, d.nshot - s0);
        p.s0 = ps.s0 = s0;
        for (int n = n_begin; n < n_end; ++n) {
            float *Sn = snap ? snap + (long long)(n - snap_first) * snap_step : nullptr;
            p.S = Sn; ps.S = Sn;
            ps.inj_amp0 = f ? f + (long long)n * d.nshot * d.nsrc : nullptr;
            ps.smp_out0 = want_rec ? rec_vx + (long long)n * d.nshot * d.nrec : nullptr;
            ps.smp_out1 = want_rec ? rec_vz + (long long)n * d.nshot * d.nrec : nullptr;
            launch_v(pl, step.v, p, cs, st);
            if (force && d.nsrc > 0 && f) {
                pf.s0 = s0; pf.gs = cs; pf.inj_amp0 = ps.inj_amp0;
                hipLaunchKernelGGL(el_inject_force, dim3(mifwi::ceil_div(cs, 64)), dim3(64), 0, st, pf,
                                   d.source_type);
            }
            if (tti) {
                // the strains go into the step's snapshot planes 0..2 where those are written, else into the work planes
                TtiParams q;
                static_cast<ElParams &>(q) = ps;
                q.E = save == 1 ? Sn : strain;
                q.e_shot = save == 1 ? pl->snap_shot : 3 * pl->splane;
                launch_v(pl, tstep.strain, q, cs, st);
                launch_s(pl, tstep.stress, q, cs, st);
            } else {
                launch_s(pl, step.s, ps, cs, st);
            }
            if (pl->rec_p && want_rec) {
                ElParams pq = ps;
                pq.s0 = s0; pq.gs = cs; pq.smp_out0 = pl->rec_p + (long long)n * d.nshot * d.nrec;
                hipLaunchKernelGGL(el_sample_pressure, dim3(mifwi::ceil_div(cs * d.nrec, 64)), dim3(64), 0, st, pq);
            }
        }
    }
}

// rel_a, rel_b: the relaxation scalars of a viscoelastic plan
int el_plan_create(mifwi_elastic_plan **plan, int device, const mifwi_elastic_desc *d, ElMedium medium, float rel_a = 0.f,
                   float rel_b = 0.f)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    int rc = check_stagger_desc(d, 4);
    if (rc) return rc;
    if (d->record_pressure != 0 && d->record_pressure != 1)
        return mifwi::fail(MIFWI_EINVAL, "record_pressure must be 0 or 1");
    if ((rc = check_stagger_scheme(d))) return rc;
    if (d->snapshot_format != MIFWI_SNAPSHOT_F32 && d->snapshot_format != MIFWI_SNAPSHOT_BF16)
        return mifwi::fail(MIFWI_EINVAL, "snapshot_format must be MIFWI_SNAPSHOT_F32 or MIFWI_SNAPSHOT_BF16");
    if ((rc = mifwi::check_device(device))) return rc;
    // function attributes and CU counts queried during set-up belong to THIS device (one process per
    // GPU sees all eight devices)
    MIFWI_HIP_TRY(hipSetDevice(device));
    StaggerGrid grid;
    if ((rc = stagger_grid(d->nz, d->nx, d->pml_width, 4, &grid))) return rc;
    mifwi_elastic_plan *pl = new mifwi_elastic_plan;
    static_cast<StaggerGrid &>(*pl) = grid;
    pl->d = *d;
    if (pl->d.fd_order == 0) pl->d.fd_order = 4;
    pl->device = device;
    pl->medium = medium;
    pl->rel_a = rel_a; pl->rel_b = rel_b;
    pl->rec_p = nullptr; pl->g_p = nullptr;
    pl->shot_stride = kMedia[medium].nfield * pl->field_stride;
    pl->fields_elems = pl->shot_stride * d->nshot;
    pl->psix_elems = pl->psix_shot * d->nshot;
    pl->psiz_elems = pl->psiz_shot * d->nshot;
    pl->lx = mifwi::pick_lx(pl->ng);
    { const int v = env_int("MIFWI_EL_LX", 0); if (v == 16 || v == 32 || v == 64) pl->lx = v; }
    pl->rz = 1;
    // 3: tile-major, shots of the launch back to back through every tile (xcd_tile); 1: every XCD walks one contiguous run of
    // the tiles of each shot; 2: whole shots per XCD.  Measured (r04): 350x1700 x 6 shots forward 43.5 -> 40.5 us per step
    // with 3 against 1, adjoint pair and the 1000x3000 passes (2-3 shots per launch) unchanged
    pl->xcd = env_int("MIFWI_EL_XCD", 3);
    // MIFWI_EL_GS, where set, names the size as the caller's shots_per_group does (no 4 -> 3 rule then)
    pl->gs = default_group_size(d->shots_per_group > 0 ? d->shots_per_group : env_int("MIFWI_EL_GS", 0), d->nshot,
                                env_int("MIFWI_EL_GS", 4));
    pl->ngroups = mifwi::ceil_div(d->nshot, pl->gs);
    pl->psi_elems = mifwi::round_up64(pl->psix_elems + pl->psiz_elems, 64);
    el_cluster_setup(pl);
    // bf16 snapshot planes: the per-step kernels only (the single-launch time loops are not bound by the
    // snapshot stream, and their grids' snapshots fit in memory many times over)
    pl->snap_bf16 = d->snapshot_format == MIFWI_SNAPSHOT_BF16 && !pl->cluster && !pl->cl_adj;
    // column-blocked snapshot planes (snap_cell): plans that never run a single-launch kernel (those write and read
    // row-major planes, and a call may change family between checkpoint segments); MIFWI_EL_SNAP_BLOCKED=0: row-major
    pl->sblk = (!pl->cluster && !pl->cl_adj && env_int("MIFWI_EL_SNAP_BLOCKED", 1) != 0) ? 1 : 0;
    pl->splane = pl->sblk ? blocked_plane_elems(d->nz, pl->ng) : pl->coef_elems;
    pl->snap_shot = pl->snap_bf16 ? mifwi::round_up64(5 * pl->splane / 2, 4) : 5 * pl->splane;
    {
        // Infinity Cache residency (per-step family, large grids): a pass over the time range takes only as
        // many shots as keep state + materials (+ gradient accumulators) under kResident bytes; measured on
        // 1000x3000: forward 3 shots (240 MB) 0.61 ms, 4 shots (300 MB) 0.82 ms = the all-shots time
        constexpr double kResident = 250e6;
        const double cells = (double)pl->coef_elems;
        const double mats = 4.0 * kMedia[medium].nmat * cells;
        const double psi1 = 4.0 * (double)(pl->psix_elems + pl->psiz_elems) / d->nshot;
        const double fstate = 4.0 * (double)pl->shot_stride + psi1;
        // forward a little below the adjoint's bound: 1000x3000 runs 0.61 ms with 3 shots (240 MB) and 0.62 ms with 2
        // (180 MB), but a set that close to the cache size fell back to the all-shots time on some boxes (acoustic plan)
        const int ps = env_int("MIFWI_EL_PASS_SHOTS", mifwi::units_per_pass(d->nshot, fstate, mats, kResident, 230e6, 1));
        pl->pass_shots = std::min(d->nshot, std::max(1, ps));
        // adjoint: groups of gs shots share one accumulator set; when the groups do not all fit, smaller groups
        // (more accumulator traffic, 40/gs B per cell-step) can still pay: 1000x3000, gs 2, one group per pass
        // 0.87 ms against 0.98 ms for gs 4 over all shots
        const double astate = 4.0 * (double)pl->shot_stride + 2.0 * psi1, accg = mats;
        if (!pl->cl_adj && d->shots_per_group <= 0 && env_int("MIFWI_EL_GS", 0) <= 0 &&
            pl->ngroups * (pl->gs * astate + accg) + mats > kResident) {
            int g = pl->gs;
            while (g > 2 && g * astate + accg + mats > kResident) g /= 2;
            if (g * astate + accg + mats <= kResident && g != pl->gs) {
                pl->gs = g;
                pl->ngroups = mifwi::ceil_div(d->nshot, g);
            }
        }
        // (nothing fits: one pass over all groups)
        const int k = env_int("MIFWI_EL_PASS_GROUPS", mifwi::units_per_pass(pl->ngroups, pl->gs * astate + accg, mats, kResident,
                                                                             kResident, pl->ngroups));
        pl->pass_groups = std::min(pl->ngroups, std::max(1, k));
    }
    // V+S in one launch pays where the time loop has to be cut into Infinity-Cache-sized passes anyway (measured,
    // 1000x3000 x 16 shots: 622 -> 558 us per step, 516 with bf16 planes; 350x1700 x 32: 232 -> 232, 214 -> 209) and
    // on any launch of a million cells or more (350x1700 x 4 shots, the chunks of a shot-chunked gradient pass:
    // 286 -> 260 us per step of all 32 shots)
    pl->fused = medium == kIsotropic && !pl->cluster && d->source_type == 0 && !d->record_pressure &&
                env_int("MIFWI_EL_FUSED", (pl->pass_shots < d->nshot || (double)d->nz * d->nx * d->nshot >= 1e6) ? 1 : 0) != 0;
    {
        const double cells = (double)pl->coef_elems, mats = 4.0 * 5.0 * cells;
        const double fstate = 4.0 * (double)pl->shot_stride + 4.0 * (double)(pl->psix_elems + pl->psiz_elems) / d->nshot;
        // (both copies of a shot's state; the bounds of pass_shots)
        const int ps = env_int("MIFWI_EL_FUSED_PASS_SHOTS", mifwi::units_per_pass(d->nshot, 2.0 * fstate, mats, 250e6, 230e6, 1));
        pl->fused_pass_shots = std::min(d->nshot, std::max(1, ps));
    }
    if (pl->cl_adj) {                    // the adjoint cluster kernel keeps one accumulator set per shot
        pl->gs = 1;
        pl->ngroups = d->nshot;
    }
    *plan = pl;
    return MIFWI_OK;
}

}  // namespace

extern "C" {

int mifwi_elastic_plan_create(mifwi_elastic_plan **plan, int device, const mifwi_elastic_desc *d)
{
    return el_plan_create(plan, device, d, kIsotropic);
}

int mifwi_elastic_plan_cluster_slabs(const mifwi_elastic_plan *plan, int32_t adjoint)
{
    if (!plan) return 0;
    return adjoint ? (plan->cl_adj ? plan->adj_NW : 0) : (plan->cluster ? plan->NW : 0);
}

int mifwi_elastic_plan_pass_sizes(const mifwi_elastic_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    if (!plan) return mifwi::fail(MIFWI_EINVAL, "null plan");
    if (forward_shots) *forward_shots = plan->pass_shots;
    if (adjoint_groups) *adjoint_groups = plan->pass_groups;
    return MIFWI_OK;
}

int mifwi_elastic_plan_bind_pressure(mifwi_elastic_plan *plan, float *rec_p, const float *g_p)
{
    if (!plan) return mifwi::fail(MIFWI_EINVAL, "null plan");
    if ((rec_p || g_p) && !plan->d.record_pressure)
        return mifwi::fail(MIFWI_EINVAL, "the plan was created with record_pressure = 0");
    plan->rec_p = rec_p;
    plan->g_p = g_p;
    return MIFWI_OK;
}

int mifwi_elastic_plan_destroy(mifwi_elastic_plan *plan)
{
    delete plan;
    return MIFWI_OK;
}

int mifwi_elastic_plan_layout(const mifwi_elastic_plan *pl, mifwi_elastic_layout *out)
{
    if (!pl || !out) return mifwi::fail(MIFWI_EINVAL, "null plan/layout");
    out->gp = pl->gp; out->pitch = pl->pitch; out->ngroups = pl->ngroups;
    out->shots_per_group = pl->gs;
    out->coef_elems = pl->coef_elems;
    out->snap_step_elems = pl->snap_shot * pl->d.nshot;
    out->snapshot_format = pl->snap_bf16 ? MIFWI_SNAPSHOT_BF16 : MIFWI_SNAPSHOT_F32;
    out->kernel_flags = (pl->cluster ? MIFWI_EL_KERNEL_FWD_SINGLE_LAUNCH : 0) | (pl->cl_adj ? MIFWI_EL_KERNEL_ADJ_SINGLE_LAUNCH : 0) |
                        (pl->fused ? MIFWI_EL_KERNEL_FWD_FUSED_STEP : 0) |
                        (pl->cluster && pl->cl_xh ? MIFWI_EL_KERNEL_FWD_LANE_HALO : 0) |
                        (pl->cl_adj && pl->adj_xh ? MIFWI_EL_KERNEL_ADJ_LANE_HALO : 0);
    const ElWork fwd = work_map(pl, false);
    out->state_elems = fwd.state;
    out->work_forward_elems = fwd.total;
    out->work_backward_elems = work_map(pl, true).total;
    return MIFWI_OK;
}

}  // extern "C"

// ---- the three calls of a plan, whatever its medium: what the entry points of the three families run --------------------
namespace {

int el_forward(mifwi_elastic_plan *pl, const float *mat, const float *pz, const float *px, const float *f,
               const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w, float *rec_vx,
               float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream)
{
    if (!pl || !mat || !pz || !px || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    const mifwi_elastic_desc &d = pl->d;
    int rc = mifwi::check_steps(n_begin, n_end, d.nt);
    if (rc) return rc;
    if (d.nsrc > 0 && (!f || !src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "sources declared but f/src_cell/src_w is null");
    if ((rec_vx || rec_vz) && (!rec_cell || !rec_w || !rec_vx || !rec_vz))
        return mifwi::fail(MIFWI_EINVAL, "receiver output needs rec_cell, rec_w, rec_vx and rec_vz");
    const ElWork m = work_map(pl, false);                 // the state is updated in place
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    float *fields = work + m.fields, *psi_state = work + m.psi;
    int *bbox = reinterpret_cast<int *>(work + m.bbox);
    if (d.nsrc > 0) launch_points_bbox(src_cell, d.nshot, d.nsrc * d.ntap, d.nx, bbox, st);
    ElParams p = el_base(pl, mat, pz, px);
    const long long snap_step = pl->snap_shot * d.nshot;
    const int save = !snap ? 0 : pl->snap_bf16 ? 2 : 1;
    const bool want_rec = rec_vx != nullptr && d.nrec > 0;
    if (pl->cluster && n_end > n_begin) {
        const mifwi::Handoff h = mifwi::cluster_handoff(pl, work, m);
        EcParams c = cluster_base<EcParams>(pl, pl->NW, pl->fwd_PL, mat, pz, px, h);
        c.n_first = n_begin; c.n_last = n_end;
        c.fields = fields; c.psix = psi_state; c.psiz = psi_state + pl->psix_elems;
        c.S = snap; c.s_first = n_begin; c.s_step = snap_step;
        c.src_cell = src_cell; c.src_w = src_w; c.f = f;
        c.rec_cell = rec_cell; c.rec_w = rec_w;
        c.rec_vx = want_rec ? rec_vx : nullptr; c.rec_vz = want_rec ? rec_vz : nullptr;
        const mifwi::TraceSpec ts = {"MIFWI_EL_CL_TRACE", 64 * 8 * 16, "# el_cluster_fwd save=%d steps=%d", snap ? 1 : 0, n_end - n_begin};
        rc = mifwi::cluster_ladder("elastic forward", work, m.state, work + m.backup, flags, st, h, ts,
                                   [&](bool agent, long long *trace) {
            mifwi::set_trace(c, trace);
            el_cluster_launch(pl, el_cluster_fwd_variant(snap != nullptr, pl->cl_ng, agent, pl->cl_xh), pl->NW, pl->cl_shots,
                              pl->cl_lds, c, st);
        });
        if (rc != mifwi::kClusterFellBack) return rc;
    }
    if (pl->fused && n_end > n_begin) {
        // V+S in one launch: the state ping-pongs between the copy at the head of the work buffer and a second
        // one behind the bounding boxes.  Shots are taken a few at a time (both copies of their state stay in the
        // Infinity Cache); a pass with an odd number of steps ends with a copy back of its shots.
        float *B = work + m.second;
        MIFWI_HIP_TRY(hipMemsetAsync(B, 0, sizeof(float) * m.state, st));     // its pad rows / columns stay zero
        ElParams q = p;
        q.ninj = d.nsrc; q.ntap_inj = d.ntap; q.inj_cell = src_cell; q.inj_w = src_w; q.inj_bbox = bbox;
        q.nsmp = want_rec ? d.nrec : 0; q.ntap_smp = d.ntap; q.smp_cell = rec_cell; q.smp_w = rec_w;
        const int tx = mifwi::ceil_div(pl->ng, FTG), tz = mifwi::ceil_div(d.nz, FTZ);
        const int ex = want_rec ? mifwi::ceil_div(mifwi::ceil_div(d.nrec, kThreads), tx) : 0;
        const ElKernel fused = el_fwd_fused_variant(save);
        for (int s0 = 0; s0 < d.nshot; s0 += pl->fused_pass_shots) {
            const int cs = std::min(pl->fused_pass_shots, d.nshot - s0);
            q.s0 = s0;
            q.tiles_z = tz;
            for (int n = n_begin; n < n_end; ++n) {
                const bool even = ((n - n_begin) & 1) == 0;
                float *in = even ? work : B, *out = even ? B : work;
                q.fields = in; q.psix = in + pl->fields_elems; q.psiz = q.psix + pl->psix_elems;
                q.fields_out = out; q.psix_out = out + pl->fields_elems; q.psiz_out = q.psix_out + pl->psix_elems;
                q.S = snap ? snap + (long long)(n - n_begin) * snap_step : nullptr;
                q.inj_amp0 = f ? f + (long long)n * d.nshot * d.nsrc : nullptr;
                // the receivers see the input state: the velocities of step n-1
                const bool smp = want_rec && n > n_begin;
                q.smp_out0 = smp ? rec_vx + (long long)(n - 1) * d.nshot * d.nrec : nullptr;
                q.smp_out1 = smp ? rec_vz + (long long)(n - 1) * d.nshot * d.nrec : nullptr;
                const dim3 grid(tx, tz + (smp ? ex : 0), cs);
                hipLaunchKernelGGL(fused, grid, dim3(kThreads), 0, st, q);
            }
            float *last = ((n_end - n_begin) & 1) ? B : work;
            if (want_rec) {
                q.fields = last; q.tiles_z = 0;
                q.smp_out0 = rec_vx + (long long)(n_end - 1) * d.nshot * d.nrec;
                q.smp_out1 = rec_vz + (long long)(n_end - 1) * d.nshot * d.nrec;
                hipLaunchKernelGGL(el_sample_v, dim3(mifwi::ceil_div(d.nrec, kThreads), 1, cs), dim3(kThreads), 0,
                                   st, q);
            }
            if (last != work) {
                const long long psix1 = pl->psix_shot, psiz1 = pl->psiz_shot;
                MIFWI_HIP_TRY(hipMemcpyAsync(work + s0 * pl->shot_stride, B + s0 * pl->shot_stride,
                                             sizeof(float) * cs * pl->shot_stride, hipMemcpyDeviceToDevice, st));
                if (psix1 > 0)
                    MIFWI_HIP_TRY(hipMemcpyAsync(work + pl->fields_elems + s0 * psix1, B + pl->fields_elems + s0 * psix1,
                                                 sizeof(float) * cs * psix1, hipMemcpyDeviceToDevice, st));
                if (psiz1 > 0)
                    MIFWI_HIP_TRY(hipMemcpyAsync(work + pl->fields_elems + pl->psix_elems + s0 * psiz1,
                                                 B + pl->fields_elems + pl->psix_elems + s0 * psiz1,
                                                 sizeof(float) * cs * psiz1, hipMemcpyDeviceToDevice, st));
            }
        }
    } else {
        p.fields = fields; p.psix = psi_state; p.psiz = psi_state + pl->psix_elems;
        el_two_launch_steps(pl, p, save, f, src_cell, src_w, bbox, rec_cell, rec_w, want_rec ? rec_vx : nullptr,
                            want_rec ? rec_vz : nullptr, snap, n_begin, n_begin, n_end, work + m.strain, st);
    }
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

int el_born(mifwi_elastic_plan *pl, const float *mat, const float *dmat, const float *pz, const float *px, const float *df,
            const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *snap,
            int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin, int32_t n_end, int32_t flags,
            void *stream)
{
    if (!pl || !mat || !pz || !px) return mifwi::fail(MIFWI_EINVAL, "null argument");
    if (!dmat || !snap || !work) return mifwi::fail(MIFWI_EINVAL, "born: dmat, snap and work must not be null");
    const mifwi_elastic_desc &d = pl->d;
    int rc = mifwi::check_steps(n_begin, n_end, d.nt);
    if (!rc) rc = mifwi::check_snapshots(snap_first, n_begin);
    if (rc) return rc;
    if (pl->snap_bf16)
        return mifwi::fail(MIFWI_EINVAL, "born: the plan keeps bf16 snapshot planes; the Born step reads f32 planes");
    if (d.source_type != 0)
        return mifwi::fail(MIFWI_EINVAL, "born: point-force sources (source_type %d) are not served", d.source_type);
    if (d.record_pressure) return mifwi::fail(MIFWI_EINVAL, "born: pressure receivers are not served");
    if (df && d.nsrc > 0 && (!src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "df given but src_cell/src_w is null");
    if ((drec_vx || drec_vz) && (!rec_cell || !rec_w || !drec_vx || !drec_vz))
        return mifwi::fail(MIFWI_EINVAL, "receiver output needs rec_cell, rec_w, drec_vx and drec_vz");
    const ElWork m = work_map(pl, false);                 // the perturbed state: the forward's map of `work`
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    int *bbox = reinterpret_cast<int *>(work + m.bbox);
    const bool inject = df != nullptr && d.nsrc > 0;
    if (inject) launch_points_bbox(src_cell, d.nshot, d.nsrc * d.ntap, d.nx, bbox, st);
    ElParams p = el_base(pl, mat, pz, px);
    p.dmat = dmat;
    p.fields = work + m.fields; p.psix = work + m.psi; p.psiz = work + m.psi + pl->psix_elems;
    const bool want_rec = drec_vx != nullptr && d.nrec > 0;
    el_two_launch_steps(pl, p, kBorn, inject ? df : nullptr, src_cell, src_w, bbox, rec_cell, rec_w,
                        want_rec ? drec_vx : nullptr, want_rec ? drec_vz : nullptr, const_cast<float *>(snap), snap_first,
                        n_begin, n_end, work + m.strain, st);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

int el_backward(mifwi_elastic_plan *pl, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo,
                int32_t flags, void *stream)
{
    if (!pl || !mat || !pz || !px || !work || !snap || !g_vx || !g_vz || !rec_cell || !rec_w)
        return mifwi::fail(MIFWI_EINVAL, "null argument");
    const mifwi_elastic_desc &d = pl->d;
    int rc = mifwi::check_adjoint_steps('n', 0, n_hi, n_lo, d.nt);
    if (!rc) rc = mifwi::check_snapshots(snap_first, n_lo);
    if (rc) return rc;
    if (grad_f && (!src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "grad_f requested but src_cell/src_w is null");
    if ((flags & MIFWI_FINALIZE) && !grad_mat)
        return mifwi::fail(MIFWI_EINVAL, "finalize requested but grad_mat is null");
    const ElWork m = work_map(pl, true);
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    float *fields = work + m.fields, *psiA = work + m.psi, *psiB = work + m.psiB, *acc = work + m.acc;
    ElParams p = el_base(pl, mat, pz, px);
    p.fields = fields;
    p.acc = acc;
    ElParams ps = p;
    ps.gs = pl->gs;
    ps.ninj = d.nrec; ps.ntap_inj = d.ntap; ps.inj_cell = rec_cell; ps.inj_w = rec_w;
    const bool want_f = grad_f != nullptr && d.nsrc > 0;
    ps.nsmp = want_f ? d.nsrc : 0; ps.ntap_smp = d.ntap; ps.smp_cell = src_cell; ps.smp_w = src_w;
    const long long snap_step = pl->snap_shot * d.nshot;
    // per-tile receiver lists of el_adj_s
    int *tile_start = nullptr, *tile_list = nullptr;
    const int tiles_x = mifwi::ceil_div(pl->ng, AGO), ntiles = tiles_x * mifwi::ceil_div(d.nz, ATZ);
    auto build_tile_lists = [&]() {
        int *base = reinterpret_cast<int *>(work + m.tile);
        tile_start = base;
        int *cursor = base + (long long)d.nshot * (ntiles + 1);
        tile_list = cursor + (long long)d.nshot * ntiles;
        hipLaunchKernelGGL(build_tile_taps, dim3(d.nshot), dim3(256), 0, st, rec_cell, d.nrec * d.ntap, d.nx, tiles_x,
                           ntiles, tile_start, cursor, tile_list);
    };
    const ElAdjKernels adj = el_adj_variant(pl->medium, pl->snap_bf16);
    bool per_step = true;
    if (pl->cl_adj && n_hi >= n_lo) {
        const mifwi::Handoff h = mifwi::cluster_handoff(pl, work, m);
        int *lists = reinterpret_cast<int *>(work + m.lists);
        launch_build_slab_lists(rec_cell, d.nshot, d.nrec, d.nz, d.nx, pl->adj_NW, 0, lists, st);
        EaParams c = cluster_base<EaParams>(pl, pl->adj_NW, pl->adj_PL, mat, pz, px, h);
        c.n_first = n_hi; c.n_last = n_lo; c.nt = d.nt;
        c.zrows_max = pl->adj_zrows;
        c.psix_elems = pl->psix_elems;
        c.fields = fields; c.psiA = psiA; c.psiB = psiB;
        c.S = snap; c.s_first = snap_first; c.s_step = snap_step;
        c.acc = acc;
        c.src_cell = src_cell; c.src_w = src_w;
        c.grad_f = want_f ? grad_f : nullptr;
        c.rec_cell = rec_cell; c.rec_w = rec_w; c.g_vx = g_vx; c.g_vz = g_vz;
        c.slab_cnt = lists; c.slab_list = lists + (long long)d.nshot * pl->adj_NW;
        c.rcv_direct = env_int("MIFWI_EL_ADJ_DIRECT", 1);
        const mifwi::TraceSpec ts = {"MIFWI_EL_CL_TRACE", 64 * 8 * 16, "# el_cluster_adj steps=%d", n_hi - n_lo + 1, 0};
        rc = mifwi::cluster_ladder("elastic adjoint", work, m.state, work + m.backup, flags, st, h, ts,
                                   [&](bool agent, long long *trace) {
            mifwi::set_trace(c, trace);
            el_cluster_launch(pl, el_cluster_adj_variant(pl->adj_ng, agent, pl->adj_xh), pl->adj_NW, pl->adj_shots, pl->adj_lds, c, st);
        });
        if (rc != MIFWI_OK && rc != mifwi::kClusterFellBack) return rc;
        per_step = rc == mifwi::kClusterFellBack;
    }
    // el_adj_s adds the adjoint sources of its tile (per-tile lists)
    if (per_step && d.nrec > 0 && n_hi >= n_lo) {
        build_tile_lists();
        ps.tile_start = tile_start; ps.tile_list = tile_list;
    }
    // shot groups are independent: a few at a time keep fields, accumulators and materials in the Infinity Cache
    for (int g0 = 0; per_step && g0 < pl->ngroups; g0 += pl->pass_groups)
    for (int n = n_hi; n >= n_lo; --n) {
        const int cg = std::min(pl->pass_groups, pl->ngroups - g0);
        const int cs = std::min(cg * ps.gs, d.nshot - g0 * ps.gs);
        p.s0 = ps.s0 = g0 * ps.gs;
        // ping-pong of the adjoint memory variables is absolute in n (resumable ranges)
        const int par = (d.nt - 1 - n) & 1;
        float *rd = par ? psiB : psiA, *wr = par ? psiA : psiB;
        ps.psix = rd; ps.psiz = rd + pl->psix_elems;
        ps.psix_out = wr; ps.psiz_out = wr + pl->psix_elems;
        ps.S = const_cast<float *>(snap) + (long long)(n - snap_first) * snap_step;
        ps.inj_amp0 = g_vx + (long long)n * d.nshot * d.nrec;
        ps.inj_amp1 = g_vz + (long long)n * d.nshot * d.nrec;
        const bool force = d.source_type != 0;        // grad_f of a point force: v_bar sampled between S^T and V^T
        ps.smp_out0 = (want_f && !force) ? grad_f + (long long)n * d.nshot * d.nsrc : nullptr;
        p.psix = ps.psix; p.psiz = ps.psiz; p.psix_out = ps.psix_out; p.psiz_out = ps.psiz_out;
        const int tx = mifwi::ceil_div(pl->ng, AGO), tz = mifwi::ceil_div(d.nz, ATZ);
        ps.tiles_z = tz;
        int ex = 0;
        if (want_f && !force) ex = mifwi::ceil_div(mifwi::ceil_div(ps.gs * ps.nsmp, kThreads), tx);
        if (pl->g_p && d.nrec > 0) {
            ElParams pq = ps;
            pq.gs = cs; pq.inj_amp0 = pl->g_p + (long long)n * d.nshot * d.nrec;
            hipLaunchKernelGGL(el_inject_pressure, dim3(mifwi::ceil_div(cs * d.nrec * d.ntap, 64)), dim3(64), 0,
                               st, pq);
        }
        if (pl->medium == kTti) {
            TtiParams q;
            static_cast<ElParams &>(q) = ps;
            q.E = work + m.strain; q.e_shot = 3 * pl->splane;
            hipLaunchKernelGGL(tti_adj_e, dim3(tx, tz, cg), dim3(kThreads), 0, st, q);
            hipLaunchKernelGGL(tti_adj_s, dim3(tx, tz + ex, cg), dim3(kThreads), 0, st, q);
        } else {
            hipLaunchKernelGGL(adj.s, dim3(tx, tz + ex, cg), dim3(kThreads), 0, st, ps);
        }
        if (want_f && force) {
            ElParams pq = ps;
            pq.gs = cs; pq.smp_out0 = grad_f + (long long)n * d.nshot * d.nsrc;
            hipLaunchKernelGGL(sample_force<ElParams>, dim3(mifwi::ceil_div(cs * d.nsrc, 64)), dim3(64), 0, st, pq,
                               d.source_type == 1 ? F_VX : F_VZ);
        }
        hipLaunchKernelGGL(adj.v, dim3(tx, tz, cs), dim3(kThreads), 0, st, p);
    }
    if (flags & MIFWI_FINALIZE) {
        const long long n5 = (long long)kMedia[pl->medium].nmat * pl->coef_elems;
        hipLaunchKernelGGL(adj.finalize, dim3((unsigned)((n5 + 255) / 256)), dim3(256), 0, st, acc,
                           pl->ngroups, d.nz, pl->gp, pl->splane, pl->cl_adj ? 0 : pl->sblk, grad_mat);
    }
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

// ---- the entry points of the three families (include/mifwi.h) -----------------------------------------------------------
// A handle of any family is a mifwi_elastic_plan (el_plan_create); plan_cast gives it back.
template <class Handle>
auto plan_cast(Handle *h)
{
    using Plan = std::conditional_t<std::is_const<Handle>::value, const mifwi_elastic_plan, mifwi_elastic_plan>;
    return reinterpret_cast<Plan *>(h);
}

// Refuses the plan of another medium: its kernels would take kMedia[].nmat planes where the caller allocated this
// family's.  (A null plan passes: the call itself refuses it.)
int check_medium(const mifwi_elastic_plan *pl, ElMedium medium)
{
    return (pl && pl->medium != medium) ? mifwi::fail(MIFWI_EINVAL, "the plan was not created by %s", kMedia[medium].created_by)
                                        : MIFWI_OK;
}

// mifwi_vti_desc / mifwi_visco_desc -> the elastic descriptor: velocity receivers, f32 snapshot planes
template <class Desc>
mifwi_elastic_desc elastic_desc(const Desc &d)
{
    mifwi_elastic_desc e;
    e.nz = d.nz; e.nx = d.nx; e.nt = d.nt; e.nshot = d.nshot; e.nsrc = d.nsrc; e.nrec = d.nrec; e.ntap = d.ntap;
    e.pml_width = d.pml_width; e.free_surface = d.free_surface; e.shots_per_group = d.shots_per_group;
    e.source_type = d.source_type; e.record_pressure = 0; e.snapshot_format = MIFWI_SNAPSHOT_F32; e.fd_order = d.fd_order;
    return e;
}

// mifwi_vti_layout / mifwi_visco_layout: the nine fields they share with the elastic layout
template <class Layout>
int family_layout(const mifwi_elastic_plan *pl, Layout *out)
{
    if (!pl || !out) return mifwi::fail(MIFWI_EINVAL, "null plan/layout");
    mifwi_elastic_layout e;
    const int rc = mifwi_elastic_plan_layout(pl, &e);
    if (rc) return rc;
    out->gp = e.gp; out->pitch = e.pitch; out->ngroups = e.ngroups; out->shots_per_group = e.shots_per_group;
    out->coef_elems = e.coef_elems; out->state_elems = e.state_elems; out->work_forward_elems = e.work_forward_elems;
    out->work_backward_elems = e.work_backward_elems; out->snap_step_elems = e.snap_step_elems;
    return MIFWI_OK;
}

}  // namespace

extern "C" {

// isotropic
int mifwi_elastic_forward(mifwi_elastic_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                          const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                          float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                          int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan, kIsotropic)) return rc;
    return el_forward(plan, mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, snap, work, n_begin,
                      n_end, flags, stream);
}

int mifwi_elastic_backward(mifwi_elastic_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                           const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                           const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                           int32_t n_lo, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan, kIsotropic)) return rc;
    return el_backward(plan, mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, snap, snap_first, grad_mat,
                       grad_f, work, n_hi, n_lo, flags, stream);
}

int mifwi_elastic_born(mifwi_elastic_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                       const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                       const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                       int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan, kIsotropic)) return rc;
    return el_born(plan, mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx, drec_vz,
                   work, n_begin, n_end, flags, stream);
}

// VTI: six planes, one launch per half step
int mifwi_vti_plan_create(mifwi_vti_plan **plan, int device, const mifwi_vti_desc *d)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    const mifwi_elastic_desc e = elastic_desc(*d);
    return el_plan_create(reinterpret_cast<mifwi_elastic_plan **>(plan), device, &e, kVti);
}

int mifwi_vti_plan_destroy(mifwi_vti_plan *plan) { return mifwi_elastic_plan_destroy(plan_cast(plan)); }

int mifwi_vti_plan_layout(const mifwi_vti_plan *plan, mifwi_vti_layout *out) { return family_layout(plan_cast(plan), out); }

int mifwi_vti_plan_pass_sizes(const mifwi_vti_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    return mifwi_elastic_plan_pass_sizes(plan_cast(plan), forward_shots, adjoint_groups);
}

int mifwi_vti_plan_cluster_slabs(const mifwi_vti_plan *, int32_t) { return 0; }

int mifwi_vti_forward(mifwi_vti_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                      const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                      float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                      int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVti)) return rc;
    return el_forward(plan_cast(plan), mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, snap, work, n_begin,
                      n_end, flags, stream);
}

int mifwi_vti_backward(mifwi_vti_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                       const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                       const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                       int32_t n_lo, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVti)) return rc;
    return el_backward(plan_cast(plan), mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, snap, snap_first, grad_mat,
                       grad_f, work, n_hi, n_lo, flags, stream);
}

int mifwi_vti_born(mifwi_vti_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                   const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                   const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                   int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVti)) return rc;
    return el_born(plan_cast(plan), mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx, drec_vz,
                   work, n_begin, n_end, flags, stream);
}

// TTI: eight planes; the stress half step and its transpose are two launches each (mifwi_tti.h)
int mifwi_tti_plan_create(mifwi_tti_plan **plan, int device, const mifwi_tti_desc *d)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    const mifwi_elastic_desc e = elastic_desc(*d);
    return el_plan_create(reinterpret_cast<mifwi_elastic_plan **>(plan), device, &e, kTti);
}

int mifwi_tti_plan_destroy(mifwi_tti_plan *plan) { return mifwi_elastic_plan_destroy(plan_cast(plan)); }

int mifwi_tti_plan_layout(const mifwi_tti_plan *plan, mifwi_tti_layout *out) { return family_layout(plan_cast(plan), out); }

int mifwi_tti_plan_pass_sizes(const mifwi_tti_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    return mifwi_elastic_plan_pass_sizes(plan_cast(plan), forward_shots, adjoint_groups);
}

int mifwi_tti_plan_cluster_slabs(const mifwi_tti_plan *, int32_t) { return 0; }

int mifwi_tti_forward(mifwi_tti_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                      const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                      float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                      int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kTti)) return rc;
    return el_forward(plan_cast(plan), mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, snap, work, n_begin,
                      n_end, flags, stream);
}

int mifwi_tti_backward(mifwi_tti_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                       const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                       const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                       int32_t n_lo, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kTti)) return rc;
    return el_backward(plan_cast(plan), mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, snap, snap_first, grad_mat,
                       grad_f, work, n_hi, n_lo, flags, stream);
}

int mifwi_tti_born(mifwi_tti_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                   const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                   const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                   int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kTti)) return rc;
    return el_born(plan_cast(plan), mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx, drec_vz,
                   work, n_begin, n_end, flags, stream);
}

// viscoelastic: eight planes and eight fields per shot, one launch per half step
int mifwi_visco_plan_create(mifwi_visco_plan **plan, int device, const mifwi_visco_desc *d)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    // a = (2 - eta) / (2 + eta), b = 2 eta / (2 + eta) with 0 < eta < 2: 0 < a < 1 and b = 1 - a
    if (!(d->relax_a > 0.f && d->relax_a < 1.f && d->relax_b > 0.f && d->relax_b < 1.f))
        return mifwi::fail(MIFWI_EINVAL, "relax_a = %g, relax_b = %g: both must lie inside (0, 1)", (double)d->relax_a,
                           (double)d->relax_b);
    const mifwi_elastic_desc e = elastic_desc(*d);
    return el_plan_create(reinterpret_cast<mifwi_elastic_plan **>(plan), device, &e, kVisco, d->relax_a, d->relax_b);
}

int mifwi_visco_plan_destroy(mifwi_visco_plan *plan) { return mifwi_elastic_plan_destroy(plan_cast(plan)); }

int mifwi_visco_plan_layout(const mifwi_visco_plan *plan, mifwi_visco_layout *out) { return family_layout(plan_cast(plan), out); }

int mifwi_visco_plan_pass_sizes(const mifwi_visco_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    return mifwi_elastic_plan_pass_sizes(plan_cast(plan), forward_shots, adjoint_groups);
}

int mifwi_visco_plan_cluster_slabs(const mifwi_visco_plan *, int32_t) { return 0; }

int mifwi_visco_forward(mifwi_visco_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                        const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                        float *rec_vx, float *rec_vz, float *snap, float *work, int32_t n_begin, int32_t n_end,
                        int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVisco)) return rc;
    return el_forward(plan_cast(plan), mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, snap, work, n_begin,
                      n_end, flags, stream);
}

int mifwi_visco_backward(mifwi_visco_plan *plan, const float *mat, const float *pz, const float *px, const int32_t *src_cell,
                         const float *src_w, const int32_t *rec_cell, const float *rec_w, const float *g_vx, const float *g_vz,
                         const float *snap, int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi,
                         int32_t n_lo, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVisco)) return rc;
    return el_backward(plan_cast(plan), mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, snap, snap_first, grad_mat,
                       grad_f, work, n_hi, n_lo, flags, stream);
}

int mifwi_visco_born(mifwi_visco_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                     const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                     const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz, float *work, int32_t n_begin,
                     int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan_cast(plan), kVisco)) return rc;
    return el_born(plan_cast(plan), mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx, drec_vz,
                   work, n_begin, n_end, flags, stream);
}

}  // extern "C"

// snapshot second moments (pseudo-Hessian ingredient): reads the snapshot buffer the way the adjoint does
#include "mifwi_elastic_moments.h"
