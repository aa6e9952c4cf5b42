// 2-D variable-density ACOUSTIC (fluid) velocity-pressure propagator for gfx950 (MI355X): forward, snapshot save and the
// exact discrete adjoint with material-gradient accumulation.  The P-SV scheme of mifwi_elastic.hip with Vs = 0, where
// sxx = szz = p and sxz = 0: three fields instead of five, four C-PML memory variables instead of eight, three snapshot
// and gradient planes instead of five (36 instead of 60 B per cell-step forward, 48 instead of 80 in the adjoint).
//
// Replaces (reference tree): the DENISE runs with PHYSICS = 2 behind pyapi_denise, models/networks.py:10445-10453.
//
// Same grid, staggering, Dp / Dm, pml / pmlT and pz / px tables as the elastic kernels - one copy of them, of the strip
// and tile helpers, of the three cold kernels and of the plan geometry, in mifwi_stagger.h; the seismograms are those of the
// elastic scheme on mat = [K, K, 0, bx, bz] bit for bit (with Ms == Ls its two stress updates are one fmaf chain).
// Forward: two launches per time step.  V: vx, vz from p, with the point force (source_type 1 / 2) added by the tile
// that owns the cells; P: p from the new velocities, with the explosive source, and the velocity receivers sampled by
// extra workgroups.  A thread owns 4 consecutive cells of one row (16-B lane accesses), the z window of its column in
// registers, x neighbours from 8-B halo loads.  C-PML memory variables live in compact strips (x strips: d1 @half,
// e1 @int; z strips: d4 @half, e2 @int).
// Adjoint: two launches per step (P^T then V^T).  The transposed C-PML acts on the material-scaled adjoint field before
// the spatial derivative, so each workgroup evaluates it on its tile + halo into LDS and applies the stencils from there.
// All three gradient accumulators are updated in the P^T launch and stay in registers across the shots of a group; the
// finalize adds the groups in a fixed order (no atomics in the gradient).
// Tiles are taken in an XCD-contiguous order, the drivers sweep the time range a few shots (shot groups) at a time when
// all of them would not stay inside the Infinity Cache.  Snapshots: f32, three planes per shot-step, blocked by columns
// of 16 groups (whole 128-byte lines per tile row).  There is no single-launch form.
// Born (mifwi_fluid_born): the same two launches on the perturbed state; instead of writing the step's three snapshot
// planes they read the background run's and add dmat times them (SAVE = kBorn), the JVP partner of the adjoint's gradients.
// Viscoacoustic medium (mifwi_viscofluid_*): the same plan with a fourth field r (the memory variable of one standard linear
// solid, on the p node), a fourth plane R and a fourth accumulator - compile-time variants Q = true of fl_step_p, fl_adj_p and
// fl_adj_v; the V launch and every point kernel are shared.  R = 0 gives the lossless bits, and on the planes of a model the
// P launch is el_step_s<..., VISCO> with Vs = 0, operand for operand (include/mifwi.h has the recursion and its transpose).
// Snapshot moments (the pseudo-Hessian's ingredient): mifwi_fluid_moments.h, included at the end.
// Arithmetic = the explicit fmaf chain stated in include/mifwi.h (build with -ffp-contract=off).
#include "mifwi_cluster_host.h"      // mifwi::env_int
#include "mifwi_stagger.h"

namespace {

enum { F_VX = 0, F_VZ = 1, F_P = 2, F_R = 3 };       // F_R: the memory variable of a viscoacoustic plan (Q kernels only)
enum { M_K = 0, M_BX = 1, M_BZ = 2, M_R = 3 };       // M_R: its fourth plane, R dt/h
enum { PSI_HALF = 0, PSI_INT = 1 };      // plane of a strip: the V launch's derivative (d1 / d4), the P launch's (e1 / e2)

struct FlParams {
    int nz, nx, ng, gp, pitch;
    unsigned field_stride;       // (nz+4)*pitch
    long long shot_stride;       // 3*field_stride (viscoacoustic: 4)
    int nshot, gs;               // gs: shots per accumulator group (P^T launch), shots of the pass (point launches)
    int s0;                      // first shot of this pass over the time range (blockIdx.z counts from it)
    int W, wl, xr0, wx;          // C-PML strip geometry; W = 0 disables the layer
    int fsurf;
    long long psix_shot, psiz_shot;   // floats per shot: 2*nz*wx, 2*2W*gp
    const float *mat, *pz, *px;
    const float *dmat;           // Born step (SAVE kBorn): perturbation of the three material planes, [3][nz][gp] like mat
    float *fields;
    float *psix, *psiz;          // forward: updated in place; adjoint: read side
    float *psix_out, *psiz_out;  // adjoint: write side (ping-pong)
    float *S;                    // snapshot slice of this step: [nshot][3] planes of splane floats (Born: read)
    unsigned splane;             // floats per snapshot / accumulator plane: nz * 64 * ceil(ng / 16)
    float *acc;                  // [ngroups][3] planes (viscoacoustic: 4)
    // injection (V: vx | vz += a; P: p += a; P^T: vx += a0, vz += a1)
    int ninj, ntap_inj, inj_field;
    const int *inj_cell;
    const float *inj_w;
    const float *inj_amp0, *inj_amp1;
    const int *inj_bbox;
    const int *tile_start, *tile_list;   // fl_adj_p: receiver taps of each (shot, tile)
    // sampling (P: vx, vz; P^T: p)
    int nsmp, ntap_smp;
    const int *smp_cell;
    const float *smp_w;
    float *smp_out0, *smp_out1;
    int tiles_z;
    FdK fd;
    float rel_a, rel_b;          // Q kernels: r <- a r - b q
};

// offset (floats) of group g of row j inside a snapshot / accumulator plane: always column-blocked
__device__ __forceinline__ unsigned snap_cell(const FlParams &p, int j, int g) { return snap_cell_blocked(p.nz, j, g); }
// memory variables of one group: plane k of the shot's x strips (row j) / z strips (strip row zs)
__device__ __forceinline__ long long psix_at(const FlParams &p, int s, int k, int j, int xs_off)
{
    return (long long)s * p.psix_shot + ((long long)k * p.nz + j) * p.wx + xs_off;
}
__device__ __forceinline__ long long psiz_at(const FlParams &p, int s, int k, int zs, int g)
{
    return (long long)s * p.psiz_shot + ((long long)k * 2 * p.W + zs) * p.gp + 4 * g;
}

// sampling workgroups (the rows by >= tiles_z of a launch), p.gs shots per z slice.
// MODE 0: out0 = sum w vx, out1 = sum w vz ; MODE 1: out0 = sum w p (adjoint of the explosive source)
template <int MODE>
__device__ void sample_points(const FlParams &p, int bx, int by, int bz, int gs)
{
    const int nrb = (int)(gridDim.y - p.tiles_z) * (int)gridDim.x;
    const int rb = (by - p.tiles_z) * (int)gridDim.x + bx;
    const int total = gs * p.nsmp;
    for (int e = rb * (int)blockDim.x + (int)threadIdx.x; e < total; e += nrb * (int)blockDim.x) {
        const int si = e / p.nsmp, ip = e - si * p.nsmp;
        const int s = p.s0 + bz * gs + si;
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
                a0 = fmaf(w, (p.fsurf && j == 0) ? 0.f : fl[F_P * p.field_stride + off], a0);
            }
        }
        p.smp_out0[(long long)s * p.nsmp + ip] = a0;
        if (MODE == 0) p.smp_out1[(long long)s * p.nsmp + ip] = a1;
    }
}

// LDS image of the shot's injection amplitudes that fall into this tile (block-uniform decision; every thread calls it)
template <int TZ, int TX>
__device__ bool stage_injection(const FlParams &p, int s, int tile_j, int tile_i, float *inj)
{
    if (p.ninj <= 0) return false;
    const int b0 = p.inj_bbox[4 * s + 0], b1 = p.inj_bbox[4 * s + 1];
    const int b2 = p.inj_bbox[4 * s + 2], b3 = p.inj_bbox[4 * s + 3];
    const bool has = (b0 < tile_j + TZ) && (b1 >= tile_j) && (b2 < tile_i + TX) && (b3 >= tile_i);
    if (!has) return false;
    for (int e = (int)threadIdx.x; e < TZ * TX; e += kThreads) inj[e] = 0.f;
    __syncthreads();
    const int total = p.ninj * p.ntap_inj;
    for (int e = (int)threadIdx.x; e < total; e += kThreads) {
        const long long ee = (long long)s * total + e;
        const int cell = p.inj_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        const int tj = j - tile_j, ti = i - tile_i;
        if (tj >= 0 && tj < TZ && ti >= 0 && ti < TX)
            atomicAdd(&inj[tj * TX + ti], p.inj_w[ee] * p.inj_amp0[(long long)s * p.ninj + e / p.ntap_inj]);
    }
    __syncthreads();
    return true;
}

struct PxTab { float4 a, b, k; };
__device__ __forceinline__ PxTab px_tab(const FlParams &p, int g, int half)
{
    const float *t = p.px + (half ? PAH : PA) * p.gp + 4 * g;
    return PxTab{ld4(t), ld4(t + p.gp), ld4(t + 2 * p.gp)};
}

// SAVE 0: no snapshots, 1: write the three planes, 2 (kBorn): the Born step - the state is the perturbed one, the planes of
// the background run are read and dmat times them is added
constexpr int kBorn = 2;

// ================================================================================================
// forward V launch:  vx += bx (Dp_x p)',  vz += bz (Dp_z p)',  then the point force of the tile
// ================================================================================================
template <int LX, int SAVE>
__global__ __launch_bounds__(kThreads) void fl_step_v(const FlParams p)
{
    const FdK K = p.fd;
    constexpr int LZ = kThreads / LX, TX = LX * 4;
    __shared__ float inj[LZ * TX];
    int bx, by, bz;
    xcd_tile_major(bx, by, bz);
    const int lx = (int)threadIdx.x % LX, lz = (int)threadIdx.x / LX;
    const int g = bx * LX + lx, j = by * LZ + lz;
    const int s = p.s0 + bz;
    const bool has_inj = stage_injection<LZ, TX>(p, s, by * LZ, bx * TX, inj);
    if (g >= p.ng || j >= p.nz) return;
    const unsigned fs = p.field_stride;
    float *fl = p.fields + (long long)s * p.shot_stride;
    const float *pp = fl + F_P * fs;
    float *vx = fl + F_VX * fs, *vz = fl + F_VZ * fs;
    const unsigned o = (unsigned)(j + 2) * p.pitch + 4 + 4 * g;
    const unsigned cc = (unsigned)j * p.gp + 4 * g;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const int xs_off = xstrip(p, g), zs = zstrip(p, j);
    // every global request up front: memory variables of the strips together with the fields
    float *q1 = nullptr, *q4 = nullptr;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 s1 = zero4, s4 = zero4;
    PxTab xt{zero4, zero4, zero4};
    float zah = 0.f, zbh = 0.f, zkh = 1.f;
    if (xs_off >= 0) {
        q1 = p.psix + psix_at(p, s, PSI_HALF, j, xs_off);
        s1 = ld4(q1);
        xt = px_tab(p, g, 1);
    }
    if (zs >= 0) {
        q4 = p.psiz + psiz_at(p, s, PSI_HALF, zs, g);
        s4 = ld4(q4);
        zah = p.pz[PAH * p.nz + j]; zbh = p.pz[PBH * p.nz + j]; zkh = p.pz[PKH * p.nz + j];
    }
    // z window of p: rows j-1 .. j+2
    float4 b0 = ld4(pp + o - p.pitch);
    const float4 b1 = ld4(pp + o), b2 = ld4(pp + o + p.pitch), b3 = ld4(pp + o + 2 * p.pitch);
    const float2 Lp = ld2(pp + o - 2), Rp = ld2(pp + o + 4);
    float4 vxv = ld4(vx + o), vzv = ld4(vz + o);
    const float4 bxs = ld4(p.mat + M_BX * ncell + cc), bzs = ld4(p.mat + M_BZ * ncell + cc);
    float4 B1 = zero4, B2 = zero4, dbx = zero4, dbz = zero4;
    if (SAVE == kBorn) {
        const float *Sp = p.S + 3LL * s * p.splane + snap_cell(p, j, g);
        B1 = mifwi::ldnt4(Sp + (long long)p.splane); B2 = mifwi::ldnt4(Sp + 2 * (long long)p.splane);
        dbx = ld4(p.dmat + M_BX * ncell + cc); dbz = ld4(p.dmat + M_BZ * ncell + cc);
    }
    if (p.fsurf && j == 0) b0 = make_float4(-b2.x, -b2.y, -b2.z, -b2.w);      // p(-1) = -p(1)
    const float xx[8] = {Lp.x, Lp.y, b1.x, b1.y, b1.z, b1.w, Rp.x, Rp.y};
    float d1[4], d4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        d1[c] = dfw(K, xx[c + 1], xx[c + 2], xx[c + 3], xx[c + 4]);
        d4[c] = dfw(K, comp(b0, c), comp(b1, c), comp(b2, c), comp(b3, c));
    }
    if (xs_off >= 0) {
        float t1[4] = {s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) d1[c] = pml(t1[c], comp(xt.a, c), comp(xt.b, c), comp(xt.k, c), d1[c]);
        st4(q1, mk4(t1));
    }
    if (zs >= 0) {
        float t4[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) d4[c] = pml(t4[c], zah, zbh, zkh, d4[c]);
        st4(q4, mk4(t4));
    }
    float nvx[4], nvz[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        nvx[c] = fmaf(comp(bxs, c), d1[c], comp(vxv, c));
        nvz[c] = fmaf(comp(bzs, c), d4[c], comp(vzv, c));
        if (SAVE == kBorn) {
            nvx[c] = fmaf(comp(dbx, c), comp(B1, c), nvx[c]);
            nvz[c] = fmaf(comp(dbz, c), comp(B2, c), nvz[c]);
        }
        if (has_inj) {
            const float a = inj[lz * TX + 4 * lx + c];
            if (p.inj_field == F_VX) nvx[c] += a; else nvz[c] += a;
        }
    }
    st4(vx + o, mk4(nvx));
    st4(vz + o, mk4(nvz));
    if (SAVE == 1) {
        float *Sp = p.S + 3LL * s * p.splane + snap_cell(p, j, g);
        mifwi::stnt4(Sp + (long long)p.splane, mk4(d1));
        mifwi::stnt4(Sp + 2 * (long long)p.splane, mk4(d4));
    }
}

// ================================================================================================
// forward P launch:  p += K (Dm_x vx)' + K (Dm_z vz)',  the explosive source of the tile;  extra workgroups sample vx, vz
// ================================================================================================
// Q (viscoacoustic): q = R (e1' + e2'), p += (1 + a)/2 r - b/2 q after the chain, r = a r - b q - the operand order of
// el_step_s<..., VISCO> with R1 == R2, so that the P-SV route with Vs = 0 gives the same bits; R = 0 leaves r at 0 and p
// the lossless chain's.  Born: q += dmat[3] S0.
template <int LX, int SAVE, bool Q>
__global__ __launch_bounds__(kThreads) void fl_step_p(const FlParams p)
{
    const FdK K = p.fd;
    constexpr int LZ = kThreads / LX, TX = LX * 4;
    __shared__ float inj[LZ * TX];
    int bx, by, bz;
    xcd_tile_major(bx, by, bz);
    if (by >= p.tiles_z) {
        sample_points<0>(p, bx, by, bz, 1);
        return;
    }
    const int lx = (int)threadIdx.x % LX, lz = (int)threadIdx.x / LX;
    const int g = bx * LX + lx, j = by * LZ + lz;
    const int s = p.s0 + bz;
    const bool has_inj = stage_injection<LZ, TX>(p, s, by * LZ, bx * TX, inj);
    if (g >= p.ng || j >= p.nz) return;
    const unsigned fs = p.field_stride;
    float *fl = p.fields + (long long)s * p.shot_stride;
    const float *vx = fl + F_VX * fs, *vz = fl + F_VZ * fs;
    float *pp = fl + F_P * fs;
    const unsigned o = (unsigned)(j + 2) * p.pitch + 4 + 4 * g;
    const unsigned cc = (unsigned)j * p.gp + 4 * g;
    const int xs_off = xstrip(p, g), zs = zstrip(p, j);
    float *q1 = nullptr, *q2 = nullptr;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 s1 = zero4, s2 = zero4;
    PxTab xt{zero4, zero4, zero4};
    float za = 0.f, zb = 0.f, zk = 1.f;
    if (xs_off >= 0) {
        q1 = p.psix + psix_at(p, s, PSI_INT, j, xs_off);
        s1 = ld4(q1);
        xt = px_tab(p, g, 0);
    }
    if (zs >= 0) {
        q2 = p.psiz + psiz_at(p, s, PSI_INT, zs, g);
        s2 = ld4(q2);
        za = p.pz[PA * p.nz + j]; zb = p.pz[PB * p.nz + j]; zk = p.pz[PK * p.nz + j];
    }
    // z window of vz: rows j-2 .. j+1 (the rows above the grid stay zero: no velocities above a free surface)
    const float4 a0 = ld4(vz + o - 2 * p.pitch), a1 = ld4(vz + o - p.pitch), a2 = ld4(vz + o), a3 = ld4(vz + o + p.pitch);
    const float4 cvx = ld4(vx + o);
    const float2 Lvx = ld2(vx + o - 2), Rvx = ld2(vx + o + 4);
    const float4 pv = ld4(pp + o);
    const float4 Ks = ld4(p.mat + cc);
    float4 B0 = zero4, dK = zero4;
    if (SAVE == kBorn) {
        B0 = mifwi::ldnt4(p.S + 3LL * s * p.splane + snap_cell(p, j, g));
        dK = ld4(p.dmat + cc);
    }
    float4 Rs = zero4, rv = zero4, dR = zero4;
    if (Q) {
        const unsigned ncell = (unsigned)p.nz * p.gp;
        Rs = ld4(p.mat + M_R * ncell + cc);
        rv = ld4(fl + F_R * fs + o);
        if (SAVE == kBorn) dR = ld4(p.dmat + M_R * ncell + cc);
    }
    const float xv[8] = {Lvx.x, Lvx.y, cvx.x, cvx.y, cvx.z, cvx.w, Rvx.x, Rvx.y};
    float e1[4], e2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        e1[c] = dbw(K, xv[c], xv[c + 1], xv[c + 2], xv[c + 3]);
        e2[c] = dbw(K, comp(a0, c), comp(a1, c), comp(a2, c), comp(a3, c));
    }
    if (xs_off >= 0) {
        float t1[4] = {s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) e1[c] = pml(t1[c], comp(xt.a, c), comp(xt.b, c), comp(xt.k, c), e1[c]);
        st4(q1, mk4(t1));
    }
    if (zs >= 0) {
        float t2[4] = {s2.x, s2.y, s2.z, s2.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) e2[c] = pml(t2[c], za, zb, zk, e2[c]);
        st4(q2, mk4(t2));
    }
    float np[4], s0v[4], nr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s0v[c] = e1[c] + e2[c];
        np[c] = fmaf(comp(Ks, c), e1[c], fmaf(comp(Ks, c), e2[c], comp(pv, c)));
        if (SAVE == kBorn) np[c] = fmaf(comp(dK, c), comp(B0, c), np[c]);
        if (Q) {
            const float ha = 0.5f * (1.f + p.rel_a), hb = 0.5f * p.rel_b;
            float q = fmaf(comp(Rs, c), e1[c], comp(Rs, c) * e2[c]);
            if (SAVE == kBorn) q = fmaf(comp(dR, c), comp(B0, c), q);
            np[c] += fmaf(ha, comp(rv, c), -(hb * q));
            nr[c] = fmaf(p.rel_a, comp(rv, c), -(p.rel_b * q));
        }
        if (has_inj) np[c] += inj[lz * TX + 4 * lx + c];
        if (p.fsurf && j == 0) np[c] = 0.f;
    }
    st4(pp + o, mk4(np));
    if (Q) st4(fl + F_R * fs + o, mk4(nr));
    if (SAVE == 1) mifwi::stnt4(p.S + 3LL * s * p.splane + snap_cell(p, j, g), mk4(s0v));
}

// ================================================================================================
// adjoint launches, on the tile of mifwi_stagger.h (ATZ x 4*AGO owned cells, staged on ASZ x ASX in LDS)
// ================================================================================================

// Staged coordinates of the halo group a thread stages besides its own group (threads 0..kHalo-1): the two rows above
// and below the tile (owned columns only: they serve the z stencil), then the left / right halo group of every owned
// row (they serve the x stencil).  The four corners of the staged image are never read.
constexpr int kHaloRows = 4 * AGO, kHalo = kHaloRows + 2 * ATZ;
__device__ __forceinline__ void halo_item(int h, int &sr, int &sg)
{
    if (h < kHaloRows) {
        const int q = h / AGO;
        sr = q < 2 ? q : ATZ + q;
        sg = 1 + (h - q * AGO);
    } else {
        const int k = h - kHaloRows;
        sr = 2 + (k >> 1);
        sg = (k & 1) * (AGX - 1);
    }
}

// The two transposed C-PML outputs of one group's material-scaled adjoint value `v`: X through the x tables, Z through the
// z tables (plane k of the strips, tables at half nodes when `half`); the memory variables are written by the owner.
// want_x / want_z: a halo group serves one stencil only.
__device__ __forceinline__ void stage_T(const FlParams &p, int s, int k, int half, int j, int g, const float4 &v, bool mine,
                                        bool want_x, bool want_z, float4 &X, float4 &Z)
{
    float x[4] = {v.x, v.y, v.z, v.w}, z[4] = {v.x, v.y, v.z, v.w};
    const int xs_off = want_x ? xstrip(p, g) : -1;
    if (xs_off >= 0) {
        const PxTab xt = px_tab(p, g, half);
        const long long q = psix_at(p, s, k, j, xs_off);
        const float4 sv = ld4(p.psix + q);
        float n[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = pmlT(comp(sv, c), comp(xt.a, c), comp(xt.b, c), comp(xt.k, c), x[c], n[c]);
        if (mine) st4(p.psix_out + q, mk4(n));
    }
    const int zs = want_z ? zstrip(p, j) : -1;
    if (zs >= 0) {
        const int r = half ? PAH : PA;
        const float za = p.pz[r * p.nz + j], zb = p.pz[(r + 1) * p.nz + j], zk = p.pz[(r + 2) * p.nz + j];
        const long long q = psiz_at(p, s, k, zs, g);
        const float4 sv = ld4(p.psiz + q);
        float n[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c] = pmlT(comp(sv, c), za, zb, zk, z[c], n[c]);
        if (mine) st4(p.psiz_out + q, mk4(n));
    }
    X = mk4(x); Z = mk4(z);
}

__device__ __forceinline__ float4 mul4(const float4 &a, const float4 &b)
{
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
// Q kernels: w = -b (r_bar + p_bar / 2), the adjoint of q;  K p_bar + R w, what goes through pmlT
__device__ __forceinline__ float4 adj_w4(float b, const float4 &rb, const float4 &pb)
{
    return make_float4(-b * fmaf(0.5f, pb.x, rb.x), -b * fmaf(0.5f, pb.y, rb.y), -b * fmaf(0.5f, pb.z, rb.z),
                       -b * fmaf(0.5f, pb.w, rb.w));
}
__device__ __forceinline__ float4 kp_rw4(const float4 &K, const float4 &pb, const float4 &R, const float4 &w)
{
    return make_float4(fmaf(K.x, pb.x, R.x * w.x), fmaf(K.y, pb.y, R.y * w.y), fmaf(K.z, pb.z, R.z * w.z),
                       fmaf(K.w, pb.w, R.w * w.w));
}

// P^T:  acc_K += S0 p_bar;  E1, E2 = pmlT(K p_bar);  vx_bar -= Dp_x E1,  vz_bar -= Dp_z E2;  acc_bx += S1 vx_bar,
//       acc_bz += S2 vz_bar.  The adjoint sources of the tile's cells (v_bar += R^T g, the head of an adjoint step) are
//       added to the loaded v_bar first (p.tile_start set).  Extra workgroups sample p_bar at the explosive sources.
// Q (viscoacoustic): w = -b (r_bar + p_bar / 2) on tile and halo from the OLD r_bar (field 3);  acc_R += S0 w;
//       E1, E2 = pmlT(K p_bar + R w).  r_bar is only read here: neighbouring tiles stage the same cells in no order, so the
//       owner advances it in fl_adj_v.
template <bool Q>
__global__ __launch_bounds__(kThreads) void fl_adj_p(const FlParams p)
{
    constexpr int NP = Q ? 4 : 3;
    const FdK K = p.fd;
    int bx, by, bz;
    xcd_tile_major(bx, by, bz);
    if (by >= p.tiles_z) {
        sample_points<1>(p, bx, by, bz, p.gs);
        return;
    }
    __shared__ float E[2][ASZ][ASX];
    const int tile_j = by * ATZ, tile_g = bx * AGO;
    const unsigned fs = p.field_stride;
    const int t = (int)threadIdx.x;
    const int orow = t / AGO, ogrp = t % AGO;
    const int oj = tile_j + orow, og = tile_g + ogrp;
    const bool own_ok = oj < p.nz && og < p.ng;
    const unsigned occ = (unsigned)oj * p.gp + 4 * og;
    const unsigned oo = (unsigned)(oj + 2) * p.pitch + 4 + 4 * og;
    const unsigned osc = snap_cell(p, oj, og);
    int hr = 0, hg = 0;
    if (t < kHalo) halo_item(t, hr, hg);
    const int hj = tile_j - 2 + hr, hgg = tile_g - 1 + hg;
    const bool halo_ok = t < kHalo && hj >= 0 && hj < p.nz && hgg >= 0 && hgg < p.ng;
    const bool halo_row = t < kHaloRows;
    const unsigned hcc = (unsigned)hj * p.gp + 4 * hgg;
    const unsigned ho = (unsigned)(hj + 2) * p.pitch + 4 + 4 * hgg;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[NP];
    float4 oK = zero4, hK = zero4, oR = zero4, hR = zero4;
    float *accp = p.acc + (long long)NP * (p.s0 / p.gs + bz) * p.splane + osc;
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = zero4;
    if (own_ok) {
#pragma unroll
        for (int k = 0; k < NP; ++k) acc[k] = ld4(accp + (long long)k * p.splane);
        oK = ld4(p.mat + occ);
        if (Q) oR = ld4(p.mat + M_R * (unsigned)p.nz * p.gp + occ);
    }
    if (halo_ok) {
        hK = ld4(p.mat + hcc);
        if (Q) hR = ld4(p.mat + M_R * (unsigned)p.nz * p.gp + hcc);
    }
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        float *fl = p.fields + (long long)s * p.shot_stride;
        float4 pb = zero4, hpb = zero4, vxb = zero4, vzb = zero4, S0 = zero4, S1 = zero4, S2 = zero4;
        float4 ow = zero4, hw = zero4;                   // Q: r_bar as loaded, then w
        if (own_ok) { pb = ld4(fl + F_P * fs + oo); vxb = ld4(fl + F_VX * fs + oo); vzb = ld4(fl + F_VZ * fs + oo); }
        if (halo_ok) hpb = ld4(fl + F_P * fs + ho);
        if (Q) {
            if (own_ok) ow = ld4(fl + F_R * fs + oo);
            if (halo_ok) hw = ld4(fl + F_R * fs + ho);
        }
        // ---- adjoint sources of this tile (workgroup-uniform branch; E is free until the staging) -----------------
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
                    if (p.inj_amp0) atomicAdd(&E[0][j - tile_j + 2][i - 4 * tile_g + 4], w * p.inj_amp0[ai]);
                    if (p.inj_amp1) atomicAdd(&E[1][j - tile_j + 2][i - 4 * tile_g + 4], w * p.inj_amp1[ai]);
                }
                __syncthreads();
                const float4 ix = ld4(&E[0][orow + 2][x]), iz = ld4(&E[1][orow + 2][x]);
                vxb = make_float4(vxb.x + ix.x, vxb.y + ix.y, vxb.z + ix.z, vxb.w + ix.w);
                vzb = make_float4(vzb.x + iz.x, vzb.y + iz.y, vzb.z + iz.z, vzb.w + iz.w);
                __syncthreads();
            }
        }
        // ---- stage E1, E2 on the tile + halo ------------------------------------------------------------------
        if (p.fsurf && oj == 0) pb = zero4;              // p(0,.) is identically 0 in the forward run: adjoint discarded
        if (p.fsurf && hj == 0) hpb = zero4;
        if (Q) { ow = adj_w4(p.rel_b, ow, pb); hw = adj_w4(p.rel_b, hw, hpb); }
        {
            float4 E1 = zero4, E2 = zero4;
            if (own_ok) stage_T(p, s, PSI_INT, 0, oj, og, Q ? kp_rw4(oK, pb, oR, ow) : mul4(oK, pb), true, true, true, E1, E2);
            const int x = 4 * (ogrp + 1);
            st4(&E[0][orow + 2][x], E1); st4(&E[1][orow + 2][x], E2);
        }
        if (t < kHalo) {
            float4 E1 = zero4, E2 = zero4;
            if (halo_ok)
                stage_T(p, s, PSI_INT, 0, hj, hgg, Q ? kp_rw4(hK, hpb, hR, hw) : mul4(hK, hpb), false, !halo_row, halo_row, E1, E2);
            if (halo_row) st4(&E[1][hr][4 * hg], E2);       // (two stores: choosing between the two float4 puts both on the stack)
            else st4(&E[0][hr][4 * hg], E1);
        }
        // the snapshot planes are only needed after the barrier: requested last, they do not delay the staging
        if (own_ok) {
            const float *Sp = p.S + 3LL * s * p.splane + osc;
            S0 = mifwi::ldnt4(Sp); S1 = mifwi::ldnt4(Sp + (long long)p.splane); S2 = mifwi::ldnt4(Sp + 2 * (long long)p.splane);
        }
        __syncthreads();
        if (own_ok) {
            const int r = orow + 2, cb = 4 * (ogrp + 1);
            const Row8 x1 = row8(&E[0][r][0], cb);
            const float4 z2a = ld4(&E[1][r - 1][cb]), z2b = ld4(&E[1][r][cb]);
            const float4 z2c = ld4(&E[1][r + 1][cb]), z2d = ld4(&E[1][r + 2][cb]);
            float nvx[4], nvz[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                nvx[c] = comp(vxb, c) - dfw(K, x1.v[c + 1], x1.v[c + 2], x1.v[c + 3], x1.v[c + 4]);
                nvz[c] = comp(vzb, c) - dfw(K, comp(z2a, c), comp(z2b, c), comp(z2c, c), comp(z2d, c));
                if (4 * og + c >= p.nx) { nvx[c] = 0.f; nvz[c] = 0.f; }
            }
            st4(fl + F_VX * fs + oo, mk4(nvx));
            st4(fl + F_VZ * fs + oo, mk4(nvz));
            acc[M_K].x = fmaf(S0.x, pb.x, acc[M_K].x); acc[M_K].y = fmaf(S0.y, pb.y, acc[M_K].y);
            acc[M_K].z = fmaf(S0.z, pb.z, acc[M_K].z); acc[M_K].w = fmaf(S0.w, pb.w, acc[M_K].w);
            acc[M_BX].x = fmaf(S1.x, nvx[0], acc[M_BX].x); acc[M_BX].y = fmaf(S1.y, nvx[1], acc[M_BX].y);
            acc[M_BX].z = fmaf(S1.z, nvx[2], acc[M_BX].z); acc[M_BX].w = fmaf(S1.w, nvx[3], acc[M_BX].w);
            acc[M_BZ].x = fmaf(S2.x, nvz[0], acc[M_BZ].x); acc[M_BZ].y = fmaf(S2.y, nvz[1], acc[M_BZ].y);
            acc[M_BZ].z = fmaf(S2.z, nvz[2], acc[M_BZ].z); acc[M_BZ].w = fmaf(S2.w, nvz[3], acc[M_BZ].w);
            if (Q) {
                acc[NP - 1].x = fmaf(S0.x, ow.x, acc[NP - 1].x); acc[NP - 1].y = fmaf(S0.y, ow.y, acc[NP - 1].y);
                acc[NP - 1].z = fmaf(S0.z, ow.z, acc[NP - 1].z); acc[NP - 1].w = fmaf(S0.w, ow.w, acc[NP - 1].w);
            }
        }
        __syncthreads();          // E is reused by the next shot
    }
    if (own_ok) {
#pragma unroll
        for (int k = 0; k < NP; ++k) st4(accp + (long long)k * p.splane, acc[k]);
    }
}

// V^T:  D1 = pmlT(bx vx_bar), D4 = pmlT(bz vz_bar);  p_bar -= Dm_x D1 + Dm_z D4;  free surface: p_bar(1,.) += C2 D4(0,.)
// Q (viscoacoustic): the owner advances r_bar = a r_bar + (1 + a)/2 p_bar with the p_bar that P^T saw (as loaded here,
//       before this launch updates it; row 0 under a free surface: the cleared one)
template <bool Q>
__global__ __launch_bounds__(kThreads) void fl_adj_v(const FlParams p)
{
    const FdK K = p.fd;
    __shared__ float D[2][ASZ][ASX];
    int bx, by, bz;
    xcd_tile_major(bx, by, bz);
    const int tile_j = by * ATZ, tile_g = bx * AGO;
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
    const bool halo_row = t < kHaloRows;
    const unsigned hcc = (unsigned)hj * p.gp + 4 * hgg;
    const unsigned ho = (unsigned)(hj + 2) * p.pitch + 4 + 4 * hgg;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ovx = zero4, ovz = zero4, obx = zero4, obz = zero4, hv = zero4, hb = zero4, pb = zero4;
    if (own_ok) {
        ovx = ld4(fl + F_VX * fs + oo); ovz = ld4(fl + F_VZ * fs + oo);
        obx = ld4(p.mat + M_BX * ncell + occ); obz = ld4(p.mat + M_BZ * ncell + occ);
    }
    if (halo_ok) {       // a row of the z halo serves Dm_z D4, a group of the x halo Dm_x D1
        hv = ld4(fl + (halo_row ? F_VZ : F_VX) * fs + ho);
        hb = ld4(p.mat + (halo_row ? M_BZ : M_BX) * ncell + hcc);
    }
    if (own_ok) pb = ld4(fl + F_P * fs + oo);
    float4 rb = zero4;
    if (Q && own_ok) rb = ld4(fl + F_R * fs + oo);
    {
        float4 D1 = zero4, D4 = zero4, unused;
        if (own_ok) {
            stage_T(p, s, PSI_HALF, 1, oj, og, mul4(obx, ovx), true, true, false, D1, unused);
            stage_T(p, s, PSI_HALF, 1, oj, og, mul4(obz, ovz), true, false, true, unused, D4);
        }
        const int x = 4 * (ogrp + 1);
        st4(&D[0][orow + 2][x], D1); st4(&D[1][orow + 2][x], D4);
    }
    if (t < kHalo) {
        float4 D1 = zero4, D4 = zero4;
        if (halo_ok) stage_T(p, s, PSI_HALF, 1, hj, hgg, mul4(hb, hv), false, !halo_row, halo_row, D1, D4);
        if (halo_row) st4(&D[1][hr][4 * hg], D4);
        else st4(&D[0][hr][4 * hg], D1);
    }
    __syncthreads();
    if (own_ok) {
        const int r = orow + 2, cb = 4 * (ogrp + 1);
        const Row8 x1 = row8(&D[0][r][0], cb);
        const float4 z4a = ld4(&D[1][r - 2][cb]), z4b = ld4(&D[1][r - 1][cb]);
        const float4 z4c = ld4(&D[1][r][cb]), z4d = ld4(&D[1][r + 1][cb]);
        float np[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dx1 = dbw(K, x1.v[c], x1.v[c + 1], x1.v[c + 2], x1.v[c + 3]);
            const float dz4 = dbw(K, comp(z4a, c), comp(z4b, c), comp(z4c, c), comp(z4d, c));
            np[c] = comp(pb, c) - (dx1 + dz4);
            // transposed odd mirroring p(-1) = -p(1) (oj == 1: tile_j == 0, so z4b is D4 of grid row 0)
            if (p.fsurf && oj == 1) np[c] = np[c] + K.c2 * comp(z4b, c);
            if (4 * og + c >= p.nx) np[c] = 0.f;
        }
        st4(fl + F_P * fs + oo, mk4(np));
        if (Q) {
            const float ha = 0.5f * (1.f + p.rel_a);
            const float4 ps = (p.fsurf && oj == 0) ? zero4 : pb;
            st4(fl + F_R * fs + oo, make_float4(fmaf(p.rel_a, rb.x, ha * ps.x), fmaf(p.rel_a, rb.y, ha * ps.y),
                                                fmaf(p.rel_a, rb.z, ha * ps.z), fmaf(p.rel_a, rb.w, ha * ps.w)));
        }
    }
}

// ---- pressure receivers: launches of their own --------------------------------------------------------------
// forward: rec_p[n] = sum w (p + p)[cell] after P and the source term, for the p.gs shots of this pass
__global__ void fl_sample_pressure(const FlParams p)
{
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= p.gs * p.nsmp) return;
    const int s = p.s0 + idx / p.nsmp;
    if (s >= p.nshot) return;
    const int e = s * p.nsmp + idx % p.nsmp;
    const float *pp = p.fields + (long long)s * p.shot_stride + F_P * (long long)p.field_stride;
    float a = 0.f;
    for (int t = 0; t < p.ntap_smp; ++t) {
        const long long ee = (long long)e * p.ntap_smp + t;
        const int cell = p.smp_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        const float v = pp[(unsigned)(j + 2) * p.pitch + 4 + i];
        a = fmaf(p.smp_w[ee], v + v, a);
    }
    p.smp_out0[e] = a;
}

// adjoint: p_bar[cell] += 2 w g_p[n] before P^T (receivers normally sit on distinct cells; taps that share a cell add
// in hardware order, as in the LDS staging of the velocity receivers)
__global__ void fl_inject_pressure(const FlParams p)
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
    const float a = p.inj_w[ee] * p.inj_amp0[(long long)s * p.ninj + r / p.ntap_inj];
    atomicAdd(p.fields + (long long)s * p.shot_stride + F_P * (long long)p.field_stride + (unsigned)(j + 2) * p.pitch + 4 + i,
              a + a);
}

}  // namespace

// ================================================================================================
// ---- the medium of a plan ---------------------------------------------------------------------------
// Every plan of this file is a mifwi_fluid_plan; its medium says which kernels serve it, how many fields a shot has and how
// many planes mat, grad_mat and the accumulators take (the kMedia row of mifwi_elastic.hip, on the fluid side).  Lossless:
// fl_step_p / fl_adj_p / fl_adj_v with Q = false, finalize_groups<3>; viscoacoustic: Q = true, finalize_groups<4>.  The V
// launch, the point kernels and the three snapshot planes are the same for both.
namespace {
enum FlMedium { kLossless = 0, kViscoacoustic = 1 };
struct FlMediumInfo { int nfield, nmat; const char *created_by; };
constexpr FlMediumInfo kFlMedia[] = {{3, 3, "mifwi_fluid_plan_create"}, {4, 4, "mifwi_viscofluid_plan_create"}};
}  // namespace

struct mifwi_fluid_plan : StaggerGrid {      // grid, pitch and strips: stagger_grid with two memory variables per strip cell
    mifwi_fluid_desc d;
    FlMedium medium;       // kFlMedia[medium]: its fields, planes and entry points
    float rel_a, rel_b;    // viscoacoustic: the relaxation scalars
    int device;
    int lx, gs, ngroups;
    long long splane;      // floats per snapshot / accumulator plane
    int pass_shots;        // forward: shots per pass over the time range
    int pass_groups;       // adjoint: shot groups per pass
    long long shot_stride, fields_elems, psix_elems, psiz_elems, psi_elems;
    long long tile_elems;  // per-tile receiver lists of fl_adj_p (ints, in floats)
};

namespace {

FlParams fl_base(const mifwi_fluid_plan *pl, const float *mat, const float *pz, const float *px)
{
    FlParams p;
    memset(&p, 0, sizeof(p));
    p.nz = pl->d.nz; p.nx = pl->d.nx; p.ng = pl->ng; p.gp = pl->gp; p.pitch = pl->pitch;
    p.field_stride = (unsigned)pl->field_stride; p.shot_stride = pl->shot_stride;
    p.nshot = pl->d.nshot; p.gs = 1;
    p.W = pl->W; p.wl = pl->wl; p.xr0 = pl->xr0; p.wx = pl->wx;
    p.fsurf = pl->d.free_surface;
    p.psix_shot = pl->psix_shot; p.psiz_shot = pl->psiz_shot;
    p.mat = mat; p.pz = pz; p.px = px;
    p.splane = (unsigned)pl->splane;
    p.fd = fd_weights(pl->d.fd_order);
    p.rel_a = pl->rel_a; p.rel_b = pl->rel_b;
    return p;
}

// the two launches of a forward step, fl_step_v<LX, SAVE> (both media's) / fl_step_p<LX, SAVE, Q>: lanes per row
// 64 | 32 | 16; save kBorn (the background's snapshots read) | 1 (snapshots written) | 0; Q: the viscoacoustic medium
using FlKernel = void (*)(FlParams);
struct FlStepKernels { FlKernel v, p; };
FlStepKernels fl_step_variant(FlMedium medium, int lx, int save)
{
    return mifwi::with_int<64, 32, 16>(lx, [&](auto LX) {
    return mifwi::with_int<kBorn, 1, 0>(save, [&](auto SAVE) {
    return mifwi::with_bool(medium == kViscoacoustic, [&](auto Q) {
        return FlStepKernels{fl_step_v<decltype(LX)::value, decltype(SAVE)::value>,
                             fl_step_p<decltype(LX)::value, decltype(SAVE)::value, decltype(Q)::value>};
    }); }); });
}
// the two launches of an adjoint step
struct FlAdjKernels { FlKernel p, v; };
FlAdjKernels fl_adj_variant(FlMedium medium)
{
    return mifwi::with_bool(medium == kViscoacoustic, [&](auto Q) {
        return FlAdjKernels{fl_adj_p<decltype(Q)::value>, fl_adj_v<decltype(Q)::value>};
    });
}

// Offsets (in floats) of the regions of the work buffer.  Forward call: [fields | psi | bbox]; backward call:
// [fields | psi | psiB | acc | tile].  fields, the C-PML memory variables (backward: two copies that ping-pong,
// absolute in n) and the gradient accumulators (backward) are the `state`: what a call hands to the call that resumes
// it and what MIFWI_ZERO_STATE zeroes.  tile: the per-tile receiver lists of fl_adj_p.
struct FlWork { long long fields, psi, psiB, acc, bbox, tile, state, total; };
FlWork work_map(const mifwi_fluid_plan *pl, bool backward)
{
    FlWork m;
    m.fields = 0; m.psi = pl->fields_elems; m.psiB = m.psi + pl->psi_elems;
    m.acc = backward ? m.psiB + pl->psi_elems : m.psiB;
    m.state = m.acc + (backward ? (long long)kFlMedia[pl->medium].nmat * pl->ngroups * pl->splane : 0);
    m.bbox = m.tile = m.state;
    m.total = m.state + (backward ? pl->tile_elems : mifwi::round_up64(4LL * pl->d.nshot, 64));
    return m;
}

// The time loop of the forward (save 0 | 1: `snap` is written when save == 1) and of the Born pass (save kBorn: `snap` is
// the background run's, read; p.dmat set; p.fields / psix / psiz the perturbed state).  Step n of the snapshot buffer sits
// at snap + (n - snap_first) * snap_step.  f NULL: nothing is injected.  rec_vx / rec_vz (together) and rec_p NULL: not
// sampled.  Shots are independent: taken a few at a time, their state and the materials stay inside the Infinity Cache.
void fl_forward_steps(const mifwi_fluid_plan *pl, FlParams p, int save, const float *f, const int32_t *src_cell,
                      const float *src_w, const int *bbox, const int32_t *rec_cell, const float *rec_w, float *rec_vx,
                      float *rec_vz, float *rec_p, float *snap, int snap_first, int n_begin, int n_end, hipStream_t st)
{
    const mifwi_fluid_desc &d = pl->d;
    const bool inject = f != nullptr, want_v = rec_vx != nullptr, want_p = rec_p != nullptr;
    const FlStepKernels step = fl_step_variant(pl->medium, pl->lx, save);
    p.ntap_inj = d.ntap; p.inj_cell = src_cell; p.inj_w = src_w; p.inj_bbox = bbox;
    p.inj_field = d.source_type == 1 ? F_VX : F_VZ;
    p.nsmp = d.nrec; p.ntap_smp = d.ntap; p.smp_cell = rec_cell; p.smp_w = rec_w;
    const long long snap_step = 3 * pl->splane * d.nshot;
    const int lz = kThreads / pl->lx;
    const int tiles_x = mifwi::ceil_div(pl->ng, pl->lx), tiles_z = mifwi::ceil_div(d.nz, lz);
    const int extra = want_v ? mifwi::ceil_div(mifwi::ceil_div(d.nrec, kThreads), tiles_x) : 0;
    p.tiles_z = tiles_z;
    for (int s0 = 0; s0 < d.nshot; s0 += pl->pass_shots) {
        const int cs = std::min(pl->pass_shots, d.nshot - s0);
        p.s0 = s0;
        for (int n = n_begin; n < n_end; ++n) {
            p.S = save ? snap + (long long)(n - snap_first) * snap_step : nullptr;
            p.inj_amp0 = inject ? f + (long long)n * d.nshot * d.nsrc : nullptr;
            FlParams pv = p, pp = p;
            pv.ninj = (inject && d.source_type != 0) ? d.nsrc : 0;
            pp.ninj = (inject && d.source_type == 0) ? d.nsrc : 0;
            hipLaunchKernelGGL(step.v, dim3(tiles_x, tiles_z, cs), dim3(kThreads), 0, st, pv);
            pp.smp_out0 = want_v ? rec_vx + (long long)n * d.nshot * d.nrec : nullptr;
            pp.smp_out1 = want_v ? rec_vz + (long long)n * d.nshot * d.nrec : nullptr;
            hipLaunchKernelGGL(step.p, dim3(tiles_x, tiles_z + extra, cs), dim3(kThreads), 0, st, pp);
            if (want_p) {
                FlParams pq = p;
                pq.gs = cs; pq.smp_out0 = rec_p + (long long)n * d.nshot * d.nrec;
                hipLaunchKernelGGL(fl_sample_pressure, dim3(mifwi::ceil_div(cs * d.nrec, 64)), dim3(64), 0, st, pq);
            }
        }
    }
}

// a viscoacoustic plan is a fluid plan of that medium; the C ABI keeps the handle types apart
int fl_plan_create(mifwi_fluid_plan **plan, int device, const mifwi_fluid_desc *d, FlMedium medium, float rel_a = 0.f,
                   float rel_b = 0.f)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    int rc = check_stagger_desc(d, 3);
    if (!rc) rc = check_stagger_scheme(d);
    if (!rc) rc = mifwi::check_device(device);
    StaggerGrid grid;
    if (!rc) rc = stagger_grid(d->nz, d->nx, d->pml_width, 2, &grid);
    if (rc) return rc;
    mifwi_fluid_plan *pl = new mifwi_fluid_plan;
    static_cast<StaggerGrid &>(*pl) = grid;
    pl->d = *d;
    if (pl->d.fd_order == 0) pl->d.fd_order = 4;
    pl->device = device;
    pl->medium = medium; pl->rel_a = rel_a; pl->rel_b = rel_b;
    const int nfield = kFlMedia[medium].nfield, nmat = kFlMedia[medium].nmat;
    pl->shot_stride = nfield * pl->field_stride;
    pl->fields_elems = pl->shot_stride * d->nshot;
    pl->psix_elems = pl->psix_shot * d->nshot;
    pl->psiz_elems = pl->psiz_shot * d->nshot;
    pl->psi_elems = mifwi::round_up64(pl->psix_elems + pl->psiz_elems, 64);
    pl->lx = mifwi::pick_lx(pl->ng);
    pl->gs = default_group_size(d->shots_per_group, d->nshot, 4);
    pl->ngroups = mifwi::ceil_div(d->nshot, pl->gs);
    pl->splane = blocked_plane_elems(d->nz, pl->ng);
    pl->tile_elems = tile_taps_elems(d->nshot, d->nz, pl->ng, d->nrec, d->ntap);
    {
        // Infinity Cache residency: a pass over the time range takes only as many shots (shot groups) as keep state,
        // materials and accumulators under the bounds the elastic per-step family measured on this cache (250 MB; the
        // forward plans for 230 MB once it has to cut).  MIFWI_FL_PASS_SHOTS / MIFWI_FL_PASS_GROUPS override the two sizes
        // (tests run passes of one shot / one group on small grids; measurements around the defaults)
        constexpr double kResident = 250e6;
        const double cells = (double)pl->coef_elems, mats = 4.0 * nmat * cells;
        const double psi1 = 4.0 * (double)(pl->psix_shot + pl->psiz_shot);
        const double fstate = 4.0 * (double)pl->shot_stride + psi1;
        const int ps = mifwi::env_int("MIFWI_FL_PASS_SHOTS", mifwi::units_per_pass(d->nshot, fstate, mats, kResident, 230e6, 1));
        pl->pass_shots = std::min(d->nshot, std::max(1, ps));
        const double astate = 4.0 * (double)pl->shot_stride + 2.0 * psi1, accg = 4.0 * nmat * cells;
        const int pg = mifwi::env_int("MIFWI_FL_PASS_GROUPS", mifwi::units_per_pass(pl->ngroups, pl->gs * astate + accg, mats,
                                                                                     kResident, kResident, pl->ngroups));
        pl->pass_groups = std::min(pl->ngroups, std::max(1, pg));
    }
    *plan = pl;
    return MIFWI_OK;
}

// Refuses the plan of the other medium: its kernels would take kFlMedia[].nmat planes and fields where the caller allocated
// this one's.  (A null plan passes: the call itself refuses it.)
int check_medium(const mifwi_fluid_plan *pl, FlMedium medium)
{
    return (pl && pl->medium != medium) ? mifwi::fail(MIFWI_EINVAL, "the plan was not created by %s", kFlMedia[medium].created_by)
                                        : MIFWI_OK;
}

}  // namespace

extern "C" {

int mifwi_fluid_plan_create(mifwi_fluid_plan **plan, int device, const mifwi_fluid_desc *d)
{
    return fl_plan_create(plan, device, d, kLossless);
}

int mifwi_fluid_plan_destroy(mifwi_fluid_plan *plan)
{
    delete plan;
    return MIFWI_OK;
}

int mifwi_fluid_plan_cluster_slabs(const mifwi_fluid_plan *, int32_t) { return 0; }

int mifwi_fluid_plan_pass_sizes(const mifwi_fluid_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    if (!plan) return mifwi::fail(MIFWI_EINVAL, "null plan");
    if (forward_shots) *forward_shots = plan->pass_shots;
    if (adjoint_groups) *adjoint_groups = plan->pass_groups;
    return MIFWI_OK;
}

int mifwi_fluid_plan_layout(const mifwi_fluid_plan *pl, mifwi_fluid_layout *out)
{
    if (!pl || !out) return mifwi::fail(MIFWI_EINVAL, "null plan/layout");
    out->gp = pl->gp; out->pitch = pl->pitch; out->ngroups = pl->ngroups;
    out->shots_per_group = pl->gs;
    out->coef_elems = pl->coef_elems;
    out->snap_step_elems = 3 * pl->splane * pl->d.nshot;
    const FlWork fwd = work_map(pl, false);
    out->state_elems = fwd.state;
    out->work_forward_elems = fwd.total;
    out->work_backward_elems = work_map(pl, true).total;
    return MIFWI_OK;
}

// ---- the three calls of a plan, whatever its medium: what the entry points of both families run ---------------------
static int fl_forward(mifwi_fluid_plan *pl, const float *mat, const float *pz, const float *px, const float *f,
                      const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                      float *rec_vx, float *rec_vz, float *rec_p, float *snap, float *work, int32_t n_begin,
                      int32_t n_end, int32_t flags, void *stream)
{
    if (!pl || !mat || !pz || !px || !work) return mifwi::fail(MIFWI_EINVAL, "null argument");
    const mifwi_fluid_desc &d = pl->d;
    int rc = mifwi::check_steps(n_begin, n_end, d.nt);
    if (rc) return rc;
    if (d.nsrc > 0 && (!f || !src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "sources declared but f/src_cell/src_w is null");
    if ((rec_vx == nullptr) != (rec_vz == nullptr))
        return mifwi::fail(MIFWI_EINVAL, "rec_vx and rec_vz go together");
    if ((rec_vx || rec_p) && (!rec_cell || !rec_w))
        return mifwi::fail(MIFWI_EINVAL, "receiver output needs rec_cell and rec_w");
    const FlWork m = work_map(pl, false);                 // the state is updated in place
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    int *bbox = reinterpret_cast<int *>(work + m.bbox);
    const bool inject = d.nsrc > 0;
    if (inject) launch_points_bbox(src_cell, d.nshot, d.nsrc * d.ntap, d.nx, bbox, st);
    FlParams p = fl_base(pl, mat, pz, px);
    p.fields = work + m.fields; p.psix = work + m.psi; p.psiz = p.psix + pl->psix_elems;
    const bool want_v = rec_vx != nullptr && d.nrec > 0, want_p = rec_p != nullptr && d.nrec > 0;
    fl_forward_steps(pl, p, snap ? 1 : 0, inject ? f : nullptr, src_cell, src_w, bbox, rec_cell, rec_w,
                     want_v ? rec_vx : nullptr, want_v ? rec_vz : nullptr, want_p ? rec_p : nullptr, snap, n_begin, n_begin,
                     n_end, st);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

static int fl_born(mifwi_fluid_plan *pl, const float *mat, const float *dmat, const float *pz, const float *px,
                   const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell,
                   const float *rec_w, const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                   float *drec_p, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream)
{
    if (!pl || !mat || !pz || !px) return mifwi::fail(MIFWI_EINVAL, "null argument");
    if (!dmat || !snap || !work) return mifwi::fail(MIFWI_EINVAL, "born: dmat, snap and work must not be null");
    const mifwi_fluid_desc &d = pl->d;
    int rc = mifwi::check_steps(n_begin, n_end, d.nt);
    if (!rc) rc = mifwi::check_snapshots(snap_first, n_begin);
    if (rc) return rc;
    if (snap_first < 0) return mifwi::fail(MIFWI_EINVAL, "born: snap_first %d < 0", snap_first);
    if (df && d.nsrc > 0 && (!src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "df given but src_cell/src_w is null");
    if ((drec_vx == nullptr) != (drec_vz == nullptr))
        return mifwi::fail(MIFWI_EINVAL, "drec_vx and drec_vz go together");
    if ((drec_vx || drec_p) && (!rec_cell || !rec_w))
        return mifwi::fail(MIFWI_EINVAL, "receiver output needs rec_cell and rec_w");
    const FlWork m = work_map(pl, false);                 // the perturbed state: the forward's map of `work`
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    int *bbox = reinterpret_cast<int *>(work + m.bbox);
    const bool inject = df != nullptr && d.nsrc > 0;
    if (inject) launch_points_bbox(src_cell, d.nshot, d.nsrc * d.ntap, d.nx, bbox, st);
    FlParams p = fl_base(pl, mat, pz, px);
    p.dmat = dmat;
    p.fields = work + m.fields; p.psix = work + m.psi; p.psiz = p.psix + pl->psix_elems;
    const bool want_v = drec_vx != nullptr && d.nrec > 0, want_p = drec_p != nullptr && d.nrec > 0;
    fl_forward_steps(pl, p, kBorn, inject ? df : nullptr, src_cell, src_w, bbox, rec_cell, rec_w,
                     want_v ? drec_vx : nullptr, want_v ? drec_vz : nullptr, want_p ? drec_p : nullptr,
                     const_cast<float *>(snap), snap_first, n_begin, n_end, st);
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

static int fl_backward(mifwi_fluid_plan *pl, const float *mat, const float *pz, const float *px,
                       const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                       const float *g_vx, const float *g_vz, const float *g_p, const float *snap, int32_t snap_first,
                       float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo, int32_t flags,
                       void *stream)
{
    if (!pl || !mat || !pz || !px || !work || !snap) return mifwi::fail(MIFWI_EINVAL, "null argument");
    const mifwi_fluid_desc &d = pl->d;
    int rc = mifwi::check_adjoint_steps('n', 0, n_hi, n_lo, d.nt);
    if (!rc) rc = mifwi::check_snapshots(snap_first, n_lo);
    if (rc) return rc;
    if ((g_vx || g_vz || g_p) && (!rec_cell || !rec_w))
        return mifwi::fail(MIFWI_EINVAL, "adjoint sources given but rec_cell/rec_w is null");
    if (grad_f && (!src_cell || !src_w))
        return mifwi::fail(MIFWI_EINVAL, "grad_f requested but src_cell/src_w is null");
    if ((flags & MIFWI_FINALIZE) && !grad_mat)
        return mifwi::fail(MIFWI_EINVAL, "finalize requested but grad_mat is null");
    const FlWork m = work_map(pl, true);
    hipStream_t st;
    if ((rc = mifwi::open_call(pl->device, stream, work, m, flags, &st))) return rc;
    float *psiA = work + m.psi, *psiB = work + m.psiB, *acc = work + m.acc;
    FlParams p = fl_base(pl, mat, pz, px);
    p.fields = work + m.fields;
    p.acc = acc;
    p.ninj = d.nrec; p.ntap_inj = d.ntap; p.inj_cell = rec_cell; p.inj_w = rec_w;
    const bool want_f = grad_f != nullptr && d.nsrc > 0, force = d.source_type != 0;
    p.nsmp = want_f ? d.nsrc : 0; p.ntap_smp = d.ntap; p.smp_cell = src_cell; p.smp_w = src_w;
    const long long snap_step = 3 * pl->splane * d.nshot;
    const int tx = mifwi::ceil_div(pl->ng, AGO), tz = mifwi::ceil_div(d.nz, ATZ);
    p.tiles_z = tz;
    const FlAdjKernels adj = fl_adj_variant(pl->medium);
    // per-tile receiver lists: fl_adj_p adds the velocity adjoint sources of its tile
    if ((g_vx || g_vz) && d.nrec > 0 && n_hi >= n_lo) {
        const int ntiles = tx * tz;
        int *start = reinterpret_cast<int *>(work + m.tile);
        int *cursor = start + (long long)d.nshot * (ntiles + 1);
        int *list = cursor + (long long)d.nshot * ntiles;
        hipLaunchKernelGGL(build_tile_taps, dim3(d.nshot), dim3(256), 0, st, rec_cell, d.nrec * d.ntap, d.nx, tx, ntiles,
                           start, cursor, list);
        p.tile_start = start; p.tile_list = list;
    }
    // shot groups are independent: a few at a time keep fields, accumulators and materials in the Infinity Cache
    for (int g0 = 0; g0 < pl->ngroups; g0 += pl->pass_groups)
    for (int n = n_hi; n >= n_lo; --n) {
        const int cg = std::min(pl->pass_groups, pl->ngroups - g0);
        const int cs = std::min(cg * pl->gs, d.nshot - g0 * pl->gs);
        p.s0 = g0 * pl->gs;
        // ping-pong of the adjoint memory variables is absolute in n (resumable ranges)
        const int par = (d.nt - 1 - n) & 1;
        float *rd = par ? psiB : psiA, *wr = par ? psiA : psiB;
        p.psix = rd; p.psiz = rd + pl->psix_elems;
        p.psix_out = wr; p.psiz_out = wr + pl->psix_elems;
        p.S = const_cast<float *>(snap) + (long long)(n - snap_first) * snap_step;
        const long long rec_n = (long long)n * d.nshot * d.nrec;
        if (g_p && d.nrec > 0) {
            FlParams pq = p;
            pq.gs = cs; pq.inj_amp0 = g_p + rec_n;
            hipLaunchKernelGGL(fl_inject_pressure, dim3(mifwi::ceil_div(cs * d.nrec * d.ntap, 64)), dim3(64), 0, st, pq);
        }
        FlParams pp = p;
        pp.gs = pl->gs;
        pp.inj_amp0 = g_vx ? g_vx + rec_n : nullptr;
        pp.inj_amp1 = g_vz ? g_vz + rec_n : nullptr;
        pp.smp_out0 = (want_f && !force) ? grad_f + (long long)n * d.nshot * d.nsrc : nullptr;
        const int ex = (want_f && !force) ? mifwi::ceil_div(mifwi::ceil_div(pl->gs * d.nsrc, kThreads), tx) : 0;
        hipLaunchKernelGGL(adj.p, dim3(tx, tz + ex, cg), dim3(kThreads), 0, st, pp);
        if (want_f && force) {
            FlParams pq = p;
            pq.gs = cs; pq.smp_out0 = grad_f + (long long)n * d.nshot * d.nsrc;
            hipLaunchKernelGGL(sample_force<FlParams>, dim3(mifwi::ceil_div(cs * d.nsrc, 64)), dim3(64), 0, st, pq,
                               d.source_type == 1 ? F_VX : F_VZ);
        }
        hipLaunchKernelGGL(adj.v, dim3(tx, tz, cs), dim3(kThreads), 0, st, p);
    }
    if (flags & MIFWI_FINALIZE) {
        const long long n3 = (long long)kFlMedia[pl->medium].nmat * pl->coef_elems;
        const auto fin = pl->medium == kViscoacoustic ? finalize_groups<4> : finalize_groups<3>;
        hipLaunchKernelGGL(fin, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, acc, pl->ngroups, d.nz,
                           pl->gp, pl->splane, 1, grad_mat);
    }
    MIFWI_HIP_TRY(hipGetLastError());
    return MIFWI_OK;
}

// lossless
int mifwi_fluid_forward(mifwi_fluid_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                        const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                        float *rec_vx, float *rec_vz, float *rec_p, float *snap, float *work, int32_t n_begin,
                        int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan, kLossless)) return rc;
    return fl_forward(plan, mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, rec_p, snap, work, n_begin,
                      n_end, flags, stream);
}

int mifwi_fluid_born(mifwi_fluid_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                     const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell,
                     const float *rec_w, const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                     float *drec_p, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(plan, kLossless)) return rc;
    return fl_born(plan, mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx, drec_vz,
                   drec_p, work, n_begin, n_end, flags, stream);
}

int mifwi_fluid_backward(mifwi_fluid_plan *plan, const float *mat, const float *pz, const float *px,
                         const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                         const float *g_vx, const float *g_vz, const float *g_p, const float *snap, int32_t snap_first,
                         float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo, int32_t flags,
                         void *stream)
{
    if (const int rc = check_medium(plan, kLossless)) return rc;
    return fl_backward(plan, mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, g_p, snap, snap_first, grad_mat,
                       grad_f, work, n_hi, n_lo, flags, stream);
}

// viscoacoustic: four fields per shot and four planes, the same launches
static mifwi_fluid_plan *fl_cast(mifwi_viscofluid_plan *h) { return reinterpret_cast<mifwi_fluid_plan *>(h); }
static const mifwi_fluid_plan *fl_cast(const mifwi_viscofluid_plan *h) { return reinterpret_cast<const mifwi_fluid_plan *>(h); }

int mifwi_viscofluid_plan_create(mifwi_viscofluid_plan **plan, int device, const mifwi_viscofluid_desc *d)
{
    if (!plan || !d) return mifwi::fail(MIFWI_EINVAL, "null plan/desc");
    // a = (2 - eta) / (2 + eta), b = 2 eta / (2 + eta) with 0 < eta < 2: 0 < a < 1 and b = 1 - a
    if (!(d->relax_a > 0.f && d->relax_a < 1.f && d->relax_b > 0.f && d->relax_b < 1.f))
        return mifwi::fail(MIFWI_EINVAL, "relax_a = %g, relax_b = %g: both must lie inside (0, 1)", (double)d->relax_a,
                           (double)d->relax_b);
    mifwi_fluid_desc e;
    e.nz = d->nz; e.nx = d->nx; e.nt = d->nt; e.nshot = d->nshot; e.nsrc = d->nsrc; e.nrec = d->nrec; e.ntap = d->ntap;
    e.pml_width = d->pml_width; e.free_surface = d->free_surface; e.shots_per_group = d->shots_per_group;
    e.source_type = d->source_type; e.fd_order = d->fd_order;
    return fl_plan_create(reinterpret_cast<mifwi_fluid_plan **>(plan), device, &e, kViscoacoustic, d->relax_a, d->relax_b);
}

int mifwi_viscofluid_plan_destroy(mifwi_viscofluid_plan *plan) { return mifwi_fluid_plan_destroy(fl_cast(plan)); }

int mifwi_viscofluid_plan_layout(const mifwi_viscofluid_plan *plan, mifwi_viscofluid_layout *out)
{
    if (!plan || !out) return mifwi::fail(MIFWI_EINVAL, "null plan/layout");
    mifwi_fluid_layout e;
    if (const int rc = mifwi_fluid_plan_layout(fl_cast(plan), &e)) return rc;
    out->gp = e.gp; out->pitch = e.pitch; out->ngroups = e.ngroups; out->shots_per_group = e.shots_per_group;
    out->coef_elems = e.coef_elems; out->state_elems = e.state_elems; out->work_forward_elems = e.work_forward_elems;
    out->work_backward_elems = e.work_backward_elems; out->snap_step_elems = e.snap_step_elems;
    return MIFWI_OK;
}

int mifwi_viscofluid_plan_pass_sizes(const mifwi_viscofluid_plan *plan, int32_t *forward_shots, int32_t *adjoint_groups)
{
    return mifwi_fluid_plan_pass_sizes(fl_cast(plan), forward_shots, adjoint_groups);
}

int mifwi_viscofluid_plan_cluster_slabs(const mifwi_viscofluid_plan *, int32_t) { return 0; }

int mifwi_viscofluid_forward(mifwi_viscofluid_plan *plan, const float *mat, const float *pz, const float *px, const float *f,
                             const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                             float *rec_vx, float *rec_vz, float *rec_p, float *snap, float *work, int32_t n_begin,
                             int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(fl_cast(plan), kViscoacoustic)) return rc;
    return fl_forward(fl_cast(plan), mat, pz, px, f, src_cell, src_w, rec_cell, rec_w, rec_vx, rec_vz, rec_p, snap, work,
                      n_begin, n_end, flags, stream);
}

int mifwi_viscofluid_born(mifwi_viscofluid_plan *plan, const float *mat, const float *dmat, const float *pz, const float *px,
                          const float *df, const int32_t *src_cell, const float *src_w, const int32_t *rec_cell,
                          const float *rec_w, const float *snap, int32_t snap_first, float *drec_vx, float *drec_vz,
                          float *drec_p, float *work, int32_t n_begin, int32_t n_end, int32_t flags, void *stream)
{
    if (const int rc = check_medium(fl_cast(plan), kViscoacoustic)) return rc;
    return fl_born(fl_cast(plan), mat, dmat, pz, px, df, src_cell, src_w, rec_cell, rec_w, snap, snap_first, drec_vx,
                   drec_vz, drec_p, work, n_begin, n_end, flags, stream);
}

int mifwi_viscofluid_backward(mifwi_viscofluid_plan *plan, const float *mat, const float *pz, const float *px,
                              const int32_t *src_cell, const float *src_w, const int32_t *rec_cell, const float *rec_w,
                              const float *g_vx, const float *g_vz, const float *g_p, const float *snap,
                              int32_t snap_first, float *grad_mat, float *grad_f, float *work, int32_t n_hi, int32_t n_lo,
                              int32_t flags, void *stream)
{
    if (const int rc = check_medium(fl_cast(plan), kViscoacoustic)) return rc;
    return fl_backward(fl_cast(plan), mat, pz, px, src_cell, src_w, rec_cell, rec_w, g_vx, g_vz, g_p, snap, snap_first,
                       grad_mat, grad_f, work, n_hi, n_lo, flags, stream);
}

}  // extern "C"

#include "mifwi_fluid_moments.h"
