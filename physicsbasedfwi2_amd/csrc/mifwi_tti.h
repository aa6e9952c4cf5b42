// Elastic P-SV propagator in a medium with a TILTED symmetry axis (TTI, mifwi_tti_*): the kernels of the stress half step
// and of its transpose.  Included by mifwi_elastic.hip; the V launches (el_step_v, el_adj_v) are every medium's.
//
// Rotating the VTI stiffnesses couples the normal stresses to the shear strain (c15, c35 on the sxx node) and the shear
// stress to the normal strains.  On the staggered grid those live on different nodes, so the coupling goes through the
// two four-point averages of include/mifwi.h, A (sxz nodes -> sxx node) and A^T (sxx nodes -> sxz node), and through
// w = (c55_xz != 0), the 0/1 mask on the sxz node that keeps the operator definite where the shear modulus vanishes:
//   sxx += c11 e1' + c13 e2' + c15 A(w e5'),  szz += c13 e1' + c33 e2' + c35 A(w e5'),  sxz += c55 e5' + w A^T(c15 e1' + c35 e2')
// A node therefore needs its neighbours' C-PML-corrected strains.  el_step_s updates the C-PML memory of its own nodes
// in place, so a neighbour's corrected strain cannot be recomputed in the same launch: the stress half step is two
// launches, and so is its transpose.
//   forward:  tti_strain  e1', e2', e5' of every node (C-PML recursion in place) -> three planes of the snapshot planes'
//                         layout: the step's snapshot planes 0..2 when they are saved (they hold exactly these), else
//                         three work planes per shot
//             tti_stress  the eight planes and the strains with their four-point footprints -> stresses; source
//                         injection and receiver sampling ride here as they ride in el_step_s.  Born step: the same on
//                         the perturbed strains, plus dmat8 on the background run's strains (w from the background c55)
//   adjoint:  tti_adj_e   e_bar = C^T sigma_bar through the symmetric operator -> three work planes per shot; the six
//                         stiffness gradients and the two coupling gradients (the neighbours' saved strains are read-only)
//             tti_adj_s   el_adj_s from there on: transposed C-PML and stencils on the staged e_bar planes, adjoint
//                         sources, g_bx and g_bz from the new v_bar, grad_f
// With c15 = c35 = 0 the coupling terms are +-0 added AFTER the VTI fmaf chain: the stored stresses are the VTI bits.
#pragma once

enum { M_C15 = 6, M_C35 = 7 };     // behind the six VTI planes; both on the sxx node

struct TtiParams : ElParams {
    float *E;              // [nshot] x three planes (p.splane floats each, snap_cell order): the strains / adjoint strains
    long long e_shot;      // floats per shot of E (p.snap_shot where E is the step's snapshot slice)
};

enum { kLayMat = 0, kLaySnap = 1, kLayField = 2 };   // a material plane [nz][gp], a snapshot-layout plane, a field of the state
template <int LAY>
__device__ __forceinline__ unsigned tti_off(const ElParams &p, int j, int g)
{
    if (LAY == kLayMat) return (unsigned)j * p.gp + 4u * (unsigned)g;
    if (LAY == kLaySnap) return snap_cell(p, j, g);
    return (unsigned)(j + 2) * p.pitch + 4u + 4u * (unsigned)g;
}
// columns 4g-1 .. 4g+3 (LEFT) or 4g .. 4g+4 of row j of a plane; entries outside the grid are 0 (g is inside it)
struct Row5 { float v[5]; };
template <int LAY, bool LEFT>
__device__ __forceinline__ Row5 tti_row5(const ElParams &p, const float *plane, int j, int g)
{
    Row5 r{{0.f, 0.f, 0.f, 0.f, 0.f}};
    if (j < 0 || j >= p.nz) return r;
    // uniform base + 32-bit lane offset (el_at): no 64-bit vector address per load
    const float4 c = ld4(el_at(plane, tti_off<LAY>(p, j, g)));
    if (LEFT) {
        if (g > 0) r.v[0] = *el_at(plane, tti_off<LAY>(p, j, g - 1) + 3u);
        r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
    } else {
        r.v[0] = c.x; r.v[1] = c.y; r.v[2] = c.z; r.v[3] = c.w;
        if (g + 1 < p.ng) r.v[4] = *el_at(plane, tti_off<LAY>(p, j, g + 1));
    }
    return r;
}
// w on columns 4g-1 .. 4g+3 of rows j and j-1: what A reads around group g of row j (w0.v[1..4]: the group's own nodes)
struct TtiMask { Row5 w0, wm; };
__device__ __forceinline__ TtiMask tti_mask(const ElParams &p, const float *c55, int j, int g)
{
    TtiMask m{tti_row5<kLayMat, true>(p, c55, j, g), tti_row5<kLayMat, true>(p, c55, j - 1, g)};
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        m.w0.v[c] = m.w0.v[c] != 0.f ? 1.f : 0.f;
        m.wm.v[c] = m.wm.v[c] != 0.f ? 1.f : 0.f;
    }
    return m;
}
// a = A(w q5) at group g of row j
template <int LAY>
__device__ __forceinline__ void tti_A(const ElParams &p, const float *q5, const TtiMask &m, int j, int g, float a[4])
{
    const Row5 r0 = tti_row5<LAY, true>(p, q5, j, g), rm = tti_row5<LAY, true>(p, q5, j - 1, g);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        a[c] = 0.25f * ((m.w0.v[c + 1] * r0.v[c + 1] + m.wm.v[c + 1] * rm.v[c + 1]) + (m.w0.v[c] * r0.v[c] + m.wm.v[c] * rm.v[c]));
}
// t = w A^T(k1 q1 + k2 q2) at group g of row j; drop_row0: q2 of row 0 counts as 0 (the adjoint szz of a free surface)
template <int LAY>
__device__ __forceinline__ void tti_At(const ElParams &p, const float *q1, const float *q2, const float *k1, const float *k2,
                                       const TtiMask &m, int j, int g, bool drop_row0, float t[4])
{
    Row5 x[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int jj = j + r;
        const Row5 a = tti_row5<LAY, false>(p, q1, jj, g), c1 = tti_row5<kLayMat, false>(p, k1, jj, g);
        const Row5 c2 = tti_row5<kLayMat, false>(p, k2, jj, g);
        Row5 b = tti_row5<LAY, false>(p, q2, jj, g);
        if (drop_row0 && jj == 0) b = Row5{{0.f, 0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < 5; ++c) x[r].v[c] = fmaf(c1.v[c], a.v[c], c2.v[c] * b.v[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        t[c] = m.w0.v[c + 1] * (0.25f * ((x[0].v[c] + x[1].v[c]) + (x[0].v[c + 1] + x[1].v[c + 1])));
}

// ================================================================================================
// forward strain launch: e1' = Dm_x vx, e2' = Dm_z vz, e5' = Dp_z vx + Dp_x vz through the C-PML, as el_step_s forms them
// (the same operations in the same order: the same bits), one thread per four-cell group
// ================================================================================================
template <int LX>
__global__ __launch_bounds__(kThreads) void tti_strain(const TtiParams p)
{
    const FdK K = p.K;
    constexpr int LZ = kThreads / LX;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    const int lx = (int)threadIdx.x % LX, lz = (int)threadIdx.x / LX;
    const int g = bx * LX + lx, j = by * LZ + lz;
    if (g >= p.ng || j >= p.nz) return;
    const int s = p.s0 + bz;
    const unsigned fs = p.field_stride;
    const float *fl = p.fields + (long long)s * p.shot_stride;
    const float *vx = fl + F_VX * fs, *vz = fl + F_VZ * fs;
    const unsigned o = (unsigned)(j + 2) * p.pitch + 4 + 4 * g;
    // vz rows j-2..j+1 (a0..a3), vx rows j-1..j+2 (b0..b3)
    const float4 a0 = ld4(vz + o - 2 * p.pitch), a1 = ld4(vz + o - p.pitch), a2 = ld4(vz + o), a3 = ld4(vz + o + p.pitch);
    const float4 b0 = ld4(vx + o - p.pitch), b1 = ld4(vx + o), b2 = ld4(vx + o + p.pitch), b3 = ld4(vx + o + 2 * p.pitch);
    const float2 Lvx = ld2(vx + o - 2), Rvx = ld2(vx + o + 4);
    const float2 Lvz = ld2(vz + o - 2), Rvz = ld2(vz + o + 4);
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
    const int xs_off = xstrip(p, g);
    if (xs_off >= 0) {
        const float4 pxa = ld4(p.px + PA * p.gp + 4 * g), pxb = ld4(p.px + PB * p.gp + 4 * g);
        const float4 pxk = ld4(p.px + PK * p.gp + 4 * g), pxah = ld4(p.px + PAH * p.gp + 4 * g);
        const float4 pxbh = ld4(p.px + PBH * p.gp + 4 * g), pxkh = ld4(p.px + PKH * p.gp + 4 * g);
        float *q5 = p.psix + (long long)s * p.psix_shot + ((long long)2 * p.nz + j) * p.wx + xs_off;
        float *q8 = p.psix + (long long)s * p.psix_shot + ((long long)3 * p.nz + j) * p.wx + xs_off;
        const float4 s5 = ld4(q5), s8 = ld4(q8);
        float t5[4] = {s5.x, s5.y, s5.z, s5.w}, t8[4] = {s8.x, s8.y, s8.z, s8.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e1[c] = pml(t5[c], comp(pxa, c), comp(pxb, c), comp(pxk, c), e1[c]);
            e4[c] = pml(t8[c], comp(pxah, c), comp(pxbh, c), comp(pxkh, c), e4[c]);
        }
        st4(q5, mk4(t5));
        st4(q8, mk4(t8));
    }
    const int zs = zstrip(p, j);
    if (zs >= 0) {
        const float za = p.pz[PA * p.nz + j], zb = p.pz[PB * p.nz + j], zk = p.pz[PK * p.nz + j];
        const float zah = p.pz[PAH * p.nz + j], zbh = p.pz[PBH * p.nz + j], zkh = p.pz[PKH * p.nz + j];
        float *q6 = p.psiz + (long long)s * p.psiz_shot + ((long long)2 * 2 * p.W + zs) * p.gp + 4 * g;
        float *q7 = p.psiz + (long long)s * p.psiz_shot + ((long long)3 * 2 * p.W + zs) * p.gp + 4 * g;
        const float4 s6 = ld4(q6), s7 = ld4(q7);
        float t6[4] = {s6.x, s6.y, s6.z, s6.w}, t7[4] = {s7.x, s7.y, s7.z, s7.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e2[c] = pml(t6[c], za, zb, zk, e2[c]);
            e3[c] = pml(t7[c], zah, zbh, zkh, e3[c]);
        }
        st4(q6, mk4(t6));
        st4(q7, mk4(t7));
    }
    float e5[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) e5[c] = e3[c] + e4[c];
    // plain stores: the stress launch reads these planes right away
    float *Ep = p.E + (long long)s * p.e_shot + snap_cell(p, j, g);
    st4(Ep, mk4(e1));
    st4(Ep + (long long)p.splane, mk4(e2));
    st4(Ep + 2 * (long long)p.splane, mk4(e5));
}

// ================================================================================================
// forward stress launch: the VTI fmaf chain, then the coupling terms; source injection and receiver sampling as in el_step_s.
// BORN: the state is the perturbed one; dmat8 acts on the strains S0..S2 of the background run's step (p.S), with the
// same footprints and the background's w
// ================================================================================================
template <int LX, bool BORN>
__global__ __launch_bounds__(kThreads) void tti_stress(const TtiParams p)
{
    constexpr int LZ = kThreads / LX;
    constexpr int TZ = LZ, TX = LX * 4;
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
    const int j = tile_j + lz;
    const bool active = (g < p.ng) && (j < p.nz);
    const unsigned fs = p.field_stride;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const long long sp = p.splane;
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        const bool has_inj = stage_injection<TZ, TX, 1>(p, s, tile_j, tile_i, inj);
        if (active) {
            float *fl = p.fields + (long long)s * p.shot_stride;
            float *sxx = fl + F_SXX * fs, *szz = fl + F_SZZ * fs, *sxz = fl + F_SXZ * fs;
            const unsigned o = (unsigned)(j + 2) * p.pitch + 4 + 4 * g;
            const unsigned cc = (unsigned)j * p.gp + 4 * g;
            const unsigned so = snap_cell(p, j, g);
            const float *Ep = p.E + (long long)s * p.e_shot;
            const float4 e1 = ld4(Ep + so), e2 = ld4(Ep + sp + so), e5 = ld4(Ep + 2 * sp + so);
            const float4 vxx = ld4(sxx + o), vzz = ld4(szz + o), vxz = ld4(sxz + o);
            const float4 c13 = ld4(p.mat + M_L * ncell + cc), c11 = ld4(p.mat + M_M * ncell + cc);
            const float4 c55 = ld4(p.mat + M_MU * ncell + cc), c33 = ld4(p.mat + M_C33 * ncell + cc);
            const float4 c15 = ld4(p.mat + M_C15 * ncell + cc), c35 = ld4(p.mat + M_C35 * ncell + cc);
            const TtiMask w = tti_mask(p, p.mat + M_MU * ncell, j, g);
            float a[4], t[4];
            tti_A<kLaySnap>(p, Ep + 2 * sp, w, j, g, a);
            tti_At<kLaySnap>(p, Ep, Ep + sp, p.mat + M_C15 * ncell, p.mat + M_C35 * ncell, w, j, g, false, t);
            float nxx[4], nzz[4], nxz[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                nxx[c] = fmaf(comp(c11, c), comp(e1, c), fmaf(comp(c13, c), comp(e2, c), comp(vxx, c))) + comp(c15, c) * a[c];
                nzz[c] = fmaf(comp(c13, c), comp(e1, c), fmaf(comp(c33, c), comp(e2, c), comp(vzz, c))) + comp(c35, c) * a[c];
                nxz[c] = fmaf(comp(c55, c), comp(e5, c), comp(vxz, c)) + t[c];
            }
            if (BORN) {
                const float *Bp = p.S + (long long)s * p.snap_shot;
                const float4 B1 = mifwi::ldnt4(Bp + so), B2 = mifwi::ldnt4(Bp + sp + so), B5 = mifwi::ldnt4(Bp + 2 * sp + so);
                const float4 d13 = ld4(p.dmat + M_L * ncell + cc), d11 = ld4(p.dmat + M_M * ncell + cc);
                const float4 d55 = ld4(p.dmat + M_MU * ncell + cc), d33 = ld4(p.dmat + M_C33 * ncell + cc);
                const float4 d15 = ld4(p.dmat + M_C15 * ncell + cc), d35 = ld4(p.dmat + M_C35 * ncell + cc);
                float ab[4], tb[4];
                tti_A<kLaySnap>(p, Bp + 2 * sp, w, j, g, ab);
                tti_At<kLaySnap>(p, Bp, Bp + sp, p.dmat + M_C15 * ncell, p.dmat + M_C35 * ncell, w, j, g, false, tb);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    nxx[c] = fmaf(comp(d11, c), comp(B1, c), fmaf(comp(d13, c), comp(B2, c), nxx[c])) + comp(d15, c) * ab[c];
                    nzz[c] = fmaf(comp(d13, c), comp(B1, c), fmaf(comp(d33, c), comp(B2, c), nzz[c])) + comp(d35, c) * ab[c];
                    nxz[c] = fmaf(comp(d55, c), comp(B5, c), nxz[c]) + tb[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (has_inj) {
                    const float amp = inj[(j - tile_j) * TX + 4 * lx + c];
                    nxx[c] += amp;
                    nzz[c] += amp;
                }
                if (p.fsurf && j == 0) nzz[c] = 0.f;
            }
            st4(sxx + o, mk4(nxx));
            st4(szz + o, mk4(nzz));
            st4(sxz + o, mk4(nxz));
        }
        if (has_inj) __syncthreads();
    }
}

// dst += a b, component by component
__device__ __forceinline__ void tti_acc(float4 &dst, const float4 &a, const float4 &b)
{
    dst = make_float4(fmaf(a.x, b.x, dst.x), fmaf(a.y, b.y, dst.y), fmaf(a.z, b.z, dst.z), fmaf(a.w, b.w, dst.w));
}

// ================================================================================================
// adjoint, first launch of S^T: e_bar = C^T sigma_bar (the 3 x 3 operator is symmetric: the same form on the adjoint
// stresses) -> p.E, and the gradients of the six planes on stress nodes:
//   g_c11 += S0 sxx_bar;  g_c33 += S1 szz_bar;  g_c13 += S1 sxx_bar + S0 szz_bar;  g_c55 += S2 sxz_bar
//   g_c15 += sxx_bar A(w S2) + S0 A(w sxz_bar);  g_c35 += szz_bar A(w S2) + S1 A(w sxz_bar)
// Reads the adjoint stresses of neighbouring nodes and writes none: no barrier, no LDS.  Accumulators stay in registers
// across the shots of a group, as in el_adj_s.
// ================================================================================================
__global__ __launch_bounds__(kThreads) void tti_adj_e(const TtiParams p)
{
    constexpr int NACC = 8;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    const int t = (int)threadIdx.x;
    const int oj = by * ATZ + t / AGO, og = bx * AGO + t % AGO;
    if (oj >= p.nz || og >= p.ng) return;
    const unsigned fs = p.field_stride;
    const unsigned ncell = (unsigned)p.nz * p.gp;
    const long long sp = p.splane;
    const unsigned occ = (unsigned)oj * p.gp + 4 * og;
    const unsigned oo = (unsigned)(oj + 2) * p.pitch + 4 + 4 * og;
    const unsigned osc = snap_cell(p, oj, og);
    float *accg = p.acc + (long long)(p.s0 / p.gs + bz) * NACC * sp + osc;
    float4 g13 = ld4(accg + M_L * sp), g11 = ld4(accg + M_M * sp), g55 = ld4(accg + M_MU * sp);
    float4 g33 = ld4(accg + M_C33 * sp), g15 = ld4(accg + M_C15 * sp), g35 = ld4(accg + M_C35 * sp);
    const float4 c13 = ld4(p.mat + M_L * ncell + occ), c11 = ld4(p.mat + M_M * ncell + occ);
    const float4 c55 = ld4(p.mat + M_MU * ncell + occ), c33 = ld4(p.mat + M_C33 * ncell + occ);
    const float4 c15 = ld4(p.mat + M_C15 * ncell + occ), c35 = ld4(p.mat + M_C35 * ncell + occ);
    const TtiMask w = tti_mask(p, p.mat + M_MU * ncell, oj, og);
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        const float *fl = p.fields + (long long)s * p.shot_stride;
        const float *sxx = fl + F_SXX * fs, *szz = fl + F_SZZ * fs, *sxz = fl + F_SXZ * fs;
        const float4 bxx = ld4(sxx + oo), bxz = ld4(sxz + oo);
        float4 bzz = ld4(szz + oo);
        if (p.fsurf && oj == 0) bzz = make_float4(0.f, 0.f, 0.f, 0.f);        // adjoint of szz(0,.) is discarded
        const float *Sp = p.S + (long long)s * p.snap_shot;
        const float4 S1 = mifwi::ldnt4(Sp + osc), S2 = mifwi::ldnt4(Sp + sp + osc), S5 = mifwi::ldnt4(Sp + 2 * sp + osc);
        float ab[4], tb[4], aS[4];
        tti_A<kLayField>(p, sxz, w, oj, og, ab);
        tti_At<kLayField>(p, sxx, szz, p.mat + M_C15 * ncell, p.mat + M_C35 * ncell, w, oj, og, p.fsurf != 0, tb);
        tti_A<kLaySnap>(p, Sp + 2 * sp, w, oj, og, aS);
        float e1[4], e2[4], e5[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e1[c] = fmaf(comp(c11, c), comp(bxx, c), comp(c13, c) * comp(bzz, c)) + comp(c15, c) * ab[c];
            e2[c] = fmaf(comp(c13, c), comp(bxx, c), comp(c33, c) * comp(bzz, c)) + comp(c35, c) * ab[c];
            e5[c] = comp(c55, c) * comp(bxz, c) + tb[c];
        }
        float *Ep = p.E + (long long)s * p.e_shot + osc;
        st4(Ep, mk4(e1));
        st4(Ep + sp, mk4(e2));
        st4(Ep + 2 * sp, mk4(e5));
        const float4 ab4 = mk4(ab), aS4 = mk4(aS);
        tti_acc(g11, S1, bxx);
        tti_acc(g33, S2, bzz);
        tti_acc(g13, S1, bzz);
        tti_acc(g13, S2, bxx);
        tti_acc(g55, S5, bxz);
        tti_acc(g15, S1, ab4);
        tti_acc(g15, bxx, aS4);
        tti_acc(g35, S2, ab4);
        tti_acc(g35, bzz, aS4);
    }
    st4(accg + M_L * sp, g13); st4(accg + M_M * sp, g11); st4(accg + M_MU * sp, g55);
    st4(accg + M_C33 * sp, g33); st4(accg + M_C15 * sp, g15); st4(accg + M_C35 * sp, g35);
}

// the transposed C-PML on e1..e4 of one group, in place (memory variables written by the owner): the second half of
// stage_E, whose first half - C^T sigma_bar - is tti_adj_e's here
__device__ __forceinline__ void stage_E_pml(const ElParams &p, int s, int j, int g, bool mine, float e1[4], float e2[4],
                                            float e3[4], float e4[4])
{
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
}

// ================================================================================================
// adjoint, second launch of S^T: el_adj_s with the staged e_bar planes of tti_adj_e in place of C^T sigma_bar - the
// transposed C-PML (memory variables written by the owner), v_bar -= stencils(E), the adjoint sources of the tile, g_bx and
// g_bz from the new v_bar, and the sampling workgroups of grad_f.
// ================================================================================================
__global__ __launch_bounds__(kThreads, 3) void tti_adj_s(const TtiParams p)
{
    constexpr int NACC = 8;
    const FdK K = p.K;
    int bx, by, bz;
    xcd_tile(p, bx, by, bz);
    if (by >= p.tiles_z) {
        sample_points<1>(p, bx, by, bz);
        return;
    }
    __shared__ float E[4][ASZ][ASX];
    const int tile_j = by * ATZ;
    const int tile_g = bx * AGO;
    const unsigned fs = p.field_stride;
    const long long sp = p.splane;
    const int t = (int)threadIdx.x;
    const int orow = t / AGO, ogrp = t % AGO;
    const int oj = tile_j + orow, og = tile_g + ogrp;
    const bool own_ok = oj < p.nz && og < p.ng;
    const unsigned oo = (unsigned)(oj + 2) * p.pitch + 4 + 4 * og;
    const unsigned osc = own_ok ? snap_cell(p, oj, og) : 0u;
    int hr = 0, hg = 0;
    if (t < kHalo) halo_item(t, hr, hg);
    const int hj = tile_j - 2 + hr, hgg = tile_g - 1 + hg;
    const bool halo_ok = t < kHalo && hj >= 0 && hj < p.nz && hgg >= 0 && hgg < p.ng;
    const unsigned hsc = halo_ok ? snap_cell(p, hj, hgg) : 0u;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float *accg = p.acc + (long long)(p.s0 / p.gs + bz) * NACC * sp + osc;
    float4 gbx = zero4, gbz = zero4;
    if (own_ok) { gbx = ld4(accg + M_BX * sp); gbz = ld4(accg + M_BZ * sp); }
    for (int si = 0; si < p.gs; ++si) {
        const int s = p.s0 + bz * p.gs + si;
        if (s >= p.nshot) break;
        float *fl = p.fields + (long long)s * p.shot_stride;
        const float *Ep = p.E + (long long)s * p.e_shot;
        float4 vxb = zero4, vzb = zero4, S4 = zero4, S5 = zero4;
        float4 o1 = zero4, o2 = zero4, o5 = zero4, h1 = zero4, h2 = zero4, h5 = zero4;
        if (own_ok) {
            o1 = ld4(Ep + osc); o2 = ld4(Ep + sp + osc); o5 = ld4(Ep + 2 * sp + osc);
            vxb = ld4(fl + F_VX * fs + oo); vzb = ld4(fl + F_VZ * fs + oo);
        }
        if (halo_ok) { h1 = ld4(Ep + hsc); h2 = ld4(Ep + sp + hsc); h5 = ld4(Ep + 2 * sp + hsc); }
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
                    const float wt = p.inj_w[(long long)s * per + tap];
                    const long long ai = (long long)s * p.ninj + tap / p.ntap_inj;
                    atomicAdd(&E[0][j - tile_j + 2][i - 4 * tile_g + 4], wt * p.inj_amp0[ai]);
                    atomicAdd(&E[1][j - tile_j + 2][i - 4 * tile_g + 4], wt * p.inj_amp1[ai]);
                }
                __syncthreads();
                const float4 ix = ld4(&E[0][orow + 2][x]), iz = ld4(&E[1][orow + 2][x]);
                vxb = make_float4(vxb.x + ix.x, vxb.y + ix.y, vxb.z + ix.z, vxb.w + ix.w);
                vzb = make_float4(vzb.x + iz.x, vzb.y + iz.y, vzb.z + iz.z, vzb.w + iz.w);
                __syncthreads();
            }
        }
        // ---- stage E1..E4 on the tile + halo: the transposed C-PML on the e_bar planes -----------------------
        {
            float e1[4] = {o1.x, o1.y, o1.z, o1.w}, e2[4] = {o2.x, o2.y, o2.z, o2.w}, e3[4] = {o5.x, o5.y, o5.z, o5.w};
            float e4[4] = {o5.x, o5.y, o5.z, o5.w};
            if (own_ok) stage_E_pml(p, s, f_opaque(oj), f_opaque(og), true, e1, e2, e3, e4);
            const int x = 4 * (ogrp + 1);
            st4(&E[0][orow + 2][x], mk4(e1)); st4(&E[1][orow + 2][x], mk4(e2));
            st4(&E[2][orow + 2][x], mk4(e3)); st4(&E[3][orow + 2][x], mk4(e4));
        }
        if (t < kHalo) {
            float e1[4] = {h1.x, h1.y, h1.z, h1.w}, e2[4] = {h2.x, h2.y, h2.z, h2.w}, e3[4] = {h5.x, h5.y, h5.z, h5.w};
            float e4[4] = {h5.x, h5.y, h5.z, h5.w};
            if (halo_ok) stage_E_pml(p, s, f_opaque(hj), f_opaque(hgg), false, e1, e2, e3, e4);
            st4(&E[0][hr][4 * hg], mk4(e1)); st4(&E[1][hr][4 * hg], mk4(e2));
            st4(&E[2][hr][4 * hg], mk4(e3)); st4(&E[3][hr][4 * hg], mk4(e4));
        }
        if (own_ok) {
            const float *Sp = p.S + (long long)s * p.snap_shot;
            S4 = mifwi::ldnt4(Sp + 3 * sp + osc); S5 = mifwi::ldnt4(Sp + 4 * sp + osc);
        }
        __syncthreads();
        // ---- stencils from LDS, g_bx and g_bz from the new v_bar ----------------------------------------------
        if (own_ok) {
            const int r = orow + 2, cb = 4 * (ogrp + 1);
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
            st4(fl + F_VX * fs + oo, mk4(nvx));
            st4(fl + F_VZ * fs + oo, mk4(nvz));
            gbx = make_float4(fmaf(S4.x, nvx[0], gbx.x), fmaf(S4.y, nvx[1], gbx.y), fmaf(S4.z, nvx[2], gbx.z), fmaf(S4.w, nvx[3], gbx.w));
            gbz = make_float4(fmaf(S5.x, nvz[0], gbz.x), fmaf(S5.y, nvz[1], gbz.y), fmaf(S5.z, nvz[2], gbz.z), fmaf(S5.w, nvz[3], gbz.w));
        }
        __syncthreads();          // E is reused by the next shot
    }
    if (own_ok) { st4(accg + M_BX * sp, gbx); st4(accg + M_BZ * sp, gbz); }
}
