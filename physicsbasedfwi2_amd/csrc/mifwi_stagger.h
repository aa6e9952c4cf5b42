// The staggered-grid toolkit of the two velocity-stress families, mifwi_elastic.hip (P-SV: elastic, VTI, viscoelastic) and
// mifwi_fluid.hip (variable-density acoustic): everything below the cell arithmetic that the two schemes have in common.
// Device: the stencil and C-PML primitives, the strip lookups, the column-blocked snapshot offset, the adjoint tile with its
// row reader, the tile-major XCD order, and the three cold kernels (per-tile receiver lists, point-force sampling, the sum
// over the shot groups).  Host: the grid / pitch / C-PML strip geometry of a plan, the sizes that follow from the tile, the
// shots-per-group rule and the descriptor checks both create functions make.
// Helpers that read the parameter struct are templates on it: ElParams and FlParams keep their own field sets.
// What differs in substance stays in the two files: halo_item / kHalo, sample_points, the pressure kernels, stage_E /
// stage_D / stage_T, the bf16 planes - and stage_injection, whose two forms load in different orders: either one changes the
// other family's forward kernels.  The scalar acoustic scheme (mifwi_acoustic.hip) shares none of this.
#pragma once
#include "mifwi_host.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;    // workgroup of every per-step kernel of both families

// staggered-grid first-derivative weights (desc.fd_order): Taylor order 4 = (9/8, -1/24),
// order 2 = (1, 0) - the same four-point form, so every kernel serves both
struct FdK { float c1, c2; };
inline FdK fd_weights(int order)
{
    return order == 2 ? FdK{1.0f, 0.0f} : FdK{(float)(9.0 / 8.0), (float)(-1.0 / 24.0)};
}

// rows of the C-PML tables pz [6][nz] and px [6][gp]: a, b, 1/kappa at integer nodes, then at half nodes
enum { PA = 0, PB = 1, PK = 2, PAH = 3, PBH = 4, PKH = 5 };

__device__ __forceinline__ float comp(const float4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float2 ld2(const float *p) { return *reinterpret_cast<const float2 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 mk4(const float *a) { return make_float4(a[0], a[1], a[2], a[3]); }
__device__ __forceinline__ float dfw(const FdK &K, float fm1, float f0, float f1, float f2)   // Dp at "0"
{
    return fmaf(K.c1, f1 - f0, K.c2 * (f2 - fm1));
}
__device__ __forceinline__ float dbw(const FdK &K, float fm2, float fm1, float f0, float f1)  // Dm at "0"
{
    return fmaf(K.c1, f0 - fm1, K.c2 * (f1 - fm2));
}
// forward C-PML: psi <- b psi + a d ; returns d*ik + psi
__device__ __forceinline__ float pml(float &psi, float a, float b, float ik, float d)
{
    psi = fmaf(b, psi, a * d);
    return fmaf(d, ik, psi);
}
// transposed C-PML: P = psib + db ; returns ik*db + a*P ; psib <- b*P
__device__ __forceinline__ float pmlT(float psib, float a, float b, float ik, float db, float &psib_new)
{
    const float P = psib + db;
    psib_new = b * P;
    return fmaf(ik, db, a * P);
}

// x-strip column offset of group g (or -1)
template <class P>
__device__ __forceinline__ int xstrip(const P &p, int g)
{
    if (p.W == 0) return -1;
    const int c0 = 4 * g;
    if (c0 < p.wl) return c0;
    if (c0 >= p.xr0) return p.wl + (c0 - p.xr0);
    return -1;
}
// z-strip row index of row j (or -1)
template <class P>
__device__ __forceinline__ int zstrip(const P &p, int j)
{
    if (p.W == 0) return -1;
    if (j < p.W) return j;
    if (j >= p.nz - p.W) return j - (p.nz - 2 * p.W);
    return -1;
}

// Offset (floats) of group g of row j inside a snapshot / accumulator plane blocked by columns of 16 groups:
// [g / 16][j][64 floats].  Every per-step kernel works on tiles 16 groups wide, so a tile row is 256 contiguous,
// 256-byte aligned bytes of the plane and consecutive rows follow each other: whole 128-byte lines on the way out
// and on the way back in.  (Row-major rows are gp * 4 bytes apart, not a multiple of 128 in general: a 256-byte tile
// row straddles three lines, and the elastic adjoint read 33 B per cell-step of the 20 B snapshot stream.)
__device__ __forceinline__ unsigned snap_cell_blocked(int nz, int j, int g)
{
    return ((unsigned)(g >> 4) * (unsigned)nz + (unsigned)j) * 64u + 4u * (unsigned)(g & 15);
}

// Workgroups are dealt to the 8 XCDs round-robin in launch order, each XCD with an L2 of its own: with the plain
// blockIdx -> tile map, neighbouring tiles never share an L2 and every halo row / column is fetched from memory again.
// Tile-major remap (a bijection on the launch grid): the sequence (tile 0: slices 0 .. gz-1), (tile 1: ...), ... is cut
// into eight contiguous pieces, one per XCD - all shots of the launch pass through a tile back to back on ONE XCD, so the
// tile's material planes come from memory once per launch, not once per shot (grids whose planes outgrow the L2s: 60 MB
// of elastic planes at 1000x3000), and neighbouring tiles follow each other on that XCD (the halo a tile reads was
// fetched by the same L2).
__device__ __forceinline__ unsigned xcd_tile_major_index(int &bz)      // the tile's number, row-major
{
    const unsigned gx = gridDim.x, n2 = gx * gridDim.y, gz = gridDim.z, total = n2 * gz;
    const unsigned L = blockIdx.x + gx * blockIdx.y + n2 * blockIdx.z;
    const unsigned c = L & 7u, idx = L >> 3, q = total >> 3, r = total & 7u;
    const unsigned e = c * q + (c < r ? c : r) + idx;
    const unsigned T = e / gz;
    bz = (int)(e - T * gz);
    return T;
}
__device__ __forceinline__ void xcd_tile_major(int &bx, int &by, int &bz)
{
    const unsigned gx = gridDim.x, T = xcd_tile_major_index(bz);
    by = (int)(T / gx); bx = (int)(T - (unsigned)by * gx);
}

// ---- the adjoint tile: ATZ x (4*AGO) owned cells, staged on (ATZ+4) x 4*(AGO+2) in LDS --------------------------
// (tests/cases.py ADJ_TILE restates ATZ and 4 * AGO; the per-tile receiver lists below are cut by them)
constexpr int ATZ = 16;          // owned rows
constexpr int AGO = 16;          // owned groups per row: a quarter wave reads one contiguous LDS row
constexpr int AGX = AGO + 2;     // staged groups per row (1 halo group each side)
constexpr int ASZ = ATZ + 4;     // staged rows
constexpr int ASX = 4 * AGX;     // staged columns (72 floats: consecutive rows start 8 banks apart)
static_assert(ATZ * AGO == kThreads, "one owned 4-cell group per thread");

// x stencils on the 8 values {L.z, L.w, C.x .. C.w, R.x, R.y} around an owned group
struct Row8 { float v[8]; };
__device__ __forceinline__ Row8 row8(const float *row, int cb)
{
    const float4 l = ld4(row + cb - 4), c = ld4(row + cb), r = ld4(row + cb + 4);
    return Row8{{l.z, l.w, c.x, c.y, c.z, c.w, r.x, r.y}};
}

// Receiver taps (adjoint sources) of every tile of the S^T / P^T launch, one block per shot: start[s][tile .. tile+1)
// indexes list[s][], which holds tap numbers (receiver * ntap + tap) sorted by tile, ascending inside a tile.  Built once
// per backward call; the time loop then adds v_bar += R^T g inside that launch, by the tile that owns the cells
// (workgroup-uniform branch, taken by the few tiles that hold receivers), instead of a launch of its own per step
// and shot pass (4.7 us each: 5 % of a step where the passes are small, e.g. the chunks of a shot-chunked gradient).
__global__ void build_tile_taps(const int *cell, int ntaps, int nx, int tx, int ntiles, int *start, int *cursor, int *list)
{
    const int s = (int)blockIdx.x, t = (int)threadIdx.x, T = (int)blockDim.x;
    start += (long long)s * (ntiles + 1); cursor += (long long)s * ntiles; list += (long long)s * ntaps;
    cell += (long long)s * ntaps;
    for (int k = t; k < ntiles; k += T) cursor[k] = 0;
    __syncthreads();
    auto tile_of = [&](int c) { const int j = c / nx, i = c - j * nx; return (j / ATZ) * tx + (i >> 2) / AGO; };
    for (int e = t; e < ntaps; e += T)
        if (cell[e] >= 0) atomicAdd(cursor + tile_of(cell[e]), 1);
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < ntiles; ++k) { start[k] = run; run += cursor[k]; cursor[k] = start[k]; }
        start[ntiles] = run;
    }
    __syncthreads();
    for (int e = t; e < ntaps; e += T)
        if (cell[e] >= 0) list[atomicAdd(cursor + tile_of(cell[e]), 1)] = e;
    __syncthreads();
    for (int k = t; k < ntiles; k += T)                   // ascending tap order inside a tile (a few entries each)
        for (int a = start[k] + 1; a < start[k + 1]; ++a) {
            const int v = list[a];
            int b = a - 1;
            while (b >= start[k] && list[b] > v) { list[b + 1] = list[b]; --b; }
            list[b + 1] = v;
        }
}

// adjoint of a point force: grad_f[n] = sum w v_bar[cell] of field `field` (F_VX | F_VZ), sampled between the two adjoint
// launches of a step
template <class P>
__global__ void sample_force(const P p, int field)
{
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);     // over the p.gs shots of this pass
    if (idx >= p.gs * p.nsmp) return;
    const int s = p.s0 + idx / p.nsmp;
    if (s >= p.nshot) return;
    const int e = s * p.nsmp + idx % p.nsmp;
    const float *v = p.fields + (long long)s * p.shot_stride + field * (long long)p.field_stride;
    float a = 0.f;
    for (int t = 0; t < p.ntap_smp; ++t) {
        const long long ee = (long long)e * p.ntap_smp + t;
        const int cell = p.smp_cell[ee];
        if (cell < 0) continue;
        const int j = cell / p.nx, i = cell - j * p.nx;
        a = fmaf(p.smp_w[ee], v[(unsigned)(j + 2) * p.pitch + 4 + i], a);
    }
    p.smp_out0[e] = a;
}

// grad[k][cell] = sum over shot groups of acc[group][k][cell], in group order; grad is row-major [NP][nz][gp] (the C-ABI's
// layout), the accumulator planes are `aplane` floats apart and column-blocked when sblk (snap_cell_blocked)
template <int NP>
__global__ void finalize_groups(const float *acc, int ngroups, int nz, int gp, long long aplane, int sblk, float *grad)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, ncell = (long long)nz * gp;
    if (idx >= NP * ncell) return;
    const int k = (int)(idx / ncell);
    const long long c = idx - (long long)k * ncell;
    const int j = (int)(c / gp), i = (int)(c - (long long)j * gp), g = i >> 2;
    const long long off = sblk ? ((long long)(g >> 4) * nz + j) * 64 + 4 * (g & 15) + (i & 3) : c;
    float a = 0.f;
    for (int gidx = 0; gidx < ngroups; ++gidx) a += acc[((long long)gidx * NP + k) * aplane + off];
    grad[idx] = a;
}

// ---- plan time (host, plain arithmetic) ----------------------------------------------------------------------
// Grid, row pitch and C-PML strip geometry of a plan.  A row holds ng groups of 4 cells (gp cells); a field plane has two
// halo rows above and below and four halo cells left of a row.  The memory variables live in compact strips of
// W = pml_width + 1 nodes per side (half-node profiles reach one node further): x strips wx columns wide (the left one
// rounded up to whole groups, the right one from the group that holds the first layer cell), z strips 2W rows.
struct StaggerGrid {
    int ng, gp, pitch;
    int W, wl, xr0, wx;                 // W = 0: no layer
    long long field_stride;             // (nz+4)*pitch
    long long coef_elems;               // nz*gp: one material / gradient plane
    long long psix_shot, psiz_shot;     // floats per shot: psi_planes*nz*wx, psi_planes*2W*gp
};
// psi_planes: memory variables per strip cell (elastic 4, fluid 2)
inline int stagger_grid(int nz, int nx, int pml_width, int psi_planes, StaggerGrid *g)
{
    g->ng = mifwi::ceil_div(nx, 4);
    g->gp = 4 * g->ng;
    g->pitch = (int)mifwi::round_up64(4 * (g->ng + 3), 32);
    g->field_stride = (long long)(nz + 4) * g->pitch;
    g->coef_elems = (long long)nz * g->gp;
    g->W = pml_width > 0 ? pml_width + 1 : 0;
    g->wl = g->xr0 = g->wx = 0;
    if (g->W > 0) {
        g->wl = (int)mifwi::round_up64(g->W, 4);
        g->xr0 = ((nx - g->W) / 4) * 4;
        if (g->xr0 < g->wl || 2 * g->W > nz)
            return mifwi::fail(MIFWI_EINVAL, "grid %dx%d too small for a %d-node C-PML", nz, nx, pml_width);
        g->wx = g->wl + (g->gp - g->xr0);
    }
    g->psix_shot = (long long)psi_planes * nz * g->wx;
    g->psiz_shot = (long long)psi_planes * 2 * g->W * g->gp;
    return MIFWI_OK;
}

// floats of one column-blocked snapshot / accumulator plane (snap_cell_blocked)
inline long long blocked_plane_elems(int nz, int ng) { return 64LL * nz * mifwi::ceil_div(ng, 16); }

// floats (holding ints) of build_tile_taps' region: start [nshot][ntiles + 1], cursor [nshot][ntiles], list [nshot][nrec * ntap]
inline long long tile_taps_elems(int nshot, int nz, int ng, int nrec, int ntap)
{
    const long long ntiles = (long long)mifwi::ceil_div(ng, AGO) * mifwi::ceil_div(nz, ATZ);
    return std::max<long long>(1024, mifwi::round_up64(nshot * (2 * ntiles + 1 + (long long)nrec * ntap), 64));
}

// Shots per accumulator group: the caller's, else `env_default`; at least 1 and at most nshot.  A default of 4 gives way
// to groups of equal size where a slightly smaller one gives them (a 6-shot chunk of a shot-chunked gradient pass: 3 + 3
// instead of 4 + 2 - the workgroups of the short group would idle while the others finish their fourth shot).
inline int default_group_size(int shots_per_group, int nshot, int env_default)
{
    int gs = shots_per_group > 0 ? shots_per_group : env_default;
    if (gs <= 0) gs = 1;
    if (gs > nshot) gs = nshot;
    if (shots_per_group <= 0 && gs == 4 && nshot % 4 != 0 && nshot % 3 == 0) gs = 3;
    return gs;
}

// The descriptor checks both create functions make, in two runs (elastic checks record_pressure between them, and the
// order of the refusals is part of the behaviour).  min_fs_nz: rows a free surface needs (its mirrored rows).
template <class Desc>
int check_stagger_desc(const Desc *d, int min_fs_nz)
{
    if (d->nz < 1 || d->nx < 1 || d->nt < 1 || d->nshot < 1 || d->nsrc < 0 || d->nrec < 0)
        return mifwi::fail(MIFWI_EINVAL, "bad sizes nz=%d nx=%d nt=%d nshot=%d", d->nz, d->nx, d->nt, d->nshot);
    if (d->ntap != 1 && d->ntap != 4) return mifwi::fail(MIFWI_EINVAL, "ntap must be 1 or 4");
    if (d->free_surface != 0 && d->free_surface != 1) return mifwi::fail(MIFWI_EINVAL, "free_surface must be 0 or 1");
    if (d->free_surface && d->nz < min_fs_nz) return mifwi::fail(MIFWI_EINVAL, "free surface needs nz >= %d", min_fs_nz);
    if (d->pml_width < 0) return mifwi::fail(MIFWI_EINVAL, "pml_width < 0");
    return MIFWI_OK;
}
template <class Desc>
int check_stagger_scheme(const Desc *d)
{
    if (d->source_type < 0 || d->source_type > 2)
        return mifwi::fail(MIFWI_EINVAL, "source_type must be 0 (explosive), 1 (force x) or 2 (force z)");
    if (d->fd_order != 0 && d->fd_order != 2 && d->fd_order != 4)
        return mifwi::fail(MIFWI_EINVAL, "fd_order %d: the staggered-grid stencils are built for order 2 and 4", d->fd_order);
    return MIFWI_OK;
}

}  // namespace
