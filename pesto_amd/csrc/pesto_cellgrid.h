// pesto_cellgrid.h - the float32 uniform cell grid of the project's neighbour searches: the contact searches (interface labels,
// pesto_eval.hip; dataset contacts, pesto_contacts.hip), lDDT's reference list (pesto_lddt.hip), the elastic network's spring list (pesto_enm.hip), the receptor's grid of the pose scoring (pesto_poses.hip, which walks the rows with a wave) and the k-NN topology (pesto_knn.hip);
// and torch.norm's distance. The scans: pesto_scan.h.
//
// The contact searches replace the reference's dense torch distance matrix per pair of subunits (locate_contacts / extract_all_contacts,
// src/data_encoding.py:116-176): every atom pair of two subunits of one assembly with |x_a - x_b| < r_thr, the distance being the
// reference's fp32 torch.norm (dist()). Each assembly of the batch gets a grid of its own:
//   - cells at least r_thr * 1.001 wide, so a pair within r_thr is never more than one cell apart, whatever the rounding of the cell
//     coordinates: the searching atom walks the 3 x 3 rows of three consecutive cells around it (for_each_neighbour) and misses nobody.
//     Whoever changes the cell edge, cell3() or the walk changes this argument for the contact searches AND lDDT, and the completeness
//     radius of the k-NN (k_knn_collate walks blocks of cells of its own on top of cell3() and derives the edge from inv_h);
//   - at most 64 cells per axis and 2 N_s + 64 cells in all (the edge grows by h *= 1.25f until they fit), so the cell arrays of a batch
//     are sized from the atom count alone: assembly s owns the cells from cells_before(off_s, s), one more than it uses (the total behind
//     its last cell), and a batch needs cells_before(n_total, n_struct);
//   - one cell (every pair is examined, inv_h = 0) when the bounding box is not finite: an atom with a NaN coordinate is farther than
//     r_thr from everybody, itself included, in every comparison.
// Build: grid_build() = k_grid_setup -> k_grid_count -> k_grid_scan -> k_grid_scatter, four launches over the five buffers of GridBufs;
// the users differ in what they check per atom in the count pass and in the payload they scatter beside the coordinates, both functors.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "pesto_scan.h"

namespace pesto {

namespace {

constexpr int GRID_MAX = 64;              // cells per axis at most
struct CellGrid { float minx, miny, minz, inv_h; int nx, ny, nz, base; };

// cells of the assemblies before s (off_s atoms), and of a whole batch for (n_total, n_struct): 2 N_s + 64 and the total slot each
__host__ __device__ inline size_t cells_before(size_t off_s, size_t s) { return 2 * off_s + 65 * s; }

__device__ __forceinline__ void cell3(const CellGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(g.nx - 1, max(0, (int)((x - g.minx) * g.inv_h)));
    cy = min(g.ny - 1, max(0, (int)((y - g.miny) * g.inv_h)));
    cz = min(g.nz - 1, max(0, (int)((z - g.minz) * g.inv_h)));
}

// torch.norm's float32 length of a difference vector: sqrt(fma(z, z, fma(y, y, x * x))), every step rounded as written (the build
// contracts only within a source expression, so the chain is spelled out rather than left to the compiler). The one chain of the contact
// searches (dist) and of the k-NN's keys (knn_key)
__device__ __forceinline__ float norm3(float rx, float ry, float rz) {
    return sqrtf(__fmaf_rn(rz, rz, __fmaf_rn(ry, ry, __fmul_rn(rx, rx))));
}
__device__ __forceinline__ float dist(float4 a, float4 b) { return norm3(b.x - a.x, b.y - a.y, b.z - a.z); }

// for the users that check nothing in the count pass / keep nothing beside the coordinates
struct NoCheck { __device__ void operator()(int, int) const {} };
struct NoPayload { __device__ void operator()(int, int) const {} };

// one workgroup per assembly: bounding box -> cell size and counts, cleared cell counters
__global__ __launch_bounds__(256) void k_grid_setup(int n_struct, const int* __restrict__ offsets, const float* __restrict__ X, float r_thr,
                                                    CellGrid* __restrict__ grids, int* __restrict__ cell_cnt) {
    const int s = blockIdx.x;
    const int s0 = offsets[s], s1 = offsets[s + 1];
    __shared__ float red[6][256];
    __shared__ CellGrid gsh;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = s0 + threadIdx.x; i < s1; i += 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = X[3 * (size_t)i + c]; mn[c] = fminf(mn[c], v); mx[c] = fmaxf(mx[c], v); }
#pragma unroll
    for (int c = 0; c < 3; ++c) { red[c][threadIdx.x] = mn[c]; red[3 + c][threadIdx.x] = mx[c]; }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                red[c][threadIdx.x] = fminf(red[c][threadIdx.x], red[c][threadIdx.x + off]);
                red[3 + c][threadIdx.x] = fmaxf(red[3 + c][threadIdx.x], red[3 + c][threadIdx.x + off]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        CellGrid g;
        g.base = (int)cells_before((size_t)s0, (size_t)s);
        g.minx = red[0][0]; g.miny = red[1][0]; g.minz = red[2][0];
        g.nx = g.ny = g.nz = 1; g.inv_h = 0.f;                 // one cell (every pair is examined): non-finite coordinates
        const float ex = red[3][0] - red[0][0], ey = red[4][0] - red[1][0], ez = red[5][0] - red[2][0];
        const float ext = fmaxf(ex, fmaxf(ey, ez));
        if (ext == ext && ext < 1e30f && g.minx == g.minx && g.miny == g.miny && g.minz == g.minz) {
            const long long cap = 2LL * (s1 - s0) + 64;
            float h = fmaxf(r_thr * 1.001f, ext / (float)GRID_MAX * 1.0001f);
            for (;;) {
                const int nx = (int)(ex / h) + 1, ny = (int)(ey / h) + 1, nz = (int)(ez / h) + 1;
                if ((long long)nx * ny * nz <= cap) { g.nx = nx; g.ny = ny; g.nz = nz; g.inv_h = 1.0f / h; break; }
                h *= 1.25f;
            }
        }
        grids[s] = g;
        gsh = g;
    }
    __syncthreads();
    const int nc = gsh.nx * gsh.ny * gsh.nz;
    for (int c = threadIdx.x; c <= nc; c += 256) cell_cnt[gsh.base + c] = 0;
}

// cell of every atom, cell counts; check(i, s) is the user's own look at atom i of assembly s (the pass reads every atom anyway)
template <class Check>
__global__ __launch_bounds__(256) void k_grid_count(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                    const CellGrid* __restrict__ grids, int* __restrict__ cell_cnt, int* __restrict__ cell_of,
                                                    Check check) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int s = struct_of(i, n_struct, offsets);
    check(i, s);
    const CellGrid g = grids[s];
    int cx, cy, cz;
    cell3(g, X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], cx, cy, cz);
    const int c = (cz * g.ny + cy) * g.nx + cx;
    cell_of[i] = c;
    atomicAdd(&cell_cnt[g.base + c], 1);
}

// exclusive scan of one assembly's cell counts (one workgroup per assembly) -> cell starts (local atom positions), cursor copy
__global__ __launch_bounds__(1024) void k_grid_scan(const CellGrid* __restrict__ grids, int* __restrict__ cell_cnt, int* __restrict__ cell_cur) {
    const CellGrid g = grids[blockIdx.x];
    const int nc = g.nx * g.ny * g.nz;
    const int total = block_scan_exclusive<1024, true>(cell_cnt + g.base, nc, cell_cur + g.base);
    if (threadIdx.x == 1023) cell_cnt[g.base + nc] = total;
}

// atoms in cell order: (x, y, z, batch index) in sorted[pos], and whatever payload(pos, i) keeps beside them
template <class Payload>
__global__ __launch_bounds__(256) void k_grid_scatter(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                      const CellGrid* __restrict__ grids, const int* __restrict__ cell_of,
                                                      int* __restrict__ cell_cur, float4* __restrict__ sorted, Payload payload) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int s = struct_of(i, n_struct, offsets);
    const int pos = offsets[s] + atomicAdd(&cell_cur[grids[s].base + cell_of[i]], 1);
    sorted[pos] = make_float4(X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], __int_as_float(i));
    payload(pos, i);
}

// the five device buffers of a batch's grids: grids [n_struct], cell_cnt / cell_cur [cells_before(n_total, n_struct)] (cell_cnt ends up as
// the cell starts), cell_of [n_total], sorted [n_total]
struct GridBufs { CellGrid* grids; int* cell_cnt; int* cell_cur; int* cell_of; float4* sorted; };

// the build, host side: the grids of every assembly for cells of at least r_thr * 1.001, the atoms in cell order in b.sorted
template <class Check, class Payload>
void grid_build(hipStream_t st, int n_total, int n_struct, const int* offsets, const float* X, float r_thr, const GridBufs& b, Check check,
                Payload payload) {
    const dim3 atoms((n_total + 255) / 256), structs(n_struct);
    const CellGrid* g = b.grids;
    hipLaunchKernelGGL(k_grid_setup, structs, dim3(256), 0, st, n_struct, offsets, X, r_thr, b.grids, b.cell_cnt);
    hipLaunchKernelGGL(k_grid_count<Check>, atoms, dim3(256), 0, st, n_total, n_struct, offsets, X, g, b.cell_cnt, b.cell_of, check);
    hipLaunchKernelGGL(k_grid_scan, structs, dim3(1024), 0, st, g, b.cell_cnt, b.cell_cur);
    hipLaunchKernelGGL(k_grid_scatter<Payload>, atoms, dim3(256), 0, st, n_total, n_struct, offsets, X, g, (const int*)b.cell_of, b.cell_cur,
                       b.sorted, payload);
}

// visit(j) for every sorted position j of the 3 x 3 rows of three consecutive cells around atom a of the assembly whose atoms start at
// s0 (each row one contiguous range of the sorted atoms; a itself is among them)
template <class Visit>
__device__ __forceinline__ void for_each_neighbour(const CellGrid g, const int* __restrict__ cell_start, int s0, float4 a, Visit visit) {
    const int* start = cell_start + g.base;
    int cx, cy, cz;
    cell3(g, a.x, a.y, a.z, cx, cy, cz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const int row = (z * g.ny + y) * g.nx;
            const int j1 = s0 + start[row + x1 + 1];
            for (int j = s0 + start[row + x0]; j < j1; ++j) visit(j);
        }
}

}  // namespace
}  // namespace pesto
