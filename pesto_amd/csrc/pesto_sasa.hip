// pesto_sasa.hip - solvent-accessible surface area (Shrake-Rupley) of every atom of every frame / structure of a launch.
//
// replaces: md.shrake_rupley as the reference calls it - over every structure of a store (interfaceome/solvent_accessible_surface_area.py,
// wrapper_solvent_accessible_surface_area) and frame by frame in a Python loop (md_analysis/mdtraj_utils/trajectory_utils.py:428-438, sasa).
//
// Definition (X float32 [F,N,3]; R float32 [N] = atomic + probe radius; S float32 [P,3] sphere points; structures = ranges of atoms).
// Every operation is rounded to float32 on its own, as written, no fused multiply-add:
//     t[c]          = X[f,i,c] + (R[i] * S[k,c])
//     d[c]          = t[c] - X[f,j,c]
//     q(f,i,k,j)    = (d.x*d.x + d.y*d.y) + d.z*d.z
//     buried(f,i,k) = some j != i of i's structure, with finite X[f,j] and R[j], has q < R[j]*R[j]
//     count[f,i]    = number of k in [0, P) that are not buried
//     area[f,i]     = float32(((c0 * count) * R[i]) * R[i])    in double
//     group[f,g]    = float32(sum of the double areas of the atoms of group g, in atom order)
// A comparison with a NaN is false, so an atom with a non-finite coordinate or radius has count = P; it also buries nothing (it stays out of
// the grid). Coincident atoms are no error. count is an integer that does not depend on the order of the occluders, on the other structures
// of the launch or on the pruning below, so every output is bit-identical from call to call.
//
// The pruning margin. Write u = 2^-24, sigma = max_k |S[k]| (Euclidean, evaluated in double; 1 to a few u for unit points), and let j bury
// point k of i: q < fl(R_j^2) <= R_j^2 (1 + u). Each d_c^2 reaches q through three roundings (product, two sums), so
// sum d_c^2 <= q / (1 - u)^3, and d_c = (t_c - X_jc)(1 + e), |e| <= u: the computed point t lies within R_j (1 + 5u) of X_j. t itself is
// X_i + R_i S_k with two roundings per component: |t - X_i| <= |R_i| sigma (1 + 2u) + u |t|, |t| <= |X_i| + |R_i| sigma (1 + 2u). Hence
//     |X_i - X_j| <= (|R_i| sigma + |R_j|)(1 + 5u) + 2u |X_i|  <  B_ij = (|R_i| sigma + |R_j|)(1 + 2^-18) + 2^-20 (|x_i| + |y_i| + |z_i|) + 1e-18
// (the last term covers products that underflow). Whoever is farther than B_ij from i - the distance evaluated in double, where the
// differences of float32 coordinates are exact to 2^-53 - buries no point of i, whatever the float32 roundings: that is the test that
// compacts the candidates. The grid's cell edge is at least max B_ij of the structure, (max|R| (sigma + 1))(1 + 2^-16) + 3 * 2^-18 max|X_c|
// + 1e-18 (cells are found in double, with a relative slack of 1e-9 for that division), so every j that passes lies in the 27 cells around i.
//
// Kernels: sigma of the points; per (frame, structure) a bounding box and a grid (k_sasa_setup), count -> scan -> scatter of (x, y, z, R)
// records in cell order like the k-NN grid of pesto_kernels.hip; the point pass (k_sasa_points: a wave per atom, candidates compacted to
// (x, y, z, R^2) in LDS, lane = points lane + 64 m, broadcast reads, ballot exit); areas and group sums in double.
// Developer hook: the environment variable PESTO_SASA_DEBUG is read per call, bit 0 = stop after the grid build (timing), bit 1 = do not
// try the lane's last occluder first (timing of that choice; the results do not depend on it).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pesto_call.h"
#include "pesto_scan.h"

namespace pesto {

namespace {

constexpr int NT = 256;             // threads per workgroup of every kernel here
constexpr int WAVES = NT / 64;      // point pass: atoms per workgroup
constexpr int TILE = 256;           // point pass: candidate records per wave in LDS (a longer list goes through in tiles)
constexpr int MU = 4;               // point pass: points a lane tests side by side against one broadcast record
constexpr int MB = 64;              // point pass: points per lane whose state one 64-bit mask holds (P <= 4096: one block)
constexpr int MAX_CELLS = 32768;    // cells per (frame, structure); never more than the structure has atoms

struct SasaGrid { double minx, miny, minz, inv_h; int nx, ny, nz, any; };

__device__ __forceinline__ bool finite4(float x, float y, float z, float r) {
    return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX && fabsf(r) <= FLT_MAX;
}

__device__ __forceinline__ int cell_axis(double x, double mn, double inv_h, int n) { return min(n - 1, max(0, (int)((x - mn) * inv_h))); }

// sigma[0] = max(1, max_k |S_k|) in double over the finite points (one workgroup). A point with a NaN or infinite component is skipped: its
// t and q are NaN or infinite for every atom, so no comparison with it is true whatever is pruned.
__global__ __launch_bounds__(NT) void k_sasa_sigma(int P, const float* __restrict__ S, double* __restrict__ sigma) {
    __shared__ double red[NT];
    double m = 1.0;
    for (int k = threadIdx.x; k < P; k += NT) {
        const float x = S[3 * k], y = S[3 * k + 1], z = S[3 * k + 2];
        if (finite4(x, y, z, 0.f)) m = fmax(m, (double)x * x + (double)y * y + (double)z * z);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) sigma[0] = sqrt(red[0]) * (1.0 + 1e-15);
}

// one workgroup per (frame, structure): bounding box, max |R| and max |coordinate| of the finite atoms, the grid, zeroed cell counts
__global__ __launch_bounds__(NT) void k_sasa_setup(int n_struct, int n_total, const int* __restrict__ offsets, const int* __restrict__ capoff,
                                                   int total_cap, const float* __restrict__ X, const float* __restrict__ radius,
                                                   const double* __restrict__ sigma, SasaGrid* __restrict__ grids, int* __restrict__ cell_cnt) {
    __shared__ float red[8][NT];
    __shared__ SasaGrid gsh;
    const int g = blockIdx.x, f = g / n_struct, s = g % n_struct;
    const int s0 = offsets[s], s1 = offsets[s + 1];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, rm = 0.f, am = 0.f;
    for (int i = s0 + threadIdx.x; i < s1; i += NT) {
        const float* p = X + ((size_t)f * n_total + i) * 3;
        const float x = p[0], y = p[1], z = p[2], r = radius[i];
        if (!finite4(x, y, z, r)) continue;
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        rm = fmaxf(rm, fabsf(r));
        am = fmaxf(am, fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { red[c][threadIdx.x] = mn[c]; red[3 + c][threadIdx.x] = -mx[c]; }
    red[6][threadIdx.x] = -rm;
    red[7][threadIdx.x] = -am;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {          // eight minima (maxima negated): the same result in any order
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int c = 0; c < 8; ++c) red[c][threadIdx.x] = fminf(red[c][threadIdx.x], red[c][threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        SasaGrid q;
        q.minx = q.miny = q.minz = 0.0; q.inv_h = 0.0; q.nx = q.ny = q.nz = 1; q.any = 0;
        if (red[0][0] <= FLT_MAX) {                         // at least one finite atom
            const int cap = capoff[s + 1] - capoff[s] - 1;
            const double ex = (double)-red[3][0] - (double)red[0][0], ey = (double)-red[4][0] - (double)red[1][0],
                         ez = (double)-red[5][0] - (double)red[2][0];
            // the margin argument at the top of the file; a structure whose cells exceed its bound gets larger cells
            double h = ((double)-red[6][0] * (sigma[0] + 1.0)) * (1.0 + 0x1p-16) + 3.0 * 0x1p-18 * (double)-red[7][0] + 1e-18;
            double nx = 1.0, ny = 1.0, nz = 1.0;
            for (int it = 0; it < 4096; ++it) {             // (h is finite and positive: float32 inputs, finite sigma; 1.26^4096 covers any extent)
                nx = floor(fmin(ex / h, 1e6)) + 1.0; ny = floor(fmin(ey / h, 1e6)) + 1.0; nz = floor(fmin(ez / h, 1e6)) + 1.0;
                if (nx * ny * nz <= (double)cap) break;
                h *= 1.26;
            }
            if (!(nx * ny * nz <= (double)cap)) { nx = ny = nz = 1.0; h = INFINITY; }     // one cell: always right
            q.minx = (double)red[0][0]; q.miny = (double)red[1][0]; q.minz = (double)red[2][0];
            q.inv_h = (1.0 - 1e-9) / h;
            q.nx = (int)nx; q.ny = (int)ny; q.nz = (int)nz; q.any = 1;
        }
        grids[g] = q;
        gsh = q;
    }
    __syncthreads();
    const int nc = gsh.nx * gsh.ny * gsh.nz;
    int* cnt = cell_cnt + (size_t)f * total_cap + capoff[s];
    for (int c = threadIdx.x; c <= nc; c += NT) cnt[c] = 0;
}

// one thread per (frame, atom): its cell (-1 for an atom with non-finite data, which stays out of the grid), counted
__global__ __launch_bounds__(NT) void k_sasa_count(size_t total, int n_struct, int n_total, const int* __restrict__ offsets,
                                                   const int* __restrict__ capoff, int total_cap, const float* __restrict__ X,
                                                   const float* __restrict__ radius, const SasaGrid* __restrict__ grids,
                                                   int* __restrict__ cell_cnt, int* __restrict__ cell_of) {
    const size_t a = (size_t)blockIdx.x * NT + threadIdx.x;
    if (a >= total) return;
    const int f = (int)(a / (size_t)n_total), i = (int)(a % (size_t)n_total);
    const float x = X[3 * a], y = X[3 * a + 1], z = X[3 * a + 2];
    int c = -1;
    if (finite4(x, y, z, radius[i])) {
        const int s = struct_of(i, n_struct, offsets);
        const SasaGrid g = grids[(size_t)f * n_struct + s];
        c = (cell_axis(z, g.minz, g.inv_h, g.nz) * g.ny + cell_axis(y, g.miny, g.inv_h, g.ny)) * g.nx + cell_axis(x, g.minx, g.inv_h, g.nx);
        atomicAdd(&cell_cnt[(size_t)f * total_cap + capoff[s] + c], 1);
    }
    cell_of[a] = c;
}

// exclusive scan of the cell counts of one (frame, structure): cnt -> first slot of each cell (and the total behind the last), cursor copy
__global__ __launch_bounds__(NT) void k_sasa_scan(int n_struct, const int* __restrict__ capoff, int total_cap, const SasaGrid* __restrict__ grids,
                                                  int* __restrict__ cell_cnt, int* __restrict__ cell_cur) {
    const int g = blockIdx.x, f = g / n_struct, s = g % n_struct;
    const int nc = grids[g].nx * grids[g].ny * grids[g].nz;
    int* cnt = cell_cnt + (size_t)f * total_cap + capoff[s];
    const int total = block_scan_exclusive<NT, true>(cnt, nc, cell_cur + (size_t)f * total_cap + capoff[s]);
    if (threadIdx.x == NT - 1) cnt[nc] = total;
}

// (x, y, z, R) records in cell order; the order inside a cell is that of the atomics and may vary, which no result depends on
__global__ __launch_bounds__(NT) void k_sasa_scatter(size_t total, int n_struct, int n_total, const int* __restrict__ offsets,
                                                     const int* __restrict__ capoff, int total_cap, const float* __restrict__ X,
                                                     const float* __restrict__ radius, const int* __restrict__ cell_of,
                                                     int* __restrict__ cell_cur, float4* __restrict__ sorted, int* __restrict__ pos_of) {
    const size_t a = (size_t)blockIdx.x * NT + threadIdx.x;
    if (a >= total) return;
    const int c = cell_of[a];
    if (c < 0) return;
    const int f = (int)(a / (size_t)n_total), i = (int)(a % (size_t)n_total);
    const int s = struct_of(i, n_struct, offsets);
    const int pos = atomicAdd(&cell_cur[(size_t)f * total_cap + capoff[s] + c], 1);      // < the structure's number of finite atoms
    sorted[(size_t)f * n_total + offsets[s] + pos] = make_float4(X[3 * a], X[3 * a + 1], X[3 * a + 2], radius[i]);
    pos_of[a] = pos;
}

// the float32 test of the definition: does the occluder (x, y, z, R^2) bury the point t
__device__ __forceinline__ bool buries(float tx, float ty, float tz, const float4 c) {
    const float dx = __fsub_rn(tx, c.x), dy = __fsub_rn(ty, c.y), dz = __fsub_rn(tz, c.z);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) < c.w;
}

// One wave per (frame, atom). The candidates of the 27 cells around the atom - nine runs of consecutive slots, one per (y, z) row of
// cells - are compacted into the wave's LDS tile as (x, y, z, R^2) by the conservative test B_ij. Lane l owns the points l + 64 m; MB of
// them at a time keep their state in one 64-bit mask, so a list longer than the tile goes through in tiles without losing what earlier
// tiles decided. Against a tile a lane first tries the record that buried its previous point (mdtraj's trick), then all lanes walk the
// tile together (the same address: a broadcast read) until every point of the wave is decided.
__global__ __launch_bounds__(NT) void k_sasa_points(size_t total, int n_struct, int n_total, const int* __restrict__ offsets,
                                                    const int* __restrict__ capoff, int total_cap, const float* __restrict__ X,
                                                    const float* __restrict__ radius, int P, const float* __restrict__ S,
                                                    const double* __restrict__ sigma, const SasaGrid* __restrict__ grids,
                                                    const int* __restrict__ cell_cnt, const int* __restrict__ cell_of,
                                                    const float4* __restrict__ sorted, const int* __restrict__ pos_of, int last_first,
                                                    int* __restrict__ counts) {
    __shared__ float4 tiles[WAVES][TILE];
    const int lane = threadIdx.x & 63;
    float4* tile = tiles[threadIdx.x >> 6];
    const size_t a = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (a >= total) return;                                  // (whole waves leave; no workgroup barrier below)
    const int cell = cell_of[a];
    if (cell < 0) {
        if (lane == 0) counts[a] = P;
        return;
    }
    const int f = (int)(a / (size_t)n_total), i = (int)(a % (size_t)n_total);
    const int s = struct_of(i, n_struct, offsets);
    const SasaGrid g = grids[(size_t)f * n_struct + s];
    const int* cnt = cell_cnt + (size_t)f * total_cap + capoff[s];
    const float4* rec = sorted + (size_t)f * n_total + offsets[s];
    const int self = pos_of[a];
    const float xi = X[3 * a], yi = X[3 * a + 1], zi = X[3 * a + 2], ri = radius[i];
    const double bi = fabs((double)ri) * sigma[0], bx = 0x1p-20 * (fabs((double)xi) + fabs((double)yi) + fabs((double)zi)) + 1e-18;
    // lane r < 9 holds the slots [first, end) of the row (cy + r % 3 - 1, cz + r / 3 - 1), cells cx - 1 .. cx + 1
    int first = 0, end = 0;
    {
        const int cx = cell % g.nx, cy = (cell / g.nx) % g.ny, cz = cell / (g.nx * g.ny);
        const int y = cy + lane % 3 - 1, z = cz + lane / 3 - 1;
        if (lane < 9 && y >= 0 && y < g.ny && z >= 0 && z < g.nz) {
            const int row = (z * g.ny + y) * g.nx;
            first = cnt[row + max(cx - 1, 0)];
            end = cnt[row + min(cx + 1, g.nx - 1) + 1];
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_m = (P + 63) >> 6;
    int exposed = 0;
    for (int mb = 0; mb < n_m; mb += MB) {
        unsigned long long buried = 0ull;                   // bit m - mb: point lane + 64 m is buried, or does not exist
        int r = 0, pos = __shfl(first, 0), stop = __shfl(end, 0);
        do {
            int n = 0;
            while (n + 64 <= TILE) {
                while (r < 9 && pos >= stop) {
                    ++r;
                    pos = __shfl(first, min(r, 8));
                    stop = __shfl(end, min(r, 8));
                }
                if (r >= 9) break;
                const int slot = pos + lane;
                bool keep = false;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (slot < stop && slot != self) {
                    v = rec[slot];
                    const double dx = (double)xi - (double)v.x, dy = (double)yi - (double)v.y, dz = (double)zi - (double)v.z;
                    const double b = (bi + fabs((double)v.w)) * (1.0 + 0x1p-18) + bx;
                    keep = dx * dx + dy * dy + dz * dz <= b * b;
                }
                const unsigned long long mask = __ballot(keep);
                if (keep) tile[n + __popcll(mask & below)] = make_float4(v.x, v.y, v.z, __fmul_rn(v.w, v.w));
                n += __popcll(mask);
                pos += 64;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            int last = -1;
            for (int g0 = 0; g0 < MB && mb + g0 < n_m; g0 += MU) {
                bool done[MU], open = false;
                float tx[MU], ty[MU], tz[MU];
#pragma unroll
                for (int u = 0; u < MU; ++u) {
                    const int k = lane + 64 * (mb + g0 + u);
                    done[u] = k >= P || ((buried >> (g0 + u)) & 1ull) != 0ull;
                    const float* p = S + 3 * (size_t)(k < P ? k : 0);
                    tx[u] = __fadd_rn(xi, __fmul_rn(ri, p[0]));
                    ty[u] = __fadd_rn(yi, __fmul_rn(ri, p[1]));
                    tz[u] = __fadd_rn(zi, __fmul_rn(ri, p[2]));
                    open |= !done[u];
                }
                if (__ballot(open) != 0ull) {
                    if (last_first && last >= 0) {
                        const float4 c = tile[last];
#pragma unroll
                        for (int u = 0; u < MU; ++u) done[u] = done[u] || buries(tx[u], ty[u], tz[u], c);
                    }
                    for (int j = 0; j < n; ++j) {
                        const float4 c = tile[j];
                        open = false;
#pragma unroll
                        for (int u = 0; u < MU; ++u) {
                            if (!done[u] && buries(tx[u], ty[u], tz[u], c)) { done[u] = true; last = j; }
                            open |= !done[u];
                        }
                        if (__ballot(open) == 0ull) break;
                    }
                }
#pragma unroll
                for (int u = 0; u < MU; ++u) buried |= (unsigned long long)(done[u] ? 1 : 0) << (g0 + u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } while (r < 9);
        const int nb = min(MB, n_m - mb);
        exposed += nb - __popcll(nb == 64 ? buried : buried & ((1ull << nb) - 1ull));
    }
    for (int o = 32; o > 0; o >>= 1) exposed += __shfl_xor(exposed, o);
    if (lane == 0) counts[a] = exposed;
}

__device__ __forceinline__ double area_of(double c0, int count, float r) {
    return __dmul_rn(__dmul_rn(__dmul_rn(c0, (double)count), (double)r), (double)r);
}

__global__ __launch_bounds__(NT) void k_sasa_area(size_t total, int n_total, double c0, const int* __restrict__ counts,
                                                  const float* __restrict__ radius, float* __restrict__ area) {
    const size_t a = (size_t)blockIdx.x * NT + threadIdx.x;
    if (a >= total) return;
    area[a] = (float)area_of(c0, counts[a], radius[a % (size_t)n_total]);
}

// one thread per (frame, group): the double areas of its atoms (perm[off[g] .. off[g + 1]), in that order) added in double
__global__ __launch_bounds__(NT) void k_sasa_groups(size_t total, int n_total, int n_groups, double c0, const int* __restrict__ counts,
                                                    const float* __restrict__ radius, const int* __restrict__ perm,
                                                    const int* __restrict__ off, float* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
    if (k >= total) return;
    const size_t f = k / (size_t)n_groups;
    const int q = (int)(k % (size_t)n_groups);
    const int a0 = max(0, min(off[q], n_total)), a1 = max(a0, min(off[q + 1], n_total));
    double sum = 0.0;
    for (int a = a0; a < a1; ++a) {
        const int p = perm[a];
        if ((unsigned)p < (unsigned)n_total) sum = __dadd_rn(sum, area_of(c0, counts[f * (size_t)n_total + p], radius[p]));
    }
    out[k] = (float)sum;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_sasa_last_error(void) { return last_error(); }

int pesto_sasa(pesto_model* m, int64_t F, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X, const float* radius,
               int32_t P, const float* points, double c0, int32_t* counts_out, float* area_out, int32_t n_groups, const int32_t* perm,
               const int32_t* group_off, float* group_out, int32_t ptr_kind, void* stream) {
    if (!struct_offsets || !X || !radius || !points) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (!counts_out && !area_out && !group_out) return fail(PESTO_ERR_INVALID, "no output requested");
    if (P < 1 || P > PESTO_SASA_MAX_POINTS) return fail(PESTO_ERR_INVALID, "1 to %d sphere points, got %d", PESTO_SASA_MAX_POINTS, P);
    if (F < 1 || n_total < 1 || F > 0x7fffffff || n_total > 0x7fffffff || F * n_total > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "F * n_total must be in 1 .. 2^31 - 1 (F = %lld, n_total = %lld)", (long long)F, (long long)n_total);
    if (n_struct < 1 || n_struct > n_total || struct_offsets[0] != 0 || struct_offsets[n_struct] != n_total)
        return fail(PESTO_ERR_INVALID, "1 <= n_struct <= n_total structures whose offsets run from 0 to n_total");
    if (const int s = first_unordered(struct_offsets, n_struct); s >= 0)
        return fail(PESTO_ERR_INVALID, "struct_offsets must increase strictly (structure %d)", s);
    if (!std::isfinite(c0)) return fail(PESTO_ERR_INVALID, "c0 must be finite");
    if (group_out && (n_groups < 1 || !perm || !group_off || F * (int64_t)n_groups > 0x7fffffff))
        return fail(PESTO_ERR_INVALID, "group sums need perm, group_off and 1 <= n_groups with F * n_groups < 2^31");
    if (F * (int64_t)n_struct > 0x7fffffff) return fail(PESTO_ERR_INVALID, "F * n_struct must stay below 2^31");
    if (int rc = begin(m, ptr_kind)) return rc;
    const char* dbg_env = std::getenv("PESTO_SASA_DEBUG");
    const int dbg = dbg_env ? std::atoi(dbg_env) : 0;
    // cells of a (frame, structure): at most its atoms and MAX_CELLS, plus the total behind the last cell
    std::vector<int32_t> capoff((size_t)n_struct + 1, 0);
    for (int s = 0; s < n_struct; ++s)
        capoff[s + 1] = capoff[s] + std::min<int32_t>(struct_offsets[s + 1] - struct_offsets[s], MAX_CELLS) + 1;
    const int total_cap = capoff[n_struct];                  // <= 2 n_total
    const size_t total = (size_t)F * n_total, n_grids = (size_t)F * n_struct, n_cells = (size_t)F * total_cap;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(X, total * 12), iR = bf.input(radius, (size_t)n_total * 4), iS = bf.input(points, (size_t)P * 12);
    const int iO = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iK = bf.table(capoff.data(), capoff.size() * 4);
    const int iC = counts_out ? bf.output(counts_out, total * 4) : bf.scratch(total * 4);
    const int iA = bf.output(area_out, total * 4);
    const int iP = bf.input(perm, group_out ? (size_t)n_total * 4 : 0), iG = bf.input(group_off, group_out ? ((size_t)n_groups + 1) * 4 : 0);
    const int iQ = bf.output(group_out, group_out ? (size_t)F * n_groups * 4 : 0);
    const int iSig = bf.scratch(8), iGr = bf.scratch(n_grids * sizeof(SasaGrid)), iCnt = bf.scratch(n_cells * 4), iCur = bf.scratch(n_cells * 4);
    const int iCell = bf.scratch(total * 4), iPos = bf.scratch(total * 4), iSort = bf.scratch(total * 16);
    int rc = bf.upload();
    if (rc == 0) {
        const int* off = bf.ptr<const int>(iO);
        const int* cap = bf.ptr<const int>(iK);
        const float* x = bf.ptr<const float>(iX);
        const float* r = bf.ptr<const float>(iR);
        hipLaunchKernelGGL(k_sasa_sigma, dim3(1), dim3(NT), 0, bf.stm, P, bf.ptr<const float>(iS), bf.ptr<double>(iSig));
        hipLaunchKernelGGL(k_sasa_setup, dim3((unsigned)n_grids), dim3(NT), 0, bf.stm, n_struct, (int)n_total, off, cap, total_cap, x, r,
                           bf.ptr<const double>(iSig), bf.ptr<SasaGrid>(iGr), bf.ptr<int>(iCnt));
        hipLaunchKernelGGL(k_sasa_count, dim3(blocks(total, NT)), dim3(NT), 0, bf.stm, total, n_struct, (int)n_total, off, cap, total_cap, x, r,
                           bf.ptr<const SasaGrid>(iGr), bf.ptr<int>(iCnt), bf.ptr<int>(iCell));
        hipLaunchKernelGGL(k_sasa_scan, dim3((unsigned)n_grids), dim3(NT), 0, bf.stm, n_struct, cap, total_cap, bf.ptr<const SasaGrid>(iGr),
                           bf.ptr<int>(iCnt), bf.ptr<int>(iCur));
        hipLaunchKernelGGL(k_sasa_scatter, dim3(blocks(total, NT)), dim3(NT), 0, bf.stm, total, n_struct, (int)n_total, off, cap, total_cap, x, r,
                           bf.ptr<const int>(iCell), bf.ptr<int>(iCur), bf.ptr<float4>(iSort), bf.ptr<int>(iPos));
        if (dbg & 1) {                                      // timing hook: the grid build alone; the outputs are zeroed
            for (int it : {iC, iA, iQ})
                if (bf.ptr<void>(it)) (void)hipMemsetAsync(bf.ptr<void>(it), 0, bf.items[it].bytes, bf.stm);
        } else {
            hipLaunchKernelGGL(k_sasa_points, dim3((unsigned)((total + WAVES - 1) / WAVES)), dim3(NT), 0, bf.stm, total, n_struct, (int)n_total, off,
                               cap, total_cap, x, r, P, bf.ptr<const float>(iS), bf.ptr<const double>(iSig), bf.ptr<const SasaGrid>(iGr),
                               bf.ptr<const int>(iCnt), bf.ptr<const int>(iCell), bf.ptr<const float4>(iSort), bf.ptr<const int>(iPos),
                               (dbg & 2) ? 0 : 1, bf.ptr<int>(iC));
            if (area_out)
                hipLaunchKernelGGL(k_sasa_area, dim3(blocks(total, NT)), dim3(NT), 0, bf.stm, total, (int)n_total, c0, bf.ptr<const int>(iC), r,
                                   bf.ptr<float>(iA));
            if (group_out)
                hipLaunchKernelGGL(k_sasa_groups, dim3(blocks((size_t)F * n_groups, NT)), dim3(NT), 0, bf.stm, (size_t)F * n_groups, (int)n_total,
                                   n_groups, c0, bf.ptr<const int>(iC), r, bf.ptr<const int>(iP), bf.ptr<const int>(iG), bf.ptr<float>(iQ));
        }
    }
    return bf.finish(rc, "sasa");
}
