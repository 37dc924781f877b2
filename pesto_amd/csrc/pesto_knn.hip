// pesto_knn.hip - the k-NN topology search + collate (launch_knn_collate) and its tie report (launch_knn_ties); declarations in
// pesto_kernels.h. Large structures search through the uniform cell grid of pesto_cellgrid.h, the fourth user of that header.
//
// replaces extract_topology (src/data_encoding.py:87-102, dense [N,N,3] on the host) and the index part of
// collate_batch_features (src/dataset.py:100-109) with one kernel over a concatenated batch.
// Contract reproduced exactly: D = |X_j - X_i| in fp32 (products and sums rounded separately, like torch.norm over a
// 3-vector), entries with D < 1e-2 (self, coincident atoms) are pushed behind every other atom of the structure - the
// reference adds max(D) to them, so they sort after all unmasked entries and by D among themselves - and the
// min(k, N_s) smallest keys are emitted in ascending order as 1-based batch-global ids, zero padded to KMAX columns.
// One wave per query atom: candidates stream through in chunks of 64 (one per lane); the running k best are kept one
// per lane, sorted across the wave; a chunk that cannot improve the current worst is rejected with one ballot, the
// others are bitonic-sorted and merged (64-bit keys: [masked | distance bits | index], so ties break by index).
#include <hip/hip_runtime.h>

#include "pesto_cellgrid.h"
#include "pesto_kernels.h"

namespace pesto {

namespace {

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}
// one compare-exchange stage of a bitonic network across the wave: partner = lane ^ j, ascending if `up`
__device__ __forceinline__ unsigned long long bitonic_step(unsigned long long v, int lane, int j, bool up) {
    const unsigned long long o = shfl_xor64(v, j);
    const bool lower = (lane & j) == 0;
    const bool take_min = lower == up;
    return take_min ? (v < o ? v : o) : (v < o ? o : v);
}

// merge one chunk of 64 candidate keys (one per lane, WORST = none) into the running top-64 (ascending across lanes)
__device__ __forceinline__ unsigned long long knn_merge(unsigned long long top, unsigned long long key, int lane) {
    const unsigned long long worst = ((unsigned long long)__shfl((unsigned)(top >> 32), 63) << 32) | __shfl((unsigned)top, 63);
    if (__ballot(key < worst) == 0ull) return top;        // nothing in this chunk beats the current k-th best
    for (int size = 2; size <= 64; size <<= 1)
        for (int jj = size >> 1; jj > 0; jj >>= 1) key = bitonic_step(key, lane, jj, (lane & size) == 0 || size == 64);
    // 64 smallest of (top ascending, chunk ascending): min(top[l], chunk[63-l]) is bitonic; merge it ascending
    const unsigned long long rev = shfl_xor64(key, 63);
    unsigned long long m = top < rev ? top : rev;
    for (int jj = 32; jj > 0; jj >>= 1) m = bitonic_step(m, lane, jj, true);
    return m;
}
__device__ __forceinline__ unsigned long long knn_key(float rx, float ry, float rz, int local_index) {
    // torch.norm over the contiguous xyz axis is the scalar loop acc = acc + v * v, which the reference's build contracts into an FMA
    // chain: d = sqrt(fma(z, z, fma(y, y, x * x))), norm3() of pesto_cellgrid.h, reproduces its distance matrix bit for bit (555,000 pairs
    // of a pdbs_test chain; separately rounded products agree on 89 % only, and a one-ulp difference reorders two neighbours in about one
    // row of 40,000) (sqrtf, not __fsqrt_rn: the intrinsic lowers to the bare v_sqrt_f32 - one ulp off in places - while sqrtf is
    // correctly rounded)
    const float d = norm3(rx, ry, rz);
    const unsigned masked = d < 1e-2f ? 1u : 0u;
    return ((unsigned long long)((masked << 31) | __float_as_uint(d)) << 32) | (unsigned)local_index;   // d >= 0: bit 31 is free
}

// Exact fp32 distance ties that STRADDLE a neighbourhood cut-off: the table orders equal distances by index, the reference's torch.topk
// leaves their order undefined (src/data_encoding.py:98-99), so for such a row the two disagree on which of two equally distant atoms
// belongs to the first 8 / 16 / 32 / 64 neighbours - the one difference between the tables that can move a logit (a tie inside a
// neighbourhood only reorders a sum). One wave per row: the keys (masked flag | distance bits, as knn_key) of the table's last column
// inside every cut, the number of columns inside the cut that carry that key, and - one scan over the atoms of the structure - the number
// of atoms that do: more atoms than columns = the tie straddles the cut. flags[i]: bit 0 / 1 / 2 / 3 = cut after column 8 / 16 / 32 / 64.
template <typename IdT>
__global__ __launch_bounds__(256) void k_knn_ties(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X, int k,
                                                  const IdT* __restrict__ ids, unsigned char* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_total) return;
    const int s = struct_of(i, n_struct, offsets);
    const int s0 = offsets[s], s1 = offsets[s + 1];
    const float xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
    auto dkey = [&](int j) -> unsigned {      // distance key of atom j (batch-global, 0-based): knn_key without the index
        return (unsigned)(knn_key(X[3 * (size_t)j] - xi, X[3 * (size_t)j + 1] - yi, X[3 * (size_t)j + 2] - zi, 0) >> 32);
    };
    // this lane's column of the table (k <= 64 columns; 0 = padding)
    const long long id = lane < k ? (long long)ids[(size_t)i * KMAX + lane] : 0;
    const bool have = id > 0;
    const unsigned mykey = have ? dkey((int)id - 1) : 0xffffffffu;
    // the four cut keys first, then ONE scan over the structure's atoms counting all four (round 4 scanned once per cut). The atom itself is
    // left out on both sides - as a column (structures of <= 64 atoms list it, masked, at the end) and in the scan: its own distance-0 key
    // used to count as a tie with every coincident atom and over-reported rows of structures with duplicated coordinates.
    unsigned kc[4];
    int inside[4], all[4] = {0, 0, 0, 0};
    bool live[4];
    const bool mine = have && (int)id - 1 != i;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cut = 8 << c;
        live[c] = cut <= k && ids[(size_t)i * KMAX + min(cut, KMAX) - 1] > 0;       // fewer than `cut` neighbours: nothing beyond the cut
        kc[c] = __shfl(mykey, min(cut, 64) - 1);
        inside[c] = __popcll(__ballot(lane < cut && mine && mykey == kc[c]));
    }
    for (int j = s0 + lane; j < s1; j += 64) {
        const unsigned kj = j == i ? 0xfffffffeu : dkey(j);      // (no key equals this one: the masked flag is the top bit, the rest distance bits)
#pragma unroll
        for (int c = 0; c < 4; ++c) all[c] += kj == kc[c] ? 1 : 0;
    }
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int a = all[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (live[c] && a > inside[c]) out |= 1u << c;
    }
    if (lane == 0) flags[i] = (unsigned char)out;
}

// ---- the grid path of large structures (N_s >= KNN_CELL_MIN): brute force is O(N_s^2); on the cell grid of pesto_cellgrid.h (cells of
// at least 4.5 A * 1.001, at most 64 per axis and 2 N_s + 64 in all) a query only meets the atoms of the (2s+1)^3 cells around it.
// Exactness is kept by a completeness test: every atom outside that block is at least s*h away from the query, so once the k-th best
// key is an unmasked distance strictly below s*h the k best are final; otherwise the block grows (s = 2, 3, 5, 8, ... until it covers
// the grid). Keys, tie-breaks and the merge network are those of the brute-force path, so both paths return identical tables, whatever
// the grid's geometry. A batch with one large structure builds the grid of every member (O(n_total) of count and scatter work); the
// small members and the one-cell grid of non-finite coordinates (inv_h = 0) stay on the brute-force path.
constexpr int KNN_CELL_MIN = 1024;        // structures at least this large use the grid (measured: 2x at N = 3,000, 5.7x at N = 20,000)
constexpr float KNN_CELL_EDGE = 4.5f;     // the r_thr of grid_build: dense clouds get cells of 4.5045 A

template <typename IdT>
__global__ __launch_bounds__(256) void k_knn_collate(int n_total, int n_struct, const int* __restrict__ offsets,
                                                     const float* __restrict__ X, int k, IdT* __restrict__ ids_out,
                                                     const CellGrid* __restrict__ grids, const int* __restrict__ cell_start,
                                                     const float4* __restrict__ sorted) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_total) return;
    const int st = struct_of(i, n_struct, offsets);      // wave-uniform
    const int s0 = offsets[st], s1 = offsets[st + 1];
    const float xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
    const unsigned long long WORST = ~0ull;
    unsigned long long top = WORST;                 // lane l holds the (l+1)-th best key so far, ascending across lanes
    const int knn = min(k, s1 - s0);
    bool done = false;
    if (grids && s1 - s0 >= KNN_CELL_MIN && grids[st].inv_h != 0.f) {
        const CellGrid g = grids[st];
        const int* cs = cell_start + g.base;
        // the cell edge: CellGrid carries inv_h = 1 / h only, and 1 / inv_h is h to within one ulp (2^-23 relative), which the 1e-4
        // margin of the completeness radius below covers beside the rounding of the cell assignment it was made for
        const float h = 1.0f / g.inv_h;
        int cx, cy, cz;
        cell3(g, xi, yi, zi, cx, cy, cz);
        // (the loop ends by construction: at most 64 cells per axis, so `whole` holds at s >= 64 at the latest - s = 88 of the sequence)
        for (int s = 2; !done; s = s < 3 ? 3 : (s * 8 + 4) / 5) {       // 2, 3, 5, 8, 13, ...
            top = WORST;
            const int x0 = max(0, cx - s), x1 = min(g.nx - 1, cx + s);
            for (int zc = max(0, cz - s); zc <= min(g.nz - 1, cz + s); ++zc)
                for (int yc = max(0, cy - s); yc <= min(g.ny - 1, cy + s); ++yc) {
                    const int row = (zc * g.ny + yc) * g.nx;
                    const int a0 = cs[row + x0], a1 = cs[row + x1 + 1];      // one contiguous run of the sorted atoms
                    for (int base = a0; base < a1; base += 64) {
                        unsigned long long key = WORST;
                        if (base + lane < a1) {
                            const float4 c = sorted[s0 + base + lane];       // (c.w: the batch index)
                            key = knn_key(c.x - xi, c.y - yi, c.z - zi, __float_as_int(c.w) - s0);
                        }
                        top = knn_merge(top, key, lane);
                    }
                }
            const bool whole = cx - s <= 0 && cy - s <= 0 && cz - s <= 0 && cx + s >= g.nx - 1 && cy + s >= g.ny - 1 && cz + s >= g.nz - 1;
            // k-th best: an unmasked distance strictly inside the radius the block guarantees (small margin for the rounding of
            // the cell assignment and of h) -> no atom outside the block can enter or tie
            const unsigned long long kth = ((unsigned long long)__shfl((unsigned)(top >> 32), knn - 1) << 32) | __shfl((unsigned)top, knn - 1);
            const unsigned hi32 = (unsigned)(kth >> 32);
            const bool ok = kth != WORST && !(hi32 >> 31) && __uint_as_float(hi32) < (float)s * h * 0.9999f;
            done = whole || ok;
        }
    }
    if (!done) {
        top = WORST;
        for (int base = s0; base < s1; base += 64) {
            const int j = base + lane;
            unsigned long long key = WORST;
            if (j < s1) key = knn_key(X[3 * (size_t)j] - xi, X[3 * (size_t)j + 1] - yi, X[3 * (size_t)j + 2] - zi, j - s0);
            top = knn_merge(top, key, lane);
        }
    }
    // lanes 0..knn-1 hold the neighbours in ascending order; zero padding beyond (dataset.py:100,109)
    long long id = 0;
    if (lane < knn) id = (long long)(unsigned)(top & 0xffffffffu) + s0 + 1;
    if (lane < KMAX) ids_out[(size_t)i * KMAX + lane] = (IdT)id;
}

}  // namespace

KnnGridBytes knn_grid_bytes(size_t n_total, size_t n_struct) {
    return {n_struct * sizeof(CellGrid), cells_before(n_total, n_struct) * sizeof(int)};
}
int knn_cell_min() { return KNN_CELL_MIN; }

void launch_knn_collate(hipStream_t st, int n_total, int n_struct, const int* offsets, const float* X, int k, void* ids_out, int ids_kind,
                        void* grids, int* cell_cnt, int* cell_cur, int* cell_of, void* sorted) {
    const CellGrid* g = (const CellGrid*)grids;
    if (g) grid_build(st, n_total, n_struct, offsets, X, KNN_CELL_EDGE, GridBufs{(CellGrid*)grids, cell_cnt, cell_cur, cell_of, (float4*)sorted}, NoCheck{}, NoPayload{});
    const dim3 grid((n_total + 3) / 4), block(256);
    if (ids_kind == PESTO_IDS_INT64)
        hipLaunchKernelGGL(k_knn_collate<long long>, grid, block, 0, st, n_total, n_struct, offsets, X, k, (long long*)ids_out, g, (const int*)cell_cnt, (const float4*)sorted);
    else
        hipLaunchKernelGGL(k_knn_collate<int>, grid, block, 0, st, n_total, n_struct, offsets, X, k, (int*)ids_out, g, (const int*)cell_cnt, (const float4*)sorted);
}

void launch_knn_ties(hipStream_t st, int n_total, int n_struct, const int* offsets, const float* X, int k, const void* ids, int ids_kind,
                      unsigned char* flags) {
    const dim3 grid((n_total + 3) / 4), block(256);
    if (ids_kind == PESTO_IDS_INT64) hipLaunchKernelGGL(k_knn_ties<long long>, grid, block, 0, st, n_total, n_struct, offsets, X, k, (const long long*)ids, flags);
    else hipLaunchKernelGGL(k_knn_ties<int>, grid, block, 0, st, n_total, n_struct, offsets, X, k, (const int*)ids, flags);
}

}  // namespace pesto
