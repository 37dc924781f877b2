// pesto_patches.hip - interface patches: the connected components of the distance-threshold graph over the residues predicted to be an
// interface of one class, or of two classes at once, for every (structure, class pair) of a batch in one call.
//
// The C entry point (include/pesto_hip.h) lives here too, on the call plumbing of pesto_call.h.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pesto_call.h"

namespace pesto {

namespace {

// replaces: cluster_interfaces / follow_rabbits (interfaceome/cluster_interfaces.py:9-56, cluster_multi_interfaces.py:9-61): a dense
// NumPy distance matrix per (structure, selection) and a set-based breadth-first search per component.
//   node(r)    = afs[r] > afs_thr & has_ca[r] & p[r,i] > p_thr & p[r,j] > p_thr          (float32, strict; NaN never passes)
//   edge(a, b) = sqrt((dx*dx + dy*dy) + dz*dz) < d_thr  with every operation rounded      (NumPy's float32 distance matrix)
// The edge test runs as s < s_star on the rounded sum s, where the host derives s_star as the smallest float with sqrt_rn(s_star) >= d_thr:
// sqrt_rn is monotonic, so the decision is the one the correctly rounded square root would make, NaN and inf included.
// Components: lock-free union-find over the node list (nodes numbered in residue order) that always links the larger root under the smaller
// one, so that every root is its component's smallest node whatever the order of the joins; finds halve the path. Patches are numbered
// in the order of their roots, which is the order follow_rabbits emits them. Sizes are exact integer counts; the mean of p[:, i] and p[:, j]
// per patch is summed in double by one wave in a fixed order (lane = node mod 64, then a fixed butterfly), so every output is bit-identical
// from call to call.
// Structures of at most PATCH_SMALL_MAX residues run one workgroup per (structure, selection) with everything in LDS; larger ones gather
// their nodes into global memory, spread the node-pair tiles over many workgroups and finish with one workgroup per (structure, selection).
constexpr int SMALL_THREADS = 256;
constexpr int LARGE_THREADS = 1024;
constexpr int TILE = 256;

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Every value a parent entry ever holds is a node of the same set with a smaller index than the entry's own (links put a root under a
// smaller root; halving stores a grandparent that was read earlier). A halving store can be stale and so RAISE an entry again, but never
// to the entry's own index or above, and never into a root (it stores only into an entry already read as a non-root, and a non-root
// never becomes a root again). So every walk ends, and the sets are exactly the unions made.
// uf_find: root of x, halving the path it walks (union phase only: the stores go into other threads' entries).
__device__ __forceinline__ int uf_find(int* par, int x) {
    for (;;) {
        const int p = ld(par + x);
        if (p == x) return x;
        const int g = ld(par + p);
        if (g != p) st(par + x, g);
        x = g;
    }
}

// uf_root: root of x, read only. The compression pass after the union phase must use this one: there every thread stores into its own
// entries only, so each entry ends the pass holding its root (with halving, a stale store into another thread's entry could leave it on a
// non-root ancestor).
__device__ __forceinline__ int uf_root(const int* par, int x) {
    for (int p = ld(par + x); p != x; p = ld(par + x)) x = p;
    return x;
}

__device__ __forceinline__ void uf_unite(int* par, int a, int b) {
    for (;;) {
        a = uf_find(par, a);
        b = uf_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;               // link the larger root a under b; fails only if a stopped being a root meanwhile
        if (__hip_atomic_compare_exchange_strong(par + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// NumPy's float32 squared distance, no contraction: (dx*dx + dy*dy) + dz*dz
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(bx, ax), dy = __fsub_rn(by, ay), dz = __fsub_rn(bz, az);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// exclusive prefix of a flag over the workgroup (NT threads, wave64); *total = number of set flags
template <int NT>
__device__ __forceinline__ int block_scan_flag(bool f, int* wsum, int* total) {
    const unsigned long long mask = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[w] = __popcll(mask);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const int v = wsum[k];
        off += k < w ? v : 0;
        tot += v;
    }
    *total = tot;
    return off + pre;
}

struct PatchArgs {
    int R, n_class, n_sel;
    const int* offsets;     // [n_struct + 1]
    const int* sel;         // [n_sel, 2]
    const float* xyz;       // [R, 3]
    const float* p;         // [R, n_class]
    const float* afs;       // [R] or null
    const unsigned char* has_ca;  // [R] or null
    float afs_thr, p_thr, s_star;
    int* patch_of;          // [n_sel, R]
    int* n_patches;         // [n_struct, n_sel]
    int* patch_size;        // [n_sel, R]
    float* patch_mean;      // [n_sel, R, 2]
};

// nodes of rows [r0, r1) in residue order: coordinates (as float bits), parent = self, local row; the outputs of the other rows
// (-1, 0, 0) are written here. Returns the node count.
template <int NT>
__device__ int patch_gather(const PatchArgs& A, int s, int k, int* nx, int* ny, int* nz, int* par, int* res, int* wsum) {
    const int r0 = A.offsets[s], r1 = A.offsets[s + 1];
    const int ci = A.sel[2 * k], cj = A.sel[2 * k + 1];
    int base = 0;
    for (int c0 = r0; c0 < r1; c0 += NT) {
        const int r = c0 + (int)threadIdx.x;
        bool node = false;
        if (r < r1) {
            const float* pr = A.p + (size_t)r * A.n_class;
            node = pr[ci] > A.p_thr && pr[cj] > A.p_thr && (!A.afs || A.afs[r] > A.afs_thr) && (!A.has_ca || A.has_ca[r] != 0);
        }
        int tot;
        const int pre = block_scan_flag<NT>(node, wsum, &tot);
        if (node) {
            const int x = base + pre;
            nx[x] = __float_as_int(A.xyz[3 * (size_t)r]);
            ny[x] = __float_as_int(A.xyz[3 * (size_t)r + 1]);
            nz[x] = __float_as_int(A.xyz[3 * (size_t)r + 2]);
            st(par + x, x);
            res[x] = r - r0;
        } else if (r < r1) {
            const size_t o = (size_t)k * A.R + r;
            A.patch_of[o] = -1;
            A.patch_size[o] = 0;
            A.patch_mean[2 * o] = 0.f;
            A.patch_mean[2 * o + 1] = 0.f;
        }
        base += tot;
    }
    return base;
}

// after every union of (s, k): compress, number the roots in node order, count, average and write the node rows' outputs.
// cnt / ord / roots reuse the coordinate arrays (n entries each).
template <int NT>
__device__ void patch_finish(const PatchArgs& A, int s, int k, int n, int* par, const int* res, int* cnt, int* ord, int* roots, int* wsum) {
    const int r0 = A.offsets[s];
    const int ci = A.sel[2 * k], cj = A.sel[2 * k + 1];
    // no more links: the roots are final. Each thread writes only its own entries (uf_root stores nothing), so after the barrier every
    // entry holds its root.
    for (int x = threadIdx.x; x < n; x += NT) st(par + x, uf_root(par, x));
    __syncthreads();
    int n_p = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int x = c0 + (int)threadIdx.x;
        const bool root = x < n && ld(par + x) == x;
        int tot;
        const int pre = block_scan_flag<NT>(root, wsum, &tot);
        if (root) { ord[x] = n_p + pre; roots[n_p + pre] = x; }
        if (x < n) st(cnt + x, 0);
        n_p += tot;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < n; x += NT) atomicAdd(cnt + ld(par + x), 1);
    __syncthreads();
    // one wave per patch: its members lie in [root, n); lane l sums the members at root + l (mod 64), in order, then a fixed butterfly
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < n_p; q += NT / 64) {
        const int rho = roots[q], c = ld(cnt + rho);
        double si = 0.0, sj = 0.0;
        for (int x0 = rho, seen = 0; seen < c; x0 += 64) {
            const int x = x0 + lane;
            const bool in = x < n && ld(par + x) == rho;
            if (in) {
                const float* pr = A.p + (size_t)(r0 + res[x]) * A.n_class;
                si += (double)pr[ci];
                sj += (double)pr[cj];
            }
            seen += __popcll(__ballot(in));
        }
        for (int o = 32; o > 0; o >>= 1) { si += __shfl_xor(si, o); sj += __shfl_xor(sj, o); }
        if (lane == 0) {
            const size_t o = (size_t)k * A.R + r0 + res[rho];
            A.patch_size[o] = c;
            A.patch_mean[2 * o] = (float)(si / (double)c);
            A.patch_mean[2 * o + 1] = (float)(sj / (double)c);
        }
    }
    for (int x = threadIdx.x; x < n; x += NT) {
        const int rt = ld(par + x);
        const size_t o = (size_t)k * A.R + r0 + res[x];
        A.patch_of[o] = ord[rt];
        if (rt != x) {
            A.patch_size[o] = 0;
            A.patch_mean[2 * o] = 0.f;
            A.patch_mean[2 * o + 1] = 0.f;
        }
    }
    if (threadIdx.x == 0) A.n_patches[(size_t)s * A.n_sel + k] = n_p;
}

// ---- small structures: one workgroup per (structure, selection), dynamic LDS of 5 ints per residue of the largest such structure. One
// launch, largest structures first. (One launch per size class was measured slower on AlphaFold-like size mixes: the launches serialise.)
__global__ __launch_bounds__(SMALL_THREADS) void k_patches_small(PatchArgs A, const int* __restrict__ structs, int cap) {
    extern __shared__ int lds[];
    __shared__ int wsum[SMALL_THREADS / 64];
    const int s = structs[blockIdx.x / A.n_sel], k = blockIdx.x % A.n_sel;
    int *nx = lds, *ny = lds + cap, *nz = lds + 2 * cap, *par = lds + 3 * cap, *res = lds + 4 * cap;
    const int n = patch_gather<SMALL_THREADS>(A, s, k, nx, ny, nz, par, res, wsum);
    __syncthreads();
    for (int a = threadIdx.x; a < n; a += SMALL_THREADS) {
        const float ax = __int_as_float(nx[a]), ay = __int_as_float(ny[a]), az = __int_as_float(nz[a]);
        for (int b = a + 1; b < n; ++b)
            if (dist2(ax, ay, az, __int_as_float(nx[b]), __int_as_float(ny[b]), __int_as_float(nz[b])) < A.s_star) uf_unite(par, a, b);
    }
    __syncthreads();
    patch_finish<SMALL_THREADS>(A, s, k, n, par, res, nx, ny, nz, wsum);
}

// ---- large structures: item = (structure, selection) with its node arrays at `base` of the global scratch
struct LargeItem { int s, k, base, n_tiles; };

__global__ __launch_bounds__(LARGE_THREADS) void k_patches_large_gather(PatchArgs A, const LargeItem* __restrict__ items, int* __restrict__ gx,
                                                                        int* __restrict__ gy, int* __restrict__ gz, int* __restrict__ gpar,
                                                                        int* __restrict__ gres, int* __restrict__ n_nodes) {
    __shared__ int wsum[LARGE_THREADS / 64];
    const LargeItem it = items[blockIdx.x];
    const int n = patch_gather<LARGE_THREADS>(A, it.s, it.k, gx + it.base, gy + it.base, gz + it.base, gpar + it.base, gres + it.base, wsum);
    if (threadIdx.x == 0) n_nodes[blockIdx.x] = n;
}

// one workgroup per (item, tile pair ta <= tb); items' blocks are contiguous (blk_off, n_items + 1 entries)
__global__ __launch_bounds__(TILE) void k_patches_large_pairs(int n_items, const LargeItem* __restrict__ items, const int* __restrict__ blk_off,
                                                              const int* __restrict__ n_nodes, const int* __restrict__ gx, const int* __restrict__ gy,
                                                              const int* __restrict__ gz, int* __restrict__ gpar, float s_star) {
    __shared__ float tx[TILE], ty[TILE], tz[TILE];
    int lo = 0, hi = n_items;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (blk_off[mid] <= (int)blockIdx.x) lo = mid; else hi = mid; }
    const LargeItem it = items[lo];
    const int n = n_nodes[lo];
    int t = (int)blockIdx.x - blk_off[lo], ta = 0;
    while (t >= it.n_tiles - ta) { t -= it.n_tiles - ta; ++ta; }
    const int tb = ta + t;
    if (tb * TILE >= n) return;
    const int b0 = tb * TILE, nb = min(TILE, n - b0);
    if ((int)threadIdx.x < nb) {
        tx[threadIdx.x] = __int_as_float(gx[it.base + b0 + threadIdx.x]);
        ty[threadIdx.x] = __int_as_float(gy[it.base + b0 + threadIdx.x]);
        tz[threadIdx.x] = __int_as_float(gz[it.base + b0 + threadIdx.x]);
    }
    __syncthreads();
    const int a = ta * TILE + (int)threadIdx.x;
    if (a >= n) return;
    const float ax = __int_as_float(gx[it.base + a]), ay = __int_as_float(gy[it.base + a]), az = __int_as_float(gz[it.base + a]);
    int* par = gpar + it.base;
    for (int j = ta == tb ? (int)threadIdx.x + 1 : 0; j < nb; ++j)
        if (dist2(ax, ay, az, tx[j], ty[j], tz[j]) < s_star) uf_unite(par, a, b0 + j);
}

__global__ __launch_bounds__(LARGE_THREADS) void k_patches_large_finish(PatchArgs A, const LargeItem* __restrict__ items, int* __restrict__ gx,
                                                                        int* __restrict__ gy, int* __restrict__ gz, int* __restrict__ gpar,
                                                                        const int* __restrict__ gres, const int* __restrict__ n_nodes) {
    __shared__ int wsum[LARGE_THREADS / 64];
    const LargeItem it = items[blockIdx.x];
    patch_finish<LARGE_THREADS>(A, it.s, it.k, n_nodes[blockIdx.x], gpar + it.base, gres + it.base, gx + it.base, gy + it.base, gz + it.base, wsum);
}

// smallest float s with sqrtf(s) >= d (d > 0 finite): sqrt(s) < d  <=>  s < s_star, for every float s (NaN compares false on both sides)
float sqrt_threshold(float d) {
    float s = d * d;
    while (!(std::sqrt(s) >= d)) s = std::nextafter(s, INFINITY);
    for (;;) {
        const float lo = std::nextafter(s, -INFINITY);
        if (!(lo >= 0.f) || !(std::sqrt(lo) >= d)) return s;
        s = lo;
    }
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_patches_last_error(void) { return last_error(); }

int pesto_interface_patches(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const float* xyz, const float* p,
                            const float* afs, const uint8_t* has_ca, int32_t n_sel, const int32_t* sel, float afs_thr, float p_thr, float d_thr,
                            int32_t* patch_of, int32_t* n_patches, int32_t* patch_size, float* patch_mean, int32_t flags, int32_t ptr_kind,
                            void* stream) {
    if (n_struct < 1 || n_class < 1 || n_class > PESTO_PATCHES_MAX_CLASSES || n_sel < 1 || n_sel > PESTO_PATCHES_MAX_SEL || !res_offsets || !xyz ||
        !p || !sel || !patch_of || !n_patches || !patch_size || !patch_mean)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (flags & ~PESTO_PATCHES_FORCE_LARGE) return fail(PESTO_ERR_INVALID, "unknown flags %d", flags);
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (!(d_thr > 0.f) || !std::isfinite(d_thr)) return fail(PESTO_ERR_INVALID, "d_thr must be a positive finite distance");
    for (int k = 0; k < n_sel; ++k)
        if (sel[2 * k] < 0 || sel[2 * k] > sel[2 * k + 1] || sel[2 * k + 1] >= n_class)
            return fail(PESTO_ERR_INVALID, "sel[%d] = (%d, %d): need 0 <= i <= j < n_class = %d", k, sel[2 * k], sel[2 * k + 1], n_class);
    if (res_offsets[0] != 0) return fail(PESTO_ERR_INVALID, "res_offsets must start at 0");
    const int64_t R = res_offsets[n_struct];
    if (int rc = check_offsets(res_offsets, n_struct, R, "res_offsets")) return rc;
    if (R > PESTO_PATCHES_MAX_ROWS || R * n_class > 0x7fffffff || R * n_sel > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "too many rows: R = %lld (at most %d, and R * n_class, R * n_sel < 2^31)", (long long)R, PESTO_PATCHES_MAX_ROWS);
    if (int rc = begin(m, ptr_kind)) return rc;
    const bool force_large = (flags & PESTO_PATCHES_FORCE_LARGE) != 0;
    // structures split by size; large items carry their scratch base and their share of the pair-tile grid
    std::vector<int> small;
    int cap = 0;
    std::vector<LargeItem> items;
    std::vector<int> blk_off(1, 0);
    int64_t rows_large = 0;
    for (int s = 0; s < n_struct; ++s) {
        const int Rs = res_offsets[s + 1] - res_offsets[s];
        if (Rs <= PESTO_PATCHES_SMALL_MAX && !force_large) {
            small.push_back(s);
            cap = std::max(cap, Rs);
            continue;
        }
        const int nt = (Rs + TILE - 1) / TILE;
        for (int k = 0; k < n_sel; ++k) {
            items.push_back(LargeItem{s, k, (int)rows_large, nt});
            rows_large += Rs;
            const int64_t nb = (int64_t)blk_off.back() + (int64_t)nt * (nt + 1) / 2;
            if (nb > 0x7fffffff) return fail(PESTO_ERR_INVALID, "too many pair tiles for the large-structure path");
            blk_off.push_back((int)nb);
        }
    }
    // largest first: the longest workgroups start early instead of forming the launch's tail (the order of the items changes no output)
    std::stable_sort(small.begin(), small.end(), [&](int a, int b) {
        return res_offsets[a + 1] - res_offsets[a] > res_offsets[b + 1] - res_offsets[b];
    });
    if ((int64_t)small.size() * n_sel > 0x7fffffff) return fail(PESTO_ERR_INVALID, "too many (structure, selection) items");
    const size_t rows = (size_t)R, n_out = rows * n_sel, n_items = items.size();
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(res_offsets, ((size_t)n_struct + 1) * 4), iSel = bf.table(sel, (size_t)n_sel * 8), iSmall = bf.table(small.data(), small.size() * 4),
              iItems = bf.table(items.data(), n_items * sizeof(LargeItem)), iBlk = bf.table(blk_off.data(), (n_items + 1) * 4);
    const int iX = bf.input(xyz, rows * 12), iP = bf.input(p, rows * n_class * 4), iA = bf.input(afs, rows * 4), iC = bf.input(has_ca, rows);
    const int iPo = bf.output(patch_of, n_out * 4), iNp = bf.output(n_patches, (size_t)n_struct * n_sel * 4), iPs = bf.output(patch_size, n_out * 4),
              iPm = bf.output(patch_mean, n_out * 8);
    const int iN = bf.scratch(n_items * 4), iG = bf.scratch((size_t)rows_large * 4 * 5);
    int rc = bf.upload();
    PatchArgs A;
    A.R = (int)R; A.n_class = n_class; A.n_sel = n_sel;
    A.offsets = bf.ptr<const int>(iOff);
    A.sel = bf.ptr<const int>(iSel);
    A.xyz = bf.ptr<const float>(iX);
    A.p = bf.ptr<const float>(iP);
    A.afs = bf.ptr<const float>(iA);
    A.has_ca = bf.ptr<const unsigned char>(iC);
    A.afs_thr = afs_thr; A.p_thr = p_thr; A.s_star = sqrt_threshold(d_thr);
    A.patch_of = bf.ptr<int>(iPo);
    A.n_patches = bf.ptr<int>(iNp);
    A.patch_size = bf.ptr<int>(iPs);
    A.patch_mean = bf.ptr<float>(iPm);
    if (rc == 0 && !small.empty()) {
        const size_t smem = (size_t)cap * 5 * 4;
        rc = hip_ok(hipFuncSetAttribute((const void*)k_patches_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "interface_patches");
        if (rc == 0)
            hipLaunchKernelGGL(k_patches_small, dim3((unsigned)(small.size() * n_sel)), dim3(SMALL_THREADS), smem, bf.stm, A, bf.ptr<const int>(iSmall), cap);
    }
    if (rc == 0 && n_items) {
        int* g = bf.ptr<int>(iG);
        const size_t L = (size_t)rows_large;
        const LargeItem* it = bf.ptr<const LargeItem>(iItems);
        int* nn = bf.ptr<int>(iN);
        hipLaunchKernelGGL(k_patches_large_gather, dim3((unsigned)n_items), dim3(LARGE_THREADS), 0, bf.stm, A, it, g, g + L, g + 2 * L, g + 3 * L, g + 4 * L, nn);
        hipLaunchKernelGGL(k_patches_large_pairs, dim3((unsigned)blk_off.back()), dim3(TILE), 0, bf.stm, (int)n_items, it, bf.ptr<const int>(iBlk), nn,
                           g, g + L, g + 2 * L, g + 3 * L, A.s_star);
        hipLaunchKernelGGL(k_patches_large_finish, dim3((unsigned)n_items), dim3(LARGE_THREADS), 0, bf.stm, A, it, g, g + L, g + 2 * L, g + 3 * L, g + 4 * L, nn);
    }
    return bf.finish(rc, "interface_patches");
}
