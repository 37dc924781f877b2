// pesto_contacts.hip - the contact side of the reference's dataset build: every atom pair closer than r_thr between two subunits of an
// assembly, in the reference's order and fp32 rounding, and the typed residue-residue contact keys of each pair of subunits.
//
// replaces: extract_all_contacts / locate_contacts (src/data_encoding.py:116-167; one dense torch distance matrix per pair of subunits) and
// contacts_types + pack_contacts_data (processing/build_dataset.py:41-83; a dense [R0, R1, 79, 79] bool map per pair, then torch.where).
// One launch sequence for a batch of assemblies:
//   grid     a uniform cell grid per assembly, cells >= r_thr * 1.001 wide (as k_lbl_grid_* of pesto_eval.hip, re-derived here)
//   count    one thread per atom a: partners b with subunit[b] > subunit[a] and d < r_thr; exclusive scan -> each atom's slot range
//   emit     the same search writes (b, d) into a's range and sorts the (short) range by b: the pairs in (a, b) order
//   regroup  a stable LSD radix sort of (subunit[a], subunit[b], position) keys: the reference's per-(i, j) lists, a then b ascending
//   keys     (group, r0, r1 | t0, t1) of every pair, stable radix sort, the last contact of each residue pair -> sorted Y keys, T;
//            the swapped (group, r1, r0 | t1, t0) radix-sorted
// Every step is deterministic: the scans and sorts fix the order, and the only atomics are counters and idempotent stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/pesto_hip.h"

namespace pesto {

namespace {

constexpr int CT_GRID_MAX = 64;           // cells per axis at most
constexpr int CT_RES_BITS = 13, CT_TYPE_BITS = 7;
struct CtGrid { float minx, miny, minz, inv_h; int nx, ny, nz, base; };

// the device counters of one call
struct CtState {
    int K;            // contacts
    int n_sort;       // K when it fits the capacity, else 0 (every later stage then has nothing to do)
    int G;            // (i, j) groups
    int U2;           // typed keys (residue pairs whose last contact is typed), per direction
    int len;          // length of the next scan (radix histograms)
    int err;          // bit 0: subunit ids not ascending / out of range; bit 1: residue or type out of range
};

__device__ __forceinline__ int ct_struct_of(int i, int n_struct, const int* __restrict__ offsets) {
    int lo = 0, hi = n_struct;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ void ct_cell3(const CtGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(g.nx - 1, max(0, (int)((x - g.minx) * g.inv_h)));
    cy = min(g.ny - 1, max(0, (int)((y - g.miny) * g.inv_h)));
    cz = min(g.nz - 1, max(0, (int)((z - g.minz) * g.inv_h)));
}
// torch.norm's float32 distance: sqrt(fma(z, z, fma(y, y, x * x))), every step rounded as written (the build contracts only within a
// source expression, so the chain is spelled out rather than left to the compiler)
__device__ __forceinline__ float ct_dist(float4 a, float4 b) {
    const float rx = b.x - a.x, ry = b.y - a.y, rz = b.z - a.z;
    return sqrtf(__fmaf_rn(rz, rz, __fmaf_rn(ry, ry, __fmul_rn(rx, rx))));
}

// ------------------------------------------------------------------------------------------------ cell grid
// one workgroup per assembly: bounding box -> cell size and counts (at most 2 N_s + 64 cells: assembly s owns cells [2 off_s + 65 s, ...))
__global__ __launch_bounds__(256) void k_ct_grid_setup(int n_struct, const int* __restrict__ offsets, const float* __restrict__ X, float r_thr,
                                                       CtGrid* __restrict__ grids, int* __restrict__ cell_cnt) {
    const int s = blockIdx.x;
    const int s0 = offsets[s], s1 = offsets[s + 1];
    __shared__ float red[6][256];
    __shared__ CtGrid gsh;
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
        CtGrid g;
        g.base = 2 * s0 + 65 * s;
        g.minx = red[0][0]; g.miny = red[1][0]; g.minz = red[2][0];
        g.nx = g.ny = g.nz = 1; g.inv_h = 0.f;                 // one cell (every pair is examined): non-finite coordinates
        const float ex = red[3][0] - red[0][0], ey = red[4][0] - red[1][0], ez = red[5][0] - red[2][0];
        const float ext = fmaxf(ex, fmaxf(ey, ez));
        if (ext == ext && ext < 1e30f && g.minx == g.minx && g.miny == g.miny && g.minz == g.minz) {
            const long long cap = 2LL * (s1 - s0) + 64;
            float h = fmaxf(r_thr * 1.001f, ext / (float)CT_GRID_MAX * 1.0001f);
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

// cell of every atom, cell counts; the per-atom checks of the call's contract
__global__ __launch_bounds__(256) void k_ct_grid_count(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                       const int* __restrict__ subunit, const int* __restrict__ residue, const int* __restrict__ type,
                                                       int n_sub, int n_types, const CtGrid* __restrict__ grids, int* __restrict__ cell_cnt,
                                                       int* __restrict__ cell_of, CtState* __restrict__ st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int s = ct_struct_of(i, n_struct, offsets);
    const int su = subunit[i];
    bool bad = su < 0 || su >= n_sub;
    if (i > 0) {
        const int prev = subunit[i - 1];
        bad |= i == offsets[s] ? su <= prev : su < prev;          // ascending along the atoms, no subunit in two assemblies
    }
    const int r = residue[i], t = type[i];
    const bool bad_rt = r < 0 || r >= (1 << CT_RES_BITS) || t < -1 || t >= n_types;
    if (bad || bad_rt) atomicOr(&st->err, (bad ? 1 : 0) | (bad_rt ? 2 : 0));
    const CtGrid g = grids[s];
    int cx, cy, cz;
    ct_cell3(g, X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], cx, cy, cz);
    const int c = (cz * g.ny + cy) * g.nx + cx;
    cell_of[i] = c;
    atomicAdd(&cell_cnt[g.base + c], 1);
}

// exclusive scan of one assembly's cell counts (one workgroup per assembly) -> cell starts (local atom positions), cursor copy
__global__ __launch_bounds__(1024) void k_ct_grid_scan(const CtGrid* __restrict__ grids, int* __restrict__ cell_cnt, int* __restrict__ cell_cur) {
    const CtGrid g = grids[blockIdx.x];
    const int nc = g.nx * g.ny * g.nz;
    int* cnt = cell_cnt + g.base;
    int* cur = cell_cur + g.base;
    __shared__ int part[1024];
    const int per = (nc + 1023) / 1024;
    const int c0 = min(nc, (int)threadIdx.x * per), c1 = min(nc, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) { const int n = cnt[c]; cnt[c] = run; cur[c] = run; run += n; }
    if (threadIdx.x == 1023) cnt[nc] = part[1023];
}

// atoms in cell order: (x, y, z, batch index) and their subunit
__global__ __launch_bounds__(256) void k_ct_grid_scatter(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                         const int* __restrict__ subunit, const CtGrid* __restrict__ grids,
                                                         const int* __restrict__ cell_of, int* __restrict__ cell_cur, float4* __restrict__ sorted,
                                                         int* __restrict__ sorted_sub) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int s = ct_struct_of(i, n_struct, offsets);
    const int pos = offsets[s] + atomicAdd(&cell_cur[grids[s].base + cell_of[i]], 1);
    sorted[pos] = make_float4(X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], __int_as_float(i));
    sorted_sub[pos] = subunit[i];
}

// ------------------------------------------------------------------------------------------------ contact pairs
// One thread per atom in cell order (the threads of a wave share their candidate cells), scanning the 3 x 3 rows of three consecutive
// cells around it. EMIT = false: cnt[a] = partners b with subunit[b] > subunit[a] and d < r_thr; ties[a] = 1 where an atom of another
// subunit lies at exactly r_thr. EMIT = true: the partners go to [off[a], off[a] + cnt[a]) (only when the total fits: st->n_sort > 0),
// then that range is insertion-sorted by b (a handful of entries per atom; the same set as the count pass, so the range fills exactly).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_ct_pairs(int n_total, int n_struct, const int* __restrict__ offsets, const CtGrid* __restrict__ grids,
                                                  const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                  const int* __restrict__ sorted_sub, float r_thr, int* __restrict__ cnt,
                                                  unsigned char* __restrict__ ties, const int* __restrict__ off, const CtState* __restrict__ st,
                                                  int* __restrict__ pb, float* __restrict__ pd) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_total) return;
    if (EMIT && st->n_sort == 0) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    const int s = ct_struct_of(p, n_struct, offsets);
    const int own = sorted_sub[p];
    const CtGrid g = grids[s];
    const int* start = cell_start + g.base;
    const int s0 = offsets[s];
    int cx, cy, cz;
    ct_cell3(g, a.x, a.y, a.z, cx, cy, cz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    int n = 0, tie = 0;
    const int o = EMIT ? off[i] : 0;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const int row = (z * g.ny + y) * g.nx;
            const int j1 = s0 + start[row + x1 + 1];
            for (int j = s0 + start[row + x0]; j < j1; ++j) {
                const int sb = sorted_sub[j];
                if (sb == own) continue;
                const float4 b = sorted[j];
                const float d = ct_dist(a, b);
                if (!EMIT && d == r_thr) tie = 1;
                if (sb > own && d < r_thr) {
                    if (EMIT) { pb[o + n] = __float_as_int(b.w); pd[o + n] = d; }
                    ++n;
                }
            }
        }
    if (!EMIT) {
        cnt[i] = n;
        ties[i] = (unsigned char)tie;
        return;
    }
    for (int u = o + 1; u < o + n; ++u) {          // insertion sort of a's partners by b (distinct indices)
        const int bk = pb[u];
        const float dk = pd[u];
        int v = u - 1;
        while (v >= o && pb[v] > bk) { pb[v + 1] = pb[v]; pd[v + 1] = pd[v]; --v; }
        pb[v + 1] = bk;
        pd[v + 1] = dk;
    }
}

// ------------------------------------------------------------------------------------------------ scans and sizes
// exclusive scan in place of data[0, len) by one workgroup (len = *len_ptr, or n when len_ptr is null); the total goes to *total (if any)
__global__ __launch_bounds__(1024) void k_ct_scan(int* __restrict__ data, int n, const int* __restrict__ len_ptr, int* __restrict__ total) {
    const int len = len_ptr ? *len_ptr : n;
    __shared__ int part[1024];
    const int per = (len + 1023) / 1024;
    const int c0 = min(len, (int)threadIdx.x * per), c1 = min(len, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += data[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) { const int v = data[c]; data[c] = run; run += v; }
    if (threadIdx.x == 1023 && total) *total = part[1023];
}

__global__ void k_ct_sizes(CtState* st, long long cap_pairs) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->n_sort = (long long)st->K <= cap_pairs ? st->K : 0;
}

// ------------------------------------------------------------------------------------------------ stable LSD radix sort of uint64 keys
// 8 bits per pass, one key per thread, 256 keys per tile. hist[digit * n_tiles + tile] -> exclusive scan (k_ct_scan) -> each key's place:
// keys of a smaller digit, then those of earlier tiles, earlier waves and earlier lanes (a wave's lanes of one digit found with 8 ballots).
constexpr int RS_TILE = 256;

// st->len for the next k_ct_scan: the histogram length of a radix pass over n_sort * mul keys (hist) or n_sort * mul itself
__global__ void k_rs_len(const int* __restrict__ n_ptr, int mul, int hist, CtState* __restrict__ st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->len = hist ? 256 * ((*n_ptr * mul + RS_TILE - 1) / RS_TILE) : *n_ptr * mul;
}

__global__ __launch_bounds__(RS_TILE) void k_rs_hist(const unsigned long long* __restrict__ in, const int* __restrict__ n_ptr, int mul, int shift,
                                                     int* __restrict__ hist) {
    const int n = *n_ptr * mul;
    const int n_tiles = (n + RS_TILE - 1) / RS_TILE;
    const int t = blockIdx.x;
    if (t >= n_tiles) return;
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int k = t * RS_TILE + threadIdx.x;
    if (k < n) atomicAdd(&cnt[(int)((in[k] >> shift) & 255)], 1);
    __syncthreads();
    hist[threadIdx.x * n_tiles + t] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(RS_TILE) void k_rs_scatter(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                        const int* __restrict__ n_ptr, int mul, int shift, const int* __restrict__ hist) {
    const int n = *n_ptr * mul;
    const int n_tiles = (n + RS_TILE - 1) / RS_TILE;
    const int t = blockIdx.x;
    if (t >= n_tiles) return;
    __shared__ int wcnt[RS_TILE / 64][256];
    for (int w = 0; w < RS_TILE / 64; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int k = t * RS_TILE + threadIdx.x;
    const bool valid = k < n;
    const unsigned long long key = valid ? in[k] : 0ull;
    const int dg = (int)((key >> shift) & 255);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long match = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot(valid && ((dg >> b) & 1));
        match &= ((dg >> b) & 1) ? m : ~m;
    }
    const int rank = __popcll(match & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[w][dg] = __popcll(match);
    __syncthreads();
    if (!valid) return;
    int base = hist[dg * n_tiles + t] + rank;
    for (int v = 0; v < w; ++v) base += wcnt[v][dg];
    out[base] = key;
}

// ------------------------------------------------------------------------------------------------ regroup and typed keys
// sort key of pair k (in (a, b) order): subunit[a] | subunit[b] | k
__global__ __launch_bounds__(256) void k_ct_pair_keys(const CtState* __restrict__ st, int n_total, const int* __restrict__ off,
                                                      const int* __restrict__ subunit, const int* __restrict__ pb, unsigned long long* __restrict__ keys) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n_total || st->n_sort == 0) return;
    const unsigned long long sa = (unsigned)subunit[a] & 0xffffu;
    for (int k = off[a], e = off[a + 1]; k < e; ++k)
        keys[k] = (sa << 48) | ((unsigned long long)((unsigned)subunit[pb[k]] & 0xffffu) << 32) | (unsigned long long)k;
}

// the pairs in group order (a recovered from the position through the per-atom offsets), group-start flags
__global__ __launch_bounds__(256) void k_ct_gather(const CtState* __restrict__ st, int n_total, const int* __restrict__ off,
                                                   const unsigned long long* __restrict__ keys, const int* __restrict__ pb, const float* __restrict__ pd,
                                                   int* __restrict__ pairs_out, float* __restrict__ d_out, int* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= st->n_sort) return;
    const unsigned long long key = keys[k];
    const int src = (int)(key & 0xffffffffull);
    int lo = 0, hi = n_total;                      // the atom a whose range holds src: the last with off[a] <= src
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= src) lo = mid; else hi = mid; }
    pairs_out[2 * (size_t)k] = lo;
    pairs_out[2 * (size_t)k + 1] = pb[src];
    d_out[k] = pd[src];
    flag[k] = (k == 0 || (keys[k - 1] >> 32) != (key >> 32)) ? 1 : 0;
}

// Typed keys. contacts_types (build_dataset.py:41-60) assigns Y[rids0, rids1] = H, one [79, 79] slab per contact, and torch's index_put_
// lets the LAST contact of a residue pair (in contact order) decide that pair's slab: its (t0, t1) when both atoms have a type, nothing
// otherwise. So every contact k gets the key (g, r0, r1 | t0, t1) - low 16 bits 0xffff for an untyped pair - and a STABLE sort on the bits
// above the types keeps contact order within each (g, r0, r1) run; the run's last key is the residue pair's slab. The forward keys come
// out sorted (one per residue pair); the swapped ones, (g, r1, r0 | t1, t0), are sorted again.
//   bits 63..42 group (22), 41..29 first residue (13), 28..16 second residue (13), 15..8 first type, 7..0 second type
constexpr int CT_KEY_G = 42, CT_KEY_R0 = 29, CT_KEY_R1 = 16;

// group table (subunit i, subunit j, first pair) and the key of every contact
__global__ __launch_bounds__(256) void k_ct_type_keys(const CtState* __restrict__ st, const int* __restrict__ pairs, const int* __restrict__ gid_excl,
                                                      const unsigned long long* __restrict__ gkeys, const int* __restrict__ residue,
                                                      const int* __restrict__ type, int n_types, long long cap_groups, int* __restrict__ groups,
                                                      unsigned long long* __restrict__ tkeys) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K) return;
    const int a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    // gid_excl: the exclusive scan of the group-start flags, so the group of k is gid_excl[k] - 1 + (k starts a group)
    const bool first = k == 0 || (gkeys[k - 1] >> 32) != (gkeys[k] >> 32);
    const int g = gid_excl[k] + (first ? 1 : 0) - 1;
    if (first && g < cap_groups) {
        const unsigned long long key = gkeys[k];
        groups[4 * (size_t)g] = (int)(key >> 48);
        groups[4 * (size_t)g + 1] = (int)((key >> 32) & 0xffff);
        groups[4 * (size_t)g + 2] = k;
    }
    const int ta = type[a], tb = type[b];
    const unsigned ra = (unsigned)residue[a] & 0x1fffu, rb = (unsigned)residue[b] & 0x1fffu;        // (out of range: reported, masked)
    const bool typed = ta >= 0 && tb >= 0 && ta < n_types && tb < n_types;
    tkeys[k] = ((unsigned long long)(g & 0x3fffff) << CT_KEY_G) | ((unsigned long long)ra << CT_KEY_R0) | ((unsigned long long)rb << CT_KEY_R1) |
               (typed ? (unsigned long long)((ta << 8) | tb) : 0xffffull);
}

// 1 where k is the last contact of its residue pair and that contact is typed
__global__ __launch_bounds__(256) void k_ct_last_flags(const CtState* __restrict__ st, const unsigned long long* __restrict__ tkeys,
                                                       int* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K) return;
    const unsigned long long key = tkeys[k];
    const bool last = k + 1 == K || (tkeys[k + 1] >> CT_KEY_R1) != (key >> CT_KEY_R1);
    flag[k] = (last && (key & 0xffffull) != 0xffffull) ? 1 : 0;
}

// forward rows (r0, r1, t0, t1), per group the key count and T[t0][t1], and the swapped keys for their own sort
__global__ __launch_bounds__(256) void k_ct_write_fwd(const CtState* __restrict__ st, const unsigned long long* __restrict__ tkeys,
                                                      const int* __restrict__ pos, int n_types, long long cap_groups, unsigned short* __restrict__ keys_out,
                                                      int* __restrict__ groups, unsigned char* __restrict__ T, unsigned long long* __restrict__ rkeys) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K || st->G > cap_groups) return;
    const unsigned long long key = tkeys[k];
    const bool last = k + 1 == K || (tkeys[k + 1] >> CT_KEY_R1) != (key >> CT_KEY_R1);
    if (!last || (key & 0xffffull) == 0xffffull) return;
    const int u = pos[k];
    const int g = (int)(key >> CT_KEY_G);
    const unsigned r0 = (unsigned)(key >> CT_KEY_R0) & 0x1fffu, r1 = (unsigned)(key >> CT_KEY_R1) & 0x1fffu;
    const unsigned t0 = (unsigned)(key >> 8) & 0xffu, t1 = (unsigned)key & 0xffu;
    unsigned short* row = keys_out + 4 * (size_t)u;
    row[0] = (unsigned short)r0; row[1] = (unsigned short)r1; row[2] = (unsigned short)t0; row[3] = (unsigned short)t1;
    atomicAdd(&groups[4 * (size_t)g + 3], 1);
    T[((size_t)g * n_types + t0) * n_types + t1] = 1;
    rkeys[u] = ((unsigned long long)g << CT_KEY_G) | ((unsigned long long)r1 << CT_KEY_R0) | ((unsigned long long)r0 << CT_KEY_R1) |
               (unsigned long long)((t1 << 8) | t0);
}

// swapped rows (r1, r0, t1, t0) from their sorted keys
__global__ __launch_bounds__(256) void k_ct_write_rev(const CtState* __restrict__ st, long long cap_groups, const unsigned long long* __restrict__ rkeys,
                                                      unsigned short* __restrict__ rkeys_out) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= st->U2 || st->G > cap_groups) return;
    const unsigned long long key = rkeys[u];
    unsigned short* row = rkeys_out + 4 * (size_t)u;
    row[0] = (unsigned short)((key >> CT_KEY_R0) & 0x1fffu); row[1] = (unsigned short)((key >> CT_KEY_R1) & 0x1fffu);
    row[2] = (unsigned short)((key >> 8) & 0xffu); row[3] = (unsigned short)(key & 0xffu);
}

__global__ void k_ct_finish(CtState* st, int* off, int n_total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) off[n_total] = st->K;
}

// stable sort of keys[0, *n_ptr) on bits [bit_lo, bit_hi) (an even number of 8-bit passes: the result ends in `keys`)
void radix_sort(hipStream_t s, unsigned long long* keys, unsigned long long* tmp, int n_cap, int mul, int bit_lo, int bit_hi, CtState* st,
                int* hist, const int* n_ptr) {
    const int nb = (int)(((long long)n_cap * mul + RS_TILE - 1) / RS_TILE);
    hipLaunchKernelGGL(k_rs_len, dim3(1), dim3(1), 0, s, n_ptr, mul, 1, st);
    for (int shift = bit_lo; shift < bit_hi; shift += 8) {
        hipLaunchKernelGGL(k_rs_hist, dim3(nb), dim3(RS_TILE), 0, s, keys, n_ptr, mul, shift, hist);
        hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, hist, 0, &st->len, (int*)nullptr);
        hipLaunchKernelGGL(k_rs_scatter, dim3(nb), dim3(RS_TILE), 0, s, keys, tmp, n_ptr, mul, shift, hist);
        unsigned long long* t = keys; keys = tmp; tmp = t;
    }
}

struct CtBuffers {
    int* offsets; CtState* st; CtGrid* grids; int* cell_cnt; int* cell_cur; int* cell_of; float4* sorted; int* sorted_sub; int* off;
    int* pb; float* pd; unsigned long long* gkeys; unsigned long long* tkeys; unsigned long long* rkeys; unsigned long long* tmp; int* flag;
    int* hist;
};

void launch_contacts(hipStream_t s, int n_total, int n_struct, int n_sub, const float* X, const int* subunit, const int* residue, const int* type,
                     int n_types, float r_thr, int cap_pairs, int cap_groups, const CtBuffers& w, int* pairs_out, float* d_out, int* groups_out,
                     unsigned short* keys_out, unsigned short* rkeys_out, unsigned char* T_out, unsigned char* ties_out) {
    const int nb = (n_total + 255) / 256, nbk = (cap_pairs + 255) / 256;
    (void)hipMemsetAsync(groups_out, 0, (size_t)cap_groups * 16, s);
    (void)hipMemsetAsync(T_out, 0, (size_t)cap_groups * n_types * n_types, s);
    hipLaunchKernelGGL(k_ct_grid_setup, dim3(n_struct), dim3(256), 0, s, n_struct, w.offsets, X, r_thr, w.grids, w.cell_cnt);
    hipLaunchKernelGGL(k_ct_grid_count, dim3(nb), dim3(256), 0, s, n_total, n_struct, w.offsets, X, subunit, residue, type, n_sub, n_types, w.grids,
                       w.cell_cnt, w.cell_of, w.st);
    hipLaunchKernelGGL(k_ct_grid_scan, dim3(n_struct), dim3(1024), 0, s, w.grids, w.cell_cnt, w.cell_cur);
    hipLaunchKernelGGL(k_ct_grid_scatter, dim3(nb), dim3(256), 0, s, n_total, n_struct, w.offsets, X, subunit, w.grids, w.cell_of, w.cell_cur,
                       w.sorted, w.sorted_sub);
    // count -> per-atom ranges -> emit in (a, b) order
    hipLaunchKernelGGL(k_ct_pairs<false>, dim3(nb), dim3(256), 0, s, n_total, n_struct, w.offsets, w.grids, w.cell_cnt, w.sorted, w.sorted_sub,
                       r_thr, w.off, ties_out, (const int*)nullptr, (const CtState*)w.st, (int*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.off, n_total, (const int*)nullptr, &w.st->K);
    hipLaunchKernelGGL(k_ct_finish, dim3(1), dim3(1), 0, s, w.st, w.off, n_total);
    hipLaunchKernelGGL(k_ct_sizes, dim3(1), dim3(1), 0, s, w.st, (long long)cap_pairs);
    hipLaunchKernelGGL(k_ct_pairs<true>, dim3(nb), dim3(256), 0, s, n_total, n_struct, w.offsets, w.grids, w.cell_cnt, w.sorted, w.sorted_sub,
                       r_thr, (int*)nullptr, (unsigned char*)nullptr, (const int*)w.off, (const CtState*)w.st, w.pb, w.pd);
    // regroup by (subunit[a], subunit[b]): the low 32 bits (the position) are in order already
    hipLaunchKernelGGL(k_ct_pair_keys, dim3(nb), dim3(256), 0, s, (const CtState*)w.st, n_total, (const int*)w.off, subunit, (const int*)w.pb,
                       w.gkeys);
    radix_sort(s, w.gkeys, w.tmp, cap_pairs, 1, 32, 64, w.st, w.hist, &w.st->n_sort);
    hipLaunchKernelGGL(k_ct_gather, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, n_total, (const int*)w.off, (const unsigned long long*)w.gkeys,
                       (const int*)w.pb, (const float*)w.pd, pairs_out, d_out, w.flag);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.flag, 0, &w.st->n_sort, &w.st->G);
    hipLaunchKernelGGL(k_ct_type_keys, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const int*)pairs_out, (const int*)w.flag,
                       (const unsigned long long*)w.gkeys, residue, type, n_types, (long long)cap_groups, groups_out, w.tkeys);
    // typed keys: stable sort on (group, r0, r1), the last of each run, the swapped keys sorted again
    radix_sort(s, w.tkeys, w.tmp, cap_pairs, 1, CT_KEY_R1, 64, w.st, w.hist, &w.st->n_sort);
    hipLaunchKernelGGL(k_ct_last_flags, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const unsigned long long*)w.tkeys, w.flag);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.flag, 0, &w.st->n_sort, &w.st->U2);
    hipLaunchKernelGGL(k_ct_write_fwd, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const unsigned long long*)w.tkeys, (const int*)w.flag,
                       n_types, (long long)cap_groups, keys_out, groups_out, T_out, w.rkeys);
    radix_sort(s, w.rkeys, w.tmp, cap_pairs, 1, CT_KEY_R1, 64, w.st, w.hist, &w.st->U2);
    hipLaunchKernelGGL(k_ct_write_rev, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (long long)cap_groups, (const unsigned long long*)w.rkeys,
                       rkeys_out);
}

thread_local std::string g_ct_err;

int cfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_ct_err = buf;
    return code;
}

#define CT_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) { rc = cfail(PESTO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); goto done; } \
    } while (0)

size_t ct_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_contacts_last_error(void) { return g_ct_err.c_str(); }

int pesto_contacts(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, int32_t n_sub, const float* X,
                   const int32_t* subunit, const int32_t* residue, const int32_t* type, int32_t n_types, float r_thr, int64_t cap_pairs,
                   int64_t cap_groups, int32_t* pairs_out, float* d_out, int32_t* groups_out, uint16_t* keys_out, uint16_t* rkeys_out,
                   uint8_t* T_out, uint8_t* ties_out, int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (n_total < 1 || n_total > 0x3ffffff0 || n_struct < 1 || n_sub < 1 || n_sub > 0xffff || !struct_offsets || !X || !subunit || !residue ||
        !type || !sizes_out || !ties_out)
        return cfail(PESTO_ERR_INVALID, "bad arguments");
    if (n_types < 1 || n_types > (1 << CT_TYPE_BITS)) return cfail(PESTO_ERR_INVALID, "n_types must be in [1, %d]", 1 << CT_TYPE_BITS);
    if (cap_pairs < 1 || cap_pairs > 0x3fffffff || cap_groups < 1 || cap_groups > 0x3fffff)
        return cfail(PESTO_ERR_INVALID, "cap_pairs must be in [1, 2^30), cap_groups in [1, 2^22)");
    if (!pairs_out || !d_out || !groups_out || !keys_out || !rkeys_out || !T_out) return cfail(PESTO_ERR_INVALID, "bad arguments");
    if (!(r_thr > 0.f) || !std::isfinite(r_thr)) return cfail(PESTO_ERR_INVALID, "r_thr must be a positive finite distance");
    if (ptr_kind != PESTO_PTR_HOST && ptr_kind != PESTO_PTR_DEVICE) return cfail(PESTO_ERR_INVALID, "ptr_kind must be PESTO_PTR_HOST or PESTO_PTR_DEVICE");
    if (struct_offsets[0] != 0 || struct_offsets[n_struct] != n_total)
        return cfail(PESTO_ERR_INVALID, "struct_offsets must span [0, %lld]", (long long)n_total);
    for (int s = 0; s < n_struct; ++s)
        if (struct_offsets[s + 1] <= struct_offsets[s]) return cfail(PESTO_ERR_INVALID, "struct_offsets: empty or unordered assembly %d", s);
    if (int rc = pesto_synchronize(m)) {
        const char* e = pesto_last_error();
        return cfail(rc, "%s", e ? e : "invalid model handle");
    }
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)n_total, C = (size_t)cap_pairs, Cg = (size_t)cap_groups, nt2 = (size_t)n_types * n_types;
    const size_t cells = 2 * n + 65 * (size_t)n_struct, tiles = (C + RS_TILE - 1) / RS_TILE;
    size_t o = 0;
    auto take = [&o](size_t b) { const size_t at = o; o += ct_align(b); return at; };
    const size_t oOff = take(((size_t)n_struct + 1) * 4), oSt = take(sizeof(CtState)), oG = take((size_t)n_struct * sizeof(CtGrid)),
                 oCnt = take(cells * 4), oCur = take(cells * 4), oCell = take(n * 4), oSort = take(n * 16), oSub = take(n * 4),
                 oAOff = take((n + 1) * 4), oPb = take(C * 4), oPd = take(C * 4), oGk = take(C * 8), oTk = take(C * 8), oRk8 = take(C * 8),
                 oTmp = take(C * 8), oFlag = take(C * 4), oHist = take(256 * tiles * 4);
    // host pointers: staged inputs [X | subunit | residue | type] and outputs
    const size_t oX = dev ? 0 : take(n * 12), oS = dev ? 0 : take(n * 4), oR = dev ? 0 : take(n * 4), oT = dev ? 0 : take(n * 4),
                 oP = dev ? 0 : take(C * 8), oD = dev ? 0 : take(C * 4), oGr = dev ? 0 : take(Cg * 16), oK = dev ? 0 : take(C * 8),
                 oRk = dev ? 0 : take(C * 8), oTt = dev ? 0 : take(Cg * nt2), oTi = dev ? 0 : take(n);
    char* w = nullptr;
    CtState hs = {};
    int rc = 0;
    if (hipMallocAsync((void**)&w, o, st) != hipSuccess) return cfail(PESTO_ERR_NOMEM, "device allocation of %zu bytes failed", o);
    {
        CtBuffers b{(int*)(w + oOff), (CtState*)(w + oSt), (CtGrid*)(w + oG), (int*)(w + oCnt), (int*)(w + oCur), (int*)(w + oCell),
                    (float4*)(w + oSort), (int*)(w + oSub), (int*)(w + oAOff), (int*)(w + oPb), (float*)(w + oPd),
                    (unsigned long long*)(w + oGk), (unsigned long long*)(w + oTk), (unsigned long long*)(w + oRk8), (unsigned long long*)(w + oTmp),
                    (int*)(w + oFlag),
                    (int*)(w + oHist)};
        int32_t* P = dev ? pairs_out : (int32_t*)(w + oP);
        float* D = dev ? d_out : (float*)(w + oD);
        int32_t* Gr = dev ? groups_out : (int32_t*)(w + oGr);
        uint16_t* Kf = dev ? keys_out : (uint16_t*)(w + oK);
        uint16_t* Kr = dev ? rkeys_out : (uint16_t*)(w + oRk);
        uint8_t* Tt = dev ? T_out : (uint8_t*)(w + oTt);
        uint8_t* Ti = dev ? ties_out : (uint8_t*)(w + oTi);
        CT_TRY(hipMemcpyAsync(b.offsets, struct_offsets, ((size_t)n_struct + 1) * 4, hipMemcpyHostToDevice, st));
        CT_TRY(hipMemsetAsync(b.st, 0, sizeof(CtState), st));
        if (!dev) {
            CT_TRY(hipMemcpyAsync(w + oX, X, n * 12, hipMemcpyHostToDevice, st));
            CT_TRY(hipMemcpyAsync(w + oS, subunit, n * 4, hipMemcpyHostToDevice, st));
            CT_TRY(hipMemcpyAsync(w + oR, residue, n * 4, hipMemcpyHostToDevice, st));
            CT_TRY(hipMemcpyAsync(w + oT, type, n * 4, hipMemcpyHostToDevice, st));
        }
        launch_contacts(st, (int)n_total, n_struct, n_sub, dev ? X : (const float*)(w + oX), dev ? subunit : (const int*)(w + oS),
                        dev ? residue : (const int*)(w + oR), dev ? type : (const int*)(w + oT), n_types, r_thr, (int)C, (int)Cg, b, P, D, Gr, Kf, Kr,
                        Tt, Ti);
        CT_TRY(hipGetLastError());
        // the one synchronisation for sizing: the counters
        CT_TRY(hipMemcpyAsync(&hs, b.st, sizeof(CtState), hipMemcpyDeviceToHost, st));
        CT_TRY(hipStreamSynchronize(st));
        const bool fits = hs.n_sort == hs.K;
        sizes_out[0] = hs.K;
        sizes_out[1] = fits ? hs.G : -1;
        sizes_out[2] = fits ? hs.U2 : -1;
        if (!dev) {
            CT_TRY(hipMemcpyAsync(ties_out, Ti, n, hipMemcpyDeviceToHost, st));
            if (fits) {
                const size_t K = (size_t)hs.K, U = (size_t)hs.U2, G = (size_t)hs.G <= Cg ? (size_t)hs.G : 0;
                if (K) {
                    CT_TRY(hipMemcpyAsync(pairs_out, P, K * 8, hipMemcpyDeviceToHost, st));
                    CT_TRY(hipMemcpyAsync(d_out, D, K * 4, hipMemcpyDeviceToHost, st));
                }
                if (U) {
                    CT_TRY(hipMemcpyAsync(keys_out, Kf, U * 8, hipMemcpyDeviceToHost, st));
                    CT_TRY(hipMemcpyAsync(rkeys_out, Kr, U * 8, hipMemcpyDeviceToHost, st));
                }
                if (G) {
                    CT_TRY(hipMemcpyAsync(groups_out, Gr, G * 16, hipMemcpyDeviceToHost, st));
                    CT_TRY(hipMemcpyAsync(T_out, Tt, G * nt2, hipMemcpyDeviceToHost, st));
                }
            }
        }
    }
done:
    (void)hipFreeAsync(w, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = cfail(PESTO_ERR_HIP, "contacts: stream synchronisation failed");
    if (rc == 0 && (hs.err & 1))
        rc = cfail(PESTO_ERR_INVALID, "subunit: ids must lie in [0, n_sub), ascend along the atoms and change between assemblies");
    if (rc == 0 && (hs.err & 2)) rc = cfail(PESTO_ERR_INVALID, "residue must lie in [0, 8192) and type in [-1, n_types)");
    return rc;
}
