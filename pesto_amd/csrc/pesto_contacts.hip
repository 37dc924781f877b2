// pesto_contacts.hip - the contact side of the reference's dataset build: every atom pair closer than r_thr between two subunits of an
// assembly, in the reference's order and fp32 rounding, and the typed residue-residue contact keys of each pair of subunits.
//
// replaces: extract_all_contacts / locate_contacts (src/data_encoding.py:116-167; one dense torch distance matrix per pair of subunits) and
// contacts_types + pack_contacts_data (processing/build_dataset.py:41-83; a dense [R0, R1, 79, 79] bool map per pair, then torch.where).
// One launch sequence for a batch of assemblies:
//   grid     a uniform cell grid per assembly (pesto_cellgrid.h); its count pass also checks the per-atom contract of the call
//   count    one thread per atom a: partners b with subunit[b] > subunit[a] and d < r_thr; exclusive scan -> each atom's slot range
//   emit     the same search writes (b, d) into a's range and sorts the (short) range by b: the pairs in (a, b) order
//   regroup  a stable LSD radix sort of (subunit[a], subunit[b], position) keys: the reference's per-(i, j) lists, a then b ascending
//   keys     (group, r0, r1 | t0, t1) of every pair, stable radix sort, the last contact of each residue pair -> sorted Y keys, T;
//            the swapped (group, r1, r0 | t1, t0) radix-sorted
// Every step is deterministic: the scans and sorts fix the order, and the only atomics are counters and idempotent stores.
#include <cmath>

#include "pesto_call.h"
#include "pesto_cellgrid.h"

namespace pesto {

namespace {

constexpr int CT_RES_BITS = 13, CT_TYPE_BITS = 7;

// the device counters of one call
struct CtState {
    int K;            // contacts
    int n_sort;       // K when it fits the capacity, else 0 (every later stage then has nothing to do)
    int G;            // (i, j) groups
    int U2;           // typed keys (residue pairs whose last contact is typed), per direction
    int len;          // length of the next scan (radix histograms)
    int err;          // bit 0: subunit ids not ascending / out of range; bit 1: residue or type out of range
};

// the per-atom checks of the call's contract, made in the grid's count pass
struct CtCheck {
    const int* offsets; const int* subunit; const int* residue; const int* type; int n_sub, n_types; CtState* st;
    __device__ void operator()(int i, int s) const {
        const int su = subunit[i];
        bool bad = su < 0 || su >= n_sub;
        if (i > 0) {
            const int prev = subunit[i - 1];
            bad |= i == offsets[s] ? su <= prev : su < prev;          // ascending along the atoms, no subunit in two assemblies
        }
        const int r = residue[i], t = type[i];
        const bool bad_rt = r < 0 || r >= (1 << CT_RES_BITS) || t < -1 || t >= n_types;
        if (bad || bad_rt) atomicOr(&st->err, (bad ? 1 : 0) | (bad_rt ? 2 : 0));
    }
};
// beside the sorted coordinates: the subunit
struct CtPayload {
    const int* subunit; int* sorted_sub;
    __device__ void operator()(int pos, int i) const { sorted_sub[pos] = subunit[i]; }
};

// ------------------------------------------------------------------------------------------------ contact pairs
// One thread per atom in cell order (the threads of a wave share their candidate cells), scanning the 3 x 3 rows of three consecutive
// cells around it. EMIT = false: cnt[a] = partners b with subunit[b] > subunit[a] and d < r_thr; ties[a] = 1 where an atom of another
// subunit lies at exactly r_thr. EMIT = true: the partners go to [off[a], off[a] + cnt[a]) (only when the total fits: st->n_sort > 0),
// then that range is insertion-sorted by b (a handful of entries per atom; the same set as the count pass, so the range fills exactly).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_ct_pairs(int n_total, int n_struct, const int* __restrict__ offsets, const CellGrid* __restrict__ grids,
                                                  const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                  const int* __restrict__ sorted_sub, float r_thr, int* __restrict__ cnt,
                                                  unsigned char* __restrict__ ties, const int* __restrict__ off, const CtState* __restrict__ st,
                                                  int* __restrict__ pb, float* __restrict__ pd) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_total) return;
    if (EMIT && st->n_sort == 0) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    const int s = struct_of(p, n_struct, offsets);
    const int own = sorted_sub[p];
    int n = 0, tie = 0;
    const int o = EMIT ? off[i] : 0;
    for_each_neighbour(grids[s], cell_start, offsets[s], a, [&](int j) {
        const int sb = sorted_sub[j];
        if (sb == own) return;
        const float4 b = sorted[j];
        const float d = dist(a, b);
        if (!EMIT && d == r_thr) tie = 1;
        if (sb > own && d < r_thr) {
            if (EMIT) { pb[o + n] = __float_as_int(b.w); pd[o + n] = d; }
            ++n;
        }
    });
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
    const int sum = block_scan_exclusive<1024, false>(data, len_ptr ? *len_ptr : n);
    if (threadIdx.x == 1023 && total) *total = sum;
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
    pairs_out[2 * (size_t)k] = struct_of(src, n_total, off);       // the atom a whose range holds src: the last with off[a] <= src
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
    int* offsets; CtState* st; CellGrid* grids; int* cell_cnt; int* cell_cur; int* cell_of; float4* sorted; int* sorted_sub; int* off;
    int* pb; float* pd; unsigned long long* gkeys; unsigned long long* tkeys; unsigned long long* rkeys; unsigned long long* tmp; int* flag;
    int* hist;
};

void launch_contacts(hipStream_t s, int n_total, int n_struct, int n_sub, const float* X, const int* subunit, const int* residue, const int* type,
                     int n_types, float r_thr, int cap_pairs, int cap_groups, const CtBuffers& w, int* pairs_out, float* d_out, int* groups_out,
                     unsigned short* keys_out, unsigned short* rkeys_out, unsigned char* T_out, unsigned char* ties_out) {
    const int nb = (n_total + 255) / 256, nbk = (cap_pairs + 255) / 256;
    (void)hipMemsetAsync(groups_out, 0, (size_t)cap_groups * 16, s);
    (void)hipMemsetAsync(T_out, 0, (size_t)cap_groups * n_types * n_types, s);
    hipLaunchKernelGGL(k_grid_setup, dim3(n_struct), dim3(256), 0, s, n_struct, (const int*)w.offsets, X, r_thr, w.grids, w.cell_cnt);
    hipLaunchKernelGGL(k_grid_count<CtCheck>, dim3(nb), dim3(256), 0, s, n_total, n_struct, (const int*)w.offsets, X, (const CellGrid*)w.grids,
                       w.cell_cnt, w.cell_of, CtCheck{w.offsets, subunit, residue, type, n_sub, n_types, w.st});
    hipLaunchKernelGGL(k_grid_scan, dim3(n_struct), dim3(1024), 0, s, (const CellGrid*)w.grids, w.cell_cnt, w.cell_cur);
    hipLaunchKernelGGL(k_grid_scatter<CtPayload>, dim3(nb), dim3(256), 0, s, n_total, n_struct, (const int*)w.offsets, X, (const CellGrid*)w.grids,
                       (const int*)w.cell_of, w.cell_cur, w.sorted, CtPayload{subunit, w.sorted_sub});
    // count -> per-atom ranges -> emit in (a, b) order
    hipLaunchKernelGGL(k_ct_pairs<false>, dim3(nb), dim3(256), 0, s, n_total, n_struct, (const int*)w.offsets, (const CellGrid*)w.grids,
                       (const int*)w.cell_cnt, (const float4*)w.sorted, (const int*)w.sorted_sub, r_thr, w.off, ties_out, (const int*)nullptr,
                       (const CtState*)w.st, (int*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.off, n_total, (const int*)nullptr, &w.st->K);
    hipLaunchKernelGGL(k_ct_finish, dim3(1), dim3(1), 0, s, w.st, w.off, n_total);
    hipLaunchKernelGGL(k_ct_sizes, dim3(1), dim3(1), 0, s, w.st, (long long)cap_pairs);
    hipLaunchKernelGGL(k_ct_pairs<true>, dim3(nb), dim3(256), 0, s, n_total, n_struct, (const int*)w.offsets, (const CellGrid*)w.grids,
                       (const int*)w.cell_cnt, (const float4*)w.sorted, (const int*)w.sorted_sub, r_thr, (int*)nullptr, (unsigned char*)nullptr,
                       (const int*)w.off, (const CtState*)w.st, w.pb, w.pd);
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

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_contacts_last_error(void) { return last_error(); }

int pesto_contacts(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, int32_t n_sub, const float* X,
                   const int32_t* subunit, const int32_t* residue, const int32_t* type, int32_t n_types, float r_thr, int64_t cap_pairs,
                   int64_t cap_groups, int32_t* pairs_out, float* d_out, int32_t* groups_out, uint16_t* keys_out, uint16_t* rkeys_out,
                   uint8_t* T_out, uint8_t* ties_out, int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (n_total < 1 || n_total > 0x3ffffff0 || n_struct < 1 || n_sub < 1 || n_sub > 0xffff || !struct_offsets || !X || !subunit || !residue ||
        !type || !sizes_out || !ties_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (n_types < 1 || n_types > (1 << CT_TYPE_BITS)) return fail(PESTO_ERR_INVALID, "n_types must be in [1, %d]", 1 << CT_TYPE_BITS);
    if (cap_pairs < 1 || cap_pairs > 0x3fffffff || cap_groups < 1 || cap_groups > 0x3fffff)
        return fail(PESTO_ERR_INVALID, "cap_pairs must be in [1, 2^30), cap_groups in [1, 2^22)");
    if (!pairs_out || !d_out || !groups_out || !keys_out || !rkeys_out || !T_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (!(r_thr > 0.f) || !std::isfinite(r_thr)) return fail(PESTO_ERR_INVALID, "r_thr must be a positive finite distance");
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (int rc = check_offsets(struct_offsets, n_struct, n_total, "struct_offsets", "assembly")) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t n = (size_t)n_total, C = (size_t)cap_pairs, Cg = (size_t)cap_groups, nt2 = (size_t)n_types * n_types;
    const size_t cells = cells_before(n, (size_t)n_struct), tiles = (C + RS_TILE - 1) / RS_TILE;
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iX = bf.input(X, n * 12), iS = bf.input(subunit, n * 4),
              iR = bf.input(residue, n * 4), iT = bf.input(type, n * 4);
    // the outputs come back as far as the counters say they were filled; ties whole
    const int iP = bf.partial(pairs_out, C * 8), iD = bf.partial(d_out, C * 4), iGr = bf.partial(groups_out, Cg * 16), iK = bf.partial(keys_out, C * 8),
              iRk = bf.partial(rkeys_out, C * 8), iTt = bf.partial(T_out, Cg * nt2), iTi = bf.output(ties_out, n);
    const int iSt = bf.scratch(sizeof(CtState)), iG = bf.scratch((size_t)n_struct * sizeof(CellGrid)), iCnt = bf.scratch(cells * 4),
              iCur = bf.scratch(cells * 4), iCell = bf.scratch(n * 4), iSort = bf.scratch(n * 16), iSub = bf.scratch(n * 4),
              iAOff = bf.scratch((n + 1) * 4), iPb = bf.scratch(C * 4), iPd = bf.scratch(C * 4), iGk = bf.scratch(C * 8), iTk = bf.scratch(C * 8),
              iRk8 = bf.scratch(C * 8), iTmp = bf.scratch(C * 8), iFlag = bf.scratch(C * 4), iHist = bf.scratch(256 * tiles * 4);
    CtState hs = {};
    int rc = bf.upload();
    if (rc == 0) rc = hip_ok(hipMemsetAsync(bf.ptr<CtState>(iSt), 0, sizeof(CtState), bf.stm), "contacts");
    if (rc == 0) {
        typedef unsigned long long u64;
        const CtBuffers b{bf.ptr<int>(iOff), bf.ptr<CtState>(iSt), bf.ptr<CellGrid>(iG), bf.ptr<int>(iCnt), bf.ptr<int>(iCur), bf.ptr<int>(iCell),
                          bf.ptr<float4>(iSort), bf.ptr<int>(iSub), bf.ptr<int>(iAOff), bf.ptr<int>(iPb), bf.ptr<float>(iPd), bf.ptr<u64>(iGk),
                          bf.ptr<u64>(iTk), bf.ptr<u64>(iRk8), bf.ptr<u64>(iTmp), bf.ptr<int>(iFlag), bf.ptr<int>(iHist)};
        launch_contacts(bf.stm, (int)n_total, n_struct, n_sub, bf.ptr<const float>(iX), bf.ptr<const int>(iS), bf.ptr<const int>(iR),
                        bf.ptr<const int>(iT), n_types, r_thr, (int)C, (int)Cg, b, bf.ptr<int>(iP), bf.ptr<float>(iD), bf.ptr<int>(iGr),
                        bf.ptr<unsigned short>(iK), bf.ptr<unsigned short>(iRk), bf.ptr<unsigned char>(iTt), bf.ptr<unsigned char>(iTi));
        rc = hip_ok(hipGetLastError(), "contacts: launch failed");
    }
    // the one synchronisation for sizing: the counters
    if (rc == 0) rc = bf.read(iSt, &hs, sizeof(CtState));
    if (rc == 0) rc = hip_ok(hipStreamSynchronize(bf.stm), "contacts: stream synchronisation failed");
    if (rc == 0) {
        const bool fits = hs.n_sort == hs.K;
        sizes_out[0] = hs.K;
        sizes_out[1] = fits ? hs.G : -1;
        sizes_out[2] = fits ? hs.U2 : -1;
        if (fits) {
            const size_t K = (size_t)hs.K, U = (size_t)hs.U2, G = (size_t)hs.G <= Cg ? (size_t)hs.G : 0;
            const struct { int item; size_t bytes; } filled[] = {{iP, K * 8}, {iD, K * 4}, {iK, U * 8}, {iRk, U * 8}, {iGr, G * 16}, {iTt, G * nt2}};
            for (const auto& f : filled)
                if (rc == 0) rc = bf.fetch(f.item, f.bytes);
        }
    }
    rc = bf.finish(rc, "contacts");
    if (rc == 0 && (hs.err & 1))
        rc = fail(PESTO_ERR_INVALID, "subunit: ids must lie in [0, n_sub), ascend along the atoms and change between assemblies");
    if (rc == 0 && (hs.err & 2)) rc = fail(PESTO_ERR_INVALID, "residue must lie in [0, 8192) and type in [-1, n_types)");
    return rc;
}
