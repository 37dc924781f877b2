// pesto_contacts.hip - the contact side of the reference's dataset build: every atom pair closer than r_thr between two subunits of an
// assembly, in the reference's order and fp32 rounding, and the typed residue-residue contact keys of each pair of subunits.
//
// replaces: extract_all_contacts / locate_contacts (src/data_encoding.py:116-167; one dense torch distance matrix per pair of subunits) and
// contacts_types + pack_contacts_data (processing/build_dataset.py:41-83; a dense [R0, R1, 79, 79] bool map per pair, then torch.where).
// One launch sequence for a batch of assemblies:
//   grid     a uniform cell grid per assembly (pesto_cellgrid.h); its count pass also checks the per-atom contract of the call
//   count    one thread per atom a: partners b with subunit[b] > subunit[a] and d < r_thr; exclusive scan -> each atom's slot range
//   emit     the same search writes (b, d) into a's range and sorts the (short) range by b: the pairs in (a, b) order
//   regroup  the stable radix sort of pesto_radix.h on (subunit[a], subunit[b], position) keys: the reference's per-(i, j) lists, a then b ascending
//   keys     (group, r0, r1 | t0, t1) of every pair, the same sort, the last contact of each residue pair -> sorted Y keys, T;
//            the swapped (group, r1, r0 | t1, t0) sorted again
// Every step is deterministic: the scans and sorts fix the order, and the only atomics are counters and idempotent stores.
#include <cmath>

#include "pesto_call.h"
#include "pesto_cellgrid.h"
#include "pesto_radix.h"

namespace pesto {

namespace {

constexpr int CT_RES_BITS = 13, CT_TYPE_BITS = 7;
constexpr int CT_KEY_G = 42, CT_KEY_R0 = 29, CT_KEY_R1 = 16;       // the fields of the typed keys (k_ct_type_keys)
// radix passes of the regroup (the subunit pair, bits 32..63 of the pair keys) and of the two typed sorts (bits CT_KEY_R1..63)
constexpr int CT_GROUP_PASSES = 4, CT_TYPED_PASSES = (64 - CT_KEY_R1) / 8;

// the device counters of one call
struct CtState {
    int K;            // contacts
    int n_sort;       // K when it fits the capacity, else 0 (every later stage then has nothing to do)
    int G;            // (i, j) groups
    int U2;           // typed keys (residue pairs whose last contact is typed), per direction
    int err;          // bit 0: subunit ids not ascending / out of range; bit 1: residue or type out of range
    RadixState rs;    // of the three sorts, one after the other (launch_contacts)
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

// ------------------------------------------------------------------------------------------------ regroup and typed keys
// sort key of pair k (in (a, b) order): subunit[a] | subunit[b] | k
__global__ __launch_bounds__(256) void k_ct_pair_keys(const CtState* __restrict__ st, int n_total, const int* __restrict__ off,
                                                      const int* __restrict__ subunit, const int* __restrict__ pb, u64* __restrict__ keys) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n_total || st->n_sort == 0) return;
    const u64 sa = (unsigned)subunit[a] & 0xffffu;
    for (int k = off[a], e = off[a + 1]; k < e; ++k)
        keys[k] = (sa << 48) | ((u64)((unsigned)subunit[pb[k]] & 0xffffu) << 32) | (u64)k;
}

// the pairs in group order (a recovered from the position through the per-atom offsets), group-start flags
__global__ __launch_bounds__(256) void k_ct_gather(const CtState* __restrict__ st, int n_total, const int* __restrict__ off,
                                                   const u64* __restrict__ gkeys, const u64* __restrict__ tmp, const int* __restrict__ pb,
                                                   const float* __restrict__ pd, int* __restrict__ pairs_out, float* __restrict__ d_out,
                                                   int* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= st->n_sort) return;
    const u64* keys = radix_sorted(gkeys, tmp, CT_GROUP_PASSES, &st->rs);
    const u64 key = keys[k];
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

// group table (subunit i, subunit j, first pair) and the key of every contact
__global__ __launch_bounds__(256) void k_ct_type_keys(const CtState* __restrict__ st, const int* __restrict__ pairs, const int* __restrict__ gid_excl,
                                                      const u64* __restrict__ gkeys_a, const u64* __restrict__ tmp,
                                                      const int* __restrict__ residue, const int* __restrict__ type, int n_types,
                                                      long long cap_groups, int* __restrict__ groups, u64* __restrict__ tkeys) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K) return;
    const u64* gkeys = radix_sorted(gkeys_a, tmp, CT_GROUP_PASSES, &st->rs);
    const int a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    // gid_excl: the exclusive scan of the group-start flags, so the group of k is gid_excl[k] - 1 + (k starts a group)
    const bool first = k == 0 || (gkeys[k - 1] >> 32) != (gkeys[k] >> 32);
    const int g = gid_excl[k] + (first ? 1 : 0) - 1;
    if (first && g < cap_groups) {
        const u64 key = gkeys[k];
        groups[4 * (size_t)g] = (int)(key >> 48);
        groups[4 * (size_t)g + 1] = (int)((key >> 32) & 0xffff);
        groups[4 * (size_t)g + 2] = k;
    }
    const int ta = type[a], tb = type[b];
    const unsigned ra = (unsigned)residue[a] & 0x1fffu, rb = (unsigned)residue[b] & 0x1fffu;        // (out of range: reported, masked)
    const bool typed = ta >= 0 && tb >= 0 && ta < n_types && tb < n_types;
    tkeys[k] = ((u64)(g & 0x3fffff) << CT_KEY_G) | ((u64)ra << CT_KEY_R0) | ((u64)rb << CT_KEY_R1) | (typed ? (u64)((ta << 8) | tb) : 0xffffull);
}

// 1 where k is the last contact of its residue pair and that contact is typed
__global__ __launch_bounds__(256) void k_ct_last_flags(const CtState* __restrict__ st, const u64* __restrict__ tkeys_a, const u64* __restrict__ tmp,
                                                       int* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K) return;
    const u64* tkeys = radix_sorted(tkeys_a, tmp, CT_TYPED_PASSES, &st->rs);
    const u64 key = tkeys[k];
    const bool last = k + 1 == K || (tkeys[k + 1] >> CT_KEY_R1) != (key >> CT_KEY_R1);
    flag[k] = (last && (key & 0xffffull) != 0xffffull) ? 1 : 0;
}

// forward rows (r0, r1, t0, t1), per group the key count and T[t0][t1], and the swapped keys for their own sort
__global__ __launch_bounds__(256) void k_ct_write_fwd(const CtState* __restrict__ st, const u64* __restrict__ tkeys_a, const u64* __restrict__ tmp,
                                                      const int* __restrict__ pos, int n_types, long long cap_groups, unsigned short* __restrict__ keys_out,
                                                      int* __restrict__ groups, unsigned char* __restrict__ T, u64* __restrict__ rkeys) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int K = st->n_sort;
    if (k >= K || st->G > cap_groups) return;
    const u64* tkeys = radix_sorted(tkeys_a, tmp, CT_TYPED_PASSES, &st->rs);
    const u64 key = tkeys[k];
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
    rkeys[u] = ((u64)g << CT_KEY_G) | ((u64)r1 << CT_KEY_R0) | ((u64)r0 << CT_KEY_R1) | (u64)((t1 << 8) | t0);
}

// swapped rows (r1, r0, t1, t0) from their sorted keys
__global__ __launch_bounds__(256) void k_ct_write_rev(const CtState* __restrict__ st, long long cap_groups, const u64* __restrict__ rkeys,
                                                      const u64* __restrict__ tmp, unsigned short* __restrict__ rkeys_out) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= st->U2 || st->G > cap_groups) return;
    const u64 key = radix_sorted(rkeys, tmp, CT_TYPED_PASSES, &st->rs)[u];
    unsigned short* row = rkeys_out + 4 * (size_t)u;
    row[0] = (unsigned short)((key >> CT_KEY_R0) & 0x1fffu); row[1] = (unsigned short)((key >> CT_KEY_R1) & 0x1fffu);
    row[2] = (unsigned short)((key >> 8) & 0xffu); row[3] = (unsigned short)(key & 0xffu);
}

__global__ void k_ct_finish(CtState* st, int* off, int n_total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) off[n_total] = st->K;
}

struct CtBuffers {
    int* offsets; CtState* st; CellGrid* grids; int* cell_cnt; int* cell_cur; int* cell_of; float4* sorted; int* sorted_sub; int* off;
    int* pb; float* pd; u64* gkeys; u64* tkeys; u64* rkeys; u64* tmp; int* flag; int* hist;
};

void launch_contacts(hipStream_t s, int n_total, int n_struct, int n_sub, const float* X, const int* subunit, const int* residue, const int* type,
                     int n_types, float r_thr, int cap_pairs, int cap_groups, const CtBuffers& w, int* pairs_out, float* d_out, int* groups_out,
                     unsigned short* keys_out, unsigned short* rkeys_out, unsigned char* T_out, unsigned char* ties_out) {
    const int nb = (n_total + 255) / 256, nbk = (cap_pairs + 255) / 256;
    grid_build(s, n_total, n_struct, (const int*)w.offsets, X, r_thr, GridBufs{w.grids, w.cell_cnt, w.cell_cur, w.cell_of, w.sorted},
               CtCheck{w.offsets, subunit, residue, type, n_sub, n_types, w.st}, CtPayload{subunit, w.sorted_sub});
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
    // The three sorts share the second buffer w.tmp and the state w.st->rs, and a sort may leave its result in either buffer (a skipped
    // pass moves nothing). That is sound because the stream runs every reader of a sorted array (radix_sorted) before the next sort's
    // first launch writes w.tmp or the state: gkeys is last read by k_ct_type_keys, tkeys by k_ct_write_fwd, rkeys by k_ct_write_rev.
    // regroup by (subunit[a], subunit[b]): the low 32 bits (the position) are in order already
    hipLaunchKernelGGL(k_ct_pair_keys, dim3(nb), dim3(256), 0, s, (const CtState*)w.st, n_total, (const int*)w.off, subunit, (const int*)w.pb,
                       w.gkeys);
    radix_sort(s, w.gkeys, w.tmp, cap_pairs, &w.st->n_sort, 32, CT_GROUP_PASSES, w.hist, &w.st->rs);
    hipLaunchKernelGGL(k_ct_gather, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, n_total, (const int*)w.off, (const u64*)w.gkeys,
                       (const u64*)w.tmp, (const int*)w.pb, (const float*)w.pd, pairs_out, d_out, w.flag);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.flag, 0, &w.st->n_sort, &w.st->G);
    hipLaunchKernelGGL(k_ct_type_keys, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const int*)pairs_out, (const int*)w.flag,
                       (const u64*)w.gkeys, (const u64*)w.tmp, residue, type, n_types, (long long)cap_groups, groups_out, w.tkeys);
    // typed keys: stable sort on (group, r0, r1), the last of each run, the swapped keys sorted again
    radix_sort(s, w.tkeys, w.tmp, cap_pairs, &w.st->n_sort, CT_KEY_R1, CT_TYPED_PASSES, w.hist, &w.st->rs);
    hipLaunchKernelGGL(k_ct_last_flags, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const u64*)w.tkeys, (const u64*)w.tmp, w.flag);
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, w.flag, 0, &w.st->n_sort, &w.st->U2);
    hipLaunchKernelGGL(k_ct_write_fwd, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (const u64*)w.tkeys, (const u64*)w.tmp, (const int*)w.flag,
                       n_types, (long long)cap_groups, keys_out, groups_out, T_out, w.rkeys);
    radix_sort(s, w.rkeys, w.tmp, cap_pairs, &w.st->U2, CT_KEY_R1, CT_TYPED_PASSES, w.hist, &w.st->rs);
    hipLaunchKernelGGL(k_ct_write_rev, dim3(nbk), dim3(256), 0, s, (const CtState*)w.st, (long long)cap_groups, (const u64*)w.rkeys,
                       (const u64*)w.tmp, rkeys_out);
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
    const size_t cells = cells_before(n, (size_t)n_struct);
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iX = bf.input(X, n * 12), iS = bf.input(subunit, n * 4),
              iR = bf.input(residue, n * 4), iT = bf.input(type, n * 4);
    // the outputs come back as far as the counters say they were filled; ties whole. The groups and their type matrices start at zero.
    const int iP = bf.partial(pairs_out, C * 8), iD = bf.partial(d_out, C * 4), iGr = bf.partial(groups_out, Cg * 16, 0), iK = bf.partial(keys_out, C * 8),
              iRk = bf.partial(rkeys_out, C * 8), iTt = bf.partial(T_out, Cg * nt2, 0), iTi = bf.output(ties_out, n);
    const int iSt = bf.scratch(sizeof(CtState), 0), iG = bf.scratch((size_t)n_struct * sizeof(CellGrid)), iCnt = bf.scratch(cells * 4),
              iCur = bf.scratch(cells * 4), iCell = bf.scratch(n * 4), iSort = bf.scratch(n * 16), iSub = bf.scratch(n * 4),
              iAOff = bf.scratch((n + 1) * 4), iPb = bf.scratch(C * 4), iPd = bf.scratch(C * 4), iGk = bf.scratch(C * 8), iTk = bf.scratch(C * 8),
              iRk8 = bf.scratch(C * 8), iTmp = bf.scratch(C * 8), iFlag = bf.scratch(C * 4), iHist = bf.scratch(radix_counter_bytes(C));
    CtState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const CtBuffers b{bf.ptr<int>(iOff), bf.ptr<CtState>(iSt), bf.ptr<CellGrid>(iG), bf.ptr<int>(iCnt), bf.ptr<int>(iCur), bf.ptr<int>(iCell),
                          bf.ptr<float4>(iSort), bf.ptr<int>(iSub), bf.ptr<int>(iAOff), bf.ptr<int>(iPb), bf.ptr<float>(iPd), bf.ptr<u64>(iGk),
                          bf.ptr<u64>(iTk), bf.ptr<u64>(iRk8), bf.ptr<u64>(iTmp), bf.ptr<int>(iFlag), bf.ptr<int>(iHist)};
        launch_contacts(bf.stm, (int)n_total, n_struct, n_sub, bf.ptr<const float>(iX), bf.ptr<const int>(iS), bf.ptr<const int>(iR),
                        bf.ptr<const int>(iT), n_types, r_thr, (int)C, (int)Cg, b, bf.ptr<int>(iP), bf.ptr<float>(iD), bf.ptr<int>(iGr),
                        bf.ptr<unsigned short>(iK), bf.ptr<unsigned short>(iRk), bf.ptr<unsigned char>(iTt), bf.ptr<unsigned char>(iTi));
    }
    // the one synchronisation for sizing: the counters
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "contacts");
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
