// pesto_rank.hip - ranking curves and pooled scores: what the reference's evaluation notebooks take from sklearn (metrics.roc_curve,
// metrics.precision_recall_curve with metrics.auc, metrics.f1_score, label-split confidence histograms) for columns of 10^5 to 10^7 pooled
// residues, where the all-pairs AUC of k_bc_scores (pesto_eval.hip) is quadratic.
//
// A column is one (segment, class) pair of y uint8 [R,C], p float32 [R,C] and res_offsets [S+1]: col = s * C + c. Every element becomes
// one 64-bit key
//     col << 33 | desc(p) << 1 | y
// desc being the order-preserving map of the float's bits, complemented (larger scores first), -0.0 canonicalised to +0.0. All columns are
// sorted at once by the LSD radix sort of pesto_radix.h, from bit 0 up (the sorted keys are where radix_sorted() says). The label rides in
// the low bit: there is no payload, and the order inside a group of equal scores is irrelevant because every output is a per-group total.
//
// After the sort everything is integer arithmetic. Column col of segment s starts at res_offsets[s] * C + c * R_s. The group ends (desc
// or the column changes) are the distinct thresholds; an inclusive scan of y over the sorted array gives at the k-th of a column
//     tps[k]                          and   fps[k] = (rank in the column) - tps[k]
// which are sklearn's _binary_clf_curve. They are kept as two compact arrays over all group ends (pt_pos, pt_tp) with the first point
// and the y total before each column (col_pt0, col_y0); the scores, the curves and the histograms are read from those.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h and the list protocol of pesto_scan.h.
#include <cmath>

#include "pesto_call.h"
#include "pesto_radix.h"

namespace pesto {

namespace {

constexpr int RK_NT = RADIX_NT;                  // threads per workgroup of every kernel here but the scans
constexpr int RK_TILE = PESTO_RANK_TILE;         // keys per workgroup of the kernels after the sort, which walk its tiles
static_assert(RK_TILE == RADIX_TILE && RK_NT * RADIX_ITEMS == RK_TILE, "the tiles of the sort, RADIX_ITEMS keys per thread");

// the device state of one call: the list protocol's counters (err bit 0: a non-finite p), the number of keys (k_rank_keys writes it
// for the sort, which reads its length on the device) and the sort's own state
struct RankState {
    ListState ls;       // (first: the item of a RankState is the call's ListState to list_offsets)
    int n;
    RadixState rs;
};

__device__ __forceinline__ unsigned rk_desc(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;                                   // -0.0 and +0.0 are one threshold
    const unsigned asc = (u >> 31) ? ~u : (u | 0x80000000u);
    return ~asc;
}

__device__ __forceinline__ float rk_score(unsigned desc) {
    const unsigned asc = ~desc;
    return __uint_as_float((asc >> 31) ? (asc & 0x7fffffffu) : ~asc);
}

__device__ __forceinline__ unsigned rk_desc_of(u64 key) { return (unsigned)(key >> 1); }

// ------------------------------------------------------------------------------------------------ keys
__global__ __launch_bounds__(RK_NT) void k_rank_keys(long long n, int n_class, int n_struct, const int* __restrict__ roff,
                                                     const unsigned char* __restrict__ y, const float* __restrict__ p, u64* __restrict__ keys,
                                                     RankState* __restrict__ st) {
    const long long e = (long long)blockIdx.x * RK_NT + threadIdx.x;
    if (e >= n) return;
    if (e == 0) st->n = (int)n;
    const int r = (int)(e / n_class), c = (int)(e - (long long)r * n_class);
    const int s = struct_of(r, n_struct, roff);
    const float v = p[e];
    if (!(fabsf(v) <= 3.402823466e38f)) atomicOr(&st->ls.err, 1);
    const u64 col = (u64)s * (u64)n_class + (u64)c;
    keys[e] = col << 33 | (u64)rk_desc(v) << 1 | (u64)(y[e] != 0);
}

// ------------------------------------------------------------------------------------------------ group ends and the scan of y
__device__ __forceinline__ bool rk_group_end(const u64* __restrict__ keys, long long j, long long n) {
    return j + 1 >= n || (keys[j] >> 1) != (keys[j + 1] >> 1);
}

// per tile: the positives and the group ends
__global__ __launch_bounds__(RK_NT) void k_rank_tile_sums(long long n, const u64* __restrict__ keys_a, const u64* __restrict__ keys_b, int n_pass,
                                                          const RankState* __restrict__ st, int* __restrict__ tile_y, int* __restrict__ tile_g) {
    __shared__ int sums[2];
    const u64* keys = radix_sorted(keys_a, keys_b, n_pass, &st->rs);
    if (threadIdx.x < 2) sums[threadIdx.x] = 0;
    __syncthreads();
    const long long j0 = (long long)blockIdx.x * RK_TILE + threadIdx.x * RADIX_ITEMS;
    int ny = 0, ng = 0;
    for (int i = 0; i < RADIX_ITEMS; ++i) {
        const long long j = j0 + i;
        if (j >= n) break;
        ny += (int)(keys[j] & 1ull);
        ng += rk_group_end(keys, j, n);
    }
    atomicAdd(&sums[0], ny);
    atomicAdd(&sums[1], ng);
    __syncthreads();
    if (threadIdx.x == 0) { tile_y[blockIdx.x] = sums[0]; tile_g[blockIdx.x] = sums[1]; }
}

// one workgroup: both tile arrays scanned in place; col_pt0[n_col] = the number of group ends
__global__ __launch_bounds__(1024) void k_rank_tile_scan(int n_tiles, int* __restrict__ tile_y, int* __restrict__ tile_g, int* __restrict__ col_pt0_end) {
    block_scan_exclusive<1024, false>(tile_y, n_tiles);
    __syncthreads();
    const int total = block_scan_exclusive<1024, false>(tile_g, n_tiles);
    if (threadIdx.x == 0) *col_pt0_end = total;
}

// per tile again, now with the tiles' bases: the g-th group end of the sorted array at position j gives pt_pos[g] = j and pt_tp[g] = the
// inclusive scan of y at j; a column's first element gives col_pt0[col] (group ends before it) and col_y0[col] (positives before it)
__global__ __launch_bounds__(RK_NT) void k_rank_points(long long n, const u64* __restrict__ keys_a, const u64* __restrict__ keys_b, int n_pass,
                                                       const RankState* __restrict__ st, const int* __restrict__ tile_y, const int* __restrict__ tile_g,
                                                       long long n_col, int* __restrict__ pt_pos, int* __restrict__ pt_tp,
                                                       int* __restrict__ col_pt0, int* __restrict__ col_y0) {
    __shared__ int packed[RK_NT];                  // positives << 16 | group ends of each thread's RADIX_ITEMS keys: both at most RK_TILE
    const u64* keys = radix_sorted(keys_a, keys_b, n_pass, &st->rs);
    const long long j0 = (long long)blockIdx.x * RK_TILE + threadIdx.x * RADIX_ITEMS;
    int ny = 0, ng = 0;
    for (int i = 0; i < RADIX_ITEMS; ++i) {
        const long long j = j0 + i;
        if (j >= n) break;
        ny += (int)(keys[j] & 1ull);
        ng += rk_group_end(keys, j, n);
    }
    packed[threadIdx.x] = ny << 16 | ng;
    __syncthreads();
    block_scan_exclusive<RK_NT, false>(packed, RK_NT);
    const int before = packed[threadIdx.x];
    int ycum = tile_y[blockIdx.x] + (before >> 16), g = tile_g[blockIdx.x] + (before & 0xffff);
    for (int i = 0; i < RADIX_ITEMS; ++i) {
        const long long j = j0 + i;
        if (j >= n) break;
        const u64 key = keys[j];
        const long long col = (long long)(key >> 33);
        if ((j == 0 || (key >> 33) != (keys[j - 1] >> 33)) && col < n_col) { col_pt0[col] = g; col_y0[col] = ycum; }
        ycum += (int)(key & 1ull);
        if (rk_group_end(keys, j, n)) { pt_pos[g] = (int)j; pt_tp[g] = ycum; ++g; }
    }
}

// ------------------------------------------------------------------------------------------------ one column's points
// tps / fps of the k-th distinct threshold of a column, k in [0, K); (0, 0) before the first
struct Column {
    const u64* keys; const int* pos; const int* tp;
    long long start;          // the column's first sorted position
    int g0, K, y0, rows;
    __device__ long long tps(int k) const { return k < 0 ? 0 : (long long)(tp[g0 + k] - y0); }
    __device__ long long fps(int k) const { return k < 0 ? 0 : ((long long)pos[g0 + k] - start + 1) - (long long)(tp[g0 + k] - y0); }
    __device__ unsigned desc(int k) const { return rk_desc_of(keys[pos[g0 + k]]); }
    // roc_curve's drop_intermediate: the ends, and where the second difference of fps or of tps is not zero
    __device__ bool corner(int k) const {
        if (k == 0 || k == K - 1) return true;
        return tps(k + 1) - 2 * tps(k) + tps(k - 1) != 0 || fps(k + 1) - 2 * fps(k) + fps(k - 1) != 0;
    }
};

__device__ __forceinline__ Column rk_column(long long col, int n_class, const int* __restrict__ roff, const u64* keys, const int* pt_pos,
                                            const int* pt_tp, const int* __restrict__ col_pt0, const int* __restrict__ col_y0) {
    const int s = (int)(col / n_class), c = (int)(col - (long long)s * n_class);
    Column v;
    v.keys = keys; v.pos = pt_pos; v.tp = pt_tp;
    v.rows = roff[s + 1] - roff[s];
    v.start = (long long)roff[s] * n_class + (long long)c * v.rows;
    v.g0 = col_pt0[col]; v.K = col_pt0[col + 1] - v.g0; v.y0 = col_y0[col];
    return v;
}

// sum over the workgroup in a fixed order (a tree over LDS): the same bits from call to call, for the float64 sum too
template <typename T>
__device__ __forceinline__ T rk_block_sum(T v, T* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = RK_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// ------------------------------------------------------------------------------------------------ scores
// one workgroup per column, every thread a contiguous run of its points. counts int64 [S,6,C]: P, N, TP, FP (q = rintf(p), as
// k_bc_scores), K, K_roc; scores float64 [S,3,C]: roc_auc, pr_auc, f1
__global__ __launch_bounds__(RK_NT) void k_rank_scores(int n_class, const int* __restrict__ roff, const u64* __restrict__ keys_a,
                                                       const u64* __restrict__ keys_b, int n_pass, const RankState* __restrict__ st,
                                                       const int* __restrict__ pt_pos, const int* __restrict__ pt_tp,
                                                       const int* __restrict__ col_pt0, const int* __restrict__ col_y0,
                                                       long long* __restrict__ counts, double* __restrict__ scores) {
    __shared__ long long red_i[RK_NT];
    __shared__ u64 red_u[RK_NT];
    __shared__ double red_d[RK_NT];
    const long long col = blockIdx.x;
    const Column v = rk_column(col, n_class, roff, radix_sorted(keys_a, keys_b, n_pass, &st->rs), pt_pos, pt_tp, col_pt0, col_y0);
    const long long P = v.tps(v.K - 1), N = v.rows - P;
    const long long per = ((long long)v.K + RK_NT - 1) / RK_NT;          // (64 bits: K may be within RK_NT of 2^31)
    const int k0 = (int)min((long long)v.K, (long long)threadIdx.x * per), k1 = (int)min((long long)v.K, k0 + per);
    long long tp = 0, fp = 0, kroc = 0;
    u64 u2 = 0;
    double area = 0.0;
    const double dP = (double)P;
    for (int k = k0; k < k1; ++k) {
        const long long t1 = v.tps(k), f1 = v.fps(k), t0 = v.tps(k - 1), f0 = v.fps(k - 1);
        u2 += (u64)(f1 - f0) * (u64)(t1 + t0);
        if (rintf(rk_score(v.desc(k))) != 0.f) { tp += t1 - t0; fp += f1 - f0; }
        kroc += v.corner(k);
        // the trapezoid of precision over recall from the closing point (recall 0, precision 1) upwards
        const double rec1 = (double)t1 / dP, rec0 = (double)t0 / dP;
        const double pre1 = (double)t1 / (double)(t1 + f1), pre0 = k > 0 ? (double)t0 / (double)(t0 + f0) : 1.0;
        const double dx = rec1 - rec0, sy = pre1 + pre0;
        const double term = dx * sy / 2.0;
        area = area + term;
    }
    const long long TP = rk_block_sum(tp, red_i), FP = rk_block_sum(fp, red_i), Kroc = rk_block_sum(kroc, red_i);
    const u64 U2 = rk_block_sum(u2, red_u);
    const double A = rk_block_sum(area, red_d);
    if (threadIdx.x != 0) return;
    const int s = (int)(col / n_class), c = (int)(col - (long long)s * n_class);
    long long* o = counts + (size_t)s * 6 * n_class + c;
    o[0 * n_class] = P; o[1 * n_class] = N; o[2 * n_class] = TP; o[3 * n_class] = FP; o[4 * n_class] = v.K; o[5 * n_class] = Kroc;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double* q = scores + (size_t)s * 3 * n_class + c;
    q[0 * n_class] = (P > 0 && N > 0) ? (double)U2 / (2.0 * (double)P * (double)N) : qnan;
    q[1 * n_class] = P > 0 ? A : qnan;
    const long long den = 2 * TP + FP + (P - TP);
    q[2 * n_class] = den ? (double)(2 * TP) / (double)den : 0.0;
}

// ------------------------------------------------------------------------------------------------ curves
// one workgroup per column, every thread a contiguous run of its points; mode 0 keeps every point, mode 1 the corners. EMIT false: the
// column's count to cnt[col]; true: thr / tps / fps from off[col], when the list fits the capacity
template <bool EMIT>
__global__ __launch_bounds__(RK_NT) void k_rank_curve(int n_class, int mode, const int* __restrict__ roff, const u64* __restrict__ keys_a,
                                                      const u64* __restrict__ keys_b, int n_pass, const RankState* __restrict__ st,
                                                      const int* __restrict__ pt_pos, const int* __restrict__ pt_tp,
                                                      const int* __restrict__ col_pt0, const int* __restrict__ col_y0, int* __restrict__ cnt,
                                                      const long long* __restrict__ off, float* __restrict__ thr, long long* __restrict__ tps,
                                                      long long* __restrict__ fps) {
    __shared__ int kept[RK_NT];
    if (EMIT && !st->ls.fits) return;
    const long long col = blockIdx.x;
    const Column v = rk_column(col, n_class, roff, radix_sorted(keys_a, keys_b, n_pass, &st->rs), pt_pos, pt_tp, col_pt0, col_y0);
    const long long per = ((long long)v.K + RK_NT - 1) / RK_NT;          // (64 bits: K may be within RK_NT of 2^31)
    const int k0 = (int)min((long long)v.K, (long long)threadIdx.x * per), k1 = (int)min((long long)v.K, k0 + per);
    int mine = 0;
    for (int k = k0; k < k1; ++k) mine += mode == 0 || v.corner(k);
    kept[threadIdx.x] = mine;
    __syncthreads();
    const int total = block_scan_exclusive<RK_NT, false>(kept, RK_NT);
    if (!EMIT) {
        if (threadIdx.x == 0) cnt[col] = total;
        return;
    }
    long long at = off[col] + kept[threadIdx.x];
    for (int k = k0; k < k1; ++k) {
        if (!(mode == 0 || v.corner(k))) continue;
        thr[at] = rk_score(v.desc(k)); tps[at] = v.tps(k); fps[at] = v.fps(k);
        ++at;
    }
}

// ------------------------------------------------------------------------------------------------ histograms
// the (rows, positives) of a column with p >= e (strict: p > e): a binary search of the thresholds, which descend
__device__ __forceinline__ void rk_at_least(const Column& v, float e, bool strict, long long& rows, long long& pos) {
    const unsigned de = rk_desc(e);
    int lo = 0, hi = v.K;                          // the first k with p_k < e (<= e)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned dk = v.desc(mid);
        if (strict ? dk < de : dk <= de) lo = mid + 1; else hi = mid;
    }
    pos = v.tps(lo - 1);
    rows = pos + v.fps(lo - 1);
}

// one thread per (column, bin): counts int64 [S,C,B,2] = np.histogram(p[y == v], edges) - left-closed bins, the last one closed
__global__ __launch_bounds__(RK_NT) void k_rank_histogram(long long n_cells, int n_class, int n_bins, const int* __restrict__ roff,
                                                          const float* __restrict__ edges, const u64* __restrict__ keys_a,
                                                          const u64* __restrict__ keys_b, int n_pass, const RankState* __restrict__ st,
                                                          const int* __restrict__ pt_pos, const int* __restrict__ pt_tp,
                                                          const int* __restrict__ col_pt0, const int* __restrict__ col_y0,
                                                          long long* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * RK_NT + threadIdx.x;
    if (i >= n_cells) return;
    const long long col = i / n_bins;
    const int b = (int)(i - col * n_bins);
    const Column v = rk_column(col, n_class, roff, radix_sorted(keys_a, keys_b, n_pass, &st->rs), pt_pos, pt_tp, col_pt0, col_y0);
    long long r0, p0, r1, p1;
    rk_at_least(v, edges[b], false, r0, p0);
    rk_at_least(v, edges[b + 1], b == n_bins - 1, r1, p1);
    counts[2 * i] = (r0 - p0) - (r1 - p1);
    counts[2 * i + 1] = p0 - p1;
}

// ------------------------------------------------------------------------------------------------ the host side of one call
struct RankCall {
    long long n;
    int n_struct, n_class, n_tiles, n_pass;
    long long n_col;
    int iOff, iY, iP, iSt, iKa, iKb, iCnt, iTy, iTg, iPos, iTp, iC0, iY0;
    RankState* st(Buffers& bf) const { return bf.ptr<RankState>(iSt); }
};

int rank_check(int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p, int32_t ptr_kind, RankCall& rk) {
    if (n_struct < 1 || n_class < 1 || n_class > 1024 || (int64_t)n_struct * n_class > 0x7fffffff || !res_offsets || !y || !p)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    const int64_t R = res_offsets[n_struct];
    if (R < 1 || R * n_class > 0x7fffffff) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_offsets(res_offsets, n_struct, R, "res_offsets")) return rc;
    rk.n = R * n_class;
    rk.n_struct = n_struct; rk.n_class = n_class;
    rk.n_col = (long long)n_struct * n_class;
    if (rk.n_col > PESTO_RANK_MAX_COLUMNS)
        return fail(PESTO_ERR_INVALID, "n_struct * n_class = %lld columns: at most 2^24 - 1 per call (a workgroup per column, a grid below 2^32 threads)",
                    rk.n_col);
    rk.n_tiles = (int)((rk.n + RK_TILE - 1) / RK_TILE);
    int bits = 33;
    while (bits < 64 && ((rk.n_col - 1) >> (bits - 33)) != 0) ++bits;
    rk.n_pass = (bits + 7) / 8;
    return 0;
}

// the inputs and the scratch of the sort and of the points, declared before upload()
void rank_declare(Buffers& bf, const int32_t* res_offsets, const uint8_t* y, const float* p, RankCall& rk) {
    const size_t n = (size_t)rk.n, nt = (size_t)rk.n_tiles, nc = (size_t)rk.n_col;
    rk.iOff = bf.table(res_offsets, ((size_t)rk.n_struct + 1) * 4);
    rk.iY = bf.input(y, n);
    rk.iP = bf.input(p, n * 4);
    rk.iSt = bf.scratch(sizeof(RankState), 0);
    rk.iKa = bf.scratch(n * 8);
    rk.iKb = bf.scratch(n * 8);
    rk.iCnt = bf.scratch(radix_counter_bytes(n));
    rk.iTy = bf.scratch(nt * 4);
    rk.iTg = bf.scratch(nt * 4);
    rk.iPos = bf.scratch(n * 4);
    rk.iTp = bf.scratch(n * 4);
    rk.iC0 = bf.scratch((nc + 1) * 4);
    rk.iY0 = bf.scratch(nc * 4);
}

// keys -> radix passes -> group ends and the scan of y: 4 + 3 n_pass launches
int rank_sort(Buffers& bf, const RankCall& rk, const char* what) {
    u64 *ka = bf.ptr<u64>(rk.iKa), *kb = bf.ptr<u64>(rk.iKb);
    hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)((rk.n + RK_NT - 1) / RK_NT)), dim3(RK_NT), 0, bf.stm, rk.n, rk.n_class, rk.n_struct,
                       bf.ptr<const int>(rk.iOff), bf.ptr<const unsigned char>(rk.iY), bf.ptr<const float>(rk.iP), ka, rk.st(bf));
    radix_sort(bf.stm, ka, kb, rk.n, &rk.st(bf)->n, 0, rk.n_pass, bf.ptr<int>(rk.iCnt), &rk.st(bf)->rs);
    hipLaunchKernelGGL(k_rank_tile_sums, dim3(rk.n_tiles), dim3(RK_NT), 0, bf.stm, rk.n, (const u64*)ka, (const u64*)kb, rk.n_pass,
                       (const RankState*)rk.st(bf), bf.ptr<int>(rk.iTy), bf.ptr<int>(rk.iTg));
    hipLaunchKernelGGL(k_rank_tile_scan, dim3(1), dim3(1024), 0, bf.stm, rk.n_tiles, bf.ptr<int>(rk.iTy), bf.ptr<int>(rk.iTg),
                       bf.ptr<int>(rk.iC0) + rk.n_col);
    hipLaunchKernelGGL(k_rank_points, dim3(rk.n_tiles), dim3(RK_NT), 0, bf.stm, rk.n, (const u64*)ka, (const u64*)kb, rk.n_pass,
                       (const RankState*)rk.st(bf), bf.ptr<const int>(rk.iTy), bf.ptr<const int>(rk.iTg), rk.n_col, bf.ptr<int>(rk.iPos),
                       bf.ptr<int>(rk.iTp), bf.ptr<int>(rk.iC0), bf.ptr<int>(rk.iY0));
    return bf.launched(what);
}

// what every kernel after the sort takes, in their order
#define RANK_POINTS(bf, rk)                                                                                                                  \
    bf.ptr<const u64>(rk.iKa), bf.ptr<const u64>(rk.iKb), rk.n_pass, (const RankState*)rk.st(bf), bf.ptr<const int>(rk.iPos),                \
        bf.ptr<const int>(rk.iTp), bf.ptr<const int>(rk.iC0), bf.ptr<const int>(rk.iY0)

int rank_finish(Buffers& bf, int rc, const RankState& hs, const char* what) {
    rc = bf.finish(rc, what);
    if (rc == 0 && (hs.ls.err & 1)) rc = fail(PESTO_ERR_INVALID, "%s: p holds a non-finite score (NaN or inf)", what);
    return rc;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_rank_last_error(void) { return last_error(); }

int pesto_rank_scores(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                      int64_t* counts_out, double* scores_out, int32_t ptr_kind, void* stream) {
    RankCall rk;
    if (!counts_out || !scores_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = rank_check(n_struct, res_offsets, n_class, y, p, ptr_kind, rk)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    rank_declare(bf, res_offsets, y, p, rk);
    const int iC = bf.output(counts_out, (size_t)rk.n_col * 6 * 8), iS = bf.output(scores_out, (size_t)rk.n_col * 3 * 8);
    RankState hs = {};
    int rc = bf.upload();
    if (rc == 0) rc = rank_sort(bf, rk, "rank_scores");
    if (rc == 0) {
        hipLaunchKernelGGL(k_rank_scores, dim3((unsigned)rk.n_col), dim3(RK_NT), 0, bf.stm, rk.n_class, bf.ptr<const int>(rk.iOff), RANK_POINTS(bf, rk),
                           bf.ptr<long long>(iC), bf.ptr<double>(iS));
        rc = bf.read(rk.iSt, &hs, sizeof hs);
    }
    return rank_finish(bf, rc, hs, "rank_scores");
}

int pesto_rank_curves(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                      int32_t mode, int64_t capacity, int64_t* offsets_out, float* thr_out, int64_t* tps_out, int64_t* fps_out,
                      int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    RankCall rk;
    if (!offsets_out || !sizes_out || (capacity > 0 && (!thr_out || !tps_out || !fps_out))) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (mode != 0 && mode != 1) return fail(PESTO_ERR_INVALID, "mode must be 0 (every threshold) or 1 (drop_intermediate)");
    if (capacity < 0 || capacity > 0x7fffffff) return fail(PESTO_ERR_INVALID, "capacity must be in [0, 2^31)");
    if (int rc = rank_check(n_struct, res_offsets, n_class, y, p, ptr_kind, rk)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t cap = (size_t)capacity;
    Buffers bf(ptr_kind, stream);
    rank_declare(bf, res_offsets, y, p, rk);
    const int iO = bf.output(offsets_out, ((size_t)rk.n_col + 1) * 8), iT = bf.partial(thr_out, cap * 4), iTps = bf.partial(tps_out, cap * 8),
              iFps = bf.partial(fps_out, cap * 8), iN = bf.scratch((size_t)rk.n_col * 4);
    RankState hs = {};
    int rc = bf.upload();
    if (rc == 0) rc = rank_sort(bf, rk, "rank_curves");
    if (rc == 0) {
        const dim3 grid((unsigned)rk.n_col);
        hipLaunchKernelGGL(k_rank_curve<false>, grid, dim3(RK_NT), 0, bf.stm, rk.n_class, mode, bf.ptr<const int>(rk.iOff), RANK_POINTS(bf, rk),
                           bf.ptr<int>(iN), (const long long*)nullptr, (float*)nullptr, (long long*)nullptr, (long long*)nullptr);
        list_offsets(bf, (int)rk.n_col, iN, iO, (long long)capacity, rk.iSt);
        hipLaunchKernelGGL(k_rank_curve<true>, grid, dim3(RK_NT), 0, bf.stm, rk.n_class, mode, bf.ptr<const int>(rk.iOff), RANK_POINTS(bf, rk),
                           bf.ptr<int>(iN), bf.ptr<const long long>(iO), bf.ptr<float>(iT), bf.ptr<long long>(iTps), bf.ptr<long long>(iFps));
    }
    // the one synchronisation for sizing: the count
    if (rc == 0) rc = bf.verdict(rk.iSt, &hs, sizeof hs, "rank_curves");
    if (rc == 0) rc = list_tail(bf, hs.ls, sizes_out, {{iT, 4}, {iTps, 8}, {iFps, 8}}, !(hs.ls.err & 1));
    return rank_finish(bf, rc, hs, "rank_curves");
}

int pesto_rank_histogram(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                         int32_t n_bins, const float* edges, int64_t* counts_out, int32_t ptr_kind, void* stream) {
    RankCall rk;
    if (!edges || !counts_out || n_bins < 1) return fail(PESTO_ERR_INVALID, "bad arguments");
    for (int b = 0; b < n_bins; ++b)
        if (!(edges[b + 1] > edges[b])) return fail(PESTO_ERR_INVALID, "edges must increase strictly (edge %d)", b + 1);
    if (int rc = rank_check(n_struct, res_offsets, n_class, y, p, ptr_kind, rk)) return rc;
    const long long cells = rk.n_col * n_bins;
    if (cells > 0x7fffffff) return fail(PESTO_ERR_INVALID, "n_struct * n_class * n_bins must stay below 2^31");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    rank_declare(bf, res_offsets, y, p, rk);
    const int iE = bf.table(edges, ((size_t)n_bins + 1) * 4), iC = bf.output(counts_out, (size_t)cells * 2 * 8);
    RankState hs = {};
    int rc = bf.upload();
    if (rc == 0) rc = rank_sort(bf, rk, "rank_histogram");
    if (rc == 0) {
        hipLaunchKernelGGL(k_rank_histogram, dim3((unsigned)((cells + RK_NT - 1) / RK_NT)), dim3(RK_NT), 0, bf.stm, cells, rk.n_class, (int)n_bins,
                           bf.ptr<const int>(rk.iOff), bf.ptr<const float>(iE), RANK_POINTS(bf, rk), bf.ptr<long long>(iC));
        rc = bf.read(rk.iSt, &hs, sizeof hs);
    }
    return rank_finish(bf, rc, hs, "rank_histogram");
}
