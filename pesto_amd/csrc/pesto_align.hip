// pesto_align.hip - pairwise sequence alignment of many pairs (Gotoh's three-state affine-gap recursion in int32; global, overlap and local
// ends), the alignment itself for a short pair list, and single-linkage clustering by identity in the launch that scores the pairs.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h, with a message channel of their own.
//
// The definition (pesto_amd/sequences.py states it in full): per cell (i, j) three states - D aligns a[i-1] to b[j-1], U sets a[i-1]
// against a gap, L sets b[j-1] against a gap - each the maximum over its three predecessors, THE FIRST IN THE ORDER D, U, L ON TIES, so
// there is exactly one canonical path. The five outputs (score, n_ident, n_aligned, n_cols, span) are functions of that path.
//
// k_align<MODE, false>: ONE WAVE computes one pair, no cell matrix and no traceback: every state carries the counts of its own canonical
// path (n_ident, n_aligned, i0, j0 at 13 bits each in two dwords) through the same predecessor choice that picks its value. Lane l owns
// the strip of W = 8 columns jb + 8 l + 1 .. jb + 8 l + 8 of b and sweeps the rows of a skewed by one lane: at step t it is on row t - l.
// What a strip hands to the next is M[i][last] (the best of D, U, L, the diagonal predecessor of row i + 1) and L[i][last + 1] (a
// function of column `last` alone), value and carry: six dwords by __shfl_up, never through memory. A strip keeps, per column, M of
// the row above and U of the row below (likewise a function of the row above alone): 7 registers per column with the code of b.
// Sequences longer than one pass of 64 strips (512 columns) run in column blocks; the block's last column goes through the call's
// allocation, 24 bytes per row and wave (lane 63 stores row i, lane 0 of the next block loads it one step ahead of its use).
// The substitution matrix (row stride 32) and the wave's two sequences sit in LDS. The recursion itself (align_wave) lives in
// pesto_alignwave.h, templated on the score source, and is shared with pesto_structalign.hip; here the source is the matrix lookup.
// k_align<MODE, true> is the same recursion storing every cell's three predecessor choices as one byte; lane 0 then walks the canonical
// path back and writes `map` and the counts IT meets, so the equality of the two kernels' outputs is a test of the carries.
//
// Clustering: with thresholds, lane 0 of the pair's wave links the two sequences in a union-find in global memory as soon as the pair
// passes the integer test. The larger root always goes under the smaller, so a component's root is its smallest member whatever the order
// of the links: labels do not depend on the schedule. k_align_labels numbers the roots in their order.
#include <climits>
#include <cmath>
#include <numeric>

#include "pesto_alignwave.h"
#include "pesto_call.h"

namespace pesto {

namespace {

using namespace wave;

constexpr int NT = 256;                         // threads per workgroup
constexpr int NW = NT / 64;                     // its waves: a pair each
constexpr int MAXLEN = PESTO_ALIGN_MAX_LENGTH;
constexpr int STRIDE = PESTO_ALIGN_MAX_ALPHABET;    // row stride of the matrix in LDS
constexpr int MAX_SLOTS = 4096;                 // waves of one launch
constexpr size_t BOUND_CAP = (size_t)256 << 20; // bytes of the column-block boundary rows of one launch (at least 256 waves' worth)
enum { OVER_SHORTER = 0, OVER_ALIGNED = 1, OVER_COLUMNS = 2 };

struct AlignArgs {
    int S, mode, go, ge, unknown, A;
    long long k0, k1;                           // the items of this launch
    const int* offs;                            // [S + 1]
    const uint8_t* codes;
    const int8_t* matrix;                       // [A, A]
    const int* pairs;                           // [P, 2], or NULL: all i < j
    const int* order;                           // explicit list: item -> pair (NULL: item = pair); all pairs: the sequences by descending length
    int *score, *ident, *aligned, *cols, *span; // all NULL when only labels are wanted
    int* par;                                   // the union-find (NULL: no clustering)
    int id_bp, cov_bp, over;
    int* bound;                                 // boundary rows, bound_rows per wave (NULL: no pair needs a second block)
    int bound_rows;
    uint8_t* tb;                                // predecessor bytes of the launch's pairs
    const long long* tb_off;                    // [P]: a pair's first byte (within its chunk)
    int* map;
    const long long* map_off;                   // [P]
    const int* err;
};

// ------------------------------------------------------------------------------------------------ union-find
// Every value an entry ever holds is a member of its set with an index below the entry's own or the entry itself (links put a root under
// a smaller root; halving stores a grandparent read earlier, which can be stale but is still such a member, and it never goes into a
// root). So walks end, and the sets are exactly the unions made.
__device__ __forceinline__ int set_find(int* par, int x) {
    for (;;) {
        const int p = ldg(par + x);
        if (p == x) return x;
        const int g = ldg(par + p);
        if (g != p) stg(par + x, g);
        x = g;
    }
}

__device__ __forceinline__ void set_link(int* par, int a, int b) {
    for (;;) {
        a = set_find(par, a);
        b = set_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;                       // the larger root a under b; fails only if a stopped being a root meanwhile
        if (__hip_atomic_compare_exchange_strong(par + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// ------------------------------------------------------------------------------------------------ the recursion
// align_wave of pesto_alignwave.h with this score source: the substitution matrix (row stride 32) and the wave's two sequences in LDS;
// a lane keeps the codes of its strip's columns in registers and looks a row of the matrix up once per row.
struct MatrixScore {
    typedef int Col;
    struct Row { int ac; const int8_t* row; };
    const uint8_t *sa, *sb;
    const int8_t* smat;
    int unknown;
    __device__ __forceinline__ Col column(int j, int n) const { return j <= n ? sb[j - 1] : 0; }
    __device__ __forceinline__ Row row(int i) const {
        const int ac = sa[i - 1];
        return Row{ac, smat + ac * STRIDE};
    }
    __device__ __forceinline__ int score(const Row& r, Col bc) const { return r.row[bc]; }
    __device__ __forceinline__ bool ident(const Row& r, Col bc) const { return r.ac == bc && r.ac != unknown; }
};

// pair `p` of all i < j in row-major order, S sequences
__device__ __forceinline__ long long pair_position(long long i, long long j, long long S) { return i * (2 * S - i - 1) / 2 + (j - i - 1); }

// Persistent waves: wave w of the launch takes the items k0 + w, + waves, ... An item is a pair of the explicit list (through `order`,
// long pairs first) or, for all against all, the k-th pair (x < y) of the sequences sorted by descending length, k = y (y - 1) / 2 + x,
// so a list of S^2 pairs is never made.
// (three waves per SIMD: 168 registers. Without the bound the compiler takes 175 to 197 and two waves fit; measured 8 % slower.)
template <int MODE, bool TRACE>
__global__ __launch_bounds__(NT, 3) void k_align(const AlignArgs A) {
    __shared__ int8_t s_mat[STRIDE * STRIDE];
    __shared__ uint8_t s_seq[NW][2][MAXLEN];
    if (*A.err) return;
    for (int k = threadIdx.x; k < STRIDE * STRIDE; k += NT) {
        const int r = k / STRIDE, c = k % STRIDE;
        s_mat[k] = r < A.A && c < A.A ? A.matrix[r * A.A + c] : (int8_t)0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slot = (long long)blockIdx.x * NW + wave, waves = (long long)gridDim.x * NW;
    uint8_t* sa = s_seq[wave][0];
    uint8_t* sb = s_seq[wave][1];
    int* bound = A.bound ? A.bound + (size_t)slot * A.bound_rows * ROW_INTS : nullptr;
    for (long long k = A.k0 + slot; k < A.k1; k += waves) {
        int ia, ib;
        long long p;
        if (A.pairs) {
            p = A.order ? A.order[k] : k;
            ia = A.pairs[2 * p];
            ib = A.pairs[2 * p + 1];
        } else {
            long long y = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
            while (y * (y - 1) / 2 > k) --y;
            while ((y + 1) * y / 2 <= k) ++y;
            const long long x = k - y * (y - 1) / 2;
            ia = A.order[x];
            ib = A.order[y];
            if (ia > ib) { const int t = ia; ia = ib; ib = t; }
            p = pair_position(ia, ib, A.S);
        }
        const int oa = A.offs[ia], ob = A.offs[ib], m = A.offs[ia + 1] - oa, n = A.offs[ib + 1] - ob;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the last pair's reads are behind us)
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < m; q += 64) sa[q] = A.codes[oa + q];
        for (int q = lane; q < n; q += 64) sb[q] = A.codes[ob + q];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint8_t* tb = TRACE ? A.tb + A.tb_off[p] : nullptr;
        const MatrixScore src{sa, sb, s_mat, A.unknown};
        const End e = align_wave<MODE, TRACE>(src, m, n, A.go, A.ge, bound, tb);
        // the end rule's border cells: an overlap end (0, n) of value 0 precedes every cell of a row i >= 1 that does not beat it
        const bool empty = (MODE == MODE_OVERLAP || MODE == MODE_LOCAL) && e.v <= 0;
        int score = empty ? 0 : e.v, i1 = empty ? 0 : e.i, j1 = empty ? (MODE == MODE_OVERLAP ? n : 0) : e.j;
        int n_ident = empty ? 0 : (int)(e.lo & 0x1fffu), n_aligned = empty ? 0 : (int)(e.lo >> 13 & 0x1fffu);
        int i0 = empty ? i1 : (int)(e.hi & 0x1fffu), j0 = empty ? j1 : (int)(e.hi >> 13 & 0x1fffu);
        if (TRACE) {
            int* map = A.map + A.map_off[p];
            __threadfence();
            // (not walk_back of pesto_alignwave.h: this walk starts in the END STATE of a global alignment, fills the rows a global path
            // leaves above its first cell, and counts the identities it meets from the two sequences, so that its five outputs test the
            // carries of k_align<MODE, false>; walk_back is the overlap / local walk of a source without an identity)
            if (lane == 0 && !empty) {                              // the canonical path, back from the end
                int i = i1, j = j1, ni = 0, na = 0;
                unsigned st = e.hi >> 26;
                for (;;) {
                    if (i == 0 || j == 0) {
                        if (MODE == MODE_GLOBAL) {
                            for (; i > 0; --i) map[i - 1] = -1;
                            j = 0;
                        }
                        break;
                    }
                    const size_t at = (size_t)(i - 1) * n + (j - 1);
                    const unsigned word = (unsigned)ldg((const int*)(tb + (at & ~(size_t)3)));
                    const unsigned pred = (word >> (8 * (at & 3)) >> (2 * st)) & 3u;
                    if (st == 0) {
                        map[i - 1] = j - 1;
                        ++na;
                        ni += sa[i - 1] == sb[j - 1] && sa[i - 1] != A.unknown ? 1 : 0;
                        --i;
                        --j;
                        if (pred == 3) break;
                    } else if (st == 1) {
                        map[i - 1] = -1;
                        --i;
                    } else {
                        --j;
                    }
                    st = pred;
                }
                i0 = i; j0 = j; n_ident = ni; n_aligned = na;
            }
            i0 = __shfl(i0, 0); j0 = __shfl(j0, 0); n_ident = __shfl(n_ident, 0); n_aligned = __shfl(n_aligned, 0);
            for (int r = lane; r < m; r += 64)
                if (r < i0 || r >= i1) map[r] = -1;
        }
        if (lane == 0) {
            const int n_cols = (i1 - i0) + (j1 - j0) - n_aligned;
            if (A.score) {
                A.score[p] = score;
                A.ident[p] = n_ident;
                A.aligned[p] = n_aligned;
                A.cols[p] = n_cols;
                A.span[4 * p] = i0; A.span[4 * p + 1] = j0; A.span[4 * p + 2] = i1; A.span[4 * p + 3] = j1;
            }
            if (!TRACE && A.par) {
                const long long denom = A.over == OVER_SHORTER ? min(m, n) : A.over == OVER_ALIGNED ? n_aligned : n_cols;
                if (denom > 0 && (long long)n_ident * 10000 >= (long long)A.id_bp * denom && (long long)n_aligned * 10000 >= (long long)A.cov_bp * max(m, n))
                    set_link(A.par, ia, ib);
            }
        }
    }
}

// every code must lie in [0, A): bit 0 of *err
__global__ __launch_bounds__(NT) void k_align_check(long long total, int A, const uint8_t* __restrict__ codes, int* __restrict__ err) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    if (k < total && codes[k] >= A) atomicOr(err, 1);
}

// One workgroup: every entry's root, the roots numbered in their order, every sequence its root's number.
__global__ __launch_bounds__(NT) void k_align_labels(int S, int* __restrict__ par, int* __restrict__ labels, const int* __restrict__ err) {
    __shared__ int s_wave[NW];
    __shared__ int s_base;
    if (*err) return;
    for (int x = threadIdx.x; x < S; x += NT) {
        int r = x;
        for (int p = ldg(par + r); p != r; p = ldg(par + r)) r = p;
        labels[x] = r;
    }
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < S; c0 += NT) {
        const int x = c0 + (int)threadIdx.x;
        const bool root = x < S && labels[x] == x;
        const unsigned long long mask = __ballot(root);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (root) par[x] = before + __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();
        if (threadIdx.x == 0) s_base += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        __syncthreads();
    }
    for (int x = threadIdx.x; x < S; x += NT) labels[x] = par[labels[x]];
}

template <bool TRACE>
void launch_align(int mode, unsigned groups, hipStream_t stm, const AlignArgs& a) {
    if (mode == MODE_GLOBAL) hipLaunchKernelGGL((k_align<MODE_GLOBAL, TRACE>), dim3(groups), dim3(NT), 0, stm, a);
    else if (mode == MODE_OVERLAP) hipLaunchKernelGGL((k_align<MODE_OVERLAP, TRACE>), dim3(groups), dim3(NT), 0, stm, a);
    else hipLaunchKernelGGL((k_align<MODE_LOCAL, TRACE>), dim3(groups), dim3(NT), 0, stm, a);
}

// the arguments both entry points share; *total_out: the number of codes
int check_common(int32_t S, const int32_t* offs, const uint8_t* codes, int32_t A, const int8_t* matrix, int32_t mode, int32_t go, int32_t ge,
                 int32_t unknown, int64_t P, const int32_t* pairs, int64_t* total_out) {
    if (!offs || !codes || !matrix) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (S < 1 || S > PESTO_ALIGN_MAX_SEQUENCES) return fail(PESTO_ERR_INVALID, "1 to %d sequences, got %d", PESTO_ALIGN_MAX_SEQUENCES, S);
    if (A < 1 || A > PESTO_ALIGN_MAX_ALPHABET) return fail(PESTO_ERR_INVALID, "an alphabet of 1 to %d codes, got %d", PESTO_ALIGN_MAX_ALPHABET, A);
    if (mode < MODE_GLOBAL || mode > MODE_LOCAL) return fail(PESTO_ERR_INVALID, "mode must be 0 (global), 1 (overlap) or 2 (local)");
    if (ge < 0 || go < ge || go > PESTO_ALIGN_MAX_GAP) return fail(PESTO_ERR_INVALID, "%d >= gap_open >= gap_extend >= 0 expected, got %d, %d", PESTO_ALIGN_MAX_GAP, go, ge);
    if (unknown < -1 || unknown >= A) return fail(PESTO_ERR_INVALID, "unknown must be a code of the alphabet or -1, got %d", unknown);
    if (offs[0] != 0) return fail(PESTO_ERR_INVALID, "seq_offsets must start at 0");
    for (int s = 0; s < S; ++s) {
        const int64_t len = (int64_t)offs[s + 1] - offs[s];
        if (len < 1 || len > MAXLEN) return fail(PESTO_ERR_INVALID, "sequence %d: 1 to %d codes, got %lld", s, MAXLEN, (long long)len);
    }
    if (P < 0 || P > PESTO_ALIGN_MAX_PAIRS) return fail(PESTO_ERR_INVALID, "at most 2^31 - 1 pairs, got %lld", (long long)P);
    if (pairs)
        for (int64_t p = 0; p < 2 * P; ++p)
            if (pairs[p] < 0 || pairs[p] >= S) return fail(PESTO_ERR_INVALID, "pair %lld names sequence %d of %d", (long long)(p / 2), pairs[p], S);
    *total_out = offs[S];
    return 0;
}

// the waves of a launch over n_items whose boundary rows (rows each, 0: none) fit BOUND_CAP: a multiple of NW
int plan_slots(int64_t n_items, int rows) {
    int64_t slots = std::min<int64_t>(std::max<int64_t>(n_items, 1), MAX_SLOTS);
    if (rows > 0) slots = std::min<int64_t>(slots, std::max<int64_t>(256, (int64_t)(BOUND_CAP / ((size_t)rows * ROW_INTS * 4))));
    return (int)((slots + NW - 1) / NW * NW);
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_align_last_error(void) { return last_error(); }

int pesto_align_scores(pesto_model* m, int32_t S, const int32_t* seq_offsets, const uint8_t* codes, int32_t A, const int8_t* matrix, int32_t mode,
                       int32_t gap_open, int32_t gap_extend, int32_t unknown, int64_t P, const int32_t* pairs, int32_t* score_out,
                       int32_t* n_ident_out, int32_t* n_aligned_out, int32_t* n_cols_out, int32_t* span_out, int32_t id_bp, int32_t cov_bp,
                       int32_t over, int32_t* labels_out, int32_t ptr_kind, void* stream) {
    int64_t total = 0;
    if (int rc = check_common(S, seq_offsets, codes, A, matrix, mode, gap_open, gap_extend, unknown, P, pairs, &total)) return rc;
    const int n_out = !!score_out + !!n_ident_out + !!n_aligned_out + !!n_cols_out + !!span_out;
    if ((n_out != 0 && n_out != 5) || (n_out == 0 && !labels_out)) return fail(PESTO_ERR_INVALID, "the five per-pair outputs together, or labels_out alone");
    if (labels_out && (id_bp < 0 || id_bp > 10000 || cov_bp < 0 || cov_bp > 10000 || over < OVER_SHORTER || over > OVER_COLUMNS))
        return fail(PESTO_ERR_INVALID, "thresholds in basis points (0 to 10000) and over 0, 1 or 2 expected");
    if (!pairs) {
        if (P != (int64_t)S * (S - 1) / 2) return fail(PESTO_ERR_INVALID, "without a list, P must be S (S - 1) / 2");
    }
    // the order of the work: long pairs first (a launch ends on its longest pair)
    std::vector<int32_t> order;
    int rows = 0;
    auto len = [&](int s) { return seq_offsets[s + 1] - seq_offsets[s]; };
    if (pairs) {
        order.resize((size_t)P);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
            return (int64_t)len(pairs[2 * (int64_t)x]) * len(pairs[2 * (int64_t)x + 1]) > (int64_t)len(pairs[2 * (int64_t)y]) * len(pairs[2 * (int64_t)y + 1]);
        });
        for (int64_t p = 0; p < P; ++p)
            if (len(pairs[2 * p + 1]) > BLOCK_COLS) rows = std::max(rows, len(pairs[2 * p]) + 1);
    } else {
        order.resize((size_t)S);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return len(x) > len(y); });
        if (len(order[0]) > BLOCK_COLS) rows = len(order[0]) + 1;
    }
    if (int rc = begin(m, ptr_kind)) return rc;
    const int slots = plan_slots(P, rows);
    std::vector<int32_t> iota;
    if (labels_out) {
        iota.resize((size_t)S);
        std::iota(iota.begin(), iota.end(), 0);
    }
    Buffers bf(ptr_kind, stream);
    const int iC = bf.input(codes, (size_t)total), iO = bf.table(seq_offsets, ((size_t)S + 1) * 4), iM = bf.table(matrix, (size_t)A * A);
    const int iP = pairs ? bf.table(pairs, (size_t)P * 8) : -1, iOr = bf.table(order.data(), order.size() * 4);
    const int iSc = bf.output(score_out, (size_t)P * 4), iId = bf.output(n_ident_out, (size_t)P * 4), iAl = bf.output(n_aligned_out, (size_t)P * 4),
              iCo = bf.output(n_cols_out, (size_t)P * 4), iSp = bf.output(span_out, (size_t)P * 16), iLb = bf.output(labels_out, (size_t)S * 4);
    const int iPar = labels_out ? bf.table(iota.data(), (size_t)S * 4) : -1;
    const int iB = rows ? bf.scratch((size_t)slots * rows * ROW_INTS * 4) : -1, iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        AlignArgs a{};
        a.S = S; a.mode = mode; a.go = gap_open; a.ge = gap_extend; a.unknown = unknown; a.A = A;
        a.k0 = 0; a.k1 = P;
        a.offs = bf.ptr<const int>(iO); a.codes = bf.ptr<const uint8_t>(iC); a.matrix = bf.ptr<const int8_t>(iM);
        a.pairs = pairs ? bf.ptr<const int>(iP) : nullptr; a.order = bf.ptr<const int>(iOr);
        a.score = bf.ptr<int>(iSc); a.ident = bf.ptr<int>(iId); a.aligned = bf.ptr<int>(iAl); a.cols = bf.ptr<int>(iCo); a.span = bf.ptr<int>(iSp);
        a.par = labels_out ? bf.ptr<int>(iPar) : nullptr; a.id_bp = id_bp; a.cov_bp = cov_bp; a.over = over;
        a.bound = rows ? bf.ptr<int>(iB) : nullptr; a.bound_rows = rows;
        a.err = bf.ptr<const int>(iSt);
        hipLaunchKernelGGL(k_align_check, dim3(blocks((size_t)total, NT)), dim3(NT), 0, bf.stm, (long long)total, (int)A, a.codes, bf.ptr<int>(iSt));
        if (P > 0) launch_align<false>(mode, (unsigned)(slots / NW), bf.stm, a);
        if (labels_out) hipLaunchKernelGGL(k_align_labels, dim3(1), dim3(NT), 0, bf.stm, (int)S, a.par, bf.ptr<int>(iLb), a.err);
    }
    // a refused call writes nothing: every kernel behind the check returns on its verdict, which is read before any output is copied back
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "align_scores");
    if (rc == 0 && (herr & 1)) rc = fail(PESTO_ERR_INVALID, "align_scores: every code must lie in [0, %d)", A);
    return bf.finish(rc, "align_scores");
}

int pesto_align_maps(pesto_model* m, int32_t S, const int32_t* seq_offsets, const uint8_t* codes, int32_t A, const int8_t* matrix, int32_t mode,
                     int32_t gap_open, int32_t gap_extend, int32_t unknown, int64_t P, const int32_t* pairs, int32_t* score_out, int32_t* n_ident_out,
                     int32_t* n_aligned_out, int32_t* n_cols_out, int32_t* span_out, int32_t* map_out, int32_t ptr_kind, void* stream) {
    int64_t total = 0;
    if (int rc = check_common(S, seq_offsets, codes, A, matrix, mode, gap_open, gap_extend, unknown, P, pairs, &total)) return rc;
    if (!pairs || !score_out || !n_ident_out || !n_aligned_out || !n_cols_out || !span_out || !map_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (P < 1 || P > PESTO_ALIGN_MAX_MAP_PAIRS) return fail(PESTO_ERR_INVALID, "1 to %d pairs, got %lld", PESTO_ALIGN_MAX_MAP_PAIRS, (long long)P);
    auto len = [&](int s) { return seq_offsets[s + 1] - seq_offsets[s]; };
    // the chunks of the list whose predecessor bytes fit the workspace (a pair alone always does: 16 MiB at most)
    std::vector<long long> tb_off((size_t)P), map_off((size_t)P);
    std::vector<int64_t> chunk_at{0};
    size_t used = 0, workspace = 0;
    long long n_map = 0;
    int rows = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int la = len(pairs[2 * p]), lb = len(pairs[2 * p + 1]);
        const size_t bytes = ((size_t)la * lb + 4 + 255) & ~(size_t)255;
        if (used && used + bytes > (size_t)PESTO_ALIGN_MAPS_WORKSPACE) {
            chunk_at.push_back(p);
            used = 0;
        }
        tb_off[(size_t)p] = (long long)used;
        used += bytes;
        workspace = std::max(workspace, used);
        map_off[(size_t)p] = n_map;
        n_map += la;
        if (lb > BLOCK_COLS) rows = std::max(rows, la + 1);
    }
    chunk_at.push_back(P);
    if (int rc = begin(m, ptr_kind)) return rc;
    int64_t widest = 0;
    for (size_t c = 0; c + 1 < chunk_at.size(); ++c) widest = std::max(widest, chunk_at[c + 1] - chunk_at[c]);
    const int slots = plan_slots(widest, rows);
    Buffers bf(ptr_kind, stream);
    const int iC = bf.input(codes, (size_t)total), iO = bf.table(seq_offsets, ((size_t)S + 1) * 4), iM = bf.table(matrix, (size_t)A * A);
    const int iP = bf.table(pairs, (size_t)P * 8), iTo = bf.table(tb_off.data(), (size_t)P * 8), iMo = bf.table(map_off.data(), (size_t)P * 8);
    const int iSc = bf.output(score_out, (size_t)P * 4), iId = bf.output(n_ident_out, (size_t)P * 4), iAl = bf.output(n_aligned_out, (size_t)P * 4),
              iCo = bf.output(n_cols_out, (size_t)P * 4), iSp = bf.output(span_out, (size_t)P * 16), iMp = bf.output(map_out, (size_t)n_map * 4);
    const int iTb = bf.scratch(workspace), iB = rows ? bf.scratch((size_t)slots * rows * ROW_INTS * 4) : -1, iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        AlignArgs a{};
        a.S = S; a.mode = mode; a.go = gap_open; a.ge = gap_extend; a.unknown = unknown; a.A = A;
        a.offs = bf.ptr<const int>(iO); a.codes = bf.ptr<const uint8_t>(iC); a.matrix = bf.ptr<const int8_t>(iM);
        a.pairs = bf.ptr<const int>(iP);
        a.score = bf.ptr<int>(iSc); a.ident = bf.ptr<int>(iId); a.aligned = bf.ptr<int>(iAl); a.cols = bf.ptr<int>(iCo); a.span = bf.ptr<int>(iSp);
        a.bound = rows ? bf.ptr<int>(iB) : nullptr; a.bound_rows = rows;
        a.tb = bf.ptr<uint8_t>(iTb); a.tb_off = bf.ptr<const long long>(iTo); a.map = bf.ptr<int>(iMp); a.map_off = bf.ptr<const long long>(iMo);
        a.err = bf.ptr<const int>(iSt);
        hipLaunchKernelGGL(k_align_check, dim3(blocks((size_t)total, NT)), dim3(NT), 0, bf.stm, (long long)total, (int)A, a.codes, bf.ptr<int>(iSt));
        for (size_t c = 0; c + 1 < chunk_at.size(); ++c) {          // (launches of one stream: a chunk's bytes are free when the next begins)
            a.k0 = chunk_at[c];
            a.k1 = chunk_at[c + 1];
            const int64_t waves = std::min<int64_t>(slots, (a.k1 - a.k0 + NW - 1) / NW * NW);
            launch_align<true>(mode, (unsigned)(waves / NW), bf.stm, a);
        }
    }
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "align_maps");
    if (rc == 0 && (herr & 1)) rc = fail(PESTO_ERR_INVALID, "align_maps: every code must lie in [0, %d)", A);
    return bf.finish(rc, "align_maps");
}
