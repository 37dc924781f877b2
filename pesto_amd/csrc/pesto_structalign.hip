// pesto_structalign.hip - structure-based alignment of CA traces: for two chains whose residue correspondence is NOT known, the alignment
// and the superposition that go together, found by alternating the two halves the library already has - Gotoh's recursion as a wavefront
// (pesto_alignwave.h) with a cell score made of the distance of two residues under a superposition, and the TM-score superposition
// search (pesto_tmscore.hip through pesto_tmsearch.h) on the residue pairs that alignment gives.
//
// The C entry point (include/pesto_hip.h, which states the definition in full; so does pesto_amd/structalign.py) lives here too, on the
// call plumbing of pesto_call.h, with a message channel of its own.
//
// k_sa_dp<TRACE>: ONE WAVE per item (a pair under one transform and one gap), persistent over an item list, one wave per workgroup so that
// the wave's two chains sit in its own dynamic LDS as float32 (12 (m + n) bytes, at most 96 KB). A lane transforms x_i once per row in
// double and keeps the eight y_j of its strip in registers (24 VGPRs): the cell is then 3 subtractions, 3 multiply-adds, one double
// division and a floor in front of the about 50 integer instructions of the three states. Without TRACE it keeps O(m + n) memory (the column-block
// boundary rows) and serves the fragment seeds; with TRACE it stores one predecessor byte per cell and lane 0 walks the path back.
// k_sa_thread / k_sa_frag: a wave per gapless offset / per fragment pair: one Kabsch fit (kabsch_fit_wave) of a window of a onto a window
// of b, as x' = x R + t; the threading also sums the integer scores over the window. k_sa_pick takes a pair's best offset and best
// fragment pair (ties to the lowest), k_sa_start lays the initial maps out per unit, k_sa_gather compacts a map's aligned pairs into two
// coordinate arrays, k_sa_round keeps the best (tm, unit, round) of a pair, compares the new maps with the old and sets the done flags,
// k_sa_final writes a pair's outputs. No atomics; a wave owns what it writes, so nothing depends on how items are shared over workgroups.
#include <cmath>

#include "pesto_alignwave.h"
#include "pesto_call.h"
#include "pesto_fit.h"
#include "pesto_tmsearch.h"

namespace pesto {

namespace {

using namespace wave;

constexpr int NT = 256;                         // threads of the workgroup kernels (k_sa_rmsd: those of k_fit_rmsd)
constexpr double Q = (double)PESTO_STRUCTALIGN_Q;
constexpr int MAX_SLOTS = 4096;                 // workgroups (waves) of one k_sa_dp launch
constexpr size_t BOUND_CAP = (size_t)256 << 20; // bytes of the column-block boundary rows of one launch
constexpr int64_t CHUNK_ITEMS = 1 << 20;        // threading offsets and fragment pairs set up at a time

// one piece of work of a wave: a pair, its gap, where its results go, a window (a from fa, b from fb, len residues) for the fits, which
// transform of the launch's list it runs under, the first predecessor byte (or the first gathered point) and the first entry of its map
struct SaItem {
    int pair, go, dst, fa, fb, len, tf, pad;
    long long tb_off, map_off;
};

// a pair of the chunk for k_sa_pick: its threading sums and fragment-pair scores in the chunk's arrays, and the offset of sum 0
struct SaPick { int thr_lo, thr_n, frag_lo, frag_n, kmin, pad; };

struct SaArgs {
    const float* xyz;
    const int *offs, *pairs;
    const double* ks;                           // [P]: scale^2 / d0s^2
    const SaItem* items;
    long long k0, k1;
    const double *rot, *tr;                     // [transforms, 9], [transforms, 3]
    int *score, *nal;                           // [dst]
    int* maps;
    uint8_t* tb;
    int* bound;
    int bound_rows;
};

// x' = x R + t of a float32 point in double, and the integer score of x' against y: floor(Q / (1 + |x' - y|^2 k) + 0.5)
__device__ __forceinline__ void transformed(const float* x, const double* R, const double* t, double* p) {
    const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
    for (int c = 0; c < 3; ++c) p[c] = ((x0 * R[c] + x1 * R[3 + c]) + x2 * R[6 + c]) + t[c];
}

__device__ __forceinline__ int cell_score(double p0, double p1, double p2, float y0, float y1, float y2, double k) {
    const double e0 = p0 - (double)y0, e1 = p1 - (double)y1, e2 = p2 - (double)y2;
    const double u = ((e0 * e0 + e1 * e1) + e2 * e2) * k;
    return (int)floor(Q / (1.0 + u) + 0.5);
}

// the geometric score source of align_wave: both chains in LDS, the transform and the pair's constant the same in every lane
struct GeoScore {
    struct Col { float y0, y1, y2; };
    struct Row { double p0, p1, p2; };
    const float *sx, *sy;
    double R[9], t[3], k;
    __device__ __forceinline__ Col column(int j, int n) const {
        if (j > n) return Col{0.f, 0.f, 0.f};
        return Col{sy[3 * (j - 1)], sy[3 * (j - 1) + 1], sy[3 * (j - 1) + 2]};
    }
    __device__ __forceinline__ Row row(int i) const {
        double p[3];
        transformed(sx + 3 * (i - 1), R, t, p);
        return Row{p[0], p[1], p[2]};
    }
    __device__ __forceinline__ int score(const Row& r, const Col& c) const { return cell_score(r.p0, r.p1, r.p2, c.y0, c.y1, c.y2, k); }
    __device__ __forceinline__ bool ident(const Row&, const Col&) const { return false; }       // (identities are counted from the map)
};

// ------------------------------------------------------------------------------------------------ the dynamic programme
// (two waves per SIMD: the strip's 24 coordinate registers and the row's doubles on top of k_align's 168 do not fit three; the kernel is
// bound by its dependent double division per cell, not by latency that a third wave would hide)
template <bool TRACE>
__global__ __launch_bounds__(64, 2) void k_sa_dp(const SaArgs A) {
    extern __shared__ float s_xy[];
    const int lane = threadIdx.x;
    int* bound = A.bound ? A.bound + (size_t)blockIdx.x * A.bound_rows * ROW_INTS : nullptr;
    for (long long k = A.k0 + blockIdx.x; k < A.k1; k += gridDim.x) {
        const SaItem it = A.items[k];
        const int ia = A.pairs[2 * it.pair], ib = A.pairs[2 * it.pair + 1];
        const int oa = A.offs[ia], ob = A.offs[ib], m = A.offs[ia + 1] - oa, n = A.offs[ib + 1] - ob;
        float* sx = s_xy;
        float* sy = s_xy + 3 * (size_t)m;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the last item's reads are behind us)
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < 3 * m; q += 64) sx[q] = A.xyz[3 * (size_t)oa + q];
        for (int q = lane; q < 3 * n; q += 64) sy[q] = A.xyz[3 * (size_t)ob + q];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        GeoScore src;
        src.sx = sx;
        src.sy = sy;
        for (int c = 0; c < 9; ++c) src.R[c] = A.rot[9 * (size_t)it.tf + c];
        for (int c = 0; c < 3; ++c) src.t[c] = A.tr[3 * (size_t)it.tf + c];
        src.k = A.ks[it.pair];
        uint8_t* tb = TRACE ? A.tb + it.tb_off : nullptr;
        const End e = align_wave<MODE_OVERLAP, TRACE>(src, m, n, it.go, 0, bound, tb);
        // the end rule's border cells: the end (0, n) of value 0 precedes every cell of a row i >= 1 that does not beat it
        const bool empty = e.v <= 0;
        if (TRACE) {
            int* map = A.maps + it.map_off;
            const int i1 = empty ? 0 : e.i, j1 = empty ? n : e.j;
            int i0 = i1, j0 = j1, na = 0;
            __threadfence();
            if (lane == 0 && !empty) na = walk_back(tb, n, i1, j1, map, i0, j0);
            i0 = __shfl(i0, 0);
            na = __shfl(na, 0);
            for (int r = lane; r < m; r += 64)
                if (r < i0 || r >= i1) map[r] = -1;
            if (lane == 0) A.nal[it.dst] = na;
        }
        if (lane == 0) A.score[it.dst] = empty ? 0 : e.v;
    }
}

// ------------------------------------------------------------------------------------------------ the initial alignments
// the fit of the window (a from fa, b from fb, len residues) as x' = x R + t, the same in every lane
__device__ __forceinline__ void window_fit(const float* X, const float* Y, int len, double* R, double* t) {
    const int lane = threadIdx.x & 63;
    unsigned long long in = 0ull;
    for (int j = 0, k = lane; k < len; ++j, k += 64) in |= 1ull << j;
    Fit ft;
    kabsch_fit_wave<true>(atoms<true>(X, nullptr), atoms<true>(Y, nullptr), len, in, ft);
    for (int c = 0; c < 9; ++c) R[c] = ft.R[c];
    for (int c = 0; c < 3; ++c) t[c] = ft.same ? 0.0 : ft.m[3 + c] - ((ft.m[0] * ft.R[c] + ft.m[1] * ft.R[3 + c]) + ft.m[2] * ft.R[6 + c]);
}

// I1: a wave per gapless offset: the fit of the overlap and the sum of its integer scores under that fit
__global__ __launch_bounds__(64) void k_sa_thread(const SaArgs A) {
    const long long k = A.k0 + blockIdx.x;
    const SaItem it = A.items[k];
    const float* X = A.xyz + 3 * ((size_t)A.offs[A.pairs[2 * it.pair]] + it.fa);
    const float* Y = A.xyz + 3 * ((size_t)A.offs[A.pairs[2 * it.pair + 1]] + it.fb);
    double R[9], t[3];
    window_fit(X, Y, it.len, R, t);
    const double ks = A.ks[it.pair];
    int sum = 0;
    for (int q = threadIdx.x; q < it.len; q += 64) {
        double p[3];
        transformed(X + 3 * q, R, t, p);
        sum += cell_score(p[0], p[1], p[2], Y[3 * q], Y[3 * q + 1], Y[3 * q + 2], ks);
    }
    sum = wave_sum(sum);
    if (threadIdx.x == 0) A.score[it.dst] = sum;
}

// I2: a wave per fragment pair: the fit of the one fragment onto the other, for the scores-only k_sa_dp of the whole chains under it
__global__ __launch_bounds__(64) void k_sa_frag(const SaArgs A, double* __restrict__ rot, double* __restrict__ tr) {
    const long long k = A.k0 + blockIdx.x;
    const SaItem it = A.items[k];
    const float* X = A.xyz + 3 * ((size_t)A.offs[A.pairs[2 * it.pair]] + it.fa);
    const float* Y = A.xyz + 3 * ((size_t)A.offs[A.pairs[2 * it.pair + 1]] + it.fb);
    double R[9], t[3];
    window_fit(X, Y, it.len, R, t);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 9; ++c) rot[9 * k + c] = R[c];
        for (int c = 0; c < 3; ++c) tr[3 * k + c] = t[c];
    }
}

// the first largest of v[0 .. n) over the wave: its index in every lane
__device__ __forceinline__ int first_max(const int* __restrict__ v, int n) {
    int bv = INT_MIN, bq = INT_MAX;
    for (int q = threadIdx.x; q < n; q += 64)
        if (v[q] > bv) { bv = v[q]; bq = q; }
    for (int o = 32; o > 0; o >>= 1) {
        const int v2 = __shfl_xor(bv, o), q2 = __shfl_xor(bq, o);
        if (v2 > bv || (v2 == bv && q2 < bq)) { bv = v2; bq = q2; }
    }
    return bq;
}

// a wave per pair of the chunk: the best offset's overlap becomes the map of units 0 and 1 (the unit of initial alignment i and gap g is
// 2 i + g; a unit's map lies at n_units * map_off[pair] + unit * m), the best fragment pair's fit the transform of the pair's traced DP
__global__ __launch_bounds__(64) void k_sa_pick(int p0, int n_units, const SaPick* __restrict__ picks, const int* __restrict__ offs,
                                                const int* __restrict__ pairs, const long long* __restrict__ map_off, const int* __restrict__ sums,
                                                const int* __restrict__ fscore, const double* __restrict__ rot, const double* __restrict__ tr,
                                                int* __restrict__ maps, double* __restrict__ rot0, double* __restrict__ tr0) {
    const int p = p0 + blockIdx.x, lane = threadIdx.x;
    const SaPick pk = picks[blockIdx.x];
    if (pk.thr_n == 0) return;                  // (a chain with a non-finite coordinate: nothing is set up)
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1], m = offs[ia + 1] - offs[ia], n = offs[ib + 1] - offs[ib];
    const int k = pk.kmin + first_max(sums + pk.thr_lo, pk.thr_n);
    int* map = maps + n_units * map_off[p];
    for (int r = lane; r < m; r += 64) {
        const int j = r + k;
        map[r] = map[m + r] = j >= 0 && j < n ? j : -1;
    }
    const int f = pk.frag_lo + first_max(fscore + pk.frag_lo, pk.frag_n);
    if (lane < 9) rot0[9 * (size_t)p + lane] = rot[9 * (size_t)f + lane];
    if (lane < 3) tr0[3 * (size_t)p + lane] = tr[3 * (size_t)f + lane];
}

// a wave per pair: unit 2's map (the traced DP under the best fragment fit) is unit 3's too, the caller's map that of units 4 and 5; every
// unit's number of aligned residues and whether it is dead from the start (state[2 u] = n_aligned, state[2 u + 1] = done)
__global__ __launch_bounds__(64) void k_sa_start(int n_units, const int* __restrict__ offs, const int* __restrict__ pairs, const long long* __restrict__ map_off,
                                                 const int* __restrict__ pair_bad, const int* __restrict__ init, int* __restrict__ maps, int* __restrict__ state) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int ia = pairs[2 * p], m = offs[ia + 1] - offs[ia];
    int* map = maps + n_units * map_off[p];
    for (int u = 0; u < n_units; u += 2) {
        int na = 0;
        if (!pair_bad[p])
            for (int r = lane; r < m; r += 64) {
                const int j = u < 4 ? map[u * m + r] : init[map_off[p] + r];
                if (u == 2) map[3 * m + r] = j;
                if (u == 4) map[4 * m + r] = map[5 * m + r] = j;
                na += j >= 0 ? 1 : 0;
            }
        na = wave_sum(na);
        if (lane < 2) {
            state[2 * ((size_t)p * n_units + u + lane)] = na;
            state[2 * ((size_t)p * n_units + u + lane) + 1] = na < 3 ? 1 : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ a round
// a wave per item: the aligned pairs of the item's map, in the order of a, into X (points of a) and Y (points of b) from it.tb_off on
__global__ __launch_bounds__(64) void k_sa_gather(const SaArgs A, float* __restrict__ X, float* __restrict__ Y) {
    const SaItem it = A.items[A.k0 + blockIdx.x];
    const int lane = threadIdx.x;
    const int oa = A.offs[A.pairs[2 * it.pair]], ob = A.offs[A.pairs[2 * it.pair + 1]], m = A.offs[A.pairs[2 * it.pair] + 1] - oa;
    const int* map = A.maps + it.map_off;
    long long at = it.tb_off;
    for (int r0 = 0; r0 < m; r0 += 64) {
        const int r = r0 + lane, j = r < m ? map[r] : -1;
        const unsigned long long mask = __ballot(j >= 0);
        if (j >= 0) {
            const long long g = at + __popcll(mask & ((1ull << lane) - 1ull));
            for (int c = 0; c < 3; ++c) {
                X[3 * g + c] = A.xyz[3 * ((size_t)oa + r) + c];
                Y[3 * g + c] = A.xyz[3 * ((size_t)ob + j) + c];
            }
        }
        at += __popcll(mask);
    }
}

struct SaRound {
    int n_units, rounds, round;
    const int *offs, *pairs;
    const long long* map_off;
    const int* live_of;                         // [units]: the unit's place in this round's batch, -1: it did not run
    const float* tm;                            // [batch]
    const int *new_score, *new_nal;             // [units]
    int *cur, *next, *best_map;
    int* state;
    double* best_tm;                            // [P], from -1
    int* best;                                  // [P, 4]: unit, round, dp_score, n_aligned; unit from -1
    double* history;
};

// a wave per pair, its units in their order: the round's history entry; the searched alignment becomes the pair's best if its tm_r is
// larger than every one before (or equal, from a lower unit: rounds ascend, so the lowest (unit, round) keeps a tie); the new map
// replaces the old, and the unit is done if the two are equal or fewer than 3 residues are aligned
__global__ __launch_bounds__(64) void k_sa_round(const SaRound A) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int ia = A.pairs[2 * p], m = A.offs[ia + 1] - A.offs[ia];
    double best_tm = A.best_tm[p];
    int best[4] = {A.best[4 * p], A.best[4 * p + 1], A.best[4 * p + 2], A.best[4 * p + 3]};
    for (int u = 0; u < A.n_units; ++u) {
        const size_t unit = (size_t)p * A.n_units + u;
        const int l = A.live_of[unit];
        if (l < 0) continue;
        const double tm = (double)A.tm[l];
        const int score = A.new_score[unit], nal = A.state[2 * unit], new_nal = A.new_nal[unit];
        int* cur = A.cur + A.n_units * A.map_off[p] + (size_t)u * m;
        const int* next = A.next + A.n_units * A.map_off[p] + (size_t)u * m;
        const bool better = tm > best_tm || (tm == best_tm && u < best[0]);
        int differ = 0;
        for (int r = lane; r < m; r += 64) {
            const int was = cur[r], now = next[r];
            if (better) A.best_map[A.map_off[p] + r] = was;
            differ |= was != now;
            cur[r] = now;
        }
        differ = __ballot(differ) != 0ull;
        if (better) {
            best_tm = tm;
            best[0] = u; best[1] = A.round; best[2] = score; best[3] = nal;
        }
        if (lane == 0) {
            double* h = A.history + (unit * A.rounds + A.round) * 3;
            h[0] = tm;
            h[1] = (double)score;
            h[2] = (double)nal;
            A.state[2 * unit] = new_nal;
            A.state[2 * unit + 1] = !differ || new_nal < 3;
        }
    }
    if (lane == 0) {
        A.best_tm[p] = best_tm;
        for (int c = 0; c < 4; ++c) A.best[4 * p + c] = best[c];
    }
}

struct SaFinal {
    const int *offs, *pairs;
    const long long* map_off;
    const int *pair_bad, *win_of, *best;
    const uint8_t* codes;
    const float *tm_a, *tm_b, *rmsd;            // [winners]
    const double *rot_a, *tr_a, *rot_b, *tr_b;
    const int* map;
    int *n_aligned, *n_ident, *dp_score, *unit, *round;
    float *tm, *rmsd_out;
    double *rot, *tr;
};

// a wave per pair: its outputs from the winner's two final searches (the transform is that of the search normalised by the shorter chain)
__global__ __launch_bounds__(64) void k_sa_final(const SaFinal A) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int ia = A.pairs[2 * p], ib = A.pairs[2 * p + 1], oa = A.offs[ia], ob = A.offs[ib], m = A.offs[ia + 1] - oa, n = A.offs[ib + 1] - ob;
    const int w = A.win_of[p];
    int na = 0, ni = 0;
    if (w >= 0)
        for (int r = lane; r < m; r += 64) {
            const int j = A.map[A.map_off[p] + r];
            na += j >= 0 ? 1 : 0;
            ni += j >= 0 && A.codes && A.codes[oa + r] == A.codes[ob + j] ? 1 : 0;
        }
    na = wave_sum(na);
    ni = wave_sum(ni);
    if (lane != 0) return;
    const bool bad = A.pair_bad[p] != 0;
    A.n_aligned[p] = na;
    A.n_ident[p] = ni;
    A.dp_score[p] = w >= 0 ? A.best[4 * p + 2] : 0;
    A.unit[p] = w >= 0 ? A.best[4 * p] : -1;
    A.round[p] = w >= 0 ? A.best[4 * p + 1] : -1;
    A.tm[2 * p] = bad ? NAN : w >= 0 ? A.tm_a[w] : 0.f;
    A.tm[2 * p + 1] = bad ? NAN : w >= 0 ? A.tm_b[w] : 0.f;
    A.rmsd_out[p] = w >= 0 ? A.rmsd[w] : NAN;
    const double* R = m <= n ? A.rot_a : A.rot_b;
    const double* t = m <= n ? A.tr_a : A.tr_b;
    for (int c = 0; c < 9; ++c) A.rot[9 * (size_t)p + c] = bad ? (double)NAN : w >= 0 ? R[9 * (size_t)w + c] : (c % 4 == 0 ? 1.0 : 0.0);
    for (int c = 0; c < 3; ++c) A.tr[3 * (size_t)p + c] = bad ? (double)NAN : w >= 0 ? t[3 * (size_t)w + c] : 0.0;
}

// rmsd[w] of winner w: pesto_fit_rmsd's fit and deviation (pesto_fit.h: the text k_fit_rmsd runs, so the same bits) on its gathered pairs,
// a workgroup per winner in ONE launch; structs[w] says where its points lie in sel
__global__ __launch_bounds__(NT) void k_sa_rmsd(const TmStruct* __restrict__ structs, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                const int* __restrict__ sel, double scale, float* __restrict__ rmsd_out) {
    __shared__ double red[NT / 64];
    __shared__ double sR[9];
    const int* sl = sel + structs[blockIdx.x].s0;
    const int L = structs[blockIdx.x].L;
    Fit ft;
    kabsch_fit<NT, true>(atoms(xyz, sl), atoms(ref, sl), L, red, sR, ft);
    const double dev = moved_deviation<NT>(atoms(xyz, sl), atoms(ref, sl), L, ft, red);
    if (threadIdx.x == 0) rmsd_out[blockIdx.x] = (float)(sqrt(dev / (double)L) * scale);
}

__global__ __launch_bounds__(NT) void k_sa_iota(long long n, int* __restrict__ out) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    if (k < n) out[k] = (int)k;
}

// bad[s] = structure s has a non-finite coordinate (a workgroup per structure)
__global__ __launch_bounds__(NT) void k_sa_finite(const int* __restrict__ offs, const float* __restrict__ xyz, int* __restrict__ bad) {
    const int s = blockIdx.x;
    int b = 0;
    for (size_t q = 3 * (size_t)offs[s] + threadIdx.x; q < 3 * (size_t)offs[s + 1]; q += NT) b |= !(fabsf(xyz[q]) <= 3.402823466e38f);
    b = __syncthreads_or(b);
    if (threadIdx.x == 0) bad[s] = b;
}

// the fragment starts of a chain of len residues: 0, stride, 2 stride, ... <= len - f, plus len - f
std::vector<int> frag_starts_of(int len, int f, int frag_starts) {
    const int last = len - f, stride = std::max(1, (last + frag_starts - 2) / (frag_starts - 1));
    std::vector<int> out;
    for (int s = 0; s <= last; s += stride) out.push_back(s);
    if (out.back() != last) out.push_back(last);
    return out;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_structalign_last_error(void) { return last_error(); }

int pesto_structalign(pesto_model* mdl, int32_t S, const int32_t* offsets, const float* xyz, const uint8_t* codes, int64_t P, const int32_t* pairs,
                      const int32_t* init, const double* d0, double gap_open, int32_t rounds, int32_t frag_starts, double scale, int32_t* map_out,
                      int32_t* n_aligned_out, int32_t* n_ident_out, int32_t* dp_score_out, int32_t* unit_out, int32_t* round_out, float* tm_out,
                      double* rotation_out, double* translation_out, float* rmsd_out, double* history_out, int32_t ptr_kind, void* stream) {
    if (!offsets || !xyz || !pairs || !d0 || !map_out || !n_aligned_out || !n_ident_out || !dp_score_out || !unit_out || !round_out || !tm_out ||
        !rotation_out || !translation_out || !rmsd_out || !history_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (S < 1 || S > PESTO_STRUCTALIGN_MAX_STRUCTURES) return fail(PESTO_ERR_INVALID, "1 to %d structures, got %d", PESTO_STRUCTALIGN_MAX_STRUCTURES, S);
    if (P < 1 || P > PESTO_STRUCTALIGN_MAX_PAIRS) return fail(PESTO_ERR_INVALID, "1 to %d pairs, got %lld", PESTO_STRUCTALIGN_MAX_PAIRS, (long long)P);
    if (rounds < 1 || rounds > PESTO_STRUCTALIGN_MAX_ROUNDS) return fail(PESTO_ERR_INVALID, "1 to %d rounds, got %d", PESTO_STRUCTALIGN_MAX_ROUNDS, rounds);
    if (frag_starts < PESTO_STRUCTALIGN_MIN_FRAG_STARTS || frag_starts > PESTO_STRUCTALIGN_MAX_FRAG_STARTS)
        return fail(PESTO_ERR_INVALID, "%d to %d frag_starts, got %d", PESTO_STRUCTALIGN_MIN_FRAG_STARTS, PESTO_STRUCTALIGN_MAX_FRAG_STARTS, frag_starts);
    if (!(gap_open >= 0.0 && gap_open <= 1.0)) return fail(PESTO_ERR_INVALID, "0 <= gap_open <= 1 expected");
    if (!(std::isfinite(scale) && scale > 0.0)) return fail(PESTO_ERR_INVALID, "scale must be positive and finite");
    if (offsets[0] != 0) return fail(PESTO_ERR_INVALID, "offsets must start at 0");
    auto len = [&](int s) { return offsets[s + 1] - offsets[s]; };
    for (int s = 0; s < S; ++s) {
        const int64_t L = (int64_t)offsets[s + 1] - offsets[s];
        if (L < PESTO_STRUCTALIGN_MIN_LENGTH || L > PESTO_STRUCTALIGN_MAX_LENGTH)
            return fail(PESTO_ERR_INVALID, "structure %d: %d to %d residues, got %lld", s, PESTO_STRUCTALIGN_MIN_LENGTH, PESTO_STRUCTALIGN_MAX_LENGTH, (long long)L);
    }
    const int NU = init ? 6 : 4, go = (int)std::lround(gap_open * Q);
    std::vector<long long> map_off((size_t)P);
    std::vector<double> ks((size_t)P);
    long long n_map = 0;
    int rows = 0, mn_max = 0;
    for (int64_t p = 0; p < P; ++p) {
        for (int c = 0; c < 2; ++c)
            if (pairs[2 * p + c] < 0 || pairs[2 * p + c] >= S) return fail(PESTO_ERR_INVALID, "pair %lld names structure %d of %d", (long long)p, pairs[2 * p + c], S);
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(d0[3 * p + c]) && d0[3 * p + c] > 0.0)) return fail(PESTO_ERR_INVALID, "pair %lld: d0 must be positive and finite", (long long)p);
        const int m = len(pairs[2 * p]), n = len(pairs[2 * p + 1]);
        map_off[(size_t)p] = n_map;
        n_map += m;
        ks[(size_t)p] = (scale * scale) / (d0[3 * p] * d0[3 * p]);
        if (n > BLOCK_COLS) rows = std::max(rows, m + 1);
        mn_max = std::max(mn_max, m + n);
    }
    if ((long long)NU * n_map > 0x7fffffffLL) return fail(PESTO_ERR_INVALID, "the maps of all units must stay below 2^31 entries: fewer or shorter pairs per call");
    if (init)
        for (int64_t p = 0; p < P; ++p) {
            const int m = len(pairs[2 * p]), n = len(pairs[2 * p + 1]);
            for (int r = 0, last = -1; r < m; ++r) {             // (an alignment: so at most min(m, n) residues are aligned)
                const int j = init[map_off[(size_t)p] + r];
                if (j < -1 || j >= n || (j >= 0 && j <= last))
                    return fail(PESTO_ERR_INVALID, "init: pair %lld maps residue %d to %d of %d; -1 or ascending indices expected", (long long)p, r, j, n);
                if (j >= 0) last = j;
            }
        }
    if (int rc = begin(mdl, ptr_kind)) return rc;

    const int64_t TU = P * NU;
    int64_t n_gather = 0;
    for (int64_t p = 0; p < P; ++p) n_gather += (int64_t)NU * std::min(len(pairs[2 * p]), len(pairs[2 * p + 1]));
    const int slots = (int)std::min<int64_t>(MAX_SLOTS, rows ? std::max<int64_t>(64, (int64_t)(BOUND_CAP / ((size_t)rows * ROW_INTS * 4))) : MAX_SLOTS);
    const size_t smem = (size_t)mn_max * 12;
    // the item list holds a round's units or a chunk of threading offsets and fragment pairs (a chunk ends with the pair that fills it)
    int64_t n_setup = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int m = len(pairs[2 * p]), n = len(pairs[2 * p + 1]), lmin = std::min(m, n), f = std::min(lmin, std::max(4, std::min(20, lmin / 3)));
        n_setup += m + n - 2 * std::max(3, (lmin + 1) / 2) + 1 + (int64_t)frag_starts_of(m, f, frag_starts).size() * (int64_t)frag_starts_of(n, f, frag_starts).size();
    }
    const int64_t n_items = std::max<int64_t>(TU, std::min<int64_t>(n_setup, CHUNK_ITEMS + 2 * (int64_t)PESTO_STRUCTALIGN_MAX_LENGTH + (int64_t)65 * 65));

    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)offsets[S] * 12), iC = bf.input(codes, (size_t)offsets[S]);
    const int iO = bf.table(offsets, ((size_t)S + 1) * 4), iP = bf.table(pairs, (size_t)P * 8), iMo = bf.table(map_off.data(), (size_t)P * 8),
              iK = bf.table(ks.data(), (size_t)P * 8), iIn = init ? bf.table(init, (size_t)n_map * 4) : -1;
    const int oMap = bf.output(map_out, (size_t)n_map * 4, 0xff), oNa = bf.output(n_aligned_out, (size_t)P * 4), oNi = bf.output(n_ident_out, (size_t)P * 4),
              oSc = bf.output(dp_score_out, (size_t)P * 4), oUn = bf.output(unit_out, (size_t)P * 4), oRo = bf.output(round_out, (size_t)P * 4),
              oTm = bf.output(tm_out, (size_t)P * 8), oR = bf.output(rotation_out, (size_t)P * 72), oT = bf.output(translation_out, (size_t)P * 24),
              oRm = bf.output(rmsd_out, (size_t)P * 4), oH = bf.output(history_out, (size_t)TU * rounds * 24, 0xff);
    const int sIo = bf.scratch((size_t)n_gather * 4);    // the identity selection of the searches, filled on the device
    const int sBad = bf.scratch((size_t)S * 4), sPb = bf.scratch((size_t)P * 4), sErr = bf.scratch(4, 0);
    const int sItems = bf.scratch((size_t)n_items * sizeof(SaItem)), sPick = bf.scratch((size_t)P * sizeof(SaPick));
    const int sRot = bf.scratch((size_t)n_items * 72), sTr = bf.scratch((size_t)n_items * 24), sScore = bf.scratch((size_t)n_items * 4),
              sNal = bf.scratch((size_t)TU * 4);
    const int sRot0 = bf.scratch((size_t)P * 72), sTr0 = bf.scratch((size_t)P * 24);
    const int sCur = bf.scratch((size_t)NU * n_map * 4), sNext = bf.scratch((size_t)NU * n_map * 4), sState = bf.scratch((size_t)TU * 8);
    const int sLive = bf.scratch((size_t)TU * 4), sBestTm = bf.scratch((size_t)P * 8), sBest = bf.scratch((size_t)P * 16, 0xff);
    const int sGx = bf.scratch((size_t)n_gather * 12), sGy = bf.scratch((size_t)n_gather * 12);
    const int sStructs = bf.scratch((size_t)TU * sizeof(TmStruct)), sParts = bf.scratch((size_t)(TU + 2048) * sizeof(TmBest));
    const int sTmv = bf.scratch((size_t)TU * 4 * 4), sCnt = bf.scratch((size_t)TU * 20), sSeed = bf.scratch((size_t)TU * 4);
    const int sRotB = bf.scratch((size_t)P * 72), sTrB = bf.scratch((size_t)P * 24), sRms = bf.scratch((size_t)P * 4), sWin = bf.scratch((size_t)P * 4);
    // the predecessor bytes of the traced launches: chunks under the cap (a pair alone always fits: 16 MiB at most)
    const size_t tb_cap = (size_t)PESTO_STRUCTALIGN_WORKSPACE;
    size_t tb_need = 0;
    for (int64_t p = 0; p < P; ++p) tb_need += (((size_t)len(pairs[2 * p]) * len(pairs[2 * p + 1]) + 4 + 255) & ~(size_t)255) * NU;
    const int sTb = bf.scratch(std::min(tb_need, tb_cap)), sBound = rows ? bf.scratch((size_t)slots * rows * ROW_INTS * 4) : -1;

    int rc = bf.upload();
    hipStream_t stm = bf.stm;
    // THE RULE for the host tables this call rebuilds (items, picks, structs, live_of ...): up() returns only when the host buffer has been
    // consumed - it synchronises the stream - so a table may be changed or freed as soon as up() is back, whatever memory it lies in. The
    // rounds end on a synchronisation anyway; what is lost is the overlap of a few small copies with the kernels in front of them.
    auto up = [&](int item, const void* host, size_t bytes) {
        if (!bytes) return 0;
        if (int e = hip_ok(hipMemcpyAsync(bf.ptr<void>(item), host, bytes, hipMemcpyHostToDevice, stm), "copy to the device failed")) return e;
        return hip_ok(hipStreamSynchronize(stm), "structalign");
    };
    if (rc == 0) rc = hip_ok(hipFuncSetAttribute((const void*)k_sa_dp<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "structalign");
    if (rc == 0) rc = hip_ok(hipFuncSetAttribute((const void*)k_sa_dp<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "structalign");

    SaArgs a{};
    std::vector<int32_t> bad((size_t)S), pair_bad((size_t)P);
    if (rc == 0) {
        a.xyz = bf.ptr<const float>(iX); a.offs = bf.ptr<const int>(iO); a.pairs = bf.ptr<const int>(iP); a.ks = bf.ptr<const double>(iK);
        a.items = bf.ptr<const SaItem>(sItems); a.bound = rows ? bf.ptr<int>(sBound) : nullptr; a.bound_rows = rows; a.tb = bf.ptr<uint8_t>(sTb);
        hipLaunchKernelGGL(k_sa_iota, dim3(blocks((size_t)n_gather, NT)), dim3(NT), 0, stm, (long long)n_gather, bf.ptr<int>(sIo));
        hipLaunchKernelGGL(k_sa_finite, dim3((unsigned)S), dim3(NT), 0, stm, a.offs, a.xyz, bf.ptr<int>(sBad));
        rc = bf.verdict(sBad, bad.data(), (size_t)S * 4, "structalign");
    }
    if (rc == 0) {
        for (int64_t p = 0; p < P; ++p) pair_bad[(size_t)p] = bad[(size_t)pairs[2 * p]] | bad[(size_t)pairs[2 * p + 1]];
        rc = up(sPb, pair_bad.data(), (size_t)P * 4);
    }

    // a traced launch list: the items' predecessor bytes laid out, chunk after chunk under the cap
    std::vector<SaItem> items;
    auto run_traced = [&](const double* rot, const double* tr, int* score, int* nal, int* maps) {
        size_t used = 0;
        std::vector<int64_t> chunk_at{0};
        for (size_t k = 0; k < items.size(); ++k) {
            SaItem& it = items[k];
            const size_t bytes = ((size_t)len(pairs[2 * it.pair]) * len(pairs[2 * it.pair + 1]) + 4 + 255) & ~(size_t)255;
            if (used && used + bytes > tb_cap) {
                chunk_at.push_back((int64_t)k);
                used = 0;
            }
            it.tb_off = (long long)used;
            used += bytes;
        }
        chunk_at.push_back((int64_t)items.size());
        if (int e = up(sItems, items.data(), items.size() * sizeof(SaItem))) return e;
        SaArgs t = a;
        t.rot = rot; t.tr = tr; t.score = score; t.nal = nal; t.maps = maps;
        for (size_t c = 0; c + 1 < chunk_at.size(); ++c) {
            t.k0 = chunk_at[c];
            t.k1 = chunk_at[c + 1];
            if (t.k1 > t.k0)
                hipLaunchKernelGGL(k_sa_dp<true>, dim3((unsigned)std::min<int64_t>(slots, t.k1 - t.k0)), dim3(64), smem, stm, t);
        }
        return bf.launched("structalign");
    };
    auto unit_map = [&](int64_t p, int u) { return (long long)NU * map_off[(size_t)p] + (long long)u * len(pairs[2 * p]); };

    // ---- the initial alignments, a chunk of pairs at a time: threading sums and fragment fits, the scores-only DP, the picks
    for (int64_t p0 = 0; rc == 0 && p0 < P;) {
        std::vector<SaPick> picks;
        items.clear();
        std::vector<SaItem> frags;
        int64_t p1 = p0;
        for (; p1 < P && (p1 == p0 || (int64_t)(items.size() + frags.size()) < CHUNK_ITEMS); ++p1) {
            SaPick pk{};
            if (!pair_bad[(size_t)p1]) {
                const int m = len(pairs[2 * p1]), n = len(pairs[2 * p1 + 1]), lmin = std::min(m, n), minov = std::max(3, (lmin + 1) / 2);
                pk.thr_lo = (int)items.size();
                pk.kmin = -(m - minov);
                for (int k = pk.kmin; k <= n - minov; ++k) {
                    const int fa = std::max(0, -k), ov = std::min(m, n - k) - fa;
                    items.push_back(SaItem{(int)p1, 0, (int)items.size(), fa, fa + k, ov, 0, 0, 0, 0});
                }
                pk.thr_n = (int)items.size() - pk.thr_lo;
                const int f = std::min(lmin, std::max(4, std::min(20, lmin / 3)));
                pk.frag_lo = (int)frags.size();
                for (int fa : frag_starts_of(m, f, frag_starts))
                    for (int fb : frag_starts_of(n, f, frag_starts)) frags.push_back(SaItem{(int)p1, 0, (int)frags.size(), fa, fb, f, 0, 0, 0, 0});
                pk.frag_n = (int)frags.size() - pk.frag_lo;
            }
            picks.push_back(pk);
        }
        const int64_t n_thr = (int64_t)items.size(), n_frag = (int64_t)frags.size();
        for (SaItem& it : frags) it.tf = (int)n_thr + it.dst;      // (k_sa_frag stores an item's fit at its place in the list)
        items.insert(items.end(), frags.begin(), frags.end());
        if (n_thr) {
            rc = up(sItems, items.data(), items.size() * sizeof(SaItem));
            if (rc == 0) rc = up(sPick, picks.data(), picks.size() * sizeof(SaPick));
            if (rc == 0) {
                SaArgs t = a;
                t.k0 = 0; t.k1 = n_thr; t.score = bf.ptr<int>(sScore);
                hipLaunchKernelGGL(k_sa_thread, dim3((unsigned)n_thr), dim3(64), 0, stm, t);
                // the fragment items follow the threading items in the list; their fits and scores are indexed by the item
                t.k0 = n_thr; t.k1 = n_thr + n_frag;
                hipLaunchKernelGGL(k_sa_frag, dim3((unsigned)n_frag), dim3(64), 0, stm, t, bf.ptr<double>(sRot), bf.ptr<double>(sTr));
                t.rot = bf.ptr<const double>(sRot); t.tr = bf.ptr<const double>(sTr);
                t.score = bf.ptr<int>(sScore) + n_thr;
                hipLaunchKernelGGL(k_sa_dp<false>, dim3((unsigned)std::min<int64_t>(slots, n_frag)), dim3(64), smem, stm, t);
                hipLaunchKernelGGL(k_sa_pick, dim3((unsigned)(p1 - p0)), dim3(64), 0, stm, (int)p0, NU, bf.ptr<const SaPick>(sPick), a.offs, a.pairs,
                                   bf.ptr<const long long>(iMo), bf.ptr<const int>(sScore), bf.ptr<const int>(sScore) + n_thr,
                                   bf.ptr<const double>(sRot) + 9 * n_thr, bf.ptr<const double>(sTr) + 3 * n_thr, bf.ptr<int>(sCur), bf.ptr<double>(sRot0),
                                   bf.ptr<double>(sTr0));
                rc = bf.launched("structalign");
            }
        }
        p0 = p1;
    }
    // I2's alignment: the traced DP under the best fragment fit, gap 0, into unit 2's map
    if (rc == 0) {
        items.clear();
        for (int64_t p = 0; p < P; ++p)
            if (!pair_bad[(size_t)p]) items.push_back(SaItem{(int)p, 0, (int)p, 0, 0, 0, (int)p, 0, 0, unit_map(p, 2)});
        if (!items.empty()) rc = run_traced(bf.ptr<const double>(sRot0), bf.ptr<const double>(sTr0), bf.ptr<int>(sScore), bf.ptr<int>(sNal), bf.ptr<int>(sCur));
    }
    std::vector<int32_t> state((size_t)TU * 2);
    if (rc == 0) {
        hipLaunchKernelGGL(k_sa_start, dim3((unsigned)P), dim3(64), 0, stm, NU, a.offs, a.pairs, bf.ptr<const long long>(iMo), bf.ptr<const int>(sPb),
                           init ? bf.ptr<const int>(iIn) : nullptr, bf.ptr<int>(sCur), bf.ptr<int>(sState));
        std::vector<double> minus((size_t)P, -1.0);
        rc = up(sBestTm, minus.data(), (size_t)P * 8);
        if (rc == 0) rc = bf.verdict(sState, state.data(), (size_t)TU * 8, "structalign");
    }

    // ---- the rounds
    std::vector<TmStruct> structs;
    std::vector<int32_t> live_of((size_t)TU);
    std::vector<SaItem> gat;
    // the search of the batch laid out in `gat` / `structs` on the gathered points
    auto search = [&](const int* maps, float* tm, double* rot, double* tr) {
        if (int e = up(sStructs, structs.data(), structs.size() * sizeof(TmStruct))) return e;
        if (maps) {
            if (int e = up(sItems, gat.data(), gat.size() * sizeof(SaItem))) return e;
            SaArgs t = a;
            t.k0 = 0; t.k1 = (long long)gat.size(); t.maps = (int*)maps;
            hipLaunchKernelGGL(k_sa_gather, dim3((unsigned)gat.size()), dim3(64), 0, stm, t, bf.ptr<float>(sGx), bf.ptr<float>(sGy));
        }
        int L_max = 0, seeds_max = 0;
        for (const TmStruct& s : structs) { L_max = std::max(L_max, s.L); seeds_max = std::max(seeds_max, s.n_seeds); }
        const int64_t U = (int64_t)structs.size();
        float* tv = bf.ptr<float>(sTmv);
        return hip_ok(tm_search_launch(stm, U, n_gather, (int)U, tm_shares(seeds_max, U), L_max, 20, scale, bf.ptr<const TmStruct>(sStructs),
                                       bf.ptr<const float>(sGy), bf.ptr<const float>(sGx), bf.ptr<const int>(sIo), bf.ptr<const int>(sErr),
                                       bf.ptr<TmBest>(sParts), tm, tv + TU, tv + 2 * TU, bf.ptr<int>(sCnt), bf.ptr<int>(sSeed), rot, tr),
                      "structalign");
    };
    for (int r = 0; rc == 0 && r < rounds; ++r) {
        gat.clear();
        structs.clear();
        items.clear();
        long long at = 0;
        for (int64_t u = 0; u < TU; ++u) {
            live_of[(size_t)u] = -1;
            const int64_t p = u / NU;
            const int na = state[2 * (size_t)u];
            if (state[2 * (size_t)u + 1] || na < 3) continue;
            live_of[(size_t)u] = (int32_t)gat.size();
            const int g = (int)(u % NU) % 2 == 0 ? go : 0;
            gat.push_back(SaItem{(int)p, g, (int)u, 0, 0, 0, (int)gat.size(), 0, at, unit_map(p, (int)(u % NU))});
            TmStruct s;
            const int lmin = std::min(len(pairs[2 * p]), len(pairs[2 * p + 1]));
            tm_plan((int)at, na, std::max(1, na >> 3), (double)lmin, d0[3 * p], s);
            structs.push_back(s);
            at += na;
        }
        if (gat.empty()) break;
        rc = search(bf.ptr<const int>(sCur), bf.ptr<float>(sTmv), bf.ptr<double>(sRot), bf.ptr<double>(sTr));
        if (rc == 0) {
            items = gat;
            rc = run_traced(bf.ptr<const double>(sRot), bf.ptr<const double>(sTr), bf.ptr<int>(sScore), bf.ptr<int>(sNal), bf.ptr<int>(sNext));
        }
        if (rc == 0) rc = up(sLive, live_of.data(), (size_t)TU * 4);
        if (rc == 0) {
            // (the traced DP writes a unit's new map where its old one lies in the other array: map_off is the unit's in both)
            SaRound ra{NU, rounds, r, a.offs, a.pairs, bf.ptr<const long long>(iMo), bf.ptr<const int>(sLive), bf.ptr<const float>(sTmv),
                       bf.ptr<const int>(sScore), bf.ptr<const int>(sNal), bf.ptr<int>(sCur), bf.ptr<int>(sNext), bf.ptr<int>(oMap), bf.ptr<int>(sState),
                       bf.ptr<double>(sBestTm), bf.ptr<int>(sBest), bf.ptr<double>(oH)};
            hipLaunchKernelGGL(k_sa_round, dim3((unsigned)P), dim3(64), 0, stm, ra);
            rc = bf.verdict(sState, state.data(), (size_t)TU * 8, "structalign");
        }
    }

    // ---- the winners' two final searches (step 1, normalised by m and by n), their RMSD and the outputs
    std::vector<int32_t> best((size_t)P * 4), win_of((size_t)P, -1);
    if (rc == 0) rc = bf.verdict(sBest, best.data(), (size_t)P * 16, "structalign");
    if (rc == 0) {
        gat.clear();
        structs.clear();
        std::vector<TmStruct> by_n;
        long long at = 0;
        for (int64_t p = 0; p < P; ++p) {
            if (best[4 * (size_t)p] < 0) continue;
            const int na = best[4 * (size_t)p + 3];
            win_of[(size_t)p] = (int32_t)gat.size();
            gat.push_back(SaItem{(int)p, 0, (int)p, 0, 0, 0, 0, 0, at, map_off[(size_t)p]});
            TmStruct s;
            tm_plan((int)at, na, 1, (double)len(pairs[2 * p]), d0[3 * p + 1], s);
            structs.push_back(s);
            tm_plan((int)at, na, 1, (double)len(pairs[2 * p + 1]), d0[3 * p + 2], s);
            by_n.push_back(s);
            at += na;
        }
        rc = up(sWin, win_of.data(), (size_t)P * 4);
        float* tv = bf.ptr<float>(sTmv);
        if (rc == 0 && !gat.empty()) {
            rc = search(bf.ptr<const int>(oMap), tv, bf.ptr<double>(sRot), bf.ptr<double>(sTr));
            if (rc == 0)
                hipLaunchKernelGGL(k_sa_rmsd, dim3((unsigned)structs.size()), dim3(NT), 0, stm, bf.ptr<const TmStruct>(sStructs), bf.ptr<const float>(sGy),
                                   bf.ptr<const float>(sGx), bf.ptr<const int>(sIo), scale, bf.ptr<float>(sRms));
            structs = by_n;                                                         // (the device's copy is replaced in stream order)
            if (rc == 0) rc = search(nullptr, tv + 3 * TU, bf.ptr<double>(sRotB), bf.ptr<double>(sTrB));
        }
        if (rc == 0) {
            SaFinal fa{a.offs, a.pairs, bf.ptr<const long long>(iMo), bf.ptr<const int>(sPb), bf.ptr<const int>(sWin), bf.ptr<const int>(sBest),
                       codes ? bf.ptr<const uint8_t>(iC) : nullptr, tv, tv + 3 * TU, bf.ptr<const float>(sRms), bf.ptr<const double>(sRot),
                       bf.ptr<const double>(sTr), bf.ptr<const double>(sRotB), bf.ptr<const double>(sTrB), bf.ptr<const int>(oMap), bf.ptr<int>(oNa),
                       bf.ptr<int>(oNi), bf.ptr<int>(oSc), bf.ptr<int>(oUn), bf.ptr<int>(oRo), bf.ptr<float>(oTm), bf.ptr<float>(oRm), bf.ptr<double>(oR),
                       bf.ptr<double>(oT)};
            hipLaunchKernelGGL(k_sa_final, dim3((unsigned)P), dim3(64), 0, stm, fa);
        }
    }
    return bf.finish(rc, "structalign");
}
