// pesto_alignwave.h - Gotoh's three-state recursion of ONE WAVE over one pair, shared by the sequence alignment (pesto_align.hip: the cell
// score is a substitution-matrix lookup) and the structure alignment (pesto_structalign.hip: the cell score comes from the distance of
// two residues under a superposition). The two differ in nothing but the SCORE SOURCE the recursion is templated on, so ties, ends,
// carries, column blocks and predecessor bytes are one text.
//
// Lane l owns the strip of W = 8 columns jb + 8 l + 1 .. jb + 8 l + 8 of b and sweeps the rows of a skewed by one lane: at step t it is
// on row t - l. What a strip hands to the next is M[i][last] (the best of D, U, L, the diagonal predecessor of row i + 1) and
// L[i][last + 1], value and carry: six dwords by __shfl_up. Sequences longer than one pass of 64 strips (512 columns) run in column
// blocks; the block's last column goes through `bound`, 24 bytes per row (lane 63 stores row i, lane 0 of the next block loads it one
// step ahead of its use). THE FIRST IN THE ORDER D, U, L WINS A TIE, so there is exactly one canonical path.
//
// A score source supplies
//     Col column(int j, int n)                what a lane keeps of column j (1-based) of b in registers (one above n is never an output)
//     Row row(int i)                          what it keeps of row i (1-based) of a while it does its strip
//     int score(const Row&, const Col&)       the score of the cell
//     bool ident(const Row&, const Col&)      whether the cell counts as an identity
//
// Everything sits in an anonymous namespace (one copy per translation unit).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace pesto {

namespace {

namespace wave {

constexpr int W = 8;                            // columns of a lane's strip
constexpr int BLOCK_COLS = 64 * W;              // columns of one pass
constexpr int NEG = -(1 << 29);                 // minus infinity: real scores stay within +-(127 * 8192 + 127 * 8193) for the matrix source and
                                                // within 1024 * 4096 + 1024 * 8192 for the geometric one, and so does the drift of what derives
                                                // from NEG, so it neither overflows nor wins
constexpr unsigned HI_MASK = 0x03ffffffu;       // i0 | j0 << 13 of a carry's second dword; bits 26-27: which state a maximum took
constexpr int ROW_INTS = 6;                     // a boundary row: M and L, value and two carry dwords each

enum { MODE_GLOBAL = 0, MODE_OVERLAP = 1, MODE_LOCAL = 2 };

// a state's value and the counts of its canonical path: lo = n_ident | n_aligned << 13, hi = i0 | j0 << 13
struct Cell { int v; unsigned lo, hi; };

__device__ __forceinline__ int ldg(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stg(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the best of a - pa, b - pb, c - pc, the first on ties, with its carry (and, for the traceback, which one in bits 26-27 of hi)
template <bool TRACE>
__device__ __forceinline__ Cell best3(const Cell& a, int pa, const Cell& b, int pb, const Cell& c, int pc) {
    Cell r = a;
    r.v = a.v - pa;
    unsigned arg = 0;
    const int bv = b.v - pb, cv = c.v - pc;
    if (bv > r.v) { r = b; r.v = bv; arg = 1; }
    if (cv > r.v) { r = c; r.v = cv; arg = 2; }
    if (TRACE) r.hi |= arg << 26;
    return r;
}

// the states of the border cells (0, j) and (i, 0)
template <int MODE>
__device__ __forceinline__ void border(int i, int j, int go, int ge, Cell& D, Cell& U, Cell& L) {
    D = U = L = Cell{NEG, 0u, 0u};
    if (MODE == MODE_GLOBAL) {
        if (i == 0 && j == 0) D.v = 0;
        else if (i == 0) L.v = -(go + (j - 1) * ge);
        else U.v = -(go + (i - 1) * ge);
    } else if (MODE == MODE_OVERLAP) {
        D.v = 0;
        D.hi = (unsigned)i | (unsigned)j << 13;
    }
}

__device__ __forceinline__ Cell shift_up(const Cell& c) { return Cell{__shfl_up(c.v, 1), __shfl_up(c.lo, 1), __shfl_up(c.hi, 1)}; }

// (v, i, j) ordered as the end rule has it: the larger value, then the smaller i, then the smaller j
__device__ __forceinline__ bool ends_before(int v, int i, int j, int v2, int i2, int j2) { return v > v2 || (v == v2 && (i < i2 || (i == i2 && j < j2))); }

struct End { int v, i, j; unsigned lo, hi; };

// One wave, one pair: a of m rows against b of n columns, scored by `src`. Returns the end cell of the canonical path with its value and
// carry in every lane (for MODE_GLOBAL hi keeps the end's state in bits 26-27 when TRACE). tb (TRACE): one byte per cell, row-major [m, n].
template <int MODE, bool TRACE, class SRC>
__device__ End align_wave(const SRC src, int m, int n, int go, int ge, int* bound, uint8_t* tb) {
    const int lane = threadIdx.x & 63;
    End best{INT_MIN, 0, 0, 0u, 0u};
    for (int jb = 0; jb < n; jb += BLOCK_COLS) {
        const bool first = jb == 0, more = jb + BLOCK_COLS < n;
        const int j0 = jb + lane * W;           // the strip is columns j0 + 1 .. j0 + W
        const int n_act = min(64, (n - jb + W - 1) / W);
        Cell Mp[W], Un[W];
        typename SRC::Col bc[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int j = j0 + c + 1;
            bc[c] = src.column(j, n);
            Cell D, U, L;
            border<MODE>(0, j, go, ge, D, U, L);
            Mp[c] = best3<TRACE>(D, 0, U, 0, L, 0);
            Un[c] = best3<TRACE>(D, go, U, ge, L, go);
        }
        Cell dsave;                             // M[i - 1][j0] for the row the lane is about to do
        {
            Cell D, U, L;
            border<MODE>(0, j0, go, ge, D, U, L);
            dsave = best3<TRACE>(D, 0, U, 0, L, 0);
        }
        End blk{INT_MIN, 0, 0, 0u, 0u};
        Cell sendM{NEG, 0u, 0u}, sendL{NEG, 0u, 0u}, nextM{NEG, 0u, 0u}, nextL{NEG, 0u, 0u};
        auto load_row = [&](int i) {
            const int* r = bound + (size_t)i * ROW_INTS;
            nextM = Cell{ldg(r), (unsigned)ldg(r + 1), (unsigned)ldg(r + 2)};
            nextL = Cell{ldg(r + 3), (unsigned)ldg(r + 4), (unsigned)ldg(r + 5)};
        };
        if (!first && lane == 0) load_row(1);
        const int steps = m + n_act - 1;
        for (int t = 1; t <= steps; ++t) {
            const int i = t - lane;
            Cell inM = shift_up(sendM), inL = shift_up(sendL);
            if (lane == 0) {
                if (first) {
                    Cell D, U, L;
                    border<MODE>(min(t, m), 0, go, ge, D, U, L);
                    inM = best3<TRACE>(D, 0, U, 0, L, 0);
                    inL = best3<TRACE>(D, go, U, go, L, ge);
                } else {
                    inM = nextM;
                    inL = nextL;
                    if (t < m) load_row(t + 1);
                }
            }
            if (i >= 1 && i <= m) {
                Cell diag = dsave, Lc = inL;
                dsave = inM;
                const auto r = src.row(i);
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const int j = j0 + c + 1;
                    const Cell above = Mp[c];
                    const int s = src.score(r, bc[c]);
                    Cell D{diag.v + s, diag.lo, TRACE ? diag.hi & HI_MASK : diag.hi};
                    unsigned pD = diag.hi >> 26;
                    if (MODE == MODE_LOCAL && diag.v < 0) {         // the fresh start is the last candidate: only below zero
                        D = Cell{s, 0u, (unsigned)(i - 1) | (unsigned)(j - 1) << 13};
                        pD = 3;
                    }
                    D.lo += (1u << 13) + (src.ident(r, bc[c]) ? 1u : 0u);
                    Cell U = Un[c], L = Lc;
                    if (TRACE) {
                        const unsigned pU = U.hi >> 26, pL = L.hi >> 26;
                        U.hi &= HI_MASK;
                        L.hi &= HI_MASK;
                        if (j <= n) tb[(size_t)(i - 1) * n + (j - 1)] = (uint8_t)(pD | pU << 2 | pL << 4);
                    }
                    const Cell M = best3<TRACE>(D, 0, U, 0, L, 0);
                    Un[c] = best3<TRACE>(D, go, U, ge, L, go);
                    Lc = best3<TRACE>(D, go, U, go, L, ge);
                    Mp[c] = M;
                    diag = above;
                    if (MODE == MODE_GLOBAL) {
                        if (i == m && j == n) blk = End{M.v, i, j, M.lo, M.hi};
                    } else {                                        // rows, then columns ascend: the first maximum met is the rule's
                        const bool cand = MODE == MODE_LOCAL ? j <= n : (j == n || (i == m && j < n));
                        if (cand && D.v > blk.v) blk = End{D.v, i, j, D.lo, D.hi};
                    }
                }
                sendM = Mp[W - 1];
                sendL = Lc;
                if (more && lane == 63) {
                    int* r = bound + (size_t)i * ROW_INTS;
                    stg(r, sendM.v); stg(r + 1, (int)sendM.lo); stg(r + 2, (int)sendM.hi);
                    stg(r + 3, sendL.v); stg(r + 4, (int)sendL.lo); stg(r + 5, (int)sendL.hi);
                }
            }
        }
        if (ends_before(blk.v, blk.i, blk.j, best.v, best.i, best.j)) best = blk;
        if (more) __threadfence();
    }
    for (int o = 32; o > 0; o >>= 1) {
        const End e{__shfl_xor(best.v, o), __shfl_xor(best.i, o), __shfl_xor(best.j, o), __shfl_xor(best.lo, o), __shfl_xor(best.hi, o)};
        if (ends_before(e.v, e.i, e.j, best.v, best.i, best.j)) best = e;
    }
    return best;
}

// The canonical path of an OVERLAP or LOCAL alignment walked back by ONE lane from its end (i1, j1) through the predecessor bytes: map[i]
// = the column of row i (0-based) or -1 for every row the path crosses; returns the path's first cell in (i0, j0) and its number of D
// columns. The rows outside [i0, i1) are the caller's to fill.
__device__ __forceinline__ int walk_back(const uint8_t* tb, int n, int i1, int j1, int* map, int& i0, int& j0) {
    int i = i1, j = j1, na = 0;
    unsigned st = 0;
    while (i > 0 && j > 0) {
        const size_t at = (size_t)(i - 1) * n + (j - 1);
        const unsigned word = (unsigned)ldg((const int*)(tb + (at & ~(size_t)3)));
        const unsigned pred = (word >> (8 * (at & 3)) >> (2 * st)) & 3u;
        if (st == 0) {
            map[i - 1] = j - 1;
            ++na;
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
    i0 = i;
    j0 = j;
    return na;
}

}  // namespace wave
}  // namespace
}  // namespace pesto
