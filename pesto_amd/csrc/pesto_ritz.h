// pesto_ritz.h - the 64-vector Rayleigh-Ritz machinery that the two eigensolvers of the analysis groups share: pca of pesto_dynamics.hip
// (the top of a covariance spectrum, block subspace iteration) and the elastic-network modes of pesto_enm.hip (the bottom of a Hessian's,
// Chebyshev-filtered subspace iteration). One text of each piece, moved here from pesto_dynamics.hip unchanged:
//   k_dyn_mma<MODE>   the tile skeleton of the tall products on the 64 x 64 double-precision tile of pesto_mma64.h; QTY ([64 x m] . [m x 64])
//                     is the mode both solvers use, GRAM / DQ / DTZ are pca's and the covariance's
//   k_dyn_reduce      the partial tiles of a K split added in a fixed order
//   k_dyn_start       the start block, a fixed counter hash
//   k_dyn_jacobi      the eigenvectors of a symmetric 64 x 64 matrix by one-sided Jacobi, sorted descending
//   k_dyn_polish / k_dyn_rotate / launch_ortho   the Gram orthonormalisation, twice, with its Newton-Schulz step
//   k_dyn_resid       the residual columns' partial square sums
// Everything sits in an anonymous namespace (one copy per translation unit, like pesto_call.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_geom.h"
#include "pesto_mma64.h"

namespace pesto {
namespace {

constexpr int NT = 256;
constexpr int TS = MT;          // rows and columns of a tile (pesto_mma64.h); also the width of the solver's block of vectors
constexpr double DROP = 1e-13;  // orthonormalisation: a direction whose Gram eigenvalue is below DROP x the largest is zeroed (the Gram
                                // matrix itself is only known to some 64 eps of its largest eigenvalue)
constexpr double JTOL = 64 * 2.220446049250313e-16;      // k_dyn_jacobi: two columns count as orthogonal at |a_p . a_q| <= JTOL |a_p| |a_q|: the
                                // rounding of that 64-term dot product itself is some 8 eps of |a_p| |a_q|, so a tighter test rotates on noise and never ends
struct DynState {
    double total;               // tr C
    int32_t done, iterations, converged, rank;
    int32_t sweeps, pad;        // the most Jacobi sweeps any of the call's 64 x 64 eigenproblems took
};

// ---- the tile skeleton
enum { M_GRAM = 0, M_DQ = 1, M_DTZ = 2, M_QTY = 3 };

struct Mma {
    int F, m, mp;               // frames, coordinates, coordinates padded to 64
    const float* Xp;            // [F][mp]
    const double* mean;         // [mp]
    const double* A;            // QTY: [K][64]
    const double* B;            // DQ, DTZ, QTY: [K][64]
    int K, chunk;               // the product's depth and the part of it one blockIdx.y takes (a multiple of KC)
    double* out;                // GRAM: C [m][m]; else the partial tiles [gridDim.y][64 gridDim.x][64]
    double fac;                 // GRAM: scale^2 / (F - ddof)
    int T;                      // GRAM: tiles a side
    const DynState* st;         // the solver's state (NULL outside it): nothing to do once done
};

// operand (k = frame, row = coordinate base + ..): one float4 of a frame per thread, centred; mu: the thread's four means
__device__ __forceinline__ void load_dcols(const Mma& a, int base, const double* mu, int k0, int kend, f64x4& r) {
    const int f = k0 + (threadIdx.x >> 4);
    if (f >= kend) { r[0] = r[1] = r[2] = r[3] = 0.0; return; }          // the K tail: zero rows of d
    const float4 x = ((const float4*)(a.Xp + (size_t)f * a.mp + base))[threadIdx.x & 15];
    r[0] = (double)x.x - mu[0]; r[1] = (double)x.y - mu[1]; r[2] = (double)x.z - mu[2]; r[3] = (double)x.w - mu[3];
}
// operand (k = coordinate, row = frame f0 + ..): one float4 of four consecutive coordinates per thread, centred
__device__ __forceinline__ void load_drows(const Mma& a, int f0, int k0, int kend, f64x4& r) {
    const int f = f0 + (threadIdx.x >> 2), j = k0 + 4 * (threadIdx.x & 3);
    if (f >= a.F || j >= kend) { r[0] = r[1] = r[2] = r[3] = 0.0; return; }
    const float4 x = *(const float4*)(a.Xp + (size_t)f * a.mp + j);
    const double* mu = a.mean + j;
    r[0] = (double)x.x - mu[0]; r[1] = (double)x.y - mu[1]; r[2] = (double)x.z - mu[2]; r[3] = (double)x.w - mu[3];
}
// operand (k = row of M, column): four doubles of a row of a [K][64] matrix per thread
__device__ __forceinline__ void load_mat(const double* __restrict__ M, int k0, int kend, f64x4& r) {
    const int k = k0 + (threadIdx.x >> 4);
    if (k >= kend) { r[0] = r[1] = r[2] = r[3] = 0.0; return; }
    const double* p = M + (size_t)k * TS + 4 * (threadIdx.x & 15);
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
}
// load_drows' four values (rows 4 (tid % 4) .., column tid / 4) into a k-major stage
__device__ __forceinline__ void store_rowmajor(double* S, const f64x4& r) {
    double* d = S + (4 * (threadIdx.x & 3)) * LS + (threadIdx.x >> 2);
    d[0] = r[0]; d[LS] = r[1]; d[2 * LS] = r[2]; d[3 * LS] = r[3];
}

// Workgroup (tile, split): sum over k in [split chunk, min(K, (split + 1) chunk)) of A[k][row] B[k][col], one tile of pesto_mma64.h.
template <int MODE>
__global__ __launch_bounds__(NT) void k_dyn_mma(Mma a) {
    __shared__ double lds[MMA64_LDS];           // the staged operands, then (GRAM) the accumulator image
    if (a.st && a.st->done) return;
    int ti = blockIdx.x, tj = 0;
    if (MODE == M_GRAM) {
        ti = blockIdx.x / a.T; tj = blockIdx.x % a.T;
        if (tj < ti) return;
    }
    const int kbeg = blockIdx.y * a.chunk, kend = min(a.K, kbeg + a.chunk);
    double mua[4] = {0.0, 0.0, 0.0, 0.0}, mub[4] = {0.0, 0.0, 0.0, 0.0};
    if (MODE == M_GRAM || MODE == M_DTZ)
        for (int i = 0; i < 4; ++i) mua[i] = a.mean[TS * ti + 4 * (threadIdx.x & 15) + i];
    if (MODE == M_GRAM)
        for (int i = 0; i < 4; ++i) mub[i] = a.mean[TS * tj + 4 * (threadIdx.x & 15) + i];
    auto load = [&](int k0, f64x4& ra, f64x4& rb) {
        if (MODE == M_GRAM) { load_dcols(a, TS * ti, mua, k0, kend, ra); load_dcols(a, TS * tj, mub, k0, kend, rb); }
        if (MODE == M_DTZ) { load_dcols(a, TS * ti, mua, k0, kend, ra); load_mat(a.B, k0, kend, rb); }
        if (MODE == M_DQ) { load_drows(a, TS * ti, k0, kend, ra); load_mat(a.B, k0, kend, rb); }
        if (MODE == M_QTY) { load_mat(a.A, k0, kend, ra); load_mat(a.B, k0, kend, rb); }
    };
    auto store = [](double* As, const f64x4& ra) { MODE == M_DQ ? store_rowmajor(As, ra) : store_kmajor(As, ra); };
    f64x4 acc[4];
    mma64_loop<f64x4, false>(lds, kbeg, kend, load, store, acc);            // every stage in full: one beyond kend holds zeros
    if (MODE != M_GRAM) { mma64_store(acc, a.out + ((size_t)blockIdx.y * gridDim.x + ti) * TS * TS, TS, 1.0); return; }
    __syncthreads();
    mma64_store(acc, lds, HS, a.fac);
    __syncthreads();
    const int I = TS * ti, J = TS * tj;
    for (int e = threadIdx.x; e < TS * TS; e += NT) {
        const int r = e >> 6, c = e & 63;
        if (ti == tj) {         // the diagonal tile: the upper triangle on both sides
            if (I + r < a.m && J + c < a.m) a.out[(size_t)(I + r) * a.m + J + c] = lds[min(r, c) * HS + max(r, c)];
        } else {
            if (I + r < a.m && J + c < a.m) a.out[(size_t)(I + r) * a.m + J + c] = lds[r * HS + c];
            if (J + r < a.m && I + c < a.m) a.out[(size_t)(J + r) * a.m + I + c] = lds[c * HS + r];          // the mirror
        }
    }
}

// out[row][c] = fac sum_s partial[s][row][c], s in order; rows < nrows of rows_pad
__global__ void k_dyn_reduce(int S, int rows_pad, int nrows, double fac, const double* __restrict__ partial, double* __restrict__ out,
                             const DynState* __restrict__ st) {
    if (st && st->done) return;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nrows * TS) return;
    double s = 0.0;
    for (int q = 0; q < S; ++q) s += partial[(size_t)q * rows_pad * TS + e];
    out[e] = s * fac;
}

// ---- the solver's small kernels
// the start block: a fixed counter hash, uniform in (-1, 1)
__global__ void k_dyn_start(int m, double* __restrict__ Z) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m * TS) return;
    uint32_t x = (uint32_t)e * 0x9E3779B9u + 0x7F4A7C15u;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    Z[e] = (double)x * (1.0 / 2147483648.0) - 1.0;
}

// One workgroup: V (columns: eigenvectors) and theta of the symmetric part of T [64][64], sorted descending (the lower index first among
// equal ones). One-sided Jacobi on the columns of A = T V: thread (pair, sub) holds the rows sub, sub + 8, ... of one of the 32 disjoint
// column pairs of a round-robin step; theta_j = v_j . (T v_j). A zero column is never rotated, so V stays the identity there.
// normalise (the orthonormalisation's Gram matrix): T is first scaled to a unit diagonal, T' = S T S with S = diag(T)^-1/2 (0 for a zero
// column), and V_out = S V: the columns of a rotated block differ in norm like the eigenvalues, and T' is known entrywise to some m eps
// where T is only known to that fraction of its largest entry.
__global__ __launch_bounds__(NT) void k_dyn_jacobi(const double* __restrict__ T, int normalise, double* __restrict__ V_out, double* __restrict__ theta_out,
                                                   DynState* __restrict__ st) {
    extern __shared__ double jm[];              // A [64][HS], V [64][HS]
    __shared__ double th[TS], dinv[TS];
    __shared__ int rotated;
    if (st->done) return;
    double* A = jm;
    double* V = jm + TS * HS;
    if (threadIdx.x < TS) {
        const double d = T[threadIdx.x * TS + threadIdx.x];
        dinv[threadIdx.x] = !normalise ? 1.0 : d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TS * TS; e += NT) {
        const int r = e >> 6, c = e & 63;
        A[r * HS + c] = (0.5 * (T[r * TS + c] + T[c * TS + r])) * (dinv[r] * dinv[c]);
        V[r * HS + c] = r == c ? 1.0 : 0.0;
    }
    const int pair = threadIdx.x >> 3, sub = threadIdx.x & 7;
    for (int sweep = 0; sweep < 60; ++sweep) {
        if (threadIdx.x == 0) rotated = 0;
        __syncthreads();
        for (int step = 0; step < TS - 1; ++step) {
            int p, q;
            if (pair == 0) { p = TS - 1; q = step; }
            else { p = (step + pair) % (TS - 1); q = (step - pair + (TS - 1)) % (TS - 1); }
            if (p > q) { const int t = p; p = q; q = t; }
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
            for (int r = sub; r < TS; r += 8) {
                const double ap = A[r * HS + p], aq = A[r * HS + q];
                alpha += ap * ap; beta += aq * aq; gamma += ap * aq;
            }
            for (int o = 1; o < 8; o <<= 1) { alpha += __shfl_xor(alpha, o); beta += __shfl_xor(beta, o); gamma += __shfl_xor(gamma, o); }
            if (fabs(gamma) > JTOL * sqrt(alpha * beta)) {
                double c, s;
                jacobi_angle(alpha, beta, gamma, c, s);
                for (int r = sub; r < TS; r += 8) {
                    const double ap = A[r * HS + p], aq = A[r * HS + q], vp = V[r * HS + p], vq = V[r * HS + q];
                    A[r * HS + p] = c * ap - s * aq; A[r * HS + q] = s * ap + c * aq;
                    V[r * HS + p] = c * vp - s * vq; V[r * HS + q] = s * vp + c * vq;
                }
                if (sub == 0) rotated = 1;
            }
            __syncthreads();
        }
        const int any = rotated;
        __syncthreads();
        if (!any || sweep == 59) {
            if (threadIdx.x == 0 && st->sweeps < sweep + 1) st->sweeps = sweep + 1;
            break;
        }
    }
    if (threadIdx.x < TS) {
        double s = 0.0;
        for (int r = 0; r < TS; ++r) s += V[r * HS + threadIdx.x] * A[r * HS + threadIdx.x];
        th[threadIdx.x] = s;
    }
    __syncthreads();
    // The Ritz rotation (not the orthonormalisation, whose eigenvalues belong to the V they were taken with): some thousand plane rotations
    // leave V orthogonal to a few 1e-14 only; one Newton-Schulz step V (3 I - V^T V) / 2 takes that drift out (A is free now)
    if (!normalise) {
        for (int e = threadIdx.x; e < TS * TS; e += NT) {
            const int i = e >> 6, j = e & 63;
            double g = 0.0;
            for (int r = 0; r < TS; ++r) g += V[r * HS + i] * V[r * HS + j];
            A[i * HS + j] = (i == j ? 1.5 : 0.0) - 0.5 * g;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < TS * TS; e += NT) {
        const int r = e >> 6, j = e & 63;
        int rank = 0;
        for (int i = 0; i < TS; ++i) rank += th[i] > th[j] || (th[i] == th[j] && i < j);
        double v = V[r * HS + j];
        if (!normalise) {
            v = 0.0;
            for (int i = 0; i < TS; ++i) v += V[r * HS + i] * A[i * HS + j];
        }
        V_out[r * TS + rank] = dinv[r] * v;
        if (r == 0) theta_out[rank] = th[j];
    }
}

// M = (3 I - W) / 2 of the symmetric part of the Gram matrix W of a nearly orthonormal block: Q M is one Newton-Schulz step on Q (a zero
// column stays zero)
__global__ void k_dyn_polish(const double* __restrict__ W, double* __restrict__ M, const DynState* __restrict__ st) {
    if (st->done) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= TS * TS) return;
    const int i = e >> 6, j = e & 63;
    M[e] = (i == j ? 1.5 : 0.0) - 0.25 * (W[i * TS + j] + W[j * TS + i]);
}

// Out [m][64] = In [m][64] . Mx [64][64], 16 rows per workgroup. s (the orthonormalisation): column c times 1 / sqrt(s[c]), a direction with
// s[c] <= DROP s[0] zeroed.
__global__ __launch_bounds__(NT) void k_dyn_rotate(int m, const double* __restrict__ In, const double* __restrict__ Mx, const double* __restrict__ s,
                                                   double* __restrict__ Out, const DynState* __restrict__ st) {
    __shared__ double Ms[TS * TS];
    __shared__ double rows[16][TS];
    if (st->done) return;
    for (int e = threadIdx.x; e < TS * TS; e += NT) Ms[e] = Mx[e];
    const int r0 = blockIdx.x * 16;
    for (int e = threadIdx.x; e < 16 * TS; e += NT) {
        const int r = r0 + (e >> 6);
        rows[e >> 6][e & 63] = r < m ? In[(size_t)r * TS + (e & 63)] : 0.0;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    double sc = 1.0;
    if (s) sc = s[c] > DROP * s[0] && s[c] > 0.0 ? 1.0 / sqrt(s[c]) : 0.0;
    for (int i = g; i < 16; i += 4) {
        if (r0 + i >= m) break;
        double v = 0.0;
        for (int j = 0; j < TS; ++j) v += rows[i][j] * Ms[j * TS + c];
        Out[(size_t)(r0 + i) * TS + c] = sc == 0.0 ? 0.0 : v * sc;
    }
}

// partial[b][g][c] = sum over the rows 64 b + g, + 4, ... of (Z[r][c] - X[r][c] theta[c])^2
__global__ __launch_bounds__(NT) void k_dyn_resid(int m, const double* __restrict__ X, const double* __restrict__ Z, const double* __restrict__ theta,
                                                  double* __restrict__ partial, const DynState* __restrict__ st) {
    if (st->done) return;
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const double th = theta[c];
    double v = 0.0;
    for (int r = blockIdx.x * TS + g; r < min(m, (int)(blockIdx.x + 1) * TS); r += 4) {
        const double d = Z[(size_t)r * TS + c] - X[(size_t)r * TS + c] * th;
        v += d * d;
    }
    partial[((size_t)blockIdx.x * 4 + g) * TS + c] = v;
}

struct Split { int S, chunk; };
// the K split of a thin product of `tiles` tiles: enough workgroups for the device, at least 64 of K each, at most 64 parts; a function of
// the shapes alone
Split split_of(int64_t K, int64_t tiles) {
    int64_t S = std::max<int64_t>(1, 512 / tiles);
    S = std::min<int64_t>(std::min<int64_t>(S, (K + 63) / 64), 64);
    const int64_t chunk = ((K + S - 1) / S + KC - 1) / KC * KC;
    return Split{(int)((K + chunk - 1) / chunk), (int)chunk};
}

struct Shape {
    int64_t F, N, n, m, mp, Fp;
    Split dq, dtz, qty;
    size_t partial_doubles() const {
        return (size_t)std::max<int64_t>(std::max<int64_t>(dq.S * Fp, dtz.S * mp), qty.S * TS) * TS;
    }
};

Shape shape_of(int64_t F, int64_t N, int64_t n) {
    Shape s;
    s.F = F; s.N = N; s.n = n; s.m = 3 * n; s.mp = (s.m + TS - 1) / TS * TS; s.Fp = (F + TS - 1) / TS * TS;
    s.dq = split_of(s.mp, s.Fp / TS);
    s.dtz = split_of(F, s.mp / TS);
    s.qty = split_of(s.m, 1);
    return s;
}

Mma mma_of(const Shape& s, const float* Xp, const double* mean, const DynState* st) {
    Mma a{};
    a.F = (int)s.F; a.m = (int)s.m; a.mp = (int)s.mp; a.Xp = Xp; a.mean = mean; a.st = st;
    return a;
}

void reduce(hipStream_t stm, int S, int64_t rows_pad, int64_t nrows, double fac, const double* partial, double* out, const DynState* st) {
    hipLaunchKernelGGL(k_dyn_reduce, dim3((unsigned)((nrows * TS + NT - 1) / NT)), dim3(NT), 0, stm, S, (int)rows_pad, (int)nrows, fac, partial, out, st);
}

// T [64][64] = A^T B, both [m][64]
void launch_qty(hipStream_t stm, const Shape& s, Mma a, const double* A, const double* B, double* partial, double* T) {
    a.A = A; a.B = B; a.K = (int)s.m; a.chunk = s.qty.chunk; a.out = partial;
    hipLaunchKernelGGL(k_dyn_mma<M_QTY>, dim3(1, (unsigned)s.qty.S), dim3(NT), 0, stm, a);
    reduce(stm, s.qty.S, TS, TS, 1.0, partial, T, a.st);
}

constexpr size_t JACOBI_LDS = 2 * TS * HS * sizeof(double);

// Out = In orthonormalised once: the Gram matrix, its eigenvectors, In U / sqrt(s)
void ortho_pass(hipStream_t stm, const Shape& s, const Mma& a, const double* In, double* Out, double* partial, double* W, double* U, double* sv) {
    launch_qty(stm, s, a, In, In, partial, W);
    hipLaunchKernelGGL(k_dyn_jacobi, dim3(1), dim3(NT), JACOBI_LDS, stm, W, 1, U, sv, const_cast<DynState*>(a.st));
    hipLaunchKernelGGL(k_dyn_rotate, dim3((unsigned)((s.m + 15) / 16)), dim3(NT), 0, stm, (int)s.m, In, U, sv, Out, a.st);
}

// Q = Z orthonormalised: twice through the Gram matrix (once loses orthogonality as the condition number squared; Z is overwritten), then
// one Newton-Schulz step, which takes out what the rotations of the second Jacobi left (a few 1e-14)
void launch_ortho(hipStream_t stm, const Shape& s, const Mma& a, double* Z, double* Tmp, double* Q, double* partial, double* W, double* U, double* sv) {
    ortho_pass(stm, s, a, Z, Tmp, partial, W, U, sv);
    ortho_pass(stm, s, a, Tmp, Z, partial, W, U, sv);
    launch_qty(stm, s, a, Z, Z, partial, W);
    hipLaunchKernelGGL(k_dyn_polish, dim3(TS * TS / NT), dim3(NT), 0, stm, W, U, a.st);
    hipLaunchKernelGGL(k_dyn_rotate, dim3((unsigned)((s.m + 15) / 16)), dim3(NT), 0, stm, (int)s.m, Z, U, (const double*)nullptr, Q, a.st);
}

}  // namespace
}  // namespace pesto
