// pesto_dynamics.hip - essential dynamics of MD frames: per-atom fluctuations (RMSF), the positional covariance matrix, the dynamic
// cross-correlation map and the principal components of the frames with the projection of frames on them (Amadei et al. 1993). The
// reference contains none of this; the definition is this library's (include/pesto_hip.h) and is checked against a float64 restatement.
//
// With x_f the selected coordinates of frame f flattened to m = 3 n values, all in double from the float32 inputs:
//     mean = (1/F) sum_f x_f,   d_f = (double)x_f - mean (centred BEFORE multiplying),   C = scale^2 sum_f d_f d_f^T / (F - ddof)
//
// k_dyn_mean      per coordinate: the mean and sum_f d^2 over the frames in a fixed order, and the selected coordinates packed as a
//                 [F][mp] float32 image (mp = m padded to a multiple of 64 with zero columns whose mean is 0)
// k_dyn_mma<MODE> ONE tile skeleton for the four tall products: the 64 x 64 double-precision tile of pesto_mma64.h (K staged through LDS
//                 16 deep), the operands centred while they are loaded (the K tail is zero rows of d, not of x):
//                     GRAM  [m x F] . [F x m]   covariance: only the tiles i <= j, mirrored through LDS, so C is bitwise symmetric
//                     DQ    [F x m] . [m x 64]  D Q of the solver, and every projection
//                     DTZ   [m x F] . [F x 64]  D^T (D Q)
//                     QTY   [64 x m] . [m x 64] Q^T Y and the Gram matrix Y^T Y of the orthonormalisation
//                 the last three split K over blockIdx.y into partial tiles that k_dyn_reduce adds in a fixed order (no float atomics)
// k_dyn_jacobi    one workgroup: the eigenvectors of a symmetric 64 x 64 matrix by one-sided Jacobi (jacobi_angle of pesto_geom.h: columns of
//                 A V rotated until orthogonal to JTOL), 32 disjoint column pairs per step in round-robin order, sorted descending
// k_dyn_rotate    Out = In . V (. diag(1 / sqrt(s)) with the directions below a relative threshold zeroed: the orthonormalisation, whose
//                 Gram matrix is scaled to a unit diagonal before its Jacobi; twice, then one Newton-Schulz step, k_dyn_polish)
// k_dyn_resid / k_dyn_check   the residual columns Y V - Q V Theta, their norms, the null directions, the done flag
// k_dyn_components            the sign rule, the zero rows beyond the rank, the basis for the projections
// k_dyn_dccm      the epilogue over the 3 x 3 blocks of C
// The solver is block subspace iteration with Rayleigh-Ritz on 64 vectors, matrix-free (pca never forms C). Every sum runs in a fixed
// order that depends on the shapes alone, so every output is bit-identical from call to call.
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_geom.h"
#include "pesto_mma64.h"

namespace pesto {
namespace {

constexpr int NT = 256;
constexpr int TS = MT;          // rows and columns of a tile (pesto_mma64.h); also the width of the solver's block of vectors
constexpr int MG = 16;          // k_dyn_mean: coordinates per workgroup, and frame groups
constexpr int ROUNDS = 4;       // solver iterations enqueued between two reads of the done flag
constexpr double DROP = 1e-13;  // orthonormalisation: a direction whose Gram eigenvalue is below DROP x the largest is zeroed (the Gram
                                // matrix itself is only known to some 64 eps of its largest eigenvalue)
constexpr double JTOL = 64 * 2.220446049250313e-16;      // k_dyn_jacobi: two columns count as orthogonal at |a_p . a_q| <= JTOL |a_p| |a_q|: the
                                // rounding of that 64-term dot product itself is some 8 eps of |a_p| |a_q|, so a tighter test rotates on noise and never ends
constexpr double RANK_TOL = 1e-12;   // a Ritz value at or below RANK_TOL x the largest is a null direction

struct DynState {
    double total;               // tr C
    int32_t done, iterations, converged, rank;
    int32_t sweeps, pad;        // the most Jacobi sweeps any of the call's 64 x 64 eigenproblems took
};

// ---- mean, square sums, the packed image
// Workgroup b: the coordinates 16 b .. 16 b + 15; thread (c, g) adds the frames g, g + 16, ... of coordinate c, the 16 partial sums are
// added in order. given: the mean is an argument (project), float32 [m].
__global__ __launch_bounds__(NT) void k_dyn_mean(int F, int N, int m, int mp, const float* __restrict__ xyz, const int* __restrict__ sel,
                                                 const float* __restrict__ given, float* __restrict__ Xp, double* __restrict__ mean,
                                                 double* __restrict__ sq) {
    __shared__ double part[MG][MG + 1];
    const int c = threadIdx.x & (MG - 1), g = threadIdx.x >> 4, j = blockIdx.x * MG + c;
    const bool live = j < m;
    size_t off = 0;
    if (live) off = (size_t)(sel ? sel[j / 3] : j / 3) * 3 + j % 3;
    const size_t stride = (size_t)N * 3;
    double s = 0.0;
    for (int f = g; f < F; f += MG) {
        const float x = live ? xyz[(size_t)f * stride + off] : 0.f;
        s += (double)x;
        if (Xp) Xp[(size_t)f * mp + j] = x;
    }
    part[g][c] = s;
    __syncthreads();
    double mu = 0.0;
    for (int q = 0; q < MG; ++q) mu += part[q][c];
    mu /= (double)F;
    if (given) mu = live ? (double)given[j] : 0.0;
    __syncthreads();
    double v = 0.0;
    if (live)
        for (int f = g; f < F; f += MG) {
            const double d = (double)xyz[(size_t)f * stride + off] - mu;
            v += d * d;
        }
    part[g][c] = v;
    __syncthreads();
    if (g == 0) {
        double t = 0.0;
        for (int q = 0; q < MG; ++q) t += part[q][c];
        mean[j] = live ? mu : 0.0;
        sq[j] = live ? t : 0.0;
    }
}

__global__ void k_dyn_fluct(int m, int F, double scale, const double* __restrict__ mean, const double* __restrict__ sq, float* __restrict__ mean_out,
                            float* __restrict__ rmsf_out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    if (mean_out) mean_out[j] = (float)mean[j];
    if (rmsf_out && j % 3 == 0) rmsf_out[j / 3] = (float)(scale * sqrt(((sq[j] + sq[j + 1]) + sq[j + 2]) / (double)F));
}

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

// tr C = fac sum_j sq[j], and the state's start
__global__ __launch_bounds__(NT) void k_dyn_total(int m, double fac, const double* __restrict__ sq, DynState* __restrict__ st) {
    __shared__ double red[NT / 64];
    double s = 0.0;
    for (int j = threadIdx.x; j < m; j += NT) s += sq[j];
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) { st->total = s * fac; st->done = 0; st->iterations = 0; st->converged = 0; st->rank = 0; st->sweeps = 0; st->pad = 0; }
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

// One workgroup of 64 threads: the residual norms, the null directions among the first k (theta <= RANK_TOL theta[0]: eigenvalue 0,
// residual 0), converged = max residual <= tol theta[0]; the Ritz values and residuals are kept for the result.
__global__ __launch_bounds__(TS) void k_dyn_check(int k, int nparts, double tol, const double* __restrict__ theta, const double* __restrict__ partial,
                                                  double* __restrict__ theta_keep, double* __restrict__ resid_keep, DynState* __restrict__ st) {
    __shared__ double res[TS];
    __shared__ int live[TS];
    if (st->done) return;
    const int c = threadIdx.x;
    double s = 0.0;
    for (int q = 0; q < nparts; ++q) s += partial[(size_t)q * TS + c];
    const double th0 = theta[0];
    const bool null_dir = !(th0 > 0.0 && theta[c] > RANK_TOL * th0);
    res[c] = null_dir ? 0.0 : sqrt(s);
    live[c] = !null_dir;
    theta_keep[c] = null_dir ? 0.0 : theta[c];
    resid_keep[c] = res[c];
    __syncthreads();
    if (c == 0) {
        double worst = 0.0;
        int rank = 0;
        for (int i = 0; i < k; ++i) { worst = fmax(worst, res[i]); rank += live[i]; }
        const int conv = worst <= tol * fmax(th0, 0.0);
        st->iterations += 1; st->converged = conv; st->rank = rank;
        if (conv) st->done = 1;
    }
}

// Workgroup c of 64: component c of the result. Sign rule: the entry of largest magnitude positive, the lowest index on ties. A null
// direction (theta_keep = 0) and, in the basis, the columns from k on are zero. basis [m][64]: the components as columns, for DQ.
__global__ __launch_bounds__(NT) void k_dyn_components(int m, int k, const double* __restrict__ X, const double* __restrict__ theta_keep,
                                                       const double* __restrict__ resid_keep, double* __restrict__ eig_out, double* __restrict__ comp_out,
                                                       double* __restrict__ resid_out, double* __restrict__ basis) {
    __shared__ double bv[NT];
    __shared__ int bi[NT];
    const int c = blockIdx.x;
    const bool zero = c >= k || !(theta_keep[c] > 0.0);
    double best = -1.0;
    int at = 0x7fffffff;
    if (!zero)
        for (int r = threadIdx.x; r < m; r += NT) {
            const double v = fabs(X[(size_t)r * TS + c]);
            if (v > best) { best = v; at = r; }
        }
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const double ov = bv[threadIdx.x + o];
            const int oi = bi[threadIdx.x + o];
            if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = ov; bi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    double sign = 0.0;
    if (!zero) sign = bi[0] < m && X[(size_t)bi[0] * TS + c] < 0.0 ? -1.0 : 1.0;          // (bi[0] >= m: nothing finite to compare)
    for (int r = threadIdx.x; r < m; r += NT) {
        const double v = zero ? 0.0 : sign * X[(size_t)r * TS + c];
        basis[(size_t)r * TS + c] = v;
        if (c < k) comp_out[(size_t)c * m + r] = v;
    }
    if (threadIdx.x == 0 && c < k) { eig_out[c] = zero ? 0.0 : theta_keep[c]; resid_out[c] = zero ? 0.0 : resid_keep[c]; }
}

// basis [m][64] from components float64 [k][m] (project)
__global__ void k_dyn_basis(int m, int k, const double* __restrict__ comp, double* __restrict__ basis) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m * TS) return;
    const int r = (int)(e >> 6), c = (int)(e & 63);
    basis[e] = c < k ? comp[(size_t)c * m + r] : 0.0;
}

__global__ void k_dyn_proj(int F, int k, double scale, const double* __restrict__ P, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)F * k) return;
    const size_t f = e / k;
    out[e] = (float)(scale * P[f * TS + (e - f * k)]);
}

// DCCM[i][j] = tr C_ij / sqrt(tr C_ii tr C_jj), 1 on the diagonal, 0 where an atom has no variance
__global__ void k_dyn_dccm(int n, const double* __restrict__ C, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * n) return;
    const size_t i = e / n, j = e - i * n, m = 3 * (size_t)n;
    auto tr = [&](size_t a, size_t b) { return (C[(3 * a) * m + 3 * b] + C[(3 * a + 1) * m + 3 * b + 1]) + C[(3 * a + 2) * m + 3 * b + 2]; };
    const double di = tr(i, i), dj = tr(j, j);
    out[e] = i == j ? 1.f : di > 0.0 && dj > 0.0 ? (float)(tr(i, j) / sqrt(di * dj)) : 0.f;
}

// ---- host side
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

int check_frames(int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale) {
    if (!xyz) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DYNAMICS_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to 2^24 frames, got %lld", (long long)F);
    if (N < 1 || N > PESTO_DYNAMICS_MAX_ATOMS || n_sel < 1 || n_sel > N || (!sel && n_sel != N))
        return fail(PESTO_ERR_INVALID, "1 <= n_sel <= N <= 2^24 atoms (n_sel = N without a selection)");
    if (!std::isfinite(scale)) return fail(PESTO_ERR_INVALID, "scale must be finite");
    return 0;
}

Mma mma_of(const Shape& s, const float* Xp, const double* mean, const DynState* st) {
    Mma a{};
    a.F = (int)s.F; a.m = (int)s.m; a.mp = (int)s.mp; a.Xp = Xp; a.mean = mean; a.st = st;
    return a;
}

void reduce(hipStream_t stm, int S, int64_t rows_pad, int64_t nrows, double fac, const double* partial, double* out, const DynState* st) {
    hipLaunchKernelGGL(k_dyn_reduce, dim3((unsigned)((nrows * TS + NT - 1) / NT)), dim3(NT), 0, stm, S, (int)rows_pad, (int)nrows, fac, partial, out, st);
}

// P [F][64] = D B, B [mp][64] (rows from m on zero)
void launch_dq(hipStream_t stm, const Shape& s, Mma a, const double* B, double* partial, double* P) {
    a.B = B; a.K = (int)s.mp; a.chunk = s.dq.chunk; a.out = partial;
    hipLaunchKernelGGL(k_dyn_mma<M_DQ>, dim3((unsigned)(s.Fp / TS), (unsigned)s.dq.S), dim3(NT), 0, stm, a);
    reduce(stm, s.dq.S, s.Fp, s.F, 1.0, partial, P, a.st);
}
// Y [m][64] = fac D^T P
void launch_dtz(hipStream_t stm, const Shape& s, Mma a, const double* P, double fac, double* partial, double* Y) {
    a.B = P; a.K = (int)s.F; a.chunk = s.dtz.chunk; a.out = partial;
    hipLaunchKernelGGL(k_dyn_mma<M_DTZ>, dim3((unsigned)(s.mp / TS), (unsigned)s.dtz.S), dim3(NT), 0, stm, a);
    reduce(stm, s.dtz.S, s.mp, s.m, fac, partial, Y, a.st);
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

using namespace pesto;

const char* pesto_dynamics_last_error(void) { return last_error(); }

int pesto_fluctuations(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale, float* mean_out,
                       float* rmsf_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_frames(F, N, n_sel, xyz, sel, scale)) return rc;
    if (!mean_out || !rmsf_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = begin(m, ptr_kind)) return rc;
    const Shape s = shape_of(F, N, n_sel);
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iM = bf.output(mean_out, (size_t)s.m * 4), iR = bf.output(rmsf_out, (size_t)n_sel * 4);
    const int iMean = bf.scratch((size_t)s.mp * 8), iSq = bf.scratch((size_t)s.mp * 8);
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_dyn_mean, dim3((unsigned)(s.mp / MG)), dim3(NT), 0, bf.stm, (int)F, (int)N, (int)s.m, (int)s.mp, bf.ptr<const float>(iX),
                           sel ? bf.ptr<const int>(iS) : nullptr, (const float*)nullptr, (float*)nullptr, bf.ptr<double>(iMean), bf.ptr<double>(iSq));
        hipLaunchKernelGGL(k_dyn_fluct, dim3((unsigned)((s.m + NT - 1) / NT)), dim3(NT), 0, bf.stm, (int)s.m, (int)F, scale, bf.ptr<const double>(iMean),
                           bf.ptr<const double>(iSq), bf.ptr<float>(iM), bf.ptr<float>(iR));
    }
    return bf.finish(rc, "fluctuations");
}

// the covariance (C_out) or, with dccm_out, the cross-correlation map through a covariance in scratch
static int covariance_call(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale, int32_t ddof,
                           double* C_out, float* dccm_out, int32_t ptr_kind, void* stream, const char* what) {
    if (int rc = check_frames(F, N, n_sel, xyz, sel, scale)) return rc;
    if (!C_out && !dccm_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if ((ddof != 0 && ddof != 1) || F - ddof < 1) return fail(PESTO_ERR_INVALID, "ddof must be 0 or 1 and F - ddof >= 1");
    if (9 * n_sel * n_sel > PESTO_DYNAMICS_MAX_COV) return fail(PESTO_ERR_INVALID, "(3 n_sel)^2 <= 2^27 entries, got n_sel = %lld", (long long)n_sel);
    if (int rc = begin(m, ptr_kind)) return rc;
    const Shape s = shape_of(F, N, n_sel);
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iC = C_out ? bf.output(C_out, (size_t)(s.m * s.m) * 8) : bf.scratch((size_t)(s.m * s.m) * 8);
    const int iD = dccm_out ? bf.output(dccm_out, (size_t)(n_sel * n_sel) * 4) : -1;
    const int iXp = bf.scratch((size_t)F * s.mp * 4), iMean = bf.scratch((size_t)s.mp * 8), iSq = bf.scratch((size_t)s.mp * 8);
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_dyn_mean, dim3((unsigned)(s.mp / MG)), dim3(NT), 0, bf.stm, (int)F, (int)N, (int)s.m, (int)s.mp, bf.ptr<const float>(iX),
                           sel ? bf.ptr<const int>(iS) : nullptr, (const float*)nullptr, bf.ptr<float>(iXp), bf.ptr<double>(iMean), bf.ptr<double>(iSq));
        Mma a = mma_of(s, bf.ptr<const float>(iXp), bf.ptr<const double>(iMean), nullptr);
        const int T = (int)(s.mp / TS);
        a.K = (int)F; a.chunk = (int)((F + KC - 1) / KC * KC); a.out = bf.ptr<double>(iC); a.fac = scale * scale / (double)(F - ddof); a.T = T;
        hipLaunchKernelGGL(k_dyn_mma<M_GRAM>, dim3((unsigned)(T * T)), dim3(NT), 0, bf.stm, a);
        if (dccm_out)
            hipLaunchKernelGGL(k_dyn_dccm, dim3((unsigned)((n_sel * n_sel + NT - 1) / NT)), dim3(NT), 0, bf.stm, (int)n_sel, bf.ptr<const double>(iC),
                               bf.ptr<float>(iD));
    }
    return bf.finish(rc, what);
}

int pesto_covariance(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale, int32_t ddof, double* C_out,
                     int32_t ptr_kind, void* stream) {
    if (!C_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    return covariance_call(m, F, N, n_sel, xyz, sel, scale, ddof, C_out, nullptr, ptr_kind, stream, "covariance");
}

int pesto_cross_correlation(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, float* dccm_out, int32_t ptr_kind,
                            void* stream) {
    if (!dccm_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    return covariance_call(m, F, N, n_sel, xyz, sel, 1.0, 0, nullptr, dccm_out, ptr_kind, stream, "cross_correlation");
}

int pesto_pca(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, int32_t k, double scale, int32_t ddof, double tol,
              int32_t max_iter, double* eig_out, double* comp_out, float* proj_out, float* mean_out, double* resid_out, double* total_variance_out,
              int32_t* info_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_frames(F, N, n_sel, xyz, sel, scale)) return rc;
    if (!eig_out || !comp_out || !proj_out || !mean_out || !resid_out || !total_variance_out || !info_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if ((ddof != 0 && ddof != 1) || F - ddof < 1) return fail(PESTO_ERR_INVALID, "ddof must be 0 or 1 and F - ddof >= 1");
    if (k < 1 || k > PESTO_DYNAMICS_MAX_COMPONENTS || k > 3 * n_sel)
        return fail(PESTO_ERR_INVALID, "1 <= n_components <= min(%d, 3 n_sel), got %d", PESTO_DYNAMICS_MAX_COMPONENTS, k);
    if (!(tol >= 0.0) || !std::isfinite(tol) || max_iter < 1) return fail(PESTO_ERR_INVALID, "tol must be finite and >= 0, max_iter >= 1");
    if (int rc = begin(m, ptr_kind)) return rc;
    const Shape s = shape_of(F, N, n_sel);
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iE = bf.output(eig_out, (size_t)k * 8), iCo = bf.output(comp_out, (size_t)k * s.m * 8), iPr = bf.output(proj_out, (size_t)F * k * 4);
    const int iMo = bf.output(mean_out, (size_t)s.m * 4), iRo = bf.output(resid_out, (size_t)k * 8);
    const int iXp = bf.scratch((size_t)F * s.mp * 4), iMean = bf.scratch((size_t)s.mp * 8), iSq = bf.scratch((size_t)s.mp * 8);
    const size_t vec = (size_t)s.mp * TS * 8;
    // the block vectors' rows from m on are read as K padding by DQ: Q and X zero once, never written
    const int iQ = bf.scratch(vec, 0), iY = bf.scratch(vec), iXv = bf.scratch(vec, 0), iZ = bf.scratch(vec), iTmp = bf.scratch(vec);
    const int iP = bf.scratch((size_t)s.Fp * TS * 8), iPart = bf.scratch(s.partial_doubles() * 8);
    const int iT = bf.scratch(TS * TS * 8), iV = bf.scratch(TS * TS * 8), iTh = bf.scratch(TS * 8), iSv = bf.scratch(TS * 8);
    const int iThK = bf.scratch(TS * 8), iRsK = bf.scratch(TS * 8);
    const int nparts = (int)(s.mp / TS) * 4;
    const int iRp = bf.scratch((size_t)nparts * TS * 8), iSt = bf.scratch(sizeof(DynState));
    int rc = bf.upload();
    DynState state{};
    if (rc == 0) rc = hip_ok(hipFuncSetAttribute((const void*)k_dyn_jacobi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JACOBI_LDS), "pca");
    if (rc == 0) {
        hipStream_t stm = bf.stm;
        DynState* st = bf.ptr<DynState>(iSt);
        double *Q = bf.ptr<double>(iQ), *Y = bf.ptr<double>(iY), *X = bf.ptr<double>(iXv), *Z = bf.ptr<double>(iZ), *Tmp = bf.ptr<double>(iTmp);
        double *P = bf.ptr<double>(iP), *part = bf.ptr<double>(iPart), *T = bf.ptr<double>(iT), *V = bf.ptr<double>(iV), *th = bf.ptr<double>(iTh);
        double* sv = bf.ptr<double>(iSv);
        const double fac = scale * scale / (double)(F - ddof);
        const unsigned gv = (unsigned)((s.m * TS + NT - 1) / NT), gr = (unsigned)((s.m + 15) / 16);
        hipLaunchKernelGGL(k_dyn_mean, dim3((unsigned)(s.mp / MG)), dim3(NT), 0, stm, (int)F, (int)N, (int)s.m, (int)s.mp, bf.ptr<const float>(iX),
                           sel ? bf.ptr<const int>(iS) : nullptr, (const float*)nullptr, bf.ptr<float>(iXp), bf.ptr<double>(iMean), bf.ptr<double>(iSq));
        hipLaunchKernelGGL(k_dyn_total, dim3(1), dim3(NT), 0, stm, (int)s.m, fac, bf.ptr<const double>(iSq), st);
        const Mma a = mma_of(s, bf.ptr<const float>(iXp), bf.ptr<const double>(iMean), st);
        hipLaunchKernelGGL(k_dyn_start, dim3(gv), dim3(NT), 0, stm, (int)s.m, Z);
        launch_ortho(stm, s, a, Z, Tmp, Q, part, T, V, sv);
        for (int it = 0; rc == 0 && !state.done && it < max_iter;) {
            const int upto = std::min(max_iter, it + ROUNDS);
            for (; it < upto; ++it) {
                launch_dq(stm, s, a, Q, part, P);
                launch_dtz(stm, s, a, P, fac, part, Y);
                launch_qty(stm, s, a, Q, Y, part, T);
                hipLaunchKernelGGL(k_dyn_jacobi, dim3(1), dim3(NT), JACOBI_LDS, stm, T, 0, V, th, st);
                hipLaunchKernelGGL(k_dyn_rotate, dim3(gr), dim3(NT), 0, stm, (int)s.m, Q, V, (const double*)nullptr, X, st);
                hipLaunchKernelGGL(k_dyn_rotate, dim3(gr), dim3(NT), 0, stm, (int)s.m, Y, V, (const double*)nullptr, Z, st);
                hipLaunchKernelGGL(k_dyn_resid, dim3((unsigned)(s.mp / TS)), dim3(NT), 0, stm, (int)s.m, X, Z, th, bf.ptr<double>(iRp), st);
                hipLaunchKernelGGL(k_dyn_check, dim3(1), dim3(TS), 0, stm, (int)k, nparts, tol, th, bf.ptr<const double>(iRp), bf.ptr<double>(iThK),
                                   bf.ptr<double>(iRsK), st);
                launch_ortho(stm, s, a, Z, Tmp, Q, part, T, V, sv);          // the next block
            }
            rc = bf.verdict(iSt, &state, sizeof state, "pca");
        }
        if (rc == 0) {
            Mma b = a;
            b.st = nullptr;
            hipLaunchKernelGGL(k_dyn_components, dim3(TS), dim3(NT), 0, stm, (int)s.m, (int)k, X, bf.ptr<const double>(iThK), bf.ptr<const double>(iRsK),
                               bf.ptr<double>(iE), bf.ptr<double>(iCo), bf.ptr<double>(iRo), Y);
            // Y now holds the basis; its rows from m on are K padding of DQ
            if (s.mp > s.m) rc = hip_ok(hipMemsetAsync(Y + (size_t)s.m * TS, 0, (size_t)(s.mp - s.m) * TS * 8, stm), "pca");
            launch_dq(stm, s, b, Y, part, P);
            hipLaunchKernelGGL(k_dyn_proj, dim3((unsigned)((F * k + NT - 1) / NT)), dim3(NT), 0, stm, (int)F, (int)k, scale, P, bf.ptr<float>(iPr));
            hipLaunchKernelGGL(k_dyn_fluct, dim3((unsigned)((s.m + NT - 1) / NT)), dim3(NT), 0, stm, (int)s.m, (int)F, scale, bf.ptr<const double>(iMean),
                               bf.ptr<const double>(iSq), bf.ptr<float>(iMo), (float*)nullptr);
        }
    }
    if (rc == 0) {
        *total_variance_out = state.total;
        info_out[0] = state.rank; info_out[1] = state.iterations; info_out[2] = state.converged; info_out[3] = state.sweeps;
    }
    return bf.finish(rc, "pca");
}

int pesto_project(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, int32_t k, const float* mean,
                  const double* components, double scale, float* proj_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_frames(F, N, n_sel, xyz, sel, scale)) return rc;
    if (!mean || !components || !proj_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (k < 1 || k > TS) return fail(PESTO_ERR_INVALID, "1 to %d components, got %d", TS, k);
    if (int rc = begin(m, ptr_kind)) return rc;
    const Shape s = shape_of(F, N, n_sel);
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iS = bf.input(sel, (size_t)n_sel * 4), iMi = bf.input(mean, (size_t)s.m * 4);
    const int iCi = bf.input(components, (size_t)k * s.m * 8), iPr = bf.output(proj_out, (size_t)F * k * 4);
    const int iXp = bf.scratch((size_t)F * s.mp * 4), iMean = bf.scratch((size_t)s.mp * 8), iSq = bf.scratch((size_t)s.mp * 8);
    const size_t vec = (size_t)s.mp * TS * 8;
    const int iB = bf.scratch(vec, 0), iP = bf.scratch((size_t)s.Fp * TS * 8), iPart = bf.scratch((size_t)s.dq.S * s.Fp * TS * 8);
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_dyn_mean, dim3((unsigned)(s.mp / MG)), dim3(NT), 0, bf.stm, (int)F, (int)N, (int)s.m, (int)s.mp, bf.ptr<const float>(iX),
                           sel ? bf.ptr<const int>(iS) : nullptr, bf.ptr<const float>(iMi), bf.ptr<float>(iXp), bf.ptr<double>(iMean), bf.ptr<double>(iSq));
        hipLaunchKernelGGL(k_dyn_basis, dim3((unsigned)((s.m * TS + NT - 1) / NT)), dim3(NT), 0, bf.stm, (int)s.m, (int)k, bf.ptr<const double>(iCi),
                           bf.ptr<double>(iB));
        const Mma a = mma_of(s, bf.ptr<const float>(iXp), bf.ptr<const double>(iMean), nullptr);
        launch_dq(bf.stm, s, a, bf.ptr<const double>(iB), bf.ptr<double>(iPart), bf.ptr<double>(iP));
        hipLaunchKernelGGL(k_dyn_proj, dim3((unsigned)((F * k + NT - 1) / NT)), dim3(NT), 0, bf.stm, (int)F, (int)k, scale, bf.ptr<const double>(iP),
                           bf.ptr<float>(iPr));
    }
    return bf.finish(rc, "project");
}
