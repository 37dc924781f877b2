// pesto_enm.hip - elastic-network normal modes of ONE structure: the anisotropic network model (ANM, Atilgan et al. 2001) and the Gaussian
// network model (GNM, Bahar et al. 1997): the spring list, the dense Hessian / Kirchhoff matrix, the lowest modes without the rigid
// motions, and what is derived from modes (fluctuations, correlations, overlaps, deformed conformers). The reference contains none of
// this; the definition is this library's (include/pesto_hip.h) and is checked against a float64 restatement.
//
// The list, once per call: the selected nodes gathered (k_enm_gather: the selection's range and the coordinates' finiteness are the
// call's device verdict), the cell grid of pesto_cellgrid.h at cutoff / scale, a count pass over for_each_neighbour, the 64-bit scan of
// pesto_scan.h and a fill pass (k_enm_list, the idiom of k_lddt_list); a wave per row then sorts the row by j and stores the stiffness
// and, for the ANM, (r, k / |r|^2) beside it (k_enm_sort); the row sums in ascending j and b = 2 max_i sum_j k_ij follow.
// k_enm_apply<DIM>  the operator on a block of 64 vectors stored [n][DIM][64] in double, one wave per node, lane = column: a neighbour's
//                   values are DIM coalesced 512-byte reads, the row is walked in list order, so every column sums in the same fixed
//                   order. The spring's geometry comes from the packed list (32 bytes an entry, read through the scalar unit) rather than
//                   from the float32 coordinates: a double-precision division per entry and lane would otherwise sit in the inner loop.
//                   The Chebyshev recurrence s1 (y - c q) - s2 q_prev is fused into the store: a filter step is one launch.
// k_enm_rigid<DIM>  R: three translations and three rotations about the centroid, orthonormalised in double (modified Gram-Schmidt,
//                   twice), null directions dropped; the constant vector for the GNM
// k_enm_rtz / k_enm_rtz_reduce / k_enm_sub   Z -= R (R^T Z), the partial sums added in a fixed order
// The solver is Chebyshev-filtered subspace iteration (Zhou & Saad 2007) on 64 vectors over the Rayleigh-Ritz machinery of pesto_ritz.h
// (the Jacobi, the Gram orthonormalisation with its Newton-Schulz step and the thin QTY product are pca's own, one text). Every sum
// runs in an order fixed by the shapes and the list alone (no float atomics), so every output repeats its bits.
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_cellgrid.h"
#include "pesto_geom.h"
#include "pesto_ritz.h"

namespace pesto {
namespace {

constexpr int NW = NT / 64;             // waves of a workgroup
constexpr int PCH = 256;                // rows of the block of vectors per workgroup of k_enm_rtz
constexpr int RC = 6;                   // columns of R at most
constexpr double FLOPPY = 1e-10;        // a Ritz value at or below FLOPPY b is a floppy direction: eigenvalue 0 (a definition)
constexpr double NULL_DIR = 1e-10;      // k_enm_rigid: a rigid motion whose norm falls below NULL_DIR of its own after the projection is dropped
constexpr double GAIN = 1e3;            // the filter's gain on the k-th mode against the damped interval
constexpr int MAX_DEGREE = 4096;        // of one filter (measured: 512 leaves a 10,000-node coil unconverged after 32 iterations, 2048 takes 18
                                        // iterations and 29,339 applications, 4096 takes 11 and 27,284; shorter filters are not affected)

enum { ERR_SEL = 1, ERR_FINITE = 2, ERR_NODE = 4 };

struct EnmInfo {
    double bound;               // b
    int32_t rrank, live;        // rank of R; the non-zero columns of the block
    int32_t n_zero, pad;        // floppy directions among the k
};

// what the host reads after every Rayleigh-Ritz step
struct EnmIter {
    DynState st;                // done, iterations, converged, sweeps (pesto_ritz.h)
    EnmInfo info;
    double theta[TS];           // the live Ritz values, ascending
    int32_t perm[TS];           // their columns
};

// ---- the list
// node i of the selection: its coordinates to Xs; the verdict: an index outside [0, N), a non-finite coordinate (both replaced by
// something harmless, the call is refused before anything else reads them)
__global__ __launch_bounds__(NT) void k_enm_gather(int N, int n, const float* __restrict__ xyz, const int* __restrict__ sel, float* __restrict__ Xs,
                                                   ListState* __restrict__ st) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    int a = sel ? sel[i] : i, bits = 0;
    if (a < 0 || a >= N) { bits |= ERR_SEL; a = 0; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = xyz[3 * (size_t)a + c];
        if (!isfinite(v)) { bits |= ERR_FINITE; v = 0.f; }
        Xs[3 * (size_t)i + c] = v;
    }
    if (bits) atomicOr(&st->err, bits);
}

// one thread per node in cell order. Node i's springs are the nodes j != i with fl32(sqrt_rn(dist2)) * scale < cutoff, decided on the
// squared distance against s_star (contact_threshold of pesto_geom.h), and dist2 > 0. FILL false: cnt[i] = their number. FILL true: they
// go to the row off[i] .. off[i + 1] in the order met.
template <bool FILL>
__global__ __launch_bounds__(NT) void k_enm_list(int n, const CellGrid* __restrict__ grids, const int* __restrict__ cell_start,
                                                 const float4* __restrict__ sorted, float s_star, int* __restrict__ cnt,
                                                 const long long* __restrict__ off, int* __restrict__ jt) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= n) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    const long long base = FILL ? off[i] : 0;
    int c = 0;
    for_each_neighbour(grids[0], cell_start, 0, a, [&](int q) {
        if (q == p) return;
        const float4 b = sorted[q];
        const float s2 = dist2(a.x, a.y, a.z, b.x, b.y, b.z);
        if (s2 < s_star && s2 > 0.f) {
            if (FILL) jt[base + c] = __float_as_int(b.w);
            ++c;
        }
    });
    if (!FILL) cnt[i] = c;
}

// one wave per row: the entries to their rank by j (a row holds every j once), with k = gamma |r|^-p, r = scale ((double)x_j - (double)x_i),
// and for the ANM (r, k / |r|^2). r_ji = -r_ij exactly, so k and k / |r|^2 are the same bits on both sides of a spring.
template <int DIM>
__global__ __launch_bounds__(NT) void k_enm_sort(int n, const float* __restrict__ Xs, double scale, double gamma, int p, const long long* __restrict__ off,
                                                 const int* __restrict__ jt, int* __restrict__ jn, double* __restrict__ kk, double4* __restrict__ geo) {
    const int i = blockIdx.x * NW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const long long e0 = off[i], e1 = off[i + 1];
    const double xi = Xs[3 * (size_t)i], yi = Xs[3 * (size_t)i + 1], zi = Xs[3 * (size_t)i + 2];
    for (long long e = e0 + lane; e < e1; e += 64) {
        const int j = jt[e];
        long long rank = 0;
        for (long long f = e0; f < e1; ++f) rank += jt[f] < j;
        const double rx = scale * ((double)Xs[3 * (size_t)j] - xi), ry = scale * ((double)Xs[3 * (size_t)j + 1] - yi),
                     rz = scale * ((double)Xs[3 * (size_t)j + 2] - zi);
        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(rx, rx), __dmul_rn(ry, ry)), __dmul_rn(rz, rz));
        const double k = p == 2 ? gamma / r2 : gamma;
        jn[e0 + rank] = j;
        kk[e0 + rank] = k;
        if (DIM == 3) geo[e0 + rank] = make_double4(rx, ry, rz, k / r2);
    }
}

// rowsum[i] = sum_j k_ij in ascending j
__global__ __launch_bounds__(NT) void k_enm_rowsum(int n, const long long* __restrict__ off, const double* __restrict__ kk, double* __restrict__ rowsum) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (long long e = off[i]; e < off[i + 1]; ++e) s += kk[e];
    rowsum[i] = s;
}

// one workgroup: b = 2 max_i rowsum[i]
__global__ __launch_bounds__(NT) void k_enm_bound(int n, const double* __restrict__ rowsum, EnmInfo* __restrict__ info) {
    __shared__ double mx[NT];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) v = fmax(v, rowsum[i]);
    mx[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) mx[threadIdx.x] = fmax(mx[threadIdx.x], mx[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) info->bound = 2.0 * mx[0];
}

// ---- the dense matrices: one wave per row of nodes. ANM: H_ij[a][b] = -(k / |r|^2) (r_a r_b), H_ii = sum_j (k / |r|^2) (r_a r_b) in
// ascending j; GNM: -k_ij and the row sum. The products commute and the two sides of a spring hold the same bits, so the matrix is
// bitwise symmetric as it is written (out is cleared before).
template <int DIM>
__global__ __launch_bounds__(NT) void k_enm_dense(int n, const long long* __restrict__ off, const int* __restrict__ jn, const double* __restrict__ kk,
                                                  const double4* __restrict__ geo, double* __restrict__ out) {
    const int i = blockIdx.x * NW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const long long e0 = off[i], e1 = off[i + 1];
    const size_t M = (size_t)DIM * n;
    for (long long e = e0 + lane; e < e1; e += 64) {
        const size_t j = (size_t)jn[e];
        if constexpr (DIM == 1) {
            out[(size_t)i * M + j] = -kk[e];
        } else {
            const double4 g = geo[e];
            const double r[3] = {g.x, g.y, g.z};
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) out[(3 * (size_t)i + a) * M + 3 * j + b] = -(g.w * (r[a] * r[b]));
        }
    }
    if (lane < DIM * DIM) {
        const int a = lane / DIM, b = lane % DIM;
        double s = 0.0;
        for (long long e = e0; e < e1; ++e) {
            if constexpr (DIM == 1) {
                s += kk[e];
            } else {
                const double4 g = geo[e];
                const double ra = a == 0 ? g.x : a == 1 ? g.y : g.z, rb = b == 0 ? g.x : b == 1 ? g.y : g.z;
                s += g.w * (ra * rb);
            }
        }
        out[(DIM * (size_t)i + a) * M + DIM * (size_t)i + b] = s;
    }
}

// ---- the operator
// out_i = s1 (y_i - cc q_i) - s2 prev_i with y_i = sum_j k_ij u_ij (u_ij . (q_i - q_j)) (ANM) or sum_j k_ij (q_i - q_j) (GNM), for the
// 64 columns of the block. prev may be NULL (s2 unused) and may be out itself (a thread reads its own element before it writes it); Q is
// read at the neighbours and must be another buffer.
template <int DIM>
__global__ __launch_bounds__(NT) void k_enm_apply(int n, const long long* __restrict__ off, const int* __restrict__ jn, const double* __restrict__ kk,
                                                  const double4* __restrict__ geo, const double* __restrict__ Q, const double* prev, double* out, double s1,
                                                  double cc, double s2) {
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * NW + (threadIdx.x >> 6)), c = threadIdx.x & 63;
    if (i >= n) return;
    const size_t at = (size_t)i * DIM * TS + c;
    double q[DIM], y[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) { q[a] = Q[at + a * TS]; y[a] = 0.0; }
    const long long e1 = off[i + 1];
#pragma unroll 4
    for (long long e = off[i]; e < e1; ++e) {
        const double* qj = Q + (size_t)jn[e] * DIM * TS + c;
        if constexpr (DIM == 3) {
            const double4 g = geo[e];
            const double d0 = q[0] - qj[0], d1 = q[1] - qj[TS], d2 = q[2] - qj[2 * TS];
            const double t = g.w * ((g.x * d0 + g.y * d1) + g.z * d2);
            y[0] += g.x * t; y[1] += g.y * t; y[2] += g.z * t;
        } else {
            y[0] += kk[e] * (q[0] - qj[0]);
        }
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        double v = s1 * (y[a] - cc * q[a]);
        if (prev) v -= s2 * prev[at + a * TS];
        out[at + a * TS] = v;
    }
}

// ---- the rigid motions
// One workgroup; R column-major [nc][m], nc = 6 (ANM) or 1 (GNM). A thread owns the nodes tid, tid + NT, ... in every phase. Column c is
// projected twice on the columns before it and normalised; one whose norm falls below NULL_DIR of what it was (the rotation about the
// line of a collinear network, every rotation of coincident nodes) becomes a zero column. info->rrank: the columns kept.
template <int DIM>
__global__ __launch_bounds__(NT) void k_enm_rigid(int n, const float* __restrict__ Xs, double scale, double* __restrict__ R, EnmInfo* __restrict__ info) {
    __shared__ double red[NW];
    const size_t m = (size_t)DIM * n;
    if (DIM == 1) {
        const double v = 1.0 / sqrt((double)n);
        for (int i = threadIdx.x; i < n; i += NT) R[i] = v;
        if (threadIdx.x == 0) info->rrank = 1;
        return;
    }
    double cen[3];
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < n; i += NT) s += scale * (double)Xs[3 * (size_t)i + c];
        cen[c] = block_sum<NT>(s, red) / (double)n;
    }
    for (int i = threadIdx.x; i < n; i += NT) {
        const double x = scale * (double)Xs[3 * (size_t)i] - cen[0], y = scale * (double)Xs[3 * (size_t)i + 1] - cen[1],
                     z = scale * (double)Xs[3 * (size_t)i + 2] - cen[2];
        double* r = R + 3 * (size_t)i;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) r[a * m + c] = a == c ? 1.0 : 0.0;
        r[3 * m] = 0.0; r[3 * m + 1] = -z; r[3 * m + 2] = y;             // e_x x r
        r[4 * m] = z; r[4 * m + 1] = 0.0; r[4 * m + 2] = -x;             // e_y x r
        r[5 * m] = -y; r[5 * m + 1] = x; r[5 * m + 2] = 0.0;             // e_z x r
    }
    int rank = 0;
    for (int c = 0; c < RC; ++c) {
        double* v = R + c * m;
        auto dot = [&](const double* w) {
            double s = 0.0;
            for (int i = threadIdx.x; i < n; i += NT)
                for (int a = 0; a < 3; ++a) s += w[3 * (size_t)i + a] * v[3 * (size_t)i + a];
            return block_sum<NT>(s, red);
        };
        const double n0 = dot(v);
        for (int pass = 0; pass < 2; ++pass)
            for (int p = 0; p < c; ++p) {
                const double* w = R + p * m;
                const double d = dot(w);
                for (int i = threadIdx.x; i < n; i += NT)
                    for (int a = 0; a < 3; ++a) v[3 * (size_t)i + a] -= d * w[3 * (size_t)i + a];
            }
        const double n1 = dot(v);
        const bool keep = n0 > 0.0 && n1 > NULL_DIR * NULL_DIR * n0;
        const double f = keep ? 1.0 / sqrt(n1) : 0.0;
        for (int i = threadIdx.x; i < n; i += NT)
            for (int a = 0; a < 3; ++a) v[3 * (size_t)i + a] = keep ? v[3 * (size_t)i + a] * f : 0.0;
        rank += keep;
    }
    if (threadIdx.x == 0) info->rrank = rank;
}

// partial[chunk][j][c] = sum over the chunk's rows r of R[j][r] Z[r][c]: thread (c, g) adds the rows g, g + 4, ..., the four in order
__global__ __launch_bounds__(NT) void k_enm_rtz(int m, int nc, const double* __restrict__ R, const double* __restrict__ Z, double* __restrict__ partial) {
    __shared__ double part[NW][RC][TS];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    double acc[RC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int r1 = min(m, (int)(blockIdx.x + 1) * PCH);
    for (int r = blockIdx.x * PCH + g; r < r1; r += NW) {
        const double z = Z[(size_t)r * TS + c];
#pragma unroll
        for (int j = 0; j < RC; ++j)
            if (j < nc) acc[j] += R[(size_t)j * m + r] * z;
    }
#pragma unroll
    for (int j = 0; j < RC; ++j) part[g][j][c] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < RC * TS; e += NT) {
        const int j = e >> 6, cc = e & 63;
        partial[(size_t)blockIdx.x * RC * TS + e] = ((part[0][j][cc] + part[1][j][cc]) + part[2][j][cc]) + part[3][j][cc];
    }
}

// C[j][c] = sum over the chunks, in order
__global__ __launch_bounds__(NT) void k_enm_rtz_reduce(int chunks, const double* __restrict__ partial, double* __restrict__ C) {
    for (int e = threadIdx.x; e < RC * TS; e += NT) {
        double s = 0.0;
        for (int q = 0; q < chunks; ++q) s += partial[(size_t)q * RC * TS + e];
        C[e] = s;
    }
}

// Z[r][c] -= sum_j R[j][r] C[j][c]
__global__ __launch_bounds__(NT) void k_enm_sub(int m, int nc, const double* __restrict__ R, const double* __restrict__ C, double* __restrict__ Z) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= (size_t)m * TS) return;
    const size_t r = e >> 6;
    const int c = (int)(e & 63);
    double s = 0.0;
    for (int j = 0; j < nc; ++j) s += R[(size_t)j * m + r] * C[j * TS + c];
    Z[e] -= s;
}

// ---- the solver's own small kernels
// One workgroup of 64 threads after a Rayleigh-Ritz step (theta descending, as k_dyn_jacobi leaves it; res2 / nrm2: the partial square
// sums of the residual columns and of the columns of X). A column of X is live when it is not a zero column (a block wider than the
// complement of R has some). The live Ritz values ascending (among equal ones the higher column first) give the modes; the k lowest
// decide: floppy directions, the residuals kept for the result, converged = max residual <= tol b.
__global__ __launch_bounds__(TS) void k_enm_check(int k, int nparts, double tol, const double* __restrict__ theta, const double* __restrict__ res2,
                                                  const double* __restrict__ nrm2, double* __restrict__ eig_keep, double* __restrict__ resid_keep,
                                                  EnmIter* __restrict__ it) {
    __shared__ double th[TS], res[TS];
    __shared__ int live[TS], perm[TS];
    const int c = threadIdx.x;
    double s = 0.0, w = 0.0;
    for (int q = 0; q < nparts; ++q) { s += res2[(size_t)q * TS + c]; w += nrm2[(size_t)q * TS + c]; }
    th[c] = theta[c]; res[c] = sqrt(s); live[c] = w > 0.25;
    perm[c] = -1;
    __syncthreads();
    int rank = 0, nlive = 0;
    for (int o = 0; o < TS; ++o) {
        nlive += live[o];
        rank += live[o] && (th[o] < th[c] || (th[o] == th[c] && o > c));
    }
    if (live[c]) perm[rank] = c;
    __syncthreads();
    const double b = it->info.bound;
    it->theta[c] = c < nlive ? th[perm[c]] : 0.0;
    it->perm[c] = perm[c];
    if (c == 0) {
        double worst = 0.0;
        int n_zero = 0;
        for (int i = 0; i < min(k, nlive); ++i) {
            const int col = perm[i];
            const bool floppy = th[col] <= FLOPPY * b;
            worst = fmax(worst, res[col]);
            n_zero += floppy;
            eig_keep[i] = floppy ? 0.0 : th[col];
            resid_keep[i] = res[col];
        }
        const int conv = nlive >= k && worst <= tol * b;
        it->st.iterations += 1; it->st.converged = conv;
        if (conv) it->st.done = 1;
        it->info.live = nlive; it->info.n_zero = n_zero;
    }
}

// Workgroup i: mode i of the result, column perm[i] of X. Sign rule: the entry of largest magnitude positive, the lowest index on ties.
__global__ __launch_bounds__(NT) void k_enm_modes(int m, const double* __restrict__ X, const EnmIter* __restrict__ it, const double* __restrict__ eig_keep,
                                                  const double* __restrict__ resid_keep, double* __restrict__ eig_out, double* __restrict__ modes_out,
                                                  double* __restrict__ resid_out) {
    __shared__ double bv[NT];
    __shared__ int bi[NT];
    const int i = blockIdx.x, c = it->perm[i];
    double best = -1.0;
    int at = 0x7fffffff;
    for (int r = threadIdx.x; r < m; r += NT) {
        const double v = fabs(X[(size_t)r * TS + c]);
        if (v > best) { best = v; at = r; }
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double ov = bv[threadIdx.x + o];
            const int oi = bi[threadIdx.x + o];
            if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = ov; bi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    const double sign = bi[0] < m && X[(size_t)bi[0] * TS + c] < 0.0 ? -1.0 : 1.0;
    for (int r = threadIdx.x; r < m; r += NT) modes_out[(size_t)i * m + r] = sign * X[(size_t)r * TS + c];
    if (threadIdx.x == 0) { eig_out[i] = eig_keep[i]; resid_out[i] = resid_keep[i]; }
}

// ---- what is derived from modes (modes [k][n][DIM], eig [k])
// out[i] = factor sum_k |v_k,i|^2 / eig_k over eig_k > 0, ascending k
__global__ __launch_bounds__(NT) void k_enm_fluct(int k, int n, int dim, double factor, const double* __restrict__ eig, const double* __restrict__ modes,
                                                  double* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int q = 0; q < k; ++q) {
        if (!(eig[q] > 0.0)) continue;
        const double* v = modes + ((size_t)q * n + i) * dim;
        double w = 0.0;
        for (int a = 0; a < dim; ++a) w += v[a] * v[a];
        s += w / eig[q];
    }
    out[i] = factor * s;
}

// out[i][j] = C_ij / sqrt(C_ii C_jj), C_ij = sum_k (v_k,i . v_k,j) / eig_k over eig_k > 0; 1 on the diagonal, 0 for a node without
// fluctuation. The same expression on both sides of the diagonal: bitwise symmetric.
__global__ __launch_bounds__(NT) void k_enm_corr(int k, int n, int dim, const double* __restrict__ eig, const double* __restrict__ modes,
                                                 float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= (size_t)n * n) return;
    const size_t i = e / n, j = e - i * n;
    double cij = 0.0, cii = 0.0, cjj = 0.0;
    for (int q = 0; q < k; ++q) {
        if (!(eig[q] > 0.0)) continue;
        const double* vi = modes + ((size_t)q * n + i) * dim;
        const double* vj = modes + ((size_t)q * n + j) * dim;
        double wij = 0.0, wii = 0.0, wjj = 0.0;
        for (int a = 0; a < dim; ++a) { wij += vi[a] * vj[a]; wii += vi[a] * vi[a]; wjj += vj[a] * vj[a]; }
        cij += wij / eig[q]; cii += wii / eig[q]; cjj += wjj / eig[q];
    }
    out[e] = i == j ? 1.f : cii > 0.0 && cjj > 0.0 ? (float)(cij / sqrt(cii * cjj)) : 0.f;
}

// workgroup (a, b): out[a][b] = |A_a . B_b| (/ |B_b| with normalise; 0 for a zero B_b)
__global__ __launch_bounds__(NT) void k_enm_overlap(int m, int kb, int normalise, const double* __restrict__ A, const double* __restrict__ B,
                                                    double* __restrict__ out) {
    __shared__ double red[NW];
    const int a = blockIdx.x / kb, b = blockIdx.x % kb;
    const double* va = A + (size_t)a * m;
    const double* vb = B + (size_t)b * m;
    double s = 0.0, w = 0.0;
    for (int r = threadIdx.x; r < m; r += NT) { s += va[r] * vb[r]; w += vb[r] * vb[r]; }
    s = block_sum<NT>(s, red);
    w = block_sum<NT>(w, red);
    if (threadIdx.x == 0) out[blockIdx.x] = !normalise ? fabs(s) : w > 0.0 ? fabs(s) / sqrt(w) : 0.0;
}

__global__ __launch_bounds__(NT) void k_enm_nodes(int N, int n, const int* __restrict__ node, ListState* __restrict__ st) {
    const int a = blockIdx.x * NT + threadIdx.x;
    if (a < N && (node[a] < 0 || node[a] >= n)) atomicOr(&st->err, ERR_NODE);
}

// out[f][a][c] = fl32((double)x_a,c + sum_k A[f][k] v_k[node(a)][c]), ascending k, in double, rounded once
__global__ __launch_bounds__(NT) void k_enm_deform(long long F, int N, int n, int k, const float* __restrict__ xyz, const double* __restrict__ modes,
                                                   const double* __restrict__ amp, const int* __restrict__ node, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= (size_t)F * N * 3) return;
    const size_t f = e / ((size_t)N * 3), ac = e - f * (size_t)N * 3, a = ac / 3, c = ac - 3 * a;
    const size_t nd = node ? (size_t)node[a] : a;
    double s = 0.0;
    for (int q = 0; q < k; ++q) s += amp[f * k + q] * modes[((size_t)q * n + nd) * 3 + c];
    out[e] = (float)((double)xyz[ac] + s);
}

// ---- host side
// the network of a call: its items in the call's block, and the list itself (allocated once the count pass has given K)
struct Net {
    int32_t offs[2];            // the grid's one structure
    int iOffs, iXs, iSt, iOff, iRow, iG, iCnt, iCur, iCell, iSort, iSum, iIt;
    long long K = 0;
    char* list = nullptr;
    double4* geo = nullptr; double* kk = nullptr; int* jn = nullptr; int* jt = nullptr;
};

void net_declare(Buffers& bf, Net& nt, size_t n) {
    nt.offs[0] = 0; nt.offs[1] = (int32_t)n;
    nt.iOffs = bf.table(nt.offs, 8);
    nt.iXs = bf.scratch(n * 12);
    nt.iSt = bf.scratch(sizeof(ListState), 0);
    nt.iOff = bf.scratch((n + 1) * 8);
    nt.iRow = bf.scratch(n * 4);
    const size_t cells = cells_before(n, 1);
    nt.iG = bf.scratch(sizeof(CellGrid));
    nt.iCnt = bf.scratch(cells * 4);
    nt.iCur = bf.scratch(cells * 4);
    nt.iCell = bf.scratch(n * 4);
    nt.iSort = bf.scratch(n * 16);
    nt.iSum = bf.scratch(n * 8);
    nt.iIt = bf.scratch(sizeof(EnmIter), 0);
}

int check_network(int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p, int32_t dim,
                  int64_t least) {
    if (!xyz) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (dim != 1 && dim != 3) return fail(PESTO_ERR_INVALID, "dim must be 3 (ANM) or 1 (GNM)");
    if (N < 1 || N > PESTO_ENM_MAX_NODES || n_sel < least || n_sel > N || (!sel && n_sel != N))
        return fail(PESTO_ERR_INVALID, "%lld <= n_sel <= N <= 2^24 nodes (n_sel = N without a selection)", (long long)least);
    const float fc = (float)cutoff, fs = (float)scale;
    if (!std::isfinite(cutoff) || !std::isfinite(scale) || !std::isfinite(fc) || !std::isfinite(fs) || !(fc > 0.f) || !(fs > 0.f) ||
        !std::isfinite(fc / fs) || !(fc / fs > 0.f))
        return fail(PESTO_ERR_INVALID, "cutoff and scale must be positive and finite");
    if (!std::isfinite(gamma) || !(gamma > 0.0)) return fail(PESTO_ERR_INVALID, "gamma must be positive and finite");
    if (p != 0 && p != 2) return fail(PESTO_ERR_INVALID, "p must be 0 or 2");
    return 0;
}

// gather + verdict + list + stiffness + row sums + b. Nothing of the caller's has been written when this refuses.
int net_build(Buffers& bf, Net& nt, int N, int n, const float* xyz, const int* sel, double cutoff, double scale, double gamma, int p, int dim,
              const char* what) {
    const float fc = (float)cutoff, fs = (float)scale;
    const float s_star = contact_threshold(fc, fs, true);       // d < cutoff  <=>  dist2 < s_star
    const unsigned nb = blocks((size_t)n, NT), nwb = blocks((size_t)n, NW);
    float* Xs = bf.ptr<float>(nt.iXs);
    CellGrid* g = bf.ptr<CellGrid>(nt.iG);
    int* cell_cnt = bf.ptr<int>(nt.iCnt);
    const long long* off = bf.ptr<const long long>(nt.iOff);
    hipLaunchKernelGGL(k_enm_gather, dim3(nb), dim3(NT), 0, bf.stm, N, n, xyz, sel, Xs, bf.ptr<ListState>(nt.iSt));
    grid_build(bf.stm, n, 1, bf.ptr<const int>(nt.iOffs), (const float*)Xs, fc / fs,
               GridBufs{g, cell_cnt, bf.ptr<int>(nt.iCur), bf.ptr<int>(nt.iCell), bf.ptr<float4>(nt.iSort)}, NoCheck{}, NoPayload{});
    hipLaunchKernelGGL(k_enm_list<false>, dim3(nb), dim3(NT), 0, bf.stm, n, (const CellGrid*)g, (const int*)cell_cnt,
                       (const float4*)bf.ptr<float4>(nt.iSort), s_star, bf.ptr<int>(nt.iRow), (const long long*)nullptr, (int*)nullptr);
    list_offsets(bf, n, nt.iRow, nt.iOff, (long long)PESTO_ENM_MAX_SPRINGS, nt.iSt);
    ListState h{};
    if (int rc = bf.verdict(nt.iSt, &h, sizeof h, what)) return rc;
    if (h.err & ERR_SEL) return fail(PESTO_ERR_INVALID, "%s: sel must hold node indices in [0, N)", what);
    if (h.err & ERR_FINITE) return fail(PESTO_ERR_INVALID, "%s: a selected node has a non-finite coordinate", what);
    nt.K = h.K;
    if (h.K > PESTO_ENM_MAX_SPRINGS) return fail(PESTO_ERR_INVALID, "%s: %lld list entries, at most 2^27 per call", what, h.K);
    const size_t K = (size_t)h.K, bytes = K * (size_t)(dim == 3 ? 48 : 16);
    if (hipMallocAsync((void**)&nt.list, std::max<size_t>(bytes, 256), bf.stm) != hipSuccess) {
        nt.list = nullptr;
        return fail(PESTO_ERR_NOMEM, "%s: device allocation of %lld list entries failed", what, h.K);
    }
    char* at = nt.list;
    if (dim == 3) { nt.geo = (double4*)at; at += K * 32; }
    nt.kk = (double*)at; at += K * 8;
    nt.jn = (int*)at; at += K * 4;
    nt.jt = (int*)at;
    hipLaunchKernelGGL(k_enm_list<true>, dim3(nb), dim3(NT), 0, bf.stm, n, (const CellGrid*)g, (const int*)cell_cnt,
                       (const float4*)bf.ptr<float4>(nt.iSort), s_star, (int*)nullptr, off, nt.jt);
    if (dim == 3)
        hipLaunchKernelGGL(k_enm_sort<3>, dim3(nwb), dim3(NT), 0, bf.stm, n, (const float*)Xs, scale, gamma, p, off, (const int*)nt.jt, nt.jn, nt.kk, nt.geo);
    else
        hipLaunchKernelGGL(k_enm_sort<1>, dim3(nwb), dim3(NT), 0, bf.stm, n, (const float*)Xs, scale, gamma, p, off, (const int*)nt.jt, nt.jn, nt.kk, nt.geo);
    hipLaunchKernelGGL(k_enm_rowsum, dim3(nb), dim3(NT), 0, bf.stm, n, off, (const double*)nt.kk, bf.ptr<double>(nt.iSum));
    hipLaunchKernelGGL(k_enm_bound, dim3(1), dim3(NT), 0, bf.stm, n, (const double*)bf.ptr<double>(nt.iSum), &bf.ptr<EnmIter>(nt.iIt)->info);
    return 0;
}

int net_finish(Buffers& bf, Net& nt, int rc, const char* what) {
    if (nt.list) (void)hipFreeAsync(nt.list, bf.stm);
    return bf.finish(rc, what);
}

// `bytes` from device memory to an output of the caller's, on either side
int to_caller(Buffers& bf, void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    return hip_ok(hipMemcpyAsync(dst, src, bytes, bf.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, bf.stm), "copy to the caller failed");
}

template <int DIM>
void launch_apply(hipStream_t stm, int n, const long long* off, const Net& nt, const double* Q, const double* prev, double* out, double s1, double cc,
                  double s2) {
    hipLaunchKernelGGL(k_enm_apply<DIM>, dim3(blocks((size_t)n, NW)), dim3(NT), 0, stm, n, off, (const int*)nt.jn, (const double*)nt.kk,
                       (const double4*)nt.geo, Q, prev, out, s1, cc, s2);
}

void apply(hipStream_t stm, int dim, int n, const long long* off, const Net& nt, const double* Q, const double* prev, double* out, double s1, double cc,
           double s2) {
    dim == 3 ? launch_apply<3>(stm, n, off, nt, Q, prev, out, s1, cc, s2) : launch_apply<1>(stm, n, off, nt, Q, prev, out, s1, cc, s2);
}

// Z -= R (R^T Z)
void project(hipStream_t stm, int m, int nc, const double* R, double* Z, double* partial, double* C) {
    const int chunks = (m + PCH - 1) / PCH;
    hipLaunchKernelGGL(k_enm_rtz, dim3(chunks), dim3(NT), 0, stm, m, nc, R, (const double*)Z, partial);
    hipLaunchKernelGGL(k_enm_rtz_reduce, dim3(1), dim3(NT), 0, stm, chunks, (const double*)partial, C);
    hipLaunchKernelGGL(k_enm_sub, dim3(blocks((size_t)m * TS, NT)), dim3(NT), 0, stm, m, nc, R, (const double*)C, Z);
}

// the modes given to the derived entry points: k rows of n nodes of dim values
int check_modes(int64_t k, int64_t n, int32_t dim, int64_t kmax) {
    if (dim != 1 && dim != 3) return fail(PESTO_ERR_INVALID, "dim must be 3 (ANM) or 1 (GNM)");
    if (k < 1 || k > kmax) return fail(PESTO_ERR_INVALID, "1 to %lld modes, got %lld", (long long)kmax, (long long)k);
    if (n < 1 || n > PESTO_ENM_MAX_NODES) return fail(PESTO_ERR_INVALID, "1 to 2^24 nodes, got %lld", (long long)n);
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_enm_last_error(void) { return last_error(); }

int pesto_enm_network(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                      int64_t capacity, int64_t* offsets_out, int32_t* j_out, double* k_out, int64_t* n_springs_out, double* bound_out, int32_t ptr_kind,
                      void* stream) {
    if (int rc = check_network(N, n_sel, xyz, sel, cutoff, scale, gamma, p, 1, 1)) return rc;
    if (!offsets_out || !n_springs_out || !bound_out || capacity < 0 || capacity > PESTO_ENM_MAX_SPRINGS || (capacity > 0 && (!j_out || !k_out)))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    Net nt;
    net_declare(bf, nt, (size_t)n_sel);
    int rc = bf.upload();
    if (rc == 0) rc = net_build(bf, nt, (int)N, (int)n_sel, bf.ptr<const float>(iX), sel ? bf.ptr<const int>(iS) : nullptr, cutoff, scale, gamma, p, 1, "network");
    EnmIter h{};
    if (rc == 0) rc = bf.verdict(nt.iIt, &h, sizeof h, "network");
    if (rc == 0) {
        *n_springs_out = nt.K;
        *bound_out = h.info.bound;
        rc = to_caller(bf, offsets_out, bf.ptr<const void>(nt.iOff), ((size_t)n_sel + 1) * 8);
        if (rc == 0 && nt.K <= capacity) {
            rc = to_caller(bf, j_out, nt.jn, (size_t)nt.K * 4);
            if (rc == 0) rc = to_caller(bf, k_out, nt.kk, (size_t)nt.K * 8);
        }
    }
    return net_finish(bf, nt, rc, "network");
}

int pesto_enm_matrix(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                     int32_t dim, double* out, int32_t ptr_kind, void* stream) {
    if (int rc = check_network(N, n_sel, xyz, sel, cutoff, scale, gamma, p, dim, 1)) return rc;
    if (!out) return fail(PESTO_ERR_INVALID, "bad arguments");
    const int64_t M = (int64_t)dim * n_sel;
    if (M * M > PESTO_ENM_MAX_DENSE) return fail(PESTO_ERR_INVALID, "(dim n_sel)^2 <= 2^27 entries, got n_sel = %lld", (long long)n_sel);
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iO = bf.output(out, (size_t)(M * M) * 8);
    Net nt;
    net_declare(bf, nt, (size_t)n_sel);
    int rc = bf.upload();
    if (rc == 0) rc = net_build(bf, nt, (int)N, (int)n_sel, bf.ptr<const float>(iX), sel ? bf.ptr<const int>(iS) : nullptr, cutoff, scale, gamma, p, dim, "matrix");
    if (rc == 0) rc = hip_ok(hipMemsetAsync(bf.ptr<void>(iO), 0, (size_t)(M * M) * 8, bf.stm), "matrix");
    if (rc == 0) {
        const long long* off = bf.ptr<const long long>(nt.iOff);
        const unsigned nwb = blocks((size_t)n_sel, NW);
        if (dim == 3)
            hipLaunchKernelGGL(k_enm_dense<3>, dim3(nwb), dim3(NT), 0, bf.stm, (int)n_sel, off, (const int*)nt.jn, (const double*)nt.kk, (const double4*)nt.geo,
                               bf.ptr<double>(iO));
        else
            hipLaunchKernelGGL(k_enm_dense<1>, dim3(nwb), dim3(NT), 0, bf.stm, (int)n_sel, off, (const int*)nt.jn, (const double*)nt.kk, (const double4*)nt.geo,
                               bf.ptr<double>(iO));
    }
    return net_finish(bf, nt, rc, "matrix");
}

int pesto_enm_modes(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                    int32_t dim, int32_t k, double tol, int32_t max_iter, double* eig_out, double* modes_out, double* resid_out, double* bound_out,
                    int64_t* n_springs_out, int32_t* info_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_network(N, n_sel, xyz, sel, cutoff, scale, gamma, p, dim, dim == 3 ? 3 : 2)) return rc;
    if (!eig_out || !modes_out || !resid_out || !bound_out || !n_springs_out || !info_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    const int64_t mm = (int64_t)dim * n_sel, room = dim == 3 ? mm - 6 : mm - 1;
    if (k < 1 || k > PESTO_ENM_MAX_MODES || k > room)
        return fail(PESTO_ERR_INVALID, "1 <= n_modes <= min(%d, %s), got %d", PESTO_ENM_MAX_MODES, dim == 3 ? "3 n_sel - 6" : "n_sel - 1", k);
    if (!(tol >= 0.0) || !std::isfinite(tol) || max_iter < 1) return fail(PESTO_ERR_INVALID, "tol must be finite and >= 0, max_iter >= 1");
    if (int rc = begin(m, ptr_kind)) return rc;
    const int n = (int)n_sel, nc = dim == 3 ? RC : 1;
    Shape s{};                  // the rows of the block of vectors, for the thin product of pesto_ritz.h
    s.F = 1; s.N = N; s.n = n_sel; s.m = mm; s.mp = (mm + TS - 1) / TS * TS; s.Fp = TS;
    s.qty = split_of(s.m, 1);
    const int chunks = (int)((mm + PCH - 1) / PCH), nparts = (int)(s.mp / TS) * 4;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iE = bf.output(eig_out, (size_t)k * 8), iMo = bf.output(modes_out, (size_t)k * mm * 8), iRo = bf.output(resid_out, (size_t)k * 8);
    Net nt;
    net_declare(bf, nt, (size_t)n_sel);
    const size_t vec = (size_t)s.mp * TS * 8;
    const int iQ = bf.scratch(vec), iY = bf.scratch(vec), iXv = bf.scratch(vec), iZ = bf.scratch(vec), iTmp = bf.scratch(vec);
    const int iR = bf.scratch((size_t)RC * mm * 8), iPp = bf.scratch((size_t)chunks * RC * TS * 8), iC = bf.scratch(RC * TS * 8);
    const int iPart = bf.scratch((size_t)s.qty.S * TS * TS * 8);
    const int iT = bf.scratch(TS * TS * 8), iV = bf.scratch(TS * TS * 8), iTh = bf.scratch(TS * 8), iSv = bf.scratch(TS * 8), iZero = bf.scratch(TS * 8, 0);
    const int iEk = bf.scratch(TS * 8, 0), iRk = bf.scratch(TS * 8, 0);
    const int iRp = bf.scratch((size_t)nparts * TS * 8), iRp2 = bf.scratch((size_t)nparts * TS * 8);
    int rc = bf.upload();
    if (rc == 0) rc = net_build(bf, nt, (int)N, n, bf.ptr<const float>(iX), sel ? bf.ptr<const int>(iS) : nullptr, cutoff, scale, gamma, p, dim, "modes");
    if (rc == 0) rc = hip_ok(hipFuncSetAttribute((const void*)k_dyn_jacobi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JACOBI_LDS), "modes");
    EnmIter h{};
    int applies = 0;
    if (rc == 0) {
        hipStream_t stm = bf.stm;
        EnmIter* it = bf.ptr<EnmIter>(nt.iIt);
        DynState* st = &it->st;
        const long long* off = bf.ptr<const long long>(nt.iOff);
        double *Q = bf.ptr<double>(iQ), *Y = bf.ptr<double>(iY), *X = bf.ptr<double>(iXv), *Z = bf.ptr<double>(iZ), *Tmp = bf.ptr<double>(iTmp);
        double *R = bf.ptr<double>(iR), *pp = bf.ptr<double>(iPp), *C = bf.ptr<double>(iC), *part = bf.ptr<double>(iPart);
        double *T = bf.ptr<double>(iT), *V = bf.ptr<double>(iV), *th = bf.ptr<double>(iTh), *sv = bf.ptr<double>(iSv);
        const unsigned gv = blocks((size_t)mm * TS, NT), gr = (unsigned)((mm + 15) / 16);
        const Mma a = mma_of(s, nullptr, nullptr, st);
        if (dim == 3) hipLaunchKernelGGL(k_enm_rigid<3>, dim3(1), dim3(NT), 0, stm, n, (const float*)bf.ptr<float>(nt.iXs), scale, R, &it->info);
        else hipLaunchKernelGGL(k_enm_rigid<1>, dim3(1), dim3(NT), 0, stm, n, (const float*)bf.ptr<float>(nt.iXs), scale, R, &it->info);
        hipLaunchKernelGGL(k_dyn_start, dim3(gv), dim3(NT), 0, stm, (int)mm, Z);
        project(stm, (int)mm, nc, R, Z, pp, C);
        launch_ortho(stm, s, a, Z, Tmp, Q, part, T, V, sv);
        for (int iter = 0; rc == 0 && iter < max_iter; ++iter) {
            // Rayleigh-Ritz: Y = P H Q, T = Q^T Y, X = Q V, Z = Y V, the residual columns Z - X Theta
            apply(stm, dim, n, off, nt, Q, nullptr, Y, 1.0, 0.0, 0.0);
            ++applies;
            project(stm, (int)mm, nc, R, Y, pp, C);
            launch_qty(stm, s, a, Q, Y, part, T);
            hipLaunchKernelGGL(k_dyn_jacobi, dim3(1), dim3(NT), JACOBI_LDS, stm, (const double*)T, 0, V, th, st);
            hipLaunchKernelGGL(k_dyn_rotate, dim3(gr), dim3(NT), 0, stm, (int)mm, (const double*)Q, (const double*)V, (const double*)nullptr, X, st);
            hipLaunchKernelGGL(k_dyn_rotate, dim3(gr), dim3(NT), 0, stm, (int)mm, (const double*)Y, (const double*)V, (const double*)nullptr, Z, st);
            hipLaunchKernelGGL(k_dyn_resid, dim3((unsigned)(s.mp / TS)), dim3(NT), 0, stm, (int)mm, (const double*)X, (const double*)Z, (const double*)th,
                               bf.ptr<double>(iRp), st);
            // (the same kernel with theta = 0: the square sums of X's columns, which tell a zero column from a mode)
            hipLaunchKernelGGL(k_dyn_resid, dim3((unsigned)(s.mp / TS)), dim3(NT), 0, stm, (int)mm, (const double*)Z, (const double*)X,
                               bf.ptr<const double>(iZero), bf.ptr<double>(iRp2), st);
            hipLaunchKernelGGL(k_enm_check, dim3(1), dim3(TS), 0, stm, (int)k, nparts, tol, (const double*)th, bf.ptr<const double>(iRp),
                               bf.ptr<const double>(iRp2), bf.ptr<double>(iEk), bf.ptr<double>(iRk), it);
            rc = bf.verdict(nt.iIt, &h, sizeof h, "modes");
            if (rc != 0) break;
            if (h.info.live < k) { rc = fail(PESTO_ERR_INVALID, "modes: the block kept %d of the %d directions asked for", h.info.live, k); break; }
            if (h.st.done || iter + 1 == max_iter) break;
            if (h.info.live >= mm - h.info.rrank) break;        // the block spans the whole complement of R: this Rayleigh-Ritz was exact
            // the scaled Chebyshev filter (Zhou & Saad 2007) that damps [cut, b] against the lowest Ritz value, on the Ritz vectors X
            const double b = h.info.bound, lo = std::max(h.theta[0], 0.0);
            double cut = h.theta[h.info.live - 1];
            if (!(cut < b) || !(cut > lo)) cut = 0.5 * (b + lo);
            const double e = 0.5 * (b - cut), c = 0.5 * (b + cut);
            const double xk = (c - std::min(std::max(h.theta[k - 1], 0.0), cut)) / e;
            int degree = MAX_DEGREE;
            if (xk > 1.0) degree = (int)std::min<double>(MAX_DEGREE, std::ceil(std::acosh(GAIN) / std::acosh(xk)));
            degree = std::max(degree, 2);
            double sigma = e / (lo - c);
            const double tau = 2.0 / sigma;
            double *cur = X, *other = Z;
            apply(stm, dim, n, off, nt, cur, nullptr, other, sigma / e, c, 0.0);
            std::swap(cur, other);                              // cur: the newest, other: the one before
            for (int d = 2; d <= degree; ++d) {
                const double sn = 1.0 / (tau - sigma);
                apply(stm, dim, n, off, nt, cur, other, other, 2.0 * sn / e, c, sigma * sn);
                std::swap(cur, other);
                sigma = sn;
            }
            applies += degree;
            project(stm, (int)mm, nc, R, cur, pp, C);
            launch_ortho(stm, s, a, cur, Tmp, Q, part, T, V, sv);
        }
        if (rc == 0) {
            // the Ritz vectors are sums of 64 rounded products of vectors in the complement: what that left along R goes now
            project(stm, (int)mm, nc, R, X, pp, C);
            hipLaunchKernelGGL(k_enm_modes, dim3((unsigned)k), dim3(NT), 0, stm, (int)mm, (const double*)X, (const EnmIter*)it, bf.ptr<const double>(iEk),
                               bf.ptr<const double>(iRk), bf.ptr<double>(iE), bf.ptr<double>(iMo), bf.ptr<double>(iRo));
        }
    }
    if (rc == 0) {
        *bound_out = h.info.bound;
        *n_springs_out = nt.K;
        info_out[0] = h.info.n_zero; info_out[1] = h.st.iterations; info_out[2] = h.st.converged; info_out[3] = applies; info_out[4] = h.st.sweeps;
        info_out[5] = h.info.rrank;
    }
    return net_finish(bf, nt, rc, "modes");
}

int pesto_enm_fluctuations(pesto_model* m, int64_t k, int64_t n, int32_t dim, const double* eig, const double* modes, double factor, double* fluct_out,
                           float* corr_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_modes(k, n, dim, 64)) return rc;
    if (!eig || !modes || (!fluct_out && !corr_out) || !std::isfinite(factor)) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (corr_out && n * n > PESTO_ENM_MAX_DENSE) return fail(PESTO_ERR_INVALID, "n^2 <= 2^27 entries, got n = %lld", (long long)n);
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iE = bf.input(eig, (size_t)k * 8), iM = bf.input(modes, (size_t)(k * n * dim) * 8);
    const int iF = bf.output(fluct_out, (size_t)n * 8), iC = bf.output(corr_out, (size_t)(n * n) * 4);
    int rc = bf.upload();
    if (rc == 0 && fluct_out)
        hipLaunchKernelGGL(k_enm_fluct, dim3(blocks((size_t)n, NT)), dim3(NT), 0, bf.stm, (int)k, (int)n, dim, factor, bf.ptr<const double>(iE),
                           bf.ptr<const double>(iM), bf.ptr<double>(iF));
    if (rc == 0 && corr_out)
        hipLaunchKernelGGL(k_enm_corr, dim3(blocks((size_t)(n * n), NT)), dim3(NT), 0, bf.stm, (int)k, (int)n, dim, bf.ptr<const double>(iE),
                           bf.ptr<const double>(iM), bf.ptr<float>(iC));
    return bf.finish(rc, "fluctuations");
}

int pesto_enm_overlap(pesto_model* m, int64_t ka, int64_t kb, int64_t len, const double* modes_a, const double* modes_b, int32_t normalise_b,
                      double* overlap_out, int32_t ptr_kind, void* stream) {
    if (ka < 1 || ka > 64 || kb < 1 || kb > 64 || len < 1 || len > 3 * (int64_t)PESTO_ENM_MAX_NODES)
        return fail(PESTO_ERR_INVALID, "1 to 64 modes a side of 1 to 3 * 2^24 values");
    if (!modes_a || !modes_b || !overlap_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iA = bf.input(modes_a, (size_t)(ka * len) * 8), iB = bf.input(modes_b, (size_t)(kb * len) * 8);
    const int iO = bf.output(overlap_out, (size_t)(ka * kb) * 8);
    int rc = bf.upload();
    if (rc == 0)
        hipLaunchKernelGGL(k_enm_overlap, dim3((unsigned)(ka * kb)), dim3(NT), 0, bf.stm, (int)len, (int)kb, normalise_b, bf.ptr<const double>(iA),
                           bf.ptr<const double>(iB), bf.ptr<double>(iO));
    return bf.finish(rc, "overlap");
}

int pesto_enm_deform(pesto_model* m, int64_t F, int64_t N, int64_t n, int64_t k, const float* xyz, const double* modes, const double* amplitudes,
                     const int32_t* node_of_atom, float* xyz_out, int32_t ptr_kind, void* stream) {
    if (!xyz || !modes || !amplitudes || !xyz_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_ENM_MAX_NODES || N < 1 || N > PESTO_ENM_MAX_NODES || n < 1 || n > N || (!node_of_atom && n != N))
        return fail(PESTO_ERR_INVALID, "1 to 2^24 frames, 1 <= n <= N <= 2^24 (n = N without node_of_atom)");
    if (k < 1 || k > 64) return fail(PESTO_ERR_INVALID, "1 to 64 modes, got %lld", (long long)k);
    if ((uint64_t)F * (uint64_t)N * 3 > (1ull << 36)) return fail(PESTO_ERR_INVALID, "F * N * 3 <= 2^36 values a call");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)N * 12), iM = bf.input(modes, (size_t)(k * n * 3) * 8), iA = bf.input(amplitudes, (size_t)(F * k) * 8);
    const int iNd = bf.input(node_of_atom, (size_t)N * 4), iO = bf.output(xyz_out, (size_t)(F * N * 3) * 4), iSt = bf.scratch(sizeof(ListState), 0);
    int rc = bf.upload();
    if (rc == 0 && node_of_atom) {
        hipLaunchKernelGGL(k_enm_nodes, dim3(blocks((size_t)N, NT)), dim3(NT), 0, bf.stm, (int)N, (int)n, bf.ptr<const int>(iNd), bf.ptr<ListState>(iSt));
        ListState h{};
        rc = bf.verdict(iSt, &h, sizeof h, "deform");
        if (rc == 0 && h.err) rc = fail(PESTO_ERR_INVALID, "deform: node_of_atom must lie in [0, n)");
    }
    if (rc == 0)
        hipLaunchKernelGGL(k_enm_deform, dim3(blocks((size_t)(F * N * 3), NT)), dim3(NT), 0, bf.stm, (long long)F, (int)N, (int)n, (int)k,
                           bf.ptr<const float>(iX), bf.ptr<const double>(iM), bf.ptr<const double>(iA), node_of_atom ? bf.ptr<const int>(iNd) : nullptr,
                           bf.ptr<float>(iO));
    return bf.finish(rc, "deform");
}
