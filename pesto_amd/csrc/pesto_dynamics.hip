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
// The tile skeleton (k_dyn_mma<MODE> over mma64_loop<f64x4, false> of pesto_mma64.h), the Jacobi, the orthonormalisation and the residual
// kernel live in pesto_ritz.h, which pesto_enm.hip shares.
// The solver is block subspace iteration with Rayleigh-Ritz on 64 vectors, matrix-free (pca never forms C). Every sum runs in a fixed
// order that depends on the shapes alone, so every output is bit-identical from call to call.
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_geom.h"
#include "pesto_mma64.h"
#include "pesto_ritz.h"

namespace pesto {
namespace {

constexpr int MG = 16;          // k_dyn_mean: coordinates per workgroup, and frame groups
constexpr int ROUNDS = 4;       // solver iterations enqueued between two reads of the done flag
constexpr double RANK_TOL = 1e-12;   // a Ritz value at or below RANK_TOL x the largest is a null direction

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

// tr C = fac sum_j sq[j], and the state's start
__global__ __launch_bounds__(NT) void k_dyn_total(int m, double fac, const double* __restrict__ sq, DynState* __restrict__ st) {
    __shared__ double red[NT / 64];
    double s = 0.0;
    for (int j = threadIdx.x; j < m; j += NT) s += sq[j];
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) { st->total = s * fac; st->done = 0; st->iterations = 0; st->converged = 0; st->rank = 0; st->sweeps = 0; st->pad = 0; }
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
int check_frames(int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale) {
    if (!xyz) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DYNAMICS_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to 2^24 frames, got %lld", (long long)F);
    if (N < 1 || N > PESTO_DYNAMICS_MAX_ATOMS || n_sel < 1 || n_sel > N || (!sel && n_sel != N))
        return fail(PESTO_ERR_INVALID, "1 <= n_sel <= N <= 2^24 atoms (n_sel = N without a selection)");
    if (!std::isfinite(scale)) return fail(PESTO_ERR_INVALID, "scale must be finite");
    return 0;
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
