// pesto_geom.h - the geometry the analysis groups share (pesto_hbonds.hip, pesto_lddt.hip, pesto_cluster.hip, pesto_peaks.hip,
// pesto_dynamics.hip, pesto_poses.hip, and pesto_trajectory.hip, pesto_docking.hip and pesto_dockq.hip through pesto_fit.h): the float32 squared distance
// of NumPy and torch, the host's derivation of squared-distance thresholds from it, the workgroup sum in double and the rotation of a
// Kabsch superposition (kabsch_rotation: the one superposition fit, pesto_fit.h; kabsch_trace: pesto_cluster.hip; jacobi_angle). Also one
// edge of the model's geometry (r, |r|, the fix-up) for the backward of the geometry pass (pesto_train.hip).
//
// Everything sits in an anonymous namespace (one copy per translation unit, like pesto_call.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace pesto {

namespace {

// NumPy's float32 squared distance, no contraction: (dx*dx + dy*dy) + dz*dz
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the point p[0 .. 2] has three finite coordinates (neither NaN nor infinite)
__device__ __forceinline__ bool finite3(const float* p) {
    return fabsf(p[0]) <= 3.402823466e38f && fabsf(p[1]) <= 3.402823466e38f && fabsf(p[2]) <= 3.402823466e38f;
}


// One edge of the model's geometry (src/model_operations.py:8-14) in the float32 operations of the forward's geometry pass (k_unpack1 /
// k_unpack2, pesto_kernels.hip, whose text is pinned by the committed profile's source stamp): the same expressions with the same
// explicit FMAs, so the backward (pesto_train.hip) gets the forward's bits of D0 and makes the forward's fix-up decision.
// r = X_j - X_i, returns D0 = |r| (torch.norm's FMA chain)
__device__ __forceinline__ float edge_vec(const float* __restrict__ xj, const float* __restrict__ xi, float& rx, float& ry, float& rz) {
    rx = xj[0] - xi[0]; ry = xj[1] - xi[1]; rz = xj[2] - xi[2];
    return sqrtf(fmaf(rz, rz, fmaf(ry, ry, rx * rx)));
}
// the fix-up of :12: an edge shorter than 1e-2 gets the call's maximal distance added
__device__ __forceinline__ bool edge_fixup(float d0) { return d0 < 1e-2f; }
__device__ __forceinline__ float edge_dist(float d0, float dmax) { return d0 + dmax * (edge_fixup(d0) ? 1.0f : 0.0f); }


// sum of v over the workgroup, the same bits in every thread: butterfly within each wave, then the four waves in turn.
// NT threads; red: NT / 64 doubles of LDS; two barriers
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t += red[w];
    return t;
}


// c, s of the Jacobi rotation that makes two columns orthogonal (alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q != 0); also k_dyn_jacobi's
__device__ __forceinline__ void jacobi_angle(double alpha, double beta, double gamma, double& c, double& s) {
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    c = 1.0 / sqrt(1.0 + t * t); s = c * t;
}

// R of the 3x3 covariance H = (ref - t_ref)^T (xyz - t) = U S V^T: R = V diag(1, 1, det(U) det(V)) U^T, by one-sided Jacobi in double
// (columns of H V rotated until orthogonal: H V = U S). With U2' = U0 x U1 and the true U2 = +-U2', the sign cancels against det(U):
// R = V0 U0^T + V1 U1^T + det(V) V2 U2'^T, columns ordered by singular value, so the smallest one is never divided by.
__device__ void kabsch_rotation(const double* H, double* R) {
    double A[3][3], V[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { A[a][b] = H[3 * a + b]; V[a][b] = a == b ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < 3; ++k) { alpha += A[k][p] * A[k][p]; beta += A[k][q] * A[k][q]; gamma += A[k][p] * A[k][q]; }
                if (fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;     // orthogonal to a few units of double rounding (also gamma == 0)
                rotated = true;
                double c, s;
                jacobi_angle(alpha, beta, gamma, c, s);
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q], vp = V[k][p], vq = V[k][q];
                    A[k][p] = c * ap - s * aq; A[k][q] = s * ap + c * aq;
                    V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double n[3];
    for (int k = 0; k < 3; ++k) n[k] = sqrt(A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k]);
    int i0 = 0, i1 = 1, i2 = 2;
    if (n[i0] < n[i1]) { const int t = i0; i0 = i1; i1 = t; }
    if (n[i1] < n[i2]) { const int t = i1; i1 = i2; i2 = t; }
    if (n[i0] < n[i1]) { const int t = i0; i0 = i1; i1 = t; }
    // A degenerate selection leaves the rotation about its line (rank 1: collinear atoms) or altogether (rank 0) undetermined. Like an SVD
    // library, return SOME proper rotation then, never a division by zero: a missing left vector is any unit vector orthogonal to the ones
    // there are (the least-squares fit is the same for every such choice).
    double U0[3] = {1.0, 0.0, 0.0}, U1[3], U2[3];
    const double tiny = 1e-300;
    if (n[i0] > tiny)
        for (int k = 0; k < 3; ++k) U0[k] = A[k][i0] / n[i0];
    if (n[i1] > tiny && n[i1] > 1e-14 * n[i0]) {
        double dot = 0.0, len = 0.0;
        for (int k = 0; k < 3; ++k) { U1[k] = A[k][i1] / n[i1]; dot += U1[k] * U0[k]; }
        for (int k = 0; k < 3; ++k) { U1[k] -= dot * U0[k]; len += U1[k] * U1[k]; }        // (re-orthogonalised: a no-op away from degeneracy)
        len = sqrt(len);
        for (int k = 0; k < 3; ++k) U1[k] /= len;
    } else {
        const int c = fabs(U0[0]) <= fabs(U0[1]) && fabs(U0[0]) <= fabs(U0[2]) ? 0 : fabs(U0[1]) <= fabs(U0[2]) ? 1 : 2;    // the axis least along U0
        double e[3] = {0.0, 0.0, 0.0}, len = 0.0;
        e[c] = 1.0;
        for (int k = 0; k < 3; ++k) { U1[k] = e[k] - U0[c] * U0[k]; len += U1[k] * U1[k]; }
        len = sqrt(len);
        for (int k = 0; k < 3; ++k) U1[k] /= len;
    }
    U2[0] = U0[1] * U1[2] - U0[2] * U1[1];
    U2[1] = U0[2] * U1[0] - U0[0] * U1[2];
    U2[2] = U0[0] * U1[1] - U0[1] * U1[0];
    const double detV = V[0][i0] * (V[1][i1] * V[2][i2] - V[2][i1] * V[1][i2]) - V[0][i1] * (V[1][i0] * V[2][i2] - V[2][i0] * V[1][i2]) +
                        V[0][i2] * (V[1][i0] * V[2][i1] - V[2][i0] * V[1][i1]);
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) R[3 * a + c] = V[a][i0] * U0[c] + V[a][i1] * U1[c] + detV * V[a][i2] * U2[c];
}


// kabsch_rotation's sibling for a caller that needs the fit but not the rotation: s0 + s1 + sign(det H) s2 of the singular values
// s0 >= s1 >= s2 of H, the trace of R^T H at the optimal proper rotation. The same one-sided Jacobi without V: the column norms of the
// rotated H are the singular values. A rank-deficient H (coincident, collinear or planar atoms) has s2 = 0, so its sign does not matter;
// the determinant is taken from H itself.
__device__ double kabsch_trace(const double* H) {
    double A[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[a][b] = H[3 * a + b];
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < 3; ++k) { alpha += A[k][p] * A[k][p]; beta += A[k][q] * A[k][q]; gamma += A[k][p] * A[k][q]; }
                if (fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;
                rotated = true;
                double c, s;
                jacobi_angle(alpha, beta, gamma, c, s);
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = c * ap - s * aq; A[k][q] = s * ap + c * aq;
                }
            }
        if (!rotated) break;
    }
    double n[3];
    for (int k = 0; k < 3; ++k) n[k] = sqrt(A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k]);
    if (n[0] < n[1]) { const double t = n[0]; n[0] = n[1]; n[1] = t; }
    if (n[1] < n[2]) { const double t = n[1]; n[1] = n[2]; n[2] = t; }
    if (n[0] < n[1]) { const double t = n[0]; n[0] = n[1]; n[1] = t; }
    return det < 0.0 ? (n[0] + n[1]) - n[2] : (n[0] + n[1]) + n[2];
}


// ---- host side
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// smallest non-negative float s (+inf if none) for which pred(s) holds; pred must be monotonic (false ... false true ... true) over
// 0 .. +inf, whose bit patterns are ordered like the values
template <class Pred> float first_true(Pred pred) {
    uint32_t lo = 0u, hi = 0x7f800000u;     // +0 .. +inf
    if (pred(from_bits(lo))) return 0.f;
    if (!pred(from_bits(hi))) return INFINITY;
    while (hi - lo > 1u) {                  // pred(lo) false, pred(hi) true
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pred(from_bits(mid))) hi = mid; else lo = mid;
    }
    return from_bits(hi);
}

float sqrt_rn(float s) { volatile float r = std::sqrt(s); return r; }

// the smallest float s whose distance fl32(sqrt_rn(s)) * scale fails `d < r_thr` (strict) or `d <= r_thr`: the test holds exactly for
// s < s_star (the product is monotonic in s)
float contact_threshold(float r_thr, float scale, bool strict) {
    return first_true([=](float s) {
        volatile float d = sqrt_rn(s) * scale;
        return strict ? !(d < r_thr) : !(d <= r_thr);
    });
}


}  // namespace
}  // namespace pesto
