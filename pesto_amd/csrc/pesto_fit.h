// pesto_fit.h - the one superposition fit of the trajectory, docking, DockQ and TM-score groups (pesto_trajectory.hip, pesto_docking.hip,
// pesto_dockq.hip, pesto_tmscore.hip): a frame fitted onto a reference on an atom selection (Kabsch; the rotation is kabsch_rotation of
// pesto_geom.h), by a workgroup or by one wave on a subset of the points, a point moved by that fit, the squared deviation summed under it, the RMSD kernel made of the three, and the check of the selections'
// indices. The groups promise bit identities between their entry points (pesto_superpose's rmsd_out, pesto_interface_rmsd,
// pesto_fit_rmsd, pesto_dockq's two RMSDs); they hold because every one of them runs the text below. The library is built with
// -ffp-contract=on, so an expression here rounds the same way in every kernel that calls it.
//
// Everything sits in an anonymous namespace (one copy per translation unit, like pesto_geom.h).
#pragma once
#include "pesto_geom.h"

namespace pesto {

namespace {

// ------------------------------------------------------------------------------------------------ the fit
// m: the mean of the fitted points, then of the reference's; R: the rotation, row-major; x' = (x - m[0..2]) R + m[3..5].
// same: the two point sets were equal bit for bit and the fit is the identity itself (R = I, x' = x), not a rotation within rounding of it
struct Fit {
    double m[6], R[9];
    bool same;
};

// a point source of the fit, (int k, double p[3]): atom sel[k] of the float32 frame X in double; OPTIONAL: atom k where there is no list
template <bool OPTIONAL = false>
__device__ __forceinline__ auto atoms(const float* __restrict__ X, const int* __restrict__ sel) {
    return [=](int k, double* p) {
        const float* x = X + (size_t)(OPTIONAL && !sel ? k : sel[k]) * 3;
        p[0] = (double)x[0]; p[1] = (double)x[1]; p[2] = (double)x[2];
    };
}

// one point pair's terms of the two mean sums m (and of the count of coordinates that differ), and of the covariance H about the means
template <bool SHORTCUT>
__device__ __forceinline__ void mean_terms(const double* x, const double* y, double* m, double& differ) {
    for (int c = 0; c < 3; ++c) {
        m[c] += x[c]; m[3 + c] += y[c];
        if (SHORTCUT) differ += x[c] == y[c] ? 0.0 : 1.0;
    }
}

__device__ __forceinline__ void covariance_terms(const double* x, const double* y, const double* m, double* H) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[3 * a + b] += (y[a] - m[3 + a]) * (x[b] - m[b]);
}

// The n points px fitted onto the n points py by the whole workgroup (NT threads, every thread gets the same Fit): the two means, the
// covariance and its rotation, everything in double in a fixed order. SHORTCUT: point sets that are equal value for value are fitted by
// the identity (Fit::same); without it same is false. red: NT / 64 doubles of LDS, sR: 9; both are free for the next use on return
// (until then sR keeps R, unless same).
template <int NT, bool SHORTCUT, class PX, class PY>
__device__ __forceinline__ void kabsch_fit(PX px, PY py, int n, double* red, double* sR, Fit& ft) {
    double* m = ft.m;
    double differ = 0.0;
    for (int c = 0; c < 6; ++c) m[c] = 0.0;
    for (int k = threadIdx.x; k < n; k += NT) {
        double x[3], y[3];
        px(k, x);
        py(k, y);
        mean_terms<SHORTCUT>(x, y, m, differ);
    }
    for (int c = 0; c < 6; ++c) m[c] = block_sum<NT>(m[c], red) / (double)n;
    ft.same = false;
    if (SHORTCUT) ft.same = block_sum<NT>(differ, red) == 0.0;
    if (!ft.same) {
        double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = threadIdx.x; k < n; k += NT) {
            double x[3], y[3];
            px(k, x);
            py(k, y);
            covariance_terms(x, y, m, H);
        }
        for (int c = 0; c < 9; ++c) H[c] = block_sum<NT>(H[c], red);
        if (threadIdx.x == 0) kabsch_rotation(H, sR);
    }
    __syncthreads();
    for (int c = 0; c < 9; ++c) ft.R[c] = ft.same ? (c % 4 == 0 ? 1.0 : 0.0) : sR[c];
    __syncthreads();                    // (sR is free again)
}

// p = x moved by the fit: (x - t) R + t_ref, the point itself under the identity short cut
__device__ __forceinline__ void moved(const double* x, const Fit& ft, double* p) {
    if (ft.same) { p[0] = x[0]; p[1] = x[1]; p[2] = x[2]; return; }
    const double* m = ft.m;
    const double* R = ft.R;
    const double d0 = x[0] - m[0], d1 = x[1] - m[1], d2 = x[2] - m[2];
    for (int c = 0; c < 3; ++c) p[c] = ((d0 * R[c] + d1 * R[3 + c]) + d2 * R[6 + c]) + m[3 + c];
}

// the summed squared deviation of the n points px, moved by the fit, from the points py (the same bits in every thread). The fitted
// points themselves or others; under the identity short cut the terms are (x - y)^2, exactly 0 for a finite point that is the reference's
template <int NT, class PX, class PY>
__device__ __forceinline__ double moved_deviation(PX px, PY py, int n, const Fit& ft, double* red) {
    double dev = 0.0;
    for (int k = threadIdx.x; k < n; k += NT) {
        double x[3], y[3], p[3];
        px(k, x);
        py(k, y);
        moved(x, ft, p);
        for (int c = 0; c < 3; ++c) {
            const double e = p[c] - y[c];
            dev += e * e;
        }
    }
    return block_sum<NT>(dev, red);
}

// ------------------------------------------------------------------------------------------------ the fit of one wave on a subset
// v summed (or its minimum taken) over the wave's 64 lanes by a fixed butterfly: the same bits in every lane, no barrier
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// kabsch_fit by ONE wave on a subset of the n points (pesto_tmscore.hip): lane l owns the points l + 64 j and bit j of its word `in`
// says whether point l + 64 j is fitted on (n <= 64 * 64; at least one point is). The same sums as kabsch_fit, over the members, by the
// wave's butterfly; every lane then runs kabsch_rotation on the same bits, so every lane holds the same Fit and nothing goes through
// LDS or a barrier: the waves of a workgroup fit independently.
template <bool SHORTCUT, class PX, class PY>
__device__ __forceinline__ void kabsch_fit_wave(PX px, PY py, int n, unsigned long long in, Fit& ft) {
    const int lane = threadIdx.x & 63;
    double* m = ft.m;
    double differ = 0.0;
    int members = 0;
    for (int c = 0; c < 6; ++c) m[c] = 0.0;
    for (int j = 0, k = lane; k < n; ++j, k += 64)
        if (in >> j & 1ull) {
            double x[3], y[3];
            px(k, x);
            py(k, y);
            mean_terms<SHORTCUT>(x, y, m, differ);
            ++members;
        }
    const double ns = (double)wave_sum(members);
    for (int c = 0; c < 6; ++c) m[c] = wave_sum(m[c]) / ns;
    ft.same = SHORTCUT && wave_sum(differ) == 0.0;
    for (int c = 0; c < 9; ++c) ft.R[c] = c % 4 == 0 ? 1.0 : 0.0;
    if (!ft.same) {
        double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0, k = lane; k < n; ++j, k += 64)
            if (in >> j & 1ull) {
                double x[3], y[3];
                px(k, x);
                py(k, y);
                covariance_terms(x, y, m, H);
            }
        for (int c = 0; c < 9; ++c) H[c] = wave_sum(H[c]);
        kabsch_rotation(H, ft.R);
    }
}

// ------------------------------------------------------------------------------------------------ the RMSD after a fit
// rmsd_out[f] = the RMSD of the atoms sel_M of frame f from the reference's after the fit on the atoms sel_F, times scale: the interface
// RMSD (sel_M = sel_F) and the ligand RMSD (fit on the receptor, measured on the ligand). One workgroup per frame; Fr = 1: one reference
// frame for all. *err != 0 (k_index_check): nothing is written.
template <int NT>
__global__ __launch_bounds__(NT) void k_fit_rmsd(int Fr, int N, int nF, int nM, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                 const int* __restrict__ sel_F, const int* __restrict__ sel_M, const int* __restrict__ err, double scale,
                                                 float* __restrict__ rmsd_out) {
    __shared__ double red[NT / 64];
    __shared__ double sR[9];
    if (*err) return;
    const size_t f = blockIdx.x;
    const float* X = xyz + f * (size_t)N * 3;
    const float* Y = ref + (Fr == 1 ? 0 : f) * (size_t)N * 3;
    Fit ft;
    kabsch_fit<NT, true>(atoms(X, sel_F), atoms(Y, sel_F), nF, red, sR, ft);
    const double dev = moved_deviation<NT>(atoms(X, sel_M), atoms(Y, sel_M), nM, ft, red);
    if (threadIdx.x == 0) rmsd_out[f] = (float)(sqrt(dev / (double)nM) * scale);
}

// ------------------------------------------------------------------------------------------------ the index check
// Every index of a selection is validated before a fit dereferences it: up to four lists, laid end to end, must lie in [0, N) (error
// bit 0 of *err). The kernels return at once when a bit is set, so a refused call writes nothing.
struct IndexLists {
    const int* list[4];
    long long n[4];             // 0: no such list
    long long total() const { return n[0] + n[1] + n[2] + n[3]; }
};

// the check of index k of the lists; false for a k past their end, which then counts from it
__device__ __forceinline__ bool check_index(long long& k, int N, const IndexLists& L, int* __restrict__ err) {
    for (int l = 0; l < 4; ++l) {
        if (k < L.n[l]) {
            const int i = L.list[l][k];
            if (i < 0 || i >= N) atomicOr(err, 1);
            return true;
        }
        k -= L.n[l];
    }
    return false;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_index_check(int N, IndexLists L, int* __restrict__ err) {
    long long k = (long long)blockIdx.x * NT + threadIdx.x;
    check_index(k, N, L, err);
}

}  // namespace
}  // namespace pesto
