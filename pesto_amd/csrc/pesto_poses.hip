// pesto_poses.hip - rigid poses of a ligand on a receptor that never moves: the step between the interface prediction and the scoring of
// finished complexes. A pose is a transform (R float32 [3,3] row-major, t float32 [3]); the ligand is seen through the placement
//     y_a = ((R[a,0]*x_0 + R[a,1]*x_1) + R[a,2]*x_2) + t_a          float32, every operation rounded as written (place())
// and through nothing else, so the frames [F, N, 3] are never stored unless the caller asks for them (pesto_poses_materialize).
//     pesto_poses_scores        per pose: atom contacts and clashes, the two posed interfaces as residue sets, their distinct residue
//                               pairs, the sums of the predicted interface probabilities over them and the soft Dice overlap
//     pesto_poses_slide         per pose: how far the ligand, withdrawn along a direction, can be pushed back until it first touches
//     pesto_poses_materialize   the placed frames, for the scoring groups that take frames
//     pesto_poses_top           the best k eligible poses by score (the radix sort of pesto_radix.h)
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h, with a message channel of their own.
//
// Scoring. One cell grid over the receptor per call (grid_build of pesto_cellgrid.h, cells at least r_contact / scale * 1.001 wide; on a
// copy of the receptor that holds finite coordinates only: k_poses_clean), one
// workgroup per pose. The ligand's atoms come sorted by residue (a permutation and its offsets); a wave owns the ligand residues
// w, w + 4, ...; it places one atom at a time in registers (the placement is wave-uniform), and its 64 lanes walk the nine rows of three
// cells around the atom, 64 receptor atoms at a time. A pair is a contact when s < s_star, s the float32 squared distance of pesto_geom.h
// and s_star the smallest float at which fl32(sqrt_rn(s)) * scale < r fails (contact_threshold), so the decision is the docking group's
// d < r exactly. Counts are ballots; the receptor residues a ligand residue touches are a bit mask of the wave in LDS (integer atomicOr),
// which gives the distinct residue pairs and their products when the residue is done and is then folded into the pose's receptor mask.
// A placed atom more than a cell and a half outside the grid is skipped (conservative: see near()); any other one outside the box is
// clamped by cell3 onto the boundary cells, whose rows hold every receptor atom within a cell of it. Nothing depends on the order of the
// atoms inside a cell, which is the one thing the grid's build leaves to scheduling: the counts are integers, the masks are ORs and the
// double sums run over the masks in bit order. No floating-point atomics anywhere.
//
// Sliding. All pairs, one workgroup per pose: a thread keeps one placed ligand atom in double registers, receptor tiles of 256 atoms are
// staged in LDS, and the root is taken only where -b + rho can still reach the running maximum. The maximum and its smallest (i, j) do
// not depend on the order, so the result is the definition's bit for bit.
#include <cmath>

#include "pesto_call.h"
#include "pesto_cellgrid.h"
#include "pesto_geom.h"
#include "pesto_radix.h"

namespace pesto {

namespace {

constexpr int NT = 256;                                 // threads per workgroup of every kernel here
constexpr int NW = NT / 64;                             // its waves
constexpr int MAXW = PESTO_POSES_MAX_RESIDUES / 32;     // words of one residue mask at most
static_assert(MAXW <= NT, "a thread per word of a residue mask");

// ------------------------------------------------------------------------------------------------ the placement
// coordinate a of the placed atom: ((R[a,0]*x0 + R[a,1]*x1) + R[a,2]*x2) + t_a, no contraction (row: R + 3 a)
__device__ __forceinline__ float place(const float* row, float t, float x0, float x1, float x2) {
#pragma clang fp contract(off)
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(row[0], x0), __fmul_rn(row[1], x1)), __fmul_rn(row[2], x2)), t);
}

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.402823466e38f; }

// sum of v over the workgroup, the same value in every thread (block_sum's integer sibling). ired: NW ints; two barriers
__device__ __forceinline__ int block_count(int v, int* ired) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = ired[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += ired[w];
    return t;
}

// ------------------------------------------------------------------------------------------------ the check
// Everything the kernels below index or rely on, validated before any of them runs; they return at once when a bit is set, so a refused
// call writes nothing. Any array may be NULL (the entry point does not take it). Error bits:
//     1   res_R outside [0, R_R), perm_L outside [0, N_L), or off_L not 0 = off_L[0] < off_L[1] < ... < off_L[R_L] = N_L
//     2   a probability that is negative or not finite
//     4   a rotation or translation (origin) that is not finite
//     8   a direction with | |u|^2 - 1 | > 1e-3 (in double)
// Workgroup 0 also leaves P_R = sum p_R and P_L = sum p_L (double, block_sum's fixed order) in psum[0 .. 1]. With grid_R (the receptor
// whose grid the call builds) anchor[0], which starts as 2^32 - 1, ends as the first receptor atom with three finite coordinates (an
// integer minimum: the same whatever the order).
__global__ __launch_bounds__(NT) void k_poses_check(long long F, int N_R, int N_L, int R_R, int R_L, const int* __restrict__ res_R,
                                                    const int* __restrict__ perm_L, const int* __restrict__ off_L, const float* __restrict__ p_R,
                                                    const float* __restrict__ p_L, const float* __restrict__ rot, const float* __restrict__ trans,
                                                    const float* __restrict__ dir, const float* __restrict__ grid_R, int* __restrict__ err,
                                                    double* __restrict__ psum, unsigned* __restrict__ anchor) {
    __shared__ double red[NW];
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    int bad = 0;
    if (grid_R && k < N_R && finite3(grid_R + 3 * (size_t)k)) atomicMin(anchor, (unsigned)k);
    if (res_R && k < N_R && (unsigned)res_R[k] >= (unsigned)R_R) bad |= 1;
    if (perm_L && k < N_L && (unsigned)perm_L[k] >= (unsigned)N_L) bad |= 1;
    if (off_L && k < R_L) {
        if (!(off_L[k] < off_L[k + 1]) || (k == 0 && off_L[0] != 0) || (k == R_L - 1 && off_L[R_L] != N_L)) bad |= 1;
    }
    if (p_R && k < R_R && !(p_R[k] >= 0.f && finite32(p_R[k]))) bad |= 2;
    if (p_L && k < R_L && !(p_L[k] >= 0.f && finite32(p_L[k]))) bad |= 2;
    if (k < F) {
        bool ok = true;
        if (rot)
            for (int c = 0; c < 9; ++c) ok = ok && finite32(rot[9 * k + c]);
        if (trans)
            for (int c = 0; c < 3; ++c) ok = ok && finite32(trans[3 * k + c]);
        if (!ok) bad |= 4;
        if (dir) {
            const double u0 = dir[3 * k], u1 = dir[3 * k + 1], u2 = dir[3 * k + 2];
            const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(u0, u0), __dmul_rn(u1, u1)), __dmul_rn(u2, u2));
            if (!(fabs(n2 - 1.0) <= 1e-3)) bad |= 8;
        }
    }
    if (bad) atomicOr(err, bad);
    if (blockIdx.x == 0 && psum) {
        double a = 0.0, b = 0.0;
        for (int r = threadIdx.x; r < R_R; r += NT) a += (double)p_R[r];
        for (int r = threadIdx.x; r < R_L; r += NT) b += (double)p_L[r];
        a = block_sum<NT>(a, red);
        b = block_sum<NT>(b, red);
        if (threadIdx.x == 0) { psum[0] = a; psum[1] = b; }
    }
}

// ------------------------------------------------------------------------------------------------ scoring
// A receptor atom with a non-finite coordinate has no pair by the definition: its distance to anything is NaN or infinite. The grid is
// built on a copy in which such an atom sits on the first finite atom (the origin for a receptor without one), as pesto_lddt.hip builds
// its own: grid_build's set-up takes the box with fminf / fmaxf, which drop a NaN, so a receptor whose atoms are all NaN on an axis would
// otherwise give it an empty box and cell counts that mean nothing. The copy has finite coordinates only; the box is the finite atoms'.
__global__ __launch_bounds__(NT) void k_poses_clean(int N_R, const float* __restrict__ X, const unsigned* __restrict__ anchor, float* __restrict__ Xc) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N_R) return;
    const unsigned a = finite3(X + 3 * (size_t)i) ? (unsigned)i : *anchor;
#pragma unroll
    for (int c = 0; c < 3; ++c) Xc[3 * (size_t)i + c] = a == 0xffffffffu ? 0.f : X[3 * (size_t)a + c];
}

// the receptor residue of every atom rides beside the cell-ordered coordinates; an atom that was moved for the grid gets NaN coordinates
// there (the scatter has just written sorted[pos]), so that it passes no test wherever it was binned
struct ResiduePayload {
    const int* res;
    int* out;
    const float* X;             // the caller's coordinates
    float4* sorted;
    __device__ void operator()(int pos, int i) const {
        out[pos] = res[i];
        if (!finite3(X + 3 * (size_t)i)) sorted[pos] = make_float4(NAN, NAN, NAN, __int_as_float(i));
    }
};

// false only where no receptor atom can lie within a cell edge h (>= r_contact / scale * 1.001) of the coordinate: fx is the cell
// coordinate before cell3 clamps it, with a relative error of a few 2^-24 (one subtraction, one product); the box starts at 0 and ends
// below n (n = (int)(extent / h) + 1), so an atom within h of it has -1 <= fx < n + 1, and the margins of a cell and a half on either
// side leave half a cell to those roundings. On the one-cell path inv_h is 0 and fx is 0 or NaN: always true. A NaN coordinate is
// true as well (its distances are NaN and pass no test).
__device__ __forceinline__ bool near(float v, float lo, float inv_h, int n) {
    const float fx = (v - lo) * inv_h;
    return !(fx < -1.5f || fx > (float)n + 1.5f);
}

// 2 w / (n + P), 0 where the denominator is 0 (double, every operation rounded as written)
__device__ __forceinline__ double dice(double w, int n, double P) {
    const double den = __dadd_rn((double)n, P);
    return den == 0.0 ? 0.0 : __ddiv_rn(__dmul_rn(2.0, w), den);
}

// one workgroup per pose: see the head of the file. masks may be NULL.
__global__ __launch_bounds__(NT) void k_pose_scores(int R_R, int R_L, const CellGrid* __restrict__ grid, const int* __restrict__ cell_start,
                                                    const float4* __restrict__ sorted, const int* __restrict__ res_sorted,
                                                    const float* __restrict__ xyz_L, const int* __restrict__ perm_L, const int* __restrict__ off_L,
                                                    const float* __restrict__ rot, const float* __restrict__ trans, const float* __restrict__ p_R,
                                                    const float* __restrict__ p_L, const double* __restrict__ psum, const int* __restrict__ err,
                                                    float s_contact, float s_clash, int* __restrict__ n_contact_out, int* __restrict__ n_clash_out,
                                                    int* __restrict__ n_res_R_out, int* __restrict__ n_res_L_out, int* __restrict__ n_pairs_out,
                                                    double* __restrict__ w_R_out, double* __restrict__ w_L_out, double* __restrict__ w_pair_out,
                                                    float* __restrict__ score_out, unsigned* __restrict__ masks_out) {
    __shared__ unsigned mR[MAXW], mL[MAXW];
    __shared__ unsigned wm[NW][MAXW];
    __shared__ double red[NW];
    __shared__ int ired[NW];
    if (*err) return;
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int WR = (R_R + 31) >> 5, WL = (R_L + 31) >> 5;
    float Rm[9], tv[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Rm[c] = rot[9 * f + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) tv[c] = trans[3 * f + c];
    if (threadIdx.x < MAXW) {
        mR[threadIdx.x] = 0u;
        mL[threadIdx.x] = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) wm[w][threadIdx.x] = 0u;
    }
    __syncthreads();
    const CellGrid g = *grid;
    const int* start = cell_start + g.base;
    int nc = 0, ncl = 0;            // wave-uniform: the contacts and clashes this wave has seen
    int npair = 0;                  // this lane's share of the distinct residue pairs
    double wp = 0.0;                // and of their products, in the fixed order (ligand residue, mask word, bit)
    for (int s = wave; s < R_L; s += NW) {
        bool any = false;
        const int a1 = off_L[s + 1];
        for (int a = off_L[s]; a < a1; ++a) {
            const float* x = xyz_L + 3 * (size_t)perm_L[a];
            const float x0 = x[0], x1 = x[1], x2 = x[2];
            const float y0 = place(Rm, tv[0], x0, x1, x2), y1 = place(Rm + 3, tv[1], x0, x1, x2), y2 = place(Rm + 6, tv[2], x0, x1, x2);
            if (!(near(y0, g.minx, g.inv_h, g.nx) && near(y1, g.miny, g.inv_h, g.ny) && near(y2, g.minz, g.inv_h, g.nz))) continue;
            int cx, cy, cz;
            cell3(g, y0, y1, y2, cx, cy, cz);
            const int c0 = max(cx - 1, 0), c1 = min(cx + 1, g.nx - 1);
            int j0[9], j1[9];                                      // the nine rows' ranges of the cell-ordered atoms (empty off the grid)
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const int z = cz + q / 3 - 1, y = cy + q % 3 - 1;
                const bool in = z >= 0 && z < g.nz && y >= 0 && y < g.ny;
                const int row = in ? (z * g.ny + y) * g.nx : 0;
                j0[q] = in ? start[row + c0] : 0;
                j1[q] = in ? start[row + c1 + 1] : 0;
            }
#pragma unroll
            for (int q = 0; q < 9; ++q)
                for (int jb = j0[q]; jb < j1[q]; jb += 64) {
                    const int j = jb + lane;
                    bool hit = false, clash = false;
                    if (j < j1[q]) {
                        const float4 b = sorted[j];
                        const float d2 = dist2(b.x, b.y, b.z, y0, y1, y2);
                        hit = d2 < s_contact;                      // (NaN: false)
                        clash = d2 < s_clash;
                    }
                    const unsigned long long h = __ballot(hit);
                    if (h != 0ull) {
                        any = true;
                        nc += __popcll(h);
                        ncl += __popcll(__ballot(clash));          // (r_clash <= r_contact: a clash is a contact)
                        if (hit) {
                            const int r = res_sorted[j];           // in [0, R_R): k_poses_check
                            atomicOr(&wm[wave][r >> 5], 1u << (r & 31));
                        }
                    }
                }
        }
        if (any) {                                                  // the residue pairs of ligand residue s: the wave's mask, word by word
            __threadfence_block();
            const double pl = (double)p_L[s];
            for (int k = lane; k < WR; k += 64) {
                unsigned bits = wm[wave][k];
                if (bits) {
                    wm[wave][k] = 0u;
                    atomicOr(&mR[k], bits);
                    npair += __popc(bits);
                    while (bits) {
                        const int b = __ffs(bits) - 1;
                        bits &= bits - 1u;
                        wp = __dadd_rn(wp, __dmul_rn((double)p_R[32 * k + b], pl));        // (the product is exact)
                    }
                }
            }
            if (lane == 0) atomicOr(&mL[s >> 5], 1u << (s & 31));
            __threadfence_block();
        }
    }
    __syncthreads();
    const int n_contact = block_count(lane == 0 ? nc : 0, ired), n_clash = block_count(lane == 0 ? ncl : 0, ired);
    const int n_pairs = block_count(npair, ired);
    const double w_pair = block_sum<NT>(wp, red);
    // the two interfaces: thread k owns word k of either mask
    int cR = 0, cL = 0;
    double sR = 0.0, sL = 0.0;
    if ((int)threadIdx.x < WR) {
        unsigned bits = mR[threadIdx.x];
        if (masks_out) masks_out[f * (size_t)(WR + WL) + threadIdx.x] = bits;
        cR = __popc(bits);
        while (bits) { const int b = __ffs(bits) - 1; bits &= bits - 1u; sR = __dadd_rn(sR, (double)p_R[32 * threadIdx.x + b]); }
    }
    if ((int)threadIdx.x < WL) {
        unsigned bits = mL[threadIdx.x];
        if (masks_out) masks_out[f * (size_t)(WR + WL) + WR + threadIdx.x] = bits;
        cL = __popc(bits);
        while (bits) { const int b = __ffs(bits) - 1; bits &= bits - 1u; sL = __dadd_rn(sL, (double)p_L[32 * threadIdx.x + b]); }
    }
    const int n_res_R = block_count(cR, ired), n_res_L = block_count(cL, ired);
    const double w_R = block_sum<NT>(sR, red), w_L = block_sum<NT>(sL, red);
    if (threadIdx.x == 0) {
        n_contact_out[f] = n_contact;
        n_clash_out[f] = n_clash;
        n_res_R_out[f] = n_res_R;
        n_res_L_out[f] = n_res_L;
        n_pairs_out[f] = n_pairs;
        w_R_out[f] = w_R;
        w_L_out[f] = w_L;
        w_pair_out[f] = w_pair;
        score_out[f] = (float)__ddiv_rn(__dadd_rn(dice(w_R, n_res_R, psum[0]), dice(w_L, n_res_L, psum[1])), 2.0);
    }
}

// ------------------------------------------------------------------------------------------------ sliding
// (s, i, j) beats (t, k, l): a larger s, or the same s at a smaller (i, then j)
__device__ __forceinline__ bool beats(double s, int i, int j, double t, int k, int l) { return s > t || (s == t && (i < k || (i == k && j < l))); }

// one workgroup per pose. In double, every operation rounded as written: w = y_j - x_i, b = w . u, c = |w|^2 - b^2, disc = rho^2 - c; a
// pair counts where disc > 0 (a NaN passes no test) and gives s_ij = -b + sqrt(disc). Where c >= 0, disc <= fl(rho^2), whose correctly
// rounded root is rho itself, so s_ij <= fl(rho - b) by the monotonicity of rounding: below the running maximum the root is not taken.
// (With c < 0, which rounding or a direction a little off unit length can give, there is no such bound and the root is taken.)
__global__ __launch_bounds__(NT) void k_pose_slide(int N_R, int N_L, const float* __restrict__ xyz_R, const float* __restrict__ xyz_L,
                                                   const float* __restrict__ rot, const float* __restrict__ org, const float* __restrict__ dir,
                                                   const int* __restrict__ err, double rho, double* __restrict__ s_out, float* __restrict__ t_out,
                                                   int* __restrict__ pair_out) {
#pragma clang fp contract(off)
    __shared__ float tile[NT * 3];
    __shared__ double sb[NT];
    __shared__ int si[NT], sj[NT];
    if (*err) return;
    const size_t f = blockIdx.x;
    float Rm[9], o[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Rm[c] = rot[9 * f + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = org[3 * f + c];
    const double u0 = dir[3 * f], u1 = dir[3 * f + 1], u2 = dir[3 * f + 2];
    const double rho2 = __dmul_rn(rho, rho);
    double best = -INFINITY;
    int bi = -1, bj = -1;
    for (int jb = 0; jb < N_L; jb += NT) {
        const int j = jb + (int)threadIdx.x;
        const bool have = j < N_L;
        double y0 = 0.0, y1 = 0.0, y2 = 0.0;
        if (have) {
            const float* x = xyz_L + 3 * (size_t)j;
            const float x0 = x[0], x1 = x[1], x2 = x[2];
            y0 = (double)place(Rm, o[0], x0, x1, x2); y1 = (double)place(Rm + 3, o[1], x0, x1, x2); y2 = (double)place(Rm + 6, o[2], x0, x1, x2);
        }
        for (int ib = 0; ib < N_R; ib += NT) {
            const int n = min(NT, N_R - ib);
            __syncthreads();
            for (int k = threadIdx.x; k < 3 * n; k += NT) tile[k] = xyz_R[3 * (size_t)ib + k];
            __syncthreads();
            if (!have) continue;
            for (int i = 0; i < n; ++i) {
                const double w0 = __dsub_rn(y0, (double)tile[3 * i]), w1 = __dsub_rn(y1, (double)tile[3 * i + 1]), w2 = __dsub_rn(y2, (double)tile[3 * i + 2]);
                const double b = __dadd_rn(__dadd_rn(__dmul_rn(w0, u0), __dmul_rn(w1, u1)), __dmul_rn(w2, u2));
                const double c = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(w0, w0), __dmul_rn(w1, w1)), __dmul_rn(w2, w2)), __dmul_rn(b, b));
                const double disc = __dsub_rn(rho2, c);
                if (!(disc > 0.0)) continue;
                if (c >= 0.0 && __dsub_rn(rho, b) < best) continue;
                const double s = __dadd_rn(-b, __dsqrt_rn(disc));
                if (beats(s, ib + i, j, best, bi, bj)) { best = s; bi = ib + i; bj = j; }
            }
        }
    }
    __syncthreads();
    sb[threadIdx.x] = best; si[threadIdx.x] = bi; sj[threadIdx.x] = bj;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && beats(sb[threadIdx.x + off], si[threadIdx.x + off], sj[threadIdx.x + off], sb[threadIdx.x], si[threadIdx.x], sj[threadIdx.x])) {
            sb[threadIdx.x] = sb[threadIdx.x + off]; si[threadIdx.x] = si[threadIdx.x + off]; sj[threadIdx.x] = sj[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool hit = si[0] >= 0;
        const double s = hit ? sb[0] : (double)NAN;
        s_out[f] = s;
        pair_out[2 * f] = hit ? si[0] : -1;
        pair_out[2 * f + 1] = hit ? sj[0] : -1;
        t_out[3 * f] = hit ? (float)__dadd_rn((double)o[0], __dmul_rn(s, u0)) : NAN;
        t_out[3 * f + 1] = hit ? (float)__dadd_rn((double)o[1], __dmul_rn(s, u1)) : NAN;
        t_out[3 * f + 2] = hit ? (float)__dadd_rn((double)o[2], __dmul_rn(s, u2)) : NAN;
    }
}

// ------------------------------------------------------------------------------------------------ the frames
// a thread per (pose, atom): the receptor's rows copied (N_R = 0 without one), the ligand's placed
__global__ __launch_bounds__(NT) void k_pose_frames(long long total, int N_R, int N_L, const float* __restrict__ xyz_R, const float* __restrict__ xyz_L,
                                                    const float* __restrict__ rot, const float* __restrict__ trans, const int* __restrict__ err,
                                                    float* __restrict__ out) {
    if (*err) return;
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int N = N_R + N_L;
    const long long f = e / N;
    const int a = (int)(e - f * N);
    float v0, v1, v2;
    if (a < N_R) {
        v0 = xyz_R[3 * (size_t)a]; v1 = xyz_R[3 * (size_t)a + 1]; v2 = xyz_R[3 * (size_t)a + 2];
    } else {
        const float* x = xyz_L + 3 * (size_t)(a - N_R);
        const float* Rm = rot + 9 * f;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        v0 = place(Rm, trans[3 * f], x0, x1, x2); v1 = place(Rm + 3, trans[3 * f + 1], x0, x1, x2); v2 = place(Rm + 6, trans[3 * f + 2], x0, x1, x2);
    }
    out[3 * e] = v0; out[3 * e + 1] = v1; out[3 * e + 2] = v2;
}

// ------------------------------------------------------------------------------------------------ the best poses
// Pose f becomes the key desc(score) << 32 | f, desc the order-preserving map of the float's bits, complemented (larger scores first),
// -0.0 canonicalised to +0.0; a pose that is not eligible (a NaN score, or more clashes than allowed) gets desc = 2^32 - 1, which no
// score that is not a NaN has. The stable sort runs on the upper 32 bits alone: equal scores keep the order of the indices.
struct TopState {
    int n;              // the number of keys, which the sort reads on the device
    int eligible;
    RadixState rs;
};

__global__ __launch_bounds__(NT) void k_top_keys(int F, const float* __restrict__ score, const int* __restrict__ n_clash, int max_clash,
                                                 u64* __restrict__ keys, TopState* __restrict__ st) {
    const int f = blockIdx.x * NT + threadIdx.x;
    bool ok = false;
    if (f < F) {
        if (f == 0) st->n = F;
        const float v = score[f];
        ok = v == v && (!n_clash || n_clash[f] <= max_clash);
        unsigned u = __float_as_uint(v);
        if (u == 0x80000000u) u = 0u;
        const unsigned asc = (u >> 31) ? ~u : (u | 0x80000000u);
        keys[f] = (u64)(ok ? ~asc : 0xffffffffu) << 32 | (u64)(unsigned)f;
    }
    const int cnt = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&st->eligible, cnt);
}

__global__ __launch_bounds__(NT) void k_top_emit(int k, const u64* __restrict__ keys_a, const u64* __restrict__ keys_b, int n_pass,
                                                 const TopState* __restrict__ st, int* __restrict__ index_out) {
    const int pos = blockIdx.x * NT + threadIdx.x;
    if (pos >= min(k, st->eligible)) return;
    index_out[pos] = (int)(unsigned)(radix_sorted(keys_a, keys_b, n_pass, &st->rs)[pos] & 0xffffffffull);
}

// ---- host side
// the error of a refused call from the check kernel's bits (0: none)
int check_error(int err, const char* what) {
    if (err & 1)
        return fail(PESTO_ERR_INVALID, "%s: res_R must lie in [0, R_R), perm_L in [0, N_L) and off_L must split [0, N_L] into R_L non-empty ranges", what);
    if (err & 2) return fail(PESTO_ERR_INVALID, "%s: the probabilities p_R and p_L must be finite and >= 0", what);
    if (err & 4) return fail(PESTO_ERR_INVALID, "%s: rotations and translations must be finite", what);
    if (err & 8) return fail(PESTO_ERR_INVALID, "%s: directions must have unit length, | |u|^2 - 1 | <= 1e-3", what);
    return 0;
}

// the common limits of a call on F poses of N_L atoms against N_R
int check_sizes(int64_t F, int64_t N_R, int64_t N_L) {
    if (F < 1 || F > PESTO_POSES_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to 2^23 poses, got %lld", (long long)F);
    if (N_R < 1 || N_L < 1 || N_R > PESTO_POSES_MAX_PAIRS || N_L > PESTO_POSES_MAX_PAIRS || N_R * N_L > PESTO_POSES_MAX_PAIRS)
        return fail(PESTO_ERR_INVALID, "N_R >= 1, N_L >= 1 and N_R * N_L < 2^31, got %lld and %lld", (long long)N_R, (long long)N_L);
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_poses_last_error(void) { return last_error(); }

int pesto_poses_scores(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, int32_t R_R, int32_t R_L, const float* xyz_R, const float* xyz_L,
                       const int32_t* res_R, const int32_t* perm_L, const int32_t* off_L, const float* rotations, const float* translations,
                       const float* p_R, const float* p_L, float r_contact, float r_clash, float scale, int32_t* n_contact_out, int32_t* n_clash_out,
                       int32_t* n_res_R_out, int32_t* n_res_L_out, int32_t* n_pairs_out, double* w_R_out, double* w_L_out, double* w_pair_out,
                       float* score_out, uint32_t* masks_out, int32_t ptr_kind, void* stream) {
    if (!xyz_R || !xyz_L || !res_R || !perm_L || !off_L || !rotations || !translations || !p_R || !p_L || !n_contact_out || !n_clash_out || !n_res_R_out ||
        !n_res_L_out || !n_pairs_out || !w_R_out || !w_L_out || !w_pair_out || !score_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_sizes(F, N_R, N_L)) return rc;
    if (R_R < 1 || R_R > PESTO_POSES_MAX_RESIDUES || R_L < 1 || R_L > PESTO_POSES_MAX_RESIDUES || R_R > N_R || R_L > N_L)
        return fail(PESTO_ERR_INVALID, "1 to %d residues a side, none without an atom, got %d and %d", (int)PESTO_POSES_MAX_RESIDUES, (int)R_R, (int)R_L);
    if (!std::isfinite(r_contact) || !std::isfinite(r_clash) || !std::isfinite(scale) || !(scale > 0.f) || !(0.f <= r_clash && r_clash <= r_contact) ||
        !std::isfinite(r_contact / scale))
        return fail(PESTO_ERR_INVALID, "0 <= r_clash <= r_contact, finite, and scale positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_contact = contact_threshold(r_contact, scale, true), s_clash = contact_threshold(r_clash, scale, true);
    const size_t nR = (size_t)N_R, nL = (size_t)N_L, W = (size_t)((R_R + 31) / 32 + (R_L + 31) / 32);
    const int32_t offs[2] = {0, (int32_t)N_R};                   // the grid's one structure
    Buffers bf(ptr_kind, stream);
    const int iXr = bf.input(xyz_R, nR * 12), iXl = bf.input(xyz_L, nL * 12), iRr = bf.input(res_R, nR * 4), iPm = bf.input(perm_L, nL * 4),
              iOl = bf.input(off_L, ((size_t)R_L + 1) * 4), iRo = bf.input(rotations, (size_t)F * 36), iTr = bf.input(translations, (size_t)F * 12),
              iPr = bf.input(p_R, (size_t)R_R * 4), iPl = bf.input(p_L, (size_t)R_L * 4);
    const int iNc = bf.output(n_contact_out, (size_t)F * 4), iNl = bf.output(n_clash_out, (size_t)F * 4), iNr = bf.output(n_res_R_out, (size_t)F * 4),
              iNs = bf.output(n_res_L_out, (size_t)F * 4), iNp = bf.output(n_pairs_out, (size_t)F * 4), iWr = bf.output(w_R_out, (size_t)F * 8),
              iWl = bf.output(w_L_out, (size_t)F * 8), iWp = bf.output(w_pair_out, (size_t)F * 8), iSc = bf.output(score_out, (size_t)F * 4),
              iMk = bf.output(masks_out, (size_t)F * W * 4);
    const size_t cells = cells_before(nR, 1);
    const int iSt = bf.scratch(sizeof(int), 0), iPs = bf.scratch(16), iOf = bf.table(offs, 8), iG = bf.scratch(sizeof(CellGrid)),
              iCnt = bf.scratch(cells * 4), iCur = bf.scratch(cells * 4), iCell = bf.scratch(nR * 4), iSort = bf.scratch(nR * 16),
              iRs = bf.scratch(nR * 4), iAn = bf.scratch(sizeof(unsigned), 0xff), iXc = bf.scratch(nR * 12);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const size_t n_check = std::max({nR, nL, (size_t)F, (size_t)R_R, (size_t)R_L});
        hipLaunchKernelGGL(k_poses_check, dim3(blocks(n_check, NT)), dim3(NT), 0, bf.stm, (long long)F, (int)N_R, (int)N_L, (int)R_R, (int)R_L,
                           bf.ptr<const int>(iRr), bf.ptr<const int>(iPm), bf.ptr<const int>(iOl), bf.ptr<const float>(iPr), bf.ptr<const float>(iPl),
                           bf.ptr<const float>(iRo), bf.ptr<const float>(iTr), (const float*)nullptr, bf.ptr<const float>(iXr), bf.ptr<int>(iSt),
                           bf.ptr<double>(iPs), bf.ptr<unsigned>(iAn));
        // the grid sees finite coordinates only (k_poses_clean)
        hipLaunchKernelGGL(k_poses_clean, dim3(blocks(nR, NT)), dim3(NT), 0, bf.stm, (int)N_R, bf.ptr<const float>(iXr), (const unsigned*)bf.ptr<unsigned>(iAn),
                           bf.ptr<float>(iXc));
        CellGrid* g = bf.ptr<CellGrid>(iG);
        int* cell_cnt = bf.ptr<int>(iCnt);
        // (a cell edge of 0 would divide by it: r_contact = 0 has no contact whatever the cells)
        grid_build(bf.stm, (int)N_R, 1, bf.ptr<const int>(iOf), (const float*)bf.ptr<float>(iXc), std::max(r_contact / scale, 1e-30f),
                   GridBufs{g, cell_cnt, bf.ptr<int>(iCur), bf.ptr<int>(iCell), bf.ptr<float4>(iSort)}, NoCheck{},
                   ResiduePayload{bf.ptr<const int>(iRr), bf.ptr<int>(iRs), bf.ptr<const float>(iXr), bf.ptr<float4>(iSort)});
        hipLaunchKernelGGL(k_pose_scores, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)R_R, (int)R_L, (const CellGrid*)g, (const int*)cell_cnt,
                           (const float4*)bf.ptr<float4>(iSort), (const int*)bf.ptr<int>(iRs), bf.ptr<const float>(iXl), bf.ptr<const int>(iPm),
                           bf.ptr<const int>(iOl), bf.ptr<const float>(iRo), bf.ptr<const float>(iTr), bf.ptr<const float>(iPr), bf.ptr<const float>(iPl),
                           (const double*)bf.ptr<double>(iPs), (const int*)bf.ptr<int>(iSt), s_contact, s_clash, bf.ptr<int>(iNc), bf.ptr<int>(iNl),
                           bf.ptr<int>(iNr), bf.ptr<int>(iNs), bf.ptr<int>(iNp), bf.ptr<double>(iWr), bf.ptr<double>(iWl), bf.ptr<double>(iWp),
                           bf.ptr<float>(iSc), bf.ptr<unsigned>(iMk));
    }
    // a refused call writes nothing: the check's verdict is read before any output is copied back
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "poses_scores");
    if (rc == 0) rc = check_error(herr, "poses_scores");
    return bf.finish(rc, "poses_scores");
}

int pesto_poses_slide(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, const float* xyz_R, const float* xyz_L, const float* rotations,
                      const float* origins, const float* directions, float r_touch, float scale, double* s_out, float* translations_out,
                      int32_t* pair_out, int32_t ptr_kind, void* stream) {
    if (!xyz_R || !xyz_L || !rotations || !origins || !directions || !s_out || !translations_out || !pair_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_sizes(F, N_R, N_L)) return rc;
    if (!std::isfinite(r_touch) || !std::isfinite(scale) || !(scale > 0.f) || !(r_touch >= 0.f))
        return fail(PESTO_ERR_INVALID, "r_touch must be finite and >= 0 and scale positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    const double rho = (double)r_touch / (double)scale;
    Buffers bf(ptr_kind, stream);
    const int iXr = bf.input(xyz_R, (size_t)N_R * 12), iXl = bf.input(xyz_L, (size_t)N_L * 12), iRo = bf.input(rotations, (size_t)F * 36),
              iOr = bf.input(origins, (size_t)F * 12), iDi = bf.input(directions, (size_t)F * 12);
    const int iS = bf.output(s_out, (size_t)F * 8), iT = bf.output(translations_out, (size_t)F * 12), iP = bf.output(pair_out, (size_t)F * 8);
    const int iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_poses_check, dim3(blocks((size_t)F, NT)), dim3(NT), 0, bf.stm, (long long)F, 0, 0, 0, 0, (const int*)nullptr,
                           (const int*)nullptr, (const int*)nullptr, (const float*)nullptr, (const float*)nullptr, bf.ptr<const float>(iRo),
                           bf.ptr<const float>(iOr), bf.ptr<const float>(iDi), (const float*)nullptr, bf.ptr<int>(iSt), (double*)nullptr, (unsigned*)nullptr);
        hipLaunchKernelGGL(k_pose_slide, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)N_R, (int)N_L, bf.ptr<const float>(iXr), bf.ptr<const float>(iXl),
                           bf.ptr<const float>(iRo), bf.ptr<const float>(iOr), bf.ptr<const float>(iDi), (const int*)bf.ptr<int>(iSt), rho,
                           bf.ptr<double>(iS), bf.ptr<float>(iT), bf.ptr<int>(iP));
    }
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "poses_slide");
    if (rc == 0) rc = check_error(herr, "poses_slide");
    return bf.finish(rc, "poses_slide");
}

int pesto_poses_materialize(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, const float* xyz_R, const float* xyz_L, const float* rotations,
                            const float* translations, float* xyz_out, int32_t ptr_kind, void* stream) {
    if (!xyz_L || !rotations || !translations || !xyz_out || (N_R > 0 && !xyz_R)) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_POSES_MAX_FRAMES || N_R < 0 || N_L < 1 || N_R > PESTO_POSES_MAX_PLACED || N_L > PESTO_POSES_MAX_PLACED ||
        F * (N_R + N_L) > PESTO_POSES_MAX_PLACED)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 poses, N_R >= 0, N_L >= 1 and F * (N_R + N_L) < 2^31");
    if (int rc = begin(m, ptr_kind)) return rc;
    const long long total = (long long)F * (N_R + N_L);
    Buffers bf(ptr_kind, stream);
    const int iXr = bf.input(N_R ? xyz_R : nullptr, (size_t)N_R * 12), iXl = bf.input(xyz_L, (size_t)N_L * 12), iRo = bf.input(rotations, (size_t)F * 36),
              iTr = bf.input(translations, (size_t)F * 12), iO = bf.output(xyz_out, (size_t)total * 12), iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_poses_check, dim3(blocks((size_t)F, NT)), dim3(NT), 0, bf.stm, (long long)F, 0, 0, 0, 0, (const int*)nullptr,
                           (const int*)nullptr, (const int*)nullptr, (const float*)nullptr, (const float*)nullptr, bf.ptr<const float>(iRo),
                           bf.ptr<const float>(iTr), (const float*)nullptr, (const float*)nullptr, bf.ptr<int>(iSt), (double*)nullptr, (unsigned*)nullptr);
        hipLaunchKernelGGL(k_pose_frames, dim3(blocks((size_t)total, NT)), dim3(NT), 0, bf.stm, total, (int)N_R, (int)N_L, bf.ptr<const float>(iXr),
                           bf.ptr<const float>(iXl), bf.ptr<const float>(iRo), bf.ptr<const float>(iTr), (const int*)bf.ptr<int>(iSt), bf.ptr<float>(iO));
    }
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "poses_materialize");
    if (rc == 0) rc = check_error(herr, "poses_materialize");
    return bf.finish(rc, "poses_materialize");
}

int pesto_poses_top(pesto_model* m, int64_t F, int64_t k, const float* score, const int32_t* n_clash, int32_t max_clash, int32_t* index_out,
                    int64_t* count_out, int32_t ptr_kind, void* stream) {
    if (!score || !count_out || (k > 0 && !index_out)) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_POSES_MAX_FRAMES || k < 0) return fail(PESTO_ERR_INVALID, "1 to 2^23 poses and k >= 0");
    if (int rc = begin(m, ptr_kind)) return rc;
    const int64_t cap = std::min(k, F);
    constexpr int n_pass = 4;                                    // the score's 32 bits
    Buffers bf(ptr_kind, stream);
    const int iSc = bf.input(score, (size_t)F * 4), iCl = bf.input(n_clash, (size_t)F * 4);
    const int iIx = bf.partial(index_out, (size_t)cap * 4);
    const int iSt = bf.scratch(sizeof(TopState), 0), iKa = bf.scratch((size_t)F * 8), iKb = bf.scratch((size_t)F * 8),
              iCnt = bf.scratch(radix_counter_bytes((size_t)F));
    TopState hs{};
    int rc = bf.upload();
    if (rc == 0) {
        TopState* st = bf.ptr<TopState>(iSt);
        u64 *ka = bf.ptr<u64>(iKa), *kb = bf.ptr<u64>(iKb);
        hipLaunchKernelGGL(k_top_keys, dim3(blocks((size_t)F, NT)), dim3(NT), 0, bf.stm, (int)F, bf.ptr<const float>(iSc), bf.ptr<const int>(iCl),
                           (int)max_clash, ka, st);
        radix_sort(bf.stm, ka, kb, (long long)F, &st->n, 32, n_pass, bf.ptr<int>(iCnt), &st->rs);
        if (cap > 0)
            hipLaunchKernelGGL(k_top_emit, dim3(blocks((size_t)cap, NT)), dim3(NT), 0, bf.stm, (int)cap, (const u64*)ka, (const u64*)kb, n_pass,
                               (const TopState*)st, bf.ptr<int>(iIx));
    }
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "poses_top");
    int64_t n = 0;
    if (rc == 0) {
        n = std::min<int64_t>(cap, hs.eligible);
        rc = bf.fetch(iIx, (size_t)n * 4);
    }
    rc = bf.finish(rc, "poses_top");
    if (rc == 0) count_out[0] = n;
    return rc;
}
