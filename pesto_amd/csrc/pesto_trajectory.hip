// pesto_trajectory.hip - MD ensemble analysis: the statistical contacts model (binned pair-distance counts over the frames, their
// distribution, per-frame log-likelihood, KL divergence), residue contact maps and native contacts, superposition / RMSD and residue
// centroids of every frame of a trajectory.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h.
//
// Distances are NumPy's / torch's float32 ones: d = sqrt_rn((dx*dx + dy*dy) + dz*dz), every operation rounded. No kernel takes the square
// root: sqrt_rn is monotonic, so every comparison of d against a bound is made on the rounded sum s against the smallest float s_star whose
// correctly rounded root reaches the bound (the host derives it by bisection over the float bit patterns). A float64 bin edge e is first
// replaced by the smallest float32 not below it, which decides d >= e and d < e exactly for every float32 d.
// Every floating-point reduction runs in double in a fixed order (strided per thread, a fixed butterfly per wave, the waves in turn), and
// partial counts are combined as integers, so every output is bit-identical from call to call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pesto_call.h"
#include "pesto_fit.h"           // (and pesto_geom.h through it)

namespace pesto {

namespace {

constexpr int NT = 256;             // threads per workgroup of every kernel here
constexpr int CT = 16;              // contact counts: a workgroup owns CT x CT atom pairs (one per thread)
constexpr int CF = 32;              // ... and stages the coordinates of CF frames at a time
constexpr int FU = 4;               // ... and runs FU frames' bin searches side by side (independent LDS chains)
constexpr int LT = 32;              // log-likelihood: a workgroup owns LT x LT atom pairs
constexpr int LF = 64;              // ... of LF frames (one per lane), the LT rows split over its four waves
constexpr int LPAD = LF + 1;
constexpr int64_t LOGLIK_SCRATCH = 64 << 20;   // bytes of tile partials per pass of pesto_contact_loglik
constexpr int JU = 4;               // ... with JU partner atoms' bin searches side by side

// Bin search over thr[0 .. 2 * top): the B + 1 thresholds, then +inf up to twice `top`, the largest power of two <= B. Starting from
// lo = 0, the steps top, top / 2, ... 1 leave the largest index whose threshold is <= s (given thr[0] <= s): the same number of steps for
// every lane, no branch. An empty bin (thr[b] == thr[b+1]) is never chosen; s >= thr[B] ends at B or above, which is no bin.
__device__ __forceinline__ void search_step(const float* thr, int step, float s, int& lo) {
    const int mid = lo + step;
    lo = thr[mid] <= s ? mid : lo;
}

__device__ __forceinline__ void lds_count(unsigned* p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- statistical contacts model
// replaces: contacts_distribution's frame loop (md_analysis/mdtraj_utils/statistical_contacts_model.py:7-30). One thread per atom pair
// counts its own bins over the frames [f0, f1) of its split: counters in LDS laid out [bin][thread] (a wave's updates fall on distinct
// banks), coordinates of CF frames staged per barrier. One split stores its counts, several add them with integer atomics into the
// zeroed output.
__global__ __launch_bounds__(NT) void k_contact_counts(int F, int Na, int Nb, const float* __restrict__ x0, const float* __restrict__ x1, int B,
                                                       int top, const float* __restrict__ sq, unsigned* __restrict__ counts, int tiles_j,
                                                       int tiles_ij, int splits, int per_split) {
    extern __shared__ float4 lds_q[];
    float4* ca = lds_q;                                 // [CF][CT] (x, y, z, -)
    float4* cb = ca + CF * CT;                          // [CF][CT]
    unsigned* cnt = (unsigned*)(cb + CF * CT);          // [B][NT]
    float* thr = (float*)(cnt + (size_t)B * NT);        // [2 * top]
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int tile = (int)(blockIdx.x % (unsigned)tiles_ij), split = (int)(blockIdx.x / (unsigned)tiles_ij);
    const int i0 = (tile / tiles_j) * CT, j0 = (tile % tiles_j) * CT;
    const int na = min(CT, Na - i0), nb = min(CT, Nb - j0);
    const int f0 = split * per_split, f1 = min(F, f0 + per_split);
    for (int b = 0; b < B; ++b) cnt[b * NT + tid] = 0u;
    for (int k = tid; k < 2 * top; k += NT) thr[k] = k <= B ? sq[k] : INFINITY;
    const float lo = sq[0], hi = sq[B];
    for (int fc = f0; fc < f1; fc += CF) {
        const int nf = min(CF, f1 - fc);
        __syncthreads();
        for (int idx = tid; idx < CF * CT; idx += NT) {     // (a NaN coordinate never hits a bin: frames and atoms beyond the end)
            const int f = idx / CT, k = idx % CT;
            float4 a = make_float4(NAN, NAN, NAN, 0.f), b = a;
            if (f < nf && k < na) { const float* p = x0 + ((size_t)(fc + f) * Na + i0 + k) * 3; a = make_float4(p[0], p[1], p[2], 0.f); }
            if (f < nf && k < nb) { const float* p = x1 + ((size_t)(fc + f) * Nb + j0 + k) * 3; b = make_float4(p[0], p[1], p[2], 0.f); }
            ca[idx] = a;
            cb[idx] = b;
        }
        __syncthreads();
        for (int f = 0; f < nf; f += FU) {
            float s[FU];
            bool h[FU], any = false;
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                const float4 a = ca[(f + u) * CT + ti], b = cb[(f + u) * CT + tj];
                s[u] = dist2(a.x, a.y, a.z, b.x, b.y, b.z);
                h[u] = s[u] >= lo && s[u] < hi;
                any |= h[u];
            }
            if (!__any(any)) continue;
            int l[FU];
#pragma unroll
            for (int u = 0; u < FU; ++u) l[u] = 0;
            for (int step = top; step > 0; step >>= 1) {
#pragma unroll
                for (int u = 0; u < FU; ++u) search_step(thr, step, s[u], l[u]);
            }
#pragma unroll
            for (int u = 0; u < FU; ++u)
                if (h[u]) lds_count(cnt + l[u] * NT + tid);
        }
    }
    __syncthreads();
    // row i0 + r of the output holds nb * B contiguous counts of this tile
    for (int r = 0; r < na; ++r) {
        unsigned* o = counts + ((size_t)(i0 + r) * Nb + j0) * B;
        for (int e = tid; e < nb * B; e += NT) {
            const unsigned v = cnt[(e % B) * NT + r * CT + e / B];
            if (splits == 1) o[e] = v;
            else if (v) atomicAdd(o + e, v);
        }
    }
}

// P = float32(count) / (float32(sum of the pair's counts) + 1e-6f): the reference's float32 normalisation (its sums are integers below 2^24,
// hence exact), the division correctly rounded
__global__ __launch_bounds__(NT) void k_contact_normalise(size_t n_pairs, int B, const unsigned* __restrict__ counts, float* __restrict__ P) {
    const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
    if (p >= n_pairs) return;
    const unsigned* c = counts + p * B;
    unsigned sum = 0u;
    for (int b = 0; b < B; ++b) sum += c[b];
    const float den = __fadd_rn((float)sum, 1e-6f);
    for (int b = 0; b < B; ++b) P[p * B + b] = __fdiv_rn((float)c[b], den);
}

// replaces: StatisticalContactsModel.loglikelihood's frame loop (statistical_contacts_model.py:47-75). A workgroup owns LT x LT atom pairs
// of LF frames: lane = frame (coordinates in LDS as [component][frame], conflict-free), wave w the tile rows w, w + 4, ...; every lane adds
// the terms of its frame in a fixed order in double, the four waves are added in turn and the tile's partial goes to part[tile][frame].
// The terms that are not log(1) = 0 are the hits: log(1 - P + floor(P)) evaluated in double from the float32 P.
__global__ __launch_bounds__(NT) void k_contact_loglik(int F, int Na, int Nb, const float* __restrict__ x0, const float* __restrict__ x1, int B,
                                                       int top, const float* __restrict__ sq, const float* __restrict__ P, double* __restrict__ part,
                                                       int tiles_j, int tiles_ij) {
    extern __shared__ float4 lds_q[];
    float* ca = (float*)lds_q;              // [LT * 3][LPAD]
    float* cb = ca + LT * 3 * LPAD;         // [LT * 3][LPAD]
    float* thr = cb + LT * 3 * LPAD;        // [2 * top]
    __shared__ double red[NT / 64][LF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = (int)(blockIdx.x % (unsigned)tiles_ij), chunk = (int)(blockIdx.x / (unsigned)tiles_ij);
    const int i0 = (tile / tiles_j) * LT, j0 = (tile % tiles_j) * LT;
    const int na = min(LT, Na - i0), nb = min(LT, Nb - j0);
    const int f0 = chunk * LF, nf = min(LF, F - f0);
    for (int k = tid; k < 2 * top; k += NT) thr[k] = k <= B ? sq[k] : INFINITY;
    for (int idx = tid; idx < LF * LT * 3; idx += NT) {     // (NaN beyond the last frame and atom: never in a bin)
        const int f = idx / (LT * 3), k = idx % (LT * 3);
        ca[k * LPAD + f] = (f < nf && k < na * 3) ? x0[((size_t)(f0 + f) * Na + i0) * 3 + k] : NAN;
        cb[k * LPAD + f] = (f < nf && k < nb * 3) ? x1[((size_t)(f0 + f) * Nb + j0) * 3 + k] : NAN;
    }
    __syncthreads();
    const float lo = thr[0], hi = sq[B];
    double acc = 0.0;
    for (int i = w; i < na; i += NT / 64) {
        const float ax = ca[(i * 3) * LPAD + lane], ay = ca[(i * 3 + 1) * LPAD + lane], az = ca[(i * 3 + 2) * LPAD + lane];
        const float* prow = P + ((size_t)(i0 + i) * Nb + j0) * B;
        for (int j = 0; j < nb; j += JU) {                  // (LT is a multiple of JU; the atoms beyond nb are NaN)
            float s[JU];
            bool h[JU], any = false;
#pragma unroll
            for (int u = 0; u < JU; ++u) {
                const int k = (j + u) * 3;
                s[u] = dist2(ax, ay, az, cb[k * LPAD + lane], cb[(k + 1) * LPAD + lane], cb[(k + 2) * LPAD + lane]);
                h[u] = s[u] >= lo && s[u] < hi;
                any |= h[u];
            }
            if (!__any(any)) continue;
            int l[JU];
#pragma unroll
            for (int u = 0; u < JU; ++u) l[u] = 0;
            for (int step = top; step > 0; step >>= 1) {
#pragma unroll
                for (int u = 0; u < JU; ++u) search_step(thr, step, s[u], l[u]);
            }
#pragma unroll
            for (int u = 0; u < JU; ++u)
                if (h[u]) {
                    const double p = (double)prow[(size_t)(j + u) * B + l[u]];
                    acc += log(1.0 - p + floor(p));
                }
        }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && lane < nf) part[(size_t)tile * F + f0 + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// L[f] = -(sum of the tiles' partials, in tile order) / (Na * Nb * B)
__global__ __launch_bounds__(NT) void k_contact_loglik_finish(int F, int tiles_ij, double n_terms, const double* __restrict__ part, float* __restrict__ L) {
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    for (int t = 0; t < tiles_ij; ++t) s += part[(size_t)t * F + f];
    L[f] = (float)(-s / n_terms);
}

// replaces: div_KL (statistical_contacts_model.py:78-81), evaluated in double from the float32 inputs
__global__ __launch_bounds__(NT) void k_contact_div_kl(size_t n_pairs, int B, const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ D) {
    const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
    if (k >= n_pairs) return;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const double p = (double)P[k * B + b], q = (double)Q[k * B + b];
        double r = q / (p + (double)1e-6f);
        if (r < (double)1e-6f) r = 1.0;
        acc += p * log(r);
    }
    D[k] = (float)(-acc);
}

// ---- residue contact maps
// replaces: the residue-pair double loop of fnat (md_analysis/mdtraj_utils/trajectory_utils.py:369-379). One workgroup row per frame: the
// frame's atoms, gathered in residue order (perm / off), sit in LDS; a thread owns a residue pair and stops at its first contact.
__global__ __launch_bounds__(NT) void k_residue_maps(int Na, int Nb, int Ra, int Rb, const float* __restrict__ xa, const float* __restrict__ xb,
                                                     const int* __restrict__ perm_a, const int* __restrict__ perm_b, const int* __restrict__ off_a,
                                                     const int* __restrict__ off_b, float s_star, unsigned char* __restrict__ maps, int ysplit) {
    extern __shared__ float4 lds_q[];
    float* A = (float*)lds_q;           // [Na][3]
    float* Bc = A + (size_t)Na * 3;     // [Nb][3]
    const int f = (int)(blockIdx.x / (unsigned)ysplit), y = (int)(blockIdx.x % (unsigned)ysplit);
    for (int k = threadIdx.x; k < Na; k += NT) {
        const float* s = xa + ((size_t)f * Na + perm_a[k]) * 3;
        A[3 * k] = s[0]; A[3 * k + 1] = s[1]; A[3 * k + 2] = s[2];
    }
    for (int k = threadIdx.x; k < Nb; k += NT) {
        const float* s = xb + ((size_t)f * Nb + perm_b[k]) * 3;
        Bc[3 * k] = s[0]; Bc[3 * k + 1] = s[1]; Bc[3 * k + 2] = s[2];
    }
    __syncthreads();
    const int n_pairs = Ra * Rb;
    for (int p = y * NT + (int)threadIdx.x; p < n_pairs; p += ysplit * NT) {
        const int r = p / Rb, s = p % Rb;
        const int a0 = off_a[r], a1 = off_a[r + 1], b0 = off_b[s], b1 = off_b[s + 1];
        bool hit = false;
        for (int i = a0; i < a1 && !hit; ++i) {
            const float ax = A[3 * i], ay = A[3 * i + 1], az = A[3 * i + 2];
            for (int j = b0; j < b1; ++j)
                if (dist2(ax, ay, az, Bc[3 * j], Bc[3 * j + 1], Bc[3 * j + 2]) < s_star) { hit = true; break; }
        }
        maps[(size_t)f * n_pairs + p] = hit ? 1 : 0;
    }
}

// out[f] = number of k < n with a[f * n + k] and b[f * stride_b + k] both non-zero (one workgroup per frame; integer sums)
__global__ __launch_bounds__(NT) void k_and_count(int n, const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, size_t stride_b,
                                                  long long* __restrict__ out) {
    __shared__ int wsum[NT / 64];
    const size_t f = blockIdx.x;
    int c = 0;
    for (int k = threadIdx.x; k < n; k += NT) c += (a[f * n + k] != 0 && b[f * stride_b + k] != 0) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[f] = (long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// out[0] = sum of in[0 .. n) (one workgroup)
__global__ __launch_bounds__(NT) void k_sum_i64(int n, const long long* __restrict__ in, long long* __restrict__ out) {
    __shared__ long long wsum[NT / 64];
    long long c = 0;
    for (int k = threadIdx.x; k < n; k += NT) c += in[k];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- superposition (kabsch_fit, moved and moved_deviation of pesto_fit.h, shared with pesto_docking.hip and pesto_dockq.hip)
// replaces: superpose_transform and the rmsd expression (trajectory_utils.py:190-207, 308-325). One workgroup per frame over the n_sel
// selected atoms, which may differ on the two sides: the fit without the identity short cut (a frame that is the reference gets its
// rotation within rounding of I, as it always has), then the deviation of the transformed selection from the reference's. tr [F] keeps
// the fit (t, R, t_ref in double) for k_superpose_apply.
__global__ __launch_bounds__(NT) void k_superpose_fit(int Fr, int Nr, int N, int n_sel, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                      const int* __restrict__ sel_ref, const int* __restrict__ sel, Fit* __restrict__ tr,
                                                      float* __restrict__ t_out, float* __restrict__ R_out, float* __restrict__ tref_out,
                                                      float* __restrict__ rmsd, double scale) {
    __shared__ double red[NT / 64];
    __shared__ double sR[9];
    const size_t f = blockIdx.x;
    const float* X = xyz + f * (size_t)N * 3;
    const float* Y = ref + (Fr == 1 ? 0 : f) * (size_t)Nr * 3;
    const auto px = atoms<true>(X, sel), py = atoms<true>(Y, sel_ref);
    Fit ft;
    kabsch_fit<NT, false>(px, py, n_sel, red, sR, ft);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 9; ++c) R_out[f * 9 + c] = (float)ft.R[c];
        for (int c = 0; c < 3; ++c) {
            t_out[f * 3 + c] = (float)ft.m[c];
            if (Fr != 1 || f == 0) tref_out[f * 3 + c] = (float)ft.m[3 + c];
        }
        tr[f] = ft;
    }
    const double dev = moved_deviation<NT>(px, py, n_sel, ft, red);
    if (threadIdx.x == 0) rmsd[f] = (float)(sqrt(dev / (double)n_sel) * scale);
}

// out[f, n, :] = (xyz[f, n, :] - t[f]) R[f] + t_ref[f], in double from the fit's double t, R, t_ref
__global__ __launch_bounds__(NT) void k_superpose_apply(size_t total, int N, const float* __restrict__ xyz, const Fit* __restrict__ tr, float* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
    if (k >= total) return;
    const double x[3] = {(double)xyz[3 * k], (double)xyz[3 * k + 1], (double)xyz[3 * k + 2]};
    double p[3];
    moved(x, tr[k / (size_t)N], p);
    for (int c = 0; c < 3; ++c) out[3 * k + c] = (float)p[c];
}

// replaces: Xp = X M / count of md_analysis/apply_model_md.ipynb. One thread per (frame, residue): its atoms (perm, in atom order) summed in double
__global__ __launch_bounds__(NT) void k_residue_centroids(size_t total, int N, int R, const float* __restrict__ X, const int* __restrict__ perm,
                                                          const int* __restrict__ off, float* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
    if (k >= total) return;
    const size_t f = k / (size_t)R;
    const int r = (int)(k % (size_t)R);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int a0 = off[r], a1 = off[r + 1];
    for (int a = a0; a < a1; ++a) {
        const float* x = X + (f * (size_t)N + perm[a]) * 3;
        s0 += (double)x[0]; s1 += (double)x[1]; s2 += (double)x[2];
    }
    const double n = (double)(a1 - a0);
    out[3 * k] = (float)(s0 / n); out[3 * k + 1] = (float)(s1 / n); out[3 * k + 2] = (float)(s2 / n);
}

// ---- host side
int pow2_floor(int B) { int t = 1; while (2 * t <= B) t *= 2; return t; }

// the squared-distance thresholds of the bin edges: d >= edge  <=>  s >= sq, for every float32 s = d * d summed as dist2 does.
// (an edge beyond the float32 range is refused: +inf could not tell d = inf from it)
int edge_thresholds(int B, const double* edges, std::vector<float>& sq) {
    sq.resize((size_t)B + 1);
    for (int b = 0; b <= B; ++b) {
        const double e = edges[b];
        if (!std::isfinite(e) || std::fabs(e) > 3.4028234663852886e38) return fail(PESTO_ERR_INVALID, "bins[%d] is not a finite float32-range edge", b);
        if (b && !(edges[b] > edges[b - 1])) return fail(PESTO_ERR_INVALID, "bins must increase strictly (bins[%d])", b);
        float e32 = (float)e;               // round to nearest, then up to the smallest float32 not below e
        if ((double)e32 < e) e32 = std::nextafter(e32, INFINITY);
        sq[b] = first_true([e32](float s) { return sqrt_rn(s) >= e32; });
    }
    return 0;
}

int check_pairs(int64_t F, int64_t Na, int64_t Nb, int B) {
    if (F < 1 || F > PESTO_TRAJECTORY_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to 2^24 frames, got %lld", (long long)F);
    if (B < 1 || B > PESTO_TRAJECTORY_MAX_BINS) return fail(PESTO_ERR_INVALID, "1 to %d bins, got %d", PESTO_TRAJECTORY_MAX_BINS, B);
    if (Na < 1 || Nb < 1 || Na > 0x7fffffff || Nb > 0x7fffffff || Na * Nb > 0x7fffffff || Na * Nb * B > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "Na * Nb * bins must be in 1 .. 2^31 - 1 (Na = %lld, Nb = %lld)", (long long)Na, (long long)Nb);
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_trajectory_last_error(void) { return last_error(); }

int pesto_contact_counts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t n_bins,
                         const double* edges, uint32_t* counts_out, float* P_out, int32_t frame_splits, int32_t ptr_kind, void* stream) {
    if (!xyz_a || !xyz_b || !edges || !counts_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_pairs(F, Na, Nb, n_bins)) return rc;
    if (frame_splits < 0) return fail(PESTO_ERR_INVALID, "frame_splits must be 0 (chosen per call) or positive");
    std::vector<float> sq;
    if (int rc = edge_thresholds(n_bins, edges, sq)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const int B = n_bins;
    const int64_t tiles_i = (Na + CT - 1) / CT, tiles_j = (Nb + CT - 1) / CT, tiles = tiles_i * tiles_j;
    const int64_t chunks = (F + CF - 1) / CF;
    // an interface-sized problem has too few tiles for the device: split the frames until some thousands of workgroups exist
    int64_t splits = frame_splits ? frame_splits : (4096 + tiles - 1) / tiles;
    splits = std::max<int64_t>(1, std::min(splits, chunks));
    const int64_t per_split = (chunks + splits - 1) / splits * CF;
    splits = (F + per_split - 1) / per_split;
    if (tiles * splits > 0x7fffffff) return fail(PESTO_ERR_INVALID, "too many workgroups (%lld tiles x %lld frame splits)", (long long)tiles, (long long)splits);
    Buffers bf(ptr_kind, stream);
    const size_t n_out = (size_t)(Na * Nb) * B;
    const int iA = bf.input(xyz_a, (size_t)F * Na * 12), iB = xyz_b == xyz_a ? iA : bf.input(xyz_b, (size_t)F * Nb * 12);
    const int iS = bf.table(sq.data(), sq.size() * 4), iC = bf.output(counts_out, n_out * 4, splits > 1 ? 0 : -1),
              iP = bf.output(P_out, n_out * 4);               // (split frames add their counts up)
    int rc = bf.upload();
    if (rc == 0) {
        const int top = pow2_floor(B);
        const size_t smem = 2 * (size_t)CF * CT * 16 + (size_t)B * NT * 4 + 2 * (size_t)top * 4;
        unsigned* cnt = bf.ptr<unsigned>(iC);
        rc = hip_ok(hipFuncSetAttribute((const void*)k_contact_counts, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "contact_counts");
        if (rc == 0) {
            hipLaunchKernelGGL(k_contact_counts, dim3((unsigned)(tiles * splits)), dim3(NT), smem, bf.stm, (int)F, (int)Na, (int)Nb,
                               bf.ptr<const float>(iA), bf.ptr<const float>(iB), B, top, bf.ptr<const float>(iS), cnt, (int)tiles_j, (int)tiles, (int)splits,
                               (int)per_split);
            if (P_out)
                hipLaunchKernelGGL(k_contact_normalise, dim3((unsigned)((Na * Nb + NT - 1) / NT)), dim3(NT), 0, bf.stm, (size_t)(Na * Nb), B, cnt,
                                   bf.ptr<float>(iP));
        }
    }
    return bf.finish(rc, "contact_counts");
}

int pesto_contact_loglik(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t n_bins,
                         const double* edges, const float* P, float* L_out, int32_t ptr_kind, void* stream) {
    if (!xyz_a || !xyz_b || !edges || !P || !L_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_pairs(F, Na, Nb, n_bins)) return rc;
    std::vector<float> sq;
    if (int rc = edge_thresholds(n_bins, edges, sq)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const int B = n_bins;
    const int64_t tiles_i = (Na + LT - 1) / LT, tiles_j = (Nb + LT - 1) / LT, tiles = tiles_i * tiles_j;
    // the tiles' partials (one double per tile and frame) live in a scratch of at most LOGLIK_SCRATCH bytes (or one LF-frame chunk, if
    // that is larger): the frames go through the two kernels in passes of `pass` frames, whatever F is
    const int64_t pass = std::min<int64_t>((F + LF - 1) / LF * LF, std::max<int64_t>(LF, LOGLIK_SCRATCH / (tiles * 8) / LF * LF));
    if (tiles * (pass / LF) > 0x7fffffff) return fail(PESTO_ERR_INVALID, "too many workgroups (%lld tiles)", (long long)tiles);
    Buffers bf(ptr_kind, stream);
    const int iA = bf.input(xyz_a, (size_t)F * Na * 12), iB = xyz_b == xyz_a ? iA : bf.input(xyz_b, (size_t)F * Nb * 12);
    const int iS = bf.table(sq.data(), sq.size() * 4), iP = bf.input(P, (size_t)(Na * Nb) * B * 4), iL = bf.output(L_out, (size_t)F * 4);
    const int iW = bf.scratch((size_t)tiles * pass * 8);
    int rc = bf.upload();
    if (rc == 0) {
        const int top = pow2_floor(B);
        const size_t smem = (2 * (size_t)LT * 3 * LPAD + 2 * (size_t)top) * 4;
        rc = hip_ok(hipFuncSetAttribute((const void*)k_contact_loglik, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "contact_loglik");
        for (int64_t f0 = 0; rc == 0 && f0 < F; f0 += pass) {
            const int64_t nf = std::min(pass, F - f0), chunks = (nf + LF - 1) / LF;
            hipLaunchKernelGGL(k_contact_loglik, dim3((unsigned)(tiles * chunks)), dim3(NT), smem, bf.stm, (int)nf, (int)Na, (int)Nb,
                               bf.ptr<const float>(iA) + (size_t)f0 * Na * 3, bf.ptr<const float>(iB) + (size_t)f0 * Nb * 3, B, top, bf.ptr<const float>(iS),
                               bf.ptr<const float>(iP), bf.ptr<double>(iW), (int)tiles_j, (int)tiles);
            hipLaunchKernelGGL(k_contact_loglik_finish, dim3((unsigned)((nf + NT - 1) / NT)), dim3(NT), 0, bf.stm, (int)nf, (int)tiles,
                               (double)Na * (double)Nb * (double)B, bf.ptr<const double>(iW), bf.ptr<float>(iL) + f0);
        }
    }
    return bf.finish(rc, "contact_loglik");
}

int pesto_contact_div_kl(pesto_model* m, int64_t n_pairs, int32_t n_bins, const float* P, const float* Q, float* D_out, int32_t ptr_kind,
                         void* stream) {
    if (!P || !Q || !D_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (n_pairs < 1 || n_bins < 1 || n_pairs > 0x7fffffff || n_pairs * n_bins > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "n_pairs * n_bins must be in 1 .. 2^31 - 1");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const size_t n = (size_t)n_pairs * n_bins * 4;
    const int iP = bf.input(P, n), iQ = Q == P ? iP : bf.input(Q, n), iD = bf.output(D_out, (size_t)n_pairs * 4);
    int rc = bf.upload();
    if (rc == 0)
        hipLaunchKernelGGL(k_contact_div_kl, dim3((unsigned)((n_pairs + NT - 1) / NT)), dim3(NT), 0, bf.stm, (size_t)n_pairs, n_bins, bf.ptr<const float>(iP),
                           bf.ptr<const float>(iQ), bf.ptr<float>(iD));
    return bf.finish(rc, "contact_div_kl");
}

int pesto_residue_contact_maps(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t Ra, int32_t Rb,
                               const int32_t* perm_a, const int32_t* off_a, const int32_t* perm_b, const int32_t* off_b, float r_thr, float scale,
                               uint8_t* maps_out, int32_t ptr_kind, void* stream) {
    if (!xyz_a || !xyz_b || !perm_a || !off_a || !perm_b || !off_b || !maps_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > 0x7fffffff || Na < 1 || Nb < 1 || Na + Nb > PESTO_TRAJECTORY_MAX_MAP_ATOMS)
        return fail(PESTO_ERR_INVALID, "F >= 1 frames and 1 <= Na, Nb with Na + Nb <= %d atoms", PESTO_TRAJECTORY_MAX_MAP_ATOMS);
    if (Ra < 1 || Rb < 1 || Ra > Na || Rb > Nb || (int64_t)Ra * Rb > 0x7fffffff) return fail(PESTO_ERR_INVALID, "1 <= Ra <= Na and 1 <= Rb <= Nb residues");
    if (!std::isfinite(r_thr) || !std::isfinite(scale) || !(scale > 0.f)) return fail(PESTO_ERR_INVALID, "r_thr must be finite and scale positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    // contact  <=>  fl(sqrt_rn(s) * scale) < r_thr  <=>  s < s_star (the product is monotonic in s)
    const float s_star = first_true([r_thr, scale](float s) { volatile float d = sqrt_rn(s) * scale; return !(d < r_thr); });
    const int64_t n_pairs = (int64_t)Ra * Rb;
    int64_t ysplit = std::max<int64_t>(1, std::min<int64_t>((n_pairs + NT - 1) / NT, (2048 + F - 1) / F));
    if (F * ysplit > 0x7fffffff) return fail(PESTO_ERR_INVALID, "too many workgroups");
    Buffers bf(ptr_kind, stream);
    const int iA = bf.input(xyz_a, (size_t)F * Na * 12), iB = bf.input(xyz_b, (size_t)F * Nb * 12);
    const int iPa = bf.input(perm_a, (size_t)Na * 4), iOa = bf.input(off_a, ((size_t)Ra + 1) * 4), iPb = bf.input(perm_b, (size_t)Nb * 4),
              iOb = bf.input(off_b, ((size_t)Rb + 1) * 4), iM = bf.output(maps_out, (size_t)F * n_pairs);
    int rc = bf.upload();
    if (rc == 0) {
        const size_t smem = (size_t)(Na + Nb) * 12;
        rc = hip_ok(hipFuncSetAttribute((const void*)k_residue_maps, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), "residue_contact_maps");
        if (rc == 0)
            hipLaunchKernelGGL(k_residue_maps, dim3((unsigned)(F * ysplit)), dim3(NT), smem, bf.stm, (int)Na, (int)Nb, Ra, Rb, bf.ptr<const float>(iA),
                               bf.ptr<const float>(iB), bf.ptr<const int>(iPa), bf.ptr<const int>(iPb), bf.ptr<const int>(iOa), bf.ptr<const int>(iOb), s_star,
                               bf.ptr<unsigned char>(iM), (int)ysplit);
    }
    return bf.finish(rc, "residue_contact_maps");
}

int pesto_native_contacts(pesto_model* m, int64_t F, int64_t F_ref, int64_t n, const uint8_t* maps_ref, const uint8_t* maps, int64_t* native_out,
                          int64_t* ref_total_out, int32_t ptr_kind, void* stream) {
    if (!maps_ref || !maps || !native_out || !ref_total_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > 0x7fffffff || (F_ref != 1 && F_ref != F) || n < 1 || n > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "F >= 1 frames, F_ref = 1 or F, 1 <= n < 2^31 residue pairs");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iR = bf.input(maps_ref, (size_t)F_ref * n), iM = bf.input(maps, (size_t)F * n), iN = bf.output(native_out, (size_t)F * 8),
              iT = bf.output(ref_total_out, 8), iW = bf.scratch((size_t)F_ref * 8);
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_and_count, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)n, bf.ptr<const unsigned char>(iM), bf.ptr<const unsigned char>(iR),
                           F_ref == 1 ? (size_t)0 : (size_t)n, bf.ptr<long long>(iN));
        hipLaunchKernelGGL(k_and_count, dim3((unsigned)F_ref), dim3(NT), 0, bf.stm, (int)n, bf.ptr<const unsigned char>(iR), bf.ptr<const unsigned char>(iR),
                           (size_t)n, bf.ptr<long long>(iW));
        hipLaunchKernelGGL(k_sum_i64, dim3(1), dim3(NT), 0, bf.stm, (int)F_ref, bf.ptr<const long long>(iW), bf.ptr<long long>(iT));
    }
    return bf.finish(rc, "native_contacts");
}

int pesto_superpose(pesto_model* m, int64_t F, int64_t F_ref, int64_t N_ref, int64_t N, int64_t n_sel, const float* xyz_ref, const float* xyz,
                    const int32_t* sel_ref, const int32_t* sel, double scale, float* t_out, float* R_out, float* t_ref_out, float* xyz_out,
                    float* rmsd_out, int32_t ptr_kind, void* stream) {
    if (!xyz_ref || !xyz || !t_out || !R_out || !t_ref_out || !rmsd_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > 0x7fffffff || (F_ref != 1 && F_ref != F) || N < 1 || N_ref < 1 || N > 0x7fffffff || N_ref > 0x7fffffff || n_sel < 3 ||
        (!sel && n_sel != N) || (!sel_ref && n_sel != N_ref) || n_sel > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "F >= 1 frames, F_ref = 1 or F, at least 3 selected atoms on both sides (all atoms without a selection)");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)F_ref * N_ref * 12), iX = bf.input(xyz, (size_t)F * N * 12);
    const int iSr = bf.input(sel_ref, (size_t)n_sel * 4), iS = bf.input(sel, (size_t)n_sel * 4);
    const int it = bf.output(t_out, (size_t)F * 12), iR = bf.output(R_out, (size_t)F * 36), itr = bf.output(t_ref_out, (size_t)F_ref * 12),
              iO = bf.output(xyz_out, (size_t)F * N * 12), iD = bf.output(rmsd_out, (size_t)F * 4), iW = bf.scratch((size_t)F * sizeof(Fit));
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_superpose_fit, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)F_ref, (int)N_ref, (int)N, (int)n_sel, bf.ptr<const float>(iY),
                           bf.ptr<const float>(iX), sel_ref ? bf.ptr<const int>(iSr) : nullptr, sel ? bf.ptr<const int>(iS) : nullptr, bf.ptr<Fit>(iW),
                           bf.ptr<float>(it), bf.ptr<float>(iR), bf.ptr<float>(itr), bf.ptr<float>(iD), scale);
        if (xyz_out) {
            const size_t total = (size_t)F * N;
            hipLaunchKernelGGL(k_superpose_apply, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, bf.stm, total, (int)N, bf.ptr<const float>(iX),
                               bf.ptr<const Fit>(iW), bf.ptr<float>(iO));
        }
    }
    return bf.finish(rc, "superpose");
}

int pesto_residue_centroids(pesto_model* m, int64_t F, int64_t N, int64_t R, const float* X_frames, const int32_t* perm, const int32_t* off,
                            float* out, int32_t ptr_kind, void* stream) {
    if (!X_frames || !perm || !off || !out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || N < 1 || R < 1 || N > 0x7fffffff || R > 0x7fffffff || F * R > (int64_t)0x7fffffff * NT)
        return fail(PESTO_ERR_INVALID, "F, N, R >= 1 and F * R below 2^39");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(X_frames, (size_t)F * N * 12), iP = bf.input(perm, (size_t)N * 4), iO = bf.input(off, ((size_t)R + 1) * 4),
              iC = bf.output(out, (size_t)F * R * 12);
    int rc = bf.upload();
    if (rc == 0) {
        const size_t total = (size_t)F * R;
        hipLaunchKernelGGL(k_residue_centroids, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, bf.stm, total, (int)N, (int)R, bf.ptr<const float>(iX),
                           bf.ptr<const int>(iP), bf.ptr<const int>(iO), bf.ptr<float>(iC));
    }
    return bf.finish(rc, "residue_centroids");
}
