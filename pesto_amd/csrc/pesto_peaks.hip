// pesto_peaks.hip - density-peak clustering of MD frames by the centre of their predicted interface: steps 3 to 5 of the clustering in
// the reference's notebooks (md_analysis/apply_model_with_clustering.ipynb, cell lines 263-343, and clustering_analysis.ipynb). The
// notebooks hand the interface centres to CLoNe, a third-party package that the reference does not contain; CLoNe is NOT reproduced
// here. What stands in its place is the published algorithm it derives from, density peaks (Rodriguez and Laio, Science 344, 2014), in
// full: the d_c percentile, the cut-off or the Gaussian kernel, delta and the nearest denser point, centre selection, label propagation
// and the halo. It runs over points (matrix-free) or over a precomputed distance matrix such as pesto_pairwise_rmsd's.
//
// weighted_centers    k_pk_centers  one workgroup per frame, two passes over the frame's residues, every sum in double (block_sum)
// pair_distance_rank  k_pairs<Src, Hist> + k_pk_select, three times: a radix select over the bit patterns of the non-negative float32
//                     distances of the pairs i < j, digits of 11, 10 and 10 bits; integer counts in LDS bins per workgroup, 64-bit totals
// density_peaks       k_pairs<Src, Density>, k_pairs<Src, Nearest>, k_pairs<None, Rank> twice, pointer jumping, k_pairs<Src, Border>
//
// k_pairs is the one all-pairs skeleton, templated over the distance source (points staged in LDS, 4 or 8 floats per point, the unused
// dimensions zero, which leaves the ascending float32 sum unchanged; rows of D; or none) and over the per-pair action. Tile edges: a
// workgroup of 256 threads owns TI = 64 rows i and walks the j tiles of TJ = 256 columns; lane r of wave q holds row r and takes columns
// 64 q .. 64 q + 63 of every tile in ascending order; the four partials of a row combine as (p0 + p1) + (p2 + p3). Every action's
// combination is either that fixed tree or order-independent (integer counts, lexicographic minima, maxima), so every output is
// bit-identical from call to call. The matrix source reads D[j, i] for the pair (i, j), rows across lanes: D is checked to be bitwise
// symmetric first. No floating-point atomics anywhere; nothing of size [n, n] is allocated.
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_geom.h"

namespace pesto {
namespace {

constexpr int NT = 256;
constexpr int TI = 64;              // rows of a workgroup
constexpr int TJ = 256;             // columns of a tile
constexpr int NQ = NT / TI;         // column slices of a tile, one per wave
constexpr int MAX_BINS = 2048;      // the widest digit of the radix select: 11 bits
static_assert(TJ == NT && TI == 64 && NQ == 4, "one staged column per thread, one row per lane, four partials per row");

enum { ST_ERR = 0, ST_DENSEST = 1, ST_CENTRES = 2, ST_WORDS = 4 };
enum { E_NONFINITE = 1, E_ASYM = 2, E_NEGATIVE = 4, E_INDEX = 8, E_WEIGHT = 16, E_RANK = 32 };

struct Lds { float* tile; double* aux; int* lab; int* bins; };

// ---- distance sources
template <int DP> struct Points {
    const float* P;             // [n, DP]: the selected points, dimensions beyond d zero
    struct Row { float x[DP]; };
    __device__ Row row(int i, bool valid) const {
        Row r;
#pragma unroll
        for (int c = 0; c < DP; ++c) r.x[c] = valid ? P[(size_t)i * DP + c] : 0.f;
        return r;
    }
    __device__ void stage(const Lds& L, int j0, int n) const {
        for (int e = threadIdx.x; e < TJ * DP; e += NT) L.tile[e] = j0 + e / DP < n ? P[(size_t)j0 * DP + e] : 0.f;
    }
    // float32, no contraction, dimensions added in ascending order; the root correctly rounded
    __device__ float dist(const Row& r, const Lds& L, int jj) const {
#pragma clang fp contract(off)
        const float* p = L.tile + jj * DP;
        float dx = __fsub_rn(r.x[0], p[0]);
        float s = __fmul_rn(dx, dx);
#pragma unroll
        for (int c = 1; c < DP; ++c) {
            dx = __fsub_rn(r.x[c], p[c]);
            s = __fadd_rn(s, __fmul_rn(dx, dx));
        }
        return sqrtf(s);
    }
};

struct Matrix {
    const float* D;             // [F, F], bitwise symmetric
    int F;
    const int* idx;             // the selected rows, or nullptr
    struct Row { int col; };
    __device__ Row row(int i, bool valid) const { return Row{valid ? (idx ? idx[i] : i) : 0}; }
    __device__ void stage(const Lds& L, int j0, int n) const {
        const int j = j0 + threadIdx.x;
        ((int*)L.tile)[threadIdx.x] = j < n ? (idx ? idx[j] : j) : 0;
    }
    // D[j, i] = D[i, j]: consecutive lanes read consecutive addresses; -0 counts as +0
    __device__ float dist(const Row& r, const Lds& L, int jj) const {
        return __uint_as_float(__float_as_uint(D[(size_t)((const int*)L.tile)[jj] * F + r.col]) & 0x7fffffffu);
    }
};

struct None {
    struct Row {};
    __device__ Row row(int, bool) const { return Row{}; }
    __device__ void stage(const Lds&, int, int) const {}
    __device__ float dist(const Row&, const Lds&, int) const { return 0.f; }
};

// ---- the skeleton. An action brings: Part (a row's partial), init(i, valid), first_tile(i0), stage (its per-column values into L.aux /
// L.lab), pair(part, i, j, d, L, jj), combine(a, b), finish(i, part), and begin / end around the walk (the histogram's LDS bins).
template <class Src, class Act>
__global__ __launch_bounds__(NT) void k_pairs(Src src, Act act, int n) {
    __shared__ float tile[TJ * 8];
    __shared__ double aux[TJ];
    __shared__ int lab[TJ];
    __shared__ int bins[Act::BINS ? Act::BINS : 1];
    __shared__ typename Act::Part part[NT];
    const Lds L{tile, aux, lab, bins};
    const int r = threadIdx.x & (TI - 1), q = threadIdx.x / TI;
    const int i = blockIdx.x * TI + r;
    const bool valid = i < n;
    const typename Src::Row row = src.row(i, valid);
    typename Act::Part p = act.init(i, valid);
    act.begin(L);
    for (int j0 = act.first_tile(blockIdx.x * TI); j0 < n; j0 += TJ) {
        __syncthreads();
        src.stage(L, j0, n);
        act.stage(L, j0, n);
        __syncthreads();
        const int jend = min(TI * q + TI, n - j0);          // the last tile is partial
        if (valid)
            for (int jj = TI * q; jj < jend; ++jj) act.pair(p, i, j0 + jj, src.dist(row, L, jj), L, jj);
    }
    part[threadIdx.x] = p;
    __syncthreads();
    act.end(L);
    if (q == 0 && valid) act.finish(i, act.combine(act.combine(part[r], part[TI + r]), act.combine(part[2 * TI + r], part[3 * TI + r])));
}

struct ActBase {
    static constexpr int BINS = 0;
    __device__ int first_tile(int) const { return 0; }
    __device__ void begin(const Lds&) const {}
    __device__ void end(const Lds&) const {}
    __device__ void stage(const Lds&, int, int) const {}
};

// key(j) > key(i): denser, the lower index first among equal densities
__device__ __forceinline__ bool denser(double rj, int j, double ri, int i) { return rj > ri || (rj == ri && j < i); }

// One digit of the radix select: the pairs i < j whose distance has the digits chosen so far, counted by the next digit.
struct Hist : ActBase {
    static constexpr int BINS = MAX_BINS;
    unsigned long long* g;                  // [nbins] totals
    const unsigned long long* kst;          // kst[1]: the digits chosen so far
    unsigned mask;                          // their bits
    int shift, nbins;
    struct Part { unsigned prefix; };
    __device__ Part init(int, bool) const { return Part{(unsigned)kst[1]}; }
    __device__ int first_tile(int i0) const { return i0 / TJ * TJ; }
    __device__ void begin(const Lds& L) const {
        for (int b = threadIdx.x; b < nbins; b += NT) L.bins[b] = 0;
    }
    __device__ void pair(Part& p, int i, int j, float d, const Lds& L, int) const {
        const unsigned u = __float_as_uint(d);
        if (j > i && (u & mask) == p.prefix) atomicAdd(&L.bins[(u >> shift) & (unsigned)(nbins - 1)], 1);
    }
    __device__ Part combine(const Part& a, const Part&) const { return a; }
    __device__ void finish(int, const Part&) const {}
    __device__ void end(const Lds& L) const {       // (after the barrier that follows the walk)
        for (int b = threadIdx.x; b < nbins; b += NT)
            if (L.bins[b]) atomicAdd(&g[b], (unsigned long long)L.bins[b]);
    }
};

// rho: the neighbours below d_c (strictly), or the Gaussian sum in double from the float32 d and d_c
template <bool GAUSS> struct Density : ActBase {
    float dc;
    double* rho;
    struct Part { double s; int c; };
    __device__ Part init(int, bool) const { return Part{0.0, 0}; }
    __device__ void pair(Part& p, int i, int j, float d, const Lds&, int) const {
        if (j == i) return;
        if (GAUSS) {
            const double a = (double)d / (double)dc;
            p.s += exp(-(a * a));
        } else {
            p.c += d < dc ? 1 : 0;
        }
    }
    __device__ Part combine(const Part& a, const Part& b) const { return Part{a.s + b.s, a.c + b.c}; }
    __device__ void finish(int i, const Part& p) const { rho[i] = GAUSS ? p.s : (double)p.c; }
};

// delta and the nearest denser point: the lexicographic minimum of (d, j) over the denser j; the largest d for the densest point
struct Nearest : ActBase {
    const double* rho;
    float* delta;
    int* nh;
    double* gamma;
    int* state;
    struct Part { double ri; float mind, maxd; int minj; };
    __device__ Part init(int i, bool valid) const { return Part{valid ? rho[i] : 0.0, INFINITY, 0.f, 0x7fffffff}; }
    __device__ void stage(const Lds& L, int j0, int n) const { L.aux[threadIdx.x] = j0 + (int)threadIdx.x < n ? rho[j0 + threadIdx.x] : 0.0; }
    __device__ void pair(Part& p, int i, int j, float d, const Lds& L, int jj) const {
        if (j == i) return;
        p.maxd = fmaxf(p.maxd, d);
        if (denser(L.aux[jj], j, p.ri, i) && (d < p.mind || (d == p.mind && j < p.minj))) { p.mind = d; p.minj = j; }
    }
    __device__ Part combine(const Part& a, const Part& b) const {
        const bool take_b = b.mind < a.mind || (b.mind == a.mind && b.minj < a.minj);
        return Part{a.ri, take_b ? b.mind : a.mind, fmaxf(a.maxd, b.maxd), take_b ? b.minj : a.minj};
    }
    __device__ void finish(int i, const Part& p) const {
        const bool top = p.minj == 0x7fffffff;              // no denser point: exactly one row, key being a total order
        const float dl = top ? p.maxd : p.mind;
        delta[i] = dl;
        nh[i] = top ? -1 : p.minj;
        gamma[i] = p.ri * (double)dl;
        if (top) state[ST_DENSEST] = i;
    }
};

// MODE 0: the centres of the n_clusters rule. The densest point, and the K - 1 others with the largest gamma (the lower index first among
//         equal ones): flag[i] = i is the densest or fewer than K - 1 others come before it.
// MODE 1: the centres in order of key: cidx[i] = the number of centres denser than centre i, centers[cidx[i]] = i.
template <int MODE> struct Rank : ActBase {
    const double* val;          // gamma / rho
    int* flag;
    int* cidx;
    int* centers;
    int* state;
    int K;
    struct Part { double vi; int cnt, top; };
    __device__ Part init(int i, bool valid) const { return Part{valid ? val[i] : 0.0, 0, MODE == 0 ? state[ST_DENSEST] : 0}; }
    __device__ void stage(const Lds& L, int j0, int n) const {
        const int j = j0 + threadIdx.x;
        L.aux[threadIdx.x] = j < n ? val[j] : 0.0;
        if (MODE == 1) L.lab[threadIdx.x] = j < n ? flag[j] : 0;
    }
    __device__ void pair(Part& p, int i, int j, float, const Lds& L, int jj) const {
        if (j == i) return;
        if (MODE == 0) p.cnt += j != p.top && denser(L.aux[jj], j, p.vi, i) ? 1 : 0;
        else p.cnt += L.lab[jj] && denser(L.aux[jj], j, p.vi, i) ? 1 : 0;
    }
    __device__ Part combine(const Part& a, const Part& b) const { return Part{a.vi, a.cnt + b.cnt, a.top}; }
    __device__ void finish(int i, const Part& p) const {
        if (MODE == 0) {
            flag[i] = i == p.top || p.cnt < K - 1 ? 1 : 0;
        } else if (flag[i]) {
            cidx[i] = p.cnt;
            centers[p.cnt] = i;
            atomicAdd(&state[ST_CENTRES], 1);
        } else {
            cidx[i] = -1;
        }
    }
};

// rho_b[c] = max over the pairs (i in c, j not in c, d < d_c) of (rho_i + rho_j) / 2: a row's maximum, then an integer atomicMax on the
// bits of the non-negative double
struct Border : ActBase {
    float dc;
    const double* rho;
    const int* labels;
    unsigned long long* rhob;
    struct Part { double ri, b; int li; };
    __device__ Part init(int i, bool valid) const { return Part{valid ? rho[i] : 0.0, 0.0, valid ? labels[i] : 0}; }
    __device__ void stage(const Lds& L, int j0, int n) const {
        const int j = j0 + threadIdx.x;
        L.aux[threadIdx.x] = j < n ? rho[j] : 0.0;
        L.lab[threadIdx.x] = j < n ? labels[j] : 0;
    }
    __device__ void pair(Part& p, int, int, float d, const Lds& L, int jj) const {
        if (L.lab[jj] != p.li && d < dc) p.b = fmax(p.b, (p.ri + L.aux[jj]) * 0.5);
    }
    __device__ Part combine(const Part& a, const Part& b) const { return Part{a.ri, fmax(a.b, b.b), a.li}; }
    __device__ void finish(int, const Part& p) const {
        if (p.b > 0.0 && p.li >= 0) atomicMax(&rhob[p.li], (unsigned long long)__double_as_longlong(p.b));
    }
};

// ---- the small kernels around the skeleton
// the selected points as [n, DP] with zero padding; an index outside [0, F) or a non-finite coordinate sets its error bit
__global__ __launch_bounds__(NT) void k_pk_gather(int F, int d, int DP, int n, const float* __restrict__ X, const int* __restrict__ idx, float* __restrict__ P,
                                                  int* __restrict__ state) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    int src = idx ? idx[i] : i;
    int err = 0;
    if (src < 0 || src >= F) { err |= E_INDEX; src = 0; }
    for (int c = 0; c < DP; ++c) {
        const float v = c < d ? X[(size_t)src * d + c] : 0.f;
        if (!isfinite(v)) err |= E_NONFINITE;
        P[(size_t)i * DP + c] = v;
    }
    if (err) atomicOr(&state[ST_ERR], err);
}

// one workgroup per row of D: off the diagonal finite and >= 0, and bitwise symmetric
__global__ __launch_bounds__(NT) void k_pk_check_matrix(int F, const float* __restrict__ D, int* __restrict__ state) {
    const int i = blockIdx.x;
    int err = 0;
    for (int j = threadIdx.x; j < F; j += NT) {
        if (j == i) continue;
        const float v = D[(size_t)i * F + j];
        if (!isfinite(v)) err |= E_NONFINITE;
        else if (!(v >= 0.f)) err |= E_NEGATIVE;
        if (j > i && __float_as_uint(v) != __float_as_uint(D[(size_t)j * F + i])) err |= E_ASYM;
    }
    if (err) atomicOr(&state[ST_ERR], err);
}

__global__ __launch_bounds__(NT) void k_pk_check_idx(int F, int n, const int* __restrict__ idx, int* __restrict__ state) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n && (idx[i] < 0 || idx[i] >= F)) atomicOr(&state[ST_ERR], E_INDEX);
}

// One workgroup: the bin that holds rank kst[0] becomes the next digit of kst[1], kst[0] the rank within it; the bins are cleared.
__global__ __launch_bounds__(NT) void k_pk_select(unsigned long long* __restrict__ bins, unsigned long long* __restrict__ kst, int nbins, int shift,
                                                  int* __restrict__ state) {
    __shared__ unsigned long long below[NT + 1];
    const int t = threadIdx.x, per = nbins / NT;            // 8 or 4 bins a thread
    unsigned long long c[MAX_BINS / NT], sum = 0ull;
    for (int e = 0; e < per; ++e) { c[e] = bins[t * per + e]; sum += c[e]; }
    const unsigned long long k = kst[0];
    below[t + 1] = sum;
    __syncthreads();
    if (t == 0) {
        below[0] = 0ull;
        for (int w = 1; w <= NT; ++w) below[w] += below[w - 1];
    }
    __syncthreads();
    unsigned long long at = below[t];
    if (k >= at && k < at + sum) {
        int e = 0;
        while (k >= at + c[e]) at += c[e++];
        kst[0] = k - at;
        kst[1] |= (unsigned long long)(t * per + e) << shift;
    }
    if (t == 0 && k >= below[NT]) atomicOr(&state[ST_ERR], E_RANK);
    for (int e = 0; e < per; ++e) bins[t * per + e] = 0ull;
}

// delta_min rule: the densest point, and every point with rho >= rho_min and delta >= delta_min
__global__ __launch_bounds__(NT) void k_pk_flag(int n, const double* __restrict__ rho, const float* __restrict__ delta, double rho_min, float delta_min,
                                                const int* __restrict__ state, int* __restrict__ flag) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) flag[i] = i == state[ST_DENSEST] || (rho[i] >= rho_min && delta[i] >= delta_min) ? 1 : 0;
}

// the chain labels[i] = labels[nh[i]] by pointer jumping: a centre points to itself
__global__ __launch_bounds__(NT) void k_pk_parent(int n, const int* __restrict__ flag, const int* __restrict__ nh, int* __restrict__ par) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) par[i] = flag[i] || nh[i] < 0 ? i : nh[i];
}
__global__ __launch_bounds__(NT) void k_pk_jump(int n, const int* __restrict__ in, int* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) out[i] = in[in[i]];
}
__global__ __launch_bounds__(NT) void k_pk_label(int n, const int* __restrict__ par, const int* __restrict__ cidx, int* __restrict__ labels,
                                                 int* __restrict__ sizes) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = cidx[par[i]];
    labels[i] = c;
    if (c >= 0) atomicAdd(&sizes[c], 1);
}
__global__ __launch_bounds__(NT) void k_pk_halo(int n, const double* __restrict__ rho, const int* __restrict__ labels, const double* __restrict__ rhob,
                                                uint8_t* __restrict__ halo) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) halo[i] = labels[i] >= 0 && rho[i] < rhob[labels[i]] ? 1 : 0;
}

// ---- interface centres: one workgroup per frame. w_r = P > p_thr (a NaN compares false) or the given weight; terms of weight 0 are skipped
__device__ __forceinline__ float weight_of(float v, int mode, float p_thr, bool& bad) {
    if (mode == PESTO_PEAKS_THRESHOLD) return v > p_thr ? 1.f : 0.f;
    if (!(v >= 0.f) || isinf(v)) { bad = true; return 0.f; }
    return v;
}

__global__ __launch_bounds__(NT) void k_pk_centers(int R, const float* __restrict__ Xp, const float* __restrict__ PW, int mode, float p_thr,
                                                   float* __restrict__ centers, double* __restrict__ wsum, float* __restrict__ rg, int* __restrict__ state) {
    __shared__ double red[NT / 64];
    const int f = blockIdx.x;
    const float* x = Xp + (size_t)f * R * 3;
    const float* pw = PW + (size_t)f * R;
    bool bad = false;
    double s = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int r = threadIdx.x; r < R; r += NT) {
        const double w = (double)weight_of(pw[r], mode, p_thr, bad);
        if (w > 0.0) {
            s += w;
            s0 += w * (double)x[3 * r]; s1 += w * (double)x[3 * r + 1]; s2 += w * (double)x[3 * r + 2];
        }
    }
    if (bad) atomicOr(&state[ST_ERR], E_WEIGHT);
    const double S = block_sum<NT>(s, red);
    const double c0 = block_sum<NT>(s0, red) / S, c1 = block_sum<NT>(s1, red) / S, c2 = block_sum<NT>(s2, red) / S;
    double g = 0.0;
    for (int r = threadIdx.x; r < R; r += NT) {
        const double w = (double)weight_of(pw[r], mode, p_thr, bad);
        if (w > 0.0) {
            const double d0 = (double)x[3 * r] - c0, d1 = (double)x[3 * r + 1] - c1, d2 = (double)x[3 * r + 2] - c2;
            g += w * (d0 * d0 + d1 * d1 + d2 * d2);
        }
    }
    g = block_sum<NT>(g, red);
    if (threadIdx.x != 0) return;
    wsum[f] = S;
    if (S > 0.0) {
        centers[3 * f] = (float)c0; centers[3 * f + 1] = (float)c1; centers[3 * f + 2] = (float)c2;
        rg[f] = (float)sqrt(g / S);
    } else {
        centers[3 * f] = centers[3 * f + 1] = centers[3 * f + 2] = rg[f] = NAN;
    }
}

// ---- host side: the distance source of one call
struct Source {
    bool matrix;
    int F, d, DP, n;
    int iIn, iIdx, iP, iSt;
};

int check_source(int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx, int64_t n_min) {
    if ((X != nullptr) == (D != nullptr)) return fail(PESTO_ERR_INVALID, "exactly one of X and D must be given");
    if (X && (d < 1 || d > PESTO_PEAKS_MAX_DIM)) return fail(PESTO_ERR_INVALID, "1 to %d dimensions, got %d", PESTO_PEAKS_MAX_DIM, d);
    if (F < 1 || F > (X ? 0x7fffffff / PESTO_PEAKS_MAX_DIM : PESTO_CLUSTER_MAX_FRAMES))
        return fail(PESTO_ERR_INVALID, "%s, got %lld", X ? "1 <= F < 2^28 points" : "1 to 16384 rows of D", (long long)F);
    if (n < n_min || n > (X ? PESTO_PEAKS_MAX_POINTS : F) || (!idx && n != F))
        return fail(PESTO_ERR_INVALID, "%lld <= n <= %lld selected rows (n = F without idx), got %lld", (long long)n_min, (long long)(X ? PESTO_PEAKS_MAX_POINTS : F),
                    (long long)n);
    return 0;
}

Source declare_source(Buffers& bf, int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx) {
    Source s;
    s.matrix = D != nullptr;
    s.F = (int)F; s.d = d; s.n = (int)n;
    s.DP = d <= 4 ? 4 : 8;
    s.iIn = s.matrix ? bf.input(D, (size_t)(F * F) * 4) : bf.input(X, (size_t)F * d * 4);
    s.iIdx = bf.input(idx, (size_t)n * 4);
    s.iP = s.matrix ? -1 : bf.scratch((size_t)n * s.DP * 4);
    s.iSt = bf.scratch(ST_WORDS * 4, 0);
    return s;
}

// the checks made on the device, and the points gathered: the one early synchronisation of a call, so that a refused call writes nothing
int validate_source(Buffers& bf, const Source& s, bool has_idx, const char* what) {
    int* st = bf.ptr<int>(s.iSt);
    const int* idx = has_idx ? bf.ptr<const int>(s.iIdx) : nullptr;
    if (s.matrix) {
        hipLaunchKernelGGL(k_pk_check_matrix, dim3((unsigned)s.F), dim3(NT), 0, bf.stm, s.F, bf.ptr<const float>(s.iIn), st);
        if (idx) hipLaunchKernelGGL(k_pk_check_idx, dim3(blocks((size_t)s.n, NT)), dim3(NT), 0, bf.stm, s.F, s.n, idx, st);
    } else {
        hipLaunchKernelGGL(k_pk_gather, dim3(blocks((size_t)s.n, NT)), dim3(NT), 0, bf.stm, s.F, s.d, s.DP, s.n, bf.ptr<const float>(s.iIn), idx, bf.ptr<float>(s.iP), st);
    }
    int32_t state[ST_WORDS] = {0, 0, 0, 0};
    if (int rc = bf.verdict(s.iSt, state, sizeof state, what)) return rc;
    const int e = state[ST_ERR];
    if (e & E_INDEX) return fail(PESTO_ERR_INVALID, "idx: row indices must lie in 0 .. %d", s.F - 1);
    if (e & E_NONFINITE) return fail(PESTO_ERR_INVALID, "%s", s.matrix ? "D has a non-finite entry" : "X has a non-finite coordinate");
    if (e & E_NEGATIVE) return fail(PESTO_ERR_INVALID, "D has a negative entry");
    if (e & E_ASYM) return fail(PESTO_ERR_INVALID, "D is not bitwise symmetric");
    return 0;
}

template <class Act> void launch_pairs(Buffers& bf, const Source& s, bool has_idx, const Act& act) {
    const dim3 grid((unsigned)((s.n + TI - 1) / TI));
    if (s.matrix)
        hipLaunchKernelGGL((k_pairs<Matrix, Act>), grid, dim3(NT), 0, bf.stm, Matrix{bf.ptr<const float>(s.iIn), s.F, has_idx ? bf.ptr<const int>(s.iIdx) : nullptr},
                           act, s.n);
    else if (s.DP == 4)
        hipLaunchKernelGGL((k_pairs<Points<4>, Act>), grid, dim3(NT), 0, bf.stm, Points<4>{bf.ptr<const float>(s.iP)}, act, s.n);
    else
        hipLaunchKernelGGL((k_pairs<Points<8>, Act>), grid, dim3(NT), 0, bf.stm, Points<8>{bf.ptr<const float>(s.iP)}, act, s.n);
}

template <class Act> void launch_rank(Buffers& bf, int n, const Act& act) {
    hipLaunchKernelGGL((k_pairs<None, Act>), dim3((unsigned)((n + TI - 1) / TI)), dim3(NT), 0, bf.stm, None{}, act, n);
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_peaks_last_error(void) { return last_error(); }

int pesto_weighted_centers(pesto_model* m, int64_t F, int64_t R, const float* Xp, const float* PW, int32_t mode, float p_thr, float* centers_out,
                           double* wsum_out, float* rg_out, int32_t ptr_kind, void* stream) {
    if (!Xp || !PW || !centers_out || !wsum_out || !rg_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_PEAKS_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to %d frames, got %lld", PESTO_PEAKS_MAX_FRAMES, (long long)F);
    if (R < 1 || R > 0x7fffffff / 3) return fail(PESTO_ERR_INVALID, "1 <= R < 2^31 / 3 residues, got %lld", (long long)R);
    if (mode != PESTO_PEAKS_THRESHOLD && mode != PESTO_PEAKS_WEIGHTS) return fail(PESTO_ERR_INVALID, "mode must be PESTO_PEAKS_THRESHOLD or PESTO_PEAKS_WEIGHTS");
    if (mode == PESTO_PEAKS_THRESHOLD && std::isnan(p_thr)) return fail(PESTO_ERR_INVALID, "p_thr must not be NaN");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(Xp, (size_t)F * R * 12), iW = bf.input(PW, (size_t)F * R * 4);
    const int iC = bf.output(centers_out, (size_t)F * 12), iS = bf.output(wsum_out, (size_t)F * 8), iG = bf.output(rg_out, (size_t)F * 4);
    // the results are made in scratch and handed over once the weights are known to be good: a refused call writes nothing
    const int tC = bf.scratch((size_t)F * 12), tS = bf.scratch((size_t)F * 8), tG = bf.scratch((size_t)F * 4), iSt = bf.scratch(ST_WORDS * 4, 0);
    int rc = bf.upload();
    int32_t state[ST_WORDS] = {0, 0, 0, 0};
    if (rc == 0) {
        hipLaunchKernelGGL(k_pk_centers, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)R, bf.ptr<const float>(iX), bf.ptr<const float>(iW), mode, p_thr,
                           bf.ptr<float>(tC), bf.ptr<double>(tS), bf.ptr<float>(tG), bf.ptr<int>(iSt));
        rc = bf.verdict(iSt, state, sizeof state, "weighted_centers");
    }
    if (rc == 0 && (state[ST_ERR] & E_WEIGHT)) rc = fail(PESTO_ERR_INVALID, "W has a negative or non-finite weight");
    if (rc == 0) rc = hip_ok(hipMemcpyAsync(bf.ptr<void>(iC), bf.ptr<void>(tC), (size_t)F * 12, hipMemcpyDeviceToDevice, bf.stm), "weighted_centers");
    if (rc == 0) rc = hip_ok(hipMemcpyAsync(bf.ptr<void>(iS), bf.ptr<void>(tS), (size_t)F * 8, hipMemcpyDeviceToDevice, bf.stm), "weighted_centers");
    if (rc == 0) rc = hip_ok(hipMemcpyAsync(bf.ptr<void>(iG), bf.ptr<void>(tG), (size_t)F * 4, hipMemcpyDeviceToDevice, bf.stm), "weighted_centers");
    return bf.finish(rc, "weighted_centers");
}

int pesto_pair_distance_rank(pesto_model* m, int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx, int64_t k,
                             float* dist_out, int32_t ptr_kind, void* stream) {
    if (!dist_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_source(F, d, X, D, n, idx, 2)) return rc;
    const int64_t M = n * (n - 1) / 2;
    if (k < 0 || k >= M) return fail(PESTO_ERR_INVALID, "the rank must lie in 0 .. %lld, got %lld", (long long)(M - 1), (long long)k);
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const Source s = declare_source(bf, F, d, X, D, n, idx);
    const unsigned long long kinit[2] = {(unsigned long long)k, 0ull};
    const int iK = bf.table(kinit, sizeof kinit), iB = bf.scratch(MAX_BINS * 8, 0);
    int rc = bf.upload();
    if (rc == 0) rc = validate_source(bf, s, idx != nullptr, "pair_distance_rank");
    unsigned long long kst[2] = {0ull, 0ull};
    int32_t state[ST_WORDS] = {0, 0, 0, 0};
    if (rc == 0) {
        // the 31 bits below the sign as digits of 11, 10 and 10 bits, the distances recomputed in every pass
        const int shifts[3] = {20, 10, 0}, nbins[3] = {2048, 1024, 1024};
        const unsigned masks[3] = {0u, 0x7ff00000u, 0x7ffffc00u};
        unsigned long long* bins = bf.ptr<unsigned long long>(iB);
        unsigned long long* dk = bf.ptr<unsigned long long>(iK);
        for (int p = 0; p < 3; ++p) {
            Hist h;
            h.g = bins; h.kst = dk; h.mask = masks[p]; h.shift = shifts[p]; h.nbins = nbins[p];
            launch_pairs(bf, s, idx != nullptr, h);
            hipLaunchKernelGGL(k_pk_select, dim3(1), dim3(NT), 0, bf.stm, bins, dk, nbins[p], shifts[p], bf.ptr<int>(s.iSt));
        }
        if ((rc = bf.read(iK, kst, sizeof kst)) == 0) rc = bf.verdict(s.iSt, state, sizeof state, "pair_distance_rank");      // (one synchronisation brings both)
    }
    if (rc == 0 && (state[ST_ERR] & E_RANK)) rc = fail(PESTO_ERR_STATE, "the histogram does not hold the rank");
    if (rc == 0) *dist_out = from_bits((uint32_t)kst[1]);
    return bf.finish(rc, "pair_distance_rank");
}

int pesto_density_peaks(pesto_model* m, int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx, float dc, int32_t kernel,
                        int32_t n_clusters, double rho_min, float delta_min, double* rho_out, float* delta_out, int32_t* nh_out, int32_t* labels_out,
                        uint8_t* halo_out, int32_t* centers_out, int32_t* sizes_out, int32_t* n_clusters_out, int32_t ptr_kind, void* stream) {
    if (!rho_out || !delta_out || !nh_out || !labels_out || !halo_out || !centers_out || !sizes_out || !n_clusters_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_source(F, d, X, D, n, idx, 1)) return rc;
    if (!(std::isfinite(dc) && dc > 0.f)) return fail(PESTO_ERR_INVALID, "dc must be finite and > 0");
    if (kernel != PESTO_PEAKS_CUTOFF && kernel != PESTO_PEAKS_GAUSSIAN) return fail(PESTO_ERR_INVALID, "kernel must be PESTO_PEAKS_CUTOFF or PESTO_PEAKS_GAUSSIAN");
    if (n_clusters < 0 || n_clusters > PESTO_PEAKS_MAX_CLUSTERS || n_clusters > n)
        return fail(PESTO_ERR_INVALID, "n_clusters must lie in 1 .. min(n, %d) (0: the delta_min rule), got %d", PESTO_PEAKS_MAX_CLUSTERS, n_clusters);
    if (n_clusters == 0 && (std::isnan(rho_min) || std::isnan(delta_min))) return fail(PESTO_ERR_INVALID, "rho_min and delta_min must not be NaN");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const Source s = declare_source(bf, F, d, X, D, n, idx);
    const size_t N = (size_t)n;
    const int iRho = bf.output(rho_out, N * 8), iDel = bf.output(delta_out, N * 4), iNh = bf.output(nh_out, N * 4), iLab = bf.output(labels_out, N * 4),
              iHalo = bf.output(halo_out, N), iCen = bf.partial(centers_out, N * 4), iSiz = bf.partial(sizes_out, N * 4);
    const int iGam = bf.scratch(N * 8), iFlag = bf.scratch(N * 4), iCidx = bf.scratch(N * 4), iPa = bf.scratch(N * 4), iPb = bf.scratch(N * 4),
              iRb = bf.scratch(N * 8);
    int rc = bf.upload();
    const bool has_idx = idx != nullptr;
    if (rc == 0) rc = validate_source(bf, s, has_idx, "density_peaks");
    int32_t state[ST_WORDS] = {0, 0, 0, 0};
    if (rc == 0) {
        const int nn = (int)n;
        int* st = bf.ptr<int>(s.iSt);
        double* rho = bf.ptr<double>(iRho);
        float* delta = bf.ptr<float>(iDel);
        int* nh = bf.ptr<int>(iNh);
        int* labels = bf.ptr<int>(iLab);
        int* flag = bf.ptr<int>(iFlag);
        int* cidx = bf.ptr<int>(iCidx);
        int* centers = bf.ptr<int>(iCen);
        int* sizes = bf.ptr<int>(iSiz);
        double* gamma = bf.ptr<double>(iGam);
        if (kernel == PESTO_PEAKS_GAUSSIAN) {
            Density<true> a; a.dc = dc; a.rho = rho;
            launch_pairs(bf, s, has_idx, a);
        } else {
            Density<false> a; a.dc = dc; a.rho = rho;
            launch_pairs(bf, s, has_idx, a);
        }
        Nearest nr; nr.rho = rho; nr.delta = delta; nr.nh = nh; nr.gamma = gamma; nr.state = st;
        launch_pairs(bf, s, has_idx, nr);
        if (n_clusters > 0) {
            Rank<0> pick; pick.val = gamma; pick.flag = flag; pick.cidx = cidx; pick.centers = centers; pick.state = st; pick.K = n_clusters;
            launch_rank(bf, nn, pick);
        } else {
            hipLaunchKernelGGL(k_pk_flag, dim3(blocks((size_t)nn, NT)), dim3(NT), 0, bf.stm, nn, rho, delta, rho_min, delta_min, st, flag);
        }
        Rank<1> order; order.val = rho; order.flag = flag; order.cidx = cidx; order.centers = centers; order.state = st; order.K = 0;
        launch_rank(bf, nn, order);
        int* pa = bf.ptr<int>(iPa);
        int* pb = bf.ptr<int>(iPb);
        hipLaunchKernelGGL(k_pk_parent, dim3(blocks((size_t)nn, NT)), dim3(NT), 0, bf.stm, nn, flag, nh, pa);
        for (int reach = 1; reach < nn; reach *= 2) {       // ceil(log2 n) rounds: a chain has at most n - 1 steps
            hipLaunchKernelGGL(k_pk_jump, dim3(blocks((size_t)nn, NT)), dim3(NT), 0, bf.stm, nn, pa, pb);
            int* t = pa; pa = pb; pb = t;
        }
        rc = hip_ok(hipMemsetAsync(sizes, 0, N * 4, bf.stm), "density_peaks");
        if (rc == 0) rc = hip_ok(hipMemsetAsync(bf.ptr<void>(iRb), 0, N * 8, bf.stm), "density_peaks");
        if (rc == 0) {
            hipLaunchKernelGGL(k_pk_label, dim3(blocks((size_t)nn, NT)), dim3(NT), 0, bf.stm, nn, pa, cidx, labels, sizes);
            Border bd; bd.dc = dc; bd.rho = rho; bd.labels = labels; bd.rhob = bf.ptr<unsigned long long>(iRb);
            launch_pairs(bf, s, has_idx, bd);
            hipLaunchKernelGGL(k_pk_halo, dim3(blocks((size_t)nn, NT)), dim3(NT), 0, bf.stm, nn, rho, labels, bf.ptr<const double>(iRb), bf.ptr<uint8_t>(iHalo));
            rc = bf.verdict(s.iSt, state, sizeof state, "density_peaks");
        }
    }
    const int C = state[ST_CENTRES];
    if (rc == 0 && (C < 1 || C > n)) rc = fail(PESTO_ERR_STATE, "the centre count %d is out of range", C);
    if (rc == 0 && (rc = bf.fetch(iCen, (size_t)C * 4)) == 0) rc = bf.fetch(iSiz, (size_t)C * 4);
    if (rc == 0) *n_clusters_out = C;
    return bf.finish(rc, "density_peaks");
}
