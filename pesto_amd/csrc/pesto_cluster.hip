// pesto_cluster.hip - conformational clustering of MD frames: the minimal RMSD of every frame against every other frame and the GROMOS
// clustering (Daura et al. 1999) over such a matrix. The reference's notebooks (md_analysis/apply_model_with_clustering.ipynb,
// clustering_analysis.ipynb) superpose the frames with trajectory_utils.superpose_transform one reference at a time and hand them to a
// third-party clusterer that is not part of the reference; here the matrix is one launch sequence and the clustering runs on the device.
//
// pairwise_rmsd   k_prmsd_pack   per frame: the selected atoms as rows (x, y, z, 1) of a [16 frames][atom][64] float32 image, the atoms
//                                padded with zero columns to a multiple of 4, the frames with zero frames to a multiple of 16; and
//                                G_f = sum |x - mean|^2 in double
//                 k_prmsd_cov    one workgroup per 16 x 16 frame pairs: the [64 x n] . [n x 64] product as one tile of pesto_mma64.h from the
//                                float32 rows converted to double (every product exact, only the accumulation rounds). Each pair's 4 x 4
//                                block holds H uncentred, both coordinate sums and n; the epilogue hands one pair to every thread:
//                                H - s_a s_b^T / n, its singular values by one-sided Jacobi (kabsch_trace, pesto_geom.h) and
//                                D = scale sqrt(max((G_a + G_b - 2 (s0 + s1 + sign(det H) s2)) / n, 0)), rounded to float32 once
// gromos_clusters k_cl_adjacency bit rows adj[i] by wave ballot, the count of every row, the bitwise symmetry check
//                 k_cl_pick      one workgroup: the active row with the largest count (lowest index on ties), its members, labels
//                 k_cl_update    every still-active row subtracts popcount(row & members)
// All sums run in a fixed order, so every output is bit-identical from call to call.
#include <cmath>
#include <cstdint>

#include "pesto_call.h"
#include "pesto_geom.h"
#include "pesto_mma64.h"

namespace pesto {
namespace {

constexpr int NT = 256;
constexpr int TF = 16;          // frames on a tile side
constexpr int TR = 4 * TF;      // rows on a tile side: (x, y, z, 1) per frame
constexpr int ROUNDS = 32;      // clustering rounds enqueued between two reads of the done flag
static_assert(TR == MT, "16 frames are one tile of pesto_mma64.h");

// ---- pairwise RMSD
// One workgroup per frame slot f of [0, 16 T): the image Pk[f / 16][k][4 (f % 16) + c] and G[f]. A slot beyond F is all zeros.
__global__ __launch_bounds__(NT) void k_prmsd_pack(int F, int N, int n, int npad, const float* __restrict__ xyz, const int* __restrict__ sel,
                                                   float* __restrict__ Pk, double* __restrict__ G) {
    __shared__ double red[NT / 64];
    const int f = blockIdx.x;
    float4* out = (float4*)(Pk + ((size_t)(f >> 4) * npad) * TR) + (f & 15);
    if (f >= F) {
        for (int k = threadIdx.x; k < npad; k += NT) out[(size_t)k * TF] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (threadIdx.x == 0) G[f] = 0.0;
        return;
    }
    const float* x = xyz + (size_t)f * N * 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < npad; k += NT) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < n) {
            const float* p = x + (size_t)(sel ? sel[k] : k) * 3;
            v = make_float4(p[0], p[1], p[2], 1.f);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z;
        }
        out[(size_t)k * TF] = v;
    }
    const double m0 = block_sum<NT>(s0, red) / n, m1 = block_sum<NT>(s1, red) / n, m2 = block_sum<NT>(s2, red) / n;
    double g = 0.0;
    for (int k = threadIdx.x; k < n; k += NT) {
        const float* p = x + (size_t)(sel ? sel[k] : k) * 3;
        const double d0 = (double)p[0] - m0, d1 = (double)p[1] - m1, d2 = (double)p[2] - m2;
        g += d0 * d0 + d1 * d1 + d2 * d2;
    }
    g = block_sum<NT>(g, red);
    if (threadIdx.x == 0) G[f] = g;
}

// a stage's operand, KC atoms x 64 rows of a tile: one float4 (one frame's row group of one atom) per thread, converted to double when staged
__device__ __forceinline__ float4 stage_load(const float* __restrict__ tile, int k0, int npad) {
    const int kk = threadIdx.x >> 4;
    if (k0 + kk >= npad) return make_float4(0.f, 0.f, 0.f, 0.f);
    return ((const float4*)(tile + (size_t)(k0 + kk) * TR))[threadIdx.x & 15];
}

// Workgroup (ti, tj): the 16 frames 16 ti .. of A against the 16 frames 16 tj .. of B, one tile of pesto_mma64.h (wave w: the rows of A's
// frames 4 w .. 4 w + 3 against all 64 rows of B). self: only tj >= ti and within a diagonal tile only j >= i are evaluated and written
// to both D[i,j] and D[j,i]; the diagonal is 0.
__global__ __launch_bounds__(NT) void k_prmsd_cov(int Fa, int Fb, int Tb, int n, int npad, const float* __restrict__ Pa, const float* __restrict__ Pb,
                                                  const double* __restrict__ Ga, const double* __restrict__ Gb, double scale, int self,
                                                  float* __restrict__ D) {
    __shared__ double lds[MMA64_LDS];           // the staged tiles, then the accumulator image (TR x HS)
    const int ti = blockIdx.x / Tb, tj = blockIdx.x % Tb;
    if (self && tj < ti) return;
    const float *ta = Pa + (size_t)ti * npad * TR, *tb = Pb + (size_t)tj * npad * TR;
    auto load = [&](int k0, float4& ra, float4& rb) { ra = stage_load(ta, k0, npad); rb = stage_load(tb, k0, npad); };
    auto store = [](double* As, const float4& ra) { store_kmajor(As, ra); };
    f64x4 acc[4];
    mma64_loop<float4, true>(lds, 0, npad, load, store, acc);            // npad is a multiple of 4: the atoms' tail is zero columns of the image
    __syncthreads();
    mma64_store(acc, lds, HS, 1.0);
    __syncthreads();
    const int fa = threadIdx.x >> 4, fb = threadIdx.x & 15;
    const int i = ti * TF + fa, j = tj * TF + fb;
    if (i >= Fa || j >= Fb || (self && i > j)) return;
    const double* blk = lds + (4 * fa) * HS + 4 * fb;
    const double nd = (double)n;
    double H[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[3 * a + b] = blk[a * HS + b] - (blk[a * HS + 3] * blk[3 * HS + b]) / nd;
    // D[i,j] and D[j,i] see H and its transpose: evaluate one of the two, chosen by the entries themselves, so both get the same bits
    const bool flip = H[1] != H[3] ? H[1] > H[3] : H[2] != H[6] ? H[2] > H[6] : H[5] > H[7];
    if (flip) {
        double t = H[1]; H[1] = H[3]; H[3] = t;
        t = H[2]; H[2] = H[6]; H[6] = t;
        t = H[5]; H[5] = H[7]; H[7] = t;
    }
    const double e = ((Ga[i] + Gb[j]) - 2.0 * kabsch_trace(H)) / nd;
    float v = (float)(scale * sqrt(fmax(e, 0.0)));
    if (self) {
        if (i == j) v = 0.f;
        D[(size_t)j * Fb + i] = v;
    }
    D[(size_t)i * Fb + j] = v;
}

// ---- GROMOS clustering
enum { ST_ASYM = 0, ST_DONE = 1, ST_CLUSTERS = 2, ST_ACTIVE = 3, ST_WORDS = 4 };

__global__ void k_cl_init(int F, int W, unsigned long long* __restrict__ active, int* __restrict__ state) {
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        const int left = F - 64 * w;
        active[w] = left >= 64 ? ~0ull : (1ull << left) - 1ull;
    }
    if (threadIdx.x == 0) { state[ST_ASYM] = 0; state[ST_DONE] = 0; state[ST_CLUSTERS] = 0; state[ST_ACTIVE] = F; }
}

// one workgroup per row i: adj[i] = (D[i,j] <= cut or i == j) as bits (a NaN compares false), cnt[i] its popcount; every j > i also
// compares the bits of D[i,j] and D[j,i]
__global__ __launch_bounds__(NT) void k_cl_adjacency(int F, int W, const float* __restrict__ D, float cut, unsigned long long* __restrict__ adj,
                                                     int* __restrict__ cnt, int* __restrict__ state) {
    __shared__ int part[NT / 64];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c = 0;
    bool asym = false;
    for (int w = wave; w < W; w += NT / 64) {
        const int j = 64 * w + lane;
        bool bit = false;
        if (j < F) {
            const float d = D[(size_t)i * F + j];
            bit = d <= cut || i == j;
            if (j > i) asym |= __float_as_uint(d) != __float_as_uint(D[(size_t)j * F + i]);
        }
        const unsigned long long m = __ballot(bit);
        if (lane == 0) adj[(size_t)i * W + w] = m;
        c += __popcll(m);
    }
    if (__ballot(asym) != 0ull && lane == 0) atomicOr(&state[ST_ASYM], 1);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[i] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup of 1024 threads. Nothing to do once done. Else the active row with the largest count, the lowest index on ties; if that
// count is 1 every remaining frame is its own cluster, in index order; otherwise the centre's active neighbours become cluster number
// state[ST_CLUSTERS] and leave the active set (members: this round's, for k_cl_update).
__global__ __launch_bounds__(1024) void k_cl_pick(int F, int W, const unsigned long long* __restrict__ adj, const int* __restrict__ cnt,
                                                  unsigned long long* __restrict__ active, unsigned long long* __restrict__ members,
                                                  int* __restrict__ labels, int* __restrict__ centers, int* __restrict__ sizes,
                                                  int* __restrict__ state) {
    __shared__ int wc[16], wi[16], best_c, best_i, size;
    __shared__ int pre[256];
    if (state[ST_DONE]) return;
    const int t = threadIdx.x, nc = state[ST_CLUSTERS], n_active = state[ST_ACTIVE];
    int bc = -1, bi = 0x7fffffff;
    for (int i = t; i < F; i += 1024)
        if ((active[i >> 6] >> (i & 63)) & 1ull) {
            const int c = cnt[i];
            if (c > bc) { bc = c; bi = i; }
        }
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o), oi = __shfl_xor(bi, o);
        if (oc > bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if ((t & 63) == 0) { wc[t >> 6] = bc; wi[t >> 6] = bi; }
    if (t == 0) size = 0;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < 16; ++k)
            if (wc[k] > bc || (wc[k] == bc && wi[k] < bi)) { bc = wc[k]; bi = wi[k]; }
        best_c = bc; best_i = bi;
    }
    __syncthreads();
    if (best_c <= 1) {
        unsigned long long m = t < W ? active[t] : 0ull;
        if (t < 256) pre[t] = __popcll(m);
        __syncthreads();
        if (t < W) {
            int at = nc;
            for (int k = 0; k < t; ++k) at += pre[k];
            while (m) {
                const int fr = 64 * t + __ffsll((long long)m) - 1;
                m &= m - 1ull;
                labels[fr] = at; centers[at] = fr; sizes[at] = 1;
                ++at;
            }
            active[t] = 0ull;
        }
        if (t == 0) { state[ST_CLUSTERS] = nc + n_active; state[ST_ACTIVE] = 0; state[ST_DONE] = 1; }
        return;
    }
    if (t < W) {
        unsigned long long m = adj[(size_t)best_i * W + t] & active[t];
        members[t] = m;
        active[t] &= ~m;
        if (m) atomicAdd(&size, __popcll(m));
        while (m) {
            labels[64 * t + __ffsll((long long)m) - 1] = nc;
            m &= m - 1ull;
        }
    }
    __syncthreads();
    if (t == 0) {
        centers[nc] = best_i; sizes[nc] = size;
        state[ST_CLUSTERS] = nc + 1; state[ST_ACTIVE] = n_active - size;
        if (n_active - size <= 0) state[ST_DONE] = 1;
    }
}

// one wave per row: a still-active row loses the members it is adjacent to
__global__ __launch_bounds__(NT) void k_cl_update(int F, int W, const unsigned long long* __restrict__ adj, const unsigned long long* __restrict__ active,
                                                  const unsigned long long* __restrict__ members, int* __restrict__ cnt, const int* __restrict__ state) {
    if (state[ST_DONE]) return;
    const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= F || !((active[i >> 6] >> (i & 63)) & 1ull)) return;
    int s = 0;
    for (int w = lane; w < W; w += 64) s += __popcll(adj[(size_t)i * W + w] & members[w]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) cnt[i] -= s;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_cluster_last_error(void) { return last_error(); }

int pesto_pairwise_rmsd(pesto_model* m, int64_t Fa, int64_t Fb, int64_t N, int64_t n_sel, const float* xyz_a, const float* xyz_b, const int32_t* sel,
                        double scale, float* D_out, int32_t ptr_kind, void* stream) {
    if (!xyz_a || !D_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    const bool self = !xyz_b;
    if (Fa < 1 || Fb < 1 || Fa > PESTO_CLUSTER_MAX_PAIRS || Fb > PESTO_CLUSTER_MAX_PAIRS || Fa * Fb > PESTO_CLUSTER_MAX_PAIRS || (self && Fa != Fb))
        return fail(PESTO_ERR_INVALID, "1 <= Fa * Fb <= 2^28 frame pairs (Fa = Fb without xyz_b), got %lld x %lld", (long long)Fa, (long long)Fb);
    if (N < 1 || N > 0x7fffffff || n_sel < 1 || n_sel > N || (!sel && n_sel != N))
        return fail(PESTO_ERR_INVALID, "1 <= n_sel <= N < 2^31 atoms (n_sel = N without a selection)");
    if (!std::isfinite(scale)) return fail(PESTO_ERR_INVALID, "scale must be finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    const int64_t npad = (n_sel + 3) & ~(int64_t)3, Ta = (Fa + TF - 1) / TF, Tb = (Fb + TF - 1) / TF;
    Buffers bf(ptr_kind, stream);
    const int iA = bf.input(xyz_a, (size_t)Fa * N * 12), iB = self ? iA : bf.input(xyz_b, (size_t)Fb * N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iD = bf.output(D_out, (size_t)(Fa * Fb) * 4);
    const int iPa = bf.scratch((size_t)Ta * npad * TR * 4), iGa = bf.scratch((size_t)Ta * TF * 8);
    const int iPb = self ? iPa : bf.scratch((size_t)Tb * npad * TR * 4), iGb = self ? iGa : bf.scratch((size_t)Tb * TF * 8);
    int rc = bf.upload();
    if (rc == 0) {
        const int* s = sel ? bf.ptr<const int>(iS) : nullptr;
        hipLaunchKernelGGL(k_prmsd_pack, dim3((unsigned)(Ta * TF)), dim3(NT), 0, bf.stm, (int)Fa, (int)N, (int)n_sel, (int)npad, bf.ptr<const float>(iA), s,
                           bf.ptr<float>(iPa), bf.ptr<double>(iGa));
        if (!self)
            hipLaunchKernelGGL(k_prmsd_pack, dim3((unsigned)(Tb * TF)), dim3(NT), 0, bf.stm, (int)Fb, (int)N, (int)n_sel, (int)npad, bf.ptr<const float>(iB),
                               s, bf.ptr<float>(iPb), bf.ptr<double>(iGb));
        hipLaunchKernelGGL(k_prmsd_cov, dim3((unsigned)(Ta * Tb)), dim3(NT), 0, bf.stm, (int)Fa, (int)Fb, (int)Tb, (int)n_sel, (int)npad,
                           bf.ptr<const float>(iPa), bf.ptr<const float>(iPb), bf.ptr<const double>(iGa), bf.ptr<const double>(iGb), scale, self ? 1 : 0,
                           bf.ptr<float>(iD));
    }
    return bf.finish(rc, "pairwise_rmsd");
}

int pesto_gromos_clusters(pesto_model* m, int64_t F, const float* D, float cutoff, int32_t* labels_out, int32_t* centers_out, int32_t* sizes_out,
                          int32_t* n_clusters_out, int32_t ptr_kind, void* stream) {
    if (!D || !labels_out || !centers_out || !sizes_out || !n_clusters_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_CLUSTER_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to %d frames, got %lld", PESTO_CLUSTER_MAX_FRAMES, (long long)F);
    if (!std::isfinite(cutoff)) return fail(PESTO_ERR_INVALID, "cutoff must be finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    const int W = (int)((F + 63) / 64);
    Buffers bf(ptr_kind, stream);
    const int iD = bf.input(D, (size_t)(F * F) * 4);
    const int iL = bf.output(labels_out, (size_t)F * 4), iC = bf.output(centers_out, (size_t)F * 4), iZ = bf.output(sizes_out, (size_t)F * 4);
    const int iAdj = bf.scratch((size_t)F * W * 8), iCnt = bf.scratch((size_t)F * 4), iAct = bf.scratch((size_t)W * 8), iMem = bf.scratch((size_t)W * 8),
              iSt = bf.scratch(ST_WORDS * 4);
    int rc = bf.upload();
    int32_t state[ST_WORDS] = {0, 0, 0, 0};
    if (rc == 0) {
        unsigned long long* adj = bf.ptr<unsigned long long>(iAdj);
        unsigned long long* act = bf.ptr<unsigned long long>(iAct);
        unsigned long long* mem = bf.ptr<unsigned long long>(iMem);
        int* cnt = bf.ptr<int>(iCnt);
        int* st = bf.ptr<int>(iSt);
        hipLaunchKernelGGL(k_cl_init, dim3(1), dim3(NT), 0, bf.stm, (int)F, W, act, st);
        hipLaunchKernelGGL(k_cl_adjacency, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)F, W, bf.ptr<const float>(iD), cutoff, adj, cnt, st);
        // every round extracts at least one frame, so F rounds always suffice; a round after the last one is two empty launches
        for (int64_t done_rounds = 0; rc == 0 && !state[ST_DONE] && done_rounds < F + ROUNDS; done_rounds += ROUNDS) {
            for (int r = 0; r < ROUNDS; ++r) {
                hipLaunchKernelGGL(k_cl_pick, dim3(1), dim3(1024), 0, bf.stm, (int)F, W, adj, cnt, act, mem, bf.ptr<int>(iL), bf.ptr<int>(iC), bf.ptr<int>(iZ), st);
                hipLaunchKernelGGL(k_cl_update, dim3((unsigned)((F + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, bf.stm, (int)F, W, adj, act, mem, cnt, st);
            }
            rc = bf.verdict(iSt, state, sizeof state, "gromos_clusters");
            // the matrix is an argument: its symmetry is known with the first read of the state, the call's one argument check on the device
            if (rc == 0 && state[ST_ASYM]) rc = fail(PESTO_ERR_INVALID, "D is not bitwise symmetric");
        }
        if (rc == 0 && !state[ST_DONE]) rc = fail(PESTO_ERR_STATE, "the clustering did not end within F rounds");
    }
    if (rc == 0) *n_clusters_out = state[ST_CLUSTERS];
    return bf.finish(rc, "gromos_clusters");
}
