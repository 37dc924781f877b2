// pesto_chainmap.hip - the chain mapping of oligomers: which model chain lies on which reference chain, for every frame of a run or every
// decoy of a set in one call, so that lDDT, DockQ and the TM-score of a complex see the copies of an entity in the reference's order.
//
// The C entry point (include/pesto_hip.h) lives here too, on the call plumbing of pesto_call.h, with a message channel of its own; the
// sizes, the layout (checked on the host before anything is launched) and the frames' scan for infinities are pesto_oligomer.h's.
//
// The mapping is a maximum over superpositions, found by a search like the TM-score's (pesto_tmscore.hip): from every seed, a chain pair of
// one entity, the model is fitted onto the reference, every chain pair of every entity is scored under that fit, the copies are assigned
// one to one so that the summed score is the exact maximum, and the mapped chains together give the next fit, until the mapping repeats.
// A workgroup runs whole seeds: the fit is kabsch_fit of pesto_fit.h on the common slots of the mapped pairs, gathered in order into two
// index lists in global memory; a wave takes a chain pair at a time for the pair sums, lanes over the slots (coordinates come from global
// memory: a complex stays in L2, 64 x 4096 residues do not fit in LDS); the assignment is a subset DP over the larger side's chains in
// 2^12 doubles of LDS, level by level in popcount. Workgroups share a frame's seeds out; k_cm_final takes the maximum over the shares,
// ties to the lowest seed, which does not depend on the sharing. No atomics on results: every output repeats its bits from call to call.
#include <climits>
#include <cmath>

#include "pesto_fit.h"
#include "pesto_oligomer.h"

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup of k_cm_search: four waves; 159 VGPRs let three such workgroups share a CU (37.4 KB of LDS each)
constexpr int NW = NT / 64;
constexpr int TARGET_GROUPS = 1024;     // workgroups a call aims at, so that one decoy still fills the device
constexpr int MAX_C = PESTO_CHAINMAP_MAX_CHAINS;
constexpr int MAX_G = PESTO_CHAINMAP_MAX_GROUP;
constexpr int SEED_NONE = INT_MAX;      // CmBest::seed of a share that visited no fit
constexpr int SEED_BAD = -1;            // ... of a frame with an infinite coordinate
constexpr int64_t MAX_CHUNK = 1 << 16;  // frames of one launch

// what a share of a frame's seeds found: the largest total, where, and the mapping, pair sums and fit there
struct CmBest {
    double total, R[9], t[3], cs[MAX_C];
    int map[MAX_C];
    int seed, round, n_mapped, pad;
};

// ------------------------------------------------------------------------------------------------ the reference
// cnt[a] = the slots of reference chain a with finite coordinates: the divisor of chain_score; -1 if the chain has an infinite
// coordinate, which also raises ref_bad for k_oligomer_frames (an integer OR: the same whatever the order). One wave per chain.
__global__ __launch_bounds__(64) void k_cm_ref_counts(const int* __restrict__ ro, const float* __restrict__ ref, int* __restrict__ cnt,
                                                      int* __restrict__ ref_bad) {
    const int a = blockIdx.x, r0 = ro[a], L = ro[a + 1] - r0;
    int n = 0, inf = 0;
    for (int k = threadIdx.x; k < L; k += 64) {
        const float* p = ref + (size_t)(r0 + k) * 3;
        n += finite3(p) ? 1 : 0;
        inf += fabsf(p[0]) == INFINITY || fabsf(p[1]) == INFINITY || fabsf(p[2]) == INFINITY ? 1 : 0;
    }
    n = wave_sum(n);
    inf = wave_sum(inf);
    if (threadIdx.x == 0) {
        cnt[a] = inf ? -1 : n;
        if (inf) atomicOr(ref_bad, 1);
    }
}

// ------------------------------------------------------------------------------------------------ the search
// replaces: the chain mapper's loop over seeds, one decoy per process. Workgroup (frame f0 + blockIdx.x / shares, share sh): the share
// runs the seeds sh, sh + shares, ... < Cr Cm of its frame in ascending order. lists: 2 cap ints per workgroup (the gathered slots).
__global__ __launch_bounds__(NT) void k_cm_search(int shares, int Cr, int Cm, int Nr, int Nm, int n_iter, double d0, double scale, int cap,
                                                  const int* __restrict__ ro_g, const int* __restrict__ rg_g, const int* __restrict__ mo_g,
                                                  const int* __restrict__ mg_g, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                  const int* __restrict__ frame_bad, int* lists, CmBest* __restrict__ out) {
    __shared__ double s_f[1 << MAX_G];          // the assignment's table: the best sum of the first popcount(mask) rows placed on mask
    __shared__ double s_S[MAX_G * MAX_G];       // the pair sums of one group, [reference chain][model chain]
    __shared__ double s_red[NW], s_R[9], s_cs[MAX_C], s_rv[NW], s_total;
    __shared__ int s_ro[MAX_C + 1], s_mo[MAX_C + 1], s_rg[MAX_C], s_mg[MAX_C], s_map[MAX_C], s_prev[MAX_C], s_fit[MAX_C];
    __shared__ int s_ra[MAX_G], s_mb[MAX_G], s_nr, s_nm, s_wcnt[NW], s_rm[NW], s_flag, s_gmax;
    __shared__ CmBest s_best;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned fl = blockIdx.x / (unsigned)shares, sh = blockIdx.x % (unsigned)shares;
    const float* X = xyz + (size_t)fl * Nm * 3;
    int* lr = lists + (size_t)blockIdx.x * 2 * cap;
    int* lm = lr + cap;
    if (frame_bad[fl]) {                        // (k_oligomer_frames: the same verdict for every share of the frame)
        if (tid == 0) out[blockIdx.x].seed = SEED_BAD;
        return;
    }
    for (int c = tid; c <= Cr; c += NT) s_ro[c] = ro_g[c];
    for (int c = tid; c <= Cm; c += NT) s_mo[c] = mo_g[c];
    for (int c = tid; c < Cr; c += NT) s_rg[c] = rg_g[c];
    for (int c = tid; c < Cm; c += NT) s_mg[c] = mg_g[c];
    __syncthreads();
    if (tid == 0) {
        int g = 0;
        for (int c = 0; c < Cr; ++c) g = max(g, s_rg[c] + 1);
        s_gmax = g;                             // (a group the reference lacks maps nothing)
        s_best.total = -1.0;
        s_best.seed = SEED_NONE;
        s_best.round = -1;
        s_best.n_mapped = 0;
    }
    __syncthreads();
    const int gmax = s_gmax;

    // the common finite slots of the chain pairs (a, s_fit[a]), in the order of a and then of the slot, as indices into the reference
    // (lr) and into the frame (lm); returns their number, the same in every thread
    auto gather = [&]() {
        int base = 0;
        for (int a = 0; a < Cr; ++a) {
            const int b = s_fit[a];
            if (b < 0) continue;
            const int r0 = s_ro[a], m0 = s_mo[b], L = s_ro[a + 1] - r0;
            for (int k0 = 0; k0 < L; k0 += NT) {
                const int k = k0 + tid;
                const bool ok = k < L && finite3(ref + (size_t)(r0 + k) * 3) && finite3(X + (size_t)(m0 + k) * 3);
                const unsigned long long vote = __ballot(ok);
                if (lane == 0) s_wcnt[wave] = __popcll(vote);
                __syncthreads();
                int at = base + __popcll(vote & ((1ull << lane) - 1ull));
                for (int w = 0; w < NW; ++w) {
                    if (w < wave) at += s_wcnt[w];
                    base += s_wcnt[w];
                }
                if (ok && at < cap) { lr[at] = r0 + k; lm[at] = m0 + k; }
                __syncthreads();
            }
        }
        return base;
    };

    const int n_pairs = Cr * Cm;
    for (int seed = (int)sh; seed < n_pairs; seed += shares) {
        const int sa = seed / Cm, sb = seed % Cm;
        if (s_rg[sa] != s_mg[sb]) continue;
        __syncthreads();
        for (int c = tid; c < Cr; c += NT) s_fit[c] = c == sa ? sb : -1;
        __syncthreads();
        int n = gather();
        if (n < 3) continue;
        for (int it = 0; it < n_iter; ++it) {
            Fit ft;
            kabsch_fit<NT, true>(atoms(X, lm), atoms(ref, lr), n, s_red, s_R, ft);
            // ---- the assignment under this fit, group after group
            for (int c = tid; c < Cr; c += NT) { s_map[c] = -1; s_cs[c] = 0.0; }
            if (tid == 0) s_total = 0.0;
            for (int g = 0; g < gmax; ++g) {
                __syncthreads();
                if (tid == 0) {
                    int nr = 0, nm = 0;
                    for (int c = 0; c < Cr; ++c)
                        if (s_rg[c] == g && nr < MAX_G) s_ra[nr++] = c;
                    for (int c = 0; c < Cm; ++c)
                        if (s_mg[c] == g && nm < MAX_G) s_mb[nm++] = c;
                    s_nr = nr;
                    s_nm = nm;
                }
                __syncthreads();
                const int nr = s_nr, nm = s_nm;
                if (nr == 0 || nm == 0) continue;
                // the pair sums: a wave per chain pair, lanes over the slots, one butterfly: the order of the additions is fixed
                for (int q = wave; q < nr * nm; q += NW) {
                    const int a = s_ra[q / nm], b = s_mb[q % nm];
                    const int r0 = s_ro[a], m0 = s_mo[b], L = s_ro[a + 1] - r0;
                    const auto px = atoms<true>(X + (size_t)m0 * 3, nullptr), py = atoms<true>(ref + (size_t)r0 * 3, nullptr);
                    double sum = 0.0;
                    for (int k = lane; k < L; k += 64) {
                        double x[3], y[3], p[3];
                        px(k, x);
                        py(k, y);
                        moved(x, ft, p);
                        const double e0 = p[0] - y[0], e1 = p[1] - y[1], e2 = p[2] - y[2];
                        const double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2) * scale;
                        const double qd = d / d0;
                        const double term = 1.0 / (1.0 + qd * qd);
                        sum += term == term ? term : 0.0;           // (a slot one of the two lacks is NaN: no term)
                    }
                    sum = wave_sum(sum);
                    if (lane == 0) s_S[q] = sum;
                }
                // the subset DP: rows are the side with fewer chains, masks run over the other side's chains
                const bool swap = nr > nm;
                const int rows = swap ? nm : nr, cols = swap ? nr : nm, n_mask = 1 << cols;
                auto val = [&](int row, int col) { return swap ? s_S[col * nm + row] : s_S[row * nm + col]; };
                if (tid == 0) s_f[0] = 0.0;
                for (int k = 1; k <= rows; ++k) {
                    __syncthreads();
                    for (int mask = tid; mask < n_mask; mask += NT) {
                        if (__popc(mask) != k) continue;
                        double v = -1.0;
                        for (int c = 0; c < cols; ++c)
                            if (mask >> c & 1) v = fmax(v, s_f[mask ^ (1 << c)] + val(k - 1, c));
                        s_f[mask] = v;
                    }
                }
                __syncthreads();
                // the best full placement: the largest sum, ties to the lowest mask
                double bv = -1.0;
                int bm = n_mask - 1;
                if (rows < cols) {
                    for (int mask = tid; mask < n_mask; mask += NT)
                        if (__popc(mask) == rows && s_f[mask] > bv) { bv = s_f[mask]; bm = mask; }
                    for (int o = 32; o > 0; o >>= 1) {
                        const double v2 = __shfl_xor(bv, o);
                        const int m2 = __shfl_xor(bm, o);
                        if (v2 > bv || (v2 == bv && m2 < bm)) { bv = v2; bm = m2; }
                    }
                    if (lane == 0) { s_rv[wave] = bv; s_rm[wave] = bm; }
                    __syncthreads();
                }
                if (tid == 0) {
                    if (rows < cols)
                        for (int w = 0; w < NW; ++w) {
                            if (w == 0 || s_rv[w] > bv || (s_rv[w] == bv && s_rm[w] < bm)) { bv = s_rv[w]; bm = s_rm[w]; }
                        }
                    s_total += s_f[bm];
                    // one lane walks back: the last row first, the lowest column whose step gives the table's value
                    int mask = bm;
                    for (int k = rows; k >= 1; --k)
                        for (int c = 0; c < cols; ++c)
                            if ((mask >> c & 1) && s_f[mask] == s_f[mask ^ (1 << c)] + val(k - 1, c)) {
                                const int a = swap ? s_ra[c] : s_ra[k - 1], b = swap ? s_mb[k - 1] : s_mb[c];
                                s_map[a] = b;
                                s_cs[a] = val(k - 1, c);
                                mask ^= 1 << c;
                                break;
                            }
                }
            }
            __syncthreads();
            // ---- this fit is visited
            if (tid == 0) {
                if (s_total > s_best.total) {           // (seeds and rounds come in ascending order: the first to attain the maximum stays)
                    s_best.total = s_total;
                    s_best.seed = seed;
                    s_best.round = it;
                    int nmap = 0;
                    for (int c = 0; c < Cr; ++c) { s_best.map[c] = s_map[c]; s_best.cs[c] = s_cs[c]; nmap += s_map[c] >= 0; }
                    s_best.n_mapped = nmap;
                    for (int c = 0; c < 9; ++c) s_best.R[c] = ft.R[c];
                    for (int c = 0; c < 3; ++c)
                        s_best.t[c] = ft.same ? 0.0 : ft.m[3 + c] - ((ft.m[0] * ft.R[c] + ft.m[1] * ft.R[3 + c]) + ft.m[2] * ft.R[6 + c]);
                }
                int same = it > 0;
                for (int c = 0; c < Cr; ++c) same &= s_map[c] == s_prev[c];
                s_flag = same;
            }
            __syncthreads();
            if (s_flag || it + 1 == n_iter) break;
            for (int c = tid; c < Cr; c += NT) { s_prev[c] = s_map[c]; s_fit[c] = s_map[c]; }
            __syncthreads();
            n = gather();
            if (n < 3) break;
        }
    }
    __syncthreads();
    // (vector stores, a member at a time)
    CmBest* o = out + blockIdx.x;
    if (tid == 0) {
        o->total = s_best.total;
        o->seed = s_best.seed;
        o->round = s_best.round;
        o->n_mapped = s_best.n_mapped;
    }
    const bool found = s_best.seed != SEED_NONE;
    if (tid < 9) o->R[tid] = found ? s_best.R[tid] : 0.0;
    if (tid < 3) o->t[tid] = found ? s_best.t[tid] : 0.0;
    for (int c = tid; c < Cr; c += NT) {
        o->map[c] = found ? s_best.map[c] : -1;
        o->cs[c] = found ? s_best.cs[c] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ the outputs
// One wave per frame: the maximum total over the frame's shares (ties: the lowest seed), the quotients, rounded once. A frame with an
// infinite coordinate or without a seed: NaN score and fit, mapping, seed and round -1.
__global__ __launch_bounds__(64) void k_cm_final(int shares, int Cr, double lnorm, const CmBest* __restrict__ parts, const int* __restrict__ ref_cnt,
                                                 float* __restrict__ score_out, int* __restrict__ map_out, float* __restrict__ cs_out,
                                                 int* __restrict__ nmap_out, int* __restrict__ seed_out, int* __restrict__ round_out,
                                                 double* __restrict__ rot_out, double* __restrict__ tr_out) {
    const size_t u = blockIdx.x;
    const CmBest* P = parts + u * (size_t)shares;
    const int lane = threadIdx.x;
    bool bad = P[0].seed == SEED_BAD;                   // (every share of the frame saw the same coordinates)
    double total = -1.0;
    int seed = SEED_NONE, at = 0;
    if (!bad)
        for (int s = lane; s < shares; s += 64) {
            const CmBest& o = P[s];
            if (o.total > total || (o.total == total && o.seed < seed)) { total = o.total; seed = o.seed; at = s; }
        }
    for (int o = 32; o > 0; o >>= 1) {
        const double t2 = __shfl_xor(total, o);
        const int seed2 = __shfl_xor(seed, o), at2 = __shfl_xor(at, o);
        if (t2 > total || (t2 == total && (seed2 < seed || (seed2 == seed && at2 < at)))) { total = t2; seed = seed2; at = at2; }
    }
    bad = bad || seed == SEED_NONE;
    const CmBest& B = P[at];
    for (int c = lane; c < Cr; c += 64) {
        const int b = bad ? -1 : B.map[c];
        map_out[u * Cr + c] = b;
        cs_out[u * Cr + c] = b < 0 || ref_cnt[c] <= 0 ? 0.0f : (float)(B.cs[c] / (double)ref_cnt[c]);
    }
    if (lane < 9) rot_out[u * 9 + lane] = bad ? (double)NAN : B.R[lane];
    if (lane < 3) tr_out[u * 3 + lane] = bad ? (double)NAN : B.t[lane];
    if (lane != 0) return;
    score_out[u] = bad ? NAN : (float)(total / lnorm);
    nmap_out[u] = bad ? 0 : B.n_mapped;
    seed_out[u] = bad ? -1 : seed;
    round_out[u] = bad ? -1 : B.round;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_chainmap_last_error(void) { return last_error(); }

int pesto_chainmap(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                   const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, double norm_len, double d0, int32_t n_iter,
                   double scale, float* score_out, int32_t* mapping_out, float* chain_score_out, int32_t* n_mapped_out, int32_t* seed_out,
                   int32_t* round_out, double* rotation_out, double* translation_out, int32_t ptr_kind, void* stream) {
    if (!ref_offsets || !ref_group || !offsets || !group || !xyz_ref || !xyz || !score_out || !mapping_out || !chain_score_out || !n_mapped_out ||
        !seed_out || !round_out || !rotation_out || !translation_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_oligomer_sizes(F, Nr, Nm, Cr, Cm, scale)) return rc;
    if (n_iter < 1 || n_iter > PESTO_CHAINMAP_MAX_ITER) return fail(PESTO_ERR_INVALID, "1 <= n_iter <= %d", PESTO_CHAINMAP_MAX_ITER);
    if (!(std::isfinite(norm_len) && norm_len > 0.0) || !(std::isfinite(d0) && d0 > 0.0)) return fail(PESTO_ERR_INVALID, "norm_len and d0 must be positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    // the layout is checked on the host before anything is declared or launched: a refused call writes nothing
    OligomerLayout lay;
    if (int rc = fetch_layout("chainmap", Nr, Nm, Cr, Cm, ref_offsets, ref_group, offsets, group, ptr_kind, stream, lay)) return rc;
    const int64_t cap = std::min(Nr, Nm);
    // the shares of a frame and the frames of one launch: their gathered slot lists (8 cap bytes a workgroup) fit the workspace
    const int shares = (int)std::min<int64_t>(std::min<int64_t>((int64_t)Cr * Cm, std::max<int64_t>(1, (TARGET_GROUPS + F - 1) / F)),
                                              std::max<int64_t>(1, (int64_t)PESTO_CHAINMAP_WORKSPACE / (cap * 8)));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(F, MAX_CHUNK), (int64_t)PESTO_CHAINMAP_WORKSPACE / (shares * cap * 8)));
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)Nr * 12), iX = bf.input(xyz, (size_t)F * Nm * 12);
    const int iRo = bf.input(ref_offsets, (size_t)(Cr + 1) * 4), iRg = bf.input(ref_group, (size_t)Cr * 4), iMo = bf.input(offsets, (size_t)(Cm + 1) * 4),
              iMg = bf.input(group, (size_t)Cm * 4);
    const int iSc = bf.output(score_out, (size_t)F * 4), iMp = bf.output(mapping_out, (size_t)F * Cr * 4), iCs = bf.output(chain_score_out, (size_t)F * Cr * 4),
              iNm = bf.output(n_mapped_out, (size_t)F * 4), iSd = bf.output(seed_out, (size_t)F * 4), iRd = bf.output(round_out, (size_t)F * 4),
              iRot = bf.output(rotation_out, (size_t)F * 72), iTr = bf.output(translation_out, (size_t)F * 24);
    const int iP = bf.scratch((size_t)chunk * shares * sizeof(CmBest)), iL = bf.scratch((size_t)chunk * shares * cap * 8), iCn = bf.scratch(MAX_C * 4, 0), iBad = bf.scratch((size_t)chunk * 4),
              iRb = bf.scratch(sizeof(int), 0);
    const int rc = bf.upload();
    if (rc == 0) {
        const int* ro = bf.ptr<const int>(iRo);
        const int* rg = bf.ptr<const int>(iRg);
        const int* mo = bf.ptr<const int>(iMo);
        const int* mg = bf.ptr<const int>(iMg);
        hipLaunchKernelGGL(k_cm_ref_counts, dim3((unsigned)Cr), dim3(64), 0, bf.stm, ro, bf.ptr<const float>(iY), bf.ptr<int>(iCn), bf.ptr<int>(iRb));
        for (int64_t f0 = 0; f0 < F; f0 += chunk) {
            const int64_t nf = std::min(chunk, F - f0);
            hipLaunchKernelGGL(k_oligomer_frames, dim3((unsigned)nf), dim3(OLIGOMER_NT), 0, bf.stm, (int)Nm, bf.ptr<const float>(iX) + (size_t)f0 * Nm * 3,
                               bf.ptr<const int>(iRb), bf.ptr<int>(iBad));
            hipLaunchKernelGGL(k_cm_search, dim3((unsigned)(nf * shares)), dim3(NT), 0, bf.stm, shares, (int)Cr, (int)Cm, (int)Nr, (int)Nm, (int)n_iter, d0, scale,
                               (int)cap, ro, rg, mo, mg, bf.ptr<const float>(iY), bf.ptr<const float>(iX) + (size_t)f0 * Nm * 3, bf.ptr<const int>(iBad), bf.ptr<int>(iL),
                               bf.ptr<CmBest>(iP));
            hipLaunchKernelGGL(k_cm_final, dim3((unsigned)nf), dim3(64), 0, bf.stm, shares, (int)Cr, norm_len, bf.ptr<const CmBest>(iP), bf.ptr<const int>(iCn),
                               bf.ptr<float>(iSc) + f0, bf.ptr<int>(iMp) + f0 * Cr, bf.ptr<float>(iCs) + f0 * Cr, bf.ptr<int>(iNm) + f0, bf.ptr<int>(iSd) + f0,
                               bf.ptr<int>(iRd) + f0, bf.ptr<double>(iRot) + f0 * 9, bf.ptr<double>(iTr) + f0 * 3);
        }
    }
    return bf.finish(rc, "chainmap");
}
