// pesto_tmscore.hip - the global fold measures of a model against its reference for a given residue correspondence: TM-score (Zhang and
// Skolnick 2004), GDT-TS and GDT-HA, for every frame of a run or every structure of a ragged batch in one launch.
//
// The C entry point (include/pesto_hip.h) lives here too, on the call plumbing of pesto_call.h, with a message channel of its own.
//
// The measures are maxima over superpositions, found by a search: from every seed window of the sequence the model is fitted onto the
// reference on the window, the points near the reference under that fit become the next set to fit on, until the set repeats. A seed
// is a short data-dependent loop of masked double-precision fits, and seeds are independent, so ONE WAVE runs whole seeds on its own: the
// workgroup stages the L selected points of the frame and of the reference in LDS once (float32, 24 L bytes), then its four waves never
// meet again before they are done. A lane owns the points lane + 64 j and keeps their membership in the set as bit j of one 64-bit word
// (L <= 64 * 64); the masked sums go through the wave's butterfly (kabsch_fit_wave, pesto_fit.h), so every lane holds the same fit and
// the same verdicts. Workgroups share a frame's seeds out; k_tm_final takes the maximum over the shares, ties to the lowest seed, which
// does not depend on how the seeds were shared. No atomics: every output repeats its bits from call to call.
#include <climits>
#include <cmath>

#include "pesto_call.h"
#include "pesto_fit.h"
#include "pesto_tmsearch.h"

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup of k_tm_search
constexpr int NW = NT / 64;             // its waves
constexpr int TARGET_GROUPS = 1024;     // workgroups a call aims at, so that one model still fills the device
constexpr int SEED_NONE = INT_MAX;      // TmBest::seed of a share without seeds
constexpr int SEED_BAD = -1;            // ... of a frame with a non-finite selected coordinate

// the seeds of a structure of L points: the lengths L >> k while above 4, then min(L, 4); the starts 0, step, 2 step, ... <= L - n and
// L - n itself
void plan_seeds(int L, int step, TmStruct& s) {
    s.step = step;
    s.n_len = 0;
    s.n_seeds = 0;
    auto add = [&](int n) {
        const int last = L - n;
        s.len[s.n_len] = n;
        s.cnt[s.n_len] = last / step + 1 + (last % step ? 1 : 0);
        s.n_seeds += s.cnt[s.n_len++];
    };
    for (int k = 0; k <= 5 && (L >> k) > 4; ++k) add(L >> k);
    add(std::min(L, 4));
}

// ------------------------------------------------------------------------------------------------ the search
// replaces: the TMscore program's superposition search, one model per process. Workgroup (unit u, share sh): unit = frame, or structure of
// a ragged batch (n_struct > 1: one frame). Wave w of share sh runs the seeds sh NW + w, + shares NW, ... of its unit.
__global__ __launch_bounds__(NT) void k_tm_search(int shares, int N, int n_struct, int n_iter, int max_raise, double scale,
                                                  const TmStruct* __restrict__ structs, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                  const int* __restrict__ sel, const int* __restrict__ err, TmBest* __restrict__ out) {
    extern __shared__ float s_pts[];            // the frame's L points, then the reference's
    __shared__ TmBest s_best[NW];
    if (*err) return;
    const unsigned u = blockIdx.x / (unsigned)shares, sh = blockIdx.x % (unsigned)shares;
    const TmStruct& S = structs[n_struct > 1 ? u : 0];
    const float* X = xyz + (n_struct > 1 ? (size_t)0 : (size_t)u * N * 3);
    const int L = S.L, step = S.step;
    float* sx = s_pts;
    float* sy = s_pts + 3 * (size_t)L;
    int bad = 0;
    for (int k = threadIdx.x; k < L; k += NT) {
        const size_t a = (size_t)sel[S.s0 + k] * 3;
        for (int c = 0; c < 3; ++c) {
            const float v = X[a + c], w = ref[a + c];
            sx[3 * k + c] = v;
            sy[3 * k + c] = w;
            bad |= !(fabsf(v) <= 3.402823466e38f) || !(fabsf(w) <= 3.402823466e38f);
        }
    }
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0) out[blockIdx.x].seed = SEED_BAD;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const auto px = atoms<true>(sx, nullptr), py = atoms<true>(sy, nullptr);
    const double d0 = S.d0, d_search = S.d_search;
    const int need = L < 3 ? L : 3;
    const double cuts[TM_N_CUT] = {0.5, 1.0, 2.0, 4.0, 8.0};
    TmBest best;
    best.tm = -1.0;
    best.seed = SEED_NONE;
    for (int c = 0; c < 9; ++c) best.R[c] = 0.0;
    for (int c = 0; c < 3; ++c) best.t[c] = 0.0;
    for (int c = 0; c < TM_N_CUT; ++c) best.cnt[c] = 0;

    for (int seed = (int)sh * NW + wave; seed < S.n_seeds; seed += shares * NW) {
        int n = 0, start = 0;
        for (int l = 0, i = seed; l < S.n_len; ++l) {
            if (i < S.cnt[l]) {
                n = S.len[l];
                start = min((long long)i * step, (long long)(L - n));
                break;
            }
            i -= S.cnt[l];
        }
        unsigned long long in = 0ull;
        for (int j = 0, k = lane; k < L; ++j, k += 64)
            if (k >= start && k < start + n) in |= 1ull << j;
        for (int it = 0; it < n_iter; ++it) {
            Fit ft;
            kabsch_fit_wave<true>(px, py, L, in, ft);
            // the points under d_cut (this lane's word, the wave's count) and the smallest distance that is not
            auto members = [&](double d_cut, unsigned long long& word, double& lowest, double* tsum, int* cnt) {
                word = 0ull;
                lowest = INFINITY;
                int ns = 0;
                for (int j = 0, k = lane; k < L; ++j, k += 64) {
                    double x[3], y[3], p[3];
                    px(k, x);
                    py(k, y);
                    moved(x, ft, p);
                    const double e0 = p[0] - y[0], e1 = p[1] - y[1], e2 = p[2] - y[2];
                    const double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2) * scale;
                    if (d < d_cut) { word |= 1ull << j; ++ns; }
                    else lowest = fmin(lowest, d);
                    if (tsum) {
                        const double q = d / d0;
                        *tsum += 1.0 / (1.0 + q * q);
                        for (int c = 0; c < TM_N_CUT; ++c) cnt[c] += d < cuts[c] ? 1 : 0;
                    }
                }
                lowest = wave_min(lowest);
                return wave_sum(ns);
            };
            double d_cut = d_search, lowest, tsum = 0.0;
            int cnt[TM_N_CUT] = {0, 0, 0, 0, 0};
            unsigned long long next;
            int ns = members(d_cut, next, lowest, &tsum, cnt);
            tsum = wave_sum(tsum);                      // (the quotient by L_norm is taken once, in k_tm_final)
            for (int c = 0; c < TM_N_CUT; ++c) best.cnt[c] = max(best.cnt[c], wave_sum(cnt[c]));
            if (tsum > best.tm) {                       // (a wave meets its seeds in ascending order: the first to attain the maximum stays)
                best.tm = tsum;
                best.seed = seed;
                for (int c = 0; c < 9; ++c) best.R[c] = ft.R[c];
                for (int c = 0; c < 3; ++c)
                    best.t[c] = ft.same ? 0.0 : ft.m[3 + c] - ((ft.m[0] * ft.R[c] + ft.m[1] * ft.R[3 + c]) + ft.m[2] * ft.R[6 + c]);
            }
            // too few points under d_cut: raise it by 0.5 until there are enough. Only a d_cut above `lowest` adds a point, so the sets in
            // between are not formed; max_raise bounds the raises of one fit (distances far beyond any structure end the seed instead)
            int raises = 0;
            while (ns < need && raises < max_raise) {
                do { d_cut += 0.5; ++raises; } while (d_cut <= lowest && raises < max_raise);
                ns = members(d_cut, next, lowest, nullptr, nullptr);
            }
            if (ns < need || __ballot(next != in) == 0ull) break;
            in = next;
        }
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; ++w) {
            const TmBest& o = s_best[w];
            for (int c = 0; c < TM_N_CUT; ++c) best.cnt[c] = max(best.cnt[c], o.cnt[c]);
            if (o.tm > best.tm || (o.tm == best.tm && o.seed < best.seed)) {
                const int keep[TM_N_CUT] = {best.cnt[0], best.cnt[1], best.cnt[2], best.cnt[3], best.cnt[4]};
                best = o;
                for (int c = 0; c < TM_N_CUT; ++c) best.cnt[c] = keep[c];
            }
        }
        out[blockIdx.x] = best;
    }
}

// ------------------------------------------------------------------------------------------------ the outputs
// One wave per unit: the maximum TM sum over the unit's shares (ties: the lowest seed), the counts' maxima, the quotients, rounded once.
// A frame with a non-finite selected coordinate: NaN scores and fit, zero counts, seed -1.
__global__ __launch_bounds__(64) void k_tm_final(int shares, int n_struct, const TmStruct* __restrict__ structs, const TmBest* __restrict__ parts,
                                                 const int* __restrict__ err, float* __restrict__ tm_out, float* __restrict__ ts_out,
                                                 float* __restrict__ ha_out, int* __restrict__ counts_out, int* __restrict__ seed_out,
                                                 double* __restrict__ rot_out, double* __restrict__ tr_out) {
    if (*err) return;
    const size_t u = blockIdx.x;
    const TmStruct& S = structs[n_struct > 1 ? u : 0];
    const TmBest* P = parts + u * (size_t)shares;
    const int lane = threadIdx.x;
    const bool bad = P[0].seed == SEED_BAD;             // (every share of the unit saw the same points)
    double tm = -1.0;
    int seed = SEED_NONE, at = 0, cnt[TM_N_CUT] = {0, 0, 0, 0, 0};
    if (!bad)
        for (int s = lane; s < shares; s += 64) {
            const TmBest& o = P[s];
            for (int c = 0; c < TM_N_CUT; ++c) cnt[c] = max(cnt[c], o.cnt[c]);
            if (o.tm > tm || (o.tm == tm && o.seed < seed)) { tm = o.tm; seed = o.seed; at = s; }
        }
    for (int o = 32; o > 0; o >>= 1) {
        const double tm2 = __shfl_xor(tm, o);
        const int seed2 = __shfl_xor(seed, o), at2 = __shfl_xor(at, o);
        if (tm2 > tm || (tm2 == tm && (seed2 < seed || (seed2 == seed && at2 < at)))) { tm = tm2; seed = seed2; at = at2; }
        for (int c = 0; c < TM_N_CUT; ++c) cnt[c] = max(cnt[c], __shfl_xor(cnt[c], o));
    }
    if (lane != 0) return;
    const double nan = NAN, four_L = 4.0 * (double)S.L;
    tm_out[u] = bad ? NAN : (float)(tm / S.lnorm);
    ts_out[u] = bad ? NAN : (float)((double)(cnt[1] + cnt[2] + cnt[3] + cnt[4]) / four_L);
    ha_out[u] = bad ? NAN : (float)((double)(cnt[0] + cnt[1] + cnt[2] + cnt[3]) / four_L);
    for (int c = 0; c < TM_N_CUT; ++c) counts_out[u * TM_N_CUT + c] = bad ? 0 : cnt[c];
    seed_out[u] = bad ? -1 : seed;
    for (int c = 0; c < 9; ++c) rot_out[u * 9 + c] = bad ? nan : P[at].R[c];
    for (int c = 0; c < 3; ++c) tr_out[u * 3 + c] = bad ? nan : P[at].t[c];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ what pesto_structalign.hip shares
// (pesto_tmsearch.h: the structure alignment runs this very search on the pairs it has aligned, round after round)
void tm_plan(int s0, int L, int step, double norm_len, double d0, TmStruct& s) {
    s.s0 = s0;
    s.L = L;
    plan_seeds(L, step, s);
    s.d0 = d0;
    s.lnorm = norm_len;
    s.d_search = std::min(8.0, std::max(4.5, d0));
}

int tm_shares(int seeds_max, int64_t U) {
    return (int)std::min<int64_t>((seeds_max + NW - 1) / NW, std::max<int64_t>(1, (TARGET_GROUPS + U - 1) / U));
}

hipError_t tm_search_launch(hipStream_t stm, int64_t U, int64_t N, int n_struct, int shares, int L_max, int n_iter, double scale, const TmStruct* structs,
                            const float* ref, const float* xyz, const int* sel, const int* err, TmBest* parts, float* tm_out, float* ts_out, float* ha_out,
                            int* counts_out, int* seed_out, double* rot_out, double* tr_out) {
    const size_t smem = (size_t)L_max * 24;
    if (hipError_t e = hipFuncSetAttribute((const void*)k_tm_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)) return e;
    hipLaunchKernelGGL(k_tm_search, dim3((unsigned)(U * shares)), dim3(NT), smem, stm, shares, (int)N, n_struct, n_iter, (int)PESTO_TMSCORE_MAX_RAISE, scale,
                       structs, ref, xyz, sel, err, parts);
    hipLaunchKernelGGL(k_tm_final, dim3((unsigned)U), dim3(64), 0, stm, shares, n_struct, structs, (const TmBest*)parts, err, tm_out, ts_out, ha_out,
                       counts_out, seed_out, rot_out, tr_out);
    return hipSuccess;
}

}  // namespace pesto

using namespace pesto;

const char* pesto_tmscore_last_error(void) { return last_error(); }

int pesto_tmscore(pesto_model* m, int64_t F, int64_t N, int32_t n_struct, const int32_t* sel_offsets, const int32_t* sel, const float* xyz_ref,
                  const float* xyz, const double* norm_len, const double* d0, int32_t step, int32_t n_iter, double scale, float* tm_out,
                  float* gdt_ts_out, float* gdt_ha_out, int32_t* counts_out, float* rmsd_out, int32_t* seed_out, double* rotation_out,
                  double* translation_out, int32_t ptr_kind, void* stream) {
    if (!sel_offsets || !sel || !xyz_ref || !xyz || !norm_len || !d0 || !tm_out || !gdt_ts_out || !gdt_ha_out || !counts_out || !rmsd_out || !seed_out ||
        !rotation_out || !translation_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_TMSCORE_MAX_FRAMES || N < 1 || N > 0x3fffffff) return fail(PESTO_ERR_INVALID, "1 to 2^23 frames and 1 <= N < 2^30 atoms");
    if (n_struct < 1 || n_struct > PESTO_TMSCORE_MAX_FRAMES || (n_struct > 1 && F != 1))
        return fail(PESTO_ERR_INVALID, "1 to 2^23 structures, and one frame where there are several");
    if (step < 1 || n_iter < 1 || n_iter > PESTO_TMSCORE_MAX_ITER) return fail(PESTO_ERR_INVALID, "step >= 1 and 1 <= n_iter <= %d", PESTO_TMSCORE_MAX_ITER);
    if (!(std::isfinite(scale) && scale > 0.0)) return fail(PESTO_ERR_INVALID, "scale must be positive and finite");
    if (sel_offsets[0] != 0) return fail(PESTO_ERR_INVALID, "sel_offsets must start at 0");
    std::vector<TmStruct> st((size_t)n_struct);
    int L_max = 0, seeds_max = 0;
    for (int b = 0; b < n_struct; ++b) {
        const int64_t L = (int64_t)sel_offsets[b + 1] - sel_offsets[b];
        if (L < 3 || L > PESTO_TMSCORE_MAX_LENGTH) return fail(PESTO_ERR_INVALID, "structure %d: 3 to %d selected atoms, got %lld", b, PESTO_TMSCORE_MAX_LENGTH, (long long)L);
        if (!(std::isfinite(norm_len[b]) && norm_len[b] > 0.0) || !(std::isfinite(d0[b]) && d0[b] > 0.0))
            return fail(PESTO_ERR_INVALID, "structure %d: norm_len and d0 must be positive and finite", b);
        TmStruct& s = st[(size_t)b];
        tm_plan(sel_offsets[b], (int)L, step, norm_len[b], d0[b], s);
        L_max = std::max(L_max, s.L);
        seeds_max = std::max(seeds_max, s.n_seeds);
    }
    if (int rc = begin(m, ptr_kind)) return rc;
    const int64_t n_sel = sel_offsets[n_struct], U = n_struct > 1 ? n_struct : F;
    const int shares = tm_shares(seeds_max, U);
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)N * 12), iX = bf.input(xyz, (size_t)F * N * 12), iS = bf.input(sel, (size_t)n_sel * 4);
    const int iT = bf.table(st.data(), st.size() * sizeof(TmStruct));
    const int iTm = bf.output(tm_out, (size_t)U * 4), iTs = bf.output(gdt_ts_out, (size_t)U * 4), iHa = bf.output(gdt_ha_out, (size_t)U * 4),
              iCn = bf.output(counts_out, (size_t)U * TM_N_CUT * 4), iRm = bf.output(rmsd_out, (size_t)U * 4), iSd = bf.output(seed_out, (size_t)U * 4),
              iRo = bf.output(rotation_out, (size_t)U * 72), iTr = bf.output(translation_out, (size_t)U * 24);
    const int iP = bf.scratch((size_t)U * shares * sizeof(TmBest)), iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const IndexLists idx = {{bf.ptr<const int>(iS)}, {n_sel}};
        hipLaunchKernelGGL(k_index_check<NT>, dim3(blocks((size_t)idx.total(), NT)), dim3(NT), 0, bf.stm, (int)N, idx, bf.ptr<int>(iSt));
        rc = hip_ok(tm_search_launch(bf.stm, U, N, (int)n_struct, shares, L_max, (int)n_iter, scale, bf.ptr<const TmStruct>(iT), bf.ptr<const float>(iY),
                                     bf.ptr<const float>(iX), bf.ptr<const int>(iS), bf.ptr<const int>(iSt), bf.ptr<TmBest>(iP), bf.ptr<float>(iTm),
                                     bf.ptr<float>(iTs), bf.ptr<float>(iHa), bf.ptr<int>(iCn), bf.ptr<int>(iSd), bf.ptr<double>(iRo), bf.ptr<double>(iTr)),
                    "tmscore");
    }
    if (rc == 0) {
        // rmsd: pesto_fit_rmsd's kernel on sel for fit and measure, a structure of a ragged batch at a time
        for (int b = 0; b < n_struct; ++b) {
            const int* sl = bf.ptr<const int>(iS) + st[(size_t)b].s0;
            hipLaunchKernelGGL(k_fit_rmsd<NT>, dim3((unsigned)(n_struct > 1 ? 1 : F)), dim3(NT), 0, bf.stm, 1, (int)N, st[(size_t)b].L, st[(size_t)b].L,
                               bf.ptr<const float>(iY), bf.ptr<const float>(iX), sl, sl, bf.ptr<const int>(iSt), scale, bf.ptr<float>(iRm) + b);
        }
    }
    // a refused call writes nothing: the check's verdict is read before any output is copied back
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "tmscore");
    if (rc == 0 && (herr & 1)) rc = fail(PESTO_ERR_INVALID, "tmscore: atom indices of sel must lie in [0, N)");
    return bf.finish(rc, "tmscore");
}
