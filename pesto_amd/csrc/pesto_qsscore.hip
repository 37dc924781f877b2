// pesto_qsscore.hip - the QS-score of assemblies (Bertoni et al. 2017) with the interface contact score ICS, for a given chain mapping or
// for the mapping that maximises it, for every frame of a run or every decoy of a set in one call.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h, with a message channel of their own; the
// sizes, the layout and its check on the host and the frames' scan for infinities are pesto_oligomer.h's, shared with pesto_chainmap.hip.
//
// Everything rests on a per-frame table of chain-pair terms: entry ((a, a'), (b, b')) holds the five weighted sums and the shared
// contact count of reference interface (a, a') under the model chain pair (b, b'). pesto_qsscore fills the Cr (Cr - 1) / 2 entries of
// its mapping, pesto_qsmap every entry of matching groups and then enumerates ALL mappings over the table (k_qs_enum), so the mapping it
// returns is the exact maximum. k_qs_tile fills the table: a workgroup takes one entry and one block of 64 slots of chain a (staged in
// LDS in double, with chain b's), its lanes run over the slots of a' and b' 64 at a time, each wave over 16 of the block's rows. The
// squared distances of a slot pair decide in double whether the pair can matter at all (neither below the cutoff: nothing else is
// computed, which is the fate of nearly every pair of two chains); only then come the square roots, the weights (one exp per side, the
// weight of the smaller distance is selected, never recomputed) and the terms. Sums have one order: a lane over its slot pairs, the
// wave's butterfly, the four waves, then the blocks in ascending order (k_qs_reduce). The totals of one side (Wref, Wmdl, the contact
// counts) come from the same kernel over one side's chain pairs. No atomics on results: every output repeats its bits from call to call.
#include <climits>
#include <cmath>

#include "pesto_fit.h"
#include "pesto_oligomer.h"

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup: four waves
constexpr int NW = NT / 64;
constexpr int RB = 64;                  // slots of the row chain per workgroup of k_qs_tile (the slot block); 16 per wave
constexpr int MAX_C = PESTO_CHAINMAP_MAX_CHAINS;
constexpr int MAX_G = PESTO_CHAINMAP_MAX_GROUP;
constexpr int64_t MAX_CHUNK = 1 << 15;  // frames of one launch (gridDim.y)

// what a workgroup, an entry or a side sums: K doubles and a count
template <int K>
struct QsPart {
    double v[K];
    long long n;
};
using QsEntry = QsPart<5>;              // num, shared, extra, mref, mmdl; n_shared
using QsSide = QsPart<1>;               // sum of w over one side's inter-chain slot pairs; its contacts
enum { E_NUM, E_SHARED, E_EXTRA, E_MREF, E_MMDL };

// the best mapping of a share of the mappings: qs_global, qs_best (-1: none / NaN) and the mapping's index
struct QsCand {
    double global, best;
    long long index;
};

// how a mapping's entries are found in a frame's table: by interface (pesto_qsscore) or by interface and the model chains' ranks
struct QsLookup {
    const int* ibase;                   // [nI] the first entry of an interface, or NULL: entry i is interface i's
    const int* mrank;                   // [Cm] the rank of a model chain within its group
    const int* nmof;                    // [Cr] the model chains of the group of a reference chain
    __device__ __forceinline__ int operator()(int i, int ap, int b, int bp) const { return ibase ? ibase[i] + mrank[b] * nmof[ap] + mrank[bp] : i; }
};

// the enumeration's groups: those present on both sides, in ascending id
struct QsGroups {
    int G;
    const int* nr;                      // [G] reference chains
    const int* nm;                      // [G] model chains
    const int* radix;                   // [G] mappings of the group: max! / (max - min)!
    const int* ref;                     // [G][MAX_G] the reference chains, ascending
    const int* mod;                     // [G][MAX_G]
};

// w(d) for d < 12
__device__ __forceinline__ double qs_weight(double d) {
    if (d <= 5.0) return 1.0;
    const double u = (d - 5.0) / 4.28;
    return exp(-2.0 * (u * u));
}

__device__ __forceinline__ bool better(const QsCand& p, const QsCand& q) {
    return p.global > q.global || (p.global == q.global && (p.best > q.best || (p.best == q.best && p.index < q.index)));
}

// ------------------------------------------------------------------------------------------------ the checks
// ref_bad = the reference has an infinite coordinate
__global__ __launch_bounds__(NT) void k_qs_ref(int Nr, const float* __restrict__ ref, int* __restrict__ ref_bad) {
    int bad = 0;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < (size_t)Nr * 3; k += (size_t)gridDim.x * NT) bad |= fabsf(ref[k]) == INFINITY;
    if (bad) atomicOr(ref_bad, 1);
}

// Every row of the mapping: model chains in [-1, Cm), each at most once (bit 0), of the reference chain's group (bit 1). Every kernel
// but the two scans for infinities returns at once when a bit is set, so nothing dereferences a mapping that was refused and no result
// is written.
__global__ __launch_bounds__(NT) void k_qs_mapcheck(long long rows, int Cr, int Cm, const int* __restrict__ rg, const int* __restrict__ mg,
                                                    const int* __restrict__ mapping, int* __restrict__ err) {
    const long long row = (long long)blockIdx.x * NT + threadIdx.x;
    if (row >= rows) return;
    const int* m = mapping + row * Cr;
    unsigned long long used = 0;
    int e = 0;
    for (int a = 0; a < Cr; ++a) {
        const int b = m[a];
        if (b < -1 || b >= Cm) e |= 1;
        else if (b >= 0) {
            if (used >> b & 1) e |= 1;
            used |= 1ull << b;
            if (rg[a] != mg[b]) e |= 2;
        }
    }
    if (e) atomicOr(err, e);
}

// ------------------------------------------------------------------------------------------------ the table (the hot path)
// replaces: the loop over residue pairs of a QS-score scorer, one decoy and one mapping per run. Workgroup (job, row block) of frame
// blockIdx.y. TWO: job = (interface (ja, jap)[jI], model pair (jb, jbp), or the mapping's where jb is NULL); the entry's six sums over
// the block's rows. Otherwise job = chain pair (ja, jap) of ONE side (Y, offsets ro): the sum of w and the contacts. A job without a model
// pair (-1) gives zeros. lim: the squared distance, in the input's unit and with a margin of 2^-20, above which a slot pair is below
// neither 12 A nor the contact threshold.
template <bool TWO>
__global__ __launch_bounds__(NT) void k_qs_tile(int nrb, int Cr, int map_per_frame, long long f0, const int* __restrict__ ro, const int* __restrict__ mo,
                                                const int* __restrict__ ja, const int* __restrict__ jap, const int* __restrict__ jI,
                                                const int* __restrict__ jb, const int* __restrict__ jbp, const int* __restrict__ mapping,
                                                const float* __restrict__ ref, const float* __restrict__ xyz, long long frame_stride, double scale,
                                                double thr, double lim, const int* __restrict__ err, const int* __restrict__ bad,
                                                QsPart<TWO ? 5 : 1>* __restrict__ out) {
    constexpr int K = TWO ? 5 : 1, D = TWO ? 6 : 3;
    __shared__ double s_row[RB][D];
    __shared__ QsPart<K> s_w[NW];
    if (*err) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y, job = blockIdx.x / (unsigned)nrb, rb = blockIdx.x % (unsigned)nrb;
    if (bad && bad[f]) return;
    QsPart<K>* o = out + ((size_t)f * gridDim.x + blockIdx.x);
    int a, ap, b = 0, bp = 0;
    if (TWO) {
        const int i = jI ? jI[job] : job;
        a = ja[i];
        ap = jap[i];
        if (jb) {
            b = jb[job];
            bp = jbp[job];
        } else {
            const int* m = mapping + (size_t)(map_per_frame ? f0 + f : 0) * Cr;
            b = m[a];
            bp = m[ap];
        }
    } else {
        a = ja[job];
        ap = jap[job];
    }
    const int r0 = ro[a], L = ro[a + 1] - r0, c0 = ro[ap], Lp = ro[ap + 1] - c0, row0 = rb * RB;
    if (row0 >= L) return;                      // (k_qs_reduce reads the blocks a chain has)
    if (TWO && (b < 0 || bp < 0)) {
        if (tid == 0) {
            for (int k = 0; k < K; ++k) o->v[k] = 0.0;
            o->n = 0;
        }
        return;
    }
    const float* Y = TWO ? ref : xyz + (size_t)f * frame_stride;
    const float* X = xyz + (size_t)f * frame_stride;
    const int x0 = TWO ? mo[b] : 0, xc0 = TWO ? mo[bp] : 0;         // (a mapped model chain has its reference chain's slots)
    for (int t = tid; t < RB * 3; t += NT) {
        const int r = t / 3, c = t % 3, row = row0 + r;
        s_row[r][c] = row < L ? (double)Y[(size_t)(r0 + row) * 3 + c] : (double)NAN;
        if (TWO) s_row[r][3 + c] = row < L ? (double)X[(size_t)(x0 + row) * 3 + c] : (double)NAN;
    }
    __syncthreads();
    double acc[K];
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    long long n = 0;
    for (int s0 = 0; s0 < Lp; s0 += 64) {
        const int s = s0 + lane;
        double c1[3], c2[3];
        for (int c = 0; c < 3; ++c) {
            c1[c] = s < Lp ? (double)Y[(size_t)(c0 + s) * 3 + c] : (double)NAN;
            c2[c] = TWO && s < Lp ? (double)X[(size_t)(xc0 + s) * 3 + c] : (double)NAN;
        }
#pragma unroll 4
        for (int k = 0; k < RB / NW; ++k) {
            const double* rw = s_row[wave * (RB / NW) + k];
            const double e0 = rw[0] - c1[0], e1 = rw[1] - c1[1], e2 = rw[2] - c1[2];
            const double t1 = (e0 * e0 + e1 * e1) + e2 * e2;
            if (TWO) {
                const double g0 = rw[3] - c2[0], g1 = rw[4] - c2[1], g2 = rw[5] - c2[2];
                const double t2 = (g0 * g0 + g1 * g1) + g2 * g2;
                if (t1 < lim || t2 < lim) {             // (a NaN compares false)
                    const double d1 = sqrt(t1) * scale, d2 = sqrt(t2) * scale;
                    if (d1 == d1 && d2 == d2) {         // a common slot pair: finite in all four chains
                        const bool in1 = d1 < 12.0, in2 = d2 < 12.0;
                        if (in1 || in2) {
                            const double w1 = in1 ? qs_weight(d1) : 0.0, w2 = in2 ? qs_weight(d2) : 0.0;
                            if (in1 && in2) {
                                const double wm = d1 <= d2 ? w1 : w2;       // w(min(d1, d2)): w does not ascend
                                acc[E_SHARED] += wm;
                                acc[E_NUM] += wm * (1.0 - fabs(d1 - d2) / 12.0);
                            } else {
                                acc[E_EXTRA] += in1 ? w1 : w2;
                            }
                            acc[E_MREF] += w1;
                            acc[E_MMDL] += w2;
                        }
                        n += d1 < thr && d2 < thr ? 1 : 0;
                    }
                }
            } else if (t1 < lim) {
                const double d1 = sqrt(t1) * scale;
                if (d1 < 12.0) acc[0] += qs_weight(d1);
                n += d1 < thr ? 1 : 0;
            }
        }
    }
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    n = wave_sum(n);
    if (lane == 0) {
        for (int k = 0; k < K; ++k) s_w[wave].v[k] = acc[k];
        s_w[wave].n = n;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < K; ++k) {
            double v = s_w[0].v[k];
            for (int w = 1; w < NW; ++w) v += s_w[w].v[k];
            o->v[k] = v;
        }
        long long c = 0;
        for (int w = 0; w < NW; ++w) c += s_w[w].n;
        o->n = c;
    }
}

// E[f][job] = the job's blocks summed in ascending order (a thread per job)
template <int K>
__global__ __launch_bounds__(NT) void k_qs_reduce(int n_jobs, int nrb, const int* __restrict__ ro, const int* __restrict__ ja, const int* __restrict__ jI,
                                                  const int* __restrict__ err, const int* __restrict__ bad, const QsPart<K>* __restrict__ parts,
                                                  QsPart<K>* __restrict__ E) {
    if (*err) return;
    const int job = blockIdx.x * NT + threadIdx.x, f = blockIdx.y;
    if (job >= n_jobs || (bad && bad[f])) return;
    const int a = ja[jI ? jI[job] : job];
    const int nb = (ro[a + 1] - ro[a] + RB - 1) / RB;
    const QsPart<K>* p = parts + ((size_t)f * n_jobs + job) * nrb;
    QsPart<K> s = p[0];
    for (int b = 1; b < nb; ++b) {
        for (int k = 0; k < K; ++k) s.v[k] += p[b].v[k];
        s.n += p[b].n;
    }
    QsPart<K>* o = E + (size_t)f * n_jobs + job;
    for (int k = 0; k < K; ++k) o->v[k] = s.v[k];
    o->n = s.n;
}

// T[f] = one side's chain pairs summed in ascending order (a thread per frame)
__global__ __launch_bounds__(NT) void k_qs_side_total(int frames, int n_jobs, const int* __restrict__ err, const int* __restrict__ bad,
                                                      const QsSide* __restrict__ E, QsSide* __restrict__ T) {
    if (*err) return;
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f >= frames || (bad && bad[f])) return;
    double w = 0.0;
    long long n = 0;
    for (int j = 0; j < n_jobs; ++j) {
        w += E[(size_t)f * n_jobs + j].v[0];
        n += E[(size_t)f * n_jobs + j].n;
    }
    T[f].v[0] = w;
    T[f].n = n;
}

// ------------------------------------------------------------------------------------------------ a mapping's score
struct QsTotal {
    double num, den, mref, mmdl;
    long long n_shared;
};

// the entries of the mapped interfaces summed in ascending (a, a'); m(a) = the model chain under reference chain a
template <class M>
__device__ __forceinline__ QsTotal sum_mapping(int Cr, M m, const QsLookup& at, const QsEntry* __restrict__ E) {
    QsTotal t{0.0, 0.0, 0.0, 0.0, 0};
    int i = 0;
    for (int a = 0; a < Cr; ++a) {
        const int b = m(a);
        if (b < 0) { i += Cr - 1 - a; continue; }
        for (int ap = a + 1; ap < Cr; ++ap, ++i) {
            const int bp = m(ap);
            if (bp < 0) continue;
            const QsEntry& e = E[at(i, ap, b, bp)];
            t.num += e.v[E_NUM];
            t.den += e.v[E_SHARED] + e.v[E_EXTRA];
            t.mref += e.v[E_MREF];
            t.mmdl += e.v[E_MMDL];
            t.n_shared += e.n;
        }
    }
    return t;
}

__device__ __forceinline__ void qs_values(const QsTotal& t, double wref, double wmdl, double& best, double& global) {
    const double dg = t.den + (wref - t.mref) + (wmdl - t.mmdl);
    best = t.den > 0.0 ? t.num / t.den : (double)NAN;
    global = dg > 0.0 ? t.num / dg : (double)NAN;
}

// Mapping `index` of the enumeration: a mixed-radix number over the groups, the lowest group id the least significant digit. A
// group's digit is again mixed-radix over the chains of its side with fewer chains (the reference's on a tie), the first of them the
// least significant: its digit q in [0, max - k) picks the q-th chain, in ascending order, of the other side that is still free.
template <class Set>
__device__ __forceinline__ void qs_decode(int index, int Cr, const QsGroups& gr, Set set) {
    for (int a = 0; a < Cr; ++a) set(a, -1);
    for (int g = 0; g < gr.G; ++g) {
        int d = index % gr.radix[g];
        index /= gr.radix[g];
        const int nr = gr.nr[g], nm = gr.nm[g], few = min(nr, nm), many = max(nr, nm);
        unsigned used = 0;
        for (int k = 0; k < few; ++k) {
            int q = d % (many - k);
            d /= many - k;
            int c = 0;
            for (;; ++c)
                if (!(used >> c & 1) && q-- == 0) break;
            used |= 1u << c;
            if (nr <= nm) set(gr.ref[g * MAX_G + k], gr.mod[g * MAX_G + c]);
            else set(gr.ref[g * MAX_G + c], gr.mod[g * MAX_G + k]);
        }
    }
}

// One wave per frame: the scores and counts of the frame under its mapping, every float rounded once, and interface_qs. A frame with
// an infinite coordinate: NaN and counts of -1.
__global__ __launch_bounds__(64) void k_qs_score(int Cr, int n_entries, int map_per_frame, long long f0, QsLookup at, const int* __restrict__ ja,
                                                 const int* __restrict__ jap, const int* __restrict__ mapping, const QsEntry* __restrict__ E_all,
                                                 const QsSide* __restrict__ Tref, const QsSide* __restrict__ Tmdl, const int* __restrict__ err,
                                                 const int* __restrict__ bad, float* __restrict__ best_out, float* __restrict__ global_out,
                                                 float* __restrict__ ics_out, float* __restrict__ prec_out, float* __restrict__ rec_out,
                                                 int* __restrict__ counts_out, float* __restrict__ iface_out) {
    if (*err) return;
    const int f = blockIdx.x, lane = threadIdx.x;
    const bool isbad = bad[f] != 0;
    const int* m = mapping + (size_t)(map_per_frame ? f0 + f : 0) * Cr;
    const QsEntry* E = E_all + (size_t)f * n_entries;
    float* q = iface_out + (size_t)f * Cr * Cr;
    for (int a = lane; a < Cr; a += 64) q[(size_t)a * Cr + a] = NAN;
    const int nI = Cr * (Cr - 1) / 2;
    for (int i = lane; i < nI; i += 64) {
        const int a = ja[i], ap = jap[i];
        float v = NAN;
        if (!isbad && m[a] >= 0 && m[ap] >= 0) {
            const QsEntry& e = E[at(i, ap, m[a], m[ap])];
            const double den = e.v[E_SHARED] + e.v[E_EXTRA];
            if (den > 0.0) v = (float)(e.v[E_NUM] / den);
        }
        q[(size_t)a * Cr + ap] = v;
        q[(size_t)ap * Cr + a] = v;
    }
    if (lane != 0) return;
    if (isbad) {
        best_out[f] = global_out[f] = ics_out[f] = prec_out[f] = rec_out[f] = NAN;
        for (int c = 0; c < 3; ++c) counts_out[(size_t)f * 3 + c] = -1;
        return;
    }
    const QsTotal t = sum_mapping(Cr, [&](int a) { return m[a]; }, at, E);
    double best, global;
    qs_values(t, Tref[0].v[0], Tmdl[f].v[0], best, global);
    best_out[f] = (float)best;
    global_out[f] = (float)global;
    const long long n_ref = Tref[0].n, n_mdl = Tmdl[f].n, n_sh = t.n_shared;
    ics_out[f] = n_ref + n_mdl > 0 ? (float)(2.0 * (double)n_sh / (double)(n_ref + n_mdl)) : NAN;
    prec_out[f] = n_mdl > 0 ? (float)((double)n_sh / (double)n_mdl) : NAN;
    rec_out[f] = n_ref > 0 ? (float)((double)n_sh / (double)n_ref) : NAN;
    counts_out[(size_t)f * 3 + 0] = (int)min(n_ref, (long long)INT_MAX);
    counts_out[(size_t)f * 3 + 1] = (int)min(n_mdl, (long long)INT_MAX);
    counts_out[(size_t)f * 3 + 2] = (int)min(n_sh, (long long)INT_MAX);
}

// ------------------------------------------------------------------------------------------------ the enumeration
// replaces: a chain mapper's search for the QS-optimal mapping, by exhaustive enumeration where the count allows. A thread per mapping
// of frame blockIdx.y: it decodes its index (the mapping sits in LDS, a column per thread), sums the mapping's entries as k_qs_score
// does, and the workgroup keeps the largest qs_global: ties to the larger qs_best, then to the lowest index. A mapping whose qs_global
// is NaN is no candidate.
__global__ __launch_bounds__(NT) void k_qs_enum(int n_map, int Cr, int n_entries, QsGroups gr, QsLookup at, const QsEntry* __restrict__ E_all,
                                                const QsSide* __restrict__ Tref, const QsSide* __restrict__ Tmdl, const int* __restrict__ err,
                                                const int* __restrict__ bad, QsCand* __restrict__ cand) {
    __shared__ signed char s_m[MAX_C][NT];
    __shared__ QsCand s_c[NW];
    if (*err) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.y;
    const int index = blockIdx.x * NT + tid;
    QsCand c{-1.0, -1.0, LLONG_MAX};
    if (!bad[f] && index < n_map) {
        qs_decode(index, Cr, gr, [&](int a, int b) { s_m[a][tid] = (signed char)b; });
        const QsTotal t = sum_mapping(Cr, [&](int a) { return (int)s_m[a][tid]; }, at, E_all + (size_t)f * n_entries);
        double best, global;
        qs_values(t, Tref[0].v[0], Tmdl[f].v[0], best, global);
        if (global == global) c = QsCand{global, best == best ? best : -1.0, (long long)index};
    }
    for (int o = 32; o > 0; o >>= 1) {
        const QsCand c2{__shfl_xor(c.global, o), __shfl_xor(c.best, o), __shfl_xor(c.index, o)};
        if (better(c2, c)) c = c2;
    }
    if (lane == 0) s_c[wave] = c;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w)
            if (better(s_c[w], c)) c = s_c[w];
        QsCand* o = cand + (size_t)f * gridDim.x + blockIdx.x;
        o->global = c.global;
        o->best = c.best;
        o->index = c.index;
    }
}

// One wave per frame: the best of the frame's workgroups, its mapping decoded. No candidate: mapping -1, n_mapped 0, index -1.
__global__ __launch_bounds__(64) void k_qs_pick(int n_blocks, int Cr, QsGroups gr, const QsCand* __restrict__ cand, const int* __restrict__ err,
                                                const int* __restrict__ bad, int* __restrict__ map_out, int* __restrict__ nmap_out,
                                                long long* __restrict__ index_out) {
    if (*err) return;
    const int f = blockIdx.x, lane = threadIdx.x;
    QsCand c{-1.0, -1.0, LLONG_MAX};
    if (!bad[f])
        for (int k = lane; k < n_blocks; k += 64)
            if (better(cand[(size_t)f * n_blocks + k], c)) c = cand[(size_t)f * n_blocks + k];
    for (int o = 32; o > 0; o >>= 1) {
        const QsCand c2{__shfl_xor(c.global, o), __shfl_xor(c.best, o), __shfl_xor(c.index, o)};
        if (better(c2, c)) c = c2;
    }
    if (lane != 0) return;
    int* m = map_out + (size_t)f * Cr;
    if (c.global < 0.0) {
        for (int a = 0; a < Cr; ++a) m[a] = -1;
        nmap_out[f] = 0;
        index_out[f] = -1;
        return;
    }
    qs_decode((int)c.index, Cr, gr, [&](int a, int b) { m[a] = b; });
    int n = 0;
    for (int a = 0; a < Cr; ++a) n += m[a] >= 0;
    nmap_out[f] = n;
    index_out[f] = c.index;
}

// ------------------------------------------------------------------------------------------------ the host side
// the pairs c < c' of C chains in ascending order
void chain_pairs(int C, std::vector<int>& first, std::vector<int>& second) {
    for (int c = 0; c < C; ++c)
        for (int cp = c + 1; cp < C; ++cp) { first.push_back(c); second.push_back(cp); }
}

template <class T> int table(Buffers& bf, const std::vector<T>& v) { return bf.table(v.data(), v.size() * sizeof(T)); }

// mapping_in: the caller's mapping (pesto_qsscore) or NULL (pesto_qsmap: every mapping is tried and the best comes back)
int qs_run(const char* who, pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
           const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, const int32_t* mapping_in, int64_t mapping_rows,
           double contact_thr, double scale, int32_t* mapping_out, int32_t* n_mapped_out, int64_t* index_out, float* qs_best_out, float* qs_global_out,
           float* ics_out, float* precision_out, float* recall_out, int32_t* counts_out, float* interface_qs_out, int32_t ptr_kind, void* stream) {
    const bool search = !mapping_in;
    if (!ref_offsets || !ref_group || !offsets || !group || !xyz_ref || !xyz || !qs_best_out || !qs_global_out || !ics_out || !precision_out || !recall_out ||
        !counts_out || !interface_qs_out || (search && (!mapping_out || !n_mapped_out || !index_out)))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_oligomer_sizes(F, Nr, Nm, Cr, Cm, scale)) return rc;
    if (!search && mapping_rows != 1 && mapping_rows != F) return fail(PESTO_ERR_INVALID, "mapping_rows must be 1 or F");
    if (!(std::isfinite(contact_thr) && contact_thr > 0.0)) return fail(PESTO_ERR_INVALID, "contact_thr must be positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    // the job lists are made on the host, from the layout as the host holds it
    OligomerLayout lay;
    if (int rc = fetch_layout(who, Nr, Nm, Cr, Cm, ref_offsets, ref_group, offsets, group, ptr_kind, stream, lay)) return rc;
    ref_offsets = lay.ro;
    ref_group = lay.rg;
    offsets = lay.mo;
    group = lay.mg;
    std::vector<int> ref_a, ref_ap, mod_b, mod_bp;      // the interfaces: the reference's chain pairs; and the model's chain pairs
    chain_pairs(Cr, ref_a, ref_ap);
    chain_pairs(Cm, mod_b, mod_bp);
    const int nI = (int)ref_a.size(), nJm = (int)mod_b.size(), nrb = (lay.longest + RB - 1) / RB;     // (the slot blocks of the longest chain)
    // the two-sided jobs: the mapping's interfaces, or every model chain pair of every interface's groups (the pair (b, b) is no job:
    // its entry is never read)
    std::vector<int> jI, jb, jbp, ibase, mrank(Cm), nmof(Cr), g_nr, g_nm, g_radix, g_ref, g_mod;
    int64_t n_map = 1;
    if (search) {
        std::vector<int> mods[PESTO_CHAINMAP_MAX_GROUPS], refs[PESTO_CHAINMAP_MAX_GROUPS];
        for (int b = 0; b < Cm; ++b) { mrank[b] = (int)mods[group[b]].size(); mods[group[b]].push_back(b); }
        for (int a = 0; a < Cr; ++a) refs[ref_group[a]].push_back(a);
        for (int a = 0; a < Cr; ++a) nmof[a] = (int)mods[ref_group[a]].size();
        for (int g = 0; g < PESTO_CHAINMAP_MAX_GROUPS; ++g) {
            const int nr = (int)refs[g].size(), nm = (int)mods[g].size();
            if (!nr || !nm) continue;
            int64_t radix = 1;
            for (int k = 0; k < std::min(nr, nm); ++k) radix *= std::max(nr, nm) - k;          // (at most 12!: no overflow)
            n_map = radix > PESTO_QSSCORE_MAX_MAPPINGS ? (int64_t)PESTO_QSSCORE_MAX_MAPPINGS + 1 : std::min<int64_t>(n_map * radix, (int64_t)PESTO_QSSCORE_MAX_MAPPINGS + 1);
            g_nr.push_back(nr);
            g_nm.push_back(nm);
            g_radix.push_back((int)std::min<int64_t>(radix, INT_MAX));
            for (int k = 0; k < MAX_G; ++k) { g_ref.push_back(k < nr ? refs[g][k] : 0); g_mod.push_back(k < nm ? mods[g][k] : 0); }
        }
        if (n_map > PESTO_QSSCORE_MAX_MAPPINGS)
            return fail(PESTO_ERR_INVALID, "%s: more than 2^20 chain mappings: map the chains with pesto_chainmap and score that mapping with pesto_qsscore", who);
        for (int i = 0; i < nI; ++i) {
            ibase.push_back((int)jI.size());
            for (int b : mods[ref_group[ref_a[i]]])
                for (int bp : mods[ref_group[ref_ap[i]]]) { jI.push_back(i); jb.push_back(b == bp ? -1 : b); jbp.push_back(b == bp ? -1 : bp); }
        }
    }
    const int nJ = search ? (int)jI.size() : nI, G = (int)g_nr.size();
    const int n_blocks = (int)((n_map + NT - 1) / NT);
    // the frames of one launch: their tables and the blocks' sums stay within the workspace
    const int64_t per_frame = (int64_t)nJ * (nrb + 1) * (int64_t)sizeof(QsEntry) + (int64_t)nJm * (nrb + 1) * (int64_t)sizeof(QsSide) + (search ? (int64_t)n_blocks * (int64_t)sizeof(QsCand) : 0) + 64;
    if (per_frame > PESTO_QSSCORE_WORKSPACE) return fail(PESTO_ERR_INVALID, "%s: the tables of one frame exceed the workspace", who);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(F, MAX_CHUNK), (int64_t)PESTO_QSSCORE_WORKSPACE / per_frame));
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)Nr * 12), iX = bf.input(xyz, (size_t)F * Nm * 12);
    const int iMin = search ? -1 : bf.input(mapping_in, (size_t)mapping_rows * Cr * 4);
    const int iRo = bf.table(ref_offsets, (size_t)(Cr + 1) * 4), iRg = bf.table(ref_group, (size_t)Cr * 4), iMo = bf.table(offsets, (size_t)(Cm + 1) * 4),
              iMg = bf.table(group, (size_t)Cm * 4);
    const int iIa = table(bf, ref_a), iIap = table(bf, ref_ap), iMa = table(bf, mod_b), iMap = table(bf, mod_bp);
    const int iJI = table(bf, jI), iJb = table(bf, jb), iJbp = table(bf, jbp), iIb = table(bf, ibase), iMr = table(bf, mrank), iNo = table(bf, nmof);
    const int iGr = table(bf, g_nr), iGm = table(bf, g_nm), iGx = table(bf, g_radix), iGf = table(bf, g_ref), iGd = table(bf, g_mod);
    const int iMp = search ? bf.output(mapping_out, (size_t)F * Cr * 4) : -1, iNm = search ? bf.output(n_mapped_out, (size_t)F * 4) : -1,
              iIx = search ? bf.output(index_out, (size_t)F * 8) : -1;
    const int iQb = bf.output(qs_best_out, (size_t)F * 4), iQg = bf.output(qs_global_out, (size_t)F * 4), iIc = bf.output(ics_out, (size_t)F * 4),
              iPr = bf.output(precision_out, (size_t)F * 4), iRc = bf.output(recall_out, (size_t)F * 4), iCn = bf.output(counts_out, (size_t)F * 12),
              iIq = bf.output(interface_qs_out, (size_t)F * Cr * Cr * 4);
    const int iP2 = bf.scratch((size_t)chunk * nJ * nrb * sizeof(QsEntry)), iE2 = bf.scratch((size_t)chunk * nJ * sizeof(QsEntry)),
              iPm = bf.scratch((size_t)chunk * nJm * nrb * sizeof(QsSide)), iEm = bf.scratch((size_t)chunk * nJm * sizeof(QsSide)),
              iTm = bf.scratch((size_t)chunk * sizeof(QsSide)), iPr1 = bf.scratch((size_t)nI * nrb * sizeof(QsSide)), iEr = bf.scratch((size_t)nI * sizeof(QsSide)),
              iTr = bf.scratch(sizeof(QsSide)), iCd = bf.scratch(search ? (size_t)chunk * n_blocks * sizeof(QsCand) : 0), iBad = bf.scratch((size_t)chunk * 4),
              iRb = bf.scratch(sizeof(int), 0), iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const int* ro = bf.ptr<const int>(iRo);
        const int* mo = bf.ptr<const int>(iMo);
        const int* ia = bf.ptr<const int>(iIa);
        const int* iap = bf.ptr<const int>(iIap);
        const int* st = bf.ptr<const int>(iSt);
        const int* rbad = bf.ptr<const int>(iRb);
        const int* fbad = bf.ptr<const int>(iBad);
        const float* Y = bf.ptr<const float>(iY);
        const double cut = std::max(12.0, contact_thr) / scale, lim = cut * cut * (1.0 + 1.0 / 1048576.0);
        const int* map_dev = search ? bf.ptr<const int>(iMp) : bf.ptr<const int>(iMin);
        const int per_frame_map = search || mapping_rows > 1 ? 1 : 0;
        const QsLookup at{search ? bf.ptr<const int>(iIb) : nullptr, bf.ptr<const int>(iMr), bf.ptr<const int>(iNo)};
        const QsGroups gr{G, bf.ptr<const int>(iGr), bf.ptr<const int>(iGm), bf.ptr<const int>(iGx), bf.ptr<const int>(iGf), bf.ptr<const int>(iGd)};
        hipLaunchKernelGGL(k_qs_ref, dim3(std::min(1024u, blocks((size_t)Nr * 3, NT))), dim3(NT), 0, bf.stm, (int)Nr, Y, bf.ptr<int>(iRb));
        if (!search)
            hipLaunchKernelGGL(k_qs_mapcheck, dim3(blocks((size_t)mapping_rows, NT)), dim3(NT), 0, bf.stm, (long long)mapping_rows, (int)Cr, (int)Cm,
                               bf.ptr<const int>(iRg), bf.ptr<const int>(iMg), map_dev, bf.ptr<int>(iSt));
        // the reference's totals, once
        if (nI > 0) {
            hipLaunchKernelGGL(k_qs_tile<false>, dim3((unsigned)(nI * nrb), 1), dim3(NT), 0, bf.stm, nrb, (int)Cr, 0, 0ll, ro, ro, ia, iap, (const int*)nullptr,
                               (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, Y, Y, 0ll, scale, contact_thr, lim, st, (const int*)nullptr,
                               bf.ptr<QsSide>(iPr1));
            hipLaunchKernelGGL(k_qs_reduce<1>, dim3(blocks((size_t)nI, NT), 1), dim3(NT), 0, bf.stm, nI, nrb, ro, ia, (const int*)nullptr, st, (const int*)nullptr,
                               bf.ptr<const QsSide>(iPr1), bf.ptr<QsSide>(iEr));
        }
        hipLaunchKernelGGL(k_qs_side_total, dim3(1), dim3(NT), 0, bf.stm, 1, nI, st, (const int*)nullptr, bf.ptr<const QsSide>(iEr), bf.ptr<QsSide>(iTr));
        for (int64_t f0 = 0; f0 < F; f0 += chunk) {
            const unsigned nf = (unsigned)std::min(chunk, F - f0);
            const float* X = bf.ptr<const float>(iX) + (size_t)f0 * Nm * 3;
            hipLaunchKernelGGL(k_oligomer_frames, dim3(nf), dim3(OLIGOMER_NT), 0, bf.stm, (int)Nm, X, rbad, bf.ptr<int>(iBad));
            if (nJm > 0) {
                hipLaunchKernelGGL(k_qs_tile<false>, dim3((unsigned)(nJm * nrb), nf), dim3(NT), 0, bf.stm, nrb, (int)Cr, 0, 0ll, mo, mo, bf.ptr<const int>(iMa),
                                   bf.ptr<const int>(iMap), (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, X, X,
                                   (long long)Nm * 3, scale, contact_thr, lim, st, fbad, bf.ptr<QsSide>(iPm));
                hipLaunchKernelGGL(k_qs_reduce<1>, dim3(blocks((size_t)nJm, NT), nf), dim3(NT), 0, bf.stm, nJm, nrb, mo, bf.ptr<const int>(iMa), (const int*)nullptr, st,
                                   fbad, bf.ptr<const QsSide>(iPm), bf.ptr<QsSide>(iEm));
            }
            hipLaunchKernelGGL(k_qs_side_total, dim3(blocks(nf, NT)), dim3(NT), 0, bf.stm, (int)nf, nJm, st, fbad, bf.ptr<const QsSide>(iEm), bf.ptr<QsSide>(iTm));
            if (nJ > 0) {
                hipLaunchKernelGGL(k_qs_tile<true>, dim3((unsigned)(nJ * nrb), nf), dim3(NT), 0, bf.stm, nrb, (int)Cr, per_frame_map, (long long)f0, ro, mo, ia, iap,
                                   search ? bf.ptr<const int>(iJI) : nullptr, search ? bf.ptr<const int>(iJb) : nullptr,
                                   search ? bf.ptr<const int>(iJbp) : nullptr, search ? nullptr : map_dev, Y, X, (long long)Nm * 3, scale, contact_thr, lim, st,
                                   fbad, bf.ptr<QsEntry>(iP2));
                hipLaunchKernelGGL(k_qs_reduce<5>, dim3(blocks((size_t)nJ, NT), nf), dim3(NT), 0, bf.stm, nJ, nrb, ro, ia, search ? bf.ptr<const int>(iJI) : nullptr, st,
                                   fbad, bf.ptr<const QsEntry>(iP2), bf.ptr<QsEntry>(iE2));
            }
            if (search) {
                hipLaunchKernelGGL(k_qs_enum, dim3((unsigned)n_blocks, nf), dim3(NT), 0, bf.stm, (int)n_map, (int)Cr, nJ, gr, at, bf.ptr<const QsEntry>(iE2),
                                   bf.ptr<const QsSide>(iTr), bf.ptr<const QsSide>(iTm), st, fbad, bf.ptr<QsCand>(iCd));
                hipLaunchKernelGGL(k_qs_pick, dim3(nf), dim3(64), 0, bf.stm, n_blocks, (int)Cr, gr, bf.ptr<const QsCand>(iCd), st, fbad,
                                   bf.ptr<int>(iMp) + f0 * Cr, bf.ptr<int>(iNm) + f0, bf.ptr<long long>(iIx) + f0);
            }
            hipLaunchKernelGGL(k_qs_score, dim3(nf), dim3(64), 0, bf.stm, (int)Cr, nJ, per_frame_map, (long long)f0, at, ia, iap, map_dev, bf.ptr<const QsEntry>(iE2),
                               bf.ptr<const QsSide>(iTr), bf.ptr<const QsSide>(iTm), st, fbad, bf.ptr<float>(iQb) + f0, bf.ptr<float>(iQg) + f0, bf.ptr<float>(iIc) + f0,
                               bf.ptr<float>(iPr) + f0, bf.ptr<float>(iRc) + f0, bf.ptr<int>(iCn) + f0 * 3, bf.ptr<float>(iIq) + f0 * Cr * Cr);
        }
    }
    // a refused call writes nothing: the check's verdict is read before any output is copied back
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, who);
    if (rc == 0 && (herr & 1)) rc = fail(PESTO_ERR_INVALID, "%s: a mapping holds model chains in [-1, %d), each at most once", who, (int)Cm);
    else if (rc == 0 && (herr & 2)) rc = fail(PESTO_ERR_INVALID, "%s: a mapping joins chains of one group only", who);
    return bf.finish(rc, who);
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_qsscore_last_error(void) { return last_error(); }

int pesto_qsscore(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                  const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, const int32_t* mapping, int64_t mapping_rows,
                  double contact_thr, double scale, float* qs_best_out, float* qs_global_out, float* ics_out, float* precision_out, float* recall_out,
                  int32_t* counts_out, float* interface_qs_out, int32_t ptr_kind, void* stream) {
    if (!mapping) return fail(PESTO_ERR_INVALID, "bad arguments");
    return qs_run("qsscore", m, F, Nr, Nm, Cr, Cm, ref_offsets, ref_group, offsets, group, xyz_ref, xyz, mapping, mapping_rows, contact_thr, scale, nullptr, nullptr,
                  nullptr, qs_best_out, qs_global_out, ics_out, precision_out, recall_out, counts_out, interface_qs_out, ptr_kind, stream);
}

int pesto_qsmap(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, double contact_thr, double scale, int32_t* mapping_out,
                int32_t* n_mapped_out, int64_t* index_out, float* qs_best_out, float* qs_global_out, float* ics_out, float* precision_out, float* recall_out,
                int32_t* counts_out, float* interface_qs_out, int32_t ptr_kind, void* stream) {
    return qs_run("qsmap", m, F, Nr, Nm, Cr, Cm, ref_offsets, ref_group, offsets, group, xyz_ref, xyz, nullptr, 0, contact_thr, scale, mapping_out, n_mapped_out,
                  index_out, qs_best_out, qs_global_out, ics_out, precision_out, recall_out, counts_out, interface_qs_out, ptr_kind, stream);
}
