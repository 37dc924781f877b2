// pesto_lddt.hip - lDDT (Mariani et al. 2013), the superposition-free, per-residue measure of how well a model or an MD frame keeps the
// distances of a reference structure: for every residue the share of its reference pairs (atoms of other residues within r_incl in the
// reference) whose distance in the frame differs from the reference's by less than each of T thresholds.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h, with a message channel of their own.
//
// The distance is the docking group's, d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale) (dist2 of pesto_geom.h, the root through
// double, which rounds correctly for a float32 argument). A call has two parts:
//   the reference list, once: the cell grid of pesto_cellgrid.h at r_incl / scale (one grid per structure of a ragged batch), a count pass
//     over for_each_neighbour, the 64-bit scan (k_list_offsets) and a fill pass give a CSR list over the atoms in the caller's numbering:
//     row i holds (j, d_ref(i, j)) of every pair of atom i. The order within a row is whatever the fill pass meets (the grid's scatter is
//     not ordered); every result below is an integer sum over a row, so it does not matter. A residue's rows are reached through the
//     atoms' order by residue (perm, res_offsets), so its atoms need not be adjacent;
//   the scoring, one launch over all frames: a wave owns one (frame, residue), walks the residue's atoms, puts its 64 lanes across the
//     row's entries, gathers x_j of the frame, forms d and |d - d_ref|, compares with the T thresholds and counts the wave's ballots in
//     integer registers; lane 0 stores preserved[f, r, 0..T). The four waves of a workgroup take four consecutive residues.
// A last launch, one workgroup per (structure, frame), sums the residues' counts in int64 and writes the two quotients. No atomics of
// any kind besides the grid's own cell counters and the error word, no floating-point sums: every output repeats its bits.
#include <cmath>

#include "pesto_call.h"
#include "pesto_cellgrid.h"
#include "pesto_geom.h"

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup of every kernel here
constexpr int NW = NT / 64;             // its waves
constexpr int MAX_T = PESTO_LDDT_MAX_THRESHOLDS;
constexpr unsigned MAX_SCORE_BLOCKS = 1u << 20;        // the scoring launch strides over its (frame, residue group) items beyond this

enum { MODE_ALL = 0, MODE_INTER = 1, MODE_INTRA = 2 };
enum { ERR_RES = 1, ERR_PERM = 2, ERR_ROFF = 4, ERR_STRUCT = 8, ERR_OFF = 16, ERR_J = 32 };

struct Thresholds { float t[MAX_T]; };

// the distance of the definition from the float32 squared distance (the double root of a float32 argument rounds to the correctly
// rounded float32 root)
__device__ __forceinline__ float scaled_dist(float s, float scale) { return __fmul_rn((float)sqrt((double)s), scale); }

// ------------------------------------------------------------------------------------------------ the index check
// Every index is validated before anything dereferences it (error bits in st->err; the host reads them before the next launch, so a
// refused call writes nothing):
//   res_of_atom in [0, R); res_offsets a non-decreasing split of [0, N] into R ranges; perm in [0, N) with perm[k]'s residue the one
//   whose range holds k; every atom of a residue in the structure whose residue range (res_struct_offsets) holds the residue; and for a
//   list that the caller passes: offsets a non-decreasing int64 [N + 1] from 0 to K, j in [0, N).
// chain_of_atom and sel are per-atom values that are only compared: they have no invalid value.
__global__ __launch_bounds__(NT) void k_lddt_check(int N, int R, int n_struct, long long K, const int* __restrict__ struct_offsets,
                                                   const int* __restrict__ res_struct_offsets, const int* __restrict__ res_of_atom,
                                                   const int* __restrict__ perm, const int* __restrict__ roff, const long long* __restrict__ off,
                                                   const int* __restrict__ jn, ListState* __restrict__ st) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    int bits = 0;
    if (k < N) {
        const int r_own = res_of_atom[k];
        if (r_own < 0 || r_own >= R) bits |= ERR_RES;
        const int i = perm[k];
        if (i < 0 || i >= N) bits |= ERR_PERM;
        else {
            const int r = struct_of((int)k, R, roff);          // reads roff[0 .. R] only, whatever it holds
            if (res_of_atom[i] != r) bits |= ERR_PERM;
            const int s = struct_of(i, n_struct, struct_offsets);
            if (r < res_struct_offsets[s] || r >= res_struct_offsets[s + 1]) bits |= ERR_STRUCT;
        }
    }
    if (k < R && roff[k] > roff[k + 1]) bits |= ERR_ROFF;
    if (k == 0 && (roff[0] != 0 || roff[R] != N)) bits |= ERR_ROFF;
    if (off) {
        if (k < N && (off[k] < 0 || off[k] > off[k + 1] || off[k + 1] > K)) bits |= ERR_OFF;
        if (k == 0 && (off[0] != 0 || off[N] != K)) bits |= ERR_OFF;
        if (k < K && (jn[k] < 0 || jn[k] >= N)) bits |= ERR_J;
    }
    if (bits) atomicOr(&st->err, bits);
}

// ------------------------------------------------------------------------------------------------ the reference list
// beside the sorted coordinates: (residue row, or -1 for an atom outside the selection or without finite coordinates; chain)
struct MetaPayload {
    const int* res; const int* chain; const unsigned char* sel; int2* meta;
    __device__ void operator()(int pos, int i) const { meta[pos] = make_int2(sel && !sel[i] ? -1 : res[i], chain ? chain[i] : 0); }
};

// The grid is built on a copy of the reference in which every atom with a non-finite coordinate is marked as outside the selection
// and sits on the first finite atom of its structure (the origin for a structure without one): such an atom has no pairs by the
// definition, and the grid's bounding box (grid_build's set-up) then only ever sees finite coordinates and is no larger than the finite atoms'
// own. k_lddt_anchor, one workgroup per structure: anchor[s] = the first atom with three finite coordinates, or -1.
__global__ __launch_bounds__(NT) void k_lddt_anchor(const int* __restrict__ offsets, const float* __restrict__ Y, int* __restrict__ anchor) {
    __shared__ int first[NT];
    const int s0 = offsets[blockIdx.x], s1 = offsets[blockIdx.x + 1];
    int mine = 0x7fffffff;
    for (int i = s0 + threadIdx.x; i < s1 && mine == 0x7fffffff; i += NT)
        if (finite3(Y + 3 * (size_t)i)) mine = i;
    first[threadIdx.x] = mine;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) first[threadIdx.x] = min(first[threadIdx.x], first[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) anchor[blockIdx.x] = first[0] == 0x7fffffff ? -1 : first[0];
}

// keep[i] = selected and finite. The pass reads every atom anyway, so it also refuses a negative residue row (the list's -1 means
// "outside the selection"): error bit ERR_RES.
__global__ __launch_bounds__(NT) void k_lddt_clean(int N, int n_struct, const int* __restrict__ offsets, const int* __restrict__ anchor,
                                                   const float* __restrict__ Y, const int* __restrict__ res, const unsigned char* __restrict__ sel,
                                                   float* __restrict__ Yc, unsigned char* __restrict__ keep, ListState* __restrict__ st) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    if (res[i] < 0) atomicOr(&st->err, ERR_RES);
    const bool finite = finite3(Y + 3 * (size_t)i);
    const int a = finite ? i : anchor[struct_of(i, n_struct, offsets)];
#pragma unroll
    for (int c = 0; c < 3; ++c) Yc[3 * (size_t)i + c] = a < 0 ? 0.f : Y[3 * (size_t)a + c];
    keep[i] = finite && (!sel || sel[i]) ? 1 : 0;
}

// one thread per atom in cell order. Atom i's pairs are the atoms j != i of its structure, both selected, of another residue, (of
// another / the same chain,) with d_ref < r_incl, decided on the squared distance against s_star, the smallest float at which the test
// fails (contact_threshold of pesto_geom.h: the root and the product are monotonic); a NaN passes no test. FILL false: cnt[i] = their number. FILL true: they go to the row off[i] .. off[i + 1] in the order met.
template <bool FILL>
__global__ __launch_bounds__(NT) void k_lddt_list(int n_total, int n_struct, const int* __restrict__ offsets, const CellGrid* __restrict__ grids,
                                                  const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                  const int2* __restrict__ meta, int mode, float s_star, float scale, int* __restrict__ cnt,
                                                  const long long* __restrict__ off, int* __restrict__ jn, float* __restrict__ dref) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= n_total) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    const int2 own = meta[p];
    int n = 0;
    if (own.x >= 0) {
        const int s = struct_of(p, n_struct, offsets);
        const long long base = FILL ? off[i] : 0;
        for_each_neighbour(grids[s], cell_start, offsets[s], a, [&](int q) {
            const int2 mq = meta[q];
            if (q == p || mq.x < 0 || mq.x == own.x) return;
            if (mode == MODE_INTER && mq.y == own.y) return;
            if (mode == MODE_INTRA && mq.y != own.y) return;
            const float4 b = sorted[q];
            const float s2 = dist2(a.x, a.y, a.z, b.x, b.y, b.z);
            if (s2 < s_star) {                                          // d_ref < r_incl exactly (NaN: false)
                if (FILL) { jn[base + n] = __float_as_int(b.w); dref[base + n] = scaled_dist(s2, scale); }
                ++n;
            }
        });
    }
    if (!FILL) cnt[i] = n;
}

// total[r]: the entries of the rows of residue r's atoms; n_pairs[s]: those of structure s (threads R .. R + n_struct - 1)
__global__ __launch_bounds__(NT) void k_lddt_total(int R, int n_struct, const int* __restrict__ struct_offsets, const int* __restrict__ perm,
                                                   const int* __restrict__ roff, const long long* __restrict__ off, int* __restrict__ total,
                                                   long long* __restrict__ n_pairs) {
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r < R) {
        long long t = 0;
        for (int a = roff[r]; a < roff[r + 1]; ++a) t += off[perm[a] + 1] - off[perm[a]];
        total[r] = (int)t;                                              // K <= 2^30
    } else if (r < R + n_struct) {
        const int s = r - R;
        n_pairs[s] = off[struct_offsets[s + 1]] - off[struct_offsets[s]];
    }
}

// ------------------------------------------------------------------------------------------------ the scoring
// An item is (frame, group of NW residues); wave w of the workgroup owns residue NW * group + w of the frame. The residue's atoms are
// taken 64 at a time, one per lane (index, row bounds, coordinates of the frame), and handed to the whole wave by a lane broadcast, so
// that walking from atom to atom waits for no load. The 64 lanes lie across a row's entries, UNROLL chunks of 64 at a time: the loads
// of (j, d_ref) of all of them are issued before the gathers of x_j, those before the arithmetic. A lane beyond the row's end (the last
// chunks of a row are partial) gathers the atom itself and counts nothing; a chunk wholly beyond it is skipped by the wave. The counts
// are taken per comparison from the wave's ballot (one vector compare each, the popcount and the sum on the scalar unit), so they are
// the same in every lane and need no reduction. TT: the comparisons made per pair, 4 or 8 (T of them count).
constexpr int UNROLL = 4;

template <int TT>
__global__ __launch_bounds__(NT) void k_lddt_score(long long n_items, int groups, int N, int R, int T, Thresholds thr, float scale,
                                                   const float* __restrict__ xyz, const int* __restrict__ perm, const int* __restrict__ roff,
                                                   const long long* __restrict__ off, const int* __restrict__ jn, const float* __restrict__ dref,
                                                   int* __restrict__ preserved) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const long long f = item / groups;
        const int r = (int)(item - f * groups) * NW + wave;
        if (r >= R) continue;                                           // (the whole wave)
        const float* X = xyz + (size_t)f * (size_t)N * 3;
        int cnt[TT];
#pragma unroll
        for (int k = 0; k < TT; ++k) cnt[k] = 0;
        const int a_end = roff[r + 1];
        for (int a0 = roff[r]; a0 < a_end; a0 += 64) {
            const int na = min(64, a_end - a0);
            int li = 0;
            long long le0 = 0, le1 = 0;
            float lx = 0.f, ly = 0.f, lz = 0.f;
            if (lane < na) {
                li = perm[a0 + lane];
                le0 = off[li];
                le1 = off[li + 1];
                lx = X[3 * (size_t)li]; ly = X[3 * (size_t)li + 1]; lz = X[3 * (size_t)li + 2];
            }
            for (int t = 0; t < na; ++t) {
                const size_t i = (size_t)__shfl(li, t);
                const long long e1 = __shfl(le1, t);
                const float xi = __shfl(lx, t), yi = __shfl(ly, t), zi = __shfl(lz, t);
                for (long long e = __shfl(le0, t); e < e1; e += 64 * UNROLL) {
                    int jj[UNROLL];
                    float dd[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const long long q = e + 64 * u + lane;
                        const bool in = q < e1;
                        jj[u] = -1;
                        dd[u] = 0.f;
                        if (e + 64 * u < e1) {                          // (the whole wave)
                            jj[u] = in ? jn[q] : -1;
                            dd[u] = in ? dref[q] : 0.f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        if (e + 64 * u >= e1) break;                    // (the whole wave)
                        const float* b = X + 3 * (jj[u] < 0 ? i : (size_t)jj[u]);
                        const float d = scaled_dist(dist2(xi, yi, zi, b[0], b[1], b[2]), scale);
                        const float gap = fabsf(__fsub_rn(d, dd[u]));   // (NaN where the frame lacks an atom: below no threshold)
#pragma unroll
                        for (int k = 0; k < TT; ++k) cnt[k] += __popcll(__ballot(jj[u] >= 0 && gap < thr.t[k]));
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < TT; ++k)                                    // (fully unrolled: the counters stay in registers)
            if (lane == 0 && k < T) preserved[((size_t)f * R + r) * T + k] = cnt[k];
    }
}

// ------------------------------------------------------------------------------------------------ the totals
// one workgroup per (structure, frame): residue[f, r] = float32(double(sum_k preserved[f, r, k]) / double(T total[r])) for the
// structure's residues, NaN where total[r] = 0; score[f, s] the same quotient over the int64 sums, NaN for a structure without pairs
__global__ __launch_bounds__(NT) void k_lddt_final(int n_struct, int R, int T, const int* __restrict__ res_struct_offsets,
                                                   const int* __restrict__ total, const int* __restrict__ preserved, float* __restrict__ residue,
                                                   float* __restrict__ score) {
    __shared__ long long red[2][NW];
    const int s = blockIdx.x % n_struct;
    const size_t f = blockIdx.x / n_struct;
    const float qnan = __int_as_float(0x7fc00000);
    long long kept = 0, all = 0;
    for (int r = res_struct_offsets[s] + threadIdx.x; r < res_struct_offsets[s + 1]; r += NT) {
        const int* p = preserved + (f * R + r) * T;
        long long k = 0;
        for (int t = 0; t < T; ++t) k += p[t];
        const long long n = (long long)T * total[r];
        residue[f * R + r] = n ? (float)__ddiv_rn((double)k, (double)n) : qnan;
        kept += k;
        all += n;
    }
    for (int o = 32; o > 0; o >>= 1) { kept += __shfl_xor(kept, o); all += __shfl_xor(all, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kept; red[1][threadIdx.x >> 6] = all; }
    __syncthreads();
    if (threadIdx.x == 0) {
        kept = all = 0;
        for (int w = 0; w < NW; ++w) { kept += red[0][w]; all += red[1][w]; }
        score[f * n_struct + s] = all ? (float)__ddiv_rn((double)kept, (double)all) : qnan;
    }
}

// ---- host side
// the error of a refused call from the check kernel's bits (0: none)
int index_error(int err, const char* what) {
    if (err & ERR_RES) return fail(PESTO_ERR_INVALID, "%s: res_of_atom must lie in [0, R) (lddt_pairs: must not be negative)", what);
    if (err & ERR_ROFF) return fail(PESTO_ERR_INVALID, "%s: res_offsets must split [0, N] into R ordered ranges", what);
    if (err & ERR_PERM) return fail(PESTO_ERR_INVALID, "%s: perm must hold the atoms in [0, N) ordered by residue row as res_offsets has them", what);
    if (err & ERR_STRUCT) return fail(PESTO_ERR_INVALID, "%s: a residue's atoms must lie in the structure that res_struct_offsets gives the residue", what);
    if (err & ERR_OFF) return fail(PESTO_ERR_INVALID, "%s: the list's offsets must ascend from 0 to K over the N atoms", what);
    if (err & ERR_J) return fail(PESTO_ERR_INVALID, "%s: the list's partners must lie in [0, N)", what);
    return 0;
}

// what the two entry points share of their arguments' checks
int check_common(int64_t N, int32_t n_struct, const int32_t* struct_offsets, int32_t mode, const int32_t* chain, float r_incl, double scale) {
    if (N < 1 || N > 0x3fffffff || n_struct < 1 || n_struct > N) return fail(PESTO_ERR_INVALID, "1 <= N < 2^30 atoms in 1 to N structures");
    if (mode != MODE_ALL && mode != MODE_INTER && mode != MODE_INTRA) return fail(PESTO_ERR_INVALID, "mode must be 0 (all), 1 (inter) or 2 (intra)");
    if (mode != MODE_ALL && !chain) return fail(PESTO_ERR_INVALID, "mode inter / intra needs chain_of_atom");
    const float fscale = (float)scale;
    if (!std::isfinite(r_incl) || !(r_incl > 0.f) || !std::isfinite(scale) || !std::isfinite(fscale) || !(fscale > 0.f) ||
        !std::isfinite(r_incl / fscale) || !(r_incl / fscale > 0.f))
        return fail(PESTO_ERR_INVALID, "r_incl and scale must be positive and finite");
    return check_offsets(struct_offsets, n_struct, N, "struct_offsets");
}

// the scratch of the list's set-up inside a call's block
struct ListScratch { int iG, iCnt, iCur, iCell, iSort, iMeta, iRow, iClean, iKeep, iAnchor; };

ListScratch list_scratch(Buffers& bf, size_t n, size_t n_struct) {
    const size_t cells = cells_before(n, n_struct);
    ListScratch ls;
    ls.iG = bf.scratch(n_struct * sizeof(CellGrid));
    ls.iCnt = bf.scratch(cells * 4);
    ls.iCur = bf.scratch(cells * 4);
    ls.iCell = bf.scratch(n * 4);
    ls.iSort = bf.scratch(n * 16);
    ls.iMeta = bf.scratch(n * 8);
    ls.iRow = bf.scratch(n * 4);
    ls.iClean = bf.scratch(n * 12);
    ls.iKeep = bf.scratch(n);
    ls.iAnchor = bf.scratch(n_struct * 4);
    return ls;
}

// the grid, the count pass and the scan: off[0 .. N] (item iO) and K (read back; the stream is synchronised)
int list_count(Buffers& bf, const ListScratch& ls, int N, int n_struct, const int* offs, const float* ref, const int* res, const int* chain,
               const unsigned char* sel, int mode, float r_incl, float scale, float s_star, int iO, int iSt, long long* K, const char* what) {
    const int nb = (int)blocks((size_t)N, NT);
    CellGrid* g = bf.ptr<CellGrid>(ls.iG);
    int* cell_cnt = bf.ptr<int>(ls.iCnt);
    float* clean = bf.ptr<float>(ls.iClean);
    unsigned char* keep = bf.ptr<unsigned char>(ls.iKeep);
    hipLaunchKernelGGL(k_lddt_anchor, dim3(n_struct), dim3(NT), 0, bf.stm, offs, ref, bf.ptr<int>(ls.iAnchor));
    hipLaunchKernelGGL(k_lddt_clean, dim3(nb), dim3(NT), 0, bf.stm, N, n_struct, offs, (const int*)bf.ptr<int>(ls.iAnchor), ref, res, sel, clean, keep,
                       bf.ptr<ListState>(iSt));
    ref = clean;
    grid_build(bf.stm, N, n_struct, offs, ref, r_incl / scale, GridBufs{g, cell_cnt, bf.ptr<int>(ls.iCur), bf.ptr<int>(ls.iCell), bf.ptr<float4>(ls.iSort)},
               NoCheck{}, MetaPayload{res, chain, keep, bf.ptr<int2>(ls.iMeta)});
    hipLaunchKernelGGL(k_lddt_list<false>, dim3(nb), dim3(NT), 0, bf.stm, N, n_struct, offs, (const CellGrid*)g, (const int*)cell_cnt,
                       (const float4*)bf.ptr<float4>(ls.iSort), (const int2*)bf.ptr<int2>(ls.iMeta), mode, s_star, scale, bf.ptr<int>(ls.iRow),
                       (const long long*)nullptr, (int*)nullptr, (float*)nullptr);
    list_offsets(bf, N, ls.iRow, iO, (long long)PESTO_LDDT_MAX_ENTRIES, iSt);
    ListState h{};
    if (int rc = bf.verdict(iSt, &h, sizeof h, what)) return rc;
    *K = h.K;
    if (h.err) return index_error(h.err, what);
    return 0;
}

// the fill pass into jn / dref (K entries, sized by the caller)
void list_fill(Buffers& bf, const ListScratch& ls, int N, int n_struct, const int* offs, int mode, float s_star, float scale,
               const long long* off, int* jn, float* dref) {
    hipLaunchKernelGGL(k_lddt_list<true>, dim3(blocks((size_t)N, NT)), dim3(NT), 0, bf.stm, N, n_struct, offs, (const CellGrid*)bf.ptr<CellGrid>(ls.iG),
                       (const int*)bf.ptr<int>(ls.iCnt), (const float4*)bf.ptr<float4>(ls.iSort), (const int2*)bf.ptr<int2>(ls.iMeta), mode,
                       s_star, scale, (int*)nullptr, off, jn, dref);
}

// the check kernel and its verdict (item iSt, declared cleared), read before anything else is launched
int run_check(Buffers& bf, int N, int R, int n_struct, long long K, const int* offs, const int* rso, const int* res, const int* perm,
              const int* roff, const long long* off, const int* jn, int iSt, const char* what) {
    const size_t n = std::max<size_t>((size_t)N + 1, off ? (size_t)K : 0);
    hipLaunchKernelGGL(k_lddt_check, dim3(blocks(n, NT)), dim3(NT), 0, bf.stm, N, R, n_struct, K, offs, rso, res, perm, roff, off, jn,
                       bf.ptr<ListState>(iSt));
    ListState h{};
    if (int rc = bf.verdict(iSt, &h, sizeof h, what)) return rc;
    return index_error(h.err, what);
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_lddt_last_error(void) { return last_error(); }

int pesto_lddt_pairs(pesto_model* m, int64_t N, int32_t n_struct, const int32_t* struct_offsets, const float* xyz_ref, const int32_t* res_of_atom,
                     const int32_t* chain_of_atom, const uint8_t* sel, int32_t mode, float r_incl, double scale, int64_t capacity,
                     int64_t* offsets_out, int32_t* j_out, float* d_out, int64_t* n_pairs_out, int32_t ptr_kind, void* stream) {
    if (!struct_offsets || !xyz_ref || !res_of_atom || !offsets_out || !n_pairs_out || capacity < 0 || capacity > PESTO_LDDT_MAX_ENTRIES ||
        (capacity > 0 && (!j_out || !d_out)))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_common(N, n_struct, struct_offsets, mode, chain_of_atom, r_incl, scale)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const float fscale = (float)scale;
    const float s_star = contact_threshold(r_incl, fscale, true);       // d_ref < r_incl  <=>  dist2 < s_star
    const size_t n = (size_t)N;
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iY = bf.input(xyz_ref, n * 12), iR = bf.input(res_of_atom, n * 4),
              iC = bf.input(chain_of_atom, n * 4), iS = bf.input(sel, n);
    const int iO = bf.output(offsets_out, (n + 1) * 8), iJ = bf.partial(j_out, (size_t)capacity * 4), iD = bf.partial(d_out, (size_t)capacity * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0);
    const ListScratch ls = list_scratch(bf, n, (size_t)n_struct);
    long long K = 0;
    int rc = bf.upload();
    // (res_of_atom, chain_of_atom and sel are only compared here: nothing to validate)
    if (rc == 0)
        rc = list_count(bf, ls, (int)N, n_struct, bf.ptr<const int>(iOff), bf.ptr<const float>(iY), bf.ptr<const int>(iR), bf.ptr<const int>(iC),
                        bf.ptr<const unsigned char>(iS), mode, r_incl, fscale, s_star, iO, iSt, &K, "lddt_pairs");
    if (rc == 0) {
        *n_pairs_out = K;
        if (K > PESTO_LDDT_MAX_ENTRIES) rc = fail(PESTO_ERR_INVALID, "lddt_pairs: %lld reference pairs, at most 2^30 per call", K);
    }
    if (rc == 0 && K > 0 && K <= capacity) {
        list_fill(bf, ls, (int)N, n_struct, bf.ptr<const int>(iOff), mode, s_star, fscale, bf.ptr<const long long>(iO), bf.ptr<int>(iJ),
                  bf.ptr<float>(iD));
        rc = bf.fetch(iJ, (size_t)K * 4);
        if (rc == 0) rc = bf.fetch(iD, (size_t)K * 4);
    }
    return bf.finish(rc, "lddt_pairs");
}

int pesto_lddt(pesto_model* m, int64_t F, int64_t N, int32_t n_struct, const int32_t* struct_offsets, const int32_t* res_struct_offsets,
               const float* xyz_ref, const float* xyz, int64_t R, const int32_t* res_of_atom, const int32_t* perm, const int32_t* res_offsets,
               const int32_t* chain_of_atom, const uint8_t* sel, int32_t mode, int32_t T, const float* thresholds, float r_incl, double scale,
               int64_t K_in, const int64_t* offsets_in, const int32_t* j_in, const float* d_in, float* score_out,
               float* residue_out, int32_t* preserved_out, int32_t* total_out, int64_t* n_pairs_out, int32_t ptr_kind, void* stream) {
    if (!struct_offsets || !res_struct_offsets || !xyz || !res_of_atom || !perm || !res_offsets || !thresholds || !score_out || !residue_out ||
        !preserved_out || !total_out || !n_pairs_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    const bool given = offsets_in != nullptr;
    if (given ? (K_in < 0 || K_in > PESTO_LDDT_MAX_ENTRIES || (K_in > 0 && (!j_in || !d_in))) : !xyz_ref)
        return fail(PESTO_ERR_INVALID, "give xyz_ref, or a list of 0 to 2^30 entries (offsets_in, j_in, d_in)");
    if (F < 1 || F > PESTO_LDDT_MAX_FRAMES) return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, got %lld", (long long)F);
    if (T < 1 || T > MAX_T) return fail(PESTO_ERR_INVALID, "1 to 8 thresholds, got %d", T);
    Thresholds thr{};
    for (int k = 0; k < T; ++k) {
        thr.t[k] = thresholds[k];
        if (!std::isfinite(thr.t[k]) || !(thr.t[k] > 0.f) || (k && !(thr.t[k] > thr.t[k - 1])))
            return fail(PESTO_ERR_INVALID, "thresholds must be positive, finite and ascending");
    }
    if (int rc = check_common(N, n_struct, struct_offsets, given ? MODE_ALL : mode, chain_of_atom, r_incl, scale)) return rc;
    if (R < 1 || R > N || R < n_struct) return fail(PESTO_ERR_INVALID, "n_struct <= R <= N residues");
    if ((uint64_t)F * (uint64_t)R * (uint64_t)T > (1ull << 36))
        return fail(PESTO_ERR_INVALID, "F * R * T = %lld * %lld * %d counts do not fit one call: pass the frames in batches", (long long)F, (long long)R, T);
    if (F * (int64_t)n_struct > 0x7fffffff) return fail(PESTO_ERR_INVALID, "F * n_struct must stay below 2^31");
    if (int rc = check_offsets(res_struct_offsets, n_struct, R, "res_struct_offsets")) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const float fscale = (float)scale;
    const float s_star = contact_threshold(r_incl, fscale, true);       // d_ref < r_incl  <=>  dist2 < s_star
    const size_t n = (size_t)N, nr = (size_t)R;
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iRso = bf.table(res_struct_offsets, ((size_t)n_struct + 1) * 4);
    const int iY = bf.input(given ? nullptr : xyz_ref, n * 12), iX = bf.input(xyz, (size_t)F * n * 12), iR = bf.input(res_of_atom, n * 4),
              iPm = bf.input(perm, n * 4), iRo = bf.input(res_offsets, (nr + 1) * 4), iC = bf.input(given ? nullptr : chain_of_atom, n * 4),
              iS = bf.input(given ? nullptr : sel, n);
    const int iOi = bf.input(offsets_in, (n + 1) * 8), iJi = bf.input(given ? j_in : nullptr, (size_t)K_in * 4),
              iDi = bf.input(given ? d_in : nullptr, (size_t)K_in * 4);
    const int iSc = bf.output(score_out, (size_t)F * n_struct * 4), iRe = bf.output(residue_out, (size_t)F * nr * 4),
              iPr = bf.output(preserved_out, (size_t)F * nr * T * 4), iTo = bf.output(total_out, nr * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iNp = bf.scratch((size_t)n_struct * 8), iOs = bf.scratch(given ? 0 : (n + 1) * 8);
    ListScratch ls{};
    if (!given) ls = list_scratch(bf, n, (size_t)n_struct);
    char* list = nullptr;               // the call's own list: K entries, known only after the count pass
    int rc = bf.upload();
    const int* offs = bf.ptr<const int>(iOff);
    const int* rso = bf.ptr<const int>(iRso);
    const long long* off = given ? bf.ptr<const long long>(iOi) : bf.ptr<const long long>(iOs);
    const int* jn = given ? bf.ptr<const int>(iJi) : nullptr;
    const float* dref = given ? bf.ptr<const float>(iDi) : nullptr;
    long long K = given ? (long long)K_in : 0;
    if (rc == 0)
        rc = run_check(bf, (int)N, (int)R, n_struct, K, offs, rso, bf.ptr<const int>(iR), bf.ptr<const int>(iPm), bf.ptr<const int>(iRo),
                       given ? off : nullptr, jn, iSt, "lddt");
    if (rc == 0 && !given) {
        rc = list_count(bf, ls, (int)N, n_struct, offs, bf.ptr<const float>(iY), bf.ptr<const int>(iR), bf.ptr<const int>(iC),
                        bf.ptr<const unsigned char>(iS), mode, r_incl, fscale, s_star, iOs, iSt, &K, "lddt");
        if (rc == 0 && K > PESTO_LDDT_MAX_ENTRIES) {
            n_pairs_out[0] = K;                                         // (the caller tells this refusal by it)
            rc = fail(PESTO_ERR_INVALID, "lddt: %lld reference pairs, at most 2^30 per call", K);
        }
        if (rc == 0 && hipMallocAsync((void**)&list, std::max<size_t>((size_t)K * 8, 256), bf.stm) != hipSuccess) {
            list = nullptr;
            rc = fail(PESTO_ERR_NOMEM, "lddt: device allocation of %lld list entries failed", K);
        }
        if (rc == 0) {
            jn = (const int*)list;
            dref = (const float*)(list + (size_t)K * 4);
            if (K > 0) list_fill(bf, ls, (int)N, n_struct, offs, mode, s_star, fscale, off, (int*)jn, (float*)dref);
        }
    }
    if (rc == 0) {
        hipLaunchKernelGGL(k_lddt_total, dim3(blocks(nr + (size_t)n_struct, NT)), dim3(NT), 0, bf.stm, (int)R, n_struct, offs, bf.ptr<const int>(iPm),
                           bf.ptr<const int>(iRo), off, bf.ptr<int>(iTo), bf.ptr<long long>(iNp));
        const int groups = (int)((R + NW - 1) / NW);
        const long long n_items = (long long)F * groups;
        for (int k = T; k < MAX_T; ++k) thr.t[k] = thr.t[T - 1];         // (compared where TT > T, never stored)
        hipLaunchKernelGGL(T <= 4 ? k_lddt_score<4> : k_lddt_score<MAX_T>, dim3((unsigned)std::min<long long>(n_items, (long long)MAX_SCORE_BLOCKS)), dim3(NT), 0,
                           bf.stm, n_items, groups, (int)N, (int)R, (int)T, thr, fscale, bf.ptr<const float>(iX), bf.ptr<const int>(iPm),
                           bf.ptr<const int>(iRo), off, jn, dref, bf.ptr<int>(iPr));
        hipLaunchKernelGGL(k_lddt_final, dim3((unsigned)(F * n_struct)), dim3(NT), 0, bf.stm, n_struct, (int)R, (int)T, rso,
                           (const int*)bf.ptr<int>(iTo), (const int*)bf.ptr<int>(iPr), bf.ptr<float>(iRe), bf.ptr<float>(iSc));
    }
    if (rc == 0) rc = bf.read(iNp, n_pairs_out, (size_t)n_struct * 8);
    if (list) (void)hipFreeAsync(list, bf.stm);
    return bf.finish(rc, "lddt");
}
