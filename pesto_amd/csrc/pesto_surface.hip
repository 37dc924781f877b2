// pesto_surface.hip - surface-vertex benchmark scoring: what masif-site_benchmark/masif_sppider_Intpred_comp.ipynb of the reference does
// with pyflann (nearest atom of every mesh vertex), pymesh (vertex_area) and Python dictionaries (labels and scores per residue), over a
// ragged batch of S structures: v_offsets over V vertices, a_offsets over N atoms, f_offsets over F faces, r_offsets over R residues.
//
//   nearest atom   brute force through LDS. A workgroup owns SF_VTILE vertices of ONE structure and one slab of that structure's atoms,
//                  which it walks in tiles of SF_ATILE float4 (x, y, z, batch index). The key is the float32 squared distance
//                  fma(rz, rz, fma(ry, ry, rx * rx)) of the rounded differences (dist() of pesto_cellgrid.h without the root); a key that
//                  is not finite never matches. A thread walks its atoms in ascending order and replaces its best on `key < best` only, so
//                  the lowest index wins inside a slab; the slabs meet in a 64-bit atomicMin on float_as_uint(key) << 32 | atom over an
//                  array of all ones. A key is never negative and never -0 (a square, or a sum of squares), so the unsigned order of its
//                  bits is the float order and the atom index breaks ties: the minimum is the same whatever the arrival order.
//   vertex areas   one thread per face: the area in float64 from the float32 corners, every operation rounded as written, a third of it as
//                  llrint(area / 3 * 2^40) added to the three corners with 64-bit integer atomics (the fixed point of the occupancy sums).
//   residue table  one thread per vertex: count, area, interface area (integer atomics) and the maximum vertex score of the residue of its
//                  nearest atom (atomicMax over the order-preserving map of the float's bits, -0.0 taken as +0.0); one thread per residue:
//                  the label iface_area > 5.0 && iface_area / area > 0.04 and the score back from its bits.
//   scored list    the residues with a vertex and a valid prediction, compacted per structure in residue order on the list protocol of
//                  pesto_scan.h (count -> k_list_offsets -> emit).
// There is no floating-point atomic in this file: every sum is an integer sum, every output the same bits from call to call.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h.
#include <cmath>

#include "pesto_call.h"
#include "pesto_scan.h"

namespace pesto {

namespace {

constexpr int SF_NT = 256;                                // threads per workgroup of every kernel here
constexpr int SF_VTILE = PESTO_SURFACE_VERTEX_TILE;       // vertices per workgroup of the search: one per thread
constexpr int SF_ATILE = PESTO_SURFACE_ATOM_TILE;         // atoms per LDS tile
constexpr int SF_WAVES = SF_NT / 64;
static_assert(SF_VTILE == SF_NT && SF_ATILE == SF_NT, "a thread owns one vertex and stages one atom per tile");
static_assert(PESTO_SURFACE_SLAB % PESTO_SURFACE_ATOM_TILE == 0, "a slab is whole tiles");

typedef unsigned long long u64;

constexpr u64 SF_NONE = ~0ull;                            // a vertex nobody matched
constexpr float SF_F32_MAX = 3.402823466e38f;
constexpr double SF_FIXED = 1099511627776.0;              // 2^40
constexpr double SF_FIXED_MAX = 9007199254740992.0;       // 2^53: a face's third above it is refused

// error bits of ListState.err
enum { SF_ERR_FACE = 1, SF_ERR_AREA = 2, SF_ERR_ATOM = 4, SF_ERR_RESIDUE = 8, SF_ERR_SCORE = 16 };

// the order-preserving map of a finite float's bits (ascending; -0.0 as +0.0). 0 is no finite float's image: the empty maximum.
__device__ __forceinline__ unsigned sf_asc(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float sf_score(unsigned asc) { return __uint_as_float((asc >> 31) ? (asc & 0x7fffffffu) : ~asc); }

__device__ __forceinline__ bool sf_finite(float v) { return fabsf(v) <= SF_F32_MAX; }

// ------------------------------------------------------------------------------------------------ nearest atom
// workgroup b is item b - item_off[s] of structure s (item_off: the structures' vertex tiles x slabs, scanned on the host): vertex tile
// item / n_slab, slab item % n_slab. A tile never holds vertices or atoms of two structures.
__global__ __launch_bounds__(SF_NT) void k_surf_nearest(int n_struct, int slab, const int* __restrict__ item_off, const int* __restrict__ voff,
                                                        const int* __restrict__ aoff, const float* __restrict__ vert,
                                                        const float* __restrict__ xyz, u64* __restrict__ packed) {
    __shared__ float4 tile[SF_ATILE];
    const int s = struct_of((int)blockIdx.x, n_struct, item_off);
    const int item = (int)blockIdx.x - item_off[s];
    const int a_lo = aoff[s], a_hi = aoff[s + 1];
    const int n_slab = (int)(((long long)(a_hi - a_lo) + slab - 1) / slab);
    const int vt = item / n_slab, sl = item - vt * n_slab;
    const long long v = (long long)voff[s] + (long long)vt * SF_VTILE + threadIdx.x;
    const bool mine = v < voff[s + 1];
    const float qnan = __uint_as_float(0x7fc00000u);
    const float px = mine ? vert[3 * v] : qnan, py = mine ? vert[3 * v + 1] : qnan, pz = mine ? vert[3 * v + 2] : qnan;
    const long long a0 = (long long)a_lo + (long long)sl * slab;
    const long long a1 = min((long long)a_hi, a0 + slab);
    float best = 0.f;
    int best_i = -1;
    for (long long t0 = a0; t0 < a1; t0 += SF_ATILE) {
        __syncthreads();
        const long long j = t0 + threadIdx.x;
        tile[threadIdx.x] = j < a1 ? make_float4(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], __int_as_float((int)j)) : make_float4(qnan, qnan, qnan, qnan);
        __syncthreads();
        const int n = (int)min((long long)SF_ATILE, a1 - t0);
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 a = tile[k];
            const float rx = a.x - px, ry = a.y - py, rz = a.z - pz;
            const float key = __fmaf_rn(rz, rz, __fmaf_rn(ry, ry, __fmul_rn(rx, rx)));
            // finite (neither NaN nor inf) and better: ascending k, strict <, so the lowest index of equal keys stays
            if (sf_finite(key) && (best_i < 0 || key < best)) { best = key; best_i = __float_as_int(a.w); }
        }
    }
    if (mine && best_i >= 0) atomicMin(&packed[v], (u64)__float_as_uint(best) << 32 | (u64)(unsigned)best_i);
}

__global__ __launch_bounds__(SF_NT) void k_surf_unpack(long long n, const u64* __restrict__ packed, int* __restrict__ index, float* __restrict__ distance) {
    const long long v = (long long)blockIdx.x * SF_NT + threadIdx.x;
    if (v >= n) return;
    const u64 k = packed[v];
    if (k == SF_NONE) {
        index[v] = -1;
        distance[v] = __uint_as_float(0x7fc00000u);
    } else {
        index[v] = (int)(unsigned)(k & 0xffffffffull);
        distance[v] = sqrtf(__uint_as_float((unsigned)(k >> 32)));
    }
}

// ------------------------------------------------------------------------------------------------ vertex areas
// one thread per face. An index outside the face's structure sets SF_ERR_FACE and the face is skipped before any read.
__global__ __launch_bounds__(SF_NT) void k_surf_areas(long long n_face, int n_struct, const int* __restrict__ voff, const int* __restrict__ foff,
                                                      const float* __restrict__ vert, const int* __restrict__ faces, long long* __restrict__ area,
                                                      ListState* __restrict__ st) {
    const long long f = (long long)blockIdx.x * SF_NT + threadIdx.x;
    if (f >= n_face) return;
    const int s = struct_of((int)f, n_struct, foff);          // (the last s with foff[s] <= f: structures without faces are passed over)
    const int v0 = voff[s], nv = voff[s + 1] - v0;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        atomicOr(&st->err, SF_ERR_FACE);
        return;
    }
    const long long g0 = (long long)v0 + i0, g1 = (long long)v0 + i1, g2 = (long long)v0 + i2;
    const double ax = vert[3 * g0], ay = vert[3 * g0 + 1], az = vert[3 * g0 + 2];
    const double ux = __dsub_rn((double)vert[3 * g1], ax), uy = __dsub_rn((double)vert[3 * g1 + 1], ay), uz = __dsub_rn((double)vert[3 * g1 + 2], az);
    const double wx = __dsub_rn((double)vert[3 * g2], ax), wy = __dsub_rn((double)vert[3 * g2 + 1], ay), wz = __dsub_rn((double)vert[3 * g2 + 2], az);
    const double cx = __dsub_rn(__dmul_rn(uy, wz), __dmul_rn(uz, wy));
    const double cy = __dsub_rn(__dmul_rn(uz, wx), __dmul_rn(ux, wz));
    const double cz = __dsub_rn(__dmul_rn(ux, wy), __dmul_rn(uy, wx));
    const double sq = __dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz));
    const double a = __dmul_rn(0.5, __dsqrt_rn(sq));
    const double third = __dmul_rn(__ddiv_rn(a, 3.0), SF_FIXED);
    if (!(third < SF_FIXED_MAX)) {                            // NaN, inf or beyond what the sums are meant for
        atomicOr(&st->err, SF_ERR_AREA);
        return;
    }
    const long long q = llrint(third);
    if (q == 0) return;
    atomicAdd((u64*)&area[g0], (u64)q);
    atomicAdd((u64*)&area[g1], (u64)q);
    atomicAdd((u64*)&area[g2], (u64)q);
}

// ------------------------------------------------------------------------------------------------ residue table
// one thread per vertex; maxkey (the max_score array as unsigned, cleared) may be NULL with score
__global__ __launch_bounds__(SF_NT) void k_surf_residue_acc(long long n_vert, int n_struct, const int* __restrict__ voff, const int* __restrict__ aoff,
                                                            const int* __restrict__ roff, const int* __restrict__ nearest,
                                                            const int* __restrict__ atom_res, const long long* __restrict__ area,
                                                            const unsigned char* __restrict__ iface, const float* __restrict__ score,
                                                            int* __restrict__ r_n, long long* __restrict__ r_area, long long* __restrict__ r_iarea,
                                                            unsigned* __restrict__ maxkey, ListState* __restrict__ st) {
    const long long v = (long long)blockIdx.x * SF_NT + threadIdx.x;
    if (v >= n_vert) return;
    if (score && !sf_finite(score[v])) atomicOr(&st->err, SF_ERR_SCORE);
    const int a = nearest[v];
    if (a == -1) return;                                       // a vertex without a nearest atom belongs to no residue
    const int s = struct_of((int)v, n_struct, voff);
    if (a < aoff[s] || a >= aoff[s + 1]) { atomicOr(&st->err, SF_ERR_ATOM); return; }
    const int rl = atom_res[a];
    if (rl < 0 || rl >= roff[s + 1] - roff[s]) { atomicOr(&st->err, SF_ERR_RESIDUE); return; }
    const long long r = (long long)roff[s] + rl;
    const long long q = area[v];
    atomicAdd(&r_n[r], 1);
    atomicAdd((u64*)&r_area[r], (u64)q);
    if (iface[v]) atomicAdd((u64*)&r_iarea[r], (u64)q);
    if (score && sf_finite(score[v])) atomicMax(&maxkey[r], sf_asc(score[v]));
}

// one thread per residue: the label from the integer sums, the maximum back from its bits (in place)
__global__ __launch_bounds__(SF_NT) void k_surf_residue_fin(long long n_res, const long long* __restrict__ r_area, const long long* __restrict__ r_iarea,
                                                            unsigned char* __restrict__ label, unsigned* __restrict__ maxkey) {
    const long long r = (long long)blockIdx.x * SF_NT + threadIdx.x;
    if (r >= n_res) return;
    const double scale = 1.0 / SF_FIXED;                       // (a power of two: the products are exact)
    const double ia = __dmul_rn((double)r_iarea[r], scale), ar = __dmul_rn((double)r_area[r], scale);
    label[r] = (ia > 5.0 && __ddiv_rn(ia, ar) > 0.04) ? 1 : 0;
    if (maxkey) {
        const unsigned k = maxkey[r];
        maxkey[r] = k ? __float_as_uint(sf_score(k)) : 0x7fc00000u;
    }
}

// ------------------------------------------------------------------------------------------------ vertex scores
__global__ __launch_bounds__(SF_NT) void k_surf_gather(long long n_vert, long long n_atom, const int* __restrict__ nearest, const float* __restrict__ p_atom,
                                                       float* __restrict__ out, ListState* __restrict__ st) {
    const long long v = (long long)blockIdx.x * SF_NT + threadIdx.x;
    if (v >= n_vert) return;
    const int a = nearest[v];
    float r = __uint_as_float(0x7fc00000u);
    if (a >= 0 && a < n_atom) r = p_atom[a];
    else if (a != -1) atomicOr(&st->err, SF_ERR_ATOM);
    out[v] = r;
}

// ------------------------------------------------------------------------------------------------ scored residues
// one workgroup per structure walks its residues in chunks of SF_NT and keeps their order (ranks by __ballot per wave, the waves' counts
// through LDS). EMIT false: the structure's count to cnt[s]; true: the entries from off[s], when the list fits the capacity
template <bool EMIT>
__global__ __launch_bounds__(SF_NT) void k_surf_scored(const int* __restrict__ roff, const int* __restrict__ r_n, const unsigned char* __restrict__ label,
                                                       const float* __restrict__ p_res, const unsigned char* __restrict__ valid, int* __restrict__ cnt,
                                                       const long long* __restrict__ off, const ListState* __restrict__ st, int* __restrict__ res_out,
                                                       unsigned char* __restrict__ y_out, float* __restrict__ p_out) {
    __shared__ int wsum[SF_WAVES];
    if (EMIT && !st->fits) return;
    const int s = blockIdx.x;
    const int r0 = roff[s], r1 = roff[s + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (long long c0 = r0; c0 < r1; c0 += SF_NT) {
        const long long r = c0 + threadIdx.x;
        const bool keep = r < r1 && r_n[r] > 0 && (!valid || valid[r]);
        const u64 b = __ballot(keep);
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < SF_WAVES; ++k) { pre += k < w ? wsum[k] : 0; tot += wsum[k]; }
        if (EMIT && keep) {
            const long long at = off[s] + base + pre + rank;
            res_out[at] = (int)r; y_out[at] = label[r] ? 1 : 0; p_out[at] = p_res[r];
        }
        base += tot;
        __syncthreads();
    }
    if (!EMIT && threadIdx.x == 0) cnt[s] = base;
}

// ------------------------------------------------------------------------------------------------ the host side
// offs[0 .. n] from 0 to its total without running backwards (a structure may have no face)
int check_face_offsets(const int32_t* offs, int32_t n) {
    if (offs[0] != 0) return fail(PESTO_ERR_INVALID, "f_offsets must start at 0");
    for (int s = 0; s < n; ++s)
        if (offs[s + 1] < offs[s]) return fail(PESTO_ERR_INVALID, "f_offsets: unordered structure %d", s);
    return 0;
}

int check_struct_offsets(int32_t n_struct, const int32_t* offs, const char* what) {
    if (n_struct < 1 || !offs) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (offs[n_struct] < 1) return fail(PESTO_ERR_INVALID, "%s must end above 0", what);
    return check_offsets(offs, n_struct, offs[n_struct], what);
}

int surf_finish(Buffers& bf, int rc, const ListState& hs, const char* what) {
    rc = bf.finish(rc, what);
    if (rc != 0) return rc;
    if (hs.err & SF_ERR_FACE) return fail(PESTO_ERR_INVALID, "%s: a face index lies outside its structure's vertices", what);
    if (hs.err & SF_ERR_AREA) return fail(PESTO_ERR_INVALID, "%s: a face's area is not finite, or its third exceeds 2^13 square units", what);
    if (hs.err & SF_ERR_ATOM) return fail(PESTO_ERR_INVALID, "%s: a nearest-atom index is neither -1 nor an atom of the vertex's structure", what);
    if (hs.err & SF_ERR_RESIDUE) return fail(PESTO_ERR_INVALID, "%s: atom_residue holds a residue outside its structure", what);
    if (hs.err & SF_ERR_SCORE) return fail(PESTO_ERR_INVALID, "%s: vertex_score holds a non-finite score (NaN or inf)", what);
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_surface_last_error(void) { return last_error(); }

int pesto_surface_nearest(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* a_offsets, const float* vertices,
                          const float* xyz, int32_t slab, int32_t* index_out, float* distance_out, int32_t ptr_kind, void* stream) {
    if (!vertices || !xyz || !index_out || !distance_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_struct_offsets(n_struct, v_offsets, "v_offsets")) return rc;
    if (int rc = check_struct_offsets(n_struct, a_offsets, "a_offsets")) return rc;
    if (slab == 0) slab = PESTO_SURFACE_SLAB;
    if (slab < SF_ATILE || slab % SF_ATILE != 0) return fail(PESTO_ERR_INVALID, "slab must be 0 (the default) or a positive multiple of %d atoms", SF_ATILE);
    const long long V = v_offsets[n_struct];
    std::vector<int32_t> item_off((size_t)n_struct + 1, 0);
    long long items = 0;
    for (int s = 0; s < n_struct; ++s) {
        const long long vt = ((long long)v_offsets[s + 1] - v_offsets[s] + SF_VTILE - 1) / SF_VTILE;
        const long long sl = ((long long)a_offsets[s + 1] - a_offsets[s] + slab - 1) / slab;
        items += vt * sl;
        if (items > 0x7fffffff) return fail(PESTO_ERR_INVALID, "more than 2^31 - 1 (vertex tile, atom slab) pairs: split the batch");
        item_off[(size_t)s + 1] = (int32_t)items;
    }
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iVo = bf.table(v_offsets, ((size_t)n_struct + 1) * 4), iAo = bf.table(a_offsets, ((size_t)n_struct + 1) * 4),
              iIo = bf.table(item_off.data(), ((size_t)n_struct + 1) * 4), iV = bf.input(vertices, (size_t)V * 12),
              iX = bf.input(xyz, (size_t)a_offsets[n_struct] * 12), iP = bf.scratch((size_t)V * 8, 0xff), iI = bf.output(index_out, (size_t)V * 4),
              iD = bf.output(distance_out, (size_t)V * 4);
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_surf_nearest, dim3((unsigned)items), dim3(SF_NT), 0, bf.stm, (int)n_struct, (int)slab, bf.ptr<const int>(iIo),
                           bf.ptr<const int>(iVo), bf.ptr<const int>(iAo), bf.ptr<const float>(iV), bf.ptr<const float>(iX), bf.ptr<u64>(iP));
        hipLaunchKernelGGL(k_surf_unpack, dim3(blocks((size_t)V, SF_NT)), dim3(SF_NT), 0, bf.stm, V, bf.ptr<const u64>(iP), bf.ptr<int>(iI), bf.ptr<float>(iD));
    }
    return bf.finish(rc, "surface_nearest");
}

int pesto_surface_areas(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* f_offsets, const float* vertices,
                        const int32_t* faces, int64_t* area_fixed_out, int32_t ptr_kind, void* stream) {
    if (!vertices || !area_fixed_out || !f_offsets) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_struct_offsets(n_struct, v_offsets, "v_offsets")) return rc;
    if (int rc = check_face_offsets(f_offsets, n_struct)) return rc;
    const long long V = v_offsets[n_struct], F = f_offsets[n_struct];
    if (F > 0 && !faces) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iVo = bf.table(v_offsets, ((size_t)n_struct + 1) * 4), iFo = bf.table(f_offsets, ((size_t)n_struct + 1) * 4),
              iV = bf.input(vertices, (size_t)V * 12), iF = bf.input(F ? faces : nullptr, (size_t)F * 12), iA = bf.output(area_fixed_out, (size_t)V * 8, 0),
              iSt = bf.scratch(sizeof(ListState), 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        if (F > 0)
            hipLaunchKernelGGL(k_surf_areas, dim3(blocks((size_t)F, SF_NT)), dim3(SF_NT), 0, bf.stm, F, (int)n_struct, bf.ptr<const int>(iVo), bf.ptr<const int>(iFo),
                               bf.ptr<const float>(iV), bf.ptr<const int>(iF), bf.ptr<long long>(iA), bf.ptr<ListState>(iSt));
        rc = bf.read(iSt, &hs, sizeof hs);
    }
    return surf_finish(bf, rc, hs, "surface_areas");
}

int pesto_surface_residues(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* a_offsets, const int32_t* r_offsets,
                           const int32_t* nearest, const int32_t* atom_residue, const int64_t* area_fixed, const uint8_t* iface,
                           const float* vertex_score, int32_t* n_vertices_out, int64_t* area_out, int64_t* iface_area_out, uint8_t* label_out,
                           float* max_score_out, int32_t ptr_kind, void* stream) {
    if (!nearest || !atom_residue || !area_fixed || !iface || !n_vertices_out || !area_out || !iface_area_out || !label_out ||
        (vertex_score && !max_score_out))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_struct_offsets(n_struct, v_offsets, "v_offsets")) return rc;
    if (int rc = check_struct_offsets(n_struct, a_offsets, "a_offsets")) return rc;
    if (int rc = check_struct_offsets(n_struct, r_offsets, "r_offsets")) return rc;
    const long long V = v_offsets[n_struct], N = a_offsets[n_struct], R = r_offsets[n_struct];
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iVo = bf.table(v_offsets, ((size_t)n_struct + 1) * 4), iAo = bf.table(a_offsets, ((size_t)n_struct + 1) * 4),
              iRo = bf.table(r_offsets, ((size_t)n_struct + 1) * 4), iNe = bf.input(nearest, (size_t)V * 4), iAr = bf.input(atom_residue, (size_t)N * 4),
              iAf = bf.input(area_fixed, (size_t)V * 8), iIf = bf.input(iface, (size_t)V), iSc = bf.input(vertex_score, (size_t)V * 4),
              iN = bf.output(n_vertices_out, (size_t)R * 4, 0), iA = bf.output(area_out, (size_t)R * 8, 0),
              iIa = bf.output(iface_area_out, (size_t)R * 8, 0), iL = bf.output(label_out, (size_t)R),
              iM = bf.output(vertex_score ? max_score_out : nullptr, (size_t)R * 4, 0),           // (a NULL output is not cleared)
              iSt = bf.scratch(sizeof(ListState), 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_surf_residue_acc, dim3(blocks((size_t)V, SF_NT)), dim3(SF_NT), 0, bf.stm, V, (int)n_struct, bf.ptr<const int>(iVo), bf.ptr<const int>(iAo),
                           bf.ptr<const int>(iRo), bf.ptr<const int>(iNe), bf.ptr<const int>(iAr), bf.ptr<const long long>(iAf),
                           bf.ptr<const unsigned char>(iIf), bf.ptr<const float>(iSc), bf.ptr<int>(iN), bf.ptr<long long>(iA), bf.ptr<long long>(iIa),
                           bf.ptr<unsigned>(iM), bf.ptr<ListState>(iSt));
        hipLaunchKernelGGL(k_surf_residue_fin, dim3(blocks((size_t)R, SF_NT)), dim3(SF_NT), 0, bf.stm, R, bf.ptr<const long long>(iA), bf.ptr<const long long>(iIa),
                           bf.ptr<unsigned char>(iL), bf.ptr<unsigned>(iM));
        rc = bf.read(iSt, &hs, sizeof hs);
    }
    return surf_finish(bf, rc, hs, "surface_residues");
}

int pesto_surface_vertex_scores(pesto_model* m, int64_t n_vertices, int64_t n_atoms, const int32_t* nearest, const float* p_atom, float* out,
                                int32_t ptr_kind, void* stream) {
    if (n_vertices < 1 || n_atoms < 1 || n_vertices > 0x7fffffff || n_atoms > 0x7fffffff || !nearest || !p_atom || !out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iNe = bf.input(nearest, (size_t)n_vertices * 4), iP = bf.input(p_atom, (size_t)n_atoms * 4), iO = bf.output(out, (size_t)n_vertices * 4),
              iSt = bf.scratch(sizeof(ListState), 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_surf_gather, dim3(blocks((size_t)n_vertices, SF_NT)), dim3(SF_NT), 0, bf.stm, (long long)n_vertices, (long long)n_atoms,
                           bf.ptr<const int>(iNe), bf.ptr<const float>(iP), bf.ptr<float>(iO), bf.ptr<ListState>(iSt));
        rc = bf.read(iSt, &hs, sizeof hs);
    }
    return surf_finish(bf, rc, hs, "surface_vertex_scores");
}

int pesto_surface_scored(pesto_model* m, int32_t n_struct, const int32_t* r_offsets, const int32_t* n_vertices, const uint8_t* label, const float* p_res,
                         const uint8_t* valid, int64_t capacity, int64_t* offsets_out, int32_t* residue_out, uint8_t* y_out, float* p_out,
                         int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (!n_vertices || !label || !p_res || !offsets_out || !sizes_out || (capacity > 0 && (!residue_out || !y_out || !p_out)))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (capacity < 0 || capacity > 0x7fffffff) return fail(PESTO_ERR_INVALID, "capacity must be in [0, 2^31)");
    if (int rc = check_struct_offsets(n_struct, r_offsets, "r_offsets")) return rc;
    const long long R = r_offsets[n_struct];
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t cap = (size_t)capacity;
    Buffers bf(ptr_kind, stream);
    const int iRo = bf.table(r_offsets, ((size_t)n_struct + 1) * 4), iN = bf.input(n_vertices, (size_t)R * 4), iL = bf.input(label, (size_t)R),
              iP = bf.input(p_res, (size_t)R * 4), iVa = bf.input(valid, (size_t)R), iO = bf.output(offsets_out, ((size_t)n_struct + 1) * 8),
              iRes = bf.partial(residue_out, cap * 4), iY = bf.partial(y_out, cap), iPo = bf.partial(p_out, cap * 4),
              iCnt = bf.scratch((size_t)n_struct * 4), iSt = bf.scratch(sizeof(ListState), 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const dim3 grid((unsigned)n_struct);
        hipLaunchKernelGGL(k_surf_scored<false>, grid, dim3(SF_NT), 0, bf.stm, bf.ptr<const int>(iRo), bf.ptr<const int>(iN),
                           bf.ptr<const unsigned char>(iL), bf.ptr<const float>(iP), bf.ptr<const unsigned char>(iVa), bf.ptr<int>(iCnt),
                           (const long long*)nullptr, (const ListState*)bf.ptr<ListState>(iSt), (int*)nullptr, (unsigned char*)nullptr, (float*)nullptr);
        list_offsets(bf, (int)n_struct, iCnt, iO, (long long)capacity, iSt);
        hipLaunchKernelGGL(k_surf_scored<true>, grid, dim3(SF_NT), 0, bf.stm, bf.ptr<const int>(iRo), bf.ptr<const int>(iN),
                           bf.ptr<const unsigned char>(iL), bf.ptr<const float>(iP), bf.ptr<const unsigned char>(iVa), bf.ptr<int>(iCnt),
                           bf.ptr<const long long>(iO), (const ListState*)bf.ptr<ListState>(iSt), bf.ptr<int>(iRes), bf.ptr<unsigned char>(iY),
                           bf.ptr<float>(iPo));
    }
    // the one synchronisation for sizing: the count
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "surface_scored");
    if (rc == 0) rc = list_tail(bf, hs, sizes_out, {{iRes, 4}, {iY, 1}, {iPo, 4}});
    return bf.finish(rc, "surface_scored");
}
