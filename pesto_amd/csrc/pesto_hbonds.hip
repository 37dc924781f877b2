// pesto_hbonds.hip - the last two array functions of md_analysis/mdtraj_utils/trajectory_utils.py: Baker-Hubbard hydrogen bonds over an MD
// run (per frame, and by occupancy over the frames) and the unwrapping of periodic images by molecule.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h.
//
// Hydrogen bonds. The candidates are the triplets (dh[p,0], dh[p,1], acc[a]) with acc[a] != dh[p,0], p ascending, then a ascending. The
// H .. A distance is the float32 one of pesto_geom.h, d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale), tested as d < r_thr on the
// rounded sum against s_star (contact_threshold); only an emitted bond takes the root. The D-H-A angle is tested in double from the float32
// coordinates, without acos or root: u = D - H, v = A - H, c = (ux*vx + uy*vy) + uz*vz, uu and vv likewise, bonded iff
// c < 0 && c*c > k * (uu*vv) with k = cos^2(angle), every operation rounded as written (hb_angle: no contraction). NaN, uu = 0 and vv = 0
// fail it (c < 0 is false).
// The frame lists come out of count -> per-frame scan -> 64-bit offsets -> emit (the list protocol of pesto_scan.h); the occupancy
// lists out of the same protocol with a donor pair in the place of a frame. Tiled brute force, no cell grid. Nothing of size [P, A] is
// stored: the frame lists keep one count per (frame, donor pair), the occupancy one per (donor pair, 64 acceptors).
// Unwrapping sums every molecule's centre of mass in double in a fixed order and picks the first of the 27 images nearest to molecule 0.
// Every output is bit-identical from call to call.
#include <cmath>

#include "pesto_call.h"
#include "pesto_scan.h"
#include "pesto_geom.h"

namespace pesto {

namespace {

constexpr int NT = 256;                                 // threads per workgroup of every kernel here
constexpr int HB_ROWS = 8;                              // donor pairs per wave (the acceptor's coordinates are loaded once for all of them)
constexpr int HB_TILE = HB_ROWS * NT / 64;              // ... and per workgroup
static_assert(HB_TILE == PESTO_HBONDS_DONOR_TILE, "the header states the donor tile");

// err of the call's ListState: bit 0: an atom of dh outside [0, N); bit 1: an atom of acc; bit 2: an atom of the molecule permutation;
// bit 3: an atom named twice by the molecule permutation (some other atom is then named by no row, and its output never written)
enum { ERR_DH = 1, ERR_ACC = 2, ERR_PERM = 4, ERR_DUP = 8 };

// the angle criterion at H: u = D - H (u[0..2], u[3] = uu), v = A - H
__device__ __forceinline__ double dot3_rn(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

__device__ __forceinline__ bool hb_angle(const double* u, float hx, float hy, float hz, float ax, float ay, float az, double k) {
#pragma clang fp contract(off)
    const double vx = __dsub_rn((double)ax, (double)hx), vy = __dsub_rn((double)ay, (double)hy), vz = __dsub_rn((double)az, (double)hz);
    const double c = dot3_rn(u[0], u[1], u[2], vx, vy, vz);
    const double vv = dot3_rn(vx, vy, vz, vx, vy, vz);
    return c < 0.0 && __dmul_rn(c, c) > __dmul_rn(k, __dmul_rn(u[3], vv));         // (NaN: false; uu = 0 or vv = 0: c = 0)
}

__device__ __forceinline__ void hb_u(float dx, float dy, float dz, float hx, float hy, float hz, double* u) {
#pragma clang fp contract(off)
    u[0] = __dsub_rn((double)dx, (double)hx);
    u[1] = __dsub_rn((double)dy, (double)hy);
    u[2] = __dsub_rn((double)dz, (double)hz);
    u[3] = dot3_rn(u[0], u[1], u[2], u[0], u[1], u[2]);
}

// every atom index of the tables must lie in [0, N): checked before a kernel dereferences it
__global__ __launch_bounds__(NT) void k_hb_check(int N, int P, int A, const int* __restrict__ dh, const int* __restrict__ acc, ListState* __restrict__ st) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x, P2 = 2 * (long long)P;
    if (k < P2) {
        if (dh[k] < 0 || dh[k] >= N) atomicOr(&st->err, ERR_DH);
    } else if (k < P2 + A) {
        if (acc[k - P2] < 0 || acc[k - P2] >= N) atomicOr(&st->err, ERR_ACC);
    }
}

// ------------------------------------------------------------------------------------------------ frame lists
// replaces: md.baker_hubbard(traj[k], periodic=False) restarted per frame and the np.isin filters behind it (hydrogen_bonds,
// md_analysis/mdtraj_utils/trajectory_utils.py:441-471). A workgroup owns HB_TILE donor pairs of one frame, a wave HB_ROWS of them, their
// H coordinates and u = D - H in registers; its lanes walk the acceptors 64 at a time, each lane's acceptor gathered through acc and
// tested against the wave's HB_ROWS donor pairs. A 64-lane ballot orders the hits of a row by a, so the count pass (EMIT = false:
// cnt[f * P + p]) and the emit pass (into [foff[f] + cnt[f * P + p] ...), cnt scanned per frame by then) see the same hits in the same
// order. group (NULL: no filter): only triplets whose donor and acceptor atoms carry different non-zero groups.
template <bool EMIT>
__global__ __launch_bounds__(NT) void k_hb_pairs(int N, int P, int A, int tiles, const float* __restrict__ xyz, const int* __restrict__ dh,
                                                 const int* __restrict__ acc, const signed char* __restrict__ group, float s_star, float scale,
                                                 double k_cos2, int* __restrict__ cnt, const long long* __restrict__ foff,
                                                 const ListState* __restrict__ st, int* __restrict__ trip, float* __restrict__ d) {
    if (st->err || (EMIT && !st->fits)) return;
    const size_t f = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63;
    const int p0 = (int)(blockIdx.x % (unsigned)tiles) * HB_TILE + (int)(threadIdx.x >> 6) * HB_ROWS;
    if (p0 >= P) return;                // (the whole wave)
    const float* X = xyz + f * (size_t)N * 3;
    float hx[HB_ROWS], hy[HB_ROWS], hz[HB_ROWS];
    double u[HB_ROWS][4];
    int don[HB_ROWS], hyd[HB_ROWS], gd[HB_ROWS], n[HB_ROWS];
    long long base[HB_ROWS];
#pragma unroll
    for (int r = 0; r < HB_ROWS; ++r) {
        const int p = min(p0 + r, P - 1);               // (a row past the end repeats the last one and is never counted)
        don[r] = dh[2 * (size_t)p];
        hyd[r] = dh[2 * (size_t)p + 1];
        hx[r] = X[3 * (size_t)hyd[r]]; hy[r] = X[3 * (size_t)hyd[r] + 1]; hz[r] = X[3 * (size_t)hyd[r] + 2];
        hb_u(X[3 * (size_t)don[r]], X[3 * (size_t)don[r] + 1], X[3 * (size_t)don[r] + 2], hx[r], hy[r], hz[r], u[r]);
        gd[r] = group ? group[don[r]] : 1;
        n[r] = 0;
        base[r] = EMIT ? foff[f] + cnt[f * (size_t)P + p] : 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int a0 = 0; a0 < A; a0 += 64) {
        const int a = a0 + lane;
        const bool valid = a < A;
        const int j = acc[valid ? a : A - 1];
        const float ax = X[3 * (size_t)j], ay = X[3 * (size_t)j + 1], az = X[3 * (size_t)j + 2];
        const int ga = group ? group[j] : 2;
#pragma unroll
        for (int r = 0; r < HB_ROWS; ++r) {
            const float s = dist2(hx[r], hy[r], hz[r], ax, ay, az);
            const bool cand = valid && p0 + r < P && j != don[r] && gd[r] != 0 && ga != 0 && gd[r] != ga;
            const bool hit = cand && s < s_star && hb_angle(u[r], hx[r], hy[r], hz[r], ax, ay, az, k_cos2);        // (NaN: false)
            const unsigned long long mask = __ballot(hit);
            if (EMIT && hit) {
                const long long k = base[r] + n[r] + __popcll(mask & below);        // < K <= capacity: the count pass saw the same hits
                trip[3 * k] = don[r];
                trip[3 * k + 1] = hyd[r];
                trip[3 * k + 2] = j;
                d[k] = __fmul_rn((float)sqrt((double)s), scale);
            }
            n[r] += __popcll(mask);
        }
    }
    if (!EMIT && lane == 0)
#pragma unroll
        for (int r = 0; r < HB_ROWS; ++r)
            if (p0 + r < P) cnt[f * (size_t)P + p0 + r] = n[r];
}

// ------------------------------------------------------------------------------------------------ occupancy
// replaces: md.baker_hubbard(traj, freq) on a whole trajectory (the reference restarts it per frame, trajectory_utils.py:446-448). A
// workgroup owns HB_TILE donor pairs x a slab of 64 acceptors, a wave HB_ROWS of the pairs and a lane one acceptor of the slab; it loops
// over the frames with the integer count of each of its (p, a) in a register. A triplet qualifies iff (double)n / (double)F > freq. The
// count pass leaves the number of qualifying a of (p, slab) in cnt[p * S + slab]; scanned per donor pair (the list protocol with a donor
// pair in the place of a frame), the emit pass writes the triplets and their n in (p, a) order. No floating-point atomics, no [P, A] array.
template <bool EMIT>
__global__ __launch_bounds__(NT) void k_hb_occupancy(int F, int N, int P, int A, int S, const float* __restrict__ xyz, const int* __restrict__ dh,
                                                     const int* __restrict__ acc, float s_star, double k_cos2, double freq, int* __restrict__ cnt,
                                                     const long long* __restrict__ roff, const ListState* __restrict__ st, int* __restrict__ trip,
                                                     int* __restrict__ n_out) {
    if (st->err || (EMIT && !st->fits)) return;
    const int slab = (int)(blockIdx.x % (unsigned)S);
    const int lane = threadIdx.x & 63;
    const int p0 = (int)(blockIdx.x / (unsigned)S) * HB_TILE + (int)(threadIdx.x >> 6) * HB_ROWS;
    if (p0 >= P) return;                // (the whole wave)
    const int a = slab * 64 + lane;
    const bool valid = a < A;
    const int j = acc[valid ? a : A - 1];
    int don[HB_ROWS], hyd[HB_ROWS], n[HB_ROWS];
#pragma unroll
    for (int r = 0; r < HB_ROWS; ++r) {
        const int p = min(p0 + r, P - 1);
        don[r] = dh[2 * (size_t)p];
        hyd[r] = dh[2 * (size_t)p + 1];
        n[r] = 0;
    }
    for (int f = 0; f < F; ++f) {
        const float* X = xyz + (size_t)f * N * 3;
        const float ax = X[3 * (size_t)j], ay = X[3 * (size_t)j + 1], az = X[3 * (size_t)j + 2];
#pragma unroll
        for (int r = 0; r < HB_ROWS; ++r) {
            const float hx = X[3 * (size_t)hyd[r]], hy = X[3 * (size_t)hyd[r] + 1], hz = X[3 * (size_t)hyd[r] + 2];
            if (dist2(hx, hy, hz, ax, ay, az) < s_star) {
                double u[4];
                hb_u(X[3 * (size_t)don[r]], X[3 * (size_t)don[r] + 1], X[3 * (size_t)don[r] + 2], hx, hy, hz, u);
                n[r] += hb_angle(u, hx, hy, hz, ax, ay, az, k_cos2) ? 1 : 0;
            }
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < HB_ROWS; ++r) {
        const bool hit = valid && p0 + r < P && j != don[r] && (double)n[r] / (double)F > freq;
        const unsigned long long mask = __ballot(hit);
        if (EMIT && hit) {
            const long long k = roff[p0 + r] + cnt[(size_t)(p0 + r) * S + slab] + __popcll(mask & below);
            trip[3 * k] = don[r];
            trip[3 * k + 1] = hyd[r];
            trip[3 * k + 2] = j;
            n_out[k] = n[r];
        }
        if (!EMIT && lane == 0 && p0 + r < P) cnt[(size_t)(p0 + r) * S + slab] = __popcll(mask);
    }
}

// ------------------------------------------------------------------------------------------------ unwrap_pbc
// replaces: unwrap_pbc (trajectory_utils.py:28-64; 27 images of every chain's centre of mass in a Python loop over chains and images, a
// copy of the trajectory). Molecule m holds the atoms perm[off[m] .. off[m + 1]).

// perm must be a permutation of [0, N): every entry in range, and (N entries for N atoms) none named twice; seen[N] starts at zero
__global__ __launch_bounds__(NT) void k_uw_check(int N, const int* __restrict__ perm, int* __restrict__ seen, ListState* __restrict__ st) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const int a = perm[i];
    if (a < 0 || a >= N) atomicOr(&st->err, ERR_PERM);
    else if (atomicAdd(&seen[a], 1) != 0) atomicOr(&st->err, ERR_DUP);
}

// one workgroup per (frame, molecule): com[f, m] = sum(mass x) / sum(mass) in double, thread t taking the atoms t, t + NT, ... of the
// molecule in turn, then block_sum: a fixed order
__global__ __launch_bounds__(NT) void k_uw_com(int N, int M, const float* __restrict__ xyz, const int* __restrict__ perm, const int* __restrict__ off,
                                               const double* __restrict__ mass, const ListState* __restrict__ st, double* __restrict__ com) {
    __shared__ double red[NT / 64];
    if (st->err) return;
    const size_t f = blockIdx.x / (unsigned)M;
    const int m = (int)(blockIdx.x % (unsigned)M);
    const float* X = xyz + f * (size_t)N * 3;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = off[m] + (int)threadIdx.x; k < off[m + 1]; k += NT) {
        const int i = perm[k];
        const double w = mass[i];
        for (int c = 0; c < 3; ++c) s[c] += w * (double)X[3 * (size_t)i + c];
        s[3] += w;
    }
    for (int c = 0; c < 4; ++c) s[c] = block_sum<NT>(s[c], red);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) com[(f * (size_t)M + m) * 3 + c] = s[c] / s[3];
}

// one workgroup per (frame, molecule): the image k of m >= 1 (every thread evaluates the 27 distances alike), then the molecule's atoms
// shifted into out; image[f, m] = k. The images run y slowest, then x, then z, each over (0, 1, -1) - np.meshgrid's default indexing.
// The first k of minimum distance wins; a NaN centre of mass or box length gives k = 0 and a bit copy.
__global__ __launch_bounds__(NT) void k_uw_shift(int N, int M, const float* __restrict__ xyz, const float* __restrict__ box, const int* __restrict__ perm,
                                                 const int* __restrict__ off, const double* __restrict__ com, const ListState* __restrict__ st,
                                                 float* __restrict__ out, int* __restrict__ image) {
    if (st->err) return;
    const size_t f = blockIdx.x / (unsigned)M;
    const int m = (int)(blockIdx.x % (unsigned)M);
    const double L[3] = {(double)box[f * 3], (double)box[f * 3 + 1], (double)box[f * 3 + 2]};
    const double* c0 = com + f * (size_t)M * 3;
    const double* cm = c0 + (size_t)m * 3;
    bool nan = false;
    for (int c = 0; c < 3; ++c) nan = nan || L[c] != L[c] || c0[c] != c0[c] || cm[c] != cm[c];
    int best = 0;
    const double g3[3] = {0.0, 1.0, -1.0};
    if (m > 0 && !nan) {
        double dmin = 0.0;
        for (int k = 0; k < 27; ++k) {
#pragma clang fp contract(off)
            const double tx = __dsub_rn(__dadd_rn(cm[0], __dmul_rn(L[0], g3[(k / 3) % 3])), c0[0]);
            const double ty = __dsub_rn(__dadd_rn(cm[1], __dmul_rn(L[1], g3[k / 9])), c0[1]);
            const double tz = __dsub_rn(__dadd_rn(cm[2], __dmul_rn(L[2], g3[k % 3])), c0[2]);
            const double dist = sqrt(dot3_rn(tx, ty, tz, tx, ty, tz));
            if (k == 0 || dist < dmin) { dmin = dist; best = k; }
        }
    }
    const bool copy = m == 0 || nan;
    const double sh[3] = {L[0] * g3[(best / 3) % 3], L[1] * g3[best / 9], L[2] * g3[best % 3]};
    const float* X = xyz + f * (size_t)N * 3;
    float* Y = out + f * (size_t)N * 3;
    for (int k = off[m] + (int)threadIdx.x; k < off[m + 1]; k += NT) {
        const size_t i = (size_t)perm[k];
        for (int c = 0; c < 3; ++c) Y[3 * i + c] = copy ? X[3 * i + c] : (float)((double)X[3 * i + c] + sh[c]);
    }
    if (threadIdx.x == 0) image[f * (size_t)M + m] = best;
}

// ---- host side
int check_criteria(float r_thr, float scale, double k_cos2) {
    if (!std::isfinite(r_thr) || !(r_thr > 0.f) || !std::isfinite(scale) || !(scale > 0.f))
        return fail(PESTO_ERR_INVALID, "r_thr and scale must be positive and finite");
    if (!(k_cos2 >= 0.0 && k_cos2 < 1.0)) return fail(PESTO_ERR_INVALID, "cos2_angle must lie in [0, 1): an angle in [90, 180) degrees");
    return 0;
}

int check_tables(int64_t F, int64_t N, int64_t P, int64_t A) {
    if (F < 1 || F > PESTO_HBONDS_MAX_FRAMES || N < 1 || N > 0x7fffffff || P < 1 || A < 1 || P > PESTO_HBONDS_MAX_PAIRS ||
        A > PESTO_HBONDS_MAX_PAIRS || P * A > PESTO_HBONDS_MAX_PAIRS)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, 1 <= N < 2^31 atoms and P * A in 1 .. 2^31 - 1 (P = %lld, A = %lld)", (long long)P, (long long)A);
    return 0;
}

int table_errors(int err) {
    if (err & ERR_DH) return fail(PESTO_ERR_INVALID, "dh: atom indices must lie in [0, N)");
    if (err & ERR_ACC) return fail(PESTO_ERR_INVALID, "acc: atom indices must lie in [0, N)");
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_hbonds_last_error(void) { return last_error(); }

int pesto_frame_hbonds(pesto_model* m, int64_t F, int64_t N, int64_t P, int64_t A, const float* xyz, const int32_t* dh, const int32_t* acc,
                       const int8_t* group, float r_thr, float scale, double cos2_angle, int64_t cap, int64_t* offsets_out, int32_t* triplets_out,
                       float* d_out, int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (!xyz || !dh || !acc || !offsets_out || !triplets_out || !d_out || !sizes_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_tables(F, N, P, A)) return rc;
    const int64_t tiles = (P + HB_TILE - 1) / HB_TILE;
    if (F * tiles >= (1 << 24)) return fail(PESTO_ERR_INVALID, "too many workgroups: F * ceil(P / %d) must stay below 2^24 (a grid below 2^32 threads)", HB_TILE);
    if (cap < 1 || cap > PESTO_HBONDS_MAX_LIST) return fail(PESTO_ERR_INVALID, "cap must be in [1, 2^30)");
    if (int rc = check_criteria(r_thr, scale, cos2_angle)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_star = contact_threshold(r_thr, scale, true);
    const size_t C = (size_t)cap;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iDh = bf.input(dh, (size_t)P * 8), iAc = bf.input(acc, (size_t)A * 4), iG = bf.input(group, (size_t)N);
    const int iO = bf.output(offsets_out, ((size_t)F + 1) * 8), iT = bf.partial(triplets_out, C * 12), iD = bf.partial(d_out, C * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iCnt = bf.scratch((size_t)F * P * 4, 0), iTot = bf.scratch((size_t)F * 4);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const dim3 grid((unsigned)(F * tiles));
        const float* X = bf.ptr<const float>(iX);
        const int *pdh = bf.ptr<const int>(iDh), *pac = bf.ptr<const int>(iAc);
        const signed char* pg = bf.ptr<const signed char>(iG);
        ListState* st = bf.ptr<ListState>(iSt);
        hipLaunchKernelGGL(k_hb_check, dim3(blocks((size_t)(2 * P + A), NT)), dim3(NT), 0, bf.stm, (int)N, (int)P, (int)A, pdh, pac, st);
        hipLaunchKernelGGL(k_hb_pairs<false>, grid, dim3(NT), 0, bf.stm, (int)N, (int)P, (int)A, (int)tiles, X, pdh, pac, pg, s_star, scale, cos2_angle,
                           bf.ptr<int>(iCnt), (const long long*)nullptr, (const ListState*)st, (int*)nullptr, (float*)nullptr);
        list_scan<NT>(bf, (int)F, (int)P, iCnt, iTot, iO, (long long)cap, iSt);
        hipLaunchKernelGGL(k_hb_pairs<true>, grid, dim3(NT), 0, bf.stm, (int)N, (int)P, (int)A, (int)tiles, X, pdh, pac, pg, s_star, scale, cos2_angle,
                           bf.ptr<int>(iCnt), bf.ptr<const long long>(iO), (const ListState*)st, bf.ptr<int>(iT), bf.ptr<float>(iD));
    }
    // the one synchronisation for sizing: the count
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "frame_hbonds");
    if (rc == 0 && !hs.err) rc = list_tail(bf, hs, sizes_out, {{iT, 12}, {iD, 4}});
    rc = bf.finish(rc, "frame_hbonds");
    return rc ? rc : table_errors(hs.err);
}

int pesto_hbond_occupancy(pesto_model* m, int64_t F, int64_t N, int64_t P, int64_t A, const float* xyz, const int32_t* dh, const int32_t* acc,
                          float r_thr, float scale, double cos2_angle, double freq, int64_t cap, int32_t* triplets_out, int32_t* counts_out,
                          int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (!xyz || !dh || !acc || !triplets_out || !counts_out || !sizes_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_tables(F, N, P, A)) return rc;
    if (cap < 1 || cap > PESTO_HBONDS_MAX_LIST) return fail(PESTO_ERR_INVALID, "cap must be in [1, 2^30)");
    if (int rc = check_criteria(r_thr, scale, cos2_angle)) return rc;
    if (!(freq >= 0.0) || !std::isfinite(freq)) return fail(PESTO_ERR_INVALID, "freq must be finite and not negative");
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_star = contact_threshold(r_thr, scale, true);
    const int64_t tiles = (P + HB_TILE - 1) / HB_TILE, S = (A + 63) / 64;           // tiles * S <= (P * A) / 2048 + P + A: below 2^32 threads
    const size_t C = (size_t)cap;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iDh = bf.input(dh, (size_t)P * 8), iAc = bf.input(acc, (size_t)A * 4);
    const int iT = bf.partial(triplets_out, C * 12), iN = bf.partial(counts_out, C * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iCnt = bf.scratch((size_t)P * S * 4, 0), iTot = bf.scratch((size_t)P * 4),
              iO = bf.scratch(((size_t)P + 1) * 8);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const dim3 grid((unsigned)(tiles * S));
        const float* X = bf.ptr<const float>(iX);
        const int *pdh = bf.ptr<const int>(iDh), *pac = bf.ptr<const int>(iAc);
        ListState* st = bf.ptr<ListState>(iSt);
        hipLaunchKernelGGL(k_hb_check, dim3(blocks((size_t)(2 * P + A), NT)), dim3(NT), 0, bf.stm, (int)N, (int)P, (int)A, pdh, pac, st);
        hipLaunchKernelGGL(k_hb_occupancy<false>, grid, dim3(NT), 0, bf.stm, (int)F, (int)N, (int)P, (int)A, (int)S, X, pdh, pac, s_star, cos2_angle, freq,
                           bf.ptr<int>(iCnt), (const long long*)nullptr, (const ListState*)st, (int*)nullptr, (int*)nullptr);
        list_scan<NT>(bf, (int)P, (int)S, iCnt, iTot, iO, (long long)cap, iSt);
        hipLaunchKernelGGL(k_hb_occupancy<true>, grid, dim3(NT), 0, bf.stm, (int)F, (int)N, (int)P, (int)A, (int)S, X, pdh, pac, s_star, cos2_angle, freq,
                           bf.ptr<int>(iCnt), bf.ptr<const long long>(iO), (const ListState*)st, bf.ptr<int>(iT), bf.ptr<int>(iN));
    }
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "hbond_occupancy");
    if (rc == 0 && !hs.err) rc = list_tail(bf, hs, sizes_out, {{iT, 12}, {iN, 4}});
    rc = bf.finish(rc, "hbond_occupancy");
    return rc ? rc : table_errors(hs.err);
}

int pesto_unwrap_pbc(pesto_model* m, int64_t F, int64_t N, int64_t M, const float* xyz, const float* unitcell_lengths, const int32_t* perm,
                     const int32_t* mol_off, const double* masses, float* xyz_out, int32_t* image_out, int32_t ptr_kind, void* stream) {
    if (!xyz || !unitcell_lengths || !perm || !mol_off || !masses || !xyz_out || !image_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_HBONDS_MAX_FRAMES || N < 1 || N > 0x7fffffff || M < 1 || M > N || F * M > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, 1 <= M <= N < 2^31 and F * M below 2^31");
    if (int rc = check_offsets(mol_off, (int32_t)M, N, "mol_off", "molecule")) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz, (size_t)F * N * 12), iL = bf.input(unitcell_lengths, (size_t)F * 12), iP = bf.input(perm, (size_t)N * 4),
              iOf = bf.table(mol_off, ((size_t)M + 1) * 4), iMs = bf.input(masses, (size_t)N * 8);
    const int iY = bf.output(xyz_out, (size_t)F * N * 12), iIm = bf.output(image_out, (size_t)F * M * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iCm = bf.scratch((size_t)F * M * 24), iSeen = bf.scratch((size_t)N * 4, 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const dim3 grid((unsigned)(F * M));
        ListState* st = bf.ptr<ListState>(iSt);
        hipLaunchKernelGGL(k_uw_check, dim3(blocks((size_t)N, NT)), dim3(NT), 0, bf.stm, (int)N, bf.ptr<const int>(iP), bf.ptr<int>(iSeen), st);
        hipLaunchKernelGGL(k_uw_com, grid, dim3(NT), 0, bf.stm, (int)N, (int)M, bf.ptr<const float>(iX), bf.ptr<const int>(iP), bf.ptr<const int>(iOf),
                           bf.ptr<const double>(iMs), (const ListState*)st, bf.ptr<double>(iCm));
        hipLaunchKernelGGL(k_uw_shift, grid, dim3(NT), 0, bf.stm, (int)N, (int)M, bf.ptr<const float>(iX), bf.ptr<const float>(iL), bf.ptr<const int>(iP),
                           bf.ptr<const int>(iOf), bf.ptr<const double>(iCm), (const ListState*)st, bf.ptr<float>(iY), bf.ptr<int>(iIm));
    }
    // (decoded after finish(), whose synchronisation brings it)
    if (rc == 0) rc = bf.read(iSt, &hs, sizeof hs);
    rc = bf.finish(rc, "unwrap_pbc");
    if (rc == 0 && (hs.err & ERR_PERM)) rc = fail(PESTO_ERR_INVALID, "perm: atom indices must lie in [0, N)");
    if (rc == 0 && (hs.err & ERR_DUP)) rc = fail(PESTO_ERR_INVALID, "perm: every atom must be named once (an index is repeated)");
    return rc;
}
