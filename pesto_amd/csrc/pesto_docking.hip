// pesto_docking.hip - how a complex holds together over an MD run: the per-frame contact lists between two subunits, their residue pairs
// with the minimum distance, the interface atoms of the reference frame and the rigid-body pose of the ligand against its bound pose.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h.
//
// Distances are the float32 ones of pesto_trajectory.hip, d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale). Membership
// (d < r_thr, d <= r_thr) is decided on the rounded sum s against the smallest float s_star at which the test fails (the product is
// monotonic in s; the host derives s_star by bisection over the float bit patterns); only an emitted contact takes the root, in double and
// rounded once to float32, which is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits).
// The lists come out of count -> scan -> emit with every position fixed by the scans; the residue pairs are the set bits of a per-frame
// [Ra, Rb] bit map in index order, their minimum an integer atomicMin over the bits of the non-negative d; the pose and the interface RMSD
// are evaluated in double in a fixed order by the superposition fit of pesto_fit.h, the one pesto_trajectory.hip and pesto_dockq.hip
// call (hence the interface RMSD's bits: pesto_superpose's off the reference frame, pesto_dockq's everywhere). Every output is
// bit-identical from call to call.
#include <cmath>

#include "pesto_call.h"
#include "pesto_scan.h"
#include "pesto_fit.h"           // (and pesto_geom.h through it)

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup of every kernel here
constexpr int FC_ROWS = 8;              // frame contacts: atoms of A per wave (their partners' coordinates are loaded once for all of them)
constexpr int FC_TILE = FC_ROWS * NT / 64;      // ... and per workgroup

// err of the call's ListState (pesto_scan.h): bit 0: an atom index outside its side; bit 1: a residue row outside 0 .. R - 1

// ------------------------------------------------------------------------------------------------ frame contacts
// replaces: the frame loop of contacts (md_analysis/mdtraj_utils/trajectory_utils.py:408-423; a dense [Na, Nb] matrix, torch.where and
// three copies to the host per frame). Tiled brute force: a workgroup owns FC_TILE atoms of A in one frame, a wave FC_ROWS of them; its
// lanes walk B 64 atoms at a time, each lane's partner tested against the wave's FC_ROWS atoms. A ballot orders the hits of a row by j,
// so the count pass (EMIT = false: cnt[f * Na + i]) and the emit pass (into [foff[f] + cnt[f * Na + i] ...), cnt scanned per frame by
// then) see the same hits in the same order: the rows fill exactly, in torch.where order.
template <bool EMIT>
__global__ __launch_bounds__(NT) void k_fc_pairs(int Na, int Nb, int tiles, const float* __restrict__ xa, const float* __restrict__ xb, float s_star,
                                                 float scale, int* __restrict__ cnt, const long long* __restrict__ foff,
                                                 const ListState* __restrict__ st, int* __restrict__ pairs, float* __restrict__ d) {
    if (EMIT && !st->fits) return;
    const size_t f = blockIdx.x / (unsigned)tiles;
    const int lane = threadIdx.x & 63;
    const int i0 = (int)(blockIdx.x % (unsigned)tiles) * FC_TILE + (int)(threadIdx.x >> 6) * FC_ROWS;
    if (i0 >= Na) return;               // (the whole wave)
    const float* A = xa + f * (size_t)Na * 3;
    const float* B = xb + f * (size_t)Nb * 3;
    float ax[FC_ROWS], ay[FC_ROWS], az[FC_ROWS];
    int n[FC_ROWS];
    long long base[FC_ROWS];
#pragma unroll
    for (int r = 0; r < FC_ROWS; ++r) {
        const int i = min(i0 + r, Na - 1);              // (a row past the end repeats the last one and is never counted)
        ax[r] = A[3 * (size_t)i]; ay[r] = A[3 * (size_t)i + 1]; az[r] = A[3 * (size_t)i + 2];
        n[r] = 0;
        base[r] = EMIT ? foff[f] + cnt[f * (size_t)Na + i] : 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j0 = 0; j0 < Nb; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < Nb;
        const int jj = valid ? j : Nb - 1;
        const float bx = B[3 * (size_t)jj], by = B[3 * (size_t)jj + 1], bz = B[3 * (size_t)jj + 2];
#pragma unroll
        for (int r = 0; r < FC_ROWS; ++r) {
            const float s = dist2(ax[r], ay[r], az[r], bx, by, bz);
            const bool hit = valid && i0 + r < Na && s < s_star;       // (NaN: false)
            const unsigned long long mask = __ballot(hit);
            if (EMIT && hit) {
                const long long k = base[r] + n[r] + __popcll(mask & below);        // < K <= capacity: the count pass saw the same hits
                pairs[2 * k] = i0 + r;
                pairs[2 * k + 1] = j;
                d[k] = __fmul_rn((float)sqrt((double)s), scale);
            }
            n[r] += __popcll(mask);
        }
    }
    if (!EMIT && lane == 0)
#pragma unroll
        for (int r = 0; r < FC_ROWS; ++r)
            if (i0 + r < Na) cnt[f * (size_t)Na + i0 + r] = n[r];
}

// (the per-frame scan k_frame_scan and the 64-bit offsets k_list_offsets: pesto_scan.h)

// ------------------------------------------------------------------------------------------------ residue contacts
// replaces: atoms_to_residue_contacts (trajectory_utils.py:233-264; np.unique and a Python loop per frame and residue pair). Frame f owns
// W words of a bit map over (ra, rb), bit ra * Rb + rb: mark sets the bit of every contact, the set bits in index order are the residue
// pairs in lexicographic order (count -> scan -> emit, as above), and every contact lowers its pair's minimum - an unsigned atomicMin over
// the bits of the non-negative float d, which no order of arrival changes.

// the word and bit of contact k, false (and an error bit) for an index outside its range
__device__ __forceinline__ bool contact_bit(long long k, int F, int Na, int Nb, int Ra, int Rb, int W, const long long* __restrict__ off,
                                            const int* __restrict__ pairs, const int* __restrict__ res_a, const int* __restrict__ res_b,
                                            ListState* __restrict__ st, size_t& word, int& bit) {
    const int i = pairs[2 * k], j = pairs[2 * k + 1];
    if (i < 0 || i >= Na || j < 0 || j >= Nb) { atomicOr(&st->err, 1); return false; }
    const int ra = res_a[i], rb = res_b[j];
    if (ra < 0 || ra >= Ra || rb < 0 || rb >= Rb) { atomicOr(&st->err, 2); return false; }
    const long long b = (long long)ra * Rb + rb;
    word = (size_t)struct_of(k, F, off) * W + (size_t)(b >> 5);
    bit = (int)(b & 31);
    return true;
}

__global__ __launch_bounds__(NT) void k_rc_mark(long long K, int F, int Na, int Nb, int Ra, int Rb, int W, const long long* __restrict__ off,
                                                const int* __restrict__ pairs, const int* __restrict__ res_a, const int* __restrict__ res_b,
                                                ListState* __restrict__ st, unsigned* __restrict__ bits) {
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    if (k >= K) return;
    size_t word;
    int bit;
    if (contact_bit(k, F, Na, Nb, Ra, Rb, W, off, pairs, res_a, res_b, st, word, bit)) atomicOr(&bits[word], 1u << bit);
}

__global__ __launch_bounds__(NT) void k_rc_count(size_t n_words, const unsigned* __restrict__ bits, int* __restrict__ cnt) {
    const size_t w = (size_t)blockIdx.x * NT + threadIdx.x;
    if (w < n_words) cnt[w] = __popc(bits[w]);
}

// the residue pairs of every word's set bits, their minimum at +inf
__global__ __launch_bounds__(NT) void k_rc_emit(size_t n_words, int W, int Rb, const unsigned* __restrict__ bits, const int* __restrict__ woff,
                                                const long long* __restrict__ roff, const ListState* __restrict__ st, int* __restrict__ rpairs,
                                                unsigned* __restrict__ dmin_bits) {
    if (!st->fits) return;
    const size_t w = (size_t)blockIdx.x * NT + threadIdx.x;
    if (w >= n_words) return;
    unsigned m = bits[w];
    long long u = roff[w / (size_t)W] + woff[w];
    const long long first = (long long)(w % (size_t)W) * 32;
    while (m) {
        const long long b = first + (__ffs(m) - 1);
        m &= m - 1;
        rpairs[2 * u] = (int)(b / Rb);
        rpairs[2 * u + 1] = (int)(b % Rb);
        dmin_bits[u] = 0x7f800000u;
        ++u;
    }
}

__global__ __launch_bounds__(NT) void k_rc_min(long long K, int F, int Na, int Nb, int Ra, int Rb, int W, const long long* __restrict__ off,
                                               const int* __restrict__ pairs, const float* __restrict__ d, const int* __restrict__ res_a,
                                               const int* __restrict__ res_b, ListState* __restrict__ st, const unsigned* __restrict__ bits,
                                               const int* __restrict__ woff, const long long* __restrict__ roff, unsigned* __restrict__ dmin_bits) {
    if (!st->fits) return;
    const long long k = (long long)blockIdx.x * NT + threadIdx.x;
    if (k >= K) return;
    size_t word;
    int bit;
    if (!contact_bit(k, F, Na, Nb, Ra, Rb, W, off, pairs, res_a, res_b, st, word, bit)) return;
    const long long u = roff[word / (size_t)W] + woff[word] + __popc(bits[word] & ((1u << bit) - 1u));
    atomicMin(&dmin_bits[u], __float_as_uint(d[k]));
}

// ------------------------------------------------------------------------------------------------ interface atoms
// replaces: interface_residues_within (trajectory_utils.py:267-297; a dense distance matrix and an [N, residues] isclose matrix). Thread t
// owns an atom of ids_a (then of ids_b) and stops at its first partner of the other subunit with s < s_star; its residue is flagged (an
// idempotent store), and every atom of the topology takes the flag of its residue. rflag: [2][R], zeroed.
__global__ __launch_bounds__(NT) void k_ia_hits(int N, int na, int nb, int R, const float* __restrict__ x, const int* __restrict__ ids_a,
                                                const int* __restrict__ ids_b, const int* __restrict__ res, float s_star, int* __restrict__ rflag,
                                                ListState* __restrict__ st) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= na + nb) return;
    const bool side_b = t >= na;
    const int* own = side_b ? ids_b : ids_a;
    const int* other = side_b ? ids_a : ids_b;
    const int n_other = side_b ? na : nb;
    const int i = own[side_b ? t - na : t];
    if (i < 0 || i >= N) { atomicOr(&st->err, 1); return; }
    const int r = res[i];
    if (r < 0 || r >= R) { atomicOr(&st->err, 2); return; }
    const float ax = x[3 * (size_t)i], ay = x[3 * (size_t)i + 1], az = x[3 * (size_t)i + 2];
    for (int k = 0; k < n_other; ++k) {
        const int j = other[k];
        if (j < 0 || j >= N) { atomicOr(&st->err, 1); return; }
        if (dist2(ax, ay, az, x[3 * (size_t)j], x[3 * (size_t)j + 1], x[3 * (size_t)j + 2]) < s_star) {
            rflag[(side_b ? R : 0) + r] = 1;
            return;
        }
    }
}

__global__ __launch_bounds__(NT) void k_ia_flags(int N, int R, const int* __restrict__ res, const int* __restrict__ rflag, ListState* __restrict__ st,
                                                 unsigned char* __restrict__ flags) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const int r = res[i];
    const bool ok = r >= 0 && r < R;
    if (!ok) atomicOr(&st->err, 2);
    flags[i] = ok && rflag[r] ? 1 : 0;
    flags[(size_t)N + i] = ok && rflag[R + r] ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ rigid docking
// replaces: interface_rigid_docking (trajectory_utils.py:474-499; two batched SVD superpositions with a transformed copy of the whole
// trajectory between them, then scipy's rotation vector). One workgroup per frame, everything in double from the float32 inputs:
//   1  fit the frame onto the reference on the receptor selection: t1, R1, t_ref1 - kabsch_fit of pesto_fit.h, the fit of
//      k_superpose_fit (pesto_trajectory.hip) and of pesto_dockq.hip
//   2  x' = (x - t1) R1 + t_ref1 for the ligand selection only (moved, pesto_fit.h), recomputed in each pass instead of stored
//   3  fit x' onto the reference's ligand selection, the same function again: t_cm = mean(x'), t_ref2, R2
//   4  t = t_ref2 - t_cm; r = the rotation vector of R2
// A selection that equals the reference's bit for bit is fitted by the identity itself, not by a rotation within rounding of it (step 1:
// x' = x; step 3: R2 = I), so a frame that is the reference gives t = 0 and r = 0 exactly.

// the rotation vector of R (row-major; the matrix scipy's Rotation.from_matrix reads): the unit quaternion by the largest of the trace
// and the diagonal, w >= 0, angle = 2 atan2(|v|, w) in [0, pi], r = angle v / |v| (0 for the identity)
__device__ void rotation_vector(const double* R, double* r) {
    const double trace = R[0] + R[4] + R[8];
    int c = 3;
    double best = trace;
    for (int k = 0; k < 3; ++k)
        if (R[4 * k] > best) { best = R[4 * k]; c = k; }
    double q[4];
    if (c == 3) {
        q[0] = R[7] - R[5]; q[1] = R[2] - R[6]; q[2] = R[3] - R[1]; q[3] = 1.0 + trace;
    } else {
        const int i = c, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1.0 - trace + 2.0 * R[4 * i];
        q[j] = R[3 * j + i] + R[3 * i + j];
        q[k] = R[3 * k + i] + R[3 * i + k];
        q[3] = R[3 * k + j] - R[3 * j + k];
    }
    const double sign = q[3] < 0.0 ? -1.0 : 1.0;
    const double v = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double angle = 2.0 * atan2(v, sign * q[3]);
    for (int a = 0; a < 3; ++a) r[a] = v > 0.0 ? angle * (sign * q[a] / v) : 0.0;
}

// the pose of every frame; behind k_index_check (pesto_fit.h), which refuses a selection index outside [0, N) before anything here
// dereferences it. (The interface RMSD is k_fit_rmsd of pesto_fit.h, fitted and measured on the one selection.)
__global__ __launch_bounds__(NT) void k_rigid_docking(int Fr, int N, int nR, int nL, const float* __restrict__ ref, const float* __restrict__ xyz,
                                                      const int* __restrict__ sel_R, const int* __restrict__ sel_L, const int* __restrict__ err,
                                                      float* __restrict__ t_out, float* __restrict__ r_out) {
    __shared__ double red[NT / 64];
    __shared__ double sR[9];
    if (*err) return;
    const size_t f = blockIdx.x;
    const float* X = xyz + f * (size_t)N * 3;
    const float* Y = ref + (Fr == 1 ? 0 : f) * (size_t)N * 3;
    Fit rec, lig;
    kabsch_fit<NT, true>(atoms(X, sel_R), atoms(Y, sel_R), nR, red, sR, rec);                                  // 1
    const auto ligand = atoms(X, sel_L);
    const auto moved_ligand = [=](int k, double* p) { double x[3]; ligand(k, x); moved(x, rec, p); };         // 2
    kabsch_fit<NT, true>(moved_ligand, atoms(Y, sel_L), nL, red, sR, lig);                                     // 3
    if (threadIdx.x == 0) {                                                                                    // 4
        double r[3] = {0.0, 0.0, 0.0};
        if (!lig.same) rotation_vector(sR, r);          // (lig.R where the fit left it: LDS takes rotation_vector's run-time indices)
        for (int c = 0; c < 3; ++c) {
            t_out[f * 3 + c] = (float)(lig.m[3 + c] - lig.m[c]);
            r_out[f * 3 + c] = (float)r[c];
        }
    }
}

// ---- host side
// (contact_threshold, the smallest float s whose distance fails the test: pesto_geom.h)
int check_cutoff(float r_thr, float scale) {
    if (!std::isfinite(r_thr) || !std::isfinite(scale) || !(scale > 0.f)) return fail(PESTO_ERR_INVALID, "r_thr must be finite and scale positive and finite");
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_docking_last_error(void) { return last_error(); }

int pesto_frame_contacts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, float r_thr, float scale,
                         int64_t cap_pairs, int64_t* offsets_out, int32_t* pairs_out, float* d_out, int64_t* sizes_out, int32_t ptr_kind,
                         void* stream) {
    if (!xyz_a || !xyz_b || !offsets_out || !pairs_out || !d_out || !sizes_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKING_MAX_FRAMES || Na < 1 || Nb < 1 || Na > 0x7fffffff || Nb > 0x7fffffff || Na * Nb > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames and Na * Nb in 1 .. 2^31 - 1 (Na = %lld, Nb = %lld)", (long long)Na, (long long)Nb);
    const int64_t tiles = (Na + FC_TILE - 1) / FC_TILE;
    if (F * tiles >= (1 << 24)) return fail(PESTO_ERR_INVALID, "too many workgroups: F * ceil(Na / %d) must stay below 2^24 (a grid below 2^32 threads)", FC_TILE);
    if (cap_pairs < 1 || cap_pairs > 0x3fffffff) return fail(PESTO_ERR_INVALID, "cap_pairs must be in [1, 2^30)");
    if (int rc = check_cutoff(r_thr, scale)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_star = contact_threshold(r_thr, scale, true);
    const size_t C = (size_t)cap_pairs;
    Buffers bf(ptr_kind, stream);
    const int iA = bf.input(xyz_a, (size_t)F * Na * 12), iB = bf.input(xyz_b, (size_t)F * Nb * 12);
    const int iO = bf.output(offsets_out, ((size_t)F + 1) * 8), iP = bf.partial(pairs_out, C * 8), iD = bf.partial(d_out, C * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iCnt = bf.scratch((size_t)F * Na * 4), iTot = bf.scratch((size_t)F * 4);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const dim3 grid((unsigned)(F * tiles));
        hipLaunchKernelGGL(k_fc_pairs<false>, grid, dim3(NT), 0, bf.stm, (int)Na, (int)Nb, (int)tiles, bf.ptr<const float>(iA), bf.ptr<const float>(iB),
                           s_star, scale, bf.ptr<int>(iCnt), (const long long*)nullptr, (const ListState*)nullptr, (int*)nullptr, (float*)nullptr);
        list_scan<NT>(bf, (int)F, (int)Na, iCnt, iTot, iO, (long long)cap_pairs, iSt);
        hipLaunchKernelGGL(k_fc_pairs<true>, grid, dim3(NT), 0, bf.stm, (int)Na, (int)Nb, (int)tiles, bf.ptr<const float>(iA), bf.ptr<const float>(iB),
                           s_star, scale, bf.ptr<int>(iCnt), bf.ptr<const long long>(iO), bf.ptr<const ListState>(iSt), bf.ptr<int>(iP),
                           bf.ptr<float>(iD));
    }
    // the one synchronisation for sizing: the count
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "frame_contacts");
    if (rc == 0) rc = list_tail(bf, hs, sizes_out, {{iP, 8}, {iD, 4}});
    return bf.finish(rc, "frame_contacts");
}

int pesto_frame_residue_contacts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, int64_t K, const int64_t* offsets, const int32_t* pairs,
                                 const float* d, const int32_t* res_a, const int32_t* res_b, int32_t Ra, int32_t Rb, int64_t cap_rpairs,
                                 int64_t* roffsets_out, int32_t* rpairs_out, float* dmin_out, int64_t* sizes_out, int32_t ptr_kind, void* stream) {
    if (!offsets || !res_a || !res_b || !roffsets_out || !rpairs_out || !dmin_out || !sizes_out || (K > 0 && (!pairs || !d)))
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKING_MAX_FRAMES || Na < 1 || Nb < 1 || Na > 0x7fffffff || Nb > 0x7fffffff || K < 0 || K > 0x3fffffff)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, 1 <= Na, Nb < 2^31 and 0 <= K < 2^30 contacts");
    if (Ra < 1 || Rb < 1 || Ra > Na || Rb > Nb) return fail(PESTO_ERR_INVALID, "1 <= Ra <= Na and 1 <= Rb <= Nb residues");
    const int64_t W = ((int64_t)Ra * Rb + 31) / 32;
    if (F * W > PESTO_DOCKING_MAX_MAP_WORDS)
        return fail(PESTO_ERR_INVALID, "F * ceil(Ra * Rb / 32) = %lld exceeds %d map words: pass the frames in batches", (long long)(F * W),
                    PESTO_DOCKING_MAX_MAP_WORDS);
    if (cap_rpairs < 1 || cap_rpairs > 0x3fffffff) return fail(PESTO_ERR_INVALID, "cap_rpairs must be in [1, 2^30)");
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t n_words = (size_t)(F * W), C = (size_t)cap_rpairs, Kz = (size_t)K;
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.input(offsets, ((size_t)F + 1) * 8), iP = bf.input(pairs, Kz * 8), iD = bf.input(d, Kz * 4), iRa = bf.input(res_a, (size_t)Na * 4),
              iRb = bf.input(res_b, (size_t)Nb * 4);
    const int iO = bf.output(roffsets_out, ((size_t)F + 1) * 8), iRp = bf.partial(rpairs_out, C * 8), iDm = bf.partial(dmin_out, C * 4);
    const int iSt = bf.scratch(sizeof(ListState), 0), iBits = bf.scratch(n_words * 4, 0), iCnt = bf.scratch(n_words * 4), iTot = bf.scratch((size_t)F * 4);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        const long long* off = bf.ptr<const long long>(iOff);
        const int *pr = bf.ptr<const int>(iP), *ra = bf.ptr<const int>(iRa), *rb = bf.ptr<const int>(iRb);
        ListState* st = bf.ptr<ListState>(iSt);
        if (K > 0)
            hipLaunchKernelGGL(k_rc_mark, dim3(blocks(Kz, NT)), dim3(NT), 0, bf.stm, (long long)K, (int)F, (int)Na, (int)Nb, Ra, Rb, (int)W, off, pr, ra, rb, st,
                               bf.ptr<unsigned>(iBits));
        hipLaunchKernelGGL(k_rc_count, dim3(blocks(n_words, NT)), dim3(NT), 0, bf.stm, n_words, bf.ptr<const unsigned>(iBits), bf.ptr<int>(iCnt));
        list_scan<NT>(bf, (int)F, (int)W, iCnt, iTot, iO, (long long)cap_rpairs, iSt);
        hipLaunchKernelGGL(k_rc_emit, dim3(blocks(n_words, NT)), dim3(NT), 0, bf.stm, n_words, (int)W, Rb, bf.ptr<const unsigned>(iBits),
                           bf.ptr<const int>(iCnt), bf.ptr<const long long>(iO), (const ListState*)st, bf.ptr<int>(iRp), bf.ptr<unsigned>(iDm));
        if (K > 0)
            hipLaunchKernelGGL(k_rc_min, dim3(blocks(Kz, NT)), dim3(NT), 0, bf.stm, (long long)K, (int)F, (int)Na, (int)Nb, Ra, Rb, (int)W, off, pr,
                               bf.ptr<const float>(iD), ra, rb, st, bf.ptr<const unsigned>(iBits), bf.ptr<const int>(iCnt), bf.ptr<const long long>(iO),
                               bf.ptr<unsigned>(iDm));
    }
    // the one synchronisation for sizing: the count
    if (rc == 0) rc = bf.verdict(iSt, &hs, sizeof hs, "frame_residue_contacts");
    if (rc == 0) rc = list_tail(bf, hs, sizes_out, {{iRp, 8}, {iDm, 4}}, !hs.err);
    rc = bf.finish(rc, "frame_residue_contacts");
    if (rc == 0 && (hs.err & 1)) rc = fail(PESTO_ERR_INVALID, "pairs: atom indices must lie in [0, Na) and [0, Nb)");
    if (rc == 0 && (hs.err & 2)) rc = fail(PESTO_ERR_INVALID, "res_a / res_b: residue rows must lie in [0, Ra) and [0, Rb)");
    return rc;
}

int pesto_interface_atoms(pesto_model* m, int64_t N, const float* xyz0, int64_t na, const int32_t* ids_a, int64_t nb, const int32_t* ids_b,
                          const int32_t* res_of_atom, int32_t R, float r_thr, float scale, uint8_t* flags_out, int32_t ptr_kind, void* stream) {
    if (!xyz0 || !ids_a || !ids_b || !res_of_atom || !flags_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (N < 1 || N > 0x3fffffff || na < 1 || nb < 1 || na > N || nb > N || R < 1 || R > N)
        return fail(PESTO_ERR_INVALID, "1 <= N < 2^30 atoms, 1 <= na, nb <= N selected and 1 <= R <= N residues");
    if (int rc = check_cutoff(r_thr, scale)) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_star = contact_threshold(r_thr, scale, false);
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(xyz0, (size_t)N * 12), iA = bf.input(ids_a, (size_t)na * 4), iB = bf.input(ids_b, (size_t)nb * 4),
              iR = bf.input(res_of_atom, (size_t)N * 4), iF = bf.output(flags_out, (size_t)N * 2);
    const int iSt = bf.scratch(sizeof(ListState), 0), iRf = bf.scratch((size_t)R * 8, 0);
    ListState hs = {};
    int rc = bf.upload();
    if (rc == 0) {
        hipLaunchKernelGGL(k_ia_hits, dim3(blocks((size_t)(na + nb), NT)), dim3(NT), 0, bf.stm, (int)N, (int)na, (int)nb, R, bf.ptr<const float>(iX),
                           bf.ptr<const int>(iA), bf.ptr<const int>(iB), bf.ptr<const int>(iR), s_star, bf.ptr<int>(iRf), bf.ptr<ListState>(iSt));
        hipLaunchKernelGGL(k_ia_flags, dim3(blocks((size_t)N, NT)), dim3(NT), 0, bf.stm, (int)N, R, bf.ptr<const int>(iR), bf.ptr<const int>(iRf),
                           bf.ptr<ListState>(iSt), bf.ptr<unsigned char>(iF));
    }
    // (decoded after finish(), whose synchronisation brings it)
    if (rc == 0) rc = bf.read(iSt, &hs, sizeof hs);
    rc = bf.finish(rc, "interface_atoms");
    if (rc == 0 && (hs.err & 1)) rc = fail(PESTO_ERR_INVALID, "ids_a / ids_b: atom indices must lie in [0, N)");
    if (rc == 0 && (hs.err & 2)) rc = fail(PESTO_ERR_INVALID, "res_of_atom: residue rows must lie in [0, R)");
    return rc;
}

namespace {

// the pose (t_out, r_out: k_rigid_docking) or the interface RMSD (rmsd_out: k_fit_rmsd on sel_R alone) of every frame, behind the index check
int launch_docking(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_R, const int32_t* sel_R,
                   int64_t n_L, const int32_t* sel_L, float* t_out, float* r_out, float* rmsd_out, double scale, int32_t ptr_kind, void* stream,
                   const char* what) {
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)F_ref * N * 12), iX = bf.input(xyz, (size_t)F * N * 12), iSr = bf.input(sel_R, (size_t)n_R * 4),
              iSl = bf.input(sel_L, (size_t)n_L * 4), iT = bf.output(t_out, (size_t)F * 12), iRv = bf.output(r_out, (size_t)F * 12),
              iRm = bf.output(rmsd_out, (size_t)F * 4), iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const IndexLists idx = {{bf.ptr<const int>(iSr), bf.ptr<const int>(iSl)}, {n_R, n_L}};
        hipLaunchKernelGGL(k_index_check<NT>, dim3(blocks((size_t)idx.total(), NT)), dim3(NT), 0, bf.stm, (int)N, idx, bf.ptr<int>(iSt));
        if (t_out)
            hipLaunchKernelGGL(k_rigid_docking, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)F_ref, (int)N, (int)n_R, (int)n_L, bf.ptr<const float>(iY),
                               bf.ptr<const float>(iX), bf.ptr<const int>(iSr), bf.ptr<const int>(iSl), bf.ptr<const int>(iSt), bf.ptr<float>(iT),
                               bf.ptr<float>(iRv));
        else
            hipLaunchKernelGGL(k_fit_rmsd<NT>, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)F_ref, (int)N, (int)n_R, (int)n_R, bf.ptr<const float>(iY),
                               bf.ptr<const float>(iX), bf.ptr<const int>(iSr), bf.ptr<const int>(iSr), bf.ptr<const int>(iSt), scale, bf.ptr<float>(iRm));
    }
    if (rc == 0) rc = bf.read(iSt, &herr, sizeof herr);
    rc = bf.finish(rc, what);
    if (rc == 0 && herr) rc = fail(PESTO_ERR_INVALID, "%s: atom indices of a selection must lie in [0, N)", what);
    return rc;
}

}  // namespace

int pesto_rigid_docking(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_R,
                        const int32_t* sel_R, int64_t n_L, const int32_t* sel_L, float* t_out, float* r_out, int32_t ptr_kind, void* stream) {
    if (!xyz_ref || !xyz || !sel_R || !sel_L || !t_out || !r_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKING_MAX_FRAMES || (F_ref != 1 && F_ref != F) || N < 1 || N > 0x7fffffff || n_R < 3 || n_L < 3 || n_R > N || n_L > N)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, F_ref = 1 or F, 3 to N selected atoms of the receptor and of the ligand");
    return launch_docking(m, F, F_ref, N, xyz_ref, xyz, n_R, sel_R, n_L, sel_L, t_out, r_out, nullptr, 1.0, ptr_kind, stream, "rigid_docking");
}

int pesto_interface_rmsd(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_sel,
                         const int32_t* sel, double scale, float* rmsd_out, int32_t ptr_kind, void* stream) {
    if (!xyz_ref || !xyz || !sel || !rmsd_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKING_MAX_FRAMES || (F_ref != 1 && F_ref != F) || N < 1 || N > 0x7fffffff || n_sel < 3 || n_sel > N || !std::isfinite(scale))
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, F_ref = 1 or F, 3 to N selected atoms, a finite scale");
    return launch_docking(m, F, F_ref, N, xyz_ref, xyz, n_sel, sel, 0, nullptr, nullptr, nullptr, rmsd_out, scale, ptr_kind, stream, "interface_rmsd");
}
