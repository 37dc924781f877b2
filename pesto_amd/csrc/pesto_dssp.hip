// pesto_dssp.hip - DSSP secondary structure (Kabsch & Sander 1983, as the DSSP 2.x program applies it) of every frame / structure of a launch.
//
// replaces: md.compute_dssp(traj, simplified=False) as the reference calls it on one structure at a time in a 12-process pool
// (interfaceome/secondary_structures.py:27-31, wrapper_secondary_structure).
//
// Definition (the contract is the module docstring of pesto_amd/dssp.py; this is its summary). Coordinates are float32 times `scale`, in
// double; every sum is evaluated left to right as written, every operation rounded on its own (contraction is switched off for this
// whole file, see the pragma below: the build's -ffp-contract=on would fuse a * b + c inside one expression), sqrt and division IEEE.
// Residues are indexed within their structure; a residue without all four backbone atoms (NA) takes part in nothing.
//     cont(i)      i - 1 and i complete, same chain number, |C(i-1) - N(i)| <= 2.5;  nobreak(a, b) = cont(a+1) .. cont(b)
//     H(i)         N(i) + (C(i-1) - O(i-1)) / |C(i-1) - O(i-1)| if cont(i) and i is no proline, else N(i)
//     e(d, a)      for d != a, a != d - 1, both complete, d no proline, |CA(d) - CA(a)| < 9:
//                  e = -27.888/|H(d)O(a)| + 27.888/|H(d)C(a)| - 27.888/|N(d)C(a)| + 27.888/|N(d)O(a)|; e_m = -9900 if a distance is < 0.5,
//                  else round-half-away(1000 e) clamped below at -9900; kept if e_m < 0
//     best two     a donor's acceptors / an acceptor's donors: the two smallest (e_m, partner index)
//     bond(d, a)   a is one of d's two acceptors with e_m < -500
//     bridges, ladders, bulge links, E / B, H / G / I, T, S: as in the docstring (k_dssp_tail follows its order)
// A NaN makes every comparison it enters false.
//
// Launch sequence (all frames and all structures in each launch):
//     k_dssp_gather   a thread per (frame, residue): backbone and H in double, cont, the break counts to scan
//     k_dssp_pairs    donor side: a wave per (frame, donor); the acceptors' CA, C, O go through LDS in tiles of TILE residues, every lane
//                     keeps its two smallest packed keys (e_m + 9900) << 32 | partner, the wave merges them by shuffles: no atomics, no
//                     dependence on the order. Run again with the roles swapped for the acceptors' two best donors when they are asked for.
//                     The 9 A test is the exact one on every pair: nothing is pruned, so there is no margin to argue.
//     k_dssp_tail     a workgroup per (frame, structure): bridges from the partner table, ladders, links, sheet codes, helices, turns, bends
// Capacities. A bridge (i, j) needs bond(i+1, j), bond(i, j-1), bond(i+1, j-1) or bond(i, j), so j or j - 1 is one of the two acceptors of
// i or of i + 1: at most 8 distinct j per residue i. Bridges, and the ladders that start at them, are kept in 8 slots per residue, which
// therefore cannot overflow; a ladder that continues ladder A through a bulge starts 1 .. 5 residues behind A's last one, i.e. in at most
// 40 slots. Scratch per (frame, residue): 15 doubles, 11 ints per slot, the partner and energy rows and four bytes - SCRATCH_PER_RESIDUE
// bytes; an allocation that fails is reported (PESTO_ERR_NOMEM), nothing is truncated.
#include <climits>
#include <cmath>
#include <vector>

#include "pesto_call.h"
#include "pesto_scan.h"

#pragma clang fp contract(off)

namespace pesto {

namespace {

constexpr int NT = 256;             // threads per workgroup of every kernel here
constexpr int WAVES = NT / 64;      // pair pass: subjects (donors, or acceptors in the second run) per workgroup
constexpr int TILE = 128;           // pair pass: partner residues per LDS tile
constexpr int SLOTS = 8;            // bridges per residue i (the bound at the top of the file)
constexpr int FIELDS = 11;          // ints per slot
constexpr size_t SCRATCH_PER_RESIDUE = 15 * 8 + SLOTS * FIELDS * 4 + 2 * 16 + 4 + 4;
constexpr unsigned long long NO_KEY = ~0ull;
constexpr double Q = 27.888, COS70 = 0.3420201433256687;

enum { F_FULL = 1, F_CONT = 2, F_PRO = 4 };
enum { BR = 0, LN, LIE, LJLO, LJHI, LAB, CN, CIMIN, CIMAX, CJMIN, CJMAX };      // slot fields: bridge, its ladder, the ladder's component

__device__ __forceinline__ double dist3(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// ---- gather: bb[g] = N, CA, C, O, H (15 doubles); flags; brk[g - 1] = !cont(g) (shifted by one, so that the exclusive scan of a
// structure's brk gives the number of breaks up to and including each residue)
__global__ __launch_bounds__(NT) void k_dssp_gather(size_t total, int R_total, int n_struct, size_t n_atoms, const int* __restrict__ offsets,
                                                    const float* __restrict__ X, double scale, const int* __restrict__ table,
                                                    const unsigned char* __restrict__ proline, const int* __restrict__ chain,
                                                    double* __restrict__ bb, unsigned char* __restrict__ flags, int* __restrict__ brk) {
    const size_t g = (size_t)blockIdx.x * NT + threadIdx.x;
    if (g >= total) return;
    const size_t f = g / (size_t)R_total;
    const int r = (int)(g % (size_t)R_total);
    const int s = struct_of(r, n_struct, offsets);
    const int r0 = offsets[s], r1 = offsets[s + 1];
    const float* Xf = X + f * n_atoms * 3;
    const int* t = table + 4 * (size_t)r;
    const bool full = t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[3] >= 0;
    double p[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) p[k] = 0.0;
    int fl = (full ? F_FULL : 0) | (proline[r] ? F_PRO : 0);
    if (full) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[3 * k + c] = (double)Xf[3 * (size_t)t[k] + c] * scale;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[12 + c] = p[c];
        if (r > r0) {
            const int* u = t - 4;
            if (u[0] >= 0 && u[1] >= 0 && u[2] >= 0 && u[3] >= 0 && chain[r - 1] == chain[r]) {
                double C[3], O[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { C[c] = (double)Xf[3 * (size_t)u[2] + c] * scale; O[c] = (double)Xf[3 * (size_t)u[3] + c] * scale; }
                if (dist3(C, p) <= 2.5) {
                    fl |= F_CONT;
                    if (!proline[r]) {
                        const double len = dist3(C, O);
#pragma unroll
                        for (int c = 0; c < 3; ++c) p[12 + c] = p[c] + (C[c] - O[c]) / len;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 15; ++k) bb[g * 15 + k] = p[k];
    flags[g] = (unsigned char)fl;
    if (r > r0) brk[g - 1] = (fl & F_CONT) ? 0 : 1;
    if (r == r1 - 1) brk[g] = 0;
}

// e_m of donor (H, N) and acceptor (C, O), biased by 9900 (0 .. 9899), or -1 if nothing is kept
__device__ __forceinline__ int biased_energy(const double* H, const double* N, const double* C, const double* O) {
    const double ho = dist3(H, O), hc = dist3(H, C), nc = dist3(N, C), no = dist3(N, O);
    if (ho < 0.5 || hc < 0.5 || nc < 0.5 || no < 0.5) return 0;
    const double e = -Q / ho + Q / hc - Q / nc + Q / no;
    const double r = round(1000.0 * e);                     // half away from zero
    if (!(r < 0.0)) return -1;
    return (int)fmax(r, -9900.0) + 9900;
}

__device__ __forceinline__ void keep_two(unsigned long long& k1, unsigned long long& k2, unsigned long long o1, unsigned long long o2) {
    const unsigned long long lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, m2 = k2 < o2 ? k2 : o2;
    k1 = lo;
    k2 = hi < m2 ? hi : m2;
}

// A workgroup per (frame, structure, group of WAVES subjects), a wave per subject. DONOR: the subject is the donor and the partners are
// acceptors (tile records CA, C, O; columns 0, 1 of the tables); otherwise the subject is the acceptor (records N, CA, H; columns 2, 3).
template <bool DONOR>
__global__ __launch_bounds__(NT) void k_dssp_pairs(int n_blk, int R_total, int n_struct, const int* __restrict__ offsets, const int* __restrict__ blkoff,
                                                   const double* __restrict__ bb, const unsigned char* __restrict__ flags,
                                                   int* __restrict__ partners, int* __restrict__ energies) {
    __shared__ double tile[TILE][9];
    __shared__ unsigned char tile_ok[TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t f = blockIdx.x / (unsigned)n_blk;
    const int b = (int)(blockIdx.x % (unsigned)n_blk);
    const int s = struct_of(b, n_struct, blkoff);
    const int r0 = offsets[s], Rs = offsets[s + 1] - r0;
    const size_t gb = f * (size_t)R_total + r0;             // the structure's first residue in this frame
    const int l = (b - blkoff[s]) * WAVES + wave;           // the wave's subject (local index); waves behind the end only help loading
    const bool valid = l < Rs;
    double me[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) me[k] = 0.0;
    bool active = false;
    if (valid) {
        const int fl = flags[gb + l];
        active = DONOR ? (fl & F_FULL) && !(fl & F_PRO) : (fl & F_FULL) != 0;
        const double* p = bb + (gb + l) * 15;
#pragma unroll
        for (int k = 0; k < 9; ++k) me[k] = DONOR ? (k < 6 ? p[k] : p[6 + k]) : p[3 + k];       // donor: N, CA, H; acceptor: CA, C, O
    }
    unsigned long long k1 = NO_KEY, k2 = NO_KEY;
    for (int t0 = 0; t0 < Rs; t0 += TILE) {
        const int cnt = min(TILE, Rs - t0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < cnt * 9; idx += NT) {
            const int rec = idx / 9, k = idx - rec * 9;
            const double* p = bb + (gb + t0 + rec) * 15;
            tile[rec][k] = DONOR ? p[3 + k] : (k < 6 ? p[k] : p[6 + k]);
        }
        for (int rec = threadIdx.x; rec < cnt; rec += NT) {
            const int fl = flags[gb + t0 + rec];
            tile_ok[rec] = DONOR ? (fl & F_FULL) != 0 : (fl & F_FULL) && !(fl & F_PRO);
        }
        __syncthreads();
        if (active) {
            for (int j = lane; j < cnt; j += 64) {
                const int o = t0 + j;
                const int d = DONOR ? l : o, a = DONOR ? o : l;
                if (!tile_ok[j] || a == d || a == d - 1) continue;
                const double* q = tile[j];
                int eb;
                if (DONOR) {
                    if (!(dist3(me + 3, q) < 9.0)) continue;
                    eb = biased_energy(me + 6, me, q + 3, q + 6);
                } else {
                    if (!(dist3(q + 3, me) < 9.0)) continue;
                    eb = biased_energy(q + 6, q, me + 3, me + 6);
                }
                if (eb < 0) continue;
                keep_two(k1, k2, ((unsigned long long)(unsigned)eb << 32) | (unsigned)o, NO_KEY);
            }
        }
    }
    if (!valid) return;                                      // (behind the last barrier)
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o1 = __shfl_xor(k1, off), o2 = __shfl_xor(k2, off);
        keep_two(k1, k2, o1, o2);
    }
    if (lane == 0) {
        const size_t at = (gb + l) * 4 + (DONOR ? 0 : 2);
        partners[at] = k1 == NO_KEY ? -1 : (int)(unsigned)(k1 & 0xffffffffull);
        partners[at + 1] = k2 == NO_KEY ? -1 : (int)(unsigned)(k2 & 0xffffffffull);
        energies[at] = k1 == NO_KEY ? 0 : (int)(k1 >> 32) - 9900;
        energies[at + 1] = k2 == NO_KEY ? 0 : (int)(k2 >> 32) - 9900;
    }
}

// the view one workgroup has of its (frame, structure): local residue indices 0 .. Rs - 1
struct Tail {
    int Rs;
    const int* brk;                 // breaks up to and including residue i
    const int* partners;
    const int* energies;
    __device__ __forceinline__ bool nobreak(int a, int b) const { return a >= 0 && a <= b && b < Rs && brk[a] == brk[b]; }
    __device__ __forceinline__ bool bond(int d, int a) const {
        if (d < 0 || d >= Rs || a < 0 || a >= Rs) return false;
        return (partners[4 * d] == a && energies[4 * d] < -500) || (partners[4 * d + 1] == a && energies[4 * d + 1] < -500);
    }
    // 0 none, 1 parallel, 2 antiparallel; the caller has checked i >= 1, j >= i + 3, j + 1 < Rs and both nobreak conditions
    __device__ __forceinline__ int bridge(int i, int j) const {
        if ((bond(i + 1, j) && bond(j, i - 1)) || (bond(j + 1, i) && bond(i, j - 1))) return 1;
        if ((bond(i + 1, j - 1) && bond(j + 1, i - 1)) || (bond(j, i) && bond(i, j))) return 2;
        return 0;
    }
};

__device__ __forceinline__ int find_slot(const int* __restrict__ slot, int i, int packed) {
    for (int k = 0; k < SLOTS; ++k)
        if (slot[((size_t)i * SLOTS + k) * FIELDS + BR] == packed) return k;
    return -1;
}

// One workgroup per (frame, structure); the phases are separated by workgroup barriers, every array is this structure's own.
__global__ __launch_bounds__(NT) void k_dssp_tail(int R_total, int n_struct, const int* __restrict__ offsets, const double* __restrict__ bb_all,
                                                  const unsigned char* __restrict__ flags_all, int* __restrict__ brk_all,
                                                  const int* __restrict__ partners_all, const int* __restrict__ energies_all,
                                                  int* __restrict__ slot_all, unsigned char* __restrict__ st_all, unsigned char* __restrict__ cond_all,
                                                  unsigned char* __restrict__ code_all) {
    const size_t f = blockIdx.x / (unsigned)n_struct;
    const int s = (int)(blockIdx.x % (unsigned)n_struct);
    const int r0 = offsets[s], Rs = offsets[s + 1] - r0;
    const size_t gb = f * (size_t)R_total + r0;
    const double* bb = bb_all + gb * 15;
    const unsigned char* flags = flags_all + gb;
    int* brk = brk_all + gb;
    int* slot = slot_all + gb * SLOTS * FIELDS;
    unsigned char* st = st_all + gb;
    unsigned char* cond = cond_all + gb;
    unsigned char* code = code_all + gb;
    const int tid = threadIdx.x;

    block_scan_exclusive<NT, false>(brk, Rs);
    __syncthreads();
    Tail T{Rs, brk, partners_all + gb * 4, energies_all + gb * 4};

    // A. bridges of residue i into its slots; codes cleared
    for (int i = tid; i < Rs; i += NT) {
        code[i] = PESTO_DSSP_BLANK;
        int found[SLOTS], seen[SLOTS], n_seen = 0, n_found = 0;
        if (i >= 1 && T.nobreak(i - 1, i + 1)) {
            for (int c = 0; c < 8; ++c) {
                const int d = i + (c >> 2);                  // acceptors of i + 1 and of i; j = a and j = a + 1
                if (d >= Rs) continue;
                const int a = T.partners[4 * d + ((c >> 1) & 1)];
                if (a < 0) continue;
                const int j = a + (c & 1);
                if (j < i + 3 || j + 1 >= Rs || !T.nobreak(j - 1, j + 1)) continue;
                bool dup = false;
                for (int k = 0; k < n_seen; ++k) dup = dup || seen[k] == j;
                if (dup) continue;
                seen[n_seen++] = j;                          // (at most 8 candidates, so n_seen <= SLOTS)
                const int t = T.bridge(i, j);
                if (t) found[n_found++] = j * 4 + t;
            }
        }
        for (int k = 0; k < SLOTS; ++k) {
            int* q = slot + ((size_t)i * SLOTS + k) * FIELDS;
            q[BR] = k < n_found ? found[k] : -1;
            q[LN] = 0; q[LAB] = i * SLOTS + k; q[CN] = 0; q[CIMIN] = INT_MAX; q[CIMAX] = -1; q[CJMIN] = INT_MAX; q[CJMAX] = -1;
        }
    }
    __syncthreads();
    // B. ladders: a bridge without a predecessor of its type starts one and walks it
    for (int e = tid; e < Rs * SLOTS; e += NT) {
        int* q = slot + (size_t)e * FIELDS;
        if (q[BR] < 0) continue;
        const int i = e / SLOTS, j = q[BR] >> 2, t = q[BR] & 3, step = t == 1 ? 1 : -1;
        if (i >= 1 && find_slot(slot, i - 1, (j - step) * 4 + t) >= 0) continue;
        int n = 1;
        while (i + n < Rs && j + step * n >= 0 && find_slot(slot, i + n, (j + step * n) * 4 + t) >= 0) ++n;
        const int j2 = j + step * (n - 1);
        q[LN] = n; q[LIE] = i + n - 1; q[LJLO] = min(j, j2); q[LJHI] = max(j, j2);
    }
    __syncthreads();
    // C. bulge links, transitive: the smallest slot number of a component spreads over it until nothing changes
    volatile int* vs = slot;
    for (;;) {
        int changed = 0;
        for (int e = tid; e < Rs * SLOTS; e += NT) {
            const int* A = slot + (size_t)e * FIELDS;
            if (A[LN] <= 0) continue;
            const int t = A[BR] & 3;
            for (int ib = A[LIE] + 1; ib <= A[LIE] + 5 && ib < Rs; ++ib)
                for (int k = 0; k < SLOTS; ++k) {
                    const int e2 = ib * SLOTS + k;
                    const int* B = slot + (size_t)e2 * FIELDS;
                    if (B[LN] <= 0 || (B[BR] & 3) != t) continue;
                    const int gi = ib - A[LIE] - 1;
                    const int gj = t == 1 ? B[LJLO] - A[LJHI] - 1 : A[LJLO] - B[LJHI] - 1;
                    if (gj < 0 || !((gi <= 1 && gj <= 4) || (gj <= 1 && gi <= 4))) continue;
                    if (!T.nobreak(A[LIE], ib) || !(t == 1 ? T.nobreak(A[LJHI], B[LJLO]) : T.nobreak(B[LJHI], A[LJLO]))) continue;
                    const int la = vs[(size_t)e * FIELDS + LAB], lb = vs[(size_t)e2 * FIELDS + LAB];
                    if (la != lb) {
                        const int m = min(la, lb);
                        atomicMin(slot + (size_t)e * FIELDS + LAB, m);
                        atomicMin(slot + (size_t)e2 * FIELDS + LAB, m);
                        changed = 1;
                    }
                }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // D. components: bridges and the extent of both strands, at the slot that names the component
    for (int e = tid; e < Rs * SLOTS; e += NT) {
        const int* A = slot + (size_t)e * FIELDS;
        if (A[LN] <= 0) continue;
        int* C = slot + (size_t)A[LAB] * FIELDS;
        atomicAdd(C + CN, A[LN]);
        atomicMin(C + CIMIN, e / SLOTS); atomicMax(C + CIMAX, A[LIE]);
        atomicMin(C + CJMIN, A[LJLO]); atomicMax(C + CJMAX, A[LJHI]);
    }
    __syncthreads();
    // E. sheet codes: B for a component of one bridge, then E (never overwritten by B) over both strands, gaps included
    for (int pass = 0; pass < 2; ++pass) {
        for (int e = tid; e < Rs * SLOTS; e += NT) {
            const int* C = slot + (size_t)e * FIELDS;
            if (C[CN] <= 0 || (C[CN] > 1) != (pass == 1)) continue;
            const unsigned char c = pass ? PESTO_DSSP_E : PESTO_DSSP_B;
            for (int r = C[CIMIN]; r <= C[CIMAX]; ++r) code[r] = c;
            for (int r = C[CJMIN]; r <= C[CJMAX]; ++r) code[r] = c;
        }
        __syncthreads();
    }
    // F. turn starts: bit n - 3 for start_n(i)
    for (int i = tid; i < Rs; i += NT) {
        int v = 0;
        for (int n = 3; n <= 5; ++n)
            if (T.nobreak(i, i + n) && T.bond(i + n, i)) v |= 1 << (n - 3);
        st[i] = (unsigned char)v;
    }
    __syncthreads();
    auto two = [&](int i, int bit) { return i >= 1 && i < Rs && (st[i - 1] >> bit & 1) && (st[i] >> bit & 1); };
    // G. H overrides E / B
    for (int r = tid; r < Rs; r += NT) {
        bool h = false;
        for (int i = r - 3; i <= r; ++i) h = h || two(i, 1);
        if (h) code[r] = PESTO_DSSP_H;
    }
    __syncthreads();
    // H. G, then I: where the minimal helix lies on blank residues (its own letter never blocks it, so the order of i does not matter)
    for (int n = 3; n <= 5; n += 2) {
        for (int i = tid; i < Rs; i += NT) {
            bool ok = two(i, n - 3);
            for (int r = i; ok && r < i + n; ++r) ok = r < Rs && code[r] == PESTO_DSSP_BLANK;
            cond[i] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int r = tid; r < Rs; r += NT) {
            bool hit = false;
            for (int i = max(0, r - n + 1); i <= r; ++i) hit = hit || cond[i];
            if (hit) code[r] = n == 3 ? PESTO_DSSP_G : PESTO_DSSP_I;
        }
        __syncthreads();
    }
    // I. turns and bends on what is still blank; NA last
    for (int r = tid; r < Rs; r += NT) {
        if (!(flags[r] & F_FULL)) { code[r] = PESTO_DSSP_NA; continue; }
        if (code[r] != PESTO_DSSP_BLANK || r < 1 || r > Rs - 2) continue;
        bool turn = false;
        for (int n = 3; n <= 5; ++n)
            for (int k = 1; k < n; ++k) turn = turn || (r - k >= 0 && (st[r - k] >> (n - 3) & 1));
        if (turn) { code[r] = PESTO_DSSP_T; continue; }
        if (!T.nobreak(r - 2, r + 2)) continue;
        const double* a = bb + (size_t)(r - 2) * 15 + 3;
        const double* b = bb + (size_t)r * 15 + 3;
        const double* c = bb + (size_t)(r + 2) * 15 + 3;
        const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - b[0], vy = c[1] - b[1], vz = c[2] - b[2];
        const double uv = ux * vx + uy * vy + uz * vz, uu = ux * ux + uy * uy + uz * uz, vv = vx * vx + vy * vy + vz * vz;
        if (uv / sqrt(uu * vv) < COS70) code[r] = PESTO_DSSP_S;
    }
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_dssp_last_error(void) { return last_error(); }

int pesto_dssp(pesto_model* m, int64_t F, int64_t n_atoms, const float* X, double scale, int64_t R_total, int32_t n_struct,
               const int32_t* res_offsets, const int32_t* bb_atoms, const uint8_t* proline, const int32_t* chain, uint8_t* codes_out,
               int32_t* partners_out, int32_t* energies_out, int32_t ptr_kind, void* stream) {
    if (!X || !res_offsets || !bb_atoms || !proline || !chain) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (!codes_out && !partners_out && !energies_out) return fail(PESTO_ERR_INVALID, "no output requested");
    if (F < 1 || n_atoms < 1 || F > 0x7fffffff || n_atoms > 0x7fffffff || F * n_atoms > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "F * n_atoms must be in 1 .. 2^31 - 1 (F = %lld, n_atoms = %lld)", (long long)F, (long long)n_atoms);
    if (R_total < 1 || R_total > 0x7fffffff || F * R_total > 0x7fffffff)
        return fail(PESTO_ERR_INVALID, "F * R_total must be in 1 .. 2^31 - 1 (F = %lld, R_total = %lld)", (long long)F, (long long)R_total);
    if (n_struct < 1 || n_struct > R_total) return fail(PESTO_ERR_INVALID, "1 <= n_struct <= R_total structures, got %d", n_struct);
    if (int rc = check_offsets(res_offsets, n_struct, R_total, "res_offsets")) return rc;
    if (F * (int64_t)n_struct > 0x7fffffff) return fail(PESTO_ERR_INVALID, "F * n_struct must stay below 2^31");
    if (!std::isfinite(scale)) return fail(PESTO_ERR_INVALID, "scale must be finite");
    std::vector<int32_t> blkoff((size_t)n_struct + 1, 0);
    for (int s = 0; s < n_struct; ++s) {
        const int32_t n = res_offsets[s + 1] - res_offsets[s];
        if (n > PESTO_DSSP_MAX_RESIDUES)
            return fail(PESTO_ERR_INVALID, "structure %d has %d residues, at most %d", s, n, (int)PESTO_DSSP_MAX_RESIDUES);
        blkoff[s + 1] = blkoff[s] + (n + WAVES - 1) / WAVES;
    }
    for (int64_t k = 0; k < 4 * R_total; ++k)
        if (bb_atoms[k] < -1 || bb_atoms[k] >= n_atoms)
            return fail(PESTO_ERR_INVALID, "bb_atoms: residue %lld names atom row %d, outside -1 .. %lld", (long long)(k / 4), bb_atoms[k],
                        (long long)n_atoms - 1);
    const int n_blk = blkoff[n_struct];
    if (F * (int64_t)n_blk > 0x7fffffff) return fail(PESTO_ERR_INVALID, "F * R_total is too large for one launch");
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t total = (size_t)F * R_total;
    Buffers bf(ptr_kind, stream);
    const int iX = bf.input(X, (size_t)F * n_atoms * 12);
    const int iO = bf.table(res_offsets, ((size_t)n_struct + 1) * 4), iB = bf.table(blkoff.data(), blkoff.size() * 4);
    const int iT = bf.table(bb_atoms, (size_t)R_total * 16), iPr = bf.table(proline, (size_t)R_total), iCh = bf.table(chain, (size_t)R_total * 4);
    const int iC = codes_out ? bf.output(codes_out, total) : bf.scratch(total);
    const int iP = partners_out ? bf.output(partners_out, total * 16) : bf.scratch(total * 16);
    const int iE = energies_out ? bf.output(energies_out, total * 16) : bf.scratch(total * 16);
    const int iBB = bf.scratch(total * 15 * 8), iFl = bf.scratch(total), iBrk = bf.scratch(total * 4);
    const int iSl = bf.scratch(codes_out ? total * SLOTS * FIELDS * 4 : 0), iSt = bf.scratch(total), iCo = bf.scratch(total);
    static_assert(SCRATCH_PER_RESIDUE == 15 * 8 + SLOTS * FIELDS * 4 + 32 + 8, "the bound stated at the top of the file");
    int rc = bf.upload();
    if (rc == 0) {
        const int* off = bf.ptr<const int>(iO);
        const int* blk = bf.ptr<const int>(iB);
        hipLaunchKernelGGL(k_dssp_gather, dim3(blocks(total, NT)), dim3(NT), 0, bf.stm, total, (int)R_total, n_struct, (size_t)n_atoms, off,
                           bf.ptr<const float>(iX), scale, bf.ptr<const int>(iT), bf.ptr<const unsigned char>(iPr), bf.ptr<const int>(iCh),
                           bf.ptr<double>(iBB), bf.ptr<unsigned char>(iFl), bf.ptr<int>(iBrk));
        const dim3 pg((unsigned)((size_t)F * n_blk));
        hipLaunchKernelGGL(k_dssp_pairs<true>, pg, dim3(NT), 0, bf.stm, n_blk, (int)R_total, n_struct, off, blk, bf.ptr<const double>(iBB),
                           bf.ptr<const unsigned char>(iFl), bf.ptr<int>(iP), bf.ptr<int>(iE));
        if (partners_out || energies_out)
            hipLaunchKernelGGL(k_dssp_pairs<false>, pg, dim3(NT), 0, bf.stm, n_blk, (int)R_total, n_struct, off, blk, bf.ptr<const double>(iBB),
                               bf.ptr<const unsigned char>(iFl), bf.ptr<int>(iP), bf.ptr<int>(iE));
        if (codes_out)
            hipLaunchKernelGGL(k_dssp_tail, dim3((unsigned)((size_t)F * n_struct)), dim3(NT), 0, bf.stm, (int)R_total, n_struct, off,
                               bf.ptr<const double>(iBB), bf.ptr<const unsigned char>(iFl), bf.ptr<int>(iBrk), bf.ptr<const int>(iP),
                               bf.ptr<const int>(iE), bf.ptr<int>(iSl), bf.ptr<unsigned char>(iSt), bf.ptr<unsigned char>(iCo),
                               bf.ptr<unsigned char>(iC));
    }
    return bf.finish(rc, "dssp");
}
