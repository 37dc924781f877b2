// pesto_dockq.hip - how well a docking decoy reproduces the bound complex: the three CAPRI measures (fraction of native contacts, interface
// RMSD, ligand RMSD), the DockQ score (Basu and Wallner 2016) and the CAPRI class of every decoy in one launch, and the RMSD of one atom
// selection after a fit on another (pesto_fit_rmsd).
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h, with a message channel of their own.
//
// fnat needs only the residue pairs in contact in the native (a few hundred; the caller lists them once per call): a pair is preserved
// in a decoy when some atom pair of its two residues has s < s_star, s the float32 squared distance of pesto_geom.h and s_star the
// smallest float at which fl32(sqrt_rn(s)) * scale < r_contact fails (contact_threshold), so the decision is the docking group's d < r_thr
// exactly. The atoms come sorted by residue (a permutation; every pair holds two ranges of it), one wave owns a pair, its 64 lanes walk
// the na * nb atom pairs 64 at a time and stop at the first step with a hit; the count is an integer sum. The two RMSDs are the fit, the
// moved point and the deviation sum of pesto_fit.h, which pesto_docking.hip and pesto_trajectory.hip call too, so the interface RMSD
// has the bits of pesto_interface_rmsd. No floating-point atomics: every output repeats its bits from call to call.
#include <cmath>

#include "pesto_call.h"
#include "pesto_fit.h"

namespace pesto {

namespace {

constexpr int NT = 256;                 // threads per workgroup of every kernel here
constexpr int NW = NT / 64;             // its waves

// ------------------------------------------------------------------------------------------------ the index check
// Every index is validated before anything dereferences it: the three selections and the permutation (idx) must lie in [0, N) (error
// bit 0: check_index of pesto_fit.h); behind them, a pair's two ranges must be non-empty ranges of the permutation with fewer than 2^31
// atom pairs between them (error bit 1). The kernels below return at once when a bit is set, so a refused call writes nothing.
__global__ __launch_bounds__(NT) void k_dq_check(int N, IndexLists idx, long long n_perm, long long P, const int* __restrict__ pairs,
                                                 int* __restrict__ err) {
    long long k = (long long)blockIdx.x * NT + threadIdx.x;
    if (!check_index(k, N, idx, err) && k < P) {
        const int* q = pairs + 4 * k;
        const long long a0 = q[0], a1 = q[1], b0 = q[2], b1 = q[3];
        const bool ok = 0 <= a0 && a0 < a1 && a1 <= n_perm && 0 <= b0 && b0 < b1 && b1 <= n_perm && (a1 - a0) * (b1 - b0) <= 0x7fffffffLL;
        if (!ok) atomicOr(err, 2);
    }
}

// ------------------------------------------------------------------------------------------------ fnat
// the number of pairs with an atom pair s < s_star in frame X (the same value in every thread). pairs int32 [P, 4]: the ranges
// [a0, a1) and [b0, b1) of perm that hold the atoms of the pair's receptor and ligand residue. Wave w owns the pairs w, w + NW, ...;
// lane l of step t tests atom pair 64 t + l of the na * nb (row-major: a receptor atom against consecutive ligand atoms), and the wave
// leaves the pair at the first step in which a lane hits. A NaN distance is no hit. ired: NW ints of LDS; two barriers.
__device__ __forceinline__ int preserved_pairs(const float* __restrict__ X, const int* __restrict__ perm, const int* __restrict__ pairs, int P,
                                               float s_star, int* ired) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int count = 0;
    for (int k = wave; k < P; k += NW) {
        const int a0 = pairs[4 * (size_t)k], b0 = pairs[4 * (size_t)k + 2];
        const unsigned na = (unsigned)(pairs[4 * (size_t)k + 1] - a0), nb = (unsigned)(pairs[4 * (size_t)k + 3] - b0);
        const unsigned total = na * nb;                 // < 2^31: k_dq_check
        bool found = false;
        for (unsigned first = 0; first < total && !found; first += 64) {
            const unsigned idx = first + (unsigned)lane;
            bool hit = false;
            if (idx < total) {
                const unsigned i = idx / nb, j = idx - i * nb;
                const float* a = X + (size_t)perm[a0 + (int)i] * 3;
                const float* b = X + (size_t)perm[b0 + (int)j] * 3;
                hit = dist2(a[0], a[1], a[2], b[0], b[1], b[2]) < s_star;       // (NaN: false)
            }
            found = __ballot(hit) != 0ull;
        }
        count += found ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) ired[wave] = count;
    __syncthreads();
    int t = ired[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += ired[w];
    return t;
}

// ------------------------------------------------------------------------------------------------ the score and the class
// (fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3 in double from the three float32 values, every operation rounded
// as written (no contraction), rounded once to float32
__device__ __forceinline__ float dockq_score(float fnat, float irmsd, float lrmsd) {
    const double a = __ddiv_rn((double)irmsd, 1.5), b = __ddiv_rn((double)lrmsd, 8.5);
    const double ti = __ddiv_rn(1.0, __dadd_rn(1.0, __dmul_rn(a, a)));
    const double tl = __ddiv_rn(1.0, __dadd_rn(1.0, __dmul_rn(b, b)));
    return (float)__ddiv_rn(__dadd_rn(__dadd_rn((double)fnat, ti), tl), 3.0);
}

// the highest CAPRI class whose condition holds; the fnat conditions (>= 0.5, 0.3, 0.1) on the integers, a NaN RMSD passes none
__device__ __forceinline__ unsigned char capri_of(long long kept, long long P, float irmsd, float lrmsd) {
    if (2 * kept >= P && (lrmsd <= 1.0f || irmsd <= 1.0f)) return 3;
    if (10 * kept >= 3 * P && (lrmsd <= 5.0f || irmsd <= 2.0f)) return 2;
    if (10 * kept >= P && (lrmsd <= 10.0f || irmsd <= 4.0f)) return 1;
    return 0;
}

// ------------------------------------------------------------------------------------------------ the kernels
// replaces, per decoy: residue_contact_maps over the full sides and native_contacts (fnat), pesto_interface_rmsd (irmsd), and what the
// package lacked (lrmsd, DockQ, the class). One workgroup per decoy, three phases: the preserved native pairs; the interface fit and its
// RMSD; the receptor fit and the ligand's deviation under it. Thread 0 writes the frame's outputs.
__global__ __launch_bounds__(NT) void k_dockq(int N, int P, int nI, int nR, int nL, const float* __restrict__ ref, const float* __restrict__ xyz,
                                              const int* __restrict__ perm, const int* __restrict__ pairs, const int* __restrict__ sel_I,
                                              const int* __restrict__ sel_R, const int* __restrict__ sel_L, const int* __restrict__ err, float s_star,
                                              double scale, float* __restrict__ fnat_out, int* __restrict__ preserved_out, float* __restrict__ irmsd_out,
                                              float* __restrict__ lrmsd_out, float* __restrict__ dockq_out, unsigned char* __restrict__ capri_out) {
    __shared__ double red[NW];
    __shared__ double sR[9];
    __shared__ int ired[NW];
    if (*err) return;
    const size_t f = blockIdx.x;
    const float* X = xyz + f * (size_t)N * 3;
    const int kept = preserved_pairs(X, perm, pairs, P, s_star, ired);
    Fit ft;
    kabsch_fit<NT, true>(atoms(X, sel_I), atoms(ref, sel_I), nI, red, sR, ft);
    const double dev_I = moved_deviation<NT>(atoms(X, sel_I), atoms(ref, sel_I), nI, ft, red);
    kabsch_fit<NT, true>(atoms(X, sel_R), atoms(ref, sel_R), nR, red, sR, ft);
    const double dev_L = moved_deviation<NT>(atoms(X, sel_L), atoms(ref, sel_L), nL, ft, red);
    if (threadIdx.x == 0) {
        const float fn = (float)((double)kept / (double)P);
        const float ir = (float)(sqrt(dev_I / (double)nI) * scale);
        const float lr = (float)(sqrt(dev_L / (double)nL) * scale);
        fnat_out[f] = fn;
        preserved_out[f] = kept;
        irmsd_out[f] = ir;
        lrmsd_out[f] = lr;
        dockq_out[f] = dockq_score(fn, ir, lr);
        capri_out[f] = capri_of(kept, P, ir, lr);
    }
}

// (k_fit_rmsd, the RMSD of sel_M after the fit on sel_F - the ligand RMSD alone, and the general "different atoms for fit and measure":
// pesto_fit.h)

// ---- host side
// the error of a refused call from the check kernel's bits (0: none)
int index_error(int err, const char* what) {
    if (err & 1) return fail(PESTO_ERR_INVALID, "%s: atom indices of a selection or of the permutation must lie in [0, N)", what);
    if (err & 2) return fail(PESTO_ERR_INVALID, "%s: a pair needs two non-empty ranges of the permutation with fewer than 2^31 atom pairs", what);
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_dockq_last_error(void) { return last_error(); }

int pesto_dockq(pesto_model* m, int64_t F, int64_t N, const float* xyz_ref, const float* xyz, int64_t P, const int32_t* pairs, int64_t n_perm,
                const int32_t* perm, int64_t n_I, const int32_t* sel_I, int64_t n_R, const int32_t* sel_R, int64_t n_L, const int32_t* sel_L,
                float r_contact, double scale, float* fnat_out, int32_t* preserved_out, float* irmsd_out, float* lrmsd_out, float* dockq_out,
                uint8_t* capri_out, int32_t ptr_kind, void* stream) {
    if (!xyz_ref || !xyz || !pairs || !perm || !sel_I || !sel_R || !sel_L || !fnat_out || !preserved_out || !irmsd_out || !lrmsd_out || !dockq_out ||
        !capri_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKQ_MAX_FRAMES || N < 1 || N > 0x3fffffff) return fail(PESTO_ERR_INVALID, "1 to 2^23 frames and 1 <= N < 2^30 atoms");
    if (P < 1 || P > PESTO_DOCKQ_MAX_PAIRS) return fail(PESTO_ERR_INVALID, "1 to 2^24 native pairs, got %lld", (long long)P);
    if (n_perm < 2 || n_perm > 2 * N || n_I < 3 || n_I > N || n_R < 3 || n_R > N || n_L < 1 || n_L > N)
        return fail(PESTO_ERR_INVALID, "2 to 2 N permuted atoms, 3 to N atoms of the interface and of the receptor, 1 to N of the ligand");
    const float fscale = (float)scale;
    if (!std::isfinite(r_contact) || !std::isfinite(scale) || !std::isfinite(fscale) || !(fscale > 0.f))
        return fail(PESTO_ERR_INVALID, "r_contact must be finite and scale positive and finite");
    if (int rc = begin(m, ptr_kind)) return rc;
    const float s_star = contact_threshold(r_contact, fscale, true);
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)N * 12), iX = bf.input(xyz, (size_t)F * N * 12), iPr = bf.input(pairs, (size_t)P * 16),
              iPm = bf.input(perm, (size_t)n_perm * 4), iSi = bf.input(sel_I, (size_t)n_I * 4), iSr = bf.input(sel_R, (size_t)n_R * 4),
              iSl = bf.input(sel_L, (size_t)n_L * 4);
    const int iFn = bf.output(fnat_out, (size_t)F * 4), iKp = bf.output(preserved_out, (size_t)F * 4), iIr = bf.output(irmsd_out, (size_t)F * 4),
              iLr = bf.output(lrmsd_out, (size_t)F * 4), iDq = bf.output(dockq_out, (size_t)F * 4), iCp = bf.output(capri_out, (size_t)F);
    const int iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const IndexLists idx = {{bf.ptr<const int>(iSi), bf.ptr<const int>(iSr), bf.ptr<const int>(iSl), bf.ptr<const int>(iPm)}, {n_I, n_R, n_L, n_perm}};
        hipLaunchKernelGGL(k_dq_check, dim3(blocks((size_t)(idx.total() + P), NT)), dim3(NT), 0, bf.stm, (int)N, idx, (long long)n_perm, (long long)P,
                           bf.ptr<const int>(iPr), bf.ptr<int>(iSt));
        hipLaunchKernelGGL(k_dockq, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)N, (int)P, (int)n_I, (int)n_R, (int)n_L, bf.ptr<const float>(iY),
                           bf.ptr<const float>(iX), bf.ptr<const int>(iPm), bf.ptr<const int>(iPr), bf.ptr<const int>(iSi), bf.ptr<const int>(iSr),
                           bf.ptr<const int>(iSl), bf.ptr<const int>(iSt), s_star, scale, bf.ptr<float>(iFn), bf.ptr<int>(iKp), bf.ptr<float>(iIr),
                           bf.ptr<float>(iLr), bf.ptr<float>(iDq), bf.ptr<unsigned char>(iCp));
    }
    // a refused call writes nothing: the check's verdict is read before any output is copied back
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "dockq");
    if (rc == 0) rc = index_error(herr, "dockq");
    return bf.finish(rc, "dockq");
}

int pesto_fit_rmsd(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_fit, const int32_t* sel_fit,
                   int64_t n_measure, const int32_t* sel_measure, double scale, float* rmsd_out, int32_t ptr_kind, void* stream) {
    if (!xyz_ref || !xyz || !sel_fit || !sel_measure || !rmsd_out) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (F < 1 || F > PESTO_DOCKQ_MAX_FRAMES || (F_ref != 1 && F_ref != F) || N < 1 || N > 0x3fffffff || n_fit < 3 || n_fit > N || n_measure < 1 ||
        n_measure > N || !std::isfinite(scale))
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames, F_ref = 1 or F, 1 <= N < 2^30, 3 to N atoms to fit, 1 to N to measure, a finite scale");
    if (int rc = begin(m, ptr_kind)) return rc;
    Buffers bf(ptr_kind, stream);
    const int iY = bf.input(xyz_ref, (size_t)F_ref * N * 12), iX = bf.input(xyz, (size_t)F * N * 12), iSf = bf.input(sel_fit, (size_t)n_fit * 4),
              iSm = bf.input(sel_measure, (size_t)n_measure * 4), iO = bf.output(rmsd_out, (size_t)F * 4), iSt = bf.scratch(sizeof(int), 0);
    int herr = 0;
    int rc = bf.upload();
    if (rc == 0) {
        const IndexLists idx = {{bf.ptr<const int>(iSf), bf.ptr<const int>(iSm)}, {n_fit, n_measure}};
        hipLaunchKernelGGL(k_index_check<NT>, dim3(blocks((size_t)idx.total(), NT)), dim3(NT), 0, bf.stm, (int)N, idx, bf.ptr<int>(iSt));
        hipLaunchKernelGGL(k_fit_rmsd<NT>, dim3((unsigned)F), dim3(NT), 0, bf.stm, (int)F_ref, (int)N, (int)n_fit, (int)n_measure, bf.ptr<const float>(iY),
                           bf.ptr<const float>(iX), bf.ptr<const int>(iSf), bf.ptr<const int>(iSm), bf.ptr<const int>(iSt), scale, bf.ptr<float>(iO));
    }
    if (rc == 0) rc = bf.verdict(iSt, &herr, sizeof herr, "fit_rmsd");
    if (rc == 0) rc = index_error(herr, "fit_rmsd");
    return bf.finish(rc, "fit_rmsd");
}
