// pesto_mma64.h - the one 64 x 64 double-precision tile of the analysis groups on v_mfma_f64_16x16x4_f64 (k_prmsd_cov of
// pesto_cluster.hip, k_dyn_mma<MODE> of pesto_dynamics.hip): C[row][col] = sum_k A[k][row] B[k][col] by a workgroup of 256 threads, both
// operands staged k-major through LDS KC deep, the next stage already in registers while this one is multiplied. Wave w owns the rows
// 16 w .. 16 w + 15 against all 64 columns (four 16 x 16 accumulators). A kernel brings its operands as a load and a store callable
// (like the point sources of kabsch_fit, pesto_fit.h) and decides what becomes of the tile.
//
// Everything sits in an anonymous namespace (one copy per translation unit, like pesto_geom.h).
#pragma once
#include <hip/hip_runtime.h>

namespace pesto {
namespace {

constexpr int MT = 64;              // rows and columns of the tile
constexpr int KC = 16;              // K per LDS stage
constexpr int LS = 80;              // doubles between two k of a staged operand: 2.5 turns of the 64 banks of 4 bytes, so the 4 k that the
                                    // lanes of one MFMA step read (k = lane >> 4) fall on both halves of the banks
constexpr int HS = MT + 1;          // doubles between two rows of a 64 x 64 image in LDS
constexpr int MMA64_LDS = MT * HS;  // doubles of LDS: the two staged operands, then, where a kernel wants it, the accumulator image
static_assert(2 * KC * LS <= MMA64_LDS, "the staged operands must fit the accumulator image");

using f64x4 = __attribute__((ext_vector_type(4))) double;

// the thread's four values of a stage (k = tid / 16, rows 4 (tid % 16) ..); R: four floats or doubles, converted here
template <class R>
__device__ __forceinline__ void store_kmajor(double* S, const R& r) {
    double* d = S + (threadIdx.x >> 4) * LS + 4 * (threadIdx.x & 15);
    d[0] = (double)r[0]; d[1] = (double)r[1]; d[2] = (double)r[2]; d[3] = (double)r[3];
}

// out = the tile over k in [kbeg, kend). load(k0, ra, rb): the thread's part of both operands of the stage at k0 into registers (R; zeros
// from the operands' end on); store(As, ra): A's into LDS (B's are k-major in every kernel). A stage is up to KC / 4 MFMA steps of 4 k.
// TAIL: kend - kbeg is a multiple of 4 and the last stage runs only its steps below kend; else every stage runs all of them, the same
// bits: the steps beyond kend multiply staged zeros. (Accumulators local: in the caller's array the compiler copies them every stage.)
template <class R, bool TAIL, class Load, class Store>
__device__ __forceinline__ void mma64_loop(double* lds, int kbeg, int kend, Load load, Store store, f64x4 (&out)[4]) {
    double *As = lds, *Bs = lds + KC * LS;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    f64x4 acc[4] = {};
    R ra, rb;
    load(kbeg, ra, rb);
    for (int k0 = kbeg; k0 < kend; k0 += KC) {
        __syncthreads();
        store(As, ra);
        store_kmajor(Bs, rb);
        __syncthreads();
        if (k0 + KC < kend) load(k0 + KC, ra, rb);
        const int steps = TAIL ? min(KC, kend - k0) >> 2 : KC / 4;
        for (int s = 0; s < steps; ++s) {
            const double* a_row = As + (4 * s + lk) * LS;
            const double* b_row = Bs + (4 * s + lk) * LS;
            const double a = a_row[16 * w + lr];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b_row[16 * c + lr], acc[c], 0, 0, 0);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = acc[c];
}

// dst[row * stride + col] = acc * fac (1.0: the accumulator itself): the [64][HS] image in LDS or a [64][64] tile in global memory.
// C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
__device__ __forceinline__ void mma64_store(const f64x4 (&acc)[4], double* dst, int stride, double fac) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(16 * w + lk + 4 * r) * stride + 16 * c + lr] = acc[c][r] * fac;
}

}  // namespace
}  // namespace pesto
