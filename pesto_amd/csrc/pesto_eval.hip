// pesto_eval.hip - evaluation kernels: interface labels of biological assemblies (contact search on the cell grid of pesto_cellgrid.h) and
// the binary-classification scores of the reference's src/scoring.py (bc_scoring), per structure and class.
//
// The C entry points (include/pesto_hip.h) live here too, on the call plumbing of pesto_call.h.
#include <cmath>

#include "pesto_call.h"
#include "pesto_cellgrid.h"

namespace pesto {

namespace {

// ------------------------------------------------------------------------------------------------ interface labels
// replaces: locate_contacts / extract_all_contacts (src/data_encoding.py:116-176), contacts_types (processing/build_dataset.py:38-51) and
// load_interface_labels (data_handler.py:9-23) OR-ed over the partners of a subunit (data_handler.py:100-126):
//     labels[res(a)] |= partner_mask[b]   for every receptor atom a and atom b of another subunit of the same assembly with |x_a - x_b| < r_thr
// beside the sorted coordinates: (subunit, partner mask)
struct LblPayload {
    const int* subunit; const unsigned* pmask; int2* sorted_sm;
    __device__ void operator()(int pos, int i) const { sorted_sm[pos] = make_int2(subunit[i], (int)pmask[i]); }
};

// one thread per atom in cell order (the threads of a wave share their candidate cells); receptor atoms scan the 3 x 3 rows of three
// consecutive cells around them (each row one contiguous range of the sorted atoms). OR is order-free: the labels are deterministic.
// ties[i] = 1: a partner atom (another subunit, non-empty mask) at exactly r_thr in fp32 - where a different rounding of the distance
// would change the answer. err bit 0: a receptor atom with a residue outside [0, n_res) (skipped).
__global__ __launch_bounds__(256) void k_contact_labels(int n_total, int n_struct, const int* __restrict__ offsets, const CellGrid* __restrict__ grids,
                                                        const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                        const int2* __restrict__ sorted_sm, const int* __restrict__ residue,
                                                        const unsigned char* __restrict__ receptor, int n_res, float r_thr,
                                                        unsigned* __restrict__ labels, unsigned char* __restrict__ ties, int* __restrict__ err) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_total) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    if (!receptor[i]) { ties[i] = 0; return; }
    const int s = struct_of(p, n_struct, offsets);
    const int own = sorted_sm[p].x;
    const int r = residue[i];
    if (r < 0 || r >= n_res) { ties[i] = 0; atomicOr(err, 1); return; }
    unsigned bits = 0;
    int tie = 0;
    for_each_neighbour(grids[s], cell_start, offsets[s], a, [&](int j) {
        const int2 sm = sorted_sm[j];
        if (sm.x == own || sm.y == 0) return;
        const float d = dist(a, sorted[j]);
        if (d < r_thr) bits |= (unsigned)sm.y;
        else if (d == r_thr) tie = 1;
    });
    ties[i] = (unsigned char)tie;
    if (bits) atomicOr(&labels[r], bits);
}

// ------------------------------------------------------------------------------------------------ scores
// replaces: bc_scoring (src/scoring.py:77-96) per structure - one workgroup per (structure, class). Exact integer counts (q = round(p)
// half to even, i.e. p > 0.5 for a probability), std as torch.std (unbiased, fp64 accumulation, NaN for R = 1), and roc_auc_score as the
// Mann-Whitney U / (P N) with ties counted 1/2: 2U counted exactly in int64 from every (positive, negative) pair - each thread takes rows of
// the smaller class and compares them with the other class, staged through LDS in tiles. The eight rows (acc, ppv, npv, tpr, tnr, mcc,
// auc, std) follow the reference's float32 arithmetic and NaN rules.
constexpr int BC_THREADS = 256;
constexpr int BC_TILE = 2048;

template <typename T>
__device__ __forceinline__ T bc_block_sum(T v, T* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    T t = 0;
#pragma unroll
    for (int k = 0; k < BC_THREADS / 64; ++k) t += red[k];
    return t;
}

__global__ __launch_bounds__(BC_THREADS) void k_bc_scores(int n_class, const int* __restrict__ roff, const unsigned char* __restrict__ y,
                                                          const float* __restrict__ p, float* __restrict__ out) {
    const int s = blockIdx.x / n_class, c = blockIdx.x % n_class;
    const int r0 = roff[s], r1 = roff[s + 1];
    __shared__ long long red_i[BC_THREADS / 64];
    __shared__ double red_d[BC_THREADS / 64];
    __shared__ unsigned long long red_u[BC_THREADS / 64];
    __shared__ float tile_p[BC_TILE];
    __shared__ unsigned char tile_y[BC_TILE];
    long long tp = 0, fp = 0, pos = 0;
    double sum = 0.0;
    for (int r = r0 + threadIdx.x; r < r1; r += BC_THREADS) {
        const float v = p[(size_t)r * n_class + c];
        const bool yt = y[(size_t)r * n_class + c] != 0, q = rintf(v) != 0.f;
        tp += yt && q; fp += !yt && q; pos += yt;
        sum += (double)v;
    }
    const long long R = r1 - r0;
    const long long TPi = bc_block_sum(tp, red_i), FPi = bc_block_sum(fp, red_i), Pi = bc_block_sum(pos, red_i);
    const long long Ni = R - Pi, FNi = Pi - TPi, TNi = Ni - FPi;
    const double mean = bc_block_sum(sum, red_d) / (double)R;
    double m2 = 0.0;
    for (int r = r0 + threadIdx.x; r < r1; r += BC_THREADS) {
        const double d = (double)p[(size_t)r * n_class + c] - mean;
        m2 += d * d;
    }
    m2 = bc_block_sum(m2, red_d);
    // 2U over the (positive, negative) pairs; the rows of the smaller class are the outer loop
    unsigned long long u2 = 0;
    if (Pi > 0 && Ni > 0) {
        const unsigned char outer = Pi <= Ni ? 1 : 0;
        for (int t0 = r0; t0 < r1; t0 += BC_TILE) {
            const int nt = min(BC_TILE, r1 - t0);
            __syncthreads();
            for (int k = threadIdx.x; k < nt; k += BC_THREADS) {
                tile_p[k] = p[(size_t)(t0 + k) * n_class + c];
                tile_y[k] = y[(size_t)(t0 + k) * n_class + c] != 0;
            }
            __syncthreads();
            for (int r = r0 + threadIdx.x; r < r1; r += BC_THREADS) {
                if ((y[(size_t)r * n_class + c] != 0) != (outer != 0)) continue;
                const float v = p[(size_t)r * n_class + c];
                unsigned cnt = 0;          // <= 2 * BC_TILE per tile
                for (int k = 0; k < nt; ++k) {
                    const float w = tile_p[k];
                    const bool other = tile_y[k] != outer;
                    const float hi = outer ? v : w, lo = outer ? w : v;       // positive's p, negative's p
                    cnt += other ? (hi > lo ? 2u : (hi == lo ? 1u : 0u)) : 0u;
                }
                u2 += cnt;
            }
        }
    }
    u2 = bc_block_sum(u2, red_u);
    if (threadIdx.x != 0) return;
    const float TP = (float)TPi, TN = (float)TNi, FP = (float)FPi, FN = (float)FNi;
    const float qnan = __int_as_float(0x7fc00000);
    auto nan_if_inf = [&](float v) { return isinf(v) ? qnan : v; };
    float* o = out + (size_t)s * 8 * n_class + c;
    o[0 * n_class] = (TP + TN) / (TP + TN + FP + FN);
    o[1 * n_class] = Pi > 0 ? TP / (TP + FP) : qnan;
    o[2 * n_class] = Ni > 0 ? TN / (TN + FN) : qnan;
    o[3 * n_class] = nan_if_inf(TP / (TP + FN));
    o[4 * n_class] = nan_if_inf(TN / (TN + FP));
    // ((TP*TN) - (FP*FN)) / sqrt((TP+FP)*(TP+FN)*(TN+FP)*(TN+FN)), every operation rounded to float32 as torch evaluates it (no contraction)
    const float num = __fsub_rn(__fmul_rn(TP, TN), __fmul_rn(FP, FN));
    const float den = sqrtf(__fmul_rn(__fmul_rn(__fmul_rn(TP + FP, TP + FN), TN + FP), TN + FN));
    o[5 * n_class] = nan_if_inf(num / den);
    o[6 * n_class] = (Pi > 0 && Ni > 0) ? (float)((double)u2 / (2.0 * (double)Pi * (double)Ni)) : qnan;
    o[7 * n_class] = (float)sqrt(m2 / (double)(R - 1));
}

void launch_contact_labels(hipStream_t st, int n_total, int n_struct, const int* offsets, const float* X, const int* subunit, const int* residue,
                           const unsigned char* receptor, const unsigned* pmask, int n_res, float r_thr, unsigned* labels, unsigned char* ties,
                           const GridBufs& g, int2* sorted_sm, int* err) {
    grid_build(st, n_total, n_struct, offsets, X, r_thr, g, NoCheck{}, LblPayload{subunit, pmask, sorted_sm});
    hipLaunchKernelGGL(k_contact_labels, dim3((n_total + 255) / 256), dim3(256), 0, st, n_total, n_struct, offsets, (const CellGrid*)g.grids,
                       (const int*)g.cell_cnt, (const float4*)g.sorted, (const int2*)sorted_sm, residue, receptor, n_res, r_thr, labels, ties, err);
}

void launch_bc_scores(hipStream_t st, int n_struct, int n_class, const int* roff, const unsigned char* y, const float* p, float* out) {
    hipLaunchKernelGGL(k_bc_scores, dim3(n_struct * n_class), dim3(BC_THREADS), 0, st, n_class, roff, y, p, out);
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_eval_last_error(void) { return last_error(); }

int pesto_interface_labels(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X,
                           const int32_t* subunit, const int32_t* residue, const uint8_t* receptor, const uint32_t* partner_mask,
                           int64_t n_res, float r_thr, uint32_t* labels_out, uint8_t* ties_out, int32_t ptr_kind, void* stream) {
    if (n_total < 1 || n_total > 0x3ffffff0 || n_struct < 1 || n_res < 1 || n_res > 0x7ffffff0 || !struct_offsets || !X || !subunit ||
        !residue || !receptor || !partner_mask || !labels_out || !ties_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (!(r_thr > 0.f) || !std::isfinite(r_thr)) return fail(PESTO_ERR_INVALID, "r_thr must be a positive finite distance");
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (int rc = check_offsets(struct_offsets, n_struct, n_total, "struct_offsets")) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t n = (size_t)n_total, cells = cells_before(n, (size_t)n_struct);
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(struct_offsets, ((size_t)n_struct + 1) * 4), iX = bf.input(X, n * 12), iS = bf.input(subunit, n * 4),
              iR = bf.input(residue, n * 4), iT = bf.input(receptor, n), iM = bf.input(partner_mask, n * 4);
    const int iL = bf.output(labels_out, (size_t)n_res * 4, 0), iTi = bf.output(ties_out, n);
    const int iErr = bf.scratch(4, 0), iG = bf.scratch((size_t)n_struct * sizeof(CellGrid)), iCnt = bf.scratch(cells * 4), iCur = bf.scratch(cells * 4),
              iCell = bf.scratch(n * 4), iSort = bf.scratch(n * 16), iSm = bf.scratch(n * 8);
    int err = 0;
    int rc = bf.upload();
    if (rc == 0) {
        launch_contact_labels(bf.stm, (int)n_total, n_struct, bf.ptr<const int>(iOff), bf.ptr<const float>(iX), bf.ptr<const int>(iS),
                              bf.ptr<const int>(iR), bf.ptr<const unsigned char>(iT), bf.ptr<const unsigned>(iM), (int)n_res, r_thr,
                              bf.ptr<unsigned>(iL), bf.ptr<unsigned char>(iTi),
                              GridBufs{bf.ptr<CellGrid>(iG), bf.ptr<int>(iCnt), bf.ptr<int>(iCur), bf.ptr<int>(iCell), bf.ptr<float4>(iSort)},
                              bf.ptr<int2>(iSm), bf.ptr<int>(iErr));
        rc = bf.read(iErr, &err, 4);
    }
    rc = bf.finish(rc, "interface_labels");
    if (rc == 0 && err) rc = fail(PESTO_ERR_INVALID, "residue: a receptor atom's residue is outside [0, n_res)");
    return rc;
}

int pesto_bc_scores(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                    float* scores_out, int32_t ptr_kind, void* stream) {
    if (n_struct < 1 || n_class < 1 || n_class > 1024 || (int64_t)n_struct * n_class > 0x7fffffff || !res_offsets || !y || !p || !scores_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    const int64_t R = res_offsets[n_struct];
    if (R < 1 || R * n_class > 0x7fffffff) return fail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_offsets(res_offsets, n_struct, R, "res_offsets")) return rc;
    if (int rc = begin(m, ptr_kind)) return rc;
    const size_t rows = (size_t)R * n_class;
    Buffers bf(ptr_kind, stream);
    const int iOff = bf.table(res_offsets, ((size_t)n_struct + 1) * 4), iY = bf.input(y, rows), iP = bf.input(p, rows * 4),
              iO = bf.output(scores_out, (size_t)n_struct * 8 * n_class * 4);
    int rc = bf.upload();
    if (rc == 0)
        launch_bc_scores(bf.stm, n_struct, n_class, bf.ptr<const int>(iOff), bf.ptr<const unsigned char>(iY), bf.ptr<const float>(iP), bf.ptr<float>(iO));
    return bf.finish(rc, "bc_scores");
}
