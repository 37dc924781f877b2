// pesto_eval.hip - evaluation kernels: interface labels of biological assemblies (contact search on a cell grid) and the
// binary-classification scores of the reference's src/scoring.py (bc_scoring), per structure and class.
//
// The C entry points (include/pesto_hip.h) live here too: they need only the handle's device (pesto_synchronize sets it and resolves a
// deferred AUTO check) and allocate their few buffers stream-ordered per call, so they share nothing with the forward's workspace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/pesto_hip.h"

namespace pesto {

namespace {

// ------------------------------------------------------------------------------------------------ interface labels
// replaces: locate_contacts / extract_all_contacts (src/data_encoding.py:116-176, a dense torch distance matrix per pair of subunits),
// contacts_types (processing/build_dataset.py:38-51) and load_interface_labels (data_handler.py:9-23) OR-ed over the partners of a
// subunit (data_handler.py:100-126):
//     labels[res(a)] |= partner_mask[b]   for every receptor atom a and atom b of another subunit of the same assembly with |x_a - x_b| < r_thr
// The distance is the reference's fp32 torch.norm (the FMA chain of knn_key). Each assembly gets a uniform grid of cells at least
// r_thr * 1.001 wide (so a pair within r_thr is never more than one cell apart, whatever the rounding of the cell coordinates) and at most
// 2 N_s + 64 cells (the cell arrays of the batch are sized from the atom count alone: assembly s owns cells [2 off_s + 65 s, ...)).
constexpr int LBL_GRID_MAX = 64;          // cells per axis at most
struct LblGrid { float minx, miny, minz, inv_h; int nx, ny, nz, base; };

__device__ __forceinline__ int lbl_struct_of(int i, int n_struct, const int* __restrict__ offsets) {
    int lo = 0, hi = n_struct;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ void lbl_cell3(const LblGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(g.nx - 1, max(0, (int)((x - g.minx) * g.inv_h)));
    cy = min(g.ny - 1, max(0, (int)((y - g.miny) * g.inv_h)));
    cz = min(g.nz - 1, max(0, (int)((z - g.minz) * g.inv_h)));
}

// one workgroup per assembly: bounding box -> cell size and counts, cleared cell counters
__global__ __launch_bounds__(256) void k_lbl_grid_setup(int n_struct, const int* __restrict__ offsets, const float* __restrict__ X, float r_thr,
                                                        LblGrid* __restrict__ grids, int* __restrict__ cell_cnt) {
    const int s = blockIdx.x;
    const int s0 = offsets[s], s1 = offsets[s + 1];
    __shared__ float red[6][256];
    __shared__ LblGrid gsh;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = s0 + threadIdx.x; i < s1; i += 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = X[3 * (size_t)i + c]; mn[c] = fminf(mn[c], v); mx[c] = fmaxf(mx[c], v); }
#pragma unroll
    for (int c = 0; c < 3; ++c) { red[c][threadIdx.x] = mn[c]; red[3 + c][threadIdx.x] = mx[c]; }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                red[c][threadIdx.x] = fminf(red[c][threadIdx.x], red[c][threadIdx.x + off]);
                red[3 + c][threadIdx.x] = fmaxf(red[3 + c][threadIdx.x], red[3 + c][threadIdx.x + off]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        LblGrid g;
        g.base = 2 * s0 + 65 * s;
        g.minx = red[0][0]; g.miny = red[1][0]; g.minz = red[2][0];
        g.nx = g.ny = g.nz = 1; g.inv_h = 0.f;                 // one cell (every pair is examined): non-finite coordinates
        const float ex = red[3][0] - red[0][0], ey = red[4][0] - red[1][0], ez = red[5][0] - red[2][0];
        const float ext = fmaxf(ex, fmaxf(ey, ez));
        if (ext == ext && ext < 1e30f && g.minx == g.minx && g.miny == g.miny && g.minz == g.minz) {
            const long long cap = 2LL * (s1 - s0) + 64;
            float h = fmaxf(r_thr * 1.001f, ext / (float)LBL_GRID_MAX * 1.0001f);
            for (;;) {
                const int nx = (int)(ex / h) + 1, ny = (int)(ey / h) + 1, nz = (int)(ez / h) + 1;
                if ((long long)nx * ny * nz <= cap) { g.nx = nx; g.ny = ny; g.nz = nz; g.inv_h = 1.0f / h; break; }
                h *= 1.25f;
            }
        }
        grids[s] = g;
        gsh = g;
    }
    __syncthreads();
    const int nc = gsh.nx * gsh.ny * gsh.nz;
    for (int c = threadIdx.x; c <= nc; c += 256) cell_cnt[gsh.base + c] = 0;
}

__global__ __launch_bounds__(256) void k_lbl_grid_count(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                        const LblGrid* __restrict__ grids, int* __restrict__ cell_cnt, int* __restrict__ cell_of) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const LblGrid g = grids[lbl_struct_of(i, n_struct, offsets)];
    int cx, cy, cz;
    lbl_cell3(g, X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], cx, cy, cz);
    const int c = (cz * g.ny + cy) * g.nx + cx;
    cell_of[i] = c;
    atomicAdd(&cell_cnt[g.base + c], 1);
}

// exclusive scan of one assembly's cell counts (one workgroup per assembly) -> cell starts (local atom positions), cursor copy
__global__ __launch_bounds__(1024) void k_lbl_grid_scan(const LblGrid* __restrict__ grids, int* __restrict__ cell_cnt, int* __restrict__ cell_cur) {
    const LblGrid g = grids[blockIdx.x];
    const int nc = g.nx * g.ny * g.nz;
    int* cnt = cell_cnt + g.base;
    int* cur = cell_cur + g.base;
    __shared__ int part[1024];
    const int per = (nc + 1023) / 1024;
    const int c0 = min(nc, (int)threadIdx.x * per), c1 = min(nc, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) { const int n = cnt[c]; cnt[c] = run; cur[c] = run; run += n; }
    if (threadIdx.x == 1023) cnt[nc] = part[1023];
}

// atoms in cell order: (x, y, z, batch index) and (subunit, partner mask)
__global__ __launch_bounds__(256) void k_lbl_grid_scatter(int n_total, int n_struct, const int* __restrict__ offsets, const float* __restrict__ X,
                                                          const int* __restrict__ subunit, const unsigned* __restrict__ pmask,
                                                          const LblGrid* __restrict__ grids, const int* __restrict__ cell_of, int* __restrict__ cell_cur,
                                                          float4* __restrict__ sorted, int2* __restrict__ sorted_sm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int s = lbl_struct_of(i, n_struct, offsets);
    const int pos = offsets[s] + atomicAdd(&cell_cur[grids[s].base + cell_of[i]], 1);
    sorted[pos] = make_float4(X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2], __int_as_float(i));
    sorted_sm[pos] = make_int2(subunit[i], (int)pmask[i]);
}

// one thread per atom in cell order (the threads of a wave share their candidate cells); receptor atoms scan the 3 x 3 rows of three
// consecutive cells around them (each row one contiguous range of the sorted atoms). OR is order-free: the labels are deterministic.
// ties[i] = 1: a partner atom (another subunit, non-empty mask) at exactly r_thr in fp32 - where a different rounding of the distance
// would change the answer. err bit 0: a receptor atom with a residue outside [0, n_res) (skipped).
__global__ __launch_bounds__(256) void k_contact_labels(int n_total, int n_struct, const int* __restrict__ offsets, const LblGrid* __restrict__ grids,
                                                        const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                        const int2* __restrict__ sorted_sm, const int* __restrict__ residue,
                                                        const unsigned char* __restrict__ receptor, int n_res, float r_thr,
                                                        unsigned* __restrict__ labels, unsigned char* __restrict__ ties, int* __restrict__ err) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_total) return;
    const float4 a = sorted[p];
    const int i = __float_as_int(a.w);
    if (!receptor[i]) { ties[i] = 0; return; }
    const int s = lbl_struct_of(p, n_struct, offsets);
    const int own = sorted_sm[p].x;
    const int r = residue[i];
    if (r < 0 || r >= n_res) { ties[i] = 0; atomicOr(err, 1); return; }
    const LblGrid g = grids[s];
    const int* start = cell_start + g.base;
    const int s0 = offsets[s];
    int cx, cy, cz;
    lbl_cell3(g, a.x, a.y, a.z, cx, cy, cz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    unsigned bits = 0;
    int tie = 0;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const int row = (z * g.ny + y) * g.nx;
            const int j1 = s0 + start[row + x1 + 1];
            for (int j = s0 + start[row + x0]; j < j1; ++j) {
                const int2 sm = sorted_sm[j];
                if (sm.x == own || sm.y == 0) continue;
                const float4 b = sorted[j];
                const float rx = b.x - a.x, ry = b.y - a.y, rz = b.z - a.z;
                const float d = sqrtf(__fmaf_rn(rz, rz, __fmaf_rn(ry, ry, __fmul_rn(rx, rx))));     // = knn_key's distance
                if (d < r_thr) bits |= (unsigned)sm.y;
                else if (d == r_thr) tie = 1;
            }
        }
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

size_t lbl_cells_total(int n_total, int n_struct) { return 2 * (size_t)n_total + 65 * (size_t)n_struct; }

void launch_contact_labels(hipStream_t st, int n_total, int n_struct, const int* offsets, const float* X, const int* subunit, const int* residue,
                           const unsigned char* receptor, const unsigned* pmask, int n_res, float r_thr, unsigned* labels, unsigned char* ties,
                           void* grids, int* cell_cnt, int* cell_cur, int* cell_of, void* sorted, void* sorted_sm, int* err) {
    const int nb = (n_total + 255) / 256;
    LblGrid* g = static_cast<LblGrid*>(grids);
    (void)hipMemsetAsync(labels, 0, (size_t)n_res * sizeof(unsigned), st);
    hipLaunchKernelGGL(k_lbl_grid_setup, dim3(n_struct), dim3(256), 0, st, n_struct, offsets, X, r_thr, g, cell_cnt);
    hipLaunchKernelGGL(k_lbl_grid_count, dim3(nb), dim3(256), 0, st, n_total, n_struct, offsets, X, g, cell_cnt, cell_of);
    hipLaunchKernelGGL(k_lbl_grid_scan, dim3(n_struct), dim3(1024), 0, st, g, cell_cnt, cell_cur);
    hipLaunchKernelGGL(k_lbl_grid_scatter, dim3(nb), dim3(256), 0, st, n_total, n_struct, offsets, X, subunit, pmask, g, cell_of, cell_cur,
                       static_cast<float4*>(sorted), static_cast<int2*>(sorted_sm));
    hipLaunchKernelGGL(k_contact_labels, dim3(nb), dim3(256), 0, st, n_total, n_struct, offsets, g, cell_cnt, static_cast<const float4*>(sorted),
                       static_cast<const int2*>(sorted_sm), residue, receptor, n_res, r_thr, labels, ties, err);
}

void launch_bc_scores(hipStream_t st, int n_struct, int n_class, const int* roff, const unsigned char* y, const float* p, float* out) {
    hipLaunchKernelGGL(k_bc_scores, dim3(n_struct * n_class), dim3(BC_THREADS), 0, st, n_class, roff, y, p, out);
}

thread_local std::string g_eval_err;

int efail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_eval_err = buf;
    return code;
}

#define EV_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) { rc = efail(PESTO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); goto done; } \
    } while (0)

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int check_offsets(const int32_t* offs, int32_t n, int64_t total, const char* what) {
    if (offs[0] != 0 || offs[n] != total) return efail(PESTO_ERR_INVALID, "%s must span [0, %lld]", what, (long long)total);
    for (int s = 0; s < n; ++s)
        if (offs[s + 1] <= offs[s]) return efail(PESTO_ERR_INVALID, "%s: empty or unordered structure %d", what, s);
    return 0;
}

// the handle's device current, a deferred AUTO check of its last launch resolved, its own stream drained
int enter(pesto_model* m) {
    if (int rc = pesto_synchronize(m)) {
        const char* e = pesto_last_error();
        return efail(rc, "%s", e ? e : "invalid model handle");
    }
    return 0;
}

}  // namespace
}  // namespace pesto

using namespace pesto;

const char* pesto_eval_last_error(void) { return g_eval_err.c_str(); }

int pesto_interface_labels(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X,
                           const int32_t* subunit, const int32_t* residue, const uint8_t* receptor, const uint32_t* partner_mask,
                           int64_t n_res, float r_thr, uint32_t* labels_out, uint8_t* ties_out, int32_t ptr_kind, void* stream) {
    if (n_total < 1 || n_total > 0x3ffffff0 || n_struct < 1 || n_res < 1 || n_res > 0x7ffffff0 || !struct_offsets || !X || !subunit ||
        !residue || !receptor || !partner_mask || !labels_out || !ties_out)
        return efail(PESTO_ERR_INVALID, "bad arguments");
    if (!(r_thr > 0.f) || !std::isfinite(r_thr)) return efail(PESTO_ERR_INVALID, "r_thr must be a positive finite distance");
    if (ptr_kind != PESTO_PTR_HOST && ptr_kind != PESTO_PTR_DEVICE) return efail(PESTO_ERR_INVALID, "ptr_kind must be PESTO_PTR_HOST or PESTO_PTR_DEVICE");
    if (int rc = check_offsets(struct_offsets, n_struct, n_total, "struct_offsets")) return rc;
    if (int rc = enter(m)) return rc;
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)n_total, cells = lbl_cells_total((int)n_total, n_struct);
    // one stream-ordered block: offsets | error word | grids | cell counts | cursors | cell of atom | sorted atoms | (subunit, mask) sorted,
    // and for host pointers the staged inputs [X | subunit | residue | partner_mask | receptor] and outputs [labels | ties]
    size_t o = 0;
    auto take = [&o](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t oOff = take(((size_t)n_struct + 1) * 4), oErr = take(4), oG = take((size_t)n_struct * sizeof(LblGrid)), oCnt = take(cells * 4),
                 oCur = take(cells * 4), oCell = take(n * 4), oSort = take(n * 16), oSm = take(n * 8);
    const size_t oX = dev ? 0 : take(n * 12), oS = dev ? 0 : take(n * 4), oR = dev ? 0 : take(n * 4), oM = dev ? 0 : take(n * 4),
                 oT = dev ? 0 : take(n), oL = dev ? 0 : take((size_t)n_res * 4), oTi = dev ? 0 : take(n);
    char* w = nullptr;
    int err = 0, rc = 0;
    if (hipMallocAsync((void**)&w, o, st) != hipSuccess) return efail(PESTO_ERR_NOMEM, "device allocation of %zu bytes failed", o);
    EV_TRY(hipMemcpyAsync(w + oOff, struct_offsets, ((size_t)n_struct + 1) * 4, hipMemcpyHostToDevice, st));
    EV_TRY(hipMemsetAsync(w + oErr, 0, 4, st));
    if (!dev) {
        EV_TRY(hipMemcpyAsync(w + oX, X, n * 12, hipMemcpyHostToDevice, st));
        EV_TRY(hipMemcpyAsync(w + oS, subunit, n * 4, hipMemcpyHostToDevice, st));
        EV_TRY(hipMemcpyAsync(w + oR, residue, n * 4, hipMemcpyHostToDevice, st));
        EV_TRY(hipMemcpyAsync(w + oM, partner_mask, n * 4, hipMemcpyHostToDevice, st));
        EV_TRY(hipMemcpyAsync(w + oT, receptor, n, hipMemcpyHostToDevice, st));
    }
    launch_contact_labels(st, (int)n_total, n_struct, (const int*)(w + oOff), dev ? X : (const float*)(w + oX), dev ? subunit : (const int*)(w + oS),
                          dev ? residue : (const int*)(w + oR), dev ? receptor : (const unsigned char*)(w + oT),
                          dev ? partner_mask : (const unsigned*)(w + oM), (int)n_res, r_thr, dev ? labels_out : (unsigned*)(w + oL),
                          dev ? ties_out : (unsigned char*)(w + oTi), w + oG, (int*)(w + oCnt), (int*)(w + oCur), (int*)(w + oCell), w + oSort, w + oSm,
                          (int*)(w + oErr));
    EV_TRY(hipGetLastError());
    if (!dev) {
        EV_TRY(hipMemcpyAsync(labels_out, w + oL, (size_t)n_res * 4, hipMemcpyDeviceToHost, st));
        EV_TRY(hipMemcpyAsync(ties_out, w + oTi, n, hipMemcpyDeviceToHost, st));
    }
    EV_TRY(hipMemcpyAsync(&err, w + oErr, 4, hipMemcpyDeviceToHost, st));
done:
    (void)hipFreeAsync(w, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = efail(PESTO_ERR_HIP, "interface_labels: stream synchronisation failed");
    if (rc == 0 && err) rc = efail(PESTO_ERR_INVALID, "residue: a receptor atom's residue is outside [0, n_res)");
    return rc;
}

int pesto_bc_scores(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                    float* scores_out, int32_t ptr_kind, void* stream) {
    if (n_struct < 1 || n_class < 1 || n_class > 1024 || (int64_t)n_struct * n_class > 0x7fffffff || !res_offsets || !y || !p || !scores_out)
        return efail(PESTO_ERR_INVALID, "bad arguments");
    if (ptr_kind != PESTO_PTR_HOST && ptr_kind != PESTO_PTR_DEVICE) return efail(PESTO_ERR_INVALID, "ptr_kind must be PESTO_PTR_HOST or PESTO_PTR_DEVICE");
    const int64_t R = res_offsets[n_struct];
    if (R < 1 || R * n_class > 0x7fffffff) return efail(PESTO_ERR_INVALID, "bad arguments");
    if (int rc = check_offsets(res_offsets, n_struct, R, "res_offsets")) return rc;
    if (int rc = enter(m)) return rc;
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)R * n_class, n_out = (size_t)n_struct * 8 * n_class * 4;
    size_t o = 0;
    auto take = [&o](size_t b) { const size_t at = o; o += align256(b); return at; };
    const size_t oOff = take(((size_t)n_struct + 1) * 4), oY = dev ? 0 : take(rows), oP = dev ? 0 : take(rows * 4), oO = dev ? 0 : take(n_out);
    char* w = nullptr;
    int rc = 0;
    if (hipMallocAsync((void**)&w, o, st) != hipSuccess) return efail(PESTO_ERR_NOMEM, "device allocation of %zu bytes failed", o);
    EV_TRY(hipMemcpyAsync(w + oOff, res_offsets, ((size_t)n_struct + 1) * 4, hipMemcpyHostToDevice, st));
    if (!dev) {
        EV_TRY(hipMemcpyAsync(w + oY, y, rows, hipMemcpyHostToDevice, st));
        EV_TRY(hipMemcpyAsync(w + oP, p, rows * 4, hipMemcpyHostToDevice, st));
    }
    launch_bc_scores(st, n_struct, n_class, (const int*)(w + oOff), dev ? y : (const unsigned char*)(w + oY), dev ? p : (const float*)(w + oP),
                     dev ? scores_out : (float*)(w + oO));
    EV_TRY(hipGetLastError());
    if (!dev) EV_TRY(hipMemcpyAsync(scores_out, w + oO, n_out, hipMemcpyDeviceToHost, st));
done:
    (void)hipFreeAsync(w, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = efail(PESTO_ERR_HIP, "bc_scores: stream synchronisation failed");
    return rc;
}
