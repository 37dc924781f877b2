// pesto_train.hip - the training step on gfx950, all float32: training forward (the exact fp32 kernels of pesto_kernels.hip, every
// layer's input state kept), loss, backward and Adam.
//
// Math restated from the reference (file:line relative to /root/reference):
//   eval_step, loss weighting           model/main.py:42-58
//   backward + optimiser step           model/main.py:186-200 (torch.optim.Adam defaults)
//   state-update layer                  src/model_operations.py:87-154, checkpointed :234-236, sink reset :239-240
//   residue pool + decoder              src/model_operations.py:197-213, model/model.py:46-50
//   geometry (for d X)                  src/model_operations.py:6-22
//   autograd use (caller's d z)         model/main.py:159, 196-200: a torch Module's forward / backward (pesto_amd.nn)
//
// The backward mirrors the forward kernels phase by phase: a kernel recomputes its stage from the stage's inputs, keeps every
// activation in LDS and walks the phases in reverse. Gradients are accumulated in the layout of the PLAIN section of the device weight
// image (pesto_schema.h) and handed out / applied in blob order through blob_to_plain_image() below. Weight gradients are reduced inside a
// workgroup first (float32, fixed order) and then added to the image-layout buffer with 64-bit fixed-point atomics (gadd below), like
// the scatter-add of the gather: the sums do not depend on the order of the workgroups, so a step is bit-reproducible from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>

#include "pesto_call.h"
#include "pesto_geom.h"
#include "pesto_kernels.h"

namespace pesto {

namespace {

__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : expf(x) - 1.0f; }
// ELU'(pre-activation) from the activation a = ELU(pre): 1 for pre > 0, exp(pre) = a + 1 otherwise
__device__ __forceinline__ float elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }
// Gradients that several workgroups add to (weight gradients, the scatter-add of the gather) are accumulated as 64-bit fixed point with
// 40 fractional bits: integer addition is associative, so the sum does not depend on the order in which the workgroups arrive and a
// step gives the same bits every time it runs. A term is rounded to 2^-40 = 9.1e-13 (Adam's eps is 1e-8: a gradient that small does
// not move a weight) and clamped to +-4e6; a sum beyond +-2^23 = 8.4e6 wraps - a run that has long diverged.
typedef long long fx_t;
constexpr float FX_SCALE = 1099511627776.0f;      // 2^40
constexpr float FX_CLAMP = 4.0e6f;
__device__ __forceinline__ fx_t to_fx(float v) { return __float2ll_rn(fminf(fmaxf(v, -FX_CLAMP), FX_CLAMP) * FX_SCALE); }
__device__ __forceinline__ float from_fx(fx_t v) { return (float)((double)v * (1.0 / 1099511627776.0)); }
__device__ __forceinline__ void gadd(fx_t* p, float v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)to_fx(v)); }

// ---------------------------------------------------------------------------------------------- small MLPs, 8 rows per workgroup
// 256 threads = 8 rows x 32 lanes (g = t >> 5, s = t & 31); every array lives in LDS, row g at [g * stride].
__device__ __forceinline__ float lin_col(const float* __restrict__ W, const LinearW l, const float* x, int s) {
    if (s >= l.n_out) return 0.0f;
    float acc = l.b >= 0 ? W[l.b + s] : 0.0f;
    const float* w = W + l.w + s;
    for (int k = 0; k < l.n_in; ++k) acc += x[k] * w[k * l.n_out];
    return acc;
}

// h1 = ELU(l0 x), h2 = ELU(l1 h1) for rows g < rows (callers sync before reading)
__device__ __forceinline__ void mlp3_hidden(const float* __restrict__ W, const MlpW& m, const float* x, int xs, float* h1, float* h2, int rows) {
    const int g = threadIdx.x >> 5, s = threadIdx.x & 31;
    if (g < rows) h1[g * 32 + s] = elu(lin_col(W, m.l[0], x + g * xs, s));
    __syncthreads();
    if (g < rows) h2[g * 32 + s] = elu(lin_col(W, m.l[1], h1 + g * 32, s));
    __syncthreads();
}

// dW[k][o] += sum_g x[g][k] dy[g][o], db[o] += sum_g dy[g][o] of one Linear (image layout Wt[in][out]), one atomic per entry
__device__ __forceinline__ void lin_wgrad(fx_t* __restrict__ G, const LinearW l, const float* x, int xs, const float* dy, int ys, int rows) {
    const int n = l.n_in * l.n_out;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int k = idx / l.n_out, o = idx - k * l.n_out;
        float v = 0.0f;
        for (int g = 0; g < rows; ++g) v += x[g * xs + k] * dy[g * ys + o];
        gadd(G + l.w + idx, v);
    }
    if (l.b >= 0 && (int)threadIdx.x < l.n_out) {
        float v = 0.0f;
        for (int g = 0; g < rows; ++g) v += dy[g * ys + threadIdx.x];
        gadd(G + l.b + threadIdx.x, v);
    }
}

// Backward of y = l2 ELU(l1 ELU(l0 x)) for rows g < rows: dy [rows][ys] (ZERO for rows that must not count), h1 / h2 the activations.
// d2 / d1: scratch [8][32]. Weight gradients first, then (dx != nullptr) dx [rows][dxs] = l0^T d1, which may overwrite x.
__device__ __forceinline__ void mlp3_bwd(const float* __restrict__ W, fx_t* __restrict__ G, const MlpW& m, const float* x, int xs,
                                         const float* h1, const float* h2, const float* dy, int ys, float* d2, float* d1, float* dx, int dxs,
                                         int rows) {
    const int g = threadIdx.x >> 5, s = threadIdx.x & 31;
    if (g < rows) {
        float acc = 0.0f;
        const float* w = W + m.l[2].w + s * m.l[2].n_out;
        for (int o = 0; o < m.l[2].n_out; ++o) acc += w[o] * dy[g * ys + o];
        d2[g * 32 + s] = acc * elu_grad(h2[g * 32 + s]);
    }
    __syncthreads();
    if (g < rows) {
        float acc = 0.0f;
        const float* w = W + m.l[1].w + s * 32;
        for (int o = 0; o < 32; ++o) acc += w[o] * d2[g * 32 + o];
        d1[g * 32 + s] = acc * elu_grad(h1[g * 32 + s]);
    }
    __syncthreads();
    lin_wgrad(G, m.l[2], h2, 32, dy, ys, rows);
    lin_wgrad(G, m.l[1], h1, 32, d2, 32, rows);
    lin_wgrad(G, m.l[0], x, xs, d1, 32, rows);
    __syncthreads();
    if (dx && g < rows) {
        for (int k = s; k < m.l[0].n_in; k += 32) {
            float acc = 0.0f;
            const float* w = W + m.l[0].w + k * 32;
            for (int o = 0; o < 32; ++o) acc += w[o] * d1[g * 32 + o];
            dx[g * dxs + k] = acc;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------- argument check
// bit 0: an id outside [0, N]; bit 1: a residue outside [0, R); bit 2: an empty residue. Also finds the residue segments (the encoding
// of seg_bound_atom, pesto_kernels.hip: lo_enc = 0x7fffffff - first atom, hi = last atom + 1; both zeroed before).
template <typename IdT>
__global__ __launch_bounds__(256) void k_train_check(int N, int R, int k, const IdT* __restrict__ ids, const int* __restrict__ roa,
                                                     int* __restrict__ lo_enc, int* __restrict__ hi, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)N * k) {
        const long long id = (long long)ids[e];
        if (id < 0 || id > N) atomicOr(flag, 1);
    }
    if (e < N) {
        const int r = roa[e];
        if (r < 0 || r >= R) atomicOr(flag, 2);
        else { atomicMax(&lo_enc[r], 0x7fffffff - (int)e); atomicMax(&hi[r], (int)e + 1); }
    }
}
__global__ __launch_bounds__(256) void k_train_check_empty(int R, const int* __restrict__ hi, int* __restrict__ flag) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R && hi[r] == 0) atomicOr(flag, 4);
}

// ---------------------------------------------------------------------------------------------- loss (model/main.py:49-58)
// pos_ratios += (mean_rows(y) - pos_ratios) / (1 + sqrt(global_step)), in device memory (one workgroup, C <= 32)
__global__ __launch_bounds__(256) void k_pos_ratios(int R, int C, const float* __restrict__ y, float* __restrict__ pos, float denom) {
    __shared__ float part[8][32];
    const int g = threadIdx.x >> 5, c = threadIdx.x & 31;
    float sum = 0.0f;
    if (c < C)
        for (int r = g; r < R; r += 8) sum += y[(size_t)r * C + c];
    part[g][c] = sum;
    __syncthreads();
    if (g == 0 && c < C) {
        float tot = 0.0f;
        for (int j = 0; j < 8; ++j) tot += part[j][c];
        const float mean = tot / (float)R;
        pos[c] += (mean - pos[c]) / denom;
    }
}
// dloss = (1 - y) z + (1 + (pos_weight - 1) y)(log1p(exp(-|z|)) + max(-z, 0)) (torch's BCEWithLogitsLoss), losses = factor dloss / R,
// p = sigmoid(z), dz = d sum(losses) / dz (the three per-class vectors carry no gradient)
__global__ __launch_bounds__(256) void k_loss(int R, int C, float f, const float* __restrict__ z, const float* __restrict__ y,
                                              const float* __restrict__ pos, float* __restrict__ losses, float* __restrict__ p_out,
                                              float* __restrict__ dz) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= R * C) return;
    const int c = e % C;
    float psum = 0.0f;
    for (int j = 0; j < C; ++j) psum += pos[j];
    const float pr = pos[c];
    const float pw = f * (1.0f - pr) / (pr + 1e-6f);
    const float factor = pr / psum;
    const float zv = z[e], yv = y[e];
    const float lw = 1.0f + (pw - 1.0f) * yv;
    const float dl = (1.0f - yv) * zv + lw * (log1pf(expf(-fabsf(zv))) + fmaxf(-zv, 0.0f));
    const float ez = expf(-fabsf(zv));
    const float sig = zv >= 0.0f ? 1.0f / (1.0f + ez) : ez / (1.0f + ez);      // sigmoid(z)
    if (losses) losses[e] = factor * dl / (float)R;
    if (p_out) p_out[e] = sig;
    if (dz) dz[e] = factor * ((1.0f - yv) - lw * (1.0f - sig)) / (float)R;
}

// ---------------------------------------------------------------------------------------------- head backward (pool + dm)
// pass 1, one wave per residue: the segmented softmax statistics and the pooled heads again (k_pool_reduce's first half):
// st [R][16] = max[8] | den[8] (channel 2h = scalar head h, 2h+1 = vector head h), qh [R][128], ph [R][3][128] flattened s*4+h
__global__ __launch_bounds__(64) void k_head_pool(int R, const float* __restrict__ q, const float* __restrict__ p, const float* __restrict__ a,
                                                  const int* __restrict__ roa, const int* __restrict__ lo, const int* __restrict__ hi,
                                                  float* __restrict__ st, float* __restrict__ qh, float* __restrict__ ph) {
    const int r = blockIdx.x, lane = threadIdx.x, s = lane & 31, hf = lane >> 5;
    const int i0 = 0x7fffffff - lo[r], i1 = hi[r];
    float mx[4], den[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { mx[c] = -INFINITY; den[c] = 0.0f; }
    for (int i = i0; i < i1; ++i)
        if (roa[i] == r) {
            const float4 v = *reinterpret_cast<const float4*>(a + (size_t)i * 8 + 4 * hf);
            mx[0] = fmaxf(mx[0], v.x); mx[1] = fmaxf(mx[1], v.y); mx[2] = fmaxf(mx[2], v.z); mx[3] = fmaxf(mx[3], v.w);
        }
    for (int i = i0; i < i1; ++i)
        if (roa[i] == r) {
            const float4 v = *reinterpret_cast<const float4*>(a + (size_t)i * 8 + 4 * hf);
            den[0] += expf(v.x - mx[0]); den[1] += expf(v.y - mx[1]); den[2] += expf(v.z - mx[2]); den[3] += expf(v.w - mx[3]);
        }
    float aq[2] = {0.f, 0.f}, ap[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int i = i0; i < i1; ++i)
        if (roa[i] == r) {
            const float4 v = *reinterpret_cast<const float4*>(a + (size_t)i * 8 + 4 * hf);
            const float w[4] = {expf(v.x - mx[0]) / den[0], expf(v.y - mx[1]) / den[1], expf(v.z - mx[2]) / den[2], expf(v.w - mx[3]) / den[3]};
            const float qv = q[(size_t)i * S + s];
            const float pv[3] = {p[(size_t)i * 96 + s], p[(size_t)i * 96 + 32 + s], p[(size_t)i * 96 + 64 + s]};
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                aq[hh] += qv * w[2 * hh];
#pragma unroll
                for (int x = 0; x < 3; ++x) ap[hh][x] += pv[x] * w[2 * hh + 1];
            }
        }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int h = 2 * hf + hh;
        qh[(size_t)r * 128 + s * PH + h] = aq[hh];
#pragma unroll
        for (int x = 0; x < 3; ++x) ph[((size_t)r * 3 + x) * 128 + s * PH + h] = ap[hh][x];
    }
    if (s == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { st[(size_t)r * 16 + 4 * hf + c] = mx[c]; st[(size_t)r * 16 + 8 + 4 * hf + c] = den[c]; }
    }
}

// pass 2, 8 residues per workgroup: zdm / zdm_vec / norm / dm forward and backward; qh / ph are overwritten with their gradients
__global__ __launch_bounds__(256) void k_head_decode_bwd(const float* __restrict__ W, fx_t* __restrict__ G, ModelW mw, int n_out, int R,
                                                         const float* __restrict__ dz, float* __restrict__ qh, float* __restrict__ ph) {
    __shared__ float xq[8][128];      // qh, then d qh
    __shared__ float xp[8][384];      // ph [x][128], then d ph
    __shared__ float zr[8][64];       // [qr | |pr|], then d zr
    __shared__ float pr[8][96];       // pr, then d pr
    __shared__ float a1[8][32], a2[8][32], b1[8][32], b2[8][32], d1[8][32], d2[8][32], dy[8][32];
    const int g = threadIdx.x >> 5, s = threadIdx.x & 31;
    const int r0 = blockIdx.x * 8, rows = min(8, R - r0);
    const int r = r0 + g;
    if (g < rows) {
        for (int k = s; k < 128; k += 32) xq[g][k] = qh[(size_t)r * 128 + k];
        for (int k = s; k < 384; k += 32) xp[g][k] = ph[(size_t)r * 384 + k];
        dy[g][s] = s < n_out ? dz[(size_t)r * n_out + s] : 0.0f;
    }
    __syncthreads();
    mlp3_hidden(W, mw.zdm, &xq[0][0], 128, &a1[0][0], &a2[0][0], rows);
    if (g < rows) {
        zr[g][s] = lin_col(W, mw.zdm.l[2], a2[g], s);
        float n2 = 0.0f;
#pragma unroll
        for (int x = 0; x < 3; ++x) { const float v = lin_col(W, mw.zdm_vec, xp[g] + 128 * x, s); pr[g][32 * x + s] = v; n2 += v * v; }
        zr[g][32 + s] = sqrtf(n2);
    }
    __syncthreads();
    mlp3_hidden(W, mw.dm, &zr[0][0], 64, &b1[0][0], &b2[0][0], rows);
    mlp3_bwd(W, G, mw.dm, &zr[0][0], 64, &b1[0][0], &b2[0][0], &dy[0][0], 32, &d2[0][0], &d1[0][0], &zr[0][0], 64, rows);
    // norm: d pr = d|pr| pr / |pr| (0 at |pr| = 0); zr now holds [d qr | d|pr|], the norm itself is taken again from pr
    if (g < rows) {
        const float v0 = pr[g][s], v1 = pr[g][32 + s], v2 = pr[g][64 + s];
        const float nrm = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
        const float f = nrm > 0.0f ? zr[g][32 + s] / nrm : 0.0f;
        pr[g][s] = f * v0; pr[g][32 + s] = f * v1; pr[g][64 + s] = f * v2;
        dy[g][s] = zr[g][s];
    }
    __syncthreads();
    // zdm_vec (bias-free, one weight for the three components): weight gradient, then d ph in place
    for (int idx = threadIdx.x; idx < 128 * 32; idx += 256) {
        const int k = idx >> 5, o = idx & 31;
        float v = 0.0f;
        for (int gg = 0; gg < rows; ++gg)
#pragma unroll
            for (int x = 0; x < 3; ++x) v += xp[gg][128 * x + k] * pr[gg][32 * x + o];
        gadd(G + mw.zdm_vec.w + idx, v);
    }
    __syncthreads();
    if (g < rows)
        for (int e = s; e < 384; e += 32) {
            const int x = e >> 7, k = e & 127;
            float acc = 0.0f;
            const float* w = W + mw.zdm_vec.w + k * 32;
            for (int o = 0; o < 32; ++o) acc += w[o] * pr[g][32 * x + o];
            xp[g][e] = acc;
        }
    __syncthreads();
    mlp3_bwd(W, G, mw.zdm, &xq[0][0], 128, &a1[0][0], &a2[0][0], &dy[0][0], 32, &d2[0][0], &d1[0][0], &xq[0][0], 128, rows);
    if (g < rows) {
        for (int k = s; k < 128; k += 32) qh[(size_t)r * 128 + k] = xq[g][k];
        for (int k = s; k < 384; k += 32) ph[(size_t)r * 384 + k] = xp[g][k];
    }
}

// pass 3, one wave per residue: the pool's weighted sums and its softmax backwards. dqh / dph: gradients of the pooled heads (pass 2).
// Writes (every atom belongs to exactly one residue) dq [N][32], dp [N][96] = the direct terms, da [N][8] = gradient of the pool logits.
__global__ __launch_bounds__(64) void k_head_pool_bwd(int R, const float* __restrict__ q, const float* __restrict__ p, const float* __restrict__ a,
                                                      const int* __restrict__ roa, const int* __restrict__ lo, const int* __restrict__ hi,
                                                      const float* __restrict__ st, const float* __restrict__ dqh, const float* __restrict__ dph,
                                                      float* __restrict__ dq, float* __restrict__ dp, float* __restrict__ da) {
    const int r = blockIdx.x, lane = threadIdx.x, s = lane & 31, hf = lane >> 5;
    const int i0 = 0x7fffffff - lo[r], i1 = hi[r];
    float mx[4], den[4], gq[2], gp[2][3];
#pragma unroll
    for (int c = 0; c < 4; ++c) { mx[c] = st[(size_t)r * 16 + 4 * hf + c]; den[c] = st[(size_t)r * 16 + 8 + 4 * hf + c]; }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int h = 2 * hf + hh;
        gq[hh] = dqh[(size_t)r * 128 + s * PH + h];
#pragma unroll
        for (int x = 0; x < 3; ++x) gp[hh][x] = dph[((size_t)r * 3 + x) * 128 + s * PH + h];
    }
    // d weight of atom i, channel c (this half's four channels): dot of the head gradient with the atom's state, summed over the 32 lanes
    auto dweights = [&](int i, float dw[4], float w[4]) {
        const float4 v = *reinterpret_cast<const float4*>(a + (size_t)i * 8 + 4 * hf);
        w[0] = expf(v.x - mx[0]) / den[0]; w[1] = expf(v.y - mx[1]) / den[1]; w[2] = expf(v.z - mx[2]) / den[2]; w[3] = expf(v.w - mx[3]) / den[3];
        const float qv = q[(size_t)i * S + s];
        const float pv[3] = {p[(size_t)i * 96 + s], p[(size_t)i * 96 + 32 + s], p[(size_t)i * 96 + 64 + s]};
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            dw[2 * hh] = gq[hh] * qv;
            dw[2 * hh + 1] = gp[hh][0] * pv[0] + gp[hh][1] * pv[1] + gp[hh][2] * pv[2];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            for (int off = 16; off > 0; off >>= 1) dw[c] += __shfl_xor(dw[c], off);      // (within the half: offsets below 32)
    };
    double dot[4] = {0., 0., 0., 0.};
    for (int i = i0; i < i1; ++i)
        if (roa[i] == r) {
            float dw[4], w[4];
            dweights(i, dw, w);
#pragma unroll
            for (int c = 0; c < 4; ++c) dot[c] += (double)(w[c] * dw[c]);
        }
    for (int i = i0; i < i1; ++i)
        if (roa[i] == r) {
            float dw[4], w[4];
            dweights(i, dw, w);
            if (s < 4) da[(size_t)i * 8 + 4 * hf + s] = w[s] * (dw[s] - (float)dot[s]);
            // direct terms: this half holds heads 2hf, 2hf+1; the other half's sum comes over by a shuffle
            float vq = w[0] * gq[0] + w[2] * gq[1];
            float vp[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) vp[x] = w[1] * gp[0][x] + w[3] * gp[1][x];
            vq += __shfl_xor(vq, 32);
#pragma unroll
            for (int x = 0; x < 3; ++x) vp[x] += __shfl_xor(vp[x], 32);
            if (hf == 0) {
                dq[(size_t)i * S + s] = vq;
#pragma unroll
                for (int x = 0; x < 3; ++x) dp[(size_t)i * 96 + 32 * x + s] = vp[x];
            }
        }
}

// pass 4, 8 atoms per workgroup: backward of sam([q_i | |p_i|]) (k_pool_logits), added to dq / dp
__global__ __launch_bounds__(256) void k_head_sam_bwd(const float* __restrict__ W, fx_t* __restrict__ G, MlpW sam, int N, const float* __restrict__ q,
                                                      const float* __restrict__ p, const float* __restrict__ da, float* __restrict__ dq,
                                                      float* __restrict__ dp) {
    __shared__ float zin[8][64], h1[8][32], h2[8][32], d1[8][32], d2[8][32], dy[8][8];
    const int g = threadIdx.x >> 5, s = threadIdx.x & 31;
    const int i0 = blockIdx.x * 8, rows = min(8, N - i0);
    const int i = i0 + g;
    float pv[3] = {0.f, 0.f, 0.f};
    if (g < rows) {
#pragma unroll
        for (int x = 0; x < 3; ++x) pv[x] = p[(size_t)i * 96 + 32 * x + s];
        zin[g][s] = q[(size_t)i * S + s];
        zin[g][32 + s] = sqrtf(pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2]);
        if (s < 8) dy[g][s] = da[(size_t)i * 8 + s];
    }
    __syncthreads();
    const float nrm = g < rows ? zin[g][32 + s] : 0.0f;
    mlp3_hidden(W, sam, &zin[0][0], 64, &h1[0][0], &h2[0][0], rows);
    mlp3_bwd(W, G, sam, &zin[0][0], 64, &h1[0][0], &h2[0][0], &dy[0][0], 8, &d2[0][0], &d1[0][0], &zin[0][0], 64, rows);
    if (g < rows) {
        dq[(size_t)i * S + s] += zin[g][s];
        const float f = nrm > 0.0f ? zin[g][32 + s] / nrm : 0.0f;
#pragma unroll
        for (int x = 0; x < 3; ++x) dp[(size_t)i * 96 + 32 * x + s] += f * pv[x];
    }
}

// ---------------------------------------------------------------------------------------------- embed backward
// 8 atoms per workgroup: em forward again from q0, weight gradients from dq (state row i + 1). dq0_out (may be null) [N][n0] receives
// d q0 = d h1 . W_em.0, the gradient of the input features (the reference's q.requires_grad_(), model/model.py:34)
__global__ __launch_bounds__(256) void k_embed_bwd(const float* __restrict__ W, fx_t* __restrict__ G, MlpW em, int N, int n0,
                                                   const float* __restrict__ q0, const float* __restrict__ dq_state, float* __restrict__ dq0_out) {
    __shared__ float xs[8][512];
    __shared__ float h1[8][32], h2[8][32], d1[8][32], d2[8][32], dy[8][32];
    const int g = threadIdx.x >> 5, s = threadIdx.x & 31;
    const int i0 = blockIdx.x * 8, rows = min(8, N - i0);
    const int i = i0 + g;
    if (g < rows) {
        for (int k = s; k < n0; k += 32) xs[g][k] = q0[(size_t)i * n0 + k];
        dy[g][s] = dq_state[(size_t)(i + 1) * S + s];
    }
    __syncthreads();
    mlp3_hidden(W, em, &xs[0][0], 512, &h1[0][0], &h2[0][0], rows);
    mlp3_bwd(W, G, em, &xs[0][0], 512, &h1[0][0], &h2[0][0], &dy[0][0], 32, &d2[0][0], &d1[0][0], dq0_out ? &xs[0][0] : nullptr, 512, rows);
    if (dq0_out && g < rows)
        for (int k = s; k < n0; k += 32) dq0_out[(size_t)i * n0 + k] = xs[g][k];
}

// ---------------------------------------------------------------------------------------------- layer backward
// k_layer_v1 (pesto_kernels.hip) again with every activation kept in LDS, then its phases in reverse. One workgroup = 64 edge rows =
// A = 64 / NN centres. dq_out / dp_out: gradient of the layer's output state; the sink row's is multiplied by 0 (model_operations.py:
// 239-240), so centre 0 contributes nothing. dq_in / dp_in (zeroed before the launch) receive the residual, the centre features and,
// as a scatter-add, the gathered neighbour states; what the gather sends to row 0 dies there and is not written.
constexpr int LD = 68;      // row stride of the k-major LDS tiles (k_layer_v1)

struct LayerBwdSmem {
    float xe[129 * LD];    // varying part of X_e, k-major: 0 d | 1..32 q_j | 33..64 |p_j| | 65..96 p_i.r | 97..128 p_j.r ; then its gradient
    float h1[128 * LD];    // edge layer 1 activations; then the gradient of its pre-activations
    float h2[128 * LD];    // edge layer 2 likewise
    float kv[76 * LD];     // 0-2 Kq, 3-11 Kp (chunk-major), 12-43 V0, 44-75 V1; then their gradient
    float xn[8 * 64];      // centre node features [q_i | |p_i|]
    float pis[8 * 96];     // centre p_i
    float cpart[8 * 128];  // b1 + W1[:, 1:65] X_n(i); backward: scratch of the small MLPs, then the per-centre sums of d h1
    float4 geo[64];
    int nb[64];
    float nq1[8 * 32], nq2[8 * 32];   // nqm activations
    float qp1[8 * 32], qp2[8 * 32];   // qpm activations
    float Q[8 * 16], dQ[8 * 16];
    float lg[8 * 64];      // [h][part][row] attention weights
    float dl[8 * 64];      // softmax scratch; backward: d weights, then d logits (scaled by 1 / sdk)
    float zs[8 * 256];     // [centre][Zq | Zp_x | Zp_y | Zp_z][h*32+s]; then its gradient
    float dqz[8 * 32];     // gradient of the centres' output state
    float dpz[8 * 96];
};

// G[goff + rowmap(k) * ldw + o] += sum_r X[(xk0 + k) * LD + r] DY[(yo0 + o) * LD + r]   (k < kn, o < on), rowmap(k) = k + (k ? kskip : 0)
__device__ __forceinline__ void edge_wgrad(fx_t* __restrict__ G, int goff, int ldw, const float* X, int xk0, int kn, const float* DY, int yo0,
                                           int on, int kskip = 0) {
    const int n = kn * on;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int k = idx / on, o = idx - k * on;
        const float4* xr = reinterpret_cast<const float4*>(X + (xk0 + k) * LD);
        const float4* yr = reinterpret_cast<const float4*>(DY + (yo0 + o) * LD);
        float acc = 0.0f;
#pragma unroll
        for (int m4 = 0; m4 < 16; ++m4) {
            const float4 a = xr[m4], b = yr[m4];
            acc += a.x * b.x; acc += a.y * b.y; acc += a.z * b.z; acc += a.w * b.w;
        }
        gadd(G + goff + (k + (k ? kskip : 0)) * ldw + o, acc);
    }
}
// G[goff + o] += sum_r DY[o * LD + r], o < on
__device__ __forceinline__ void edge_bgrad(fx_t* __restrict__ G, int goff, const float* DY, int on) {
    if ((int)threadIdx.x < on) {
        const float4* yr = reinterpret_cast<const float4*>(DY + threadIdx.x * LD);
        double acc = 0.0;      // (the key biases' gradients are analytically zero: what is left of them is this sum's rounding)
#pragma unroll
        for (int m4 = 0; m4 < 16; ++m4) { const float4 b = yr[m4]; acc += b.x; acc += b.y; acc += b.z; acc += b.w; }
        gadd(G + goff + threadIdx.x, (float)acc);
    }
}

// GEO = true also forms the gradient of every edge's geometry, (d r^_x, d r^_y, d r^_z, d d), from the four places it enters the layer
// (src/model_operations.py:109-116, 131-136): the distance column of X_e, p_i.r^ and p_j.r^, and V[:,1] (x) r^ of Vp. It is staged per
// edge row in dgs (1 KB of LDS on top of LayerBwdSmem) and added into dgeo [(N+1)][KMAX]: a centre's slots belong to one workgroup and
// the stream runs layer after layer, so the read-add-write is plain and in a fixed order. GEO = false is the kernel without any of it.
template <int NN, bool GEO>
__global__ __launch_bounds__(256) void k_layer_v1_bwd(const float* __restrict__ W, fx_t* __restrict__ G, LayerW lw, int N1,
                                                      const int* __restrict__ ids_s, const float4* __restrict__ geo,
                                                      const float* __restrict__ q_in, const float* __restrict__ p_in,
                                                      const fx_t* __restrict__ dq_out, const fx_t* __restrict__ dp_out,
                                                      fx_t* __restrict__ dq_in, fx_t* __restrict__ dp_in, float4* __restrict__ dgeo) {
    constexpr int A = 64 / NN;
    __shared__ LayerBwdSmem sm;
    __shared__ float4 dgs[GEO ? 64 : 1];
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * A;
    const float sdk = sqrtf((float)NK);
    const int ca = t >> 5, cs = t & 31;                 // the (centre, state channel) role of a thread
    const int ci = c0 + ca;
    const bool cvalid = ca < A && ci < N1 && ci != 0;   // a centre whose output gradient counts

    // ================================================================== forward (phases of k_layer_v1)
    if (t < 64) {
        const int a = t / NN, c = t % NN, i = c0 + a;
        const bool valid = i < N1;
        sm.nb[t] = valid ? ids_s[(size_t)i * KMAX + c] : 0;
        sm.geo[t] = valid ? geo[(size_t)i * KMAX + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (ca < A) {
        const int i = min(ci, N1 - 1);
        const float qv = q_in[(size_t)i * S + cs];
        const float p0 = p_in[(size_t)i * 96 + cs], p1 = p_in[(size_t)i * 96 + 32 + cs], p2 = p_in[(size_t)i * 96 + 64 + cs];
        sm.xn[ca * 64 + cs] = qv;
        sm.xn[ca * 64 + 32 + cs] = sqrtf(p0 * p0 + p1 * p1 + p2 * p2);
        sm.pis[ca * 96 + cs] = p0; sm.pis[ca * 96 + 32 + cs] = p1; sm.pis[ca * 96 + 64 + cs] = p2;
        sm.dqz[ca * 32 + cs] = cvalid ? from_fx(dq_out[(size_t)ci * S + cs]) : 0.0f;
#pragma unroll
        for (int x = 0; x < 3; ++x) sm.dpz[ca * 96 + 32 * x + cs] = cvalid ? from_fx(dp_out[(size_t)ci * 96 + 32 * x + cs]) : 0.0f;
    }
    __syncthreads();
    {
        const int s = t & 31, rg = t >> 5;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int r = rg + 8 * it, a = r / NN;
            const int j = sm.nb[r];
            const float4 g = sm.geo[r];
            const float qj = q_in[(size_t)j * S + s];
            const float pj0 = p_in[(size_t)j * 96 + s], pj1 = p_in[(size_t)j * 96 + 32 + s], pj2 = p_in[(size_t)j * 96 + 64 + s];
            sm.xe[(1 + s) * LD + r] = qj;
            sm.xe[(33 + s) * LD + r] = sqrtf(pj0 * pj0 + pj1 * pj1 + pj2 * pj2);
            sm.xe[(65 + s) * LD + r] = sm.pis[a * 96 + s] * g.x + sm.pis[a * 96 + 32 + s] * g.y + sm.pis[a * 96 + 64 + s] * g.z;
            sm.xe[(97 + s) * LD + r] = pj0 * g.x + pj1 * g.y + pj2 * g.z;
            if (s == 0) sm.xe[r] = g.w;
        }
    }
    const int o = t & 127, rh = t >> 7;
    for (int a = rh; a < A; a += 2) {
        float acc = W[lw.b1 + o];
        for (int k = 0; k < 64; ++k) acc += sm.xn[a * 64 + k] * W[lw.w1 + (1 + k) * 128 + o];
        sm.cpart[a * 128 + o] = acc;
    }
    mlp3_hidden(W, lw.nqm, sm.xn, 64, sm.nq1, sm.nq2, A);      // (syncs: xe and cpart are complete behind it)
    if (ca < A && cs < 12) sm.Q[ca * 16 + cs] = lin_col(W, lw.nqm.l[2], sm.nq2 + ca * 32, cs);
    float acc[32];
    {   // edge layer 1
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = sm.cpart[((rh * 32 + m) / NN) * 128 + o];
        for (int k = 0; k < 129; ++k) {
            const float w = W[lw.w1 + (k == 0 ? 0 : 64 + k) * 128 + o];
            const float4* xr = reinterpret_cast<const float4*>(sm.xe + k * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.h1 + o * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4)
            hw[m4] = make_float4(elu(acc[4 * m4]), elu(acc[4 * m4 + 1]), elu(acc[4 * m4 + 2]), elu(acc[4 * m4 + 3]));
    }
    __syncthreads();
    // the block structure of edge layers 2 and 3 seen from column o (forward) / from input row o (backward)
    int kb2, kn2, ld2, oc2; const float* wp2;
    if (o < 32) { kb2 = 0; kn2 = 32; ld2 = 32; oc2 = o; wp2 = W + lw.w2eq; }
    else if (o < 64) { kb2 = 32; kn2 = 32; ld2 = 32; oc2 = o - 32; wp2 = W + lw.w2ep; }
    else { kb2 = 64; kn2 = 64; ld2 = 64; oc2 = o - 64; wp2 = W + lw.w2ev; }
    {   // edge layer 2
        const float b = W[lw.b2 + o];
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = b;
        for (int k = 0; k < kn2; ++k) {
            const float w = wp2[k * ld2 + oc2];
            const float4* xr = reinterpret_cast<const float4*>(sm.h1 + (kb2 + k) * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.h2 + o * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4)
            hw[m4] = make_float4(elu(acc[4 * m4]), elu(acc[4 * m4 + 1]), elu(acc[4 * m4 + 2]), elu(acc[4 * m4 + 3]));
    }
    __syncthreads();
    if (o < 76) {   // edge layer 3
        int kb, kn, ldw, oc; const float* wp;
        if (o < 3) { kb = 0; kn = 32; ldw = 3; oc = o; wp = W + lw.w3eq; }
        else if (o < 12) { kb = 32; kn = 32; ldw = 9; oc = o - 3; wp = W + lw.w3ep; }
        else { kb = 64; kn = 64; ldw = 64; oc = o - 12; wp = W + lw.w3ev; }
        const float b = W[lw.b3 + o];
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = b;
        for (int k = 0; k < kn; ++k) {
            const float w = wp[k * ldw + oc];
            const float4* xr = reinterpret_cast<const float4*>(sm.h2 + (kb + k) * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.kv + o * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) hw[m4] = make_float4(acc[4 * m4], acc[4 * m4 + 1], acc[4 * m4 + 2], acc[4 * m4 + 3]);
    }
    __syncthreads();
    float* kv = sm.kv;
    const int ar = t & 63, apart = t >> 6, aa = ar / NN, ag0 = aa * NN;     // the (row, part) role of the attention phases
    {   // logits and softmax (part 0: scalar keys over NN slots; parts 1..3 together over 3 NN slots)
        const int kr = apart == 0 ? 0 : 3 + (apart - 1) * 3;
        float l[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* Qv = sm.Q + aa * 16 + (apart ? 6 : 0) + h * 3;
            l[h] = (Qv[0] * kv[(kr + 0) * LD + ar] + Qv[1] * kv[(kr + 1) * LD + ar] + Qv[2] * kv[(kr + 2) * LD + ar]) / sdk;
            sm.lg[(h * 4 + apart) * 64 + ar] = l[h];
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float mx = -INFINITY;
            if (apart == 0) {
                for (int c = 0; c < NN; ++c) mx = fmaxf(mx, sm.lg[(h * 4) * 64 + ag0 + c]);
            } else {
                for (int pp = 1; pp < 4; ++pp)
                    for (int c = 0; c < NN; ++c) mx = fmaxf(mx, sm.lg[(h * 4 + pp) * 64 + ag0 + c]);
            }
            l[h] = expf(l[h] - mx);
            sm.dl[(h * 4 + apart) * 64 + ar] = l[h];
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float sum = 0.0f;
            if (apart == 0) {
                for (int c = 0; c < NN; ++c) sum += sm.dl[(h * 4) * 64 + ag0 + c];
            } else {
                for (int pp = 1; pp < 4; ++pp)
                    for (int c = 0; c < NN; ++c) sum += sm.dl[(h * 4 + pp) * 64 + ag0 + c];
            }
            sm.lg[(h * 4 + apart) * 64 + ar] = l[h] / sum;
        }
        __syncthreads();
    }
    {   // attention-weighted sums
        const int s = t & 31, h = (t >> 5) & 1, xq = t >> 6;
        for (int a = 0; a < A; ++a) {
            const int g0 = a * NN;
            float z = 0.0f;
            if (xq == 0) {
                for (int c = 0; c < NN; ++c) z += sm.lg[(h * 4) * 64 + g0 + c] * kv[(12 + s) * LD + g0 + c];
            } else {
                const int x = xq - 1;
                float wsum = 0.0f, z3 = 0.0f;
                for (int c = 0; c < NN; ++c) {
                    const int r = g0 + c;
                    const float4 g = sm.geo[r];
                    const float gx = x == 0 ? g.x : (x == 1 ? g.y : g.z);
                    z += sm.lg[(h * 4 + 1) * 64 + r] * (kv[(44 + s) * LD + r] * gx);
                    wsum += sm.lg[(h * 4 + 2) * 64 + r];
                    z3 += sm.lg[(h * 4 + 3) * 64 + r] * p_in[(size_t)sm.nb[r] * 96 + x * 32 + s];
                }
                z += wsum * sm.pis[a * 96 + x * 32 + s];
                z += z3;
            }
            sm.zs[a * 256 + xq * 64 + h * 32 + s] = z;
        }
    }
    __syncthreads();
    mlp3_hidden(W, lw.qpm, sm.zs, 256, sm.qp1, sm.qp2, A);

    // ================================================================== backward
    float* sc2 = sm.cpart;            // scratch of the small MLPs (cpart is free since edge layer 1)
    float* sc1 = sm.cpart + 256;
    float* dxn = sm.cpart + 512;      // [8][64]
    // what this thread adds to row ci of dq_in / dp_in: the residual, then the centre features
    float cq = sm.dqz[(ca < A ? ca : 0) * 32 + cs], cn = 0.0f, cp[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) cp[x] = sm.dpz[(ca < A ? ca : 0) * 96 + 32 * x + cs];
    // ---- output MLPs: qh = qpm(Zq), ph_x = ppm(Zp_x); zs becomes d zs
    mlp3_bwd(W, G, lw.qpm, sm.zs, 256, sm.qp1, sm.qp2, sm.dqz, 32, sc2, sc1, sm.zs, 256, A);
    for (int idx = t; idx < 64 * 32; idx += 256) {
        const int k = idx >> 5, oo = idx & 31;
        float v = 0.0f;
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int x = 0; x < 3; ++x) v += sm.zs[a * 256 + 64 * (1 + x) + k] * sm.dpz[a * 96 + 32 * x + oo];
        gadd(G + lw.ppm.w + idx, v);
    }
    __syncthreads();
    if (ca < A) {
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int k = cs + 32 * half;
                const float* w = W + lw.ppm.w + k * 32;
                float v = 0.0f;
                for (int oo = 0; oo < 32; ++oo) v += w[oo] * sm.dpz[ca * 96 + 32 * x + oo];
                sm.zs[ca * 256 + 64 * (1 + x) + k] = v;
            }
    }
    __syncthreads();
    // ---- attention: d weights
    {
        float dm[2] = {0.f, 0.f};
        const float4 g = sm.geo[ar];
        const float* dz = sm.zs + aa * 256;
        if (apart == 0) {
            for (int s = 0; s < 32; ++s) {
                const float v = kv[(12 + s) * LD + ar];
                dm[0] += dz[s] * v; dm[1] += dz[32 + s] * v;
            }
        } else {
            const int j = sm.nb[ar];
            float tg[3] = {0.f, 0.f, 0.f};      // GEO: the edge's term of Zp contracted with V1 instead of r^
            const float lg0 = sm.lg[(0 * 4 + 1) * 64 + ar], lg1 = sm.lg[(1 * 4 + 1) * 64 + ar];
            for (int x = 0; x < 3; ++x) {
                const float gx = x == 0 ? g.x : (x == 1 ? g.y : g.z);
                for (int s = 0; s < 32; ++s) {
                    float v;
                    if (apart == 1) {
                        v = kv[(44 + s) * LD + ar] * gx;
                        if constexpr (GEO) tg[x] += (lg0 * dz[64 * (1 + x) + s] + lg1 * dz[64 * (1 + x) + 32 + s]) * kv[(44 + s) * LD + ar];
                    }
                    else if (apart == 2) v = sm.pis[aa * 96 + 32 * x + s];
                    else v = p_in[(size_t)j * 96 + 32 * x + s];
                    dm[0] += dz[64 * (1 + x) + s] * v; dm[1] += dz[64 * (1 + x) + 32 + s] * v;
                }
            }
            if constexpr (GEO)
                if (apart == 1) dgs[ar] = make_float4(tg[0], tg[1], tg[2], 0.0f);
        }
        sm.dl[(0 * 4 + apart) * 64 + ar] = dm[0];
        sm.dl[(1 * 4 + apart) * 64 + ar] = dm[1];
        __syncthreads();
        // softmax: d logit = w (d w - sum w d w) / sdk. The float32 weights sum to 1 + a few units in the last place, and the d logits of
        // one softmax must sum to zero (the key biases' gradients are analytically zero): the mean is taken over the weights as they are,
        // sum w d w / sum w, and subtracted in double, so what is left of that sum is rounding relative to |d w - mean| and not to
        // |mean| (rows of equal edges - padding slots of a structure below k atoms - have d w = mean in every slot)
        float dlr[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double dot = 0.0, wsum = 0.0;
            if (apart == 0) {
                for (int c = 0; c < NN; ++c) {
                    const double w = sm.lg[(h * 4) * 64 + ag0 + c];
                    dot += w * sm.dl[(h * 4) * 64 + ag0 + c]; wsum += w;
                }
            } else {
                for (int pp = 1; pp < 4; ++pp)
                    for (int c = 0; c < NN; ++c) {
                        const double w = sm.lg[(h * 4 + pp) * 64 + ag0 + c];
                        dot += w * sm.dl[(h * 4 + pp) * 64 + ag0 + c]; wsum += w;
                    }
            }
            dlr[h] = sm.lg[(h * 4 + apart) * 64 + ar] * (float)((double)dm[h] - dot / wsum) / sdk;
        }
        __syncthreads();
        sm.dl[(0 * 4 + apart) * 64 + ar] = dlr[0];
        sm.dl[(1 * 4 + apart) * 64 + ar] = dlr[1];
        __syncthreads();
    }
    // ---- d Q (12 per centre), and the centre's own p through the second chunk of Vp
    if (ca < A) {
        const int g0 = ca * NN;
        if (cs < 12) {
            float v = 0.0f;
            if (cs < 6) {
                const int h = cs / 3, kap = cs % 3;
                for (int c = 0; c < NN; ++c) v += sm.dl[(h * 4) * 64 + g0 + c] * kv[kap * LD + g0 + c];
            } else {
                const int h = (cs - 6) / 3, kap = (cs - 6) % 3;
                for (int pp = 1; pp < 4; ++pp)
                    for (int c = 0; c < NN; ++c) v += sm.dl[(h * 4 + pp) * 64 + g0 + c] * kv[(3 + 3 * (pp - 1) + kap) * LD + g0 + c];
            }
            sm.dQ[ca * 16 + cs] = v;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float wsum = 0.0f;
            for (int c = 0; c < NN; ++c) wsum += sm.lg[(h * 4 + 2) * 64 + g0 + c];
#pragma unroll
            for (int x = 0; x < 3; ++x) cp[x] += wsum * sm.zs[ca * 256 + 64 * (1 + x) + h * 32 + cs];
        }
    }
    __syncthreads();
    // ---- d kv in place (keys from d logits and Q, values from the weights and d zs)
    if (o < 76) {
        float4* hw = reinterpret_cast<float4*>(kv + o * LD + rh * 32);
        float out[32];
#pragma unroll
        for (int m = 0; m < 32; ++m) {
            const int r = rh * 32 + m, a = r / NN;
            float v = 0.0f;
            if (o < 3) {
                v = sm.dl[(0) * 64 + r] * sm.Q[a * 16 + o] + sm.dl[(4) * 64 + r] * sm.Q[a * 16 + 3 + o];
            } else if (o < 12) {
                const int pp = 1 + (o - 3) / 3, kap = (o - 3) % 3;
                v = sm.dl[(pp) * 64 + r] * sm.Q[a * 16 + 6 + kap] + sm.dl[(4 + pp) * 64 + r] * sm.Q[a * 16 + 9 + kap];
            } else if (o < 44) {
                const int s = o - 12;
                v = sm.lg[(0) * 64 + r] * sm.zs[a * 256 + s] + sm.lg[(4) * 64 + r] * sm.zs[a * 256 + 32 + s];
            } else {
                const int s = o - 44;
                const float4 g = sm.geo[r];
                const float* dz = sm.zs + a * 256;
                const float d0 = dz[64 + s] * g.x + dz[128 + s] * g.y + dz[192 + s] * g.z;
                const float d1 = dz[64 + 32 + s] * g.x + dz[128 + 32 + s] * g.y + dz[192 + 32 + s] * g.z;
                v = sm.lg[(1) * 64 + r] * d0 + sm.lg[(4 + 1) * 64 + r] * d1;
            }
            out[m] = v;
        }
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) hw[m4] = make_float4(out[4 * m4], out[4 * m4 + 1], out[4 * m4 + 2], out[4 * m4 + 3]);
    }
    // ---- node query MLP: Q = nqm(X_n)
    mlp3_bwd(W, G, lw.nqm, sm.xn, 64, sm.nq1, sm.nq2, sm.dQ, 16, sc2, sc1, dxn, 64, A);      // (its first sync publishes d kv)
    if (ca < A) { cq += dxn[ca * 64 + cs]; cn += dxn[ca * 64 + 32 + cs]; }
    // ---- edge layer 3: weight gradients, then d h2 (pre-activation) in place
    edge_wgrad(G, lw.w3eq, 3, sm.h2, 0, 32, kv, 0, 3);
    edge_wgrad(G, lw.w3ep, 9, sm.h2, 32, 32, kv, 3, 9);
    edge_wgrad(G, lw.w3ev, 64, sm.h2, 64, 64, kv, 12, 64);
    edge_bgrad(G, lw.b3, kv, 76);
    __syncthreads();
    {
        int ob, on, ldw; const float* wp;      // input row o of layer 3 feeds the outputs [ob, ob + on)
        if (o < 32) { ob = 0; on = 3; ldw = 3; wp = W + lw.w3eq + o * 3; }
        else if (o < 64) { ob = 3; on = 9; ldw = 9; wp = W + lw.w3ep + (o - 32) * 9; }
        else { ob = 12; on = 64; ldw = 64; wp = W + lw.w3ev + (o - 64) * 64; }
        (void)ldw;
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = 0.0f;
        for (int k = 0; k < on; ++k) {
            const float w = wp[k];
            const float4* xr = reinterpret_cast<const float4*>(kv + (ob + k) * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.h2 + o * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) {
            const float4 a = hw[m4];
            hw[m4] = make_float4(acc[4 * m4] * elu_grad(a.x), acc[4 * m4 + 1] * elu_grad(a.y), acc[4 * m4 + 2] * elu_grad(a.z),
                                 acc[4 * m4 + 3] * elu_grad(a.w));
        }
    }
    __syncthreads();
    // ---- edge layer 2
    edge_wgrad(G, lw.w2eq, 32, sm.h1, 0, 32, sm.h2, 0, 32);
    edge_wgrad(G, lw.w2ep, 32, sm.h1, 32, 32, sm.h2, 32, 32);
    edge_wgrad(G, lw.w2ev, 64, sm.h1, 64, 64, sm.h2, 64, 64);
    edge_bgrad(G, lw.b2, sm.h2, 128);
    __syncthreads();
    {
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = 0.0f;
        const float* wp = wp2 + oc2 * ld2;      // input row o of layer 2: the row oc2 of its block, outputs [kb2, kb2 + kn2)
        for (int k = 0; k < kn2; ++k) {
            const float w = wp[k];
            const float4* xr = reinterpret_cast<const float4*>(sm.h2 + (kb2 + k) * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.h1 + o * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) {
            const float4 a = hw[m4];
            hw[m4] = make_float4(acc[4 * m4] * elu_grad(a.x), acc[4 * m4 + 1] * elu_grad(a.y), acc[4 * m4 + 2] * elu_grad(a.z),
                                 acc[4 * m4 + 3] * elu_grad(a.w));
        }
    }
    __syncthreads();
    // ---- edge layer 1: the varying rows (image rows 0 and 65..192), the bias, and the centre rows 1..64 through per-centre sums
    edge_wgrad(G, lw.w1, 128, sm.xe, 0, 129, sm.h1, 0, 128, 64);
    edge_bgrad(G, lw.b1, sm.h1, 128);
    for (int a = rh; a < A; a += 2) {
        float v = 0.0f;
        for (int c = 0; c < NN; ++c) v += sm.h1[o * LD + a * NN + c];
        sm.cpart[a * 128 + o] = v;
    }
    __syncthreads();
    for (int idx = t; idx < 64 * 128; idx += 256) {
        const int k = idx >> 7, oo = idx & 127;
        float v = 0.0f;
        for (int a = 0; a < A; ++a) v += sm.xn[a * 64 + k] * sm.cpart[a * 128 + oo];
        gadd(G + lw.w1 + (1 + k) * 128 + oo, v);
    }
    if (ca < A) {
        const float* w0 = W + lw.w1 + (1 + cs) * 128;
        const float* w1 = W + lw.w1 + (33 + cs) * 128;
        float v0 = 0.0f, v1 = 0.0f;
        for (int oo = 0; oo < 128; ++oo) { const float c = sm.cpart[ca * 128 + oo]; v0 += w0[oo] * c; v1 += w1[oo] * c; }
        cq += v0; cn += v1;
    }
    if constexpr (GEO) {   // row 0 of d xe, the distance: sum_k W1[0][k] d h1[k][edge] (dgs[t].xyz was written in the attention phase)
        if (t < 64) {
            float v = 0.0f;
            for (int k = 0; k < 128; ++k) v += W[lw.w1 + k] * sm.h1[k * LD + t];
            dgs[t].w = v;
        }
    }
    {   // d xe in place: row 1 + o (row 0, the distance, is formed above and only under GEO)
        const float* wr = W + lw.w1 + (65 + o) * 128;
#pragma unroll
        for (int m = 0; m < 32; ++m) acc[m] = 0.0f;
        for (int k = 0; k < 128; ++k) {
            const float w = wr[k];
            const float4* xr = reinterpret_cast<const float4*>(sm.h1 + k * LD + rh * 32);
#pragma unroll
            for (int m4 = 0; m4 < 8; ++m4) {
                const float4 v = xr[m4];
                acc[4 * m4 + 0] += v.x * w; acc[4 * m4 + 1] += v.y * w; acc[4 * m4 + 2] += v.z * w; acc[4 * m4 + 3] += v.w * w;
            }
        }
        float4* hw = reinterpret_cast<float4*>(sm.xe + (1 + o) * LD + rh * 32);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) hw[m4] = make_float4(acc[4 * m4], acc[4 * m4 + 1], acc[4 * m4 + 2], acc[4 * m4 + 3]);
    }
    __syncthreads();      // (every edge_wgrad read of xe is in front of the previous sync)
    // ---- the gather as a scatter-add: q_j, |p_j|, p_j.r and the third chunk of Vp
    {
        const int s = t & 31, rg = t >> 5;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int r = rg + 8 * it, a = r / NN, i = c0 + a;
            const int j = sm.nb[r];
            if constexpr (GEO) {   // p_i.r^ and p_j.r^: rows 65..128 of d xe times p_i / p_j, summed over the 32 channels of the row
                const bool iv = i < N1 && i != 0;      // (a padded slot, j == 0, has a real geometry: X[-1], model_operations.py:8)
                float gv[3];
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    gv[x] = iv ? sm.xe[(65 + s) * LD + r] * sm.pis[a * 96 + 32 * x + s] + sm.xe[(97 + s) * LD + r] * p_in[(size_t)j * 96 + 32 * x + s] : 0.0f;
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    for (int off = 16; off > 0; off >>= 1) gv[x] += __shfl_xor(gv[x], off);      // (within the row's 32 lanes)
                if (iv && s == 0) {
                    const float4 d = dgs[r];
                    float4* gp = dgeo + (size_t)i * KMAX + (r - a * NN);
                    float4 acc4 = *gp;
                    acc4.x += d.x + gv[0]; acc4.y += d.y + gv[1]; acc4.z += d.z + gv[2]; acc4.w += d.w;
                    *gp = acc4;
                }
            }
            if (i >= N1 || i == 0 || j == 0) continue;
            const float4 g = sm.geo[r];
            const float pj[3] = {p_in[(size_t)j * 96 + s], p_in[(size_t)j * 96 + 32 + s], p_in[(size_t)j * 96 + 64 + s]};
            const float nrm = sqrtf(pj[0] * pj[0] + pj[1] * pj[1] + pj[2] * pj[2]);
            const float fn = nrm > 0.0f ? sm.xe[(33 + s) * LD + r] / nrm : 0.0f;
            const float gpr = sm.xe[(97 + s) * LD + r];
            const float w0 = sm.lg[(3) * 64 + r], w1 = sm.lg[(4 + 3) * 64 + r];
            gadd(dq_in + (size_t)j * S + s, sm.xe[(1 + s) * LD + r]);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const float gx = x == 0 ? g.x : (x == 1 ? g.y : g.z);
                const float v = fn * pj[x] + gpr * gx + w0 * sm.zs[a * 256 + 64 * (1 + x) + s] + w1 * sm.zs[a * 256 + 64 * (1 + x) + 32 + s];
                gadd(dp_in + (size_t)j * 96 + 32 * x + s, v);
            }
        }
    }
    // ---- the centre's row: p_i.r, |p_i|, and what was collected above
    if (cvalid) {
        const int g0 = ca * NN;
        for (int c = 0; c < NN; ++c) {
            const float4 g = sm.geo[g0 + c];
            const float v = sm.xe[(65 + cs) * LD + g0 + c];
            cp[0] += v * g.x; cp[1] += v * g.y; cp[2] += v * g.z;
        }
        const float nrm = sm.xn[ca * 64 + 32 + cs];
        const float fn = nrm > 0.0f ? cn / nrm : 0.0f;
        gadd(dq_in + (size_t)ci * S + cs, cq);
#pragma unroll
        for (int x = 0; x < 3; ++x) gadd(dp_in + (size_t)ci * 96 + 32 * x + cs, cp[x] + fn * sm.pis[ca * 96 + 32 * x + cs]);
    }
}

template <bool GEO>
void launch_layer_v1_bwd_geo(hipStream_t st, const float* W, fx_t* G, const LayerW& lw, int N1, const int* ids_s, const float4* geo, const float* q_in,
                             const float* p_in, const fx_t* dq_out, const fx_t* dp_out, fx_t* dq_in, fx_t* dp_in, float4* dgeo) {
    const int A = 64 / lw.nn;
    const dim3 grid((N1 + A - 1) / A), block(256);
    switch (lw.nn) {
        case 8: hipLaunchKernelGGL((k_layer_v1_bwd<8, GEO>), grid, block, 0, st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, dgeo); break;
        case 16: hipLaunchKernelGGL((k_layer_v1_bwd<16, GEO>), grid, block, 0, st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, dgeo); break;
        case 32: hipLaunchKernelGGL((k_layer_v1_bwd<32, GEO>), grid, block, 0, st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, dgeo); break;
        default: hipLaunchKernelGGL((k_layer_v1_bwd<64, GEO>), grid, block, 0, st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, dgeo); break;
    }
}
// dgeo == nullptr: parameter and state gradients only (the instantiation the training step runs)
void launch_layer_v1_bwd(hipStream_t st, const float* W, fx_t* G, const LayerW& lw, int N1, const int* ids_s, const float4* geo, const float* q_in,
                         const float* p_in, const fx_t* dq_out, const fx_t* dp_out, fx_t* dq_in, fx_t* dp_in, float4* dgeo = nullptr) {
    if (dgeo) launch_layer_v1_bwd_geo<true>(st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, dgeo);
    else launch_layer_v1_bwd_geo<false>(st, W, G, lw, N1, ids_s, geo, q_in, p_in, dq_out, dp_out, dq_in, dp_in, nullptr);
}

// ---------------------------------------------------------------------------------------------- geometry backward
// Backward of unpack_state_features (src/model_operations.py:8-14) from dgeo, one thread per (atom, slot). With r = X_j - X_i, D0 = |r|,
// D = D0 + m [D0 < 1e-2], m = max D0 over the call and r^ = r / D:
//   d D  = d d - (d r^ . r^) / D            (the distance column, and D as the divisor of r^)
//   d r  = d r^ / D + d D r / D0            (d|r|/dr = 0 at r = 0, torch's convention)
//   d m  = sum over the fix-up edges of d D (fixed-point atomic), handed to the maximal edges by k_unpack_bwd_max
// +d r goes to X_j and -d r to X_i; j follows the forward's rule (a zero id is the call's last atom). r, D0 and the fix-up decision
// come from pesto_geom.h, which restates k_unpack1 / k_unpack2 operation for operation, so the mask is the forward's. dX is 64-bit
// fixed point: a repeated call gives the same bits.
__global__ __launch_bounds__(256) void k_unpack_bwd(int N, const float* __restrict__ X, const int* __restrict__ ids_s, const float4* __restrict__ dgeo,
                                                    const unsigned* __restrict__ dmax_bits, fx_t* __restrict__ dX, fx_t* __restrict__ dm,
                                                    int* __restrict__ n_max) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * KMAX) return;      // (a wave = the 64 slots of one atom: it leaves as a whole)
    const int i = (int)(e >> 6), c = (int)(e & 63);
    const int id = ids_s[(size_t)(i + 1) * KMAX + c];
    const int j = id > 0 ? id - 1 : N - 1;
    float rx, ry, rz;
    const float d0 = edge_vec(X + (size_t)3 * j, X + (size_t)3 * i, rx, ry, rz);
    const unsigned mb = dmax_bits[0];
    const bool fix = edge_fixup(d0);
    const float D = edge_dist(d0, __uint_as_float(mb));
    const float4 g = dgeo[(size_t)(i + 1) * KMAX + c];
    const float dD = g.w - (g.x * (rx / D) + g.y * (ry / D) + g.z * (rz / D)) / D;
    const float f = d0 > 0.0f ? dD / d0 : 0.0f;
    float dr[3] = {g.x / D + f * rx, g.y / D + f * ry, g.z / D + f * rz};
    if (fix) gadd(dm, dD);
    if (d0 > 0.0f && __float_as_uint(d0) == mb) atomicAdd(n_max, 1);
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        gadd(dX + (size_t)3 * j + x, dr[x]);
        float sum = dr[x];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (c == 0) gadd(dX + (size_t)3 * i + x, -sum);
    }
}
// m = max D0: d m is split evenly over the maximal edges (torch.max's backward). The fixtures contain one maximal edge or the two
// directions of one pair, for which every split gives the same dX; other ties are not defined by the reference's gradient.
__global__ __launch_bounds__(256) void k_unpack_bwd_max(int N, const float* __restrict__ X, const int* __restrict__ ids_s,
                                                        const unsigned* __restrict__ dmax_bits, fx_t* __restrict__ dX, const fx_t* __restrict__ dm,
                                                        const int* __restrict__ n_max) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * KMAX) return;
    const int i = (int)(e >> 6), c = (int)(e & 63);
    const int id = ids_s[(size_t)(i + 1) * KMAX + c];
    const int j = id > 0 ? id - 1 : N - 1;
    float rx, ry, rz;
    const float d0 = edge_vec(X + (size_t)3 * j, X + (size_t)3 * i, rx, ry, rz);
    if (!(d0 > 0.0f) || __float_as_uint(d0) != dmax_bits[0]) return;
    const float f = from_fx(dm[0]) / (float)n_max[0] / d0;
    const float dr[3] = {f * rx, f * ry, f * rz};
#pragma unroll
    for (int x = 0; x < 3; ++x) { gadd(dX + (size_t)3 * j + x, dr[x]); gadd(dX + (size_t)3 * i + x, -dr[x]); }
}

// ---------------------------------------------------------------------------------------------- blob order <-> image layout, Adam
__global__ __launch_bounds__(256) void k_gather_grads(int64_t n, const int* __restrict__ map, const fx_t* __restrict__ Gimg, float* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] = from_fx(Gimg[map[i]]);
}
// the inverse direction: the plain section of the weight image from a blob (pesto_train_set_weights)
__global__ __launch_bounds__(256) void k_scatter_weights(int64_t n, const int* __restrict__ map, const float* __restrict__ w, float* __restrict__ Wimg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) Wimg[map[i]] = w[i];
}
__global__ __launch_bounds__(256) void k_to_fixed(int64_t n, const float* __restrict__ a, fx_t* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) b[i] = to_fx(a[i]);
}
__global__ __launch_bounds__(256) void k_to_float(int64_t n, const fx_t* __restrict__ a, float* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) b[i] = from_fx(a[i]);
}
// torch.optim.Adam (defaults) over the flat blob; the plain section of the weight image is refreshed along the way.
// c1 = lr / (1 - beta1^t), c2 = 1 / sqrt(1 - beta2^t)
__global__ __launch_bounds__(256) void k_adam(int64_t n, const int* __restrict__ map, const float* __restrict__ g, float* __restrict__ w,
                                              float* __restrict__ m, float* __restrict__ v, float* __restrict__ Wimg, float c1, float c2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // torch hands 1 - beta over as a double rounded to float32 once: 1.0f - 0.999f would be off by 1.3e-5 of itself
    constexpr float omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999);
    const float gi = g[i];
    const float mi = m[i] + (gi - m[i]) * omb1;
    const float vi = v[i] * 0.999f + omb2 * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) * c2 + 1e-8f;
    const float wi = w[i] - c1 * (mi / denom);
    w[i] = wi;
    Wimg[map[i]] = wi;
}

// Where every float of the host blob sits in the PLAIN section of the device image (the transposed Linears and the concatenated edge
// layers the exact fp32 kernels read): out[i] = image offset of blob[i], empty on failure. Derived from build_device_image itself - the
// image of a blob that holds its own indices (i + 1, exact in float32 below 2^24) is read back - so the layout stays stated once, in
// pesto_schema.cpp. The plain section is the model-level block in front of the first layer and [w1, e_lds) of every layer; the MFMA
// tables behind them hold scaled copies.
std::vector<int32_t> blob_to_plain_image(const pesto_config& c) {
    const HostSchema h = host_schema(c);
    if (h.total >= (1 << 24)) return {};
    std::vector<int32_t> out((size_t)h.total, -1);
    std::vector<float> idx((size_t)h.total);
    for (int64_t i = 0; i < h.total; ++i) idx[i] = (float)(i + 1);
    const DeviceImage d = build_device_image(c, idx.data());
    auto scan = [&](int32_t lo, int32_t hi) {
        for (int32_t pos = lo; pos < hi; ++pos) {
            const int64_t i = (int64_t)d.data[pos] - 1;
            if (i >= 0 && i < h.total && d.data[pos] == (float)(i + 1) && out[i] < 0) out[i] = pos;
        }
    };
    scan(0, d.layers[0].w1);
    for (const LayerW& L : d.layers) scan(L.w1, L.e_lds);
    for (int32_t v : out)
        if (v < 0) return {};
    return out;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return 1; }
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

}  // namespace
}  // namespace pesto

using namespace pesto;

struct pesto_trainer {
    pesto_config cfg;
    int device = 0;
    float lr = 1e-5f, f = 0.5f;
    int64_t n_weights = 0, global_step = 0, adam_t = 0;
    size_t img_floats = 0;
    ModelW model;
    std::vector<LayerW> layers;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timing = false, timed = false;
    DevBuf W, G, blob, am, av, gblob, map, pos, flags;
    // per-call workspace
    DevBuf sq, sp, ids_s, geo, dmax, a_tmp, seg, z, dz, st, qh, ph, da, dqa, dpa, dqb, dpb, fq, fp;
    DevBuf in_X, in_ids, in_q0, in_roa, in_y, out_l, out_p;
    DevBuf dgeo, dxf, gmax, out_dq0, out_dx;      // input gradients (pesto_train_backward)
    // the kept forward a backward may follow (pesto_train_forward with keep != 0): valid == 0 means none. The pointers are the caller's
    // device arrays or the handle's staging copies.
    struct Kept {
        int64_t valid = 0, N = 0, R = 0;
        const float* X = nullptr;
        const float* q0 = nullptr;
        const int32_t* roa = nullptr;
    } kept;
    int64_t tickets = 0;
    void release() {
        for (DevBuf* b : {&W, &G, &blob, &am, &av, &gblob, &map, &pos, &flags, &sq, &sp, &ids_s, &geo, &dmax, &a_tmp, &seg, &z, &dz, &st, &qh, &ph,
                          &da, &dqa, &dpa, &dqb, &dpb, &fq, &fp, &in_X, &in_ids, &in_q0, &in_roa, &in_y, &out_l, &out_p, &dgeo, &dxf, &gmax,
                          &out_dq0, &out_dx})
            b->release();
        for (hipEvent_t& e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    }
};

namespace {

#define TRY_HIP(expr) do { if (int rc_ = hip_ok((expr), #expr)) return rc_; } while (0)

int* err_ptr(pesto_trainer* t) { return t->flags.as<int>() + 1; }

int check_trainer(pesto_trainer* t) {
    if (!t) return fail(PESTO_ERR_INVALID, "null trainer handle");
    return hip_ok(hipSetDevice(t->device), "hipSetDevice");
}

int ensure_state(pesto_trainer* t, int64_t N, int64_t R, int n_states) {
    const size_t N1 = (size_t)N + 1;
    const int C = t->cfg.n_out;
    int bad = 0;
    bad |= t->sq.ensure((size_t)n_states * N1 * S * 4) | t->sp.ensure((size_t)n_states * N1 * 96 * 4);
    bad |= t->ids_s.ensure(N1 * KMAX * 4) | t->geo.ensure(N1 * KMAX * 16) | t->dmax.ensure(256);
    bad |= t->a_tmp.ensure((size_t)N * 8 * 4) | t->da.ensure((size_t)N * 8 * 4) | t->seg.ensure((size_t)R * 2 * 4);
    bad |= t->z.ensure((size_t)R * C * 4) | t->dz.ensure((size_t)R * C * 4) | t->st.ensure((size_t)R * 16 * 4);
    bad |= t->qh.ensure((size_t)R * 128 * 4) | t->ph.ensure((size_t)R * 384 * 4);
    bad |= t->dqa.ensure(N1 * S * 8) | t->dpa.ensure(N1 * 96 * 8) | t->dqb.ensure(N1 * S * 8) | t->dpb.ensure(N1 * 96 * 8);      // (fixed point)
    bad |= t->fq.ensure(N1 * S * 4) | t->fp.ensure(N1 * 96 * 4);
    return bad ? fail(PESTO_ERR_NOMEM, "workspace allocation failed (N = %lld, R = %lld)", (long long)N, (long long)R) : 0;
}

// geometry of the call (src/model_operations.py:6-22); ids are known to be in range
int run_unpack(pesto_trainer* t, hipStream_t st, int64_t N, int k, const float* X, const void* ids, int ids_kind) {
    TRY_HIP(hipMemsetAsync(t->flags.p, 0, 256, st));
    TRY_HIP(hipMemsetAsync(t->dmax.p, 0, 256, st));
    launch_unpack(st, (int)N, 1, k, X, 3 * N, 3, ids, ids_kind, t->ids_s.as<int>(), t->geo.as<float4>(), t->dmax.as<unsigned>(), err_ptr(t));
    return 0;
}

void to_fixed(hipStream_t st, size_t n, const float* a, fx_t* b) {
    hipLaunchKernelGGL(k_to_fixed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int64_t)n, a, b);
}
void to_float(hipStream_t st, size_t n, const fx_t* a, float* b) {
    hipLaunchKernelGGL(k_to_float, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int64_t)n, a, b);
}

// backward of pool + dm from dz: leaves d q / d p of the last state in fq / fp (float; rows 1..N, row 0 zero) and in dqa / dpa (fixed point)
void run_head_bwd(pesto_trainer* t, hipStream_t st, int64_t N, int64_t R, const float* q, const float* p, const int* roa) {
    const size_t N1 = (size_t)N + 1;
    int* lo = t->seg.as<int>();
    int* hi = lo + R;
    (void)hipMemsetAsync(t->fq.p, 0, N1 * S * 4, st);
    (void)hipMemsetAsync(t->fp.p, 0, N1 * 96 * 4, st);
    hipLaunchKernelGGL(k_head_pool, dim3((unsigned)R), dim3(64), 0, st, (int)R, q, p, t->a_tmp.as<float>(), roa, lo, hi, t->st.as<float>(),
                       t->qh.as<float>(), t->ph.as<float>());
    hipLaunchKernelGGL(k_head_decode_bwd, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, st, t->W.as<float>(), t->G.as<fx_t>(), t->model, t->cfg.n_out,
                       (int)R, t->dz.as<float>(), t->qh.as<float>(), t->ph.as<float>());
    hipLaunchKernelGGL(k_head_pool_bwd, dim3((unsigned)R), dim3(64), 0, st, (int)R, q, p, t->a_tmp.as<float>(), roa, lo, hi, t->st.as<float>(),
                       t->qh.as<float>(), t->ph.as<float>(), t->fq.as<float>() + S, t->fp.as<float>() + 96, t->da.as<float>());
    hipLaunchKernelGGL(k_head_sam_bwd, dim3((unsigned)((N + 7) / 8)), dim3(256), 0, st, t->W.as<float>(), t->G.as<fx_t>(), t->model.sam, (int)N, q, p,
                       t->da.as<float>(), t->fq.as<float>() + S, t->fp.as<float>() + 96);
    to_fixed(st, N1 * S, t->fq.as<float>(), t->dqa.as<fx_t>());
    to_fixed(st, N1 * 96, t->fp.as<float>(), t->dpa.as<fx_t>());
}

int gather_grads(pesto_trainer* t, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_grads, dim3((unsigned)((t->n_weights + 255) / 256)), dim3(256), 0, st, t->n_weights, t->map.as<int>(), t->G.as<fx_t>(),
                       t->gblob.as<float>());
    return hip_ok(hipGetLastError(), "gradient gather");
}

int run_adam(pesto_trainer* t, hipStream_t st) {
    t->adam_t += 1;
    const double c1 = (double)t->lr / (1.0 - std::pow(0.9, (double)t->adam_t));
    const double c2 = 1.0 / std::sqrt(1.0 - std::pow(0.999, (double)t->adam_t));
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((t->n_weights + 255) / 256)), dim3(256), 0, st, t->n_weights, t->map.as<int>(), t->gblob.as<float>(),
                       t->blob.as<float>(), t->am.as<float>(), t->av.as<float>(), t->W.as<float>(), (float)c1, (float)c2);
    return hip_ok(hipGetLastError(), "Adam update");
}

// the stage entry points work on a zeroed gradient buffer and hand it out in blob order
int stage_finish(pesto_trainer* t, hipStream_t st, float* grads_out) {
    if (int rc = gather_grads(t, st)) return rc;
    if (grads_out) TRY_HIP(hipMemcpyAsync(grads_out, t->gblob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    return 0;
}

// ---- the pieces pesto_train_step, pesto_train_forward and pesto_train_backward share
struct CallIn {
    const float* X;
    const void* ids;
    const float* q0;
    const int32_t* roa;
};

int check_call_args(int64_t N, int64_t R, int32_t k, int32_t ids_kind, const CallIn& in, int32_t ptr_kind) {
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (N < 1 || R < 1 || N > (1 << 24) || R > N || k < 1 || k > KMAX) return fail(PESTO_ERR_INVALID, "need 1 <= R <= N <= 2^24 and 1 <= k <= %d", KMAX);
    if (ids_kind != PESTO_IDS_INT32 && ids_kind != PESTO_IDS_INT64) return fail(PESTO_ERR_INVALID, "ids_kind must be 32 or 64");
    if (!in.X || !in.ids || !in.q0 || !in.roa) return fail(PESTO_ERR_INVALID, "null input");
    return 0;
}

// host pointers: the inputs are copied to the handle's staging buffers, and `in` then names those
int stage_inputs(pesto_trainer* t, hipStream_t st, int64_t N, int32_t k, int32_t ids_kind, CallIn& in) {
    const int n0 = t->cfg.n0;
    const size_t id_sz = ids_kind == PESTO_IDS_INT64 ? 8 : 4;
    if (t->in_X.ensure((size_t)N * 12) || t->in_ids.ensure((size_t)N * k * id_sz) || t->in_q0.ensure((size_t)N * n0 * 4) || t->in_roa.ensure((size_t)N * 4))
        return fail(PESTO_ERR_NOMEM, "staging allocation failed");
    TRY_HIP(hipMemcpyAsync(t->in_X.p, in.X, (size_t)N * 12, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->in_ids.p, in.ids, (size_t)N * k * id_sz, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->in_q0.p, in.q0, (size_t)N * n0 * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->in_roa.p, in.roa, (size_t)N * 4, hipMemcpyHostToDevice, st));
    in.X = t->in_X.as<float>(); in.ids = t->in_ids.p; in.q0 = t->in_q0.as<float>(); in.roa = t->in_roa.as<int32_t>();
    return 0;
}

// the argument check on the device, read back before anything else is launched; also finds the residue segments (t->seg)
int check_on_device(pesto_trainer* t, hipStream_t st, int64_t N, int64_t R, int32_t k, int32_t ids_kind, const CallIn& in) {
    int* lo = t->seg.as<int>();
    int* hi = lo + R;
    TRY_HIP(hipMemsetAsync(t->flags.p, 0, 256, st));
    TRY_HIP(hipMemsetAsync(t->seg.p, 0, (size_t)R * 8, st));
    const int64_t n = std::max<int64_t>(N * k, N);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (ids_kind == PESTO_IDS_INT64)
        hipLaunchKernelGGL(k_train_check<long long>, grid, dim3(256), 0, st, (int)N, (int)R, k, (const long long*)in.ids, in.roa, lo, hi, err_ptr(t));
    else
        hipLaunchKernelGGL(k_train_check<int>, grid, dim3(256), 0, st, (int)N, (int)R, k, (const int*)in.ids, in.roa, lo, hi, err_ptr(t));
    hipLaunchKernelGGL(k_train_check_empty, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, (int)R, hi, err_ptr(t));
    int flag = 0;
    TRY_HIP(hipMemcpyAsync(&flag, err_ptr(t), 4, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    if (flag & 1) return fail(PESTO_ERR_INVALID, "ids_topk holds an id outside [0, N]");
    if (flag & 2) return fail(PESTO_ERR_INVALID, "res_of_atom holds a residue outside [0, R)");
    if (flag & 4) return fail(PESTO_ERR_INVALID, "a residue has no atom");
    return 0;
}

// state l of a kept forward is slot l; without keeping, the layers run on two ping-pong slots
inline int state_slot(bool keep, int l) { return keep ? l : (l & 1); }

// the training forward (k_embed, k_unpack*, k_layer_v1, pool): logits in t->z. keep: every layer's input state stays (L + 1 slots)
int run_forward(pesto_trainer* t, hipStream_t st, int64_t N, int64_t R, int32_t k, int32_t ids_kind, const CallIn& in, bool keep) {
    const int L = t->cfg.n_layers;
    const size_t N1 = (size_t)N + 1;
    float* sq = t->sq.as<float>();
    float* sp = t->sp.as<float>();
    const float* W = t->W.as<float>();
    int* lo = t->seg.as<int>();
    launch_embed(st, W, t->model.em, (int)N, (int)N, t->cfg.n0, in.q0, sq, sp);
    // (the argument check has drained the stream, so the flags word may be cleared again for the geometry pass)
    if (int rc = run_unpack(t, st, N, k, in.X, in.ids, ids_kind)) return rc;
    for (int l = 0; l < L; ++l) {
        const size_t a = (size_t)state_slot(keep, l), b = (size_t)state_slot(keep, l + 1);
        launch_layer_v1(st, W, t->layers[l], (int)N1, t->ids_s.as<int>(), t->geo.as<float4>(), sq + a * N1 * S, sp + a * N1 * 96, sq + b * N1 * S,
                        sp + b * N1 * 96);
    }
    const size_t last = (size_t)state_slot(keep, L);
    launch_pool(st, W, t->model, t->cfg.n_out, (int)N, (int)R, sq + last * N1 * S + S, sp + last * N1 * 96 + 96, in.roa, t->a_tmp.as<float>(), lo, lo + R,
                err_ptr(t), nullptr, nullptr, t->z.as<float>(), true);
    return 0;
}

// the backward of a kept forward from t->dz: parameter gradients in t->gblob (blob order). dq0 (device, may be null) [N][n0];
// want_dx: d X is left in t->dxf (fixed point, [N][3])
int run_backward(pesto_trainer* t, hipStream_t st, int64_t N, int64_t R, const float* X, const float* q0, const int32_t* roa, float* dq0, bool want_dx) {
    const int L = t->cfg.n_layers;
    const size_t N1 = (size_t)N + 1;
    const float* sq = t->sq.as<float>();
    const float* sp = t->sp.as<float>();
    const float* W = t->W.as<float>();
    TRY_HIP(hipMemsetAsync(t->G.p, 0, t->img_floats * 8, st));
    run_head_bwd(t, st, N, R, sq + (size_t)L * N1 * S + S, sp + (size_t)L * N1 * 96 + 96, roa);
    float4* dgeo = want_dx ? t->dgeo.as<float4>() : nullptr;
    if (want_dx) TRY_HIP(hipMemsetAsync(t->dgeo.p, 0, N1 * KMAX * 16, st));
    fx_t *dqo = t->dqa.as<fx_t>(), *dpo = t->dpa.as<fx_t>(), *dqi = t->dqb.as<fx_t>(), *dpi = t->dpb.as<fx_t>();
    for (int l = L - 1; l >= 0; --l) {
        TRY_HIP(hipMemsetAsync(dqi, 0, N1 * S * 8, st));
        TRY_HIP(hipMemsetAsync(dpi, 0, N1 * 96 * 8, st));
        launch_layer_v1_bwd(st, W, t->G.as<fx_t>(), t->layers[l], (int)N1, t->ids_s.as<int>(), t->geo.as<float4>(), sq + (size_t)l * N1 * S,
                            sp + (size_t)l * N1 * 96, dqo, dpo, dqi, dpi, dgeo);
        std::swap(dqo, dqi); std::swap(dpo, dpi);
    }
    to_float(st, N1 * S, dqo, t->fq.as<float>());
    hipLaunchKernelGGL(k_embed_bwd, dim3((unsigned)((N + 7) / 8)), dim3(256), 0, st, W, t->G.as<fx_t>(), t->model.em, (int)N, t->cfg.n0, q0, t->fq.as<float>(),
                       dq0);
    if (want_dx) {
        const dim3 grid((unsigned)(((size_t)N * KMAX + 255) / 256));
        TRY_HIP(hipMemsetAsync(t->dxf.p, 0, (size_t)N * 3 * 8, st));
        TRY_HIP(hipMemsetAsync(t->gmax.p, 0, 256, st));
        fx_t* dm = t->gmax.as<fx_t>();
        int* n_max = t->gmax.as<int>() + 4;
        hipLaunchKernelGGL(k_unpack_bwd, grid, dim3(256), 0, st, (int)N, X, t->ids_s.as<int>(), dgeo, t->dmax.as<unsigned>(), t->dxf.as<fx_t>(), dm, n_max);
        hipLaunchKernelGGL(k_unpack_bwd_max, grid, dim3(256), 0, st, (int)N, X, t->ids_s.as<int>(), t->dmax.as<unsigned>(), t->dxf.as<fx_t>(), dm, n_max);
    }
    return gather_grads(t, st);
}

}  // namespace

extern "C" {

const char* pesto_train_last_error(void) { return last_error(); }

int pesto_train_create(const pesto_config* cfg, const float* weights, int64_t n_weights, int device, float lr, float pos_weight_factor,
                       pesto_trainer** out) {
    if (out) *out = nullptr;
    if (!config_ok(cfg)) return fail(PESTO_ERR_INVALID, "invalid pesto_config");
    if (!weights || !out) return fail(PESTO_ERR_INVALID, "null argument");
    if (cfg->em_depth != 3 || cfg->dm_depth != 3)
        return fail(PESTO_ERR_INVALID, "training needs the three-Linear em and dm (em_depth = dm_depth = 3); single-Linear variants are not supported");
    if (!(lr >= 0.0f)) return fail(PESTO_ERR_INVALID, "lr must be >= 0");
    const HostSchema h = host_schema(*cfg);
    if (n_weights != h.total) return fail(PESTO_ERR_INVALID, "weight blob has %lld floats, the configuration needs %lld", (long long)n_weights, (long long)h.total);
    const std::vector<int32_t> map = blob_to_plain_image(*cfg);
    if ((int64_t)map.size() != h.total) return fail(PESTO_ERR_INVALID, "the weight image does not hold every parameter exactly once");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail(PESTO_ERR_HIP, "no HIP device available (training runs on the GPU only)");
    if (device < 0 || device >= n_dev) return fail(PESTO_ERR_INVALID, "device %d out of range (%d devices)", device, n_dev);
    TRY_HIP(hipSetDevice(device));
    pesto_trainer* t = new (std::nothrow) pesto_trainer();
    if (!t) return fail(PESTO_ERR_NOMEM, "out of host memory");
    t->cfg = *cfg; t->device = device; t->lr = lr; t->f = pos_weight_factor; t->n_weights = n_weights;
    const DeviceImage img = build_device_image(*cfg, weights);
    t->model = img.model; t->layers = img.layers; t->img_floats = img.data.size();
    const size_t wb = (size_t)n_weights * 4, ib = t->img_floats * 4;
    int rc = 0;
    do {
        if (hipStreamCreate(&t->stream) != hipSuccess) { rc = fail(PESTO_ERR_HIP, "stream creation failed"); break; }
        bool ev_ok = true;
        for (hipEvent_t& e : t->ev) ev_ok = ev_ok && hipEventCreate(&e) == hipSuccess;
        if (!ev_ok) { rc = fail(PESTO_ERR_HIP, "event creation failed"); break; }
        if (t->W.ensure(ib) || t->G.ensure(2 * ib) || t->blob.ensure(wb) || t->am.ensure(wb) || t->av.ensure(wb) || t->gblob.ensure(wb) || t->map.ensure(wb) ||
            t->pos.ensure(256) || t->flags.ensure(256)) { rc = fail(PESTO_ERR_NOMEM, "device allocation failed"); break; }
        std::vector<float> pos(64, 0.0f);
        for (int c = 0; c < cfg->n_out; ++c) pos[c] = 0.5f;
        hipError_t he = hipMemcpy(t->W.p, img.data.data(), ib, hipMemcpyHostToDevice);
        auto also = [&he](hipError_t e) { if (he == hipSuccess) he = e; };
        also(hipMemcpy(t->blob.p, weights, wb, hipMemcpyHostToDevice));
        also(hipMemcpy(t->map.p, map.data(), wb, hipMemcpyHostToDevice));
        also(hipMemcpy(t->pos.p, pos.data(), 256, hipMemcpyHostToDevice));
        also(hipMemset(t->am.p, 0, wb));
        also(hipMemset(t->av.p, 0, wb));
        also(hipMemset(t->G.p, 0, 2 * ib));
        also(hipMemset(t->flags.p, 0, 256));
        if (he != hipSuccess) { rc = fail(PESTO_ERR_HIP, "upload failed: %s", hipGetErrorString(he)); break; }
    } while (0);
    if (rc) { t->release(); delete t; return rc; }
    *out = t;
    return 0;
}

int pesto_train_destroy(pesto_trainer* t) {
    if (!t) return 0;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    t->release();
    delete t;
    return 0;
}

int pesto_train_step(pesto_trainer* t, int32_t mode, int64_t N, int64_t R, int32_t k, int32_t C, const float* X, const void* ids_topk,
                     int32_t ids_kind, const float* q0, const int32_t* res_of_atom, const float* y, float* losses_out, float* p_out,
                     float* z_out, float* grads_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_trainer(t)) return rc;
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (mode < 0 || mode > 2) return fail(PESTO_ERR_INVALID, "mode must be 0 (eval_step), 1 (loss_and_grad) or 2 (train_step)");
    CallIn in{X, ids_topk, q0, res_of_atom};
    if (int rc = check_call_args(N, R, k, ids_kind, in, ptr_kind)) return rc;
    if (C != t->cfg.n_out) return fail(PESTO_ERR_INVALID, "y has %d columns, the model has n_out = %d", C, t->cfg.n_out);
    if (!y) return fail(PESTO_ERR_INVALID, "null input");
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = dev ? (hipStream_t)stream : t->stream;
    const int L = t->cfg.n_layers;
    const size_t rc4 = (size_t)R * C * 4;
    t->kept.valid = 0;      // the states of a kept forward are overwritten
    if (int rc = ensure_state(t, N, R, L + 1)) return rc;
    if (t->out_l.ensure(rc4) || t->out_p.ensure(rc4)) return fail(PESTO_ERR_NOMEM, "workspace allocation failed");
    if (!dev) {
        if (t->in_y.ensure(rc4)) return fail(PESTO_ERR_NOMEM, "staging allocation failed");
        if (int rc = stage_inputs(t, st, N, k, ids_kind, in)) return rc;
        TRY_HIP(hipMemcpyAsync(t->in_y.p, y, rc4, hipMemcpyHostToDevice, st));
        y = t->in_y.as<float>();
    }
    if (int rc = check_on_device(t, st, N, R, k, ids_kind, in)) return rc;
    if (mode == 2) t->global_step += 1;
    if (t->timing) TRY_HIP(hipEventRecord(t->ev[0], st));
    // ---- training forward: every layer's input state is kept
    if (int rc = run_forward(t, st, N, R, k, ids_kind, in, true)) return rc;
    // ---- loss
    hipLaunchKernelGGL(k_pos_ratios, dim3(1), dim3(256), 0, st, (int)R, C, y, t->pos.as<float>(), (float)(1.0 + std::sqrt((double)t->global_step)));
    float* losses_d = dev && losses_out ? losses_out : t->out_l.as<float>();
    float* p_d = dev && p_out ? p_out : t->out_p.as<float>();
    hipLaunchKernelGGL(k_loss, dim3((unsigned)((R * C + 255) / 256)), dim3(256), 0, st, (int)R, C, t->f, t->z.as<float>(), y, t->pos.as<float>(), losses_d, p_d,
                       mode ? t->dz.as<float>() : nullptr);
    if (t->timing) TRY_HIP(hipEventRecord(t->ev[1], st));
    if (mode) {
        // ---- backward
        if (int rc = run_backward(t, st, N, R, in.X, in.q0, in.roa, nullptr, false)) return rc;
        if (t->timing) TRY_HIP(hipEventRecord(t->ev[2], st));
        if (mode == 2) {
            if (int rc = run_adam(t, st)) return rc;
        }
        if (t->timing) TRY_HIP(hipEventRecord(t->ev[3], st));
    }
    t->timed = t->timing && mode == 2;
    TRY_HIP(hipGetLastError());
    if (dev) {
        if (z_out) TRY_HIP(hipMemcpyAsync(z_out, t->z.p, rc4, hipMemcpyDeviceToDevice, st));
        if (grads_out && mode) TRY_HIP(hipMemcpyAsync(grads_out, t->gblob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (losses_out) TRY_HIP(hipMemcpyAsync(losses_out, losses_d, rc4, hipMemcpyDeviceToHost, st));
    if (p_out) TRY_HIP(hipMemcpyAsync(p_out, p_d, rc4, hipMemcpyDeviceToHost, st));
    if (z_out) TRY_HIP(hipMemcpyAsync(z_out, t->z.p, rc4, hipMemcpyDeviceToHost, st));
    if (grads_out && mode) TRY_HIP(hipMemcpyAsync(grads_out, t->gblob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    return 0;
}

int pesto_train_set_weights(pesto_trainer* t, const float* blob, int32_t ptr_kind, void* stream) {
    if (int rc = check_trainer(t)) return rc;
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (!blob) return fail(PESTO_ERR_INVALID, "null weight blob");
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = dev ? (hipStream_t)stream : t->stream;
    t->kept.valid = 0;      // a backward would recompute the kept forward from other weights
    if (!dev) TRY_HIP(hipDeviceSynchronize());
    TRY_HIP(hipMemcpyAsync(t->blob.p, blob, (size_t)t->n_weights * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_scatter_weights, dim3((unsigned)((t->n_weights + 255) / 256)), dim3(256), 0, st, t->n_weights, t->map.as<int>(),
                       t->blob.as<float>(), t->W.as<float>());
    TRY_HIP(hipGetLastError());
    if (!dev) TRY_HIP(hipStreamSynchronize(st));
    return 0;
}

int pesto_train_forward(pesto_trainer* t, int32_t keep, int64_t N, int64_t R, int32_t k, const float* X, const void* ids_topk, int32_t ids_kind,
                        const float* q0, const int32_t* res_of_atom, float* z_out, int64_t* ticket_out, int32_t ptr_kind, void* stream) {
    if (int rc = check_trainer(t)) return rc;
    CallIn in{X, ids_topk, q0, res_of_atom};
    if (int rc = check_call_args(N, R, k, ids_kind, in, ptr_kind)) return rc;
    if (!z_out || (keep && !ticket_out)) return fail(PESTO_ERR_INVALID, "null output");
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = dev ? (hipStream_t)stream : t->stream;
    const size_t rc4 = (size_t)R * t->cfg.n_out * 4;
    t->kept.valid = 0;      // every forward runs on the handle's one workspace: an earlier ticket ends here
    if (int rc = ensure_state(t, N, R, keep ? t->cfg.n_layers + 1 : 2)) return rc;
    if (!dev)
        if (int rc = stage_inputs(t, st, N, k, ids_kind, in)) return rc;
    if (int rc = check_on_device(t, st, N, R, k, ids_kind, in)) return rc;
    if (int rc = run_forward(t, st, N, R, k, ids_kind, in, keep != 0)) return rc;
    TRY_HIP(hipGetLastError());
    TRY_HIP(hipMemcpyAsync(z_out, t->z.p, rc4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (!dev) TRY_HIP(hipStreamSynchronize(st));
    if (keep) {
        t->kept.valid = ++t->tickets;
        t->kept.N = N; t->kept.R = R; t->kept.X = in.X; t->kept.q0 = in.q0; t->kept.roa = in.roa;
        *ticket_out = t->kept.valid;
    }
    return 0;
}

int pesto_train_backward(pesto_trainer* t, int64_t ticket, const float* dz, float* grads_out, float* dq0_out, float* dX_out, int32_t ptr_kind,
                         void* stream) {
    if (int rc = check_trainer(t)) return rc;
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (!dz) return fail(PESTO_ERR_INVALID, "null dz");
    if (ticket < 1 || ticket != t->kept.valid)
        return fail(PESTO_ERR_INVALID, "ticket %lld is not the handle's last kept forward: a later forward, training step, stage call or weight "
                    "update has replaced its states (backward must follow its own forward)", (long long)ticket);
    const bool dev = ptr_kind == PESTO_PTR_DEVICE;
    hipStream_t st = dev ? (hipStream_t)stream : t->stream;
    const int64_t N = t->kept.N, R = t->kept.R;
    const int n0 = t->cfg.n0;
    const size_t rc4 = (size_t)R * t->cfg.n_out * 4, N1 = (size_t)N + 1;
    if (dX_out && (t->dgeo.ensure(N1 * KMAX * 16) || t->dxf.ensure((size_t)N * 3 * 8) || t->gmax.ensure(256) || t->out_dx.ensure((size_t)N * 12)))
        return fail(PESTO_ERR_NOMEM, "workspace allocation failed");
    if (dq0_out && !dev && t->out_dq0.ensure((size_t)N * n0 * 4)) return fail(PESTO_ERR_NOMEM, "workspace allocation failed");
    TRY_HIP(hipMemcpyAsync(t->dz.p, dz, rc4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    float* dq0_d = !dq0_out ? nullptr : dev ? dq0_out : t->out_dq0.as<float>();
    if (int rc = run_backward(t, st, N, R, t->kept.X, t->kept.q0, t->kept.roa, dq0_d, dX_out != nullptr)) return rc;
    float* dx_d = dev ? dX_out : t->out_dx.as<float>();
    if (dX_out) to_float(st, (size_t)N * 3, t->dxf.as<fx_t>(), dx_d);
    TRY_HIP(hipGetLastError());
    if (dev) {
        if (grads_out) TRY_HIP(hipMemcpyAsync(grads_out, t->gblob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (grads_out) TRY_HIP(hipMemcpyAsync(grads_out, t->gblob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToHost, st));
    if (dq0_out) TRY_HIP(hipMemcpyAsync(dq0_out, dq0_d, (size_t)N * n0 * 4, hipMemcpyDeviceToHost, st));
    if (dX_out) TRY_HIP(hipMemcpyAsync(dX_out, dx_d, (size_t)N * 12, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    return 0;
}

int pesto_train_adam(pesto_trainer* t, const float* grads) {
    if (int rc = check_trainer(t)) return rc;
    if (!grads) return fail(PESTO_ERR_INVALID, "null gradient");
    t->kept.valid = 0;
    TRY_HIP(hipDeviceSynchronize());
    TRY_HIP(hipMemcpyAsync(t->gblob.p, grads, (size_t)t->n_weights * 4, hipMemcpyHostToDevice, t->stream));
    if (int rc = run_adam(t, t->stream)) return rc;
    TRY_HIP(hipStreamSynchronize(t->stream));
    return 0;
}

int pesto_train_get_state(pesto_trainer* t, float* weights_out, float* pos_ratios_out, int64_t* global_step, float* lr) {
    if (int rc = check_trainer(t)) return rc;
    TRY_HIP(hipDeviceSynchronize());
    if (weights_out) TRY_HIP(hipMemcpy(weights_out, t->blob.p, (size_t)t->n_weights * 4, hipMemcpyDeviceToHost));
    if (pos_ratios_out) TRY_HIP(hipMemcpy(pos_ratios_out, t->pos.p, (size_t)t->cfg.n_out * 4, hipMemcpyDeviceToHost));
    if (global_step) *global_step = t->global_step;
    if (lr) *lr = t->lr;
    return 0;
}

int pesto_train_set_state(pesto_trainer* t, const float* pos_ratios, const int64_t* global_step, const float* lr) {
    if (int rc = check_trainer(t)) return rc;
    if (global_step && *global_step < 0) return fail(PESTO_ERR_INVALID, "global_step must be >= 0");
    if (lr && !(*lr >= 0.0f)) return fail(PESTO_ERR_INVALID, "lr must be >= 0");
    TRY_HIP(hipDeviceSynchronize());
    if (pos_ratios) TRY_HIP(hipMemcpy(t->pos.p, pos_ratios, (size_t)t->cfg.n_out * 4, hipMemcpyHostToDevice));
    if (global_step) t->global_step = *global_step;
    if (lr) t->lr = *lr;
    return 0;
}

int pesto_train_set_timing(pesto_trainer* t, int32_t enabled) {
    if (int rc = check_trainer(t)) return rc;
    t->timing = enabled != 0;
    t->timed = false;
    return 0;
}

int pesto_train_get_timing(pesto_trainer* t, double* ms_out) {
    if (int rc = check_trainer(t)) return rc;
    if (!ms_out) return fail(PESTO_ERR_INVALID, "null argument");
    if (!t->timed) return fail(PESTO_ERR_STATE, "no timed train_step yet (pesto_train_set_timing, then pesto_train_step with mode 2)");
    TRY_HIP(hipEventSynchronize(t->ev[3]));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.0f;
        TRY_HIP(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
        ms_out[i] = ms;
    }
    return 0;
}

int pesto_train_stage_embed(pesto_trainer* t, int64_t N, const float* q0, const float* dq, float* grads_out) {
    if (int rc = check_trainer(t)) return rc;
    if (N < 1 || N > (1 << 24) || !q0 || !dq) return fail(PESTO_ERR_INVALID, "bad arguments");
    t->kept.valid = 0;
    if (int rc = ensure_state(t, N, 1, 1)) return rc;
    const int n0 = t->cfg.n0;
    if (t->in_q0.ensure((size_t)N * n0 * 4)) return fail(PESTO_ERR_NOMEM, "staging allocation failed");
    hipStream_t st = t->stream;
    TRY_HIP(hipDeviceSynchronize());
    TRY_HIP(hipMemsetAsync(t->G.p, 0, t->img_floats * 8, st));
    TRY_HIP(hipMemcpyAsync(t->in_q0.p, q0, (size_t)N * n0 * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->fq.as<float>() + S, dq, (size_t)N * S * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_embed_bwd, dim3((unsigned)((N + 7) / 8)), dim3(256), 0, st, t->W.as<float>(), t->G.as<fx_t>(), t->model.em, (int)N, n0,
                       t->in_q0.as<float>(), t->fq.as<float>(), (float*)nullptr);
    return stage_finish(t, st, grads_out);
}

int pesto_train_stage_layer(pesto_trainer* t, int32_t layer, int64_t N, int32_t k, const float* X, const void* ids_topk, int32_t ids_kind,
                            const float* q_in, const float* p_in, const float* dq_out, const float* dp_out, float* dq_in, float* dp_in,
                            float* grads_out) {
    if (int rc = check_trainer(t)) return rc;
    if (layer < 0 || layer >= t->cfg.n_layers || N < 1 || N > (1 << 24) || k < 1 || k > KMAX || !X || !ids_topk || !q_in || !p_in || !dq_out || !dp_out)
        return fail(PESTO_ERR_INVALID, "bad arguments");
    if (ids_kind != PESTO_IDS_INT32 && ids_kind != PESTO_IDS_INT64) return fail(PESTO_ERR_INVALID, "ids_kind must be 32 or 64");
    t->kept.valid = 0;
    if (int rc = ensure_state(t, N, 1, 1)) return rc;
    const size_t N1 = (size_t)N + 1, id_sz = ids_kind == PESTO_IDS_INT64 ? 8 : 4;
    if (t->in_X.ensure((size_t)N * 12) || t->in_ids.ensure((size_t)N * k * id_sz)) return fail(PESTO_ERR_NOMEM, "staging allocation failed");
    hipStream_t st = t->stream;
    TRY_HIP(hipDeviceSynchronize());
    // the ids are checked on the host here (host pointers): nothing out of range reaches a kernel
    for (size_t e = 0; e < (size_t)N * k; ++e) {
        const long long id = ids_kind == PESTO_IDS_INT64 ? ((const long long*)ids_topk)[e] : (long long)((const int*)ids_topk)[e];
        if (id < 0 || id > N) return fail(PESTO_ERR_INVALID, "ids_topk holds an id outside [0, N]");
    }
    TRY_HIP(hipMemsetAsync(t->G.p, 0, t->img_floats * 8, st));
    TRY_HIP(hipMemcpyAsync(t->in_X.p, X, (size_t)N * 12, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->in_ids.p, ids_topk, (size_t)N * k * id_sz, hipMemcpyHostToDevice, st));
    if (int rc = run_unpack(t, st, N, k, t->in_X.as<float>(), t->in_ids.p, ids_kind)) return rc;
    TRY_HIP(hipMemcpyAsync(t->sq.p, q_in, N1 * S * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->sp.p, p_in, N1 * 96 * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->fq.p, dq_out, N1 * S * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->fp.p, dp_out, N1 * 96 * 4, hipMemcpyHostToDevice, st));
    to_fixed(st, N1 * S, t->fq.as<float>(), t->dqa.as<fx_t>());
    to_fixed(st, N1 * 96, t->fp.as<float>(), t->dpa.as<fx_t>());
    TRY_HIP(hipMemsetAsync(t->dqb.p, 0, N1 * S * 8, st));
    TRY_HIP(hipMemsetAsync(t->dpb.p, 0, N1 * 96 * 8, st));
    launch_layer_v1_bwd(st, t->W.as<float>(), t->G.as<fx_t>(), t->layers[layer], (int)N1, t->ids_s.as<int>(), t->geo.as<float4>(), t->sq.as<float>(),
                        t->sp.as<float>(), t->dqa.as<fx_t>(), t->dpa.as<fx_t>(), t->dqb.as<fx_t>(), t->dpb.as<fx_t>());
    to_float(st, N1 * S, t->dqb.as<fx_t>(), t->fq.as<float>());
    to_float(st, N1 * 96, t->dpb.as<fx_t>(), t->fp.as<float>());
    TRY_HIP(hipGetLastError());
    if (dq_in) TRY_HIP(hipMemcpyAsync(dq_in, t->fq.p, N1 * S * 4, hipMemcpyDeviceToHost, st));
    if (dp_in) TRY_HIP(hipMemcpyAsync(dp_in, t->fp.p, N1 * 96 * 4, hipMemcpyDeviceToHost, st));
    return stage_finish(t, st, grads_out);
}

int pesto_train_stage_head(pesto_trainer* t, int64_t N, int64_t R, const float* q, const float* p, const int32_t* res_of_atom, const float* dz,
                           float* dq, float* dp, float* grads_out) {
    if (int rc = check_trainer(t)) return rc;
    if (N < 1 || N > (1 << 24) || R < 1 || R > N || !q || !p || !res_of_atom || !dz) return fail(PESTO_ERR_INVALID, "bad arguments");
    {   // host pointers: the residue map is checked here, nothing out of range reaches a kernel
        std::vector<char> seen((size_t)R, 0);
        for (int64_t i = 0; i < N; ++i) {
            if (res_of_atom[i] < 0 || res_of_atom[i] >= R) return fail(PESTO_ERR_INVALID, "res_of_atom holds a residue outside [0, R)");
            seen[res_of_atom[i]] = 1;
        }
        for (int64_t r = 0; r < R; ++r)
            if (!seen[r]) return fail(PESTO_ERR_INVALID, "a residue has no atom");
    }
    t->kept.valid = 0;
    if (int rc = ensure_state(t, N, R, 1)) return rc;
    if (t->in_roa.ensure((size_t)N * 4)) return fail(PESTO_ERR_NOMEM, "staging allocation failed");
    const int C = t->cfg.n_out;
    hipStream_t st = t->stream;
    TRY_HIP(hipDeviceSynchronize());
    float* qd = t->sq.as<float>() + S;
    float* pd = t->sp.as<float>() + 96;
    TRY_HIP(hipMemsetAsync(t->G.p, 0, t->img_floats * 8, st));
    TRY_HIP(hipMemsetAsync(t->flags.p, 0, 256, st));
    TRY_HIP(hipMemcpyAsync(qd, q, (size_t)N * S * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(pd, p, (size_t)N * 96 * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->in_roa.p, res_of_atom, (size_t)N * 4, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(t->dz.p, dz, (size_t)R * C * 4, hipMemcpyHostToDevice, st));
    int* lo = t->seg.as<int>();
    launch_pool(st, t->W.as<float>(), t->model, C, (int)N, (int)R, qd, pd, t->in_roa.as<int>(), t->a_tmp.as<float>(), lo, lo + R, err_ptr(t), nullptr, nullptr,
                t->z.as<float>());
    run_head_bwd(t, st, N, R, qd, pd, t->in_roa.as<int>());
    TRY_HIP(hipGetLastError());
    if (dq) TRY_HIP(hipMemcpyAsync(dq, t->fq.as<float>() + S, (size_t)N * S * 4, hipMemcpyDeviceToHost, st));
    if (dp) TRY_HIP(hipMemcpyAsync(dp, t->fp.as<float>() + 96, (size_t)N * 96 * 4, hipMemcpyDeviceToHost, st));
    return stage_finish(t, st, grads_out);
}

}  // extern "C"
