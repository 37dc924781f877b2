// pesto_scan.h - the scans and searches the analysis groups share: the range of an offsets array that holds an index (struct_of), the
// one-workgroup exclusive scan (block_scan_exclusive) and the list protocol of the list-valued entry points (count -> scan per frame ->
// 64-bit offsets -> emit: ListState, k_frame_scan, k_list_offsets on the device; list_scan, list_offsets, list_tail on the host).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "pesto_call.h"

namespace pesto {

namespace {

// the range [offsets[k], offsets[k + 1]) of offsets[0 .. n] that holds i (offsets[0] <= i)
__device__ __forceinline__ int struct_of(int i, int n, const int* __restrict__ offsets) {
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// ... over 64-bit offsets: the frame that owns list entry k, off[f] <= k < off[f + 1]
__device__ __forceinline__ int struct_of(long long k, int F, const long long* __restrict__ off) {
    int lo = 0, hi = F;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

// exclusive scan in place of data[0, len) by one workgroup of NT threads (all of them call); with COPY, `copy` receives the result too
// (a compile-time choice: the loop is a chain of dependent loads, a test per element shows). Returns the total in every thread.
template <int NT, bool COPY>
__device__ __forceinline__ int block_scan_exclusive(int* __restrict__ data, int len, int* __restrict__ copy = nullptr) {
    __shared__ int part[NT];
    const int per = (len + NT - 1) / NT;
    const int c0 = min(len, (int)threadIdx.x * per), c1 = min(len, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += data[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) {
        const int n = data[c];
        data[c] = run;
        if (COPY) copy[c] = run;
        run += n;
    }
    return part[NT - 1];
}

// ---- the list protocol of pesto_docking.hip and pesto_hbonds.hip: count -> scan per frame -> 64-bit offsets -> emit
constexpr int LIST_SCAN_NT = 1024;      // threads of the one workgroup that scans the frames' totals

// the device counters of one call
struct ListState {
    long long K;      // list entries over all frames
    int fits;         // K <= capacity: the emit pass runs
    int err;          // error bits of the call's own index checks
};

// one workgroup per frame: the frame's n counts scanned in place (exclusive), their total to ftot[f]
template <int NT>
__global__ __launch_bounds__(NT) void k_frame_scan(int n, int* __restrict__ cnt, int* __restrict__ ftot) {
    const int total = block_scan_exclusive<NT, false>(cnt + (size_t)blockIdx.x * n, n);
    if (threadIdx.x == 0) ftot[blockIdx.x] = total;
}

// one workgroup: off[0 .. F] = exclusive scan of the frames' totals in 64 bits; K and whether it fits the capacity
__global__ __launch_bounds__(LIST_SCAN_NT) void k_list_offsets(int F, const int* __restrict__ ftot, long long* __restrict__ off, long long cap,
                                                               ListState* __restrict__ st) {
    __shared__ long long part[LIST_SCAN_NT];
    const int per = (F + LIST_SCAN_NT - 1) / LIST_SCAN_NT;
    const int c0 = min(F, (int)threadIdx.x * per), c1 = min(F, c0 + per);
    long long sum = 0;
    for (int c = c0; c < c1; ++c) sum += ftot[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < LIST_SCAN_NT; o <<= 1) {
        const long long v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - sum;
    for (int c = c0; c < c1; ++c) { off[c] = run; run += ftot[c]; }
    if (threadIdx.x == LIST_SCAN_NT - 1) {
        off[F] = part[LIST_SCAN_NT - 1];
        st->K = part[LIST_SCAN_NT - 1];
        st->fits = part[LIST_SCAN_NT - 1] <= cap ? 1 : 0;
    }
}

// ---- the host half: the scan's launches between the call's count and emit passes, and the list's way back after verdict()

// off[0 .. F] (item iOff), K and whether it fits `cap` (item iSt, a ListState) from the F totals of item iTot
void list_offsets(Buffers& bf, int F, int iTot, int iOff, long long cap, int iSt) {
    hipLaunchKernelGGL(k_list_offsets, dim3(1), dim3(LIST_SCAN_NT), 0, bf.stm, F, bf.ptr<const int>(iTot), bf.ptr<long long>(iOff), cap,
                       bf.ptr<ListState>(iSt));
}

// ... from F frames of n counts each (item iCnt, scanned in place per frame; their totals to item iTot)
template <int NT>
void list_scan(Buffers& bf, int F, int n, int iCnt, int iTot, int iOff, long long cap, int iSt) {
    hipLaunchKernelGGL(k_frame_scan<NT>, dim3((unsigned)F), dim3(NT), 0, bf.stm, n, bf.ptr<int>(iCnt), bf.ptr<int>(iTot));
    list_offsets(bf, F, iTot, iOff, cap, iSt);
}

// sizes_out[0] = K; where the list fits (and the caller's own condition `take` holds), the first K entries of every partial output
// named as {item, bytes per entry}
struct ListPart { int item; size_t bytes; };

int list_tail(Buffers& bf, const ListState& hs, int64_t* sizes_out, std::initializer_list<ListPart> parts, bool take = true) {
    sizes_out[0] = hs.K;
    if (hs.fits && take)
        for (const ListPart& p : parts)
            if (int rc = bf.fetch(p.item, (size_t)hs.K * p.bytes)) return rc;
    return 0;
}

}  // namespace
}  // namespace pesto
