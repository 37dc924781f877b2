// pesto_radix.h - the library's one sort, for the ranking columns (pesto_rank.hip), the dataset contacts (pesto_contacts.hip) and the best poses (pesto_poses.hip): a stable
// LSD radix sort of 64-bit keys on the bits [bit_lo, bit_lo + 8 n_pass). 8-bit digits, per pass a histogram per workgroup tile, one scan
// of the [digit][tile] counters and a scatter that is stable within the pass (ranks by __ballot per wave, wave offsets through LDS); the
// keys are double-buffered and a pass whose counters show one occupied bucket moves nothing (the buffers' roles are device state,
// RadixState.src). The length is read on the device (*n_ptr, at most the capacity that sizes the launches). There is no payload.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pesto_hip.h"
#include "pesto_scan.h"

namespace pesto {

namespace {

typedef unsigned long long u64;

constexpr int RADIX_NT = 256;                    // threads per workgroup of the histogram and the scatter
constexpr int RADIX_ITEMS = 8;                   // keys per thread and radix pass
constexpr int RADIX_TILE = PESTO_RANK_TILE;      // keys per workgroup and radix pass
constexpr int RADIX_WAVES = RADIX_NT / 64;
constexpr int RADIX_MAX_PASSES = 8;
static_assert(RADIX_TILE == RADIX_NT * RADIX_ITEMS, "a tile is RADIX_ITEMS rounds of one key per thread");

// which of the two key buffers pass k reads (0: a; src[n_pass]: where the sorted keys are) and the passes that move nothing. A sort
// starts from src[0] == 0 and writes src[1 .. n_pass] and skip[0 .. n_pass) only, so one zeroed state serves several sorts in stream order.
struct RadixState {
    int src[RADIX_MAX_PASSES + 1];
    int skip[RADIX_MAX_PASSES];
};

// the sorted keys after n_pass passes over (a, b)
__device__ __forceinline__ const u64* radix_sorted(const u64* a, const u64* b, int n_pass, const RadixState* __restrict__ st) {
    return st->src[n_pass] ? b : a;
}

__host__ __device__ inline long long radix_tiles(long long n) { return (n + RADIX_TILE - 1) / RADIX_TILE; }
inline size_t radix_counter_bytes(size_t cap) { return 256 * (size_t)radix_tiles((long long)cap) * sizeof(int); }   // bytes of the counters of a sort of at most cap keys

// digit counts of tile blockIdx.x -> counters[digit * n_tiles + tile]
__global__ __launch_bounds__(RADIX_NT) void k_radix_hist(const int* __restrict__ n_ptr, int bit_lo, int pass, const u64* __restrict__ keys_a,
                                                         const u64* __restrict__ keys_b, const RadixState* __restrict__ st, int* __restrict__ counters) {
    __shared__ int hist[256];
    const long long n = *n_ptr;
    const int n_tiles = (int)radix_tiles(n);
    if ((int)blockIdx.x >= n_tiles) return;
    const u64* src = st->src[pass] ? keys_b : keys_a;
    const int shift = bit_lo + 8 * pass;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * RADIX_TILE;
#pragma unroll
    for (int i = 0; i < RADIX_ITEMS; ++i) {
        const long long j = t0 + i * RADIX_NT + threadIdx.x;
        if (j < n) atomicAdd(&hist[(unsigned)(src[j] >> shift) & 255u], 1);
    }
    __syncthreads();
    counters[(size_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
}

// one workgroup: the counters scanned in place (digit-major, so tile t's keys of digit d start at counters[d * n_tiles + t]); a pass
// with one occupied bucket (or no key at all) is skipped and leaves the buffers' roles as they are
__global__ __launch_bounds__(1024) void k_radix_scan(const int* __restrict__ n_ptr, int pass, int* __restrict__ counters, RadixState* __restrict__ st) {
    __shared__ int one;
    const long long n = *n_ptr;
    const int n_tiles = (int)radix_tiles(n);
    if (threadIdx.x == 0) one = n == 0;
    block_scan_exclusive<1024, false>(counters, 256 * n_tiles);
    __syncthreads();
    if (threadIdx.x < 256 && n > 0) {
        const long long hi = threadIdx.x < 255 ? counters[((size_t)threadIdx.x + 1) * n_tiles] : n;
        if (hi - counters[(size_t)threadIdx.x * n_tiles] == n) one = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st->skip[pass] = one;
        st->src[pass + 1] = one ? st->src[pass] : 1 - st->src[pass];
    }
}

// the keys of tile blockIdx.x to their places, in their order within the tile (key i * RADIX_NT + t is the i-th round's t-th): per round
// every wave matches equal digits with eight ballots (rank among the lanes before, count), the waves' counts meet in LDS
__global__ __launch_bounds__(RADIX_NT) void k_radix_scatter(const int* __restrict__ n_ptr, int bit_lo, int pass, u64* __restrict__ keys_a,
                                                            u64* __restrict__ keys_b, const RadixState* __restrict__ st, const int* __restrict__ counters) {
    if (st->skip[pass]) return;
    __shared__ int base[256];
    __shared__ int wcnt[RADIX_WAVES][256];
    const long long n = *n_ptr;
    const int n_tiles = (int)radix_tiles(n);
    if ((int)blockIdx.x >= n_tiles) return;
    const int from = st->src[pass];
    const u64* src = from ? keys_b : keys_a;
    u64* dst = from ? keys_a : keys_b;
    const int shift = bit_lo + 8 * pass;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    base[threadIdx.x] = counters[(size_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < RADIX_WAVES; ++k) wcnt[k][threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * RADIX_TILE;
    for (int i = 0; i < RADIX_ITEMS; ++i) {
        const long long j = t0 + i * RADIX_NT + threadIdx.x;
        const bool valid = j < n;
        const u64 key = valid ? src[j] : 0;
        const unsigned d = (unsigned)(key >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[w][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            long long pos = base[d] + rank;
            for (int k = 0; k < w; ++k) pos += wcnt[k][d];
            if (pos < n) dst[pos] = key;                           // (always, when the counters are this buffer's)
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int k = 0; k < RADIX_WAVES; ++k) { add += wcnt[k][threadIdx.x]; wcnt[k][threadIdx.x] = 0; }
        base[threadIdx.x] += add;
        __syncthreads();
    }
}

// the stable sort of the first *n_ptr (<= cap) keys of `a` on the bits [bit_lo, bit_lo + 8 n_pass), `b` the second buffer and `counters`
// radix_counter_bytes(cap) of scratch: 3 n_pass launches; the sorted keys are radix_sorted(a, b, n_pass, st) afterwards
inline void radix_sort(hipStream_t s, u64* a, u64* b, long long cap, const int* n_ptr, int bit_lo, int n_pass, int* counters, RadixState* st) {
    const dim3 grid((unsigned)radix_tiles(cap));
    for (int pass = 0; pass < n_pass; ++pass) {
        hipLaunchKernelGGL(k_radix_hist, grid, dim3(RADIX_NT), 0, s, n_ptr, bit_lo, pass, (const u64*)a, (const u64*)b, (const RadixState*)st, counters);
        hipLaunchKernelGGL(k_radix_scan, dim3(1), dim3(1024), 0, s, n_ptr, pass, counters, st);
        hipLaunchKernelGGL(k_radix_scatter, grid, dim3(RADIX_NT), 0, s, n_ptr, bit_lo, pass, a, b, (const RadixState*)st, (const int*)counters);
    }
}

}  // namespace
}  // namespace pesto
