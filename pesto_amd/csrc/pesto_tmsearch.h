// pesto_tmsearch.h - the TM-score superposition search of pesto_tmscore.hip as other translation units launch it: the structure alignment
// (pesto_structalign.hip) runs it on the residue pairs it has aligned, as a ragged batch on device arrays it owns. The kernels stay where
// they are; this declares the host-made table entry of a structure, what a share reports, and the launch of the two kernels. A call made
// through here computes what pesto_tmscore computes for the same points, constants and step, bit for bit: it is the same launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pesto {

constexpr int TM_MAX_LENGTHS = 7;       // window lengths L >> 0 .. 5, then min(L, 4)
constexpr int TM_N_CUT = 5;             // GDT cut-offs

// one structure of the call: its range of sel, its seeds (cnt[l] windows of length len[l], numbered length first, then start; the starts
// 0, step, 2 step, ...) and its constants
struct TmStruct {
    int s0, L, n_len, n_seeds;
    int len[TM_MAX_LENGTHS], cnt[TM_MAX_LENGTHS];
    int step, pad;
    double d0, lnorm, d_search;
};

// what a share found: the best TM sum over its visited fits with its seed and fit (x' = x R + t), and the largest counts
struct TmBest {
    double tm, R[9], t[3];
    int seed, cnt[TM_N_CUT];
};

// the table entry of a structure of L selected atoms from sel[s0] on
void tm_plan(int s0, int L, int step, double norm_len, double d0, TmStruct& s);

// the workgroups a unit's seeds are shared over, for U units whose largest number of seeds is seeds_max
int tm_shares(int seeds_max, int64_t U);

// k_tm_search and k_tm_final on device pointers: U units (frames of one structure, or the n_struct > 1 structures of one frame) of at
// most L_max selected atoms; structs [n_struct] is on the device, parts [U * shares] is scratch, *err != 0 makes both kernels return at once
hipError_t tm_search_launch(hipStream_t stm, int64_t U, int64_t N, int n_struct, int shares, int L_max, int n_iter, double scale, const TmStruct* structs,
                            const float* ref, const float* xyz, const int* sel, const int* err, TmBest* parts, float* tm_out, float* ts_out, float* ha_out,
                            int* counts_out, int* seed_out, double* rot_out, double* tr_out);

}  // namespace pesto
