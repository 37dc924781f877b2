// pesto_oligomer.h - the input the oligomer scorers share (pesto_chainmap.hip, pesto_qsscore.hip): a reference and F models, each a run of
// chains given by offsets and group ids, within the limits PESTO_CHAINMAP_MAX_*; a missing residue is NaN, an infinite coordinate spoils
// its frame. Here are the check of the sizes, the layout step (the four small arrays brought to the host and checked there, before
// anything is launched) and the per-frame scan for an infinite coordinate.
//
// Everything sits in an anonymous namespace, like pesto_call.h: fail() writes to the message channel of the including translation unit.
#pragma once
#include <cmath>

#include "pesto_call.h"

namespace pesto {

namespace {

constexpr int OLIGOMER_NT = 256;        // threads per workgroup of k_oligomer_frames

int check_oligomer_sizes(int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, double scale) {
    if (F < 1 || F > PESTO_CHAINMAP_MAX_FRAMES || Nr < 3 || Nr > 0x3fffffff || Nm < 3 || Nm > 0x3fffffff)
        return fail(PESTO_ERR_INVALID, "1 to 2^23 frames and 3 <= Nr, Nm < 2^30 residues");
    if (Cr < 1 || Cr > PESTO_CHAINMAP_MAX_CHAINS || Cm < 1 || Cm > PESTO_CHAINMAP_MAX_CHAINS)
        return fail(PESTO_ERR_INVALID, "1 to %d chains on each side", PESTO_CHAINMAP_MAX_CHAINS);
    if (!(std::isfinite(scale) && scale > 0.0)) return fail(PESTO_ERR_INVALID, "scale must be positive and finite");
    return 0;
}

// the layout of both sides on the host
struct OligomerLayout {
    const int32_t* ro;                  // [Cr + 1] the reference's offsets
    const int32_t* rg;                  // [Cr] its group ids
    const int32_t* mo;                  // [Cm + 1] the models'
    const int32_t* mg;                  // [Cm]
    int longest = 0;                    // slots of the longest chain
    std::vector<int32_t> fetched;       // the four arrays, where they came from the device
};

// The layout step of a call, after check_oligomer_sizes and begin(): the four arrays live where ptr_kind says, so device arrays (at most
// 65 ints each) are brought over first, on the call's stream. Then, per side, offsets from 0 to N in ascending order, and per chain a
// group id in [0, MAX_GROUPS), 3 to MAX_LENGTH slots and as many as every chain of its group met so far ON EITHER SIDE, at most MAX_GROUP
// chains of a group on the side. Nothing has been launched when a layout is refused.
int fetch_layout(const char* who, int64_t Nr, int64_t Nm, int Cr, int Cm, const int32_t* ref_offsets, const int32_t* ref_group, const int32_t* offsets,
                 const int32_t* group, int32_t ptr_kind, void* stream, OligomerLayout& lay) {
    const int32_t* at[4] = {ref_offsets, ref_group, offsets, group};
    if (ptr_kind == PESTO_PTR_DEVICE) {
        const size_t n[4] = {(size_t)Cr + 1, (size_t)Cr, (size_t)Cm + 1, (size_t)Cm};
        lay.fetched.resize(n[0] + n[1] + n[2] + n[3]);
        int32_t* h = lay.fetched.data();
        for (int k = 0; k < 4; ++k) {
            if (int rc = hip_ok(hipMemcpyAsync(h, at[k], n[k] * 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "copy of the layout to the host failed")) return rc;
            at[k] = h;
            h += n[k];
        }
        if (int rc = hip_ok(hipStreamSynchronize((hipStream_t)stream), "copy of the layout to the host failed")) return rc;
    }
    lay.ro = at[0];
    lay.rg = at[1];
    lay.mo = at[2];
    lay.mg = at[3];
    int len[PESTO_CHAINMAP_MAX_GROUPS];
    for (int& v : len) v = 0;
    for (int side = 0; side < 2; ++side) {
        const int32_t* off = side ? lay.mo : lay.ro;
        const int32_t* grp = side ? lay.mg : lay.rg;
        const int C = side ? Cm : Cr;
        const int64_t N = side ? Nm : Nr;
        if (off[0] != 0 || off[C] != N || first_unordered(off, C) >= 0)
            return fail(PESTO_ERR_INVALID, "%s: offsets must start at 0, end at the number of residues and ascend", who);
        int count[PESTO_CHAINMAP_MAX_GROUPS];
        for (int& v : count) v = 0;
        for (int c = 0; c < C; ++c) {
            if (grp[c] < 0 || grp[c] >= PESTO_CHAINMAP_MAX_GROUPS) return fail(PESTO_ERR_INVALID, "%s: group ids must lie in [0, %d)", who, PESTO_CHAINMAP_MAX_GROUPS);
            const int L = off[c + 1] - off[c];
            if (L < 3 || L > PESTO_CHAINMAP_MAX_LENGTH || (len[grp[c]] && len[grp[c]] != L))
                return fail(PESTO_ERR_INVALID, "%s: a chain must have 3 to %d slots, as many as every chain of its group", who, PESTO_CHAINMAP_MAX_LENGTH);
            len[grp[c]] = L;
            lay.longest = std::max(lay.longest, L);
            if (++count[grp[c]] > PESTO_CHAINMAP_MAX_GROUP) return fail(PESTO_ERR_INVALID, "%s: at most %d chains of a group on a side", who, PESTO_CHAINMAP_MAX_GROUP);
        }
    }
    return 0;
}

// bad[f] = frame f has an infinite coordinate, or *ref_bad: the reference has one. Scanned once per frame, read by everything that
// works on the frame.
__global__ __launch_bounds__(OLIGOMER_NT) void k_oligomer_frames(int Nm, const float* __restrict__ xyz, const int* __restrict__ ref_bad,
                                                                 int* __restrict__ bad_out) {
    const float* X = xyz + (size_t)blockIdx.x * Nm * 3;
    int bad = *ref_bad;
    for (size_t k = threadIdx.x; k < (size_t)Nm * 3; k += OLIGOMER_NT) bad |= fabsf(X[k]) == INFINITY;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_out[blockIdx.x] = bad ? 1 : 0;
}

}  // namespace
}  // namespace pesto
