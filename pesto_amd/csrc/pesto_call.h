// pesto_call.h - the host plumbing of one analysis call (pesto_eval / patches / contacts / trajectory / sasa / dssp / rank / surface /
// docking / dockq / poses / hbonds / lddt / tmscore / align / structalign / cluster / peaks / dynamics / enm .hip, and the message channel of pesto_train.hip): the group's message
// channel, the handle's synchronisation, the offsets check, the launch shape and the call's one stream-ordered allocation with its staged
// copies, its cleared buffers and the read of the device's verdict. (pesto_chainmap.hip and pesto_qsscore.hip come here through
// pesto_oligomer.h, which adds the layout of an oligomer and its check.)
//
// The protocol of one call: declare the buffers (a cleared one with its fill byte) -> upload() -> launch -> verdict(), where the host
// needs the device's verdict before it goes on (to size a list: list_tail of pesto_scan.h; to refuse before anything is written;
// between two phases), or read() of it where it is decoded only after finish() -> finish() -> decode the error bits into the group's
// own messages.
//
// Everything sits in an anonymous namespace, so every translation unit that includes this header keeps a message of its own
// (pesto_*_last_error of that group returns last_error()). These entry points need only the handle's device (pesto_synchronize sets it and
// resolves a deferred AUTO check) and allocate per call, so they share nothing with the forward's workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/pesto_hip.h"

namespace pesto {

namespace {

thread_local std::string g_call_err;

const char* last_error() { return g_call_err.c_str(); }

__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_call_err = buf;
    return code;
}

// 0, or PESTO_ERR_HIP with "<what>: <HIP's message>"
int hip_ok(hipError_t e, const char* what) { return e == hipSuccess ? 0 : fail(PESTO_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }

int check_ptr_kind(int32_t ptr_kind) {
    if (ptr_kind != PESTO_PTR_HOST && ptr_kind != PESTO_PTR_DEVICE) return fail(PESTO_ERR_INVALID, "ptr_kind must be PESTO_PTR_HOST or PESTO_PTR_DEVICE");
    return 0;
}

// the last argument check of every entry point: ptr_kind, then the handle's device current, a deferred AUTO check of its last launch
// resolved and its own stream drained
int begin(pesto_model* m, int32_t ptr_kind) {
    if (int rc = check_ptr_kind(ptr_kind)) return rc;
    if (int rc = pesto_synchronize(m)) {
        const char* e = pesto_last_error();
        return fail(rc, "%s", e ? e : "invalid model handle");
    }
    return 0;
}

// the first range of offs[0 .. n] that is empty or runs backwards, -1 if none
int first_unordered(const int32_t* offs, int32_t n) {
    for (int s = 0; s < n; ++s)
        if (offs[s + 1] <= offs[s]) return s;
    return -1;
}

// offs[0 .. n] must split [0, total] into n non-empty ranges (`unit`s, in the message)
int check_offsets(const int32_t* offs, int32_t n, int64_t total, const char* what, const char* unit = "structure") {
    if (offs[0] != 0 || offs[n] != total) return fail(PESTO_ERR_INVALID, "%s must span [0, %lld]", what, (long long)total);
    const int s = first_unordered(offs, n);
    return s < 0 ? 0 : fail(PESTO_ERR_INVALID, "%s: empty or unordered %s %d", what, unit, s);
}

// workgroups of nt threads over n items
unsigned blocks(size_t n, int nt) { return (unsigned)((n + nt - 1) / nt); }

// The buffers of one call, declared first and then allocated as ONE stream-ordered block that finish() frees on every path. Inputs and
// outputs are the caller's own pointers on the device side and staged copies on the host side (a NULL one stays NULL on either side);
// scratch and host-made tables always live in the block. upload() allocates, copies the staged inputs and the tables in and clears the
// outputs and scratch declared with a fill byte (the caller's own arrays too, on the device side); finish() checks the launches, copies
// the staged outputs out, frees and synchronises.
struct Buffers {
    struct Item { const void* in; void* out; size_t bytes, at; bool own, whole; int fill; };
    bool dev;
    hipStream_t stm;
    char* w = nullptr;
    size_t total = 0;
    std::vector<Item> items;
    Buffers(int32_t ptr_kind, void* stream) : dev(ptr_kind == PESTO_PTR_DEVICE), stm((hipStream_t)stream) {}
    int add(const void* in, void* out, size_t bytes, bool own, bool whole = true, int fill = -1) {
        Item it{in, out, bytes, total, own, whole, fill};
        if (own) total += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        items.push_back(it);
        return (int)items.size() - 1;
    }
    int input(const void* p, size_t bytes) { return add(p, nullptr, bytes, !dev && p); }
    int table(const void* host, size_t bytes) { return add(host, nullptr, bytes, true); }
    // (fill >= 0, here and for scratch: every byte is set to it before the call's first launch)
    int output(void* p, size_t bytes, int fill = -1) { return add(nullptr, p, bytes, !dev && p, true, fill); }
    // an output of which the call itself brings back what it filled (fetch); finish() leaves it alone
    int partial(void* p, size_t bytes, int fill = -1) { return add(nullptr, p, bytes, !dev && p, false, fill); }
    int scratch(size_t bytes, int fill = -1) { return add(nullptr, nullptr, bytes, true, true, fill); }
    template <class T> T* ptr(int i) const {
        const Item& it = items[i];
        if (it.own) return (T*)(w + it.at);
        return (T*)(it.in ? it.in : it.out);
    }
    int upload() {
        if (hipMallocAsync((void**)&w, std::max<size_t>(total, 256), stm) != hipSuccess) {
            w = nullptr;
            return fail(PESTO_ERR_NOMEM, "device allocation of %zu bytes failed", total);
        }
        for (const Item& it : items)
            if (it.own && it.in)
                if (int rc = hip_ok(hipMemcpyAsync(w + it.at, it.in, it.bytes, hipMemcpyHostToDevice, stm), "copy to the device failed")) return rc;
        for (int i = 0; i < (int)items.size(); ++i)
            if (items[i].fill >= 0 && items[i].bytes && ptr<void>(i))
                if (int rc = hip_ok(hipMemsetAsync(ptr<void>(i), items[i].fill, items[i].bytes, stm), "clearing a device buffer failed")) return rc;
        return 0;
    }
    // 0, or PESTO_ERR_HIP with "<what>: launch failed: <HIP's message>"
    int launched(const char* what) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail(PESTO_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    }
    // the first `bytes` of item i to host memory, in stream order
    int read(int i, void* host, size_t bytes) {
        return hip_ok(hipMemcpyAsync(host, ptr<const void>(i), bytes, hipMemcpyDeviceToHost, stm), "copy to the host failed");
    }
    // the first `bytes` of a staged output to the caller's array (nothing to do on the device side)
    int fetch(int i, size_t bytes) { return items[i].own && items[i].out && bytes ? read(i, items[i].out, bytes) : 0; }
    // the device's verdict on what has been launched so far: the launch check, the first `bytes` of item i to `host` and the call's one
    // synchronisation before finish()
    int verdict(int i, void* host, size_t bytes, const char* what) {
        if (int rc = launched(what)) return rc;
        if (int rc = read(i, host, bytes)) return rc;
        const hipError_t e = hipStreamSynchronize(stm);
        return e == hipSuccess ? 0 : fail(PESTO_ERR_HIP, "%s: stream synchronisation failed: %s", what, hipGetErrorString(e));
    }
    int finish(int rc, const char* what) {
        if (rc == 0) rc = launched(what);
        if (rc == 0)
            for (const Item& it : items)
                if (it.own && it.out && it.whole) {
                    hipError_t e = hipMemcpyAsync(it.out, w + it.at, it.bytes, hipMemcpyDeviceToHost, stm);
                    if (e != hipSuccess) { rc = fail(PESTO_ERR_HIP, "%s: copy to the host failed: %s", what, hipGetErrorString(e)); break; }
                }
        if (w) (void)hipFreeAsync(w, stm);
        if (hipStreamSynchronize(stm) != hipSuccess && rc == 0) rc = fail(PESTO_ERR_HIP, "%s: stream synchronisation failed", what);
        return rc;
    }
};

}  // namespace
}  // namespace pesto
