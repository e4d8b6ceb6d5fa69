// Error plumbing and small RAII helpers shared by the host drivers.
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/plp_front.h"

namespace plp {

plp_status set_error(plp_status s, const char* msg);
plp_status set_hip_error(hipError_t e, const char* expr, const char* file, int line);

#define PLP_HIP(expr)                                                                 \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) return ::plp::set_hip_error(_e, #expr, __FILE__, __LINE__); \
    } while (0)
#define PLP_TRY(expr)                        \
    do {                                     \
        plp_status _s = (expr);              \
        if (_s != PLP_OK) return _s;         \
    } while (0)

// Grow-only device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }   // (hipFree waits for the device's outstanding work)
    hipError_t upload(const void* src, size_t n, hipStream_t st) {
        hipError_t e = reserve(n);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, st);
    }
};

// Page-locked bounce buffer of a context for the host-pointer entry points: the caller's image is copied into it by the CPU and
// goes to the device from there, so that no DMA / blit ever addresses the caller's pageable memory (whose pages the caller may
// unmap right after the call; a randomised sweep that allocated a fresh image per call hit rare GPU page faults otherwise).
struct HostPinned {
    void* p = nullptr;
    size_t bytes = 0;
    HostPinned() = default;
    HostPinned(const HostPinned&) = delete;
    HostPinned& operator=(const HostPinned&) = delete;
    ~HostPinned() { if (p) (void)hipHostFree(p); }
    hipError_t reserve(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { hipError_t e = hipHostFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        if (n == 0) n = 16;
        // one page of slack behind the payload: a copy engine / blit kernel that fetches its source in 16-byte (or wider) pieces may
        // touch a few bytes past the last requested one, and the page after a host allocation need not be mapped
        hipError_t e = hipHostMalloc(&p, n + 4096, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    // rows x cols bytes from a pitched host image into the buffer at byte offset off, densely packed (pitch = cols)
    void pack(size_t off, const uint8_t* src, size_t step, int rows, int cols) {
        uint8_t* d = static_cast<uint8_t*>(p) + off;
        if (step == (size_t)cols) memcpy(d, src, (size_t)rows * cols);
        else for (int y = 0; y < rows; ++y) memcpy(d + (size_t)y * cols, src + (size_t)y * step, (size_t)cols);
    }
};

// The arrays of one host-pointer entry, staged through a context's slab.  For the matcher context the declarations are a call's plan
// (matcher_context.hpp), which host_call() runs with a Stage and device_call() with a DeviceRooms, so that both forms of an entry read one
// list.  Every array is declared once, by reference to the pointer field of the kernel-argument struct that holds its HOST address, with its
// element count (bytes = count * sizeof(T)):
//   in    uploaded;
//   out   downloaded by finish().  keep: uploaded first, as the caller holds it.  The kernels write only the slots they compute (below a
//         problem's count, not skipped), and finish() copies the whole block back, so the unwritten slots must hold the caller's values, as
//         on the device entry (plp_front.h), not what an earlier call left in the slab.  keep = false is for an array every slot of which
//         the kernel writes;
//   room  a device-only region (scratch, an image packed elsewhere); the pointer's old value is ignored.
// upload() lays the arrays out in the order declared, 256-byte aligned, reserves the slab, rewrites every declared pointer to its device
// address and issues the host-to-device copies.  A NULL pointer or a count of 0 is not staged: the kernel sees NULL for it.
// finish() issues the device-to-host copies and waits for the stream.  The slab must not be reserved again in between.
// Nothing checks that every pointer field of an argument struct was declared: a field left out of the plan reaches the kernel as the caller's
// HOST address.  After upload() a declared pointer is a device address, whatever its name: host code must not dereference it.
class Stage {
public:
    Stage(DevBuf& slab, hipStream_t st) : slab_(slab), st_(st) { parts_.reserve(32); }
    template <class T> void in(const T*& p, size_t count) { parts_.push_back({&p, p, nullptr, p ? count * sizeof(T) : 0, 0}); }
    template <class T> void out(T*& p, size_t count, bool keep = true) { parts_.push_back({&p, keep ? p : nullptr, p, p ? count * sizeof(T) : 0, 0}); }
    template <class T> void room(T*& p, size_t count) { parts_.push_back({&p, nullptr, nullptr, count * sizeof(T), 0}); }
    template <class T> void room(DevBuf&, T*& p, size_t count) { parts_.push_back({&p, nullptr, nullptr, count * sizeof(T), 0}); }   // a plan's room (matcher_context.hpp): the slab serves, not the context's buffer
    plp_status upload() {
        size_t tot = 0;
        for (Part& p : parts_) { p.off = tot; tot += (p.bytes + 255) / 256 * 256; }
        PLP_HIP(slab_.reserve(tot));
        for (const Part& p : parts_) {
            void* d = p.bytes ? static_cast<uint8_t*>(slab_.p) + p.off : nullptr;
            memcpy(p.field, &d, sizeof d);   // the field is a `T*` or `const T*` object: same representation
            if (d && p.src) PLP_HIP(hipMemcpyAsync(d, p.src, p.bytes, hipMemcpyHostToDevice, st_));
        }
        return PLP_OK;
    }
    plp_status finish() {
        for (const Part& p : parts_)
            if (p.bytes && p.dst) PLP_HIP(hipMemcpyAsync(p.dst, static_cast<uint8_t*>(slab_.p) + p.off, p.bytes, hipMemcpyDeviceToHost, st_));
        PLP_HIP(hipStreamSynchronize(st_));
        return PLP_OK;
    }

private:
    struct Part { void* field; const void* src; void* dst; size_t bytes; size_t off; };   // src: uploaded from; dst: downloaded to
    DevBuf& slab_;
    hipStream_t st_;
    std::vector<Part> parts_;
};

}  // namespace plp
