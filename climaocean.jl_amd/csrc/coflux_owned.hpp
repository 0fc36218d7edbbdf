// coflux_owned.hpp — the single owner of every device resource of the host layer (coflux_ctx.hpp includes it; nothing else
// does).  A resource is held by exactly one Owned member or local: it is released when that owner is reset, assigned to or
// destroyed, and by nothing else — no error path and no teardown code frees by hand.  Owners are empty by default, move-only
// and never throw; every create… returns the HIP error and leaves the owner EMPTY on failure, so "is it there" is one test.
// What kernels and device-visible structs see stays a raw pointer taken from get(); the owner lives beside it.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace cf {

template <class Handle, hipError_t (*Release)(Handle)>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, Handle{})) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, Handle{});
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }

    Handle get() const { return h_; }
    explicit operator bool() const { return h_ != Handle{}; }
    void reset() {
        if (h_ != Handle{}) (void)Release(h_);
        h_ = Handle{};
    }

protected:
    // create… is `return keep(hipX(fresh(), …))`: what was held is released first, a failed call leaves the owner empty
    Handle* fresh() {
        reset();
        return &h_;
    }
    hipError_t keep(hipError_t e) {
        if (e != hipSuccess) h_ = Handle{};
        return e;
    }

private:
    Handle h_{};
};

// Device memory on the current device.  hipFree waits for the device: work still in flight on the buffer has finished
// before it goes.  The fine-grained flavour is what a peer's stores and the owner's polling loads need to meet in memory.
template <class T = void>
struct DeviceBuffer : Owned<void*, hipFree> {
    hipError_t create(size_t bytes) { return keep(hipMalloc(fresh(), bytes)); }
    hipError_t create_fine_grained(size_t bytes) { return keep(hipExtMallocWithFlags(fresh(), bytes, hipDeviceMallocFinegrained)); }
    T* get() const { return static_cast<T*>(Owned::get()); }
};

// One allocation carved into pieces: add() each piece's bytes in order and keep the offset it returns, create bytes, then
// at<T>(base, offset).  Every piece starts 16-byte aligned within the allocation.
struct Layout {
    size_t bytes = 0;
    size_t add(size_t n) {
        const size_t at = bytes;
        bytes += (n + 15) & ~(size_t)15;
        return at;
    }
    template <class T>
    static T* at(void* base, size_t offset) {
        return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + offset);
    }
};

template <class T = void>
struct PinnedBuffer : Owned<void*, hipHostFree> {
    hipError_t create(size_t bytes) { return keep(hipHostMalloc(fresh(), bytes, hipHostMallocDefault)); }
    T* get() const { return static_cast<T*>(Owned::get()); }
};

// a non-blocking stream on the current device (the caller synchronises it before the release where work may be queued)
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return keep(hipStreamCreateWithFlags(fresh(), hipStreamNonBlocking)); }
};

// hipEventDisableTiming for ordering, hipEventDefault where elapsed times are read
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags) { return keep(hipEventCreateWithFlags(fresh(), flags)); }
};

// another process's device allocation, mapped through HIP IPC
struct IpcMapping : Owned<void*, hipIpcCloseMemHandle> {
    hipError_t create(const hipIpcMemHandle_t& handle) { return keep(hipIpcOpenMemHandle(fresh(), handle, hipIpcMemLazyEnablePeerAccess)); }
};

}  // namespace cf
