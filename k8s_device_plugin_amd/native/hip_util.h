// Host-side HIP scaffolding shared by health_probe.hip and the sweeps:
// a throwing HIP_CHECK, RAII device buffer and event pair, and the one
// "warm up, record, run, record, sync, elapsed" timing helper.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define HIP_CHECK(expr)                                                        \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess)                                                  \
            throw std::runtime_error(std::string("HIP error at " #expr ": ") + \
                                     hipGetErrorString(_e));                   \
    } while (0)

// count elements of T in device memory, freed on scope exit (also when a
// later HIP_CHECK throws).
template <typename T>
class DeviceBuffer {
  public:
    explicit DeviceBuffer(size_t count) {
        HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ptr_), count * sizeof(T)));
    }
    ~DeviceBuffer() { (void)hipFree(ptr_); }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    T *get() const { return ptr_; }

  private:
    T *ptr_ = nullptr;
};

struct EventPair {
    hipEvent_t start = nullptr, stop = nullptr;
    EventPair() {
        HIP_CHECK(hipEventCreate(&start));
        hipError_t e = hipEventCreate(&stop);
        if (e != hipSuccess) {  // no destructor runs for a throwing constructor
            (void)hipEventDestroy(start);
            HIP_CHECK(e);
        }
    }
    ~EventPair() {
        (void)hipEventDestroy(start);
        (void)hipEventDestroy(stop);
    }
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
};

// Runs warmup(), drains the device, then returns the milliseconds that
// timed() takes on the current device's null stream between two events.
template <typename Warmup, typename Timed>
float timed_ms(Warmup &&warmup, Timed &&timed) {
    warmup();
    HIP_CHECK(hipDeviceSynchronize());
    EventPair ev;
    HIP_CHECK(hipEventRecord(ev.start));
    timed();
    HIP_CHECK(hipEventRecord(ev.stop));
    HIP_CHECK(hipEventSynchronize(ev.stop));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev.start, ev.stop));
    return ms;
}
