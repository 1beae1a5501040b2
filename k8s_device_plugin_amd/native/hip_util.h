// Host-side HIP scaffolding shared by health_probe.hip and the sweeps:
// a throwing HIP_CHECK, RAII device buffer and event pair with the one
// "record, run, record, sync, elapsed" timing helper, and timed_ms on top.
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

    // The milliseconds that launch() takes on the current device's null
    // stream between the two events; a launch that failed throws.
    template <typename Launch>
    float time(Launch &&launch) {
        HIP_CHECK(hipEventRecord(start));
        launch();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(stop));
        HIP_CHECK(hipEventSynchronize(stop));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, start, stop));
        return ms;
    }
};

// Runs warmup(), drains the device, then returns the milliseconds that
// timed() takes on the current device's null stream between two events.
template <typename Warmup, typename Timed>
float timed_ms(Warmup &&warmup, Timed &&timed) {
    warmup();
    HIP_CHECK(hipDeviceSynchronize());
    return EventPair().time(timed);
}
