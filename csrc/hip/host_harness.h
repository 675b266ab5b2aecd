// Host-side harness of the single-kernel ops (ops.cpp) and the micro-benchmarks (engine_bench.cpp,
// the bindings): the stream and device allocations of one call (Scratch) and the two timing
// sequences (timeEagerUs, timeGraphUs). Whatever a call creates here is released on scope exit,
// also when a DL_HIP or DL_CHECK throws half-way. Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "device_comm.h"

namespace dl {

// Device allocations of one op call, released on scope exit.
class Scratch {
  public:
    Scratch() { DL_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~Scratch() {
        for (void *p : mem_) (void)hipFree(p);
        (void)hipStreamDestroy(s);
    }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    // not zero-filled: an operand that a fill kernel, a copy or the launch itself writes whole
    template <typename T>
    T *allocRaw(size_t count) {
        void *p = nullptr;
        DL_HIP(hipMalloc(&p, bytesOf<T>(count)));
        mem_.push_back(p);
        return static_cast<T *>(p);
    }
    template <typename T>
    T *alloc(size_t count) {
        T *p = allocRaw<T>(count);
        DL_HIP(hipMemsetAsync(p, 0, bytesOf<T>(count), s));
        return p;
    }
    template <typename T>
    T *upload(const std::vector<T> &v) {
        if (v.empty()) return nullptr;
        T *p = alloc<T>(v.size());
        DL_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        return p;
    }
    template <typename T>
    std::vector<T> download(const T *p, size_t count) {
        std::vector<T> v(count);
        DL_HIP(hipMemcpyAsync(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost, s));
        DL_HIP(hipStreamSynchronize(s));
        return v;
    }
    void sync() {
        DL_HIP(hipGetLastError());
        DL_HIP(hipStreamSynchronize(s));
    }
    // Output buffer of `rows` rows of `ld` elements of which the first `valid` are results and the
    // rest (ld - valid >= one workgroup's rows) guard, every byte preset to kGuardByte (a result
    // the launch never wrote reads back as NaN). checkGuards() throws when a launch changed a
    // guard byte: a store past the last valid row of an op is an error, not silent corruption.
    static constexpr uint8_t kGuardByte = 0xFF;
    template <typename T>
    T *allocGuarded(size_t rows, size_t valid, size_t ld, const char *what) {
        DL_CHECK(ld > valid && rows > 0, "guarded buffer needs a guard region");
        T *p = allocRaw<T>(rows * ld);
        DL_HIP(hipMemsetAsync(p, kGuardByte, rows * ld * sizeof(T), s));
        guards_.push_back({reinterpret_cast<uint8_t *>(p), rows, valid * sizeof(T), ld * sizeof(T), what});
        return p;
    }
    // ... followed by `tail` whole guard rows (a store to a row past the last valid one); here the
    // rows may be all valid (ld == valid: no room for a guard inside the row)
    template <typename T>
    T *allocGuardedTail(size_t rows, size_t valid, size_t ld, size_t tail, const char *what) {
        DL_CHECK(ld >= valid && rows > 0 && tail > 0, "guarded buffer needs a guard region");
        T *p = allocRaw<T>((rows + tail) * ld);
        DL_HIP(hipMemsetAsync(p, kGuardByte, (rows + tail) * ld * sizeof(T), s));
        uint8_t *b = reinterpret_cast<uint8_t *>(p);
        guards_.push_back({b, rows, valid * sizeof(T), ld * sizeof(T), what});
        guards_.push_back({b + rows * ld * sizeof(T), tail, 0, ld * sizeof(T), what});
        return p;
    }
    // The rows of an in-place op (or the preset of an output), packed, with `tail` guard elements
    // behind the last row.
    template <typename T>
    T *uploadGuardedTail(const std::vector<T> &v, size_t tail, const char *what) {
        T *p = allocGuarded<T>(1, v.size(), v.size() + tail, what);
        DL_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        return p;
    }
    void checkGuards() {
        for (const Guard &g : guards_) {
            const std::vector<uint8_t> v = download(g.p, g.rows * g.ld);
            for (size_t r = 0; r < g.rows; r++)
                for (size_t i = g.valid; i < g.ld; i++)
                    DL_CHECK(v[r * g.ld + i] == kGuardByte,
                             std::string("ops: the launch wrote past the valid part of ") + g.what + " (row " +
                                 std::to_string(r) + ", byte " + std::to_string(i - g.valid) + " of its guard)");
        }
    }
    // the valid part of a guarded buffer, rows packed
    template <typename T>
    std::vector<T> downloadRows(const T *p, size_t rows, size_t valid, size_t ld) {
        const std::vector<T> all = download(p, rows * ld);
        std::vector<T> v(rows * valid);
        for (size_t r = 0; r < rows; r++) std::copy(all.begin() + r * ld, all.begin() + r * ld + valid, v.begin() + r * valid);
        return v;
    }
    hipStream_t s = nullptr;

  private:
    template <typename T>
    static size_t bytesOf(size_t count) {
        return count * sizeof(T) < 16 ? 16 : count * sizeof(T);
    }
    struct Guard {
        uint8_t *p;
        size_t rows, valid, ld;  // bytes
        const char *what;
    };
    std::vector<void *> mem_;
    std::vector<Guard> guards_;
};

// A timing event, destroyed on scope exit.
struct TimingEvent {
    TimingEvent() { DL_HIP(hipEventCreate(&e)); }
    ~TimingEvent() { (void)hipEventDestroy(e); }
    TimingEvent(const TimingEvent &) = delete;
    TimingEvent &operator=(const TimingEvent &) = delete;
    // microseconds from `start` to this event, once this one has happened
    double usSince(const TimingEvent &start) {
        DL_HIP(hipEventSynchronize(e));
        float ms = 0;
        DL_HIP(hipEventElapsedTime(&ms, start.e, e));
        return (double)ms * 1000.0;
    }
    hipEvent_t e = nullptr;
};

// The launches that `record()` enqueues on `s`, captured (thread-local mode) into one graph and
// instantiated; graph and executable live until scope exit. A throwing record() ends the capture.
struct CapturedGraph {
    CapturedGraph() = default;
    ~CapturedGraph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
    CapturedGraph(const CapturedGraph &) = delete;
    CapturedGraph &operator=(const CapturedGraph &) = delete;
    template <typename Record>
    void capture(hipStream_t s, Record record) {
        DL_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
            record();
        } catch (...) {
            (void)hipStreamEndCapture(s, &graph);
            throw;
        }
        DL_HIP(hipStreamEndCapture(s, &graph));
        DL_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    }
    void launch(hipStream_t s) { DL_HIP(hipGraphLaunch(exec, s)); }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// Microseconds per launch() of `iters` back-to-back eager launches on `s`, between two events,
// after `warmups` untimed ones.
template <typename Launch>
double timeEagerUs(hipStream_t s, int iters, int warmups, Launch launch) {
    TimingEvent e0, e1;
    for (int i = 0; i < warmups; i++) launch();
    DL_HIP(hipEventRecord(e0.e, s));
    for (int i = 0; i < iters; i++) launch();
    DL_HIP(hipEventRecord(e1.e, s));
    return e1.usSince(e0) / iters;
}

// Microseconds per launch(i) of one graph of launch(0) .. launch(iters - 1), a serial chain on `s`:
// one eager launch(0) (its launch error surfaces here, not inside the capture), the capture, one
// warm replay, then one replay between two events.
template <typename Launch>
double timeGraphUs(hipStream_t s, int iters, Launch launch) {
    launch(0);
    DL_HIP(hipGetLastError());
    CapturedGraph g;
    g.capture(s, [&] {
        for (int i = 0; i < iters; i++) launch(i);
    });
    g.launch(s);
    DL_HIP(hipStreamSynchronize(s));
    TimingEvent e0, e1;
    DL_HIP(hipEventRecord(e0.e, s));
    g.launch(s);
    DL_HIP(hipEventRecord(e1.e, s));
    return e1.usSince(e0) / iters;
}

}  // namespace dl
