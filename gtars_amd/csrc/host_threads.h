// host_threads.h -- every host thread of the library is started here.  Plain C++17: no HIP, no GTARS_* switches; the caller
// passes the thread count (host_thread_budget(cap) / gtars_host_threads(cap)).
//
// The exception rule: no exception ever meets a joinable std::thread, and none ends on a worker.  parallel_for joins every
// thread it started and then rethrows a body's first exception on the CALLER, whichever thread ran that body -- so it reaches
// the guard of the C entry point like any exception of the calling thread.  Threads that outlive one loop belong to a
// JoinedThreads, whose destructor stops and joins them on every way out of the scope; their bodies must not throw.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace gtars {

// Threads that outlive one loop (a pool of loaders, the workers of a queue) and what makes them return: the destructor runs
// the stop action, then joins -- on a return and on an exception alike.  The stop action and the thread bodies must not throw.
class JoinedThreads {
  public:
    explicit JoinedThreads(std::function<void()> stop) : stop_(std::move(stop)) {}
    ~JoinedThreads() { stop_and_join(); }
    template <class F>
    void start(unsigned n, const F &body) {  // (a thread that cannot be started throws; the ones before it are still owned)
        th_.reserve(th_.size() + n);
        for (unsigned k = 0; k < n; ++k) th_.emplace_back(body);
    }
    void stop_and_join() {
        if (th_.empty()) return;
        stop_();
        for (std::thread &t : th_) t.join();
        th_.clear();
    }

  private:
    std::function<void()> stop_;
    std::vector<std::thread> th_;
};

// body(i) for every i in [0, n), on at most `threads` threads of which the caller is one; a thread takes `chunk` consecutive
// indices at a time (small chunks where the indices differ a lot in cost).  One thread, or n <= chunk: inline, nothing is
// started.  A body that throws ends the hand-out of indices; bodies already running finish, every thread is joined, and the
// first exception is rethrown here.
template <class F>
void parallel_for(size_t n, unsigned threads, size_t chunk, F &&body) {
    chunk = std::max<size_t>(chunk, 1);
    const size_t nt = std::min<size_t>(threads, n / chunk + (n % chunk != 0));
    if (nt <= 1) {
        for (size_t i = 0; i < n; ++i) body(i);
        return;
    }
    std::atomic<size_t> next{0};
    std::atomic<bool> stop{false};
    std::mutex mx;
    std::exception_ptr first;
    auto work = [&]() noexcept {
        try {
            while (!stop.load()) {
                const size_t i0 = next.fetch_add(chunk);
                if (i0 >= n) return;
                for (size_t i = i0; i < std::min(n, i0 + chunk); ++i) body(i);
            }
        } catch (...) {
            stop.store(true);
            std::lock_guard<std::mutex> lk(mx);
            if (!first) first = std::current_exception();
        }
    };
    {
        // (the stop action matters when a thread cannot be started; once work() has returned every index is handed out)
        JoinedThreads th([&] { stop.store(true); });
        th.start((unsigned)nt - 1, work);
        work();
    }
    if (first) std::rethrow_exception(first);
}

// Something built on first use and read by any thread afterwards.  run(build): under the mutex, returns 0 at once when the
// build has succeeded before; otherwise calls build(), whose status it returns -- 0 publishes what build() wrote (release),
// anything else leaves the guard clear, so a later call tries again.  done() is the matching acquire load: a thread that
// sees true also sees everything the successful build() wrote, without taking the mutex.
class Once {
  public:
    template <class F>
    auto run(F &&build) -> decltype(build()) {
        std::lock_guard<std::mutex> lk(mu_);
        if (done_.load(std::memory_order_relaxed)) return {};
        const auto st = build();
        if (!st) done_.store(true, std::memory_order_release);
        return st;
    }
    bool done() const { return done_.load(std::memory_order_acquire); }

  private:
    std::mutex mu_;
    std::atomic<bool> done_{false};
};

// `parts` + 1 ascending offsets into text[0, n): the first is 0, the last n, every other one lies just behind a '\n' (or is n) --
// the text cut at line starts into `parts` chunks of about n / parts bytes.  A cut never lies in front of the one before it:
// behind a line longer than a chunk the next cut is the next line start.
inline std::vector<size_t> cut_at_lines(const char *text, size_t n, unsigned parts) {
    parts = std::max(parts, 1u);
    std::vector<size_t> cut(parts + 1, n);
    cut[0] = 0;
    for (unsigned i = 1; i < parts; ++i) {
        const size_t at = std::max(cut[i - 1], n / parts * i);
        const char *nl = at < n ? (const char *)memchr(text + at, '\n', n - at) : nullptr;
        cut[i] = nl ? (size_t)(nl - text) + 1 : n;
    }
    return cut;
}

}  // namespace gtars
