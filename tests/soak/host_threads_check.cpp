// host_threads_check.cpp -- csrc/host_threads.h on its own, meant to be built with -fsanitize=thread (tests/test_host_cpu.py):
// parallel_for visits every index once and brings a body's exception to the caller with every thread joined, cut_at_lines cuts
// at line starts, JoinedThreads stops and joins on the way out of an exception, Once builds until a build succeeds and
// publishes what it built to readers that only look at done().
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -o host_threads_check host_threads_check.cpp && ./host_threads_check
#include "../../gtars_amd/csrc/host_threads.h"

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

using gtars::cut_at_lines;
using gtars::JoinedThreads;
using gtars::parallel_for;

static void coverage() {
    for (unsigned threads : {1u, 2u, 7u})
        for (size_t chunk : {(size_t)1, (size_t)8})
            for (size_t n : {(size_t)0, (size_t)1, (size_t)threads - 1, (size_t)threads, (size_t)threads + 1, (size_t)10007}) {
                std::vector<std::atomic<int>> seen(n);
                for (auto &s : seen) s = 0;
                parallel_for(n, threads, chunk, [&](size_t i) {
                    CHECK(i < n);
                    ++seen[i];
                });
                for (size_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
            }
}

struct Thrown : std::runtime_error {
    size_t index;
    explicit Thrown(size_t i) : std::runtime_error("thrown by a body"), index(i) {}
};

// Two indices on two threads: each body waits until the other one is under way too, so one of them runs on the caller and one on
// the worker, whichever way the scheduler hands them out; the body on the side asked for throws.
static void one_side_throws(bool the_callers) {
    const std::thread::id caller = std::this_thread::get_id();
    std::mutex mx;
    std::condition_variable cv;
    int arrived = 0;
    std::atomic<int> running{0};
    std::atomic<size_t> thrown_at{2};
    bool caught = false;
    try {
        parallel_for(2, 2, 1, [&](size_t i) {
            ++running;
            {
                std::unique_lock<std::mutex> lk(mx);
                ++arrived;
                cv.notify_all();
                cv.wait(lk, [&] { return arrived == 2; });
            }
            --running;
            if ((std::this_thread::get_id() == caller) == the_callers) {
                thrown_at = i;
                throw Thrown(i);
            }
        });
    } catch (const Thrown &e) {
        caught = true;
        CHECK(e.index == thrown_at);
        CHECK(running == 0);  // every thread is joined: no body is under way
    }
    CHECK(caught);
}

static void two_throw_one_arrives() {
    std::mutex mx;
    std::condition_variable cv;
    int arrived = 0;
    int caught = 0;
    try {
        parallel_for(2, 2, 1, [&](size_t i) {  // both bodies are under way before either throws
            {
                std::unique_lock<std::mutex> lk(mx);
                ++arrived;
                cv.notify_all();
                cv.wait(lk, [&] { return arrived == 2; });
            }
            throw Thrown(i);
        });
    } catch (const Thrown &e) {
        ++caught;
        CHECK(e.index < 2);
    }
    CHECK(caught == 1);
}

static void a_throw_stops_the_hand_out() {
    const size_t n = 1000000;
    std::atomic<size_t> ran{0};
    bool caught = false;
    try {
        parallel_for(n, 7, 1, [&](size_t i) {
            ++ran;
            if (i == 0) throw Thrown(i);
        });
    } catch (const Thrown &e) {
        caught = true;
        CHECK(e.index == 0);
    }
    CHECK(caught);
    CHECK(ran < n);
    // inline (one thread): the loop ends at the throw
    ran = 0;
    try {
        parallel_for(n, 1, 1, [&](size_t i) {
            ++ran;
            if (i == 2) throw Thrown(i);
        });
        CHECK(false);
    } catch (const Thrown &) {
        CHECK(ran == 3);
    }
}

static void cuts_ok(const std::string &text, unsigned parts) {
    const std::vector<size_t> cut = cut_at_lines(text.data(), text.size(), parts);
    CHECK(cut.size() == (size_t)parts + 1);
    CHECK(cut.front() == 0 && cut.back() == text.size());
    for (size_t i = 1; i < cut.size(); ++i) {
        CHECK(cut[i - 1] <= cut[i]);
        if (i < parts) CHECK(cut[i] == text.size() || (cut[i] > 0 && text[cut[i] - 1] == '\n'));
    }
}

static void cuts() {
    std::string lines;
    for (int i = 0; i < 100; ++i) lines += "chr1\t" + std::to_string(i * 10) + "\t" + std::to_string(i * 10 + 5) + "\n";
    const std::string one_long = "a\n" + std::string(500, 'x') + "\nb\nc\n";  // a line longer than n / parts
    for (unsigned parts : {1u, 2u, 3u, 7u, 16u, 32u}) {
        cuts_ok("", parts);
        cuts_ok("no newline at all", parts);
        cuts_ok("\n\n\n\n\n\n\n\n\n\n", parts);
        cuts_ok(one_long, parts);
        cuts_ok("x\ny\n", parts);  // more parts than lines
        cuts_ok("x\ny", parts);
        cuts_ok(lines, parts);
        cuts_ok(lines + "last line without a newline", parts);
    }
    // the chunks are the text: every line lies in exactly one of them
    const std::vector<size_t> cut = cut_at_lines(lines.data(), lines.size(), 7);
    size_t n_lines = 0;
    for (size_t k = 0; k + 1 < cut.size(); ++k)
        for (size_t i = cut[k]; i < cut[k + 1]; ++i) n_lines += lines[i] == '\n';
    CHECK(n_lines == 100);
}

static void joined_threads() {
    std::mutex mx;
    std::condition_variable cv;
    bool stop = false;
    int stops = 0;
    std::atomic<int> running{0}, finished{0};
    bool caught = false;
    try {
        JoinedThreads pool([&] {
            {
                std::lock_guard<std::mutex> lk(mx);
                stop = true;
                ++stops;
            }
            cv.notify_all();
        });
        pool.start(3, [&] {
            ++running;
            {
                std::unique_lock<std::mutex> lk(mx);
                cv.wait(lk, [&] { return stop; });
            }
            --running;
            ++finished;
        });
        throw std::runtime_error("the scope is left by an exception");
    } catch (const std::runtime_error &) {
        caught = true;
        CHECK(stops == 1);     // (read without the lock: the threads that could touch it are gone)
        CHECK(running == 0 && finished == 3);  // joined: each of the three ran to its end
    }
    CHECK(caught);
    // stop_and_join by hand, then the destructor: the stop action runs once
    stops = 0;
    stop = false;
    {
        JoinedThreads pool([&] {
            std::lock_guard<std::mutex> lk(mx);
            stop = true;
            ++stops;
        });
        pool.start(2, [&] {
            for (;;) {
                std::lock_guard<std::mutex> lk(mx);
                if (stop) return;
            }
        });
        pool.stop_and_join();
        CHECK(stops == 1);
    }
    CHECK(stops == 1);
}

// Eight threads call run() on one Once at the same moment; the builder fails on its first call and succeeds on its second.
// Two readers never take the mutex: they spin on done() and then read what the builder stored (plain int: a done() that
// did not order the read behind the builder's write is a race ThreadSanitizer reports).
static void once_guard() {
    gtars::Once once;
    int value = 0;
    std::atomic<int> builds{0}, failed{0}, succeeded{0};
    std::atomic<bool> go{false};
    auto builder = [&]() -> int {
        if (++builds == 1) return 7;  // (the guard stays clear: the next caller builds again)
        value = 42;
        return 0;
    };
    {
        JoinedThreads th([] {});
        th.start(8, [&] {
            while (!go.load()) std::this_thread::yield();
            const int st = once.run(builder);
            if (st) {
                CHECK(st == 7);
                ++failed;
            } else {
                CHECK(once.done() && value == 42);
                ++succeeded;
            }
        });
        th.start(2, [&] {
            while (!once.done()) std::this_thread::yield();
            CHECK(value == 42);
        });
        CHECK(!once.done());
        go.store(true);
    }
    CHECK(builds == 2);  // one failure, one success, six calls that found it done
    CHECK(failed == 1 && succeeded == 7);
    CHECK(once.run([&]() -> int { return ++builds; }) == 0);  // done: returns 0 and does not call the builder
    CHECK(builds == 2 && once.done() && value == 42);
}

int main() {
    coverage();
    for (int rep = 0; rep < 20; ++rep) once_guard();
    for (int rep = 0; rep < 20; ++rep) {
        one_side_throws(false);
        one_side_throws(true);
        two_throw_one_arrives();
    }
    a_throw_stops_the_hand_out();
    cuts();
    joined_threads();
    printf("host_threads: all checks passed\n");
    return 0;
}
