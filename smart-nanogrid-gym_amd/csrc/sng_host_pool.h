// sng_host_pool.h -- the host worker threads of the library: how many, the pool that keeps them, and
// parallel_ranges over it.  Host only, no HIP: it compiles with plain g++ (tests/native/host_pool_check.cpp
// stresses the pool on the CPU).
#pragma once
#include <sched.h>
#include <stdint.h>

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace sng {

// Host threads for the reference-RNG day generator and the scenario encoder: the CPUs this process
// may run on (sched_getaffinity), capped by SNG_HOST_THREADS or OMP_NUM_THREADS when set (a GPU box
// shows the whole machine's CPUs but gives one process a share of them).
static inline int host_threads() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    for (const char *var : {"SNG_HOST_THREADS", "OMP_NUM_THREADS"}) {
        const char *v = std::getenv(var);
        if (v && std::atoi(v) > 0) {
            n = std::min(n, std::atoi(v));
            break;
        }
    }
    return std::max(1, std::min(n, 64));
}

// A process-wide pool of host worker threads, started on first use and kept for the life of the
// process (never destroyed, so no worker is joined or torn down during static destruction).  A reset
// of 65,536 envs draws the Python-stream PV ratios in ~0.1 ms of work per thread; starting 15 threads
// for every reset cost more than the work.  (Hidden: one pool for the whole library, not an export of it.)
class __attribute__((visibility("hidden"))) HostPool {
  public:
    static HostPool &get() {
        static HostPool *pool = new HostPool();
        return *pool;
    }
    // run job(k) for k in [0, parts) on the pool plus the calling thread; returns when all are done
    void run(int parts, const std::function<void(int)> &job) {
        std::unique_lock<std::mutex> call(call_mu_);   // one parallel section at a time
        grow(parts - 1);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &job;
            parts_ = parts;
            next_ = 1;   // part 0 is the caller's
            done_ = 0;
            ++gen_;
        }
        cv_.notify_all();
        job(0);
        int k;
        while ((k = claim()) >= 0) {
            job(k);
            std::lock_guard<std::mutex> lk(mu_);
            ++done_;   // parts 1 .. parts - 1 count as done, whoever ran them
        }
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return done_ == parts_ - 1; });
        job_ = nullptr;
    }

  private:
    int claim() {
        std::lock_guard<std::mutex> lk(mu_);
        return next_ < parts_ ? next_++ : -1;
    }
    void grow(int want) {
        while ((int)workers_.size() < want) workers_.push_back(new std::thread([this] { loop(); }));
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *job;
            int k;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen && job_ && next_ < parts_; });
                seen = gen_;
                job = job_;
                k = next_++;
            }
            for (;;) {
                (*job)(k);
                std::lock_guard<std::mutex> lk(mu_);
                ++done_;
                if (done_ == parts_ - 1) done_cv_.notify_one();
                if (next_ >= parts_) break;
                k = next_++;
            }
        }
    }
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread *> workers_;
    const std::function<void(int)> *job_ = nullptr;
    int parts_ = 0, next_ = 0, done_ = 0;
    uint64_t gen_ = 0;
};

// fn(begin, end) over [0, n) in contiguous ranges on up to `threads` threads of the pool (the calling
// thread takes a range too); serial below `grain` items per thread.
template <class Fn>
static void parallel_ranges_on(int threads, int64_t n, int64_t grain, Fn &&fn) {
    const int nt = (int)std::min<int64_t>(threads, std::max<int64_t>(1, n / grain));
    if (nt <= 1) {
        fn((int64_t)0, n);
        return;
    }
    const int64_t per = (n + nt - 1) / nt;
    HostPool::get().run(nt, [&](int k) {
        const int64_t b = k * per, en = std::min(n, b + per);
        if (b < en) fn(b, en);
    });
}
// ... on host_threads() threads
template <class Fn>
static void parallel_ranges(int64_t n, int64_t grain, Fn &&fn) {
    parallel_ranges_on(host_threads(), n, grain, fn);
}

}  // namespace sng
