// hfv_host_pipe.h -- the host control flow of the host-memory paths (hfv_host_path.cpp), free of HIP so
// that a plain host program can run it (tests/host_pipe_driver.cpp): the worker pool of the staging
// copies, parallel_rows over it, and the two-slot chunk schedule all three chunked calls run on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// HFV_MUT_HOSTCHUNK (make hostchunk; 0 in every product build): see hfv_host_path.cpp.  Number 1 is here.
#ifndef HFV_MUT_HOSTCHUNK
#define HFV_MUT_HOSTCHUNK 0
#endif

// Library code, none of it part of the ABI.
#pragma GCC visibility push(hidden)
namespace hfv {

// Persistent host worker threads for the staging copies (spawning threads per copy cost more
// than the copies: 32 spawns per 2^20-frame router batch).  Part 0 of every job runs on the
// calling thread, parts 1..nt-1 on the workers, each of which calls on_start (nullable) once
// before its first job.  Jobs come from one ctx thread at a time.
class HostPool {
  public:
    HostPool(int nt, void (*on_start)()) : nt_(nt)
    {
        for (int k = 1; k < nt_; ++k) th_.emplace_back([this, k, on_start] {
            if (on_start) on_start();
            work(k);
        });
    }
    ~HostPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run(size_t n, const std::function<void(size_t, size_t)> &fn)
    {
        std::unique_lock<std::mutex> lk(job_m_);   // one job at a time
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            n_ = n;
            left_ = nt_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        fn(0, n / nt_);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return left_ == 0; });
        fn_ = nullptr;
    }
    int threads() const { return nt_; }

  private:
    void work(int k)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)> *fn;
            size_t n;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                fn = fn_;
                n = n_;
            }
            (*fn)(n * k / nt_, n * (k + 1) / nt_);
            std::lock_guard<std::mutex> g(m_);
            if (--left_ == 0) done_.notify_one();
        }
    }
    int nt_;
    std::vector<std::thread> th_;
    std::mutex m_, job_m_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t n_ = 0;
    int left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// fn(a, b) over [0, n) split into `threads` contiguous parts on pool() (a HostPool of that many
// threads, first asked for when a job needs it); inline with one thread or below inline_below items.
template <class Pool, class F>
static inline void parallel_rows(int threads, size_t inline_below, Pool pool, size_t n, F fn)
{
    if (threads <= 1 || n < inline_below) {
        fn((size_t)0, n);
        return;
    }
    pool().run(n, std::function<void(size_t, size_t)>(fn));
}

// Chunks of `chunk` items over [0, n) on two alternating slots: before chunk c is submitted on
// slot c & 1, chunk c - 2 (same slot) is waited for and retired; the last two are retired at the end.
// wait(sl), submit(sl, first, cnt) and retire(sl, first, cnt) return an int: the first that is not 0
// ends the loop and is returned.  *reuses (nullable) counts the chunks submitted on a slot that the
// call had used before.
template <class Wait, class Submit, class Retire>
static inline int two_slot_chunks(size_t n, size_t chunk, Wait wait, Submit submit, Retire retire, uint64_t *reuses)
{
    const size_t nchunks = (n + chunk - 1) / chunk;
    size_t at[2] = {0, 0}, len[2] = {0, 0};   // the chunk in flight on each slot
    for (size_t c = 0; c < nchunks + 2; ++c) {
        const int sl = (int)(c & 1);
        if (c >= 2) {
            int rc = wait(sl);
            if (rc) return rc;
            size_t first = at[sl], cnt = len[sl];
            if (HFV_MUT_HOSTCHUNK == 1) {   // the other slot's place, cut at n
                first = at[sl ^ 1];
                if (cnt > n - first) cnt = n - first;
            }
            rc = retire(sl, first, cnt);
            if (rc) return rc;
        }
        if (c >= nchunks) continue;
        if (c >= 2 && reuses) ++*reuses;
        const size_t first = c * chunk, cnt = n - first < chunk ? n - first : chunk;
        int rc = submit(sl, first, cnt);
        if (rc) return rc;
        at[sl] = first;
        len[sl] = cnt;
    }
    return 0;
}

}  // namespace hfv
#pragma GCC visibility pop
