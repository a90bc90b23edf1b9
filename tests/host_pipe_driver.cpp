// The host control flow of the host-memory paths (csrc/hfv_host_pipe.h) run as a plain host program,
// for tests/test_host_chunks.py, which builds it under the thread sanitizer and under the address and
// undefined-behaviour sanitizers:
//   sched N CHUNK [N CHUNK ...]   two_slot_chunks' calls in order, one per line, then "end RC REUSES"
//   fail N CHUNK K CODE           the same with submit returning CODE on chunk K
//   pool                          parallel_rows and HostPool::run touch every row exactly once
//   stress JOBS                   JOBS back-to-back jobs on one pool of 8 threads
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "hfv_host_pipe.h"

using namespace hfv;

static int schedule(size_t n, size_t chunk, long fail_chunk, int code)
{
    uint64_t reuses = 0;
    printf("case %zu %zu\n", n, chunk);
    int rc = two_slot_chunks(
        n, chunk,
        [&](int sl) {
            printf("wait %d\n", sl);
            return 0;
        },
        [&](int sl, size_t first, size_t cnt) {
            printf("launch %d %zu %zu\n", sl, first, cnt);
            return (long)(first / chunk) == fail_chunk ? code : 0;
        },
        [&](int sl, size_t first, size_t cnt) {
            printf("retire %d %zu %zu\n", sl, first, cnt);
            return 0;
        },
        &reuses);
    printf("end %d %llu\n", rc, (unsigned long long)reuses);
    return 0;
}

static std::atomic<int> g_started{0};
static void on_start() { ++g_started; }

// Plain (not atomic) counters: two parts that overlapped would also be a data race.
static bool touched_once(const std::vector<int> &seen)
{
    for (int v : seen)
        if (v != 1) return false;
    return true;
}

static int pool()
{
    const int threads[] = {1, 3, 8};
    const size_t sizes[] = {0, 1, 7, 8, 4097};
    int workers = 0;
    for (int nt : threads) {
        HostPool p(nt, on_start);
        workers += nt - 1;
        if (p.threads() != nt) return 1;
        for (size_t n : sizes) {
            for (size_t inline_below : {(size_t)0, (size_t)8}) {
                std::vector<int> seen(n, 0);
                parallel_rows(nt, inline_below, [&]() -> HostPool & { return p; }, n, [&](size_t a, size_t b) {
                    for (size_t i = a; i < b; ++i) ++seen[i];
                });
                if (!touched_once(seen)) return fprintf(stderr, "parallel_rows: %d threads, %zu rows\n", nt, n), 1;
            }
            std::vector<int> seen(n, 0);
            std::atomic<int> parts{0};
            p.run(n, [&](size_t a, size_t b) {
                ++parts;
                for (size_t i = a; i < b; ++i) ++seen[i];
            });
            if (!touched_once(seen) || parts != nt) return fprintf(stderr, "run: %d threads, %zu rows\n", nt, n), 1;
        }
    }
    // every worker called on_start, once (the pools are joined: their workers have all started)
    if (g_started != workers) return fprintf(stderr, "on_start ran %d times for %d workers\n", (int)g_started, workers), 1;
    HostPool quiet(3, nullptr);   // no start function, no job
    printf("pool ok\n");
    return 0;
}

static int stress(size_t jobs)
{
    HostPool p(8, nullptr);
    std::vector<uint64_t> acc(64, 0);
    for (size_t j = 0; j < jobs; ++j)
        p.run(acc.size(), [&](size_t a, size_t b) {
            for (size_t i = a; i < b; ++i) acc[i] += j + i;
        });
    for (size_t i = 0; i < acc.size(); ++i)
        if (acc[i] != jobs * (jobs - 1) / 2 + jobs * i) return fprintf(stderr, "stress: row %zu\n", i), 1;
    printf("stress ok %zu\n", jobs);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "sched") && argc % 2 == 0) {
        for (int k = 2; k + 1 < argc; k += 2) schedule(strtoull(argv[k], nullptr, 10), strtoull(argv[k + 1], nullptr, 10), -1, 0);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "fail"))
        return schedule(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), atol(argv[4]), atoi(argv[5]));
    if (argc == 2 && !strcmp(argv[1], "pool")) return pool();
    if (argc == 3 && !strcmp(argv[1], "stress")) return stress(strtoull(argv[2], nullptr, 10));
    fprintf(stderr, "usage: see the head of host_pipe_driver.cpp\n");
    return 2;
}
