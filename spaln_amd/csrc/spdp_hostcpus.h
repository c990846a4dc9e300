// spdp_hostcpus.h -- how many host threads are worth starting, and a "parallel for" over them
#ifndef SPDP_HOSTCPUS_H_
#define SPDP_HOSTCPUS_H_
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

// CPUs this process may actually use: the affinity mask, capped by the cgroup CPU quota (a container on a 256-thread host
// may be granted 16 CPUs worth of time: more runnable threads than that only contend)
static inline int spdp_host_cpus()
{
    int n = (int) std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min(n > 0 ? n : 1 << 20, (int) CPU_COUNT(&set));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0}; long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
            n = std::min(n, std::max(1, (int) ((atol(q) + period / 2) / period)));
        fclose(f);
    }
    return std::max(1, n);
}

// f(0) .. f(n - 1) on up to spdp_host_cpus() threads, the caller's among them; items are taken in turn, so f(k) may run on any
// thread.  A worker's exception is rethrown as bad_alloc after the join; a thread that fails to start leaves its share to the others.
template <class F> void on_host_threads(int n, F f)
{
    std::atomic<int> next{0};
    std::atomic<bool> failed{false};
    auto work = [&] { try { for (int k; (k = next++) < n; ) f(k); } catch (...) { failed = true; } };
    const int nt = std::max(1, std::min(spdp_host_cpus(), n));
    std::vector<std::thread> th;
    try { for (int t = 1; t < nt; ++t) th.emplace_back(work); } catch (...) {}
    work();
    for (std::thread& t : th) t.join();
    if (failed) throw std::bad_alloc();
}

#endif
