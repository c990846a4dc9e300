// spdp_chunk_plan.h -- how a batch is cut into the chunks of the software pipeline of spdp_host.cpp (align_on_store).
// A pure function of its arguments: no device, no globals (spdp_chunk_plan in include/spdp.h exports it).
//
// The chunks' linear-space sweeps follow each other on the GPU, and the host work, the slab tracebacks and the walk of
// chunk c run beside the sweep of chunk c + 1.  What follows the LAST sweep runs beside nothing, so the last chunk should
// be small; and the post-work of chunk c has to fit under the sweep of chunk c + 1, so a chunk cannot be much smaller than
// the one before it.  Hence a geometric plan: chunk c + 1 holds `ratio` times the DP cells of chunk c.
#ifndef SPDP_CHUNK_PLAN_H_
#define SPDP_CHUNK_PLAN_H_
#include <stdint.h>
#include <algorithm>
#include <vector>

#define SPDP_CHUNK_LEAST 64         // problems: no chunk is smaller

// cells[0 .. n): DP cells per problem, in caller order (values below 1 count as 1).  Cuts [0, n) into at most max_chunks
// contiguous chunks of at least max(SPDP_CHUNK_LEAST, min_chunk) problems each; the cumulative cells at the end of chunk c
// are the first to reach (1 + ratio + .. + ratio^c) / (1 + ratio + .. + ratio^(k - 1)) of the total.  Boundaries then move
// right while a chunk holds more cells than the one before it, and a count k whose plan still has a chunk that exceeds the
// one before it by more than the largest problem is given up for k - 1.  bounds[0 .. k] are written; returns k >= 1.
static inline int spdp_chunk_plan_of(const int64_t* cells, int n, int max_chunks, double ratio, int min_chunk, int* bounds)
{
    bounds[0] = 0; bounds[1] = std::max(n, 0);
    if (n <= 0 || max_chunks <= 1) return 1;
    const int least = std::max(SPDP_CHUNK_LEAST, min_chunk);
    if (!(ratio > 0.) || ratio > 1.) ratio = 1.;                    // (a NaN too)
    std::vector<int64_t> cum((size_t) n + 1, 0);
    int64_t biggest = 1;
    for (int i = 0; i < n; ++i) {
        const int64_t c = std::max<int64_t>(cells[i], 1);
        cum[i + 1] = cum[i] + c;
        biggest = std::max(biggest, c);
    }
    const double total = (double) cum[n];
    auto held = [&](int c) { return cum[bounds[c + 1]] - cum[bounds[c]]; };
    for (int k = std::min(max_chunks, n / least); k >= 2; --k) {
        double wsum = 0., w = 1.;
        for (int c = 0; c < k; ++c) { wsum += w; w *= ratio; }
        double acc = 0.;
        w = 1.;
        for (int c = 0; c + 1 < k; ++c) {
            acc += w; w *= ratio;
            const double target = total * acc / wsum;
            const int lo = bounds[c] + least, hi = n - (k - 1 - c) * least;     // lo <= hi: k * least <= n
            int i = lo;
            while (i < hi && (double) cum[i] + 0.5 < target) ++i;
            bounds[c + 1] = i;
        }
        bounds[k] = n;
        for (bool moved = true; moved; ) {                          // (boundaries only move right: this ends)
            moved = false;
            for (int c = 0; c + 1 < k; ++c)
                while (held(c + 1) > held(c) && bounds[c + 2] - bounds[c + 1] > least) { ++bounds[c + 1]; moved = true; }
        }
        bool ok = true;
        for (int c = 0; c + 1 < k; ++c) ok = ok && held(c + 1) <= held(c) + biggest;
        if (ok) return k;
    }
    bounds[1] = n;
    return 1;
}

#endif
