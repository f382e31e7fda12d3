// Stand-alone host program for tests/test_slab_defer_host.py: exercises csrc/slab_defer.h (the queue and the scope of the
// deferred slab reductions) without HIP.  Built with -fsanitize=address,undefined; exit status 0 = every check held.
#include "slab_defer.h"

#include <cstdio>

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static float g_part[4], g_out[MAX_SLAB_JOBS + 1];

// what misc.hip::launch_slab_reduce_strided asks: true = queued, false = "launch it yourself"
static bool push(int64_t n, int64_t stride = 512, int k = 0) { return SlabDefer::push(g_part, 3 + k, stride, n, g_out + k, k & 1); }

int main() {
    // no scope alive: refused
    CHECK(!push(100));
    // an `off` scope refuses as well, and hands over nothing
    {
        SlabDefer off(false);
        CHECK(!push(100));
        CHECK(off.take().njobs == 0);
    }
    // an `on` scope queues MAX_SLAB_JOBS jobs and refuses the next one; blk_end is the running sum of ceil(n / 128);
    // take() returns the jobs in order and deactivates the scope
    {
        const int64_t n[MAX_SLAB_JOBS] = {1, 127, 128, 129, 16384, 49152, 256 * 128 + 1, (1ll << 31) - 1};
        SlabDefer on(true);
        for (int k = 0; k < MAX_SLAB_JOBS; ++k) CHECK(push(n[k], 1000 + k, k));
        CHECK(!push(100));
        const SlabQueue q = on.take();
        CHECK(q.njobs == MAX_SLAB_JOBS);
        int64_t sum = 0;
        for (int k = 0; k < MAX_SLAB_JOBS; ++k) {
            sum += (n[k] + 127) / 128;
            CHECK(q.part[k] == g_part && q.out[k] == g_out + k && q.nparts[k] == 3 + k && q.n[k] == n[k]);
            CHECK(q.stride[k] == 1000 + k && q.vec_ok[k] == (k & 1) && q.blk_end[k] == sum);
        }
        CHECK(!push(100));                      // deactivated by take()
        CHECK(on.take().njobs == 0);            // and empty
    }
    // n or stride of 2^31 and more do not fit the queue's fields: refused, nothing queued
    {
        SlabDefer on(true);
        CHECK(!push(1ll << 31));
        CHECK(!push(100, 1ll << 31));
        CHECK(!push(1ll << 40, 1ll << 40));
        CHECK(push(100, (1ll << 31) - 1));
        CHECK(on.take().njobs == 1);
    }
    // the finding: a scope destroyed with jobs still queued (an early return between the first block and the flush) leaves
    // the thread as it found it -- the next push is refused, and a later scope starts empty
    {
        {
            SlabDefer on(true);
            CHECK(push(300));
            CHECK(push(500));
        }
        CHECK(!push(100));
        SlabDefer next(true);
        CHECK(push(129));
        const SlabQueue q = next.take();
        CHECK(q.njobs == 1 && q.n[0] == 129 && q.blk_end[0] == 2);
    }
    // a destroyed `off` scope does not deactivate a live `on` scope
    {
        SlabDefer on(true);
        { SlabDefer off(false); }
        CHECK(push(100));
    }
    CHECK(!push(100));
    if (g_failed) return 1;
    std::printf("slab_defer_host: OK\n");
    return 0;
}
