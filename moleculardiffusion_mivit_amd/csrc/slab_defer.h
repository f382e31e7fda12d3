// Deferred slab reductions ("Slab deferral").  While a SlabDefer scope constructed with on = true is alive on a
// thread, misc.hip::launch_slab_reduce_strided queues its reductions there instead of launching them, and flush() runs the
// queue as ONE launch.  A scope destroyed without a flush -- an early return -- drops its queue, so outside the lifetime of a
// scope every reduction launches.  Host only, no HIP: the launch itself is in misc.hip.
#pragma once
#include <cstdint>

constexpr int MAX_SLAB_JOBS = 8;
struct SlabQueue {      // (the fields of misc.hip's kernel argument)
    const float *part[MAX_SLAB_JOBS]; float *out[MAX_SLAB_JOBS];
    int nparts[MAX_SLAB_JOBS], n[MAX_SLAB_JOBS], stride[MAX_SLAB_JOBS], vec_ok[MAX_SLAB_JOBS], blk_end[MAX_SLAB_JOBS];
    int njobs;
};

class SlabDefer {
public:
    explicit SlabDefer(bool on) { if (on) active() = this; }          // (scopes do not nest: the newest one owns the thread)
    ~SlabDefer() { deactivate(); }
    SlabDefer(const SlabDefer &) = delete;
    // true: queued on this thread's active scope.  false: the caller launches now (no active scope, queue full, or n / stride
    // beyond the 32-bit fields).  A job covers ceil(n / 128) blocks of the one launch; blk_end is their running sum.
    static bool push(const float *part, int nparts, int64_t stride, int64_t n, float *out, int vec_ok) {
        SlabDefer *d = active();
        if (!d || d->q_.njobs >= MAX_SLAB_JOBS || n >= (1ll << 31) || stride >= (1ll << 31)) return false;
        SlabQueue &q = d->q_;
        const int k = q.njobs++;
        q.part[k] = part; q.out[k] = out; q.nparts[k] = nparts; q.n[k] = (int)n; q.stride[k] = (int)stride; q.vec_ok[k] = vec_ok;
        q.blk_end[k] = (k ? q.blk_end[k - 1] : 0) + (int)((n + 127) / 128);
        return true;
    }
    // the queued jobs in order (njobs may be 0); the scope is empty and inactive afterwards
    SlabQueue take() { deactivate(); const SlabQueue q = q_; q_.njobs = 0; return q; }
    int flush(void *stream);          // misc.hip: take() + one launch on the hipStream_t `stream`
private:
    static SlabDefer *&active() { static thread_local SlabDefer *t = nullptr; return t; }
    void deactivate() { if (active() == this) active() = nullptr; }
    SlabQueue q_ = {};
};
