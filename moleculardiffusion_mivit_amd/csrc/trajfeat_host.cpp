// Host build of csrc/trajfeat.h (libmivit_trajfeat_host.so, compiled with the host C++ compiler by csrc/build.py).
// TEST INFRASTRUCTURE ONLY: tests/test_trajfeat_host.py holds this library against scipy and the reference goldens, and
// tests/test_features_gpu.py holds the kernel (the same header on the device) against it.  The product never loads it.
#include <stdlib.h>
#include <vector>

#include "trajfeat.h"

namespace {
template <typename T>
void run(const T *traj, int N, int T_, int npos, double dt, double *feats, T *avg) {
    const int nf = T_ / npos;
    std::vector<double> pos(2 * (size_t)nf + 1), msd((size_t)nf + 1);
    for (int n = 0; n < N; ++n) {
        const T *src = traj + (int64_t)n * T_ * 2;
        for (int f = 0; f < nf; ++f) {
            T ax, ay;
            trajfeat::average_frame(src + (int64_t)f * npos * 2, npos, ax, ay);
            pos[2 * f] = (double)ax;
            pos[2 * f + 1] = (double)ay;
            if (avg) {
                avg[((int64_t)n * nf + f) * 2] = ax;
                avg[((int64_t)n * nf + f) * 2 + 1] = ay;
            }
        }
        trajfeat::features(trajfeat::Buf{pos.data(), 1}, nf, dt, trajfeat::Buf{msd.data(), 1}, feats + (int64_t)n * 25);
    }
}
}  // namespace

// the same argument rules as mivit_trajectory_features; dtype 0 = fp32, 3 = fp64
extern "C" int trajfeat_host_features(const void *traj, int dtype, int N, int T, int npos, double dt, double *feats,
                                      void *avg) {
    if (N < 0 || npos < 1 || T < npos || T / npos > trajfeat::MAX_FRAMES || (dtype != 0 && dtype != 3)) return 1;
    if (N > 0 && (!traj || !feats)) return 1;
    if (dtype == 0) run((const float *)traj, N, T, npos, dt, feats, (float *)avg);
    else run((const double *)traj, N, T, npos, dt, feats, (double *)avg);
    return 0;
}
