// The 25 trajectory descriptors of the ImagesFeatures experiment on the GPU (the descriptor part):
// the counterpart of the reference's compute_features_for_multiple_trajectories loop (helpers/helpersFeatures.py:524-567)
// without its nan_to_num, i.e. helpers/features.compute_features_for_trajectories' feature matrix.  One thread per
// trajectory: frame averaging fused in (input precision), then csrc/trajfeat.h in fp64 -- lag moments, the restated scipy
// 'trf' power-law fit, hull, the rest.  The serial fit dominates; there is nothing to share between trajectories, so the
// only tuning is how many lanes a wave gets (see mivit_trajectory_features).
//
// Workspace (fp64, per trajectory, element-strided by N so that neighbouring lanes touch neighbouring words):
//   [0, 2 nf)      averaged positions x0 y0 x1 y1 ...
//   [2 nf, 3 nf)   MSD of lags 1 .. nl (nl < nf)
#include "common.h"
#include "trajfeat.h"

namespace {

template <typename T>
__global__ __launch_bounds__(64) void trajfeat_kernel(const T *__restrict__ traj, int N, int Tn, int npos, double dt,
                                                     double *__restrict__ feats, T *__restrict__ avg, double *ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int nf = Tn / npos;
    const trajfeat::Buf pos{ws + i, (int64_t)N};
    const trajfeat::Buf msd{ws + (int64_t)2 * nf * N + i, (int64_t)N};
    const T *src = traj + (int64_t)i * Tn * 2;
    for (int f = 0; f < nf; ++f) {
        T ax, ay;
        trajfeat::average_frame(src + (int64_t)f * npos * 2, npos, ax, ay);
        pos[2 * f] = (double)ax;
        pos[2 * f + 1] = (double)ay;
        if (avg) {
            avg[((int64_t)i * nf + f) * 2] = ax;
            avg[((int64_t)i * nf + f) * 2 + 1] = ay;
        }
    }
    trajfeat::features(pos, nf, dt, msd, feats + (int64_t)i * trajfeat::N_FEATURES);
}

}  // namespace

extern "C" size_t mivit_trajectory_features_workspace_bytes(int N, int T, int npos) {
    if (N <= 0 || npos < 1 || T < npos) return 0;
    return (size_t)3 * (size_t)(T / npos) * (size_t)N * sizeof(double);
}

extern "C" int mivit_trajectory_features(const void *traj, int dtype, int N, int T, int npos, double dt, double *feats,
                                         void *avg, void *workspace, size_t workspace_bytes, void *stream) {
    MIVIT_CHECK(N >= 0, "trajectory_features: N = %d < 0", N);
    MIVIT_CHECK(npos >= 1 && npos <= T, "trajectory_features: need 1 <= npos <= T (npos = %d, T = %d)", npos, T);
    MIVIT_CHECK(T / npos <= trajfeat::MAX_FRAMES, "trajectory_features: %d frames > %d", T / npos, (int)trajfeat::MAX_FRAMES);
    MIVIT_CHECK(dtype == MIVIT_F32 || dtype == MIVIT_F64, "trajectory_features: dtype %d is not MIVIT_F32 / MIVIT_F64", dtype);
    if (N == 0) return 0;
    MIVIT_CHECK(traj && feats && workspace, "trajectory_features: null pointer");
    MIVIT_CHECK(workspace_bytes >= mivit_trajectory_features_workspace_bytes(N, T, npos),
                "trajectory_features: workspace of %zu bytes < %zu", workspace_bytes,
                mivit_trajectory_features_workspace_bytes(N, T, npos));
    // lanes per wave: enough waves to reach every CU first (256 on MI355X), full waves once there are more trajectories.
    // A lane's fit is serial and lanes of a wave diverge in their iteration counts, so small batches run faster with
    // partly filled waves spread over more CUs than with a few full ones.
    int tpb = 64;
    while (tpb > 1 && (int64_t)tpb * 256 > N) tpb >>= 1;
    const int blocks = (N + tpb - 1) / tpb;
    prof_set_tag(MIVIT_PROF_OP);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *ws = static_cast<double *>(workspace);
    if (dtype == MIVIT_F32)
        hipLaunchKernelGGL(trajfeat_kernel<float>, dim3(blocks), dim3(tpb), 0, s, static_cast<const float *>(traj), N, T,
                           npos, dt, feats, static_cast<float *>(avg), ws);
    else
        hipLaunchKernelGGL(trajfeat_kernel<double>, dim3(blocks), dim3(tpb), 0, s, static_cast<const double *>(traj), N,
                           T, npos, dt, feats, static_cast<double *>(avg), ws);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
