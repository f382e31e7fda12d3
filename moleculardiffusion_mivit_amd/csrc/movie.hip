// Noise-free rendering of a whole field of view with many particles: the image model of csrc/render.hip (one spot of the
// reference's helpers/helpersGeneration.py:283-310: Gaussian on a grid `up` times finer than the camera, rescaled to its PEAK
// on that grid, mean-pooled up x up), extended by linearity to Np particles that share one [F, H, W] movie.
//
// Definition (positions (y, x) = (row, column) in camera pixels, pixel centres at integers, as in the tracking tables):
//   fine sample g = i up + k of camera pixel i sits at fine coordinate g; a position c sits at u = c up + (up - 1) / 2;
//   g* = rint(u), dpk = g* - u;  prof(i; c) = (1 / up) sum_{k < up} exp(-((g - u)^2 - dpk^2) / (2 sigma_hr^2));
//   a sub-position adds amp prof(y; c_y) prof(x; c_x) to the pixels with |y - rint(c_y)| <= radius and |x - rint(c_x)| <= radius
//   and nothing elsewhere.
// The profile is evaluated relative to rint(c): with c = ic + fc (ic = rint(c), |fc| <= 1/2, both exact in fp32)
//   g - u = ((i - ic) up + k) - (fc up + (up - 1) / 2),     g* - u = rint(fc up + (up - 1) / 2) - (fc up + (up - 1) / 2),
// a small exact integer minus a small number, so the error does not grow with the size of the field.
//
// One workgroup of 256 threads per (frame, 32 x 64 tile).  It walks the (particle, sub-position) pairs of its frame in chunks
// of 256, one pair per thread: visibility (first / last), finiteness, window against tile.  The survivors are compacted IN
// ORDER (wave ballot + prefix over the four waves: no atomics), their two 1-D profiles restricted to the tile's rows and
// columns are built in LDS in batches of 64 (the amplitude folded into the row profile, zero outside the window), and every
// thread accumulates its eight pixels (rows ty + 4 r, column tx) in survivor order = particles ascending, sub-positions
// ascending.  A culled pair would add exactly +0, so the sum of a pixel does not depend on how the field is cut into tiles.
// Every pixel is stored once, 64 consecutive floats per wave.  LDS: 64 x (32 + 64) floats + 256 + 4 ints = 25.6 KB, whatever
// radius and npos are.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int MV_TH = 32, MV_TW = 64;        // tile: rows x columns
constexpr int MV_THREADS = 256;
constexpr int MV_ROWS = MV_TH / (MV_THREADS / MV_TW);      // pixels per thread (8)
constexpr int MV_CHUNK = MV_THREADS;         // pairs culled per pass, one per thread
constexpr int MV_BATCH = 64;                 // survivors whose profiles are in LDS at once
constexpr int MV_MAX_RADIUS = 64;            // documented caps (include/mivit_hip.h)
constexpr int MV_MAX_NPOS = 256;
constexpr int MV_MAX_UP = 64;
constexpr float MV_MAX_COORD = 1073741824.f; // 2^30: a position at or beyond it (or NaN / inf) contributes nothing

struct MovieArgs {
    const float *pos;          // [Np, F * npos, 2] (y, x)
    const float *amp;          // [Np, F, npos]
    const int *first, *last;   // [Np] or both null
    float *movie;              // [F, H, W]
    int Np, F, npos, up, radius, H, W, tilesX, tilesY;
    float inv2s2;
};

__global__ __launch_bounds__(MV_THREADS) void render_movie_kernel(const MovieArgs a) {
    __shared__ float s_py[MV_BATCH][MV_TH];          // amp * prof(y), 0 outside the window
    __shared__ float s_px[MV_BATCH][MV_TW];          // prof(x), 0 outside the window
    __shared__ int s_surv[MV_CHUNK];                 // surviving pairs of the chunk (index within the chunk), ascending
    __shared__ int s_wave[MV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid % MV_TW, ty = tid / MV_TW;
    int t = blockIdx.x;
    const int tileX = t % a.tilesX;
    t /= a.tilesX;
    const int tileY = t % a.tilesY, f = t / a.tilesY;
    const int y0 = tileY * MV_TH, x0 = tileX * MV_TW;
    const int npos = a.npos, up = a.up, radius = a.radius;
    const float half = 0.5f * (float)(up - 1), inv_up = 1.f / (float)up;
    float v[MV_ROWS];
#pragma unroll
    for (int r = 0; r < MV_ROWS; ++r) v[r] = 0.f;

    const int64_t pairs = (int64_t)a.Np * npos;
    for (int64_t q0 = 0; q0 < pairs; q0 += MV_CHUNK) {
        const int64_t q = q0 + tid;
        bool hit = false;
        if (q < pairs) {
            const int64_t p = q / npos;
            const int s = (int)(q - p * npos);
            if (!a.first || (a.first[p] <= f && f <= a.last[p])) {
                const int64_t e = (p * a.F + f) * npos + s;
                const float cy = a.pos[2 * e], cx = a.pos[2 * e + 1], am = a.amp[e];
                if (fabsf(cy) < MV_MAX_COORD && fabsf(cx) < MV_MAX_COORD && fabsf(am) <= FLT_MAX) {       // false for NaN
                    const int iy = (int)rintf(cy), ix = (int)rintf(cx);
                    hit = iy + radius >= y0 && iy - radius < y0 + MV_TH && ix + radius >= x0 && ix - radius < x0 + MV_TW;
                }
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, nsurv = 0;
#pragma unroll
        for (int w = 0; w < MV_THREADS / 64; ++w) {
            const int c = s_wave[w];
            if (w < wave) before += c;
            nsurv += c;
        }
        if (hit) s_surv[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
        __syncthreads();
        for (int b0 = 0; b0 < nsurv; b0 += MV_BATCH) {
            const int nb = min(MV_BATCH, nsurv - b0);
            // profiles: task = (survivor, row or column of the tile)
            for (int k = tid; k < nb * (MV_TH + MV_TW); k += MV_THREADS) {
                const int j = k / (MV_TH + MV_TW), r = k - j * (MV_TH + MV_TW);
                const bool isx = r >= MV_TH;
                const int i = isx ? x0 + (r - MV_TH) : y0 + r;
                const int64_t qq = q0 + s_surv[b0 + j];
                const int64_t p = qq / npos;
                const int64_t e = (p * a.F + f) * npos + (qq - p * npos);
                const float c = a.pos[2 * e + (isx ? 1 : 0)];
                const int ic = (int)rintf(c);
                float val = 0.f;
                const int di = i - ic;
                if (di >= -radius && di <= radius) {
                    const float uf = (c - (float)ic) * (float)up + half;
                    const float dpk = rintf(uf) - uf;
                    const float base = (float)(di * up) - uf;
                    float acc = 0.f;
                    for (int kk = 0; kk < up; ++kk) {
                        const float d = base + (float)kk;
                        acc += __expf(-(d * d - dpk * dpk) * a.inv2s2);
                    }
                    val = acc * inv_up;
                }
                if (isx) s_px[j][r - MV_TH] = val;
                else s_py[j][r] = a.amp[e] * val;
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) {
                const float pxv = s_px[j][tx];
#pragma unroll
                for (int r = 0; r < MV_ROWS; ++r) v[r] += s_py[j][ty + r * (MV_THREADS / MV_TW)] * pxv;
            }
            __syncthreads();
        }
    }
    const int x = x0 + tx;
    if (x < a.W) {
#pragma unroll
        for (int r = 0; r < MV_ROWS; ++r) {
            const int y = y0 + ty + r * (MV_THREADS / MV_TW);
            if (y < a.H) a.movie[((int64_t)f * a.H + y) * a.W + x] = v[r];
        }
    }
}

}  // namespace

extern "C" int mivit_render_movie(const float *pos, const float *amp, const int *first, const int *last, int Np, int F, int npos,
                                  float sigma_hr, int up, int radius, int H, int W, float *movie, void *stream) {
    MIVIT_CHECK(movie, "render_movie: null pointer (movie)");
    MIVIT_CHECK(Np >= 0, "render_movie: Np = %d < 0", Np);
    MIVIT_CHECK(Np == 0 || (pos && amp), "render_movie: null pointer (pos / amp)");
    MIVIT_CHECK((first == nullptr) == (last == nullptr), "render_movie: first and last must both be given or both be null");
    MIVIT_CHECK(F >= 1 && npos >= 1 && up >= 1 && H >= 1 && W >= 1, "render_movie: F, npos, up, H, W must be >= 1, got %d, %d, %d, %d, %d",
                F, npos, up, H, W);
    MIVIT_CHECK(radius >= 0 && radius <= MV_MAX_RADIUS, "render_movie: radius = %d outside 0 .. %d", radius, MV_MAX_RADIUS);
    MIVIT_CHECK(npos <= MV_MAX_NPOS, "render_movie: npos = %d, the limit is %d", npos, MV_MAX_NPOS);
    MIVIT_CHECK(up <= MV_MAX_UP, "render_movie: up = %d, the limit is %d", up, MV_MAX_UP);
    MIVIT_CHECK(H <= (1 << 24) && W <= (1 << 24), "render_movie: field of %d x %d, the limit is 2^24 per side", H, W);
    const float inv2s2 = 1.f / (2.f * sigma_hr * sigma_hr);
    MIVIT_CHECK(sigma_hr > 0.f && inv2s2 > 0.f && inv2s2 <= FLT_MAX, "render_movie: sigma_hr = %g is not a usable width", (double)sigma_hr);
    const int64_t tilesX = (W + MV_TW - 1) / MV_TW, tilesY = (H + MV_TH - 1) / MV_TH;
    const int64_t blocks = tilesX * tilesY * (int64_t)F;
    MIVIT_CHECK(blocks <= INT_MAX, "render_movie: %lld tiles in one launch, the limit is 2^31 - 1; render fewer frames per call",
                (long long)blocks);
    MovieArgs a{pos, amp, first, last, movie, Np, F, npos, up, radius, H, W, (int)tilesX, (int)tilesY, inv2s2};
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(render_movie_kernel, dim3((unsigned)blocks), dim3(MV_THREADS), 0, static_cast<hipStream_t>(stream), a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
