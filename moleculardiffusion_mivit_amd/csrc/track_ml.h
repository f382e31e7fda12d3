// What the per-track maximum-likelihood fits share (likelihood.hip, fbm_ml.hip, confined_ml.hip, directed_ml.hip): the usable-row rule, the
// clamp of a range, the pass for the reference scale, the determinant as an exactly rescaled product with the closing of
// the cost, the arg-min of a wave, the 3 x 3 stencil of the observed information, and the host checks of the common
// arguments.  Nothing here knows a model: recurrences, searches and outputs are in the model's file.  The numpy restatement
// of every piece is in helpers/msd.py under the same name (_ml_usable, _ml_finish_cost, _ml_hessian).
//
// The arithmetic is fp64 in a fixed order that the restatements repeat, so nothing may be contracted into FMA: the pragma
// below holds for the rest of the translation unit, and ONLY TRANSLATION UNITS THAT WANT NO CONTRACTION MAY INCLUDE THIS FILE.
#pragma once
#pragma clang fp contract(off)

#include "common.h"

constexpr int TM_WAVE = 64;
constexpr double TM_LOG_2PI = 1.8378770664093453;                         // np.log(2 * np.pi)
constexpr double TM_LN2 = 0.6931471805599453;                             // np.log(2)
constexpr double TM_H = 0.015625;                                         // 1 / 64: the step of the curvature's differences
constexpr double TM_EXP_H = 1.0157477085866857;                           // np.exp(1 / 64)
constexpr double TM_EXP_MH = 0.9844964370054085;                          // np.exp(-1 / 64)

// ------------------------------------------------------------------------------------------------
// rows
// ------------------------------------------------------------------------------------------------
struct TmRows {
    const double *pos, *var;
    const int *frames;
    const unsigned char *use;
    int a, b;                                                             // the range, clamped into [0, N]
};

struct TmRow {
    double y, x, vy, vx;
    int f;
    bool ok;
};

__device__ __forceinline__ bool tm_finite(double v) { return fabs(v) < INFINITY; }

// row r of the range: usable when its flag is set, both coordinates are finite and both variances are finite and >= 0
__device__ __forceinline__ TmRow tm_row(const TmRows &R, int r) {
    TmRow w;
    w.y = R.pos[2 * (int64_t)r];
    w.x = R.pos[2 * (int64_t)r + 1];
    w.vy = R.var ? R.var[2 * (int64_t)r] : 0.0;
    w.vx = R.var ? R.var[2 * (int64_t)r + 1] : 0.0;
    w.f = R.frames ? R.frames[r] : r - R.a;
    w.ok = (R.use ? R.use[r] != 0 : true) && tm_finite(w.y) && tm_finite(w.x) && w.vy >= 0.0 && w.vy < INFINITY &&
           w.vx >= 0.0 && w.vx < INFINITY;
    return w;
}

__device__ __forceinline__ void tm_clamp_range(const int *offsets, int k, int N, int &a, int &b) {
    a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read outside [0, N), whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
}

// ------------------------------------------------------------------------------------------------
// the reference scale: D_ref = sum d^2 (both axes) / (4 dt sum g) over the increments between usable rows
// ------------------------------------------------------------------------------------------------
struct TmScale {
    int cnt;                                                              // usable rows
    double S;                                                             // sum d^2, both axes
    int64_t G;                                                            // sum of the gaps in frames
    double sy, sx;                                                        // sums of the positions (dead where not used)
    __device__ __forceinline__ int n_inc() const { return cnt > 0 ? cnt - 1 : 0; }
};

__device__ __forceinline__ double tm_d_ref(double S, double dt, int64_t G) { return S / ((4.0 * dt) * (double)G); }

// one walk over the rows, the same in every lane
__device__ __forceinline__ TmScale tm_scale(const TmRows &R) {
    double S = 0.0, sy = 0.0, sx = 0.0, py = 0.0, px = 0.0;
    int64_t G = 0;
    int pf = 0, cnt = 0;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;
        if (cnt > 0) {
            const double dy = w.y - py, dx = w.x - px;
            S = S + (dy * dy + dx * dx);
            G += w.f - pf;
        }
        sy = sy + w.y, sx = sx + w.x;
        py = w.y, px = w.x, pf = w.f;
        ++cnt;
    }
    return TmScale{cnt, S, G, sy, sx};
}

// ------------------------------------------------------------------------------------------------
// the determinant as a product rescaled exactly (mantissa in [0.5, 1) and an integer exponent), and the cost it closes
// ------------------------------------------------------------------------------------------------
struct TmProd {
    double m = 0.5;
    int e = 1;
    __device__ __forceinline__ void mul(double x) {
        int ex;
        m = frexp(m * x, &ex);
        e += ex;
    }
    __device__ __forceinline__ double log() const { return ::log(m) + (double)e * TM_LN2; }
};

// -2 log L = log det + Q + 2 n_inc log 2 pi; +inf for a rejected candidate and for a cost that is not a number
__device__ __forceinline__ double tm_finish_cost(const TmProd &det, double Q, int n_inc, bool bad) {
    const double cost = (det.log() + Q) + (double)(2 * n_inc) * TM_LOG_2PI;
    return (bad || !(cost < INFINITY)) ? INFINITY : cost;
}

// every lane of the wave ends with the least cost and its lowest lane
__device__ __forceinline__ void tm_wave_argmin(double &c, int &j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(c, o, TM_WAVE);
        const int oj = __shfl_xor(j, o, TM_WAVE);
        if (oc < c || (oc == c && oj < j)) c = oc, j = oj;
    }
}

// ------------------------------------------------------------------------------------------------
// the observed information from differences of the cost with the step h = 1 / 64
// ------------------------------------------------------------------------------------------------
// half the second difference over h^2: the curvature of -log L
__device__ __forceinline__ double tm_curvature(double cp, double c0, double cm) { return ((cp - c0) + (cm - c0)) * 2048.0; }

// the 2 x 2 information in (u, v) from the nine costs of the stencil, c[3 a + b] at (u + (a - 1) h, v + (b - 1) h)
struct TmHess2 {
    double uu, vv, uv, det;
    __device__ __forceinline__ explicit TmHess2(const double *c) {
        const double c0 = c[4];
        uu = tm_curvature(c[7], c0, c[1]);
        vv = tm_curvature(c[5], c0, c[3]);
        uv = ((c[8] - c[6]) - (c[2] - c[0])) * 512.0;                     // 1 / (8 h^2)
        det = uu * vv - uv * uv;
    }
    __device__ __forceinline__ bool pd() const { return uu > 0.0 && vv > 0.0 && det > 0.0 && det < INFINITY; }
};

// ------------------------------------------------------------------------------------------------
// host: the checks of the arguments every entry point takes.  0 with n == 0 says nothing about the pointers.
// ------------------------------------------------------------------------------------------------
inline int tm_check_rows(const char *name, const double *pos, int N, const int *offsets, int n, double dt) {
    MIVIT_CHECK(N >= 0 && n >= 0, "%s: N = %d, n = %d: negative size", name, N, n);
    MIVIT_CHECK(dt > 0.0 && dt < INFINITY, "%s: dt = %g must be positive and finite", name, dt);
    if (n == 0) return 0;
    MIVIT_CHECK(offsets && (pos || N == 0), "%s: null pointer", name);
    return 0;
}
