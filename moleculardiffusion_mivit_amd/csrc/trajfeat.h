// The 25 trajectory descriptors of the ImagesFeatures experiment (helpers/features.py:compute_diffusion_features, pinned
// to the reference's helpers/helpersFeatures.py:448-519), written once for the device (csrc/features.hip, one thread per
// trajectory) and the host (libmivit_trajfeat_host.so, test infrastructure).  Plain scalar code: no wave intrinsics, no
// LDS, no per-thread arrays indexed at run time (every local array is indexed by constants after unrolling, so nothing
// goes to scratch).  fp64 throughout, as the reference.
//
// The power-law fit restates the exact path scipy 1.15.3 takes for the reference's call
//     curve_fit(power_law, t, msd, p0=[msd[0]/(4dt), 1, 1e-3], bounds=([1e-5,1e-5,0],[inf,10,inf]), method="trf",
//               maxfev=10000)
// i.e. scipy/optimize/_lsq/least_squares.py, trf.py (trf_bounds, select_step), common.py (solve_lsq_trust_region,
// update_tr_radius, check_termination, CL_scaling_vector, make_strictly_feasible, step_size_to_bound, ...) and
// _numdiff.py (the '2-point' Jacobian).  scipy is BSD-3-Clause licensed (Copyright (c) 2001-2002 Enthought, Inc.,
// 2003-2024 SciPy Developers); the algorithm is restated here, with its branch structure and constants, so that the
// numbers follow scipy's iterates rather than those of a better optimiser (scipy stops early on flat cost surfaces).
// Differences in rounding only: the exact-trust-region SVD of [J d; diag(diag_h^1/2)] is taken from the 3x3 R of a
// Givens QR of J (kept, with Q^T f, instead of J itself) followed by a one-sided Jacobi SVD, never from J^T J.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TF_HD __host__ __device__ __forceinline__
#define TF_MEMBER __host__ __device__ __forceinline__
#else
#define TF_HD static inline
#define TF_MEMBER inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace trajfeat {

enum { N_FEATURES = 25, MAX_FRAMES = 1024 };

// element k of a per-trajectory buffer: base[k * stride] (stride = number of trajectories in the kernel, so that
// neighbouring threads touch neighbouring words; 1 on the host)
struct Buf {
    double *base;
    int64_t stride;
    TF_MEMBER double &operator[](int k) const { return base[(int64_t)k * stride]; }
};

TF_HD double pymax(double a, double b) { return b > a ? b : a; }      // Python's max(a, b)
TF_HD double pymin(double a, double b) { return b < a ? b : a; }      // Python's min(a, b)
TF_HD double npmax(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }   // np.maximum
TF_HD double npsign(double a) { return a > 0 ? 1.0 : (a < 0 ? -1.0 : (a == 0 ? 0.0 : a)); }

// numpy's pairwise summation (np.add.reduce of a contiguous float64 vector: 8 accumulators per block of <= 128 elements,
// halves split at a multiple of 8 above that), of get(0) .. get(n-1).  DEPTH bounds the static recursion (n <= 128 << DEPTH).
template <int DEPTH, typename G>
TF_HD double pairwise_sum(const G &get, int off, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += get(off + i);
        return r;
    }
    if (DEPTH == 0 || n <= 128) {
        double r0 = get(off), r1 = get(off + 1), r2 = get(off + 2), r3 = get(off + 3), r4 = get(off + 4),
               r5 = get(off + 5), r6 = get(off + 6), r7 = get(off + 7);
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
            r0 += get(off + i); r1 += get(off + i + 1); r2 += get(off + i + 2); r3 += get(off + i + 3);
            r4 += get(off + i + 4); r5 += get(off + i + 5); r6 += get(off + i + 6); r7 += get(off + i + 7);
        }
        double r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) r += get(off + i);
        return r;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum<(DEPTH > 0 ? DEPTH - 1 : 0)>(get, off, n2) + pairwise_sum<(DEPTH > 0 ? DEPTH - 1 : 0)>(get, off + n2, n - n2);
}

// ---------------------------------------------------------------------------------------------------------------------
// frame averaging in the input precision: sub-steps summed one after another, then divided by npos (numpy mean(axis=2))
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
TF_HD void average_frame(const T *seg, int npos, T &ax, T &ay) {
    T sx = seg[0], sy = seg[1];
    for (int j = 1; j < npos; ++j) {
        sx += seg[2 * j];
        sy += seg[2 * j + 1];
    }
    ax = sx / (T)npos;
    ay = sy / (T)npos;
}

// ---------------------------------------------------------------------------------------------------------------------
// the fit: MSD(t) = 4 D t^alpha + offset, t = (1 .. m) dt; residual f_i = model_i - msd_i (curve_fit's _wrap_func)
// ---------------------------------------------------------------------------------------------------------------------
struct Fit {
    Buf msd;
    int m;
    double dt;
};

#define TF_EPS 2.220446049250313e-16
#define TF_INF (__builtin_huge_val())

TF_HD double lb_of(int k) { return k == 2 ? 0.0 : 1e-5; }
TF_HD double ub_of(int k) { return k == 1 ? 10.0 : TF_INF; }

TF_HD double resid(const Fit &F, int i, double D, double a, double off) {
    const double t = (double)(i + 1) * F.dt;
    return ((4.0 * D) * pow(t, a) + off) - F.msd[i];
}

TF_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
TF_HD double norm3(const double *a) { return sqrt(dot3(a, a)); }

// rotate the row (r, rf) into the upper-triangular R / Q^T f (R starts at zero: any number of rows, m < 3 included)
TF_HD void givens_row(double R[3][3], double qtf[3], double r[3], double rf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (r[k] != 0.0) {
            const double a = R[k][k], b = r[k], h = hypot(a, b), c = a / h, s = b / h;
            R[k][k] = h;
#pragma unroll
            for (int j = k + 1; j < 3; ++j) {
                const double t1 = R[k][j], t2 = r[j];
                R[k][j] = c * t1 + s * t2;
                r[j] = -s * t1 + c * t2;
            }
            const double t1 = qtf[k];
            qtf[k] = c * t1 + s * rf;
            rf = -s * t1 + c * rf;
        }
    }
}

// J at x ('2-point', _numdiff.approx_derivative with bounds) folded into R / Q^T f on the fly; g = J^T f; J is not kept
TF_HD void jacobian(const Fit &F, const double x[3], double R[3][3], double qtf[3], double g[3]) {
    double xp[3], dx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lb = lb_of(k), ub = ub_of(k);
        double h = 1.4901161193847656e-08 * (x[k] >= 0 ? 1.0 : -1.0) * fmax(1.0, fabs(x[k]));   // EPS**0.5
        const double lower = x[k] - lb, upper = ub - x[k];
        const double xt = x[k] + h;
        const bool violated = (xt < lb) || (xt > ub), fitting = fabs(h) <= npmax(lower, upper);
        if (violated && fitting) h = -h;
        else if (!fitting) h = upper >= lower ? upper : -lower;
        xp[k] = x[k] + h;
        dx[k] = xp[k] - x[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        qtf[k] = g[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) R[k][j] = 0.0;
    }
    for (int i = 0; i < F.m; ++i) {
        const double f = resid(F, i, x[0], x[1], x[2]);
        double r[3];
        r[0] = (resid(F, i, xp[0], x[1], x[2]) - f) / dx[0];
        r[1] = (resid(F, i, x[0], xp[1], x[2]) - f) / dx[1];
        r[2] = (resid(F, i, x[0], x[1], xp[2]) - f) / dx[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += r[k] * f;
        givens_row(R, qtf, r, f);
    }
}

// 0.5 |f(x)|^2 ; false if a residual is not finite
TF_HD bool cost_at(const Fit &F, const double x[3], double &cost) {
    double s = 0.0;
    bool fin = true;
    for (int i = 0; i < F.m; ++i) {
        const double f = resid(F, i, x[0], x[1], x[2]);
        fin = fin && isfinite(f);
        s += f * f;
    }
    cost = 0.5 * s;
    return fin;
}

// J_h s = J (d * s) = Q (R (d * s)):  Rd = R diag(d)
TF_HD void mulR(const double Rd[3][3], const double *s, double *out) {
    out[0] = Rd[0][0] * s[0] + Rd[0][1] * s[1] + Rd[0][2] * s[2];
    out[1] = Rd[1][1] * s[1] + Rd[1][2] * s[2];
    out[2] = Rd[2][2] * s[2];
}

TF_HD double evaluate_quadratic(const double Rd[3][3], const double g[3], const double s[3], const double diag[3]) {
    double Js[3], sd[3];
    mulR(Rd, s, Js);
    double q = dot3(Js, Js);
#pragma unroll
    for (int k = 0; k < 3; ++k) sd[k] = s[k] * diag[k];
    q += dot3(sd, s);
    return 0.5 * q + dot3(s, g);
}

// build_quadratic_1d with s0 (returns a, b, c) or without (c = 0)
TF_HD void build_quadratic_1d(const double Rd[3][3], const double g[3], const double s[3], const double diag[3],
                              const double *s0, double &a, double &b, double &c) {
    double v[3], sd[3];
    mulR(Rd, s, v);
    a = dot3(v, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) sd[k] = s[k] * diag[k];
    a += dot3(sd, s);
    a *= 0.5;
    b = dot3(g, s);
    c = 0.0;
    if (s0) {
        double u[3], s0d[3];
        mulR(Rd, s0, u);
        b += dot3(u, v);
        c = 0.5 * dot3(u, u) + dot3(g, s0);
#pragma unroll
        for (int k = 0; k < 3; ++k) s0d[k] = s0[k] * diag[k];
        b += dot3(s0d, s);
        c += 0.5 * dot3(s0d, s0);
    }
}

TF_HD void minimize_quadratic_1d(double a, double b, double lb, double ub, double c, double &t_out, double &y_out) {
    double t0 = lb, t1 = ub, t2 = 0.0;
    int nt = 2;
    if (a != 0) {
        const double ext = -0.5 * b / a;
        if (lb < ext && ext < ub) { t2 = ext; nt = 3; }
    }
    const double y0 = t0 * (a * t0 + b) + c, y1 = t1 * (a * t1 + b) + c, y2 = t2 * (a * t2 + b) + c;
    // np.argmin: the first minimum, a NaN counts as the minimum
    t_out = t0; y_out = y0;
    if (y0 != y0) return;
    if (y1 != y1 || y1 < y_out) { t_out = t1; y_out = y1; if (y1 != y1) return; }
    if (nt == 3 && (y2 != y2 || y2 < y_out)) { t_out = t2; y_out = y2; }
}

// step_size_to_bound: min over k of the stride to the bound along s, and hits (sign of s where the minimum is reached)
TF_HD double step_size_to_bound(const double x[3], const double s[3], double hits[3]) {
    double st[3], mn;
#pragma unroll
    for (int k = 0; k < 3; ++k) st[k] = s[k] != 0 ? npmax((lb_of(k) - x[k]) / s[k], (ub_of(k) - x[k]) / s[k]) : TF_INF;
    // np.min propagates NaN
    mn = st[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) mn = (mn != mn) ? mn : ((st[k] != st[k] || st[k] < mn) ? st[k] : mn);
#pragma unroll
    for (int k = 0; k < 3; ++k) hits[k] = (st[k] == mn ? 1.0 : 0.0) * npsign(s[k]);
    return mn;
}

TF_HD bool in_bounds(const double x[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && (x[k] >= lb_of(k)) && (x[k] <= ub_of(k));
    return ok;
}

// solve_lsq_trust_region (n = 3) on the SVD (s descending, V columns, uf = U^T f_aug)
TF_HD void solve_lsq_trust_region(int m, const double uf[3], const double s[3], const double V[3][3], double Delta,
                                  double &alpha, double p[3]) {
    double suf[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) suf[k] = s[k] * uf[k];
    const bool full_rank = m >= 3 ? s[2] > TF_EPS * m * s[0] : false;
    if (full_rank) {
        double w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = uf[k] / s[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = -(V[k][0] * w[0] + V[k][1] * w[1] + V[k][2] * w[2]);
        if (norm3(p) <= Delta) { alpha = 0.0; return; }
    }
    // phi_and_derivative
    auto phi_of = [&](double al, double &phi, double &dphi) {
        double q[3], den[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { den[k] = s[k] * s[k] + al; q[k] = suf[k] / den[k]; }
        const double pn = norm3(q);
        phi = pn - Delta;
        dphi = -((suf[0] * suf[0] / pow(den[0], 3.0) + suf[1] * suf[1] / pow(den[1], 3.0)) +
                 suf[2] * suf[2] / pow(den[2], 3.0)) / pn;
    };
    double a_up = norm3(suf) / Delta, a_lo = 0.0;
    if (full_rank) {
        double phi, dphi;
        phi_of(0.0, phi, dphi);
        a_lo = -phi / dphi;
    }
    if (!full_rank && alpha == 0) alpha = pymax(0.001 * a_up, pow(a_lo * a_up, 0.5));
    for (int it = 0; it < 10; ++it) {
        if (alpha < a_lo || alpha > a_up) alpha = pymax(0.001 * a_up, pow(a_lo * a_up, 0.5));
        double phi, dphi;
        phi_of(alpha, phi, dphi);
        if (phi < 0) a_up = alpha;
        const double ratio = phi / dphi;
        a_lo = pymax(a_lo, alpha - ratio);
        alpha -= (phi + Delta) * ratio / Delta;
        if (fabs(phi) < 0.01 * Delta) break;
    }
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = suf[k] / (s[k] * s[k] + alpha);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = -(V[k][0] * w[0] + V[k][1] * w[1] + V[k][2] * w[2]);
    const double sc = Delta / norm3(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] *= sc;
}

// SVD of the augmented system [J d; diag(diag_h^1/2)] from the QR of J: fold the three diagonal rows into R diag(d), then a
// one-sided (Hestenes) Jacobi SVD of the 3x3 triangle.  s descending, V columns = right singular vectors, uf = U^T [f; 0].
TF_HD void augmented_svd(const double Rd[3][3], const double qtf[3], const double diag_h[3], double s[3], double V[3][3],
                         double uf[3]) {
    double W[3][3], q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        q[i] = qtf[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) { W[i][j] = j >= i ? Rd[i][j] : 0.0; V[i][j] = i == j ? 1.0 : 0.0; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double r[3] = {0.0, 0.0, 0.0};
        r[k] = sqrt(diag_h[k]);
        givens_row(W, q, r, 0.0);
    }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int P = pq == 2 ? 1 : 0, Q = pq == 0 ? 1 : 2;
            double a = 0, b = 0, c = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) { a += W[i][P] * W[i][P]; b += W[i][Q] * W[i][Q]; c += W[i][P] * W[i][Q]; }
            if (c != 0.0 && fabs(c) > TF_EPS * sqrt(a * b)) {
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + hypot(1.0, zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double wp = W[i][P], wq = W[i][Q];
                    W[i][P] = cs * wp - sn * wq;
                    W[i][Q] = sn * wp + cs * wq;
                    const double vp = V[i][P], vq = V[i][Q];
                    V[i][P] = cs * vp - sn * vq;
                    V[i][Q] = sn * vp + cs * vq;
                }
                rotated = true;
            }
        }
        if (!rotated) break;
    }
    double suf[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = sqrt(W[0][k] * W[0][k] + W[1][k] * W[1][k] + W[2][k] * W[2][k]);
        suf[k] = W[0][k] * q[0] + W[1][k] * q[1] + W[2][k] * q[2];     // s_k (u_k . [Q^T f])
    }
    // sort descending (three compare-exchanges on constant indices)
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
        const int P = pq == 2 ? 1 : 0, Q = pq == 0 ? 1 : 2;              // (0,1) (0,2) (1,2)
        if (s[Q] > s[P]) {
            double t = s[P]; s[P] = s[Q]; s[Q] = t;
            t = suf[P]; suf[P] = suf[Q]; suf[Q] = t;
#pragma unroll
            for (int i = 0; i < 3; ++i) { t = V[i][P]; V[i][P] = V[i][Q]; V[i][Q] = t; }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) uf[k] = s[k] > 0 ? suf[k] / s[k] : 0.0;
}

// select_step of trf.py (reflective Trust Region); false where scipy raises (intersect_trust_region's ValueError)
TF_HD bool select_step(const double x[3], const double Rd[3][3], const double diag_h[3], const double g_h[3], double p[3],
                       double p_h[3], const double d[3], double Delta, double theta, double step[3], double step_h[3],
                       double &pred) {
    double xp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xp[k] = x[k] + p[k];
    if (in_bounds(xp)) {
        pred = -evaluate_quadratic(Rd, g_h, p_h, diag_h);
#pragma unroll
        for (int k = 0; k < 3; ++k) { step[k] = p[k]; step_h[k] = p_h[k]; }
        return true;
    }
    double hits[3], r_h[3], r[3], xb[3], dummy[3];
    const double p_stride = step_size_to_bound(x, p, hits);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r_h[k] = hits[k] != 0 ? -p_h[k] : p_h[k];
        r[k] = d[k] * r_h[k];
        p[k] *= p_stride;
        p_h[k] *= p_stride;
        xb[k] = x[k] + p[k];
    }
    // intersect_trust_region(p_h, r_h, Delta): the larger root
    const double qa = dot3(r_h, r_h);
    if (qa == 0) return false;
    const double qb = dot3(p_h, r_h), qc = dot3(p_h, p_h) - Delta * Delta;
    if (qc > 0) return false;
    const double qd = sqrt(qb * qb - qa * qc);
    const double qq = -(qb + copysign(qd, qb));
    const double t1 = qq / qa, t2 = qc / qq;
    const double to_tr = t1 < t2 ? t2 : t1;
    const double to_bound = step_size_to_bound(xb, r, dummy);
    double r_stride = pymin(to_bound, to_tr), r_lo, r_up;
    if (r_stride > 0) {
        r_lo = (1 - theta) * p_stride / r_stride;
        r_up = r_stride == to_bound ? theta * to_bound : to_tr;
    } else {
        r_lo = 0;
        r_up = -1;
    }
    double r_value;
    if (r_lo <= r_up) {
        double a, b, c;
        build_quadratic_1d(Rd, g_h, r_h, diag_h, p_h, a, b, c);
        minimize_quadratic_1d(a, b, r_lo, r_up, c, r_stride, r_value);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r_h[k] *= r_stride;
            r_h[k] += p_h[k];
            r[k] = r_h[k] * d[k];
        }
    } else {
        r_value = TF_INF;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] *= theta; p_h[k] *= theta; }
    const double p_value = evaluate_quadratic(Rd, g_h, p_h, diag_h);
    double ag_h[3], ag[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ag_h[k] = -g_h[k]; ag[k] = d[k] * ag_h[k]; }
    const double to_tr_g = Delta / norm3(ag_h);
    const double to_bound_g = step_size_to_bound(x, ag, dummy);
    double ag_stride = to_bound_g < to_tr_g ? theta * to_bound_g : to_tr_g;
    double a, b, c, ag_value;
    build_quadratic_1d(Rd, g_h, ag_h, diag_h, nullptr, a, b, c);
    minimize_quadratic_1d(a, b, 0, ag_stride, 0.0, ag_stride, ag_value);
#pragma unroll
    for (int k = 0; k < 3; ++k) { ag_h[k] *= ag_stride; ag[k] *= ag_stride; }
    if (p_value < r_value && p_value < ag_value) {
        pred = -p_value;
#pragma unroll
        for (int k = 0; k < 3; ++k) { step[k] = p[k]; step_h[k] = p_h[k]; }
    } else if (r_value < p_value && r_value < ag_value) {
        pred = -r_value;
#pragma unroll
        for (int k = 0; k < 3; ++k) { step[k] = r[k]; step_h[k] = r_h[k]; }
    } else {
        pred = -ag_value;
#pragma unroll
        for (int k = 0; k < 3; ++k) { step[k] = ag[k]; step_h[k] = ag_h[k]; }
    }
    return true;
}

// curve_fit(...) of helpers/features.py:_fit_power_law.  Returns false where that call raises (infeasible p0, non-finite
// data or residuals, maxfev reached, a ValueError inside the step selection): the caller then uses (D, alpha) = (0, 0),
// r2 = 0.  On success x = (D, alpha, offset).
TF_HD bool fit_power_law(const Fit &F, double x[3]) {
    const double ftol = 1e-8, xtol = 1e-8, gtol = 1e-8;
    const int max_nfev = 10000;
    for (int i = 0; i < F.m; ++i)
        if (!isfinite(F.msd[i])) return false;                     // np.asarray_chkfinite
    x[0] = F.msd[0] / (4.0 * F.dt);
    x[1] = 1.0;
    x[2] = 0.001;
    if (!in_bounds(x)) return false;                               // "Initial guess is outside of provided bounds"
    // make_strictly_feasible(x0, lb, ub) with rstep = 1e-10
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lb = lb_of(k), ub = ub_of(k);
        const double lo = x[k] - lb, up = ub - x[k];
        const double lth = 1e-10 * fmax(1.0, fabs(lb)), uth = 1e-10 * fmax(1.0, fabs(ub));
        int act = 0;
        if (isfinite(lb) && lo <= fmin(up, lth)) act = -1;
        if (isfinite(ub) && up <= fmin(lo, uth)) act = 1;
        if (act == -1) x[k] = lb + 1e-10 * fmax(1.0, fabs(lb));
        if (act == 1) x[k] = ub - 1e-10 * fmax(1.0, fabs(ub));
        if (x[k] < lb || x[k] > ub) x[k] = 0.5 * (lb + ub);
    }
    double cost;
    if (!cost_at(F, x, cost)) return false;                        // "Residuals are not finite in the initial point."
    int nfev = 1;
    double R[3][3], qtf[3], g[3];
    jacobian(F, x, R, qtf, g);
    // trf_bounds (x_scale = 1, linear loss, tr_solver 'exact')
    double v[3], dv[3];
    auto cl_scaling = [&]() {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = 1.0;
            dv[k] = 0.0;
            if (g[k] < 0 && isfinite(ub_of(k))) { v[k] = ub_of(k) - x[k]; dv[k] = -1.0; }
            if (g[k] > 0 && isfinite(lb_of(k))) { v[k] = x[k] - lb_of(k); dv[k] = 1.0; }
        }
    };
    cl_scaling();
    double Delta;
    {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = x[k] / sqrt(v[k]);
        Delta = norm3(t);
        if (Delta == 0) Delta = 1.0;
    }
    double alpha = 0.0;
    int status = -1;                                               // None
    for (;;) {
        cl_scaling();
        double g_norm = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) g_norm = npmax(g_norm, fabs(g[k] * v[k]));
        if (g_norm < gtol) status = 1;
        if (status != -1 || nfev == max_nfev) break;
        double d[3], diag_h[3], g_h[3], Rd[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = sqrt(v[k]);
            diag_h[k] = g[k] * dv[k];
            g_h[k] = d[k] * g[k];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rd[i][j] = j >= i ? R[i][j] * d[j] : 0.0;
        double s[3], V[3][3], uf[3];
        augmented_svd(Rd, qtf, diag_h, s, V, uf);
        const double theta = pymax(0.995, 1 - g_norm);
        double actual_reduction = -1, x_new[3], cost_new = cost;
        while (actual_reduction <= 0 && nfev < max_nfev) {
            double p_h[3], p[3], step[3], step_h[3], pred;
            solve_lsq_trust_region(F.m, uf, s, V, Delta, alpha, p_h);
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = d[k] * p_h[k];
            if (!select_step(x, Rd, diag_h, g_h, p, p_h, d, Delta, theta, step, step_h, pred)) return false;
            // make_strictly_feasible(x + step, lb, ub, rstep=0)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double lb = lb_of(k), ub = ub_of(k);
                double xn = x[k] + step[k];
                if (xn <= lb) xn = nextafter(lb, ub);
                else if (xn >= ub) xn = nextafter(ub, lb);
                if (xn < lb || xn > ub) xn = 0.5 * (lb + ub);
                x_new[k] = xn;
            }
            const bool finite = cost_at(F, x_new, cost_new);
            nfev += 1;
            const double step_h_norm = norm3(step_h);
            if (!finite) {
                Delta = 0.25 * step_h_norm;
                continue;
            }
            actual_reduction = cost - cost_new;
            // update_tr_radius
            double ratio, Delta_new = Delta;
            if (pred > 0) ratio = actual_reduction / pred;
            else if (pred == actual_reduction && actual_reduction == 0) ratio = 1;
            else ratio = 0;
            if (ratio < 0.25) Delta_new = 0.25 * step_h_norm;
            else if (ratio > 0.75 && step_h_norm > 0.95 * Delta) Delta_new *= 2.0;
            // check_termination
            const double step_norm = norm3(step), x_norm = norm3(x);
            const bool ftol_ok = actual_reduction < ftol * cost && ratio > 0.25;
            const bool xtol_ok = step_norm < xtol * (xtol + x_norm);
            if (ftol_ok && xtol_ok) status = 4;
            else if (ftol_ok) status = 2;
            else if (xtol_ok) status = 3;
            if (status != -1) break;
            alpha *= Delta / Delta_new;
            Delta = Delta_new;
        }
        if (actual_reduction > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = x_new[k];
            cost = cost_new;
            jacobian(F, x, R, qtf, g);
        }
    }
    return status > 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the 25 descriptors of n positions pos(i) = (P[2i], P[2i+1]); msd: a buffer of at least n values (lags 1 .. nl)
// ---------------------------------------------------------------------------------------------------------------------
TF_HD void features(const Buf &P, int n, double dt, const Buf &msd, double *out) {
    const double nan = __builtin_nan("");
    if (n < 3) {
        for (int k = 0; k < N_FEATURES; ++k) out[k] = nan;
        return;
    }
    const int nl = (n > 20 ? (int)(n * 0.5) : n) - 1;
    // lag moments: msd (kept) and the gaussianity sum over lags with a non-zero MSD
    double gsum = 0.0, msd_sum = 0.0;
    int gcnt = 0;
    for (int lag = 1; lag <= nl; ++lag) {
        // the MSD feeds the fit: summed in numpy's order, so that it matches the reference's to the last bit
        const auto sq = [&](int j) {
            const double dx = P[2 * (j + lag)] - P[2 * j], dy = P[2 * (j + lag) + 1] - P[2 * j + 1];
            return dx * dx + dy * dy;
        };
        const double m2 = pairwise_sum<3>(sq, 0, n - lag) / (double)(n - lag);
        double m4 = 0.0;
        for (int j = 0; j + lag < n; ++j) {
            const double dx = P[2 * (j + lag)] - P[2 * j], dy = P[2 * (j + lag) + 1] - P[2 * j + 1];
            m4 += pow(dx, 4.0) + pow(dy, 4.0);
        }
        m4 /= (double)(n - lag);
        msd[lag - 1] = m2;
        msd_sum += m2;
        if (m2 > 0) {
            gsum += m4 / (2 * (m2 * m2));
            ++gcnt;
        }
    }
    // largest squared pair distance, steps
    double max_sq = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double dx = P[2 * i] - P[2 * j], dy = P[2 * i + 1] - P[2 * j + 1];
            max_sq = fmax(max_sq, dx * dx + dy * dy);
        }
    double bottom = 0.0, total = 0.0, smin = TF_INF, smax = -TF_INF, dsum = 0.0;
    int nsmall = 0, nlarge = 0, npos_dots = 0, nsame = 0;
    double pdx = 0, pdy = 0, pdot = 0;
    for (int i = 0; i + 1 < n; ++i) {
        const double dx = P[2 * i + 2] - P[2 * i], dy = P[2 * i + 3] - P[2 * i + 1];
        const double sl = sqrt(dx * dx + dy * dy);
        bottom += sl * sl;
        total += sl;
        smin = fmin(smin, sl);
        smax = fmax(smax, sl);
        nsmall += sl < 0.1;
        nlarge += sl > 0.4;
        if (i > 0) {
            const double dot = pdx * dx + pdy * dy;
            dsum += dot;
            npos_dots += dot > 0;
            if (i > 1) nsame += npsign(dot) == npsign(pdot);
            pdot = dot;
        }
        pdx = dx;
        pdy = dy;
    }
    const int ns = n - 1, nd = n - 2;
    const double mean_sl = total / ns;
    double var = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
        const double dx = P[2 * i + 2] - P[2 * i], dy = P[2 * i + 3] - P[2 * i + 1];
        const double e = sqrt(dx * dx + dy * dy) - mean_sl;
        var += e * e;
    }
    // fit
    Fit F{msd, nl, dt};
    double x[3];
    double D = 0.0, alpha = 0.0, r2 = 0.0;
    if (fit_power_law(F, x)) {
        D = x[0];
        alpha = x[1];
        const double mmean = msd_sum / nl;
        double sres = 0.0, stot = 0.0;
        for (int i = 0; i < nl; ++i) {
            const double r = msd[i] - ((4.0 * D) * pow((double)(i + 1) * dt, alpha) + x[2]);
            const double e = msd[i] - mmean;
            sres += r * r;
            stot += e * e;
        }
        r2 = 1 - sres / stot;
    }
    // efficiency
    const double dxe = P[2 * (n - 1)] - P[0], dye = P[2 * (n - 1) + 1] - P[1];
    const double top = dxe * dxe + dye * dye;
    double eff_log, eff;
    if (bottom == 0) {
        eff_log = -TF_INF;
        eff = 0;
    } else {
        eff = top / ((n - 1) * bottom);
        eff_log = log(eff);
    }
    const double fractal = total == 0 ? 1.0 : log((double)n) / (log((double)n) + log(sqrt(max_sq) / total));
    const double gauss = gcnt ? gsum / gcnt : nan;
    // kurtosis of the projection on the dominant axis of the sample covariance (closed-form 2x2 eigenvector)
    double kurt;
    {
        double mx = 0, my = 0;
        for (int i = 0; i < n; ++i) { mx += P[2 * i]; my += P[2 * i + 1]; }
        mx /= n;
        my /= n;
        double sxx = 0, syy = 0, sxy = 0;
        for (int i = 0; i < n; ++i) {
            const double ex = P[2 * i] - mx, ey = P[2 * i + 1] - my;
            sxx += ex * ex; syy += ey * ey; sxy += ex * ey;
        }
        const double a = sxx / (n - 1), c = syy / (n - 1), b = sxy / (n - 1);
        double ux, uy;
        if (b == 0) {                              // numpy: eigenvalues in order (a, c); ties keep the second
            ux = a > c ? 1.0 : 0.0;
            uy = a > c ? 0.0 : 1.0;
        } else {
            const double h = 0.5 * (a - c), l1 = 0.5 * (a + c) + hypot(h, b);
            if (a >= c) { ux = l1 - c; uy = b; } else { ux = b; uy = l1 - a; }
            const double nn = hypot(ux, uy);
            ux /= nn;
            uy /= nn;
        }
        double pm = 0;
        for (int i = 0; i < n; ++i) pm += P[2 * i] * ux + P[2 * i + 1] * uy;
        pm /= n;
        double c2 = 0, c4 = 0;
        for (int i = 0; i < n; ++i) {
            const double e = (P[2 * i] * ux + P[2 * i + 1] * uy) - pm;
            c2 += e * e;
            c4 += pow(e, 4.0);
        }
        c2 /= n;
        c4 /= n;
        kurt = c4 / (c2 * c2);
    }
    double msd_ratio = nan;
    if (nl >= 2) {
        double s = 0.0;
        for (int k = 1; k < nl; ++k) s += msd[k - 1] / msd[k] - (double)k / (double)(k + 1);
        msd_ratio = s / (nl - 1);
    }
    const double r0 = sqrt(max_sq) / 2;
    const double trapped = (r0 == 0 || D == 0) ? 0.0 : 1 - exp(0.2045 - 0.25117 * (D * n) / (r0 * r0));
    // convex hull area: gift wrapping (counter-clockwise), shoelace relative to the start point; collinear -> 0
    double hull = 0.0;
    {
        int start = 0;
        for (int i = 1; i < n; ++i)
            if (P[2 * i] < P[2 * start] || (P[2 * i] == P[2 * start] && P[2 * i + 1] < P[2 * start + 1])) start = i;
        const double ox = P[2 * start], oy = P[2 * start + 1];
        int cur = start;
        double area2 = 0.0;
        for (int step = 0; step < n; ++step) {
            const double cx = P[2 * cur] - ox, cy = P[2 * cur + 1] - oy;
            int nxt = -1;
            double nx = 0, ny = 0;
            for (int q = 0; q < n; ++q) {
                const double qx = P[2 * q] - ox, qy = P[2 * q + 1] - oy;
                if (qx == cx && qy == cy) continue;
                if (nxt < 0) { nxt = q; nx = qx; ny = qy; continue; }
                const double cr = (nx - cx) * (qy - cy) - (ny - cy) * (qx - cx);
                const bool farther = (qx - cx) * (qx - cx) + (qy - cy) * (qy - cy) > (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
                if (cr < 0 || (cr == 0 && farther)) { nxt = q; nx = qx; ny = qy; }
            }
            if (nxt < 0) break;                                     // all points coincide
            area2 += cx * ny - nx * cy;
            cur = nxt;
            if (nx == 0 && ny == 0) break;                          // back at the start
        }
        hull = 0.5 * fabs(area2);
    }
    const double mean_msd = msd_sum / nl;
    out[0] = alpha;
    out[1] = D;
    out[2] = r2;
    out[3] = eff_log;
    out[4] = eff;
    out[5] = fractal;
    out[6] = gauss;
    out[7] = kurt;
    out[8] = msd_ratio;
    out[9] = trapped;
    out[10] = (double)n;
    out[11] = mean_sl;
    out[12] = mean_msd;
    out[13] = dsum / nd;
    out[14] = nd > 1 ? (double)nsame / (nd - 1) : nan;
    out[15] = (double)npos_dots / nd;
    out[16] = total;
    out[17] = smin;
    out[18] = smax;
    out[19] = smax - smin;
    out[20] = total / n;
    out[21] = (mean_sl > 0 && ns > 1) ? sqrt(var / (ns - 1)) / mean_sl : nan;
    out[22] = (double)nsmall / ns;
    out[23] = (double)nlarge / ns;
    out[24] = hull;
}

}  // namespace trajfeat
