// pose_graph.cpp — the pose graph of include/youth_loop.h:
// Gauss-Newton over camera -> world poses with relative-pose edges, and the
// re-hanging of a trajectory on optimised keyframes.  Host only, fp64, no HIP
// include: it builds with any C++17 compiler (tests/loop_asan).
//
// Edge (i, j, Z, w): E = Z^-1 X_i^-1 X_j, e = [Log_SO3(R_E); t_E].  A node moves
// by X <- X D(d), D(d) = [exp(d_w), d_v; 0 1], so with A = X_i^-1 X_j = Z E
//   de/dd_j = [ Jr^-1(e_w)            0     ]   de/dd_i = [ -Jr^-1(e_w) R_A^T    0     ]
//             [ 0                     R_E   ]             [  R_Z^T [t_A]x       -R_Z^T ]
// Jr^-1 the inverse right Jacobian of SO(3).  Node 0 is the gauge: it has no
// columns.  The normal equations are stored dense (6 (n - 1) unknowns, n <=
// 512) and solved by a row-oriented Cholesky factorisation that skips each
// row's leading zeros; its inner loops are dot products of contiguous rows.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "youth_loop.h"

namespace {

thread_local char g_pg_err[256] = "";

__attribute__((format(printf, 2, 3))) int pg_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_pg_err, sizeof(g_pg_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Pose {
    double R[9];
    double t[3];
};

Pose from16(const double* T)
{
    Pose p;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[r * 3 + c] = T[r * 4 + c];
        p.t[r] = T[r * 4 + 3];
    }
    return p;
}

void to16(const Pose& p, double* T)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[r * 4 + c] = p.R[r * 3 + c];
        T[r * 4 + 3] = p.t[r];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// C = A B (3x3)
void mul33(const double* A, const double* B, double* C)
{
    double O[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            O[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
    memcpy(C, O, sizeof(O));
}

// C = A^T B (3x3)
void mulT33(const double* A, const double* B, double* C)
{
    double O[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            O[r * 3 + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
    memcpy(C, O, sizeof(O));
}

Pose compose(const Pose& a, const Pose& b)
{
    Pose o;
    mul33(a.R, b.R, o.R);
    for (int r = 0; r < 3; ++r)
        o.t[r] = a.R[r * 3] * b.t[0] + a.R[r * 3 + 1] * b.t[1] + a.R[r * 3 + 2] * b.t[2] + a.t[r];
    return o;
}

Pose inverse(const Pose& a)
{
    Pose o;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.R[r * 3 + c] = a.R[c * 3 + r];
    for (int r = 0; r < 3; ++r)
        o.t[r] = -(o.R[r * 3] * a.t[0] + o.R[r * 3 + 1] * a.t[1] + o.R[r * 3 + 2] * a.t[2]);
    return o;
}

void skew(const double* v, double* S)
{
    S[0] = 0.0, S[1] = -v[2], S[2] = v[1];
    S[3] = v[2], S[4] = 0.0, S[5] = -v[0];
    S[6] = -v[1], S[7] = v[0], S[8] = 0.0;
}

// Rodrigues: exp of the rotation vector w
void exp_so3(const double* w, double* R)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    double a, b;  // sin(th)/th, (1 - cos(th))/th^2
    if (th < 1e-6) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    double S[9], S2[9];
    skew(w, S);
    mul33(S, S, S2);
    for (int k = 0; k < 9; ++k) R[k] = a * S[k] + b * S2[k];
    R[0] += 1.0, R[4] += 1.0, R[8] += 1.0;
}

// The rotation vector of R (angle below pi; at pi the axis' sign is lost and
// the vector of the antisymmetric part, zero, is returned scaled: an edge that
// far from its measurement is not one this optimiser is for)
void log_so3(const double* R, double* w)
{
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double th = atan2(s, c);
    const double k = s < 1e-9 ? 1.0 + th * th / 6.0 : th / s;
    for (int a = 0; a < 3; ++a) w[a] = k * v[a];
}

// Jr^-1(w) = I + 1/2 [w]x + (1/th^2 - (1 + cos th) / (2 th sin th)) [w]x^2
void jr_inv(const double* w, double* J)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    const double k = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0
                               : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    double S[9], S2[9];
    skew(w, S);
    mul33(S, S, S2);
    for (int a = 0; a < 9; ++a) J[a] = 0.5 * S[a] + k * S2[a];
    J[0] += 1.0, J[4] += 1.0, J[8] += 1.0;
}

// rows made orthonormal again (Gram-Schmidt, the third row a cross product)
void orthonormalise(double* R)
{
    double* r0 = R;
    double* r1 = R + 3;
    double* r2 = R + 6;
    double n = sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]);
    for (int a = 0; a < 3; ++a) r0[a] /= n;
    const double d = r1[0] * r0[0] + r1[1] * r0[1] + r1[2] * r0[2];
    for (int a = 0; a < 3; ++a) r1[a] -= d * r0[a];
    n = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
    for (int a = 0; a < 3; ++a) r1[a] /= n;
    r2[0] = r0[1] * r1[2] - r0[2] * r1[1];
    r2[1] = r0[2] * r1[0] - r0[0] * r1[2];
    r2[2] = r0[0] * r1[1] - r0[1] * r1[0];
}

struct Residual {
    double e[6];
    Pose E, A;
};

Residual residual(const Pose& Xi, const Pose& Xj, const Pose& Z)
{
    Residual r;
    r.A = compose(inverse(Xi), Xj);
    r.E = compose(inverse(Z), r.A);
    log_so3(r.E.R, r.e);
    for (int a = 0; a < 3; ++a) r.e[3 + a] = r.E.t[a];
    return r;
}

double graph_cost(const std::vector<Pose>& X, const std::vector<Pose>& Z, int n_edges,
                  const youth_loop_edge* edges, const youth_posegraph_params& P)
{
    double cost = 0.0;
    for (int k = 0; k < n_edges; ++k) {
        const Residual r = residual(X[edges[k].i], X[edges[k].j], Z[k]);
        const double* e = r.e;
        cost += edges[k].w * (P.w_rot * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) +
                              P.w_trans * (e[3] * e[3] + e[4] * e[4] + e[5] * e[5]));
    }
    return cost;
}

bool finite16(const double* T)
{
    for (int a = 0; a < 16; ++a)
        if (!isfinite(T[a])) return false;
    return true;
}

// sum a[k] b[k] over k0 <= k < k1 in four independent partial sums (the chain
// of one accumulator's adds is what bounds a plain loop)
double dot(const double* a, const double* b, int k0, int k1)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = k0;
    for (; k + 3 < k1; k += 4) {
        s0 += a[k] * b[k];
        s1 += a[k + 1] * b[k + 1];
        s2 += a[k + 2] * b[k + 2];
        s3 += a[k + 3] * b[k + 3];
    }
    for (; k < k1; ++k) s0 += a[k] * b[k];
    return (s0 + s1) + (s2 + s3);
}

// In-place Cholesky of the symmetric m x m matrix in H (lower triangle read
// and overwritten by L), then L L^T x = b solved into b.  false: not positive
// definite.  Envelope form: row i of L is zero left of the row's first
// non-zero of H, first[i] (a chain of odometry edges is a band of 12; a loop
// edge lengthens the rows of its later node), so every dot product starts at
// the later of the two rows' firsts.
bool cholesky_solve(double* H, double* b, int m)
{
    std::vector<int> first((size_t)m);
    for (int i = 0; i < m; ++i) {
        const double* Hi = H + (size_t)i * m;
        int f = 0;
        while (f < i && Hi[f] == 0.0) ++f;
        first[i] = f;
    }
    for (int i = 0; i < m; ++i) {
        double* Li = H + (size_t)i * m;
        const double diag = Li[i];   // a pivot that cancels to rounding noise is a zero pivot
        for (int j = first[i]; j <= i; ++j) {
            const double* Lj = H + (size_t)j * m;
            const int k0 = first[i] > first[j] ? first[i] : first[j];
            const double s = Li[j] - (k0 < j ? dot(Li, Lj, k0, j) : 0.0);
            if (j < i) {
                Li[j] = s / Lj[j];
            } else {
                if (!(s > 1e-12 * diag) || !isfinite(s)) return false;
                Li[i] = sqrt(s);
            }
        }
    }
    for (int i = 0; i < m; ++i) {   // L y = b
        const double* Li = H + (size_t)i * m;
        b[i] = (b[i] - dot(Li, b, first[i], i)) / Li[i];
    }
    for (int i = m - 1; i >= 0; --i) {   // L^T x = y, by rows of L
        const double* Li = H + (size_t)i * m;
        b[i] /= Li[i];
        for (int k = first[i]; k < i; ++k) b[k] -= Li[k] * b[i];
    }
    return true;
}

}  // namespace

extern "C" {

const char* youth_posegraph_last_error(void) { return g_pg_err; }

youth_posegraph_params youth_posegraph_default_params(void)
{
    youth_posegraph_params p;
    p.w_rot = 1.0;
    p.w_trans = 1.0;
    p.max_iters = 20;
    return p;
}

int youth_posegraph_optimize(int n, double* X16, int n_edges, const youth_loop_edge* edges,
                             const youth_posegraph_params* params, double* cost_before,
                             double* cost_after)
{
    static const char* who = "youth_posegraph_optimize";
    const youth_posegraph_params P = params ? *params : youth_posegraph_default_params();
    if (!X16 || n < 2 || n > YOUTH_LOOP_MAX_KEYFRAMES || n_edges < 0 || (n_edges > 0 && !edges))
        return pg_fail(YOUTH_EINVAL, "%s: %d nodes, %d edges (need 2 <= nodes <= %d)", who, n, n_edges,
                       YOUTH_LOOP_MAX_KEYFRAMES);
    if (!isfinite(P.w_rot) || !isfinite(P.w_trans) || !(P.w_rot > 0.0) || !(P.w_trans > 0.0) ||
        P.max_iters < 0)
        return pg_fail(YOUTH_EINVAL, "%s: bad parameters", who);
    for (int k = 0; k < n; ++k)
        if (!finite16(X16 + (size_t)k * 16)) return pg_fail(YOUTH_EINVAL, "%s: node %d is not finite", who, k);
    for (int k = 0; k < n_edges; ++k) {
        const youth_loop_edge& e = edges[k];
        if (e.i < 0 || e.i >= n || e.j < 0 || e.j >= n || e.i == e.j)
            return pg_fail(YOUTH_EINVAL, "%s: edge %d joins nodes %d and %d of %d", who, k, e.i, e.j, n);
        if (!finite16(e.Z) || !isfinite(e.w) || e.w < 0.0)
            return pg_fail(YOUTH_EINVAL, "%s: edge %d is not finite or has a negative weight", who, k);
    }
    std::vector<Pose> X, Z;
    std::vector<double> H, g;
    const int m = 6 * (n - 1);
    try {
        X.resize((size_t)n);
        Z.resize((size_t)n_edges);
        H.resize((size_t)m * m);
        g.resize((size_t)m);
    } catch (const std::bad_alloc&) {
        return pg_fail(YOUTH_ENOMEM, "%s: no memory for a %d x %d system", who, m, m);
    }
    for (int k = 0; k < n; ++k) X[k] = from16(X16 + (size_t)k * 16);
    for (int k = 0; k < n_edges; ++k) Z[k] = from16(edges[k].Z);
    const double c0 = graph_cost(X, Z, n_edges, edges, P);

    for (int it = 0; it < P.max_iters; ++it) {
        std::fill(H.begin(), H.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        for (int k = 0; k < n_edges; ++k) {
            const int ni = edges[k].i, nj = edges[k].j;
            const Residual r = residual(X[ni], X[nj], Z[k]);
            // the two 6x6 blocks of the edge's Jacobian
            double Ji[36] = {0}, Jj[36] = {0};
            double Jr[9], JrRA[9], RzT_tA[9], S[9];
            jr_inv(r.e, Jr);
            for (int a = 0; a < 3; ++a)        // Jr^-1 R_A^T
                for (int b = 0; b < 3; ++b)
                    JrRA[a * 3 + b] = Jr[a * 3] * r.A.R[b * 3] + Jr[a * 3 + 1] * r.A.R[b * 3 + 1] +
                                      Jr[a * 3 + 2] * r.A.R[b * 3 + 2];
            skew(r.A.t, S);
            mulT33(Z[k].R, S, RzT_tA);         // R_Z^T [t_A]x
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    Jj[a * 6 + b] = Jr[a * 3 + b];
                    Jj[(3 + a) * 6 + 3 + b] = r.E.R[a * 3 + b];
                    Ji[a * 6 + b] = -JrRA[a * 3 + b];
                    Ji[(3 + a) * 6 + b] = RzT_tA[a * 3 + b];
                    Ji[(3 + a) * 6 + 3 + b] = -Z[k].R[b * 3 + a];
                }
            double wt[6];
            for (int a = 0; a < 6; ++a) wt[a] = edges[k].w * (a < 3 ? P.w_rot : P.w_trans);
            const int node[2] = {ni, nj};
            const double* J[2] = {Ji, Jj};
            for (int p = 0; p < 2; ++p) {
                if (node[p] == 0) continue;
                const int rp = 6 * (node[p] - 1);
                for (int a = 0; a < 6; ++a) {
                    double s = 0.0;
                    for (int c = 0; c < 6; ++c) s += J[p][c * 6 + a] * wt[c] * r.e[c];
                    g[rp + a] += s;
                }
                for (int q = 0; q < 2; ++q) {
                    if (node[q] == 0) continue;
                    const int rq = 6 * (node[q] - 1);
                    if (rq > rp) continue;     // the lower triangle is enough
                    for (int a = 0; a < 6; ++a)
                        for (int b = 0; b < 6; ++b) {
                            double s = 0.0;
                            for (int c = 0; c < 6; ++c) s += J[p][c * 6 + a] * wt[c] * J[q][c * 6 + b];
                            H[(size_t)(rp + a) * m + rq + b] += s;
                        }
                }
            }
        }
        for (int a = 0; a < m; ++a) g[a] = -g[a];
        if (!cholesky_solve(H.data(), g.data(), m))
            return pg_fail(YOUTH_EINVAL, "%s: the system is not positive definite (a node no edge reaches?)",
                           who);
        double dmax = 0.0;
        for (int k = 1; k < n; ++k) {
            const double* d = g.data() + 6 * (k - 1);
            double dR[9];
            exp_so3(d, dR);
            Pose& x = X[k];
            for (int a = 0; a < 3; ++a)
                x.t[a] += x.R[a * 3] * d[3] + x.R[a * 3 + 1] * d[4] + x.R[a * 3 + 2] * d[5];
            mul33(x.R, dR, x.R);
            orthonormalise(x.R);
            for (int a = 0; a < 6; ++a) dmax = fmax(dmax, fabs(d[a]));
        }
        if (dmax < 1e-12) break;
    }
    if (cost_before) *cost_before = c0;
    if (cost_after) *cost_after = graph_cost(X, Z, n_edges, edges, P);
    for (int k = 1; k < n; ++k) to16(X[k], X16 + (size_t)k * 16);
    return YOUTH_OK;
}

int youth_posegraph_interpolate(int n_frames, double* X16, int n_kf, const int32_t* kf_frame,
                                const double* X_kf_old, const double* X_kf_new)
{
    static const char* who = "youth_posegraph_interpolate";
    if (n_frames < 0 || n_kf < 1 || !kf_frame || !X_kf_old || !X_kf_new || (n_frames > 0 && !X16))
        return pg_fail(YOUTH_EINVAL, "%s: bad arguments", who);
    if (kf_frame[0] != 0) return pg_fail(YOUTH_EINVAL, "%s: the first keyframe must be frame 0", who);
    for (int k = 1; k < n_kf; ++k)
        if (kf_frame[k] <= kf_frame[k - 1])
            return pg_fail(YOUTH_EINVAL, "%s: keyframe frames must ascend", who);
    for (int k = 0; k < n_kf; ++k)
        if (!finite16(X_kf_old + (size_t)k * 16) || !finite16(X_kf_new + (size_t)k * 16))
            return pg_fail(YOUTH_EINVAL, "%s: keyframe %d is not finite", who, k);
    for (int f = 0; f < n_frames; ++f)
        if (!finite16(X16 + (size_t)f * 16)) return pg_fail(YOUTH_EINVAL, "%s: frame %d is not finite", who, f);
    int kf = 0;
    for (int f = 0; f < n_frames; ++f) {
        while (kf + 1 < n_kf && kf_frame[kf + 1] <= f) ++kf;
        const Pose rel = compose(inverse(from16(X_kf_old + (size_t)kf * 16)), from16(X16 + (size_t)f * 16));
        to16(compose(from16(X_kf_new + (size_t)kf * 16), rel), X16 + (size_t)f * 16);
    }
    return YOUTH_OK;
}

}  // extern "C"
