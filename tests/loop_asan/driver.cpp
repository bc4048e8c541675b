// Stand-alone driver of the pose graph (pose_graph.cpp) for the sanitizer build
// of tests/loop_asan: the biased C5 keyframe graph of tests/test_loop.py (17
// ground-truth poses, every odometry step right-multiplied by a fixed twist,
// one exact loop edge), the same chain with loop edges between free nodes (the
// long rows of the envelope solver), the argument errors and the
// interpolation.  Exits 0 only when every check holds.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "youth_loop.h"
#include "youth_synth.h"

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);   \
            ++g_failed;                                                 \
        }                                                               \
    } while (0)

static void mul(const double* A, const double* B, double* C)
{
    double O[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
            O[i * 4 + j] = s;
        }
    memcpy(C, O, sizeof(O));
}

static void inv(const double* A, double* B)
{
    double O[16] = {0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) O[r * 4 + c] = A[c * 4 + r];
        O[r * 4 + 3] = -(A[r] * A[3] + A[4 + r] * A[7] + A[8 + r] * A[11]);
    }
    O[15] = 1.0;
    memcpy(B, O, sizeof(O));
}

// exp of the twist (w, v), rotation first
static void se3_exp(const double* xi, double* T)
{
    const double* w = xi;
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double S[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double S2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            S2[r * 3 + c] = S[r * 3] * S[c] + S[r * 3 + 1] * S[3 + c] + S[r * 3 + 2] * S[6 + c];
    const double a = sin(th) / th, b = (1.0 - cos(th)) / (th * th), c3 = (th - sin(th)) / (th * th * th);
    memset(T, 0, 16 * sizeof(double));
    for (int r = 0; r < 3; ++r) {
        double t = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double I = r == c ? 1.0 : 0.0;
            T[r * 4 + c] = I + a * S[r * 3 + c] + b * S2[r * 3 + c];
            t += (I + b * S[r * 3 + c] + c3 * S2[r * 3 + c]) * xi[3 + c];
        }
        T[r * 4 + 3] = t;
    }
    T[15] = 1.0;
}

// (degrees, metres) between two poses
static void pose_error(const double* T, const double* G, double* deg, double* m)
{
    double Gi[16], D[16];
    inv(G, Gi);
    mul(Gi, T, D);
    const double vx = 0.5 * (D[9] - D[6]), vy = 0.5 * (D[2] - D[8]), vz = 0.5 * (D[4] - D[1]);
    *deg = atan2(sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (D[0] + D[5] + D[10] - 1.0)) * 180.0 / M_PI;
    *m = sqrt(D[3] * D[3] + D[7] * D[7] + D[11] * D[11]);
}

int main()
{
    const int n = 17;
    std::vector<double> X((size_t)n * 16);
    {
        const int W = 32, H = 24;
        youth_intrinsics K = {35.0f, 35.0f, 16.0f, 12.0f, 1000.0f};
        std::vector<int16_t> frame((size_t)W * H);
        for (int k = 0; k < n; ++k) {
            const int f = k < 16 ? 40 * k : 630;
            youth_synth_sequence(0x5EED1000ull, f, 1, W, H, &K, 0, frame.data(), X.data() + (size_t)k * 16);
        }
    }
    const double bias[6] = {0.004, -0.006, 0.005, 0.006, -0.004, 0.008};
    double B[16];
    se3_exp(bias, B);
    std::vector<youth_loop_edge> edges((size_t)n);
    std::vector<double> Xb(X.begin(), X.begin() + 16);
    for (int k = 1; k < n; ++k) {
        youth_loop_edge& e = edges[k - 1];
        memset(&e, 0, sizeof(e));
        e.i = k - 1;
        e.j = k;
        e.w = 1.0;
        double Ai[16];
        inv(X.data() + (size_t)(k - 1) * 16, Ai);
        mul(Ai, X.data() + (size_t)k * 16, e.Z);
        mul(e.Z, B, e.Z);
        double next[16];
        mul(Xb.data() + (size_t)(k - 1) * 16, e.Z, next);
        Xb.insert(Xb.end(), next, next + 16);
    }
    {
        youth_loop_edge& e = edges[n - 1];   // the exact loop edge (0, 16)
        memset(&e, 0, sizeof(e));
        e.i = 0;
        e.j = n - 1;
        e.w = 1.0;
        double Ai[16];
        inv(X.data(), Ai);
        mul(Ai, X.data() + (size_t)(n - 1) * 16, e.Z);
    }

    // case (b): the loop is pulled shut
    std::vector<double> Xo = Xb;
    double c0 = -1.0, c1 = -1.0, d0, m0, d1, m1;
    CHECK(youth_posegraph_optimize(n, Xo.data(), n, edges.data(), nullptr, &c0, &c1) == YOUTH_OK);
    pose_error(Xb.data() + 16 * 16, X.data() + 16 * 16, &d0, &m0);
    pose_error(Xo.data() + 16 * 16, X.data() + 16 * 16, &d1, &m1);
    printf("cost %.6g -> %.6g; node 16: %.3f deg / %.2f mm -> %.3f deg / %.2f mm\n", c0, c1, d0, m0 * 1e3,
           d1, m1 * 1e3);
    CHECK(c1 < c0 && c1 >= 0.0);
    CHECK(d1 < d0 / 4 && m1 < m0 / 4);
    CHECK(memcmp(Xo.data(), Xb.data(), 16 * sizeof(double)) == 0);
    // exact odometry: nothing moves
    {
        std::vector<youth_loop_edge> ex = edges;
        double Bi[16];
        inv(B, Bi);
        for (int k = 0; k < n - 1; ++k) mul(ex[k].Z, Bi, ex[k].Z);
        std::vector<double> Xe = X;
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, ex.data(), nullptr, &c0, &c1) == YOUTH_OK);
        double worst = 0.0;
        for (size_t a = 0; a < Xe.size(); ++a) worst = fmax(worst, fabs(Xe[a] - X[a]));
        CHECK(worst <= 1e-9);
    }

    // beyond the band: exact loop edges between free nodes, (14, 5) given with
    // i > j, two sharing node 3, weights other than 1, one edge of weight 0 with
    // a wrong Z, w_rot != w_trans.  H gets blocks far off the diagonal and the
    // envelope solver long rows.
    {
        const int li[4] = {3, 14, 3, 6}, lj[4] = {12, 5, 9, 10};
        const double lw[4] = {2.0, 0.5, 1.0, 0.0};
        std::vector<youth_loop_edge> in(edges.begin(), edges.begin() + (n - 1));
        for (int k = 0; k < 4; ++k) {
            youth_loop_edge e;
            memset(&e, 0, sizeof(e));
            e.i = li[k];
            e.j = lj[k];
            e.w = lw[k];
            double Ai[16];
            inv(X.data() + (size_t)li[k] * 16, Ai);
            mul(Ai, X.data() + (size_t)lj[k] * 16, e.Z);
            if (lw[k] == 0.0) mul(e.Z, B, e.Z);
            in.push_back(e);
        }
        youth_posegraph_params P = youth_posegraph_default_params();
        P.w_rot = 3.0;
        P.w_trans = 0.5;
        std::vector<double> Xi = Xb;
        CHECK(youth_posegraph_optimize(n, Xi.data(), (int)in.size(), in.data(), &P, &c0, &c1) == YOUTH_OK);
        pose_error(Xb.data() + 12 * 16, X.data() + 12 * 16, &d0, &m0);
        pose_error(Xi.data() + 12 * 16, X.data() + 12 * 16, &d1, &m1);
        printf("interior loops: cost %.6g -> %.6g; node 12: %.3f deg / %.2f mm -> %.3f deg / %.2f mm\n", c0, c1,
               d0, m0 * 1e3, d1, m1 * 1e3);
        CHECK(c1 < c0 && c1 >= 0.0);
        CHECK(d1 < d0 && m1 < m0);
        CHECK(memcmp(Xi.data(), Xb.data(), 16 * sizeof(double)) == 0);
        // the edge of weight 0 counts for nothing
        std::vector<double> Xw = Xb;
        double w0, w1, worst = 0.0;
        CHECK(youth_posegraph_optimize(n, Xw.data(), (int)in.size() - 1, in.data(), &P, &w0, &w1) == YOUTH_OK);
        for (size_t a = 0; a < Xw.size(); ++a) worst = fmax(worst, fabs(Xw[a] - Xi[a]));
        CHECK(worst <= 1e-12 && fabs(w0 - c0) <= 1e-12 && fabs(w1 - c1) <= 1e-12);
        // exact odometry: nothing moves
        double Bi[16];
        inv(B, Bi);
        for (int k = 0; k < n - 1; ++k) mul(in[k].Z, Bi, in[k].Z);
        std::vector<double> Xe = X;
        CHECK(youth_posegraph_optimize(n, Xe.data(), (int)in.size(), in.data(), &P, &c0, &c1) == YOUTH_OK);
        worst = 0.0;
        for (size_t a = 0; a < Xe.size(); ++a) worst = fmax(worst, fabs(Xe[a] - X[a]));
        CHECK(worst <= 1e-9 && c0 <= 1e-20 && c1 <= 1e-20);
    }

    // the argument errors leave X alone
    {
        std::vector<double> Xe = Xb;
        youth_posegraph_params P = youth_posegraph_default_params();
        CHECK(P.max_iters == 20 && P.w_rot == 1.0 && P.w_trans == 1.0);
        CHECK(youth_posegraph_optimize(1, Xe.data(), 0, nullptr, nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        CHECK(youth_posegraph_optimize(513, Xe.data(), 0, nullptr, nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        CHECK(youth_posegraph_optimize(n, nullptr, n, edges.data(), nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        std::vector<youth_loop_edge> bad = edges;
        bad[3].j = n;
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, bad.data(), nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        bad = edges;
        bad[3].i = -1;
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, bad.data(), nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        bad = edges;
        bad[5].Z[7] = NAN;
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, bad.data(), nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        Xe[40] = INFINITY;
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, edges.data(), nullptr, nullptr, nullptr) == YOUTH_EINVAL);
        Xe = Xb;
        // node 0 cut off: every other node floats
        CHECK(youth_posegraph_optimize(n, Xe.data(), n - 2, edges.data() + 1, nullptr, nullptr, nullptr) ==
              YOUTH_EINVAL);
        CHECK(memcmp(Xe.data(), Xb.data(), Xb.size() * sizeof(double)) == 0);
        CHECK(strlen(youth_posegraph_last_error()) > 0);
        P.max_iters = 0;   // no iteration: costs equal, poses unchanged
        CHECK(youth_posegraph_optimize(n, Xe.data(), n, edges.data(), &P, &c0, &c1) == YOUTH_OK && c0 == c1);
    }

    // interpolation: five frames on two keyframes
    {
        const int32_t kf[2] = {0, 3};
        std::vector<double> F(Xb.begin(), Xb.begin() + 5 * 16), oldk(32), newk(32);
        memcpy(oldk.data(), F.data(), 16 * sizeof(double));
        memcpy(oldk.data() + 16, F.data() + 3 * 16, 16 * sizeof(double));
        newk = oldk;
        mul(B, oldk.data() + 16, newk.data() + 16);
        std::vector<double> G = F;
        CHECK(youth_posegraph_interpolate(5, G.data(), 2, kf, oldk.data(), newk.data()) == YOUTH_OK);
        CHECK(memcmp(G.data(), F.data(), 16 * sizeof(double)) == 0);
        double worst = 0.0;
        for (int a = 0; a < 16; ++a) worst = fmax(worst, fabs(G[3 * 16 + a] - newk[16 + a]));
        CHECK(worst <= 1e-12);
        double rel0[16], rel1[16], Ai[16];
        inv(F.data() + 3 * 16, Ai);
        mul(Ai, F.data() + 4 * 16, rel0);
        inv(G.data() + 3 * 16, Ai);
        mul(Ai, G.data() + 4 * 16, rel1);
        worst = 0.0;
        for (int a = 0; a < 16; ++a) worst = fmax(worst, fabs(rel0[a] - rel1[a]));
        CHECK(worst <= 1e-12);
        const int32_t bad[2] = {1, 3};
        CHECK(youth_posegraph_interpolate(5, G.data(), 2, bad, oldk.data(), newk.data()) == YOUTH_EINVAL);
        CHECK(youth_posegraph_interpolate(5, G.data(), 0, kf, oldk.data(), newk.data()) == YOUTH_EINVAL);
    }

    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("pose graph ok\n");
    return 0;
}
