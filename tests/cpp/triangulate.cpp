// cv-geom's doc-test (cv-geom/src/triangulation.rs:26-38) restated against include/akaze.hpp and run as a native process
// linked to libakz.so: point (0.3, 0.1, 2.0), pose translation (0.1, 0.1, 0.1), rotation Rotation3::new((0.1, 0.1, 0.1)).
#include <cmath>
#include <cstdio>

#include "akaze.hpp"

static std::array<double, 3> unit(double x, double y, double z)
{
    const double n = std::sqrt(x * x + y * y + z * z);
    return {x / n, y / n, z / n};
}

int main()
{
    // Rotation3::new(v): Rodrigues' formula for the scaled axis v
    const double v[3] = {0.1, 0.1, 0.1};
    const double th = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double k[3] = {v[0] / th, v[1] / th, v[2] / th};
    const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int m = 0; m < 3; ++m) kk += K[i][m] * K[m][j];
            R[i][j] = (i == j ? 1.0 : 0.0) + std::sin(th) * K[i][j] + (1.0 - std::cos(th)) * kk;
        }
    cv_core::CameraToCamera pose{};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pose.rt[i * 4 + j] = R[i][j];
        pose.rt[i * 4 + 3] = 0.1;
    }
    const double X[3] = {0.3, 0.1, 2.0};
    double q[3];
    for (int i = 0; i < 3; ++i) q[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + 0.1;
    const auto a = unit(X[0], X[1], X[2]), b = unit(q[0], q[1], q[2]);
    cv_geom::LinearEigenTriangulator tri;
    const auto p = tri.triangulate_relative(pose, a, b);
    if (!p) { std::printf("no point, reason %d\n", (int)tri.last_reason()); return 1; }
    const double d = std::sqrt(std::pow((*p)[0] / (*p)[3] - X[0], 2) + std::pow((*p)[1] / (*p)[3] - X[1], 2) +
                               std::pow((*p)[2] / (*p)[3] - X[2], 2));
    std::printf("doc-test distance %.3g\n", d);
    if (!(d < 1e-6)) return 1;
    // the same through triangulate_observations, bit for bit
    const cv_core::WorldToCamera ident{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
    const auto p2 = tri.triangulate_observations({{ident, a}, {cv_core::WorldToCamera{pose.rt}, b}});
    if (!p2 || *p2 != *p) return 1;
    // None: fewer than two observations; a point behind the second camera; a solver that may not iterate
    if (tri.triangulate_observations({{ident, a}}) || tri.last_reason() != RS_TRI_TOO_FEW) return 1;
    if (tri.triangulate_relative(pose, a, {-b[0], -b[1], -b[2]}) || tri.last_reason() != RS_TRI_CHEIRALITY) return 1;
    auto one = tri.max_iterations(1);
    if (one.triangulate_relative(pose, a, b) || one.last_reason() != RS_TRI_EIGEN) return 1;
    if (!tri.epsilon(1e-9).triangulate_relative(pose, a, b)) return 1;
    std::printf("none cases ok\n");
    std::printf("triangulate ok\n");
    return 0;
}
