// Device helpers of the per-landmark consensus, shared by the translation units that run it (fusion.hip: solve_kernel;
// report.hip: report_kernel, which repeats the solve with these functions in the same order and must land on the same bits).
#pragma once
#include "common.h"

namespace {

constexpr int MAX_VIEWS = 1024;

__device__ inline double wave_sum(double v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// Moore-Penrose inverse of a symmetric 3x3 applied to c, through a cyclic Jacobi
// eigen-decomposition; eigenvalues with |l| <= 1e-15 * max|l| are dropped, which is
// np.linalg.pinv's default cutoff on the singular values (utils3d.py:123).
__device__ void pinv3_apply(const double s_in[6], const double c[3], double p[3]) {
    double a[3][3] = {{s_in[0], s_in[3], s_in[4]}, {s_in[3], s_in[1], s_in[5]}, {s_in[4], s_in[5], s_in[2]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off == 0.0) break;
        for (int pi = 0; pi < 2; ++pi)
            for (int qi = pi + 1; qi < 3; ++qi) {
                const double apq = a[pi][qi];
                if (apq == 0.0) continue;
                // After a few sweeps an off-diagonal element that no longer registers beside BOTH of its diagonal elements
                // (|a_pp| + 100 |a_pq| == |a_pp| in double arithmetic) is set to zero instead of rotated (the classical cyclic
                // Jacobi termination): its rotation would move the eigenvalues by less than an ulp, and without this the
                // two-sided update never leaves an exact 0.0 behind, so every solve ran all 30 sweeps - 45 of the kernel's
                // 68 us, on one wavefront per landmark (round 5).
                if (sweep > 2) {
                    const double g = 100.0 * fabs(apq);
                    if (fabs(a[pi][pi]) + g == fabs(a[pi][pi]) && fabs(a[qi][qi]) + g == fabs(a[qi][qi])) {
                        a[pi][qi] = 0.0;
                        a[qi][pi] = 0.0;
                        continue;
                    }
                }
                const double theta = (a[qi][qi] - a[pi][pi]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) {  // columns p,q of A
                    const double akp = a[k][pi], akq = a[k][qi];
                    a[k][pi] = cs * akp - sn * akq;
                    a[k][qi] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; ++k) {  // rows p,q of A
                    const double apk = a[pi][k], aqk = a[qi][k];
                    a[pi][k] = cs * apk - sn * aqk;
                    a[qi][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][pi], vkq = v[k][qi];
                    v[k][pi] = cs * vkp - sn * vkq;
                    v[k][qi] = sn * vkp + cs * vkq;
                }
            }
    }
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    const double lmax = fmax(fabs(l0), fmax(fabs(l1), fabs(l2)));
    const double cutoff = 1e-15 * lmax;
    const double lam[3] = {l0, l1, l2};
    p[0] = p[1] = p[2] = 0.0;
    for (int e = 0; e < 3; ++e) {
        if (!(fabs(lam[e]) > cutoff)) continue;
        const double proj = (v[0][e] * c[0] + v[1][e] * c[1] + v[2][e] * c[2]) / lam[e];
        p[0] += v[0][e] * proj;
        p[1] += v[1][e] * proj;
        p[2] += v[2][e] * proj;
    }
}

struct Line {
    double ax, ay, az, bx, by, bz;
};

__device__ inline Line load_line(const double* s, const double* e, size_t i) {
    return {s[i * 3], s[i * 3 + 1], s[i * 3 + 2], e[i * 3], e[i * 3 + 1], e[i * 3 + 2]};
}

// accumulate one line's contribution to S (6 unique entries) and c (utils3d.py:101-120)
__device__ inline void lsq_accum(const Line& l, double acc[9]) {
    const double sx = l.bx - l.ax, sy = l.by - l.ay, sz = l.bz - l.az;
    const double len = sqrt(sx * sx + sy * sy + sz * sz);
    const double nx = sx / len, ny = sy / len, nz = sz / len;
    acc[0] += nx * nx - 1;
    acc[1] += ny * ny - 1;
    acc[2] += nz * nz - 1;
    acc[3] += nx * ny;
    acc[4] += nx * nz;
    acc[5] += ny * nz;
    acc[6] += l.ax * (nx * nx - 1) + l.ay * (nx * ny) + l.az * (nx * nz);
    acc[7] += l.ax * (nx * ny) + l.ay * (ny * ny - 1) + l.az * (ny * nz);
    acc[8] += l.ax * (nx * nz) + l.ay * (ny * nz) + l.az * (nz * nz - 1);
}

__device__ inline void lsq_solve(double acc[9], double p[3]) {
    for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
    pinv3_apply(acc, acc + 6, p);
}

// squared point-line distance (estimator3d.py:109-111)
__device__ inline double sq_dist(const Line& l, const double p[3]) {
    const double ux = p[0] - l.ax, uy = p[1] - l.ay, uz = p[2] - l.az;
    const double wx = p[0] - l.bx, wy = p[1] - l.by, wz = p[2] - l.bz;
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    const double bx = l.bx - l.ax, by = l.by - l.ay, bz = l.bz - l.az;
    const double r = sqrt(cx * cx + cy * cy + cz * cz) / sqrt(bx * bx + by * by + bz * bz);
    return r * r;
}

}  // namespace
