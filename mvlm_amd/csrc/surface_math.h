// Device helpers of the surface snap, shared by the translation units that walk a triangle's Voronoi regions (surface.hip;
// surface_attach.hip, whose snapped point must be the snap's own, bit for bit).
#pragma once
#include "common.h"

namespace {

struct V3 {
    double x, y, z;
};
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 madd(V3 a, V3 d, double t) { return {a.x + t * d.x, a.y + t * d.y, a.z + t * d.z}; }

// closest point on triangle (a,b,c) to p: walk the Voronoi regions (vertex, edge, face)
__device__ V3 closest_on_triangle(V3 p, V3 a, V3 b, V3 c) {
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0 && d2 <= 0) return a;
    const V3 bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) return b;
    const double vc = d1 * d4 - d3 * d2;
    // (d1 - d3 = |ab|^2: a triangle with a == b is the segment ac - vtkCleanPolyData turns it into a line cell - and belongs
    //  to the edge-ac branch below, not to a 0 / 0 here)
    if (vc <= 0 && d1 >= 0 && d3 <= 0 && d1 > d3) return madd(a, ab, d1 / (d1 - d3));
    const V3 cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) return c;
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) return madd(a, ac, d2 / (d2 - d6));
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) return madd(b, sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6)));
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, w = vc * denom;
    return {a.x + ab.x * v + ac.x * w, a.y + ab.y * v + ac.y * w, a.z + ab.z * v + ac.z * w};
}

}  // namespace
