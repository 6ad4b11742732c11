// The surface distances on the host: mvlm_amd/csrc/geodesic_math.h - the header the kernels include - with a plain sweep round it
// (test infrastructure, tests/test_geodesic_cpu.py).  The sweep scatters over triangles where the kernels gather over a vertex's
// list; the rule's min is order-free, so the values must equal tests/geodesic_model.py's bit for bit.
// Built with g++ -O2 -ffp-contract=off.
#include <cstdint>
#include <vector>

#include "../../mvlm_amd/csrc/geodesic_math.h"

namespace {

gd_vec3 vert(const float* verts, int v) { return gd_v3(double(verts[3 * v]), double(verts[3 * v + 1]), double(verts[3 * v + 2])); }
gd_vec3 point(const double* p, int i) { return gd_v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

bool tri_valid(const float* verts, int V, const int32_t* tris, int t) {
    for (int e = 0; e < 3; ++e) {
        const int v = tris[3 * t + e];
        if (v < 0 || v >= V || !gd_finite3(vert(verts, v))) return false;
    }
    return true;
}

}  // namespace

// D, E f64[n,n], sweeps i32[n], fields f64[n,V] or null.  Returns 0, or 1 + the first source that did not settle within max_sweeps
// (the outputs are then unspecified).
extern "C" int geodesic_host(const float* verts, int V, const int32_t* tris, int T, const double* snapped, const int32_t* tri, int n,
                             int init_rings, int max_sweeps, double* D, double* E, int32_t* sweeps, double* fields) {
    const double nan = __builtin_nan("");
    std::vector<char> valid(T), ok(n);
    for (int t = 0; t < T; ++t) valid[t] = tri_valid(verts, V, tris, t);
    for (int i = 0; i < n; ++i) ok[i] = tri[i] >= 0 && tri[i] < T && valid[tri[i]] && gd_finite3(point(snapped, i));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) E[i * n + j] = gd_dist(point(snapped, i), point(snapped, j));
    std::vector<double> d(V), next(V);
    std::vector<char> in(V), in_next(V);
    for (int i = 0; i < n; ++i) {
        sweeps[i] = -1;
        for (int j = 0; j < n; ++j) D[i * n + j] = nan;
        if (fields)
            for (int v = 0; v < V; ++v) fields[size_t(i) * V + v] = nan;
        if (!ok[i]) continue;
        const gd_vec3 P = point(snapped, i);
        in.assign(V, 0);
        for (int e = 0; e < 3; ++e) in[tris[3 * tri[i] + e]] = 1;
        for (int r = 0; r < init_rings; ++r) {
            in_next = in;
            for (int t = 0; t < T; ++t)
                if (valid[t] && (in[tris[3 * t]] || in[tris[3 * t + 1]] || in[tris[3 * t + 2]]))
                    for (int e = 0; e < 3; ++e) in_next[tris[3 * t + e]] = 1;
            in.swap(in_next);
        }
        for (int v = 0; v < V; ++v) d[v] = in[v] ? gd_dist(vert(verts, v), P) : gd_inf();
        int k = 0;
        for (;; ++k) {
            if (k == max_sweeps) return 1 + i;
            next = d;
            for (int t = 0; t < T; ++t) {
                if (!valid[t]) continue;
                for (int e = 0; e < 3; ++e) {
                    const int c = tris[3 * t + e], a = tris[3 * t + (e + 1) % 3], b = tris[3 * t + (e + 2) % 3];
                    next[c] = gd_min(next[c], gd_update(d[a], d[b], gd_make_frame(vert(verts, a), vert(verts, b), vert(verts, c))));
                }
            }
            bool changed = false;
            for (int v = 0; v < V; ++v) changed = changed || next[v] != d[v];
            d.swap(next);
            if (!changed) break;
        }
        sweeps[i] = k;
        if (fields)
            for (int v = 0; v < V; ++v) fields[size_t(i) * V + v] = d[v];
        for (int j = 0; j < n; ++j) {
            if (!ok[j]) continue;
            if (i == j) {
                D[i * n + j] = 0.0;
                continue;
            }
            const gd_vec3 Q = point(snapped, j);
            double out = gd_inf();
            for (int e = 0; e < 3; ++e) {
                const int a = tris[3 * tri[j] + (e + 1) % 3], b = tris[3 * tri[j] + (e + 2) % 3];
                out = gd_min(out, gd_update(d[a], d[b], gd_make_frame(vert(verts, a), vert(verts, b), Q)));
            }
            if (tri[i] == tri[j]) out = gd_min(out, gd_dist(P, Q));
            D[i * n + j] = out;
        }
    }
    return 0;
}
