// The host-side mesh handle behind mvlm_obj_read / mvlm_mesh_read (include/mvlm_hip.h), shared by the readers.
#ifndef MVLM_MESH_OBJ_H
#define MVLM_MESH_OBJ_H
#include <cstdint>
#include <vector>

struct mvlm_obj {
    std::vector<float> verts;   // [V,3] corner-expanded (or the raw points for a point cloud)
    std::vector<float> uvs;     // [V,2] or empty
    std::vector<int32_t> tris;  // [T,3]
    int64_t n_positions = 0;
    std::vector<uint8_t> colors;  // [V,3] per-point r g b (PLY red green blue, VTK COLOR_SCALARS, OBJ "v x y z r g b") or empty
    std::vector<float> normals;   // [V,3] per-point normals as written (PLY nx ny nz, VTK POINT_DATA NORMALS) or empty
};

// A colour channel written as a float in [0,1] (ASCII .vtk COLOR_SCALARS, OBJ "v x y z r g b") -> its byte: clamped, rounded
// to nearest, so that c / 255 written with six decimals reads back as c.  NaN reads as 0.  (VTK's own readers convert with
// code of theirs that cannot be run here to compare; a file written from bytes round-trips under any sensible rule.)
inline uint8_t mvlm_color_byte(double f) {
    if (!(f > 0.0)) return 0;
    if (f >= 1.0) return 255;
    return uint8_t(int(255.0 * f + 0.5));
}
#endif
