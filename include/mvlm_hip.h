/*
 * mvlm_hip.h - C ABI of libmvlm_hip.so: the MI355X (gfx950) implementation of the
 * cvjena/mvlm `Pipeline.predict_one_file` hot path.
 *
 * The reference is pure Python and has no FFI of its own; the interface each entry
 * point replaces is the Python method cited next to it (paths relative to the
 * reference's src/mvlm/).  INTEGRATION.md shows the ctypes binding a maintainer
 * adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from mvlm_last_error(ctx) - the CALLING THREAD's last failure on that
 *     ctx, valid until that thread's next failing call.  Nothing throws across the boundary.
 *   - "_dev" pointers are device (HBM) addresses owned by the caller (e.g. a torch
 *     tensor's data_ptr()); "_host" pointers are ordinary host memory.  The library
 *     never frees caller memory.
 *   - all work is enqueued on the ctx's HIP stream (mvlm_set_stream; default: the
 *     null stream).  Functions that return host results synchronise that stream.
 *   - a ctx serialises its callers with an internal mutex (the reference server
 *     calls predict_one_file from a thread pool without locks, 3DMD_server.py:26-31);
 *     one C call is atomic, a SEQUENCE of calls that shares buffers is the caller's to
 *     order (the Python Pipeline holds a lock of its own around a whole scan).
 *     The mvlm_mesh_upload* / mvlm_texture_* / mvlm_jpeg_decode calls may run on other threads
 *     beside the launching one: their host work and their device work (a copy / decode stream
 *     of the context's own) happen outside the ctx mutex, under an upload mutex of their own.
 *     mvlm_obj_read / mvlm_mesh_read / mvlm_jpeg_info need no ctx at all
 *     (mvlm_obj_read parses on up to 16 threads of its own - the host's cores divided by the number of
 *     mvlm_obj_read calls in flight; MVLM_OBJ_THREADS overrides).
 */
#ifndef MVLM_HIP_H
#define MVLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvlm_ctx mvlm_ctx;
typedef struct mvlm_mesh mvlm_mesh;
typedef struct mvlm_texture mvlm_texture;

#define MVLM_IMAGE_SIZE 256          /* render3d.py / general_pipeline.py:57 */
#define MVLM_CONV_DESC_INTS 12       /* ints per conv slot, see mvlm_amd/weights.py */

enum { MVLM_MODE_QUANTILE = 0, MVLM_MODE_ABSOLUTE = 1 };   /* estimator3d.py:166-171 */
enum { MVLM_MAXIMA_SIMPLE = 0, MVLM_MAXIMA_MOMENT = 1 };   /* paulsenpredictor.py:121,129 */

/* ---- context ------------------------------------------------------------------ */
int mvlm_ctx_create(int device, mvlm_ctx** out);
void mvlm_ctx_destroy(mvlm_ctx* ctx);
const char* mvlm_last_error(mvlm_ctx* ctx);
/* the stream the context's next calls enqueue on (default: the null stream).  A context reuses device scratch from call to
 * call; when the stream CHANGES, the new stream is made to wait for what the context enqueued on the previous one, so two
 * users of one context under different streams stay ordered. */
int mvlm_set_stream(mvlm_ctx* ctx, void* hip_stream);
int mvlm_synchronize(mvlm_ctx* ctx);
/* name of the GPU architecture the library was built for ("gfx950") */
const char* mvlm_build_arch(void);

/* ---- OBJ ingest on the host (replaces utils3d.py:16-24, vtkOBJReader) ------------ */
/* Parses a Wavefront OBJ into float32 points, one texture coordinate per point (a point is
 * duplicated when it is used with several `vt` indices), polygons as triangle fans; `.mtl`,
 * normals and groups are ignored.  Needs no ctx and no GPU.  Errors mirror the reference's
 * ValueErrors: missing file (utils3d.py:13-14), no points (:20-21). */
typedef struct mvlm_obj mvlm_obj;
enum { MVLM_OBJ_ERR_ARGS = 1, MVLM_OBJ_ERR_FILE = 2, MVLM_OBJ_ERR_EMPTY = 3, MVLM_OBJ_ERR_INDEX = 4,
       MVLM_OBJ_ERR_SYNTAX = 5 };
int mvlm_obj_read(const char* path, mvlm_obj** out, char* err, int err_len);
int mvlm_obj_info(const mvlm_obj* obj, int64_t* n_verts, int64_t* n_tris, int* has_uvs);
/* copies into caller arrays sized from mvlm_obj_info: verts f32[V,3], uvs f32[V,2] (may be NULL),
 * tris i32[T,3] */
int mvlm_obj_copy(const mvlm_obj* obj, float* verts, float* uvs, int32_t* tris);
/* per-point colours, where the file carries them (.ply uchar red green blue / diffuse_*, .vtk POINT_DATA COLOR_SCALARS with 3
 * or 4 components, .obj "v x y z r g b" on every v line): *has = 1, and rgb u8[V,3] receives them (a duplicated point keeps
 * its colour).  mvlm_obj_copy_colors on a mesh without colours returns MVLM_OBJ_ERR_EMPTY. */
int mvlm_obj_has_colors(const mvlm_obj* obj, int* has);
int mvlm_obj_copy_colors(const mvlm_obj* obj, uint8_t* rgb);
/* per-point normals, where the file carries them (.ply float / double nx ny nz, all three; legacy .vtk POINT_DATA NORMALS):
 * *has = 1, and normals f32[V,3] receives them as written (not normalised).  A count other than the points' means none; OBJ
 * "vn" lines are not read.  mvlm_obj_copy_normals on a mesh without normals returns MVLM_OBJ_ERR_EMPTY. */
int mvlm_obj_has_normals(const mvlm_obj* obj, int* has);
int mvlm_obj_copy_normals(const mvlm_obj* obj, float* normals);
void mvlm_obj_free(mvlm_obj* obj);
/* The reference's legacy multi-format reader (Utils3D.multi_read_surface, utils3d.py:389-423) by file extension:
 * .obj (as above), .ply (ASCII / binary), .stl (ASCII / binary, coincident points merged like vtkSTLReader),
 * .vtk (legacy POLYDATA, ASCII / BINARY), .wrl (VRML 2.0 IndexedFaceSet, the last one of the file).  Fills the
 * same handle; texture coordinates are kept where the format carries them per point / corner. */
int mvlm_mesh_read(const char* path, mvlm_obj** out, char* err, int err_len);

/* ---- mesh (replaces utils3d.py:10-85 obj_to_actor's upload half) ---------------- */
/* verts f32[V,3], uvs f32[V,2] or NULL, tris i32[T,3], tex u8[H,W,3] (row 0 = top of
 * the image file) or NULL (=> pure white mesh, utils3d.py:58-64).  Host pointers;
 * the data is copied into pinned staging before the call returns (the host arrays are
 * the caller's again) and travels to the device asynchronously on a copy stream of
 * the context's own; mvlm_render / mvlm_project_to_surface / mvlm_clip_rays_to_mesh
 * wait for it on their stream.  May be called from another thread than the one that
 * launches work (a reader thread uploading the next scan). */
int mvlm_mesh_upload(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                     const int32_t* tris_host, int n_tris, const uint8_t* tex_host, int tex_h, int tex_w,
                     mvlm_mesh** out);
/* Per-vertex colours, rgb_host u8[V,3], for a mesh made by any mvlm_mesh_upload* entry (n_verts must be the mesh's count).
 * They shade the RGB planes when the render's shading is 0 (unlit) and the mesh has NO usable texture (no uvs or no texture
 * image): per channel the plane through vertex 0 of c / 255, clamped to [0,1], then converted through 16-bit fixed point like
 * the OpenGL the contract is pinned to (rm_color_u8, DESIGN.md 5.1: round-to-nearest but for values within 1/512 of k + 1/2).
 * A mesh with a texture and uvs renders with its texture alone (VTK would multiply texel and colour: not built); geometry shading and the
 * depth plane never see colours.  Same staging, copy stream and ready event as the mesh upload; may run on a reader thread. */
int mvlm_mesh_upload_colors(mvlm_ctx* ctx, mvlm_mesh* mesh, const uint8_t* rgb_host, int n_verts);
/* ---- point clouds: a scan with points and no faces ---------------------------------
 * mvlm_mesh_upload with n_tris == 0 (tris_host may be NULL) makes a POINT MESH; uvs and texture arguments are ignored, and the
 * JPEG / texture upload entries refuse n_tris == 0.  mvlm_mesh_upload_colors works as for any mesh.  The reference has no
 * such path (vtkOBJReader yields no cells: white views, nothing to snap to), so the contract is this build's own
 * (csrc/raster_points_math.h, DESIGN.md 5.1 "Point clouds"):
 *   - mvlm_render draws every point as a SPLAT: position and depth from the mesh path's transform, a disc of R =
 *     floor(r * 256 / 300 * 256 + 0.5) steps of 1/256 pixel that covers the pixel centres with dx^2 + dy^2 <= R^2, a depth that
 *     rises towards the rim, z_pix = z + (float)d2 * c with c = (float)(r / 1500 / R^2) - so neighbouring splats share the
 *     screen like a Voronoi diagram - clipped to [0,1]; the least z_pix wins a pixel, the higher point id on ties; RGB is
 *     the winner's colour (white without colours), the depth plane its z_pix.  A non-finite point draws nothing.
 *   - mvlm_project_to_surface returns the NEAREST POINT's own coordinates (float64 distances, lowest id on ties, non-finite
 *     points never, a non-finite landmark passed through).
 *   - refused with an argument error before anything is launched: mvlm_render with shading 1 (geometry) or 4 multisamples,
 *     mvlm_render_landmark_view, mvlm_render_ray_view, mvlm_clip_rays_to_mesh, mvlm_surface_attach.  These refusals stand for
 *     every point mesh; the way round them is to give the cloud triangles first (mvlm_mesh_triangulate_points, below) and to
 *     upload the result as an ordinary mesh.
 * The radius r (model units) is per mesh: at upload the automatic one, mvlm_points_auto_radius of the uploaded points;
 * mvlm_mesh_set_point_radius replaces it - an error outside 0.75..8 pixels (0.87890625..9.375 model units) or on a mesh with
 * triangles; mvlm_mesh_point_radius reads it (non-zero for a mesh with triangles). */
int mvlm_mesh_set_point_radius(mvlm_ctx* ctx, mvlm_mesh* mesh, double r_model_units);
int mvlm_mesh_point_radius(const mvlm_mesh* mesh, double* r_model_units);
/* The automatic radius; host only, no ctx, no GPU.  verts f32[n,3].  Bounding box of the points whose three coordinates are
 * finite, extents sorted ex >= ey >= ez, s = sqrt(ex * ey / n_finite), r = clamp(1.25 s, 0.75, 8.0) * 300 / 256: a regular grid
 * of spacing s leaves no pixel centre farther than 0.71 s from a point and rotation only shrinks projected spacing; a dense
 * scan lands on the 0.75 pixel floor, as does a cloud with s = 0 (one point, collinear points, no finite point). */
int mvlm_points_auto_radius(const float* verts_host, int n, double* r_model_units);
/* measuring hooks: the splat kernel's counting form, and what the last counted render saw (pixels past coverage and clip;
 * atomics issued - the others found a smaller key stored already).  mvlm_points_get_stats synchronises the stream. */
int mvlm_points_set_counting(mvlm_ctx* ctx, int enabled);
int mvlm_points_get_stats(mvlm_ctx* ctx, unsigned long long* covered, unsigned long long* issued);
/* ms2[0], ms2[1]: milliseconds of the splat and of the tile kernel of the last cloud render made while
 * mvlm_render_set_profiling was on; synchronises the stream. */
int mvlm_points_stage_ms(mvlm_ctx* ctx, float* ms2);
/* ---- normals of a point cloud: geometry shading of its splats (csrc/cloud_normals_math.h, DESIGN.md 5.1 "Point clouds") ----
 * A cloud that HAS normals renders under shading 1: the splat kernel runs unchanged, then a tile kernel of its own writes
 * shade / 255 into planes 0..2, shade = (int)(|nz| / len * 255 + 0.5) in float64 with nz = (M[6] n.x + M[7] n.y) + M[8] n.z and
 * len = sqrt((n.x n.x + n.y n.y) + n.z n.z) of the winner's float32 normal n - two-sided, so the sign of n does not matter; 0
 * where len is zero or not finite; colours are ignored, the depth plane and the background are the texture mode's.  A cloud
 * WITHOUT normals is still refused under shading 1, as are multisampled clouds.
 *   mvlm_mesh_upload_normals  normals_host f32[V,3] (a file's nx ny nz; any length) become the cloud's normals; an error on a
 *                             mesh with triangles or for another count.  Staging, copy stream and ready event of the mesh upload.
 *   mvlm_mesh_estimate_normals  estimates them on the device and attaches them: per finite point the K = 16 finite points of
 *                             least (d2, id), itself included, d2 = (dx dx + dy dy) + dz dz in float64; centroid and 3x3
 *                             covariance in float64, summed in that order; the unit eigenvector of the least eigenvalue (cyclic
 *                             Jacobi, float64), stored as float32, sign unspecified; (0,0,0) for a non-finite point, fewer than 3
 *                             neighbours or a zero covariance.  neighbors_dev: NULL, or i32[V,16] on the device that receives
 *                             each row in ascending (d2, id), unused slots -1, a non-finite point's row all -1.  The result does
 *                             not depend on the order in which threads or atomics land.  Only enqueues work.
 *   mvlm_mesh_copy_normals    the device copy's normals -> host f32[V,3]; waits for the stream; an error without normals.
 *   mvlm_normals_stage_ms     ms3: grid build, search, solve of the last estimate made while mvlm_render_set_profiling was on.
 *   mvlm_normals_get_stats    measuring hook: with mvlm_points_set_counting on, an estimate runs the search kernel's counting form;
 *                             stats3 receives what the last such estimate summed over all points: shells walked, candidates
 *                             tested, candidates that entered a list.  Waits for the stream. */
int mvlm_mesh_upload_normals(mvlm_ctx* ctx, mvlm_mesh* mesh, const float* normals_host, int n_verts);
int mvlm_mesh_estimate_normals(mvlm_ctx* ctx, mvlm_mesh* mesh, int32_t* neighbors_dev);
int mvlm_mesh_copy_normals(mvlm_ctx* ctx, const mvlm_mesh* mesh, float* normals_host);
int mvlm_normals_stage_ms(mvlm_ctx* ctx, float* ms3);
int mvlm_normals_get_stats(mvlm_ctx* ctx, unsigned long long* stats3);
/* ---- a triangle surface for a point cloud (csrc/cloud_mesh_math.h, DESIGN.md 5.1 "Point clouds") -------------------------------
 * The refusals above stand for every cloud.  The way round them is to give the cloud triangles: mvlm_mesh_triangulate_points
 * computes, on the device, a triangle list over the cloud's points, which the caller uploads as an ordinary mesh (the same points,
 * these triangles) - and that mesh has everything a mesh has (HipRenderer3D.triangulate_point_cloud, Pipeline(point_surface="mesh")).
 *   mvlm_mesh_triangulate_points  cloud: a point mesh WITH normals (mvlm_mesh_upload_normals or mvlm_mesh_estimate_normals);
 *                             neighbors_dev i32[V,16]: the table mvlm_mesh_estimate_normals left for THIS cloud.  All in float64:
 *                             every point is shifted by 1/256 of its nearest-neighbour distance in a direction hashed from its id
 *                             (exact ties of a regular grid break the same way everywhere); the star of a point p is the set of
 *                             pairs {a, b} of its neighbours that are a hull edge of the neighbours' tangent-plane positions
 *                             inverted about p (w = q / |q|^2: "empty circle through p" becomes "hull edge"), at most 16; the triangle
 *                             {i < j < k} is emitted iff {j,k} is in i's star, {i,k} in j's, {i,j} in k's and, on the unshifted
 *                             points, |cross|^2 * 1024 > (longest edge^2)^2 (height above 1/32 of the longest edge).  Rows (i, j, k)
 *                             ascending, the winding unspecified, no row touches a non-finite point; the sign of a normal does not
 *                             matter and the bytes are the same from run to run (no atomics).  n_tris_dev i32[1] always receives
 *                             the full count; tris_dev i32[cap,3] receives the rows below cap, none beyond; tris_dev == NULL only
 *                             counts.  Only enqueues work; leaves the cloud's device copy and the render's key plane as they were.
 *                             A mesh with triangles, a cloud without normals, NULL neighbors_dev or n_tris_dev, a negative cap or
 *                             more than 67108864 points set an error that starts with "triangulate points:" and launch nothing.
 *                             Meant for scanner-like sampling (a depth camera's grid, a structured-light scan), not a general
 *                             surface reconstruction: where 16 neighbours do not surround a point, its star has gaps.
 *   mvlm_cloud_mesh_stage_ms  ms3: star (with the shift), count + scan, emit of the last triangulation made while
 *                             mvlm_render_set_profiling was on; waits for the stream. */
int mvlm_mesh_triangulate_points(mvlm_ctx* ctx, const mvlm_mesh* cloud, const int32_t* neighbors_dev, int32_t* tris_dev, long long cap,
                                 int32_t* n_tris_dev);
int mvlm_cloud_mesh_stage_ms(mvlm_ctx* ctx, float* ms3);
void mvlm_mesh_free(mvlm_ctx* ctx, mvlm_mesh* mesh);

/* ---- JPEG texture decoded on the device (replaces vtkJPEGReader in obj_to_actor, utils3d.py:28-34 / :42-48, and in
 * multi_read_surface's texture lookup, utils3d.py:457-462; the decoder behind vtkJPEGReader is libjpeg-turbo with its
 * defaults - JDCT_ISLOW, fancy upsampling, RGB out - and the bytes produced here are libjpeg's) ---------------------
 * Taken: baseline / extended sequential Huffman JPEG (SOF0 / SOF1), 8 bit, one interleaved scan, grey or YCbCr with
 * 1x1 / 2x1 / 2x2 luma sampling over 1x1 chroma, restart intervals.  Return code 2 = "not taken" (progressive,
 * arithmetic, CMYK, 12 bit, other sampling, corrupt entropy-coded data; mvlm_last_error / why says which): the caller
 * decodes such a file with libjpeg on the host and uploads the pixels with mvlm_mesh_upload. */
/* header only, no GPU, no ctx: 0 and the size if the device decoder takes this stream, 2 and the reason in why if not */
int mvlm_jpeg_info(const uint8_t* jpeg_host, size_t n_bytes, int* width, int* height, int* components, char* why, int why_len);
/* mvlm_mesh_upload with the texture given as the JPEG file's bytes: headers are parsed and byte stuffing is removed on the
 * host (into pinned staging), entropy decoding, inverse DCT, chroma upsampling and colour conversion run on the context's
 * upload stream.  The calling thread waits for that stream (not for the launch stream) before it returns. */
int mvlm_mesh_upload_jpeg(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                          const int32_t* tris_host, int n_tris, const uint8_t* jpeg_host, size_t jpeg_bytes,
                          mvlm_mesh** out);
/* The texture decoded AHEAD of its mesh, so that one thread can decode (GPU work + this thread waiting for it) while another
 * still parses the geometry (obj_to_actor does both in sequence, utils3d.py:16-34): the pixels go into a device buffer of
 * the context's mesh pool.  The handle is consumed by a successful mvlm_mesh_upload_texture that uses it (*consumed = 1; a
 * mesh without texture coordinates does not use a texture, utils3d.py:26) and must be given back with mvlm_texture_free
 * otherwise.  Return codes as mvlm_mesh_upload_jpeg (2 = not taken: decode on the host). */
int mvlm_texture_from_jpeg(mvlm_ctx* ctx, const uint8_t* jpeg_host, size_t jpeg_bytes, mvlm_texture** out);
int mvlm_texture_size(const mvlm_texture* tex, int* height, int* width);
void mvlm_texture_free(mvlm_ctx* ctx, mvlm_texture* tex);
int mvlm_mesh_upload_texture(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                             const int32_t* tris_host, int n_tris, mvlm_texture* tex, int* consumed, mvlm_mesh** out);
/* the decoder alone: rgb_dev u8[H,W,3] (sizes from mvlm_jpeg_info) is complete when the call returns; rounds_out (may be
 * NULL): how many synchronisation rounds the parallel entropy decoder needed */
int mvlm_jpeg_decode(mvlm_ctx* ctx, const uint8_t* jpeg_host, size_t jpeg_bytes, uint8_t* rgb_dev, int* rounds_out);

/* ---- render (replaces render3d.py:114-177 + :191, all poses in one launch set) --- */
/* rot_host f64[N,9]: row-major M = Ry*Rx*Rz per view (render3d.py:140-144).
 * out_dev f32[N,256,256,4]: RGB + depth planes in [0,1], already flipped to
 * image orientation (render3d.py:177) and divided by 255 (:191). */
int mvlm_render(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, float* out_dev);
/* The device copy of the last render's rotations, f64[n_views,9] (the context's scratch: valid until the next mvlm_render):
 * mvlm_estimate_lines of the same views takes it as rot_dev, and the table crosses PCIe once per mesh. */
int mvlm_render_rotations_dev(mvlm_ctx* ctx, const double** rot_dev);
/* what the RGB planes hold: 0 = unlit white x nearest texel, exactly what the reference renders
 * (utils3d.py:58-64); 1 = build-defined "geometry" shading (flat two-sided head light, grey in all
 * three planes) for models trained on geometry renderings - the reference's renderer has no such
 * mode, parity unpinned. */
int mvlm_set_render_shading(mvlm_ctx* ctx, int shading);
/* The one rasterisation parameter OpenGL leaves to the implementation that is a NUMBER: vertices snap to 2^-bits pixel
 * (GL_SUBPIXEL_BITS; the reference's images depend on the OpenGL its VTK runs on, render3d.py:60-65).  8 (default) = what
 * GPUs report; 4 = the standard's minimum and the software OpenGL tests/golden/gl_raster.npz was drawn with.  4..8. */
int mvlm_set_render_subpixel_bits(mvlm_ctx* ctx, int bits);
/* The other rasterisation choice OpenGL leaves open: multisampling (vtkRenderWindow.MultiSamples, which the reference never
 * sets, render3d.py:60-65, so its views follow the installed VTK's default).  0 (default) = one sample at the pixel centre, the
 * contract every other test pins; 4 = four samples per pixel at the rotated-grid positions (3,6) (13,10) (6,13) (10,3) in
 * 1/16 pixel from the lower-left corner, coverage and depth per sample, the colour evaluated once per pixel at its centre and
 * resolved by pairwise rounding-up averages per byte, the depth byte from sample 0 - what the OpenGL behind
 * tests/golden/gl_raster_msaa4.npz does.  Any other value is an error. */
int mvlm_set_render_multisamples(mvlm_ctx* ctx, int samples);
/* HIP-event timing of the render kernels (bench.py's rasteriser roofline): while enabled every mvlm_render
 * records one {n_views, n_verts, n_tris, ms}; get_profile waits for the stream, fills up to `cap` records,
 * clears them and returns the count (-1 on failure). */
int mvlm_render_set_profiling(mvlm_ctx* ctx, int enabled);
int mvlm_render_get_profile(mvlm_ctx* ctx, int32_t* n_views, int32_t* n_verts, int32_t* n_tris, float* ms, int cap);
/* mvlm_render only enqueues work; this waits for the stream and reports a deferred failure
 * (tile lists overflowed) of the renders since the last check */
int mvlm_render_check(mvlm_ctx* ctx);

/* ---- landmark view (replaces utils/viewer.py's offscreen window: VTKViewer(..., save=True), main.py:66-67) ---- */
/* The mesh with a shaded sphere at every landmark, in a window of `size` x `size` pixels (a multiple of 16, 64..2048;
 * n_views <= 128 and n_views * size * size <= 8 * 2048 * 2048 per call: 8 views at 2048, 32 at 1024, 128 up to 512) - a rasteriser object of its own beside mvlm_render, whose kernels,
 * scratch and key planes it does not touch ("Landmark view"; build-defined, the viewer's arithmetic lives in VTK).
 *   rot_host f64[n_views,9]     M = Ry*Rx*Rz per view, as mvlm_render takes them
 *   frame_host f32[n_views,3]   cx, cy, half: the view-space point at the window's centre and the model units from the centre to
 *                               the border (0, 0, 150 = the window the network sees)
 *   landmarks_host f64[n_lm,3]  in the mesh's coordinates (NULL allowed when n_lm == 0); radius: the spheres', in model units
 *   lm_rgb_host u8[n_lm,3]      a colour per landmark, NULL = blue (viewer.py:71)
 *   out_dev u8[n_views,size,size,4]  RGBA, alpha 255, top row first
 *   lm_pixels_dev i32[n_views,n_lm] or NULL: the pixels each landmark's sphere won in each view (0 = hidden there)
 * The mesh is drawn by mvlm_render's one-sample contract with the window generalised, under the context's shading and
 * sub-pixel-bits settings: at size 256 with the frame (0, 0, 150) and no landmarks the RGB bytes are 255 x mvlm_render's RGB
 * planes.  It draws ONE sample per pixel: mvlm_set_render_multisamples does not apply to it.  The spheres are analytic under the
 * orthographic camera, shaded by a head light (colour x height / radius), depth-tested against the mesh (they win ties; among
 * spheres the nearer wins, the higher index on equal depth).
 * A size or view count outside the range, a non-finite frame or half <= 0, a negative or non-finite radius, a non-finite landmark return an
 * error and launch nothing.  Only enqueues work on the launch stream; a tile-list overflow is reported by mvlm_render_check. */
int mvlm_render_landmark_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                              const float* frame_host /* [n_views,3]: cx, cy, half */,
                              const double* landmarks_host /* [n_lm,3], may be NULL when n_lm == 0 */, int n_lm,
                              float radius, const uint8_t* lm_rgb_host /* [n_lm,3] or NULL = blue */,
                              uint8_t* out_dev /* [n_views,size,size,4] */, int32_t* lm_pixels_dev /* [n_views,n_lm] or NULL */);
/* With mvlm_render_set_profiling on, the last landmark view's stages in milliseconds (HIP events), f32[7]: the copies and fills in
 * front of the kernels (the key plane, 8 bytes per pixel, is filled in every call), transform, classify, scan, bin fill, landmark
 * projection, tile.  Waits for the stream. */
int mvlm_landmark_view_stage_ms(mvlm_ctx* ctx, float* ms7);
/* mvlm_render_landmark_view with a colour per vertex given by the caller: vert_rgba_dev u8[n_verts,4] on the device, 4-byte aligned,
 * r g b and a fourth byte that is not read (mvlm_surface_heat writes this layout).  The same checks and the same launch set; the
 * tile kernel shades with those colours, no texture and shading 0.  Contract: byte for byte mvlm_render_landmark_view of the same
 * geometry uploaded with those colours as its vertex colours and no texture, under shading 0.  A NULL or misaligned vert_rgba_dev
 * returns an error and launches nothing. */
int mvlm_render_landmark_view_colored(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                                      const float* frame_host, const double* landmarks_host, int n_lm, float radius,
                                      const uint8_t* lm_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev,
                                      const uint8_t* vert_rgba_dev /* [n_verts,4] */);

/* ---- ray view (replaces visualization/ray_visualizer.py's RayVisualizer for the offscreen case) ---- */
/* mvlm_render_landmark_view's picture with n_rays rays between the mesh and the spheres: each an opaque, head-lit capsule, the
 * points within ray_radius model units of the segment start -> end ("Ray view").  Every argument shared with
 * mvlm_render_landmark_view means the same and is checked the same.
 *   starts_dev, ends_dev f64[n_rays,3]  ON THE DEVICE, in the mesh's coordinates (mvlm_estimate_lines' starts / ends, clipped or
 *                               not); NULL allowed when n_rays == 0; at most 65 536 rays and n_views * n_rays <= 1 048 576
 *                               per call (a 64-byte record per view and ray in the context's grow-only scratch: at most 64 MB).  A ray with a non-finite
 *                               coordinate is skipped: it covers no pixel and raises no error
 *   ray_rgb_host u8[n_rays,3]   a colour per ray, NULL = (26, 230, 26), the reference's (0.1, 0.9, 0.1)
 *   ray_pixels_dev i32[n_views,n_rays] or NULL: the pixels each ray won in each view
 * Order: the mesh, then the rays (a ray wins an equal depth against the mesh; among rays the nearer wins, the higher index on
 * equal depth), then the spheres (a sphere wins an equal depth against a ray).  A ray seen end-on, or projected shorter than
 * 1 / 256 of its radius in pixels, is the sphere of its nearer end, bit for bit.  With n_rays == 0 the output is
 * mvlm_render_landmark_view's, byte for byte.  A negative or non-finite ray_radius, n_rays outside 0..65536, n_views * n_rays beyond 1 048 576, NULL starts or ends
 * with n_rays > 0 set an error that starts with "ray view:" and launch nothing.  Only enqueues work; a tile-list overflow is
 * reported by mvlm_render_check. */
int mvlm_render_ray_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                         const float* frame_host, const double* landmarks_host, int n_lm, float radius, const uint8_t* lm_rgb_host,
                         const double* starts_dev, const double* ends_dev, int n_rays /* f64[n_rays,3], device */,
                         float ray_radius, const uint8_t* ray_rgb_host /* [n_rays,3] or NULL = (26,230,26) */,
                         uint8_t* out_dev, int32_t* lm_pixels_dev, int32_t* ray_pixels_dev /* [n_views,n_rays] or NULL */);
/* With mvlm_render_set_profiling on, the last ray view's stages in milliseconds, f32[8]: mvlm_landmark_view_stage_ms's first six
 * (copies and fills, transform, classify, scan, bin fill, landmark projection), the ray projection, the tile kernel. */
int mvlm_ray_view_stage_ms(mvlm_ctx* ctx, float* ms8);

/* ---- view sheet (replaces Predictor2D.draw_image_with_landmarks, prediction/predictor2d.py:29-53, for all views at once) ---- */
/* The layout of a sheet of n_views views ("View sheet"): cols columns (cols_in, or ceil(sqrt(n_views)) when
 * cols_in is 0), rows = ceil(n_views / cols), view v in cell (v / cols, v % cols), a cell 256 * scale pixels a side, gap pixels
 * between cells and around the sheet: width = cols * 256 * scale + (cols + 1) * gap, height likewise with rows.  Host only: no
 * context, no GPU.  0, or non-zero with the reason in why (may be NULL): n_views < 1, cols_in < 0, scale outside 1..4, gap outside
 * 0..16, or a width or height above 4096 (mvlm_png_encode's limit) - that message names the largest scale that fits. */
int mvlm_view_sheet_layout(int n_views, int cols_in, int scale, int gap, int* cols, int* rows, int* width, int* height, char* why,
                           int why_len);
/* The sheet: every view of the stack in its cell, each sheet pixel (x, y) of a cell showing view pixel (y / scale, x / scale) - planes
 * 0..2 as bytes (background 0) or plane 3 as a grey (background 1), a byte being (int)(p * 255 + 0.5) in float32 - gaps and cells
 * beyond n_views grey (128, 128, 128), then per (view, landmark) the residual and the marker:
 *   images_dev f32[n_views,256,256,4]  mvlm_render's stack, on the device
 *   maxima_dev f32[n_lm,n_views,3]     (a, b, score) as mvlm_cnn_maxima leaves them, on the device; NULL: the views alone.  The
 *                               marker stands at X = b, Y = a + 1 view pixels from the cell's left and top edge - where the
 *                               prediction's ray pierces the image - and covers the sheet pixels whose centre (i + 0.5, j + 0.5)
 *                               has dx^2 + dy^2 <= (marker_radius * scale)^2, dx = (i + 0.5) - scale * X; a non-finite a, b or
 *                               score draws nothing
 *   rot_host f64[n_views,9], landmarks_host f64[n_lm,3]  both or neither (NULL): the consensus landmarks in the space the mesh
 *                               was uploaded in.  q = M p, X' = (q.x + 150) * 256 / 300, Y' = 256 - (q.y + 150) * 256 / 300; the
 *                               segment marker -> (X', Y') is drawn red, max(0.5, scale / 2) sheet pixels to either side; a
 *                               non-finite landmark draws no segment
 *   lm_rgb_host u8[n_lm,3]      a colour per landmark, NULL = blue (0, 0, 255)
 *   used_host u8[n_lm,n_views]  0: the marker is a ring, the outer max(1, scale) sheet pixels of its disc; NULL = all used
 *   marker_radius               in view pixels, finite, 0.5..16
 *   out_dev u8[height,width,4]  RGBA, alpha 255, top row first (mvlm_view_sheet_layout gives the extents)
 * Order: background, residuals, markers; in landmark order within each, the later one wins.  Markers and residuals are clipped to
 * their cell.  All of it in float64, in the operation order of csrc/view_sheet_math.h.  A bad layout, background, radius, n_lm outside
 * 0..65536, a non-finite rotation or a NULL images_dev / out_dev set an error that starts with "view sheet:" and launch nothing.
 * Only enqueues work on the launch stream. */
int mvlm_render_view_sheet(mvlm_ctx* ctx, const float* images_dev, int n_views, const float* maxima_dev, int n_lm,
                           const double* rot_host, const double* landmarks_host, const uint8_t* lm_rgb_host, const uint8_t* used_host,
                           int background, int cols_in, int scale, int gap, double marker_radius, uint8_t* out_dev);

/* ---- heat sheet (the view sheet's cells with the network's heatmaps laid over them; DESIGN.md 5.1, "Heat sheet") ---- */
/* The peak of each of n_planes heatmap planes of 256 x 256 floats: its largest finite value, -inf when it has none (NaN and +-inf
 * are not counted, so the value does not depend on the order of the reduction; +0 counts as larger than -0).
 *   heat_dev  f32[n_planes,256,256]  on the device, 16-byte aligned
 *   peaks_dev f32[n_planes]          on the device
 * n_planes 1..32768.  A value out of range, a NULL or misaligned pointer set an error that starts with "heat sheet:" and launch
 * nothing.  Only enqueues work on the launch stream. */
int mvlm_heat_plane_peaks(mvlm_ctx* ctx, const float* heat_dev, int n_planes, float* peaks_dev);
/* The sheet of mvlm_render_view_sheet(..., maxima_dev = NULL, ...) - the views alone, by the same code: cells, gaps, background
 * bytes - and over it, per view pixel (v, y, x) - heat pixel [row, col] lies over image pixel [row, col] - the heatmaps:
 *   images_dev f32[n_views,256,256,4]    mvlm_render's stack, on the device
 *   heat_dev   f32[n_views,n_lm,256,256] as mvlm_cnn_heatmaps leaves them, on the device, 16-byte aligned
 *   sel_host    u8[n_lm]                 0: the landmark is left out; NULL = all
 *   lm_rgb_host u8[n_lm,3]               a colour per landmark; NULL = red (255, 0, 0)
 *   floor, opacity                       finite, floor in [0, 1), opacity in (0, 1]
 *   out_dev u8[height,width,4]           RGBA, alpha 255, top row first (mvlm_view_sheet_layout gives the extents)
 * With m = the peak of plane (v, l) as mvlm_heat_plane_peaks gives it and h = heat[v, l, y, x]: among the selected landmarks in
 * ascending order, those with m finite and > 0 and h finite are candidates with t = (double)h / (double)m; the largest t wins, the
 * lowest index on equal t.  Without a candidate, or with the winner's t <= floor, the pixel stays as the background left it.
 * Otherwise a = opacity * (t - floor) / (1.0 - floor) and per channel out = (int)(bg + a * ((double)col - bg) + 0.5), bg the
 * background's byte and col the winner's colour byte as doubles; all scale x scale sheet pixels of the view pixel get the result.
 * All of it in float64, in the operation order of csrc/heat_sheet_math.h.  No markers are drawn (the view sheet places its
 * markers at X = b, Y = a + 1 in ray coordinates, another rule than this overlay's; the two never meet in one picture).
 * n_lm 1..65536 and n_views * n_lm <= 32768 planes (8 GiB of heatmaps) per call; the layout is checked as
 * mvlm_view_sheet_layout checks it and refused in its words.  A bad layout, background, floor, opacity, n_lm, plane count, a
 * NULL images_dev / heat_dev / out_dev or a misaligned heat_dev set an error that starts with "heat sheet:" and launch nothing.
 * Only enqueues work on the launch stream. */
int mvlm_render_heat_sheet(mvlm_ctx* ctx, const float* images_dev, const float* heat_dev, int n_views, int n_lm,
                           const uint8_t* sel_host /* u8[n_lm], NULL = all */, const uint8_t* lm_rgb_host /* u8[n_lm,3], NULL = (255,0,0) */,
                           int background, int cols_in, int scale, int gap, double floor, double opacity, uint8_t* out_dev);
/* With mvlm_render_set_profiling on, the last heat sheet's stages in milliseconds (HIP events), f32[3]: background (the views
 * alone, with the copies of the two small tables), peak, compose.  Waits for the stream. */
int mvlm_heat_sheet_stage_ms(mvlm_ctx* ctx, float* ms3);

/* ---- surface heat (all views' heatmaps laid on the scan; DESIGN.md 5.1, "Surface heat") ---- */
/* Every vertex of the mesh is carried into every view with mvlm_render's own transform (the context's sub-pixel bits), tested
 * against the depth plane the network saw, and where a view sees it the view's heatmap values at its pixel add up per landmark.
 *   rot_dev     f64[n_views,9]             the rendered views' rotations on the device (mvlm_render_rotations_dev)
 *   images_dev  f32[n_views,256,256,4]     mvlm_render's stack (plane 3, the depth, is read), 16-byte aligned
 *   heat_dev    f32[n_views,n_lm,256,256]  as mvlm_cnn_heatmaps leaves them, 16-byte aligned
 *   sel_host    u8[n_lm] or NULL           the landmarks that may win a vertex's colour; NULL = all
 *   lm_rgb_host u8[n_lm,3] or NULL         a colour per landmark; NULL = (255, 0, 0)
 *   floor in [0, 1): scores up to it are not drawn; opacity in (0, 1]: at score 1; depth_tol 0..255: the depth steps (1/255 of the
 *   clip range, 5.9 model units) a vertex may lie behind the rendered surface and still count as seen
 *   vert_rgba_dev    u8[n_verts,4]         r g b 255 per vertex: what mvlm_render_landmark_view_colored takes
 *   score_dev        f32[n_verts,n_lm] or NULL (then the scores live in the context's scratch)
 *   n_vis_dev        i32[n_verts] or NULL  the views that see each vertex
 *   peak_vertex_dev  i32[n_lm]             per landmark the vertex of the largest score above 0, the lowest id on a tie; -1: none
 *   peak_score_dev   f32[n_lm]             that score; 0 for -1
 * Vertex v lies in view n at o = rm_transform(rot[n], v): pixel i = floor(o.X / 256), j = floor(o.Y / 256), inside iff v is finite,
 * 0 <= i, j < 256 and o.z in [0, 1]; the heat / image pixel is [255 - j, i].  It is seen iff inside and
 * trunc(255 o.z) <= ((256 - trunc(images[n,255-j,i,3] * 255 + 0.5)) & 255) + depth_tol.  With m the peak of plane (n, l) as
 * mvlm_heat_plane_peaks gives it and h the plane's value at the pixel, a view that sees v adds max(h / m, 0) where m is finite and
 * above 0 and h is finite, else 0; score[v,l] = (float)(the float64 sum over the views in ascending order / the views that see v),
 * 0 where none does.  Colour: the selected landmark of the largest score, the lowest index on a tie; a score <= floor leaves the
 * base - the vertex's own colour, else the nearest texel of its texture coordinates, else (200, 200, 200) -, otherwise the
 * landmark's colour is laid over the base with opacity * (score - floor) / (1 - floor), as the heat sheet blends.  All of it in
 * float64 or integers in the operation order of csrc/surface_backproject_math.h; no value depends on the scheduling.
 * n_lm 1..65536, n_views * n_lm <= 32768 planes and n_verts * n_lm <= 268435456 scores per call.  A NULL or misaligned pointer, a
 * value out of range or a point cloud ("point cloud" is in the message) set an error that starts with "surface heat:" and launch
 * nothing.  Only enqueues work on the launch stream. */
int mvlm_surface_heat(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_dev, const float* images_dev, const float* heat_dev,
                      int n_views, int n_lm, const uint8_t* sel_host, const uint8_t* lm_rgb_host, double floor, double opacity,
                      int depth_tol, uint8_t* vert_rgba_dev, float* score_dev /* f32[V,n_lm] or NULL */,
                      int32_t* n_vis_dev /* i32[V] or NULL */, int32_t* peak_vertex_dev /* i32[n_lm] */,
                      float* peak_score_dev /* f32[n_lm] */);
/* With mvlm_render_set_profiling on, the last surface heat's stages in milliseconds (HIP events), f32[3]: peak, back-projection
 * (the scores), paint (colours and per-landmark peaks).  Waits for the stream. */
int mvlm_surface_heat_stage_ms(mvlm_ctx* ctx, float* ms3);
/* Frees the surface heat's grow-only scratch (peaks, keys, the two small tables; the scores - 4 bytes per vertex and landmark -
 * where a call kept no score_dev).  Waits for the stream; the next mvlm_surface_heat allocates again. */
int mvlm_surface_heat_release(mvlm_ctx* ctx);
/* Bytes of the context's grow-only internal scratch whose names start with `prefix` ("backproject": the surface heat's; "": all). */
int mvlm_scratch_bytes(mvlm_ctx* ctx, const char* prefix, size_t* bytes);

/* ---- surface distances between landmarks (csrc/geodesic_math.h, DESIGN.md 5.1 "Surface distances") ---- */
/* The distance along the scan's triangles - the "tape-measure" distance - between landmarks, beside the straight one.  One distance
 * field per source landmark: the first-order fast-marching update (Hopf-Lax over a triangle's edge, Kimmel-Sethian / Bornemann-Rasch),
 * swept Jacobi-fashion until a sweep changes nothing.  It is NOT an exact polyhedral geodesic: it overestimates by a few per cent
 * (DESIGN.md 5.1 has the measured figures).  csrc/geodesic_math.h states the rule and every operation's order; all of it is
 * float64 on the mesh's float32 vertices, and no value depends on scheduling or on the order of a vertex's triangle list.
 *   pts_dev      f64[n,3]           the landmarks; each is attached as mvlm_surface_attach attaches it
 *   init_rings   0..8               the source triangle's corners are widened by this many rings of triangles, each vertex of the
 *                                   set starting at its straight distance from the snapped point (2 is the Python default)
 *   max_sweeps   1..1048576, 0 = 4096: a source that has not settled by then is an error that names it; the outputs are then
 *                                   filled with NaN / -1, never with a partial result
 *   max_scratch_bytes  0 = 512 MiB: the sources are processed in groups whose two field buffers (16 bytes per vertex and source,
 *                                   plus the context scratch's headroom: a quarter and 256 bytes) stay under it; a cap that cannot
 *                                   hold one source is an error
 *   pairs_host   i32[n_pairs,2] or NULL: with pairs only the landmarks named in one get a field, and only D[i,j] and D[j,i] of
 *                                   every pair (i, j) are computed; the other entries of D are NaN
 *   snapped_dev  f64[n,3], tri_dev i32[n]   the attachment (tri -1: no finite distance to any triangle)
 *   D_dev        f64[n,n]           D[i,j]: from source i to target j, read over the three edges of j's triangle; the straight
 *                                   distance where both lie in one triangle; 0 on the diagonal; +inf in another connected
 *                                   component; NaN in the row and column of a landmark that is not attached (tri -1, a triangle
 *                                   with a non-finite vertex, a non-finite point).  Directed: D[i,j] and D[j,i] differ by
 *                                   discretisation; the reported distance is their mean, their difference says how far to trust it
 *   E_dev        f64[n,n]           |P_i - P_j| of the snapped points, always all of it
 *   sweeps_dev   i32[n]             per source the index of the first sweep that changed nothing; -1 without a field
 *   field_dev    f64[n,n_verts] or NULL   the fields themselves; a row of NaN for a landmark without one
 * The adjacency (vertex -> incident triangles), the field buffers and the small tables live in the context's grow-only scratch
 * under "geodesic." (mvlm_scratch_bytes); mvlm_geodesic_release frees them.  n 1..65536.  A point cloud ("point cloud" is in the
 * message), a NULL or misaligned pointer, a value out of range or a pair index outside 0..n-1 set an error that starts with
 * "geodesics:" and launch nothing.  The sweep boundary is a kernel boundary: no workgroup ever waits for another.
 * WAITS FOR THE STREAM: the work is enqueued on the launch stream, but after every batch of 32 sweeps the host reads the
 * per-source settled flags, so the call returns only when the distances are final. */
int mvlm_landmark_geodesics(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n, int init_rings, int max_sweeps,
                            long long max_scratch_bytes, const int32_t* pairs_host, int n_pairs, double* snapped_dev,
                            int32_t* tri_dev, double* D_dev, double* E_dev, int32_t* sweeps_dev, double* field_dev);
/* With mvlm_render_set_profiling on, the last call's stages in milliseconds (HIP events), f32[4]: adjacency (with the attachment
 * and the straight distances), init, sweeps (with the host's reads), targets - the last three added up over the call's source
 * groups.  Waits for the stream. */
int mvlm_geodesic_stage_ms(mvlm_ctx* ctx, float* ms4);
/* Frees the "geodesic." scratch.  Waits for the stream; the next mvlm_landmark_geodesics allocates again. */
int mvlm_geodesic_release(mvlm_ctx* ctx);

/* ---- PNG on the device (the views' files without the picture crossing to the host) ---- */
/* Bytes that hold any file mvlm_png_encode writes for a picture of height x width (each 1..4096): the filtered stream
 * height * (1 + 3 * width), 10 bytes per 32 768-byte segment of it (5 of a stored block's header, 5 of the flush), and 63 of
 * signature, IHDR, IDAT framing, zlib header, Adler-32 and IEND.  No GPU and no context.  0, or 1 for a size out of range, 2 for
 * a NULL pointer. */
int mvlm_png_bound(int height, int width, size_t* bytes);
/* rgba_dev u8[n_images,height,width,4] on the device, the layout mvlm_render_landmark_view and mvlm_render_ray_view write (alpha
 * is dropped) -> n_images complete PNG files (8-bit RGB: colour type 2, no interlace, one IDAT) in host memory, file i at
 * png_host + i * stride_bytes with png_bytes_out[i] bytes.  The files are complete when the call returns (it waits for the
 * launch stream); only the compressed bytes are copied from the device.
 *   filter_mode   -1: every row takes the filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) with the smallest sum of
 *                 b < 128 ? b : 256 - b over its filtered bytes, the lowest type on a tie; 0..4: that type for every row
 * The filtered stream is cut into segments of 32 768 bytes, each compressed on its own by one workgroup: literals and matches
 * of distance 1 (runs), one DEFLATE block per segment - stored, fixed or dynamic Huffman, whichever makes the segment smallest -
 * and an empty stored block behind every compressed segment but the last.  The bytes are a function of the pixels only
 * (DESIGN.md 4.5 states every rule; tests/png_model.py states them a second time).
 * height and width 1..4096, n_images 1..128, n_images * height * width <= 8 * 2048 * 2048 as the view calls allow; a value out of
 * range, a filter_mode outside -1..4, stride_bytes below mvlm_png_bound's, a NULL pointer return an error that starts with
 * "png:" and launch nothing. */
int mvlm_png_encode(mvlm_ctx* ctx, const uint8_t* rgba_dev, int n_images, int height, int width, int filter_mode,
                    uint8_t* png_host, size_t stride_bytes, size_t* png_bytes_out /* [n_images] */);
/* With mvlm_render_set_profiling on, the last mvlm_png_encode's stages in milliseconds (HIP events), f32[4]: filter, deflate,
 * gather (offsets and copy on the device), copy to host (with the host's wait for the sizes in front of it). */
int mvlm_png_stage_ms(mvlm_ctx* ctx, float* ms4);

/* ---- landmark network (replaces paulsenpredictor.py:89-110, :167-217) ------------ */
/* blob/desc: output of mvlm_amd.weights.pack_for_device (BN folded, weights as
 * [tap][cin_pad][cout_pad]); copied to the device. */
int mvlm_cnn_load(mvlm_ctx* ctx, const float* blob_host, size_t n_floats, const int32_t* desc_host, int n_slots,
                  int n_landmarks, int in_channels);
/* bytes of caller-provided device scratch needed to push `batch` views at once */
size_t mvlm_cnn_workspace_bytes(mvlm_ctx* ctx, int batch);
/* images_dev f32[N,256,256,4]; chan_sel_host int[in_channels] picks the planes fed to
 * the net; maxima_dev f32[NL,N,3] = (row-1, col-0.5, value) per (landmark, view)
 * (paulsenpredictor.py:123-127).  Views are processed `batch` at a time. */
int mvlm_cnn_maxima(mvlm_ctx* ctx, const float* images_dev, int n_views, const int32_t* chan_sel_host,
                    float* maxima_dev, void* workspace_dev, size_t workspace_bytes, int batch);
/* which maximum mvlm_cnn_maxima reports per (view, landmark) plane (paulsenpredictor.py:112-158): MVLM_MAXIMA_SIMPLE
 * (default) the argmax pixel, MVLM_MAXIMA_MOMENT the 31x31 centroid around it where the peak lies more than 15 pixels
 * from every border.  Both come out of the fused path - the heatmaps are never written: for "moment" the window around
 * each peak is recomputed from conv10's output with conv11's own arithmetic (bit for bit what mvlm_cnn_heatmaps +
 * mvlm_heatmap_maxima(method 1) give).  Fails when the packed weights carry conv11 without its parity slots. */
int mvlm_cnn_set_selection(mvlm_ctx* ctx, int method);
/* same network, but materialises the final-stage heatmaps f32[N,NL,256,256]
 * (what paulsenpredictor.py:187-212 accumulates); used by tests and diagnostics. */
int mvlm_cnn_heatmaps(mvlm_ctx* ctx, const float* images_dev, int n_views, const int32_t* chan_sel_host,
                      float* heat_dev, void* workspace_dev, size_t workspace_bytes, int batch);
/* How the ~140 launches of a forward pass are issued.  graph_mode 1 (default): a pass over the same buffers and
 * shapes is captured as a hipGraph the second time it is seen and replayed afterwards; 0: always launch by
 * launch.  concurrency: 0 (default, the supported mode) = one stream.  1 = EXPERIMENT ONLY: for batches of <= 32 views
 * the lower hourglass pyramid goes to a second stream beside the 128x128 / 64x64 skip blocks - measured 2-10 % SLOWER
 * on the MI355X and kept for that measurement, not for use.  Results are identical in every mode.
 * mvlm_cnn_set_pairing: independent residual blocks of a hourglass level (the skip block and the first block of the
 * next lower level, paulsenpredictor.py:301-361) share launches conv by conv - 0 never, 1 (default) where the measured
 * table (csrc/conv_pair_tuned.h) says one two-problem launch beats two launches, 2 wherever one kernel variant can
 * serve both (tests, tuning).  Per convolution the arithmetic is that of the kernel variant that runs it; a pair may
 * run another variant than the single launch would, so results can differ in the last bits between pairing modes.
 * mvlm_cnn_execution_stats reports how many passes ran eagerly / were captured / replayed, and how many
 * captures failed (those passes ran eagerly instead). */
int mvlm_cnn_set_execution(mvlm_ctx* ctx, int graph_mode, int concurrency);
int mvlm_cnn_set_pairing(mvlm_ctx* ctx, int mode);
/* F(2,3) Winograd tiles on the exact path (csrc/conv_wino.h; conv_cfg.h: Cfg::WINO): the large stride-1 3x3 layers computed as four
 * GEMMs over row-transformed inputs and load-time-transformed weights - fp32 in, fp32 accumulation on the same MFMA, 4
 * multiplies per output pair where the direct form spends 6.  mode 0: never (the direct tiles only), 1 (default): where the
 * measured table csrc/conv_tuned_wino.h lists the layer (shape, kind, device batch), 2: every layer a Winograd variant can
 * serve (tests).  A new context takes its default from the environment variable MVLM_WINOGRAD (0 | 1 | 2).  Results differ
 * from the direct tiles' in the last bits (another summation order).  Profile records of such a launch
 * (mvlm_cnn_get_profile) count the FLOPs its MFMAs execute: 12 Cin Cout H W B, not 18.
 * mvlm_pack_winograd_weights: the host transform mvlm_cnn_load applies, packed f32[9][cin_pad][cout_pad] (tap = ky * 3 + kx) ->
 * f32[12][cin_pad][cout_pad] (slice t * 3 + kx; u0 = g0, u1 = (g0 + g1 + g2) / 2, u2 = (g0 - g1 + g2) / 2, u3 = g2 over ky,
 * float64 arithmetic, one rounding). */
int mvlm_cnn_set_winograd(mvlm_ctx* ctx, int mode);
int mvlm_pack_winograd_weights(const float* w9_host, int cin_pad, int cout_pad, float* w12_host);
/* The F(4,3) Winograd tile (csrc/conv_wino4.h; conv_cfg.h: Cfg::WINO4, variant conv3x3q_c32_t16x32): four output rows from six transformed
 * input rows and six GEMMs on the points 0, 1, -1, 2, -1/2, inf - 6 multiplies per four outputs where F(2,3) spends 8 and the
 * direct form 12, fp32 in and fp32 accumulation on the same MFMA.  It is consulted ahead of the F(2,3) table while the Winograd
 * mode is not 0.  mode 0: never, 1 (default): where the measured table csrc/conv_tuned_wino4.h lists the layer and the Winograd
 * mode is 1, 2: every layer the tile can serve (tests).  A new context takes MVLM_WINOGRAD4 (0 | 1 | 2) from the environment.
 * Profile records of such a launch count 9 Cin Cout H W B FLOPs.
 * mvlm_pack_winograd4_weights: f32[9][cin_pad][cout_pad] -> f32[18][cin_pad][cout_pad] (slice t * 3 + kx; u0 = g0,
 * u1 = -(g0 + g1 + g2) / 3, u2 = (g0 - g1 + g2) / 3, u3 = (g0 + 2 g1 + 4 g2) / 15, u4 = (-16 g0 + 8 g1 - 4 g2) / 15, u5 = g2 over
 * ky, float64 arithmetic, one rounding). */
int mvlm_cnn_set_winograd4(mvlm_ctx* ctx, int mode);
int mvlm_pack_winograd4_weights(const float* w9_host, int cin_pad, int cout_pad, float* w18_host);
/* The workgroup shape of that tile's launches.  A launch of code 2048 whose padded output channels are a multiple of 64 runs on
 * the wide shape - 64 output channels x 8 rows x 32 pixels, one staged input tile for two 32-channel halves - and every other
 * one on the 32 x 16 shape; the variant code, the FLOPs of a profile record and every output bit are the same either way.
 *   mvlm_cnn_set_winograd4_wide: 1 (default) as above, 0 the 32 x 16 shape on every launch; other values are refused.  A new
 *     context takes MVLM_WINOGRAD4_WIDE (0 | 1) from the environment.  The few (shape, kind) keys that measured slower on the wide
 *     shape inside the network (csrc/conv_wino4_wide_hold.h) stay on the 32 x 16 shape under either setting.
 *   mvlm_conv_wino4_wide_serves: 1 where a launch of this shape on code 2048 takes the wide shape while the switch is on.
 *   mvlm_conv_wino4_wide_launches: *count = launches issued on the wide shape by this context so far (host counter; a graph
 *     replay issues none); reset != 0 sets it to zero afterwards. */
int mvlm_cnn_set_winograd4_wide(mvlm_ctx* ctx, int on);
int mvlm_conv_wino4_wide_serves(int ksize, int cin_pad, int cout_pad, int size);
int mvlm_conv_wino4_wide_launches(mvlm_ctx* ctx, int64_t* count, int reset);
/* The 3x3 layers whose padded output channels are no multiple of 32 - conv6 / conv10 of an 84-landmark network on the 84-row direct
 * tile (variant 26), of a 73-landmark one on the 80-row tile (variant 16) - on that F(4,3) tile.  The dispatcher's choice of variant does
 * not move: once it is made, the dispatcher runs an eligible launch (plain 3x3 + bias into a plain tensor, size a multiple of 16, up
 * to 256 input channels, no variant forced, Winograd mode and F(4,3) mode not 0) on the F(4,3) kernel over weights [18][cin_pad][P]
 * and a bias [P], P = cout_pad rounded up to whole 32s, zeros beyond cout_pad; both are made once, where the weights are packed.
 * A profile record of such a launch carries code 2048 and the FLOPs of that tile.
 *   mvlm_cnn_set_winograd4_padded: 0 never (the direct tiles' launches and bits), 1 where the measured table
 *     csrc/conv_tuned_wino4_pad.h has a row (default), 2 every eligible launch (tests); MVLM_WINOGRAD4_PADDED likewise for a new context.
 *   mvlm_conv_wino4_padded_launches: *count = launches run that way by this context so far (host counter; a graph replay issues
 *     none); reset != 0 sets it to zero afterwards.
 *   mvlm_conv_wino4_padded_stride: P for this cout_pad.
 *   mvlm_pack_winograd4_weights_padded: host, w9 [9][cin_pad][cout_pad] -> w18_pad [18][cin_pad][P], columns below cout_pad as
 *     mvlm_pack_winograd4_weights gives them; bias [cout_pad] -> bias_pad [P] (both may be null: a layer without bias). */
int mvlm_cnn_set_winograd4_padded(mvlm_ctx* ctx, int mode);
int mvlm_conv_wino4_padded_launches(mvlm_ctx* ctx, int64_t* count, int reset);
int mvlm_conv_wino4_padded_stride(int cout_pad);
int mvlm_pack_winograd4_weights_padded(const float* w9_host, const float* bias_host, int cin_pad, int cout_pad, float* w18_pad_host,
                                       float* bias_pad_host);
int mvlm_cnn_execution_stats(mvlm_ctx* ctx, int64_t* eager_runs, int64_t* graph_captures, int64_t* graph_replays,
                             int64_t* graph_failures);
/* OPT-IN reduced-cost arithmetic ("fast" precision, mvlm_amd/csrc/conv_fast.hip): the big 3x3 layers (input channels a
 * multiple of 16, output channels of 64, 32-pixel rows) multiply bf16x3-split operands on the bf16 matrix cores - 6 of the 9
 * cross products, fp32 accumulation - at 6/16 of the exact path's matrix time.  Results are fp32-accurate but NOT bit-identical
 * to the exact path (argmax near-ties can flip); the default and every parity claim is the exact path.
 *   mvlm_pack_fast_weights: host; w f32[cout][cin][3][3] -> u16 [cin_pad/16][3][3][2][3][cout_pad][8]; returns the element
 *     count (out == NULL: only the count).
 *   mvlm_cnn_load_fast: after mvlm_cnn_load; one blob of packed layers, slot_offsets[n_slots] = u16 offset per conv slot or -1.
 *   mvlm_cnn_set_precision: 0 exact (default), 1 fast (bf16x3), 2 fast16 (f16x2, below).
 *   mvlm_conv2d_fast: test hook like mvlm_conv2d (3x3 only). */
size_t mvlm_pack_fast_weights(const float* w, int cout, int cin, int cout_pad, int cin_pad, uint16_t* out);
int mvlm_cnn_load_fast(mvlm_ctx* ctx, const uint16_t* blob_host, size_t n_u16, const int64_t* slot_offsets, int n_slots);
int mvlm_cnn_set_precision(mvlm_ctx* ctx, int fast);
int mvlm_conv2d_fast(mvlm_ctx* ctx, const float* x_dev, int batch, int cin, int h, int w, const float* w_host, int cout,
                     const float* bias_host, const float* pre_scale_host, const float* pre_shift_host,
                     const float* post_scale_host, const float* post_shift_host, const float* r_dev, float* y_dev);
/* Second opt-in form, mvlm_cnn_set_precision(ctx, 2) ("fast16"): the same layers on f16x2-split operands - x = h + l as two
 * fp16 terms (22 significant bits), the three cross products xh*wh + xh*wl + xl*wh on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation: 3/16 of the exact path's matrix time.  Per product 3-4 x the error of the bf16x3 form, still of the order of
 * an fp32 summation's own rounding.  The weights are scaled per layer by a power of two on the host (fp16's exponent is
 * narrow; the epilogue multiplies by the inverse, exactly); an activation with |x| >= 65504 has no fp16 form: the kernel
 * raises a flag, the pass's maxima scores (mvlm_cnn_maxima) / the first value of every heatmap plane (mvlm_cnn_heatmaps)
 * come back as NaN, and the Python layer repeats the pass with the bf16x3 form.
 *   mvlm_pack_fast_weights16: like mvlm_pack_fast_weights with two splits per operand; *unscale = the inverse scale.
 *   mvlm_cnn_load_fast16: after mvlm_cnn_load; slot_unscale[n_slots] = the inverse scale per conv slot.
 *   mvlm_cnn_fast16_overflowed: *overflowed = 1 when the last mvlm_cnn_maxima / mvlm_cnn_heatmaps call on this context met
 *     such an activation (waits for the context's stream).
 *   mvlm_conv2d_fast16: test hook like mvlm_conv2d_fast. */
size_t mvlm_pack_fast_weights16(const float* w, int cout, int cin, int cout_pad, int cin_pad, uint16_t* out, float* unscale);
int mvlm_cnn_load_fast16(mvlm_ctx* ctx, const uint16_t* blob_host, size_t n_u16, const int64_t* slot_offsets,
                         const float* slot_unscale, int n_slots);
int mvlm_cnn_fast16_overflowed(mvlm_ctx* ctx, int* overflowed);
int mvlm_conv2d_fast16(mvlm_ctx* ctx, const float* x_dev, int batch, int cin, int h, int w, const float* w_host, int cout,
                       const float* bias_host, const float* pre_scale_host, const float* pre_shift_host,
                       const float* post_scale_host, const float* post_shift_host, const float* r_dev, float* y_dev);
/* per-kernel timing of the last mvlm_cnn_* call when profiling is on: fills up to
 * `cap` records of {slot, kernel_variant, flops, ms}; returns the record count. */
int mvlm_cnn_set_profiling(mvlm_ctx* ctx, int enabled);
int mvlm_cnn_get_profile(mvlm_ctx* ctx, int32_t* slot, int32_t* variant, double* flops, float* ms, int cap);
const char* mvlm_conv_variant_name(int variant);
/* shapes of those records, in the same order: {ksize, cin_pad, cout_pad, size, kind, batch} per record (kind: 0 plain /
 * residual-block layer, 1 scatter into the skip tensor, 2 pooled output wanted; slot -1 = the pool kernel: channels in
 * cout_pad).  Returns the record count. */
int mvlm_cnn_get_profile_shapes(mvlm_ctx* ctx, int32_t* shapes6, int cap);
/* tuning hooks of tools/tune_in_network.py: mvlm_conv_variant_serves - can kernel variant `variant` run a 3x3 layer of this
 * shape and kind (1 / 0); mvlm_conv_set_override - every launch of this (shape, kind) on this context runs that variant,
 * ahead of the measured tables (variant < 0 removes the entry, ksize 0 all of them). */
int mvlm_conv_variant_serves(int variant, int ksize, int cin_pad, int cout_pad, int size, int kind);
int mvlm_conv_set_override(mvlm_ctx* ctx, int ksize, int cin_pad, int cout_pad, int size, int kind, int variant);

/* heatmap maxima of materialised heatmaps (replaces paulsenpredictor.py:112-165).
 * heat_dev f32[N,NL,S,S] -> out_dev f32[NL,N,3]. */
int mvlm_heatmap_maxima(mvlm_ctx* ctx, const float* heat_dev, int n_views, int n_landmarks, int size, int method,
                        float* out_dev);

/* one generic convolution launch (the kernel the network is made of); test hook.
 * x_dev f32[B,Cin,H,W] -> y_dev f32[B,Cout,H,W]; w_host f32[Cout,Cin,k,k] (k = 1|3,
 * stride 1, pad k/2); optional bias / pre-BN+ReLU (scale,shift per Cin) / post-BN+ReLU
 * (per Cout) / residual add r_dev f32[B,Cout,H,W]. */
int mvlm_conv2d(mvlm_ctx* ctx, const float* x_dev, int batch, int cin, int h, int w, const float* w_host, int cout,
                int ksize, const float* bias_host, const float* pre_scale_host, const float* pre_shift_host,
                const float* post_scale_host, const float* post_shift_host, const float* r_dev, int upsample_in,
                float* y_dev);

/* test hook for the two-problem launch: x_i f32[B,cin,size_i,size_i] * w_i f32[cout,cin,3,3] (shared pre-BN+ReLU per
 * input channel, optional residual r_i and raw copy raw_i, both f32[B,cout,size_i,size_i]) -> y_i, both in ONE grid of
 * kernel variant (variant & 255) with 1 << ((variant >> 8) & 3) / 1 << ((variant >> 10) & 3) K parts.  The results equal
 * mvlm_conv2d's with that variant forced, bit for bit. */
int mvlm_conv2d_pair(mvlm_ctx* ctx, int batch, int cin, int cout, const float* x0_dev, int size0, const float* w0_host,
                     const float* r0_dev, float* raw0_dev, float* y0_dev, const float* x1_dev, int size1,
                     const float* w1_host, const float* r1_dev, float* raw1_dev, float* y1_dev,
                     const float* pre_scale_host, const float* pre_shift_host, int variant);
/* test hook: mvlm_conv2d on this ctx runs kernel variant `variant` (ids of mvlm_conv_variant_name; -1 = automatic) */
int mvlm_conv_force_variant(mvlm_ctx* ctx, int variant);
/* kernel-variant timing for tools/tune_conv.py: `iters` launches of one layer shape on zero data with kernel
 * variant `variant` (< 0: the dispatcher's choice, reported in *variant_used); flags: 1 pre-BN+ReLU, 2 residual
 * add + raw copy, 4 bias, 8 post-BN+ReLU.  Fails for shapes the variant cannot serve. */
int mvlm_conv_bench(mvlm_ctx* ctx, int batch, int cin, int cout, int ksize, int size, int flags, int variant, int iters,
                    float* ms_per_launch, int* variant_used);
/* the same for tools/tune_conv_pairs.py: the 3x3 layer at `size` and at size / 2 (conv j of two independent residual
 * blocks) as the two tuned single launches (variant < 0) or as ONE two-problem launch of kernel variant (variant & 255)
 * with 1 << ((variant >> 8) & 3) and 1 << ((variant >> 10) & 3) K parts for the two problems. */
int mvlm_conv_pair_bench(mvlm_ctx* ctx, int batch, int cin, int cout, int size, int flags, int variant, int iters,
                         float* ms_per_launch);

/* ---- rays + consensus (replaces estimator3d.py:31-90, :92-183, utils3d.py:99-124) - */
/* maxima_dev f32[NL,N,3], rot_dev f64[N,9] -> starts_dev, ends_dev f64[NL,N,3] */
int mvlm_estimate_lines(mvlm_ctx* ctx, const float* maxima_dev, const double* rot_dev, int n_views, int n_landmarks,
                        int image_size, double* starts_dev, double* ends_dev);
/* view filter (estimator3d.py:140-155): mask_dev u8[NL,N], count_dev i32[NL] */
int mvlm_consensus_mask(mvlm_ctx* ctx, const float* maxima_dev, int n_views, int n_landmarks, int mode, double q,
                        double thr, uint8_t* mask_dev, int32_t* count_dev);
/* one wavefront per landmark: one-shot RANSAC + least squares (estimator3d.py:92-137,
 * :173-181).  draws_dev i32[NL,8] = the host's np.random.choice draws (indices into the
 * masked line list; ignored where count < 3).  out_dev f64[NL,3], err_dev f64[NL]
 * (the landmark's contribution to sum_error; 0 where count < 3). */
int mvlm_consensus_solve(mvlm_ctx* ctx, const double* starts_dev, const double* ends_dev, const uint8_t* mask_dev,
                         const int32_t* count_dev, const int32_t* draws_dev, int n_views, int n_landmarks,
                         double* out_dev, double* err_dev);

/* Opt-in quality report of the consensus.  One wavefront per landmark repeats mvlm_consensus_solve on the same inputs
 * (out_dev f64[NL,3] and err_dev f64[NL] are that call's, bit for bit) and writes what the solve decides and drops:
 *   counts_dev i32[NL,4]  k (surviving lines), n_inliers (squared distance < 100 to the 8-draw sample fit; 0 where k < 3),
 *                         n_used (lines of the final fit), branch (0: k < 3, plain least squares; 1: refit on the inliers;
 *                         2: "RANSAC failed", all lines, error 1e8)
 *   stats_dev f64[NL,MVLM_REPORT_STATS]  rms = sqrt(mean d2) and max_dist = sqrt(max d2) over the used lines, measured to
 *                         the final point (NaN where n_used == 0); sigma2 = sum d2 / (2 n_used - 3) (NaN where 2 n_used <= 3);
 *                         cov = sigma2 pinv(A), A = sum over the used lines of (I - n n^T), as xx yy zz xy xz yz
 *   dist2_dev f64[NL,N]   squared distance of EVERY view's ray to the final point (estimator3d.py:109-111)
 *   flags_dev u8[NL,N]    MVLM_VIEW_KEPT | _DRAWN | _INLIER | _USED */
#define MVLM_REPORT_STATS 9
#define MVLM_VIEW_KEPT 1
#define MVLM_VIEW_DRAWN 2
#define MVLM_VIEW_INLIER 4
#define MVLM_VIEW_USED 8
int mvlm_consensus_report(mvlm_ctx* ctx, const double* starts_dev, const double* ends_dev, const uint8_t* mask_dev,
                          const int32_t* draws_dev, int n_views, int n_landmarks, double* out_dev, double* err_dev,
                          double* stats_dev, int32_t* counts_dev, double* dist2_dev, uint8_t* flags_dev);

/* ---- surface snap (replaces estimator3d.py:252-285) ------------------------------ */
/* pts_dev f64[NL,3] -> out_dev f64[NL,3]: closest point on the triangle surface (of a point mesh: the nearest point) */
int mvlm_project_to_surface(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points,
                            double* out_dev);

/* The snap with its attachment: snapped_dev f64[n,3] is mvlm_project_to_surface's output, bit for bit; tri_dev i32[n] the
 * triangle that holds it (lowest id on ties; -1 for a landmark without a finite distance, which is passed through);
 * bary_dev f64[n,3] its weights of the triangle's corners, from the same Voronoi walk (NaN where tri is -1); uv_dev f64[n,2]
 * the mesh's texture coordinates interpolated with them (NaN when the mesh has none). */
int mvlm_surface_attach(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, double* snapped_dev,
                        int32_t* tri_dev, double* bary_dev, double* uv_dev);

/* ---- ray clipping / depth unprojection (replaces visualization/ray_visualizer.py:172-192) */
/* starts_dev, ends_dev f64[R,3] (e.g. the [NL,N,3] arrays of mvlm_estimate_lines) -> new_ends_dev f64[R,3]:
 * the first intersection of each segment with the triangle surface, or the old end when it misses;
 * hit_dev u8[R] (may be NULL) flags the hits.  Along a view ray this is the surface point the view's
 * depth buffer stores, evaluated at the maximum's sub-pixel position. */
int mvlm_clip_rays_to_mesh(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* starts_dev, const double* ends_dev,
                           int n_rays, double* new_ends_dev, uint8_t* hit_dev);

/* ---- multi-GPU: the one exchange of the sharded path (the reference's counterpart is the dormant
 * nn.DataParallel of paulsenpredictor.py:100-105) ---------------------------------------------------------------------
 * Views are sharded contiguously over `world` ranks (rank r holds views [r*base + min(r, rem), ...), sizes differing by at most
 * one: mvlm_amd/parallel.py shard_range); every rank passes the maxima of ITS views, f32[NL, n_local, 3] (NULL when it holds
 * none), and receives all of them in pose-table order, f32[NL, n_total, 3], on the context's stream: pack, ONE ncclAllGather
 * over `nccl_comm` (an ncclComm_t of the caller's RCCL, whose device is this context's), unpack.  RCCL is looked up at first
 * use (MVLM_RCCL_LIB = path, else the RCCL already loaded in the process, else librccl.so.1): nothing links against it.
 * nccl_comm == NULL is allowed in a world of one.  The Python host uses torch.distributed instead (same layout). */
int mvlm_allgather_maxima(mvlm_ctx* ctx, void* nccl_comm, int rank, int world, const float* maxima_local_dev, int n_total,
                          int n_landmarks, float* maxima_all_dev);
/* The two halves around the transport, for a host that moves the slots itself (MPI, hipMemcpyPeerAsync): a rank's slot is
 * f32[n_max, NL, 3], n_max = ceil(n_total / world), short shards zero-padded; slots_dev = the `world` slots in rank order. */
int mvlm_gather_pack(mvlm_ctx* ctx, const float* maxima_local_dev, int n_local, int n_max, int n_landmarks, float* slot_dev);
int mvlm_gather_unpack(mvlm_ctx* ctx, const float* slots_dev, int world, int n_total, int n_landmarks, float* maxima_all_dev);

#ifdef __cplusplus
}
#endif
#endif /* MVLM_HIP_H */
