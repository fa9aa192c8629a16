/* gp_tsdf.h -- TSDF fusion of depth renders and mesh extraction on the device: the C entry points of csrc/tsdf_kernels.hip, a part of
 * libgp_hip.so with an ABI number of its own.  (The header lives beside the sources, not in include/: see DESIGN section 26.)
 *
 * What it adds: gp_depth.h stops at one loose point cloud per view.  Here the depth maps of many views of one instant are fused into
 * one truncated signed distance volume, and the surface tsdf = iso leaves as a watertight triangle mesh with colours.
 *
 * Everything is float32, one correctly rounded operation at a time (the library is built without contraction; fmaf is one operation).
 *
 * The volume: nx x ny x nz grid POINTS.  Point (i, j, k) is at (fmaf((float)i, voxel, origin_x), fmaf((float)j, voxel, origin_y),
 * fmaf((float)k, voxel, origin_z)); its linear index is n = (k*ny + j)*nx + i.  tsdf [nz][ny][nx], weight [nz][ny][nx], color
 * [3][nz][ny][nx] (or NULL: a volume without colour), float32 on the device.  A fresh volume is all zeros.
 *
 * 1. Integrate: V views in ONE launch, 1 <= V <= GP_TSDF_MAX_VIEWS.  A lane takes one grid point (x fastest across lanes), keeps its
 *    tsdf, weight and colour in registers over the V views in their order, and stores them once: the volume is read and written once
 *    for V views.  A view: world_view [16] float32 on the device, the camera's world_view_transform as stored, m[col*4 + row], and the
 *    tangents of its half angles.  For view v and the point (x, y, z):
 *      P_r = fmaf(m[r], x, fmaf(m[4 + r], y, fmaf(m[8 + r], z, m[12 + r])))     r = 0, 1, 2
 *      skipped unless P_z > z_min
 *      xn = P_x / (P_z * tanfovx);  px = ((xn + 1.f) * (float)W - 1.f) * 0.5f      (the projection kernel's own pixel centre)
 *      fx = floorf(px + 0.5f);  skipped unless fx is finite and 0 <= fx < (float)W    (compared as floats);  ix = (int)fx
 *      the same with P_y, tanfovy, H for fy, iy
 *      d = depth[v][iy][ix];  skipped unless valid[v][iy][ix] != 0 (a NULL array: every pixel), d is finite and d > 0
 *      s = d - P_z;  skipped if s < -trunc
 *      t = fminf(1.f, s / trunc);  wn = w + view_weight
 *      tsdf = (tsdf * w + t * view_weight) / wn;  color_c = (color_c * w + image[v][c][iy][ix] * view_weight) / wn
 *      w = fminf(wn, weight_max)
 *    No atomics: a point's result depends on its own history only, so V views in one call equal V calls of one view, byte for byte.
 *
 * 2. Extraction: marching tetrahedra on the Kuhn (Freudenthal) split of every cell.  With the corners of a cell numbered by their
 *    offsets as bits (x = 1, y = 2, z = 4), tetrahedron q of the six is (v0, v1, v2, v3) = (0, 1<<a, (1<<a)|(1<<b), 7), the axis orders
 *    (a, b, c) in lexicographic order: 012, 021, 102, 120, 201, 210.  det[v1 - v0, v2 - v0, v3 - v0] is the sign of the permutation: q =
 *    0, 3, 4 are positively oriented, q = 1, 2, 5 negatively.  The split is the same in every cell, so the diagonals of a face agree
 *    between the two cells that share it and the surface is watertight by construction; no 256-row table is needed.
 *      Point USABLE: weight >= min_weight and tsdf finite.  Point INSIDE: tsdf < iso (a sample equal to iso is NOT inside).
 *      Cell ACTIVE: all eight corners usable.  A cell is numbered by its corner 000.
 *      Edges: every grid point owns the seven lattice edges towards +x, +y, +z, +xy, +xz, +yz, +xyz (e = 0 .. 6, direction bits 1, 2,
 *      4, 3, 5, 6, 7); edge id 7*n + e.  These are all the edges of all tetrahedra.  An edge CROSSES iff it lies in at least one
 *      active cell (the owner's cell stepped back along any of the axes the edge does not run along) and its ends differ in INSIDE.
 *    Vertices: one per crossing edge, in ascending edge id.  p0 the owning end, p1 the other, t0 and t1 their tsdf:
 *      a = (iso - t0) / (t1 - t0);  position_c = fmaf(a, p1_c - p0_c, p0_c);  colour_c = fmaf(a, color1_c - color0_c, color0_c)
 *    computed once per edge: every triangle that shares the vertex sees the same bits.
 *    Triangles: in ascending cell index, then tetrahedron 0 .. 5, then triangle 0 .. 1; active cells only.  For a POSITIVELY oriented
 *    tetrahedron, writing ij for the vertex on the edge between tetrahedron vertices i and j:
 *      one vertex i inside, the others j, k, l with (i, j, k, l) an even permutation of (0, 1, 2, 3):     (ij, ik, il)
 *      one vertex i outside, likewise:                                                                   (ij, il, ik)
 *      two inside i < j, two outside k, l with (i, j, k, l) even: the quadrilateral ik, il, jl, jk is cut along ik-jl into
 *                                                                                                        (ik, il, jl), (ik, jl, jk)
 *      none or all four inside: no triangle.
 *    A negatively oriented tetrahedron swaps the second and third vertex of each triangle.  The geometric normal (b - a) x (c - a) of a
 *    triangle (a, b, c) then points from inside to outside, towards larger tsdf.  (tsdf_core.h holds the sixteen rows this rule gives;
 *    tests/tsdf_ref.py derives them again from the rule, and the tests hold closed surfaces to: every edge in two triangles, every
 *    directed edge once, V - E + F = 2, a positive volume.)  A sample equal to iso puts a vertex ON that grid point (a = 1 or 0); the
 *    zero-area triangles this can produce are KEPT, so that the mesh stays closed.
 *    faces [F][3] int32: vertex numbers.
 *
 *    Two calls, because the sizes are known on the device only:
 *      gp_tsdf_extract_count  the active byte of every cell; the seven crossing bits of every point and the triangles of its cell
 *                             (plain stores); per tile of GP_TSDF_TILE consecutive points the two sums; one workgroup scans the tiles
 *                             in order and leaves counts = (vertices, faces); then every point's first vertex and first triangle:
 *                             its tile's offset plus an ordered scan inside the tile (wave scans, the sixteen wave totals through LDS).
 *      gp_tsdf_extract_fill   vertices, colors, faces from the same scratch, the same volume and the same iso.  A triangle finds its
 *                             vertex as first_vertex[owner] + the crossing bits of the owner below the edge's own.
 *    The scratch: per grid point one active byte, one byte of crossing bits, one byte of triangles, a uint32 first vertex and a uint32
 *    first triangle -- 11 bytes a point -- plus two uint32 per tile, each array 256-byte aligned.
 *    counts[1] is computed in 32 bits: a volume with more than 2^31 - 1 triangles (at least 178 956 971 cells) is not supported.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  No entry
 * synchronises or reads the device.  Refused everywhere: a null volume or null tsdf or weight; nx, ny or nz < 1; 7*nx*ny*nz >= 2^31;
 * voxel or trunc not > 0; a non-finite origin, voxel or trunc.  gp_tsdf_integrate also: V < 1 or V > GP_TSDF_MAX_VIEWS; H or W <= 0
 * or H*W >= 2^31; null depth, views or a view's world_view; non-finite tangents; an image without a colour volume or a colour volume
 * without an image; z_min, view_weight or weight_max not finite or not > 0.  The extraction also: a non-finite iso, a NaN min_weight,
 * null or unaligned (4 bytes) scratch, null counts, vertices or faces; colors without a colour volume or a colour volume without. */
#ifndef GP_TSDF_H
#define GP_TSDF_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_TSDF_ABI_VERSION 1

#define GP_TSDF_MAX_VIEWS 16         /* the views of one gp_tsdf_integrate launch */
#define GP_TSDF_TILE 1024            /* grid points per workgroup of the extraction's ordered scans */
#define GP_TSDF_EDGES 7              /* the lattice edges a grid point owns */

typedef struct gp_tsdf_volume {
    float* tsdf;                     /* [nz][ny][nx] on the device */
    float* weight;                   /* [nz][ny][nx] */
    float* color;                    /* [3][nz][ny][nx], or NULL */
    int32_t nx, ny, nz;
    float origin_x, origin_y, origin_z, voxel, trunc;
} gp_tsdf_volume;

typedef struct gp_tsdf_view {
    const float* world_view;         /* [16] on the device: the camera's world_view_transform as stored, m[col*4 + row] */
    float tanfovx, tanfovy;
} gp_tsdf_view;

int gp_tsdf_abi_version(void);

/* vol, views: on the HOST (views: an array of V, carried into the launch by value).  depth: [V][H][W] float32; valid: [V][H][W] uint8 or
 * NULL; image: [V][3][H][W] float32, required iff vol->color, all on the device. */
int gp_tsdf_integrate(const gp_tsdf_volume* vol, const float* depth, const uint8_t* valid, const float* image, const gp_tsdf_view* views,
                      int32_t V, int32_t H, int32_t W, float z_min, float view_weight, float weight_max, gp_stream_t stream);

/* The bytes of the extraction's scratch, as stated above.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);

/* vol: on the HOST.  scratch: as sized above; counts: [2] int32 (vertices, faces), on the device. */
int gp_tsdf_extract_count(const gp_tsdf_volume* vol, float iso, float min_weight, void* scratch, int32_t* counts, gp_stream_t stream);

/* After gp_tsdf_extract_count on the same stream, with the same vol, iso and scratch.  vertices: [counts[0]][3] float32; colors:
 * [counts[0]][3] float32, required iff vol->color; faces: [counts[1]][3] int32, on the device. */
int gp_tsdf_extract_fill(const gp_tsdf_volume* vol, float iso, const void* scratch, float* vertices, float* colors, int32_t* faces,
                         gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
