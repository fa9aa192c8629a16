/* gp_trajectory.h -- motion trajectories drawn on the device: the C entry points of csrc/trajectory_kernels.hip, a part of libgp_hip.so
 * with an ABI number of its own.  (The header lives beside the sources, not in include/: see DESIGN section 21.)
 *
 * What it replaces: the drawing loop of [REF eval.py:38-73] (project_trajectory), up to H*W cv2.line calls per step on the host.  cv2
 * is not installed where this was written: PARITY WITH cv2.line IS UNPINNED, the definition below is this project's own.
 *
 * Projection of a point (x, y, z), in float32, one rounding per operation, no contraction [REF eval.py:48-62,
 * utils/camera_utils.py:195-267]:
 *   xc = ((R[0]*x + R[1]*y) + R[2]*z) + t[0],  yc and zc likewise from rows 1 and 2 of R;
 *   den = zc + 0.0001f;  u = (f*xc)/den + cx;  v = (f*yc)/den + cy   (the reference's one focal length for both axes);
 *   the point is DRAWABLE iff u and v are finite, |u| < 2^20, |v| < 2^20 and not zc <= min_depth (a NaN min_depth: no depth test);
 *   its pixel is ((int)u, (int)v), truncated toward zero.  A point that is not drawable is stored as
 *   (GP_TRAJ_NOT_DRAWABLE, GP_TRAJ_NOT_DRAWABLE), and a segment with such an end is skipped.
 *
 * Segment from pixel a (step s-1) to pixel b (step s): the major axis is x if |dx| >= |dy|, else y; dm, dn the absolute major and
 * minor deltas, sm, sn their signs.  dm == 0: the one pixel a.  Otherwise for k = 0 .. dm the pixel
 *   major = a_major + sm*k,  minor = a_minor + sn*floor((2*k*dn + dm - 1) / (2*dm))      (64-bit integers)
 * which is the incremental 8-connected Bresenham  e = dm - 2*dn; per pixel: if (e < 0) { minor += sn; e += 2*dm; } e -= 2*dn  started
 * at a.  Only the pixels inside the image are claimed, and only the k whose major coordinate is inside the image are visited.
 *
 * Order: step s of point j claims its pixels with key s*P + j + 1, by a 32-bit atomic maximum on owner[H][W] (uint32, zero = untouched):
 * a later step wins over an earlier one, a later point over an earlier one inside a step, and the result does not depend on the
 * schedule.  (s + 1)*P >= 2^32 - 1 is refused.
 *
 * Resolve: out[c][y][x] = colors[(key - 1) % P][c] where key != 0, else base[c][y][x], or 0 without a base.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  Neither
 * entry synchronises or reads the device. */
#ifndef GP_TRAJECTORY_H
#define GP_TRAJECTORY_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_TRAJ_ABI_VERSION 1

#define GP_TRAJ_NOT_DRAWABLE (-2147483647 - 1)    /* both members of the stored pixel of a point that is not drawable */
#define GP_TRAJ_COORD_LIMIT 1048576               /* |u|, |v| below 2^20 */

typedef struct gp_traj_view {
    float R[9];          /* view.R transposed (world -> camera), row-major */
    float t[3];          /* view.T */
    float f, cx, cy;     /* fov2focal(FoVx, W), W / 2, H / 2 */
} gp_traj_view;

int gp_traj_abi_version(void);

/* One step.  view: on the HOST.  xyz: [N][3] float32 on the device.  idx: [P] int32 on the device, point j is row idx[j] of xyz (a row
 * outside [0, N) is not drawable: nothing outside xyz is read), or NULL: point j is row j, and then N >= P.  px: [P][2] int32 on the
 * device, read when s > 0 (the pixels of step s - 1) and written (those of step s).  owner: [H][W] uint32 on the device, zeroed by the
 * caller before step 0.  P == 0 launches nothing.  Refused: N, P, s < 0; H or W <= 0 or H*W >= 2^31; P >= 2^31; (s + 1)*P >= 2^32 - 1;
 * idx == NULL and N < P; idx != NULL and N == 0 and P > 0; a null pointer. */
int gp_traj_step(const gp_traj_view* view, const float* xyz, const int32_t* idx, int64_t N, int64_t P, int64_t s, int32_t* px,
                 uint32_t* owner, int32_t H, int32_t W, float min_depth, gp_stream_t stream);

/* colors: [P][3] float32; base: [3][H][W] float32 or NULL; out: [3][H][W] float32, all on the device.  A key whose point is not below
 * P cannot come from gp_traj_step with this P; with P == 0 every pixel is the base's. */
int gp_traj_resolve(const uint32_t* owner, const float* colors, int64_t P, const float* base, float* out, int32_t H, int32_t W,
                    gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
