/* gp_voxel.h -- voxel-grid downsampling of a point cloud on the device, in the semantics of Open3D's PointCloud::VoxelDownSample:
 * the C entry points of csrc/voxel_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * What it replaces: pcd.voxel_down_sample(voxel_size) in the loop of [REF utils/prepare/downsample_points.py], which makes the
 * points3D_downsample.ply that [REF scene/dataset_readers.py:294] opens.  Open3D is not installed where this was written: the
 * semantics below are restated from its published source and parity with its binary is unpinned.
 *
 * Semantics, all in float64 without contraction (one pass over N points [N][3], optional colours [N][3] and normals [N][3]):
 *   min_bound = min(points) - voxel_size / 2 and max_bound = max(points) + voxel_size / 2, per axis;
 *   refused: voxel_size <= 0; voxel_size * INT32_MAX < max over the axes of (max_bound - min_bound) ("voxel_size is too small");
 *            a coordinate that is not finite (it never reaches a conversion to an integer); N >= 2^31;
 *   index = (int32)floor((p - min_bound) / voxel_size) per axis: that subtraction and that IEEE division, no reciprocal; >= 0;
 *   one output row per occupied voxel: the sum of its rows, added one by one in ascending input row, starting from zero, divided by
 *   double(count); colours and normals are averaged the same way and normals are not re-normalised;
 *   the output rows ascend in (ix, iy, iz), x most significant.  (Open3D's order is that of its hash map: only the SET of rows is
 *   Open3D's.)
 *
 * The device pass is two entries because its refusals and the width of its sort key need the bounds on the host:
 *   gp_voxel_bounds       two launches -> `record` on the device; the caller reads its 8 doubles (the first host read of a pass)
 *   gp_voxel_downsample   takes those 8 doubles back as a HOST array, refuses or launches the rest, leaves M on the device in `m_out`;
 *                         the caller reads it (the second and last host read of a pass) and keeps the first M rows of the outputs
 * Neither entry synchronises or reads the device itself.  Nothing is a floating-point atomic and no sum depends on a schedule: two
 * calls on equal inputs give equal bytes.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 (or -1 from a query) plus gp_last_error(), a
 * gp_stream_t last. */
#ifndef GP_VOXEL_H
#define GP_VOXEL_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_VOXEL_ABI_VERSION 1

#define GP_VOXEL_RECORD_DOUBLES 8    /* min x y z, max x y z, 1.0 where a coordinate was not finite (else 0.0), 0.0 */

int gp_voxel_abi_version(void);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for both device entries on n points; -1 for n < 0 or n >= 2^31. */
int64_t gp_voxel_scratch_bytes(int64_t n);

/* points: [n][3] float64 on the device, n >= 1.  record: GP_VOXEL_RECORD_DOUBLES float64 on the device.  min and max are exact in any
 * order; a coordinate that is not finite sets record[6] and takes no part in them. */
int gp_voxel_bounds(int64_t n, const double* points, void* scratch, double* record, gp_stream_t stream);

/* One pass.  points / colors / normals: [n][3] float64 on the device, colors and normals may be NULL, and then so are their outputs.
 * bounds: the record of gp_voxel_bounds on these points, on the HOST.  out_*: [n][3] on the device (n rows: M is not known before the
 * launches), of which the first M are written; out_index: the int32 voxel index (ix, iy, iz) of each output row.  m_out: one int32 on
 * the device.  n == 0 stores M = 0 and launches nothing else. */
int gp_voxel_downsample(int64_t n, const double* points, const double* colors, const double* normals, double voxel_size,
                        const double* bounds, double* out_points, double* out_colors, double* out_normals, int32_t* out_index,
                        int32_t* m_out, void* scratch, gp_stream_t stream);

/* The same pass on HOST pointers, through the same programs (csrc/voxel_core.h), for the tests that run without a device: it is not a
 * fallback of the device entries.  The outputs hold n rows; *m_out = M. */
int gp_voxel_downsample_host(int64_t n, const double* points, const double* colors, const double* normals, double voxel_size,
                             double* out_points, double* out_colors, double* out_normals, int32_t* out_index, int64_t* m_out);

#ifdef __cplusplus
}
#endif
#endif
