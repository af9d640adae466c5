/*
 * lidargs_knn.h -- C ABI of the model initialisation of GaussianModel.create_from_pcd (the reference's scene/gaussian_model.py:272-318).
 *
 * lidargs_knn_mean_dist replaces distCUDA2 of the third-party `simple_knn` extension (CUDA only, not vendored in the reference; what is
 * written below about it rests on its published behaviour, not on its source, which this project does not have).  The contract this
 * library implements and its tests pin:
 *   points f32, row i at points + i * row_stride (row_stride >= 3 floats: a [P, 4] layout is read in place); out f32[P]; device pointers,
 *   the work runs on `stream` with no host read.
 *   For point i the candidates are all j != i (self is excluded by INDEX: a duplicate of i is a candidate at distance 0).
 *   d = dx*dx + dy*dy + dz*dz in float32 with dx = p_j.x - p_i.x, evaluated as written, without contraction.
 *   The 3 smallest d that are < FLT_MAX are kept; a slot without a candidate holds FLT_MAX.
 *   out[i] = ((b0 + b1) + b2) / 3.0f with b0 <= b1 <= b2, in float32, correctly rounded division.
 *   Hence: P = 1 and P = 2 give +inf; P = 3 gives a finite value near FLT_MAX / 3; a point with a NaN or inf coordinate is never anyone's
 *   neighbour and its own value is +inf.  The result depends only on the multiset of the 3 smallest float32 distances: it is
 *   deterministic and independent of the input order.
 *   scratch: lidargs_knn_scratch_bytes(P) bytes of device memory (about 44 bytes per point).  P <= 2^30.  Returns 0 or a negative
 *   LIDARGS_ERR_* code.
 *
 * lidargs_voxelize_sample replaces voxelize_sample (:272-276) after its shuffle: np.unique(np.round(data / voxel_size), axis=0) * voxel_size.
 *   points: P rows of 3 contiguous values, float32 (is_double = 0) or float64 (is_double = 1).  The quotient is the correctly rounded
 *   division by voxel_size rounded to the data's precision, np.round is rint (half to even), the product is in the data's precision.
 *   The output, `alloc_out(out_user, U * 3 * element size)` (device memory, called once, not at all for P = 0), receives the U distinct
 *   rows in ascending lexicographic (x, y, z) order.  Returns U >= 0 or a negative LIDARGS_ERR_* code: LIDARGS_ERR_INVALID_ARGUMENT for
 *   voxel_size <= 0 or not finite, and for a row that is not finite or whose quotient reaches 2^62 in magnitude.  One -0.0 / +0.0 choice
 *   differs from numpy's, which depends on the shuffle: the output holds +0.0.  Two host reads (the key span, the row count).
 *   scratch: lidargs_voxelize_scratch_bytes(P) bytes of device memory.
 */
#ifndef LIDARGS_KNN_H
#define LIDARGS_KNN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t lidargs_knn_scratch_bytes(int P);
int lidargs_knn_mean_dist(int P, const float* points, int row_stride, float* out, char* scratch, size_t scratch_bytes, void* stream);

size_t lidargs_voxelize_scratch_bytes(int P);
int lidargs_voxelize_sample(int P, const void* points, int is_double, double voxel_size, char* scratch, size_t scratch_bytes,
                            char* (*alloc_out)(void* user, size_t bytes), void* out_user, void* stream);

#ifdef __cplusplus
}
#endif
#endif
