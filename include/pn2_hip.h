/*
 * include/pn2_hip.h -- C ABI of the MI355X-native PointNet++ set-abstraction operators.
 *
 * Drop-in boundary for 3DIoUMatch's `pointnet2._ext` (reference pybind surface:
 * pointnet2/_ext_src/src/bindings.cpp:11-24).  Every entry point below replaces one of
 * the reference's C-level launchers (the `*_kernel_wrapper` functions the pybind layer
 * calls); the argument order and meaning are the reference's, with two additions:
 *   - an explicit `hipStream_t` (passed as void*) -- the reference takes the current
 *     torch stream implicitly (at::cuda::getCurrentCUDAStream(), e.g. ball_query_gpu.cu:54);
 *   - an `int` return (hipError_t value, 0 = success) instead of fprintf+exit(-1)
 *     (cuda_utils.h:35-44).
 * Pointers are DEVICE pointers unless stated.  No torch types cross this boundary.
 *
 * Layouts (all contiguous, as the reference requires via CHECK_CONTIGUOUS, utils.h:16-19):
 *   xyz / new_xyz / unknown / known : (B, N, 3) float32
 *   points / features / grads       : (B, C, N) float32
 *   idx                             : int32
 */
#ifndef PN2_HIP_H
#define PN2_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* replaces furthest_point_sampling_kernel_wrapper (sampling.cpp:16-18, sampling_gpu.cu:180-234).
 * dataset (b,n,3); temp (b,n) scratch -- contents on entry are ignored (the reference's
 * pybind layer fills it with 1e10, sampling.cpp:78-80; this library initialises it itself);
 * idxs (b,m) int32, idxs[:,0] = 0.  Index-exact vs the reference, including its
 * tie-breaking order and its |p|^2 <= 1e-3 skip rule. */
int pn2_furthest_point_sampling(int b, int n, int m, const float *dataset, float *temp,
                                int *idxs, void *stream);

/* Same operator with a caller-provided workspace of pn2_fps_workspace_bytes(b,n,m) bytes
 * (replaces furthest_point_sampling_kernel_wrapper, sampling.cpp:16-18, like the entry point
 * above).  Large clouds then run the bucketed tier: the cloud is sorted once into spatial
 * buckets and each of the m-1 rounds only touches buckets whose bounding box is closer to the
 * new sample than their largest running distance -- same indices, ~10x fewer bytes per round. */
int pn2_furthest_point_sampling_ws(int b, int n, int m, const float *dataset, int *idxs,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* workspace size for pn2_furthest_point_sampling_ws; the reference's counterpart is the (b,n)
 * float `temp` tensor it allocates per call (sampling.cpp:78-80) */
size_t pn2_fps_workspace_bytes(int b, int n, int m);

/* replaces gather_points_kernel_wrapper (sampling.cpp:9-11, sampling_gpu.cu:13-35).
 * points (b,c,n), idx (b,npoints) -> out (b,c,npoints). */
int pn2_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                      float *out, void *stream);

/* replaces gather_points_grad_kernel_wrapper (sampling.cpp:12-14, sampling_gpu.cu:39-62).
 * grad_out (b,c,npoints), idx (b,npoints) -> grad_points (b,c,n); the callee zeroes
 * grad_points first (the reference relies on torch::zeros, sampling.cpp:57-59). */
int pn2_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                           const int *idx, float *grad_points, void *stream);

/* replaces query_ball_point_kernel_wrapper (ball_query.cpp:9-11, ball_query_gpu.cu:14-59).
 * new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample): first nsample point indices (ascending)
 * with squared distance < radius*radius, remaining slots padded with the first hit, all-zero
 * row when there is no hit.  The callee writes every element of idx (no pre-zeroing needed).
 * workspace: device scratch of at least pn2_ball_query_workspace_bytes(b,n,m,nsample) bytes
 * (may be NULL when that function returns 0). */
int pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                   const float *xyz, int *idx, void *workspace, size_t workspace_bytes,
                   void *stream);
/* scratch size for pn2_ball_query above (the reference needs none, ball_query.cpp:24-33) */
size_t pn2_ball_query_workspace_bytes(int b, int n, int m, int nsample);

/* replaces group_points_kernel_wrapper (group_points.cpp:9-11, group_points_gpu.cu:13-46).
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample). */
int pn2_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                     const int *idx, float *out, void *stream);

/* replaces group_points_grad_kernel_wrapper (group_points.cpp:13-15, group_points_gpu.cu:48-80).
 * grad_out (b,c,npoints,nsample), idx -> grad_points (b,c,n); callee zeroes grad_points. */
int pn2_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                          const int *idx, float *grad_points, void *stream);

/* replaces three_nn_kernel_wrapper (interpolate.cpp:9-10, interpolate_gpu.cu:14-73).
 * unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) SQUARED distances, idx (b,n,3). */
int pn2_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                 int *idx, void *stream);

/* replaces three_interpolate_kernel_wrapper (interpolate.cpp:11-13, interpolate_gpu.cu:77-117).
 * points (b,c,m), idx (b,n,3), weight (b,n,3) -> out (b,c,n). */
int pn2_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                          const float *weight, float *out, void *stream);

/* three_interpolate (interpolate.cpp:47-75, K8 interpolate_gpu.cu:77-117) plus an affine term in
 * three more inputs per query: out (b,c,n) = interpolate(points (b,c,m), idx, weight) +
 * affine_w (c,3) . affine_x (b,3,n).  For a 1x1 convolution over cat([3 coordinate rows,
 * interpolated features]) (models/grid_conv_module.py:87-110): the convolution commutes with the
 * interpolation, so the GEMM runs over the m source points and this call writes the layer's output.
 * m <= 2048, n a multiple of 4, 16-byte aligned idx / weight / affine_x / out. */
int pn2_three_interpolate_affine_supported(int c, int m, int n);
int pn2_three_interpolate_affine(int b, int c, int m, int n, const float *points, const int *idx,
                                 const float *weight, const float *affine_w, const float *affine_x,
                                 float *out, void *stream);
/* the same with affine_w as a view of a wider row-major matrix, row l at affine_w + l * affine_w_ld
 * (>= 3): the coordinate columns of the convolution's weight (models/grid_conv_module.py:87-110) read
 * in place, without a copy of the slice */
int pn2_three_interpolate_affine_ld(int b, int c, int m, int n, const float *points, const int *idx,
                                    const float *weight, const float *affine_w, int affine_w_ld,
                                    const float *affine_x, float *out, void *stream);

/* replaces three_interpolate_grad_kernel_wrapper (interpolate.cpp:14-17,
 * interpolate_gpu.cu:121-159) -- the INTENDED scatter-add.  The reference's pybind layer
 * never reaches that launcher (interpolate.cpp:95 dispatches the forward kernel instead,
 * SURVEY section 0 defect 1); this entry point computes the true gradient.
 * grad_out (b,c,n), idx (b,n,3), weight (b,n,3) -> grad_points (b,c,m); callee zeroes it. */
int pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                               const int *idx, const float *weight, float *grad_points,
                               void *stream);

/* pn2_three_interpolate / pn2_three_interpolate_grad (interpolate.cpp:47-104) on channel SLICES
 * of wider tensors: out / grad_out point at the first channel of a c-channel slice inside a
 * (b, c_total, n) tensor.  PointnetFPModule concatenates the interpolated features with the skip
 * features (pointnet2_modules.py:404-410): writing straight into the concatenated buffer and
 * reading the gradient straight out of the concatenated gradient saves a copy of both. */
int pn2_three_interpolate_into(int b, int c, int m, int n, const float *points, const int *idx,
                               const float *weight, float *out, int c_total, void *stream);
/* pn2_three_interpolate_into (interpolate.cpp:47-75) at channels [channel0, channel0 + c) of out
 * (b, c_total, n) -- out is the tensor's BASE here -- plus, in the same launch, rows (b, rows_c, n)
 * copied into channels [rows_channel0, rows_channel0 + rows_c): both halves of the concatenations of
 * pointnet2_modules.py:404-410 (skip features after the block) and models/grid_conv_module.py:87-110
 * (coordinate rows before it).  The two channel ranges must not overlap. */
int pn2_three_interpolate_rows_into(int b, int c, int m, int n, const float *points, const int *idx,
                                    const float *weight, float *out, int c_total, int channel0,
                                    const float *rows, int rows_c, int rows_channel0, void *stream);
/* (interpolate.cpp:77-104, the intended scatter-add, on a slice of the gradient) */
int pn2_three_interpolate_grad_from(int b, int c, int n, int m, const float *grad_out, int c_total,
                                    const int *idx, const float *weight, float *grad_points,
                                    void *stream);

/* ---- additions (no reference counterpart; the reference composes these in Python) ---- */

/* Fused QueryAndGroup front end (pointnet2_utils.py:335-358): ball query, gather of xyz and
 * of the C feature channels, centroid subtraction and optional 1/radius scaling, written once
 * into the concatenated (b, 3+c, m, nsample) tensor the shared MLP consumes.  features may be
 * NULL (c == 0).  idx (b,m,nsample) is also returned (needed by the backward pass).
 * normalize_xyz != 0 divides the relative xyz by radius (pointnet2_utils.py:352-353). */
int pn2_query_and_group(int b, int n, int m, int c, float radius, int nsample, int normalize_xyz,
                        const float *new_xyz, const float *xyz, const float *features,
                        int *idx, float *out, void *workspace, size_t workspace_bytes,
                        void *stream);

/* Second half of pn2_query_and_group alone, for an idx computed earlier (e.g. one step ahead on a
 * side stream): the gathers + centroid subtraction + concatenation of pointnet2_utils.py:348-358. */
int pn2_group_concat(int b, int n, int m, int c, float radius, int nsample, int normalize_xyz,
                     const float *new_xyz, const float *xyz, const float *features,
                     const int *idx, float *out, void *stream);

/* ---- cell lists as an object (no reference counterpart: the reference's ball query scans the
 * whole cloud per centroid, ball_query_gpu.cu:24-47) ------------------------------------------
 * pn2_ball_query / pn2_query_and_group above build the cell lists of `xyz` inside the call (two
 * kernels) and throw them away.  A set-abstraction layer samples the cloud (FPS) and then queries
 * balls in the SAME cloud (pointnet2_modules.py:236-250), so the lists can be left behind by the
 * sampling kernel, which streams the cloud anyway, and be queried any number of times. */

/* bytes of a cell-list object for b clouds of n points; 0 = shape not covered (n < 4096 or
 * n > 131072): use pn2_ball_query (the reference allocates nothing, ball_query.cpp:24-33) */
size_t pn2_grid_bytes(int b, int n);

/* Launch order of the ball queries (an addition without a reference counterpart: the reference's
 * query_ball_point_kernel, ball_query_gpu.cu:14-49, answers centroid blockIdx-major in the order
 * given).  pn2_furthest_point_sampling_grid knows both the lists and the centroids it picked, and
 * leaves a permutation of 0..m-1 in the object, longest query first; the query kernels follow it
 * when they are asked for the same number of centroids (any permutation gives the same rows).
 * This call tells where: cloud i's int32 row of cells starts at
 * start_offset + 4 * start_stride * i bytes, its entry [order_for_slot] holds the m the order is
 * for (0: none), and its order at order_offset + 4 * n * i bytes. */
int pn2_grid_launch_order(int b, int n, size_t *start_offset, int *start_stride,
                          int *order_for_slot, size_t *order_offset);

/* build the cell lists of xyz (b,n,3) for balls of `radius` into grid (pn2_grid_bytes bytes);
 * the stand-alone form of what query_ball_point_kernel_wrapper's replacement does internally
 * (ball_query.cpp:9-11) */
int pn2_grid_build(int b, int n, float radius, const float *xyz, void *grid, size_t grid_bytes,
                   void *stream);

/* pn2_ball_query on prebuilt cell lists (same radius as at build time): replaces
 * query_ball_point_kernel_wrapper (ball_query.cpp:9-11, ball_query_gpu.cu:14-59), same result;
 * nsample <= 256 */
int pn2_ball_query_prebuilt(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                            const float *xyz, int *idx, const void *grid, size_t grid_bytes,
                            void *stream);

/* pn2_query_and_group on prebuilt cell lists: ONE kernel for the ball query and the gathers of
 * QueryAndGroup.forward (pointnet2_utils.py:335-358) */
int pn2_query_and_group_prebuilt(int b, int n, int m, int c, float radius, int nsample,
                                 int normalize_xyz, const float *new_xyz, const float *xyz,
                                 const float *features, int *idx, float *out, const void *grid,
                                 size_t grid_bytes, void *stream);

/* pn2_query_and_group_prebuilt for the case the set-abstraction layer is in
 * (pointnet2_modules.py:236-250): `grid` was left behind by pn2_furthest_point_sampling_grid(b, n, m, xyz, idxs, ...) and
 * new_xyz[i][j] == xyz[i][idxs[i][j]] -- the centroids ARE that call's picks, in pick order.  The
 * sampling kernel then also left, per centroid, a QUERY PLAN next to the lists (row offsets and
 * lengths of its nine cell rows, the centroid, its place in the launch order -- 64 bytes, 144
 * for a neighbourhood that needs more than one pass of nine loads; csrc/grid_common.h), and a query wave starts from one scalar load instead of walking
 * order -> centroid -> cell -> row offsets.  Same rows, same bits as pn2_query_and_group_prebuilt
 * (which this call becomes when the object holds no plan for m: m > n / 8, or lists from
 * pn2_grid_build).  With other centroids the result is undefined: use _prebuilt. */
int pn2_query_and_group_picks(int b, int n, int m, int c, float radius, int nsample,
                              int normalize_xyz, const float *new_xyz, const float *xyz,
                              const float *features, int *idx, float *out, const void *grid,
                              size_t grid_bytes, void *stream);

/* 1 if pn2_furthest_point_sampling_grid can leave cell lists behind for clouds of n points
 * (bucketed tier, 8192 <= n <= 65535); the reference's kernel has no such by-product
 * (sampling_gpu.cu:75-178) */
int pn2_fps_grid_supported(int n);

/* pn2_furthest_point_sampling_ws (furthest_point_sampling_kernel_wrapper, sampling.cpp:16-18)
 * that ALSO fills `grid` with the cell lists of `dataset` for balls of grid_radius -- the indices
 * are exactly those of pn2_furthest_point_sampling_ws. */
int pn2_furthest_point_sampling_grid(int b, int n, int m, const float *dataset, int *idxs,
                                     void *workspace, size_t workspace_bytes, float grid_radius,
                                     void *grid, size_t grid_bytes, void *stream);

/* ---- sampling a sampled cloud -------------------------------------------------------------
 * A set-abstraction stack samples the cloud it has just sampled: SA2 runs
 * furthest_point_sampling on the 2048 centroids SA1 picked, in the order SA1 picked them
 * (pointnet2_modules.py:236-240 on the previous layer's new_xyz; backbone_module.py:97-112).  The
 * reference's K1 (sampling_gpu.cu:75-178) starts from index 0 and then takes, round after round,
 * the point farthest from everything taken so far.  On a cloud S = (s_0, s_1, ...) that IS such a
 * sequence over a larger cloud, round j finds s_j again: s_j was the strict maximum over the
 * whole cloud, hence over S, and the running distances of the points of S evolve exactly as they
 * did (same picks, same fp32 operations in the same order).  So the answer is 0, 1, ..., m-1
 * -- unless some round of the run that produced S had TWO points equally far (the reference's
 * reduction-tree key then decides by index, and the indices of S are new), or had nothing left to
 * take (a maximum of zero: the run then repeats earlier picks, and a cloud that holds the same
 * point twice ties with itself from the first round on).
 *
 * pn2_furthest_point_sampling_ties = pn2_furthest_point_sampling_grid (grid may be null: no cell
 * lists) that also reports, per cloud, first_tie[b] = the first round whose maximum was held by
 * two or more points or was zero (m if none; 0 when no point takes part): the first first_tie
 * picks are strict maxima over the whole cloud, and distinct.
 * pn2_furthest_point_sampling_prefix = pn2_furthest_point_sampling_ws for a cloud of n points that
 * is the head (first n picks, in order) of the sequence a _ties call produced, or of a head of
 * it: clouds with first_tie[b] >= n get 0..m-1 without running a round; the others are sampled
 * as usual.  first_tie is read on the device (graph-capturable); null = always sample. */
int pn2_fps_ties_supported(int n);
int pn2_furthest_point_sampling_ties(int b, int n, int m, const float *dataset, int *idxs,
                                     void *workspace, size_t workspace_bytes, float grid_radius,
                                     void *grid, size_t grid_bytes, int *first_tie, void *stream);
int pn2_furthest_point_sampling_prefix(int b, int n, int m, const float *dataset, int *idxs,
                                       void *workspace, size_t workspace_bytes,
                                       const int *first_tie, void *stream);

/* ---- scatter-add through an inverse index ---------------------------------------------------
 * group_points_grad (group_points.cpp:42-65, K6 group_points_gpu.cu:48-69) adds every element of
 * grad_out into grad_points[idx] with a same-address atomic.  idx is reused by every channel and
 * every step, so it can be inverted once: inv (b, npoints*nsample) holds the positions of a cloud
 * sorted by the point they refer to (point << 16 | position).  Covered: n <= 4096 and
 * npoints*nsample <= 32768 (SA2 .. SA4 and the vote aggregation of the network). */
int pn2_group_inverse_supported(int n, int npoints, int nsample);
/* entries per cloud of the inverse (npoints*nsample rounded up to 4096/8192/16384/32768; the
 * surplus slots hold 0xFFFFFFFF); 0 when out of range (sizing helper for group_points.cpp:42-65) */
int pn2_group_inverse_entries(int npoints, int nsample);
/* idx (b,npoints,nsample) with values < n -> inv (b, pn2_group_inverse_entries()) uint32, sorted
 * entry s stored at [(s % chunk) * 1024 + s / chunk], chunk = entries / 1024
 * (no reference counterpart; input of the gradient kernel below, group_points.cpp:42-65) */
int pn2_group_inverse_build(int b, int n, int npoints, int nsample, const int *idx,
                            unsigned *inv, void *stream);
/* replaces group_points_grad_kernel_wrapper (group_points.cpp:13-15, group_points_gpu.cu:48-80)
 * given inv: channels channel0 .. channel0+c-1 of grad_out (b,c_total,npoints,nsample) ->
 * grad_points (b,c,n), every element written once (c_total = c, channel0 = 0: the reference's
 * argument; the slice form reads the feature part of a QueryAndGroup gradient in place) */
int pn2_group_points_grad_sorted(int b, int c, int n, int npoints, int nsample,
                                 const float *grad_out, int c_total, int channel0,
                                 const unsigned *inv, float *grad_points, void *stream);

/* normalised inverse-distance weights of the three nearest neighbours: replaces
 * weight = 1 / (dist + 1e-8); weight / sum(weight) of models/grid_conv_module.py:94-98 and
 * pointnet2_modules.py:395-398 (and the sqrt of pointnet2_utils.py:147); dist2 (n,3) as returned
 * by pn2_three_nn -> weight (n,3) */
int pn2_three_nn_weights(long long n, const float *dist2, float *weight, void *stream);

/* n device-to-device copies in one launch; table: n rows of (src, dst, bytes) as 64-bit values
 * in device memory, max_bytes the largest row (no reference counterpart: the reference feeds
 * each batch to the network directly, train.py:305-371 / pretrain.py:260-300; here a prefetched
 * batch is staged into the buffers the captured graphs read) */
int pn2_multi_copy(int n, const void *table, long long max_bytes, void *stream);

/* Human-readable text for a non-zero return value (hipGetErrorString); stands in for the
 * message the reference prints before exit(-1) in CUDA_CHECK_ERRORS (cuda_utils.h:35-44). */
const char *pn2_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* PN2_HIP_H */
