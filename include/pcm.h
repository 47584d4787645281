/*
 * pcm.h -- C ABI of libpcm_hip.so, the MI355X (gfx950) point-set metric library.
 *
 * Drop-in boundary for 3D-FENet's loss/metric hot path.  Every entry point
 * replaces one pybind/ATen entry of the reference's vendored CUDA extensions:
 *
 *   pcm_chamfer_forward   <- chamfer_3D.forward   (metric/chamfer3D/chamfer_cuda.cpp:17-19,
 *                                                  metric/chamfer3D/chamfer3D.cu:136-154)
 *   pcm_chamfer_backward  <- chamfer_3D.backward  (metric/chamfer3D/chamfer_cuda.cpp:22-27,
 *                                                  metric/chamfer3D/chamfer3D.cu:176-195)
 *   pcm_emd_forward       <- emd.forward          (metric/emd/emd.cpp:12-17,
 *                                                  metric/emd/emd_cuda.cu:228-282)
 *   pcm_emd_backward      <- emd.backward         (metric/emd/emd.cpp:19-23,
 *                                                  metric/emd/emd_cuda.cu:302-316)
 *   pcm_icp, pcm_nearest_neighbor, pcm_best_fit_transform
 *                         <- icp / nearest_neighbor / best_fit_transform
 *                            (utils/icp.py:68-118, :49-65, :4-46; numpy + sklearn
 *                            on the host in the reference, testnet.py:62-64)
 *   pcm_silhouette_forward / _backward, pcm_proj_bce
 *                         <- cont_proj (utils/projection.py:4-67) and the 'bce_prob'
 *                            loss (loss/proj_loss.py:17-19, :43): torch ops in the
 *                            reference, finetune.py:154-162
 *   pcm_fps               <- farthest_point_sample + index_points (utils/utils.py:316-360;
 *                            a torch loop in the reference, utils/datasets_sample_pcl.py:87-94)
 *   pcm_knn, pcm_repulsion_loss
 *                         <- knn_cuda.KNN and Loss.get_repulsion_loss, which the reference's
 *                            loss class was written around and then dropped (loss/loss.py:16-17)
 *
 * Conventions:
 *   - all pointers are DEVICE pointers to contiguous row-major arrays:
 *     clouds [b, n, 3] float32 (AoS xyz), per-point outputs [b, n];
 *     indices are int32 like the reference's IntTensor outputs;
 *   - the caller owns every buffer (as the reference's Python wrappers do);
 *     outputs are fully written by the library (no caller zero-fill needed,
 *     except where a function says so);
 *   - work is enqueued asynchronously on `stream` (a hipStream_t; NULL = the
 *     null stream) of the CURRENT HIP device; nothing here synchronises,
 *     allocates device memory or keeps global state, so every call is
 *     reentrant and capturable into a hipGraph;
 *   - return value: PCM_OK (0) or a negative pcm_status; pcm_strerror()
 *     names it.  (The reference returned 1/0/-1 and its Python ignored it;
 *     the Python wrappers here raise RuntimeError on any non-zero status.)
 */
#ifndef PCM_H_
#define PCM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pcm_status {
    PCM_OK = 0,
    PCM_ERR_INVALID_ARG = -1,   /* bad shape / size / null pointer (reference: -1)  */
    PCM_ERR_LAUNCH = -2,        /* HIP launch or runtime error (reference: 0)      */
    PCM_ERR_WORKSPACE = -3,     /* workspace missing or too small                  */
    PCM_ERR_UNSUPPORTED = -4,   /* size outside what this build supports          */
    PCM_ERR_IO = -5,            /* file missing, unreadable or truncated           */
    PCM_ERR_FORMAT = -6         /* not an (npoints, 3) float .npy array            */
} pcm_status;

/* Library / ABI version: major*10000 + minor*100 + patch. */
int pcm_version(void);

/* Human-readable name of a status code (static string, never NULL). */
const char *pcm_strerror(int status);

/* ---------------------------------------------------------------------- */
/* Chamfer3D                                                               */
/* ---------------------------------------------------------------------- */

/*
 * Bidirectional nearest neighbour, squared L2 (chamfer3D.cu:12-154).
 *   dist1[b,j] = min_k ||xyz2[b,k] - xyz1[b,j]||^2 , idx1 = lowest argmin k
 *   dist2[b,k] = min_j ||xyz1[b,j] - xyz2[b,k]||^2 , idx2 = lowest argmin j
 * Distance is evaluated as fmaf(dz,dz,fmaf(dy,dy,dx*dx)), dx = target - query.
 * Non-finite inputs follow the reference's 512-point tile semantics exactly.
 * m == 0 leaves dist1/idx1 untouched, n == 0 leaves dist2/idx2 untouched
 * (as the reference's loops do).  b, n, m >= 0.
 */
int pcm_chamfer_forward(const float *xyz1, const float *xyz2, int b, int n, int m,
                        float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                        void *stream);

/*
 * Fused forward + loss (extension; replaces the torch reductions that
 * loss/loss.py:34-36 and utils/metrics.py:56-60 run on the forward's outputs):
 * everything pcm_chamfer_forward does, plus
 *   mean_out[0] = mean(dist1), mean_out[1] = mean(dist2)   (device float[2])
 * summed in a fixed order (deterministic run to run).  Needs b, n, m > 0 and a
 * device workspace of pcm_chamfer_workspace_bytes(b, n, m) bytes that is
 * ZERO-FILLED when first allocated; the kernels keep it consistent across
 * stream-ordered calls (not concurrent ones), so it is zero-filled only once.
 */
size_t pcm_chamfer_workspace_bytes(int b, int n, int m);
int pcm_chamfer_forward_loss(const float *xyz1, const float *xyz2, int b, int n, int m,
                             float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                             float *mean_out, void *workspace, size_t workspace_bytes,
                             void *stream);

/*
 * Fused Chamfer loss + gradient (extension): the training step of
 * loss/loss.py:31-37 (chamfer_3DDist forward + torch.mean(dist1) +
 * torch.mean(dist2)) and its backward (chamfer3D.cu:155-195) in ONE launch:
 *   - everything pcm_chamfer_forward does (dist1, dist2, idx1, idx2);
 *   - mean_out[0] = mean(dist1), mean_out[1] = mean(dist2),
 *     mean_out[2] = mean_out[0] + mean_out[1]        (device float[3]);
 *   - gradxyz1/gradxyz2 = gradients of  w1*sum(dist1) + w2*sum(dist2),
 *     bit-identical to pcm_chamfer_backward with graddist1 = w1 and
 *     graddist2 = w2 everywhere (w1 = 1/(b*n), w2 = 1/(b*m) for the mean loss).
 * Deterministic.  Needs b > 0, 0 < n, m <= 1024 (else PCM_ERR_UNSUPPORTED:
 * use pcm_chamfer_forward_loss + pcm_chamfer_backward) and the zero-filled
 * workspace of pcm_chamfer_workspace_bytes(b, n, m) (the same buffer serves
 * pcm_chamfer_forward_loss; stream-ordered reuse only).
 */
int pcm_chamfer_loss_grad(const float *xyz1, const float *xyz2, int b, int n, int m, float w1, float w2,
                          float *dist1, float *dist2, int32_t *idx1, int32_t *idx2, float *mean_out,
                          float *gradxyz1, float *gradxyz2, void *workspace, size_t workspace_bytes,
                          void *stream);

/*
 * The fused loss + gradient as train.py:163-176 drives it (extension):
 *   chamfer_loss = mean(dist1) + mean(dist2) on fake.transpose(2, 1), then
 *   total_loss = chamfer_loss * lambda_cd + ..., total_loss.backward().
 * pcm_chamfer_loss_grad_layout is pcm_chamfer_loss_grad with
 *   - either cloud in channel planes (layout 1, as pcm_chamfer_forward_layout),
 *     read in place, its gradient written in the same layout;
 *   - grad_scale (nullable, device float): the upstream gradient the loss is
 *     expected to receive.  The gradients are those of
 *     grad_scale * (w1 sum(dist1) + w2 sum(dist2)) computed as the reference's
 *     backward does it: graddist = fl(grad_scale * w) (torch's mean backward,
 *     w = fl(1/(b n)) as torch forms it), g = 2 graddist
 *     (chamfer3D.cu:160-171).  mean_out then needs 4 floats: mean_out[3]
 *     receives the scale used.  NULL: scale 1 (pcm_chamfer_loss_grad).
 * pcm_chamfer_loss_grad_rescale is its backward once the real upstream
 * gradient *grad_loss is known (device floats; none of them may alias):
 *   - *grad_loss == *scale_used bit for bit (pass mean_out + 3): the step's
 *     gradients are already exact and the launch does nothing;
 *   - otherwise gradxyz1/2 are recomputed in place from idx1/idx2 with
 *     graddist = fl(*grad_loss * w) -- bit-identical to pcm_chamfer_backward
 *     fed that constant -- and scale_used NULL always recomputes;
 *   - *scale_next = *grad_loss (nullable): the expectation for the next step.
 * A training loop with a constant loss weight therefore recomputes once, on
 * its first step, and from then on runs the forward, the loss and the exact
 * weighted gradient in one launch plus one empty launch.  Needs 0 < n, m <=
 * 1024 and the workspace of pcm_chamfer_loss_grad.
 */
int pcm_chamfer_loss_grad_layout(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                                 float w1, float w2, const float *grad_scale, float *dist1, float *dist2,
                                 int32_t *idx1, int32_t *idx2, float *mean_out, float *gradxyz1, float *gradxyz2,
                                 void *workspace, size_t workspace_bytes, void *stream);
int pcm_chamfer_loss_grad_rescale(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                  int layout2, float w1, float w2, const float *grad_loss, const float *scale_used,
                                  float *scale_next, const int32_t *idx1, const int32_t *idx2, float *gradxyz1,
                                  float *gradxyz2, void *stream);
/*
 * `steps` back-to-back pcm_chamfer_loss_grad launches from one host call with
 * the arguments bound once: K steps of a native training loop on fixed
 * buffers (bench.py's N=1 region).  steps >= 0.
 */
int pcm_chamfer_loss_grad_steps(int steps, const float *xyz1, const float *xyz2, int b, int n, int m, float w1,
                                float w2, float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                float *mean_out, float *gradxyz1, float *gradxyz2, void *workspace,
                                size_t workspace_bytes, void *stream);

/*
 * Device-side failure of the fused-loss kernels on `workspace`: PCM_OK or
 * PCM_ERR_LAUNCH.  A gradient-phase wait of pcm_chamfer_loss_grad that times
 * out (workgroups that are not resident) is NOT a failure: the waiting
 * workgroup computes the missing argmins itself, so dist/idx/gradients are
 * exact and only time is lost.  The failure reported here is the loss poll's
 * own wait (a much longer bound) timing out: that call's means are NaN and the
 * error is sticky -- every later call on that workspace reports NaN means
 * until the caller zero-fills the workspace again (the Python wrappers detect
 * it one call later and do that, raising PcmError).  Synchronises `stream`.
 */
int pcm_chamfer_workspace_status(const void *workspace, size_t workspace_bytes, int b, int n, int m, void *stream);

/*
 * Chamfer backward (chamfer3D.cu:155-195).  With g = 2*graddist:
 *   gradxyz1[j] = g1[j](xyz1[j]-xyz2[idx1[j]]) - sum_{k: idx2[k]=j} g2[k](xyz2[k]-xyz1[j])
 *   gradxyz2[k] = g2[k](xyz2[k]-xyz1[idx2[k]]) - sum_{j: idx1[j]=k} g1[j](xyz1[j]-xyz2[k])
 * Deterministic: scatter terms are summed in ascending source index, in the
 * kernel order of the reference (gradxyz1: direct term first; gradxyz2: direct
 * term last).  gradxyz1/gradxyz2 are fully overwritten.
 */
int pcm_chamfer_backward(const float *xyz1, const float *xyz2, int b, int n, int m,
                         const float *graddist1, const float *graddist2,
                         const int32_t *idx1, const int32_t *idx2,
                         float *gradxyz1, float *gradxyz2, void *stream);

/*
 * Clouds in either layout (extension): layout 0 = [b, n, 3] rows, as above;
 * layout 1 = [b, 3, n] channel planes -- the generator's B x 3 x N output,
 * which train.py:163 hands to the loss as fake.transpose(2, 1); the
 * reference's wrapper copies such a view to rows first (dist_chamfer_3D.py:79-80),
 * these read it in place, and the backward writes each cloud's gradient in
 * that cloud's layout (so autograd's transpose backward needs no copy either).
 * Results are bit-identical to pcm_chamfer_forward / pcm_chamfer_backward on
 * the rows.  float32 only; per-point outputs and graddists stay [b, n].
 */
int pcm_chamfer_forward_layout(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                               float *dist1, float *dist2, int32_t *idx1, int32_t *idx2, void *stream);
int pcm_chamfer_backward_layout(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                                const float *graddist1, const float *graddist2, const int32_t *idx1,
                                const int32_t *idx2, float *gradxyz1, float *gradxyz2, void *stream);
/*
 * The layout backward with graddists read in place at any element strides
 * (batch, point) >= 0 (extension): graddist1[bi * gd1_batch_stride +
 * j * gd1_point_stride].  Strides 0 read the expanded scalar torch.mean's
 * backward hands chamfer_3DFunction.backward (loss/loss.py:36), which the
 * reference's wrapper materialised with graddist.contiguous()
 * (dist_chamfer_3D.py:59-60).  Results are bit-identical to the contiguous call.
 */
int pcm_chamfer_backward_strided(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                 int layout2, const float *graddist1, long long gd1_batch_stride,
                                 long long gd1_point_stride, const float *graddist2, long long gd2_batch_stride,
                                 long long gd2_point_stride, const int32_t *idx1, const int32_t *idx2,
                                 float *gradxyz1, float *gradxyz2, void *stream);

/*
 * fp16 clouds (extension for BASELINE config 5; the reference accepted fp32
 * only).  xyz1/xyz2 hold IEEE binary16 values.  Coordinates are widened to
 * fp32 exactly, so dist/idx are bit-identical to pcm_chamfer_forward on the
 * widened clouds (fp32 outputs, as the reference's), and the gradients are the
 * fp32 path's gradients rounded once to binary16 (nearest even).
 */
int pcm_chamfer_forward_f16(const uint16_t *xyz1, const uint16_t *xyz2, int b, int n, int m,
                            float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                            void *stream);
int pcm_chamfer_backward_f16(const uint16_t *xyz1, const uint16_t *xyz2, int b, int n, int m,
                             const float *graddist1, const float *graddist2,
                             const int32_t *idx1, const int32_t *idx2,
                             uint16_t *gradxyz1, uint16_t *gradxyz2, void *stream);

/*
 * Forward with a caller-owned workspace (extension): the same outputs as
 * pcm_chamfer_forward / pcm_chamfer_forward_f16, bit for bit.  When both
 * clouds hold >= 4096 points and b*n*m >= 2^28 it sorts them into a uniform
 * grid in the workspace and scans only the cells around each block of
 * queries (with a proof that no farther point can win, else a wider scan),
 * which is what large clouds (BASELINE config 5, N=M=16384) need; smaller
 * problems take the dense kernels and ignore the workspace.  The workspace
 * needs no initialisation and holds no state between calls.
 * pcm_chamfer_forward_ws_bytes returns 0 for a problem that takes the dense
 * kernels, so the size does not grow with the shape: a buffer shared by
 * several shapes must be sized by querying each of them (the largest answer
 * serves all); a buffer sized for a dense-path shape is too small for a grid
 * one (PCM_ERR_WORKSPACE).
 */
size_t pcm_chamfer_forward_ws_bytes(int b, int n, int m);
int pcm_chamfer_forward_ws(const float *xyz1, const float *xyz2, int b, int n, int m,
                           float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                           void *workspace, size_t workspace_bytes, void *stream);
int pcm_chamfer_forward_ws_f16(const uint16_t *xyz1, const uint16_t *xyz2, int b, int n, int m,
                               float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * One-pass Chamfer evaluation (extension): the F-score, precision and recall of
 * loss/loss_.py:122-140 (fscore) at up to eight squared-distance thresholds,
 * and the per-cloud mean nearest-neighbour distances, without the B x N x M
 * float64 distance matrix of batch_NN_loss (:93-109), without argmins and
 * without any per-point output.  It replaces fscore's compare / cast / mean /
 * arithmetic / NaN fix-up (:132-138) as well: two launches in all.
 *
 * Contract: for every batch element and both directions the per-point value is
 * exactly the dist1[b,j] / dist2[b,k] pcm_chamfer_forward would produce -- for
 * finite inputs the minimum of the pinned fmaf(dz,dz,fmaf(dy,dy,dx*dx)) values
 * (independent of the scan order, so no index is tracked); with non-finite
 * coordinates the reference's 512-point tile rule decides, as there.
 *   thresholds: HOST pointer to nth floats (1 <= nth <= 8, any order), read
 *     during the call and passed to the kernel by value: no device-side
 *     threshold buffer, so the call is capturable.
 *   With c1 = #{j: dist1[b,j] < th[t]} and c2 = #{k: dist2[b,k] < th[t]}
 *   (strict '<', loss_.py:132-133; a NaN distance is never counted):
 *     counts[b,t,0] = c1, counts[b,t,1] = c2                       (int32)
 *     p_x = (float)c1 / (float)n    share of xyz1's points within th of xyz2
 *     p_y = (float)c2 / (float)m    share of xyz2's points within th of xyz1
 *     f   = (c1 + c2 == 0) ? 0.f : ((2.f * p_y) * p_x) / (p_y + p_x)
 *                                   (loss_.py:134-135: the 0/0 NaN becomes 0)
 *     scores[b,t,:] = f, p_x, p_y
 *     mean_dist[b,0] = sum_j dist1[b,j] / (float)n, mean_dist[b,1] = sum_k dist2[b,k] / (float)m
 *   batch_scores (nullable) [nth,3]: loss_.py:136-138 -- the sequential fp32
 *     sum over b = 0, 1, ... of scores[b,t,:], divided by (float)b.
 *   fscore(X, Y, th) of the reference = batch_scores[0,0], [0,2], [0,1]
 *   (its precision_1 is the mean over Y's points: p_y).
 * Sums are formed in a fixed order (wave, workgroup, then each cloud's
 * workgroups in ascending order): deterministic, no float atomics.
 * Any n, m >= 1; b limited only by the grid (else PCM_ERR_UNSUPPORTED).
 * PCM_ERR_INVALID_ARG before any device call for negative sizes, n == 0 or
 * m == 0 with b > 0, nth outside 1..8, or a null cloud / threshold / output
 * pointer with b > 0; PCM_ERR_WORKSPACE for a workspace that is NULL or
 * shorter than pcm_chamfer_eval_workspace_bytes(b, n, m, nth); b == 0 is a
 * no-op.  The workspace needs no initialisation and holds no state between
 * calls; every output element is fully written.
 * pcm_chamfer_eval_f16: IEEE binary16 clouds widened exactly, so every output
 * is bit-identical to pcm_chamfer_eval on the widened clouds.
 */
size_t pcm_chamfer_eval_workspace_bytes(int b, int n, int m, int nth);
int pcm_chamfer_eval(const float *xyz1, const float *xyz2, int b, int n, int m, const float *thresholds, int nth,
                     float *mean_dist, int32_t *counts, float *scores, float *batch_scores, void *workspace,
                     size_t workspace_bytes, void *stream);
int pcm_chamfer_eval_f16(const uint16_t *xyz1, const uint16_t *xyz2, int b, int n, int m, const float *thresholds,
                         int nth, float *mean_dist, int32_t *counts, float *scores, float *batch_scores,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Cross Chamfer matrix                                                    */
/* ---------------------------------------------------------------------- */

/* Largest cloud (points) pcm_chamfer_cross takes (else PCM_ERR_UNSUPPORTED). */
#define PCM_CROSS_MAX_POINTS 16384

/*
 * Cross Chamfer matrix (extension): the mean nearest-neighbour squared distance
 * of EVERY cloud of one set to EVERY cloud of another, both directions -- what
 * nearest-shape retrieval, MMD-CD / COV-CD / 1-NNA-CD and duplicate checks
 * between splits are functions of.  xyz1 holds s clouds of n points, xyz2 r
 * clouds of m points.
 * Values, both stored at [i, j] of an [s, r] matrix, so the caller's Chamfer
 *   distance of (x_i, y_j) is their sum:
 *     mean12[i, j] = (1/n) sum_p min_q d2(x_i[p], y_j[q])
 *     mean21[i, j] = (1/m) sum_q min_p d2(x_i[p], y_j[q])
 * Per-point arithmetic: d2 is the pinned fmaf(dz,dz,fmaf(dy,dy,dx*dx)) of
 *   float32 differences; for finite input the per-point minimum is exactly the
 *   dist1 / dist2 entry pcm_chamfer_forward gives for that pair of clouds (the
 *   minimum of the pinned values is independent of the scan order: no argmin,
 *   no rescan).
 * Sums: a cloud's per-point minima are added in float64 in a fixed order (a
 *   lane its queries ascending, a wave by the six DPP steps, the waves
 *   ascending, then the cloud's workgroups ascending), divided by (double)n
 *   (or m) and rounded ONCE to float32.  No float atomics.  Results are
 *   bit-identical from run to run and across layouts, and entry (i, j) depends
 *   on x_i and y_j alone: it equals the s = r = 1 call on those two clouds bit
 *   for bit, wherever they stand in the sets.  The float64 accumulation keeps
 *   the result within 1 ulp of float32(exact sum / n) whatever the order.
 * mean21 == NULL skips that direction and changes no bit of mean12.
 * layout1 / layout2: 0 = [., n, 3] rows, 1 = [., 3, n] channel planes; clouds
 *   are read in place.
 * Non-finite input: an entry whose cloud pair holds a non-finite coordinate is
 *   unspecified but written; every other entry is unaffected, bit for bit; the
 *   call always returns.
 * Validation, before any device call: negative sizes or a layout outside
 *   {0, 1} -> PCM_ERR_INVALID_ARG; then s == 0 or r == 0 is a no-op (PCM_OK,
 *   also with null pointers); n == 0 or m == 0, a null cloud or a null mean12
 *   -> PCM_ERR_INVALID_ARG; n or m above PCM_CROSS_MAX_POINTS, or s r or the
 *   grid beyond the launch limits (2^31 - 1) -> PCM_ERR_UNSUPPORTED, nothing
 *   launched; a workspace that is NULL or shorter than
 *   pcm_chamfer_cross_workspace_bytes(s, r, n, m) -> PCM_ERR_WORKSPACE; one not
 *   8-byte aligned -> PCM_ERR_INVALID_ARG.
 * The workspace (one float64 record per entry, direction and workgroup of a
 *   query cloud) needs no initialisation and keeps no state;
 *   pcm_chamfer_cross_workspace_bytes is 0 for empty problems.
 * Launches on `stream`: at most two -- the scan of both directions, then, only
 *   if a cloud spans several workgroups (more than 1024 points), a finalise
 *   that adds the partial records in ascending order (the hand-off is the
 *   kernel boundary, as in pcm_chamfer_eval).  Capturable: no host
 *   synchronisation, no allocation, nothing read back, no waiting between
 *   workgroups.
 */
size_t pcm_chamfer_cross_workspace_bytes(int s, int r, int n, int m);
int pcm_chamfer_cross(const float *xyz1 /* s clouds of n points */, const float *xyz2 /* r clouds of m points */,
                      int s, int r, int n, int m, int layout1, int layout2,
                      float *mean12 /* [s, r] */, float *mean21 /* NULL or [s, r] */,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* N-D Chamfer distance (1 to 8 coordinates a point)                       */
/* ---------------------------------------------------------------------- */

/* Most coordinates a point may have (else PCM_ERR_UNSUPPORTED). */
#define PCM_CHAMFER_ND_MAX_DIM 8
/* Largest cloud (points) the N-D entries take (else PCM_ERR_UNSUPPORTED). */
#define PCM_CHAMFER_ND_MAX_POINTS 16384

/*
 * N-D Chamfer distance (extension; upstream ChamferDistancePytorch ships
 * chamfer2D / 3D / 5D / 6D): nearest neighbour with argmin in both directions,
 * and a deterministic backward, for float32 clouds x1 [b, n, D] and
 * x2 [b, m, D], 1 <= D = dim <= PCM_CHAMFER_ND_MAX_DIM.
 * layout1 / layout2: 0 = contiguous rows [b, n, D], 1 = contiguous channel
 *   planes [b, D, n]; clouds are read in place.
 *
 * Forward, direction 1 (direction 2 is the same with the roles swapped).  For
 * query j and candidate k, every step in float32:
 *     c_t = x2[k][t] - x1[j][t]
 *     s   = c_0 * c_0                       (a rounded product)
 *     s   = fmaf(c_t, c_t, s)               for t = 1 .. D-1
 *   At D = 3 this is the library's pinned fmaf(dz,dz,fmaf(dy,dy,dx*dx)).
 *     key_k    = s, or +inf if s is NaN
 *     dist1[j] = min_k key_k
 *     idx1[j]  = the lowest k with key_k == dist1[j]
 *   So a NaN never wins; a query or candidate cloud that yields no finite key
 *   gives (+inf, 0); ties go to the lowest index wherever the tied candidates
 *   stand.  This is simpler than pcm_chamfer_forward's 512-point-tile NaN rule;
 *   the two agree, bit for bit, on every input whose distances are all non-NaN.
 *   m == 0 leaves dist1 / idx1 untouched and n == 0 leaves dist2 / idx2
 *   untouched, as pcm_chamfer_forward does; b == 0 is a no-op.
 *
 * Backward: the order of pcm_chamfer_backward, per coordinate t.  With
 * g = graddist * 2.f:
 *     grad1[i] = ((+0 + direct) + s_j0) + s_j1 + ...   over the cloud-2 points
 *                j with idx2[j] == i, ascending
 *     grad2[k] = ((+0 + s_j0) + s_j1 + ...) + direct   over the cloud-1 points
 *                j with idx1[j] == k, ascending, the direct term last
 *     direct_t = g_self * (p_t - q_t),     p the point itself, q = other[idx_self]
 *     s_j,t    = -(g_j * (p'_t - q_t)),    p' = other[j], q the point itself
 *   Every operation is a separate float32 rounding; no float atomics: results
 *   are bit-identical from run to run.  Gradients are fully overwritten and
 *   written in their cloud's layout.  graddist1 [b, n], graddist2 [b, m],
 *   idx1 [b, n] and idx2 [b, m] are contiguous.  n, m > 0 are required, and
 *   every index must lie inside the cloud it points into (an index outside is
 *   never followed, and the gradients it touches are unspecified).
 *
 * Validation, before any device call: negative sizes, dim < 1 or a layout
 *   outside {0, 1} -> PCM_ERR_INVALID_ARG; dim > PCM_CHAMFER_ND_MAX_DIM or a
 *   cloud above PCM_CHAMFER_ND_MAX_POINTS -> PCM_ERR_UNSUPPORTED; then b == 0
 *   (forward: also n == 0 or m == 0) is a no-op (PCM_OK, also with null
 *   pointers); backward with n == 0 or m == 0, or any null pointer ->
 *   PCM_ERR_INVALID_ARG.
 * Caller-owned buffers, no workspace, no allocation, no synchronisation; one
 *   launch each on `stream`; capturable; no waiting between workgroups.
 */
int pcm_chamfer_nd_forward(const float *x1, const float *x2, int b, int n, int m, int dim,
                           int layout1, int layout2, float *dist1, float *dist2,
                           int32_t *idx1, int32_t *idx2, void *stream);
int pcm_chamfer_nd_backward(const float *x1, const float *x2, int b, int n, int m, int dim,
                            int layout1, int layout2, const float *graddist1, const float *graddist2,
                            const int32_t *idx1, const int32_t *idx2,
                            float *grad1, float *grad2, void *stream);

/* ---------------------------------------------------------------------- */
/* Projection loss (finetune.py:154-162)                                   */
/* ---------------------------------------------------------------------- */

/* Largest grid_h / grid_w of the silhouette entries (else PCM_ERR_UNSUPPORTED). */
#define PCM_SILHOUETTE_MAX_GRID 128
/* Longest sequential chain of float32 additions behind pcm_proj_bce's
 * loss_out for any count <= 2^20 (see the summation order below). */
#define PCM_PROJ_BCE_CHAIN 30

/*
 * Gaussian-splatted silhouette of a point cloud (extension): cont_proj of
 * utils/projection.py:4-67, which materialises a B x N x H x W x 2 float32
 * difference tensor, its exponential (apply_kernel, :97-108), a B x N x H x W
 * product and a sum over N (on the CPU, utils/utils.py:232), as one launch
 * that keeps nothing of size N x H x W anywhere.
 *
 * Contract.  Coordinate map, float32, as projection.py:20-21:
 *     gx = ((px + 1.f) * (float)grid_h) / 2.f     (row index h: first coordinate)
 *     gy = ((py + 1.f) * (float)grid_w) / 2.f     (column w: second coordinate)
 *   pz is never read.  Coordinates outside (-1, 1) are legal (their terms
 *   underflow).  For 0 <= h < grid_h, 0 <= w < grid_w:
 *     sil[b,h,w] = sum_n ex[n,h] * ey[n,w],
 *     ex[n,h] = exp(-(gx_n - h)^2 / (2 sigma_sq)), ey[n,w] likewise with gy_n, w
 *   (grid_h + grid_w exponentials per point, each one hardware exp2 of
 *   (d * d) * fl(-log2(e) / (2 sigma_sq)); products that would be denormal
 *   may be flushed to zero).
 *   Summation order of every cell: with the points in chunks of 128, eight
 *   sequential partial sums -- partial k takes points 128 c + 16 k + j,
 *   c ascending, then j = 0..15 ascending, each term added by one fused
 *   multiply-add -- and then ((p0 + p1) + p2) + .. + p7.  It depends on n
 *   alone: deterministic run to run, no float atomics, and cloud i evaluated
 *   alone (b = 1) equals cloud i of any batch bit for bit.
 *   Non-finite inputs, as the reference's sum: a NaN px or py makes every cell
 *   of that cloud NaN; +-inf px or py contributes 0; pz changes nothing.
 *   Every element of sil [b, grid_h, grid_w] is written.
 * pcm_silhouette_backward: with G = grad_sil [b, grid_h, grid_w] (dL/dsil),
 *     gradxyz[b,n,0] = (grid_h / 2) sum_h (-(gx_n - h) / sigma_sq) ex[n,h] (sum_w G[b,h,w] ey[n,w])
 *     gradxyz[b,n,1] = (grid_w / 2) sum_w (-(gy_n - w) / sigma_sq) ey[n,w] (sum_h G[b,h,w] ex[n,h])
 *     gradxyz[b,n,2] = 0 exactly
 *   (autograd's backward of the sum above).  Order: per row h the columns in
 *   slices of eight (pairwise inside a slice), rows ascending, then the slices
 *   ascending; it depends on the grid alone.  Fully overwritten, no atomics.
 *   Its result for a point with a non-finite coordinate is unspecified for
 *   that point; all other points are unaffected.
 * layout: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, as
 *   pcm_chamfer_forward_layout: read in place, and gradxyz is written in the
 *   same layout.  perspective_transform returns such a view of planes
 *   (projection.py:146), and that is what cont_proj receives.
 * Validation, before any device call: b < 0, n < 0, a layout outside {0, 1},
 *   grid_h < 1 or grid_w < 1, sigma_sq not finite or <= 0 ->
 *   PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK); n == 0 or a null
 *   pointer with b > 0 -> PCM_ERR_INVALID_ARG; grid_h or grid_w above
 *   PCM_SILHOUETTE_MAX_GRID -> PCM_ERR_UNSUPPORTED.
 */
int pcm_silhouette_forward(const float *xyz, int b, int n, int layout, int grid_h, int grid_w,
                           float sigma_sq, float *sil /* [b,grid_h,grid_w] */, void *stream);
int pcm_silhouette_backward(const float *xyz, int b, int n, int layout, int grid_h, int grid_w,
                            float sigma_sq, const float *grad_sil, float *gradxyz /* xyz's layout */, void *stream);

/*
 * Projection loss 'bce_prob' (extension): loss/proj_loss.py:17-19 and the mean
 * of :43 -- six elementwise torch kernels and a reduction in the reference --
 * with the gradient for pred from the same launch.  pred, gt, grad_pred hold
 * `count` contiguous float32 elements.  Per element, in float32 and in this order:
 *     a = pred + 1e-8f
 *     c = fabsf((1.f - pred) - 1e-8f)
 *     term = ((-gt) * logf(a)) * w - (1.f - gt) * logf(c)
 *   loss_out[0] = sum(term) / (float)count                       (device float)
 *   grad_pred[i] (nullable) = (-gt w / a + (1 - gt) / ((1.f - pred) - 1e-8f)) / (float)count,
 *     the gradient of that mean with respect to pred; the two quotients can
 *     cancel, so they are formed and added in double and rounded once.
 * Summation order: workgroup k owns elements [2048 k, 2048 k + 2048); thread t
 *   of 256 adds elements t, t + 256, .., t + 1792 in order (chain 8); a wave's
 *   64 sums are added by six DPP steps (shift by 1, 2, 4, 8 lanes, then rows
 *   16 and 32: chain 6); the four waves in ascending order (4).  A single
 *   workgroup (count <= 2048) divides and stores.  Otherwise its partial goes
 *   to the workspace and a second launch of one workgroup adds them: thread t
 *   adds partials t, t + 256, .. in order (chain ceil(blocks / 256), 2 at
 *   count = 2^20), then wave and workgroup as before (6 + 4).  Longest chain:
 *   L = 18 + ceil(ceil(count / 2048) / 256) + 10 = PCM_PROJ_BCE_CHAIN for
 *   2^19 < count <= 2^20, less below.  Deterministic, no float atomics.
 * The workspace (pcm_proj_bce_workspace_bytes(count) bytes, at least 128 for
 *   count > 0) needs no initialisation and holds no state between calls.
 * Validation, before any device call: count < 0 -> PCM_ERR_INVALID_ARG;
 *   count == 0 is a no-op (PCM_OK); a null pred / gt / loss_out ->
 *   PCM_ERR_INVALID_ARG; a workspace that is NULL or too short ->
 *   PCM_ERR_WORKSPACE.
 */
size_t pcm_proj_bce_workspace_bytes(long long count);
int pcm_proj_bce(const float *pred, const float *gt, long long count, float w, float *loss_out,
                 float *grad_pred /* nullable */, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Farthest point sampling (utils/datasets_sample_pcl.py:87-94)            */
/* ---------------------------------------------------------------------- */

/* Largest cloud (points per batch element) pcm_fps takes (else PCM_ERR_UNSUPPORTED). */
#define PCM_FPS_MAX_POINTS 16384

/*
 * Farthest point sampling (extension): farthest_point_sample and index_points
 * of utils/utils.py:316-360 -- npoint dependent iterations of 21 small device
 * kernels each (torch.profiler's count), with a boolean-mask assignment that synchronises with the host
 * -- as ONE launch of one workgroup per cloud, the running minima in registers.
 *
 * Contract.  Per cloud p[0..n), with far = start and run[k] = 1e10f for every
 * k, repeat for i = 0 .. npoint - 1:
 *     idx_out[b,i] = far
 *     for every k:  d = fmaf(dz,dz,fmaf(dy,dy,dx*dx)), (dx,dy,dz) = p[k] - p[far]
 *                   (the library's pinned order, as pcm_chamfer_forward);
 *                   run[k] = d only if d < run[k]
 *                   (a NaN distance never changes a running minimum)
 *     far = the lowest k that attains max_k run[k]
 *   Consequences: running minima are never NaN and every index is in [0, n)
 *   for any input bits; npoint > n is legal and follows the same rule (once
 *   every point of a cloud of distinct finite points is taken, index 0
 *   repeats); a point with a NaN coordinate keeps run = 1e10f and, once it is
 *   the lowest such point, repeats for the rest of the call.
 *   Squared distances of 1e10 and above (coordinates around 1e5) never lower
 *   the 1e10f start value: the points they leave saturated all attain the
 *   maximum, so the seeds follow index order among the saturated points, as
 *   the reference's do (tests/test_geometry_gpu.py pins this on a cloud
 *   scaled by 2e5).
 *   The reference forms d as a torch sum of three squares; where its winner
 *   beats the runner-up by more than a few float32 ulps, or ties it exactly,
 *   the indices are the same.
 *   sampled_out (nullable) [b, npoint, 3], always contiguous rows: p[idx_out[b,i]]
 *   bit for bit, from the same launch.  idx_out [b, npoint] int64, as the
 *   reference's torch.long centroids.  Every element of both is written.
 * layout: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, read in place as
 *   pcm_chamfer_forward_layout does.  start: the first index of every cloud
 *   (the reference draws it from torch.randint(0, 1) or (1, 2): 0 or 1).
 * No workspace, no allocation, no host synchronisation: one launch on `stream`,
 *   capturable.  Deterministic; b is limited only by the grid.
 * Validation, before any device call: b < 0, n < 0, npoint < 0 or a layout
 *   outside {0, 1} -> PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK, also
 *   with null pointers); n == 0 or npoint == 0, start < 0 or start >= n, a null
 *   xyz or idx_out -> PCM_ERR_INVALID_ARG; n above PCM_FPS_MAX_POINTS ->
 *   PCM_ERR_UNSUPPORTED.
 */
int pcm_fps(const float *xyz, int b, int n, int layout, int npoint, int start,
            int64_t *idx_out /* [b, npoint] */, float *sampled_out /* [b, npoint, 3] or NULL */,
            void *stream);

/* ---------------------------------------------------------------------- */
/* k nearest neighbours and the repulsion loss                             */
/* ---------------------------------------------------------------------- */

/* Longest list pcm_knn returns (else PCM_ERR_UNSUPPORTED). */
#define PCM_KNN_MAX_K 32
/* Largest cloud (points per batch element), query or reference, that pcm_knn
 * and pcm_repulsion_loss take (else PCM_ERR_UNSUPPORTED). */
#define PCM_KNN_MAX_POINTS 16384

/*
 * k nearest neighbours (extension): the knn_cuda.KNN the reference's loss class
 * was written around (the commented-out KNN(k=2) / KNN(k=20) members of
 * loss/loss.py:16-17) as ONE launch, every query's list kept in registers.
 *
 * Contract.  For cloud bi and query i, candidate j (0 <= j < m) has
 *     d = fmaf(dz,dz,fmaf(dy,dy,dx*dx)), (dx,dy,dz) = ref[bi,j] - query[bi,i]
 *   (the library's pinned order, as pcm_chamfer_forward).
 *   dist_out[bi,i,0..k) / idx_out[bi,i,0..k) are the k smallest pairs (d, j) in
 *   lexicographic order -- d compared with '<', equal d broken by the lower j
 *   -- in ascending slots; slot 0 is therefore exactly dist1 / idx1 of
 *   pcm_chamfer_forward on finite clouds.
 *   A candidate whose d is NaN or +inf is never listed.  Slots left without a
 *   candidate hold (+inf, -1): when m < k, when candidates are non-finite, or
 *   when the query is.  Nothing is excluded: in a self search (the same
 *   pointer passed twice) a point lists itself.
 *   Every element of both outputs is written; distances are SQUARED.
 * layout_q / layout_r: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, each
 *   cloud read in place as pcm_chamfer_forward_layout does.
 * No workspace, no allocation, no host synchronisation, no atomics and no
 *   waiting between workgroups: one launch on `stream`, capturable.
 *   Deterministic; b is limited only by the grid.
 * Validation, before any device call: negative sizes, a layout outside {0, 1}
 *   or k < 1 -> PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK, also with
 *   null pointers); n == 0, m == 0 or a null pointer -> PCM_ERR_INVALID_ARG;
 *   k above PCM_KNN_MAX_K, or n or m above PCM_KNN_MAX_POINTS ->
 *   PCM_ERR_UNSUPPORTED: nothing is launched and the outputs are left alone.
 */
int pcm_knn(const float *query, const float *ref, int b, int n, int m, int layout_q, int layout_r, int k,
            float *dist_out /* [b, n, k] */, int32_t *idx_out /* [b, n, k] */, void *stream);

/*
 * Repulsion loss (extension): PU-GAN's point-distribution regulariser, the
 * get_repulsion_loss the reference's loss class once had, with its gradient
 * from the same call (the reference's ran knn_cuda under torch.no_grad() and
 * could train nothing).
 *
 * Contract.  With (d[i,t], j[i,t]) slot t of point i's pcm_knn list (k = 5) in
 * its own cloud, searched against itself:
 *     loss_out[0] = (1 / (4 b n)) sum_bi sum_i sum_{t=1..4} max(0, h - d[i,t])
 *   Slot 0 is skipped whatever it holds (the reference's dist[:, :, 1:5]); a
 *   +inf slot contributes 0.  Each term h - d is formed in float32; the terms
 *   are added in double in a fixed order (a point's four slots ascending, the
 *   six DPP steps of a wave of 64 points, the waves' partials ascending in
 *   strides of 64, then the six DPP steps again),
 *   scaled by 1 / (4 b n) in double and rounded once.
 *   gradxyz (nullable; xyz's shape AND layout): the full gradient.  Every
 *   active term (h - d > 0) at (i, j) adds -(2 / (4 b n)) (p_i - p_j) to point i
 *   and +(2 / (4 b n)) (p_i - p_j) to point j, so a point collects from its own
 *   list and from every list it appears in.  Per component it is
 *   fl(2 / (4 b n)) * a, where a is a float32 sum of (p_other - p_i) in a
 *   fixed order: four partial sums, partial w over the points s with
 *   (s mod 1024) div 256 == w whose active slots name the point, s ascending
 *   (partial 0 begins with the point's own active slots 1..4, ascending),
 *   then ((a0 + a1) + a2) + a3.  No float atomics: bit-identical from run to
 *   run.  Fully overwritten.
 * layout: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, read in place.
 * Three launches on `stream`, capturable; no host synchronisation.  The
 *   workspace (pcm_repulsion_workspace_bytes(b, n) bytes, 8-byte aligned)
 *   holds the lists; it needs no initialisation and keeps no state.
 * Validation, before any device call: b < 0, n < 0, a layout outside {0, 1} or
 *   h not finite -> PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK;
 *   loss_out is not written: the mean over nothing is the caller's to define);
 *   n < 5, a null xyz or loss_out, a misaligned workspace ->
 *   PCM_ERR_INVALID_ARG; n above PCM_KNN_MAX_POINTS -> PCM_ERR_UNSUPPORTED; a
 *   workspace that is NULL or too short -> PCM_ERR_WORKSPACE.
 */
size_t pcm_repulsion_workspace_bytes(int b, int n);
int pcm_repulsion_loss(const float *xyz, int b, int n, int layout, float h, float *loss_out /* 1 float */,
                       float *gradxyz /* NULL, or xyz's layout */, void *workspace, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Ball query, grouping and the uniform loss                               */
/* ---------------------------------------------------------------------- */

/* Longest list pcm_ball_query returns, and longest group of one scale of
 * pcm_uniform_loss (else PCM_ERR_UNSUPPORTED). */
#define PCM_BALL_MAX_NSAMPLE 64
/* Most scales (radii) one pcm_uniform_loss call takes. */
#define PCM_UNIFORM_MAX_SCALES 8

/*
 * Ball query (extension): pointnet2's ball_query, which the reference's dropped
 * get_uniform_loss called through pointnet2_ops, as ONE launch.
 * pointnet2_ops is not installed where this library was written and could not
 * be fetched: the rule below -- in particular the padding -- is pointnet2's
 * published one, stated from its source; it is NOT verified against that
 * library.  This text is the contract.
 *
 * Contract.  For cloud bi and centre c, point k (0 <= k < n) has
 *     d = fmaf(dz,dz,fmaf(dy,dy,dx*dx)), (dx,dy,dz) = xyz[bi,k] - new_xyz[bi,c]
 *   (the library's pinned order, as pcm_knn), and r2 = radius * radius, rounded
 *   once to float32.  Point k is a hit iff d < r2: a NaN d is never a hit and a
 *   point at exactly r2 is outside.  With h_0 < h_1 < ... the hits in ascending
 *   k and c_n = min(number of hits, nsample):
 *     idx_out[bi,c,t] = h_t for t < c_n;
 *     every remaining slot holds h_0 (pointnet2's padding: the first hit
 *       repeated); with no hit every slot holds 0 (its zero-initialised output);
 *     cnt_out[bi,c] = c_n (cnt_out is nullable).
 *   A group is the first nsample hits IN INDEX ORDER, not the nearest ones.
 *   Every element of both outputs is written and every index is in [0, n) for
 *   any input bits.
 * layout_xyz / layout_new: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes,
 *   each cloud read in place as pcm_knn does.
 * No workspace, no allocation, no host synchronisation, no atomics and no
 *   waiting between workgroups: one launch on `stream`, capturable.
 *   Deterministic; b is limited only by the grid.
 * Validation, before any device call: negative sizes, a layout outside {0, 1},
 *   nsample < 1 or a radius that is not finite and positive ->
 *   PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK, also with null
 *   pointers); n == 0, s == 0 or a null xyz, new_xyz or idx_out ->
 *   PCM_ERR_INVALID_ARG; nsample above PCM_BALL_MAX_NSAMPLE or n above
 *   PCM_KNN_MAX_POINTS -> PCM_ERR_UNSUPPORTED: nothing is launched and the
 *   outputs are left alone.
 */
int pcm_ball_query(const float *xyz, const float *new_xyz, int b, int n, int s, int layout_xyz, int layout_new,
                   float radius, int nsample, int32_t *idx_out /* [b, s, nsample] */,
                   int32_t *cnt_out /* [b, s] or NULL */, void *stream);

/*
 * Uniform loss (extension): PU-GAN's other point-distribution regulariser, the
 * get_uniform_loss the reference's loss class once had, with its full gradient
 * from the same call.  nsample, ball_radius and weight are HOST arrays of
 * nscales entries, read before the call returns (they travel as kernel
 * arguments).
 *
 * Contract.
 *   Seeds: seed[bi, 0..npoint) are pcm_fps's indices of cloud bi with start = 0.
 *   Groups: for scale q and seed s, G[0..nsample[q]) is pcm_ball_query's list
 *   around p[seed] in the seed's own cloud with radius ball_radius[q] (the
 *   same unverified padding rule).  groups_out (nullable) receives them:
 *   row (bi, s) holds the lists of scale 0, 1, .. one after the other.
 *   For slot t of a group: the pcm_knn distances (pinned order, p[G_v] - p[G_t])
 *   to every slot v of the group, v = t included; the pairs (distance, v) in
 *   lexicographic order; e_t is the distance of the second-smallest pair and
 *   v* its slot -- exactly slot 1 of pcm_knn(k = 2) on the group, with its
 *   rules that a NaN or +inf distance is never listed and an unfilled slot is
 *   +inf.  root_t = sqrtf(e_t), correctly rounded; u_t = root_t + 1e-8f in
 *   float32 (the reference's abs is then a no-op).  From here in double:
 *     m = (sum_t u_t) / nsample[q];  term = (m - L)^2 / (L + 1e-8), L = expect_len;
 *     loss_out[0] = sum_q weight[q] (sum_{bi,s} term) / (b npoint), rounded once.
 *   Fixed order of the sums: a seed's slots are numbered (first slot of q) + t,
 *   S = sum_q nsample[q] in all, and taken 64 at a time, lane = number mod 64; a
 *   group's u_t among them are added by the six DPP steps of a wave (the other
 *   lanes hold 0) and the passes' sums ascending;
 *   a seed's weight[q] * term over q ascending; of the seeds'
 *   sums, numbered bi * npoint + s, thread t of 1024 adds t, t + 1024, ..
 *   ascending, every wave its 64 threads by the six DPP steps, and the sixteen
 *   waves' sums are added ascending; the division by b npoint last.
 *   gradxyz (nullable; xyz's shape AND layout), fully overwritten: seeds, ball
 *   membership and the choice of neighbour carry no gradient.  With
 *     c = weight[q] 2 (m - L) / ((L + 1e-8) b npoint nsample[q])   (double),
 *   every slot t with 0 < e_t < inf contributes g = fl(c) * ((p_i - p_j) / root_t)
 *   (float32 throughout) to point i = G_t and -g to point j = G_{v*}.  A slot
 *   with e_t == 0 (a padding copy, coincident points) contributes nothing: the
 *   subgradient, where the reference's would be infinite.  A point that fills
 *   several slots collects from each.  No float atomics: the slots' records
 *   (i, j, g) of a cloud are numbered r = (s * S + first slot of q + t) and a
 *   point's gradient is a float32 sum of four partial
 *   sums, partial w over the records r with (r mod 1024) div 256 == w that
 *   name the point, r ascending, +g as point i before -g as point j, then
 *   ((a0 + a1) + a2) + a3: bit-identical from run to run.
 *   Non-finite input: the call returns and every index written is in range;
 *   the loss follows IEEE from the rules above (it may be inf or NaN); the
 *   gradient is then unspecified.
 * layout: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, read in place.
 * Four launches on `stream` (three without gradxyz), capturable; no host
 *   synchronisation and no waiting between workgroups.  The workspace
 *   (pcm_uniform_workspace_bytes bytes, 8-byte aligned) holds the seeds and
 *   the records; it needs no initialisation and keeps no state.
 * Validation, before any device call: b < 0, n < 0, a layout outside {0, 1},
 *   nscales outside [1, PCM_UNIFORM_MAX_SCALES], a null host array,
 *   npoint < 1, any nsample[q] < 2, a ball_radius, weight or expect_len that
 *   is not finite, a ball_radius or expect_len that is not positive ->
 *   PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK; loss_out is not
 *   written); n == 0, a null xyz or loss_out, a misaligned workspace ->
 *   PCM_ERR_INVALID_ARG; any nsample[q] above PCM_BALL_MAX_NSAMPLE or n above
 *   PCM_KNN_MAX_POINTS -> PCM_ERR_UNSUPPORTED; a workspace that is NULL or too
 *   short -> PCM_ERR_WORKSPACE.
 * pcm_uniform_workspace_bytes: 0 when b, n or npoint is not positive or the
 *   scales would be rejected as invalid arguments.
 */
size_t pcm_uniform_workspace_bytes(int b, int n, int npoint, int nscales, const int *nsample);
int pcm_uniform_loss(const float *xyz, int b, int n, int layout, int npoint, int nscales, const int *nsample,
                     const float *ball_radius, const double *weight, double expect_len,
                     float *loss_out /* 1 float */, float *gradxyz /* NULL, or xyz's layout */,
                     int32_t *groups_out /* NULL, or [b, npoint, sum_q nsample[q]] */, void *workspace,
                     size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Kernel-norm (MMD) losses: Gaussian, Laplacian, energy distance          */
/* ---------------------------------------------------------------------- */

#define PCM_KERNEL_GAUSSIAN 0
#define PCM_KERNEL_LAPLACIAN 1
#define PCM_KERNEL_ENERGY 2
/* Largest cloud (points per batch element) pcm_kernel_loss takes (else
 * PCM_ERR_UNSUPPORTED). */
#define PCM_KERNEL_LOSS_MAX_POINTS 16384

/*
 * Kernel norm of two unweighted clouds (extension): what geomloss's
 * SamplesLoss(loss='gaussian' | 'laplacian' | 'energy') computes, which the
 * reference's batch_EMD_loss (loss/loss_.py:111-120) calls once per cloud with
 * loss='gaussian'.  geomloss is not installed where this library was written
 * and could not be fetched: the formulas below are the published ones and are
 * NOT verified against that package.  This text is the contract.
 *
 * Contract.  Per batch element, cloud x = xyz1[bi] has n points of weight
 *   a = 1/n and cloud y = xyz2[bi] has m points of weight b = 1/m:
 *     loss_out[bi] = 1/2 sum_{i,i'} a a k(x_i,x_i') + 1/2 sum_{j,j'} b b k(y_j,y_j')
 *                    - sum_{i,j} a b k(x_i,y_j)
 *   (the diagonal pairs i = i', j = j' included).  For a pair (p, q), with
 *   (dx,dy,dz) = p - q in float32, d2 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)) (the
 *   library's pinned order), r = sqrtf(d2) correctly rounded, sigma = blur:
 *     PCM_KERNEL_GAUSSIAN   k = exp2(d2 * c), c = fl(-log2(e) / (2 sigma^2)),
 *                           one hardware exp2 (as pcm_silhouette_forward's);
 *     PCM_KERNEL_LAPLACIAN  k = exp2(r * c),  c = fl(-log2(e) / sigma);
 *     PCM_KERNEL_ENERGY     k = -r (blur is checked but not used).
 *   c is formed in double from the float blur and rounded once.  There is no
 *   clamp on r: a coincident pair has r = 0 exactly (geomloss's dense path
 *   clamps the squared distance at 1e-8: a documented deviation).
 *   Row sums.  Every point p ("row") of either cloud gets, against its own
 *   cloud and against the other one, the float32 sums S = sum_q k(p,q) and
 *   V = sum_q g(p,q) (p - q) with g = k (Gaussian), k / r (Laplacian), 1 / r
 *   (energy) -- the divisions correctly rounded, g = 0 where r = 0 (the
 *   subgradient: a coincident pair adds nothing to a gradient, the rule of
 *   pcm_uniform_loss) -- each term entering V by one fmaf per component.
 *   Order of a row sum over a cloud of c points: eight partial sums, partial w
 *   over the points q with (q mod 1024) div 128 == w, q ascending, from 0;
 *   then (((s0 + s1) + s2) + ..) + s7.  The longest float32 chain behind a row
 *   sum is
 *     chain(c) = 128 floor(c / 1024) + min(128, c mod 1024) + 7
 *   additions, and chain(n, m) = max(chain(n), chain(m)): 135 at 1024 points,
 *   2055 at 16384.
 *   loss_out[bi]: in double, row r of the concatenation x || y (weight w_r, the
 *   other cloud's w_o) contributes 1/2 w_r (w_r S_own - w_o S_other); thread t
 *   of 256 adds rows t, t + 256, .. ascending, every wave its 64 threads by the
 *   six DPP steps, the four waves' sums ascending; rounded once to float32.
 *   gradxyz1 / gradxyz2 (each nullable on its own; the cloud's shape AND
 *   layout; fully overwritten): the gradient of loss_out[bi] with unit upstream
 *   gradient, per component fmaf(fl(C w_r w_r), V_own, fl(-C w_r w_o) * V_other)
 *   with C = -1/sigma^2 (Gaussian), -1/sigma (Laplacian), -1 (energy), the two
 *   coefficients formed in double and rounded once.  A cloud whose gradient
 *   pointer is NULL gets no V sums (with both NULL none are formed); loss_out
 *   and the other gradient do not change by a bit.
 *   No float atomics; the order of every sum depends on (n, m) alone: results
 *   are bit-identical from run to run, and element bi of a batch equals the
 *   same clouds evaluated alone (b = 1) bit for bit.
 *   Non-finite input: a NaN coordinate makes loss_out of ITS element NaN and
 *   leaves the other elements' outputs untouched; that element's gradients are
 *   unspecified.  The call always returns.
 * layout1 / layout2: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, each
 *   cloud read in place and its gradient written in the same layout.
 * Two launches on `stream`, capturable; no host synchronisation, no
 *   allocation, no waiting between workgroups.  The workspace
 *   (pcm_kernel_loss_workspace_bytes(b, n, m) bytes, 8-byte aligned) holds the
 *   rows' two S sums; it needs no initialisation and keeps no state.
 * Validation, before any device call: negative sizes, a layout outside {0, 1},
 *   a kernel outside 0..2, a blur that is not finite or not positive (for the
 *   energy distance too) -> PCM_ERR_INVALID_ARG; then b == 0 is a no-op
 *   (PCM_OK, also with null pointers); n == 0, m == 0, a null cloud or
 *   loss_out -> PCM_ERR_INVALID_ARG; n or m above PCM_KERNEL_LOSS_MAX_POINTS
 *   (or b beyond the grid) -> PCM_ERR_UNSUPPORTED: nothing is launched; a
 *   workspace that is NULL or too short -> PCM_ERR_WORKSPACE; a misaligned one
 *   -> PCM_ERR_INVALID_ARG.
 * pcm_kernel_loss_workspace_bytes: 0 when b, n or m is not positive.
 */
size_t pcm_kernel_loss_workspace_bytes(int b, int n, int m);
int pcm_kernel_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2, int kernel,
                    float blur, float *loss_out /* [b] */, float *gradxyz1 /* NULL or xyz1's shape and layout */,
                    float *gradxyz2 /* NULL or xyz2's shape and layout */, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ---------------------------------------------------------------------- */
/* Sinkhorn divergence (debiased, balanced, p = 2, uniform weights)        */
/* ---------------------------------------------------------------------- */

/* Largest cloud (points per batch element) pcm_sinkhorn_loss takes and the
 * longest epsilon schedule it runs (else PCM_ERR_UNSUPPORTED). */
#define PCM_SINKHORN_MAX_POINTS 16384
#define PCM_SINKHORN_MAX_STEPS 128

/*
 * Debiased Sinkhorn divergence of two unweighted clouds (extension): what
 * geomloss's SamplesLoss(loss='sinkhorn', p=2, debias=True) computes for
 * uniform weights.  geomloss is not installed where this library was written
 * and could not be fetched: the algorithm below is the published one
 * (sinkhorn_loop: symmetric averaged updates, epsilon-scaling, a last
 * extrapolation step) and is NOT verified against that package.  This text is
 * the contract.
 *
 * Contract.  Per batch element, cloud x = xyz1[bi] has n points of weight
 *   a = 1/n and cloud y = xyz2[bi] has m points of weight b = 1/m; la = log a,
 *   lb = log b.  Cost of a pair (p, q): C = d2 / 2 with (dx,dy,dz) = p - q in
 *   float32 and d2 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)) (the library's pinned
 *   order).  softmin_eps(C, h)_i = -eps log sum_j exp(h_j - C_ij / eps).
 *   Schedule (pcm_sinkhorn_schedule; host only, in double, no device call):
 *   with D = diameter, s = scaling:  eps_0 = D^2;  eps_k = exp(2 ln D +
 *   (k - 1) 2 ln s) for k = 1, 2, .. while 2 ln D + (k - 1) 2 ln s > 2 ln blur
 *   (so eps_1 = eps_0, the published list's duplicate);  a last entry blur^2.
 *   blur 0.05, scaling 0.5, D = sqrt(3) give T = 8 entries: 3, 3, 0.75, 0.1875,
 *   0.046875, 0.01171875, 0.0029296875, 0.0025.  The function returns T and
 *   fills eps_out[0..T) when eps_out is not NULL and capacity >= T.  A negative
 *   return is a pcm_status: blur, scaling or diameter not finite, blur <= 0,
 *   diameter <= 0, scaling outside (0, 1) -> PCM_ERR_INVALID_ARG; T above
 *   PCM_SINKHORN_MAX_STEPS -> PCM_ERR_UNSUPPORTED.
 *   Iteration.  At eps_0:  f_ba = softmin(C_xy, lb), g_ab = softmin(C_yx, la),
 *   f_aa = softmin(C_xx, la), g_bb = softmin(C_yy, lb).  Then for every eps of
 *   the schedule in order, all four from the OLD values,
 *     ft_ba = softmin_eps(C_xy, lb + g_ab / eps),  gt_ab = softmin_eps(C_yx, la + f_ba / eps),
 *     ft_aa = softmin_eps(C_xx, la + f_aa / eps),  gt_bb = softmin_eps(C_yy, lb + g_bb / eps),
 *   and each potential becomes the mean 0.5 (old + new).  Last, at eps = blur^2,
 *   one extrapolation without averaging, again from the old values:
 *     F_ba = softmin(C_xy, lb + g_ab / eps),  G_ab = softmin(C_yx, la + f_ba / eps),
 *     F_aa = softmin(C_xx, la + f_aa / eps),  G_bb = softmin(C_yy, lb + g_bb / eps).
 *   loss_out[bi] = sum_i a (F_ba,i - F_aa,i) + sum_j b (G_ab,j - G_bb,j): in
 *   double, row r of the concatenation x || y contributes w_r (F_cross - F_own)
 *   in pcm_kernel_loss's fixed order (thread t of 256 adds rows t, t + 256, ..
 *   ascending, every wave its 64 threads by the six DPP steps, the four waves'
 *   sums ascending); rounded once to float32.
 *   Gradients: of loss_out[bi] with unit upstream gradient, from the
 *   extrapolation step with the averaged potentials (and the column points)
 *   held fixed -- the envelope rule:
 *     gradxyz1[i] = a (sum_k Q_ik x_k - sum_j P_ij y_j),
 *   P_i. the softmax over j of (lb + g_ab / eps - C_xy / eps), Q_i. the softmax
 *   over k of (la + f_aa / eps - C_xx / eps); gradxyz2 with the roles swapped.
 *   The kernel forms the same quantity as a (sum_j P_ij (x_i - y_j) -
 *   sum_k Q_ik (x_i - x_k)) from the differences it already holds.  Each
 *   gradient is nullable on its own, has its cloud's shape AND layout and is
 *   fully overwritten; a NULL gradient pointer changes no other output by a bit.
 *   potentials_out (NULL, or [b, n + m, 2] float32): for row r of x || y the
 *   pair (F_cross, F_own) -- diagnostics and parity tests, as `price` is in
 *   pcm_emd_forward.
 *   Numerics.  float32 throughout the scans, in base 2 on the hardware
 *   v_exp_f32 / v_log_f32: a column carries h2 = fmaf(potential,
 *   fl(log2(e) / eps), fl(-log2 count)), a pair's exponent is t = fmaf(d2,
 *   fl(-log2(e) / (2 eps)), h2), and a softmin is (M + log2 sum 2^(t - M)) *
 *   fl(-eps ln 2) with M the running maximum of t, so no sum overflows or is
 *   empty for finite input.  The three per-step constants are formed in double
 *   from the schedule's double eps and rounded once.
 *   Order.  A softmin over a cloud of c points: eight partial (max, sum) pairs,
 *   partial w over the points q with (q mod 1024) div 128 == w, q ascending in
 *   groups of four (then single points up to the end of the share): the group's
 *   maximum joins the running one, the running sum is rescaled by
 *   2^(old max - new max) (skipped where it is 1 for a whole wave: the same
 *   bits), then the group's terms are added in order; the
 *   partials merge as (((p0 + p1) + p2) + ..) + p7, each merge rescaling both
 *   sides to the larger maximum.  The own cloud is scanned first.  No float
 *   atomics; the order of every sum depends on (n, m) alone: results are
 *   bit-identical from run to run, across layouts, and element bi of a batch
 *   equals the same clouds evaluated alone (b = 1) bit for bit.
 *   Non-finite input: a NaN coordinate makes loss_out of ITS element NaN and
 *   leaves the other elements' outputs untouched; that element's gradients are
 *   unspecified.  The call always returns.
 * layout1 / layout2: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, each
 *   cloud read in place and its gradient written in the same layout.
 * T + 3 launches on `stream` (the initialisation, one per schedule entry, the
 *   extrapolation, the loss finish), capturable; no host synchronisation, no
 *   allocation, no waiting between workgroups.  `diameter` is a host argument
 *   so that nothing is read back.  The workspace
 *   (pcm_sinkhorn_workspace_bytes(b, n, m) bytes, 8-byte aligned) holds two
 *   halves of (cross, own) potentials a point that the steps ping-pong
 *   between; it needs no initialisation and keeps no state.
 * Validation, before any device call: negative sizes, a layout outside {0, 1},
 *   a schedule error (PCM_ERR_INVALID_ARG, or PCM_ERR_UNSUPPORTED for too many
 *   steps); then b == 0 is a no-op (PCM_OK, also with null pointers); n == 0,
 *   m == 0, a null cloud or loss_out -> PCM_ERR_INVALID_ARG; n or m above
 *   PCM_SINKHORN_MAX_POINTS (or b beyond the grid) -> PCM_ERR_UNSUPPORTED:
 *   nothing is launched; a workspace that is NULL or too short ->
 *   PCM_ERR_WORKSPACE; a misaligned one -> PCM_ERR_INVALID_ARG.
 * pcm_sinkhorn_workspace_bytes: 0 when b, n or m is not positive.
 */
int pcm_sinkhorn_schedule(float blur, float scaling, float diameter, double *eps_out /* NULL or [capacity] */,
                          int capacity);
size_t pcm_sinkhorn_workspace_bytes(int b, int n, int m);
int pcm_sinkhorn_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                      float blur, float scaling, float diameter, float *loss_out /* [b] */,
                      float *gradxyz1 /* NULL or xyz1's shape and layout */,
                      float *gradxyz2 /* NULL or xyz2's shape and layout */,
                      float *potentials_out /* NULL or [b, n + m, 2] */, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ---------------------------------------------------------------------- */
/* Sliced Wasserstein distance (p = 2, uniform masses)                     */
/* ---------------------------------------------------------------------- */

/* Largest cloud (points per batch element) and most directions
 * pcm_sliced_wasserstein_loss takes (else PCM_ERR_UNSUPPORTED). */
#define PCM_SLICED_MAX_POINTS 16384
#define PCM_SLICED_MAX_DIRS   1024
/* Switch-over: with both clouds at or below it one workgroup projects, sorts
 * and matches an (element, direction) out of LDS in one launch; above it each
 * cloud is sorted by a workgroup of its own and the sorted (key, index)
 * composites pass through the workspace.  Results do not depend on the path. */
#define PCM_SLICED_FUSED_MAX_POINTS 2048

/*
 * Sliced 2-Wasserstein distance of two unweighted clouds (extension; Nguyen et
 * al., "Point-set distances for learning representations of 3D point clouds"):
 * the mean over l directions of the exact 1-D transport cost between the
 * clouds' projections.  This text is the contract.
 *
 * Per batch element, cloud x = xyz1[bi] has n points of mass 1/n and cloud
 *   y = xyz2[bi] has m points of mass 1/m.  The l directions theta = dirs[li]
 *   (device memory, [l, 3] float32, contiguous) are taken as given -- the
 *   library does not normalise them -- and are shared by the batch.
 * Projection, pinned: p = fmaf(tz, z, fmaf(ty, y, tx * x)) in float32, explicit
 *   fused steps and no other contraction.
 * Order, pinned and total: the key of p is u = bits(p), then u ^ 0xFFFFFFFF if
 *   the sign bit is set, else u | 0x80000000, compared as unsigned: -0.0 sorts
 *   before +0.0 and NaNs sort by their bits at the two ends.  Equal keys are
 *   ordered by ascending point index.  order1_out[bi, li, r] (NULL or
 *   [b, l, n] int32) is the index of the point of rank r; order2_out the same
 *   for y.  They EQUAL np.lexsort((index, key)).
 * Matching, exact 1-D transport of uniform masses: rank r of x covers the
 *   quantile interval [r/n, (r+1)/n) and overlaps ranks s of y from
 *   (r m) div n to ceil((r+1) m / n) - 1 with the integer weight
 *   w_rs = min((r+1) m, (s+1) n) - max(r m, s n).  With a, b the sorted
 *   projections,
 *     slice = (1 / (n m)) sum_r sum_s w_rs (a_r - b_s)^2
 *   (for n = m: (1/n) sum_r (a_r - b_r)^2);  slices_out[bi, li] (NULL or
 *   [b, l]) = slice rounded once;  loss_out[bi] = (1/l) sum_li slice,
 *   accumulated in double and rounded once.
 * Gradients of loss_out[bi] with unit upstream gradient:
 *     gradxyz1[i] = (1/l) sum_li theta_li (2 / (n m)) sum_s w_rs (a_r - b_s),
 *   r the rank of i in slice li;  gradxyz2[j] the same with the roles swapped
 *   and the sign flipped ((2 / (n m)) sum_r w_rs (b_s - a_r)).  In exact
 *   arithmetic sum_i gradxyz1 + sum_j gradxyz2 = 0.  Each gradient is nullable
 *   on its own, has its cloud's shape AND layout and is fully overwritten; a
 *   NULL pointer for any optional output changes no other output by a bit.
 * Numerics and order of the sums.  a_r - b_s, the products with w_rs and all
 *   sums are in double.  A slice: a thread adds its ranks r ascending and for
 *   each the ranks s ascending (up to the fused size the thread of cloud x's
 *   E = 4 or 16 consecutive ranks, above it ranks t, t + 256, .. of 256
 *   threads); every wave adds its 64 threads by the six DPP steps, the waves'
 *   sums are added ascending; the total is divided by (double) n m.  A point's
 *   coefficient c = fl32((2 / (n m)) sum_s w_rs (a_r - b_s)) is rounded to
 *   float32 once; its gradient is four partial sums of (double) theta_li *
 *   (double) c, partial w over li in [w q, min(l, (w + 1) q)), q = ceil(l / 4),
 *   ascending, added in order, divided by l, rounded once.  loss_out: thread t
 *   of 256 adds the slices t, t + 256, .., then waves and workgroup as above,
 *   divided by l.
 *   No float atomics, no waiting between workgroups; the order of every sum
 *   depends on (n, m, l) alone: results are bit-identical from run to run,
 *   across layouts, and element bi of a batch equals the same clouds evaluated
 *   alone (b = 1) bit for bit.
 * Non-finite input: the order stays total, so the call always returns and
 *   never indexes out of range.  An element with a NaN coordinate gets a NaN
 *   loss_out; its order*_out still equal the lexsort of the keys of the
 *   projections the device's fused multiply-adds give (a NaN operand comes
 *   through with its sign and payload, quieted); its gradients are
 *   unspecified.  The other elements' outputs are untouched, bit for bit.
 * layout1 / layout2: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, each
 *   cloud read in place and its gradient written in the same layout.
 * Launches on `stream`: two (sort-and-match, finish) when both clouds are at
 *   most PCM_SLICED_FUSED_MAX_POINTS, else three (sort, match, finish) -- a
 *   fixed function of the shape; capturable; no host synchronisation, no
 *   allocation.  The workspace (pcm_sliced_workspace_bytes(b, n, m, l) bytes,
 *   8-byte aligned: b l doubles for the slices, b l (n + m) floats for the
 *   points' coefficients by original index and, above the fused size,
 *   b l (n + m) 8-byte sorted composites) needs no initialisation and keeps no
 *   state.
 * Validation, before any device call: negative sizes, a layout outside {0, 1},
 *   l <= 0 -> PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK, also with
 *   null pointers); n == 0, m == 0, a null cloud, dirs or loss_out ->
 *   PCM_ERR_INVALID_ARG; n or m above PCM_SLICED_MAX_POINTS, l above
 *   PCM_SLICED_MAX_DIRS (or b l beyond the grid) -> PCM_ERR_UNSUPPORTED; a
 *   workspace that is NULL or too short -> PCM_ERR_WORKSPACE; a misaligned one
 *   -> PCM_ERR_INVALID_ARG.
 * pcm_sliced_workspace_bytes: 0 when b, n, m or l is not positive.
 */
size_t pcm_sliced_workspace_bytes(int b, int n, int m, int l);
int pcm_sliced_wasserstein_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                                const float *dirs /* device, [l, 3] */, int l, float *loss_out /* [b] */,
                                float *slices_out /* NULL or [b, l] */,
                                float *gradxyz1 /* NULL or xyz1's shape and layout */,
                                float *gradxyz2 /* NULL or xyz2's shape and layout */,
                                int32_t *order1_out /* NULL or [b, l, n] */,
                                int32_t *order2_out /* NULL or [b, l, m] */, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---------------------------------------------------------------------- */
/* Density-aware Chamfer distance                                          */
/* ---------------------------------------------------------------------- */

/* Largest cloud (points per batch element) pcm_dcd_loss takes (else
 * PCM_ERR_UNSUPPORTED): both clouds' hit counts of one element live in one
 * workgroup's LDS, 2 x 16384 x 4 bytes. */
#define PCM_DCD_MAX_POINTS 16384

/*
 * Density-aware Chamfer distance (extension; Wu et al., "Density-aware Chamfer
 * Distance as a Comprehensive Metric for Point Cloud Completion", NeurIPS
 * 2021).  The formula is stated from the published source, not verified
 * against it (the package is not installed where this was written); this text
 * is the contract.
 *
 * Per batch element, for xyz1 [b, n, 3] and xyz2 [b, m, 3]:
 *   d1, i1, d2, i2 are exactly what pcm_chamfer_forward returns for the clouds
 *   (squared distances in the pinned order, lowest-index argmins).
 *   Hit counts: count2[k] = #{j : i1[j] = k} (how many points of xyz1 have
 *   xyz2[k] as their neighbour), count1[j] = #{k : i2[k] = j}.
 *   count1_out (NULL or [b, n] int32) and count2_out (NULL or [b, m] int32)
 *   EQUAL np.bincount of the argmins.
 *   Direction 1 has the n points of xyz1 as queries into the m targets of
 *   xyz2, direction 2 the reverse.  The ratio of a direction with Q queries
 *   and T targets is r = (float)Q / (float)T, or with non_reg != 0
 *   r = max(1.f, (float)Q / (float)T).
 *   term(q) = 1 - exp(-alpha d(q)) r / (c(idx(q))^lambda + 1e-6), c the TARGET
 *   cloud's counts (direction 1: count2[i1[j]]; a query's own target has
 *   c >= 1);
 *   loss_out[bi] = (mean_j term1(j) + mean_k term2(k)) / 2.
 *   cd_out (NULL or [b, 2]): cd_out[bi, 0] = (mean_j sqrt(d1) + mean_k sqrt(d2)) / 2
 *   ("cd_p"), cd_out[bi, 1] = mean_j d1 + mean_k d2 ("cd_t").
 * float32 evaluation order of a term, pinned (every operation rounded once, no
 * contraction):
 *     a = alpha * d;  e = expf(-a)   (the device library's expf, not the
 *                                     hardware's approximate exponential);
 *     p = c (the count converted, exact) when lambda == 1, 1.f when
 *         lambda == 0, else powf((float)c, lambda): lambda == 1 never calls powf;
 *     w = (1.f / (p + 1e-6f)) * r;   r multiplies the reciprocal, not e;
 *     g = e * w;  term = 1.f - g;
 *     graddist = (alpha * g) / (float)(2 Q).
 * Sums: a thread adds the terms of queries t, t + 1024, ... (a workgroup of
 *   1024 threads) ascending in double, sqrtf(d) and d likewise; a wave adds
 *   its 64 lanes by the six DPP steps, the waves' sums are added ascending (cd_t
 *   is the plain sum of the two directions' means); each sum is divided
 *   by its query count in double, the two directions are added, halved (loss,
 *   cd_p) and rounded to float32 once.  One workgroup holds an element, so no
 *   sum crosses workgroups.
 * Gradients.  The counts carry no gradient (the published code detaches them):
 *   graddist1[j] = alpha r1 exp(-alpha d1[j]) / (count2[i1[j]]^lambda + 1e-6) / (2 n),
 *   graddist2[k] the same with r2, count1[i2[k]] and 2 m, both in the order
 *   pinned above.  graddist1_out (NULL or [b, n]) and graddist2_out (NULL or
 *   [b, m]) receive them; gradxyz1 / gradxyz2 (each NULL or its cloud's shape
 *   AND layout) are what pcm_chamfer_backward_strided gives for these
 *   graddists, bit for bit -- the gradient of loss_out[bi] with unit upstream
 *   gradient.  A NULL pointer for any optional output changes no other output
 *   by a bit; every output element is fully overwritten.
 * Non-finite input.  A query whose distance is +inf has e = 0: term 1,
 *   graddist 0.  A NaN distance gives that element a NaN loss; argmins stay in
 *   range (pcm_chamfer_forward's tile rule), the counts are still their
 *   bincount, and the other elements' outputs are untouched, bit for bit.
 * Launches on `stream`: the forward exactly as pcm_chamfer_forward_ws picks it
 *   for row clouds (the grid forward when both clouds hold >= 4096 points and
 *   b n m >= 2^28, else the dense kernels) or pcm_chamfer_forward_layout when
 *   a cloud is in channel planes; ONE launch for counts, terms, graddists and
 *   sums (one workgroup an element; integer LDS atomics only, whose sums do not
 *   depend on their order); pcm_chamfer_backward_strided only when a gradient
 *   is asked for.  Deterministic: no float atomics, no waiting between
 *   workgroups; element bi of a batch equals the same clouds evaluated alone.
 *   Capturable: no host synchronisation, no allocation, no state.
 *   The workspace (pcm_dcd_workspace_bytes(b, n, m) bytes, 16-byte aligned:
 *   the grid forward's bytes when that path is taken, d and i of both
 *   directions, the graddists and a gradient each for the pointers that may be
 *   NULL) needs no initialisation.
 * layout1 / layout2: 0 = [b, n, 3] rows, 1 = [b, 3, n] channel planes, each
 *   cloud read in place and its gradient written in the same layout.
 * Validation, before any device call: negative sizes, a layout outside {0, 1},
 *   alpha not finite or <= 0, n_lambda not finite or < 0 ->
 *   PCM_ERR_INVALID_ARG; then b == 0 is a no-op (PCM_OK, also with null
 *   pointers); n == 0, m == 0, a null cloud or loss_out -> PCM_ERR_INVALID_ARG;
 *   n or m above PCM_DCD_MAX_POINTS -> PCM_ERR_UNSUPPORTED; a workspace that is
 *   NULL or too short -> PCM_ERR_WORKSPACE; a misaligned one ->
 *   PCM_ERR_INVALID_ARG.
 * pcm_dcd_workspace_bytes: 0 when b, n or m is not positive.
 */
size_t pcm_dcd_workspace_bytes(int b, int n, int m);
int pcm_dcd_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2, float alpha,
                 float n_lambda, int non_reg, float *loss_out /* [b] */, float *cd_out /* NULL or [b, 2] */,
                 float *gradxyz1 /* NULL or xyz1's shape and layout */,
                 float *gradxyz2 /* NULL or xyz2's shape and layout */, int32_t *count1_out /* NULL or [b, n] */,
                 int32_t *count2_out /* NULL or [b, m] */, float *graddist1_out /* NULL or [b, n] */,
                 float *graddist2_out /* NULL or [b, m] */, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* EMD (auction approximation)                                           */
/* ---------------------------------------------------------------------- */

/* Device workspace (bytes) pcm_emd_forward needs for a [b, n] problem. */
size_t pcm_emd_workspace_bytes(int b, int n);

/*
 * Auction-algorithm approximate EMD (emd_cuda.cu:23-282), deterministic:
 * bidders tying within the reference's 1e-6 window resolve to the lowest
 * point index (the reference lets a racing writer win).  A bidder whose best
 * value is attained by several objects bids on the one the reference's Bid
 * finds first (emd_cuda.cu:108-110, 136-139, 165-173: the lowest (thread
 * range, tile, index); the lowest index whenever n <= 2048).  Requirements as the
 * reference (emd_cuda.cu:236-249): both clouds [b, n, 3] (same n), b <= 512,
 * n % 1024 == 0 (any such n up to 2^21, else PCM_ERR_UNSUPPORTED); iters >= 1.  Outputs dist [b, n] (squared
 * distance to the assigned point) and assignment [b, n] (int32; not
 * guaranteed a bijection).  `workspace` must hold pcm_emd_workspace_bytes(b, n)
 * bytes; its content on entry is irrelevant; calls that share a workspace must
 * be stream-ordered.  `price` may be NULL; otherwise it receives the final
 * object prices [b, n] (diagnostics / parity tests).
 * Input contract: any finite coordinates for which every pairwise squared
 * distance is finite in float32 (not only the reference's [0, 1]); eps >= 0,
 * which the proofs behind the kernel's pruning need (prices must never fall).
 * There assignment, dist and price equal the CPU oracle's bit for bit
 * (tests/test_emd_stress_gpu.py: scales 1e-4 to 1e5, offsets, planar,
 * collinear, lattice, coincident, collapsed and bimodal clouds).  Non-finite
 * coordinates, or magnitudes at which a squared distance overflows to
 * infinity (coordinates apart by more than about 1e19), are outside it and
 * untested.
 */
int pcm_emd_forward(const float *xyz1, const float *xyz2, int b, int n, float eps, int iters,
                    float *dist, int32_t *assignment, float *price,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Status of the last pcm_emd_forward on `workspace`; synchronises `stream`
 * (it reads device memory).  The auction's helper workgroups take heavy
 * iterations' full scans; a helper job whose result does not arrive within a
 * bounded wait (helpers not resident) is scanned by the batch element's own
 * workgroup instead, and no further jobs are posted in that call, so the
 * outputs never depend on residency: PCM_OK unless reading the workspace fails.
 */
int pcm_emd_workspace_status(const void *workspace, size_t workspace_bytes, int b, int n, void *stream);

/*
 * EMD backward (emd_cuda.cu:284-316): gradxyz1[j] = 2*graddist[j]*(xyz1[j] - xyz2[a[j]]).
 * The reference returns no gradient for xyz2 (emd_module.py:84-87).
 * gradxyz1 is fully overwritten.
 */
int pcm_emd_backward(const float *xyz1, const float *xyz2, int b, int n,
                     const float *graddist, const int32_t *assignment,
                     float *gradxyz1, void *stream);

/* ---------------------------------------------------------------------- */
/* ICP alignment (evaluation caller)           */
/* ---------------------------------------------------------------------- */

/*
 * Batched icp (utils/icp.py:68-118) for b independent pairs, as testnet.py:63
 * calls it per sample: A [b,n,3] (source) and B [b,n,3] (destination), float64
 * (the reference copies its inputs into float64 arrays, icp.py:89-92).
 * init_pose: NULL or [b,4,4] float64 row-major (icp.py:95-96).  Per pair:
 *   repeat: nearest neighbour of every src point in B (float64 Euclidean,
 *           lowest index on exact ties), best-fit rigid transform, src = T src,
 *   until |prev - mean(distances)| < tolerance or max_iterations passes;
 *   T_out [b,4,4] = best_fit_transform(A, src) (row-major, float64),
 *   distances [b,n] = the last pass's Euclidean NN distances (float64),
 *   iterations [b] = the reference's returned loop index i.
 * A prep launch writes B's float32 screening rows into `workspace`
 * (pcm_icp_workspace_bytes(b, n) bytes, content on entry irrelevant); then the
 * whole loop runs in one launch (each pair's source points split over K <= 16
 * workgroups, K b <= the device's CU count, so a batch of one pair still fills
 * 16 CUs).  Needs
 * max_iterations >= 1 (the reference fails otherwise), 0 < n <= 16384
 * (else PCM_ERR_UNSUPPORTED); a batch goes out in launches of at most one
 * workgroup per compute unit (K workgroups per pair, so a pair's slices are
 * resident together).  Non-finite inputs give unspecified values (the
 * reference's sklearn rejects them; the Python wrapper does the same).
 */
size_t pcm_icp_workspace_bytes(int b, int m);
int pcm_icp(const double *A, const double *B, int b, int n, const double *init_pose, int max_iterations,
            double tolerance, double *T_out, double *distances, int32_t *iterations, void *workspace,
            size_t workspace_bytes, void *stream);

/*
 * Device-side failure of the last pcm_icp on `workspace`: a pair's source
 * points are split over up to 16 workgroups that meet once per pass; a wait
 * that timed out (workgroups that could not all be resident) sets an error
 * word: PCM_ERR_LAUNCH, and the transforms are NaN.  Synchronises `stream`.
 */
int pcm_icp_workspace_status(const void *workspace, size_t workspace_bytes, int b, int n, void *stream);

/*
 * nearest_neighbor (utils/icp.py:49-65, sklearn NearestNeighbors(n_neighbors=1)):
 * for each src[b,i] (n points) the nearest dst[b,k] (m points), float64:
 *   distances[b,i] = sqrt((dx*dx + dy*dy) + dz*dz), indices[b,i] = k (int32,
 *   lowest index on exact ties).  `workspace`: pcm_icp_workspace_bytes(b, m)
 *   bytes (content on entry irrelevant).  Any m >= 1.
 */
int pcm_nearest_neighbor(const double *src, const double *dst, int b, int n, int m, double *distances,
                         int32_t *indices, void *workspace, size_t workspace_bytes, void *stream);

/*
 * best_fit_transform (utils/icp.py:4-46) for b pairs of corresponding clouds
 * A, B [b,n,3] float64: T_out [b,4,4] maps A onto B (proper rotation, the
 * reflection case fixed as icp.py:34-36 does).
 */
int pcm_best_fit_transform(const double *A, const double *B, int b, int n, double *T_out, void *stream);

/* ---------------------------------------------------------------------- */
/* Ground-truth cloud ingestion (host only)    */
/* ---------------------------------------------------------------------- */

/*
 * The reference loads each sample's ground truth with
 * np.load(data_dir_pcl + model + '/pointcloud_<numpoints>.npy')
 * (utils/datasets_old.py:37-38) and copies the collated batch to the GPU.
 * These read .npy files (format 1.0-3.0; '<f4' '>f4' '<f8' '>f8'; C or
 * Fortran order; shape (npoints, 3)) on the HOST:
 *   pcm_npy_cloud_points: *npoints = the file's row count;
 *   pcm_npy_load_clouds:  out[count, npoints, 3] float32 (host memory, e.g. a
 *     pinned staging buffer) = np.load(paths[i]).astype(float32), read by
 *     nthreads threads.  On failure returns PCM_ERR_IO / PCM_ERR_FORMAT /
 *     PCM_ERR_INVALID_ARG for the lowest failing index, stored in
 *     *failed_index (-1 on success); other slots may be partly written.
 */
int pcm_npy_cloud_points(const char *path, int *npoints);
int pcm_npy_load_clouds(const char *const *paths, int count, int npoints, float *out, int nthreads,
                        int *failed_index);

#ifdef __cplusplus
}
#endif

#endif /* PCM_H_ */
