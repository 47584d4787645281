/*
 * ref_entry.cpp -- C entry points over the reference's four host functions, as
 * compiled for the CPU by oracle/ref_build.py (test infrastructure only).
 *
 * Every buffer, the auction's state included, belongs to the caller, which
 * initialises it the way the reference's Python wrappers do.  Nothing here
 * computes anything.
 */
#include "cuda_on_cpu.h"

/* defined by the reference's chamfer3D.cu and emd_cuda.cu (argument order as
 * its Python wrappers pass them: dist_chamfer_3D.py:52,68, emd_module.py:56-86) */
using at::Tensor;
int chamfer_cuda_forward(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor);
int chamfer_cuda_backward(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor);
int emd_cuda_forward(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor,
                     Tensor, Tensor, Tensor, float, int);
int emd_cuda_backward(Tensor, Tensor, Tensor, Tensor, Tensor);

static at::Tensor tensor(const void *p, int64_t d0, int64_t d1 = 1, int64_t d2 = 1) {
    return at::Tensor{const_cast<void *>(p), {d0, d1, d2}};
}

extern "C" {

int pcm_ref_chamfer_forward(const float *xyz1, const float *xyz2, int b, int n, int m, float *dist1,
                            float *dist2, int32_t *idx1, int32_t *idx2) {
    return chamfer_cuda_forward(tensor(xyz1, b, n, 3), tensor(xyz2, b, m, 3), tensor(dist1, b, n),
                                tensor(dist2, b, m), tensor(idx1, b, n), tensor(idx2, b, m));
}

int pcm_ref_chamfer_backward(const float *xyz1, const float *xyz2, int b, int n, int m,
                             float *gradxyz1, float *gradxyz2, const float *graddist1,
                             const float *graddist2, const int32_t *idx1, const int32_t *idx2) {
    return chamfer_cuda_backward(tensor(xyz1, b, n, 3), tensor(xyz2, b, m, 3),
                                 tensor(gradxyz1, b, n, 3), tensor(gradxyz2, b, m, 3),
                                 tensor(graddist1, b, n), tensor(graddist2, b, m), tensor(idx1, b, n),
                                 tensor(idx2, b, m));
}

int pcm_ref_emd_forward(const float *xyz1, const float *xyz2, int b, int n, float eps, int iters,
                        float *dist, int32_t *assignment, float *price, int32_t *assignment_inv,
                        int32_t *bid, float *bid_increments, float *max_increments,
                        int32_t *unass_idx, int32_t *unass_cnt, int32_t *unass_cnt_sum,
                        int32_t *cnt_tmp, int32_t *max_idx) {
    return emd_cuda_forward(tensor(xyz1, b, n, 3), tensor(xyz2, b, n, 3), tensor(dist, b, n),
                            tensor(assignment, b, n), tensor(price, b, n), tensor(assignment_inv, b, n),
                            tensor(bid, b, n), tensor(bid_increments, b, n), tensor(max_increments, b, n),
                            tensor(unass_idx, (int64_t)b * n), tensor(unass_cnt, 512),
                            tensor(unass_cnt_sum, 512), tensor(cnt_tmp, 512),
                            tensor(max_idx, (int64_t)b * n), eps, iters);
}

int pcm_ref_emd_backward(const float *xyz1, const float *xyz2, int b, int n, float *gradxyz,
                         const float *graddist, const int32_t *assignment) {
    return emd_cuda_backward(tensor(xyz1, b, n, 3), tensor(xyz2, b, n, 3), tensor(gradxyz, b, n, 3),
                             tensor(graddist, b, n), tensor(assignment, b, n));
}

}  /* extern "C" */
