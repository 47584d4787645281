// dcd.hip -- density-aware Chamfer distance (Wu et al., NeurIPS 2021) for MI355X
// (gfx950, CDNA4): the step between the Chamfer forward (distances and
// lowest-index argmins, csrc/chamfer*.hip, called through its host entries and
// not copied) and the Chamfer backward (a deterministic scatter of per-point
// upstream weights).  include/pcm.h has the contract; DESIGN.md section 3.19
// has the rationale and the numbers.
//
// dcd_terms, one launch, one workgroup a batch element:
//   1. both hit-count histograms of the element in LDS (count2[k] = queries of
//      cloud 1 whose argmin is k, count1[j] the reverse) by integer LDS atomics
//      without return -- integer sums do not depend on their order, so the
//      counts are deterministic;
//   2. every query looks up its target's count and evaluates the pinned float32
//      term and its graddist;
//   3. the terms, sqrtf(d) and d are added in double: a thread its queries
//      ascending, a wave by the six DPP steps, the waves ascending;
//   4. the optional count outputs are copied out of LDS.
// The LDS request is 4 (n + m) bytes plus the waves' partial sums, so clouds of
// 1024 points leave room for two workgroups of 1024 threads a compute unit and
// only the largest (2 x 16384 counts, 128 KiB) take a unit each.
// Measured alternatives (profiles/dcd/terms_split_threads.txt, a timing-only
// build): 1024 threads beat 256 and 512 at every size (B=32, N=M=1024: 5.2 us
// against 10.5 and 5.7; the launch is a chain of dependent round trips -- argmin
// load, LDS atomic, barrier, count read, expf, sums -- and more waves hide more
// of it); unrolling the loops by four changes nothing.  A split of one element
// over S workgroups, each rebuilding both histograms and owning a slice of the
// queries, gains nothing at 1024 points (5.2 us at S = 4 too), 6.6 -> 5.3 us at
// 2048 and 27.5 -> 16.6 us at 16384 points and S = 32 -- before the further
// launch (or the state in the workspace) that the fixed-order sum across
// workgroups would need, about 5 us, and out of a call of 90 us.  One histogram
// pass a workgroup stops paying there; the simple form stays.
#include "pcm_common.h"

namespace {

constexpr int kDcdMaxN = PCM_DCD_MAX_POINTS;
constexpr int kDcdThreads = 1024;
constexpr int kDcdMaxWaves = kDcdThreads / 64;
constexpr int kDcdSums = 6;             // term, sqrt(d), d of each direction
constexpr size_t kDcdRedBytes = (size_t)kDcdMaxWaves * kDcdSums * sizeof(double);
static_assert(kDcdRedBytes % 16 == 0, "the histograms start 16-byte aligned");
static_assert(kDcdRedBytes + 2 * (size_t)kDcdMaxN * sizeof(int) <= 160 * 1024, "both histograms fit one unit's LDS");

struct DcdDir {
    const float *dist;  // [cnt] the element's squared distances
    const int *idx;     // [cnt] argmins into the other cloud
    float *graddist;    // [cnt]
    int cnt, targets;   // queries and targets
    float ratio;        // r
};

// the pinned term of one query: g = e * w, term = 1 - g, graddist = (alpha * g) / (2 Q)
__device__ __forceinline__ float dcd_g(float d, int c, float alpha, float lambda, float ratio) {
    const float a = alpha * d;
    const float e = expf(-a);
    const float cf = (float)c;
    const float p = lambda == 1.f ? cf : lambda == 0.f ? 1.f : powf(cf, lambda);
    const float w = (1.f / (p + 1e-6f)) * ratio;
    return e * w;
}

// one direction: graddists written, the thread's three sums returned
__device__ __forceinline__ void dcd_direction(const DcdDir D, const int *hist, float alpha, float lambda, double &st,
                                              double &ss, double &sd) {
    const float two_q = (float)(2 * D.cnt);
    for (int q = threadIdx.x; q < D.cnt; q += blockDim.x) {
        const float d = D.dist[q];
        const int k = D.idx[q];
        // an argmin is in range by the forward's contract; an index that were not must not read past the counts
        const int c = (unsigned)k < (unsigned)D.targets ? hist[k] : 1;
        const float g = dcd_g(d, c, alpha, lambda, D.ratio);
        D.graddist[q] = (alpha * g) / two_q;
        st += (double)(1.f - g);
        ss += (double)sqrtf(d);
        sd += (double)d;
    }
}

__global__ __launch_bounds__(kDcdThreads) void dcd_terms(
    const float *__restrict__ dist1, const float *__restrict__ dist2, const int *__restrict__ idx1,
    const int *__restrict__ idx2, int n, int m, float alpha, float lambda, float ratio1, float ratio2,
    float *__restrict__ graddist1, float *__restrict__ graddist2, int *__restrict__ count1_out,
    int *__restrict__ count2_out, float *__restrict__ loss_out, float *__restrict__ cd_out) {
    extern __shared__ __attribute__((aligned(16))) char dcd_lds[];
    double *sRed = (double *)dcd_lds;               // [waves][kDcdSums]
    int *hist1 = (int *)(dcd_lds + kDcdRedBytes);   // [n] hits on cloud 1's points
    int *hist2 = hist1 + n;                         // [m] hits on cloud 2's points
    const int bi = blockIdx.x, T = blockDim.x;
    const size_t o1 = (size_t)bi * n, o2 = (size_t)bi * m;

    for (int k = threadIdx.x; k < n + m; k += T) hist1[k] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += T) {
        const int k = idx1[o1 + j];
        if ((unsigned)k < (unsigned)m) atomicAdd(&hist2[k], 1);
    }
    for (int k = threadIdx.x; k < m; k += T) {
        const int j = idx2[o2 + k];
        if ((unsigned)j < (unsigned)n) atomicAdd(&hist1[j], 1);
    }
    __syncthreads();

    double s[kDcdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    dcd_direction(DcdDir{dist1 + o1, idx1 + o1, graddist1 + o1, n, m, ratio1}, hist2, alpha, lambda, s[0], s[1], s[2]);
    dcd_direction(DcdDir{dist2 + o2, idx2 + o2, graddist2 + o2, m, n, ratio2}, hist1, alpha, lambda, s[3], s[4], s[5]);
    if (count1_out)
        for (int j = threadIdx.x; j < n; j += T) count1_out[o1 + j] = hist1[j];
    if (count2_out)
        for (int k = threadIdx.x; k < m; k += T) count2_out[o2 + k] = hist2[k];

    const int wave = threadIdx.x >> 6, waves = T >> 6;
#pragma unroll
    for (int q = 0; q < kDcdSums; ++q) {
        const double wsum = pcm_wave_sum_f64(s[q]);
        if ((threadIdx.x & 63) == 0) sRed[wave * kDcdSums + q] = wsum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[kDcdSums];
    for (int q = 0; q < kDcdSums; ++q) {
        double acc = 0.0;
        for (int w = 0; w < waves; ++w) acc += sRed[w * kDcdSums + q];  // the waves ascending
        tot[q] = acc / (double)(q < 3 ? n : m);
    }
    loss_out[bi] = (float)((tot[0] + tot[3]) * 0.5);
    if (cd_out) {
        cd_out[2 * (size_t)bi] = (float)((tot[1] + tot[4]) * 0.5);
        cd_out[2 * (size_t)bi + 1] = (float)(tot[2] + tot[5]);
    }
}

inline size_t dcd_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: the grid forward's bytes (0 for a dense problem) rounded up to 256, then [b n] and [b m] of
// dist, idx and graddist, then a gradient of each cloud's size for a gradient pointer that is NULL while the
// other is not (the backward writes both)
struct DcdLayout {
    size_t fwd, dist1, dist2, idx1, idx2, gd1, gd2, grad1, grad2, total;
};
inline DcdLayout dcd_layout(int b, int n, int m) {
    DcdLayout L;
    const size_t p1 = dcd_align256((size_t)b * n * 4), p2 = dcd_align256((size_t)b * m * 4);
    L.fwd = dcd_align256(pcm_chamfer_forward_ws_bytes(b, n, m));
    L.dist1 = L.fwd;
    L.dist2 = L.dist1 + p1;
    L.idx1 = L.dist2 + p2;
    L.idx2 = L.idx1 + p1;
    L.gd1 = L.idx2 + p2;
    L.gd2 = L.gd1 + p1;
    L.grad1 = L.gd2 + p2;
    L.grad2 = L.grad1 + 3 * p1;
    L.total = L.grad2 + 3 * p2;
    return L;
}

}  // namespace

extern "C" size_t pcm_dcd_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return dcd_layout(b, n, m).total;
}

extern "C" int pcm_dcd_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                            float alpha, float n_lambda, int non_reg, float *loss_out, float *cd_out, float *gradxyz1,
                            float *gradxyz2, int32_t *count1_out, int32_t *count2_out, float *graddist1_out,
                            float *graddist2_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 0 || n < 0 || m < 0) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    if (!(alpha > 0.f) || !__builtin_isfinite(alpha) || !(n_lambda >= 0.f) || !__builtin_isfinite(n_lambda)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0 || !xyz1 || !xyz2 || !loss_out) return PCM_ERR_INVALID_ARG;
    if (n > kDcdMaxN || m > kDcdMaxN) return PCM_ERR_UNSUPPORTED;
    const DcdLayout L = dcd_layout(b, n, m);
    if (!workspace || workspace_bytes < L.total) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return PCM_ERR_INVALID_ARG;

    char *base = (char *)workspace;
    float *dist1 = (float *)(base + L.dist1), *dist2 = (float *)(base + L.dist2);
    int32_t *idx1 = (int32_t *)(base + L.idx1), *idx2 = (int32_t *)(base + L.idx2);
    float *gd1 = graddist1_out ? graddist1_out : (float *)(base + L.gd1);
    float *gd2 = graddist2_out ? graddist2_out : (float *)(base + L.gd2);

    // 1. the forward, as pcm_hip.chamfer_forward picks it for rows; channel planes are read in place
    const int fwd = (layout1 == 0 && layout2 == 0)
                        ? pcm_chamfer_forward_ws(xyz1, xyz2, b, n, m, dist1, dist2, idx1, idx2, base, L.fwd, stream)
                        : pcm_chamfer_forward_layout(xyz1, xyz2, b, n, m, layout1, layout2, dist1, dist2, idx1, idx2,
                                                     stream);
    if (fwd != PCM_OK) return fwd;

    // 2. counts, terms, graddists and sums
    float r1 = (float)n / (float)m, r2 = (float)m / (float)n;
    if (non_reg) {
        r1 = r1 > 1.f ? r1 : 1.f;
        r2 = r2 > 1.f ? r2 : 1.f;
    }
    const size_t lds = kDcdRedBytes + ((size_t)n + (size_t)m) * sizeof(int);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)dcd_terms, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
        return PCM_ERR_LAUNCH;
    hipLaunchKernelGGL(dcd_terms, dim3((unsigned)b), dim3(kDcdThreads), lds, (hipStream_t)stream, (const float *)dist1,
                       (const float *)dist2, (const int *)idx1, (const int *)idx2, n, m, alpha, n_lambda, r1, r2, gd1,
                       gd2, count1_out, count2_out, loss_out, cd_out);
    const int st = pcm_launch_status();
    if (st != PCM_OK || (!gradxyz1 && !gradxyz2)) return st;

    // 3. the existing deterministic scatter on the graddists
    float *g1 = gradxyz1 ? gradxyz1 : (float *)(base + L.grad1);
    float *g2 = gradxyz2 ? gradxyz2 : (float *)(base + L.grad2);
    return pcm_chamfer_backward_strided(xyz1, xyz2, b, n, m, layout1, layout2, gd1, n, 1, gd2, m, 1, idx1, idx2, g1,
                                        g2, stream);
}
